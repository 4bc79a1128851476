"""The level table as a field of the force kernel's argument block (csrc/mtp_device.hpp, level_rows), without a GPU:
what the host-only planner reports equals the padded level table the blob carries -- recomputed here from the file's
alpha_index_times with the schedule's rules (csrc/mtp_potential.cpp: find_leaves, build_levels, pad_levels), sharing
no code with the library -- for every committed potential; a re-fit keeps the shape, a table whose rows sit in other
levels does not."""
import os
import re

import pytest

from _mutate import mutate_mtp
from lammps_mtp_kokkos_amd import capi, mtpgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
CUS, INUM, MAXN = 256, 65536, 94
ARR_LEN = 14   # MTP_PSTRIDE + 2
COMMITTED = [("W_L8.mtp", False), ("W_L16.mtp", False), ("W_L16_nbh.almtp", True), ("WRe_L10_cfg.almtp", True),
             ("WRe_L20.mtp", False)]


def _ints(txt, key):
    m = re.search(r"^\s*%s\s*=\s*(.*)$" % key, txt, flags=re.M)
    return [int(v) for v in re.findall(r"-?\d+", m.group(1))]


def level_table(path):
    """padded row offsets of the dependency levels and of the leaf block: [0, end of level 1, ..., end of the leaf rows]"""
    raw = open(path, "rb").read()
    cut = raw.find(b"#MVS_v1.1")
    txt = (raw if cut < 0 else raw[:cut]).decode()
    A = _ints(txt, "alpha_moments_count")[0]
    B = _ints(txt, "alpha_index_basic_count")[0]
    t = _ints(txt, "alpha_index_times")
    rows = [tuple(t[4 * k:4 * k + 4]) for k in range(len(t) // 4)]
    assert len(rows) == _ints(txt, "alpha_index_times_count")[0]
    is_factor, is_target, last_write = [False] * A, [False] * A, [-1] * A
    for k, (a0, a1, _, a3) in enumerate(rows):
        is_factor[a0] = is_factor[a1] = True
        is_target[a3] = True
        last_write[a3] = k
    # leaf: a product that no row reads, unless one of its factors is written again later in file order
    leaf = [m >= B and is_target[m] and not is_factor[m] for m in range(A)]
    for k, (a0, a1, _, a3) in enumerate(rows):
        if leaf[a3] and (last_write[a0] > k or last_write[a1] > k):
            leaf[a3] = False
    wlevel, rlevel, count = [0] * A, [0] * A, {}
    nlev = 0
    for a0, a1, _, a3 in rows:
        if leaf[a3]:
            continue
        lv = max(wlevel[a0], wlevel[a1], rlevel[a3]) + 1
        wlevel[a3] = max(wlevel[a3], lv)
        rlevel[a0] = max(rlevel[a0], lv)
        rlevel[a1] = max(rlevel[a1], lv)
        count[lv] = count.get(lv, 0) + 1
        nlev = max(nlev, lv)
    count[nlev + 1] = sum(1 for r in rows if leaf[r[3]])
    off = [0]
    for lv in range(1, nlev + 2):
        off.append(off[-1] + (count.get(lv, 0) + 63) // 64 * 64)
    return off


@pytest.mark.parametrize("name,selection", COMMITTED)
def test_level_rows_are_the_level_table_of_the_file(name, selection):
    path = os.path.join(POT, name)
    want = level_table(path)
    pot = capi.Potential(path, selection=selection)
    assert pot.sizes["levels"] == len(want) - 2
    for grade in ([False, True] if selection else [False]):
        got = pot.plan_fixed_fields(CUS, INUM, MAXN, grade=grade)
        assert got["nlevels"] == len(want) - 2
        assert len(got["level_rows"]) == ARR_LEN
        if len(want) <= ARR_LEN:
            assert got["level_rows"] == want + [0] * (ARR_LEN - len(want)), (name, want)
        else:   # the table does not fit: the field stays zero and the kernels keep reading the blob
            assert got["level_rows"] == [0] * ARR_LEN


def test_headline_table_has_the_blocks_the_fixed_shape_unrolls():
    """level 16: 10 | 2 | 1 blocks and 3 leaf blocks -- an odd block count in the last level and in the leaf sweep"""
    assert level_table(os.path.join(POT, "W_L16.mtp")) == [0, 640, 768, 832, 1024]
    # level 8: every level is a single block, so every trip of two has an idle slot
    t8 = level_table(os.path.join(POT, "W_L8.mtp"))
    assert all(b - a == 64 for a, b in zip(t8, t8[1:])), t8


def test_refit_keeps_level_rows_and_the_shape(tmp_pot_dir):
    p = mtpgen.random_potential(mtpgen.build_table(16), 1, 20251, 1.7, 5.6, 8, 0.37)
    path = str(tmp_pot_dir / "refit16_levels.mtp")
    mtpgen.write_mtp(p, path)
    pot = capi.Potential(path)
    assert pot.plan_fixed_shape(CUS, INUM, MAXN) == "w16_force_3ps"
    assert pot.plan_fixed_fields(CUS, INUM, MAXN)["level_rows"] == level_table(os.path.join(POT, "W_L16.mtp")) + [0] * 9


def _move_row_behind_its_readers(src, dst):
    """the text handling of tests/_mutate.py with another pick: the FIRST row of alpha_index_times (a product of two
    basics that deeper rows read) goes to the end of the file.  In file order (pair_mtp.cpp:196-201) its target is then
    complete only after its readers ran, so the row sits in a dependency level of its own behind them: more levels, the
    same counts (mutate_mtp's own pick stays inside the padding of the 64-row blocks)."""
    from _mutate import _block
    text = open(src).read()
    mt = _block(text, "alpha_index_times")
    rows = [tuple(int(v) for v in r) for r in re.findall(r"\{\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*\}", mt.group(2))]
    assert any(rows[0][3] in (r[0], r[1]) for r in rows[1:])
    rows.append(rows.pop(0))
    text = text[:mt.start(2)] + ", ".join("{%d, %d, %d, %d}" % r for r in rows) + text[mt.end(2):]
    open(dst, "w").write(text)
    return len(rows)


def test_a_row_in_another_level_does_not_match(tmp_pot_dir):
    """a level-16 table of the same sizes (rows, moments, basics, scalars) whose rows sit in other levels: the fixed
    shape must refuse it on level_rows / nlevels"""
    src = os.path.join(POT, "W_L16.mtp")
    dst = str(tmp_pot_dir / "moved16.mtp")
    assert _move_row_behind_its_readers(src, dst) == 894
    want = level_table(dst)
    assert want != level_table(src) and len(want) <= ARR_LEN
    pot, ref = capi.Potential(dst), capi.Potential(src)
    assert pot.sizes == dict(ref.sizes, levels=len(want) - 2)
    got = pot.plan_fixed_fields(CUS, INUM, MAXN)
    assert got["level_rows"] == want + [0] * (ARR_LEN - len(want))
    assert got["level_rows"] != ref.plan_fixed_fields(CUS, INUM, MAXN)["level_rows"]
    assert pot.plan_fixed_shape(CUS, INUM, MAXN) == ""
    # tests/_mutate.py's own pick (a late writer of a leaf row's factor) keeps the padded table, and with it the shape's
    # level constants stay valid: the match is decided by the other fields
    info = mutate_mtp(src, str(tmp_pot_dir / "late16.mtp"), late_writer=True, dup_mapping=False)
    assert "moved_row" in info
    late = capi.Potential(str(tmp_pot_dir / "late16.mtp"))
    assert late.plan_fixed_fields(CUS, INUM, MAXN)["level_rows"][:5] == level_table(str(tmp_pot_dir / "late16.mtp"))
