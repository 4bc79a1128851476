"""Host side of installing new coefficients into a live context (include/mtp_mi355x.h, "installing ..."): the
coefficient tables of the native schedule rebuilt on a fixed structure, the structure gate, and both under ASan + UBSan.
The device side is tests/test_install_gpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _install import CELLS, POT, ROOT, bound, golden_cell, text_only, write_perturbed   # noqa: E402
from _mutate import mutate_mtp   # noqa: E402

COMMITTED = ["W_L8.mtp", "W_L16.mtp", "W_L16_nbh.almtp", "WRe_L20.mtp", "WRe_L10_cfg.almtp"]
MUTANTS = {"dup_mapping": dict(late_writer=False, dup_mapping=True), "late_writer": dict(late_writer=True, dup_mapping=False),
           "both": dict(late_writer=True, dup_mapping=True)}
TABLES = ("radial", "species", "seed_val", "e_lin", "leaf_cf", "leaf_cb")


def _source(tmp_path, name):
    """path of a committed potential, or of a mutant of W_L16.mtp / WRe_L10_cfg.almtp (text only)"""
    if name in COMMITTED:
        return os.path.join(POT, name)
    base, kind = name.split(":")
    plain = text_only(os.path.join(POT, base), str(tmp_path / "plain.mtp"))
    dst = str(tmp_path / ("%s.mtp" % kind))
    info = mutate_mtp(plain, dst, **MUTANTS[kind])
    assert info["leaves"] > 0
    return dst


ALL = COMMITTED + ["W_L16.mtp:%s" % k for k in MUTANTS] + ["WRe_L10_cfg.almtp:dup_mapping"]


# ---- 1. the tables on the old structure against a load of the written file ------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_coeff_tables_equal_a_load_of_the_written_file(tmp_path, name):
    """mtp_potential_coeff_tables(old potential, new arrays) is, bit for bit, what a potential loaded from the file that
    carries the new arrays holds: the writer guarantees a bit-for-bit read-back and both sides run one function."""
    src = _source(tmp_path, name)
    dst = str(tmp_path / "new.mtp")
    ra, sp, mo = write_perturbed(src, dst)
    old, new = capi.Potential(src), capi.Potential(dst)
    got, want = old.coeff_tables(ra, sp, mo), new.coeff_tables()
    own = old.coeff_tables()
    for k in TABLES:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["radial"], ra) and np.array_equal(got["species"], sp)
    assert not np.array_equal(own["seed_val"], got["seed_val"]) or len(own["seed_val"]) == 0
    assert len(got["leaf_cf"]) == len(got["leaf_cb"])
    if "dup_mapping" in name or name.endswith(":both"):
        # two scalars on one leaf moment: the energy constant sums them, the adjoint constant keeps the last
        assert not np.array_equal(got["leaf_cf"], got["leaf_cb"])
    elif ":" not in name:
        assert np.array_equal(got["leaf_cf"], got["leaf_cb"])
    # one block at a time: the other two keep the potential's values
    part = old.coeff_tables(moment_coeffs=mo)
    assert np.array_equal(part["radial"], own["radial"]) and np.array_equal(part["species"], own["species"])
    for k in ("seed_val", "e_lin", "leaf_cf", "leaf_cb"):
        assert np.array_equal(part[k], got[k]), k


def test_coeff_tables_refuse_bad_input():
    pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
    t = pot.tables()
    for key, kw in (("radial_coeffs", "radial_coeffs"), ("species_coeffs", "species_coeffs"), ("moment_coeffs", "moment_coeffs")):
        for bad in (np.nan, np.inf, -np.inf):
            a = t[key].copy().reshape(-1)
            a[-1] = bad
            with pytest.raises(capi.MtpError) as e:
                pot.coeff_tables(**{kw: a})
            assert e.value.code == -20
        with pytest.raises(capi.MtpError) as e:
            pot.coeff_tables(**{kw: np.zeros(t[key].size + 1)})
        assert e.value.code == -20


# ---- 2. the structure gate --------------------------------------------------------------------------------------------------
def _edit(src, dst, pattern, repl, count=1):
    data = open(src, "rb").read()
    new, n = re.subn(pattern, repl, data, count=count)
    assert n == count, pattern
    open(dst, "wb").write(new)
    return dst


def test_compatible_accepts_new_coefficients_and_selection_blocks(tmp_path):
    src = os.path.join(POT, "W_L16_nbh.almtp")
    pot = capi.Potential(src, selection=True)
    dst = str(tmp_path / "coeffs.mtp")
    write_perturbed(src, dst)                                  # (the writer leaves the #MVS tail out)
    assert pot.compatible(dst, selection=False) is None
    with pytest.raises(capi.MtpError) as e:                    # no tail: with a selection wish the file does not parse
        pot.compatible(dst)
    assert e.value.code == -8
    C = pot.info.coeff_count
    rng = np.random.default_rng(3)
    S = 2.0 * np.eye(C) + 0.05 * rng.uniform(-1, 1, (C, C))
    sel = str(tmp_path / "sel.almtp")
    capi.write_selection(src, sel, S, np.linalg.inv(S))
    assert pot.compatible(sel) is None and pot.compatible(src) is None


def test_compatible_names_the_first_difference(tmp_path):
    src = os.path.join(POT, "W_L16_nbh.almtp")
    pot = capi.Potential(src, selection=True)
    t = pot.tables()
    row = t["alpha_index_times"][5]
    cases = {
        "alpha_index_times[5][2]": _edit(src, str(tmp_path / "times.almtp"),
                                         (r"\{%d, %d, %d, %d\}" % tuple(row)).encode(),
                                         ("{%d, %d, %d, %d}" % (row[0], row[1], row[2] + 1, row[3])).encode()),
        "scaling": _edit(src, str(tmp_path / "scaling.almtp"), rb"(potential_name = [^\n]*\n)", rb"\1scaling = 1.5\n"),
        "max_dist": _edit(src, str(tmp_path / "cut.almtp"), rb"max_dist = 5\.0+e\+00", b"max_dist = 5.100000000000000e+00"),
        "selection mode": _edit(_edit(src, str(tmp_path / "mode0.almtp"), rb"energy_weight = 0", b"energy_weight = 1"),
                                str(tmp_path / "mode.almtp"), rb"site_en_weight = 1", b"site_en_weight = 0"),
    }
    S = pot.info.alpha_scalar_count
    mapping = t["alpha_moment_mapping"]
    new_last = int(mapping[-2])
    cases["alpha_moment_mapping[%d]" % (S - 1)] = _edit(
        src, str(tmp_path / "map.almtp"), (r"(alpha_moment_mapping = \{[^}]*)\b%d\}" % mapping[-1]).encode(), (r"\g<1>%d}" % new_last).encode())
    for field, path in cases.items():
        msg = pot.compatible(path)
        assert msg is not None and field in msg, (field, msg)
    # nothing else differs: without a selection wish the mode is not looked at
    assert pot.compatible(cases["selection mode"], selection=False) is None
    # the level (another table), species_count and radial_basis_size: generated potentials that differ in one thing
    tab8 = mtpgen.level8_template()

    def gen(name, table=tab8, **kw):
        path = str(tmp_path / name)
        mtpgen.write_mtp(mtpgen.random_potential(table, **kw), path)
        return path
    base = capi.Potential(gen("base.mtp", species_count=1, seed=7))
    assert base.compatible(gen("same.mtp", species_count=1, seed=8)) is None          # other values, same structure
    assert "species_count" in base.compatible(gen("sp2.mtp", species_count=2, seed=7))
    assert "radial_basis_size" in base.compatible(gen("r6.mtp", species_count=1, seed=7, radial_basis_size=6))
    msg = base.compatible(gen("l10.mtp", table=mtpgen.build_table(10), species_count=1, seed=7))
    assert msg is not None and re.search(r"radial_funcs_count|alpha_\w+", msg), msg
    msg = pot.compatible(os.path.join(POT, "W_L8.mtp"), selection=False)
    assert msg is not None and re.search(r"radial_funcs_count|alpha_\w+", msg), msg


# ---- 3. the perturbation is no no-op: the GPU comparison of an installed context cannot pass with stale tables --------------
@pytest.mark.parametrize("name", ["W_L8.mtp", "W_L16.mtp", "WRe_L20.mtp"])
def test_perturbation_moves_the_forces_far_beyond_the_parity_bound(tmp_path, name):
    from oracle.pyoracle import Oracle
    src = os.path.join(POT, name)
    s = golden_cell(name)
    f_old = Oracle(src).compute(s.x, s.types, s.ilist, s.first, s.neigh)["f"]
    for blocks in (("radial", "species", "moments"), ("radial",), ("moments",)):
        dst = str(tmp_path / ("new_%s.mtp" % "_".join(blocks)))
        write_perturbed(src, dst, blocks=blocks)
        f_new = Oracle(dst).compute(s.x, s.types, s.ilist, s.first, s.neigh)["f"]
        moved = float(np.abs(f_new - f_old).max())
        print("%s %s: max|F_new - F_old| = %.3e, bound %.3e" % (name, blocks, moved, bound(f_new)))
        assert moved >= 1e3 * bound(f_new), (name, blocks, moved)
    # (the species block moves energies only: eatom)
    dst = str(tmp_path / "new_species.mtp")
    write_perturbed(src, dst, blocks=("species",))
    e_old = Oracle(src).compute(s.x, s.types, s.ilist, s.first, s.neigh)["eatom"]
    e_new = Oracle(dst).compute(s.x, s.types, s.ilist, s.first, s.neigh)["eatom"]
    assert float(np.abs(e_new - e_old).max()) >= 1e3 * bound(e_new)
    assert set(CELLS) >= {name}


# ---- 4. both under ASan + UBSan, in a program of their own -------------------------------------------------------------------
@pytest.fixture(scope="module")
def san_exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "host"), "san_install"])
    return os.path.join(ROOT, "tests", "cpp", "test_install_san")


@pytest.mark.parametrize("name", ALL)
def test_tables_and_gate_run_clean_under_sanitizers(san_exe, tmp_path, name):
    src = text_only(_source(tmp_path, name), str(tmp_path / "src.mtp"))
    others = [os.path.join(POT, "W_L8.mtp"), os.path.join(POT, "WRe_L20.mtp"), src]
    # (one round of the LDS-bank search and no program refinement: the numbering is not what this program checks, and the
    # instrumented build pays for every proposal)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               MTP_BANK_ROUNDS="1", MTP_BANK_SCALE="1", MTP_REFINE_PROGRAMS="0")
    r = subprocess.run([san_exe, src, str(tmp_path / "out.mtp")] + others, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
    words = r.stdout.split()
    assert words[0] == "OK", r.stdout
    want = [0 if os.path.basename(o) == name or o == src else -6 for o in others]
    assert [int(w) for w in words[5:]] == want, r.stdout
    if "dup_mapping" in name or name.endswith(":both"):
        assert int(words[4]) > 0, r.stdout                      # leaf rows whose two constants differ
