"""The slot tables as fields of the force kernel's argument block (csrc/mtp_device.hpp: slot_row, slot_mu_lo / _hi),
without a GPU: what the host-only planner reports equals the slot and slot -> mu tables the blob carries -- recomputed
here from the file's alpha_index_basic with the numbering rule of csrc/mtp_potential.cpp (build_slots: by tensor rank,
then by radial function, over the (mu, rank) pairs that occur), sharing no code with the library -- for every committed
potential; neither the fit nor the bank-search effort moves them, and a table with another slot structure does not match
the fixed shape."""
import importlib.util
import os
import re

import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
CUS, INUM, MAXN = 256, 65536, 94
PSTRIDE, ROWS_MU = 12, 4   # MTP_PSTRIDE, MTP_SLOT_ROWS_MU
FORCE = "w16_force_3ps"
COMMITTED = [("W_L8.mtp", False), ("W_L16.mtp", False), ("W_L16_nbh.almtp", True), ("WRe_L10_cfg.almtp", True),
             ("WRe_L20.mtp", False)]


def _ints(txt, key):
    m = re.search(r"^\s*%s\s*=\s*(.*)$" % key, txt, flags=re.M)
    return [int(v) for v in re.findall(r"-?\d+", m.group(1))]


def slot_tables(path):
    """(Mu, P, slot_of {(mu, nu): slot}, slot_mu [slot] -> mu) of the file"""
    raw = open(path, "rb").read()
    cut = raw.find(b"#MVS_v1.1")
    txt = (raw if cut < 0 else raw[:cut]).decode()
    Mu = _ints(txt, "radial_funcs_count")[0]
    b = _ints(txt, "alpha_index_basic")
    basics = [tuple(b[4 * k:4 * k + 4]) for k in range(len(b) // 4)]
    assert len(basics) == _ints(txt, "alpha_index_basic_count")[0]
    used = {(q[0], q[1] + q[2] + q[3]) for q in basics}
    P = max(nu for _, nu in used) + 1
    slot_of, slot_mu = {}, []
    for nu in range(P):
        for mu in range(Mu):
            if (mu, nu) in used:
                slot_of[(mu, nu)] = len(slot_mu)
                slot_mu.append(mu)
    return Mu, P, slot_of, slot_mu


def expected_fields(path):
    Mu, P, slot_of, slot_mu = slot_tables(path)
    bits = 0
    if Mu <= 4 and len(slot_mu) <= 32:
        for s, mu in enumerate(slot_mu):
            bits |= mu << (2 * s)
    row = [-1] * (ROWS_MU * PSTRIDE)
    if Mu <= ROWS_MU and len(slot_mu) <= 127 and P <= PSTRIDE:
        for (mu, nu), s in slot_of.items():
            row[mu * PSTRIDE + nu] = s

    def i32(v):
        return v - (1 << 32) if v >= 1 << 31 else v
    return dict(slot_row=row, slot_mu_lo=i32(bits & 0xffffffff), slot_mu_hi=i32(bits >> 32))


def _slot_fields(fields):
    return {k: fields[k] for k in ("slot_row", "slot_mu_lo", "slot_mu_hi")}


def _written(tmp_pot_dir, name, pot):
    path = str(tmp_pot_dir / name)
    mtpgen.write_mtp(pot, path)
    return path


@pytest.mark.parametrize("name,selection", COMMITTED)
def test_slot_fields_are_the_slot_tables_of_the_file(name, selection):
    path = os.path.join(POT, name)
    want = expected_fields(path)
    Mu, P, slot_of, slot_mu = slot_tables(path)
    pot = capi.Potential(path, selection=selection)
    for grade in ([False, True] if selection else [False]):
        got = pot.plan_fixed_fields(CUS, INUM, MAXN, grade=grade)
        assert got["Mu"] == Mu and got["P"] == P and got["nslot"] == len(slot_mu)
        assert len(got["slot_row"]) == ROWS_MU * PSTRIDE
        assert _slot_fields(got) == want, name
        # the ranks' first slots, which the force phase pairs with the map, count the same slots
        assert got["deg_first"][:P + 1] == [sum(1 for (_, nu) in slot_of if nu < d) for d in range(P + 1)]


def test_headline_table_has_the_rows_the_fixed_shape_builds_from():
    """level 16: sixteen slots; radial functions 0 / 1 and 2 / 3 (one per half-wavefront) have their rows one apart where
    both have one, and ranks 5, 6 (mu = 0) and 1, 2 (mu = 2) belong to one half only"""
    Mu, P, slot_of, slot_mu = slot_tables(os.path.join(POT, "W_L16.mtp"))
    assert (Mu, P, len(slot_mu)) == (4, 7, 16)
    assert [slot_of.get((0, nu), -1) for nu in range(P)] == [0, 4, 7, 10, 12, 14, 15]
    assert [slot_of.get((1, nu), -1) for nu in range(P)] == [1, 5, 8, 11, 13, -1, -1]
    assert [slot_of.get((2, nu), -1) for nu in range(P)] == [2, 6, 9, -1, -1, -1, -1]
    assert [slot_of.get((3, nu), -1) for nu in range(P)] == [3, -1, -1, -1, -1, -1, -1]
    assert slot_mu == [0, 1, 2, 3, 0, 1, 2, 0, 1, 2, 0, 1, 0, 1, 0, 0]


def test_committed_shape_carries_the_slot_tables():
    spec = importlib.util.spec_from_file_location("gen_fixed_shapes", os.path.join(ROOT, "scripts", "gen_fixed_shapes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text = open(gen.OUT).read()
    force = text[text.index("struct Shape_" + FORCE):text.index("struct Shape_w16_grade_3ps")]
    want = expected_fields(os.path.join(POT, "W_L16.mtp"))
    assert "slot_mu_lo = %d;" % want["slot_mu_lo"] in force and "slot_mu_hi = %d;" % want["slot_mu_hi"] in force
    assert "v[48] = {%s};" % ", ".join(str(v) for v in want["slot_row"]) in force


@pytest.mark.parametrize("rounds", ["0", "2", "8"])
def test_slot_fields_do_not_depend_on_the_bank_search_effort(rounds, monkeypatch):
    path = os.path.join(POT, "W_L16.mtp")
    with monkeypatch.context() as m:
        m.setenv("MTP_BANK_ROUNDS", rounds)
        if rounds == "8":
            m.delenv("MTP_BANK_SCALE", raising=False)
        pot = capi.Potential(path)
    assert _slot_fields(pot.plan_fixed_fields(CUS, INUM, MAXN)) == expected_fields(path)
    assert pot.plan_fixed_shape(CUS, INUM, MAXN) == FORCE


def test_refit_of_the_level_16_table_keeps_the_slot_fields(tmp_pot_dir):
    """the potential of tests/test_fixed_shapes_cpu.py: other coefficients, cutoffs and scaling"""
    p = mtpgen.random_potential(mtpgen.build_table(16), 1, 20251, 1.7, 5.6, 8, 0.37)
    path = _written(tmp_pot_dir, "refit16_slots.mtp", p)
    pot = capi.Potential(path)
    want = expected_fields(os.path.join(POT, "W_L16.mtp"))
    assert expected_fields(path) == want
    assert _slot_fields(pot.plan_fixed_fields(CUS, INUM, MAXN)) == want
    assert pot.plan_fixed_shape(CUS, INUM, MAXN) == FORCE


def test_another_slot_structure_does_not_match(tmp_pot_dir):
    ref = expected_fields(os.path.join(POT, "W_L16.mtp"))
    # level 16 with two species: the same slots (the alpha tables do not know the species), refused on Sp
    two = _written(tmp_pot_dir, "two16_slots.mtp", mtpgen.random_potential(mtpgen.build_table(16), 2, 4242))
    pot2 = capi.Potential(two)
    got2 = pot2.plan_fixed_fields(CUS, INUM, MAXN)
    assert _slot_fields(got2) == expected_fields(two) == ref
    assert got2["Sp"] == 2 and pot2.plan_fixed_shape(CUS, INUM, MAXN) == ""
    # level 8: other slots
    w8 = os.path.join(POT, "W_L8.mtp")
    pot8 = capi.Potential(w8)
    got8 = _slot_fields(pot8.plan_fixed_fields(CUS, INUM, MAXN))
    assert got8 == expected_fields(w8)
    assert got8["slot_row"] != ref["slot_row"] and got8["slot_mu_lo"] != ref["slot_mu_lo"]
    assert pot8.plan_fixed_shape(CUS, INUM, MAXN) == ""
