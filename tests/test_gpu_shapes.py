"""GPU parity on tables the level generator never makes (tests/_tables.py): one case per shipped force-kernel
instantiation, non-default radial bases (R, scaling, window), grades on both sides of the fused path, sparse tables
(coefficient blocks with holes), every forced LDS layout, the refusal limits at their edge and one past it, and four
and five species.  Tolerances are those of tests/test_gpu_parity.py."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system
from oracle.pyoracle import Oracle

import _tables
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")


def _system(ncell=(3, 3, 3), species=1, a=3.165, list_cutoff=7.0, seed=777):
    pos, box = mtpgen.bcc_lattice(*ncell, a=a, seed=seed)
    types = np.random.default_rng(5).integers(1, species + 1, size=len(pos)).astype(np.int32)
    return periodic_system(pos, box, types, list_cutoff)


def _check(path, s, grade=False, ctx_hook=None):
    """one call against the oracle: forces, energy per atom, eatom, virial, vatom; grades / coeff_ders on grade calls"""
    pot = capi.Potential(path, selection=grade)
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    if ctx_hook:
        ctx_hook(pot, ctx)
    got = ctx.compute(s.x, s.types, eflag=3, vflag=4, grade=grade)
    want = Oracle(path, selection=grade).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4,
                                                 extrapolation=grade, natoms=s.nlocal)
    _close(got["f"], want["f"], "forces")
    n = max(1, len(s.ilist))
    assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n)
    _close(got["eatom"], want["eatom"], "eatom", atol=1e-10)
    _close(got["virial"], want["virial"], "virial", atol=1e-8)
    _close(got["vatom"], want["vatom"], "vatom")
    if grade:
        if pot.info.configuration_mode:
            _close(got["coeff_ders"], want["coeff_ders"], "coeff_ders", atol=1e-9, rtol=1e-10)
        else:
            _close(got["grades"][s.ilist], want["grades"][s.ilist], "grades", atol=1e-9, rtol=1e-9)
            assert abs(got["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])
    return pot, ctx, got, want


# ---- one case per mtp_wave_kernel<KL, NB, PITCH, GRADE, DEG, WPS> (tests/test_shapes_cpu.py checks the list) -------


@pytest.mark.parametrize("case", _tables.MATRIX, ids=_tables.case_id)
def test_instantiation(tmp_path, monkeypatch, case):
    slots, subsets = _tables.case_slots(case)
    tab, nfac = _tables.make_table(slots, subsets)
    path = _tables.write(tab, nfac, str(tmp_path / "p.almtp"), mvs="nbh" if case["grade"] else None)
    monkeypatch.setenv("MTP_WPS", str(case["wps"]))
    # every other case on a compressed lattice: more than one 32-neighbour tile per atom
    dense = case["NB"] in (2, 4) or case["DEG"] == 6 and case["wps"] == 3
    s = _system((3, 3, 3), a=2.6 if dense else 3.165, list_cutoff=6.0)

    def hook(pot, ctx):
        ks = pot.kernel_shape()
        assert (ks["block_lanes"], ks["blocks_per_lane"], ks["max_degree"]) == (case["KL"], case["NB"], case["DEG"])
        assert ctx.plan_info()["waves_per_simd"] == case["wps"]

    _check(path, s, grade=case["grade"], ctx_hook=hook)


# ---- radial bases: R, scaling and the window ----------------------------------------------------------------------


@pytest.mark.parametrize("table,R,scaling,window", [
    (10, 1, 0.37, (2.9, 5.0)), (10, 2, 2.5, (1.4, 6.2)), (16, 3, 2.5, (2.9, 5.0)), (16, 7, 0.37, (1.4, 6.2)),
    (16, 9, 2.5, (1.4, 6.2)), ("wide", 16, 0.37, (2.9, 5.0)), ("wide", 9, 2.5, (1.4, 6.2))])
def test_radial_basis(tmp_path, table, R, scaling, window):
    path = str(tmp_path / "p.mtp")
    if table == "wide":
        tab, nfac = _tables.make_table(*_tables.shape_table(64, 2, 8))
        _tables.write(tab, nfac, path, species=2, R=R, scaling=scaling, min_dist=window[0], max_dist=window[1])
    else:
        mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(table), 2, 4242, window[0], window[1], R, scaling),
                         path)
    s = _system((3, 3, 3), species=2, list_cutoff=window[1] + 1.0)
    _check(path, s)


# ---- grades at the fused / unfused boundary (fused: R == 8, Mu <= 4, Sp <= 2) --------------------------------------


@pytest.mark.parametrize("level,species,R,scaling,mvs", [
    (16, 2, 8, 2.5, "nbh"),       # fused, scaling != 1
    (16, 1, 7, 1.0, "nbh"),       # unfused: R = 7
    (16, 2, 9, 0.37, "nbh"),      # unfused: R = 9
    (20, 1, 8, 1.0, "nbh"),       # unfused: Mu = 5
    (10, 3, 8, 1.0, "nbh"),       # unfused: Sp = 3
    (10, 2, 5, 2.5, "cfg")])      # configuration mode, R != 8
def test_grades_fused_boundary(tmp_path, level, species, R, scaling, mvs):
    p = mtpgen.random_potential(mtpgen.build_table(level), species, 99, 2.0, 5.0, R, scaling)
    mtpgen.add_selection_state(p, mvs, seed=3)
    path = str(tmp_path / "p.almtp")
    mtpgen.write_mtp(p, path)
    _check(path, _system((3, 3, 3), species=species, a=2.9, list_cutoff=6.0), grade=True)


# ---- sparse tables: coefficient blocks with holes, zero-filled per atom ----------------------------------------------


@pytest.mark.parametrize("shape", [(32, 1, 6), (64, 2, 8)])
@pytest.mark.parametrize("grade", [False, True])
def test_sparse_after_dense(tmp_path, shape, grade):
    """a dense potential first, then a sparse one: stale coefficients of an earlier atom (or potential) would show"""
    mvs = "nbh" if grade else None
    s = _system((3, 3, 3), a=2.6, list_cutoff=6.0)
    _check(os.path.join(POT, "W_L16_nbh.almtp" if grade else "W_L16.mtp"), s, grade=grade)
    slots, subsets = _tables.shape_table(*shape)
    assert any(len(v) < len(mtpgen.monomials(k[1])) for k, v in subsets.items())
    tab, nfac = _tables.make_table(slots, subsets)
    _check(_tables.write(tab, nfac, str(tmp_path / "sparse.almtp"), mvs=mvs), s, grade=grade)


# ---- forced LDS layouts ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("layout,mode", [("keep", 0), ("lean", 1), ("rebuild", 2), ("rebuild-nodg", 3)])
def test_forced_layout(monkeypatch, layout, mode):
    monkeypatch.setenv("MTP_LAYOUT", layout)
    monkeypatch.setenv("MTP_WPS", "2")
    for name, grade in (("W_L16.mtp", False), ("W_L16_nbh.almtp", True)):

        def hook(pot, ctx):
            assert ctx.layout_mode() == mode

        _check(os.path.join(POT, name), _system((3, 3, 3)), grade=grade, ctx_hook=hook)


# ---- limits at the edge, and one step past ------------------------------------------------------------------------


def test_grade_limit_sp_mu_r_256(tmp_path):
    tab, nfac = _tables.make_table([(mu, 0) for mu in range(8)] + [(0, 2), (7, 3)])
    s = _system((2, 2, 2), species=2)
    at = _tables.write(tab, nfac, str(tmp_path / "r16.almtp"), mvs="nbh", species=2, R=16)
    _check(at, s, grade=True)
    past = _tables.write(tab, nfac, str(tmp_path / "r17.almtp"), mvs="nbh", species=2, R=17)
    pot = capi.Potential(past, selection=True)
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    with pytest.raises(capi.MtpError, match="Sp\\*Mu\\*R above 256") as ei:
        ctx.compute(s.x, s.types, grade=True)
    assert ei.value.code == -24
    got = ctx.compute(s.x, s.types)                    # the same context still runs force calls
    want = Oracle(past).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(got["f"], want["f"], "forces after the refused grade call")


@pytest.mark.parametrize("what,edge,past,msg", [
    ("blocks", lambda: _tables.exact_blocks(256), lambda: _tables.exact_blocks(257),
     "more than 256 head x tail blocks"),
    ("basics", lambda: _tables.basic_limit_slots(0), lambda: _tables.basic_limit_slots(1),
     "alpha_index_basic_count above 640")], ids=["blocks", "basics"])
def test_context_limit(tmp_path, what, edge, past, msg):
    s = _system((3, 3, 3), a=2.9, list_cutoff=6.0)
    tab, nfac = _tables.make_table(*past())
    pot = capi.Potential(_tables.write(tab, nfac, str(tmp_path / "past.mtp")))
    with pytest.raises(capi.MtpError, match=msg) as ei:
        capi.Context(pot, 0)
    assert ei.value.code == -24
    tab, nfac = _tables.make_table(*edge())
    path = _tables.write(tab, nfac, str(tmp_path / "edge.mtp"))
    if what == "basics":
        assert capi.Potential(path).sizes["B"] == 640
    _check(path, s)                                    # a fresh context after the refusal


# ---- four and five species ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("species", [4, 5])
def test_many_species(tmp_path, species):
    path = str(tmp_path / "p.mtp")
    mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(10), species, 4242), path)
    _check(path, _system((3, 3, 3), species=species))


# ---- the context's plan is the host-only planner's (csrc/mtp_plan.hpp, tests/plan_dump.cpp) ------------------------------


@pytest.mark.parametrize("name", ["W_L8", "W_L16"])
@pytest.mark.parametrize("layout", [None, "rebuild"])
def test_context_plan_is_what_plan_dump_prints(tmp_path, monkeypatch, name, layout):
    """a context on the 54-atom cell of the golden fixtures reports the plan that the planner, built without the HIP
    runtime, prints for the same potential, CU count, list size, longest row and environment"""
    import torch
    from test_plan_cpu import dump

    g = np.load(os.path.join(ROOT, "tests", "golden", name + "_54.npz"))
    if layout:
        monkeypatch.setenv("MTP_LAYOUT", layout)
    ctx = capi.Context(capi.Potential(os.path.join(POT, name + ".mtp")), 0)
    ctx.set_neighbors(g["ilist"], g["first"], g["neigh"], len(g["x"]))
    got = ctx.compute(g["x"], g["types"])
    _close(got["f"], g["f"], "forces")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    inum, longest = len(g["ilist"]), int(np.diff(g["first"]).max())
    listf = tmp_path / "one.txt"
    listf.write_text("%s.mtp %d %d %d 0 %d%s\n" % (name, cus, inum, longest, inum, " MTP_LAYOUT=" + layout if layout else ""))
    header, line = dump(str(listf), tmp_path)
    rc, lp0, _, _, force = [part.split() for part in line.split(" | ")[:5]]
    assert rc == ["0", "0"]
    mode, wpb, grid, wave_doubles, rebuild, wps = (int(lp0[k]) for k in (0, 9, 10, 11, 16, 17))
    assert ctx.launch_info() == dict(lds_bytes_per_wave=8 * wave_doubles, waves_per_block=wpb, grid_blocks=grid,
                                     neighbor_tile=int(force[-3]))
    assert ctx.plan_info() == dict(waves_per_simd=wps, rebuild_tables=rebuild)
    assert ctx.layout_mode() == mode
