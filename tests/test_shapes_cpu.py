"""Tables beyond the level generator, without a GPU: every shipped force-kernel instantiation is claimed by a case of
the GPU matrix (tests/test_gpu_shapes.py) whose table the library really sends there (mtp_potential_kernel_shape);
the parser agrees with the oracle's on them; the oracle agrees with the closed-form definition for non-default radial
bases and with finite differences on rank-11, Mu-16 and sparse tables; the rank and radial-index caps are refused."""
import os
import re

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system
from oracle.pyoracle import Oracle

import _definition as defn
import _tables
from _codeobj import _kernels, code_object  # noqa: F401  (code_object: fixture)


def _instantiations(notes):
    """(KL, NB, GRADE, DEG, WPS) of every mtp_wave_kernel<KL, NB, PITCH, GRADE, DEG, WPS> in the code object"""
    out = set()
    for name in _kernels(notes):
        m = re.search(r"mtp_wave_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELi(\d+)E", name)
        if m:
            kl, nb, _pitch, g, deg, wps = (int(v) for v in m.groups())
            out.add((kl, nb, bool(g), deg, wps))
    return out


def _key(case):
    return (case["KL"], case["NB"], case["grade"], case["DEG"], case["wps"])


def test_every_instantiation_has_a_gpu_case(code_object):
    shipped = _instantiations(code_object[0])
    assert len(shipped) == 28, sorted(shipped)
    matrix = {_key(c) for c in _tables.MATRIX}
    assert shipped - matrix == set(), "instantiations no GPU case runs: %s" % sorted(shipped - matrix)
    assert matrix - shipped == set(), "GPU cases for instantiations the library does not ship: %s" % sorted(matrix - shipped)


@pytest.mark.parametrize("case", _tables.MATRIX, ids=_tables.case_id)
def test_matrix_case_lands_on_its_instantiation(tmp_path, case):
    tab, nfac = _tables.make_table(*_tables.case_slots(case))
    pot = capi.Potential(_tables.write(tab, nfac, str(tmp_path / "p.mtp")))
    ks = pot.kernel_shape()
    assert (ks["block_lanes"], ks["blocks_per_lane"], ks["max_degree"]) == (case["KL"], case["NB"], case["DEG"]), ks
    assert ks["fwd_blocks"] == _tables.block_count(*_tables.case_slots(case))
    if case["wps"] == 3:    # the 168-VGPR build only takes the dg-free layouts
        assert pot.sizes["Mu"] <= 4 and pot.sizes["P"] - 1 <= 6


def test_kernel_shape_rank_rule_at_dlow():
    """ranks exactly DLOW and DLOW + 1 on the narrow and the wide grids, rank 11 (P = MTP_PSTRIDE)"""
    want = {(16, 6): 6, (16, 7): 11, (32, 6): 6, (32, 7): 11, (64, 8): 8, (64, 9): 11, (64, 11): 11}
    got = {}
    for c in _tables.MATRIX:
        if c["wps"] == 2:
            tab, _ = _tables.make_table(*_tables.case_slots(c))
            got[(c["KL"], tab.sizes["P"] - 1)] = c["DEG"]
    for k, v in want.items():
        assert got.get(k) == v, (k, got)


def test_block_limit_is_refused_one_past_the_edge(tmp_path):
    tab, nfac = _tables.make_table(*_tables.exact_blocks(256))
    pot = capi.Potential(_tables.write(tab, nfac, str(tmp_path / "a.mtp")))
    assert pot.kernel_shape() == dict(fwd_blocks=256, block_lanes=64, blocks_per_lane=4, max_degree=11)
    tab, nfac = _tables.make_table(*_tables.exact_blocks(257))
    pot = capi.Potential(_tables.write(tab, nfac, str(tmp_path / "b.mtp")))
    with pytest.raises(capi.MtpError, match="257 head x tail blocks") as ei:
        pot.kernel_shape()
    assert ei.value.code == -24


@pytest.mark.parametrize("R,scaling,window,sparse", [(1, 0.37, (2.9, 5.0), False), (2, 2.5, (1.4, 6.2), True),
                                                     (3, 1.0, (2.0, 5.0), True), (13, 0.37, (1.4, 6.2), False),
                                                     (16, 2.5, (2.9, 5.0), True)])
def test_parser_matches_oracle_parser_on_new_tables(tmp_path, R, scaling, window, sparse):
    slots, subsets = _tables.shape_table(32, 1, 11) if sparse else (_tables.WPS3_SLOTS[32], {})
    tab, nfac = _tables.make_table(slots, subsets)
    path = _tables.write(tab, nfac, str(tmp_path / "p.almtp"), mvs="nbh", species=2, R=R, scaling=scaling,
                         min_dist=window[0], max_dist=window[1])
    p, o = capi.Potential(path, selection=True), Oracle(path, selection=True)
    so, sp = o.sizes, p.sizes
    for k in ("Sp", "R", "Mu", "A", "B", "T", "S", "P", "C"):
        assert so[k] == sp[k], k
    assert sp["R"] == R
    t = p.tables()
    np.testing.assert_array_equal(t["alpha_index_basic"].ravel(), o.arr("alpha_index_basic", 4 * so["B"], np.int32))
    np.testing.assert_array_equal(t["alpha_index_times"].ravel(), o.arr("alpha_index_times", 4 * so["T"], np.int32))
    np.testing.assert_array_equal(t["alpha_moment_mapping"], o.arr("alpha_moment_mapping", so["S"], np.int32))
    np.testing.assert_array_equal(t["radial_coeffs"], o.arr("radial_basis_coeffs", t["radial_coeffs"].size))
    np.testing.assert_array_equal(t["moment_coeffs"], o.arr("linear_coeffs", so["S"]))
    np.testing.assert_array_equal(t["species_coeffs"], o.arr("species_coeffs", so["Sp"]))
    np.testing.assert_array_equal(t["inverse_active_set"].ravel(), o.arr("inverse_active_set", so["C"] ** 2))
    assert p.info.max_cutoff == o.m.max_cutoff == window[1] and p.info.min_cutoff == o.m.min_cutoff == window[0]
    assert p.info.scaling == o.m.scaling == scaling


def _system(ncell=(3, 3, 3), species=1, a=3.165, list_cutoff=7.0, seed=777):
    pos, box = mtpgen.bcc_lattice(*ncell, a=a, seed=seed)
    types = np.random.default_rng(5).integers(1, species + 1, size=len(pos)).astype(np.int32)
    return periodic_system(pos, box, types, list_cutoff)


@pytest.mark.parametrize("level,R,scaling,window", [(8, 1, 0.37, (2.9, 5.0)), (8, 13, 2.5, (1.4, 6.2)),
                                                    (10, 2, 2.5, (2.9, 5.0)), (10, 5, 0.37, (1.4, 6.2)),
                                                    (12, 3, 0.37, (2.9, 5.0)), (12, 13, 2.5, (2.9, 5.0))])
def test_oracle_matches_definition_for_other_radial_bases(tmp_path, level, R, scaling, window):
    """R, scaling and the [min_dist, max_dist] window against the closed-form Chebyshev of tests/_definition.py; the
    bcc nearest neighbours (2.74 A) sit below min_dist = 2.9, where ksi < -1"""
    pot = mtpgen.random_potential(mtpgen.build_table(level), 2, 4242, window[0], window[1], R, scaling)
    path = str(tmp_path / "p.mtp")
    mtpgen.write_mtp(pot, path)
    s = _system((2, 2, 2), species=2, list_cutoff=window[1] + 1.0)
    d = np.linalg.norm(s.x[s.neigh] - s.x[np.repeat(s.ilist, np.diff(s.first))], axis=1)
    if window[0] > 2.8:
        assert (d < window[0]).any()
    res = Oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    E, _ = defn.site_energies(pot, pot.table.graphs, s)
    np.testing.assert_allclose(res["eatom"][:s.nlocal], E, rtol=2e-11, atol=1e-11)
    assert abs(res["energy"] - E.sum()) < 1e-10 * max(1.0, abs(E.sum()))


@pytest.mark.parametrize("which", ["rank11", "mu16", "sparse"])
def test_oracle_forces_are_minus_gradient_on_new_tables(tmp_path, which):
    slots, subsets = {"rank11": ([(0, 0), (0, 11), (1, 11)], {}),
                      "mu16": ([(mu, 0) for mu in range(16)] + [(mu, 2) for mu in range(0, 16, 3)], {}),
                      "sparse": _tables.shape_table(64, 2, 8)}[which]
    tab, nfac = _tables.make_table(slots, subsets)
    path = _tables.write(tab, nfac, str(tmp_path / "p.mtp"), species=2, R=9, scaling=2.5, min_dist=2.9, max_dist=5.0)
    o = Oracle(path)
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    types = np.random.default_rng(5).integers(1, 3, size=len(pos)).astype(np.int32)

    def energy_forces(p):
        s = periodic_system(p, box, types, 6.0)
        r = o.compute(s.x, s.types, s.ilist, s.first, s.neigh)
        return r["energy"], s.fold_forces(r["f"])

    E, F = energy_forces(pos)
    assert np.abs(F).max() > 1e-3
    assert np.abs(F.sum(0)).max() < 1e-10 * max(1.0, np.abs(F).max())
    h = 1e-5
    for (a, c) in [(0, 0), (5, 1), (11, 2), (15, 0)]:
        pp = pos.copy(); pp[a, c] += h
        pm = pos.copy(); pm[a, c] -= h
        fd = -(energy_forces(pp)[0] - energy_forces(pm)[0]) / (2 * h)
        assert abs(fd - F[a, c]) < 2e-7 * max(1.0, np.abs(F).max()), (a, c, fd, F[a, c])


@pytest.mark.parametrize("slots,what", [([(0, 0), (0, 12)], "tensor rank above 11"),
                                        ([(0, 0), (16, 1)], "radial function index above 15")])
def test_load_time_limits_refused(tmp_path, slots, what):
    tab, nfac = _tables.make_table(slots)
    path = _tables.write(tab, nfac, str(tmp_path / "p.mtp"))
    with pytest.raises(capi.MtpError, match=what) as ei:
        capi.Potential(path)
    assert ei.value.code == -24
    ok, nfac = _tables.make_table([(s[0] if s[0] < 16 else 15, min(s[1], 11)) for s in slots])
    capi.Potential(_tables.write(ok, nfac, str(tmp_path / "ok.mtp")))   # one step inside: loads
