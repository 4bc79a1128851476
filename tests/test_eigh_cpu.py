"""The batched symmetric eigen-solver without a GPU (mtp_eigh_batched, md.modes_cells): the round-robin pair schedule, the numpy
twin of tests/_eigh.py -- the kernel's algorithm, order and threshold -- against numpy.linalg.eigh over the matrix families
within the issue's bounds, exact scaling by powers of two, and the refusals that come before a device is touched."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, md

import _eigh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_pair_once_per_sweep_and_disjoint_within_a_step():
    for N in range(1, 194):
        Ne = N + (N & 1)
        steps = _eigh.schedule(N)
        assert len(steps) == Ne - 1
        seen = set()
        for p, q in steps:
            assert len(p) == Ne // 2 and (p < q).all()
            both = np.concatenate([p, q])
            assert len(np.unique(both)) == Ne and both.min() == 0 and both.max() == Ne - 1, N        # disjoint, and everyone is in
            if N & 1:
                assert q[0] == N and (q[1:] < N).all(), N         # the padding index sits in pair 0 and nowhere else
            seen.update(zip(p.tolist(), q.tolist()))
        assert len(seen) == Ne * (Ne - 1) // 2, N                 # (Ne - 1) Ne / 2 slots, as many different pairs: each once


@functools.lru_cache(maxsize=None)
def _solved(name, N):
    A, root, project = _eigh.family(name, N)
    return _eigh.solve(A, root, project)


@pytest.mark.parametrize("name", _eigh.FAMILIES)
def test_twin_against_lapack(name):
    """|lambda - lambda_lapack| <= 8 N eps |A|_F, max |A V - V Lambda| <= 8 N eps |A|_F, max |V^T V - I| <= 16 N eps and at most
    30 sweeps, A the prepared matrix.  The constants are 4-5 times the worst ratios a prototype of this algorithm showed against
    LAPACK (1.65, 1.38, 3.1; at most 15 sweeps); they are not derived."""
    worst, most = np.zeros(3), 0
    for N in _eigh.SIZES:
        r = _solved(name, N)
        assert r["status"] == 0 and r["info"][0] <= 30, (name, N)
        got = np.array(_eigh.ratios(r["A"], r["W"], r["V"]))
        worst, most = np.maximum(worst, got), max(most, int(r["info"][0]))
        assert (np.diff(r["W"]) >= 0.0).all(), (name, N)
        assert (got <= np.array(_eigh.BOUNDS)).all(), (name, N, got)
        if name in ("diagonal", "zero"):
            assert r["info"][0] == 1 and r["info"][1] == 0.0 and np.array_equal(r["V"], np.eye(N)[:, np.argsort(np.diag(r["A"]), kind="stable")])
    print("%s: worst ratios to N eps |A|_F, N eps |A|_F, N eps: %.2f %.2f %.2f (bounds 8, 8, 16); at most %d sweeps"
          % (name, worst[0], worst[1], worst[2], most))


def test_the_projected_family_has_three_zero_modes_and_the_matrix_of_md_modes():
    """The prepared matrix is P (H / root root^T) P of md.modes: u is a sum of N / 3 products against a unit vector, so an entry
    is off by at most about N eps |A|_F on either side: 4 N eps |A|_F between the two."""
    worst = 0.0
    for N in _eigh.SIZES:
        A, root, _ = _eigh.family("projected", N)
        r = _solved("projected", N)
        Hw = A / np.outer(root, root)
        P = _eigh.projector(N, root)
        want = P @ (0.5 * (Hw + Hw.T)) @ P
        scale = N * _eigh.EPS * np.linalg.norm(Hw)
        worst = max(worst, np.abs(r["A"] - want).max() / scale)
        assert np.abs(r["A"] - want).max() <= 4.0 * scale, N
        assert np.sort(np.abs(r["W"]))[2] <= 8.0 * scale, N
        if N > 3:
            assert np.sort(np.abs(r["W"]))[3] > 1e3 * scale, N
        host = md.modes(A, root[::3] ** 2)
        assert np.abs(host["eigenvalues"] - r["W"]).max() <= 8.0 * scale + 8.0 * N * _eigh.EPS * np.linalg.norm(r["A"]), N
    print("projected: worst |A - P H P| / (N eps |H|_F) = %.3f (bound 4)" % worst)


def test_eigenvalues_in_triples_come_out_as_triples():
    for N in _eigh.SIZES:
        r = _solved("triples", N)
        want = 1.0 + (np.arange(N) // 3)
        assert np.abs(r["W"] - want).max() <= 8.0 * N * _eigh.EPS * np.linalg.norm(r["A"]), N


@pytest.mark.parametrize("power", [100, -100])
def test_a_power_of_two_scales_the_eigenvalues_exactly(power):
    for N in _eigh.SIZES:
        A = _eigh.random_symmetric(N, 11)
        base, scaled = _solved("random", N), _eigh.solve(A * 2.0 ** power)
        assert np.array_equal(scaled["W"], base["W"] * 2.0 ** power), (N, power)
        assert np.array_equal(scaled["V"], base["V"]) and scaled["info"][0] == base["info"][0], (N, power)


def test_max_sweeps_ends_the_solve_and_a_bad_matrix_fails():
    A = _eigh.random_symmetric(48, 5)
    r = _eigh.solve(A, max_sweeps=1)
    assert r["status"] == _eigh.NOT_CONVERGED and r["info"][0] == 1 and r["info"][1] > 0.0 and (np.diff(r["W"]) >= 0.0).all()
    B = A.copy()
    B[3, 7] = np.nan
    r = _eigh.solve(B)
    assert r["status"] == _eigh.FAILED and np.isnan(r["W"]).all() and np.isnan(r["V"]).all() and np.isnan(r["info"]).all()
    assert _eigh.solve(_eigh.random_symmetric(49, 5), project=True)["status"] == _eigh.FAILED


# ---- refusals before a device is touched -------------------------------------------------------------------------------------

def test_the_binding_has_the_headers_constants():
    text = open(os.path.join(ROOT, "include", "mtp_mi355x.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert "mtp_eigh_batched" in capi.EXPORTS
    assert capi.EIGH_STATUS == ("ok", "failed", "not converged", "too large")
    assert [value("MTP_EIGH_FAILED"), value("MTP_EIGH_NOT_CONVERGED"), value("MTP_EIGH_TOO_LARGE")] == [1, 2, 3]
    assert capi.EIGH_MAX_N == value("MTP_EIGH_MAX_N") == _eigh.MAX_N
    assert capi.EIGH_MAX_N_VECTORS == value("MTP_EIGH_MAX_N_VECTORS") == _eigh.MAX_N_VECTORS
    assert value("MTP_EIGH_TIER_SMALL") == _eigh.TIER_SMALL


def test_the_entry_point_refuses_bad_arguments_before_touching_a_pointer():
    """every pointer is a made-up address: a call that got past the checks would crash here"""
    L = capi.lib()
    p = C.c_void_p(4096)
    required = (0, 1, 2, 3, 5, 7, 8)          # n, a_first, A, w_first, W, info, status; 4 (root) and 6 (V) may be NULL

    def call(stream=p, nmat=3, project=1, max_sweeps=30, null=None):
        q = [None if i == null else p for i in range(9)]
        return L.mtp_eigh_batched(stream, nmat, q[0], q[1], q[2], q[3], q[4], project, max_sweeps, q[5], q[6], q[7], q[8])

    assert call(stream=None) == -20 and call(nmat=-1) == -20 and call(max_sweeps=0) == -20 and call(max_sweeps=-3) == -20
    for i in required:
        assert call(null=i) == -20, i
    assert call(nmat=0) == 0 and call(nmat=0, null=2) == 0                    # no-op successes
    assert call(nmat=0, stream=None) == -20 and call(nmat=0, max_sweeps=0) == -20


def test_modes_cells_refuses_bad_arguments_before_touching_the_device():
    H = _eigh.random_symmetric(6, 1)
    bad = [dict(hessians=[np.zeros((6, 5))]), dict(hessians=[np.zeros((4, 4))]), dict(hessians=[np.zeros(9)]),
           dict(hessians=[H], masses_of_atoms=[[1.0, 2.0, 3.0]]), dict(hessians=[H], masses_of_atoms=[[1.0, -2.0]]),
           dict(hessians=[H], masses_of_atoms=-1.0), dict(hessians=[H, H], masses_of_atoms=[[1.0, 2.0]]),
           dict(hessians=[H], masses_of_atoms=[[1.0, np.inf]]), dict(hessians=[H], zero_tol=-1.0), dict(hessians=[H], max_sweeps=0),
           dict(hessians=[H, np.full((3, 3), np.nan)])]
    for kw in bad:
        with pytest.raises(ValueError):
            md.modes_cells(**kw)
    assert md.modes_cells([]) == []
