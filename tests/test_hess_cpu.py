"""Batched force constants without a GPU: the numpy twin of mtp_hess_step / mtp_hess_finish (tests/_hess.py) on the analytic
surface of tests/_neb.py at its saddle against the analytic Hessian, within the truncation error of a central difference
derived from the surface's constants; md.modes and md.vineyard_prefactor on spectra known in closed form; the refusals of
md.hessian_cells and of the two entry points before anything touches a device; and the pass cut by max_hessian_bytes."""
import ctypes as C
import types

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi
from lammps_mtp_kokkos_amd.md import FTM2V, cut_hessian_passes, hessian_cells, modes, plan_cell_passes, vineyard_prefactor

import _cells
import _hess
import _neb

EPS = np.finfo(np.float64).eps


# ---- the twin on the surface -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes, h", [((1,), 0.01), ((5,), 0.01), ((2, 0, 7), 0.02), ((3, 64), 0.005)])
def test_the_twin_finds_the_saddle_hessian_within_the_truncation_error(sizes, h):
    """Atoms exactly at their saddles u = (0, C, 0).  The surface is E = A q^2 + B w^2 + D uz^2 + G d^2 with q = ux^2 - 1 and
    w = uy + C q: a polynomial, of degree 4 in ux (terms A ux^4 and B C^2 ux^4) and of degree 2 in everything else.  A central
    difference of a cubic force is f' + h^2 / 6 f''' exactly, and the only third derivative of a force that does not vanish
    is d^3 fx / dux^3 = -d^4 E / dux^4 = -24 (A + B C^2): the xx entry of every atom is off by exactly 4 (A + B C^2) h^2, every
    other entry by rounding alone.  Rounding: u = x - site loses eps |x| absolutely, which the force carries with |H|, and the
    difference quotient divides the two errors by 2 h; sixteen such terms are allowed."""
    S = _hess.surface_batch(sizes, noise=0.0)
    twin, x = _hess.run_surface(S, "all", h)
    assert np.array_equal(x, S["x0"]) and not twin.status.any()
    for j, n in enumerate(sizes):
        if n == 0:
            continue
        r0, r1 = int(S["cfg_first"][j]), int(S["cfg_first"][j + 1])
        want = _neb.saddle_hessian(*[S[k][r0:r1] for k in ("A", "B", "C", "D", "G")])
        trunc = np.zeros_like(want)
        trunc[np.arange(0, 3 * n, 3), np.arange(0, 3 * n, 3)] = 4.0 * (S["A"][r0:r1] + S["B"][r0:r1] * S["C"][r0:r1] ** 2) * h * h
        rounding = 16.0 * EPS * float(np.abs(S["x0"][r0:r1]).max()) * float(np.abs(want).max()) / h
        got = twin.matrix(j)
        err = np.abs(got - want)
        print("%d atoms, h %g: worst error %.3e (truncation bound %.3e, rounding allowance %.3e), asymmetry %.3e, sum rule %.3e"
              % (n, h, err.max(), trunc.max(), rounding, twin.diag[j, 0], twin.diag[j, 1]))
        assert (err <= trunc + rounding).all()
        assert np.abs(got - (want + trunc)).max() <= rounding          # the truncation error is exactly the one derived
        assert np.array_equal(got, got.T) and twin.diag[j, 0] <= rounding
        # f0, fmax and the energy of launch 0 are those of the surface
        e, f = _neb.surface(np, S["x0"], *[S[k] for k in _neb.SURFACE_KEYS])
        assert np.array_equal(twin.f0[r0:r1], f[r0:r1])
        assert twin.fmax[j] == np.sqrt(((f[r0:r1, 0] ** 2 + f[r0:r1, 1] ** 2) + f[r0:r1, 2] ** 2).max())
        assert abs(twin.energy[j] - e[r0:r1].sum()) <= n * EPS * np.abs(e[r0:r1]).sum()


def test_the_twin_selections_are_blocks_of_the_full_matrix_and_failures_stay_at_home():
    S = _hess.surface_batch((5, 3, 8, 0, 6), noise=0.02)
    full, _ = _hess.run_surface(S, "all")
    for mode in ("none", "one", "last", "mixed"):
        sel_first, sel = _hess.selection(S["cfg_first"], mode)
        twin, x = _hess.run_surface(S, mode)
        assert np.array_equal(x, S["x0"])
        for j in range(5):
            rows = sel[sel_first[j]: sel_first[j + 1]] - S["cfg_first"][j]
            idx = (3 * rows[:, None] + np.arange(3)).reshape(-1)
            raw = full.matrix(j)[np.ix_(idx, idx)] if len(idx) else np.zeros((0, 0))
            # (the full matrix was symmetrised against other partners only outside the block: inside it the pairs are the same)
            assert np.array_equal(twin.matrix(j), raw), (mode, j)
    # a poisoned force component after a +h call (launch 2 k + 1 harvests it) and after a -h call
    for launch in (7, 8):
        row = int(S["cfg_first"][2]) + 4
        bad, x = _hess.run_surface(S, "all", nan_at=(launch, row, 1))
        assert list(bad.status) == [0, 0, _hess.FAILED, 0, 0] and np.array_equal(x, S["x0"])
        for j in (0, 1, 4):
            assert np.array_equal(bad.matrix(j), full.matrix(j))
        assert not bad.diag[2].any()


def test_the_fixed_order_sums_of_the_twin():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 256, 257, 700):
        v = rng.normal(size=n)
        nt = _hess.threads_of(n)
        got = _hess.segment_total(_hess.thread_sums(v, nt))
        assert abs(got - v.sum()) <= n * EPS * np.abs(v).sum() and nt == (64 if n <= 256 else 256)
    lanes = rng.normal(size=64)                               # the butterfly pairs neighbours, then pairs of pairs, ...
    want = lanes.copy()
    while len(want) > 1:
        want = want[0::2] + want[1::2]
    assert _hess.segment_total(lanes) == want[0]


# ---- modes and the prefactor -------------------------------------------------------------------------------------------------

def _thz(lam):
    return np.sqrt(lam * FTM2V) / (2.0 * np.pi)


def test_modes_of_a_diatomic():
    """two masses on a spring k along x: one vibration with omega^2 = k (1 / m1 + 1 / m2), five zero modes"""
    k, m1, m2 = 3.7, 183.84, 186.207
    H = np.zeros((6, 6))
    H[np.ix_([0, 3], [0, 3])] = k * np.array([[1.0, -1.0], [-1.0, 1.0]])
    for project in (True, False):
        r = modes(H, [m1, m2], project_translations=project)
        nu = r["frequencies"]
        assert r["n_unstable"] == 0 and r["n_zero"] == 5 and np.abs(nu[:5]).max() <= 1e-6
        assert abs(nu[5] - _thz(k * (1.0 / m1 + 1.0 / m2))) <= 1e-12 * nu[5]
        vec = r["eigenvectors"][:, 5] / np.sqrt(np.repeat([m1, m2], 3))          # back to displacements: the centre of mass rests
        assert abs(m1 * vec[0] + m2 * vec[3]) <= 1e-12 * abs(m1 * vec[0])
    # the conversion itself: lambda = 1 eV/(A^2 g/mol) is sqrt(FTM2V) rad/ps
    one = modes(np.eye(3), None, project_translations=False)
    assert np.allclose(one["frequencies"], np.sqrt(FTM2V) / (2.0 * np.pi), rtol=1e-15) and np.allclose(one["eigenvalues"], 1.0)
    assert abs(FTM2V - 1.0 / 1.0364269e-4) <= 1e-12 * FTM2V


def test_modes_of_a_ring_of_equal_masses():
    """N atoms on a ring with springs k along x: omega_q^2 = (4 k / m) sin^2(pi q / N); y and z do not move"""
    N, k, m = 12, 2.5, 95.95
    H = np.zeros((3 * N, 3 * N))
    for j in range(N):
        H[3 * j, 3 * j] += 2.0 * k
        H[3 * j, 3 * ((j + 1) % N)] -= k
        H[3 * j, 3 * ((j - 1) % N)] -= k
    r = modes(H, m)
    want = np.sort(np.concatenate([np.zeros(2 * N), _thz(4.0 * k / m * np.sin(np.pi * np.arange(N) / N) ** 2)]))
    assert np.abs(r["frequencies"] - want).max() <= 1e-6 and r["n_unstable"] == 0 and r["n_zero"] == 2 * N + 1
    assert np.abs(r["frequencies"][2 * N + 1:] - want[2 * N + 1:]).max() <= 1e-12 * want.max()


def test_modes_of_the_surface_saddle_has_one_unstable_mode():
    A, B, C, D, G = [np.array([q]) for q in (0.45, 2.0, 0.6, 1.5, 0.05)]
    M = 30.0
    r = modes(_neb.saddle_hessian(A, B, C, D, G), [M], project_translations=False)
    want = np.array([-_thz(4.0 * A[0] / M), _thz(2.0 * D[0] / M), _thz(2.0 * B[0] / M)])
    assert r["n_unstable"] == 1 and r["n_zero"] == 0 and np.abs(r["frequencies"] - want).max() <= 1e-12 * want.max()
    # a chain of four at their saddles, coupled weakly: four unstable modes, counted as such
    four = modes(_neb.saddle_hessian(*[np.full(4, q[0]) for q in (A, B, C, D, G)]), np.full(4, M), project_translations=False)
    assert four["n_unstable"] == 4
    # zero_tol decides what counts
    assert modes(np.diag([-1e-12, 1.0, 1.0]), 1.0, False)["n_unstable"] == 0
    assert modes(np.diag([-1e-12, 1.0, 1.0]), 1.0, False, zero_tol=0.0)["n_unstable"] == 1


def test_modes_projects_the_three_translations():
    """a random symmetric matrix that knows nothing of translation invariance: after the projection exactly three zero modes,
    and they span the mass-weighted uniform translations"""
    rng = np.random.default_rng(4)
    n = 7
    R = rng.normal(size=(3 * n, 3 * n))
    H = R @ R.T + 3.0 * np.eye(3 * n)
    M = rng.uniform(20.0, 200.0, n)
    raw = modes(H, M, project_translations=False)
    assert raw["n_zero"] == 0 and raw["n_unstable"] == 0
    r = modes(H, M)
    assert r["n_zero"] == 3 and r["n_unstable"] == 0 and np.abs(r["frequencies"][:3]).max() <= 1e-6
    T = np.zeros((3 * n, 3))
    for d in range(3):
        T[d::3, d] = np.sqrt(M)
    T /= np.linalg.norm(T, axis=0)
    zero = r["eigenvectors"][:, np.argsort(np.abs(r["frequencies"]))[:3]]
    assert np.abs(zero @ (zero.T @ T) - T).max() <= 1e-10
    # a matrix that does obey the sum rule (pair springs) keeps its other modes
    K = np.zeros((3 * n, 3 * n))
    for i in range(n):
        for j in range(i + 1, n):
            q = rng.normal(size=(3, 3))
            pair = np.zeros((3, 3 * n))
            pair[:, 3 * i: 3 * i + 3], pair[:, 3 * j: 3 * j + 3] = q, -q
            K += pair.T @ pair
    same = modes(K, 50.0)
    plain = modes(K, 50.0, project_translations=False)
    assert np.abs(np.sort(np.abs(same["frequencies"])) - np.sort(np.abs(plain["frequencies"]))).max() <= 1e-6


def test_modes_refusals():
    for bad in (np.zeros((3, 4)), np.zeros((4, 4)), np.zeros(9), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="modes"):
            modes(bad, 1.0)
    for bad_m in ([1.0, 2.0], 0.0, -1.0, [np.inf]):
        with pytest.raises(ValueError, match="modes"):
            modes(np.eye(3), bad_m)
    with pytest.raises(ValueError, match="modes"):
        modes(np.eye(3), 1.0, zero_tol=-1.0)
    empty = modes(np.zeros((0, 0)), np.zeros(0))
    assert empty["frequencies"].shape == (0,) and empty["n_unstable"] == 0


def test_vineyard_prefactor():
    """a single atom in a well (nu1, nu2, nu3) over a saddle (-nub, mu2, mu3): nu* = nu1 nu2 nu3 / (mu2 mu3); through logarithms
    it holds for a thousand modes whose plain product overflows"""
    lo, hi = np.array([3.0, 4.0, 5.0]), np.array([-2.0, 4.5, 5.5])
    assert abs(vineyard_prefactor(lo, hi) - 60.0 / 24.75) <= 1e-14 * 60.0 / 24.75
    zeros = np.array([0.0, 1e-7, -1e-7])                       # translations on both sides do not count
    assert abs(vineyard_prefactor(np.concatenate([zeros, lo]), np.concatenate([hi, zeros])) - 60.0 / 24.75) <= 1e-14 * 3.0
    big = np.full(1000, 1e3)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.prod(big))
    got = vineyard_prefactor(np.concatenate([big, [7.0]]), np.concatenate([big, [-1.0]]))
    assert abs(got - 7.0) <= 1e-9
    refusals = {
        "no unstable mode at the saddle": (lo, np.array([2.0, 4.5, 5.5])),
        "two unstable modes": (lo, np.array([-2.0, -4.5, 5.5])),
        "an unstable minimum": (np.array([-3.0, 4.0, 5.0]), hi),
        "as many stable modes": (lo, np.array([-2.0, 4.5, 5.5, 6.0])),
        "two stable modes fewer": (lo, np.array([-2.0, 4.5])),
        "not finite": (lo, np.array([-2.0, np.nan, 5.5])),
    }
    for what, (a, b) in refusals.items():
        with pytest.raises(ValueError, match="vineyard_prefactor"):
            vineyard_prefactor(a, b)


# ---- refusals before a device is touched -------------------------------------------------------------------------------------

def test_the_entry_points_refuse_bad_arguments_before_touching_a_pointer():
    """every pointer is a made-up address: a call that got past the checks would crash here"""
    L = capi.lib()
    assert "mtp_hess_step" in capi.EXPORTS and "mtp_hess_finish" in capi.EXPORTS
    p = C.c_void_p(4096)

    def step(stream=p, ncfg=3, sel_max=5, k=0, h=0.01, null=None):
        ptrs = [None if i == null else p for i in range(13)]
        return L.mtp_hess_step(stream, ncfg, ptrs[0], ptrs[1], ptrs[2], sel_max, k, C.c_double(h), *ptrs[3:])

    def finish(stream=p, ncfg=3, null=None):
        ptrs = [None if i == null else p for i in range(8)]
        return L.mtp_hess_finish(stream, ncfg, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 1, *ptrs[4:])

    assert step(stream=None) == -20 and finish(stream=None) == -20
    assert step(ncfg=-1) == -20 and finish(ncfg=-1) == -20
    for h in (0.0, -0.01, float("nan"), float("inf")):
        assert step(h=h) == -20
    assert step(k=-1) == -20 and step(k=31) == -20 and step(sel_max=-1) == -20 and step(sel_max=0, k=1) == -20
    assert step(sel_max=capi.HESS_MAX_SELECTED + 1) == -20
    for i in range(13):
        assert step(null=i) == -20, i
    for i in range(8):
        assert finish(null=i) == -20, i
    assert step(ncfg=0) == 0 and finish(ncfg=0) == 0 and step(ncfg=0, k=30) == 0       # no-op successes


def _stub(max_cutoff=5.0):
    """what hessian_cells reads of a context before it plans: anything past the host checks fails on it with AttributeError"""
    return types.SimpleNamespace(pot=types.SimpleNamespace(info=types.SimpleNamespace(max_cutoff=max_cutoff)))


def test_hessian_cells_refuses_before_it_touches_the_device():
    cfg = _cells.tilted5_cell()
    cases = {
        "h 0": dict(h=0.0), "h < 0": dict(h=-0.01), "h nan": dict(h=float("nan")), "h inf": dict(h=float("inf")),
        "h at half the skin": dict(h=1.0), "h above it": dict(h=1.5),
        "an atom out of range": dict(atoms=[[0, 5]]), "a negative atom": dict(atoms=[[-1]]), "an atom twice": dict(atoms=[[1, 3, 1]]),
        "atoms for two configurations": dict(atoms=[[0], [1]]),
        "a mass of 0": dict(masses=0.0), "a negative mass": dict(masses=[183.84, -1.0]),
        "a Hessian above the limit": dict(max_hessian_bytes=8 * 15 * 15 - 1),
    }
    for what, kw in cases.items():
        with pytest.raises(ValueError, match="hessian_cells") as ei:
            hessian_cells(_stub(), [cfg], **kw)
        print(what, "->", ei.value)
    with pytest.raises(ValueError, match="configuration 1"):
        hessian_cells(_stub(), [cfg, cfg], atoms=[None, [7]])
    with pytest.raises(ValueError, match="configuration 2"):
        hessian_cells(_stub(), [_cells.cubic2_cell(), _cells.cubic2_cell(), cfg], max_hessian_bytes=8 * 15 * 15 - 1)
    for kw in (dict(h=0.999), dict(atoms=[[4, 0]]), dict(max_hessian_bytes=8 * 15 * 15)):     # just inside: past the host checks
        with pytest.raises(AttributeError):
            hessian_cells(_stub(), [cfg], **kw)


def test_the_pass_cut_respects_max_hessian_bytes():
    batch = [_cells.tilted5_cell(), _cells.cubic2_cell(), _cells.primitive_cell(), _cells.tilted5_cell(), _cells.cubic2_cell(),
             (np.zeros((0, 3)), _cells.CUBIC.copy(), np.zeros(0, dtype=np.int32)), _cells.tilted5_cell()]
    cells, natoms = np.array([c for _, c, _ in batch]), np.array([len(p) for p, _, _ in batch])
    nsel = natoms.copy()
    nsel[3] = 2                                                # a partial selection counts with its own size
    size = 8 * (3 * nsel) ** 2
    plan = plan_cell_passes(cells, natoms, 7.0)[0]
    assert [(a, b) for a, b, _ in cut_hessian_passes(plan, cells, nsel, 7.0)] == [(0, len(batch))]
    assert cut_hessian_passes(plan, cells, nsel, 7.0)[0][2] is plan[0][2]
    cut_somewhere = 0
    for limit in (int(size.max()), int(size.max()) + 1, 2000, 2500, 3000, 4000, int(size.sum()) - 1, int(size.sum())):
        for cap in (None, 6, 8):
            plain = plan_cell_passes(cells, natoms, 7.0, cap)[0]
            got = cut_hessian_passes(plain, cells, nsel, 7.0, limit)
            spans = [(a, b) for a, b, _ in got]
            print("max_hessian_bytes %d, max_atoms_per_pass %r: %r" % (limit, cap, spans))
            assert spans[0][0] == 0 and spans[-1][1] == len(batch) and all(b > a for a, b in spans)
            assert all(a1 == b0 for (_, b0), (a1, _) in zip(spans, spans[1:]))
            assert all(int(size[a:b].sum()) <= limit for a, b in spans)
            assert {a for a, _, _ in plain} <= {a for a, _ in spans}                   # the cuts of the atoms stay
            for a, b in spans:                                                         # greedy: a pass ends only where it must
                if b < len(batch) and b not in {p for p, _, _ in plain}:
                    assert int(size[a: b + 1].sum()) > limit
            for a, b, lay in got:
                assert lay["origins"].shape == (b - a, 3)
            cut_somewhere += len(spans) > len(plain)
    assert cut_somewhere > 0
    with pytest.raises(ValueError, match="configuration 0"):
        cut_hessian_passes(plan, cells, nsel, 7.0, int(size.max()) - 1)
