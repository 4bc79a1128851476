"""The batched symmetric eigen-solver on the device (mtp_eigh_batched, md.modes_cells, md.hessian_cells(modes=True)).  The kernel
alone against the numpy twin of tests/_eigh.py BIT FOR BIT over one ragged batch that carries every size and tier edge, with one
sentinel element behind every array: with and without mass roots and projection, the statuses, batch independence, failures that
stay at home, argument errors.  Then the device results against LAPACK within the bounds of tests/test_eigh_cpu.py, modes_cells
against md.modes, and relax_cells -> hessian_cells(modes=True) end to end over two potentials."""
import functools
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, md

import _batch
import _cells
import _eigh
from _cells import LIST_CUTOFF, POT

SENTINEL = -77.0
WITH_VECTORS = (0, 1, 2, 3, 6, 45, 48, 49, 51, 96, 99, 193)      # 99 and 193: above what the tiers serve with vectors
WITHOUT_VECTORS = (97, 162, 192, 193)
MASSES = {1: np.array([183.84]), 2: np.array([183.84, 186.207])}
H_STEP = 0.01


def _matrices(sizes, seed=2):
    """a random symmetric matrix and mass roots (in triples where the size allows) per size; draws depend on (seed, position)"""
    mats, roots = [], []
    for k, N in enumerate(sizes):
        rng = np.random.default_rng([seed, k])
        B = rng.standard_normal((N, N)) * 30.0
        mats.append(B + 0.25 * B.T)                               # (not symmetric: the load symmetrises)
        r = np.sqrt(rng.uniform(20.0, 200.0, (N + 2) // 3))
        roots.append(np.repeat(r, 3)[:N])
    return mats, roots


def _device(mats, roots=None, project=False, vectors=True, max_sweeps=30, status=None, stream="own", drop=None):
    """mtp_eigh_batched over the ragged batch `mats`; every array has one element (one matrix) more than the batch, filled with a
    sentinel like the outputs themselves.  Returns dict(W, V, info, status: per matrix, as numpy)."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream if stream == "own" else stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sizes = np.array([len(A) for A in mats], dtype=np.int64)
    nmat = len(mats)
    af, wf = np.concatenate([[0], np.cumsum(sizes ** 2)]), np.concatenate([[0], np.cumsum(sizes)])
    A_t = to(np.concatenate([np.asarray(A, dtype=np.float64).reshape(-1) for A in mats] + [np.full(1, SENTINEL)]))
    T = dict(n=to(sizes.astype(np.int32)), a_first=to(af[:-1].astype(np.int64)), A=A_t, w_first=to(wf[:-1].astype(np.int64)),
             root=None if roots is None else to(np.concatenate(list(roots) + [np.full(1, SENTINEL)])),
             W=torch.full((int(wf[-1]) + 1,), SENTINEL, dtype=torch.float64, device=dev),
             V=torch.full((int(af[-1]) + 1,), SENTINEL, dtype=torch.float64, device=dev) if vectors else None,
             info=torch.full((nmat + 1, 2), SENTINEL, dtype=torch.float64, device=dev),
             status=to(np.concatenate([np.zeros(nmat) if status is None else status, [int(SENTINEL)]]).astype(np.int32)))
    if drop:
        T[drop] = None
    before = {k: v.clone() for k, v in T.items() if v is not None}
    # (the wrapper counts the matrices on n: the batch's own count goes in, not the padded one)
    rc = capi.lib().mtp_eigh_batched(capi._st(st) if st is not None else None, nmat, *[capi._ptr(T[k]) for k in ("n", "a_first", "A", "w_first", "root")],
                                     int(project), int(max_sweeps), *[capi._ptr(T[k]) for k in ("W", "V", "info", "status")])
    torch.cuda.synchronize()
    if rc:
        for k, v in before.items():
            assert torch.equal(T[k], v), k                        # an argument error launches nothing
        return rc
    assert torch.equal(T["A"].view(torch.int64), before["A"].view(torch.int64))         # the matrices are only read (bits: one may hold a NaN)
    W, info, sh = T["W"].cpu().numpy(), T["info"].cpu().numpy(), T["status"].cpu().numpy()
    V = T["V"].cpu().numpy() if vectors else None
    assert W[wf[-1]] == SENTINEL and (info[nmat] == SENTINEL).all() and sh[nmat] == int(SENTINEL)
    assert V is None or V[af[-1]] == SENTINEL
    return dict(W=[W[wf[j]: wf[j + 1]] for j in range(nmat)],
                V=[V[af[j]: af[j + 1]].reshape(sizes[j], sizes[j]) if vectors else None for j in range(nmat)],
                info=[info[j] for j in range(nmat)], status=sh[:nmat])


def _same_bits(have, want):
    have, want = np.ascontiguousarray(have, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    nan = np.isnan(want)                                          # (a poisoned number: NaN where the twin has NaN, whatever its payload)
    return have.shape == want.shape and np.array_equal(np.isnan(have), nan) and \
        np.array_equal(have[~nan].view(np.int64), want[~nan].view(np.int64))


def _untouched(got, j):
    return (got["W"][j] == SENTINEL).all() and (got["info"][j] == SENTINEL).all() and \
        (got["V"][j] is None or (got["V"][j] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _twin(sizes, k, with_root, project, vectors, max_sweeps=30):
    mats, roots = _matrices(sizes)
    return _eigh.solve(mats[k], roots[k] if with_root else None, project, max_sweeps=max_sweeps, vectors=vectors)


def _assert_twin(got, sizes, with_root, project, vectors, what):
    limit = _eigh.MAX_N_VECTORS if vectors else _eigh.MAX_N
    for k, N in enumerate(sizes):
        if N == 0:
            assert got["status"][k] == 0 and (got["info"][k] == SENTINEL).all(), (what, N)
            continue
        if N > limit:
            assert got["status"][k] == _eigh.TOO_LARGE and _untouched(got, k), (what, N)
            continue
        want = _twin(sizes, k, with_root, project, vectors)
        assert got["status"][k] == want["status"], (what, N, got["status"][k])
        for key in ("W", "V", "info") if vectors else ("W", "info"):
            same = _same_bits(got[key][k], want[key])
            if not same:
                print("%s: N = %d: %s differs, worst %.3e" % (what, N, key, float(np.nanmax(np.abs(got[key][k] - want[key])))))
            assert same, (what, N, key)
        if project and N % 3:
            assert want["status"] == _eigh.FAILED, (what, N)


# ---- mtp_eigh_batched alone --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("with_root,project", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "root", "project", "root_project"])
def test_kernel_equals_the_twin_bit_for_bit(with_root, project):
    for sizes, vectors in ((WITH_VECTORS, True), (WITHOUT_VECTORS, False)):
        mats, roots = _matrices(sizes)
        got = _device(mats, roots if with_root else None, project, vectors)
        _assert_twin(got, sizes, with_root, project, vectors, "vectors" if vectors else "values")
    # the sizes of the first two tiers without vectors take the other instantiations: the same eigenvalues and info
    sizes = WITH_VECTORS[:10]
    mats, roots = _matrices(sizes)
    got = _device(mats, roots if with_root else None, project, False)
    for k, N in enumerate(sizes):
        if N:
            want = _twin(sizes, k, with_root, project, True)
            assert got["status"][k] == want["status"] and _same_bits(got["W"][k], want["W"]) and _same_bits(got["info"][k], want["info"]), N


@pytest.mark.gpu
def test_seven_matrices_alone_have_the_bits_they_have_inside_a_batch_of_300():
    rng = np.random.default_rng(8)
    sizes = tuple(int(s) for s in rng.choice([1, 2, 3, 5, 6, 12, 24, 45, 48, 49, 60], 300))
    which = [0, 41, 97, 150, 203, 256, 299]
    sizes = tuple(96 if k == 150 else 48 if k == 0 else s for k, s in enumerate(sizes))
    mats, roots = _matrices(sizes, seed=9)
    batch = _device(mats, roots, False, True)
    alone = _device([mats[k] for k in which], [roots[k] for k in which], False, True)
    assert (batch["status"] == 0).all()
    for i, k in enumerate(which):
        for key in ("W", "V", "info"):
            assert _same_bits(alone[key][i], batch[key][k]), (k, key)
        assert np.abs(batch["W"][k]).max() > 1e-3


@pytest.mark.gpu
def test_a_poisoned_entry_fails_its_matrix_only_and_a_marked_matrix_is_skipped():
    sizes = (6, 48, 45, 51, 3)
    mats, _ = _matrices(sizes, seed=4)
    clean = _device(mats)
    bad = [A.copy() for A in mats]
    bad[2][7, 31] = np.nan
    entry = np.array([0, 0, 0, 5, 0])
    got = _device(bad, status=entry)
    assert list(got["status"]) == [0, 0, _eigh.FAILED, 5, 0]
    assert np.isnan(got["W"][2]).all() and np.isnan(got["V"][2]).all() and np.isnan(got["info"][2]).all()
    assert _untouched(got, 3)
    for j in (0, 1, 4):
        for key in ("W", "V", "info"):
            assert _same_bits(got[key][j], clean[key][j]), (j, key)
    # an infinite mass root fails like an entry
    roots = [np.ones(N) for N in sizes]
    roots[1][5] = np.inf
    got = _device(mats, roots)
    assert list(got["status"]) == [0, _eigh.FAILED, 0, 0, 0] and np.isnan(got["W"][1]).all()


@pytest.mark.gpu
def test_one_sweep_of_a_random_48_is_not_converged_and_equals_the_twin_after_one_sweep():
    sizes = (48,)
    mats, _ = _matrices(sizes)
    got = _device(mats, max_sweeps=1)
    want = _twin(sizes, 0, False, False, True, 1)
    assert got["status"][0] == want["status"] == _eigh.NOT_CONVERGED and got["info"][0][0] == 1.0 and got["info"][0][1] > 0.0
    for key in ("W", "V", "info"):
        assert _same_bits(got[key][0], want[key]), key


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    mats, roots = _matrices((6, 3))
    assert _device(mats, stream=None) == -20
    assert _device(mats, max_sweeps=0) == -20
    for key in ("n", "a_first", "A", "w_first", "W", "info", "status"):
        assert _device(mats, roots, drop=key) == -20, key
    with pytest.raises(capi.MtpError) as ei:
        import torch
        z = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        capi.eigh_batched(z, None, None, None, None, False, 30, None, None, None, z, stream=capi.use_private_torch_stream(z.device).cuda_stream)
    assert ei.value.code == -20
    assert isinstance(_device([], vectors=False), dict)           # nmat = 0: MTP_OK, nothing written


# ---- the device against LAPACK -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _unscaled(N):
    return _eigh.solve(_eigh.family("random", N)[0], vectors=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _eigh.FAMILIES + ("scaled_up", "scaled_down"))
def test_device_against_lapack(name):
    """the bounds of tests/test_eigh_cpu.py, for the device's own results: |lambda - lambda_lapack| and max |A V - V Lambda| <=
    8 N eps |A|_F, max |V^T V - I| <= 16 N eps, at most 30 sweeps; A is the prepared matrix.  Eigenvectors up to N = 96."""
    scale = {"scaled_up": 2.0 ** 100, "scaled_down": 2.0 ** -100}.get(name, 1.0)
    fam = "random" if name.startswith("scaled") else name
    worst = np.zeros(3)
    for vectors in (True, False):
        sizes = [N for N in _eigh.SIZES if (N <= _eigh.MAX_N_VECTORS) == vectors]
        cases = [_eigh.family(fam, N) for N in sizes]
        project = cases[0][2]
        got = _device([A * scale for A, _, _ in cases], [r for _, r, _ in cases] if cases[0][1] is not None else None, project, vectors)
        assert (got["status"] == 0).all(), name
        for k, (A, root, _) in enumerate(cases):
            prepared = _eigh.prepare(A * scale, root, project)
            prepared = prepared + np.tril(prepared, -1).T
            r = np.array(_eigh.ratios(prepared, got["W"][k], got["V"][k]))
            worst[: len(r)] = np.maximum(worst[: len(r)], r)
            assert got["info"][k][0] <= 30 and (np.diff(got["W"][k]) >= 0.0).all(), (name, sizes[k])
            assert (r <= np.array(_eigh.BOUNDS)[: len(r)]).all(), (name, sizes[k], r)
            if name.startswith("scaled"):                         # a power of two scales the eigenvalues exactly
                assert _same_bits(got["W"][k], _unscaled(sizes[k])["W"] * scale), (name, sizes[k])
    print("%s on the device: worst ratios %.2f %.2f %.2f (bounds 8, 8, 16)" % (name, worst[0], worst[1], worst[2]))


# ---- md.modes_cells ----------------------------------------------------------------------------------------------------------

def _assert_modes(got, H, masses, project, zero_tol, what):
    """against md.modes on the same matrix: every eigenvalue within 8 N eps |D|_F, the counts equal, the frequencies the same
    expression of lambda.  D is the mass-weighted, symmetrised matrix BEFORE the projection: the two paths prepare P D P each in
    its own order, with rounding errors that are proportional to |D|_F (tests/test_eigh_cpu.py, (d)), whatever is left of D
    afterwards -- of a single atom, nothing but those errors.  Without projection D is the prepared matrix itself."""
    want = md.modes(H, masses, project, zero_tol)
    N = len(H)
    lam = want["eigenvalues"]
    D = np.asarray(H, dtype=np.float64)
    if masses is not None and N:
        root = np.repeat(np.sqrt(np.full(N // 3, masses) if np.ndim(masses) == 0 else np.asarray(masses, dtype=np.float64)), 3)
        D = D / np.outer(root, root)
    bound = 8.0 * N * _eigh.EPS * float(np.linalg.norm(0.5 * (D + D.T))) if N else 0.0
    err = float(np.abs(got["eigenvalues"] - lam).max()) if N else 0.0
    print("%s: N = %d, solver %s, |d lambda| %.3e (bound %.3e)" % (what, N, got["solver"], err, bound))
    assert err <= bound, what
    assert got["n_unstable"] == want["n_unstable"] and got["n_zero"] == want["n_zero"], what
    nu = np.sign(got["eigenvalues"]) * np.sqrt(np.abs(got["eigenvalues"]) * md.FTM2V) / (2.0 * np.pi)
    assert np.array_equal(got["frequencies"], nu), what
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("vectors", [False, True])
def test_modes_cells_against_modes(vectors):
    sizes = (3, 6, 48, 0, 99, 162, 195)
    rng = np.random.default_rng(3)
    mats = [_eigh.random_symmetric(N, 20 + N) * 40.0 for N in sizes]
    masses = [rng.uniform(20.0, 200.0, N // 3) for N in sizes]
    masses[1] = 55.0
    got = md.modes_cells(mats, masses, vectors=vectors)
    limit = capi.EIGH_MAX_N_VECTORS if vectors else capi.EIGH_MAX_N
    for j, N in enumerate(sizes):
        _assert_modes(got[j], mats[j], masses[j], True, 1e-3, "modes_cells")
        assert got[j]["solver"] == ("host" if N > limit else "device") and got[j]["status"] == "ok"
        assert got[j]["sweeps"] >= (1 if 0 < N <= limit else 0)
        if N:
            assert got[j]["n_zero"] >= 3
        if vectors:
            V, A = got[j]["eigenvectors"], None
            assert V.shape == (N, N)
            if 0 < N <= limit:
                root = np.repeat(np.sqrt(np.full(N // 3, masses[j]) if np.ndim(masses[j]) == 0 else masses[j]), 3)
                A = _eigh.prepare(mats[j], root, True)
                A = A + np.tril(A, -1).T
                r = _eigh.ratios(A, got[j]["eigenvalues"], V)
                assert r[1] <= 8.0 and r[2] <= 16.0, (N, r)
        else:
            assert got[j]["eigenvectors"] is None
    # already weighted, no projection, one number for all
    plain = md.modes_cells(mats[:3], None, project_translations=False)
    for j in range(3):
        _assert_modes(plain[j], mats[j], None, False, 1e-3, "weighted")
    one = md.modes_cells(mats[:3], 100.0)
    for j in range(3):
        _assert_modes(one[j], mats[j], 100.0, True, 1e-3, "one mass")
    capped = md.modes_cells([mats[2]], None, max_sweeps=1)[0]
    assert capped["status"] == "not converged" and capped["sweeps"] == 1 and capped["solver"] == "device"


# ---- hessian_cells(modes=True) ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ctx(fname):
    return capi.Context(capi.Potential(os.path.join(POT, fname)), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species,which", [("W_L8.mtp", 1, "cubic2"), ("WRe_L20.mtp", 2, "tilted5")])
def test_relax_then_hessian_with_modes_end_to_end(fname, species, which):
    cfg = _cells.cubic2_cell() if which == "cubic2" else _cells.tilted5_cell(species)
    ctx = _ctx(fname)
    relaxed = md.relax_cells(ctx, [cfg], 2000, ftol=1e-6, masses=MASSES[species], list_cutoff=LIST_CUTOFF)["final"][0]
    assert relaxed["status"] == "converged"                       # (otherwise the test's inputs are wrong)
    masses = MASSES[species][np.asarray(cfg[2]) - 1]
    n = len(cfg[0])
    for vectors in (False, True):
        r = md.hessian_cells(ctx, [(relaxed["x"], cfg[1], cfg[2])], h=H_STEP, masses=MASSES[species], list_cutoff=LIST_CUTOFF,
                             modes=True, vectors=vectors)[0]
        assert r["status"] == "ok" and r["modes_status"] == "ok" and r["solver"] == "device"
        got = dict(r, status=r["modes_status"])
        want = _assert_modes(got, r["hessian"], masses, True, 1e-3, fname)
        assert r["n_unstable"] == 0 and r["n_zero"] == 3
        assert (r["eigenvectors"] is None) == (not vectors)
        if vectors:
            V = r["eigenvectors"]
            assert V.shape == (3 * n, 3 * n) and np.abs(V.T @ V - np.eye(3 * n)).max() <= 16.0 * 3 * n * _eigh.EPS
        if which == "cubic2":
            print("W_L8 cubic2: frequencies [THz] %s" % np.array2string(r["frequencies"], precision=4))
            assert np.abs(r["frequencies"][3:] - 1.94).max() < 0.01 and np.abs(want["frequencies"][3:] - 1.94).max() < 0.01


@pytest.mark.gpu
def test_mixed_batch_with_modes(monkeypatch):
    """the mixed batch (1, 2, 5, 0, 8, 54 atoms): the 54-atom member is above the tier that keeps eigenvectors and goes to the host
    with them, to the device without; a Hessian that failed keeps modes_status "failed" and NaN frequencies, its neighbours are
    solved as ever.  The failure is the one mtp_hess_step marks: status 1 on the device at the end of the pass."""
    fname, species = "WRe_L20.mtp", 2
    batch = _batch.mixed_batch(species)
    ctx = _ctx(fname)
    mass = lambda j: MASSES[species][np.asarray(batch[j][2]) - 1] if len(batch[j][0]) else None
    got = md.hessian_cells(ctx, batch, h=H_STEP, masses=MASSES[species], list_cutoff=LIST_CUTOFF, modes=True, vectors=True)
    for j, (pos, _, _) in enumerate(batch):
        r = got[j]
        assert r["status"] == "ok" and r["modes_status"] == "ok"
        assert r["solver"] == ("host" if len(pos) == 54 else "device"), j
        _assert_modes(dict(r, status=r["modes_status"]), r["hessian"], mass(j), True, 1e-3, "mixed %d" % j)
        assert len(r["frequencies"]) == 3 * len(pos) and r["eigenvectors"].shape == (3 * len(pos), 3 * len(pos))

    real = md._hessian_pass

    def failing(run, setup, selections, h, mass_weight, status):
        hp = real(run, setup, selections, h, mass_weight, status)
        status[2] = 1
        return hp

    monkeypatch.setattr(md, "_hessian_pass", failing)
    got = md.hessian_cells(ctx, batch, h=H_STEP, masses=MASSES[species], list_cutoff=LIST_CUTOFF, modes=True)
    assert got[2]["status"] == "failed" and got[2]["modes_status"] == "failed" and got[2]["solver"] == "device"
    assert np.isnan(got[2]["frequencies"]).all() and np.isnan(got[2]["eigenvalues"]).all() and len(got[2]["frequencies"]) == 15
    for j in (0, 1, 3, 4, 5):
        r = got[j]
        assert r["modes_status"] == "ok" and r["solver"] == "device" and r["eigenvectors"] is None, j
        _assert_modes(dict(r, status="ok"), r["hessian"], mass(j), True, 1e-3, "beside a failure %d" % j)


@pytest.mark.gpu
def test_partial_selections_are_not_projected_and_weighted_hessians_need_no_roots():
    """project_translations=None projects the full selections only -- a pass that mixes both is solved in two launches --, and
    with mass_weight the Hessian is weighted already: modes() with masses None is the reference"""
    fname, species = "WRe_L20.mtp", 2
    batch = _batch.mixed_batch(species)[:5]
    atoms = [None, None, [4, 1], None, [3, 0, 5]]
    got = md.hessian_cells(_ctx(fname), batch, h=H_STEP, atoms=atoms, masses=MASSES[species], list_cutoff=LIST_CUTOFF, modes=True,
                           mass_weight=True)
    for j, r in enumerate(got):
        _assert_modes(dict(r, status=r["modes_status"]), r["hessian"], None, atoms[j] is None, 1e-3, "weighted %d" % j)
        assert r["modes_status"] == "ok" and r["solver"] == "device"
    assert got[4]["n_zero"] == 0 and len(got[4]["frequencies"]) == 9 and got[1]["n_zero"] == 3
    forced = md.hessian_cells(_ctx(fname), batch[:2], h=H_STEP, masses=MASSES[species], list_cutoff=LIST_CUTOFF, modes=True,
                              project_translations=False)
    for j, r in enumerate(forced):
        _assert_modes(dict(r, status=r["modes_status"]), r["hessian"], MASSES[species][np.asarray(batch[j][2]) - 1], False, 1e-3, "forced %d" % j)
