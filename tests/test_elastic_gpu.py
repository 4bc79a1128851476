"""Batched elastic constants on the device (md.elastic_cells; mtp_elastic_step, mtp_elastic_finish, mtp_elastic_relax).  The
first two kernels alone against the numpy twin of tests/_elastic.py BIT FOR BIT, with forces and per-atom energies of the
analytic surface of tests/_neb.py and a made-up virial computed by torch between the launches (the twin is handed the very
numbers the kernel saw): every segment size and workgroup filling, batch independence, failures that stay at home, argument
errors.  mtp_elastic_relax alone on hand-made Hessians within Cholesky's backward error bound.  Then whole runs over two
potentials against the host-driven loop (md.evaluate_cells on every explicitly strained copy) and against the CPU oracle, within
the project's parity bounds divided by the step, and relax_cells_vc -> elastic_cells -> moduli end to end."""
import functools
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, md

import _batch
import _cells
import _elastic
import _hess
import _neb
from _cells import LIST_CUTOFF, POT

SENTINEL = -77.0
SIZES = (1, 2, 5, 0, 8, 54, 256, 257)         # 257: the first segment above MTP_BATCH_WAVE_ROWS, served by a whole workgroup
H_STRAIN = 0.005
EYE9 = np.eye(3).reshape(9)


# ---- mtp_elastic_step and mtp_elastic_finish alone ---------------------------------------------------------------------------

def _geometry(S, seed=1):
    """slot origins [ncfg, 3] and cells h0 [ncfg, 9] for the batch S, drawn per configuration in order (a configuration's draws
    do not depend on the batch around it for equal `seed` and position: _sub takes them along)"""
    rng = np.random.default_rng(seed)
    ncfg = len(S["cfg_first"]) - 1
    origins = rng.uniform(-30.0, 30.0, (ncfg, 3))
    h0 = np.array([(_neb.TRICLINIC * rng.uniform(0.8, 1.2)).reshape(9) for _ in range(ncfg)])
    return origins, h0


def _sub(S, G, which):
    return _hess.sub_batch(S, which), (G[0][list(which)], G[1][list(which)])


def _device_pass(S, G, h=H_STRAIN, nan_at=None, with_twin=True):
    """mtp_elastic_step for launches 0 .. 12 and mtp_elastic_finish over the batch S with the geometry G; eatom and forces are the
    surface's, the virial of configuration j is a fixed elementwise function of its first and last row, all by torch between
    the launches.  One row (one element, one configuration) more than the batch holds is allocated in every array and filled
    with a sentinel.  With `with_twin` the twin is stepped along on the numbers of every launch, copied back.  Returns the
    device's arrays (numpy) and the twin."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pad = lambda a, fill: np.concatenate([a, np.full((1,) + a.shape[1:], fill, dtype=a.dtype)])
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=dev)
    cf = np.asarray(S["cfg_first"], dtype=np.int64)
    ncfg, n = len(cf) - 1, int(cf[-1])
    origins, h0 = G
    twin = _elastic.Twin(cf, h)
    consts = [to(pad(S[k], 0.0)) for k in _neb.SURFACE_KEYS]
    xt0 = S["x0"] - np.repeat(origins, np.diff(cf), axis=0)
    x, xt = to(pad(S["x0"], SENTINEL)), to(pad(xt0, SENTINEL))
    x0 = x.clone()
    A = dict(cfg_first=to(cf.astype(np.int32)), c_first=to(pad(18 * cf[:-1], -1)), origins=to(pad(origins, SENTINEL)),
             h0=to(pad(h0, SENTINEL)), T=full(ncfg + 1, 9), Bt=torch.zeros(ncfg + 1, 36, dtype=torch.float64, device=dev), B=full(ncfg + 1, 36),
             C=full(ncfg + 1, 36), coupling=torch.zeros(18 * n + 1, dtype=torch.float64, device=dev), f0=full(n + 1, 3),
             fmax=torch.zeros(ncfg + 1, dtype=torch.float64, device=dev), energy=torch.zeros(ncfg + 1, dtype=torch.float64, device=dev),
             stress0=full(ncfg + 1, 6), status=torch.zeros(ncfg + 1, dtype=torch.int32, device=dev), diag=full(ncfg + 1, 2))
    A["Bt"][ncfg], A["coupling"][18 * n] = SENTINEL, SENTINEL
    for key in ("fmax", "energy", "status"):
        A[key][ncfg] = SENTINEL
    lo = to(np.minimum(cf[:-1], max(n - 1, 0)))
    hi = to(np.clip(cf[1:] - 1, 0, max(n - 1, 0)))
    xh, xh0 = S["x0"].copy(), S["x0"].copy()
    for k in range(13):
        e, f = _neb.surface(torch, x, *consts)
        W = torch.cat([x[lo] * f[hi] + 0.25 * f[lo], 3.0 * x[hi] * x[lo] - f[hi] * f[lo]], 1) if n else torch.zeros(ncfg, 6, dtype=torch.float64, device=dev)
        if nan_at is not None and nan_at[0] == k:
            (f if nan_at[1] == "f" else W)[nan_at[2], nan_at[3]] = float("nan")
        capi.elastic_step(A["cfg_first"], k, h, x, x0, xt, A["origins"], A["h0"], f, e, W, A["T"], A["Bt"], A["coupling"], A["c_first"],
                          A["f0"], A["fmax"], A["energy"], A["stress0"], A["status"], stream=st)
        if with_twin:
            twin.step(k, xh, xh0, xt0, origins, h0, f.cpu().numpy()[:n], W.cpu().numpy(), eatom=e.cpu().numpy()[:n])
    capi.elastic_finish(A["cfg_first"], A["c_first"], A["coupling"], A["stress0"], A["Bt"], A["B"], A["C"], A["diag"], A["status"], stream=st)
    twin.finish()
    torch.cuda.synchronize()
    got = {k: A[k].cpu().numpy() for k in ("T", "Bt", "B", "C", "coupling", "f0", "fmax", "energy", "stress0", "status", "diag")}
    got["x"] = x.cpu().numpy()
    # nothing behind the last row, element or configuration, and after launch 12 the positions are the saved ones to the bit
    assert got["coupling"][18 * n] == SENTINEL and (got["f0"][n] == SENTINEL).all() and (got["x"][n] == SENTINEL).all()
    for key in ("T", "Bt", "B", "C", "stress0", "diag", "fmax", "energy"):
        assert (got[key][ncfg] == SENTINEL).all(), key
    assert got["status"][ncfg] == int(SENTINEL)
    assert np.array_equal(got["x"][:n], S["x0"])
    if with_twin:
        assert np.array_equal(xh, S["x0"])
    return got, twin


def _assert_bits(got, twin, what):
    ncfg, n = twin.ncfg, len(twin.f0)
    live = np.array([twin.first[j + 1] > twin.first[j] for j in range(ncfg)])
    ok = live & (twin.status == 0)
    pairs = [("coupling", got["coupling"][: 18 * n], twin.coupling), ("Bt", got["Bt"][:ncfg].reshape(ncfg, 6, 6), twin.Bt),
             ("f0", got["f0"][:n], twin.f0), ("fmax", got["fmax"][:ncfg], twin.fmax), ("energy", got["energy"][:ncfg], twin.energy),
             ("stress0", got["stress0"][:ncfg][live], twin.stress0[live]), ("T", got["T"][:ncfg][live], twin.T[live]),
             ("B", got["B"][:ncfg].reshape(ncfg, 6, 6)[ok], twin.B[ok]), ("C", got["C"][:ncfg].reshape(ncfg, 6, 6)[ok], twin.C[ok]),
             ("diag", got["diag"][:ncfg][ok], twin.diag[ok])]
    for key, have, want in pairs:
        have, want = np.ascontiguousarray(have), np.ascontiguousarray(want)
        nan = np.isnan(want)                                  # (a poisoned number: NaN where the twin has NaN, whatever its payload)
        same = np.array_equal(np.isnan(have), nan) and np.array_equal(have[~nan].view(np.int64), want[~nan].view(np.int64))
        if not same:
            print("%s: %s differs, worst %.3e" % (what, key, float(np.nanmax(np.abs(have - want)))))
        assert same, (what, key)
    assert np.array_equal(got["status"][:ncfg], twin.status), what
    # what is skipped is not written: an empty or failed configuration keeps the sentinel in B, C and diag
    for key in ("B", "C", "diag"):
        assert (got[key][:ncfg][~ok] == SENTINEL).all(), key


@functools.lru_cache(maxsize=None)
def _surface(sizes=SIZES, seed=3):
    return _hess.surface_batch(sizes, seed=seed)


@pytest.mark.gpu
def test_kernels_alone_equal_the_twin_bit_for_bit():
    """configurations of 1, 2, 5, 0, 8, 54, 256 and 257 rows in one batch (two workgroups): Bt, B, C, the coupling, T, f0, fmax,
    energy, stress, status and the two diagnostics have the twin's bits; x == x0 to the bit after launch 12 (in _device_pass)"""
    S = _surface()
    got, twin = _device_pass(S, _geometry(S))
    _assert_bits(got, twin, "sizes %r" % (SIZES,))
    assert not twin.status.any() and (twin.fmax[[0, 1, 2, 4, 5, 6, 7]] > 0.0).all() and twin.fmax[3] == 0.0
    live = [0, 1, 2, 4, 5, 6, 7]
    assert np.array_equal(got["T"][live], np.tile(EYE9, (7, 1))) and (got["T"][3] == SENTINEL).all()
    print("asymmetry %s\nsum rule %s" % (twin.diag[:, 0], twin.diag[:, 1]))
    assert (np.abs(twin.B[live]).max((1, 2)) > 1e-3).all() and (twin.diag[live, 1] > 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(8,), (257,), (1, 2, 5, 8), (1, 2, 5, 0, 8)], ids=lambda s: "ncfg%d_%d" % (len(s), s[0]))
def test_kernels_alone_with_one_four_and_five_configurations(sizes):
    """ncfg = 1, 4 and 5: a workgroup's four wavefronts are once partly idle, once all busy, and once a second workgroup has
    one busy wavefront; a batch that is one long segment"""
    S = _surface(sizes, 7)
    got, twin = _device_pass(S, _geometry(S, 2))
    _assert_bits(got, twin, repr(sizes))
    assert not twin.status.any()


@pytest.mark.gpu
def test_a_configuration_alone_has_the_bits_it_has_inside_a_batch_of_300():
    sizes = tuple([(1, 2, 5, 0, 8, 3)[j % 6] for j in range(295)] + [54, 1, 2, 5] + [257])
    S = _surface(sizes, 11)
    G = _geometry(S, 3)
    batch, twin = _device_pass(S, G, with_twin=False)
    for j in (0, 4, 7, 155, 296, 295, 299):
        S1, G1 = _sub(S, G, [j])
        alone, _ = _device_pass(S1, G1, with_twin=False)
        r0, r1 = int(S["cfg_first"][j]), int(S["cfg_first"][j + 1])
        assert np.array_equal(alone["coupling"][:-1], batch["coupling"][18 * r0: 18 * r1]), j
        assert np.array_equal(alone["f0"][:-1], batch["f0"][r0:r1])
        for key in ("Bt", "B", "C", "stress0", "fmax", "energy", "diag", "status", "T"):
            assert np.array_equal(alone[key][0], batch[key][j]), (j, key)
        print("configuration %d (%d rows): the same bits alone" % (j, r1 - r0))
    assert np.abs(batch["B"][:-1][np.diff(S["cfg_first"]) > 0]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("launch,what", [(0, "f"), (0, "w"), (1, "f"), (1, "w"), (2, "f"), (2, "w")],
                         ids=["f0", "w0", "f_after_plus_h", "w_after_plus_h", "f_after_minus_h", "w_after_minus_h"])
def test_a_poisoned_force_or_virial_fails_its_configuration_only(launch, what):
    """one NaN in a force component or in a virial component of the 8-atom configuration in front of launch 0 (the unstrained
    call), launch 1 (which harvests the +h call) or launch 2 (the -h call): its status is "failed" from then on, nothing more of
    it is written, its positions are back at x0 and its T at I; every other configuration has the bits of the clean run"""
    S = _surface((5, 3, 8, 0, 6, 70, 257), 13)
    G = _geometry(S, 4)
    clean, _ = _device_pass(S, G, with_twin=False)
    nan_at = (launch, "f", int(S["cfg_first"][2]) + 4, 1) if what == "f" else (launch, "w", 2, 3)
    got, twin = _device_pass(S, G, nan_at=nan_at)
    _assert_bits(got, twin, "poisoned at launch %d" % launch)
    assert list(twin.status) == [0, 0, _elastic.FAILED, 0, 0, 0, 0]
    assert np.array_equal(got["T"][2], EYE9)
    for j in (0, 1, 4, 5, 6):
        for key in ("Bt", "B", "C", "diag", "stress0"):
            assert np.array_equal(got[key][j], clean[key][j]), (j, key)
    r0, r1 = int(S["cfg_first"][2]), int(S["cfg_first"][3])
    mine, bt = got["coupling"][18 * r0: 18 * r1].reshape(6, 24), got["Bt"][2].reshape(6, 6)
    # in front of launch 2 row 0 is there as parked by launch 1; otherwise nothing of the configuration was ever written
    parked = 1 if launch == 2 else 0
    assert not mine[parked:].any() and not bt[parked:].any() and (mine[:parked].any() or not parked)
    others = np.r_[0: 18 * r0, 18 * r1: len(clean["coupling"]) - 1]
    assert np.array_equal(got["coupling"][others], clean["coupling"][others])


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    import torch
    S = _surface((5, 3, 8), 17)
    origins, h0 = _geometry(S, 5)
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=dev)
    n, ncfg = len(S["x0"]), 3
    cf = S["cfg_first"].astype(np.int64)
    out = dict(x=to(S["x0"]), T=full(ncfg, 9), Bt=full(ncfg, 36), coupling=full(18 * n), f0=full(n, 3), fmax=full(ncfg), energy=full(ncfg),
               stress0=full(ncfg, 6), status=torch.zeros(ncfg, dtype=torch.int32, device=dev), B=full(ncfg, 36), C=full(ncfg, 36),
               diag=full(ncfg, 2), U=full(18 * n), B_rel=full(ncfg, 36), C_rel=full(ncfg, 36))
    before = {k: v.clone() for k, v in out.items()}
    fix = dict(cfg_first=to(S["cfg_first"]), x0=to(S["x0"]), xt=to(S["x0"] - np.repeat(origins, np.diff(cf), axis=0)), origins=to(origins),
               h0=to(h0), f=torch.ones((n, 3), dtype=torch.float64, device=dev), eatom=torch.ones(n, dtype=torch.float64, device=dev),
               virial=torch.ones((ncfg, 6), dtype=torch.float64, device=dev), c_first=to(18 * cf[:-1]),
               h_first=to(np.concatenate([[0], np.cumsum((3 * np.diff(cf)) ** 2)])[:-1]),
               H=torch.ones(int(((3 * np.diff(cf)) ** 2).sum()), dtype=torch.float64, device=dev),
               vol=torch.ones(ncfg, dtype=torch.float64, device=dev))

    def step(stream=st, k=0, h=H_STRAIN, **swap):
        a = dict(fix, **out)
        a.update(swap)
        capi.elastic_step(a["cfg_first"], k, h, a["x"], a["x0"], a["xt"], a["origins"], a["h0"], a["f"], a["eatom"], a["virial"], a["T"],
                          a["Bt"], a["coupling"], a["c_first"], a["f0"], a["fmax"], a["energy"], a["stress0"], a["status"], stream=stream)

    def finish(stream=st, **swap):
        a = dict(fix, **out)
        a.update(swap)
        capi.elastic_finish(a["cfg_first"], a["c_first"], a["coupling"], a["stress0"], a["Bt"], a["B"], a["C"], a["diag"], a["status"],
                            stream=stream)

    def relax(stream=st, **swap):
        a = dict(fix, **out)
        a.update(swap)
        capi.elastic_relax(a["cfg_first"], a["h_first"], a["H"], a["c_first"], a["coupling"], a["vol"], a["B"], a["C"], a["U"], a["B_rel"],
                           a["C_rel"], a["status"], stream=stream)

    bad = [dict(stream=None), dict(h=0.0), dict(h=-H_STRAIN), dict(h=float("nan")), dict(h=float("inf")), dict(k=-1), dict(k=13)]
    bad += [{key: None} for key in ("x", "x0", "xt", "origins", "h0", "f", "eatom", "virial", "T", "Bt", "coupling", "c_first", "f0", "fmax",
                                    "energy", "stress0", "status")]
    for kw in bad:
        with pytest.raises(capi.MtpError) as ei:
            step(**kw)
        assert ei.value.code == -20, kw
    # (the wrappers count the configurations on cfg_first: that one missing is tests/test_elastic_cpu.py's)
    for kw in [dict(stream=None)] + [{key: None} for key in ("c_first", "coupling", "stress0", "Bt", "B", "C", "diag", "status")]:
        with pytest.raises(capi.MtpError) as ei:
            finish(**kw)
        assert ei.value.code == -20, kw
    for kw in [dict(stream=None)] + [{key: None} for key in ("h_first", "H", "c_first", "coupling", "vol", "B", "C", "U", "B_rel", "C_rel",
                                                              "status")]:
        with pytest.raises(capi.MtpError) as ei:
            relax(**kw)
        assert ei.value.code == -20, kw
    torch.cuda.synchronize()
    for key, t in out.items():
        assert torch.equal(t, before[key]), key
    step(k=12)                                                       # the ends of the range are inside: the last launch ...
    torch.cuda.synchronize()
    assert torch.equal(out["x"], fix["x0"]) and np.array_equal(out["T"].cpu().numpy(), np.tile(EYE9, (3, 1)))
    step(k=0)                                                        # ... and the first
    torch.cuda.synchronize()
    assert not torch.equal(out["f0"], before["f0"]) and not torch.equal(out["x"], fix["x0"])


# ---- mtp_elastic_relax alone ---------------------------------------------------------------------------------------------------

RELAX_ATOMS = (1, 2, 8, 54, 17, 33)           # N = 3, 6, 24, 162, and 51, 99: one above the edge of the first and second LDS tier


def _relax_inputs(atoms=RELAX_ATOMS, saddle_at=None):
    """hand-made Hessians and couplings, one configuration per entry of `atoms`, with clamped B and C and a volume each;
    `saddle_at`: that configuration gets the saddle Hessian of the surface of tests/_neb.py (one negative curvature per atom)"""
    rng = np.random.default_rng(21)
    cfgs = []
    for j, n in enumerate(atoms):
        H, L = _elastic.spring_network(n, 100 + j)
        if j == saddle_at:
            S = _hess.surface_batch((n,), seed=5)
            H = _neb.saddle_hessian(S["A"], S["B"], S["C"], S["D"], S["G"])
        Cm, _ = _elastic.random_constants(200 + j)
        cfgs.append(dict(n=n, H=H, L=L, C=Cm, B=Cm + rng.normal(size=(6, 6)), V=float(rng.uniform(20.0, 400.0))))
    return cfgs


def _device_relax(cfgs):
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pad = lambda a: np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1), [SENTINEL]])
    ncfg = len(cfgs)
    cf = np.concatenate([[0], np.cumsum([c["n"] for c in cfgs])]).astype(np.int64)
    hf = np.concatenate([[0], np.cumsum([(3 * c["n"]) ** 2 for c in cfgs])]).astype(np.int64)
    n = int(cf[-1])
    U, Br, Cr = [torch.full((m,), SENTINEL, dtype=torch.float64, device=dev) for m in (18 * n + 1, 36 * (ncfg + 1), 36 * (ncfg + 1))]
    status = torch.zeros(ncfg + 1, dtype=torch.int32, device=dev)
    status[ncfg] = int(SENTINEL)
    capi.elastic_relax(to(cf.astype(np.int32)), to(hf[:-1].copy()), to(pad(np.concatenate([c["H"].reshape(-1) for c in cfgs]))),
                       to(18 * cf[:-1]), to(pad(np.concatenate([c["L"].reshape(-1) for c in cfgs]))), to(pad([c["V"] for c in cfgs])),
                       to(pad(np.concatenate([c["B"].reshape(-1) for c in cfgs]))), to(pad(np.concatenate([c["C"].reshape(-1) for c in cfgs]))),
                       U, Br, Cr, status, stream=st)
    torch.cuda.synchronize()
    Uh, Bh, Ch, sh = U.cpu().numpy(), Br.cpu().numpy().reshape(ncfg + 1, 6, 6), Cr.cpu().numpy().reshape(ncfg + 1, 6, 6), status.cpu().numpy()
    assert Uh[18 * n] == SENTINEL and (Bh[ncfg] == SENTINEL).all() and (Ch[ncfg] == SENTINEL).all() and sh[ncfg] == int(SENTINEL)
    return [dict(U=Uh[18 * cf[j]: 18 * cf[j + 1]].reshape(6, 3 * c["n"]), B_rel=Bh[j], C_rel=Ch[j], status=int(sh[j])) for j, c in enumerate(cfgs)]


def _assert_relaxed(c, got, what):
    """Cholesky's normwise backward error (Higham, Accuracy and Stability of Numerical Algorithms, Thm. 10.4) for every
    right-hand side, against A formed in float64 numpy; then the relaxed matrices against md.relax_ions on the device's U"""
    n, N = c["n"], 3 * c["n"]
    assert got["status"] == 0, what
    if n == 1:                                                        # the only degrees of freedom are the translations
        assert not got["U"].any() and np.array_equal(got["B_rel"], c["B"]) and np.array_equal(got["C_rel"], c["C"])
        return
    A = c["H"].copy()
    for d in range(3):
        A[d::3, d::3] += (np.trace(c["H"]) / N) / n
    Lp = (c["L"].reshape(6, n, 3) - c["L"].reshape(6, n, 3).mean(1, keepdims=True)).reshape(6, N)
    U = got["U"]
    norm = lambda M: float(np.abs(M).sum(1).max())
    err = norm(A @ U.T - Lp.T) / (norm(A) * norm(U.T))
    bound = 4.0 * N * N * 2.0 ** -53
    want = md.relax_ions(c["B"], c["C"], c["L"], c["H"], c["V"], internal_strain=U)
    host = md.relax_ions(c["B"], c["C"], c["L"], c["H"], c["V"])
    R = np.abs(Lp) @ np.abs(U.T)
    tol = (N + 4) * 2.0 ** -53 * float(R.max()) / c["V"] + 4 * 2.0 ** -53 * float(np.abs(c["B"]).max())     # a sum of N products, a division, a subtraction
    dB, dC = np.abs(got["B_rel"] - want["birch_relaxed"]).max(), np.abs(got["C_rel"] - want["elastic_relaxed"]).max()
    print("%s: N = %d: backward error %.3e (bound %.3e), |dB_rel| %.3e |dC_rel| %.3e (tolerance %.3e), |U - host's|/|U| %.3e, ionic term %.3e"
          % (what, N, err, bound, dB, dC, tol, np.abs(U - host["internal_strain"]).max() / np.abs(U).max(),
             np.abs(want["elastic_relaxed"] - c["C"]).max()))
    assert err <= bound and dB <= tol and dC <= tol, what
    assert host["status"] == "ok" and np.abs(want["elastic_relaxed"] - c["C"]).max() > 1e-4


@pytest.mark.gpu
def test_relax_alone_within_the_backward_error_bound_of_cholesky():
    """N = 3, 6, 24, 162 and one above the edge of each smaller LDS tier, in one batch: ||A U - Lambda^T|| / (||A|| ||U||) <=
    4 N^2 2^-53 in the infinity norm; B_rel and C_rel equal md.relax_ions on the device's own U to rounding"""
    cfgs = _relax_inputs()
    got = _device_relax(cfgs)
    for j, c in enumerate(cfgs):
        _assert_relaxed(c, got[j], "configuration %d" % j)


@pytest.mark.gpu
def test_relax_alone_a_saddle_is_unstable_and_a_configuration_alone_has_its_bits():
    cfgs = _relax_inputs((2, 8, 5, 17, 54), saddle_at=2)
    got = _device_relax(cfgs)
    assert [g["status"] for g in got] == [0, 0, _elastic.UNSTABLE, 0, 0]
    assert np.isnan(got[2]["U"]).all() and np.isnan(got[2]["B_rel"]).all() and np.isnan(got[2]["C_rel"]).all()
    assert md.relax_ions(cfgs[2]["B"], cfgs[2]["C"], cfgs[2]["L"], cfgs[2]["H"], cfgs[2]["V"])["status"] == "unstable"
    for j in (0, 1, 3, 4):
        _assert_relaxed(cfgs[j], got[j], "beside the saddle, configuration %d" % j)
        alone = _device_relax([cfgs[j]])[0]
        for key in ("U", "B_rel", "C_rel"):
            assert np.array_equal(alone[key], got[j][key]), (j, key)


# ---- whole runs ------------------------------------------------------------------------------------------------------------

POTS = [("W_L8.mtp", 1), ("WRe_L20.mtp", 2)]
MASSES = {1: np.array([183.84]), 2: np.array([183.84, 186.207])}


@functools.lru_cache(maxsize=None)
def _ctx(fname):
    return capi.Context(capi.Potential(os.path.join(POT, fname)), 0)


@functools.lru_cache(maxsize=None)
def _oracle(fname):
    from oracle.pyoracle import Oracle
    return Oracle(os.path.join(POT, fname))


@functools.lru_cache(maxsize=None)
def _run(fname, species, h=H_STRAIN):
    """md.elastic_cells on the mixed batch: made once, shared, never written to"""
    return md.elastic_cells(_ctx(fname), _batch.mixed_batch(species), h=h, list_cutoff=LIST_CUTOFF)


@functools.lru_cache(maxsize=None)
def _reference(fname, species):
    return _elastic.reference_loop(_ctx(fname), _batch.mixed_batch(species), H_STRAIN, list_cutoff=LIST_CUTOFF)


def _bounds(wmax, fmax, volume, h=H_STRAIN):
    """The project's parity bounds (tests/test_batch_gpu.py: virial 1e-8 + 1e-10 max(1, |W|max), force 1e-9 + 1e-10 max(1,
    |f|max)) for each of the two numbers of a difference quotient, divided by 2 h; the stress is the virial over the volume."""
    return (1e-8 + 1e-10 * max(1.0, wmax)) / (volume * h), (1e-9 + 1e-10 * max(1.0, fmax)) / h


def _assert_same(got, want, batch, what, skip=()):
    """birch and coupling of every configuration within the bounds; `want` [j]: dict(birch, coupling, wmax, fmax)"""
    for j, (pos, cell, _) in enumerate(batch):
        if j in skip or not len(pos):
            continue
        bB, bL = _bounds(want[j]["wmax"], want[j]["fmax"], abs(float(np.linalg.det(cell))))
        eB = float(np.abs(got[j]["birch"] - want[j]["birch"]).max())
        eL = float(np.abs(got[j]["coupling"] - want[j]["coupling"]).max())
        print("%s, configuration %d (%d atoms): |dB| %.3e (bound %.3e, |B|max %.3e), |dLambda| %.3e (bound %.3e, |Lambda|max %.3e)"
              % (what, j, len(pos), eB, bB, np.abs(want[j]["birch"]).max(), eL, bL, np.abs(want[j]["coupling"]).max()))
        assert eB <= bB and eL <= bL, (what, j)


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_elastic_cells_against_the_host_driven_loop(fname, species):
    """the mixed batch (1, 2, 5, 0, 8 and 54 atoms): birch and coupling within the virial and force parity bounds over the step;
    stress, f0 and the energy against evaluate_cells at their own bounds; the sum rule within 3 n times the force bound; elastic
    is sym(birch - K(stress)) and the asymmetry that of birch - K"""
    batch = _batch.mixed_batch(species)
    got = _run(fname, species)
    want, calls = _reference(fname, species)
    assert calls == 13
    _assert_same(got, want, batch, fname)
    for j, (pos, cell, _) in enumerate(batch):
        r, n = got[j], len(pos)
        assert r["status"] == "ok" and r["birch"].shape == (6, 6) and r["elastic"].shape == (6, 6) and r["coupling"].shape == (6, 3 * n)
        assert r["f0"].shape == (n, 3) and r["stress"].shape == (6,) and abs(r["volume"] - abs(np.linalg.det(cell))) <= 1e-12 * r["volume"]
        if not n:
            assert not r["birch"].any() and not r["elastic"].any() and r["energy"] == 0.0 and r["fmax"] == 0.0 and r["sum_rule"] == 0.0
            continue
        _batch.close(r["f0"], want[j]["f0"], "f0, configuration %d" % j)
        _batch.close_energy(r["energy"], want[j]["energy"], n, "energy, configuration %d" % j)
        _batch.close(r["stress"] * r["volume"], want[j]["stress"] * r["volume"], "stress x volume, configuration %d" % j, atol=1e-8)
        want_fmax = float(np.sqrt((want[j]["f0"] ** 2).sum(1)).max())
        assert abs(r["fmax"] - want_fmax) <= 1e-9 + 1e-10 * max(1.0, want_fmax)
        bL = _bounds(want[j]["wmax"], want[j]["fmax"], r["volume"])[1]
        M = r["birch"] - md.stress_correction(r["stress"])
        print("configuration %d: asymmetry %.3e, sum rule %.3e (bound %.3e), raw asymmetry of birch %.3e"
              % (j, r["asymmetry"], r["sum_rule"], 3 * n * bL, np.abs(r["birch"] - r["birch"].T).max()))
        assert r["sum_rule"] <= 3 * n * bL
        assert np.abs(r["elastic"] - 0.5 * (M + M.T)).max() <= 1e-14 * np.abs(M).max() and np.array_equal(r["elastic"], r["elastic"].T)
        assert abs(r["asymmetry"] - np.abs(M - M.T).max()) <= 1e-14 * np.abs(M).max()
    assert max(np.abs(got[j]["birch"]).max() for j in (1, 2, 4, 5)) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_elastic_cells_against_the_cpu_oracle(fname, species):
    """the members of up to 8 atoms: the cell and the atoms strained on the host, virial and forces from the CPU oracle on the
    images of the numpy ghost twin, the same difference quotients.  The bounds are the same."""
    batch = _batch.mixed_batch(species)
    got = _run(fname, species)
    orc = _oracle(fname)
    want = {}
    for j in (0, 1, 2, 4):
        pos, cell, types = batch[j]
        w = dict(birch=np.zeros((6, 6)), coupling=np.zeros((6, 3 * len(pos))), wmax=0.0, fmax=0.0)
        for k in range(12):
            c, s, D = _elastic.strain_of(k, H_STRAIN)
            _, f, vir, _, _ = _cells.oracle_cell(orc, pos @ D, cell @ D, types)
            sign = -1.0 if k & 1 else 1.0
            w["birch"][:, c] += sign * (-np.asarray(vir) / float(np.linalg.det(cell @ D))) / (2.0 * H_STRAIN)
            w["coupling"][c] += sign * f.reshape(-1) / (2.0 * H_STRAIN)
            w["wmax"], w["fmax"] = max(w["wmax"], float(np.abs(vir).max())), max(w["fmax"], float(np.abs(f).max()))
        want[j] = w
    _assert_same(got, want, batch, "%s, oracle" % fname, skip=(3, 5))


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_the_primitive_cell_is_cubic(fname, species):
    """one atom in the bcc primitive cell: birch has three equal diagonal, three equal off-diagonal and three equal shear entries
    and nothing else, it is symmetric (the stress is hydrostatic), and no strain puts a force on the atom -- all within the
    bounds of the comparison with the host-driven loop (two entries that should be equal are each within the bound)"""
    r = _run(fname, species)[0]
    want = _reference(fname, species)[0][0]
    bB, bL = _bounds(want["wmax"], want["fmax"], r["volume"])
    B = r["birch"]
    c11, c12, c44 = B[0, 0], B[0, 1], B[3, 3]
    cubic = np.zeros((6, 6))
    cubic[:3, :3] = c12
    cubic[range(3), range(3)] = c11
    cubic[range(3, 6), range(3, 6)] = c44
    print("%s: B11 %.6f B12 %.6f B44 %.6f, off cubic %.3e (bound %.3e), |B - B^T| %.3e, |coupling| %.3e (bound %.3e), sum rule %.3e"
          % (fname, c11, c12, c44, np.abs(B - cubic).max(), 2 * bB, np.abs(B - B.T).max(), np.abs(r["coupling"]).max(), bL, r["sum_rule"]))
    assert np.abs(B - cubic).max() <= 2 * bB and np.abs(B - B.T).max() <= 2 * bB
    assert np.abs(r["coupling"]).max() <= bL and r["coupling"].shape == (6, 3)
    assert min(abs(c11), abs(c12), abs(c44)) > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_the_asymmetry_falls_with_the_square_of_the_step(fname, species):
    """asymmetry = max |(B - K) - (B - K)^T| is a truncation quantity of order h^2: at h = 0.002 it is below a tenth of what it is
    at h = 0.01 (the CPU oracle gives ratios near 25), for the configurations 1, 2 and 4"""
    fine, coarse = _run(fname, species, 0.002), _run(fname, species, 0.01)
    for j in (1, 2, 4):
        print("%s, configuration %d: asymmetry %.3e at h = 0.002, %.3e at h = 0.01, ratio %.1f; raw asymmetry of birch %.3e"
              % (fname, j, fine[j]["asymmetry"], coarse[j]["asymmetry"], coarse[j]["asymmetry"] / fine[j]["asymmetry"],
                 np.abs(fine[j]["birch"] - fine[j]["birch"].T).max()))
        assert fine[j]["asymmetry"] < 0.1 * coarse[j]["asymmetry"], j


def _as_wanted(run):
    return [dict(r, wmax=float(np.abs(r["stress"]).max()) * r["volume"] + H_STRAIN * float(np.abs(r["birch"]).max()) * r["volume"],
                 fmax=float(np.abs(r["f0"]).max(initial=0.0)) + H_STRAIN * float(np.abs(r["coupling"]).max(initial=0.0))) for r in run]


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_far_positions_and_a_split_batch_give_the_same_matrices(fname, species):
    """the tilted cell handed over with its atoms many lattice vectors away (the same crystal), and the batch split into the
    passes 1 2 5 0 | 8 | 54 by max_atoms_per_pass = 10: the matrices of the whole batch within the bounds"""
    batch = _batch.mixed_batch(species)
    want = _as_wanted(_run(fname, species))
    far = list(batch)
    pos, cell, types = far[2]
    far[2] = (pos + np.array([[3, -2, 1], [0, 0, 0], [-7, 4, 0], [1, 1, 1], [0, -5, 2]]) @ cell, cell, types)
    got = md.elastic_cells(_ctx(fname), far, h=H_STRAIN, list_cutoff=LIST_CUTOFF)
    _assert_same(got, want, batch, "%s, far" % fname)
    _batch.close(got[2]["f0"], want[2]["f0"], "f0 of the far configuration")
    split = md.elastic_cells(_ctx(fname), batch, h=H_STRAIN, list_cutoff=LIST_CUTOFF, max_atoms_per_pass=10)
    _assert_same(split, want, batch, "%s, split" % fname)
    for j in range(len(batch)):
        assert split[j]["status"] == "ok"
        _batch.close(split[j]["f0"], want[j]["f0"], "f0, configuration %d" % j)


# ---- end to end ------------------------------------------------------------------------------------------------------------

E2E_STOL, E2E_FTOL = 1e-6, 1e-6


def _end_to_end(fname, species, which, **fire):
    """relax_cells_vc -> elastic_cells(relax_ions=True) -> moduli on one cell, then for the strains xx and xy the stress
    difference of the cell strained by +-h with the atoms RE-RELAXED by relax_cells, against birch_relaxed and against birch.
    `fire`: minimiser settings for both relaxations.  Returns the figures."""
    cfg = {"cubic2": _cells.cubic2_cell, "tilted5": lambda: _cells.tilted5_cell(species),
           "sheared8": lambda: _batch.sheared8_cell(species)}[which]()
    ctx, types, masses = _ctx(fname), cfg[2], MASSES[species]
    vc = md.relax_cells_vc(ctx, [cfg], 4000, stol=E2E_STOL, ftol=E2E_FTOL, masses=masses, list_cutoff=LIST_CUTOFF, **fire)["final"][0]
    print("%s, %s: relax_cells_vc: %s at step %d, fmax %.3e, smax %.3e" % (fname, which, vc["status"], vc["step"], vc["fmax"], vc["smax"]))
    assert vc["status"] == "converged"                                         # (otherwise the test's inputs are wrong)
    x, cell = vc["x"], vc["cell"]
    r = md.elastic_cells(ctx, [(x, cell, types)], h=H_STRAIN, relax_ions=True, list_cutoff=LIST_CUTOFF)[0]
    out = dict(r=r, moduli=md.moduli(r["elastic_relaxed"]) if r["status"] == "ok" else None, relaxed=[], clamped=[])
    bB = _bounds(float(np.abs(r["stress"]).max()) * r["volume"] + H_STRAIN * float(np.abs(r["birch"]).max()) * r["volume"], 1.0,
                 r["volume"])[0]
    out["ionic"], out["bound"] = float(np.abs(r["birch_relaxed"] - r["birch"]).max()), bB
    for w in (0, 3):
        sig = []
        for sign in (1.0, -1.0):
            D = _elastic.strain_matrix(w, sign * H_STRAIN).reshape(3, 3)
            got = md.relax_cells(ctx, [(x @ D, cell @ D, types)], 4000, ftol=E2E_FTOL, masses=masses, list_cutoff=LIST_CUTOFF, **fire)["final"][0]
            assert got["status"] == "converged", (w, sign)
            ev = md.evaluate_cells(ctx, [(got["x"], cell @ D, types)], list_cutoff=LIST_CUTOFF)[0]
            sig.append(-ev["virial"] / float(np.linalg.det(cell @ D)))
        dq = (sig[0] - sig[1]) / (2.0 * H_STRAIN)
        out["relaxed"].append(float(np.abs(dq - r["birch_relaxed"][:, w]).max()))
        out["clamped"].append(float(np.abs(dq - r["birch"][:, w]).max()))
    return out


GENTLE = dict(dmax=0.01, dt_max=2e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species,which,fire", [("W_L8.mtp", 1, "sheared8", GENTLE), ("WRe_L20.mtp", 2, "tilted5", {})],
                         ids=["W_L8-sheared8", "WRe_L20-tilted5"])
def test_relax_vc_then_elastic_then_moduli_end_to_end(fname, species, which, fire):
    """A cell relaxed together with its atoms, its elastic constants with relaxed ions, its moduli.  The stress is within the stol
    used and the status "ok" (the relaxed cell is a minimum).  What the ionic term is for: the stress response of the cell
    strained by +-h with its atoms re-relaxed is that of birch_relaxed, not of birch -- the discrepancy of the relaxed matrix is
    below a tenth of the clamped one's, for the strains xx and xy.  Both are printed; no absolute tolerance is fixed here, since
    it depends on ftol and on h^2 terms.

    The cells are those of tests/test_hess_gpu.py's end-to-end test with one exchange: under W_L8.mtp the noisy cubic 2-atom cell
    relaxes to bcc sites, where every atom is a centre of inversion and the coupling vanishes (measured with WRe_L20.mtp: an ionic
    term of 1.6e-16 eV/A^3 against 100 x bound = 7.5e-6), so it shows nothing of the ionic term; the sheared 8-atom cell stands
    in for it.  W_L8.mtp is a generated potential whose energy surface has wells hundreds of eV deep a few tenths of an angstrom
    away: its variable-cell relaxation is run with a short step (dmax 0.01 A, dt_max 2 fs) so that it settles in the basin
    it starts in.  Measured (eV/A^3; relaxed | clamped discrepancy for xx, xy): WRe_L20.mtp tilted5 4.0e-3, 9.7e-4 | 1.1e-1,
    6.2e-2, ionic term 0.40; W_L8.mtp sheared8 1.3e-3, 1.7e-4 | 1.3e-1, 3.6e-2, ionic term 0.20."""
    e = _end_to_end(fname, species, which, **fire)
    r, m = e["r"], e["moduli"]
    print("%s, %s: status %s, fmax %.3e, |stress|max %.3e, asymmetry %.3e, ionic term %.3e (100 x bound %.3e)"
          % (fname, which, r["status"], r["fmax"], np.abs(r["stress"]).max(), r["asymmetry"], e["ionic"], 100 * e["bound"]))
    print("moduli:", {k: (round(v, 6) if isinstance(v, float) else v) for k, v in m.items()})
    print("discrepancy of the re-relaxed stress response, strains xx, xy: relaxed %s, clamped %s" % (e["relaxed"], e["clamped"]))
    assert r["status"] == "ok" and np.abs(r["stress"]).max() <= E2E_STOL * (1.0 + 1e-9) + e["bound"] * H_STRAIN
    assert r["hessian"].shape == (3 * len(r["f0"]),) * 2 and r["internal_strain"].shape == r["coupling"].shape
    assert e["ionic"] >= 100 * e["bound"]                                     # (otherwise this cell shows nothing of the ionic term)
    assert np.isfinite(m["compressibility"]) and m["bulk_reuss"] <= m["bulk_voigt"] * (1.0 + 1e-12)
    for w in range(2):
        assert e["relaxed"][w] < 0.1 * e["clamped"][w], w
