"""Batched variable-cell relaxation on the device (md.relax_cells_vc; mtp_relax_cell_step, mtp_ghosts_deform): the kernel alone
against the numpy twin of tests/_relax_vc.py on the analytic model (forces and virials made by the test between launches from
the device's own positions and cells), its failed states, batch independence to the bit and the argument errors; the ghosts
that follow a deforming cell; the generalised forces against central differences of E + p V through the real potential; then
the whole loop against the host-driven loop, the fixed-cell limit against md.relax_cells, convergence end to end and capture
under cell relaxation.  Every comparison asserts the twin's four tie margins first: rounding is 1e-12, so with margins of 1e-6
no decision can flip."""
import functools

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

import _batch
import _cells
import _relax_vc
import _sample
from _cells import LIST_CUTOFF
from _relax_vc import GPA, det3, sym
from test_relax_vc_cpu import bcc2, oracle_evaluate
from test_sample_gpu import BIG, E_TOL, MASSES, V_TOL, X_TOL, _ctx, _midpoint_threshold

FROZEN = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.int32)             # the 64-atom configuration is frozen from the start
PARAMS = dict(dt_max=2e-2, pressure=2.0 * GPA, stol=1e-4, ftol=1e-3)
KEEP = (2, 10, 29, 60, 199)
SENTINEL = -77.0
ORIGINS = np.random.default_rng(4).uniform(-60.0, 60.0, (7, 3))
PER_ROW = ("x", "xt", "vt")
PER_CFG = ("D", "vq", "dt", "alpha", "fmax", "smax", "gcell", "h", "T", "cellmove")
INTS = ("npos", "frozen", "done_step")


# ---- the kernel alone ----------------------------------------------------------------------------------------------------

def _model():
    """strain 0.015: with |dD| <= dmax / L a step the 256- and 257-atom cells reach their minimum within the 200 steps too, so
    that the state after the last step has every velocity at exactly 0, as in tests/test_relax_gpu.py"""
    return _relax_vc.Model(strain=0.015)


def _params(cell_factor=None, cell_mass=None, cell_mask=(1, 1, 1, 1, 1, 1), isotropic=False, pressure=0.0, stol=1e-4, **fire):
    p = dict(_relax_vc.DEFAULTS, **fire)
    par = capi.RelaxParams(p["ftol"], p["dt_max"], p["dmax"], p["f_inc"], p["f_dec"], p["alpha_start"], p["f_alpha"], p["n_min"])
    return capi.relax_cell_params(par, stol, pressure, 1.0 if cell_factor is None else cell_factor,
                                  _relax_vc.MODEL_MASSES.mean() if cell_mass is None else cell_mass, cell_mask, isotropic,
                                  cell_factor is None)


def _device_model(model, steps, frozen, origins, poison=None, keep=(), dt=1e-3, **kw):
    """mtp_relax_cell_step on the model for steps 0 .. steps - 1; between the launches the test reads x and h back, evaluates
    the model in numpy and uploads f and W.  poison = (step, "W", k, q, value) or (step, "D", k, matrix).  One row and one
    configuration more than the batch holds are allocated and filled with a sentinel.  Returns the arrays after the last
    step and copies of them after the steps of `keep`."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ncfg, n = model.ncfg, model.n
    pad = lambda a: np.concatenate([a, np.full((1,) + a.shape[1:], SENTINEL, dtype=a.dtype)])
    par = _params(**kw)
    eye = np.tile(np.eye(3).reshape(1, 9), (ncfg, 1))
    h0 = model.h0.reshape(ncfg, 9)
    x0 = model.x0 + origins[model.cfg]
    nimg = np.array([_relax_vc.images(c, LIST_CUTOFF) for c in model.h0], dtype=np.int32).reshape(ncfg, 3)
    A = dict(cfg_first=to(model.cf), x=to(pad(x0)), xt=to(pad(model.x0)), vt=to(pad(np.zeros_like(x0))), f=to(pad(np.zeros_like(x0))),
             type=to(pad(model.types)), inv_mass=to(1.0 / _relax_vc.MODEL_MASSES), virial=to(np.zeros((ncfg, 6))), h0=to(h0),
             origins=to(origins), D=to(pad(eye)), vq=to(pad(np.zeros((ncfg, 9)))), Dbinv=to(eye), href=to(h0), nimg=to(nimg),
             dt=to(pad(np.full(ncfg, dt))), alpha=to(pad(np.full(ncfg, kw.get("alpha_start", _relax_vc.DEFAULTS["alpha_start"])))),
             npos=to(pad(np.zeros(ncfg, dtype=np.int32))), frozen=to(pad(np.asarray(frozen, dtype=np.int32))),
             done_step=to(pad(np.full(ncfg, -1, dtype=np.int32))), fmax=to(pad(np.zeros(ncfg))), smax=to(pad(np.zeros(ncfg))),
             gcell=to(pad(np.zeros((ncfg, 9)))), h=to(pad(h0)), T=to(pad(eye)), cellmove=to(pad(np.zeros(ncfg))),
             counts=to(np.zeros(3, dtype=np.int32)))

    def state(f, W, s):
        torch.cuda.synchronize()
        out = {k: A[k].cpu().numpy() for k in PER_ROW + PER_CFG + INTS + ("counts",)}
        out.update(f=f, W=W, step=s)
        return out

    kept, f, W, s = {}, np.zeros((n, 3)), np.zeros((ncfg, 6)), -1
    for s in range(steps):
        torch.cuda.synchronize()
        xh, hh = A["x"].cpu().numpy()[:n], A["h"].cpu().numpy()[:ncfg].reshape(ncfg, 3, 3)
        with np.errstate(all="ignore"):
            _, f, W = model.all(xh, hh, origins)
        if poison is not None and poison[0] == s:
            if poison[1] == "W":
                W[poison[2], poison[3]] = poison[4]
            else:
                A["D"][poison[2]] = to(np.asarray(poison[3], dtype=np.float64).reshape(9))
        A["f"][:n] = to(f)
        A["virial"].copy_(to(W))
        capi.relax_cell_step(ncfg, par, s, A, stream=st)
        if s in keep:
            kept[s] = state(f, W, s)
    out = state(f, W, s)
    for k in PER_ROW:                                                                # nothing behind the last row ...
        assert (out[k][n:] == SENTINEL).all(), k
    for k in PER_CFG + INTS:                                                         # ... or the last configuration
        assert (out[k][ncfg:] == SENTINEL).all(), k
    return out, kept


def _twin_poison(poison):
    if poison is None:
        return None
    if poison[1] == "W":
        return poison[0], lambda f, W, twin: W.__setitem__((poison[2], poison[3]), poison[4])
    return poison[0], lambda f, W, twin: twin.D.__setitem__(poison[2], np.asarray(poison[3], dtype=np.float64))


@functools.lru_cache(maxsize=None)
def _batch_run():
    """the batch of the kernel tests on the device, 200 steps, with its state after the steps of KEEP: made once, never written to"""
    return _device_model(_model(), 200, FROZEN, ORIGINS, keep=KEEP, **PARAMS)


def _rel(got, want):
    if not np.size(want):
        return 0.0
    scale, err = float(np.abs(want).max()), float(np.abs(np.asarray(got).reshape(np.shape(want)) - want).max())
    return err / scale if scale > 0.0 else err


def _assert_follows(got, want, twin, model, what, converged=False):
    """x, xt, vt, D, vq, dt, alpha, h, T within 1e-12 relative (of the largest entry), the integers exactly.  fmax, smax and G:
    1e-12 of the largest entry while everything moves; converged=True (the state after the small configurations have converged)
    takes the caveat of tests/test_relax_gpu.py::_assert_follows -- the model's f = -k (x - s0 . h) and h h^T - G_eq subtract
    numbers far larger than what is left near the minimum, so positions and cells that agree to 1e-12 relative give forces and
    virials that agree to 1e-12 of k |x| and of K2 |h|^4 and no better: fmax within 1e-12 of the largest k |s0 . h|, smax and
    G within 1e-12 of the largest K2 |h|^4 / V and K2 |h|^4 / L."""
    n, ncfg = model.n, model.ncfg
    errs = {k: _rel(got[k][:n], want[k]) for k in PER_ROW}
    errs.update({k: _rel(got[k][:ncfg], want[k]) for k in ("D", "vq", "dt", "alpha", "h", "T")})
    loose = {k: _rel(got[k][:ncfg], want[k]) for k in ("fmax", "smax", "gcell")}
    move = float(np.abs(got["cellmove"][:ncfg] - want["cellmove"]).max())
    print(what, " ".join("%s %.2e" % kv for kv in list(errs.items()) + list(loose.items())), "cellmove %.2e A" % move)
    assert all(e <= 1e-12 for e in errs.values()), errs
    assert move <= 1e-12 * 4.0 * float(np.abs(want["h"]).max()) * 3
    if converged:
        h4 = np.array([np.abs(h).max() ** 4 for h in want["h"]]) * model.k2
        vol = np.array([det3(h) for h in want["h"]])
        fscale = float(np.abs(model.k[model.cfg][:, None] * np.einsum("ia,iab->ib", model.s0, want["h"][model.cfg])).max())
        assert float(np.abs(got["fmax"][:ncfg] - want["fmax"]).max()) <= 1e-12 * fscale
        assert float(np.abs(got["smax"][:ncfg] - want["smax"]).max()) <= 1e-12 * float((h4 / vol).max())
        assert float(np.abs(got["gcell"][:ncfg].reshape(ncfg, 3, 3) - want["gcell"]).max()) <= 1e-12 * float((h4 / np.maximum(twin.L, 1.0)).max())
    else:
        assert all(e <= 1e-12 for e in loose.values()), loose
    for k in INTS:
        assert np.array_equal(got[k][:ncfg], want[k]), k


def _assert_own_fmax(got, model, frozen0, what):
    """fmax of every configuration the launch of got["step"] looked at, against sqrt(max |f_i|^2) of the very forces that launch
    was given: 1e-12 relative, entry by entry -- what the kernel itself adds, free of the model's cancellation"""
    worst = 0.0
    for k in range(model.ncfg):
        a, b = int(model.cf[k]), int(model.cf[k + 1])
        if b == a or frozen0[k] or not (got["frozen"][k] == 0 or got["done_step"][k] == got["step"]):
            continue
        fmax = float(np.sqrt(np.fmax.reduce((got["f"][a:b] ** 2).sum(1))))
        worst = max(worst, abs(got["fmax"][k] - fmax) / fmax)
    print(what, "fmax against the launch's own forces: %.3e relative" % worst)
    assert worst <= 1e-12


@pytest.mark.gpu
def test_kernel_alone_follows_the_twin_on_the_model_for_200_steps():
    """configurations of 0, 1, 63, 64, 65, 256 and 257 atoms: the lane and wavefront widths and both sides of the switch from a
    wavefront to the workgroup; two masses; slot origins up to 60 A; the 64-atom one frozen from the start; p = 2 GPa.  Compared
    after step 60, while everything still moves (the first configuration converges at step 81), and after step 199, when all
    have converged: in between the velocities shrink towards rounding of the model's own subtractions (_assert_follows)."""
    model = _model()
    twin, x, xt, vt, kept = _relax_vc.run_model(model, 200, frozen=FROZEN, origins=ORIGINS, keep=(60, 199), **PARAMS)
    twin.assert_margins()
    print("twin: done_step", twin.done_step, "uphill", twin.uphill, "capped", twin.capped, "margins", twin.margins())
    assert twin.uphill >= 1 and twin.capped >= 1
    assert list(twin.frozen) == [0, 2, 2, 1, 2, 2, 2] and twin.done_step[twin.frozen == 2].min() > 60
    got, dev_kept = _batch_run()
    _assert_follows(dev_kept[60], kept[60], twin, model, "after step 60:")
    assert np.abs(kept[60]["vt"]).max() > 0.0 and np.abs(kept[60]["vq"]).max() > 0.0 and np.abs(kept[60]["D"] - np.eye(3)).max() > 1e-3
    _assert_follows(got, kept[199], twin, model, "after step 199:", converged=True)
    assert list(got["counts"]) == [0, 0, twin.count]
    for s in KEEP:
        _assert_own_fmax(dev_kept[s], model, FROZEN, "after step %d:" % s)
    # the frozen and the empty configuration: bitwise untouched
    a, b = int(model.cf[3]), int(model.cf[4])
    assert np.array_equal(got["xt"][a:b], model.x0[a:b]) and not got["vt"][a:b].any()
    for k in (0, 3):
        assert got["dt"][k] == 1e-3 and got["alpha"][k] == 0.1 and got["npos"][k] == 0 and got["done_step"][k] == -1
        assert got["fmax"][k] == 0.0 and got["smax"][k] == 0.0 and got["frozen"][k] == FROZEN[k] and got["cellmove"][k] == 0.0
        assert np.array_equal(got["D"][k], np.eye(3).reshape(9)) and not got["vq"][k].any() and not got["gcell"][k].any()
    # a converged configuration: velocities zeroed, x = origin + xt . D to rounding
    for k in (1, 2, 4, 5, 6):
        a, b = int(model.cf[k]), int(model.cf[k + 1])
        assert not got["vt"][a:b].any() and not got["vq"][k].any()
        assert np.abs(got["x"][a:b] - ORIGINS[k] - got["xt"][a:b] @ got["D"][k].reshape(3, 3)).max() < 1e-13
        assert np.abs(got["h"][k].reshape(3, 3) - model.h0[k] @ got["D"][k].reshape(3, 3)).max() < 1e-14


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [(3, "W", 4, 5, float("nan")), (3, "W", 6, 0, float("inf")),
                                    (3, "D", 4, np.diag([1.0, 1.0, -1.0])), (3, "D", 6, np.zeros((3, 3)))],
                         ids=["nan-virial", "inf-virial-workgroup", "negative-det", "singular-D-workgroup"])
def test_a_bad_virial_or_deformation_fails_its_configuration_and_no_other(poison):
    model = _model()
    kf = poison[2]
    a, b = int(model.cf[kf]), int(model.cf[kf + 1])
    got, kept = _device_model(model, 11, FROZEN, ORIGINS, poison=poison, keep=(2,), **PARAMS)
    twin = _relax_vc.run_model(model, 11, frozen=FROZEN, origins=ORIGINS, poison=_twin_poison(poison), **PARAMS)[0]
    clean = _batch_run()[1]
    assert got["frozen"][kf] == _relax_vc.FAILED and got["done_step"][kf] == 3
    assert np.array_equal(got["frozen"][:7], twin.frozen) and np.array_equal(got["done_step"][:7], twin.done_step)
    before = kept[2]
    for key in PER_ROW:
        assert np.array_equal(got[key][a:b], before[key][a:b]), key
    for key in ("vq", "dt", "alpha", "npos") + (("D",) if poison[1] == "W" else ()):
        assert np.array_equal(got[key][kf], before[key][kf]), key
    assert before["vt"][a:b].any()
    others = np.ones(model.n + 1, dtype=bool)
    others[a:b] = False
    ok = np.arange(8) != kf
    for key in PER_ROW:
        assert np.array_equal(got[key][others], clean[10][key][others]), key
    for key in PER_CFG + INTS:
        assert np.array_equal(got[key][ok], clean[10][key][ok]), key
    assert list(got["counts"]) == [0, 0, 1] and list(clean[10]["counts"]) == [0, 0, 0]


@pytest.mark.gpu
def test_a_configuration_alone_has_the_bits_it_has_in_the_batch():
    model = _model()
    batch = _batch_run()[1][29]
    for k in range(7):
        a, b = int(model.cf[k]), int(model.cf[k + 1])
        one, _ = _device_model(model.take(k), 30, FROZEN[k: k + 1], ORIGINS[k: k + 1], **PARAMS)
        for key in PER_ROW:
            assert np.array_equal(one[key][: b - a], batch[key][a:b]), (k, key)
        for key in PER_CFG + INTS:
            assert np.array_equal(one[key][0], batch[key][k]), (k, key)
    assert batch["vt"].any() and batch["vq"].any()


@pytest.mark.gpu
def test_isotropic_and_masked_cells_on_the_device():
    """the twin's properties hold on the device to the bit: an isotropic cell keeps D a multiple of I, a cell without the shear
    components keeps D diagonal, a mask of zeros keeps D = I and x = origin + xt"""
    model = _relax_vc.Model(sizes=[2, 5, 300], k_cfg=(2.0, 5.0, 9.0), seed=5)
    org = ORIGINS[:3]
    off = ~np.eye(3, dtype=bool).reshape(9)
    iso, _ = _device_model(model, 40, np.zeros(3), org, isotropic=True, pressure=2.0 * GPA)
    shear, _ = _device_model(model, 40, np.zeros(3), org, cell_mask=(1, 1, 1, 0, 0, 0))
    fixed, _ = _device_model(model, 40, np.zeros(3), org, cell_mask=(0, 0, 0, 0, 0, 0))
    for k in range(3):
        D = iso["D"][k]
        assert (D[off] == 0.0).all() and D[0] == D[4] == D[8] != 1.0 and (iso["vq"][k][off] == 0.0).all()
        D = shear["D"][k]
        assert (D[off] == 0.0).all() and len({D[0], D[4], D[8], 1.0}) == 4
        assert np.array_equal(fixed["D"][k], np.eye(3).reshape(9)) and np.array_equal(fixed["T"][k], np.eye(3).reshape(9))
        assert fixed["smax"][k] == 0.0 and fixed["cellmove"][k] == 0.0
    tw = _relax_vc.run_model(model, 40, origins=org, isotropic=True, pressure=2.0 * GPA)[0]
    tw.assert_margins()
    assert _rel(iso["D"][:3].reshape(3, 3, 3), tw.D) <= 1e-12


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    import torch
    model = _relax_vc.Model(sizes=[3, 70], k_cfg=(2.0, 5.0))
    base, _ = _device_model(model, 1, np.zeros(2), ORIGINS[:2])
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    n = model.n
    A = dict(cfg_first=to(model.cf), x=to(base["x"]), xt=to(base["xt"]), vt=to(base["vt"]), f=to(rng.normal(size=(n + 1, 3))),
             type=to(np.append(model.types, 1).astype(np.int32)), inv_mass=to(1.0 / _relax_vc.MODEL_MASSES),
             virial=to(rng.normal(size=(2, 6))), h0=to(model.h0.reshape(2, 9)), origins=to(ORIGINS[:2]), D=to(base["D"]), vq=to(base["vq"]),
             Dbinv=to(np.tile(np.eye(3).reshape(1, 9), (2, 1))), href=to(model.h0.reshape(2, 9)), nimg=to(np.full((2, 3), 2, dtype=np.int32)),
             dt=to(base["dt"]), alpha=to(base["alpha"]), npos=to(base["npos"]), frozen=to(np.zeros(3, dtype=np.int32)),
             done_step=to(base["done_step"]), fmax=to(base["fmax"]), smax=to(base["smax"]), gcell=to(base["gcell"]), h=to(base["h"]),
             T=to(base["T"]), cellmove=to(base["cellmove"]), counts=to(np.zeros(3, dtype=np.int32)))
    before = {k: t.clone() for k, t in A.items()}

    def call(stream=st, step=0, arrays=None, **kw):
        capi.relax_cell_step(2, _params(**kw), step, A if arrays is None else arrays, stream=stream)

    nan, inf = float("nan"), float("inf")
    bad = [dict(stream=None), dict(step=-1), dict(ftol=-1e-3), dict(ftol=nan), dict(dt_max=0.0), dict(dt_max=inf), dict(dmax=0.0),
           dict(dmax=nan), dict(f_inc=0.99), dict(f_inc=inf), dict(f_dec=0.0), dict(f_dec=1.0), dict(f_dec=nan), dict(alpha_start=-0.1),
           dict(alpha_start=1.1), dict(f_alpha=0.0), dict(f_alpha=1.01), dict(n_min=-1),
           dict(stol=-1e-9), dict(stol=nan), dict(pressure=nan), dict(pressure=inf), dict(cell_factor=0.0), dict(cell_factor=-2.0),
           dict(cell_factor=inf), dict(cell_mass=0.0), dict(cell_mass=nan), dict(cell_mask=(1, 1, 1, 2, 0, 0)),
           dict(cell_mask=(-1, 1, 1, 0, 0, 0))]
    for kw in bad:
        with pytest.raises(capi.MtpError) as ei:
            call(**kw)
        assert ei.value.code == -20, kw
    for missing in capi.RELAX_CELL_ARRAYS:                                           # a missing array, each of them
        with pytest.raises(capi.MtpError) as ei:
            call(arrays={k: t for k, t in A.items() if k != missing})
        assert ei.value.code == -20, missing
    torch.cuda.synchronize()
    for k, t in A.items():
        assert torch.equal(t, before[k]), k
    call(ftol=0.0, stol=0.0, f_inc=1.0, alpha_start=0.0, f_alpha=1.0, n_min=0, cell_mask=(0, 0, 0, 0, 0, 0))   # the ends of the ranges are inside
    torch.cuda.synchronize()
    assert not torch.equal(A["vt"], before["vt"])


# ---- ghosts that follow the cell -----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_ghosts_follow_a_deformed_cell():
    """the tilted 5-atom cell and the sub-cutoff primitive cell in one batch; T random within 1e-3 of I per configuration.  After
    deform + forward every ghost row is its owner + n . (h . T), n recovered by rounding shift . h^-1 of the build; deforming twice
    from the same build gives the bits of deforming once (the shifts of the build are kept: rounding does not accumulate)."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    batch = [_cells.tilted5_cell(), _cells.primitive_cell()]
    cells = np.array([c[1] for c in batch])
    cf = np.array([0, 5, 6], dtype=np.int32)
    lay = capi.batch_layout(cells, LIST_CUTOFF)
    x = torch.zeros((4096, 3), dtype=torch.float64, device=dev)
    x[:6] = to(np.concatenate([c[0] for c in batch]))
    g = capi.Ghosts(0)
    nall = g.build_batch(x, cf, cells, lay["origins"], LIST_CUTOFF, stream=st)
    assert 6 + 511 < nall <= 4096
    row_cfg = torch.zeros(6, dtype=torch.int32, device=dev)
    capi.sample_row_map(to(cf), row_cfg, stream=st)
    owner_t = torch.zeros(4096, dtype=torch.int32, device=dev)
    owner_t[:6] = torch.arange(6, dtype=torch.int32, device=dev)
    g.types(owner_t, stream=st)                                                      # (ghost "types" <- the owners' row numbers)
    torch.cuda.synchronize()
    owner = owner_t.cpu().numpy()[:nall]
    x0 = x.cpu().numpy()[:nall]
    cfg = np.array([0] * 5 + [1])[owner]
    shift0 = x0 - x0[owner]
    nint = np.array([np.round(shift0[i] @ np.linalg.inv(cells[cfg[i]])) for i in range(nall)])
    assert np.abs(np.einsum("ia,iab->ib", nint, cells[cfg]) - shift0).max() < 1e-12 and (np.abs(nint[6:]).sum(1) > 0).all()
    rng = np.random.default_rng(12)
    T1, T2 = (np.eye(3) + rng.uniform(-1e-3, 1e-3, (2, 3, 3)) for _ in range(2))
    g.deform(row_cfg, to(T2.reshape(2, 9)), stream=st)
    g.forward(x, stream=st)
    torch.cuda.synchronize()
    once = x.cpu().numpy()[:nall]
    want = once[owner] + np.einsum("ia,iab->ib", nint, np.einsum("kab,kbc->kac", cells, T2)[cfg])
    err = float(np.abs(once - want).max())
    print("%d ghosts: ghost rows against owner + n . (h . T): %.3e A" % (nall - 6, err))
    assert err <= 1e-13 and np.array_equal(once[:6], x0[:6]) and np.abs(once[6:] - x0[6:]).max() > 1e-4
    g.deform(row_cfg, to(T1.reshape(2, 9)), stream=st)
    g.deform(row_cfg, to(T2.reshape(2, 9)), stream=st)
    g.forward(x, stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy()[:nall], once)
    with pytest.raises(capi.MtpError) as ei:
        g.deform(row_cfg, to(T2.reshape(2, 9)), stream=None)
    assert ei.value.code == -20


# ---- the generalised forces through the real potential --------------------------------------------------------------------

def _generalised(evaluate, pos, cell, types, D, p, delta=1e-5):
    """(G, ft) from the virial and forces of `evaluate` at x = pos . D, h = cell . D, and the same two from central differences
    of E + p V; L = the atom count"""
    n = len(pos)
    L = float(n)
    configs = [(pos @ D, cell @ D, types)]
    for a in range(3):
        for b in range(3):
            for sgn in (1.0, -1.0):
                Dd = D.copy()
                Dd[a, b] += sgn * delta
                configs.append((pos @ Dd, cell @ Dd, types))
    for i in range(n):
        for c in range(3):
            for sgn in (1.0, -1.0):
                xt = pos.copy()
                xt[i, c] += sgn * delta
                configs.append((xt @ D, cell @ D, types))
    res = evaluate(configs, False)
    H = np.array([r["energy"] + p * det3(c[1]) for r, c in zip(res, configs)])
    V = det3(cell @ D)
    G = np.linalg.inv(D).T @ (sym(res[0]["virial"]) - p * V * np.eye(3)) / L
    ft = res[0]["f"] @ D.T
    Gd = -(H[1:19:2] - H[2:19:2]).reshape(3, 3) / (2.0 * delta * L)
    fd = -(H[19::2] - H[20::2]).reshape(n, 3) / (2.0 * delta)
    return G, ft, Gd, fd, res[0]


@pytest.mark.gpu
@pytest.mark.parametrize("fname,cell_fn", [("W_L8.mtp", _cells.cubic2_cell), ("WRe_L20.mtp", _cells.tilted5_cell)])
def test_generalised_forces_are_the_gradient_of_the_enthalpy(fname, cell_fn):
    """G and ft as mtp_relax_cell_step makes them (read back from its outputs after one step from rest: gcell, and the kicks
    vq = (dt ftm2v / cell_mass) G, vt = (dt ftm2v / m) ft) against central differences (delta = 1e-5) of E + p V from
    md.evaluate_cells in D and in xt, at a random D within 1e-2 of I and p = 3 GPa.  The bound is 100 times the discrepancy the CPU
    oracle's own virial and forces show against the same differences of its own energy on the same cells."""
    import torch
    pos, cell, types = cell_fn()
    n = len(pos)
    D = np.eye(3) + np.random.default_rng(31).uniform(-1e-2, 1e-2, (3, 3))
    p = 3.0 * GPA
    ctx = _ctx(fname)
    Go, fo, God, fod, _ = _generalised(oracle_evaluate(fname), pos, cell, types, D, p)
    own_G, own_f = np.abs(Go - God).max() / np.abs(God).max(), np.abs(fo - fod).max() / np.abs(fod).max()
    Ge, fe, Gd, fd, r0 = _generalised(_relax_vc.evaluate_with(ctx, LIST_CUTOFF), pos, cell, types, D, p)
    # the kernel, one step from rest on the device's own f and W
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    masses = MASSES[2]
    dt, cell_mass = 1e-3, 150.0
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    eye = np.eye(3).reshape(1, 9)
    A = dict(cfg_first=to(np.array([0, n], dtype=np.int32)), x=to(pos @ D), xt=to(pos), vt=z(n, 3), f=to(r0["f"]), type=to(types),
             inv_mass=to(1.0 / masses), virial=to(r0["virial"].reshape(1, 6)), h0=to(cell.reshape(1, 9)), origins=z(1, 3),
             D=to(D.reshape(1, 9)), vq=z(1, 9), Dbinv=to(eye), href=to(cell.reshape(1, 9)), nimg=to(np.full((1, 3), 2, dtype=np.int32)),
             dt=to(np.array([dt])), alpha=to(np.array([0.1])), npos=to(np.zeros(1, dtype=np.int32)), frozen=to(np.zeros(1, dtype=np.int32)),
             done_step=to(np.full(1, -1, dtype=np.int32)), fmax=z(1), smax=z(1), gcell=z(1, 9), h=to(cell.reshape(1, 9)), T=to(eye),
             cellmove=z(1), counts=to(np.zeros(3, dtype=np.int32)))
    capi.relax_cell_step(1, _params(cell_mass=cell_mass, pressure=p, ftol=0.0, stol=0.0), 0, A, stream=st)
    torch.cuda.synchronize()
    Gk = A["gcell"].cpu().numpy().reshape(3, 3)
    Gkick = A["vq"].cpu().numpy().reshape(3, 3) * cell_mass / (dt * _sample.FTM2V)
    fk = A["vt"].cpu().numpy() * masses[types - 1][:, None] / (dt * _sample.FTM2V)
    assert np.array_equal(A["xt"].cpu().numpy(), pos) and A["frozen"].item() == 0      # from rest: v' = 0, nothing moved
    eG, eGk = np.abs(Gk - Gd).max() / np.abs(Gd).max(), np.abs(Gkick - Gk).max() / np.abs(Gk).max()
    ef = np.abs(fk - fd).max() / np.abs(fd).max()
    print("%s, %d atoms: oracle against its own differences: G %.3e ft %.3e relative; kernel against the device's: G %.3e ft %.3e; "
          "kick against gcell %.3e; kernel against numpy on the same f, W: G %.3e ft %.3e"
          % (fname, n, own_G, own_f, eG, ef, eGk, np.abs(Gk - Ge).max() / np.abs(Ge).max(), np.abs(fk - fe).max() / np.abs(fe).max()))
    assert eG <= 100.0 * own_G and ef <= 100.0 * own_f
    assert eGk <= 1e-12 and np.abs(Gk - Ge).max() <= 1e-12 * np.abs(Ge).max() and np.abs(fk - fe).max() <= 1e-12 * np.abs(fe).max()


# ---- the whole loop ------------------------------------------------------------------------------------------------------

POTS = [("W_L8.mtp", 1), ("WRe_L20.mtp", 2)]
GRADED = [("W_L16_nbh.almtp", 1), ("WRe_L10_cfg.almtp", 2)]


def _cell_diff(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_relax_cells_vc_follows_the_host_driven_loop(fname, species):
    """the batch of the fixed-cell test, 12 steps with dmax = 0.02 A at p = 1 GPa (the shape of DESIGN.md 5.3.6: no atom travels
    further than 0.42 A, and |dD| <= 0.02 / n a step, so nothing reaches the short distances where the generated potentials have
    holes).  every=5: the re-layout at a rebuild runs twice."""
    from lammps_mtp_kokkos_amd.md import relax_cells_vc
    batch = _batch.mixed_batch(species)
    ctx = _ctx(fname)
    p = 1.0 * GPA
    ref = _relax_vc.reference_loop(_relax_vc.evaluate_with(ctx, LIST_CUTOFF), batch, 12, masses=MASSES[species], dmax=0.02, pressure=p)
    ref["twin"].assert_margins()
    got = relax_cells_vc(ctx, batch, 12, pressure=p, masses=MASSES[species], dmax=0.02, every=5, list_cutoff=LIST_CUTOFF, trace=True)
    assert got["steps_done"] == ref["steps_done"] == 12 and got["records"] == [] and got["candidates"] == [] and got["dropped"] == 0
    assert got["builds"] >= 3
    worst = [0.0] * 6
    for k, (pos, cell, _) in enumerate(batch):
        f = got["final"][k]
        dx = _sample.wrapped_diff(f["x"], ref["final_x"][k], ref["final_cell"][k])
        dh = _cell_diff(f["cell"], ref["final_cell"][k])
        de = float(np.abs(got["trace"]["energy"][:, k] - ref["energy"][:, k]).max())
        df = float(np.abs(got["trace"]["fmax"][:, k] - ref["fmax"][:, k]).max())
        ds = float(np.abs(got["trace"]["smax"][:, k] - ref["smax"][:, k]).max())
        dv = float(np.abs(got["trace"]["volume"][:, k] - ref["volume"][:, k]).max())
        print("%s, configuration %d (%d atoms): dx %.3e dcell %.3e dE %.3e dfmax %.3e dsmax %.3e dV %.3e, %s at %d; cell moved %.3e A"
              % (fname, k, len(pos), dx, dh, de, df, ds, dv, f["status"], f["step"], _cell_diff(f["cell"], cell)))
        worst = [max(a, b) for a, b in zip(worst, (dx, dh, de, df, ds, dv))]
        assert f["x"].shape == (len(pos), 3) and f["cell"].shape == (3, 3) and f["virial"].shape == (6,)
        assert f["status"] == capi.RELAX_STATUS[ref["status"][k]] and f["step"] == ref["done_step"][k]
        assert abs(f["dt"] - ref["dt"][k]) <= 1e-12 * ref["dt"][k] and abs(f["fmax"] - ref["fmax"][-1, k]) < V_TOL
        assert abs(f["energy"] - ref["energy"][-1, k]) < E_TOL and abs(f["volume"] - det3(ref["final_cell"][k])) < 1e-8
        assert abs(f["enthalpy"] - (f["energy"] + p * f["volume"])) < 1e-12 and np.abs(f["virial"] - ref["virial"][k]).max() < E_TOL
        assert abs(f["smax"] - ref["smax"][-1, k]) < V_TOL
    # positions and cells 1e-10 A, energies 1e-8 eV, forces 1e-9 eV/A; smax [eV/A^3] as the forces, volumes [A^3] as the energies
    assert worst[0] < X_TOL and worst[1] < X_TOL and worst[2] < E_TOL and worst[3] < V_TOL and worst[4] < V_TOL and worst[5] < E_TOL, worst
    empty = got["final"][3]
    assert empty["status"] == "running" and empty["x"].shape == (0, 3) and empty["energy"] == 0.0 and np.array_equal(empty["cell"], batch[3][1])
    moved = max(_cell_diff(got["final"][k]["cell"], batch[k][1]) for k in (0, 1, 2, 4, 5))
    assert moved > 1e-3                                                              # (the minimiser did move the cells)
    h0 = ref["energy"][0] + p * ref["volume"][0]
    h1 = ref["energy"][-1] + p * ref["volume"][-1]
    assert (h1[[0, 1, 2, 4, 5]] < h0[[0, 1, 2, 4, 5]]).all()                         # (downhill in the enthalpy)
    with pytest.raises(capi.MtpError) as ei:                                         # no selection state
        relax_cells_vc(ctx, batch, 1, threshold_break=5.0)
    assert ei.value.code == -23


@pytest.mark.gpu
def test_with_the_cell_masked_out_relax_cells_comes_back():
    from lammps_mtp_kokkos_amd.md import relax_cells, relax_cells_vc
    batch = _batch.mixed_batch(1)
    ctx = _ctx("W_L8.mtp")
    kw = dict(masses=MASSES[1], dmax=0.02, every=5, list_cutoff=LIST_CUTOFF)
    want = relax_cells(ctx, batch, 12, **kw)
    got = relax_cells_vc(ctx, batch, 12, cell_mask=(0, 0, 0, 0, 0, 0), pressure=1.0 * GPA, **kw)
    assert got["steps_done"] == want["steps_done"] and got["builds"] == want["builds"]
    for k, (pos, cell, _) in enumerate(batch):
        f, w = got["final"][k], want["final"][k]
        dx = _sample.wrapped_diff(f["x"], w["x"], cell)
        print("configuration %d: dx %.3e, %s at %d" % (k, dx, f["status"], f["step"]))
        assert dx < X_TOL and f["status"] == w["status"] and f["step"] == w["step"] and np.array_equal(f["cell"], cell)
        assert abs(f["energy"] - w["energy"]) < E_TOL and abs(f["fmax"] - w["fmax"]) < V_TOL and f["smax"] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("isotropic", [True, False], ids=["isotropic", "full-mask"])
def test_the_bcc_cell_relaxes_to_its_lattice_parameter_and_ends_early(isotropic):
    """the perfect 2-atom bcc cell under W_L16.mtp from a = 3.482 A (tests/test_relax_vc_cpu.py confirms with the CPU oracle that
    the twin converges from there, near 3.576 A): the device run converges at the step of the host-driven loop, lattice parameters
    to 1e-8 A; under 10 GPa it ends at a smaller volume with W / V = p I within stol."""
    from lammps_mtp_kokkos_amd.md import relax_cells_vc
    ctx = _ctx("W_L16.mtp")
    batch = [bcc2(), _batch.empty_cell()]
    kw = dict(isotropic=isotropic, stol=1e-5)
    volumes = {}
    for p in (0.0, 10.0 * GPA):
        ref = _relax_vc.reference_loop(_relax_vc.evaluate_with(ctx, LIST_CUTOFF), batch, 400, pressure=p, **kw)
        ref["twin"].assert_margins()
        done = int(ref["done_step"][0])
        assert ref["status"][0] == _relax_vc.CONVERGED and 0 < done < 400
        got = relax_cells_vc(ctx, batch, 400, pressure=p, list_cutoff=LIST_CUTOFF, **kw)
        f = got["final"][0]
        a, aw = np.sqrt((f["cell"] ** 2).sum(1)), np.sqrt((ref["final_cell"][0] ** 2).sum(1))
        print("p = %.4f eV/A^3: converged at step %d (host-driven loop: %d), steps_done %d, builds %d, a = %r (differs by %.3e A), V %.6f, "
              "W/V %r" % (p, f["step"], done, got["steps_done"], got["builds"], a, np.abs(a - aw).max(), f["volume"], f["virial"] / f["volume"]))
        assert f["status"] == "converged" and f["step"] == done and done <= got["steps_done"] <= done + 4 < 400
        assert np.abs(a - aw).max() < 1e-8 and _cell_diff(f["cell"], ref["final_cell"][0]) < 1e-8
        assert np.abs(sym(f["virial"]) / f["volume"] - p * np.eye(3)).max() <= 1e-5 and f["smax"] <= 1e-5 and f["fmax"] <= 1e-3
        assert abs(f["energy"] - ref["energy"][-1, 0]) < E_TOL
        assert got["final"][1]["status"] == "running" and got["final"][1]["volume"] == det3(batch[1][1])
        volumes[p] = f["volume"]
        if p == 0.0:
            assert np.abs(a - 3.576).max() < 5e-3 and abs(f["energy"] + 37.5) < 0.1
    assert volumes[10.0 * GPA] < volumes[0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", GRADED)
def test_candidates_carry_the_cell_they_were_graded_in(fname, species):
    """grade steps 0, 4, 8, 12 under cell relaxation, thresholds as in tests/test_relax_gpu.py; every=5, so that lists and layout
    are rebuilt between captures.  Every candidate is (positions, the cell of its captured step, types) of the host-driven loop,
    and select_cells takes the list and finds the grades again."""
    from lammps_mtp_kokkos_amd.md import relax_cells_vc, select_cells
    batch = _batch.mixed_batch(species)
    natoms = [len(c[0]) for c in batch]
    ctx = _ctx(fname, True)
    ev = _relax_vc.evaluate_with(ctx, LIST_CUTOFF)
    kw = dict(masses=MASSES[species], dmax=0.02, grade_every=4, pressure=1.0 * GPA)
    table = _relax_vc.reference_loop(ev, batch, 12, select=BIG, brk=BIG, **kw)["grades"]
    assert sorted(table) == [0, 4, 8, 12]
    select, brk = sorted([_midpoint_threshold(table, natoms), _midpoint_threshold(table, natoms, central=True)])
    ref = _relax_vc.reference_loop(ev, batch, 12, select=select, brk=brk, **kw)
    ref["twin"].assert_margins()
    want = ref["capture"].records
    print("threshold_select %.9g threshold_break %.9g records" % (select, brk), want, "status", ref["status"])
    assert len(want) > 0 and (ref["status"] == _relax_vc.CAPTURED).any(), "the test's inputs are wrong: nothing is captured and frozen"
    assert any(s > 0 for _, s, _ in want), "the test's inputs are wrong: every capture is at step 0, in the cells given"
    got = relax_cells_vc(ctx, batch, 12, threshold_select=select, threshold_break=brk, every=5, list_cutoff=LIST_CUTOFF, **kw)
    assert got["dropped"] == 0 and got["builds"] >= 3
    assert [(k, s) for k, s, _ in got["records"]] == [(k, s) for k, s, _ in want]
    assert [f["status"] for f in got["final"]] == [capi.RELAX_STATUS[q] for q in ref["status"]]
    for (k, s, g), (_, _, gw), (pos, cell, types), (xs, hs) in zip(got["records"], want, got["candidates"], ref["snapshots"]):
        assert abs(g - gw) <= 1e-9 * max(1.0, abs(gw)), (k, s, g, gw)
        dh = _cell_diff(cell, hs)
        print("candidate of configuration %d at step %d: cell differs by %.3e A from the loop's, by %.3e A from the cell given"
              % (k, s, dh, _cell_diff(cell, batch[k][1])))
        assert dh < X_TOL and _sample.wrapped_diff(pos, xs, hs) < 1e-9 and np.array_equal(types, batch[k][2])
        assert np.array_equal(cell, batch[k][1]) == (s == 0)
    for k, (pos, _, _) in enumerate(batch):
        f = got["final"][k]
        if len(pos):
            assert _sample.wrapped_diff(f["x"], ref["final_x"][k], ref["final_cell"][k]) < X_TOL and _cell_diff(f["cell"], ref["final_cell"][k]) < X_TOL
    sel = select_cells(ctx, got["candidates"], threshold=1.1, list_cutoff=LIST_CUTOFF, max_swaps=0)
    for gb, (_, _, g) in zip(sel["grade_before"], got["records"]):
        assert abs(gb - g) <= 1e-9 * max(1.0, g)


@pytest.mark.gpu
@pytest.mark.parametrize("graded", [False, True], ids=["plain", "graded"])
def test_a_batch_split_into_passes_has_the_run_of_the_whole_batch(graded):
    """tests/_passes.py.  plain: the run of test_relax_cells_vc_follows_the_host_driven_loop; graded: potential and thresholds
    of the capture test, max_candidates at its default (nothing is dropped).  every=20 is beyond the run; whether the moving
    cells make a pass rebuild is the pass's own affair, so the builds are those of the passes' configurations run alone.  A
    candidate carries the cell of its graded step.  Slot translation costs bits: the bounds are those of the host-driven-loop
    test."""
    import _passes
    from lammps_mtp_kokkos_amd.md import relax_cells_vc
    fname, species = GRADED[0] if graded else POTS[0]
    batch = _batch.mixed_batch(species)
    ctx = _ctx(fname, graded)
    kw = dict(masses=MASSES[species], dmax=0.02, pressure=1.0 * GPA)
    if graded:
        kw["grade_every"] = 4
        natoms = [len(c[0]) for c in batch]
        table = _relax_vc.reference_loop(_relax_vc.evaluate_with(ctx, LIST_CUTOFF), batch, 12, select=BIG, brk=BIG, **kw)["grades"]
        select, brk = sorted([_midpoint_threshold(table, natoms), _midpoint_threshold(table, natoms, central=True)])
        kw.update(threshold_select=select, threshold_break=brk)

    def run(a, b, cap):
        return relax_cells_vc(ctx, batch[a:b], 12, every=20, list_cutoff=LIST_CUTOFF, max_atoms_per_pass=cap, trace=True, **kw)

    def same_final(f, w, config):
        assert sorted(f) == sorted(w) and f["x"].shape == w["x"].shape == config[0].shape
        assert _sample.wrapped_diff(f["x"], w["x"], w["cell"]) < X_TOL and _cell_diff(f["cell"], w["cell"]) < X_TOL
        assert abs(f["energy"] - w["energy"]) < E_TOL and abs(f["fmax"] - w["fmax"]) < V_TOL and abs(f["smax"] - w["smax"]) < V_TOL
        assert abs(f["dt"] - w["dt"]) <= 1e-12 * w["dt"] and f["status"] == w["status"] and f["step"] == w["step"]
        assert np.abs(f["virial"] - w["virial"]).max() < E_TOL and abs(f["volume"] - w["volume"]) < 1e-8
        assert abs(f["enthalpy"] - w["enthalpy"]) < E_TOL

    def same_cell(got, want, given, step):
        assert _cell_diff(got, want) < X_TOL and np.array_equal(got, given) == (step == 0)

    whole, split = _passes.assert_split_runs_are_the_whole_run(run, batch, LIST_CUTOFF, same_final,
                                                               dict(energy=E_TOL, fmax=V_TOL, smax=V_TOL, volume=E_TOL), X_TOL, same_cell)
    assert whole["steps_done"] == 12 and graded == (len(whole["records"]) > 0)
    assert not graded or any(s > 0 for _, s, _ in whole["records"])
