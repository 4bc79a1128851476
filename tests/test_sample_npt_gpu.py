"""Batched constant-pressure sampling on the device (md.sample_cells_npt; mtp_sample_cell_step): the kernel alone against the
numpy twin of tests/_sample_npt.py on the analytic model of tests/_relax_vc.py (forces and virials made by the test between
launches from the device's own positions and cells), the barostat switched off against mtp_sample_initial to the bit, batch
independence to the bit, a bad virial, the argument errors; then the whole loop against the host-driven loop, the limit
tau_p = None against md.sample_cells, candidates with the cell of their graded step, and a batch split into passes.
Trajectory bounds are those of tests/test_sample_gpu.py; cells to 1e-10 relative."""
import functools

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

import _batch
import _relax_vc
import _sample
import _sample_npt
from _cells import LIST_CUTOFF
from _relax_vc import GPA
from _sample_npt import det3
from test_sample_gpu import BIG, E_TOL, MASSES, V_TOL, X_TOL, _ctx, _midpoint_threshold, _setup

SIZES = [0, 1, 63, 64, 65, 257]
FROZEN = np.array([0, 0, 0, 1, 0, 0], dtype=np.int32)               # the 64-atom configuration is frozen from the start
TEMPS = np.array([300.0, 900.0, 300.0, 900.0, 300.0, 900.0])
KEYS = np.array([2 ** 63 + 17, 5, 2 ** 40 + 3, 77, 2 ** 33, 123456789012345], dtype=np.uint64)
ORIGINS = np.random.default_rng(4).uniform(-60.0, 60.0, (6, 3))
SENTINEL = -77.0
DT, T_DAMP, SEED = 1e-3, 0.1, 0x1234567887654321
# the stiffest cell of the model (257 atoms: K2 |h|^4 of 4e5 eV) answers at M C dt = 0.04 a step with these
BARO = dict(pressure=2.0 * GPA, compressibility=0.01, tau_p=0.5)
MODES = dict(full=dict(), isotropic=dict(isotropic=True), diag=dict(cell_mask=(1, 1, 1, 0, 0, 0), strain_max=1.5e-4))
KEEP = (10, 29, 199)
PER_ROW = ("x", "v")
PER_CFG = ("h", "T", "cellmove", "press")
INTS = ("frozen", "done_step", "capped")


def _model(sizes=SIZES):
    return _relax_vc.Model(sizes=sizes, k_cfg=_relax_vc.MODEL_K[: len(sizes)], seed=21)


def _velocities(model, temps):
    m = _relax_vc.MODEL_MASSES[model.types - 1]
    return np.random.default_rng(9).normal(size=(model.n, 3)) * np.sqrt(_sample.KB * temps[model.cfg] / (m * _sample.MVV2E))[:, None]


def _params(dt=DT, tau_p=0.5, compressibility=0.01, pressure=0.0, strain_max=0.01, cell_mask=(1, 1, 1, 1, 1, 1), isotropic=False,
            seed=SEED, dtf=None):
    return capi.sample_cell_params(dt, 0.5 * dt * _sample.FTM2V if dtf is None else dtf, tau_p, compressibility, pressure, strain_max,
                                   cell_mask, isotropic, seed)


def _device_arrays(model, temps, keys, frozen, origins, v0):
    """the arrays of mtp_sample_cell_step for the model, one row and one configuration more than the batch holds allocated and
    filled with a sentinel"""
    import torch
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ncfg = model.ncfg
    pad = lambda a: np.concatenate([a, np.full((1,) + a.shape[1:], SENTINEL, dtype=a.dtype)])
    eye = np.tile(np.eye(3).reshape(1, 9), (ncfg, 1))
    h0 = model.h0.reshape(ncfg, 9)
    nimg = np.array([_relax_vc.images(c, LIST_CUTOFF) for c in model.h0], dtype=np.int32).reshape(ncfg, 3)
    A = dict(cfg_first=to(model.cf), x=to(pad(model.x0 + origins[model.cfg])), v=to(pad(v0)), f=to(pad(np.zeros_like(v0))),
             type=to(pad(model.types)), inv_mass=to(1.0 / _relax_vc.MODEL_MASSES), mass=to(_relax_vc.MODEL_MASSES),
             virial=to(np.zeros((ncfg, 6))), temperature=to(temps), key=to(keys.view(np.int64)), origins=to(origins),
             V0=to(det3(model.h0)), h=to(pad(h0)), T=to(pad(eye)), href=to(h0), nimg=to(nimg),
             frozen=to(pad(np.asarray(frozen, dtype=np.int32))), done_step=to(pad(np.full(ncfg, -1, dtype=np.int32))),
             cellmove=to(pad(np.zeros(ncfg))), capped=to(pad(np.zeros(ncfg, dtype=np.int32))), press=to(pad(np.zeros(ncfg))),
             counts=to(np.zeros(3, dtype=np.int32)))
    return A, to


def _device_model(model, steps, temps, keys, frozen, origins, poison=None, keep=(), v0=None, **kw):
    """step 0 (forces, thermostat force) and steps 1 .. steps of the sampler on the model: mtp_sample_cell_step, then x and h
    read back, the model in numpy, f and W uploaded, mtp_sample_final.  poison = (step, k, q, value) edits W in front of that
    step's launch.  Returns the arrays after the last step and copies of them after the steps of `keep`."""
    import torch
    st = capi.use_private_torch_stream(torch.device("cuda:0")).cuda_stream
    ncfg, n = model.ncfg, model.n
    A, to = _device_arrays(model, temps, keys, frozen, origins, _velocities(model, temps) if v0 is None else v0)
    par = _params(**kw)
    row_cfg = to(model.cfg.astype(np.int32))

    def forces():
        torch.cuda.synchronize()
        xh, hh = A["x"].cpu().numpy()[:n], A["h"].cpu().numpy()[:ncfg].reshape(ncfg, 3, 3)
        with np.errstate(all="ignore"):
            _, f, W = model.all(xh, hh, origins)
        A["f"][:n] = to(f)
        A["virial"].copy_(to(W))

    def second_half(step, kick):
        capi.sample_final(n, row_cfg, A["cfg_first"], A["frozen"], A["v"], A["f"], A["type"], A["mass"], A["inv_mass"],
                          A["temperature"], A["key"], SEED, step, kick, DT, T_DAMP, stream=st)

    def state():
        torch.cuda.synchronize()
        return {k: A[k].cpu().numpy() for k in PER_ROW + PER_CFG + INTS + ("counts",)}

    forces()
    second_half(0, 0.0)
    kept = {}
    for s in range(1, steps + 1):
        if poison is not None and poison[0] == s:
            A["virial"][poison[1], poison[2]] = poison[3]
        capi.sample_cell_step(ncfg, par, s, A, stream=st)
        forces()
        second_half(s, par.dtf)
        if s in keep:
            kept[s] = state()
    out = state()
    for k in PER_ROW:                                                                # nothing behind the last row ...
        assert (out[k][n:] == SENTINEL).all(), k
    for k in PER_CFG + INTS:                                                         # ... or the last configuration
        assert (out[k][ncfg:] == SENTINEL).all(), k
    return out, kept


def _twin_model(model, steps, temps, keys, frozen, origins, poison=None, keep=(), dt=DT, **kw):
    """the same run by the twin"""
    n = model.n
    m, inv_m = _relax_vc.MODEL_MASSES[model.types - 1], model.inv_m
    twin = _sample_npt.Twin(model.cf, model.h0, temps, keys, dt, kw.pop("pressure", 0.0), kw.pop("compressibility", 0.01), seed=SEED,
                            origins=origins, frozen=frozen, rghost=LIST_CUTOFF, **kw)
    x, v = model.x0 + origins[model.cfg], _velocities(model, temps)
    index = np.concatenate([np.arange(s) for s in np.diff(model.cf)]).astype(np.uint64)
    key_row, T_row = keys[model.cfg], temps[model.cfg]
    _, f, W = model.all(x, twin.h, origins)
    _sample.second_half(v, f, m, inv_m, T_row, T_DAMP, dt, 0.0, 0, index, key_row, SEED, twin.frozen[model.cfg] == 0)
    kept = {}
    for s in range(1, steps + 1):
        if poison is not None and poison[0] == s:
            W[poison[1], poison[2]] = poison[3]
        twin.step(s, x, v, f, W, m, inv_m)
        with np.errstate(all="ignore"):
            _, f, W = model.all(x, twin.h, origins)
        _sample.second_half(v, f, m, inv_m, T_row, T_DAMP, dt, twin.dtf, s, index, key_row, SEED, twin.frozen[model.cfg] == 0)
        if s in keep:
            kept[s] = dict(x=x.copy(), v=v.copy(), h=twin.h.copy(), T=twin.T.copy(), cellmove=twin.cellmove.copy(), press=twin.press.copy(),
                           frozen=twin.frozen.copy(), done_step=twin.done_step.copy(), capped=twin.capped.copy())
    return twin, kept


@functools.lru_cache(maxsize=None)
def _batch_run(mode):
    """the batch of the kernel tests on the device, 200 steps, with its state after the steps of KEEP: made once, never written to"""
    return _device_model(_model(), 200, TEMPS, KEYS, FROZEN, ORIGINS, keep=KEEP, **BARO, **MODES[mode])


def _rel(got, want):
    if not np.size(want):
        return 0.0
    scale, err = float(np.abs(want).max()), float(np.abs(np.asarray(got).reshape(np.shape(want)) - want).max())
    return err / scale if scale > 0.0 else err


# ---- the kernel alone ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_kernel_alone_follows_the_twin_on_the_model_for_200_steps(mode):
    """configurations of 0, 1, 63, 64, 65 and 257 atoms: the lane and wavefront widths and both sides of the switch from a
    wavefront to the workgroup; two temperatures, two masses, slot origins up to 60 A, the 64-atom one frozen from the start,
    p = 2 GPa.  Modes: all six components, isotropic, and the diagonal alone with strain_max = 1.5e-4, which caps (no component of
    the run comes within 1e-6 relative of that tie).  Only rounding separates device and twin: 1e-12 of the largest entry, the
    bound of the other kernel-alone tests."""
    model = _model()
    n, ncfg = model.n, model.ncfg
    twin, kept = _twin_model(model, 200, TEMPS, KEYS, FROZEN, ORIGINS, keep=(199,), **BARO, **MODES[mode])
    want = kept[199]
    got = _batch_run(mode)[1][199]
    assert twin.margin_cap >= 1e-6, "the test's inputs are wrong: a strain component ties with strain_max"
    errs = {k: _rel(got[k][:n], want[k]) for k in PER_ROW}
    errs.update({k: _rel(got[k][:ncfg], want[k]) for k in ("h", "T", "press")})
    move = float(np.abs(got["cellmove"][:ncfg] - want["cellmove"]).max())
    print(mode, " ".join("%s %.2e" % kv for kv in errs.items()), "cellmove %.2e A" % move, "capped", want["capped"],
          "largest |F - I| %.2e" % np.abs(twin.F - np.eye(3)).max())
    assert all(e <= 1e-12 for e in errs.values()), errs
    assert move <= 1e-12 * 4.0 * float(np.abs(want["h"]).max()) * 3
    for k in INTS:
        assert np.array_equal(got[k][:ncfg], want[k]), k
    assert list(got["counts"]) == [0, 0, 0] and not twin.frozen[[0, 1, 2, 4, 5]].any()
    assert (mode == "diag") == bool(want["capped"].any())
    assert np.abs(twin.F[[1, 2, 4, 5]] - np.eye(3)).max() > 1e-5                      # (the cells did move)
    # the frozen and the empty configuration: bitwise untouched
    a, b = int(model.cf[3]), int(model.cf[4])
    assert np.array_equal(got["x"][a:b], model.x0[a:b] + ORIGINS[3]) and np.array_equal(got["v"][a:b], _velocities(model, TEMPS)[a:b])
    for k in (0, 3):
        assert np.array_equal(got["h"][k], model.h0[k].reshape(9)) and np.array_equal(got["T"][k], np.eye(3).reshape(9))
        assert got["cellmove"][k] == 0.0 and got["press"][k] == 0.0 and got["capped"][k] == 0 and got["done_step"][k] == -1
    off = ~np.eye(3, dtype=bool).reshape(9)
    if mode != "full":                                                               # T = prod E: diagonal to the bit
        assert (got["T"][[1, 2, 4, 5]][:, off] == 0.0).all()
    if mode == "isotropic":
        assert (got["T"][:, 0] == got["T"][:, 4]).all() and (got["T"][:, 0] == got["T"][:, 8]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("off", [dict(tau_p=None), dict(tau_p=float("nan")), dict(tau_p=-1.0), dict(cell_mask=(0, 0, 0, 0, 0, 0))],
                         ids=["tau_p-none", "tau_p-nan", "tau_p-negative", "zero-mask"])
def test_with_the_barostat_off_the_rows_are_bitwise_those_of_sample_initial(off):
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    model = _model()
    n, ncfg = model.n, model.ncfg
    rng = np.random.default_rng(2)
    v0 = _velocities(model, TEMPS)
    A, to = _device_arrays(model, TEMPS, KEYS, FROZEN, ORIGINS, v0)
    row_cfg = to(model.cfg.astype(np.int32))
    xb, vb = A["x"].clone(), A["v"].clone()
    before = {k: A[k].clone() for k in ("h", "T", "cellmove", "capped", "done_step", "frozen", "counts")}
    par = _params(pressure=1.0 * GPA, **off)
    for step in range(1, 6):
        A["f"][:n] = to(rng.normal(0.0, 1.5, (n, 3)))
        A["virial"].copy_(to(rng.normal(0.0, 5.0, (ncfg, 6))))
        capi.sample_cell_step(ncfg, par, step, A, stream=st)
        capi.sample_initial(n, row_cfg, A["frozen"], xb, vb, A["f"], A["type"], A["inv_mass"], par.dtf, DT, stream=st)
    torch.cuda.synchronize()
    assert torch.equal(A["x"], xb) and torch.equal(A["v"], vb)
    moving = FROZEN[model.cfg] == 0
    assert not np.array_equal(xb.cpu().numpy()[:n][moving], (model.x0 + ORIGINS[model.cfg])[moving])
    for k, t in before.items():
        assert torch.equal(A[k], t), k
    press = A["press"].cpu().numpy()
    assert press[[1, 2, 4, 5]].all() and press[0] == 0.0 and press[3] == 0.0 and press[6] == SENTINEL


@pytest.mark.gpu
def test_a_configuration_alone_has_the_bits_it_has_in_the_batch():
    model = _model()
    batch = _batch_run("full")[1][29]
    for k in range(6):
        a, b = int(model.cf[k]), int(model.cf[k + 1])
        one, _ = _device_model(model.take(k), 29, TEMPS[k: k + 1], KEYS[k: k + 1], FROZEN[k: k + 1], ORIGINS[k: k + 1],
                               v0=_velocities(model, TEMPS)[a:b], **BARO)
        for key in PER_ROW:
            assert np.array_equal(one[key][: b - a], batch[key][a:b]), (k, key)
        for key in PER_CFG + INTS:
            assert np.array_equal(one[key][0], batch[key][k]), (k, key)
    assert not np.array_equal(batch["h"][5], model.h0[5].reshape(9))


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [(4, 4, 5, float("nan")), (4, 5, 0, float("inf"))], ids=["nan-virial", "inf-virial-workgroup"])
def test_a_bad_virial_fails_its_configuration_and_writes_to_no_other(poison):
    model = _model()
    kf = poison[1]
    a, b = int(model.cf[kf]), int(model.cf[kf + 1])
    got, kept = _device_model(model, 10, TEMPS, KEYS, FROZEN, ORIGINS, poison=poison, keep=(3,), **BARO)
    twin, _ = _twin_model(model, 10, TEMPS, KEYS, FROZEN, ORIGINS, poison=poison, **BARO)
    clean = _batch_run("full")[1][10]
    assert got["frozen"][kf] == _relax_vc.FAILED and got["done_step"][kf] == 4
    assert np.array_equal(got["frozen"][:6], twin.frozen) and np.array_equal(got["done_step"][:6], twin.done_step)
    before = kept[3]
    for key in PER_ROW:                                                              # none of its rows or cell state is written
        assert np.array_equal(got[key][a:b], before[key][a:b]), key
    for key in ("h", "T", "cellmove", "press", "capped"):
        assert np.array_equal(got[key][kf], before[key][kf]), key
    others = np.ones(model.n + 1, dtype=bool)
    others[a:b] = False
    ok = np.arange(7) != kf
    for key in PER_ROW:
        assert np.array_equal(got[key][others], clean[key][others]), key
    for key in PER_CFG + INTS:
        assert np.array_equal(got[key][ok], clean[key][ok]), key
    assert list(got["counts"]) == [0, 0, 1] and list(clean["counts"]) == [0, 0, 0]


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    model = _relax_vc.Model(sizes=[3, 70], k_cfg=(2.0, 5.0))
    temps, keys = TEMPS[:2], KEYS[:2]
    A, to = _device_arrays(model, temps, keys, np.zeros(2), ORIGINS[:2], _velocities(model, temps))
    rng = np.random.default_rng(0)
    A["f"][: model.n] = to(rng.normal(size=(model.n, 3)))
    A["virial"].copy_(to(rng.normal(size=(2, 6))))
    before = {k: t.clone() for k, t in A.items()}

    def call(stream=st, step=1, arrays=None, **kw):
        capi.sample_cell_step(2, _params(**kw), step, A if arrays is None else arrays, stream=stream)

    nan, inf = float("nan"), float("inf")
    bad = [dict(stream=None), dict(step=-1), dict(dt=0.0), dict(dt=-1e-3), dict(dt=nan), dict(dt=inf), dict(dtf=nan), dict(pressure=nan),
           dict(pressure=inf), dict(compressibility=0.0), dict(compressibility=-1.0), dict(compressibility=nan), dict(compressibility=inf),
           dict(strain_max=0.0), dict(strain_max=-0.01), dict(strain_max=0.0500001), dict(strain_max=nan),
           dict(cell_mask=(1, 1, 1, 2, 0, 0)), dict(cell_mask=(-1, 1, 1, 0, 0, 0)), dict(isotropic=True, cell_mask=(1, 0, 1, 0, 0, 0))]
    for kw in bad:
        with pytest.raises(capi.MtpError) as ei:
            call(**kw)
        assert ei.value.code == -20, kw
    for missing in capi.SAMPLE_CELL_ARRAYS:                                          # a missing array, each of them
        with pytest.raises(capi.MtpError) as ei:
            call(arrays={k: t for k, t in A.items() if k != missing})
        assert ei.value.code == -20, missing
    torch.cuda.synchronize()
    for k, t in A.items():
        assert torch.equal(t, before[k]), k
    call(strain_max=0.05, pressure=-1.0 * GPA, isotropic=True)                       # the ends of the ranges are inside
    torch.cuda.synchronize()
    assert not torch.equal(A["v"], before["v"]) and not torch.equal(A["h"], before["h"])


# ---- the whole loop ------------------------------------------------------------------------------------------------------

POTS = [("W_L8.mtp", 1), ("WRe_L20.mtp", 2)]
GRADED = [("W_L16_nbh.almtp", 1), ("WRe_L10_cfg.almtp", 2)]
# tungsten: a bulk modulus of 310 GPa is a compressibility of 0.52 A^3/eV; tau_p = 0.1 ps moves the cells by 1e-3 a step
NPT = dict(pressure=1.0 * GPA, compressibility=0.52, tau_p=0.1)


def _cell_rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _npt(fname, selection, species, T, dt, steps, lo=0, hi=None, **kw):
    from lammps_mtp_kokkos_amd.md import sample_cells_npt
    batch, keys, temps, vel = _setup(species, T)
    kw = dict(dict(every=3), **kw)
    return sample_cells_npt(_ctx(fname, selection), batch[lo:hi], temps[lo:hi], NPT["pressure"], steps, dt,
                            compressibility=NPT["compressibility"], tau_p=kw.pop("tau_p", NPT["tau_p"]), t_damp=0.1, seed=5, keys=keys[lo:hi],
                            masses=MASSES[species], velocities=vel[lo:hi], list_cutoff=LIST_CUTOFF, **kw)


def _npt_reference(fname, selection, species, T, dt, steps, **kw):
    batch, keys, temps, vel = _setup(species, T)
    return _sample_npt.reference_loop(_relax_vc.evaluate_with(_ctx(fname, selection), LIST_CUTOFF), batch, temps, NPT["pressure"], steps, dt,
                                      vel, keys, MASSES[species], NPT["compressibility"], NPT["tau_p"], t_damp=0.1, seed=5,
                                      rghost=LIST_CUTOFF, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_sample_cells_npt_follows_the_host_driven_loop(fname, species):
    """the batch of tests/test_sample_gpu.py (cubic, tilted and sub-cutoff cells, the empty configuration), 10 steps at 300 K and
    1 GPa; every=3: lists and layout are rebuilt for the moved cells three times"""
    batch = _batch.mixed_batch(species)
    ref = _npt_reference(fname, False, species, 300.0, 1e-3, 10)
    got = _npt(fname, False, species, 300.0, 1e-3, 10, trace=True)
    assert got["steps_done"] == 10 and got["records"] == [] and got["candidates"] == [] and got["dropped"] == 0
    assert got["builds"] >= 4 and not got["frozen"].any()
    worst = [0.0] * 6
    for k, (pos, cell, _) in enumerate(batch):
        f = got["final"][k]
        dx = _sample.wrapped_diff(f["x"], ref["x"][10][k], ref["cells"][10][k])
        dv = float(np.abs(f["v"] - ref["v"][10][k]).max()) if len(pos) else 0.0
        dh = _cell_rel(f["cell"], ref["cells"][10][k])
        de = float(np.abs(got["trace"]["energy"][:, k] + got["trace"]["kinetic"][:, k] - ref["energy"][:, k] - ref["kinetic"][:, k]).max())
        dvol = float(np.abs(got["trace"]["volume"][:, k] - ref["volume"][:, k]).max())
        dp = float(np.abs(got["trace"]["pressure"][:, k] - ref["pressure"][:, k]).max())
        print("%s, configuration %d (%d atoms): dx %.3e dv %.3e dcell %.3e (relative) dE %.3e dV %.3e dp %.3e; cell moved %.3e A, capped %d"
              % (fname, k, len(pos), dx, dv, dh, de, dvol, dp, np.abs(f["cell"] - cell).max(), f["capped"]))
        worst = [max(a, b) for a, b in zip(worst, (dx, dv, dh, de, dvol, dp))]
        assert f["x"].shape == (len(pos), 3) and f["cell"].shape == (3, 3) and f["virial"].shape == (6,) and f["status"] == "running"
        assert f["step"] == -1 and f["capped"] == ref["twin"].capped[k] and abs(f["volume"] - det3(ref["cells"][10][k])) < 1e-8
        assert np.abs(f["virial"] - ref["virial"][k]).max() < E_TOL and abs(f["pressure"] - ref["pressure"][10][k]) < V_TOL
        assert abs(f["energy"] - ref["energy"][10][k]) < E_TOL
    # positions 1e-10 A, velocities 1e-9, cells 1e-10 relative, energies 1e-8 eV; volumes [A^3] as the energies, pressures
    # [eV/A^3] as the velocities
    assert worst[0] < X_TOL and worst[1] < V_TOL and worst[2] < 1e-10 and worst[3] < E_TOL and worst[4] < E_TOL and worst[5] < V_TOL, worst
    moved = min(np.abs(got["final"][k]["cell"] - batch[k][1]).max() for k in (0, 1, 2, 4, 5))
    assert moved > 1e-4                                                              # (the barostat did move every cell)
    empty = got["final"][3]
    assert empty["x"].shape == (0, 3) and np.array_equal(empty["cell"], batch[3][1]) and empty["pressure"] == 0.0
    with pytest.raises(capi.MtpError) as ei:                                         # no selection state
        _npt(fname, False, species, 300.0, 1e-3, 1, threshold_select=2.0)
    assert ei.value.code == -23


@pytest.mark.gpu
def test_with_tau_p_none_the_trajectory_is_that_of_sample_cells():
    from lammps_mtp_kokkos_amd.md import sample_cells
    fname, species = POTS[0]
    batch, keys, temps, vel = _setup(species, 300.0)
    want = sample_cells(_ctx(fname), batch, temps, 10, 1e-3, t_damp=0.1, seed=5, keys=keys, masses=MASSES[species], velocities=vel,
                        list_cutoff=LIST_CUTOFF, every=3, trace=True)
    got = _npt(fname, False, species, 300.0, 1e-3, 10, tau_p=None, trace=True)
    assert got["steps_done"] == want["steps_done"] == 10 and got["builds"] == want["builds"]
    bits = True
    for k, (pos, cell, _) in enumerate(batch):
        f, w = got["final"][k], want["final"][k]
        dx = _sample.wrapped_diff(f["x"], w["x"], cell)
        dv = float(np.abs(f["v"] - w["v"]).max()) if len(pos) else 0.0
        de = float(np.abs(got["trace"]["energy"][:, k] - want["trace"]["energy"][:, k]).max())
        bits = bits and np.array_equal(f["x"], w["x"]) and np.array_equal(f["v"], w["v"])
        print("configuration %d: dx %.3e dv %.3e dE %.3e" % (k, dx, dv, de))
        assert dx < X_TOL and dv < V_TOL and de < E_TOL and np.array_equal(f["cell"], cell) and f["capped"] == 0
        assert abs(f["temperature"] - w["temperature"]) <= 1e-9 * max(1.0, w["temperature"])
    print("tau_p = None against sample_cells: bit-equal positions and velocities: %s" % bits)


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", GRADED)
def test_candidates_carry_the_cell_of_their_graded_step(fname, species):
    """the cold run of tests/test_sample_gpu.py (30 K, 0.25 fs, grade steps 0, 4, 8, 12) under the barostat; every=3, so that
    lists and layout are rebuilt between captures.  Every candidate is (positions, the cell of its captured step, types) of the
    host-driven loop, and select_cells finds the grades again."""
    from lammps_mtp_kokkos_amd.md import select_cells
    T, dt, steps = 30.0, 2.5e-4, 12
    batch = _batch.mixed_batch(species)
    natoms = [len(c[0]) for c in batch]
    table = _npt_reference(fname, True, species, T, dt, steps, grade_every=4, select=BIG, brk=BIG)["grades"]
    assert sorted(table) == [0, 4, 8, 12]
    select, brk = sorted([_midpoint_threshold(table, natoms), _midpoint_threshold(table, natoms, central=True)])
    ref = _npt_reference(fname, True, species, T, dt, steps, grade_every=4, select=select, brk=brk)
    want = ref["capture"].records
    print("threshold_select %.9g threshold_break %.9g records" % (select, brk), want, "status", ref["twin"].frozen)
    assert len(want) > 0 and any(s > 0 for _, s, _ in want), "the test's inputs are wrong: no capture after step 0"
    got = _npt(fname, True, species, T, dt, steps, grade_every=4, threshold_select=select, threshold_break=brk)
    assert got["dropped"] == 0 and got["builds"] >= 4
    assert [(k, s) for k, s, _ in got["records"]] == [(k, s) for k, s, _ in want]
    assert [f["status"] for f in got["final"]] == [capi.RELAX_STATUS[q] for q in ref["twin"].frozen]
    assert list(got["frozen"]) == list(ref["twin"].frozen != 0)
    for (k, s, g), (_, _, gw), (pos, cell, types), (xs, hs) in zip(got["records"], want, got["candidates"], ref["snapshots"]):
        assert abs(g - gw) <= 1e-9 * max(1.0, abs(gw)), (k, s, g, gw)
        print("candidate of configuration %d at step %d: cell differs by %.3e (relative) from the loop's, by %.3e A from the cell given"
              % (k, s, _cell_rel(cell, hs), np.abs(cell - batch[k][1]).max()))
        assert _cell_rel(cell, hs) < 1e-10 and _sample.wrapped_diff(pos, xs, hs) < 1e-9 and np.array_equal(types, batch[k][2])
        assert np.array_equal(cell, batch[k][1]) == (s == 0)
    sel = select_cells(_ctx(fname, True), got["candidates"], threshold=1.1, list_cutoff=LIST_CUTOFF, max_swaps=0)
    for gb, (_, _, g) in zip(sel["grade_before"], got["records"]):
        assert abs(gb - g) <= 1e-9 * max(1.0, g)


@pytest.mark.gpu
def test_a_batch_split_into_passes_has_the_run_of_the_whole_batch():
    """tests/_passes.py on the run of the host-driven-loop test with every=20 (beyond the run): whether the moving cells make a
    pass rebuild is the pass's own affair.  Slot translation costs bits: the bounds are those of the host-driven-loop test."""
    import _passes
    fname, species = POTS[0]
    batch = _batch.mixed_batch(species)

    def run(a, b, cap):
        return _npt(fname, False, species, 300.0, 1e-3, 10, lo=a, hi=b, every=20, max_atoms_per_pass=cap, trace=True)

    def same_final(f, w, config):
        assert sorted(f) == sorted(w) and f["x"].shape == w["x"].shape == config[0].shape
        assert _sample.wrapped_diff(f["x"], w["x"], w["cell"]) < X_TOL and _cell_rel(f["cell"], w["cell"]) < 1e-10
        assert np.abs(f["v"] - w["v"]).max(initial=0.0) < V_TOL and abs(f["energy"] - w["energy"]) < E_TOL
        assert abs(f["temperature"] - w["temperature"]) <= 1e-9 * max(1.0, w["temperature"]) and f["status"] == w["status"]
        assert np.abs(f["virial"] - w["virial"]).max() < E_TOL and abs(f["volume"] - w["volume"]) < 1e-8
        assert abs(f["pressure"] - w["pressure"]) < V_TOL and f["capped"] == w["capped"] and f["step"] == w["step"]

    whole, split = _passes.assert_split_runs_are_the_whole_run(run, batch, LIST_CUTOFF, same_final,
                                                               dict(energy=E_TOL, kinetic=E_TOL, volume=E_TOL, pressure=V_TOL), X_TOL)
    assert whole["steps_done"] == 10 and whole["records"] == []
