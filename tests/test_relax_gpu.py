"""Batched FIRE relaxation on the device (md.relax_cells; mtp_relax_step): the kernel alone against the numpy twin of
tests/_relax.py on anisotropic harmonic wells (forces made by the test between launches), its failed state, batch
independence to the bit, many workgroups and the argument errors; then the whole loop against the host-driven loop (forces,
energies and grades from md.evaluate_cells), convergence end to end and capture under relaxation.  Every comparison asserts
the twin's two tie margins first: rounding is 1e-12, so with margins of 1e-6 no decision can flip.  Trajectory bounds are those
of tests/test_sample_gpu.py: the same force path over the same number of steps."""
import functools

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

import _batch
import _cells
import _relax
import _sample
from _cells import LIST_CUTOFF
from test_sample_gpu import BIG, E_TOL, MASSES, V_TOL, X_TOL, _ctx, _midpoint_threshold

WELL_FROZEN = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.int32)      # the 64-atom configuration is frozen from the start
WELL_PARAMS = dict(dt_max=2e-2)
KEEP = (2, 10, 29, 100, 199)
SENTINEL = -77.0


# ---- the kernel alone ----------------------------------------------------------------------------------------------------

def _device_wells(cf, types, x_eq, x0, kk, steps, frozen, nan_at=None, keep=(), dt=1e-3, **params):
    """mtp_relax_step on the wells for steps 0 .. steps - 1, forces by torch between the launches (elementwise: the bits of
    numpy's).  One row more than the batch holds is allocated and filled with a sentinel.  Returns the arrays after the last
    step and copies of them after the steps of `keep`."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ncfg, n = len(cf) - 1, int(cf[-1])
    pad = lambda a: np.concatenate([a, np.full((1,) + a.shape[1:], SENTINEL, dtype=a.dtype)])
    p = dict(_relax.DEFAULTS, **params)
    par = capi.RelaxParams(p["ftol"], p["dt_max"], p["dmax"], p["f_inc"], p["f_dec"], p["alpha_start"], p["f_alpha"], p["n_min"])
    cf_t, ty_t, inv_t = to(cf), to(pad(types)), to(1.0 / _relax.WELL_MASSES)
    x, v, xeq_t, kk_t = to(pad(x0)), to(pad(np.zeros_like(x0))), to(pad(x_eq)), to(pad(kk))
    dt_t = torch.full((ncfg,), dt, dtype=torch.float64, device=dev)
    alpha_t = torch.full((ncfg,), p["alpha_start"], dtype=torch.float64, device=dev)
    npos_t = torch.zeros(ncfg, dtype=torch.int32, device=dev)
    frozen_t = to(np.asarray(frozen, dtype=np.int32))
    done_t = torch.full((ncfg,), -1, dtype=torch.int32, device=dev)
    fmax_t = torch.zeros(ncfg, dtype=torch.float64, device=dev)
    counts_t = torch.zeros(3, dtype=torch.int32, device=dev)

    def state(f, s):
        torch.cuda.synchronize()
        return dict(f=f.cpu().numpy(), step=s, x=x.cpu().numpy(), v=v.cpu().numpy(), dt=dt_t.cpu().numpy(), alpha=alpha_t.cpu().numpy(), npos=npos_t.cpu().numpy(),
                    frozen=frozen_t.cpu().numpy(), done_step=done_t.cpu().numpy(), fmax=fmax_t.cpu().numpy(),
                    counts=counts_t.cpu().numpy())

    kept, f, s = {}, torch.zeros_like(x), -1
    for s in range(steps):
        f = -(kk_t * (x - xeq_t))
        if nan_at is not None and nan_at[0] == s:
            f[nan_at[1], nan_at[2]] = float("nan")
        capi.relax_step(cf_t, par, s, x, v, f, ty_t, inv_t, dt_t, alpha_t, npos_t, frozen_t, done_t, fmax_t, counts_t, stream=st)
        if s in keep:
            kept[s] = state(f, s)
    out = state(f, s)
    assert (out["x"][n:] == SENTINEL).all() and (out["v"][n:] == SENTINEL).all()            # nothing behind the last row
    return out, kept


@functools.lru_cache(maxsize=None)
def _batch_run():
    """the batch of the kernel tests on the device, 200 steps, with its state after the steps of KEEP: made once, never written to"""
    cf, types, x_eq, x0, kk = _relax.wells()
    return _device_wells(cf, types, x_eq, x0, kk, 200, WELL_FROZEN, keep=KEEP, **WELL_PARAMS)


def _rel(got, want):
    scale = float(np.abs(want).max()) if np.size(want) else 0.0
    return (float(np.abs(got - want).max()) / scale if scale > 0.0 else float(np.abs(got - want).max())) if np.size(want) else 0.0


def _assert_own_fmax(got, cf, frozen0, what):
    """fmax of every configuration the launch of got["step"] looked at, against sqrt(max |f_i|^2) of the very forces that
    launch was given (the device's, copied back): 1e-12 relative, entry by entry -- a square root and three products apart"""
    worst = 0.0
    for k in range(len(cf) - 1):
        a, b = int(cf[k]), int(cf[k + 1])
        if b > a and not frozen0[k] and (got["frozen"][k] == 0 or got["done_step"][k] == got["step"]):
            want = float(np.sqrt(np.fmax.reduce((got["f"][a:b] ** 2).sum(1))))
            worst = max(worst, abs(got["fmax"][k] - want) / want)
    print(what, "fmax against the launch's own forces: %.3e relative" % worst)
    assert worst <= 1e-12


def _assert_follows(got, twin, x, v, fmax, n, fscale, what, converged=False):
    """the bounds of the kernel tests: x, v, dt, alpha, fmax within 1e-12 relative (of the largest entry), the integers exactly.
    converged=True (the state after the wells have converged): fmax within 1e-12 of `fscale`, the largest |k x_eq| of the
    batch, instead: the test's own f = -k (x - x_eq) subtracts numbers of
    that size, so positions that agree to 1e-12 relative -- the bound above -- give forces, and an fmax, that agree to 1e-12 of
    it and no better.  Near convergence fmax is 1e-3 while k |x| is 1e2 to 1e3, so half an ulp of x (which only bit-equal
    arithmetic could avoid) already shows as 1e-12 of fmax: measured 1.8e-12 of the largest entry after step 199, with x at
    2.8e-16.  What the kernel itself adds to fmax is bounded to 1e-12 relative by _assert_own_fmax."""
    errs = dict(x=_rel(got["x"][:n], x), v=_rel(got["v"][:n], v), dt=_rel(got["dt"], twin.dt), alpha=_rel(got["alpha"], twin.alpha))
    dfmax = float(np.abs(got["fmax"] - fmax).max())
    print(what, " ".join("%s %.3e" % kv for kv in errs.items()), "fmax %.3e absolute, %.3e of the largest entry, %.3e of k |x_eq|"
          % (dfmax, _rel(got["fmax"], fmax), dfmax / fscale))
    assert all(e <= 1e-12 for e in errs.values()), errs
    assert dfmax <= 1e-12 * (fscale if converged else np.abs(fmax).max())
    assert np.array_equal(got["npos"], twin.npos) and np.array_equal(got["frozen"], twin.frozen)
    assert np.array_equal(got["done_step"], twin.done_step) and list(got["counts"]) == [0, 0, twin.count]


@pytest.mark.gpu
def test_kernel_alone_follows_the_twin_on_harmonic_wells_for_200_steps():
    """configurations of 0, 1, 63, 64, 65, 256 and 257 atoms: the lane and wavefront widths and both sides of the switch from a
    wavefront to the workgroup; two masses; the 64-atom one frozen from the start.  Only fused multiply-add rounding separates
    device and twin: 200 steps x a few ulp, a factor ten on top -> 1e-12 relative, as for the sampling kernels (fmax: see
    _assert_follows)."""
    cf, types, x_eq, x0, kk = _relax.wells()
    n = int(cf[-1])
    twin, x, v, kept = _relax.run_wells(cf, types, x_eq, x0, kk, 200, frozen=WELL_FROZEN, keep=(100,), **WELL_PARAMS)
    twin.assert_margins()
    print("twin: done_step", twin.done_step, "uphill", twin.uphill, "capped", twin.capped, "margins %.3e %.3e" % (twin.margin_p, twin.margin_tol))
    assert twin.uphill >= 1 and twin.capped >= 1
    live = (np.diff(cf) > 0) & (WELL_FROZEN == 0)
    assert (twin.frozen[live] == _relax.CONVERGED).all()
    got, dev_kept = _batch_run()
    fscale = float(np.abs(kk * x_eq).max())
    _assert_follows(got, twin, x, v, twin.fmax, n, fscale, "after step 199:", converged=True)
    # mid-run, while everything still moves (the velocities at the end are zeros: converged)
    xm, vm, dtm, alm, fmm, frm = kept[100]
    mid = dev_kept[100]
    errs = [_rel(mid["x"][:n], xm), _rel(mid["v"][:n], vm), _rel(mid["dt"], dtm), _rel(mid["alpha"], alm)]
    dfm = float(np.abs(mid["fmax"] - fmm).max())
    print("after step 100: x %.3e v %.3e dt %.3e alpha %.3e; fmax %.3e absolute, %.3e of the largest entry" % (*errs, dfm, _rel(mid["fmax"], fmm)))
    assert max(errs) <= 1e-12 and dfm <= 1e-12 * np.abs(fmm).max() and np.abs(vm).max() > 0.0 and np.array_equal(mid["frozen"], frm)
    for s in KEEP:
        _assert_own_fmax(dev_kept[s], cf, WELL_FROZEN, "after step %d:" % s)
    # the frozen and the empty configuration: bitwise untouched
    a, b = int(cf[3]), int(cf[4])
    assert np.array_equal(got["x"][a:b], x0[a:b]) and not got["v"][a:b].any()
    for k in (0, 3):
        assert got["dt"][k] == 1e-3 and got["alpha"][k] == 0.1 and got["npos"][k] == 0 and got["done_step"][k] == -1
        assert got["fmax"][k] == 0.0 and got["frozen"][k] == WELL_FROZEN[k]


@pytest.mark.gpu
def test_a_non_finite_force_fails_its_configuration_and_no_other():
    cf, types, x_eq, x0, kk = _relax.wells()
    a, b = int(cf[4]), int(cf[5])                                                    # the 65-atom configuration
    got, kept = _device_wells(cf, types, x_eq, x0, kk, 11, WELL_FROZEN, nan_at=(3, a + 17, 1), keep=(2,), **WELL_PARAMS)
    clean = _batch_run()[1]
    assert got["frozen"][4] == _relax.FAILED and got["done_step"][4] == 3
    before = kept[2]
    assert np.array_equal(got["x"][a:b], before["x"][a:b]) and np.array_equal(got["v"][a:b], before["v"][a:b])
    assert got["dt"][4] == before["dt"][4] and got["alpha"][4] == before["alpha"][4] and got["npos"][4] == before["npos"][4]
    assert np.array_equal(before["x"][a:b], clean[2]["x"][a:b]) and before["v"][a:b].any()
    others = np.ones(len(x0) + 1, dtype=bool)
    others[a:b] = False
    ok = np.arange(7) != 4
    for key in ("x", "v"):
        assert np.array_equal(got[key][others], clean[10][key][others]), key
    for key in ("dt", "alpha", "npos", "frozen", "done_step", "fmax"):
        assert np.array_equal(got[key][ok], clean[10][key][ok]), key
    assert list(got["counts"]) == [0, 0, 1] and list(clean[10]["counts"]) == [0, 0, 0]


@pytest.mark.gpu
def test_a_configuration_alone_has_the_bits_it_has_in_the_batch():
    cf, types, x_eq, x0, kk = _relax.wells()
    batch = _batch_run()[1][29]
    for k in range(7):
        a, b = int(cf[k]), int(cf[k + 1])
        one, _ = _device_wells(np.array([0, b - a], dtype=np.int32), types[a:b], x_eq[a:b], x0[a:b], kk[a:b], 30, WELL_FROZEN[k: k + 1],
                               **WELL_PARAMS)
        assert np.array_equal(one["x"][: b - a], batch["x"][a:b]) and np.array_equal(one["v"][: b - a], batch["v"][a:b]), k
        for key in ("dt", "alpha", "fmax", "npos", "frozen", "done_step"):
            assert one[key][0] == batch[key][k], (k, key)
    assert batch["v"].any()


@pytest.mark.gpu
def test_1001_configurations_over_many_workgroups_follow_the_twin():
    sizes = np.arange(1001) % 6
    k_cfg = np.array([2.0, 5.0, 9.0])[np.arange(1001) % 3]
    cf, types, x_eq, x0, kk = _relax.wells(sizes, k_cfg, seed=9)
    n = int(cf[-1])
    frozen = np.zeros(1001, dtype=np.int32)
    twin, x, v, _ = _relax.run_wells(cf, types, x_eq, x0, kk, 20, **WELL_PARAMS)
    twin.assert_margins()
    got, _ = _device_wells(cf, types, x_eq, x0, kk, 20, frozen, **WELL_PARAMS)
    _assert_follows(got, twin, x, v, twin.fmax, n, float(np.abs(kk * x_eq).max()), "1001 configurations, 20 steps:")
    _assert_own_fmax(got, cf, frozen, "1001 configurations, after step 19:")
    assert np.abs(v).max() > 0.0 and not np.array_equal(x, x0)
    empty = sizes == 0
    assert (got["fmax"][empty] == 0.0).all() and (got["frozen"][empty] == 0).all() and (got["dt"][empty] == 1e-3).all()


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cf, types, x_eq, x0, kk = _relax.wells([3, 70], (2.0, 5.0))
    n = int(cf[-1])
    rng = np.random.default_rng(0)
    arrays = dict(x=to(x0), v=to(rng.normal(size=(n, 3))), f=to(rng.normal(size=(n, 3))), dt=to(np.full(2, 1e-3)), alpha=to(np.full(2, 0.1)),
                  npos=to(np.zeros(2, dtype=np.int32)), frozen=to(np.zeros(2, dtype=np.int32)), done=to(np.full(2, -1, dtype=np.int32)),
                  fmax=to(np.zeros(2)), counts=to(np.zeros(3, dtype=np.int32)))
    before = {k: t.clone() for k, t in arrays.items()}
    cf_t, ty_t, inv_t = to(cf), to(types), to(1.0 / _relax.WELL_MASSES)

    def call(stream=st, step=0, **kw):
        p = dict(_relax.DEFAULTS, **kw)
        par = capi.RelaxParams(p["ftol"], p["dt_max"], p["dmax"], p["f_inc"], p["f_dec"], p["alpha_start"], p["f_alpha"], p["n_min"])
        A = arrays
        capi.relax_step(cf_t, par, step, A["x"], A["v"], A["f"], ty_t, inv_t, A["dt"], A["alpha"], A["npos"], A["frozen"], A["done"],
                        A["fmax"], A["counts"], stream=stream)

    nan, inf = float("nan"), float("inf")
    bad = [dict(stream=None), dict(step=-1), dict(ftol=-1e-3), dict(ftol=nan), dict(dt_max=0.0), dict(dt_max=inf), dict(dmax=0.0),
           dict(dmax=nan), dict(f_inc=0.99), dict(f_inc=inf), dict(f_dec=0.0), dict(f_dec=1.0), dict(f_dec=nan), dict(alpha_start=-0.1),
           dict(alpha_start=1.1), dict(f_alpha=0.0), dict(f_alpha=1.01), dict(n_min=-1)]
    for kw in bad:
        with pytest.raises(capi.MtpError) as ei:
            call(**kw)
        assert ei.value.code == -20, kw
    keep = arrays["x"]
    arrays["x"] = None                                                               # a missing array
    with pytest.raises(capi.MtpError) as ei:
        call()
    assert ei.value.code == -20
    arrays["x"] = keep
    torch.cuda.synchronize()
    for k, t in arrays.items():
        assert torch.equal(t, before[k]), k
    call(ftol=0.0, f_inc=1.0, alpha_start=0.0, f_alpha=1.0, n_min=0)                 # the ends of the ranges are inside
    torch.cuda.synchronize()
    assert not torch.equal(arrays["v"], before["v"])


# ---- the whole loop ------------------------------------------------------------------------------------------------------

POTS = [("W_L8.mtp", 1), ("WRe_L20.mtp", 2)]
GRADED = [("W_L16_nbh.almtp", 1), ("WRe_L10_cfg.almtp", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_relax_cells_follows_the_host_driven_loop(fname, species):
    """the batch of the sampling tests, 12 steps with dmax = 0.02 A: no atom travels further than 12 x 0.02 x sqrt(3) < 0.42 A
    while the closest pair is 2.4 A apart, so nothing reaches the short distances where the generated potentials have holes.
    every=3: the slot-coordinate rebuild runs."""
    from lammps_mtp_kokkos_amd.md import relax_cells
    batch = _batch.mixed_batch(species)
    ctx = _ctx(fname)
    ref = _relax.reference_loop(ctx, batch, 12, masses=MASSES[species], list_cutoff=LIST_CUTOFF, dmax=0.02)
    ref["twin"].assert_margins()
    got = relax_cells(ctx, batch, 12, masses=MASSES[species], dmax=0.02, every=3, list_cutoff=LIST_CUTOFF, trace=True)
    assert got["steps_done"] == ref["steps_done"] == 12 and got["records"] == [] and got["candidates"] == [] and got["dropped"] == 0
    assert got["builds"] >= 4
    worst = [0.0, 0.0, 0.0]
    for k, (pos, cell, _) in enumerate(batch):
        dx = _sample.wrapped_diff(got["final"][k]["x"], ref["final_x"][k], cell)
        de = float(np.abs(got["trace"]["energy"][:, k] - ref["energy"][:, k]).max())
        df = float(np.abs(got["trace"]["fmax"][:, k] - ref["fmax"][:, k]).max())
        print("%s, configuration %d (%d atoms): dx %.3e dE %.3e dfmax %.3e, %s at %d" %
              (fname, k, len(pos), dx, de, df, got["final"][k]["status"], got["final"][k]["step"]))
        worst = [max(a, b) for a, b in zip(worst, (dx, de, df))]
        f = got["final"][k]
        assert f["x"].shape == (len(pos), 3)
        assert f["status"] == capi.RELAX_STATUS[ref["status"][k]] and f["step"] == ref["done_step"][k]
        assert abs(f["dt"] - ref["dt"][k]) <= 1e-12 * ref["dt"][k] and abs(f["fmax"] - ref["fmax"][-1, k]) < V_TOL
        assert abs(f["energy"] - ref["energy"][-1, k]) < E_TOL
    assert worst[0] < X_TOL and worst[1] < E_TOL and worst[2] < V_TOL, worst
    assert got["final"][0]["status"] == "converged" and got["final"][0]["step"] == 0      # one atom: no force on it
    assert got["final"][3]["status"] == "running" and got["final"][3]["x"].shape == (0, 3) and got["final"][3]["energy"] == 0.0
    moved = max(np.abs(ref["final_x"][k] - batch[k][0]).max() for k in (1, 2, 4, 5))
    assert moved > 1e-3                                                              # (the minimiser did move the atoms)
    assert (ref["energy"][-1, [1, 2, 4, 5]] < ref["energy"][0, [1, 2, 4, 5]]).all()
    with pytest.raises(capi.MtpError) as ei:                                         # no selection state
        relax_cells(ctx, batch, 1, threshold_break=5.0)
    assert ei.value.code == -23


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_relaxation_converges_and_ends_early(fname, species):
    """one atom, the noisy 2-atom cubic cell and an empty configuration, 120 steps at the defaults.  The host-driven loop on the
    CPU oracle converged the 2-atom cell at step 47 (W_L8.mtp) and 51 (WRe_L20.mtp) with a closest approach of 2.56 A.
    The difference of the final positions to the host-driven loop is printed, not asserted."""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, relax_cells
    batch = [_cells.primitive_cell(), _cells.cubic2_cell(), _batch.empty_cell()]
    ctx = _ctx(fname)
    ref = _relax.reference_loop(ctx, batch, 120, masses=MASSES[species], list_cutoff=LIST_CUTOFF)
    ref["twin"].assert_margins()
    assert list(ref["status"]) == [_relax.CONVERGED, _relax.CONVERGED, 0] and 0 < ref["done_step"][1] < 120
    got = relax_cells(ctx, batch, 120, masses=MASSES[species], list_cutoff=LIST_CUTOFF, trace=True)
    done = int(ref["done_step"][1])
    print("%s: converged at step %d, steps_done %d, builds %d" % (fname, done, got["steps_done"], got["builds"]))
    assert [f["status"] for f in got["final"]] == ["converged", "converged", "running"]
    assert [f["step"] for f in got["final"]] == [0, done, -1]
    assert done <= got["steps_done"] <= done + 4 < 120                               # seen at the next read (check_every = 4)
    again = evaluate_cells(ctx, [(got["final"][k]["x"], batch[k][1], batch[k][2]) for k in range(3)], list_cutoff=LIST_CUTOFF, vflag=0)
    fmax = float(np.sqrt((again[1]["f"] ** 2).sum(1)).max())
    e0, e1 = float(got["trace"]["energy"][0, 1]), got["final"][1]["energy"]
    dx = _sample.wrapped_diff(got["final"][1]["x"], ref["final_x"][1], batch[1][1])
    print("fmax at the returned positions %.6e (reported %.6e); E %.9f -> %.9f; final positions differ by %.3e from the host-driven loop"
          % (fmax, got["final"][1]["fmax"], e0, e1, dx))
    assert fmax <= 1e-3 + 1e-9 and got["final"][1]["fmax"] <= 1e-3
    assert e1 < e0 and abs(e1 - ref["energy"][-1, 1]) < E_TOL and abs(again[1]["energy"] - e1) < E_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", GRADED)
def test_capture_under_relaxation_follows_the_twin_and_feeds_select_cells(fname, species):
    """grade steps 0, 4, 8, 12; the two thresholds are the midpoint of the widest gap of the table of grades and that of the
    widest gap of its central half, the lower one as threshold_select (in both tables the widest gap lies ABOVE the central
    one, and threshold_select above threshold_break is refused).  The capture precedes the minimiser: a configuration it freezes keeps the positions it was graded at.
    The lists are not rebuilt in between (every beyond the run; 0.42 A of travel is below half the skin), so that those
    positions can be compared to the bit: a rebuild wraps and translates every row again."""
    from lammps_mtp_kokkos_amd.md import relax_cells, select_cells
    batch = _batch.mixed_batch(species)
    natoms = [len(c[0]) for c in batch]
    ctx = _ctx(fname, True)
    kw = dict(masses=MASSES[species], list_cutoff=LIST_CUTOFF, dmax=0.02, grade_every=4)
    table = _relax.reference_loop(ctx, batch, 12, select=BIG, brk=BIG, **kw)["grades"]
    assert sorted(table) == [0, 4, 8, 12]
    select, brk = sorted([_midpoint_threshold(table, natoms), _midpoint_threshold(table, natoms, central=True)])
    for s in sorted(table):
        print("step %2d grades" % s, table[s])
    print("threshold_select %.9g threshold_break %.9g" % (select, brk))
    ref = _relax.reference_loop(ctx, batch, 12, select=select, brk=brk, **kw)
    ref["twin"].assert_margins()
    want = ref["capture"].records
    print("records", want, "status", ref["status"])
    assert len(want) > 0 and (ref["status"] == _relax.CAPTURED).any(), "the test's inputs are wrong: nothing is captured and frozen"
    got = relax_cells(ctx, batch, 12, threshold_select=select, threshold_break=brk, every=20, trace=True, **kw)
    assert got["builds"] == 1 and got["dropped"] == 0
    assert [(k, s) for k, s, _ in got["records"]] == [(k, s) for k, s, _ in want]
    assert [f["status"] for f in got["final"]] == [capi.RELAX_STATUS[q] for q in ref["status"]]
    snap = {}
    for (k, s, g), (_, _, gw), (pos, cell, types), xs in zip(got["records"], want, got["candidates"], ref["snapshots"]):
        assert abs(g - gw) <= 1e-9 * max(1.0, abs(gw)), (k, s, g, gw)
        assert _sample.wrapped_diff(pos, xs, batch[k][1]) < 1e-9 and np.array_equal(cell, batch[k][1]) and np.array_equal(types, batch[k][2])
        snap[k] = (s, pos)
    for k, (pos, cell, _) in enumerate(batch):
        f = got["final"][k]
        if f["status"] == "captured-frozen":
            s, at = snap[k]
            assert np.array_equal(f["x"], at), k                                      # bitwise: never written after the capture
            assert _sample.wrapped_diff(f["x"], ref["x"][s][k], cell) < 1e-9
        elif len(pos):
            assert _sample.wrapped_diff(f["x"], ref["final_x"][k], cell) < X_TOL
    sel = select_cells(ctx, got["candidates"], threshold=1.1, list_cutoff=LIST_CUTOFF, max_swaps=0)
    for gb, (_, _, g) in zip(sel["grade_before"], got["records"]):
        assert abs(gb - g) <= 1e-9 * max(1.0, g)


@pytest.mark.gpu
@pytest.mark.parametrize("graded", [False, True], ids=["plain", "graded"])
def test_a_batch_split_into_passes_has_the_run_of_the_whole_batch(graded):
    """tests/_passes.py.  plain: the run of test_relax_cells_follows_the_host_driven_loop; graded: potential and thresholds of
    the capture test, max_candidates at its default (nothing is dropped).  every=20 is beyond the run and 0.42 A of travel is
    below half the skin, so every pass with an atom in it builds its lists once.  The one-atom configuration converges at
    step 0: alone in its pass, it ends that pass there.  Slot translation costs bits: the bounds are the trajectory bounds."""
    import _passes
    from lammps_mtp_kokkos_amd.md import relax_cells
    fname, species = GRADED[0] if graded else POTS[0]
    batch = _batch.mixed_batch(species)
    ctx = _ctx(fname, graded)
    kw = dict(masses=MASSES[species], list_cutoff=LIST_CUTOFF, dmax=0.02)
    if graded:
        kw["grade_every"] = 4
        natoms = [len(c[0]) for c in batch]
        table = _relax.reference_loop(ctx, batch, 12, select=BIG, brk=BIG, **kw)["grades"]
        select, brk = sorted([_midpoint_threshold(table, natoms), _midpoint_threshold(table, natoms, central=True)])
        kw.update(threshold_select=select, threshold_break=brk)

    def run(a, b, cap):
        return relax_cells(ctx, batch[a:b], 12, every=20, max_atoms_per_pass=cap, trace=True, **kw)

    def same_final(f, w, config):
        assert sorted(f) == sorted(w) and f["x"].shape == w["x"].shape == config[0].shape
        assert _sample.wrapped_diff(f["x"], w["x"], config[1]) < X_TOL and abs(f["energy"] - w["energy"]) < E_TOL
        assert abs(f["fmax"] - w["fmax"]) < V_TOL and abs(f["dt"] - w["dt"]) <= 1e-12 * w["dt"]
        assert f["status"] == w["status"] and f["step"] == w["step"]

    whole, split = _passes.assert_split_runs_are_the_whole_run(run, batch, LIST_CUTOFF, same_final, dict(energy=E_TOL, fmax=V_TOL), X_TOL)
    assert whole["steps_done"] == 12 and whole["builds"] == 1 and split[1]["builds"] == 5 and split[8]["builds"] == 3
    assert graded == (len(whole["records"]) > 0)
    assert not graded or "captured-frozen" in [f["status"] for f in whole["final"]]
