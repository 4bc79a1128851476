"""Batched Langevin sampling on the device (md.sample_cells; mtp_sample_*): the kernels alone against the numpy twin, NVE
mode against DeviceNVE, the whole loop against the host-driven loop of tests/_sample.py (forces and grades from
md.evaluate_cells), batch independence, capture in both grade modes, capacity, the capture scan beyond one workgroup and the
early end.  Trajectory bounds are those of tests/test_md_gpu.py for ten steps: positions 1e-10 modulo the cell, velocities
1e-9, energies 1e-8; grades to the 1e-9 max(1, g) of tests/test_batch_gpu.py."""
import functools
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen

import _batch
import _cells
import _sample
from _cells import POT, LIST_CUTOFF

MASSES = {1: np.array([183.84]), 2: np.array([183.84, 186.207])}
X_TOL, V_TOL, E_TOL = 1e-10, 1e-9, 1e-8
BIG = 1e300


@functools.lru_cache(maxsize=None)
def _ctx(fname, selection=False):
    return capi.Context(capi.Potential(os.path.join(POT, fname), selection=selection), 0)


def _setup(species, T):
    from lammps_mtp_kokkos_amd.md import maxwell_boltzmann
    batch = _batch.mixed_batch(species)
    keys = [0xabcdef0123456789 + 1000003 * k for k in range(len(batch))]
    temps = np.full(len(batch), float(T))
    vel = maxwell_boltzmann([(p, t) for p, _, t in batch], MASSES[species], temps, 5, keys)
    return batch, keys, temps, vel


@functools.lru_cache(maxsize=None)
def _reference(fname, selection, species, T, dt, steps, grade_every):
    """the host-driven loop without any capture (thresholds out of reach): trajectories, energies and the table of grades.
    Computed once per setting, shared, never written to."""
    batch, keys, temps, vel = _setup(species, T)
    return _sample.reference_loop(_ctx(fname, selection), batch, temps, steps, dt, vel, keys, MASSES[species], t_damp=0.1, seed=5,
                                  grade_every=grade_every, select=BIG, brk=BIG, list_cutoff=LIST_CUTOFF)


def _run(fname, selection, species, T, dt, steps, **kw):
    from lammps_mtp_kokkos_amd.md import sample_cells
    batch, keys, temps, vel = _setup(species, T)
    return sample_cells(_ctx(fname, selection), batch, temps, steps, dt, t_damp=0.1, seed=5, keys=keys, masses=MASSES[species],
                        velocities=vel, list_cutoff=LIST_CUTOFF, every=3, **kw)


def _check_trajectory(got, ref, batch, steps, what):
    worst = [0.0, 0.0, 0.0]
    for k, (pos, cell, _) in enumerate(batch):
        dx = _sample.wrapped_diff(got["final"][k]["x"], ref["x"][steps][k], cell)
        dv = float(np.abs(got["final"][k]["v"] - ref["v"][steps][k]).max()) if len(pos) else 0.0
        de = float(np.abs(got["trace"]["energy"][:, k] + got["trace"]["kinetic"][:, k] - ref["energy"][:, k] - ref["kinetic"][:, k]).max())
        print("%s, configuration %d (%d atoms): dx %.3e dv %.3e dE %.3e" % (what, k, len(pos), dx, dv, de))
        worst = [max(a, b) for a, b in zip(worst, (dx, dv, de))]
        assert got["final"][k]["x"].shape == (len(pos), 3)
    assert worst[0] < X_TOL and worst[1] < V_TOL and worst[2] < E_TOL, worst
    assert abs(got["final"][-1]["energy"] - ref["energy"][steps][-1]) < E_TOL


def _midpoint_threshold(table, natoms, central=False):
    """the midpoint of the widest gap between neighbouring sorted grades of the non-empty configurations (central: the widest
    gap within the central half of the sorted grades, so that the threshold splits the table and not its tail)"""
    g = np.sort(np.unique(np.concatenate([np.asarray(v)[np.asarray(natoms) > 0] for v in table.values()])))
    assert len(g) >= 2, "the table of grades holds one value only"
    lo, hi = (len(g) // 4, 3 * len(g) // 4) if central else (0, len(g) - 1)
    i = lo + int(np.argmax(np.diff(g[lo: hi + 1])))
    assert g[i + 1] - g[i] >= 1e-6 * max(1.0, abs(g[i + 1])), "the test's inputs are wrong: no gap between the grades"
    return 0.5 * (g[i] + g[i + 1])


def _twin_records(table, natoms, select, brk, gap=0, max_candidates=10 ** 9):
    cap = _sample.Capture(natoms, select, brk, gap, max_candidates)
    for step in sorted(table):
        cap.step(step, table[step])
    return cap


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------

def _kernel_batch(dev):
    import torch
    sizes = [0, 1, 63, 64, 65, 257]
    cf = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(cf[-1])
    rng = np.random.default_rng(8)
    types = rng.integers(1, 3, n).astype(np.int32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    row_cfg = torch.empty(n, dtype=torch.int32, device=dev)
    return sizes, cf, n, rng, types, to, row_cfg


@pytest.mark.gpu
def test_kernels_alone_follow_the_twin_for_200_steps_without_forces():
    """f = 0 from the force call, configurations of 0, 1, 63, 64, 65 and 257 atoms (the lane and workgroup widths of the
    per-configuration reduction), two temperatures, two masses, the 64-atom configuration frozen from the start.  Only fused
    multiply-add rounding separates device and twin: 200 steps x a few ulp, a factor ten on top -> 1e-12 relative."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    sizes, cf, n, rng, types, to, row_cfg = _kernel_batch(dev)
    ncfg = len(sizes)
    masses = MASSES[2]
    temps = np.array([300.0, 900.0, 300.0, 900.0, 300.0, 900.0])
    keys = np.array([2 ** 63 + 17, 5, 2 ** 40 + 3, 77, 2 ** 33, 123456789012345], dtype=np.uint64)
    frozen_np = np.array([0, 0, 0, 1, 0, 0], dtype=np.int32)
    x0, v0 = rng.normal(0.0, 3.0, (n, 3)), rng.normal(0.0, 2.0, (n, 3))
    dt, t_damp, seed, steps = 1e-3, 0.1, 0x1234567887654321, 200
    dtf = 0.5 * dt * _sample.FTM2V
    cf_t, ty_t, frozen = to(cf), to(types), to(frozen_np)
    capi.sample_row_map(cf_t, row_cfg, stream=st)
    cfg_row = np.repeat(np.arange(ncfg), sizes)
    assert np.array_equal(row_cfg.cpu().numpy(), cfg_row)
    x, v, f = to(x0), to(v0), torch.zeros((n, 3), dtype=torch.float64, device=dev)
    mass_t, inv_t, T_t, key_t = to(masses), to(1.0 / masses), to(temps), to(keys.view(np.int64))
    capi.sample_final(n, row_cfg, cf_t, frozen, v, f, ty_t, mass_t, inv_t, T_t, key_t, seed, 0, 0.0, dt, t_damp, stream=st)
    for step in range(1, steps + 1):
        capi.sample_initial(n, row_cfg, frozen, x, v, f, ty_t, inv_t, dtf, dt, stream=st)
        f.zero_()
        capi.sample_final(n, row_cfg, cf_t, frozen, v, f, ty_t, mass_t, inv_t, T_t, key_t, seed, step, dtf, dt, t_damp, stream=st)
    counts = to(np.array([3, 1, 1, 0], dtype=np.int32))
    mon = torch.zeros(2 * ncfg + 4, dtype=torch.float64, device=dev)
    capi.sample_monitor(cf_t, frozen, x, to(x0), v, ty_t, mass_t, counts, mon[:ncfg], mon[ncfg: 2 * ncfg], mon[2 * ncfg:], stream=st)
    torch.cuda.synchronize()
    # the twin
    m, inv_m = masses[types - 1], (1.0 / masses)[types - 1]
    index = np.concatenate([np.arange(s) for s in sizes])
    moving = frozen_np[cfg_row] == 0
    xt, vt, ft = x0.copy(), v0.copy(), np.zeros((n, 3))
    _sample.second_half(vt, ft, m, inv_m, temps[cfg_row], t_damp, dt, 0.0, 0, index, keys[cfg_row], seed, moving)
    for step in range(1, steps + 1):
        _sample.first_half(xt, vt, ft, inv_m, dtf, dt, moving)
        ft = np.zeros((n, 3))
        _sample.second_half(vt, ft, m, inv_m, temps[cfg_row], t_damp, dt, dtf, step, index, keys[cfg_row], seed, moving)
    xg, vg, mh = x.cpu().numpy(), v.cpu().numpy(), mon.cpu().numpy()
    dv, dx = np.abs(vg - vt).max(), np.abs(xg - xt).max()
    print("max|dv| %.3e of max|v| %.3e; max|dx| %.3e" % (dv, np.abs(vt).max(), dx))
    assert dv <= 1e-12 * np.abs(vt).max() and dx <= 1e-12 * np.abs(xt).max()
    assert np.array_equal(xg[~moving], x0[~moving]) and np.array_equal(vg[~moving], v0[~moving])      # bitwise
    assert not np.array_equal(vg[moving], v0[moving])
    mv2 = np.array([(m[cfg_row == k, None] * vt[cfg_row == k] ** 2).sum() for k in range(ncfg)])
    print("sum m v^2: rel err", np.abs(mh[:ncfg] - mv2).max() / mv2.max())
    assert (np.abs(mh[:ncfg] - mv2) <= 1e-12 * np.maximum(mv2, 1e-300)).all() and mh[0] == 0.0
    d2 = np.array([((xt - x0)[cfg_row == k] ** 2).sum(1).max() if sizes[k] and not frozen_np[k] else 0.0 for k in range(ncfg)])
    assert (np.abs(mh[ncfg: 2 * ncfg] - d2) <= 1e-11 * d2.max()).all()
    assert abs(mh[2 * ncfg] - d2.max()) <= 1e-11 * d2.max() and list(mh[2 * ncfg + 1:]) == [1.0, 3.0, 1.0]
    # the temperatures the thermostat was given are the temperatures it holds (two groups of ~300 atoms, 100 steps on)
    T_got = _sample.MVV2E * mh[:ncfg] / (3.0 * np.maximum(sizes, 1) * _sample.KB)
    print("kinetic temperatures", T_got)


@pytest.mark.gpu
def test_kernels_with_the_thermostat_off_are_bitwise_the_nve_kernels():
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    sizes, cf, n, rng, types, to, row_cfg = _kernel_batch(dev)
    masses = MASSES[2]
    frozen_np = np.array([0, 0, 0, 1, 0, 0], dtype=np.int32)
    moving = np.repeat(frozen_np, sizes) == 0
    x0, v0 = rng.normal(0.0, 3.0, (n, 3)), rng.normal(0.0, 2.0, (n, 3))
    forces = [to(rng.normal(0.0, 1.5, (n, 3))) for _ in range(6)]
    dt = 1e-3
    dtf = 0.5 * dt * _sample.FTM2V
    cf_t, ty_t, frozen, inv_t = to(cf), to(types), to(frozen_np), to(1.0 / masses)
    capi.sample_row_map(cf_t, row_cfg, stream=st)
    xa, va, xb, vb = to(x0), to(v0), to(x0), to(v0)
    for t_damp in (0.0, -1.0, float("inf")):
        for step in range(1, 6):
            fa = forces[step - 1].clone()
            capi.sample_initial(n, row_cfg, frozen, xa, va, fa, ty_t, inv_t, dtf, dt, stream=st)
            fa = forces[step].clone()
            capi.sample_final(n, row_cfg, cf_t, frozen, va, fa, ty_t, None, inv_t, None, None, 9, step, dtf, dt, t_damp, stream=st)
            assert torch.equal(fa, forces[step])                                             # f is not written
            capi.nve_initial(n, xb, vb, forces[step - 1], ty_t, inv_t, dtf, dt, stream=st)
            capi.nve_final(n, vb, forces[step], ty_t, inv_t, dtf, stream=st)
    torch.cuda.synchronize()
    xa, va, xb, vb = (t.cpu().numpy() for t in (xa, va, xb, vb))
    assert np.array_equal(xa[moving], xb[moving]) and np.array_equal(va[moving], vb[moving])
    assert np.array_equal(xa[~moving], x0[~moving]) and np.array_equal(va[~moving], v0[~moving])
    assert not np.array_equal(xb[~moving], x0[~moving])


# ---- 2. NVE mode against DeviceNVE -------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_nve_mode_follows_device_nve():
    import torch
    from lammps_mtp_kokkos_amd.md import DeviceNVE, sample_cells
    ctx = _ctx("W_L8.mtp")
    pos0, box = mtpgen.bcc_lattice(4, 4, 8)
    rng = np.random.default_rng(300)
    vel0 = rng.normal(size=pos0.shape) * np.sqrt(_sample.KB * 300.0 / (183.84 * _sample.MVV2E))
    vel0 -= vel0.mean(0)
    got = sample_cells(ctx, [(pos0, np.diag(box), None)], 300.0, 10, 1e-3, t_damp=None, velocities=[vel0], masses=183.84,
                       list_cutoff=LIST_CUTOFF, every=3, trace=True)
    assert got["steps_done"] == 10 and got["records"] == [] and got["candidates"] == [] and not got["frozen"].any()
    md = DeviceNVE(ctx, pos0.copy(), box, rc=ctx.pot.info.max_cutoff, mass=183.84, list_cutoff=LIST_CUTOFF, every=3)
    md.v.copy_(torch.from_numpy(vel0))
    e = [md.total_energy()]
    for _ in range(10):
        md.step(1e-3)
        e.append(md.total_energy())
    dx = _sample.wrapped_diff(got["final"][0]["x"], md.x.cpu().numpy(), np.diag(box))
    dv = np.abs(got["final"][0]["v"] - md.v.cpu().numpy()).max()
    de = np.abs(got["trace"]["energy"][:, 0] + got["trace"]["kinetic"][:, 0] - np.array(e)).max()
    print("dx %.3e dv %.3e dE %.3e" % (dx, dv, de))
    assert dx < X_TOL and dv < V_TOL and de < E_TOL
    T = got["final"][0]["temperature"]
    assert abs(T - _sample.MVV2E * 183.84 * (got["final"][0]["v"] ** 2).sum() / (3 * 256 * _sample.KB)) < 1e-9 * T


# ---- 3. Langevin batch against the host-driven loop --------------------------------------------------------------------

LANGEVIN = [("W_L8.mtp", 1, 300.0, 1e-3), ("WRe_L20.mtp", 2, 300.0, 1e-3)]


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species,T,dt", LANGEVIN)
def test_langevin_batch_follows_the_host_driven_loop(fname, species, T, dt):
    """the 1-atom cell, sub-cutoff and tilted cells and the empty configuration; every=3: the slot-coordinate rebuild runs"""
    batch = _batch.mixed_batch(species)
    ref = _reference(fname, False, species, T, dt, 10, 0)
    got = _run(fname, False, species, T, dt, 10, trace=True)
    assert got["steps_done"] == 10 and got["records"] == [] and got["dropped"] == 0
    _check_trajectory(got, ref, batch, 10, fname)
    moved = max(np.abs(ref["x"][10][k] - ref["x"][0][k]).max() for k in (1, 2, 4, 5))
    assert moved > 1e-3                                     # (the thermostat and the forces did move the atoms)
    with pytest.raises(capi.MtpError) as ei:               # no selection state: thresholds cannot be asked for
        _run(fname, False, species, T, dt, 1, threshold_select=2.0)
    assert ei.value.code == -23


# ---- 4. batch independence ---------------------------------------------------------------------------------------------

COLD = dict(T=30.0, dt=2.5e-4, steps=12, grade_every=4)
GRADED = [("W_L16_nbh.almtp", 1), ("WRe_L10_cfg.almtp", 2)]


def _alone(fname, selection, species, T, dt, steps, k, **kw):
    from lammps_mtp_kokkos_amd.md import sample_cells
    batch, keys, temps, vel = _setup(species, T)
    return sample_cells(_ctx(fname, selection), [batch[k]], temps[k], steps, dt, t_damp=0.1, seed=5, keys=[keys[k]],
                        masses=MASSES[species], velocities=[vel[k]], list_cutoff=LIST_CUTOFF, every=3, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("fname,selection,species,T,dt,steps,graded", [("W_L8.mtp", False, 1, 300.0, 1e-3, 10, False),
                                                                       ("W_L16_nbh.almtp", True, 1, 30.0, 2.5e-4, 12, True)])
def test_a_configuration_alone_has_the_trajectory_and_records_it_had_in_the_batch(fname, selection, species, T, dt, steps, graded):
    """same keys entry, same velocities: slot translation costs bits, so the match is to the trajectory bounds, not bitwise"""
    batch = _batch.mixed_batch(species)
    kw = {}
    if graded:
        thr = _midpoint_threshold(_reference(fname, True, species, T, dt, steps, 4)["grades"], [len(c[0]) for c in batch])
        kw = dict(grade_every=4, threshold_select=thr, threshold_break=BIG)
    whole = _run(fname, selection, species, T, dt, steps, trace=True, **kw)
    seen = []
    for k, (pos, cell, _) in enumerate(batch):
        one = _alone(fname, selection, species, T, dt, steps, k, trace=True, **kw)
        dx = _sample.wrapped_diff(one["final"][0]["x"], whole["final"][k]["x"], cell)
        dv = float(np.abs(one["final"][0]["v"] - whole["final"][k]["v"]).max()) if len(pos) else 0.0
        de = float(np.abs(one["trace"]["energy"][:, 0] + one["trace"]["kinetic"][:, 0] - whole["trace"]["energy"][:, k] -
                          whole["trace"]["kinetic"][:, k]).max())
        print("configuration %d alone: dx %.3e dv %.3e dE %.3e" % (k, dx, dv, de))
        assert dx < X_TOL and dv < V_TOL and de < E_TOL
        mine = [(s, g) for c, s, g in whole["records"] if c == k]
        assert [s for _, s, _ in one["records"]] == [s for s, _ in mine]
        for (_, _, g1), (_, g2) in zip(one["records"], mine):
            assert abs(g1 - g2) <= 1e-9 * max(1.0, abs(g2))
        seen += mine
    assert len(seen) == len(whole["records"]) and (not graded or 0 < len(seen))


# ---- 5. / 6. capture in neighbourhood and in configuration mode --------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", GRADED)
def test_capture_follows_the_twin_and_feeds_select_cells(fname, species):
    from lammps_mtp_kokkos_amd.md import select_cells
    T, dt, steps, ge = COLD["T"], COLD["dt"], COLD["steps"], COLD["grade_every"]
    batch = _batch.mixed_batch(species)
    natoms = [len(c[0]) for c in batch]
    ref = _reference(fname, True, species, T, dt, steps, ge)
    assert sorted(ref["grades"]) == [0, 4, 8, 12]
    thr = _midpoint_threshold(ref["grades"], natoms)
    for s in sorted(ref["grades"]):
        print("step %2d grades" % s, ref["grades"][s])
    print("threshold_select", thr)
    twin = _twin_records(ref["grades"], natoms, thr, BIG)
    assert 0 < len(twin.records) < 4 * sum(n > 0 for n in natoms)
    got = _run(fname, True, species, T, dt, steps, grade_every=ge, threshold_select=thr, threshold_break=BIG, trace=True)
    _check_trajectory(got, ref, batch, steps, fname)
    assert [(k, s) for k, s, _ in got["records"]] == [(k, s) for k, s, _ in twin.records]
    assert got["dropped"] == 0 and not got["frozen"].any() and got["steps_done"] == steps
    for (k, s, g), (_, _, want), (pos, cell, types) in zip(got["records"], twin.records, got["candidates"]):
        assert abs(g - want) <= 1e-9 * max(1.0, want), (k, s, g, want)
        assert _sample.wrapped_diff(pos, ref["x"][s][k], batch[k][1]) < 1e-9 and np.array_equal(cell, batch[k][1])
        assert np.array_equal(types, batch[k][2])
    sel = select_cells(_ctx(fname, True), got["candidates"], threshold=1.1, list_cutoff=LIST_CUTOFF, max_swaps=0)
    for gb, (_, _, g) in zip(sel["grade_before"], got["records"]):
        assert abs(gb - g) <= 1e-9 * max(1.0, g)
    # the same threshold as threshold_break: a captured configuration is frozen from its capture step on
    twin2 = _twin_records(ref["grades"], natoms, thr, thr)
    run2 = _run(fname, True, species, T, dt, steps, grade_every=ge, threshold_select=thr, threshold_break=thr, trace=True)
    assert [(k, s) for k, s, _ in run2["records"]] == [(k, s) for k, s, _ in twin2.records]
    assert list(run2["frozen"]) == list(twin2.frozen) and run2["frozen"].any() and not run2["frozen"].all()
    snap = {k: pos for (k, _, _), (pos, _, _) in zip(run2["records"], run2["candidates"])}
    for k, (pos, cell, _) in enumerate(batch):
        if run2["frozen"][k]:
            s = [r[1] for r in run2["records"] if r[0] == k][0]
            assert _sample.wrapped_diff(run2["final"][k]["x"], snap[k], cell) < X_TOL
            assert _sample.wrapped_diff(run2["final"][k]["x"], ref["x"][s][k], cell) < 1e-9
            assert np.abs(run2["final"][k]["v"] - ref["v"][s][k]).max() < V_TOL
        else:
            assert _sample.wrapped_diff(run2["final"][k]["x"], got["final"][k]["x"], cell) < X_TOL
            assert not len(pos) or np.abs(run2["final"][k]["v"] - got["final"][k]["v"]).max() < V_TOL
            assert np.abs(run2["trace"]["energy"][:, k] - got["trace"]["energy"][:, k]).max() < E_TOL


# ---- 7. capacity -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_full_candidate_buffer_drops_whole_snapshots():
    fname, species = GRADED[0]
    T, dt, ge = COLD["T"], COLD["dt"], COLD["grade_every"]
    batch = _batch.mixed_batch(species)
    natoms = [len(c[0]) for c in batch]
    ref = _reference(fname, True, species, T, dt, COLD["steps"], ge)
    table = {s: ref["grades"][s] for s in (0, 4)}
    twin = _twin_records(table, natoms, 0.0, BIG, max_candidates=2)
    assert [(k, s) for k, s, _ in twin.records] == [(0, 0), (1, 0)] and twin.dropped == 8
    got = _run(fname, True, species, T, dt, 4, grade_every=ge, threshold_select=0.0, threshold_break=BIG, max_candidates=2)
    assert [(k, s) for k, s, _ in got["records"]] == [(0, 0), (1, 0)] and got["dropped"] == 8 and len(got["candidates"]) == 2
    for (pos, _, _), k in zip(got["candidates"], (0, 1)):
        assert _sample.wrapped_diff(pos, ref["x"][0][k], batch[k][1]) < 1e-9
    none = _run(fname, True, species, T, dt, 4, grade_every=ge, threshold_select=0.0, threshold_break=BIG, max_candidates=0)
    assert none["records"] == [] and none["dropped"] == 10 and not none["frozen"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("ncfg,max_candidates", [(6, 2), (300, 40), (1000, 10 ** 6)])
def test_capture_kernel_alone_slots_sentinels_and_counts(ncfg, max_candidates):
    """mtp_sample_capture on made-up grades (NaN among them), three grade steps with a capture gap: records, frozen flags and
    counts against the twin; sentinels behind the candidate buffer, behind the records and in the unused rows of a slot are
    untouched.  1000 configurations: four rounds of the scan's workgroup, the last one partial."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    rng = np.random.default_rng(ncfg)
    natoms = rng.integers(0, 6, ncfg)
    natoms[:2] = (3, 0)
    stride = int(natoms.max())
    cf = np.concatenate([[0], np.cumsum(natoms)]).astype(np.int32)
    n = int(cf[-1])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x_np, org_np = rng.normal(0, 5, (n, 3)), rng.normal(0, 50, (ncfg, 3))
    cf_t, x, org = to(cf), to(x_np), to(org_np)
    row_cfg = torch.empty(n, dtype=torch.int32, device=dev)
    capi.sample_row_map(cf_t, row_cfg, stream=st)
    room = min(max_candidates, 4 * ncfg)
    cand = torch.full((room + 2, stride, 3), -77.0, dtype=torch.float64, device=dev)
    rec = torch.full((room + 2, 2), -7, dtype=torch.int32, device=dev)
    rec_g = torch.full((room + 2,), -77.0, dtype=torch.float64, device=dev)
    frozen = torch.zeros(ncfg, dtype=torch.int32, device=dev)
    last = torch.full((ncfg,), -2 ** 30, dtype=torch.int32, device=dev)
    slot = torch.zeros(ncfg, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    twin = _sample.Capture(natoms, 2.0, 5.0, 6, room)
    want_snap = []
    for step in (0, 4, 8):
        g = rng.uniform(0.0, 7.0, ncfg)
        g[rng.random(ncfg) < 0.05] = np.nan
        x_np = x_np + 0.01
        x.copy_(to(x_np))
        capi.sample_capture(cf_t, n, row_cfg, to(g), step, 2.0, 5.0, 6, x, org, frozen, last, slot, room, stride, cand, rec, rec_g,
                            counts, stream=st)
        taken = twin.step(step, g)
        want_snap += [x_np[cf[k]:cf[k + 1]] - org_np[k] for k in taken]
        torch.cuda.synchronize()
        sl = slot.cpu().numpy()
        assert sorted(np.nonzero(sl >= 0)[0]) == sorted(taken)
    ch, rh, gh, snap = counts.cpu().numpy(), rec.cpu().numpy(), rec_g.cpu().numpy(), cand.cpu().numpy()
    ncap = len(twin.records)
    print("ncfg %d: %d captured, %d dropped, %d frozen" % (ncfg, ncap, twin.dropped, twin.frozen.sum()))
    assert list(ch[:3]) == [ncap, twin.dropped, int(twin.frozen.sum())] and ncap > 0
    assert (max_candidates >= 4 * ncfg) == (twin.dropped == 0)
    assert [tuple(r) for r in rh[:ncap]] == [(k, s) for k, s, _ in twin.records]
    assert np.array_equal(gh[:ncap], np.array([g for _, _, g in twin.records]), equal_nan=True)
    assert np.array_equal(frozen.cpu().numpy() != 0, twin.frozen)
    assert (rh[ncap:] == -7).all() and (gh[ncap:] == -77.0).all() and (snap[ncap:] == -77.0).all()     # the sentinels
    for j, want in enumerate(want_snap):
        assert np.array_equal(snap[j, : len(want)], want) and (snap[j, len(want):] == -77.0).all()


# ---- 8. more configurations than one workgroup of the capture scan ------------------------------------------------------

@pytest.mark.gpu
def test_capture_scan_over_300_configurations():
    from lammps_mtp_kokkos_amd.md import maxwell_boltzmann, sample_cells
    ctx = _ctx("W_L16_nbh.almtp", True)
    ncfg = 300
    batch = [_cells.cubic2_cell() for _ in range(ncfg)]
    temps = np.linspace(50.0, 3000.0, ncfg)
    keys = list(range(1000, 1000 + ncfg))
    vel = maxwell_boltzmann([(p, t) for p, _, t in batch], MASSES[1], temps, 3, keys)
    kw = dict(t_damp=0.1, seed=3, keys=keys, masses=MASSES[1], velocities=vel, list_cutoff=LIST_CUTOFF, grade_every=1)
    dt = 2e-3
    ref = _sample.reference_loop(ctx, batch, temps, 2, dt, vel, keys, MASSES[1], t_damp=0.1, seed=3, grade_every=1, select=BIG,
                                 brk=BIG, list_cutoff=LIST_CUTOFF)
    thr = _midpoint_threshold(ref["grades"], [2] * ncfg, central=True)
    twin = _twin_records(ref["grades"], [2] * ncfg, thr, BIG)
    per_step = [sum(1 for r in twin.records if r[1] == s) for s in (0, 1, 2)]
    print("threshold %.9g: captures per step" % thr, per_step)
    assert 0 < len(twin.records) < 3 * ncfg and any(0 < c < ncfg for c in per_step)
    got = sample_cells(ctx, batch, temps, 2, dt, threshold_select=thr, threshold_break=BIG, **kw)
    assert [(k, s) for k, s, _ in got["records"]] == [(k, s) for k, s, _ in twin.records]       # in order: no duplicates, no holes
    assert len(got["candidates"]) == len(twin.records) and got["dropped"] == 0
    for (k, s, g), (_, _, want), (pos, _, _) in zip(got["records"], twin.records, got["candidates"]):
        assert abs(g - want) <= 1e-9 * max(1.0, want)
        assert _sample.wrapped_diff(pos, ref["x"][s][k], batch[k][1]) < 1e-9


# ---- 9. early end -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_everything_frozen_at_step_0_ends_the_run_there():
    fname, species = GRADED[0]
    batch, keys, temps, vel = _setup(species, COLD["T"])
    got = _run(fname, True, species, COLD["T"], COLD["dt"], 50, grade_every=4, threshold_select=0.0, threshold_break=0.0)
    assert got["steps_done"] == 0
    assert list(got["frozen"]) == [len(c[0]) > 0 for c in batch]
    assert [(k, s) for k, s, _ in got["records"]] == [(k, 0) for k, c in enumerate(batch) if len(c[0])] and got["dropped"] == 0
    for k, (pos, cell, _) in enumerate(batch):
        assert _sample.wrapped_diff(got["final"][k]["x"], pos, cell) < 1e-12                    # nothing moved (beyond the wrap)
        assert np.array_equal(got["final"][k]["v"], vel[k])


@pytest.mark.gpu
@pytest.mark.parametrize("check_every,seen_at", [(2, 4), (4, 5)])
def test_everything_frozen_at_a_later_grade_step_ends_the_run_at_the_next_read(check_every, seen_at):
    """the empty configuration and the 54-atom one, whose grade rises along the cold run: threshold_break between its grades of
    steps 0 and 4 freezes it at step 4.  With lists rebuilt every 3 steps the monitor block is read at step 5 (two steps after
    the rebuild of step 3) with check_every = 2 -- that first half wrote nothing, so four steps were made -- and at the
    rebuild of step 6 with check_every = 4: five steps.  Nothing moves after the capture either way."""
    from lammps_mtp_kokkos_amd.md import sample_cells
    fname, species = GRADED[0]
    T, dt, ge = COLD["T"], COLD["dt"], COLD["grade_every"]
    batch, keys, temps, vel = _setup(species, T)
    ref = _reference(fname, True, species, T, dt, COLD["steps"], ge)
    g0, g4 = ref["grades"][0][5], ref["grades"][4][5]
    assert g4 - g0 >= 1e-6 * g4, "the test's inputs are wrong: the grade of the 54-atom cell does not rise"
    thr = 0.5 * (g0 + g4)
    got = sample_cells(_ctx(fname, True), [batch[3], batch[5]], temps[[3, 5]], 50, dt, t_damp=0.1, seed=5, keys=[keys[3], keys[5]],
                       masses=MASSES[species], velocities=[vel[3], vel[5]], list_cutoff=LIST_CUTOFF, every=3, check_every=check_every,
                       grade_every=ge, threshold_select=thr, threshold_break=thr)
    assert got["steps_done"] == seen_at and got["builds"] == 1 + (seen_at - 1) // 3
    assert [(k, s) for k, s, _ in got["records"]] == [(1, 4)] and list(got["frozen"]) == [False, True] and got["dropped"] == 0
    assert abs(got["records"][0][2] - g4) <= 1e-9 * max(1.0, g4)
    cell = batch[5][1]
    assert _sample.wrapped_diff(got["final"][1]["x"], got["candidates"][0][0], cell) < X_TOL
    assert _sample.wrapped_diff(got["final"][1]["x"], ref["x"][4][5], cell) < 1e-9
    assert np.abs(got["final"][1]["v"] - ref["v"][4][5]).max() < V_TOL


@pytest.mark.gpu
def test_half_skin_displacement_triggers_a_rebuild():
    """one atom in the primitive cell (no force on it: every image moves with it), NVE at 95 A/ps and 1 fs: 0.095 A a step.  With
    the regular rebuild out of reach and the block read every second step, the displacement passes half the skin (1 A) at
    the read of step 12 after each build (0.95 A at step 10, 1.14 A at step 12): builds at steps 12, 24 and 36 of 40.  The atom keeps its straight line."""
    from lammps_mtp_kokkos_amd.md import sample_cells
    ctx = _ctx("W_L8.mtp")
    assert abs(0.5 * (LIST_CUTOFF - ctx.pot.info.max_cutoff) - 1.0) < 1e-12
    pos, cell, types = _cells.primitive_cell()
    v0 = 95.0 * np.array([[0.6, 0.0, 0.8]])
    got = sample_cells(ctx, [(pos, cell, types)], 300.0, 40, 1e-3, t_damp=None, velocities=[v0], masses=183.84,
                       list_cutoff=LIST_CUTOFF, every=1000, check_every=2)
    assert got["steps_done"] == 40 and got["builds"] == 4
    assert np.abs(got["final"][0]["v"] - v0).max() < 1e-9
    assert _sample.wrapped_diff(got["final"][0]["x"], pos + 40 * 1e-3 * v0, cell) < X_TOL
    still = sample_cells(ctx, [(pos, cell, types)], 300.0, 40, 1e-3, t_damp=None, velocities=[v0], masses=183.84,
                         list_cutoff=LIST_CUTOFF, every=1000, check_every=0)
    assert still["builds"] == 1                                # (without the read nothing asks for one)


# ---- 10. more than one pass ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("graded", [False, True], ids=["plain", "graded"])
def test_a_batch_split_into_passes_has_the_run_of_the_whole_batch(graded):
    """tests/_passes.py.  plain: the Langevin run of the host-driven-loop test; graded: the cold run, potential and threshold of
    the capture test, max_candidates at its default (nothing is dropped).  every=20 is beyond both runs and nothing travels
    half the skin (1 A) in them, so every pass with an atom in it builds its lists once.  Slot translation costs bits: the
    bounds are those of test_a_configuration_alone_has_the_trajectory_and_records_it_had_in_the_batch."""
    import _passes
    from lammps_mtp_kokkos_amd.md import sample_cells
    fname, selection, species, T, dt, steps = ("W_L16_nbh.almtp", True, 1, COLD["T"], COLD["dt"], COLD["steps"]) if graded else \
        ("W_L8.mtp", False, 1, 300.0, 1e-3, 10)
    batch, keys, temps, vel = _setup(species, T)
    kw = {}
    if graded:
        thr = _midpoint_threshold(_reference(fname, True, species, T, dt, steps, 4)["grades"], [len(c[0]) for c in batch])
        kw = dict(grade_every=4, threshold_select=thr, threshold_break=BIG)

    def run(a, b, cap):
        return sample_cells(_ctx(fname, selection), batch[a:b], temps[a:b], steps, dt, t_damp=0.1, seed=5, keys=keys[a:b],
                            masses=MASSES[species], velocities=vel[a:b], list_cutoff=LIST_CUTOFF, every=20, max_atoms_per_pass=cap,
                            trace=True, **kw)

    def same_final(f, w, config):
        assert sorted(f) == sorted(w) and f["x"].shape == w["x"].shape == config[0].shape
        assert _sample.wrapped_diff(f["x"], w["x"], config[1]) < X_TOL
        assert np.abs(f["v"] - w["v"]).max(initial=0.0) < V_TOL and abs(f["energy"] - w["energy"]) < E_TOL
        assert abs(f["temperature"] - w["temperature"]) <= 1e-9 * max(1.0, w["temperature"])

    whole, split = _passes.assert_split_runs_are_the_whole_run(run, batch, LIST_CUTOFF, same_final, dict(energy=E_TOL, kinetic=E_TOL),
                                                               X_TOL)
    assert whole["steps_done"] == steps and whole["builds"] == 1 and split[1]["builds"] == 5 and split[8]["builds"] == 3
    assert graded == (len(whole["records"]) > 0)
