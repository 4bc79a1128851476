"""Batched nudged elastic band on the device (md.neb_cells; mtp_neb_step): the kernel alone against the numpy twin of
tests/_neb.py on the analytic double-well surface (forces and per-atom energies made by torch between the launches), the
minimum image, batch independence to the bit over many workgroups, the ways a band stops and the argument errors; then the
whole loop against the host-driven loop (forces, energies and grades from md.evaluate_cells), convergence end to end, capture
under NEB and split passes.  Every comparison asserts the twin's tie margins first: rounding is 1e-12, so with margins of 1e-6
no decision can flip.  Trajectory bounds are those of tests/test_sample_gpu.py: the same force path over the same number of
steps."""
import functools

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

import _batch
import _cells
import _neb
import _sample
from _cells import LIST_CUTOFF
from test_sample_gpu import BIG, E_TOL, MASSES, V_TOL, X_TOL, _ctx, _midpoint_threshold

SHAPES = [(M, n) for M in (3, 4, 9) for n in (1, 63, 64, 65, 257)] + [(4, 64)]       # the last band: frozen from the start
KEEP = (2, 10, 29, 100, 199)
PARAMS = dict(climb_step=20)
SENTINEL = -77.0
STATE_KEYS = ("dt", "alpha", "fmax", "npos", "done_step", "climber", "status")


def _frozen_from_the_start(S):
    frozen = np.zeros(len(S["cfg_first"]) - 1, dtype=np.int32)
    frozen[int(S["band_first"][-2]) + 2] = 1                                         # an interior image of the last band
    return frozen


# ---- the kernel alone ----------------------------------------------------------------------------------------------------

def _device_bands(S, steps, frozen=None, nan_at=None, keep=(), last_at=None, dt=1e-3, nan_energy_at=None, **params):
    """mtp_neb_step on the surface bands `S` for steps 0 .. steps - 1, eatom and forces by torch between the launches (the
    expression of the twin, elementwise).  One row more than the batch holds is allocated and filled with a sentinel.  Returns
    the arrays after the last step and copies of them after the steps of `keep`."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nband, ncfg, n = len(S["band_first"]) - 1, len(S["cfg_first"]) - 1, int(S["cfg_first"][-1])
    pad = lambda a, fill: np.concatenate([a, np.full((1,) + a.shape[1:], fill, dtype=a.dtype)])
    p = dict(_neb.DEFAULTS, **params)
    par = capi.NebParams(capi.RelaxParams(p["ftol"], p["dt_max"], p["dmax"], p["f_inc"], p["f_dec"], p["alpha_start"], p["f_alpha"],
                                          p["n_min"]), p["spring"], p["climb_step"])
    consts = [to(pad(S[k], 0.0)) for k in _neb.SURFACE_KEYS]
    x, v = to(pad(S["x0"], SENTINEL)), to(pad(np.zeros_like(S["x0"]), SENTINEL))
    A = dict(band_first=to(S["band_first"]), cfg_first=to(S["cfg_first"]), x=x, v=v, type=to(pad(S["types"], 1)),
             inv_mass=to(1.0 / _neb.SURFACE_MASSES), origins=to(S["origins"]), cell=to(S["cells"].reshape(nband, 9)),
             cell_inv=to(np.linalg.inv(S["cells"]).reshape(nband, 9)), fneb=to(pad(np.zeros_like(S["x0"]), SENTINEL)),
             energy=torch.zeros(ncfg, dtype=torch.float64, device=dev),
             dt=torch.full((nband,), dt, dtype=torch.float64, device=dev),
             alpha=torch.full((nband,), p["alpha_start"], dtype=torch.float64, device=dev),
             npos=torch.zeros(nband, dtype=torch.int32, device=dev), done_step=torch.full((nband,), -1, dtype=torch.int32, device=dev),
             fmax=torch.zeros(nband, dtype=torch.float64, device=dev), climber=torch.full((nband,), -1, dtype=torch.int32, device=dev),
             band_status=torch.zeros(nband, dtype=torch.int32, device=dev),
             frozen=to(np.zeros(ncfg, dtype=np.int32) if frozen is None else np.asarray(frozen, dtype=np.int32)),
             counts=torch.zeros(3, dtype=torch.int32, device=dev))

    def state(s):
        torch.cuda.synchronize()
        out = {k: t.cpu().numpy() for k, t in A.items() if k not in ("band_first", "cfg_first", "type", "inv_mass", "origins", "cell", "cell_inv")}
        out.update(step=s, status=out.pop("band_status"))
        return out

    kept, s = {}, -1
    for s in range(steps):
        e, f = _neb.surface(torch, x, *consts)
        if nan_at is not None and nan_at[0] == s:
            f[nan_at[1], nan_at[2]] = float("nan")
        if nan_energy_at is not None and nan_energy_at[0] == s:
            e[nan_energy_at[1]] = float("nan")
        A.update(f=f, eatom=e)
        capi.neb_step(S["band_first"], ncfg, par, s, A, last=s == last_at, stream=st)
        if s in keep:
            kept[s] = state(s)
    out = state(s)
    for key in ("x", "v", "fneb"):
        assert (out[key][n:] == SENTINEL).all(), key                                 # nothing behind the last row
    return out, kept


@functools.lru_cache(maxsize=None)
def _surface():
    return _neb.surface_bands(SHAPES, seed=5)


@functools.lru_cache(maxsize=None)
def _batch_run():
    """the batch of the kernel tests on the device, 200 steps, with its state after the steps of KEEP: made once, never written to"""
    S = _surface()
    return _device_bands(S, 200, _frozen_from_the_start(S), keep=KEEP, **PARAMS)


@functools.lru_cache(maxsize=None)
def _twin_run():
    S = _surface()
    return _neb.run_surface(S, 200, frozen=_frozen_from_the_start(S), keep=KEEP, **PARAMS)


def _rel(got, want):
    scale = float(np.abs(want).max()) if np.size(want) else 0.0
    return (float(np.abs(got - want).max()) / scale if scale > 0.0 else float(np.abs(got - want).max())) if np.size(want) else 0.0


def _assert_own_fmax(got, S, what):
    """fmax of every band the launch of got["step"] looked at, against the largest row norm of the very F_neb that launch wrote
    (the device's, copied back): 1e-12 relative -- a square root and three products apart"""
    worst = 0.0
    for b in range(len(S["band_first"]) - 1):
        if got["status"][b] == 0 or (got["done_step"][b] == got["step"] and got["status"][b] != _neb.CAPTURED):
            r0, r1 = int(S["cfg_first"][S["band_first"][b] + 1]), int(S["cfg_first"][S["band_first"][b + 1] - 1])
            want = float(np.sqrt(np.fmax.reduce((got["fneb"][r0:r1] ** 2).sum(1))))
            worst = max(worst, abs(got["fmax"][b] - want) / want)
    print(what, "fmax against the launch's own F_neb: %.3e relative" % worst)
    assert worst <= 1e-12


def _assert_follows(got, want, n, what, forces=True):
    """x, dt, alpha, the image energies and, with `forces`, v, F_neb and fmax within 1e-12 relative (of the largest entry), the
    integers exactly"""
    errs = dict(x=_rel(got["x"][:n], want["x"]), dt=_rel(got["dt"], want["dt"]), alpha=_rel(got["alpha"], want["alpha"]),
                energy=_rel(got["energy"], want["energy"]))
    if forces:
        errs.update(v=_rel(got["v"][:n], want["v"]), fneb=_rel(got["fneb"][:n], want["fneb"]), fmax=_rel(got["fmax"], want["fmax"]))
    print(what, " ".join("%s %.3e" % kv for kv in errs.items()))
    assert all(e <= 1e-12 for e in errs.values()), errs
    for key in ("npos", "frozen", "done_step", "climber", "status"):
        assert np.array_equal(got[key], want[key]), key
    assert list(got["counts"]) == [0, 0, want["count"]]


MOVING = dict(climb_step=20, ftol=0.0, dmax=1e-3)


@pytest.mark.gpu
def test_kernel_alone_follows_the_twin_for_200_steps():
    """bands of 3, 4 and 9 images with 1, 63, 64, 65 and 257 atoms: the lane and wavefront widths and the stride loops, one, two
    and seven interior images (fewer and more than the four wavefronts); a triclinic cell, slot origins that differ from image
    to image, two masses, the climbing image from step 20, and a band with an image frozen from the start.  ftol = 0 and
    dmax = 0.001 A: nothing converges and no coordinate travels further than 0.2 A, so F_neb stays of order 1 eV/A in every
    band for all 200 steps (asserted) and the comparison is well conditioned to the end: x, v, dt, alpha, F_neb, the image
    energies and fmax within 1e-12 relative after steps 2, 10, 29, 100 and 199, the integers exactly -- only fused multiply-add
    rounding separates device and twin: 200 steps x a few ulp, a factor ten on top, the bound of tests/test_relax_gpu.py."""
    S = _surface()
    n = int(S["cfg_first"][-1])
    frozen = _frozen_from_the_start(S)
    twin, x, v, kept = _neb.run_surface(S, 200, frozen=frozen, keep=KEEP, **MOVING)
    twin.assert_margins()
    print("twin: climber", twin.climber, "uphill", twin.uphill, "capped", twin.capped, "margins", twin.margins())
    assert (twin.status[:-1] == 0).all() and twin.status[-1] == _neb.CAPTURED and twin.capped >= 1 and (twin.climber[:-1] > 0).all()
    got, dev_kept = _device_bands(S, 200, frozen, keep=KEEP, **MOVING)
    for s in KEEP:
        assert kept[s]["fmax"][:-1].min() > 0.5 and np.abs(kept[s]["v"]).max() > 1.0
        _assert_follows(dev_kept[s], kept[s], n, "after step %d:" % s)
        _assert_own_fmax(dev_kept[s], S, "after step %d:" % s)
    assert np.array_equal(got["x"], dev_kept[199]["x"]) and np.abs(x - S["x0"]).max() > 0.05


@pytest.mark.gpu
def test_kernel_alone_follows_the_twin_to_convergence():
    """the same bands at the defaults (ftol 1e-3, dmax 0.1 A): steps uphill and steps without the cap, and 14 of the 15 bands
    converge between steps 103 and 178.  While the forces are of order 1 (steps 2, 10, 29) everything is compared as above.
    Later F_neb is a difference of the surface's O(1) terms that has shrunk to 1e-3, and velocities are what its kicks leave:
    agreement of those with the twin is then limited by the test's own force expression, not by the kernel, and is not asserted
    here (the run above holds it for 200 steps).  What is asserted to the end: positions, dt, alpha and image energies within
    1e-12 relative, every integer -- npos, the climber, the status and the step of convergence of every band, frozen of every
    image, the count --, fmax against the launch's own F_neb, and velocities of converged bands that are zero."""
    S = _surface()
    n = int(S["cfg_first"][-1])
    twin, x, v, kept = _twin_run()
    twin.assert_margins()
    print("twin: status", twin.status, "done_step", twin.done_step, "climber", twin.climber, "uphill", twin.uphill, "capped", twin.capped,
          "margins", twin.margins())
    assert twin.uphill >= 1 and twin.capped >= 1
    assert (twin.status[:-1] == _neb.CONVERGED).sum() >= 10 and (twin.status == 0).any() and twin.status[-1] == _neb.CAPTURED
    got, dev_kept = _batch_run()
    for s in KEEP:
        assert np.abs(kept[s]["v"]).max() > 0.0
        _assert_follows(dev_kept[s], kept[s], n, "after step %d:" % s, forces=s <= 29)
        _assert_own_fmax(dev_kept[s], S, "after step %d:" % s)
    assert np.array_equal(got["x"], dev_kept[199]["x"])
    for b in np.nonzero(got["status"] == _neb.CONVERGED)[0]:                         # converged: fmax <= ftol, velocities zeroed
        r0, r1 = int(S["cfg_first"][S["band_first"][b]]), int(S["cfg_first"][S["band_first"][b + 1]])
        assert got["fmax"][b] <= 1e-3 and not got["v"][r0:r1].any()
        assert (got["frozen"][S["band_first"][b]: S["band_first"][b + 1]] == _neb.CONVERGED).all()
    # the two end images of every band: bitwise where they were, never given a velocity, F_neb = 0
    for b in range(len(SHAPES)):
        for k in (int(S["band_first"][b]), int(S["band_first"][b + 1]) - 1):
            r0, r1 = int(S["cfg_first"][k]), int(S["cfg_first"][k + 1])
            assert np.array_equal(got["x"][r0:r1], S["x0"][r0:r1]) and not got["v"][r0:r1].any()
            assert not got["fneb"][r0:r1].any()
    # the band frozen from the start stopped at step 0 by rule 1 and nothing else of it was written
    b = len(SHAPES) - 1
    k0, k1 = int(S["band_first"][b]), int(S["band_first"][b + 1])
    r0, r1 = int(S["cfg_first"][k0]), int(S["cfg_first"][k1])
    assert got["status"][b] == _neb.CAPTURED and got["done_step"][b] == 0 and (got["frozen"][k0:k1] == 1).all()
    assert np.array_equal(got["x"][r0:r1], S["x0"][r0:r1]) and not got["v"][r0:r1].any() and not got["fneb"][r0:r1].any()
    assert not got["energy"][k0:k1].any() and got["dt"][b] == 1e-3 and got["fmax"][b] == 0.0 and got["climber"][b] == -1
    assert dev_kept[2]["counts"][2] == 3                                             # (its three other images were counted)


@pytest.mark.gpu
def test_images_shifted_by_lattice_vectors_give_the_same_band():
    """rule 3's minimum image: what a re-neighbouring does to a band -- every image wrapped on its own"""
    S = _neb.surface_bands([(3, 5), (4, 65), (9, 3)], seed=7)
    T, shift = _neb.shifted_by_lattice_vectors(S)
    n = int(S["cfg_first"][-1])
    assert (np.abs(shift).max(1) > 5.0).sum() > n // 5
    twin, xt, _, _ = _neb.run_surface(S, 30, climb_step=10)
    twin.assert_margins()
    a, _ = _device_bands(S, 30, climb_step=10)
    b, _ = _device_bands(T, 30, climb_step=10)
    moves = _rel(b["x"][:n] - T["x0"], a["x"][:n] - S["x0"])
    print("F_neb %.3e, moves %.3e, v %.3e relative; against the twin x %.3e" % (_rel(b["fneb"][:n], a["fneb"][:n]), moves,
                                                                                 _rel(b["v"][:n], a["v"][:n]), _rel(a["x"][:n], xt)))
    assert _rel(b["fneb"][:n], a["fneb"][:n]) <= 1e-12 and moves <= 1e-12 and _rel(b["v"][:n], a["v"][:n]) <= 1e-12
    assert _rel(b["energy"], a["energy"]) <= 1e-12 and _rel(a["x"][:n], xt) <= 1e-12
    for key in ("npos", "climber", "status", "done_step"):
        assert np.array_equal(a[key], b[key]), key
    assert np.abs(a["x"][:n] - S["x0"]).max() > 0.05


BATCH_SHAPES = [[(3, 1), (4, 5), (5, 66), (3, 2), (6, 7), (4, 64)][i % 6] for i in range(300)]


@pytest.mark.gpu
def test_a_band_alone_has_the_bits_it_has_in_a_batch_of_300_bands():
    """300 workgroups; the batch follows the twin, and bands of every shape in it, run alone, come out bit for bit"""
    S = _neb.surface_bands(BATCH_SHAPES, seed=9)
    n = int(S["cfg_first"][-1])
    twin, x, v, _ = _neb.run_surface(S, 20, climb_step=10)
    twin.assert_margins()
    batch, _ = _device_bands(S, 20, climb_step=10)
    print("300 bands, 20 steps: x %.3e v %.3e F_neb %.3e relative" % (_rel(batch["x"][:n], x), _rel(batch["v"][:n], v),
                                                                      _rel(batch["fneb"][:n], twin.fneb)))
    assert _rel(batch["x"][:n], x) <= 1e-12 and _rel(batch["v"][:n], v) <= 1e-12 and _rel(batch["fneb"][:n], twin.fneb) <= 1e-12
    assert np.array_equal(batch["npos"], twin.npos) and np.array_equal(batch["climber"], twin.climber) and batch["v"].any()
    for b in (0, 1, 2, 3, 4, 5, 296, 299):
        one, _ = _device_bands(_neb.sub_bands(S, [b]), 20, climb_step=10)
        k0, k1 = int(S["band_first"][b]), int(S["band_first"][b + 1])
        r0, r1 = int(S["cfg_first"][k0]), int(S["cfg_first"][k1])
        for key in ("x", "v", "fneb"):
            assert np.array_equal(one[key][: r1 - r0], batch[key][r0:r1]), (b, key)
        assert np.array_equal(one["energy"], batch["energy"][k0:k1]) and np.array_equal(one["frozen"], batch["frozen"][k0:k1])
        for key in STATE_KEYS:
            assert one[key][0] == batch[key][b], (b, key)


@pytest.mark.gpu
def test_a_non_finite_force_fails_its_band_and_no_other():
    S = _surface()
    b = 7                                                                            # 4 images of 64 atoms
    k0, k1 = int(S["band_first"][b]), int(S["band_first"][b + 1])
    r0, r1 = int(S["cfg_first"][k0]), int(S["cfg_first"][k1])
    row = int(S["cfg_first"][k0 + 2]) + 17                                           # an atom of its second interior image
    got, kept = _device_bands(S, 11, _frozen_from_the_start(S), nan_at=(3, row, 1), keep=(2,), **PARAMS)
    clean = _batch_run()[1]
    assert got["status"][b] == _neb.FAILED and got["done_step"][b] == 3 and (got["frozen"][k0:k1] == 3).all()
    before = kept[2]
    assert np.array_equal(got["x"][r0:r1], before["x"][r0:r1]) and np.array_equal(got["v"][r0:r1], before["v"][r0:r1])
    assert got["dt"][b] == before["dt"][b] and got["alpha"][b] == before["alpha"][b] and got["npos"][b] == before["npos"][b]
    assert np.array_equal(before["x"][r0:r1], clean[2]["x"][r0:r1]) and before["v"][r0:r1].any()
    others = np.ones(len(S["x0"]) + 1, dtype=bool)
    others[r0:r1] = False
    ok = np.arange(len(SHAPES)) != b
    cfg_ok = np.ones(len(S["cfg_first"]) - 1, dtype=bool)
    cfg_ok[k0:k1] = False
    for key in ("x", "v", "fneb"):
        assert np.array_equal(got[key][others], clean[10][key][others]), key
    for key in STATE_KEYS:
        assert np.array_equal(got[key][ok], clean[10][key][ok]), key
    assert np.array_equal(got["energy"][cfg_ok], clean[10]["energy"][cfg_ok]) and np.array_equal(got["frozen"][cfg_ok], clean[10]["frozen"][cfg_ok])
    assert list(got["counts"]) == [0, 0, 3 + 4] and list(clean[10]["counts"]) == [0, 0, 3]


@pytest.mark.gpu
def test_an_image_energy_that_is_not_finite_fails_its_band_and_no_other():
    """finite forces, one NaN per-atom energy in an END image at step 3: no tangent is made from it"""
    S = _neb.surface_bands([(5, 66), (3, 2), (4, 5)], seed=11)
    n = int(S["cfg_first"][-1])
    row = int(S["cfg_first"][5]) + 1                                                 # the first image of the second band
    twin, x, v, _ = _neb.run_surface(S, 8, nan_energy_at=(3, row), climb_step=2)
    twin.assert_margins()
    assert list(twin.status) == [0, _neb.FAILED, 0] and twin.done_step[1] == 3 and twin.count == 3

    got, _ = _device_bands(S, 8, nan_energy_at=(3, row), climb_step=2)
    want = dict(x=x, v=v, dt=twin.dt, alpha=twin.alpha, fmax=twin.fmax, fneb=twin.fneb, energy=twin.energy.copy(), npos=twin.npos,
                frozen=twin.frozen, done_step=twin.done_step, climber=twin.climber, status=twin.status, count=twin.count)
    assert np.isnan(got["energy"][5]) and np.isnan(want["energy"][5])                # (the energies are written before the band fails)
    got["energy"][5] = want["energy"][5] = 0.0
    assert got["fmax"][1] == 0.0 and got["climber"][1] == -1 and list(got["frozen"][5:8]) == [3, 3, 3]
    _assert_follows(got, want, n, "after step 7, a NaN energy at step 3:")


@pytest.mark.gpu
def test_a_frozen_end_image_stops_its_band_and_last_only_decides():
    S = _neb.surface_bands([(5, 66), (3, 2), (4, 5)], seed=11)
    n = int(S["cfg_first"][-1])
    frozen = np.zeros(12, dtype=np.int32)
    frozen[7] = 1                                                                    # the LAST image of the second band
    twin, x, v, kept = _neb.run_surface(S, 6, frozen=frozen, keep=(4,), last_at=5, climb_step=2)
    twin.assert_margins()
    got, dev_kept = _device_bands(S, 6, frozen, keep=(4,), last_at=5, climb_step=2)
    assert list(got["status"]) == [0, _neb.CAPTURED, 0] and list(got["done_step"]) == [-1, 0, -1]
    assert list(got["frozen"]) == [0] * 5 + [1] * 3 + [0] * 4 and list(got["counts"]) == [0, 0, 2]
    before = dev_kept[4]
    for key in ("x", "v", "dt", "alpha", "npos"):                                    # step 5 was made with `last`
        assert np.array_equal(got[key], before[key]), key
    assert not np.array_equal(got["fneb"], before["fneb"]) and not np.array_equal(got["energy"], before["energy"])
    assert not np.array_equal(got["fmax"], before["fmax"])
    want = dict(x=x, v=v, dt=twin.dt, alpha=twin.alpha, energy=twin.energy, fneb=twin.fneb, fmax=twin.fmax, npos=twin.npos,
                frozen=twin.frozen, done_step=twin.done_step, climber=twin.climber, status=twin.status, count=twin.count)
    _assert_follows(got, want, n, "after the deciding step 5:")
    assert _rel(before["x"][:n], kept[4]["x"]) <= 1e-12


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S = _neb.surface_bands([(3, 3), (4, 70)], seed=3)
    n, ncfg, nband = int(S["cfg_first"][-1]), 7, 2
    rng = np.random.default_rng(0)
    e, f = _neb.surface(np, S["x0"], *[S[k] for k in _neb.SURFACE_KEYS])
    A = dict(band_first=to(S["band_first"]), cfg_first=to(S["cfg_first"]), x=to(S["x0"]), v=to(rng.normal(size=(n, 3))), f=to(f),
             eatom=to(e), type=to(S["types"]), inv_mass=to(1.0 / _neb.SURFACE_MASSES), origins=to(S["origins"]),
             cell=to(S["cells"].reshape(nband, 9)), cell_inv=to(np.linalg.inv(S["cells"]).reshape(nband, 9)), fneb=to(np.zeros((n, 3))),
             energy=to(np.zeros(ncfg)), dt=to(np.full(nband, 1e-3)), alpha=to(np.full(nband, 0.1)), npos=to(np.zeros(nband, dtype=np.int32)),
             done_step=to(np.full(nband, -1, dtype=np.int32)), fmax=to(np.zeros(nband)), climber=to(np.full(nband, -1, dtype=np.int32)),
             band_status=to(np.zeros(nband, dtype=np.int32)), frozen=to(np.zeros(ncfg, dtype=np.int32)),
             counts=to(np.zeros(3, dtype=np.int32)))
    before = {k: t.clone() for k, t in A.items()}

    def call(stream=st, step=0, band_first=S["band_first"], ncfg=ncfg, missing=None, **kw):
        p = dict(_neb.DEFAULTS, **kw)
        par = capi.NebParams(capi.RelaxParams(p["ftol"], p["dt_max"], p["dmax"], p["f_inc"], p["f_dec"], p["alpha_start"], p["f_alpha"],
                                              p["n_min"]), p["spring"], p["climb_step"])
        capi.neb_step(band_first, ncfg, par, step, {k: t for k, t in A.items() if k != missing}, stream=stream)

    nan, inf = float("nan"), float("inf")
    many = capi.NEB_MAX_IMAGES + 1
    bad = [dict(stream=None), dict(step=-1), dict(ncfg=-1), dict(ncfg=6), dict(spring=0.0), dict(spring=-5.0), dict(spring=nan),
           dict(spring=inf), dict(ftol=-1e-3), dict(ftol=nan), dict(dt_max=0.0), dict(dt_max=inf), dict(dmax=0.0), dict(dmax=nan),
           dict(f_inc=0.99), dict(f_inc=inf), dict(f_dec=0.0), dict(f_dec=1.0), dict(f_dec=nan), dict(alpha_start=-0.1),
           dict(alpha_start=1.1), dict(f_alpha=0.0), dict(f_alpha=1.01), dict(n_min=-1),
           dict(band_first=np.array([0, 2, 7])), dict(band_first=np.array([0, 3, 5])), dict(band_first=np.array([-1, 3, 7])),
           dict(band_first=np.array([0, many]), ncfg=many), dict(band_first=np.array([3, 0, 7]))]
    bad += [dict(missing=k) for k in capi.NEB_ARRAYS]
    for kw in bad:
        with pytest.raises(capi.MtpError) as ei:
            call(**kw)
        assert ei.value.code == -20, kw
    torch.cuda.synchronize()
    for k, t in A.items():
        assert torch.equal(t, before[k]), k
    with pytest.raises(capi.MtpError) as ei:                                         # an empty host table: nband = -1
        call(band_first=np.zeros(0, dtype=np.int32))
    assert ei.value.code == -20
    call(band_first=np.array([0]), missing="x")                                      # no band: nothing to launch, nothing to miss
    call(ftol=0.0, f_inc=1.0, alpha_start=0.0, f_alpha=1.0, n_min=0, climb_step=0, spring=1e-300)   # the ends of the ranges are inside
    torch.cuda.synchronize()
    assert not torch.equal(A["v"], before["v"]) and list(A["climber"].cpu().numpy()) == [1, 1 + int(np.argmax(A["energy"].cpu().numpy()[4:6]))]
    # a device table that disagrees with the host's (which passed the check): its first band has two images and is skipped, its
    # second starts inside the first and has images of 3 and of 70 atoms -- it fails, and no row of either is touched
    keep = {k: t.clone() for k, t in A.items()}
    A["band_first"] = to(np.array([0, 2, 7], dtype=np.int32))
    call()
    torch.cuda.synchronize()
    assert list(A["band_status"].cpu().numpy()) == [0, 3] and list(A["frozen"].cpu().numpy()) == [0, 0, 3, 3, 3, 3, 3]
    assert list(A["counts"].cpu().numpy()) == [0, 0, 5] and list(A["done_step"].cpu().numpy()) == [keep["done_step"][0].item(), 0]
    for k in ("x", "v", "fneb", "energy", "dt", "alpha", "npos"):
        assert torch.equal(A[k], keep[k]), k
    # 64 images are a band: one atom each on a straight line through its well
    T = _neb.surface_bands([(capi.NEB_MAX_IMAGES, 1)], seed=4)
    twin, x, v, _ = _neb.run_surface(T, 5)
    got, _ = _device_bands(T, 5)
    assert _rel(got["x"][:64], x) <= 1e-12 and got["v"][1:63].any() and list(got["status"]) == [0]


# ---- the whole loop ------------------------------------------------------------------------------------------------------

POTS = [("W_L8.mtp", 1), ("WRe_L20.mtp", 2)]


def _displaced_bands(species, seed=21, nimages=5):
    """a band per configuration of _batch.mixed_batch with more than one atom (one atom alone in a periodic cell has the same
    energy wherever it is: every comparison of the tangent rule would be a tie): from the configuration to a copy with every
    coordinate displaced by at most 0.3 A"""
    from lammps_mtp_kokkos_amd.md import interpolate_band
    rng = np.random.default_rng(seed)
    bands = []
    for pos, cell, types in _batch.mixed_batch(species):
        if len(pos) > 1:
            bands.append((interpolate_band(pos, pos + rng.uniform(-0.3, 0.3, pos.shape), cell, nimages), cell, types))
    return bands


def _assert_bands_follow(got, ref, bands, what):
    configs, band_first = _neb.flatten(bands)
    worst = [0.0, 0.0, 0.0]
    for k, (pos, cell, _) in enumerate(configs):
        dx = _sample.wrapped_diff(got["final"][k]["x"], ref["final_x"][k], cell)
        de = float(np.abs(got["trace"]["energy"][:, k] - ref["energy"][:, k]).max())
        worst = [max(worst[0], dx), max(worst[1], de), worst[2]]
    for b, (images, cell, _) in enumerate(bands):
        r, k0 = got["bands"][b], int(band_first[b])
        df = float(np.abs(got["trace"]["fmax"][:, b] - ref["fmax"][:, b]).max())
        worst[2] = max(worst[2], df)
        print("%s, band %d (%d images of %d atoms): dfmax %.3e, %s at %d, barriers %.6f %.6f" %
              (what, b, len(images), len(images[0]), df, r["status"], r["step"], r["barrier_forward"], r["barrier_backward"]))
        assert r["status"] == capi.NEB_STATUS[ref["status"][b]] and r["step"] == ref["done_step"][b]
        assert abs(r["dt"] - ref["dt"][b]) <= 1e-12 * ref["dt"][b] and abs(r["fmax"] - ref["fmax"][-1, b]) < V_TOL
        e = ref["energy"][-1, k0: k0 + len(images)]
        assert np.abs(r["energies"] - e).max() < E_TOL and r["highest"] == int(np.argmax(e))
        assert abs(r["barrier_forward"] - (e.max() - e[0])) < 2 * E_TOL and abs(r["barrier_backward"] - (e.max() - e[-1])) < 2 * E_TOL
        # images: continuous along the band, each the final configuration up to lattice vectors
        inv = np.linalg.inv(cell)
        for i, img in enumerate(r["images"]):
            assert img.shape == images[0].shape and _sample.wrapped_diff(img, ref["final_x"][k0 + i], cell) < X_TOL
            if i:
                d = img - r["images"][i - 1]
                assert np.abs(d - _neb.mic(d, cell, inv)).max() == 0.0
    print(what, "worst dx %.3e dE %.3e dfmax %.3e" % tuple(worst))
    assert worst[0] < X_TOL and worst[1] < E_TOL and worst[2] < V_TOL, worst


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_neb_cells_follows_the_host_driven_loop(fname, species):
    """bands of 5 images over 2, 5, 8 and 54 atoms, 12 steps with dmax = 0.02 A, the climbing image from step 4: no atom
    travels further than 12 x 0.02 x sqrt(3) < 0.42 A from images that are themselves within 0.3 A of configurations whose
    closest pair is 2.4 A apart.  every=3: the rebuild in slot coordinates runs, and wraps every image on its own."""
    from lammps_mtp_kokkos_amd.md import neb_cells
    bands = _displaced_bands(species)
    ctx = _ctx(fname)
    kw = dict(masses=MASSES[species], list_cutoff=LIST_CUTOFF, dmax=0.02, spring=5.0)
    ref = _neb.reference_loop(ctx, bands, 12, climb_step=4, **kw)
    ref["twin"].assert_margins()
    got = neb_cells(ctx, bands, 12, climb_after=4, every=3, trace=True, **kw)
    assert got["steps_done"] == ref["steps_done"] == 12 and got["records"] == [] and got["candidates"] == [] and got["dropped"] == 0
    assert got["builds"] >= 4 and got["trace"]["fmax"].shape == (13, len(bands)) and got["trace"]["energy"].shape == (13, 5 * len(bands))
    _assert_bands_follow(got, ref, bands, fname)
    moved = max(np.abs(ref["final_x"][k] - c[0]).max() for k, c in enumerate(_neb.flatten(bands)[0]))
    assert moved > 1e-3 and (ref["twin"].climber > 0).all()
    for b, (images, _, _) in enumerate(bands):                                       # the ends: where they were given
        assert _sample.wrapped_diff(got["bands"][b]["images"][0], images[0], bands[b][1]) < X_TOL
        assert _sample.wrapped_diff(got["bands"][b]["images"][-1], images[-1], bands[b][1]) < X_TOL
    with pytest.raises(capi.MtpError) as ei:                                         # no selection state
        neb_cells(ctx, bands, 1, threshold_break=5.0)
    assert ei.value.code == -23


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species,cell_of", [("W_L8.mtp", 1, "cubic2_cell"), ("WRe_L20.mtp", 2, "tilted5_cell")])
def test_a_band_into_a_basin_converges_and_ends_early(fname, species, cell_of):
    """a basin path (the generated potentials have holes at short range, and a vacancy hop falls into one): the last image is the
    relaxed cell, the first that plus a centred random displacement of amplitude 0.25 A, 5 images, spring 5, no climbing image.
    The host-driven loop on the CPU oracle converged such bands to ftol 1e-3 at steps 153 and 167 with closest approaches of 2.29 A
    and 3.08 A; the step asserted is the one the host-driven loop of this run finds."""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, interpolate_band, neb_cells, relax_cells
    pos, cell, types = getattr(_cells, cell_of)()
    ctx = _ctx(fname)
    kw = dict(masses=MASSES[species], list_cutoff=LIST_CUTOFF)
    low = relax_cells(ctx, [(pos, cell, types)], 400, ftol=1e-5, **kw)["final"][0]
    assert low["status"] == "converged"
    rng = np.random.default_rng(31)
    d = rng.uniform(-0.25, 0.25, pos.shape)
    bands = [(interpolate_band(low["x"] + d - d.mean(0), low["x"], cell, 5), cell, types)]
    ref = _neb.reference_loop(ctx, bands, 250, **kw)
    ref["twin"].assert_margins()
    done = int(ref["done_step"][0])
    assert ref["status"][0] == _neb.CONVERGED and 0 < done < 250
    got = neb_cells(ctx, bands, 250, **kw)
    r = got["bands"][0]
    print("%s: converged at step %d, steps_done %d, builds %d, energies %s" % (fname, done, got["steps_done"], got["builds"], r["energies"]))
    assert r["status"] == "converged" and r["step"] == done and r["fmax"] <= 1e-3
    assert done <= got["steps_done"] <= done + 4 < 250                               # seen at the next read (check_every = 4)
    again = evaluate_cells(ctx, [(img, cell, types) for img in r["images"]], list_cutoff=LIST_CUTOFF, vflag=0)
    E = np.array([a["energy"] for a in again])
    fn, bad = _neb.neb_force(r["images"], [a["f"] for a in again], E, cell, np.linalg.inv(cell), 5.0)
    fmax = max(float(np.sqrt((q ** 2).sum(1)).max()) for q in fn)
    print("fmax of F_neb at the returned images %.6e (reported %.6e)" % (fmax, r["fmax"]))
    assert not bad and fmax <= 1e-3 + 1e-9
    assert np.abs(E - r["energies"]).max() < E_TOL and np.abs(r["energies"] - ref["energy"][-1]).max() < E_TOL
    assert r["highest"] == 0 and r["barrier_forward"] == 0.0 and r["barrier_backward"] > 0.0


def _graded_run(bands, ctx, **kw):
    natoms = [len(c[0]) for c in _neb.flatten(bands)[0]]
    table = _neb.reference_loop(ctx, bands, 12, select=BIG, brk=BIG, **kw)["grades"]
    assert sorted(table) == [0, 4, 8, 12]
    return sorted([_midpoint_threshold(table, natoms), _midpoint_threshold(table, natoms, central=True)]), table


@pytest.mark.gpu
def test_capture_under_neb_stops_the_band_and_feeds_select_cells():
    """W_L16_nbh.almtp, grade steps 0, 4, 8, 12, thresholds as in the capture test of tests/test_relax_gpu.py.  The capture
    precedes mtp_neb_step: an image over threshold_break freezes, and rule 1 stops its band in the same step."""
    from lammps_mtp_kokkos_amd.md import neb_cells, select_cells
    bands = _displaced_bands(1)
    configs, band_first = _neb.flatten(bands)
    ctx = _ctx("W_L16_nbh.almtp", True)
    kw = dict(masses=MASSES[1], list_cutoff=LIST_CUTOFF, dmax=0.02, grade_every=4)
    (select, brk), table = _graded_run(bands, ctx, **kw)
    for s in sorted(table):
        print("step %2d grades" % s, table[s])
    print("threshold_select %.9g threshold_break %.9g" % (select, brk))
    ref = _neb.reference_loop(ctx, bands, 12, select=select, brk=brk, **kw)
    ref["twin"].assert_margins()
    want = ref["capture"].records
    print("records", want, "status", ref["status"])
    assert len(want) > 0 and (ref["status"] == _neb.CAPTURED).any(), "the test's inputs are wrong: no band is stopped by a capture"
    got = neb_cells(ctx, bands, 12, threshold_select=select, threshold_break=brk, every=20, trace=True, **kw)
    assert got["builds"] == 1 and got["dropped"] == 0
    assert [(k, s) for k, s, _ in got["records"]] == [(k, s) for k, s, _ in want]
    assert [r["status"] for r in got["bands"]] == [capi.NEB_STATUS[q] for q in ref["status"]]
    assert [r["step"] for r in got["bands"]] == list(ref["done_step"])
    for (k, s, g), (_, _, gw), (pos, cell, types), xs in zip(got["records"], want, got["candidates"], ref["snapshots"]):
        assert abs(g - gw) <= 1e-9 * max(1.0, abs(gw)), (k, s, g, gw)
        assert _sample.wrapped_diff(pos, xs, configs[k][1]) < 1e-9 and np.array_equal(cell, configs[k][1]) and np.array_equal(types, configs[k][2])
    for k, (pos, cell, _) in enumerate(configs):
        assert _sample.wrapped_diff(got["final"][k]["x"], ref["final_x"][k], cell) < X_TOL
    sel = select_cells(ctx, got["candidates"], threshold=1.1, list_cutoff=LIST_CUTOFF, max_swaps=0)
    for gb, (_, _, g) in zip(sel["grade_before"], got["records"]):
        assert abs(gb - g) <= 1e-9 * max(1.0, g)


@pytest.mark.gpu
def test_bands_split_into_passes_have_the_run_of_the_whole_batch():
    """max_atoms_per_pass = 35 puts the bands of 2 and 5 atoms in one pass and those of 8 and 54 in a pass each; = 1 gives every
    band its own.  A pass is a complete run of its bands; slot translation costs bits: the bounds are the trajectory bounds."""
    from lammps_mtp_kokkos_amd.md import neb_cells, plan_band_passes
    bands = _displaced_bands(1)
    configs, band_first = _neb.flatten(bands)
    ctx = _ctx("W_L8.mtp")
    cells, natoms = np.array([c[1] for c in configs]), np.array([len(c[0]) for c in configs])
    run = lambda cap: neb_cells(ctx, bands, 12, climb_after=4, every=20, max_atoms_per_pass=cap, trace=True, masses=MASSES[1],
                                list_cutoff=LIST_CUTOFF, dmax=0.02)
    whole = run(None)
    assert whole["builds"] == 1 and whole["steps_done"] == 12
    for cap, passes in ((35, [(0, 10), (10, 15), (15, 20)]), (1, [(0, 5), (5, 10), (10, 15), (15, 20)])):
        assert [(a, b) for a, b, _ in plan_band_passes(cells, natoms, band_first, LIST_CUTOFF, cap)[0]] == passes
        got = run(cap)
        assert got["builds"] == len(passes) and got["steps_done"] == 12 and got["dropped"] == 0
        de = float(np.abs(got["trace"]["energy"] - whole["trace"]["energy"]).max())
        df = float(np.abs(got["trace"]["fmax"] - whole["trace"]["fmax"]).max())
        dx = max(_sample.wrapped_diff(got["final"][k]["x"], whole["final"][k]["x"], c[1]) for k, c in enumerate(configs))
        print("max_atoms_per_pass %d: passes %r, dE %.3e dfmax %.3e dx %.3e" % (cap, passes, de, df, dx))
        assert de < E_TOL and df < V_TOL and dx < X_TOL
        for r, w in zip(got["bands"], whole["bands"]):
            assert r["status"] == w["status"] and r["step"] == w["step"] and r["highest"] == w["highest"]
            assert abs(r["dt"] - w["dt"]) <= 1e-12 * w["dt"] and np.abs(r["energies"] - w["energies"]).max() < E_TOL
