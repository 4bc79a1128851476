"""The batched minimiser without a GPU: the numpy twin of mtp_relax_step (tests/_relax.py) on anisotropic harmonic wells --
it converges, lowers the energy, and takes both the uphill branch and the displacement cap -- its edge rules, and the
argument checks of md.relax_cells, which are made before anything touches the device."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

import _batch
import _relax
from _stub_run import StubRun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_converges_every_live_well_through_the_uphill_branch_and_the_cap():
    cf, types, x_eq, x0, kk = _relax.wells()
    frozen = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.int32)
    twin, x, v, _ = _relax.run_wells(cf, types, x_eq, x0, kk, 200, frozen=frozen, dt_max=2e-2)
    twin.assert_margins()
    print("done_step", twin.done_step, "uphill", twin.uphill, "capped", twin.capped, "margins", twin.margin_p, twin.margin_tol)
    live = (np.diff(cf) > 0) & (frozen == 0)
    assert (twin.frozen[live] == _relax.CONVERGED).all() and (twin.done_step[live] > 0).all() and twin.count == int(live.sum())
    assert twin.frozen[0] == 0 and twin.frozen[3] == 1 and twin.done_step[0] == twin.done_step[3] == -1
    e0, e1 = _relax.well_energy(x0, x_eq, kk, cf), _relax.well_energy(x, x_eq, kk, cf)
    assert (e1[live] < e0[live]).all()
    assert (twin.fmax[live] <= 1e-3).all()
    assert twin.uphill >= 1 and twin.capped >= 1
    assert np.array_equal(x[cf[3]:cf[4]], x0[cf[3]:cf[4]])                          # the frozen configuration: never written


def test_twin_edge_rules():
    cf = np.array([0, 2, 2, 4, 6])                                                  # live, empty, frozen, live
    inv_m = np.full(6, 1.0 / 183.84)
    rng = np.random.default_rng(1)
    x0 = rng.normal(size=(6, 3))
    f = rng.normal(size=(6, 3))
    # at rest (step 0): the branch of P <= 0, and dt is not shrunk
    twin = _relax.Twin(cf, 1e-3, frozen=[0, 0, 1, 0])
    x, v = x0.copy(), np.zeros((6, 3))
    twin.step(0, x, v, f, inv_m)
    assert list(twin.dt) == [1e-3] * 4 and list(twin.npos) == [0] * 4 and twin.uphill == 0
    assert np.array_equal(x, x0)                                                    # v' = 0: the first step only kicks
    assert np.array_equal(x[2:4], x0[2:4]) and not v[2:4].any() and v[:2].all() and v[4:].all()
    assert twin.fmax[1] == 0.0 and twin.fmax[2] == 0.0 and twin.done_step[2] == -1  # empty and frozen: nothing written
    # uphill with vv > 0 does shrink it, and stops the configuration
    twin.step(1, x, v, -f, inv_m)
    assert twin.dt[0] == 0.5e-3 and twin.dt[3] == 0.5e-3 and twin.dt[2] == 1e-3 and twin.uphill == 2
    # a NaN force: failed, rows untouched, counted once, and never looked at again
    fn = -f                                                                         # (downhill for the first one: it moves)
    fn[5, 1] = np.nan
    xb, vb, dtb = x.copy(), v.copy(), twin.dt.copy()
    twin.step(2, x, v, fn, inv_m)
    assert twin.frozen[3] == _relax.FAILED and twin.done_step[3] == 2 and twin.count == 1
    assert np.array_equal(x[4:], xb[4:]) and np.array_equal(v[4:], vb[4:]) and twin.dt[3] == dtb[3]
    assert not np.array_equal(x[:2], xb[:2])
    twin.step(3, x, v, f, inv_m)
    assert twin.done_step[3] == 2 and np.array_equal(x[4:], xb[4:]) and twin.count == 1
    # converged: v = 0, x not written
    small = 1e-4 * f / np.abs(f).max()
    xb = x.copy()
    assert v[:2].any()
    twin.step(4, x, v, small, inv_m)
    assert twin.frozen[0] == _relax.CONVERGED and twin.done_step[0] == 4 and not v[:2].any() and np.array_equal(x[:2], xb[:2])
    assert twin.count == 2 and np.array_equal(x[2:4], x0[2:4])
    # the last launch only decides
    twin = _relax.Twin(cf, 1e-3)
    x, v = x0.copy(), np.zeros((6, 3))
    twin.step(0, x, v, f, inv_m, last=True)
    assert np.array_equal(x, x0) and not v.any() and not twin.frozen.any() and twin.fmax[0] > 0.0


def test_relax_cells_checks_its_arguments_before_the_device(monkeypatch):
    from lammps_mtp_kokkos_amd import md

    def touched(*a, **k):
        raise AssertionError("the device was touched")

    for name in ("Ghosts", "use_private_torch_stream", "relax_step", "batch_layout"):
        monkeypatch.setattr(capi, name, touched)
    batch = _batch.mixed_batch(1)

    class Ctx:                                                                       # (no context without a GPU)
        pot = capi.Potential(os.path.join(ROOT, "potentials", "W_L8.mtp"))

    bad = [dict(steps=-1), dict(ftol=-1e-3), dict(ftol=float("nan")), dict(dt=0.0), dict(dt_max=0.0), dict(dmax=0.0),
           dict(dmax=float("inf")), dict(f_inc=0.9), dict(f_dec=1.0), dict(f_dec=0.0), dict(alpha_start=1.5), dict(alpha_start=-0.1),
           dict(f_alpha=0.0), dict(f_alpha=1.1), dict(n_min=-1), dict(masses=0.0), dict(masses=[183.84, -1.0]), dict(every=0),
           dict(check_every=-1), dict(capture_gap=-1), dict(grade_every=-1), dict(max_candidates=-1),
           dict(threshold_select=3.0, threshold_break=2.0)]
    for kw in bad:
        kw = dict(dict(steps=5), **kw)
        with pytest.raises(ValueError, match="relax_cells"):
            md.relax_cells(Ctx, batch, **kw)
    with pytest.raises(ValueError, match="types for"):
        md.relax_cells(Ctx, [(np.zeros((2, 3)), np.eye(3) * 5.0, [1])], 5)
    with pytest.raises(ValueError, match="count from 1"):
        md.relax_cells(Ctx, [(np.zeros((1, 3)), np.eye(3) * 5.0, [0])], 5)
    for kw in (dict(threshold_select=2.0), dict(threshold_break=5.0)):               # no selection state
        with pytest.raises(capi.MtpError) as ei:
            md.relax_cells(Ctx, batch, 5, **kw)
        assert ei.value.code == -23


@pytest.mark.parametrize("kw,answers,want,s_want", [
    (dict(steps=5, every=3, check_every=2), (), "F S0 M | F S1 M | F S2 M B | F S3 | F S4 M | F S5last", 5),
    (dict(steps=5, every=3, check_every=0), (), "F S0 M | F S1 | F S2 M B | F S3 | F S4 | F S5last", 5),
    (dict(steps=5, every=3, check_every=2), [(False, False), (False, True)],
     "F S0 M | F S1 M B | F S2 | F S3 M | F S4 M B | F S5last", 5),
    (dict(steps=5, every=3, check_every=2), [(True, False)], "F S0 M", 0),
    (dict(steps=0, every=3, check_every=2), (), "F S0last", 0),
    (dict(steps=5, every=3, check_every=2, grade_every=2), (), "F C0 S0 M | F S1 M | F C2 S2 M B | F S3 | F C4 S4 M | F S5last", 5),
], ids=["cadence", "no-checks", "stale", "all-done", "no-steps", "graded"])
def test_the_minimiser_loop_asks_the_run_in_the_order_of_relax_cells(kw, answers, want, s_want):
    """md._minimise_pass, the step loop of relax_cells and relax_cells_vc, with a run that has no device behind it.  The
    sequences are read off the loop relax_cells had of its own: forces, on a grade step the capture, the minimiser launch; then
    since += 1, the read after step 0, at since >= every and at since % check_every == 0, the all-done break, the rebuild when
    due or stale (since = 0).  Case "stale": the rebuild of step 1 restarts the count, so the next reads are those of steps 3
    (since = 2) and 4 (since = 3 = every)."""
    from lammps_mtp_kokkos_amd import md
    run = StubRun(answers)
    ge = kw.get("grade_every", 0)
    s = md._minimise_pass(run, kw["steps"], lambda step: bool(ge) and step % ge == 0, run.step, kw["every"], kw["check_every"])
    assert " ".join(run.log) == want.replace(" |", "")
    assert s == s_want and run.log.count("B") == want.count("B")
    assert run.graded_forces == [bool(ge) and q % ge == 0 for q in range(len(run.graded_forces))]
    assert run.moves == sum(1 for w in run.log if w.startswith("S") and not w.endswith("last"))     # after every move, and only then
