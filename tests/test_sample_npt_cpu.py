"""The batched constant-pressure sampler without a GPU: the numpy twin of mtp_sample_cell_step (tests/_sample_npt.py) defines
the physics.  The ideal gas in an isotropic cell must hold the volume (N + 1) kT / p -- and must miss it by 20 % with the
`+ kT I` term taken out of the drift --, a fully flexible cell on the analytic model of tests/_relax_vc.py must satisfy the
stationarity identity <(Wt - p V I)_ab> = -kT delta_ab, the isotropic, masked and switched-off barostats keep to the bit what
they must keep, the argument errors of md.sample_cells_npt come before the device is touched, and the barostat's noise
counters never meet an atom's.

Time steps.  Both statistical tests use dt = 4 fs.  The ideal gas (tau_p = 1 ps, compressibility 1 / p, t_damp = 1 ps) gave
<V> / ((N + 1) kT / p) = 1.012, 1.005, 1.003 (+- 0.007, 0.007, 0.003) at dt = 8, 4, 2 fs: the mean stops moving within its error
at 4 fs, and the O(dt) bias left there is below 1 %, the allowance of the test.  The flexible cell (tau_p = 0.5 ps) gave diagonal
means of -1.13, -1.35, -1.18 kT at 4 fs and -1.06, -1.16, -1.14 kT at 2 fs (+- 0.15 kT each): no trend beyond the error; the
allowance is 0.2 kT."""
import numpy as np
import pytest

import _cells
import _relax_vc
import _sample
import _sample_npt
from _relax_vc import GPA
from _sample import KB, MVV2E
from _sample_npt import Twin, det3

DT, SEED = 4e-3, 11


def _ideal_gas(steps, with_kt, dt=DT, tau_p=1.0, ncfg=256, natoms=4, T=300.0, vmean=100.0, t_damp=1.0):
    """f = 0 and W = 0: 256 independent configurations of 4 atoms in cubic cells, isotropic barostat at the pressure that makes
    (N + 1) kT / p = vmean, thermostat by tests/_sample.py.  Returns the volumes [steps, ncfg], the twin and the pressure."""
    kT = KB * T
    p = (natoms + 1) * kT / vmean
    n = ncfg * natoms
    edge = vmean ** (1.0 / 3.0)
    rng = np.random.default_rng(SEED)
    m, inv_m = np.full(n, 183.84), np.full(n, 1.0 / 183.84)
    x = rng.random((n, 3)) * edge
    v = rng.normal(size=(n, 3)) * np.sqrt(kT / (183.84 * MVV2E))
    keys = np.arange(ncfg, dtype=np.uint64) + np.uint64(1000)
    twin = Twin(np.arange(ncfg + 1) * natoms, np.tile(np.eye(3) * edge, (ncfg, 1, 1)), T, keys, dt, p, 1.0 / p, tau_p, isotropic=True,
                strain_max=0.05, seed=SEED, with_kt=with_kt)
    index, key_row, T_row = np.tile(np.arange(natoms), ncfg).astype(np.uint64), keys[twin.cfg_row], np.full(n, T)
    moving, W, f = np.ones(n, dtype=bool), np.zeros((ncfg, 6)), np.zeros((n, 3))
    _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, 0.0, 0, index, key_row, SEED, moving)
    vols = np.zeros((steps, ncfg))
    for s in range(1, steps + 1):
        twin.step(s, x, v, f, W, m, inv_m)
        f = np.zeros((n, 3))
        _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, twin.dtf, s, index, key_row, SEED, moving)
        vols[s - 1] = det3(twin.h)
    return vols, twin, p


def test_the_ideal_gas_holds_the_volume_of_its_marginal_and_misses_it_without_the_kT_term():
    """the marginal of the target over the atoms is V^N exp(-beta p V) dV: <V> = (N + 1) kT / p = 100 A^3.  Without `+ kT I` the
    scheme samples V^(N - 1) exp(-beta p V): N kT / p = 80 A^3.  2000 steps of 4 fs, the first 2 ps (two barostat times; the
    volume relaxes in tau_p / 3) left out; the mean over the configurations, 16 blocks.  Bound: 5 standard errors plus 1 % of the
    target for the time step (module docstring)."""
    want, allowance, steps, skip = 100.0, 1.0, 2000, 500
    vols, twin, p = _ideal_gas(steps, True)
    mean, err = _sample_npt.block_error(vols[skip:].mean(1))
    print("dt %g ps, tau_p 1 ps, %d steps: <V> = %.3f +- %.3f A^3, (N + 1) kT / p = %.1f; capped %d" % (DT, steps, mean, err, want, twin.capped.sum()))
    assert abs(twin.press.mean() - p) < 0.5 * p and not twin.frozen.any()
    assert err < 1.5 and abs(mean - want) <= 5.0 * err + allowance
    vols, twin, _ = _ideal_gas(steps, False)
    mean0, err0 = _sample_npt.block_error(vols[skip:].mean(1))
    print("without the kT term: <V> = %.3f +- %.3f A^3, N kT / p = %.1f" % (mean0, err0, 0.8 * want))
    assert err0 < 1.5 and not abs(mean0 - want) <= 5.0 * err0 + allowance            # the negative control: it must FAIL the bound ...
    assert abs(mean0 - 0.8 * want) <= 5.0 * err0 + allowance                         # ... and sit at N kT / p


def test_a_fully_flexible_cell_is_stationary_on_the_model():
    """256 configurations of 4 atoms of the analytic model with a soft cell (K2 |h|^4 of a few eV, so that kT shows against the
    fluctuations of W), p = 0.1 GPa, all six components free.  Stationarity of exp(-beta (K + U + p V)) V against the Haar measure
    under h -> h exp(t S) gives <(Wt - p V I) : S> = -kT tr S for every symmetric S: -kT on the diagonal, 0 off it.  2500 steps of
    4 fs, the first 3 ps left out; 5 block-averaged standard errors plus 0.2 kT for the time step (module docstring)."""
    ncfg, natoms, T, tau_p, t_damp, p, steps, skip = 256, 4, 300.0, 0.5, 0.1, 0.1 * GPA, 2500, 750
    kT = KB * T
    model = _relax_vc.Model(sizes=[natoms] * ncfg, k_cfg=[2.0] * ncfg, k2=6e-3, seed=SEED, a0=3.0, strain=0.0, noise=0.05)
    n = model.n
    m, inv_m = _relax_vc.MODEL_MASSES[model.types - 1], model.inv_m
    stiffness = 2.0 * model.k2[0] * 3.0 ** 4                                         # d2E/d(eps_aa)2 of the cell term at h = a0 I
    x = model.x0.copy()
    v = np.random.default_rng(SEED + 1).normal(size=(n, 3)) * np.sqrt(kT / (m * MVV2E))[:, None]
    keys = np.arange(ncfg, dtype=np.uint64) + np.uint64(1000)
    twin = Twin(model.cf, model.h0, T, keys, DT, p, 3.0 * det3(model.h0).mean() / stiffness, tau_p, strain_max=0.05, seed=SEED)
    index, key_row, T_row = np.tile(np.arange(natoms), ncfg).astype(np.uint64), keys[twin.cfg_row], np.full(n, T)
    moving = np.ones(n, dtype=bool)
    _, f, W = _sample_npt.model_all(model, x, twin.h)
    e1, f1, W1 = model.all(x, twin.h)                                                # (the vectorised model is the model)
    assert np.abs(f - f1).max() < 1e-12 and np.abs(W - W1).max() < 1e-12
    _sample.second_half(v, f, m, inv_m, T_row, t_damp, DT, 0.0, 0, index, key_row, SEED, moving)
    series = []
    for s in range(1, steps + 1):
        twin.step(s, x, v, f, W, m, inv_m)
        _, f, W = _sample_npt.model_all(model, x, twin.h)
        _sample.second_half(v, f, m, inv_m, T_row, t_damp, DT, twin.dtf, s, index, key_row, SEED, moving)
        if s > skip:
            g = W + twin.kinetic(m, v)
            g[:, :3] -= (p * det3(twin.h))[:, None]
            series.append(g.mean(0))
    mean, err = _sample_npt.block_error(np.array(series))
    want = np.array([-kT, -kT, -kT, 0.0, 0.0, 0.0])
    print("dt %g ps, tau_p %g ps: <(Wt - p V I)_ab> / kT =" % (DT, tau_p), np.round(mean / kT, 3), "+-", np.round(err / kT, 3), "capped", twin.capped.sum())
    assert not twin.frozen.any() and (err < 0.3 * kT).all()
    assert (np.abs(mean - want) <= 5.0 * err + 0.2 * kT).all()
    assert np.abs(twin.F - np.eye(3)).max() > 0.05                                   # (the cells did move, and sheared)
    assert np.abs(twin.F[:, 0, 1]).max() > 0.01


# ---- bits ----------------------------------------------------------------------------------------------------------------

def _model_run(steps=40, sizes=(2, 5, 0, 3), diagonal=False, **kw):
    """the twin on the small model with thermostat, `steps` steps at 1 GPa; returns the twin, x, v and the model"""
    model = _relax_vc.Model(sizes=list(sizes), k_cfg=(2.0, 5.0, 9.0, 3.0), seed=5)
    if diagonal:
        model.h0 = np.array([np.diag(np.diag(h)) for h in model.h0])
    n, T, dt, t_damp = model.n, 600.0, 2e-3, 0.1
    m, inv_m = _relax_vc.MODEL_MASSES[model.types - 1], model.inv_m
    x = model.x0.copy()
    v = np.random.default_rng(3).normal(size=(n, 3)) * np.sqrt(KB * T / (m * MVV2E))[:, None]
    keys = np.array([7, 2 ** 40 + 1, 9, 2 ** 63 + 5], dtype=np.uint64)
    kw.setdefault("tau_p", 0.2)
    twin = Twin(model.cf, model.h0, T, keys, dt, 1.0 * GPA, 0.05, seed=SEED, **kw)
    index = np.concatenate([np.arange(s) for s in sizes]).astype(np.uint64)
    key_row, T_row, moving = keys[twin.cfg_row], np.full(n, T), np.ones(n, dtype=bool)
    _, f, W = model.all(x, twin.h)
    _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, 0.0, 0, index, key_row, SEED, moving)
    for s in range(1, steps + 1):
        twin.step(s, x, v, f, W, m, inv_m)
        _, f, W = model.all(x, twin.h)
        _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, twin.dtf, s, index, key_row, SEED, moving)
    return twin, x, v, model


OFF = ~np.eye(3, dtype=bool)


def test_an_isotropic_barostat_keeps_the_shape_of_the_cell_to_the_bit():
    """every E is a multiple of I with three equal diagonal entries, so F = prod E (h . h0^-1 in exact arithmetic) has
    off-diagonals of exactly 0 and one diagonal value; for a diagonal h0 the same holds for h . h0^-1 as computed"""
    twin, _, _, model = _model_run(isotropic=True)
    for k in (0, 1, 3):
        assert (twin.F[k][OFF] == 0.0).all() and twin.F[k][0, 0] == twin.F[k][1, 1] == twin.F[k][2, 2] != 1.0
    assert np.array_equal(twin.F[2], np.eye(3)) and np.array_equal(twin.h[2], model.h0[2])      # the empty configuration
    twin, _, _, model = _model_run(isotropic=True, diagonal=True)
    for k in (0, 1, 3):
        r = twin.h[k] @ _relax_vc.inv3(model.h0[k], _relax_vc.det3(model.h0[k]))
        assert (r[OFF] == 0.0).all() and np.abs(np.diag(r) - twin.F[k][0, 0]).max() < 1e-14


def test_with_the_shear_mask_off_the_cell_is_not_sheared():
    twin, _, _, model = _model_run(cell_mask=(1, 1, 1, 0, 0, 0))
    for k in (0, 1, 3):
        d = np.diag(twin.F[k])
        assert (twin.F[k][OFF] == 0.0).all() and len({d[0], d[1], d[2], 1.0}) == 4
    twin, _, _, model = _model_run(cell_mask=(1, 1, 1, 0, 0, 0), diagonal=True)
    for k in (0, 1, 3):
        assert (twin.h[k][OFF] == 0.0).all() and (np.diag(twin.h[k]) != np.diag(model.h0[k])).all()


@pytest.mark.parametrize("off", [dict(cell_mask=(0, 0, 0, 0, 0, 0)), dict(tau_p=None), dict(tau_p=0.0), dict(tau_p=float("inf"))],
                         ids=["zero-mask", "tau_p-none", "tau_p-zero", "tau_p-inf"])
def test_a_barostat_that_is_off_leaves_the_cell_and_the_first_half_step_to_the_bit(off):
    twin, x, v, model = _model_run(**off)
    assert np.array_equal(twin.h, model.h0) and np.array_equal(twin.T, np.tile(np.eye(3), (4, 1, 1))) and not twin.cellmove.any()
    assert not twin.capped.any() and twin.press[[0, 1, 3]].all()
    # one more step by hand: tests/_sample.first_half on the same inputs
    rng = np.random.default_rng(0)
    f, W = rng.normal(size=x.shape), rng.normal(size=(4, 6))
    m, inv_m = _relax_vc.MODEL_MASSES[model.types - 1], model.inv_m
    x1, v1 = x.copy(), v.copy()
    _sample.first_half(x1, v1, f, inv_m, twin.dtf, twin.dt, np.ones(len(x), dtype=bool))
    twin.step(41, x, v, f, W, m, inv_m)
    assert np.array_equal(x, x1) and np.array_equal(v, v1)


def test_a_bad_virial_fails_its_configuration_in_the_twin():
    twin, x, v, model = _model_run(steps=3)
    m, inv_m = _relax_vc.MODEL_MASSES[model.types - 1], model.inv_m
    _, f, W = model.all(x, twin.h)
    W[1, 4] = np.nan
    h0, x0, v0 = twin.h.copy(), x.copy(), v.copy()
    twin.step(4, x, v, f, W, m, inv_m)
    a, b = int(model.cf[1]), int(model.cf[2])
    assert twin.frozen[1] == _relax_vc.FAILED and twin.done_step[1] == 4 and twin.count == 1
    assert np.array_equal(twin.h[1], h0[1]) and np.array_equal(x[a:b], x0[a:b]) and np.array_equal(v[a:b], v0[a:b])
    assert not np.array_equal(twin.h[0], h0[0]) and not np.array_equal(x[:a], x0[:a]) and list(twin.frozen) == [0, 3, 0, 0]


# ---- arguments and counters ----------------------------------------------------------------------------------------------

def test_argument_errors_of_sample_cells_npt_are_raised_before_the_device_is_touched():
    from lammps_mtp_kokkos_amd.md import sample_cells_npt
    batch = [_cells.cubic2_cell()]
    nan, inf = float("nan"), float("inf")
    bad = [dict(pressure=nan), dict(pressure=inf), dict(compressibility=0.0), dict(compressibility=-1.0), dict(compressibility=inf),
           dict(compressibility=nan), dict(t_damp=None), dict(t_damp=0.0), dict(t_damp=-0.1), dict(t_damp=inf), dict(strain_max=0.0),
           dict(strain_max=0.051), dict(strain_max=nan), dict(cell_mask=(1, 1, 1)), dict(cell_mask=(1, 1, 1, 2, 0, 0)),
           dict(cell_mask=(1, 1, 1, 0.5, 0, 0)), dict(cell_mask=1), dict(isotropic=True, cell_mask=(1, 1, 0, 0, 0, 0)),
           dict(isotropic=True, cell_mask=(0, 0, 0, 0, 0, 0)),
           # those of sample_cells
           dict(steps=-1), dict(dt=0.0), dict(dt=inf), dict(temperature=-1.0), dict(temperature=[300.0, 300.0]), dict(keys=[1, 2]),
           dict(masses=-1.0), dict(every=0), dict(max_candidates=-1), dict(capture_gap=-1), dict(velocities=[np.zeros((3, 3))]),
           dict(threshold_select=5.0, threshold_break=1.0)]
    for kw in bad:
        args = dict(temperature=300.0, pressure=0.0, steps=3, dt=1e-3, compressibility=0.5)
        args.update(kw)
        with pytest.raises(ValueError) as ei:                    # ctx = None: anything that touched it would not be a ValueError
            sample_cells_npt(None, batch, **args)
        assert "sample_cells_npt" in str(ei.value), kw
    with pytest.raises(TypeError):                               # compressibility has no default: it is the caller's estimate
        sample_cells_npt(None, batch, 300.0, 0.0, 3, 1e-3)


def test_the_noise_counters_differ_from_every_atom_counter():
    """an atom's counter is (step, index within its configuration < 2^31, key lo, key hi); the barostat's second word is
    2^31 + j.  Same step, same key: the words differ, and so do the outputs"""
    keys = np.array([0, 5, 2 ** 63 + 17, 2 ** 64 - 1], dtype=np.uint64)
    for step in (0, 1, 2 ** 30 - 1):
        c = _sample_npt.counters(step, keys)
        assert c.shape == (4, 2, 4) and (c[:, :, 1] >= 2 ** 31).all() and (c[:, :, 1] < 2 ** 32).all()
        assert (c[:, :, 0] == step).all() and np.array_equal(c[:, 0, 2:], c[:, 1, 2:]) and (c[:, 0, 1] != c[:, 1, 1]).all()
        assert np.array_equal(c[:, 0, 2] | (c[:, 0, 3] << np.uint64(32)), keys)
    # the largest index an atom can have (rows are counted in int32)
    assert 2 ** 31 - 1 < _sample_npt.NOISE_INDEX
    xi = _sample_npt.noise(7, keys, 99)
    atoms = _sample.noise(7, np.array([0, 1, 2 ** 31 - 1], dtype=np.uint64), keys[1], 99)
    assert xi.shape == (4, 6) and (np.abs(xi) < np.sqrt(3.0)).all()
    assert not np.isin(np.round((xi[1] / np.sqrt(12.0)), 12), np.round(atoms, 12)).any()
    # zero mean, unit variance, zero third moment over many steps
    big = np.concatenate([_sample_npt.noise(s, keys, 99).ravel() for s in range(2000)])
    assert abs(big.mean()) < 0.03 and abs(big.var() - 1.0) < 0.03 and abs((big ** 3).mean()) < 0.05
