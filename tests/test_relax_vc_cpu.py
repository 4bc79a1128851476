"""The batched variable-cell minimiser without a GPU: the analytic model of tests/_relax_vc.py against central differences,
the numpy twin of mtp_relax_cell_step on that model (convergence with and without pressure, the isotropic and the masked
cell), the rebuild rule on hand-made numbers, the argument errors of md.relax_cells_vc, and the twin driven by the CPU oracle
on the 2-atom bcc cell the GPU convergence test uses."""
import os

import numpy as np
import pytest

import _cells
import _relax_vc
from _relax_vc import GPA, Model, det3, sym


def _small(seed=5, **kw):
    return Model(sizes=[2, 5, 0, 3], k_cfg=(2.0, 5.0, 9.0, 3.0), seed=seed, **kw)


def test_the_model_forces_and_virial_are_the_derivatives_of_its_energy():
    """central differences, delta = 1e-5: the truncation error is delta^2 times a third derivative, rounding 1e-16 E / delta ->
    1e-8 relative is ten times both for energies of order 1 to 10 eV"""
    m = _small()
    rng = np.random.default_rng(2)
    delta = 1e-5
    for k in (0, 1, 3):
        a0, a1 = int(m.cf[k]), int(m.cf[k + 1])
        h = m.h0[k] @ (np.eye(3) + rng.normal(0.0, 0.02, (3, 3)))
        x = m.x0[a0:a1] + rng.normal(0.0, 0.05, (a1 - a0, 3))
        e, f, w6 = m.one(k, x, h)
        fd = np.zeros_like(f)
        for i in range(a1 - a0):
            for c in range(3):
                xp, xm = x.copy(), x.copy()
                xp[i, c] += delta
                xm[i, c] -= delta
                fd[i, c] = -(m.one(k, xp, h)[0] - m.one(k, xm, h)[0]) / (2 * delta)
        wd = np.zeros((3, 3))
        for a in range(3):
            for b in range(3):
                eps = np.zeros((3, 3))
                eps[a, b] = delta
                wd[a, b] = -(m.one(k, x @ (np.eye(3) + eps), h @ (np.eye(3) + eps))[0]
                             - m.one(k, x @ (np.eye(3) - eps), h @ (np.eye(3) - eps))[0]) / (2 * delta)
        ef, ew = np.abs(f - fd).max() / np.abs(f).max(), np.abs(sym(w6) - wd).max() / np.abs(wd).max()
        print("configuration %d: E %.6f, f against differences %.3e, W %.3e relative; W asymmetry %.3e" % (k, e, ef, ew, np.abs(wd - wd.T).max()))
        assert ef < 1e-8 and ew < 1e-8


@pytest.mark.parametrize("pressure", [0.0, 5.0 * GPA])
def test_the_twin_converges_on_the_model(pressure):
    m = _small()
    stol = 1e-5
    twin, x, xt, vt, _ = _relax_vc.run_model(m, 3000, pressure=pressure, stol=stol, ftol=1e-4)
    print("done at", twin.done_step, "uphill", twin.uphill, "capped", twin.capped, "margins", twin.margins())
    live = np.diff(m.cf) > 0
    assert (twin.frozen[live] == _relax_vc.CONVERGED).all() and (twin.frozen[~live] == 0).all()
    assert twin.uphill >= 1
    _, f, W = m.all(x, twin.h)
    free = _relax_vc.run_model(m, 3000, pressure=0.0, stol=stol, ftol=1e-4)[0] if pressure else None
    for k in np.nonzero(live)[0]:
        V = det3(twin.h[k])
        s = sym(W[k]) / V
        print("configuration %d: V %.6f W/V" % (k, V), _relax_vc.voigt(s))
        assert np.abs(s - pressure * np.eye(3)).max() <= stol
        assert np.sqrt((f[m.cf[k]:m.cf[k + 1]] ** 2).sum(1)).max() <= 1e-4
        assert np.allclose(x[m.cf[k]:m.cf[k + 1]], xt[m.cf[k]:m.cf[k + 1]] @ twin.D[k], rtol=0, atol=1e-13)
        if pressure:
            assert V < det3(free.h[k])                           # under pressure the volume is smaller


def test_an_isotropic_cell_keeps_its_shape_to_the_bit():
    m = _small()
    twin, *_ = _relax_vc.run_model(m, 200, isotropic=True, pressure=2.0 * GPA)
    for k in (0, 1, 3):
        D = twin.D[k]
        off = D[~np.eye(3, dtype=bool)]
        print("configuration %d: D diagonal %r" % (k, D[0, 0]))
        assert (off == 0.0).all() and D[0, 0] == D[1, 1] == D[2, 2] and D[0, 0] != 1.0
        assert (twin.vq[k][~np.eye(3, dtype=bool)] == 0.0).all()


def test_with_the_shear_mask_off_the_cell_is_not_sheared():
    m = _small()
    twin, *_ = _relax_vc.run_model(m, 200, cell_mask=(1, 1, 1, 0, 0, 0))
    for k in (0, 1, 3):
        D = twin.D[k]
        assert (D[~np.eye(3, dtype=bool)] == 0.0).all() and len({D[0, 0], D[1, 1], D[2, 2], 1.0}) == 4
    fixed, x, xt, *_ = _relax_vc.run_model(m, 50, cell_mask=(0, 0, 0, 0, 0, 0))
    assert np.array_equal(fixed.D, np.tile(np.eye(3), (4, 1, 1))) and np.array_equal(x, xt) and (fixed.smax == 0.0).all()


def test_the_rebuild_rule_on_hand_made_numbers():
    from lammps_mtp_kokkos_amd.md import cell_list_stale
    skin = 2.0
    cases = [(([0.0, 0.99 ** 2], [0.0, 0.0]), False),            # cellmove = 0: the half-skin test
             (([0.0, 1.01 ** 2], [0.0, 0.0]), True),
             (([0.25, 0.0], [0.99, 1.9]), False),                 # 2 * 0.5 + 0.99 and 0 + 1.9
             (([0.25, 0.0], [1.01, 0.0]), True),
             (([0.0, 0.0], [0.0, 2.01]), True),
             (([], []), False)]
    for (d2, cm), want in cases:
        assert cell_list_stale(d2, cm, skin) is want, (d2, cm)
        assert _relax_vc.needs_rebuild(d2, cm, skin) is want, (d2, cm)
    # the measure itself: (nimg_a + 1) |h_a - href_a| summed over the rows
    href = np.diag([3.0, 4.0, 5.0])
    h = href + np.array([[0.3, 0.4, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, -0.1]])
    assert abs(_relax_vc.cell_move(h, href, [3, 2, 2]) - (4 * 0.5 + 3 * 0.1)) < 1e-15
    assert list(_relax_vc.images(href, 7.0)) == [3, 2, 2]


def test_the_image_counts_of_a_rebuild_are_those_of_the_ghost_build():
    """md._cell_images (all cells of a pass at once) against mtp_ghosts_cell_bounds, cell by cell"""
    import _batch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import _cell_images
    rng = np.random.default_rng(1)
    cells = [c[1] for c in _batch.mixed_batch()] + [c @ (np.eye(3) + rng.normal(0.0, 0.05, (3, 3))) for c in [_cells.TILTED, _cells.SHEARED, _cells.PRIMITIVE] * 5]
    for cut in (7.0, 5.0, 12.3):
        want = np.array([capi.ghosts_cell_bounds(c, cut)["nimage"] for c in cells])
        assert np.array_equal(_cell_images(cells, cut), want) and np.array_equal([_relax_vc.images(c, cut) for c in cells], want)


def test_argument_errors_of_relax_cells_vc_are_raised_before_the_device_is_touched():
    from lammps_mtp_kokkos_amd.md import relax_cells_vc
    batch = [_cells.cubic2_cell()]
    nan, inf = float("nan"), float("inf")
    bad = [dict(stol=-1e-9), dict(stol=nan), dict(pressure=inf), dict(pressure=nan), dict(cell_factor=0.0), dict(cell_factor=-1.0),
           dict(cell_factor=inf), dict(cell_mass=0.0), dict(cell_mass=nan), dict(cell_mask=(1, 1, 1)), dict(cell_mask=(1, 1, 1, 2, 0, 0)),
           dict(cell_mask=(1, 1, 1, 0.5, 0, 0)), dict(cell_mask=1),
           # those of relax_cells
           dict(steps=-1), dict(ftol=-1.0), dict(dt=0.0), dict(dt_max=inf), dict(dmax=0.0), dict(f_inc=0.5), dict(f_dec=1.0),
           dict(alpha_start=2.0), dict(f_alpha=0.0), dict(n_min=-1), dict(masses=-1.0), dict(every=0), dict(max_candidates=-1),
           dict(threshold_select=5.0, threshold_break=1.0)]
    for kw in bad:
        args = dict(steps=3)
        args.update(kw)
        with pytest.raises(ValueError) as ei:                    # ctx = None: anything that touched it would not be a ValueError
            relax_cells_vc(None, batch, **args)
        assert "relax_cells_vc" in str(ei.value), kw


# ---- the oracle-driven twin on the cell of the GPU convergence test ----------------------------------------------------

BCC_START = 3.482


def bcc2(a=BCC_START):
    return np.array([[0.0, 0.0, 0.0], [0.5 * a, 0.5 * a, 0.5 * a]]), a * np.eye(3), np.ones(2, dtype=np.int32)


def oracle_evaluate(fname):
    from oracle.pyoracle import Oracle
    orc = Oracle(os.path.join(_cells.POT, fname))

    def evaluate(configs, graded):
        out = []
        for pos, cell, types in configs:
            e, f, w, _, _ = _cells.oracle_cell(orc, np.asarray(pos), np.asarray(cell), np.asarray(types, dtype=np.int32))
            out.append(dict(energy=e, f=f, virial=np.asarray(w)))
        return out
    return evaluate


@pytest.mark.parametrize("isotropic", [True, False])
def test_the_oracle_driven_twin_converges_in_the_well_of_the_level_16_potential(isotropic):
    """the perfect 2-atom bcc cell from a = 3.482 A: the forces vanish by symmetry, the cell relaxes to the minimum of E(a) near
    3.576 A; under 10 GPa to a smaller one with W / V = p I"""
    ev = oracle_evaluate("W_L16.mtp")
    kw = dict(isotropic=isotropic, stol=1e-5)
    ref = _relax_vc.reference_loop(ev, [bcc2()], 400, **kw)
    ref["twin"].assert_margins()
    a = np.sqrt((ref["final_cell"][0] ** 2).sum(1))
    print("isotropic %s: converged at step %d, a = %r, E = %.6f, margins %s" % (isotropic, ref["done_step"][0], a, ref["energy"][-1, 0], ref["twin"].margins()))
    assert ref["status"][0] == _relax_vc.CONVERGED and 0 < ref["done_step"][0] < 400
    assert np.abs(a - 3.576).max() < 5e-3 and abs(ref["energy"][-1, 0] + 37.5) < 0.1
    p = 10.0 * GPA
    pr = _relax_vc.reference_loop(ev, [bcc2()], 400, pressure=p, **kw)
    pr["twin"].assert_margins()
    V = pr["volume"][-1, 0]
    print("10 GPa: converged at step %d, V %.6f against %.6f, W/V" % (pr["done_step"][0], V, ref["volume"][-1, 0]), pr["virial"][0] / V)
    assert pr["status"][0] == _relax_vc.CONVERGED and V < ref["volume"][-1, 0]
    assert np.abs(sym(pr["virial"][0]) / V - p * np.eye(3)).max() <= 1e-5
