"""The host side of the batched nudged elastic band (md.neb_cells; include/mtp_mi355x.h, "batched nudged elastic band"), no
device needed: the numpy twin of mtp_neb_step (tests/_neb.py) finds the saddle of an analytic double well, interpolate_band
across a periodic boundary, the refusals neb_cells makes before anything touches the device, and plan_band_passes."""
import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi
from lammps_mtp_kokkos_amd.md import interpolate_band, neb_cells, plan_band_passes, plan_cell_passes

import _cells
import _neb

FTOL = 1e-3


def _saddle_band(n, A, G, seed=5):
    """one band of 7 images in which all n atoms hop together from their minima at ux = -1 to a point NEAR those at ux = 1 (the
    far end is displaced: a symmetric band has equal energies left and right of its top image, a tie the margins refuse), the
    interior images interpolated"""
    S = _neb.surface_bands([(7, n)], seed=seed, A=A, G=G, noise=0.0, end_noise=0.0, hopping=None)
    org, cell = S["origins"], S["cells"][0]
    last = S["x0"][-n:] - org[-1] + np.array([-0.12, 0.05, 0.03])
    images = interpolate_band(S["x0"][:n] - org[0], last, cell, 7)
    S["x0"] = np.concatenate([p + o for p, o in zip(images, org)])
    return S


@pytest.mark.parametrize("n,A,G", [(1, (0.5, 0.5), 0.0), (3, (0.45, 0.55), 2.5)], ids=["one-atom", "three-coupled"])
def test_the_twin_finds_the_saddle_of_the_double_well(n, A, G):
    """per atom A_j (x^2 - 1)^2 + B (y - C (1 - x^2))^2 + D z^2 with B = 2, C = 0.6, D = 1.5, 7 images, spring 5, the climbing
    image from step 30, ftol 1e-3: the saddle is u_j = (0, C, 0) for every atom, the barrier sum A_j.  Three atoms are coupled by
    G (x_j - x_j+1)^2 with G = 2.5, stiff enough that the Hessian at the saddle keeps ONE negative eigenvalue (asserted) and the
    atoms hop together.  |F_neb| of the climbing image is |F|, so at convergence every atom of it has |grad| <= ftol and the
    image lies within sqrt(n) ftol / min |eigenvalue| of the saddle in the harmonic picture; the bound is 2 ftol / min |eigenvalue|
    per atom (n <= 3: sqrt(n) < 2), and 1/2 max |eigenvalue| n times its square for the energy."""
    S = _saddle_band(n, A, G)
    twin, x, v, _ = _neb.run_surface(S, 400, ftol=FTOL, spring=5.0, climb_step=30)
    print("status", twin.status, "step", twin.done_step, "margins", twin.margins(), "uphill", twin.uphill, "energies", twin.energy)
    twin.assert_margins()
    assert twin.status[0] == _neb.CONVERGED and 30 < twin.done_step[0] < 400 and twin.fmax[0] <= FTOL
    assert (twin.frozen == _neb.CONVERGED).all() and twin.count == 7 and not v.any()
    eig = np.linalg.eigvalsh(_neb.saddle_hessian(S["A"][:n], S["B"][:n], S["C"][:n], S["D"][:n], S["G"][:n]))
    assert (eig < 0.0).sum() == 1
    tol = 2.0 * FTOL / np.abs(eig).min()
    c = int(twin.climber[0])
    assert c == int(np.argmax(twin.energy)) and 0 < c < 6
    r0 = int(S["cfg_first"][c])
    u = (x - S["site"])[r0: r0 + n]
    dev = float(np.sqrt(((u - np.array([0.0, 0.6, 0.0])) ** 2).sum(1)).max())
    barrier = float(S["A"][:n].sum())
    print("climber %d: %.3e A from the saddle (bound %.3e), E %.9f against the barrier %.9f" % (c, dev, tol, twin.energy[c], barrier))
    assert dev <= tol
    assert abs(twin.energy[c] - barrier) <= 0.5 * np.abs(eig).max() * n * tol * tol
    assert twin.energy[0] == 0.0                              # (the first image sits in its minima and was never moved)
    assert np.array_equal(x[:n], S["x0"][:n]) and np.array_equal(x[-n:], S["x0"][-n:])


def test_the_tangent_rule_case_by_case():
    """the improved tangent: D+ on a rising slope, D- on a falling one, the energy-weighted mix at an extremum"""
    assert _neb.tangent_weights(0.0, 1.0, 2.0) == (1.0, 0.0) and _neb.tangent_weights(2.0, 1.0, 0.0) == (0.0, 1.0)
    assert _neb.tangent_weights(0.0, 3.0, 1.0) == (3.0, 2.0)          # a maximum, the right neighbour the higher one: the big weight on D+
    assert _neb.tangent_weights(1.0, 3.0, 0.0) == (2.0, 3.0)          # the left one higher: the big weight on D-
    assert _neb.tangent_weights(5.0, 1.0, 2.0) == (1.0, 4.0)          # a minimum, the left neighbour higher
    got = []
    _neb.tangent_weights(1.0, 1.0 + 1e-9, 0.5, got)
    assert min(got) < 1e-6                                            # a near tie is recorded
    cell = _neb.TRICLINIC
    d = np.array([[0.3, -0.2, 0.1]])
    shifted = d + np.array([[2.0, -1.0, 3.0]]) @ cell
    assert np.abs(_neb.mic(shifted, cell, np.linalg.inv(cell)) - d).max() < 1e-13


def test_interpolate_band_takes_the_short_way_across_a_periodic_boundary():
    cell = _cells.TILTED
    inv = np.linalg.inv(cell)
    a = np.array([[0.95, 0.50, 0.50], [0.20, 0.05, 0.40], [0.50, 0.50, 0.97]]) @ cell
    b = np.array([[0.05, 0.52, 0.50], [0.22, 0.93, 0.40], [0.50, 0.48, 0.03]]) @ cell
    images = interpolate_band(a, b, cell, 6)
    assert len(images) == 6 and np.array_equal(images[0], a)
    short = _neb.mic(b - a, cell, inv)
    assert (np.sqrt((short ** 2).sum(1)) < np.sqrt(((b - a) ** 2).sum(1))).all()      # every atom crosses a boundary
    for i in range(5):
        assert np.abs(images[i + 1] - images[i] - short / 5.0).max() < 1e-13
    lattice = (images[-1] - b) @ inv
    assert np.abs(lattice - np.rint(lattice)).max() < 1e-13 and np.abs(np.rint(lattice)).sum() == 3
    frac = (images[3] @ inv)[0, 0]
    assert frac > 1.0                                                 # (continuous: not wrapped back into the cell)
    with pytest.raises(ValueError):
        interpolate_band(a, b[:2], cell, 6)
    with pytest.raises(ValueError):
        interpolate_band(a, b, cell, 1)


def _band(nimages=5, natoms=5, shift=0.1):
    pos, cell, types = _cells.tilted5_cell()
    pos, types = pos[:natoms], types[:natoms]
    return interpolate_band(pos, pos + shift, cell, nimages), cell, types


def test_neb_cells_refuses_bad_bands_before_it_touches_the_device():
    """ctx = None: anything past the host checks would fail on it with another error"""
    good = _band()
    cases = {
        "two images": dict(bands=[(good[0][:2], good[1], good[2])]),
        "65 images": dict(bands=[_band(65, shift=1.0)]),
        "differing atom counts": dict(bands=[(good[0][:2] + [good[0][2][:4]] + good[0][3:], good[1], good[2])]),
        "no atoms": dict(bands=[([np.zeros((0, 3))] * 3, good[1], np.zeros(0, dtype=np.int32))]),
        "spring 0": dict(bands=[good], spring=0.0),
        "spring < 0": dict(bands=[good], spring=-5.0),
        "spring nan": dict(bands=[good], spring=float("nan")),
        "spring inf": dict(bands=[good], spring=float("inf")),
        "climb_after < 0": dict(bands=[good], climb_after=-1),
        "a degenerate cell": dict(bands=[(good[0], np.zeros((3, 3)), good[2])]),
        "ftol < 0": dict(bands=[good], ftol=-1.0),
        "steps < 0": dict(bands=[good], steps=-1),
    }
    # neighbouring images further apart than a quarter of the smallest cell height (the second band: the error names it)
    cell = good[1]
    height = min(abs(np.linalg.det(cell)) / np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3])) for a in range(3))
    far = _band(3, shift=np.array([0.51 * height, 0.0, 0.0]))         # 0.255 of the height between neighbours
    near = _band(3, shift=np.array([0.49 * height, 0.0, 0.0]))
    cases["a jump of more than a quarter of the cell height"] = dict(bands=[good, far])
    for what, kw in cases.items():
        kw = dict(dict(steps=5), **kw)
        with pytest.raises(ValueError) as ei:
            neb_cells(None, **kw)
        print(what, "->", ei.value)
        assert "neb_cells" in str(ei.value), what
    assert "band 1" in str(ei.value)
    with pytest.raises(AttributeError):                               # just inside the bound: past the host checks
        neb_cells(None, [good, near], 5)
    # the jump is measured after minimum image: an image shifted by lattice vectors is as near as before
    images = [p.copy() for p in near[0]]
    images[1][2] += cell[0] - 2.0 * cell[2]
    with pytest.raises(AttributeError):
        neb_cells(None, [(images, near[1], near[2])], 5)


def _cells_of(bands):
    cells = np.array([b[1] for b in bands for _ in b[0]])
    natoms = np.array([len(p) for b in bands for p in b[0]])
    band_first = np.concatenate([[0], np.cumsum([len(b[0]) for b in bands])])
    return cells, natoms, band_first


def test_plan_band_passes_never_splits_a_band():
    bands = [_band(3, 4), _band(4, 5), _band(3, 2), _band(9, 1), _band(5, 3)]
    cells, natoms, band_first = _cells_of(bands)
    whole = plan_band_passes(cells, natoms, band_first, 7.0)
    assert [(a, b) for a, b, _ in whole[0]] == [(0, len(cells))]
    assert np.array_equal(whole[1], plan_cell_passes(cells, natoms, 7.0)[1])
    moved = 0
    for cap in (1, 2, 7, 10, 12, 13, 20, 21, 33, 40, 100):
        plain = [(a, b) for a, b, _ in plan_cell_passes(cells, natoms, 7.0, cap)[0]]
        got = plan_band_passes(cells, natoms, band_first, 7.0, cap)[0]
        spans = [(a, b) for a, b, _ in got]
        print("max_atoms_per_pass %d: %r (configurations alone: %r)" % (cap, spans, plain))
        assert spans[0][0] == 0 and spans[-1][1] == len(cells)
        assert all(a1 == b0 for (_, b0), (a1, _) in zip(spans, spans[1:])) and all(b > a for a, b in spans)
        assert all(a in band_first and b in band_first for a, b in spans)
        # a boundary inside a band went to the band's start, the others stayed
        want = sorted({int(band_first[np.searchsorted(band_first, a, side="right") - 1]) for a, _ in plain})
        assert [a for a, _ in spans] == want
        moved += sum(a not in band_first for a, _ in plain)
        for a, b, lay in got:
            assert lay["origins"].shape == (b - a, 3)
    assert moved > 0
    assert [(a, b) for a, b, _ in plan_band_passes(cells, natoms, band_first, 7.0, 1)[0]] == list(zip(band_first[:-1], band_first[1:]))


def test_a_band_that_does_not_fit_a_pass_alone_is_named():
    """cells of 2100 A: one fits the layout's 2048 A on each side of the origin, the three images of a band do not"""
    big = ([np.full((1, 3), 5.0) + 0.1 * i for i in range(3)], 2100.0 * np.eye(3), np.ones(1, dtype=np.int32))
    bands = [_band(3, 2), big, _band(3, 2)]
    cells, natoms, band_first = _cells_of(bands)
    assert len(plan_cell_passes(cells, natoms, 7.0)[0]) > 1            # (configurations alone would be split)
    with pytest.raises(capi.MtpError) as ei:
        plan_band_passes(cells, natoms, band_first, 7.0)
    print(ei.value)
    assert ei.value.code == -24 and "band 1 " in str(ei.value) and "configurations 3 to 5" in str(ei.value)
