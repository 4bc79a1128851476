"""Ghost images of any periodic cell -- triclinic, or smaller than the cutoff -- on the host side: the numpy twin of
mtp_ghosts_build_cell (driver.make_ghosts_cell / periodic_system_cell) fed to the CPU oracle, and the host arithmetic
of mtp_ghosts_cell_bounds through ctypes.  The physics checks need no second implementation: a cell and its replica
are the same crystal, and the virial is the strain derivative of the energy through regenerated images."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import make_ghosts, make_ghosts_cell, periodic_system
from oracle.pyoracle import Oracle

import _cells
from _cells import POT, LIST_CUTOFF


def _close(got, want, what, atol=1e-9, rtol=1e-10):
    """the bounds of tests/test_gpu_parity.py::_close"""
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print("%s: max abs err %.3e (scale %.3e)" % (what, err, scale))
    assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)


def _supercell_check(path, pos, cell, types, reps):
    orc = Oracle(path)
    e1, f1, v1, _, s1 = _cells.oracle_cell(orc, pos, cell, types)
    pos_n, cell_n, types_n = _cells.replicate(pos, cell, types, reps)
    en, fn, vn, _, sn = _cells.oracle_cell(orc, pos_n, cell_n, types_n)
    nrep = int(np.prod(reps))
    _close(en / nrep, e1, "energy per cell")
    _close(fn, np.tile(f1, (nrep, 1)), "forces per atom")
    _close(vn / nrep, v1, "virial per cell")
    return s1, sn


@pytest.mark.parametrize("fname", ["W_L8.mtp", "W_L16.mtp"])
def test_primitive_cell_equals_its_4x4x4_replica(fname):
    pos, cell, types = _cells.primitive_cell()
    s1, _ = _supercell_check(os.path.join(POT, fname), pos, cell, types, (4, 4, 4))
    # one atom under a 7 A list cutoff: 511 images, 88 neighbours, all of them the atom's own images
    assert s1.nall - 1 == 511 and s1.first[1] == 88 and (s1.owner == 0).all()


@pytest.mark.parametrize("fname", ["W_L8.mtp", "W_L16.mtp"])
def test_cubic_two_atom_cell_equals_its_4x4x4_replica(fname):
    pos, cell, types = _cells.cubic2_cell()
    s1, _ = _supercell_check(os.path.join(POT, fname), pos, cell, types, (4, 4, 4))
    # 3.165 A edge under a 7 A shell: 5 or 6 shifts per direction, and each atom among its own neighbours
    assert 2 * (5 ** 3 - 1) <= s1.nall - 2 <= 2 * (6 ** 3 - 1)
    assert np.abs(make_ghosts_cell(pos, cell, LIST_CUTOFF)[2]).max() >= 2
    assert 0 in s1.owner[s1.neigh[s1.first[0]:s1.first[1]]]


def test_tilted_two_species_cell_equals_its_3x2x2_replica():
    pos, cell, types = _cells.tilted5_cell()
    assert _cells.min_image_distance(pos, cell) > 2.4
    _supercell_check(os.path.join(POT, "WRe_L20.mtp"), pos, cell, types, (3, 2, 2))


@pytest.mark.parametrize("fname", ["W_L8.mtp", "W_L16.mtp"])
def test_small_cell_through_cell_images_equals_replica_through_box_images(fname):
    """the new twin against the existing orthogonal one-image construction: 2-atom cubic cell vs its 3x3x3 replica
    (edge 9.495 A >= 7 A) through driver.periodic_system"""
    orc = Oracle(os.path.join(POT, fname))
    pos, cell, types = _cells.cubic2_cell()
    e1, f1, v1, _, _ = _cells.oracle_cell(orc, pos, cell, types)
    pos_n, cell_n, types_n = _cells.replicate(pos, cell, types, (3, 3, 3))
    s = periodic_system(pos_n, np.diag(cell_n).copy(), types_n, LIST_CUTOFF)
    r = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(r["energy"] / 27, e1, "energy per cell")
    _close(s.fold_forces(r["f"]), np.tile(f1, (27, 1)), "forces per atom")
    _close(r["virial"] / 27, v1, "virial per cell")


@pytest.mark.parametrize("fname,species", [("W_L16.mtp", 1), ("WRe_L20.mtp", 2)])
def test_virial_is_the_strain_derivative_through_regenerated_images(fname, species):
    """dE/d(eps_ab) = -virial_ab (LAMMPS sign), all six components, with the cell and the positions strained together
    and the images REBUILT for every strained cell (tests/test_oracle.py strains the images of the unstrained cell)"""
    orc = Oracle(os.path.join(POT, fname))
    pos, cell, types = _cells.tilted5_cell(species)
    _, _, v0, _, _ = _cells.oracle_cell(orc, pos, cell, types)

    def energy(eps):
        d = (np.eye(3) + eps).T
        return _cells.oracle_cell(orc, pos @ d, cell @ d, types)[0]

    h = 1e-6
    for (a, b), v in [((0, 0), 0), ((1, 1), 1), ((2, 2), 2), ((0, 1), 3), ((0, 2), 4), ((1, 2), 5)]:
        e = np.zeros((3, 3))
        e[a, b] = e[b, a] = h
        # symmetric strain: for a != b both eps_ab and eps_ba are switched on, dE = -2 v_ab h
        dE = (energy(e) - energy(-e)) / (2 * h)
        want = -v0[v] * (2.0 if a != b else 1.0)
        print("strain %d%d: dE/deps %.9e  -virial %.9e  rel %.2e" % (a, b, dE, want, abs(dE - want) / max(1.0, abs(dE))))
        assert abs(dE - want) < 1e-6 * max(1.0, abs(dE)), ((a, b), dE, want)


def test_diagonal_cell_gives_the_images_of_the_orthogonal_construction():
    pos, box = mtpgen.bcc_lattice(4, 4, 4)
    rng = np.random.default_rng(3)
    pos = pos + rng.normal(0, 0.3, pos.shape) + np.array([40.0, -13.0, 0.2]) * (rng.random((len(pos), 1)) < 0.1)
    n = len(pos)
    assert (box >= LIST_CUTOFF).all()
    wrapped = pos - np.floor(pos / box) * box
    want_x, want_owner = make_ghosts(wrapped, box, LIST_CUTOFF)
    x, owner, shift = make_ghosts_cell(pos, np.diag(box), LIST_CUTOFF)
    assert len(x) == len(want_x) and np.abs(x[:n] - wrapped).max() < 1e-12
    key = lambda o, p: np.lexsort((np.round(p[:, 2], 9), np.round(p[:, 1], 9), np.round(p[:, 0], 9), o))
    k0, k1 = key(owner, x), key(want_owner, want_x)
    assert np.array_equal(owner[k0], want_owner[k1]) and np.abs(x[k0] - want_x[k1]).max() < 1e-12
    assert np.abs(shift).max() == 1


def test_ghost_order_is_atom_then_lexicographic_shift():
    pos, cell, _ = _cells.tilted5_cell()
    x, owner, shift = make_ghosts_cell(pos, cell, LIST_CUTOFF)
    n = len(pos)
    assert np.array_equal(owner[:n], np.arange(n)) and not shift[:n].any() and shift[n:].any(1).all()
    rows = np.column_stack([owner[n:], shift[n:]])
    assert np.array_equal(rows, rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))])
    assert len(np.unique(rows, axis=0)) == len(rows)
    assert np.abs(x - (x[owner] - shift @ cell)[owner] - shift @ cell).max() < 1e-12     # image = owner + n . cell
    # the criterion itself: fractional coordinates of every image inside the slab, of every left-out image outside
    hinv = np.linalg.inv(cell)
    d = np.array([np.linalg.det(cell) / np.linalg.norm(np.cross(cell[(a + 1) % 3], cell[(a + 2) % 3])) for a in range(3)])
    m = LIST_CUTOFF / d
    t = x[n:] @ hinv
    assert (t >= -m - 1e-12).all() and (t < 1 + m + 1e-12).all()
    nim = int(np.ceil(m).max()) + 1
    r = np.arange(-nim, nim + 1)
    allsh = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    s = x[:n] @ hinv
    inside = sum(int((np.all((s[i] + allsh >= -m) & (s[i] + allsh < 1 + m), axis=1)).sum()) - 1 for i in range(n))
    assert inside == len(x) - n


@pytest.mark.parametrize("which", ["primitive", "cubic2", "tilted5", "sheared"])
def test_cell_bounds_contain_every_image_and_report_the_volume(which):
    if which == "sheared":
        cell = _cells.SHEARED.copy()
        pos = np.random.default_rng(4).random((40, 3)) @ cell
    else:
        pos, cell, _ = getattr(_cells, which + "_cell")()
    b = capi.ghosts_cell_bounds(cell, LIST_CUTOFF)
    x, _, shift = make_ghosts_cell(pos, cell, LIST_CUTOFF)
    assert (x >= b["lo"]).all() and (x <= b["hi"]).all()
    assert abs(b["volume"] - abs(np.linalg.det(cell))) <= 1e-12 * abs(np.linalg.det(cell))
    assert (np.abs(shift).max(0) <= b["nimage"]).all()
    # not loose either: the corners of the slab [-m, 1 + m]^3 are reached to within the widening
    far = np.random.default_rng(5).random((4000, 3)) @ cell
    xf, _, _ = make_ghosts_cell(far, cell, LIST_CUTOFF)
    ext = b["hi"] - b["lo"]
    assert ((xf.min(0) - b["lo"]) < 0.25 * ext).all() and ((b["hi"] - xf.max(0)) < 0.25 * ext).all()


def test_cell_bounds_refuse_what_is_not_a_cell():
    for bad in (np.zeros((3, 3)), np.diag([1.0, 1.0, -1.0]) * 5, np.array([[5.0, 0, 0], [0, 5.0, 0], [5.0, 5.0, 0]]),
                np.diag([5.0, np.nan, 5.0]), np.diag([5.0, np.inf, 5.0])):
        with pytest.raises(capi.MtpError) as ei:
            capi.ghosts_cell_bounds(bad, LIST_CUTOFF)
        assert ei.value.code == -20
    with pytest.raises(capi.MtpError):
        capi.ghosts_cell_bounds(np.eye(3) * 5, 0.0)
    with pytest.raises(ValueError):
        make_ghosts_cell(np.zeros((1, 3)), np.diag([1.0, 1.0, -1.0]), LIST_CUTOFF)
