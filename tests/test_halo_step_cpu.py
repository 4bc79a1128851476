"""The host side of tests/test_halo_step_gpu.py: every geometry of tests/_halo_step.py sits on the edge it was picked for,
the library's layout check accepts each plan, and the numpy model of the step -- the reference of the GPU tests -- gives
what the single-box route (periodic_system, oracle, fold_forces) gives."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi
from lammps_mtp_kokkos_amd.driver import periodic_system
from oracle.pyoracle import Oracle

import _halo_step as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")


@pytest.mark.parametrize("name", sorted(hs.FACTS))
def test_geometry_sits_on_its_edge(name):
    p = hs.plan(name)
    nlocal, nghost, n3, half, split, most = hs.FACTS[name]
    assert (p.nlocal, p.nghost) == (nlocal, nghost)
    assert p.send_counts == [nghost] and p.recv_counts == [nghost] and len(p.send_idx) == nghost
    assert hs.launch_sizes(p) == (n3, half)
    assert p.nall % 2 == (0 if "even" in name else 1)
    if name.startswith("pack") or name == "bcc8_cut7":
        assert n3 > half                       # the pack sizes halo_pack_zero_kernel's launch
    else:
        assert n3 < half                       # the zeroing does: threads past 3 nsend only clear f
        assert (n3 + 255) // 256 < (half + 255) // 256     # ... and a grid from 3 nsend alone would be a block short
    ilist, first, neigh, got_split = hs.natural_order(p)
    assert got_split == split and sum(got_split) == nlocal
    assert sorted(ilist.tolist()) == list(range(nlocal))
    if most is not None:
        assert hs.images(p).max() == most
    if split[0] == 0:
        assert hs.images(p).min() >= 1          # every owned atom is a ghost somewhere: no interior rows at all


def test_two_species_plan_carries_ghost_types():
    p = hs.plan("pack_even_two_species")
    assert set(np.unique(p.types)) == {1, 2}
    assert np.array_equal(p.types[p.nlocal:], p.types[: p.nlocal][p.send_idx])
    assert len(set(p.types[p.nlocal:].tolist())) == 2


def test_hand_made_splits_keep_boundary_rows_in_the_middle():
    p = hs.plan("pack_odd_split")
    for kind, want in (("empty_first", (0, 241, 9)), ("empty_last", (9, 241, 0))):
        ilist, first, neigh, split = hs.hand_order(p, kind)
        assert split == want and sorted(ilist.tolist()) == list(range(p.nlocal))
        na, nb, nc = split
        ghost_in_row = np.array([(neigh[first[r]:first[r + 1]] >= p.nlocal).any() for r in range(p.nlocal)])
        assert not ghost_in_row[:na].any() and not ghost_in_row[na + nb:].any() and ghost_in_row[na:na + nb].all()
        for r in (0, p.nlocal - 1):             # the rows moved with their atoms
            i = ilist[r]
            assert np.array_equal(neigh[first[r]:first[r + 1]], p.neigh[p.first[i]:p.first[i + 1]])
    for name in hs.CLUSTERS:
        c = hs.plan(name)
        ilist, first, neigh, split = hs.hand_order(c, "empty_middle")
        assert split[1] == 0 and split[0] > 0 and split[2] > 0 and sum(split) == c.nlocal


def test_clusters_have_no_ghosts_and_both_parities():
    even, odd = (hs.plan(n) for n in hs.CLUSTERS)
    assert (even.nlocal, odd.nlocal) == (54, 53) and even.nghost == odd.nghost == 0
    assert (3 * even.nall) % 2 == 0 and (3 * odd.nall) % 2 == 1
    for c in (even, odd):
        assert hs.launch_sizes(c)[0] == 0 and len(c.send_idx) == 0 and c.send_counts == c.recv_counts == [0]
        assert c.neigh.max() < c.nlocal and np.diff(c.first).min() > 0


@pytest.mark.parametrize("name", sorted(hs.FACTS) + list(hs.CLUSTERS))
def test_layout_accepts_the_plan(name):
    p = hs.plan(name)
    so, ro = capi.halo_layout(p)
    assert so.tolist() == [0, p.nghost] and ro.tolist() == [0, p.nghost]     # the clusters: [0, 0]


def test_model_of_the_step_is_the_single_box_calculation():
    """forward gather + shift, oracle on x_all, np.add.at of the ghost rows == periodic_system + oracle + fold_forces:
    the reference side of the GPU tests is right before a GPU is involved."""
    p = hs.plan("pack_odd_tiny")
    path = os.path.join(POT, "W_L8.mtp")
    orc = Oracle(path)
    x_own = hs.positions(p)
    got = hs.model_step(orc, p, x_own)
    s = periodic_system(x_own, p.box, None, 7.0)
    want = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=1)
    F = s.fold_forces(want["f"])
    scale = max(1.0, np.abs(F).max())
    err = np.abs(got["f"] - F).max()
    print("model vs single box: forces %.3e (scale %.3e)" % (err, scale))
    assert err <= 1e-9 + 1e-10 * scale
    assert abs(got["energy"] - want["energy"]) <= 1e-10 * p.nlocal * max(1.0, abs(want["energy"]) / p.nlocal)
    assert np.abs(got["virial"] - want["virial"]).max() <= 1e-8 + 1e-10 * np.abs(want["virial"]).max()
    assert np.abs(got["eatom"][: p.nlocal] - want["eatom"][: p.nlocal]).max() <= 1e-10
    assert np.abs(F).max() > 1e-3               # the jitter makes the forces worth comparing


def test_unpack_bound_covers_a_reordered_sum():
    """the derived bound of the 26-image fold holds between two host orders of the same additions"""
    p = hs.plan("pack_odd_tiny")
    f = np.random.default_rng(4).normal(size=(p.nall, 3))
    a = hs.fold(p, f)
    b = f[: p.nlocal].copy()
    np.add.at(b, p.send_idx[::-1], f[p.nlocal:][::-1])
    assert (np.abs(a - b) <= hs.unpack_bound(p, f)).all() and np.abs(a - b).max() > 0
