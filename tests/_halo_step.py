"""Geometries, plan helpers and a numpy model of the decomposed force step (mtp_halo_force_step, csrc/mtp_halo.hip).

Every geometry is a single-rank plan whose only peer is the rank itself, picked so that one edge of the step's two fused
kernels is on the far side of what tests/test_gpu_halo.py runs (8x8x8 cells, 7 A list: odd nall, the pack sizes the
launch, a three-way split, at most 7 images of an owner):

  halo_pack_zero_kernel    the grid is max(3 nsend, (3 nall + 1) / 2) threads: which of the two sizes it, and whether
                           3 nall is even (no odd last element) or odd
  mtp_ev_finish_unpack     how many ghost rows are added onto one owner (boxes below twice the list cutoff: 26 images),
                           n3 = 0 (a rank without ghosts), fold = 0
  the overlapped schedule  rows_a = rows_c = 0 (every owned atom has a ghost in its row), an empty first, middle or last
                           launch

FACTS pins what domain.decompose gives for each of them; tests/test_halo_step_cpu.py asserts the table, so a change in
decompose cannot silently move a case off its edge."""
import functools

import numpy as np

from lammps_mtp_kokkos_amd import mtpgen
from lammps_mtp_kokkos_amd.domain import HaloPlan, decompose, overlap_order, split_interior, sub_list
from lammps_mtp_kokkos_amd.driver import full_neighbor_list

# name: cells, list cutoff, species
GEOMETRIES = {
    "pack_odd_tiny": ((4, 4, 4), 7.0, 1),
    "pack_even_tiny": ((4, 4, 5), 7.0, 1),
    "pack_even_two_species": ((3, 4, 5), 6.0, 2),
    "pack_odd_split": ((5, 5, 5), 5.5, 1),
    "zero_odd": ((14, 14, 14), 5.5, 1),
    "zero_even": ((14, 14, 15), 5.5, 1),
    "bcc8_cut7": ((8, 8, 8), 7.0, 1),          # the geometry of tests/test_gpu_halo.py
}
# name: nlocal, nghost, 3 nsend, (3 nall + 1) / 2, split of overlap_order, most images of one owner (26 = all of 3^3 - 1:
# only the box with every edge below twice the list cutoff; one longer edge leaves 17, a 6 A list 11)
FACTS = {
    "pack_odd_tiny": (128, 1113, 3339, 1862, (0, 128, 0), 26),
    "pack_even_tiny": (160, 1226, 3678, 2079, (0, 160, 0), 17),
    "pack_even_two_species": (120, 720, 2160, 1260, (0, 120, 0), 11),
    "pack_odd_split": (250, 991, 2973, 1862, (4, 242, 4), 7),
    "zero_odd": (5488, 5257, 15771, 16118, (1182, 3124, 1182), 7),
    "zero_even": (5880, 5478, 16434, 17037, (1293, 3294, 1293), 7),
    "bcc8_cut7": (1024, 2901, 8703, 5888, (63, 898, 63), 7),
}
CLUSTER_CUT = 5.5
CLUSTERS = ("no_ghosts_even", "no_ghosts_odd")   # 3 nlocal = 162 / 159


@functools.lru_cache(maxsize=None)
def plan(name):
    """The HaloPlan of a geometry (cached: treat it as read-only)."""
    if name in CLUSTERS:
        return cluster_plan(drop=name.endswith("odd"))
    cells, cut, species = GEOMETRIES[name]
    pos, box = mtpgen.bcc_lattice(*cells)
    types = None
    if species > 1:
        types = np.random.default_rng(11).integers(1, species + 1, size=len(pos)).astype(np.int32)
    p = decompose(pos, box, types, 1, 0, cut)
    p.box = box
    return p


def cluster_plan(drop=False):
    """A rank without ghosts: the 3x3x3 lattice block of 54 atoms (53 with `drop`) as a free cluster -- empty send
    lists, counts [0], a list over the owned atoms only."""
    pos, _ = mtpgen.bcc_lattice(3, 3, 3)
    if drop:
        pos = pos[:-1]
    n = len(pos)
    first, neigh = full_neighbor_list(pos, n, CLUSTER_CUT)
    return HaloPlan(rank=0, nranks=1, grid=(1, 1, 1), nlocal=n, nghost=0, owned_global=np.arange(n), x0=pos.copy(),
                    types=np.ones(n, dtype=np.int32), ilist=np.arange(n, dtype=np.int32), first=first, neigh=neigh,
                    send_idx=np.zeros(0, dtype=np.int64), send_shift=np.zeros((0, 3)), send_counts=[0], recv_counts=[0],
                    ghost_global=np.zeros(0, dtype=np.int64))


def launch_sizes(p):
    """(3 nsend, (3 nall + 1) / 2): the two sizes halo_pack_zero_kernel's grid is the maximum of."""
    return 3 * len(p.send_idx), (3 * p.nall + 1) // 2


def natural_order(p):
    """(ilist, first, neigh, (na, nb, nc)) of domain.overlap_order."""
    return overlap_order(p)


def hand_order(p, kind):
    """Row orders overlap_order never gives, each with a list reordered to match.  An atom with a ghost in its row
    (boundary) must sit in the middle launch: rows A run beside the forward exchange, before the ghost positions have
    landed, and rows C beside the reverse exchange, which is reading the ghost forces.
      "empty_first"   boundary | all interior atoms          (0, nb, na + nc)
      "empty_last"    all interior atoms | boundary          (na + nc, nb, 0): the middle launch folds the tallies
      "empty_middle"  only for a plan without boundary atoms: (n / 2, 0, n - n / 2)"""
    interior, boundary = split_interior(p)
    if kind == "empty_first":
        order, split = np.concatenate([boundary, interior]), (0, len(boundary), len(interior))
    elif kind == "empty_last":
        order, split = np.concatenate([interior, boundary]), (len(interior), len(boundary), 0)
    elif kind == "empty_middle":
        assert len(boundary) == 0
        order, split = interior, (p.nlocal // 2, 0, p.nlocal - p.nlocal // 2)
    else:
        raise ValueError(kind)
    ilist, first, neigh = sub_list(p, order.astype(np.int64))
    return ilist, first, neigh, split


def order_of(p, kind):
    return natural_order(p) if kind == "natural" else hand_order(p, kind)


def positions(p, seed=5):
    """owned positions: the lattice plus rng.normal(0, 0.03)"""
    return p.x0[: p.nlocal] + np.random.default_rng(seed).normal(0, 0.03, (p.nlocal, 3))


def ghosts_of(p, x_own):
    """what the forward halo must leave in the ghost rows, bit for bit (a copy and one add each)"""
    return x_own[p.send_idx] + np.asarray(p.send_shift).reshape(-1, 3)


def x_all(p, x_own):
    return np.concatenate([x_own, ghosts_of(p, x_own)])


def fold(p, f_all):
    """reverse halo on the host: owned rows + np.add.at of the ghost rows onto send_idx"""
    out = np.array(f_all[: p.nlocal], dtype=np.float64, copy=True)
    np.add.at(out, p.send_idx, f_all[p.nlocal:])
    return out


def model_step(orc, p, x_own, eflag=3, vflag=1, grade=False):
    """numpy model of one step: forward gather + shift, the oracle on x_all over the plan's own list, np.add.at of
    the ghost rows.  Returns the oracle's dict with "f_all" (what the force call leaves, ghosts included) beside the
    folded "f" [nlocal, 3]."""
    want = orc.compute(x_all(p, x_own), p.types, p.ilist, p.first, p.neigh, eflag=eflag, vflag=vflag, extrapolation=grade,
                       natoms=p.nlocal)
    want["f_all"] = want["f"]
    want["f"] = fold(p, want["f_all"])
    return want


def images(p):
    """[nlocal] how many ghost rows are folded onto each owned atom"""
    return np.bincount(p.send_idx, minlength=p.nlocal)


def unpack_bound(p, f_all):
    """Bound on |device fold - np.add.at| per component: the two add the same m + 1 terms (the owner's own value and
    its m ghost rows) in different orders, so they differ by at most (m + 1) 2^-53 sum |terms|."""
    a = np.abs(np.asarray(f_all))
    return (images(p) + 1)[:, None] * 2.0 ** -53 * fold(p, a)
