"""Periodic cells the cell-ghost tests share (tests/test_cell_cpu.py, tests/test_cell_gpu.py): a bcc primitive cell
(1 atom, far smaller than the cutoff), a noisy cubic 2-atom cell, a tilted 5-atom two-species cell, their replicas,
and the oracle evaluation of a cell through the numpy twin of the device ghost build."""
import os

import numpy as np

from lammps_mtp_kokkos_amd.driver import periodic_system_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
A0 = 3.165
LIST_CUTOFF = 7.0

PRIMITIVE = 0.5 * A0 * np.array([[-1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, -1.0]])
CUBIC = A0 * np.eye(3)
TILTED = np.array([[6.4, 0.0, 0.0], [2.1, 5.9, 0.0], [-1.7, 1.3, 6.2]])
SHEARED = np.array([[6.6, 0.0, 0.0], [3.3, 6.1, 0.0], [3.3, 3.05, 6.4]])      # tilt factors 0.5 of the edge they tilt along


def primitive_cell():
    """(pos, cell, types): one atom at the origin (s = 0 exactly: 8 shifts per direction, 511 images under 7 A)"""
    return np.zeros((1, 3)), PRIMITIVE.copy(), np.ones(1, dtype=np.int32)


def cubic2_cell(seed=11):
    rng = np.random.default_rng(seed)
    pos = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.75]]) * A0 + rng.normal(0.0, 0.08, (2, 3))
    return pos, CUBIC.copy(), np.ones(2, dtype=np.int32)


def tilted5_cell(species=2):
    """five atoms at fixed fractional sites of the tilted cell, no pair (images included) closer than 2.4 A"""
    frac = np.array([[0.08, 0.12, 0.10], [0.55, 0.20, 0.31], [0.27, 0.66, 0.18], [0.71, 0.74, 0.62], [0.16, 0.38, 0.77]])
    types = np.array([1, 2, 1, 1, 2], dtype=np.int32) if species == 2 else np.ones(5, dtype=np.int32)
    return frac @ TILTED, TILTED.copy(), types


def replicate(pos, cell, types, reps):
    """the reps[0] x reps[1] x reps[2] supercell: atoms of replica (i, j, k) follow each other in the order of `pos`"""
    out = [pos + i * cell[0] + j * cell[1] + k * cell[2] for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])]
    return np.concatenate(out), cell * np.asarray(reps, dtype=np.float64)[:, None], np.tile(types, int(np.prod(reps)))


def min_image_distance(pos, cell):
    """smallest distance between two atoms or an atom and an image (brute force over +-3 cells)"""
    r = np.arange(-3, 4)
    sh = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3) @ cell
    d = pos[:, None, None, :] - pos[None, :, None, :] - sh[None, None, :, :]
    d = np.sqrt((d ** 2).sum(-1))
    return float(d[d > 1e-9].min())


def oracle_cell(orc, pos, cell, types, list_cutoff=LIST_CUTOFF, **kw):
    """energy, forces folded onto the owned atoms [n, 3], virial [6] and the raw result of one oracle call on the
    images the twin builds"""
    s = periodic_system_cell(pos, cell, types, list_cutoff)
    r = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh, **kw)
    return r["energy"], s.fold_forces(r["f"]), r["virial"], r, s
