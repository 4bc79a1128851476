"""Batches of periodic cells the batched-evaluation tests share (tests/test_batch_cpu.py, tests/test_batch_gpu.py), built
from the cells of tests/_cells.py, and the bounds of the existing cell tests (tests/test_cell_gpu.py)."""
import numpy as np

import _cells

SHEARED8 = np.array([[0.05, 0.12, 0.11], [0.06, 0.14, 0.59], [0.08, 0.64, 0.15], [0.08, 0.63, 0.60],
                     [0.61, 0.05, 0.10], [0.57, 0.10, 0.57], [0.58, 0.59, 0.14], [0.58, 0.55, 0.63]])


def sheared8_cell(species=1):
    """eight atoms at fixed fractional sites of the sheared cell, no pair (images included) closer than 3 A"""
    types = np.array([1, 2, 2, 1, 1, 1, 2, 1], dtype=np.int32) if species == 2 else np.ones(8, dtype=np.int32)
    return SHEARED8 @ _cells.SHEARED, _cells.SHEARED.copy(), types


def replica54_cell(species=1, seed=3):
    """the noisy 2-atom cubic cell 3x3x3, every atom jittered on its own"""
    pos, cell, types = _cells.replicate(*_cells.cubic2_cell(), (3, 3, 3))
    rng = np.random.default_rng(seed)
    pos = pos + rng.normal(0.0, 0.05, pos.shape)
    if species == 2:
        types = (1 + (rng.random(len(pos)) < 0.3)).astype(np.int32)
    return pos, cell, types


def empty_cell():
    return np.zeros((0, 3)), _cells.CUBIC.copy(), np.zeros(0, dtype=np.int32)


def mixed_batch(species=1):
    """primitive 1-atom, cubic 2-atom, tilted 5-atom, an EMPTY configuration in the middle, sheared 8-atom, 54-atom replica"""
    return [_cells.primitive_cell(), _cells.cubic2_cell(), _cells.tilted5_cell(species), empty_cell(), sheared8_cell(species),
            replica54_cell(species)]


def carved(nkeep, species=1, seed=0):
    """a configuration of exactly nkeep atoms: a replica of the tilted 5-atom cell with atoms removed"""
    pos, cell, types = _cells.tilted5_cell(species)
    reps = (1, 1, 1)
    for reps in ((1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4)):
        if 5 * int(np.prod(reps)) >= nkeep:
            break
    pos, cell, types = _cells.replicate(pos, cell, types, reps)
    keep = np.sort(np.random.default_rng(seed).permutation(len(pos))[:nkeep])
    return pos[keep], cell, types[keep]


def close(got, want, what, atol=1e-9, rtol=1e-10):
    """the bounds of tests/test_gpu_parity.py::_close"""
    scale = max(1.0, float(np.abs(want).max())) if np.size(want) else 1.0
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max()) if np.size(want) else 0.0
    print("%s: max abs err %.3e (scale %.3e)" % (what, err, scale))
    assert np.shape(got) == np.shape(want), what
    assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)


def close_energy(got, want, n, what="energy"):
    """1e-10 per atom, relative to max(1, |E| / n)"""
    n = max(n, 1)
    print("%s/atom: got %.12e want %.12e" % (what, got / n, want / n))
    assert abs(got - want) / n <= 1e-10 * max(1.0, abs(want) / n), what
