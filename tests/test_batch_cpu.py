"""Batched configurations without a GPU: the slot layout (mtp_batch_layout), its refusals, and -- with the numpy twin of
the batched ghost build (driver.make_ghosts_batch) and the CPU oracle -- that configurations placed in their slots do
not see each other: one oracle call over the merged system reproduces every configuration on its own."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi
from lammps_mtp_kokkos_amd.driver import full_neighbor_list, make_ghosts_batch

import _batch
import _cells
from _cells import POT, LIST_CUTOFF


def _slots(batch, lay, cut):
    """[lo, hi] of every configuration's ghost parallelepiped, translated by its origin"""
    out = []
    for (_, cell, _), org in zip(batch, lay["origins"]):
        b = capi.ghosts_cell_bounds(cell, cut)
        out.append((b["lo"] + org, b["hi"] + org))
    return out


def test_layout_gives_every_configuration_a_slot_of_its_own():
    batch = _batch.mixed_batch()
    gap = LIST_CUTOFF
    lay = capi.batch_layout([c for _, c, _ in batch], LIST_CUTOFF, gap)
    x, owner, shift, cfg, cfg_first = make_ghosts_batch([(p, c) for p, c, _ in batch], lay["origins"], LIST_CUTOFF)
    assert list(np.diff(cfg_first)) == [1, 2, 5, 0, 8, 54] and len(x) == len(cfg) > cfg_first[-1]
    slots = _slots(batch, lay, LIST_CUTOFF)
    for k, (lo, hi) in enumerate(slots):
        rows = x[cfg == k]
        assert len(rows) == (0 if k == 3 else len(rows)) and (k == 3 or len(rows) > len(batch[k][0]))
        assert (rows >= lo).all() and (rows <= hi).all(), k                       # inside its slot
        assert (lo >= lay["lo"]).all() and (hi <= lay["hi"]).all(), k             # the slot inside the box
    assert (x >= lay["lo"]).all() and (x <= lay["hi"]).all()
    assert np.abs(x).max() < 2048.0
    for j in range(len(batch)):
        for k in range(j):
            # slots: the largest axis separation (1e-9: the test's own rounding of lo + origin)
            sep = np.maximum(slots[j][0] - slots[k][1], slots[k][0] - slots[j][1]).max()
            assert sep >= gap - 1e-9, (j, k, sep)
            a, b = x[cfg == j], x[cfg == k]
            if len(a) and len(b):                                                 # and the atoms in them, exactly
                assert np.maximum(a.min(0) - b.max(0), b.min(0) - a.max(0)).max() >= gap, (j, k)
    assert lay["ncells"] == int(np.prod(np.ceil((lay["hi"] - lay["lo"]) / LIST_CUTOFF)))
    # the ghosts follow their owners by owner + shift . cell, and belong to their owner's configuration
    h = np.stack([c for _, c, _ in batch])[cfg]
    assert np.abs(x - (x[owner] + np.einsum("ni,nij->nj", shift.astype(float), h))).max() < 1e-12
    assert np.array_equal(cfg, cfg[owner]) and np.array_equal(owner[: cfg_first[-1]], np.arange(cfg_first[-1]))
    assert (np.diff(owner[cfg_first[-1]:]) >= 0).all()                            # ghosts in atom order


def test_layout_refuses_a_degenerate_cell_and_names_it():
    cells = [c for _, c, _ in _batch.mixed_batch()]
    for bad in (np.zeros((3, 3)), np.diag([5.0, 5.0, -5.0]), np.array([[5.0, 0, 0], [0, np.nan, 0], [0, 0, 5.0]])):
        with pytest.raises(capi.MtpError, match="configuration 2:") as ei:
            capi.batch_layout(cells[:2] + [bad] + cells[2:], LIST_CUTOFF)
        assert ei.value.code == -20
    with pytest.raises(capi.MtpError) as ei:                                       # a gap below the list cutoff
        capi.batch_layout(cells, LIST_CUTOFF, 0.5 * LIST_CUTOFF)
    assert ei.value.code == -20


@pytest.mark.parametrize("ncfg,cut,why", [(20000, 60.0, "2048 A"), (300000, 1.0, "2\\^26 list cells")])
def test_layout_refuses_a_batch_beyond_its_limits_and_says_where_to_split(ncfg, cut, why):
    cells = np.broadcast_to(_cells.CUBIC, (ncfg, 3, 3))
    with pytest.raises(capi.MtpError, match=why) as ei:
        capi.batch_layout(cells, cut)
    nfit = ei.value.nfit
    assert ei.value.code == -24 and 0 < nfit < ncfg and ("configuration %d " % nfit) in str(ei.value)
    lay = capi.batch_layout(cells[:nfit], cut)                                     # the prefix it names does fit
    assert np.abs(lay["lo"]).max() <= 2048.0 and np.abs(lay["hi"]).max() <= 2048.0 and lay["ncells"] <= 2 ** 26
    with pytest.raises(capi.MtpError) as ei:
        capi.batch_layout(cells[: nfit + 1], cut)
    assert ei.value.code == -24 and ei.value.nfit == nfit


@pytest.mark.parametrize("fname,species", [("W_L16.mtp", 1), ("WRe_L20.mtp", 2)])
def test_merged_system_reproduces_every_configuration_alone(fname, species):
    """isolation on the CPU: the twin's merged system and ONE list over all its positions, in one oracle call"""
    from oracle.pyoracle import Oracle
    orc = Oracle(os.path.join(POT, fname))
    batch = _batch.mixed_batch(species)
    lay = capi.batch_layout([c for _, c, _ in batch], LIST_CUTOFF)
    x, owner, _, cfg, cfg_first = make_ghosts_batch([(p, c) for p, c, _ in batch], lay["origins"], LIST_CUTOFF)
    ntot = int(cfg_first[-1])
    types = np.concatenate([t for _, _, t in batch]).astype(np.int32)[owner]
    first, neigh = full_neighbor_list(x, ntot, LIST_CUTOFF)
    rows = np.repeat(np.arange(ntot), np.diff(first))
    assert np.array_equal(cfg[neigh], cfg[rows])                                   # no entry from another configuration
    got = orc.compute(x, types, np.arange(ntot, dtype=np.int32), first, neigh)
    fold = np.zeros((ntot, 3))
    np.add.at(fold, owner, got["f"])
    assert not got["vatom"][ntot:].any() and not got["eatom"][ntot:].any()       # tallied on the central atom
    for k, (pos, cell, ty) in enumerate(batch):
        a, b = int(cfg_first[k]), int(cfg_first[k + 1])
        if a == b:                                                                 # the empty configuration: no rows at all
            assert len(pos) == 0 and not (cfg == k).any()
            continue
        e, f, v, r, s = _cells.oracle_cell(orc, pos, cell, ty)
        _batch.close(fold[a:b], f, "forces of configuration %d" % k)
        _batch.close_energy(got["eatom"][a:b].sum(), e, b - a, "energy of configuration %d" % k)
        _batch.close(got["eatom"][a:b], r["eatom"][: b - a], "eatom of configuration %d" % k, atol=1e-10, rtol=1e-10)
        _batch.close(got["vatom"][a:b].sum(0), v, "virial of configuration %d" % k, atol=1e-8)
        _batch.close(x[a:b] - lay["origins"][k], s.x[: b - a], "wrapped positions", atol=1e-11, rtol=0)


def _covers_in_order(passes, ncfg):
    assert passes[0][0] == 0 and passes[-1][1] == ncfg
    assert all(a[1] == b[0] for a, b in zip(passes, passes[1:])) and all(k0 < k1 for k0, k1, _ in passes)


def test_passes_split_by_atoms_by_the_layout_limits_and_by_the_row_count():
    """md.plan_cell_passes, the host half of md.evaluate_cells"""
    from lammps_mtp_kokkos_amd.md import plan_cell_passes
    batch = _batch.mixed_batch()
    cells, natoms = [c for _, c, _ in batch], [len(p) for p, _, _ in batch]
    one, volume, rows = plan_cell_passes(cells, natoms, LIST_CUTOFF)
    assert [(a, b) for a, b, _ in one] == [(0, 6)]
    assert np.allclose(volume, [np.linalg.det(c) for c in cells], rtol=1e-14, atol=0)
    x, _, _, cfg, _ = make_ghosts_batch([(p, c) for p, c, _ in batch], one[0][2]["origins"], LIST_CUTOFF)
    assert (np.bincount(cfg, minlength=6) <= rows).all() and rows[3] == 0          # an upper bound of every configuration's rows
    three, _, _ = plan_cell_passes(cells, natoms, LIST_CUTOFF, max_atoms_per_pass=10)
    assert [(a, b) for a, b, _ in three] == [(0, 4), (4, 5), (5, 6)]               # 1 + 2 + 5 + 0 | 8 | 54: never split
    # beyond the list-cell limit: split where the layout says, every pass inside the limits
    ncfg = 300000
    many = np.broadcast_to(_cells.CUBIC, (ncfg, 3, 3))
    with pytest.raises(capi.MtpError) as ei:
        capi.batch_layout(many, 1.0)
    passes, _, _ = plan_cell_passes(many, np.full(ncfg, 2), 1.0)
    _covers_in_order(passes, ncfg)
    assert len(passes) >= 2 and passes[0][1] == ei.value.nfit
    for k0, k1, lay in passes:
        assert lay["ncells"] <= capi.BATCH_MAX_CELLS and max(np.abs(lay["lo"]).max(), np.abs(lay["hi"]).max()) <= capi.BATCH_MAX_COORD
        assert len(lay["origins"]) == k1 - k0
    # cells far smaller than the cutoff: owned + ghost atoms of a pass stay below 2^31
    tiny = np.broadcast_to(0.5 * np.eye(3), (500, 3, 3))
    passes, _, rows = plan_cell_passes(tiny, np.full(500, 200), LIST_CUTOFF)
    _covers_in_order(passes, 500)
    assert rows.sum() > 2 ** 31 and len(passes) >= 2
    assert all(rows[k0:k1].sum() + 200 * (k1 - k0) < 2 ** 31 for k0, k1, _ in passes)
    with pytest.raises(capi.MtpError, match="configuration 2:") as ei:
        plan_cell_passes(cells[:2] + [np.zeros((3, 3))] + cells[2:], [1, 2, 3] + natoms[2:], LIST_CUTOFF)
    assert ei.value.code == -20
