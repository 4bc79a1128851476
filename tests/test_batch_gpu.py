"""Batched evaluation of many small periodic cells in one device pass (md.evaluate_cells; mtp_batch_layout,
mtp_ghosts_build_batch, mtp_batch_reduce, mtp_batch_cfg_grades): against the numpy twin, the CPU oracle per
configuration and the one-cell path (md.evaluate_cell).  Tolerances: those of tests/test_cell_gpu.py."""
import functools
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi
from lammps_mtp_kokkos_amd.driver import full_neighbor_list, make_ghosts_batch, make_ghosts_cell, periodic_system_cell

import _batch
import _cells
from _cells import POT, LIST_CUTOFF


def _device_stream():
    import torch
    dev = torch.device("cuda:0")
    return dev, capi.use_private_torch_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def _ctx(fname, selection=False):
    return capi.Context(capi.Potential(os.path.join(POT, fname), selection=selection), 0)


@functools.lru_cache(maxsize=None)
def _oracle(fname, selection=False):
    from oracle.pyoracle import Oracle
    return Oracle(os.path.join(POT, fname), selection=selection)


def _far(batch):
    """the tilted cell handed over with its atoms many cells away (the same crystal)"""
    batch = list(batch)
    pos, cell, types = batch[2]
    batch[2] = (pos + np.array([[3, -2, 1], [0, 0, 0], [-7, 4, 0], [1, 1, 1], [0, -5, 2]]) @ cell, cell, types)
    return batch


@functools.lru_cache(maxsize=None)
def _mixed_reference(fname, species):
    """the oracle on every configuration of the mixed batch alone: computed once, shared, never written to"""
    return [None if len(p) == 0 else _cells.oracle_cell(_oracle(fname), p, c, t)[:3] for p, c, t in _batch.mixed_batch(species)]


def _check_against(got, want, n, what, cell=None):
    e, f, v = want
    _batch.close(got["f"], f, "forces, " + what)
    _batch.close_energy(got["energy"], e, n, "energy, " + what)
    _batch.close(got["virial"], v, "virial, " + what, atol=1e-8)
    if cell is not None:
        assert abs(got["volume"] - np.linalg.det(cell)) <= 1e-12 * np.linalg.det(cell)


def _assert_empty(r):
    assert r["energy"] == 0.0 and r["f"].shape == (0, 3) and r["x"].shape == (0, 3) and not r["virial"].any()


def _upload_batch(batch, extra_rows=0):
    """(x tensor [nall + extra_rows, 3] holding the owned atoms, twin, layout, cfg_first) of a batch"""
    import torch
    dev, st = _device_stream()
    lay = capi.batch_layout([c for _, c, _ in batch], LIST_CUTOFF)
    twin = make_ghosts_batch([(p, c) for p, c, _ in batch], lay["origins"], LIST_CUTOFF)
    n = int(twin[4][-1])
    xa = torch.zeros((len(twin[0]) + extra_rows, 3), dtype=torch.float64, device=dev)
    xa[:n] = torch.from_numpy(np.concatenate([p for p, _, _ in batch]))
    return xa, twin, lay, twin[4].astype(np.int32), dev, st


@pytest.mark.gpu
def test_build_batch_matches_the_numpy_twin():
    """owners and integer shifts exactly, positions to 1e-12, in the documented order; the capacity protocol"""
    import torch
    batch = _far(_batch.mixed_batch())
    cells = [c for _, c, _ in batch]
    xa, (want_x, want_owner, want_shift, want_cfg, _), lay, cf, dev, st = _upload_batch(batch)
    n, nall = int(cf[-1]), len(want_x)
    g = capi.Ghosts(0)
    short = torch.full((n + 7, 3), -77.0, dtype=torch.float64, device=dev)          # too short: sizes reported, nothing written
    short[:n] = xa[:n]
    with pytest.raises(capi.MtpError) as ei:
        g.build_batch(short, cf, cells, lay["origins"], LIST_CUTOFF, stream=st)
    assert ei.value.code == -24 and g.nall == nall
    sh = short.cpu().numpy()
    assert np.abs(sh[:n] - want_x[:n]).max() < 1e-12 and (sh[n:] == -77.0).all()      # (beyond the wrap of the owned atoms)
    assert g.build_batch(xa, cf, cells, lay["origins"], LIST_CUTOFF, stream=st) == nall
    got = xa.cpu().numpy()
    assert np.abs(got - want_x).max() < 1e-12
    ty = torch.zeros(nall, dtype=torch.int32, device=dev)                              # owners, through the type fold
    ty[:n] = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    g.types(ty, stream=st)
    torch.cuda.synchronize()
    owner = ty.cpu().numpy().astype(np.int64) - 1
    assert np.array_equal(owner, want_owner)
    hinv = np.stack([np.linalg.inv(c) for c in cells])[want_cfg]
    s = np.einsum("ni,nij->nj", got - got[owner], hinv)
    assert np.abs(s - np.round(s)).max() < 1e-9 and np.array_equal(np.round(s).astype(np.int64), want_shift)
    # forward / reverse on the handle: a moved owner's ghosts follow it, ghost rows fold onto owner rows
    rng = np.random.default_rng(5)
    moved = got[:n] + rng.normal(0, 0.05, (n, 3))
    xa[:n] = torch.from_numpy(moved)
    g.forward(xa, stream=st)
    f_np = rng.normal(size=(nall, 3))
    f = torch.from_numpy(f_np.copy()).to(dev)
    g.reverse(f, stream=st)
    torch.cuda.synchronize()
    assert np.abs((xa.cpu().numpy()[n:] - got[n:]) - (moved - got[:n])[want_owner[n:]]).max() < 1e-12
    want_f = f_np[:n].copy()
    np.add.at(want_f, want_owner[n:], f_np[n:])
    assert np.abs(f.cpu().numpy()[:n] - want_f).max() < 1e-12 * nall


@pytest.mark.gpu
def test_build_batch_error_paths_launch_nothing():
    import torch
    batch = _far(_batch.mixed_batch())
    cells = [c for _, c, _ in batch]
    xa, twin, lay, cf, dev, st = _upload_batch(batch)
    before = xa.cpu().numpy().copy()
    g = capi.Ghosts(0)
    with pytest.raises(capi.MtpError) as ei:
        g.build_batch(xa, cf, cells, lay["origins"], LIST_CUTOFF, stream=None)
    assert ei.value.code == -20 and "NULL stream" in str(ei.value)
    down = cf.copy()
    down[3] = down[2] - 1
    for bad_first in (down, cf + 1):
        with pytest.raises(capi.MtpError) as ei:
            g.build_batch(xa, bad_first, cells, lay["origins"], LIST_CUTOFF, stream=st)
        assert ei.value.code == -20
    for bad in (np.zeros((3, 3)), cells[2][[1, 0, 2]], np.array([[5.0, 0, 0], [0, np.inf, 0], [0, 0, 5.0]])):
        with pytest.raises(capi.MtpError, match="configuration 4") as ei:
            g.build_batch(xa, cf, cells[:4] + [bad] + cells[5:], lay["origins"], LIST_CUTOFF, stream=st)
        assert ei.value.code == -20
    torch.cuda.synchronize()
    assert np.array_equal(xa.cpu().numpy(), before)
    assert g.build_batch(xa, cf, cells, lay["origins"], LIST_CUTOFF, stream=st) == len(twin[0])   # the handle is still good


@pytest.mark.gpu
def test_device_list_over_the_batch_is_the_union_of_the_single_lists():
    """row by row as sets, the single-configuration entries mapped through (owner, shift); nothing crosses a slot"""
    batch = _far(_batch.mixed_batch())
    cells = [c for _, c, _ in batch]
    xa, (want_x, want_owner, want_shift, want_cfg, _), lay, cf, dev, st = _upload_batch(batch)
    n = int(cf[-1])
    ctx = _ctx("W_L8.mtp")
    g = capi.Ghosts(0)
    nall = g.build_batch(xa, cf, cells, lay["origins"], LIST_CUTOFF, stream=st)
    total, longest = ctx.build_neighbors_device(xa, n, nall, LIST_CUTOFF, lay["lo"], lay["hi"], stream=st)
    first, neigh = ctx.neighbors_to_host()
    rows = np.repeat(np.arange(n), np.diff(first))
    assert np.array_equal(want_cfg[neigh], want_cfg[rows])                          # no cross-configuration entry
    row_of = {(int(o), tuple(int(v) for v in s)): r for r, (o, s) in enumerate(zip(want_owner, want_shift))}
    assert len(row_of) == nall
    count = 0
    for k, (pos, cell, _) in enumerate(batch):
        a, nk = int(cf[k]), len(pos)
        x1, owner1, shift1 = make_ghosts_cell(pos, cell, LIST_CUTOFF)
        first1, neigh1 = full_neighbor_list(x1, nk, LIST_CUTOFF)
        to_batch = np.array([row_of[(a + int(o), tuple(int(v) for v in s))] for o, s in zip(owner1, shift1)], dtype=np.int64)
        for i in range(nk):
            want = np.sort(to_batch[neigh1[first1[i]:first1[i + 1]]])
            assert np.array_equal(np.sort(neigh[first[a + i]:first[a + i + 1]]), want), (k, i)
            count += len(want)
    assert count == total == first[-1] and longest == np.diff(first).max()


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", [("W_L8.mtp", 1), ("W_L16.mtp", 1), ("WRe_L20.mtp", 2)])
def test_evaluate_cells_matches_the_oracle_and_evaluate_cell_per_configuration(fname, species):
    """cells smaller than the cutoff, a cell handed over with atoms far outside it, an empty configuration in the middle"""
    from lammps_mtp_kokkos_amd.md import evaluate_cell, evaluate_cells
    ctx = _ctx(fname)
    batch = _far(_batch.mixed_batch(species))
    got = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, vflag=1)
    assert len(got) == len(batch)
    for k, ((pos, cell, types), r, want) in enumerate(zip(batch, got, _mixed_reference(fname, species))):
        if len(pos) == 0:
            _assert_empty(r)
            continue
        _check_against(r, want, len(pos), "configuration %d against the oracle" % k, cell)
        one = evaluate_cell(ctx, pos, cell, types, list_cutoff=LIST_CUTOFF, vflag=1)
        _check_against(r, (one["energy"], one["f"], one["virial"]), len(pos), "configuration %d against evaluate_cell" % k)
        _batch.close(r["x"], one["x"], "wrapped positions of configuration %d" % k, atol=1e-11, rtol=0)
        assert abs(r["volume"] - one["volume"]) <= 1e-12 * one["volume"]
    novirial = evaluate_cells(ctx, batch[:3], list_cutoff=LIST_CUTOFF, vflag=0)
    for r, full in zip(novirial, got):
        assert not r["virial"].any()
        _batch.close(r["f"], full["f"], "forces without the virial")


EDGE_SIZES = [1, 2, capi.BATCH_WAVE_LANES - 1, capi.BATCH_WAVE_LANES, capi.BATCH_WAVE_LANES + 1, 3 * capi.BATCH_WAVE_LANES + 1,
              capi.BATCH_BLOCK - 1, capi.BATCH_BLOCK, capi.BATCH_BLOCK + 1, 0, 2, 1]


@pytest.mark.gpu
def test_segmented_sums_at_the_edges_of_their_lane_and_workgroup_widths():
    """configuration sizes one below, at and one above the wavefront's lanes, the longest segment a wavefront takes (= the
    workgroup size), and one round of the coalesced vatom walk more; 1 and 2 atoms first and last.  mtp_batch_reduce
    against the host sums of the SAME per-atom arrays (only the order of summation differs: 1e-13 of sum |terms|), and
    against the oracle per configuration"""
    import torch
    assert capi.BATCH_WAVE_ROWS == capi.BATCH_BLOCK
    ctx = _ctx("W_L8.mtp")
    small = {0: _batch.empty_cell, 1: _cells.primitive_cell, 2: _cells.cubic2_cell}       # (dense: every atom has neighbours)
    batch = [small[m]() if m in small else _batch.carved(m, seed=q) for q, m in enumerate(EDGE_SIZES)]
    cells = [c for _, c, _ in batch]
    xa, twin, lay, cf, dev, st = _upload_batch(batch)
    n, ncfg = int(cf[-1]), len(batch)
    g = capi.Ghosts(0)
    nall = g.build_batch(xa, cf, cells, lay["origins"], LIST_CUTOFF, stream=st)
    ty = torch.ones(nall, dtype=torch.int32, device=dev)
    ctx.build_neighbors_device(xa, n, nall, LIST_CUTOFF, lay["lo"], lay["hi"], stream=st)
    f = torch.zeros((nall, 3), dtype=torch.float64, device=dev)
    ev = torch.zeros(8, dtype=torch.float64, device=dev)
    eatom = torch.zeros(nall, dtype=torch.float64, device=dev)
    vatom = torch.zeros((nall, 6), dtype=torch.float64, device=dev)
    ctx.compute_device_rows(0, n, False, xa, ty, f, eflag=3, vflag=4, eatom_t=eatom, vatom_t=vatom, ev_t=ev, stream=st)
    g.reverse_finish(ctx, f, ev, eflag=3, vflag=4, stream=st)
    cf_t = torch.from_numpy(cf).to(dev)
    energy = torch.full((ncfg,), -7.0, dtype=torch.float64, device=dev)
    virial = torch.full((ncfg, 6), -7.0, dtype=torch.float64, device=dev)
    cmax = torch.full((ncfg,), -7.0, dtype=torch.float64, device=dev)
    eabs = eatom.abs()                                                               # stands in for per-atom grades
    capi.batch_reduce(cf_t, eatom_t=eatom, vatom_t=vatom, grades_t=eabs, energy_t=energy, virial_t=virial, cfg_grade_t=cmax,
                      stream=st)
    ctx.synchronize(stream=st)
    with pytest.raises(capi.MtpError):
        capi.batch_reduce(cf_t, eatom_t=eatom, energy_t=energy, stream=None)
    ea, va, fh = eatom.cpu().numpy(), vatom.cpu().numpy(), f.cpu().numpy()
    assert not va[n:].any() and not ea[n:].any()                                    # ghost rows carry no tally
    eh, vh, mh, evh = energy.cpu().numpy(), virial.cpu().numpy(), cmax.cpu().numpy(), ev.cpu().numpy()
    for k, (pos, cell, types) in enumerate(batch):
        a, b = int(cf[k]), int(cf[k + 1])
        if a == b:
            assert eh[k] == 0.0 and not vh[k].any() and mh[k] == 0.0
            continue
        err_e = abs(eh[k] - ea[a:b].sum())
        err_v, sum_v = np.abs(vh[k] - va[a:b].sum(0)), np.abs(va[a:b]).sum(0)
        print("n = %d: |dE| %.3e of %.3e, max |dV| %.3e of %.3e" % (b - a, err_e, np.abs(ea[a:b]).sum(), err_v.max(), sum_v.max()))
        assert err_e <= 1e-13 * np.abs(ea[a:b]).sum() and (err_v <= 1e-13 * sum_v).all(), (k, b - a)
        assert mh[k] == np.abs(ea[a:b]).max()
        e, fo, v = _cells.oracle_cell(_oracle("W_L8.mtp"), pos, cell, types)[:3]
        _check_against(dict(energy=eh[k], f=fh[a:b], virial=vh[k]), (e, fo, v), b - a, "n = %d against the oracle" % (b - a))
    # the whole-batch totals of the same call (folded by the ghost fold's launch)
    assert abs(evh[0] - eh.sum()) <= 1e-12 * np.abs(ea).sum() and (np.abs(evh[1:7] - vh.sum(0)) <= 1e-12 * np.abs(va).sum(0)).all()


@pytest.mark.gpu
def test_permuting_the_batch_permutes_the_results():
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    ctx = _ctx("W_L16.mtp")
    batch = _far(_batch.mixed_batch())
    perm = [4, 0, 5, 3, 2, 1]
    got = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF)
    other = evaluate_cells(ctx, [batch[p] for p in perm], list_cutoff=LIST_CUTOFF)
    for j, p in enumerate(perm):
        if len(batch[p][0]) == 0:
            _assert_empty(other[j])
            continue
        _check_against(other[j], (got[p]["energy"], got[p]["f"], got[p]["virial"]), len(batch[p][0]), "configuration %d moved" % p)


@pytest.mark.gpu
def test_neighbourhood_grades_per_atom_and_per_configuration_match_the_oracle():
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    fname = "W_L16_nbh.almtp"
    ctx, orc = _ctx(fname, True), _oracle(fname, True)
    batch = _far(_batch.mixed_batch())
    got = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    for k, ((pos, cell, types), r) in enumerate(zip(batch, got)):
        if len(pos) == 0:
            _assert_empty(r)
            assert r["grades"].shape == (0,) and r["max_grade"] == 0.0
            continue
        s = periodic_system_cell(pos, cell, types, LIST_CUTOFF)
        want = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=s.nlocal)
        _batch.close(r["grades"], want["grades"][: s.nlocal], "grades of configuration %d" % k, atol=1e-9, rtol=1e-9)
        assert abs(r["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"]), k
        assert r["max_grade"] == r["grades"].max()
        _check_against(r, (want["energy"], s.fold_forces(want["f"]), want["virial"]), len(pos), "configuration %d (grade call)" % k)


def _cfg_grade_want(orc, pos, cell, types):
    s = periodic_system_cell(pos, cell, types, LIST_CUTOFF)
    return orc.compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=s.nlocal)


@pytest.mark.gpu
def test_configuration_grades_match_the_oracle_per_configuration():
    """configurations of 1, 2, 5, 0, 8 and 54 atoms of both species: an unsegmented sum or the wrong divisor fails"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    fname = "WRe_L10_cfg.almtp"
    ctx, orc = _ctx(fname, True), _oracle(fname, True)
    assert ctx.pot.info.configuration_mode
    batch = _far(_batch.mixed_batch(2))
    batch[0] = (batch[0][0], batch[0][1], np.array([2], dtype=np.int32))
    got = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    seen = []
    for k, ((pos, cell, types), r) in enumerate(zip(batch, got)):
        assert "grades" not in r
        if len(pos) == 0:
            _assert_empty(r)
            assert r["cfg_grade"] == 0.0
            continue
        want = _cfg_grade_want(orc, pos, cell, types)
        print("configuration %d (%d atoms): cfg_grade %.12e want %.12e" % (k, len(pos), r["cfg_grade"], want["max_grade"]))
        assert abs(r["cfg_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"]), k
        _check_against(r, (want["energy"], periodic_system_cell(pos, cell, types, LIST_CUTOFF).fold_forces(want["f"]),
                           want["virial"]), len(pos), "configuration %d (grade call)" % k)
        seen.append(want["max_grade"])
    assert len(set(np.round(seen, 6))) == len(seen)                                 # the grades do tell the configurations apart


@pytest.mark.gpu
def test_configuration_grades_of_more_configurations_than_a_grade_workgroup_takes():
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    fname = "WRe_L10_cfg.almtp"
    ctx, orc = _ctx(fname, True), _oracle(fname, True)
    ncfg = capi.GRADE_ROWS_PER_BLOCK + 22
    rng = np.random.default_rng(12)
    batch = []
    for k in range(ncfg):                                                            # the primitive cell, strained
        strain = np.eye(3) + rng.uniform(-0.04, 0.04, (3, 3))
        batch.append((np.zeros((1, 3)), _cells.PRIMITIVE @ strain, np.array([1 + k % 2], dtype=np.int32)))
    batch[ncfg // 2] = _batch.empty_cell()
    got = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    for k, ((pos, cell, types), r) in enumerate(zip(batch, got)):
        if len(pos) == 0:
            assert r["cfg_grade"] == 0.0
            continue
        want = _cfg_grade_want(orc, pos, cell, types)
        assert abs(r["cfg_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"]), k
        _batch.close_energy(r["energy"], want["energy"], 1, "energy of configuration %d" % k)


@pytest.mark.gpu
def test_three_passes_give_the_results_of_one_in_input_order(monkeypatch):
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    ctx = _ctx("W_L16.mtp")
    batch = _far(_batch.mixed_batch())
    builds = []
    real = capi.Ghosts.build_batch

    def counted(self, x_t, cfg_first, *a, **kw):
        builds.append(int(cfg_first[-1]))
        return real(self, x_t, cfg_first, *a, **kw)

    monkeypatch.setattr(capi.Ghosts, "build_batch", counted)
    one = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF)
    assert builds == [70]
    del builds[:]
    three = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, max_atoms_per_pass=10)
    assert builds == [8, 8, 54]                                                      # 1 + 2 + 5 + 0 | 8 | 54 owned atoms
    for k, (a, b) in enumerate(zip(one, three)):
        if len(batch[k][0]) == 0:
            _assert_empty(b)
            continue
        _check_against(b, (a["energy"], a["f"], a["virial"]), len(batch[k][0]), "configuration %d" % k)
        _batch.close(b["x"], a["x"], "wrapped positions of configuration %d" % k, atol=1e-11, rtol=0)


@pytest.mark.gpu
def test_an_atom_type_outside_the_potential_is_reported_at_the_synchronise_naming_the_pass():
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    ctx = _ctx("W_L8.mtp")
    batch = _batch.mixed_batch()
    batch[4] = (batch[4][0], batch[4][1], np.array([1, 1, 1, 2, 1, 1, 1, 1], dtype=np.int32))
    with pytest.raises(capi.MtpError, match="pass 2") as ei:
        evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, max_atoms_per_pass=10)
    assert ei.value.code == -22
    good = evaluate_cells(ctx, _batch.mixed_batch()[:3], list_cutoff=LIST_CUTOFF)     # the context is still good
    _check_against(good[1], _mixed_reference("W_L8.mtp", 1)[1], 2, "after the refusal")


# ---- the single-cell build and the batched build are one criterion with two sources of the cell; one handle serves both ------

def _owners(g, n, nall, dev, st):
    """the owner row of every row of the last build, read through the type fold"""
    import torch
    ty = torch.zeros(nall, dtype=torch.int32, device=dev)
    ty[:n] = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    g.types(ty, stream=st)
    torch.cuda.synchronize()
    return ty.cpu().numpy().astype(np.int64) - 1


def _rows(pos, nall, dev):
    import torch
    xa = torch.zeros((nall, 3), dtype=torch.float64, device=dev)
    xa[:len(pos)] = torch.from_numpy(np.ascontiguousarray(pos))
    return xa


def _one_cell_case(which):
    if which == "primitive":                       # hundreds of images of its one atom: the zero-shift skip, the per-ghost decode
        pos, cell, _ = _cells.primitive_cell()
    elif which == "tilted5_far":
        pos, cell, _ = _far(_batch.mixed_batch())[2]
    else:
        pos, cell, _ = _batch.sheared8_cell()
    return pos, cell


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["primitive", "tilted5_far", "sheared8"])
def test_a_batch_of_one_configuration_is_the_single_cell_build(which):
    """build_batch with cfg_first = [0, n] and a zero origin against build_cell on another handle: the same count, owners and
    ghost offsets from their owners (both form a ghost as owner + shift) bit for bit; the owned rows with ==, since the
    origin add can only turn a -0.0 into +0.0.  The tilted cell again under a non-zero origin: rows minus the origin to
    1e-12, the bound of the twin tests for a translated cell."""
    pos, cell = _one_cell_case(which)
    n = len(pos)
    dev, st = _device_stream()
    nall = len(make_ghosts_cell(pos, cell, LIST_CUTOFF)[0])
    assert nall > n
    cf = np.array([0, n], dtype=np.int32)
    gc, xc = capi.Ghosts(0), _rows(pos, nall, dev)
    assert gc.build_cell(xc, n, cell, LIST_CUTOFF, stream=st) == nall
    owner_c, one = _owners(gc, n, nall, dev, st), xc.cpu().numpy()
    origins = [np.zeros((1, 3))] + ([np.array([[11.5, -3.25, 0.75]])] if which == "tilted5_far" else [])
    for org in origins:
        gb, xb = capi.Ghosts(0), _rows(pos, nall, dev)
        assert gb.build_batch(xb, cf, [cell], org, LIST_CUTOFF, stream=st) == nall
        owner_b, many = _owners(gb, n, nall, dev, st), xb.cpu().numpy()
        assert np.array_equal(owner_b, owner_c) and np.array_equal(owner_c[:n], np.arange(n))
        if not org.any():
            assert np.array_equal(many[n:] - many[owner_b[n:]], one[n:] - one[owner_c[n:]])
            assert (many[:n] == one[:n]).all()
        else:
            err = float(np.abs((many - org) - one).max())
            print("%s under origin %s: max |rows - origin - single-cell rows| %.3e" % (which, org[0], err))
            assert err < 1e-12


@pytest.mark.gpu
def test_one_handle_across_every_build_growing_and_shrinking():
    """orthogonal build, build_cell and build_batch in turn on ONE handle, sizes going 16 -> 1 -> 70 -> 300 -> 3 -> 1 owned
    atoms (every buffer regrows at the 300, the range buffer with its 64-bit total behind it among them): after each, nall,
    owners and positions are those a fresh handle gives for the same call -- the same code on the same input, compared
    exactly.  After each of the last two builds owner(), then deform with identity matrices: forward reproduces that build's
    ghost rows exactly -- the second time only if the build in between dropped the shifts the first deform had kept."""
    import torch
    from lammps_mtp_kokkos_amd import mtpgen
    dev, st = _device_stream()

    def cell_step(pos, cell):
        nall = len(make_ghosts_cell(pos, cell, LIST_CUTOFF)[0])
        return len(pos), (lambda: _rows(pos, nall, dev)), (lambda g, x: g.build_cell(x, len(pos), cell, LIST_CUTOFF, stream=st))

    def batch_step(batch):
        xa, twin, lay, cf, _, _ = _upload_batch(batch)
        cells = [c for _, c, _ in batch]
        return int(cf[-1]), xa.clone, (lambda g, x: g.build_batch(x, cf, cells, lay["origins"], LIST_CUTOFF, stream=st))

    bpos, box = mtpgen.bcc_lattice(2, 2, 2)
    assert (box >= 3.0).all()
    ppos, pcell, _ = _cells.primitive_cell()
    tpos, tcell, _ = _cells.replicate(*_cells.tilted5_cell(), (4, 3, 5))
    assert len(tpos) == 300
    steps = [("box", (len(bpos), (lambda: _rows(bpos, 27 * len(bpos), dev)),
                      (lambda g, x: g.build(x, len(bpos), box, 3.0, stream=st)))),
             ("primitive", cell_step(ppos, pcell)),
             ("mixed batch", batch_step(_batch.mixed_batch())),
             ("tilted 300", cell_step(tpos, tcell)),
             ("first two of the batch", batch_step(_batch.mixed_batch()[:2])),
             ("primitive again", cell_step(ppos, pcell))]
    row_cfg_of = {"first two of the batch": [0, 1, 1], "primitive again": [0]}    # the configuration of every owned row
    g = capi.Ghosts(0)
    for what, (n, rows, build) in steps:
        got, want = [], []
        for handle, out in ((g, got), (capi.Ghosts(0), want)):
            x = rows()
            nall = build(handle, x)
            out += [nall, _owners(handle, n, nall, dev, st), x.cpu().numpy()[:nall], x]
        print("%s: %d owned, %d rows" % (what, n, got[0]))
        assert got[0] == want[0] > n, what
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
        if what not in row_cfg_of:
            continue
        nall, owner, built, x = got
        ptr, nown = g.owner(stream=st)                                               # identity | owners, in the handle's storage

        class _Span:
            pass
        span = _Span()
        span.__cuda_array_interface__ = dict(shape=(nown,), typestr="<i4", data=(int(ptr), False), version=2, strides=None)
        torch.cuda.synchronize()
        assert nown == nall and np.array_equal(torch.as_tensor(span, device=dev).cpu().numpy(), owner)
        row_cfg = torch.tensor(row_cfg_of[what], dtype=torch.int32, device=dev)
        eye = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(max(row_cfg_of[what]) + 1, 1).contiguous()
        g.deform(row_cfg, eye, stream=st)
        x[n:] = -5.0
        g.forward(x, stream=st)
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy()[:nall], built)
