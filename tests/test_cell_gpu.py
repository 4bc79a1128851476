"""Device ghost images for any periodic cell (mtp_ghosts_build_cell, md.evaluate_cell, md.DeviceNVE with a 3x3 cell):
against the numpy twin (driver.make_ghosts_cell), the CPU oracle fed by that twin, the orthogonal build, and the
cell-vs-replica invariance on the device."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import full_neighbor_list, make_ghosts_cell

import _cells
from _cells import POT, LIST_CUTOFF

MVV2E = 1.0364269e-4          # (g/mol)(A/ps)^2 -> eV
FTM2V = 1.0 / MVV2E           # eV/A / (g/mol) -> A/ps^2
KB = 8.617343e-5
MASS = 183.84


def _close(got, want, what, atol=1e-9, rtol=1e-10):
    """the bounds of tests/test_gpu_parity.py::_close"""
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print("%s: max abs err %.3e (scale %.3e)" % (what, err, scale))
    assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)


def _random_case(which, seed=21):
    """(pos, cell): random positions (exact lattice sites sit on ties of the criterion), a tenth of the atoms thrown
    many cells away"""
    rng = np.random.default_rng(seed)
    if which == "tilted5":
        pos, cell, _ = _cells.tilted5_cell()
    elif which == "tilted300":
        pos, cell, types = _cells.tilted5_cell()
        pos, cell, _ = _cells.replicate(pos, cell, types, (4, 3, 5))
    elif which == "primitive":
        cell = _cells.PRIMITIVE.copy()
        pos = np.array([[0.37, 0.61, 0.83]]) @ cell
    elif which == "sheared":
        cell = _cells.SHEARED.copy()
        pos = rng.random((40, 3)) @ cell
    else:
        pos, box = mtpgen.bcc_lattice(8, 8, 8)
        cell = np.diag(box)
    pos = pos + rng.normal(0, 0.3, pos.shape) + np.array([40.0, -13.0, 0.2]) * (rng.random((len(pos), 1)) < 0.1)
    return pos, cell


def _device_stream():
    import torch
    dev = torch.device("cuda:0")
    return dev, capi.use_private_torch_stream(dev).cuda_stream


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tilted5", "tilted300", "primitive", "bcc8"])
def test_build_cell_matches_the_numpy_twin(which):
    """same count, same (owner type, position) rows -- in the documented order: atom, then lexicographic shift --, owned
    atoms wrapped into the cell; the capacity protocol; forward / reverse / types on the handle afterwards"""
    import torch
    pos, cell = _random_case(which)
    n = len(pos)
    rng = np.random.default_rng(5)
    dev, st = _device_stream()
    g = capi.Ghosts(0)
    x = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    x.copy_(torch.from_numpy(pos))
    with pytest.raises(capi.MtpError) as ei:       # no room for ghosts: the size needed is reported
        g.build_cell(x, n, cell, LIST_CUTOFF, stream=st)
    assert ei.value.code == -24 and g.nall > n
    want_x, want_owner, want_shift = make_ghosts_cell(pos, cell, LIST_CUTOFF)
    assert g.nall == len(want_x)
    assert np.abs(x.cpu().numpy() - want_x[:n]).max() < 1e-12          # the refused call wrapped, and wrote nothing else
    xa = torch.zeros((g.nall, 3), dtype=torch.float64, device=dev)
    xa[:n] = torch.from_numpy(pos)
    nall = g.build_cell(xa, n, cell, LIST_CUTOFF, stream=st)
    got = xa.cpu().numpy()
    assert nall == len(want_x)
    s = got[:n] @ np.linalg.inv(cell)
    assert np.abs(got[:n] - want_x[:n]).max() < 1e-12 and (s > -1e-12).all() and (s < 1 + 1e-12).all()
    tyh = rng.integers(1, 4, n).astype(np.int32)
    ty = torch.zeros(nall, dtype=torch.int32, device=dev)
    ty[:n] = torch.from_numpy(tyh)
    g.types(ty, stream=st)
    torch.cuda.synchronize()
    order = lambda t, p: np.lexsort((np.round(p[:, 2], 6), np.round(p[:, 1], 6), np.round(p[:, 0], 6), t))
    got_t, want_t = ty.cpu().numpy()[n:], tyh[want_owner[n:]]
    ko, kw = order(got_t, got[n:]), order(want_t, want_x[n:])
    assert np.array_equal(got_t[ko], want_t[kw]) and np.abs(got[n:][ko] - want_x[n:][kw]).max() < 1e-9   # the multiset
    assert np.abs(got[n:] - want_x[n:]).max() < 1e-9                    # and the order
    assert np.array_equal(ty.cpu().numpy()[n:], tyh[want_owner[n:]])
    # forward: ghosts follow their owners; reverse: ghost rows add onto owner rows
    moved = got[:n] + rng.normal(0, 0.05, (n, 3))
    xa[:n] = torch.from_numpy(moved)
    g.forward(xa, stream=st)
    f_np = rng.normal(size=(nall, 3))
    f = torch.from_numpy(f_np.copy()).to(dev)
    g.reverse(f, stream=st)
    torch.cuda.synchronize()
    new = xa.cpu().numpy()
    assert np.abs((new[n:] - got[n:]) - (moved - got[:n])[want_owner[n:]]).max() < 1e-12
    want_f = f_np[:n].copy()
    np.add.at(want_f, want_owner[n:], f_np[n:])
    assert np.abs(f.cpu().numpy()[:n] - want_f).max() < 1e-12 * max(1.0, nall / n)


@pytest.mark.gpu
@pytest.mark.parametrize("ncell,cut", [((4, 4, 4), 7.0), ((3, 5, 4), 5.5)])
def test_diagonal_cell_gives_the_rows_of_the_orthogonal_build_in_order(ncell, cut):
    import torch
    pos, box = mtpgen.bcc_lattice(*ncell)
    rng = np.random.default_rng(21)
    pos = pos + rng.normal(0, 0.3, pos.shape) + np.array([40.0, -13.0, 0.2]) * (rng.random((len(pos), 1)) < 0.1)
    n = len(pos)
    dev, st = _device_stream()
    out = []
    for cell in (None, np.diag(box)):
        g = capi.Ghosts(0)
        xa = torch.zeros((40 * n, 3), dtype=torch.float64, device=dev)
        xa[:n] = torch.from_numpy(pos)
        nall = g.build(xa, n, box, cut, stream=st) if cell is None else g.build_cell(xa, n, cell, cut, stream=st)
        out.append(xa[:nall].cpu().numpy())
    assert out[0].shape == out[1].shape and len(out[0]) > n
    assert np.abs(out[0] - out[1]).max() < 1e-12


def _oracle_vs_device(fname, pos, cell, types):
    from oracle.pyoracle import Oracle
    from lammps_mtp_kokkos_amd.md import evaluate_cell
    path = os.path.join(POT, fname)
    ctx = capi.Context(capi.Potential(path), 0)
    got = evaluate_cell(ctx, pos, cell, types, list_cutoff=LIST_CUTOFF, vflag=1)
    e, f, v, _, _ = _cells.oracle_cell(Oracle(path), pos, cell, types)
    n = len(pos)
    _close(got["f"], f, "forces")
    print("energy/atom: got %.12e want %.12e" % (got["energy"] / n, e / n))
    assert abs(got["energy"] - e) / n <= 1e-10 * max(1.0, abs(e) / n)
    _close(got["virial"], v, "virial", atol=1e-8)
    assert abs(got["volume"] - np.linalg.det(cell)) <= 1e-12 * np.linalg.det(cell)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("fname", ["W_L8.mtp", "W_L16.mtp"])
@pytest.mark.parametrize("which", ["primitive", "cubic2"])
def test_evaluate_cell_matches_oracle_on_cells_smaller_than_the_cutoff(which, fname):
    pos, cell, types = getattr(_cells, which + "_cell")()
    _oracle_vs_device(fname, pos, cell, types)


@pytest.mark.gpu
def test_evaluate_cell_matches_oracle_on_the_tilted_two_species_cell():
    pos, cell, types = _cells.tilted5_cell()
    _oracle_vs_device("WRe_L20.mtp", pos, cell, types)
    # atoms handed over outside the cell: same crystal
    far = pos + np.array([[3, -2, 1], [0, 0, 0], [-7, 4, 0], [1, 1, 1], [0, -5, 2]]) @ cell
    _oracle_vs_device("WRe_L20.mtp", far, cell, types)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["primitive", "cubic2", "tilted5"])
def test_evaluate_cell_grades_match_oracle(which):
    from oracle.pyoracle import Oracle
    from lammps_mtp_kokkos_amd.md import evaluate_cell
    from lammps_mtp_kokkos_amd.driver import periodic_system_cell
    path = os.path.join(POT, "W_L16_nbh.almtp")
    pos, cell, types = getattr(_cells, which + "_cell")() if which != "tilted5" else _cells.tilted5_cell(1)
    ctx = capi.Context(capi.Potential(path, selection=True), 0)
    got = evaluate_cell(ctx, pos, cell, types, list_cutoff=LIST_CUTOFF, vflag=1, grades=True)
    s = periodic_system_cell(pos, cell, types, LIST_CUTOFF)
    want = Oracle(path, selection=True).compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=s.nlocal)
    _close(got["grades"], want["grades"][: s.nlocal], "grades", atol=1e-9, rtol=1e-9)
    assert abs(got["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])
    _close(got["f"], s.fold_forces(want["f"]), "forces (grade call)")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tilted5", "tilted300", "primitive", "sheared"])
def test_device_list_over_cell_ghosts_equals_host_list(which):
    """mtp_build_neighbors_device inside the bounding box mtp_ghosts_cell_bounds reports (its corner cells are empty
    for a tilted cell), row by row as sets against the host list over the same positions"""
    import torch
    pos, cell = _random_case(which, seed=8)
    n = len(pos)
    dev, st = _device_stream()
    ctx = capi.Context(capi.Potential(os.path.join(POT, "W_L8.mtp")), 0)
    g = capi.Ghosts(0)
    want_n = len(make_ghosts_cell(pos, cell, LIST_CUTOFF)[0])
    xa = torch.zeros((want_n, 3), dtype=torch.float64, device=dev)
    xa[:n] = torch.from_numpy(pos)
    nall = g.build_cell(xa, n, cell, LIST_CUTOFF, stream=st)
    assert nall == want_n
    b = capi.ghosts_cell_bounds(cell, LIST_CUTOFF)
    x = xa.cpu().numpy()
    assert (x >= b["lo"]).all() and (x <= b["hi"]).all()
    total, longest = ctx.build_neighbors_device(xa, n, nall, LIST_CUTOFF, b["lo"], b["hi"], stream=st)
    first, neigh = ctx.neighbors_to_host()
    wfirst, wneigh = full_neighbor_list(x, n, LIST_CUTOFF)
    assert total == wfirst[-1] and np.array_equal(first, wfirst) and longest == np.diff(wfirst).max()
    for i in range(n):
        assert np.array_equal(np.sort(neigh[first[i]:first[i + 1]]), np.sort(wneigh[wfirst[i]:wfirst[i + 1]])), i
    if which == "primitive":                   # every neighbour is a ghost, the atom's own images
        assert n == 1 and (neigh >= 1).all() and len(neigh) > 60


@pytest.mark.gpu
@pytest.mark.parametrize("fname", ["W_L8.mtp", "W_L16.mtp"])
def test_primitive_cell_equals_its_replica_on_the_device(fname):
    from lammps_mtp_kokkos_amd.md import evaluate_cell
    ctx = capi.Context(capi.Potential(os.path.join(POT, fname)), 0)
    pos, cell, types = _cells.primitive_cell()
    one = evaluate_cell(ctx, pos, cell, types, list_cutoff=LIST_CUTOFF)
    pos_n, cell_n, types_n = _cells.replicate(pos, cell, types, (4, 4, 4))
    many = evaluate_cell(ctx, pos_n, cell_n, types_n, list_cutoff=LIST_CUTOFF)
    _close(many["energy"] / 64, one["energy"], "energy per cell")
    _close(many["f"], np.tile(one["f"], (64, 1)), "forces per atom")
    _close(many["virial"] / 64, one["virial"], "virial per cell", atol=1e-8)
    assert abs(many["volume"] - 64 * one["volume"]) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("fname", ["W_L8.mtp", "W_L16.mtp"])
def test_small_cell_equals_its_replica_through_the_orthogonal_device_path(fname):
    """2-atom cubic cell through evaluate_cell against its 3x3x3 replica through the existing DeviceNVE(box=...) force
    path (mtp_ghosts_build, one image per direction)"""
    from lammps_mtp_kokkos_amd.md import DeviceNVE, evaluate_cell
    pot = capi.Potential(os.path.join(POT, fname))
    ctx = capi.Context(pot, 0)
    pos, cell, types = _cells.cubic2_cell()
    one = evaluate_cell(ctx, pos, cell, types, list_cutoff=LIST_CUTOFF)
    pos_n, cell_n, types_n = _cells.replicate(pos, cell, types, (3, 3, 3))
    md = DeviceNVE(ctx, pos_n, np.diag(cell_n).copy(), rc=pot.info.max_cutoff, types=types_n, list_cutoff=LIST_CUTOFF, vflag=1)
    ev = md.ev.cpu().numpy()
    _close(ev[0] / 27, one["energy"], "energy per cell")
    _close(md.f.cpu().numpy(), np.tile(one["f"], (27, 1)), "forces per atom")
    _close(ev[1:7] / 27, one["virial"], "virial per cell", atol=1e-8)


def _cell_diff(a, b, cell):
    """max |a - b| modulo the lattice (the device driver wraps owned atoms into the cell at every re-neighbouring)"""
    s = (a - b) @ np.linalg.inv(cell)
    return float(np.abs((s - np.round(s)) @ cell).max())


@pytest.mark.gpu
def test_device_resident_nve_in_a_tilted_cell_follows_the_oracle_and_conserves_energy():
    """320 atoms (the tilted 5-atom cell 4x4x4), W_L8, ten 1 fs steps from 300 K, ghosts and list rebuilt on the device
    every 3 steps through the cell path, against the same integrator driven by the oracle through the twin; bounds of
    tests/test_md_gpu.py::test_device_resident_nve_matches_host_driven_loop and the drift bound of its config-1 test"""
    import torch
    from oracle.pyoracle import Oracle
    from lammps_mtp_kokkos_amd.md import DeviceNVE
    path = os.path.join(POT, "W_L8.mtp")
    pos0, cell, types = _cells.tilted5_cell(1)
    pos0, cell, types = _cells.replicate(pos0, cell, types, (4, 4, 4))
    n = len(pos0)
    assert n >= 256
    rng = np.random.default_rng(300)
    vel0 = rng.normal(size=pos0.shape) * np.sqrt(KB * 300.0 / (MASS * MVV2E))
    vel0 -= vel0.mean(0)
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    orc = Oracle(path)

    def cpu_force(p):
        e, f, _, _, _ = _cells.oracle_cell(orc, p, cell, types, eflag=1, vflag=0)
        return f, e

    md = DeviceNVE(ctx, pos0.copy(), cell, rc=pot.info.max_cutoff, mass=MASS, list_cutoff=LIST_CUTOFF, every=3)
    md.v.copy_(torch.from_numpy(vel0))
    eg = []
    for _ in range(10):
        md.step(1e-3)
        eg.append(md.total_energy())
    pos, vel, ec = pos0.copy(), vel0.copy(), []
    f, e = cpu_force(pos)
    for _ in range(10):
        vel = vel + 0.5 * 1e-3 * FTM2V * f / MASS
        pos = pos + 1e-3 * vel
        f, e = cpu_force(pos)
        vel = vel + 0.5 * 1e-3 * FTM2V * f / MASS
        ec.append(e + 0.5 * MVV2E * MASS * (vel ** 2).sum())
    eg, ec = np.array(eg), np.array(ec)
    dx, dv = _cell_diff(md.x.cpu().numpy(), pos, cell), float(np.abs(md.v.cpu().numpy() - vel).max())
    print("builds %d  |dx| %.3e  |dv| %.3e  |dE| %.3e  drift %.3e" % (md.builds, dx, dv, np.abs(eg - ec).max(),
                                                                     np.abs(eg - eg[0]).max()))
    assert md.builds >= 4                                   # re-neighboured on the device along the way
    assert dx < 1e-10 and dv < 1e-9
    assert np.abs(eg - ec).max() < 1e-8
    assert np.abs(eg - eg[0]).max() < 2e-4 * n              # NVE drift over 10 fs, eV


@pytest.mark.gpu
def test_build_cell_error_paths_launch_nothing():
    import torch
    pos, cell, _ = _cells.tilted5_cell()
    far = pos + np.array([3.0, -2.0, 1.0]) @ cell            # a launch would wrap these
    dev, st = _device_stream()
    g = capi.Ghosts(0)
    xa = torch.zeros((4000, 3), dtype=torch.float64, device=dev)
    xa[:5] = torch.from_numpy(far)
    bad = [np.diag([5.0, 5.0, -5.0]), np.zeros((3, 3)), cell[[1, 0, 2]],
           np.array([[5.0, 0, 0], [0, np.nan, 0], [0, 0, 5.0]]), np.array([[5.0, 0, 0], [0, 5.0, np.inf], [0, 0, 5.0]])]
    for c in bad:
        with pytest.raises(capi.MtpError) as ei:
            g.build_cell(xa, 5, c, LIST_CUTOFF, stream=st)
        assert ei.value.code == -20, c
    for c, cut in ((cell, 0.0), (cell, float("nan"))):
        with pytest.raises(capi.MtpError) as ei:
            g.build_cell(xa, 5, c, cut, stream=st)
        assert ei.value.code == -20
    with pytest.raises(capi.MtpError) as ei:
        g.build_cell(xa, 5, cell, LIST_CUTOFF, stream=None)
    assert ei.value.code == -20 and "NULL stream" in str(ei.value)
    torch.cuda.synchronize()
    assert np.array_equal(xa[:5].cpu().numpy(), far) and not xa[5:].any()
    assert g.build_cell(xa, 5, cell, LIST_CUTOFF, stream=st) > 5          # the handle is still good


@pytest.mark.gpu
def test_build_cell_ghost_count_beyond_int_is_refused_not_wrapped():
    """margins so large that owned + ghost atoms come near or beyond 2^31: the count is taken in 64 bits, reported
    exactly while it fits an int (the capacity protocol), refused with INT_MAX when it does not; nothing is allocated"""
    import torch
    dev, st = _device_stream()
    g = capi.Ghosts(0)
    x = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    cell, rghost = np.eye(3), 644.75               # m = 644.75: 1290 or 1291 shifts per direction, depending on s

    def refused(pos):
        x.copy_(torch.from_numpy(np.array([pos])))
        with pytest.raises(capi.MtpError) as ei:
            g.build_cell(x, 1, cell, rghost, stream=st)
        assert ei.value.code == -24
        return g.nall

    assert refused([0.8, 0.85, 0.9]) == 1290 ** 3                       # 2 146 689 000 < 2^31: the exact size
    assert refused([0.3, 0.6, 0.9]) == 2 ** 31 - 1                      # 1291 * 1291 * 1290 > 2^31: not wrapped
    assert refused([0.3, 0.6, 0.2]) == 2 ** 31 - 1
    x.zero_()
    with pytest.raises(capi.MtpError) as ei:                            # a cell of 1e-3 A under a 7 A shell
        g.build_cell(x, 1, 1e-3 * np.eye(3), LIST_CUTOFF, stream=st)
    assert ei.value.code == -24 and g.nall == 2 ** 31 - 1
    with pytest.raises(capi.MtpError):
        g.forward(x, stream=None)
    g.forward(x, stream=st)                                             # the handle holds no ghosts: nothing to do
    torch.cuda.synchronize()
    assert not x.any()
