"""Parity of the HIP path (through the C ABI) against the CPU oracle on identical
inputs.  Tolerances (fp64): |dF| <= 1e-9 eV/A + 1e-10 |F|max, |dE|/atom <= 1e-10 eV --
three orders inside the north-star bound of 1e-6 eV/A; the differences come from
re-association (lane-parallel sums, FMA contraction), nothing else.
"""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")


def _oracle(path, selection=False):
    from oracle.pyoracle import Oracle
    return Oracle(path, selection=selection)


def _close(got, want, what, atol=1e-9, rtol=1e-10):
    scale = max(1.0, float(np.abs(want).max())) if np.size(want) else 1.0
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max()) if np.size(want) else 0.0
    assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)
    return err


def _compare(path, s, eflag=3, vflag=4, variant=None, selection=False):
    pot = capi.Potential(path, selection=selection)
    ctx = capi.Context(pot, 0)
    if variant is not None:
        ctx.set_variant(variant)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    got = ctx.compute(s.x, s.types, eflag=eflag, vflag=vflag)
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=eflag, vflag=vflag)
    _close(got["f"], want["f"], "forces")
    n = max(1, len(s.ilist))
    assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n)
    _close(got["eatom"], want["eatom"], "eatom", atol=1e-10)
    _close(got["virial"], want["virial"], "virial", atol=1e-8)
    _close(got["vatom"], want["vatom"], "vatom")
    return got, want, ctx


def _system(ncell, species=1, a=3.165, list_cutoff=7.0, seed=777):
    pos, box = mtpgen.bcc_lattice(*ncell, a=a, seed=seed)
    rng = np.random.default_rng(5)
    types = rng.integers(1, species + 1, size=len(pos)).astype(np.int32)
    return periodic_system(pos, box, types, list_cutoff)


def _pot(tmp, level, species, name):
    tab = mtpgen.level8_template() if level == 8 else mtpgen.build_table(level)
    p = mtpgen.random_potential(tab, species, 4242)
    path = str(tmp / name)
    mtpgen.write_mtp(p, path)
    return path


def test_config1_level8_256_atoms():
    s = _system((4, 4, 8))
    assert s.nlocal == 256
    _compare(os.path.join(POT, "W_L8.mtp"), s)


def test_level16_432_atoms():
    _compare(os.path.join(POT, "W_L16.mtp"), _system((6, 6, 6)))


def test_production_bank_search_effort(monkeypatch):
    """The suites run with two rounds of the LDS-bank search (tests/conftest.py); this one loads the headline potential
    with the shipped effort (eight rounds of four times the proposals for row-per-lane potentials) -- another numbering
    of the moments and another order of the rows inside the levels, same results."""
    monkeypatch.delenv("MTP_BANK_ROUNDS", raising=False)
    monkeypatch.delenv("MTP_BANK_SCALE", raising=False)
    _compare(os.path.join(POT, "W_L16.mtp"), _system((3, 3, 3)))


def test_level20_two_species():
    _compare(os.path.join(POT, "WRe_L20.mtp"), _system((3, 3, 3), species=2))


@pytest.mark.parametrize("level,species", [(4, 1), (6, 1), (10, 3), (12, 2), (14, 1), (18, 1), (22, 1)])   # (level 4: its one product is a leaf row)
def test_other_levels_and_species(tmp_path, level, species):
    # levels 2 and 4 are not loadable by the reference either: its line buffers are sized from the (tiny) table
    # counts and truncate e.g. "alpha_index_times = {}" (pair_mtp.cpp:522-531); the parser here mirrors that
    _compare(_pot(tmp_path, level, species, "p.mtp"), _system((3, 3, 3), species=species))


@pytest.mark.parametrize("no_leaf", [False, True])
def test_schedule_corner_cases_late_writer_and_shared_scalar(tmp_path, monkeypatch, no_leaf):
    """The product schedule on a table real generators do not emit (tests/_mutate.py): a row that adds to a factor
    AFTER never-read scalars used it, and two coefficients on one never-read scalar -- against the oracle's file-order
    loops (pair_mtp.cpp:196-233), with the leaf-row treatment on and off (MTP_NO_LEAF, read when the file is loaded)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _mutate import mutate_mtp
    if no_leaf:
        monkeypatch.setenv("MTP_NO_LEAF", "1")
    for src, level, species in ((os.path.join(POT, "W_L16.mtp"), 16, 1), (_pot(tmp_path, 18, 2, "l18.mtp"), 18, 2)):
        dst = str(tmp_path / ("mut%d.mtp" % level))
        info = mutate_mtp(src, dst)
        assert info["leaves"] > 0
        _compare(dst, _system((3, 3, 3), species))


@pytest.mark.parametrize("prefix", ["core", "tgt", "norows", "rows"])
def test_every_table_blob_prefix(monkeypatch, prefix):
    """The workgroup-shared tables are copied into LDS as one of four prefixes [core | scatter targets | basic
    descriptors | rows + leaf constants]; what is left out is read from HBM / L2 (csrc/mtp_plan.cpp, choose_prefix).  Each
    prefix, forced, against the oracle -- levels 16 (row-per-lane passes) and 20 (gather passes)."""
    monkeypatch.setenv("MTP_BLOB_PREFIX", prefix)
    _compare(os.path.join(POT, "W_L16.mtp"), _system((3, 3, 3)))
    _compare(os.path.join(POT, "WRe_L20.mtp"), _system((3, 3, 3), species=2))


def test_many_in_cutoff_neighbours_multi_tile():
    """compressed lattice: 58 neighbours inside 5 A -> more than one 32-neighbour LDS tile"""
    s = _system((4, 4, 4), a=2.6, list_cutoff=6.0)
    incut = []
    for i in range(s.nlocal):
        js = s.neigh[s.first[i]:s.first[i + 1]]
        incut.append(int((((s.x[js] - s.x[i]) ** 2).sum(1) <= 25.0).sum()))
    assert max(incut) > 32
    _compare(os.path.join(POT, "W_L16.mtp"), s)


def test_ragged_lists_empty_rows_and_subset_ilist():
    s = _system((3, 3, 3))
    rng = np.random.default_rng(9)
    keep = rng.permutation(s.nlocal)[: s.nlocal - 7].astype(np.int32)      # permuted subset
    rows = []
    for ii, i in enumerate(keep):
        r = s.neigh[s.first[i]:s.first[i + 1]].copy()
        rng.shuffle(r)
        if ii % 5 == 0:
            r = r[: len(r) // 3]          # truncated row
        if ii % 11 == 0:
            r = r[:0]                     # atom with no neighbours at all
        r = (r.astype(np.uint32) | np.uint32(int(rng.integers(0, 4)) << 30)).view(np.int32)   # LAMMPS special bits
        rows.append(r)
    first = np.zeros(len(keep) + 1, np.int32)
    first[1:] = np.cumsum([len(r) for r in rows])
    s.ilist, s.first, s.neigh = keep, first, np.concatenate(rows).astype(np.int32)
    _compare(os.path.join(POT, "W_L16.mtp"), s)


@pytest.mark.parametrize("name", ["W_L16.mtp", "WRe_L20.mtp"])
def test_every_row_empty_isolated_atoms(name):
    """No atom has a neighbour and the id array has NO entries at all (pair_mtp.cpp:107-109 with jnum = 0 everywhere):
    site energies are the species coefficients plus the scalars of all-zero moments, forces and virial are zero.  The
    atom loop requests the next atom's ids one atom ahead: an empty row must not make it read them."""
    s = _system((3, 3, 3), species=2 if name.startswith("WRe") else 1)
    s.ilist = np.arange(s.nlocal, dtype=np.int32)
    s.first = np.zeros(s.nlocal + 1, np.int32)
    s.neigh = np.zeros(0, np.int32)
    got, want, _ = _compare(os.path.join(POT, name), s)
    assert not got["f"].any() and not got["virial"].any()


def test_rows_with_neighbours_only_at_the_end_of_the_list():
    """every row empty except the LAST one (the row whose ids sit at the very end of the id array)"""
    s = _system((3, 3, 3))
    last = s.nlocal - 1
    row = s.neigh[s.first[last]:s.first[last + 1]].copy()
    s.ilist = np.arange(s.nlocal, dtype=np.int32)
    first = np.zeros(s.nlocal + 1, np.int32)
    first[-1] = len(row)
    s.first, s.neigh = first, row
    _compare(os.path.join(POT, "W_L16.mtp"), s)


def test_empty_ilist():
    s = _system((2, 2, 2))
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32), s.nall)
    r = ctx.compute(s.x, s.types)
    assert r["energy"] == 0 and not r["f"].any()


def test_lammps_form_neighbor_list_and_accumulate_semantics():
    s = _system((3, 3, 3))
    path = os.path.join(POT, "W_L16.mtp")
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    numneigh = np.zeros(s.nall, np.int32)
    rows = [np.zeros(0, np.int32)] * s.nall
    for ii, i in enumerate(s.ilist):
        rows[i] = s.neigh[s.first[ii]:s.first[ii + 1]]
        numneigh[i] = len(rows[i])
    ctx.set_neighbors_lammps(s.ilist, numneigh, rows, s.nall)
    a = ctx.compute(s.x, s.types)
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(a["f"], want["f"], "forces")
    # f/virial/energy accumulate into what the caller passes; eatom is assigned
    import ctypes as C
    f = np.full((s.nall, 3), 0.5)
    e = C.c_double(10.0)
    vir = np.full(6, 2.0)
    eatom = np.full(s.nall, -7.0)
    rc = capi.lib().mtp_compute(ctx.h, s.x.ctypes.data_as(C.POINTER(C.c_double)),
                                s.types.ctypes.data_as(C.POINTER(C.c_int)), 3, 1, 0,
                                f.ctypes.data_as(C.POINTER(C.c_double)), eatom.ctypes.data_as(C.POINTER(C.c_double)),
                                None, C.byref(e), vir.ctypes.data_as(C.POINTER(C.c_double)), None, None, None)
    assert rc == 0
    _close(f - 0.5, want["f"], "accumulated forces")
    assert abs(e.value - 10.0 - want["energy"]) < 1e-8
    _close(vir - 2.0, want["virial"], "virial", atol=1e-8)
    _close(eatom[: s.nlocal], want["eatom"][: s.nlocal], "eatom")
    assert (eatom[s.nlocal:] == -7.0).all()          # ghosts untouched (pair_mtp.cpp:210)


def test_flags_off_leave_outputs_untouched():
    s = _system((3, 3, 3))
    path = os.path.join(POT, "W_L8.mtp")
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    r = ctx.compute(s.x, s.types, eflag=0, vflag=0)
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=0, vflag=0)
    _close(r["f"], want["f"], "forces")
    assert r["energy"] == 0 and not r["eatom"].any() and not r["virial"].any() and not r["vatom"].any()
    r = ctx.compute(s.x, s.types, eflag=1, vflag=2)          # global only
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=1, vflag=2)
    assert abs(r["energy"] - want["energy"]) < 1e-9
    _close(r["virial"], want["virial"], "virial", atol=1e-8)
    assert not r["eatom"].any() and not r["vatom"].any()


def test_species_outside_potential_is_reported():
    s = _system((3, 3, 3))
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    t = s.types.copy()
    t[5] = 2
    with pytest.raises(capi.MtpError, match="Too few species") as ei:
        ctx.compute(s.x, t)
    assert ei.value.code == -22
    ctx.compute(s.x, s.types)                      # the context stays usable


def test_compute_before_neighbors_is_an_error():
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    ctx = capi.Context(pot, 0)
    with pytest.raises(capi.MtpError) as ei:
        ctx.nall = 1
        ctx.compute(np.zeros((1, 3)), np.ones(1, np.int32))
    assert ei.value.code == -23


def test_variants_agree():
    s = _system((4, 4, 4))
    path = os.path.join(POT, "W_L16.mtp")
    a, _, ca = _compare(path, s, variant=capi.VARIANT_LARGE)
    b, _, cb = _compare(path, s, variant=capi.VARIANT_SMALL)
    assert cb.launch_info()["waves_per_block"] == 1
    _close(a["f"], b["f"], "variant forces", atol=1e-10)


def test_device_pointer_path_matches_host_path():
    import torch
    s = _system((4, 4, 4))
    path = os.path.join(POT, "W_L16.mtp")
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    dev = torch.device("cuda:0")
    il = torch.from_numpy(s.ilist).to(dev)
    fi = torch.from_numpy(s.first).to(dev)
    ne = torch.from_numpy(s.neigh).to(dev)
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    x = torch.from_numpy(s.x).to(dev)
    ty = torch.from_numpy(s.types).to(dev)
    f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    ea = torch.zeros(s.nall, dtype=torch.float64, device=dev)
    va = torch.zeros((s.nall, 6), dtype=torch.float64, device=dev)
    ev = torch.zeros(8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream    # null handle under pytest: the context's own stream (synchronised above)
    for _ in range(2):                                   # forces accumulate over calls
        ctx.compute_device(x, ty, f, eflag=3, vflag=4, eatom_t=ea, vatom_t=va, ev_t=ev, stream=st)
    ctx.synchronize(st)
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(f.cpu().numpy() / 2, want["f"], "device forces")
    _close(ev.cpu().numpy()[0] / 2, want["energy"], "device energy", atol=1e-8)
    _close(ev.cpu().numpy()[1:7] / 2, want["virial"], "device virial", atol=1e-8)
    _close(ea.cpu().numpy(), want["eatom"], "device eatom")


def test_step_is_capturable_in_a_hip_graph():
    """The device path only launches kernels on the caller's stream (no allocation, copy or synchronisation after the
    first call), so a caller can capture zero + force call + tally fold in a HIP graph; the replays must reproduce the
    oracle.  (Measured on MI355X / ROCm 7.2: replaying is slower than launching -- bench.py --graph --, so the bench
    does not use it by default.)"""
    import torch
    s = _system((4, 4, 4))
    path = os.path.join(POT, "W_L16.mtp")
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    dev = torch.device("cuda:0")
    il, fi, ne = (torch.from_numpy(a).to(dev) for a in (s.ilist, s.first, s.neigh))
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    x = torch.from_numpy(s.x).to(dev)
    ty = torch.from_numpy(s.types).to(dev)
    f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    ev = torch.zeros(8, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def step(st):
        capi.zero_async(f, st)
        ctx.compute_device(x, ty, f, eflag=1, vflag=1, ev_t=ev, stream=st)

    with torch.cuda.stream(side):
        step(side.cuda_stream)                       # first call: buffers, kernel attributes
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step(side.cuda_stream)
        ev.zero_()
        for _ in range(3):
            graph.replay()
        side.synchronize()
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(f.cpu().numpy(), want["f"], "forces of the replayed step")
    assert abs(float(ev[0].item()) / 3 - want["energy"]) <= 1e-10 * max(1.0, abs(want["energy"]))


def test_understated_max_numneigh_is_reported_not_overrun():
    """mtp_set_neighbors_device sizes an LDS array from the caller's max_numneigh; a row with more in-cutoff
    neighbours than that must end in MTP_ERR_LIMIT, not in an LDS overrun."""
    import torch
    s = _system((4, 4, 4), a=2.2, list_cutoff=6.0)      # ~100 neighbours inside the 5 A cutoff
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    ctx = capi.Context(pot, 0)
    dev = torch.device("cuda:0")
    il, fi, ne = (torch.from_numpy(a).to(dev) for a in (s.ilist, s.first, s.neigh))
    ctx.set_neighbors_device(il, fi, ne, s.nall, 8)      # declares 8: the id array holds 64
    x = torch.from_numpy(s.x).to(dev)
    ty = torch.from_numpy(s.types).to(dev)
    f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    ctx.compute_device(x, ty, f, eflag=0, vflag=0)
    with pytest.raises(capi.MtpError) as ei:
        ctx.synchronize()
    assert ei.value.code == -24
    # the same list with an honest declaration works
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    f.zero_()
    ctx.compute_device(x, ty, f, eflag=0, vflag=0)
    ctx.synchronize()
    want = _oracle(os.path.join(POT, "W_L8.mtp")).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(f.cpu().numpy(), want["f"], "forces after re-declaring")


def _rows_as_sets(first, neigh):
    return [np.sort(neigh[first[i]:first[i + 1]]) for i in range(len(first) - 1)]


@pytest.mark.parametrize("ncell,a,cut,sort_path", [((4, 4, 4), 3.165, 7.0, False), ((3, 4, 5), 2.9, 5.5, False),
                                                   ((2, 2, 2), 3.165, 7.0, False), ((3, 4, 5), 2.9, 5.5, True),
                                                   ((6, 6, 6), 3.165, 3.0, False)])
def test_device_neighbour_build_matches_host_list(ncell, a, cut, sort_path, monkeypatch):
    """the GPU-built full list holds, row by row, exactly the atoms of the host KD-tree list
    (integer work: compared as sets, bit-exact), and forces computed from it match the oracle.  sort_path: the
    placement by a stable radix sort that grids above 65,536 cells take (MTP_NB_SORT); the 3 A case has cells with
    very few atoms and many cells."""
    import torch
    if sort_path:
        monkeypatch.setenv("MTP_NB_SORT", "1")
    s = _system(ncell, a=a, list_cutoff=cut)
    path = os.path.join(POT, "W_L8.mtp")
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(s.x).to(dev)
    lo, hi = s.x.min(0) - 1e-9, s.x.max(0) + 1e-9
    total, mx = ctx.build_neighbors_device(x, s.nlocal, s.nall, cut, lo, hi)
    first, neigh = ctx.neighbors_to_host()
    assert total == s.first[-1] and mx == np.diff(s.first).max()
    assert np.array_equal(first, s.first)
    for got, want in zip(_rows_as_sets(first, neigh), _rows_as_sets(s.first, s.neigh)):
        assert np.array_equal(got, want)
    ty = torch.from_numpy(s.types).to(dev)
    f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    ctx.compute_device(x, ty, f, eflag=0, vflag=0)
    ctx.synchronize()
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(f.cpu().numpy(), want["f"], "forces from the device-built list")
    # rebuilding after the atoms moved gives the list of the new positions
    rng = np.random.default_rng(11)
    x2 = s.x + rng.normal(0, 0.2, s.x.shape)
    from lammps_mtp_kokkos_amd.driver import full_neighbor_list
    f2, n2 = full_neighbor_list(x2, s.nlocal, cut)
    xt2 = torch.from_numpy(x2).to(dev)
    ctx.build_neighbors_device(xt2, s.nlocal, s.nall, cut, x2.min(0), x2.max(0))
    first2, neigh2 = ctx.neighbors_to_host()
    assert np.array_equal(first2, f2)
    for got, want in zip(_rows_as_sets(first2, neigh2), _rows_as_sets(f2, n2)):
        assert np.array_equal(got, want)


def test_device_neighbour_build_empty_and_single():
    import torch
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    ctx = capi.Context(pot, 0)
    dev = torch.device("cuda:0")
    x = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    total, mx = ctx.build_neighbors_device(x, 1, 1, 5.0, [0, 0, 0], [0, 0, 0])
    assert (total, mx) == (0, 0)
    first, neigh = ctx.neighbors_to_host()
    assert first.tolist() == [0, 0] and len(neigh) == 0
    total, mx = ctx.build_neighbors_device(x, 0, 1, 5.0, [0, 0, 0], [0, 0, 0])   # ghosts only
    assert (total, mx) == (0, 0)


def test_golden_fixtures():
    gdir = os.path.join(ROOT, "tests", "golden")
    names = sorted(f for f in os.listdir(gdir) if f.endswith(".npz"))
    assert names
    for n in names:
        g = np.load(os.path.join(gdir, n))
        path = os.path.join(POT, str(g["potential"]))
        pot = capi.Potential(path)
        ctx = capi.Context(pot, 0)
        ctx.set_neighbors(g["ilist"], g["first"], g["neigh"], len(g["x"]))
        r = ctx.compute(g["x"], g["types"])
        _close(r["f"], g["f"], n + " forces")
        _close(r["eatom"], g["eatom"], n + " eatom")
        _close(r["virial"], g["virial"], n + " virial", atol=1e-8)
        assert abs(r["energy"] - float(g["energy"])) <= 1e-10 * len(g["ilist"]) * max(1, abs(float(g["energy"])) / len(g["ilist"]))


def test_config2_size_properties_64k_atoms():
    """BASELINE config 2 at full size: properties that need no CPU pass over all atoms
    (sum F = 0 after the ghost fold, E = sum eatom, virial = sum vatom) plus oracle
    parity of the site energies of a 512-atom sample."""
    pos, box = mtpgen.bcc_lattice(32, 32, 32)
    s = periodic_system(pos, box, None, 7.0)
    assert s.nlocal == 65536
    path = os.path.join(POT, "W_L16.mtp")
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    r = ctx.compute(s.x, s.types)
    F = s.fold_forces(r["f"])
    assert np.abs(F.sum(0)).max() < 1e-7
    assert abs(r["energy"] - r["eatom"][: s.nlocal].sum()) < 1e-6
    _close(r["vatom"][: s.nlocal].sum(0), r["virial"], "virial sum", atol=1e-6)
    pick = np.random.default_rng(0).choice(s.nlocal, 512, replace=False).astype(np.int32)
    first = np.zeros(513, np.int32)
    first[1:] = np.cumsum(s.first[pick + 1] - s.first[pick])
    neigh = np.concatenate([s.neigh[s.first[i]:s.first[i + 1]] for i in pick])
    want = _oracle(path).compute(s.x, s.types, pick, first, neigh)
    _close(r["eatom"][pick], want["eatom"][pick], "sampled eatom")
    # translation of the whole crystal changes nothing
    r2 = ctx.compute(s.x + np.array([0.37, -1.1, 2.2]), s.types)
    _close(r2["f"], r["f"], "translated forces", atol=1e-8)


# ---- MaxVol extrapolation grades (pair_style mtp/extrapolation) -------------------------------------


def _grade_compare(path, s, natoms=None):
    pot = capi.Potential(path, selection=True)
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    got = ctx.compute(s.x, s.types, grade=True)
    want = _oracle(path, selection=True).compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True,
                                                 natoms=natoms or s.nlocal)
    _close(got["f"], want["f"], "forces (grade call)")
    _close(got["eatom"], want["eatom"], "eatom (grade call)", atol=1e-10)
    return pot, got, want


def test_neighbourhood_grades_level16():
    s = _system((4, 4, 4))
    pot, got, want = _grade_compare(os.path.join(POT, "W_L16_nbh.almtp"), s)
    assert not pot.info.configuration_mode
    _close(got["grades"][s.ilist], want["grades"][s.ilist], "grades", atol=1e-9, rtol=1e-9)
    assert abs(got["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])
    assert not got["grades"][s.nlocal:].any()          # ghosts untouched


def test_neighbourhood_grades_two_species_multi_tile(tmp_path):
    tab = mtpgen.build_table(10)
    p = mtpgen.random_potential(tab, 2, 77)
    mtpgen.add_selection_state(p, "nbh", seed=5)
    path = str(tmp_path / "nbh2.almtp")
    mtpgen.write_mtp(p, path)
    s = _system((4, 4, 4), species=2, a=2.6, list_cutoff=6.0)      # > 32 in-cutoff neighbours
    pot, got, want = _grade_compare(path, s)
    _close(got["grades"][s.ilist], want["grades"][s.ilist], "grades", atol=1e-9, rtol=1e-9)
    assert abs(got["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])


def test_configuration_mode_candidate_vector():
    s = _system((3, 3, 3), species=2)
    path = os.path.join(POT, "WRe_L10_cfg.almtp")
    pot, got, want = _grade_compare(path, s)
    assert pot.info.configuration_mode
    _close(got["coeff_ders"], want["coeff_ders"], "sum_i dE_i/dtheta", atol=1e-9, rtol=1e-10)
    g = pot.cfg_grade(got["coeff_ders"]) / s.nlocal                 # compile_grades, :369-376
    assert abs(g - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])


def test_grades_general_path_matches_fused_path(monkeypatch):
    """Shapes outside the fused case (R != 8, Mu > 4, more than two species) leave the adjoints of the basics in
    HBM for mtp_cvec_kernel; MTP_GRADE_UNFUSED forces that path for a shape both can run."""
    s = _system((3, 3, 3))
    path = os.path.join(POT, "W_L16_nbh.almtp")
    monkeypatch.setenv("MTP_GRADE_UNFUSED", "1")
    pot, got, want = _grade_compare(path, s)
    _close(got["grades"][s.ilist], want["grades"][s.ilist], "grades (general path)", atol=1e-9, rtol=1e-9)
    monkeypatch.delenv("MTP_GRADE_UNFUSED")
    pot2, got2, _ = _grade_compare(path, s)
    _close(got2["grades"][s.ilist], got["grades"][s.ilist], "fused vs general", atol=1e-9, rtol=1e-9)


def test_grades_without_selection_state_is_an_error():
    s = _system((2, 2, 2))
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    with pytest.raises(capi.MtpError) as ei:
        ctx.compute(s.x, s.types, grade=True)
    assert ei.value.code == -23


def test_golden_grades():
    gdir = os.path.join(ROOT, "tests", "golden")
    for n in ("W_L16_nbh_16.npz", "WRe_L10_cfg_16.npz"):
        g = np.load(os.path.join(gdir, n))
        pot = capi.Potential(os.path.join(POT, str(g["potential"])), selection=True)
        ctx = capi.Context(pot, 0)
        ctx.set_neighbors(g["ilist"], g["first"], g["neigh"], len(g["x"]))
        r = ctx.compute(g["x"], g["types"], grade=True)
        _close(r["f"], g["f"], n + " forces")
        if pot.info.configuration_mode:
            _close(r["coeff_ders"], g["coeff_ders"], n + " coeff_ders", rtol=1e-10)
        else:
            _close(r["grades"], g["grades"], n + " grades", rtol=1e-9)
            assert abs(r["max_grade"] - float(g["max_grade"])) <= 1e-9 * max(1.0, float(g["max_grade"]))


def test_deterministic_mode_is_bitwise_reproducible():
    """mtp_context_set_deterministic: fixed-point force accumulation -> the same bits on every call (the default fp64
    atomics agree to rounding only), still within tolerance of the oracle."""
    s = _system((5, 5, 5))
    path = os.path.join(POT, "W_L16.mtp")
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    ctx.set_deterministic(True)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    runs = [ctx.compute(s.x, s.types) for _ in range(4)]
    for r in runs[1:]:
        assert np.array_equal(r["f"], runs[0]["f"])
        assert r["energy"] == runs[0]["energy"] and np.array_equal(r["virial"], runs[0]["virial"])
        assert np.array_equal(r["eatom"], runs[0]["eatom"]) and np.array_equal(r["vatom"], runs[0]["vatom"])
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(runs[0]["f"], want["f"], "deterministic forces")
    ctx.set_deterministic(False)
    _close(ctx.compute(s.x, s.types)["f"], runs[0]["f"], "atomic vs fixed-point forces", atol=1e-10)


# ---- LAMMPS-KOKKOS list views (mtp_set_neighbors_device_2d) and the NULL-stream rule -------------------------------

@pytest.mark.parametrize("layout", ["left", "right"])
def test_kokkos_2d_neighbour_view_both_layouts(layout):
    """The list as the reference's /kk styles read it on the device -- d_ilist(ii), d_numneigh(i), padded 2-D view
    d_neighbors(i, jj) (/root/reference/LAMMPS/KOKKOS/pair_mtp_kokkos.cpp:236-239, pair_mtp_kokkos.h:115) -- in both
    Kokkos layouts, with a permuted subset ilist, ragged / empty rows, special-bond bits in the entries and garbage in
    the padding; compacted on the device, then forces / energies / virials against the oracle on the same list."""
    import torch
    s = _system((4, 4, 4))
    rng = np.random.default_rng(31)
    keep = rng.permutation(s.nlocal)[: s.nlocal - 9].astype(np.int32)
    numneigh = np.zeros(s.nall, np.int32)                         # indexed by atom id, as in LAMMPS
    maxn = int(np.diff(s.first).max()) + 5                        # extent(1) of the view: longer than any row
    view = rng.integers(0, s.nall, size=(s.nall, maxn)).astype(np.int32)      # padding = garbage
    rows = {}
    for ii, i in enumerate(keep):
        r = s.neigh[s.first[i]:s.first[i + 1]].copy()
        rng.shuffle(r)
        if ii % 7 == 0:
            r = r[: len(r) // 2]
        if ii % 13 == 0:
            r = r[:0]
        r = (r.astype(np.uint32) | np.uint32(int(rng.integers(0, 4)) << 30)).view(np.int32)   # LAMMPS special bits
        rows[int(i)] = r
        numneigh[i] = len(r)
        view[i, : len(r)] = r
    dev = torch.device("cuda:0")
    stream = capi.use_private_torch_stream(dev)
    if layout == "left":                                          # Kokkos::LayoutLeft: (i, jj) at i + jj * extent(0)
        flat = torch.from_numpy(np.ascontiguousarray(view.T).ravel()).to(dev)
        stride_i, stride_jj = 1, s.nall
    else:                                                         # LayoutRight: (i, jj) at i * extent(1) + jj
        flat = torch.from_numpy(view.ravel().copy()).to(dev)
        stride_i, stride_jj = maxn, 1
    path = os.path.join(POT, "W_L16.mtp")
    ctx = capi.Context(capi.Potential(path), 0)
    il = torch.from_numpy(keep).to(dev)
    nn = torch.from_numpy(numneigh).to(dev)
    ctx.set_neighbors_device_2d(il, nn, flat, stride_i, stride_jj, maxn, s.nall, stream=stream.cuda_stream)
    first = np.zeros(len(keep) + 1, np.int32)
    first[1:] = np.cumsum([len(rows[int(i)]) for i in keep])
    neigh = np.concatenate([rows[int(i)] for i in keep]).astype(np.int32)
    got_first, got_neigh = ctx.neighbors_to_host()
    assert np.array_equal(got_first, first) and np.array_equal(got_neigh, neigh)         # integer work: bit-exact
    x = torch.from_numpy(s.x).to(dev)
    ty = torch.from_numpy(s.types).to(dev)
    f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    ea = torch.zeros(s.nall, dtype=torch.float64, device=dev)
    ev = torch.zeros(8, dtype=torch.float64, device=dev)
    ctx.compute_device(x, ty, f, eflag=3, vflag=1, eatom_t=ea, ev_t=ev, stream=stream.cuda_stream)
    ctx.synchronize(stream.cuda_stream)
    want = _oracle(path).compute(s.x, s.types, keep, first, neigh, eflag=3, vflag=1)
    _close(f.cpu().numpy(), want["f"], "forces from the 2-D view")
    _close(ea.cpu().numpy(), want["eatom"], "eatom", atol=1e-10)
    evh = ev.cpu().numpy()
    assert abs(evh[0] - want["energy"]) <= 1e-10 * len(keep) * max(1.0, abs(want["energy"]) / len(keep))
    _close(evh[1:7], want["virial"], "virial", atol=1e-8)
    # a row longer than the view's second extent is refused, not read
    numneigh[keep[3]] = maxn + 1
    with pytest.raises(capi.MtpError) as e:
        ctx.set_neighbors_device_2d(il, torch.from_numpy(numneigh).to(dev), flat, stride_i, stride_jj, maxn, s.nall,
                                    stream=stream.cuda_stream)
    assert e.value.code == -20


def test_null_stream_rule():
    """include/mtp_mi355x.h "Streams": entry points with a context map NULL to the context's stream; those without one
    (halo, ghosts, nve, zero) reject NULL instead of falling onto the legacy null stream."""
    import ctypes as C
    import torch
    from lammps_mtp_kokkos_amd.domain import decompose
    L = capi.lib()
    dev = torch.device("cuda:0")
    t = torch.zeros(64, dtype=torch.float64, device=dev)
    assert L.mtp_zero_async(None, C.c_void_p(t.data_ptr()), C.c_longlong(64)) == -20
    pos, box = mtpgen.bcc_lattice(8, 8, 8)
    plan = decompose(pos, box, None, 1, 0, 7.0, with_lists=False)
    halo = capi.Halo(plan, 0, None)
    x = torch.from_numpy(plan.x0).to(dev)
    for call in (halo.forward_begin, halo.forward, halo.reverse, lambda a, st: halo.pack_forward(a, st),
                 lambda a, st: halo.unpack_reverse(a, st)):
        with pytest.raises(capi.MtpError) as e:
            call(x, None)
        assert e.value.code == -20 and "NULL stream" in str(e.value)
    g = capi.Ghosts(0)
    with pytest.raises(capi.MtpError) as e:
        g.build(x, plan.nlocal, box, 7.0, stream=None)
    assert e.value.code == -20
    iv = torch.zeros(1, dtype=torch.float64, device=dev)
    ty = torch.ones(plan.nall, dtype=torch.int32, device=dev)
    with pytest.raises(capi.MtpError):
        capi.nve_final(plan.nlocal, x, x, ty, iv, 0.0, stream=None)
    # with a context NULL is the context's stream: a whole call runs and synchronises on it
    s = _system((3, 3, 3))
    path = os.path.join(POT, "W_L8.mtp")
    ctx = capi.Context(capi.Potential(path), 0)
    il, fi, ne = (torch.from_numpy(a).to(dev) for a in (s.ilist, s.first, s.neigh))
    torch.cuda.synchronize()
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    xs = torch.from_numpy(s.x).to(dev)
    tys = torch.from_numpy(s.types).to(dev)
    f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.compute_device(xs, tys, f, stream=None)
    ctx.synchronize(None)
    want = _oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh)
    _close(f.cpu().numpy(), want["f"], "forces on the context's own stream")
