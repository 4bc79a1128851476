"""The geometry axis on the GPU: neighbour-count and distance edges through the force and grade kernels (disjoint
stars, tests/_stars.py) and the device neighbour build on uneven density.

The force kernel's control flow is decided by two numbers per atom, the listed row length L and the in-cutoff count K:
compaction sweeps the row 128 entries at a time, the first NT survivors go straight into the tile arrays and the rest
through cj[], tile 0 is padded to a multiple of NG = 64 / KL, tiles hold NT, single-tile atoms of the persistent layouts
reuse what the first build left, and cnt is checked against cj_cap.  The lattices of the other GPU tests give twenty
values of K and a dozen of L; here every K in {0..5, m NT - 1, m NT, m NT + 1 (m = 1..4)} meets every L in
{K, K + 1, 64, 127, 128, 129, K + 130, 256, 257, 300} in ONE launch, rows in random order, so that a wavefront walks
rows of differing counts one after the other.  Every per-atom output is compared per star with the star's own scale
(_stars.per_star_check: |dF| <= 1e-9 + 1e-10 max(1, max|F_star|), eatom atol 1e-10, vatom and grades with the
constants of tests/test_gpu_parity.py); tests/test_stars_cpu.py shows that the reference's own re-association noise on
these inputs is below 1e-2 of that tolerance (measured: 3.9e-4 at most).

The neighbour build runs on point sets whose cells hold more than two 64-atom chunks, whose 27-cell walks take more than
two candidate batches, with empty cells, ghost-only cells, atoms outside the declared bounds and grids of one and two
cells along an axis; a numpy twin of cell_of asserts that each set has those properties.
"""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import full_neighbor_list
from oracle.pyoracle import Oracle

import _stars
import _tables
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")

# name -> (file or generator, species, grade call, block_lanes KL [, blocks_per_lane NB])
SHIPPED = dict(L8=("W_L8.mtp", 1, False, 16), L16=("W_L16.mtp", 1, False, 32), L20=("WRe_L20.mtp", 2, False, 64),
               L16nbh=("W_L16_nbh.almtp", 1, True, 32), L10cfg=("WRe_L10_cfg.almtp", 2, True, None))
_LOADED = {}


def _pot(name, tmp_pot_dir):
    """(path, species, grade, capi.Potential, Oracle) of a named potential; loaded once per session (the LAYOUT / WPS /
    MAX_WAVES / XCD overrides are read when a context plans, not when the file is loaded)"""
    if name not in _LOADED:
        if name in SHIPPED:
            fn, species, grade, kl = SHIPPED[name]
            path, nb = os.path.join(POT, fn), None
        elif name == "NB2":            # a two-blocks-per-lane table (tests/_tables.py): KL 64, NB 2
            tab, nfac = _tables.make_table(*_tables.shape_table(64, 2, 8))
            path = _tables.write(tab, nfac, str(tmp_pot_dir / "geom_nb2.mtp"))
            species, grade, kl, nb = 1, False, 64, 2
        elif name == "R7nbh":          # R = 7: outside the fused grade path, the candidate-vector kernel builds its own tiles
            p = mtpgen.random_potential(mtpgen.build_table(16), 1, 99, 2.0, 5.0, 7, 1.0)
            mtpgen.add_selection_state(p, "nbh", seed=3)
            path = str(tmp_pot_dir / "geom_r7.almtp")
            mtpgen.write_mtp(p, path)
            species, grade, kl, nb = 1, True, 32, 1
        else:
            raise KeyError(name)
        pot = capi.Potential(path, selection=grade)
        ks = pot.kernel_shape()
        if kl is not None:
            assert ks["block_lanes"] == kl, ks
        if nb is not None:
            assert ks["blocks_per_lane"] == nb, ks
        assert pot.info.max_cutoff == 5.0 and pot.info.min_cutoff == 2.0
        _LOADED[name] = (path, species, grade, pot, Oracle(path, selection=grade))
    return _LOADED[name]


def _env(monkeypatch, layout=None, wps=None, max_waves=None, xcd=None):
    for k, v in (("MTP_LAYOUT", layout), ("MTP_WPS", wps), ("MTP_MAX_WAVES", max_waves), ("MTP_XCD_MAP", xcd)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


LAYOUT_MODE = {"keep": 0, "lean": 1, "rebuild": 2, "rebuild-nodg": 3}


def _context(pot, st, layout=None, wps=None, deterministic=False):
    ctx = capi.Context(pot, 0)
    if deterministic:
        ctx.set_deterministic(True)
    ctx.set_neighbors(st.ilist, st.first, st.neigh, st.nall)
    if layout is not None:
        assert ctx.layout_mode() == LAYOUT_MODE[layout]
    if wps is not None:
        assert ctx.plan_info()["waves_per_simd"] == int(wps)
    return ctx


def _parity(loaded, st, ctx, label):
    path, species, grade, pot, oracle = loaded
    assert _stars.counts(st) == st.KL                    # what the kernel will count is what the case asked for
    got = ctx.compute(st.x, st.types, eflag=3, vflag=4, grade=grade)
    want = oracle.compute(st.x, st.types, st.ilist, st.first, st.neigh, eflag=3, vflag=4, extrapolation=grade,
                          natoms=len(st.ilist))
    worst = _stars.per_star_check(st, got, want, grade, bool(pot.info.configuration_mode), label)
    print("%s: %d stars, %d atoms, worst error / per-star tolerance %s" % (
        label, len(st.ilist), st.nall, " ".join("%s %.2e" % kv for kv in worst.items())))
    return got, want


_NT = {}


def _tile(pot):
    """neighbour tile size NT of the force kernel, from launch_info of a context with a list"""
    if id(pot) not in _NT:
        s = _stars.stars([(1, 1)], np.random.default_rng(0))
        ctx = capi.Context(pot, 0)
        ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
        _NT[id(pot)] = ctx.launch_info()["neighbor_tile"]
    return _NT[id(pot)]


# ---- 2. count edges: K x L in one launch --------------------------------------------------------------------------

# (potential, layout, wps): ids read shape-layout-wps-call
SWEEP = [("L8", None, 2), ("L16", "keep", 2), ("L16", "lean", 2), ("L16", "rebuild", 2), ("L16", "rebuild-nodg", 2),
         ("L16", None, 3), ("L20", None, 2), ("L20", "keep", 2), ("NB2", None, 2),
         ("L16nbh", None, 2), ("L16nbh", None, 3), ("R7nbh", None, 2), ("L10cfg", None, 2)]
SHAPE_ID = dict(L8="KL16", L16="KL32", L20="KL64gather", NB2="KL64xNB2", L16nbh="KL32", R7nbh="KL32", L10cfg="level10")
CALL_ID = dict(L8="force", L16="force", L20="force", NB2="force", L16nbh="grade-fused", R7nbh="grade-unfused",
               L10cfg="grade-cfg")


def _sweep_id(c):
    return "%s-%s-wps%d-%s" % (SHAPE_ID[c[0]], c[1] or "default", c[2], CALL_ID[c[0]])


@pytest.mark.parametrize("seed,order", [(11, "mixed"), (12, "straddle")], ids=["mixed", "straddle"])
@pytest.mark.parametrize("case", SWEEP, ids=_sweep_id)
def test_count_edges_in_one_launch(case, seed, order, monkeypatch, tmp_pot_dir):
    """every K edge x every L edge, one star each, rows in random order, one launch"""
    name, layout, wps = case
    loaded = _pot(name, tmp_pot_dir)
    _env(monkeypatch, layout=layout, wps=wps)
    rng = np.random.default_rng(seed)
    KL = _stars.edge_pairs(_tile(loaded[3]))
    KL = [KL[k] for k in rng.permutation(len(KL))]
    st = _stars.stars(KL, rng, species=loaded[1], order=order)
    ctx = _context(loaded[3], st, layout, wps)
    _parity(loaded, st, ctx, _sweep_id(case) + "-" + order)


def test_count_edges_deterministic_mode(monkeypatch, tmp_pot_dir):
    """fixed-point force accumulation (2^-40 eV/A, |f| < 2^23) over the K x L edges: bitwise equal across calls, within
    the per-star tolerance of the oracle; the shell starts at 3.2 A so that 129 neighbours stay inside its range"""
    loaded = _pot("L16", tmp_pot_dir)
    _env(monkeypatch)
    rng = np.random.default_rng(13)
    KL = _stars.edge_pairs(_tile(loaded[3]))
    KL = [KL[k] for k in rng.permutation(len(KL))]
    st = _stars.stars(KL, rng, rin=(3.2, 5.0))
    ctx = _context(loaded[3], st, deterministic=True)
    got, want = _parity(loaded, st, ctx, "deterministic")
    assert np.abs(want["f"]).max() < 2.0 ** 22
    again = ctx.compute(st.x, st.types, eflag=3, vflag=4)
    for k in ("f", "eatom", "vatom", "virial"):
        assert np.array_equal(got[k], again[k]), k
    assert got["energy"] == again["energy"]


# ---- several rows of differing counts per wavefront ----------------------------------------------------------------

# (potential, wps, MTP_MAX_WAVES, stars wanted, short rows only)
MULTI = [("L8", 2, 1, 1100, False), ("L16", 2, 1, 1100, False), ("L16", 3, 12, 12400, True), ("L20", 2, 1, 1100, False),
         ("L16nbh", 2, 1, 1100, False)]


@pytest.mark.parametrize("xcd", [None, 0], ids=["xcdmap", "noxcdmap"])
@pytest.mark.parametrize("case", MULTI, ids=lambda c: "%s-default-wps%d-%s-maxwaves%d" % (SHAPE_ID[c[0]], c[1], CALL_ID[c[0]], c[2]))
def test_count_edges_several_rows_per_wavefront(case, xcd, monkeypatch, tmp_pot_dir):
    """The same edges with the grid capped (MTP_MAX_WAVES) and the set repeated with fresh shells until every wavefront
    of the persistent grid walks at least four rows: what a three-tile atom leaves behind (tile arrays, padding, parked
    derivatives, coefficient blocks, the ids requested one atom ahead) meets a one-neighbour or empty atom next."""
    name, wps, max_waves, nstars, short = case
    loaded = _pot(name, tmp_pot_dir)
    _env(monkeypatch, wps=wps, max_waves=max_waves, xcd=xcd)
    NT = _tile(loaded[3])
    rng = np.random.default_rng(17 + wps)
    if short:
        KL = [(K, L) for K in _stars.count_edges(NT) for L in sorted({K, K + 1, max(K, 64)})]
    else:
        KL = _stars.edge_pairs(NT)
    KL = KL * (nstars // len(KL) + 1)
    KL = [KL[k] for k in rng.permutation(len(KL))]
    st = _stars.stars(KL, rng, species=loaded[1])
    ctx = _context(loaded[3], st, wps=wps)
    li = ctx.launch_info()
    waves = li["grid_blocks"] * li["waves_per_block"]
    print("grid %d x %d wavefronts, %d rows" % (li["grid_blocks"], li["waves_per_block"], len(st.ilist)))
    assert len(st.ilist) >= 4 * waves, (len(st.ilist), li)
    if xcd is None:
        assert li["grid_blocks"] % 8 == 0 and len(st.ilist) >= 512      # the XCD-aware atom map is really on
    _parity(loaded, st, ctx, "several rows per wavefront")


# ---- cnt == cj_cap ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["L8", "L16", "L20"])
@pytest.mark.parametrize("top", [64, 96])
def test_longest_row_fills_cj_cap_exactly(name, top, monkeypatch, tmp_pot_dir):
    """set_neighbors_device with an honest max_numneigh whose longest row lies wholly inside the cutoff:
    cj_cap = max(64, round32(max_numneigh)) = cnt.  No limit error, parity."""
    import torch
    loaded = _pot(name, tmp_pot_dir)
    path, species, grade, pot, oracle = loaded
    _env(monkeypatch)
    rng = np.random.default_rng(top)
    KL = [(top, top), (1, 1), (top - 1, top), (0, top), (top, top), (33, 40), (0, 0), (top - 1, top - 1), (top, top)]
    st = _stars.stars(KL, rng, species=species, order="mixed")
    assert _stars.counts(st) == KL and int(np.diff(st.first).max()) == top
    dev = torch.device("cuda:0")
    ctx = capi.Context(pot, 0)
    il, fi, ne = (torch.from_numpy(a).to(dev) for a in (st.ilist, st.first, st.neigh))
    ctx.set_neighbors_device(il, fi, ne, st.nall, top)
    x, ty = torch.from_numpy(st.x).to(dev), torch.from_numpy(st.types).to(dev)
    f = torch.zeros((st.nall, 3), dtype=torch.float64, device=dev)
    ea = torch.zeros(st.nall, dtype=torch.float64, device=dev)
    va = torch.zeros((st.nall, 6), dtype=torch.float64, device=dev)
    ev = torch.zeros(8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.compute_device(x, ty, f, eflag=3, vflag=4, eatom_t=ea, vatom_t=va, ev_t=ev)
    ctx.synchronize()                                    # (raises MtpError(LIMIT) if the kernel flagged the row)
    evh = ev.cpu().numpy()
    got = dict(f=f.cpu().numpy(), eatom=ea.cpu().numpy(), vatom=va.cpu().numpy(), energy=float(evh[0]), virial=evh[1:7])
    want = oracle.compute(st.x, st.types, st.ilist, st.first, st.neigh)
    _stars.per_star_check(st, got, want, label="cnt == cj_cap == %d" % top)


# ---- distance edges -------------------------------------------------------------------------------------------------

DISTANCES = dict(exact_cutoff=dict(special="edge"), below_min_dist=dict(rin=(1.0, 5.0)),
                 offset_1e5=dict(offset=(1e5, 1e5, 1e5)), offset_negative=dict(offset=(-731.25, -1e5, -3.5)))


@pytest.mark.parametrize("kind", list(DISTANCES))
@pytest.mark.parametrize("name", ["L16", "L20"])
def test_distance_edges(name, kind, monkeypatch, tmp_pot_dir):
    """exact_cutoff: in every star the LAST survivor of the row sits at r^2 == r_c^2 bit-exact -- inside (the reference
    drops r^2 > r_c^2 only); its value and slope vanish, but it counts: with K = NT + 1 it is the entry that opens tile 1,
    with K a multiple of NG the one that completes a padding group, with K = m NT the one that fills a tile -- and one
    listed atom sits one representable coordinate beyond r_c: outside.  below_min_dist: shells down to 0.5 min_dist (the
    Chebyshev argument leaves [-1, 1]).  offsets: the whole system shifted rigidly; nothing may depend on absolute
    coordinates beyond the rounding of the stored positions, which the oracle sees too."""
    loaded = _pot(name, tmp_pot_dir)
    _env(monkeypatch)
    NT = _tile(loaded[3])
    NG = 64 // loaded[3].kernel_shape()["block_lanes"]
    rng = np.random.default_rng(23)
    KL = _stars.edge_pairs(NT)
    # the exact-cutoff entry as the one that opens a tile / completes a padding group / opens a group that needs padding
    KL += [(NT + 1, L) for L in (NT + 1, NT + 2, 129, 300)] + [(NG, NG), (NG, 129), (4, 4), (4, 130), (NG + 1, 200)]
    KL = [KL[k] for k in rng.permutation(len(KL))]
    for order in ("mixed", "straddle"):
        st = _stars.stars(KL, rng, species=loaded[1], order=order, **DISTANCES[kind])
        if kind == "exact_cutoff":
            d = st.x[st.neigh] - np.repeat(st.x[st.ilist], np.diff(st.first), axis=0)
            assert ((d * d).sum(1) == 25.0).sum() == sum(1 for K, _ in KL if K > 0)
        ctx = _context(loaded[3], st)
        _parity(loaded, st, ctx, "%s %s %s" % (name, kind, order))


# ---- 3. device neighbour build on uneven density ---------------------------------------------------------------------


def _cells(x, cut, lo, hi):
    """numpy twin of cell_of / mtp_build_neighbors_device's grid: (n[3], cell index [nall, 3])"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    n = np.maximum(1, np.ceil((hi - lo) / cut).astype(int))
    inv = 1.0 / cut
    c = np.floor((x - lo) * inv).astype(int)
    return n, np.minimum(np.maximum(c, 0), n - 1)


def _grid_facts(x, inum, cut, lo, hi):
    n, c = _cells(x, cut, lo, hi)
    count = np.zeros(tuple(n), int)
    np.add.at(count, tuple(c.T), 1)
    owned = np.zeros(tuple(n), int)
    np.add.at(owned, tuple(c[:inum].T), 1)
    pad = np.pad(count, 1)
    walk = sum(pad[1 + a:1 + a + n[0], 1 + b:1 + b + n[1], 1 + d:1 + d + n[2]]
               for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1))      # candidates of a cell's 27-cell walk
    return dict(n=tuple(int(v) for v in n), max_cell=int(count.max()), max_walk=int(walk[owned > 0].max()),
                empty_beside_atoms=int(((count == 0) & (walk > 0)).sum()),
                ghost_only=int(((count > 0) & (owned == 0)).sum()),
                outside=int(((x < np.asarray(lo)) | (x > np.asarray(hi))).any(1).sum()))


def _away_from_cutoff(x, inum, cut):
    """no pair within 1e-9 relative of the list cutoff: the kernel tests r^2 <= c^2, the KD-tree r <= c"""
    f_in, _ = full_neighbor_list(x, inum, cut * (1 - 2e-9))
    f_out, _ = full_neighbor_list(x, inum, cut * (1 + 2e-9))
    return np.array_equal(f_in, f_out)


def _thinned_lattice(rng, n3, spacing=2.2, jitter=0.3, keep=0.6):
    """uneven density with a minimum separation (forces stay finite): a jittered grid with sites knocked out"""
    g = np.stack(np.meshgrid(*[np.arange(k) for k in n3], indexing="ij"), -1).reshape(-1, 3) * spacing
    g = g[rng.random(len(g)) < keep]
    return g + rng.uniform(-jitter, jitter, g.shape)


def _point_set(kind, seed):
    """(x, inum, cut, lo, hi, preconditions on _grid_facts) -- owned atoms first, the rest ghosts"""
    rng = np.random.default_rng(seed)
    if kind == "block_and_gas":
        # a compressed block (0.65 / A^3) beside vacuum, a dilute gas over the whole box; owned and ghosts interleaved
        # in space, bounds declared tighter than the gas (atoms beyond them go to the border cells), one gas cell made
        # ghost-only
        cut = 6.0
        x = np.concatenate([rng.uniform(0, 18, (3790, 3)) + np.array([6.5, 12.5, 12.5]),      # (on the cell borders)
                            rng.uniform(0, 1, (360, 3)) * np.array([60.0, 36.0, 36.0])])
        x = x[rng.permutation(len(x))]
        lo, hi = np.array([0.5, 0.5, 0.5]), np.array([59.5, 35.5, 35.5])
        n, c = _cells(x, cut, lo, hi)
        inum = int(0.7 * len(x))
        # the atoms of the least populated non-empty cell go behind the owned ones: a cell holding ghosts only
        flat = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
        pop = np.bincount(flat)
        same = flat == np.flatnonzero(pop == pop[pop > 0].min())[0]
        x = np.concatenate([x[~same], x[same]])
        assert inum <= int((~same).sum())
        need = dict(min_cell=129, min_walk=1537, empty=1, ghost_only=1, outside=1)
    elif kind == "slab_one_cell_z":
        cut = 6.0
        x = _thinned_lattice(rng, (14, 12, 3))
        x[:, 2] *= 0.8
        lo, hi = x.min(0) - 1e-9, x.max(0) + 1e-9
        x = x[rng.permutation(len(x))]
        inum = int(0.8 * len(x))
        need = dict(n_axis=(2, 1))
    elif kind == "rod_one_cell_yz":
        cut = 6.0
        x = _thinned_lattice(rng, (40, 3, 3), keep=0.7)
        lo, hi = x.min(0) - 1e-9, x.max(0) + 1e-9
        x = x[rng.permutation(len(x))]
        inum = int(0.75 * len(x))
        need = dict(n_axis=(1, 1), n_axis2=(2, 1))
    elif kind == "two_cells_x":
        cut = 6.0
        x = _thinned_lattice(rng, (5, 9, 8))
        lo, hi = x.min(0) - 1e-9, x.max(0) + 1e-9
        x = x[rng.permutation(len(x))]
        inum = int(0.6 * len(x))
        need = dict(n_axis=(0, 2))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(x), inum, cut, lo, hi, need


_SETS = {}


def _set(kind):
    """the point set, re-drawn until no pair sits on the list cutoff, with its host list"""
    if kind not in _SETS:
        for seed in range(41, 61):
            x, inum, cut, lo, hi, need = _point_set(kind, seed)
            if _away_from_cutoff(x, inum, cut):
                break
        else:
            raise AssertionError("no draw of %s keeps its pairs away from the list cutoff" % kind)
        first, neigh = full_neighbor_list(x, inum, cut)
        _SETS[kind] = (x, inum, cut, lo, hi, need, first, neigh)
    return _SETS[kind]


def _sorted_rows(first, neigh):
    """every row ascending (rows compared as sets, vectorised)"""
    rows = np.repeat(np.arange(len(first) - 1, dtype=np.int64), np.diff(first))
    return neigh[np.lexsort((neigh, rows))]


NB_PATHS = {"default": {}, "sort": {"MTP_NB_SORT": "1"}, "split1": {"MTP_NB_SPLIT": "1"}, "split4": {"MTP_NB_SPLIT": "4"}}


@pytest.mark.parametrize("path_id", list(NB_PATHS))
@pytest.mark.parametrize("kind", ["block_and_gas", "slab_one_cell_z", "rod_one_cell_yz", "two_cells_x"])
def test_device_neighbour_build_uneven_density(kind, path_id, monkeypatch, tmp_pot_dir):
    """Non-periodic point sets, owned atoms first: the rows of the GPU-built list are exactly the rows of the host
    KD-tree list (as sets), first[] and the reported (entries, longest row) exact.  The preconditions are asserted, not
    measured: block_and_gas has a cell of more than 128 atoms (three chunks in nb_order_cell and in nb_walk_cell's atom
    loop), a 27-cell walk of more than 1 536 candidates (three batches: a row's fill position carries over), an empty cell
    beside a non-empty one, a cell of ghosts only and atoms outside the declared bounds; the other three have grid
    extents of 1 and 2."""
    import torch
    x, inum, cut, lo, hi, need, first, neigh = _set(kind)
    facts = _grid_facts(x, inum, cut, lo, hi)
    print(kind, len(x), "points", inum, "owned", facts, "entries", int(first[-1]), "longest row", int(np.diff(first).max()))
    if "min_cell" in need:
        assert facts["max_cell"] >= need["min_cell"] and facts["max_walk"] >= need["min_walk"]
        assert facts["empty_beside_atoms"] >= need["empty"] and facts["ghost_only"] >= need["ghost_only"]
        assert facts["outside"] >= need["outside"]
    for key in ("n_axis", "n_axis2"):
        if key in need:
            assert facts["n"][need[key][0]] == need[key][1], facts["n"]
    for k in ("MTP_NB_SORT", "MTP_NB_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in NB_PATHS[path_id].items():
        monkeypatch.setenv(k, v)
    loaded = _pot("L8", tmp_pot_dir)
    ctx = capi.Context(loaded[3], 0)
    dev = torch.device("cuda:0")
    xt = torch.from_numpy(x).to(dev)
    total, mx = ctx.build_neighbors_device(xt, inum, len(x), cut, lo, hi)
    got_first, got_neigh = ctx.neighbors_to_host()
    assert total == first[-1] and mx == np.diff(first).max()
    assert np.array_equal(got_first, first)
    assert np.array_equal(_sorted_rows(got_first, got_neigh), _sorted_rows(first, neigh))
    if kind == "slab_one_cell_z" and path_id in ("default", "sort"):
        # forces from the device-built list against the oracle on the host-built list
        types = np.ones(len(x), np.int32)
        f = torch.zeros((len(x), 3), dtype=torch.float64, device=dev)
        ctx.compute_device(xt, torch.from_numpy(types).to(dev), f, eflag=0, vflag=0)
        ctx.synchronize()
        want = loaded[4].compute(x, types, np.arange(inum, dtype=np.int32), first, neigh)
        _close(f.cpu().numpy(), want["f"], "forces from the device-built list")
