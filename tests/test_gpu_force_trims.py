"""The trims of the fixed force shape of level 16 on the GPU (csrc/mtp_wave_body.hpp: sum_t_ct, cnt_sgpr_ct): the six
basic-moment accumulators cross the two neighbour groups in pairs and both halves store, and the neighbour count sits in
an SGPR behind the compaction, so the tile and column tests are scalar branches.  Neither changes an operand or an order
of additions, so in deterministic mode every output is bitwise that of the generic kernel (MTP_FIXED_SHAPE=0, read at
every launch).  The cases are the edges of the compaction and of the tile loop, where a count or a tile width decides a
branch.

The centres are far from one another and their neighbours are atoms of their own, listed in their centre's row only, so
a row's length and its count inside the cutoff are set independently:
  counts   four centres for each count 0, 1, 2, 3 (odd counts take the dummy pad), 31, 32, 33 (one tile against two:
           tile 0 gathered again through cj[] in the force phase), 64, 65 (two and three tiles);
  rows     listed lengths 1, 64, 65, 128, 129 (one half of a chunk, two halves, a second chunk) with counts on either side
           of a tile, shuffled, and rows whose ids inside the cutoff all sit at the list's end;
  pairs    3,552 centres on the 3,072 wavefronts of the twelve-wavefront launch: some wavefronts take one atom and others
           two, so that a single-tile atom follows a three-tile one in the same LDS image and the other way round.
The 'large' variant plans the twelve-wavefront launch, and with it the fixed shapes, for lists this short."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
W16, W16_NBH = os.path.join(POT, "W_L16.mtp"), os.path.join(POT, "W_L16_nbh.almtp")
FORCE, GRADE = "w16_force_3ps", "w16_grade_3ps"
RC = 5.0   # cutoff of the level-16 potentials
FLAGS = [(1, 1), (3, 4), (0, 0)]
COUNTS = (0, 1, 2, 3, 31, 32, 33, 64, 65)
# (listed length, count inside the cutoff, the inside ids at the row's end)
ROWS = [(1, 0, False), (1, 1, False), (64, 9, False), (64, 64, False), (65, 33, False), (65, 65, False), (128, 31, False),
        (128, 70, False), (129, 5, False), (129, 66, False), (129, 5, True), (129, 40, True), (128, 33, True), (65, 1, True),
        (64, 32, True)]
PAIR_CYCLE = (0, 1, 2, 3, 26, 33, 2, 65, 1, 31, 3, 32, 64)
PAIR_ROWS = 3552


class _System:
    pass


def _build(rows, seed):
    """rows: [(listed length, count inside the cutoff, inside ids last)]"""
    rng = np.random.default_rng(seed)
    n = len(rows)
    side = int(np.ceil(np.sqrt(n)))
    grid = np.array([(i % side, i // side, 0) for i in range(n)], np.float64) * 25.0
    centres = grid + rng.uniform(-0.5, 0.5, size=(n, 3))
    total = sum(length for length, _, _ in rows)
    u = rng.normal(size=(total, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = np.empty(total)
    owner = np.repeat(np.arange(n), [length for length, _, _ in rows])
    neigh = np.empty(total, np.int32)
    at = 0
    for length, k, last in rows:
        assert 0 <= k <= length
        r[at:at + k] = rng.uniform(2.3, RC - 0.2, size=k)
        r[at + k:at + length] = rng.uniform(RC + 0.3, RC + 1.5, size=length - k)
        ids = n + at + np.arange(length)
        if last:
            ids = np.concatenate([ids[k:], ids[:k]])
        else:
            rng.shuffle(ids)
        neigh[at:at + length] = ids
        at += length
    s = _System()
    s.x = np.ascontiguousarray(np.vstack([centres, centres[owner] + u * r[:, None]]))
    s.nlocal, s.nall = n, n + total
    s.types = np.ones(s.nall, np.int32)
    s.ilist = np.arange(n, dtype=np.int32)
    s.first = np.zeros(n + 1, np.int32)
    np.cumsum([length for length, _, _ in rows], out=s.first[1:])
    s.neigh = neigh
    s.want = [k for _, k, _ in rows]
    # the counts, from the list as the kernels get it
    d = s.x[s.neigh] - s.x[owner]
    inside = (d * d).sum(1) <= RC * RC
    assert list(np.bincount(owner, weights=inside, minlength=n).astype(int)) == s.want
    for i, (length, k, last) in enumerate(rows):
        if last:
            assert inside[s.first[i + 1] - k:s.first[i + 1]].all() and not inside[s.first[i]:s.first[i + 1] - k].any()
    for a in (s.x, s.types, s.ilist, s.first, s.neigh):
        a.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def counts_system():
    # three entries outside the cutoff beside the neighbours; the first row of count 0 is empty
    rows = [(k + (0 if i == 0 else 3), k, False) for i, k in enumerate(k for k in COUNTS for _ in range(4))]
    s = _build(rows, 20261021)
    assert s.first[1] == 0 and 16 <= s.nlocal <= 64
    return s


@pytest.fixture(scope="module")
def rows_system():
    s = _build(ROWS, 20261022)
    assert sorted(set(int(v) for v in np.diff(s.first))) == [1, 64, 65, 128, 129]
    return s


@pytest.fixture(scope="module")
def pairs_system():
    return _build([(k + 2, k, False) for k in (PAIR_CYCLE[i % len(PAIR_CYCLE)] for i in range(PAIR_ROWS))], 20261023)


def _context(path, s, selection=False):
    pot = capi.Potential(path, selection=selection)
    assert pot.info.max_cutoff == RC
    ctx = capi.Context(pot, 0)
    ctx.set_variant(capi.VARIANT_LARGE)
    ctx.set_deterministic(True)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    return pot, ctx


def _both(ctx, s, monkeypatch, **kw):
    with monkeypatch.context() as m:
        m.delenv("MTP_FIXED_SHAPE", raising=False)
        a = ctx.compute(s.x, s.types, **kw)
        na = ctx.last_shape()
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        b = ctx.compute(s.x, s.types, **kw)
        nb = ctx.last_shape()
    return a, na, b, nb


def _bitwise(a, b, what):
    assert np.abs(a["f"]).max() > 1e-3
    for k in ("f", "eatom", "vatom", "energy", "virial"):
        ga, gb = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(ga, gb), (what, k, float(np.abs(ga - gb).max()))
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def _check(s, a, flags):
    f = np.asarray(a["f"])
    lone = [i for i, k in enumerate(s.want) if k == 0]
    some = [i for i, k in enumerate(s.want) if k > 0]
    assert not f[lone].any() and np.abs(f[some]).max(1).min() > 0.0
    if flags[0] & 1:
        assert a["energy"] != 0.0
    if flags[0] & 2:
        assert np.count_nonzero(a["eatom"][some]) == len(some)
    if flags[1]:
        assert np.abs(a["virial"]).min() > 0.0
    if flags[1] & 4:
        assert np.abs(a["vatom"][some]).max(1).min() > 0.0


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("path", [W16, W16_NBH], ids=["W_L16", "W_L16_nbh"])
def test_neighbour_counts(counts_system, monkeypatch, path, flags):
    s = counts_system
    _, ctx = _context(path, s)
    a, na, b, nb = _both(ctx, s, monkeypatch, eflag=flags[0], vflag=flags[1])
    assert na == FORCE and nb == ""
    _bitwise(a, b, "counts, eflag %d vflag %d" % flags)
    _check(s, a, flags)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("path", [W16, W16_NBH], ids=["W_L16", "W_L16_nbh"])
def test_row_lengths_and_ids_at_the_rows_end(rows_system, monkeypatch, path, flags):
    s = rows_system
    _, ctx = _context(path, s)
    a, na, b, nb = _both(ctx, s, monkeypatch, eflag=flags[0], vflag=flags[1])
    assert na == FORCE and nb == ""
    _bitwise(a, b, "rows, eflag %d vflag %d" % flags)
    _check(s, a, flags)


def test_wavefronts_of_one_and_of_two_atoms(pairs_system, monkeypatch):
    s = pairs_system
    _, ctx = _context(W16, s)
    a, na, b, nb = _both(ctx, s, monkeypatch, eflag=3, vflag=4)
    assert na == FORCE and nb == ""
    info = ctx.launch_info()
    waves = info["waves_per_block"] * info["grid_blocks"]
    assert info["waves_per_block"] == 12 and waves < s.nlocal < 2 * waves, info
    _bitwise(a, b, "one and two atoms a wavefront")
    _check(s, a, (3, 4))


def test_grade_shape_is_untouched(counts_system, monkeypatch):
    s = counts_system
    _, ctx = _context(W16_NBH, s, selection=True)
    a, na, b, nb = _both(ctx, s, monkeypatch, eflag=3, vflag=4, grade=True)
    assert na == GRADE and nb == ""
    assert a["max_grade"] > 0.0 and a["max_grade"] == b["max_grade"]
    _bitwise(a, b, "grade call")
