"""The rows of the first product level kept across the atom loop of the fixed force shape of level 16, on the GPU
(csrc/mtp_wave_body.hpp: row_keep_l1_ct -- each lane's row of the first four blocks of the first product level is loaded
once per wavefront, from the blob, and both passes take those two trips from registers; the gathered ids of a later
tile are indexed by lane & 31 there, gather_lane).  Neither changes a value, a lane or an order, so in deterministic
mode every output is bitwise that of the generic kernel (MTP_FIXED_SHAPE=0, read at every launch).

The system is the 13 x 13 x 13 lattice of tests/test_gpu_fixed_shapes.py (4,394 atoms: the smallest that gets the
twelve-wavefront plan).  Forty of its rows are rewritten to 0, 1, 32, 33 and 65 entries inside the cutoff (no tile, a
padded tile, a full tile, two tiles, three tiles: from the second tile on the ids are gathered), by atoms of their own
listed in that row only; entries outside the cutoff leave in exchange, so the longest row and with it the launch plan
stay.  The cases:
  flags     eflag / vflag 0/0, 1/1 and 3/5;
  range     rows [0, 3552) on the 3,072 wavefronts of the launch: wavefronts of one atom and of two, so what a wavefront
            keeps across its atom loop serves a second atom on some and not on others;
  table     W_L16.mtp loaded with another MTP_BANK_ROUNDS: other packed rows under the same shape and the same kernel
            (last_shape()).  A row taken from anywhere but the blob would show here."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W16 = os.path.join(ROOT, "potentials", "W_L16.mtp")
FORCE = "w16_force_3ps"
RC = 5.0                      # cutoff of the level-16 potential
COUNTS = (0, 1, 32, 33, 65)   # entries inside the cutoff of the rewritten rows
PER_COUNT = 8
FLAGS = [(0, 0), (1, 1), (3, 5)]
RANGE_ROWS = 3552             # more than the 3,072 wavefronts, fewer than twice as many


class _System:
    pass


@pytest.fixture(scope="module")
def system():
    pos, box = mtpgen.bcc_lattice(13, 13, 13, a=3.04, jitter=0.1, seed=31)
    s = periodic_system(pos, box, None, 7.0)
    assert s.nlocal == 4394 and s.nlocal >= 256 * 16
    rng = np.random.default_rng(20261024)
    lengths = np.diff(s.first)
    longest = int(lengths.max())
    assert longest >= max(COUNTS)
    # (a row of the longest length stays as it is: the plan follows it)
    pool = np.flatnonzero(np.arange(s.nlocal) != int(lengths.argmax()))
    chosen = rng.choice(pool, size=PER_COUNT * len(COUNTS), replace=False)
    want = {int(a): COUNTS[k % len(COUNTS)] for k, a in enumerate(chosen)}
    assert sum(1 for a in want if a < RANGE_ROWS) >= 2 * len(COUNTS)
    rows, extra, n_extra = [], [], 0
    for i in range(s.nlocal):
        row = s.neigh[s.first[i]:s.first[i + 1]]
        if i in want:
            k = want[i]
            d = s.x[row] - s.x[s.ilist[i]]
            r2 = (d * d).sum(1)
            assert np.abs(np.sqrt(r2) - RC).min() > 1e-9   # no entry whose side of the cutoff is a matter of rounding
            inn, out = row[r2 <= RC * RC], row[r2 > RC * RC]
            if len(inn) >= k:
                row = np.concatenate([inn[:k], out])
            else:   # added neighbours between 2.3 A and RC - 0.2 A, in this row only
                n_add = k - len(inn)
                u = rng.normal(size=(n_add, 3))
                u /= np.linalg.norm(u, axis=1)[:, None]
                ids = s.x.shape[0] + n_extra + np.arange(n_add)
                extra.append(s.x[s.ilist[i]] + u * rng.uniform(2.3, RC - 0.2, size=n_add)[:, None])
                n_extra += n_add
                row = np.concatenate([inn, ids, out[:longest - k]])
            rng.shuffle(row)
        rows.append(np.asarray(row, np.int32))
    t = _System()
    t.x = np.ascontiguousarray(np.vstack([s.x] + extra))
    t.types = np.concatenate([s.types, np.ones(n_extra, np.int32)]).astype(np.int32)
    t.ilist = np.ascontiguousarray(s.ilist, np.int32)
    t.first = np.zeros(s.nlocal + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=t.first[1:])
    t.neigh = np.concatenate(rows)
    t.nlocal, t.nall, t.want = s.nlocal, t.x.shape[0], want
    assert int(np.diff(t.first).max()) == longest
    # the counts, from the lists as the kernels get them
    owner = np.repeat(np.arange(t.nlocal), np.diff(t.first))
    d = t.x[t.neigh] - t.x[t.ilist[owner]]
    t.counts = np.bincount(owner, weights=(d * d).sum(1) <= RC * RC, minlength=t.nlocal).astype(int)
    assert all(t.counts[i] == k for i, k in want.items())
    rest = np.delete(t.counts, list(want))
    assert rest.min() >= 1 and (rest <= 32).sum() >= 100 and (rest > 32).sum() >= 100
    for a in (t.x, t.types, t.ilist, t.first, t.neigh):
        a.setflags(write=False)
    return t


def _context(pot, s):
    assert pot.info.max_cutoff == RC
    ctx = capi.Context(pot, 0)
    ctx.set_deterministic(True)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    return ctx


@pytest.fixture(scope="module")
def default_table(system):
    """W_L16.mtp as the suites load it (MTP_BANK_ROUNDS=2, tests/conftest.py), one context for all cases"""
    pot = capi.Potential(W16)
    return pot, _context(pot, system)


def _both(ctx, s, monkeypatch, **kw):
    with monkeypatch.context() as m:
        m.delenv("MTP_FIXED_SHAPE", raising=False)
        a = ctx.compute(s.x, s.types, **kw)
        na = ctx.last_shape()
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        b = ctx.compute(s.x, s.types, **kw)
        nb = ctx.last_shape()
    assert na == FORCE and nb == ""
    return a, b


def _bitwise(a, b, what):
    assert np.abs(a["f"]).max() > 1e-3
    for k in a:
        ga, gb = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(ga, gb), (what, k, float(np.abs(ga - gb).max()))


@pytest.mark.parametrize("flags", FLAGS, ids=["e0v0", "e1v1", "e3v5"])
def test_flag_sets_and_neighbour_counts_are_bitwise_the_generic_kernel(system, default_table, monkeypatch, flags):
    s = system
    pot, ctx = default_table
    a, b = _both(ctx, s, monkeypatch, eflag=flags[0], vflag=flags[1])
    info = ctx.launch_info()
    assert info["waves_per_block"] == 12, info
    _bitwise(a, b, "eflag %d vflag %d" % flags)
    lone = [i for i, k in s.want.items() if k == 0]
    assert len(lone) == PER_COUNT
    if flags[0] & 1:
        assert a["energy"] != 0.0
    if flags[0] & 2:   # an atom without neighbours has exactly the species energy
        species = float(pot.tables()["species_coeffs"].reshape(-1)[0])
        assert np.array_equal(a["eatom"][s.ilist[lone]], np.full(len(lone), species))
    if flags[1]:
        assert np.abs(a["virial"]).min() > 0.0


def test_row_range_with_wavefronts_of_one_and_of_two_atoms(system, default_table, monkeypatch):
    import torch
    s = system
    _, ctx0 = default_table
    dev = torch.device("cuda", 0)
    ctx = capi.Context(default_table[0], 0)
    ctx.set_deterministic(True)
    il, fi, ne = (torch.from_numpy(np.array(v, np.int32)).to(dev) for v in (s.ilist, s.first, s.neigh))
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    x = torch.from_numpy(np.array(s.x)).to(dev)
    ty = torch.from_numpy(np.array(s.types, np.int32)).to(dev)

    def run():
        f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
        ev = torch.zeros(8, dtype=torch.float64, device=dev)
        ea = torch.zeros(s.nall, dtype=torch.float64, device=dev)
        va = torch.zeros((s.nall, 6), dtype=torch.float64, device=dev)
        ctx.compute_device_rows(0, RANGE_ROWS, True, x, ty, f, eflag=3, vflag=5, eatom_t=ea, vatom_t=va, ev_t=ev)
        name = ctx.last_shape()
        ctx.synchronize()
        torch.cuda.synchronize()
        return dict(f=f.cpu().numpy(), ev=ev.cpu().numpy(), eatom=ea.cpu().numpy(), vatom=va.cpu().numpy()), name

    with monkeypatch.context() as m:
        m.delenv("MTP_FIXED_SHAPE", raising=False)
        a, na = run()
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        b, nb = run()
    assert na == FORCE and nb == ""
    info = ctx.launch_info()
    waves = info["waves_per_block"] * info["grid_blocks"]
    assert info["waves_per_block"] == 12 and waves < RANGE_ROWS < 2 * waves, info
    _bitwise(a, b, "rows [0, %d)" % RANGE_ROWS)
    assert np.count_nonzero(a["eatom"][s.ilist[:RANGE_ROWS]]) > RANGE_ROWS // 2 and not a["eatom"][s.ilist[RANGE_ROWS:]].any()
    # per-atom energies do not depend on how the rows are dealt to wavefronts: those of the whole call
    whole = ctx0.compute(s.x, s.types, eflag=3, vflag=5)
    assert np.array_equal(a["eatom"][s.ilist[:RANGE_ROWS]], np.asarray(whole["eatom"])[s.ilist[:RANGE_ROWS]])


def test_other_rows_under_the_same_shape_come_from_the_blob(system, default_table, monkeypatch):
    """no bank search numbers the moments differently: other packed rows (the kept ones among them) in the blob, every
    field of the shape and the kernel unchanged"""
    s = system
    with monkeypatch.context() as m:
        m.setenv("MTP_BANK_ROUNDS", "0")
        m.setenv("MTP_BANK_SCALE", "1")
        pot = capi.Potential(W16)
    ctx = _context(pot, s)
    a, b = _both(ctx, s, monkeypatch, eflag=3, vflag=5)
    _bitwise(a, b, "bank rounds 0")
    c = default_table[1].compute(s.x, s.types, eflag=3, vflag=5)
    assert default_table[1].last_shape() == FORCE
    # the same potential to rounding ...
    assert float(np.abs(a["f"] - c["f"]).max()) <= 1e-9 + 1e-10 * max(1.0, float(np.abs(c["f"]).max()))
    # ... and another table: the rows of a level come in another order, the sums of the product passes round differently
    diff = int((np.asarray(a["eatom"]) != np.asarray(c["eatom"])).sum())
    print("atoms whose energy differs in the last bits between the two tables: %d of %d" % (diff, s.nlocal))
    assert diff > 0
