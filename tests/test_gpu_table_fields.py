"""The product passes with their level bounds as constants of a fixed shape (csrc/mtp_wave_body.hpp: level_ct, level_row,
forward_levels_ct / backward_levels_ct and the leaf sweep), on the GPU: against the oracle at the tolerances of tests/test_gpu_parity.py, and -- where a
fixed-shape kernel runs -- bit for bit against the generic kernel (MTP_FIXED_SHAPE=0) in deterministic mode.

The lists are cut down per atom so that the in-cutoff neighbour counts are exactly 0 (no tile: the product passes run,
the force phase is skipped), 1, 31 (an odd padded tile), 32, 33 (two tiles) and the full shell (50: two tiles); the
entries beyond the cutoff all stay, so the compaction sees them.  Potentials: level 8 (every level a single block: each
trip of two has an idle slot), level 16 (10 | 2 | 1 blocks, 3 leaf blocks) and the two-species level 10 with Mu = 3."""
import dataclasses
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
FORCE, GRADE = "w16_force_3ps", "w16_grade_3ps"
PATTERN = (0, 1, 31, 32, 33, None)   # in-cutoff entries of atom ii: PATTERN[ii % 6] (None: all of them)


def _cut_down(s, rc):
    rows = np.repeat(np.arange(s.nlocal), np.diff(s.first))
    d = s.x[s.neigh] - s.x[s.ilist[rows]]
    inside = (d * d).sum(1) <= rc * rc
    csum = np.concatenate(([0], np.cumsum(inside)))
    rank = csum[1:] - csum[s.first[:-1]][rows]          # 1-based rank of an in-cutoff entry within its row
    full = (csum[s.first[1:]] - csum[s.first[:-1]]).astype(int)
    assert full.min() >= 34, full.min()
    want = np.array([10 ** 9 if p is None else p for p in PATTERN])[np.arange(s.nlocal) % len(PATTERN)]
    keep = ~inside | (rank <= want[rows])
    first = np.concatenate(([0], np.cumsum(np.bincount(rows[keep], minlength=s.nlocal)))).astype(np.int32)
    out = dataclasses.replace(s, first=first, neigh=np.ascontiguousarray(s.neigh[keep]))
    return out, np.minimum(full, want)


def _lattice(n, rc, species, seed):
    """BCC with the fourth shell (24 atoms at 1.658 a) inside the cutoff and the fifth (1.732 a) outside: 50 neighbours"""
    pos, box = mtpgen.bcc_lattice(n, n, n, a=0.59 * rc, jitter=0.03, seed=seed)
    types = np.random.default_rng(seed).integers(1, species + 1, size=len(pos)).astype(np.int32)
    return _cut_down(periodic_system(pos, box, types, 1.4 * rc), rc)


@pytest.fixture(scope="module")
def big():
    """4,394 atoms: more than 256 x 16 rows, so the level-16 launches take the twelve-wavefront plan of the fixed shapes"""
    s, counts = _lattice(13, 5.0, 1, 31)
    assert s.nlocal >= 256 * 16
    return s, counts


_REF = {}


def _reference(name, s, key, **kw):
    """the oracle's result for (potential, system), computed once per module"""
    if (name, key) not in _REF:
        from oracle.pyoracle import Oracle
        sel = name.endswith(".almtp")
        _REF[(name, key)] = Oracle(os.path.join(POT, name), selection=sel).compute(s.x, s.types, s.ilist, s.first, s.neigh, **kw)
    return _REF[(name, key)]


def _close(got, want, what, atol=1e-9, rtol=1e-10):
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)


def _against_oracle(got, want, n, eflag, vflag, what):
    _close(got["f"], want["f"], what + " forces")
    if eflag & 1:
        assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n), what
    if eflag & 2:
        _close(got["eatom"], want["eatom"], what + " eatom", atol=1e-10)
    if vflag & 1:
        _close(got["virial"], want["virial"], what + " virial", atol=1e-8)
    if vflag & 4:
        _close(got["vatom"], want["vatom"], what + " vatom")


def _context(name, s):
    pot = capi.Potential(os.path.join(POT, name), selection=name.endswith(".almtp"))
    ctx = capi.Context(pot, 0)
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
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max()))


def test_the_lists_have_the_neighbour_counts(big):
    s, counts = big
    rc = capi.Potential(os.path.join(POT, "W_L16.mtp")).info.max_cutoff
    assert rc == 5.0
    for k, p in enumerate(PATTERN):
        c = counts[k::len(PATTERN)]
        assert len(c) > 700 and ((c == p).all() if p is not None else (c >= 34).all()), (p, c.min(), c.max())
    assert (np.diff(s.first) > counts).all()   # every row also has entries beyond the cutoff


@pytest.mark.parametrize("name,species", [("W_L8.mtp", 1), ("W_L16.mtp", 1), ("WRe_L10_cfg.almtp", 2)])
@pytest.mark.parametrize("eflag,vflag", [(0, 0), (3, 5)])
def test_generic_kernels_against_the_oracle(name, species, eflag, vflag):
    """128 atoms: the generic kernels (level bounds from the blob's table) behind the new argument-block field"""
    pot = capi.Potential(os.path.join(POT, name), selection=name.endswith(".almtp"))
    s, counts = _lattice(4, pot.info.max_cutoff, species, 7)
    assert set(counts[:5]) == {0, 1, 31, 32, 33}
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    got = ctx.compute(s.x, s.types, eflag=eflag, vflag=vflag)
    assert ctx.last_shape() == ""
    want = _reference(name, s, "small", eflag=3, vflag=5)
    assert np.abs(want["f"]).max() > 1e-3
    _against_oracle(got, want, s.nlocal, eflag, vflag, "%s eflag %d vflag %d" % (name, eflag, vflag))


@pytest.mark.parametrize("eflag,vflag", [(0, 0), (3, 5)])
def test_fixed_force_shape_against_the_oracle_and_the_generic_kernel(big, monkeypatch, eflag, vflag):
    s, _ = big
    _, ctx = _context("W_L16.mtp", s)
    a, na, b, nb = _both(ctx, s, monkeypatch, eflag=eflag, vflag=vflag)
    assert na == FORCE and nb == ""
    _bitwise(a, b, "eflag %d vflag %d" % (eflag, vflag))
    want = _reference("W_L16.mtp", s, "big", eflag=3, vflag=5)
    _against_oracle(a, want, s.nlocal, eflag, vflag, "fixed force shape")
    if eflag & 2:   # atoms without an in-cutoff neighbour: the species energy alone
        assert np.ptp(a["eatom"][s.ilist[0::len(PATTERN)]]) == 0.0


def test_fixed_grade_shape_against_the_oracle_and_the_generic_kernel(big, monkeypatch):
    s, _ = big
    _, ctx = _context("W_L16_nbh.almtp", s)
    a, na, b, nb = _both(ctx, s, monkeypatch, eflag=3, vflag=5, grade=True)
    assert na == GRADE and nb == ""
    assert a["max_grade"] > 0.0 and a["max_grade"] == b["max_grade"]
    _bitwise(a, b, "grade call")
    want = _reference("W_L16_nbh.almtp", s, "big-grade", extrapolation=True, natoms=s.nlocal)
    _close(a["f"], want["f"], "forces (grade call)")
    _close(a["eatom"], want["eatom"], "eatom (grade call)", atol=1e-10)
    _close(a["grades"][s.ilist], want["grades"][s.ilist], "grades", atol=1e-9, rtol=1e-9)
    assert abs(a["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])


def test_a_row_range_takes_the_fixed_kernel_and_agrees(big, monkeypatch):
    import torch
    s, _ = big
    dev = torch.device("cuda", 0)
    pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
    ctx = capi.Context(pot, 0)
    ctx.set_deterministic(True)
    il, fi, ne = (torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(dev) for v in (s.ilist, s.first, s.neigh))
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    x = torch.from_numpy(s.x).to(dev)
    ty = torch.from_numpy(np.ascontiguousarray(s.types, np.int32)).to(dev)
    cut = 1531   # an uneven split (1531 = 6 x 255 + 1: the ranges start on different neighbour counts)

    def run():
        f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
        ev = torch.zeros(8, dtype=torch.float64, device=dev)
        ea = torch.zeros(s.nall, dtype=torch.float64, device=dev)
        kw = dict(eflag=3, vflag=1, eatom_t=ea, ev_t=ev)
        ctx.compute_device_rows(0, cut, False, x, ty, f, **kw)
        names = [ctx.last_shape()]
        ctx.compute_device_rows(cut, s.nlocal - cut, True, x, ty, f, **kw)
        names.append(ctx.last_shape())
        ctx.synchronize()
        torch.cuda.synchronize()
        return dict(f=f.cpu().numpy(), ev=ev.cpu().numpy(), eatom=ea.cpu().numpy()), names

    with monkeypatch.context() as m:
        m.delenv("MTP_FIXED_SHAPE", raising=False)
        a, na = run()
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        b, nb = run()
    assert na == [FORCE, FORCE] and nb == ["", ""]
    _bitwise(a, b, "row ranges")
    want = _reference("W_L16.mtp", s, "big", eflag=3, vflag=5)
    _close(a["f"], want["f"], "forces (row ranges)")
    _close(a["eatom"], want["eatom"], "eatom (row ranges)", atol=1e-10)
