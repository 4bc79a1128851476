"""The basic-moment pass in five-factor blocks on the GPU (csrc/mtp_wave_body.hpp, fwd5_ct): the fixed force shape of
level 16 reads ten rows a column into six accumulators where the generic kernels (and the grade shape) read twelve into
nine, and every basic moment stays the same sum over the same columns -- in deterministic mode the outputs are bitwise
those of the generic kernel (MTP_FIXED_SHAPE=0, read at every launch).

36 centre atoms far from one another, four for each in-cutoff neighbour count 0, 1, 2, 3, 31, 32, 33, 64, 65: the pass
walks the two neighbour groups of a tile column by column, so the odd counts end in a padded column, 31 / 32 / 33 sit on
the tile edge and 64 / 65 are two and three tiles.  The neighbours are atoms of their own, listed in their centre's row
only, with three entries outside the cutoff beside them (one row of count 0 is empty).  The 'large' variant plans the
twelve-wavefront launch, and with it the fixed shapes, for a list this short."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
W16, W16_NBH = os.path.join(POT, "W_L16.mtp"), os.path.join(POT, "W_L16_nbh.almtp")
FORCE, GRADE = "w16_force_3ps", "w16_grade_3ps"
COUNTS = (0, 1, 2, 3, 31, 32, 33, 64, 65)
RC = 5.0   # cutoff of the level-16 potentials


class _System:
    pass


@pytest.fixture(scope="module")
def system():
    for path in (W16, W16_NBH):
        assert capi.Potential(path).info.max_cutoff == RC
    rng = np.random.default_rng(20261020)
    want = [k for k in COUNTS for _ in range(4)]
    n = len(want)
    grid = np.array([(i % 6, (i // 6) % 6, 0) for i in range(n)], np.float64) * 25.0
    xs, rows = [grid + rng.uniform(-0.5, 0.5, size=(n, 3))], []
    nall = n
    for i, k in enumerate(want):
        n_out = 0 if i == 0 else 3
        u = rng.normal(size=(k + n_out, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        r = np.concatenate([rng.uniform(2.3, RC - 0.2, size=k), rng.uniform(RC + 0.3, RC + 1.5, size=n_out)])
        xs.append(xs[0][i] + u * r[:, None])
        row = nall + np.arange(k + n_out)
        rng.shuffle(row)
        rows.append(row.astype(np.int32))
        nall += k + n_out
    s = _System()
    s.x = np.ascontiguousarray(np.vstack(xs))
    s.types = np.ones(nall, np.int32)
    s.ilist = np.arange(n, dtype=np.int32)
    s.first = np.zeros(n + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=s.first[1:])
    s.neigh = np.concatenate(rows).astype(np.int32)
    s.nlocal, s.nall, s.want = n, nall, want
    # the counts, from the list as the kernels get it
    owner = np.repeat(np.arange(n), np.diff(s.first))
    d = s.x[s.neigh] - s.x[owner]
    counts = np.bincount(owner, weights=(d * d).sum(1) <= RC * RC, minlength=n).astype(int)
    assert list(counts) == want and 16 <= n <= 64 and s.first[1] == 0
    for a in (s.x, s.types, s.ilist, s.first, s.neigh):
        a.setflags(write=False)
    return s


def _context(path, s, selection=False, deterministic=True):
    pot = capi.Potential(path, selection=selection)
    ctx = capi.Context(pot, 0)
    ctx.set_variant(capi.VARIANT_LARGE)
    ctx.set_deterministic(deterministic)
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
    for k in a:
        ga, gb = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(ga, gb), (what, k, float(np.abs(ga - gb).max()))


def _close(g, w, what, atol=1e-9, rtol=1e-10):   # the tolerances of tests/test_gpu_fixed_shapes.py
    scale = max(1.0, float(np.abs(w).max()))
    err = float(np.abs(np.asarray(g) - np.asarray(w)).max())
    print("%s: max abs err %.3e (scale %.3e)" % (what, err, scale))
    assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)


def _against_oracle(got, want, n):
    _close(got["f"], want["f"], "forces")
    assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n)
    _close(got["eatom"], want["eatom"], "eatom", atol=1e-10)
    _close(got["virial"], want["virial"], "virial", atol=1e-8)
    _close(got["vatom"], want["vatom"], "vatom")


@pytest.mark.parametrize("flags", [(0, 0), (1, 1), (3, 5)])
@pytest.mark.parametrize("path", [W16, W16_NBH], ids=["W_L16", "W_L16_nbh"])
def test_force_shape_is_bitwise_the_generic_kernel(system, monkeypatch, path, flags):
    _, ctx = _context(path, system)
    a, na, b, nb = _both(ctx, system, monkeypatch, eflag=flags[0], vflag=flags[1])
    assert na == FORCE and nb == ""
    _bitwise(a, b, "eflag %d vflag %d" % flags)
    # the neighbours of a centre feel it; an atom listed nowhere inside a cutoff feels nothing
    f = np.asarray(a["f"])
    lone = [i for i, k in enumerate(system.want) if k == 0]
    assert not f[lone].any() and np.abs(f[[i for i, k in enumerate(system.want) if k > 0]]).max(1).min() > 0.0


@pytest.mark.parametrize("path", [W16, W16_NBH], ids=["W_L16", "W_L16_nbh"])
def test_force_shape_against_the_oracle(system, monkeypatch, path):
    from oracle.pyoracle import Oracle
    monkeypatch.delenv("MTP_FIXED_SHAPE", raising=False)
    s = system
    _, ctx = _context(path, s, deterministic=False)   # default mode: native fp64 atomics
    got = ctx.compute(s.x, s.types, eflag=3, vflag=5)
    assert ctx.last_shape() == FORCE
    want = Oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)
    _against_oracle(got, want, s.nlocal)


def test_grade_shape_is_bitwise_the_generic_kernel_and_agrees_with_the_oracle(system, monkeypatch):
    from oracle.pyoracle import Oracle
    s = system
    _, ctx = _context(W16_NBH, s, selection=True)
    a, na, b, nb = _both(ctx, s, monkeypatch, eflag=3, vflag=5, grade=True)
    assert na == GRADE and nb == ""
    assert a["max_grade"] > 0.0 and a["max_grade"] == b["max_grade"]
    _bitwise(a, b, "grade call")
    want = Oracle(W16_NBH, selection=True).compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=s.nlocal)
    _close(a["f"], want["f"], "forces (grade call)")
    _close(a["eatom"], want["eatom"], "eatom (grade call)", atol=1e-10)
    # (grades: the tolerance of tests/test_gpu_parity.py)
    _close(a["grades"][s.ilist], want["grades"][s.ilist], "grades", atol=1e-9, rtol=1e-9)
    assert abs(a["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])


def test_another_block_count_falls_back_to_the_generic_kernel(system, monkeypatch, tmp_path):
    """the level-16 table with rank 1 of radial function 3 added (three basics no row reads): a thirteenth head in the
    grid of t = 1, so 29 five-factor blocks.  No fixed shape takes it, the generic kernel of the same lane grid does, and
    the oracle agrees"""
    from oracle.pyoracle import Oracle
    monkeypatch.delenv("MTP_FIXED_SHAPE", raising=False)
    s = system
    t = mtpgen.build_table(16)
    B = len(t.basic)
    extra = [(3, 1, 0, 0), (3, 0, 1, 0), (3, 0, 0, 1)]
    assert not set(extra) & set(t.basic) and (3, 0, 0, 0) in t.basic
    up = lambda m: m + 3 if m >= B else m
    t2 = mtpgen.MTPTable(level=16, basic=list(t.basic) + extra,
                         times=[(up(a0), up(a1), mult, up(a3)) for a0, a1, mult, a3 in t.times],
                         mapping=[up(m) for m in t.mapping], nmoments=t.nmoments + 3, graphs=list(t.graphs))
    t2.radial_funcs = t.radial_funcs
    path = str(tmp_path / "w16_plus_one.mtp")
    mtpgen.write_mtp(mtpgen.random_potential(t2, 1, 20251, 2.0, RC, 8, 0.37), path)
    pot, ctx = _context(path, s, deterministic=False)
    assert len(capi.Potential(W16).moment_blocks(five=True)[0]) == 28 and len(pot.moment_blocks(five=True)[0]) == 29
    assert pot.kernel_shape()["block_lanes"] == 32 and pot.plan_fixed_shape(256, s.nlocal, 96, capi.VARIANT_LARGE) == ""
    got = ctx.compute(s.x, s.types, eflag=3, vflag=5)
    assert ctx.last_shape() == "" and ctx.plan_info()["waves_per_simd"] == 3
    want = Oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)
    _against_oracle(got, want, s.nlocal)
