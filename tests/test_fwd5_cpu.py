"""The five-factor blocks of the basic-moment pass (csrc/mtp_potential.cpp, build_blocks5; layout in csrc/mtp_potential.hpp)
as the fixed force shape of level 16 reads them, checked on the host against the potential's own basics and against the
3 x 3 head x tail blocks the generic kernels keep.

A block is five factors, each a pair of table rows: a head {g row of slot s, x^a} or a tail {y^b, z^c}.  Factors 0, 1 are
heads and 3, 4 tails; factor 2 is a head when the shape bit is set (3 heads x 2 tails) and a tail otherwise (2 x 3).  Six
products: (0,3) (0,4) (1,3) (1,4), then (2,3) (2,4) or (0,2) (1,2).

The replay forms every basic moment from random tile tables the way either pass does -- per neighbour column, in order,
acc += (row * row) * (row * row) with both inner products rounded first.  numpy has no fused multiply-add, so both
replays round the outer product before the addition; the kernels fuse it in both passes.  Either way the two passes
apply the same operations to the same operands in the same order, which is what bitwise equality of the replays
shows."""
import os
import re

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
COMMITTED = ["W_L8.mtp", "W_L16.mtp", "W_L16_nbh.almtp", "WRe_L10_cfg.almtp", "WRe_L20.mtp"]
PRODUCTS_3X2 = [(0, 3), (0, 4), (1, 3), (1, 4), (2, 3), (2, 4)]   # (head factor, tail factor) of each product slot
PRODUCTS_2X3 = [(0, 3), (0, 4), (1, 3), (1, 4), (0, 2), (1, 2)]


def _decode5(blocks):
    """[(factors [(lo, hi)] * 5, wide, kk [6])] of the five-factor blocks"""
    out = []
    for w in blocks:
        u = w.astype(np.int64) & 0xffffffff
        factors = [(int(u[f] & 0xffff), int((u[f] >> 16) & 0x7fff)) for f in range(5)]
        kk = np.ascontiguousarray(w[5:8]).view(np.int16)
        assert kk.shape == (6,)
        out.append((factors, bool(u[2] >> 31), [int(k) for k in kk]))
    return out


def _decode3(blocks):
    """[(heads [(s, a)] * 3, tails [(b, c)] * 3, kk [9])] of the 3 x 3 blocks (head-major indices)"""
    out = []
    for w in blocks:
        u = w.astype(np.int64) & 0xffffffff
        heads = [(int((u[0] >> (8 * h)) & 255), int((u[1] >> (4 * h)) & 15)) for h in range(3)]
        tails = [(int((u[1] >> (12 + 4 * t)) & 15), int((u[2] >> (4 * t)) & 15)) for t in range(3)]
        kk = np.ascontiguousarray(w[3:8]).view(np.int16)[:9]
        out.append((heads, tails, [int(k) for k in kk]))
    return out


def _unpack(pack):
    """(slot, a, b, c) of the basic at each LDS number"""
    p = pack.astype(np.int64)
    return [(int(v & 255), int((v >> 8) & 15), int((v >> 12) & 15), int((v >> 16) & 15)) for v in p]


def _products5(blocks):
    """{k: (head (s, a), tail (b, c))} over every product slot that names a basic, with the structural checks"""
    seen = {}
    for factors, wide, kk in _decode5(blocks):
        prods = PRODUCTS_3X2 if wide else PRODUCTS_2X3
        for e, (hf, tf) in enumerate(prods):
            k = kk[e]
            assert k >= -1
            if k < 0:
                continue
            assert k not in seen, "basic %d in two product slots" % k
            seen[k] = (factors[hf], factors[tf])
    return seen


def _check_potential(path, selection=False):
    pot = capi.Potential(path, selection=selection)
    b5, pack = pot.moment_blocks(five=True)
    b3, pack3 = pot.moment_blocks(five=False)
    assert np.array_equal(pack, pack3)
    B, P = pot.sizes["B"], pot.sizes["P"]
    basics = _unpack(pack)
    nslot = 1 + max(s for s, _, _, _ in basics)
    assert b5.shape == (len(b5), 8) and len(b5) >= (B + 5) // 6
    # every basic in exactly one product slot, as the product of the head and the tail it is made of
    seen = _products5(b5)
    assert sorted(seen) == list(range(B))
    for k, ((s, a), (b, c)) in seen.items():
        assert (s, a, b, c) == basics[k], (k, (s, a, b, c), basics[k])
    # at most five factors (the layout has five), with rows in range whatever the factor's kind: a head's (slot, a), a tail's (b, c)
    for factors, wide, kk in _decode5(b5):
        assert any(k >= 0 for k in kk), "an empty block"
        for f, (lo, hi) in enumerate(factors):
            head = f < 2 or (f == 2 and wide)
            assert (lo < nslot if head else lo < P) and hi < P, (f, lo, hi)
    # ... and as rows of the tile table of a planned launch
    try:
        fields = pot.plan_fixed_fields(256, 65536, 96)
    except capi.MtpError:
        fields = None
    if fields is not None:
        assert fields["nfb5"] == len(b5) and fields["nfb"] == len(b3)
        top = fields["pow_row"] + 3 * fields["P"]
        assert top <= fields["tab_rows"] and nslot <= fields["pow_row"]
    return pot, b3, b5, pack


def _replay(pot, b3, b5, pack, seed):
    """basic moments from random tile tables by the 3 x 3 pass and by the five-factor pass"""
    rng = np.random.default_rng(seed)
    B, P = pot.sizes["B"], pot.sizes["P"]
    nslot = 1 + max(s for s, _, _, _ in _unpack(pack))
    ncol = 13   # the headline lattice: 26 neighbours in two groups
    G, X, Y, Z = (rng.uniform(-1.5, 1.5, size=(n, ncol)) for n in (nslot, P, P, P))

    def accumulate(pairs):   # [(k, (s, a), (b, c))] -> M[k] = sum over the columns, in order
        M = np.zeros(B)
        ks = np.array([k for k, _, _ in pairs])
        s, a = (np.array([h[i] for _, h, _ in pairs]) for i in (0, 1))
        b, c = (np.array([t[i] for _, _, t in pairs]) for i in (0, 1))
        acc = np.zeros(len(pairs))
        for col in range(ncol):
            hd = G[s, col] * X[a, col]
            tl = Y[b, col] * Z[c, col]
            acc = acc + hd * tl
        M[ks] = acc
        return M

    three = [(kk[3 * h + t], heads[h], tails[t]) for heads, tails, kk in _decode3(b3) for h in range(3) for t in range(3)
             if kk[3 * h + t] >= 0]
    five = [(k, h, t) for k, (h, t) in _products5(b5).items()]
    assert sorted(k for k, _, _ in three) == list(range(B))
    return accumulate(three), accumulate(five)


@pytest.mark.parametrize("name", COMMITTED)
def test_committed_potentials(name):
    pot, b3, b5, pack = _check_potential(os.path.join(POT, name))
    M3, M5 = _replay(pot, b3, b5, pack, 5)
    assert np.abs(M3).min() > 0.0 and np.array_equal(M3, M5)


def test_level16_count_is_the_fixed_shapes_constant():
    """28 blocks: 6 + 4 (3 x 2), 5 (2 x 3), 4 (3 x 2), 4 + 2 + 3 (2 x 3) over t = 0 .. 6; one lane each at KL = 32"""
    text = open(os.path.join(ROOT, "lammps_mtp_kokkos_amd", "csrc", "mtp_fixed_shapes.hpp")).read()
    consts = [int(v) for v in re.findall(r"static constexpr int nfb5 = (\d+);", text)]
    assert len(consts) == 1   # the force shape (the grade shape keeps the 3 x 3 pass and leaves the field dynamic)
    for name, selection in (("W_L16.mtp", False), ("W_L16_nbh.almtp", True)):
        pot = capi.Potential(os.path.join(POT, name), selection=selection)
        b5, _ = pot.moment_blocks(five=True)
        assert len(b5) <= 32 and all(len(b5) == c for c in consts), (len(b5), consts)
        wide = [w for _, w, _ in _decode5(b5)]
        assert len(b5) == 28 and sum(wide) == 14
        # the plans of the headline launch are the two shapes'
        assert pot.plan_fixed_shape(256, 65536, 96) == "w16_force_3ps"
        assert pot.plan_fixed_shape(256, 65536, 96, grade=True) == "w16_grade_3ps"


@pytest.fixture(scope="module")
def tables():
    return {L: mtpgen.build_table(L) for L in range(4, 23, 2)}


@pytest.mark.parametrize("species", [1, 2])
@pytest.mark.parametrize("level", list(range(4, 23, 2)))
def test_generated_potentials(tables, tmp_path, level, species):
    p = mtpgen.random_potential(tables[level], species, 400 + level)
    path = str(tmp_path / ("gen%d_%d.mtp" % (level, species)))
    mtpgen.write_mtp(p, path)
    if (level, species) == (4, 2):
        # The reference's reader does not accept this file (two species with the two scalars of level 4: "Moment
        # coefficients not found"), the oracle's copy of it says so, and the library refuses it with the same code:
        # there is no potential to tile.  Every other case must load.
        from oracle.pyoracle import Oracle
        with pytest.raises(Exception) as eo:
            Oracle(path)
        with pytest.raises(capi.MtpError) as el:
            capi.Potential(path)
        assert "rc=%d" % el.value.code in str(eo.value) and "Moment coefficients not found" in str(el.value)
        return
    pot, b3, b5, pack = _check_potential(path)
    M3, M5 = _replay(pot, b3, b5, pack, level)
    assert np.array_equal(M3, M5)


def _with_extra_basics(table, extra):
    """the table with basics appended that no row reads (moments behind the basics move up)"""
    B, n = len(table.basic), len(extra)
    up = lambda m: m + n if m >= B else m
    t = mtpgen.MTPTable(level=table.level, basic=list(table.basic) + list(extra),
                        times=[(up(a0), up(a1), mult, up(a3)) for a0, a1, mult, a3 in table.times],
                        mapping=[up(m) for m in table.mapping], nmoments=table.nmoments + n, graphs=list(table.graphs))
    t.radial_funcs = 1 + max(b[0] for b in t.basic)
    return t


def test_partly_listed_group_is_covered(tables, tmp_path):
    """rank 5 of radial function 0 lists 3 of its 21 monomials (one of them alone in its t-group): the grids of t = 0, 3
    and 5 are not full, and the blocks that hold the three have -1 in other product slots"""
    base = tables[10]
    extra = [(0, 5, 0, 0), (0, 2, 2, 1), (0, 0, 1, 4)]
    assert 1 + max(b[1] + b[2] + b[3] for b in base.basic) <= 5 and not set(extra) & set(base.basic)
    p = mtpgen.random_potential(_with_extra_basics(base, extra), 1, 77)
    path = str(tmp_path / "partial.mtp")
    mtpgen.write_mtp(p, path)
    pot, b3, b5, pack = _check_potential(path)
    assert pot.sizes["B"] == len(base.basic) + 3 and pot.sizes["P"] == 6
    slots = [k for _, _, kk in _decode5(b5) for k in kk]
    assert slots.count(-1) == 6 * len(b5) - pot.sizes["B"] > 0
    M3, M5 = _replay(pot, b3, b5, pack, 9)
    assert np.array_equal(M3, M5)
