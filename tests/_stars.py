"""Disjoint stars: geometries with EXACT neighbour counts for the force kernel.

Star s is one centre, K_s atoms inside the cutoff and L_s - K_s listed atoms outside it; every atom belongs to one star
and only row s of the list names it.  The oracle and the library take any CSR list and only centre-neighbour distances
enter an MTP, so 129 atoms in one shell are no problem, and the two numbers that decide the force kernel's control flow
-- the listed row length L and the in-cutoff count K -- are whatever the caller asks for (the lattices of the other GPU
tests give twenty values of K in all).

Because only row s writes to the atoms of star s, every per-atom output is compared PER STAR with the star's own scale
(per_star_check): a three-tile star with forces of 1e7 eV/A cannot hide a wrong one-neighbour star.

Shared by tests/test_stars_cpu.py, tests/test_gpu_geometry.py, tests/_fuzz.py.
"""
from types import SimpleNamespace

import numpy as np

ORDERS = ("front", "back", "mixed", "straddle")

# the K and L edges of the force kernel: compaction sweeps the row 128 entries at a time, tiles hold NT survivors
def count_edges(NT=32):
    return [0, 1, 2, 3, 4, 5] + [m * NT + d for m in (1, 2, 3, 4) for d in (-1, 0, 1)]


def length_edges(K):
    return sorted(L for L in {K, K + 1, 64, 127, 128, 129, K + 130, 256, 257, 300} if L >= K)


def edge_pairs(NT=32):
    """every K edge crossed with every L edge (L >= K)"""
    return [(K, L) for K in count_edges(NT) for L in length_edges(K)]


def _shell(rng, n, lo, hi):
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u * rng.uniform(lo, hi, n)[:, None]


def _tags(rng, K, L, order):
    """1 = inside the cutoff, 0 = listed but outside, in row order"""
    if order == "front":
        return [1] * K + [0] * (L - K)
    if order == "back":
        return [0] * (L - K) + [1] * K
    if order == "straddle" and L > 128 and K >= 2:
        b = min(K - 1, L - 128)          # survivors behind entry 128 ...
        a = K - b                        # ... and in front of it, touching it on both sides
        if a <= 128:
            t = [0] * L
            for k in range(128 - a, 128 + b):
                t[k] = 1
            return t
    t = np.array([1] * K + [0] * (L - K))
    return list(t[rng.permutation(L)])   # "mixed", and "straddle" where the row cannot straddle


def stars(KL, rng, species=1, rc=5.0, rin=(2.1, 5.0), rout=(5.0, 7.0), order="mixed", special=None, offset=None):
    """KL: [(K, L)] per star.  rin / rout: radial range of the in-cutoff shell and of the listed atoms outside.
    special = "edge": in every star with K > 0 the LAST in-cutoff entry of the row sits at r^2 == rc^2 bit-exact (integer
    centre, offset (rc, 0, 0): inside, the reference drops r^2 > rc^2 only), and one outside entry (if any) one ulp of
    the stored coordinate beyond rc along y: outside.  offset: rigid shift of the whole system (not with "edge": the
    exact offset would not survive the subtraction).
    Returns a namespace: x, types, ilist, first, neigh, nall, sid (star of every atom), KL, start (first atom of every
    star; its centre), rc."""
    assert order in ORDERS and special in (None, "edge") and not (special and offset is not None)
    xs, ilist, first, neigh, sid, start = [], [], [0], [], [], []
    n = 0
    for s, (K, L) in enumerate(KL):
        assert 0 <= K <= L
        c = np.round(rng.uniform(-50, 50, 3))          # integer centre: exact offsets survive the subtraction
        pin = _shell(rng, K, *rin)
        pout = _shell(rng, L - K, np.nextafter(rout[0], np.inf) + 1e-6, rout[1])
        tags = _tags(rng, K, L, order)
        pts = np.zeros((L, 3))
        where_in = [k for k, t in enumerate(tags) if t]
        where_out = [k for k, t in enumerate(tags) if not t]
        pts[where_in] = pin
        pts[where_out] = pout
        row = c + pts
        if special == "edge" and K > 0:
            row[where_in[-1]] = c + np.array([rc, 0.0, 0.0])
            if where_out:
                k = where_out[int(rng.integers(len(where_out)))]
                y = c[1] + np.nextafter(rc, np.inf)
                while not (y - c[1]) * (y - c[1]) > rc * rc:      # (the sum may have rounded back onto c + rc)
                    y = np.nextafter(y, np.inf)
                row[k] = [c[0], y, c[2]]
        start.append(n)
        xs.append(c[None, :])
        xs.append(row)
        ilist.append(n)
        neigh.append(np.arange(n + 1, n + 1 + L))
        first.append(first[-1] + L)
        sid.append(np.full(L + 1, s))
        n += L + 1
    x = np.concatenate(xs) if xs else np.zeros((0, 3))
    if offset is not None:
        x = x + np.asarray(offset, dtype=np.float64)
    types = rng.integers(1, species + 1, len(x)).astype(np.int32)
    return SimpleNamespace(x=np.ascontiguousarray(x), types=types, ilist=np.array(ilist, np.int32),
                           first=np.array(first, np.int32),
                           neigh=np.concatenate(neigh).astype(np.int32) if neigh else np.zeros(0, np.int32),
                           nall=len(x), sid=np.concatenate(sid) if sid else np.zeros(0, int), KL=list(KL),
                           start=np.array(start, dtype=np.int64), rc=rc)


def counts(st, rc=None):
    """(K, L) per star as the force kernel counts them: listed entries, and those with !(r^2 > rc^2) in fp64"""
    rc = st.rc if rc is None else rc
    d = st.x[st.neigh] - np.repeat(st.x[st.ilist], np.diff(st.first), axis=0)
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    inside = ~(r2 > rc * rc)
    cs = np.concatenate([[0], np.cumsum(inside)])
    return [(int(cs[st.first[s + 1]] - cs[st.first[s]]), int(st.first[s + 1] - st.first[s])) for s in range(len(st.ilist))]


def shuffled_rows(st, rng):
    """the same list with every row in another order"""
    ne = st.neigh.copy()
    for s in range(len(st.ilist)):
        ne[st.first[s]:st.first[s + 1]] = rng.permutation(ne[st.first[s]:st.first[s + 1]])
    return ne


def in_cutoff_entries(st, s, neigh=None):
    """positions in the list (indices into neigh) of star s's entries inside the cutoff, in row order: the order in which
    the compaction of the centre kernels keeps them, entry k of it in tile k // 32"""
    ne = st.neigh if neigh is None else neigh
    a, b = int(st.first[s]), int(st.first[s + 1])
    d = st.x[ne[a:b]] - st.x[st.ilist[s]]
    return a + np.flatnonzero(~(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] > st.rc * st.rc))


def centres_first(st):
    """the same stars with the atoms renumbered: the centres are atoms 0 .. stars - 1 in row order (ilist = arange), the
    outer atoms follow in their old order.  For owner maps that fold the outer atoms onto a few owned rows behind the
    centres.  The atoms of a star are no longer contiguous: start is None."""
    n = len(st.ilist)
    outer = np.setdiff1d(np.arange(st.nall), st.ilist)
    old = np.concatenate([st.ilist, outer]).astype(np.int64)       # old[new]
    new = np.empty(st.nall, dtype=np.int64)
    new[old] = np.arange(st.nall)
    return SimpleNamespace(x=np.ascontiguousarray(st.x[old]), types=st.types[old].copy(), ilist=np.arange(n, dtype=np.int32),
                           first=st.first.copy(), neigh=new[st.neigh].astype(np.int32), nall=st.nall, sid=st.sid[old],
                           KL=list(st.KL), start=None, rc=st.rc)


def _star_max(st, a):
    """max |a| over the atoms of every star -> [stars]"""
    a = np.abs(np.asarray(a, dtype=np.float64)).reshape(len(a), -1).max(1)
    return np.maximum.reduceat(a, st.start) if len(st.start) else np.zeros(0)


# (atol, rtol) of tests/test_gpu_parity.py and tests/test_gpu_shapes.py, applied per star
PER_STAR_TOL = dict(f=(1e-9, 1e-10), eatom=(1e-10, 1e-10), vatom=(1e-9, 1e-10), grades=(1e-9, 1e-9))


def per_star_ratios(st, got, want, keys=("f", "eatom", "vatom")):
    """{key: error / tolerance per star}, tolerance = atol + rtol * max(1, max |want| over the star's atoms)"""
    out = {}
    for k in keys:
        atol, rtol = PER_STAR_TOL[k]
        err = _star_max(st, np.asarray(got[k]) - np.asarray(want[k]))
        scale = np.maximum(1.0, _star_max(st, want[k]))
        out[k] = err / (atol + rtol * scale)
    return out


def per_star_check(st, got, want, grade=False, configuration_mode=False, label=""):
    """Per-star comparison of f, eatom, vatom (grades on neighbourhood-mode grade calls), then the totals in the global
    form of tests/test_gpu_parity.py.  Returns the worst error / tolerance per quantity."""
    keys = ("f", "eatom", "vatom") + (("grades",) if grade and not configuration_mode else ())
    worst = {}
    ratios = per_star_ratios(st, got, want, keys)
    for k in keys:
        r = ratios[k]
        if len(r) == 0:
            continue
        s = int(np.argmax(r))
        worst[k] = float(r[s])
        assert np.isfinite(r).all() and r[s] <= 1.0, "%s %s: star %d (K, L) = %s misses its tolerance %.2f-fold" % (
            label, k, s, st.KL[s], r[s])
    n = max(1, len(st.ilist))
    assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n), label + " energy"
    vs = max(1.0, float(np.abs(want["virial"]).max()))
    assert np.abs(got["virial"] - want["virial"]).max() <= 1e-8 + 1e-10 * vs, label + " virial"
    if grade and configuration_mode:
        cs = max(1.0, float(np.abs(want["coeff_ders"]).max()))
        assert np.abs(got["coeff_ders"] - want["coeff_ders"]).max() <= 1e-9 + 1e-10 * cs, label + " coeff_ders"
    elif grade:
        assert abs(got["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"]), label + " max_grade"
    return worst
