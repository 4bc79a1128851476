"""The star generator of tests/_stars.py, on the CPU: the counts that come out are the counts asked for (recomputed
with the force kernel's predicate), the special distances are what they claim, the oracle's forces on stars are the
gradient of its energy, and the inputs are well conditioned for the reference: the oracle against itself with every row
re-shuffled stays far inside the per-star tolerance the GPU tests apply."""
import os

import numpy as np
import pytest

from oracle.pyoracle import Oracle

import _stars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")


@pytest.mark.parametrize("order", _stars.ORDERS)
@pytest.mark.parametrize("kind", ["plain", "edge", "below_min_dist", "offset_1e5", "offset_negative"])
def test_counts_are_the_counts_asked_for(order, kind):
    KL = _stars.edge_pairs(32)
    assert len({K for K, _ in KL}) == 18 and {L for _, L in KL} >= {64, 127, 128, 129, 256, 257, 300}
    kw = dict(plain={}, edge=dict(special="edge"), below_min_dist=dict(rin=(1.0, 5.0)),
              offset_1e5=dict(offset=(1e5, 1e5, 1e5)), offset_negative=dict(offset=(-731.25, -1e5, -3.5)))[kind]
    st = _stars.stars(KL, np.random.default_rng(3), species=2, order=order, **kw)
    assert _stars.counts(st) == KL
    # every atom belongs to one star and only its row names it
    assert st.nall == sum(L + 1 for _, L in KL) and np.array_equal(np.sort(np.concatenate([st.neigh, st.ilist])),
                                                                   np.arange(st.nall))
    assert np.array_equal(st.sid[st.ilist], np.arange(len(KL))) and np.array_equal(st.sid[st.neigh],
                                                                                   np.repeat(np.arange(len(KL)), np.diff(st.first)))
    assert set(np.unique(st.types)) == {1, 2}


def test_row_orders():
    KL = [(40, 300), (2, 129), (129, 129), (129, 259), (5, 64), (0, 130)]
    rng = np.random.default_rng(1)
    for order in _stars.ORDERS:
        st = _stars.stars(KL, rng, order=order)
        d = st.x[st.neigh] - np.repeat(st.x[st.ilist], np.diff(st.first), axis=0)
        inside = ~((d * d).sum(1) > 25.0)
        for s, (K, L) in enumerate(KL):
            row = inside[st.first[s]:st.first[s + 1]]
            if order == "front":
                assert row[:K].all()
            elif order == "back":
                assert row[L - K:].all()
            elif order == "straddle" and L > 128 and K >= 2:
                # survivors on both sides of entry 128: the second sweep of the compaction continues a count
                assert row[127] and row[128] and row[:128].sum() + row[128:].sum() == K


def test_exact_cutoff_entry_is_inside_and_its_neighbour_outside():
    KL = [(33, 64), (4, 5), (1, 2), (32, 129), (65, 300), (5, 5)]
    for order in _stars.ORDERS:
        st = _stars.stars(KL, np.random.default_rng(8), special="edge", order=order)
        assert _stars.counts(st) == KL
        for s, (K, L) in enumerate(KL):
            js = st.neigh[st.first[s]:st.first[s + 1]]
            d = st.x[js] - st.x[st.ilist[s]]
            r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            at = np.flatnonzero(r2 == 25.0)
            assert len(at) == 1                                   # bit-exact, and counted inside by !(r2 > 25)
            assert at[0] == np.flatnonzero(~(r2 > 25.0))[-1]      # the LAST survivor of the row: it takes place K - 1
            if L > K:
                just = r2[r2 > 25.0].min()
                assert 25.0 < just < 25.0 * (1 + 1e-13)           # the next representable coordinate: outside


@pytest.mark.parametrize("name,species", [("W_L8.mtp", 1), ("W_L16.mtp", 1), ("WRe_L20.mtp", 2)])
def test_oracle_forces_on_stars_are_central_differences(name, species):
    KL = [(1, 3), (3, 3), (5, 9), (33, 40)]
    st = _stars.stars(KL, np.random.default_rng(21), species=species, rin=(2.1, 4.6))
    o = Oracle(os.path.join(POT, name))

    def energy(x):
        return o.compute(x, st.types, st.ilist, st.first, st.neigh)["energy"]

    F = o.compute(st.x, st.types, st.ilist, st.first, st.neigh)["f"]
    h = 1e-5
    rng = np.random.default_rng(2)
    for s in range(len(KL)):
        atoms = np.flatnonzero(st.sid == s)
        scale = max(1.0, np.abs(F[atoms]).max())
        for a in [atoms[0]] + list(rng.choice(atoms[1:], 2, replace=False)):
            for c in range(3):
                xp, xm = st.x.copy(), st.x.copy()
                xp[a, c] += h
                xm[a, c] -= h
                fd = -(energy(xp) - energy(xm)) / (2 * h)
                assert abs(fd - F[a, c]) < 2e-7 * scale, (KL[s], a, c, fd, F[a, c])
    # a star is closed: its forces sum to zero
    for s in range(len(KL)):
        m = st.sid == s
        assert np.abs(F[m].sum(0)).max() < 1e-10 * max(1.0, np.abs(F[m]).max())


@pytest.mark.parametrize("name,species", [("W_L8.mtp", 1), ("W_L16.mtp", 1), ("WRe_L20.mtp", 2)])
@pytest.mark.parametrize("kind", ["plain", "edge", "below_min_dist"])
def test_reference_self_noise_is_far_inside_the_per_star_tolerance(name, species, kind):
    """The oracle against itself with every row in another order -- the reference's own re-association noise -- in
    units of the per-star tolerance of _stars.per_star_check.  Measured over the K x L edges: at most 1.5e-4 for F,
    eatom and vatom (levels 8 / 16 / 20); the bound 1e-2 leaves margin for other seeds.  A case that fails here is badly
    conditioned for the reference and must not be used to judge a kernel."""
    kw = dict(plain={}, edge=dict(special="edge"), below_min_dist=dict(rin=(1.0, 5.0)))[kind]
    KL = _stars.edge_pairs(32)
    rng = np.random.default_rng(5)
    KL = [KL[k] for k in rng.permutation(len(KL))]
    st = _stars.stars(KL, rng, species=species, **kw)
    o = Oracle(os.path.join(POT, name))
    a = o.compute(st.x, st.types, st.ilist, st.first, st.neigh)
    b = o.compute(st.x, st.types, st.ilist, st.first, _stars.shuffled_rows(st, np.random.default_rng(6)))
    ratios = _stars.per_star_ratios(st, b, a)
    for k, r in ratios.items():
        s = int(np.argmax(r))
        print("%s %s %s: worst noise / tolerance %.2e at (K, L) = %s" % (name, kind, k, r[s], KL[s]))
        assert r[s] < 1e-2, (k, KL[s], r[s])
