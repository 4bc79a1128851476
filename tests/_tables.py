"""Seeded MLIP-3 tables that do not come from the level generator (mtpgen.build_table): any set of radial slots
(mu, nu), each with all of its monomials or a chosen subset (a sparse table: coefficient blocks with holes), any
radial basis size, scaling and window.  Shared by tests/test_shapes_cpu.py and tests/test_gpu_shapes.py.

Scalars of a table:
  * every rank-0 basic on its own;
  * the full self-contraction of every slot of rank > 0, and cross-contractions of equal-rank slots:
    sum_{|m| = nu} multinomial(m) M_s[m] M_t[m] over the monomials both slots list -- one times row per monomial, the
    multinomial as its multiplicity (rank 11 peaks at 11!/(4! 4! 3!) = 11 550, inside the loader's 16 bits);
  * a few three-factor chains: (contraction) x (rank-0 basic).
Rows are written target by target, each target after its factors: topologically ordered.
"""
import numpy as np

from lammps_mtp_kokkos_amd import mtpgen


def block_count(slots, subsets=None):
    """Head x tail blocks the library's build_blocks makes for these slots (same walk: for every j, heads = slots of
    rank >= j in (rank, mu) order with a = nu - j, tails = (b, c) with b + c = j, both cut into threes; a block with no
    listed basic is dropped)."""
    subsets = subsets or {}
    slots = sorted(set(slots), key=lambda s: (s[1], s[0]))
    P = 1 + max(nu for _, nu in slots)
    have = {s: set(subsets.get(s, mtpgen.monomials(s[1]))) for s in slots}
    n = 0
    for j in range(P):
        heads = [(s, s[1] - j) for s in slots if s[1] >= j]
        tails = [(j - c, c) for c in range(j + 1)]
        for h0 in range(0, len(heads), 3):
            for t0 in range(0, len(tails), 3):
                if any((a, b, c) in have[s] for s, a in heads[h0:h0 + 3] for b, c in tails[t0:t0 + 3]):
                    n += 1
    return n


def make_table(slots, subsets=None, cross=8, chains=3, seed=0):
    """MTPTable over `slots` [(mu, nu)]; `subsets` {slot: [(a, b, c)]} lists only those monomials for a slot (sparse).
    `cross` caps the cross-contractions, `chains` the three-factor products.  Returns (table, factors per scalar)."""
    rng = np.random.default_rng(seed)
    subsets = subsets or {}
    slots = sorted(set(slots))
    basic, index = [], {}
    for (mu, nu) in slots:
        mons = mtpgen.monomials(nu)
        want = set(subsets.get((mu, nu), mons))
        assert want <= set(mons) and want, (mu, nu)
        for m in mons:
            if m in want:
                index[(mu, m)] = len(basic)
                basic.append((mu,) + m)
    times, mapping, nfac = [], [], []
    nmom = len(basic)
    for (mu, nu) in slots:
        if nu == 0:
            mapping.append(index[(mu, (0, 0, 0))])
            nfac.append(1)

    def contract(s, t):
        nonlocal nmom
        common = [m for m in mtpgen.monomials(s[1]) if (s[0], m) in index and (t[0], m) in index]
        if not common:
            return None
        out = nmom
        nmom += 1
        for m in common:
            a0, a1 = sorted((index[(s[0], m)], index[(t[0], m)]))
            times.append((a0, a1, mtpgen.multinomial(m), out))
        return out

    contractions = []
    for s in slots:
        if s[1] > 0:
            contractions.append(contract(s, s))
    pairs = [(s, t) for i, s in enumerate(slots) for t in slots[i + 1:] if s[1] == t[1] and s[1] > 0]
    for k in rng.permutation(len(pairs))[:cross]:
        c = contract(*pairs[k])
        if c is not None:
            contractions.append(c)
    mapping += contractions
    nfac += [2] * len(contractions)
    scal0 = [index[(mu, (0, 0, 0))] for (mu, nu) in slots if nu == 0]
    if scal0 and contractions:
        for k in range(chains):
            c = contractions[int(rng.integers(len(contractions)))]
            z = scal0[int(rng.integers(len(scal0)))]
            times.append((min(c, z), max(c, z), 1, nmom))
            mapping.append(nmom)
            nfac.append(3)
            nmom += 1
    tab = mtpgen.MTPTable(level=0, basic=basic, times=times, mapping=mapping, nmoments=nmom)
    tab.radial_funcs = 1 + max(b[0] for b in basic)
    return tab, np.array(nfac)


def potential(tab, nfac, species=1, seed=4242, R=8, scaling=1.0, min_dist=2.0, max_dist=5.0, damp=0.25):
    """mtpgen.Potential with random_potential's ranges; moment coefficients damped by the number of tensor factors
    (random_potential only knows the level-8 damping for tables without graphs)."""
    p = mtpgen.random_potential(mtpgen.level8_template(), species, seed, min_dist, max_dist, R, scaling)
    rng = np.random.default_rng(seed + 1)
    p.table = tab
    p.radial_coeffs = rng.uniform(-0.1, 0.1, size=(species * species, tab.radial_funcs, R))
    p.moment_coeffs = rng.uniform(-0.5, 0.5, size=len(tab.mapping)) * damp ** (nfac - 1)
    return p


def pad_rows(tab):
    """write_mtp asserts the reference reader's line limits: every line after alpha_index_times must fit in T*32+20
    characters, so a table with many scalars and few rows gets extra rows (x += 0 * y, on a fresh moment)."""
    while len(tab.times) * 32 + 20 < 26 * len(tab.mapping) + 64:
        tab.times.append((0, 0, 0, tab.nmoments))
        tab.nmoments += 1
    return tab


def write(tab, nfac, path, mvs=None, **kw):
    p = potential(pad_rows(tab), nfac, **kw)
    if mvs:
        mtpgen.add_selection_state(p, mvs)
    mtpgen.write_mtp(p, path)
    return path


# ---- tables that land on a requested (KL, NB, DEG) ----------------------------------------------------------------


def _sparse_slots(nblk_target, max_rank, Mu, seed):
    """Slots of ranks <= max_rank over Mu radial functions, each keeping a few monomials, until block_count reaches
    nblk_target; roughly one basic per block keeps B within 640."""
    rng = np.random.default_rng(seed)
    slots, subsets = [(0, 0), (0, max_rank)], {}
    subsets[(0, max_rank)] = mtpgen.monomials(max_rank)[:3]
    cand = [(mu, nu) for nu in range(1, max_rank + 1) for mu in range(Mu) if (mu, nu) not in slots]
    rng.shuffle(cand)
    for s in cand:
        mons = mtpgen.monomials(s[1])
        pick = [mons[int(k)] for k in rng.choice(len(mons), min(len(mons), int(rng.integers(2, 5))), replace=False)]
        trial = dict(subsets)
        trial[s] = pick
        n = block_count(slots + [s], trial)
        if n > nblk_target:
            continue
        slots.append(s)
        subsets = trial
        if n == nblk_target:
            break
    return slots, subsets


def shape_table(KL, NB, DEG, seed=0, Mu=None):
    """(slots, subsets) whose table lands on lane grid KL x NB with force-phase rank cap DEG (kernel_shape reports it)."""
    lo = {16: 1, 32: 17, 64: 33}[KL] if NB == 1 else 64 * (NB - 1) + 1
    hi = KL * NB
    dlow = 6 if KL <= 32 else 8
    rank = dlow if DEG == dlow else (dlow + 1 if (KL, NB) != (64, 4) else 11)
    if KL == 16 and NB == 1:
        base = [(0, 0), (0, rank)] + ([(1, 0)] if DEG == 6 else [])
        return base, {}
    target = (lo + hi) // 2
    return _sparse_slots(target, rank, Mu or (16 if NB >= 3 else 8), seed)


def exact_blocks(target):
    """(slots, subsets) with exactly `target` head x tail blocks on few slots (each slot's derivative-coefficient block
    takes LDS whether its monomials are listed or not): ranks 10 and 11 over Mu = 16, one monomial each to start, then
    single monomials added where each one opens exactly one more block."""
    slots = [(0, 0)] + [(mu, nu) for nu in (10, 11) for mu in range(16)]
    subsets = {s: mtpgen.monomials(s[1])[:1] for s in slots}
    n = block_count(slots, subsets)
    for s in slots:
        for m in mtpgen.monomials(s[1])[1:]:
            if n == target:
                break
            trial = dict(subsets)
            trial[s] = subsets[s] + [m]
            k = block_count(slots, trial)
            if k == n + 1:
                subsets, n = trial, k
    assert n == target, (n, target)
    return slots, subsets


# ---- the instantiation matrix: one case per shipped mtp_wave_kernel<KL, NB, PITCH, GRADE, DEG, WPS> ---------------

SHAPES = [(16, 1, 6), (16, 1, 11), (32, 1, 6), (32, 1, 11), (64, 1, 8), (64, 1, 11),
          (64, 2, 8), (64, 2, 11), (64, 3, 8), (64, 3, 11), (64, 4, 8), (64, 4, 11)]
# the three-wavefronts-per-SIMD build carries the dg-free layouts only: Mu <= 4, ranks <= 6 on a KL <= 32 grid
WPS3_SLOTS = {16: [(0, 0), (0, 6), (1, 0)],
              32: [(mu, 0) for mu in range(4)] + [(mu, 6) for mu in range(4)]}


def case_slots(case):
    """(slots, subsets) of a MATRIX case"""
    if case["wps"] == 3:
        return WPS3_SLOTS[case["KL"]], {}
    return shape_table(case["KL"], case["NB"], case["DEG"])


MATRIX = [dict(KL=kl, NB=nb, DEG=deg, grade=g, wps=2) for (kl, nb, deg) in SHAPES for g in (False, True)] + \
         [dict(KL=kl, NB=1, DEG=6, grade=g, wps=3) for kl in (16, 32) for g in (False, True)]


def case_id(case):
    return "KL%d_NB%d_DEG%d_%s_wps%d" % (case["KL"], case["NB"], case["DEG"], "grade" if case["grade"] else "force",
                                          case["wps"])


def basic_limit_slots(extra):
    """B = 640 (the candidate-vector lane grids' cap) + `extra`: eight dense rank-11 slots and sixteen rank-0 slots,
    plus `extra` single monomials of rank 1 (95 + extra head x tail blocks)."""
    slots = [(mu, 11) for mu in range(8)] + [(mu, 0) for mu in range(16)]
    subsets = {}
    for k in range(extra):
        slots.append((8 + k, 1))
        subsets[(8 + k, 1)] = [(1, 0, 0)]
    return slots, subsets
