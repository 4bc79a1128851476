"""Seeded MLIP-3 tables that do not come from the level generator (mtpgen.build_table): any set of radial slots
(mu, nu), each with all of its monomials or a chosen subset (a sparse table: coefficient blocks with holes), any
radial basis size, scaling and window.  Shared by the force kernel's instantiation matrix (tests/test_shapes_cpu.py,
tests/test_gpu_shapes.py, tests/test_gpu_geometry.py) and, through CENTRE_TABLES at the end of the file, by the tests of the
two per-centre kernels: the design rows (tests/_design.py, tests/test_design_cpu.py, tests/test_design_gpu.py) and the
training gradient (tests/test_train_cpu.py, tests/test_train_gpu.py).

Scalars of a table:
  * every rank-0 basic on its own;
  * the full self-contraction of every slot of rank > 0, and cross-contractions of equal-rank slots:
    sum_{|m| = nu} multinomial(m) M_s[m] M_t[m] over the monomials both slots list -- one times row per monomial, the
    multinomial as its multiplicity (rank 11 peaks at 11!/(4! 4! 3!) = 11 550, inside the loader's 16 bits);
  * a few three-factor chains: (contraction) x (rank-0 basic).
Rows are written target by target, each target after its factors: topologically ordered.
"""
import functools
import os
import tempfile
from types import SimpleNamespace

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


# ---- tables for the per-centre kernels (csrc/mtp_design.hip, csrc/mtp_train.hip, csrc/mtp_centre_common.hpp) -----------
# The level generator stops at five radial functions, dense slots and rank 8.  Each case below is the smallest table that
# reaches one more path of those kernels; `reaches` says which (NT = 32 columns per tile, eight threads -- parts -- per
# column, 256 threads; tile_radial deals radial function mu to part 7 - mu % 8).
_MU16 = [(mu, 0) for mu in range(16)] + [(0, 1), (7, 1), (8, 1), (15, 1), (15, 2), (8, 3), (0, 6)]
_MU16_SUB = {(0, 6): [(6, 0, 0), (2, 2, 2), (0, 3, 3), (1, 0, 5), (4, 1, 1)]}
CENTRE_TABLES = dict(
    mu6=dict(slots=[(mu, 0) for mu in range(6)] + [(5, 1), (4, 2)], species=1,
             reaches="parts 3 and 2 compute a radial function and write a power row"),
    mu8=dict(slots=[(mu, 0) for mu in range(8)] + [(0, 1), (7, 1), (3, 2), (7, 2), (1, 3), (6, 3)], species=2,
             reaches="every part computes a radial function: part 0 (nb, r^-nu) computes mu = 7"),
    mu9=dict(slots=[(mu, 0) for mu in range(9)] + [(8, 1), (0, 2), (8, 2), (3, 3)], species=2, R=9, scaling=0.37,
             reaches="second trip of the dealing loop in part 7 only, the thread that keeps Q and Q'; R != 8 behind 2 Mu"),
    mu13_gaps=dict(slots=[(0, 0), (2, 0), (5, 0), (7, 0), (12, 0), (2, 1), (12, 1), (5, 2), (7, 3), (0, 4)],
                   subsets={(0, 4): [(4, 0, 0), (2, 1, 1), (0, 2, 2), (1, 3, 0), (0, 0, 4), (1, 1, 2)]}, species=2,
                   reaches="radial functions without basics (empty mufirst runs), 2 Mu > 24 scratch rows, blk = 208"),
    mu16_sp3=dict(slots=_MU16, subsets=_MU16_SUB, species=3,
                  reaches="Mu NT = 512 items and blk = 384: second trips of both vjp loops; 1152 radial columns"),
    mu16_sp2_nbh=dict(slots=_MU16, subsets=_MU16_SUB, species=2, mvs="nbh",
                      reaches="Sp Mu R = 256, the grade kernels' limit: the unfused candidate vectors at Mu = 16"),
    rank11=dict(slots=[(0, 0), (1, 0), (0, 11), (1, 11)],
                subsets={(0, 11): [(11, 0, 0), (4, 4, 3), (5, 3, 3), (0, 0, 11)],
                         (1, 11): [(4, 4, 3), (0, 11, 0), (5, 3, 3), (1, 1, 9)]}, species=1,
                reaches="P = 12, the loader's cap; multiplicity 11 550 in the packed rows; holes in coefficient blocks"),
)
# exact neighbour counts of the star sets these tables are run on: no, one and two neighbours, a full tile, one past it,
# three tiles; row lengths K, K + 1 and past two compaction sweeps
CENTRE_KL = [(K, L) for K in (0, 1, 2, 32, 33, 65) for L in (K, K + 1, 129)]


def deal_wrongly(radial_coeffs, Sp, Mu, how):
    """a copy of the radial block [Sp Sp, Mu, R] (flat) as a wrong tile_radial would use it.  "dropped": the second trip of
    its loop never runs, every mu >= 8 gives zero; "modulo": the coefficient row is taken at mu % 8; "part0": the share of
    part 0, radial function 7, is never computed.  For the tests that show that their rule rejects such a kernel."""
    rc = np.array(radial_coeffs, dtype=np.float64).reshape(Sp * Sp, Mu, -1)
    if how == "dropped":
        rc[:, 8:] = 0.0
    elif how == "modulo":
        rc[:, 8:] = rc[:, :Mu - 8].copy()
    else:
        assert how == "part0" and Mu >= 8
        rc[:, 7] = 0.0
    assert not np.array_equal(rc.reshape(-1), np.asarray(radial_coeffs).reshape(-1))
    return rc.reshape(-1)


# (case, damage) pairs of the "judge rejects" tests: every case with a second trip, and part 0's share on mu8
DEALT_WRONGLY = [(n, h) for n in ("mu9", "mu13_gaps", "mu16_sp3", "mu16_sp2_nbh") for h in ("dropped", "modulo")] + [("mu8", "part0")]


def centre_table(name):
    """(table, factors per scalar) of a case of CENTRE_TABLES"""
    c = CENTRE_TABLES[name]
    return make_table(c["slots"], c.get("subsets"))


def write_centre(name, path, mvs=None):
    """the case written to `path`; mvs: a selection state of that mode where the case itself has none"""
    c = CENTRE_TABLES[name]
    tab, nfac = centre_table(name)
    return write(tab, nfac, path, mvs=mvs or c.get("mvs"), species=c["species"], R=c.get("R", 8), scaling=c.get("scaling", 1.0))


@functools.lru_cache(maxsize=None)
def centre_handles(name):
    """namespace(path, pot, tables, orc, keep) of a case, as tests/_design.handles returns it (which hands these names on to
    here): written once into a directory that lives as long as the process.  Every case must be one the training calls
    accept."""
    from lammps_mtp_kokkos_amd import capi
    from oracle.pyoracle import Oracle
    keep = tempfile.TemporaryDirectory()
    path = write_centre(name, os.path.join(keep.name, name + (".almtp" if CENTRE_TABLES[name].get("mvs") else ".mtp")))
    pot = capi.Potential(path)
    t = pot.train_table()
    assert t["supported"], (name, t["message"])
    return SimpleNamespace(path=path, pot=pot, tables=pot.tables(), orc=Oracle(path), keep=keep)
