"""The numpy twin of the batched force constants (md.hessian_cells; include/mtp_mi355x.h, "batched force constants"), shared by
tests/test_hess_cpu.py and tests/test_hess_gpu.py: mtp_hess_step and mtp_hess_finish rule by rule with the kernels' own
expressions and the kernels' own order of every sum (so that the device can be asked for the same BITS), batches of
configurations on the analytic surface of tests/_neb.py around its saddle, and a host-driven loop that takes the forces of
every explicitly displaced copy from md.evaluate_cells and lets the twin assemble them."""
import numpy as np

import _neb

FAILED = 1
WAVE_ROWS, BLOCK = 256, 256          # MTP_BATCH_WAVE_ROWS, MTP_BATCH_BLOCK


def _butterfly(v, op):
    """the xor butterfly of a wavefront over v [64]: the value every lane ends with"""
    lanes, s = np.arange(64), 1
    while s < 64:
        v = op(v, v[lanes ^ s])
        s <<= 1
    return v[0]


def segment_total(per_thread, op=np.add):
    """batch_step::segment_total over the partials of NT = 64 or 256 threads: the wavefronts' butterflies, combined in wave order"""
    waves = [_butterfly(per_thread[w: w + 64], op) for w in range(0, len(per_thread), 64)]
    total = waves[0]
    for u in waves[1:]:
        total = op(total, u)
    return float(total)


def thread_sums(values, nt):
    """what thread t of nt has after its sweep: values[t] + values[t + nt] + ... in that order, from 0.0"""
    acc = np.zeros(nt)
    for i in range(0, len(values), nt):
        chunk = values[i: i + nt]
        acc[: len(chunk)] = acc[: len(chunk)] + chunk
    return acc


def threads_of(rows):
    return 64 if rows <= WAVE_ROWS else BLOCK


class Twin:
    """the arrays of a pass and its launches.  cfg_first [ncfg + 1] (rows), sel_first [ncfg + 1], sel (row numbers of the batch),
    h; x [n, 3] is the caller's and is displaced and restored in place, x0 its saved copy."""

    def __init__(self, cfg_first, sel_first, sel, h, sel_max=None):
        self.first = np.asarray(cfg_first, dtype=np.int64)
        self.sel_first = np.asarray(sel_first, dtype=np.int64)
        self.sel = np.asarray(sel, dtype=np.int64)
        self.ncfg = len(self.first) - 1
        self.m = np.diff(self.sel_first)
        self.h_first = np.concatenate([[0], np.cumsum((3 * self.m) ** 2)]).astype(np.int64)
        self.H = np.zeros(int(self.h_first[-1]))
        self.sel_max = int(self.m.max(initial=0)) if sel_max is None else int(sel_max)
        self.K = 6 * self.sel_max
        self.h = float(h)
        self.inv2h = 1.0 / (2.0 * self.h)
        n = int(self.first[-1])
        self.f0 = np.zeros((n, 3))
        self.fmax, self.energy = np.zeros(self.ncfg), np.zeros(self.ncfg)
        self.status = np.zeros(self.ncfg, dtype=np.int32)
        self.diag = np.zeros((self.ncfg, 2))

    def matrix(self, j):
        """H_j [3 m, 3 m]: a view"""
        N = 3 * int(self.m[j])
        return self.H[int(self.h_first[j]): int(self.h_first[j]) + N * N].reshape(N, N)

    def step(self, k, x, x0, f, eatom=None, energy=None):
        """launch k.  `energy` [ncfg] stands in for the sums of `eatom` [n] where the caller has only those"""
        h = self.h
        for j in range(self.ncfg):
            r0, r1 = int(self.first[j]), int(self.first[j + 1])
            if r1 == r0 or self.status[j]:
                continue
            s0, m = int(self.sel_first[j]), int(self.m[j])
            rows = self.sel[s0: s0 + m]
            if k == 0:                                                               # 1.
                bad = m > r1 - r0 or m > self.sel_max or bool(((rows < r0) | (rows >= r1)).any())
                fj = f[r0:r1]
                self.f0[r0:r1] = fj
                with np.errstate(all="ignore"):
                    f2 = ((0.0 + fj[:, 0] * fj[:, 0]) + fj[:, 1] * fj[:, 1]) + fj[:, 2] * fj[:, 2]
                    self.fmax[j] = np.sqrt(np.fmax.reduce(f2, initial=0.0))
                    self.energy[j] = (segment_total(thread_sums(eatom[r0:r1], threads_of(r1 - r0))) if energy is None
                                      else energy[j])
                if bad or not np.isfinite(fj).all():
                    self.status[j] = FAILED
                    continue
            else:
                a, d, minus = (k - 1) // 6, ((k - 1) % 6) // 2, (k - 1) & 1
                if a < m:
                    fi = f[rows].reshape(-1)
                    bad = not np.isfinite(fi).all()
                    row = self.matrix(j)[3 * a + d]
                    if not bad:                                                      # 2.
                        row[:] = (fi - row) * self.inv2h if minus else fi
                    x[rows[a], d] = x0[rows[a], d]                                   # 3.
                    if bad:
                        self.status[j] = FAILED
                        continue
            if k < self.K and k // 6 < m:                                            # 4.
                q, d = rows[k // 6], (k % 6) // 2
                x[q, d] = x0[q, d] - h if k & 1 else x0[q, d] + h

    def finish(self, types=None, mass=None, mass_weight=False):
        """mtp_hess_finish: the diagnostics from the matrix as harvested, then H <- 0.5 (H + H^T) (and the mass weights)"""
        for j in range(self.ncfg):
            m = int(self.m[j])
            if m == 0 or self.status[j]:
                continue
            H = self.matrix(j)
            with np.errstate(all="ignore"):
                self.diag[j, 0] = np.fmax.reduce(np.abs(H - H.T)[np.triu_indices(3 * m, 1)], initial=0.0)
                S = np.zeros((3 * m, 3))
                for b in range(m):
                    S = S + H[:, 3 * b: 3 * b + 3]
                self.diag[j, 1] = np.fmax.reduce(np.abs(S).reshape(-1), initial=0.0)
                Hs = 0.5 * (H + H.T)
                if mass_weight:
                    M = np.repeat(np.asarray(mass, dtype=np.float64)[types[self.sel[int(self.sel_first[j]): int(self.sel_first[j]) + m]] - 1], 3)
                    Hs = Hs * (1.0 / np.sqrt(np.outer(M, M)))
            H[:] = Hs

    def run(self, x, forces, types=None, mass=None, mass_weight=False, nan_at=None):
        """a whole pass on x (changed in place and restored): forces(x) -> (eatom [n], f [n, 3]); nan_at = (launch, row, component)
        poisons one force component in front of that launch"""
        x0 = x.copy()
        for k in range(self.K + 1):
            e, f = forces(x)
            if nan_at is not None and nan_at[0] == k:
                f = f.copy()
                f[nan_at[1], nan_at[2]] = np.nan
            self.step(k, x, x0, f, eatom=e)
        self.finish(types, mass, mass_weight)
        return self


# ---- selections --------------------------------------------------------------------------------------------------------------

def selection(cfg_first, mode):
    """(sel_first, sel) over the configurations: mode "none", "one" (a middle atom), "last", "all", or "mixed" (configuration j
    takes the j-th of these in turn; atoms out of order where there are several)"""
    first, out = [0], []
    for j in range(len(cfg_first) - 1):
        r0, r1 = int(cfg_first[j]), int(cfg_first[j + 1])
        mj = ("all", "one", "last", "none", "some")[j % 5] if mode == "mixed" else mode
        if r1 == r0 or mj == "none":
            rows = []
        elif mj == "one":
            rows = [r0 + (r1 - r0) // 2]
        elif mj == "last":
            rows = [r1 - 1]
        elif mj == "some":
            rows = list(range(r1 - 1, r0 - 1, -2))
        else:
            rows = list(range(r0, r1))
        out += rows
        first.append(len(out))
    return np.array(first, dtype=np.int32), np.array(out, dtype=np.int32)


# ---- configurations on the analytic surface of tests/_neb.py, near the saddle of every atom ------------------------------------

def surface_batch(sizes, seed=3, noise=0.02, A=(0.3, 0.7), B=2.0, C=0.6, D=1.5, G=0.05):
    """configurations of sizes[j] atoms (0: an empty one) with u = (0, C, 0) + noise: the arrays of _neb.surface per row, x0, types
    and cfg_first.  A configuration's draws depend on its size and position in `sizes` only through the generator's state."""
    rng = np.random.default_rng(seed)
    rows = dict(site=[], A=[], x0=[], link=[], types=[])
    for n in sizes:
        site = rng.uniform(-20.0, 20.0, (n, 3))
        u = np.zeros((n, 3))
        u[:, 1] = C
        rows["site"].append(site)
        rows["x0"].append(site + u + rng.normal(0.0, noise, (n, 3)))
        rows["A"].append(rng.uniform(A[0], A[1], n))
        rows["link"].append(np.concatenate([np.ones(max(n - 1, 0)), np.zeros(min(n, 1))]))
        rows["types"].append(rng.integers(1, 3, n).astype(np.int32))
    S = {k: np.concatenate(v) for k, v in rows.items()}
    n = len(S["A"])
    S.update(B=np.full(n, float(B)), C=np.full(n, float(C)), D=np.full(n, float(D)), G=np.full(n, float(G)),
             cfg_first=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    return S


def sub_batch(S, which):
    """the configurations `which` of S as a batch of their own: the same bits, rows renumbered"""
    keys = ("site", "A", "x0", "link", "types", "B", "C", "D", "G")
    pick = [np.arange(int(S["cfg_first"][j]), int(S["cfg_first"][j + 1])) for j in which]
    rows = np.concatenate(pick) if pick else np.zeros(0, dtype=np.int64)
    T = {k: S[k][rows] for k in keys}
    T["cfg_first"] = np.concatenate([[0], np.cumsum([len(p) for p in pick])]).astype(np.int32)
    return T


def surface_forces(S):
    consts = [S[k] for k in _neb.SURFACE_KEYS]
    return lambda x: _neb.surface(np, x, *consts)


def run_surface(S, mode="all", h=0.01, mass_weight=False, nan_at=None):
    """the twin over the batch S with the surface's forces in numpy; returns the twin and x after the pass"""
    sel_first, sel = selection(S["cfg_first"], mode)
    x = S["x0"].copy()
    twin = Twin(S["cfg_first"], sel_first, sel, h).run(x, surface_forces(S), S["types"], _neb.SURFACE_MASSES, mass_weight, nan_at)
    return twin, x


# ---- the host-driven loop ------------------------------------------------------------------------------------------------------

def reference_loop(ctx, configs, h=0.01, atoms=None, masses=183.84, mass_weight=False, list_cutoff=7.0):
    """md.hessian_cells driven from the host: one md.evaluate_cells call per displacement over explicitly displaced copies of
    all configurations (positions as given, never wrapped), assembled by the twin.  Returns the twin (matrix(j), f0, fmax,
    energy, diag, status) and the number of evaluate_cells calls."""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    natoms = np.array([len(c[0]) for c in configs])
    first = np.concatenate([[0], np.cumsum(natoms)]).astype(np.int64)
    types = np.concatenate([np.asarray(c[2], dtype=np.int64).reshape(-1) for c in configs])
    mass_of_type = np.atleast_1d(np.asarray(masses, dtype=np.float64))
    if len(mass_of_type) == 1:
        mass_of_type = np.full(max(int(types.max(initial=1)), 1), mass_of_type[0])
    atoms = [None] * len(configs) if atoms is None else atoms
    picks = [np.arange(natoms[j]) if a is None else np.asarray(a, dtype=np.int64) for j, a in enumerate(atoms)]
    sel = np.concatenate([first[j] + p for j, p in enumerate(picks)]).astype(np.int64)
    sel_first = np.concatenate([[0], np.cumsum([len(p) for p in picks])])
    x = np.concatenate([np.asarray(c[0], dtype=np.float64).reshape(-1, 3) for c in configs]).copy()
    x0 = x.copy()
    twin = Twin(first, sel_first, sel, h)
    for k in range(twin.K + 1):
        res = evaluate_cells(ctx, [(x[first[j]: first[j + 1]], c[1], c[2]) for j, c in enumerate(configs)], list_cutoff=list_cutoff,
                             vflag=0)
        twin.step(k, x, x0, np.concatenate([r["f"] for r in res]), energy=np.array([r["energy"] for r in res]))
    assert np.array_equal(x, x0)
    twin.finish(types, mass_of_type, mass_weight)
    return twin, twin.K + 1
