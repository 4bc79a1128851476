"""The numpy twin of the batched sampler (md.sample_cells; include/mtp_mi355x.h, "batched sampling"), shared by
tests/test_sample_cpu.py and tests/test_sample_gpu.py: Philox4x32-10, the two half steps with fix langevin's force, the
capture and freeze rules with their slot order, and a host-driven reference loop that takes forces and grades from
md.evaluate_cells and integrates with the twin."""
import numpy as np

MVV2E = 1.0364269e-4
FTM2V = 1.0 / MVV2E
KB = 8.617343e-5
M32 = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcast against each other) as integers below 2^32 -> output words [..., 4] uint32"""
    c = np.asarray(counter, dtype=np.uint64) & M32
    k = np.asarray(key, dtype=np.uint64) & M32
    c0, c1, c2, c3 = (c[..., q].copy() for q in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def noise(step, index, key64, seed):
    """u - 0.5 [n, 3] of the atoms with in-configuration indices `index` [n] and configuration keys `key64` [n] at `step`"""
    index = np.asarray(index, dtype=np.uint64)
    key64 = np.broadcast_to(np.asarray(key64, dtype=np.uint64), index.shape)
    ctr = np.stack([np.full(index.shape, step, dtype=np.uint64), index, key64 & M32, key64 >> np.uint64(32)], axis=-1)
    seed = int(seed) & (2 ** 64 - 1)
    w = philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))
    return (w[:, :3].astype(np.float64) + 0.5) * 2.0 ** -32 - 0.5


def first_half(x, v, f, inv_m, dtf, dt, moving):
    """v += dtf f / m; x += dt v on the rows where `moving`; the others are left as they are.  In place."""
    vv = v + (dtf * inv_m)[:, None] * f
    v[moving] = vv[moving]
    x[moving] = (x + dt * vv)[moving]


def second_half(v, f, m, inv_m, T_row, t_damp, dt, dtf, step, index, key_row, seed, moving):
    """fix langevin's force (f is modified in place) and the second kick, on the rows where `moving`"""
    if t_damp and t_damp > 0 and np.isfinite(t_damp):
        g1 = -m / t_damp / FTM2V
        g2 = np.sqrt(m) * np.sqrt(24.0 * KB * T_row / t_damp / dt / MVV2E) / FTM2V
        fn = f + g1[:, None] * v + g2[:, None] * noise(step, index, key_row, seed)
        f[moving] = fn[moving]
    vv = v + (dtf * inv_m)[:, None] * f
    v[moving] = vv[moving]


class Capture:
    """the capture and freeze rules of mtp_sample_capture: slots in ascending (step, configuration) order, a full buffer
    drops whole snapshots, a NaN grade captures and freezes, an empty or frozen configuration is never captured"""

    def __init__(self, natoms, select, brk, gap, max_candidates):
        self.natoms = np.asarray(natoms)
        self.select, self.brk, self.gap, self.max = select, brk, gap, max_candidates
        self.frozen = np.zeros(len(self.natoms), dtype=bool)
        self.last = np.full(len(self.natoms), -2 ** 30, dtype=np.int64)
        self.records, self.dropped = [], 0

    def step(self, step, grades):
        """returns the configurations captured at this step (those whose snapshot is to be taken)"""
        taken = []
        for k, g in enumerate(grades):
            if self.frozen[k] or self.natoms[k] == 0 or g < self.select or step - self.last[k] < self.gap:
                continue
            if len(self.records) >= self.max:
                self.dropped += 1
                continue
            self.records.append((k, step, float(g)))
            self.last[k] = step
            taken.append(k)
            if not g < self.brk:
                self.frozen[k] = True
        return taken


def rows_of(configs, per_cfg):
    return np.concatenate([np.full(len(c[0]), per_cfg[k]) for k, c in enumerate(configs)]) if len(configs) else np.zeros(0)


def wrapped_diff(a, b, cell):
    """max |a - b| modulo the lattice of `cell` (rows = lattice vectors)"""
    if not len(a):
        return 0.0
    d = np.asarray(a) - np.asarray(b)
    d = d - np.round(d @ np.linalg.inv(cell)) @ cell
    return float(np.abs(d).max())


def reference_loop(ctx, configs, temperature, steps, dt, velocities, keys, masses, t_damp=0.1, seed=0, grade_every=0,
                   select=2.0, brk=10.0, gap=0, max_candidates=10 ** 9, list_cutoff=7.0):
    """md.sample_cells driven from the host: forces, energies and grades of every step from md.evaluate_cells (one call per
    step), integration and capture by the twin.  Returns dict(x, v: per step lists of per-configuration arrays, step 0
    first; energy, kinetic [steps + 1, ncfg]; grades {step: [ncfg]}; capture: the Capture; snapshots: positions per record)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    ncfg = len(configs)
    natoms = np.array([len(c[0]) for c in configs])
    first = np.concatenate([[0], np.cumsum(natoms)])
    types = np.concatenate([np.asarray(c[2], dtype=np.int64) for c in configs])
    mass_of_type = np.atleast_1d(np.asarray(masses, dtype=np.float64))
    if len(mass_of_type) == 1:
        mass_of_type = np.full(max(int(types.max()), 1), mass_of_type[0])
    m = mass_of_type[types - 1]
    inv_m = (1.0 / mass_of_type)[types - 1]
    T_row = rows_of(configs, np.broadcast_to(np.asarray(temperature, dtype=np.float64), (ncfg,)))
    key_row = rows_of(configs, np.asarray(keys, dtype=np.uint64)).astype(np.uint64)
    index = np.concatenate([np.arange(n) for n in natoms]).astype(np.uint64)
    cfg_row = rows_of(configs, np.arange(ncfg)).astype(np.int64)
    x = np.concatenate([np.asarray(c[0], dtype=np.float64).reshape(-1, 3) for c in configs]).copy()
    v = np.concatenate([np.asarray(q, dtype=np.float64).reshape(-1, 3) for q in velocities]).copy()
    cap = Capture(natoms, select, brk, gap, max_candidates)
    dtf = 0.5 * dt * FTM2V
    split = lambda a: [a[first[k]:first[k + 1]].copy() for k in range(ncfg)]
    out = dict(x=[], v=[], energy=np.zeros((steps + 1, ncfg)), kinetic=np.zeros((steps + 1, ncfg)), grades={}, capture=cap,
               snapshots=[])

    def evaluate(step):
        graded = bool(grade_every) and step % grade_every == 0
        res = evaluate_cells(ctx, [(x[first[k]:first[k + 1]], c[1], c[2]) for k, c in enumerate(configs)], list_cutoff=list_cutoff,
                             vflag=0, grades=graded)
        f = np.concatenate([r["f"] for r in res]).copy()
        out["energy"][step] = [r["energy"] for r in res]
        return f, (np.array([r["cfg_grade"] if "cfg_grade" in r else r["max_grade"] for r in res]) if graded else None)

    def after(step, g):
        if g is not None:
            out["grades"][step] = g
            for k in cap.step(step, g):
                out["snapshots"].append(x[first[k]:first[k + 1]].copy())
        out["x"].append(split(x))
        out["v"].append(split(v))
        out["kinetic"][step] = [0.5 * MVV2E * (m[first[k]:first[k + 1], None] * v[first[k]:first[k + 1]] ** 2).sum() for k in range(ncfg)]

    f, g = evaluate(0)
    moving = ~cap.frozen[cfg_row]
    if t_damp and t_damp > 0:                                 # fix langevin's setup: the thermostat force of step 0, no kick
        second_half(v, f, m, inv_m, T_row, t_damp, dt, 0.0, 0, index, key_row, seed, moving)
    after(0, g)
    for step in range(1, steps + 1):
        moving = ~cap.frozen[cfg_row]
        first_half(x, v, f, inv_m, dtf, dt, moving)
        f, g = evaluate(step)
        second_half(v, f, m, inv_m, T_row, t_damp, dt, dtf, step, index, key_row, seed, moving)
        after(step, g)
    return out
