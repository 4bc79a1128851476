"""The numpy twin of the batched constant-pressure sampler (md.sample_cells_npt; include/mtp_mi355x.h, "batched
constant-pressure sampling"), shared by tests/test_sample_npt_cpu.py and tests/test_sample_npt_gpu.py: mtp_sample_cell_step
rule by rule, vectorised over the configurations, the barostat's noise from the Philox twin of tests/_sample.py, an equal-size
vectorised evaluation of the analytic model of tests/_relax_vc.py, and a host-driven loop that takes energies, forces, virials
and grades from one md.evaluate_cells call per step at the current cells.  Row-vector convention: a cell has the lattice
vectors as rows, x = s . h, W = -dE/d(eps) for x -> x (I + eps) in the order xx yy zz xy xz yz."""
import numpy as np

import _sample
from _relax_vc import CAPTURED, FAILED, VOIGT, images
from _sample import FTM2V, KB, MVV2E

NOISE_INDEX = 0x80000000                                      # the barostat's counters: (step, NOISE_INDEX + j, key lo, key hi)


def det3(h):
    """determinants of [..., 3, 3] arrays, the products of the kernel"""
    return (h[..., 0, 0] * (h[..., 1, 1] * h[..., 2, 2] - h[..., 1, 2] * h[..., 2, 1])
            - h[..., 0, 1] * (h[..., 1, 0] * h[..., 2, 2] - h[..., 1, 2] * h[..., 2, 0])
            + h[..., 0, 2] * (h[..., 1, 0] * h[..., 2, 1] - h[..., 1, 1] * h[..., 2, 0]))


def sym(a6):
    """[..., 6] (xx yy zz xy xz yz) -> symmetric [..., 3, 3]"""
    a6 = np.asarray(a6)
    m = np.zeros(a6.shape[:-1] + (3, 3), dtype=a6.dtype)
    for q, (a, b) in enumerate(VOIGT):
        m[..., a, b] = m[..., b, a] = a6[..., q]
    return m


def counters(step, keys):
    """the barostat's Philox counters [ncfg, 2, 4] at `step` for the configuration keys [ncfg] uint64"""
    keys = np.asarray(keys, dtype=np.uint64)
    c = np.zeros((len(keys), 2, 4), dtype=np.uint64)
    c[:, :, 0] = step
    c[:, 0, 1], c[:, 1, 1] = NOISE_INDEX, NOISE_INDEX + 1
    c[:, :, 2] = (keys & _sample.M32)[:, None]
    c[:, :, 3] = (keys >> np.uint64(32))[:, None]
    return c


def noise(step, keys, seed):
    """xi [ncfg, 6] (xx yy zz xy xz yz): sqrt(12) (u - 0.5), zero mean, unit variance"""
    seed = int(seed) & (2 ** 64 - 1)
    w = _sample.philox4x32_10(counters(step, keys), np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))
    u = (w[:, :, :3].astype(np.float64) + 0.5) * 2.0 ** -32
    return (np.sqrt(12.0) * (u - 0.5)).reshape(len(w), 6)


def exp_series(A, sign):
    """I + sign A + A^2/2 + sign A^3/6 + A^4/24, [..., 3, 3], in the kernel's order"""
    A2 = A @ A
    A3, A4 = A2 @ A, A2 @ A2
    return (((np.eye(3) + sign * A) + A2 / 2.0) + sign * (A3 / 6.0)) + A4 / 24.0


class Twin:
    """the per-configuration state of mtp_sample_cell_step and the step itself.  cfg_first [ncfg + 1], cells [ncfg, 3, 3];
    temperature, keys [ncfg]; m, inv_m [n] per row.  x, v [n, 3] are the caller's and updated in place.  with_kt=False leaves
    the `+ kT I` term out of the drift (the negative control of the ideal-gas test)."""

    def __init__(self, cfg_first, cells, temperature, keys, dt, pressure, compressibility, tau_p=1.0, cell_mask=(1, 1, 1, 1, 1, 1),
                 isotropic=False, strain_max=0.01, seed=0, origins=None, frozen=None, rghost=7.0, with_kt=True):
        self.first = np.asarray(cfg_first, dtype=np.int64)
        ncfg = self.ncfg = len(self.first) - 1
        self.sizes = np.diff(self.first)
        self.cfg_row = np.repeat(np.arange(ncfg), self.sizes)
        self.h = np.array(cells, dtype=np.float64).reshape(ncfg, 3, 3)
        self.V0 = det3(self.h)
        self.kT = KB * np.broadcast_to(np.asarray(temperature, dtype=np.float64), (ncfg,)).copy()
        self.keys = np.asarray(keys, dtype=np.uint64)
        self.dt, self.dtf = float(dt), 0.5 * float(dt) * FTM2V
        self.pressure, self.compressibility, self.strain_max, self.seed = float(pressure), float(compressibility), float(strain_max), seed
        self.mask6 = np.array([int(q) for q in cell_mask], dtype=bool)
        self.isotropic, self.with_kt = bool(isotropic), bool(with_kt)
        if self.isotropic and not self.mask6[:3].all():
            raise ValueError("isotropic needs the three diagonal mask entries")
        self.tau_p = None if tau_p is None or not np.isfinite(tau_p) or tau_p <= 0.0 else float(tau_p)
        self.barostat = self.tau_p is not None and bool(self.mask6.any())
        self.origins = np.zeros((ncfg, 3)) if origins is None else np.array(origins, dtype=np.float64)
        self.rghost = rghost
        self.T = np.tile(np.eye(3), (ncfg, 1, 1))
        self.F = np.tile(np.eye(3), (ncfg, 1, 1))             # the product of every E: h . h0^-1 in exact arithmetic
        self.href = self.h.copy()
        with np.errstate(all="ignore"):
            self.nimg = np.array([images(c, rghost) for c in self.h]).reshape(ncfg, 3)
        self.cellmove = np.zeros(ncfg)
        self.frozen = np.zeros(ncfg, dtype=np.int32) if frozen is None else np.array(frozen, dtype=np.int32)
        self.done_step = np.full(ncfg, -1, dtype=np.int32)
        self.capped = np.zeros(ncfg, dtype=np.int32)
        self.press = np.zeros(ncfg)
        self.count = 0
        self.margin_cap = np.inf                              # how close a component came to a tie with strain_max (relative)

    def kinetic(self, m, vk):
        kt = np.zeros((self.ncfg, 6))
        for q, (a, b) in enumerate(VOIGT):
            kt[:, q] = MVV2E * np.bincount(self.cfg_row, weights=m * vk[:, a] * vk[:, b], minlength=self.ncfg)
        return kt

    def step(self, step, x, v, f, W, m, inv_m):
        ncfg, row = self.ncfg, self.cfg_row
        W = np.asarray(W, dtype=np.float64).reshape(ncfg, 6)
        with np.errstate(all="ignore"):
            vk = v + (self.dtf * inv_m)[:, None] * f
            kt = self.kinetic(m, vk)
            V = det3(self.h)
            active = (self.sizes > 0) & (self.frozen == 0)
            ok = np.isfinite(W).all(1) & np.isfinite(kt).all(1) & np.isfinite(V) & (V > 0.0) & np.isfinite(self.V0) & (self.V0 > 0.0)
            failed = active & ~ok
            self.frozen[failed], self.done_step[failed] = FAILED, step
            self.count += int(failed.sum())
            go = active & ok
            wt = W + kt
            self.press[go] = (((wt[:, 0] + wt[:, 1]) + wt[:, 2]) / (3.0 * V))[go]
            rows = go[row]
            if not self.barostat:
                v[rows] = vk[rows]
                x[rows] = (x + self.dt * vk)[rows]
                return
            c = self.compressibility / (3.0 * self.tau_p * self.V0) * self.dt
            s = np.sqrt(2.0 * self.kT * c)
            xi = noise(step, self.keys, self.seed)
            drift = wt.copy()
            drift[:, :3] = (wt[:, :3] - (self.pressure * V)[:, None]) + (self.kT[:, None] if self.with_kt else 0.0)
            xi[:, 3:] = xi[:, 3:] * np.sqrt(0.5)
            a6 = np.where(self.mask6, c[:, None] * drift + s[:, None] * xi, 0.0)
            if self.isotropic:
                a6[:, :3] = (((a6[:, 0] + a6[:, 1]) + a6[:, 2]) / 3.0)[:, None]
                a6[:, 3:] = 0.0
            over = np.abs(a6) > self.strain_max
            self.margin_cap = min(self.margin_cap, float(np.abs(np.abs(a6[go]) / self.strain_max - 1.0).min(initial=np.inf)))
            a6 = np.where(over, np.copysign(self.strain_max, a6), a6)
            self.capped[go & over.any(1)] += 1
            A = sym(a6)
            E, Einv = exp_series(A, 1.0), exp_series(A, -1.0)
            org = self.origins[row]
            d = (x - org) + self.dt * vk
            x[rows] = (org + np.einsum("ia,iab->ib", d, E[row]))[rows]
            v[rows] = np.einsum("ia,iab->ib", vk, Einv[row])[rows]
            self.h[go] = (self.h @ E)[go]
            self.T[go] = (self.T @ E)[go]
            self.F[go] = (self.F @ E)[go]
            move = ((self.nimg + 1) * np.sqrt(((self.h - self.href) ** 2).sum(2))).sum(1)
            self.cellmove[go] = move[go]


# ---- the analytic model of tests/_relax_vc.py for configurations of ONE size, all at once ------------------------------------

def model_all(model, x, h):
    """_relax_vc.Model.all for a model whose configurations all have the same size: energies [ncfg], f [n, 3], W [ncfg, 6]"""
    ncfg, n = model.ncfg, model.n // model.ncfg
    xs, s0 = x.reshape(ncfg, n, 3), model.s0.reshape(ncfg, n, 3)
    d = xs - s0 @ h
    mm = h @ h.transpose(0, 2, 1) - model.geq
    e = 0.5 * model.k * (d * d).sum((1, 2)) + 0.25 * model.k2 * (mm * mm).sum((1, 2))
    w = -model.k[:, None, None] * (d.transpose(0, 2, 1) @ d) - model.k2[:, None, None] * (h.transpose(0, 2, 1) @ mm @ h)
    return e, (-model.k[:, None, None] * d).reshape(-1, 3), np.stack([w[:, a, b] for a, b in VOIGT], axis=1)


def block_error(series, nblocks=16):
    """mean and block-averaged standard error of a series [samples, ...] (blocks of consecutive samples)"""
    series = np.asarray(series, dtype=np.float64)
    n = len(series) // nblocks * nblocks
    blocks = series[:n].reshape((nblocks, n // nblocks) + series.shape[1:]).mean(1)
    return series[:n].mean(0), blocks.std(0, ddof=1) / np.sqrt(nblocks)


# ---- the host-driven loop -----------------------------------------------------------------------------------------------

def reference_loop(evaluate, configs, temperature, pressure, steps, dt, velocities, keys, masses, compressibility, tau_p=1.0,
                   t_damp=0.1, seed=0, grade_every=0, select=2.0, brk=10.0, gap=0, max_candidates=10 ** 9, **kw):
    """md.sample_cells_npt driven from the host: energy, forces, virial and grades of every step from ONE `evaluate` call
    (_relax_vc.evaluate_with) at the current cells, the first half and the barostat by the twin, the second half and the capture
    by tests/_sample.py.  Positions are kept unwrapped, without origins.  Returns dict(x, v, cells: per step lists, step 0 first;
    energy, kinetic, volume, pressure [steps + 1, ncfg]; grades {step: [ncfg]}; capture; snapshots [(x, cell)]; twin; virial
    [ncfg, 6] of the last evaluation)."""
    ncfg = len(configs)
    natoms = np.array([len(c[0]) for c in configs])
    first = np.concatenate([[0], np.cumsum(natoms)])
    types = np.concatenate([np.asarray(c[2], dtype=np.int64) for c in configs])
    mass_of_type = np.atleast_1d(np.asarray(masses, dtype=np.float64))
    if len(mass_of_type) == 1:
        mass_of_type = np.full(max(int(types.max()), 1), mass_of_type[0])
    m, inv_m = mass_of_type[types - 1], (1.0 / mass_of_type)[types - 1]
    temps = np.broadcast_to(np.asarray(temperature, dtype=np.float64), (ncfg,))
    T_row = _sample.rows_of(configs, temps)
    key_row = _sample.rows_of(configs, np.asarray(keys, dtype=np.uint64)).astype(np.uint64)
    index = np.concatenate([np.arange(n) for n in natoms]).astype(np.uint64)
    x = np.concatenate([np.asarray(c[0], dtype=np.float64).reshape(-1, 3) for c in configs]).copy()
    v = np.concatenate([np.asarray(q, dtype=np.float64).reshape(-1, 3) for q in velocities]).copy()
    cap = _sample.Capture(natoms, select, brk, gap, max_candidates)
    twin = Twin(first, np.array([c[1] for c in configs]), temps, keys, dt, pressure, compressibility, tau_p, seed=seed, **kw)
    dtf = twin.dtf
    split = lambda a: [a[first[k]:first[k + 1]].copy() for k in range(ncfg)]
    out = dict(x=[], v=[], cells=[], energy=np.zeros((steps + 1, ncfg)), kinetic=np.zeros((steps + 1, ncfg)),
               volume=np.zeros((steps + 1, ncfg)), pressure=np.zeros((steps + 1, ncfg)), grades={}, capture=cap, twin=twin, snapshots=[])

    def evaluate_at(step):
        graded = bool(grade_every) and step % grade_every == 0
        res = evaluate([(x[first[k]:first[k + 1]], twin.h[k], c[2]) for k, c in enumerate(configs)], graded)
        out["energy"][step] = [r["energy"] for r in res]
        g = np.array([r["cfg_grade"] if "cfg_grade" in r else r["max_grade"] for r in res]) if graded else None
        return np.concatenate([r["f"] for r in res]).copy(), np.array([r["virial"] for r in res]).reshape(ncfg, 6), g

    def after(step, g, W):
        if g is not None:
            out["grades"][step] = g
            cap.frozen = twin.frozen != 0
            for k in cap.step(step, g):
                out["snapshots"].append((x[first[k]:first[k + 1]].copy(), twin.h[k].copy()))
            twin.frozen[cap.frozen & (twin.frozen == 0)] = CAPTURED
        out["x"].append(split(x))
        out["v"].append(split(v))
        out["cells"].append(twin.h.copy())
        mv2 = np.array([(m[first[k]:first[k + 1], None] * v[first[k]:first[k + 1]] ** 2).sum() for k in range(ncfg)])
        out["kinetic"][step] = 0.5 * MVV2E * mv2
        out["volume"][step] = det3(twin.h)
        out["pressure"][step] = (W[:, :3].sum(1) + MVV2E * mv2) / (3.0 * out["volume"][step])

    f, W, g = evaluate_at(0)
    moving = twin.frozen[twin.cfg_row] == 0
    _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, 0.0, 0, index, key_row, seed, moving)
    after(0, g, W)
    for step in range(1, steps + 1):
        twin.step(step, x, v, f, W, m, inv_m)
        moving = twin.frozen[twin.cfg_row] == 0
        f, W, g = evaluate_at(step)
        _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, dtf, step, index, key_row, seed, moving)
        after(step, g, W)
    out["virial"] = W
    return out
