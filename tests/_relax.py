"""The numpy twin of the batched minimiser (md.relax_cells; include/mtp_mi355x.h, "batched relaxation"), shared by
tests/test_relax_cpu.py and tests/test_relax_gpu.py: mtp_relax_step rule by rule, the two tie margins of a run, the
harmonic wells of the kernel tests, and a host-driven reference loop that takes forces, energies and grades from
md.evaluate_cells, captures with tests/_sample.py's Capture and minimises with the twin."""
import numpy as np

import _sample
from _sample import FTM2V

RUNNING, CAPTURED, CONVERGED, FAILED = 0, 1, 2, 3
DEFAULTS = dict(ftol=1e-3, dt_max=1e-2, dmax=0.1, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, n_min=5)
MARGIN = 1e-6


class Twin:
    """the per-configuration state of mtp_relax_step and the step itself.  cfg_first [ncfg + 1]; x, v, f [n, 3] are the
    caller's and x, v are updated in place; inv_m [n] per row."""

    def __init__(self, cfg_first, dt, frozen=None, **params):
        self.p = dict(DEFAULTS, **params)
        self.first = np.asarray(cfg_first, dtype=np.int64)
        ncfg = len(self.first) - 1
        self.dt = np.full(ncfg, float(dt))
        self.alpha = np.full(ncfg, float(self.p["alpha_start"]))
        self.npos = np.zeros(ncfg, dtype=np.int32)
        self.frozen = np.zeros(ncfg, dtype=np.int32) if frozen is None else np.array(frozen, dtype=np.int32)
        self.done_step = np.full(ncfg, -1, dtype=np.int32)
        self.fmax = np.zeros(ncfg)
        self.count = 0                      # what the kernel adds to counts[2]
        self.uphill = self.capped = 0       # events over the run
        self.margin_p = self.margin_tol = np.inf

    def step(self, step, x, v, f, inv_m, last=False):
        p = self.p
        for k in range(len(self.dt)):
            a0, a1 = int(self.first[k]), int(self.first[k + 1])
            if a1 == a0 or self.frozen[k]:
                continue
            fk, vk = f[a0:a1], v[a0:a1]
            with np.errstate(invalid="ignore", over="ignore"):
                P, vv = float((fk * vk).sum()), float((vk * vk).sum())
                f2 = (fk * fk).sum(1)
                ff, fmax2 = float(f2.sum()), float(np.fmax.reduce(f2, initial=0.0))
            self.fmax[k] = np.sqrt(fmax2)
            tol2 = p["ftol"] * p["ftol"]
            if not np.isfinite(ff):
                self.frozen[k], self.done_step[k] = FAILED, step
                self.count += 1
                continue
            if tol2 > 0.0:
                self.margin_tol = min(self.margin_tol, abs(fmax2 - tol2) / tol2)
            if fmax2 <= tol2:
                self.frozen[k], self.done_step[k] = CONVERGED, step
                self.count += 1
                v[a0:a1] = 0.0
                continue
            if last:
                continue
            if vv > 0.0:
                self.margin_p = min(self.margin_p, abs(P) / np.sqrt(vv * ff))
            if P > 0.0:
                a, b = 1.0 - self.alpha[k], self.alpha[k] * np.sqrt(vv / ff)
                self.npos[k] += 1
                if self.npos[k] > p["n_min"]:
                    self.dt[k] = min(self.dt[k] * p["f_inc"], p["dt_max"])
                    self.alpha[k] *= p["f_alpha"]
            else:
                a = b = 0.0
                self.npos[k] = 0
                self.alpha[k] = p["alpha_start"]
                if vv > 0.0:
                    self.dt[k] *= p["f_dec"]
                    self.uphill += 1
            vm = a * vk + b * fk
            vmax = float(np.abs(vm).max())
            dtv = self.dt[k]
            if dtv * vmax > p["dmax"]:
                dtv = p["dmax"] / vmax
                self.capped += 1
            x[a0:a1] += dtv * vm
            v[a0:a1] = vm + ((dtv * FTM2V) * inv_m[a0:a1])[:, None] * fk

    def assert_margins(self):
        """rounding is 1e-12: with both margins above 1e-6 no decision of the run can flip between twin and device"""
        assert self.margin_p >= MARGIN and self.margin_tol >= MARGIN, \
            "the test's inputs are wrong: a decision is a tie (P margin %.3e, tolerance margin %.3e)" % (self.margin_p, self.margin_tol)


# ---- anisotropic harmonic wells: f = -k_cfg (1, 4, 16) (x - x_eq) ------------------------------------------------------------

WELL_SIZES = [0, 1, 63, 64, 65, 256, 257]
WELL_K = (2.0, 5.0, 9.0, 2.0, 5.0, 9.0, 2.0)
WELL_MASSES = np.array([183.84, 186.207])


def wells(sizes=WELL_SIZES, k_cfg=WELL_K, seed=8):
    """cfg_first, types, x_eq, x0 and the stiffness per coordinate kk [n, 3] (draw order: types, x_eq, the offset of x0)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    cf = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(cf[-1])
    rng = np.random.default_rng(seed)
    types = rng.integers(1, 3, n).astype(np.int32)
    x_eq = rng.normal(0.0, 3.0, (n, 3))
    x0 = x_eq + rng.normal(0.0, 0.3, (n, 3))
    kk = np.repeat(np.asarray(k_cfg, dtype=np.float64)[: len(sizes)], sizes)[:, None] * np.array([1.0, 4.0, 16.0])
    return cf, types, x_eq, x0, kk


def well_force(x, x_eq, kk):
    return -(kk * (x - x_eq))


def well_energy(x, x_eq, kk, cf):
    e = 0.5 * (kk * (x - x_eq) ** 2).sum(1)
    return np.array([e[cf[k]:cf[k + 1]].sum() for k in range(len(cf) - 1)])


def run_wells(cf, types, x_eq, x0, kk, steps, dt=1e-3, frozen=None, nan_at=None, keep=(), **params):
    """the twin on the wells for steps 0 .. steps - 1 (every one of them moves).  nan_at = (step, row, component) poisons one
    force component of that step.  Returns the twin, x, v and {step: (x, v, dt, alpha, fmax, frozen) copies} for `keep`."""
    twin = Twin(cf, dt, frozen=frozen, **params)
    inv_m = (1.0 / WELL_MASSES)[types - 1]
    x, v = x0.copy(), np.zeros_like(x0)
    kept = {}
    for s in range(steps):
        f = well_force(x, x_eq, kk)
        if nan_at is not None and nan_at[0] == s:
            f[nan_at[1], nan_at[2]] = np.nan
        twin.step(s, x, v, f, inv_m)
        if s in keep:
            kept[s] = (x.copy(), v.copy(), twin.dt.copy(), twin.alpha.copy(), twin.fmax.copy(), twin.frozen.copy())
    return twin, x, v, kept


# ---- the host-driven loop -----------------------------------------------------------------------------------------------

def reference_loop(ctx, configs, steps, dt=1e-3, masses=183.84, grade_every=0, select=2.0, brk=10.0, gap=0,
                   max_candidates=10 ** 9, list_cutoff=7.0, **params):
    """md.relax_cells driven from the host: forces, energies and grades of every step from md.evaluate_cells (one call a
    step), capture by _sample.Capture BEFORE the twin, the move by the twin; the launch of step `steps` only decides.  Stops
    after the step at which every non-empty configuration is frozen.  Returns dict(x: per step lists of per-configuration
    arrays (the positions the forces of that step were taken at); energy, fmax [steps_done + 1, ncfg]; grades {step: [ncfg]};
    capture; twin; status, done_step, dt [ncfg]; final_x; steps_done)."""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    ncfg = len(configs)
    natoms = np.array([len(c[0]) for c in configs])
    first = np.concatenate([[0], np.cumsum(natoms)])
    types = np.concatenate([np.asarray(c[2], dtype=np.int64) for c in configs]) if ncfg else np.zeros(0, dtype=np.int64)
    mass_of_type = np.atleast_1d(np.asarray(masses, dtype=np.float64))
    if len(mass_of_type) == 1:
        mass_of_type = np.full(max(int(types.max()) if len(types) else 1, 1), mass_of_type[0])
    inv_m = (1.0 / mass_of_type)[types - 1]
    x = np.concatenate([np.asarray(c[0], dtype=np.float64).reshape(-1, 3) for c in configs]).copy()
    v = np.zeros_like(x)
    cap = _sample.Capture(natoms, select, brk, gap, max_candidates)
    twin = Twin(first, dt, **params)
    split = lambda a: [a[first[k]:first[k + 1]].copy() for k in range(ncfg)]
    out = dict(x=[], energy=[], fmax=[], grades={}, capture=cap, twin=twin, snapshots=[])
    for s in range(steps + 1):
        graded = bool(grade_every) and s % grade_every == 0
        res = evaluate_cells(ctx, [(x[first[k]:first[k + 1]], c[1], c[2]) for k, c in enumerate(configs)], list_cutoff=list_cutoff,
                             vflag=0, grades=graded)
        f = np.concatenate([r["f"] for r in res]).copy()
        out["x"].append(split(x))
        out["energy"].append([r["energy"] for r in res])
        if graded:
            g = np.array([r["cfg_grade"] if "cfg_grade" in r else r["max_grade"] for r in res])
            out["grades"][s] = g
            cap.frozen = twin.frozen != 0
            for k in cap.step(s, g):
                out["snapshots"].append(x[first[k]:first[k + 1]].copy())
            twin.frozen[cap.frozen & (twin.frozen == 0)] = CAPTURED
        twin.step(s, x, v, f, inv_m, last=s == steps)
        out["fmax"].append(twin.fmax.copy())
        if ((twin.frozen != 0) | (natoms == 0)).all():
            break
    out.update(energy=np.array(out["energy"]), fmax=np.array(out["fmax"]), status=twin.frozen.copy(), done_step=twin.done_step.copy(),
               dt=twin.dt.copy(), final_x=split(x), steps_done=s)
    return out
