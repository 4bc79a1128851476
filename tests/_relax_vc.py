"""The numpy twin of the batched variable-cell minimiser (md.relax_cells_vc; include/mtp_mi355x.h, "batched variable-cell
relaxation"), shared by tests/test_relax_vc_cpu.py and tests/test_relax_vc_gpu.py: mtp_relax_cell_step rule by rule with
the four tie margins of a run, an analytic model whose symmetric virial derives from an energy, the rebuild measure, and a
host-driven loop that takes energies, forces, virials and grades from one md.evaluate_cells call per step at the current
cells.  Row-vector convention: a cell has the lattice vectors as rows, x = s . h, W = -dE/d(eps) for x -> x (I + eps) in the
order xx yy zz xy xz yz."""
import numpy as np

import _sample
from _relax import CAPTURED, CONVERGED, DEFAULTS, FAILED, MARGIN, RUNNING  # noqa: F401
from _sample import FTM2V

GPA = 1.0 / 160.21766
VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def sym(w6):
    m = np.zeros((3, 3))
    for q, (a, b) in enumerate(VOIGT):
        m[a, b] = m[b, a] = w6[q]
    return m


def voigt(m):
    return np.array([m[a, b] for a, b in VOIGT])


def det3(m):
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def inv3(m, det):
    """cofactors over the determinant, the products of the kernel (diagonal matrices stay diagonal to the bit)"""
    c = np.array([[m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                  [m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2], m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                  [m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]])
    return c / det


def images(cell, rghost):
    """mtp_ghosts_cell_bounds' nimage: ceil(rghost / plane spacing) per direction"""
    cell = np.asarray(cell, dtype=np.float64)
    cross = np.array([np.cross(cell[1], cell[2]), np.cross(cell[2], cell[0]), np.cross(cell[0], cell[1])])
    return np.ceil(rghost * np.sqrt((cross ** 2).sum(1)) / det3(cell)).astype(np.int64)


def cell_move(h, href, nimg):
    return float(((np.asarray(nimg) + 1) * np.sqrt(((h - href) ** 2).sum(1))).sum())


def needs_rebuild(d2, cellmove, skin):
    """the rebuild rule: a pair changes its distance by at most two atom displacements plus |n . dh|"""
    return bool((2.0 * np.sqrt(np.asarray(d2)) + np.asarray(cellmove)).max(initial=0.0) > skin)


class Twin:
    """the per-configuration state of mtp_relax_cell_step and the step itself.  cfg_first [ncfg + 1], cells [ncfg, 3, 3] (h0).
    x, xt, vt [n, 3] are the caller's and updated in place (x = origin + xt . D); f [n, 3], W [ncfg, 6], inv_m [n] per row."""

    def __init__(self, cfg_first, cells, dt, cell_mass, pressure=0.0, stol=1e-4, cell_mask=(1, 1, 1, 1, 1, 1), isotropic=False,
                 cell_factor=None, origins=None, frozen=None, rghost=7.0, **params):
        self.p = dict(DEFAULTS, **params)
        self.first = np.asarray(cfg_first, dtype=np.int64)
        ncfg = self.ncfg = len(self.first) - 1
        self.h0 = np.array(cells, dtype=np.float64).reshape(ncfg, 3, 3)
        self.pressure, self.stol, self.isotropic, self.cell_mass = float(pressure), float(stol), bool(isotropic), float(cell_mass)
        self.mask = sym(np.asarray(cell_mask, dtype=np.float64)) != 0.0
        self.L = np.diff(self.first).astype(np.float64) if cell_factor is None else np.full(ncfg, float(cell_factor))
        self.origins = np.zeros((ncfg, 3)) if origins is None else np.array(origins, dtype=np.float64)
        self.rghost = rghost
        self.D = np.tile(np.eye(3), (ncfg, 1, 1))
        self.vq = np.zeros((ncfg, 3, 3))
        self.h = self.h0.copy()
        self.G = np.zeros((ncfg, 3, 3))
        self.T = np.tile(np.eye(3), (ncfg, 1, 1))
        self.Dbinv = np.tile(np.eye(3), (ncfg, 1, 1))
        self.href = self.h0.copy()
        self.nimg = np.array([images(c, rghost) for c in self.h0]).reshape(ncfg, 3)
        self.cellmove = np.zeros(ncfg)
        self.dt = np.full(ncfg, float(dt))
        self.alpha = np.full(ncfg, float(self.p["alpha_start"]))
        self.npos = np.zeros(ncfg, dtype=np.int32)
        self.frozen = np.zeros(ncfg, dtype=np.int32) if frozen is None else np.array(frozen, dtype=np.int32)
        self.done_step = np.full(ncfg, -1, dtype=np.int32)
        self.fmax, self.smax = np.zeros(ncfg), np.zeros(ncfg)
        self.count = 0
        self.uphill = self.capped = 0
        self.margin_p = self.margin_tol = self.margin_stol = self.margin_cap = np.inf

    def rebase(self, k):
        """what a rebuild does to configuration k: the reference cell, its image counts and D^-1 of the build"""
        self.href[k] = self.h[k]
        self.nimg[k] = images(self.h[k], self.rghost)
        self.Dbinv[k] = inv3(self.D[k], det3(self.D[k]))
        self.cellmove[k] = 0.0

    def step(self, step, x, xt, vt, f, W, inv_m, last=False):
        p = self.p
        for k in range(self.ncfg):
            a0, a1 = int(self.first[k]), int(self.first[k + 1])
            if a1 == a0 or self.frozen[k]:
                continue
            D, vq, L = self.D[k].copy(), self.vq[k].copy(), self.L[k]
            fk, vk = f[a0:a1], vt[a0:a1]
            with np.errstate(all="ignore"):
                h = self.h0[k] @ D
                V, detD = det3(h), det3(D)
                Wp = np.where(self.mask, sym(W[k]) - self.pressure * V * np.eye(3), 0.0)
                if self.isotropic:
                    Wp = np.eye(3) * ((Wp[0, 0] + Wp[1, 1] + Wp[2, 2]) / 3.0)
                G = inv3(D, detD).T @ Wp / L
                ft = fk @ D.T
                fmax2 = float(np.fmax.reduce((fk * fk).sum(1), initial=0.0))
                P = float((ft * vk).sum())
                vv = float((vk * vk).sum())
                ff = float((ft * ft).sum())
                for q in range(9):                                  # the cell rows, after the atom total
                    P += G.flat[q] * vq.flat[q]
                    vv += vq.flat[q] * vq.flat[q]
                    ff += G.flat[q] * G.flat[q]
                smax = float(np.fmax.reduce(np.abs(Wp).ravel(), initial=0.0)) / V
            self.fmax[k], self.smax[k], self.G[k], self.h[k] = np.sqrt(fmax2), smax, G, h
            if not (np.isfinite(ff) and np.isfinite(W[k]).all() and np.isfinite(V) and np.isfinite(detD) and detD > 0.0):
                self.frozen[k], self.done_step[k] = FAILED, step
                self.count += 1
                continue
            tol2 = p["ftol"] * p["ftol"]
            if tol2 > 0.0:
                self.margin_tol = min(self.margin_tol, abs(fmax2 - tol2) / tol2)
            if self.stol > 0.0:
                self.margin_stol = min(self.margin_stol, abs(smax - self.stol) / self.stol)
            if fmax2 <= tol2 and smax <= self.stol:
                self.frozen[k], self.done_step[k] = CONVERGED, step
                self.count += 1
                vt[a0:a1] = 0.0
                self.vq[k] = 0.0
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
            vm, vqm = a * vk + b * ft, a * vq + b * G
            vmax = max(float(np.abs(vm).max()), float(np.abs(vqm).max()))
            dtv = self.dt[k]
            self.margin_cap = min(self.margin_cap, abs(dtv * vmax - p["dmax"]) / p["dmax"])
            if dtv * vmax > p["dmax"]:
                dtv = p["dmax"] / vmax
                self.capped += 1
            Dn = D + dtv * vqm / L
            self.vq[k] = vqm + ((dtv * FTM2V) / self.cell_mass) * G
            xt[a0:a1] += dtv * vm
            vt[a0:a1] = vm + ((dtv * FTM2V) * inv_m[a0:a1])[:, None] * ft
            x[a0:a1] = self.origins[k] + xt[a0:a1] @ Dn
            self.D[k] = Dn
            self.h[k] = self.h0[k] @ Dn
            self.T[k] = self.Dbinv[k] @ Dn
            self.cellmove[k] = cell_move(self.h[k], self.href[k], self.nimg[k])

    def margins(self):
        return dict(P=self.margin_p, ftol=self.margin_tol, stol=self.margin_stol, cap=self.margin_cap)

    def assert_margins(self):
        """rounding is 1e-12: with every margin above 1e-6 no decision of the run can flip between twin and device"""
        m = self.margins()
        assert min(m.values()) >= MARGIN, "the test's inputs are wrong: a decision is a tie (%s)" % m


# ---- the analytic model: E = k/2 sum |x_i - s0_i . h|^2 + K2/4 |h h^T - G_eq|_F^2 ------------------------------------------

MODEL_SIZES = [0, 1, 63, 64, 65, 256, 257]
MODEL_K = (2.0, 5.0, 9.0, 2.0, 5.0, 9.0, 2.0)
MODEL_MASSES = np.array([183.84, 186.207])


class Model:
    """a batch of such configurations: sizes [ncfg], stiffness k per configuration, K2 = k2 (n / 2)^2 so that the cell
    coordinate L D (L = n) is about as stiff as an atom"""

    def __init__(self, sizes=MODEL_SIZES, k_cfg=MODEL_K, k2=0.05, seed=21, a0=4.0, strain=0.03, noise=0.05):
        sizes = np.asarray(sizes, dtype=np.int64)
        self.cf = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.ncfg, self.n = len(sizes), int(self.cf[-1])
        rng = np.random.default_rng(seed)
        self.types = rng.integers(1, 3, self.n).astype(np.int32)
        self.s0 = rng.random((self.n, 3))
        self.h0 = a0 * np.eye(3) + rng.normal(0.0, 0.3, (self.ncfg, 3, 3))
        eps = rng.normal(0.0, strain, (self.ncfg, 3, 3))
        heq = np.einsum("kab,kbc->kac", self.h0, np.eye(3) + 0.5 * (eps + eps.transpose(0, 2, 1)))
        self.geq = np.einsum("kab,kcb->kac", heq, heq)
        self.k = np.asarray(k_cfg, dtype=np.float64)[: self.ncfg]
        self.k2 = k2 * (np.maximum(sizes, 1) / 2.0) ** 2
        self.cfg = np.repeat(np.arange(self.ncfg), sizes)
        self.x0 = np.einsum("ia,iab->ib", self.s0, self.h0[self.cfg]) + rng.normal(0.0, noise, (self.n, 3))
        self.inv_m = (1.0 / MODEL_MASSES)[self.types - 1]

    def take(self, k):
        """configuration k as a batch of its own"""
        a0, a1 = int(self.cf[k]), int(self.cf[k + 1])
        m = object.__new__(Model)
        m.cf, m.ncfg, m.n = np.array([0, a1 - a0], dtype=np.int32), 1, a1 - a0
        m.types, m.s0, m.x0, m.inv_m = self.types[a0:a1], self.s0[a0:a1], self.x0[a0:a1], self.inv_m[a0:a1]
        m.h0, m.geq, m.k, m.k2 = self.h0[k: k + 1], self.geq[k: k + 1], self.k[k: k + 1], self.k2[k: k + 1]
        m.cfg = np.zeros(a1 - a0, dtype=np.int64)
        return m

    def one(self, k, x, h):
        """E, f [n_k, 3], W [6] of configuration k at positions x [n_k, 3] (without origin) and cell h"""
        a0, a1 = int(self.cf[k]), int(self.cf[k + 1])
        d = x - self.s0[a0:a1] @ h
        m = h @ h.T - self.geq[k]
        e = 0.5 * self.k[k] * float((d * d).sum()) + 0.25 * self.k2[k] * float((m * m).sum())
        w = -self.k[k] * (d.T @ d) - self.k2[k] * (h.T @ m @ h)
        return e, -self.k[k] * d, voigt(w)

    def all(self, x, h, origins=None):
        """energies [ncfg], f [n, 3], W [ncfg, 6] of the batch at x [n, 3] (slot coordinates if `origins`) and cells h"""
        e, f, w = np.zeros(self.ncfg), np.zeros((self.n, 3)), np.zeros((self.ncfg, 6))
        for k in range(self.ncfg):
            a0, a1 = int(self.cf[k]), int(self.cf[k + 1])
            xk = x[a0:a1] if origins is None else x[a0:a1] - origins[k]
            e[k], f[a0:a1], w[k] = self.one(k, xk, h[k])
        return e, f, w


def run_model(model, steps, dt=1e-3, frozen=None, poison=None, keep=(), origins=None, last_at=None, **kw):
    """the twin on the model for steps 0 .. steps - 1.  poison = (step, fn(f, W, twin)) edits the inputs of that step.  Returns
    the twin, x, xt, vt and {step: copies of the state} for `keep`."""
    twin = Twin(model.cf, model.h0, dt, MODEL_MASSES.mean(), frozen=frozen, origins=origins, **kw)
    org = twin.origins[model.cfg]
    xt, vt = model.x0.copy(), np.zeros_like(model.x0)
    x = xt + org
    kept = {}
    for s in range(steps):
        _, f, W = model.all(x, twin.h, twin.origins)
        if poison is not None and poison[0] == s:
            poison[1](f, W, twin)
        twin.step(s, x, xt, vt, f, W, model.inv_m, last=last_at == s)
        if s in keep:
            kept[s] = snapshot(twin, x, xt, vt)
    return twin, x, xt, vt, kept


def snapshot(twin, x, xt, vt):
    return dict(x=x.copy(), xt=xt.copy(), vt=vt.copy(), D=twin.D.copy(), vq=twin.vq.copy(), dt=twin.dt.copy(), alpha=twin.alpha.copy(),
                npos=twin.npos.copy(), frozen=twin.frozen.copy(), done_step=twin.done_step.copy(), fmax=twin.fmax.copy(),
                smax=twin.smax.copy(), gcell=twin.G.copy(), h=twin.h.copy(), T=twin.T.copy(), cellmove=twin.cellmove.copy())


# ---- the host-driven loop -----------------------------------------------------------------------------------------------

def evaluate_with(ctx, list_cutoff):
    """(configs, graded) -> results: one md.evaluate_cells call on the device"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    return lambda configs, graded: evaluate_cells(ctx, configs, list_cutoff=list_cutoff, vflag=1, grades=graded)


def reference_loop(evaluate, configs, steps, dt=1e-3, masses=183.84, cell_mass=None, grade_every=0, select=2.0, brk=10.0, gap=0,
                   max_candidates=10 ** 9, **kw):
    """md.relax_cells_vc driven from the host: energy, forces, virial and grades of every step from ONE `evaluate` call at the
    current cells, capture by _sample.Capture BEFORE the twin, the move by the twin; the launch of step `steps` only decides.
    Positions are kept unwrapped (x = xt . D, no origin).  Stops after the step at which every non-empty configuration is
    frozen.  Returns dict(x, cells: per step lists (what the forces of that step were taken at); energy, fmax, smax, volume
    [steps_done + 1, ncfg]; grades {step: [ncfg]}; capture; snapshots [(x, cell)]; twin; status, done_step, dt; final_x;
    final_cell; virial [ncfg, 6] of the last evaluation; steps_done)."""
    ncfg = len(configs)
    natoms = np.array([len(c[0]) for c in configs])
    first = np.concatenate([[0], np.cumsum(natoms)])
    types = np.concatenate([np.asarray(c[2], dtype=np.int64) for c in configs]) if ncfg else np.zeros(0, dtype=np.int64)
    mass_of_type = np.atleast_1d(np.asarray(masses, dtype=np.float64))
    if cell_mass is None:
        cell_mass = float(mass_of_type.mean())
    if len(mass_of_type) == 1:
        mass_of_type = np.full(max(int(types.max()) if len(types) else 1, 1), mass_of_type[0])
    inv_m = (1.0 / mass_of_type)[types - 1]
    xt = np.concatenate([np.asarray(c[0], dtype=np.float64).reshape(-1, 3) for c in configs]).copy()
    x, vt = xt.copy(), np.zeros_like(xt)
    cap = _sample.Capture(natoms, select, brk, gap, max_candidates)
    twin = Twin(first, np.array([c[1] for c in configs]), dt, cell_mass, **kw)
    split = lambda a: [a[first[k]:first[k + 1]].copy() for k in range(ncfg)]
    out = dict(x=[], cells=[], energy=[], fmax=[], smax=[], volume=[], grades={}, capture=cap, twin=twin, snapshots=[])
    W = np.zeros((ncfg, 6))
    for s in range(steps + 1):
        graded = bool(grade_every) and s % grade_every == 0
        res = evaluate([(x[first[k]:first[k + 1]], twin.h[k], c[2]) for k, c in enumerate(configs)], graded)
        f = np.concatenate([r["f"] for r in res]).copy()
        W = np.array([r["virial"] for r in res]).reshape(ncfg, 6)
        out["x"].append(split(x))
        out["cells"].append(twin.h.copy())
        out["energy"].append([r["energy"] for r in res])
        out["volume"].append([det3(h) for h in twin.h])
        if graded:
            g = np.array([r["cfg_grade"] if "cfg_grade" in r else r["max_grade"] for r in res])
            out["grades"][s] = g
            cap.frozen = twin.frozen != 0
            for k in cap.step(s, g):
                out["snapshots"].append((x[first[k]:first[k + 1]].copy(), twin.h[k].copy()))
            twin.frozen[cap.frozen & (twin.frozen == 0)] = CAPTURED
        twin.step(s, x, xt, vt, f, W, inv_m, last=s == steps)
        out["fmax"].append(twin.fmax.copy())
        out["smax"].append(twin.smax.copy())
        if ((twin.frozen != 0) | (natoms == 0)).all():
            break
    out.update(energy=np.array(out["energy"]), fmax=np.array(out["fmax"]), smax=np.array(out["smax"]), volume=np.array(out["volume"]),
               status=twin.frozen.copy(), done_step=twin.done_step.copy(), dt=twin.dt.copy(), final_x=split(x),
               final_cell=twin.h.copy(), virial=W, steps_done=s)
    return out
