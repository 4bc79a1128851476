"""The numpy twin of the batched nudged elastic band (md.neb_cells; include/mtp_mi355x.h, "batched nudged elastic band"),
shared by tests/test_neb_cpu.py and tests/test_neb_gpu.py: the minimum image, mtp_neb_step rule by rule (capture check,
energies, improved tangent, F_neb with the climbing image, the band's FIRE step), the tie margins of a run, the analytic
double-well surface of the kernel tests (written once for numpy and torch), and a host-driven reference loop that takes forces,
energies and grades from md.evaluate_cells, captures with tests/_sample.py's Capture and moves with the twin."""
import numpy as np

import _relax
import _sample
from _relax import CAPTURED, CONVERGED, FAILED, MARGIN
from _sample import FTM2V

DEFAULTS = dict(_relax.DEFAULTS, spring=5.0, climb_step=-1)


def mic(d, cell, cell_inv):
    """d - rint(d . h^-1) . h, rows of `cell` the lattice vectors"""
    return d - np.rint(d @ cell_inv) @ cell


def _gap(a, b):
    """how far from a tie the comparison of a with b is, relative to the larger of the two"""
    scale = max(abs(a), abs(b))
    return abs(a - b) / scale if scale > 0.0 else 0.0


def tangent_weights(em, e0, ep, margins=None):
    """(w+, w-) of tau = w+ D+ + w- D-: the improved tangent of Henkelman & Jonsson (rule 3); `margins` collects how far from a
    tie each comparison made was"""
    note = (lambda a, b: margins.append(_gap(a, b))) if margins is not None and np.isfinite([em, e0, ep]).all() else (lambda a, b: None)
    note(ep, e0)
    note(e0, em)
    if ep > e0 > em:
        return 1.0, 0.0
    if ep < e0 < em:
        return 0.0, 1.0
    note(ep, em)
    up, dn = abs(ep - e0), abs(em - e0)
    big, small = float(np.fmax(up, dn)), float(np.fmin(up, dn))
    return (big, small) if ep > em else (small, big)


def neb_force(c, f, E, cell, cell_inv, spring, climber=-1, margins=None):
    """rules 3 and 4 for one band: c [M][n, 3] cell coordinates, f [M][n, 3], E [M].  Returns F_neb [M][n, 3] (zeros for the two
    end images) and whether a tangent was zero or not finite."""
    M = len(c)
    out, bad = [np.zeros_like(c[0])], False
    for i in range(1, M - 1):
        dp, dm = mic(c[i + 1] - c[i], cell, cell_inv), mic(c[i] - c[i - 1], cell, cell_inv)
        wp, wm = tangent_weights(E[i - 1], E[i], E[i + 1], margins)
        tau = wp * dp + wm * dm
        with np.errstate(all="ignore"):
            sp, sm, tt, ft = float((dp * dp).sum()), float((dm * dm).sum()), float((tau * tau).sum()), float((f[i] * tau).sum())
            norm = np.sqrt(tt)
            fpar = np.float64(ft) / norm
            g = (-2.0 * fpar if i == climber else spring * (np.sqrt(sp) - np.sqrt(sm)) - fpar) / norm
            out.append(f[i] + g * tau)
        bad = bad or not (norm > 0.0 and np.isfinite(norm))
    out.append(np.zeros_like(c[0]))
    return out, bad


class Twin:
    """the state of mtp_neb_step and the step itself.  band_first [nband + 1] (configurations), cfg_first [ncfg + 1] (rows),
    cells [nband, 3, 3]; x, v, f [n, 3] are the caller's and x, v are updated in place; inv_m [n] per row; `frozen` [ncfg] is
    what mtp_sample_capture shares with the kernel."""

    def __init__(self, band_first, cfg_first, cells, dt, frozen=None, **params):
        self.p = dict(DEFAULTS, **params)
        self.band_first = np.asarray(band_first, dtype=np.int64)
        self.first = np.asarray(cfg_first, dtype=np.int64)
        self.cell = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
        self.cell_inv = np.linalg.inv(self.cell)
        nband, ncfg, n = len(self.band_first) - 1, len(self.first) - 1, int(self.first[-1])
        assert len(self.cell) == nband
        self.dt = np.full(nband, float(dt))
        self.alpha = np.full(nband, float(self.p["alpha_start"]))
        self.npos = np.zeros(nband, dtype=np.int32)
        self.status = np.zeros(nband, dtype=np.int32)
        self.done_step = np.full(nband, -1, dtype=np.int32)
        self.climber = np.full(nband, -1, dtype=np.int32)
        self.fmax = np.zeros(nband)
        self.frozen = np.zeros(ncfg, dtype=np.int32) if frozen is None else np.array(frozen, dtype=np.int32)
        self.energy = np.zeros(ncfg)
        self.fneb = np.zeros((n, 3))
        self.count = 0                      # what the kernel adds to counts[2]
        self.uphill = self.capped = 0       # events over the run
        self.margin_p = self.margin_tol = self.margin_e = self.margin_climb = np.inf

    def step(self, step, x, v, f, origins, inv_m, eatom=None, energy=None, last=False):
        """`energy` [ncfg] stands in for the sums of `eatom` [n] where the caller has only those"""
        p = self.p
        tol2 = p["ftol"] * p["ftol"]
        for b in range(len(self.dt)):
            k0, k1 = int(self.band_first[b]), int(self.band_first[b + 1])
            M = k1 - k0
            if self.status[b]:
                continue
            if self.frozen[k0:k1].any():                                             # 1. the capture check
                new = self.frozen[k0:k1] == 0
                self.frozen[k0:k1][new] = CAPTURED
                self.count += int(new.sum())
                self.status[b], self.done_step[b] = CAPTURED, step
                continue
            rows = [(int(self.first[k]), int(self.first[k + 1])) for k in range(k0, k1)]
            assert len({r1 - r0 for r0, r1 in rows}) == 1
            E = np.array([eatom[r0:r1].sum() for r0, r1 in rows]) if energy is None else np.asarray(energy[k0:k1], dtype=np.float64)
            self.energy[k0:k1] = E                                                   # 2.
            if not np.isfinite(E).all():                                             # (no tangent is made from such an energy)
                self.fmax[b], self.climber[b] = 0.0, -1
                self.frozen[k0:k1], self.status[b], self.done_step[b] = FAILED, FAILED, step
                self.count += M
                continue
            climber = -1
            if p["climb_step"] >= 0 and step >= p["climb_step"]:
                climber = 1 + int(np.argmax(E[1: M - 1]))                            # (the first of equal maxima)
                if M > 3:
                    second = np.sort(E[1: M - 1])[-2]
                    self.margin_climb = min(self.margin_climb, _gap(E[climber], second))
            margins = []
            fn, bad = neb_force([x[r0:r1] - origins[k0 + i] for i, (r0, r1) in enumerate(rows)], [f[r0:r1] for r0, r1 in rows], E,
                                self.cell[b], self.cell_inv[b], p["spring"], climber, margins)   # 3., 4.
            self.margin_e = min([self.margin_e] + margins)
            for (r0, r1), fi in zip(rows, fn):
                self.fneb[r0:r1] = fi
            self.climber[b] = climber
            a0, a1 = rows[1][0], rows[M - 1][0]                                      # 5. FIRE over the interior rows
            fk, vk = self.fneb[a0:a1], v[a0:a1]
            with np.errstate(invalid="ignore", over="ignore"):
                P, vv = float((fk * vk).sum()), float((vk * vk).sum())
                f2 = (fk * fk).sum(1)
                ff, fmax2 = float(f2.sum()), float(np.fmax.reduce(f2, initial=0.0))
            self.fmax[b] = np.sqrt(fmax2)
            if bad or not np.isfinite(ff):
                self.frozen[k0:k1], self.status[b], self.done_step[b] = FAILED, FAILED, step
                self.count += M
                continue
            if tol2 > 0.0:
                self.margin_tol = min(self.margin_tol, abs(fmax2 - tol2) / tol2)
            if fmax2 <= tol2:
                self.frozen[k0:k1], self.status[b], self.done_step[b] = CONVERGED, CONVERGED, step
                self.count += M
                v[a0:a1] = 0.0
                continue
            if last:
                continue
            if vv > 0.0:
                self.margin_p = min(self.margin_p, abs(P) / np.sqrt(vv * ff))
            if P > 0.0:
                a, bb = 1.0 - self.alpha[b], self.alpha[b] * np.sqrt(vv / ff)
                self.npos[b] += 1
                if self.npos[b] > p["n_min"]:
                    self.dt[b] = min(self.dt[b] * p["f_inc"], p["dt_max"])
                    self.alpha[b] *= p["f_alpha"]
            else:
                a = bb = 0.0
                self.npos[b] = 0
                self.alpha[b] = p["alpha_start"]
                if vv > 0.0:
                    self.dt[b] *= p["f_dec"]
                    self.uphill += 1
            vm = a * vk + bb * fk
            vmax = float(np.abs(vm).max())
            dtv = self.dt[b]
            if dtv * vmax > p["dmax"]:
                dtv = p["dmax"] / vmax
                self.capped += 1
            x[a0:a1] += dtv * vm
            v[a0:a1] = vm + ((dtv * FTM2V) * inv_m[a0:a1])[:, None] * fk

    def margins(self):
        return dict(P=self.margin_p, tolerance=self.margin_tol, energy=self.margin_e, climber=self.margin_climb)

    def assert_margins(self):
        """rounding is 1e-12: with every margin above 1e-6 no decision of the run can flip between twin and device"""
        assert min(self.margins().values()) >= MARGIN, "the test's inputs are wrong: a decision is a tie: %r" % (self.margins(),)


# ---- the analytic surface: per atom A (ux^2 - 1)^2 + B (uy - C (1 - ux^2))^2 + D uz^2 with u = x - site, and the coupling
# ---- G (ux_j - ux_j+1)^2 between consecutive atoms of an image, booked on atom j ----------------------------------------------

TRICLINIC = np.array([[11.0, 0.0, 0.0], [2.5, 10.0, 0.0], [-1.5, 2.0, 9.5]])
SURFACE_MASSES = np.array([30.0, 45.0])


def surface(xp, x, site, A, B, C, D, G, link):
    """(eatom [n], f [n, 3]) for rows x [n, 3]; every constant is an array [n]; link[r] = 1 where row r + 1 is the next atom of
    the same image.  `xp` is numpy or torch: elementwise operations and one shift, the same expression for both."""
    ux, uy, uz = x[:, 0] - site[:, 0], x[:, 1] - site[:, 1], x[:, 2] - site[:, 2]
    q = ux * ux - 1.0
    w = uy + C * q
    d = (ux - xp.roll(ux, -1, 0)) * link
    e = A * q * q + B * w * w + D * uz * uz + G * d * d
    fx = -(4.0 * A * q * ux + 4.0 * B * C * w * ux) - 2.0 * G * d + 2.0 * xp.roll(G * d, 1, 0)
    return e, xp.stack([fx, -2.0 * B * w, -2.0 * D * uz], 1)


def saddle_hessian(A, B, C, D, G):
    """the Hessian [3 n, 3 n] (atom-major) of one image of n atoms at its saddle u_j = (0, C, 0), where the cross terms vanish:
    d2/dx2 = -4 A_j plus the chain coupling 2 G (x_j - x_j+1)^2 / 2, d2/dy2 = 2 B, d2/dz2 = 2 D.  Constants are arrays [n]."""
    n = len(A)
    H = np.zeros((3 * n, 3 * n))
    for j in range(n):
        H[3 * j, 3 * j], H[3 * j + 1, 3 * j + 1], H[3 * j + 2, 3 * j + 2] = -4.0 * A[j], 2.0 * B[j], 2.0 * D[j]
    for j in range(n - 1):
        H[3 * j, 3 * j] += 2.0 * G[j]
        H[3 * j + 3, 3 * j + 3] += 2.0 * G[j]
        H[3 * j, 3 * j + 3] -= 2.0 * G[j]
        H[3 * j + 3, 3 * j] -= 2.0 * G[j]
    return H


def surface_bands(shapes, seed=5, cell=TRICLINIC, A=(0.3, 0.7), B=2.0, C=0.6, D=1.5, G=0.05, noise=0.05, end_noise=0.1, hopping=1):
    """Bands of (M images, n atoms) on the surface, every atom in a well of its own around a random site of `cell`.  The first
    `hopping` atoms (None: all) hop: image i starts them at ux = -1 + 2 i / (M - 1); the others stay in their minimum at ux = 1 and
    only follow through the coupling -- one negative curvature at the saddle, as for a defect that hops in a crystal that relaxes
    (atoms that hop independently, each with a barrier of its own, give the climbing image no maximum to climb to).  `noise` is
    added on the interior images and `end_noise` on the hopping atoms of the two ends (a band that is not symmetric: no two
    image energies tie; the others sit in their minima there, so that the ends lie lower than the barrier).  Rows in batch order, slot origins that differ from configuration to configuration.
    Returns a dict of arrays: band_first, cfg_first, cells [nband, 3, 3], origins [ncfg, 3], types [n], x0 (slot coordinates), site
    (slot coordinates), and the constants A, B, C, D, G, link per row."""
    rng = np.random.default_rng(seed)
    band_first, cfg_first, x0, site, link, origins, types, Arow = [0], [0], [], [], [], [], [], []
    for M, n in shapes:
        s = rng.random((n, 3)) @ cell
        a = rng.uniform(A[0], A[1], n)
        ty = rng.integers(1, 3, n).astype(np.int32)
        for i in range(M):
            org = rng.integers(-2, 3, 3) * 4.0
            u = np.zeros((n, 3))
            u[:, 0] = 1.0
            u[:hopping, 0] = -1.0 + 2.0 * i / (M - 1)
            if i in (0, M - 1):
                u[:hopping] += rng.normal(0.0, end_noise, u[:hopping].shape)
            else:
                u += rng.normal(0.0, noise, (n, 3))
            x0.append(org + s + u)
            site.append(org + s)
            link.append(np.concatenate([np.ones(n - 1), [0.0]]))
            origins.append(org)
            types.append(ty)
            Arow.append(a)
            cfg_first.append(cfg_first[-1] + n)
        band_first.append(band_first[-1] + M)
    n = cfg_first[-1]
    const = lambda q: np.full(n, float(q))
    return dict(band_first=np.array(band_first, dtype=np.int32), cfg_first=np.array(cfg_first, dtype=np.int32),
                cells=np.array([cell] * len(shapes), dtype=np.float64), origins=np.array(origins, dtype=np.float64),
                types=np.concatenate(types), x0=np.concatenate(x0), site=np.concatenate(site), A=np.concatenate(Arow), B=const(B),
                C=const(C), D=const(D), G=const(G), link=np.concatenate(link))


SURFACE_KEYS = ("site", "A", "B", "C", "D", "G", "link")
ROW_KEYS = ("types", "x0") + SURFACE_KEYS


def sub_bands(S, which):
    """the bands `which` of `S` as a batch of their own (rows, configurations and bands renumbered; the same bits)"""
    out = dict(band_first=[0], cfg_first=[0], cells=S["cells"][list(which)], origins=[])
    rows = {k: [] for k in ROW_KEYS}
    for b in which:
        k0, k1 = int(S["band_first"][b]), int(S["band_first"][b + 1])
        for k in range(k0, k1):
            r0, r1 = int(S["cfg_first"][k]), int(S["cfg_first"][k + 1])
            for key in ROW_KEYS:
                rows[key].append(S[key][r0:r1])
            out["cfg_first"].append(out["cfg_first"][-1] + r1 - r0)
            out["origins"].append(S["origins"][k])
        out["band_first"].append(out["band_first"][-1] + k1 - k0)
    out.update({k: np.concatenate(v) for k, v in rows.items()})
    out.update(band_first=np.array(out["band_first"], dtype=np.int32), cfg_first=np.array(out["cfg_first"], dtype=np.int32),
               origins=np.array(out["origins"]))
    return out


def shifted_by_lattice_vectors(S, seed=2, share=0.3):
    """`S` with a share of the atoms of every image -- the end images too -- moved by lattice vectors of up to +-2 cells, a
    different one per atom and image (site moves along: the surface sees the same u).  Returns the copy and the shifts [n, 3]."""
    rng = np.random.default_rng(seed)
    T = dict(S)
    shift = np.zeros_like(S["x0"])
    for b in range(len(S["band_first"]) - 1):
        r0, r1 = int(S["cfg_first"][S["band_first"][b]]), int(S["cfg_first"][S["band_first"][b + 1]])
        pick = rng.random(r1 - r0) < share
        shift[r0:r1][pick] = rng.integers(-2, 3, (int(pick.sum()), 3)) @ S["cells"][b]
    T["x0"], T["site"] = S["x0"] + shift, S["site"] + shift
    return T, shift


def run_surface(S, steps, dt=1e-3, frozen=None, nan_at=None, keep=(), last_at=None, nan_energy_at=None, **params):
    """the twin on the surface bands `S` for steps 0 .. steps - 1.  nan_at = (step, row, component) poisons one force component of
    that step, nan_energy_at = (step, row) one per-atom energy; the step last_at is made with `last`.  Returns the twin, x, v and {step: dict of copies} for `keep`."""
    twin = Twin(S["band_first"], S["cfg_first"], S["cells"], dt, frozen=frozen, **params)
    inv_m = (1.0 / SURFACE_MASSES)[S["types"] - 1]
    x, v = S["x0"].copy(), np.zeros_like(S["x0"])
    kept = {}
    for s in range(steps):
        e, f = surface(np, x, *[S[k] for k in SURFACE_KEYS])
        if nan_at is not None and nan_at[0] == s:
            f[nan_at[1], nan_at[2]] = np.nan
        if nan_energy_at is not None and nan_energy_at[0] == s:
            e[nan_energy_at[1]] = np.nan
        twin.step(s, x, v, f, S["origins"], inv_m, eatom=e, last=s == last_at)
        if s in keep:
            kept[s] = dict(x=x.copy(), v=v.copy(), dt=twin.dt.copy(), alpha=twin.alpha.copy(), fmax=twin.fmax.copy(),
                           frozen=twin.frozen.copy(), status=twin.status.copy(), fneb=twin.fneb.copy(), energy=twin.energy.copy(),
                           npos=twin.npos.copy(), climber=twin.climber.copy(), done_step=twin.done_step.copy(), count=twin.count)
    return twin, x, v, kept


# ---- the host-driven loop -----------------------------------------------------------------------------------------------

def flatten(bands):
    """the images of all bands as configurations (pos, cell, types) and the band table"""
    configs, band_first = [], [0]
    for images, cell, types in bands:
        configs += [(np.asarray(p, dtype=np.float64), np.asarray(cell, dtype=np.float64), np.asarray(types)) for p in images]
        band_first.append(len(configs))
    return configs, np.array(band_first, dtype=np.int64)


def reference_loop(ctx, bands, steps, dt=1e-3, masses=183.84, grade_every=0, select=2.0, brk=10.0, gap=0, max_candidates=10 ** 9,
                   list_cutoff=7.0, **params):
    """md.neb_cells driven from the host: forces, energies and grades of every step from md.evaluate_cells (one call a step over
    the images of all bands), capture by _sample.Capture BEFORE the twin, the band arithmetic and the move by the twin on
    positions that are never wrapped; the launch of step `steps` only decides.  Stops after the step at which every band has
    stopped.  Returns dict(energy [steps_done + 1, ncfg]; fmax [steps_done + 1, nband]; grades {step: [ncfg]}; capture; twin;
    status, done_step, dt [nband]; final_x: per configuration; snapshots; steps_done)."""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    configs, band_first = flatten(bands)
    ncfg = len(configs)
    natoms = np.array([len(c[0]) for c in configs])
    first = np.concatenate([[0], np.cumsum(natoms)])
    types = np.concatenate([np.asarray(c[2], dtype=np.int64) for c in configs])
    mass_of_type = np.atleast_1d(np.asarray(masses, dtype=np.float64))
    if len(mass_of_type) == 1:
        mass_of_type = np.full(max(int(types.max()), 1), mass_of_type[0])
    inv_m = (1.0 / mass_of_type)[types - 1]
    x = np.concatenate([c[0].reshape(-1, 3) for c in configs]).copy()
    v = np.zeros_like(x)
    cap = _sample.Capture(natoms, select, brk, gap, max_candidates)
    twin = Twin(band_first, first, [b[1] for b in bands], dt, **params)
    split = lambda a: [a[first[k]:first[k + 1]].copy() for k in range(ncfg)]
    out = dict(energy=[], fmax=[], grades={}, capture=cap, twin=twin, snapshots=[], x=[])
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
        twin.step(s, x, v, f, np.zeros((ncfg, 3)), inv_m, energy=np.array(out["energy"][-1]), last=s == steps)
        out["fmax"].append(twin.fmax.copy())
        if (twin.frozen != 0).all():
            break
    out.update(energy=np.array(out["energy"]), fmax=np.array(out["fmax"]), status=twin.status.copy(), done_step=twin.done_step.copy(),
               dt=twin.dt.copy(), final_x=split(x), steps_done=s)
    return out
