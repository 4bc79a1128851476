"""The numpy twin of the batched elastic constants (md.elastic_cells; include/mtp_mi355x.h, "batched elastic constants"), shared
by tests/test_elastic_cpu.py and tests/test_elastic_gpu.py: mtp_elastic_step and mtp_elastic_finish rule by rule with the
kernels' own expressions and the kernels' own order of every sum (so that the device can be asked for the same BITS), two
analytic models of a strained solid, and a host-driven loop that takes stress and forces of every explicitly strained copy from
md.evaluate_cells."""
import numpy as np

from _hess import segment_total, thread_sums, threads_of

FAILED, UNSTABLE = 1, 2
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))       # xx yy zz xy xz yz
DVEC = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])


def det3(m):
    """batch_step::det3 of a row-major [9]: cofactors along the first row, as written"""
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])


def strain_matrix(w, s):
    """D = I + s E_w, row-major [9]: a 1 on the diagonal, or a half on both off-diagonal entries"""
    D = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    a, b = PAIRS[w]
    if a == b:
        D[4 * a] = 1.0 + s
    else:
        D[3 * a + b] = 0.5 * s
        D[3 * b + a] = 0.5 * s
    return D


def strain_of(k, h):
    """(w, s, D [3, 3]) of strain k = 0 ... 11"""
    w, s = k // 2, (-h if k & 1 else h)
    return w, s, strain_matrix(w, s).reshape(3, 3)


def correction(s):
    """K [6, 6] of Wallace's relation with the kernel's expression, term by term"""
    full = np.array([[s[0], s[3], s[4]], [s[3], s[1], s[5]], [s[4], s[5], s[2]]])
    dl = lambda a, b: 1.0 if a == b else 0.0
    K = np.zeros((6, 6))
    for v, (i, j) in enumerate(PAIRS):
        for w, (k, l) in enumerate(PAIRS):
            K[v, w] = 0.5 * ((((dl(i, k) * full[j, l] + dl(j, k) * full[i, l]) + dl(i, l) * full[j, k]) + dl(j, l) * full[i, k])
                             - 2.0 * dl(k, l) * full[i, j])
    return K


class Twin:
    """the arrays of a pass and its launches.  cfg_first [ncfg + 1] (rows), origins [ncfg, 3], h0 [ncfg, 9], h; x [n, 3] is the
    caller's and is strained and restored in place, x0 its saved copy, xt the positions without the slot origins."""

    def __init__(self, cfg_first, h):
        self.first = np.asarray(cfg_first, dtype=np.int64)
        self.ncfg = ncfg = len(self.first) - 1
        n = int(self.first[-1])
        self.h, self.inv2h = float(h), 1.0 / (2.0 * float(h))
        self.c_first = 18 * self.first
        self.coupling = np.zeros(18 * n)
        self.Bt, self.B, self.C = np.zeros((ncfg, 6, 6)), np.zeros((ncfg, 6, 6)), np.zeros((ncfg, 6, 6))
        self.T = np.zeros((ncfg, 9))
        self.f0, self.stress0 = np.zeros((n, 3)), np.zeros((ncfg, 6))
        self.fmax, self.energy = np.zeros(ncfg), np.zeros(ncfg)
        self.status = np.zeros(ncfg, dtype=np.int32)
        self.diag = np.zeros((ncfg, 2))

    def lam(self, j):
        """Lambda_j [6, 3 n]: a view"""
        a, b = int(self.c_first[j]), int(self.c_first[j + 1])
        return self.coupling[a:b].reshape(6, (b - a) // 6)

    def step(self, k, x, x0, xt, origins, h0, f, virial, eatom=None, energy=None):
        """launch k.  `energy` [ncfg] stands in for the sums of `eatom` [n] where the caller has only those"""
        h = self.h
        for j in range(self.ncfg):
            r0, r1 = int(self.first[j]), int(self.first[j + 1])
            if r1 == r0 or self.status[j]:
                continue
            W, fj = virial[j], f[r0:r1]
            with np.errstate(all="ignore"):
                V0 = det3(h0[j])
                bad = not np.isfinite(W).all() or not np.isfinite(fj).all()
                if k == 0:                                                               # 1.
                    bad = bad or not (V0 > 0.0) or not np.isfinite(V0)
                    self.f0[r0:r1] = fj
                    f2 = ((0.0 + fj[:, 0] * fj[:, 0]) + fj[:, 1] * fj[:, 1]) + fj[:, 2] * fj[:, 2]
                    self.fmax[j] = np.sqrt(np.fmax.reduce(f2, initial=0.0))
                    self.energy[j] = (segment_total(thread_sums(eatom[r0:r1], threads_of(r1 - r0))) if energy is None
                                      else energy[j])
                    self.stress0[j] = -(W / V0)
                elif not bad:                                                            # 2.
                    w, minus = (k - 1) // 2, (k - 1) & 1
                    V = V0 * det3(strain_matrix(w, -h if minus else h))
                    sig, row, fi = -(W / V), self.lam(j)[w], fj.reshape(-1)
                    row[:] = (row - fi) * self.inv2h if minus else fi
                    self.Bt[j, w] = (self.Bt[j, w] - sig) * self.inv2h if minus else sig
            if bad or k == 12:                                                           # 3.
                if bad:
                    self.status[j] = FAILED
                x[r0:r1] = x0[r0:r1]
                self.T[j] = strain_matrix(0, 0.0)
                continue
            D = strain_matrix(k // 2, -h if k & 1 else h)
            a, o = xt[r0:r1], origins[j]
            for b in range(3):
                x[r0:r1, b] = o[b] + ((a[:, 0] * D[b] + a[:, 1] * D[3 + b]) + a[:, 2] * D[6 + b])
            self.T[j] = D

    def finish(self):
        """mtp_elastic_finish: B = Bt^T, C = sym(B - K), the asymmetry before symmetrising and the sum rule over the atoms in order"""
        for j in range(self.ncfg):
            n = int(self.first[j + 1] - self.first[j])
            if n == 0 or self.status[j]:
                continue
            with np.errstate(all="ignore"):
                B = self.Bt[j].T.copy()
                M = B - correction(self.stress0[j])
                self.diag[j, 0] = np.fmax.reduce(np.abs(M - M.T)[np.triu_indices(6, 1)], initial=0.0)
                S, L = np.zeros((6, 3)), self.lam(j)
                for i in range(n):
                    S = S + L[:, 3 * i: 3 * i + 3]
                self.diag[j, 1] = np.fmax.reduce(np.abs(S).reshape(-1), initial=0.0)
                self.B[j], self.C[j] = B, 0.5 * (M + M.T)

    def run(self, x, origins, h0, model, nan_at=None):
        """a whole pass on x (changed in place and restored): model(x) -> (eatom [n], f [n, 3], virial [ncfg, 6]); nan_at =
        (launch, "f" or "w", index...) poisons one number in front of that launch"""
        x0 = x.copy()
        xt = x0 - np.repeat(origins, np.diff(self.first), axis=0)
        for k in range(13):
            e, f, W = model(x)
            if nan_at is not None and nan_at[0] == k:
                f, W = f.copy(), W.copy()
                (f if nan_at[1] == "f" else W)[nan_at[2], nan_at[3]] = np.nan
            self.step(k, x, x0, xt, origins, h0, f, W, eatom=e)
        self.finish()
        return self


# ---- analytic solids -------------------------------------------------------------------------------------------------------

def full3(s):
    return np.array([[s[0], s[3], s[4]], [s[3], s[1], s[5]], [s[4], s[5], s[2]]])


def six(m):
    return np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]])


def random_constants(seed, scale=1.0):
    """a symmetric positive definite C [6, 6] and a stress [6]"""
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(6, 6))
    return scale * (Q @ Q.T + 6.0 * np.eye(6)), 0.3 * scale * rng.normal(size=6)


class LinearSolid:
    """One configuration whose Cauchy stress and forces are LINEAR in the strain (its energy quadratic in it): for x = xt . D,
    D = I + eps with eps read off x itself, sigma = sigma0 + B eps6 with B = C + K(sigma0) (eps6 with engineering shears), the
    virial W = -sigma V0 det D, and f = f0 + Lambda^T eps6 with sum_i Lambda = 0.  Central differences are then exact up to
    rounding."""

    def __init__(self, n, seed, cell):
        rng = np.random.default_rng(seed)
        self.C, self.sigma = random_constants(seed)
        self.B = self.C + correction(self.sigma)
        self.cell, self.V0 = cell, float(np.linalg.det(cell))
        self.frac = rng.random((n, 3))
        self.pos = self.frac @ cell
        L = rng.normal(size=(6, n, 3))
        self.Lam = (L - L.mean(1, keepdims=True)).reshape(6, 3 * n)
        f0 = rng.normal(size=(n, 3))
        self.f0 = f0 - f0.mean(0)
        self.e0 = rng.normal(size=n)

    def __call__(self, x, origin):
        D = np.linalg.lstsq(self.pos, x - origin, rcond=None)[0]                # (n >= 3 atoms that span the space)
        eps = D - np.eye(3)
        e6 = np.array([eps[0, 0], eps[1, 1], eps[2, 2], 2.0 * eps[0, 1], 2.0 * eps[0, 2], 2.0 * eps[1, 2]])
        sig = self.sigma + self.B @ e6
        W = -sig * self.V0 * np.linalg.det(D)
        return self.e0.copy(), self.f0 + (e6 @ self.Lam).reshape(-1, 3), W


def hyperelastic_virial(C, S, V0, D):
    """W [6] of the solid with E = V0 (S : eta + eta : C : eta / 2) in the Lagrangian strain eta = (D D^T - I) / 2 of x -> x D:
    the second Piola-Kirchhoff stress S + C eta pushed forward, sigma = D^T (S + C eta) D / det D (rows of x are vectors, so the
    deformation gradient is D^T), W = -sigma V0 det D.  C [6, 6] with engineering shears, S [6]."""
    eta = 0.5 * (D @ D.T - np.eye(3))
    e6 = np.array([eta[0, 0], eta[1, 1], eta[2, 2], 2.0 * eta[0, 1], 2.0 * eta[0, 2], 2.0 * eta[1, 2]])
    pk = full3(S + C @ e6)
    return -six(D.T @ pk @ D) * V0


# ---- the host-driven loop ------------------------------------------------------------------------------------------------------

def reference_loop(ctx, configs, h, list_cutoff=7.0):
    """md.elastic_cells driven from the host: md.evaluate_cells on the configurations as given and on the 12 explicitly strained
    copies (pos @ D, cell @ D), stress = -W / det(cell @ D), the difference quotients in numpy.  Returns one dict per
    configuration (stress, birch, coupling, f0, energy, wmax, fmax: the largest |W| and |f| component over the 13 calls) and the
    number of evaluate_cells calls."""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    base = evaluate_cells(ctx, configs, list_cutoff=list_cutoff)
    out = [dict(stress=-r["virial"] / r["volume"] if len(c[0]) else np.zeros(6), birch=np.zeros((6, 6)),
                coupling=np.zeros((6, 3 * len(c[0]))), f0=r["f"], energy=r["energy"],
                wmax=float(np.abs(r["virial"]).max()), fmax=float(np.abs(r["f"]).max(initial=0.0))) for c, r in zip(configs, base)]
    for k in range(12):
        w, s, D = strain_of(k, h)
        res = evaluate_cells(ctx, [(np.asarray(c[0]).reshape(-1, 3) @ D, np.asarray(c[1]) @ D, c[2]) for c in configs],
                             list_cutoff=list_cutoff)
        for j, (c, r) in enumerate(zip(configs, res)):
            if not len(c[0]):
                continue
            sig = -r["virial"] / float(np.linalg.det(np.asarray(c[1]) @ D))
            sign = -1.0 if k & 1 else 1.0
            out[j]["birch"][:, w] += sign * sig / (2.0 * h)
            out[j]["coupling"][w] += sign * r["f"].reshape(-1) / (2.0 * h)
            out[j]["wmax"] = max(out[j]["wmax"], float(np.abs(r["virial"]).max()))
            out[j]["fmax"] = max(out[j]["fmax"], float(np.abs(r["f"]).max()))
    return out, 13


# ---- hand-made inputs of mtp_elastic_relax -------------------------------------------------------------------------------------

def spring_network(n, seed, negative=False):
    """(H [3 n, 3 n], Lambda [6, 3 n]) of n atoms: a translation-invariant positive semi-definite Hessian (random springs between
    pairs, every atom tied to the next so that the translations are its only null vectors) and a coupling whose rows sum to zero
    over the atoms.  `negative` flips one spring."""
    rng = np.random.default_rng(seed)
    H = np.zeros((3 * n, 3 * n))
    pairs = [(i, (i + 1) % n) for i in range(n)] + [tuple(rng.choice(n, 2, replace=False)) for _ in range(2 * n)] if n > 1 else []
    for q, (i, j) in enumerate(pairs):
        if i == j:
            continue
        G = rng.normal(size=(3, 3))
        k = G @ G.T + 0.5 * np.eye(3)
        if negative and q == 0:
            k = -40.0 * k
        for a, b, sgn in ((i, i, 1.0), (j, j, 1.0), (i, j, -1.0), (j, i, -1.0)):
            H[3 * a: 3 * a + 3, 3 * b: 3 * b + 3] += sgn * k
    L = rng.normal(size=(6, n, 3))
    return 0.5 * (H + H.T), (L - L.mean(1, keepdims=True)).reshape(6, 3 * n)
