"""Host-side stand-ins for the LAMMPS core pieces either side of the pair style
(Neighbor, Comm ghosts) so the hot path can be exercised
without LAMMPS: periodic ghost images, a *full* neighbour list (the reference requests
REQ_FULL, /root/reference/LAMMPS/ML-MTP/pair_mtp.cpp:318) in CSR form, and the
reverse-communication fold of ghost forces onto their owners (newton_pair on,
pair_mtp.cpp:252-254, 315).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class System:
    x: np.ndarray          # [nall, 3] owned atoms first, then ghosts
    types: np.ndarray      # [nall] int32, 1-based (LAMMPS)
    nlocal: int
    owner: np.ndarray      # [nall] index of the owned atom each entry images (identity for owned)
    box: np.ndarray        # [3]
    ilist: np.ndarray      # [nlocal] int32
    first: np.ndarray      # [nlocal+1] int32 CSR offsets
    neigh: np.ndarray      # [first[-1]] int32 neighbour indices into x
    cutoff: float

    @property
    def nall(self):
        return self.x.shape[0]

    def fold_forces(self, f):
        """Reverse communication: add ghost forces to their owners; returns [nlocal,3]."""
        out = np.zeros((self.nlocal, 3))
        np.add.at(out, self.owner, f)
        return out


def make_ghosts(pos, box, rghost, lo=None):
    """Periodic images within `rghost` of the box [lo, lo+box) (orthogonal cell)."""
    pos = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    lo = np.zeros(3) if lo is None else np.asarray(lo, dtype=np.float64)
    n = pos.shape[0]
    nimg = np.ceil(rghost / box).astype(int)
    xs = [pos]
    owners = [np.arange(n)]
    for sx in range(-nimg[0], nimg[0] + 1):
        for sy in range(-nimg[1], nimg[1] + 1):
            for sz in range(-nimg[2], nimg[2] + 1):
                if sx == sy == sz == 0:
                    continue
                sh = np.array([sx, sy, sz]) * box
                p = pos + sh
                m = np.all((p >= lo - rghost) & (p < lo + box + rghost), axis=1)
                if m.any():
                    xs.append(p[m])
                    owners.append(np.nonzero(m)[0])
    return np.concatenate(xs), np.concatenate(owners)


def cell_margins(cell, rghost):
    """(cell^-1, margins m_a = rghost / d_a, volume) of a right-handed cell whose rows are the lattice vectors;
    d_a = V / |cell_b x cell_c| is the spacing of the lattice planes normal to direction a.  Same arithmetic, in
    the same order, as the library's mtp_ghosts_build_cell."""
    h = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    cross = np.array([np.cross(h[1], h[2]), np.cross(h[2], h[0]), np.cross(h[0], h[1])])
    det = h[0, 0] * cross[0, 0] + h[0, 1] * cross[0, 1] + h[0, 2] * cross[0, 2]
    if not (np.isfinite(h).all() and det > 0.0):
        raise ValueError("cell must be finite, right-handed and non-degenerate (det > 0)")
    hinv = (cross / det).T                                   # column k of cell^-1 = (h_{k+1} x h_{k+2}) / det
    m = rghost * np.sqrt(cross[:, 0] * cross[:, 0] + cross[:, 1] * cross[:, 1] + cross[:, 2] * cross[:, 2]) / det
    return hinv, m, float(det)


def make_ghosts_cell(pos, cell, rghost):
    """Periodic images for any cell (triclinic, smaller than rghost): the numpy twin of mtp_ghosts_build_cell.
    With fractional coordinates s = x . cell^-1 the owned atoms are wrapped to s in [0, 1)^3 (and returned as
    s . cell); the image of atom i under the integer shift n != 0 is a ghost iff -m_a <= s_a + n_a < 1 + m_a in
    all three directions.  Returns (x [nall, 3], owner [nall], shifts [nall, 3] integer), owned atoms first, ghosts
    in atom order, then lexicographic shift order."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    h = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    hinv, m, _ = cell_margins(h, rghost)
    n = pos.shape[0]
    s = (pos[:, 0:1] * hinv[0] + pos[:, 1:2] * hinv[1]) + pos[:, 2:3] * hinv[2]
    s = s - np.floor(s)
    s[~(s < 1.0)] = 0.0                                      # floor() rounding at the upper edge
    lo = np.ceil(-m - s).astype(np.int64)                    # allowed shifts: lo <= n_a <= hi, lo <= 0 <= hi
    hi = np.ceil(1.0 + m - s).astype(np.int64) - 1
    wrapped = (s[:, 0:1] * h[0] + s[:, 1:2] * h[1]) + s[:, 2:3] * h[2]
    owners, shifts = [np.arange(n)], [np.zeros((n, 3), dtype=np.int64)]
    if n:
        for sx in range(int(lo[:, 0].min()), int(hi[:, 0].max()) + 1):
            for sy in range(int(lo[:, 1].min()), int(hi[:, 1].max()) + 1):
                for sz in range(int(lo[:, 2].min()), int(hi[:, 2].max()) + 1):
                    if sx == sy == sz == 0:
                        continue
                    sh = np.array([sx, sy, sz])
                    idx = np.nonzero(np.all((lo <= sh) & (sh <= hi), axis=1))[0]
                    if len(idx):
                        owners.append(idx)
                        shifts.append(np.tile(sh, (len(idx), 1)))
    owner = np.concatenate(owners)
    shift = np.concatenate(shifts)
    order = np.concatenate([np.arange(n), n + np.argsort(owner[n:], kind="stable")])   # atom order, then shift order
    owner, shift = owner[order], shift[order]
    sf = shift.astype(np.float64)
    x = wrapped[owner] + ((sf[:, 0:1] * h[0] + sf[:, 1:2] * h[1]) + sf[:, 2:3] * h[2])
    return x, owner, shift


def make_ghosts_batch(configs, origins, rghost):
    """Many cells in one system: the numpy twin of mtp_ghosts_build_batch.  configs: sequence of (pos, cell); origins
    [ncfg, 3] (capi.batch_layout).  make_ghosts_cell per configuration, translated by its origin and re-ordered to the
    device's order: all owned atoms first (configuration after configuration), then the ghosts in atom order, then
    lexicographic shift order.  The origin is added to the wrapped owned positions and the ghosts are owner + shift,
    rounded in that order, as on the device.  Returns (x [nall, 3], owner [nall] rows of x, shift [nall, 3] integer,
    cfg [nall] the configuration of every row, cfg_first [ncfg + 1])."""
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    counts = [len(np.asarray(p).reshape(-1, 3)) for p, _ in configs]
    cfg_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    own_x, gh_x, gh_owner, gh_shift, gh_cfg = [], [], [], [], []
    for k, (pos, cell) in enumerate(configs):
        n = counts[k]
        h = np.asarray(cell, dtype=np.float64).reshape(3, 3)
        x, owner, shift = make_ghosts_cell(np.asarray(pos, dtype=np.float64).reshape(-1, 3), h, rghost)
        xo = x[:n] + origins[k]
        sf = shift[n:].astype(np.float64)
        own_x.append(xo)
        gh_x.append(xo[owner[n:]] + ((sf[:, 0:1] * h[0] + sf[:, 1:2] * h[1]) + sf[:, 2:3] * h[2]))
        gh_owner.append(owner[n:] + cfg_first[k])
        gh_shift.append(shift[n:])
        gh_cfg.append(np.full(len(owner) - n, k, dtype=np.int64))
    ntot = int(cfg_first[-1])
    x = np.concatenate(own_x + gh_x).reshape(-1, 3) if configs else np.zeros((0, 3))
    owner = np.concatenate([np.arange(ntot)] + gh_owner).astype(np.int64)
    shift = np.concatenate([np.zeros((ntot, 3), dtype=np.int64)] + gh_shift).reshape(-1, 3)
    cfg = np.concatenate([np.repeat(np.arange(len(configs)), counts)] + gh_cfg).astype(np.int64)
    return x, owner, shift, cfg, cfg_first


def full_neighbor_list(x, nlocal, cutoff, chunk=65536):
    """CSR full list over the first nlocal atoms: every j != i with |x_j - x_i| <= cutoff.  Rows are queried in
    chunks, so the Python lists of a 500k-atom system never exist all at once."""
    from scipy.spatial import cKDTree

    tree = cKDTree(x)
    counts = np.zeros(nlocal, dtype=np.int64)
    parts = []
    for c0 in range(0, nlocal, chunk):
        c1 = min(nlocal, c0 + chunk)
        lists = tree.query_ball_point(x[c0:c1], cutoff, workers=-1, return_sorted=True)
        lens = np.fromiter((len(l) for l in lists), dtype=np.int64, count=c1 - c0)
        flat = np.fromiter((j for l in lists for j in l), dtype=np.int32, count=int(lens.sum()))
        rows = np.repeat(np.arange(c0, c1, dtype=np.int64), lens)
        keep = flat != rows                                   # the atom itself
        parts.append(flat[keep])
        counts[c0:c1] = lens - 1
    first = np.zeros(nlocal + 1, dtype=np.int64)
    np.cumsum(counts, out=first[1:])
    neigh = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    assert first[-1] < 2 ** 31 and len(neigh) == first[-1]
    return first.astype(np.int32), neigh


def periodic_system(pos, box, types=None, list_cutoff=7.0):
    """Owned atoms + ghost images + full neighbour list with cutoff `list_cutoff`
    (LAMMPS builds the list with cutoff + skin; 5 A + 2 A metal-units skin = 7 A in the
    BASELINE configs)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    if types is None:
        types = np.ones(n, dtype=np.int32)
    x, owner = make_ghosts(pos, box, list_cutoff)
    first, neigh = full_neighbor_list(x, n, list_cutoff)
    return System(x=x, types=np.asarray(types, dtype=np.int32)[owner], nlocal=n, owner=owner,
                  box=np.asarray(box, dtype=np.float64), ilist=np.arange(n, dtype=np.int32),
                  first=first, neigh=neigh, cutoff=float(list_cutoff))


def periodic_system_cell(pos, cell, types=None, list_cutoff=7.0):
    """periodic_system for any cell (make_ghosts_cell): `box` of the result holds the cell's diagonal only; the
    owned rows of `x` are the positions wrapped into the cell."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    if types is None:
        types = np.ones(n, dtype=np.int32)
    x, owner, _ = make_ghosts_cell(pos, cell, list_cutoff)
    first, neigh = full_neighbor_list(x, n, list_cutoff)
    return System(x=x, types=np.asarray(types, dtype=np.int32)[owner], nlocal=n, owner=owner,
                  box=np.diag(np.asarray(cell, dtype=np.float64).reshape(3, 3)).copy(), ilist=np.arange(n, dtype=np.int32),
                  first=first, neigh=neigh, cutoff=float(list_cutoff))


def maxvol_select_numpy(V, S, W, threshold, max_swaps):
    """numpy twin of the library's mtp_maxvol_select (include/mtp_mi355x.h, "MaxVol selection"): the columns of S are the
    selected candidate vectors, W = S^-1, G = V W^T.  While some |G[i, j]| exceeds `threshold`, the largest one -- ties to
    the smaller linear index i * C + j, which is what np.argmax over the flattened matrix returns -- is swapped in:
    S[:, j] <- V[i] and, with p = G[i, j] and u = (G[i, :] - e_j) / p, every row r of W^T and of G becomes r - r[j] u.
    At most max_swaps swaps.  Returns (S', W', swaps = [(i, j, p)], G): G is the rank-1-updated matrix, not a fresh
    V W'^T -- their difference is the drift the tests bound."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    S = np.array(S, dtype=np.float64)
    Wt = np.array(W, dtype=np.float64).T.copy()
    C = S.shape[0]
    G = V[:, :C] @ Wt
    swaps = []
    while len(swaps) < max_swaps and G.size:
        k = int(np.argmax(np.abs(G)))
        i, j = divmod(k, C)
        p = float(G[i, j])
        if not abs(p) > threshold:
            break
        u = G[i].copy()
        u[j] -= 1.0
        u /= p
        Wt -= np.outer(Wt[:, j], u)
        G -= np.outer(G[:, j], u)
        S[:, j] = V[i, :C]
        swaps.append((i, j, p))
    return S, Wt.T.copy(), swaps, G


def design_twin(tables, system):
    """numpy twin of the design-row kernel (csrc/mtp_design.hip; include/mtp_mi355x.h, "linear refit"): forward mode from
    the parsed tables (capi.Potential.tables()), direction by direction.  For every centre atom the basics and their
    derivatives with respect to each in-cutoff neighbour vector (pair_mtp.cpp:163-191) are pushed through the times rows in
    FILE order, dM[a3] += mult (dM[a0] M[a1] + M[a0] dM[a1]) with M the moments after ALL rows -- the transpose of the
    reference's reverse sweep (:221-233), which multiplies by the final moments even where a row read a partial one;
    G = dM[alpha_moment_mapping] goes to the owner row of the
    neighbour with a minus sign and to the centre's row with a plus sign, and into the virial with the sign and
    symmetrisation of pair_mtp.cpp:257-276.  A scalar whose moment a later scalar is mapped to as well gets zero force and
    virial columns (the reference seeds the adjoint by assignment, :217-218).  `system`: driver.System (owner folding).
    Returns dict(basis [nlocal, Sp + S], energy [Sp + S], force [3 nlocal, Sp + S], virial [6, Sp + S], virial_atom
    [nlocal, 6, Sp + S]); columns [species | moments]."""
    basic = np.asarray(tables["alpha_index_basic"], dtype=np.int64).reshape(-1, 4)
    times = np.asarray(tables["alpha_index_times"], dtype=np.int64).reshape(-1, 4)
    mapping = np.asarray(tables["alpha_moment_mapping"], dtype=np.int64)
    Sp, S, B = len(tables["species_coeffs"]), len(mapping), len(basic)
    Mu = int(basic[:, 0].max()) + 1
    R = len(tables["radial_coeffs"]) // (Sp * Sp * Mu)
    radial = np.asarray(tables["radial_coeffs"], dtype=np.float64).reshape(Sp, Sp, Mu, R)
    A = int(max(B, times[:, [0, 1, 3]].max() + 1 if len(times) else 0, mapping.max() + 1 if S else 0))
    scaling, rmin, rmax = float(tables["scaling"]), float(tables["min_cutoff"]), float(tables["max_cutoff"])
    last = {int(m): s for s, m in enumerate(mapping)}
    fcol = np.array([last[int(m)] == s for s, m in enumerate(mapping)], dtype=bool)
    n = system.nlocal
    ncol = Sp + S
    basis = np.zeros((n, ncol))
    force = np.zeros((3 * n, ncol))
    vatom = np.zeros((n, 6, ncol))
    mu_k, ea, eb, ec = basic[:, 0], basic[:, 1], basic[:, 2], basic[:, 3]
    nu_k = ea + eb + ec
    P = int(nu_k.max()) + 1
    for ii, i in enumerate(system.ilist):
        it = int(system.types[i]) - 1
        js = system.neigh[system.first[ii]:system.first[ii + 1]] & 0x1FFFFFFF
        u = system.x[js] - system.x[i]
        r2 = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]
        keep = ~(r2 > rmax * rmax)
        js, u = js[keep], u[keep]
        K = len(js)
        basis[ii, it] = 1.0
        M = np.zeros(A)
        dM = np.zeros((A, K, 3))
        if K:
            r = np.sqrt(r2[keep])
            inv = 1.0 / r
            jt = system.types[js].astype(np.int64) - 1
            d, ksi, mult = r - rmax, (2.0 * r - (rmin + rmax)) / (rmax - rmin), 2.0 / (rmax - rmin)
            q = np.zeros((R, K))
            e = np.zeros((R, K))
            q[0], e[0] = scaling * (d * d), scaling * 2.0 * d
            if R > 1:
                q[1], e[1] = scaling * (ksi * d * d), scaling * (mult * d * d + 2.0 * ksi * d)
            for ri in range(2, R):
                q[ri] = 2.0 * ksi * q[ri - 1] - q[ri - 2]
                e[ri] = 2.0 * (mult * q[ri - 1] + ksi * e[ri - 1]) - e[ri - 2]
            c = radial[it, jt]                                   # [K, Mu, R]
            val_mu = np.einsum("kmr,rk->mk", c, q)
            der_mu = np.einsum("kmr,rk->mk", c, e)
            rinv = inv[None, :] ** np.arange(P)[:, None]          # [P, K]
            pw = u.T[:, None, :] ** np.arange(P)[None, :, None]   # [3, P, K]
            val = val_mu[mu_k] * rinv[nu_k]                       # [B, K]
            der = der_mu[mu_k] * rinv[nu_k] - nu_k[:, None] * val * inv
            pa, pb, pc = pw[0][ea], pw[1][eb], pw[2][ec]
            M[:B] = (val * (pa * pb * pc)).sum(1)
            jac = ((pa * pb * pc) * der * inv)[:, :, None] * u[None, :, :]
            jac[:, :, 0] += val * ea[:, None] * pw[0][np.maximum(ea - 1, 0)] * pb * pc
            jac[:, :, 1] += val * eb[:, None] * pa * pw[1][np.maximum(eb - 1, 0)] * pc
            jac[:, :, 2] += val * ec[:, None] * pa * pb * pw[2][np.maximum(ec - 1, 0)]
            dM[:B] = jac
        for a0, a1, mlt, a3 in times:
            M[a3] += mlt * M[a0] * M[a1]
        for a0, a1, mlt, a3 in times:                            # (with the FINAL moments, as the reference's reverse sweep)
            dM[a3] += mlt * (dM[a0] * M[a1] + M[a0] * dM[a1])
        basis[ii, Sp:] = M[mapping]
        G = dM[mapping] * fcol[:, None, None]                     # [S, K, 3]
        own = np.asarray(system.owner)[js]
        io = int(np.asarray(system.owner)[i])
        for c3 in range(3):
            np.subtract.at(force[:, Sp:], 3 * own + c3, G[:, :, c3].T)
            force[3 * io + c3, Sp:] += G[:, :, c3].sum(1)
        if K:
            vatom[ii, 0, Sp:] = -(G[:, :, 0] * u[:, 0]).sum(1)
            vatom[ii, 1, Sp:] = -(G[:, :, 1] * u[:, 1]).sum(1)
            vatom[ii, 2, Sp:] = -(G[:, :, 2] * u[:, 2]).sum(1)
            vatom[ii, 3, Sp:] = -0.5 * (G[:, :, 0] * u[:, 1] + G[:, :, 1] * u[:, 0]).sum(1)
            vatom[ii, 4, Sp:] = -0.5 * (G[:, :, 0] * u[:, 2] + G[:, :, 2] * u[:, 0]).sum(1)
            vatom[ii, 5, Sp:] = -0.5 * (G[:, :, 1] * u[:, 2] + G[:, :, 2] * u[:, 1]).sum(1)
    return dict(basis=basis, energy=basis.sum(0), force=force, virial=vatom.sum(0), virial_atom=vatom)


def train_twin(tables, system, theta=None, ebar=None, fbar=None, vbar=None):
    """numpy twin of both modes of the training kernel (csrc/mtp_train.hip; include/mtp_mi355x.h, "training gradient";
    DESIGN.md 5.3.2).  `theta` [C] holds ALL coefficients in candidate-vector order [radial Sp Sp Mu R | species Sp |
    moments S] (None: the file's).  value: eatom, folded forces and vatom with the semantics of PairMTP::compute.  vjp:
    for cotangents ebar [nlocal], fbar [nlocal, 3] (owned atoms) and vbar [nlocal, 6] (None = zero), row i is the derivative
    with respect to theta of  ebar_i eatom_i + sum_n t_n . (fbar_owner(i) - fbar_owner(n) - Vs u_n),  t_n the centre's force
    term on neighbour n and Vs the symmetric matrix of vbar_i with halved off-diagonals: ONE tangent direction du_n per
    centre pushed through the basics and the times rows (FILE order, final moments), and through the reverse sweep with its
    tangent dD.  Tables in which a row reads a moment a later row adds to, or two scalars share a moment, are outside
    these formulas (mtp_potential_train_table refuses them).
    Returns dict(eatom [nlocal], force [nlocal, 3], vatom [nlocal, 6], rows [nlocal, C])."""
    basic = np.asarray(tables["alpha_index_basic"], dtype=np.int64).reshape(-1, 4)
    times = np.asarray(tables["alpha_index_times"], dtype=np.int64).reshape(-1, 4)
    mapping = np.asarray(tables["alpha_moment_mapping"], dtype=np.int64)
    Sp, S, B = len(tables["species_coeffs"]), len(mapping), len(basic)
    Mu = int(basic[:, 0].max()) + 1
    R = len(tables["radial_coeffs"]) // (Sp * Sp * Mu)
    nrad = Sp * Sp * Mu * R
    C = nrad + Sp + S
    if theta is None:
        theta = np.concatenate([tables["radial_coeffs"], tables["species_coeffs"], tables["moment_coeffs"]])
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    assert len(theta) == C, (len(theta), C)
    radial = theta[:nrad].reshape(Sp, Sp, Mu, R)
    species, xi = theta[nrad:nrad + Sp], theta[nrad + Sp:]
    A = int(max(B, times[:, [0, 1, 3]].max() + 1 if len(times) else 0, mapping.max() + 1 if S else 0))
    scaling, rmin, rmax = float(tables["scaling"]), float(tables["min_cutoff"]), float(tables["max_cutoff"])
    n = system.nlocal
    ebar = np.zeros(n) if ebar is None else np.asarray(ebar, dtype=np.float64).reshape(n)
    fbar = np.zeros((n, 3)) if fbar is None else np.asarray(fbar, dtype=np.float64).reshape(n, 3)
    vbar = np.zeros((n, 6)) if vbar is None else np.asarray(vbar, dtype=np.float64).reshape(n, 6)
    eatom, force, vatom, rows = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, C))
    mu_k, ea, eb, ec = basic[:, 0], basic[:, 1], basic[:, 2], basic[:, 3]
    nu_k = ea + eb + ec
    P = int(nu_k.max()) + 1
    owner = np.asarray(system.owner)
    for ii, i in enumerate(system.ilist):
        it = int(system.types[i]) - 1
        js = system.neigh[system.first[ii]:system.first[ii + 1]] & 0x1FFFFFFF
        u = system.x[js] - system.x[i]
        r2 = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]
        keep = ~(r2 > rmax * rmax)
        js, u = js[keep], u[keep]
        K = len(js)
        io = int(owner[i])
        M, dM = np.zeros(A), np.zeros(A)
        if K:
            r = np.sqrt(r2[keep])
            inv = 1.0 / r
            jt = system.types[js].astype(np.int64) - 1
            d, ksi, mult = r - rmax, (2.0 * r - (rmin + rmax)) / (rmax - rmin), 2.0 / (rmax - rmin)
            q = np.zeros((R, K))
            e = np.zeros((R, K))
            q[0], e[0] = scaling * (d * d), scaling * 2.0 * d
            if R > 1:
                q[1], e[1] = scaling * (ksi * d * d), scaling * (mult * d * d + 2.0 * ksi * d)
            for ri in range(2, R):
                q[ri] = 2.0 * ksi * q[ri - 1] - q[ri - 2]
                e[ri] = 2.0 * (mult * q[ri - 1] + ksi * e[ri - 1]) - e[ri - 2]
            c = radial[it, jt]                                   # [K, Mu, R]
            val_mu = np.einsum("kmr,rk->mk", c, q)
            der_mu = np.einsum("kmr,rk->mk", c, e)
            v = vbar[ii]
            Vs = np.array([[v[0], 0.5 * v[3], 0.5 * v[4]], [0.5 * v[3], v[1], 0.5 * v[5]], [0.5 * v[4], 0.5 * v[5], v[2]]])
            du = fbar[io][None, :] - fbar[owner[js]] - u @ Vs     # [K, 3]
            dr = (u * du).sum(1) * inv
            rinv = inv[None, :] ** np.arange(P)[:, None]          # [P, K]
            pw = u.T[:, None, :] ** np.arange(P)[None, :, None]   # [3, P, K]
            pa, pb, pc = pw[0][ea], pw[1][eb], pw[2][ec]
            mono = pa * pb * pc                                   # [B, K]
            grad = np.stack([ea[:, None] * pw[0][np.maximum(ea - 1, 0)] * pb * pc,
                             eb[:, None] * pa * pw[1][np.maximum(eb - 1, 0)] * pc,
                             ec[:, None] * pa * pb * pw[2][np.maximum(ec - 1, 0)]], axis=2)   # [B, K, 3]
            w = rinv[nu_k] * mono
            gw = rinv[nu_k][:, :, None] * grad - (nu_k[:, None] * w * inv)[:, :, None] * (u * inv[:, None])[None, :, :]
            dw = (gw * du[None, :, :]).sum(2)                     # [B, K]
            fv, fd = val_mu[mu_k], der_mu[mu_k]
            M[:B] = (fv * w).sum(1)
            dM[:B] = (fd * dr * w + fv * dw).sum(1)
        for a0, a1, mlt, a3 in times:
            M[a3] += mlt * M[a0] * M[a1]
        for a0, a1, mlt, a3 in times:
            dM[a3] += mlt * (dM[a0] * M[a1] + M[a0] * dM[a1])
        D, dD = np.zeros(A), np.zeros(A)
        for s in range(S):
            D[mapping[s]] = xi[s]
        for a0, a1, mlt, a3 in times[::-1]:
            dD[a1] += mlt * (dD[a3] * M[a0] + D[a3] * dM[a0])
            dD[a0] += mlt * (dD[a3] * M[a1] + D[a3] * dM[a1])
            D[a1] += mlt * D[a3] * M[a0]
            D[a0] += mlt * D[a3] * M[a1]
        eatom[ii] = species[it] + (xi * M[mapping]).sum()
        rows[ii, nrad + it] = ebar[ii]
        rows[ii, nrad + Sp:] = ebar[ii] * M[mapping] + dM[mapping]
        if K:
            # force term of the centre on every neighbour: t_n = sum_k D_k dM_k / du_n
            jac = fd[:, :, None] * w[:, :, None] * (u * inv[:, None])[None, :, :] + fv[:, :, None] * gw
            t = (D[:B, None, None] * jac).sum(0)                 # [K, 3]
            force[io] += t.sum(0)
            np.subtract.at(force, owner[js], t)
            vatom[ii, 0] = -(t[:, 0] * u[:, 0]).sum()
            vatom[ii, 1] = -(t[:, 1] * u[:, 1]).sum()
            vatom[ii, 2] = -(t[:, 2] * u[:, 2]).sum()
            vatom[ii, 3] = -0.5 * (t[:, 0] * u[:, 1] + t[:, 1] * u[:, 0]).sum()
            vatom[ii, 4] = -0.5 * (t[:, 0] * u[:, 2] + t[:, 2] * u[:, 0]).sum()
            vatom[ii, 5] = -0.5 * (t[:, 1] * u[:, 2] + t[:, 2] * u[:, 1]).sum()
            Db, dDb = D[:B, None], dD[:B, None]
            ta = (ebar[ii] * Db + dDb) * w + Db * dw             # [B, K]
            tb = Db * w * dr[None, :]
            for m in range(Mu):
                sel = mu_k == m
                a_mu, b_mu = ta[sel].sum(0), tb[sel].sum(0)       # [K]
                blk = q * a_mu[None, :] + e * b_mu[None, :]       # [R, K]
                for tj in range(Sp):
                    rows[ii, ((it * Sp + tj) * Mu + m) * R:((it * Sp + tj) * Mu + m + 1) * R] += blk[:, jt == tj].sum(1)
    return dict(eatom=eatom, force=force, vatom=vatom, rows=rows)


# ---- numpy twin of the normal-equation kernels (csrc/mtp_normal.hip, csrc/mtp_dd.hpp) ---------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """p + e = a b exactly without an fma (Dekker / Veltkamp splitting): the same e an fma returns, barring overflow"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(ahi, alo, bhi, blo):
    s, e = _two_sum(ahi, bhi)
    t, f = _two_sum(alo, blo)
    s, e = _two_sum(s, e + t)
    return _two_sum(s, e + f)


def normal_twin(rows, scale, target, ncols, state=None, slice_rows=256):
    """numpy twin of mtp_normal_accumulate, operation for operation: b = fl(scale * [rows[:, :ncols] | target]), rows of
    scale 0 skipped (they may hold NaN) and not counted, columns [ncols, ld) never read; slices of `slice_rows` rows summed
    in row order with dd_mac (hi by TwoSum, lo by plain additions), normalised, and added in slice order to the state with
    dd_add.  `state` = (hi [n, n], lo [n, n], count) or None for zeros; returns the new (hi, lo, count)."""
    n = ncols + 1
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(len(scale), rows.size // max(len(scale), 1))
    scale, target = np.asarray(scale, dtype=np.float64), np.asarray(target, dtype=np.float64)
    hi, lo, count = (np.zeros((n, n)), np.zeros((n, n)), 0) if state is None else (state[0].copy(), state[1].copy(), int(state[2]))
    with np.errstate(invalid="ignore"):
        for s0 in range(0, len(scale), slice_rows):
            ahi, alo = np.zeros((n, n)), np.zeros((n, n))
            for i in range(s0, min(s0 + slice_rows, len(scale))):
                if scale[i] == 0.0:
                    continue
                count += 1
                b = np.concatenate([scale[i] * rows[i, :ncols], [scale[i] * target[i]]])
                p, e = _two_prod(b[:, None], b[None, :])
                ahi, t = _two_sum(ahi, p)
                alo = alo + (t + e)
            ahi, alo = _two_sum(ahi, alo)
            hi, lo = _dd_add(hi, lo, ahi, alo)
    return hi, lo, count
