"""Shared by the training-gradient tests (tests/test_train_cpu.py, tests/test_train_gpu.py).  The judge of a gradient row
is the reference algorithm itself: the scalar  sum_i ebar_i eatom_i + sum_j fbar_j . F_j + sum_i vbar_i . vatom_i  (F the
folded force) evaluated by the CPU oracle with ONE coefficient changed in place through its Model pointers, central
differences at h, h/2 and h/4 with h = 1e-3 max(|c|, 0.05), Richardson-extrapolated twice."""
import numpy as np


def sizes(orc):
    m = orc.m
    nrad = m.species_count ** 2 * m.radial_func_count * m.radial_basis_size
    return nrad, m.species_count, m.alpha_scalar_count


def pointer_of(orc, col):
    """(pointer, index) of coefficient `col` in candidate-vector order [radial | species | moments]"""
    nrad, Sp, S = sizes(orc)
    if col < nrad:
        return orc.m.radial_basis_coeffs, col
    if col < nrad + Sp:
        return orc.m.species_coeffs, col - nrad
    return orc.m.linear_coeffs, col - nrad - Sp


def get_theta(orc):
    nrad, Sp, S = sizes(orc)
    return np.array([pointer_of(orc, c)[0][pointer_of(orc, c)[1]] for c in range(nrad + Sp + S)])


def set_theta(orc, theta):
    for c, v in enumerate(theta):
        p, k = pointer_of(orc, c)
        p[k] = float(v)


def oracle_value(orc, s):
    """dict(eatom [nlocal], force [nlocal, 3] folded, vatom [nlocal, 6]) of a driver.System"""
    r = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh)
    return dict(eatom=r["eatom"][:s.nlocal].copy(), force=s.fold_forces(r["f"]), vatom=r["vatom"][:s.nlocal].copy())


def scalar(val, ebar, fbar, vbar):
    return float((ebar * val["eatom"]).sum() + (fbar * val["force"]).sum() + (vbar * val["vatom"]).sum())


def fd_gradient(orc, s, ebar, fbar, vbar, cols):
    """Richardson finite difference of the oracle's scalar for the listed columns; returns (grad [len(cols)], floor: the
    largest disagreement between the last two extrapolations)"""
    out, floor = np.zeros(len(cols)), 0.0
    for q, col in enumerate(cols):
        p, k = pointer_of(orc, col)
        c0 = p[k]
        h = 1e-3 * max(abs(c0), 0.05)
        d = []
        try:
            for hh in (h, 0.5 * h, 0.25 * h):
                p[k] = c0 + hh
                sp = scalar(oracle_value(orc, s), ebar, fbar, vbar)
                p[k] = c0 - hh
                sm = scalar(oracle_value(orc, s), ebar, fbar, vbar)
                d.append((sp - sm) / (2.0 * hh))
        finally:
            p[k] = c0
        r1 = [(4.0 * d[1] - d[0]) / 3.0, (4.0 * d[2] - d[1]) / 3.0]
        r2 = (16.0 * r1[1] - r1[0]) / 15.0
        out[q] = r2
        floor = max(floor, abs(r2 - r1[1]))
    return out, floor


def cotangents(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=(n, 6))


def sample_columns(orc, nradial, seed=11):
    """a fixed-seed sample of `nradial` radial columns plus every species column and the first and last moment column"""
    nrad, Sp, S = sizes(orc)
    rad = np.sort(np.random.default_rng(seed).choice(nrad, size=min(nradial, nrad), replace=False))
    return [int(c) for c in rad] + list(range(nrad, nrad + Sp)) + [nrad + Sp, nrad + Sp + S - 1]


def twin_loss(tables, systems, labels, theta, weights=(1.0, 0.01, 0.001), grad=True):
    """the objective of md.loss_cells from the numpy twin: systems = driver.System per configuration (None for an empty
    one), labels as for md.fit_linear.  Returns dict(loss, grad [C], grad_cfg [ncfg, C], row_absmax [C]: the largest per-atom row entry of
    every column, energy, forces, virial)."""
    from lammps_mtp_kokkos_amd.driver import train_twin
    w_e, w_f, w_s = weights
    C = len(theta)
    loss, rows, es, fs, vs = 0.0, [], [], [], []
    absmax = np.zeros(C)
    for s, l in zip(systems, labels):
        if s is None or s.nlocal == 0:
            rows.append(np.zeros(C)), es.append(0.0), fs.append(np.zeros((0, 3))), vs.append(np.zeros(6))
            continue
        n = s.nlocal
        val = train_twin(tables, s, theta)
        E, F, V = val["eatom"].sum(), val["force"], val["vatom"].sum(0)
        ebar, fbar, vbar = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 6))
        if l.get("energy") is not None and w_e > 0:
            loss += w_e * ((E - l["energy"]) / n) ** 2
            ebar[:] = 2.0 * w_e * (E - l["energy"]) / n ** 2
        if l.get("f") is not None and w_f > 0:
            loss += w_f * ((F - l["f"]) ** 2).sum()
            fbar = 2.0 * w_f * (F - l["f"])
        if l.get("virial") is not None and w_s > 0:
            loss += w_s * (((V - l["virial"]) / n) ** 2).sum()
            vbar[:] = 2.0 * w_s * (V - l["virial"]) / n ** 2
        r = train_twin(tables, s, theta, ebar, fbar, vbar)["rows"] if grad else np.zeros((n, C))
        absmax = np.maximum(absmax, np.abs(r).max(0))
        rows.append(r.sum(0))
        es.append(E), fs.append(F), vs.append(V)
    g = np.array(rows)
    return dict(loss=float(loss), grad=g.sum(0), grad_cfg=g, row_absmax=absmax, energy=np.array(es), forces=np.concatenate(fs), virial=np.array(vs))


def star_system(st, neigh=None):
    """a star set of tests/_stars.py as a driver.System in which every atom is owned and is its own owner (nlocal = nall,
    owner = arange): list row k belongs to atom ilist[k], so per-row and per-atom arrays no longer coincide"""
    from lammps_mtp_kokkos_amd.driver import System
    return System(x=st.x, types=st.types, nlocal=st.nall, owner=np.arange(st.nall), box=np.zeros(3), ilist=st.ilist,
                  first=st.first, neigh=st.neigh if neigh is None else neigh, cutoff=st.rc)


def star_set(tables, KL, seed, special=None, order="mixed", shuffle=True):
    """stars of tests/_stars.py for a potential's species count and cutoff, their exact counts asserted, rows shuffled (not where the order of a row is the point: shuffle = False)"""
    import _stars
    Sp, rc = len(tables["species_coeffs"]), float(tables["max_cutoff"])
    rng = np.random.default_rng(seed)
    st = _stars.stars(KL, rng, species=Sp, rc=rc, rin=(2.1, rc), rout=(rc, rc + 2.0), order=order, special=special)
    assert _stars.counts(st) == KL
    if shuffle:
        st.neigh = _stars.shuffled_rows(st, rng)
    return st


def row_cotangents(st, seed):
    """ebar [stars], fbar [nall, 3], vbar [stars, 6]: by list row, by atom, by list row"""
    rng = np.random.default_rng(seed)
    n = len(st.ilist)
    return rng.normal(size=n), rng.normal(size=(st.nall, 3)), rng.normal(size=(n, 6))


def by_atom(st, a):
    """a per-row array on the atoms: out[ilist[k]] = a[k], zero elsewhere (the twin and the device take ebar and vbar by
    ROW, the oracle's scalar of _train.fd_gradient by ATOM)"""
    out = np.zeros((st.nall,) + a.shape[1:])
    out[st.ilist] = a
    return out


def padded_rows(st, a):
    """a per-row array at the length the twin asks for (nlocal = nall); rows past the list are never read"""
    out = np.zeros((st.nall,) + a.shape[1:])
    out[:len(a)] = a
    return out


# K and L of the training and design kernels' edges: tiles of 32 survivors, a compaction sweep of 64 listed entries
STAR_EDGE_KL = [(K, L) for K in (0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 97) for L in (K, K + 1, 129)] + \
    [(K, L) for K in (1, 33) for L in (63, 64, 65, 128)]


def grid_stride_KL(num_cus, rng):
    """8 num_cus + 64 rows: more than any launch of the training or design kernel has workgroups (at most 8 per CU), so
    the last rows are second trips of the first workgroups.  With the full 8 per CU workgroup b < 64 takes row b and then
    row 8 num_cus + b: a K = 0 row after a three-tile row, a three-tile row after a one-neighbour row, one tile after four"""
    head = [(K, K + 1) for K in (65, 64, 33, 32, 1, 0, 97, 2)] * 8
    tail = [(K, K + 1) for K in (0, 1, 33, 2, 65, 0, 3, 1)] * 8
    mid = [(int(K), int(K)) for K in rng.integers(0, 4, 8 * num_cus - 64)]
    return head + mid + tail


def star_block_ratio(got_rows, want_rows, nrad, Sp, KL, what):
    """gradient rows of a star set, one row per star: |got - want| / (1e-9 + 1e-10 max |want| over THAT star's row in the
    block), per block of columns (radial, species, moments) -- the bound of _design.column_ratio with the scale taken per
    star, so that a three-tile star with entries of 1e6 cannot hide a one-neighbour star (the rule of
    _stars.per_star_check).  Prints and returns the worst ratio; a miss names the star's (K, L)."""
    got, want = np.asarray(got_rows, dtype=np.float64), np.asarray(want_rows, dtype=np.float64)
    assert got.shape == want.shape == (len(KL), want.shape[-1]), (got.shape, want.shape, len(KL))
    assert np.isfinite(got).all(), what + ": a gradient row is not finite"
    worst = 0.0
    for name, a, b in (("radial", 0, nrad), ("species", nrad, nrad + Sp), ("moments", nrad + Sp, want.shape[-1])):
        if len(KL) == 0 or b == a:
            continue
        w = want[:, a:b]
        ratio = (np.abs(got[:, a:b] - w) / (1e-9 + 1e-10 * np.abs(w).max(1))[:, None]).max(1)
        s = int(np.argmax(ratio))
        print("%s %s: worst error / bound %.3e at star %d (K, L) = %s" % (what, name, ratio[s], s, KL[s]))
        assert ratio[s] <= 1.0, "%s %s: star %d (K, L) = %s misses 1e-9 + 1e-10 max|its row| %.2f-fold" % (
            what, name, s, KL[s], ratio[s])
        worst = max(worst, float(ratio[s]))
    return worst


def block_ratio(got, want, nrad, Sp, what):
    """_design.column_ratio per block of columns (radial, species, moments); prints and returns the worst"""
    import _design
    worst = 0.0
    for name, a, b in (("radial", 0, nrad), ("species", nrad, nrad + Sp), ("moments", nrad + Sp, want.shape[-1])):
        r = _design.column_ratio(got[..., a:b], want[..., a:b])
        print("%s %s: worst error / bound %.3e" % (what, name, r))
        worst = max(worst, r)
    return worst


def sum_ratio(got, want, nrows, row_absmax, what):
    """a sum of `nrows` per-atom gradient rows against the same sum of twin rows.  Every per-atom entry is held to
    1e-9 + 1e-10 max |column| over the per-atom rows (the bound of _design.column_ratio), so a sum of nrows of them is held
    to nrows times that; prints and returns the worst error / bound"""
    bound = max(int(nrows), 1) * (1e-9 + 1e-10 * np.asarray(row_absmax))
    ratio = float((np.abs(np.asarray(got) - np.asarray(want)) / bound).max())
    print("%s: worst error / bound %.3e" % (what, ratio))
    return ratio
