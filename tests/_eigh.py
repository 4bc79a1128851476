"""The numpy twin of the batched symmetric eigen-solver (mtp_eigh_batched; include/mtp_mi355x.h, "batched symmetric
eigen-solver"), shared by tests/test_eigh_cpu.py and tests/test_eigh_gpu.py: steps 1-5 with the kernel's own expressions, the
kernel's own order of every sum and the kernel's own threshold (so that the device can be asked for the same BITS), stepped per
rotation step with vectorised element updates; the round-robin pair schedule; and the matrix families of the tests."""
import numpy as np

from _hess import BLOCK, segment_total, thread_sums

FAILED, NOT_CONVERGED, TOO_LARGE = 1, 2, 3
TIER_SMALL, MAX_N_VECTORS, MAX_N = 48, 96, 192
EPS = 2.0 ** -53


def schedule(N):
    """the steps of one sweep: for s = 0 ... M - 1 the arrays (p, q), p < q, of the Ne / 2 pairs in the kernel's order; an odd N
    has the padding index N in pair 0"""
    Ne = N + (N & 1)
    M, P = Ne - 1, Ne // 2
    k = np.arange(1, P)
    out = []
    for s in range(M):
        a = np.concatenate([[M], (s + k) % M])
        b = np.concatenate([[s], (s - k) % M])
        out.append((np.minimum(a, b), np.maximum(a, b)))
    return out


def _norm2(L, diagonal):
    """the kernel's norm2: thread t adds a_rc^2 for r N + c = t, t + NT, ..., then the workgroup total"""
    full = np.tril(L) + np.tril(L, -1).T
    sq = (full * full).reshape(-1)
    if not diagonal:
        keep = ~np.eye(len(L), dtype=bool).reshape(-1)
        # a skipped element leaves the thread's sum as it is: adding 0.0 does the same to a sum that starts at 0.0
        sq = np.where(keep, sq, 0.0)
    return segment_total(thread_sums(sq, BLOCK))


def prepare(A, root=None, project=False):
    """steps 1 and 2: the lower triangle the sweeps start from, as a full [N, N] array whose upper triangle is not used"""
    A = np.asarray(A, dtype=np.float64)
    N = len(A)
    with np.errstate(all="ignore"):
        if root is not None:
            rr = np.outer(root, root)
            x, y = A / rr, A.T / rr.T
        else:
            x, y = A, A.T
        L = np.tril(0.5 * (x + y))
        if project:
            rt = np.ones(N) if root is None else np.asarray(root, dtype=np.float64)
            nrm = np.zeros(3)
            for d in range(3):
                s = 0.0
                for i in range(d, N, 3):
                    s = s + rt[i] * rt[i]
                nrm[d] = np.sqrt(s)
            tau = rt / nrm[np.arange(N) % 3]
            full = L + np.tril(L, -1).T
            u = np.zeros((N, 3))
            for d in range(3):
                s = np.zeros(N)
                for i in range(d, N, 3):
                    s = s + full[:, i] * tau[i]
                u[:, d] = s
            g = np.zeros((3, 3))
            for d in range(3):
                s = np.zeros(3)
                for i in range(d, N, 3):
                    s = s + tau[i] * u[i]
                g[d] = s
            m3 = np.arange(N) % 3
            tr, tc = tau[:, None], tau[None, :]
            ucr = u[:, m3].T          # ucr[r, c] = u[c][r % 3]
            urc = u[:, m3]            # urc[r, c] = u[r][c % 3]
            grc = g[m3][:, m3]        # grc[r, c] = g[r % 3][c % 3]
            L = np.tril(((L - tr * ucr) - urc * tc) + (tr * grc) * tc)
    return L


def solve(A, root=None, project=False, max_sweeps=30, vectors=True):
    """What the kernel leaves for one matrix it serves: dict(W, V (None without `vectors`), info [2], status, A: the prepared
    matrix, symmetric).  A failed matrix has NaN in W, V and info."""
    A = np.asarray(A, dtype=np.float64)
    N = len(A)
    nan = np.nan
    failed = dict(W=np.full(N, nan), V=np.full((N, N), nan) if vectors else None, info=np.full(2, nan), status=FAILED, A=None)
    if (project and N % 3) or (root is not None and not np.isfinite(root).all()):
        return failed
    L = prepare(A, root, project)
    with np.errstate(all="ignore"):
        norm = np.sqrt(_norm2(L, True))
    if not np.isfinite(norm):
        return failed
    prepared = L + np.tril(L, -1).T
    thr = (norm * EPS) / float(N)
    Ne = N + (N & 1)
    P = Ne // 2
    # the work array has the padding row and column of an odd N: they read 0.0 and what is written there is thrown away
    Lp = np.zeros((Ne, Ne))
    Lp[:N, :N] = L
    V = np.eye(N)
    k1, k2 = np.tril_indices(P, -1)
    steps = schedule(N)
    sweeps, status = 0, NOT_CONVERGED
    while sweeps < max_sweeps:
        rotated = False
        for p, q in steps:
            real = q < N
            app, aqq, apq = Lp[p, p], Lp[q, q], Lp[q, p]
            rot = real & (np.abs(apq) > thr)
            with np.errstate(all="ignore"):
                zeta = (aqq - app) / (2.0 * apq)
                tn = np.where(zeta < 0.0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + tn * tn)
                sn = tn * c
                new_pp, new_qq = app - tn * apq, aqq + tn * apq
            c, sn = np.where(rot, c, 1.0), np.where(rot, sn, 0.0)
            Lp[p[rot], p[rot]], Lp[q[rot], q[rot]], Lp[q[rot], p[rot]] = new_pp[rot], new_qq[rot], 0.0
            rotated = rotated or bool(rot.any())
            if len(k1):
                p1, q1, p2, q2 = p[k1], q[k1], p[k2], q[k2]
                c1, s1, c2, s2 = c[k1], sn[k1], c[k2], sn[k2]
                live = (s1 != 0.0) | (s2 != 0.0)

                def at(r, cc):
                    return np.maximum(r, cc), np.minimum(r, cc)

                ipp, ipq, iqp, iqq = at(p1, p2), at(p1, q2), at(q1, p2), at(q1, q2)
                bpp, bpq, bqp, bqq = Lp[ipp], Lp[ipq], Lp[iqp], Lp[iqq]
                xpp, xpq = c1 * bpp - s1 * bqp, c1 * bpq - s1 * bqq
                xqp, xqq = s1 * bpp + c1 * bqp, s1 * bpq + c1 * bqq
                for idx, val in ((ipp, c2 * xpp - s2 * xpq), (ipq, s2 * xpp + c2 * xpq), (iqp, c2 * xqp - s2 * xqq),
                                 (iqq, s2 * xqp + c2 * xqq)):
                    Lp[idx[0][live], idx[1][live]] = val[live]
                if Ne != N:
                    Lp[N, :] = 0.0
                    Lp[:, N] = 0.0
            if vectors:
                use = real & (sn != 0.0)
                pu, qu, cu, su = p[use], q[use], c[use], sn[use]
                vp, vq = V[:, pu].copy(), V[:, qu].copy()
                V[:, pu] = cu * vp - su * vq
                V[:, qu] = su * vp + cu * vq
        sweeps += 1
        if not rotated:
            status = 0
            break
    L = np.tril(Lp[:N, :N])
    d = np.diag(L).copy()
    idx = np.arange(N)
    rank = ((d[None, :] < d[:, None]) | ((d[None, :] == d[:, None]) & (idx[None, :] < idx[:, None]))).sum(axis=1)
    W = np.zeros(N)
    W[rank] = d
    Vout = None
    if vectors:
        Vout = np.zeros((N, N))
        Vout[:, rank] = V
    with np.errstate(all="ignore"):
        off = np.sqrt(_norm2(L, False))
    return dict(W=W, V=Vout, info=np.array([float(sweeps), off]), status=status, A=prepared)


# ---- the matrix families of the tests

SIZES = (3, 6, 45, 48, 51, 96, 99, 162, 192)


def random_symmetric(N, seed):
    B = np.random.default_rng(seed).standard_normal((N, N))
    return 0.5 * (B + B.T)


def projector(N, root=None):
    """I - sum_d t_d t_d^T of md.modes (N a multiple of 3)"""
    rt = np.ones(N) if root is None else root
    T = np.zeros((N, 3))
    for d in range(3):
        T[d::3, d] = rt[d::3]
    T /= np.linalg.norm(T, axis=0)
    return np.eye(N) - T @ T.T


def degenerate_triples(N, seed):
    """eigenvalues 1, 1, 1, 2, 2, 2, ... in a random orthogonal frame"""
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((N, N)))[0]
    lam = 1.0 + (np.arange(N) // 3).astype(np.float64)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def family(name, N, seed=11):
    """(A, root, project) of the family `name` at size N"""
    if name == "random":
        return random_symmetric(N, seed), None, False
    if name == "projected":
        root = np.repeat(np.sqrt(np.random.default_rng(seed + 1).uniform(20.0, 200.0, N // 3)), 3)
        return random_symmetric(N, seed) * 50.0, root, True
    if name == "triples":
        return degenerate_triples(N, seed), None, False
    if name == "diagonal":
        return np.diag(np.random.default_rng(seed).standard_normal(N)), None, False
    if name == "zero":
        return np.zeros((N, N)), None, False
    raise KeyError(name)


FAMILIES = ("random", "projected", "triples", "diagonal", "zero")


def ratios(A, W, V):
    """the three figures of the bounds over their bounds' variable part: |lambda - lambda_lapack| / (N eps |A|_F),
    max |A V - V Lambda| / (N eps |A|_F) and max |V^T V - I| / (N eps); a zero matrix gives 0.0 for the first two when they vanish"""
    N = len(A)
    scale = N * EPS * np.linalg.norm(A)
    ref = np.linalg.eigvalsh(A)

    def over(x):
        return 0.0 if x == 0.0 else x / scale

    out = [over(np.abs(W - ref).max())]
    if V is not None:
        out += [over(np.abs(A @ V - V * W).max()), np.abs(V.T @ V - np.eye(N)).max() / (N * EPS)]
    return out


BOUNDS = (8.0, 8.0, 16.0)
