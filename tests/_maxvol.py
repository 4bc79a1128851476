"""What the MaxVol selection tests share (tests/test_maxvol_cpu.py, tests/test_maxvol_gpu.py): the random pools, potential
files that carry a given selection state, the numpy twin's own drift (from which every device-against-numpy bound is
derived) and the replay of a logged swap sequence."""
import functools
import os

import numpy as np

from lammps_mtp_kokkos_amd.driver import maxvol_select_numpy

from _cells import POT

# coefficient count -> the committed potential whose text part a selection file of that size is built on
BASE = {26: "W_L8.mtp", 115: "WRe_L10_cfg.almtp", 149: "W_L16_nbh.almtp", 622: "WRe_L20.mtp"}
MVS = b"#MVS_v1.1"


def random_state(C, seed=99):
    """(S, W): S = 2 I + 0.05 U(-1, 1), W = inv(S) -- mtpgen.add_selection_state"""
    rng = np.random.default_rng(seed)
    S = 2.0 * np.eye(C) + 0.05 * rng.uniform(-1, 1, size=(C, C))
    return S, np.linalg.inv(S)


def random_pool(C, N, seed=7):
    """V [N, C] = normal(N, C) . exp(normal(0, 2)) per column"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(N, C)) * np.exp(rng.normal(0.0, 2.0, size=C))[None, :]


def selection_file(path, C, S, W, mode="nbh"):
    """a potential file with the text part of BASE[C] and the selection state (S, W) written by hand (not by the library)"""
    raw = open(os.path.join(POT, BASE[C]), "rb").read()
    cut = raw.find(MVS)
    text = raw if cut < 0 else raw[:cut]
    cfg = mode == "cfg"
    tail = ["#MVS_v1.1", "energy_weight = %d" % (1 if cfg else 0), "force_weight = 0", "stress_weight = 0",
            "site_en_weight = %d" % (0 if cfg else 1), "weight_scaling = 1"]
    with open(path, "wb") as fh:
        fh.write(text + ("\n".join(tail) + "\n").encode() + b"#" + np.ascontiguousarray(S, dtype="<f8").tobytes()
                 + np.ascontiguousarray(W, dtype="<f8").tobytes())
    return str(path)


@functools.lru_cache(maxsize=None)
def twin_run(C, N, threshold, seed=7):
    """the twin on the random pool: computed once per case, shared, never written to"""
    S, W = random_state(C)
    V = random_pool(C, N, seed)
    S1, W1, swaps, G = maxvol_select_numpy(V, S, W, threshold, 4 * C)
    return dict(S=S, W=W, V=V, S1=S1, W1=W1, swaps=swaps, G=G)


def twin_drift(V, S, W, threshold, max_swaps):
    """what the twin itself loses on this pool: max |rank-1-updated G - V W'^T| and max |W' S' - I|, with max |G|"""
    S1, W1, swaps, G = maxvol_select_numpy(V, S, W, threshold, max_swaps)
    C = S.shape[0]
    fresh = V[:, :C] @ W1.T
    drift = float(np.abs(G - fresh).max()) if G.size else 0.0
    return max(drift, float(np.abs(W1 @ S1 - np.eye(C)).max())), max(1.0, float(np.abs(fresh).max()) if G.size else 1.0)


def bound(V, S, W, threshold, max_swaps):
    """The tolerance rule of every device-against-numpy comparison: 100 x the twin's own drift on the same pool (floor
    1e-12), scaled by max(1, max |G|).  The figure comes from the twin, never from the device; the factor 100 covers the
    different association of the device's sums (MFMA order, FMA contraction)."""
    drift, scale = twin_drift(V, S, W, threshold, max_swaps)
    return max(100.0 * drift, 1e-12) * scale


def replay(V, S, W, swaps, threshold, tol):
    """The twin replays a logged swap sequence [(i, j, p)]: at every step the logged pivot must be, within tol, the largest
    |G| entry of the twin's own matrix, exceed the threshold and equal the twin's G[i, j].  Returns (S', W', G)."""
    C = S.shape[0]
    S = np.array(S, dtype=np.float64)
    Wt = np.array(W, dtype=np.float64).T.copy()
    G = V[:, :C] @ Wt
    for k, (i, j, p) in enumerate(swaps):
        top = float(np.abs(G).max())
        assert abs(G[i, j] - p) <= tol, "swap %d: logged pivot %.17g, the twin has %.17g" % (k, p, G[i, j])
        assert abs(p) >= top - tol, "swap %d: |pivot| %.17g is not the largest entry %.17g" % (k, abs(p), top)
        assert abs(p) > threshold, "swap %d: |pivot| %.17g does not exceed the threshold" % (k, abs(p))
        u = G[i].copy()
        u[j] -= 1.0
        u /= G[i, j]
        Wt -= np.outer(Wt[:, j], u)
        G -= np.outer(G[:, j], u)
        S[:, j] = V[i, :C]
    return S, Wt.T.copy(), G


def slot_source_of(swaps, C):
    src = np.full(C, -1, dtype=np.int64)
    for i, j, _ in swaps:
        src[j] = i
    return src
