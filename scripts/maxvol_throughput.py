#!/usr/bin/env python
"""Time per swap of the device MaxVol selection (mtp_maxvol_select) against the same loop written with torch.

Pool: the 65,536 per-atom candidate vectors of the headline lattice (32 x 32 x 32 jittered bcc cells) on W_L16_nbh.almtp
(C = 149, cpad = 160), threshold 1.1.  Both legs start from the potential's active set and run in one process, in
alternation (library, torch, library, torch, ...) after one warm-up each; a run is timed with a host clock around a call
that ends in a device synchronise, and the median of `--runs` runs is reported.

  library   Context.maxvol_select: one pivot kernel and one pass over the (C + N) x cpad stacked matrix per swap, a
            16-byte status read every 16 swaps, fresh grades every 64 swaps and before the end
  torch     what a user can do without it: G = V W^T once, then per swap argmax |G| (one host wait), u, and two `outer`
            updates (W^T and G)

--pool random times the same loop on a pool that needs about C swaps (profiles/maxvol_throughput_random.json).  The
byte floor per swap is 2 * 8 * (N + C) * cpad bytes (the stacked matrix read and written once); its fraction is taken
over 6.3 TB/s.  Writes profiles/maxvol_throughput.json.

    python scripts/maxvol_throughput.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12   # bytes per second


def torch_loop(torch, V, S, W, threshold, max_swaps):
    C = S.shape[0]
    Wt = W.t().contiguous()
    G = V[:, :C] @ Wt
    swaps = 0
    while swaps < max_swaps:
        k = torch.argmax(G.abs())
        k, p = torch.stack([k.double(), G.view(-1)[k]]).tolist()   # the host wait of every swap: index and pivot together
        if not abs(p) > threshold:
            break
        i, j = divmod(int(k), C)
        u = G[i].clone()
        u[j] -= 1.0
        u /= p
        Wt -= torch.outer(Wt[:, j], u)
        G -= torch.outer(G[:, j], u)
        swaps += 1
    torch.cuda.synchronize()
    return swaps, Wt.t().contiguous(), float(G.abs().max().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32, help="bcc cells per edge (32 -> 65,536 atoms)")
    ap.add_argument("--threshold", type=float, default=1.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pool", default="lattice", choices=["lattice", "random"],
                    help="random: as many rows of normal(N, C) . exp(normal(0, 2)) per column -- a pool that needs about C "
                         "swaps, where the per-call costs no longer weigh on the time per swap")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxvol_throughput.json"))
    args = ap.parse_args()
    import torch
    from lammps_mtp_kokkos_amd import capi, mtpgen
    from lammps_mtp_kokkos_amd.md import evaluate_cell
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    pot = capi.Potential(os.path.join(ROOT, "potentials", "W_L16_nbh.almtp"), selection=True)
    ctx = capi.Context(pot, 0)
    C = int(pot.info.coeff_count)
    cpad = (C + 15) // 16 * 16
    pos, box = mtpgen.bcc_lattice(args.cells, args.cells, args.cells, a=3.165, jitter=0.05, seed=777)
    r = evaluate_cell(ctx, pos, np.diag(box), list_cutoff=7.0, vflag=0, grades=True)
    N = len(pos)
    V = ctx.candidates()[:N].clone()
    if args.pool == "random":
        rng = np.random.default_rng(7)
        V = torch.from_numpy(rng.normal(size=(N, C)) * np.exp(rng.normal(0.0, 2.0, size=C))[None, :]).cuda()
    st = torch.cuda.current_stream().cuda_stream
    S_t = torch.from_numpy(pot.active_set()).cuda()
    W_t = torch.from_numpy(pot.tables()["inverse_active_set"]).cuda()
    max_swaps = 4 * C

    def library():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ctx.maxvol_select(V, args.threshold, stream=st)     # ends in a synchronise of its stream
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    def with_torch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = torch_loop(torch, V, S_t, W_t, args.threshold, max_swaps)
        return time.perf_counter() - t0, out

    library()
    with_torch()
    lib_s, torch_s = [], []
    for _ in range(args.runs):
        t, res = library()
        lib_s.append(t)
        t, (tswaps, tW, tmax) = with_torch()
        torch_s.append(t)
    ns = res["nswaps"]
    floor_bytes = 2 * 8 * (N + C) * cpad
    lib_med, torch_med = float(np.median(lib_s)), float(np.median(torch_s))
    what = "per-atom candidate vectors, %d^3 jittered bcc cells" % args.cells if args.pool == "lattice" else "random rows"
    out = dict(pool="%d %s, W_L16_nbh.almtp" % (N, what), N=N, C=C,
               cpad=cpad, threshold=args.threshold, max_grade_before=r["max_grade"], converged=res["converged"], swaps=ns,
               max_grade_after=res["max_grade_after"], log_volume_gain=res["log_volume_gain"],
               library_seconds=lib_s, torch_seconds=torch_s, torch_swaps=tswaps, torch_max_grade_after=tmax,
               library_us_per_swap=1e6 * lib_med / max(ns, 1), torch_us_per_swap=1e6 * torch_med / max(tswaps, 1),
               floor_bytes_per_swap=floor_bytes, floor_us_per_swap=1e6 * floor_bytes / HBM_ACHIEVABLE,
               fraction_of_byte_floor=(floor_bytes / HBM_ACHIEVABLE) / (lib_med / max(ns, 1)),
               library_over_torch_time=lib_med / torch_med,
               max_abs_difference_of_inverse=float(np.abs(tW.cpu().numpy() - res["inverse_active_set"]).max()))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("swaps", "torch_swaps", "library_us_per_swap", "torch_us_per_swap",
                                          "fraction_of_byte_floor", "library_over_torch_time")}))


if __name__ == "__main__":
    main()
