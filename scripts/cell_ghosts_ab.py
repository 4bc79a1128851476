"""A/B of the two device ghost builds on the headline box (32x32x32 bcc W, W_L16.mtp, rghost 7.0), alternating in one
process: mtp_ghosts_build (orthogonal box) against mtp_ghosts_build_cell (the same box as a diagonal 3x3 cell), and
the whole device-resident MD step of md.DeviceNVE with box= against cell=, set up as bench.py's whole-step number.

  python scripts/cell_ghosts_ab.py [--rounds 3] [--modes box,cell] [--cells 32]

--modes box runs on a library without the cell entry point (a parent build), for the parent's figure.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="box,cell")
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--builds", type=int, default=50)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    import torch
    from lammps_mtp_kokkos_amd import capi, mtpgen
    from lammps_mtp_kokkos_amd.md import DeviceNVE, MVV2E
    modes = args.modes.split(",")
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    pos, box = mtpgen.bcc_lattice(args.cells, args.cells, args.cells, a=3.165, jitter=0.05, seed=777)
    n = len(pos)
    shape = {"box": box, "cell": np.diag(box)}
    out = {"atoms": n, "rghost": 7.0, "modes": modes, "build_ms": {m: [] for m in modes}, "step_ms": {m: [] for m in modes}}

    # ---- the build alone: wrap + count + scan + fill + first forward, one stream synchronisation inside --------------
    g = {m: capi.Ghosts(0) for m in modes}
    xa = torch.zeros((int(n * 1.6) + 1024, 3), dtype=torch.float64, device=dev)
    x0 = torch.from_numpy(pos).to(dev)

    def build(m):
        return (g[m].build if m == "box" else g[m].build_cell)(xa, n, shape[m], 7.0, stream=st)

    for r in range(args.rounds + 1):          # round 0 warms up (allocations, code objects)
        for m in modes:
            t = 0.0
            for _ in range(args.builds):
                xa[:n] = x0                   # unwrapped input every time, outside the clock
                torch.cuda.synchronize()
                c0 = time.perf_counter()
                nall = build(m)
                torch.cuda.synchronize()
                t += time.perf_counter() - c0
            out.setdefault("ghosts", {})[m] = nall - n
            if r:
                out["build_ms"][m].append(t / args.builds * 1e3)

    # ---- the whole step, as bench.py --full sets it up ---------------------------------------------------------------
    pot = capi.Potential(os.path.join(ROOT, "potentials", "W_L16.mtp"))
    rng = np.random.default_rng(300)
    vel = rng.normal(size=pos.shape) * np.sqrt(8.617343e-5 * 30.0 / (183.84 * MVV2E))
    vel_t = torch.from_numpy(vel - vel.mean(0)).to(dev)
    ctx = {m: capi.Context(pot, 0) for m in modes}
    last = {}
    for r in range(args.rounds):
        for m in modes:
            # a fresh run every window, as bench.py does: the synthetic potential is stiff and a bcc lattice is not its
            # minimum, so a trajectory is only followed for 10 + 60 steps of 0.25 fs from 30 K
            md = DeviceNVE(ctx[m], pos, shape[m], rc=pot.info.max_cutoff, mass=183.84, list_cutoff=7.0, device=dev, every=10,
                           check_every=0, vflag=1)
            md.v.copy_(vel_t)
            for _ in range(10):
                md.step(2.5e-4)
            torch.cuda.synchronize()
            b0 = md.builds
            c0 = time.perf_counter()
            for _ in range(args.steps):
                md.step(2.5e-4)
            torch.cuda.synchronize()
            out["step_ms"][m].append((time.perf_counter() - c0) / args.steps * 1e3)
            out.setdefault("rebuilds_per_window", {})[m] = md.builds - b0
            last[m] = md.x.cpu().numpy()
            del md
    if len(modes) == 2:                       # both integrate the same trajectory
        out["max_position_difference"] = float(np.abs(last[modes[0]] - last[modes[1]]).max())
    for k in ("build_ms", "step_ms"):
        out[k + "_mean"] = {m: float(np.mean(v)) for m, v in out[k].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
