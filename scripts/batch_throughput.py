#!/usr/bin/env python
"""Configurations per second for many small periodic cells: the loop over md.evaluate_cell (one ghost build, one list
build and one force launch per configuration) against md.evaluate_cells (one of each per batch).

Workload: 512 jittered 16-atom bcc cells (2 x 2 x 2 cubic), W_L16.mtp, forces + virial.  Each leg runs in a fresh child
process under its own `timeout`, warms up, then times `--windows` windows with a host clock around work that ends in a
device synchronise; a leg that fails ends the run.  The parent writes the two rates (median window) and their ratio to
profiles/batch_throughput.json.

    python scripts/batch_throughput.py                  # both legs, writes the profile
    python scripts/batch_throughput.py --leg batch      # one leg in this process, prints its JSON line
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(ncfg, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    rng = np.random.default_rng(seed)
    return [(pos + rng.normal(0.0, 0.05, pos.shape), np.diag(box), None) for _ in range(ncfg)]


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import evaluate_cell, evaluate_cells
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", "W_L16.mtp")), 0)
    cfgs = workload(args.configs)
    if args.leg == "loop":
        def once():
            return [evaluate_cell(ctx, p, c, t, list_cutoff=7.0, vflag=1) for p, c, t in cfgs]
        calls = 1
    else:
        def once():
            return evaluate_cells(ctx, cfgs, list_cutoff=7.0, vflag=1)
        calls = args.batch_calls
    out = once()                                             # warm-up: every shape of the timed window
    once()
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = once()                                     # (both paths end in a device synchronise and a copy back)
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / calls)
    res = dict(leg=args.leg, configs=args.configs, atoms_per_config=16, potential="W_L16.mtp", vflag=1,
               calls_per_window=calls, seconds_per_batch=windows, configs_per_second=args.configs / float(np.median(windows)),
               energy_sum=float(sum(r["energy"] for r in out)), fmax=float(max(np.abs(r["f"]).max() for r in out)))
    if args.leg == "batch":                                  # the two paths compute the same thing
        ref = [evaluate_cell(ctx, p, c, t, list_cutoff=7.0, vflag=1) for p, c, t in cfgs[:16]]
        res["max_force_difference_to_evaluate_cell"] = float(max(np.abs(a["f"] - b["f"]).max() for a, b in zip(out, ref)))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["loop", "batch"], default=None)
    ap.add_argument("--configs", type=int, default=512)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--batch-calls", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in ("loop", "batch"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--configs", str(args.configs), "--windows", str(args.windows), "--batch-calls", str(args.batch_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    result = dict(workload="%d jittered 16-atom bcc cells (2x2x2 cubic), W_L16.mtp, forces + virial" % args.configs,
                  loop_configs_per_second=legs["loop"]["configs_per_second"],
                  batch_configs_per_second=legs["batch"]["configs_per_second"],
                  ratio=legs["batch"]["configs_per_second"] / legs["loop"]["configs_per_second"], legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("loop_configs_per_second", "batch_configs_per_second", "ratio")}))


if __name__ == "__main__":
    main()
