#!/usr/bin/env python
"""The linear refit without the design matrix (md.normal_cells, md.solve_normal, csrc/mtp_normal.hip) against the SVD path.

Method of scripts/design_throughput.py: every leg runs in a process of its own under its own `timeout`, makes one warm-up
call and then times one window with a host clock around work that ends in a device synchronise; the parent starts the legs
in alternation, `--windows` processes per leg, and reports every window and the median.  Nothing more is started on the GPU
after a leg fails.

  (a) md.fit_linear on 512 jittered 16-atom bcc cells, W_L16.mtp (117 columns), labels from the potential itself:
      method="svd" against method="normal", a window is --fit-reps calls.  At this size the passes dominate both legs; no
      ratio is claimed.
  (b) the accumulate kernel alone (capi.Normal.accumulate, force kind) on resident synthetic matrices of 118 and 463
      augmented columns, as multiply-adds per second: `useful` counts rows n (n + 1) / 2, `issued` what the kernel executes
      (whole 64 x 64 tiles of the upper triangle); a window is --kernel-reps calls back to back.  Beside them the ceiling
      DESIGN.md 5.1 derives for vector instructions -- 0.25 per cycle and SIMD, 256 CUs x 4 SIMDs x 64 lanes at 2.4 GHz =
      3.93e13 lane-instructions / s -- at 10 per multiply-add.
  (c) a training set that md.design_cells refuses at the default max_design_bytes (2 GiB), fitted by method="normal": the
      time and the peak device memory (torch.cuda.max_memory_allocated).

    python scripts/normal_throughput.py                       # writes profiles/normal_throughput.json
    python scripts/normal_throughput.py --child a:normal      # one leg in this process, prints its JSON line
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

CEILING_MACS = 256 * 4 * 64 * 0.25 * 2.4e9 / 10.0
LEGS = ("a:svd", "a:normal", "b:118", "b:463", "c:normal")


def workload(ncfg, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    rng = np.random.default_rng(seed)
    return [(pos + rng.normal(0.0, 0.05, pos.shape), np.diag(box), None) for _ in range(ncfg)]


def own_labels(ctx, cfgs, chunk=4096):
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    out = []
    for a in range(0, len(cfgs), chunk):
        out += [dict(energy=r["energy"], f=r["f"], virial=r["virial"]) for r in evaluate_cells(ctx, cfgs[a:a + chunk])]
    return out


def child(leg, args):
    import torch
    from lammps_mtp_kokkos_amd import capi, md
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    os.environ.setdefault("MTP_BANK_ROUNDS", "2")              # the settings of scripts/design_throughput.py
    os.environ.setdefault("MTP_BANK_SCALE", "1")
    part, which = leg.split(":")
    dev = torch.device("cuda:0")

    def timed(fn):
        fn()                                                   # the warm-up: every shape of the timed window
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if part == "b":
        n = int(which)
        nrows, ld = args.kernel_rows, n - 1 + ((n - 1) & 1)
        st = capi.use_private_torch_stream(dev).cuda_stream
        g = torch.Generator(device=dev).manual_seed(5)
        rows = torch.randn((nrows, ld), dtype=torch.float64, device=dev, generator=g)
        scale = torch.ones(nrows, dtype=torch.float64, device=dev)
        target = torch.randn(nrows, dtype=torch.float64, device=dev, generator=g)
        nm = capi.Normal(n - 1, 0)

        def calls():                                           # one call is milliseconds: a window is --kernel-reps of them
            for _ in range(args.kernel_reps):
                nm.accumulate(1, nrows, ld, rows, scale, target, stream=st)

        seconds = timed(calls)[0] / args.kernel_reps
        tiles = (n + 63) // 64
        useful, issued = nrows * n * (n + 1) / 2.0, nrows * 4096.0 * tiles * (tiles + 1) / 2.0
        return dict(seconds=seconds, calls_per_window=args.kernel_reps, rows=nrows, augmented_columns=n,
                    useful_macs_per_second=useful / seconds, issued_macs_per_second=issued / seconds, ceiling_macs_per_second=CEILING_MACS,
                    issued_over_ceiling=issued / seconds / CEILING_MACS, round_slices=nm.info()["round_slices"])
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", "W_L16.mtp")), 0)
    if part == "a":
        cfgs = workload(args.configs)
        labels = own_labels(ctx, cfgs)
        seconds, res = timed(lambda: [md.fit_linear(ctx, cfgs, labels, method=which, device=dev) for _ in range(args.fit_reps)][-1])
        return dict(seconds=seconds / args.fit_reps, calls_per_window=args.fit_reps, configs=len(cfgs), rank=res["rank"], rmse_after=res["rmse_after"],
                    peak_bytes=int(torch.cuda.max_memory_allocated()))
    cfgs = workload(args.large_configs)
    labels = own_labels(ctx, cfgs)
    refused = None
    try:
        md.design_cells(ctx, cfgs, device=dev)
    except ValueError as e:
        refused = str(e)
    assert refused is not None, "design_cells accepted the large training set: raise --large-configs"
    seconds, res = timed(lambda: md.fit_linear(ctx, cfgs, labels, method="normal", max_atoms_per_pass=args.pass_atoms, device=dev))
    return dict(seconds=seconds, configs=len(cfgs), atoms=16 * len(cfgs), rank=res["rank"], rmse_after=res["rmse_after"],
                rows=res["state"].counts, peak_bytes=int(torch.cuda.max_memory_allocated()), design_cells_said=refused)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="one of " + ", ".join(LEGS))
    ap.add_argument("--configs", type=int, default=512)
    ap.add_argument("--large-configs", type=int, default=49152, help="(c): 786 432 atoms need 7.7 GB in design_cells")
    ap.add_argument("--pass-atoms", type=int, default=32768)
    ap.add_argument("--kernel-rows", type=int, default=262144)
    ap.add_argument("--fit-reps", type=int, default=5, help="(a): fit_linear calls in one timed window")
    ap.add_argument("--kernel-reps", type=int, default=20, help="(b): accumulate calls in one timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for one measuring process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_throughput.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child, args)))
        return
    runs = {leg: [] for leg in LEGS}
    for group in (("a:svd", "a:normal"), ("b:118", "b:463"), ("c:normal",)):
        for _ in range(args.windows):                          # the legs of a group in alternation
            for leg in group:
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", leg,
                       "--configs", str(args.configs), "--large-configs", str(args.large_configs), "--pass-atoms",
                       str(args.pass_atoms), "--kernel-rows", str(args.kernel_rows), "--kernel-reps", str(args.kernel_reps),
                       "--fit-reps", str(args.fit_reps)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if p.returncode != 0:                          # nothing more is started on the GPU after a failure
                    sys.exit("leg %s failed with status %d" % (leg, p.returncode))
                runs[leg].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print("[normal_throughput] %s: %.4f s" % (leg, runs[leg][-1]["seconds"]), file=sys.stderr, flush=True)
    result = {}
    for leg, rs in runs.items():
        sec = [r["seconds"] for r in rs]
        result[leg] = dict(median_seconds=float(np.median(sec)), window_seconds=sec, last=rs[-1])
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({leg: result[leg]["median_seconds"] for leg in LEGS}))


if __name__ == "__main__":
    main()
