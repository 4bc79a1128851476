#!/usr/bin/env python
"""Training gradient: one md.loss_cells call (loss and its gradient with respect to all C coefficients) against the only
route to the same vector before it existed -- central differences of the loss through md.evaluate_cells on 2 C
potentials, each the source with one coefficient moved by +h or -h, written by capi.write_all_coeffs.

Workload: 512 jittered 16-atom bcc cells (2 x 2 x 2 cubic), W_L16.mtp, C = 149 coefficients; labels are the potential's
own energies, forces and virials, the gradient is taken at coefficients 1 % away from the file's.  One child process under
its own `timeout` writes and loads the 2 C potentials (outside the timed windows; every potential of both legs is loaded
with the same settings), warms both legs up and times them in alternation, `--windows` windows each, with a host clock
around calls that end in a device synchronise; a window of the new leg is `--reps` calls back to back.  The parent writes
the two times (median window), their ratio and the largest difference between the two gradients to
profiles/train_throughput.json.

    python scripts/train_throughput.py                  # writes the profile
    python scripts/train_throughput.py --child          # the measurement in this process, prints its JSON line
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(ncfg, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    rng = np.random.default_rng(seed)
    return [(pos + rng.normal(0.0, 0.05, pos.shape), np.diag(box), None) for _ in range(ncfg)]


def host_loss(res, labels, weights):
    w_e, w_f, w_s = weights
    loss = 0.0
    for r, l in zip(res, labels):
        n = len(l["f"])
        loss += w_e * ((r["energy"] - l["energy"]) / n) ** 2 + w_f * ((r["f"] - l["f"]) ** 2).sum() \
            + w_s * (((r["virial"] - l["virial"]) / n) ** 2).sum()
    return float(loss)


def child(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import evaluate_cells, loss_cells
    assert torch.cuda.is_available(), "this measurement needs the MI355X"

    def stage(what):                                         # progress on stderr: a run that its time limit ends says where
        print("[train_throughput %7.1f s] %s" % (time.perf_counter() - t_start, what), file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    os.environ.setdefault("MTP_BANK_ROUNDS", "2")            # (as scripts/design_throughput.py: the same settings for every load)
    os.environ.setdefault("MTP_BANK_SCALE", "1")
    weights = (1.0, 0.01, 0.001)
    src = os.path.join(ROOT, "potentials", "W_L16.mtp")
    pot = capi.Potential(src)
    ctx = capi.Context(pot, 0)
    info = pot.info
    Sp, S = info.species_count, info.alpha_scalar_count
    nrad = Sp * Sp * info.radial_func_count * info.radial_basis_size
    cfgs = workload(args.configs)
    ntot = sum(len(p) for p, _, _ in cfgs)
    labels = [dict(energy=r["energy"], f=r["f"], virial=r["virial"]) for r in evaluate_cells(ctx, cfgs, list_cutoff=7.0, vflag=1)]
    theta = pot.theta() * (1.0 + 0.01 * np.random.default_rng(5).normal(size=nrad + Sp + S))
    cols = list(range(len(theta))) if args.columns <= 0 else list(range(0, len(theta), max(1, len(theta) // args.columns)))
    steps = [1e-4 * max(abs(theta[c]), 0.05) for c in cols]
    stage("source potential loaded, labels computed")
    with tempfile.TemporaryDirectory() as tmp:               # files and contexts: outside the timed windows
        pairs = []
        for c, h in zip(cols, steps):
            pair = []
            for sign in (1.0, -1.0):
                th = theta.copy()
                th[c] += sign * h
                path = os.path.join(tmp, "p.mtp")
                capi.write_all_coeffs(src, path, th[nrad + Sp:], th[nrad:nrad + Sp], th[:nrad])
                pair.append(capi.Context(capi.Potential(path), 0))
            pairs.append(pair)
    stage("%d displaced potentials written and loaded" % (2 * len(pairs)))

    def new_leg():
        return loss_cells(ctx, cfgs, labels, theta=theta, weights=weights, list_cutoff=7.0)["grad"]   # (ends in a synchronise)

    def loop_leg():
        return np.array([(host_loss(evaluate_cells(p, cfgs, list_cutoff=7.0, vflag=1), labels, weights)
                          - host_loss(evaluate_cells(m, cfgs, list_cutoff=7.0, vflag=1), labels, weights)) / (2.0 * h)
                         for (p, m), h in zip(pairs, steps)])

    reps = dict(loss_cells=args.reps, loop=1)
    g = new_leg()
    stage("loss_cells leg warmed up")
    fd = loop_leg()
    stage("finite-difference leg warmed up")
    times = dict(loss_cells=[], loop=[])
    for _ in range(args.windows):                            # the two legs in alternation
        for name, leg in (("loss_cells", new_leg), ("loop", loop_leg)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                out = leg()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps[name])
            stage("%s leg: %.5f s per gradient, window of %d" % (name, times[name][-1], reps[name]))
            if name == "loss_cells":
                g = out
            else:
                fd = out
    scale = len(theta) / len(cols)                           # a sampled loop, scaled to all C columns
    print(json.dumps(dict(configs=args.configs, atoms=ntot, coefficients=len(theta), columns_differenced=len(cols),
                          potential="W_L16.mtp", windows=args.windows, loss_cells_calls_per_window=args.reps,
                          loss_cells_seconds=times["loss_cells"], loop_seconds=times["loop"],
                          loss_cells_median=float(np.median(times["loss_cells"])),
                          loop_median=float(np.median(times["loop"])), loop_scaled_to_all_columns=float(np.median(times["loop"]) * scale),
                          max_abs_difference=float(np.abs(g[cols] - fd).max()), max_abs_gradient=float(np.abs(g).max()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--configs", type=int, default=512)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="loss_cells calls in one timed window of the new leg")
    ap.add_argument("--columns", type=int, default=0, help="difference about this many columns only and scale (0: all C)")
    ap.add_argument("--timeout", type=int, default=900, help="seconds for the measuring process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_throughput.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--configs", str(args.configs), "--windows", str(args.windows), "--reps", str(args.reps), "--columns", str(args.columns)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:                                    # nothing more is started on the GPU after a failure
        sys.exit("the measurement failed with status %d" % p.returncode)
    m = json.loads(p.stdout.strip().splitlines()[-1])
    result = dict(workload="%d jittered 16-atom bcc cells (2x2x2 cubic), W_L16.mtp, loss and gradient for %d coefficients"
                  % (args.configs, m["coefficients"]),
                  loss_cells_seconds=m["loss_cells_median"], finite_difference_loop_seconds=m["loop_scaled_to_all_columns"],
                  ratio=m["loop_scaled_to_all_columns"] / m["loss_cells_median"], max_abs_difference=m["max_abs_difference"],
                  max_abs_gradient=m["max_abs_gradient"], measurement=m)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("loss_cells_seconds", "finite_difference_loop_seconds", "ratio", "max_abs_difference")}))


if __name__ == "__main__":
    main()
