#!/usr/bin/env python
"""Configuration-steps per second of md.relax_cells_vc against what a user could do without it -- one md.evaluate_cells call per
step at the current cells with the variable-cell FIRE minimiser in numpy (the rules of mtp_relax_cell_step, vectorised over equal
cells) -- and against md.relax_cells on the same batch: the price of the per-atom virial, its reduction, the deform launch and
the wider monitor read.

Workload and rules: those of scripts/relax_throughput.py -- 512 jittered 16-atom bcc cells, W_L16.mtp, no grade steps, FIRE at
the defaults except ftol = stol = 0 (nothing converges, so all legs make the same steps) and dmax = 0.001 A (see there: the
synthetic potentials have holes; with this cap no coordinate travels further than 0.1 A and no cell strains by more than
100 x 0.001 / 16 in the timed 100 steps), pressure 0, the full cell mask.  Each leg runs in a fresh child process under its own
`timeout`, warms up with a shorter run of the same shapes, then times `--windows` windows with a host clock around work that
ends in a device synchronise; a leg that fails ends the run and nothing is tried again.  The variable-cell leg also checks
itself at the timed size: 20 steps against the per-call loop.  The parent writes the three rates (median window) to
profiles/relax_vc_throughput.json.

    python scripts/relax_vc_throughput.py               # the three legs, writes the profile
    python scripts/relax_vc_throughput.py --leg vc      # one leg in this process, prints its JSON line
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

from scripts.relax_throughput import FIRE, MASS, POTENTIAL, workload  # noqa: E402

FIRE = dict(FIRE)
VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def host_loop_vc(ctx, cfgs, steps, full=False):
    """what a user does without relax_cells_vc: evaluate_cells once per step at the current cells, FIRE over atoms and cells in
    numpy over all cells at once (they have the same size; nothing converges).  Returns the sum of the final energies, or with
    full=True (x, cells, energies)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, FTM2V
    p = FIRE
    xt = np.stack([c[0] for c in cfgs])
    h0 = np.stack([c[1] for c in cfgs])
    ncfg, L = len(cfgs), float(xt.shape[1])
    D = np.tile(np.eye(3), (ncfg, 1, 1))
    vt, vq = np.zeros_like(xt), np.zeros_like(D)
    dt, alpha, npos = np.full(ncfg, p["dt"]), np.full(ncfg, p["alpha_start"]), np.zeros(ncfg, dtype=np.int64)
    for step in range(steps + 1):
        h, x = h0 @ D, xt @ D
        res = evaluate_cells(ctx, [(x[k], h[k], c[2]) for k, c in enumerate(cfgs)], list_cutoff=7.0, vflag=1)
        if step == steps:                                    # (the last step only decides)
            break
        f = np.stack([r["f"] for r in res])
        W = np.zeros((ncfg, 3, 3))
        for q, (a, b) in enumerate(VOIGT):
            W[:, a, b] = W[:, b, a] = [r["virial"][q] for r in res]
        G = np.linalg.inv(D).transpose(0, 2, 1) @ W / L       # (pressure 0, the full mask)
        ft = f @ D.transpose(0, 2, 1)
        P = (ft * vt).sum((1, 2)) + (G * vq).sum((1, 2))
        vv = (vt * vt).sum((1, 2)) + (vq * vq).sum((1, 2))
        ff = (ft * ft).sum((1, 2)) + (G * G).sum((1, 2))
        down = P > 0.0
        npos = np.where(down, npos + 1, 0)
        grow = down & (npos > p["n_min"])
        a = np.where(down, 1.0 - alpha, 0.0)[:, None, None]
        b = np.where(down, alpha * np.sqrt(vv / ff), 0.0)[:, None, None]
        dt = np.where(grow, np.minimum(dt * p["f_inc"], p["dt_max"]), np.where(~down & (vv > 0.0), dt * p["f_dec"], dt))
        alpha = np.where(grow, alpha * p["f_alpha"], np.where(down, alpha, p["alpha_start"]))
        vm, vqm = a * vt + b * ft, a * vq + b * G
        vmax = np.maximum(np.abs(vm).max((1, 2)), np.abs(vqm).max((1, 2)))
        dtv = np.where(dt * vmax > p["dmax"], p["dmax"] / np.maximum(vmax, 1e-300), dt)[:, None, None]
        xt += dtv * vm
        D = D + dtv * vqm / L
        vt = vm + (dtv * FTM2V / MASS) * ft
        vq = vqm + (dtv * FTM2V / MASS) * G
    e = np.array([r["energy"] for r in res])
    return (x, h, e) if full else float(e.sum())


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import relax_cells, relax_cells_vc
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", POTENTIAL)), 0)
    cfgs = workload(args.configs)
    calls, checks = args.relax_calls, {}
    vc = dict(FIRE, stol=0.0, pressure=0.0, masses=MASS, list_cutoff=7.0)
    if args.leg == "vc":
        got = relax_cells_vc(ctx, cfgs, 20, **vc)
        xw, hw, ew = host_loop_vc(ctx, cfgs, 20, full=True)
        dx = np.stack([q["x"] for q in got["final"]]) - xw
        dx -= np.round(dx @ np.linalg.inv(hw)) @ hw
        checks = dict(fire20_max_position_difference_to_per_call_loop=float(np.abs(dx).max()),
                      fire20_max_cell_difference_to_per_call_loop=float(np.abs(np.stack([q["cell"] for q in got["final"]]) - hw).max()),
                      fire20_max_energy_difference_to_per_call_loop=float(np.abs(np.array([q["energy"] for q in got["final"]]) - ew).max()),
                      fire20_max_cell_change=float(np.abs(hw - np.stack([c[1] for c in cfgs])).max()))
        assert checks["fire20_max_position_difference_to_per_call_loop"] < 1e-10, checks
        assert checks["fire20_max_cell_difference_to_per_call_loop"] < 1e-10, checks
        assert checks["fire20_max_energy_difference_to_per_call_loop"] < 1e-8, checks

        def once(steps):
            r = relax_cells_vc(ctx, cfgs, steps, **vc)
            assert r["steps_done"] == steps and all(q["status"] == "running" for q in r["final"])
            return float(sum(q["energy"] for q in r["final"]))
    elif args.leg == "fixed":
        def once(steps):
            r = relax_cells(ctx, cfgs, steps, masses=MASS, list_cutoff=7.0, **FIRE)
            assert r["steps_done"] == steps and all(q["status"] == "running" for q in r["final"])
            return float(sum(q["energy"] for q in r["final"]))
    else:
        calls = 1

        def once(steps):
            return host_loop_vc(ctx, cfgs, steps)
    once(20)                                                 # warm-up: every shape and every kernel of the timed window
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            check = once(args.steps)                         # (every path ends in a copy back, which waits for the device)
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / calls)
        assert np.isfinite(check), "the state of leg %s went non-finite: nothing was measured" % args.leg
    print(json.dumps(dict(leg=args.leg, configs=args.configs, steps=args.steps, atoms_per_config=16, potential=POTENTIAL,
                          calls_per_window=calls, seconds_per_call=windows,
                          config_steps_per_second=args.configs * args.steps / float(np.median(windows)), energy_sum=check, **checks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["percall", "vc", "fixed"], default=None)
    ap.add_argument("--configs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--relax-calls", type=int, default=10, help="relax_cells_vc / relax_cells runs per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_vc_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in ("percall", "vc", "fixed"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--configs", str(args.configs), "--steps", str(args.steps), "--windows", str(args.windows),
               "--relax-calls", str(args.relax_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    rate = {k: v["config_steps_per_second"] for k, v in legs.items()}
    result = dict(workload="%d jittered 16-atom bcc cells (2x2x2 cubic), %s, %d FIRE steps over atoms and cells, ftol 0, stol 0, "
                           "dmax 0.001 A, pressure 0, no grade steps" % (args.configs, POTENTIAL, args.steps),
                  relax_cells_vc_config_steps_per_second=rate["vc"],
                  evaluate_cells_per_step_config_steps_per_second=rate["percall"],
                  relax_cells_config_steps_per_second=rate["fixed"],
                  ratio_to_evaluate_cells_per_step=rate["vc"] / rate["percall"],
                  ratio_to_relax_cells=rate["vc"] / rate["fixed"], legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("legs", "workload")}))


if __name__ == "__main__":
    main()
