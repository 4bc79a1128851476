#!/usr/bin/env python
"""Configuration-steps per second of md.relax_cells against what a user could do without it: one md.evaluate_cells call
per step with the FIRE minimiser in numpy (the rules of mtp_relax_step, vectorised over equal cells).

Workload: jittered 16-atom bcc cells (2 x 2 x 2 cubic) as in scripts/sample_throughput.py, W_L16.mtp (level 16), no grade
steps, FIRE at the defaults of relax_cells except ftol = 0 (nothing converges, so both legs make the same steps) and
dmax = 0.001 A.  The cap is that small on purpose: the synthetic potentials have holes at short distance, the jittered cells
carry forces of 30 eV/A, and at the default cap of 0.1 A a cell walks into a hole within some twenty steps -- timings of a
non-finite state say nothing.  With 0.001 A no coordinate travels further than 0.1 A in the timed 100 steps, the state stays
finite (every leg asserts it, and the relax leg that no configuration failed), and the time of a step does not depend on the
cap.  Each leg runs in a fresh child process under its own `timeout`, warms up with a shorter run of the same shapes, then
times `--windows` windows with a host clock around work that ends in a device synchronise; a leg that fails ends the run and
nothing is tried again.  The relax leg also checks itself at the timed size: 20 steps against the per-call loop.  The parent
writes the two rates (median window) to profiles/relax_throughput.json.

    python scripts/relax_throughput.py                  # both legs, writes the profile
    python scripts/relax_throughput.py --leg relax      # one leg in this process, prints its JSON line
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

MASS, POTENTIAL = 183.84, "W_L16.mtp"
FIRE = dict(ftol=0.0, dt=1e-3, dt_max=1e-2, dmax=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)


def workload(ncfg, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    rng = np.random.default_rng(seed)
    return [(pos + rng.normal(0.0, 0.05, pos.shape), np.diag(box), np.ones(len(pos), dtype=np.int32)) for _ in range(ncfg)]


def host_loop(ctx, cfgs, steps, full=False):
    """what a user does without relax_cells: evaluate_cells once per step, FIRE in numpy over all cells at once (they have the
    same size; nothing converges with ftol = 0).  Returns the sum of the final energies, or with full=True (x, energies)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, FTM2V
    p = FIRE
    x = np.stack([c[0] for c in cfgs])
    v = np.zeros_like(x)
    ncfg = len(cfgs)
    dt, alpha, npos = np.full(ncfg, p["dt"]), np.full(ncfg, p["alpha_start"]), np.zeros(ncfg, dtype=np.int64)
    for step in range(steps + 1):
        res = evaluate_cells(ctx, [(x[k], c[1], c[2]) for k, c in enumerate(cfgs)], list_cutoff=7.0, vflag=0)
        if step == steps:                                    # (the last step only decides)
            break
        f = np.stack([r["f"] for r in res])
        P, vv, ff = (f * v).sum((1, 2)), (v * v).sum((1, 2)), (f * f).sum((1, 2))
        down = P > 0.0
        npos = np.where(down, npos + 1, 0)
        grow = down & (npos > p["n_min"])
        a = np.where(down, 1.0 - alpha, 0.0)
        b = np.where(down, alpha * np.sqrt(vv / ff), 0.0)
        dt = np.where(grow, np.minimum(dt * p["f_inc"], p["dt_max"]), np.where(~down & (vv > 0.0), dt * p["f_dec"], dt))
        alpha = np.where(grow, alpha * p["f_alpha"], np.where(down, alpha, p["alpha_start"]))
        vm = a[:, None, None] * v + b[:, None, None] * f
        vmax = np.abs(vm).max((1, 2))
        dtv = np.where(dt * vmax > p["dmax"], p["dmax"] / np.maximum(vmax, 1e-300), dt)
        x += dtv[:, None, None] * vm
        v = vm + (dtv * FTM2V / MASS)[:, None, None] * f
    e = np.array([r["energy"] for r in res])
    return (x, e) if full else float(e.sum())


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import relax_cells
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", POTENTIAL)), 0)
    cfgs = workload(args.configs)
    calls, checks = 1, {}
    if args.leg == "relax":
        calls = args.relax_calls
        got = relax_cells(ctx, cfgs, 20, masses=MASS, list_cutoff=7.0, **FIRE)
        xw, ew = host_loop(ctx, cfgs, 20, full=True)
        box = np.diag(cfgs[0][1])
        dx = np.stack([q["x"] for q in got["final"]]) - xw
        checks = dict(fire20_max_position_difference_to_per_call_loop=float(np.abs(dx - box * np.round(dx / box)).max()),
                      fire20_max_energy_difference_to_per_call_loop=float(np.abs(np.array([q["energy"] for q in got["final"]]) - ew).max()),
                      fire20_max_displacement=float(np.abs(xw - np.stack([c[0] for c in cfgs])).max()))
        assert checks["fire20_max_position_difference_to_per_call_loop"] < 1e-10, checks
        assert checks["fire20_max_energy_difference_to_per_call_loop"] < 1e-8, checks

        def once(steps):
            r = relax_cells(ctx, cfgs, steps, masses=MASS, list_cutoff=7.0, **FIRE)
            assert r["steps_done"] == steps and all(q["status"] == "running" for q in r["final"])
            return float(sum(q["energy"] for q in r["final"]))
    else:
        def once(steps):
            return host_loop(ctx, cfgs, steps)
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
    ap.add_argument("--leg", choices=["relax", "percall"], default=None)
    ap.add_argument("--configs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--relax-calls", type=int, default=10, help="relax_cells runs per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in ("percall", "relax"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--configs", str(args.configs), "--steps", str(args.steps), "--windows", str(args.windows),
               "--relax-calls", str(args.relax_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    rate = {k: v["config_steps_per_second"] for k, v in legs.items()}
    result = dict(workload="%d jittered 16-atom bcc cells (2x2x2 cubic), %s, %d FIRE steps, ftol 0, dmax 0.001 A, no grade steps"
                           % (args.configs, POTENTIAL, args.steps),
                  relax_cells_config_steps_per_second=rate["relax"],
                  evaluate_cells_per_step_config_steps_per_second=rate["percall"],
                  ratio_to_evaluate_cells_per_step=rate["relax"] / rate["percall"], legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("legs", "workload")}))


if __name__ == "__main__":
    main()
