#!/usr/bin/env python
"""Configuration-steps per second of md.sample_cells against the two things a user could do without it: one
md.evaluate_cells call per step with the integrator in numpy, and one md.DeviceNVE per cell, run in turn.

Workload: jittered 16-atom bcc cells (2 x 2 x 2 cubic) as in scripts/batch_throughput.py, W_L16_nbh.almtp (level 16,
neighbourhood grades), Langevin at 30 K with t_damp = 0.1 ps, grades every 10 steps with both thresholds out of reach (the
grade steps and the capture decisions run; nothing is captured or frozen, so every leg does the same number of steps).  The
synthetic potential is stiff and unbounded -- the jittered cells carry forces of 30 eV/A, which would carry a W atom 2 A in
50 fs -- so dt = 0.025 fs: the timed 200 steps are 5 fs, the atoms move about 0.02 A, the state stays finite (every leg
asserts it) and the work per step is that of real cells.  The time of a step does not depend on dt.  The DeviceNVE leg is NVE without grades -- that class has neither -- over the
first `--nve-cells` cells.  Each leg runs in a fresh child process under its own `timeout`, warms up with a shorter run of the
same shapes, then times `--windows` windows with a host clock around work that ends in a device synchronise; a leg that
fails ends the run.  The sample leg also checks itself at the timed size: its energies at step 0 against evaluate_cells, and
20 NVE steps against the evaluate_cells-per-step loop (the numpy noise of that loop is not the device's, so the Langevin runs
themselves cannot be compared).  The parent writes the three rates (median window) to profiles/sample_throughput.json.

    python scripts/sample_throughput.py                  # all legs, writes the profile
    python scripts/sample_throughput.py --leg sample     # one leg in this process, prints its JSON line
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

MASS, T, DT, T_DAMP, GRADE_EVERY, OUT_OF_REACH = 183.84, 30.0, 2.5e-5, 0.1, 10, 1e300


def workload(ncfg, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    rng = np.random.default_rng(seed)
    return [(pos + rng.normal(0.0, 0.05, pos.shape), np.diag(box), np.ones(len(pos), dtype=np.int32)) for _ in range(ncfg)]


def host_loop(ctx, cfgs, vel, steps, seed=1, thermostat=True, full=False):
    """what a user does without sample_cells: evaluate_cells once per step, fix langevin + fix nve in numpy (thermostat=False:
    fix nve alone).  Returns the sum of the final energies, or with full=True (x, v, energies)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, FTM2V, MVV2E, KB
    rng = np.random.default_rng(seed)
    x = np.stack([c[0] for c in cfgs])
    v = np.stack(vel)
    dtf = 0.5 * DT * FTM2V
    g1 = -MASS / T_DAMP / FTM2V
    g2 = np.sqrt(MASS) * np.sqrt(24.0 * KB * T / T_DAMP / DT / MVV2E) / FTM2V

    def forces(step):
        res = evaluate_cells(ctx, [(x[k], c[1], c[2]) for k, c in enumerate(cfgs)], list_cutoff=7.0, vflag=0,
                             grades=step % GRADE_EVERY == 0)
        f = np.stack([r["f"] for r in res])
        return (f + g1 * v + g2 * (rng.random(f.shape) - 0.5) if thermostat else f), res

    f, res = forces(0)
    for step in range(1, steps + 1):
        v += dtf / MASS * f
        x += DT * v
        f, res = forces(step)
        v += dtf / MASS * f
    if full:
        return x, v, np.array([r["energy"] for r in res])
    return float(sum(r["energy"] for r in res))


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import DeviceNVE, evaluate_cells, maxwell_boltzmann, sample_cells
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    pot = capi.Potential(os.path.join(ROOT, "potentials", "W_L16_nbh.almtp"), selection=True)
    ctx = capi.Context(pot, 0)
    cfgs = workload(args.configs)
    keys = list(range(args.configs))
    vel = maxwell_boltzmann([(p, t) for p, _, t in cfgs], np.array([MASS]), np.full(args.configs, T), 1, keys)
    calls, checks = 1, {}
    if args.leg == "sample":
        ncfg, calls = args.configs, args.sample_calls
        # the two paths compute the same thing at the size that is timed: energies at step 0, and 20 NVE steps
        kw = dict(seed=1, keys=keys, masses=MASS, velocities=vel, list_cutoff=7.0)
        e0 = np.array([q["energy"] for q in sample_cells(ctx, cfgs, T, 0, DT, t_damp=T_DAMP, grade_every=0, **kw)["final"]])
        want0 = np.array([r["energy"] for r in evaluate_cells(ctx, cfgs, list_cutoff=7.0, vflag=0)])
        got = sample_cells(ctx, cfgs, T, 20, DT, t_damp=None, grade_every=0, **kw)
        xw, vw, ew = host_loop(ctx, cfgs, vel, 20, thermostat=False, full=True)
        box = np.diag(cfgs[0][1])
        dx = np.stack([q["x"] for q in got["final"]]) - xw
        checks = dict(max_energy_difference_to_evaluate_cells_at_step_0=float(np.abs(e0 - want0).max()),
                      nve20_max_position_difference_to_per_call_loop=float(np.abs(dx - box * np.round(dx / box)).max()),
                      nve20_max_velocity_difference_to_per_call_loop=float(np.abs(np.stack([q["v"] for q in got["final"]]) - vw).max()),
                      nve20_max_energy_difference_to_per_call_loop=float(np.abs(np.array([q["energy"] for q in got["final"]]) - ew).max()),
                      nve20_max_displacement=float(np.abs(xw - np.stack([c[0] for c in cfgs])).max()))
        assert checks["max_energy_difference_to_evaluate_cells_at_step_0"] < 1e-8, checks
        assert checks["nve20_max_position_difference_to_per_call_loop"] < 1e-10, checks
        assert checks["nve20_max_velocity_difference_to_per_call_loop"] < 1e-9, checks
        assert checks["nve20_max_energy_difference_to_per_call_loop"] < 1e-8, checks

        def once(steps):
            r = sample_cells(ctx, cfgs, T, steps, DT, t_damp=T_DAMP, seed=1, keys=keys, masses=MASS, grade_every=GRADE_EVERY,
                             threshold_select=OUT_OF_REACH, threshold_break=OUT_OF_REACH, velocities=vel, list_cutoff=7.0)
            assert r["steps_done"] == steps and not r["records"]
            return float(sum(q["energy"] for q in r["final"]))
    elif args.leg == "percall":
        ncfg = args.configs

        def once(steps):
            return host_loop(ctx, cfgs, vel, steps)
    else:
        ncfg = min(args.nve_cells, args.configs)

        def once(steps):
            e = 0.0
            for (p, c, _), v0 in zip(cfgs[:ncfg], vel):
                md = DeviceNVE(ctx, p.copy(), c, rc=pot.info.max_cutoff, mass=MASS, list_cutoff=7.0)
                md.v.copy_(torch.from_numpy(v0))
                for _ in range(steps):
                    md.step(DT)
                e += md.total_energy()
            return e
    once(2 * GRADE_EVERY)                                    # warm-up: every shape and every kernel of the timed window
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            check = once(args.steps)                         # (every path ends in a copy back, which waits for the device)
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / calls)
        assert np.isfinite(check), "the state of leg %s went non-finite: nothing was measured" % args.leg
    print(json.dumps(dict(leg=args.leg, configs=ncfg, steps=args.steps, atoms_per_config=16, potential="W_L16_nbh.almtp",
                          calls_per_window=calls, seconds_per_call=windows, config_steps_per_second=ncfg * args.steps / float(np.median(windows)),
                          energy_sum=check, **checks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["sample", "percall", "nve"], default=None)
    ap.add_argument("--configs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sample-calls", type=int, default=20, help="sample_cells runs per timed window")
    ap.add_argument("--nve-cells", type=int, default=32)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in ("percall", "nve", "sample"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--configs", str(args.configs), "--steps", str(args.steps), "--nve-cells", str(args.nve_cells),
               "--windows", str(args.windows), "--sample-calls", str(args.sample_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    rate = {k: v["config_steps_per_second"] for k, v in legs.items()}
    result = dict(workload="%d jittered 16-atom bcc cells (2x2x2 cubic), W_L16_nbh.almtp, %d steps of 0.025 fs at 30 K, t_damp 0.1 ps, "
                           "grades every %d steps, thresholds out of reach; DeviceNVE leg: NVE, no grades, %d cells in turn"
                           % (args.configs, args.steps, GRADE_EVERY, legs["nve"]["configs"]),
                  sample_cells_config_steps_per_second=rate["sample"],
                  evaluate_cells_per_step_config_steps_per_second=rate["percall"],
                  device_nve_per_cell_config_steps_per_second=rate["nve"],
                  ratio_to_evaluate_cells_per_step=rate["sample"] / rate["percall"],
                  ratio_to_device_nve_per_cell=rate["sample"] / rate["nve"], legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("legs", "workload")}))


if __name__ == "__main__":
    main()
