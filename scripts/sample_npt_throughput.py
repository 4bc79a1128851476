#!/usr/bin/env python
"""Configuration-steps per second of md.sample_cells_npt against what a user could do without it -- one md.evaluate_cells call per
step at the current cells with thermostat, integrator and barostat in numpy (the rules of mtp_sample_cell_step, vectorised over
equal cells) -- and against md.sample_cells on the same batch: the price of the per-atom virial, its reduction, the deform launch
and the wider monitor read.

Workload and rules: those of scripts/sample_throughput.py -- jittered 16-atom bcc cells, W_L16_nbh.almtp, Langevin at 30 K with
t_damp = 0.1 ps, dt = 0.025 fs (see there: the synthetic potential is stiff), grades every 10 steps with both thresholds out of
reach --, at 1 GPa with the compressibility of tungsten (0.52 A^3/eV), tau_p = 0.1 ps and all six components free.  Each leg runs
in a fresh child process under its own `timeout`, warms up with a shorter run of the same shapes, then times `--windows` windows
with a host clock around work that ends in a device synchronise; a leg that fails ends the run and nothing is tried again.  The
constant-pressure leg also checks itself at the timed size: 20 steps at 0 K, where neither thermostat nor barostat draws noise,
against the per-call loop (the numpy noise of that loop is not the device's, so the runs at 30 K cannot be compared).  The parent
writes the three rates (median window) to profiles/sample_npt_throughput.json.

    python scripts/sample_npt_throughput.py               # the three legs, writes the profile
    python scripts/sample_npt_throughput.py --leg npt     # one leg in this process, prints its JSON line
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

from scripts.sample_throughput import DT, GRADE_EVERY, MASS, OUT_OF_REACH, T, T_DAMP, workload  # noqa: E402

POTENTIAL = "W_L16_nbh.almtp"
PRESSURE, COMPRESSIBILITY, TAU_P, STRAIN_MAX = 1.0 / 160.21766, 0.52, 0.1, 0.01
VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def host_loop_npt(ctx, cfgs, vel, steps, temperature=T, seed=1, full=False):
    """what a user does without sample_cells_npt: evaluate_cells once per step at the current cells; fix langevin, the two half
    steps and the stochastic cell rescaling in numpy over all cells at once (they have the same size).  Returns the sum of the
    final energies, or with full=True (x, v, cells, energies)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, FTM2V, MVV2E, KB
    rng = np.random.default_rng(seed)
    x, v, h = np.stack([c[0] for c in cfgs]), np.stack(vel), np.stack([c[1] for c in cfgs])
    ncfg = len(cfgs)
    kT = KB * temperature
    dtf = 0.5 * DT * FTM2V
    g1 = -MASS / T_DAMP / FTM2V
    g2 = np.sqrt(MASS) * np.sqrt(24.0 * kT / T_DAMP / DT / MVV2E) / FTM2V
    c = COMPRESSIBILITY / (3.0 * TAU_P * np.linalg.det(h)) * DT
    s = np.sqrt(2.0 * kT * c)
    eye = np.eye(3)

    def forces(step):
        res = evaluate_cells(ctx, [(x[k], h[k], cfg[2]) for k, cfg in enumerate(cfgs)], list_cutoff=7.0, vflag=1,
                             grades=step % GRADE_EVERY == 0)
        f = np.stack([r["f"] for r in res])
        W = np.zeros((ncfg, 3, 3))
        for q, (a, b) in enumerate(VOIGT):
            W[:, a, b] = W[:, b, a] = [r["virial"][q] for r in res]
        return f + g1 * v + g2 * (rng.random(f.shape) - 0.5), W, res

    f, W, res = forces(0)
    for step in range(1, steps + 1):
        v += dtf / MASS * f
        Wt = W + MVV2E * MASS * np.einsum("kia,kib->kab", v, v)
        xi = np.sqrt(12.0) * (rng.random((ncfg, 3, 3)) - 0.5)
        N = np.where(eye > 0.0, xi, (np.triu(xi, 1) + np.triu(xi, 1).transpose(0, 2, 1)) * np.sqrt(0.5))
        A = c[:, None, None] * (Wt + (kT - PRESSURE * np.linalg.det(h))[:, None, None] * eye) + s[:, None, None] * N
        A = np.clip(A, -STRAIN_MAX, STRAIN_MAX)
        A2 = A @ A
        A3, A4 = A2 @ A, A2 @ A2
        E, Einv = eye + A + A2 / 2.0 + A3 / 6.0 + A4 / 24.0, eye - A + A2 / 2.0 - A3 / 6.0 + A4 / 24.0
        x, v, h = (x + DT * v) @ E, v @ Einv, h @ E
        f, W, res = forces(step)
        v += dtf / MASS * f
    e = np.array([r["energy"] for r in res])
    return (x, v, h, e) if full else float(e.sum())


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import maxwell_boltzmann, sample_cells, sample_cells_npt
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", POTENTIAL), selection=True), 0)
    cfgs = workload(args.configs)
    keys = list(range(args.configs))
    vel = maxwell_boltzmann([(p, t) for p, _, t in cfgs], np.array([MASS]), np.full(args.configs, T), 1, keys)
    calls, checks = args.sample_calls, {}
    kw = dict(t_damp=T_DAMP, seed=1, keys=keys, masses=MASS, velocities=vel, list_cutoff=7.0)
    npt = dict(kw, compressibility=COMPRESSIBILITY, tau_p=TAU_P, strain_max=STRAIN_MAX)
    if args.leg == "npt":
        got = sample_cells_npt(ctx, cfgs, 0.0, PRESSURE, 20, DT, grade_every=0, **npt)
        xw, vw, hw, ew = host_loop_npt(ctx, cfgs, vel, 20, temperature=0.0, full=True)
        dx = np.stack([q["x"] for q in got["final"]]) - xw
        dx -= np.round(dx @ np.linalg.inv(hw)) @ hw
        checks = dict(cold20_max_position_difference_to_per_call_loop=float(np.abs(dx).max()),
                      cold20_max_velocity_difference_to_per_call_loop=float(np.abs(np.stack([q["v"] for q in got["final"]]) - vw).max()),
                      cold20_max_cell_difference_to_per_call_loop=float(np.abs(np.stack([q["cell"] for q in got["final"]]) - hw).max()),
                      cold20_max_energy_difference_to_per_call_loop=float(np.abs(np.array([q["energy"] for q in got["final"]]) - ew).max()),
                      cold20_max_cell_change=float(np.abs(hw - np.stack([c[1] for c in cfgs])).max()),
                      cold20_capped=int(sum(q["capped"] for q in got["final"])))
        assert checks["cold20_max_position_difference_to_per_call_loop"] < 1e-10, checks
        assert checks["cold20_max_velocity_difference_to_per_call_loop"] < 1e-9, checks
        assert checks["cold20_max_cell_difference_to_per_call_loop"] < 1e-10, checks
        assert checks["cold20_max_energy_difference_to_per_call_loop"] < 1e-8, checks

        def once(steps):
            r = sample_cells_npt(ctx, cfgs, T, PRESSURE, steps, DT, grade_every=GRADE_EVERY, threshold_select=OUT_OF_REACH,
                                 threshold_break=OUT_OF_REACH, **npt)
            assert r["steps_done"] == steps and not r["records"] and all(q["status"] == "running" for q in r["final"])
            return float(sum(q["energy"] for q in r["final"]))
    elif args.leg == "fixed":
        def once(steps):
            r = sample_cells(ctx, cfgs, T, steps, DT, grade_every=GRADE_EVERY, threshold_select=OUT_OF_REACH,
                             threshold_break=OUT_OF_REACH, **kw)
            assert r["steps_done"] == steps and not r["records"]
            return float(sum(q["energy"] for q in r["final"]))
    else:
        calls = 1

        def once(steps):
            return host_loop_npt(ctx, cfgs, vel, steps)
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
    print(json.dumps(dict(leg=args.leg, configs=args.configs, steps=args.steps, atoms_per_config=16, potential=POTENTIAL,
                          calls_per_window=calls, seconds_per_call=windows,
                          config_steps_per_second=args.configs * args.steps / float(np.median(windows)), energy_sum=check, **checks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["percall", "npt", "fixed"], default=None)
    ap.add_argument("--configs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sample-calls", type=int, default=10, help="sample_cells_npt / sample_cells runs per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_npt_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in ("percall", "npt", "fixed"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--configs", str(args.configs), "--steps", str(args.steps), "--windows", str(args.windows),
               "--sample-calls", str(args.sample_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    rate = {k: v["config_steps_per_second"] for k, v in legs.items()}
    result = dict(workload="%d jittered 16-atom bcc cells (2x2x2 cubic), %s, %d steps of 0.025 fs at 30 K and 1 GPa, t_damp 0.1 ps, "
                           "compressibility 0.52 A^3/eV, tau_p 0.1 ps, six free components, grades every %d steps, thresholds out of "
                           "reach" % (args.configs, POTENTIAL, args.steps, GRADE_EVERY),
                  sample_cells_npt_config_steps_per_second=rate["npt"],
                  evaluate_cells_per_step_config_steps_per_second=rate["percall"],
                  sample_cells_config_steps_per_second=rate["fixed"],
                  ratio_to_evaluate_cells_per_step=rate["npt"] / rate["percall"],
                  ratio_to_sample_cells=rate["npt"] / rate["fixed"], legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("legs", "workload")}))


if __name__ == "__main__":
    main()
