#!/usr/bin/env python
"""Hessians per second of md.hessian_cells against what a user could do without it -- one md.evaluate_cells call per
displacement over explicitly displaced copies of all configurations, with the difference quotients and the symmetrisation (the
assembly of tests/_hess.py, vectorised over equal configurations) in numpy -- and the time md.modes then takes on the host
for the same Hessians, beside what the device eigen-solver takes for them: md.hessian_cells(modes=True), which solves inside the
pass, and md.modes_cells on the Hessians handed back (the copy to the device included).

Workload: jitters (0.05 A) of the 16-atom bcc cell (2 x 2 x 2 cubic) of scripts/relax_throughput.py, W_L16.mtp (level 16),
h = 0.01 A, all atoms: 6 x 16 + 1 = 97 force calls a pass.  Each leg runs in a fresh child process under its own `timeout`,
warms up with a run of the same shapes, then times `--windows` windows with a host clock around work that ends in a device
synchronise (the modes leg is host work alone, on Hessians it computes first); a leg that fails ends the run and nothing is
tried again.  The hessian leg also checks itself at the timed size against the per-call loop, within the force parity bound
over the step; the modes_device leg checks both its paths at the timed size against md.modes on the same Hessians, every
eigenvalue within 8 N eps |D|_F.  The parent writes the rates (median window) to profiles/hessian_throughput.json.

    python scripts/hessian_throughput.py                  # all legs, writes the profile
    python scripts/hessian_throughput.py --leg hessian    # one leg in this process, prints its JSON line
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

MASS, POTENTIAL, H_STEP, ATOMS = 183.84, "W_L16.mtp", 0.01, 16
CALLS = 6 * ATOMS + 1


def workload(ncfg, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    assert len(pos) == ATOMS
    rng = np.random.default_rng(seed)
    cell, types = np.diag(box), np.ones(len(pos), dtype=np.int32)
    return [(pos + rng.normal(0.0, 0.05, pos.shape), cell, types) for _ in range(ncfg)]


def host_loop(ctx, configs):
    """what a user does without hessian_cells: evaluate_cells once per displacement over every configuration, rows parked after
    +h and finished after -h, H <- 0.5 (H + H^T).  Returns (H [ncfg, 48, 48], f0 [ncfg, 16, 3])"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    cell, types = configs[0][1], configs[0][2]
    x0 = np.stack([c[0] for c in configs])
    B, n = x0.shape[:2]
    inv2h = 1.0 / (2.0 * H_STEP)
    forces = lambda x: np.stack([r["f"] for r in evaluate_cells(ctx, [(x[b], cell, types) for b in range(B)], list_cutoff=7.0, vflag=0)])
    f0 = forces(x0)
    H = np.zeros((B, 3 * n, 3 * n))
    for c in range(3 * n):
        x = x0.copy()
        x[:, c // 3, c % 3] = x0[:, c // 3, c % 3] + H_STEP
        plus = forces(x).reshape(B, -1)
        x[:, c // 3, c % 3] = x0[:, c // 3, c % 3] - H_STEP
        H[:, c] = (forces(x).reshape(B, -1) - plus) * inv2h
    return 0.5 * (H + H.transpose(0, 2, 1)), f0


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import hessian_cells, modes, modes_cells
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", POTENTIAL)), 0)
    configs = workload(args.configs)
    kw = dict(h=H_STEP, masses=MASS, list_cutoff=7.0)
    checks, more = {}, {}

    def device():
        res = hessian_cells(ctx, configs, **kw)
        assert all(r["status"] == "ok" for r in res)
        return res

    if args.leg == "hessian":
        got = device()
        want, f0 = host_loop(ctx, configs)
        Hd = np.stack([r["hessian"] for r in got])
        scale = max(1.0, float(np.abs(f0).max()) + H_STEP * float(np.abs(want).max()))
        bound = (1e-9 + 1e-10 * scale) / H_STEP
        checks = dict(max_difference_to_per_call_loop=float(np.abs(Hd - want).max()), bound=bound, largest_force_constant=float(np.abs(want).max()),
                      largest_asymmetry=max(r["asymmetry"] for r in got), largest_sum_rule=max(r["sum_rule"] for r in got))
        assert checks["max_difference_to_per_call_loop"] <= bound, checks
        once = lambda: float(sum(r["hessian"].trace() for r in device()))
    elif args.leg == "percall":
        once = lambda: float(np.trace(host_loop(ctx, configs)[0], axis1=1, axis2=2).sum())
    elif args.leg == "modes_device":
        masses = np.full(ATOMS, MASS)
        inside = lambda: hessian_cells(ctx, configs, modes=True, **kw)
        got = inside()
        handed = [r["hessian"] for r in got]
        after = lambda: modes_cells(handed, [masses] * len(handed))
        want = [modes(H, masses) for H in handed]
        worst = 0.0
        for found in (got, after()):
            for r, w in zip(found, want):
                assert r["solver"] == "device" and r.get("modes_status", r["status"]) == "ok", r["solver"]
                bound = 8.0 * len(w["eigenvalues"]) * 2.0 ** -53 * float(np.sqrt((w["eigenvalues"] ** 2).sum()))
                worst = max(worst, float(np.abs(r["eigenvalues"] - w["eigenvalues"]).max()) / bound)
                assert r["n_unstable"] == w["n_unstable"] and r["n_zero"] == w["n_zero"]
        assert worst <= 1.0, worst
        checks = dict(worst_eigenvalue_difference_over_bound=worst, unstable_modes=int(sum(r["n_unstable"] for r in got)),
                      zero_modes=int(sum(r["n_zero"] for r in got)))
        once = lambda: float(sum(r["frequencies"].sum() for r in inside()))
        alone = lambda: float(sum(r["frequencies"].sum() for r in after()))
        alone()
        windows = []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            alone()
            torch.cuda.synchronize()
            windows.append(time.perf_counter() - t0)
        more = dict(seconds_per_window_modes_cells=windows)
    else:
        got = device()
        masses = np.full(ATOMS, MASS)

        def once():
            out = [modes(r["hessian"], masses) for r in got]
            checks.update(unstable_modes=int(sum(q["n_unstable"] for q in out)), zero_modes=int(sum(q["n_zero"] for q in out)))
            return float(sum(q["frequencies"].sum() for q in out))
    once()                                                   # warm-up: every shape and every kernel of the timed window
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        check = once()                                       # (every device path ends in a copy back, which waits for the device)
        torch.cuda.synchronize()
        windows.append(time.perf_counter() - t0)
        assert np.isfinite(check), "the result of leg %s is not finite: nothing was measured" % args.leg
    t = float(np.median(windows))
    print(json.dumps(dict(leg=args.leg, configs=args.configs, atoms=ATOMS, force_calls_per_pass=CALLS, potential=POTENTIAL,
                          seconds_per_window=windows, hessians_per_second=args.configs / t,
                          configuration_evaluations_per_second=None if args.leg == "modes" else args.configs * CALLS / t,
                          checksum=check, **checks, **more)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["percall", "hessian", "modes", "modes_device"], default=None)
    ap.add_argument("--configs", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hessian_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in ("percall", "hessian", "modes", "modes_device"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--configs", str(args.configs), "--windows", str(args.windows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    t = {k: float(np.median(v["seconds_per_window"])) for k, v in legs.items()}
    result = dict(workload="%d jitters of the 16-atom bcc cell (2x2x2 cubic), %s, h = %g A, all atoms: %d force calls a pass"
                           % (args.configs, POTENTIAL, H_STEP, CALLS),
                  hessian_cells_hessians_per_second=legs["hessian"]["hessians_per_second"],
                  hessian_cells_configuration_evaluations_per_second=legs["hessian"]["configuration_evaluations_per_second"],
                  evaluate_cells_per_displacement_hessians_per_second=legs["percall"]["hessians_per_second"],
                  evaluate_cells_per_displacement_configuration_evaluations_per_second=legs["percall"]["configuration_evaluations_per_second"],
                  ratio_to_evaluate_cells_per_displacement=t["percall"] / t["hessian"],
                  modes_on_the_host_hessians_per_second=legs["modes"]["hessians_per_second"],
                  seconds_hessian_cells=t["hessian"], seconds_modes_on_the_host=t["modes"],
                  modes_share_of_hessian_plus_modes=t["modes"] / (t["hessian"] + t["modes"]),
                  seconds_hessian_cells_with_modes=t["modes_device"],
                  seconds_modes_on_the_device=max(t["modes_device"] - t["hessian"], 0.0),
                  seconds_modes_cells=float(np.median(legs["modes_device"]["seconds_per_window_modes_cells"])),
                  device_modes_share_of_hessian_plus_modes=max(t["modes_device"] - t["hessian"], 0.0) / t["modes_device"],
                  modes_host_over_modes_cells=t["modes"] / float(np.median(legs["modes_device"]["seconds_per_window_modes_cells"])),
                  legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("legs", "workload")}))


if __name__ == "__main__":
    main()
