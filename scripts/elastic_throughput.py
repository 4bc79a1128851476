#!/usr/bin/env python
"""Sets of elastic constants per second of md.elastic_cells against what a user could do without it -- md.evaluate_cells on the
configurations as given and on twelve explicitly strained copies (pos @ D, cell @ D) of all of them, with the stress, the
difference quotients, Wallace's correction and the symmetrisation in numpy -- clamped and with relaxed ions, where the loop goes
on with one evaluate_cells call per displaced coordinate and takes the ionic term from md.relax_ions (numpy's Cholesky); and the
time md.relax_ions alone takes on the host for the same Hessians, so that the share of mtp_elastic_relax can be read off.

Workload: jitters (0.02 A) of the 16-atom bcc cell (2 x 2 x 2 cubic) at the lattice parameter W_L16.mtp (level 16) relaxes the bcc
cell to, 3.576 A, each taken to a local minimum by md.relax_cells before anything is timed (untimed, in every leg) -- the
synthetic W_L16 has unstable zone-boundary modes in this cell, so every unrelaxed jitter would end the ionic term at a negative
pivot and mtp_elastic_relax would be timed on its way out --, strain step 0.005, displacement 0.01 A: 13 force calls a pass
clamped, 13 + 97 with relaxed ions.  Each leg runs in a fresh child process under its own `timeout`, warms up with a run of the same shapes, then times `--windows` windows with a host clock
around work that ends in a device synchronise; a leg that fails ends the run and nothing is tried again.  The two device legs
also check themselves at the timed size against their loops, within the parity bounds over the steps.  The parent writes the
rates (median window) to profiles/elastic_throughput.json.

    python scripts/elastic_throughput.py                  # all legs, writes the profile
    python scripts/elastic_throughput.py --leg elastic    # one leg in this process, prints its JSON line
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

POTENTIAL, H_STRAIN, H_ATOMS, ATOMS = "W_L16.mtp", 0.005, 0.01, 16
LATTICE, JITTER, RELAX_STEPS, RELAX_FTOL = 3.576, 0.02, 3000, 1e-4
CALLS = {"percall": 13, "elastic": 13, "percall_relaxed": 13 + 6 * ATOMS + 1, "relaxed": 13 + 6 * ATOMS + 1, "ionic_host": 0}
LEGS = ("percall", "elastic", "percall_relaxed", "relaxed", "ionic_host")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def workload(ctx, ncfg, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    from lammps_mtp_kokkos_amd.md import relax_cells
    pos, box = mtpgen.bcc_lattice(2, 2, 2, a=LATTICE, jitter=0.0)
    assert len(pos) == ATOMS
    rng = np.random.default_rng(seed)
    cell, types = np.diag(box), np.ones(len(pos), dtype=np.int32)
    start = [(pos + rng.normal(0.0, JITTER, pos.shape), cell, types) for _ in range(ncfg)]
    final = relax_cells(ctx, start, RELAX_STEPS, ftol=RELAX_FTOL, dmax=0.01, dt_max=2e-3, grade_every=0, list_cutoff=7.0)["final"]
    return [(r["x"], cell, types) for r in final], sum(r["status"] == "converged" for r in final)


def strain(w, s):
    D = np.eye(3)
    a, b = PAIRS[w]
    if a == b:
        D[a, a] += s
    else:
        D[a, b] = D[b, a] = 0.5 * s
    return D


def host_loop(ctx, configs, ionic):
    """what a user does without elastic_cells.  Returns dict(birch, elastic [ncfg, 6, 6], coupling [ncfg, 6, 48], stress [ncfg, 6],
    f0, and with `ionic` hessian [ncfg, 48, 48], elastic_relaxed [ncfg, 6, 6])"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, relax_ions, stress_correction
    cell, types = configs[0][1], configs[0][2]
    x0 = np.stack([c[0] for c in configs])
    nb, n = x0.shape[:2]

    def call(x, h, vflag=1):
        res = evaluate_cells(ctx, [(x[b], h, types) for b in range(nb)], list_cutoff=7.0, vflag=vflag)
        return np.stack([r["f"] for r in res]).reshape(nb, -1), np.stack([r["virial"] for r in res])

    f0, w0 = call(x0, cell)
    vol = float(np.linalg.det(cell))
    stress = -w0 / vol
    B, L = np.zeros((nb, 6, 6)), np.zeros((nb, 6, 3 * n))
    for w in range(6):
        for sign in (1.0, -1.0):
            D = strain(w, sign * H_STRAIN)
            f, vir = call(x0 @ D, cell @ D)
            B[:, :, w] += sign * (-vir / float(np.linalg.det(cell @ D))) / (2.0 * H_STRAIN)
            L[:, w] += sign * f / (2.0 * H_STRAIN)
    M = B - np.stack([stress_correction(s) for s in stress])
    out = dict(birch=B, elastic=0.5 * (M + M.transpose(0, 2, 1)), coupling=L, stress=stress, f0=f0, wmax=float(np.abs(w0).max()))
    if ionic:
        H = np.zeros((nb, 3 * n, 3 * n))
        for c in range(3 * n):
            x = x0.copy()
            x[:, c // 3, c % 3] = x0[:, c // 3, c % 3] + H_ATOMS
            plus = call(x, cell, 0)[0]
            x[:, c // 3, c % 3] = x0[:, c // 3, c % 3] - H_ATOMS
            H[:, c] = (call(x, cell, 0)[0] - plus) / (2.0 * H_ATOMS)
        out["hessian"] = 0.5 * (H + H.transpose(0, 2, 1))
        rel = [relax_ions(B[b], out["elastic"][b], L[b], out["hessian"][b], vol) for b in range(nb)]
        out["elastic_relaxed"] = np.stack([r["elastic_relaxed"] for r in rel])
    return out


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import elastic_cells, relax_ions
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", POTENTIAL)), 0)
    configs, converged = workload(ctx, args.configs)
    ionic = args.leg in ("relaxed", "percall_relaxed", "ionic_host")
    checks = dict(relaxed_to_a_minimum=converged)

    def device():
        res = elastic_cells(ctx, configs, h=H_STRAIN, relax_ions=ionic, h_atoms=H_ATOMS, list_cutoff=7.0)
        assert all(r["status"] != "failed" for r in res)
        checks["unstable"] = sum(r["status"] == "unstable" for r in res)   # (a jitter with a negative mode: NaN, left out of the sums)
        return res

    key = "elastic_relaxed" if ionic else "elastic"
    if args.leg in ("elastic", "relaxed"):
        got, want = device(), host_loop(ctx, configs, ionic)
        vol = got[0]["volume"]
        bound_b = (1e-8 + 1e-10 * max(1.0, want["wmax"] * (1.0 + 3.0 * H_STRAIN))) / (vol * H_STRAIN)
        err_b = float(np.abs(np.stack([r["birch"] for r in got]) - want["birch"]).max())
        checks.update(max_difference_of_birch_to_per_call_loop=err_b, bound=bound_b, largest_elastic_constant=float(np.abs(want["elastic"]).max()),
                      largest_asymmetry=max(r["asymmetry"] for r in got), largest_sum_rule=max(r["sum_rule"] for r in got),
                      largest_fmax=max(r["fmax"] for r in got))
        assert err_b <= bound_b, checks
        if ionic:
            # the two Hessians differ within the force parity bound over the displacement; through the ionic term that is a
            # relative matter: reported, not bounded here (tests/test_elastic_gpu.py bounds the solve on equal inputs)
            checks["max_difference_of_elastic_relaxed_to_per_call_loop"] = float(
                np.nanmax(np.abs(np.stack([r["elastic_relaxed"] for r in got]) - want["elastic_relaxed"])))
            checks["largest_ionic_term"] = float(np.nanmax(np.abs(want["elastic_relaxed"] - want["elastic"])))
        once = lambda: float(np.nansum([r[key].trace() for r in device()]))
    elif args.leg in ("percall", "percall_relaxed"):
        once = lambda: float(np.nansum(np.trace(host_loop(ctx, configs, ionic)[key], axis1=1, axis2=2)))
    else:
        got = device()
        once = lambda: float(np.nansum([relax_ions(r["birch"], r["elastic"], r["coupling"], r["hessian"], r["volume"])["elastic_relaxed"].trace()
                                        for r in got]))
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
    calls = CALLS[args.leg]
    print(json.dumps(dict(leg=args.leg, configs=args.configs, atoms=ATOMS, force_calls_per_pass=calls, potential=POTENTIAL,
                          seconds_per_window=windows, sets_per_second=args.configs / t,
                          configuration_evaluations_per_second=args.configs * calls / t if calls else None, checksum=check, **checks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS, default=None)
    ap.add_argument("--configs", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in LEGS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--configs", str(args.configs), "--windows", str(args.windows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    t = {k: float(np.median(v["seconds_per_window"])) for k, v in legs.items()}
    result = dict(workload="%d jitters (%g A) of the 16-atom bcc cell (2x2x2 cubic, a = %g A), relaxed by relax_cells (%d steps, ftol %g), "
                           "%s, strain step %g, displacement %g A: 13 force calls a pass clamped, %d with relaxed ions"
                           % (args.configs, JITTER, LATTICE, RELAX_STEPS, RELAX_FTOL, POTENTIAL, H_STRAIN, H_ATOMS, CALLS["relaxed"]),
                  relaxed_to_a_minimum=legs["relaxed"]["relaxed_to_a_minimum"],
                  unstable_configurations=legs["relaxed"]["unstable"],
                  elastic_cells_sets_per_second=legs["elastic"]["sets_per_second"],
                  evaluate_cells_per_strain_sets_per_second=legs["percall"]["sets_per_second"],
                  ratio_clamped=t["percall"] / t["elastic"],
                  elastic_cells_relaxed_sets_per_second=legs["relaxed"]["sets_per_second"],
                  evaluate_cells_per_strain_and_displacement_sets_per_second=legs["percall_relaxed"]["sets_per_second"],
                  ratio_relaxed=t["percall_relaxed"] / t["relaxed"],
                  relax_ions_on_the_host_sets_per_second=legs["ionic_host"]["sets_per_second"],
                  seconds_elastic_cells=t["elastic"], seconds_elastic_cells_relaxed=t["relaxed"],
                  seconds_relax_ions_on_the_host=t["ionic_host"], legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("legs", "workload")}))


if __name__ == "__main__":
    main()
