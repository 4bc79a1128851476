#!/usr/bin/env python
"""Band-steps per second of md.neb_cells against what a user could do without it: one md.evaluate_cells call per step over
the images of all bands with the band arithmetic (minimum image, improved tangent, spring and climbing image, FIRE per band:
the rules of mtp_neb_step, vectorised over equal bands) in numpy.

Workload: bands of 5 images between two jitters of the 16-atom bcc cell (2 x 2 x 2 cubic) of scripts/relax_throughput.py,
W_L16.mtp (level 16), spring 5 eV/A^2, the climbing image from step 10, no grade steps, FIRE at the defaults of neb_cells
except ftol = 0 (nothing converges, so both legs make the same steps) and dmax = 0.001 A -- that small for the reason given in
scripts/relax_throughput.py: the synthetic potentials have holes at short distance, and timings of a non-finite state say
nothing.  Every leg asserts that its state stays finite, the neb leg that no band failed.  Each leg runs in a fresh child
process under its own `timeout`, warms up with a shorter run of the same shapes, then times `--windows` windows with a host
clock around work that ends in a device synchronise; a leg that fails ends the run and nothing is tried again.  The neb leg
also checks itself at the timed size: 20 steps against the per-call loop.  The parent writes the two rates (median window) to
profiles/neb_throughput.json.

    python scripts/neb_throughput.py                  # both legs, writes the profile
    python scripts/neb_throughput.py --leg neb        # one leg in this process, prints its JSON line
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

MASS, POTENTIAL, IMAGES, SPRING, CLIMB = 183.84, "W_L16.mtp", 5, 5.0, 10
FIRE = dict(ftol=0.0, dt=1e-3, dt_max=1e-2, dmax=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)


def workload(nbands, seed=2024):
    from lammps_mtp_kokkos_amd import mtpgen
    from lammps_mtp_kokkos_amd.md import interpolate_band
    pos, box = mtpgen.bcc_lattice(2, 2, 2)
    rng = np.random.default_rng(seed)
    cell, types = np.diag(box), np.ones(len(pos), dtype=np.int32)
    return [(interpolate_band(pos + rng.normal(0.0, 0.05, pos.shape), pos + rng.normal(0.0, 0.05, pos.shape), cell, IMAGES), cell, types)
            for _ in range(nbands)]


def host_loop(ctx, bands, steps, full=False):
    """what a user does without neb_cells: evaluate_cells once per step over every image, the bands in numpy, all at once (they
    have the same shape; nothing converges with ftol = 0).  Returns the sum of the final energies, or with full=True (x, energies)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, FTM2V
    p = FIRE
    cell, types = bands[0][1], bands[0][2]
    inv = np.linalg.inv(cell)
    mic = lambda d: d - np.rint(d @ inv) @ cell
    x = np.stack([np.stack(b[0]) for b in bands])                                     # [bands, images, atoms, 3]
    B, M = x.shape[:2]
    v = np.zeros_like(x[:, 1:-1])
    dt, alpha, npos = np.full(B, p["dt"]), np.full(B, p["alpha_start"]), np.zeros(B, dtype=np.int64)
    col = lambda a: a[:, None, None, None]
    for step in range(steps + 1):
        res = evaluate_cells(ctx, [(x[b, i], cell, types) for b in range(B) for i in range(M)], list_cutoff=7.0, vflag=0)
        E = np.array([r["energy"] for r in res]).reshape(B, M)
        if step == steps:                                    # (the last step only decides)
            break
        f = np.stack([r["f"] for r in res]).reshape(x.shape)[:, 1:-1]
        dp, dm = mic(x[:, 2:] - x[:, 1:-1]), mic(x[:, 1:-1] - x[:, :-2])
        em, e0, ep = E[:, :-2], E[:, 1:-1], E[:, 2:]
        up, dn = np.abs(ep - e0), np.abs(em - e0)
        big, small = np.maximum(up, dn), np.minimum(up, dn)
        rising, falling = (ep > e0) & (e0 > em), (ep < e0) & (e0 < em)
        wp = np.where(rising, 1.0, np.where(falling, 0.0, np.where(ep > em, big, small)))
        wm = np.where(rising, 0.0, np.where(falling, 1.0, np.where(ep > em, small, big)))
        tau = wp[:, :, None, None] * dp + wm[:, :, None, None] * dm
        norm = np.sqrt((tau * tau).sum((2, 3)))
        fpar = (f * tau).sum((2, 3)) / norm
        g = SPRING * (np.sqrt((dp * dp).sum((2, 3))) - np.sqrt((dm * dm).sum((2, 3)))) - fpar
        if step >= CLIMB:
            top = np.argmax(e0, axis=1)
            g[np.arange(B), top] = -2.0 * fpar[np.arange(B), top]
        f = f + (g / norm)[:, :, None, None] * tau
        P, vv, ff = (f * v).sum((1, 2, 3)), (v * v).sum((1, 2, 3)), (f * f).sum((1, 2, 3))
        down = P > 0.0
        npos = np.where(down, npos + 1, 0)
        grow = down & (npos > p["n_min"])
        a = np.where(down, 1.0 - alpha, 0.0)
        b = np.where(down, alpha * np.sqrt(vv / ff), 0.0)
        dt = np.where(grow, np.minimum(dt * p["f_inc"], p["dt_max"]), np.where(~down & (vv > 0.0), dt * p["f_dec"], dt))
        alpha = np.where(grow, alpha * p["f_alpha"], np.where(down, alpha, p["alpha_start"]))
        vm = col(a) * v + col(b) * f
        vmax = np.abs(vm).max((1, 2, 3))
        dtv = np.where(dt * vmax > p["dmax"], p["dmax"] / np.maximum(vmax, 1e-300), dt)
        x[:, 1:-1] += col(dtv) * vm
        v = vm + col(dtv * FTM2V / MASS) * f
    return (x, E) if full else float(E.sum())


def run_leg(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import neb_cells
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    ctx = capi.Context(capi.Potential(os.path.join(ROOT, "potentials", POTENTIAL)), 0)
    bands = workload(args.bands)
    kw = dict(masses=MASS, list_cutoff=7.0, spring=SPRING, climb_after=CLIMB, **FIRE)
    calls, checks = 1, {}
    if args.leg == "neb":
        calls = args.neb_calls
        got = neb_cells(ctx, bands, 20, **kw)
        xw, ew = host_loop(ctx, bands, 20, full=True)
        box = np.diag(bands[0][1])
        dx = np.stack([np.stack(r["images"]) for r in got["bands"]]) - xw
        checks = dict(neb20_max_position_difference_to_per_call_loop=float(np.abs(dx - box * np.round(dx / box)).max()),
                      neb20_max_energy_difference_to_per_call_loop=float(np.abs(np.stack([r["energies"] for r in got["bands"]]) - ew).max()),
                      neb20_max_displacement=float(np.abs(xw - np.stack([np.stack(b[0]) for b in bands])).max()))
        assert checks["neb20_max_position_difference_to_per_call_loop"] < 1e-10, checks
        assert checks["neb20_max_energy_difference_to_per_call_loop"] < 1e-8, checks

        def once(steps):
            r = neb_cells(ctx, bands, steps, **kw)
            assert r["steps_done"] == steps and all(q["status"] == "running" for q in r["bands"])
            return float(sum(q["energies"].sum() for q in r["bands"]))
    else:
        def once(steps):
            return host_loop(ctx, bands, steps)
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
    print(json.dumps(dict(leg=args.leg, bands=args.bands, images_per_band=IMAGES, steps=args.steps, atoms_per_image=16,
                          potential=POTENTIAL, calls_per_window=calls, seconds_per_call=windows,
                          band_steps_per_second=args.bands * args.steps / float(np.median(windows)), energy_sum=check, **checks)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["neb", "percall"], default=None)
    ap.add_argument("--bands", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--neb-calls", type=int, default=10, help="neb_cells runs per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds, per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neb_throughput.json"))
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = {}
    for leg in ("percall", "neb"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--bands", str(args.bands), "--steps", str(args.steps), "--windows", str(args.windows),
               "--neb-calls", str(args.neb_calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("leg %s failed with status %d" % (leg, p.returncode))
        legs[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    rate = {k: v["band_steps_per_second"] for k, v in legs.items()}
    result = dict(workload="%d bands of %d images of the jittered 16-atom bcc cell (2x2x2 cubic), %s, %d NEB steps, spring %g, climbing "
                           "image from step %d, ftol 0, dmax 0.001 A, no grade steps" % (args.bands, IMAGES, POTENTIAL, args.steps, SPRING, CLIMB),
                  neb_cells_band_steps_per_second=rate["neb"],
                  evaluate_cells_per_step_band_steps_per_second=rate["percall"],
                  ratio_to_evaluate_cells_per_step=rate["neb"] / rate["percall"], legs=legs)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k not in ("legs", "workload")}))


if __name__ == "__main__":
    main()
