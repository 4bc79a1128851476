#!/usr/bin/env python
"""Installing into a live context against the reload route it replaces: one Context.install_coeffs and one
Context.install_selection call against writing the potential file (capi.write_all_coeffs, or Context.save where there is a
selection state), mtp_potential_load and mtp_context_create -- the latter at the SHIPPED effort of the LDS-bank search
(MTP_BANK_ROUNDS / MTP_BANK_SCALE unset), which is what every rank pays per load today.

Potentials: W_L16_nbh.almtp (coefficients and selection) and WRe_L20.mtp (coefficients only: it carries no selection
state).  Per potential one child process under its own `timeout`; the legs run in alternation, a warm-up each, `--windows`
windows, with a host clock around calls that end in a stream synchronise.  The parent writes the median times to
profiles/install_throughput.json; no ratio is claimed in advance, the file states what was measured.

    python scripts/install_throughput.py                  # writes the profile
    python scripts/install_throughput.py --child NAME     # the measurement of one potential in this process, prints its JSON line
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
POTENTIALS = (("W_L16_nbh.almtp", True), ("WRe_L20.mtp", False))


def child(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    os.environ.pop("MTP_BANK_ROUNDS", None)                  # the shipped search effort for every load of the reload leg
    os.environ.pop("MTP_BANK_SCALE", None)
    name, selection = next(p for p in POTENTIALS if p[0] == args.child)
    src = os.path.join(ROOT, "potentials", name)
    t_start = time.perf_counter()

    def stage(what):                                         # progress on stderr: a run that its time limit ends says where
        print("[install_throughput %7.1f s] %s" % (time.perf_counter() - t_start, what), file=sys.stderr, flush=True)

    pot = capi.Potential(src, selection=selection)
    ctx = capi.Context(pot, 0)
    stage("source potential loaded")
    rng = np.random.default_rng(7)
    t = pot.tables()
    blocks = [t[k].reshape(-1) * (1.0 + 0.01 * rng.standard_normal(t[k].size)) for k in ("radial_coeffs", "species_coeffs", "moment_coeffs")]
    if selection:
        C = int(pot.info.coeff_count)
        S = 2.0 * np.eye(C) + 0.05 * rng.uniform(-1, 1, (C, C))
        W = np.linalg.inv(S)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "state" + os.path.splitext(name)[1])

        def install_coeffs():
            ctx.install_coeffs(*blocks)                      # (returns after its stream has drained)

        def install_selection():
            ctx.install_selection(S, W)

        def reload_route():
            if selection:
                ctx.save(path)
            else:
                capi.write_all_coeffs(src, path, blocks[2], blocks[1], blocks[0])
            c = capi.Context(capi.Potential(path, selection=selection), 0)
            c.synchronize()
            return c

        legs = [("install_coeffs", install_coeffs), ("reload", reload_route)]
        if selection:
            legs.insert(1, ("install_selection", install_selection))
        for leg_name, leg in legs:                           # a warm-up each
            leg()
            stage("%s leg warmed up" % leg_name)
        times = {leg_name: [] for leg_name, _ in legs}
        for _ in range(args.windows):                        # the legs in alternation
            for leg_name, leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                torch.cuda.synchronize()
                times[leg_name].append(time.perf_counter() - t0)
                stage("%s: %.6f s" % (leg_name, times[leg_name][-1]))
        same = None
        if not selection:                                    # the two routes end in the same device tables
            a, b = ctx.coeff_tables_device(), reload_route().coeff_tables_device()
            same = all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in a)
    print(json.dumps(dict(potential=name, coefficients=int(pot.info.coeff_count), windows=args.windows, seconds=times,
                          median={k: float(np.median(v)) for k, v in times.items()}, tables_equal=same,
                          bank_search="shipped (MTP_BANK_ROUNDS and MTP_BANK_SCALE unset)")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for each measuring process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "install_throughput.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    for name, _ in POTENTIALS:                               # every GPU step under its own time limit, chained: a failure ends the run
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", name,
               "--windows", str(args.windows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                # nothing more is started on the GPU after a failure
            sys.exit("the measurement of %s failed with status %d" % (name, p.returncode))
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    out = dict(what="one install into a live context against write + mtp_potential_load + mtp_context_create, seconds (median "
                    "of %d windows, legs in alternation, a warm-up each)" % args.windows, potentials=results)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps([dict(potential=r["potential"], **r["median"]) for r in results]))


if __name__ == "__main__":
    main()
