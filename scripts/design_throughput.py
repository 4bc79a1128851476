#!/usr/bin/env python
"""Design matrix of the linear refit: one md.design_cells call against what a user could do before it existed -- one
md.evaluate_cells call per column, each on a context of a potential file with a unit coefficient vector (species_coeffs
= e_t, moment_coeffs = 0 or species_coeffs = 0, moment_coeffs = e_a): by linearity its energies, forces and virials are
that column.

Workload: 512 jittered 16-atom bcc cells (2 x 2 x 2 cubic), W_L16.mtp, Sp + S = 117 columns.  One child process under its
own `timeout` makes the unit-coefficient files and contexts (outside the timed windows; every potential of both legs is
loaded with the same settings), warms both legs up and times them in alternation, reporting each stage on stderr as it
ends, `--windows` windows each, with a host clock around calls that end in a device synchronise.  One design_cells call
is a few milliseconds, too short a window for a host clock, so a window of the new leg is `--reps` calls back to back and
its time the window's divided by `--reps`; a window of the loop leg is one pass over all the columns.  The
parent writes the two times (median window), their ratio and the largest difference between the two matrices to
profiles/design_throughput.json.

    python scripts/design_throughput.py                  # writes the profile
    python scripts/design_throughput.py --child          # the measurement in this process, prints its JSON line
"""
import argparse
import json
import os
import re
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


def unit_file(src_text, path, Sp, S, col):
    """the potential with a unit coefficient vector: a text rewrite of the two coefficient lines"""
    sp = ["1.0" if col == t else "0.0" for t in range(Sp)]
    mo = ["1.0" if col == Sp + a else "0.0" for a in range(S)]
    text = re.sub(r"^species_coeffs\s*=\s*\{[^}]*\}", "species_coeffs = {%s}" % ", ".join(sp), src_text, flags=re.M)
    text = re.sub(r"^moment_coeffs\s*=\s*\{[^}]*\}", "moment_coeffs = {%s}" % ", ".join(mo), text, flags=re.M)
    open(path, "w").write(text)
    return path


def child(args):
    import torch
    from lammps_mtp_kokkos_amd import capi
    from lammps_mtp_kokkos_amd.md import design_cells, evaluate_cells
    assert torch.cuda.is_available(), "this measurement needs the MI355X"

    def stage(what):                                         # progress on stderr: a run that its time limit ends says where
        print("[design_throughput %7.1f s] %s" % (time.perf_counter() - t_start, what), file=sys.stderr, flush=True)

    t_start = time.perf_counter()
    # 118 loads, all with the same settings: the LDS-bank search of the product rows at the effort the test suites use (two
    # rounds; the shipped default takes up to ~10 s per load).  The loads are outside the timed windows.
    os.environ.setdefault("MTP_BANK_ROUNDS", "2")
    os.environ.setdefault("MTP_BANK_SCALE", "1")
    src = os.path.join(ROOT, "potentials", "W_L16.mtp")
    pot = capi.Potential(src)
    Sp, S = pot.info.species_count, pot.info.alpha_scalar_count
    ctx = capi.Context(pot, 0)
    cfgs = workload(args.configs)
    ntot = sum(len(p) for p, _, _ in cfgs)
    stage("potential and context of the design leg loaded")
    with tempfile.TemporaryDirectory() as tmp:               # files and contexts: outside the timed windows
        text = open(src).read()
        units = [capi.Context(capi.Potential(unit_file(text, os.path.join(tmp, "u%d.mtp" % c), Sp, S, c)), 0) for c in range(Sp + S)]

    stage("%d unit-coefficient contexts loaded" % len(units))

    def new_leg():
        d = design_cells(ctx, cfgs, list_cutoff=7.0, virial=True)    # (ends in a device synchronise)
        return d

    reps = dict(design=args.reps, loop=1)                    # calls per timed window

    def loop_leg():
        return [evaluate_cells(u, cfgs, list_cutoff=7.0, vflag=1) for u in units]

    d = new_leg()                                            # warm-up: every shape of the timed windows
    stage("design leg warmed up")
    cols = loop_leg()
    stage("loop leg warmed up")
    times = dict(design=[], loop=[])
    for _ in range(args.windows):                            # the two legs in alternation
        for name, leg in (("design", new_leg), ("loop", loop_leg)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                out = leg()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps[name])
            stage("%s leg: %.5f s per pass, window of %d" % (name, times[name][-1], reps[name]))
            if name == "design":
                d = out
            else:
                cols = out
    # the two matrices, entry by entry
    e, f, v = d["energy"].cpu().numpy(), d["force"].cpu().numpy(), d["virial"].cpu().numpy()
    diff = dict(energy=0.0, force=0.0, virial=0.0)
    scale = dict(energy=0.0, force=0.0, virial=0.0)
    first = np.concatenate([[0], np.cumsum([len(p) for p, _, _ in cfgs])])
    for c, res in enumerate(cols):
        ec = np.array([r["energy"] for r in res])
        fc = np.concatenate([r["f"].reshape(-1) for r in res])
        vc = np.array([r["virial"] for r in res])
        for k, (a, b) in dict(energy=(e[:, c], ec), force=(f[:, c], fc), virial=(v[:, :, c], vc)).items():
            diff[k] = max(diff[k], float(np.abs(a - b).max()))
            scale[k] = max(scale[k], float(np.abs(b).max()))
    assert first[-1] == ntot
    print(json.dumps(dict(configs=args.configs, atoms=ntot, columns=Sp + S, potential="W_L16.mtp", windows=args.windows,
                          design_calls_per_window=args.reps,
                          design_seconds=times["design"], loop_seconds=times["loop"],
                          design_median=float(np.median(times["design"])), loop_median=float(np.median(times["loop"])),
                          max_abs_difference=diff, max_abs_entry=scale,
                          matrix_bytes=int(8 * (Sp + S) * (args.configs * 7 + 3 * ntot)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--configs", type=int, default=512)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=25, help="design_cells calls in one timed window of the new leg")
    ap.add_argument("--timeout", type=int, default=480, help="seconds for the measuring process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "design_throughput.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--configs", str(args.configs), "--windows", str(args.windows),
           "--reps", str(args.reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:                                    # nothing more is started on the GPU after a failure
        sys.exit("the measurement failed with status %d" % p.returncode)
    m = json.loads(p.stdout.strip().splitlines()[-1])
    result = dict(workload="%d jittered 16-atom bcc cells (2x2x2 cubic), W_L16.mtp, %d columns, energy + force + virial rows"
                  % (args.configs, m["columns"]),
                  design_cells_seconds=m["design_median"], unit_coefficient_loop_seconds=m["loop_median"],
                  ratio=m["loop_median"] / m["design_median"], max_abs_difference=m["max_abs_difference"],
                  max_abs_entry=m["max_abs_entry"], measurement=m)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("design_cells_seconds", "unit_coefficient_loop_seconds", "ratio", "max_abs_difference")}))


if __name__ == "__main__":
    main()
