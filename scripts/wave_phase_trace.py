#!/usr/bin/env python3
"""Diagnostic: how the wavefronts of a CU run against each other in the force kernel, from the per-wavefront phase trace
of the stamped build (make -C lammps_mtp_kokkos_amd/csrc stamps; csrc/mtp_device.hpp, MTP_TRACE_*).

    MTP_LIB=lammps_mtp_kokkos_amd/ab/libmtp_mi355x_stamps.so python scripts/wave_phase_trace.py collect OUT.npz
        the headline launch (bench.py's lattice: 32^3 BCC cells, W_L16.mtp) on the GPU; the trace of the last launch
    python scripts/wave_phase_trace.py reduce OUT.npz [OUT2.npz ...]
        no GPU: the summary that goes into profiles/

One workgroup per XCD is traced (one workgroup per CU in the headline plan, so a traced workgroup is a traced CU).  Two
quantities, each at the start of the launch and over its last third, each beside what INDEPENDENT, evenly spread
wavefronts would give -- every wavefront at a uniformly random point of its own cycle, with the share of its time it
really spent in the phases in question during the window (Poisson-binomial over the wavefronts):
  per SIMD   share of time in which 0 / 1 / 2 / 3 of its wavefronts are in a burst phase
             (tile tables, basic moments, coefficient blocks, forces)
  per CU     distribution of how many of its wavefronts are inside the product passes at once
             (products forward with the leaf sweep, energy, products backward)
It also prints which wavefronts share a SIMD (hardware-id register), the duration of an atom by SIMD slot, and how far
the later wavefronts of a SIMD have fallen behind the first one at a few atoms of the launch.
Clocks are s_memtime ticks; the ticks of a microsecond are taken from the kernel time of HIP events against the longest
traced wavefront's life.  The stamped build is slower than the shipped one (its stamps cost registers, and a stamp
drains the LDS and scalar counters): the trace shows how the wavefronts stand to each other, not the shipped kernel's
time."""
import os
import sys

import numpy as np

HDR, ATOMS, WGS, WPB_MAX = 8, 24, 8, 12          # mtp_device.hpp
WAVE_WORDS = HDR + 10 * ATOMS
NAMES = ["loop head", "compaction", "tile tables", "basic moments", "products fwd", "energy", "products bwd", "forces",
         "totals", "coef blocks"]
ORDER = [0, 1, 2, 3, 4, 5, 6, 9, 7, 8]            # the stamps of an atom in program order
BURST = (2, 3, 9, 7)
PRODUCT = (4, 5, 6)


def collect(out):
    import ctypes as C
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from lammps_mtp_kokkos_amd import capi, mtpgen
    from lammps_mtp_kokkos_amd.domain import decompose

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pos, box = mtpgen.bcc_lattice(32, 32, 32, a=3.165, jitter=0.05, seed=777)
    plan = decompose(pos, box, None, 1, 0, 7.0)
    ctx = capi.Context(capi.Potential(os.path.join(root, "potentials", "W_L16.mtp")), 0)
    dev = torch.device("cuda:0")
    il, fi, ne = (torch.from_numpy(a).to(dev) for a in (plan.ilist, plan.first, plan.neigh))
    ctx.set_neighbors_device(il, fi, ne, plan.nall, int(np.diff(plan.first).max()))
    x = torch.from_numpy(plan.x0).to(dev)
    ty = torch.from_numpy(plan.types).to(dev)
    f = torch.zeros((plan.nall, 3), dtype=torch.float64, device=dev)
    ev = torch.zeros(8, dtype=torch.float64, device=dev)
    L = capi.lib()
    words = WGS * WPB_MAX * WAVE_WORDS
    buf = (C.c_ulonglong * words)()
    sums = (C.c_ulonglong * 16)()
    ctx.set_timing(True)
    for _ in range(12):
        ctx.compute_device(x, ty, f, eflag=1, vflag=1, ev_t=ev)
        ctx.synchronize()
        L.mtp_debug_read_stamps(ctx.h, sums)
    ms = ctx.last_kernel_ms()
    rc = L.mtp_debug_read_trace(ctx.h, buf, words)
    assert rc == 0, rc
    info = ctx.launch_info()
    np.savez_compressed(out, trace=np.array(buf, dtype=np.uint64), sums=np.array(sums, dtype=np.uint64), kernel_ms=ms,
                        wpb=info["waves_per_block"], grid=info["grid_blocks"], shape=ctx.last_shape(),
                        flags=capi.build_flags() if hasattr(capi, "build_flags") else "", nlocal=plan.nlocal)
    print("collected %s: kernel %.4f ms, shape %r, launch %s" % (out, ms, ctx.last_shape(), info))


def poisson_binomial(p):
    d = np.array([1.0])
    for q in p:
        d = np.convolve(d, [1.0 - q, q])
    return d


def count_shares(intervals, t0, t1, nmax):
    """share of [t0, t1) in which k = 0 .. nmax of the interval lists are inside one of their intervals"""
    ev = []
    for iv in intervals:
        for a, b in iv:
            a, b = max(a, t0), min(b, t1)
            if b > a:
                ev.append((a, 1))
                ev.append((b, -1))
    ev.sort()
    out = np.zeros(nmax + 1)
    t, k = t0, 0
    for when, d in ev:
        out[k] += when - t
        t, k = when, k + d
    out[k] += t1 - t
    return out / max(1, t1 - t0)


def inside_share(iv, t0, t1):
    return sum(max(0, min(b, t1) - max(a, t0)) for a, b in iv) / max(1, t1 - t0)


def waves_of(trace, wpb):
    """[(workgroup, wave, record)] of the traced wavefronts that ran"""
    t = trace.reshape(WGS, WPB_MAX, WAVE_WORDS).astype(np.int64)
    out = []
    for g in range(WGS):
        for w in range(wpb):
            r = t[g, w]
            n = int(r[2])
            if r[3] == 0 or n == 0:
                continue
            n = min(n, ATOMS)
            st = r[HDR:HDR + 10 * n].reshape(n, 10)
            beg = np.concatenate([[r[5]], st[:-1, 8]])           # an atom begins where the one before ended
            phases = {k: [] for k in range(10)}
            for a in range(n):
                prev = beg[a]
                for k in ORDER:
                    if st[a, k] > prev:                           # (a stamp the atom did not pass stays at an older clock)
                        phases[k].append((prev, st[a, k]))
                        prev = st[a, k]
            out.append(dict(wg=g, wave=w, hw=int(r[0]), xcc=int(r[1]), n=n, entry=int(r[3]), prologue=int(r[4]),
                            start=int(r[5]), end=int(st[-1, 8]), atom=st[:, 8] - beg, phases=phases))
    return out


def fmt(v):
    return "  ".join("%5.1f" % (100 * x) for x in v)


def reduce(path):
    z = np.load(path, allow_pickle=False)
    wpb = int(z["wpb"])
    ws = waves_of(z["trace"], wpb)
    ms = float(z["kernel_ms"])
    print("=" * 100)
    print("%s: shape %s, kernel %.4f ms (HIP events, stamped build), %d workgroups x %d wavefronts, %d traced wavefronts" % (
        os.path.basename(path), str(z["shape"]), ms, int(z["grid"]), wpb, len(ws)))
    if not ws:
        print("no trace")
        return
    life = max(w["end"] - w["entry"] for w in ws)
    tick_us = life / (1e3 * ms)
    print("longest traced wavefront: %d ticks entry -> last atom, i.e. about %.1f ticks per microsecond of the kernel time" % (life, tick_us))
    # ---- which wavefronts share a SIMD ------------------------------------------------------------------------------
    print("hardware ids (HW_ID: wave slot [3:0], SIMD [5:4], CU [11:8], SE [15:13]; XCC_ID [3:0]):")
    rr = True
    for g in sorted({w["wg"] for w in ws}):
        mine = [w for w in ws if w["wg"] == g]
        cu = {(w["xcc"] & 15, (w["hw"] >> 13) & 7, (w["hw"] >> 8) & 15) for w in mine}
        simd = [(w["hw"] >> 4) & 3 for w in mine]
        rr = rr and all(simd[k] == simd[k % 4] for k in range(len(simd))) and len(set(simd[:4])) == min(4, len(simd))
        print("  workgroup %d  (xcc, se, cu) %s  SIMD of wavefronts 0..%d: %s  slots: %s" % (
            g, sorted(cu), len(mine) - 1, " ".join(str(s) for s in simd), " ".join(str(w["hw"] & 15) for w in mine)))
    print("  wavefront k shares its SIMD with k + 4 and k + 8 in every traced workgroup: %s" % ("yes" if rr else "NO"))
    # ---- durations --------------------------------------------------------------------------------------------------
    atom = np.concatenate([w["atom"] for w in ws])
    print("atom duration per wavefront: mean %.1f ticks (%.2f us), median %.1f, min %d, max %d; atoms per wavefront %s" % (
        atom.mean(), atom.mean() / tick_us, np.median(atom), atom.min(), atom.max(), sorted({w["n"] for w in ws})))
    tot = {k: sum(b - a for w in ws for a, b in w["phases"][k]) for k in range(10)}
    for k in ORDER:
        print("    %-14s %5.1f %%  %7.1f ticks / atom" % (NAMES[k], 100 * tot[k] / max(1, sum(tot.values())), tot[k] / len(atom)))
    print("  burst phases %.1f %%, product passes %.1f %% of an atom" % (
        100 * sum(tot[k] for k in BURST) / sum(tot.values()), 100 * sum(tot[k] for k in PRODUCT) / sum(tot.values())))
    wait = {}
    for w in ws:
        wait.setdefault((w["wave"] // 4, w["n"]), []).append(w["start"] - w["prologue"])
    print("prologue end -> first atom, by (wave / 4, atoms): " + "; ".join(
        "%s: %.0f ticks = %.3f atoms" % (k, np.mean(v), np.mean(v) / atom.mean()) for k, v in sorted(wait.items())))
    # ---- do the wavefronts of a SIMD keep step? ---------------------------------------------------------------------
    med = float(np.median(atom))
    for s in range(3):
        d = np.concatenate([w["atom"][1:] for w in ws if w["wave"] // 4 == s] or [np.zeros(1)])
        print("  wavefronts %d..%d (SIMD slot %d): atom duration mean %.0f, median %.0f ticks; life entry -> end mean %.0f ticks" % (
            4 * s, 4 * s + 3, s, d.mean(), np.median(d), np.mean([w["end"] - w["entry"] for w in ws if w["wave"] // 4 == s] or [0])))
    for a in (5, 10, 15, 20):
        lag = {1: [], 2: []}
        for g in sorted({w["wg"] for w in ws}):
            mine = {w["wave"]: w for w in ws if w["wg"] == g and w["n"] > a}
            for k, w in mine.items():
                if k >= 4 and k % 4 in mine and k // 4 in lag:
                    lag[k // 4].append((w["phases"][0][a][0] - mine[k % 4]["phases"][0][a][0]) / med)
        print("  start of atom %2d behind the SIMD's first wavefront, in median atoms: slot 1 %+.2f, slot 2 %+.2f" % (
            a, np.mean(lag[1] or [0]), np.mean(lag[2] or [0])))
    # ---- the two quantities -----------------------------------------------------------------------------------------
    for label in ("start of the launch (first third)", "last third"):
        simd_meas, simd_ind, cu_meas, cu_ind = [], [], [], []
        for g in sorted({w["wg"] for w in ws}):
            mine = [w for w in ws if w["wg"] == g]
            t_a, t_b = max(w["start"] for w in mine), min(w["end"] for w in mine)
            third = (t_b - t_a) // 3
            t0, t1 = (t_a, t_a + third) if label.startswith("start") else (t_b - third, t_b)
            burst = {w["wave"]: sorted(sum((w["phases"][k] for k in BURST), [])) for w in mine}
            prod = {w["wave"]: sorted(sum((w["phases"][k] for k in PRODUCT), [])) for w in mine}
            for s in range(4):
                on = [w["wave"] for w in mine if ((w["hw"] >> 4) & 3) == s]
                if len(on) != 3:
                    continue
                simd_meas.append(count_shares([burst[k] for k in on], t0, t1, 3))
                simd_ind.append(poisson_binomial([inside_share(burst[k], t0, t1) for k in on]))
            cu_meas.append(count_shares(list(prod.values()), t0, t1, wpb))
            cu_ind.append(poisson_binomial([inside_share(v, t0, t1) for v in prod.values()]))
        print("-- %s" % label)
        if simd_meas:
            m, i = np.mean(simd_meas, 0), np.mean(simd_ind, 0)
            print("  per SIMD (%d SIMDs), %% of time with 0 / 1 / 2 / 3 wavefronts in a burst phase" % len(simd_meas))
            print("      measured      %s" % fmt(m))
            print("      independent   %s" % fmt(i))
            print("      all three at once: %.2f x independent; none: %.2f x independent" % (m[3] / max(i[3], 1e-12), m[0] / max(i[0], 1e-12)))
        m, i = np.mean(cu_meas, 0), np.mean(cu_ind, 0)
        k = np.arange(len(m))
        print("  per CU (%d CUs), %% of time with k = 0 .. %d wavefronts inside the product passes" % (len(cu_meas), wpb))
        print("      measured      %s" % fmt(m))
        print("      independent   %s" % fmt(i))
        sd = lambda d: float(np.sqrt((d * k * k).sum() - (d * k).sum() ** 2))   # noqa: E731
        print("      mean %.2f (independent %.2f), standard deviation %.2f (independent %.2f)" % (
            (m * k).sum(), (i * k).sum(), sd(m), sd(i)))


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "collect":
        collect(sys.argv[2])
        reduce(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == "reduce":
        for p in sys.argv[2:]:
            reduce(p)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
