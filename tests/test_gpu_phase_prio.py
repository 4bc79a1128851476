"""The fixed force kernel with its issue priority set by phase (csrc/mtp_wave_body.hpp, MTP_PHASE_PRIO), at every way
a launch's last round of atoms can be filled: the wavefronts of a CU then hold unequal atom counts, run out of step and
end at different times, which is what the priorities act on.  They decide which wavefront issues next, never what it
computes: W_L16.mtp in deterministic mode, forces, energy and virial of compute_device_rows bitwise those of the same
call under MTP_FIXED_SHAPE=0 (the generic kernel sets no priority), and one case against the oracle at the tolerances
of tests/test_gpu_parity.py.  (The same cases were written for a start offset per SIMD slot, which waited only in
wavefronts below the launch's maximum count; it was measured and is not in the sources, profiles/r13_ab_wave_phases.txt.
A library without either passes the same test.)

Row counts come from ctx.launch_info() of the context itself: with W wavefronts in the planned grid, W R + r rows for
R in {1, 2} and r in {0, 1, W/3 - 1, W/3, W/3 + 1, 2W/3, W - 1}, a range shorter than one round, and a single row.  A
16 x 16 x 18 bcc lattice (9,216 atoms, a = 3.04, jitter 0.1, list cutoff 7 A) is the smallest that reaches 2 W + W - 1
rows at W = 3,072.

Each case checks first, from a replica of the kernel's deal of rows to wavefronts (mtp_wave_kernel_body.hpp: an eighth of
the rows per XCD, wave-major numbering when the last round is partly filled), that its remainder class was produced:
how many wavefronts of workgroup 0 hold the launch's maximum count, and which SIMD slots of it (wavefront / 4) hold
wavefronts below it.  No class is unreachable at this size, so none is skipped."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W16 = os.path.join(ROOT, "potentials", "W_L16.mtp")
FORCE = "w16_force_3ps"
# remainder r (as a function of W) -> (name, wavefronts of workgroup 0 with the maximum count as a function of wpb,
# slots of workgroup 0 in which some wavefront is below the maximum)
CLASSES = {
    "0": (lambda W: 0, lambda wpb: wpb, set()),                       # whole rounds: every wavefront at the maximum
    "1": (lambda W: 1, lambda wpb: 1, {0, 1, 2}),                     # one wavefront of workgroup 0 holds the extra atom
    "W/3-1": (lambda W: W // 3 - 1, lambda wpb: wpb // 3, {1, 2}),
    "W/3": (lambda W: W // 3, lambda wpb: wpb // 3, {1, 2}),          # the headline launch's class: slot 0 holds the extra atoms
    "W/3+1": (lambda W: W // 3 + 1, lambda wpb: wpb // 3 + 1, {1, 2}),
    "2W/3": (lambda W: 2 * W // 3, lambda wpb: 2 * wpb // 3, {2}),
    "W-1": (lambda W: W - 1, lambda wpb: wpb, set()),                 # whole rounds in XCD 0; the last XCD is one row short
}


def deal(rows, grid, wpb):
    """atoms of every wavefront, [grid, wpb]: the kernel's map of rows to wavefronts (xcd_map is set from 512 rows up)"""
    n = np.zeros((grid, wpb), int)
    xcd_map = rows >= 8 * 64 and grid % 8 == 0
    for b in range(grid):
        for w in range(wpb):
            if xcd_map:
                chunk, xcd, nb8 = (rows + 7) >> 3, b & 7, grid >> 3
                step = nb8 * wpb
                beg = xcd * chunk + (w * nb8 + (b >> 3) if chunk % step else (b >> 3) * wpb + w)
                end = min(rows, (xcd + 1) * chunk)
            else:
                step = grid * wpb
                beg = w * grid + b if rows % step else b * wpb + w
                end = rows
            n[b, w] = (end - beg + step - 1) // step if beg < end else 0
    return n


def row_range_plan(rows, info, cus=256):
    """(grid, wpb) of a row range under the list's plan (csrc/mtp_plan.cpp, plan_row_range), for the full-width ranges"""
    wpb, grid = info["waves_per_block"], info["grid_blocks"]
    assert rows >= cus * wpb and grid == cus     # the short ranges take narrower workgroups: not replicated here
    g = min(grid, (rows + wpb - 1) // wpb)
    return (g + 7) // 8 * 8, wpb


@pytest.fixture(scope="module")
def system():
    import torch
    pos, box = mtpgen.bcc_lattice(16, 16, 18, a=3.04, jitter=0.1, seed=47)
    s = periodic_system(pos, box, None, 7.0)
    assert s.nlocal == 9216
    dev = torch.device("cuda", 0)
    ctx = capi.Context(capi.Potential(W16), 0)
    ctx.set_deterministic(True)
    il, fi, ne = (torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(dev) for v in (s.ilist, s.first, s.neigh))
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    x = torch.from_numpy(np.ascontiguousarray(s.x)).to(dev)
    ty = torch.from_numpy(np.ascontiguousarray(s.types, np.int32)).to(dev)
    info = ctx.launch_info()
    W = info["grid_blocks"] * info["waves_per_block"]
    assert W % 3 == 0 and 3 * W - 1 <= s.nlocal < 2 * 16 * 16 * 19, (W, s.nlocal)   # the smallest lattice that reaches 3 W - 1
    return dict(s=s, ctx=ctx, x=x, ty=ty, dev=dev, info=info, W=W, keep=(il, fi, ne))


def _run(sysd, rows, monkeypatch, fixed):
    import torch
    s, ctx, dev = sysd["s"], sysd["ctx"], sysd["dev"]
    f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    ev = torch.zeros(8, dtype=torch.float64, device=dev)
    with monkeypatch.context() as m:
        if fixed:
            m.delenv("MTP_FIXED_SHAPE", raising=False)
        else:
            m.setenv("MTP_FIXED_SHAPE", "0")
        ctx.compute_device_rows(0, rows, True, sysd["x"], sysd["ty"], f, eflag=1, vflag=1, ev_t=ev)
        name = ctx.last_shape()
    ctx.synchronize()
    torch.cuda.synchronize()
    return dict(f=f.cpu().numpy(), ev=ev.cpu().numpy()), name


def _bitwise(sysd, rows, monkeypatch):
    a, na = _run(sysd, rows, monkeypatch, True)
    b, nb = _run(sysd, rows, monkeypatch, False)
    assert na == FORCE and nb == "", (na, nb)     # mtp_context_last_shape: the fixed kernel ran, then the generic one
    assert np.abs(a["f"]).max() > 1e-3 and a["ev"][0] != 0.0 and np.abs(a["ev"][1:7]).min() > 0.0
    for k in a:
        assert np.array_equal(a[k], b[k]), (rows, k, float(np.abs(a[k] - b[k]).max()))
    return a


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_remainder_class_is_bitwise_the_generic_kernel(system, monkeypatch, cls, R):
    W, info = system["W"], system["info"]
    r_of, at_max_of, below = CLASSES[cls]
    rows = W * R + r_of(W)
    grid, wpb = row_range_plan(rows, info)
    assert grid * wpb == W
    n = deal(rows, grid, wpb)
    assert n.sum() == rows
    n_max = int(n.max())
    assert n_max == (R if r_of(W) == 0 else R + 1)
    # the class, as the plan produced it: workgroup 0's wavefronts with the maximum count, and its slots with wavefronts below it
    assert int((n[0] == n_max).sum()) == at_max_of(wpb), (cls, n[0])
    slots = {w // 4 for w in range(wpb) if 0 < n[0, w] < n_max}
    assert {s for s in slots if s > 0} == {s for s in below if s > 0}, (cls, n[0], slots)
    if not below:
        assert (n[0] == n_max).all()
    print("%s R %d: %d rows, %d x %d wavefronts, counts of workgroup 0 %s, %d wavefronts of the launch below the maximum" % (
        cls, R, rows, grid, wpb, n[0].tolist(), int((n < n_max).sum())))
    _bitwise(system, rows, monkeypatch)


@pytest.mark.parametrize("what", ["half a round", "one row"])
def test_short_ranges_are_bitwise_the_generic_kernel(system, monkeypatch, what):
    rows = system["W"] // 2 if what == "half a round" else 1
    _bitwise(system, rows, monkeypatch)


def test_headline_class_against_the_oracle(system, monkeypatch):
    from oracle.pyoracle import Oracle
    s, W = system["s"], system["W"]
    rows = W + W // 3
    got = _bitwise(system, rows, monkeypatch)
    want = Oracle(W16).compute(s.x, s.types, s.ilist[:rows], s.first[:rows + 1], s.neigh[:s.first[rows]])

    def close(g, w, what, atol=1e-9, rtol=1e-10):   # the tolerances of tests/test_gpu_parity.py
        scale = max(1.0, float(np.abs(w).max()))
        err = float(np.abs(np.asarray(g) - np.asarray(w)).max())
        print("%s: max abs err %.3e (scale %.3e)" % (what, err, scale))
        assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)

    close(got["f"], want["f"], "forces")
    assert abs(got["ev"][0] - want["energy"]) / rows <= 1e-10 * max(1.0, abs(want["energy"]) / rows)
    close(got["ev"][1:7], want["virial"], "virial", atol=1e-8)
