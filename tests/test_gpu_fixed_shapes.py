"""The fixed-shape force kernels on the GPU (csrc/mtp_kernels_fixed.hip): a launch whose table structure and LDS plan
equal a compiled shape runs that shape's kernel, and computes bit for bit what the generic kernel computes
(MTP_FIXED_SHAPE=0, read at every launch) -- the fixed fields are integers, no sum is reordered.  Deterministic mode
throughout: there the force sums do not depend on the arrival order of the atomics either."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
FORCE, GRADE = "w16_force_3ps", "w16_grade_3ps"


@pytest.fixture(scope="module")
def system():
    """4,394 atoms (more than 256 x 16: the twelve-wavefront plan), BCC with a = 3.04 and a jitter of 0.1: the fourth
    shell (24 atoms at 5.04) straddles the 5.0 cutoff, so atoms have 26 .. 40 neighbours inside it -- one and two tiles"""
    pos, box = mtpgen.bcc_lattice(13, 13, 13, a=3.04, jitter=0.1, seed=31)
    s = periodic_system(pos, box, None, 7.0)
    assert s.nlocal >= 256 * 16
    return s


def _in_cutoff_counts(s, rc):
    rows = np.repeat(np.arange(s.nlocal), np.diff(s.first))
    d = s.x[s.neigh] - s.x[s.ilist[rows]]
    return np.bincount(rows, weights=((d * d).sum(1) <= rc * rc).astype(np.float64), minlength=s.nlocal).astype(int)


def _context(path, s, selection=False):
    pot = capi.Potential(path, selection=selection)
    ctx = capi.Context(pot, 0)
    ctx.set_deterministic(True)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    return pot, ctx


def _both(ctx, s, monkeypatch, **kw):
    """the same call through the fixed-shape kernel and through the generic one, with what the query reported"""
    with monkeypatch.context() as m:
        m.delenv("MTP_FIXED_SHAPE", raising=False)
        a = ctx.compute(s.x, s.types, **kw)
        na = ctx.last_shape()
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        b = ctx.compute(s.x, s.types, **kw)
        nb = ctx.last_shape()
    return a, na, b, nb


def _bitwise(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max()))


def test_system_has_one_tile_and_multi_tile_atoms(system):
    pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
    cnt = _in_cutoff_counts(system, pot.info.max_cutoff)
    assert (cnt <= 32).sum() >= 100 and (cnt > 32).sum() >= 100, (cnt.min(), cnt.max())


@pytest.mark.parametrize("eflag", [0, 1, 3])
@pytest.mark.parametrize("vflag", [0, 1, 5])
def test_force_shape_is_bitwise_the_generic_kernel(system, monkeypatch, eflag, vflag):
    _, ctx = _context(os.path.join(POT, "W_L16.mtp"), system)
    a, na, b, nb = _both(ctx, system, monkeypatch, eflag=eflag, vflag=vflag)
    assert na == FORCE and nb == ""
    assert np.abs(a["f"]).max() > 1e-3
    _bitwise(a, b, "eflag %d vflag %d" % (eflag, vflag))


def test_grade_shape_is_bitwise_the_generic_kernel(system, monkeypatch):
    _, ctx = _context(os.path.join(POT, "W_L16_nbh.almtp"), system, selection=True)
    a, na, b, nb = _both(ctx, system, monkeypatch, eflag=3, vflag=5, grade=True)
    assert na == GRADE and nb == ""
    assert a["max_grade"] > 0.0 and a["max_grade"] == b["max_grade"]
    _bitwise(a, b, "grade call")
    # a force call of the same context takes the force shape
    a, na, b, nb = _both(ctx, system, monkeypatch, eflag=1, vflag=1)
    assert na == FORCE and nb == ""
    _bitwise(a, b, "force call of the selection potential")


def test_row_ranges_take_the_fixed_kernel_and_agree_bitwise(system, monkeypatch):
    import torch
    s = system
    dev = torch.device("cuda", 0)
    pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
    ctx = capi.Context(pot, 0)
    ctx.set_deterministic(True)
    il, fi, ne = (torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(dev) for v in (s.ilist, s.first, s.neigh))
    ctx.set_neighbors_device(il, fi, ne, s.nall, int(np.diff(s.first).max()))
    x = torch.from_numpy(s.x).to(dev)
    ty = torch.from_numpy(np.ascontiguousarray(s.types, np.int32)).to(dev)
    cut = 1531   # an uneven split: [0, 1531) and [1531, nlocal)

    def run(split):
        f = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
        ev = torch.zeros(8, dtype=torch.float64, device=dev)
        ea = torch.zeros(s.nall, dtype=torch.float64, device=dev)
        va = torch.zeros((s.nall, 6), dtype=torch.float64, device=dev)
        names = []
        kw = dict(eflag=3, vflag=5, eatom_t=ea, vatom_t=va, ev_t=ev)
        if split:
            ctx.compute_device_rows(0, cut, False, x, ty, f, **kw)
            names.append(ctx.last_shape())
            ctx.compute_device_rows(cut, s.nlocal - cut, True, x, ty, f, **kw)
            names.append(ctx.last_shape())
        else:
            ctx.compute_device(x, ty, f, **kw)
            names.append(ctx.last_shape())
        ctx.synchronize()
        torch.cuda.synchronize()
        return dict(f=f.cpu().numpy(), ev=ev.cpu().numpy(), eatom=ea.cpu().numpy(), vatom=va.cpu().numpy()), names

    with monkeypatch.context() as m:
        m.delenv("MTP_FIXED_SHAPE", raising=False)
        a, na = run(True)
        whole, nw = run(False)
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        b, nb = run(True)
    assert na == [FORCE, FORCE] and nw == [FORCE] and nb == ["", ""]
    _bitwise(a, b, "row ranges")
    # per-atom outputs and the fixed-point forces do not depend on the split either
    for k in ("f", "eatom", "vatom"):
        assert np.array_equal(a[k], whole[k]), k


def test_refit_of_the_table_runs_the_fixed_kernel_and_agrees_with_the_oracle(system, tmp_pot_dir, monkeypatch):
    """the potential of tests/test_fixed_shapes_cpu.py: the level-16 table with other coefficients, cutoffs and scaling"""
    from oracle.pyoracle import Oracle
    monkeypatch.delenv("MTP_FIXED_SHAPE", raising=False)
    s = system
    p = mtpgen.random_potential(mtpgen.build_table(16), 1, 20251, 1.7, 5.6, 8, 0.37)
    path = str(tmp_pot_dir / "refit16_gpu.mtp")
    mtpgen.write_mtp(p, path)
    pot = capi.Potential(path)
    ctx = capi.Context(pot, 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    got = ctx.compute(s.x, s.types, eflag=3, vflag=4)
    assert ctx.last_shape() == FORCE
    want = Oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)

    def close(g, w, what, atol=1e-9, rtol=1e-10):   # the tolerances of tests/test_gpu_parity.py
        scale = max(1.0, float(np.abs(w).max()))
        err = float(np.abs(np.asarray(g) - np.asarray(w)).max())
        assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)

    close(got["f"], want["f"], "forces")
    n = len(s.ilist)
    assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n)
    close(got["eatom"], want["eatom"], "eatom", atol=1e-10)
    close(got["virial"], want["virial"], "virial", atol=1e-8)
    close(got["vatom"], want["vatom"], "vatom")
