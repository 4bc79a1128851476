"""The fixed-shape force kernel with the slot tables as constants and f' from registers (csrc/mtp_wave_body.hpp:
slot_rows_ct, fp_regs_ct) at the neighbour-count edges of its tile build and of the exchange between the halves.

The 4,394-atom lattice of tests/test_gpu_fixed_shapes.py (the fixed shape is planned from 4,096 rows up), with the
list rows of 33 chosen atoms changed so that exactly 0, 1, 2, 3, 31, 32, 33, 34, 63, 64 and 65 of their entries lie
inside the potential's cutoff: the edges of the dummy padding to a multiple of NG = 2, of the half exchange
(v_permlane32_swap after each tile build that parks), and of the second and third tile.  A count below the atom's own is
reached by cutting in-cutoff entries out of its row.  No atom of this lattice has 63 neighbours inside 5.0 A (or 5.6 A
for the refit), so the counts above an atom's own are reached by added neighbours: ghost atoms placed inside the cutoff
of the chosen atom and listed in its row only (out-of-cutoff entries leave the row in exchange, the longest row and
with it the launch plan stay what they were).  The kernels and the oracle get the same positions and the same lists.

Deterministic mode: the fixed kernel is bitwise the generic one (MTP_FIXED_SHAPE=0), and both agree with the oracle
within the tolerances of tests/test_gpu_parity.py.  The same with a refit of the level-16 table."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
FORCE = "w16_force_3ps"
COUNTS = (0, 1, 2, 3, 31, 32, 33, 34, 63, 64, 65)
PER_COUNT = 3


@pytest.fixture(scope="module")
def lattice():
    pos, box = mtpgen.bcc_lattice(13, 13, 13, a=3.04, jitter=0.1, seed=31)
    s = periodic_system(pos, box, None, 7.0)
    assert s.nlocal >= 256 * 16
    return s


def _edge_system(s, rc, seed):
    """(x, types, first, neigh, {atom: count}) with the rows of the chosen atoms cut or filled to the counts of COUNTS"""
    rng = np.random.default_rng(seed)
    longest = int(np.diff(s.first).max())
    chosen = rng.choice(s.nlocal, size=len(COUNTS) * PER_COUNT, replace=False)
    want = {int(a): COUNTS[k % len(COUNTS)] for k, a in enumerate(chosen)}
    rows, extra = [], []
    for i in range(s.nlocal):
        row = s.neigh[s.first[i]:s.first[i + 1]]
        if i in want:
            k = want[i]
            d = s.x[row] - s.x[i]
            inside = (d * d).sum(1) <= rc * rc
            assert abs(np.sqrt((d * d).sum(1)) - rc).min() > 1e-6   # no entry whose side of the cutoff is a matter of rounding
            inn, out = row[inside], row[~inside]
            if len(inn) >= k:
                row = np.concatenate([inn[:k], out])
            else:   # added neighbours between 2.3 A and rc - 0.2 A, in this row only
                n_add = k - len(inn)
                u = rng.normal(size=(n_add, 3))
                u /= np.linalg.norm(u, axis=1)[:, None]
                r = rng.uniform(2.3, rc - 0.2, size=n_add)
                ids = s.x.shape[0] + len(extra) + np.arange(n_add)
                extra.extend(s.x[i] + u * r[:, None])
                row = np.concatenate([inn, ids, out[:max(0, longest - k)]])
            rng.shuffle(row)
        rows.append(np.asarray(row, np.int32))
    x = np.vstack([s.x, np.asarray(extra).reshape(-1, 3)])
    types = np.concatenate([s.types, np.ones(len(extra), np.int32)]).astype(np.int32)
    first = np.zeros(s.nlocal + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=first[1:])
    neigh = np.concatenate(rows)
    assert int(np.diff(first).max()) <= longest
    # the counts, from the lists as the kernels get them
    got = {}
    for i, k in want.items():
        d = x[neigh[first[i]:first[i + 1]]] - x[i]
        got[i] = int(((d * d).sum(1) <= rc * rc).sum())
    assert got == want
    assert sorted(set(got.values())) == list(COUNTS)
    return x, types, first.astype(np.int32), neigh, want


def _refit_path(tmp_pot_dir):
    """the potential of tests/test_fixed_shapes_cpu.py: the level-16 table with other coefficients, cutoffs and scaling"""
    p = mtpgen.random_potential(mtpgen.build_table(16), 1, 20251, 1.7, 5.6, 8, 0.37)
    path = str(tmp_pot_dir / "refit16_slot_gpu.mtp")
    if not os.path.exists(path):
        mtpgen.write_mtp(p, path)
    return path


@pytest.fixture(scope="module", params=["W_L16", "refit"])
def case(request, lattice, tmp_path_factory):
    """one potential with its edge system, its deterministic context and the oracle's result (computed once, not changed)"""
    from oracle.pyoracle import Oracle
    if request.param == "W_L16":
        path = os.path.join(POT, "W_L16.mtp")
    else:
        path = _refit_path(tmp_path_factory.mktemp("slot_pots"))
    pot = capi.Potential(path)
    x, types, first, neigh, want = _edge_system(lattice, pot.info.max_cutoff, 97)
    ctx = capi.Context(pot, 0)
    ctx.set_deterministic(True)
    ctx.set_neighbors(lattice.ilist, first, neigh, x.shape[0])
    ref = Oracle(path).compute(x, types, lattice.ilist, first, neigh, eflag=3, vflag=4)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(name=request.param, ctx=ctx, x=x, types=types, want=want, ref=ref, nlocal=lattice.nlocal)


def _both(case, monkeypatch, **kw):
    ctx = case["ctx"]
    with monkeypatch.context() as m:
        m.delenv("MTP_FIXED_SHAPE", raising=False)
        a = ctx.compute(case["x"], case["types"], **kw)
        na = ctx.last_shape()
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        b = ctx.compute(case["x"], case["types"], **kw)
        nb = ctx.last_shape()
    return a, na, b, nb


@pytest.mark.parametrize("eflag", [1, 3])
@pytest.mark.parametrize("vflag", [1, 5])
def test_fixed_kernel_is_bitwise_the_generic_one_at_the_count_edges(case, monkeypatch, eflag, vflag):
    a, na, b, nb = _both(case, monkeypatch, eflag=eflag, vflag=vflag)
    assert na == FORCE and nb == ""
    assert np.abs(a["f"]).max() > 1e-3
    for k in a:
        ga, gb = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(ga, gb), (case["name"], eflag, vflag, k, float(np.abs(ga - gb).max()))


def test_fixed_kernel_agrees_with_the_oracle_at_the_count_edges(case, monkeypatch):
    monkeypatch.delenv("MTP_FIXED_SHAPE", raising=False)
    got = case["ctx"].compute(case["x"], case["types"], eflag=3, vflag=4)
    assert case["ctx"].last_shape() == FORCE
    want = case["ref"]

    def close(g, w, what, atol=1e-9, rtol=1e-10):   # the tolerances of tests/test_gpu_parity.py
        scale = max(1.0, float(np.abs(w).max()))
        err = float(np.abs(np.asarray(g) - np.asarray(w)).max())
        assert err <= atol + rtol * scale, "%s %s: max abs err %.3e (scale %.3e)" % (case["name"], what, err, scale)

    close(got["f"], want["f"], "forces")
    n = case["nlocal"]
    assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n)
    close(got["eatom"], want["eatom"], "eatom", atol=1e-10)
    close(got["virial"], want["virial"], "virial", atol=1e-8)
    close(got["vatom"], want["vatom"], "vatom")
    # an atom without neighbours has the species energy alone and no force of its own making
    lone = [i for i, k in case["want"].items() if k == 0]
    assert len(lone) == PER_COUNT
    assert np.array_equal(got["eatom"][lone], np.full(len(lone), got["eatom"][lone[0]]))
