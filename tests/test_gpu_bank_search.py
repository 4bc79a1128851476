"""The table of the annealed bank search (csrc/mtp_bank_search.hpp: search, v2) under the force kernels, on the GPU.

v2 exchanges the two factors of product rows, moves rows inside their levels and numbers the moments differently; the
kernels read all of that from the blob, so with its table the fixed force shape of level 16 is still bitwise the generic
kernel (MTP_FIXED_SHAPE=0) in deterministic mode, and forces, energies and virials agree with the v1 table
(MTP_BANK_SEARCH=v1) and with the oracle inside the tolerances of tests/test_gpu_parity.py (_close and _compare there:
forces 1e-9 + 1e-10 |F|max, energy per atom 1e-10 relative, per-atom energies 1e-10, virial 1e-8).  The system is the
13 x 13 x 13 lattice of tests/test_gpu_row_reads.py with its rewritten rows (0, 1, 32, 33 and 65 entries inside the
cutoff).  One grade call on W_L16_nbh.almtp covers the candidate vectors, which read the same numbering."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

from test_gpu_parity import _close, _grade_compare, _system
from test_gpu_row_reads import FLAGS, FORCE, W16, _bitwise, _both, _context, system  # noqa: F401  (system: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(system):
    """W_L16.mtp under both searches at the effort of the suites, one context each; the oracle's answer once"""
    from oracle.pyoracle import Oracle
    out = {}
    for search in ("v2", "v1"):
        mp = pytest.MonkeyPatch()
        if search == "v1":
            mp.setenv("MTP_BANK_SEARCH", "v1")
        else:
            mp.delenv("MTP_BANK_SEARCH", raising=False)
        try:
            pot = capi.Potential(W16)
        finally:
            mp.undo()
        out[search] = (pot, _context(pot, system))
    s = system
    want = Oracle(W16).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    out["oracle"] = want
    return out


@pytest.mark.parametrize("flags", FLAGS, ids=["e0v0", "e1v1", "e3v5"])
def test_fixed_shape_is_bitwise_the_generic_kernel_with_the_new_table(system, tables, monkeypatch, flags):
    _, ctx = tables["v2"]
    a, b = _both(ctx, system, monkeypatch, eflag=flags[0], vflag=flags[1])   # (asserts last_shape() of both)
    _bitwise(a, b, "v2 table, eflag %d vflag %d" % flags)


def test_new_table_agrees_with_the_v1_table_and_the_oracle(system, tables, monkeypatch):
    s, want = system, tables["oracle"]
    got = {}
    for search in ("v2", "v1"):
        ctx = tables[search][1]
        with monkeypatch.context() as m:
            m.delenv("MTP_FIXED_SHAPE", raising=False)
            got[search] = ctx.compute(s.x, s.types, eflag=3, vflag=4)
            assert ctx.last_shape() == FORCE
    n = s.nlocal
    for name, ref in (("v1 table", got["v1"]), ("oracle", want)):
        g = got["v2"]
        print("%s: max |dF| %.3e, |dE|/atom %.3e, max |d eatom| %.3e, max |d virial| %.3e" % (
            name, np.abs(g["f"] - ref["f"]).max(), abs(g["energy"] - ref["energy"]) / n,
            np.abs(g["eatom"] - ref["eatom"]).max(), np.abs(np.asarray(g["virial"]) - np.asarray(ref["virial"])).max()))
        _close(g["f"], ref["f"], "forces against the " + name)
        assert abs(g["energy"] - ref["energy"]) / n <= 1e-10 * max(1.0, abs(ref["energy"]) / n)
        _close(g["eatom"], ref["eatom"], "eatom against the " + name, atol=1e-10)
        _close(g["virial"], ref["virial"], "virial against the " + name, atol=1e-8)
        _close(g["vatom"], ref["vatom"], "vatom against the " + name)
    # two tables: the sums of the product passes round differently somewhere
    assert (np.asarray(got["v2"]["eatom"]) != np.asarray(got["v1"]["eatom"])).any()


def test_grades_read_the_new_numbering(monkeypatch):
    monkeypatch.delenv("MTP_BANK_SEARCH", raising=False)
    s = _system((4, 4, 4))
    pot, got, want = _grade_compare(os.path.join(ROOT, "potentials", "W_L16_nbh.almtp"), s)
    _close(got["grades"][s.ilist], want["grades"][s.ilist], "grades", atol=1e-9, rtol=1e-9)
    assert abs(got["max_grade"] - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])
