"""The fixed-shape force kernel with table values kept in registers across its atom loop (csrc/mtp_wave_body.hpp:
block_regs_ct -- the row offsets of a lane's basic-moment block, decoded from the blob once per wavefront;
row_regs_ct -- the packed rows of the short product levels, loaded from the blob once per wavefront), on a system where
one wavefront meets atoms of every kind in every order.  (A third lever, g of the force phase from registers parked
by the tile build, passed these tests too and was dropped for want of a measured gain: profiles/r10_ab_force_regs.txt.)

A 17 x 17 x 17 bcc lattice (9,826 atoms, a = 3.04, jitter 0.1, list cutoff 7 A): the fixed shape is planned from 4,096
rows up, and the 3,072 wavefronts of its launch take three or four atoms each, so whatever a wavefront keeps across the
atom loop meets more than one atom.  With tests/test_gpu_slot_fields.py::_edge_system as the model, a quarter of the
rows (chosen with a fixed seed) get 0 entries inside the potential's cutoff, a quarter get 33, 64 or 65, the rest stay
as they are (one tile or two): a lone atom (no tile: the block addresses are formed and not used), a multi-tile atom
(every tile is built again in the force phase) and a single-tile atom (the tile and the park of the first build must
survive the product passes) follow one another.
Counts above an atom's own are reached by ghost atoms placed inside its cutoff and listed in its row only;
out-of-cutoff entries leave the row in exchange, so the longest row and with it the launch plan stay what they were.

Deterministic mode: the fixed kernel is bitwise the generic one (MTP_FIXED_SHAPE=0) on every output key -- for every
eflag x vflag, a refit of the level-16 table, a table loaded with another effort of the bank search (other packed rows
and block descriptors under the same shape: anything taken from the shape instead of the blob would show), and after an
install of new coefficients into the live context.  Default mode: against the oracle at the tolerances of
tests/test_gpu_parity.py.  Row ranges (compute_device_rows) take the fixed shape too (tests/test_gpu_table_fields.py), so
a three-range call is compared as well."""
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
W16 = os.path.join(POT, "W_L16.mtp")
FORCE = "w16_force_3ps"
FILLED = (33, 64, 65)


@pytest.fixture(scope="module")
def lattice():
    pos, box = mtpgen.bcc_lattice(17, 17, 17, a=3.04, jitter=0.1, seed=31)
    s = periodic_system(pos, box, None, 7.0)
    assert s.nlocal == 9826
    return s


def _edge_system(s, rc, seed):
    """(x, types, first, neigh, want, counts): want[i] = in-cutoff entries of a rewritten row i (0 | 33 | 64 | 65), counts =
    in-cutoff entries of every row"""
    rng = np.random.default_rng(seed)
    longest = int(np.diff(s.first).max())
    quarter = s.nlocal // 4
    chosen = rng.choice(s.nlocal, size=2 * quarter, replace=False)
    want = {int(a): 0 for a in chosen[:quarter]}
    want.update({int(a): FILLED[k % len(FILLED)] for k, a in enumerate(chosen[quarter:])})
    rows, extra, n_extra = [], [], 0
    for i in range(s.nlocal):
        row = s.neigh[s.first[i]:s.first[i + 1]]
        if i in want:
            k = want[i]
            d = s.x[row] - s.x[i]
            r2 = (d * d).sum(1)
            inside = r2 <= rc * rc
            assert np.abs(np.sqrt(r2) - rc).min() > 1e-9   # no entry whose side of the cutoff is a matter of rounding
            inn, out = row[inside], row[~inside]
            if len(inn) >= k:
                row = np.concatenate([inn[:k], out])
            else:   # added neighbours between 2.3 A and rc - 0.2 A, in this row only
                n_add = k - len(inn)
                u = rng.normal(size=(n_add, 3))
                u /= np.linalg.norm(u, axis=1)[:, None]
                r = rng.uniform(2.3, rc - 0.2, size=n_add)
                ids = s.x.shape[0] + n_extra + np.arange(n_add)
                extra.append(s.x[i] + u * r[:, None])
                n_extra += n_add
                row = np.concatenate([inn, ids, out[:max(0, longest - k)]])
            rng.shuffle(row)
        rows.append(np.asarray(row, np.int32))
    x = np.vstack([s.x] + extra)
    types = np.concatenate([s.types, np.ones(n_extra, np.int32)]).astype(np.int32)
    first = np.zeros(s.nlocal + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=first[1:])
    neigh = np.concatenate(rows)
    assert int(np.diff(first).max()) == longest
    # the counts, from the lists as the kernels get them
    owner = np.repeat(np.arange(s.nlocal), np.diff(first))
    d = x[neigh] - x[s.ilist[owner]]
    counts = np.bincount(owner, weights=(d * d).sum(1) <= rc * rc, minlength=s.nlocal).astype(int)
    assert all(counts[i] == k for i, k in want.items())
    got = np.bincount(counts[list(want)], minlength=66)
    assert got[0] == quarter and got[33] + got[64] + got[65] == quarter and min(got[33], got[64], got[65]) >= quarter // 3
    return x, types, first.astype(np.int32), neigh, want, counts


def _refit_path(tmp_pot_dir):
    """the potential of tests/test_fixed_shapes_cpu.py: the level-16 table with other coefficients, cutoffs and scaling"""
    p = mtpgen.random_potential(mtpgen.build_table(16), 1, 20251, 1.7, 5.6, 8, 0.37)
    path = str(tmp_pot_dir / "refit16_force_regs.mtp")
    if not os.path.exists(path):
        mtpgen.write_mtp(p, path)
    return path


def _case(lattice, pot, seed=131):
    x, types, first, neigh, want, counts = _edge_system(lattice, pot.info.max_cutoff, seed)
    ctx = capi.Context(pot, 0)
    ctx.set_deterministic(True)
    ctx.set_neighbors(lattice.ilist, first, neigh, x.shape[0])
    return dict(ctx=ctx, x=x, types=types, first=first, neigh=neigh, want=want, counts=counts, nlocal=lattice.nlocal)


@pytest.fixture(scope="module")
def w16(lattice):
    """W_L16.mtp with its edge system and a deterministic context (the system is computed once, not changed)"""
    c = _case(lattice, capi.Potential(W16))
    for k in ("x", "types", "first", "neigh"):
        c[k].setflags(write=False)
    rest = np.delete(c["counts"], list(c["want"]))   # the rows left as they were: single-tile and two-tile atoms
    assert rest.min() >= 1 and (rest <= 32).sum() > 100 and (rest > 32).sum() > 100
    return c


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
    assert na == FORCE and nb == ""
    return a, b


def _bitwise(a, b, what):
    assert np.abs(a["f"]).max() > 1e-3
    for k in a:
        ga, gb = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(ga, gb), (what, k, float(np.abs(ga - gb).max()))


@pytest.mark.parametrize("eflag", [0, 1, 2, 3])
@pytest.mark.parametrize("vflag", [0, 1, 4, 5])
def test_every_flag_combination_is_bitwise_the_generic_kernel(w16, monkeypatch, eflag, vflag):
    a, b = _both(w16, monkeypatch, eflag=eflag, vflag=vflag)
    _bitwise(a, b, "eflag %d vflag %d" % (eflag, vflag))


def test_refit_is_bitwise_the_generic_kernel(lattice, monkeypatch, tmp_path_factory):
    case = _case(lattice, capi.Potential(_refit_path(tmp_path_factory.mktemp("force_regs_pots"))))
    a, b = _both(case, monkeypatch, eflag=3, vflag=5)
    _bitwise(a, b, "refit")


def test_another_bank_search_effort_is_bitwise_the_generic_kernel(lattice, w16, monkeypatch):
    """the suites load with MTP_BANK_ROUNDS=2 (tests/conftest.py); no search at all numbers the moments differently, so
    the packed rows and the block descriptors in the blob differ while every field of the shape stays"""
    with monkeypatch.context() as m:
        m.setenv("MTP_BANK_ROUNDS", "0")
        m.setenv("MTP_BANK_SCALE", "1")
        pot = capi.Potential(W16)
    case = _case(lattice, pot)
    a, b = _both(case, monkeypatch, eflag=3, vflag=5)
    _bitwise(a, b, "bank rounds 0")
    # and the numbering is a speed matter only: the forces are those of the default table to rounding
    c = w16["ctx"].compute(w16["x"], w16["types"], eflag=3, vflag=5)
    assert w16["ctx"].last_shape() == FORCE
    assert float(np.abs(a["f"] - c["f"]).max()) <= 1e-9 + 1e-10 * max(1.0, float(np.abs(c["f"]).max()))
    # ... and it IS another table: the rows of a level are taken in another order, so the sums of the product passes
    # round differently and the per-atom energies differ from the default table's in their last bits
    diff = int((a["eatom"] != c["eatom"]).sum())
    print("atoms whose energy differs in the last bits between the two tables: %d of %d" % (diff, case["nlocal"]))
    assert diff > 0


def test_install_on_a_live_context_is_bitwise_the_generic_kernel(lattice, monkeypatch):
    pot = capi.Potential(W16)
    case = _case(lattice, pot)
    ctx = case["ctx"]
    first = ctx.compute(case["x"], case["types"], eflag=3, vflag=5)
    assert ctx.last_shape() == FORCE
    rng = np.random.default_rng(20261018)
    t = pot.tables()
    new = [np.asarray(t[k], np.float64).reshape(-1) * (1.0 + 1e-2 * rng.standard_normal(np.size(t[k])))
           for k in ("radial_coeffs", "species_coeffs", "moment_coeffs")]
    ctx.install_coeffs(*new)
    a, b = _both(case, monkeypatch, eflag=3, vflag=5)
    _bitwise(a, b, "after install")
    assert not np.array_equal(a["f"], first["f"]) and a["energy"] != first["energy"]
    assert not np.array_equal(a["eatom"], first["eatom"])


def test_default_mode_against_the_oracle(lattice, w16, monkeypatch):
    from oracle.pyoracle import Oracle
    monkeypatch.delenv("MTP_FIXED_SHAPE", raising=False)
    ctx = capi.Context(capi.Potential(W16), 0)   # default mode: native fp64 atomics
    ctx.set_neighbors(lattice.ilist, w16["first"], w16["neigh"], w16["x"].shape[0])
    got = ctx.compute(w16["x"], w16["types"], eflag=3, vflag=5)
    assert ctx.last_shape() == FORCE
    want = Oracle(W16).compute(w16["x"], w16["types"], lattice.ilist, w16["first"], w16["neigh"], eflag=3, vflag=4)

    def close(g, w, what, atol=1e-9, rtol=1e-10):   # the tolerances of tests/test_gpu_parity.py
        scale = max(1.0, float(np.abs(w).max()))
        err = float(np.abs(np.asarray(g) - np.asarray(w)).max())
        print("%s: max abs err %.3e (scale %.3e)" % (what, err, scale))
        assert err <= atol + rtol * scale, "%s: max abs err %.3e (scale %.3e)" % (what, err, scale)

    close(got["f"], want["f"], "forces")
    n = w16["nlocal"]
    assert abs(got["energy"] - want["energy"]) / n <= 1e-10 * max(1.0, abs(want["energy"]) / n)
    close(got["eatom"], want["eatom"], "eatom", atol=1e-10)
    close(got["virial"], want["virial"], "virial", atol=1e-8)
    close(got["vatom"], want["vatom"], "vatom")
    # an atom without neighbours has exactly the species energy
    lone = [i for i, k in w16["want"].items() if k == 0]
    assert len(lone) == n // 4
    species = float(capi.Potential(W16).tables()["species_coeffs"].reshape(-1)[0])
    assert np.array_equal(got["eatom"][lone], np.full(len(lone), species))


def test_three_row_ranges_agree_with_the_whole_call(lattice, w16, monkeypatch):
    """compute_device_rows launches take the fixed shape.  Forces (fixed-point sums in deterministic mode), eatom and
    vatom do not depend on how the rows are dealt to wavefronts: bitwise the whole call.  The energy and virial totals are
    floating-point sums per wavefront, whose order follows the deal: bitwise the generic kernel over the same three
    ranges, and the whole call's to the tolerance of tests/test_gpu_parity.py."""
    import torch
    monkeypatch.delenv("MTP_FIXED_SHAPE", raising=False)
    dev = torch.device("cuda", 0)
    n, nall = w16["nlocal"], w16["x"].shape[0]
    ctx = capi.Context(capi.Potential(W16), 0)
    ctx.set_deterministic(True)
    il, fi, ne = (torch.from_numpy(np.ascontiguousarray(v, np.int32)).to(dev) for v in (lattice.ilist, w16["first"], w16["neigh"]))
    ctx.set_neighbors_device(il, fi, ne, nall, int(np.diff(w16["first"]).max()))
    x = torch.from_numpy(np.ascontiguousarray(w16["x"])).to(dev)
    ty = torch.from_numpy(np.ascontiguousarray(w16["types"], np.int32)).to(dev)
    cuts = [0, 3001, 6503, n]   # three uneven ranges (the plan, and with it the shape, follows the list, not the range)

    def run(ranges):
        f = torch.zeros((nall, 3), dtype=torch.float64, device=dev)
        ev = torch.zeros(8, dtype=torch.float64, device=dev)
        ea = torch.zeros(nall, dtype=torch.float64, device=dev)
        va = torch.zeros((nall, 6), dtype=torch.float64, device=dev)
        kw = dict(eflag=3, vflag=5, eatom_t=ea, vatom_t=va, ev_t=ev)
        names = []
        for k, (b, e) in enumerate(ranges):
            ctx.compute_device_rows(b, e - b, k == len(ranges) - 1, x, ty, f, **kw)
            names.append(ctx.last_shape())
        ctx.synchronize()
        torch.cuda.synchronize()
        return dict(f=f.cpu().numpy(), ev=ev.cpu().numpy(), eatom=ea.cpu().numpy(), vatom=va.cpu().numpy()), names

    three = list(zip(cuts[:-1], cuts[1:]))
    whole, nw = run([(0, n)])
    parts, np_ = run(three)
    with monkeypatch.context() as m:
        m.setenv("MTP_FIXED_SHAPE", "0")
        gen, ng = run(three)
    assert nw == [FORCE] and ng == ["", "", ""]
    assert np_ == [FORCE, FORCE, FORCE]
    _bitwise(parts, gen, "three ranges, fixed against generic")
    for k in ("f", "eatom", "vatom"):
        assert np.array_equal(parts[k], whole[k]), (k, float(np.abs(parts[k] - whole[k]).max()))
    assert np.abs(parts["ev"] - whole["ev"]).max() <= 1e-8 + 1e-10 * max(1.0, float(np.abs(whole["ev"]).max()))
