"""Batched force constants on the device (md.hessian_cells; mtp_hess_step, mtp_hess_finish).  The kernels alone against the numpy
twin of tests/_hess.py BIT FOR BIT, with forces and per-atom energies of the analytic surface of tests/_neb.py made by torch
between the launches (the twin is handed the very forces the kernel saw): every segment size, selection and workgroup filling,
batch independence, failures that stay at home, argument errors.  Then whole runs over two potentials against the host-driven
loop (one md.evaluate_cells call per explicitly displaced copy) and against central differences of the CPU oracle, within the
project's force parity bound divided by the step, and relax_cells -> hessian_cells -> modes end to end."""
import functools
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

import _batch
import _cells
import _hess
import _neb
from _cells import LIST_CUTOFF, POT

SENTINEL = -77.0
SIZES = (1, 2, 5, 0, 8, 54, 256, 257)         # 257: the first segment above MTP_BATCH_WAVE_ROWS, served by a whole workgroup
MASSES = {1: np.array([183.84]), 2: np.array([183.84, 186.207])}
H_STEP = 0.01


# ---- the kernels alone ---------------------------------------------------------------------------------------------------

def _device_pass(S, mode, h=H_STEP, mass_weight=False, nan_at=None, with_twin=True):
    """mtp_hess_step for launches 0 .. K and mtp_hess_finish over the batch S with the selection `mode`, eatom and forces by
    torch between the launches.  One row (one element) more than the batch holds is allocated in every array and filled with a
    sentinel.  With `with_twin` the twin is stepped along on the forces of every launch, copied back.  Returns the device's
    arrays (numpy) and the twin."""
    import torch
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = lambda shape, fill=SENTINEL, dtype=torch.float64: torch.full(shape, fill, dtype=dtype, device=dev)
    pad = lambda a, fill: np.concatenate([a, np.full((1,) + a.shape[1:], fill, dtype=a.dtype)])
    ncfg, n = len(S["cfg_first"]) - 1, int(S["cfg_first"][-1])
    sel_first, sel = _hess.selection(S["cfg_first"], mode)
    twin = _hess.Twin(S["cfg_first"], sel_first, sel, h)
    total = int(twin.h_first[-1])
    consts = [to(pad(S[k], 0.0)) for k in _neb.SURFACE_KEYS]
    x = to(pad(S["x0"], SENTINEL))
    x0 = x.clone()
    H = torch.zeros(total + 1, dtype=torch.float64, device=dev)
    H[total] = SENTINEL
    A = dict(cfg_first=to(S["cfg_first"]), sel_first=to(sel_first), sel=to(pad(sel, -1)), h_first=to(twin.h_first[:-1].copy()),
             type=to(pad(S["types"], 1)), mass=to(_neb.SURFACE_MASSES), f0=full((n + 1, 3)),
             fmax=torch.zeros(ncfg + 1, dtype=torch.float64, device=dev), energy=torch.zeros(ncfg + 1, dtype=torch.float64, device=dev),
             status=torch.zeros(ncfg + 1, dtype=torch.int32, device=dev), diag=torch.zeros((ncfg + 1, 2), dtype=torch.float64, device=dev))
    for key in ("fmax", "energy", "status", "diag"):
        A[key][ncfg] = SENTINEL
    cf_t = A["cfg_first"]
    xh, xh0 = S["x0"].copy(), S["x0"].copy()
    for k in range(twin.K + 1):
        e, f = _neb.surface(torch, x, *consts)
        if nan_at is not None and nan_at[0] == k:
            f[nan_at[1], nan_at[2]] = float("nan")
        capi.hess_step(cf_t, A["sel_first"], A["sel"], twin.sel_max, k, h, x, x0, f, e, A["h_first"], H, A["f0"], A["fmax"], A["energy"],
                       A["status"], stream=st)
        if with_twin:
            twin.step(k, xh, xh0, f.cpu().numpy()[:n], eatom=e.cpu().numpy()[:n])
    capi.hess_finish(A["sel_first"], A["sel"], A["type"], A["mass"], mass_weight, A["h_first"], H, A["diag"], A["status"], stream=st)
    twin.finish(S["types"], _neb.SURFACE_MASSES, mass_weight)
    torch.cuda.synchronize()
    got = {k: A[k].cpu().numpy() for k in ("f0", "fmax", "energy", "status", "diag")}
    got.update(H=H.cpu().numpy(), x=x.cpu().numpy(), first=twin.h_first)
    # nothing behind the last row, element or configuration, and after launch K the positions are the saved ones to the bit
    assert got["H"][total] == SENTINEL and (got["f0"][n] == SENTINEL).all() and (got["x"][n] == SENTINEL).all()
    assert got["fmax"][ncfg] == SENTINEL and got["energy"][ncfg] == SENTINEL and got["status"][ncfg] == int(SENTINEL)
    assert (got["diag"][ncfg] == SENTINEL).all()
    assert np.array_equal(got["x"][:n], S["x0"])
    if with_twin:
        assert np.array_equal(xh, S["x0"])
    return got, twin


def _assert_bits(got, twin, what):
    n, ncfg, total = len(twin.f0), twin.ncfg, int(twin.h_first[-1])
    for key, want in (("H", twin.H), ("f0", twin.f0), ("fmax", twin.fmax), ("energy", twin.energy), ("diag", twin.diag)):
        have = got[key][: len(want)]
        same = np.array_equal(have.view(np.int64), np.ascontiguousarray(want).view(np.int64))
        if not same:
            print("%s: %s differs, worst %.3e" % (what, key, float(np.nanmax(np.abs(have - want)))))
        assert same, (what, key)
    assert np.array_equal(got["status"][:ncfg], twin.status), what
    assert len(got["H"]) == total + 1 and len(got["f0"]) == n + 1


@functools.lru_cache(maxsize=None)
def _surface(sizes=SIZES, seed=3):
    return _hess.surface_batch(sizes, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,mass_weight", [("none", False), ("one", True), ("last", False), ("all", True), ("mixed", False),
                                              ("mixed", True)])
def test_kernels_alone_equal_the_twin_bit_for_bit(mode, mass_weight):
    """configurations of 1, 2, 5, 0, 8, 54, 256 and 257 rows in one batch (two workgroups), selections of none, one atom, the
    last atom only, all, and a different one per configuration with atoms out of order: H, f0, fmax, energy, status and the two
    diagnostics have the twin's bits.  The Hessians are those of the surface: the asymmetry is rounding only, off its xx
    entries the surface is quadratic."""
    S = _surface()
    got, twin = _device_pass(S, mode, mass_weight=mass_weight)
    _assert_bits(got, twin, "%s, mass_weight %r" % (mode, mass_weight))
    assert not twin.status.any()
    m = twin.m
    print("%s: m = %r, K = %d, asymmetry %.3e, sum rule %.3e" % (mode, list(m), twin.K, twin.diag[:, 0].max(), twin.diag[:, 1].max()))
    assert (mode == "none") == (twin.K == 0) and (twin.fmax[[0, 1, 2, 4, 5, 6, 7]] > 0.0).all() and twin.fmax[3] == 0.0
    if mode == "all":
        assert twin.K == 6 * 257
        j = 5                                                 # the matrix is the surface's: mass-weighted analytic curvatures
        r0, r1 = int(S["cfg_first"][j]), int(S["cfg_first"][j + 1])
        Hj = twin.matrix(j) * np.sqrt(np.outer(*[np.repeat(_neb.SURFACE_MASSES[S["types"][r0:r1] - 1], 3)] * 2))
        assert np.abs(np.diag(Hj)[1::3] - 2.0 * S["B"][r0:r1]).max() < 1e-9 and np.abs(np.diag(Hj)[2::3] - 2.0 * S["D"][r0:r1]).max() < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(8,), (257,), (1, 2, 5, 8), (1, 2, 5, 0, 8)], ids=lambda s: "ncfg%d_%d" % (len(s), s[0]))
def test_kernels_alone_with_one_four_and_five_configurations(sizes):
    """ncfg = 1, 4 and 5: a workgroup's four wavefronts are once partly idle, once all busy, and once a second workgroup has
    one busy wavefront; a batch that is one long segment"""
    S = _surface(sizes, 7)
    mode = "some" if sizes == (257,) else "all"
    got, twin = _device_pass(S, mode)
    _assert_bits(got, twin, repr(sizes))
    assert not twin.status.any() and twin.K == 6 * int(twin.m.max())


@pytest.mark.gpu
def test_a_configuration_alone_has_the_bits_it_has_inside_a_batch_of_300():
    sizes = tuple([(1, 2, 5, 0, 8, 3)[j % 6] for j in range(295)] + [54, 1, 2, 5] + [257])
    S = _surface(sizes, 11)
    batch, twin = _device_pass(S, "mixed", mass_weight=True, with_twin=False)
    first = twin.h_first
    for j in (0, 4, 7, 155, 296, 295, 299):
        # the selection pattern of "mixed" goes by the configuration's number: alone it is number 0, so pick its mode by name
        mode = ("all", "one", "last", "none", "some")[j % 5]
        alone, t1 = _device_pass(_hess.sub_batch(S, [j]), mode, mass_weight=True, with_twin=False)
        r0, r1 = int(S["cfg_first"][j]), int(S["cfg_first"][j + 1])
        assert int(t1.m[0]) == int(twin.m[j])
        assert np.array_equal(alone["H"][:-1], batch["H"][first[j]: first[j + 1]]), j
        assert np.array_equal(alone["f0"][:-1], batch["f0"][r0:r1])
        for key in ("fmax", "energy", "diag", "status"):
            assert np.array_equal(alone[key][0], batch[key][j]), (j, key)
        print("configuration %d (%d rows, %d selected): the same bits alone" % (j, r1 - r0, int(twin.m[j])))
    assert np.abs(batch["H"][:-1]).max() > 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("launch", [7, 8, 0], ids=["after_plus_h", "after_minus_h", "f0"])
def test_a_poisoned_force_fails_its_configuration_only(launch):
    """one NaN in a selected force component of the 8-atom configuration in front of launch 7 (which harvests a +h call), launch 8
    (a -h call) or launch 0 (f0): its status is "failed" from then on, what it had of H stays as it was and nothing more is
    written, its positions are back at x0; every other configuration has the bits of the clean run"""
    S = _surface((5, 3, 8, 0, 6, 70, 257), 13)
    clean, ctwin = _device_pass(S, "all", with_twin=False)
    row = int(S["cfg_first"][2]) + 4
    got, twin = _device_pass(S, "all", nan_at=(launch, row, 1))
    _assert_bits(got, twin, "poisoned at launch %d" % launch)
    assert list(twin.status) == [0, 0, _hess.FAILED, 0, 0, 0, 0] and not got["diag"][2].any()
    first = twin.h_first
    for j in (0, 1, 4, 5, 6):
        assert np.array_equal(got["H"][first[j]: first[j + 1]], clean["H"][first[j]: first[j + 1]]), j
        assert np.array_equal(got["diag"][j], clean["diag"][j])
    # launches 2, 4, 6 completed rows 0, 1, 2 and launch 7 parks row 3: those are there (in front of launch 8: row 3 still as
    # parked), every later row was never written
    mine = got["H"][first[2]: first[3]].reshape(24, 24)
    written = {7: 3, 8: 4, 0: 0}[launch]
    assert not mine[written:].any() and all(mine[c].any() for c in range(written))


@pytest.mark.gpu
def test_argument_errors_launch_nothing():
    import torch
    S = _surface((5, 3, 8), 17)
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sel_first, sel = _hess.selection(S["cfg_first"], "all")
    n, ncfg = len(S["x0"]), 3
    h_first = np.concatenate([[0], np.cumsum((3 * np.diff(sel_first)) ** 2)]).astype(np.int64)
    out = dict(x=to(S["x0"]), H=torch.full((int(h_first[-1]),), SENTINEL, dtype=torch.float64, device=dev),
               f0=torch.full((n, 3), SENTINEL, dtype=torch.float64, device=dev),
               fmax=torch.full((ncfg,), SENTINEL, dtype=torch.float64, device=dev),
               energy=torch.full((ncfg,), SENTINEL, dtype=torch.float64, device=dev),
               status=torch.zeros(ncfg, dtype=torch.int32, device=dev),
               diag=torch.full((ncfg, 2), SENTINEL, dtype=torch.float64, device=dev))
    before = {k: v.clone() for k, v in out.items()}
    fix = dict(cfg_first=to(S["cfg_first"]), sel_first=to(sel_first), sel=to(sel), x0=to(S["x0"]), f=torch.ones((n, 3), dtype=torch.float64, device=dev),
               eatom=torch.ones(n, dtype=torch.float64, device=dev), h_first=to(h_first[:-1].copy()), type=to(S["types"]),
               mass=to(_neb.SURFACE_MASSES))

    def step(stream=st, sel_max=8, k=0, h=H_STEP, **swap):
        a = dict(fix, **out)
        a.update(swap)
        capi.hess_step(a["cfg_first"], a["sel_first"], a["sel"], sel_max, k, h, a["x"], a["x0"], a["f"], a["eatom"], a["h_first"],
                       a["H"], a["f0"], a["fmax"], a["energy"], a["status"], stream=stream)

    def finish(stream=st, **swap):
        a = dict(fix, **out)
        a.update(swap)
        capi.hess_finish(a["sel_first"], a["sel"], a["type"], a["mass"], True, a["h_first"], a["H"], a["diag"], a["status"], stream=stream)

    bad = [dict(stream=None), dict(h=0.0), dict(h=-H_STEP), dict(h=float("nan")), dict(h=float("inf")), dict(k=-1), dict(k=49),
           dict(sel_max=-1), dict(sel_max=0, k=1), dict(sel_max=capi.HESS_MAX_SELECTED + 1)]
    bad += [{key: None} for key in ("sel_first", "sel", "x", "x0", "f", "eatom", "h_first", "H", "f0", "fmax", "energy", "status")]
    for kw in bad:
        with pytest.raises(capi.MtpError) as ei:
            step(**kw)
        assert ei.value.code == -20, kw
    # (the wrapper counts the configurations on sel_first: that one missing is tests/test_hess_cpu.py's)
    for kw in [dict(stream=None)] + [{key: None} for key in ("sel", "type", "mass", "h_first", "H", "diag", "status")]:
        with pytest.raises(capi.MtpError) as ei:
            finish(**kw)
        assert ei.value.code == -20, kw
    torch.cuda.synchronize()
    for key, t in out.items():
        assert torch.equal(t, before[key]), key
    step(k=48)                                                       # the ends of the range are inside: the last launch ...
    step(sel_max=0, k=0)                                             # ... and a pass without a displacement
    torch.cuda.synchronize()
    assert not torch.equal(out["f0"], before["f0"])


# ---- whole runs ------------------------------------------------------------------------------------------------------------

POTS = [("W_L8.mtp", 1), ("WRe_L20.mtp", 2)]
SIX = [3, 50, 17, 0, 53, 29]                  # 6 of the 54 atoms, out of order


@functools.lru_cache(maxsize=None)
def _ctx(fname):
    return capi.Context(capi.Potential(os.path.join(POT, fname)), 0)


@functools.lru_cache(maxsize=None)
def _oracle(fname):
    from oracle.pyoracle import Oracle
    return Oracle(os.path.join(POT, fname))


def _atoms(case):
    return [None] * 5 + [SIX] if case == "six" else None


@functools.lru_cache(maxsize=None)
def _run(fname, species, case):
    """md.hessian_cells on the mixed batch: made once, shared, never written to"""
    from lammps_mtp_kokkos_amd.md import hessian_cells
    return hessian_cells(_ctx(fname), _batch.mixed_batch(species), h=H_STEP, atoms=_atoms(case), masses=MASSES[species],
                         list_cutoff=LIST_CUTOFF)


@functools.lru_cache(maxsize=None)
def _reference(fname, species, case):
    return _hess.reference_loop(_ctx(fname), _batch.mixed_batch(species), H_STEP, _atoms(case), MASSES[species], list_cutoff=LIST_CUTOFF)


def _bound(f0, H, h=H_STEP):
    """The project's force parity bound (_batch.close: 1e-9 + 1e-10 max(1, |f|max)) for each of the two forces of a difference
    quotient, divided by 2 h: |dH| <= (1e-9 + 1e-10 max(1, |f|max)) / h.  |f|max over the displaced copies is at most that of
    f0 plus h times the largest force constant."""
    fmax = (float(np.abs(f0).max()) if np.size(f0) else 0.0) + h * (float(np.abs(H).max()) if np.size(H) else 0.0)
    return (1e-9 + 1e-10 * max(1.0, fmax)) / h


def _assert_same_hessians(got, want_matrix, batch, what, skip=()):
    worst = 0.0
    for j, (pos, _, _) in enumerate(batch):
        if j in skip:
            continue
        want = want_matrix(j)
        bound = _bound(got[j]["f0"], want)
        err = float(np.abs(got[j]["hessian"] - want).max()) if want.size else 0.0
        print("%s, configuration %d (%d atoms, %d selected): |dH| %.3e (bound %.3e, |H|max %.3e)"
              % (what, j, len(pos), len(got[j]["atoms"]), err, bound, float(np.abs(want).max()) if want.size else 0.0))
        assert got[j]["hessian"].shape == want.shape and err <= bound, (what, j)
        worst = max(worst, err / bound)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["six", "all"])
@pytest.mark.parametrize("fname,species", POTS)
def test_hessian_cells_against_the_host_driven_loop(fname, species, case):
    """the mixed batch (1, 2, 5, 0, 8 and 54 atoms; the 54-atom member with 6 of its atoms, out of order, or with all): H within
    the force parity bound over the step; f0 and the energy against evaluate_cells at its own bounds; the sum rule within 3 n
    times the bound for the full selections; the asymmetry is printed (an O(h^2) truncation quantity, no derivable bound)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells
    batch = _batch.mixed_batch(species)
    got = _run(fname, species, case)
    twin, calls = _reference(fname, species, case)
    assert calls == 6 * (8 if case == "six" else 54) + 1 and not twin.status.any()
    _assert_same_hessians(got, twin.matrix, batch, "%s, %s" % (fname, case))
    plain = evaluate_cells(_ctx(fname), batch, list_cutoff=LIST_CUTOFF, vflag=0)
    for j, (pos, _, _) in enumerate(batch):
        r, n = got[j], len(pos)
        m = n if case == "all" or j != 5 else 6
        assert r["status"] == "ok" and r["hessian"].shape == (3 * m, 3 * m) and r["f0"].shape == (n, 3)
        assert np.array_equal(r["atoms"], np.arange(n) if m == n else SIX) and np.array_equal(r["hessian"], r["hessian"].T)
        _batch.close(r["f0"], plain[j]["f"], "f0, configuration %d" % j)
        _batch.close_energy(r["energy"], plain[j]["energy"], n, "energy, configuration %d" % j)
        want_fmax = float(np.sqrt((plain[j]["f"] ** 2).sum(1)).max()) if n else 0.0
        assert abs(r["fmax"] - want_fmax) <= 1e-9 + 1e-10 * max(1.0, want_fmax)
        bound = _bound(r["f0"], r["hessian"])
        print("configuration %d: asymmetry %.3e, sum rule %.3e (bound %.3e), twin: %.3e, %.3e"
              % (j, r["asymmetry"], r["sum_rule"], 3 * n * bound, twin.diag[j, 0], twin.diag[j, 1]))
        if m == n:
            assert r["sum_rule"] <= 3 * n * bound
    assert got[3]["hessian"].shape == (0, 0) and got[3]["energy"] == 0.0 and got[3]["fmax"] == 0.0
    assert max(np.abs(got[j]["hessian"]).max() for j in (1, 2, 4, 5)) > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_hessian_cells_against_central_differences_of_the_cpu_oracle(fname, species):
    """the members of up to 8 atoms: every atom displaced by +-h along every axis on the host, forces from the CPU oracle on the
    images of the numpy ghost twin, the same difference quotient and symmetrisation.  The bound is the same."""
    batch = _batch.mixed_batch(species)
    got = _run(fname, species, "all")
    orc = _oracle(fname)

    def want(j):
        pos, cell, types = batch[j]
        n = len(pos)
        H = np.zeros((3 * n, 3 * n))
        for c in range(3 * n):
            f = []
            for sign in (1.0, -1.0):
                p = pos.copy()
                p[c // 3, c % 3] = pos[c // 3, c % 3] + sign * H_STEP
                f.append(_cells.oracle_cell(orc, p, cell, types)[1].reshape(-1))
            H[c] = (f[1] - f[0]) * (1.0 / (2.0 * H_STEP))
        return 0.5 * (H + H.T)

    _assert_same_hessians(got, want, batch, "%s, oracle" % fname, skip=(5,))


def _far(batch):
    """the tilted cell handed over with its atoms many lattice vectors away (the same crystal)"""
    batch = list(batch)
    pos, cell, types = batch[2]
    batch[2] = (pos + np.array([[3, -2, 1], [0, 0, 0], [-7, 4, 0], [1, 1, 1], [0, -5, 2]]) @ cell, cell, types)
    return batch


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species", POTS)
def test_positions_many_lattice_vectors_away_give_the_same_hessian(fname, species):
    from lammps_mtp_kokkos_amd.md import hessian_cells
    batch = _far(_batch.mixed_batch(species))
    got = hessian_cells(_ctx(fname), batch, h=H_STEP, atoms=_atoms("six"), masses=MASSES[species], list_cutoff=LIST_CUTOFF)
    want = _run(fname, species, "six")
    _assert_same_hessians(got, lambda j: want[j]["hessian"], batch, "%s, far" % fname)
    _batch.close(got[2]["f0"], want[2]["f0"], "f0 of the far configuration")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [dict(max_atoms_per_pass=10), dict(max_hessian_bytes=8 * 24 * 24),
                                   dict(max_atoms_per_pass=7, max_hessian_bytes=8 * 24 * 24)], ids=["atoms", "bytes", "both"])
def test_a_batch_split_into_passes_has_the_hessians_of_the_whole_batch(split):
    """by atoms (1 2 5 0 | 8 | 54), by bytes (1 2 5 0 | 8 | 54 with its 6 selected) and by both (1 2 | 5 0 | 8 | 54): the empty
    configuration rides along in a pass"""
    from lammps_mtp_kokkos_amd.md import cut_hessian_passes, hessian_cells, plan_cell_passes
    fname, species = POTS[1]
    batch = _batch.mixed_batch(species)
    cells, natoms = np.array([c for _, c, _ in batch]), np.array([len(p) for p, _, _ in batch])
    nsel = np.array([1, 2, 5, 0, 8, 6])
    plan = cut_hessian_passes(plan_cell_passes(cells, natoms, LIST_CUTOFF, split.get("max_atoms_per_pass"))[0], cells, nsel, LIST_CUTOFF,
                              split.get("max_hessian_bytes", 2 ** 31))
    print("passes:", [(a, b) for a, b, _ in plan])
    assert len(plan) >= 3
    got = hessian_cells(_ctx(fname), batch, h=H_STEP, atoms=_atoms("six"), masses=MASSES[species], list_cutoff=LIST_CUTOFF, **split)
    want = _run(fname, species, "six")
    _assert_same_hessians(got, lambda j: want[j]["hessian"], batch, "%s, %r" % (fname, split))
    for j in range(len(batch)):
        _batch.close(got[j]["f0"], want[j]["f0"], "f0, configuration %d" % j)
        assert got[j]["status"] == "ok" and abs(got[j]["energy"] - want[j]["energy"]) <= 1e-10 * max(1.0, abs(want[j]["energy"]))


@pytest.mark.gpu
def test_mass_weighting_on_the_device_is_the_division_by_the_root_masses():
    from lammps_mtp_kokkos_amd.md import hessian_cells
    fname, species = POTS[1]
    batch = _batch.mixed_batch(species)
    got = hessian_cells(_ctx(fname), batch, h=H_STEP, atoms=_atoms("six"), masses=MASSES[species], mass_weight=True,
                        list_cutoff=LIST_CUTOFF)
    want = _run(fname, species, "six")
    """(two runs of the force call need not agree to the bit: the bound on H, divided by the masses)"""
    for j, (_, _, types) in enumerate(batch):
        M = np.repeat(MASSES[species][np.asarray(types)[want[j]["atoms"]] - 1], 3)
        w = 1.0 / np.sqrt(np.outer(M, M))
        err = np.abs(got[j]["hessian"] - want[j]["hessian"] * w)
        assert (err <= _bound(want[j]["f0"], want[j]["hessian"]) * w).all(), j
    # The largest entry of H / sqrt(m_c m_r) over the largest entry of H lies between 1 / m_max and 1 / m_min in exact
    # arithmetic, and ON an end of that interval when both maxima sit in a block of two atoms of one species (here they do:
    # the lighter species, the upper end).  So this is an equality test, and its two sides differ by
    #   (a) roundings.  Device: p = fl(m_c m_r), q = fl(sqrt p), t = fl(1 / q), fl(s t), each correctly rounded: relative
    #       errors u / 2 (the square root halves p's), u, u, u with u = 2^-53.  Host: the quotient of the two maxima and
    #       1 / m, u each.  5.5 u in all, which is 2.75 eps: 3 eps.
    #   (b) the two runs.  `got` and `want` come from two passes of force calls whose atomic sums need not run in the same
    #       order, so their H differ in the last places -- enough to put the quotient on either side of 1 / m from one
    #       run to the next (measured: 3 eps below in one run, equal in the next), which is how this assertion failed
    #       on unchanged kernels and passed when run again.  No count of roundings bounds that; the project's force
    #       parity bound does.  The loop above has just held every entry of got to want w within _bound w, hence
    #       max |got| <= (max |H| + _bound) / m_min and max |got| >= (max |H| - _bound) / m_max.
    hmax = np.abs(want[5]["hessian"]).max()
    ratio = np.abs(got[5]["hessian"]).max() / hmax
    slack = _bound(want[5]["f0"], want[5]["hessian"]) / hmax + 3.0 * np.finfo(np.float64).eps
    lo, hi = 1.0 / MASSES[species].max(), 1.0 / MASSES[species].min()
    print("mass weighting: max |H w| / max |H| = 1 / m_min x (1 %+.3e), = 1 / m_max x (1 %+.3e); eps %.3e, slack %.3e"
          % (ratio / hi - 1.0, ratio / lo - 1.0, np.finfo(np.float64).eps, slack))
    assert lo * (1.0 - slack) <= ratio <= hi * (1.0 + slack)


@pytest.mark.gpu
@pytest.mark.parametrize("fname,species,which", [("W_L8.mtp", 1, "cubic2"), ("WRe_L20.mtp", 2, "tilted5")])
def test_relax_then_hessian_then_modes_end_to_end(fname, species, which):
    """An input the relaxation tests converge, taken to ftol = 1e-6 eV/A, then hessian_cells and modes: a minimum has no unstable
    mode and exactly three zero modes (the translations).  The zero bound: the Hessian is off by at most dH = the force parity
    bound over h per entry, so by Weyl's inequality no eigenvalue of the mass-weighted matrix moves further than
    |dH|_2 / m_min <= 3 n dH / m_min; as a frequency that is sqrt(3 n dH FTM2V / m_min) / (2 pi)."""
    from lammps_mtp_kokkos_amd.md import FTM2V, hessian_cells, modes, relax_cells
    cfg = _cells.cubic2_cell() if which == "cubic2" else _cells.tilted5_cell(species)
    ctx = _ctx(fname)
    relaxed = relax_cells(ctx, [cfg], 2000, ftol=1e-6, masses=MASSES[species], list_cutoff=LIST_CUTOFF)["final"][0]
    print("%s: relax_cells: %s at step %d, fmax %.3e" % (fname, relaxed["status"], relaxed["step"], relaxed["fmax"]))
    assert relaxed["status"] == "converged" and relaxed["fmax"] <= 1e-6      # (otherwise the test's inputs are wrong)
    n = len(cfg[0])
    r = hessian_cells(ctx, [(relaxed["x"], cfg[1], cfg[2])], h=H_STEP, masses=MASSES[species], list_cutoff=LIST_CUTOFF)[0]
    assert r["status"] == "ok" and r["fmax"] <= 1e-6 + 1e-9
    masses = MASSES[species][np.asarray(cfg[2]) - 1]
    zero = np.sqrt(3 * n * _bound(r["f0"], r["hessian"]) * FTM2V / masses.min()) / (2.0 * np.pi)
    got = modes(r["hessian"], masses, zero_tol=zero)
    nu = got["frequencies"]
    print("%s: zero bound %.3e THz, frequencies [THz] %s, asymmetry %.3e, sum rule %.3e"
          % (fname, zero, np.array2string(nu, precision=4), r["asymmetry"], r["sum_rule"]))
    assert got["n_unstable"] == 0 and got["n_zero"] == 3 and int((np.abs(nu) <= zero).sum()) == 3
