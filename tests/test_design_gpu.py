"""Design rows of the linear refit on the device (csrc/mtp_design.hip; Context.design_rows, md.design_cells,
md.fit_linear).  The judge of every matrix entry is the reference algorithm by linearity: the oracle's unit-coefficient
columns (tests/_design.py), each entry within 1e-9 + 1e-10 max |column|.  Above level 8 the tests judge matrix entries,
residuals and predictions, never recovered coefficients: the complete level-16 table is rank deficient by construction."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _batch  # noqa: E402
import _cells  # noqa: E402
import _design  # noqa: E402
import _stars  # noqa: E402
import _train  # noqa: E402
from lammps_mtp_kokkos_amd import capi, md  # noqa: E402

POT = _design.POT


def _device_stream():
    import torch
    dev = torch.device("cuda:0")
    return dev, capi.use_private_torch_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def _ctx(fname):
    return capi.Context(capi.Potential(os.path.join(POT, fname)), 0)


@functools.lru_cache(maxsize=None)
def _oracle(fname):
    from oracle.pyoracle import Oracle
    return Oracle(os.path.join(POT, fname))


def _theta0(fname):
    t = capi.Potential(os.path.join(POT, fname)).tables()
    return np.concatenate([t["species_coeffs"], t["moment_coeffs"]])


# ---- batches and their oracle matrices: computed once, shared, never written to -------------------------------------------
def batch1():
    """W_L16.mtp: primitive (every neighbour an image of the centre), cubic2, an EMPTY configuration, a 16-atom replica, an
    isolated atom (K = 0), a compressed bcc cell (88 neighbours: three tiles)"""
    return [_cells.primitive_cell(), _cells.cubic2_cell(), _batch.empty_cell(), _design.replica16_cell(),
            _design.isolated_cell(), _design.compressed_cell()]


def batch2():
    """WRe_L20.mtp: the tilted 5-atom cell with two species (every i-j radial block in use)"""
    return [_cells.tilted5_cell(2)]


def fit_batch8():
    """eight small cells for the level-8 fit"""
    return [_cells.primitive_cell(), _cells.cubic2_cell(), _cells.tilted5_cell(1), _design.replica16_cell(5),
            _design.replica16_cell(6), _design.replica16_cell(7), _batch.sheared8_cell(1), _cells.cubic2_cell(seed=12)]


def fit_batch16():
    """cells for the level-16 refit: 135 energy + force rows and 30 virial rows over 117 columns"""
    return [_cells.primitive_cell(), _cells.cubic2_cell(), _cells.tilted5_cell(1), _design.replica16_cell(5),
            _batch.sheared8_cell(1), _design.replica16_cell(6)]


@functools.lru_cache(maxsize=None)
def _reference(fname, which):
    return _design.oracle_design(_oracle(fname), dict(batch1=batch1, batch2=batch2, fit16=fit_batch16)[which]())


def _host(d):
    return dict(energy=d["energy"].cpu().numpy(), force=d["force"].cpu().numpy(),
                virial=None if d["virial"] is None else d["virial"].cpu().numpy())


# ---- entries through the low-level call, on stars with exact neighbour counts ----------------------------------------------
def _design_rows_of_stars(fname, st, neigh=None, ctx=None):
    """Context.design_rows over a star system with d_owner = NULL (every atom is its own owner): dict(basis [stars, cols],
    force [nall, 3, cols], virial [stars, 6, cols]); ctx: another context than the shared one of the file"""
    import torch
    dev, stream = _device_stream()
    ctx = ctx or _ctx(fname)
    info = ctx.pot.info
    cols = info.species_count + info.alpha_scalar_count
    ld = cols + (cols & 1) + 2                               # (a leading dimension above the columns: the pad is zeroed)
    ctx.set_neighbors(st.ilist, st.first, st.neigh if neigh is None else neigh, st.nall)
    x_t = torch.from_numpy(st.x).to(dev)
    t_t = torch.from_numpy(st.types).to(dev)
    nrows = len(st.ilist)
    force = torch.zeros((3 * st.nall, ld), dtype=torch.float64, device=dev)
    basis = torch.full((nrows, ld), 7.0, dtype=torch.float64, device=dev)
    virial = torch.full((nrows, 6, ld), 7.0, dtype=torch.float64, device=dev)
    ctx.design_rows(0, nrows, x_t, t_t, force, st.nall, ld, basis_t=basis, virial_t=virial, stream=stream)
    ctx.synchronize(stream=stream)
    b, f, v = basis.cpu().numpy(), force.cpu().numpy(), virial.cpu().numpy()
    assert not b[:, cols:].any() and not f[:, cols:].any() and not v[:, :, cols:].any()
    return dict(basis=b[:, :cols], force=f[:, :cols].reshape(st.nall, 3, cols), virial=v[:, :, :cols])


def _check_stars(fname, st, got, label, orc=None):
    """per star and per column with the star's own scale (the rule of _stars.per_star_check): a three-tile star must not be
    able to hide a one-neighbour one; orc: another oracle than the shared one of the file"""
    want = _design.oracle_columns(orc or _oracle(fname), st.x, st.types, st.ilist, st.first, st.neigh)
    worst = 0.0
    bounds = list(st.start) + [st.nall]
    for s in range(len(st.ilist)):
        a, b, c = bounds[s], bounds[s + 1], st.ilist[s]
        ncol = want["energy"].size
        kinds = dict(basis=(got["basis"][s][None, :], want["eatom"][c][None, :]),
                     force=(got["force"][a:b].reshape(-1, ncol), want["f_all"][a:b].reshape(-1, ncol)),
                     virial=(got["virial"][s], want["vatom"][c]))
        for kind, (g, w) in kinds.items():                   # each kind with the column's maximum over its own rows
            ratio = _design.column_ratio(g, w)
            assert np.isfinite(g).all() and ratio <= 1.0, "%s %s: star %d (K, L) = %s misses its bound %.2f-fold" % (
                label, kind, s, st.KL[s], ratio)
        worst = max(worst, ratio)
    print("%s: worst error / bound over %d stars %.3e" % (label, len(st.ilist), worst))


@pytest.mark.gpu
def test_level8_stars_every_tile_and_row_length_edge():
    """K in {0, 1, 2, 31, 32, 33, 63, 64, 65} x L in {K, K + 1, 129}: tile and lane-grid edges in one launch, rows
    shuffled; in every star with K > 0 one entry sits at r^2 == r_c^2 bit-exact (inside) and, where the row lists atoms
    outside, one a representable step beyond (outside)"""
    rng = np.random.default_rng(21)
    KL = [(K, L) for K in (0, 1, 2, 31, 32, 33, 63, 64, 65) for L in (K, K + 1, 129)]
    st = _stars.stars(KL, rng, special="edge")
    assert _stars.counts(st) == KL
    st.neigh = _stars.shuffled_rows(st, rng)
    _check_stars("W_L8.mtp", st, _design_rows_of_stars("W_L8.mtp", st), "level 8 stars")


@pytest.mark.gpu
def test_level16_stars_with_leaf_moments():
    rng = np.random.default_rng(22)
    KL = [(K, L) for K in (0, 1, 32, 33, 65) for L in (K, K + 1, 129)]
    st = _stars.stars(KL, rng, special="edge")
    assert _stars.counts(st) == KL
    st.neigh = _stars.shuffled_rows(st, rng)
    _check_stars("W_L16.mtp", st, _design_rows_of_stars("W_L16.mtp", st), "level 16 stars")


@pytest.mark.gpu
def test_more_rows_than_workgroups_second_trips_of_the_grid_stride_loop():
    """8 CUs + 64 rows, the star set of the training kernel's test of the same name (tests/_train.grid_stride_KL): the
    launch has at most 8 workgroups per CU, so a workgroup that has done a three-tile row goes on to a K = 0 or one-tile row"""
    import torch
    rng = np.random.default_rng(23)
    KL = _train.grid_stride_KL(torch.cuda.get_device_properties(0).multi_processor_count, rng)
    st = _stars.stars(KL, rng)
    assert _stars.counts(st) == KL
    st.neigh = _stars.shuffled_rows(st, rng)
    _check_stars("W_L8.mtp", st, _design_rows_of_stars("W_L8.mtp", st), "grid stride, %d stars" % len(KL))


# ---- through md.design_cells: the owner fold and the batch -------------------------------------------------------------------
def _check_batch(got, want, what):
    e, f, v, natoms = want
    return _design.check_columns(got, dict(energy=e, force=f, virial=v), what)


@pytest.mark.gpu
def test_design_cells_level16_batch_against_the_oracle_columns():
    dev, _ = _device_stream()
    batch = batch1()
    d = md.design_cells(_ctx("W_L16.mtp"), batch, device=dev)
    got = _host(d)
    assert d["columns"] == 117 and list(d["natoms"]) == [1, 2, 0, 16, 1, 16]
    assert list(d["cfg_first"].cpu().numpy()) == [0, 1, 3, 3, 19, 20, 36]
    _check_batch(got, _reference("W_L16.mtp", "batch1"), "level 16 batch")
    # the 1-atom primitive cell: every neighbour is an image of the centre -- force rows exactly zero, the energy row the
    # basis values; an empty configuration: zero rows; the isolated atom: the species column is 1, everything else 0
    assert not got["force"][0:3].any() and got["energy"][0, 0] == 1.0 and got["energy"][0, 1:].all()
    assert not got["energy"][2].any() and not got["virial"][2].any()
    assert got["energy"][4, 0] == 1.0 and not got["energy"][4, 1:].any() and not got["force"][57:60].any() and not got["virial"][4].any()
    assert not got["force"][:, 0].any() and not got["virial"][:, :, 0].any()          # species columns of force and virial
    # the same matrices from a batch split into passes of one configuration
    split = _host(md.design_cells(_ctx("W_L16.mtp"), batch, max_atoms_per_pass=1, device=dev))
    _design.check_columns(split, got, "split against unsplit")


@pytest.mark.gpu
def test_design_cells_level20_two_species():
    dev, _ = _device_stream()
    d = md.design_cells(_ctx("WRe_L20.mtp"), batch2(), device=dev)
    assert d["columns"] == 462
    _check_batch(_host(d), _reference("WRe_L20.mtp", "batch2"), "level 20, two species")


@pytest.mark.gpu
@pytest.mark.parametrize("fname,which", [("W_L16.mtp", "batch1"), ("WRe_L20.mtp", "batch2")])
def test_design_rows_times_theta_is_what_evaluate_cells_returns(fname, which):
    """linearity end to end, independent of the oracle, with the tolerances of tests/test_batch_gpu.py"""
    dev, _ = _device_stream()
    batch = dict(batch1=batch1, batch2=batch2)[which]()
    ctx = _ctx(fname)
    got = _host(md.design_cells(ctx, batch, device=dev))
    res = md.evaluate_cells(ctx, batch, device=dev)
    theta = _theta0(fname)
    first = np.concatenate([[0], np.cumsum([len(p) for p, _, _ in batch])])
    for k, r in enumerate(res):
        n = len(batch[k][0])
        _batch.close((got["force"][3 * first[k]: 3 * first[k + 1]] @ theta).reshape(n, 3), r["f"], "forces of configuration %d" % k)
        _batch.close_energy(float(got["energy"][k] @ theta), r["energy"], n, "energy of configuration %d" % k)
        _batch.close(got["virial"][k] @ theta, r["virial"], "virial of configuration %d" % k, atol=1e-8)


# ---- fit_linear ----------------------------------------------------------------------------------------------------------------
def _check_labels(path, batch, labels):
    dev, _ = _device_stream()
    res = md.evaluate_cells(capi.Context(capi.Potential(path), 0), batch, device=dev)
    for k, (r, l) in enumerate(zip(res, labels)):
        _batch.close(r["f"], l["f"], "forces of configuration %d" % k)
        _batch.close_energy(r["energy"], l["energy"], len(l["f"]), "energy of configuration %d" % k)
        _batch.close(r["virial"], l["virial"], "virial of configuration %d" % k, atol=1e-8)


@pytest.mark.gpu
def test_fit_linear_recovers_the_level8_coefficients(tmp_path):
    """labels from W_L8.mtp itself on eight small cells, start from moment_coeffs perturbed by 10 %: full rank (cond 966
    measured on the CPU), so the written coefficients are the original's to 1e-9 (cond x the 1e-12 label noise, with margin)"""
    dev, _ = _device_stream()
    src = os.path.join(POT, "W_L8.mtp")
    t = capi.Potential(src).tables()
    rng = np.random.default_rng(31)
    start = _design.rewrite_coeffs(src, str(tmp_path / "start.mtp"), t["moment_coeffs"] * (1.0 + 0.1 * rng.uniform(-1, 1, 9)))
    batch = fit_batch8()
    labels = _design.oracle_labels(_oracle("W_L8.mtp"), batch)
    out = str(tmp_path / "fit.mtp")
    res = md.fit_linear(capi.Context(capi.Potential(start), 0), batch, labels, out_path=out, device=dev)
    print("level 8 fit: rank %d, rmse before %s, after %s" % (res["rank"], res["rmse_before"], res["rmse_after"]))
    assert res["rank"] == 10 and res["wrote"] == 0
    back = capi.Potential(out).tables()
    np.testing.assert_array_equal(back["moment_coeffs"], res["moment_coeffs"])
    err = max(np.abs(back["moment_coeffs"] - t["moment_coeffs"]).max(), np.abs(back["species_coeffs"] - t["species_coeffs"]).max())
    print("level 8 fit: largest coefficient error %.3e" % err)
    assert err <= 1e-9
    assert res["rmse_after"]["force"] < 1e-9 < res["rmse_before"]["force"]
    _check_labels(out, batch, labels)


def test_level16_refit_bound_on_the_oracle_built_matrix():
    """CPU: the same weighted solve on the matrix the ORACLE builds for the level-16 fit batch, labels from the potential
    itself.  Rank 116 of 117 (one exact dependency in the complete table); the refit from theta_0 moves no coefficient by
    more than 1e-6 -- this run prints the figure the GPU test's bound rests on."""
    e, f, v, natoms = _reference("W_L16.mtp", "fit16")
    labels = _design.oracle_labels(_oracle("W_L16.mtp"), fit_batch16())
    theta0 = _theta0("W_L16.mtp")
    res = md.solve_linear(e, f, v, natoms, labels, theta0)
    move = float(np.abs(res["theta"] - theta0).max())
    print("level 16 refit on the oracle's matrix: rank %d of %d, largest coefficient change %.3e, rmse after %s"
          % (res["rank"], len(theta0), move, res["rmse_after"]))
    assert res["rank"] < len(theta0)
    assert move <= 1e-6


@pytest.mark.gpu
def test_fit_linear_level16_refit_on_its_own_labels(tmp_path):
    dev, _ = _device_stream()
    batch = fit_batch16()
    labels = _design.oracle_labels(_oracle("W_L16.mtp"), batch)
    out = str(tmp_path / "refit.mtp")
    res = md.fit_linear(_ctx("W_L16.mtp"), batch, labels, out_path=out, device=dev)
    theta0 = _theta0("W_L16.mtp")
    move = float(np.abs(np.concatenate([res["species_coeffs"], res["moment_coeffs"]]) - theta0).max())
    print("level 16 refit: rank %d, largest coefficient change %.3e" % (res["rank"], move))
    assert res["rank"] < 117
    assert move <= 1e-6
    _check_labels(out, batch, labels)


# ---- error paths and untouched paths -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_design_error_paths():
    import torch
    dev, stream = _device_stream()
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    ctx = capi.Context(pot, 0)
    st = _stars.stars([(3, 4), (2, 2)], np.random.default_rng(5))
    x_t, t_t = torch.from_numpy(st.x).to(dev), torch.from_numpy(st.types).to(dev)
    force = torch.zeros((3 * st.nall, 12), dtype=torch.float64, device=dev)
    with pytest.raises(capi.MtpError) as ei:                                  # no list installed
        ctx.design_rows(0, 2, x_t, t_t, force, st.nall, 10, stream=stream)
    assert ei.value.code == -23
    ctx.set_neighbors(st.ilist, st.first, st.neigh, st.nall)
    for ld in (8, 11):                                                       # too small, odd
        with pytest.raises(capi.MtpError) as ei:
            ctx.design_rows(0, 2, x_t, t_t, force, st.nall, ld, stream=stream)
        assert ei.value.code == -20
    with pytest.raises(capi.MtpError) as ei:                                  # no force rows
        ctx.design_rows(0, 2, x_t, t_t, None, st.nall, 10, stream=stream)
    assert ei.value.code == -20
    with pytest.raises(capi.MtpError) as ei:                                  # rows outside the list
        ctx.design_rows(1, 2, x_t, t_t, force, st.nall, 10, stream=stream)
    assert ei.value.code == -20
    # a type outside the potential: reported at the synchronise, the message names the pass
    pos, cell, types = _cells.cubic2_cell()
    with pytest.raises(capi.MtpError, match="pass 2") as ei:
        md.design_cells(ctx, [_cells.primitive_cell(), (pos, cell, np.array([1, 2], dtype=np.int32))], max_atoms_per_pass=1, device=dev)
    assert ei.value.code == -22
    ok = md.design_cells(ctx, [_cells.primitive_cell()], device=dev)          # the flag was cleared
    assert ok["energy"].shape == (1, 10)
    with pytest.raises(ValueError, match="max_design_bytes"):
        md.design_cells(ctx, [_cells.cubic2_cell()], max_design_bytes=8 * 10 * (1 + 6 + 6 + 7 * 2) - 1, device=dev)
    assert md.design_cells(ctx, [_cells.cubic2_cell()], max_design_bytes=8 * 10 * (1 + 6 + 6 + 7 * 2), device=dev)["columns"] == 10


@pytest.mark.gpu
def test_a_design_call_leaves_the_force_plan_alone():
    """launch_info / plan_info / layout_mode of a context before and after its first design call, and of one that never
    makes one: the tangent kernel's table is uploaded lazily and shares nothing with the force kernel's plan"""
    import torch
    dev, stream = _device_stream()
    pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
    st = _stars.stars([(5, 6), (33, 40)], np.random.default_rng(6))
    a, b = capi.Context(pot, 0), capi.Context(pot, 0)
    for c in (a, b):
        c.set_neighbors(st.ilist, st.first, st.neigh, st.nall)
    before = (a.launch_info(), a.plan_info(), a.layout_mode())
    x_t, t_t = torch.from_numpy(st.x).to(dev), torch.from_numpy(st.types).to(dev)
    force = torch.zeros((3 * st.nall, 118), dtype=torch.float64, device=dev)
    a.design_rows(0, 2, x_t, t_t, force, st.nall, 118, stream=stream)
    a.synchronize(stream=stream)
    assert (a.launch_info(), a.plan_info(), a.layout_mode()) == before == (b.launch_info(), b.plan_info(), b.layout_mode())
    ra, rb = a.compute(st.x, st.types), b.compute(st.x, st.types)
    assert np.array_equal(ra["eatom"], rb["eatom"]) and abs(ra["f"] - rb["f"]).max() <= 1e-12 * max(1.0, abs(rb["f"]).max())
