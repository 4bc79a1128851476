"""The normal-equation refit on the device (csrc/mtp_normal.hip; capi.Normal, md.normal_cells, md.normal_from_design,
md.solve_normal, md.fit_linear(method="normal")).  The accumulate and fold kernels are judged exactly (tests/_normal.py:
integer arithmetic on the doubles' bits, the bound 4 m 2^-106 sum |b b|) and bit for bit against the numpy twin; the solve is
judged against the SVD path on the SAME device rows."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _batch  # noqa: E402
import _cells  # noqa: E402
import _design  # noqa: E402
import _normal  # noqa: E402
from lammps_mtp_kokkos_amd import capi, md  # noqa: E402
from lammps_mtp_kokkos_amd.driver import normal_twin  # noqa: E402

POT = _design.POT


def _device_stream():
    import torch
    dev = torch.device("cuda:0")
    return dev, capi.use_private_torch_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def _ctx(fname):
    return capi.Context(_design.handles(fname).pot, 0)


def _perturbed(fname):
    t = _design.handles(fname).tables
    return t["moment_coeffs"] * (1.0 + 0.1 * np.random.default_rng(31).uniform(-1, 1, len(t["moment_coeffs"])))


def _labels(fname, batch):
    """oracle labels; an empty configuration gets zeros of the right shapes (its rows are skipped)"""
    orc = _design.handles(fname).orc
    return [dict(energy=0.0, f=np.zeros((0, 3)), virial=np.zeros(6)) if len(c[0]) == 0 else _design.oracle_labels(orc, [c])[0]
            for c in batch]


def _within(got, want, theta0, what):
    """the solver bound of tests/test_normal_cpu.py: 1e-6 max(1, movement)"""
    diff, move = float(np.abs(got - want).max()), float(np.abs(want - theta0).max())
    print("%s: max|dtheta| %.3e, movement %.3e" % (what, diff, move))
    assert diff <= 1e-6 * max(1.0, move), what


# ---- 1: the kernels alone --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ncols", _normal.NCOLS)
def test_accumulate_against_exact_sums(ncols):
    import torch
    dev, st = _device_stream()
    sizes = capi.normal_sizes()
    S = sizes["slice"]
    nm = capi.Normal(ncols, 0)
    assert nm.info()["round_slices"] >= 3
    entries = _normal.sample_entries(ncols + 1)
    ld = ncols + _normal.PAD
    for nrows in _normal.nrows_cases(sizes["panel"], S):
        case = _normal.kernel_case(ncols, nrows)
        rows, scale, target = (torch.from_numpy(case[k]).to(dev) for k in ("rows", "scale", "target"))

        def run(cuts, slices=None):
            nm.clear(stream=st)
            if slices is not None:
                nm.set_round_slices(slices)
            for a, b in zip(cuts[:-1], cuts[1:]):
                nm.accumulate(1, b - a, ld, rows[a:], scale[a:], target[a:], stream=st)
            if slices is not None:
                nm.set_round_slices(full_round)
            return nm.get(stream=st)

        full_round = nm.info()["round_slices"]
        hi, lo, counts = run([0, nrows])
        B = _normal.scaled_rows(case)
        what = "%d columns, %d rows" % (ncols, nrows)
        assert list(counts) == [0, len(B), 0], what
        assert not hi[0].any() and not hi[2].any() and not lo[0].any() and not lo[2].any(), what
        worst = _normal.check_gram(hi[1], lo[1], B, entries, what)
        np.testing.assert_array_equal(hi[1], hi[1].T, err_msg=what)
        np.testing.assert_array_equal(lo[1], lo[1].T, err_msg=what)
        # the numpy twin, operation for operation
        thi, tlo, tcount = normal_twin(case["rows"][:nrows], case["scale"][:nrows], case["target"][:nrows], ncols, slice_rows=S)
        assert tcount == len(B) and np.array_equal(thi, hi[1]) and np.array_equal(tlo, lo[1]), what + ": not the twin's bits"
        # the same call again on a cleared state; a split at a multiple of the slice; several rounds: the same bits
        for name, args in (("again", ([0, nrows],)), ("split at a slice", ([0, min(S, nrows), nrows],)), ("rounds of one slice", ([0, nrows], 1))):
            h2, l2, c2 = run(*args)
            assert np.array_equal(h2, hi) and np.array_equal(l2, lo) and np.array_equal(c2, counts), "%s: %s differs" % (what, name)
        if nrows == 2 * S + sizes["panel"] + 3:                      # an arbitrary split: another sum order, the same bound
            h3, l3, c3 = run([0, nrows // 3, nrows])
            assert np.array_equal(c3, counts)
            print("%s: worst error / bound %.3e, split at %d %.3e"
                  % (what, worst, nrows // 3, _normal.check_gram(h3[1], l3[1], B, entries, what + " split")))


# ---- 2: the same rows, two solvers ------------------------------------------------------------------------------------------
def _two_solvers(d, labels, theta0, figure, what):
    state = md.normal_from_design(d, labels)
    got = md.solve_normal(state, theta0)
    want = md.solve_linear(d["energy"].cpu().numpy(), d["force"].cpu().numpy(), d["virial"].cpu().numpy(), d["natoms"], labels, theta0)
    diff = float(np.abs(got["theta"] - want["theta"]).max())
    print("%s: rank %d / %d, max|theta_normal - theta_svd| %.3e (CPU figure %.1e), dropped %d, rmse after %s"
          % (what, got["rank"], want["rank"], diff, figure, len(got["dropped_columns"]), got["rmse_after"]))
    assert got["rank"] == want["rank"]
    assert diff <= 100.0 * figure
    assert state.counts == dict(energy=len(labels), force=3 * int(d["natoms"].sum()), virial=6 * len(labels))


@pytest.mark.gpu
def test_same_rows_two_solvers_level16(tmp_path):
    import test_design_gpu as tdg
    dev, _ = _device_stream()
    src = os.path.join(POT, "W_L16.mtp")
    start = _design.rewrite_coeffs(src, str(tmp_path / "start.mtp"), _perturbed("W_L16.mtp"))
    ctx = capi.Context(capi.Potential(start), 0)
    batch = tdg.fit_batch16()
    d = md.design_cells(ctx, batch, device=dev)
    t = ctx.coeffs()
    _two_solvers(d, _labels("W_L16.mtp", batch), np.concatenate([t["species_coeffs"], t["moment_coeffs"]]),
                 _normal.CPU_THETA_FIGURE["W_L16 perturbed"], "W_L16 fit_batch16")


@pytest.mark.gpu
def test_same_rows_two_solvers_level20():
    import test_design_gpu as tdg
    dev, _ = _device_stream()
    batch = tdg.batch2()
    d = md.design_cells(_ctx("WRe_L20.mtp"), batch, device=dev)
    theta0 = np.concatenate([_design.handles("WRe_L20.mtp").tables["species_coeffs"], _perturbed("WRe_L20.mtp")])
    _two_solvers(d, _labels("WRe_L20.mtp", batch), theta0, _normal.CPU_THETA_FIGURE["WRe_L20 batch2"], "WRe_L20 batch2")


# ---- 3: normal_cells streams -------------------------------------------------------------------------------------------------
def _theta16():
    return np.concatenate([_design.handles("W_L16.mtp").tables["species_coeffs"], _perturbed("W_L16.mtp")])


@pytest.mark.gpu
def test_normal_cells_one_pass_or_one_atom_a_pass():
    import test_design_gpu as tdg
    dev, _ = _device_stream()
    batch = tdg.batch1()                  # the 1-atom cell, the EMPTY configuration, the isolated atom, the three-tile cell
    labels = _labels("W_L16.mtp", batch)
    ctx, theta0 = _ctx("W_L16.mtp"), _theta16()
    whole = md.normal_cells(ctx, batch, labels, device=dev)
    split = md.normal_cells(ctx, batch, labels, max_atoms_per_pass=1, device=dev)
    natoms = sum(len(c[0]) for c in batch)
    assert whole.counts == split.counts == dict(energy=len(batch) - 1, force=3 * natoms, virial=6 * (len(batch) - 1))
    a, b = md.solve_normal(whole, theta0), md.solve_normal(split, theta0)
    assert a["rank"] == b["rank"]
    _within(b["theta"], a["theta"], theta0, "batch1 one atom a pass against one pass")
    # ... and the same rows through design_cells
    c = md.solve_normal(md.normal_from_design(md.design_cells(ctx, batch, device=dev), labels), theta0)
    _within(c["theta"], a["theta"], theta0, "batch1 from the design matrix against one pass")


@pytest.mark.gpu
def test_normal_cells_fits_where_design_cells_refuses():
    dev, _ = _device_stream()
    batch = [_design.replica16_cell(300 + s) for s in range(40)]
    labels = _labels("W_L16.mtp", batch)
    ctx, theta0 = _ctx("W_L16.mtp"), _theta16()
    ld, ncfg, ntot = 118, 40, 640
    need = 8 * ld * (ncfg + 3 * ntot + 6 * ncfg + 7 * ntot)          # design_cells' formula, one pass
    with pytest.raises(ValueError, match="max_design_bytes"):
        md.design_cells(ctx, batch, max_design_bytes=need - 1, device=dev)
    small = md.normal_cells(ctx, batch, labels, max_bytes=need // 2, device=dev)
    info = small.normal.info()
    assert info["state_bytes"] + info["workspace_bytes"] < need // 2
    assert small.counts == dict(energy=ncfg, force=3 * ntot, virial=6 * ncfg)
    large = md.normal_cells(ctx, batch, labels, device=dev)
    a, b = md.solve_normal(large, theta0), md.solve_normal(small, theta0)
    assert a["rank"] == b["rank"]
    _within(b["theta"], a["theta"], theta0, "40 cells under half of design_cells' bytes")
    with pytest.raises(ValueError, match="max_bytes"):
        md.normal_cells(ctx, batch, labels, max_bytes=info["state_bytes"], device=dev)


# ---- 4: fit_linear(method="normal") end to end, the criteria of tests/test_design_gpu.py ----------------------------------------
def _check_labels(ctx, batch, labels):
    dev, _ = _device_stream()
    res = md.evaluate_cells(ctx, batch, device=dev)
    for k, (r, l) in enumerate(zip(res, labels)):
        _batch.close(r["f"], l["f"], "forces of configuration %d" % k)
        _batch.close_energy(r["energy"], l["energy"], len(l["f"]), "energy of configuration %d" % k)
        _batch.close(r["virial"], l["virial"], "virial of configuration %d" % k, atol=1e-8)


@pytest.mark.gpu
def test_fit_linear_normal_recovers_the_level8_coefficients(tmp_path):
    import test_design_gpu as tdg
    dev, _ = _device_stream()
    src = os.path.join(POT, "W_L8.mtp")
    t = capi.Potential(src).tables()
    rng = np.random.default_rng(31)
    start = _design.rewrite_coeffs(src, str(tmp_path / "start.mtp"), t["moment_coeffs"] * (1.0 + 0.1 * rng.uniform(-1, 1, 9)))
    batch = tdg.fit_batch8()
    labels = _labels("W_L8.mtp", batch)
    out = str(tmp_path / "fit.mtp")
    ctx = capi.Context(capi.Potential(start), 0)
    res = md.fit_linear(ctx, batch, labels, out_path=out, device=dev, method="normal", install=True)
    print("level 8 fit: rank %d, rmse before %s, after %s" % (res["rank"], res["rmse_before"], res["rmse_after"]))
    assert res["rank"] == 10 and res["wrote"] == 0 and len(res["dropped_columns"]) == 0
    back = capi.Potential(out).tables()
    np.testing.assert_array_equal(back["moment_coeffs"], res["moment_coeffs"])
    err = max(np.abs(back["moment_coeffs"] - t["moment_coeffs"]).max(), np.abs(back["species_coeffs"] - t["species_coeffs"]).max())
    print("level 8 fit: largest coefficient error %.3e" % err)
    assert err <= 1e-9
    assert res["rmse_after"]["force"] < 1e-9 < res["rmse_before"]["force"]
    _check_labels(capi.Context(capi.Potential(out), 0), batch, labels)
    _check_labels(ctx, batch, labels)                                  # install=True: the context evaluates the new coefficients
    np.testing.assert_array_equal(ctx.coeffs()["moment_coeffs"], res["moment_coeffs"])
    assert isinstance(res["state"], md.NormalState)
    with pytest.raises(ValueError, match="method"):
        md.fit_linear(ctx, batch, labels, device=dev, method="qr")
    with pytest.raises(ValueError, match="method"):
        md.fit_linear(ctx, batch, labels, device=dev, state=res["state"])


@pytest.mark.gpu
def test_fit_linear_normal_level16_refit_on_its_own_labels(tmp_path):
    import test_design_gpu as tdg
    dev, _ = _device_stream()
    batch = tdg.fit_batch16()
    labels = _labels("W_L16.mtp", batch)
    out = str(tmp_path / "refit.mtp")
    res = md.fit_linear(_ctx("W_L16.mtp"), batch, labels, out_path=out, device=dev, method="normal")
    t = _design.handles("W_L16.mtp").tables
    theta0 = np.concatenate([t["species_coeffs"], t["moment_coeffs"]])
    move = float(np.abs(np.concatenate([res["species_coeffs"], res["moment_coeffs"]]) - theta0).max())
    print("level 16 refit: rank %d, largest coefficient change %.3e, dropped %s" % (res["rank"], move, res["dropped_columns"]))
    assert res["rank"] < 117
    assert move <= 1e-6
    _check_labels(capi.Context(capi.Potential(out), 0), batch, labels)


# ---- 5: incremental rounds ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_saved_state_extended_by_new_configurations(tmp_path):
    import test_design_gpu as tdg
    dev, _ = _device_stream()
    batch = tdg.fit_batch16()
    labels = _labels("W_L16.mtp", batch)
    ctx, theta0 = capi.Context(capi.Potential(os.path.join(POT, "W_L16.mtp")), 0), _theta16()
    first = md.normal_cells(ctx, batch[:3], labels[:3], device=dev)
    path = str(tmp_path / "round1.npz")
    first.save(path)
    loaded = md.NormalState.load(path, dev)
    for x, y in zip(first.arrays(), loaded.arrays()):
        assert x.tobytes() == y.tobytes()
    assert loaded.fingerprint == first.fingerprint == md.design_fingerprint(ctx)
    both = md.normal_cells(ctx, batch[3:], labels[3:], state=loaded, device=dev)
    assert both is loaded
    once = md.normal_cells(ctx, batch, labels, device=dev)
    assert both.counts == once.counts
    a, b = md.solve_normal(once, theta0), md.solve_normal(both, theta0)
    assert a["rank"] == b["rank"]
    _within(b["theta"], a["theta"], theta0, "rounds A then B against A + B")
    # linear coefficients only: the state stays valid; a changed radial block: stale
    before = [x.copy() for x in both.arrays()]
    ctx.install_coeffs(moment_coeffs=a["theta"][1:])
    md.normal_cells(ctx, batch[:1], labels[:1], state=both, device=dev)
    assert both.counts["energy"] == once.counts["energy"] + 1
    both.normal.set(*before, stream=_device_stream()[1])
    ctx.install_coeffs(radial_coeffs=ctx.coeffs()["radial_coeffs"] * 1.001)
    with pytest.raises(ValueError, match="fingerprint"):
        md.normal_cells(ctx, batch[:1], labels[:1], state=both, device=dev)
    for x, y in zip(before, both.arrays()):
        assert x.tobytes() == y.tobytes()


# ---- 6: error paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_normal_error_paths():
    import torch
    dev, st = _device_stream()
    nm = capi.Normal(10, 0)
    rows = torch.ones((4, 12), dtype=torch.float64, device=dev)
    vec = torch.ones(4, dtype=torch.float64, device=dev)
    nm.accumulate(0, 4, 12, rows, vec, vec, stream=st)
    before = nm.get(stream=st)
    assert before[0][0, 3, 10] == 4.0 and list(before[2]) == [4, 0, 0]
    for kwargs in (dict(stream=None), dict(ld=9), dict(kind=3), dict(kind=-1), dict(nrows=-1), dict(rows=None), dict(scale=None)):
        a = dict(kind=0, nrows=4, ld=12, rows=rows, scale=vec, target=vec, stream=st)
        a.update(kwargs)
        with pytest.raises(capi.MtpError) as ei:
            nm.accumulate(a["kind"], a["nrows"], a["ld"], a["rows"], a["scale"], a["target"], stream=a["stream"])
        assert ei.value.code == -20, kwargs
    nm.accumulate(2, 0, 12, None, None, None, stream=st)                # nrows == 0 launches nothing
    for call in (lambda: nm.clear(stream=None), lambda: nm.get(stream=None), lambda: nm.set(*before, stream=None),
                 lambda: nm.set_round_slices(0), lambda: nm.set_round_slices(10 ** 6)):
        with pytest.raises(capi.MtpError) as ei:
            call()
        assert ei.value.code == -20
    with pytest.raises(capi.MtpError):
        capi.Normal(0, 0)
    after = nm.get(stream=st)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    # labels of the wrong shape, the wrong number of labels: ValueError before anything is launched
    ctx = _ctx("W_L8.mtp")
    cell = _cells.cubic2_cell()
    good = dict(energy=0.0, f=np.zeros((2, 3)), virial=np.zeros(6))
    state = md.normal_cells(ctx, [cell], [good], device=dev)
    kept = state.arrays()
    with pytest.raises(ValueError, match=r"\[2, 3\]"):
        md.normal_cells(ctx, [cell], [dict(good, f=np.zeros((3, 3)))], state=state, device=dev)
    with pytest.raises(ValueError, match="labels for"):
        md.normal_cells(ctx, [cell], [good, good], state=state, device=dev)
    for x, y in zip(kept, state.arrays()):
        assert x.tobytes() == y.tobytes()
    nm.clear(stream=st)
    assert not nm.get(stream=st)[0].any() and list(nm.get(stream=st)[2]) == [0, 0, 0]
