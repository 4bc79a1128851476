"""MaxVol selection on the device (mtp_maxvol_select, md.select_cells) against the numpy twin (driver.maxvol_select_numpy).

Tolerance rule (tests/_maxvol.py, bound): 100 x the twin's own drift on the same pool, floor 1e-12, scaled by
max(1, max |G|) -- a figure of the twin, never of the device.  Swap sequences are not compared: real pools hold near-ties,
so the twin REPLAYS the device's logged swaps and checks every pivot against its own matrix (tests/_maxvol.py, replay)."""
import functools
import os
import tempfile

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi
from lammps_mtp_kokkos_amd.driver import periodic_system_cell

import _batch
import _cells
import _maxvol
from _cells import POT, LIST_CUTOFF

_TMP = tempfile.TemporaryDirectory(prefix="maxvol_")


def _device_stream():
    import torch
    dev = torch.device("cuda:0")
    return dev, capi.use_private_torch_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def _ctx(C):
    """a context whose potential carries _maxvol.random_state(C)"""
    S, W = _maxvol.random_state(C)
    path = _maxvol.selection_file(os.path.join(_TMP.name, "state%d.almtp" % C), C, S, W)
    pot = capi.Potential(path, selection=True)
    assert np.array_equal(pot.active_set(), S) and np.array_equal(pot.tables()["inverse_active_set"], W)
    return capi.Context(pot, 0), S, W


def _select(ctx, V, threshold, ld=None, **kw):
    import torch
    dev, st = _device_stream()
    V = np.ascontiguousarray(V, dtype=np.float64)
    if ld is None:
        rows = torch.from_numpy(V).to(dev)
    else:                                                    # rows ld doubles apart, the space between them poisoned
        full = torch.full((len(V), ld), 1e300, dtype=torch.float64, device=dev)
        full[:, : V.shape[1]] = torch.from_numpy(V).to(dev)
        rows = full[:, : V.shape[1]]
    return ctx.maxvol_select(rows, threshold, stream=st, **kw)


def _check_result(res, V, S, W, threshold, tol, converged=True):
    """everything a finished selection must satisfy; returns the twin's replayed (S', W', G)"""
    C = S.shape[0]
    assert res["converged"] == converged and res["nswaps"] == len(res["swaps"]) <= 4 * C
    assert all(0 <= i < len(V) and 0 <= j < C for i, j, _ in res["swaps"])            # never a padding column
    St, Wt, Gt = _maxvol.replay(V, S, W, res["swaps"], threshold, tol)
    S1, W1 = res["active_set"], res["inverse_active_set"]
    src = res["slot_source"]
    assert np.array_equal(src, _maxvol.slot_source_of(res["swaps"], C))
    for j in range(C):                                       # column provenance, bit for bit
        assert np.array_equal(S1[:, j], S[:, j] if src[j] < 0 else V[src[j], :C]), j
    assert np.array_equal(S1, St)
    err_w, err_i = np.abs(W1 - Wt).max(), np.abs(W1 @ S1 - np.eye(C)).max()
    grades = np.abs(np.linalg.solve(S1, V[:, :C].T)) if len(V) else np.zeros((C, 0))
    top = float(grades.max()) if grades.size else 0.0
    gain = float(sum(np.log(abs(p)) for _, _, p in res["swaps"]))
    det = np.linalg.slogdet(S1)[1] - np.linalg.slogdet(S)[1]
    print("C = %d N = %d threshold %.7g: %d swaps, tol %.3e, |W' - twin| %.3e, |W'S' - I| %.3e, max grade %.15g reported "
          "%.15g, gain %.12g slogdet %.12g" % (C, len(V), threshold, res["nswaps"], tol, err_w, err_i, top,
                                               res["max_grade_after"], gain, det))
    assert err_w <= tol and err_i <= tol
    assert abs(res["max_grade_after"] - top) <= tol
    if converged:
        assert top <= threshold * (1.0 + tol)
    assert abs(res["log_volume_gain"] - gain) <= 1e-12 * max(1.0, abs(gain)) and abs(gain - det) <= 1e-9 * max(1.0, abs(det))
    return St, Wt, Gt


@pytest.mark.gpu
@pytest.mark.parametrize("C,N", [(26, 1), (26, 300), (115, 1000), (149, 257), (149, 4096)])
@pytest.mark.parametrize("threshold", [2.0, 1.0 + 1e-6])
def test_random_pools_against_the_replaying_twin(C, N, threshold):
    """cpad 32, 128 and 160; a one-row pool; pools of one and of many workgroups"""
    ctx, S, W = _ctx(C)
    r = _maxvol.twin_run(C, N, threshold)
    V = r["V"]
    drift = max(float(np.abs(r["G"] - V @ r["W1"].T).max()), float(np.abs(r["W1"] @ r["S1"] - np.eye(C)).max()))
    tol = max(100.0 * drift, 1e-12) * max(1.0, float(np.abs(V @ r["W1"].T).max()))
    res = _select(ctx, V, threshold)
    _check_result(res, V, S, W, threshold, tol)
    assert N == 1 or res["nswaps"] > 0


@pytest.mark.gpu
def test_the_row_at_a_time_path_above_cpad_256():
    """C = 622 (WRe_L20.mtp, cpad 624): maxvol_update<.., 0>, which reads r[j] from memory ahead of the row's stores"""
    C, N = 622, 97
    ctx, S, W = _ctx(C)
    V = _maxvol.random_pool(C, N)
    tol = _maxvol.bound(V, S, W, 2.0, 4 * C)
    res = _select(ctx, V, 2.0)
    _check_result(res, V, S, W, 2.0, tol)
    assert res["nswaps"] > 0 and max(j for _, j, _ in res["swaps"]) >= 512


def _quiet_pool(C, N, S, seed=3):
    """rows well inside the span of the active set: every grade below 0.2"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, size=(N, C)) * (0.2 / C)) @ S.T


@pytest.mark.gpu
def test_empty_and_quiet_pools_return_the_inputs_bit_for_bit():
    import torch
    C = 26
    ctx, S, W = _ctx(C)
    dev, st = _device_stream()
    for rows in (torch.zeros((0, C), dtype=torch.float64, device=dev), None):
        res = ctx.maxvol_select(rows, 1.1, stream=st) if rows is not None else _select(ctx, _quiet_pool(C, 300, S), 1.1)
        assert res["converged"] and res["nswaps"] == 0 and res["swaps"] == [] and res["log_volume_gain"] == 0.0
        assert np.array_equal(res["active_set"], S) and np.array_equal(res["inverse_active_set"], W)
        assert (res["slot_source"] == -1).all()
    V = _quiet_pool(C, 300, S)
    assert abs(res["max_grade_after"] - np.abs(V @ W.T).max()) <= 1e-12 and 0.0 < res["max_grade_after"] < 0.2


@pytest.mark.gpu
def test_a_copy_of_an_active_set_column_grades_one_and_is_never_swapped():
    C = 26
    ctx, S, W = _ctx(C)
    V = _quiet_pool(C, 70, S)
    V[33] = S[:, 9]
    res = _select(ctx, V, 1.0 + 1e-6)
    tol = _maxvol.bound(V, S, W, 1.0 + 1e-6, 4 * C)
    assert res["nswaps"] == 0 and res["converged"] and abs(res["max_grade_after"] - 1.0) <= tol
    # ... and in a pool that does swap.  Two rows that lean on columns 3 and 17 enter those slots; the copy's grades are
    # exactly e_9, so r[3] = r[17] = 0 and neither update touches its row: slot 9 stays and the copy still grades one
    V = _quiet_pool(C, 70, S)
    V[12] += 50.0 * S[:, 3]
    V[51] += 50.0 * S[:, 17]
    V[33] = S[:, 9]
    res = _select(ctx, V, 1.1)
    tol = _maxvol.bound(V, S, W, 1.1, 4 * C)
    _check_result(res, V, S, W, 1.1, tol)
    assert sorted(sw[:2] for sw in res["swaps"]) == [(12, 3), (51, 17)]
    assert res["slot_source"][9] == -1 and 33 not in [i for i, _, _ in res["swaps"]]
    assert abs(np.abs(res["inverse_active_set"] @ V[33]).max() - 1.0) <= tol


@pytest.mark.gpu
def test_bit_identical_rows_resolve_to_the_lower_row():
    C = 26
    ctx, S, W = _ctx(C)
    V = _maxvol.random_pool(C, 300)
    i0, j0 = divmod(int(np.argmax(np.abs(V @ W.T))), C)
    hi = 299 if i0 != 299 else 298
    lo, hi = min(i0, hi), max(i0, hi)
    V[lo] = V[hi] = V[i0].copy()                              # the global maximum, twice
    res = _select(ctx, V, 1.1)
    tol = _maxvol.bound(V, S, W, 1.1, 4 * C)
    _check_result(res, V, S, W, 1.1, tol)
    assert res["swaps"][0][:2] == (lo, j0)
    inside = False                                           # while lo sits in the set its twin grades one and never enters
    for i, j, _ in res["swaps"]:
        assert not (inside and i == hi)
        inside = (i == lo) if j == j0 else inside
    # a pool where lo certainly stays: quiet rows and the maximum twice.  One swap, and the twin row ends with grade one
    V = _quiet_pool(C, 300, S)
    V[41] = V[207] = 50.0 * S[:, 11] + V[41]
    res = _select(ctx, V, 1.1)
    tol = _maxvol.bound(V, S, W, 1.1, 4 * C)
    _check_result(res, V, S, W, 1.1, tol)
    assert [sw[:2] for sw in res["swaps"]] == [(41, 11)] and res["slot_source"][11] == 41
    assert abs(np.abs(res["inverse_active_set"] @ V[207]).max() - 1.0) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("C,N,row,col,ld", [(26, 300, 299, 4, None), (26, 300, 17, 25, None), (149, 1030, 1029, 148, None),
                                           (26, 300, 299, 25, 48), (149, 257, 0, 148, 200)])
def test_maximum_in_the_last_row_or_the_last_column_and_rows_wider_than_cpad(C, N, row, col, ld):
    ctx, S, W = _ctx(C)
    V = _quiet_pool(C, N, S)
    V[row] = 50.0 * S[:, col] + V[row]
    res = _select(ctx, V, 1.1, ld=ld)
    tol = _maxvol.bound(V, S, W, 1.1, 4 * C)
    _check_result(res, V, S, W, 1.1, tol)
    assert res["swaps"][0][:2] == (row, col) and abs(res["swaps"][0][2] - 50.0) < 1.0


@pytest.mark.gpu
def test_max_swaps_stops_early_with_the_state_reached():
    C = 26
    ctx, S, W = _ctx(C)
    V = _maxvol.random_pool(C, 300)
    tol = _maxvol.bound(V, S, W, 1.1, 4 * C)
    res = _select(ctx, V, 1.1, max_swaps=3)
    assert res["nswaps"] == 3 and not res["converged"]
    St, Wt, Gt = _check_result(res, V, S, W, 1.1, tol, converged=False)
    assert np.abs(res["inverse_active_set"] - Wt).max() <= tol and res["max_grade_after"] > 1.1   # the twin's state after those three
    none = _select(ctx, V, 1.1, max_swaps=0)
    assert none["nswaps"] == 0 and not none["converged"] and np.array_equal(none["inverse_active_set"], W)


@pytest.mark.gpu
def test_refresh_every_swap_and_never_give_sets_with_the_same_properties():
    C = 115
    ctx, S, W = _ctx(C)
    r = _maxvol.twin_run(C, 1000, 2.0)
    V = r["V"]
    tol = _maxvol.bound(V, S, W, 2.0, 4 * C)
    gains = []
    for refresh in (1, 10 ** 6):
        res = _select(ctx, V, 2.0, refresh=refresh)
        _check_result(res, V, S, W, 2.0, tol)
        gains.append(res["log_volume_gain"])
    assert min(gains) > 0.0


@pytest.mark.gpu
def test_non_finite_candidates_and_bad_arguments_are_refused():
    import torch
    C = 26
    ctx, S, W = _ctx(C)
    dev, st = _device_stream()
    for bad in (np.nan, np.inf):
        V = _maxvol.random_pool(C, 300)
        V[123, 7] = bad
        with pytest.raises(capi.MtpError) as ei:
            _select(ctx, V, 1.1)
        assert ei.value.code == -20
        res = ei.value.result                                # the state before the offending pivot
        assert res["nswaps"] == 0 and not res["converged"] and np.array_equal(res["inverse_active_set"], W)
        assert np.array_equal(res["active_set"], S)
    good = torch.from_numpy(_maxvol.random_pool(C, 300)).to(dev)
    for kw, rows in ((dict(threshold=0.5), good), (dict(threshold=float("nan")), good), (dict(threshold=1.1, max_swaps=-1), good),
                     (dict(threshold=1.1, refresh=0), good), (dict(threshold=1.1), good[:, : C - 1])):
        with pytest.raises(capi.MtpError) as ei:
            ctx.maxvol_select(rows, stream=st, **kw)
        assert ei.value.code == -20 and ei.value.result["nswaps"] == 0
    plain = capi.Context(capi.Potential(os.path.join(POT, "W_L8.mtp")), 0)       # no selection block
    with pytest.raises(capi.MtpError) as ei:
        plain.maxvol_select(good, 1.1, stream=st)
    assert ei.value.code == -23
    with pytest.raises(capi.MtpError) as ei:
        ctx.candidates()                                     # no grade call yet
    assert ei.value.code == -23
    _check_result(ctx.maxvol_select(good, 1.1, stream=st), good.cpu().numpy(), S, W, 1.1,
                  _maxvol.bound(good.cpu().numpy(), S, W, 1.1, 4 * C))           # the context is still good


def _nbh_cells():
    return [_cells.tilted5_cell(1), _batch.sheared8_cell(), _batch.replica54_cell(), _batch.carved(23), _batch.carved(40)]


@pytest.mark.gpu
def test_select_cells_neighbourhood_mode_end_to_end(tmp_path):
    from lammps_mtp_kokkos_amd.md import evaluate_cells, select_cells
    from oracle.pyoracle import Oracle
    src = os.path.join(POT, "W_L16_nbh.almtp")
    pot = capi.Potential(src, selection=True)
    ctx = capi.Context(pot, 0)
    C = pot.info.coeff_count
    S, W = pot.active_set(), pot.tables()["inverse_active_set"]
    batch = _nbh_cells()
    first = np.concatenate([[0], np.cumsum([len(p) for p, _, _ in batch])])
    out = str(tmp_path / "selected.almtp")
    before = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    sel = select_cells(ctx, batch, threshold=1.1, out_path=out, list_cutoff=LIST_CUTOFF)
    assert sel["converged"] and 0 < sel["nswaps"] <= 4 * C
    assert np.array_equal(sel["grade_before"], [r["max_grade"] for r in before])
    owners = sorted({s[0] for s in sel["slot_source"] if s is not None})
    assert sel["selected"] == owners and len(sel["slot_source"]) == C
    for j, s in enumerate(sel["slot_source"]):
        assert s is not None or np.array_equal(sel["active_set"][:, j], S[:, j])
        assert s is None or 0 <= s[1] < len(batch[s[0]][0])
    # the written file, reloaded
    new_pot = capi.Potential(out, selection=True)
    assert np.array_equal(new_pot.active_set(), sel["active_set"])
    assert np.array_equal(new_pot.tables()["inverse_active_set"], sel["inverse_active_set"])
    new_ctx = capi.Context(new_pot, 0)
    got = evaluate_cells(new_ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    n = int(first[-1])
    pool = new_ctx.candidates()[:n, :C].cpu().numpy()         # the per-atom candidate vectors, read back from the device
    assert n == 130 and np.isfinite(pool).all()
    tol = _maxvol.bound(pool, S, W, 1.1, 4 * C)
    _check_result(dict(sel, slot_source=np.array([-1 if s is None else first[s[0]] + s[1] for s in sel["slot_source"]])),
                  pool, S, W, 1.1, tol)
    want = np.abs(pool @ sel["inverse_active_set"].T).max(1)
    grades = np.concatenate([r["grades"] for r in got])
    print("grades after the reload: max %.15g, against numpy W' c: max abs err %.3e (tol %.3e)" % (
        grades.max(), np.abs(grades - want).max(), tol))
    assert np.abs(grades - want).max() <= tol and grades.max() <= 1.1 * (1.0 + tol)
    assert abs(sel["max_grade_after"] - grades.max()) <= tol
    orc = Oracle(out, selection=True)
    for k, ((pos, cell, types), r) in enumerate(zip(batch, got)):
        s = periodic_system_cell(pos, cell, types, LIST_CUTOFF)
        ow = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=s.nlocal)
        _batch.close(r["grades"], ow["grades"][: s.nlocal], "grades of configuration %d on the written file" % k, atol=1e-9, rtol=1e-9)
    # every atom now in the set grades one
    for s in sel["slot_source"]:
        if s is not None:
            assert abs(got[s[0]]["grades"][s[1]] - 1.0) <= tol
    with pytest.raises(ValueError, match="max_pool_bytes"):
        select_cells(ctx, batch, list_cutoff=LIST_CUTOFF, max_pool_bytes=129 * 160 * 8)


@pytest.mark.gpu
def test_select_cells_configuration_mode_end_to_end(tmp_path, monkeypatch):
    from lammps_mtp_kokkos_amd.md import evaluate_cells, select_cells
    src = os.path.join(POT, "WRe_L10_cfg.almtp")
    pot = capi.Potential(src, selection=True)
    ctx = capi.Context(pot, 0)
    C = pot.info.coeff_count
    S, W = pot.active_set(), pot.tables()["inverse_active_set"]
    batch = _batch.mixed_batch(2)
    empty = [k for k, (p, _, _) in enumerate(batch) if len(p) == 0]
    assert empty == [3]
    pools = []
    real = ctx.maxvol_select
    monkeypatch.setattr(ctx, "maxvol_select", lambda rows, *a, **kw: (pools.append(rows.cpu().numpy().copy()), real(rows, *a, **kw))[1])
    out = str(tmp_path / "selected.almtp")
    before = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    threshold = 1.1
    sel = select_cells(ctx, batch, threshold=threshold, out_path=out, list_cutoff=LIST_CUTOFF)
    pool = pools[0][:, :C]
    assert pool.shape == (6, C) and not pools[0][3].any() and all(pool[k].any() for k in range(6) if k != 3)
    assert not pools[0][:, C:].any()
    grade_of_rows = np.abs(pool @ W.T).max(1)                 # a row's grade is the configuration grade the library reports
    assert np.abs(grade_of_rows - [r["cfg_grade"] for r in before]).max() <= 1e-9 * max(1.0, grade_of_rows.max())
    assert np.array_equal(sel["grade_before"], [r["cfg_grade"] for r in before])
    tol = _maxvol.bound(pool, S, W, threshold, 4 * C)
    assert sel["converged"] and 3 not in sel["selected"]
    # (the file's set is 2 I + noise, no real vector: every real configuration grades far above any threshold near one)
    assert grade_of_rows[[0, 1, 2, 4, 5]].min() > threshold and sel["nswaps"] > 0
    _check_result(dict(sel, slot_source=np.array([-1 if s is None else s for s in sel["slot_source"]])), pool, S, W, threshold, tol)
    assert sel["selected"] == sorted({s for s in sel["slot_source"] if s is not None})
    new_ctx = capi.Context(capi.Potential(out, selection=True), 0)
    got = evaluate_cells(new_ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    after = np.array([r["cfg_grade"] for r in got])
    print("configuration grades before", grade_of_rows, "after", after, "tol %.3e" % tol)
    assert after.max() <= threshold * (1.0 + tol) and after[3] == 0.0
    assert np.abs(after - np.abs(pool @ sel["inverse_active_set"].T).max(1)).max() <= tol


@pytest.mark.gpu
def test_select_cells_leaves_the_context_and_evaluate_cells_unchanged():
    from lammps_mtp_kokkos_amd.md import evaluate_cells, select_cells
    ctx = capi.Context(capi.Potential(os.path.join(POT, "W_L16_nbh.almtp"), selection=True), 0)
    batch = _batch.mixed_batch()
    before = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    sel = select_cells(ctx, batch, threshold=1.1, list_cutoff=LIST_CUTOFF)
    assert sel["converged"]
    after = evaluate_cells(ctx, batch, list_cutoff=LIST_CUTOFF, grades=True)
    for a, b in zip(before, after):
        assert np.array_equal(a["grades"], b["grades"]) and a["max_grade"] == b["max_grade"]
