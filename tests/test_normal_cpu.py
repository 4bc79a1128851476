"""The normal-equation refit on the CPU (csrc/mtp_dd.hpp, csrc/mtp_normal.cpp, driver.normal_twin, md.solve_normal): the
double-double arithmetic judged exactly, the numpy twin of the kernels on the shapes of the GPU test, and the solver against
the SVD path (md.solve_linear) on oracle-built matrices.  The device kernels are judged in tests/test_normal_gpu.py."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _design  # noqa: E402
import _normal  # noqa: E402
from lammps_mtp_kokkos_amd import capi, md  # noqa: E402
from lammps_mtp_kokkos_amd.driver import normal_twin  # noqa: E402

ROOT = _design.ROOT
POT = _design.POT


# ---- 1, 2: the arithmetic under ASan + UBSan, in a program of its own -----------------------------------------------------
@pytest.fixture(scope="module")
def san_exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "host"), "san_normal"])
    return os.path.join(ROOT, "tests", "cpp", "test_normal_san")


def _run_san(san_exe, tmp_path, scale, rows, target):
    """the program's Gram matrix (hi, lo [n, n]) and factor outputs for rows [m, ncols]"""
    m, ncols = rows.shape
    with open(tmp_path / "matrix.txt", "w") as f:
        f.write("%d %d\n" % (m, ncols))
        for i in range(m):
            f.write(" ".join(float(v).hex() for v in [scale[i], *rows[i], target[i]]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_exe, str(tmp_path / "matrix.txt")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "GRAM %d" % (ncols + 1) and lines[-1] == "OK", r.stdout[-500:]
    n = ncols + 1
    pairs = np.array([[float.fromhex(w) for w in l.split()] for l in lines[1: 1 + n * n]])
    at = 1 + n * n
    rank, ndropped = (int(w) for w in lines[at].split()[1:])
    nums = lambda l: np.array([float.fromhex(w) for w in l.split()])
    R = np.array([nums(l) for l in lines[at + 1: at + 1 + rank]]).reshape(rank, ncols)
    q, order, dropped, ratios = (lines[at + 1 + rank + k] for k in range(4))
    return dict(hi=pairs[:, 0].reshape(n, n), lo=pairs[:, 1].reshape(n, n), rank=rank, ndropped=ndropped, R=R, q=nums(q),
                order=[int(w) for w in order.split()], dropped=[int(w) for w in dropped.split()], ratios=nums(ratios),
                quadratic=float.fromhex(lines[at + 5 + rank].split()[1]))


def test_integer_inputs_give_the_exact_sum_under_sanitizers(san_exe, tmp_path):
    """integers below 2^20 times powers of two: every product and every partial sum fits 106 bits, so hi + lo is the sum"""
    rng = np.random.default_rng(3)
    m, ncols = 200, 6
    rows = np.ldexp(rng.integers(-2 ** 20, 2 ** 20, (m, ncols)).astype(np.float64), rng.integers(-5, 6, (m, ncols)))
    target = np.ldexp(rng.integers(-2 ** 20, 2 ** 20, m).astype(np.float64), rng.integers(-5, 6, m))
    scale = np.ldexp(1.0, rng.integers(-2, 3, m))
    got = _run_san(san_exe, tmp_path, scale, rows, target)
    B = scale[:, None] * np.concatenate([rows, target[:, None]], axis=1)
    assert np.abs(B.T @ B).max() > 2.0 ** 53                       # (more than fp64 holds: lo is needed)
    for err, _ in _normal.gram_errors(got["hi"], got["lo"], B, _normal.sample_entries(ncols + 1)):
        assert err == 0
    np.testing.assert_array_equal(got["hi"], got["hi"].T)
    np.testing.assert_array_equal(got["lo"], got["lo"].T)


def test_general_inputs_meet_the_bound_and_plain_fp64_misses_it(san_exe, tmp_path):
    """entries spanning 2^-20 ... 2^30 with full mantissas, every tenth row skipped (NaN): the program's pairs are inside
    4 m 2^-106 sum |b b|; a plain fp64 B^T B of the same rows misses that bound by many orders, so neither a kernel nor a
    twin that silently lost lo could pass; the factor reproduces the Gram matrix"""
    case = _normal.kernel_case(10, 300, seed=4)
    rows, scale, target = case["rows"][:300, :10], case["scale"][:300], case["target"][:300]
    got = _run_san(san_exe, tmp_path, scale, rows, target)
    B = _normal.scaled_rows(case)
    entries = _normal.sample_entries(11)
    worst = _normal.check_gram(got["hi"], got["lo"], B, entries, "sanitizer build")
    plain = B.T @ B
    miss = max(float(err / bound) for err, bound in _normal.gram_errors(plain, np.zeros_like(plain), B, entries))
    print("double-double: worst error / bound %.3e; plain fp64: %.3e" % (worst, miss))
    assert miss > 1e9
    # the factor: R^T R = G on the columns, R^T q = G[:, target], all columns kept
    assert got["rank"] == 10 and got["ndropped"] == 0 and sorted(got["order"]) == list(range(10))
    G = got["hi"] + got["lo"]
    scale_g = np.sqrt(np.outer(np.diag(G), np.diag(G)))
    assert (np.abs(got["R"].T @ got["R"] - G[:10, :10]) <= 1e-13 * scale_g[:10, :10]).all()
    assert (np.abs(got["R"].T @ got["q"] - G[:10, 10]) <= 1e-13 * scale_g[:10, 10]).all()
    assert got["quadratic"] == pytest.approx(G[10, 10], rel=1e-15)


# ---- 3: the numpy twin on the shapes of the GPU test --------------------------------------------------------------------
@pytest.mark.parametrize("ncols", _normal.NCOLS)
def test_twin_meets_the_bound_on_the_shapes_of_the_gpu_test(ncols):
    sizes = capi.normal_sizes()
    entries = _normal.sample_entries(ncols + 1)
    for nrows in _normal.nrows_cases(sizes["panel"], sizes["slice"]):
        case = _normal.kernel_case(ncols, nrows)
        hi, lo, count = normal_twin(case["rows"][:nrows], case["scale"][:nrows], case["target"][:nrows], ncols,
                                    slice_rows=sizes["slice"])
        B = _normal.scaled_rows(case)
        assert count == len(B)
        worst = _normal.check_gram(hi, lo, B, entries, "twin, %d columns, %d rows" % (ncols, nrows))
        np.testing.assert_array_equal(hi, hi.T)
        np.testing.assert_array_equal(lo, lo.T)
    print("%d columns: worst error / bound at the largest size %.3e" % (ncols, worst))


def test_twin_without_lo_misses_the_bound():
    case = _normal.kernel_case(10, 257)
    hi, lo, _ = normal_twin(case["rows"][:257], case["scale"][:257], case["target"][:257], 10)
    B = _normal.scaled_rows(case)
    with pytest.raises(AssertionError, match="misses"):
        _normal.check_gram(hi, np.zeros_like(lo), B, _normal.sample_entries(11), "hi alone")


# ---- 4: the solver against the SVD path on oracle-built matrices -----------------------------------------------------------
def _theta(fname, perturbed):
    t = _design.handles(fname).tables
    mo = t["moment_coeffs"]
    if perturbed:
        mo = mo * (1.0 + 0.1 * np.random.default_rng(31).uniform(-1, 1, len(mo)))
    return np.concatenate([t["species_coeffs"], mo])


SOLVER_CASES = {                    # name -> (potential, batch of _normal.oracle_matrices, start perturbed by 10 %)
    "W_L8 perturbed": ("W_L8.mtp", "fit8", True),
    "W_L16 own labels": ("W_L16.mtp", "fit16", False),
    "W_L16 perturbed": ("W_L16.mtp", "fit16", True),
    "W_L16 37 configurations": ("W_L16.mtp", "batch37", True),
    "WRe_L20 8 tilted cells": ("WRe_L20.mtp", "tilted8", True),
    "WRe_L20 batch2": ("WRe_L20.mtp", "batch2", True),
}


def _solver_inputs(name):
    import test_design_gpu as tdg
    fname, which, perturbed = SOLVER_CASES[name]
    e, f, v, natoms = _normal.oracle_matrices(fname, which)
    batch = dict(fit8=tdg.fit_batch8, fit16=tdg.fit_batch16, batch37=_normal.batch37, tilted8=lambda: _normal.tilted_batch(8),
                 batch2=tdg.batch2)[which]()
    labels = _design.oracle_labels(_design.handles(fname).orc, batch)
    return e, f, v, natoms, labels, _theta(fname, perturbed)


@pytest.mark.parametrize("name", sorted(SOLVER_CASES))
def test_solver_against_the_svd_path(name):
    e, f, v, natoms, labels, theta0 = _solver_inputs(name)
    want = md.solve_linear(e, f, v, natoms, labels, theta0)
    got = md.solve_normal(_normal.twin_state(e, f, v, natoms, labels), theta0)
    cols, rank = len(theta0), got["rank"]
    kept, refused = got["pivot_ratios"][:cols - len(got["dropped_columns"])], got["pivot_ratios"][cols - len(got["dropped_columns"]):]
    diff = float(np.abs(got["theta"] - want["theta"]).max())
    move = float(np.abs(want["theta"] - theta0).max())
    print("%s: rank %d / %d of %d, max|theta_normal - theta_svd| %.3e, movement %.3e (normal %.3e), smallest kept pivot ratio "
          "2^%.1f, largest refused 2^%.1f, rmse after %s (svd %s)"
          % (name, rank, want["rank"], cols, diff, move, float(np.abs(got["theta"] - theta0).max()), np.log2(kept.min()),
             np.log2(max(refused.max(), 2.0 ** -1000)) if len(refused) else -np.inf, got["rmse_after"], want["rmse_after"]))
    assert rank == want["rank"]
    assert (len(got["dropped_columns"]) > 0) == (rank < cols)
    np.testing.assert_allclose(got["singular_values"][:rank], want["singular_values"][:rank], rtol=1e-6)
    assert kept.min() >= 2.0 ** -60
    assert len(refused) == 0 or refused.max() <= 2.0 ** -90
    assert diff <= 1e-6 * max(1.0, move)
    if name == "W_L16 own labels":
        assert float(np.abs(got["theta"] - theta0).max()) <= 1e-6
    for kind in ("energy", "force", "virial"):                     # 5: rmse_before is solve_linear's
        if want["rmse_before"][kind] > 1e-6:
            assert got["rmse_before"][kind] == pytest.approx(want["rmse_before"][kind], rel=1e-9)


# ---- 5: invariances ------------------------------------------------------------------------------------------------------------
def test_weights_at_solve_time_equal_weights_on_the_rows():
    e, f, v, natoms, labels, theta0 = _solver_inputs("W_L16 perturbed")
    w = (1.0, 0.01, 0.001)
    late = md.solve_normal(_normal.twin_state(e, f, v, natoms, labels), theta0, weights=w)
    early = md.solve_normal(_normal.twin_state(e, f, v, natoms, labels, weights=w), theta0, weights=(1.0, 1.0, 1.0))
    diff, move = float(np.abs(late["theta"] - early["theta"]).max()), float(np.abs(late["theta"] - theta0).max())
    print("weights late against early: max|dtheta| %.3e, movement %.3e" % (diff, move))
    assert late["rank"] == early["rank"]
    assert diff <= 1e-6 * max(1.0, move)


def test_a_state_accumulated_in_two_halves_is_the_state_of_the_whole():
    e, f, v, natoms, labels, _ = _solver_inputs("W_L16 perturbed")
    whole = _normal.twin_state(e, f, v, natoms, labels)
    split = _normal.twin_state(e, f, v, natoms, labels, halves=100)             # (no multiple of the slice: another sum order)
    _, _, (f_scale, f_target), _ = md._normal_labels(labels, natoms)
    B = f_scale[:, None] * np.concatenate([f, f_target[:, None]], axis=1)
    entries = _normal.sample_entries(B.shape[1])
    for name, st in (("whole", whole), ("halves", split)):
        print("%s: worst error / bound %.3e" % (name, _normal.check_gram(st[0][1], st[1][1], B, entries, name)))
    np.testing.assert_array_equal(whole[2], split[2])
    cut = _normal.twin_state(e, f, v, natoms, labels, halves=256)               # at a slice boundary: the same bits
    np.testing.assert_array_equal(cut[0], whole[0])
    np.testing.assert_array_equal(cut[1], whole[1])


def test_save_and_load_are_bit_equal(tmp_path):
    rng = np.random.default_rng(8)
    hi, lo = _normal.wide_values(rng, (3, 5, 5)), _normal.wide_values(rng, (3, 5, 5)) * 2.0 ** -60
    path = str(tmp_path / "state.npz")
    md.NormalState.write_arrays(path, hi, lo, [3, 2 ** 40, 0], "abc")
    back = md.NormalState.read_arrays(path)
    assert back[0].tobytes() == hi.tobytes() and back[1].tobytes() == lo.tobytes()
    assert list(back[2]) == [3, 2 ** 40, 0] and back[3] == "abc"
    md.NormalState.write_arrays(path, hi, lo, [0, 0, 0], None)
    assert md.NormalState.read_arrays(path)[3] is None


def test_a_changed_fingerprint_raises():
    """the fingerprint follows the radial block, the tables and the list cutoff, not the linear coefficients; a state with
    another one is refused"""
    pot = capi.Potential(os.path.join(POT, "W_L8.mtp"))
    t = pot.tables()
    ctx = SimpleNamespace(pot=pot, coeffs=lambda: dict(radial_coeffs=t["radial_coeffs"], moment_coeffs=t["moment_coeffs"] * 2.0))
    moved = SimpleNamespace(pot=pot, coeffs=lambda: dict(radial_coeffs=t["radial_coeffs"] * (1.0 + 1e-15)))
    other = SimpleNamespace(pot=capi.Potential(os.path.join(POT, "W_L16.mtp")), coeffs=lambda: dict(radial_coeffs=t["radial_coeffs"]))
    fp = md.design_fingerprint(ctx)
    assert fp == md.design_fingerprint(SimpleNamespace(pot=pot, coeffs=lambda: dict(radial_coeffs=t["radial_coeffs"].copy())))
    assert len({fp, md.design_fingerprint(moved), md.design_fingerprint(other), md.design_fingerprint(ctx, list_cutoff=6.0)}) == 4
    state = SimpleNamespace(ncols=10, fingerprint=fp)
    assert md._normal_state(state, 10, fp, None, 0, "test") is state
    for ncols, f in ((10, md.design_fingerprint(moved)), (11, fp), (10, None)):
        with pytest.raises(ValueError, match="fingerprint"):
            md._normal_state(state, ncols, f, None, 0, "test")


def test_solver_refusals():
    G = np.zeros((3, 3, 3))
    G[0] = np.eye(3)
    with pytest.raises(capi.MtpError) as ei:
        capi.normal_factor(G, np.zeros_like(G), (-1.0, 0.0, 0.0), np.zeros(2))
    assert ei.value.code == -20
    bad = G.copy()
    bad[0, 1, 1] = -1.0
    for hi in (bad, np.where(G == 1.0, np.nan, G)):
        with pytest.raises(capi.MtpError) as ei:
            capi.normal_factor(hi, np.zeros_like(G), (1.0, 0.0, 0.0), np.zeros(2))
        assert ei.value.code == -20
    with pytest.raises(ValueError, match="no labelled rows"):
        md.solve_normal((G, np.zeros_like(G), [0, 0, 0]), np.zeros(2))
    assert capi.build_flags() == ""
