"""Shared by the normal-equation tests (tests/test_normal_cpu.py, tests/test_normal_gpu.py): inputs of the accumulate
kernel, the exact judge of a double-double Gram matrix (integer arithmetic on the doubles' own bits, compared as
fractions.Fraction), and the batches of the solver tests with their oracle-built matrices.

The judge's bound for entry (j, k) of m rows is 4 m 2^-106 sum_i |b_ij b_ik|: dd_mac keeps the sum's and the product's
rounding errors exactly and adds them into lo with plain additions, two per row, each rounding at 2^-53 of a lo that is
itself bounded by 2^-53 of the partial sums; the factor 4 is the margin on those 2 m roundings and the final folds."""
import functools
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cells  # noqa: E402
import _design  # noqa: E402

NCOLS = (1, 10, 62, 63, 64, 117, 130)          # augmented 2, 11, 63, 64, 65, 118, 131: both sides of one and two tiles
PAD = 3                                        # ld = ncols + PAD, NaN in the padding
TAIL = 2                                       # NaN rows behind nrows
SAMPLE = 2000                                  # entries judged above 64 columns

# max |theta_normal - theta_svd| that tests/test_normal_cpu.py::test_solver_against_the_svd_path prints for these batches
# (twin-accumulated states of oracle-built matrices, the C++ solver); DESIGN.md 5.3.5 quotes them, and the GPU test of the
# same rows allows 100 x these
CPU_THETA_FIGURE = {"W_L16 perturbed": 4.9e-12, "WRe_L20 batch2": 2.4e-15}


def nrows_cases(panel, slice_rows):
    return (0, 1, panel - 1, panel, panel + 1, slice_rows - 1, slice_rows, slice_rows + 1, 2 * slice_rows + panel + 3)


def wide_values(rng, shape):
    """doubles with full 53-bit mantissas and magnitudes spanning 2^-20 ... 2^30, either sign"""
    return np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-20, 30, shape)) * rng.choice([-1.0, 1.0], shape)


def kernel_case(ncols, nrows, seed=0):
    """dict(rows [nrows + TAIL, ncols + PAD], scale, target [nrows + TAIL], ncols, nrows): wide_values everywhere that is
    read; NaN in the padding columns, in the rows behind nrows and in EVERY entry (target included) of the rows whose scale
    is 0 -- every tenth row"""
    rng = np.random.default_rng([seed, ncols, nrows])
    rows = wide_values(rng, (nrows + TAIL, ncols + PAD))
    target = wide_values(rng, nrows + TAIL)
    scale = rng.uniform(0.5, 2.0, nrows + TAIL)
    scale[9::10] = 0.0
    rows[:, ncols:] = np.nan
    rows[scale == 0.0] = np.nan
    target[scale == 0.0] = np.nan
    rows[nrows:], target[nrows:], scale[nrows:] = np.nan, np.nan, np.nan
    return dict(rows=rows, scale=scale, target=target, ncols=ncols, nrows=nrows)


def scaled_rows(case, begin=0, end=None):
    """B of the rows [begin, end) that enter: fl(scale * [rows[:, :ncols] | target]), ONE multiply"""
    end = case["nrows"] if end is None else end
    keep = np.flatnonzero(case["scale"][begin:end] != 0.0) + begin
    a = np.concatenate([case["rows"][keep, :case["ncols"]], case["target"][keep, None]], axis=1)
    return case["scale"][keep, None] * a


def to_integers(B):
    """(object array of Python ints, K) with B = ints / 2^K exactly"""
    flat = [float(x).as_integer_ratio() for x in np.asarray(B, dtype=np.float64).reshape(-1)]
    K = max([q.bit_length() - 1 for _, q in flat], default=0)
    ints = np.array([p * ((1 << K) // q) for p, q in flat], dtype=object).reshape(np.shape(B))
    return ints, K


def sample_entries(n, seed=1):
    """all (j, k) of an [n, n] matrix up to 65 columns, a fixed random sample of SAMPLE entries above"""
    if n <= 65:
        return [(j, k) for j in range(n) for k in range(n)]
    rng = np.random.default_rng(seed)
    return [(int(j), int(k)) for j, k in zip(rng.integers(0, n, SAMPLE), rng.integers(0, n, SAMPLE))]


def gram_errors(hi, lo, B, entries, terms=None):
    """per entry (|hi + lo - exact|, bound = 4 m 2^-106 sum_i |b_ij b_ik|) as Fractions; `terms` overrides m"""
    ints, K = to_integers(B)
    m = len(B) if terms is None else terms
    mags = np.abs(ints)
    out = []
    for j, k in entries:
        exact = Fraction(int((ints[:, j] * ints[:, k]).sum()) if len(B) else 0, 1 << (2 * K))
        total = Fraction(int((mags[:, j] * mags[:, k]).sum()) if len(B) else 0, 1 << (2 * K))
        got = Fraction(float(hi[j, k])) + Fraction(float(lo[j, k]))
        out.append((abs(got - exact), 4 * m * total / (1 << 106)))
    return out


def check_gram(hi, lo, B, entries, what, terms=None):
    """the bound on every entry; returns the worst error / bound"""
    assert np.isfinite(hi).all() and np.isfinite(lo).all(), what
    worst = 0.0
    for (j, k), (err, bound) in zip(entries, gram_errors(hi, lo, B, entries, terms)):
        assert err <= bound, "%s: entry (%d, %d) misses 4 m 2^-106 sum|b b| %.3g-fold" % (what, j, k, float(err / bound))
        worst = max(worst, float(err / bound) if bound else 0.0)
    return worst


def jittered(cell_fn, seed, sigma=0.05):
    pos, cell, types = cell_fn()
    return pos + np.random.default_rng(seed).normal(0.0, sigma, pos.shape), cell, types


def batch37():
    """fit_batch16 of test_design_gpu.py, 30 jittered 16-atom cells and the compressed cell: 1891 rows over 117 columns"""
    from test_design_gpu import fit_batch16
    return fit_batch16() + [_design.replica16_cell(100 + s) for s in range(30)] + [_design.compressed_cell()]


def tilted_batch(count):
    """`count` jittered copies of the two-species tilted 5-atom cell (22 rows each; WRe_L20.mtp has 462 columns)"""
    return [jittered(lambda: _cells.tilted5_cell(2), 200 + s) for s in range(count)]


@functools.lru_cache(maxsize=None)
def oracle_matrices(fname, which):
    """(energy, force, virial, natoms) of a named batch from the oracle's columns: built once, shared, never written to"""
    import test_design_gpu as tdg
    batch = dict(fit8=tdg.fit_batch8, fit16=tdg.fit_batch16, batch37=batch37, tilted8=lambda: tilted_batch(8),
                 batch2=tdg.batch2)[which]()
    if which == "fit16":
        return tdg._reference(fname, "fit16")
    return _design.oracle_design(_design.handles(fname).orc, batch)


def twin_state(energy, force, virial, natoms, labels, weights=None, halves=None):
    """the state (hi [3, n, n], lo [3, n, n], counts [3]) the device would hold for these matrices: md._normal_labels for
    scale and target, driver.normal_twin per kind.  weights: sqrt(w_k) multiplied into the scales BEFORE accumulation (the
    invariance test); halves = r: every kind accumulated as rows [0, r) then [r, end)."""
    from lammps_mtp_kokkos_amd import md
    from lammps_mtp_kokkos_amd.driver import normal_twin
    ncols = energy.shape[1]
    _, e_l, f_l, v_l = md._normal_labels(labels, np.asarray(natoms, dtype=np.int64))
    hi, lo, counts = np.zeros((3, ncols + 1, ncols + 1)), np.zeros((3, ncols + 1, ncols + 1)), np.zeros(3, dtype=np.int64)
    for k, (rows, (scale, target)) in enumerate(((energy, e_l), (force, f_l), (virial.reshape(-1, ncols), v_l))):
        if weights is not None:
            scale = scale * np.sqrt(weights[k])
        cuts = [0, len(scale)] if halves is None else [0, min(halves, len(scale)), len(scale)]
        st = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            st = normal_twin(rows[a:b], scale[a:b], target[a:b], ncols, state=st)
        hi[k], lo[k], counts[k] = st
    return hi, lo, counts
