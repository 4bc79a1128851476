"""CPU checks of the linear refit (include/mtp_mi355x.h, "linear refit"): the numpy twin of the design-row kernel against
the oracle's unit-coefficient columns, the coefficient writer, the tangent kernel's host-side table, and both under the
sanitizers in a stand-alone program."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cells  # noqa: E402
import _design  # noqa: E402
import _tables  # noqa: E402
from _mutate import mutate_mtp  # noqa: E402
from lammps_mtp_kokkos_amd import capi, driver, mtpgen  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402

ROOT, POT = _design.ROOT, _design.POT
ALL_POTENTIALS = ["W_L8.mtp", "W_L16.mtp", "W_L16_nbh.almtp", "WRe_L20.mtp", "WRe_L10_cfg.almtp"]


def _twin_against_oracle(path, cell3, what):
    orc, pot = Oracle(path), capi.Potential(path)
    want, s = _design.oracle_cell_columns(orc, *cell3)
    got = driver.design_twin(pot.tables(), s)
    return _design.check_columns(got, want, what)


@pytest.mark.parametrize("fname,cell", [("W_L8.mtp", "primitive"), ("W_L8.mtp", "cubic2"), ("W_L8.mtp", "tilted5"),
                                        ("W_L16.mtp", "cubic2"), ("W_L16.mtp", "replica16"), ("WRe_L20.mtp", "tilted5")])
def test_design_twin_equals_the_oracle_columns(fname, cell):
    cells = dict(primitive=_cells.primitive_cell, cubic2=_cells.cubic2_cell, replica16=_design.replica16_cell,
                 tilted5=lambda: _cells.tilted5_cell(2 if fname.startswith("WRe") else 1))
    _twin_against_oracle(os.path.join(POT, fname), cells[cell](), "%s %s" % (fname, cell))


def test_design_twin_with_scaling_and_another_window(tmp_path):
    """scaling = 2.5, R = 6, window [1.9, 4.6]: a table of tests/_tables.py, two species"""
    tab, nfac = _tables.make_table([(0, 0), (1, 0), (0, 1), (1, 2), (0, 3)], seed=3)
    path = _tables.write(tab, nfac, str(tmp_path / "scaled.mtp"), species=2, R=6, scaling=2.5, min_dist=1.9, max_dist=4.6)
    assert capi.Potential(path).info.scaling == 2.5
    _twin_against_oracle(path, _cells.tilted5_cell(2), "scaled")


# ---- the tangent kernel's table ----------------------------------------------------------------------------------------
def _replay(pot, rng):
    """the table's level-ordered rows over an image with every moment stored, values AND tangents, against the file-order
    loop (pair_mtp.cpp:196-201) on random basics"""
    t, d = pot.tables(), pot.design_table()
    A, B, S = pot.info.alpha_moment_count, pot.info.alpha_index_basic_count, pot.info.alpha_scalar_count
    assert (d["A"], d["B"]) == (A, B) and d["level_offset"][0] == 0 and d["level_offset"][-1] == len(d["rows"])
    assert (np.diff(d["level_offset"]) >= 0).all() and (np.diff(d["level_offset"]) % 64 == 0).all()
    m0, g0 = rng.uniform(-1, 1, B), rng.uniform(-1, 1, B)
    m, g = np.zeros(A), np.zeros(A)
    m[:B], g[:B] = m0, g0
    for a0, a1, mu, a3 in t["alpha_index_times"]:
        m[a3] += mu * m[a0] * m[a1]
    for a0, a1, mu, a3 in t["alpha_index_times"]:                # tangents with the FINAL moments: the transpose of :221-233
        g[a3] += mu * (g[a0] * m[a1] + m[a0] * g[a1])
    # the table numbers the moments for the LDS banks; its basics are a permutation of the file's, named by their descriptors
    ab, pk = t["alpha_index_basic"], d["basic_pack"]
    where = {tuple(int(v) for v in q): k for k, q in enumerate(ab)}
    file_of = np.array([where[(int(v >> 20) & 15, int(v >> 8) & 15, int(v >> 12) & 15, int(v >> 16) & 15)] for v in pk])
    assert sorted(file_of) == list(range(B))
    M, G = np.zeros(A), np.zeros(A)
    M[:B], G[:B] = m0[file_of], g0[file_of]
    real = 0
    levels = [d["rows"][d["level_offset"][l]:d["level_offset"][l + 1]] for l in range(len(d["level_offset"]) - 1)]
    for rows in levels:
        add_m = np.zeros(A)                                      # all rows of a level read the state before it
        np.add.at(add_m, rows[:, 3], rows[:, 2] * M[rows[:, 0]] * M[rows[:, 1]])
        live = rows[rows[:, 2] != 0]                             # (padding rows have multiplicity 0: they add zero)
        assert not (set(live[:, 3]) & (set(live[:, 0]) | set(live[:, 1])))   # no row reads a target of its level
        M += add_m
        real += len(live)
    for rows in levels:                                          # the kernel's order: M complete, then the tangents
        add_g = np.zeros(A)
        np.add.at(add_g, rows[:, 3], rows[:, 2] * (G[rows[:, 0]] * M[rows[:, 1]] + M[rows[:, 0]] * G[rows[:, 1]]))
        G += add_g
    assert real <= len(t["alpha_index_times"]) <= len(d["rows"])
    mp = t["alpha_moment_mapping"]
    np.testing.assert_allclose(M[d["scalar_map"]], m[mp], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(G[d["scalar_map"]], g[mp], rtol=1e-12, atol=1e-13)
    # every moment has a slot: the scalar map covers [0, A) indices, and force_map drops all but the last scalar of a moment
    assert d["scalar_map"].min() >= 0 and d["scalar_map"].max() < A
    last = {int(v): k for k, v in enumerate(mp)}
    assert [int(v) for v in d["force_map"]] == [int(d["scalar_map"][k]) if last[int(mp[k])] == k else -1 for k in range(S)]
    return d


@pytest.mark.parametrize("fname", ALL_POTENTIALS)
def test_design_table_replays_the_file_order_loop(fname):
    _replay(capi.Potential(os.path.join(POT, fname)), np.random.default_rng(7))


def test_design_table_of_a_mutated_table(tmp_path):
    """a late row that still adds to a factor of never-read scalars, and two scalars on one moment (tests/_mutate.py)"""
    dst = str(tmp_path / "mutated.mtp")
    info = mutate_mtp(os.path.join(POT, "W_L16.mtp"), dst)
    assert info["leaves"] > 0
    d = _replay(capi.Potential(dst), np.random.default_rng(8))
    assert (d["force_map"] < 0).sum() == 1
    # ... and the twin, which drops that scalar's force columns, still agrees with the oracle's columns
    _twin_against_oracle(dst, _cells.cubic2_cell(), "mutated")


# ---- the coefficient writer -------------------------------------------------------------------------------------------
def _new_coeffs(pot, seed):
    rng = np.random.default_rng(seed)
    t = pot.tables()
    return t, t["species_coeffs"] + rng.normal(0, 1, len(t["species_coeffs"])), t["moment_coeffs"] * rng.uniform(0.5, 1.5, len(t["moment_coeffs"])) + 1e-3 * np.pi


@pytest.mark.parametrize("fname", ["W_L8.mtp", "W_L16.mtp", "WRe_L20.mtp"])
def test_write_coeffs_round_trips_bit_for_bit(tmp_path, fname):
    src, dst = os.path.join(POT, fname), str(tmp_path / "new.mtp")
    t, sp, mo = _new_coeffs(capi.Potential(src), 1)
    assert capi.write_coeffs(src, dst, mo, sp) == 0
    back, orc = capi.Potential(dst).tables(), Oracle(dst)
    np.testing.assert_array_equal(back["moment_coeffs"], mo)
    np.testing.assert_array_equal(back["species_coeffs"], sp)
    np.testing.assert_array_equal(orc.arr("linear_coeffs", len(mo)), mo)
    np.testing.assert_array_equal(orc.arr("species_coeffs", len(sp)), sp)
    for k in ("alpha_index_basic", "alpha_index_times", "alpha_moment_mapping", "radial_coeffs", "scaling", "min_cutoff", "max_cutoff"):
        np.testing.assert_array_equal(back[k], t[k])
    # every other byte is the source's
    a, b = open(src, "rb").read(), open(dst, "rb").read()
    cut = a.index(b"species_coeffs")
    assert a[:cut] == b[:cut] and not [f for f in os.listdir(tmp_path) if ".tmp" in f]
    # species_coeffs = None keeps that line
    assert capi.write_coeffs(src, dst, mo) == 0
    back = capi.Potential(dst).tables()
    np.testing.assert_array_equal(back["species_coeffs"], t["species_coeffs"])
    np.testing.assert_array_equal(back["moment_coeffs"], mo)


@pytest.mark.parametrize("fname", ["W_L16_nbh.almtp", "WRe_L10_cfg.almtp"])
def test_write_coeffs_leaves_the_selection_tail_out(tmp_path, fname):
    src, dst = os.path.join(POT, fname), str(tmp_path / "new.mtp")
    t, sp, mo = _new_coeffs(capi.Potential(src), 2)
    assert capi.write_coeffs(src, dst, mo, sp) == capi.WROTE_WITHOUT_SELECTION == 1
    data = open(dst, "rb").read()
    assert b"#MVS" not in data and data.endswith(b"}\n")
    back = capi.Potential(dst).tables()
    np.testing.assert_array_equal(back["moment_coeffs"], mo)
    np.testing.assert_array_equal(back["radial_coeffs"], t["radial_coeffs"])
    with pytest.raises(capi.MtpError) as ei:
        capi.Potential(dst, selection=True)
    assert ei.value.code == -8


def test_write_coeffs_refuses_wrong_counts_and_non_finite_numbers(tmp_path):
    src, dst = os.path.join(POT, "W_L8.mtp"), str(tmp_path / "new.mtp")
    t, sp, mo = _new_coeffs(capi.Potential(src), 3)
    for bad_mo, bad_sp in ((mo[:-1], sp), (np.append(mo, 0.0), sp), (mo, np.append(sp, 0.0))):
        with pytest.raises(capi.MtpError) as ei:
            capi.write_coeffs(src, dst, bad_mo, bad_sp)
        assert ei.value.code == -20
    for bad in (np.nan, np.inf, -np.inf):
        m2, s2 = mo.copy(), sp.copy()
        m2[3] = bad
        with pytest.raises(capi.MtpError) as ei:
            capi.write_coeffs(src, dst, m2, sp)
        assert ei.value.code == -20
        s2[0] = bad
        with pytest.raises(capi.MtpError) as ei:
            capi.write_coeffs(src, dst, mo, s2)
        assert ei.value.code == -20
    assert not os.path.exists(dst) and not os.listdir(tmp_path)
    with pytest.raises(capi.MtpError) as ei:
        capi.write_coeffs(str(tmp_path / "nope.mtp"), dst, mo, sp)
    assert ei.value.code == -2


def test_write_coeffs_on_the_level_4_short_line_buffer(tmp_path):
    """DESIGN.md section 2, finding (1): at level 4 the reader's line buffer (T * 32 + 20 = 52 characters) is shorter than
    the moment_coeffs line, so a reader gets the line back in pieces.  The writer reads its file back before the rename:
    either the new numbers come back bit for bit, or the call is refused with MTP_ERR_LIMIT and nothing is written."""
    src, dst = str(tmp_path / "l4.mtp"), str(tmp_path / "new.mtp")
    mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(4), 1, 5), src)
    pot = capi.Potential(src)
    assert pot.info.alpha_index_times_count * 32 + 20 == 52 and pot.info.alpha_scalar_count == 2
    t, sp, mo = _new_coeffs(pot, 4)
    try:
        rc = capi.write_coeffs(src, dst, mo, sp)
    except capi.MtpError as e:
        assert e.code == -24 and not os.path.exists(dst) and sorted(os.listdir(tmp_path)) == ["l4.mtp"]
    else:
        assert rc == 0
        np.testing.assert_array_equal(capi.Potential(dst).tables()["moment_coeffs"], mo)
        np.testing.assert_array_equal(Oracle(dst).arr("linear_coeffs", len(mo)), mo)


# ---- both under ASan + UBSan, in a program of their own ------------------------------------------------------------------
@pytest.fixture(scope="module")
def san_exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "host"), "san_design"])
    return os.path.join(ROOT, "tests", "cpp", "test_design_san")


@pytest.mark.parametrize("fname", ALL_POTENTIALS)
def test_writer_and_table_builder_run_clean_under_sanitizers(san_exe, tmp_path, fname):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_exe, os.path.join(POT, fname), str(tmp_path / "out.mtp")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "OK" and int(words[1]) == (1 if fname.endswith(".almtp") else 0), r.stdout
    assert float(words[2]) < 1e-12, r.stdout           # the table's replay against the file-order loop
