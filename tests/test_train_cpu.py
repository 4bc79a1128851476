"""The training gradient without a GPU: the numpy twin of the training kernel (driver.train_twin) against the CPU oracle,
the writer of all coefficients (capi.write_all_coeffs) and the training table (capi.Potential.train_table).

The judge of the twin's gradient rows is the reference algorithm itself: Richardson-extrapolated central differences of the
oracle's scalar with one coefficient changed through its Model pointers (tests/_train.py).  Bound: |twin - fd| <= 1e-9
max |gradient|, the floor of the finite difference (it disagrees with itself between its last two extrapolations by up to
a few 1e-12 of that scale), not of the twin.  Worst ratios measured, |twin - fd| / max |gradient|:
W_L8 3.4e-12, WRe_L10_cfg 3.8e-13, W_L16 6.2e-13, WRe_L20 3.9e-15, scaling 2.5 1.9e-13, three tiles 8.7e-13, K = 0 2.7e-13,
1-atom cell 3.8e-12: none above 1e-10.  Star by star (list row k is not atom k): W_L8 5.1e-12, with an entry on the cutoff
2.3e-12, five species 1.0e-11, three species R = 9 with an entry on the cutoff 3.2e-12."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _batch  # noqa: E402
import _cells  # noqa: E402
import _design  # noqa: E402
import _mutate  # noqa: E402
import _stars  # noqa: E402
import _tables  # noqa: E402
import _train  # noqa: E402
from lammps_mtp_kokkos_amd import capi, mtpgen  # noqa: E402
from lammps_mtp_kokkos_amd.driver import design_twin, periodic_system_cell, train_twin  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402

ROOT = _design.ROOT
POT = _design.POT
ALL_POTENTIALS = ["W_L8.mtp", "W_L16.mtp", "W_L16_nbh.almtp", "WRe_L10_cfg.almtp", "WRe_L20.mtp"]


@functools.lru_cache(maxsize=None)
def _pot(path):
    return capi.Potential(path)


def _random_types(cell3, seed):
    pos, cell, types = cell3
    return pos, cell, (1 + (np.random.default_rng(seed).random(len(pos)) < 0.4)).astype(np.int32)


def _scaled_potential(tmp):
    path = os.path.join(tmp, "scaled.mtp")
    mtpgen.write_mtp(mtpgen.random_potential(mtpgen.level8_template(), 1, 4242, 2.0, 5.0, 8, 2.5), path)
    return path


# (label, potential, cell, radial columns sampled or None for all C columns)
FD_CASES = [
    ("W_L8 all columns", "W_L8.mtp", _design.replica16_cell, None),
    ("WRe_L10_cfg random types all columns", "WRe_L10_cfg.almtp", lambda: _random_types(_design.replica16_cell(), 4), None),
    ("W_L16 sampled", "W_L16.mtp", _design.replica16_cell, 24),
    ("WRe_L20 two species sampled", "WRe_L20.mtp", lambda: _random_types(_design.replica16_cell(), 4), 24),
    ("scaling 2.5", None, _design.replica16_cell, None),
    ("three tiles", "W_L8.mtp", _design.compressed_cell, None),
    ("K = 0", "W_L8.mtp", _design.isolated_cell, None),
    ("1-atom cell", "W_L8.mtp", _cells.primitive_cell, None),
]


@pytest.mark.parametrize("label,fname,cell,nsample", FD_CASES, ids=[c[0] for c in FD_CASES])
def test_twin_gradient_against_the_oracles_richardson_finite_difference(tmp_path, label, fname, cell, nsample):
    path = os.path.join(POT, fname) if fname else _scaled_potential(str(tmp_path))
    orc = Oracle(path)
    tables = _pot(path).tables() if fname else capi.Potential(path).tables()
    if not fname:
        assert tables["scaling"] == 2.5
    s = periodic_system_cell(*cell(), _cells.LIST_CUTOFF)
    ebar, fbar, vbar = _train.cotangents(s.nlocal, 3)
    tw = train_twin(tables, s, None, ebar, fbar, vbar)
    grad = tw["rows"].sum(0)
    nrad, Sp, S = _train.sizes(orc)
    assert len(grad) == nrad + Sp + S
    cols = list(range(len(grad))) if nsample is None else _train.sample_columns(orc, nsample)
    fd, floor = _train.fd_gradient(orc, s, ebar, fbar, vbar, cols)
    scale = np.abs(grad).max()
    ratio = np.abs(grad[cols] - fd).max() / scale
    print("%s: %d columns, worst |twin - fd| / max|grad| = %.3e (finite-difference floor %.3e)" % (label, len(cols), ratio, floor / scale))
    assert ratio <= 1e-9
    if label == "K = 0":                                     # ebar in the species column and nothing else
        assert np.count_nonzero(tw["rows"]) == 1 and tw["rows"][0, nrad] == ebar[0]
    if label == "1-atom cell":                               # every neighbour an image of the centre
        only_f = train_twin(tables, s, None, None, fbar, None)["rows"]
        only_v = train_twin(tables, s, None, None, None, vbar)["rows"]
        assert not only_f.any() and np.abs(only_v).max() > 1e-6


@pytest.mark.parametrize("fname,cell", [("W_L16.mtp", _design.replica16_cell), ("WRe_L20.mtp", lambda: _cells.tilted5_cell(2)),
                                        ("W_L8.mtp", _design.compressed_cell)])
def test_twin_value_is_the_oracle_at_the_files_and_at_a_perturbed_theta(fname, cell):
    path = os.path.join(POT, fname)
    orc = Oracle(path)
    tables = _pot(path).tables()
    s = periodic_system_cell(*cell(), _cells.LIST_CUTOFF)
    theta0 = _train.get_theta(orc)
    np.testing.assert_array_equal(theta0, _pot(path).theta())
    for what, theta in (("file", theta0), ("perturbed", theta0 * (1.0 + 0.05 * np.random.default_rng(2).normal(size=len(theta0))))):
        try:
            _train.set_theta(orc, theta)
            want = _train.oracle_value(orc, s)
        finally:
            _train.set_theta(orc, theta0)
        got = train_twin(tables, s, theta)
        _batch.close(got["eatom"], want["eatom"], "%s %s eatom" % (fname, what), atol=1e-10)
        _batch.close(got["force"], want["force"], "%s %s force" % (fname, what))
        _batch.close(got["vatom"], want["vatom"], "%s %s vatom" % (fname, what), atol=1e-8)


# ---- stars: list row k is not atom k, neighbour types missing from a row, an entry on the cutoff ---------------------------
def _w8(tmp):
    return os.path.join(POT, "W_L8.mtp")


def _five_species(tmp):
    path = os.path.join(tmp, "five.mtp")
    mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(6), 5, 4242), path)
    return path


def _nine_radial(tmp):
    path = os.path.join(tmp, "nine.mtp")
    mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(8), 3, 7, 1.7, 5.5, 9, 0.37), path)
    return path


STAR_FD_KL = [(1, 1), (1, 2), (2, 3), (33, 40), (65, 129)]
STAR_FD_CASES = [("W_L8 plain", _w8, None), ("W_L8 edge", _w8, "edge"), ("5 species level 6", _five_species, None),
                 ("3 species R = 9 edge", _nine_radial, "edge")]
# the hand-made tables of tests/_tables.CENTRE_TABLES (Mu up to 16, rank 11, sparse slots), and one of them with an entry on
# the cutoff.  Worst ratios measured: mu6 9.1e-12, mu8 1.1e-11, mu9 8.5e-12 (edge 1.7e-11), mu13_gaps 5.8e-12, mu16_sp3
# 1.2e-11, mu16_sp2_nbh 5.8e-12, rank11 1.1e-11
STAR_FD_CASES += [(name, lambda tmp, name=name: _design.handles(name).path, None) for name in sorted(_tables.CENTRE_TABLES)]
STAR_FD_CASES += [("mu9 edge", lambda tmp: _design.handles("mu9").path, "edge")]


@pytest.mark.parametrize("label,make,special", STAR_FD_CASES, ids=[c[0] for c in STAR_FD_CASES])
def test_twin_rows_of_stars_against_the_oracles_finite_difference_star_by_star(tmp_path, label, make, special):
    """row k of the twin against the finite difference of the oracle's scalar with the cotangents of star k ONLY, at a
    perturbed theta; |twin - fd| <= 1e-9 max |row|.  Worst measured 1.1e-11."""
    path = make(str(tmp_path))
    orc = Oracle(path)
    tables = capi.Potential(path).tables()
    st = _train.star_set(tables, STAR_FD_KL, 61, special)
    s = _train.star_system(st)
    theta0 = _train.get_theta(orc)
    theta = theta0 * (1.0 + 0.05 * np.random.default_rng(2).normal(size=len(theta0)))
    ebar, fbar, vbar = _train.row_cotangents(st, 8)
    rows = train_twin(tables, s, theta, _train.padded_rows(st, ebar), fbar, _train.padded_rows(st, vbar))["rows"][:len(st.ilist)]
    cols = list(range(len(theta))) if len(theta) < 40 else _train.sample_columns(orc, 24)
    if label.split()[0] in _tables.CENTRE_TABLES and len(theta) >= 40:
        # the sample may miss what the table is there for: one column of EVERY radial function (pair 1-1) as well, those
        # without a basic (their columns are zero) included
        Mu, R = orc.m.radial_func_count, orc.m.radial_basis_size
        cols = sorted(set(cols) | set(mu * R + mu % R for mu in range(Mu)))
    worst = 0.0
    try:
        _train.set_theta(orc, theta)
        for k in range(len(st.ilist)):
            mine = st.sid == k
            e_k, v_k = np.zeros(st.nall), np.zeros((st.nall, 6))
            e_k[st.ilist[k]], v_k[st.ilist[k]] = ebar[k], vbar[k]
            fd, floor = _train.fd_gradient(orc, s, e_k, fbar * mine[:, None], v_k, cols)
            scale = np.abs(rows[k]).max()
            ratio = np.abs(rows[k, cols] - fd).max() / scale
            print("%s star %d (K, L) = %s: %d columns, worst |twin - fd| / max|row| = %.3e (finite-difference floor %.3e)"
                  % (label, k, st.KL[k], len(cols), ratio, floor / scale))
            assert ratio <= 1e-9, (label, k, st.KL[k], ratio)
            worst = max(worst, ratio)
    finally:
        _train.set_theta(orc, theta0)
    print("%s: worst over the stars %.3e" % (label, worst))


@pytest.mark.parametrize("special,order", [(None, "mixed"), ("edge", "mixed"), (None, "straddle")])
def test_twin_value_of_stars_is_the_oracle_at_a_perturbed_theta(special, order):
    path = os.path.join(POT, "W_L8.mtp")
    orc = Oracle(path)
    tables = _pot(path).tables()
    st = _train.star_set(tables, _train.STAR_EDGE_KL, 62, special, order, shuffle=order != "straddle")
    s = _train.star_system(st)
    theta0 = _train.get_theta(orc)
    theta = theta0 * (1.0 + 0.05 * np.random.default_rng(2).normal(size=len(theta0)))
    try:
        _train.set_theta(orc, theta)
        r = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh)
    finally:
        _train.set_theta(orc, theta0)
    tw = train_twin(tables, s, theta)
    n = len(st.ilist)
    got = dict(f=tw["force"], eatom=_train.by_atom(st, tw["eatom"][:n]), vatom=_train.by_atom(st, tw["vatom"][:n]))
    ratios = _stars.per_star_ratios(st, got, r)
    for k, v in ratios.items():
        w = int(np.argmax(v))
        print("twin value %s %s %s: worst error / tolerance %.3e at star %d (K, L) = %s" % (special, order, k, v[w], w, st.KL[w]))
        assert np.isfinite(v).all() and v[w] <= 1.0, (k, w, st.KL[w], v[w])


@pytest.mark.parametrize("special", [None, "edge"])
@pytest.mark.parametrize("name", sorted(_tables.CENTRE_TABLES))
def test_twin_value_on_the_hand_made_tables_is_the_oracle_at_a_perturbed_theta(name, special):
    """tests/_tables.CENTRE_TABLES on the stars of the GPU tests (tests/_tables.CENTRE_KL), per star, through
    _train.oracle_value"""
    h = _design.handles(name)
    st = _train.star_set(h.tables, _tables.CENTRE_KL, 74, special)
    s = _train.star_system(st)
    theta0 = _train.get_theta(h.orc)
    np.testing.assert_array_equal(theta0, h.pot.theta())
    theta = theta0 * (1.0 + 0.05 * np.random.default_rng(2).normal(size=len(theta0)))
    try:
        _train.set_theta(h.orc, theta)
        want = _train.oracle_value(h.orc, s)
    finally:
        _train.set_theta(h.orc, theta0)
    tw = train_twin(h.tables, s, theta)
    n = len(st.ilist)                                        # (the twin's eatom and vatom by list row, the oracle's by atom)
    ratios = _stars.per_star_ratios(st, dict(f=tw["force"], eatom=_train.by_atom(st, tw["eatom"][:n]), vatom=_train.by_atom(st, tw["vatom"][:n])),
                                    dict(f=want["force"], eatom=want["eatom"], vatom=want["vatom"]))
    for k, v in ratios.items():
        w = int(np.argmax(v))
        print("twin value %s %s %s: worst error / tolerance %.3e at star %d (K, L) = %s" % (name, special, k, v[w], w, st.KL[w]))
        assert np.isfinite(v).all() and v[w] <= 1.0, (k, w, st.KL[w], v[w])
    assert np.abs(want["force"]).max() > 1e-3


@pytest.mark.parametrize("name,how", _tables.DEALT_WRONGLY)
def test_the_rule_of_the_gpu_rows_rejects_radial_functions_dealt_wrongly(name, how):
    """the GPU tests hold the kernel's gradient rows to the twin's with _train.star_block_ratio.  Rows of a twin whose radial
    functions are those a wrong tile_radial would compute ("dropped": no second trip, mu >= 8 gives zero; "modulo": the
    coefficient row of mu % 8; "part0": radial function 7 never computed) are refused by that rule at every star with a
    neighbour inside the cutoff, one tile or several, and pass at the K = 0 stars, whose rows hold ebar alone"""
    h = _design.handles(name)
    st = _train.star_set(h.tables, _tables.CENTRE_KL, 74)
    s = _train.star_system(st)
    n, Sp, nrad = len(st.ilist), len(h.tables["species_coeffs"]), len(h.tables["radial_coeffs"])
    theta0 = h.pot.theta()
    theta = theta0 * (1.0 + 0.05 * np.random.default_rng(2).normal(size=len(theta0)))
    ebar, fbar, vbar = _train.row_cotangents(st, 174)
    cots = (_train.padded_rows(st, ebar), fbar, _train.padded_rows(st, vbar))
    good = train_twin(h.tables, s, theta, *cots)["rows"][:n]
    wrong = np.concatenate([_tables.deal_wrongly(theta[:nrad], Sp, h.pot.sizes["Mu"], how), theta[nrad:]])
    bad = train_twin(h.tables, s, wrong, *cots)["rows"][:n]
    folds = {}
    for k, (K, L) in enumerate(st.KL):
        if K == 0:
            assert _train.star_block_ratio(bad[k:k + 1], good[k:k + 1], nrad, Sp, st.KL[k:k + 1], "%s %s K = 0" % (name, how)) <= 1.0
            continue
        with pytest.raises(AssertionError, match="misses 1e-9") as ei:
            _train.star_block_ratio(bad[k:k + 1], good[k:k + 1], nrad, Sp, st.KL[k:k + 1], "%s %s" % (name, how))
        w = good[k]
        folds[k] = float((np.abs(bad[k] - w) / (1e-9 + 1e-10 * np.abs(w).max())).max())
    one = [f for k, f in folds.items() if st.KL[k][0] <= 32]
    many = [f for k, f in folds.items() if st.KL[k][0] > 32]
    print("%s %s: the damaged twin's rows miss the bound %.1e-fold at least on one tile, %.1e-fold on several" % (
        name, how, min(one), min(many)))
    assert len(one) == 9 and len(many) == 6 and min(one) > 1.0 and min(many) > 1.0


def test_unit_energy_cotangent_rows_are_the_oracles_coeff_ders():
    """ebar = 1, fbar = vbar = 0: row i is the candidate vector dE_i / dtheta of the grade calls
    (pair_mtp_extrapolation.cpp:240-252, 323-329); in neighbourhood mode the oracle returns it per call, so one atom per call"""
    path = os.path.join(POT, "W_L16_nbh.almtp")
    orc = Oracle(path, selection=True)
    s = periodic_system_cell(*_design.replica16_cell(), _cells.LIST_CUTOFF)
    rows = train_twin(_pot(path).tables(), s, None, np.ones(s.nlocal), None, None)["rows"]
    want = np.zeros_like(rows)
    for i in range(s.nlocal):
        r = orc.compute(s.x, s.types, s.ilist[i:i + 1], np.array([0, s.first[i + 1] - s.first[i]], dtype=np.int32),
                        s.neigh[s.first[i]:s.first[i + 1]], extrapolation=True)
        want[i] = r["coeff_ders"]
    ratio = _design.column_ratio(rows, want)
    print("ebar = 1 rows against the oracle's coeff_ders: worst error / bound %.3e" % ratio)
    assert ratio <= 1.0


def test_zero_energy_cotangent_moment_columns_are_the_design_rows_transposed():
    path = os.path.join(POT, "W_L16.mtp")
    tables = _pot(path).tables()
    s = periodic_system_cell(*_design.replica16_cell(), _cells.LIST_CUTOFF)
    _, fbar, vbar = _train.cotangents(s.nlocal, 3)
    rows = train_twin(tables, s, None, None, fbar, vbar)["rows"]
    d = design_twin(tables, s)
    nrad, Sp = len(tables["radial_coeffs"]), len(tables["species_coeffs"])
    want = d["force"].T @ fbar.reshape(-1) + np.einsum("iac,ia->c", d["virial_atom"], vbar)
    ratio = _design.column_ratio(rows.sum(0)[None, nrad:], want[None, :])
    print("ebar = 0 linear columns against design_twin^T (fbar, vbar): worst error / bound %.3e" % ratio)
    assert ratio <= 1.0 and not rows[:, nrad:nrad + Sp].any()


# ---- the writer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ALL_POTENTIALS)
def test_write_all_coeffs_round_trip_bit_for_bit(tmp_path, fname):
    src, dst = os.path.join(POT, fname), str(tmp_path / ("out" + os.path.splitext(fname)[1]))
    t = _pot(src).tables()
    rng = np.random.default_rng(17)
    ra = t["radial_coeffs"] * (1.0 + 0.25 * rng.uniform(-1, 1, len(t["radial_coeffs"]))) + 1e-3 * rng.normal(size=len(t["radial_coeffs"]))
    sp = t["species_coeffs"] + rng.normal(size=len(t["species_coeffs"]))
    mo = t["moment_coeffs"] * (1.0 + 0.25 * rng.uniform(-1, 1, len(t["moment_coeffs"])))
    rc = capi.write_all_coeffs(src, dst, mo, sp, ra)
    text = open(dst, "rb").read()
    assert rc == (capi.WROTE_WITHOUT_SELECTION if fname.endswith(".almtp") else 0) and b"#MVS" not in text
    assert sorted(os.listdir(tmp_path)) == [os.path.basename(dst)]          # no temporary file left
    back = capi.Potential(dst)
    np.testing.assert_array_equal(back.theta(), np.concatenate([ra, sp, mo]))
    o = Oracle(dst)
    np.testing.assert_array_equal(_train.get_theta(o), np.concatenate([ra, sp, mo]))
    for k in ("alpha_index_basic", "alpha_index_times", "alpha_moment_mapping"):
        np.testing.assert_array_equal(back.tables()[k], t[k])
    # the source's layout: pair lines and brace lines indented as in the source, Mu brace lines of R numbers per pair
    src_lines, dst_lines = open(src, "rb").read().split(b"\n"), text.split(b"\n")
    a = next(i for i, l in enumerate(src_lines) if l.strip() == b"radial_coeffs")
    assert dst_lines[:a + 1] == src_lines[:a + 1]
    indent = lambda l: l[:len(l) - len(l.lstrip())]
    assert indent(dst_lines[a + 1]) == indent(src_lines[a + 1]) and indent(dst_lines[a + 2]) == indent(src_lines[a + 2])
    s = back.sizes
    assert dst_lines[a + 1 + s["Sp"] ** 2 * (s["Mu"] + 1)].startswith(b"alpha_moments_count")
    # radial_coeffs = None keeps the block byte for byte: the same file write_coeffs writes
    capi.write_all_coeffs(src, str(tmp_path / "a"), mo, sp, None)
    capi.write_coeffs(src, str(tmp_path / "b"), mo, sp)
    assert open(str(tmp_path / "a"), "rb").read() == open(str(tmp_path / "b"), "rb").read()


def test_write_all_coeffs_refusals(tmp_path):
    src, dst = os.path.join(POT, "WRe_L10_cfg.almtp"), str(tmp_path / "out.almtp")
    t = _pot(src).tables()
    ra, sp, mo = t["radial_coeffs"], t["species_coeffs"], t["moment_coeffs"]
    for bad in (np.nan, np.inf):
        for which in range(3):
            args = [mo.copy(), sp.copy(), ra.copy()]
            args[which][-1] = bad
            with pytest.raises(capi.MtpError) as ei:
                capi.write_all_coeffs(src, dst, *args)
            assert ei.value.code == -20
    for args in ((mo[:-1], sp, ra), (mo, sp[:-1], ra), (mo, sp, ra[:-1]), (mo, sp, np.concatenate([ra, [0.0]]))):
        with pytest.raises(capi.MtpError) as ei:
            capi.write_all_coeffs(src, dst, *args)
        assert ei.value.code == -20
    with pytest.raises(capi.MtpError):
        capi.write_all_coeffs(str(tmp_path / "missing.mtp"), dst, mo, sp, ra)
    assert os.listdir(tmp_path) == []


# ---- the training table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ALL_POTENTIALS)
def test_every_committed_potential_has_a_supported_table(fname):
    pot = _pot(os.path.join(POT, fname))
    t = pot.train_table()
    s = pot.sizes
    assert t["supported"] and t["late_row"] == t["dup_scalar"] == -1 and t["message"] == ""
    assert t["C"] == s["Sp"] ** 2 * s["Mu"] * s["R"] + s["Sp"] + s["S"] == len(pot.theta())
    d = pot.design_table()
    assert (t["rows"], t["A"], t["B"], t["Mu"]) == (len(d["rows"]), d["A"], d["B"], s["Mu"])
    assert sorted(t["bymu"]) == list(range(s["B"])) and t["mufirst"][0] == 0 and t["mufirst"][-1] == s["B"]
    mu_of = (d["basic_pack"] >> 20) & 15
    assert all((mu_of[t["bymu"][t["mufirst"][m]:t["mufirst"][m + 1]]] == m).all() for m in range(s["Mu"]))


@pytest.mark.parametrize("level", [8, 6, 10, 12])
def test_the_generators_default_tables_are_supported(tmp_path, level):
    tab = mtpgen.level8_template() if level == 8 else mtpgen.build_table(level)
    path = str(tmp_path / "gen.mtp")
    mtpgen.write_mtp(mtpgen.random_potential(tab, 2), path)
    t = capi.Potential(path).train_table()
    assert t["supported"], t["message"]


@pytest.mark.parametrize("late,dup", [(True, False), (False, True), (True, True)])
def test_the_mutated_table_is_reported(tmp_path, late, dup):
    """a row that reads a moment a later row still adds to, and two scalars on one moment (tests/_mutate.py): for both the
    reference's forces are not the gradient of its energy, and the table says which row or scalar"""
    path = str(tmp_path / "mutated.mtp")
    info = _mutate.mutate_mtp(os.path.join(POT, "W_L16.mtp"), path, late_writer=late, dup_mapping=dup)
    pot = capi.Potential(path)
    t = pot.train_table()
    tab = pot.tables()
    assert not t["supported"]
    if late:
        times = tab["alpha_index_times"]
        k = t["late_row"]
        assert k >= 0 and info["moved_target"] in (times[k, 0], times[k, 1]) and times[-1, 3] == info["moved_target"]
        assert not any(times[j, 3] in (times[q, 0], times[q, 1]) for q in range(k) for j in range(q, len(times)))   # the first
        assert "row %d of alpha_index_times" % k in t["message"]
    else:
        assert t["late_row"] == -1
    if dup:
        assert t["dup_scalar"] == len(tab["alpha_moment_mapping"]) - 1
        if not late:
            assert "scalar %d of alpha_moment_mapping" % t["dup_scalar"] in t["message"]
    else:
        assert t["dup_scalar"] == -1


# ---- both under ASan + UBSan, in a program of their own ------------------------------------------------------------------
@pytest.fixture(scope="module")
def san_exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "host"), "san_train"])
    return os.path.join(ROOT, "tests", "cpp", "test_train_san")


@pytest.mark.parametrize("fname", ALL_POTENTIALS)
def test_writer_and_training_table_run_clean_under_sanitizers(san_exe, tmp_path, fname):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_exe, os.path.join(POT, fname), str(tmp_path / "out.mtp")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "OK" and int(words[1]) == (1 if fname.endswith(".almtp") else 0), r.stdout
    assert words[2:] == ["-1", "-1"], r.stdout
