"""CPU checks of the linear refit (include/mtp_mi355x.h, "linear refit"): the numpy twin of the design-row kernel against
the oracle's unit-coefficient columns, the coefficient writer, the tangent kernel's host-side table, and both under the
sanitizers in a stand-alone program."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cells  # noqa: E402
import _design  # noqa: E402
import _stars  # noqa: E402
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


# ---- the star sets of tests/test_design_gpu.py: the twin alone, and the judge on damaged copies of the twin's rows -------------
# tests/_design.star_case builds every set the GPU tests run (tile, row-length and straddle edges up to four tiles, levels 16
# and 20, the generated potentials with five and three species, a scaling, nine radial functions and a 5.5 A cutoff, the
# row-range set and the three owner maps); star_ratios is the rule of test_design_gpu._check_stars.  First the reference
# alone: the twin must be inside 1e-9 + 1e-10 max |column| on every one of them, else the INPUT is wrong for the bound.
# Then the twin's rows damaged the way a subtly wrong kernel would damage them: the rule must reject the damaged star, and
# no other.  The GPU entries land a thousand times inside the bound; this is what shows the bound still bites.
@functools.lru_cache(maxsize=None)
def _twin(name):
    c = _design.star_case(name)
    return _design.twin_rows(c.h.tables, c.st, c.owner, c.nowned)


def _ratios(name, got):
    c = _design.star_case(name)
    return _design.star_ratios(c.st, got, _design.case_want(name), c.per_star)


def _copy(rows):
    return {k: v.copy() for k, v in rows.items()}


def _only(r, stars, kinds=("basis", "force", "virial"), what=""):
    """the listed kinds miss the bound at every listed star; every other star, and the other kinds, are inside it"""
    stars = np.atleast_1d(stars)
    assert len(stars), what + ": no star is damaged"
    for k in ("basis", "force", "virial"):
        hit = np.zeros(len(r[k]), dtype=bool)
        if k in kinds:
            hit[stars] = True
        print("%s %s: error / bound at the damaged stars %.3e .. %.3e, elsewhere at most %.3e" % (
            what, k, r[k][hit].min() if hit.any() else 0.0, r[k][hit].max() if hit.any() else 0.0,
            r[k][~hit].max() if (~hit).any() else 0.0))
        assert (r[k][hit] > 1.0).all(), (what, k, "accepted at star", int(np.flatnonzero(hit)[np.argmin(r[k][hit])]))
        assert (r[k][~hit] <= 1.0).all(), (what, k, "rejected at star", int(np.flatnonzero(~hit)[np.argmax(r[k][~hit])]))


@pytest.mark.parametrize("name", _design.all_cases())
def test_twin_alone_is_inside_the_bound_on_every_star_set_of_the_gpu_tests(name):
    r = _ratios(name, _twin(name))
    worst = max(float(v.max()) for v in r.values())
    print("%s: twin against the oracle's columns, worst error / bound over %d stars %.3e" % (name, len(r["basis"]), worst))
    assert worst <= 1.0


def _virial_of(G, u):
    """the six virial rows [6, cols] of one neighbour at u with tangent G [3, cols] (pair_mtp.cpp:257-276)"""
    return -np.array([G[0] * u[0], G[1] * u[1], G[2] * u[2], 0.5 * (G[0] * u[1] + G[1] * u[0]),
                      0.5 * (G[0] * u[2] + G[2] * u[0]), 0.5 * (G[1] * u[2] + G[2] * u[1])])


PLAIN8 = "level8-None-mixed"


def _star_with(name, K):
    return [k for k, l in _design.star_case(name).st.KL].index(K)


def test_judge_rejects_the_33rd_neighbour_left_out_of_the_basics():
    """the one column of a second tile: the twin over a list without the entry; basis row, force rows and virial rows of
    that star all lack it"""
    c = _design.star_case(PLAIN8)
    st, s = c.st, _star_with(PLAIN8, 33)
    e = int(_stars.in_cutoff_entries(st, s)[32])
    first = st.first.copy()
    first[s + 1:] -= 1
    cut = SimpleNamespace(**dict(vars(st), first=first, neigh=np.delete(st.neigh, e)))
    _only(_ratios(PLAIN8, _design.twin_rows(c.h.tables, cut)), s, what="33rd neighbour not in the basics")


def test_judge_rejects_the_33rd_neighbour_left_out_of_the_directions():
    """its direction never run: the basis row is right, its own force row stays zero, the centre's row and the virial
    rows lack its term"""
    c = _design.star_case(PLAIN8)
    st, s = c.st, _star_with(PLAIN8, 33)
    j, i = int(st.neigh[_stars.in_cutoff_entries(st, s)[32]]), int(st.ilist[s])
    got = _copy(_twin(PLAIN8))
    G = -got["force"][j]
    got["force"][j] = 0.0
    got["force"][i] -= G
    got["virial"][s] -= _virial_of(G, st.x[j] - st.x[i])
    _only(_ratios(PLAIN8, got), s, ("force", "virial"), "33rd neighbour not in the directions")


@pytest.mark.parametrize("name", ["scaling-None", "nine_radial-None"])
def test_judge_rejects_the_radial_block_of_the_transposed_species_pair(name):
    """jt * Sp + itype for itype * Sp + jt, on two and on three species: every star with an in-cutoff neighbour of another
    species than its centre is rejected, every other one (K = 0, one species throughout) is untouched"""
    c = _design.star_case(name)
    st, t = c.st, dict(c.h.tables)
    Sp = len(t["species_coeffs"])
    assert Sp == (2 if name.startswith("scaling") else 3)
    t["radial_coeffs"] = np.asarray(t["radial_coeffs"]).reshape(Sp, Sp, -1).transpose(1, 0, 2).reshape(-1).copy()
    mixed = [s for s in range(len(st.ilist))
             if (st.types[st.neigh[_stars.in_cutoff_entries(st, s)]] != st.types[st.ilist[s]]).any()]
    assert 0 < len(mixed) < len(st.ilist) and any(st.KL[s][0] == 1 for s in mixed)
    _only(_ratios(name, _design.twin_rows(t, st)), mixed, what="transposed pair, %d species" % Sp)


def test_judge_rejects_a_scaling_taken_as_one():
    c = _design.star_case("scaling-None")
    assert c.h.tables["scaling"] == 2.5
    some = [s for s, (K, L) in enumerate(c.st.KL) if K > 0]
    _only(_ratios("scaling-None", _design.twin_rows(dict(c.h.tables, scaling=1.0), c.st)), some, what="scaling = 1")


def _chain_term(tables, st, s, coord):
    """(G [K, cols], js, u): the part of the tangents of star s that comes from the e - 1 term of coordinate `coord` alone
    (val e u_c^(e-1) times the other two powers, pair_mtp.cpp:163-191), pushed through the times rows as the twin does"""
    basic = np.asarray(tables["alpha_index_basic"], dtype=np.int64).reshape(-1, 4)
    times = np.asarray(tables["alpha_index_times"], dtype=np.int64).reshape(-1, 4)
    mapping = np.asarray(tables["alpha_moment_mapping"], dtype=np.int64)
    Sp, B = len(tables["species_coeffs"]), len(basic)
    Mu = int(basic[:, 0].max()) + 1
    radial = np.asarray(tables["radial_coeffs"], dtype=np.float64).reshape(Sp, Sp, Mu, -1)
    R = radial.shape[-1]
    A = int(max(B, times[:, [0, 1, 3]].max() + 1, mapping.max() + 1))
    rmin, rmax = float(tables["min_cutoff"]), float(tables["max_cutoff"])
    i = int(st.ilist[s])
    js = st.neigh[_stars.in_cutoff_entries(st, s)]
    u = st.x[js] - st.x[i]
    r = np.sqrt((u * u).sum(1))
    d, ksi = r - rmax, (2.0 * r - (rmin + rmax)) / (rmax - rmin)
    q = np.zeros((R, len(js)))
    q[0], q[1] = float(tables["scaling"]) * d * d, float(tables["scaling"]) * ksi * d * d
    for ri in range(2, R):
        q[ri] = 2.0 * ksi * q[ri - 1] - q[ri - 2]
    val_mu = np.einsum("kmr,rk->mk", radial[st.types[i] - 1, st.types[js] - 1], q)
    ex = basic[:, 1:4]
    P = int(ex.sum(1).max()) + 1
    pw = u.T[:, None, :] ** np.arange(P)[None, :, None]
    val = val_mu[basic[:, 0]] * (1.0 / r)[None, :] ** ex.sum(1)[:, None]
    p = [pw[0][ex[:, 0]], pw[1][ex[:, 1]], pw[2][ex[:, 2]]]
    M, dM = np.zeros(A), np.zeros((A, len(js)))
    M[:B] = (val * p[0] * p[1] * p[2]).sum(1)
    p[coord] = ex[:, coord][:, None] * pw[coord][np.maximum(ex[:, coord] - 1, 0)]
    dM[:B] = val * p[0] * p[1] * p[2]
    for a0, a1, mlt, a3 in times:
        M[a3] += mlt * M[a0] * M[a1]
    for a0, a1, mlt, a3 in times:
        dM[a3] += mlt * (dM[a0] * M[a1] + M[a0] * dM[a1])
    last = {int(m): k for k, m in enumerate(mapping)}
    fcol = np.array([last[int(m)] == k for k, m in enumerate(mapping)])
    return np.concatenate([np.zeros((Sp, len(js))), dM[mapping] * fcol[:, None]]).T, js, u


@pytest.mark.parametrize("coord", [0, 2])
def test_judge_rejects_a_dropped_chain_rule_term_of_one_coordinate(coord):
    c = _design.star_case(PLAIN8)
    st, s = c.st, _star_with(PLAIN8, 2)
    Gc, js, u = _chain_term(c.h.tables, st, s, coord)
    got = _copy(_twin(PLAIN8))
    # the twin's rows are right with the term: taking it out of a copy and putting it back must give the rows again
    for sign in (1.0, -1.0):
        for n, j in enumerate(js):
            G = np.zeros((3, Gc.shape[1]))
            G[coord] = sign * Gc[n]
            got["force"][j] += G
            got["force"][st.ilist[s]] -= G
            got["virial"][s] -= _virial_of(G, u[n])
        if sign > 0:
            _only(_ratios(PLAIN8, got), s, ("force", "virial"), "e - 1 term of coordinate %d dropped" % coord)
    assert max(float(v.max()) for v in _ratios(PLAIN8, got).values()) <= 1.0


def test_judge_rejects_exchanged_xz_and_yz_virial_halves():
    c = _design.star_case(PLAIN8)
    got = _copy(_twin(PLAIN8))
    got["virial"][:, [4, 5]] = got["virial"][:, [5, 4]]
    _only(_ratios(PLAIN8, got), [s for s, (K, L) in enumerate(c.st.KL) if K > 0], ("virial",), "xz and yz exchanged")


def test_judge_rejects_rows_of_a_ranged_call_placed_at_ii():
    """rows [a, b) of the row-range set written at ii where they belong at ii - a, into arrays of b - a rows filled with
    7.0: the rows that still land inside the array are other stars' rows, the rest keeps the fill"""
    a, b = _design.RANGE_CUTS
    got = _copy(_twin("ranges"))
    for kind in ("basis", "virial"):
        out = np.full((b - a,) + got[kind].shape[1:], 7.0)
        for ii in range(a, b):
            if ii < b - a:
                out[ii] = got[kind][ii]
        got[kind][a:b] = out
    _only(_ratios("ranges", got), np.arange(a, b), ("basis", "virial"), "rows at ii")


def test_judge_rejects_1e8_relative_on_one_column_of_a_one_neighbour_star_beside_four_tile_stars():
    """the per-star scale is what catches it: with the column's scale taken over all stars, the 97-neighbour stars' entries
    would let it pass"""
    c = _design.star_case(PLAIN8)
    st, want = c.st, _design.case_want(PLAIN8)
    bounds = list(st.start) + [st.nall]
    best = (0.0, None, None)
    for s, (K, L) in enumerate(st.KL):
        if K == 1:
            m = np.abs(want["f_all"][bounds[s]:bounds[s + 1]]).max((0, 1))
            best = max(best, (float(m.max()), s, int(np.argmax(m))))
    m, s, col = best
    # 1e-8 m > 1e-9 + 1e-10 m needs m > 0.102
    assert m > 0.2 and max(K for K, L in st.KL) == 97, m
    got = _copy(_twin(PLAIN8))
    got["force"][bounds[s]:bounds[s + 1], :, col] *= 1.0 + 1e-8
    _only(_ratios(PLAIN8, got), s, ("force",), "1e-8 relative on column %d of star %d" % (col, s))
    assert _design.column_ratio(got["force"], want["f_all"]) <= 1.0


# ---- hand-made tables for the per-centre kernels (tests/_tables.CENTRE_TABLES): Mu up to 16, rank 11, sparse slots ---------
# Their star sets are registered in _design.star_cases(), so test_twin_alone_is_inside_the_bound_... above holds the twin to
# the oracle's columns on each of them.  Here: every case has the property it is in the catalogue for, and the rule rejects a
# twin whose radial functions are dealt the way a wrong tile_radial would deal them.
# name -> Mu, blk = Sp Mu R, [radial functions without a basic], [P, largest multiplicity]
CENTRE_PROPERTIES = dict(mu6=(6, 48, []), mu8=(8, 128, []), mu9=(9, 162, []), mu13_gaps=(13, 208, [1, 3, 4, 6, 8, 9, 10, 11]),
                         mu16_sp3=(16, 384, []), mu16_sp2_nbh=(16, 256, []), rank11=(2, 16, [], 12, 11550))


def test_the_catalogue_is_the_list_of_properties():
    assert sorted(CENTRE_PROPERTIES) == sorted(_tables.CENTRE_TABLES)


@pytest.mark.parametrize("name", sorted(CENTRE_PROPERTIES))
def test_every_centre_table_is_supported_and_has_the_property_it_is_there_for(name):
    Mu, blk, empty = CENTRE_PROPERTIES[name][:3]
    case, h = _tables.CENTRE_TABLES[name], _design.handles(name)
    s, t = h.pot.sizes, h.pot.train_table()
    assert t["supported"] and t["message"] == "" and t["C"] == len(h.pot.theta())
    assert (s["Mu"], s["Sp"] * s["Mu"] * s["R"], s["Sp"], s["R"]) == (Mu, blk, case["species"], case.get("R", 8))
    assert h.tables["scaling"] == case.get("scaling", 1.0) and (b"#MVS" in open(h.path, "rb").read()) == bool(case.get("mvs"))
    mf = t["mufirst"]
    assert [mu for mu in range(Mu) if mf[mu] == mf[mu + 1]] == empty and mf[0] == 0 and mf[-1] == s["B"]
    used = sorted(set(int(mu) for mu in h.tables["alpha_index_basic"][:, 0]))
    assert used == [mu for mu in range(Mu) if mu not in empty]
    # what the training kernel's loops do with it (NT = 32 columns, 256 threads, 24 scratch rows for value mode)
    assert (Mu > 8) == (name in ("mu9", "mu13_gaps", "mu16_sp3", "mu16_sp2_nbh")), "second trip of the dealing and item loops"
    assert (2 * Mu > 24) == (name in ("mu13_gaps", "mu16_sp3", "mu16_sp2_nbh")), "scratch rows sized by 2 Mu"
    assert (blk > 256) == (name == "mu16_sp3"), "second trip of the loop over the radial block"
    for slot, mons in case.get("subsets", {}).items():           # a sparse slot: some of its monomials, not all
        have = [tuple(b[1:]) for b in h.tables["alpha_index_basic"] if b[0] == slot[0] and sum(b[1:]) == slot[1]]
        assert sorted(have) == sorted(mons) and len(mons) < len(mtpgen.monomials(slot[1]))
    if len(CENTRE_PROPERTIES[name]) > 3:
        P, mult = CENTRE_PROPERTIES[name][3:]
        assert s["P"] == P and int(h.tables["alpha_index_times"][:, 2].max()) == mult
        for slot in case["subsets"]:
            assert (4, 4, 3) in case["subsets"][slot]
    print("%s: Mu %d, blk %d, B %d, A %d, S %d, C %d: %s" % (name, Mu, blk, s["B"], s["A"], s["S"], s["C"], case["reaches"]))


def _deal_wrongly(tables, how):
    """the tables with the radial block as a wrong tile_radial would use it (tests/_tables.deal_wrongly)"""
    Mu = int(np.asarray(tables["alpha_index_basic"])[:, 0].max()) + 1
    return dict(tables, radial_coeffs=_tables.deal_wrongly(tables["radial_coeffs"], len(tables["species_coeffs"]), Mu, how))


@pytest.mark.parametrize("special", [None, "edge"])
@pytest.mark.parametrize("name,how", _tables.DEALT_WRONGLY)
def test_judge_rejects_radial_functions_dealt_wrongly_over_the_eight_parts(name, how, special):
    """every star with a neighbour strictly inside the cutoff is rejected, in its basis row, its force rows and its virial
    rows; a star without one (K = 0, or K = 1 with its one neighbour ON the cutoff, where every radial function and its
    derivative vanish) sees nothing of the radial block and stays inside the bound"""
    case = "%s-%s" % (name, special)
    c = _design.star_case(case)
    r = _ratios(case, _design.twin_rows(_deal_wrongly(c.h.tables, how), c.st))
    seen = [s for s, (K, L) in enumerate(c.st.KL) if K > (1 if special == "edge" else 0)]
    _only(r, seen, what="%s %s" % (case, how))
    fold = np.minimum(np.minimum(r["basis"], r["force"]), r["virial"])
    one = [s for s in seen if c.st.KL[s][0] <= 32]
    many = [s for s in seen if c.st.KL[s][0] > 32]
    print("%s %s: the damaged twin misses the bound %.1e-fold at least on one tile, %.1e-fold on several" % (
        case, how, fold[one].min(), fold[many].min()))
    assert len(one) and len(many) and (fold[one] > 1.0).all() and (fold[many] > 1.0).all()
    if special is None:
        assert any(c.st.KL[s][0] == 1 for s in seen) and any(c.st.KL[s][0] == 2 for s in seen)


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
