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
import _tables  # noqa: E402
import _train  # noqa: E402
from lammps_mtp_kokkos_amd import capi, md  # noqa: E402

POT = _design.POT


def _device_stream():
    import torch
    dev = torch.device("cuda:0")
    return dev, capi.use_private_torch_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def _ctx(fname):
    """the shared context of a file of potentials/ or of a generated potential (tests/_design.handles)"""
    return capi.Context(_design.handles(fname).pot, 0)


def _oracle(fname):
    return _design.handles(fname).orc


def _theta0(fname):
    t = _design.handles(fname).tables
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
TAIL = 2                                                     # rows behind row_count in basis and virial: they keep their fill


def _design_call(ctx, st, row_begin=0, row_count=None, owner=None, nowned=None, basis=True, virial=True, force_t=None, neigh=None,
                 max_numneigh=None):
    """one Context.design_rows call over rows [row_begin, row_begin + row_count) of a star set and its synchronise.
    owner: None (d_owner = NULL, every atom its own owner) or the map as an array, passed on the device; force_t: the
    [3 nowned, ld] array of an earlier call to accumulate into (None: zeros); basis / virial = False: that output NULL;
    neigh: another list than st.neigh; max_numneigh: install the list as DEVICE arrays with this declared row length.
    Returns dict(basis [row_count, cols] or None, force [nowned, 3, cols], virial [row_count, 6, cols] or None, force_t).
    The leading dimension is above the columns and the outputs hold TAIL rows more than asked for, all filled with 7.0:
    asserted here are zero padding columns and an untouched tail."""
    import torch
    dev, stream = _device_stream()
    info = ctx.pot.info
    cols = info.species_count + info.alpha_scalar_count
    ld = cols + (cols & 1) + 2
    nowned = st.nall if nowned is None else nowned
    nrows = len(st.ilist) - row_begin if row_count is None else row_count
    to = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, dtype=ty)).to(dev)
    ne = st.neigh if neigh is None else neigh
    if max_numneigh is None:
        ctx.set_neighbors(st.ilist, st.first, ne, st.nall)
    else:
        ctx.set_neighbors_device(to(st.ilist, np.int32), to(st.first, np.int32), to(ne, np.int32), st.nall, max_numneigh)
    x_t, t_t = to(st.x, np.float64), to(st.types, np.int32)
    own_t = None if owner is None else to(owner, np.int32)
    if force_t is None:
        force_t = torch.zeros((3 * nowned, ld), dtype=torch.float64, device=dev)
    basis_t = torch.full((nrows + TAIL, ld), 7.0, dtype=torch.float64, device=dev) if basis else None
    virial_t = torch.full((nrows + TAIL, 6, ld), 7.0, dtype=torch.float64, device=dev) if virial else None
    ctx.design_rows(row_begin, nrows, x_t, t_t, force_t, nowned, ld, basis_t=basis_t, virial_t=virial_t,
                    owner=None if own_t is None else own_t.data_ptr(), stream=stream)
    ctx.synchronize(stream=stream)
    f = force_t.cpu().numpy()
    assert not f[:, cols:].any(), "padding columns of the force rows must be zero"
    out = dict(basis=None, virial=None, force=f[:, :cols].reshape(nowned, 3, cols), force_t=force_t)
    for key, t in (("basis", basis_t), ("virial", virial_t)):
        if t is not None:
            a = t.cpu().numpy()
            assert (a[nrows:] == 7.0).all(), "%s rows behind row_count must keep their fill" % key
            assert not a[:nrows, ..., cols:].any(), "padding columns of the %s rows must be zero" % key
            out[key] = a[:nrows, ..., :cols]
    return out


def _design_rows_of_stars(fname, st, neigh=None, ctx=None):
    """Context.design_rows over a star system with d_owner = NULL (every atom is its own owner): dict(basis [stars, cols],
    force [nall, 3, cols], virial [stars, 6, cols]); ctx: another context than the shared one of the file"""
    return _design_call(ctx or _ctx(fname), st, neigh=neigh)


def _check_stars(fname, st, got, label, orc=None, want=None, per_star=True):
    """per star and per column with the star's own scale (the rule of _stars.per_star_check, in tests/_design.star_ratios): a
    three-tile star must not be able to hide a one-neighbour one; orc: another oracle than the shared one of the file;
    want: the oracle's columns where they are at hand; per_star = False: see star_ratios"""
    if want is None:
        want = _design.oracle_columns(orc or _oracle(fname), st.x, st.types, st.ilist, st.first, st.neigh)
    ratios = _design.star_ratios(st, got, want, per_star)
    worst = 0.0
    for kind, r in ratios.items():                           # each kind with the column's maximum over its own rows
        for s, ratio in enumerate(r):
            assert ratio <= 1.0, "%s %s: star %d (K, L) = %s misses its bound %.2f-fold" % (label, kind, s, st.KL[s], ratio)
        worst = max([worst] + list(r))
    print("%s: worst error / bound over %d stars %.3e" % (label, len(st.ilist), worst))
    return worst


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


# ---- the edges the sets above leave out: species pairs, radial parameters, four tiles, plain and straddle rows, row
# ranges, optional outputs, owner maps, special-bond bits.  The sets are those of tests/_design.star_case and their oracle
# columns are computed once (_design.case_want); tests/test_design_cpu.py runs the twin alone on the same sets and shows on
# damaged copies that the bound rejects a kernel that is wrong in each of these ways.  Worst ratios: DESIGN.md 5.3.1. -----
def _run_case(name, ctx=None, **call):
    """the design rows of a case of tests/_design.star_case against its oracle columns; the exact rows of every K = 0 star"""
    c = _design.star_case(name)
    want = _design.case_want(name)
    got = _design_call(ctx or _ctx(c.pot), c.st, owner=c.owner, nowned=c.nowned, **call)
    _check_stars(None, c.st, got, name, want=want, per_star=c.per_star)
    _exact_rows_of_empty_stars(c, got)
    return c, want, got


def _exact_rows_of_empty_stars(c, got, rows=None):
    """K = 0: the basis row is 1 in the centre's species column and 0 elsewhere, the star's force rows and its virial rows
    are zero, exactly (rows: the list rows that got's basis and virial rows belong to)"""
    st = c.st
    for k, s in enumerate(range(len(st.ilist)) if rows is None else rows):
        if st.KL[s][0] == 0:
            one_hot = np.zeros(got["force"].shape[-1])
            one_hot[st.types[st.ilist[s]] - 1] = 1.0
            assert got["basis"] is None or np.array_equal(got["basis"][k], one_hot), (c.name, s)
            assert got["virial"] is None or not got["virial"][k].any(), (c.name, s)
            if c.per_star:
                assert not got["force"][st.sid == s].any(), (c.name, s)


@pytest.mark.gpu
@pytest.mark.parametrize("special,order", _design.LEVEL8_MODES)
def test_level8_stars_one_to_four_tiles_plain_edge_and_straddle_rows(special, order):
    """tests/_train.STAR_EDGE_KL: K in {0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 97} x L in {K, K + 1, 129}, and L in {63, 64,
    65, 128} for K in {1, 33}.  The plain set is what tests K = 1 and 2 with neighbours that contribute and one tile on
    the "a single tile still holds its tables" side of the shortcut without an entry at r_c; "straddle": survivors touching
    entry 128 on both sides, rows in that order (the second sweep of the compaction continues a count)"""
    c, want, got = _run_case("level8-%s-%s" % (special, order))
    assert c.st.KL == _train.STAR_EDGE_KL and sum(K == 0 for K, L in c.st.KL) == 3
    if special is None and order == "mixed":                 # no vacuous comparison: every moment column of the force rows
        bounds = list(c.st.start) + [c.st.nall]
        for s, (K, L) in enumerate(c.st.KL):
            if K >= 2:
                assert (np.abs(want["f_all"][bounds[s]:bounds[s + 1], :, 1:]).max((0, 1)) > 1e-3).all(), (s, K, L)


@pytest.mark.gpu
@pytest.mark.parametrize("special", [None, "edge"])
@pytest.mark.parametrize("fname", ["W_L16.mtp", "WRe_L20.mtp"])
def test_level16_and_two_species_level20_stars_plain_and_edge(fname, special):
    c, want, got = _run_case("%s-%s" % (fname, special))
    if fname == "WRe_L20.mtp":
        assert set(c.st.types[c.st.ilist]) == {1, 2}, "a centre of each species"


@pytest.mark.gpu
@pytest.mark.parametrize("special", [None, "edge"])
@pytest.mark.parametrize("which", ["five_species", "nine_radial", "scaling"])
def test_generated_potentials_species_pairs_radial_size_scaling_and_cutoff(which, special):
    """the potentials of test_train_gpu.GENERATED: Sp = 5 / Sp = 2, scaling = 2.5 / Sp = 3, R = 9, scaling = 0.37, cutoff
    5.5 -- the pair index itype Sp + jt and the block stride Mu R of the design kernel's own radial buffer, rmin, rmax and
    inv_span, the R > 1 and ri >= 2 legs of the recurrence, rows of 1 to 6 neighbours that lack a species"""
    from test_train_gpu import GENERATED
    level, Sp, seed, rmin, rmax, R, scaling = GENERATED[which]
    c, want, got = _run_case("%s-%s" % (which, special))
    t, st = c.h.tables, c.st
    assert (len(t["species_coeffs"]), t["scaling"], t["max_cutoff"], t["min_cutoff"]) == (Sp, scaling, rmax, rmin)
    assert _ctx(which).pot.info.radial_basis_size == R and st.rc == rmax
    assert set(st.types[st.ilist]) == set(range(1, Sp + 1)), "a centre of every species"
    small = [k for k, (K, L) in enumerate(st.KL) if 0 < K <= 6]
    if Sp >= 3:
        assert any(len(set(st.types[st.neigh[st.first[k]:st.first[k + 1]]])) < Sp for k in small), "a row that lacks a neighbour type"


@pytest.mark.gpu
@pytest.mark.parametrize("special", [None, "edge"])
@pytest.mark.parametrize("name", sorted(_tables.CENTRE_TABLES))
def test_hand_made_tables_six_to_sixteen_radial_functions_rank_eleven_and_sparse_slots(name, special):
    """tests/_tables.CENTRE_TABLES, which the level generator cannot make: every part of a neighbour column computes a radial
    function (Mu = 6, 8), the second trip of tile_radial's dealing loop (Mu = 9, 13, 16), radial functions without a basic,
    three species at Mu = 16, P = 12 with a multiplicity of 11 550 in the packed rows, slots that list some of their
    monomials.  K in {0, 1, 2, 32, 33, 65} x L in {K, K + 1, 129}, rows shuffled, one launch; plain and with an entry on the
    cutoff.  tests/test_design_cpu.py shows that the rule rejects radial functions dealt wrongly on these very sets"""
    c, want, got = _run_case("%s-%s" % (name, special))
    case = _tables.CENTRE_TABLES[name]
    assert c.st.KL == _tables.CENTRE_KL and _ctx(name).pot.sizes["Sp"] == case["species"]
    assert set(c.st.types[c.st.ilist]) == set(range(1, case["species"] + 1)), "a centre of every species"
    if special is None:                                      # no vacuous comparison: no scalar's force column is all zero
        bounds = list(c.st.start) + [c.st.nall]
        for s, (K, L) in enumerate(c.st.KL):
            if K >= 2:
                assert np.abs(want["f_all"][bounds[s]:bounds[s + 1], :, case["species"]:]).max((0, 1)).all(), (s, K, L)


def _outer(st):
    """the atoms that are no centre: in a star set each receives one atomic add per column, from its one list entry"""
    return np.setdiff1d(np.arange(st.nall), st.ilist)


@pytest.mark.gpu
@pytest.mark.parametrize("basis,virial", [(True, True), (False, True), (True, False), (False, False)])
def test_row_ranges_land_at_ii_minus_row_begin_with_and_without_the_optional_outputs(basis, virial):
    """one call over all rows against the calls [0, a), [a, b), [b, n) that accumulate into one force array: basis and virial
    rows of a range at ii - row_begin (judged against the ORACLE's rows of that range), rows behind row_count and padding
    columns untouched (_design_call), with basis = NULL, virial = NULL and both.  A neighbour's force row receives one
    atomic add per entry, onto zero: bit-equal between all variants; centre rows collect LDS sums of four wavefronts"""
    c, want, whole = _run_case("ranges")
    st, n = c.st, len(c.st.ilist)
    a, b = _design.RANGE_CUTS
    cuts = [0, a, b, n]
    assert st.KL[0][0] == 0 and st.KL[a][0] == 0 and st.KL[a - 1][0] == 65 and st.KL[n - 1][0] == 65
    parts, force_t = [], None
    for lo, hi in zip(cuts, cuts[1:]):
        parts.append(_design_call(_ctx(c.pot), st, lo, hi - lo, basis=basis, virial=virial, force_t=force_t))
        force_t = parts[-1]["force_t"]
        _exact_rows_of_empty_stars(c, parts[-1], range(lo, hi))
    got = dict(force=parts[-1]["force"],
               basis=np.concatenate([p["basis"] for p in parts]) if basis else whole["basis"],
               virial=np.concatenate([p["virial"] for p in parts]) if virial else whole["virial"])
    _check_stars(None, st, got, "ranges, basis %s, virial %s" % (basis, virial), want=want)
    assert np.array_equal(got["force"][_outer(st)], whole["force"][_outer(st)]), "neighbour rows: one add each, bit-equal"
    assert np.abs(whole["force"][_outer(st)]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("form", _design.OWNER_FORMS)
def test_owner_map_given_identity_many_to_one_fold_and_neighbours_owned_by_their_centre(form):
    """(identity) the p.owner != NULL branch; (fold) outer atoms folded onto the centres plus SHARED_ROWS rows: many atomic
    adds per row, from several stars; (self) own == i for two in-cutoff neighbours in different tiles of a K = 33 star:
    both of their force terms are skipped, so their own rows stay exactly zero and the centre's row lacks their -G"""
    c, want, got = _run_case("owner-" + form)
    st, n = c.st, len(c.st.ilist)
    if form == "fold":
        assert c.nowned == n + _design.SHARED_ROWS and (c.owner[:c.nowned] == np.arange(c.nowned)).all()
        own = [c.owner[st.neigh[_stars.in_cutoff_entries(st, s)]] for s in range(n)]
        assert any(K == 65 and len(set(o)) < len(o) for (K, L), o in zip(st.KL, own)), "two neighbours of a three-tile star on one row"
        assert len(set(own[2]) & set(own[3])) > 0, "two stars on one owner row"
        assert all((o >= n).all() for o in own)
    if form == "self":
        s = [K for K, L in st.KL].index(33)
        e = _stars.in_cutoff_entries(st, s)
        js = st.neigh[e[[0, 32]]]
        assert (c.owner[js] == st.ilist[s]).all() and (c.owner != np.arange(st.nall)).sum() == 2
        assert not got["force"][js].any(), "the rows of neighbours owned by their centre"
        plain = _design.case_want("owner-identity")["f_all"]
        assert np.abs(plain[js]).max() > 1e-3 and np.abs(want["force"].reshape(plain.shape)[st.ilist[s]] - plain[st.ilist[s]]).max() > 1e-3


@pytest.mark.gpu
def test_list_entries_with_special_bond_bits_give_the_rows_of_the_clean_list():
    """& MTP_NEIGHMASK in compact_neighbours: the ids that reach the tiles, the owner lookup and the force rows are the
    masked ones"""
    c, want, clean = _run_case("bits")
    got = _design_call(_ctx(c.pot), c.st, neigh=_design.marked_list(c.st))
    _check_stars(None, c.st, got, "marked list", want=want)
    assert np.array_equal(got["force"][_outer(c.st)], clean["force"][_outer(c.st)]) and np.abs(clean["force"]).max() > 1e-3


@pytest.mark.gpu
def test_two_design_calls_on_one_context_the_second_keeps_nothing_of_the_first():
    h = _design.handles("W_L8.mtp")
    ctx = capi.Context(h.pot, 0)
    first = _train.star_set(h.tables, [(97, 129), (65, 66), (33, 33)], 76)
    _design_call(ctx, first)
    c = _design.star_case("second")
    assert sum(K == 0 for K, L in c.st.KL) == 2
    _run_case("second", ctx=ctx)


# ---- refusals: checked return paths of the kernel ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_owner_outside_the_owned_atoms_is_reported_and_the_flag_cleared():
    """one in-cutoff neighbour's owner equals nowned: the direction writes no force row (own_ok; the row address falls back
    to row 0 and is not used), flag 3 is raised, the synchronise reports MTP_ERR_ARG and clears the flag, and the next call,
    with the identity map given, agrees with the oracle"""
    c = _design.star_case("owner-identity")
    ctx = capi.Context(c.h.pot, 0)
    st = c.st
    s = [K for K, L in st.KL].index(33)
    bad = c.owner.copy()
    bad[st.neigh[_stars.in_cutoff_entries(st, s)[32]]] = c.nowned
    with pytest.raises(capi.MtpError, match="outside") as ei:
        _design_call(ctx, st, owner=bad, nowned=c.nowned)
    assert ei.value.code == -20
    _run_case("owner-identity", ctx=ctx)


@pytest.mark.gpu
def test_understated_max_numneigh_is_reported_not_overrun():
    """a device list of stars (9, 9), (3, 3) declared with max_numneigh = 8: cj_cap is 8 and the row keeps 9, so
    compact_neighbours stores 8 ids (pos < cj_cap), clips the count and raises flag 2; the synchronise reports
    MTP_ERR_LIMIT.  The same list with the honest length then gives the oracle's rows"""
    c = _design.star_case("understated")
    assert _stars.counts(c.st) == [(9, 9), (3, 3)]
    ctx = capi.Context(c.h.pot, 0)
    with pytest.raises(capi.MtpError, match="max_numneigh") as ei:
        _design_call(ctx, c.st, max_numneigh=8)
    assert ei.value.code == -24
    _run_case("understated", ctx=ctx, max_numneigh=9)


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
