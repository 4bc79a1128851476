"""The oracle, the product's parser and the .cfg writer against the COMPILED REFERENCE.

oracle/_ref/libmtp_ref.so is the reference's own `mtp` / `mtp/extrapolation` pair styles, compiled unchanged by
`make -C oracle ref` against the stand-in LAMMPS headers of tests/cpp/lammps_mock (oracle/pyref.py loads it).  The
oracle (oracle/mtp_oracle.c) claims the reference's operation order, both are built with -O2 -ffp-contract=off, so the
assertion is EXACT equality (np.array_equal) of every output: mathematics cannot pin conventions -- the order of the
species-pair blocks, `>` at the cutoff, what happens below min_dist, scaling, the layout of the candidate vector, the
natoms normalisation, which outputs a flag touches, the bytes of the .cfg -- and a running reference can.

Build policy: the library is built on demand here.  Where the reference's sources exist a failed build fails the tests;
the module skips only when neither the sources nor a library built elsewhere are there.

One reference behaviour is out of reach of a comparison and is avoided, not hidden: in neighbourhood mode the style keeps
`inum` grades but writes them by ATOM index, so a list naming an atom at or beyond inum makes it write past its array
(oracle/ref_driver.cpp refuses such a call).  Subset lists are therefore compared on the force path, and on the grade
path with a subset of the leading atoms only.
"""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system
from oracle import pyref
from oracle.pyoracle import Oracle

import _stars
import _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FORCE_KEYS = ("f", "eatom", "energy", "virial", "vatom")
GRADE_KEYS = ("grades", "max_grade", "coeff_ders")


@pytest.fixture(scope="module", autouse=True)
def _reference_library():
    if pyref.have_sources():
        pyref.build()                      # a failed build is a failed test
        assert pyref.available()
    elif not pyref.available():
        pytest.skip("neither the reference's sources nor oracle/_ref/libmtp_ref.so are here")


_PAIRS = {}


def _pair(path, ext=False):
    """(Reference, Oracle) of a file, loaded once"""
    key = (str(path), bool(ext))
    if key not in _PAIRS:
        _PAIRS[key] = (pyref.Reference(str(path), selection=ext), Oracle(str(path), selection=ext))
    return _PAIRS[key]


def _same(path, s, ext=False, grade=None, natoms=None, eflag=3, vflag=4, label=""):
    """one call through both judges, every output bit for bit; returns the reference's outputs"""
    grade = ext if grade is None else grade
    ref, orc = _pair(path, ext)
    n = len(s.ilist) if natoms is None else natoms
    a = ref.compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag, vflag, extrapolation=grade, natoms=n)
    b = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag, vflag, extrapolation=grade, natoms=n)
    for k in FORCE_KEYS + (GRADE_KEYS if grade else ()):
        assert np.array_equal(a[k], b[k]), "%s %s: oracle and reference differ by %.3e" % (
            label, k, np.abs(np.asarray(a[k]) - np.asarray(b[k])).max())
    assert np.isfinite(a["f"]).all()
    return a


def _system(ncell=(2, 2, 2), species=1, a=3.165, list_cutoff=6.0, seed=31):
    pos, box = mtpgen.bcc_lattice(*ncell, a=a, seed=seed)
    types = np.random.default_rng(5).integers(1, species + 1, size=len(pos)).astype(np.int32)
    return periodic_system(pos, box, types, list_cutoff)


# ---- committed files ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["W_L8_54", "W_L16_54", "WRe_L20_16", "W_L16_nbh_16", "WRe_L10_cfg_16"])
def test_committed_goldens_are_reference_outputs(name):
    """tests/golden/*.npz were written by the oracle; the compiled reference gives the same bits on the same inputs"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    ext = "grades" in g.files
    path = os.path.join(POT, str(g["potential"]))
    s = SimpleNamespace(x=g["x"], types=g["types"], ilist=g["ilist"], first=g["first"], neigh=g["neigh"])
    r = _same(path, s, ext, natoms=int(g["nlocal"]), label=name)
    for k in FORCE_KEYS + (GRADE_KEYS if ext else ()):
        assert np.array_equal(r[k], g[k]), k
    ref, orc = _pair(path, ext)
    assert ref.sizes == orc.sizes
    assert (ref.scaling, ref.min_cutoff, ref.max_cutoff) == (orc.m.scaling, orc.m.min_cutoff, orc.m.max_cutoff)
    assert ref.init_one(1, 1) == orc.m.max_cutoff
    if ext:
        assert ref.configuration_mode == orc.m.configuration_mode


# ---- table shapes ----------------------------------------------------------------------------------------------------


def test_level_4_short_line_buffer_is_mirrored(tmp_path):
    """The style sizes its reader's line buffer from the table (B * 20 + 20, then T * 32 + 20: 40 and 52 characters at
    level 4), so the 63-character moment_coeffs line of a level-4 file comes back in pieces and its second number is cut.
    The oracle and the product's parser mirror that on purpose (tests/test_gpu_parity.py::test_other_levels_and_species):
    all three read the SAME coefficients, which are not the file's."""
    path = str(tmp_path / "p.mtp")
    p = mtpgen.random_potential(mtpgen.build_table(4), 1, 4242)
    mtpgen.write_mtp(p, path)
    written = np.array([float("%.15e" % v) for v in p.moment_coeffs])
    read = Oracle(path).arr("linear_coeffs", 2)
    assert read[0] == written[0] and read[1] != written[1]
    assert np.array_equal(capi.Potential(path).tables()["moment_coeffs"], read)
    _same(path, _system((2, 2, 2)), label="level 4")         # ... and the reference computes with the same ones


@pytest.mark.parametrize("level,species", [(4, 1), (6, 1), (10, 3), (12, 2), (22, 1), (10, 4), (10, 5)])
def test_generated_levels_and_species(tmp_path, level, species):
    """with 3, 4 and 5 species every i-j radial block is distinct (random_potential draws them independently): a block
    taken as j-i, or a wrong stride of the pair offset, changes the forces"""
    path = str(tmp_path / "p.mtp")
    p = mtpgen.random_potential(mtpgen.build_table(level), species, 4242)
    assert len({p.radial_coeffs[k].tobytes() for k in range(species * species)}) == species * species
    mtpgen.write_mtp(p, path)
    s = _system((2, 2, 3) if species > 2 else (2, 2, 2), species=species)
    assert len(set(s.types[s.ilist])) == species
    _same(path, s, label="level %d, %d species" % (level, species))


@pytest.mark.parametrize("table,R,scaling,window", [
    (10, 1, 0.37, (2.9, 5.0)), (10, 2, 2.5, (1.4, 6.2)), (16, 3, 2.5, (2.9, 5.0)), (16, 7, 0.37, (1.4, 6.2)),
    (16, 9, 2.5, (1.4, 6.2)), ("wide", 16, 0.37, (2.9, 5.0)), ("wide", 9, 2.5, (1.4, 6.2))])
def test_radial_windows(tmp_path, table, R, scaling, window):
    """the R, scaling, min_dist and max_dist cases of tests/test_gpu_shapes.py::test_radial_basis"""
    path = str(tmp_path / "p.mtp")
    if table == "wide":
        tab, nfac = _tables.make_table(*_tables.shape_table(64, 2, 8))
        _tables.write(tab, nfac, path, species=2, R=R, scaling=scaling, min_dist=window[0], max_dist=window[1])
    else:
        mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(table), 2, 4242, window[0], window[1], R, scaling),
                         path)
    ref, orc = _pair(path)
    assert ref.scaling == scaling == orc.m.scaling and (ref.min_cutoff, ref.max_cutoff) == window
    s = _system((2, 2, 2), species=2, list_cutoff=window[1] + 1.0)
    r = _same(path, s, label="R %d scaling %g" % (R, scaling))
    assert np.abs(r["f"]).max() > 1e-6


# ---- geometry ----------------------------------------------------------------------------------------------------------

# a few dozen stars: empty rows, rows wholly outside the cutoff, one neighbour, odd counts, more than a tile
STAR_KL = [(0, 0), (0, 5), (1, 1), (1, 9), (2, 2), (3, 7), (5, 5), (17, 30), (33, 40), (0, 1), (4, 4), (31, 31)]
GEOM_POTS = {"L16": ("W_L16.mtp", 1, False), "L20": ("WRe_L20.mtp", 2, False), "L16nbh": ("W_L16_nbh.almtp", 1, True),
             "L10cfg": ("WRe_L10_cfg.almtp", 2, True)}


def _star_kinds():
    from test_gpu_geometry import DISTANCES
    kinds = dict(DISTANCES)
    kinds["plain"] = {}
    return kinds


@pytest.mark.parametrize("kind", ["plain", "exact_cutoff", "below_min_dist", "offset_1e5", "offset_negative"])
@pytest.mark.parametrize("name", list(GEOM_POTS))
def test_star_and_distance_edges(name, kind):
    """exact_cutoff: one entry per star at r^2 == r_c^2 bit-exact (inside: the reference drops r^2 > r_c^2 only) and one
    a representable step beyond (outside); below_min_dist: shells down to 0.5 min_dist; offsets of +-1e5 A; rows with
    K = 0, and rows whose every listed atom is outside"""
    fn, species, ext = GEOM_POTS[name]
    rng = np.random.default_rng(23)
    for order in ("mixed", "back"):
        st = _stars.stars(STAR_KL, rng, species=species, order=order, **_star_kinds()[kind])
        assert _stars.counts(st) == STAR_KL
        if kind == "exact_cutoff":
            d = st.x[st.neigh] - np.repeat(st.x[st.ilist], np.diff(st.first), axis=0)
            assert ((d * d).sum(1) == 25.0).sum() == sum(1 for K, _ in STAR_KL if K > 0)
        if kind == "below_min_dist":
            d = st.x[st.neigh] - np.repeat(st.x[st.ilist], np.diff(st.first), axis=0)
            assert np.sqrt((d * d).sum(1)).min() < 1.5
        # star centres are not the leading atoms: the grade path takes the force call only (see the module docstring)
        _same(os.path.join(POT, fn), st, ext, grade=False, label="%s %s %s" % (name, kind, order))


def _leading_stars(KL, rng, species, **kw):
    """the same stars with the centres renumbered to 0 .. n-1 (what LAMMPS does: owned atoms first), so that the
    reference's grade array, indexed by atom, holds them"""
    st = _stars.stars(KL, rng, species=species, **kw)
    n = len(st.ilist)
    rest = np.setdiff1d(np.arange(st.nall), st.ilist)
    order = np.concatenate([st.ilist, rest])                 # new -> old
    new_of = np.empty(st.nall, np.int64)
    new_of[order] = np.arange(st.nall)
    return SimpleNamespace(x=np.ascontiguousarray(st.x[order]), types=st.types[order],
                                  ilist=np.arange(n, dtype=np.int32), first=st.first,
                                  neigh=new_of[st.neigh].astype(np.int32), nall=st.nall, KL=st.KL)


@pytest.mark.parametrize("kind", ["plain", "exact_cutoff", "below_min_dist"])
@pytest.mark.parametrize("name", ["L16nbh", "L10cfg"])
def test_star_edges_on_the_grade_path(name, kind):
    fn, species, ext = GEOM_POTS[name]
    st = _leading_stars(STAR_KL, np.random.default_rng(29), species, **_star_kinds()[kind])
    r = _same(os.path.join(POT, fn), st, True, label="%s %s grades" % (name, kind))
    if name == "L16nbh":
        assert (r["grades"][: len(st.ilist)] > 0).all()      # an empty neighbourhood still has its species entry


def test_lists_subset_empty_ghosts_and_high_bits():
    path = os.path.join(POT, "WRe_L20.mtp")
    s = _system((2, 2, 2), species=2)
    assert s.nall > len(s.ilist)                                               # ghost neighbours
    full = _same(path, s, label="full list")
    assert np.abs(full["f"][len(s.ilist):]).max() > 0                          # ... which receive force
    # a subset ilist: every third row, in descending order
    rows = np.arange(len(s.ilist))[::3][::-1]
    first = np.concatenate([[0], np.cumsum([s.first[r + 1] - s.first[r] for r in rows])]).astype(np.int32)
    neigh = np.concatenate([s.neigh[s.first[r]:s.first[r + 1]] for r in rows]).astype(np.int32)
    sub = SimpleNamespace(x=s.x, types=s.types, ilist=s.ilist[rows], first=first, neigh=neigh)
    r = _same(path, sub, label="subset list")
    assert not np.array_equal(r["f"], full["f"]) and (r["eatom"][np.setdiff1d(s.ilist, sub.ilist)] == 0).all()
    # an empty ilist
    none = SimpleNamespace(x=s.x, types=s.types, ilist=np.zeros(0, np.int32), first=np.zeros(1, np.int32),
                                  neigh=np.zeros(0, np.int32))
    r = _same(path, none, label="empty list")
    assert not r["f"].any() and r["energy"] == 0.0
    # bits above NEIGHMASK (LAMMPS' special-bond bits 30 and 31 of the entry; 29 is the top bit of NEIGHMASK's complement)
    bits = (np.arange(len(s.neigh)) % 4).astype(np.uint32) << 30
    hi = SimpleNamespace(x=s.x, types=s.types, ilist=s.ilist, first=s.first,
                                neigh=(s.neigh.astype(np.uint32) | bits).view(np.int32))
    assert (hi.neigh < 0).any() and (hi.neigh != s.neigh).any()
    r = _same(path, hi, label="special bits")
    for k in FORCE_KEYS:
        assert np.array_equal(r[k], full[k]), k
    # the grade path on a subset of the leading rows (neighbourhood and configuration mode)
    for fn, sp in (("W_L16_nbh.almtp", 1), ("WRe_L10_cfg.almtp", 2)):
        s = _system((2, 2, 2), species=sp)
        m = len(s.ilist) // 2
        head = SimpleNamespace(x=s.x, types=s.types, ilist=s.ilist[:m], first=s.first[:m + 1],
                                      neigh=s.neigh[:s.first[m]])
        _same(os.path.join(POT, fn), head, True, natoms=len(s.ilist), label="leading subset, grades")


# ---- flags -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ext", [False, True], ids=["mtp", "extrapolation"])
@pytest.mark.parametrize("vflag", [0, 1, 4, 5])
@pytest.mark.parametrize("eflag", [0, 1, 2, 3])
def test_flags(eflag, vflag, ext):
    """What a flag combination tallies is equal; what it does not tally is left as handed in, by both.  (LAMMPS zeroes an
    accumulator that the call tallies -- Pair::ev_setup -- where the oracle's caller does: compared from zero, then with
    every output pre-filled.)  The global virial is tallied on the raw vflag (pair_mtp.cpp:257), vflag = 4 included."""
    path = os.path.join(POT, "W_L16_nbh.almtp" if ext else "WRe_L20.mtp")
    s = _system((2, 2, 2), species=1 if ext else 2)
    r = _same(path, s, ext, eflag=eflag, vflag=vflag, label="eflag %d vflag %d" % (eflag, vflag))
    assert (r["energy"] != 0) == bool(eflag & 1) and r["eatom"].any() == bool(eflag & 2)
    assert r["virial"].any() == bool(vflag) and r["vatom"].any() == bool(vflag & 4)
    ref, orc = _pair(path, ext)
    fill = 7.25
    for judge in (ref, orc):
        o = judge.compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag, vflag, extrapolation=ext, natoms=len(s.ilist),
                          prefill=fill)
        assert np.array_equal(o["f"], r["f"])
        untouched = dict(energy=not eflag & 1, eatom=not eflag & 2, virial=not vflag, vatom=not vflag & 4)
        for k, keep in untouched.items():
            if keep:
                assert (np.asarray(o[k]) == fill).all(), (k, type(judge).__name__)
        if ext:
            for k in GRADE_KEYS:
                assert np.array_equal(o[k], r[k]), k


# ---- grade path ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("natoms", ["inum", "larger", "zero"])
@pytest.mark.parametrize("fn,species", [("W_L16_nbh.almtp", 1), ("WRe_L10_cfg.almtp", 2)])
def test_natoms_normalisation(fn, species, natoms):
    """configuration mode: max |A^-1 c| / natoms with the GLOBAL atom count, 0 when that is 0; neighbourhood mode does
    not look at natoms"""
    s = _system((2, 2, 2), species=species)
    n = {"inum": len(s.ilist), "larger": 3 * len(s.ilist) + 1, "zero": 0}[natoms]
    r = _same(os.path.join(POT, fn), s, True, natoms=n, label=natoms)
    base = _same(os.path.join(POT, fn), s, True, natoms=len(s.ilist))
    assert r["pvector0"] == r["max_grade"]
    if species == 1:
        assert r["max_grade"] == base["max_grade"] > 0
    elif n == 0:
        assert r["max_grade"] == 0.0 and base["max_grade"] > 0
    else:
        assert r["max_grade"] == base["max_grade"] * len(s.ilist) / n or abs(
            r["max_grade"] * n - base["max_grade"] * len(s.ilist)) < 1e-12 * base["max_grade"] * len(s.ilist)


def test_extrapolation_flag_off_and_extract_peratom():
    """extract("extrapolation_flag") off: the extrapolation style runs the plain force call; pvector[0] keeps the last
    grade.  extract_peratom("extrapolation"): a per-atom vector in neighbourhood mode, an error in configuration mode
    (the oracle has no such entry point: its grades array stays zero in configuration mode)."""
    s = _system((2, 2, 2))
    path = os.path.join(POT, "W_L16_nbh.almtp")
    ref, orc = _pair(path, True)
    assert ref.set_extrapolation_flag(False) and not pyref.Reference(os.path.join(POT, "W_L16.mtp")).set_extrapolation_flag(True)
    off = _same(path, s, True, grade=False, label="flag off")
    plain = _same(os.path.join(POT, "W_L16.mtp"), s, label="plain")
    on = _same(path, s, True, label="flag on")
    for k in FORCE_KEYS:
        assert np.array_equal(off[k], on[k]), k
    assert ref.extract_peratom() == 0
    s2 = _system((2, 2, 2), species=2)
    cpath = os.path.join(POT, "WRe_L10_cfg.almtp")
    cref, _ = _pair(cpath, True)
    r = _same(cpath, s2, True, label="configuration mode")
    assert not r["grades"].any()
    with pytest.raises(pyref.ReferenceError_, match="MLIP-3 style extrapolation for configuration mode"):
        cref.extract_peratom()
    assert plain["energy"] != 0


def _almtp_variant(tmp_path, name, edit):
    raw = open(os.path.join(POT, "W_L16_nbh.almtp"), "rb").read()
    cut = raw.index(b"#MVS_v1.1")
    end = raw.index(b"#", cut + 1)
    head = edit(raw[cut:end].decode())
    path = str(tmp_path / (name + ".almtp"))
    with open(path, "wb") as fh:
        fh.write(raw[:cut] + head.encode() + raw[end:])
    return path


ALMTP_HEADERS = {
    "as_written": (lambda h: h, True),
    "weights_as_floats": (lambda h: h.replace("site_en_weight = 1", "site_en_weight = 1.0"), True),
    "comment_after_header": (lambda h: h.replace("force_weight = 0", "force_weight = 0 # unused"), True),
    "wrong_mvs_version": (lambda h: h.replace("#MVS_v1.1", "#MVS_v1.0"), False),
    "both_weights": (lambda h: h.replace("energy_weight = 0", "energy_weight = 1"), False),
    "missing_stress_weight": (lambda h: h.replace("stress_weight = 0\n", ""), False),
}


@pytest.mark.parametrize("case", list(ALMTP_HEADERS))
def test_almtp_header_lines(tmp_path, case):
    edit, ok = ALMTP_HEADERS[case]
    path = _almtp_variant(tmp_path, case, edit)
    s = _system((2, 2, 2))
    if ok:
        r = _same(path, s, True, label=case)
        base = _same(os.path.join(POT, "W_L16_nbh.almtp"), s, True)
        assert np.array_equal(r["grades"], base["grades"])
        assert capi.Potential(path, selection=True).info.configuration_mode == 0
    else:
        with pytest.raises(pyref.ReferenceError_):
            pyref.Reference(path, selection=True)
        with pytest.raises(RuntimeError):
            Oracle(path, selection=True)
        with pytest.raises(capi.MtpError):
            capi.Potential(path, selection=True)


def test_plain_file_has_no_selection_state():
    path = os.path.join(POT, "W_L16.mtp")
    with pytest.raises(pyref.ReferenceError_, match="No selection state found"):
        pyref.Reference(path, selection=True)
    with pytest.raises(RuntimeError, match="No selection state found"):
        Oracle(path, selection=True)
    with pytest.raises(capi.MtpError, match="No selection state found"):
        capi.Potential(path, selection=True)


# ---- other ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("who", ["centre", "neighbour"])
def test_type_beyond_species_count_is_an_error_in_both(ext, who):
    path = os.path.join(POT, "W_L16_nbh.almtp" if ext else "W_L16.mtp")
    s = _system((2, 2, 2))
    types = s.types.copy()
    ghost = int(s.neigh[s.neigh >= len(s.ilist)][0])
    types[0 if who == "centre" else ghost] = 2                 # an owned centre / a ghost that is only ever a neighbour
    ref, orc = _pair(path, ext)
    with pytest.raises(pyref.ReferenceError_, match="Too few species count in the MTP potential!"):
        ref.compute(s.x, types, s.ilist, s.first, s.neigh, extrapolation=ext)
    with pytest.raises(RuntimeError, match="rc=-1"):
        orc.compute(s.x, types, s.ilist, s.first, s.neigh, extrapolation=ext)


@pytest.mark.parametrize("threads", [1, 3])
def test_threaded_oracle_against_the_reference(threads):
    """Oracle.compute_mt at the tolerances of tests/test_oracle.py::test_threaded_oracle_matches_serial_oracle"""
    path = os.path.join(POT, "WRe_L20.mtp")
    s = _system((2, 2, 2), species=2)
    ref, orc = _pair(path)
    a = ref.compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)
    b = orc.compute_mt(threads, s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)
    assert np.abs(a["f"] - b["f"]).max() <= 1e-12 * max(1.0, np.abs(a["f"]).max())
    assert np.array_equal(a["eatom"], b["eatom"])
    assert abs(a["energy"] - b["energy"]) <= 1e-11 * max(1.0, abs(a["energy"]))
    assert np.abs(a["virial"] - b["virial"]).max() <= 1e-10 * max(1.0, np.abs(a["virial"]).max())
    assert np.abs(a["vatom"] - b["vatom"]).max() <= 1e-12 * max(1.0, np.abs(a["vatom"]).max())


# ---- parser ----------------------------------------------------------------------------------------------------------------


def _base_text(tmp_path):
    path = str(tmp_path / "base.mtp")
    p = mtpgen.random_potential(mtpgen.build_table(6), 2, 77)
    p.name = "small"
    mtpgen.write_mtp(p, path)
    return open(path).read()


def _sub(old, new):
    def edit(t):
        assert old in t, old
        return t.replace(old, new, 1)
    return edit


def _shorten_basic(t):
    lines = t.split("\n")
    k = next(i for i, l in enumerate(lines) if l.startswith("alpha_index_basic ="))
    lines[k] = lines[k][: lines[k].rindex(", {")] + "}"
    return "\n".join(lines)


def _blanks_but_version(t):
    return "\n".join(l if l.startswith("version") else l + "  \t" for l in t.split("\n"))


# name -> (edit of the file's text, what the reference does, note)
PARSER = {
    "as_written": (lambda t: t, "accept"),
    "no_potential_name": (_sub("potential_name = small\n", ""), "accept"),
    "potential_name_without_value": (_sub("potential_name = small\n", "potential_name = \n"), "accept"),
    "no_potential_tag": (_sub("potential_tag = \n", ""), "accept"),
    "potential_tag_with_value": (_sub("potential_tag = \n", "potential_tag = trained\n"), "accept"),
    "scaling_line": (_sub("species_count", "scaling = 2.5e+00\nspecies_count"), "accept"),
    "scaling_in_the_basis_block": (_sub("\tmin_dist", "\tscaling = 3.0\n\tmin_dist"), "accept"),      # read, overwritten by 1
    "min_val_max_val": (lambda t: t.replace("min_dist", "min_val").replace("max_dist", "max_val"), "accept"),
    "trailing_blanks": (_blanks_but_version, "accept"),
    "comments_and_empty_lines": (_sub("species_count = 2\n", "\n# a comment line\nspecies_count = 2   # two species\n\n"),
                                 "accept"),
    "wrong_version": (_sub("version = 1.1.0", "version = 1.0.0"), "reject"),
    "blank_after_version": (_sub("version = 1.1.0\n", "version = 1.1.0 \n"), "reject"),      # compared with its newline
    "crlf": (lambda t: t.replace("\n", "\r\n"), "reject"),                                   # ... so CRLF fails there
    "wrong_first_word": (_sub("MTP\n", "MTPX\n"), "reject"),
    "unknown_basis_type": (_sub("RBChebyshev", "RBShapeev"), "reject"),
    "magnetic_basis": (_sub("\tradial_coeffs\n", "\tmagnetic_basis_type = BChebyshev\n\tradial_coeffs\n"), "reject"),
    "radial_funcs_count_too_large": (lambda t: t.replace("radial_funcs_count = ", "radial_funcs_count = 1"), "reject"),
    "alpha_index_basic_short": (_shorten_basic, "reject"),
    "no_species_count": (_sub("species_count = 2\n", ""), "reject"),
    "no_max_dist": (lambda t: "\n".join(l for l in t.split("\n") if "max_dist" not in l), "reject"),
}
# (blank_after_version, crlf: the reference compares the version line with "version = 1.1.0\n" byte for byte, so a file
# saved with CRLF line ends or a blank after the version cannot be loaded; the product and the oracle do the same.  No
# case was found where the product is stricter or looser than the reference.)


@pytest.mark.parametrize("case", list(PARSER))
def test_parser_variants(tmp_path, case):
    """a file the reference accepts is accepted by the oracle and by the product's parser, with equal sizes, cutoffs and
    scaling and, through the oracle, equal forces; a file the reference rejects is rejected by the product with an
    error code (and by the oracle)"""
    edit, verdict = PARSER[case]
    base = _base_text(tmp_path)
    path = str(tmp_path / (case + ".mtp"))
    with open(path, "w", newline="") as fh:
        fh.write(edit(base))
    if verdict == "accept":
        ref = pyref.Reference(path)
        orc = Oracle(path)
        pot = capi.Potential(path)
        sizes = {k: v for k, v in pot.sizes.items() if k != "levels"}
        assert ref.sizes == orc.sizes == sizes
        assert ref.scaling == orc.m.scaling == pot.info.scaling == (2.5 if case == "scaling_line" else 1.0)
        assert (ref.min_cutoff, ref.max_cutoff) == (orc.m.min_cutoff, orc.m.max_cutoff) == (
            pot.info.min_cutoff, pot.info.max_cutoff) == (2.0, 5.0)
        said = "The scaling is : %.2e.\nThere are 2 species.\n" % ref.scaling
        assert ref.log == said + ("MTP Scaling Value = 3 " if case == "scaling_in_the_basis_block" else "")
        s = _system((2, 2, 2), species=2)
        r = _same(path, s, label=case)
        if case not in ("as_written", "scaling_line"):
            with open(str(tmp_path / "again.mtp"), "w") as fh:
                fh.write(base)
            b = _same(str(tmp_path / "again.mtp"), s)
            for k in FORCE_KEYS:
                assert np.array_equal(r[k], b[k]), k
        tabs = pot.tables()
        n = ref.sizes["Sp"] ** 2 * ref.sizes["Mu"] * ref.sizes["R"]
        assert np.array_equal(tabs["radial_coeffs"], orc.arr("radial_basis_coeffs", n))
        assert np.array_equal(tabs["moment_coeffs"], orc.arr("linear_coeffs", ref.sizes["S"]))
        assert np.array_equal(tabs["species_coeffs"], orc.arr("species_coeffs", ref.sizes["Sp"]))
    else:
        with pytest.raises(pyref.ReferenceError_):
            pyref.Reference(path)
        with pytest.raises(capi.MtpError) as ei:
            capi.Potential(path)
        assert ei.value.code < 0
        with pytest.raises(RuntimeError):
            Oracle(path)


# ---- .cfg writer and log lines -------------------------------------------------------------------------------------------

EXE = os.path.join(ROOT, "tests", "cpp", "test_pair_host")


def _write_system(path, s):
    with open(path, "w") as fh:
        fh.write("%d %d %.17g %.17g %.17g\n" % (s.nlocal, s.nall, *s.box))
        for (x, y, z), t in zip(s.x, s.types):
            fh.write("%.17g %.17g %.17g %d\n" % (x, y, z, t))
        for i in range(s.nlocal):
            row = s.neigh[s.first[i]:s.first[i + 1]]
            fh.write("%d %s\n" % (len(row), " ".join(map(str, row))))


@pytest.mark.parametrize("cfg_mode", [0, 1])
def test_cfg_writer_and_log_lines_against_the_reference(tmp_path, cfg_mode):
    """host/mtp_cfg_writer.hpp through tests/cpp/test_pair_host `cfg` (1-, 2- and 3-rank jobs, tilted cell) against the
    reference's own write_config on the same atoms, grades and Domain values, byte for byte; and the utils::logmesg
    lines of settings().  tests/test_pair_host.py spells the same expectations out by hand: two independent judges."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "host")])
    pos, box = mtpgen.bcc_lattice(2, 2, 3)
    types = np.random.default_rng(8).integers(1, 3, len(pos)).astype(np.int32)
    s = periodic_system(pos, box, types, 4.0)
    sysf = str(tmp_path / "sys.txt")
    _write_system(sysf, s)
    r = subprocess.run([EXE, "cfg", sysf, str(tmp_path), str(cfg_mode)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n = s.nlocal
    x = np.array([[float(v) for v in l.split()[:3]] for l in open(sysf).read().split("\n")[1:1 + n]])   # as the driver reads them
    grades = np.array([0.37 * i + 1.0 / (i + 3.0) for i in range(n)])
    out = str(tmp_path / "ref.cfg")
    potf = os.path.join(POT, "WRe_L10_cfg.almtp" if cfg_mode else "W_L16_nbh.almtp")
    ref = pyref.Reference(potf, mlip3=(out, "2.0", "10.5"))
    assert ref.configuration_mode == cfg_mode
    ref.write_config(x, s.types[:n], grades, 3.14159265, n, [s.box[0], s.box[1], s.box[2], 0.25, -0.5, 0.125])
    want = open(out, "rb").read()
    for ranks in (1, 2, 3):
        assert open(tmp_path / ("cfg_%d.cfg" % ranks), "rb").read() == want, ranks
    assert want.startswith(b"BEGIN_CFG\nSize\n%d\nSupercell\n" % n) and want.endswith(b"END_CFG\n\n")
    ref.write_config(x, s.types[:n], grades, 3.14159265, n, [s.box[0], s.box[1], s.box[2], 0.25, -0.5, 0.125])
    assert open(out, "rb").read() == want + want                       # records are appended
    # log lines: the driver prints scaling(1.0), species(2), the MLIP-3 scheme line (neighbourhood, 2.0, 10.5) and the
    # plain mode line (configuration); the reference says them when it loads such files in such forms
    nbh = pyref.Reference(os.path.join(POT, "W_L16_nbh.almtp"), mlip3=(str(tmp_path / "x.cfg"), "2.0", "10.5")).log
    cfg = pyref.Reference(os.path.join(POT, "WRe_L10_cfg.almtp"), selection=True).log
    nbh, cfg = nbh.splitlines(True), cfg.splitlines(True)
    assert len(nbh) == 3 and len(cfg) == 3 and nbh[1] == "There are 1 species.\n"
    assert r.stdout == cfg[0] + cfg[1] + nbh[2] + cfg[2]


@pytest.mark.parametrize("fn,species", [("W_L16_nbh.almtp", 1), ("WRe_L10_cfg.almtp", 2)])
def test_mlip3_form_thresholds_file_and_break_message(tmp_path, fn, species):
    """the four-argument form end to end: grades on every call, a record when max_grade >= select, the run ended with the
    reference's message when max_grade >= break; outputs equal to the oracle's grade call"""
    path = os.path.join(POT, fn)
    s = _system((2, 2, 2), species=species)
    n = len(s.ilist)
    want = Oracle(path, selection=True).compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=n)
    mg = want["max_grade"]
    dom = [6.33, 6.33, 6.33, 0.25, -0.5, 0.125]
    quiet = pyref.run_mlip3(path, str(tmp_path / "a.cfg"), 2 * mg, 4 * mg, dom, s.x, s.types, s.ilist, s.first, s.neigh)
    assert quiet["cfg"] == b"" and quiet["error"] == ""
    for k in FORCE_KEYS + GRADE_KEYS:
        assert np.array_equal(quiet["out"][k], want[k]), k
    sel = pyref.run_mlip3(path, str(tmp_path / "b.cfg"), 0.5 * mg, 4 * mg, dom, s.x, s.types, s.ilist, s.first, s.neigh)
    rec = sel["cfg"].decode().split("\n")
    assert sel["error"] == "" and rec[:4] == ["BEGIN_CFG", "Size", str(n), "Supercell"]
    assert rec[4:7] == ["6.330000 0.000000 0.000000", "0.250000 6.330000 0.000000", "-0.500000 0.125000 6.330000"]
    rows = [l.split("\t") for l in rec[8:8 + n]]
    assert [r[:5] for r in rows] == [[str(i + 1), str(s.types[i] - 1)] + ["%.6f" % v for v in s.x[i]] for i in range(n)]
    if species == 1:
        assert [r[5] for r in rows] == ["%.5f" % g for g in want["grades"][:n]]
    else:
        assert all(len(r) == 5 for r in rows)
    assert rec[8 + n:] == ["Feature   MV_grade\t%.6f" % mg, "END_CFG", "", ""]
    assert sel["log"].splitlines()[2] == ("Extrapolation Scheme: %s mode, with a selection threshold of %s and break "
                                          "threshold of %s." % ("Neighborhood" if species == 1 else "Configuration",
                                                                repr(0.5 * mg), repr(4 * mg)))
    brk = pyref.run_mlip3(path, str(tmp_path / "c.cfg"), 0.5 * mg, 0.9 * mg, dom, s.x, s.types, s.ilist, s.first, s.neigh)
    assert brk["error"] == "ERROR on proc 0: Exceeded Break Threshold: %.5f. Terminating simulation.\n" % mg
    assert brk["cfg"] == sel["cfg"]                                    # written and flushed before the run ends


# ---- the committed reference fixtures ------------------------------------------------------------------------------------

FIXTURES = os.path.join(GOLDEN, "ref")


def test_reference_fixture_set_is_complete_and_small():
    from golden import make_reference_golden as mk
    names = sorted(f[:-4] for f in os.listdir(FIXTURES) if f.endswith(".npz"))
    assert names == sorted(mk.CASES)
    for n in names:
        assert os.path.getsize(os.path.join(FIXTURES, n + ".npz")) <= 22 * 1024, n


@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(FIXTURES) if f.endswith(".npz")))
def test_compiled_reference_reproduces_every_fixture(tmp_path, name):
    """tests/golden/ref/*.npz (the judge of tests/test_gpu_reference.py) are what the compiled reference gives, bit for
    bit -- and what the oracle gives"""
    from golden.make_reference_golden import potential_path
    g = np.load(os.path.join(FIXTURES, name + ".npz"))
    sel = bool(g["selection"])
    path = potential_path(g, tmp_path)
    s = SimpleNamespace(x=g["x"], types=g["types"], ilist=g["ilist"], first=g["first"], neigh=g["neigh"])
    r = _same(path, s, sel, natoms=int(g["natoms"]), label=name)
    for k in FORCE_KEYS + (GRADE_KEYS if sel else ()):
        assert np.array_equal(r[k], g[k]), k
    assert len(g["sid"]) == len(g["x"]) and (g["sid"][g["ilist"]] == np.arange(len(g["ilist"]))).all()
