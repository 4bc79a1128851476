"""Shared by the design-row tests (tests/test_design_cpu.py, tests/test_design_gpu.py): the judge of every entry of a
design matrix is the reference algorithm itself, by linearity.  Column Sp + a of the design matrix of a system is the
oracle's {energy, folded forces, virial} for the same potential with species_coeffs = 0 and moment_coeffs = e_a; column t
is the same with species_coeffs = e_t and moment_coeffs = 0.  The coefficients are set in place through the oracle's
Model.linear_coeffs / species_coeffs pointers and restored afterwards."""
import functools
import os
import tempfile
from types import SimpleNamespace

import numpy as np

import _cells
import _stars
import _tables
import _train
from lammps_mtp_kokkos_amd.driver import periodic_system_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")


def oracle_columns(orc, x, types, ilist, first, neigh, owner=None, nlocal=None):
    """dict(energy [cols], force [3 nlocal, cols], virial [6, cols], vatom [nall, 6, cols], f_all [nall, 3, cols], eatom
    [nall, cols]) of
    one system, one oracle call per column.  owner: the owned row of every row of x (None: identity, nlocal = nall)."""
    Sp, S = orc.m.species_count, orc.m.alpha_scalar_count
    nall = len(x)
    owner = np.arange(nall) if owner is None else np.asarray(owner)
    nlocal = nall if nlocal is None else nlocal
    lin, spc = orc.m.linear_coeffs, orc.m.species_coeffs
    keep_l, keep_s = [lin[k] for k in range(S)], [spc[k] for k in range(Sp)]
    out = dict(energy=np.zeros(Sp + S), force=np.zeros((3 * nlocal, Sp + S)), virial=np.zeros((6, Sp + S)),
               vatom=np.zeros((nall, 6, Sp + S)), f_all=np.zeros((nall, 3, Sp + S)), eatom=np.zeros((nall, Sp + S)))
    try:
        for k in range(S):
            lin[k] = 0.0
        for k in range(Sp):
            spc[k] = 0.0
        for col in range(Sp + S):
            ptr, k = (spc, col) if col < Sp else (lin, col - Sp)
            ptr[k] = 1.0
            r = orc.compute(x, types, ilist, first, neigh)
            ptr[k] = 0.0
            f = np.zeros((nlocal, 3))
            np.add.at(f, owner, r["f"])
            out["energy"][col] = r["energy"]
            out["force"][:, col] = f.reshape(-1)
            out["virial"][:, col] = r["virial"]
            out["vatom"][:, :, col] = r["vatom"]
            out["f_all"][:, :, col] = r["f"]
            out["eatom"][:, col] = r["eatom"]
    finally:
        for k in range(S):
            lin[k] = keep_l[k]
        for k in range(Sp):
            spc[k] = keep_s[k]
    return out


def oracle_cell_columns(orc, pos, cell, types, list_cutoff=_cells.LIST_CUTOFF):
    """(oracle_columns of a periodic cell through the numpy twin of the device ghost build, the driver.System)"""
    s = periodic_system_cell(pos, cell, types, list_cutoff)
    return oracle_columns(orc, s.x, s.types, s.ilist, s.first, s.neigh, s.owner, s.nlocal), s


def column_ratio(got, want):
    """worst |got - want| / (1e-9 + 1e-10 max |column|) over the entries of a matrix whose LAST axis is the column; the
    scale of a column is taken over all of its entries in `want`"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    w = want.reshape(-1, want.shape[-1])
    scale = np.abs(w).max(0)
    ratio = np.abs(got.reshape(w.shape) - w) / (1e-9 + 1e-10 * scale)
    return float(ratio.max())


def check_columns(got, want, what, kinds=("energy", "force", "virial")):
    """every entry within 1e-9 + 1e-10 max |column|, each kind of row (energy, force, virial) judged with the column's
    maximum over the rows of ITS OWN kind -- the rule of tests/_batch.close per array, per column --, so that large energy
    or virial entries cannot loosen the bound of the force rows; prints how far inside the bound each kind lands and
    returns the worst ratio"""
    worst = 0.0
    for k in kinds:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        ratio = column_ratio(g, w)
        print("%s %s: worst error / bound %.3e" % (what, k, ratio))
        assert np.isfinite(g).all() and ratio <= 1.0, "%s %s: misses 1e-9 + 1e-10 max|column| %.2f-fold" % (what, k, ratio)
        worst = max(worst, ratio)
    return worst


def star_ratios(st, got, want, per_star=True):
    """the rule of test_design_gpu._check_stars: dict(basis, force, virial) of error / bound per star, each kind with the
    column's maximum over the star's own rows of that kind, so that a three-tile star cannot hide a one-neighbour one.
    got: dict(basis [stars, cols], force [owned atoms, 3, cols], virial [stars, 6, cols]); want: oracle_columns.
    per_star = False (an owner map that folds atoms of several stars onto one row): the force rows are judged once, with
    the column's scale over all owned rows, and every star carries that figure.  A non-finite entry gives inf."""
    n, ncol = len(st.ilist), want["energy"].size
    wf = want["force"].reshape(-1, 3, ncol)
    assert got["basis"].shape == (n, ncol) and got["virial"].shape == (n, 6, ncol) and got["force"].shape == wf.shape, (
        got["basis"].shape, got["virial"].shape, got["force"].shape, wf.shape)

    def ratio(g, w):
        return column_ratio(g, w) if np.isfinite(g).all() else np.inf

    out = dict(basis=np.zeros(n), force=np.zeros(n), virial=np.zeros(n))
    bounds = None if not per_star else list(st.start) + [st.nall]
    for s in range(n):
        c = st.ilist[s]
        out["basis"][s] = ratio(got["basis"][s][None, :], want["eatom"][c][None, :])
        out["virial"][s] = ratio(got["virial"][s], want["vatom"][c])
        if per_star:
            a, b = bounds[s], bounds[s + 1]
            out["force"][s] = ratio(got["force"][a:b].reshape(-1, ncol), wf[a:b].reshape(-1, ncol))
    if not per_star and n:
        out["force"][:] = ratio(got["force"].reshape(-1, ncol), wf.reshape(-1, ncol))
    return out


# ---- the star sets of the design kernel's edge tests: tests/test_design_gpu.py runs the kernel on them, tests/test_design_cpu.py
# the numpy twin and damaged copies of its output.  Built once, shared, never written to. -----------------------------------
LEVEL8_MODES = [(None, "mixed"), ("edge", "mixed"), (None, "straddle")]
# K = 0, 1, 33 and 65 mixed; the cuts make a K = 0 row the first and a three-tile row the last of a range
RANGE_KL = [(0, 2), (1, 3), (33, 40), (65, 70), (0, 0), (1, 1), (33, 33), (65, 129), (1, 5), (33, 64), (0, 1), (65, 66)]
RANGE_CUTS = (4, 10)
OWNER_FORMS = ("identity", "fold", "self")
SHARED_ROWS = 8
BITS_KL = [(0, 1), (1, 2), (33, 40), (5, 9), (2, 2)]
SECOND_KL = [(0, 3), (1, 2), (33, 40), (2, 2), (64, 70), (0, 0)]
UNDERSTATED_KL = [(9, 9), (3, 3)]
SPECIAL_BITS = np.int32(-2 ** 31 + 2 ** 30)                      # the top two bits of a list entry


@functools.lru_cache(maxsize=None)
def handles(name):
    """namespace(path, pot, tables, orc) of a file of potentials/, of a key of test_train_gpu.GENERATED or of a case of
    tests/_tables.CENTRE_TABLES; the latter two are written once into a directory that lives as long as the process"""
    from lammps_mtp_kokkos_amd import capi, mtpgen
    from oracle.pyoracle import Oracle
    if name in _tables.CENTRE_TABLES:
        return _tables.centre_handles(name)
    path, keep = os.path.join(POT, name), None
    if not os.path.exists(path):
        from test_train_gpu import GENERATED
        level, Sp, seed, rmin, rmax, R, scaling = GENERATED[name]
        keep = tempfile.TemporaryDirectory()
        path = os.path.join(keep.name, name + ".mtp")
        mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(level), Sp, seed, rmin, rmax, R, scaling), path)
    pot = capi.Potential(path)
    return SimpleNamespace(path=path, pot=pot, tables=pot.tables(), orc=Oracle(path), keep=keep)


def star_cases():
    """name -> (potential, [(K, L)], seed, special, order) of every plain star set of the edge tests"""
    from test_train_gpu import GENERATED, GENERATED_KL, SMALL_KL
    cases = {}
    for special, order in LEVEL8_MODES:
        cases["level8-%s-%s" % (special, order)] = ("W_L8.mtp", _train.STAR_EDGE_KL, 71, special, order)
    for special in (None, "edge"):
        for fname in ("W_L16.mtp", "WRe_L20.mtp"):
            cases["%s-%s" % (fname, special)] = (fname, SMALL_KL, 72, special, "mixed")
        for which in sorted(GENERATED):
            cases["%s-%s" % (which, special)] = (which, GENERATED_KL, 73, special, "mixed")
        for which in sorted(_tables.CENTRE_TABLES):          # hand-made tables: Mu up to 16, rank 11, sparse slots
            cases["%s-%s" % (which, special)] = (which, _tables.CENTRE_KL, 74, special, "mixed")
    cases["ranges"] = ("W_L8.mtp", RANGE_KL, 91, None, "mixed")
    cases["bits"] = ("W_L8.mtp", BITS_KL, 93, None, "mixed")
    cases["second"] = ("W_L8.mtp", SECOND_KL, 94, None, "mixed")
    cases["understated"] = ("W_L8.mtp", UNDERSTATED_KL, 95, None, "mixed")
    return cases


def all_cases():
    return sorted(star_cases()) + ["owner-" + f for f in OWNER_FORMS]


@functools.lru_cache(maxsize=None)
def star_case(name):
    """namespace(name, pot, h, st, owner, nowned, per_star) of a case of all_cases().  The owner cases are the stars of
    RANGE_KL under a map that is (identity) arange, GIVEN; (fold) many-to-one: the atoms renumbered centres first, the owned
    atoms are the centres and the SHARED_ROWS outer atoms behind them, every other outer atom j is folded onto owned row
    stars + j % SHARED_ROWS; (self) the identity, except that in the first K = 33 star the first in-cutoff entry of the row
    (tile 0) and the 33rd (tile 1) are owned by the star's own centre"""
    if name.startswith("owner-"):
        pot, form = "W_L8.mtp", name[len("owner-"):]
        st = _train.star_set(handles(pot).tables, RANGE_KL, 92)
        owner, nowned = np.arange(st.nall, dtype=np.int32), st.nall
        if form == "fold":
            st = _stars.centres_first(st)
            n = len(st.ilist)
            nowned = n + SHARED_ROWS
            owner[nowned:] = n + np.arange(nowned, st.nall) % SHARED_ROWS
        elif form == "self":
            s = [K for K, L in st.KL].index(33)
            e = _stars.in_cutoff_entries(st, s)
            owner[st.neigh[e[[0, 32]]]] = st.ilist[s]
        else:
            assert form == "identity"
        return SimpleNamespace(name=name, pot=pot, h=handles(pot), st=st, owner=owner, nowned=nowned, per_star=form != "fold")
    pot, KL, seed, special, order = star_cases()[name]
    st = _train.star_set(handles(pot).tables, KL, seed, special, order, shuffle=order != "straddle")
    return SimpleNamespace(name=name, pot=pot, h=handles(pot), st=st, owner=None, nowned=st.nall, per_star=True)


@functools.lru_cache(maxsize=None)
def case_want(name):
    """oracle_columns of a case: one oracle call per column, made once"""
    c = star_case(name)
    st = c.st
    return oracle_columns(c.h.orc, st.x, st.types, st.ilist, st.first, st.neigh, c.owner, c.nowned)


def marked_list(st):
    """a copy of the list with the top two bits set on every third entry, the 33rd in-cutoff entry of the K = 33 star among
    them: the marked entries span both tiles of that star"""
    s = [K for K, L in st.KL].index(33)
    in33 = _stars.in_cutoff_entries(st, s)
    ne = st.neigh.copy()
    ne[int(in33[32]) % 3::3] |= SPECIAL_BITS
    pos = np.flatnonzero(ne[in33] < 0)
    assert (pos < 32).any() and pos[-1] == 32 and ((ne & 0x1FFFFFFF) == st.neigh).all() and (ne < 0).sum() >= len(ne) // 3
    return ne


def twin_rows(tables, st, owner=None, nowned=None, neigh=None):
    """driver.design_twin over a star set, in the form star_ratios takes"""
    from lammps_mtp_kokkos_amd.driver import System, design_twin
    s = System(x=st.x, types=st.types, nlocal=st.nall if nowned is None else nowned,
               owner=np.arange(st.nall) if owner is None else owner, box=np.zeros(3), ilist=st.ilist, first=st.first,
               neigh=st.neigh if neigh is None else neigh, cutoff=st.rc)
    t = design_twin(tables, s)
    n, ncol = len(st.ilist), t["basis"].shape[1]
    return dict(basis=t["basis"][:n].copy(), force=t["force"].reshape(-1, 3, ncol).copy(), virial=t["virial_atom"][:n].copy())


def replica16_cell(seed=5):
    """the noisy 2-atom cubic cell 2x2x2, every atom jittered on its own: 16 atoms"""
    pos, cell, types = _cells.replicate(*_cells.cubic2_cell(), (2, 2, 2))
    return pos + np.random.default_rng(seed).normal(0.0, 0.05, pos.shape), cell, types


def isolated_cell():
    """one atom in a 12 A cubic cell: no neighbour inside 5 A (K = 0)"""
    return np.array([[1.0, 2.0, 3.0]]), 12.0 * np.eye(3), np.ones(1, dtype=np.int32)


def compressed_cell():
    """bcc 2x2x2 at a0 = 2.27 A: 88 neighbours inside 5 A (three tiles of 32), the next shell at 5.08 A"""
    a = 2.27
    base = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]]) * a
    pos, cell, types = _cells.replicate(base, a * np.eye(3), np.ones(2, dtype=np.int32), (2, 2, 2))
    return pos + np.random.default_rng(9).normal(0.0, 0.03, pos.shape), cell, types


def rewrite_coeffs(src, dst, moment_coeffs=None, species_coeffs=None):
    """a text rewrite of the tests' own (NOT the library's writer): the species_coeffs / moment_coeffs lines of a file
    without a selection tail replaced, 17 significant digits"""
    import re
    text = open(src).read()
    assert "#MVS" not in text
    for key, v in (("species_coeffs", species_coeffs), ("moment_coeffs", moment_coeffs)):
        if v is not None:
            line = "%s = {%s}" % (key, ", ".join("%.16e" % float(x) for x in v))
            text, n = re.subn(r"^%s\s*=\s*\{[^}]*\}" % key, line, text, flags=re.M)
            assert n == 1, key
    open(dst, "w").write(text)
    return dst


def oracle_labels(orc, batch):
    """labels of md.fit_linear from the oracle: energy, folded forces [n, 3], virial [6] per configuration"""
    out = []
    for pos, cell, types in batch:
        e, f, v = _cells.oracle_cell(orc, pos, cell, types)[:3]
        out.append(dict(energy=e, f=f, virial=v))
    return out


def oracle_design(orc, batch):
    """(energy [ncfg, cols], force [3 sum n, cols], virial [ncfg, 6, cols], natoms) of a batch from the oracle's columns"""
    cols = [None if len(p) == 0 else oracle_cell_columns(orc, p, c, t)[0] for p, c, t in batch]
    ncol = orc.m.species_count + orc.m.alpha_scalar_count
    energy = np.array([np.zeros(ncol) if c is None else c["energy"] for c in cols])
    force = np.concatenate([np.zeros((0, ncol)) if c is None else c["force"] for c in cols])
    virial = np.array([np.zeros((6, ncol)) if c is None else c["virial"] for c in cols])
    return energy, force, virial, np.array([len(p) for p, _, _ in batch])
