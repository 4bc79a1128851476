"""Shared by the design-row tests (tests/test_design_cpu.py, tests/test_design_gpu.py): the judge of every entry of a
design matrix is the reference algorithm itself, by linearity.  Column Sp + a of the design matrix of a system is the
oracle's {energy, folded forces, virial} for the same potential with species_coeffs = 0 and moment_coeffs = e_a; column t
is the same with species_coeffs = e_t and moment_coeffs = 0.  The coefficients are set in place through the oracle's
Model.linear_coeffs / species_coeffs pointers and restored afterwards."""
import os

import numpy as np

import _cells
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
