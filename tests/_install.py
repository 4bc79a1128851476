"""Shared by the install tests (tests/test_install_cpu.py, tests/test_install_gpu.py): the perturbation of a potential's
three coefficient blocks, the file that carries it (the reload route an install is compared with), the committed golden
cells as neighbour lists, and the project's parity bound."""
import functools
import os
import types

import numpy as np

from lammps_mtp_kokkos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 20261018
# potential -> golden cell (16 or 54 owned atoms with their ghost images and full lists)
CELLS = {"W_L8.mtp": "W_L8_54.npz", "W_L16.mtp": "W_L16_54.npz", "WRe_L20.mtp": "WRe_L20_16.npz",
         "W_L16_nbh.almtp": "W_L16_nbh_16.npz", "WRe_L10_cfg.almtp": "WRe_L10_cfg_16.npz"}


@functools.lru_cache(maxsize=None)
def potential(path, selection=False):
    """a capi.Potential loaded once per file: potentials are const and may be shared by any number of contexts, and a
    level-20 load costs seconds"""
    return capi.Potential(path, selection=selection)


def perturb(tables, seed=SEED, rel=1e-2):
    """all three blocks times 1 + rel N(0, 1): (radial, species, moments), flat"""
    rng = np.random.default_rng(seed)
    return tuple(np.asarray(tables[k], dtype=np.float64).reshape(-1) * (1.0 + rel * rng.standard_normal(np.size(tables[k])))
                 for k in ("radial_coeffs", "species_coeffs", "moment_coeffs"))


def write_perturbed(src, dst, seed=SEED, blocks=("radial", "species", "moments")):
    """`src` with the named blocks perturbed, written by capi.write_all_coeffs (an #MVS tail is left out by the writer);
    returns (radial, species, moments) as written, the untouched blocks being the source's"""
    t = potential(src).tables()
    ra, sp, mo = perturb(t, seed)
    if "radial" not in blocks:
        ra = t["radial_coeffs"].copy()
    if "species" not in blocks:
        sp = t["species_coeffs"].copy()
    if "moments" not in blocks:
        mo = t["moment_coeffs"].copy()
    capi.write_all_coeffs(src, dst, mo, sp, ra)
    return ra, sp, mo


def golden_cell(potential_name):
    g = np.load(os.path.join(GOLDEN, CELLS[potential_name]))
    return types.SimpleNamespace(x=g["x"], types=g["types"].astype(np.int32), ilist=g["ilist"].astype(np.int32),
                                 first=g["first"].astype(np.int32), neigh=g["neigh"].astype(np.int32), nall=len(g["x"]),
                                 nlocal=int(g["nlocal"]))


def bound(ref):
    """the project's parity bound per quantity: 1e-9 + 1e-10 max(1, max |reference|)"""
    ref = np.asarray(ref, dtype=np.float64)
    return 1e-9 + 1e-10 * max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)


def text_only(src, dst):
    """`src` without its #MVS selection tail"""
    data = open(src, "rb").read()
    open(dst, "wb").write(data[: data.index(b"#MVS_v1.1")] if b"#MVS_v1.1" in data else data)
    return dst
