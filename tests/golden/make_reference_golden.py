"""Writes tests/golden/ref/*.npz: inputs and the outputs of the COMPILED REFERENCE (oracle/_ref/libmtp_ref.so, the
reference's own pair styles built by `make -C oracle ref`; oracle/pyref.py) on the edges that the geometry and shape
suites exercise.  Unlike tests/golden/*.npz these are not the oracle's numbers: tests/test_gpu_reference.py judges the
HIP path by them on a machine that has neither the reference nor the oracle's agreement with it to lean on, and
tests/test_reference_cpu.py asserts that the compiled reference, where it exists, reproduces every file exactly.

    python tests/golden/make_reference_golden.py

Every file: x, types, ilist, first, neigh, sid (the star of every atom: per-star tolerances), natoms, selection,
`potential` (a committed file under potentials/) or `potential_text` (the bytes of a generated one), and the reference's
f, eatom, energy, virial, vatom (grades, max_grade, coeff_ders for the grade files).  Stars are tests/_stars.py's, few
and small (a file stays under 22 KB): empty rows, rows wholly outside the cutoff, one neighbour, a row of 33 inside (more
than one 32-neighbour tile); kinds: plain, an entry at r^2 == r_c^2 bit-exact with one a representable step beyond,
shells down to 0.5 min_dist, the whole set shifted by +1e5 and by (-731.25, -1e5, -3.5) A.
"""
import os
import sys
import zlib
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _stars  # noqa: E402
from lammps_mtp_kokkos_amd import mtpgen  # noqa: E402

OUT = os.path.join(HERE, "ref")
KL = [(0, 0), (0, 3), (1, 1), (2, 5), (5, 5), (33, 36)]
KINDS = dict(plain={}, exact_cutoff=dict(special="edge"), below_min_dist=dict(rin=(1.0, 5.0)),
             offset_1e5=dict(offset=(1e5, 1e5, 1e5)), offset_negative=dict(offset=(-731.25, -1e5, -3.5)))
FORCE_KEYS = ("f", "eatom", "energy", "virial", "vatom")
GRADE_KEYS = ("grades", "max_grade", "coeff_ders")


def star_sets(kinds, species, seed, leading=False):
    """one system: the stars of every kind side by side (disjoint, so the kinds do not see each other); leading: centres
    renumbered to 0 .. n-1, owned atoms first as LAMMPS has them (the reference indexes its grades by atom)"""
    rng = np.random.default_rng(seed)
    xs, ty, il, fi, ne, sid = [], [], [], [0], [], []
    n = ns = 0
    for kind in kinds:
        st = _stars.stars(KL, rng, species=species, order="mixed", **KINDS[kind])
        assert _stars.counts(st) == KL
        xs.append(st.x)
        ty.append(st.types)
        il.append(st.ilist + n)
        ne.append(st.neigh + n)
        fi += list(st.first[1:] + fi[-1])
        sid.append(st.sid + ns)
        n += st.nall
        ns += len(KL)
    s = SimpleNamespace(x=np.concatenate(xs), types=np.concatenate(ty).astype(np.int32),
                        ilist=np.concatenate(il).astype(np.int32), first=np.array(fi, np.int32),
                        neigh=np.concatenate(ne).astype(np.int32), sid=np.concatenate(sid).astype(np.int16), nall=n)
    if leading:
        rest = np.setdiff1d(np.arange(n), s.ilist)
        order = np.concatenate([s.ilist, rest])
        new_of = np.empty(n, np.int64)
        new_of[order] = np.arange(n)
        s = SimpleNamespace(x=np.ascontiguousarray(s.x[order]), types=s.types[order],
                            ilist=np.arange(len(s.ilist), dtype=np.int32), first=s.first,
                            neigh=new_of[s.neigh].astype(np.int32), sid=s.sid[order], nall=n)
    return s


def five_species_text(tmp):
    p = mtpgen.random_potential(mtpgen.build_table(6), 5, 4242)
    assert len({p.radial_coeffs[k].tobytes() for k in range(25)}) == 25       # every i-j block distinct
    return open(mtpgen.write_mtp(p, tmp), "rb").read()


def scaled_text(tmp):
    p = mtpgen.random_potential(mtpgen.build_table(10), 2, 99, 2.0, 5.0, 8, 2.5)
    return open(mtpgen.write_mtp(p, tmp), "rb").read()


# Shells below min_dist give forces far outside the range of the library's deterministic (fixed-point) mode,
# |f| < 2^23 eV/A, at levels 16 and 20; they get files of their own, which tests/test_gpu_reference.py runs through the
# default call only.  Every other file stays inside 2^22 (asserted below).
EDGES = ["plain", "exact_cutoff", "offset_1e5", "offset_negative"]
# name -> (committed potential or text writer, species, selection, kinds, seed)
CASES = {
    "stars_W_L16": ("W_L16.mtp", 1, False, EDGES, 101),
    "stars_W_L16_below_min_dist": ("W_L16.mtp", 1, False, ["below_min_dist"], 111),
    "stars_WRe_L20": ("WRe_L20.mtp", 2, False, EDGES, 102),
    "stars_WRe_L20_below_min_dist": ("WRe_L20.mtp", 2, False, ["below_min_dist"], 112),
    "stars_five_species_L6": (five_species_text, 5, False, ["plain", "exact_cutoff", "offset_1e5"], 103),
    "stars_scaling_2p5_L10": (scaled_text, 2, False, ["plain", "exact_cutoff", "offset_negative"], 104),
    "stars_scaling_2p5_L10_below_min_dist": (scaled_text, 2, False, ["below_min_dist"], 114),
    "grades_nbh_W_L16": ("W_L16_nbh.almtp", 1, True, ["plain", "exact_cutoff"], 105),
    "grades_nbh_W_L16_below_min_dist": ("W_L16_nbh.almtp", 1, True, ["below_min_dist"], 115),
    "grades_cfg_WRe_L10": ("WRe_L10_cfg.almtp", 2, True, ["plain", "exact_cutoff"], 106),
    "grades_cfg_WRe_L10_below_min_dist": ("WRe_L10_cfg.almtp", 2, True, ["below_min_dist"], 116),
}


def potential_path(g, tmp_dir):
    """the potential file of a loaded fixture (a generated one is written into tmp_dir)"""
    if "potential" in g.files:
        return os.path.join(ROOT, "potentials", str(g["potential"]))
    path = os.path.join(str(tmp_dir), "fixture_%08x.mtp" % zlib.crc32(g["potential_text"].tobytes()))
    with open(path, "wb") as fh:
        fh.write(g["potential_text"].tobytes())
    return path


if __name__ == "__main__":
    import tempfile
    from oracle import pyref
    pyref.build()
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (pot, species, sel, kinds, seed) in CASES.items():
            s = star_sets(kinds, species, seed, leading=sel)
            extra = {}
            if callable(pot):
                text = pot(os.path.join(tmp, name + ".mtp"))
                extra["potential_text"] = np.frombuffer(text, np.uint8)
                path = os.path.join(tmp, name + ".mtp")
            else:
                extra["potential"] = pot
                path = os.path.join(ROOT, "potentials", pot)
            assert len(set(s.types[s.ilist])) == species and len(set(s.types)) == species
            r = pyref.Reference(path, selection=sel).compute(s.x, s.types, s.ilist, s.first, s.neigh, 3, 4,
                                                             extrapolation=sel, natoms=len(s.ilist))
            assert np.isfinite(r["f"]).all()
            assert (np.abs(r["f"]).max() < 2.0 ** 22) == ("below_min_dist" not in name), np.abs(r["f"]).max()
            keys = FORCE_KEYS + (GRADE_KEYS if sel else ())
            out = os.path.join(OUT, name + ".npz")
            np.savez_compressed(out, x=s.x, types=s.types, ilist=s.ilist, first=s.first, neigh=s.neigh, sid=s.sid,
                                natoms=len(s.ilist), selection=sel, **extra, **{k: r[k] for k in keys})
            print("%-24s %4d atoms %3d stars  max|f| %.3e  %6d bytes" % (name, s.nall, len(s.ilist), np.abs(r["f"]).max(),
                                                                         os.path.getsize(out)))
