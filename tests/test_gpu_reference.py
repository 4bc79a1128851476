"""The HIP path against outputs of the COMPILED REFERENCE.

tests/golden/ref/*.npz hold inputs and what the reference's own pair styles gave on them (written by
tests/golden/make_reference_golden.py from oracle/_ref/libmtp_ref.so; tests/test_reference_cpu.py asserts that the
compiled reference reproduces them bit for bit).  Every other GPU test is judged by the oracle; here nothing stands
between the kernels and the reference: star and distance edges on the level-16 and the two-species level-20 table, five
species (every i-j radial block distinct), scaling != 1, both grade modes.  Nothing outside the repository is read.

Tolerances: per star, |dF| <= 1e-9 + 1e-10 max(1, max|F_star|) and the eatom / vatom / grades constants of
tests/_stars.py (the rule of tests/test_gpu_geometry.py); totals with _close of tests/test_gpu_parity.py.

The last test needs the compiled reference itself and runs only where oracle/_ref/libmtp_ref.so loads.
"""
import os
import subprocess

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system

import _stars
from golden.make_reference_golden import potential_path
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
FIXTURES = os.path.join(ROOT, "tests", "golden", "ref")
NAMES = sorted(f[:-4] for f in os.listdir(FIXTURES) if f.endswith(".npz"))
# shells below min_dist: forces of 1e14 .. 1e24 eV/A, outside the fixed-point range of the deterministic mode
IN_RANGE = [n for n in NAMES if "below_min_dist" not in n]
GRADES = [n for n in NAMES if n.startswith("grades_")]

_LOADED = {}


def _fixture(name, tmp_pot_dir):
    """(arrays, capi.Potential), loaded once per session"""
    if name not in _LOADED:
        g = np.load(os.path.join(FIXTURES, name + ".npz"))
        _LOADED[name] = (g, capi.Potential(potential_path(g, tmp_pot_dir), selection=bool(g["selection"])))
    return _LOADED[name]


def _star_max(sid, a, nstars):
    a = np.abs(np.asarray(a, dtype=np.float64)).reshape(len(a), -1).max(1)
    out = np.zeros(nstars)
    np.maximum.at(out, sid, a)
    return out


def _judge(g, got, grade, label):
    """per star, then the totals; prints the worst error / tolerance per quantity"""
    sid, n = g["sid"].astype(np.int64), len(g["ilist"])
    cfg = grade and "grades" in g.files and not g["grades"].any()
    keys = ("f", "eatom", "vatom") + (("grades",) if grade and not cfg else ())
    worst = {}
    for k in keys:
        atol, rtol = _stars.PER_STAR_TOL[k]
        err = _star_max(sid, np.asarray(got[k]) - g[k], n)
        tol = atol + rtol * np.maximum(1.0, _star_max(sid, g[k], n))
        r = err / tol
        worst[k] = float(r.max())
        assert np.isfinite(r).all() and r.max() <= 1.0, "%s %s: star %d misses its tolerance %.2f-fold" % (
            label, k, int(np.argmax(r)), r.max())
    e = float(g["energy"])
    assert abs(got["energy"] - e) / n <= 1e-10 * max(1.0, abs(e) / n), label + " energy"
    _close(got["virial"], g["virial"], label + " virial", atol=1e-8)
    if grade:
        if cfg:
            _close(got["coeff_ders"], g["coeff_ders"], label + " coeff_ders", atol=1e-9, rtol=1e-10)
        mg = float(g["max_grade"])
        assert abs(got["max_grade"] - mg) <= 1e-9 * max(1.0, mg), label + " max_grade"
    print("%s: %d stars, %d atoms, worst error / per-star tolerance %s" % (
        label, n, len(sid), " ".join("%s %.2e" % kv for kv in worst.items())))


def _context(pot, g, deterministic=False):
    ctx = capi.Context(pot, 0)
    if deterministic:
        ctx.set_deterministic(True)
    ctx.set_neighbors(g["ilist"], g["first"], g["neigh"], len(g["x"]))
    return ctx


@pytest.mark.parametrize("name", NAMES)
def test_default_call(name, tmp_pot_dir):
    g, pot = _fixture(name, tmp_pot_dir)
    got = _context(pot, g).compute(g["x"], g["types"], eflag=3, vflag=4)
    _judge(g, got, False, name + " default")


@pytest.mark.parametrize("name", IN_RANGE)
def test_deterministic_mode(name, tmp_pot_dir):
    """fixed-point force accumulation (|f| < 2^23 eV/A): within the same tolerances, and bitwise equal across calls"""
    g, pot = _fixture(name, tmp_pot_dir)
    assert np.abs(g["f"]).max() < 2.0 ** 22
    ctx = _context(pot, g, deterministic=True)
    got = ctx.compute(g["x"], g["types"], eflag=3, vflag=4)
    _judge(g, got, False, name + " deterministic")
    again = ctx.compute(g["x"], g["types"], eflag=3, vflag=4)
    for k in ("f", "eatom", "vatom", "virial"):
        assert np.array_equal(got[k], again[k]), k


@pytest.mark.parametrize("name", GRADES)
def test_grade_call(name, tmp_pot_dir):
    """neighbourhood mode on the level-16 table (R = 8, Mu <= 4, one species: the fused grade kernel) and
    configuration-mode grades: per-atom grades, max_grade with the natoms normalisation, the candidate vector"""
    g, pot = _fixture(name, tmp_pot_dir)
    cfg = name.startswith("grades_cfg")
    assert bool(pot.info.configuration_mode) == cfg and int(g["natoms"]) == len(g["ilist"])
    got = _context(pot, g).compute(g["x"], g["types"], eflag=3, vflag=4, grade=True)
    if cfg:
        # the library hands back max |A^-1 c| of the call; the style divides by the global atom count
        got["max_grade"] = pot.cfg_grade(got["coeff_ders"]) / int(g["natoms"])
    _judge(g, got, True, name + " grade")


# ---- the host mirror's styles beside the reference class itself -------------------------------------------------------

EXE = os.path.join(ROOT, "tests", "cpp", "test_pair_host")


def _write_system(path, s):
    with open(path, "w") as fh:
        fh.write("%d %d %.17g %.17g %.17g\n" % (s.nlocal, s.nall, *s.box))
        for (x, y, z), t in zip(s.x, s.types):
            fh.write("%.17g %.17g %.17g %d\n" % (x, y, z, t))
        for i in range(s.nlocal):
            row = s.neigh[s.first[i]:s.first[i + 1]]
            fh.write("%d %s\n" % (len(row), " ".join(map(str, row))))


def test_host_mirror_styles_beside_the_reference_class(tmp_path):
    """`mtp` and `mtp/extrapolation` of the host mirror (the driver of tests/test_pair_host.py) and the reference's own
    classes on the same 128 atoms: energy, forces, virial, pvector[0], per-atom grades, and the written .cfg line by line
    -- every field textually equal except the %.5f grade column, compared as numbers within one unit of its last digit"""
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref/libmtp_ref.so is not on this machine")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "host")])
    pos, box = mtpgen.bcc_lattice(4, 4, 4)
    s = periodic_system(pos, box, None, 7.0)
    assert s.nlocal == 128
    sysf, outf, cfgf = str(tmp_path / "sys.txt"), str(tmp_path / "out.txt"), str(tmp_path / "sel.cfg")
    _write_system(sysf, s)
    # pair_style mtp
    potf = os.path.join(POT, "W_L16.mtp")
    r = subprocess.run([EXE, "run", "mtp", sysf, outf, potf], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = open(outf).read().split("\n")
    e, cut = map(float, lines[0].split())
    vir = np.array(lines[1].split(), float)
    arr = np.array([l.split() for l in lines[2:2 + s.nall]], float)
    ref = pyref.Reference(potf)
    want = ref.compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)
    assert cut == ref.init_one(1, 1)
    assert abs(e - want["energy"]) / s.nlocal <= 1e-10 * max(1.0, abs(want["energy"]) / s.nlocal)
    _close(arr[:, :3], want["f"], "forces")
    _close(arr[:, 3], want["eatom"], "eatom", atol=1e-10)
    _close(vir, want["virial"], "virial", atol=1e-8)
    # pair_style mtp/extrapolation <file> <cfg> <select> <break>
    potf = os.path.join(POT, "W_L16_nbh.almtp")
    probe = pyref.Reference(potf, selection=True).compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True)
    mg = probe["max_grade"]
    sel, brk = "%.6f" % (0.5 * mg), "%.6f" % (2 * mg)
    r = subprocess.run([EXE, "runext", "mtp/extrapolation", sysf, outf, potf, cfgf, sel, brk], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    dom = [s.box[0], s.box[1], s.box[2], 0.0, 0.0, 0.0]
    want = pyref.run_mlip3(potf, str(tmp_path / "ref.cfg"), sel, brk, dom, s.x, s.types, s.ilist, s.first, s.neigh,
                           eflag=3, vflag=0, natoms=s.nlocal)
    lines = open(outf).read().split("\n")
    e, e_plain, pv, stopped = lines[0].split()
    w = want["out"]
    assert stopped == "0" and want["error"] == ""
    for v in (float(e), float(e_plain)):
        assert abs(v - w["energy"]) / s.nlocal <= 1e-10 * max(1.0, abs(w["energy"]) / s.nlocal)
    assert abs(float(pv) - w["pvector0"]) <= 1e-9 * max(1.0, w["pvector0"])
    _close(np.array(lines[1:1 + s.nlocal], float), w["grades"][:s.nlocal], "grades", atol=1e-9, rtol=1e-9)
    # the mirror grades on both of its compute calls (MLIP-3 form): two equal records; the reference ran one
    got = open(cfgf).read().split("END_CFG\n\n")
    ref_rec = want["cfg"].decode().split("END_CFG\n\n")
    assert len(got) == 3 and got[2] == "" and len(ref_rec) == 2 and ref_rec[1] == ""
    b = ref_rec[0].split("\n")
    for rec in got[:2]:
        a = rec.split("\n")
        assert len(a) == len(b) == 8 + s.nlocal + 2
        for la, lb in zip(a, b):
            fa, fb = la.split("\t"), lb.split("\t")
            if len(fb) == 6:                               # an atom line: id type x y z grade
                assert fa[:5] == fb[:5], (la, lb)
                assert len(fa[5].split(".")[1]) == 5 and abs(float(fa[5]) - float(fb[5])) <= 1.0000001e-5, (la, lb)
            else:
                assert la == lb
    # break threshold below the max grade: the reference's message
    r = subprocess.run([EXE, "runext", "mtp/extrapolation", sysf, outf, potf, cfgf, sel, "%.6f" % (0.9 * mg)],
                       capture_output=True, text=True)
    want = pyref.run_mlip3(potf, str(tmp_path / "ref2.cfg"), sel, "%.6f" % (0.9 * mg), dom, s.x, s.types, s.ilist,
                           s.first, s.neigh, eflag=3, vflag=0, natoms=s.nlocal)
    assert want["error"].startswith("ERROR on proc 0: Exceeded Break Threshold: ")
    assert want["error"][len("ERROR on proc 0: "):] in r.stdout + r.stderr
