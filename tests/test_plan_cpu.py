"""The launch planner as a host-only unit (csrc/mtp_plan.hpp, csrc/mtp_plan.cpp): tests/plan_dump.cpp, built with the
plain C++ compiler from mtp_plan.cpp and mtp_potential.cpp alone, prints every plan, both argument blocks and the row
ranges for the lines of tests/golden/plan_inputs.txt, and the output equals tests/golden/plan_parent.txt line by line.
That file was written by the planner of commit 78152b6 (the one function of 236 lines in mtp_context.hip and the row-range
block of mtp_compute_device_rows), never by the code under test.

`python tests/test_plan_cpu.py list` prints the committed input list, `... sweep` the full product of its axes (1.3 million
lines; both planners were run over it once), `... potentials DIR` writes the generated potentials."""
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lammps_mtp_kokkos_amd import mtpgen  # noqa: E402

import _tables  # noqa: E402

POT = os.path.join(ROOT, "potentials")
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "tests", "cpp", "plan_dump")

COMMITTED = ["W_L8.mtp", "W_L16.mtp", "W_L16_nbh.almtp", "WRe_L10_cfg.almtp", "WRe_L20.mtp"]
# name: (level, species, R); "mu9": nine radial functions (no level table has more than five)
GENERATED = {"gen_L6_s1.mtp": (6, 1, 8), "gen_L12_s2.mtp": (12, 2, 8), "gen_L18_s3.mtp": (18, 3, 8),
             "gen_L20_s1.mtp": (20, 1, 8), "gen_L16_s3_R9.mtp": (16, 3, 9), "gen_mu9_s2.mtp": ("mu9", 2, 8)}
CUS = [8, 256, 304]
INUM = [0, 1, 63, 2048, 4095, 4096, 65536]
MAX_NUMNEIGH = [0, 31, 32, 33, 64, 65, 94, 257, 100000]     # the last: nothing fits one CU's LDS
VARIANTS = [0, 1, 2]
SINGLES = [[]] + [["%s=%s" % (k, v)] for k, vs in [
    ("MTP_MAX_WAVES", [1, 4, 8, 12, 16]), ("MTP_LAYOUT", ["keep", "nodg", "lean", "rebuild", "rebuild-nodg", "other"]),
    ("MTP_WPS", [2, 3]), ("MTP_GRADE_WPS3", [0, 1]), ("MTP_WPB", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]),
    ("MTP_BLOB_PREFIX", ["core", "tgt", "norows", "rows", "other"]), ("MTP_ROWS_LDS", [0, 1]),
    ("MTP_SCALARS_LDS", [0, 1])] for v in vs]
PAIRS = [["MTP_LAYOUT=%s" % y, "MTP_WPS=%d" % w] for y in ("keep", "nodg", "lean", "rebuild", "rebuild-nodg", "other")
         for w in (2, 3)] + [["MTP_WPS=%d" % w, "MTP_MAX_WAVES=%d" % m] for w in (2, 3) for m in (1, 4, 8, 12, 16)]


def write_generated(d):
    for name, (level, species, R) in GENERATED.items():
        path = os.path.join(str(d), name)
        if level == "mu9":
            tab, nfac = _tables.make_table([(mu, 0) for mu in range(9)] + [(0, 2), (8, 3)])
            _tables.write(tab, nfac, path, species=species, R=R)
        else:
            mtpgen.write_mtp(mtpgen.random_potential(mtpgen.build_table(level), species, 4242, 2.0, 5.0, R), path)


def _rows(cus, inum):
    return sorted({1, cus, inum // 8, inum})


def _line(pot, cus, inum, mnn, variant, rows, env=()):
    return " ".join([pot, str(cus), str(inum), str(mnn), str(variant), str(rows)] + list(env))


def committed_list():
    """each potential at the headline size; each axis alone around it for two potentials; every override alone and
    the pairs the suites use"""
    base = (256, 65536, 94, 0)
    out = [_line(p, *base, 65536) for p in COMMITTED + list(GENERATED)]
    for p in ("W_L16.mtp", "WRe_L20.mtp"):
        out += [_line(p, c, 65536, 94, 0, c) for c in CUS if c != 256]
        out += [_line(p, 256, n, 94, 0, n // 8) for n in INUM if n != 65536]
        out += [_line(p, 256, 4096, m, 0, 4096) for m in MAX_NUMNEIGH]
        out += [_line(p, 256, 65536, 94, v, 65536) for v in VARIANTS[1:]]
        out += [_line(p, 256, 65536, 94, 0, r) for r in _rows(256, 65536)[:-1]]
    out += [_line("W_L16.mtp", *base, 256, e) for e in SINGLES[1:] + PAIRS]
    out += [_line("WRe_L20.mtp", 256, 4096, 65, 0, 512, e) for e in SINGLES[1:]]
    out += [_line("W_L8.mtp", 256, 2048, 64, 0, 2048, e) for e in PAIRS]
    return out


def sweep_list():
    for p, c, n, m, v in itertools.product(COMMITTED + list(GENERATED), CUS, INUM, MAX_NUMNEIGH, VARIANTS):
        for r in _rows(c, n):
            for e in SINGLES + PAIRS:
                yield _line(p, c, n, m, v, r, e)


def dump(list_path, gen_dir):
    """plan_dump's output lines; the LDS-bank search of the loader is off (it renumbers moments: never a plan input)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "csrc"), "plan_dump"])
    env = dict(os.environ, MTP_BANK_ROUNDS="0", MTP_BANK_SCALE="1")
    r = subprocess.run([EXE, list_path, POT, str(gen_dir)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_committed_list_is_what_the_axes_give():
    assert open(os.path.join(GOLDEN, "plan_inputs.txt")).read().splitlines() == committed_list()


def test_every_plan_equals_the_parents(tmp_path):
    write_generated(tmp_path)
    got = dump(os.path.join(GOLDEN, "plan_inputs.txt"), tmp_path)
    want = open(os.path.join(GOLDEN, "plan_parent.txt")).read().splitlines()
    inputs = ["(header)"] + committed_list()
    assert len(got) == len(want) == len(inputs)
    bad = [(inputs[k], got[k], want[k]) for k in range(len(want)) if got[k] != want[k]]
    assert not bad, "%d of %d lines differ, the first: %s\n got %s\nwant %s" % ((len(bad), len(want)) + bad[0])
    # the axes are live: the refusal, all four layouts and both register builds are in the list
    rows = [l.split(" | ") for l in want[1:]]
    assert {r[0] for r in rows} == {"0 0", "-24 -24"}
    assert {r[1].split()[0] for r in rows if r[0] == "0 0"} == {"0", "1", "2", "3"}
    assert {r[1].split()[17] for r in rows} == {"2", "3"}


if __name__ == "__main__":
    if sys.argv[1] == "potentials":
        write_generated(sys.argv[2])
    else:
        for text in (committed_list() if sys.argv[1] == "list" else sweep_list()):
            print(text)
