"""The LDS-bank search of the schedule builder (csrc/mtp_bank_search.hpp: search, which mtp_potential::finalize runs
through search_banks), host only.

tests/cpp/bank_search_dump.cpp is built from mtp_potential.cpp + mtp_plan.cpp alone (as `make plan_dump` builds its
program) and prints the rows, the numbering and a hash of both after a load; MTP_DEBUG_BANKS=1 makes the library print
its model on stderr.  Two searches: v1 (MTP_BANK_SEARCH=v1: greedy, two move kinds; the table of the commit before the
annealed search, whose hashes are in tests/golden/bank_search_v1.json) and v2 (the default for row-per-lane potentials:
annealed, with factor exchange and compound row moves).  Both run the same rounds on one incremental state of the model
(State); they differ in the moves the row round proposes and in the acceptance rule.

Checked for every committed potential at effort 2 x 1 (what the suites run), and for W_L16.mtp at the shipped default:
  same rows      the rows after the search are the file's rows as a multiset of {unordered (a0, a1), mult, a3} in file
                 numbering, each inside its own level or the leaf block (the blocks of the v1 table, which never exchanges
                 or moves a row out of its level), level_offset as in v1, moment_perm a permutation that keeps the
                 classes basics / stored products / leaves;
  determinism    two loads print the same bytes;
  v1             reproduces the recorded hash;
  tables         every load gives the hash and the model (before, after, reads, adds) that the last commit with the search
                 inside mtp_potential.cpp gave (tests/golden/bank_search_tables.json): both searches at 2 x 1, W_L16.mtp
                 at v1 8 x 4, v1 4 x 16, v2 4 x 16 and v2 0 x 1, W_L8.mtp and WRe_L20.mtp with nothing set;
  improvement    the model of v2 is below that of v1 at the same effort, and the printed floor of forced same-address
                 adds is at or below the count reached.  W_L8.mtp has 14 stored moments for add groups of 16 lanes: two
                 same-address adds per group and stream are forced, v1 already sits on that floor (64 = 64), and there
                 v2 has to reach the floor as well -- nothing is below it.
A hand-made level of 32 rows whose hot factor is a0 in every row must end with that factor in both streams, the
program built with -fsanitize=address,undefined must run W_L16.mtp at 2 x 1 clean, and tests/cpp/bank_state_check.cpp
(built the same way, from the header alone) holds the incremental state against the from-scratch count of the model
over 20 000 random mutations of a hand-made table."""
import collections
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import mtpgen

import _mutate
import _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
CSRC = os.path.join(ROOT, "lammps_mtp_kokkos_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bank_search_v1.json")
TABLES = os.path.join(ROOT, "tests", "golden", "bank_search_tables.json")
DEFAULTS = ("W_L8.mtp", "WRe_L20.mtp")   # also loaded with nothing set
POTENTIALS = ["W_L8.mtp", "W_L16.mtp", "WRe_L20.mtp", "WRe_L10_cfg.almtp", "W_L16_nbh.almtp"]
SUITE = (2, 1)            # the effort of the suites (tests/conftest.py)
SHIPPED_V1 = (8, 4)       # what v1 shipped for row-per-lane potentials
SHIPPED_V2 = (4, 16)      # BANK_ROUNDS_V2 x BANK_SCALE_V2


def _compiler():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    return cxx


DUMP_SRC = [os.path.join(ROOT, "tests", "cpp", "bank_search_dump.cpp"), os.path.join(CSRC, "mtp_plan.cpp"),
            os.path.join(CSRC, "mtp_potential.cpp")]
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _build(out, extra=(), src=DUMP_SRC):
    cmd = [_compiler(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", *extra, "-o", out, *src]
    subprocess.run(cmd, check=True)
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("bank_search") / "bank_search_dump"))


def _env(search, effort):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MTP_")}
    env["MTP_DEBUG_BANKS"] = "1"
    if search == "v1":
        env["MTP_BANK_SEARCH"] = "v1"
    if effort is not None:
        env["MTP_BANK_ROUNDS"], env["MTP_BANK_SCALE"] = str(effort[0]), str(effort[1])
    return env


def _start(program, path, search, effort):
    return subprocess.Popen([program, path], env=_env(search, effort), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True)


def _finish(proc):
    out, err = proc.communicate()
    assert proc.returncode == 0, err
    lines = dict(l.split(" ", 1) for l in out.splitlines())
    r = {"stdout": re.sub(r"^counts .*\n", "", out), "stderr": err}   # (the counts line carries the wall time)
    A, B, stored, levels, _ = lines["counts"].split()
    r["A"], r["B"], r["stored"], r["levels"] = int(A), int(B), int(stored), int(levels)
    r["hash"] = lines["hash"].strip()
    r["level_offset"] = [int(v) for v in lines["level_offset"].split()]
    r["perm"] = np.array(lines["perm"].split(), dtype=np.int64)
    r["rows"] = np.array(lines["rows"].split(), dtype=np.int64).reshape(-1, 4)
    m = re.search(r"product passes: (\d+) -> (\d+) extra cycles per atom \(reads (\d+), adds (\d+)\).*search (v\d)", err)
    r["before"], r["model"], r["reads"], r["adds"], r["search"] = int(m[1]), int(m[2]), int(m[3]), int(m[4]), m[5]
    m = re.search(r"after: .*D\[a0\] (\d+) / \d+, D\[a1\] (\d+) / \d+, M\[a3\] (\d+) / \d+", err)
    r["same_d"], r["same_m"] = int(m[1]) + int(m[2]), int(m[3])
    m = re.search(r"forced same-address adds in all: D\[a0\] \+ D\[a1\] (\d+), M\[a3\] (\d+)", err)
    r["forced_d"], r["forced_m"] = int(m[1]), int(m[2])
    assert "before: reads" in err
    return r


def _load(program, path, search, effort):
    return _finish(_start(program, path, search, effort))


def _file_rows(path):
    """the times rows of the file, file numbering"""
    text = open(path, errors="replace").read()
    body = _mutate._block(text, "alpha_index_times").group(2)
    return [tuple(int(v) for v in r) for r in re.findall(r"\{\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*\}", body)]


def _key(a0, a1, mult, a3):
    return (min(a0, a1), max(a0, a1), mult, a3)


def _in_file_numbering(r):
    inv = np.empty(r["A"], dtype=np.int64)
    inv[r["perm"]] = np.arange(r["A"])
    rows = r["rows"].copy()
    for c in (0, 1, 3):
        rows[:, c] = inv[rows[:, c]]
    return rows


def _check_same_rows(path, new, old):
    A, B, stored = new["A"], new["B"], new["stored"]
    # the numbering: a permutation inside each class
    assert sorted(new["perm"].tolist()) == list(range(A))
    assert sorted(new["perm"][:B].tolist()) == list(range(B))
    assert (new["stored"], new["levels"]) == (old["stored"], old["levels"])
    old_leaf, new_leaf = old["perm"] >= stored, new["perm"] >= stored
    assert np.array_equal(old_leaf, new_leaf)
    # the rows: those of the file (padding rows have multiplicity 0 and are not the file's) ...
    assert new["level_offset"] == old["level_offset"] and new["level_offset"][-1] == len(new["rows"])
    rows, rows_old = _in_file_numbering(new), _in_file_numbering(old)
    want = collections.Counter(_key(*r) for r in _file_rows(path) if r[2] != 0)
    got = collections.Counter(_key(*r) for r in rows.tolist() if r[2] != 0)
    zero_mult_file = sum(1 for r in _file_rows(path) if r[2] == 0)
    assert got == want
    assert len(rows) - sum(got.values()) >= zero_mult_file
    # ... each in the block v1 has it in
    off = new["level_offset"]
    for b, e in zip(off[:-1], off[1:]):
        assert collections.Counter(_key(*r) for r in rows[b:e].tolist()) == \
            collections.Counter(_key(*r) for r in rows_old[b:e].tolist()), (b, e)
        if b >= off[new["levels"]]:   # the leaf block: every target a leaf
            assert all(new_leaf[r[3]] for r in rows[b:e].tolist() if r[2] != 0)


def _check_improvement(new, old):
    print("model v1 %d (reads %d, adds %d), v2 %d (reads %d, adds %d); same-address adds v2: D %d, M %d; forced: D %d, M %d"
          % (old["model"], old["reads"], old["adds"], new["model"], new["reads"], new["adds"], new["same_d"], new["same_m"],
             new["forced_d"], new["forced_m"]))
    assert (new["before"], new["forced_d"], new["forced_m"]) == (old["before"], old["forced_d"], old["forced_m"])
    assert new["forced_d"] <= new["same_d"] and new["forced_m"] <= new["same_m"]
    floor = new["forced_d"] + new["forced_m"]
    if old["model"] == floor:   # v1 on the floor already (W_L8.mtp): nothing is below it
        assert new["model"] == floor
    else:
        assert new["model"] < old["model"]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def tables():
    return json.load(open(TABLES))


def _check_table(r, want):
    assert {"hash": r["hash"], "before": r["before"], "after": r["model"], "reads": r["reads"], "adds": r["adds"]} == want


@pytest.mark.parametrize("name", POTENTIALS)
def test_suite_effort_same_rows_determinism_v1_and_improvement(program, golden, tables, name):
    path = os.path.join(POT, name)
    procs = [_start(program, path, s, SUITE) for s in ("v1", "v2", "v2")]
    if name in DEFAULTS:
        procs.append(_start(program, path, None, None))
    old, new, again = [_finish(p) for p in procs[:3]]
    assert old["search"] == "v1" and old["hash"] == golden["%s@%dx%d" % ((name,) + SUITE)]
    _check_table(old, tables["%s@v1@%dx%d" % ((name,) + SUITE)])
    _check_table(new, tables["%s@v2@%dx%d" % ((name,) + SUITE)])
    if name in DEFAULTS:
        _check_table(_finish(procs[3]), tables["%s@default" % name])
    assert new["stdout"] == again["stdout"] and new["stderr"] == again["stderr"]
    _check_same_rows(path, new, old)
    row_per_lane = int(re.search(r"(\d+) head x tail blocks", new["stderr"])[1]) <= 32
    if not row_per_lane:   # the gather-form potentials keep v1
        assert new["search"] == "v1" and new["hash"] == old["hash"]
        return
    assert new["search"] == "v2"
    _check_improvement(new, old)


def test_shipped_effort_level16(program, golden, tables):
    path = os.path.join(POT, "W_L16.mtp")
    procs = [_start(program, path, "v1", None), _start(program, path, "v1", SHIPPED_V2), _start(program, path, "v2", None),
             _start(program, path, "v2", None)]
    parent, old, new, again = [_finish(p) for p in procs]
    assert "%d rounds x %d, search v1" % SHIPPED_V1 in parent["stderr"] and "%d rounds x %d, search v2" % SHIPPED_V2 in new["stderr"]
    assert parent["hash"] == golden["W_L16.mtp@%dx%d" % SHIPPED_V1]
    _check_table(parent, tables["W_L16.mtp@v1@%dx%d" % SHIPPED_V1])
    _check_table(old, tables["W_L16.mtp@v1@%dx%d" % SHIPPED_V2])
    _check_table(new, tables["W_L16.mtp@v2@%dx%d" % SHIPPED_V2])
    assert new["stdout"] == again["stdout"] and new["stderr"] == again["stderr"]
    _check_same_rows(path, new, old)
    _check_improvement(new, old)      # v1 at v2's effort
    _check_improvement(new, parent)   # v1 at the effort it shipped with


def test_mutated_table_keeps_its_rows(program, tmp_path):
    """tests/_mutate.py: a late writer that keeps scalars from being leaves, two scalars on one moment"""
    path = str(tmp_path / "mutated.mtp")
    info = _mutate.mutate_mtp(os.path.join(POT, "W_L16.mtp"), path)
    assert "moved_row" in info
    old, new = _load(program, path, "v1", SUITE), _load(program, path, "v2", SUITE)
    _check_same_rows(path, new, old)
    _check_improvement(new, old)


def test_hot_factor_ends_in_both_streams(program, tmp_path):
    """One level of 32 rows T_j += M[hot] M[k], k one of eight basics, the hot factor written as a0 in all of them: in
    a 16-row group the 16 adds to D[hot] serialise in one stream and every D[k] is added to twice in the other; with
    exchanges each group can hold hot and every k once per stream."""
    slots = [(0, 0), (0, 1), (0, 2)]
    basic = [(mu,) + m for (mu, nu) in slots for m in mtpgen.monomials(nu)]
    assert basic[0] == (0, 0, 0, 0) and len(basic) >= 9
    B, hot = len(basic), 0
    times = [(hot, 1 + j % 8, 1, B + j) for j in range(32)]          # level 1: the products, stored ...
    scalar = B + 32
    times += [(B + j, B + j, 1, scalar) for j in range(32)]          # ... because the leaf rows read them
    tab = mtpgen.MTPTable(level=0, basic=basic, times=times, mapping=[hot, scalar], nmoments=scalar + 1)
    tab.radial_funcs = 1
    path = _tables.write(tab, np.array([1, 4]), str(tmp_path / "hot.mtp"))
    assert all(r[0] == hot for r in _file_rows(path)[:32])
    new = _load(program, path, "v2", SUITE)
    assert new["search"] == "v2" and new["levels"] == 1
    rows = _in_file_numbering(new)[:new["level_offset"][1]]
    real = rows[rows[:, 2] != 0]
    assert len(real) == 32 and all((r[0] == hot) != (r[1] == hot) for r in real.tolist())
    as_a0, as_a1 = int((real[:, 0] == hot).sum()), int((real[:, 1] == hot).sum())
    print("hot factor as a0 in %d rows, as a1 in %d" % (as_a0, as_a1))
    assert as_a0 > 0 and as_a1 > 0
    # v1 cannot exchange: the factor stays where the file has it
    old = _load(program, path, "v1", SUITE)
    rows_old = _in_file_numbering(old)[:old["level_offset"][1]]
    assert all(r[0] == hot for r in rows_old[rows_old[:, 2] != 0].tolist())
    assert new["model"] < old["model"]


def test_zero_rounds_is_no_search(program, tables):
    path = os.path.join(POT, "W_L16.mtp")
    a, b = _load(program, path, "v1", (0, 1)), _load(program, path, "v2", (0, 1))
    _check_table(b, tables["W_L16.mtp@v2@0x1"])
    assert a["hash"] == b["hash"] and a["model"] == a["before"] == b["model"]
    assert np.array_equal(a["perm"][:a["B"]], np.arange(a["B"]))


def test_sanitized_program_runs_clean(tmp_path):
    """a stand-alone program with its own main, built with -fsanitize=address,undefined: nothing is loaded into Python"""
    exe = _build(str(tmp_path / "bank_search_dump_san"), extra=SANITIZE)
    r = _load(exe, os.path.join(POT, "W_L16.mtp"), "v2", SUITE)
    assert r["search"] == "v2" and "runtime error" not in r["stderr"] and "AddressSanitizer" not in r["stderr"]


def test_state_against_recount(tmp_path):
    """tests/cpp/bank_state_check.cpp: a stand-alone program with its own main on csrc/mtp_bank_search.hpp alone, built
    with -fsanitize=address,undefined; it exits non-zero at the first mismatch of State and recount"""
    exe = _build(str(tmp_path / "bank_state_check"), extra=SANITIZE, src=[os.path.join(ROOT, "tests", "cpp", "bank_state_check.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("bank_state_check: ok, 20000 mutations") and r.stderr == ""
