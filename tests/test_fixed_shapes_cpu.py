"""Fixed-shape force kernels without a GPU (csrc/mtp_kernels_fixed.hip, csrc/mtp_shape_fields.hpp): the committed
shapes are what the generator writes, the host-only planner matches a launch to a shape exactly when the table
structure and the LDS plan are the shape's -- whatever the fit -- and the fixed kernels in the built library keep the
register budget recorded in profiles/r07_code_objects.txt."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from _codeobj import LIB, ROOT, _kernels, _tool
from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.domain import decompose

POT = os.path.join(ROOT, "potentials")
CUS = 256
FORCE, GRADE = "w16_force_3ps", "w16_grade_3ps"


def _generator():
    spec = importlib.util.spec_from_file_location("gen_fixed_shapes", os.path.join(ROOT, "scripts", "gen_fixed_shapes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def bench_max_numneigh():
    """longest list row of the headline workload (bench.py: 32^3 BCC cells, a = 3.165, jitter 0.05, list cutoff 7.0)"""
    pos, box = mtpgen.bcc_lattice(32, 32, 32, a=3.165, jitter=0.05, seed=777)
    plan = decompose(pos, box, None, 1, 0, 7.0)
    assert plan.nlocal == 65536
    return int(np.diff(plan.first).max())


def _written(tmp_pot_dir, name, pot):
    path = str(tmp_pot_dir / name)
    mtpgen.write_mtp(pot, path)
    return path


def test_generator_reproduces_the_committed_include():
    gen = _generator()
    assert gen.include_text() == open(gen.OUT).read()
    first = open(gen.OUT).read().splitlines()[1]
    assert "scripts/gen_fixed_shapes.py" in first   # the header names the generator command


def test_shape_names_are_those_of_the_generator():
    assert [s["name"] for s in _generator().SHAPES] == [FORCE, GRADE]


def test_headline_and_grade_launches_match_their_shapes(bench_max_numneigh):
    pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
    assert pot.plan_fixed_shape(CUS, 65536, bench_max_numneigh) == FORCE
    sel = capi.Potential(os.path.join(POT, "W_L16_nbh.almtp"), selection=True)
    assert sel.plan_fixed_shape(CUS, 65536, bench_max_numneigh, grade=True) == GRADE
    # a force call of the potential with selection data is a force launch of the same table
    assert sel.plan_fixed_shape(CUS, 65536, bench_max_numneigh, grade=False) == FORCE


def test_refit_of_the_same_table_matches(tmp_pot_dir, bench_max_numneigh):
    """other coefficients, cutoffs and scaling: none of them is a shape field"""
    p = mtpgen.random_potential(mtpgen.build_table(16), 1, 20251, 1.7, 5.6, 8, 0.37)
    pot = capi.Potential(_written(tmp_pot_dir, "refit16.mtp", p))
    assert pot.plan_fixed_shape(CUS, 65536, bench_max_numneigh) == FORCE
    want = capi.Potential(os.path.join(POT, "W_L16.mtp")).plan_fixed_fields(CUS, 65536, bench_max_numneigh)
    assert pot.plan_fixed_fields(CUS, 65536, bench_max_numneigh) == want


def test_other_tables_and_plans_do_not_match(tmp_pot_dir, bench_max_numneigh, monkeypatch):
    n = bench_max_numneigh
    assert capi.Potential(os.path.join(POT, "W_L8.mtp")).plan_fixed_shape(CUS, 65536, n) == ""
    two = mtpgen.random_potential(mtpgen.build_table(16), 2, 4242)
    assert capi.Potential(_written(tmp_pot_dir, "two16.mtp", two)).plan_fixed_shape(CUS, 65536, n) == ""
    r9 = mtpgen.random_potential(mtpgen.build_table(16), 1, 4242, 2.0, 5.0, 9, 1.0)
    assert capi.Potential(_written(tmp_pot_dir, "r9_16.mtp", r9)).plan_fixed_shape(CUS, 65536, n) == ""
    w16 = os.path.join(POT, "W_L16.mtp")
    # a 2,048-atom plan (fewer than 16 atoms per CU: two wavefronts per SIMD), and the small variant at any size
    assert capi.Potential(w16).plan_fixed_shape(CUS, 2048, n) == ""
    assert capi.Potential(w16).plan_fixed_shape(CUS, 65536, n, variant=capi.VARIANT_SMALL) == ""
    with monkeypatch.context() as m:
        m.setenv("MTP_LAYOUT", "keep")
        assert capi.Potential(w16).plan_fixed_shape(CUS, 65536, n) == ""
    with monkeypatch.context() as m:
        m.setenv("MTP_NO_LEAF", "1")
        assert capi.Potential(w16).plan_fixed_shape(CUS, 65536, n) == ""
    assert capi.Potential(w16).plan_fixed_shape(CUS, 65536, n) == FORCE


def test_match_does_not_depend_on_the_bank_search_effort(bench_max_numneigh, monkeypatch):
    """the search renumbers moments and swaps rows inside a level: table contents, never a shape field"""
    fields = []
    for rounds in ("0", "2", "8"):
        with monkeypatch.context() as m:
            m.setenv("MTP_BANK_ROUNDS", rounds)
            if rounds == "8":
                m.delenv("MTP_BANK_SCALE", raising=False)
            pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
        assert pot.plan_fixed_shape(CUS, 65536, bench_max_numneigh) == FORCE
        fields.append(pot.plan_fixed_fields(CUS, 65536, bench_max_numneigh))
    assert fields[0] == fields[1] == fields[2]


def test_planner_arguments_are_checked():
    pot = capi.Potential(os.path.join(POT, "W_L16.mtp"))
    with pytest.raises(capi.MtpError):
        pot.plan_fixed_shape(0, 65536, 94)
    with pytest.raises(capi.MtpError):
        pot.plan_fixed_shape(CUS, 65536, 94, variant=7)


# ---- the code objects ----------------------------------------------------------------------------------------------
# Every translation unit of the library carries a code object of its own in .hip_fatbin (the fixed-shape kernels are
# not in the one of mtp_kernels.hip that the `code_object` fixture of _codeobj.py reads): all of them are read here.
@pytest.fixture(scope="module")
def all_code_objects(tmp_path_factory):
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    if not all(tools.values()):
        pytest.skip("ROCm LLVM tools not found")
    if not os.path.exists(LIB):
        pytest.skip("libmtp_mi355x.so not built")
    d = tmp_path_factory.mktemp("co_all")
    fb = str(d / "fatbin")
    subprocess.check_call([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", LIB, fb])
    data = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)] + [len(data)]
    notes, dis = "", ""
    for k in range(len(starts) - 1):
        part, co = str(d / ("bundle%d" % k)), str(d / ("gfx950_%d.elf" % k))
        with open(part, "wb") as f:
            f.write(data[starts[k]:starts[k + 1]])
        subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part, "--output=" + co])
        if os.path.getsize(co) == 0:
            continue
        notes += subprocess.run([tools["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
        dis += subprocess.run([tools["llvm-objdump"], "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                              text=True).stdout
    return notes, dis


def _s_loads(dis, key):
    n, cur, found = 0, False, 0
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = key in m.group(1)
            found += cur
        elif cur and line.startswith("\t") and line.split("//")[0].strip().startswith("s_load_"):
            n += 1
    assert found == 1, (key, found)
    return n


def _r07_spills():
    """{shape name: spilled VGPR dwords} from the fixed-kernel table of profiles/r07_code_objects.txt"""
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "r07_code_objects.txt")):
        m = re.match(r"fixed\s+(\w+)\s+<[^>]*>\s+(\d+)\s+(\d+)\s", line)
        if m:
            out[m.group(1)] = int(m.group(3))
    return out


def test_fixed_kernels_are_present_and_within_their_budget(all_code_objects):
    notes, dis = all_code_objects
    kernels = _kernels(notes)
    want = _r07_spills()
    shapes = _generator().SHAPES
    assert set(want) == {s["name"] for s in shapes}
    for s in shapes:
        grade = "Lb1E" if s["grade"] else "Lb0E"
        args = "ILi32ELi1ELi33E%sLi6ELi3E" % grade
        fixed = [n for n in kernels if "mtp_wave_kernel_fixed" + args in n and "Shape_" + s["name"] in n]
        assert len(fixed) == 1, (s["name"], fixed)
        assert "mtp_wave_kernelILi" not in fixed[0]
        r = kernels[fixed[0]]
        assert r["vgpr_count"] <= 168, (fixed[0], r)                       # three wavefronts per SIMD
        assert r["vgpr_spill_count"] <= want[s["name"]], (fixed[0], r, want[s["name"]])
        assert _s_loads(dis, fixed[0]) < _s_loads(dis, "mtp_wave_kernel" + args), s["name"]
