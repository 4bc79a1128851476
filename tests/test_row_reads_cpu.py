"""The rows of the first product level kept across the atom loop of the fixed force shape w16_force_3ps
(csrc/mtp_wave_body.hpp: row_keep_l1_ct, beside row_regs_ct), without a GPU.

The trait is checked as what it is, a compile-time constant: a syntax-only device pass of hipcc over the kernel's
headers with static_asserts (as tests/test_force_regs_cpu.py does for row_regs_ct).  It is on for the force shape, off
for the grade shape and the generic kernels, and off for stand-in shapes: the force shape with a first level of one
block (nothing long to keep a part of), with a first level shorter than the kept part, and with its rows outside LDS.

The function itself, read from the gfx950 code object in libmtp_mi355x.so with the ROCm LLVM tools (tests/_codeobj.py):
at most 168 VGPRs, no spilled VGPR or SGPR, no scratch, and the atom loop (from its first s_setprio on)
holds eight row reads of the first level fewer than with the switch off would need: the level's ten blocks are two
trips from registers and three trips of two reads, in each pass."""
import os
import re
import subprocess

import pytest

from _codeobj import LIB, _kernels, _tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps_mtp_kokkos_amd", "csrc")
FORCE = "w16_force_3ps"
ARGS = "ILi32ELi1ELi33ELb0ELi6ELi3E"

TRAITS = r"""
#include "mtp_wave_body.hpp"
#include "mtp_fixed_shapes.hpp"
static_assert(row_keep_l1_ct<Shape_w16_force_3ps>, "on in the force shape");
static_assert(ROW_KEEP_L1 == 4 && kept_l1_count<Shape_w16_force_3ps>() == 4, "four blocks: two trips at MTP_PU = 2");
static_assert(level_blocks<Shape_w16_force_3ps>(0) == 10 && !level_kept<Shape_w16_force_3ps>(0), "a long first level");
static_assert(kept_count<Shape_w16_force_3ps>() == 3, "the short levels keep their three blocks");
static_assert(!row_keep_l1_ct<Shape_w16_grade_3ps> && !row_keep_l1_shape<Shape_w16_grade_3ps>(), "off in the grade shape");
static_assert(!row_keep_l1_ct<ShapeGeneric> && !row_keep_l1_shape<ShapeGeneric>(), "off in the generic kernels");
// stand-ins: the force shape with another level table, or with its rows in HBM / L2
struct OneBlockFirst : Shape_w16_force_3ps {
  static constexpr int level_rows(int k)
  {
    constexpr int v[14] = {0, 64, 192, 256, 448, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return v[k];
  }
};
static_assert(level_blocks<OneBlockFirst>(0) == 1 && !row_keep_l1_ct<OneBlockFirst>, "a one-block first level");
struct ThreeBlockFirst : Shape_w16_force_3ps {
  static constexpr int level_rows(int k)
  {
    constexpr int v[14] = {0, 192, 320, 384, 576, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return v[k];
  }
};
static_assert(row_regs_ct<ThreeBlockFirst> && !row_keep_l1_ct<ThreeBlockFirst>, "a first level shorter than the kept part");
struct RowsFar : Shape_w16_force_3ps {
  static constexpr int rows_in_lds = 0;
};
static_assert(!row_regs_ct<RowsFar> && !row_keep_l1_ct<RowsFar>, "rows outside LDS");
struct GradeTwin : Shape_w16_force_3ps {
  static constexpr bool kGRADE = true;
};
static_assert(!row_keep_l1_ct<GradeTwin>, "a grade call");
static_assert(MTP_ROW_KEEP_L1 == 1, "the switch defaults to on");
"""


def test_trait_selects_the_force_shape_only(tmp_path):
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
    if not os.access(hipcc, os.X_OK):
        pytest.skip("hipcc not found")
    src = tmp_path / "traits.hip"
    src.write_text(TRAITS)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-fsyntax-only", "-I", CSRC,
                        "-x", "hip", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_a_failing_assertion_is_noticed(tmp_path):
    """the pass above is a check: the same translation unit with the trait's value turned round does not compile"""
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
    if not os.access(hipcc, os.X_OK):
        pytest.skip("hipcc not found")
    src = tmp_path / "traits_wrong.hip"
    src.write_text(TRAITS + 'static_assert(row_keep_l1_ct<RowsFar>, "must fail");\n')
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-fsyntax-only", "-I", CSRC,
                        "-x", "hip", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "must fail" in r.stderr


def test_switch_is_named_by_the_build_flags():
    text = open(os.path.join(CSRC, "mtp_wave_body.hpp")).read()
    assert re.search(r"#ifndef MTP_ROW_KEEP_L1\n#define MTP_ROW_KEEP_L1 1 ", text)
    assert re.search(r"constexpr bool row_keep_l1_ct = MTP_ROW_KEEP_L1 && row_regs_ct<SH> && row_keep_l1_shape<SH>\(\);", text)
    flags = open(os.path.join(CSRC, "mtp_kernels.hip")).read()
    assert '"MTP_ROW_KEEP_L1=" MTP_STR(MTP_ROW_KEEP_L1)' in flags


KERNEL_UNITS = ("mtp_wave_body.hpp", "mtp_wave_kernel_body.hpp", "mtp_kernels.hip", "mtp_kernels_fixed.hip",
                "mtp_kernel_common.hpp")
# the twelve retired switches, without their MTP_ prefix (a search of the tree for a retired name then finds nothing)
RETIRED = ["MTP_" + s for s in ("LD", "POLY_ACC", "POLY_CH", "COEF_DPP", "LEAF_SWEEP", "E_HOIST", "MU_BITS", "LEVEL_ARGS",
                                "SLOT_ARGS", "FP_REGS", "BLOCK_REGS", "ROW_REGS")]


def _switch_defaults(text):
    """the MTP_ names given a default: every #define between an #ifndef MTP_... and its #endif"""
    names, inside = [], False
    for line in text.splitlines():
        if re.match(r"#\s*ifndef\s+MTP_\w+", line):
            inside = True
        elif re.match(r"#\s*endif", line):
            inside = False
        elif inside:
            names += re.findall(r"^#\s*define\s+(MTP_\w+)", line)
    return names


def test_every_switch_default_is_named_by_the_build_flags():
    """A library built with any compile-time switch of the force or grade kernels off its default says so: every default
    in the kernels' files has its entry in mtp_kernel_build_flags(), so that build_flags() == "" (tests/test_domain_cpu.py)
    means the shipped values.  MTP_GRADE_WPE is set together with MTP_GRADE_TPB and reported under its entry."""
    flags = open(os.path.join(CSRC, "mtp_kernels.hip")).read()
    body = flags[flags.index("const char *mtp_kernel_build_flags()"):]
    body = body[:body.index("\n}\n")]
    found = []
    for unit in KERNEL_UNITS:
        found += _switch_defaults(open(os.path.join(CSRC, unit)).read())
    assert {"MTP_PU", "MTP_FWD5", "MTP_SUM_T", "MTP_CNT_SGPR", "MTP_GRADE_TPB", "MTP_GRADE_WPE"} <= set(found), found
    for name in found:
        if name != "MTP_GRADE_WPE":
            assert '"%s=" MTP_STR(%s)' % (name, name) in body, name
    assert "MTP_GRADE_WPE" in body


def test_retired_switches_are_gone_from_the_sources():
    """the switches of decided comparisons left the sources with the arm that lost"""
    pattern = re.compile(r"\b(%s)\b" % "|".join(RETIRED))
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path) and not name.endswith(".so"):
            hits = pattern.findall(open(path, errors="replace").read())
            assert not hits, (name, hits)


@pytest.fixture(scope="module")
def force_function(tmp_path_factory):
    """(resource notes, [(address, instruction text)]) of w16_force_3ps; every offload bundle of the library is read"""
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    if not all(tools.values()):
        pytest.skip("ROCm LLVM tools not found")
    if not os.path.exists(LIB):
        pytest.skip("libmtp_mi355x.so not built")
    d = tmp_path_factory.mktemp("co_row_reads")
    fb = str(d / "fatbin")
    subprocess.check_call([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", LIB, fb])
    data = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)] + [len(data)]
    for k in range(len(starts) - 1):
        part, co = str(d / ("bundle%d" % k)), str(d / ("gfx950_%d.elf" % k))
        with open(part, "wb") as f:
            f.write(data[starts[k]:starts[k + 1]])
        subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part, "--output=" + co])
        if os.path.getsize(co) == 0:
            continue
        kernels = _kernels(subprocess.run([tools["llvm-readelf"], "--notes", co], check=True, capture_output=True,
                                          text=True).stdout)
        names = [n for n in kernels if "mtp_wave_kernel_fixed" + ARGS in n and "Shape_" + FORCE in n]
        if not names:
            continue
        assert len(names) == 1, names
        dis = subprocess.run([tools["llvm-objdump"], "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                             text=True).stdout
        body, inside = [], False
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                inside = m.group(1) == names[0]
            elif inside and line.startswith("\t") and "//" in line:
                text, note = line.split("//", 1)
                body.append((int(note.split(":")[0].strip(), 16), text.strip(), note))
        assert body
        return kernels[names[0]], body
    pytest.fail("w16_force_3ps is in no code object of the library")


def _atom_loop(body):
    """the instructions from the atom loop's head on: the loop opens with the first s_setprio of the function (the
    shape sets its issue priority by phase, csrc/mtp_wave_body.hpp phase_prio), and what follows the loop -- the fold of
    the tallies -- reads no LDS"""
    texts = [text for _, text, _ in body]
    head = next(k for k, text in enumerate(texts) if text.startswith("s_setprio"))
    assert any(text.startswith("s_barrier") for text in texts[:head])   # the table copy and the kept rows stand ahead of it
    return texts[head:]


def test_force_kernel_stays_inside_three_wavefronts_per_simd(force_function):
    r, _ = force_function
    assert r["vgpr_count"] <= 168, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r


def test_atom_loop_reads_six_blocks_of_the_first_level_per_pass(force_function):
    """Each pass reads the rows of a trip's two blocks with one ds_read2st64_b64 (512 bytes apart).  With all ten blocks
    of the first level read per atom that is five a pass, ten in the loop, beside the leaf sweep's and the coefficient
    blocks' (four: the count with the switch off is fourteen); with four blocks in registers, three a pass: ten."""
    _, body = force_function
    loop = _atom_loop(body)
    assert len(loop) > len(body) // 2, (len(loop), len(body))   # the loop is most of the function
    st64 = [t for t in loop if t.startswith("ds_read2st64_b64")]
    print("ds_read2st64_b64 in the atom loop: %d" % len(st64))
    assert len(st64) == 10, st64
    assert sum(1 for t in loop if t.startswith("ds_add_f64")) == 45   # every add of the passes is still there
