"""The fixed force kernel w16_force_3ps after the register levers of csrc/mtp_wave_body.hpp (block_regs_ct: the row
offsets of a lane's basic-moment block kept across the atom loop; row_regs_ct: the packed rows of the short product
levels kept across it), without a GPU: read from the gfx950 code object in libmtp_mi355x.so with the ROCm LLVM tools
(tests/_codeobj.py), the function stays inside the budget of three wavefronts per SIMD -- at most 168 VGPRs, no spilled
VGPR dword, no scratch, no spilled SGPR -- and holds fewer static LDS instructions than its parent, whose count, 711
(profiles/r09_code_objects.txt), was recounted with the counting rule below on the parent's library before the change
(711 again; the shipped function has 709: the levers take reads out of the atom loop, and most of them stand once
ahead of it instead).

The library embeds one offload bundle per translation unit, so every bundle is read (as tests/test_fixed_shapes_cpu.py
does); the tools and the note parser are those of tests/_codeobj.py.

The traits of the levers are checked as what they are, compile-time constants: a syntax-only pass of hipcc over the
kernel's headers with static_asserts that they are on for the force shape and off for the grade shape and for
ShapeGeneric (profiles/r10_code_objects.txt shows the same from the other side: those kernels are the parent's code
objects column for column)."""
import os
import re
import subprocess

import pytest

from _codeobj import LIB, _kernels, _tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCE = "w16_force_3ps"
ARGS = "ILi32ELi1ELi33ELb0ELi6ELi3E"
PARENT_DS = 711   # static LDS instructions of the parent's w16_force_3ps (recounted: 711)


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    if not all(tools.values()):
        pytest.skip("ROCm LLVM tools not found")
    if not os.path.exists(LIB):
        pytest.skip("libmtp_mi355x.so not built")
    d = tmp_path_factory.mktemp("co_force_regs")
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
    return _kernels(notes), dis


def _lds_instructions(dis):
    """{function: static LDS instructions of any kind (mnemonic ds_*)}"""
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif cur and line.startswith("\t") and line.split("//")[0].strip().startswith("ds_"):
            out[cur] += 1
    return out


def _force_kernel(kernels):
    names = [n for n in kernels if "mtp_wave_kernel_fixed" + ARGS in n and "Shape_" + FORCE in n]
    assert len(names) == 1, names
    return names[0]


def test_force_kernel_keeps_three_wavefronts_per_simd(code_objects):
    kernels, _ = code_objects
    r = kernels[_force_kernel(kernels)]
    assert r["vgpr_count"] <= 168, r
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["sgpr_spill_count"] == 0, r   # the parent's count


def test_force_kernel_has_fewer_lds_instructions_than_its_parent(code_objects):
    kernels, dis = code_objects
    ds = _lds_instructions(dis)[_force_kernel(kernels)]
    print("static LDS instructions of %s: %d (parent %d)" % (FORCE, ds, PARENT_DS))
    assert ds < PARENT_DS, ds


TRAITS = r"""
#include "mtp_wave_body.hpp"
#include "mtp_fixed_shapes.hpp"
static_assert(block_regs_ct<Shape_w16_force_3ps> && row_regs_ct<Shape_w16_force_3ps>, "on in the force shape");
static_assert(kept_count<Shape_w16_force_3ps>() == 3, "levels 1 and 2 of the level-16 table: 2 + 1 blocks");
static_assert(!block_regs_ct<Shape_w16_grade_3ps> && !row_regs_ct<Shape_w16_grade_3ps>, "off in the grade shape");
static_assert(!block_regs_ct<ShapeGeneric> && !row_regs_ct<ShapeGeneric>, "off in the generic kernels");
"""


def test_levers_are_off_in_the_grade_shape_and_the_generic_kernels(tmp_path):
    """the traits themselves, by a syntax-only device pass over the kernel's headers (nothing is built or linked)"""
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
    if not os.access(hipcc, os.X_OK):
        pytest.skip("hipcc not found")
    src = tmp_path / "traits.hip"
    src.write_text(TRAITS)
    csrc = os.path.join(ROOT, "lammps_mtp_kokkos_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-fsyntax-only", "-I", csrc,
                        "-x", "hip", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
