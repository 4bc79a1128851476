"""Issue priority by phase in the fixed force kernel (csrc/mtp_wave_body.hpp, MTP_PHASE_PRIO; csrc/mtp_wave_kernel_body.hpp)
without a GPU, read from the gfx950 code objects in libmtp_mi355x.so with the ROCm LLVM tools (tests/_codeobj.py; every
offload bundle of the library, as tests/test_fixed_shapes_cpu.py does).

w16_force_3ps holds the s_setprio instructions of the four phase boundaries of an atom -- raised at the loop head and
behind the basic moments, lowered behind the compaction and behind the reverse product pass -- and one behind the atom
loop, alternating in program order, and stays inside the budget of three wavefronts per SIMD.  No other kernel of the
library holds an s_setprio: the generic force kernels and the grade shape are not touched by the switch.  The traits are
checked as what they are, compile-time constants, by a syntax-only device pass over the kernel's headers.

(The start offset per SIMD slot that was measured beside the priorities is not in the sources:
profiles/r13_ab_wave_phases.txt.)"""
import os
import re
import subprocess

import pytest

from _codeobj import LIB, _kernels, _tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps_mtp_kokkos_amd", "csrc")
FORCE = "w16_force_3ps"


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    if not all(tools.values()):
        pytest.skip("ROCm LLVM tools not found")
    if not os.path.exists(LIB):
        pytest.skip("libmtp_mi355x.so not built")
    d = tmp_path_factory.mktemp("co_phase_prio")
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


def _setprio(dis):
    """{function: the operands of its s_setprio instructions, in program order}"""
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.startswith("\t"):
            ins = line.split("//")[0].split()
            if ins and ins[0] == "s_setprio":
                out[cur].append(int(ins[1], 0))
    return out


def test_force_kernel_sets_its_priority_at_the_phase_boundaries(code_objects):
    kernels, dis = code_objects
    prio = _setprio(dis)
    names = [n for n in kernels if "mtp_wave_kernel_fixed" in n and "Shape_" + FORCE in n]
    assert len(names) == 1, names
    got = prio[names[0]]
    print("s_setprio of %s: %s" % (FORCE, got))
    assert got == [2, 0, 2, 0, 0], got   # loop head, compaction | basic moments, reverse pass | behind the loop
    r = kernels[names[0]]
    assert r["vgpr_count"] <= 168 and r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["sgpr_spill_count"] == 0, r


def test_no_other_kernel_sets_a_priority(code_objects):
    kernels, dis = code_objects
    prio = _setprio(dis)
    others = {n: v for n, v in prio.items() if v and not ("mtp_wave_kernel_fixed" in n and "Shape_" + FORCE in n)}
    assert not others, others
    assert sum(1 for n in kernels if "mtp_wave_kernelILi" in n) >= 28   # the generic force kernels were read


TRAITS = r"""
#include "mtp_wave_body.hpp"
#include "mtp_fixed_shapes.hpp"
static_assert(MTP_PHASE_PRIO == 1 && phase_prio_ct<Shape_w16_force_3ps>, "on in the force shape");
static_assert(!phase_prio_ct<Shape_w16_grade_3ps>, "off in the grade shape");
static_assert(!phase_prio_ct<ShapeGeneric>, "off in the generic kernels");
static_assert(MTP_PRIO_CHAIN > MTP_PRIO_BURST && MTP_PRIO_CHAIN <= 3 && MTP_PRIO_BURST >= 0, "s_setprio takes 0 .. 3");
"""


def test_priorities_are_off_in_the_grade_shape_and_the_generic_kernels(tmp_path):
    hipcc = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"))
    if not os.access(hipcc, os.X_OK):
        pytest.skip("hipcc not found")
    src = tmp_path / "traits.hip"
    src.write_text(TRAITS)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-fsyntax-only", "-I", CSRC,
                        "-x", "hip", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
