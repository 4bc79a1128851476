"""The gfx950 code object embedded in libmtp_mi355x.so, read with the ROCm LLVM tools (no GPU): the `code_object`
fixture skips where they are not installed.  Shared by tests/test_isa_cpu.py and tests/test_shapes_cpu.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lammps_mtp_kokkos_amd", "libmtp_mi355x.so")


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    tools = {n: _tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")}
    if not all(tools.values()):
        pytest.skip("ROCm LLVM tools not found")
    if not os.path.exists(LIB):
        pytest.skip("libmtp_mi355x.so not built")
    d = tmp_path_factory.mktemp("co")
    fb, co = str(d / "fatbin"), str(d / "gfx950.elf")
    subprocess.check_call([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", LIB, fb])
    subprocess.check_call([tools["clang-offload-bundler"], "--unbundle", "--type=o",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co])
    notes = subprocess.run([tools["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
    dis = subprocess.run([tools["llvm-objdump"], "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                         text=True).stdout
    return notes, dis


def _kernels(notes):
    out = {}
    for ent in re.split(r"\n  - (?=\.)", notes):
        m = re.search(r"\.name:\s+(\S+)", ent)
        if not m:
            continue
        out[m.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(vgpr_count|vgpr_spill_count|sgpr_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ent)}
    return out
