"""Code-object checks of the built library (no GPU) that go with the parameter-block measurements of
profiles/r06_ab_param_loads.txt: the scalar loads of the headline force kernel and the VGPR spills of every
mtp_wave_kernel instantiation against the record in profiles/r05_code_objects.txt.  Reads the gfx950 code object
embedded in libmtp_mi355x.so with the ROCm LLVM tools; skips where they are not installed."""
import os
import re

from _codeobj import ROOT, _kernels, code_object  # noqa: F401  (code_object: fixture)

HEADLINE = "mtp_wave_kernelILi32ELi1ELi33ELb0ELi6ELi3E"
# s_load_* instructions in the headline function.  121 is the parent's count at 7f218e6, and it is also what this
# build has: the measurements found the argument-block loads free (r06_ab_param_loads.txt), so none was removed, and
# the parent's count is pinned as the guard against new ones.
HEADLINE_S_LOADS = 121


def _function(dis, key):
    out, cur = [], False
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = key in m.group(1)
        elif cur and line.startswith("\t"):
            ins = line.split("//")[0].strip()
            if ins:
                out.append(ins)
    return out


def _r05_spills():
    """{(KL, NB, PITCH, GRADE, DEG, WPS): spilled VGPR dwords} from the table in profiles/r05_code_objects.txt"""
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "r05_code_objects.txt")):
        m = re.match(r"<(\d+), (\d+), (\d+), (true|false), (\d+), (\d+)>\s+\d+\s+\d+\s+(\d+)", line)
        if m:
            out[tuple(int(m.group(k)) for k in (1, 2, 3)) + (m.group(4) == "true", int(m.group(5)), int(m.group(6)))] = \
                int(m.group(7))
    return out


def test_headline_scalar_loads(code_object):
    ins = _function(code_object[1], HEADLINE)
    assert ins
    n = sum(1 for i in ins if i.startswith("s_load_"))
    assert n <= HEADLINE_S_LOADS, n


def test_no_instantiation_spills_more_than_r05(code_object):
    want = _r05_spills()
    assert len(want) == 28, len(want)
    seen = 0
    for name, r in _kernels(code_object[0]).items():
        m = re.search(r"mtp_wave_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELi(\d+)ELi(\d+)E", name)
        if not m:
            continue
        key = tuple(int(m.group(k)) for k in (1, 2, 3)) + (m.group(4) == "1", int(m.group(5)), int(m.group(6)))
        assert key in want, name
        assert r["vgpr_spill_count"] <= want[key], (name, r, want[key])
        seen += 1
    assert seen == len(want), seen
