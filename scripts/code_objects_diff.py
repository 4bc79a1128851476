#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libmtp_mi355x.so, function by function (no GPU).

    python scripts/code_objects_diff.py PARENT.so NEW.so

Every offload bundle of both libraries is unbundled (as tests/_codeobj.py and tests/test_fixed_shapes_cpu.py do), every
code object disassembled with llvm-objdump -d --no-show-raw-insn, and the kernel notes read with llvm-readelf.  A
function is its instruction texts in order; the address column and the symbolic branch target that objdump appends
behind "//" are set aside, so that a function that merely moved inside its code object compares equal (a branch
operand is relative and stays).  Two functions are equal when every instruction and every note agree.

Prints
    functions: parent N new N common N
    distinct names: parent N new N          (a template that two translation units instantiate has a copy in each)
    equal instruction for instruction: N
and, per differing function, its notes in both builds and the first instruction that differs; functions that only one
build has are listed by name.  Exit status 0 when the function sets agree and all are equal, 1 otherwise."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

NOTES = ("vgpr_count", "vgpr_spill_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size",
         "group_segment_fixed_size")
SHORT = {"vgpr_count": "vgpr", "vgpr_spill_count": "vgpr_spill", "agpr_count": "agpr", "sgpr_count": "sgpr",
         "sgpr_spill_count": "sgpr_spill", "private_segment_fixed_size": "scratch", "group_segment_fixed_size": "lds"}


def tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    p = shutil.which(name)
    if not p:
        sys.exit("code_objects_diff: %s not found" % name)
    return p


def kernel_notes(text):
    """{kernel symbol without .kd: {note: value}} from llvm-readelf --notes"""
    out = {}
    for ent in re.split(r"\n  - (?=\.)", text):
        m = re.search(r"\.name:\s+(\S+)", ent)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(NOTES), ent)}
    return out


def functions(lib, work):
    """{function: (notes, [instruction text])} over every gfx950 code object of the library"""
    fb = os.path.join(work, "fatbin")
    subprocess.check_call([tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fb])
    data = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)] + [len(data)]
    out = {}
    for k in range(len(starts) - 1):
        part, co = os.path.join(work, "bundle%d" % k), os.path.join(work, "gfx950_%d.elf" % k)
        with open(part, "wb") as f:
            f.write(data[starts[k]:starts[k + 1]])
        subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part, "--output=" + co])
        if os.path.getsize(co) == 0:
            continue
        notes = kernel_notes(subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                            text=True).stdout)
        dis = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                             text=True).stdout
        name = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                sym, n = m.group(1), 1
                name = sym
                while name in out:   # a library template instantiated by two translation units: one copy in each
                    n += 1
                    name = "%s [copy %d]" % (sym, n)
                out[name] = (notes.get(sym, {}), [])
            elif name is not None and line.startswith("\t"):
                out[name][1].append(line.split("//", 1)[0].strip())
    return out


def show_notes(n):
    return " ".join("%s %d" % (SHORT[k], n[k]) for k in NOTES if k in n)


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        a, b = functions(argv[1], da), functions(argv[2], db)
    common = sorted(set(a) & set(b))
    differ = [f for f in common if a[f] != b[f]]
    print("functions: parent %d new %d common %d" % (len(a), len(b), len(common)))
    print("distinct names: parent %d new %d" % tuple(sum(1 for f in x if "[copy " not in f) for x in (a, b)))
    print("equal instruction for instruction: %d" % (len(common) - len(differ)))
    for label, only in (("parent", sorted(set(a) - set(b))), ("new", sorted(set(b) - set(a)))):
        for f in only:
            print("only in %s: %s" % (label, f))
    for f in differ:
        (na, ia), (nb, ib) = a[f], b[f]
        print(f)
        print("  parent  %s insts %d" % (show_notes(na), len(ia)))
        print("  new     %s insts %d" % (show_notes(nb), len(ib)))
        k = next((k for k, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
        if k < len(ia) or k < len(ib):
            print("  first difference at instruction %d: parent `%s` | new `%s`"
                  % (k, ia[k] if k < len(ia) else "(end)", ib[k] if k < len(ib) else "(end)"))
        else:
            print("  the instructions agree: the notes differ")
    return 0 if not differ and len(common) == len(a) == len(b) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
