"""Code-object checks of the built library (no GPU): register budget of the headline force kernel and the DPP form
of the force phase's coefficient broadcast (csrc/mtp_kernels.hip, poly_eval_dpp; csrc/mtp_kernel_common.hpp,
fmac_row_bcast).  Reads the gfx950 code object embedded in libmtp_mi355x.so with the ROCm LLVM tools; skips where
they are not installed."""
import re

from _codeobj import _kernels, code_object  # noqa: F401  (code_object: fixture)

# the level-16 headline shape: KL = 32 block lanes, one block per lane, pitch 33, force call, ranks <= 6, 3 per SIMD
HEADLINE = "mtp_wave_kernelILi32ELi1ELi33ELb0ELi6ELi3E"


def _functions(dis):
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            ins = line.split("//")[0].strip()
            if ins:
                cur.append(ins)
    return out


def _vgprs(op):
    m = re.match(r"v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", op)
    return {int(m.group(1))} if m else set()


def _dpp_hazards(ins):
    """v_fmac_f64_dpp whose broadcast operand (src0) a VALU instruction wrote fewer than 2 wait states earlier in
    the same straight-line code (the hazard hipcc does not pad ahead of an asm statement)."""
    bad = []
    for k, i in enumerate(ins):
        if not i.startswith("v_fmac_f64_dpp"):
            continue
        src0 = _vgprs(i.split(None, 1)[1].split(",")[1].strip())
        states, j = 0, k - 1
        while j >= 0 and states < 2:
            p = ins[j]
            if p.startswith(("s_branch", "s_cbranch", "s_setpc", "s_endpgm")):
                break
            nop = re.match(r"s_nop (\d+)", p)
            if nop:
                states += int(nop.group(1)) + 1
            else:
                if p.startswith("v_") and " " in p and _vgprs(p.split(None, 1)[1].split(",")[0].strip()) & src0:
                    bad.append((k, p, i))
                states += 1
            j -= 1
    return bad


def _headline(kernels):
    names = [n for n in kernels if HEADLINE in n]
    assert len(names) == 1, names
    return names[0]


def test_headline_register_budget(code_object):
    k = _kernels(code_object[0])
    r = k[_headline(k)]
    assert r["vgpr_count"] <= 168, r          # three wavefronts per SIMD
    assert r["vgpr_spill_count"] <= 5, r


def test_force_phase_uses_dpp_broadcast(code_object):
    funcs = _functions(code_object[1])
    name = _headline(_kernels(code_object[0]))
    assert any(i.startswith("v_fmac_f64_dpp") and "row_newbcast" in i for i in funcs[name])
    waves = [n for n in funcs if "mtp_wave_kernel" in n]
    assert waves and all(any(i.startswith("v_fmac_f64_dpp") for i in funcs[n]) for n in waves)


def test_dpp_operands_need_no_wait_states(code_object):
    funcs = _functions(code_object[1])
    for n, ins in funcs.items():
        if "mtp_wave_kernel" in n:
            assert not _dpp_hazards(ins), (n, _dpp_hazards(ins)[:3])
