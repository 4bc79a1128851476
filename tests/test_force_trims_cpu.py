"""The transposed moment store of the fixed force shape (csrc/mtp_wave_body.hpp, sum_t_ct; statements in
csrc/mtp_wave_kernel_body.hpp), replayed on the host from the five-factor blocks as the kernel reads them.

Behind the tile loop accumulator e of a block is exchanged against accumulator e + 3 between the two halves of the
wavefront, so half q of the lane pair that owns a block ends with the totals of products 3 q + 0 .. 3 q + 2 and stores
those three.  The lane's three int16 basic indices are packed once per wavefront from the block's last three words
{y, z, w} into two registers: half 0 {y, z & 0xffff}, half 1 {z >> 16 | w << 16, w >> 16}; index e is the 16-bit half
e & 1 of register e >> 1, sign-extended, and a negative index stores nothing."""
import os
import re

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
CSRC = os.path.join(ROOT, "lammps_mtp_kokkos_amd", "csrc")
COMMITTED = ["W_L8.mtp", "W_L16.mtp", "W_L16_nbh.almtp", "WRe_L10_cfg.almtp", "WRe_L20.mtp"]


def _lane_indices(words, q):
    """the three basic indices half q of a block's lane pair stores, by the kernel's packing"""
    y, z, w = (int(v) & 0xffffffff for v in words[5:8])
    if q:
        kk = [((z >> 16) | (w << 16)) & 0xffffffff, w >> 16]
    else:
        kk = [y, z & 0xffff]
    out = []
    for e in range(3):
        h = (kk[e >> 1] >> (16 * (e & 1))) & 0xffff
        out.append(h - 0x10000 if h & 0x8000 else h)
    return out


@pytest.mark.parametrize("name", COMMITTED)
def test_both_halves_together_store_every_basic_once(name):
    pot = capi.Potential(os.path.join(POT, name))
    b5, _ = pot.moment_blocks(five=True)
    B = pot.sizes["B"]
    stored = []
    for words in b5:
        kk = [int(k) for k in np.ascontiguousarray(words[5:8]).view(np.int16)]
        for q in (0, 1):
            got = _lane_indices(words, q)
            assert got == kk[3 * q:3 * q + 3], (q, got, kk)   # product 3 q + e, the accumulator that half ends with
            stored += [k for k in got if k >= 0]              # (k < 0: no store)
    assert all(0 <= k < B for k in stored)
    assert sorted(stored) == list(range(B)), "every basic exactly once, and no other LDS slot"


def test_level16_uses_both_halves():
    """the fixed force shape: 28 blocks, 130 basics, and both halves have something to store in most blocks"""
    b5, _ = capi.Potential(os.path.join(POT, "W_L16.mtp")).moment_blocks(five=True)
    per_half = [[sum(k >= 0 for k in _lane_indices(words, q)) for words in b5] for q in (0, 1)]
    assert len(b5) == 28 and sum(per_half[0]) + sum(per_half[1]) == 130
    assert min(per_half[0]) >= 1 and sum(1 for n in per_half[1] if n) >= 20


def test_the_switches_default_to_on_and_name_the_force_shape_only():
    text = open(os.path.join(CSRC, "mtp_wave_body.hpp")).read()
    for name in ("MTP_SUM_T", "MTP_CNT_SGPR"):
        assert re.search(r"#ifndef %s\n#define %s 1 " % (name, name), text), name
    # both traits hang on force5_shape: a five-factor shape that is no grade call
    assert re.search(r"force5_shape\(\)\n\{\n  if constexpr \(fwd5_shape<SH>\(\)\) return !SH::kGRADE;", text)
    for trait in ("sum_t_ct", "cnt_sgpr_ct"):
        assert re.search(r"constexpr bool %s = MTP_\w+ && MTP_FWD5 && force5_shape<SH>\(\);" % trait, text), trait
