// Device helpers shared by the wavefront-per-atom and the workgroup-per-atom kernels (internal).
#pragma once

#include <hip/hip_runtime.h>

#include "mtp_device.hpp"

#define MTP_NEIGHMASK 0x1FFFFFFF   // LAMMPS NEIGHMASK (pair_mtp.cpp:114)

// Diagnostic build only (make stamps): per-phase s_memtime sums per launch into p.stamps[16].
// The shipped library is built without MTP_STAMPS and executes no stamp.
// The traced wavefronts (st_trace != nullptr: mtp_device.hpp, MTP_TRACE_*) also leave every clock itself, per atom.
#ifdef MTP_STAMPS
#define STAMP(k)                                                         \
  do {                                                                   \
    const unsigned long long _t = __builtin_amdgcn_s_memtime();          \
    __builtin_amdgcn_s_waitcnt(0xC07F);                                  \
    st_acc[k] += _t - st_prev;                                           \
    st_prev = _t;                                                        \
    if (st_trace && st_atom < MTP_TRACE_ATOMS && lane == 0)              \
      st_trace[MTP_TRACE_HDR + 10 * st_atom + (k)] = _t;                 \
  } while (0)
#else
#define STAMP(k) ((void) 0)
#endif


static __device__ __forceinline__ void wave_fence()
{
  // LDS operations of one wavefront execute in program order; this only stops the
  // compiler from moving LDS accesses across a phase boundary.
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// r = sqrt(r2) and inv = 1 / r from ONE v_rsq_f64 (r2 > 0, normal range: squared interatomic distances): two
// Newton steps on y ~ r2^-1/2 (relative error 2^-26 -> 2^-52 -> rounding), then r = r2 y with one correction step.
// Both results are within 1 ulp of the correctly rounded values the reference's std::sqrt and division give
// (pair_mtp.cpp:128-129) -- 1e-16 relative, seven orders inside the parity tolerance -- at 11 instead of 24 VALU
// instructions (sqrt expansion + division expansion).
static __device__ __forceinline__ void sqrt_and_inverse(double r2, double &r, double &inv)
{
  double y = __builtin_amdgcn_rsq(r2);
  const double h = 0.5 * r2;
  y = y * fma(-h * y, y, 1.5);
  y = y * fma(-h * y, y, 1.5);
  double s = r2 * y;
  s = fma(fma(-s, s, r2), 0.5 * y, s);
  r = s;
  inv = y;
}

static __device__ __forceinline__ double shfl_xor_f64(double v, int mask) { return __shfl_xor(v, mask, 64); }

// a * b for per-lane operands below 2^23 (table rows, slots, byte offsets inside one LDS image): v_mul_i32_i24 /
// v_mad_i32_i24 issue at full rate, the 32- and 64-bit integer multiplies (v_mul_lo_u32, v_mad_u64_u32) at a quarter
static __device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }
// &base[3 j] for an [n][3] double array: 24 j as shift-adds in 32 bits (j < 2^27 atoms), added as an unsigned offset
static __device__ __forceinline__ const double *row3(const double *base, int j)
{
  unsigned j2 = (unsigned) j << 1;
  asm volatile("" : "+v"(j2));   // (keeps the optimiser from folding the shift-adds back into a quarter-rate v_mul_lo_u32)
  const unsigned j3 = j2 + (unsigned) j;
  return reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + (size_t) (j3 << 3));
}

// Requests every 64-byte line of a kernel's argument block at once.  The block is written by the host for each launch, so
// its lines miss every cache the first time a wavefront of a CU reads them; the kernel body reads its fields where it
// needs them, which made those misses SERIAL (a dozen lines, one memory round trip each: measured as +9 us per launch
// with the block in host memory against device memory).  After this the body's reads hit the scalar cache.
template <int BYTES, class PTR> static __device__ __forceinline__ void kernarg_touch(PTR ka)
{
  static_assert(BYTES <= 16 * 64, "kernarg_touch: up to sixteen lines");
  unsigned t;   // (ONE statement: no load may still be in flight when the compiler gets the register back)
  constexpr int LAST = BYTES - 4;   // lines past the end of the block re-read its last word
#define MTP_KA_OFF(k) "i"((k) * 64 < LAST ? (k) * 64 : LAST)
  asm volatile("s_load_dword %0, %1, %2\n\ts_load_dword %0, %1, %3\n\ts_load_dword %0, %1, %4\n\ts_load_dword %0, %1, %5\n\t"
               "s_load_dword %0, %1, %6\n\ts_load_dword %0, %1, %7\n\ts_load_dword %0, %1, %8\n\ts_load_dword %0, %1, %9\n\t"
               "s_load_dword %0, %1, %10\n\ts_load_dword %0, %1, %11\n\ts_load_dword %0, %1, %12\n\ts_load_dword %0, %1, %13\n\t"
               "s_load_dword %0, %1, %14\n\ts_load_dword %0, %1, %15\n\ts_load_dword %0, %1, %16\n\ts_load_dword %0, %1, %17\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&s"(t)
               : "s"(ka), MTP_KA_OFF(0), MTP_KA_OFF(1), MTP_KA_OFF(2), MTP_KA_OFF(3), MTP_KA_OFF(4), MTP_KA_OFF(5), MTP_KA_OFF(6),
                 MTP_KA_OFF(7), MTP_KA_OFF(8), MTP_KA_OFF(9), MTP_KA_OFF(10), MTP_KA_OFF(11), MTP_KA_OFF(12), MTP_KA_OFF(13),
                 MTP_KA_OFF(14), MTP_KA_OFF(15)
               : "memory");
#undef MTP_KA_OFF
}

static __device__ __forceinline__ double uniform_f64(double v)   // v is wave-uniform: move it to SGPRs
{
  const long long b = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned) b);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned) (b >> 32));
  return __longlong_as_double((long long) (((unsigned long long) hi << 32) | lo));
}

// Cross-lane moves inside a row of 16 lanes on the VALU (DPP), no LDS traffic: the partner of lane l is
// l^1, l^2 (quad permutes), l^7 (row_half_mirror) or l^15 (row_mirror).  Any of them flips exactly the
// lane bit a butterfly step splits on (bit 0, 1, 2, 3), which is all the reductions below need.
template <int CTRL> static __device__ __forceinline__ double dpp_f64(double v)
{
  const long long b = __double_as_longlong(v);
  int lo = (int) b, hi = (int) (b >> 32);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __longlong_as_double((long long) (((unsigned long long) (unsigned) hi << 32) | (unsigned) lo));
}
// acc += (c of lane N of this lane's row of 16) * m[i] for i < NT, the c lane of term i being N = i: one
// v_fmac_f64_dpp row_newbcast per term (the DPP64 control gfx950 has), the same FMA as a v_fmac_f64 on a value
// broadcast from LDS -- one per-lane ds_read_b64 of 16 coefficients instead of 16 broadcast reads.
// Preconditions:
//   - full EXEC: a masked-off source lane still feeds its whole row;
//   - c is a VGPR pair that no VALU instruction wrote in the two instructions ahead of the statement (VALU write ->
//     DPP read: 2 wait states, which hipcc does not insert ahead of an asm statement).  The callers pass a value fresh
//     from an LDS load, which needs none; anything else needs an s_nop 1 in front (tests/test_isa_cpu.py checks the ISA);
//   - m[i] are VGPR pairs.
// All NT terms go into ONE statement: hipcc pads every instruction that reads the output of an asm statement with one
// wait state (s_nop 0), so one statement per term would cost an s_nop per FMA; this way it is one per chunk.
#define MTP_FMAC_DPP(i, op) "v_fmac_f64_dpp %0, %1, %" #op " row_newbcast:" #i " row_mask:0xf bank_mask:0xf\n\t"
#define MTP_FD1 MTP_FMAC_DPP(0, 2)
#define MTP_FD2 MTP_FD1 MTP_FMAC_DPP(1, 3)
#define MTP_FD3 MTP_FD2 MTP_FMAC_DPP(2, 4)
#define MTP_FD4 MTP_FD3 MTP_FMAC_DPP(3, 5)
#define MTP_FD5 MTP_FD4 MTP_FMAC_DPP(4, 6)
#define MTP_FD6 MTP_FD5 MTP_FMAC_DPP(5, 7)
#define MTP_FD7 MTP_FD6 MTP_FMAC_DPP(6, 8)
#define MTP_FD8 MTP_FD7 MTP_FMAC_DPP(7, 9)
#define MTP_FD9 MTP_FD8 MTP_FMAC_DPP(8, 10)
#define MTP_FD10 MTP_FD9 MTP_FMAC_DPP(9, 11)
#define MTP_FD11 MTP_FD10 MTP_FMAC_DPP(10, 12)
#define MTP_FD12 MTP_FD11 MTP_FMAC_DPP(11, 13)
#define MTP_FD13 MTP_FD12 MTP_FMAC_DPP(12, 14)
#define MTP_FD14 MTP_FD13 MTP_FMAC_DPP(13, 15)
#define MTP_FD15 MTP_FD14 MTP_FMAC_DPP(14, 16)
#define MTP_FD16 MTP_FD15 MTP_FMAC_DPP(15, 17)
#define MTP_FO1 "v"(m[0])
#define MTP_FO2 MTP_FO1, "v"(m[1])
#define MTP_FO3 MTP_FO2, "v"(m[2])
#define MTP_FO4 MTP_FO3, "v"(m[3])
#define MTP_FO5 MTP_FO4, "v"(m[4])
#define MTP_FO6 MTP_FO5, "v"(m[5])
#define MTP_FO7 MTP_FO6, "v"(m[6])
#define MTP_FO8 MTP_FO7, "v"(m[7])
#define MTP_FO9 MTP_FO8, "v"(m[8])
#define MTP_FO10 MTP_FO9, "v"(m[9])
#define MTP_FO11 MTP_FO10, "v"(m[10])
#define MTP_FO12 MTP_FO11, "v"(m[11])
#define MTP_FO13 MTP_FO12, "v"(m[12])
#define MTP_FO14 MTP_FO13, "v"(m[13])
#define MTP_FO15 MTP_FO14, "v"(m[14])
#define MTP_FO16 MTP_FO15, "v"(m[15])
template <int NT> static __device__ __forceinline__ void fmac_row_bcast(double &acc, double c, const double *m)
{
  static_assert(NT >= 1 && NT <= 16, "one row of 16 lanes");
#define MTP_FD_CASE(n) \
  if constexpr (NT == n) asm("" MTP_FD##n : "+v"(acc) : "v"(c), MTP_FO##n);
  MTP_FD_CASE(1) MTP_FD_CASE(2) MTP_FD_CASE(3) MTP_FD_CASE(4) MTP_FD_CASE(5) MTP_FD_CASE(6) MTP_FD_CASE(7) MTP_FD_CASE(8)
  MTP_FD_CASE(9) MTP_FD_CASE(10) MTP_FD_CASE(11) MTP_FD_CASE(12) MTP_FD_CASE(13) MTP_FD_CASE(14) MTP_FD_CASE(15) MTP_FD_CASE(16)
#undef MTP_FD_CASE
}
// one term: acc += row_bcast<N>(c) * m (same preconditions)
template <int N> static __device__ __forceinline__ void fmac_row_bcast1(double &acc, double c, double m)
{
  static_assert(N >= 0 && N < 16, "lane of a row of 16");
  asm(MTP_FMAC_DPP(%c2, 3) : "+v"(acc) : "v"(c), "i"(N), "v"(m));
}
// c of lane N of this lane's row of 16 (v_mov_b32_dpp row_newbcast on both halves)
template <int N> static __device__ __forceinline__ double row_bcast(double c)
{
  return dpp_f64<0x150 + N>(c);
}

// value of the lane that differs in bit log2(H) (and possibly lower bits).  H = 16 / 32 use gfx950's row / half
// swaps (lane maps measured with scripts/probes/permlane_probe.hip): with both operands equal to v,
// v_permlane16_swap leaves rows {0,0,2,2} of v in the first register and rows {1,1,3,3} in the second.
template <int H> static __device__ __forceinline__ double partner_f64(double v, int lane = 0)
{
  if constexpr (H == 1) return dpp_f64<0xB1>(v);        // quad_perm [1,0,3,2]
  else if constexpr (H == 2) return dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  else if constexpr (H == 4) return dpp_f64<0x141>(v);  // row_half_mirror
  else if constexpr (H == 8) return dpp_f64<0x140>(v);  // row_mirror
  else {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned) b, hi = (unsigned) (b >> 32);
    if constexpr (H == 16) {
      const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
      const auto c = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
      const unsigned rl = (lane & 16) ? a[0] : a[1], rh = (lane & 16) ? c[0] : c[1];
      return __longlong_as_double((long long) (((unsigned long long) rh << 32) | rl));
    } else {
      static_assert(H == 32, "partner distance");
      const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
      const auto c = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
      const unsigned rl = (lane & 32) ? a[0] : a[1], rh = (lane & 32) ? c[0] : c[1];
      return __longlong_as_double((long long) (((unsigned long long) rh << 32) | rl));
    }
  }
}

// v + (value of lane l^16) and v + (value of lane l^32) with gfx950's row / half swaps: with both operands equal
// to v, v_permlane16_swap leaves {rows 0,0,2,2} in one register and {rows 1,1,3,3} in the other (measured
// lane maps: scripts/probes/permlane_probe.hip), so their sum is the pair sum in every lane, in the same
// operand order everywhere; v_permlane32_swap does the same for the wavefront halves.  No LDS traffic.
static __device__ __forceinline__ double pair_sum16(double v)
{
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned) b, hi = (unsigned) (b >> 32);
  const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto c = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __longlong_as_double((long long) (((unsigned long long) c[0] << 32) | a[0])) +
      __longlong_as_double((long long) (((unsigned long long) c[1] << 32) | a[1]));
}
static __device__ __forceinline__ double pair_sum32(double v)
{
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned) b, hi = (unsigned) (b >> 32);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto c = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __longlong_as_double((long long) (((unsigned long long) c[0] << 32) | a[0])) +
      __longlong_as_double((long long) (((unsigned long long) c[1] << 32) | a[1]));
}

// pair_sum32 of two values for one exchange: v_permlane32_swap of a against b leaves {a of half 0 | b of half 0} in one
// register and {a of half 1 | b of half 1} in the other, so their sum is the pair sum of a in the lanes of half 0 and
// the pair sum of b in those of half 1, each the half-0 term plus the half-1 term as pair_sum32 adds them.
static __device__ __forceinline__ double pair_sum32_t(double a, double b)
{
  const long long ba = __double_as_longlong(a), bb = __double_as_longlong(b);
  const auto l = __builtin_amdgcn_permlane32_swap((unsigned) ba, (unsigned) bb, false, false);
  const auto h = __builtin_amdgcn_permlane32_swap((unsigned) (ba >> 32), (unsigned) (bb >> 32), false, false);
  return __longlong_as_double((long long) (((unsigned long long) h[0] << 32) | l[0])) +
      __longlong_as_double((long long) (((unsigned long long) h[1] << 32) | l[1]));
}

static __device__ __forceinline__ double wave_sum(double v)   // same bits in every lane
{
  v += partner_f64<1>(v);
  v += partner_f64<2>(v);
  v += partner_f64<4>(v);
  v += partner_f64<8>(v);   // every lane: sum of its row of 16
  return pair_sum32(pair_sum16(v));
}

static __device__ __forceinline__ void lds_add(double *p, double v)
{
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// LDS read at (32-bit LDS byte address + compile-time byte offset): the offset lands in the
// ds_read immediate field, so inner loops spend no VALU on addressing.
typedef __attribute__((address_space(3))) const double lds_cdouble;
// (no generic -> LDS pointer casts: hipcc 7.2 miscompiles their null check on gfx950; LDS byte
// addresses are formed as the LDS address of the dynamic array + an offset instead)
// volatile: hipcc otherwise fuses neighbouring reads into ds_read2_b64, which moves 16 B per lane in
// 8 LDS cycles where two ds_read_b64 take 4 (MI355X_MICROARCH.md, LDS table)
static __device__ __forceinline__ double lds_ld(unsigned base, int off_doubles)   // off: constant after unrolling
{
  return *(volatile lds_cdouble *) (size_t) (base + 8u * (unsigned) off_doubles);
}

// Butterfly transpose-reduce over the lane bits below N: every lane enters with N partial
// sums v[0..N); on exit v[0] of lane l holds entry (l mod N) summed over the N lanes that
// differ from l only in those bits (steps within a row of 16 lanes run on DPP).  N-1 adds and N-1 exchanges instead of N*log2(N).
template <int N> struct Butterfly {
  static __device__ __forceinline__ void run(double *v, int lane)
  {
    constexpr int H = N / 2;
    const bool hi = (lane & H) != 0;
#pragma unroll
    for (int i = 0; i < H; i++) {
      const double keep = hi ? v[i + H] : v[i];
      const double send = hi ? v[i] : v[i + H];
      v[i] = keep + partner_f64<H>(send, lane);
    }
    Butterfly<H>::run(v, lane);
  }
};
template <> struct Butterfly<1> {
  static __device__ __forceinline__ void run(double *, int) {}
};

// The same for NINE entries v[0..8] over the lane bits below 16 (the force totals: 3 force and 6 virial components):
// entry 8 pairs with entry 0 in the first step; entries 1..7 have no partner entry there, so that step is a plain
// pair sum for them (3 instead of 7 instructions each).  On exit v[0] of lane l holds entry l for l & 15 in 0..8.
static __device__ __forceinline__ void butterfly9(double *v, int lane)
{
  const bool hi = (lane & 8) != 0;
  {
    const double keep = hi ? v[8] : v[0];
    const double send = hi ? v[0] : v[8];
    v[0] = keep + partner_f64<8>(send, lane);
  }
#pragma unroll
  for (int i = 1; i < 8; i++) v[i] += partner_f64<8>(v[i], lane);
  Butterfly<8>::run(v, lane);
}

struct BlockTables {   // views into the workgroup-shared head of LDS
  const MtpRow8 *rows;
  const int *level, *slot, *seed_idx, *map, *pack, *coef, *smu, *fwd, *seg_fwd, *seg_bwd;
  const double *radial, *seed_val, *lin, *leaf_cf, *leaf_cb;
};

