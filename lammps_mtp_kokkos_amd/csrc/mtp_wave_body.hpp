// Device helpers of the force kernel (included by mtp_kernels.hip and mtp_kernels_fixed.hip; internal).  The kernel's
// statements are in mtp_wave_kernel_body.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "mtp_device.hpp"

#include "mtp_kernel_common.hpp"
#include "mtp_shape_fields.hpp"

namespace {

// ---- compile-time switches of the force kernel -----------------------------------------------------------------------
// All of them, with their shipped values; `make variant EXTRA=-DMTP_...=` builds another.  mtp_kernel_build_flags()
// (mtp_kernels.hip) names every one that differs from the value here, in this order, then MTP_GRADE_TPB / MTP_GRADE_WPE
// of the grade GEMM, whose defaults stand beside that kernel; MTP_STAMPS (a diagnostic build, no value) is named by
// mtp_build_flags() itself.  tests/test_row_reads_cpu.py checks that no default here lacks its entry there.  The switches
// of decided comparisons are taken out of the sources with the arm that lost.
#ifndef MTP_PU
#define MTP_PU 2   // times rows in flight per lane in the row-per-lane product passes (4 until the leaf moments and the
                   // per-tile totals changed the balance: re-measured 1 / 2 / 3 / 4 / 5 / 6 rows: 0.473 / 0.473 / 0.477 / 0.482 /
                   // 0.486 / 0.496 ms at level 16)
#endif
#ifndef MTP_FWD5
#define MTP_FWD5 1   // 0: the 3 x 3 blocks in the fixed shapes too, for A/B runs (fwd5_ct)
#endif
#ifndef MTP_SUM_T
#define MTP_SUM_T 1   // 0: six pair_sum32 and six stores from half 0, for A/B runs (sum_t_ct)
#endif
#ifndef MTP_CNT_SGPR
#define MTP_CNT_SGPR 1   // 0: the count as the optimiser leaves it, for A/B runs (cnt_sgpr_ct)
#endif
#ifndef MTP_ROW_KEEP_L1
#define MTP_ROW_KEEP_L1 1   // 0: the first level reads all its rows per atom, for A/B runs (row_keep_l1_ct)
#endif
#ifndef MTP_PHASE_PRIO
#define MTP_PHASE_PRIO 1   // 0: every phase at the launch's priority, for A/B runs (phase_prio_ct)
#endif

// The parameter block is read through the kernarg segment pointer (address space 4: scalar loads from the constant
// cache that the compiler re-issues where a field is needed) instead of a by-value struct, which it kept in SGPRs
// across the whole atom loop and spilled into VGPR lanes (a quarter of the static VALU instructions were
// v_readlane / v_writelane, 255 VGPRs; now 229 and none).  Making the pointer opaque again at every phase boundary
// was measured 1 % slower.
typedef const __attribute__((address_space(4))) MtpDevParams *KP;

// One accessor for every field of the argument block that a shape may fix: SHF(field) / SHA(array, index) yield the
// shape's constant when SH fixes the field and kp->field otherwise (MTP_SHAPE_INT_FIELDS / MTP_SHAPE_ARR_FIELDS are
// also what the launcher's field-wise match and the generator of mtp_fixed_shapes.hpp are made from).
namespace shape_get {
#define MTP_X(f)                                                                  \
  template <class SH> __device__ __forceinline__ int f(KP kp)                     \
  {                                                                               \
    if constexpr (mtp_shape::has_##f<SH>::value) return SH::f;                    \
    else return kp->f;                                                            \
  }
MTP_SHAPE_INT_FIELDS(MTP_X)
MTP_SHAPE_EXT_FIELDS(MTP_X)
#undef MTP_X
#define MTP_X(f)                                                                  \
  template <class SH> __device__ __forceinline__ int f(KP kp, int k)              \
  {                                                                               \
    if constexpr (mtp_shape::has_##f<SH>::value) return SH::f(k);                 \
    else return kp->f[k];                                                         \
  }
MTP_SHAPE_ARR_FIELDS(MTP_X)
MTP_SHAPE_TAB_FIELDS(MTP_X)
#undef MTP_X
}   // namespace shape_get
#define SHF(f) (shape_get::f<SH>(kp))
#define SHA(f, k) (shape_get::f<SH>(kp, (k)))
#define SHT(f, k) (shape_get::f<SH>(kp, (k)))

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order
template <class F, int... I> __device__ __forceinline__ void static_for(F &&f, std::integer_sequence<int, I...>)
{
  (f(std::integral_constant<int, I>()), ...);
}

// The slot tables of a shape that fixes them (MtpDevParams::slot_row, slot_mu_lo / _hi).  Both are atom-invariant table
// structure, yet read from the LDS blob the tile build waits for three 16-byte reads of slot[] at the head of every
// radial function before a store address exists, tests every row index (an EXEC region each) and multiplies it by
// the pitch, and the kernel entry forms the slot -> mu word by two ballots.  slot_ct: the tile build takes the rows
// from the shape (build_tile) and SlotMu::bits is the shape's constant.  The generic kernels keep the reads
// (profiles/r09_ab_slot_tables.txt has the timing).
template <class SH>
constexpr bool slot_rows_ct = mtp_shape::has_slot_row<SH>::value && mtp_shape::has_Mu<SH>::value &&
    mtp_shape::has_P<SH>::value && mtp_shape::has_R<SH>::value;
template <class SH>
constexpr bool slot_mu_ct = mtp_shape::has_slot_mu_lo<SH>::value && mtp_shape::has_slot_mu_hi<SH>::value &&
    mtp_shape::has_nslot<SH>::value && mtp_shape::has_Mu<SH>::value;
template <class SH> constexpr unsigned long long slot_mu_bits()
{
  if constexpr (slot_mu_ct<SH>) return ((unsigned long long) (unsigned) SH::slot_mu_hi << 32) | (unsigned) SH::slot_mu_lo;
  else return 0ull;   // (never used: a shape without the map)
}
template <class SH> __device__ __forceinline__ int slot_mu_of(int s) { return (int) (slot_mu_bits<SH>() >> (2 * s)) & 3; }
// f' rows of the force phase from registers (nodg layouts): the radial derivatives never left the wavefront -- lane
// (n, h) parked f'_h and f'_{h+2} of neighbour n in the tile build, lane (n, 1 - h) the other two.  One exchange between
// the halves (v_permlane32_swap with both operands equal leaves the low half's value in one register and the high
// half's in the other, in every lane: pair_sum32) hands all four to both, and where the shape fixes the slot -> mu map
// and the slots of every rank, each slot visit takes the register of its mu: no f' rows are written (fp_from_parked),
// no fence, no read per slot visit.  Same bits as the stored and re-read value, same arithmetic after it (timed against
// the rows through LDS in the same log).
template <class SH> constexpr bool fp_regs_ct = slot_mu_ct<SH> && mtp_shape::has_deg_first<SH>::value;
#define MTP_FP_N 4   // f'_0 .. f'_3: Mu <= 4 in the nodg layouts
__device__ __forceinline__ void fp_exchange(const double (&park)[2], double (&F)[MTP_FP_N])
{
#pragma unroll
  for (int mi = 0; mi < 2; mi++) {
    const long long b = __double_as_longlong(park[mi]);
    const unsigned lo = (unsigned) b, hi = (unsigned) (b >> 32);
    const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto c = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    F[2 * mi] = __longlong_as_double((long long) (((unsigned long long) c[0] << 32) | a[0]));       // half 0 parked mu = 2 mi
    F[2 * mi + 1] = __longlong_as_double((long long) (((unsigned long long) c[1] << 32) | a[1]));   // half 1: mu = 2 mi + 1
  }
}
// F[mu]: a chain of selects, so that F stays in registers whatever mu is; it folds to one register where mu is a constant
__device__ __forceinline__ double fp_pick(const double (&F)[MTP_FP_N], int mu)
{
  return mu == 0 ? F[0] : mu == 1 ? F[1] : mu == 2 ? F[2] : F[3];
}
// Row offsets of the basic-moment blocks kept across the atom loop (3-per-SIMD force build, one block per lane).  The
// twelve LDS addresses of a lane's block are the wavefront's table base plus row x pitch, the rows decoded from three
// descriptor words of the blob: the same for every atom, yet formed per atom since the twelve finished addresses did
// not fit beside the rest of the loop.  Their row byte offsets (below 2^16: tab_rows x 8 PITCH) do, as 16-bit halves of
// six registers, and an address per atom is then one add of the base and a 16-bit word.  The descriptors are table
// contents and are still read from the blob, once per wavefront.  Not in the grade shape: that build has no register
// to spare.  (Against the decode per atom: profiles/r10_ab_force_regs.txt.)
template <class SH> constexpr bool block_regs_shape()
{
  if constexpr (mtp_shape::has_pow_row<SH>::value && mtp_shape::has_P<SH>::value && mtp_shape::has_tab_rows<SH>::value)
    return !SH::kGRADE && SH::kWPS == 3 && SH::kNB == 1 && SH::tab_rows * 8 * SH::kPITCH < 65536;
  else return false;
}
template <class SH> constexpr bool block_regs_ct = block_regs_shape<SH>();
// Basic-moment pass in five-factor blocks (mtp_potential.hpp, fwd5_blocks) in the fixed shapes of the 3-per-SIMD build
// that name the table (nfb5, off_fwd5) and keep a lane's block in registers (block_regs_ct: the force shape).  The 3 x 3 blocks of level 16 are half empty -- 130 basics in 26 blocks of
// nine, because the head x tail grids are thin at both ends (16 x 1 ... 1 x 7) --, and a column costs a lane twelve
// ds_read_b64.  Blocks of five factors and six products, cut 3 x 2 or 2 x 3 per grid, cover the same grids in 28: ten
// reads a column, six accumulators, six reductions and six stores per atom, the indices from registers.  The table is
// read from HBM / L2 once per wavefront: it is in no LDS prefix, so no launch plan changes.  The third factor's
// partners differ between the two cuts: two selects per column, their mask one SGPR pair formed once per wavefront
// (select_f64).  Every basic is the same sum over the same columns of (row x row) x (row x row), so the bits do not
// change.  The generic kernels and the grade shape (no register to spare for the block) keep the 3 x 3 pass.
template <class SH> constexpr bool fwd5_shape()
{
  if constexpr (mtp_shape::has_nfb5<SH>::value && mtp_shape::has_off_fwd5<SH>::value &&
                mtp_shape::has_pow_row<SH>::value && mtp_shape::has_P<SH>::value && mtp_shape::has_tab_rows<SH>::value)
    return SH::kWPS == 3 && SH::kNB == 1 && SH::nfb5 <= SH::kKL && SH::tab_rows * 8 * SH::kPITCH < 65536;
  else return false;
}
template <class SH> constexpr bool fwd5_ct = MTP_FWD5 && fwd5_shape<SH>();
// mask bit of the lane ? b : a, the lane mask in an SGPR pair (no VGPR holds the predicate)
__device__ __forceinline__ double select_f64(unsigned long long mask, double a, double b)
{
  const unsigned alo = (unsigned) __double2loint(a), ahi = (unsigned) __double2hiint(a);
  const unsigned blo = (unsigned) __double2loint(b), bhi = (unsigned) __double2hiint(b);
  unsigned lo, hi;
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(lo) : "v"(alo), "v"(blo), "s"(mask));
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(hi) : "v"(ahi), "v"(bhi), "s"(mask));
  return __hiloint2double((int) hi, (int) lo);
}
// Two trims of the five-factor force shape (fwd5_ct and no grade call); every output bit stays.
// sum_t_ct: the six accumulators cross the two neighbour groups in pairs (pair_sum32_t, mtp_kernel_common.hpp): half 0
// ends with the totals of products 0..2, half 1 with those of 3..5, and every lane of a block stores three moments --
// three exchanges, adds and stores per atom instead of six.  The lane's three int16 indices (products 3 q + 0..2) are
// packed into kk5[0..1] once per wavefront.
template <class SH> constexpr bool force5_shape()
{
  if constexpr (fwd5_shape<SH>()) return !SH::kGRADE;
  else return false;
}
template <class SH> constexpr bool sum_t_ct = MTP_SUM_T && MTP_FWD5 && force5_shape<SH>();
// cnt_sgpr_ct: the neighbour count goes back into an SGPR behind the compaction.  The optimiser merges the branch that
// clamps it to cj_cap with the lane test of the error flag inside and leaves the count in a VGPR, and every test behind
// it -- the tile count, the padded tile width, the sixteen column tests of the basic-moment pass in both copies of the
// tile loop -- is then a vector compare with an EXEC region around the column.  From an SGPR they are scalar compares
// and branches.
template <class SH> constexpr bool cnt_sgpr_ct = MTP_CNT_SGPR && MTP_FWD5 && force5_shape<SH>();

// Issue priority by phase (s_setprio), in the fixed FORCE shapes of the 3-per-SIMD build.  The phases of an atom want
// opposite things of the SIMD: tile tables, basic moments, coefficient blocks and forces are VALU bursts; the loop head,
// the compaction and both product passes with the leaf sweep and the energy issue a few instructions between dependent
// memory or LDS round trips.  At equal priority the issue arbiter favours the oldest wavefront of a SIMD, so a chain's
// next instruction queues behind another wavefront's burst and the younger wavefronts fall behind by whole atoms (the
// per-wavefront phase trace: scripts/wave_phase_trace.py, profiles/r13_ab_wave_phases.txt).  Raised in the chains and
// lowered in the bursts: four s_setprio per atom, -5.7 % per step on the headline launch.  The generic kernels and the
// grade shape compile as they did.  (A start offset per SIMD slot, MTP_WAVE_STAGGER, was measured beside it, lost, and
// is not in the sources: the same record.)
template <class SH, class = void> struct has_kernel_args : std::false_type {};
template <class SH> struct has_kernel_args<SH, std::void_t<decltype(&SH::kGRADE), decltype(&SH::kWPS)>> : std::true_type {};
template <class SH> constexpr bool phase_prio_shape()
{
  if constexpr (has_kernel_args<SH>::value) return !SH::kGRADE && SH::kWPS == 3;   // (ShapeGeneric names no kernel)
  else return false;
}
template <class SH> constexpr bool phase_prio_ct = MTP_PHASE_PRIO && phase_prio_shape<SH>();
#define MTP_PRIO_CHAIN 2
#define MTP_PRIO_BURST 0
template <bool ON, int PRIO> __device__ __forceinline__ void phase_prio()
{
  if constexpr (ON) __builtin_amdgcn_s_setprio(PRIO);
}

// f[idx] += v.  Default: native fp64 HBM atomics (the sum depends on the arrival order in the last bits).
// Deterministic mode (mtp_context_set_deterministic, tests / reproducible goldens): the contributions are added as
// 64-bit fixed-point integers (2^-40 eV/A resolution, |f| < 2^23), which commute exactly, and converted once at the end.
#define MTP_FIXED_SCALE 1099511627776.0   // 2^40
static __device__ __forceinline__ void force_add(KP kp, size_t idx, double v)
{
  if (kp->fq) atomicAdd(reinterpret_cast<unsigned long long *>(kp->fq) + idx, (unsigned long long) __double2ll_rn(v * MTP_FIXED_SCALE));
  else unsafeAtomicAdd(&kp->f[idx], v);
}

template <int PITCH> struct WaveLds {
  static constexpr int NT = 32;   // neighbours per tile; the row pitch (33 doubles: odd, so the 32 lanes of a half-wavefront
                                  // reading 32 different rows of one column hit 32 different 8-byte banks) is the template parameter
  double *M, *D, *coef, *tab, *nbx, *nby, *nbz, *nbr, *nbi;
  int *nbj, *nbjt, *cj;
  unsigned m_addr;   // LDS byte address of M
  __device__ __forceinline__ unsigned addr(const double *ptr) const { return m_addr + 8u * (unsigned) (ptr - M); }
  template <class SH> __device__ __forceinline__ WaveLds(double *base, unsigned base_addr, KP kp, SH)
  {
    // Layouts of the per-atom image, chosen by the host planner (mtp_context.hip, plan()); all of them are
    // [tables | overlay | neighbour arrays] with the regions placed through offsets in the parameter block
    // (dg_mode: bit 0 = no dg rows, bit 1 = rebuild):
    //   keep     [g rows | dg rows | overlay]: the coordinate-power rows live in the overlay from the tile build to the
    //            end of the basic-moment pass, the moments / adjoints (later the derivative-polynomial coefficients)
    //            from there on -- the two are never live together;
    //   nodg     [g rows | overlay] (Mu <= 4): no dg rows.  d/dr (f_mu / r^nu) = f'_mu / r^nu - nu g / r, so
    //            sum_s (dg_s / nu) G_s = sum_s f'_mu(s) (r^-nu / nu) G_s - (1/r) sum_s g_s G_s: the tile build parks the
    //            radial derivatives f'_mu(r) of its neighbour in registers, Mu rows of them (instead of one dg row per
    //            slot) are written behind the coefficient blocks ahead of the force phase, which multiplies them in
    //            per slot and subtracts the g sums it forms anyway;
    //   rebuild  everything overlays everything (potentials with many moments): the moments and adjoints sit on the
    //            g rows, which are built a second time (with the dg rows unless nodg) ahead of the force phase (the
    //            coefficient blocks sit behind the rows, the adjoints of the basics D[0, B) in front: the host checks
    //            that they cannot meet).
    tab = base;
    M = tab + SHF(w_m);
    D = tab + SHF(w_d);
    coef = tab + SHF(w_coef);
    nbx = tab + SHF(w_nb);
    m_addr = base_addr + 8u * (unsigned) (M - tab);
    nby = nbx + NT;
    nbz = nby + NT;
    nbr = nbz + NT;
    nbi = nbr + NT;
    nbj = reinterpret_cast<int *>(nbi + NT);
    nbjt = nbj + NT;
    cj = nbjt + NT;
  }
};

// Phase 2: tables of one tile; columns [0, ntp) are written, ntp = nt rounded up to the
// neighbour-group count with dummy neighbours sitting exactly on the cutoff (g = dg = 0).
// with_dg: write the dg rows; do_park (nodg layouts): park[] receives f'_mu(r) of this lane's neighbour for its radial
// functions mu = h, h + 2 (park[0..1]), from which fp_from_parked() writes the f' rows ahead of the force phase.
#define MTP_PARK 2   // radial functions per half-wavefront that can be parked: Mu <= 4
// rows between the g rows of radial functions 2 mi and 2 mi + 1 at the first nu where both have one (0: nowhere)
template <class SH, int MI> constexpr int slot_delta()
{
  if (2 * MI + 1 < SH::Mu)
    for (int nu = 0; nu < SH::P; nu++) {
      const int r0 = SH::slot_row(2 * MI * MTP_PSTRIDE + nu), r1 = SH::slot_row((2 * MI + 1) * MTP_PSTRIDE + nu);
      if (r0 >= 0 && r1 >= 0) return r1 - r0;
    }
  return 0;
}
// the lane's index into the gathered ids: lane, spelled lane & 31 under row_keep_l1_ct (defined with it below)
template <class SH> __device__ __forceinline__ int gather_lane(int lane);
template <int PITCH, class SH>
__device__ __forceinline__ void build_tile(KP kp, const BlockTables &bt, const WaveLds<PITCH> &w,
                                           int t0, int cnt, int ntp, bool gather, bool powers, bool with_dg, bool do_park,
                                           double (&park)[MTP_PARK],
                                           double xi0, double xi1, double xi2, int i, int itype, int lane)
{
  if (gather) {
    if (lane < ntp) {
      const bool real = t0 + lane < cnt;
      const int j = real ? w.cj[t0 + gather_lane<SH>(lane)] : i;
      double dx = 0, dy = 0, dz = 0, r = kp->rmax, inv = kp->inv_rmax;
      if (real) {
        const double *xj = row3(kp->x, j);
        dx = xj[0] - xi0;
        dy = xj[1] - xi1;
        dz = xj[2] - xi2;
        sqrt_and_inverse(dx * dx + dy * dy + dz * dz, r, inv);
      }
      w.nbx[lane] = dx;
      w.nby[lane] = dy;
      w.nbz[lane] = dz;
      w.nbr[lane] = r;
      w.nbi[lane] = inv;
      w.nbj[lane] = j;
      w.nbjt[lane] = real ? kp->type[j] - 1 : itype;
    }
    wave_fence();
  }
  // lanes = (neighbour n, half h): one pass over the tile.  The Chebyshev values q_k(r) and derivatives are
  // shared by all radial functions of the neighbour; half h contracts them for mu = h, h+2, ... and writes
  // the g / dg rows of those mu; the coordinate-power rows are split x,y | z between the halves.
  const int Mu = SHF(Mu), P = SHF(P), R = SHF(R);
  const double mult = 2.0 * kp->inv_span;
  const int n = lane & 31, h = lane >> 5;
  if (n < ntp) {
    const double r = w.nbr[n], inv = w.nbi[n];
    const int jt = w.nbjt[n];
    const double d = r - kp->rmax;
    const double ksi = (2.0 * r - (kp->rmin + kp->rmax)) * kp->inv_span;
    double *col = w.tab + n;
    // radial functions of this half: mu = h, h + 2, ...; the first MTP_PARK of them with static indices, so that the
    // parked derivatives stay in registers (a loop-carried index would put the array into scratch memory)
    auto each_mu = [&](auto &&body) {
      double d0 = 0.0, d1 = 0.0;
      if (h < Mu) d0 = body(h);
      if (h + 2 < Mu) d1 = body(h + 2);
      for (int mu = h + 2 * MTP_PARK; mu < Mu; mu += 2) (void) body(mu);
      if (do_park) {
        park[0] = d0;
        park[1] = d1;
      }
    };
    if (R == 8) {   // the MLIP default: basis in registers, coefficients in bursts of 16-byte reads
      double qv[8], ev[8];
      qv[0] = kp->scaling * (d * d);
      qv[1] = kp->scaling * (ksi * d * d);
      ev[0] = kp->scaling * 2.0 * d;
      ev[1] = kp->scaling * (mult * d * d + 2.0 * ksi * d);
#pragma unroll
      for (int ri = 2; ri < 8; ri++) {   // mtp_rb_chevbyshev_basis.cpp:29-54
        qv[ri] = 2.0 * ksi * qv[ri - 1] - qv[ri - 2];
        ev[ri] = 2.0 * (mult * qv[ri - 1] + ksi * ev[ri - 1]) - ev[ri - 2];
      }
      if constexpr (slot_rows_ct<SH>) {
        // rows from the shape: radial functions 2 mi (half 0) and 2 mi + 1 (half 1) of step mi.  Where both have a row
        // for nu and the two rows lie DELTA apart like the first such pair, the address is this half's column base
        // (col, + DELTA rows in half 1) plus an immediate; other pairs take one select between two constants; a row
        // of one half only is stored by that half; (mu, nu) without a row emit nothing.
        static_assert(SH::Mu <= 2 * MTP_PARK && SH::Mu <= MTP_SLOT_ROWS_MU && SH::P <= MTP_PSTRIDE && SH::R == 8, "slot_row: the nodg tables");
        double dpark[MTP_PARK] = {0.0, 0.0};
        static_for([&](auto MI) {
          constexpr int mi = decltype(MI)::value, mu0 = 2 * mi, mu1 = 2 * mi + 1;
          if constexpr (mu0 < SH::Mu) {
            constexpr bool two = mu1 < SH::Mu;
            const int mu = two ? mu0 + h : mu0;
            if (two || h == 0) {
              const double2 *c2 = reinterpret_cast<const double2 *>(bt.radial + (mul24(itype * SHF(Sp) + jt, Mu) + mu) * 8);
              const double2 c01 = c2[0], c23 = c2[1], c45 = c2[2], c67 = c2[3];
              const double cc[8] = {c01.x, c01.y, c23.x, c23.y, c45.x, c45.y, c67.x, c67.y};
              double val = cc[0] * qv[0], der = cc[0] * ev[0];
#pragma unroll
              for (int ri = 1; ri < 8; ri++) {
                val = fma(cc[ri], qv[ri], val);
                der = fma(cc[ri], ev[ri], der);
              }
              constexpr int delta = slot_delta<SH, mi>();
              double *colh = col + (h ? delta * PITCH : 0);
              double rp = 1.0;
              static_for([&](auto NU) {
                constexpr int nu = decltype(NU)::value;
                constexpr int r0 = SH::slot_row(mu0 * MTP_PSTRIDE + nu), r1 = two ? SH::slot_row(mu1 * MTP_PSTRIDE + nu) : -1;
                const double g = val * rp;
                auto put = [&](double *gp) {
                  *gp = g;                                                       // f_mu / r^nu
                  if (with_dg) gp[SHF(dg_off)] = der * rp - nu * g * inv;         // d/dr (f_mu / r^nu)
                };
                if constexpr (r0 >= 0 && r1 >= 0) {
                  if constexpr (r1 - r0 == delta) put(colh + r0 * PITCH);
                  else put(col + (h ? r1 * PITCH : r0 * PITCH));
                } else if constexpr (r0 >= 0) {
                  if (h == 0) put(col + r0 * PITCH);
                } else if constexpr (r1 >= 0) {
                  if (h == 1) put(col + r1 * PITCH);
                }
                rp *= inv;
              }, std::make_integer_sequence<int, SH::P>());
              dpark[mi] = der;
            }
          }
        }, std::make_integer_sequence<int, MTP_PARK>());
        if (do_park) {
          park[0] = dpark[0];
          park[1] = dpark[1];
        }
      } else
      each_mu([&](int mu) {
        const int4 *sl4 = reinterpret_cast<const int4 *>(bt.slot + mu * MTP_PSTRIDE);
        const int4 sa = sl4[0], sb = sl4[1], sc = sl4[2];
        const int sv[MTP_PSTRIDE] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w, sc.x, sc.y, sc.z, sc.w};
        const double2 *c2 = reinterpret_cast<const double2 *>(bt.radial + (mul24(itype * SHF(Sp) + jt, Mu) + mu) * 8);
        const double2 c01 = c2[0], c23 = c2[1], c45 = c2[2], c67 = c2[3];
        const double cc[8] = {c01.x, c01.y, c23.x, c23.y, c45.x, c45.y, c67.x, c67.y};
        double val = cc[0] * qv[0], der = cc[0] * ev[0];
#pragma unroll
        for (int ri = 1; ri < 8; ri++) {
          val = fma(cc[ri], qv[ri], val);
          der = fma(cc[ri], ev[ri], der);
        }
        double rp = 1.0;
#pragma unroll
        for (int nu = 0; nu < MTP_PSTRIDE; nu++) {
          if (nu < P) {
            const int sidx = sv[nu];
            const double g = val * rp;
            if (sidx >= 0) {
              double *gp = col + mul24(sidx, PITCH);
              *gp = g;                                                       // f_mu / r^nu
              if (with_dg) gp[SHF(dg_off)] = der * rp - nu * g * inv;         // d/dr (f_mu / r^nu)
            }
            rp *= inv;
          }
        }
        return der;
      });
    } else {
      each_mu([&](int mu) {
        const int *sl = bt.slot + mu * MTP_PSTRIDE;
        const double *c = bt.radial + mul24(mul24(itype * SHF(Sp) + jt, Mu) + mu, R);
        double q0 = kp->scaling * (d * d), q1 = kp->scaling * (ksi * d * d);
        double e0 = kp->scaling * 2.0 * d, e1 = kp->scaling * (mult * d * d + 2.0 * ksi * d);
        double val = c[0] * q0, der = c[0] * e0;
        if (R > 1) {
          val += c[1] * q1;
          der += c[1] * e1;
        }
        for (int ri = 2; ri < R; ri++) {
          const double q2 = 2.0 * ksi * q1 - q0;
          const double e2 = 2.0 * (mult * q1 + ksi * e1) - e0;
          val += c[ri] * q2;
          der += c[ri] * e2;
          q0 = q1;
          q1 = q2;
          e0 = e1;
          e1 = e2;
        }
        double rp = 1.0;
        for (int nu = 0; nu < P; nu++) {
          const int sidx = sl[nu];
          const double g = val * rp;
          if (sidx >= 0) {
            double *gp = col + mul24(sidx, PITCH);
            *gp = g;
            if (with_dg) gp[SHF(dg_off)] = der * rp - nu * g * inv;
          }
          rp *= inv;
        }
        return der;
      });
    }
    if (powers) {   // rows of one axis: [q] = u^q
      const double u0 = h == 0 ? w.nbx[n] : w.nbz[n];
      double *pc = col + mul24(SHF(pow_row) + (h == 0 ? 0 : 2 * P), PITCH);
      double cur = 1.0;
      pc[0] = 1.0;
      for (int q = 1; q < P; q++) {
        cur *= u0;
        pc[q * PITCH] = cur;
      }
      if (h == 0) {
        const double u1 = w.nby[n];
        pc += mul24(P, PITCH);
        cur = 1.0;
        pc[0] = 1.0;
        for (int q = 1; q < P; q++) {
          cur *= u1;
          pc[q * PITCH] = cur;
        }
      }
    }
  }
  wave_fence();
}

// nodg layouts, ahead of the force phase: the Mu rows f'_mu(r_n) of the tile from the derivatives the tile build parked
// in registers (row fp_row + mu; two stores per lane instead of one dg row per slot)
template <int PITCH, class SH>
__device__ __forceinline__ void fp_from_parked(KP kp, const WaveLds<PITCH> &w, int ntp, const double (&park)[MTP_PARK], int lane)
{
  const int n = lane & 31, h = lane >> 5, Mu = SHF(Mu);
  if (n < ntp) {
    double *col = w.tab + n + (size_t) SHF(fp_row) * PITCH;
#pragma unroll
    for (int mi = 0; mi < MTP_PARK; mi++) {
      const int mu = 2 * mi + h;
      if (mu < Mu) col[mul24(mu, PITCH)] = park[mi];
    }
  }
  wave_fence();
}

// Packed rows carry BYTE offsets (8 x moment index) in their 16-bit fields, so that an LDS address is one
// v_add_u32_sdwa (base + 16-bit word of the row) instead of a bit-field extract and a shift-add.
static __device__ __forceinline__ double &at8(double *base, unsigned byte_off)
{
  return *reinterpret_cast<double *>(reinterpret_cast<char *>(base) + byte_off);
}
static __device__ __forceinline__ const double &at8(const double *base, unsigned byte_off)
{
  return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + byte_off);
}

// Row bounds of the product levels.  The level table is atom-invariant and wave-uniform, yet read from the LDS blob
// every level start waits for an LDS round trip (and a lane read) before its first row address exists: seven such
// starts per atom at level 16 (three levels forward, the leaf block, three levels in reverse).  MtpDevParams::level_rows
// is the same table in the argument block, a shape field like the others: a fixed shape that lists it (and nlevels)
// has the bounds, and with them the block count of every level, as constants (level_ct).  The generic kernels keep the
// LDS reads: a scalar load of the field per bound costs their headline function ten more s_load than the round-6 guard
// allows (tests/test_isa_params_cpu.py; profiles/r08_ab_table_reads.txt has the timing).
template <class SH> constexpr bool level_ct = mtp_shape::has_nlevels<SH>::value && mtp_shape::has_level_rows<SH>::value;
template <class SH> __device__ __forceinline__ int level_row(const int *level, int l)   // l wave-uniform
{
  if constexpr (level_ct<SH>) return SH::level_rows(l);
  else return __builtin_amdgcn_readfirstlane(level[l]);
}

// Phase 4a: M[a3] += mult * M[a0] * M[a1], one dependency level at a time.  Rows of one level
// never write an operand of the same level, so four rows per lane are in flight before their
// ds_add_f64 issue.  (Two call sites, LDS-resident and HBM-resident rows: a select between the two
// pointers would go through a generic pointer, which hipcc 7.2 miscompiles on gfx950.)
// one level of nit blocks in trips of U (nit a constant where the shape fixes the level table: the loop unrolls and the idle
// slot of an odd count, whose clamped index re-reads the last block, folds into the slot before it)
template <int U> __device__ __forceinline__ void forward_level(const MtpRow8 *rp, int nit, double *M)
{
  for (int it = 0; it < nit; it += U) {
    MtpRow8 rw[U];
    double v[U];
#pragma unroll
    for (int u = 0; u < U; u++) rw[u] = rp[64 * min(it + u, nit - 1)];   // uniform clamp: the tail re-reads the last block
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = at8(M, rw[u].lo & 0xffffu) * at8(M, rw[u].lo >> 16);
#pragma unroll
    for (int u = 0; u < U; u++)
      if (it + u < nit) lds_add(&at8(M, rw[u].hi & 0xffffu), (double) ((int) rw[u].hi >> 16) * v[u]);   // uniform branch
  }
}
template <int U, class SH, int L> __device__ __forceinline__ void forward_levels_ct(const MtpRow8 *rows, double *M, int lane)
{
  if constexpr (L < SH::nlevels) {
    constexpr int beg = SH::level_rows(L), nit = (SH::level_rows(L + 1) - beg) >> 6;
    forward_level<U>(rows + beg + lane, nit, M);
    wave_fence();
    forward_levels_ct<U, SH, L + 1>(rows, M, lane);
  }
}
template <int U, class SH>
__device__ __forceinline__ void products_forward(KP kp, const MtpRow8 *rows, const int *level, double *M, int lane)
{
  if constexpr (level_ct<SH>) {
    static_assert(SH::nlevels + 2 <= MTP_SHAPE_ARR_LEN, "level_rows holds the whole level table or zeros");
    forward_levels_ct<U, SH, 0>(rows, M, lane);
  } else {
    for (int l = 0; l < SHF(nlevels); l++) {
      // levels are padded to whole 64-row blocks on the host (neutral rows): no bounds checks, no lane masks
      const int beg = level_row<SH>(level, l);
      forward_level<U>(rows + beg + lane, (level_row<SH>(level, l + 1) - beg) >> 6, M);
      wave_fence();
    }
  }
}

// Phase 4b: D[a1] += D[a3] mult M[a0]; D[a0] += D[a3] mult M[a1], levels in reverse.
template <int U> __device__ __forceinline__ void backward_level(const MtpRow8 *rp, int nit, const double *M, double *D)
{
  for (int it = 0; it < nit; it += U) {
    MtpRow8 rw[U];
    double d3[U], m0[U], m1[U];
#pragma unroll
    for (int u = 0; u < U; u++) rw[u] = rp[64 * min(it + u, nit - 1)];
#pragma unroll
    for (int u = 0; u < U; u++) {
      d3[u] = at8(D, rw[u].hi & 0xffffu) * (double) ((int) rw[u].hi >> 16);
      m0[u] = at8(M, rw[u].lo & 0xffffu);
      m1[u] = at8(M, rw[u].lo >> 16);
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      if (it + u < nit) {
        lds_add(&at8(D, rw[u].lo >> 16), d3[u] * m0[u]);
        lds_add(&at8(D, rw[u].lo & 0xffffu), d3[u] * m1[u]);
      }
  }
}
template <int U, class SH, int L>
__device__ __forceinline__ void backward_levels_ct(const MtpRow8 *rows, const double *M, double *D, int lane)
{
  if constexpr (L >= 0) {
    constexpr int beg = SH::level_rows(L), nit = (SH::level_rows(L + 1) - beg) >> 6;
    backward_level<U>(rows + beg + lane, nit, M, D);
    wave_fence();
    backward_levels_ct<U, SH, L - 1>(rows, M, D, lane);
  }
}
template <int U, class SH>
__device__ __forceinline__ void products_backward(KP kp, const MtpRow8 *rows, const int *level, const double *M, double *D,
                                                  int lane)
{
  if constexpr (level_ct<SH>) {
    backward_levels_ct<U, SH, SH::nlevels - 1>(rows, M, D, lane);
  } else {
    for (int l = SHF(nlevels) - 1; l >= 0; l--) {
      const int beg = level_row<SH>(level, l);
      backward_level<U>(rows + beg + lane, (level_row<SH>(level, l + 1) - beg) >> 6, M, D);
      wave_fence();
    }
  }
}

// Packed rows of the short levels kept across the atom loop.  A level of one or two blocks is one trip of its pass, and
// the trip starts with a row read that its operand reads wait for: latency the level cannot hide.  The rows are the
// same for every atom, so where the shape fixes the level table (level_ct: which levels are short is then a constant)
// and keeps the rows in the LDS blob, each lane loads the rows of those blocks once per wavefront, from the blob (rows
// are table contents, not shape), and both passes take them from registers: same rows, same lanes, same order
// (profiles/r10_ab_force_regs.txt).
constexpr int ROW_KEEP_LEVEL = 2;   // blocks of a level that is kept (one trip at MTP_PU = 2)
constexpr int ROW_KEEP_MAX = 3;     // blocks kept in all: two registers each
template <class SH> constexpr int level_blocks(int l) { return (SH::level_rows(l + 1) - SH::level_rows(l)) >> 6; }
template <class SH> constexpr bool level_kept(int l) { return level_blocks<SH>(l) >= 1 && level_blocks<SH>(l) <= ROW_KEEP_LEVEL; }
// blocks kept of the levels below l (l = nlevels: of all levels)
template <class SH> constexpr int kept_before(int l)
{
  int n = 0;
  for (int k = 0; k < l; k++)
    if (level_kept<SH>(k)) n += level_blocks<SH>(k);
  return n;
}
template <class SH> constexpr bool row_regs_shape()
{
  if constexpr (level_ct<SH> && mtp_shape::has_rows_in_lds<SH>::value)
    return !SH::kGRADE && SH::rows_in_lds == 1 && kept_before<SH>(SH::nlevels) >= 1 &&
        kept_before<SH>(SH::nlevels) <= ROW_KEEP_MAX;
  else return false;
}
template <class SH> constexpr bool row_regs_ct = row_regs_shape<SH>();
template <class SH> constexpr int kept_count()
{
  if constexpr (row_regs_ct<SH>) return kept_before<SH>(SH::nlevels);
  else return 1;   // (an array nobody reads)
}
template <class SH, int L, int NK> __device__ __forceinline__ void load_kept_rows(const MtpRow8 *rows, MtpRow8 (&kr)[NK], int lane)
{
  if constexpr (L < SH::nlevels) {
    if constexpr (level_kept<SH>(L)) {
#pragma unroll
      for (int b = 0; b < level_blocks<SH>(L); b++) kr[kept_before<SH>(L) + b] = rows[SH::level_rows(L) + 64 * b + lane];
    }
    load_kept_rows<SH, L + 1>(rows, kr, lane);
  }
}
// forward_level / backward_level of a kept level: block b of the level is kr[b]
template <int U, int NIT> __device__ __forceinline__ void forward_level_kept(const MtpRow8 *kr, double *M)
{
  static_assert(NIT <= U, "one trip");
  double v[NIT];
#pragma unroll
  for (int u = 0; u < NIT; u++) v[u] = at8(M, kr[u].lo & 0xffffu) * at8(M, kr[u].lo >> 16);
#pragma unroll
  for (int u = 0; u < NIT; u++) lds_add(&at8(M, kr[u].hi & 0xffffu), (double) ((int) kr[u].hi >> 16) * v[u]);
}
template <int U, int NIT> __device__ __forceinline__ void backward_level_kept(const MtpRow8 *kr, const double *M, double *D)
{
  static_assert(NIT <= U, "one trip");
  double d3[NIT], m0[NIT], m1[NIT];
#pragma unroll
  for (int u = 0; u < NIT; u++) {
    d3[u] = at8(D, kr[u].hi & 0xffffu) * (double) ((int) kr[u].hi >> 16);
    m0[u] = at8(M, kr[u].lo & 0xffffu);
    m1[u] = at8(M, kr[u].lo >> 16);
  }
#pragma unroll
  for (int u = 0; u < NIT; u++) {
    lds_add(&at8(D, kr[u].lo >> 16), d3[u] * m0[u]);
    lds_add(&at8(D, kr[u].lo & 0xffffu), d3[u] * m1[u]);
  }
}
// row_keep_l1_ct (round 16): the first ROW_KEEP_L1 blocks of the first level, a long one, join the kept rows -- its first
// two trips at MTP_PU = 2.  Each lane loads its row of them once per wavefront, from the blob, both passes take those
// trips from registers and run the level's other blocks as before, in the same order.  Two registers a block: with
// them the function stands at 168 VGPRs.
constexpr int ROW_KEEP_L1 = 4;
template <class SH> constexpr bool row_keep_l1_shape()
{
  if constexpr (row_regs_shape<SH>()) return level_blocks<SH>(0) >= ROW_KEEP_L1 && !level_kept<SH>(0);
  else return false;
}
template <class SH> constexpr bool row_keep_l1_ct = MTP_ROW_KEEP_L1 && row_regs_ct<SH> && row_keep_l1_shape<SH>();
template <class SH> constexpr int kept_l1_count() { return row_keep_l1_ct<SH> ? ROW_KEEP_L1 : 1; }   // (1: an array nobody reads)
template <class SH, int N1> __device__ __forceinline__ void load_kept_l1_rows(const MtpRow8 *rows, MtpRow8 (&k1)[N1], int lane)
{
#pragma unroll
  for (int b = 0; b < N1; b++) k1[b] = rows[SH::level_rows(0) + 64 * b + lane];
}
// At 168 VGPRs hipcc spilled one dword of that build: the LDS address of the gather's cj[] read (build_tile), base + 4
// lane, which it keeps across the atom loop for the atoms of more than one tile.  The gather runs in the lanes below
// ntp <= 32, where lane & 31 is lane; spelled so, the address can be formed from the lane & 31 registers that the
// force phase keeps anyway, and nothing spills.  The other kernels keep the plain spelling and with it their code.
template <class SH> __device__ __forceinline__ int gather_lane(int lane)
{
  if constexpr (row_keep_l1_ct<SH>) return lane & 31;
  else return lane;
}
// K1: the first ROW_KEEP_L1 blocks of level 0 are k1[] (whole trips: ROW_KEEP_L1 is a multiple of U)
template <int U, class SH, int L, bool K1, int NK, int N1>
__device__ __forceinline__ void forward_levels_kept(const MtpRow8 *rows, const MtpRow8 (&kr)[NK], const MtpRow8 (&k1)[N1], double *M,
                                                    int lane)
{
  if constexpr (L < SH::nlevels) {
    constexpr int beg = SH::level_rows(L), nit = level_blocks<SH>(L);
    if constexpr (level_kept<SH>(L)) {
      forward_level_kept<U, nit>(&kr[kept_before<SH>(L)], M);
    } else if constexpr (K1 && L == 0) {
      static_assert(N1 == ROW_KEEP_L1 && ROW_KEEP_L1 % U == 0 && nit >= ROW_KEEP_L1, "whole trips from registers");
#pragma unroll
      for (int b = 0; b < ROW_KEEP_L1; b += U) forward_level_kept<U, U>(&k1[b], M);
      forward_level<U>(rows + (beg + 64 * ROW_KEEP_L1) + lane, nit - ROW_KEEP_L1, M);
    } else {
      forward_level<U>(rows + beg + lane, nit, M);
    }
    wave_fence();
    forward_levels_kept<U, SH, L + 1, K1>(rows, kr, k1, M, lane);
  }
}
// (K counts the levels done: level L = nlevels - 1 - K, so that the call site names no member of SH)
template <int U, class SH, int K, bool K1, int NK, int N1>
__device__ __forceinline__ void backward_levels_kept(const MtpRow8 *rows, const MtpRow8 (&kr)[NK], const MtpRow8 (&k1)[N1],
                                                     const double *M, double *D, int lane)
{
  if constexpr (K < SH::nlevels) {
    constexpr int L = SH::nlevels - 1 - K;
    constexpr int beg = SH::level_rows(L), nit = level_blocks<SH>(L);
    if constexpr (level_kept<SH>(L)) {
      backward_level_kept<U, nit>(&kr[kept_before<SH>(L)], M, D);
    } else if constexpr (K1 && L == 0) {
      static_assert(N1 == ROW_KEEP_L1 && ROW_KEEP_L1 % U == 0 && nit >= ROW_KEEP_L1, "whole trips from registers");
#pragma unroll
      for (int b = 0; b < ROW_KEEP_L1; b += U) backward_level_kept<U, U>(&k1[b], M, D);
      backward_level<U>(rows + (beg + 64 * ROW_KEEP_L1) + lane, nit - ROW_KEEP_L1, M, D);
    } else {
      backward_level<U>(rows + beg + lane, nit, M, D);
    }
    wave_fence();
    backward_levels_kept<U, SH, K + 1, K1>(rows, kr, k1, M, D, lane);
  }
}

// Leaf rows (mtp_potential.hpp: products that no row reads, i.e. scalars of the basis; pair_mtp.cpp:204-233).  Their
// moments have no LDS slot in force calls.  Forward: the row's product goes straight into the site energy,
// e += cf M[a0] M[a1] with cf = linear coefficient x mult (grade calls also keep M[a3] += mult M[a0] M[a1]: the
// candidate vector lists the leaves' values).  Reverse: D[a0] += cb M[a1], D[a1] += cb M[a0] with the constant adjoint
// cb = seed(a3) x mult -- no D[a3] read.  Row per lane as above; the constants are lane-contiguous like the rows.
// The factors are final once the stored levels are done and cb is a constant, so the reverse terms issue in the same
// sweep from the factors already in registers (D must hold the seeds by then).  Every D slot still receives its seed,
// then the leaf terms in the same row and lane order, then the level terms: bitwise the same as a second pass over the
// leaf rows behind the energy, which was measured slower (profiles/r05_ab_product_tail.txt).
// FAR: rows and constants come from HBM / L2 (wide lane grids, whose rows do not fit in LDS): batches of U rows are
// requested AHEAD batches ahead of their use, as in the gather passes (one; two: equal, four: 2 % slower at level 20);
// otherwise both sit in the LDS blob.  (The ring is written for any AHEAD, and stays so: with the one-trip loops over
// it folded by hand the optimiser takes another path through the generic kernels and every one of them changes by a
// few instructions.)
template <int U, bool STORE, bool FAR>
__device__ __forceinline__ double leaf_forward(const MtpRow8 *rows, const double *cf, const double *cb, int beg, int nit,
                                               double *M, double *D, int lane)
{
  constexpr int AHEAD = 1;   // batches in flight (FAR)
  constexpr int NC = 2;      // constants per row: cf, cb
  double e = 0.0;
  const MtpRow8 *rp = rows + beg + lane;
  const double *cp = cf + lane, *bp = cb + lane;
  const int nb = (nit + U - 1) / U;
  MtpRow8 q[AHEAD][U];
  double qc[AHEAD][NC][U];
  auto fetch = [&](int b, MtpRow8 (&r)[U], double (&c)[NC][U]) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int o = 64 * min(b * U + u, nit - 1);   // uniform clamp: the tail re-reads the last block
      r[u] = rp[o];
      c[0][u] = cp[o];
      c[1][u] = bp[o];
    }
  };
  if (FAR) {
#pragma unroll
    for (int d = 0; d < AHEAD; d++)
      if (d < nb) fetch(d, q[d], qc[d]);   // uniform
  }
  for (int b0 = 0; b0 < nb; b0 += AHEAD) {
#pragma unroll
    for (int d = 0; d < AHEAD; d++) {
      const int b = b0 + d;
      if (b < nb) {   // uniform
        MtpRow8 rw[U];
        double c[NC][U], m0[U], m1[U];
        if (FAR) {
#pragma unroll
          for (int u = 0; u < U; u++) {
            rw[u] = q[d][u];
#pragma unroll
            for (int k = 0; k < NC; k++) c[k][u] = qc[d][k][u];
          }
          if (b + AHEAD < nb) fetch(b + AHEAD, q[d], qc[d]);   // uniform
        } else {
          fetch(b, rw, c);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          m0[u] = at8(M, rw[u].lo & 0xffffu);
          m1[u] = at8(M, rw[u].lo >> 16);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
          if (b * U + u < nit) {   // uniform branch
            const double v = m0[u] * m1[u];
            e = fma(c[0][u], v, e);
            if (STORE) lds_add(&at8(M, rw[u].hi & 0xffffu), (double) ((int) rw[u].hi >> 16) * v);
            lds_add(&at8(D, rw[u].lo >> 16), c[1][u] * m0[u]);
            lds_add(&at8(D, rw[u].lo & 0xffffu), c[1][u] * m1[u]);
          }
      }
    }
  }
  wave_fence();
  return e;
}

// Phase 4, gather form (round 2).  A level of a pass is a list of chunks; lane l of a group of 64 lanes runs one chunk:
// acc = sum_u mult_u X[o0_u] Y[o1_u] over its CS operations, then ONE atomic add T[tgt] += acc.  Forward: X = Y = T =
// moments (rows of one target); reverse: X = adjoints, Y = moments, T = adjoints (the terms of one destination), so a
// reverse level issues one ds_add_f64 per CS terms instead of two per row.  Operations (8 bytes, lane-contiguous) come
// from HBM / L2; those of the next trip are requested before the current trip's operands are read (a ring of 2, 4 or
// 8 trips in flight was measured slower at level 20: 1.46 / 1.50 / 1.60 against 1.40 ms).
template <int CS>
__device__ __forceinline__ void gather_groups(const MtpRow8 *rp, int ngroups, const double *X, const double *Y, double *T)
{
  constexpr int U = CS >= 4 ? 4 : CS;        // operations of one chunk in flight
  constexpr int G = CS >= 4 ? 1 : 4 / CS;    // chunks in flight
  constexpr int PARTS = CS / U;              // trips per chunk (CS = 8: two)
  const int ntrip = ((ngroups + G - 1) / G) * PARTS;
  auto fetch = [&](int trip, MtpRow8 (&dst)[G][U]) {
    const int g0 = (trip / PARTS) * G, part = trip % PARTS;
#pragma unroll
    for (int j = 0; j < G; j++)
#pragma unroll
      for (int u = 0; u < U; u++) dst[j][u] = rp[64 * (min(g0 + j, ngroups - 1) * CS + part * U + u)];
  };
  double acc[G];
#pragma unroll
  for (int j = 0; j < G; j++) acc[j] = 0.0;
  MtpRow8 nxt[G][U];
  fetch(0, nxt);
  for (int trip = 0; trip < ntrip; trip++) {
    MtpRow8 cur[G][U];
#pragma unroll
    for (int j = 0; j < G; j++)
#pragma unroll
      for (int u = 0; u < U; u++) cur[j][u] = nxt[j][u];
    if (trip + 1 < ntrip) fetch(trip + 1, nxt);   // uniform
    double xv[G][U], yv[G][U];
#pragma unroll
    for (int j = 0; j < G; j++)
#pragma unroll
      for (int u = 0; u < U; u++) {
        xv[j][u] = at8(X, cur[j][u].lo & 0xffffu);
        yv[j][u] = at8(Y, cur[j][u].lo >> 16);
      }
#pragma unroll
    for (int j = 0; j < G; j++)
#pragma unroll
      for (int u = 0; u < U; u++) acc[j] = fma((double) ((int) cur[j][u].hi >> 16) * xv[j][u], yv[j][u], acc[j]);
    if (trip % PARTS == PARTS - 1) {
      const int g0 = (trip / PARTS) * G;
#pragma unroll
      for (int j = 0; j < G; j++) {
        if (g0 + j < ngroups) lds_add(&at8(T, cur[j][0].hi & 0xffffu), acc[j]);   // uniform branch
        acc[j] = 0.0;
      }
    }
  }
}

// one pass: the levels in the order the segment table lists them (forward: ascending, reverse: descending)
__device__ __forceinline__ void gather_pass(const MtpRow8 *prog, const int *seg, int nlevels, const double *X,
                                            const double *Y, double *T, int lane)
{
  for (int l = 0; l < nlevels; l++) {
    const int first = __builtin_amdgcn_readfirstlane(seg[4 * l]), ngroups = __builtin_amdgcn_readfirstlane(seg[4 * l + 1]);
    const int cs = __builtin_amdgcn_readfirstlane(seg[4 * l + 2]);
    const MtpRow8 *rp = prog + (size_t) first * 64 + lane;
    if (cs == 4) gather_groups<4>(rp, ngroups, X, Y, T);
    else if (cs == 8) gather_groups<8>(rp, ngroups, X, Y, T);
    else if (cs == 2) gather_groups<2>(rp, ngroups, X, Y, T);
    else gather_groups<1>(rp, ngroups, X, Y, T);
    wave_fence();
  }
}

// ---- phase 5 helpers ------------------------------------------------------------------------
// sum_{i<C} coef[i] * m[i] in one accumulation chain from 0.0; the coefficient address is the same in all lanes of a
// half (LDS broadcast: a ds_read_b64 per coefficient; two and four chains were measured 0.5 % and 0.9 % slower)
template <int C> __device__ __forceinline__ double poly_eval(unsigned coef, const double *m)
{
  double a = 0.0;
#pragma unroll
  for (int i = 0; i < C; i++) a = fma(lds_ld(coef, i), m[i], a);
  return a;
}

// The same sum with the coefficients broadcast by DPP instead of by LDS: the lanes of a row of 16 belong to one half
// (rows 0-1: half 0, rows 2-3: half 1), so coef_l = the block of this lane's half + 8 (lane & 15) bytes reads 16
// coefficients per ds_read_b64 (one LDS cycle per half-wavefront, 32 consecutive banks: conflict-free), and
// v_fmac_f64_dpp row_newbcast:i hands coefficient i to its row.  Same FMAs in the same order as poly_eval (bitwise the
// same G; profiles/r04_ab_coef_dpp.txt has the timing of the two); lanes whose coefficient lies past the block read
// whatever follows it in the image and are never broadcast.
template <int C, int K0> __device__ __forceinline__ void dpp_chunks(double &a, const double *c, const double *m)
{
  if constexpr (K0 < C) {
    fmac_row_bcast<(C - K0 < 16 ? C - K0 : 16)>(a, c[K0 / 16], m + K0);
    dpp_chunks<C, K0 + 16>(a, c, m);
  }
}
template <int C> __device__ __forceinline__ double poly_eval_dpp(unsigned coef_l, const double *m)
{
  constexpr int K = (C + 15) / 16;   // 16-coefficient chunks: all reads first, one accumulation chain
  double c[K];
#pragma unroll
  for (int k = 0; k < K; k++) c[k] = lds_ld(coef_l, 16 * k);
  double a = 0.0;
  dpp_chunks<C, 0>(a, c, m);
  return a;
}
// DPP for C >= 2 only: a single coefficient is one read either way, and the DPP form adds the zeroing of the sum.
// coef: the block's address, + 8 (lane & 15) bytes where coef_dpp<C>.
template <int C> constexpr bool coef_dpp = C >= 2;
template <int C> __device__ __forceinline__ double poly_sum(unsigned coef, const double *m)
{
  if constexpr (coef_dpp<C>) return poly_eval_dpp<C>(coef, m);
  else return poly_eval<C>(coef, m);
}

// Slots of tensor rank NU: m[] holds the monomials of degree NU-1 of this lane's neighbour, ordered
// (a descending, then b descending): idx(a, b, c) = j (j + 1) / 2 + c with j = b + c.  A slot's coefficient
// block is [d/dx | d/dy | d/dz], each over those monomials.  UA/VA collect sum_s g_s dP_s/dx (half 0) or
// dP_s/dz (half 1) and the same with dg_s / nu; UB/VB the d/dy terms of the slots this half owns.
// NODG: no dg rows -- VA / VB collect sum_s f'_mu(s) (r^-nu / nu) G_s instead (f'_mu(r) of this lane's neighbour from
// row fp_row + mu of the tile, rw = r^-NU on entry) and the caller subtracts (UA, UB) / r at the end:
// dg_s = f'_mu r^-nu - nu g_s / r.
// GRADE (fused candidate vectors): W[mu] collects this lane's share of W_mu(n) = sum_{s in mu} P_s(r_n) / r_n^nu
// (pair_mtp_extrapolation.cpp:193-198), again through P_s = (r . grad P_s) / nu.
// The radial function mu of a slot, for the force phase.  The table smu[] in the LDS blob is atom-invariant, and in the
// nodg layouts the row address of f'_mu depends on it: read where it is needed, every slot of every tile costs two
// dependent LDS round trips (mu, then f'_mu) instead of one.  The 3-per-SIMD build has Mu <= 4 and ranks <= 6, hence at
// most 28 slots (the planner checks 32, mtp_context.hip): there the whole table is two bits per slot in one SGPR pair,
// formed once per wavefront, and a lookup is a shift and a mask (scalar for a uniform slot, v_lshrrev_b64 per lane).
// The 2-per-SIMD builds keep the reads (PACKED = false): two more SGPRs across the atom loop cost them spills
// (profiles/r06_ab_param_loads.txt).
template <bool PACKED> struct SlotMu {
  const int *smu;
  unsigned long long bits;   // PACKED: mu(s) = bits >> 2 s & 3
  template <bool NODG, bool GRADE> __device__ __forceinline__ int uniform(int s) const   // s wave-uniform
  {
    if constexpr (PACKED) return (int) (bits >> (2 * s)) & 3;
    else return (NODG || GRADE) ? __builtin_amdgcn_readfirstlane(smu[s]) : 0;
  }
  template <bool NODG, bool GRADE> __device__ __forceinline__ int per_lane(int s) const
  {
    if constexpr (PACKED) return (int) (bits >> (2 * s)) & 3;
    else return (NODG || GRADE) ? smu[s] : 0;
  }
};

// FPR (fp_regs_ct, NODG only): f'_mu of this lane's neighbour comes from F[mu] instead of row fp_row + mu.
template <int NU, int DEG, int PITCH, bool GRADE, bool NODG, class SH, class SMU, bool FPR = false>
__device__ __forceinline__ void force_degree(KP kp, unsigned pcol, unsigned pcoef, unsigned pcoef_l, int part, double x,
                                             double y, double z, double *m, double &UA, double &VA, double &UB,
                                             double &VB, const SMU &smu, double inv, double rw, double *W,
                                             const double (&F)[MTP_FP_N])
{
  if constexpr (NU <= DEG) {
    constexpr int C = NU * (NU + 1) / 2;   // monomials of degree NU-1
    const unsigned pc = coef_dpp<C> ? pcoef_l : pcoef;   // pcoef_l = pcoef + 8 (lane & 15): DPP chunks (poly_sum)
    if (NU < SHF(P)) {
      const int s0 = SHA(deg_first, NU), cnt = SHA(deg_first, NU + 1) - s0;
      const double inv_nu = 1.0 / NU;
      const unsigned dgo = 8u * (unsigned) SHF(dg_off);
      const unsigned pfp = pcol + 8u * (unsigned) (SHF(fp_row) * PITCH);   // f' rows of this lane's column (NODG)
      const double rwn = rw * inv_nu;
      const double wa = GRADE ? (part ? z : x) * rwn : 0.0, wb = GRADE ? y * rwn : 0.0;
      {
        unsigned ca = pc + 8u * (unsigned) (SHA(deg_coef, NU) + part * 2 * C);
        unsigned cg = pcol + 8u * (unsigned) (s0 * PITCH);
        for (int it = 0; it < cnt; it++) {
          // the slot, hence mu, is wave-uniform in this pass
          const int mu = smu.template uniform<NODG, GRADE>(s0 + it);
          const double g = lds_ld(cg, 0);
          double dg;
          if constexpr (FPR) dg = fp_pick(F, slot_mu_of<SH>(s0 + it));
          else dg = NODG ? lds_ld(pfp + 8u * (unsigned) (mu * PITCH), 0) : lds_ld(cg + dgo, 0);   // NODG: f'_mu (mu: SGPR)
          const double G = poly_sum<C>(ca, m);
          UA = fma(g, G, UA);
          VA = fma(dg * (NODG ? rwn : inv_nu), G, VA);
          if (GRADE) {
            const double val = G * wa;
            if (mu == 0) W[0] += val;
            else if (mu == 1) W[1] += val;
            else if (mu == 2) W[2] += val;
            else W[3] += val;
          }
          ca += 8u * 3 * C;
          cg += 8u * PITCH;
        }
      }
      for (int it = 0; 2 * it < cnt; it++) {
        const int si = 2 * it + part;
        const bool ok = si < cnt;
        const int sc = ok ? si : 0;
        // (per-lane sc: 24-bit multiplies are full rate, 32-bit ones a quarter of it)
        const unsigned cb = pc + 8u * (unsigned) (SHA(deg_coef, NU) + C) + (unsigned) mul24(sc, 8 * 3 * C);
        const unsigned cg = pcol + (unsigned) mul24(s0 + sc, 8 * PITCH);
        // (the halves hold different slots, hence different mu: a per-lane value here)
        const int mu_raw = smu.template per_lane<NODG, GRADE>(s0 + sc);
        const double g_raw = lds_ld(cg, 0);
        double dg_raw;
        if constexpr (FPR) {   // the halves' slots s0 + 2 it and s0 + 2 it + 1 are uniform: one select between their registers
          const double f0 = fp_pick(F, slot_mu_of<SH>(s0 + 2 * it));
          const double f1 = 2 * it + 1 < cnt ? fp_pick(F, slot_mu_of<SH>(s0 + 2 * it + 1)) : 0.0;
          dg_raw = part ? f1 : f0;
        } else {
          dg_raw = NODG ? lds_ld(pfp + (unsigned) mul24(mu_raw, 8 * PITCH), 0) : lds_ld(cg + dgo, 0);
        }
        const double G = poly_sum<C>(cb, m);
        const double g = ok ? g_raw : 0.0, dg = ok ? dg_raw : 0.0;
        UB = fma(g, G, UB);
        VB = fma(dg * (NODG ? rwn : inv_nu), G, VB);
        const int mu = ok ? mu_raw : -1;
        if (GRADE) {
          const double val = G * wb;
#pragma unroll
          for (int v = 0; v < 4; v++) W[v] += mu == v ? val : 0.0;
        }
      }
      if constexpr (NU < DEG) {
        // raise the monomials to degree NU: the new a = 0 tail from the old one, then the head times x
        constexpr int T0 = (NU - 1) * NU / 2;
#pragma unroll
        for (int c = 0; c < NU; c++) m[C + c] = y * m[T0 + c];
        m[C + NU] = z * m[T0 + NU - 1];
#pragma unroll
        for (int i = 0; i < C; i++) m[i] *= x;
        force_degree<NU + 1, DEG, PITCH, GRADE, NODG, SH, SMU, FPR>(kp, pcol, pcoef, pcoef_l, part, x, y, z, m, UA, VA, UB, VB, smu, inv, rw * inv, W, F);
      }
    }
  }
}

}   // namespace
