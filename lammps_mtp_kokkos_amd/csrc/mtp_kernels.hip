// CDNA4 (gfx950) kernels of the MTP pair-style compute path.
//
// One 64-lane wavefront owns one atom (the native counterpart of both reference GPU
// styles, KOKKOS/pair_mtp_kokkos.cpp:404-660 and KOKKOS/pair_mtps_kokkos.cpp:438-708),
// and the per-pair Jacobian the reference spills to HBM
// (d_moment_jacobian[N][J][B][3], pair_mtp_kokkos.cpp:270-282) is never formed:
//
//   0. tables       every workgroup copies the read-mostly potential tables (packed times
//                   rows, level offsets, radial coefficients, slots, seeds) into the head
//                   of its LDS once; a persistent grid-stride loop over atoms follows
//   1. compaction   lanes = list entries: r^2 <= rc^2 test (pair_mtp.cpp:120-127),
//                   ballot/prefix -> in-cutoff neighbours in LDS
//   2. tile tables  per in-cutoff neighbour n, entry-major in LDS (row e, column n):
//                   g[mu,nu](n) = f_mu(r)/r^nu and dg/dr (Chebyshev recurrence + radial
//                   contraction, mtp_rb_chevbyshev_basis.cpp:29-54, pair_mtp.cpp:139-166)
//                   and the coordinate powers x^p (pair_mtp.cpp:133-136)
//   3. basic moments the wavefront is NG neighbour groups x KL block lanes: lane (q, kl) owns NB blocks of
//                   3 heads (g_s x^a) x 3 tails (y^b z^c) = 9 basics (tiled on the host) and the neighbours
//                   n = q + NG m, and accumulates M_k += g x^a y^b z^c in registers (pair_mtp.cpp:154-172)
//                   from 12 LDS reads per block and column; the table row pitch is a compile-time constant
//                   so every LDS read is base register + immediate; NG-way permlane-swap sum at the end
//   4. products     lanes = times rows, one dependency level at a time, moments and
//                   adjoints in LDS with ds_add_f64 (pair_mtp.cpp:196-233)
//   5. forces       per radial slot s = (mu, nu) the adjoints of its basics are the coefficients of a
//                   homogeneous polynomial P_s(x, y, z) = sum_k D_k x^a y^b z^c of degree nu, and
//                   F_ij = sum_s [ dg_s P_s r/|r| + g_s grad P_s ]  (pair_mtp.cpp:174-191, 236-246 summed
//                   over k), with P_s = (r . grad P_s) / nu (Euler).  Lanes = (neighbour, half): every
//                   lane raises the monomials of its neighbour degree by degree in registers and
//                   evaluates the derivative polynomials with coefficients broadcast by DPP from one per-lane LDS
//                   read per 16 of them (half 0: d/dx, half 1: d/dz, d/dy split between the halves by slot); 64 lanes then scatter
//                   f_j -= F_ij with fp64 HBM atomics and tally the virial (pair_mtp.cpp:248-277)
//
// Everything is fp64 (the reference's F_FLOAT); indices are int32.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mtp_device.hpp"

#include "mtp_kernel_common.hpp"
#include "mtp_wave_body.hpp"

namespace {

// WPS = wavefronts per SIMD the register budget is sized for (mtp_wave_kernel_body.hpp).  The generic kernels: no field of the
// argument block is fixed at build time.
template <int KL, int NB, int PITCH, bool GRADE, int DEG, int WPS>
__global__ void __launch_bounds__(WPS == 3 ? 768 : 512, WPS) mtp_wave_kernel(const MtpDevParams p_arg)
{
  (void) p_arg;   // read through the kernarg segment pointer
  using SH = ShapeGeneric;
#include "mtp_wave_kernel_body.hpp"
}

// f[k] += fq[k] 2^-40, fq[k] = 0: the end of a deterministic-mode force call
__global__ void __launch_bounds__(256) mtp_fixed_to_force(long long *__restrict__ fq, double *__restrict__ f, int n3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const long long q = fq[e];
  if (q != 0) {
    f[e] += (double) q * (1.0 / MTP_FIXED_SCALE);
    fq[e] = 0;
  }
}

// folds the per-wave tally slots into ev[7] (accumulating) and clears them: one workgroup of 512 threads per
// quantity, a fixed summation order (lane-strided partial sums, then a fixed tree), so the totals do not depend on timing
__global__ void __launch_bounds__(512) mtp_ev_finish(double *ev_slots, double *ev)
{
  __shared__ double part[8];
  const int q = blockIdx.x;   // 0..6
  double s = 0.0;
  for (int k = threadIdx.x; k < MTP_EV_SLOTS; k += 512) {
    s += ev_slots[(size_t) q * MTP_EV_SLOTS + k];
    ev_slots[(size_t) q * MTP_EV_SLOTS + k] = 0.0;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < 8; w++) t += part[w];
    ev[q] += t;
  }
}

// The tally fold and the fold of the received ghost forces of a decomposed step in one launch (mtp_halo_force_step):
// workgroups [0, 7) are mtp_ev_finish (when `fold`), the others add frecv[e] onto f[3 idx[e / 3] + e % 3] (fp64
// atomics: an owned atom can be a ghost on several peers).
__global__ void __launch_bounds__(512) mtp_ev_finish_unpack(double *ev_slots, double *ev, int fold, double *__restrict__ f,
                                                           const int *__restrict__ idx, const double *__restrict__ frecv,
                                                           int n3)
{
  if (blockIdx.x >= 7) {
    const int e = (blockIdx.x - 7) * 512 + threadIdx.x;
    if (e < n3) {
      const int k = e / 3, c = e - 3 * k;
      unsafeAtomicAdd(&f[3 * (size_t) idx[k] + c], frecv[e]);
    }
    return;
  }
  if (!fold) return;   // (whole workgroup)
  __shared__ double part[8];
  const int q = blockIdx.x;   // 0..6
  double s = 0.0;
  for (int k = threadIdx.x; k < MTP_EV_SLOTS; k += 512) {
    s += ev_slots[(size_t) q * MTP_EV_SLOTS + k];
    ev_slots[(size_t) q * MTP_EV_SLOTS + k] = 0.0;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < 8; w++) t += part[w];
    ev[q] += t;
  }
}

// f[0, n) = 0 in one launch (hipMemsetAsync splits into two fill kernels for sizes that are not multiples of its tile)
__global__ void __launch_bounds__(256) mtp_zero_kernel(double2 *__restrict__ p, size_t n2, double *__restrict__ tail, int ntail)
{
  const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (i < n2) p[i] = make_double2(0.0, 0.0);
  if (i < (size_t) ntail) tail[i] = 0.0;
}

// ---- MaxVol grade: grades[i] = max_r | sum_c cvec[i][c] Ainv[r][c] |  (pair_mtp_extrapolation.cpp:347-358)
// One inverse active set for every atom: a dense [atoms x C] x [C x C] fp64 contraction, done on
// the matrix cores with v_mfma_f64_16x16x4_f64.  One wavefront owns 16 atoms; M = atoms, N = rows of
// Ainv, K = coefficients.  Operand lane maps (cdna_hip_programming.md section 3): A[i = l&15][k = l>>4],
// B[k = l>>4][j = l&15], D: col = l&15, row = (l>>4) + 4*reg.  Both arrays are zero padded to cpad
// (multiple of 16), so no bounds checks on c or r.
typedef double double4_t __attribute__((ext_vector_type(4)));

template <int KS_REG>   // > 0: the 16 x cpad block of cvec lives in registers (cpad <= 4*KS_REG)
__global__ void __launch_bounds__(256) mtp_grade_kernel(const double *__restrict__ cvec,
                                                       const double *__restrict__ ainv, int cpad, int inum,
                                                       const int *__restrict__ ilist, double *grades,
                                                       double *max_grade)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int atom0 = (blockIdx.x * 4 + wave) * 16;
  if (atom0 >= inum) return;
  const int li = lane & 15, lk = lane >> 4;
  const int ksteps = cpad >> 2;
  const int arow = min(atom0 + li, inum - 1);   // clamped: rows past the end are computed and dropped
  const double *ap = cvec + (size_t) arow * cpad + lk;
  double areg[KS_REG > 0 ? KS_REG : 1];
  if (KS_REG > 0) {
#pragma unroll
    for (int ks = 0; ks < KS_REG; ks++) areg[ks] = ks < ksteps ? ap[4 * ks] : 0.0;
  }
  double gmax[4] = {0.0, 0.0, 0.0, 0.0};
  for (int n0 = 0; n0 < cpad; n0 += 16) {
    const double *bp = ainv + (size_t) (n0 + li) * cpad + lk;   // B[k][j] = Ainv[n0 + j][k]
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    if (KS_REG > 0) {
#pragma unroll
      for (int ks = 0; ks < KS_REG; ks++)
        if (ks < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[ks], bp[4 * ks], acc, 0, 0, 0);
    } else {
      for (int ks = 0; ks < ksteps; ks++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * ks], bp[4 * ks], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) gmax[r] = fmax(gmax[r], fabs(acc[r]));
  }
  // max over the 16 lanes (Ainv rows) that share l>>4
#pragma unroll
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int sft = 1; sft < 16; sft <<= 1) gmax[r] = fmax(gmax[r], shfl_xor_f64(gmax[r], sft));
  }
  double wmax = 0.0;
  if (li == 0) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int a = atom0 + lk + 4 * r;   // D row = (l>>4) + 4*reg
      if (a < inum) {
        grades[ilist[a]] = gmax[r];   // pair_mtp_extrapolation.cpp:335
        wmax = fmax(wmax, gmax[r]);
      }
    }
  }
#pragma unroll
  for (int sft = 16; sft < 64; sft <<= 1) wmax = fmax(wmax, shfl_xor_f64(wmax, sft));
  // grades are >= 0, so their IEEE bit patterns order like unsigned integers
  if (lane == 0 && max_grade)
    atomicMax(reinterpret_cast<unsigned long long *>(max_grade), (unsigned long long) __double_as_longlong(wmax));
}

// The same contraction for cpad <= 160 with the inverse active set shared through LDS: a workgroup of 8 wavefronts
// (128 atoms, their 16 x cpad blocks of cvec in registers) walks the 16-row tiles of Ainv together; each tile is
// fetched from L2 once per workgroup into a double-buffered LDS stage, already in MFMA operand order (the host
// stores Ainv as [tile][k-step][lane], lane (j = l&15, k = l>>4) holding Ainv[16 tile + j][4 kstep + k]), so a B
// operand is one conflict-free 512-byte ds_read per MFMA.  L2 traffic drops from 205 KB per 16 atoms to per 128.
template <int KS_REG>
__global__ void __launch_bounds__(512) mtp_grade_kernel_lds(const double *__restrict__ cvec,
                                                           const double *__restrict__ ainv_t, int cpad, int inum,
                                                           const int *__restrict__ ilist, double *grades,
                                                           double *max_grade)
{
  extern __shared__ double stage[];   // [2][cpad * 16]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int atom0 = (blockIdx.x * 8 + wave) * 16;
  const bool live = atom0 < inum;     // idle wavefronts still take part in the staging and the barriers
  const int li = lane & 15, lk = lane >> 4;
  const int ksteps = cpad >> 2, ntile = cpad >> 4, tile_doubles = cpad * 16;
  const int arow = min(atom0 + li, inum - 1);   // clamped: rows past the end are computed and dropped
  const double *ap = cvec + (size_t) arow * cpad + lk;
  double areg[KS_REG];
#pragma unroll
  for (int ks = 0; ks < KS_REG; ks++) areg[ks] = ks < ksteps ? ap[4 * ks] : 0.0;
  constexpr int PF = (KS_REG * 64 + 511) / 512;   // doubles per thread per tile
  double pf[PF];
#pragma unroll
  for (int u = 0; u < PF; u++) {
    const int e = threadIdx.x + 512 * u;
    if (e < tile_doubles) stage[e] = ainv_t[e];
  }
  __syncthreads();
  double gmax[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = 0; t < ntile; t++) {
    const double *cur = stage + (size_t) (t & 1) * tile_doubles;
    double *nxt = stage + (size_t) ((t + 1) & 1) * tile_doubles;
    if (t + 1 < ntile) {
#pragma unroll
      for (int u = 0; u < PF; u++) {
        const int e = threadIdx.x + 512 * u;
        pf[u] = e < tile_doubles ? ainv_t[(size_t) (t + 1) * tile_doubles + e] : 0.0;
      }
    }
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS_REG; ks++)
      if (ks < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[ks], cur[ks * 64 + lane], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) gmax[r] = fmax(gmax[r], fabs(acc[r]));
    if (t + 1 < ntile) {
#pragma unroll
      for (int u = 0; u < PF; u++) {
        const int e = threadIdx.x + 512 * u;
        if (e < tile_doubles) nxt[e] = pf[u];
      }
    }
    __syncthreads();
  }
  // max over the 16 lanes (Ainv rows) that share l>>4
#pragma unroll
  for (int r = 0; r < 4; r++) {
    gmax[r] = fmax(gmax[r], partner_f64<1>(gmax[r]));
    gmax[r] = fmax(gmax[r], partner_f64<2>(gmax[r]));
    gmax[r] = fmax(gmax[r], partner_f64<4>(gmax[r]));
    gmax[r] = fmax(gmax[r], partner_f64<8>(gmax[r]));
  }
  double wmax = 0.0;
  if (live && li == 0) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int a = atom0 + lk + 4 * r;   // D row = (l>>4) + 4*reg
      if (a < inum) {
        grades[ilist[a]] = gmax[r];   // pair_mtp_extrapolation.cpp:335
        wmax = fmax(wmax, gmax[r]);
      }
    }
  }
  wmax = fmax(wmax, partner_f64<16>(wmax, lane));
  wmax = fmax(wmax, partner_f64<32>(wmax, lane));
  // grades are >= 0, so their IEEE bit patterns order like unsigned integers
  if (live && lane == 0 && max_grade)
    atomicMax(reinterpret_cast<unsigned long long *>(max_grade), (unsigned long long) __double_as_longlong(wmax));
}

// Output-stationary form of the same contraction (round 2): the wavefront keeps the NT = cpad / 16 accumulator tiles of
// its 16 atoms (16 atoms x cpad rows of Ainv) and walks K in slabs of four k-steps; a slab of Ainv (4 k-steps of EVERY
// 16-row tile, 2 KB per tile, contiguous in the tiled layout) is staged through the double-buffered LDS by the
// workgroup and the four A operands of the next slab are fetched while the current slab's 4 NT MFMAs run.  The
// A-stationary kernel above first pulls its whole 16 x cpad block of candidate vectors into registers -- every
// wavefront of the one-round launch at the same time, 84 MB with the matrix pipe idle -- and its MFMAs form one
// dependent chain per tile; here the loads are spread over the K loop and NT independent chains are in flight.
#ifndef MTP_GRADE_TPB
#define MTP_GRADE_TPB 512
#define MTP_GRADE_WPE 2
#endif
template <int NT, int TPB, int WPE>   // TPB threads per workgroup (TPB / 64 wavefronts of 16 atoms), WPE wavefronts per SIMD
__global__ void __launch_bounds__(TPB, WPE) mtp_grade_kernel_os(const double *__restrict__ cvec,
                                                          const double *__restrict__ ainv_t, int inum,
                                                          const int *__restrict__ ilist, double *grades,
                                                          double *max_grade)
{
  extern __shared__ double stage[];   // [2][NT * 256]
  constexpr int cpad = 16 * NT, KS = 4 * NT, NSLAB = NT, slab_doubles = NT * 256;
  constexpr int PF = (slab_doubles + TPB - 1) / TPB;   // doubles per thread per slab
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int atom0 = (blockIdx.x * (TPB / 64) + wave) * 16;
  const bool live = atom0 < inum;     // idle wavefronts still take part in the staging and the barriers
  const int li = lane & 15, lk = lane >> 4;
  const int arow = min(atom0 + li, inum - 1);   // clamped: rows past the end are computed and dropped
  const double *ap = cvec + (size_t) arow * cpad + lk;
  // slab c, element e = tile * 256 + (u * 64 + lane)  <-  ainv_t[(tile * KS + 4 c) * 64 + (u * 64 + lane)]
  auto src = [&](int c, int e) { return ainv_t[((size_t) (e >> 8) * KS + 4 * c) * 64 + (e & 255)]; };
  double pf[PF], a_cur[4], a_nxt[4];
#pragma unroll
  for (int u = 0; u < PF; u++) {
    const int e = threadIdx.x + TPB * u;
    if (e < slab_doubles) stage[e] = src(0, e);
  }
#pragma unroll
  for (int u = 0; u < 4; u++) a_cur[u] = ap[4 * u];
  __syncthreads();
  double4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < NSLAB; c++) {
    const double *cur = stage + (size_t) (c & 1) * slab_doubles + lane;
    double *nxt = stage + (size_t) ((c + 1) & 1) * slab_doubles;
    if (c + 1 < NSLAB) {
#pragma unroll
      for (int u = 0; u < PF; u++) {
        const int e = threadIdx.x + TPB * u;
        pf[u] = e < slab_doubles ? src(c + 1, e) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) a_nxt[u] = ap[4 * (4 * (c + 1) + u)];
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int t = 0; t < NT; t++)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[u], cur[(t * 4 + u) * 64], acc[t], 0, 0, 0);
    if (c + 1 < NSLAB) {
#pragma unroll
      for (int u = 0; u < PF; u++) {
        const int e = threadIdx.x + TPB * u;
        if (e < slab_doubles) nxt[e] = pf[u];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) a_cur[u] = a_nxt[u];
    }
    __syncthreads();
  }
  double gmax[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) gmax[r] = fmax(gmax[r], fabs(acc[t][r]));
  // max over the 16 lanes (Ainv rows) that share l>>4
#pragma unroll
  for (int r = 0; r < 4; r++) {
    gmax[r] = fmax(gmax[r], partner_f64<1>(gmax[r]));
    gmax[r] = fmax(gmax[r], partner_f64<2>(gmax[r]));
    gmax[r] = fmax(gmax[r], partner_f64<4>(gmax[r]));
    gmax[r] = fmax(gmax[r], partner_f64<8>(gmax[r]));
  }
  double wmax = 0.0;
  if (live && li == 0) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int a = atom0 + lk + 4 * r;   // D row = (l>>4) + 4*reg
      if (a < inum) {
        grades[ilist[a]] = gmax[r];   // pair_mtp_extrapolation.cpp:335
        wmax = fmax(wmax, gmax[r]);
      }
    }
  }
  wmax = fmax(wmax, partner_f64<16>(wmax, lane));
  wmax = fmax(wmax, partner_f64<32>(wmax, lane));
  if (live && lane == 0 && max_grade)
    atomicMax(reinterpret_cast<unsigned long long *>(max_grade), (unsigned long long) __double_as_longlong(wmax));
}

// configuration mode: coeff_ders[c] += sum_i cvec[i][c]  (pair_mtp_extrapolation.cpp:97-98, 240-252, 327)
__global__ void __launch_bounds__(256) mtp_colsum_kernel(const double *__restrict__ cvec, int cpad, int C, int inum,
                                                        double *coeff_ders)
{
  const int rows_per_block = 256;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(inum, r0 + rows_per_block);
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int r = r0; r < r1; r++) s += cvec[(size_t) r * cpad + c];
  unsafeAtomicAdd(&coeff_ders[c], s);
}

// ---- batched configurations: per-configuration (segmented) forms of the tallies above.  Configuration k owns rows
// [cfg_first[k], cfg_first[k + 1]) of the per-atom outputs of ONE force call over many cells (mtp_ghosts_build_batch).
// No atomics, and the order of every sum depends on the segment's length alone: a configuration's result does not
// depend on what else is in the batch.

// what thread t of NT co-operating threads adds up of rows [r0, r1): v[0] = sum eatom, v[1..6] = sum vatom (the
// reference tallies vatom on the central atom, pair_mtp.cpp:268-276: ghosts carry none), v[7] = max grades.  All reads
// are coalesced: vatom is walked as the flat array it is, 3 NT elements a round -- 3 NT is a multiple of 6 and NT = 4
// (mod 6) for NT = 64 and 256, so element t + NT j of every round is component (t + 4 j) % 6.
template <int NT>
__device__ __forceinline__ void segment_partials(int t, int r0, int r1, const double *__restrict__ eatom,
                                                 const double *__restrict__ vatom, const double *__restrict__ grades, double v[8])
{
  static_assert(NT % 6 == 4, "component map of the flat vatom walk");
  double e = 0.0, g = 0.0, acc[3] = {0.0, 0.0, 0.0};
  for (int r = r0 + t; r < r1; r += NT) {
    if (eatom) e += eatom[r];
    if (grades) g = fmax(g, grades[r]);
  }
  if (vatom) {
    const double *__restrict__ base = vatom + 6 * (size_t) r0;
    const int n6 = 6 * (r1 - r0);
    for (int e0 = 0; e0 < n6; e0 += 3 * NT) {
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int q = e0 + t + NT * j;
        if (q < n6) acc[j] += base[q];
      }
    }
  }
  v[0] = e;
  v[7] = g;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) s += (t + 4 * j) % 6 == c ? acc[j] : 0.0;
    v[1 + c] = s;
  }
}

static __device__ __forceinline__ void segment_wave_fold(double v[8])   // sums and the maximum over the wavefront
{
#pragma unroll
  for (int q = 0; q < 7; q++) v[q] = wave_sum(v[q]);
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) v[7] = fmax(v[7], shfl_xor_f64(v[7], sft));
}

// A workgroup of four wavefronts owns four consecutive configurations: one wavefront each for segments of up to
// MTP_BATCH_WAVE_ROWS rows (the sizes this path is for: 1 to 200 atoms), the whole workgroup, one after another, for the
// longer ones.  energy[k] and virial[k][6] carry the sign and component order of d_ev; cfg_grade[k] = max of the
// segment's grades (neighbourhood mode); an empty segment writes zeros.  Any output (with its input) may be null.
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) mtp_batch_reduce_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                                          const double *__restrict__ eatom,
                                                                          const double *__restrict__ vatom,
                                                                          const double *__restrict__ grades,
                                                                          double *__restrict__ energy, double *__restrict__ virial,
                                                                          double *__restrict__ cfg_grade)
{
  __shared__ double part[MTP_BATCH_BLOCK / 64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = blockIdx.x * (MTP_BATCH_BLOCK / 64);
  auto write = [&](int k, const double *v) {
    if (energy) energy[k] = v[0];
    if (virial) {
#pragma unroll
      for (int c = 0; c < 6; c++) virial[6 * (size_t) k + c] = v[1 + c];
    }
    if (cfg_grade) cfg_grade[k] = v[7];
  };
  double v[8];
  if (k0 + wave < ncfg) {   // (the whole wavefront)
    const int k = k0 + wave, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 - r0 <= MTP_BATCH_WAVE_ROWS) {
      segment_partials<64>(lane, r0, r1, eatom, vatom, grades, v);
      segment_wave_fold(v);
      if (lane == 0) write(k, v);
    }
  }
  for (int w = 0; w < MTP_BATCH_BLOCK / 64 && k0 + w < ncfg; w++) {   // (the whole workgroup)
    const int k = k0 + w, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 - r0 <= MTP_BATCH_WAVE_ROWS) continue;
    segment_partials<MTP_BATCH_BLOCK>(threadIdx.x, r0, r1, eatom, vatom, grades, v);
    segment_wave_fold(v);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 8; q++) part[wave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double t[8];
#pragma unroll
      for (int q = 0; q < 8; q++) {
        t[q] = part[0][q];
#pragma unroll
        for (int u = 1; u < MTP_BATCH_BLOCK / 64; u++) t[q] = q < 7 ? t[q] + part[u][q] : fmax(t[q], part[u][q]);
      }
      write(k, t);
    }
    __syncthreads();
  }
}

// configuration mode: csum[k][c] = sum over the rows of configuration k of cvec[row][c] -- mtp_colsum_kernel per
// configuration (pair_mtp_extrapolation.cpp:97-98, 240-252, 327, with one "rank" per configuration).  Columns over lanes
// (every row is read coalesced), configurations over workgroups, rows in order: no atomics.  cvec is zero padded to cpad,
// so csum is; ident[k] = k is the ilist the grade kernel then takes the rows of csum by.
__global__ void __launch_bounds__(256) mtp_batch_colsum_kernel(const double *__restrict__ cvec, int cpad, int ncfg,
                                                              const int *__restrict__ cfg_first, double *__restrict__ csum,
                                                              int *__restrict__ ident)
{
  const int k = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (k >= ncfg) return;
  if (c == 0) ident[k] = k;
  if (c >= cpad) return;
  const int r0 = cfg_first[k], r1 = cfg_first[k + 1];
  double s = 0.0;
  for (int r = r0; r < r1; r++) s += cvec[(size_t) r * cpad + c];
  csum[(size_t) k * cpad + c] = s;
}

// max_grade /= natoms, 0 for no atoms (pair_mtp_extrapolation.cpp:373-376), per configuration
__global__ void __launch_bounds__(256) mtp_batch_grade_scale_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                                   double *__restrict__ cfg_grade)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= ncfg) return;
  const int n = cfg_first[k + 1] - cfg_first[k];
  cfg_grade[k] = n > 0 ? cfg_grade[k] / (double) n : 0.0;
}

template <int KL, int NB, int PITCH, bool GRADE, int DEG, int WPS>
hipError_t launch_one(const MtpDevParams &p, int grid, int wpb, size_t lds, hipStream_t st)
{
  static std::atomic<unsigned long long> attr_mask{0};
  const hipError_t e = mtp_raise_lds_limit(reinterpret_cast<const void *>(&mtp_wave_kernel<KL, NB, PITCH, GRADE, DEG, WPS>), attr_mask);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((mtp_wave_kernel<KL, NB, PITCH, GRADE, DEG, WPS>), dim3(grid), dim3(64 * wpb), lds, st, p);
  return hipGetLastError();
}

template <int KL, int NB, int DEG, int WPS>
hipError_t launch_grade(const MtpDevParams &p, int grid, int wpb, size_t lds, hipStream_t st)
{
  // only the 32-neighbour tile (pitch MTP_PITCH) is instantiated; the grade variant is its own instantiation so the
  // force-only kernel keeps its register budget
  return p.grade_flag ? launch_one<KL, NB, MTP_PITCH, true, DEG, WPS>(p, grid, wpb, lds, st)
                      : launch_one<KL, NB, MTP_PITCH, false, DEG, WPS>(p, grid, wpb, lds, st);
}

// DEG = highest tensor rank the unrolled force phase covers (monomials up to degree DEG-1 in registers):
// narrow lane grids come with ranks <= 6 in the MLIP level tables, wide ones with ranks <= 8;
// DEG = 11 is the general instantiation (the loader caps the rank at 11).  The 168-VGPR build (three wavefronts per
// SIMD) exists for the narrow grids with ranks <= 6 -- the shapes whose per-atom LDS image lets twelve wavefronts
// share a CU (mtp_wave_kernel_has_wps3() tells the planner).
template <int KL, int NB> hipError_t launch_pitch(const MtpDevParams &p, int grid, int wpb, size_t lds, hipStream_t st)
{
  constexpr int DLOW = mtp_wave_kernel_dlow(KL);
  if (mtp_wave_kernel_deg(KL, p.P) == DLOW) {
    if constexpr (KL <= 32 && NB == 1)
      if (p.wps == 3) return launch_grade<KL, NB, DLOW, 3>(p, grid, wpb, lds, st);
    return launch_grade<KL, NB, DLOW, 2>(p, grid, wpb, lds, st);
  }
  return launch_grade<KL, NB, 11, 2>(p, grid, wpb, lds, st);
}

}   // namespace

hipError_t mtp_launch_wave_kernel(const MtpDevParams &p, int grid, int wpb, size_t lds, hipStream_t st, const char **used)
{
  int KL = 0, NB = 0;
  if (used) *used = nullptr;
  if (mtp_pick_fwd_shape(p.nfb, &KL, &NB) != 0 || p.NT != 32) return hipErrorInvalidValue;
  if (wpb < 1 || wpb > (p.wps == 3 ? 12 : 8)) return hipErrorInvalidValue;
  const char *knob = std::getenv("MTP_FIXED_SHAPE");   // tests and A/B runs: 0 = generic kernels only
  if (!(knob && std::atoi(knob) == 0)) {
    const char *name = nullptr;
    const hipError_t e = mtp_launch_wave_kernel_fixed(p, grid, wpb, lds, st, &name);
    if (name) {
      if (used) *used = name;
      return e;
    }
  }
#define MTP_CASE(kl, nb) \
  if (KL == kl && NB == nb) return launch_pitch<kl, nb>(p, grid, wpb, lds, st);
  MTP_CASE(16, 1)
  MTP_CASE(32, 1)
  MTP_CASE(64, 1)
  MTP_CASE(64, 2)
  MTP_CASE(64, 3)
  MTP_CASE(64, 4)
#undef MTP_CASE
  return hipErrorInvalidValue;
}

hipError_t mtp_launch_grade_kernel(const double *cvec, const double *ainv_pad, const double *ainv_tiled, int cpad,
                                   int C, int inum, const int *ilist, double *grades, double *max_grade, hipStream_t st)
{
  (void) C;
  static const bool use_os = !(std::getenv("MTP_GRADE_OS") && std::atoi(std::getenv("MTP_GRADE_OS")) == 0);   // tuning
  if (cpad <= 160 && ainv_tiled && use_os) {
    const size_t lds = (size_t) 2 * cpad * 16 * sizeof(double);
    constexpr int TPB = MTP_GRADE_TPB, WPE = MTP_GRADE_WPE;
    const dim3 grid((inum + TPB / 4 - 1) / (TPB / 4)), block(TPB);
#define MTP_GRADE_OS_CASE(NT)                                                                                         \
  case NT:                                                                                                            \
    hipLaunchKernelGGL((mtp_grade_kernel_os<NT, TPB, WPE>), grid, block, lds, st, cvec, ainv_tiled, inum, ilist, grades,  \
                       max_grade);                                                                                    \
    break;
    switch (cpad / 16) {
      MTP_GRADE_OS_CASE(1) MTP_GRADE_OS_CASE(2) MTP_GRADE_OS_CASE(3) MTP_GRADE_OS_CASE(4) MTP_GRADE_OS_CASE(5)
      MTP_GRADE_OS_CASE(6) MTP_GRADE_OS_CASE(7) MTP_GRADE_OS_CASE(8) MTP_GRADE_OS_CASE(9) MTP_GRADE_OS_CASE(10)
      default: return hipErrorInvalidValue;
    }
#undef MTP_GRADE_OS_CASE
  } else if (cpad <= 160 && ainv_tiled) {
    const size_t lds = (size_t) 2 * cpad * 16 * sizeof(double);
    hipLaunchKernelGGL(mtp_grade_kernel_lds<40>, dim3((inum + 127) / 128), dim3(512), lds, st, cvec, ainv_tiled, cpad,
                       inum, ilist, grades, max_grade);
  } else {
    hipLaunchKernelGGL(mtp_grade_kernel<0>, dim3((inum + 63) / 64), dim3(256), 0, st, cvec, ainv_pad, cpad, inum, ilist,
                       grades, max_grade);
  }
  return hipGetLastError();
}

hipError_t mtp_launch_colsum_kernel(const double *cvec, int cpad, int C, int inum, double *coeff_ders, hipStream_t st)
{
  hipLaunchKernelGGL(mtp_colsum_kernel, dim3((C + 255) / 256, (inum + 255) / 256), dim3(256), 0, st, cvec, cpad, C, inum,
                     coeff_ders);
  return hipGetLastError();
}

hipError_t mtp_launch_batch_reduce(int ncfg, const int *cfg_first, const double *eatom, const double *vatom, const double *grades,
                                   double *energy, double *virial, double *cfg_grade, hipStream_t st)
{
  constexpr int per_block = MTP_BATCH_BLOCK / 64;
  hipLaunchKernelGGL(mtp_batch_reduce_kernel, dim3((ncfg + per_block - 1) / per_block), dim3(MTP_BATCH_BLOCK), 0, st, ncfg,
                     cfg_first, eatom, vatom, grades, energy, virial, cfg_grade);
  return hipGetLastError();
}

hipError_t mtp_launch_batch_colsum(const double *cvec, int cpad, int ncfg, const int *cfg_first, double *csum, int *ident,
                                   hipStream_t st)
{
  hipLaunchKernelGGL(mtp_batch_colsum_kernel, dim3(ncfg, (cpad + 255) / 256), dim3(256), 0, st, cvec, cpad, ncfg, cfg_first, csum,
                     ident);
  return hipGetLastError();
}

hipError_t mtp_launch_batch_grade_scale(int ncfg, const int *cfg_first, double *cfg_grade, hipStream_t st)
{
  hipLaunchKernelGGL(mtp_batch_grade_scale_kernel, dim3((ncfg + 255) / 256), dim3(256), 0, st, ncfg, cfg_first, cfg_grade);
  return hipGetLastError();
}

hipError_t mtp_raise_lds_limit(const void *fn, std::atomic<unsigned long long> &mask)
{
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev > 63 || !((mask.load(std::memory_order_acquire) >> dev) & 1ull)) {
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev <= 63) mask.fetch_or(1ull << dev, std::memory_order_release);
  }
  return hipSuccess;
}

hipError_t mtp_launch_fixed_to_force(long long *fq, double *f, int nall, hipStream_t st)
{
  hipLaunchKernelGGL(mtp_fixed_to_force, dim3((3 * nall + 255) / 256), dim3(256), 0, st, fq, f, 3 * nall);
  return hipGetLastError();
}

hipError_t mtp_launch_ev_finish_unpack(double *ev_slots, double *ev, int fold, double *f, const int *idx, const double *frecv,
                                       int n3, hipStream_t st)
{
  hipLaunchKernelGGL(mtp_ev_finish_unpack, dim3(7 + (n3 + 511) / 512), dim3(512), 0, st, ev_slots, ev, fold, f, idx, frecv, n3);
  return hipGetLastError();
}

hipError_t mtp_launch_ev_finish(double *ev_slots, double *ev, hipStream_t st)
{
  hipLaunchKernelGGL(mtp_ev_finish, dim3(7), dim3(512), 0, st, ev_slots, ev);
  return hipGetLastError();
}

// Every compile-time switch of the force kernel that differs from its shipped value, in the order of the block of
// defaults at the top of mtp_wave_body.hpp, then the grade GEMM's pair (defaults beside mtp_grade_kernel_os above).
const char *mtp_kernel_build_flags()
{
#define MTP_STR2(x) #x
#define MTP_STR(x) MTP_STR2(x)
  return ""
#if MTP_PU != 2
      "MTP_PU=" MTP_STR(MTP_PU) " "
#endif
#if MTP_FWD5 != 1
      "MTP_FWD5=" MTP_STR(MTP_FWD5) " "
#endif
#if MTP_SUM_T != 1
      "MTP_SUM_T=" MTP_STR(MTP_SUM_T) " "
#endif
#if MTP_CNT_SGPR != 1
      "MTP_CNT_SGPR=" MTP_STR(MTP_CNT_SGPR) " "
#endif
#if MTP_ROW_KEEP_L1 != 1
      "MTP_ROW_KEEP_L1=" MTP_STR(MTP_ROW_KEEP_L1) " "
#endif
#if MTP_PHASE_PRIO != 1
      "MTP_PHASE_PRIO=" MTP_STR(MTP_PHASE_PRIO) " "
#endif
#if MTP_GRADE_TPB != 512 || MTP_GRADE_WPE != 2
      "MTP_GRADE_TPB=" MTP_STR(MTP_GRADE_TPB) " "
#endif
      ;
}

hipError_t mtp_launch_zero(double *p, size_t n, hipStream_t st)   // p 16-byte aligned (hipMalloc / torch allocations are)
{
  if (n == 0) return hipSuccess;
  const size_t n2 = n / 2;
  hipLaunchKernelGGL(mtp_zero_kernel, dim3((unsigned) ((std::max<size_t>(n2, 1) + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<double2 *>(p), n2, p + 2 * n2, (int) (n - 2 * n2));
  return hipGetLastError();
}
