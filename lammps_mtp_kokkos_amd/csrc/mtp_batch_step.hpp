// What every one-launch-a-step kernel over the batched layout shares (mtp_relax.hip, mtp_relax_cell.hip, mtp_sample.hip,
// mtp_sample_cell.hip, mtp_neb.hip, mtp_hess.hip, mtp_elastic.hip): the unit constants, the fixed-order reductions over a wavefront or a workgroup of
// MTP_BATCH_BLOCK threads, the split of a workgroup over the configurations that still run, the FIRE rule with the row sweeps
// of its fixed-cell users, the 3 x 3 helpers of the kernels that move cells, and the host side of an entry point: the range
// check of the FIRE parameters, the pointer check and the launch epilogue.  Each of these is defined here and nowhere else.
// Device code is inlined into each kernel; host code is `inline`.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>
#include <type_traits>

#include "../../include/mtp_mi355x.h"
#include "mtp_device.hpp"

namespace batch_step {

// LAMMPS metal units (update.cpp): the constants of lammps_mtp_kokkos_amd/md.py
constexpr double MVV2E = 1.0364269e-4;
constexpr double FTM2V = 1.0 / MVV2E;
constexpr double KB = 8.617343e-5;

constexpr int BATCH_WAVES = MTP_BATCH_BLOCK / 64;

// the wavefront reductions: xor butterfly, a fixed order, the same bits in every lane
__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ double wave_max64(double v)
{
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v = fmax(v, __shfl_xor(v, s, 64));
  return v;
}

// the total over NT co-operating threads, the same bits in every one of them: the wavefront's own (NT = 64), or the
// wavefronts' partials combined in wave order through `part` (NT = MTP_BATCH_BLOCK: every thread of the workgroup calls)
template <int NT, bool MAX>
__device__ __forceinline__ double segment_total(double val, double *part)
{
  val = MAX ? wave_max64(val) : wave_sum64(val);
  if (NT == 64) return val;
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = val;
  __syncthreads();
  double t = part[0];
#pragma unroll
  for (int u = 1; u < BATCH_WAVES; u++) t = MAX ? fmax(t, part[u]) : t + part[u];
  __syncthreads();
  return t;
}

// The split of the kernels that skip frozen configurations (the grid is (ncfg + BATCH_WAVES - 1) / BATCH_WAVES workgroups of
// MTP_BATCH_BLOCK threads): a workgroup of four wavefronts owns four consecutive configurations, one wavefront each for
// segments of up to MTP_BATCH_WAVE_ROWS rows, the whole workgroup, one after another, for the longer ones.  Empty and frozen
// configurations are skipped: nothing of theirs is written.  body(NT, t, k, r0, r1) serves configuration k, rows [r0, r1), as
// thread t of NT -- NT a std::integral_constant, 64 or MTP_BATCH_BLOCK; it may set frozen[k] from its thread 0.  The order of
// every floating-point sum in it then depends on the segment's length alone.
template <class Body>
__device__ __forceinline__ void for_each_live_segment(int ncfg, const int *cfg_first, const int *frozen, Body body)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = blockIdx.x * BATCH_WAVES;
  if (k0 + wave < ncfg) {   // (the whole wavefront)
    const int k = k0 + wave, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 > r0 && r1 - r0 <= MTP_BATCH_WAVE_ROWS && frozen[k] == 0) body(std::integral_constant<int, 64>{}, lane, k, r0, r1);
  }
  for (int w = 0; w < BATCH_WAVES && k0 + w < ncfg; w++) {   // (the whole workgroup)
    const int k = k0 + w, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 - r0 <= MTP_BATCH_WAVE_ROWS) continue;
    const int fr = frozen[k];
    __syncthreads();   // every thread has read the flag before thread 0 may set it
    if (fr == 0) body(std::integral_constant<int, MTP_BATCH_BLOCK>{}, (int) threadIdx.x, k, r0, r1);
  }
}

// The FIRE rule.  Its state, kept per configuration or per band by the caller:
struct fire_state {
  double dt, alpha;
  int npos;
};

// one step of the state machine from the totals P = F . v, vv = v . v, ff = F . F: the mixed velocity is a v + b F
__device__ __forceinline__ void fire_mix(double P, double vv, double ff, const mtp_relax_params &p, fire_state &s, double &a,
                                         double &b)
{
  if (P > 0.0) {
    a = 1.0 - s.alpha;
    b = s.alpha * sqrt(vv / ff);
    s.npos += 1;
    if (s.npos > p.n_min) {
      s.dt = fmin(s.dt * p.f_inc, p.dt_max);
      s.alpha *= p.f_alpha;
    }
  } else {
    a = b = 0.0;
    s.npos = 0;
    s.alpha = p.alpha_start;
    if (vv > 0.0) s.dt *= p.f_dec;
  }
}

// the time step of the move: dt, cut so that no component moves further than dmax (vmax = the largest |a v + b F|)
__device__ __forceinline__ double fire_step(double dt, double vmax, const mtp_relax_params &p)
{
  double dtv = dt;
  if (dtv * vmax > p.dmax) dtv = p.dmax / vmax;
  return dtv;
}

// The row sweeps of the fixed-cell users over rows [r0, r1), thread t of NT (F = f, or the band's F_neb).  What this thread
// finds of vmax:
template <int NT>
__device__ __forceinline__ double fire_rows_vmax(int t, int r0, int r1, double a, double b, const double *v, const double *f)
{
  double vmax = 0.0;
  for (int r = r0 + t; r < r1; r += NT) {
#pragma unroll
    for (int c = 0; c < 3; c++) vmax = fmax(vmax, fabs(a * v[3 * (size_t) r + c] + b * f[3 * (size_t) r + c]));
  }
  return vmax;
}

// the move: x += dtv vm, v = vm + kick F with vm = a v + b F computed again rather than staged
template <int NT>
__device__ __forceinline__ void fire_rows_move(int t, int r0, int r1, double a, double b, double dtv, double *x, double *v,
                                               const double *f, const int *type, const double *inv_mass)
{
  for (int r = r0 + t; r < r1; r += NT) {
    const double kick = (dtv * FTM2V) * inv_mass[type[r] - 1];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double fc = f[3 * (size_t) r + c];
      const double vm = a * v[3 * (size_t) r + c] + b * fc;
      x[3 * (size_t) r + c] += dtv * vm;
      v[3 * (size_t) r + c] = vm + kick * fc;
    }
  }
}

// 3 x 3 matrices of a cell, row-major [3 a + b] (the two kernels that move cells: mtp_relax_cell.hip, mtp_sample_cell.hip)
__device__ __forceinline__ double det3(const double *m)
{
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// inv = m^-1 (cofactors over the determinant)
__device__ __forceinline__ void inv3(const double *m, double det, double *inv)
{
  inv[0] = (m[4] * m[8] - m[5] * m[7]) / det;
  inv[1] = (m[2] * m[7] - m[1] * m[8]) / det;
  inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  inv[3] = (m[5] * m[6] - m[3] * m[8]) / det;
  inv[4] = (m[0] * m[8] - m[2] * m[6]) / det;
  inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  inv[6] = (m[3] * m[7] - m[4] * m[6]) / det;
  inv[7] = (m[1] * m[6] - m[0] * m[7]) / det;
  inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}

// c = a . b
__device__ __forceinline__ void mul3(const double *a, const double *b, double *c)
{
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// sum_a (nimg_a + 1) |h_a - href_a| over the rows of a cell: the list-validity measure of a moving cell (mtp_relax_cell_step, 8.)
__device__ __forceinline__ double cell_move(const double *h, const double *href, const int *nimg)
{
  double move = 0.0;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double d0 = h[3 * r] - href[3 * r], d1 = h[3 * r + 1] - href[3 * r + 1], d2 = h[3 * r + 2] - href[3 * r + 2];
    move += (double) (nimg[r] + 1) * sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  }
  return move;
}

// The host side of an entry point.
inline bool in_range(const mtp_relax_params &p)
{
  const double all[7] = {p.ftol, p.dt_max, p.dmax, p.f_inc, p.f_dec, p.alpha_start, p.f_alpha};
  for (double q : all)
    if (!std::isfinite(q)) return false;
  return p.ftol >= 0.0 && p.dt_max > 0.0 && p.dmax > 0.0 && p.f_inc >= 1.0 && p.f_dec > 0.0 && p.f_dec < 1.0 &&
      p.alpha_start >= 0.0 && p.alpha_start <= 1.0 && p.f_alpha > 0.0 && p.f_alpha <= 1.0 && p.n_min >= 0;
}

// is any of these pointers null (the arrays an entry point needs: checked before anything is launched)
inline bool any_null(std::initializer_list<const void *> ptrs)
{
  for (const void *q : ptrs)
    if (!q) return true;
  return false;
}

// the launch epilogue
inline int launched() { return hipGetLastError() == hipSuccess ? MTP_OK : MTP_ERR_DEVICE; }

}   // namespace batch_step
