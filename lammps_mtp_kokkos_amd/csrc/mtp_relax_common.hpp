// What the two batched minimisers share (mtp_relax.hip: fixed cells; mtp_relax_cell.hip: cells that relax with the atoms):
// the unit constant, the fixed-order reductions over a wavefront or a workgroup of MTP_BATCH_BLOCK threads, and the range
// check of the FIRE parameters.  Device code is inlined into each kernel: the fixed-cell kernel has the code it always had.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mtp_mi355x.h"
#include "mtp_device.hpp"

namespace relax_common {

constexpr double RELAX_FTM2V = 1.0 / 1.0364269e-4;   // LAMMPS metal units (update.cpp), as mtp_sample.hip

constexpr int RELAX_WAVES = MTP_BATCH_BLOCK / 64;

// the wavefront reductions of mtp_sample.hip: xor butterfly, a fixed order, the same bits in every lane
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
__device__ __forceinline__ double relax_total(double val, double *part)
{
  val = MAX ? wave_max64(val) : wave_sum64(val);
  if (NT == 64) return val;
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = val;
  __syncthreads();
  double t = part[0];
#pragma unroll
  for (int u = 1; u < RELAX_WAVES; u++) t = MAX ? fmax(t, part[u]) : t + part[u];
  __syncthreads();
  return t;
}

// 3 x 3 matrices of a cell, row-major [3 a + b] (the two kernels that move cells: mtp_relax_cell.hip, mtp_sample_cell.hip)
__device__ __forceinline__ double det3(const double *m)
{
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
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

inline bool in_range(const mtp_relax_params &p)
{
  const double all[7] = {p.ftol, p.dt_max, p.dmax, p.f_inc, p.f_dec, p.alpha_start, p.f_alpha};
  for (double q : all)
    if (!std::isfinite(q)) return false;
  return p.ftol >= 0.0 && p.dt_max > 0.0 && p.dmax > 0.0 && p.f_inc >= 1.0 && p.f_dec > 0.0 && p.f_dec < 1.0 &&
      p.alpha_start >= 0.0 && p.alpha_start <= 1.0 && p.f_alpha > 0.0 && p.f_alpha <= 1.0 && p.n_min >= 0;
}

}   // namespace relax_common
