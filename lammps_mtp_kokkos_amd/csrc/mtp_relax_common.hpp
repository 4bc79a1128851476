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

inline bool in_range(const mtp_relax_params &p)
{
  const double all[7] = {p.ftol, p.dt_max, p.dmax, p.f_inc, p.f_dec, p.alpha_start, p.f_alpha};
  for (double q : all)
    if (!std::isfinite(q)) return false;
  return p.ftol >= 0.0 && p.dt_max > 0.0 && p.dmax > 0.0 && p.f_inc >= 1.0 && p.f_dec > 0.0 && p.f_dec < 1.0 &&
      p.alpha_start >= 0.0 && p.alpha_start <= 1.0 && p.f_alpha > 0.0 && p.f_alpha <= 1.0 && p.n_min >= 0;
}

}   // namespace relax_common
