// Batched relaxation (include/mtp_mi355x.h, "batched relaxation"): the FIRE minimiser over a batch of independent periodic
// cells in the layout of the batched configurations -- owned rows of configuration k are [cfg_first[k], cfg_first[k + 1]) of
// every per-atom array, positions in slot coordinates between re-neighbourings.  ONE launch a step, after the force call and
// the ghost fold: the per-configuration reductions, the FIRE state machine, the convergence decision and the move, so that
// nothing is read back between re-neighbourings.  No context, no handle: every array is the caller's, and the entry point
// takes the stream and rejects NULL (the rule of mtp_sample_*).
#include "mtp_relax_common.hpp"

namespace {

using namespace relax_common;   // the reductions and the parameter check, shared with mtp_relax_cell.hip

// One configuration, served by thread t of NT (all of them take every branch together: each decision is made from totals
// that are the same in all).  Rows are read one per thread, consecutive threads consecutive rows; v' = a v + b f is computed
// again in the last sweep rather than staged.
template <int NT>
__device__ __forceinline__ void relax_configuration(int t, int k, int r0, int r1, const mtp_relax_params &p, int step, int last,
                                                    double *__restrict__ x, double *__restrict__ v,
                                                    const double *__restrict__ f, const int *__restrict__ type,
                                                    const double *__restrict__ inv_mass, double *__restrict__ d_dt,
                                                    double *__restrict__ d_alpha, int *__restrict__ d_npos, int *d_frozen,
                                                    int *__restrict__ d_done_step, double *__restrict__ d_fmax,
                                                    int *__restrict__ d_counts, double *part)
{
  double P = 0.0, vv = 0.0, ff = 0.0, fmax2 = 0.0;
  for (int r = r0 + t; r < r1; r += NT) {
    double f2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double fa = f[3 * (size_t) r + a], va = v[3 * (size_t) r + a];
      P += fa * va;
      vv += va * va;
      f2 += fa * fa;
    }
    ff += f2;
    fmax2 = fmax(fmax2, f2);
  }
  P = relax_total<NT, false>(P, part);
  vv = relax_total<NT, false>(vv, part);
  ff = relax_total<NT, false>(ff, part);
  fmax2 = relax_total<NT, true>(fmax2, part);
  if (t == 0) d_fmax[k] = sqrt(fmax2);
  const bool failed = !isfinite(ff);
  if (failed || fmax2 <= p.ftol * p.ftol) {
    if (!failed)
      for (int r = r0 + t; r < r1; r += NT) {
#pragma unroll
        for (int a = 0; a < 3; a++) v[3 * (size_t) r + a] = 0.0;
      }
    if (t == 0) {
      d_frozen[k] = failed ? 3 : 2;
      d_done_step[k] = step;
      atomicAdd(&d_counts[2], 1);
    }
    return;
  }
  if (last) return;
  double dt = d_dt[k], alpha = d_alpha[k], a, b;
  int npos = d_npos[k];
  if (P > 0.0) {
    a = 1.0 - alpha;
    b = alpha * sqrt(vv / ff);
    npos += 1;
    if (npos > p.n_min) {
      dt = fmin(dt * p.f_inc, p.dt_max);
      alpha *= p.f_alpha;
    }
  } else {
    a = b = 0.0;
    npos = 0;
    alpha = p.alpha_start;
    if (vv > 0.0) dt *= p.f_dec;
  }
  double vmax = 0.0;
  for (int r = r0 + t; r < r1; r += NT) {
#pragma unroll
    for (int c = 0; c < 3; c++) vmax = fmax(vmax, fabs(a * v[3 * (size_t) r + c] + b * f[3 * (size_t) r + c]));
  }
  vmax = relax_total<NT, true>(vmax, part);
  double dtv = dt;
  if (dtv * vmax > p.dmax) dtv = p.dmax / vmax;
  for (int r = r0 + t; r < r1; r += NT) {
    const double kick = (dtv * RELAX_FTM2V) * inv_mass[type[r] - 1];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double fc = f[3 * (size_t) r + c];
      const double vm = a * v[3 * (size_t) r + c] + b * fc;
      x[3 * (size_t) r + c] += dtv * vm;
      v[3 * (size_t) r + c] = vm + kick * fc;
    }
  }
  if (t == 0) {
    d_dt[k] = dt;
    d_alpha[k] = alpha;
    d_npos[k] = npos;
  }
}

// The layout of sample_monitor_kernel / mtp_batch_reduce_kernel: a workgroup of four wavefronts owns four consecutive
// configurations, one wavefront each for segments of up to MTP_BATCH_WAVE_ROWS rows, the whole workgroup, one after another,
// for the longer ones.  Empty and frozen configurations are skipped: nothing of theirs is written.  The one atomic is the
// integer count of frozen configurations; the order of every floating-point sum depends on the segment's length alone.
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) relax_step_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                                    mtp_relax_params p, int step, int last,
                                                                    double *__restrict__ x, double *__restrict__ v,
                                                                    const double *__restrict__ f, const int *__restrict__ type,
                                                                    const double *__restrict__ inv_mass,
                                                                    double *__restrict__ d_dt, double *__restrict__ d_alpha,
                                                                    int *__restrict__ d_npos, int *d_frozen,
                                                                    int *__restrict__ d_done_step, double *__restrict__ d_fmax,
                                                                    int *__restrict__ d_counts)
{
  __shared__ double part[RELAX_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = blockIdx.x * RELAX_WAVES;
  if (k0 + wave < ncfg) {   // (the whole wavefront)
    const int k = k0 + wave, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 > r0 && r1 - r0 <= MTP_BATCH_WAVE_ROWS && d_frozen[k] == 0)
      relax_configuration<64>(lane, k, r0, r1, p, step, last, x, v, f, type, inv_mass, d_dt, d_alpha, d_npos, d_frozen,
                              d_done_step, d_fmax, d_counts, part);
  }
  for (int w = 0; w < RELAX_WAVES && k0 + w < ncfg; w++) {   // (the whole workgroup)
    const int k = k0 + w, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 - r0 <= MTP_BATCH_WAVE_ROWS) continue;
    const int fr = d_frozen[k];
    __syncthreads();   // every thread has read the flag before thread 0 may set it
    if (fr == 0)
      relax_configuration<MTP_BATCH_BLOCK>(threadIdx.x, k, r0, r1, p, step, last, x, v, f, type, inv_mass, d_dt, d_alpha, d_npos,
                                           d_frozen, d_done_step, d_fmax, d_counts, part);
  }
}

}   // namespace

extern "C" {

int mtp_relax_step(void *stream, int ncfg, const int *d_cfg_first, const mtp_relax_params *params, int step, int last,
                   double *d_x, double *d_v, const double *d_f, const int *d_type, const double *d_inv_mass, double *d_dt,
                   double *d_alpha, int *d_npos, int *d_frozen, int *d_done_step, double *d_fmax, int *d_counts)
{
  if (!stream || ncfg < 0 || step < 0 || !params || !in_range(*params) ||
      (ncfg > 0 && (!d_cfg_first || !d_x || !d_v || !d_f || !d_type || !d_inv_mass || !d_dt || !d_alpha || !d_npos ||
                    !d_frozen || !d_done_step || !d_fmax || !d_counts)))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(relax_step_kernel, dim3((ncfg + RELAX_WAVES - 1) / RELAX_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, d_cfg_first, *params, step, last ? 1 : 0, d_x, d_v, d_f, d_type,
                     d_inv_mass, d_dt, d_alpha, d_npos, d_frozen, d_done_step, d_fmax, d_counts);
  return hipGetLastError() == hipSuccess ? MTP_OK : MTP_ERR_DEVICE;
}

}   // extern "C"
