// Batched relaxation (include/mtp_mi355x.h, "batched relaxation"): the FIRE minimiser over a batch of independent periodic
// cells in the layout of the batched configurations -- owned rows of configuration k are [cfg_first[k], cfg_first[k + 1]) of
// every per-atom array, positions in slot coordinates between re-neighbourings.  ONE launch a step, after the force call and
// the ghost fold: the per-configuration reductions, the FIRE state machine, the convergence decision and the move, so that
// nothing is read back between re-neighbourings.  No context, no handle: every array is the caller's, and the entry point
// takes the stream and rejects NULL (the rule of mtp_sample_*).  The FIRE rule, its row sweeps, the reductions and the split of a
// workgroup over the configurations are the family's: mtp_batch_step.hpp.
#include "mtp_batch_step.hpp"

namespace {

using namespace batch_step;

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
  P = segment_total<NT, false>(P, part);
  vv = segment_total<NT, false>(vv, part);
  ff = segment_total<NT, false>(ff, part);
  fmax2 = segment_total<NT, true>(fmax2, part);
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
  fire_state s = {d_dt[k], d_alpha[k], d_npos[k]};
  double a, b;
  fire_mix(P, vv, ff, p, s, a, b);
  const double vmax = segment_total<NT, true>(fire_rows_vmax<NT>(t, r0, r1, a, b, v, f), part);
  fire_rows_move<NT>(t, r0, r1, a, b, fire_step(s.dt, vmax, p), x, v, f, type, inv_mass);
  if (t == 0) {
    d_dt[k] = s.dt;
    d_alpha[k] = s.alpha;
    d_npos[k] = s.npos;
  }
}

// for_each_live_segment's split (mtp_batch_step.hpp).  The one atomic is the integer count of frozen configurations.
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
  __shared__ double part[BATCH_WAVES];
  for_each_live_segment(ncfg, cfg_first, d_frozen, [&](auto nt, int t, int k, int r0, int r1) {
    relax_configuration<decltype(nt)::value>(t, k, r0, r1, p, step, last, x, v, f, type, inv_mass, d_dt, d_alpha, d_npos, d_frozen,
                                             d_done_step, d_fmax, d_counts, part);
  });
}

}   // namespace

extern "C" {

int mtp_relax_step(void *stream, int ncfg, const int *d_cfg_first, const mtp_relax_params *params, int step, int last,
                   double *d_x, double *d_v, const double *d_f, const int *d_type, const double *d_inv_mass, double *d_dt,
                   double *d_alpha, int *d_npos, int *d_frozen, int *d_done_step, double *d_fmax, int *d_counts)
{
  if (!stream || ncfg < 0 || step < 0 || !params || !in_range(*params) ||
      (ncfg > 0 && any_null({d_cfg_first, d_x, d_v, d_f, d_type, d_inv_mass, d_dt, d_alpha, d_npos, d_frozen, d_done_step, d_fmax,
                             d_counts})))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(relax_step_kernel, dim3((ncfg + BATCH_WAVES - 1) / BATCH_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, d_cfg_first, *params, step, last ? 1 : 0, d_x, d_v, d_f, d_type,
                     d_inv_mass, d_dt, d_alpha, d_npos, d_frozen, d_done_step, d_fmax, d_counts);
  return launched();
}

}   // extern "C"
