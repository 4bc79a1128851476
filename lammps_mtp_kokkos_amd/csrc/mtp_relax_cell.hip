// Batched variable-cell relaxation (include/mtp_mi355x.h, "batched variable-cell relaxation"): mtp_relax_step with the cell
// among the degrees of freedom.  The layout, the wavefront / workgroup split, the fixed-order reductions and the FIRE rule are
// the family's (mtp_batch_step.hpp); the 3 x 3 quantities of a configuration -- D, h = h0 . D, W', G, the new D -- are
// computed by every thread that serves it, from the same inputs in the same order, so that every branch is taken by all of
// them together and nothing is staged.  Matrices are row-major [3 a + b]; vectors are rows (x = s . h).
#include "mtp_batch_step.hpp"

namespace {

using namespace batch_step;

// One configuration, served by thread t of NT.  Everything per configuration is read before the first reduction (in the
// workgroup's case: before its first barrier), and thread 0 writes it back after the last one.  The row sweeps are this
// kernel's own: the forces are transformed by D inside them.
template <int NT>
__device__ __forceinline__ void relax_cell_configuration(int t, int k, int r0, int r1, const mtp_relax_cell_params &p, int step,
                                                         int last, const mtp_relax_cell_arrays &A, double *part)
{
  const mtp_relax_params &fp = p.fire;
  double D[9], vq[9], h[9], Wp[9], G[9], Dinv[9], w6[6];
#pragma unroll
  for (int q = 0; q < 9; q++) {
    D[q] = A.D[9 * (size_t) k + q];
    vq[q] = A.vq[9 * (size_t) k + q];
  }
#pragma unroll
  for (int q = 0; q < 6; q++) w6[q] = A.virial[6 * (size_t) k + q];
  const double org[3] = {A.origins[3 * (size_t) k], A.origins[3 * (size_t) k + 1], A.origins[3 * (size_t) k + 2]};
  const double L = p.factor_per_atom ? p.cell_factor * (double) (r1 - r0) : p.cell_factor;
  mul3(A.h0 + 9 * (size_t) k, D, h);
  const double V = det3(h), detD = det3(D);
  {
    const double pv = p.pressure * V;
    const int *m = p.cell_mask;
    Wp[0] = m[0] ? w6[0] - pv : 0.0;
    Wp[4] = m[1] ? w6[1] - pv : 0.0;
    Wp[8] = m[2] ? w6[2] - pv : 0.0;
    Wp[1] = Wp[3] = m[3] ? w6[3] : 0.0;
    Wp[2] = Wp[6] = m[4] ? w6[4] : 0.0;
    Wp[5] = Wp[7] = m[5] ? w6[5] : 0.0;
    if (p.isotropic) {
      const double tr = (Wp[0] + Wp[4] + Wp[8]) / 3.0;
      Wp[0] = Wp[4] = Wp[8] = tr;
      Wp[1] = Wp[2] = Wp[3] = Wp[5] = Wp[6] = Wp[7] = 0.0;
    }
  }
  inv3(D, detD, Dinv);
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) G[3 * a + b] = (Dinv[a] * Wp[b] + Dinv[3 + a] * Wp[3 + b] + Dinv[6 + a] * Wp[6 + b]) / L;

  double P = 0.0, vv = 0.0, ff = 0.0, fmax2 = 0.0;
  for (int r = r0 + t; r < r1; r += NT) {
    const double f0 = A.f[3 * (size_t) r], f1 = A.f[3 * (size_t) r + 1], f2 = A.f[3 * (size_t) r + 2];
    fmax2 = fmax(fmax2, f0 * f0 + f1 * f1 + f2 * f2);
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const double fa = f0 * D[3 * b] + f1 * D[3 * b + 1] + f2 * D[3 * b + 2], va = A.vt[3 * (size_t) r + b];
      P += fa * va;
      vv += va * va;
      ff += fa * fa;
    }
  }
  P = segment_total<NT, false>(P, part);
  vv = segment_total<NT, false>(vv, part);
  ff = segment_total<NT, false>(ff, part);
  fmax2 = segment_total<NT, true>(fmax2, part);
  double smax = 0.0;
#pragma unroll
  for (int q = 0; q < 9; q++) {   // the cell rows, after the atom total
    P += G[q] * vq[q];
    vv += vq[q] * vq[q];
    ff += G[q] * G[q];
    smax = fmax(smax, fabs(Wp[q]));
  }
  smax /= V;
  if (t == 0) {
    A.fmax[k] = sqrt(fmax2);
    A.smax[k] = smax;
#pragma unroll
    for (int q = 0; q < 9; q++) {
      A.gcell[9 * (size_t) k + q] = G[q];
      A.h[9 * (size_t) k + q] = h[q];
    }
  }
  bool failed = !isfinite(ff) || !isfinite(V) || !isfinite(detD) || !(detD > 0.0);
#pragma unroll
  for (int q = 0; q < 6; q++) failed = failed || !isfinite(w6[q]);
  if (failed || (fmax2 <= fp.ftol * fp.ftol && smax <= p.stol)) {
    if (!failed) {
      for (int r = r0 + t; r < r1; r += NT) {
#pragma unroll
        for (int a = 0; a < 3; a++) A.vt[3 * (size_t) r + a] = 0.0;
      }
      if (t == 0) {
#pragma unroll
        for (int q = 0; q < 9; q++) A.vq[9 * (size_t) k + q] = 0.0;
      }
    }
    if (t == 0) {
      A.frozen[k] = failed ? 3 : 2;
      A.done_step[k] = step;
      atomicAdd(&A.counts[2], 1);
    }
    return;
  }
  if (last) return;
  fire_state s = {A.dt[k], A.alpha[k], A.npos[k]};
  double a, b;
  fire_mix(P, vv, ff, fp, s, a, b);
  double vmax = 0.0;
  for (int r = r0 + t; r < r1; r += NT) {
    const double f0 = A.f[3 * (size_t) r], f1 = A.f[3 * (size_t) r + 1], f2 = A.f[3 * (size_t) r + 2];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double fc = f0 * D[3 * c] + f1 * D[3 * c + 1] + f2 * D[3 * c + 2];
      vmax = fmax(vmax, fabs(a * A.vt[3 * (size_t) r + c] + b * fc));
    }
  }
  vmax = segment_total<NT, true>(vmax, part);
#pragma unroll
  for (int q = 0; q < 9; q++) vmax = fmax(vmax, fabs(a * vq[q] + b * G[q]));
  const double dtv = fire_step(s.dt, vmax, fp);
  double Dn[9], vqn[9];
  {
    const double kick = (dtv * FTM2V) / p.cell_mass;
#pragma unroll
    for (int q = 0; q < 9; q++) {
      const double vm = a * vq[q] + b * G[q];
      Dn[q] = D[q] + dtv * vm / L;
      vqn[q] = vm + kick * G[q];
    }
  }
  for (int r = r0 + t; r < r1; r += NT) {
    const double kick = (dtv * FTM2V) * A.inv_mass[A.type[r] - 1];
    const double f0 = A.f[3 * (size_t) r], f1 = A.f[3 * (size_t) r + 1], f2 = A.f[3 * (size_t) r + 2];
    double xn[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double fc = f0 * D[3 * c] + f1 * D[3 * c + 1] + f2 * D[3 * c + 2];   // (the D the forces were taken at)
      const double vm = a * A.vt[3 * (size_t) r + c] + b * fc;
      xn[c] = A.xt[3 * (size_t) r + c] + dtv * vm;
      A.xt[3 * (size_t) r + c] = xn[c];
      A.vt[3 * (size_t) r + c] = vm + kick * fc;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) A.x[3 * (size_t) r + c] = org[c] + (xn[0] * Dn[c] + xn[1] * Dn[3 + c] + xn[2] * Dn[6 + c]);
  }
  if (t == 0) {
    double hn[9], T[9];
    mul3(A.h0 + 9 * (size_t) k, Dn, hn);
    mul3(A.Dbinv + 9 * (size_t) k, Dn, T);
    A.dt[k] = s.dt;
    A.alpha[k] = s.alpha;
    A.npos[k] = s.npos;
    A.cellmove[k] = cell_move(hn, A.href + 9 * (size_t) k, A.nimg + 3 * (size_t) k);
#pragma unroll
    for (int q = 0; q < 9; q++) {
      A.D[9 * (size_t) k + q] = Dn[q];
      A.vq[9 * (size_t) k + q] = vqn[q];
      A.h[9 * (size_t) k + q] = hn[q];
      A.T[9 * (size_t) k + q] = T[q];
    }
  }
}

// for_each_live_segment's split (mtp_batch_step.hpp)
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) relax_cell_step_kernel(int ncfg, mtp_relax_cell_params p, int step, int last,
                                                                         mtp_relax_cell_arrays A)
{
  __shared__ double part[BATCH_WAVES];
  for_each_live_segment(ncfg, A.cfg_first, A.frozen, [&](auto nt, int t, int k, int r0, int r1) {
    relax_cell_configuration<decltype(nt)::value>(t, k, r0, r1, p, step, last, A, part);
  });
}

// xt = (x - origin) . D^-1 per owned row (one lane a row); the first row of a configuration also leaves Dbinv = D^-1
__global__ void __launch_bounds__(256) relax_cell_rebase_kernel(int nrows, const int *__restrict__ row_cfg,
                                                               const double *__restrict__ origins, const double *__restrict__ x,
                                                               const double *__restrict__ Dall, double *__restrict__ xt,
                                                               double *__restrict__ Dbinv)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nrows) return;
  const int k = row_cfg[i];
  double D[9], inv[9];
#pragma unroll
  for (int q = 0; q < 9; q++) D[q] = Dall[9 * (size_t) k + q];
  const double det = det3(D);
  if (!(det > 0.0) || !isfinite(det)) return;
  inv3(D, det, inv);
  const double d0 = x[3 * (size_t) i] - origins[3 * (size_t) k], d1 = x[3 * (size_t) i + 1] - origins[3 * (size_t) k + 1],
               d2 = x[3 * (size_t) i + 2] - origins[3 * (size_t) k + 2];
#pragma unroll
  for (int c = 0; c < 3; c++) xt[3 * (size_t) i + c] = d0 * inv[c] + d1 * inv[3 + c] + d2 * inv[6 + c];
  if (i == 0 || row_cfg[i - 1] != k) {
#pragma unroll
    for (int q = 0; q < 9; q++) Dbinv[9 * (size_t) k + q] = inv[q];
  }
}

__global__ void __launch_bounds__(256) relax_cell_capture_cells_kernel(int ncfg, const int *__restrict__ slot, int max_candidates,
                                                                      const double *__restrict__ h, double *__restrict__ cand_cell)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 9 * ncfg) return;
  const int k = e / 9, s = slot[k];
  if (s < 0 || s >= max_candidates) return;
  cand_cell[9 * (size_t) s + (e - 9 * k)] = h[e];
}

bool cell_in_range(const mtp_relax_cell_params &p)
{
  if (!in_range(p.fire)) return false;
  if (!std::isfinite(p.stol) || !std::isfinite(p.pressure) || !std::isfinite(p.cell_factor) || !std::isfinite(p.cell_mass)) return false;
  for (int m : p.cell_mask)
    if (m != 0 && m != 1) return false;
  return p.stol >= 0.0 && p.cell_factor > 0.0 && p.cell_mass > 0.0;
}

}   // namespace

extern "C" {

int mtp_relax_cell_step(void *stream, int ncfg, const mtp_relax_cell_params *params, int step, int last,
                        const mtp_relax_cell_arrays *arrays)
{
  if (!stream || ncfg < 0 || step < 0 || !params || !cell_in_range(*params)) return MTP_ERR_ARG;
  if (ncfg > 0) {
    if (!arrays) return MTP_ERR_ARG;
    const mtp_relax_cell_arrays &A = *arrays;
    if (any_null({A.cfg_first, A.x, A.xt, A.vt, A.f, A.type, A.inv_mass, A.virial, A.h0, A.origins, A.D, A.vq, A.Dbinv, A.href,
                  A.nimg, A.dt, A.alpha, A.npos, A.frozen, A.done_step, A.fmax, A.smax, A.gcell, A.h, A.T, A.cellmove, A.counts}))
      return MTP_ERR_ARG;
  }
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(relax_cell_step_kernel, dim3((ncfg + BATCH_WAVES - 1) / BATCH_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, *params, step, last ? 1 : 0, *arrays);
  return launched();
}

int mtp_relax_cell_rebase(void *stream, int ncfg, int nrows, const int *d_row_cfg, const double *d_origins, const double *d_x,
                          const double *d_D, double *d_xt, double *d_Dbinv)
{
  if (!stream || ncfg < 0 || nrows < 0 || (nrows > 0 && (ncfg == 0 || !d_row_cfg || !d_origins || !d_x || !d_D || !d_xt || !d_Dbinv)))
    return MTP_ERR_ARG;
  if (nrows == 0) return MTP_OK;
  hipLaunchKernelGGL(relax_cell_rebase_kernel, dim3((nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), nrows,
                     d_row_cfg, d_origins, d_x, d_D, d_xt, d_Dbinv);
  return launched();
}

int mtp_relax_cell_capture_cells(void *stream, int ncfg, const int *d_slot, int max_candidates, const double *d_h,
                                 double *d_cand_cell)
{
  if (!stream || ncfg < 0 || max_candidates < 0 || (ncfg > 0 && (!d_slot || !d_h || (max_candidates > 0 && !d_cand_cell))))
    return MTP_ERR_ARG;
  if (ncfg == 0 || max_candidates == 0) return MTP_OK;
  hipLaunchKernelGGL(relax_cell_capture_cells_kernel, dim3((9 * ncfg + 255) / 256), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, d_slot, max_candidates, d_h, d_cand_cell);
  return launched();
}

}   // extern "C"
