// Batched force constants (include/mtp_mi355x.h, "batched force constants"): the Hessian of every configuration of a batch in
// the layout of the batched configurations, by central differences of the forces.  A displacement of a hundredth of an
// angstrom is far inside the skin, so ONE ghost build and ONE list serve every force call of a pass; between two force calls
// ONE launch (mtp_hess_step) harvests the forces of the displacement just made into its row of H, puts the moved coordinate
// back from the saved copy and makes the next displacement -- nothing is read back.  ONE launch a pass (mtp_hess_finish)
// measures the asymmetry and the translation sum rule, symmetrises and, if asked, mass-weights.  No context, no handle: every
// array is the caller's, and the entry points take the stream and reject NULL (the rule of mtp_relax_step).  The reductions,
// the split of a workgroup over the configurations and the entry-point checks are the family's: mtp_batch_step.hpp.
#include "mtp_batch_step.hpp"

// every expression below is evaluated as written (no fused multiply-add): tests/_hess.py follows them bit for bit
#pragma clang fp contract(off)

namespace {

using namespace batch_step;

// Launch k of a pass for one configuration j, rows [r0, r1), served by thread t of NT (all of them take every branch together:
// each decision is made from totals that are the same in all, or from k and the configuration's own sizes).
template <int NT>
__device__ __forceinline__ void hess_configuration(int t, int j, int r0, int r1, const int *__restrict__ sel_first,
                                                   const int *__restrict__ sel, int sel_max, int k, double h, double inv2h,
                                                   double *__restrict__ x, const double *__restrict__ x0,
                                                   const double *__restrict__ f, const double *__restrict__ eatom,
                                                   const long long *__restrict__ h_first, double *__restrict__ H,
                                                   double *__restrict__ f0, double *__restrict__ d_fmax,
                                                   double *__restrict__ d_energy, int *d_status, double *part)
{
  const int s0 = sel_first[j], m = sel_first[j + 1] - s0;
  if (k == 0) {
    // 1. the forces at the undisplaced positions, the largest of them, the energy; a selection that is not rows of this
    // configuration fails it like a force that is not finite
    double bad = (m < 0 || m > r1 - r0 || m > sel_max) ? 1.0 : 0.0;
    if (bad == 0.0)
      for (int i = t; i < m; i += NT) {
        const int row = sel[s0 + i];
        if (row < r0 || row >= r1) bad = 1.0;
      }
    double fmax2 = 0.0, e = 0.0;
    for (int r = r0 + t; r < r1; r += NT) {
      double f2 = 0.0;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double fa = f[3 * (size_t) r + a];
        f0[3 * (size_t) r + a] = fa;
        f2 += fa * fa;
        if (!isfinite(fa)) bad = 1.0;
      }
      fmax2 = fmax(fmax2, f2);
      e += eatom[r];
    }
    bad = segment_total<NT, true>(bad, part);
    fmax2 = segment_total<NT, true>(fmax2, part);
    e = segment_total<NT, false>(e, part);
    if (t == 0) {
      d_fmax[j] = sqrt(fmax2);
      d_energy[j] = e;
    }
    if (bad != 0.0) {
      if (t == 0) d_status[j] = MTP_HESS_FAILED;
      return;
    }
  } else {
    // 2. harvest displacement k - 1 into row c of H, then 3. put the moved coordinate back from the saved copy
    const int a = (k - 1) / 6, d = ((k - 1) % 6) / 2, minus = (k - 1) & 1;
    if (a < m) {
      const int N = 3 * m;
      double *Hc = H + h_first[j] + (size_t) (3 * a + d) * N;
      double bad = 0.0;
      for (int i = t; i < N; i += NT)
        if (!isfinite(f[3 * (size_t) sel[s0 + i / 3] + i % 3])) bad = 1.0;
      bad = segment_total<NT, true>(bad, part);
      if (bad == 0.0)
        for (int i = t; i < N; i += NT) {
          const double fi = f[3 * (size_t) sel[s0 + i / 3] + i % 3];
          Hc[i] = minus ? (fi - Hc[i]) * inv2h : fi;   // after + h the row is parked, after - h it is (f- - f+) / (2 h)
        }
      if (t == 0) {
        const size_t q = 3 * (size_t) sel[s0 + a] + d;
        x[q] = x0[q];
        if (bad != 0.0) d_status[j] = MTP_HESS_FAILED;
      }
      if (bad != 0.0) return;
    }
  }
  // 4. displacement k
  if (k < 6 * sel_max && k / 6 < m && t == 0) {
    const size_t q = 3 * (size_t) sel[s0 + k / 6] + (k % 6) / 2;
    x[q] = (k & 1) ? x0[q] - h : x0[q] + h;
  }
}

// for_each_live_segment's split (mtp_batch_step.hpp) over the rows of the configurations; a failed configuration is skipped
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) hess_step_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                                   const int *__restrict__ sel_first,
                                                                   const int *__restrict__ sel, int sel_max, int k, double h,
                                                                   double inv2h, double *__restrict__ x,
                                                                   const double *__restrict__ x0, const double *__restrict__ f,
                                                                   const double *__restrict__ eatom,
                                                                   const long long *__restrict__ h_first, double *__restrict__ H,
                                                                   double *__restrict__ f0, double *__restrict__ d_fmax,
                                                                   double *__restrict__ d_energy, int *d_status)
{
  __shared__ double part[BATCH_WAVES];
  for_each_live_segment(ncfg, cfg_first, d_status, [&](auto nt, int t, int j, int r0, int r1) {
    hess_configuration<decltype(nt)::value>(t, j, r0, r1, sel_first, sel, sel_max, k, h, inv2h, x, x0, f, eatom, h_first, H, f0, d_fmax,
                                            d_energy, d_status, part);
  });
}

// The end of a pass for one configuration: its selection is entries [s0, s1) of sel, H_j is [3 m][3 m].  The two diagnostics
// are taken from the matrix as harvested and only then is the matrix rewritten: the totals in between are a barrier (every
// thread's reads are in before any thread writes), and a pair (c, r) is read once, by the thread that writes both its members.
template <int NT>
__device__ __forceinline__ void finish_configuration(int t, int j, int s0, int s1, const int *__restrict__ sel,
                                                     const int *__restrict__ type, const double *__restrict__ mass,
                                                     int mass_weight, const long long *__restrict__ h_first,
                                                     double *__restrict__ H, double *__restrict__ diag, double *part)
{
  const int m = s1 - s0, N = 3 * m;
  double *Hj = H + h_first[j];
  double asym = 0.0, rule = 0.0;
  for (int c = 0; c < N; c++)
    for (int r = c + 1 + t; r < N; r += NT) asym = fmax(asym, fabs(Hj[(size_t) c * N + r] - Hj[(size_t) r * N + c]));
  for (int i = t; i < 3 * N; i += NT) {   // (c, e): the sum over the responding atoms b, in their order
    const int c = i / 3, e = i % 3;
    double s = 0.0;
    for (int b = 0; b < m; b++) s += Hj[(size_t) c * N + 3 * b + e];
    rule = fmax(rule, fabs(s));
  }
  asym = segment_total<NT, true>(asym, part);
  rule = segment_total<NT, true>(rule, part);
  if (t == 0) {
    diag[2 * (size_t) j] = asym;
    diag[2 * (size_t) j + 1] = rule;
  }
  for (int c = 0; c < N; c++) {
    const double mc = mass_weight ? mass[type[sel[s0 + c / 3]] - 1] : 1.0;
    for (int r = c + t; r < N; r += NT) {
      double s = 0.5 * (Hj[(size_t) c * N + r] + Hj[(size_t) r * N + c]);
      if (mass_weight) s *= 1.0 / sqrt(mc * mass[type[sel[s0 + r / 3]] - 1]);
      Hj[(size_t) c * N + r] = s;
      Hj[(size_t) r * N + c] = s;
    }
  }
}

// the same split over the SELECTIONS: a wavefront for up to MTP_BATCH_WAVE_ROWS selected atoms, the workgroup for more
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) hess_finish_kernel(int ncfg, const int *__restrict__ sel_first,
                                                                     const int *__restrict__ sel, const int *__restrict__ type,
                                                                     const double *__restrict__ mass, int mass_weight,
                                                                     const long long *__restrict__ h_first,
                                                                     double *__restrict__ H, double *__restrict__ diag,
                                                                     const int *d_status)
{
  __shared__ double part[BATCH_WAVES];
  for_each_live_segment(ncfg, sel_first, d_status, [&](auto nt, int t, int j, int s0, int s1) {
    finish_configuration<decltype(nt)::value>(t, j, s0, s1, sel, type, mass, mass_weight, h_first, H, diag, part);
  });
}

}   // namespace

extern "C" {

int mtp_hess_step(void *stream, int ncfg, const int *d_cfg_first, const int *d_sel_first, const int *d_sel, int sel_max, int k,
                  double h, double *d_x, const double *d_x0, const double *d_f, const double *d_eatom, const long long *d_h_first,
                  double *d_H, double *d_f0, double *d_fmax, double *d_energy, int *d_status)
{
  if (!stream || ncfg < 0 || sel_max < 0 || sel_max > MTP_HESS_MAX_SELECTED || k < 0 || k > 6 * sel_max || !std::isfinite(h) ||
      !(h > 0.0) ||
      (ncfg > 0 &&
       any_null({d_cfg_first, d_sel_first, d_sel, d_x, d_x0, d_f, d_eatom, d_h_first, d_H, d_f0, d_fmax, d_energy, d_status})))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(hess_step_kernel, dim3((ncfg + BATCH_WAVES - 1) / BATCH_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, d_cfg_first, d_sel_first, d_sel, sel_max, k, h, 1.0 / (2.0 * h),
                     d_x, d_x0, d_f, d_eatom, d_h_first, d_H, d_f0, d_fmax, d_energy, d_status);
  return launched();
}

int mtp_hess_finish(void *stream, int ncfg, const int *d_sel_first, const int *d_sel, const int *d_type, const double *d_mass,
                    int mass_weight, const long long *d_h_first, double *d_H, double *d_diag, const int *d_status)
{
  if (!stream || ncfg < 0 || (ncfg > 0 && any_null({d_sel_first, d_sel, d_type, d_mass, d_h_first, d_H, d_diag, d_status})))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(hess_finish_kernel, dim3((ncfg + BATCH_WAVES - 1) / BATCH_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, d_sel_first, d_sel, d_type, d_mass, mass_weight ? 1 : 0, d_h_first,
                     d_H, d_diag, d_status);
  return launched();
}

}   // extern "C"
