// Batched elastic constants (include/mtp_mi355x.h, "batched elastic constants"): the second derivatives of every configuration of
// a batch with respect to its CELL, by central differences of the stress and of the forces over twelve homogeneous strains
// x -> x (I +- h E_w).  A strain of half a percent is far inside the skin, so ONE ghost build and ONE list serve the thirteen
// force calls of a pass; between two force calls ONE launch (mtp_elastic_step) harvests the stress and the forces of the strain
// just made into their rows, and lays the atoms and the ghost transform T out for the next strain -- nothing is read back.  ONE
// launch a pass (mtp_elastic_finish) turns the stress-strain coefficients into elastic constants, and ONE more, if asked
// (mtp_elastic_relax), solves for the internal-strain displacements with the Hessian of mtp_hess_step in LDS.  No context, no
// handle: every array is the caller's, and the entry points take the stream and reject NULL (the rule of mtp_relax_step).  The
// reductions, the split of a workgroup over the configurations and the entry-point checks are the family's: mtp_batch_step.hpp.
#include "mtp_batch_step.hpp"

// every expression below is evaluated as written (no fused multiply-add): tests/_elastic.py follows them bit for bit
#pragma clang fp contract(off)

namespace {

using namespace batch_step;

// the two indices (a, b), a <= b, of component w in the project's order xx yy zz xy xz yz
__device__ __forceinline__ int comp_a(int w) { return w < 3 ? w : (w == 5 ? 1 : 0); }
__device__ __forceinline__ int comp_b(int w) { return w < 3 ? w : (w == 3 ? 1 : 2); }

// D = I + s E_w, row-major [9]: a 1 on the diagonal for w < 3, a half on both off-diagonal entries otherwise
__device__ __forceinline__ void strain_matrix(int w, double s, double *D)
{
#pragma unroll
  for (int i = 0; i < 9; i++) D[i] = (i % 4 == 0) ? 1.0 : 0.0;
  const int a = comp_a(w), b = comp_b(w);
  if (a == b) {
    D[4 * a] = 1.0 + s;
  } else {
    D[3 * a + b] = 0.5 * s;
    D[3 * b + a] = 0.5 * s;
  }
}

// rows [r0, r1) back to the saved copy, T = I: the end of a pass, and of a configuration that failed
template <int NT>
__device__ __forceinline__ void restore(int t, int j, int r0, int r1, double *__restrict__ x, const double *__restrict__ x0,
                                        double *__restrict__ T)
{
  for (int i = 3 * r0 + t; i < 3 * r1; i += NT) x[i] = x0[i];
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) T[9 * (size_t) j + i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
}

// Launch k of a pass for one configuration j, rows [r0, r1), served by thread t of NT (all of them take every branch together:
// each decision is made from totals that are the same in all, or from k).
template <int NT>
__device__ __forceinline__ void elastic_configuration(int t, int j, int r0, int r1, int k, double h, double inv2h,
                                                      double *__restrict__ x, const double *__restrict__ x0,
                                                      const double *__restrict__ xt, const double *__restrict__ origins,
                                                      const double *__restrict__ h0, const double *__restrict__ f,
                                                      const double *__restrict__ eatom, const double *__restrict__ virial,
                                                      double *__restrict__ T, double *__restrict__ Bt,
                                                      double *__restrict__ coupling, const long long *__restrict__ c_first,
                                                      double *__restrict__ f0, double *__restrict__ d_fmax,
                                                      double *__restrict__ d_energy, double *__restrict__ stress0, int *d_status,
                                                      double *part)
{
  const int N = 3 * (r1 - r0);
  const double *W = virial + 6 * (size_t) j;
  const double V0 = det3(h0 + 9 * (size_t) j);
  double bad = 0.0;
#pragma unroll
  for (int v = 0; v < 6; v++)
    if (!isfinite(W[v])) bad = 1.0;
  if (k == 0) {
    // 1. the forces at zero strain, the largest of them, the energy and the stress
    if (!(V0 > 0.0) || !isfinite(V0)) bad = 1.0;
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
#pragma unroll
      for (int v = 0; v < 6; v++) stress0[6 * (size_t) j + v] = -(W[v] / V0);
    }
  } else {
    // 2. harvest strain k - 1 into row w of Bt and of the coupling
    const int w = (k - 1) / 2, minus = (k - 1) & 1;
    double D[9];
    strain_matrix(w, minus ? -h : h, D);
    const double V = V0 * det3(D);
    const double *fj = f + 3 * (size_t) r0;
    for (int i = t; i < N; i += NT)
      if (!isfinite(fj[i])) bad = 1.0;
    bad = segment_total<NT, true>(bad, part);
    if (bad == 0.0) {
      double *Lw = coupling + c_first[j] + (size_t) w * N;
      for (int i = t; i < N; i += NT) Lw[i] = minus ? (Lw[i] - fj[i]) * inv2h : fj[i];   // parked after + h, then (f+ - f-) / (2 h)
      if (t < 6) {
        double *b = Bt + 36 * (size_t) j + 6 * w + t;
        const double sig = -(W[t] / V);
        *b = minus ? (*b - sig) * inv2h : sig;
      }
    }
  }
  if (bad != 0.0) {
    if (t == 0) d_status[j] = MTP_ELASTIC_FAILED;
    restore<NT>(t, j, r0, r1, x, x0, T);
    return;
  }
  // 3. the geometry of strain k
  if (k == 12) {
    restore<NT>(t, j, r0, r1, x, x0, T);
    return;
  }
  double D[9];
  strain_matrix(k / 2, (k & 1) ? -h : h, D);
  const double *o = origins + 3 * (size_t) j;
  for (int r = r0 + t; r < r1; r += NT) {
    const double a0 = xt[3 * (size_t) r], a1 = xt[3 * (size_t) r + 1], a2 = xt[3 * (size_t) r + 2];
#pragma unroll
    for (int b = 0; b < 3; b++) x[3 * (size_t) r + b] = o[b] + ((a0 * D[b] + a1 * D[3 + b]) + a2 * D[6 + b]);
  }
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) T[9 * (size_t) j + i] = D[i];
  }
}

// for_each_live_segment's split (mtp_batch_step.hpp) over the rows of the configurations; a failed configuration is skipped
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) elastic_step_kernel(
    int ncfg, const int *__restrict__ cfg_first, int k, double h, double inv2h, double *__restrict__ x, const double *__restrict__ x0,
    const double *__restrict__ xt, const double *__restrict__ origins, const double *__restrict__ h0, const double *__restrict__ f,
    const double *__restrict__ eatom, const double *__restrict__ virial, double *__restrict__ T, double *__restrict__ Bt,
    double *__restrict__ coupling, const long long *__restrict__ c_first, double *__restrict__ f0, double *__restrict__ d_fmax,
    double *__restrict__ d_energy, double *__restrict__ stress0, int *d_status)
{
  __shared__ double part[BATCH_WAVES];
  for_each_live_segment(ncfg, cfg_first, d_status, [&](auto nt, int t, int j, int r0, int r1) {
    elastic_configuration<decltype(nt)::value>(t, j, r0, r1, k, h, inv2h, x, x0, xt, origins, h0, f, eatom, virial, T, Bt, coupling,
                                               c_first, f0, d_fmax, d_energy, stress0, d_status, part);
  });
}

// K[v][w] of Wallace's relation for the stress s [6]: v = (i, j), w = (k, l)
__device__ __forceinline__ double stress_correction(const double *s, int v, int w)
{
  const int i = comp_a(v), j = comp_b(v), k = comp_a(w), l = comp_b(w);
  auto sg = [&](int a, int b) {   // sigma_ab from the six components
    if (a == b) return s[a];
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return s[lo == 0 ? (hi == 1 ? 3 : 4) : 5];
  };
  auto dl = [](int a, int b) { return a == b ? 1.0 : 0.0; };
  return 0.5 * ((((dl(i, k) * sg(j, l) + dl(j, k) * sg(i, l)) + dl(i, l) * sg(j, k)) + dl(j, l) * sg(i, k)) -
                2.0 * dl(k, l) * sg(i, j));
}

// The end of a pass: one wavefront per configuration, whatever its size.  A pair (v, w) is read once and both its members are
// written by one lane; the sum rule runs over the atoms in their order.
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) elastic_finish_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                                        const long long *__restrict__ c_first,
                                                                        const double *__restrict__ coupling,
                                                                        const double *__restrict__ stress0,
                                                                        const double *__restrict__ Bt, double *__restrict__ B,
                                                                        double *__restrict__ Cm, double *__restrict__ diag,
                                                                        const int *d_status)
{
  const int t = threadIdx.x & 63, j = blockIdx.x * BATCH_WAVES + (threadIdx.x >> 6);
  if (j >= ncfg) return;   // (the whole wavefront)
  const int n = cfg_first[j + 1] - cfg_first[j];
  if (n <= 0 || d_status[j] != 0) return;
  const double *s = stress0 + 6 * (size_t) j, *bt = Bt + 36 * (size_t) j;
  double asym = 0.0, rule = 0.0;
  if (t < 36) {
    const int v = t / 6, w = t % 6;
    if (v <= w) {
      const double bvw = bt[6 * w + v], bwv = bt[6 * v + w];
      const double mvw = bvw - stress_correction(s, v, w), mwv = bwv - stress_correction(s, w, v);
      const double c = 0.5 * (mvw + mwv);
      asym = fabs(mvw - mwv);
      B[36 * (size_t) j + 6 * v + w] = bvw;
      B[36 * (size_t) j + 6 * w + v] = bwv;
      Cm[36 * (size_t) j + 6 * v + w] = c;
      Cm[36 * (size_t) j + 6 * w + v] = c;
    }
  }
  if (t < 18) {
    const int N = 3 * n, w = t / 3, d = t % 3;
    const double *Lw = coupling + c_first[j] + (size_t) w * N;
    double sum = 0.0;
    for (int i = 0; i < n; i++) sum += Lw[3 * i + d];
    rule = fabs(sum);
  }
  asym = wave_max64(asym);
  rule = wave_max64(rule);
  if (t == 0) {
    diag[2 * (size_t) j] = asym;
    diag[2 * (size_t) j + 1] = rule;
  }
}

// element (r, c), c <= r, of a packed lower triangle
__device__ __forceinline__ int tri(int r, int c) { return r * (r + 1) / 2 + c; }

// The ionic term of one configuration, one workgroup: N = 3 n in (NMIN, NMAX].  A = H + tau sum_d t_d t_d^T in LDS as a packed
// lower triangle, its Cholesky factor in place, the six right-hand sides in LDS beside it.  Every element of the trailing
// matrix is updated once per column, in column order, whichever thread does it: the factor does not depend on the split.
template <int NMIN, int NMAX>
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) elastic_relax_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                                       const long long *__restrict__ h_first,
                                                                       const double *__restrict__ H,
                                                                       const long long *__restrict__ c_first,
                                                                       const double *__restrict__ coupling,
                                                                       const double *__restrict__ vol, const double *__restrict__ B,
                                                                       const double *__restrict__ Cm, double *__restrict__ U,
                                                                       double *__restrict__ B_rel, double *__restrict__ C_rel,
                                                                       int *d_status)
{
  constexpr int NT = MTP_BATCH_BLOCK;
  __shared__ double L[NMAX * (NMAX + 1) / 2];
  __shared__ double Y[6 * NMAX];
  __shared__ double R[36];
  __shared__ double mean[18];
  __shared__ double part[BATCH_WAVES];
  const int j = blockIdx.x, t = threadIdx.x;
  const int n = cfg_first[j + 1] - cfg_first[j], N = 3 * n;
  if (N <= NMIN || N > NMAX || d_status[j] != 0) return;   // (the whole workgroup)
  const double *Hj = H + h_first[j], *Lam = coupling + c_first[j];
  double *Uj = U + c_first[j];
  if (n == 1) {   // one atom: its only degrees of freedom are the translations, nothing relaxes
    if (t < 18) Uj[t] = 0.0;
    if (t < 36) {
      B_rel[36 * (size_t) j + t] = B[36 * (size_t) j + t];
      C_rel[36 * (size_t) j + t] = Cm[36 * (size_t) j + t];
    }
    return;
  }

  // 1. A = H + (tau / n) on the entries of equal direction, tau = trace(H) / N
  double tr = 0.0;
  for (int i = t; i < N; i += NT) tr += Hj[(size_t) i * N + i];
  tr = segment_total<NT, false>(tr, part);
  const double tn = (tr / (double) N) / (double) n;
  for (int q = t; q < N * N; q += NT) {
    const int r = q / N, c = q % N;
    if (c <= r) L[tri(r, c)] = (r % 3 == c % 3) ? Hj[q] + tn : Hj[q];
  }
  // the right-hand sides without their translations: Lambda[w][3 i + d] - mean_i, the sum over the atoms in their order
  if (t < 18) {
    const int w = t / 3, d = t % 3;
    double sum = 0.0;
    for (int i = 0; i < n; i++) sum += Lam[w * N + 3 * i + d];
    mean[t] = sum / (double) n;
  }
  __syncthreads();
  for (int q = t; q < 6 * N; q += NT) Y[q] = Lam[q] - mean[3 * (q / N) + (q % N) % 3];

  // 2. Cholesky, column by column; a pivot that is not a positive finite number ends it
  bool ok = true;
  for (int k = 0; k < N; k++) {
    __syncthreads();   // the trailing update of column k - 1 is in
    const double p = L[tri(k, k)];
    if (!(p > 0.0) || !isfinite(p)) {
      ok = false;
      break;
    }
    const double d = sqrt(p);
    for (int i = k + 1 + t; i < N; i += NT) L[tri(i, k)] = L[tri(i, k)] / d;
    __syncthreads();
    if (t == 0) L[tri(k, k)] = d;   // (read again by the solves only)
    const int m = N - k - 1;
    for (int q = t; q < m * m; q += NT) {
      const int i = k + 1 + q / m, c = k + 1 + q % m;
      if (c <= i) L[tri(i, c)] = L[tri(i, c)] - L[tri(i, k)] * L[tri(c, k)];
    }
  }
  if (!ok) {   // (every thread saw the same pivot)
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int q = t; q < 6 * N; q += NT) Uj[q] = nan;
    if (t < 36) {
      B_rel[36 * (size_t) j + t] = nan;
      C_rel[36 * (size_t) j + t] = nan;
    }
    if (t == 0) d_status[j] = MTP_ELASTIC_UNSTABLE;
    return;
  }

  // 3. L y = Lambda^T, then L^T u = y, the six right-hand sides side by side
  for (int k = 0; k < N; k++) {
    __syncthreads();
    if (t < 6) Y[t * N + k] = Y[t * N + k] / L[tri(k, k)];
    __syncthreads();
    const int m = N - k - 1;
    for (int q = t; q < 6 * m; q += NT) {
      const int w = q / m, i = k + 1 + q % m;
      Y[w * N + i] = Y[w * N + i] - L[tri(i, k)] * Y[w * N + k];
    }
  }
  for (int k = N - 1; k >= 0; k--) {
    __syncthreads();
    if (t < 6) Y[t * N + k] = Y[t * N + k] / L[tri(k, k)];
    __syncthreads();
    for (int q = t; q < 6 * k; q += NT) {
      const int w = q / k, i = q % k;
      Y[w * N + i] = Y[w * N + i] - L[tri(k, i)] * Y[w * N + k];
    }
  }
  __syncthreads();

  // 4. U, R = Lambda' U^T (Lambda' without the translations; the sum over the coordinates in their order) and the two relaxed matrices
  for (int q = t; q < 6 * N; q += NT) Uj[q] = Y[q];
  if (t < 36) {
    const int v = t / 6, w = t % 6;
    double sum = 0.0;
    for (int i = 0; i < N; i++) sum += (Lam[v * N + i] - mean[3 * v + i % 3]) * Y[w * N + i];
    R[t] = sum;
  }
  __syncthreads();
  if (t < 36) {
    const int v = t / 6, w = t % 6;
    const double V0 = vol[j];
    B_rel[36 * (size_t) j + t] = B[36 * (size_t) j + t] - R[t] / V0;
    C_rel[36 * (size_t) j + t] = Cm[36 * (size_t) j + t] - (0.5 * (R[6 * v + w] + R[6 * w + v])) / V0;
  }
}

}   // namespace

extern "C" {

int mtp_elastic_step(void *stream, int ncfg, const int *d_cfg_first, int k, double h, double *d_x, const double *d_x0,
                     const double *d_xt, const double *d_origins, const double *d_h0, const double *d_f, const double *d_eatom,
                     const double *d_virial, double *d_T, double *d_Bt, double *d_coupling, const long long *d_c_first,
                     double *d_f0, double *d_fmax, double *d_energy, double *d_stress0, int *d_status)
{
  if (!stream || ncfg < 0 || k < 0 || k > 12 || !std::isfinite(h) || !(h > 0.0) ||
      (ncfg > 0 && any_null({d_cfg_first, d_x, d_x0, d_xt, d_origins, d_h0, d_f, d_eatom, d_virial, d_T, d_Bt, d_coupling, d_c_first,
                             d_f0, d_fmax, d_energy, d_stress0, d_status})))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(elastic_step_kernel, dim3((ncfg + BATCH_WAVES - 1) / BATCH_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, d_cfg_first, k, h, 1.0 / (2.0 * h), d_x, d_x0, d_xt, d_origins, d_h0,
                     d_f, d_eatom, d_virial, d_T, d_Bt, d_coupling, d_c_first, d_f0, d_fmax, d_energy, d_stress0, d_status);
  return launched();
}

int mtp_elastic_finish(void *stream, int ncfg, const int *d_cfg_first, const long long *d_c_first, const double *d_coupling,
                       const double *d_stress0, const double *d_Bt, double *d_B, double *d_C, double *d_diag, const int *d_status)
{
  if (!stream || ncfg < 0 ||
      (ncfg > 0 && any_null({d_cfg_first, d_c_first, d_coupling, d_stress0, d_Bt, d_B, d_C, d_diag, d_status})))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(elastic_finish_kernel, dim3((ncfg + BATCH_WAVES - 1) / BATCH_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ncfg, d_cfg_first, d_c_first, d_coupling, d_stress0, d_Bt, d_B, d_C, d_diag,
                     d_status);
  return launched();
}

int mtp_elastic_relax(void *stream, int ncfg, const int *d_cfg_first, const long long *d_h_first, const double *d_H,
                      const long long *d_c_first, const double *d_coupling, const double *d_vol, const double *d_B,
                      const double *d_C, double *d_U, double *d_B_rel, double *d_C_rel, int *d_status)
{
  if (!stream || ncfg < 0 ||
      (ncfg > 0 &&
       any_null({d_cfg_first, d_h_first, d_H, d_c_first, d_coupling, d_vol, d_B, d_C, d_U, d_B_rel, d_C_rel, d_status})))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  // the LDS tiers: a workgroup of a launch serves its configuration if N = 3 n lies in the tier, and leaves at once otherwise
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define MTP_ELASTIC_TIER(NMIN, NMAX)                                                                                               \
  hipLaunchKernelGGL((elastic_relax_kernel<NMIN, NMAX>), dim3(ncfg), dim3(MTP_BATCH_BLOCK), 0, st, ncfg, d_cfg_first, d_h_first, d_H, \
                     d_c_first, d_coupling, d_vol, d_B, d_C, d_U, d_B_rel, d_C_rel, d_status);                                       \
  if (hipGetLastError() != hipSuccess) return MTP_ERR_DEVICE
  MTP_ELASTIC_TIER(0, MTP_ELASTIC_TIER_SMALL);
  MTP_ELASTIC_TIER(MTP_ELASTIC_TIER_SMALL, MTP_ELASTIC_TIER_MIDDLE);
  MTP_ELASTIC_TIER(MTP_ELASTIC_TIER_MIDDLE, MTP_ELASTIC_RELAX_MAX_N);
#undef MTP_ELASTIC_TIER
  return MTP_OK;
}

}   // extern "C"
