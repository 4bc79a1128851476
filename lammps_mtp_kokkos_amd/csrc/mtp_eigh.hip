// Batched symmetric eigen-solver (include/mtp_mi355x.h, "batched symmetric eigen-solver"): eigenvalues and, if asked,
// eigenvectors of every matrix of a ragged batch -- the blocks mtp_hess_finish leaves behind h_first -- by cyclic two-sided
// Jacobi in LDS, ONE launch per LDS tier, ONE workgroup per matrix, nothing read back in between.  Mass weights and the
// projection of the three translations are applied on the way in, so the Hessians of a pass become frequencies without a copy
// to the host.  No context, no handle: every array is the caller's, and the entry point takes the stream and rejects NULL (the
// rule of mtp_relax_step).  The reductions and the entry-point checks are the family's: mtp_batch_step.hpp.
//
// The order of the operations (tests/_eigh.py follows it bit for bit), for one matrix of N rows, thread t of NT = MTP_BATCH_BLOCK:
//   load       a_rc = 0.5 * (x + y), x = A_rc / (root_r * root_c), y = A_cr / (root_c * root_r) (no division without root), r >= c
//   project    nrm_d = sqrt(sum root_i^2) over i = d, d + 3, ... from 0.0;  tau_i = root_i / nrm_(i % 3)  (root = 1.0 without)
//              u[r][d] = sum a_ri * tau_i over i = d, d + 3, ... from 0.0;  g[d][e] = sum tau_i * u[i][e] over i = d, d + 3, ...
//              a_rc <- ((a_rc - tau_r * u[c][r % 3]) - u[r][c % 3] * tau_c) + (tau_r * g[r % 3][c % 3]) * tau_c,  r >= c
//   norm       thread t adds a_rc^2 for q = r N + c = t, t + NT, ... from 0.0 (both triangles), segment_total, sqrt;
//              thr = (norm * 2^-53) / N;  the off-diagonal norm at the end is the same sum without r == c
//   a step     thread k < Ne / 2 owns pair k = (p, q): it rotates iff q < N and |a_qp| > thr, with zeta = (a_qq - a_pp) / (2 a_qp),
//              t = (zeta < 0 ? -1 : 1) / (|zeta| + sqrt(1 + zeta * zeta)), c = 1 / sqrt(1 + t * t), s = t * c (c = 1, s = 0
//              otherwise), a_pp <- a_pp - t * a_qp, a_qq <- a_qq + t * a_qp, a_qp <- 0, and parks (c, s).  After the barrier the 2 x 2
//              block B where pairs k1 > k2 meet (rows p1 q1, columns p2 q2; the padding index reads 0.0 and is not written), unless
//              s1 == 0 and s2 == 0:  X = J1^T B: x_p. = c1 * b_p. - s1 * b_q.,  x_q. = s1 * b_p. + c1 * b_q.;
//              then B <- X J2: b_.p = c2 * x_.p - s2 * x_.q,  b_.q = s2 * x_.p + c2 * x_.q.
//              V, unless s == 0 or q is the padding index:  v_rp <- c * v_rp - s * v_rq,  v_rq <- s * v_rp + c * v_rq (old values).
#include "mtp_batch_step.hpp"

// every expression below is evaluated as written (no fused multiply-add): tests/_eigh.py follows them bit for bit
#pragma clang fp contract(off)

namespace {

using namespace batch_step;

// element (r, c), c <= r, of a packed lower triangle; and element (r, c) of the symmetric matrix kept in it
__device__ __forceinline__ int tri(int r, int c) { return r * (r + 1) / 2 + c; }
__device__ __forceinline__ int sym(int r, int c) { return r >= c ? tri(r, c) : tri(c, r); }

// pair k = 0 ... Ne / 2 - 1 of step s = 0 ... M - 1 of the round-robin order, M = Ne - 1: (M, s), ((s + k) mod M, (s - k) mod M),
// taken as p < q
__device__ __forceinline__ void pair_of(int k, int s, int M, int &p, int &q)
{
  const int a = k == 0 ? M : (s + k) % M, b = k == 0 ? s : (s - k + M) % M;
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// the sum of a_rc^2 over the whole matrix (both triangles), with or without its diagonal
template <int NT>
__device__ __forceinline__ double norm2(int t, int N, const double *L, bool diagonal, double *part)
{
  double s = 0.0;
  for (int i = t; i < N * N; i += NT) {
    const int r = i / N, c = i % N;
    if (r == c && !diagonal) continue;
    const double x = L[sym(r, c)];
    s += x * x;
  }
  return segment_total<NT, false>(s, part);
}

// One matrix, one workgroup: N in (NMIN, NMAX].  A as a packed lower triangle in LDS, with VEC the vectors V [N][N] beside it.
// The workgroups of the first tier also mark what no tier serves (N > limit).
template <int NMIN, int NMAX, bool VEC>
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) eigh_kernel(int nmat, const int *__restrict__ d_n,
                                                              const long long *__restrict__ a_first, const double *__restrict__ A,
                                                              const long long *__restrict__ w_first, const double *__restrict__ root,
                                                              int project, int max_sweeps, int limit, double *__restrict__ W,
                                                              double *__restrict__ V, double *__restrict__ info, int *d_status)
{
  constexpr int NT = MTP_BATCH_BLOCK, PMAX = (NMAX + 1) / 2;
  __shared__ double L[NMAX * (NMAX + 1) / 2];
  __shared__ double Vs[VEC ? NMAX * NMAX : 1];
  __shared__ double tau[NMAX], u[3 * NMAX], g[9], nrm[3], rc[PMAX], rs[PMAX];
  __shared__ double part[BATCH_WAVES];
  __shared__ int rank[NMAX];
  const int j = blockIdx.x, t = threadIdx.x;
  const int N = d_n[j];
  if (N <= NMIN || d_status[j] != 0) return;   // (the whole workgroup)
  if (N > NMAX) {
    if (NMIN == 0 && N > limit && t == 0) d_status[j] = MTP_EIGH_TOO_LARGE;
    return;
  }
  const double *Aj = A + a_first[j], *rt = root ? root + w_first[j] : nullptr;
  double *Wj = W + w_first[j], *Vj = VEC ? V + a_first[j] : nullptr;

  // 1. load, mass-weight, symmetrise
  for (int i = t; i < N * N; i += NT) {
    const int r = i / N, c = i % N;
    if (c > r) continue;
    double x = Aj[(size_t) r * N + c], y = Aj[(size_t) c * N + r];
    if (rt) {
      x = x / (rt[r] * rt[c]);
      y = y / (rt[c] * rt[r]);
    }
    L[tri(r, c)] = 0.5 * (x + y);
  }
  double bad = (project && N % 3 != 0) ? 1.0 : 0.0;
  if (rt)
    for (int i = t; i < N; i += NT)
      if (!isfinite(rt[i])) bad = 1.0;   // (an infinite root would only zero its row)
  const bool ok = segment_total<NT, true>(bad, part) == 0.0;
  // 2. A <- P A P without the three translations
  if (project && ok) {
    if (t < 3) {
      double s = 0.0;
      for (int i = t; i < N; i += 3) {
        const double ri = rt ? rt[i] : 1.0;
        s += ri * ri;
      }
      nrm[t] = sqrt(s);
    }
    __syncthreads();
    for (int i = t; i < N; i += NT) tau[i] = (rt ? rt[i] : 1.0) / nrm[i % 3];
    __syncthreads();
    for (int i = t; i < 3 * N; i += NT) {
      const int r = i / 3, d = i % 3;
      double s = 0.0;
      for (int k = d; k < N; k += 3) s += L[sym(r, k)] * tau[k];
      u[i] = s;
    }
    __syncthreads();
    if (t < 9) {
      const int d = t / 3, e = t % 3;
      double s = 0.0;
      for (int k = d; k < N; k += 3) s += tau[k] * u[3 * k + e];
      g[t] = s;
    }
    __syncthreads();
    for (int i = t; i < N * N; i += NT) {
      const int r = i / N, c = i % N;
      if (c > r) continue;
      L[tri(r, c)] = ((L[tri(r, c)] - tau[r] * u[3 * c + r % 3]) - u[3 * r + c % 3] * tau[c]) + (tau[r] * g[3 * (r % 3) + c % 3]) * tau[c];
    }
  }
  __syncthreads();
  // 3. the norm and the threshold
  const double norm = ok ? sqrt(norm2<NT>(t, N, L, true, part)) : 0.0;
  if (!ok || !isfinite(norm)) {   // (every thread has the same total)
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = t; i < N; i += NT) Wj[i] = nan;
    if (VEC)
      for (int i = t; i < N * N; i += NT) Vj[i] = nan;
    if (t == 0) {
      info[2 * (size_t) j] = nan;
      info[2 * (size_t) j + 1] = nan;
      d_status[j] = MTP_EIGH_FAILED;
    }
    return;
  }
  const double thr = (norm * 0x1p-53) / (double) N;
  if (VEC)
    for (int i = t; i < N * N; i += NT) Vs[i] = (i / N == i % N) ? 1.0 : 0.0;

  // 4. sweeps of M steps; the barrier at the end of a step also covers V's start
  const int Ne = N + (N & 1), M = Ne - 1, P = Ne / 2;
  int sweeps = 0, st = MTP_EIGH_NOT_CONVERGED;
  while (sweeps < max_sweeps) {
    int rotated = 0;
    for (int s = 0; s < M; s++) {
      __syncthreads();
      if (t < P) {
        int p, q;
        pair_of(t, s, M, p, q);
        double c = 1.0, sn = 0.0;
        if (q < N) {
          const double apq = L[tri(q, p)];
          if (fabs(apq) > thr) {
            const double app = L[tri(p, p)], aqq = L[tri(q, q)];
            const double zeta = (aqq - app) / (2.0 * apq);
            const double tn = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            c = 1.0 / sqrt(1.0 + tn * tn);
            sn = tn * c;
            L[tri(p, p)] = app - tn * apq;
            L[tri(q, q)] = aqq + tn * apq;
            L[tri(q, p)] = 0.0;
            rotated = 1;
          }
        }
        rc[t] = c;
        rs[t] = sn;
      }
      __syncthreads();
      for (int b = t; b < P * (P - 1) / 2; b += NT) {
        int k1 = (int) ((1.0f + sqrtf(1.0f + 8.0f * (float) b)) * 0.5f);   // k1 (k1 - 1) / 2 <= b < (k1 + 1) k1 / 2
        while (k1 * (k1 - 1) / 2 > b) k1--;
        while ((k1 + 1) * k1 / 2 <= b) k1++;
        const int k2 = b - k1 * (k1 - 1) / 2;
        const double c1 = rc[k1], s1 = rs[k1], c2 = rc[k2], s2 = rs[k2];
        if (s1 == 0.0 && s2 == 0.0) continue;
        int p1, q1, p2, q2;
        pair_of(k1, s, M, p1, q1);
        pair_of(k2, s, M, p2, q2);
        const bool in1 = q1 < N, in2 = q2 < N;
        const int ipp = sym(p1, p2), ipq = sym(p1, q2), iqp = sym(q1, p2), iqq = sym(q1, q2);
        const double bpp = L[ipp], bpq = in2 ? L[ipq] : 0.0, bqp = in1 ? L[iqp] : 0.0, bqq = (in1 && in2) ? L[iqq] : 0.0;
        const double xpp = c1 * bpp - s1 * bqp, xpq = c1 * bpq - s1 * bqq;
        const double xqp = s1 * bpp + c1 * bqp, xqq = s1 * bpq + c1 * bqq;
        L[ipp] = c2 * xpp - s2 * xpq;
        if (in2) L[ipq] = s2 * xpp + c2 * xpq;
        if (in1) L[iqp] = c2 * xqp - s2 * xqq;
        if (in1 && in2) L[iqq] = s2 * xqp + c2 * xqq;
      }
      if (VEC)
        for (int i = t; i < N * P; i += NT) {
          const int r = i / P, k = i % P;
          const double c = rc[k], sn = rs[k];
          if (sn == 0.0) continue;
          int p, q;
          pair_of(k, s, M, p, q);
          if (q >= N) continue;
          const double vp = Vs[r * N + p], vq = Vs[r * N + q];
          Vs[r * N + p] = c * vp - sn * vq;
          Vs[r * N + q] = sn * vp + c * vq;
        }
    }
    sweeps++;
    if (!__syncthreads_or(rotated)) {
      st = 0;
      break;
    }
  }
  __syncthreads();

  // 5. ascending by rank, ties by index
  for (int i = t; i < N; i += NT) {
    const double d = L[tri(i, i)];
    int rk = 0;
    for (int k = 0; k < N; k++) {
      const double dk = L[tri(k, k)];
      rk += (dk < d || (dk == d && k < i)) ? 1 : 0;
    }
    rank[i] = rk;
    Wj[rk] = d;
  }
  const double off = sqrt(norm2<NT>(t, N, L, false, part));   // (its barriers order rank before the columns below)
  if (VEC)
    for (int i = t; i < N * N; i += NT) Vj[(size_t) (i / N) * N + rank[i % N]] = Vs[i];
  if (t == 0) {
    info[2 * (size_t) j] = (double) sweeps;
    info[2 * (size_t) j + 1] = off;
    if (st != 0) d_status[j] = st;
  }
}

}   // namespace

extern "C" {

int mtp_eigh_batched(void *stream, int nmat, const int *d_n, const long long *d_a_first, const double *d_A,
                     const long long *d_w_first, const double *d_root, int project, int max_sweeps, double *d_W, double *d_V,
                     double *d_info, int *d_status)
{
  if (!stream || nmat < 0 || max_sweeps < 1 || (nmat > 0 && any_null({d_n, d_a_first, d_A, d_w_first, d_W, d_info, d_status})))
    return MTP_ERR_ARG;
  if (nmat == 0) return MTP_OK;
  // the LDS tiers: a workgroup of a launch serves its matrix if N lies in the tier, and leaves at once otherwise
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int limit = d_V ? MTP_EIGH_MAX_N_VECTORS : MTP_EIGH_MAX_N, pr = project ? 1 : 0;
#define MTP_EIGH_TIER(NMIN, NMAX, VEC)                                                                                             \
  hipLaunchKernelGGL((eigh_kernel<NMIN, NMAX, VEC>), dim3(nmat), dim3(MTP_BATCH_BLOCK), 0, st, nmat, d_n, d_a_first, d_A, d_w_first, \
                     d_root, pr, max_sweeps, limit, d_W, d_V, d_info, d_status);                                                   \
  if (hipGetLastError() != hipSuccess) return MTP_ERR_DEVICE
  if (d_V) {
    MTP_EIGH_TIER(0, MTP_EIGH_TIER_SMALL, true);
    MTP_EIGH_TIER(MTP_EIGH_TIER_SMALL, MTP_EIGH_MAX_N_VECTORS, true);
  } else {
    MTP_EIGH_TIER(0, MTP_EIGH_TIER_SMALL, false);
    MTP_EIGH_TIER(MTP_EIGH_TIER_SMALL, MTP_EIGH_MAX_N_VECTORS, false);
    MTP_EIGH_TIER(MTP_EIGH_MAX_N_VECTORS, MTP_EIGH_MAX_N, false);
  }
#undef MTP_EIGH_TIER
  return MTP_OK;
}

}   // extern "C"
