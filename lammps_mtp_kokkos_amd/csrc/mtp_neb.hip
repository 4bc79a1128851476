// Batched nudged elastic band (include/mtp_mi355x.h, "batched nudged elastic band"): the climbing-image NEB over a batch of
// independent bands in the layout of the batched configurations.  A band is a run of consecutive configurations (images) with
// the same atoms in the same fixed cell; its first and last image are never moved.  ONE launch a step, after the force call
// and the ghost fold: the image energies, the tangents under the minimum image, the NEB force, ONE FIRE state machine per band
// over its interior rows, the convergence decision and the move.  This is the one kernel of the batched family that couples
// configurations: a workgroup owns a band.  No context, no handle: every array is the caller's, and the entry point takes the
// stream and rejects NULL (the rule of mtp_relax_step).  The FIRE rule, its row sweeps and the fixed-order reductions are the
// family's: mtp_batch_step.hpp.
#include "mtp_batch_step.hpp"

namespace {

using namespace batch_step;

constexpr int NT = MTP_BATCH_BLOCK;

// d - rint(d . h^-1) . h, row-vector convention (rows of h are the lattice vectors)
__device__ __forceinline__ void mic(const double *h, const double *hi, double *d)
{
  const double n0 = rint(d[0] * hi[0] + d[1] * hi[3] + d[2] * hi[6]);
  const double n1 = rint(d[0] * hi[1] + d[1] * hi[4] + d[2] * hi[7]);
  const double n2 = rint(d[0] * hi[2] + d[1] * hi[5] + d[2] * hi[8]);
#pragma unroll
  for (int a = 0; a < 3; a++) d[a] -= n0 * h[a] + n1 * h[3 + a] + n2 * h[6 + a];
}

// tau = wp D+ + wm D- of one atom: rows rm, r0, rp of the images i - 1, i, i + 1, origins om, o0, op; dp and dm are D+ and D-
__device__ __forceinline__ void tangent_row(const double *x, size_t rm, size_t r0, size_t rp, const double *om, const double *o0,
                                            const double *op, const double *h, const double *hi, double wp, double wm, double *dp,
                                            double *dm, double *tau)
{
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double c0 = x[3 * r0 + a] - o0[a];
    dp[a] = (x[3 * rp + a] - op[a]) - c0;
    dm[a] = c0 - (x[3 * rm + a] - om[a]);
  }
  mic(h, hi, dp);
  mic(h, hi, dm);
#pragma unroll
  for (int a = 0; a < 3; a++) tau[a] = wp * dp[a] + wm * dm[a];
}

// One workgroup, one band.  Every thread takes every branch together: each decision is made from values that are the same in
// all of them (LDS totals, or the workgroup's vote).  An image is served by one wavefront, images in turn over the four; the
// interior rows of a band are consecutive rows, and the FIRE sweeps run over them with the whole workgroup.
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) neb_step_kernel(mtp_neb_params p, int step, int last, mtp_neb_arrays A)
{
  __shared__ double sE[MTP_NEB_MAX_IMAGES], sP[MTP_NEB_MAX_IMAGES], sVV[MTP_NEB_MAX_IMAGES], sFF[MTP_NEB_MAX_IMAGES],
      sFM[MTP_NEB_MAX_IMAGES], part[BATCH_WAVES];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int k0 = A.band_first[b], M = A.band_first[b + 1] - k0;
  if (M < 3 || M > MTP_NEB_MAX_IMAGES) return;   // (the host copy of the table was checked: the device copy must not overrun LDS)
  const int *cfg_first = A.cfg_first + k0;
  const int n = cfg_first[1] - cfg_first[0];
  const int status = A.band_status[b];
  // 1. the capture check (and the atom counts: images that differ in theirs have no tangent)
  int held = 0, broken = 0;   // broken: no tangent can be made (atom counts here, an energy that is not finite below)
  for (int i = t; i < M; i += NT) {
    held |= A.frozen[k0 + i] != 0;
    broken |= cfg_first[i + 1] - cfg_first[i] != n;
  }
  held = __syncthreads_or(held);       // every thread has read the flags before one of them is set
  broken = __syncthreads_or(broken);
  if (status != 0) return;
  if (held) {
    for (int i = t; i < M; i += NT)
      if (A.frozen[k0 + i] == 0) {
        A.frozen[k0 + i] = 1;
        atomicAdd(&A.counts[2], 1);
      }
    if (t == 0) {
      A.band_status[b] = 1;
      A.done_step[b] = step;
    }
    return;
  }
  // 2. the energies of the images
  if (!broken)
    for (int i = wave; i < M; i += BATCH_WAVES) {
      const double *ea = A.eatom + cfg_first[i];
      double e = 0.0;
      for (int j = lane; j < n; j += 64) e += ea[j];
      e = segment_total<64, false>(e, part);
      if (lane == 0) {
        sE[i] = e;
        A.energy[k0 + i] = e;
      }
    }
  __syncthreads();
  if (!broken)   // an image energy that is not finite fails the band like images of different sizes: no tangent is made from it
    for (int i = 0; i < M; i++) broken |= !isfinite(sE[i]);
  int climber = -1;
  if (!broken && p.climb_step >= 0 && step >= p.climb_step) {
    climber = 1;
    for (int i = 2; i < M - 1; i++)
      if (sE[i] > sE[climber]) climber = i;
  }
  // 3., 4. tangents and the NEB force, image by image; the image's share of the FIRE totals goes to LDS
  double h[9], hi[9];
#pragma unroll
  for (int a = 0; a < 9; a++) {
    h[a] = A.cell[9 * (size_t) b + a];
    hi[a] = A.cell_inv[9 * (size_t) b + a];
  }
  if (!broken)
    for (int i = wave; i < M; i += BATCH_WAVES) {
      const size_t r0 = (size_t) cfg_first[i];
      if (i == 0 || i == M - 1) {
        for (int j = lane; j < n; j += 64) {
#pragma unroll
          for (int a = 0; a < 3; a++) A.fneb[3 * (r0 + j) + a] = 0.0;
        }
        continue;
      }
      const size_t rm = (size_t) cfg_first[i - 1], rp = (size_t) cfg_first[i + 1];
      const double *om = A.origins + 3 * (size_t) (k0 + i - 1), *o0 = om + 3, *op = om + 6;
      const double em = sE[i - 1], e0 = sE[i], ep = sE[i + 1];
      double wp, wm;
      if (ep > e0 && e0 > em) {
        wp = 1.0, wm = 0.0;
      } else if (ep < e0 && e0 < em) {
        wp = 0.0, wm = 1.0;
      } else {
        const double up = fabs(ep - e0), dn = fabs(em - e0), big = fmax(up, dn), small = fmin(up, dn);
        if (ep > em)
          wp = big, wm = small;
        else
          wp = small, wm = big;
      }
      double sp = 0.0, sm = 0.0, tt = 0.0, ft = 0.0, dp[3], dm[3], tau[3];
      for (int j = lane; j < n; j += 64) {
        tangent_row(A.x, rm + j, r0 + j, rp + j, om, o0, op, h, hi, wp, wm, dp, dm, tau);
#pragma unroll
        for (int a = 0; a < 3; a++) {
          sp += dp[a] * dp[a];
          sm += dm[a] * dm[a];
          tt += tau[a] * tau[a];
          ft += A.f[3 * (r0 + j) + a] * tau[a];
        }
      }
      sp = segment_total<64, false>(sp, part);
      sm = segment_total<64, false>(sm, part);
      tt = segment_total<64, false>(tt, part);
      ft = segment_total<64, false>(ft, part);
      const double norm = sqrt(tt), fpar = ft / norm;
      const bool bad = !(norm > 0.0 && isfinite(norm));
      const double g = (i == climber ? -2.0 * fpar : p.spring * (sqrt(sp) - sqrt(sm)) - fpar) / norm;
      double P = 0.0, vv = 0.0, ff = 0.0, fm = 0.0;
      for (int j = lane; j < n; j += 64) {
        tangent_row(A.x, rm + j, r0 + j, rp + j, om, o0, op, h, hi, wp, wm, dp, dm, tau);
        double f2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const double fa = A.f[3 * (r0 + j) + a] + g * tau[a], va = A.v[3 * (r0 + j) + a];
          A.fneb[3 * (r0 + j) + a] = fa;
          P += fa * va;
          vv += va * va;
          f2 += fa * fa;
        }
        ff += f2;
        fm = fmax(fm, f2);
      }
      P = segment_total<64, false>(P, part);
      vv = segment_total<64, false>(vv, part);
      ff = segment_total<64, false>(ff, part);
      fm = segment_total<64, true>(fm, part);
      if (lane == 0) {
        sP[i] = P;
        sVV[i] = vv;
        sFF[i] = bad ? NAN : ff;
        sFM[i] = fm;
      }
    }
  __syncthreads();   // the totals in LDS, and d_fneb of every image, are there for every thread
  // 5. FIRE over the interior rows: the rule of mtp_batch_step.hpp with F_neb in place of f, ONE state machine for the band
  double P = 0.0, vv = 0.0, ff = broken ? NAN : 0.0, fmax2 = 0.0;
  if (!broken)
    for (int i = 1; i < M - 1; i++) {
      P += sP[i];
      vv += sVV[i];
      ff += sFF[i];
      fmax2 = fmax(fmax2, sFM[i]);
    }
  const int r0 = cfg_first[1], r1 = cfg_first[M - 1];
  if (t == 0) {
    A.fmax[b] = sqrt(fmax2);
    A.climber[b] = climber;
  }
  const bool failed = !isfinite(ff);
  if (failed || fmax2 <= p.fire.ftol * p.fire.ftol) {
    if (!failed)
      for (int r = r0 + t; r < r1; r += NT) {
#pragma unroll
        for (int a = 0; a < 3; a++) A.v[3 * (size_t) r + a] = 0.0;
      }
    for (int i = t; i < M; i += NT) A.frozen[k0 + i] = failed ? 3 : 2;
    if (t == 0) {
      A.band_status[b] = failed ? 3 : 2;
      A.done_step[b] = step;
      atomicAdd(&A.counts[2], M);
    }
    return;
  }
  if (last) return;
  fire_state s = {A.dt[b], A.alpha[b], A.npos[b]};
  double ca, cb;
  fire_mix(P, vv, ff, p.fire, s, ca, cb);
  // (the total's barriers: every thread has read dt, alpha and npos before thread 0 writes them)
  const double vmax = segment_total<NT, true>(fire_rows_vmax<NT>(t, r0, r1, ca, cb, A.v, A.fneb), part);
  fire_rows_move<NT>(t, r0, r1, ca, cb, fire_step(s.dt, vmax, p.fire), A.x, A.v, A.fneb, A.type, A.inv_mass);
  if (t == 0) {
    A.dt[b] = s.dt;
    A.alpha[b] = s.alpha;
    A.npos[b] = s.npos;
  }
}

}   // namespace

extern "C" {

int mtp_neb_step(void *stream, int nband, const int *band_first, int ncfg, const mtp_neb_params *params, int step, int last,
                 const mtp_neb_arrays *arrays)
{
  if (!stream || nband < 0 || ncfg < 0 || step < 0 || !params || !in_range(params->fire) || !std::isfinite(params->spring) ||
      !(params->spring > 0.0))
    return MTP_ERR_ARG;
  if (nband == 0) return MTP_OK;
  if (!band_first || !arrays) return MTP_ERR_ARG;
  const mtp_neb_arrays &A = *arrays;
  if (any_null({A.band_first, A.cfg_first, A.x, A.v, A.f, A.eatom, A.type, A.inv_mass, A.origins, A.cell, A.cell_inv, A.fneb,
                A.energy, A.dt, A.alpha, A.npos, A.done_step, A.fmax, A.climber, A.band_status, A.frozen, A.counts}))
    return MTP_ERR_ARG;
  if (band_first[0] < 0 || band_first[nband] > ncfg) return MTP_ERR_ARG;
  for (int b = 0; b < nband; b++) {
    const long long m = (long long) band_first[b + 1] - band_first[b];
    if (m < 3 || m > MTP_NEB_MAX_IMAGES) return MTP_ERR_ARG;
  }
  hipLaunchKernelGGL(neb_step_kernel, dim3(nband), dim3(MTP_BATCH_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), *params, step,
                     last ? 1 : 0, A);
  return launched();
}

}   // extern "C"
