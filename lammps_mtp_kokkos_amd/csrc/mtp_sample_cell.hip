// Batched constant-pressure sampling (include/mtp_mi355x.h, "batched constant-pressure sampling"): mtp_sample_initial with the
// cell moved by stochastic cell rescaling.  The layout, the wavefront / workgroup split and the fixed-order reductions are
// the family's (mtp_batch_step.hpp, with the unit constants); the 3 x 3 quantities of a configuration -- the kinetic tensor, the
// strain A, E = exp(A), E^-1 -- are computed by every thread that serves it, from the same inputs in the same order, so that every
// branch is taken by all of them together and nothing is staged.  Matrices are row-major [3 a + b]; vectors are rows (x = s . h).
#include "mtp_batch_step.hpp"
#include "mtp_philox.hpp"

namespace {

using namespace batch_step;

constexpr double NPT_SQRT12 = 3.4641016151377544;
constexpr double NPT_SQRT1_2 = 0.70710678118654752;

// The argument block is the kernel's only argument and is read through the kernarg segment pointer (address space 4: scalar
// loads where a value is used), as the force kernel reads its own: by-value kernel arguments are all loaded ahead of the first
// loop, and the 22 pointers with the parameters are more than the SGPR file holds (57 SGPRs get parked in VGPR lanes).
struct sample_cell_args {
  int ncfg, barostat, step;
  mtp_sample_cell_params p;
  mtp_sample_cell_arrays A;
};
#define MTP_AS4 __attribute__((address_space(4)))
typedef const sample_cell_args MTP_AS4 *KP;

// the kicked velocity of row r: mtp_sample_initial's expression
__device__ __forceinline__ void kicked(const MTP_AS4 mtp_sample_cell_arrays &A, double dtf, int r, double *vk)
{
  const double im = A.inv_mass[A.type[r] - 1];
#pragma unroll
  for (int a = 0; a < 3; a++) vk[a] = A.v[3 * (size_t) r + a] + dtf * im * A.f[3 * (size_t) r + a];
}

// out = I + sign A + A2 / 2 + sign A3 / 6 + A4 / 24
__device__ __forceinline__ void exp_series(const double *A1, const double *A2, const double *A3, const double *A4, double sign,
                                           double *out)
{
#pragma unroll
  for (int q = 0; q < 9; q++)
    out[q] = ((((q % 4 == 0 ? 1.0 : 0.0) + sign * A1[q]) + A2[q] / 2.0) + sign * (A3[q] / 6.0)) + A4[q] / 24.0;
}

// One configuration, served by thread t of NT.  Everything per configuration is read before the first reduction (in the
// workgroup's case: before its first barrier), and thread 0 writes it back after the last one.
template <int NT>
__device__ __forceinline__ void sample_cell_configuration(int t, int k, int r0, int r1, KP kp, double *part)
{
  const MTP_AS4 mtp_sample_cell_params &p = kp->p;
  const MTP_AS4 mtp_sample_cell_arrays &A = kp->A;
  const int step = kp->step;
  double w6[6], h[9], kt[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 6; q++) w6[q] = A.virial[6 * (size_t) k + q];
#pragma unroll
  for (int q = 0; q < 9; q++) h[q] = A.h[9 * (size_t) k + q];
  const double org[3] = {A.origins[3 * (size_t) k], A.origins[3 * (size_t) k + 1], A.origins[3 * (size_t) k + 2]};
  const double V = det3(h), V0 = A.V0[k], kT = KB * A.temperature[k];
  for (int r = r0 + t; r < r1; r += NT) {   // the kinetic tensor of the kicked velocities
    const double m = A.mass[A.type[r] - 1];
    double vk[3];
    kicked(A, p.dtf, r, vk);
    kt[0] += m * vk[0] * vk[0];
    kt[1] += m * vk[1] * vk[1];
    kt[2] += m * vk[2] * vk[2];
    kt[3] += m * vk[0] * vk[1];
    kt[4] += m * vk[0] * vk[2];
    kt[5] += m * vk[1] * vk[2];
  }
  bool failed = !isfinite(V) || !(V > 0.0) || !isfinite(V0) || !(V0 > 0.0);
#pragma unroll
  for (int q = 0; q < 6; q++) {
    kt[q] = MVV2E * segment_total<NT, false>(kt[q], part);
    failed = failed || !isfinite(w6[q]) || !isfinite(kt[q]);
  }
  if (failed) {
    if (t == 0) {
      A.frozen[k] = 3;
      A.done_step[k] = step;
      atomicAdd(&A.counts[2], 1);
    }
    return;
  }
  double wt[6];
#pragma unroll
  for (int q = 0; q < 6; q++) wt[q] = w6[q] + kt[q];
  const double press = ((wt[0] + wt[1]) + wt[2]) / (3.0 * V);
  if (!kp->barostat) {   // mtp_sample_initial, bit for bit
    for (int r = r0 + t; r < r1; r += NT) {
      double vk[3];
      kicked(A, p.dtf, r, vk);
#pragma unroll
      for (int a = 0; a < 3; a++) {
        A.v[3 * (size_t) r + a] = vk[a];
        A.x[3 * (size_t) r + a] += p.dt * vk[a];
      }
    }
    if (t == 0) A.press[k] = press;
    return;
  }
  // the strain of this step
  double a6[6];
  {
    const double c = p.compressibility / (3.0 * p.tau_p * V0) * p.dt, s = sqrt(2.0 * kT * c), pv = p.pressure * V;
    double xi[6];
#pragma unroll
    for (int j = 0; j < 2; j++) {
      unsigned ctr[4] = {(unsigned) step, 0x80000000u + (unsigned) j, (unsigned) (A.key[k] & 0xffffffffull), (unsigned) (A.key[k] >> 32)};
      philox4x32_10(ctr, (unsigned) (p.seed & 0xffffffffull), (unsigned) (p.seed >> 32));
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double u = ((double) ctr[a] + 0.5) * 2.3283064365386963e-10;   // 2^-32: exact, in (0, 1)
        xi[3 * j + a] = NPT_SQRT12 * (u - 0.5);
      }
    }
#pragma unroll
    for (int q = 0; q < 3; q++) a6[q] = p.cell_mask[q] ? c * ((wt[q] - pv) + kT) + s * xi[q] : 0.0;
#pragma unroll
    for (int q = 3; q < 6; q++) a6[q] = p.cell_mask[q] ? c * wt[q] + s * (xi[q] * NPT_SQRT1_2) : 0.0;
  }
  if (p.isotropic) {
    a6[0] = a6[1] = a6[2] = ((a6[0] + a6[1]) + a6[2]) / 3.0;
    a6[3] = a6[4] = a6[5] = 0.0;
  }
  int capped = 0;
#pragma unroll
  for (int q = 0; q < 6; q++)
    if (fabs(a6[q]) > p.strain_max) {
      a6[q] = copysign(p.strain_max, a6[q]);
      capped = 1;
    }
  double E[9], Einv[9];
  {
    const double A1[9] = {a6[0], a6[3], a6[4], a6[3], a6[1], a6[5], a6[4], a6[5], a6[2]};
    double A2[9], A3[9], A4[9];
    mul3(A1, A1, A2);
    mul3(A2, A1, A3);
    mul3(A2, A2, A4);
    exp_series(A1, A2, A3, A4, 1.0, E);
    exp_series(A1, A2, A3, A4, -1.0, Einv);
  }
  for (int r = r0 + t; r < r1; r += NT) {
    double vk[3], d[3];
    kicked(A, p.dtf, r, vk);
#pragma unroll
    for (int a = 0; a < 3; a++) d[a] = (A.x[3 * (size_t) r + a] - org[a]) + p.dt * vk[a];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      A.x[3 * (size_t) r + c] = org[c] + (d[0] * E[c] + d[1] * E[3 + c] + d[2] * E[6 + c]);
      A.v[3 * (size_t) r + c] = vk[0] * Einv[c] + vk[1] * Einv[3 + c] + vk[2] * Einv[6 + c];
    }
  }
  if (t == 0) {
    double hn[9], Tn[9];
    mul3(h, E, hn);
    mul3(A.T + 9 * (size_t) k, E, Tn);
    A.cellmove[k] = cell_move(hn, A.href + 9 * (size_t) k, A.nimg + 3 * (size_t) k);
    A.capped[k] += capped;
    A.press[k] = press;
#pragma unroll
    for (int q = 0; q < 9; q++) {
      A.h[9 * (size_t) k + q] = hn[q];
      A.T[9 * (size_t) k + q] = Tn[q];
    }
  }
}

// for_each_live_segment's split (mtp_batch_step.hpp); the two pointers it walks are taken from the argument block by value
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) sample_cell_step_kernel(sample_cell_args args)
{
  (void) args;   // read through the kernarg segment pointer
  KP kp = (KP) __builtin_amdgcn_kernarg_segment_ptr();
  __shared__ double part[BATCH_WAVES];
  for_each_live_segment(kp->ncfg, kp->A.cfg_first, kp->A.frozen, [&](auto nt, int t, int k, int r0, int r1) {
    sample_cell_configuration<decltype(nt)::value>(t, k, r0, r1, kp, part);
  });
}

// the ranges of the parameters; *barostat = whether the cell moves at all
bool cell_in_range(const mtp_sample_cell_params &p, int *barostat)
{
  if (!(p.dt > 0.0) || !std::isfinite(p.dt) || !std::isfinite(p.dtf) || !std::isfinite(p.pressure) ||
      !std::isfinite(p.compressibility) || !(p.compressibility > 0.0) || !(p.strain_max > 0.0) || !(p.strain_max <= 0.05))
    return false;
  int any = 0;
  for (int m : p.cell_mask) {
    if (m != 0 && m != 1) return false;
    any |= m;
  }
  if (p.isotropic && !(p.cell_mask[0] && p.cell_mask[1] && p.cell_mask[2])) return false;
  *barostat = any && std::isfinite(p.tau_p) && p.tau_p > 0.0;
  return true;
}

}   // namespace

extern "C" {

int mtp_sample_cell_step(void *stream, int ncfg, const mtp_sample_cell_params *params, int step, const mtp_sample_cell_arrays *arrays)
{
  int barostat = 0;
  if (!stream || ncfg < 0 || step < 0 || !params || !cell_in_range(*params, &barostat)) return MTP_ERR_ARG;
  if (ncfg > 0) {
    if (!arrays) return MTP_ERR_ARG;
    const mtp_sample_cell_arrays &A = *arrays;
    if (any_null({A.cfg_first, A.x, A.v, A.f, A.type, A.inv_mass, A.mass, A.virial, A.temperature, A.key, A.origins, A.V0, A.h, A.T,
                  A.href, A.nimg, A.frozen, A.done_step, A.cellmove, A.capped, A.press, A.counts}))
      return MTP_ERR_ARG;
  }
  if (ncfg == 0) return MTP_OK;
  hipLaunchKernelGGL(sample_cell_step_kernel, dim3((ncfg + BATCH_WAVES - 1) / BATCH_WAVES), dim3(MTP_BATCH_BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), sample_cell_args{ncfg, barostat, step, *params, *arrays});
  return launched();
}

}   // extern "C"
