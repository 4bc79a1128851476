// Batched sampling (include/mtp_mi355x.h, "batched sampling"): the integrator pieces of finite-temperature MD over a batch
// of independent periodic cells in the layout of the batched configurations -- owned rows of configuration k are
// [cfg_first[k], cfg_first[k + 1]) of every per-atom array, positions in slot coordinates (cell coordinates + origins[k])
// between re-neighbourings.  Either side of the force call: the first half step, LAMMPS' fix langevin (uniform noise,
// counter-based: Philox4x32-10) with the second half step in one launch, the per-configuration monitor, and the capture of
// extrapolating configurations -- select / break decisions, slot hand-out and snapshot on the device.  No context, no
// handle: every array is the caller's, every entry point takes the stream and rejects NULL (the rule of mtp_nve_*).  The unit
// constants, the wavefront reductions and the launch epilogue are the family's: mtp_batch_step.hpp.
#include "mtp_batch_step.hpp"
#include "mtp_philox.hpp"

namespace {

using namespace batch_step;

// row_cfg[i] = the configuration of owned row i: the last k < ncfg with cfg_first[k] <= i (empty configurations share
// their start with the next one, which this skips).  The one binary search per row of a pass.
__global__ void __launch_bounds__(256) sample_row_map_kernel(int ncfg, const int *__restrict__ cfg_first, int nrows,
                                                            int *__restrict__ row_cfg)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nrows) return;
  int lo = 0, hi = ncfg - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (cfg_first[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  row_cfg[i] = lo;
}

// fix nve, first half, for the rows of unfrozen configurations (one lane per coordinate, the expressions of
// nve_initial_kernel); rows of a frozen configuration are not written
__global__ void __launch_bounds__(256) sample_initial_kernel(const int *__restrict__ row_cfg, const int *__restrict__ frozen,
                                                            double *__restrict__ x, double *__restrict__ v,
                                                            const double *__restrict__ f, const int *__restrict__ type,
                                                            const double *__restrict__ inv_mass, double dtf, double dt, int n3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int i = e / 3;
  if (frozen[row_cfg[i]]) return;
  const double vv = v[e] + dtf * inv_mass[type[i] - 1] * f[e];
  v[e] = vv;
  x[e] += dt * vv;
}

// fix langevin's post_force (uniform noise, no tally, no zero) followed by fix nve's second half, one lane per atom:
//   f += gamma1 v + gamma2 (u - 0.5)  (stored back: the next first half kicks with it);  v += dtf f / m
// THERMOSTAT = false: the second half alone (nve_final_kernel's expression), nothing drawn, f not written
template <bool THERMOSTAT>
__global__ void __launch_bounds__(256) sample_final_kernel(int nrows, const int *__restrict__ row_cfg,
                                                          const int *__restrict__ cfg_first, const int *__restrict__ frozen,
                                                          double *__restrict__ v, double *__restrict__ f,
                                                          const int *__restrict__ type, const double *__restrict__ mass,
                                                          const double *__restrict__ inv_mass,
                                                          const double *__restrict__ temperature,
                                                          const unsigned long long *__restrict__ key, unsigned seed_lo,
                                                          unsigned seed_hi, unsigned step, double dtf, double dt, double t_damp)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nrows) return;
  const int k = row_cfg[i];
  if (frozen[k]) return;
  const int t = type[i] - 1;
  const double im = inv_mass[t];
  double fi[3] = {f[3 * (size_t) i], f[3 * (size_t) i + 1], f[3 * (size_t) i + 2]};
  if (THERMOSTAT) {
    const double m = mass[t];
    const double gamma1 = -m / t_damp / FTM2V;
    const double gamma2 = sqrt(m) * sqrt(24.0 * KB * temperature[k] / t_damp / dt / MVV2E) / FTM2V;
    const unsigned long long kk = key[k];
    unsigned c[4] = {step, (unsigned) (i - cfg_first[k]), (unsigned) (kk & 0xffffffffull), (unsigned) (kk >> 32)};
    philox4x32_10(c, seed_lo, seed_hi);
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double u = ((double) c[a] + 0.5) * 2.3283064365386963e-10;   // 2^-32: exact, in (0, 1)
      fi[a] = fi[a] + gamma1 * v[3 * (size_t) i + a] + gamma2 * (u - 0.5);
      f[3 * (size_t) i + a] = fi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) v[3 * (size_t) i + a] += dtf * im * fi[a];
}

// what thread t of NT co-operating threads finds in rows [r0, r1): sum m v^2 and max |x - x_ref|^2
template <int NT>
__device__ __forceinline__ void monitor_partials(int t, int r0, int r1, const double *__restrict__ x,
                                                 const double *__restrict__ x_ref, const double *__restrict__ v,
                                                 const int *__restrict__ type, const double *__restrict__ mass, double &mv2,
                                                 double &d2max)
{
  mv2 = 0.0;
  d2max = 0.0;
  for (int r = r0 + t; r < r1; r += NT) {
    double d2 = 0.0, vv = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double d = x[3 * (size_t) r + a] - x_ref[3 * (size_t) r + a];
      d2 += d * d;
      vv += v[3 * (size_t) r + a] * v[3 * (size_t) r + a];
    }
    mv2 += mass[type[r] - 1] * vv;
    d2max = fmax(d2max, d2);
  }
}

// The split of for_each_live_segment (mtp_batch_step.hpp), written out: this kernel also serves empty and frozen
// configurations, and combines its two values on thread 0 with one barrier pair for both, where the shared function's
// segment_total would cost a pair for each.  mv2[k] = sum m v^2, d2[k] = the largest squared displacement from x_ref (0 for a
// frozen configuration: it does not move, and must not ask for a re-neighbouring).  No atomics; the order of every sum
// depends on the segment's length alone.
__global__ void __launch_bounds__(MTP_BATCH_BLOCK) sample_monitor_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                                        const int *__restrict__ frozen,
                                                                        const double *__restrict__ x,
                                                                        const double *__restrict__ x_ref,
                                                                        const double *__restrict__ v,
                                                                        const int *__restrict__ type,
                                                                        const double *__restrict__ mass,
                                                                        double *__restrict__ mv2, double *__restrict__ d2)
{
  __shared__ double part[MTP_BATCH_BLOCK / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = blockIdx.x * (MTP_BATCH_BLOCK / 64);
  double s, m;
  if (k0 + wave < ncfg) {   // (the whole wavefront)
    const int k = k0 + wave, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 - r0 <= MTP_BATCH_WAVE_ROWS) {
      monitor_partials<64>(lane, r0, r1, x, x_ref, v, type, mass, s, m);
      s = wave_sum64(s);
      m = wave_max64(m);
      if (lane == 0) {
        mv2[k] = s;
        d2[k] = frozen[k] ? 0.0 : m;
      }
    }
  }
  for (int w = 0; w < MTP_BATCH_BLOCK / 64 && k0 + w < ncfg; w++) {   // (the whole workgroup)
    const int k = k0 + w, r0 = cfg_first[k], r1 = cfg_first[k + 1];
    if (r1 - r0 <= MTP_BATCH_WAVE_ROWS) continue;
    monitor_partials<MTP_BATCH_BLOCK>(threadIdx.x, r0, r1, x, x_ref, v, type, mass, s, m);
    s = wave_sum64(s);
    m = wave_max64(m);
    if (lane == 0) {
      part[wave][0] = s;
      part[wave][1] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double ts = part[0][0], tm = part[0][1];
#pragma unroll
      for (int u = 1; u < MTP_BATCH_BLOCK / 64; u++) {
        ts += part[u][0];
        tm = fmax(tm, part[u][1]);
      }
      mv2[k] = ts;
      d2[k] = frozen[k] ? 0.0 : tm;
    }
    __syncthreads();
  }
}

// the host-visible block: {max_k d2[k], frozen, captured, dropped} (counts as doubles).  One workgroup walks d2.
__global__ void __launch_bounds__(256) sample_block_kernel(int ncfg, const double *__restrict__ d2, const int *__restrict__ counts,
                                                          double *__restrict__ block)
{
  __shared__ double part[4];
  double m = 0.0;
  for (int k = threadIdx.x; k < ncfg; k += 256) m = fmax(m, d2[k]);
  m = wave_max64(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    block[0] = fmax(fmax(part[0], part[1]), fmax(part[2], part[3]));
    block[1] = (double) counts[2];
    block[2] = (double) counts[0];
    block[3] = (double) counts[1];
  }
}

// The capture decisions of one grade step, ONE workgroup walking the configurations 256 at a time with a running count
// (an exclusive scan: slots in ascending configuration order, no atomic counter, any ncfg).  Configuration k wants a slot
// if it is neither frozen nor empty, !(g < select) and step - last_capture[k] >= gap; it gets slot captured + (wanting
// configurations before it) if that is below max_candidates, otherwise it is dropped -- nothing of it is written.  A
// configuration that got its slot freezes if !(g < brk).  slot[k] = the slot (its snapshot is sample_snapshot_kernel's), -1
// for none.  counts = {captured, dropped, frozen}.
__global__ void __launch_bounds__(256) sample_capture_kernel(int ncfg, const int *__restrict__ cfg_first,
                                                            const double *__restrict__ grade, int step, double select, double brk,
                                                            int gap, int *__restrict__ frozen, int *__restrict__ last_capture,
                                                            int *__restrict__ slot, int max_candidates, int *__restrict__ rec,
                                                            double *__restrict__ rec_grade, int *__restrict__ counts)
{
  __shared__ int scan[256];
  __shared__ int carry[3];   // captured, dropped, frozen so far
  const int t = threadIdx.x;
  if (t == 0) {
    carry[0] = counts[0];
    carry[1] = counts[1];
    carry[2] = counts[2];
  }
  __syncthreads();
  for (int base = 0; base < ncfg; base += 256) {
    const int k = base + t;
    double g = 0.0;
    int want = 0;
    if (k < ncfg) {
      g = grade[k];
      want = !frozen[k] && cfg_first[k + 1] > cfg_first[k] && !(g < select) &&
          (long long) step - (long long) last_capture[k] >= (long long) gap;
    }
    scan[t] = want;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {   // inclusive Hillis-Steele scan of the chunk
      const int add = t >= s ? scan[t - s] : 0;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    const int before = scan[t] - want, total = scan[255];
    // wanting configurations so far: the kept ones came first, so once one was dropped first_slot is beyond the buffer
    const int first_slot = carry[0] + carry[1];
    int got = -1, froze = 0;
    if (want) {
      const int s = first_slot + before;   // its rank among all wanting configurations of the run
      if (s < max_candidates) {
        got = s;
        rec[2 * (size_t) s] = k;
        rec[2 * (size_t) s + 1] = step;
        rec_grade[s] = g;
        last_capture[k] = step;
        if (!(g < brk)) {
          frozen[k] = 1;
          froze = 1;
        }
      }
    }
    if (k < ncfg) slot[k] = got;
    __syncthreads();
    scan[t] = froze;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) scan[t] += scan[t + s];
      __syncthreads();
    }
    if (t == 0) {
      const int room = max_candidates > first_slot ? max_candidates - first_slot : 0;
      const int kept = total < room ? total : room;
      carry[0] += kept;
      carry[1] += total - kept;
      carry[2] += scan[0];
    }
    __syncthreads();
  }
  if (t == 0) {
    counts[0] = carry[0];
    counts[1] = carry[1];
    counts[2] = carry[2];
  }
}

// the snapshot of every configuration that got a slot: its owned positions minus the slot origin, `stride` rows a slot
__global__ void __launch_bounds__(256) sample_snapshot_kernel(int n3, const int *__restrict__ row_cfg,
                                                             const int *__restrict__ cfg_first, const int *__restrict__ slot,
                                                             const double *__restrict__ x, const double *__restrict__ origins,
                                                             int max_candidates, int stride, double *__restrict__ cand_x)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int i = e / 3, a = e - 3 * i, k = row_cfg[i], s = slot[k], j = i - cfg_first[k];
  if (s < 0 || s >= max_candidates || j >= stride) return;
  cand_x[3 * ((size_t) s * stride + j) + a] = x[e] - origins[3 * (size_t) k + a];
}

// slot coordinates back to cell coordinates (what mtp_ghosts_build_batch wraps and translates again)
__global__ void __launch_bounds__(256) sample_to_cell_kernel(int n3, const int *__restrict__ row_cfg,
                                                            const double *__restrict__ origins, double *__restrict__ x)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int i = e / 3;
  x[e] -= origins[3 * (size_t) row_cfg[i] + (e - 3 * i)];
}

}   // namespace

extern "C" {

int mtp_sample_row_map(void *stream, int ncfg, const int *d_cfg_first, int nrows, int *d_row_cfg)
{
  if (!stream || ncfg < 0 || nrows < 0 || (nrows > 0 && (ncfg < 1 || !d_cfg_first || !d_row_cfg))) return MTP_ERR_ARG;
  if (nrows > 0)
    hipLaunchKernelGGL(sample_row_map_kernel, dim3((nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       ncfg, d_cfg_first, nrows, d_row_cfg);
  return launched();
}

int mtp_sample_initial(void *stream, int nrows, const int *d_row_cfg, const int *d_frozen, double *d_x, double *d_v,
                       const double *d_f, const int *d_type, const double *d_inv_mass, double dtf, double dt)
{
  if (!stream || nrows < 0 || nrows > 0x7fffffff / 3 ||
      (nrows > 0 && (!d_row_cfg || !d_frozen || !d_x || !d_v || !d_f || !d_type || !d_inv_mass)))
    return MTP_ERR_ARG;
  if (nrows > 0)
    hipLaunchKernelGGL(sample_initial_kernel, dim3((3 * nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       d_row_cfg, d_frozen, d_x, d_v, d_f, d_type, d_inv_mass, dtf, dt, 3 * nrows);
  return launched();
}

int mtp_sample_final(void *stream, int nrows, const int *d_row_cfg, const int *d_cfg_first, const int *d_frozen, double *d_v,
                     double *d_f, const int *d_type, const double *d_mass, const double *d_inv_mass,
                     const double *d_temperature, const unsigned long long *d_key, unsigned long long seed, int step, double dtf,
                     double dt, double t_damp)
{
  const bool thermostat = t_damp > 0.0 && std::isfinite(t_damp);
  if (!stream || nrows < 0 || step < 0 || !(dt > 0.0) ||
      (nrows > 0 && (!d_row_cfg || !d_cfg_first || !d_frozen || !d_v || !d_f || !d_type || !d_inv_mass)) ||
      (nrows > 0 && thermostat && (!d_mass || !d_temperature || !d_key)))
    return MTP_ERR_ARG;
  if (nrows > 0) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned lo = (unsigned) (seed & 0xffffffffull), hi = (unsigned) (seed >> 32);
    if (thermostat)
      hipLaunchKernelGGL(sample_final_kernel<true>, dim3((nrows + 255) / 256), dim3(256), 0, st, nrows, d_row_cfg, d_cfg_first,
                         d_frozen, d_v, d_f, d_type, d_mass, d_inv_mass, d_temperature, d_key, lo, hi, (unsigned) step, dtf, dt,
                         t_damp);
    else
      hipLaunchKernelGGL(sample_final_kernel<false>, dim3((nrows + 255) / 256), dim3(256), 0, st, nrows, d_row_cfg, d_cfg_first,
                         d_frozen, d_v, d_f, d_type, d_mass, d_inv_mass, d_temperature, d_key, lo, hi, (unsigned) step, dtf, dt,
                         t_damp);
  }
  return launched();
}

int mtp_sample_monitor(void *stream, int ncfg, const int *d_cfg_first, const int *d_frozen, const double *d_x,
                       const double *d_x_ref, const double *d_v, const int *d_type, const double *d_mass, const int *d_counts,
                       double *d_mv2, double *d_d2, double *d_block4)
{
  if (!stream || ncfg < 0 || !d_counts || !d_block4 ||
      (ncfg > 0 && (!d_cfg_first || !d_frozen || !d_x || !d_x_ref || !d_v || !d_type || !d_mass || !d_mv2 || !d_d2)))
    return MTP_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  constexpr int per_block = MTP_BATCH_BLOCK / 64;
  if (ncfg > 0)
    hipLaunchKernelGGL(sample_monitor_kernel, dim3((ncfg + per_block - 1) / per_block), dim3(MTP_BATCH_BLOCK), 0, st, ncfg,
                       d_cfg_first, d_frozen, d_x, d_x_ref, d_v, d_type, d_mass, d_mv2, d_d2);
  hipLaunchKernelGGL(sample_block_kernel, dim3(1), dim3(256), 0, st, ncfg, d_d2, d_counts, d_block4);
  return launched();
}

int mtp_sample_capture(void *stream, int ncfg, const int *d_cfg_first, int nrows, const int *d_row_cfg,
                       const double *d_cfg_grade, int step, double threshold_select, double threshold_break, int capture_gap,
                       const double *d_x, const double *d_origins, int *d_frozen, int *d_last_capture, int *d_slot,
                       int max_candidates, int stride, double *d_cand_x, int *d_rec, double *d_rec_grade, int *d_counts)
{
  if (!stream || ncfg < 0 || nrows < 0 || nrows > 0x7fffffff / 3 || step < 0 || max_candidates < 0 || stride < 0 || !d_counts ||
      capture_gap < 0 || (ncfg > 0 && (!d_cfg_first || !d_cfg_grade || !d_frozen || !d_last_capture || !d_slot)) ||
      (nrows > 0 && (!d_row_cfg || !d_x || !d_origins)) || (max_candidates > 0 && (!d_rec || !d_rec_grade)) ||
      (max_candidates > 0 && stride > 0 && !d_cand_x))
    return MTP_ERR_ARG;
  if (ncfg == 0) return MTP_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sample_capture_kernel, dim3(1), dim3(256), 0, st, ncfg, d_cfg_first, d_cfg_grade, step, threshold_select,
                     threshold_break, capture_gap, d_frozen, d_last_capture, d_slot, max_candidates, d_rec, d_rec_grade, d_counts);
  if (nrows > 0 && max_candidates > 0 && stride > 0)
    hipLaunchKernelGGL(sample_snapshot_kernel, dim3((3 * nrows + 255) / 256), dim3(256), 0, st, 3 * nrows, d_row_cfg, d_cfg_first,
                       d_slot, d_x, d_origins, max_candidates, stride, d_cand_x);
  return launched();
}

int mtp_sample_to_cell(void *stream, int nrows, const int *d_row_cfg, const double *d_origins, double *d_x)
{
  if (!stream || nrows < 0 || nrows > 0x7fffffff / 3 || (nrows > 0 && (!d_row_cfg || !d_origins || !d_x))) return MTP_ERR_ARG;
  if (nrows > 0)
    hipLaunchKernelGGL(sample_to_cell_kernel, dim3((3 * nrows + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       3 * nrows, d_row_cfg, d_origins, d_x);
  return launched();
}

}   // extern "C"
