// MaxVol selection on the device: which candidate vectors enter the active set (include/mtp_mi355x.h,
// mtp_maxvol_select).
//
// Convention (include/mtp_mi355x.h): the columns of the file's first raw block S are the selected candidate vectors, the
// second block is W = S^-1, and a candidate c grades gamma = W c (pair_mtp_extrapolation.cpp:347-358).  A swap puts pool
// row i into slot j, S[:, j] <- v_i.  With G = V W^T (G[n, :] = grades of pool row n) and the pivot p = G[i, j], every
// row r of the stacked matrix M = [W^T ; G] takes the same rank-1 update
//     u = (G[i, :] - e_j) / p,      r <- r - r[j] u,
// and |det S| grows by |p|.  M is [(C + N)][cpad] fp64, zero padded: padding columns have u = 0 and stay zero.
//
// Three kernels and a host loop:
//   maxvol_gemm    G = V M[0, C) with v_mfma_f64_16x16x4_f64 (once per refresh, not once per swap)
//   maxvol_update  the hot path: one pass over M applies the swap and leaves every workgroup's (max |G|, linear index)
//   maxvol_pivot   one workgroup folds those maxima, decides, and writes the next pivot record, u and the swap log
// The host enqueues pivot -> update pairs in chunks and reads a 16-byte status once per chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "mtp_device.hpp"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

// compile-time tunables (make variant EXTRA=-D...; DESIGN.md 5.2.1 has the sweep the defaults come from)
#define MTP_MV_STR2(x) #x
#define MTP_MV_STR(x) MTP_MV_STR2(x)
#ifdef MTP_MV_ROWS
#define MTP_MV_ROWS_FLAG "MTP_MV_ROWS=" MTP_MV_STR(MTP_MV_ROWS) " "
#else
#define MTP_MV_ROWS 4
#define MTP_MV_ROWS_FLAG ""
#endif
#ifdef MTP_MV_CHUNK
#define MTP_MV_CHUNK_FLAG "MTP_MV_CHUNK=" MTP_MV_STR(MTP_MV_CHUNK) " "
#else
#define MTP_MV_CHUNK 16
#define MTP_MV_CHUNK_FLAG ""
#endif
#ifdef MTP_MV_WAVES
#define MTP_MV_WAVES_FLAG "MTP_MV_WAVES=" MTP_MV_STR(MTP_MV_WAVES) " "
#else
#define MTP_MV_WAVES 16
#define MTP_MV_WAVES_FLAG ""
#endif
constexpr int kUpdateBlock = 256;             // four wavefronts, one row each at a time
constexpr int kUpdateRows = MTP_MV_ROWS;      // rows a wavefront keeps in flight
constexpr int kChunk = MTP_MV_CHUNK;          // pivot -> update pairs between two status reads
constexpr int kWavesPerCU = MTP_MV_WAVES;     // grid cap: wavefronts per CU (16 = four per SIMD)

// what maxvol_pivot decides; the host reads {done, err, nswaps, pad} (16 bytes) once per chunk
struct MaxvolState {
  int i, j;        // pivot: pool row, slot
  double p;        // G[i][j]
  double maxval;   // largest |G| entry the last pivot search saw
  double pad0;
  int done;        // 1: no entry above the threshold; 2: swap budget used up with one still above it
  int err;         // 1: non-finite maximum
  int nswaps;
  int pad1;
};

// ordering of the pivot search: larger |value| first, ties to the smaller linear index n * C + j
__device__ __forceinline__ void take_max(double &best, long long &bidx, double a, long long idx)
{
  if (a > best || (a == best && idx < bidx)) {
    best = a;
    bidx = idx;
  }
}

__device__ __forceinline__ double abs_or_inf(double v)   // NaN and Inf both order as +Inf: fmax would drop a NaN
{
  const double a = fabs(v);
  return a <= DBL_MAX ? a : HUGE_VAL;
}

__device__ __forceinline__ void block_fold_max(double best, long long bidx, double *part_max, long long *part_idx)
{
  __shared__ double s_max[kUpdateBlock / 64];
  __shared__ long long s_idx[kUpdateBlock / 64];
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) {
    const double ob = __shfl_xor(best, sft, 64);
    const long long oi = __shfl_xor(bidx, sft, 64);
    take_max(best, bidx, ob, oi);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_max[wave] = best;
    s_idx[wave] = bidx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kUpdateBlock / 64; w++) take_max(best, bidx, s_max[w], s_idx[w]);
    part_max[blockIdx.x] = best;
    part_idx[blockIdx.x] = bidx;
  }
}

// G[n][a] = sum_b V[n][b] M[b][a], b < C.  One wavefront owns 16 pool rows and 64 columns (four 16 x 16 tiles); operand
// lane maps as in the grade kernel (mtp_kernels.hip): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15],
// D: col = l & 15, row = (l >> 4) + 4 reg.  V has ld >= C doubles per row and no padding of its own, M has only C rows in
// front of G: both operands are guarded by b < C, pool rows by n < N, columns by a < cpad.
__global__ void __launch_bounds__(256) maxvol_gemm(const double *__restrict__ V, long long N, int ld, int C, int cpad,
                                                   double *__restrict__ M)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n0 = ((long long) blockIdx.x * 4 + wave) * 16;
  if (n0 >= N) return;
  const int li = lane & 15, lk = lane >> 4;
  const int a0 = blockIdx.y * 64;
  const long long arow = n0 + li;
  const double *ap = V + (size_t) (arow < N ? arow : N - 1) * ld;
  const bool arow_ok = arow < N;
  double4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < C; k0 += 4) {
    const int b = k0 + lk;
    const bool bok = b < C;
    const double av = (bok && arow_ok) ? ap[b] : 0.0;
    const double *bp = M + (size_t) (bok ? b : 0) * cpad;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int a = a0 + 16 * t + li;
      const double bv = (bok && a < cpad) ? bp[a] : 0.0;
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
    }
  }
  double *G = M + (size_t) C * cpad;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int a = a0 + 16 * t + li;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const long long n = n0 + lk + 4 * r;
      if (n < N && a < cpad) G[(size_t) n * cpad + a] = acc[t][r];
    }
  }
}

// One pass over the R = C + N rows of M.  A wavefront takes kUpdateRows consecutive rows at a time; lanes run over the
// columns in 16-byte pieces (piece q = lane + 64 t holds columns 2q, 2q + 1; T = pieces per lane, 0: any cpad, a
// row at a time).  r[j] comes from the lane that loaded it.  UPDATE = false only searches (a freshly computed G).
// Each workgroup writes the (max |value|, linear index) of the G rows it touched; the W^T rows take no part.
template <bool UPDATE, int T>
__global__ void __launch_bounds__(kUpdateBlock) maxvol_update(double *__restrict__ M, long long R, int C, int cpad,
                                                              const MaxvolState *__restrict__ state,
                                                              const double *__restrict__ u, double *__restrict__ part_max,
                                                              long long *__restrict__ part_idx)
{
  if (UPDATE && state->done) return;   // (part_max / part_idx keep the values the deciding search read)
  const int lane = threadIdx.x & 63;
  const long long wave = (long long) blockIdx.x * (kUpdateBlock / 64) + (threadIdx.x >> 6);
  const long long nwaves = (long long) gridDim.x * (kUpdateBlock / 64);
  const int pieces = cpad >> 1;
  const int j = UPDATE ? state->j : 0;
  double best = -1.0;
  long long bidx = LLONG_MAX;
  if constexpr (T > 0) {
    const int jt = (j >> 1) >> 6, jl = (j >> 1) & 63, jc = j & 1;
    double2 uu[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
      const int q = lane + 64 * t;
      uu[t] = (UPDATE && q < pieces) ? reinterpret_cast<const double2 *>(u)[q] : make_double2(0.0, 0.0);
    }
    for (long long r0 = wave * kUpdateRows; r0 < R; r0 += nwaves * kUpdateRows) {
      double2 v[kUpdateRows][T];
#pragma unroll
      for (int k = 0; k < kUpdateRows; k++) {
        const double2 *row = reinterpret_cast<const double2 *>(M + (size_t) (r0 + k) * cpad);
#pragma unroll
        for (int t = 0; t < T; t++) {
          const int q = lane + 64 * t;
          v[k][t] = (r0 + k < R && q < pieces) ? row[q] : make_double2(0.0, 0.0);
        }
      }
#pragma unroll
      for (int k = 0; k < kUpdateRows; k++) {
        if (r0 + k >= R) continue;   // (the whole wavefront)
        if (UPDATE) {
          // r[j] from the lane that loaded it: both halves of every piece are handed round and picked by the wavefront-
          // uniform (jt, jc) afterwards -- a pick ahead of the shuffle indexes v[][] dynamically and sends it to scratch
          double rj = 0.0;
#pragma unroll
          for (int t = 0; t < T; t++) {
            const double sx = __shfl(v[k][t].x, jl, 64), sy = __shfl(v[k][t].y, jl, 64);
            if (t == jt) rj = jc ? sy : sx;
          }
          double2 *row = reinterpret_cast<double2 *>(M + (size_t) (r0 + k) * cpad);
#pragma unroll
          for (int t = 0; t < T; t++) {
            const int q = lane + 64 * t;
            v[k][t].x -= rj * uu[t].x;
            v[k][t].y -= rj * uu[t].y;
            if (q < pieces) row[q] = v[k][t];
          }
        }
        if (r0 + k >= C) {
          const long long base = (r0 + k - C) * C;
#pragma unroll
          for (int t = 0; t < T; t++) {
            const int c = 2 * (lane + 64 * t);
            if (c < C) take_max(best, bidx, abs_or_inf(v[k][t].x), base + c);
            if (c + 1 < C) take_max(best, bidx, abs_or_inf(v[k][t].y), base + c + 1);
          }
        }
      }
    }
  } else {
    for (long long r = wave; r < R; r += nwaves) {
      double2 *row = reinterpret_cast<double2 *>(M + (size_t) r * cpad);
      const double rj = UPDATE ? M[(size_t) r * cpad + j] : 0.0;   // one address for the wavefront, read before any store
      for (int q = lane; q < pieces; q += 64) {
        double2 x = row[q];
        if (UPDATE) {
          const double2 w = reinterpret_cast<const double2 *>(u)[q];
          x.x -= rj * w.x;
          x.y -= rj * w.y;
          row[q] = x;
        }
        if (r >= C) {
          const long long base = (r - C) * C;
          if (2 * q < C) take_max(best, bidx, abs_or_inf(x.x), base + 2 * q);
          if (2 * q + 1 < C) take_max(best, bidx, abs_or_inf(x.y), base + 2 * q + 1);
        }
      }
    }
  }
  block_fold_max(best, bidx, part_max, part_idx);
}

// One workgroup.  Folds the nblocks per-workgroup maxima (strided partials, then a tree: the ordering of take_max is total,
// so the winner does not depend on the grid), then decides: non-finite -> err and done; <= threshold -> done = 1; swap
// budget used up -> done = 2; else the pivot record, u = (G[i, :] - e_j) / p, slot_source[j] = i and one more log entry.
__global__ void __launch_bounds__(256) maxvol_pivot(const double *__restrict__ M, int C, int cpad, int nblocks,
                                                    const double *__restrict__ part_max,
                                                    const long long *__restrict__ part_idx, double threshold, int max_swaps,
                                                    MaxvolState *__restrict__ state, double *__restrict__ u,
                                                    int *__restrict__ slot_source, int *__restrict__ log_rows,
                                                    int *__restrict__ log_slots, double *__restrict__ log_pivots)
{
  __shared__ double s_max[256];
  __shared__ long long s_idx[256];
  if (state->done) return;
  double best = -1.0;
  long long bidx = LLONG_MAX;
  for (int b = threadIdx.x; b < nblocks; b += 256) take_max(best, bidx, part_max[b], part_idx[b]);
  s_max[threadIdx.x] = best;
  s_idx[threadIdx.x] = bidx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int) threadIdx.x < s) {
      take_max(s_max[threadIdx.x], s_idx[threadIdx.x], s_max[threadIdx.x + s], s_idx[threadIdx.x + s]);
    }
    __syncthreads();
  }
  best = s_max[0];
  bidx = s_idx[0];
  const int nswaps = state->nswaps;
  __syncthreads();   // every thread has read the state before thread 0 rewrites it
  const bool bad = !(best <= DBL_MAX);
  const bool below = !bad && best <= threshold;
  const bool spent = !bad && !below && nswaps >= max_swaps;
  if (bad || below || spent) {
    if (threadIdx.x == 0) {
      state->maxval = best < 0.0 ? 0.0 : best;
      state->err = bad ? 1 : 0;
      state->done = spent ? 2 : 1;
    }
    return;
  }
  const int i = (int) (bidx / C), j = (int) (bidx % C);
  const double *g = M + ((size_t) C + (size_t) i) * cpad;
  const double p = g[j];
  for (int c = threadIdx.x; c < cpad; c += 256) u[c] = (g[c] - (c == j ? 1.0 : 0.0)) / p;
  if (threadIdx.x == 0) {
    state->i = i;
    state->j = j;
    state->p = p;
    state->maxval = best;
    state->nswaps = nswaps + 1;
    slot_source[j] = i;
    log_rows[nswaps] = i;
    log_slots[nswaps] = j;
    log_pivots[nswaps] = p;
  }
}

// cols[j][c] = V[slot_source[j]][c] for the slots that took a pool row (the new columns of S, bit for bit)
__global__ void __launch_bounds__(256) maxvol_gather(const double *__restrict__ V, int ld, int C,
                                                     const int *__restrict__ slot_source, double *__restrict__ cols)
{
  const int j = blockIdx.x, src = slot_source[j];
  if (src < 0) return;
  for (int c = threadIdx.x; c < C; c += 256) cols[(size_t) j * C + c] = V[(size_t) src * ld + c];
}

// rows[k][:] /= atoms of configuration k (a zero row for an empty one)
__global__ void __launch_bounds__(256) maxvol_scale_rows(double *__restrict__ rows, int cpad, int ncfg,
                                                         const int *__restrict__ cfg_first)
{
  const int k = blockIdx.x;
  const int n = cfg_first[k + 1] - cfg_first[k];
  for (int c = threadIdx.x; c < cpad; c += 256) rows[(size_t) k * cpad + c] = n > 0 ? rows[(size_t) k * cpad + c] / (double) n : 0.0;
}

template <bool UPDATE>
void launch_update(int grid, double *M, long long R, int C, int cpad, const MaxvolState *state, const double *u,
                   double *part_max, long long *part_idx, hipStream_t st)
{
  const int T = (cpad / 2 + 63) / 64;
#define MTP_MAXVOL_CASE(t)                                                                                                  \
  hipLaunchKernelGGL((maxvol_update<UPDATE, t>), dim3(grid), dim3(kUpdateBlock), 0, st, M, R, C, cpad, state, u, part_max, \
                     part_idx)
  if (T == 1)
    MTP_MAXVOL_CASE(1);
  else if (T == 2)
    MTP_MAXVOL_CASE(2);
  else   // cpad above 256: a row at a time
    MTP_MAXVOL_CASE(0);
#undef MTP_MAXVOL_CASE
}

// How mtp_maxvol_run lays its device memory out in one arena of doubles (the int arrays rounded up to whole doubles)
struct Arena {
  int cpad, grid;
  size_t M, u, part_max, part_idx, state, slot, log_i, log_j, log_p, cols, total;   // offsets in doubles
  Arena(int num_cus, int C, long long N, int max_swaps)
  {
    cpad = (C + 15) / 16 * 16;
    const long long R = (long long) C + N;
    // one round of workgroups at every instantiation's register count
    const int nwave_rows = (int) std::min<long long>((R + kUpdateRows - 1) / kUpdateRows, (long long) num_cus * kWavesPerCU);
    grid = std::max(1, (nwave_rows + kUpdateBlock / 64 - 1) / (kUpdateBlock / 64));
    const size_t half = ((size_t) max_swaps + 1) / 2;
    size_t o = 0;
    auto take = [&o](size_t n) {
      const size_t at = o;
      o += (n + 1) / 2 * 2;   // 16-byte pieces
      return at;
    };
    M = take((size_t) R * cpad);
    u = take((size_t) cpad);
    part_max = take((size_t) grid);
    part_idx = take((size_t) grid);
    state = take(sizeof(MaxvolState) / sizeof(double));
    slot = take(((size_t) C + 1) / 2);
    log_i = take(half);
    log_j = take(half);
    log_p = take((size_t) max_swaps);
    cols = take((size_t) C * C);
    total = o;
  }
};
static_assert(sizeof(MaxvolState) % sizeof(double) == 0, "the state is a whole number of doubles");

}   // namespace

const char *mtp_maxvol_build_flags() { return MTP_MV_ROWS_FLAG MTP_MV_CHUNK_FLAG MTP_MV_WAVES_FLAG; }

hipError_t mtp_launch_maxvol_scale_rows(double *rows, int cpad, int ncfg, const int *cfg_first, hipStream_t st)
{
  hipLaunchKernelGGL(maxvol_scale_rows, dim3(ncfg), dim3(256), 0, st, rows, cpad, ncfg, cfg_first);
  return hipGetLastError();
}

#define MV_CHECK(call)                  \
  do {                                  \
    const hipError_t _e = (call);       \
    if (_e != hipSuccess) return _e;    \
  } while (0)

size_t mtp_maxvol_arena_doubles(int num_cus, int C, long long N, int max_swaps)
{
  return Arena(num_cus, C, N, max_swaps).total;
}

hipError_t mtp_maxvol_run(hipStream_t st, int num_cus, double *arena, int C, const double *S, const double *W,
                          const double *d_rows, long long N, int ld, double threshold, int max_swaps, int refresh, double *S_out,
                          double *W_out,
                          int *slot_source, int *swap_rows, int *swap_slots, double *swap_pivots, int *nswaps_out,
                          int *converged, double *max_grade_after, int *nonfinite)
{
  const Arena at(num_cus, C, N, max_swaps);
  const int cpad = at.cpad, grid = at.grid;
  const long long R = (long long) C + N;
  double *M = arena + at.M, *u = arena + at.u, *part_max = arena + at.part_max, *log_p = arena + at.log_p;
  double *cols = arena + at.cols;
  long long *part_idx = reinterpret_cast<long long *>(arena + at.part_idx);
  MaxvolState *state = reinterpret_cast<MaxvolState *>(arena + at.state);
  int *d_slot = reinterpret_cast<int *>(arena + at.slot), *log_i = reinterpret_cast<int *>(arena + at.log_i);
  int *log_j = reinterpret_cast<int *>(arena + at.log_j);
  // W^T, zero padded, in front of G
  std::vector<double> wt((size_t) C * cpad, 0.0);
  for (int a = 0; a < C; a++)
    for (int b = 0; b < C; b++) wt[(size_t) b * cpad + a] = W[(size_t) a * C + b];
  MV_CHECK(hipMemcpyAsync(M, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice, st));
  MV_CHECK(hipMemsetAsync(state, 0, sizeof(MaxvolState), st));
  MV_CHECK(hipMemsetAsync(d_slot, 0xff, (size_t) C * sizeof(int), st));   // -1: the original column
  MV_CHECK(hipMemsetAsync(u, 0, (size_t) cpad * sizeof(double), st));

  int status[4] = {0, 0, 0, 0};   // done, err, nswaps, pad
  auto read_status = [&]() -> hipError_t {
    MV_CHECK(hipMemcpyAsync(status, &state->done, sizeof(status), hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
  };
  auto pivot = [&]() -> hipError_t {
    hipLaunchKernelGGL(maxvol_pivot, dim3(1), dim3(256), 0, st, M, C, cpad, grid, part_max, part_idx, threshold, max_swaps,
                       state, u, d_slot, log_i, log_j, log_p);
    return hipGetLastError();
  };
  // A round: fresh grades from V and the current W, the search over them, then up to `refresh` pivot -> update pairs in
  // chunks.  A pair after `done` is set returns at once, so a chunk may run past the decision.  A decision taken on
  // rank-1-updated grades only ends the round; the call ends on a decision the first pivot of a round takes, on fresh ones.
  bool finished = false;
  while (!finished) {
    hipLaunchKernelGGL(maxvol_gemm, dim3((unsigned) ((N + 63) / 64), (cpad + 63) / 64), dim3(256), 0, st, d_rows, N, ld, C,
                       cpad, M);
    MV_CHECK(hipGetLastError());
    launch_update<false>(grid, M, R, C, cpad, state, u, part_max, part_idx, st);
    MV_CHECK(hipGetLastError());
    const int at_refresh = status[2];
    for (int queued = 0; queued < refresh;) {
      const int n = std::min(kChunk, refresh - queued);
      for (int k = 0; k < n; k++) {
        MV_CHECK(pivot());
        launch_update<true>(grid, M, R, C, cpad, state, u, part_max, part_idx, st);
        MV_CHECK(hipGetLastError());
      }
      queued += n;
      MV_CHECK(read_status());
      if (!status[0]) continue;
      if (status[1] || status[2] == at_refresh)
        finished = true;
      else
        MV_CHECK(hipMemsetAsync(&state->done, 0, sizeof(int), st));
      break;
    }
  }
  const bool conv = status[0] == 1 && !status[1];
  const int ns = status[2];
  *nswaps_out = ns;
  *converged = conv ? 1 : 0;
  *nonfinite = status[1];
  MaxvolState hs;
  std::vector<double> wt_out((size_t) C * cpad), hcols((size_t) C * C);
  hipLaunchKernelGGL(maxvol_gather, dim3(C), dim3(256), 0, st, d_rows, ld, C, d_slot, cols);
  MV_CHECK(hipGetLastError());
  MV_CHECK(hipMemcpyAsync(&hs, state, sizeof(hs), hipMemcpyDeviceToHost, st));
  MV_CHECK(hipMemcpyAsync(wt_out.data(), M, wt_out.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  MV_CHECK(hipMemcpyAsync(hcols.data(), cols, hcols.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  MV_CHECK(hipMemcpyAsync(slot_source, d_slot, (size_t) C * sizeof(int), hipMemcpyDeviceToHost, st));
  if (ns > 0) {
    MV_CHECK(hipMemcpyAsync(swap_rows, log_i, (size_t) ns * sizeof(int), hipMemcpyDeviceToHost, st));
    MV_CHECK(hipMemcpyAsync(swap_slots, log_j, (size_t) ns * sizeof(int), hipMemcpyDeviceToHost, st));
    MV_CHECK(hipMemcpyAsync(swap_pivots, log_p, (size_t) ns * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  MV_CHECK(hipStreamSynchronize(st));
  *max_grade_after = hs.maxval;
  std::memcpy(S_out, S, (size_t) C * C * sizeof(double));
  for (int j = 0; j < C; j++) {
    if (slot_source[j] < 0) continue;
    for (int c = 0; c < C; c++) S_out[(size_t) c * C + j] = hcols[(size_t) j * C + c];
  }
  for (int a = 0; a < C; a++)
    for (int b = 0; b < C; b++) W_out[(size_t) a * C + b] = wt_out[(size_t) b * cpad + a];
  return hipSuccess;
}
