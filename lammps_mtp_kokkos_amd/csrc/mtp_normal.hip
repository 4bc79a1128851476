// Normal equations of the linear refit in double-double (include/mtp_mi355x.h, "linear refit without the design matrix").
//
// The state holds, per kind of row (energy, force, virial), the augmented Gram matrix G = B^T B of n = ncols + 1 columns as
// two [n][n] fp64 planes hi and lo, and the number of rows that entered (rows whose scale is not zero).  Column ncols of B
// is the target.  B is never stored: b[i][c] = fl(scale[i] * rows[i][c]) is formed when a row panel is staged into LDS.
//
//   normal_accumulate_kernel   one workgroup per (tile pair (tj <= tk) of the upper triangle, slice of MTP_NM_SLICE rows).
//                              256 threads, a 64 x 64 tile, a 4 x 4 micro-tile of double-double accumulators per thread
//                              (entries (ty + 16 a, tx + 16 b): LDS reads of a wavefront are a broadcast and a contiguous
//                              run), MTP_NM_PANEL rows of both tile columns in LDS, the next panel's loads in flight while
//                              the current one is consumed.  10 fp64 VALU instructions per multiply-add (dd_mac).  The
//                              normalised partial tile goes to the workspace; no atomics, no MFMA (v_mfma_f64 returns no
//                              rounding error term).
//   normal_fold_kernel         adds the slices' partial tiles to the state in slice order (dd_add) and writes both
//                              triangles from the same value; adds the row count.
//
// The slice length is a compile-time constant, so the order of every sum -- and with it every bit of the result -- is the
// same on any device and for any nrows.  When a call has more slices than the workspace holds, the launcher runs several
// rounds of accumulate + fold, cut at slice boundaries and folded in order: the result does not depend on the cuts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "../../include/mtp_mi355x.h"
#include "mtp_device.hpp"
#include "mtp_dd.hpp"

// ---- make variant tunables (mtp_build_flags names the ones that differ from the shipped values) --------------------------
#define MTP_NM_STR2(x) #x
#define MTP_NM_STR(x) MTP_NM_STR2(x)
#ifdef MTP_NM_PANEL
#define MTP_NM_PANEL_FLAG "MTP_NM_PANEL=" MTP_NM_STR(MTP_NM_PANEL) " "
#else
#define MTP_NM_PANEL 16          // rows staged in LDS at a time
#define MTP_NM_PANEL_FLAG ""
#endif
#ifdef MTP_NM_SLICE
#define MTP_NM_SLICE_FLAG "MTP_NM_SLICE=" MTP_NM_STR(MTP_NM_SLICE) " "
#else
#define MTP_NM_SLICE 256         // rows of one workgroup: the unit of the sum order
#define MTP_NM_SLICE_FLAG ""
#endif
#ifdef MTP_NM_WS_MIB
#define MTP_NM_WS_MIB_FLAG "MTP_NM_WS_MIB=" MTP_NM_STR(MTP_NM_WS_MIB) " "
#else
#define MTP_NM_WS_MIB 256        // the fixed cap of the workspace
#define MTP_NM_WS_MIB_FLAG ""
#endif
static_assert(MTP_NM_PANEL >= 1 && MTP_NM_SLICE % MTP_NM_PANEL == 0, "a slice is a whole number of panels");
static_assert(MTP_NM_SLICE >= 1 && MTP_NM_SLICE <= 256, "the row count of a slice is taken by one pass of 256 threads");
static_assert(MTP_NM_WS_MIB >= 1, "workspace cap");

const char *mtp_normal_build_flags() { return MTP_NM_PANEL_FLAG MTP_NM_SLICE_FLAG MTP_NM_WS_MIB_FLAG; }

namespace {

constexpr int TILE = 64;                                   // 16 x 16 threads, 4 x 4 entries each
constexpr int TILE_ENTRIES = TILE * TILE;
constexpr size_t TILE_BYTES = (size_t) TILE_ENTRIES * 2 * sizeof(double);   // hi and lo planes of one partial tile
constexpr int MAX_ROUND_SLICES = 256;                      // slices of one round (grid y)
constexpr int PANEL_LOADS = MTP_NM_PANEL * TILE / 256;     // doubles a thread stages per tile column and panel
static_assert(MTP_NM_PANEL * TILE % 256 == 0, "a panel is staged by whole passes of 256 threads");

// the tile pair (tj <= tk) of index p in row-major order of the upper triangle
__device__ __forceinline__ void pair_of(int p, int ntiles, int &tj, int &tk)
{
  int j = 0;
  while (p >= ntiles - j) {
    p -= ntiles - j;
    j++;
  }
  tj = j;
  tk = j + p;
}

// b[i][c] of one staged element: rows of scale 0 and rows behind nrows are never read; column ncols is the target; columns
// behind it are zero (rows[i][c] for c >= ncols is never read)
__device__ __forceinline__ double staged(const double *__restrict__ rows, const double *__restrict__ scale,
                                         const double *__restrict__ target, long long nrows, int ld, int ncols, long long i, int c)
{
  if (i >= nrows || c > ncols) return 0.0;
  const double s = scale[i];
  if (s == 0.0) return 0.0;
  return s * (c < ncols ? rows[(size_t) i * ld + c] : target[i]);
}

__global__ void __launch_bounds__(256) normal_accumulate_kernel(const double *__restrict__ rows, const double *__restrict__ scale,
                                                                const double *__restrict__ target, long long row0, long long nrows,
                                                                int ld, int ncols, int ntiles, int npairs,
                                                                double *__restrict__ ws, unsigned long long *__restrict__ ws_count)
{
  __shared__ double pa[MTP_NM_PANEL][TILE];
  __shared__ double pb[MTP_NM_PANEL][TILE];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int pair = blockIdx.x, slice = blockIdx.y;
  int tj, tk;
  pair_of(pair, ntiles, tj, tk);
  const long long first = row0 + (long long) slice * MTP_NM_SLICE;     // the slice's first row (all rows of the call: [0, nrows))

  if (pair == 0) {   // the rows of this slice that enter: counted once per slice
    const long long i = first + tid;
    const int c = __syncthreads_count(tid < MTP_NM_SLICE && i < nrows && scale[i] != 0.0);
    if (tid == 0) ws_count[slice] = (unsigned long long) c;
  }

  mtp_dd acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = mtp_dd{0.0, 0.0};

  // element e = tid + 256 l of a panel: row e / 64, tile column e % 64 (a wavefront reads 64 consecutive doubles of a row)
  double ra[PANEL_LOADS], rb[PANEL_LOADS];
#pragma unroll
  for (int l = 0; l < PANEL_LOADS; l++) {
    const int e = tid + 256 * l;
    const long long i = first + (e >> 6);
    ra[l] = staged(rows, scale, target, nrows, ld, ncols, i, tj * TILE + (e & 63));
    rb[l] = tj == tk ? 0.0 : staged(rows, scale, target, nrows, ld, ncols, i, tk * TILE + (e & 63));
  }
  for (int p0 = 0; p0 < MTP_NM_SLICE; p0 += MTP_NM_PANEL) {
    __syncthreads();   // the panel before this one has been consumed
#pragma unroll
    for (int l = 0; l < PANEL_LOADS; l++) {
      const int e = tid + 256 * l;
      pa[e >> 6][e & 63] = ra[l];
      pb[e >> 6][e & 63] = tj == tk ? ra[l] : rb[l];
    }
    __syncthreads();
    const int p1 = p0 + MTP_NM_PANEL;
    if (p1 < MTP_NM_SLICE && first + p1 < nrows) {   // the next panel's loads, in flight during the arithmetic below
#pragma unroll
      for (int l = 0; l < PANEL_LOADS; l++) {
        const int e = tid + 256 * l;
        const long long i = first + p1 + (e >> 6);
        ra[l] = staged(rows, scale, target, nrows, ld, ncols, i, tj * TILE + (e & 63));
        rb[l] = tj == tk ? 0.0 : staged(rows, scale, target, nrows, ld, ncols, i, tk * TILE + (e & 63));
      }
    }
    if (first + p0 < nrows) {   // (a panel wholly behind nrows holds zeros: adding them changes no bit)
#pragma unroll 4
      for (int r = 0; r < MTP_NM_PANEL; r++) {
        double xa[4], xb[4];
#pragma unroll
        for (int a = 0; a < 4; a++) xa[a] = pa[r][ty + 16 * a];
#pragma unroll
        for (int b = 0; b < 4; b++) xb[b] = pb[r][tx + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int b = 0; b < 4; b++) acc[a][b] = dd_mac(acc[a][b], xa[a], xb[b]);
      }
    }
  }
  // the partial tile of (slice, pair): hi plane, then lo plane, entry (ty + 16 a) * 64 + tx + 16 b
  double *out = ws + ((size_t) slice * npairs + pair) * (2 * TILE_ENTRIES);
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const mtp_dd v = dd_normal(acc[a][b]);
      const int e = (ty + 16 * a) * TILE + tx + 16 * b;
      out[e] = v.hi;
      out[TILE_ENTRIES + e] = v.lo;
    }
}

// grid (npairs, 16): thread e of a tile pair adds its entry of every slice, in slice order, to the state and writes it to
// (j, k) and (k, j); on a diagonal tile only j <= k is taken, so both triangles come from one value
__global__ void __launch_bounds__(256) normal_fold_kernel(const double *__restrict__ ws, const unsigned long long *__restrict__ ws_count,
                                                          int nslices, int n, int ntiles, int npairs, double *__restrict__ hi,
                                                          double *__restrict__ lo, unsigned long long *__restrict__ count)
{
  const int pair = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
  if (pair == 0 && e == 0) {
    unsigned long long c = *count;
    for (int s = 0; s < nslices; s++) c += ws_count[s];
    *count = c;
  }
  int tj, tk;
  pair_of(pair, ntiles, tj, tk);
  const int j = tj * TILE + (e >> 6), k = tk * TILE + (e & 63);
  if (j >= n || k >= n || j > k) return;
  mtp_dd g{hi[(size_t) j * n + k], lo[(size_t) j * n + k]};
  for (int s = 0; s < nslices; s++) {
    const double *t = ws + ((size_t) s * npairs + pair) * (2 * TILE_ENTRIES);
    g = dd_add(g, mtp_dd{t[e], t[TILE_ENTRIES + e]});
  }
  hi[(size_t) j * n + k] = g.hi;
  lo[(size_t) j * n + k] = g.lo;
  hi[(size_t) k * n + j] = g.hi;
  lo[(size_t) k * n + j] = g.lo;
}

__global__ void __launch_bounds__(256) normal_zero_kernel(double *__restrict__ g, size_t ndoubles, unsigned long long *__restrict__ count)
{
  const size_t stride = (size_t) gridDim.x * 256;
  for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < ndoubles; i += stride) g[i] = 0.0;
  if (blockIdx.x == 0 && threadIdx.x < 3) count[threadIdx.x] = 0ull;
}

}   // namespace

struct mtp_normal {
  int device = 0;
  int ncols = 0, n = 0, ntiles = 0, npairs = 0;
  double *d_g = nullptr;                   // [3 kinds][2 planes][n][n]
  unsigned long long *d_count = nullptr;   // [3]
  double *d_ws = nullptr;                  // partial tiles of one round: [slices][npairs][2][64][64]
  unsigned long long *d_ws_count = nullptr;   // [MAX_ROUND_SLICES]
  size_t ws_bytes = 0;
  int round_slices = 0;                    // slices one round may hold: ws_bytes / (npairs * TILE_BYTES), at most MAX_ROUND_SLICES
  std::string last_error;
};

int mtp_normal_sizes(int *tile, int *panel, int *slice, long long *workspace_cap_bytes)
{
  if (tile) *tile = TILE;
  if (panel) *panel = MTP_NM_PANEL;
  if (slice) *slice = MTP_NM_SLICE;
  if (workspace_cap_bytes) *workspace_cap_bytes = (long long) MTP_NM_WS_MIB << 20;
  return MTP_OK;
}

const char *mtp_normal_last_error(const mtp_normal *h) { return h ? h->last_error.c_str() : "null normal state"; }

namespace {
int normal_fail(mtp_normal *h, const char *what, hipError_t e)
{
  h->last_error = std::string(what) + ": " + hipGetErrorString(e);
  return MTP_ERR_DEVICE;
}
}   // namespace

#define NM_HIP(h, call)                                         \
  do {                                                          \
    hipError_t _e = (call);                                     \
    if (_e != hipSuccess) return normal_fail(h, #call, _e);     \
  } while (0)

int mtp_normal_create(int device_id, int ncols, long long workspace_bytes, mtp_normal **out)
{
  if (!out) return MTP_ERR_ARG;
  *out = nullptr;
  if (ncols < 1 || ncols > 32766 || workspace_bytes < 0) return MTP_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return MTP_ERR_DEVICE;
  mtp_normal *h = new (std::nothrow) mtp_normal();
  if (!h) return MTP_ERR_ARG;
  h->device = device_id;
  h->ncols = ncols;
  h->n = ncols + 1;
  h->ntiles = (h->n + TILE - 1) / TILE;
  h->npairs = h->ntiles * (h->ntiles + 1) / 2;
  // the workspace: whole rounds of slices, at least one slice, at most the fixed cap and MAX_ROUND_SLICES slices
  const size_t per_slice = (size_t) h->npairs * TILE_BYTES;
  const size_t cap = (size_t) MTP_NM_WS_MIB << 20;
  size_t want = workspace_bytes > 0 ? (size_t) workspace_bytes : cap;
  size_t slices = std::min(std::min(want, cap) / per_slice, (size_t) MAX_ROUND_SLICES);
  if (slices < 1) slices = 1;
  h->round_slices = (int) slices;
  h->ws_bytes = slices * per_slice;
  const size_t g_doubles = (size_t) 6 * h->n * h->n;
  hipError_t e = hipSetDevice(device_id);
  if (e == hipSuccess) e = hipMalloc((void **) &h->d_g, g_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **) &h->d_count, 3 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void **) &h->d_ws, h->ws_bytes);
  if (e == hipSuccess) e = hipMalloc((void **) &h->d_ws_count, MAX_ROUND_SLICES * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(h->d_g, 0, g_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMemset(h->d_count, 0, 3 * sizeof(unsigned long long));
  if (e != hipSuccess) {
    mtp_normal_destroy(h);
    return MTP_ERR_DEVICE;
  }
  *out = h;
  return MTP_OK;
}

void mtp_normal_destroy(mtp_normal *h)
{
  if (!h) return;
  if (h->d_g) (void) hipFree(h->d_g);
  if (h->d_count) (void) hipFree(h->d_count);
  if (h->d_ws) (void) hipFree(h->d_ws);
  if (h->d_ws_count) (void) hipFree(h->d_ws_count);
  delete h;
}

int mtp_normal_info(const mtp_normal *h, int *ncols, int *round_slices, long long *workspace_bytes, long long *state_bytes)
{
  if (!h) return MTP_ERR_ARG;
  if (ncols) *ncols = h->ncols;
  if (round_slices) *round_slices = h->round_slices;
  if (workspace_bytes) *workspace_bytes = (long long) h->ws_bytes;
  if (state_bytes) *state_bytes = (long long) ((size_t) 6 * h->n * h->n * sizeof(double));
  return MTP_OK;
}

int mtp_normal_set_round_slices(mtp_normal *h, int slices)
{
  // fewer slices a round than the workspace holds (tests: the result must not depend on where the rounds are cut)
  if (!h || slices < 1 || (size_t) slices * h->npairs * TILE_BYTES > h->ws_bytes || slices > MAX_ROUND_SLICES) return MTP_ERR_ARG;
  h->round_slices = slices;
  return MTP_OK;
}

static int normal_null_stream(mtp_normal *h, const char *fn)
{
  h->last_error = std::string(fn) + ": a NULL stream is not accepted (the state has no stream of its own)";
  return MTP_ERR_ARG;
}

int mtp_normal_clear(mtp_normal *h, void *stream)
{
  if (!h) return MTP_ERR_ARG;
  if (!stream) return normal_null_stream(h, "mtp_normal_clear");
  NM_HIP(h, hipSetDevice(h->device));
  const size_t nd = (size_t) 6 * h->n * h->n;
  const int grid = (int) std::min((nd + 255) / 256, (size_t) 4096);
  hipLaunchKernelGGL(normal_zero_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), h->d_g, nd, h->d_count);
  NM_HIP(h, hipGetLastError());
  return MTP_OK;
}

int mtp_normal_accumulate(mtp_normal *h, void *stream, int kind, long long nrows, int ld, const double *d_rows,
                          const double *d_scale, const double *d_target)
{
  if (!h) return MTP_ERR_ARG;
  if (!stream) return normal_null_stream(h, "mtp_normal_accumulate");
  if (kind < 0 || kind > 2 || nrows < 0 || ld < h->ncols || (nrows > 0 && (!d_rows || !d_scale || !d_target))) {
    h->last_error = "mtp_normal_accumulate: needs kind in 0..2, nrows >= 0, ld >= ncols and, with rows, all three arrays";
    return MTP_ERR_ARG;
  }
  if (nrows == 0) return MTP_OK;
  NM_HIP(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t plane = (size_t) h->n * h->n;
  double *hi = h->d_g + (size_t) kind * 2 * plane, *lo = hi + plane;
  const long long nslices = (nrows + MTP_NM_SLICE - 1) / MTP_NM_SLICE;
  for (long long s0 = 0; s0 < nslices; s0 += h->round_slices) {
    const int ns = (int) std::min<long long>(h->round_slices, nslices - s0);
    hipLaunchKernelGGL(normal_accumulate_kernel, dim3(h->npairs, ns), dim3(256), 0, st, d_rows, d_scale, d_target,
                       s0 * MTP_NM_SLICE, nrows, ld, h->ncols, h->ntiles, h->npairs, h->d_ws, h->d_ws_count);
    hipLaunchKernelGGL(normal_fold_kernel, dim3(h->npairs, TILE_ENTRIES / 256), dim3(256), 0, st, h->d_ws, h->d_ws_count, ns, h->n,
                       h->ntiles, h->npairs, hi, lo, h->d_count + kind);
  }
  NM_HIP(h, hipGetLastError());
  return MTP_OK;
}

int mtp_normal_get(mtp_normal *h, void *stream, double *hi, double *lo, long long counts[3])
{
  if (!h) return MTP_ERR_ARG;
  if (!stream) return normal_null_stream(h, "mtp_normal_get");
  NM_HIP(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t plane = (size_t) h->n * h->n;
  for (int k = 0; k < 3; k++) {
    if (hi) NM_HIP(h, hipMemcpyAsync(hi + k * plane, h->d_g + (size_t) k * 2 * plane, plane * sizeof(double), hipMemcpyDeviceToHost, st));
    if (lo) NM_HIP(h, hipMemcpyAsync(lo + k * plane, h->d_g + (size_t) k * 2 * plane + plane, plane * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  unsigned long long c[3] = {0, 0, 0};
  if (counts) NM_HIP(h, hipMemcpyAsync(c, h->d_count, sizeof(c), hipMemcpyDeviceToHost, st));
  NM_HIP(h, hipStreamSynchronize(st));
  if (counts)
    for (int k = 0; k < 3; k++) counts[k] = (long long) c[k];
  return MTP_OK;
}

int mtp_normal_set(mtp_normal *h, void *stream, const double *hi, const double *lo, const long long counts[3])
{
  if (!h || !hi || !lo || !counts || counts[0] < 0 || counts[1] < 0 || counts[2] < 0) return MTP_ERR_ARG;
  if (!stream) return normal_null_stream(h, "mtp_normal_set");
  NM_HIP(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t plane = (size_t) h->n * h->n;
  for (int k = 0; k < 3; k++) {
    NM_HIP(h, hipMemcpyAsync(h->d_g + (size_t) k * 2 * plane, hi + k * plane, plane * sizeof(double), hipMemcpyHostToDevice, st));
    NM_HIP(h, hipMemcpyAsync(h->d_g + (size_t) k * 2 * plane + plane, lo + k * plane, plane * sizeof(double), hipMemcpyHostToDevice, st));
  }
  const unsigned long long c[3] = {(unsigned long long) counts[0], (unsigned long long) counts[1], (unsigned long long) counts[2]};
  NM_HIP(h, hipMemcpyAsync(h->d_count, c, sizeof(c), hipMemcpyHostToDevice, st));
  NM_HIP(h, hipStreamSynchronize(st));
  return MTP_OK;
}
