// Device-resident pieces of a standalone MD step either side of the force call --
// what LAMMPS core does around Pair::compute and the reference therefore does not contain: the periodic ghost
// images of one GPU's own atoms (Comm::borders for one rank: rebuilt at every re-neighbouring), their per-step
// refresh and the fold of their forces onto the owners (Comm::forward_comm / reverse_comm; the pair style writes
// forces onto ghosts, /root/reference/LAMMPS/ML-MTP/pair_mtp.cpp:252-254, 315), and the two halves of a
// velocity-Verlet step (fix nve).  Positions, velocities, forces, ghost maps and the neighbour list stay in HBM;
// the host sees one integer (the ghost count) per re-neighbouring.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "../../include/mtp_mi355x.h"
#include "mtp_device.hpp"

namespace {

struct Box3 {
  double len[3], rg;
};

// number of periodic images (other than the atom itself) of wrapped position p that fall inside the shell
// [-rg, len + rg) around the box: per direction the atom has an image above the box when p < rg and one below when
// p >= len - rg (the bounds of lammps_mtp_kokkos_amd/driver.py make_ghosts)
__device__ __forceinline__ int image_flags(const Box3 &b, const double *p, int lo[3], int hi[3])
{
  int n = 1;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = p[a] >= b.len[a] - b.rg ? -1 : 0;   // shift -1 allowed
    hi[a] = p[a] < b.rg ? 1 : 0;                // shift +1 allowed
    n *= 1 + hi[a] - lo[a];
  }
  return n - 1;
}

// wraps the owned atoms into [0, len) and counts their ghost images
__global__ void __launch_bounds__(256) ghosts_count_kernel(Box3 b, double *__restrict__ x, int n, int *__restrict__ count)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double p[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    double v = x[3 * (size_t) i + a];
    v -= floor(v / b.len[a]) * b.len[a];
    if (v >= b.len[a]) v -= b.len[a];   // floor() rounding at the upper edge
    p[a] = v;
    x[3 * (size_t) i + a] = v;
  }
  int lo[3], hi[3];
  count[i] = image_flags(b, p, lo, hi);
}

// ghost k of atom i (images in lexicographic shift order) -> owner[k], shift[k]
__global__ void __launch_bounds__(256) ghosts_fill_kernel(Box3 b, const double *__restrict__ x, int n,
                                                         const int *__restrict__ first, int *__restrict__ owner,
                                                         double *__restrict__ shift, int capacity)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {x[3 * (size_t) i], x[3 * (size_t) i + 1], x[3 * (size_t) i + 2]};
  int lo[3], hi[3];
  (void) image_flags(b, p, lo, hi);
  int k = first[i];
  for (int sx = lo[0]; sx <= hi[0]; sx++)
    for (int sy = lo[1]; sy <= hi[1]; sy++)
      for (int sz = lo[2]; sz <= hi[2]; sz++) {
        if (sx == 0 && sy == 0 && sz == 0) continue;
        if (k < capacity) {
          owner[k] = i;
          shift[3 * (size_t) k] = sx * b.len[0];
          shift[3 * (size_t) k + 1] = sy * b.len[1];
          shift[3 * (size_t) k + 2] = sz * b.len[2];
        }
        k++;
      }
}

// ---- any periodic cell, one or many (mtp_ghosts_build_cell, mtp_ghosts_build_batch): rows of h are the lattice vectors,
// hinv its inverse, s = x . hinv the fractional coordinates, m[a] = rghost / (spacing of the lattice planes normal to
// direction a).  The image of an atom under the integer shift n is a ghost iff -m[a] <= s[a] + n[a] < 1 + m[a] in all three
// directions (the slab criterion of LAMMPS' triclinic ghost cutoffs): separable, so the allowed n[a] form the closed range
// below and nothing is looped over.  ONE criterion (wrap_and_count, shift_of) and TWO sources of the cell (OneCell,
// SlotCells): the numpy twins in driver.py agree bit for bit with both builds because the arithmetic below is rounded one
// operation at a time, in this order, in this one place.
struct Cell9 {
  double h[9], hinv[9], m[3];
};

// per-atom shift ranges as the count pass found them; the fill pass reads them back instead of deriving them again from
// the wrapped Cartesian position ((s . h) . hinv may land one ulp on the other side of a bound, and the fill would then
// write past its atom's slots)
struct alignas(16) ShiftRange {
  int lo[3], cnt[3], pad[2];   // n[a] in [lo[a], lo[a] + cnt[a]); pad[0] the configuration; 32 bytes, two 16-byte stores / loads
};

// wraps p into s in [0, 1)^3 of the cell -> w = s . h (+ org when there is one: a separate rounded add, and none at all
// without, since + 0.0 would turn a -0.0 coordinate into +0.0), the shift ranges r.lo / r.cnt, and the number of images,
// saturated at 2^32 - 1 (2^31 atoms of these still sum below 2^64)
__device__ __forceinline__ unsigned long long wrap_and_count(const double *__restrict__ h, const double *__restrict__ hinv,
                                                             const double *__restrict__ m, const double *__restrict__ org,
                                                             const double p[3], double w[3], ShiftRange &r)
{
  double s[3];
  unsigned long long prod = 1;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    // (products and sums rounded one by one, in this order: the numpy twin in driver.make_ghosts_cell does the same)
    double v = __dadd_rn(__dadd_rn(__dmul_rn(p[0], hinv[a]), __dmul_rn(p[1], hinv[3 + a])), __dmul_rn(p[2], hinv[6 + a]));
    v -= floor(v);
    if (!(v < 1.0)) v = 0.0;   // floor() rounding at the upper edge (and a non-finite coordinate: counted from 0)
    s[a] = v;
    const double lo = ceil(-m[a] - v), hi = ceil(1.0 + m[a] - v) - 1.0;   // lo <= 0 <= hi
    r.lo[a] = (int) fmax(lo, -1073741824.0);
    r.cnt[a] = (int) fmin(hi - lo + 1.0, 1073741824.0);
    prod = prod > 0xffffffffull ? prod : prod * (unsigned long long) r.cnt[a];   // stays below 2^63
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    w[a] = __dadd_rn(__dadd_rn(__dmul_rn(s[0], h[a]), __dmul_rn(s[1], h[3 + a])), __dmul_rn(s[2], h[6 + a]));
    if (org) w[a] = __dadd_rn(w[a], org[a]);   // (the ghosts follow through owner + shift)
  }
  return prod - 1 > 0xffffffffull ? 0xffffffffull : prod - 1;
}

// image e of an atom (its box of shifts in lexicographic order, the zero shift left out) -> sh = n . h
__device__ __forceinline__ void shift_of(const ShiftRange &r, int e, const double *__restrict__ h, double sh[3])
{
  const int zero = (-r.lo[0] * r.cnt[1] - r.lo[1]) * r.cnt[2] - r.lo[2];   // where the atom itself would stand
  if (e >= zero) e++;
  const int q = e / r.cnt[2];
  const double n2 = r.lo[2] + (e - q * r.cnt[2]);
  const int q1 = q / r.cnt[1];
  const double n1 = r.lo[1] + (q - q1 * r.cnt[1]), n0 = r.lo[0] + q1;
#pragma unroll
  for (int a = 0; a < 3; a++) sh[a] = __dadd_rn(__dadd_rn(__dmul_rn(n0, h[a]), __dmul_rn(n1, h[3 + a])), __dmul_rn(n2, h[6 + a]));
}

// the last k < n with first[k] <= i (first[0] = 0 <= i): the owner of ghost i among the scanned offsets, the configuration
// of owned row i among cfg_first (empty configurations share their start with the next one, which this skips).  (A 16-ary
// search, 15 independent probes a round, measured slower on MI355X: 17 us against 7.5 us for 31 773 ghosts of 65 536 atoms.)
__device__ __forceinline__ int last_at_or_below(const int *__restrict__ first, int n, int i)
{
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (first[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// where the cell of a row comes from.  One cell for every row: a kernel argument by value, so h, hinv and m stay in scalar
// registers; no origin.
struct OneCell {
  Cell9 c;
  __device__ __forceinline__ int cfg_of_row(int) const { return 0; }
  __device__ __forceinline__ const Cell9 &cell(int) const { return c; }
  __device__ __forceinline__ const double *origin(int) const { return nullptr; }
};

// Many cells in one pass: owned atoms of configuration k are rows [cfg_first[k], cfg_first[k + 1]); slot[k] holds its cell
// and the origin its images are translated by (mtp_batch_layout keeps the slots of two configurations at least the list
// cutoff apart).
struct CellSlot {
  Cell9 c;
  double org[3];
};
struct SlotCells {
  const CellSlot *slot;
  const int *cfg_first;
  int ncfg;
  __device__ __forceinline__ int cfg_of_row(int i) const { return last_at_or_below(cfg_first, ncfg, i); }
  __device__ __forceinline__ const Cell9 &cell(int cfg) const { return slot[cfg].c; }
  __device__ __forceinline__ const double *origin(int cfg) const { return slot[cfg].org; }
};

// wraps the owned atoms into their cells and counts their images; the shift ranges and the configuration go to range[] for
// the fill pass.  SUM64 (only when the host cannot rule out a total beyond int from the margins alone): count[i] saturates
// at INT_MAX and the exact total goes to *total64, one atomic per block, so that such a total is seen on the host rather
// than wrapped by the scan
template <class Cells, bool SUM64>
__global__ void __launch_bounds__(256) ghosts_cell_count_kernel(Cells cells, double *__restrict__ x, int n, int *__restrict__ count,
                                                               ShiftRange *__restrict__ range,
                                                               unsigned long long *__restrict__ total64)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned long long mine = 0;
  if (i < n) {
    const int cfg = cells.cfg_of_row(i);
    const Cell9 &c = cells.cell(cfg);
    const double p[3] = {x[3 * (size_t) i], x[3 * (size_t) i + 1], x[3 * (size_t) i + 2]};
    double w[3];
    ShiftRange r;
    mine = wrap_and_count(c.h, c.hinv, c.m, cells.origin(cfg), p, w, r);
    r.pad[0] = cfg;
    r.pad[1] = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) x[3 * (size_t) i + a] = w[a];
    count[i] = mine > 0x7fffffffull ? 0x7fffffff : (int) mine;
    range[i] = r;
  }
  if (SUM64) {
    typedef hipcub::BlockReduce<unsigned long long, 256> Red;
    __shared__ typename Red::TempStorage tmp;
    const unsigned long long bsum = Red(tmp).Sum(mine);
    if (threadIdx.x == 0 && bsum) atomicAdd(total64, bsum);
  }
}

// one lane per GHOST (a 1-atom cell has hundreds of images of its one atom): the owner is the last atom whose scanned
// offset is <= k (first[n] = total > k), the shift triple comes from the position of k in that atom's box of shifts and
// the cell of the owner's configuration -> owner[k], shift[k]
template <class Cells>
__global__ void __launch_bounds__(256) ghosts_cell_fill_kernel(Cells cells, int n, int total, const int *__restrict__ first,
                                                              const ShiftRange *__restrict__ range, int *__restrict__ owner,
                                                              double *__restrict__ shift, int capacity)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= total || k >= capacity) return;
  const int i = last_at_or_below(first, n, k);
  const ShiftRange r = range[i];
  double sh[3];
  shift_of(r, k - first[i], cells.cell(r.pad[0]).h, sh);
  owner[k] = i;
#pragma unroll
  for (int a = 0; a < 3; a++) shift[3 * (size_t) k + a] = sh[a];
}

// x[nlocal + k] = x[owner[k]] + shift[k]   (one lane per coordinate)
__global__ void __launch_bounds__(256) ghosts_forward_kernel(double *__restrict__ x, int nlocal,
                                                            const int *__restrict__ owner,
                                                            const double *__restrict__ shift, int n3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int k = e / 3, c = e - 3 * k;
  x[3 * (size_t) nlocal + e] = x[3 * (size_t) owner[k] + c] + shift[e];
}

// f[owner[k]] += f[nlocal + k]
__global__ void __launch_bounds__(256) ghosts_reverse_kernel(double *__restrict__ f, int nlocal,
                                                            const int *__restrict__ owner, int n3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int k = e / 3, c = e - 3 * k;
  unsafeAtomicAdd(&f[3 * (size_t) owner[k] + c], f[3 * (size_t) nlocal + e]);
}

// owner_all[r] = r for the owned rows, owner[r - nlocal] behind them
__global__ void __launch_bounds__(256) ghosts_owner_all_kernel(int *__restrict__ owner_all, int nlocal, const int *__restrict__ owner,
                                                               int nall)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nall) owner_all[r] = r < nlocal ? r : owner[r - nlocal];
}

__global__ void __launch_bounds__(256) ghosts_types_kernel(int *__restrict__ type, int nlocal, const int *__restrict__ owner,
                                                          int nghost)
{
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < nghost) type[nlocal + k] = type[owner[k]];
}

// shift[k] = shift0[k] . T[cfg of owner[k]]   (one lane per coordinate; rows are vectors)
__global__ void __launch_bounds__(256) ghosts_deform_kernel(const int *__restrict__ owner, const int *__restrict__ row_cfg,
                                                           const double *__restrict__ T, const double *__restrict__ shift0,
                                                           double *__restrict__ shift, int n3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const int k = e / 3, c = e - 3 * k;
  const double *__restrict__ t = T + 9 * (size_t) row_cfg[owner[k]];
  const double *__restrict__ s = shift0 + 3 * (size_t) k;
  shift[e] = s[0] * t[c] + s[1] * t[3 + c] + s[2] * t[6 + c];
}

// fix nve, first half: v += dtf f / m; x += dt v.  second half: v += dtf f / m.  (metal units: dtf = dt/2 * ftm2v)
__global__ void __launch_bounds__(256) nve_initial_kernel(double *__restrict__ x, double *__restrict__ v,
                                                         const double *__restrict__ f, const int *__restrict__ type,
                                                         const double *__restrict__ inv_mass, double dtf, double dt, int n3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  const double vv = v[e] + dtf * inv_mass[type[e / 3] - 1] * f[e];
  v[e] = vv;
  x[e] += dt * vv;
}
__global__ void __launch_bounds__(256) nve_final_kernel(double *__restrict__ v, const double *__restrict__ f,
                                                       const int *__restrict__ type, const double *__restrict__ inv_mass,
                                                       double dtf, int n3)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n3) return;
  v[e] += dtf * inv_mass[type[e / 3] - 1] * f[e];
}

// largest squared displacement since the last re-neighbouring and the kinetic energy sum m v^2, by 64-bit atomics
// on the non-negative fp64 bit pattern (max) / fp64 add
__global__ void __launch_bounds__(256) nve_monitor_kernel(const double *__restrict__ x, const double *__restrict__ x_ref,
                                                         const double *__restrict__ v, const int *__restrict__ type,
                                                         const double *__restrict__ mass, int n, double *__restrict__ out)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  double d2 = 0.0, ke = 0.0;
  if (i < n) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double d = x[3 * (size_t) i + a] - x_ref[3 * (size_t) i + a];
      d2 += d * d;
      ke += v[3 * (size_t) i + a] * v[3 * (size_t) i + a];
    }
    ke *= mass[type[i] - 1];
  }
  typedef hipcub::BlockReduce<double, 256> Red;
  __shared__ typename Red::TempStorage tmp;
  const double bmax = Red(tmp).Reduce(d2, hipcub::Max());
  __syncthreads();
  const double bsum = Red(tmp).Sum(ke);
  if (threadIdx.x == 0) {
    atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long) __double_as_longlong(bmax));
    unsafeAtomicAdd(out + 1, bsum);
  }
}

}   // namespace

// grow-only device array of the handle.  reserve(n) makes room for n elements: what was there is released first (no build
// carries contents over), and a failed allocation leaves the buffer empty.  It reports through hipError_t, as everything
// in this file does (MD_HIP; no exceptions).
template <class T>
struct GrowBuf {
  T *p = nullptr;
  size_t cap = 0;   // elements
  GrowBuf() = default;
  GrowBuf(const GrowBuf &) = delete;
  GrowBuf &operator=(const GrowBuf &) = delete;
  ~GrowBuf() { release(); }
  void release()
  {
    if (p) (void) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  hipError_t reserve(size_t n)
  {
    if (n <= cap) return hipSuccess;
    release();
    const hipError_t e = hipMalloc((void **) &p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
};

// Buffers that grow together (d_count / d_tmp / d_first, d_owner / d_shift, d_slot / d_cfg_first) are ALL released before the
// first of them is allocated again, in the order they stand here: the last of a group has room only if every member has,
// so its capacity is the one that is asked, and a build after a failed allocation allocates the whole group again.
struct mtp_ghosts {
  int device = 0, nlocal = 0, nghost = 0;    // nghost > 0 only while d_owner / d_shift hold the maps of a finished build
  GrowBuf<int> d_count;                      // [nlocal + 1 + nlocal / 8] per-atom image counts,
  GrowBuf<char> d_tmp;                       // the workspace of a scan over that many (bytes),
  GrowBuf<int> d_first;                      // their scanned offsets
  GrowBuf<ShiftRange> d_range;               // cell builds only: [d_first.cap] ranges + one 64-bit total in the last element
  GrowBuf<int> d_owner;                      // [cap_ghost()]
  GrowBuf<double> d_shift;                   // [cap_ghost()][3]
  GrowBuf<double> d_shift0;                  // mtp_ghosts_deform only: [d_shift.cap] the shifts as the last build left them
  bool shift0_valid = false;                 // d_shift0 holds the shifts of the last build
  GrowBuf<int> d_owner_all;                  // mtp_ghosts_owner_device only: identity | d_owner
  GrowBuf<CellSlot> d_slot;                  // mtp_ghosts_build_batch only: [ncfg + ncfg / 8] cells + origins, and the
  GrowBuf<int> d_cfg_first;                  // [d_slot.cap + 1] first owned rows of the configurations
  std::vector<CellSlot> h_slot;              // host staging of d_slot
  std::string last_error;
  int cap_ghost() const { return (int) (d_shift.cap / 3); }
  unsigned long long *d_total64() const { return reinterpret_cast<unsigned long long *>(d_range.p + (d_range.cap - 1)); }
  ~mtp_ghosts() { (void) hipSetDevice(device); }   // (runs before the members free themselves)
};

#define MD_HIP(call)                                                                        \
  do {                                                                                      \
    hipError_t _e = (call);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      g->last_error = std::string(#call) + ": " + hipGetErrorString(_e);                    \
      return MTP_ERR_DEVICE;                                                                \
    }                                                                                       \
  } while (0)

static int ghosts_null_stream(mtp_ghosts *g, const char *fn)
{
  g->last_error = std::string(fn) + ": a NULL stream is not accepted (no context to take a stream from)";
  return MTP_ERR_ARG;
}

// every build starts here once its arguments are accepted, BEFORE a buffer is grown or freed: whatever fails later, the
// handle reports no ghosts rather than those of the build before over maps that are gone.  nghost becomes the new total
// only after ghosts_reserve_ghosts has succeeded.
static void ghosts_reset(mtp_ghosts *g, int nlocal)
{
  g->nlocal = nlocal;
  g->nghost = 0;
  g->shift0_valid = false;
}

// allocation growth shared by the builds: per-atom counts / offsets (+ the scan's workspace), per-ghost maps
static hipError_t ghosts_reserve_local(mtp_ghosts *g, int nlocal, hipStream_t st)
{
  if ((size_t) nlocal + 1 <= g->d_first.cap) return hipSuccess;
  hipError_t e;
  const size_t n = (size_t) nlocal + 1 + nlocal / 8;
  size_t need = 0;   // (a size query: no pointer is read)
  (void) hipcub::DeviceScan::ExclusiveSum(nullptr, need, g->d_count.p, g->d_first.p, (int) n, st);
  g->d_count.release();
  g->d_tmp.release();
  g->d_first.release();
  if ((e = g->d_count.reserve(n)) != hipSuccess) return e;
  if ((e = g->d_tmp.reserve(need)) != hipSuccess) return e;
  return g->d_first.reserve(n);
}

static hipError_t ghosts_reserve_ghosts(mtp_ghosts *g, int total)
{
  if (total <= g->cap_ghost()) return hipSuccess;
  const size_t n = std::min((size_t) total + total / 8 + 64, (size_t) 0x7fffffff);
  g->d_owner.release();
  g->d_shift.release();
  const hipError_t e = g->d_owner.reserve(n);
  return e != hipSuccess ? e : g->d_shift.reserve(3 * n);
}

// what mtp_ghosts_build_cell and mtp_ghosts_build_batch share once the entry point `fn` has checked its arguments, reset
// the handle, set the device and has its cells where the kernels read them: count, scan, ONE read-back, fill.  `hint`
// ends the refusal of a total beyond 32 bits; sum64 is the caller's own bound (an atom has at most floor(1 + 2 m_a) + 1
// shifts per direction: when that bound over all atoms fits an int -- every cell a simulation meets -- the scanned int
// total is exact and the 64-bit sum is not taken).  nlocal > 0.
template <class Cells>
static int ghosts_build_cells(mtp_ghosts *g, const char *fn, const char *hint, hipStream_t st, const Cells &cells,
                              double *d_x, int nlocal, int capacity, bool sum64, int *nall_out)
{
  MD_HIP(ghosts_reserve_local(g, nlocal, st));
  if ((size_t) nlocal + 2 > g->d_range.cap) MD_HIP(g->d_range.reserve(g->d_first.cap + 1));
  MD_HIP(hipMemsetAsync(g->d_count.p, 0, ((size_t) nlocal + 1) * sizeof(int), st));
  if (sum64) MD_HIP(hipMemsetAsync(g->d_total64(), 0, sizeof(unsigned long long), st));
  const int nb = (nlocal + 255) / 256;
  if (sum64)
    hipLaunchKernelGGL((ghosts_cell_count_kernel<Cells, true>), dim3(nb), dim3(256), 0, st, cells, d_x, nlocal, g->d_count.p,
                       g->d_range.p, g->d_total64());
  else
    hipLaunchKernelGGL((ghosts_cell_count_kernel<Cells, false>), dim3(nb), dim3(256), 0, st, cells, d_x, nlocal, g->d_count.p,
                       g->d_range.p, g->d_total64());
  size_t tb = g->d_tmp.cap;
  MD_HIP(hipcub::DeviceScan::ExclusiveSum(g->d_tmp.p, tb, g->d_count.p, g->d_first.p, nlocal + 1, st));
  int total = 0;
  unsigned long long total64 = 0;
  if (sum64) MD_HIP(hipMemcpyAsync(&total64, g->d_total64(), sizeof(total64), hipMemcpyDeviceToHost, st));
  else MD_HIP(hipMemcpyAsync(&total, g->d_first.p + nlocal, sizeof(int), hipMemcpyDeviceToHost, st));
  MD_HIP(hipStreamSynchronize(st));
  if (sum64) {
    if (total64 > 0x7fffffffull - (unsigned long long) nlocal) {   // never wrapped: the scanned offsets are not used
      *nall_out = 0x7fffffff;
      g->last_error = std::string(fn) + ": owned + ghost atoms do not fit a 32-bit count " + hint;
      return MTP_ERR_LIMIT;
    }
    total = (int) total64;   // == d_first[nlocal]: no per-atom count saturated
  }
  *nall_out = nlocal + total;
  if (nlocal + total > capacity) {   // the caller's arrays are too short: sizes are reported, nothing is written or kept
    g->last_error = std::string(fn) + ": capacity of the position array is smaller than owned + ghost atoms";
    return MTP_ERR_LIMIT;
  }
  MD_HIP(ghosts_reserve_ghosts(g, total));
  g->nghost = total;
  if (total > 0) {
    hipLaunchKernelGGL(ghosts_cell_fill_kernel<Cells>, dim3((total + 255) / 256), dim3(256), 0, st, cells, nlocal, total,
                       g->d_first.p, g->d_range.p, g->d_owner.p, g->d_shift.p, g->cap_ghost());
    hipLaunchKernelGGL(ghosts_forward_kernel, dim3((3 * total + 255) / 256), dim3(256), 0, st, d_x, nlocal, g->d_owner.p,
                       g->d_shift.p, 3 * total);
  }
  MD_HIP(hipGetLastError());
  return MTP_OK;
}

// h^-1 (cofactors over the determinant), the margins m[a] = rghost / d_a with d_a = V / |h_b x h_c| the spacing of the
// lattice planes normal to direction a; returns the determinant (<= 0 or non-finite: not a cell this library takes)
static double cell_setup(const double h[9], double rghost, double hinv[9], double m[3])
{
  for (int k = 0; k < 9; k++)
    if (!std::isfinite(h[k])) return 0.0;
  const double *a = h, *b = h + 3, *c = h + 6;
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double det = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
  if (!std::isfinite(det) || !(det > 0.0)) return 0.0;
  const double *cross[3] = {bc, ca, ab};
  for (int k = 0; k < 3; k++) {
    for (int r = 0; r < 3; r++) hinv[3 * r + k] = cross[k][r] / det;   // column k of h^-1 = (h_{k+1} x h_{k+2}) / det
    m[k] = rghost * std::sqrt(cross[k][0] * cross[k][0] + cross[k][1] * cross[k][1] + cross[k][2] * cross[k][2]) / det;
    if (!std::isfinite(m[k])) return 0.0;
  }
  return det;
}

extern "C" {

int mtp_ghosts_create(int device_id, mtp_ghosts **out)
{
  if (!out) return MTP_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return MTP_ERR_DEVICE;
  mtp_ghosts *g = new (std::nothrow) mtp_ghosts();
  if (!g) return MTP_ERR_ARG;
  g->device = device_id;
  *out = g;
  return MTP_OK;
}

void mtp_ghosts_destroy(mtp_ghosts *g) { delete g; }

const char *mtp_ghosts_last_error(const mtp_ghosts *g) { return g ? g->last_error.c_str() : "null ghosts"; }

int mtp_ghosts_build(mtp_ghosts *g, void *stream, double *d_x, int nlocal, int capacity, const double box[3],
                     double rghost, int *nall_out)
{
  if (!g || !d_x || nlocal < 0 || capacity < nlocal || !box || !(rghost > 0.0) || !nall_out) return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_build");
  for (int a = 0; a < 3; a++)
    if (!(box[a] >= rghost)) {   // one image per direction and sign: the shell must not be thicker than the box
      g->last_error = "mtp_ghosts_build: box edge shorter than the ghost cutoff";
      return MTP_ERR_LIMIT;
    }
  ghosts_reset(g, nlocal);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MD_HIP(hipSetDevice(g->device));
  MD_HIP(ghosts_reserve_local(g, nlocal, st));
  Box3 b{{box[0], box[1], box[2]}, rghost};
  const int nb = (nlocal + 255) / 256;
  MD_HIP(hipMemsetAsync(g->d_count.p, 0, ((size_t) nlocal + 1) * sizeof(int), st));
  if (nlocal > 0) hipLaunchKernelGGL(ghosts_count_kernel, dim3(nb), dim3(256), 0, st, b, d_x, nlocal, g->d_count.p);
  size_t tb = g->d_tmp.cap;
  MD_HIP(hipcub::DeviceScan::ExclusiveSum(g->d_tmp.p, tb, g->d_count.p, g->d_first.p, nlocal + 1, st));
  int total = 0;
  MD_HIP(hipMemcpyAsync(&total, g->d_first.p + nlocal, sizeof(int), hipMemcpyDeviceToHost, st));
  MD_HIP(hipStreamSynchronize(st));
  MD_HIP(ghosts_reserve_ghosts(g, total));
  g->nghost = total;
  *nall_out = nlocal + total;
  if (nlocal + total > capacity) {   // the caller's arrays are too short: sizes are reported, nothing is written
    g->last_error = "mtp_ghosts_build: capacity of the position array is smaller than owned + ghost atoms";
    return MTP_ERR_LIMIT;
  }
  if (nlocal > 0 && total > 0) {
    hipLaunchKernelGGL(ghosts_fill_kernel, dim3(nb), dim3(256), 0, st, b, d_x, nlocal, g->d_first.p, g->d_owner.p, g->d_shift.p,
                       g->cap_ghost());
    hipLaunchKernelGGL(ghosts_forward_kernel, dim3((3 * total + 255) / 256), dim3(256), 0, st, d_x, nlocal, g->d_owner.p,
                       g->d_shift.p, 3 * total);
  }
  MD_HIP(hipGetLastError());
  return MTP_OK;
}

int mtp_ghosts_cell_bounds(const double cell[9], double rghost, double lo[3], double hi[3], double *volume, int nimage[3])
{
  if (!cell || !(rghost > 0.0) || !std::isfinite(rghost)) return MTP_ERR_ARG;
  double hinv[9], m[3];
  const double det = cell_setup(cell, rghost, hinv, m);
  if (!(det > 0.0)) return MTP_ERR_ARG;
  if (volume) *volume = det;
  for (int a = 0; a < 3; a++) {
    if (nimage) nimage[a] = (int) std::fmin(std::ceil(m[a]), 2147483647.0);
    // every position written has fractional coordinates in [-m, 1 + m]^3: the box of that parallelepiped's corners,
    // widened by the rounding of s . cell + n . cell
    double l = 0.0, u = 0.0;
    for (int k = 0; k < 3; k++) {
      const double t0 = -m[k] * cell[3 * k + a], t1 = (1.0 + m[k]) * cell[3 * k + a];
      l += std::fmin(t0, t1);
      u += std::fmax(t0, t1);
    }
    const double pad = 1e-9 * (u - l) + 1e-12;
    if (lo) lo[a] = l - pad;
    if (hi) hi[a] = u + pad;
  }
  return MTP_OK;
}

int mtp_ghosts_build_cell(mtp_ghosts *g, void *stream, double *d_x, int nlocal, int capacity, const double cell[9],
                          double rghost, int *nall_out)
{
  if (!g || !d_x || nlocal < 0 || capacity < nlocal || !cell || !(rghost > 0.0) || !std::isfinite(rghost) || !nall_out)
    return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_build_cell");
  OneCell one;
  for (int k = 0; k < 9; k++) one.c.h[k] = cell[k];
  if (!(cell_setup(cell, rghost, one.c.hinv, one.c.m) > 0.0)) {
    g->last_error = "mtp_ghosts_build_cell: the cell must be finite, right-handed and non-degenerate (det > 0)";
    return MTP_ERR_ARG;
  }
  ghosts_reset(g, nlocal);
  if (nlocal == 0) {   // nothing to wrap, no images
    *nall_out = 0;
    return MTP_OK;
  }
  double bound = (double) nlocal;
  for (int a = 0; a < 3; a++) bound *= std::floor(1.0 + 2.0 * one.c.m[a]) + 1.0;
  const bool sum64 = !(bound + (double) nlocal < 2147483647.0);
  MD_HIP(hipSetDevice(g->device));
  return ghosts_build_cells(g, "mtp_ghosts_build_cell", "(cell far smaller than rghost?)", reinterpret_cast<hipStream_t>(stream), one,
                            d_x, nlocal, capacity, sum64, nall_out);
}

// ---- batched configurations ------------------------------------------------------------------------------------------

int mtp_batch_layout(int ncfg, const double *cells, double rghost, double gap, double *origins, double lo[3], double hi[3],
                     long long *ncells_out, int *nfit_out, char *err, int errlen)
{
  auto fail = [&](int code, const std::string &msg) {
    if (err && errlen > 0) std::snprintf(err, (size_t) errlen, "%s", msg.c_str());
    return code;
  };
  if (nfit_out) *nfit_out = 0;
  if (ncfg < 0 || (ncfg > 0 && (!cells || !origins)) || !lo || !hi || !(rghost > 0.0) || !std::isfinite(rghost) ||
      !std::isfinite(gap) || !(gap >= rghost))
    return fail(MTP_ERR_ARG, "mtp_batch_layout: needs cells, origins, lo, hi, rghost > 0 and gap >= rghost");
  // bounding boxes of the ghost parallelepipeds, and the largest extents of every prefix of the batch (the slots of a
  // prefix are uniform, sized by them)
  std::vector<double> blo((size_t) 3 * ncfg), pmax((size_t) 3 * ncfg);
  for (int k = 0; k < ncfg; k++) {
    double l[3], u[3];
    if (mtp_ghosts_cell_bounds(cells + 9 * (size_t) k, rghost, l, u, nullptr, nullptr) != MTP_OK)
      return fail(MTP_ERR_ARG, "mtp_batch_layout: configuration " + std::to_string(k) +
                                   ": the cell must be finite, right-handed and non-degenerate (det > 0)");
    for (int a = 0; a < 3; a++) {
      blo[3 * (size_t) k + a] = l[a];
      pmax[3 * (size_t) k + a] = std::max(u[a] - l[a], k > 0 ? pmax[3 * (size_t) (k - 1) + a] : 0.0);
    }
  }
  struct Grid {
    int g[3];
    double pitch[3], base[3], lo[3], hi[3];
    long long ncells;
    int why;   // 0 fits, 1 coordinate cap, 2 cell limit
  };
  // the first n configurations on a 3-D grid of uniform slots, grown along the axis that keeps the box smallest, centred
  // on the origin (coordinates stay small: their magnitude costs bits of the interatomic distances)
  auto place = [&](int n) {
    Grid G{};
    double S[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 3 && n > 0; a++) S[a] = pmax[3 * (size_t) (n - 1) + a];
    for (int a = 0; a < 3; a++) {
      G.g[a] = 1;
      G.pitch[a] = S[a] + gap;
    }
    while ((long long) G.g[0] * G.g[1] * G.g[2] < n) {
      int best = 0;
      for (int a = 1; a < 3; a++)
        if ((G.g[a] + 1) * G.pitch[a] < (G.g[best] + 1) * G.pitch[best]) best = a;
      G.g[best]++;
    }
    double ncells = 1.0;
    for (int a = 0; a < 3; a++) {
      const double total = (G.g[a] - 1) * G.pitch[a] + S[a];
      G.base[a] = -0.5 * total;
      G.lo[a] = G.base[a] - 1e-9;
      G.hi[a] = G.base[a] + total + 1e-9;
      if (std::fmax(std::fabs(G.lo[a]), std::fabs(G.hi[a])) > 2048.0) G.why = 1;
      // (the count mtp_build_neighbors_device derives from lo / hi)
      ncells *= std::fmax(1.0, std::ceil((G.hi[a] - G.lo[a]) / rghost));
    }
    G.ncells = ncells < 4e18 ? (long long) ncells : (1ll << 62);
    if (!G.why && G.ncells > (1ll << 26)) G.why = 2;
    return G;
  };
  Grid G = place(ncfg);
  if (G.why) {
    int fit = 0, top = ncfg - 1;   // the longest prefix that fits (the empty one does)
    while (fit < top) {
      const int mid = fit + (top - fit + 1) / 2;
      if (place(mid).why == 0) fit = mid;
      else top = mid - 1;
    }
    if (nfit_out) *nfit_out = fit;
    return fail(MTP_ERR_LIMIT, "mtp_batch_layout: configuration " + std::to_string(fit) + " is the first that does not fit: " +
                                   (G.why == 1 ? "a coordinate of the batch would exceed 2048 A in magnitude"
                                               : "the batch would need more than 2^26 list cells") +
                                   " (split the batch)");
  }
  for (int k = 0; k < ncfg; k++) {
    const int idx[3] = {k / (G.g[1] * G.g[2]), (k / G.g[2]) % G.g[1], k % G.g[2]};
    for (int a = 0; a < 3; a++) origins[3 * (size_t) k + a] = (G.base[a] + idx[a] * G.pitch[a]) - blo[3 * (size_t) k + a];
  }
  for (int a = 0; a < 3; a++) {
    lo[a] = G.lo[a];
    hi[a] = G.hi[a];
  }
  if (ncells_out) *ncells_out = G.ncells;
  if (nfit_out) *nfit_out = ncfg;
  return MTP_OK;
}

int mtp_ghosts_build_batch(mtp_ghosts *g, void *stream, double *d_x, int ncfg, const int *cfg_first, const double *cells,
                           const double *origins, int capacity, double rghost, int *nall_out)
{
  if (!g || !d_x || ncfg < 0 || !cfg_first || (ncfg > 0 && (!cells || !origins)) || !(rghost > 0.0) || !std::isfinite(rghost) ||
      !nall_out)
    return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_build_batch");
  if (cfg_first[0] != 0) {
    g->last_error = "mtp_ghosts_build_batch: cfg_first[0] must be 0";
    return MTP_ERR_ARG;
  }
  for (int k = 0; k < ncfg; k++)
    if (cfg_first[k + 1] < cfg_first[k]) {
      g->last_error = "mtp_ghosts_build_batch: cfg_first decreases at configuration " + std::to_string(k);
      return MTP_ERR_ARG;
    }
  const int nlocal = cfg_first[ncfg];
  if (capacity < nlocal) {
    g->last_error = "mtp_ghosts_build_batch: capacity is smaller than the owned atoms";
    return MTP_ERR_ARG;
  }
  // (the bound of ghosts_build_cells, summed over the batch)
  g->h_slot.resize((size_t) ncfg);
  double bound = (double) nlocal;
  for (int k = 0; k < ncfg; k++) {
    CellSlot &s = g->h_slot[(size_t) k];
    for (int q = 0; q < 9; q++) s.c.h[q] = cells[9 * (size_t) k + q];
    if (!(cell_setup(s.c.h, rghost, s.c.hinv, s.c.m) > 0.0)) {
      g->last_error = "mtp_ghosts_build_batch: configuration " + std::to_string(k) +
          ": the cell must be finite, right-handed and non-degenerate (det > 0)";
      return MTP_ERR_ARG;
    }
    double per_atom = 1.0;
    for (int a = 0; a < 3; a++) {
      s.org[a] = origins[3 * (size_t) k + a];
      if (!std::isfinite(s.org[a])) {
        g->last_error = "mtp_ghosts_build_batch: configuration " + std::to_string(k) + ": non-finite origin";
        return MTP_ERR_ARG;
      }
      per_atom *= std::floor(1.0 + 2.0 * s.c.m[a]) + 1.0;
    }
    bound += per_atom * (double) (cfg_first[k + 1] - cfg_first[k]);
  }
  ghosts_reset(g, nlocal);
  *nall_out = nlocal;
  if (nlocal == 0) return MTP_OK;   // nothing to wrap, no images
  const bool sum64 = !(bound < 2147483647.0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MD_HIP(hipSetDevice(g->device));
  if ((size_t) ncfg + 1 > g->d_cfg_first.cap) {
    const size_t n = (size_t) ncfg + ncfg / 8;
    g->d_slot.release();
    g->d_cfg_first.release();
    MD_HIP(g->d_slot.reserve(n));
    MD_HIP(g->d_cfg_first.reserve(n + 1));
  }
  // (ghosts_build_cells synchronises the stream before this call returns: the host arrays outlive both copies)
  MD_HIP(hipMemcpyAsync(g->d_slot.p, g->h_slot.data(), (size_t) ncfg * sizeof(CellSlot), hipMemcpyHostToDevice, st));
  MD_HIP(hipMemcpyAsync(g->d_cfg_first.p, cfg_first, ((size_t) ncfg + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  return ghosts_build_cells(g, "mtp_ghosts_build_batch", "(split the batch)", st, SlotCells{g->d_slot.p, g->d_cfg_first.p, ncfg}, d_x,
                            nlocal, capacity, sum64, nall_out);
}

int mtp_ghosts_forward(mtp_ghosts *g, void *stream, double *d_x)
{
  if (!g || !d_x) return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_forward");
  if (g->nghost > 0)
    hipLaunchKernelGGL(ghosts_forward_kernel, dim3((3 * g->nghost + 255) / 256), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), d_x, g->nlocal, g->d_owner.p, g->d_shift.p, 3 * g->nghost);
  MD_HIP(hipGetLastError());
  return MTP_OK;
}

int mtp_ghosts_reverse(mtp_ghosts *g, void *stream, double *d_f)
{
  if (!g || !d_f) return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_reverse");
  if (g->nghost > 0)
    hipLaunchKernelGGL(ghosts_reverse_kernel, dim3((3 * g->nghost + 255) / 256), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), d_f, g->nlocal, g->d_owner.p, 3 * g->nghost);
  MD_HIP(hipGetLastError());
  return MTP_OK;
}

int mtp_ghosts_reverse_finish(mtp_ghosts *g, mtp_context *ctx, void *stream, int eflag, int vflag, double *d_f, double *d_ev)
{
  if (!g || !ctx || !d_f) return MTP_ERR_ARG;
  // the tally fold of a force call made with finish_tallies = 0 rides in the launch that folds the ghost forces
  // (a context is at hand: NULL -> the context's stream, as in mtp_compute_device)
  return mtp_internal_finish_unpack(ctx, stream, eflag, vflag, d_ev, d_f, g->d_owner.p, d_f + 3 * (size_t) g->nlocal, 3 * g->nghost);
}

int mtp_ghosts_types(mtp_ghosts *g, void *stream, int *d_type)
{
  if (!g || !d_type) return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_types");
  if (g->nghost > 0)
    hipLaunchKernelGGL(ghosts_types_kernel, dim3((g->nghost + 255) / 256), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), d_type, g->nlocal, g->d_owner.p, g->nghost);
  MD_HIP(hipGetLastError());
  return MTP_OK;
}

int mtp_ghosts_deform(mtp_ghosts *g, void *stream, const int *d_row_cfg, const double *d_T)
{
  if (!g || !d_row_cfg || !d_T) return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_deform");
  if (g->nghost == 0) return MTP_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  MD_HIP(hipSetDevice(g->device));
  if (!g->shift0_valid) {   // the first call after a build keeps that build's shifts
    if (3 * (size_t) g->nghost > g->d_shift0.cap) MD_HIP(g->d_shift0.reserve(g->d_shift.cap));
    MD_HIP(hipMemcpyAsync(g->d_shift0.p, g->d_shift.p, 3 * (size_t) g->nghost * sizeof(double), hipMemcpyDeviceToDevice, st));
    g->shift0_valid = true;
  }
  hipLaunchKernelGGL(ghosts_deform_kernel, dim3((3 * g->nghost + 255) / 256), dim3(256), 0, st, g->d_owner.p, d_row_cfg, d_T,
                     g->d_shift0.p, g->d_shift.p, 3 * g->nghost);
  MD_HIP(hipGetLastError());
  return MTP_OK;
}

int mtp_ghosts_owner_device(mtp_ghosts *g, void *stream, const int **d_owner, int *nall)
{
  if (!g || !d_owner || !nall) return MTP_ERR_ARG;
  if (!stream) return ghosts_null_stream(g, "mtp_ghosts_owner_device");
  const int n = g->nlocal + g->nghost;
  MD_HIP(hipSetDevice(g->device));
  if ((size_t) n > g->d_owner_all.cap || !g->d_owner_all.p) MD_HIP(g->d_owner_all.reserve((size_t) n + n / 8 + 64));
  if (n > 0)
    hipLaunchKernelGGL(ghosts_owner_all_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       g->d_owner_all.p, g->nlocal, g->d_owner.p, n);
  MD_HIP(hipGetLastError());
  *d_owner = g->d_owner_all.p;
  *nall = n;
  return MTP_OK;
}

int mtp_nve_initial(void *stream, int nlocal, double *d_x, double *d_v, const double *d_f, const int *d_type,
                    const double *d_inv_mass, double dtf, double dt)
{
  if (!stream || nlocal < 0 || (nlocal > 0 && (!d_x || !d_v || !d_f || !d_type || !d_inv_mass))) return MTP_ERR_ARG;
  if (nlocal > 0)
    hipLaunchKernelGGL(nve_initial_kernel, dim3((3 * nlocal + 255) / 256), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), d_x, d_v, d_f, d_type, d_inv_mass, dtf, dt, 3 * nlocal);
  return hipGetLastError() == hipSuccess ? MTP_OK : MTP_ERR_DEVICE;
}

int mtp_nve_final(void *stream, int nlocal, double *d_v, const double *d_f, const int *d_type,
                  const double *d_inv_mass, double dtf)
{
  if (!stream || nlocal < 0 || (nlocal > 0 && (!d_v || !d_f || !d_type || !d_inv_mass))) return MTP_ERR_ARG;
  if (nlocal > 0)
    hipLaunchKernelGGL(nve_final_kernel, dim3((3 * nlocal + 255) / 256), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), d_v, d_f, d_type, d_inv_mass, dtf, 3 * nlocal);
  return hipGetLastError() == hipSuccess ? MTP_OK : MTP_ERR_DEVICE;
}

int mtp_nve_monitor(void *stream, int nlocal, const double *d_x, const double *d_x_ref, const double *d_v,
                    const int *d_type, const double *d_mass, double *d_out2)
{
  if (!stream || nlocal < 0 || !d_out2 || (nlocal > 0 && (!d_x || !d_x_ref || !d_v || !d_type || !d_mass))) return MTP_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(d_out2, 0, 2 * sizeof(double), st) != hipSuccess) return MTP_ERR_DEVICE;
  if (nlocal > 0)
    hipLaunchKernelGGL(nve_monitor_kernel, dim3((nlocal + 255) / 256), dim3(256), 0, st, d_x, d_x_ref, d_v, d_type, d_mass,
                       nlocal, d_out2);
  return hipGetLastError() == hipSuccess ? MTP_OK : MTP_ERR_DEVICE;
}

}   // extern "C"
