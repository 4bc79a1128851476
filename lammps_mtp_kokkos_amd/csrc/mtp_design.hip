// Design rows of the linear refit (include/mtp_mi355x.h, "linear refit"): forward-mode tangents of the
// basis functions with respect to every neighbour coordinate.
//
//   m_k(n)   = f_mu(r_n; t_i, t_n) / r_n^nu  x^a y^b z^c           basic k = (mu; a, b, c), nu = a + b + c
//   M_k      = sum_n m_k(n),   M[a3] += mult M[a0] M[a1]            the times rows, level by level
//   direction d = (n, c):  dM_k = d m_k(n) / d u_{n,c}              (pair_mtp.cpp:163-191)
//                          dM[a3] += mult (dM[a0] M[a1] + M[a0] dM[a1])
//   G_a(i, n, c) = dM[map[a]]
//
// One workgroup of MTP_DESIGN_WAVES wavefronts per centre atom.  Compaction, tile tables, the basics and the product
// levels of M run once per workgroup (lanes = basics, then lanes = rows of a level, ds_add_f64 into the shared image); the
// 3 K directions are then dealt to the wavefronts, each with a private dM image in LDS (lanes = basics, rows, scalars in
// turn).  Per direction S fp64 atomic adds go to the owner row of the neighbour; the centre's own force rows and its six
// virial rows are summed in LDS over all directions and leave once per centre.  The times rows themselves (8 bytes each)
// are read from HBM / L2, lane-contiguous: at level 20 they are 51 KB, which would halve the directions in flight.
#include <hip/hip_runtime.h>

#include "mtp_centre_common.hpp"

namespace {

constexpr int NT = MTP_DESIGN_NT;
constexpr int NW = MTP_DESIGN_WAVES;
constexpr int NTHREADS = 64 * NW;
constexpr int PITCH = MTP_PITCH;

struct DesignInts {   // the integer tail of the image
  int *pack, *fmap, *map, *level, *nbown, *cj, *cnt;
};

// tile tables (mtp_centre_common.hpp; no rows of the kernel's own: the powers start at row 2 Mu); nb: u [3] | 1/r
__device__ __forceinline__ void build_tile(const MtpDesignParams &p, double *tab, double *nb, const DesignInts &it, int t0, int nt,
                                           int itype, double xi0, double xi1, double xi2, int tid)
{
  const int n = tid & (NT - 1), part = tid / NT;
  static_assert(NTHREADS / NT == 8, "eight threads per neighbour column");
  if (n < nt) {
    const int j = it.cj[t0 + n];
    const CentreGeom g = tile_geom(p, j, xi0, xi1, xi2);
    if (part == 0) {
      tile_nb<NT>(nb, n, g.dx, g.dy, g.dz, g.inv);
      it.nbown[n] = p.owner ? p.owner[j] : j;
    }
    tile_powers(tab + n, 2 * p.Mu, p.P, part, g.dx, g.dy, g.dz, g.inv);
    const int jt = p.type[j] - 1;   // (inside the potential: the compaction dropped the others)
    tile_radial<false>(p, p.radial, itype * p.Sp + jt, g.r, tab + n, part);
  }
}

__global__ void __launch_bounds__(NTHREADS) mtp_design_kernel(const MtpDesignParams p)
{
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Sp = p.Sp, Mu = p.Mu, P = p.P, A = p.A, B = p.B, S = p.S;
  double *M = lds;
  double *dM = lds + p.off_dm + wave * p.a_pad;
  double *acc = lds + p.off_acc;   // [9][S]: own force rows x, y, z, then the virial rows xx, yy, zz, xy, xz, yz
  double *tab = lds + p.off_tab;
  double *nb = lds + p.off_nb;
  DesignInts it;
  it.pack = reinterpret_cast<int *>(lds + p.off_int);
  it.fmap = it.pack + B;
  it.map = it.fmap + S;
  it.level = it.map + S;
  it.nbown = it.level + p.nblocks + 1;
  it.cj = it.nbown + NT;
  it.cnt = it.cj + p.cj_cap;

  for (int k = tid; k < B; k += NTHREADS) it.pack[k] = p.pack[k];
  for (int k = tid; k < S; k += NTHREADS) {
    it.fmap[k] = p.fmap[k];
    it.map[k] = p.map[k];
  }
  for (int k = tid; k <= p.nblocks; k += NTHREADS) it.level[k] = p.level[k];
  __syncthreads();

  for (int ii = p.row0 + blockIdx.x; ii < p.row0 + p.nrows; ii += gridDim.x) {
    const int i = p.ilist[ii];
    const int itype = p.type[i] - 1;
    if (!centre_ok(p, i, itype, tid)) continue;
    const double xi0 = p.x[3 * (size_t) i], xi1 = p.x[3 * (size_t) i + 1], xi2 = p.x[3 * (size_t) i + 2];
    const int jbeg = p.first[ii], jnum = p.first[ii + 1] - jbeg;

    // ---- compaction (wavefront 0, in list order), M and the accumulators zeroed by all
    if (wave == 0) compact_neighbours(p, jbeg, jnum, xi0, xi1, xi2, lane, it.cj, it.cnt);
    for (int k = tid; k < A; k += NTHREADS) M[k] = 0.0;
    for (int k = tid; k < 9 * S; k += NTHREADS) acc[k] = 0.0;
    __syncthreads();
    const int cnt = it.cnt[0];
    const int ntiles = (cnt + NT - 1) / NT;

    // ---- basics: M_k = sum_n m_k(n), tile after tile (thread k owns M[k])
    for (int tile = 0; tile < ntiles; tile++) {
      const int t0 = tile * NT, nt = min(NT, cnt - t0);
      if (tile > 0) __syncthreads();
      build_tile(p, tab, nb, it, t0, nt, itype, xi0, xi1, xi2, tid);
      __syncthreads();
      for (int k = tid; k < B; k += NTHREADS) {
        const CentreBasic bk = decode_basic(it.pack[k]);
        const double *rv = tab + bk.mu * PITCH, *ri = tab + (2 * Mu + bk.a + bk.b + bk.c) * PITCH;
        const double *xa = tab + (2 * Mu + P + bk.a) * PITCH, *yb = tab + (2 * Mu + 2 * P + bk.b) * PITCH,
                     *zc = tab + (2 * Mu + 3 * P + bk.c) * PITCH;
        double s = 0.0;
        for (int n = 0; n < nt; n++) s += (rv[n] * ri[n]) * (xa[n] * (yb[n] * zc[n]));
        M[k] += s;
      }
    }
    __syncthreads();
    // ---- products of M
    product_pass<true, false, NTHREADS>(p.rows, it.level, p.nblocks, M, nullptr, tid);
    // ---- site-energy design row
    if (p.basis) {
      double *row = p.basis + (size_t) (ii - p.row0) * p.ld;
      for (int c = tid; c < p.ld; c += NTHREADS) row[c] = c < Sp ? (c == itype ? 1.0 : 0.0) : c < Sp + S ? M[it.map[c - Sp]] : 0.0;
    }

    // ---- directions, tile after tile
    for (int tile = 0; tile < ntiles; tile++) {
      const int t0 = tile * NT, nt = min(NT, cnt - t0);
      if (ntiles > 1) {   // (a single tile still holds its tables)
        __syncthreads();
        build_tile(p, tab, nb, it, t0, nt, itype, xi0, xi1, xi2, tid);
        __syncthreads();
      }
      for (int d = wave; d < 3 * nt; d += NW) {
        const int n = d / 3, c = d - 3 * n;
        const double u0 = nb[n], u1 = nb[NT + n], u2 = nb[2 * NT + n], inv = nb[3 * NT + n];
        const double uc = c == 0 ? u0 : c == 1 ? u1 : u2;
        const double *col = tab + n;
        // tangents of the basics; every other moment starts at zero
        for (int k = lane; k < A; k += 64) {
          double v = 0.0;
          if (k < B) {
            const CentreBasic bk = decode_basic(it.pack[k]);
            const CentreTangent t = basic_tangent(col, Mu, 2 * Mu, P, bk, inv);
            v = (t.pa * t.pb * t.pc) * (t.der * inv) * uc;
            const int e = c == 0 ? bk.a : c == 1 ? bk.b : bk.c;
            if (e > 0) {   // chain rule for the monomial
              const double others = c == 0 ? t.pb * t.pc : c == 1 ? t.pa * t.pc : t.pa * t.pb;
              v += t.val * (double) e * tangent_low(col, 2 * Mu, P, c, e) * others;
            }
          }
          dM[k] = v;
        }
        wave_fence();
        product_pass<false, true, 64>(p.rows, it.level, p.nblocks, M, dM, lane);
        // scatter: lanes = scalars.  An image of the centre itself takes the two force terms to the same row: they cancel
        const int own = it.nbown[n];
        const bool own_ok = (unsigned) own < (unsigned) p.nowned;
        if (!own_ok && lane == 0) atomicExch(p.err_flag, 3);
        const bool forces = own_ok && own != i;
        double *frow = p.force + ((size_t) 3 * (own_ok ? own : 0) + c) * p.ld + Sp;
        // virial rows this direction feeds (pair_mtp.cpp:260-266): the diagonal one and two halves off it
        const int o1 = c == 0 ? 6 : c == 1 ? 6 : 7, o2 = c == 0 ? 7 : c == 1 ? 8 : 8;
        const double w1 = c == 0 ? u1 : u0, w2 = c == 2 ? u1 : u2;
        for (int al = lane; al < S; al += 64) {
          const int m = it.fmap[al];
          const double g = m >= 0 ? dM[m] : 0.0;
          if (forces) {
            unsafeAtomicAdd(frow + al, -g);
            lds_add(&acc[c * S + al], g);
          }
          if (p.virial) {
            lds_add(&acc[(3 + c) * S + al], -g * uc);
            lds_add(&acc[o1 * S + al], -0.5 * g * w1);
            lds_add(&acc[o2 * S + al], -0.5 * g * w2);
          }
        }
        wave_fence();
      }
    }
    __syncthreads();
    // ---- the centre's own force rows (other centres add to them as well) and its virial rows (written once)
    if (cnt > 0) {
      double *frow = p.force + (size_t) 3 * i * p.ld + Sp;
      for (int e = tid; e < 3 * S; e += NTHREADS) {
        const int c = e / S;
        unsafeAtomicAdd(frow + (size_t) c * p.ld + (e - c * S), acc[e]);
      }
    }
    if (p.virial) {
      double *vrow = p.virial + (size_t) (ii - p.row0) * 6 * p.ld;
      for (int e = tid; e < 6 * p.ld; e += NTHREADS) {
        const int ab = e / p.ld, c = e - ab * p.ld;
        vrow[e] = c >= Sp && c < Sp + S ? acc[(3 + ab) * S + c - Sp] : 0.0;
      }
    }
    __syncthreads();
  }
}

// energy[k][c] = sum of basis rows, virial[k][ab][c] = sum of virial_atom rows of configuration k: blockIdx.y = 0 the
// energy row, 1..6 the virial rows; columns over the threads, rows in order
__global__ void __launch_bounds__(256) mtp_batch_design_reduce_kernel(int ld, const int *__restrict__ cfg_first,
                                                                        const double *__restrict__ basis,
                                                                        const double *__restrict__ virial_atom,
                                                                        double *__restrict__ energy, double *__restrict__ virial)
{
  const int k = blockIdx.x, q = blockIdx.y;
  const int b = cfg_first[k], e = cfg_first[k + 1];
  if (q == 0 ? energy == nullptr : virial == nullptr) return;
  for (int c = threadIdx.x; c < ld; c += blockDim.x) {
    double s = 0.0;
    if (q == 0)
      for (int r = b; r < e; r++) s += basis[(size_t) r * ld + c];
    else
      for (int r = b; r < e; r++) s += virial_atom[((size_t) r * 6 + (q - 1)) * ld + c];
    if (q == 0) energy[(size_t) k * ld + c] = s;
    else virial[((size_t) k * 6 + (q - 1)) * ld + c] = s;
  }
}

}   // namespace

size_t mtp_design_lds_layout(MtpDesignParams &p)
{
  p.a_pad = (p.A + 1) & ~1;
  p.tab_rows = 2 * p.Mu + 4 * p.P;
  p.off_dm = p.a_pad;
  p.off_acc = p.off_dm + MTP_DESIGN_WAVES * p.a_pad;
  p.off_tab = p.off_acc + 9 * p.S;
  p.off_nb = p.off_tab + p.tab_rows * MTP_PITCH;
  p.off_int = p.off_nb + 4 * MTP_DESIGN_NT;
  const size_t ints = (size_t) p.B + 2 * (size_t) p.S + p.nblocks + 1 + MTP_DESIGN_NT + (size_t) p.cj_cap + 2;
  return ((size_t) p.off_int + (ints + 1) / 2) * sizeof(double);
}

hipError_t mtp_launch_design_kernel(const MtpDesignParams &p, int grid, size_t lds, hipStream_t st)
{
  static std::atomic<unsigned long long> attr_mask{0};
  const hipError_t e = mtp_raise_lds_limit(reinterpret_cast<const void *>(&mtp_design_kernel), attr_mask);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mtp_design_kernel, dim3(grid), dim3(NTHREADS), lds, st, p);
  return hipGetLastError();
}

hipError_t mtp_launch_batch_design_reduce(int ncfg, const int *cfg_first, int ld, const double *basis, const double *virial_atom,
                                          double *energy, double *virial, hipStream_t st)
{
  hipLaunchKernelGGL(mtp_batch_design_reduce_kernel, dim3(ncfg, 7), dim3(256), 0, st, ld, cfg_first, basis, virial_atom, energy,
                     virial);
  return hipGetLastError();
}
