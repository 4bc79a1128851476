// Training gradient (include/mtp_mi355x.h, "training gradient"): value and vector-Jacobian product of
// {eatom, folded force, vatom} with respect to ALL coefficients theta = [radial | species | moments], which arrive as one
// device vector and not from the context's force tables.
//
//   value:  M (basics, times rows level by level), D seeded with the moment coefficients and swept in reverse,
//           t_n = sum_k D_k dM_k / du_n;   eatom, +t on the centre's row and -t on owner(n), vatom (pair_mtp.cpp:196-276)
//   vjp:    ONE tangent direction per centre, du_n = fbar_i - fbar_owner(n) - Vs u_n, dr_n = u_n . du_n / r_n:
//           dM through the basics and the times rows, dD through the reverse sweep (dD starts at 0: the seeds are constants)
//           row = [ Q_rho a_mu(n) + Q'_rho b_mu(n)  summed over n by neighbour type | ebar at t_i | ebar M[map] + dM[map] ]
//           a_mu(n) = sum_{k: mu_k = mu} (ebar D_k + dD_k) w_k(n) + D_k dw_k(n),   b_mu(n) = dr_n sum_k D_k w_k(n)
//
// One workgroup of MTP_TRAIN_WAVES wavefronts per centre atom, as the design kernel (mtp_design.hip): its compaction, its
// tile tables (Q_rho and Q'_rho kept per neighbour in addition) and its level-by-level product passes.  Every sum over
// neighbours has one owner thread and runs in tile order; LDS atomics are used in the product passes only, where rows of
// one level share a target.  The gradient row is assigned by its workgroup: no atomics to global memory in vjp mode.
#include <hip/hip_runtime.h>

#include "mtp_centre_common.hpp"

namespace {

constexpr int NT = MTP_TRAIN_NT;
constexpr int NW = MTP_TRAIN_WAVES;
constexpr int NTHREADS = 64 * NW;
constexpr int PITCH = MTP_PITCH;
constexpr int NPART = NTHREADS / NT;
static_assert(NPART == 8, "eight threads per neighbour column");

struct TrainInts {   // the integer tail of the image
  int *pack, *map, *level, *bymu, *mufirst, *nbown, *nbtype, *cj, *cnt;
};

// tile tables: val_mu | der_mu [Mu each] | Q_rho | Q'_rho [R each] | r^-nu [P] | x^e, y^e, z^e [P each], one column per
// neighbour; nb: u [3] | 1/r | du [3] | dr.  Eight threads share a neighbour.
template <bool VJP>
__device__ __forceinline__ void build_tile(const MtpTrainParams &p, double *tab, double *nb, const TrainInts &it, int t0, int nt,
                                           int i, int itype, int row, double xi0, double xi1, double xi2, int tid)
{
  const int n = tid & (NT - 1), part = tid / NT;
  if (n < nt) {
    const int j = it.cj[t0 + n];
    const CentreGeom g = tile_geom(p, j, xi0, xi1, xi2);
    const double dx = g.dx, dy = g.dy, dz = g.dz, inv = g.inv;
    const int jt = p.type[j] - 1;   // (inside the potential: the compaction dropped the others)
    if (part == 0) {
      tile_nb<NT>(nb, n, dx, dy, dz, inv);
      it.nbtype[n] = jt;
    }
    tile_powers(tab + n, 2 * p.Mu + 2 * p.R, p.P, part, dx, dy, dz, inv);
    if (part == 4) {
      int own = p.owner ? p.owner[j] : j;
      if ((unsigned) own >= (unsigned) p.nowned) {
        atomicExch(p.err_flag, 3);
        own = -1;   // (no force row and no fbar for it)
      }
      it.nbown[n] = own;
      if (VJP) {
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        if (p.fbar && own >= 0) {
          d0 = p.fbar[3 * (size_t) i] - p.fbar[3 * (size_t) own];
          d1 = p.fbar[3 * (size_t) i + 1] - p.fbar[3 * (size_t) own + 1];
          d2 = p.fbar[3 * (size_t) i + 2] - p.fbar[3 * (size_t) own + 2];
        }
        if (p.vbar) {
          const double *v = p.vbar + 6 * (size_t) row;
          d0 -= v[0] * dx + 0.5 * (v[3] * dy + v[4] * dz);
          d1 -= v[1] * dy + 0.5 * (v[3] * dx + v[5] * dz);
          d2 -= v[2] * dz + 0.5 * (v[4] * dx + v[5] * dy);
        }
        nb[4 * NT + n] = d0;
        nb[5 * NT + n] = d1;
        nb[6 * NT + n] = d2;
        nb[7 * NT + n] = (dx * d0 + dy * d1 + dz * d2) * inv;
      }
    }
    tile_radial<true>(p, p.theta, itype * p.Sp + jt, g.r, tab + n, part);   // (Q_rho and Q'_rho kept)
  }
}

template <bool VJP> __global__ void __launch_bounds__(NTHREADS) mtp_train_kernel(const MtpTrainParams p)
{
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Sp = p.Sp, Mu = p.Mu, P = p.P, R = p.R, B = p.B, S = p.S;
  const int pw0 = 2 * Mu + 2 * R;
  const int nrad = Sp * Sp * Mu * R, blk = Sp * Mu * R;
  double *M = lds, *dM = lds + p.a_pad, *D = lds + 2 * p.a_pad, *dD = lds + 3 * p.a_pad;
  double *tab = lds + p.off_tab;
  double *nb = lds + p.off_nb;
  double *scr = lds + p.off_scr;   // vjp: a_mu(n) | b_mu(n) [Mu][NT] each; value: partial t [NPART][3][NT], then t [3][NT]
  double *rad = lds + p.off_rad;   // [Sp][Mu][R]: the centre's block of radial columns
  TrainInts it;
  it.pack = reinterpret_cast<int *>(lds + p.off_int);
  it.map = it.pack + B;
  it.level = it.map + S;
  it.bymu = it.level + p.nblocks + 1;
  it.mufirst = it.bymu + B;
  it.nbown = it.mufirst + Mu + 1;
  it.nbtype = it.nbown + NT;
  it.cj = it.nbtype + NT;
  it.cnt = it.cj + p.cj_cap;
  const double *xi = p.theta + nrad + Sp;

  for (int k = tid; k < B; k += NTHREADS) {
    it.pack[k] = p.pack[k];
    it.bymu[k] = p.bymu[k];
  }
  for (int k = tid; k < S; k += NTHREADS) it.map[k] = p.map[k];
  for (int k = tid; k <= p.nblocks; k += NTHREADS) it.level[k] = p.level[k];
  for (int k = tid; k <= Mu; k += NTHREADS) it.mufirst[k] = p.mufirst[k];
  __syncthreads();

  for (int ii = p.row0 + blockIdx.x; ii < p.row0 + p.nrows; ii += gridDim.x) {
    const int i = p.ilist[ii];
    const int row = ii - p.row0;
    const int itype = p.type[i] - 1;
    if (!centre_ok(p, i, itype, tid)) continue;
    const double xi0 = p.x[3 * (size_t) i], xi1 = p.x[3 * (size_t) i + 1], xi2 = p.x[3 * (size_t) i + 2];
    const int jbeg = p.first[ii], jnum = p.first[ii + 1] - jbeg;
    const double eb = VJP && p.ebar ? p.ebar[row] : 0.0;

    // ---- compaction (wavefront 0, in list order); the images zeroed by all
    if (wave == 0) compact_neighbours(p, jbeg, jnum, xi0, xi1, xi2, lane, it.cj, it.cnt);
    for (int k = tid; k < 4 * p.a_pad; k += NTHREADS) M[k] = 0.0;   // M | dM | D | dD
    for (int k = tid; k < blk; k += NTHREADS) rad[k] = 0.0;
    __syncthreads();
    const int cnt = it.cnt[0];
    const int ntiles = (cnt + NT - 1) / NT;

    // ---- basics: M_k = sum_n f_mu w_k, dM_k = sum_n f'_mu dr w_k + f_mu dw_k, tile after tile (thread k owns slot k)
    for (int tile = 0; tile < ntiles; tile++) {
      const int t0 = tile * NT, nt = min(NT, cnt - t0);
      if (tile > 0) __syncthreads();
      build_tile<VJP>(p, tab, nb, it, t0, nt, i, itype, row, xi0, xi1, xi2, tid);
      __syncthreads();
      for (int k = tid; k < B; k += NTHREADS) {
        const CentreBasic bk = decode_basic(it.pack[k]);
        const int a = bk.a, b = bk.b, c = bk.c, mu = bk.mu, nu = bk.nu;
        const double *rv = tab + mu * PITCH, *rd = tab + (Mu + mu) * PITCH, *ri = tab + (pw0 + nu) * PITCH;
        const double *xa = tab + (pw0 + P + a) * PITCH, *yb = tab + (pw0 + 2 * P + b) * PITCH, *zc = tab + (pw0 + 3 * P + c) * PITCH;
        double s = 0.0, ds = 0.0;
        for (int n = 0; n < nt; n++) {
          const double pa = xa[n], pb = yb[n], pc = zc[n];
          const double w = ri[n] * (pa * (pb * pc));
          s += rv[n] * w;
          if (VJP) {
            double gm = 0.0;   // grad(x^a y^b z^c) . du
            if (a > 0) gm += (double) a * xa[n - PITCH] * pb * pc * nb[4 * NT + n];
            if (b > 0) gm += (double) b * pa * yb[n - PITCH] * pc * nb[5 * NT + n];
            if (c > 0) gm += (double) c * pa * pb * zc[n - PITCH] * nb[6 * NT + n];
            const double dr = nb[7 * NT + n];
            const double dw = ri[n] * gm - (double) nu * w * nb[3 * NT + n] * dr;
            ds += rd[n] * dr * w + rv[n] * dw;
          }
        }
        M[k] += s;
        if (VJP) dM[k] += ds;
      }
    }
    __syncthreads();
    // ---- products of M (and of dM)
    product_pass<true, VJP, NTHREADS>(p.rows, it.level, p.nblocks, M, dM, tid);
    // ---- adjoint: seeded by assignment with the moment coefficients (one scalar per moment: the table was checked), swept
    // through the levels in reverse; a row's target is complete before its level is reached
    for (int s = tid; s < S; s += NTHREADS) D[it.map[s]] = xi[s];
    __syncthreads();
    for (int l = p.nblocks - 1; l >= 0; l--) {
      for (int r = it.level[l] + tid; r < it.level[l + 1]; r += NTHREADS) {
        const CentreRow w = decode_row(p.rows[r]);
        const int a0 = w.a0(), a1 = w.a1(), a3 = w.a3();
        const double m = w.mult(), d3 = m * D[a3], m0 = M[a0], m1 = M[a1];
        if (VJP) {
          const double dd3 = m * dD[a3];
          lds_add(&dD[a1], dd3 * m0 + d3 * dM[a0]);
          lds_add(&dD[a0], dd3 * m1 + d3 * dM[a1]);
        }
        lds_add(&D[a1], d3 * m0);
        lds_add(&D[a0], d3 * m1);
      }
      __syncthreads();
    }

    if (!VJP) {
      // ---- site energy (wavefront 0)
      if (wave == 0) {
        double e = 0.0;
        for (int s = lane; s < S; s += 64) e += xi[s] * M[it.map[s]];
        e = wave_sum(e);
        if (lane == 0 && p.eatom) p.eatom[row] = p.theta[nrad + itype] + e;
      }
      // ---- forces, tile after tile: thread (n, part) sums its share of the basics, thread (c, n) the eight parts; threads
      // 0..8 own the centre's force and its six virial components over all neighbours, in list order
      double own9 = 0.0;
      for (int tile = 0; tile < ntiles; tile++) {
        const int t0 = tile * NT, nt = min(NT, cnt - t0);
        if (ntiles > 1) {   // (a single tile still holds its tables)
          __syncthreads();
          build_tile<VJP>(p, tab, nb, it, t0, nt, i, itype, row, xi0, xi1, xi2, tid);
          __syncthreads();
        }
        {
          const int n = tid & (NT - 1), part = tid / NT;
          double t0x = 0.0, t1x = 0.0, t2x = 0.0;
          if (n < nt) {
            const double u0 = nb[n], u1 = nb[NT + n], u2 = nb[2 * NT + n], inv = nb[3 * NT + n];
            const double *col = tab + n;
            for (int k = part; k < B; k += NPART) {
              const CentreBasic bk = decode_basic(it.pack[k]);
              const int a = bk.a, b = bk.b, c = bk.c;
              const CentreTangent t = basic_tangent(col, Mu, pw0, P, bk, inv);
              const double pa = t.pa, pb = t.pb, pc = t.pc;
              const double dk = D[k];
              const double rad_part = dk * (pa * pb * pc) * (t.der * inv);
              double g0 = rad_part * u0, g1 = rad_part * u1, g2 = rad_part * u2;
              const double dv = dk * t.val;
              if (a > 0) g0 += dv * (double) a * tangent_low(col, pw0, P, 0, a) * pb * pc;
              if (b > 0) g1 += dv * (double) b * pa * tangent_low(col, pw0, P, 1, b) * pc;
              if (c > 0) g2 += dv * (double) c * pa * pb * tangent_low(col, pw0, P, 2, c);
              t0x += g0;
              t1x += g1;
              t2x += g2;
            }
          }
          scr[(part * 3 + 0) * NT + n] = t0x;
          scr[(part * 3 + 1) * NT + n] = t1x;
          scr[(part * 3 + 2) * NT + n] = t2x;
        }
        __syncthreads();
        double t = 0.0;
        if (tid < 3 * NT) {
          const int c = tid / NT, n = tid - c * NT;
          for (int q = 0; q < NPART; q++) t += scr[(q * 3 + c) * NT + n];
          const int own = n < nt ? it.nbown[n] : -1;
          if (own >= 0) unsafeAtomicAdd(p.force + 3 * (size_t) own + c, -t);   // pair_mtp.cpp:252-254: f[j] -= t
        }
        __syncthreads();
        if (tid < 3 * NT) scr[tid] = t;   // t [3][NT] over the first rows of the scratch
        __syncthreads();
        if (tid < 9) {
          // pair_mtp.cpp:257-276: f[i] += t; vatom[i] -= t (x) u, the off-diagonal ones symmetrised
          const int c1 = tid < 3 ? tid : tid < 6 ? tid - 3 : tid == 6 ? 0 : tid == 7 ? 0 : 1;
          const int c2 = tid < 6 ? c1 : tid == 6 ? 1 : 2;
          for (int n = 0; n < nt; n++) {
            if (tid < 3) own9 += scr[c1 * NT + n];
            else if (tid < 6) own9 -= scr[c1 * NT + n] * nb[c1 * NT + n];
            else own9 -= 0.5 * (scr[c1 * NT + n] * nb[c2 * NT + n] + scr[c2 * NT + n] * nb[c1 * NT + n]);
          }
        }
      }
      if (tid < 3) {
        if (cnt > 0) unsafeAtomicAdd(p.force + 3 * (size_t) i + tid, own9);
      } else if (tid < 9 && p.vatom) {
        p.vatom[6 * (size_t) row + tid - 3] = own9;
      }
    } else {
      // ---- radial columns, tile after tile: thread (mu, n) sums a_mu(n) and b_mu(n) over the basics of mu, thread
      // (t_n, mu, rho) adds the tile's neighbours of type t_n to its column, in list order
      for (int tile = 0; tile < ntiles; tile++) {
        const int t0 = tile * NT, nt = min(NT, cnt - t0);
        if (ntiles > 1) {
          __syncthreads();
          build_tile<VJP>(p, tab, nb, it, t0, nt, i, itype, row, xi0, xi1, xi2, tid);
          __syncthreads();
        }
        for (int item = tid; item < Mu * NT; item += NTHREADS) {
          const int mu = item / NT, n = item - mu * NT;
          double sa = 0.0, sb = 0.0;
          if (n < nt) {
            const double inv = nb[3 * NT + n], du0 = nb[4 * NT + n], du1 = nb[5 * NT + n], du2 = nb[6 * NT + n], dr = nb[7 * NT + n];
            const double *col = tab + n;
            for (int q = it.mufirst[mu]; q < it.mufirst[mu + 1]; q++) {
              const int k = it.bymu[q];
              const CentreBasic bk = decode_basic(it.pack[k]);
              const int a = bk.a, b = bk.b, c = bk.c;
              const CentreTangent t = basic_tangent(col, Mu, pw0, P, bk, inv);   // (f_mu is Q_rho's factor here: nf and the powers)
              const double pa = t.pa, pb = t.pb, pc = t.pc;
              const double w = t.nf * (pa * (pb * pc));
              double gm = 0.0;
              if (a > 0) gm += (double) a * tangent_low(col, pw0, P, 0, a) * pb * pc * du0;
              if (b > 0) gm += (double) b * pa * tangent_low(col, pw0, P, 1, b) * pc * du1;
              if (c > 0) gm += (double) c * pa * pb * tangent_low(col, pw0, P, 2, c) * du2;
              const double dw = t.nf * gm - (double) bk.nu * w * inv * dr;
              const double dk = D[k];
              sa += (eb * dk + dD[k]) * w + dk * dw;
              sb += dk * w;
            }
            sb *= dr;
          }
          scr[mu * NT + n] = sa;
          scr[(Mu + mu) * NT + n] = sb;
        }
        __syncthreads();
        for (int e = tid; e < blk; e += NTHREADS) {
          const int tj = e / (Mu * R), rem = e - tj * (Mu * R), mu = rem / R, rho = rem - mu * R;
          const double *q = tab + (2 * Mu + rho) * PITCH, *qd = tab + (2 * Mu + R + rho) * PITCH;
          const double *sa = scr + mu * NT, *sb = scr + (Mu + mu) * NT;
          double s = 0.0;
          for (int n = 0; n < nt; n++)
            if (it.nbtype[n] == tj) s += q[n] * sa[n] + qd[n] * sb[n];
          rad[e] += s;
        }
      }
      __syncthreads();
      // ---- the row: [radial | species | moments | padding]
      double *out = p.grad + (size_t) row * p.ld;
      for (int c = tid; c < p.ld; c += NTHREADS) {
        double v = 0.0;
        if (c < nrad) {
          const int e = c - itype * blk;
          if (e >= 0 && e < blk) v = rad[e];
        } else if (c < nrad + Sp) {
          if (c - nrad == itype) v = eb;
        } else if (c < nrad + Sp + S) {
          const int m = it.map[c - nrad - Sp];
          v = eb * M[m] + dM[m];
        }
        out[c] = v;
      }
    }
    __syncthreads();
  }
}

}   // namespace

size_t mtp_train_lds_layout(MtpTrainParams &p)
{
  p.a_pad = (p.A + 1) & ~1;
  p.tab_rows = 2 * p.Mu + 2 * p.R + 4 * p.P;
  p.off_tab = 4 * p.a_pad;
  p.off_nb = p.off_tab + p.tab_rows * MTP_PITCH;
  p.off_scr = p.off_nb + 8 * MTP_TRAIN_NT;
  const int scr_rows = 2 * p.Mu > 3 * NPART ? 2 * p.Mu : 3 * NPART;
  p.off_rad = p.off_scr + scr_rows * MTP_TRAIN_NT;
  p.off_int = p.off_rad + ((p.Sp * p.Mu * p.R + 1) & ~1);
  const size_t ints = 2 * (size_t) p.B + (size_t) p.S + p.nblocks + 1 + p.Mu + 1 + 2 * MTP_TRAIN_NT + (size_t) p.cj_cap + 2;
  return ((size_t) p.off_int + (ints + 1) / 2) * sizeof(double);
}

hipError_t mtp_launch_train_kernel(const MtpTrainParams &p, bool vjp, int grid, size_t lds, hipStream_t st)
{
  static std::atomic<unsigned long long> attr_mask[2];   // (value, vjp: two functions, each with its own limit)
  const void *fn = vjp ? reinterpret_cast<const void *>(&mtp_train_kernel<true>) : reinterpret_cast<const void *>(&mtp_train_kernel<false>);
  const hipError_t e = mtp_raise_lds_limit(fn, attr_mask[vjp]);
  if (e != hipSuccess) return e;
  if (vjp) hipLaunchKernelGGL(mtp_train_kernel<true>, dim3(grid), dim3(NTHREADS), lds, st, p);
  else hipLaunchKernelGGL(mtp_train_kernel<false>, dim3(grid), dim3(NTHREADS), lds, st, p);
  return hipGetLastError();
}
