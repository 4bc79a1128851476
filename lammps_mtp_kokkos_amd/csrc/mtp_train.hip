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

#include <atomic>

#include "mtp_kernel_common.hpp"

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
    const double dx = p.x[3 * (size_t) j] - xi0, dy = p.x[3 * (size_t) j + 1] - xi1, dz = p.x[3 * (size_t) j + 2] - xi2;
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    const double inv = 1.0 / r;
    const int Mu = p.Mu, P = p.P, R = p.R;
    const int pw0 = 2 * Mu + 2 * R;
    double *col = tab + n;
    const int jt = p.type[j] - 1;   // (inside the potential: the compaction dropped the others)
    if (part == 0) {
      nb[n] = dx;
      nb[NT + n] = dy;
      nb[2 * NT + n] = dz;
      nb[3 * NT + n] = inv;
      it.nbtype[n] = jt;
      double rp = 1.0;
      for (int nu = 0; nu < P; nu++) {
        col[(pw0 + nu) * PITCH] = rp;
        rp *= inv;
      }
    } else if (part <= 3) {
      const double u = part == 1 ? dx : part == 2 ? dy : dz;
      double cur = 1.0;
      double *cp = col + (size_t) (pw0 + part * P) * PITCH;
      for (int e = 0; e < P; e++) {
        cp[e * PITCH] = cur;
        cur *= u;
      }
    } else if (part == 4) {
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
    // Q_ri(r) and dQ_ri/dr (mtp_rb_chevbyshev_basis.cpp:29-54); the thread of mu = 0 keeps them
    const double d = r - p.rmax, mult = 2.0 * p.inv_span;
    const double ksi = (2.0 * r - (p.rmin + p.rmax)) * p.inv_span;
    for (int mu = 7 - part; mu < Mu; mu += 8) {
      const double *c = p.theta + (size_t) ((itype * p.Sp + jt) * Mu + mu) * R;
      const bool keep = mu == 0;
      double q0 = p.scaling * (d * d), q1 = p.scaling * (ksi * d * d);
      double e0 = p.scaling * 2.0 * d, e1 = p.scaling * (mult * d * d + 2.0 * ksi * d);
      double val = c[0] * q0, der = c[0] * e0;
      if (keep) {
        col[(2 * Mu) * PITCH] = q0;
        col[(2 * Mu + R) * PITCH] = e0;
      }
      if (R > 1) {
        val += c[1] * q1;
        der += c[1] * e1;
        if (keep) {
          col[(2 * Mu + 1) * PITCH] = q1;
          col[(2 * Mu + R + 1) * PITCH] = e1;
        }
      }
      for (int ri = 2; ri < R; ri++) {
        const double q2 = 2.0 * ksi * q1 - q0;
        const double e2 = 2.0 * (mult * q1 + ksi * e1) - e0;
        val += c[ri] * q2;
        der += c[ri] * e2;
        if (keep) {
          col[(2 * Mu + ri) * PITCH] = q2;
          col[(2 * Mu + R + ri) * PITCH] = e2;
        }
        q0 = q1;
        q1 = q2;
        e0 = e1;
        e1 = e2;
      }
      col[mu * PITCH] = val;
      col[(Mu + mu) * PITCH] = der;
    }
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
    if (itype < 0 || itype >= Sp || (unsigned) i >= (unsigned) p.nowned) {   // (uniform) pair_mtp.cpp:91-93
      if (tid == 0) atomicExch(p.err_flag, itype < 0 || itype >= Sp ? 1 : 3);
      continue;   // its outputs are left unassigned: the call has failed, the synchronise says so
    }
    const double xi0 = p.x[3 * (size_t) i], xi1 = p.x[3 * (size_t) i + 1], xi2 = p.x[3 * (size_t) i + 2];
    const int jbeg = p.first[ii], jnum = p.first[ii + 1] - jbeg;
    const double eb = VJP && p.ebar ? p.ebar[row] : 0.0;

    // ---- compaction (wavefront 0, in list order); the images zeroed by all
    if (wave == 0) {
      int cnt = 0;
      for (int c0 = 0; c0 < jnum; c0 += 64) {
        const int jj = c0 + lane;
        bool in = false;
        int j = 0;
        if (jj < jnum) {
          j = p.neigh[jbeg + jj] & MTP_NEIGHMASK;
          if ((unsigned) j >= (unsigned) p.nall) {
            atomicExch(p.err_flag, 3);
          } else {
            const int jt = p.type[j] - 1;
            if (jt < 0 || jt >= Sp) {   // pair_mtp.cpp:116-118
              atomicExch(p.err_flag, 1);
            } else {
              const double dx = p.x[3 * (size_t) j] - xi0, dy = p.x[3 * (size_t) j + 1] - xi1, dz = p.x[3 * (size_t) j + 2] - xi2;
              in = !(dx * dx + dy * dy + dz * dz > p.cutsq);
            }
          }
        }
        const unsigned long long m = __ballot(in);
        const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (in && pos < p.cj_cap) it.cj[pos] = j;
        cnt += __popcll(m);
      }
      if (cnt > p.cj_cap) {   // the list's max_numneigh sized the id array: refuse instead of overrunning LDS
        if (lane == 0) atomicExch(p.err_flag, 2);
        cnt = p.cj_cap;
      }
      if (lane == 0) it.cnt[0] = cnt;
    }
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
        const int pk = it.pack[k];
        const int a = (pk >> 8) & 15, b = (pk >> 12) & 15, c = (pk >> 16) & 15, mu = (pk >> 20) & 15, nu = a + b + c;
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
    // ---- products, one dependency level at a time (rows of a level commute; padding rows add zero)
    for (int l = 0; l < p.nblocks; l++) {
      for (int r = it.level[l] + tid; r < it.level[l + 1]; r += NTHREADS) {
        const MtpRow8 rw = p.rows[r];
        const int a0 = (rw.lo & 0xffffu) >> 3, a1 = rw.lo >> 19, a3 = (rw.hi & 0xffffu) >> 3;
        const double m = (double) ((int) rw.hi >> 16);
        lds_add(&M[a3], m * (M[a0] * M[a1]));
        if (VJP) lds_add(&dM[a3], m * (dM[a0] * M[a1] + M[a0] * dM[a1]));
      }
      __syncthreads();
    }
    // ---- adjoint: seeded by assignment with the moment coefficients (one scalar per moment: the table was checked), swept
    // through the levels in reverse; a row's target is complete before its level is reached
    for (int s = tid; s < S; s += NTHREADS) D[it.map[s]] = xi[s];
    __syncthreads();
    for (int l = p.nblocks - 1; l >= 0; l--) {
      for (int r = it.level[l] + tid; r < it.level[l + 1]; r += NTHREADS) {
        const MtpRow8 rw = p.rows[r];
        const int a0 = (rw.lo & 0xffffu) >> 3, a1 = rw.lo >> 19, a3 = (rw.hi & 0xffffu) >> 3;
        const double m = (double) ((int) rw.hi >> 16);
        const double d3 = m * D[a3], m0 = M[a0], m1 = M[a1];
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
              const int pk = it.pack[k];
              const int a = (pk >> 8) & 15, b = (pk >> 12) & 15, c = (pk >> 16) & 15, mu = (pk >> 20) & 15, nu = a + b + c;
              const double nf = col[(pw0 + nu) * PITCH];
              const double val = col[mu * PITCH] * nf;
              const double der = col[(Mu + mu) * PITCH] * nf - (double) nu * val * inv;
              const double pa = col[(pw0 + P + a) * PITCH], pb = col[(pw0 + 2 * P + b) * PITCH], pc = col[(pw0 + 3 * P + c) * PITCH];
              const double dk = D[k];
              const double rad_part = dk * (pa * pb * pc) * (der * inv);
              double g0 = rad_part * u0, g1 = rad_part * u1, g2 = rad_part * u2;
              const double dv = dk * val;
              if (a > 0) g0 += dv * (double) a * col[(pw0 + P + a - 1) * PITCH] * pb * pc;
              if (b > 0) g1 += dv * (double) b * pa * col[(pw0 + 2 * P + b - 1) * PITCH] * pc;
              if (c > 0) g2 += dv * (double) c * pa * pb * col[(pw0 + 3 * P + c - 1) * PITCH];
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
              const int pk = it.pack[k];
              const int a = (pk >> 8) & 15, b = (pk >> 12) & 15, c = (pk >> 16) & 15, nu = a + b + c;
              const double nf = col[(pw0 + nu) * PITCH];
              const double pa = col[(pw0 + P + a) * PITCH], pb = col[(pw0 + 2 * P + b) * PITCH], pc = col[(pw0 + 3 * P + c) * PITCH];
              const double w = nf * (pa * (pb * pc));
              double gm = 0.0;
              if (a > 0) gm += (double) a * col[(pw0 + P + a - 1) * PITCH] * pb * pc * du0;
              if (b > 0) gm += (double) b * pa * col[(pw0 + 2 * P + b - 1) * PITCH] * pc * du1;
              if (c > 0) gm += (double) c * pa * pb * col[(pw0 + 3 * P + c - 1) * PITCH] * du2;
              const double dw = nf * gm - (double) nu * w * inv * dr;
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
  // the dynamic-LDS limit is a per-device attribute of each function: one bit per device id (as the design launcher)
  static std::atomic<unsigned long long> attr_mask{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev > 63 || !((attr_mask.load(std::memory_order_acquire) >> dev) & 1ull)) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&mtp_train_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&mtp_train_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev <= 63) attr_mask.fetch_or(1ull << dev, std::memory_order_release);
  }
  if (vjp) hipLaunchKernelGGL(mtp_train_kernel<true>, dim3(grid), dim3(NTHREADS), lds, st, p);
  else hipLaunchKernelGGL(mtp_train_kernel<false>, dim3(grid), dim3(NTHREADS), lds, st, p);
  return hipGetLastError();
}
