// Device pieces shared by the kernels that give a whole workgroup to one centre atom (mtp_design.hip, mtp_train.hip;
// internal): the centre check, the neighbour compaction, the decoded table entries, the tile tables, the factors of a basic
// at one neighbour and the level-by-level product pass.  What differs between the kernels stays in the kernel that owns it.
#pragma once

#include "mtp_kernel_common.hpp"

// a basic descriptor (pack: slot | a << 8 | b << 12 | c << 16 | mu << 20) and a packed times row (MtpRow8), decoded
struct CentreBasic {
  int a, b, c, mu, nu;   // nu = a + b + c
};
static __device__ __forceinline__ CentreBasic decode_basic(int pk)
{
  const int a = (pk >> 8) & 15, b = (pk >> 12) & 15, c = (pk >> 16) & 15;
  return {a, b, c, (pk >> 20) & 15, a + b + c};
}
struct CentreRow {   // a3 += mult a0 a1 (moment indices).  Each field is decoded where it is read: all four up front made
  uint32_t lo, hi;   // hipcc pair the shifts of a0 and a3 in one vector operation, three more instructions per row
  __device__ __forceinline__ unsigned a0() const { return (lo & 0xffffu) >> 3; }
  __device__ __forceinline__ unsigned a1() const { return lo >> 19; }
  __device__ __forceinline__ unsigned a3() const { return (hi & 0xffffu) >> 3; }
  __device__ __forceinline__ double mult() const { return (double) ((int) hi >> 16); }
};
static __device__ __forceinline__ CentreRow decode_row(const MtpRow8 &rw) { return {rw.lo, rw.hi}; }

// (uniform) pair_mtp.cpp:91-93: a centre outside the potential's species raises flag 1, one that is not an owned atom 3; its
// outputs are left unassigned: the call has failed, the synchronise says so
static __device__ __forceinline__ bool centre_ok(const MtpCentreParams &p, int i, int itype, int tid)
{
  if (itype < 0 || itype >= p.Sp || (unsigned) i >= (unsigned) p.nowned) {
    if (tid == 0) atomicExch(p.err_flag, itype < 0 || itype >= p.Sp ? 1 : 3);
    return false;
  }
  return true;
}

// compaction by ONE wavefront, in list order: the ids of the row's neighbours inside the cutoff to cj, their count to
// cnt[0] (and back)
static __device__ __forceinline__ int compact_neighbours(const MtpCentreParams &p, int jbeg, int jnum, double xi0, double xi1,
                                                         double xi2, int lane, int *cj, int *cntp)
{
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
        if (jt < 0 || jt >= p.Sp) {   // pair_mtp.cpp:116-118
          atomicExch(p.err_flag, 1);
        } else {
          const double dx = p.x[3 * (size_t) j] - xi0, dy = p.x[3 * (size_t) j + 1] - xi1, dz = p.x[3 * (size_t) j + 2] - xi2;
          in = !(dx * dx + dy * dy + dz * dz > p.cutsq);
        }
      }
    }
    const unsigned long long m = __ballot(in);
    const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
    if (in && pos < p.cj_cap) cj[pos] = j;
    cnt += __popcll(m);
  }
  if (cnt > p.cj_cap) {   // the list's max_numneigh sized the id array: refuse instead of overrunning LDS
    if (lane == 0) atomicExch(p.err_flag, 2);
    cnt = p.cj_cap;
  }
  if (lane == 0) cntp[0] = cnt;
  return cnt;
}

// Tile tables, one column per neighbour (col = tab + n): val_mu | der_mu [Mu each] | the kernel's own rows | r^-nu [P] |
// x^e, y^e, z^e [P each] from row pw0 on.  Eight threads (part = 0..7) share a neighbour: the power rows are dealt from
// the bottom of the eight, the radial functions from the top.
struct CentreGeom {
  double dx, dy, dz, r, inv;
};
static __device__ __forceinline__ CentreGeom tile_geom(const MtpCentreParams &p, int j, double xi0, double xi1, double xi2)
{
  const double dx = p.x[3 * (size_t) j] - xi0, dy = p.x[3 * (size_t) j + 1] - xi1, dz = p.x[3 * (size_t) j + 2] - xi2;
  const double r = sqrt(dx * dx + dy * dy + dz * dz);
  return {dx, dy, dz, r, 1.0 / r};
}
// u and 1 / r to nb rows 0..3 [NT each] (part 0)
template <int NT> static __device__ __forceinline__ void tile_nb(double *nb, int n, double dx, double dy, double dz, double inv)
{
  nb[n] = dx;
  nb[NT + n] = dy;
  nb[2 * NT + n] = dz;
  nb[3 * NT + n] = inv;
}
// part 0: the r^-nu row; parts 1..3: the power rows of x, y, z
static __device__ __forceinline__ void tile_powers(double *col, int pw0, int P, int part, double dx, double dy, double dz, double inv)
{
  if (part == 0) {
    double rp = 1.0;
    for (int nu = 0; nu < P; nu++) {
      col[(pw0 + nu) * MTP_PITCH] = rp;
      rp *= inv;
    }
  } else if (part <= 3) {
    const double u = part == 1 ? dx : part == 2 ? dy : dz;
    double cur = 1.0;
    double *cp = col + (size_t) (pw0 + part * P) * MTP_PITCH;
    for (int e = 0; e < P; e++) {
      cp[e * MTP_PITCH] = cur;
      cur *= u;
    }
  }
}
// val_mu = sum_rho c[mu][rho] Q_rho(r) and der_mu (with Q'_rho) for this part's share of mu; radial [.][Mu][R], pair = the
// block of the two species.  Q_ri(r) and dQ_ri/dr: mtp_rb_chevbyshev_basis.cpp:29-54.  KEEP: the thread of mu = 0
// stores Q_rho | Q'_rho [R each] from row 2 Mu on as well
template <bool KEEP> static __device__ __forceinline__ void tile_radial(const MtpCentreParams &p, const double *radial, int pair,
                                                                        double r, double *col, int part)
{
  const int Mu = p.Mu, R = p.R;
  const double d = r - p.rmax, mult = 2.0 * p.inv_span;
  const double ksi = (2.0 * r - (p.rmin + p.rmax)) * p.inv_span;
  for (int mu = 7 - part; mu < Mu; mu += 8) {
    const double *c = radial + (size_t) (pair * Mu + mu) * R;
    const bool keep = KEEP && mu == 0;
    double q0 = p.scaling * (d * d), q1 = p.scaling * (ksi * d * d);
    double e0 = p.scaling * 2.0 * d, e1 = p.scaling * (mult * d * d + 2.0 * ksi * d);
    double val = c[0] * q0, der = c[0] * e0;
    if (keep) {
      col[(2 * Mu) * MTP_PITCH] = q0;
      col[(2 * Mu + R) * MTP_PITCH] = e0;
    }
    if (R > 1) {
      val += c[1] * q1;
      der += c[1] * e1;
      if (keep) {
        col[(2 * Mu + 1) * MTP_PITCH] = q1;
        col[(2 * Mu + R + 1) * MTP_PITCH] = e1;
      }
    }
    for (int ri = 2; ri < R; ri++) {
      const double q2 = 2.0 * ksi * q1 - q0;
      const double e2 = 2.0 * (mult * q1 + ksi * e1) - e0;
      val += c[ri] * q2;
      der += c[ri] * e2;
      if (keep) {
        col[(2 * Mu + ri) * MTP_PITCH] = q2;
        col[(2 * Mu + R + ri) * MTP_PITCH] = e2;
      }
      q0 = q1;
      q1 = q2;
      e0 = e1;
      e1 = e2;
    }
    col[mu * MTP_PITCH] = val;
    col[(Mu + mu) * MTP_PITCH] = der;
  }
}

// The factors of the tangent of basic k at one neighbour (column col of the tile, pair_mtp.cpp:163-191):
//   m_k = val x^a y^b z^c,   d m_k / d u_c = pa pb pc (der / r) u_c + val e_c low(c) (the other two powers)
// nf = r^-nu, val = f_mu / r^nu, der = d val / dr, pa, pb, pc = x^a, y^b, z^c; tangent_low = the power e - 1 of coordinate c
// (the chain rule of the monomial).  The callers keep their own products: each scales and associates them its own way.
struct CentreTangent {
  double nf, val, der, pa, pb, pc;
};
static __device__ __forceinline__ double tangent_low(const double *col, int pw0, int P, int c, int e)
{
  return col[(pw0 + (1 + c) * P + e - 1) * MTP_PITCH];
}
static __device__ __forceinline__ CentreTangent basic_tangent(const double *col, int Mu, int pw0, int P, const CentreBasic k, double inv)
{
  CentreTangent t;
  t.nf = col[(pw0 + k.nu) * MTP_PITCH];
  t.val = col[k.mu * MTP_PITCH] * t.nf;
  t.der = col[(Mu + k.mu) * MTP_PITCH] * t.nf - (double) k.nu * t.val * inv;
  t.pa = col[(pw0 + P + k.a) * MTP_PITCH];
  t.pb = col[(pw0 + 2 * P + k.b) * MTP_PITCH];
  t.pc = col[(pw0 + 3 * P + k.c) * MTP_PITCH];
  return t;
}

// The times rows, one dependency level at a time (rows of a level commute; padding rows add zero), rows t, t + STRIDE, ...
// of every level: VALUE: M[a3] += mult M[a0] M[a1]; TANGENT: dM[a3] += mult (dM[a0] M[a1] + M[a0] dM[a1]).  STRIDE = 64:
// one wavefront on images of its own (a wave fence after each level), else the workgroup (a barrier)
template <bool VALUE, bool TANGENT, int STRIDE>
static __device__ __forceinline__ void product_pass(const MtpRow8 *rows, const int *level, int nblocks, double *M, double *dM, int t)
{
  for (int l = 0; l < nblocks; l++) {
    for (int r = level[l] + t; r < level[l + 1]; r += STRIDE) {
      const CentreRow w = decode_row(rows[r]);
      const unsigned a0 = w.a0(), a1 = w.a1();
      if (VALUE) {
        const double v = M[a0] * M[a1];
        lds_add(&M[w.a3()], w.mult() * v);
      }
      if (TANGENT) {
        const double v = dM[a0] * M[a1] + M[a0] * dM[a1];
        lds_add(&dM[w.a3()], w.mult() * v);
      }
    }
    if (STRIDE == 64) wave_fence();
    else __syncthreads();
  }
}
