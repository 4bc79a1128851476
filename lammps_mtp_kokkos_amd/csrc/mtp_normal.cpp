// Host-only solver of the normal-equation refit (include/mtp_mi355x.h, "linear refit without the design matrix"): builds with
// g++ alone and makes no HIP call.  Everything here is double-double (mtp_dd.hpp); only the outputs are rounded to fp64.
//
// mtp_normal_factor: G = sum_k w_k G_k, then a Cholesky factorisation with diagonal pivoting over the first ncols columns,
// the target column riding along.  At every step the pivot is the remaining column with the largest ratio
// (remaining diagonal) / (original diagonal); the factorisation stops when that ratio is <= drop.  With G = A^T A the rows
// of R are Q^T A for an orthonormal Q, so R has the singular values of A and lstsq(R, Q^T y) is lstsq(A, y).
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

#include "../../include/mtp_mi355x.h"
#include "mtp_dd.hpp"

namespace {

bool finite_all(const double *a, size_t n)
{
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(a[i])) return false;
  return true;
}

}   // namespace

int mtp_normal_factor(int n, const double *const hi[3], const double *const lo[3], const double weights[3], const double *theta0,
                      double drop, double *R, double *q, int *rank_out, int *pivot_order, int *dropped, int *ndropped_out,
                      double *pivot_ratios)
{
  if (n < 2 || !hi || !lo || !weights || !theta0 || !R || !q || !rank_out || !(drop >= 0.0) || !std::isfinite(drop)) return MTP_ERR_ARG;
  const int ncols = n - 1;
  const size_t nn = (size_t) n * n;
  if (!finite_all(theta0, ncols)) return MTP_ERR_ARG;
  bool any = false;
  for (int k = 0; k < 3; k++) {
    if (!(weights[k] >= 0.0) || !std::isfinite(weights[k])) return MTP_ERR_ARG;
    if (weights[k] == 0.0 || !hi[k]) continue;
    if (!lo[k] || !finite_all(hi[k], nn) || !finite_all(lo[k], nn)) return MTP_ERR_ARG;
    for (int j = 0; j < n; j++)
      if (hi[k][(size_t) j * n + j] < 0.0) return MTP_ERR_ARG;
    any = true;
  }
  if (!any) return MTP_ERR_ARG;
  try {
    // the weighted sum; only the upper triangle (j <= c) is used from here on
    std::vector<mtp_dd> A(nn, mtp_dd{0.0, 0.0});
    for (int k = 0; k < 3; k++) {
      if (weights[k] == 0.0 || !hi[k]) continue;
      for (int j = 0; j < n; j++)
        for (int c = j; c < n; c++) {
          const size_t at = (size_t) j * n + c;
          A[at] = dd_add(A[at], dd_mul_d(mtp_dd{hi[k][at], lo[k][at]}, weights[k]));
        }
    }
    std::vector<mtp_dd> d0(ncols);
    std::vector<int> rem;   // the columns still to be eliminated, ascending
    std::vector<int> drop_col;         // dropped columns and their ratios, in the order they were dropped
    std::vector<double> drop_ratio;
    for (int j = 0; j < ncols; j++) {
      d0[j] = A[(size_t) j * n + j];
      if (d0[j].hi > 0.0) {
        rem.push_back(j);
      } else {   // a zero diagonal: the column is zero
        drop_col.push_back(j);
        drop_ratio.push_back(0.0);
      }
    }
    std::vector<mtp_dd> row(n);
    int rank = 0;
    while (!rem.empty()) {
      // the pivot: the largest remaining diagonal relative to the original one
      size_t best = 0;
      double best_ratio = -1.0;
      for (size_t t = 0; t < rem.size(); t++) {
        const int j = rem[t];
        const double ratio = dd_round(dd_div(A[(size_t) j * n + j], d0[j]));
        if (ratio > best_ratio) best_ratio = ratio, best = t;
      }
      if (!(best_ratio > drop)) {   // every remaining column is refused: their ratios are the gap's far side
        for (size_t t = 0; t < rem.size(); t++) {
          const int j = rem[t];
          drop_col.push_back(j);
          drop_ratio.push_back(dd_round(dd_div(A[(size_t) j * n + j], d0[j])));
        }
        break;
      }
      const int p = rem[best];
      rem.erase(rem.begin() + (std::ptrdiff_t) best);
      if (pivot_order) pivot_order[rank] = p;
      if (pivot_ratios) pivot_ratios[rank] = best_ratio;
      const mtp_dd piv = dd_sqrt(A[(size_t) p * n + p]);
      // row `rank` of the factor over the remaining columns and the target; zero where a column was eliminated before
      for (int c = 0; c < n; c++) row[c] = mtp_dd{0.0, 0.0};
      row[p] = piv;
      for (size_t t = 0; t <= rem.size(); t++) {
        const int c = t < rem.size() ? rem[t] : ncols;
        const mtp_dd a = p < c ? A[(size_t) p * n + c] : A[(size_t) c * n + p];
        row[c] = dd_div(a, piv);
      }
      // the Schur complement of the remaining columns, the target column and the target's own diagonal entry
      for (size_t s = 0; s <= rem.size(); s++) {
        const int a = s < rem.size() ? rem[s] : ncols;
        for (size_t t = s; t <= rem.size(); t++) {
          const int c = t < rem.size() ? rem[t] : ncols;
          const size_t at = (size_t) a * n + c;
          A[at] = dd_sub(A[at], dd_mul(row[a], row[c]));
        }
      }
      // outputs of this row: R rounded, q = (Q^T y) - R theta0 formed in double-double
      mtp_dd z = row[ncols];
      for (int c = 0; c < ncols; c++) {
        R[(size_t) rank * ncols + c] = dd_round(row[c]);
        if (row[c].hi != 0.0 || row[c].lo != 0.0) z = dd_sub(z, dd_mul_d(row[c], theta0[c]));
      }
      q[rank] = dd_round(z);
      rank++;
    }
    *rank_out = rank;   // rank + dropped = ncols: pivot_ratios holds the kept ratios, then those of `dropped`
    for (size_t t = 0; t < drop_col.size(); t++) {
      if (dropped) dropped[t] = drop_col[t];
      if (pivot_ratios) pivot_ratios[rank + t] = drop_ratio[t];
    }
    if (ndropped_out) *ndropped_out = (int) drop_col.size();
  } catch (const std::bad_alloc &) {
    return MTP_ERR_LIMIT;
  }
  return MTP_OK;
}

int mtp_normal_quadratic(int n, const double *hi, const double *lo, const double *theta, double *out)
{
  if (n < 2 || !hi || !lo || !theta || !out) return MTP_ERR_ARG;
  const int ncols = n - 1;
  if (!finite_all(theta, ncols) || !finite_all(hi, (size_t) n * n) || !finite_all(lo, (size_t) n * n)) return MTP_ERR_ARG;
  // v^T G v with v = (theta, -1): y^T y - 2 theta^T g + theta^T G theta
  mtp_dd sum{0.0, 0.0};
  for (int j = 0; j < n; j++) {
    const double vj = j < ncols ? theta[j] : -1.0;
    if (vj == 0.0) continue;
    mtp_dd r{0.0, 0.0};
    for (int c = 0; c < n; c++) {
      const double vc = c < ncols ? theta[c] : -1.0;
      const size_t at = (size_t) j * n + c;
      r = dd_add(r, dd_mul_d(mtp_dd{hi[at], lo[at]}, vc));
    }
    sum = dd_add(sum, dd_mul_d(r, vj));
  }
  const double v = dd_round(sum);
  *out = v > 0.0 ? v : 0.0;
  return MTP_OK;
}
