// Stand-alone program (ASan + UBSan build: host/Makefile `san_normal`) of the normal-equation refit's host-only code: the
// double-double arithmetic of csrc/mtp_dd.hpp and the solver of csrc/mtp_normal.cpp.
//
//   test_normal_san MATRIX
// MATRIX is text: "m ncols", then m lines of ncols + 2 C hexadecimal floats: scale, the row, the target.  The program
// accumulates the augmented Gram matrix with dd_mac as the kernel does (b = fl(scale * value), rows of scale 0 skipped, one
// slice, normalised at the end) and prints
//   GRAM n            then n * n lines "hi lo"
//   FACTOR rank ndropped, then rank lines of R (ncols numbers each), one line of q, one of the pivot order, one of the
//                     dropped columns and one of the ncols pivot ratios
//   QUADRATIC v       mtp_normal_quadratic at theta = 0 (the target's squared norm)
// all as hexadecimal floats.  tests/test_normal_cpu.py judges the pairs with fractions.Fraction.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/mtp_mi355x.h"
#include "../../lammps_mtp_kokkos_amd/csrc/mtp_dd.hpp"

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int m = 0, ncols = 0;
  if (std::fscanf(f, "%d %d", &m, &ncols) != 2 || m < 0 || ncols < 1) return 2;
  const int n = ncols + 1;
  std::vector<mtp_dd> acc((size_t) n * n, mtp_dd{0.0, 0.0});
  std::vector<double> b(n), line(ncols + 2);
  for (int i = 0; i < m; i++) {
    for (int c = 0; c < ncols + 2; c++) {
      char word[64];
      if (std::fscanf(f, "%63s", word) != 1) return 2;
      line[c] = std::strtod(word, nullptr);
    }
    if (line[0] == 0.0) continue;
    for (int c = 0; c < n; c++) b[c] = line[0] * line[1 + c];
    for (int j = 0; j < n; j++)
      for (int k = 0; k < n; k++) acc[(size_t) j * n + k] = dd_mac(acc[(size_t) j * n + k], b[j], b[k]);
  }
  std::fclose(f);
  std::vector<double> hi((size_t) n * n), lo((size_t) n * n);
  std::printf("GRAM %d\n", n);
  for (size_t e = 0; e < acc.size(); e++) {
    const mtp_dd v = dd_normal(acc[e]);
    hi[e] = v.hi;
    lo[e] = v.lo;
    std::printf("%a %a\n", v.hi, v.lo);
  }
  const double *his[3] = {hi.data(), nullptr, nullptr}, *los[3] = {lo.data(), nullptr, nullptr};
  const double weights[3] = {1.0, 0.0, 0.0};
  std::vector<double> theta0(ncols, 0.0), R((size_t) ncols * ncols, 0.0), q(ncols, 0.0), ratios(ncols, 0.0);
  std::vector<int> order(ncols, -1), dropped(ncols, -1);
  int rank = 0, ndropped = 0;
  int rc = mtp_normal_factor(n, his, los, weights, theta0.data(), 0x1p-80, R.data(), q.data(), &rank, order.data(), dropped.data(),
                             &ndropped, ratios.data());
  if (rc != MTP_OK) {
    std::printf("FACTOR failed %d\n", rc);
    return 1;
  }
  std::printf("FACTOR %d %d\n", rank, ndropped);
  for (int r = 0; r < rank; r++) {
    for (int c = 0; c < ncols; c++) std::printf("%a ", R[(size_t) r * ncols + c]);
    std::printf("\n");
  }
  for (int r = 0; r < rank; r++) std::printf("%a ", q[r]);
  std::printf("\n");
  for (int r = 0; r < rank; r++) std::printf("%d ", order[r]);
  std::printf("\n");
  for (int r = 0; r < ndropped; r++) std::printf("%d ", dropped[r]);
  std::printf("\n");
  for (int r = 0; r < ncols; r++) std::printf("%a ", ratios[r]);
  std::printf("\n");
  double v = -1.0;
  rc = mtp_normal_quadratic(n, hi.data(), lo.data(), theta0.data(), &v);
  if (rc != MTP_OK) return 1;
  std::printf("QUADRATIC %a\n", v);
  // the refusals: a negative weight, a non-finite entry, a negative diagonal
  const double bad_w[3] = {-1.0, 0.0, 0.0};
  if (mtp_normal_factor(n, his, los, bad_w, theta0.data(), 0x1p-80, R.data(), q.data(), &rank, nullptr, nullptr, nullptr, nullptr) !=
      MTP_ERR_ARG)
    return 1;
  std::vector<double> dmg(hi);
  dmg[0] = -1.0;
  const double *dh[3] = {dmg.data(), nullptr, nullptr};
  if (mtp_normal_factor(n, dh, los, weights, theta0.data(), 0x1p-80, R.data(), q.data(), &rank, nullptr, nullptr, nullptr, nullptr) !=
      MTP_ERR_ARG)
    return 1;
  dmg[0] = hi[0] / 0.0;
  if (mtp_normal_quadratic(n, dmg.data(), lo.data(), theta0.data(), &v) != MTP_ERR_ARG) return 1;
  std::printf("OK\n");
  return 0;
}
