// Sanitizer driver for the host-only parts of the training gradient (include/mtp_mi355x.h, "training gradient"): the
// training table builder (mtp_build_train_table, mtp_potential_train_table) and the writer of all coefficients
// (mtp_potential_write_all_coeffs), csrc/mtp_potential.cpp.  Built with -fsanitize=address,undefined by
// `make -C lammps_mtp_kokkos_amd/host san_train`; tests/test_train_cpu.py runs it on every committed potential.
// No GPU, no HIP runtime.
//
//   test_train_san <potential> <output file>     prints "OK <writer's return value> <late row> <dup scalar>" or "ERR <what>"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mtp_mi355x.h"
#include "../../lammps_mtp_kokkos_amd/csrc/mtp_potential.hpp"

static int fail(const std::string &what)
{
  std::printf("ERR %s\n", what.c_str());
  return 1;
}

int main(int argc, char **argv)
{
  if (argc < 3) return 2;
  mtp_potential pot;
  std::string err;
  if (mtp_parse_file(argv[1], false, pot, err) != 0) return fail(err);
  const int B = pot.alpha_index_basic_count, S = pot.alpha_scalar_count, Sp = pot.species_count, Mu = pot.radial_func_count;
  const int nrad = Sp * Sp * Mu * pot.radial_basis_size;

  // ---- the table through the C entry point, sized by its own counts; the refusal conditions recomputed in file order
  int32_t counts[6] = {0, 0, 0, 0, 0, 0}, refused[2] = {0, 0};
  char msg[512];
  int rc = mtp_potential_train_table(&pot, counts, nullptr, nullptr, nullptr, nullptr, 0);
  if (rc != 0 && rc != MTP_ERR_UNSUPPORTED) return fail("counts");
  if (counts[3] != B || counts[4] != Mu || counts[5] != nrad + Sp + S || counts[2] != pot.alpha_moment_count) return fail("inconsistent counts");
  std::vector<int32_t> bymu((size_t) B), mufirst((size_t) Mu + 1);
  rc = mtp_potential_train_table(&pot, nullptr, bymu.data(), mufirst.data(), refused, msg, 16);   // (a short message buffer)
  if (rc != 0 && rc != MTP_ERR_UNSUPPORTED) return fail("tables");
  rc = mtp_potential_train_table(&pot, nullptr, bymu.data(), mufirst.data(), refused, msg, sizeof msg);
  if ((rc == 0) != (refused[0] < 0 && refused[1] < 0)) return fail("return code and refusal flags disagree");
  if (rc != 0 && !msg[0]) return fail("a refusal without a message");
  int32_t pack_counts[4];
  std::vector<int32_t> pack((size_t) B);
  if (mtp_potential_design_table(&pot, pack_counts, nullptr, nullptr, nullptr, nullptr, pack.data()) != 0) return fail("pack");
  if (mufirst.front() != 0 || mufirst.back() != B) return fail("mu offsets");
  std::vector<char> seen((size_t) B, 0);
  for (int mu = 0; mu < Mu; mu++)
    for (int q = mufirst[(size_t) mu]; q < mufirst[(size_t) mu + 1]; q++) {
      const int k = bymu[(size_t) q];
      if (k < 0 || k >= B || seen[(size_t) k] || ((pack[(size_t) k] >> 20) & 15) != mu) return fail("basics by mu");
      seen[(size_t) k] = 1;
    }
  int late = -1, dup = -1;
  const int T = pot.alpha_index_times_count;
  for (int k = 0; k < T && late < 0; k++)
    for (int j = k; j < T && late < 0; j++) {
      const int a3 = pot.alpha_index_times[4 * (size_t) j + 3];
      if (a3 == pot.alpha_index_times[4 * (size_t) k] || a3 == pot.alpha_index_times[4 * (size_t) k + 1]) late = k;
    }
  for (int s = 0; s < S && dup < 0; s++)
    for (int q = 0; q < s && dup < 0; q++)
      if (pot.alpha_moment_mapping[(size_t) q] == pot.alpha_moment_mapping[(size_t) s]) dup = s;
  if (late != refused[0] || dup != refused[1]) return fail("refusal conditions differ from the file-order scan");

  // ---- the writer: refusals first (nothing may be written), then new coefficients that must read back bit for bit
  unsigned long long rng = 4711;
  auto next = [&]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double) (rng >> 11) / 9007199254740992.0 - 0.5;
  };
  std::vector<double> ra(pot.radial_basis_coeffs), mo(pot.linear_coeffs), sp(pot.species_coeffs);
  for (double &v : ra) v = v * (1.0 + 0.25 * next()) + 1e-3 * next();
  for (double &v : mo) v = v * (1.0 + 0.25 * next()) + 1e-3 * next();
  for (double &v : sp) v += next();
  if (mtp_potential_write_all_coeffs(argv[1], argv[2], ra.data(), sp.data(), mo.data(), nrad + 1, Sp, S, msg, sizeof msg) != MTP_ERR_ARG)
    return fail("a wrong radial count was accepted");
  if (mtp_potential_write_all_coeffs(argv[1], argv[2], ra.data(), sp.data(), mo.data(), nrad, Sp, S + 1, msg, 8) != MTP_ERR_ARG)
    return fail("a wrong moment count was accepted");
  {
    std::vector<double> bad(ra);
    bad.front() = std::numeric_limits<double>::infinity();
    if (mtp_potential_write_all_coeffs(argv[1], argv[2], bad.data(), nullptr, mo.data(), nrad, 0, S, msg, sizeof msg) != MTP_ERR_ARG)
      return fail("an infinite radial coefficient was accepted");
  }
  if (FILE *f = std::fopen(argv[2], "rb")) {
    std::fclose(f);
    return fail("a refused call left a file");
  }
  const int wrote = mtp_potential_write_all_coeffs(argv[1], argv[2], ra.data(), sp.data(), mo.data(), nrad, Sp, S, msg, sizeof msg);
  if (wrote < 0) return fail(msg);
  mtp_potential back;
  if (mtp_parse_text_file(argv[2], false, back, err) != 0) return fail("written file: " + err);
  if (back.radial_basis_coeffs.size() != ra.size() ||
      std::memcmp(back.radial_basis_coeffs.data(), ra.data(), sizeof(double) * ra.size()) != 0 ||
      back.linear_coeffs.size() != mo.size() || std::memcmp(back.linear_coeffs.data(), mo.data(), sizeof(double) * mo.size()) != 0 ||
      back.species_coeffs.size() != sp.size() || std::memcmp(back.species_coeffs.data(), sp.data(), sizeof(double) * sp.size()) != 0)
    return fail("coefficients do not read back bit for bit");
  if (back.alpha_index_times != pot.alpha_index_times || back.alpha_index_basic != pot.alpha_index_basic ||
      back.alpha_moment_mapping != pot.alpha_moment_mapping)
    return fail("another table changed");
  std::printf("OK %d %d %d\n", wrote, refused[0], refused[1]);
  return 0;
}
