// Sanitizer driver for the host-only parts of the linear refit (include/mtp_mi355x.h, "linear refit"): the tangent
// kernel's table builder (mtp_build_design_table, mtp_potential_design_table) and the coefficient writer
// (mtp_potential_write_coeffs), csrc/mtp_potential.cpp.  Built with -fsanitize=address,undefined by
// `make -C lammps_mtp_kokkos_amd/host san_design`; tests/test_design_cpu.py runs it on every committed potential.
// No GPU, no HIP runtime.
//
//   test_design_san <potential> <output file>     prints "OK <writer's return value> <replay error>" or "ERR <what>"
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
  const int A = pot.alpha_moment_count, B = pot.alpha_index_basic_count, T = pot.alpha_index_times_count;
  const int S = pot.alpha_scalar_count, Sp = pot.species_count;

  // ---- the table: through the C entry point, sized by its own counts, then replayed (values and tangents) against the
  // file-order loop of pair_mtp.cpp:196-201 on pseudo-random basics
  int32_t counts[4] = {0, 0, 0, 0};
  if (mtp_potential_design_table(&pot, counts, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return fail("counts");
  if (counts[2] != A || counts[3] != B || counts[0] < T || counts[1] < 1) return fail("inconsistent counts");
  std::vector<int32_t> rows((size_t) 4 * counts[0]), level((size_t) counts[1] + 1), smap((size_t) S), fmap((size_t) S),
      pack((size_t) B);
  if (mtp_potential_design_table(&pot, nullptr, rows.data(), level.data(), smap.data(), fmap.data(), pack.data()) != 0)
    return fail("tables");
  if (level.front() != 0 || level.back() != counts[0]) return fail("level offsets");
  std::vector<double> m((size_t) A, 0.0), g((size_t) A, 0.0), M((size_t) A, 0.0), G((size_t) A, 0.0);
  unsigned long long rng = 4711;
  auto next = [&]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double) (rng >> 11) / 9007199254740992.0 - 0.5;
  };
  for (int k = 0; k < B; k++) {
    m[(size_t) k] = next();
    g[(size_t) k] = next();
  }
  for (int k = 0; k < B; k++) {   // the table's basics are a permutation of the file's, named by their descriptors
    const int pk = pack[(size_t) k];
    const int32_t want[4] = {(pk >> 20) & 15, (pk >> 8) & 15, (pk >> 12) & 15, (pk >> 16) & 15};
    int file = -1;
    for (int q = 0; q < B && file < 0; q++)
      if (std::memcmp(&pot.alpha_index_basic[4 * (size_t) q], want, sizeof want) == 0) file = q;
    if (file < 0) return fail("basic descriptor without a basic");
    M[(size_t) k] = m[(size_t) file];
    G[(size_t) k] = g[(size_t) file];
  }
  for (int k = 0; k < T; k++) {
    const int32_t *q = &pot.alpha_index_times[4 * (size_t) k];
    m[(size_t) q[3]] += q[2] * m[(size_t) q[0]] * m[(size_t) q[1]];
  }
  for (int k = 0; k < T; k++) {   // tangents with the FINAL moments: the transpose of the reverse sweep, :221-233
    const int32_t *q = &pot.alpha_index_times[4 * (size_t) k];
    g[(size_t) q[3]] += q[2] * (g[(size_t) q[0]] * m[(size_t) q[1]] + m[(size_t) q[0]] * g[(size_t) q[1]]);
  }
  for (int pass = 0; pass < 2; pass++)   // as the kernel: the moments through all levels, then the tangents
    for (size_t l = 0; l + 1 < level.size(); l++) {
      if (level[l + 1] < level[l]) return fail("level offsets decrease");
      std::vector<double> add((size_t) A, 0.0);   // the rows of a level all read the state before it
      for (int r = level[l]; r < level[l + 1]; r++) {
        const int32_t *q = &rows[4 * (size_t) r];
        if (q[0] < 0 || q[0] >= A || q[1] < 0 || q[1] >= A || q[3] < 0 || q[3] >= A) return fail("row outside the image");
        add[(size_t) q[3]] += pass == 0 ? q[2] * M[(size_t) q[0]] * M[(size_t) q[1]]
                                        : q[2] * (G[(size_t) q[0]] * M[(size_t) q[1]] + M[(size_t) q[0]] * G[(size_t) q[1]]);
      }
      for (int k = 0; k < A; k++) (pass == 0 ? M : G)[(size_t) k] += add[(size_t) k];
    }
  double replay = 0.0;
  for (int s = 0; s < S; s++) {
    const int file = pot.alpha_moment_mapping[(size_t) s], lds = smap[(size_t) s];
    if (lds < 0 || lds >= A || (fmap[(size_t) s] != -1 && fmap[(size_t) s] != lds)) return fail("scalar map");
    replay = std::fmax(replay, std::fabs(M[(size_t) lds] - m[(size_t) file]) / std::fmax(1.0, std::fabs(m[(size_t) file])));
    replay = std::fmax(replay, std::fabs(G[(size_t) lds] - g[(size_t) file]) / std::fmax(1.0, std::fabs(g[(size_t) file])));
  }

  // ---- the writer: refusals first (nothing may be written), then new coefficients that must read back bit for bit
  std::vector<double> mo(pot.linear_coeffs), sp(pot.species_coeffs);
  for (double &v : mo) v = v * (1.0 + 0.25 * next()) + 1e-3 * next();
  for (double &v : sp) v += next();
  char msg[512];
  if (mtp_potential_write_coeffs(argv[1], argv[2], sp.data(), mo.data(), Sp, S + 1, msg, sizeof msg) != MTP_ERR_ARG)
    return fail("a wrong moment count was accepted");
  if (mtp_potential_write_coeffs(argv[1], argv[2], sp.data(), mo.data(), Sp + 1, S, msg, 8) != MTP_ERR_ARG)
    return fail("a wrong species count was accepted");
  {
    std::vector<double> bad(mo);
    bad.back() = std::numeric_limits<double>::quiet_NaN();
    if (mtp_potential_write_coeffs(argv[1], argv[2], nullptr, bad.data(), 0, S, msg, sizeof msg) != MTP_ERR_ARG)
      return fail("a NaN was accepted");
  }
  if (FILE *f = std::fopen(argv[2], "rb")) {
    std::fclose(f);
    return fail("a refused call left a file");
  }
  const int rc = mtp_potential_write_coeffs(argv[1], argv[2], sp.data(), mo.data(), Sp, S, msg, sizeof msg);
  if (rc < 0) return fail(msg);
  mtp_potential back;
  if (mtp_parse_text_file(argv[2], false, back, err) != 0) return fail("written file: " + err);
  if (back.linear_coeffs.size() != mo.size() || std::memcmp(back.linear_coeffs.data(), mo.data(), sizeof(double) * mo.size()) != 0 ||
      back.species_coeffs.size() != sp.size() || std::memcmp(back.species_coeffs.data(), sp.data(), sizeof(double) * sp.size()) != 0)
    return fail("coefficients do not read back bit for bit");
  if (back.alpha_index_times != pot.alpha_index_times || back.radial_basis_coeffs != pot.radial_basis_coeffs)
    return fail("another table changed");
  std::printf("OK %d %.3e\n", rc, replay);
  return 0;
}
