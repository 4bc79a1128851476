// Sanitizer driver for the host-only parts of an install into a live context (include/mtp_mi355x.h, "installing ..."): the
// coefficient tables of the native schedule (mtp_build_coeff_tables, mtp_potential_coeff_tables) and the structure gate
// (mtp_check_compatible, mtp_potential_compatible), csrc/mtp_potential.cpp.  Built with -fsanitize=address,undefined by
// `make -C lammps_mtp_kokkos_amd/host san_install`; tests/test_install_cpu.py runs it on the committed and the mutated
// potentials.  No GPU, no HIP runtime.
//
//   test_install_san <potential> <scratch file> [other potential ...]
//       prints "OK <seed_val> <e_lin> <leaf rows> <leaf rows with cf != cb> <rc of compatible per other file ...>" or "ERR <what>"
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

static bool same(const std::vector<double> &a, const std::vector<double> &b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

int main(int argc, char **argv)
{
  if (argc < 3) return 2;
  mtp_potential pot;
  std::string err;
  if (mtp_parse_file(argv[1], false, pot, err) != 0) return fail(err);
  const int S = pot.alpha_scalar_count, Sp = pot.species_count;
  const int nrad = (int) pot.radial_basis_coeffs.size();

  // ---- the tables through the C entry point, sized by its own counts; NULL arrays = the potential's own values
  int32_t counts[6] = {0, 0, 0, 0, 0, 0};
  if (mtp_potential_coeff_tables(&pot, nullptr, nullptr, nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0)
    return fail("counts");
  if (counts[0] != nrad || counts[1] != Sp || counts[2] != (int) pot.seed_val.size() || counts[3] != (int) pot.e_lin.size() ||
      counts[4] != (int) pot.leaf_cf.size() || counts[5] != (int) pot.leaf_cb.size() || counts[2] != (int) pot.seed_idx.size() ||
      counts[3] != (int) pot.e_map.size())
    return fail("inconsistent counts");
  auto tables = [&](const mtp_potential &p, const double *ra, const double *sp, const double *mo, mtp_coeff_tables &t) {
    t.radial.assign((size_t) counts[0], -1.0);
    t.species.assign((size_t) counts[1], -1.0);
    t.seed_val.assign((size_t) counts[2], -1.0);
    t.e_lin.assign((size_t) counts[3], -1.0);
    t.leaf_cf.assign((size_t) counts[4], -1.0);
    t.leaf_cb.assign((size_t) counts[5], -1.0);
    return mtp_potential_coeff_tables(&p, ra, sp, mo, nullptr, t.radial.data(), t.species.data(), t.seed_val.data(), t.e_lin.data(),
                                      t.leaf_cf.data(), t.leaf_cb.data());
  };
  mtp_coeff_tables own;
  if (tables(pot, nullptr, nullptr, nullptr, own) != 0) return fail("own tables");
  if (!same(own.radial, pot.radial_basis_coeffs) || !same(own.species, pot.species_coeffs) || !same(own.seed_val, pot.seed_val) ||
      !same(own.e_lin, pot.e_lin) || !same(own.leaf_cf, pot.leaf_cf) || !same(own.leaf_cb, pot.leaf_cb))
    return fail("the tables of the potential's own values are not the ones finalize built");

  // ---- new values: the tables on the OLD structure against a full load of the written file
  unsigned long long rng = 4711;
  auto next = [&]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double) (rng >> 11) / 9007199254740992.0 - 0.5;
  };
  std::vector<double> ra(pot.radial_basis_coeffs), mo(pot.linear_coeffs), sp(pot.species_coeffs);
  for (double &v : ra) v = v * (1.0 + 0.25 * next()) + 1e-3 * next();
  for (double &v : mo) v = v * (1.0 + 0.25 * next()) + 1e-3 * next();
  for (double &v : sp) v += next();
  char msg[512];
  if (mtp_potential_write_all_coeffs(argv[1], argv[2], ra.data(), sp.data(), mo.data(), nrad, Sp, S, msg, sizeof msg) < 0) return fail(msg);
  mtp_potential back;
  if (mtp_parse_file(argv[2], false, back, err) != 0) return fail("written file: " + err);
  mtp_coeff_tables t_new, t_back;
  if (tables(pot, ra.data(), sp.data(), mo.data(), t_new) != 0 || tables(back, nullptr, nullptr, nullptr, t_back) != 0)
    return fail("tables of the new values");
  if (!same(t_new.radial, t_back.radial) || !same(t_new.species, t_back.species) || !same(t_new.seed_val, t_back.seed_val) ||
      !same(t_new.e_lin, t_back.e_lin) || !same(t_new.leaf_cf, t_back.leaf_cf) || !same(t_new.leaf_cb, t_back.leaf_cb))
    return fail("tables on the old structure differ from a load of the written file");
  // one block at a time: the others keep the potential's values
  mtp_coeff_tables t_mo;
  if (tables(pot, nullptr, nullptr, mo.data(), t_mo) != 0) return fail("moment block alone");
  if (!same(t_mo.radial, pot.radial_basis_coeffs) || !same(t_mo.species, pot.species_coeffs) || !same(t_mo.seed_val, t_new.seed_val) ||
      !same(t_mo.leaf_cf, t_new.leaf_cf))
    return fail("a partial triple mixed its blocks up");
  int differ = 0;
  for (size_t r = 0; r < t_new.leaf_cf.size(); r++) differ += t_new.leaf_cf[r] != t_new.leaf_cb[r];
  // refusals
  for (int which = 0; which < 3; which++) {
    std::vector<double> bad(which == 0 ? ra : (which == 1 ? sp : mo));
    if (bad.empty()) continue;
    bad.back() = which == 1 ? std::numeric_limits<double>::quiet_NaN() : std::numeric_limits<double>::infinity();
    if (mtp_potential_coeff_tables(&pot, which == 0 ? bad.data() : nullptr, which == 1 ? bad.data() : nullptr,
                                   which == 2 ? bad.data() : nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) !=
        MTP_ERR_ARG)
      return fail("a non-finite coefficient was accepted");
  }

  // ---- the structure gate: the file itself, the written file (coefficients only differ), short and absent message buffers
  if (mtp_potential_compatible(&pot, argv[1], 0, msg, sizeof msg) != 0) return fail(std::string("not compatible with itself: ") + msg);
  if (mtp_potential_compatible(&pot, argv[2], 0, msg, 8) != 0) return fail("not compatible with the written file");
  if (mtp_potential_compatible(&pot, argv[2], 0, nullptr, 0) != 0) return fail("null message buffer");
  if (mtp_potential_compatible(&pot, "/nonexistent/file.mtp", 0, msg, sizeof msg) != MTP_ERR_IO) return fail("a missing file");
  if (mtp_potential_compatible(nullptr, argv[1], 0, msg, sizeof msg) != MTP_ERR_ARG) return fail("a null potential");
  std::string rcs;
  for (int k = 3; k < argc; k++) {
    msg[0] = 0;
    const int rc = mtp_potential_compatible(&pot, argv[k], 0, msg, 24);   // (a short buffer: the message is cut, not overrun)
    if (rc != 0 && !msg[0]) return fail("a refusal without a message");
    rcs += " " + std::to_string(rc);
  }
  std::printf("OK %d %d %d %d%s\n", counts[2], counts[3], counts[4], differ, rcs.c_str());
  return 0;
}
