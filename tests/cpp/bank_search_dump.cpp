// What the bank search of the schedule builder (csrc/mtp_bank_search.hpp, search) leaves behind, printed without a
// device: tests/test_bank_search_cpu.py builds this from mtp_potential.cpp + mtp_plan.cpp alone (once more with
// -fsanitize=address,undefined) and reads the lines.  The search itself is steered by the environment (MTP_BANK_SEARCH,
// MTP_BANK_ROUNDS, MTP_BANK_SCALE, MTP_DEBUG_BANKS), as in the library.
//
//   bank_search_dump FILE [want_selection 0|1]
//
// prints
//   counts A B stored normal_levels seconds      (seconds: wall time of the load, parse and finalize)
//   hash   64-bit FNV-1a of rows_by_level, level_offset and moment_perm (each: its length, then its bytes)
//   level_offset ...
//   perm ...                                     moment_perm[file index] = LDS number
//   rows a0 a1 mult a3 ...                       rows_by_level, LDS numbering, padding rows included
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../lammps_mtp_kokkos_amd/csrc/mtp_potential.hpp"

int main(int argc, char **argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: bank_search_dump FILE [want_selection]\n");
    return 2;
  }
  mtp_potential pot;
  std::string err;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = mtp_parse_file(argv[1], argc > 2 && std::atoi(argv[2]) != 0, pot, err);
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (rc != 0) {
    std::fprintf(stderr, "bank_search_dump: %s: %s\n", argv[1], err.c_str());
    return 1;
  }
  uint64_t digest = 14695981039346656037ull;
  auto hash_bytes = [&](const void *p, size_t n) {
    for (size_t i = 0; i < n; i++) digest = (digest ^ ((const unsigned char *) p)[i]) * 1099511628211ull;
  };
  auto hash_vec = [&](const auto &v) {
    const uint64_t n = v.size();
    hash_bytes(&n, sizeof n);
    hash_bytes(v.data(), v.size() * sizeof(v[0]));
  };
  hash_vec(pot.rows_by_level);
  hash_vec(pot.level_offset);
  hash_vec(pot.moment_perm);
  std::printf("counts %d %d %d %d %.3f\n", pot.alpha_moment_count, pot.alpha_index_basic_count, pot.stored_moment_count,
              pot.normal_levels, seconds);
  std::printf("hash %016llx\n", (unsigned long long) digest);
  std::printf("level_offset");
  for (int v : pot.level_offset) std::printf(" %d", v);
  std::printf("\nperm");
  for (int v : pot.moment_perm) std::printf(" %d", v);
  std::printf("\nrows");
  for (const MtpRow &r : pot.rows_by_level) std::printf(" %d %d %d %d", (int) r.a0, (int) r.a1, (int) r.mult, (int) r.a3);
  std::printf("\n");
  return 0;
}
