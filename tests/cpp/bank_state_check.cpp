// The incremental state of the bank search (csrc/mtp_bank_search.hpp: State) against the from-scratch count (recount),
// without a device and without a potential: tests/test_bank_search_cpu.py builds this with -fsanitize=address,undefined
// and runs it.
//
// The table is hand-made, the smallest on which every rule of the model is live: 8 basics, 16 stored products and 8
// leaves (A = 32); two levels of 64 rows and a leaf block of 64, whole 64-row blocks as pad_levels leaves them.  The
// rows come from a fixed-seed Lcg: squares (a0 == a1), few moments for many rows (one moment read by several rows of a
// 32-row group: broadcast; several rows of a 16-row group on one target: same-address adds) and padding rows of
// multiplicity 0.  Then 20000 random mutations through the state's mutators -- an exchange of a row's factors, a swap
// of two rows inside a 32-row group or across two, a three-cycle, a swap of two numbers inside a class -- and after each
//   the delta returned equals the difference of two from-scratch totals,
//   every per-group add cost equals the recount,
//   undoing the mutation restores every counter (checked on a copy of them, then the mutation is made again).
// Prints one line; exits non-zero at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lammps_mtp_kokkos_amd/csrc/mtp_bank_search.hpp"

using namespace mtp_bank_search;

namespace {

constexpr int B = 8, STORED = 24, A = 32, LEVEL_ROWS = 64, MUTATIONS = 20000;

[[noreturn]] void fail(int step, const char *what, long long got, long long want)
{
  std::printf("bank_state_check: mutation %d: %s: state %lld, recount %lld\n", step, what, got, want);
  std::exit(1);
}

struct Counters {   // every counter of the state
  std::vector<uint8_t> load, readers;
  std::vector<int> add_cost;
  void take(const State &s) { load = s.load, readers = s.readers, add_cost = s.add_cost; }
  bool in(const State &s) const { return load == s.load && readers == s.readers && add_cost == s.add_cost; }
};

}   // namespace

int main()
{
  Lcg next{0x2545F4914F6CDD1Dull};
  auto below = [&](int n) { return (int) (next() % (uint32_t) n); };
  std::vector<MtpRow> rows;
  for (int l = 0; l < 3; l++)
    for (int i = 0; i < LEVEL_ROWS; i++) {
      const bool leaf_block = l == 2;
      // level 1 multiplies basics, level 2 and the leaf block anything stored; targets: stored products or leaves
      const int nfac = l == 0 ? B : STORED;
      const int a3 = leaf_block ? STORED + below(A - STORED) : B + below(STORED - B);
      const int a0 = below(nfac), a1 = i % 8 == 0 ? a0 : below(nfac);   // (every eighth row a square)
      const int mult = 1 + below(3), pad = below(STORED);
      if (i < LEVEL_ROWS - 6)
        rows.push_back(MtpRow{a0, a1, mult, a3});
      else
        rows.push_back(MtpRow{pad, pad, 0, pad});   // padding: multiplicity 0, operands = target, a stored moment
    }
  std::vector<int32_t> perm(A), level_offset = {0, LEVEL_ROWS, 2 * LEVEL_ROWS, 3 * LEVEL_ROWS};
  for (int m = 0; m < A; m++) perm[(size_t) m] = m;
  std::vector<char> leaf(A, 0);
  for (int m = STORED; m < A; m++) leaf[(size_t) m] = 1;
  Table t{rows, perm, level_offset, 2 * LEVEL_ROWS, B, leaf};

  // every rule is live in the table as drawn
  int squares = 0, padding = 0, shared_reads = 0, shared_targets = 0;
  for (size_t r = 0; r < rows.size(); r++) {
    squares += rows[r].mult != 0 && rows[r].a0 == rows[r].a1;
    padding += rows[r].mult == 0;
    for (size_t q = r / 32 * 32; q < r; q++) shared_reads += rows[q].a0 == rows[r].a0;
    for (size_t q = r / 16 * 16; q < r; q++) shared_targets += (int) r < t.leaf_row0 && rows[q].a3 == rows[r].a3;
  }
  if (!squares || !padding || !shared_reads || !shared_targets) {
    std::printf("bank_state_check: the table lacks a case: squares %d, padding %d, shared reads %d, shared targets %d\n", squares,
                padding, shared_reads, shared_targets);
    return 1;
  }

  State s(t);
  Count c = recount(t);
  // (32 numbers on 32 read banks: the reads cost nothing as long as both counts let one address broadcast)
  if (c.same_addr[2] == 0 || c.same_bank[0] == 0 || c.reads != 0) fail(-1, "the start: same-address adds, same-bank adds, reads", c.reads, 0);
  const long long start = c.total();
  int kinds[5] = {0, 0, 0, 0, 0};
  Counters before;
  for (int step = 0; step < MUTATIONS; step++) {
    const int kind = below(5);   // 0 exchange, 1 swap inside a 32-row group, 2 swap across, 3 three-cycle, 4 numbers
    before.take(s);
    const long long total0 = c.total();
    int delta = 0, back = 0;
    if (kind == 4) {
      const int cls = below(3), lo = cls == 0 ? 0 : (cls == 1 ? B : STORED), hi = cls == 0 ? B : (cls == 1 ? STORED : A);
      const int m1 = lo + below(hi - lo), m2 = lo + (m1 - lo + 1 + below(hi - lo - 1)) % (hi - lo);
      const int quoted = s.swap_delta(m1, m2);
      delta = s.swap_numbers(m1, m2);
      if (quoted != delta) fail(step, "swap_delta against swap_numbers", quoted, delta);
      back = s.swap_numbers(m1, m2);
      if (!before.in(s)) fail(step, "counters after a number swap and its undo", 0, 1);
      (void) s.swap_numbers(m1, m2);
    } else {
      const int b = LEVEL_ROWS * below(3);
      int pos[3] = {b + below(LEVEL_ROWS), 0, 0}, np = kind == 0 ? 1 : (kind == 3 ? 3 : 2);
      do {
        if (kind == 1) pos[1] = pos[0] / 32 * 32 + below(32);
        if (kind == 2) pos[1] = ((pos[0] / 32 * 32) ^ 32) + below(32);   // (a level is two 32-row groups)
        if (kind == 3) pos[1] = b + below(LEVEL_ROWS), pos[2] = b + below(LEVEL_ROWS);
      } while (np > 1 && (pos[0] == pos[1] || (np == 3 && (pos[2] == pos[0] || pos[2] == pos[1]))));
      MtpRow was[3], now[3];
      for (int j = 0; j < np; j++) was[j] = rows[(size_t) pos[j]];
      for (int j = 0; j < np; j++) now[j] = was[(j + np - 1) % np];
      if (kind == 0) now[0] = MtpRow{was[0].a1, was[0].a0, was[0].mult, was[0].a3};
      delta = s.place(pos, now, np);
      back = s.place(pos, was, np);
      if (!before.in(s)) fail(step, "counters after a row move and its undo", 0, 1);
      (void) s.place(pos, now, np);
    }
    kinds[kind]++;
    c = recount(t);
    if (delta != c.total() - total0) fail(step, "delta", delta, c.total() - total0);
    if (back != -delta) fail(step, "delta of the undo", back, -delta);
    long long adds = 0;
    for (size_t g = 0; g < c.add_group.size(); g++) {
      if (s.add_cost[g] != c.add_group[g]) fail(step, "add cost of a group", s.add_cost[g], c.add_group[g]);
      adds += s.add_cost[g];
    }
    if (adds != c.adds) fail(step, "adds", adds, c.adds);
  }
  for (int k : kinds)
    if (k < MUTATIONS / 10) fail(MUTATIONS, "mutations of one kind", k, MUTATIONS / 10);
  std::printf("bank_state_check: ok, %d mutations (%d exchanges, %d + %d swaps, %d three-cycles, %d number swaps), model %lld -> %lld\n",
              kinds[0] + kinds[1] + kinds[2] + kinds[3] + kinds[4], kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], start,
              c.total());
  return 0;
}
