// LDS-bank search of the product rows (host only): the LDS numbering of the moments and the order of the rows inside
// their levels, by a deterministic local search on a model of the cycles the product passes lose to LDS bank collisions.
// Included by mtp_potential.cpp (search_banks, which mtp_potential::finalize calls) and by tests/cpp/bank_state_check.cpp,
// and by nothing else.  The model is stated once, in Model::of_row; the from-scratch count (recount) and the incremental
// state of the rounds (State) are both written against it.
#pragma once

#include "mtp_potential.hpp"   // MtpRow

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace mtp_bank_search {

struct Lcg {   // fixed-seed LCG of the local searches: the schedule is deterministic
  uint64_t state;
  uint32_t operator()() { return (uint32_t) ((state = state * 6364136223846793005ull + 1442695040888963407ull) >> 33); }
};

struct Table {   // what the search works on: it changes the rows and the numbering and reads the rest
  std::vector<MtpRow> &rows;                  // rows_by_level in file numbering, every level in whole 64-row blocks
  std::vector<int32_t> &perm;                 // moment_perm[file index] = LDS number
  const std::vector<int32_t> &level_offset;   // level l: rows [level_offset[l], level_offset[l + 1]); the leaf block is last
  int leaf_row0, B;                           // first row of the leaf block; the basics are the file indices [0, B)
  const std::vector<char> &leaf;              // [file index]: a leaf (they are numbered behind the stored moments)
  int A() const { return (int) perm.size(); }
};

struct Options {
  bool v1;               // the greedy two-move search (the gather-form potentials run it whatever this says)
  int rounds, scale;     // -1: the shipped effort (search)
  bool debug;            // print the model on stderr
  int fwd_block_count;   // head x tail blocks of the basic-moment pass: row per lane or gather form; report line
};

// ---- the model ---------------------------------------------------------------------------------------------------------
// The product passes read M[a0], M[a1], D[a3] (ds_read_b64: the two 32-lane halves of a wave instruction are banked
// separately over 32 eight-byte banks) and add into D[a0], D[a1], M[a3] (ds_add_f64, banked like ds_write_b64: four
// 16-lane groups over 16 eight-byte banks); distinct moments of one group on one bank serialise (MI355X_MICROARCH.md,
// LDS table).  Reads of one address broadcast, adds to one address serialise.  The model: extra cycles per atom.
struct AccessKind {
  int lanes;        // rows of a group, and the banks they spread over
  bool broadcast;   // the rows of a group on one moment count once (reads) or one by one (adds)
  int weight[3];    // cycles per extra access, by stream: a0, a1, a3
};
constexpr AccessKind kRead{32, true, {2, 2, 1}};   // a0, a1 are read in both passes, D[a3] in the reverse one
constexpr AccessKind kAdd{16, false, {1, 1, 1}};
constexpr int kBankSlots = 32;   // counters kept per access (the adds use 16 of them)
inline int pen(int n) { return n > 1 ? n - 1 : 0; }

struct Access {   // the part of one row in one LDS instruction of its lane group
  int id, group, st;   // id: kind x group x stream, the reads before the adds
  const AccessKind *kind;
  int moment;   // file index; its bank: perm[moment] % kind->lanes
};

struct Model {
  int nrows, leaf_row0;
  int accesses() const { return 3 * (nrows / kRead.lanes + nrows / kAdd.lanes); }
  // f(access) for every access row r takes part in.  Leaf rows neither read D[a3] nor add into M[a3].
  template <class F> void of_row(int r, const MtpRow &row, F &&f) const
  {
    const int m3[3] = {row.a0, row.a1, row.a3}, gr = r / kRead.lanes, ga = r / kAdd.lanes;
    for (int st = 0; st < (r >= leaf_row0 ? 2 : 3); st++) {
      f(Access{3 * gr + st, gr, st, &kRead, m3[st]});
      f(Access{3 * (nrows / kRead.lanes + ga) + st, ga, st, &kAdd, m3[st]});
    }
  }
};

// The model counted from scratch: what the reports print and what the state is tested against.
struct Count {
  long long reads = 0, adds = 0;
  std::vector<int> add_group;                                     // add cycles of every 16-row group
  long long same_addr[3] = {0, 0, 0}, same_bank[3] = {0, 0, 0};   // the adds by stream: same / other address on the bank
  long long total() const { return reads + adds; }
};

inline Count recount(const Table &t)
{
  const Model model{(int) t.rows.size(), t.leaf_row0};
  struct Members {
    Access a{0, 0, 0, nullptr, 0};
    int n = 0, nums[kBankSlots];   // the LDS number each row of the group brings
  };
  std::vector<Members> of((size_t) model.accesses());
  for (int r = 0; r < model.nrows; r++)
    model.of_row(r, t.rows[(size_t) r], [&](const Access &a) {
      of[(size_t) a.id].a = a;
      of[(size_t) a.id].nums[of[(size_t) a.id].n++] = t.perm[(size_t) a.moment];
    });
  Count c;
  c.add_group.assign((size_t) (model.nrows / kAdd.lanes), 0);
  for (Members &x : of) {
    if (!x.a.kind) continue;   // (stream a3 of a leaf group)
    std::sort(x.nums, x.nums + x.n);
    int h[kBankSlots] = {0}, repeats = 0, extra = 0;
    for (int i = 0; i < x.n; i++) {
      const bool repeat = i > 0 && x.nums[i] == x.nums[i - 1];
      repeats += repeat;
      if (!repeat || !x.a.kind->broadcast) h[x.nums[i] % x.a.kind->lanes]++;
    }
    for (int b = 0; b < x.a.kind->lanes; b++) extra += pen(h[b]);
    const int cost = x.a.kind->weight[x.a.st] * extra;
    (x.a.kind->broadcast ? c.reads : c.adds) += cost;
    if (x.a.kind->broadcast) continue;
    c.add_group[(size_t) x.a.group] += cost;
    c.same_addr[x.a.st] += repeats;
    c.same_bank[x.a.st] += extra - repeats;
  }
  return c;
}

// The model kept incrementally: a proposal costs a few counter updates per row, or per use of a moment.
struct State {
  Table &t;
  const Model model;
  std::vector<uint8_t> load;      // [access][kBankSlots]: rows (adds) or distinct moments (reads) on each bank
  std::vector<uint8_t> readers;   // [read access][moment]: rows of the group that read the moment
  std::vector<int> add_cost;      // add cycles of every 16-row group: where the row proposals start
  // the index of the number swaps, built through of_row and rebuilt after row moves: per moment its accesses (ascending
  // id) and what it weighs in each (k: 1 if it broadcasts, else its rows); per access what the swap needs of it
  struct Use { int id, k; };
  struct Slot { int lanes, weight, add_group; };   // (add_group: -1 for a read)
  std::vector<std::vector<Use>> uses;   // [moment]
  std::vector<Slot> slot;               // [access]
  bool indexed = false;

  explicit State(Table &t_) : t(t_), model{(int) t_.rows.size(), t_.leaf_row0} { reset(); }
  void reset()   // (after the rows or the numbering changed behind the state's back)
  {
    load.assign((size_t) model.accesses() * kBankSlots, 0);
    readers.assign((size_t) 3 * (model.nrows / kRead.lanes) * t.A(), 0);
    add_cost.assign((size_t) (model.nrows / kAdd.lanes), 0);
    for (int r = 0; r < model.nrows; r++) (void) put(r, +1);
  }
  // row r enters (s = +1) or leaves (s = -1) its accesses; returns the change of the model
  int put(int r, int s)
  {
    // (locals: the byte stores below may alias any member, and the compiler would load each again after every store)
    const Model mdl = model;
    const int A = t.A();
    const int32_t *perm = t.perm.data();
    uint8_t *rd = readers.data(), *ld = load.data();
    int *cost = add_cost.data(), d = 0;
    mdl.of_row(r, t.rows[(size_t) r], [&](const Access &a) {
      if (a.kind->broadcast) {
        uint8_t &c = rd[(size_t) a.id * A + a.moment];
        const bool others = (s > 0 ? c : c - 1) != 0;
        c = (uint8_t) (c + s);
        if (others) return;
      }
      uint8_t &h = ld[(size_t) a.id * kBankSlots + perm[(size_t) a.moment] % a.kind->lanes];
      const int da = a.kind->weight[a.st] * (pen(h + s) - pen(h));
      h = (uint8_t) (h + s);
      if (a.kind == &kAdd) cost[(size_t) a.group] += da;
      d += da;
    });
    indexed = false;
    return d;
  }
  // the rows at pos[0..n) take the contents now[0..n); returns the change of the model
  int place(const int *pos, const MtpRow *now, int n)
  {
    int d = 0;
    for (int i = 0; i < n; i++) d += put(pos[i], -1);
    for (int i = 0; i < n; i++) t.rows[(size_t) pos[i]] = now[i];
    for (int i = 0; i < n; i++) d += put(pos[i], +1);
    return d;
  }
  // moments m1 and m2 (file indices) swap their numbers; both return the change of the model, swap_delta changes nothing
  int swap_delta(int m1, int m2) { return swap<false>(m1, m2); }
  int swap_numbers(int m1, int m2) { return swap<true>(m1, m2); }

private:
  template <bool apply> int swap(int m1, int m2)
  {
    if (!indexed) index_moments();
    const int p1 = t.perm[(size_t) m1], p2 = t.perm[(size_t) m2];
    if (apply) std::swap(t.perm[(size_t) m1], t.perm[(size_t) m2]);
    return move<apply>(m1, p1, p2, m2) + move<apply>(m2, p2, p1, m1);
  }
  void index_moments()
  {
    uses.resize((size_t) t.A());
    for (auto &u : uses) u.clear();
    slot.assign((size_t) model.accesses(), Slot{1, 0, -1});
    for (int r = 0; r < model.nrows; r++)
      model.of_row(r, t.rows[(size_t) r], [&](const Access &a) {
        uses[(size_t) a.moment].push_back({a.id, a.kind->broadcast ? 0 : 1});
        slot[(size_t) a.id] = Slot{a.kind->lanes, a.kind->weight[a.st], a.kind == &kAdd ? a.group : -1};
      });
    for (auto &u : uses) {   // one entry per access: k = 1 + the further rows that count
      std::sort(u.begin(), u.end(), [](const Use &x, const Use &y) { return x.id < y.id; });
      size_t n = 0;
      for (const Use &e : u)
        if (n > 0 && u[n - 1].id == e.id)
          u[n - 1].k += e.k;
        else
          u[n++] = Use{e.id, 1};
      u.resize(n);
    }
    indexed = true;
  }
  int weight_in(int m, int id) const   // 0 if moment m takes no part in the access
  {
    const auto &u = uses[(size_t) m];
    auto it = std::lower_bound(u.begin(), u.end(), id, [](const Use &x, int i) { return x.id < i; });
    return it != u.end() && it->id == id ? it->k : 0;
  }
  // moment m goes from number `from` to number `to`, which `other` leaves for `from`: the change over m's accesses;
  // those that hold both moments are counted once, from the smaller one.  (apply at compile time: the loop that only
  // asks has no stores and keeps its pointers in registers)
  template <bool apply> int move(int m, int from, int to, int other)
  {
    int d = 0;
    for (const Use &e : uses[(size_t) m]) {
      const int k = e.k, k2 = weight_in(other, e.id);
      if (k2 > 0 && m > other) continue;
      const Slot &a = slot[(size_t) e.id];
      const int f = from % a.lanes, g = to % a.lanes;
      if (f == g) continue;
      uint8_t *h = &load[(size_t) e.id * kBankSlots];
      const int da = a.weight * (pen(h[f] - k + k2) + pen(h[g] + k - k2) - pen(h[f]) - pen(h[g]));
      d += da;
      if (!apply) continue;
      h[f] = (uint8_t) (h[f] - k + k2);
      h[g] = (uint8_t) (h[g] + k - k2);
      if (a.add_group >= 0) add_cost[(size_t) a.add_group] += da;
    }
    return d;
  }
};

// ---- the rounds --------------------------------------------------------------------------------------------------------
// The annealed search (v2).  Shipped effort for row-per-lane potentials: 4 rounds x 16 times the proposals; at level 16
// that takes the model from 888 to about 210 extra cycles per atom in half the time v1 needed for 335
// (profiles/bank_search_ab.txt).  Inverse temperatures by Acceptance's scale: a round starts at ANNEAL_K0 plus up to
// ANNEAL_K_STEP (the last round) and ends at ANNEAL_K1; hotter starts lose the greedy order for nothing.
constexpr int BANK_ROUNDS_V2 = 4, BANK_SCALE_V2 = 16;
constexpr int ANNEAL_K0 = 24, ANNEAL_K_STEP = 8, ANNEAL_K1 = 60;
constexpr int ROW_TRIALS_V2 = 200;   // row proposals per row, round and unit of scale ...
constexpr long long ROW_TRIALS_MIN = 200000;   // ... and at least so many a round: small tables cost next to nothing
constexpr long long RENUMBER_TRIALS_MIN = 50000;   // (likewise for the renumbering proposals of a round)

// The acceptance rule of both rounds.  Greedy (v1): only a strict decrease of the model passes.  Annealed (v2): a
// proposal that raises the model by d > 0 cycles passes with probability 2^(-d k / 4); the inverse temperature k rises
// linearly from k0 to k1 over the proposals of a round; proposals that keep the model pass.  Integer arithmetic and the
// caller's Lcg only, so the walk is the same on every host.  A round takes its rule by value: each starts it afresh.
struct Acceptance {
  bool annealed;
  int k0, k1, k = -1;
  uint32_t thr[8] = {0};   // thr[d]: passes if the next 31-bit draw is below it
  void at(long long t, long long trials)
  {
    const int kk = k0 + (int) ((long long) (k1 - k0) * t / std::max(trials, 1ll));
    if (!annealed || kk == k) return;
    k = kk;
    uint64_t qk = 1ull << 32, f = 1ull << 31;
    for (int i = 0; i < k; i++) qk = (qk * 3611622603ull) >> 32;   // 2^(-1/4) in 32 fractional bits
    for (int d = 1; d < 8; d++) thr[d] = (uint32_t) (f = (f * qk) >> 32);
  }
  bool pass(int d, Lcg &next) const { return annealed ? d <= 0 || (d < 8 && next() < thr[d]) : d < 0; }
};

// A round ends on the best array (numbering or rows) it has seen: a copy is taken when a move first leaves the best and
// dropped on return to it; among equals the latest counts, since the other round may find a way on from it.
template <class T> struct BestSeen {
  long long cur = 0, best = 0;   // the model relative to the start of the round
  std::vector<T> saved;          // empty: the live array is the best
  // `live` has just made an accepted move of `delta`, which undo(copy) takes back
  template <class Undo> void moved(const std::vector<T> &live, int delta, Undo &&undo)
  {
    if (delta > 0 && cur == best && saved.empty()) undo(saved = live);
    cur += delta;
    if (cur > best) return;
    best = cur;
    saved.clear();
  }
  void restore(std::vector<T> &live, State &s)
  {
    if (!saved.empty()) live.swap(saved), s.reset();
  }
};

// Search round (a): renumber moments, rows fixed.  Numbers swap inside a class only (cls_members: basics, stored
// products, leaves).
inline void renumber_round(State &s, const std::vector<int> cls_members[3], Lcg &next, long long trials, Acceptance rule)
{
  Table &t = s.t;
  BestSeen<int32_t> best;
  for (long long i = 0; i < trials; i++) {
    rule.at(i, trials);
    // three proposals in four start from a moment some row uses (weighted by use: the often-used moments are the ones
    // that collide), the rest from any moment
    int m1 = (int) (next() % (uint32_t) t.A());
    if ((next() & 3) != 0) {
      const MtpRow &pr = t.rows[next() % (uint32_t) t.rows.size()];
      const uint32_t st = next() % 3u;
      m1 = st == 0 ? pr.a0 : (st == 1 ? pr.a1 : pr.a3);
    }
    const std::vector<int> &cls = cls_members[m1 < t.B ? 0 : (t.leaf[(size_t) m1] ? 2 : 1)];
    if (cls.size() < 2) continue;
    const int m2 = cls[next() % (uint32_t) cls.size()];
    if (m1 == m2) continue;
    const int delta = s.swap_delta(m1, m2);
    if (!rule.pass(delta, next)) continue;
    (void) s.swap_numbers(m1, m2);
    best.moved(t.perm, delta, [&](std::vector<int32_t> &perm) { std::swap(perm[(size_t) m1], perm[(size_t) m2]); });
  }
  best.restore(t.perm, s);
}

// Search round (b): moves of rows inside a level (they commute), numbering fixed.  Two rows of a level may swap places:
// all that v1 proposes (swaps_only).  v2 also lets a row exchange its two factors (the product commutes, and the reverse
// pass adds d3 m0 to D[a1] and d3 m1 to D[a0] either way: the exchange only decides which of the two add instructions,
// and which of the two reads, carries which moment), swaps with an exchange in either row, and rotates three rows over
// three add groups.  A proposal is placed, and put back if the rule refuses its change of the model.
inline void rows_round(State &s, Lcg &next, long long trials, Acceptance rule, bool swaps_only)
{
  Table &t = s.t;
  const int nlev2 = (int) t.level_offset.size() - 1;
  auto exchanged = [](const MtpRow &r) { return MtpRow{r.a1, r.a0, r.mult, r.a3}; };
  BestSeen<MtpRow> best;
  for (long long i = 0; i < trials; i++) {
    rule.at(i, trials);
    const int l = (int) (next() % (uint32_t) nlev2);
    const int b = t.level_offset[(size_t) l], n = t.level_offset[(size_t) l + 1] - b;
    if (n == 0) continue;   // (whole 64-row blocks otherwise)
    // the first row comes from a 16-row group that has a collision (four tries), its partners from anywhere in the level
    int pos[3] = {b + (int) (next() % (uint32_t) n), 0, 0};
    for (int tries = 0; tries < 4 && s.add_cost[(size_t) (pos[0] / 16)] == 0; tries++) pos[0] = b + (int) (next() % (uint32_t) n);
    const uint32_t kind = swaps_only ? 2u : next() % 8u;   // 0-1 exchange, 2-3 swap, 4-5 swap and exchange, 6-7 three-cycle
    MtpRow was[3], now[3];
    int np = 1;
    if (kind < 2) {
      if (t.rows[(size_t) pos[0]].a0 == t.rows[(size_t) pos[0]].a1) continue;   // a square: nothing changes
    } else {
      np = kind < 6 ? 2 : 3;
      for (int j = 1; j < np; j++) pos[j] = b + (int) (next() % (uint32_t) n);
      // rows of one add group (hence of one read group) trade places for nothing
      if (pos[0] / 16 == pos[1] / 16 || (np == 3 && (pos[2] / 16 == pos[0] / 16 || pos[2] / 16 == pos[1] / 16))) continue;
    }
    for (int j = 0; j < np; j++) was[j] = t.rows[(size_t) pos[j]];
    for (int j = 0; j < np; j++) now[j] = was[(j + np - 1) % np];   // (a swap: the other's row; a three-cycle: 2, 0, 1)
    // the exchanges: in the lone row, or with a swap in the row that arrives at pos[0], at pos[1], or in both
    const uint32_t which = kind < 2 ? 1u : (kind == 4 || kind == 5 ? 1u + next() % 3u : 0u);
    if (which & 1u) now[0] = exchanged(now[0]);
    if (which & 2u) now[1] = exchanged(now[1]);
    const int delta = s.place(pos, now, np);
    if (!rule.pass(delta, next)) {
      (void) s.place(pos, was, np);
      continue;
    }
    best.moved(t.rows, delta, [&](std::vector<MtpRow> &rows) {
      for (int j = 0; j < np; j++) rows[(size_t) pos[j]] = was[j];
    });
  }
  best.restore(t.rows, s);
}

// ---- the report (Options::debug) ---------------------------------------------------------------------------------------
// One line of the model, the adds split by stream (a0, a1: reverse pass; a3: forward) and into same-address /
// same-bank shares
inline void report_split(const Count &c, const char *when)
{
  std::fprintf(stderr, "mtp:   %s: reads %lld, adds %lld; adds, same address / other address on the bank: D[a0] %lld / %lld, D[a1] %lld / %lld, M[a3] %lld / %lld\n",
               when, c.reads, c.adds, c.same_addr[0], c.same_bank[0], c.same_addr[1], c.same_bank[1], c.same_addr[2],
               c.same_bank[2]);
}

// The model before and after the search, and the same-address adds that no search can avoid.  A moment used u times in
// a level of G add groups has to share a group u - G times; a factor may sit in either D stream (factor exchange), so
// the two streams count as one of 2 G places.  Neutral padding rows count like any row.
inline void report_banks(const Table &t, const Count &before, const Count &after, int fwd_block_count, int rounds, int scale,
                         bool v1)
{
  std::fprintf(stderr, "mtp: LDS bank model of the product passes: %lld -> %lld extra cycles per atom (reads %lld, adds %lld); "
                       "%d head x tail blocks, %d rounds x %d, search %s\n", before.total(), after.total(), after.reads,
               after.adds, fwd_block_count, rounds, scale, v1 ? "v1" : "v2");
  report_split(after, "after");
  long long forced_d = 0, forced_m = 0;
  std::vector<int> uf((size_t) t.A()), ut((size_t) t.A());
  for (size_t l = 0; l + 1 < t.level_offset.size(); l++) {
    const int b = t.level_offset[l], e = t.level_offset[l + 1], groups = (e - b) / 16;
    std::fill(uf.begin(), uf.end(), 0);
    std::fill(ut.begin(), ut.end(), 0);
    for (int r = b; r < e; r++) {
      uf[(size_t) t.rows[(size_t) r].a0]++;
      uf[(size_t) t.rows[(size_t) r].a1]++;
      if (r < t.leaf_row0) ut[(size_t) t.rows[(size_t) r].a3]++;
    }
    long long fd = 0, fm = 0;
    for (int m = 0; m < t.A(); m++) {
      fd += std::max(0, uf[(size_t) m] - 2 * groups);
      fm += std::max(0, ut[(size_t) m] - groups);
    }
    std::fprintf(stderr, "mtp:   forced same-address adds, %s %d (%d add groups): D[a0] + D[a1] %lld, M[a3] %lld\n",
                 b >= t.leaf_row0 ? "leaf block" : "level", (int) l + 1, groups, fd, fm);
    forced_d += fd;
    forced_m += fm;
  }
  std::fprintf(stderr, "mtp:   forced same-address adds in all: D[a0] + D[a1] %lld, M[a3] %lld\n", forced_d, forced_m);
}

// ---- the search --------------------------------------------------------------------------------------------------------
// The moments are renumbered -- basics among [0, B), stored products and leaves among their own numbers, so the
// zero-fill and the k < B loops of the kernel keep working -- in rounds that alternate with moves of rows inside a level.
// v2 (the default for row-per-lane potentials) anneals both and ends each on the best state it saw; v1 (Options::v1, and
// the gather-form potentials) lets only proposals pass that lower the model, and its row round only swaps two rows.
inline void search(Table &t, const Options &opt)
{
  assert(t.rows.size() % 64 == 0 && t.A() >= 2);
  std::vector<int> cls_members[3];   // 0 basics, 1 stored products, 2 leaves (file indices)
  for (int m = 0; m < t.A(); m++) cls_members[m < t.B ? 0 : (t.leaf[(size_t) m] ? 2 : 1)].push_back(m);
  State state(t);
  const Count before = recount(t);
  if (opt.debug) report_split(before, "before");
  // Search effort.  Potentials whose product passes run row per lane (the narrow lane grids: up to level 16) pay every
  // modelled collision in ds_add_f64 cycles, the busiest pipe of their kernel.  v1 ran eight rounds of four times the
  // proposals for them (16 s at level 16 on the development host, once per potential load; model 888 -> 335 extra cycles
  // per atom).  v2 runs BANK_ROUNDS_V2 x BANK_SCALE_V2 (see there).  The wide grids run the gather programs, which have
  // their own refinement (refine_program): two rounds of v1, whose model the kernel does not follow for them.
  // MTP_BANK_ROUNDS / MTP_BANK_SCALE (Options::rounds, scale) override; tests use two rounds.  (row per lane <=> at most
  // 32 head x tail blocks in the basic-moment pass, mtp_pick_fwd_shape)
  const bool row_per_lane = opt.fwd_block_count <= 32;
  const bool v1 = opt.v1 || !row_per_lane;
  const int rounds = opt.rounds >= 0 ? opt.rounds : (!row_per_lane ? 2 : (v1 ? 8 : BANK_ROUNDS_V2));
  const int scale = opt.scale >= 1 ? opt.scale : (!row_per_lane ? 1 : (v1 ? 4 : BANK_SCALE_V2));
  const long long nrows = (long long) t.rows.size();
  long long renumber_trials = scale * std::min<long long>(200ll * t.A(), 300000ll);
  long long row_trials = scale * std::min<long long>(100ll * nrows, 250000ll);
  if (!v1) {
    renumber_trials = std::max(renumber_trials, RENUMBER_TRIALS_MIN);
    row_trials = std::max(scale * ROW_TRIALS_V2 * nrows, ROW_TRIALS_MIN);
  }
  Lcg next{0x9E3779B97F4A7C15ull};
  for (int round = 0; round < rounds; round++) {
    // every annealed round reheats, later rounds less: the first one leaves the greedy order of order_rows behind, the
    // last ones only polish
    const Acceptance rule{!v1, ANNEAL_K0 + ANNEAL_K_STEP * round / std::max(rounds - 1, 1), ANNEAL_K1};
    renumber_round(state, cls_members, next, renumber_trials, rule);
    rows_round(state, next, row_trials, rule, v1);
  }
  if (opt.debug) report_banks(t, before, recount(t), opt.fwd_block_count, rounds, scale, v1);
}

}   // namespace mtp_bank_search
