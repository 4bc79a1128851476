// MLIP-3 potential file reader and native schedule builder (host only).
//
// Grammar and error behaviour follow PairMTP::read_file
// (/root/reference/LAMMPS/ML-MTP/pair_mtp.cpp:335-570), RadialMTPBasis::ReadBasisProperties
// (mtp_radial_basis.cpp:59-102) and PairMTPExtrapolation::read_file
// (pair_mtp_extrapolation.cpp:528-612); SURVEY.md App. A is the condensed grammar.
#include "mtp_potential.hpp"
#include "mtp_bank_search.hpp"

#include "../../include/mtp_mi355x.h"

#include <algorithm>
#include <cassert>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include <unistd.h>

namespace {

struct ParseError {
  int code;
  std::string msg;
};

// LAMMPS TextFileReader semantics the reference depends on: fgets into a buffer whose
// size the caller may change (pair_mtp.cpp:489-492, 525-528), '#' starts a comment when
// ignore_comments is set, lines without words are skipped.
class LineReader {
 public:
  explicit LineReader(FILE *fp) : fp_(fp), buf_(1024) {}
  bool ignore_comments = true;
  void set_bufsize(size_t n) { buf_.assign(std::max<size_t>(n, 2), '\0'); }
  // returns false at end of file
  bool next(std::string &out)
  {
    while (fgets(buf_.data(), (int) buf_.size(), fp_)) {
      out.assign(buf_.data());
      if (ignore_comments) {
        auto p = out.find('#');
        if (p != std::string::npos) out.erase(p);
      }
      if (out.find_first_not_of(" \t\r\n\f") != std::string::npos) return true;
    }
    return false;
  }

 private:
  FILE *fp_;
  std::vector<char> buf_;
};

// ValueTokenizer: split on a separator set; typed getters fail loudly.
class Tokens {
 public:
  Tokens() = default;
  Tokens(const std::string &line, const char *seps) : s_(line), seps_(seps) {}
  bool next(std::string &w)
  {
    size_t b = s_.find_first_not_of(seps_, pos_);
    if (b == std::string::npos) return false;
    size_t e = s_.find_first_of(seps_, b);
    if (e == std::string::npos) e = s_.size();
    w = s_.substr(b, e - b);
    pos_ = e;
    return true;
  }
  std::string word()
  {
    std::string w;
    if (!next(w)) throw ParseError{MTP_ERR_PARSE, "Not enough tokens"};
    return w;
  }
  int integer()
  {
    std::string w = word();
    char *e = nullptr;
    errno = 0;
    long v = std::strtol(w.c_str(), &e, 10);
    if (*e || errno) throw ParseError{MTP_ERR_PARSE, "Not a valid integer number: '" + w + "'"};
    return (int) v;
  }
  double real()
  {
    std::string w = word();
    char *e = nullptr;
    double v = std::strtod(w.c_str(), &e);
    if (*e) throw ParseError{MTP_ERR_PARSE, "Not a valid floating-point number: '" + w + "'"};
    return v;
  }

 private:
  std::string s_;
  std::string seps_;
  size_t pos_ = 0;
};

const char *kSeps = " \t\r\n\f=, ";
const char *kSepsDash = " \t\r\n\f=, -";
const char *kSepsBrace = " \t\r\n\f=, {},";

struct Cursor {
  LineReader &rd;
  std::string line, key;
  Tokens tok;
  void advance(const char *seps)
  {
    if (!rd.next(line)) throw ParseError{MTP_ERR_EOF, "Unexpected end of MTP file."};
    tok = Tokens(line, seps);
    if (!tok.next(key)) key.clear();
  }
  void expect(const char *kw, const char *msg)
  {
    if (key != kw) throw ParseError{MTP_ERR_PARSE, msg};
  }
};

void parse_text(FILE *fp, bool want_selection, mtp_potential &p)
{
  LineReader rd(fp);
  Cursor c{rd, {}, {}, {}};

  c.advance(kSeps);
  if (c.key != "MTP") throw ParseError{MTP_ERR_FORMAT, "Only MTP potential files are accepted."};
  {
    std::string ver;
    if (!rd.next(ver) || ver != "version = 1.1.0\n")   // exact, newline included (:357)
      throw ParseError{MTP_ERR_FORMAT, "MTP file must have version \"1.1.0\""};
  }
  c.advance(kSeps);
  if (c.key == "potential_name") {
    std::string w;
    p.potential_name = c.tok.next(w) ? w : "";
    c.advance(kSeps);
  }
  p.scaling = 1.0;
  if (c.key == "scaling") {
    p.scaling = c.tok.real();
    c.advance(kSeps);
  }
  c.expect("species_count", "Error reading MTP file. Species count not found.");
  p.species_count = c.tok.integer();
  if (p.species_count < 1) throw ParseError{MTP_ERR_PARSE, "species_count must be positive"};

  c.advance(kSeps);
  if (c.key == "potential_tag") {
    std::string w;
    p.potential_tag = c.tok.next(w) ? w : "";
    c.advance(kSeps);
  }
  c.expect("radial_basis_type", "Error reading MTP file. No radial basis set type is specified.");
  {
    std::string ty = c.tok.word();
    if (ty != "RBChebyshev")
      throw ParseError{MTP_ERR_UNSUPPORTED,
                       "Error reading MTP file. The specified radial basis set type, " + ty + ", was not found.."};
  }
  // radial basis block (mtp_radial_basis.cpp:59-102)
  c.advance(kSeps);
  if (c.key == "scaling") {   // parsed, then superseded by the top-level value (pair_mtp.cpp:416)
    (void) c.tok.real();
    c.advance(kSeps);
  }
  if (c.key != "min_val" && c.key != "min_dist")
    throw ParseError{MTP_ERR_PARSE, "Error in reading MTP file. Cannot read lower cutoff."};
  p.min_cutoff = c.tok.real();
  c.advance(kSeps);
  if (c.key != "max_val" && c.key != "max_dist")
    throw ParseError{MTP_ERR_PARSE, "Error in reading MTP file. Cannot read upper cutoff."};
  p.max_cutoff = c.tok.real();
  c.advance(kSeps);
  c.expect("radial_basis_size", "Error in reading MTP file. Cannot read radial basis set size.");
  p.radial_basis_size = c.tok.integer();

  c.advance(kSeps);
  c.expect("radial_funcs_count", "Error in reading MTP file. Cannot read radial function count.");
  p.radial_func_count = c.tok.integer();
  c.advance(kSeps);
  if (c.key != "radial_coeffs") {
    if (c.key == "magnetic_basis_type")
      throw ParseError{MTP_ERR_UNSUPPORTED, "Magnetic basis is currently not supported."};
    throw ParseError{MTP_ERR_PARSE, "Error in reading MTP file. Cannot read radial coeffs count."};
  }
  const int Sp = p.species_count, R = p.radial_basis_size, Mu = p.radial_func_count;
  if (R < 1 || Mu < 1) throw ParseError{MTP_ERR_PARSE, "radial basis sizes must be positive"};
  p.radial_basis_coeffs.assign((size_t) Sp * Sp * Mu * R, 0.0);
  p.setflag.assign((size_t) (Sp + 1) * (Sp + 1), 0);
  for (int blk = 0; blk < Sp * Sp; blk++) {   // any order, 0-based species (:450-469)
    if (!rd.next(c.line)) throw ParseError{MTP_ERR_EOF, "Unexpected end of MTP file."};
    Tokens hdr(c.line, kSepsDash);
    int t1 = hdr.integer(), t2 = hdr.integer();
    if (t1 < 0 || t2 < 0 || t1 >= Sp || t2 >= Sp)
      throw ParseError{MTP_ERR_PARSE, "radial_coeffs block names a species outside species_count"};
    p.setflag[(size_t) (t1 + 1) * (Sp + 1) + t2 + 1] = 1;
    double *dst = &p.radial_basis_coeffs[(size_t) (t1 * Sp + t2) * Mu * R];
    for (int mu = 0; mu < Mu; mu++) {
      if (!rd.next(c.line)) throw ParseError{MTP_ERR_EOF, "Unexpected end of MTP file."};
      Tokens row(c.line, kSepsBrace);
      for (int ri = 0; ri < R; ri++) dst[mu * R + ri] = row.real();
    }
  }
  c.advance(kSeps);
  c.expect("alpha_moments_count", "Error reading MTP file. Alpha moment count not found.");
  p.alpha_moment_count = c.tok.integer();
  c.advance(kSeps);
  c.expect("alpha_index_basic_count", "Error reading MTP file. Alpha moment count not found.");
  p.alpha_index_basic_count = c.tok.integer();
  const int B = p.alpha_index_basic_count;
  if (B < 1) throw ParseError{MTP_ERR_TABLE, "alpha_index_basic_count must be positive"};

  rd.set_bufsize((size_t) B * 20 + 20);
  c.advance(kSepsBrace);
  c.expect("alpha_index_basic", "Error reading MTP file. Alpha index basic not found.");
  p.alpha_index_basic.resize((size_t) B * 4);
  int mu_max = 0, rank_max = 0;
  for (int i = 0; i < B; i++) {
    int32_t *q = &p.alpha_index_basic[4 * (size_t) i];
    for (int j = 0; j < 4; j++) q[j] = c.tok.integer();
    mu_max = std::max(mu_max, (int) q[0]);
    rank_max = std::max(rank_max, (int) (q[1] + q[2] + q[3]));
  }
  if (mu_max != Mu - 1) throw ParseError{MTP_ERR_TABLE, "Wrong number of radial functions specified!"};
  p.max_alpha_index_basic = rank_max + 1;

  c.advance(kSeps);
  c.expect("alpha_index_times_count", "Error reading MTP file. Alpha index times count not found.");
  p.alpha_index_times_count = c.tok.integer();
  const int T = p.alpha_index_times_count;
  rd.set_bufsize((size_t) std::max(T, 0) * 32 + 20);
  c.advance(kSepsBrace);
  c.expect("alpha_index_times", "Error reading MTP file. Alpha index times not found.");
  p.alpha_index_times.resize((size_t) std::max(T, 0) * 4);
  for (size_t i = 0; i < p.alpha_index_times.size(); i++) p.alpha_index_times[i] = c.tok.integer();

  c.advance(kSeps);
  c.expect("alpha_scalar_moments", "Error reading MTP file. Alpha scalar moment count not found.");
  p.alpha_scalar_count = c.tok.integer();
  const int S = p.alpha_scalar_count;
  c.advance(kSepsBrace);
  c.expect("alpha_moment_mapping", "Error reading MTP file. Alpha moment mappings not found.");
  p.alpha_moment_mapping.resize((size_t) S);
  for (int i = 0; i < S; i++) p.alpha_moment_mapping[i] = c.tok.integer();
  c.advance(kSepsBrace);
  c.expect("species_coeffs", "Error reading MTP file. Species coefficients not found.");
  p.species_coeffs.resize((size_t) Sp);
  for (int i = 0; i < Sp; i++) p.species_coeffs[i] = c.tok.real();
  c.advance(kSepsBrace);
  c.expect("moment_coeffs", "Error reading MTP file. Moment coefficients not found.");
  p.linear_coeffs.resize((size_t) S);
  for (int i = 0; i < S; i++) p.linear_coeffs[i] = c.tok.real();

  p.coeff_count = Sp * Sp * Mu * R + Sp + S;

  if (!want_selection) return;
  // selection state (pair_mtp_extrapolation.cpp:545-612)
  rd.ignore_comments = false;
  std::string ln;
  if (!rd.next(ln)) {
    p.selection_absent = true;
    throw ParseError{MTP_ERR_SELECTION,
                     "No selection state found! Consider training/retraining or disabling extrapolation!"};
  }
  {
    Tokens t(ln, kSeps);
    std::string w;
    if (!t.next(w) || w != "#MVS_v1.1")
      throw ParseError{MTP_ERR_SELECTION,
                       "Error in reading MTP file selection state. Please verify MVS version is #MVS_v1.1!"};
  }
  rd.ignore_comments = true;
  int energy_weight = 0, site_en_weight = 0;
  static const char *names[5] = {"energy_weight", "force_weight", "stress_weight", "site_en_weight",
                                 "weight_scaling"};
  for (int w = 0; w < 5; w++) {
    c.advance(kSeps);
    if (c.key != names[w])
      throw ParseError{MTP_ERR_SELECTION, std::string("Error in reading MTP file, ") + names[w]};
    if (w == 0) energy_weight = (int) c.tok.real();
    if (w == 3) site_en_weight = (int) c.tok.real();
  }
  if (energy_weight + site_en_weight > 1)
    throw ParseError{MTP_ERR_MODE,
                     "Error, the MTP currently only supports configuration mode (energy_weight=1) or "
                     "neighbourhood mode (site_en_weight=1). Please retrain the MTP with the correct modes!"};
  p.configuration_mode = (energy_weight == 1);
  const size_t n = (size_t) p.coeff_count * p.coeff_count;
  p.active_set.resize(n);
  p.inverse_active_set.resize(n);
  fgetc(fp);   // the '#' in front of the raw fp64 block (:607)
  p.selection_offset = std::ftell(fp);
  if (fread(p.active_set.data(), sizeof(double), n, fp) != n ||
      fread(p.inverse_active_set.data(), sizeof(double), n, fp) != n)
    throw ParseError{MTP_ERR_IO, "Unexpected end of file while reading the active set"};
  p.has_selection = true;
}

}   // namespace

int mtp_parse_file(const char *path, bool want_selection, mtp_potential &pot, std::string &err)
{
  const int rc = mtp_parse_text_file(path, want_selection, pot, err);
  return rc == MTP_OK ? pot.finalize(err) : rc;
}

int mtp_parse_text_file(const char *path, bool want_selection, mtp_potential &pot, std::string &err)
{
  FILE *fp = std::fopen(path, "rb");
  if (!fp) {
    err = std::string("Cannot open potential file ") + path + ": " + std::strerror(errno);
    return MTP_ERR_IO;
  }
  int rc = MTP_OK;
  try {
    parse_text(fp, want_selection, pot);
  } catch (const ParseError &e) {
    err = e.msg;
    rc = e.code;
  } catch (const std::exception &e) {
    err = e.what();
    rc = MTP_ERR_PARSE;
  }
  std::fclose(fp);
  return rc;
}

// ---- the coefficient-dependent tables of the schedule (mtp_potential.hpp) ---------------------------------------------
// Reads the structure only as relabel leaves it: rows_by_level in LDS numbering, level_offset / normal_levels,
// moment_perm and stored_moment_count (a moment is a leaf iff its LDS number is not below stored_moment_count).
void mtp_build_coeff_tables(const mtp_potential &p, const double *radial, const double *species, const double *moments,
                            mtp_coeff_tables &out)
{
  const int A = p.alpha_moment_count, S = p.alpha_scalar_count;
  const std::vector<int32_t> &perm = p.moment_perm;
  const double *lin = moments ? moments : p.linear_coeffs.data();
  const double *ra = radial ? radial : p.radial_basis_coeffs.data();
  const double *sp = species ? species : p.species_coeffs.data();
  out.radial.assign(ra, ra + p.radial_basis_coeffs.size());
  out.species.assign(sp, sp + p.species_coeffs.size());
  auto is_leaf = [&](int m) { return perm[(size_t) m] >= p.stored_moment_count; };
  // adjoint seeds: assignment, so the last scalar mapped to a moment wins (:217-218)
  std::vector<int> last((size_t) A, -1);
  for (int i = 0; i < S; i++) last[(size_t) p.alpha_moment_mapping[(size_t) i]] = i;
  out.seed_val.clear();
  for (int m = 0; m < A; m++)
    if (last[(size_t) m] >= 0 && !is_leaf(m)) out.seed_val.push_back(lin[last[(size_t) m]]);
  // constants of the leaf rows and the energy table of the stored scalars
  std::vector<double> c_energy((size_t) A, 0.0), c_seed((size_t) A, 0.0);   // by LDS number
  out.e_lin.clear();
  for (int i = 0; i < S; i++) {
    const int m = p.alpha_moment_mapping[(size_t) i], ml = perm[(size_t) m];
    if (is_leaf(m)) {
      c_energy[(size_t) ml] += lin[i];
      c_seed[(size_t) ml] = lin[i];   // the last one wins (:217-218)
    } else {
      out.e_lin.push_back(lin[i]);
    }
  }
  const size_t leaf_row0 = (size_t) p.level_offset[(size_t) p.normal_levels];
  const size_t nleaf_rows = p.rows_by_level.size() - leaf_row0;
  out.leaf_cf.assign(nleaf_rows, 0.0);
  out.leaf_cb.assign(nleaf_rows, 0.0);
  for (size_t r = 0; r < nleaf_rows; r++) {
    const MtpRow &row = p.rows_by_level[leaf_row0 + r];
    if (row.mult == 0) continue;   // padding
    out.leaf_cf[r] = c_energy[(size_t) row.a3] * row.mult;
    out.leaf_cb[r] = c_seed[(size_t) row.a3] * row.mult;
  }
}

// first difference between `a` and another potential "as read" in what the schedule and the argument block depend on
int mtp_check_compatible(const mtp_potential &a, const mtp_potential &b, bool want_selection, std::string &err)
{
  auto differ = [&](const std::string &name, const std::string &x, const std::string &y) {
    err = "the new file differs in " + name + ": " + y + ", the loaded potential has " + x;
    return (int) MTP_ERR_UNSUPPORTED;
  };
  auto num = [](double v) {
    char t[40];
    std::snprintf(t, sizeof t, "%.17g", v);
    return std::string(t);
  };
#define MTP_SAME_INT(field, name) \
  if (a.field != b.field) return differ(name, std::to_string(a.field), std::to_string(b.field))
#define MTP_SAME_REAL(field, name) \
  if (!(a.field == b.field)) return differ(name, num(a.field), num(b.field))
  MTP_SAME_REAL(scaling, "scaling");
  MTP_SAME_INT(species_count, "species_count");
  MTP_SAME_REAL(min_cutoff, "min_dist");
  MTP_SAME_REAL(max_cutoff, "max_dist");
  MTP_SAME_INT(radial_basis_size, "radial_basis_size");
  MTP_SAME_INT(radial_func_count, "radial_funcs_count");
  MTP_SAME_INT(alpha_moment_count, "alpha_moments_count");
  MTP_SAME_INT(alpha_index_basic_count, "alpha_index_basic_count");
  MTP_SAME_INT(alpha_index_times_count, "alpha_index_times_count");
  MTP_SAME_INT(alpha_scalar_count, "alpha_scalar_moments");
#undef MTP_SAME_INT
#undef MTP_SAME_REAL
  auto table = [&](const char *name, const std::vector<int32_t> &x, const std::vector<int32_t> &y, size_t width) {
    if (x.size() != y.size()) return differ(name, std::to_string(x.size()) + " entries", std::to_string(y.size()) + " entries");
    for (size_t k = 0; k < x.size(); k++)
      if (x[k] != y[k])
        return differ(std::string(name) + "[" + std::to_string(k / width) + (width > 1 ? "][" + std::to_string(k % width) + "]" : "]"),
                      std::to_string(x[k]), std::to_string(y[k]));
    return (int) MTP_OK;
  };
  int rc = table("alpha_index_basic", a.alpha_index_basic, b.alpha_index_basic, 4);
  if (rc == MTP_OK) rc = table("alpha_index_times", a.alpha_index_times, b.alpha_index_times, 4);
  if (rc == MTP_OK) rc = table("alpha_moment_mapping", a.alpha_moment_mapping, b.alpha_moment_mapping, 1);
  if (rc != MTP_OK) return rc;
  if (want_selection) {
    const char *modes[2] = {"neighbourhood (site_en_weight = 1)", "configuration (energy_weight = 1)"};
    if (a.coeff_count != b.coeff_count) return differ("coeff_count", std::to_string(a.coeff_count), std::to_string(b.coeff_count));
    if (a.has_selection != b.has_selection)
      return differ("selection state", a.has_selection ? "present" : "absent", b.has_selection ? "present" : "absent");
    if (a.configuration_mode != b.configuration_mode)
      return differ("selection mode", modes[a.configuration_mode ? 1 : 0], modes[b.configuration_mode ? 1 : 0]);
  }
  return MTP_OK;
}

// ---- native schedule: the passes of mtp_potential::finalize, in the order it runs them -----------------------------
namespace {

// Load-time switches of the schedule builder, read once per finalize; -1 = decided from the number of
// head x tail blocks
struct ScheduleOptions {
  bool leaves, renumber, debug_banks;   // MTP_NO_LEAF and MTP_NO_RENUMBER unset, MTP_DEBUG_BANKS set
  bool search_v1;                       // MTP_BANK_SEARCH=v1: the greedy two-move search (search_banks)
  int bank_rounds = -1, bank_scale = -1, refine_programs = -1;   // MTP_BANK_ROUNDS, MTP_BANK_SCALE, MTP_REFINE_PROGRAMS
};

ScheduleOptions read_options()
{
  ScheduleOptions o;
  o.leaves = !std::getenv("MTP_NO_LEAF");
  o.renumber = !std::getenv("MTP_NO_RENUMBER");
  o.debug_banks = std::getenv("MTP_DEBUG_BANKS") != nullptr;
  const char *search = std::getenv("MTP_BANK_SEARCH");
  o.search_v1 = search && std::strcmp(search, "v1") == 0;
  if (const char *e = std::getenv("MTP_BANK_ROUNDS")) o.bank_rounds = std::max(0, std::atoi(e));
  if (const char *e = std::getenv("MTP_BANK_SCALE")) o.bank_scale = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("MTP_REFINE_PROGRAMS")) o.refine_programs = std::atoi(e) != 0;
  return o;
}

int refuse(std::string &err, int code, const char *msg)
{
  err = msg;
  return code;
}

// Every input check, ahead of any schedule work; a file with several faults gets the error of the first one in this
// order.  The slot and coefficient-block limits and the duplicate basics follow in build_slots.
int validate(const mtp_potential &p, std::string &err)
{
  const int A = p.alpha_moment_count, B = p.alpha_index_basic_count, T = p.alpha_index_times_count;
  if (A < B) return refuse(err, MTP_ERR_TABLE, "alpha_moments_count is smaller than alpha_index_basic_count");
  for (int i = 0; i < B; i++) {
    const int32_t *q = &p.alpha_index_basic[4 * (size_t) i];
    if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0)
      return refuse(err, MTP_ERR_TABLE, "negative entry in alpha_index_basic");
    if (q[1] > 15 || q[2] > 15 || q[3] > 15)
      return refuse(err, MTP_ERR_LIMIT, "alpha_index_basic exponent above 15 is not supported");
  }
  if (p.max_alpha_index_basic > 12)
    return refuse(err, MTP_ERR_LIMIT, "tensor rank above 11 is not supported by this build");
  for (int k = 0; k < T; k++) {
    const int32_t *q = &p.alpha_index_times[4 * (size_t) k];
    for (int j : {0, 1, 3})
      if (q[j] < 0 || q[j] >= A)
        return refuse(err, MTP_ERR_TABLE, "alpha_index_times refers to a moment outside alpha_moments_count");
  }
  for (int m : p.alpha_moment_mapping)
    if (m < 0 || m >= A)
      return refuse(err, MTP_ERR_TABLE, "alpha_moment_mapping refers to a moment outside alpha_moments_count");
  for (int i = 0; i < B; i++)
    if (p.alpha_index_basic[4 * (size_t) i] > 15)
      return refuse(err, MTP_ERR_LIMIT, "radial function index above 15 is not supported");
  return MTP_OK;
}

// Radial slots = distinct (mu, nu) of the basics, numbered by tensor rank nu, then mu; the packed basic descriptors and
// the coefficient targets per basic, in file numbering (relabel moves basic_tgt to LDS numbering).
int build_slots(mtp_potential &p, std::string &err)
{
  const int B = p.alpha_index_basic_count, P = p.max_alpha_index_basic, Mu = p.radial_func_count;
  p.slot_of.assign((size_t) Mu * P, -1);
  for (int i = 0; i < B; i++) {
    const int32_t *q = &p.alpha_index_basic[4 * (size_t) i];
    p.slot_of[(size_t) q[0] * P + (q[1] + q[2] + q[3])] = -2;   // used, not yet numbered
  }
  p.slot_count = 0;
  p.slot_coef_off.clear();
  p.slot_mu.clear();
  p.coef_total = 0;
  for (int nu = 0; nu < 14; nu++) {
    p.deg_first[nu] = p.slot_count;
    p.deg_coef[nu] = p.coef_total;
    if (nu >= P) continue;
    for (int mu = 0; mu < Mu; mu++)
      if (p.slot_of[(size_t) mu * P + nu] == -2) {
        p.slot_of[(size_t) mu * P + nu] = p.slot_count++;
        p.slot_coef_off.push_back(p.coef_total);
        p.slot_mu.push_back(mu);
        p.coef_total += nu == 0 ? 1 : 3 * (nu * (nu + 1) / 2);
      }
  }
  if (p.slot_count > 256) return refuse(err, MTP_ERR_LIMIT, "more than 256 distinct (mu, nu) radial slots");
  p.basic_pack.resize((size_t) B);
  for (int i = 0; i < B; i++) {
    const int32_t *q = &p.alpha_index_basic[4 * (size_t) i];
    const int s = p.slot_of[(size_t) q[0] * P + (q[1] + q[2] + q[3])];
    p.basic_pack[i] = s | (q[1] << 8) | (q[2] << 12) | (q[3] << 16) | (q[0] << 20);
  }
  // where each basic's adjoint goes in the derivative-polynomial coefficient blocks: basic (s; a, b, c)
  // contributes a*D to the d/dx coefficient of x^(a-1) y^b z^c, b*D and c*D alike (monomials of degree
  // nu-1 ordered a descending, then b descending: index j(j+1)/2 + c with j = b + c); rank 0: D itself
  if (p.coef_total > 65534)
    return refuse(err, MTP_ERR_LIMIT,
                  "derivative-polynomial coefficient blocks above 65534 entries are not supported by this build");
  p.basic_tgt.assign((size_t) 2 * B, 0);
  std::vector<int> hits((size_t) p.coef_total, 0);
  for (int i = 0; i < B; i++) {
    const int32_t *q = &p.alpha_index_basic[4 * (size_t) i];
    const int a = q[1], b = q[2], c = q[3], j = b + c, nu = a + j, C = nu * (nu + 1) / 2;
    const int base = p.slot_coef_off[(size_t) (p.basic_pack[i] & 255)];
    uint32_t tx = 0xffffu, ty = 0xffffu, tz = 0xffffu, fa = (uint32_t) a;
    if (nu == 0) {
      tx = (uint32_t) base;
      fa = 1;
    }
    if (a > 0) tx = (uint32_t) (base + j * (j + 1) / 2 + c);
    if (b > 0) ty = (uint32_t) (base + C + (j - 1) * j / 2 + c);
    if (c > 0) tz = (uint32_t) (base + 2 * C + (j - 1) * j / 2 + c - 1);
    for (uint32_t t : {tx, ty, tz})
      if (t != 0xffffu) hits[t]++;
    p.basic_tgt[2 * (size_t) i] = (int32_t) (tx | (ty << 16));
    p.basic_tgt[2 * (size_t) i + 1] = (int32_t) (tz | (fa << 16) | ((uint32_t) b << 20) | ((uint32_t) c << 24));
  }
  p.coef_dense = 1;
  for (int t = 0; t < p.coef_total; t++) {
    if (hits[t] > 1) return refuse(err, MTP_ERR_TABLE, "alpha_index_basic lists the same (mu, a, b, c) twice");
    if (hits[t] == 0) p.coef_dense = 0;
  }
  return MTP_OK;
}

// Head x tail blocks of the basic-moment pass (layout: mtp_potential.hpp).  They depend on the slots and the basics
// only, so they are built once, before the bank search (whose effort follows their number); the nine basic indices are
// in file numbering here and relabel moves them to LDS numbering.
int build_blocks(mtp_potential &p, std::string &err)
{
  const int B = p.alpha_index_basic_count, P = p.max_alpha_index_basic, slot_count = p.slot_count;
  std::vector<int> basic_of((size_t) slot_count * 16 * 16 * 16, -1);   // (slot, a, b, c) -> k
  for (int i = 0; i < B; i++) {
    const int32_t *q = &p.alpha_index_basic[4 * (size_t) i];
    basic_of[(((size_t) (p.basic_pack[i] & 255) * 16 + q[1]) * 16 + q[2]) * 16 + q[3]] = i;
  }
  p.fwd_blocks.clear();
  p.fwd_block_count = 0;
  std::vector<int> covered((size_t) B, 0);
  for (int j = 0; j < P; j++) {
    std::vector<std::pair<int, int>> heads, tails;   // (slot, a), (b, c)
    for (int nu = j; nu < P; nu++)   // (slots are numbered by nu)
      for (int sidx = p.deg_first[nu]; sidx < p.deg_first[nu + 1]; sidx++) heads.push_back({sidx, nu - j});
    for (int c = 0; c <= j; c++) tails.push_back({j - c, c});
    for (size_t h0 = 0; h0 < heads.size(); h0 += 3)
      for (size_t t0 = 0; t0 < tails.size(); t0 += 3) {
        int32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int16_t kk[10];
        for (int e = 0; e < 10; e++) kk[e] = -1;
        bool any = false;
        for (int h = 0; h < 3 && h0 + h < heads.size(); h++) {
          w[0] |= heads[h0 + h].first << (8 * h);
          w[1] |= heads[h0 + h].second << (4 * h);
        }
        for (int t = 0; t < 3 && t0 + t < tails.size(); t++) {
          w[1] |= tails[t0 + t].first << (12 + 4 * t);
          w[2] |= tails[t0 + t].second << (4 * t);
        }
        for (int h = 0; h < 3 && h0 + h < heads.size(); h++)
          for (int t = 0; t < 3 && t0 + t < tails.size(); t++) {
            const int k = basic_of[(((size_t) heads[h0 + h].first * 16 + heads[h0 + h].second) * 16 +
                                    tails[t0 + t].first) * 16 + tails[t0 + t].second];
            if (k >= 0) {
              kk[3 * h + t] = (int16_t) k;
              covered[k]++;
              any = true;
            }
          }
        if (!any) continue;
        std::memcpy(&w[3], kk, sizeof(int16_t) * 10);
        p.fwd_blocks.insert(p.fwd_blocks.end(), w, w + 8);
        p.fwd_block_count++;
      }
  }
  for (int i = 0; i < B; i++)
    if (covered[i] != 1)
      return refuse(err, MTP_ERR_TABLE, "internal: basic moment not covered exactly once by the head x tail blocks");
  return MTP_OK;
}

// Five-factor blocks of the basic-moment pass (layout: mtp_potential.hpp), beside the 3 x 3 ones: the same head x tail
// grids, one per j = nu - a = b + c, cut into 3 heads x 2 tails or 2 heads x 3 tails, whichever takes fewer blocks for
// the grid (the 3 x 2 cut at equal counts).  Heads and tails that no listed basic uses are left out of the grid first,
// so a partly listed group is covered by the blocks its basics need, with -1 in the product slots that have no basic.
// Basic indices in file numbering; relabel moves them to LDS numbering.
int build_blocks5(mtp_potential &p, std::string &err)
{
  const int B = p.alpha_index_basic_count, P = p.max_alpha_index_basic, slot_count = p.slot_count;
  std::vector<int> basic_of((size_t) slot_count * 16 * 16 * 16, -1);   // (slot, a, b, c) -> k
  for (int i = 0; i < B; i++) {
    const int32_t *q = &p.alpha_index_basic[4 * (size_t) i];
    basic_of[(((size_t) (p.basic_pack[i] & 255) * 16 + q[1]) * 16 + q[2]) * 16 + q[3]] = i;
  }
  p.fwd5_blocks.clear();
  p.fwd5_block_count = 0;
  std::vector<int> covered((size_t) B, 0);
  typedef std::pair<int, int> Pair;
  for (int j = 0; j < P; j++) {
    std::vector<Pair> heads, tails;   // (slot, a), (b, c)
    auto basic = [&](const Pair &h, const Pair &t) {
      return basic_of[(((size_t) h.first * 16 + h.second) * 16 + t.first) * 16 + t.second];
    };
    {
      std::vector<Pair> all_heads, all_tails;
      for (int nu = j; nu < P; nu++)   // (slots are numbered by nu)
        for (int sidx = p.deg_first[nu]; sidx < p.deg_first[nu + 1]; sidx++) all_heads.push_back({sidx, nu - j});
      for (int c = 0; c <= j; c++) all_tails.push_back({j - c, c});
      for (const Pair &h : all_heads)
        if (std::any_of(all_tails.begin(), all_tails.end(), [&](const Pair &t) { return basic(h, t) >= 0; })) heads.push_back(h);
      for (const Pair &t : all_tails)
        if (std::any_of(heads.begin(), heads.end(), [&](const Pair &h) { return basic(h, t) >= 0; })) tails.push_back(t);
    }
    // the blocks of the grid cut nh heads x nt tails (3 x 2 or 2 x 3), empty ones left out
    auto cut = [&](int nh, int nt, std::vector<int32_t> *out) {
      int count = 0;
      for (size_t h0 = 0; h0 < heads.size(); h0 += nh)
        for (size_t t0 = 0; t0 < tails.size(); t0 += nt) {
          // factors 0, 1: heads; 3, 4: tails; 2: the third head (3 x 2) or the third tail (2 x 3)
          const int hf[3] = {0, 1, 2}, tf[3] = {3, 4, 2};
          int32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          int16_t kk[6] = {-1, -1, -1, -1, -1, -1};
          bool any = false;
          for (int h = 0; h < nh && h0 + h < heads.size(); h++) w[hf[h]] |= heads[h0 + h].first | (heads[h0 + h].second << 16);
          for (int t = 0; t < nt && t0 + t < tails.size(); t++) w[tf[t]] |= tails[t0 + t].first | (tails[t0 + t].second << 16);
          if (nh == 3) w[2] |= (int32_t) 0x80000000u;   // shape bit: factor 2 is a head
          for (int h = 0; h < nh && h0 + h < heads.size(); h++)
            for (int t = 0; t < nt && t0 + t < tails.size(); t++) {
              const int k = basic(heads[h0 + h], tails[t0 + t]);
              if (k < 0) continue;
              // products (0,3) (0,4) (1,3) (1,4), then (2,3) (2,4) of the 3 x 2 shape or (0,2) (1,2) of the 2 x 3 one
              const int e = h < 2 && t < 2 ? 2 * h + t : nh == 3 ? 4 + t : 4 + h;
              kk[e] = (int16_t) k;
              if (out) covered[k]++;
              any = true;
            }
          if (!any) continue;
          count++;
          if (out) {
            std::memcpy(&w[5], kk, sizeof kk);
            out->insert(out->end(), w, w + 8);
          }
        }
      return count;
    };
    if (heads.empty()) continue;
    const bool wide = cut(3, 2, nullptr) <= cut(2, 3, nullptr);
    p.fwd5_block_count += wide ? cut(3, 2, &p.fwd5_blocks) : cut(2, 3, &p.fwd5_blocks);
  }
  for (int i = 0; i < B; i++)
    if (covered[i] != 1)
      return refuse(err, MTP_ERR_TABLE, "internal: basic moment not covered exactly once by the five-factor blocks");
  return MTP_OK;
}

// leaf moments (mtp_potential.hpp): written by rows, never read by one, not a basic.  Their rows are deferred to the
// end of the forward pass, which keeps the reference's in-order semantics only if no later row still adds to one of
// the row's factors: a leaf with such a row stays an ordinary stored moment.
std::vector<char> find_leaves(const mtp_potential &p, bool enabled)
{
  const int A = p.alpha_moment_count, B = p.alpha_index_basic_count, T = p.alpha_index_times_count;
  std::vector<char> leaf((size_t) A, 0);
  if (!enabled) return leaf;
  std::vector<char> is_factor((size_t) A, 0), is_target((size_t) A, 0);
  std::vector<int> last_write((size_t) A, -1);
  for (int k = 0; k < T; k++) {
    const int32_t *q = &p.alpha_index_times[4 * (size_t) k];
    is_factor[q[0]] = is_factor[q[1]] = 1;
    is_target[q[3]] = 1;
    last_write[q[3]] = k;
  }
  for (int m = B; m < A; m++) leaf[m] = is_target[m] && !is_factor[m];
  for (int k = 0; k < T; k++) {
    const int32_t *q = &p.alpha_index_times[4 * (size_t) k];
    if (leaf[q[3]] && (last_write[q[0]] > k || last_write[q[1]] > k)) leaf[q[3]] = 0;
  }
  return leaf;
}

// Dependency levels of the times rows (finalize): rows_by_level (file numbering, stable within a level), level_offset
// and normal_levels
void build_levels(mtp_potential &p, const std::vector<char> &leaf)
{
  const int A = p.alpha_moment_count, T = p.alpha_index_times_count;
  std::vector<int> wlevel((size_t) A, 0), rlevel((size_t) A, 0);
  std::vector<int> lvl((size_t) T, 0);
  int nlev = 0;
  for (int k = 0; k < T; k++) {
    const int32_t *q = &p.alpha_index_times[4 * (size_t) k];
    if (leaf[q[3]]) continue;
    int l = std::max(wlevel[q[0]], wlevel[q[1]]) + 1;   // operands complete
    l = std::max(l, rlevel[q[3]] + 1);                  // earlier readers of a3 come first
    lvl[k] = l;
    wlevel[q[3]] = std::max(wlevel[q[3]], l);
    rlevel[q[0]] = std::max(rlevel[q[0]], l);
    rlevel[q[1]] = std::max(rlevel[q[1]], l);
    nlev = std::max(nlev, l);
  }
  p.normal_levels = nlev;
  nlev++;   // the leaf rows: one more "level" behind the others (possibly empty)
  for (int k = 0; k < T; k++)
    if (leaf[p.alpha_index_times[4 * (size_t) k + 3]]) lvl[k] = nlev;
  p.level_offset.assign((size_t) nlev + 1, 0);
  for (int k = 0; k < T; k++) p.level_offset[lvl[k]]++;        // counts at [1..nlev]
  for (int l = 1; l <= nlev; l++) p.level_offset[l] += p.level_offset[l - 1];
  // level_offset[l] now = end of level l; shift to starts
  std::vector<int32_t> cur((size_t) nlev + 1, 0);
  for (int l = 1; l <= nlev; l++) cur[l] = p.level_offset[l - 1];
  p.rows_by_level.assign((size_t) T, MtpRow{0, 0, 0, 0});
  for (int k = 0; k < T; k++) {
    const int32_t *q = &p.alpha_index_times[4 * (size_t) k];
    p.rows_by_level[cur[lvl[k]]++] = MtpRow{q[0], q[1], q[2], q[3]};
  }
}

// Rows of one level commute, so order them for the LDS: a wave instruction touches 64 consecutive
// rows, served in lane groups of 32 (reads) / 16 (ds_add_f64).  Greedy: fill each group of 16 with
// the rows whose operand and target moments fall on banks not yet used by a different moment of the
// group (same moment = broadcast for reads, but serialised for the atomic adds).
void order_rows(mtp_potential &p)
{
  const int nlev = p.normal_levels + 1;
  for (int l = 1; l <= nlev; l++) {   // level l (1-based) spans [level_offset[l-1], level_offset[l])
    const int b = p.level_offset[l - 1], e = p.level_offset[l];
    const int n = e - b;
    if (n <= 16) continue;
    std::vector<MtpRow> pool(p.rows_by_level.begin() + b, p.rows_by_level.begin() + e), out;
    std::vector<char> used((size_t) n, 0);
    out.reserve((size_t) n);
    int remaining = n, scan_from = 0;
    while (remaining > 0) {
      int rd0[32], rd1[32], rd3[32];          // moment occupying each read bank in the current 32-group (-1 free)
      for (int h = 0; h < 2 && remaining > 0; h++) {   // two 16-lane halves share the 32-lane read group
        if (h == 0)
          for (int q = 0; q < 32; q++) rd0[q] = rd1[q] = rd3[q] = -1;
        int at0[16], at1[16], at3[16];        // atomic-add banks of this 16-group
        for (int q = 0; q < 16; q++) at0[q] = at1[q] = at3[q] = -1;
        for (int slot = 0; slot < 16 && remaining > 0; slot++) {
          int best = -1, best_cost = 1 << 30;
          int seen = 0;
          for (int k = scan_from; k < n && seen < 256; k++) {   // bounded look-ahead keeps this O(n * 256)
            if (used[k]) continue;
            seen++;
            const MtpRow &r = pool[k];
            int cost = 0;
            cost += (rd0[r.a0 & 31] >= 0 && rd0[r.a0 & 31] != r.a0);
            cost += (rd1[r.a1 & 31] >= 0 && rd1[r.a1 & 31] != r.a1);
            if (l < nlev) {   // (leaf rows neither read D[a3] nor add into M[a3])
              cost += (rd3[r.a3 & 31] >= 0 && rd3[r.a3 & 31] != r.a3);
              cost += 2 * (at3[r.a3 & 15] >= 0);            // forward ds_add target
            }
            cost += (at0[r.a0 & 15] >= 0) + (at1[r.a1 & 15] >= 0);   // backward ds_add targets
            if (cost < best_cost) {
              best_cost = cost;
              best = k;
              if (cost == 0) break;
            }
          }
          assert(best >= 0);   // rows remain, and scan_from is the first unused one
          const MtpRow &r = pool[best];
          used[best] = 1;
          remaining--;
          while (scan_from < n && used[scan_from]) scan_from++;
          rd0[r.a0 & 31] = r.a0;
          rd1[r.a1 & 31] = r.a1;
          rd3[r.a3 & 31] = r.a3;
          at0[r.a0 & 15] = r.a0;
          at1[r.a1 & 15] = r.a1;
          at3[r.a3 & 15] = r.a3;
          out.push_back(r);
        }
      }
    }
    std::copy(out.begin(), out.end(), p.rows_by_level.begin() + b);
  }
}

// Pad every level to whole 64-row blocks with neutral rows (multiplicity 0, operands = target, a
// different moment in every lane): the product kernels then run without bounds checks or lane masks.
void pad_levels(mtp_potential &p, const std::vector<char> &leaf)
{
  const int nlev = p.normal_levels + 1;
  std::vector<int> stored;   // (file numbering; the leaves have no LDS slot a padding row could touch)
  for (int m = 0; m < p.alpha_moment_count; m++)
    if (!leaf[m]) stored.push_back(m);
  if (stored.empty()) stored.push_back(0);
  std::vector<MtpRow> padded;
  std::vector<int32_t> off((size_t) nlev + 1, 0);
  for (int l = 1; l <= nlev; l++) {
    const int b = p.level_offset[l - 1], e = p.level_offset[l];
    padded.insert(padded.end(), p.rows_by_level.begin() + b, p.rows_by_level.begin() + e);
    while ((int) padded.size() % 64 != 0) {
      const int t = stored[(size_t) ((int) padded.size() % 64) % stored.size()];
      padded.push_back(MtpRow{t, t, 0, t});
    }
    off[l] = (int32_t) padded.size();
  }
  p.rows_by_level.swap(padded);
  p.level_offset.swap(off);
}

// The starting LDS numbering: basics keep their numbers, the stored products follow in file order, and the leaves take
// the numbers behind the stored moments (only grade calls give them LDS slots).
void number_moments(mtp_potential &p, const std::vector<char> &leaf)
{
  const int A = p.alpha_moment_count, B = p.alpha_index_basic_count;
  int nstored = B;
  for (int m = B; m < A; m++) nstored += !leaf[m];
  p.stored_moment_count = nstored;
  p.moment_perm.resize((size_t) A);
  int next_stored = B, next_leaf = nstored;
  for (int m = 0; m < A; m++) p.moment_perm[m] = m < B ? m : (leaf[m] ? next_leaf++ : next_stored++);
}

// LDS numbering of the moments and order of the rows inside their levels, by the bank search (mtp_bank_search.hpp) on
// the rows, the numbering and the level bounds alone.  moment_perm[file index] = LDS index; relabel writes every device
// table in LDS numbering.
void search_banks(mtp_potential &p, const std::vector<char> &leaf, const ScheduleOptions &opt)
{
  mtp_bank_search::Table table{p.rows_by_level, p.moment_perm, p.level_offset, p.level_offset[(size_t) p.normal_levels],
                               p.alpha_index_basic_count, leaf};
  mtp_bank_search::search(table, {opt.search_v1, opt.bank_rounds, opt.bank_scale, opt.debug_banks, p.fwd_block_count});
}

// Everything the kernels index by moment, in LDS numbering (moment_perm): the rows, the adjoint seeds, the leaf and
// energy tables, mapping_lds, the basic descriptors and targets and the head x tail blocks.
void relabel(mtp_potential &p, const std::vector<char> &leaf)
{
  const int A = p.alpha_moment_count, B = p.alpha_index_basic_count, S = p.alpha_scalar_count;
  const std::vector<int32_t> &perm = p.moment_perm;
  for (MtpRow &row : p.rows_by_level) {
    row.a0 = perm[row.a0];
    row.a1 = perm[row.a1];
    row.a3 = perm[row.a3];
  }
  // the index side of the scalar tables (structure only); their values: mtp_build_coeff_tables
  std::vector<int> last((size_t) A, -1);
  for (int i = 0; i < S; i++) last[p.alpha_moment_mapping[i]] = i;
  p.seed_idx.clear();
  for (int m = 0; m < A; m++) {
    assert((leaf[m] != 0) == (perm[m] >= p.stored_moment_count));   // numbers swap inside a class only
    if (last[m] >= 0 && !leaf[m]) p.seed_idx.push_back(perm[m]);
  }
  p.e_map.clear();
  for (int i = 0; i < S; i++)
    if (!leaf[p.alpha_moment_mapping[i]]) p.e_map.push_back(perm[p.alpha_moment_mapping[i]]);
  mtp_coeff_tables ct;
  mtp_build_coeff_tables(p, nullptr, nullptr, nullptr, ct);
  p.seed_val.swap(ct.seed_val);
  p.e_lin.swap(ct.e_lin);
  p.leaf_cf.swap(ct.leaf_cf);
  p.leaf_cb.swap(ct.leaf_cb);
  p.mapping_lds.resize((size_t) S);
  for (int i = 0; i < S; i++) p.mapping_lds[i] = perm[p.alpha_moment_mapping[i]];
  // packed basic descriptors (mtp_cvec_kernel pairs them with dbasic[k] = D[k]) and coefficient targets at the basic's
  // LDS number: the kernel walks D[k], tgt[k] with k in LDS numbering
  p.basic_pack_lds.assign((size_t) B, 0);
  std::vector<int32_t> tgt((size_t) 2 * B, 0);
  for (int i = 0; i < B; i++) {
    p.basic_pack_lds[(size_t) perm[i]] = p.basic_pack[i];
    tgt[2 * (size_t) perm[i]] = p.basic_tgt[2 * (size_t) i];
    tgt[2 * (size_t) perm[i] + 1] = p.basic_tgt[2 * (size_t) i + 1];
  }
  p.basic_tgt.swap(tgt);
  for (int blk = 0; blk < p.fwd_block_count; blk++) {   // the nine basic indices of each head x tail block
    int16_t kk[10];
    std::memcpy(kk, &p.fwd_blocks[(size_t) 8 * blk + 3], sizeof kk);
    for (int16_t &k : kk)
      if (k >= 0) k = (int16_t) perm[k];
    std::memcpy(&p.fwd_blocks[(size_t) 8 * blk + 3], kk, sizeof kk);
  }
  for (int blk = 0; blk < p.fwd5_block_count; blk++) {   // and the six of each five-factor block
    int16_t kk[6];
    std::memcpy(kk, &p.fwd5_blocks[(size_t) 8 * blk + 5], sizeof kk);
    for (int16_t &k : kk)
      if (k >= 0) k = (int16_t) perm[k];
    std::memcpy(&p.fwd5_blocks[(size_t) 8 * blk + 5], kk, sizeof kk);
  }
}

// ---- gather programs of the product passes ---------------------------------------------------------------------
// The product passes as the kernel runs them (mtp_kernels.hip, gather_pass): per level a list of *chunks*; a chunk
// holds up to cs operations acc += mult * X[o0] * Y[o1] that share one target, lane l of a group of 64 lanes runs one
// chunk and ends it with ONE atomic add T[tgt] += acc.  Forward pass (pair_mtp.cpp:196-201): X = Y = T = moments,
// chunks = the rows of a target.  Reverse pass (:221-233): X = adjoints, Y = moments, T = adjoints, chunks = the
// terms D[a3] mult M[other] of one destination moment -- so the reverse pass needs two atomics per FOUR-TO-EIGHT
// rows instead of two per row.  The chunk size cs in {1, 2, 4, 8} is chosen per level and pass by modelled LDS cycles
// (2 per read, 15 per atomic add, padding included); chunks are dealt to lanes greedily so that the operands of one
// wave instruction spread over the LDS banks (reads: 32 lanes over 32 eight-byte banks, adds: 16 lanes over 16).

// one level of a program: G groups of 64 lanes x cs operations from prog[base]
struct ProgramLevel {
  std::vector<MtpRow> &prog;
  size_t base;
  int G, cs;
  MtpRow &op(int g, int u, int lane) const { return prog[base + ((size_t) g * cs + u) * 64 + lane]; }
  bool real_chunk(int g, int lane) const
  {
    for (int u = 0; u < cs; u++)
      if (op(g, u, lane).mult != 0) return true;
    return false;
  }
};

// Local search on top of the greedy deal (deterministic, fixed-seed LCG): swap the chunks of two lanes of the level,
// or two operations inside a chunk (their sum does not depend on the order), whenever the modelled extra cycles --
// per wave instruction and 32-lane half the largest number of distinct addresses on one read bank, per 16-lane
// group the largest number of adds on one bank -- do not grow.  Padding operations (mult 0) are wildcards: they
// end up on an address another lane of their half reads anyway (a broadcast, fill_wildcards).  Measured on the
// level-20 programs: average bank load of the reads 2.1 -> 1.3.
void refine_program(const ProgramLevel &lv)
{
  const int G = lv.G, cs = lv.cs;
  int hot = 0;   // a lane on the most loaded bank of the last read_cost call
  auto read_cost = [&](int g, int u, int half, int which) {
    int first[32], extra[32][7], mx = 0;
    uint8_t n[32] = {0};
    for (int lane = 32 * half; lane < 32 * half + 32; lane++) {
      const MtpRow &o = lv.op(g, u, lane);
      if (o.mult == 0) continue;
      const int a = which ? o.a1 : o.a0, b = a & 31;
      bool dup = false;
      if (n[b] > 0) {
        dup = first[b] == a;
        for (int k = 0; k + 1 < n[b] && k < 7 && !dup; k++) dup = extra[b][k] == a;
      }
      if (!dup) {
        if (n[b] == 0) first[b] = a;
        else if (n[b] - 1 < 7) extra[b][n[b] - 1] = a;
        n[b]++;
        if (n[b] > mx) {
          mx = n[b];
          hot = lane;
        }
      }
    }
    return mx > 1 ? mx - 1 : 0;
  };
  auto add_cost = [&](int g, int q) {
    uint8_t h[16] = {0};
    int mx = 0;
    for (int lane = 16 * q; lane < 16 * q + 16; lane++)
      if (lv.real_chunk(g, lane) && ++h[lv.op(g, 0, lane).a3 & 15] > mx) {
        mx = h[lv.op(g, 0, lane).a3 & 15];
        hot = lane;
      }
    return mx > 1 ? 2 * (mx - 1) : 0;
  };
  std::vector<int> rc((size_t) G * cs * 4), ac((size_t) G * 4);
  for (int g = 0; g < G; g++) {
    for (int u = 0; u < cs; u++)
      for (int hw = 0; hw < 4; hw++) rc[((size_t) g * cs + u) * 4 + hw] = read_cost(g, u, hw >> 1, hw & 1);
    for (int q = 0; q < 4; q++) ac[(size_t) g * 4 + q] = add_cost(g, q);
  }
  mtp_bank_search::Lcg next{0xD1B54A32D192ED03ull};
  const long long trials = std::min<long long>(300ll * G * 64, 300000ll);
  for (long long t = 0; t < trials; t++) {
    // start from a read (or, one time in four, an add) that has a conflict: a lane on its most loaded bank moves
    const int g0 = (int) (next() % (uint32_t) G), u0 = (int) (next() % (uint32_t) cs), hw0 = (int) (next() & 3);
    const bool from_add = (next() & 3) == 0;
    if (from_add) {
      if (ac[(size_t) g0 * 4 + hw0] == 0) continue;
      (void) add_cost(g0, hw0);
    } else {
      if (rc[((size_t) g0 * cs + u0) * 4 + hw0] == 0) continue;
      (void) read_cost(g0, u0, hw0 >> 1, hw0 & 1);
    }
    const int lane0 = hot;
    if (!from_add && cs > 1 && (next() & 1) == 0) {   // two operations of one chunk
      const int g = g0, lane = lane0, half = lane >> 5;
      const int u1 = u0, u2 = (int) (next() % (uint32_t) cs);
      if (u1 == u2) continue;
      int before = 0, after = 0;
      for (int w = 0; w < 2; w++) before += rc[((size_t) g * cs + u1) * 4 + 2 * half + w] + rc[((size_t) g * cs + u2) * 4 + 2 * half + w];
      std::swap(lv.op(g, u1, lane), lv.op(g, u2, lane));
      int nc[4];
      for (int w = 0; w < 2; w++) {
        nc[w] = read_cost(g, u1, half, w);
        nc[2 + w] = read_cost(g, u2, half, w);
        after += nc[w] + nc[2 + w];
      }
      if (after > before) {
        std::swap(lv.op(g, u1, lane), lv.op(g, u2, lane));
        continue;
      }
      for (int w = 0; w < 2; w++) {
        rc[((size_t) g * cs + u1) * 4 + 2 * half + w] = nc[w];
        rc[((size_t) g * cs + u2) * 4 + 2 * half + w] = nc[2 + w];
      }
    } else {   // the chunks of two lanes
      const int g1 = g0, l1 = lane0;
      const int g2 = (int) (next() % (uint32_t) G), l2 = (int) (next() & 63);
      const int h1 = l1 >> 5, h2 = l2 >> 5, q1 = l1 >> 4, q2 = l2 >> 4;
      if (g1 == g2 && q1 == q2) continue;   // same add group, hence same read half: nothing changes
      const bool same_half = g1 == g2 && h1 == h2;
      int before = ac[(size_t) g1 * 4 + q1] + ac[(size_t) g2 * 4 + q2], after = 0;
      for (int u = 0; u < cs; u++)
        for (int w = 0; w < 2; w++) {
          before += rc[((size_t) g1 * cs + u) * 4 + 2 * h1 + w];
          if (!same_half) before += rc[((size_t) g2 * cs + u) * 4 + 2 * h2 + w];
        }
      for (int u = 0; u < cs; u++) std::swap(lv.op(g1, u, l1), lv.op(g2, u, l2));
      int n1[16], n2[16];
      for (int u = 0; u < cs; u++)
        for (int w = 0; w < 2; w++) {
          n1[2 * u + w] = read_cost(g1, u, h1, w);
          after += n1[2 * u + w];
          if (!same_half) {
            n2[2 * u + w] = read_cost(g2, u, h2, w);
            after += n2[2 * u + w];
          }
        }
      const int a1 = add_cost(g1, q1), a2 = add_cost(g2, q2);
      after += a1 + a2;
      if (after > before) {
        for (int u = 0; u < cs; u++) std::swap(lv.op(g1, u, l1), lv.op(g2, u, l2));
        continue;
      }
      for (int u = 0; u < cs; u++)
        for (int w = 0; w < 2; w++) {
          rc[((size_t) g1 * cs + u) * 4 + 2 * h1 + w] = n1[2 * u + w];
          if (!same_half) rc[((size_t) g2 * cs + u) * 4 + 2 * h2 + w] = n2[2 * u + w];
        }
      ac[(size_t) g1 * 4 + q1] = a1;
      ac[(size_t) g2 * 4 + q2] = a2;
    }
  }
}

// wildcards: read what another lane of the half reads (broadcast); padding chunks add 0.0 on a free add bank
void fill_wildcards(const ProgramLevel &lv, int A_st)
{
  for (int g = 0; g < lv.G; g++) {
    for (int u = 0; u < lv.cs; u++)
      for (int half = 0; half < 2; half++) {
        int a0 = 0, a1 = 0;
        for (int lane = 32 * half; lane < 32 * half + 32; lane++)
          if (lv.op(g, u, lane).mult != 0) {
            a0 = lv.op(g, u, lane).a0;
            a1 = lv.op(g, u, lane).a1;
            break;
          }
        for (int lane = 32 * half; lane < 32 * half + 32; lane++)
          if (lv.op(g, u, lane).mult == 0) {
            lv.op(g, u, lane).a0 = a0;
            lv.op(g, u, lane).a1 = a1;
          }
      }
    for (int q = 0; q < 4; q++) {
      bool busy[16] = {false};
      for (int lane = 16 * q; lane < 16 * q + 16; lane++)
        if (lv.real_chunk(g, lane)) busy[lv.op(g, 0, lane).a3 & 15] = true;
      for (int lane = 16 * q; lane < 16 * q + 16; lane++) {
        if (lv.real_chunk(g, lane)) continue;
        int t = lv.op(g, 0, lane).a3;
        for (int m = 0; m < A_st; m++)
          if (!busy[m & 15]) {
            t = m;
            break;
          }
        busy[t & 15] = true;
        for (int u = 0; u < lv.cs; u++) lv.op(g, u, lane).a3 = t;
      }
    }
  }
}

// the gather program of one pass (levels in execution order) and its per-level segments
void build_program(const mtp_potential &p, bool reverse, bool refine, std::vector<MtpRow> &prog,
                   std::vector<int32_t> &seg)
{
  const int A = p.alpha_moment_count;
  const int nlev2 = p.normal_levels;   // (the leaf rows keep the row-per-lane form: no target to share)
  const int A_st = p.stored_moment_count;
  prog.clear();
  seg.clear();
  for (int li = 0; li < nlev2; li++) {
    const int l = reverse ? nlev2 - 1 - li : li;
    // operations of the level, keyed by target
    std::vector<std::vector<MtpRow>> by_tgt((size_t) A);
    for (int r = p.level_offset[l]; r < p.level_offset[l + 1]; r++) {
      const MtpRow &row = p.rows_by_level[(size_t) r];
      if (row.mult == 0) continue;   // neutral padding rows of the old layout
      if (!reverse) {
        by_tgt[(size_t) row.a3].push_back(row);
      } else if (row.a0 == row.a1 && 2 * row.mult <= 32767 && 2 * row.mult >= -32768) {
        by_tgt[(size_t) row.a0].push_back(MtpRow{row.a3, row.a0, 2 * row.mult, row.a0});   // both terms in one
      } else {
        by_tgt[(size_t) row.a1].push_back(MtpRow{row.a3, row.a0, row.mult, row.a1});       // D[a1] += D[a3] mult M[a0]
        by_tgt[(size_t) row.a0].push_back(MtpRow{row.a3, row.a1, row.mult, row.a0});       // D[a0] += D[a3] mult M[a1]
      }
    }
    // chunk size by modelled LDS cycles
    int best_cs = 1;
    long long best_cost = -1;
    for (int cs : {1, 2, 4, 8}) {
      long long chunks = 0;
      for (const auto &v : by_tgt) chunks += ((long long) v.size() + cs - 1) / cs;
      const long long groups = (chunks + 63) / 64, cost = groups * cs * 6 + groups * 15;
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best_cs = cs;
      }
    }
    const int cs = best_cs;
    struct Chunk {
      int tgt;
      MtpRow op[8];
    };
    std::vector<Chunk> chunks;
    for (int t = 0; t < A; t++) {
      const auto &v = by_tgt[(size_t) t];
      for (size_t b = 0; b < v.size(); b += (size_t) cs) {
        Chunk c;
        c.tgt = t;
        for (int u = 0; u < cs; u++) c.op[u] = b + u < v.size() ? v[b + u] : MtpRow{t, t, 0, t};
        chunks.push_back(c);
      }
    }
    // longest-first would not matter (all chunks are cs long after padding); keep file order, pad to whole groups
    const int ngroups = (int) ((chunks.size() + 63) / 64);
    const int first_block = (int) (prog.size() / 64);
    std::vector<char> used(chunks.size(), 0);
    size_t scan_from = 0;
    for (int g = 0; g < ngroups; g++) {
      int occx[8][2][32], occy[8][2][32], occt[4][16];
      std::fill_n(&occx[0][0][0], 8 * 2 * 32, -1);
      std::fill_n(&occy[0][0][0], 8 * 2 * 32, -1);
      std::fill_n(&occt[0][0], 4 * 16, -1);
      std::vector<MtpRow> blk((size_t) 64 * cs);
      for (int lane = 0; lane < 64; lane++) {
        const int half = lane >> 5, q16 = lane >> 4;
        int best = -1, best_rot = 0, bcost = 1 << 30, seen = 0;
        for (size_t k = scan_from; k < chunks.size() && seen < 128; k++) {
          if (used[k]) continue;
          seen++;
          const Chunk &c = chunks[k];
          const int tcost = 3 * (occt[q16][c.tgt & 15] >= 0);
          for (int rot = 0; rot < cs; rot++) {
            int cost = tcost;
            for (int u = 0; u < cs; u++) {
              const MtpRow &o = c.op[(u + rot) % cs];
              const int bx = occx[u][half][o.a0 & 31], by = occy[u][half][o.a1 & 31];
              cost += (bx >= 0 && bx != o.a0) + (by >= 0 && by != o.a1);
            }
            if (cost < bcost) {
              bcost = cost;
              best = (int) k;
              best_rot = rot;
            }
            if (cost == 0) break;
          }
          if (bcost == 0) break;
        }
        Chunk c;
        if (best >= 0) {
          c = chunks[(size_t) best];
          used[(size_t) best] = 1;
          while (scan_from < chunks.size() && used[scan_from]) scan_from++;
        } else {   // padding chunk: adds 0.0 to a moment whose add bank is still free in this 16-lane group
          int t = 0;
          for (int m = 0; m < A_st; m++)
            if (occt[q16][m & 15] < 0) {
              t = m;
              break;
            }
          c.tgt = t;
          for (int u = 0; u < cs; u++) c.op[u] = MtpRow{t, t, 0, t};
          best_rot = 0;
        }
        occt[q16][c.tgt & 15] = c.tgt;
        for (int u = 0; u < cs; u++) {
          MtpRow o = c.op[(u + best_rot) % cs];
          o.a3 = c.tgt;
          occx[u][half][o.a0 & 31] = o.a0;
          occy[u][half][o.a1 & 31] = o.a1;
          blk[(size_t) u * 64 + lane] = o;
        }
      }
      prog.insert(prog.end(), blk.begin(), blk.end());
    }
    const ProgramLevel lv{prog, (size_t) first_block * 64, ngroups, cs};
    if (refine && ngroups > 0) {
      refine_program(lv);
      fill_wildcards(lv, A_st);
    }
    seg.insert(seg.end(), {first_block, ngroups, cs, 0});
  }
}

}   // namespace

// Build the native schedule.  The reference executes the times rows strictly in file
// order (pair_mtp.cpp:196-201) and in reverse for the adjoint (:221-233).  Rows are
// assigned to dependency levels so that any two rows in one level commute under that
// sequential semantics (read-after-write and write-after-read on the moment array are
// both respected); a level is then executed by all lanes at once.  Every input check
// runs before the schedule work.
int mtp_potential::finalize(std::string &err)
{
  const ScheduleOptions opt = read_options();
  int rc = validate(*this, err);
  if (rc == MTP_OK) rc = build_slots(*this, err);
  if (rc == MTP_OK) rc = build_blocks(*this, err);
  if (rc == MTP_OK) rc = build_blocks5(*this, err);
  if (rc != MTP_OK) return rc;
  const std::vector<char> leaf = find_leaves(*this, opt.leaves);
  build_levels(*this, leaf);
  order_rows(*this);
  pad_levels(*this, leaf);
  number_moments(*this, leaf);
  if (alpha_moment_count >= 2 && !rows_by_level.empty() && opt.renumber) search_banks(*this, leaf, opt);
  relabel(*this, leaf);
  // the kernel runs the gather programs in its 64-lane block grids only -- more than 32 head x tail blocks --, unless
  // it was built with -DMTP_GATHER_ALL; MTP_REFINE_PROGRAMS=0 / 1 overrides the local search on them
  const bool refine = opt.refine_programs >= 0 ? opt.refine_programs != 0 : fwd_block_count > 32;
  build_program(*this, false, refine, prog_fwd, seg_fwd);
  build_program(*this, true, refine, prog_bwd, seg_bwd);
  return MTP_OK;
}

// ---- the tangent kernel's table and the coefficient writer (host only; include/mtp_mi355x.h, "linear refit") ---------
void mtp_build_design_table(const mtp_potential &pot, mtp_design_table &out)
{
  out.A = pot.alpha_moment_count;
  out.B = pot.alpha_index_basic_count;
  out.S = pot.alpha_scalar_count;
  out.nblocks = (int) pot.level_offset.size() - 1;   // the dependency levels and the leaf block behind them
  out.rows = pot.rows_by_level;
  out.level_offset = pot.level_offset;
  out.scalar_map = pot.mapping_lds;
  out.basic_pack = pot.basic_pack_lds;
  out.force_map.assign((size_t) out.S, -1);
  std::vector<int> last((size_t) std::max(out.A, 1), -1);
  for (int s = 0; s < out.S; s++) last[(size_t) pot.mapping_lds[(size_t) s]] = s;
  for (int s = 0; s < out.S; s++)
    if (last[(size_t) pot.mapping_lds[(size_t) s]] == s) out.force_map[(size_t) s] = pot.mapping_lds[(size_t) s];
}

// the training kernel's table: the design table, the basics ordered by mu, and the two shapes its formulas do not cover
int mtp_build_train_table(const mtp_potential &pot, mtp_train_table &out, std::string &err)
{
  mtp_build_design_table(pot, out.design);
  const int B = out.design.B, Mu = pot.radial_func_count;
  out.mufirst.assign((size_t) Mu + 1, 0);
  out.bymu.clear();
  for (int mu = 0; mu < Mu; mu++) {
    for (int k = 0; k < B; k++)
      if (((out.design.basic_pack[(size_t) k] >> 20) & 15) == mu) out.bymu.push_back(k);
    out.mufirst[(size_t) mu + 1] = (int32_t) out.bymu.size();
  }
  out.late_row = -1;
  out.dup_scalar = -1;
  // in FILE order: a row that reads a moment a later row (or itself) still adds to -- the reference's reverse sweep is then
  // not the transpose of its forward sweep (pair_mtp.cpp:196-233)
  const int T = pot.alpha_index_times_count;
  std::vector<int> last_writer((size_t) std::max(pot.alpha_moment_count, 1), -1);
  for (int k = 0; k < T; k++) last_writer[(size_t) pot.alpha_index_times[4 * (size_t) k + 3]] = k;
  for (int k = 0; k < T && out.late_row < 0; k++)
    if (last_writer[(size_t) pot.alpha_index_times[4 * (size_t) k]] >= k || last_writer[(size_t) pot.alpha_index_times[4 * (size_t) k + 1]] >= k)
      out.late_row = k;
  // two scalars on one moment: the energy sums them, the adjoint keeps the last (:204-218)
  std::vector<int> seen((size_t) std::max(pot.alpha_moment_count, 1), -1);
  for (int s = 0; s < pot.alpha_scalar_count && out.dup_scalar < 0; s++) {
    int &q = seen[(size_t) pot.alpha_moment_mapping[(size_t) s]];
    if (q >= 0) out.dup_scalar = s;
    q = s;
  }
  if (out.late_row >= 0) {
    err = "training gradient: row " + std::to_string(out.late_row) + " of alpha_index_times reads a moment that row " +
        std::to_string(std::max(last_writer[(size_t) pot.alpha_index_times[4 * (size_t) out.late_row]],
                                last_writer[(size_t) pot.alpha_index_times[4 * (size_t) out.late_row + 1]])) +
        " still adds to: the forces of such a table are not the gradient of its energy";
    return MTP_ERR_UNSUPPORTED;
  }
  if (out.dup_scalar >= 0) {
    err = "training gradient: scalar " + std::to_string(out.dup_scalar) + " of alpha_moment_mapping is mapped to moment " +
        std::to_string(pot.alpha_moment_mapping[(size_t) out.dup_scalar]) +
        ", which an earlier scalar is mapped to as well: the forces of such a table are not the gradient of its energy";
    return MTP_ERR_UNSUPPORTED;
  }
  return MTP_OK;
}

namespace {

void copy_message(const std::string &s, char *err, int errlen)
{
  if (err && errlen > 0) std::snprintf(err, (size_t) errlen, "%s", s.c_str());
}

// first word of a line under the parser's separators, comments stripped as the reader strips them
std::string first_word(const std::string &line, bool strip_comment)
{
  std::string s = line;
  if (strip_comment) {
    const size_t p = s.find('#');
    if (p != std::string::npos) s.erase(p);
  }
  const char *seps = " \t\r\n\f=,{}";
  const size_t b = s.find_first_not_of(seps);
  if (b == std::string::npos) return "";
  const size_t e = s.find_first_of(seps, b);
  return s.substr(b, (e == std::string::npos ? s.size() : e) - b);
}

std::string coeff_line(const char *key, const double *v, int n, const std::string &eol)
{
  std::string s = std::string(key) + " = {";
  char num[40];
  for (int i = 0; i < n; i++) {
    std::snprintf(num, sizeof num, "%.16e", v[i]);   // 17 significant digits: strtod returns the same bits
    if (i) s += ", ";
    s += num;
  }
  return s + "}" + eol;
}

}   // namespace

extern "C" {

int mtp_potential_design_table(const mtp_potential *pot, int32_t *counts, int32_t *rows, int32_t *level_offset,
                               int32_t *scalar_map, int32_t *force_map, int32_t *basic_pack)
{
  if (!pot) return MTP_ERR_ARG;
  mtp_design_table t;
  mtp_build_design_table(*pot, t);
  if (counts) {
    counts[0] = (int32_t) t.rows.size();
    counts[1] = t.nblocks;
    counts[2] = t.A;
    counts[3] = t.B;
  }
  if (rows)
    for (size_t k = 0; k < t.rows.size(); k++) {
      rows[4 * k] = t.rows[k].a0;
      rows[4 * k + 1] = t.rows[k].a1;
      rows[4 * k + 2] = t.rows[k].mult;
      rows[4 * k + 3] = t.rows[k].a3;
    }
  if (level_offset) std::copy(t.level_offset.begin(), t.level_offset.end(), level_offset);
  if (scalar_map) std::copy(t.scalar_map.begin(), t.scalar_map.end(), scalar_map);
  if (force_map) std::copy(t.force_map.begin(), t.force_map.end(), force_map);
  if (basic_pack) std::copy(t.basic_pack.begin(), t.basic_pack.end(), basic_pack);
  return MTP_OK;
}

// the two writers: `radial` == nullptr keeps the radial block of the source byte for byte
static int write_coeffs_common(const std::string &who, const char *src_path, const char *dst_path, const double *radial,
                               int radial_count, const double *species_coeffs, const double *moment_coeffs, int species_count,
                               int scalar_count, char *err, int errlen)
{
  if (!src_path || !dst_path || !moment_coeffs) {
    copy_message(who + ": null argument", err, errlen);
    return MTP_ERR_ARG;
  }
  mtp_potential src;
  std::string msg;
  int rc = mtp_parse_text_file(src_path, false, src, msg);   // (the tables as read: no schedule is needed here)
  if (rc != MTP_OK) {
    copy_message(msg, err, errlen);
    return rc;
  }
  if ((species_coeffs && species_count != src.species_count) || scalar_count != src.alpha_scalar_count) {
    copy_message(who + ": " + std::to_string(species_count) + " species and " +
                     std::to_string(scalar_count) + " moment coefficients given, the file has " +
                     std::to_string(src.species_count) + " and " + std::to_string(src.alpha_scalar_count),
                 err, errlen);
    return MTP_ERR_ARG;
  }
  if (radial && (size_t) radial_count != src.radial_basis_coeffs.size()) {
    copy_message(who + ": " + std::to_string(radial_count) + " radial coefficients given, the file has " +
                     std::to_string(src.radial_basis_coeffs.size()),
                 err, errlen);
    return MTP_ERR_ARG;
  }
  bool finite = true;
  for (int i = 0; radial && i < radial_count; i++) finite = finite && std::isfinite(radial[i]);
  for (int i = 0; i < scalar_count; i++) finite = finite && std::isfinite(moment_coeffs[i]);
  for (int i = 0; species_coeffs && i < species_count; i++) finite = finite && std::isfinite(species_coeffs[i]);
  if (!finite) {
    copy_message(who + ": a coefficient is not finite", err, errlen);
    return MTP_ERR_ARG;
  }
  std::string text;
  {
    FILE *in = std::fopen(src_path, "rb");
    char chunk[65536];
    size_t got = 0;
    while (in && (got = std::fread(chunk, 1, sizeof chunk, in)) > 0) text.append(chunk, got);
    const bool bad = !in || std::ferror(in);
    if (in) std::fclose(in);
    if (bad) {
      copy_message(std::string("Cannot read potential file ") + src_path, err, errlen);
      return MTP_ERR_IO;
    }
  }
  // the last species_coeffs line, the moment_coeffs line behind it and, if there is one, the "#MVS_v1.1" line: the text
  // in front of the tail is kept byte for byte except for the two coefficient lines; the tail is left out
  size_t sp_b = std::string::npos, sp_e = 0, mo_b = std::string::npos, mo_e = 0, tail = std::string::npos;
  size_t ra_b = std::string::npos, ra_e = 0, am_b = std::string::npos;   // the radial_coeffs line, the alpha_moments_count line
  for (size_t b = 0; b < text.size();) {
    size_t e = text.find('\n', b);
    e = e == std::string::npos ? text.size() : e + 1;
    const std::string line = text.substr(b, e - b);
    if (mo_b != std::string::npos && first_word(line, false) == "#MVS_v1.1") {
      tail = b;
      break;
    }
    const std::string w = first_word(line, true);
    if (w == "radial_coeffs" && ra_b == std::string::npos) {
      ra_b = b;
      ra_e = e;
    } else if (w == "alpha_moments_count" && ra_b != std::string::npos && am_b == std::string::npos) {
      am_b = b;
    }
    if (w == "species_coeffs") {
      sp_b = b;
      sp_e = e;
      mo_b = std::string::npos;
    } else if (w == "moment_coeffs" && sp_b != std::string::npos) {
      mo_b = b;
      mo_e = e;
    }
    b = e;
  }
  if (sp_b == std::string::npos || mo_b == std::string::npos || mo_b < sp_e) {
    copy_message(who + ": species_coeffs / moment_coeffs lines not found", err, errlen);
    return MTP_ERR_PARSE;
  }
  auto eol_of = [&](size_t b, size_t e) {
    size_t k = e;
    while (k > b && (text[k - 1] == '\n' || text[k - 1] == '\r')) k--;
    return text.substr(k, e - k);
  };
  if (radial && (ra_b == std::string::npos || am_b == std::string::npos || am_b < ra_e || am_b > sp_b)) {
    copy_message(who + ": radial_coeffs / alpha_moments_count lines not found", err, errlen);
    return MTP_ERR_PARSE;
  }
  std::string out;
  if (radial) {
    // every t1-t2 pair in row-major order, Mu brace lines of R numbers each; indentation of the source's first pair line
    // and first brace line
    auto indent_of = [&](size_t b) {
      size_t k = b;
      while (k < text.size() && (text[k] == ' ' || text[k] == '\t')) k++;
      return text.substr(b, k - b);
    };
    const std::string eol = eol_of(ra_b, ra_e);
    const std::string ind1 = indent_of(ra_e);
    size_t l2 = text.find('\n', ra_e);
    const std::string ind2 = l2 != std::string::npos && l2 + 1 < am_b ? indent_of(l2 + 1) : ind1 + "\t";
    out = text.substr(0, ra_e);
    const int Sp = src.species_count, Mu = src.radial_func_count, R = src.radial_basis_size;
    char num[40];
    for (int t1 = 0; t1 < Sp; t1++)
      for (int t2 = 0; t2 < Sp; t2++) {
        out += ind1 + std::to_string(t1) + "-" + std::to_string(t2) + eol;
        for (int mu = 0; mu < Mu; mu++) {
          out += ind2 + "{";
          for (int ri = 0; ri < R; ri++) {
            std::snprintf(num, sizeof num, "%.16e", radial[((size_t) (t1 * Sp + t2) * Mu + mu) * R + ri]);
            if (ri) out += ", ";
            out += num;
          }
          out += "}" + eol;
        }
      }
    out += text.substr(am_b, sp_b - am_b);
  } else {
    out = text.substr(0, sp_b);
  }
  out += species_coeffs ? coeff_line("species_coeffs", species_coeffs, species_count, eol_of(sp_b, sp_e))
                        : text.substr(sp_b, sp_e - sp_b);
  out += text.substr(sp_e, mo_b - sp_e);
  out += coeff_line("moment_coeffs", moment_coeffs, scalar_count, eol_of(mo_b, mo_e));
  out += text.substr(mo_e, (tail == std::string::npos ? text.size() : tail) - mo_e);

  const std::string tmp = std::string(dst_path) + ".tmp" + std::to_string((long) getpid());
  FILE *fo = std::fopen(tmp.c_str(), "wb");
  if (!fo) {
    copy_message("Cannot open " + tmp + " for writing: " + std::strerror(errno), err, errlen);
    return MTP_ERR_IO;
  }
  bool ok = std::fwrite(out.data(), 1, out.size(), fo) == out.size();
  int why = ok ? 0 : errno;
  if (std::fclose(fo) != 0 && ok) {
    ok = false;
    why = errno;
  }
  if (ok) {
    // what a reader gets back: its line buffer is sized from the table (T * 32 + 20 characters), so a long coefficient line
    // of a very small table comes back in pieces -- such a file is refused, not written
    mtp_potential back;
    rc = mtp_parse_text_file(tmp.c_str(), false, back, msg);
    bool same = rc == MTP_OK && back.linear_coeffs.size() == (size_t) scalar_count &&
        std::memcmp(back.linear_coeffs.data(), moment_coeffs, sizeof(double) * (size_t) scalar_count) == 0 &&
        back.alpha_index_basic == src.alpha_index_basic && back.alpha_index_times == src.alpha_index_times &&
        back.alpha_moment_mapping == src.alpha_moment_mapping && back.alpha_moment_count == src.alpha_moment_count &&
        back.radial_basis_coeffs.size() == src.radial_basis_coeffs.size() &&
        std::memcmp(back.radial_basis_coeffs.data(), radial ? radial : src.radial_basis_coeffs.data(),
                    sizeof(double) * src.radial_basis_coeffs.size()) == 0;
    const std::vector<double> &want_sp = src.species_coeffs;
    if (same)
      same = back.species_coeffs.size() == want_sp.size() &&
          std::memcmp(back.species_coeffs.data(), species_coeffs ? species_coeffs : want_sp.data(),
                      sizeof(double) * want_sp.size()) == 0;
    if (!same) {
      std::remove(tmp.c_str());
      copy_message(who + ": the written coefficients do not read back (the reader's line buffer of " +
                       std::to_string((long) src.alpha_index_times_count * 32 + 20) +
                       " characters, sized from alpha_index_times_count, is shorter than a coefficient line)" +
                       (rc != MTP_OK ? ": " + msg : std::string()),
                   err, errlen);
      return MTP_ERR_LIMIT;
    }
  }
  if (ok && std::rename(tmp.c_str(), dst_path) != 0) {
    ok = false;
    why = errno;
  }
  if (!ok) {
    copy_message(std::string("Cannot write potential file ") + dst_path + ": " + std::strerror(why), err, errlen);
    std::remove(tmp.c_str());
    return MTP_ERR_IO;
  }
  return tail == std::string::npos ? MTP_OK : MTP_WROTE_WITHOUT_SELECTION;
}

int mtp_potential_write_coeffs(const char *src_path, const char *dst_path, const double *species_coeffs,
                               const double *moment_coeffs, int species_count, int scalar_count, char *err, int errlen)
{
  return write_coeffs_common("mtp_potential_write_coeffs", src_path, dst_path, nullptr, 0, species_coeffs, moment_coeffs,
                             species_count, scalar_count, err, errlen);
}

int mtp_potential_write_all_coeffs(const char *src_path, const char *dst_path, const double *radial_coeffs,
                                   const double *species_coeffs, const double *moment_coeffs, int radial_count, int species_count,
                                   int scalar_count, char *err, int errlen)
{
  return write_coeffs_common("mtp_potential_write_all_coeffs", src_path, dst_path, radial_coeffs, radial_count, species_coeffs,
                             moment_coeffs, species_count, scalar_count, err, errlen);
}

int mtp_potential_train_table(const mtp_potential *pot, int32_t *counts, int32_t *bymu, int32_t *mufirst, int32_t *refused,
                              char *err, int errlen)
{
  if (!pot) return MTP_ERR_ARG;
  mtp_train_table t;
  std::string msg;
  const int rc = mtp_build_train_table(*pot, t, msg);
  if (counts) {
    counts[0] = (int32_t) t.design.rows.size();
    counts[1] = t.design.nblocks;
    counts[2] = t.design.A;
    counts[3] = t.design.B;
    counts[4] = pot->radial_func_count;
    counts[5] = pot->species_count * pot->species_count * pot->radial_func_count * pot->radial_basis_size + pot->species_count +
        pot->alpha_scalar_count;
  }
  if (bymu) std::copy(t.bymu.begin(), t.bymu.end(), bymu);
  if (mufirst) std::copy(t.mufirst.begin(), t.mufirst.end(), mufirst);
  if (refused) {
    refused[0] = t.late_row;
    refused[1] = t.dup_scalar;
  }
  copy_message(msg, err, errlen);
  return rc;
}

int mtp_potential_coeff_tables(const mtp_potential *pot, const double *radial_coeffs, const double *species_coeffs,
                               const double *moment_coeffs, int32_t *counts, double *radial_out, double *species_out,
                               double *seed_val, double *e_lin, double *leaf_cf, double *leaf_cb)
{
  if (!pot) return MTP_ERR_ARG;
  bool finite = true;
  for (size_t i = 0; radial_coeffs && i < pot->radial_basis_coeffs.size(); i++) finite = finite && std::isfinite(radial_coeffs[i]);
  for (size_t i = 0; species_coeffs && i < pot->species_coeffs.size(); i++) finite = finite && std::isfinite(species_coeffs[i]);
  for (size_t i = 0; moment_coeffs && i < pot->linear_coeffs.size(); i++) finite = finite && std::isfinite(moment_coeffs[i]);
  if (!finite) return MTP_ERR_ARG;
  mtp_coeff_tables t;
  mtp_build_coeff_tables(*pot, radial_coeffs, species_coeffs, moment_coeffs, t);
  const std::vector<double> *v[6] = {&t.radial, &t.species, &t.seed_val, &t.e_lin, &t.leaf_cf, &t.leaf_cb};
  double *dst[6] = {radial_out, species_out, seed_val, e_lin, leaf_cf, leaf_cb};
  for (int k = 0; k < 6; k++) {
    if (counts) counts[k] = (int32_t) v[k]->size();
    if (dst[k] && !v[k]->empty()) std::memcpy(dst[k], v[k]->data(), v[k]->size() * sizeof(double));
  }
  return MTP_OK;
}

int mtp_potential_compatible(const mtp_potential *pot, const char *path, int want_selection, char *err, int errlen)
{
  if (!pot || !path) {
    copy_message("mtp_potential_compatible: null argument", err, errlen);
    return MTP_ERR_ARG;
  }
  mtp_potential other;
  std::string msg;
  int rc = mtp_parse_text_file(path, want_selection != 0, other, msg);
  if (rc == MTP_OK) rc = mtp_check_compatible(*pot, other, want_selection != 0, msg);
  copy_message(msg, err, errlen);
  return rc;
}

}   // extern "C"
