// TEST INFRASTRUCTURE ONLY -- C entry points around the REFERENCE's own pair styles (`mtp`, `mtp/extrapolation`),
// compiled unchanged from $(MTP_REFERENCE_DIR) by `make -C oracle ref` against the stand-in LAMMPS headers of
// tests/cpp/lammps_mock into oracle/_ref/libmtp_ref.so (git-ignored; nothing of the reference is committed).  This file
// is the project's own code: it builds the one-rank LAMMPS stand-in, hands the styles a caller's arrays and walks
// settings -> compute.  Protected members are reached through derived classes with using-declarations; the reference's
// headers are compiled as they are.  Loaded by oracle/pyref.py.
#include "pair_mtp_extrapolation.h"

#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "neigh_list.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace LAMMPS_NS;

namespace {

struct Open : PairMTPExtrapolation {
  using PairMTPExtrapolation::PairMTPExtrapolation;
  using PairMTP::alpha_index_basic_count;
  using PairMTP::alpha_index_times_count;
  using PairMTP::alpha_moment_count;
  using PairMTP::alpha_scalar_count;
  using PairMTP::max_alpha_index_basic;
  using PairMTP::max_cutoff;
  using PairMTP::min_cutoff;
  using PairMTP::potential_name;
  using PairMTP::potential_tag;
  using PairMTP::radial_basis;
  using PairMTP::radial_basis_size;
  using PairMTP::radial_func_count;
  using PairMTP::scaling;
  using PairMTP::species_count;
  using PairMTPExtrapolation::coeff_count;
  using PairMTPExtrapolation::configuration_mode;
  using PairMTPExtrapolation::energy_ders_wrt_coeffs;
  using PairMTPExtrapolation::max_grade;
  using PairMTPExtrapolation::mlip3_style;
  using PairMTPExtrapolation::nbh_count;
  using PairMTPExtrapolation::nbh_extrapolation_grades;
  using PairMTPExtrapolation::preselected_file;
  using PairMTPExtrapolation::write_config;
};

// the plain style's members, through the same route
struct OpenBase : PairMTP {
  using PairMTP::PairMTP;
  using PairMTP::alpha_index_basic_count;
  using PairMTP::alpha_index_times_count;
  using PairMTP::alpha_moment_count;
  using PairMTP::alpha_scalar_count;
  using PairMTP::max_alpha_index_basic;
  using PairMTP::max_cutoff;
  using PairMTP::min_cutoff;
  using PairMTP::radial_basis_size;
  using PairMTP::radial_func_count;
  using PairMTP::scaling;
  using PairMTP::species_count;
};

struct Handle {
  LAMMPS lmp;
  NeighList list;
  OpenBase *plain = nullptr;
  Open *ext = nullptr;
  bool cfg_open = false;   // MLIP-3 form: the preselected file is open
  Pair *pair() { return ext ? (Pair *) ext : (Pair *) plain; }
  ~Handle()
  {
    delete plain;
    delete ext;
    delete lmp.memory;
    delete lmp.error;
    delete lmp.atom;
    delete lmp.comm;
    delete lmp.force;
    delete lmp.domain;
    delete lmp.neighbor;
  }
};

void put(char *dst, int len, const std::string &s)
{
  if (!dst || len <= 0) return;
  std::snprintf(dst, (size_t) len, "%s", s.c_str());
}

// caller's CSR list and flat arrays as the Atom / NeighList members the styles read
struct Bound {
  std::vector<double *> x, f, vatom;
  std::vector<int> numneigh;
  std::vector<int *> firstneigh;
  void bind(Handle *h, Pair *p, int nall, int inum, const int *ilist, const int *first, const int *neigh, double *xx,
            const int *type, double *ff, double *eatom, double *va)
  {
    x.resize(nall + 1);
    f.resize(nall + 1);
    vatom.resize(nall + 1);
    for (int i = 0; i < nall; i++) {
      x[i] = xx + 3 * (size_t) i;
      f[i] = ff + 3 * (size_t) i;
      vatom[i] = va + 6 * (size_t) i;
    }
    numneigh.assign(nall + 1, 0);
    firstneigh.assign(nall + 1, nullptr);
    for (int ii = 0; ii < inum; ii++) {
      numneigh[ilist[ii]] = first[ii + 1] - first[ii];
      firstneigh[ilist[ii]] = const_cast<int *>(neigh) + first[ii];
    }
    Atom *a = h->lmp.atom;
    a->x = x.data();
    a->f = f.data();
    a->type = const_cast<int *>(type);
    a->nlocal = inum;
    a->nghost = nall - inum;
    h->list.inum = inum;
    h->list.ilist = const_cast<int *>(ilist);
    h->list.numneigh = numneigh.data();
    h->list.firstneigh = firstneigh.data();
    p->list = &h->list;
    // the caller's eatom / vatom ARE the style's per-atom arrays: ev_setup finds them large enough and zeroes what the
    // flags ask for, nothing else
    p->eatom = eatom;
    p->vatom = vatom.data();
    p->maxeatom = p->maxvatom = nall;
  }
  static void unbind(Pair *p)
  {
    p->eatom = nullptr;
    p->vatom = nullptr;
    p->maxeatom = p->maxvatom = 0;
    p->list = nullptr;
  }
};

}   // namespace

extern "C" {

// style 0: `pair_style mtp <file>`; 1: `pair_style mtp/extrapolation <file>`; 2: the MLIP-3 form
// `mtp/extrapolation <file> <cfg_out> <select> <break>`.  Returns a handle, or null with `err` filled.  `log` receives
// the utils::logmesg text of settings().
void *mtp_ref_open(int style, const char *file, const char *cfg_out, const char *select_thr, const char *break_thr,
                   char *log, int loglen, char *err, int errlen)
{
  std::unique_ptr<Handle> h(new Handle);
  h->lmp.quiet = true;
  put(err, errlen, "");
  if (FILE *fp = std::fopen(file, "r"))
    std::fclose(fp);
  else {
    put(err, errlen, std::string("cannot open potential file ") + file);
    return nullptr;
  }
  std::string a0(file), a1(cfg_out ? cfg_out : ""), a2(select_thr ? select_thr : ""), a3(break_thr ? break_thr : "");
  char *argv[4] = {&a0[0], &a1[0], &a2[0], &a3[0]};
  try {
    if (style == 0) {
      h->plain = new OpenBase(&h->lmp);
      h->plain->settings(1, argv);
    } else {
      h->ext = new Open(&h->lmp);
      int dim = 0;
      *(int *) h->ext->extract("extrapolation_flag", dim) = 0;   // (the style leaves it to `fix pair`)
      h->ext->settings(style == 2 ? 4 : 1, argv);
    }
  } catch (const std::exception &e) {
    put(err, errlen, e.what());
    put(log, loglen, h->lmp.log);
    // a style that threw inside read_file holds half-built tables: it is leaked, not destroyed
    h->plain = nullptr;
    h->ext = nullptr;
    return nullptr;
  }
  put(log, loglen, h->lmp.log);
  h->cfg_open = style == 2 && h->ext->preselected_file != nullptr;
  return h.release();
}

void mtp_ref_close(void *hv)
{
  Handle *h = (Handle *) hv;
  if (!h) return;
  // the style never closes its preselected file, except when the break threshold ends the run
  if (h->ext && h->cfg_open) std::fclose(h->ext->preselected_file);
  delete h;
}

// iv[10] = species_count, radial_basis_size, radial_func_count, alpha_moment_count, alpha_index_basic_count,
// alpha_index_times_count, alpha_scalar_count, max_alpha_index_basic, coeff_count, configuration_mode (the last two 0
// / -1 for the plain style); dv[3] = scaling, min_cutoff, max_cutoff
void mtp_ref_sizes(void *hv, int *iv, double *dv)
{
  Handle *h = (Handle *) hv;
  if (h->ext) {
    Open *p = h->ext;
    int v[10] = {p->species_count, p->radial_basis_size, p->radial_func_count, p->alpha_moment_count,
                 p->alpha_index_basic_count, p->alpha_index_times_count, p->alpha_scalar_count,
                 p->max_alpha_index_basic, p->coeff_count, p->configuration_mode};
    std::memcpy(iv, v, sizeof(v));
    dv[0] = p->scaling, dv[1] = p->min_cutoff, dv[2] = p->max_cutoff;
  } else {
    OpenBase *p = h->plain;
    int v[10] = {p->species_count, p->radial_basis_size, p->radial_func_count, p->alpha_moment_count,
                 p->alpha_index_basic_count, p->alpha_index_times_count, p->alpha_scalar_count,
                 p->max_alpha_index_basic, 0, -1};
    std::memcpy(iv, v, sizeof(v));
    dv[0] = p->scaling, dv[1] = p->min_cutoff, dv[2] = p->max_cutoff;
  }
}

double mtp_ref_init_one(void *hv, int i, int j, char *err, int errlen)
{
  Handle *h = (Handle *) hv;
  try {
    return h->pair()->init_one(i, j);
  } catch (const std::exception &e) {
    put(err, errlen, e.what());
    return -1.0;
  }
}

// extract("extrapolation_flag"): 1 when the style hands out a pointer (and sets it to `value`), else 0
int mtp_ref_set_extrapolation_flag(void *hv, int value)
{
  Handle *h = (Handle *) hv;
  int dim = -1;
  void *p = h->pair()->extract("extrapolation_flag", dim);
  if (!p) return 0;
  *(int *) p = value;
  return 1;
}

// extract_peratom("extrapolation"): 0 and ncol, 1 when the style knows no such array, -1 with `err` when it raises
int mtp_ref_extract_peratom(void *hv, int *ncol, char *err, int errlen)
{
  Handle *h = (Handle *) hv;
  try {
    *ncol = -1;
    void *p = h->pair()->extract_peratom("extrapolation", *ncol);
    (void) p;
    return h->ext ? 0 : 1;
  } catch (const std::exception &e) {
    put(err, errlen, e.what());
    return -1;
  }
}

// One compute(eflag, vflag) on the caller's arrays.  f accumulates; *energy, virial[6], eatom[nall], vatom[nall][6]
// are handed to the style holding what the caller put there (it zeroes what it will tally: Pair::ev_setup).  Grade
// outputs (extrapolation styles with the flag set, or MLIP-3 form): grades[nall] -- the style keeps inum of them,
// indexed by atom, so only ilist entries below inum are copied out --, *max_grade = pvector[0], coeff_ders[C] the
// candidate vector as the last neighbourhood (neighbourhood mode) or the call (configuration mode) left it.
// domain6 = xprd yprd zprd xy xz yz (may be null).  Returns 0, or -1 with `err` when the style raised.
int mtp_ref_compute(void *hv, int nall, int inum, const int *ilist, const int *first, const int *neigh, double *x,
                    const int *type, int eflag, int vflag, long natoms, const double *domain6, double *f,
                    double *energy, double *eatom, double *virial, double *vatom, double *grades, double *max_grade,
                    double *coeff_ders, char *log, int loglen, char *err, int errlen)
{
  Handle *h = (Handle *) hv;
  Pair *p = h->pair();
  // the style keeps inum grades and writes them by ATOM index (nbh_extrapolation_grades[i]): a list that names an atom
  // at or beyond inum would make it write past its array, so such a call is refused here, not run
  int dim = 0;
  if (h->ext && !h->ext->configuration_mode && (h->ext->mlip3_style || *(int *) h->ext->extract("extrapolation_flag", dim)))
    for (int ii = 0; ii < inum; ii++)
      if (ilist[ii] >= inum) {
        put(err, errlen, "refused: neighbourhood-mode grades of a list that names atoms at or beyond inum");
        return -2;
      }
  Bound b;
  b.bind(h, p, nall, inum, ilist, first, neigh, x, type, f, eatom, vatom);
  h->lmp.atom->natoms = natoms;
  if (domain6) {
    Domain *d = h->lmp.domain;
    d->xprd = domain6[0], d->yprd = domain6[1], d->zprd = domain6[2];
    d->xy = domain6[3], d->xz = domain6[4], d->yz = domain6[5];
  }
  p->eng_vdwl = *energy;
  for (int q = 0; q < 6; q++) p->virial[q] = virial[q];
  h->lmp.log.clear();
  int rc = 0;
  try {
    p->compute(eflag, vflag);
  } catch (const std::exception &e) {
    put(err, errlen, e.what());
    rc = -1;
    if (std::strstr(e.what(), "Exceeded Break Threshold")) h->cfg_open = false;   // (closed by evaluate_grades)
  }
  if (h->cfg_open) std::fflush(h->ext->preselected_file);
  put(log, loglen, h->lmp.log);
  *energy = p->eng_vdwl;
  for (int q = 0; q < 6; q++) virial[q] = p->virial[q];
  if (h->ext) {
    Open *e = h->ext;
    if (max_grade) *max_grade = e->pvector[0];
    if (grades && !e->configuration_mode && e->nbh_extrapolation_grades)
      for (int ii = 0; ii < inum; ii++)
        if (ilist[ii] < e->nbh_count) grades[ilist[ii]] = e->nbh_extrapolation_grades[ilist[ii]];
    if (coeff_ders) std::memcpy(coeff_ders, e->energy_ders_wrt_coeffs, sizeof(double) * (size_t) e->coeff_count);
  }
  Bound::unbind(p);
  return rc;
}

// write_config() on prescribed grades (MLIP-3 form handles only): one record of `inum` atoms appended to the handle's
// preselected file, which is flushed.  Returns 0, -1 when the handle has no such file.
int mtp_ref_write_config(void *hv, int inum, double *x, const int *type, const double *grades, double max_grade,
                         long natoms, const double *domain6)
{
  Handle *h = (Handle *) hv;
  Open *e = h->ext;
  if (!e || !h->cfg_open) return -1;
  std::vector<double *> rows(inum + 1);
  for (int i = 0; i < inum; i++) rows[i] = x + 3 * (size_t) i;
  Atom *a = h->lmp.atom;
  a->x = rows.data();
  a->type = const_cast<int *>(type);
  a->nlocal = inum;
  a->natoms = natoms;
  Domain *d = h->lmp.domain;
  d->xprd = domain6[0], d->yprd = domain6[1], d->zprd = domain6[2];
  d->xy = domain6[3], d->xz = domain6[4], d->yz = domain6[5];
  h->list.inum = inum;
  e->list = &h->list;
  if (!e->configuration_mode) {
    if (e->nbh_count < inum) {
      h->lmp.memory->grow(e->nbh_extrapolation_grades, inum, "nbh_extrapolation_grades");
      e->nbh_count = inum;
    }
    for (int i = 0; i < inum; i++) e->nbh_extrapolation_grades[i] = grades[i];
  }
  e->max_grade = max_grade;
  e->write_config();
  std::fflush(e->preselected_file);
  e->list = nullptr;
  a->x = nullptr;
  a->type = nullptr;
  return 0;
}

}   // extern "C"
