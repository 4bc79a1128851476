// Everything the launch planner decides (csrc/mtp_plan.hpp), printed without a device: tests/test_plan_cpu.py compares the
// lines with tests/golden/plan_parent.txt, which the planner of commit 78152b6 wrote for the same input.
//
//   plan_dump LIST [DIR ...]
//
// Every line of LIST is `potential num_cus inum max_numneigh variant row_count [NAME=value ...]`: the potential (looked up
// in each DIR, loaded once) is planned for a list of inum rows whose longest holds max_numneigh entries, with the NAME=value
// pairs in the environment of that line alone, and a launch of row_count rows is asked for.  One output line per input
// line, in the columns the first output line names; arrays are written as runs, value*count.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../include/mtp_mi355x.h"
#include "../lammps_mtp_kokkos_amd/csrc/mtp_plan.hpp"
#include "../lammps_mtp_kokkos_amd/csrc/mtp_shape_fields.hpp"

using namespace mtp_plan;

struct Answer {
  int rc[2] = {0, 0};   // of the force and of the grade argument block
  LaunchPlan lp[3];
  MtpDevParams block[2] = {};
  RowRange range[2] = {}, cvec = {};
};

static void ask(const mtp_potential &pot, int num_cus, int inum, int max_numneigh, int variant, int row_count, Answer &a)
{
  for (int g = 0; g < 2; g++) a.rc[g] = plan_params(&pot, num_cus, inum, max_numneigh, variant, g, a.block[g]);
  MtpDevParams base{};
  const std::vector<MtpRow8> rows8(pot.rows_by_level.size());
  BlobSizes bs;
  std::vector<unsigned char> blob;
  build_blob(pot, rows8, read_tuning(), base, bs, blob);
  (void) plan_launch(pot, bs, num_cus, inum, max_numneigh, variant, a.lp, base);
  a.range[0] = plan_row_range(a.lp[0], num_cus, row_count);
  a.range[1] = plan_row_range(a.lp[2], num_cus, row_count);
  a.cvec = plan_cvec_range(a.lp[1], row_count);
}

// ---- input, environment and output ------------------------------------------------------------------------------------
static const char *HEADER =
    "# rc_force rc_grade | lp[0..2]: mode pow_row dg_off fp_row off_m off_d off_coef off_nb layout.m_doubles wpb grid wave_doubles "
    "tab_rows g_doubles m_doubles ov_doubles rebuild wps rows_lds tgt_lds blob_bytes lds_bytes | force, grade block: the "
    "MTP_SHAPE_INT_FIELDS, MTP_SHAPE_ARR_FIELDS and MTP_SHAPE_TAB_FIELDS of mtp_shape_fields.hpp in their order, then wps "
    "wave_doubles NT cj_cap rebuild_tables | row range of the force, of the grade launch: wpb grid lds_bytes | of the "
    "candidate-vector kernel: wpb grid lds_bytes";

template <class T> static void put_runs(std::string &s, const T *v, int n)
{
  for (int k = 0; k < n;) {
    int m = 1;
    while (k + m < n && v[k + m] == v[k]) m++;
    s += " " + std::to_string((int) v[k]);
    if (m > 1) s += "*" + std::to_string(m);
    k += m;
  }
}

static std::string line_of(const Answer &a)
{
  std::string s = std::to_string(a.rc[0]) + " " + std::to_string(a.rc[1]);
  auto put = [&](long long v) { s += " " + std::to_string(v); };
  for (const LaunchPlan &L : a.lp) {
    s += " |";
    const Layout &y = L.layout;
    for (int v : {y.mode, y.pow_row, y.dg_off, y.fp_row, y.off_m, y.off_d, y.off_coef, y.off_nb, y.m_doubles, L.wpb, L.grid,
                  L.wave_doubles, L.tab_rows, L.g_doubles, L.m_doubles, L.ov_doubles, (int) L.rebuild, L.wps, (int) L.rows_lds,
                  (int) L.tgt_lds, L.blob_bytes})
      put(v);
    put((long long) L.lds_bytes);
  }
  for (const MtpDevParams &p : a.block) {
    s += " |";
#define MTP_X(f) put(p.f);
    MTP_SHAPE_INT_FIELDS(MTP_X)
#undef MTP_X
#define MTP_X(f) put_runs(s, p.f, MTP_SHAPE_ARR_LEN);
    MTP_SHAPE_ARR_FIELDS(MTP_X)
#undef MTP_X
#define MTP_X(f) put_runs(s, p.f, MTP_SHAPE_TAB_LEN);
    MTP_SHAPE_TAB_FIELDS(MTP_X)
#undef MTP_X
    for (int v : {p.wps, p.wave_doubles, p.NT, p.cj_cap, p.rebuild_tables}) put(v);
  }
  for (const RowRange &r : {a.range[0], a.range[1], a.cvec}) {
    s += " |";
    put(r.wpb);
    put(r.grid);
    put((long long) r.lds_bytes);
  }
  return s;
}

int main(int argc, char **argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: plan_dump LIST [DIR ...]\n");
    return 2;
  }
  std::ifstream list(argv[1]);
  if (!list) {
    std::fprintf(stderr, "plan_dump: cannot read %s\n", argv[1]);
    return 2;
  }
  std::map<std::string, std::unique_ptr<mtp_potential>> loaded;
  std::puts(HEADER);
  std::string text;
  for (int lineno = 1; std::getline(list, text); lineno++) {
    if (text.empty() || text[0] == '#') continue;
    std::istringstream in(text);
    std::string name, pair;
    int num_cus = 0, inum = 0, max_numneigh = 0, variant = 0, row_count = 0;
    if (!(in >> name >> num_cus >> inum >> max_numneigh >> variant >> row_count)) {
      std::fprintf(stderr, "plan_dump: %s:%d: six fields expected\n", argv[1], lineno);
      return 2;
    }
    std::unique_ptr<mtp_potential> &pot = loaded[name];
    for (int d = 2; !pot && d <= argc; d++) {   // (after the DIRs, the name as it stands)
      const std::string path = d < argc ? std::string(argv[d]) + "/" + name : name;
      if (!std::ifstream(path)) continue;
      pot.reset(new mtp_potential());
      std::string msg;
      if (mtp_parse_file(path.c_str(), false, *pot, msg) != MTP_OK) {
        std::fprintf(stderr, "plan_dump: %s: %s\n", path.c_str(), msg.c_str());
        return 2;
      }
    }
    if (!pot) {
      std::fprintf(stderr, "plan_dump: %s:%d: potential %s not found\n", argv[1], lineno, name.c_str());
      return 2;
    }
    std::vector<std::string> set;
    while (in >> pair) {
      const size_t eq = pair.find('=');
      if (eq == std::string::npos || eq == 0) {
        std::fprintf(stderr, "plan_dump: %s:%d: NAME=value expected, got %s\n", argv[1], lineno, pair.c_str());
        return 2;
      }
      set.push_back(pair.substr(0, eq));
      setenv(set.back().c_str(), pair.c_str() + eq + 1, 1);
    }
    Answer a;
    ask(*pot, num_cus, inum, max_numneigh, variant, row_count, a);
    std::puts(line_of(a).c_str());
    for (const std::string &n : set) unsetenv(n.c_str());
  }
  return 0;
}
