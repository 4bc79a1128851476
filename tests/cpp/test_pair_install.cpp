// Driver for the install route of the C++ host mirror (lammps_mtp_kokkos_amd/host): pair_style re-issued on a mirror
// that already runs.  The sequence is settings -> init_style -> compute -> settings with a retrained file of the same
// structure -> compute, WITHOUT a new neighbour list in between; then a file of another structure, which must take the
// full load.  tests/test_install_gpu.py writes the system and the files and judges the numbers.
//
//   test_pair_install plain <system> <out> <file> <retrained file> <incompatible file>
//   test_pair_install ext   <system> <out> <file> <file with a new active set> <incompatible file>
//
// <out>: line 1 "same_context installs context_after_incompatible installs_after_incompatible computed_without_a_list
// pvector[0]_before", then for the installed mirror and for a mirror freshly constructed on the second file: energy, six
// virial components and pvector[0] on one line, and nall lines fx fy fz eatom and the six per-atom virial components.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../lammps_mtp_kokkos_amd/host/pair_mtp_mi355x.hpp"

using namespace mtp_mi355x;

struct System {
  int nlocal = 0, nall = 0;
  std::vector<double> x, f;
  std::vector<int> type, ilist, numneigh;
  std::vector<std::vector<int>> rows;
  std::vector<const int *> firstneigh;
  double box[3] = {0, 0, 0};
  void read(const char *path)
  {
    std::ifstream in(path);
    if (!in) throw std::runtime_error(std::string("cannot open ") + path);
    in >> nlocal >> nall >> box[0] >> box[1] >> box[2];
    x.resize(3 * (size_t) nall);
    type.resize((size_t) nall);
    for (int i = 0; i < nall; i++) in >> x[3 * i] >> x[3 * i + 1] >> x[3 * i + 2] >> type[i];
    numneigh.assign((size_t) nall, 0);
    rows.assign((size_t) nall, {});
    for (int i = 0; i < nlocal; i++) {
      int n;
      in >> n;
      numneigh[i] = n;
      rows[i].resize((size_t) n);
      for (int k = 0; k < n; k++) in >> rows[i][k];
      ilist.push_back(i);
    }
    firstneigh.resize((size_t) nall);
    for (int i = 0; i < nall; i++) firstneigh[i] = rows[i].data();
    f.assign(3 * (size_t) nall, 0.0);
  }
};

struct Snapshot {   // what LAMMPS reads back after a step
  double e = 0, virial[6] = {0, 0, 0, 0, 0, 0}, pv = 0;
  std::vector<double> f, eatom, vatom;
  void write(std::ofstream &out, int nall) const
  {
    out << e;
    for (int q = 0; q < 6; q++) out << " " << virial[q];
    out << " " << pv << "\n";
    for (int i = 0; i < nall; i++) {
      out << f[3 * i] << " " << f[3 * i + 1] << " " << f[3 * i + 2] << " " << eatom[i];
      for (int q = 0; q < 6; q++) out << " " << vatom[6 * (size_t) i + q];
      out << "\n";
    }
  }
};

static double pvector0(PairMTP &) { return 0.0; }
static double pvector0(PairMTPExtrapolation &p) { return p.pvector[0]; }
static void grade_every_step(PairMTP &) {}
static void grade_every_step(PairMTPExtrapolation &p)
{
  int dim = 0;
  *(int *) p.extract("extrapolation_flag", dim) = 1;   // what `fix pair` does
}

template <class P> static Snapshot step(P &p, System &s)
{
  std::fill(s.f.begin(), s.f.end(), 0.0);
  p.compute(3, 4);
  Snapshot r;
  r.e = p.eng_vdwl;
  std::copy(p.virial, p.virial + 6, r.virial);
  r.pv = pvector0(p);
  r.f = s.f;
  r.eatom = p.eatom;
  r.vatom = p.vatom;
  return r;
}

template <class P> static int run(System &s, const char *outpath, char *file, char *retrained, char *incompatible)
{
  AtomView av;
  av.x = s.x.data();
  av.f = s.f.data();
  av.type = s.type.data();
  av.nlocal = s.nlocal;
  av.nall = s.nall;
  av.natoms = s.nlocal;
  NeighListView lv{s.nlocal, s.ilist.data(), s.numneigh.data(), s.firstneigh.data()};
  char star[] = "*";
  char *cf[2] = {star, star};
  auto start = [&](P &p, char *path) {   // the call sequence of a first `run`
    char *a[1] = {path};
    p.settings(1, a);
    p.coeff(2, cf);
    p.init_style(1);
    p.bind(av);
    p.set_neighbor_list(lv);
    grade_every_step(p);
  };
  P p;
  start(p, file);
  const Snapshot before = step(p, s);
  const mtp_context *ctx0 = p.context();
  // the retrained file: installed, and the next step runs on the list and the plan that are there
  char *a2[1] = {retrained};
  p.settings(1, a2);
  const int installs = p.installs();
  p.init_style(1);   // (LAMMPS calls it before the next run: the context is kept)
  const int same = ctx0 != nullptr && p.context() == ctx0;
  const Snapshot installed = step(p, s);
  // a mirror freshly constructed on that file
  P q;
  start(q, retrained);
  const Snapshot fresh = step(q, s);
  // another structure: the full load -- no context until init_style, and a step needs a list again
  char *a3[1] = {incompatible};
  p.settings(1, a3);
  const int ctx_after = p.context() != nullptr, installs_after = p.installs();
  p.init_style(1);
  int computed = 0;
  try {
    p.compute(3, 4);
    computed = 1;
  } catch (const Error &) {
  }
  std::ofstream out(outpath);
  out.precision(17);
  out << same << " " << installs << " " << ctx_after << " " << installs_after << " " << computed << " " << before.pv << "\n";
  installed.write(out, s.nall);
  fresh.write(out, s.nall);
  return 0;
}

int main(int argc, char **argv)
{
  try {
    if (argc < 7) {
      std::fprintf(stderr, "usage: see the header of this file\n");
      return 2;
    }
    System s;
    s.read(argv[2]);
    if (!std::strcmp(argv[1], "ext")) return run<PairMTPExtrapolation>(s, argv[3], argv[4], argv[5], argv[6]);
    return run<PairMTP>(s, argv[3], argv[4], argv[5], argv[6]);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "ERROR: %s\n", e.what());
    return 1;
  }
}
