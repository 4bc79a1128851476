// Launch planner (internal, host only): the table blob, the per-atom LDS layout, the occupancy, the workgroup width and the
// grid of every force and grade launch, from the potential, the CU count and the size of the list.  Calls no HIP function
// and needs no device: mtp_plan.cpp builds with mtp_potential.cpp alone (tests/plan_dump.cpp).
#pragma once

#include <cstddef>
#include <vector>

#include "mtp_device.hpp"
#include "mtp_potential.hpp"

namespace mtp_plan {

constexpr size_t CU_LDS_BYTES = 160 * 1024;   // LDS of one CU: what the workgroups that share it may take together

constexpr const char *NO_FIT = "potential + neighbour list exceed one CU's LDS";   // the message of plan_launch's refusal

// LDS table blob: the pieces a launch plan may leave in HBM / L2 are its tail -- [core | adjoint scatter targets |
// basic descriptors (candidate-vector kernel) | packed times rows]; a plan copies one of these four prefixes
struct BlobSizes {
  int core = 0, tgt = 0, norows = 0, rows = 0;
};

struct Layout {   // per-atom LDS image, offsets in doubles (MtpDevParams: dg_mode, pow_row, dg_off, off_*)
  int mode = 0, pow_row = 0, dg_off = 0, fp_row = 0, off_m = 0, off_d = 0, off_coef = 0, off_nb = 0, m_doubles = 0;
};

struct LaunchPlan {
  Layout layout;
  int wpb = 1, grid = 1, wave_doubles = 0, tab_rows = 0, g_doubles = 0, m_doubles = 0, ov_doubles = 0;
  bool rebuild = false;
  int wps = 2;
  bool rows_lds = false, tgt_lds = true;
  int blob_bytes = 0;   // the blob prefix this plan copies
  size_t lds_bytes = 0;
};

// The tuning overrides (benchmarks and tests), one field per environment variable.  read_tuning() is their only reader and
// runs on EVERY planning call (tests set the variables after the library is loaded); the planner's steps take the struct.
struct PlanTuning {
  int wave_cap = 32;   // MTP_MAX_WAVES: wavefronts per CU, clamped to [1, 16] when set
  // MTP_LAYOUT = keep | nodg (lean) | rebuild | rebuild-nodg; any other word, or an ineligible layout, changes nothing
  enum LayoutPick { ANY, KEEP, NODG, REBUILD, REBUILD_NODG } layout = ANY;
  int wps = 0;               // MTP_WPS: 2 = never the 3-per-SIMD build, 3 = whenever it fits (also for few atoms); 0 (unset): by size
  bool grade_wps3 = true;    // MTP_GRADE_WPS3=0: the grade instantiation stays at 2 per SIMD
  int wpb = 0;               // MTP_WPB in [1, 8]: wavefronts per workgroup of the 2-per-SIMD plan (3 per SIMD ignores it); 0: planned
  // MTP_BLOB_PREFIX = core | tgt | norows | rows: plan against that prefix only; another word: against EACH.  Set to
  // anything, exactly the planned prefix is copied ("forced")
  enum Prefix { BEST, CORE, TGT, NOROWS, ROWS, EACH } prefix = BEST;
  bool rows_lds = true;   // MTP_ROWS_LDS=0: the packed times rows stay in HBM / L2
  int scalars_lds = -1;   // MTP_SCALARS_LDS: 0 / 1 = the scalar-side tables out of / in the blob whatever their size; -1: by size
};
PlanTuning read_tuning();

// The three plans of a list: [0] force calls (wavefront per atom), [1] candidate-vector kernel of grade calls, [2] the
// fused kernel's grade instantiation (its image also holds the leaf moments' values); also NT, cj_cap and d_doubles of
// `base`.  False (NO_FIT): one wavefront's image and the shortest blob prefix exceed a CU's LDS; plans already made stay.
bool plan_launch(const mtp_potential &p, const BlobSizes &bs, int num_cus, int inum, int max_numneigh, int variant,
                 LaunchPlan (&lp)[3], MtpDevParams &base);

struct RowRange {   // what a launch of `row_count` rows of the planned list runs with
  int wpb, grid;
  size_t lds_bytes;
};
RowRange plan_row_range(const LaunchPlan &L, int num_cus, int row_count);   // force / grade launch ([0], [2])
RowRange plan_cvec_range(const LaunchPlan &L, int row_count);               // candidate-vector kernel ([1])
// the part of a launch's argument block that its plan decides
void apply_plan(MtpDevParams &p, const LaunchPlan &L, const mtp_potential &pot, bool grade);
// the table blob every workgroup copies into LDS and its offsets in the argument block (the pointers of the HBM / L2
// copies are the context's business)
void build_blob(const mtp_potential &pot, const std::vector<MtpRow8> &rows8, const PlanTuning &tune, MtpDevParams &bb,
                BlobSizes &bs, std::vector<unsigned char> &blob);
// the sizes and counts of the potential's tables in the argument block
void fill_sizes(const mtp_potential &pot, MtpDevParams &b);
// packed rows (8 B each): moment ids in 16 bits, multiplicity in a signed 16 bits; nullptr, or the refusal of a wider one
const char *pack_rows(const std::vector<MtpRow> &rows, std::vector<MtpRow8> &out);
// the argument block of a force (or grade) launch as far as the potential and the plan decide it; pointers stay null
int plan_params(const mtp_potential *pot, int num_cus, int inum, int max_numneigh, int variant, int grade, MtpDevParams &p);

}   // namespace mtp_plan
