// Launch planner (mtp_plan.hpp): host only, no HIP call.  Choose the workgroup shape from the LDS budget (160 KiB / CU):
// every workgroup carries one copy of the table blob plus one private region per wavefront.  Grade calls need extra table
// rows (r^-nu, Q_ri) and scratch, so they get their own plan.  The steps, in the order plan_one takes them:
// candidate_layouts, (waves2 / best2 / shape3), choose_layout, choose_width, choose_prefix.
#include "mtp_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/mtp_mi355x.h"
#include "mtp_shape_fields.hpp"

// ---- lane grids and register builds of the kernels (declared in mtp_device.hpp) ---------------------------------------
// Lane grids of the candidate-vector kernel (KL k-lanes x KB basics per lane); also sizes dbasic rows.
int mtp_pick_shape(int B, int *KL, int *KB)
{
  static const int kb16[] = {2, 3, 5, 7, 9, 10}, kbw[] = {6, 7, 8, 10};
  for (int v : kb16)
    if (B <= 16 * v) {
      *KL = 16;
      *KB = v;
      return 0;
    }
  for (int kl : {32, 64})
    for (int v : kbw)
      if (B <= kl * v) {
        *KL = kl;
        *KB = v;
        return 0;
      }
  return -1;
}

// Lane grids of the force kernel's basic-moment pass: KL block lanes x NB 3x3 blocks per lane (KL * NB >= blocks);
// mtp_pick_fwd_shape() is the single source of truth for the host.
int mtp_pick_fwd_shape(int nblk, int *KL, int *NB)
{
  for (int kl : {16, 32, 64})
    if (nblk <= kl) {
      *KL = kl;
      *NB = 1;
      return 0;
    }
  for (int nb : {2, 3, 4})
    if (nblk <= 64 * nb) {
      *KL = 64;
      *NB = nb;
      return 0;
    }
  return -1;
}

// whether the three-wavefronts-per-SIMD build exists for this table shape (mtp_kernels.hip, launch_pitch)
bool mtp_wave_kernel_has_wps3(int nfb, int P)
{
  int KL = 0, NB = 0;
  return mtp_pick_fwd_shape(nfb, &KL, &NB) == 0 && KL <= 32 && NB == 1 && mtp_wave_kernel_deg(KL, P) == mtp_wave_kernel_dlow(KL);
}

namespace mtp_plan {

PlanTuning read_tuning()
{
  PlanTuning t;
  auto num = [](const char *name, int &v) {
    const char *e = std::getenv(name);
    if (e) v = std::atoi(e);
    return e != nullptr;
  };
  int v = 0;
  if (num("MTP_MAX_WAVES", v)) t.wave_cap = std::max(1, std::min(16, v));
  if (const char *e = std::getenv("MTP_LAYOUT")) {
    const std::string s(e);
    t.layout = s == "keep" ? PlanTuning::KEEP : s == "nodg" || s == "lean" ? PlanTuning::NODG : s == "rebuild" ? PlanTuning::REBUILD
        : s == "rebuild-nodg" ? PlanTuning::REBUILD_NODG : PlanTuning::ANY;
  }
  if (num("MTP_WPS", v)) t.wps = v == 3 ? 3 : 2;
  if (num("MTP_GRADE_WPS3", v)) t.grade_wps3 = v != 0;
  if (num("MTP_WPB", v) && v >= 1 && v <= 8) t.wpb = v;
  if (const char *e = std::getenv("MTP_BLOB_PREFIX")) {
    const std::string s(e);
    t.prefix = s == "core" ? PlanTuning::CORE : s == "tgt" ? PlanTuning::TGT : s == "norows" ? PlanTuning::NOROWS
        : s == "rows" ? PlanTuning::ROWS : PlanTuning::EACH;
  }
  if (num("MTP_ROWS_LDS", v)) t.rows_lds = v != 0;
  if (num("MTP_SCALARS_LDS", v)) t.scalars_lds = v != 0;
  return t;
}

namespace {

constexpr int NT = 32;   // neighbours per LDS tile

struct Candidate {
  Layout layout;
  bool ok = false;
  size_t wave_bytes = 0;   // one wavefront's image, the neighbour arrays behind the tables included
};

// Layouts.  The four layouts of the per-atom LDS image (mtp_wave_body.hpp, WaveLds), sizes in doubles, with their
// eligibility and their bytes per wavefront, in the order of preference at equal occupancy: nodg (least work), keep,
// then the rebuilding ones.  Leaf moments have no LDS slot in force calls; grade calls keep their values (candidate
// vector), not their adjoints.  (The force phase reads its coefficient blocks 16 at a time, up to 15 doubles past the last
// block: every layout keeps off_coef + coef_total <= off_nb, and the neighbour arrays behind off_nb are longer than that,
// so those reads stay inside the wave's image without slack.)
void candidate_layouts(const mtp_potential &p, int cap, bool grade, Candidate (&c)[4])
{
  const int A = p.alpha_moment_count, P = p.max_alpha_index_basic, Mu = p.radial_func_count;
  const int d_doubles = p.stored_moment_count, Am = grade ? A : p.stored_moment_count;
  const int grows = p.slot_count * MTP_PITCH;   // g rows; the dg rows take as much again
  const int trows = 2 * grows;
  // (a Layout below: {mode, pow_row, dg_off, fp_row, off_m, off_d, off_coef, off_nb, m_doubles})
  //   keep     [g rows | dg rows | overlay]; coordinate-power rows and moments / adjoints share the overlay
  //            (never live together); the derivative-polynomial coefficients later take the moments' place
  const int m_keep = std::max(std::max(Am, p.coef_total), 16), ov_keep = std::max(3 * P * MTP_PITCH, d_doubles + m_keep);
  const Layout keep{0, 2 * p.slot_count, grows, 0, trows, trows + m_keep, trows, trows + ov_keep, m_keep};
  //   nodg     [g rows | overlay] (Mu <= 4): no dg rows; Mu rows f'_mu (written ahead of the force phase from radial
  //            derivatives the tile build parked in registers) sit behind the coefficient blocks: 11.7 instead of
  //            15.7 KB per atom at level 16, and neither the 16 dg rows nor a second evaluation of the radial functions
  const bool nodg_ok = Mu <= 4;
  const int fp_row = (grows + p.coef_total + MTP_PITCH - 1) / MTP_PITCH, fp_end = (fp_row + Mu) * MTP_PITCH;
  const Layout lean{1, p.slot_count, 0, fp_row, grows, grows + m_keep, grows, std::max(grows + ov_keep, fp_end), m_keep};
  //   rebuild  everything overlays everything (many moments): first table build = g rows and power rows only;
  //            moments and adjoints then take the front of the region; ahead of the force phase the g and dg rows
  //            are built again (coefficient blocks behind them, D[0, B) in front).  One more pass over the
  //            neighbours' radial functions buys LDS: level 20 goes from 37 to 24 KB per atom.
  const int m_reb = std::max(Am, 16), pow_end = grows + 3 * P * MTP_PITCH;
  const Layout reb{2, p.slot_count, grows, 0, d_doubles, 0, trows, std::max(std::max(pow_end, trows + p.coef_total), d_doubles + m_reb),
                   m_reb};
  //   rebuild without dg rows (Mu <= 4): the second build writes the g rows only, the f' rows follow the coefficients
  const Layout rebn{3, p.slot_count, 0, fp_row, d_doubles, 0, grows, std::max(std::max(pow_end, fp_end), d_doubles + m_reb), m_reb};
  const Layout *ys[4] = {&lean, &keep, &rebn, &reb};
  const bool oks[4] = {nodg_ok, true, nodg_ok && grows >= p.alpha_index_basic_count, trows >= p.alpha_index_basic_count};
  const size_t tail = 5 * (size_t) NT * 8 + ((size_t) 2 * NT + cap) * 4;   // neighbour arrays behind the tables
  for (int k = 0; k < 4; k++) {
    c[k].layout = *ys[k];
    c[k].ok = oks[k];
    c[k].wave_bytes = ((size_t) ys[k]->off_nb * 8 + tail + 15) / 16 * 16;
  }
}

// Occupancy.  Wavefronts per CU that workgroups of w wavefronts of wbytes each reach beside one copy of `blob`.
// Registers: 8 wavefronts per CU (2 per SIMD at <= 256 VGPRs) in workgroups of up to 8, or -- for the table shapes that
// have the 168-VGPR build -- 12 (3 per SIMD).  Measured on MI355X: a workgroup is only admitted when every SIMD it lands
// on has room, and workgroups of 5..7 wavefronts load the SIMDs unevenly (two 6-wavefront workgroups never shared a CU at
// 3 per SIMD); so the 3-per-SIMD plan uses one workgroup of 12 or three of 4.
struct Budget {
  size_t blob;    // the blob prefix every workgroup copies
  int wave_cap;   // PlanTuning::wave_cap
};
int waves2(const Budget &b, int w, size_t wbytes)   // 2-per-SIMD build, w wavefronts per workgroup
{
  const size_t blk = b.blob + w * wbytes;
  if (w > 8 || blk > CU_LDS_BYTES) return 0;
  return std::min<int>(std::min(b.wave_cap, 8), (int) (CU_LDS_BYTES / blk) * w);
}
int best2(const Budget &b, size_t wbytes)
{
  int v = 0;
  for (int w = 1; w <= 8; w++) v = std::max(v, waves2(b, w, wbytes));
  return v;
}
int shape3(const Budget &b, size_t wbytes)   // 3-per-SIMD build: wavefronts per workgroup that reach 12 per CU, or 0
{
  if (b.wave_cap < 12) return 0;
  if (b.blob + 12 * wbytes <= CU_LDS_BYTES) return 12;
  if (3 * (b.blob + 4 * wbytes) <= CU_LDS_BYTES) return 4;
  return 0;
}

// Whether the plan may take the 3-per-SIMD build.  It pays when there are atoms enough to fill twelve wavefronts per CU
// (slots: the 3-per-SIMD build keeps mu of every slot in one SGPR pair, two bits each; Mu <= 4 and ranks <= 6 give 28).
// (The grade instantiation spilled 52 dwords at 168 VGPRs and was 2.6 % slower there until the force totals were reduced
// per tile: 35 now, and 12 wavefronts per CU make the grade call 8 % faster; MTP_GRADE_WPS3=0 turns it off.)
bool may_wps3(const mtp_potential &p, const PlanTuning &t, bool fine, bool grade)
{
  const bool has3 = mtp_wave_kernel_has_wps3(p.fwd_block_count, p.max_alpha_index_basic) && p.slot_count <= 32;
  return has3 && (t.wps ? t.wps == 3 : !fine) && (!grade || t.grade_wps3);
}

// Layout choice.  The first candidate, in their order of preference, that reaches the most wavefronts per CU, and the
// register build it reaches them with (the 3-per-SIMD build carries the dg-free force phase only).  MTP_LAYOUT narrows
// the candidates to one when that one is eligible.  pick == nullptr: nothing fits.
struct Choice {
  const Candidate *pick = nullptr;
  int wps = 2, w3 = 0;   // w3: wavefronts per workgroup of the 3-per-SIMD plan
};
Choice choose_layout(const Candidate (&c)[4], const PlanTuning &t, const Budget &b, bool has3)
{
  const Candidate &lean = c[0], &keep = c[1], &rebn = c[2], &reb = c[3];
  const Candidate *only = nullptr;
  if (t.layout == PlanTuning::KEEP) only = &keep;
  else if (t.layout == PlanTuning::NODG && lean.ok) only = &lean;
  else if (t.layout == PlanTuning::REBUILD && reb.ok) only = &reb;
  else if ((t.layout == PlanTuning::REBUILD_NODG || t.layout == PlanTuning::REBUILD) && rebn.ok) only = &rebn;
  Choice ch;
  int pick_waves = 0;
  for (const Candidate &y : c) {
    if (only ? &y != only : !y.ok) continue;
    int v = best2(b, y.wave_bytes), vw3 = 0;
    if (has3 && (y.layout.mode & 1) && (vw3 = shape3(b, y.wave_bytes)) > 0) v = 12;
    if (v > pick_waves) {
      pick_waves = v;
      ch.pick = &y;
      ch.wps = vw3 > 0 ? 3 : 2;
      ch.w3 = vw3;
    }
  }
  return ch;
}

// Workgroup width of the 2-per-SIMD plan (0: nothing fits).  Few atoms (`fine`: fewer than 16 per CU, or the "small"
// variant): the finest spread that still reaches the best occupancy; many atoms: as many wavefronts per workgroup as
// possible (fewer copies of the table blob).  MTP_WPB (benchmarks only) replaces the result by any width that fits.
int choose_width(const Budget &b, const PlanTuning &t, size_t wb, bool fine, int num_cus, int inum)
{
  int best_w = 0, best = 0;
  for (int w = 1; w <= 8; w++) {
    const int v = waves2(b, w, wb);
    if (v > best || (v == best && v > 0 && !fine)) {
      best = v;
      best_w = w;
    }
  }
  if (best == 0) return 0;
  if (fine) {
    // ... every atom its own wavefront, in the WIDEST workgroups that still leave no CU without one (fewer copies of
    // the table blob, fewer workgroups to dispatch: 2,048 atoms in 256 workgroups of 8 wavefronts run 3 % faster than
    // in 1,024 of 2); narrower only when the atoms would not cover the CUs
    int pick_w = 0;
    for (int w = 1; w <= 8; w++)
      if (waves2(b, w, wb) > 0 && (long long) num_cus * waves2(b, w, wb) >= inum && (inum + w - 1) / w >= num_cus) pick_w = w;
    if (pick_w == 0)
      for (int w = 1; w < best_w && pick_w == 0; w++)
        if ((long long) num_cus * waves2(b, w, wb) >= inum) pick_w = w;
    if (pick_w > 0) best_w = pick_w;
  }
  if (t.wpb && waves2(b, t.wpb, wb) > 0) best_w = t.wpb;
  return best_w;
}

// Blob prefix.  Which prefix the launch copies: the packed times rows in LDS when the chosen shape still fits with them
// (or when they are tiny), else the longest prefix that fits.  With MTP_BLOB_PREFIX set, exactly the planned prefix
// (the basic descriptors at most, unless it is the whole blob).
void choose_prefix(const BlobSizes &bs, const PlanTuning &t, size_t blob, int blocks_per_cu, int wpb, size_t wb, LaunchPlan &L)
{
  auto fits = [&](int bytes) { return (size_t) blocks_per_cu * ((size_t) bytes + wpb * wb) <= CU_LDS_BYTES; };
  const bool forced = t.prefix != PlanTuning::BEST;
  L.rows_lds = (forced ? (int) blob == bs.rows : fits(bs.rows)) && t.rows_lds;
  L.tgt_lds = forced ? (int) blob >= bs.tgt : (L.rows_lds || fits(bs.tgt));
  if (forced) L.blob_bytes = L.rows_lds ? bs.rows : std::min((int) blob, bs.norows);
  else L.blob_bytes = L.rows_lds ? bs.rows : (fits(bs.norows) ? bs.norows : (L.tgt_lds ? bs.tgt : bs.core));
}

struct ListSize {
  int num_cus, inum, cap;   // cap: capacity of the compacted id list (cj_cap)
  bool fine;                // few atoms, or the "small" variant
};

// Assembly.  One plan of the force kernel (grade: of its grade instantiation) against the blob prefix of `blob` bytes;
// returns the wavefronts per CU it reaches (0: does not fit).
int plan_one(const mtp_potential &p, const BlobSizes &bs, const PlanTuning &t, const ListSize &n, bool grade, size_t blob,
             LaunchPlan &L)
{
  Candidate cands[4];
  candidate_layouts(p, n.cap, grade, cands);
  const Budget b{blob, t.wave_cap};
  const Choice ch = choose_layout(cands, t, b, may_wps3(p, t, n.fine, grade));
  if (!ch.pick) return 0;
  const size_t wb = ch.pick->wave_bytes;
  int wpb = ch.w3, waves = 12;
  if (ch.wps == 2) {
    wpb = choose_width(b, t, wb, n.fine, n.num_cus, n.inum);
    if (wpb == 0) return 0;
    waves = std::max(1, waves2(b, wpb, wb));
  }
  const int blocks_per_cu = std::max(1, waves / wpb);
  L.layout = ch.pick->layout;
  L.rebuild = (L.layout.mode & 2) != 0;
  L.wps = ch.wps;
  L.tab_rows = 2 * p.slot_count + 3 * p.max_alpha_index_basic;
  L.g_doubles = 0;
  L.m_doubles = L.layout.m_doubles;
  L.ov_doubles = L.layout.off_nb;
  choose_prefix(bs, t, blob, blocks_per_cu, wpb, wb, L);
  L.wpb = wpb;
  L.wave_doubles = (int) (wb / 8);
  L.lds_bytes = (size_t) L.blob_bytes + wb * wpb;
  L.grid = std::max(1, std::min((n.inum + wpb - 1) / wpb, n.num_cus * blocks_per_cu));
  return waves;
}

// [1] candidate-vector kernel of grade calls: small table (r^-nu, Q_ri, powers), 8 wavefronts per workgroup
void plan_cvec(const mtp_potential &p, const BlobSizes &bs, const ListSize &n, LaunchPlan &L)
{
  int KL = 16, KB = 1;
  (void) mtp_pick_shape(p.alpha_index_basic_count, &KL, &KB);
  const int P = p.max_alpha_index_basic, Mu = p.radial_func_count, R = p.radial_basis_size, Sp = p.species_count;
  const size_t dbl = (size_t) KL * KB + (size_t) (4 * P + R) * (NT + 2) + 4 * (size_t) NT + (size_t) Mu * NT + (size_t) Sp * Mu * R;
  const size_t ints = (size_t) NT + n.cap;
  const size_t wb = (dbl * 8 + ints * 4 + 15) / 16 * 16;
  const size_t blob = (size_t) bs.norows;   // (this kernel reads the basic descriptors)
  int w = 8;
  while (w > 1 && blob + w * wb > CU_LDS_BYTES) w--;
  L.wpb = w;
  L.wave_doubles = (int) (wb / 8);
  L.lds_bytes = blob + wb * w;
  const int blocks_per_cu = std::max<int>(1, std::min<int>(8 / w, (int) (CU_LDS_BYTES / L.lds_bytes)));
  L.grid = std::max(1, std::min((n.inum + w - 1) / w, n.num_cus * blocks_per_cu));
  L.tab_rows = 4 * P + R;
  L.m_doubles = KL * KB;
  L.g_doubles = 0;
}

}   // namespace

bool plan_launch(const mtp_potential &p, const BlobSizes &bs, int num_cus, int inum, int max_numneigh, int variant,
                 LaunchPlan (&lp)[3], MtpDevParams &base)
{
  const PlanTuning t = read_tuning();
  const ListSize n{num_cus, inum, std::max(64, (max_numneigh + 31) / 32 * 32),
                   variant == MTP_VARIANT_SMALL || (variant == MTP_VARIANT_AUTO && inum < num_cus * 16)};
  // The shape is planned against each prefix of the table blob, longest first: a shorter prefix (tables read from
  // HBM / L2 instead) is taken only when it buys wavefronts per CU (level 20: 8 instead of 7 with the core prefix).
  std::vector<int> prefixes = {bs.rows, bs.norows, bs.tgt, bs.core};
  if (t.prefix != PlanTuning::BEST && t.prefix != PlanTuning::EACH)
    prefixes = {t.prefix == PlanTuning::CORE ? bs.core : t.prefix == PlanTuning::TGT ? bs.tgt
                    : t.prefix == PlanTuning::NOROWS ? bs.norows : bs.rows};
  for (int which : {0, 2}) {   // [0] fused force kernel, [2] its grade instantiation
    int best_waves = 0;
    for (int bytes : prefixes) {
      LaunchPlan L;
      const int v = plan_one(p, bs, t, n, which == 2, (size_t) bytes, L);
      if (v > best_waves) {
        best_waves = v;
        lp[which] = L;
      }
    }
    if (best_waves == 0) return false;
  }
  plan_cvec(p, bs, n, lp[1]);
  base.NT = NT;
  base.cj_cap = n.cap;
  base.d_doubles = p.stored_moment_count;
  return true;
}

// The plan covers the whole list.  A row range too short to fill it (the interior / boundary pieces of a small domain,
// strong scaling) runs in smaller workgroups, so that its atoms spread over all CUs instead of filling a few of them:
// per-atom latency, not throughput, is what such a launch waits for.
RowRange plan_row_range(const LaunchPlan &L, int num_cus, int row_count)
{
  int wpb = L.wpb;
  const int waves_per_cu = L.wpb * std::max(1, L.grid / std::max(1, num_cus));
  if (row_count < num_cus * waves_per_cu && L.grid >= num_cus) {
    const int small = L.wps == 3 ? 4 : 2;   // (multiples of 4 keep the SIMDs balanced at 3 per SIMD)
    if (small < wpb) wpb = small;
  }
  const size_t lds = (size_t) L.blob_bytes + (size_t) wpb * L.wave_doubles * 8;
  int g = (row_count + wpb - 1) / wpb;
  if (wpb == L.wpb) g = std::min(L.grid, g);
  else g = std::min(g, num_cus * (int) std::max<size_t>(1, CU_LDS_BYTES / std::max<size_t>(lds, 1)));
  if (g >= 8) g = (g + 7) / 8 * 8;   // whole rounds of the 8 XCDs for the XCD-aware atom map
  return {wpb, std::max(1, g), lds};
}

RowRange plan_cvec_range(const LaunchPlan &L, int row_count)
{
  return {L.wpb, std::max(1, std::min(L.grid, (row_count + L.wpb - 1) / L.wpb)), L.lds_bytes};
}

void apply_plan(MtpDevParams &p, const LaunchPlan &L, const mtp_potential &pot, bool grade)
{
  p.tab_rows = L.tab_rows;
  p.m_doubles = L.m_doubles;
  p.Am = grade ? pot.alpha_moment_count : pot.stored_moment_count;
  p.ov_doubles = L.ov_doubles;
  p.rebuild_tables = L.rebuild ? 1 : 0;
  p.rows_in_lds = L.rows_lds ? 1 : 0;
  p.blob_bytes = L.blob_bytes;
  p.tgt_in_lds = L.tgt_lds ? 1 : 0;
  p.dg_mode = L.layout.mode;
  p.pow_row = L.layout.pow_row;
  p.dg_off = L.layout.dg_off;
  p.fp_row = L.layout.fp_row;
  p.w_m = L.layout.off_m;
  p.w_d = L.layout.off_d;
  p.w_coef = L.layout.off_coef;
  p.w_nb = L.layout.off_nb;
  p.wps = L.wps;
  p.wave_doubles = L.wave_doubles;
  p.grade_flag = grade ? 1 : 0;
}

void build_blob(const mtp_potential &pot, const std::vector<MtpRow8> &rows8, const PlanTuning &tune, MtpDevParams &bb,
                BlobSizes &bs, std::vector<unsigned char> &blob)
{
  // The packed rows are the LAST piece of the blob: a launch plan copies them into LDS (BlobSizes::rows) or leaves
  // them in HBM/L2 (BlobSizes::norows) -- measured at level 16: rows in LDS are 1.2 % faster when they fit beside
  // the wavefronts' private regions anyway, and < 1 % slower otherwise (row reads do not depend on data).
  auto put = [&](const void *src, size_t bytes) {
    size_t off = (blob.size() + 15) / 16 * 16;
    blob.resize(off + bytes, 0);
    if (bytes) std::memcpy(blob.data() + off, src, bytes);
    return (int) off;
  };
  auto end_prefix = [&] {
    blob.resize((blob.size() + 15) / 16 * 16, 0);
    return (int) blob.size();
  };
  bb.off_level = put(pot.level_offset.data(), pot.level_offset.size() * sizeof(int32_t));
  bb.off_seg_fwd = put(pot.seg_fwd.data(), pot.seg_fwd.size() * sizeof(int32_t));
  bb.off_seg_bwd = put(pot.seg_bwd.data(), pot.seg_bwd.size() * sizeof(int32_t));
  std::vector<int32_t> slot_pad((size_t) pot.radial_func_count * MTP_PSTRIDE, -1);
  for (int mu = 0; mu < pot.radial_func_count; mu++)
    for (int nu = 0; nu < pot.max_alpha_index_basic; nu++)
      slot_pad[(size_t) mu * MTP_PSTRIDE + nu] = pot.slot_of[(size_t) mu * pot.max_alpha_index_basic + nu];
  bb.off_slot = put(slot_pad.data(), slot_pad.size() * sizeof(int32_t));
  bb.off_radial = put(pot.radial_basis_coeffs.data(), pot.radial_basis_coeffs.size() * sizeof(double));
  // scalar-side tables (24 B per basis function): LDS when they are small, HBM/L2 otherwise
  bb.scalars_in_lds = tune.scalars_lds >= 0 ? tune.scalars_lds : (pot.e_map.size() + pot.seed_idx.size()) * 12 <= 4096;
  if (bb.scalars_in_lds) {
    bb.off_seed_idx = put(pot.seed_idx.data(), pot.seed_idx.size() * sizeof(int32_t));
    bb.off_seed_val = put(pot.seed_val.data(), pot.seed_val.size() * sizeof(double));
    bb.off_map = put(pot.e_map.data(), pot.e_map.size() * sizeof(int32_t));
    bb.off_lin = put(pot.e_lin.data(), pot.e_lin.size() * sizeof(double));
  } else {
    bb.off_seed_idx = bb.off_seed_val = bb.off_map = bb.off_lin = 0;
  }
  bb.off_smu = put(pot.slot_mu.data(), pot.slot_mu.size() * sizeof(int32_t));
  bb.off_fwd = put(pot.fwd_blocks.data(), pot.fwd_blocks.size() * sizeof(int32_t));
  bb.nfb = pot.fwd_block_count;
  bs.core = end_prefix();
  bb.off_coef = put(pot.basic_tgt.data(), pot.basic_tgt.size() * sizeof(int32_t));
  bs.tgt = end_prefix();
  bb.off_pack = put(pot.basic_pack_lds.data(), pot.basic_pack_lds.size() * sizeof(int32_t));
  bs.norows = end_prefix();
  bb.off_rows = put(rows8.data(), rows8.size() * sizeof(MtpRow8));
  bb.off_leaf_cf = put(pot.leaf_cf.data(), pot.leaf_cf.size() * sizeof(double));
  bb.off_leaf_cb = pot.leaf_cb == pot.leaf_cf ? bb.off_leaf_cf : put(pot.leaf_cb.data(), pot.leaf_cb.size() * sizeof(double));
  bs.rows = end_prefix();
  // behind every prefix, so in HBM / L2 only and no part of any LDS plan: the five-factor blocks of the basic-moment
  // pass, which the kernels that take them read once per wavefront
  bb.off_fwd5 = put(pot.fwd5_blocks.data(), pot.fwd5_blocks.size() * sizeof(int32_t));
  bb.nfb5 = pot.fwd5_block_count;
  bb.blob_bytes = bs.norows;   // plan_launch decides per launch plan
  bb.rows_in_lds = 0;
}

void fill_sizes(const mtp_potential &pot, MtpDevParams &b)
{
  b.Sp = pot.species_count;
  b.R = pot.radial_basis_size;
  b.Mu = pot.radial_func_count;
  b.P = pot.max_alpha_index_basic;
  b.A = pot.alpha_moment_count;
  b.B = pot.alpha_index_basic_count;
  b.T = pot.alpha_index_times_count;
  b.S = pot.alpha_scalar_count;
  b.C = pot.coeff_count;
  b.nslot = pot.slot_count;
  b.coef_total = pot.coef_total;
  b.coef_dense = pot.coef_dense;
  for (int d = 0; d <= MTP_PSTRIDE; d++) {
    b.deg_first[d] = pot.deg_first[d];
    b.deg_coef[d] = pot.deg_coef[d];
  }
  b.nlevels = pot.normal_levels;   // (the level table has one more entry: the leaf rows)
  // the same table in the argument block when it fits (mtp_device.hpp); all zero otherwise
  const bool lv_fit = pot.level_offset.size() == (size_t) pot.normal_levels + 2 && pot.level_offset.size() <= MTP_SHAPE_ARR_LEN;
  for (int k = 0; k < MTP_SHAPE_ARR_LEN; k++) b.level_rows[k] = lv_fit && k < (int) pot.level_offset.size() ? pot.level_offset[k] : 0;
  // the slot tables likewise (mtp_device.hpp): table structure only, numbered by build_slots from the alpha tables
  unsigned long long mu_bits = 0;
  if (pot.radial_func_count <= 4 && pot.slot_count <= 32)
    for (int s = 0; s < pot.slot_count; s++) mu_bits |= (unsigned long long) (pot.slot_mu[s] & 3) << (2 * s);
  b.slot_mu_lo = (int) (unsigned) mu_bits;
  b.slot_mu_hi = (int) (unsigned) (mu_bits >> 32);
  const bool sr_fit = pot.radial_func_count <= MTP_SLOT_ROWS_MU && pot.slot_count <= 127 && pot.max_alpha_index_basic <= MTP_PSTRIDE;
  for (int k = 0; k < MTP_SHAPE_TAB_LEN; k++) {
    const int mu = k / MTP_PSTRIDE, nu = k % MTP_PSTRIDE;
    const bool in = sr_fit && mu < pot.radial_func_count && nu < pot.max_alpha_index_basic;
    b.slot_row[k] = (signed char) (in ? pot.slot_of[(size_t) mu * pot.max_alpha_index_basic + nu] : -1);
  }
  b.nseed = (int) pot.seed_idx.size();
  b.Ad = pot.stored_moment_count;
  b.Am = b.Ad;                      // per launch: the grade instantiation keeps the leaves' values too
  b.Se = (int) pot.e_map.size();
}

const char *pack_rows(const std::vector<MtpRow> &rows, std::vector<MtpRow8> &out)
{
  out.resize(rows.size());
  for (size_t k = 0; k < rows.size(); k++) {
    const MtpRow &r = rows[k];
    if (r.mult > 32767 || r.mult < -32768) return "alpha_index_times multiplicity outside 16 bits is not supported by this build";
    out[k].lo = (uint32_t) (8 * r.a0) | ((uint32_t) (8 * r.a1) << 16);
    out[k].hi = (uint32_t) (8 * r.a3) | (((uint32_t) r.mult & 0xffffu) << 16);
  }
  return nullptr;
}

int plan_params(const mtp_potential *pot, int num_cus, int inum, int max_numneigh, int variant, int grade, MtpDevParams &p)
{
  if (!pot || num_cus < 1 || inum < 0 || max_numneigh < 0 || variant < MTP_VARIANT_AUTO || variant > MTP_VARIANT_SMALL)
    return MTP_ERR_ARG;
  p = MtpDevParams{};
  const std::vector<MtpRow8> rows8(pot->rows_by_level.size());   // (only their size matters here)
  BlobSizes bs;
  std::vector<unsigned char> blob;
  build_blob(*pot, rows8, read_tuning(), p, bs, blob);
  fill_sizes(*pot, p);
  int kl_ = 0, kb_ = 0;
  if (mtp_pick_fwd_shape(pot->fwd_block_count, &kl_, &kb_) != 0) return MTP_ERR_LIMIT;
  LaunchPlan lp[3];
  if (!plan_launch(*pot, bs, num_cus, inum, max_numneigh, variant, lp, p)) return MTP_ERR_LIMIT;
  apply_plan(p, lp[grade ? 2 : 0], *pot, grade != 0);
  return MTP_OK;
}

}   // namespace mtp_plan

extern "C" int mtp_plan_fixed_fields(const mtp_potential *pot, int num_cus, int inum, int max_numneigh, int variant, int grade,
                                     char *buf, int buflen)
{
  MtpDevParams p;
  int rc = mtp_plan::plan_params(pot, num_cus, inum, max_numneigh, variant, grade, p);
  if (rc != MTP_OK) return rc;
  if (!buf || buflen <= 0) return MTP_ERR_ARG;
  int KL = 0, NB = 0;
  (void) mtp_pick_fwd_shape(p.nfb, &KL, &NB);
  const int dlow = mtp_wave_kernel_deg(KL, p.P) == mtp_wave_kernel_dlow(KL);
  std::string s;
  auto put = [&](const char *k, int v) { s += std::string(k) + "=" + std::to_string(v) + "\n"; };
  put("KL", KL);
  put("NB", NB);
  put("PITCH", MTP_PITCH);
  put("GRADE", grade ? 1 : 0);
  put("DEG", mtp_wave_kernel_deg(KL, p.P));
  put("WPS", dlow && p.wps == 3 ? 3 : 2);
  auto put_all = [&](const char *k, const auto *v, int n) {
    s += std::string(k) + "=";
    for (int i = 0; i < n; i++) s += (i ? "," : "") + std::to_string((int) v[i]);
    s += "\n";
  };
#define MTP_X(f) put(#f, p.f);
  MTP_SHAPE_INT_FIELDS(MTP_X)
  MTP_SHAPE_EXT_FIELDS(MTP_X)
#undef MTP_X
#define MTP_X(f) put_all(#f, p.f, MTP_SHAPE_ARR_LEN);
  MTP_SHAPE_ARR_FIELDS(MTP_X)
#undef MTP_X
#define MTP_X(f) put_all(#f, p.f, MTP_SHAPE_TAB_LEN);
  MTP_SHAPE_TAB_FIELDS(MTP_X)
#undef MTP_X
  if ((int) s.size() + 1 > buflen) return MTP_ERR_LIMIT;
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return MTP_OK;
}
