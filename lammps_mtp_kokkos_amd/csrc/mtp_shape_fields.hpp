// Shapes of a force-kernel launch (internal): which fields of the argument block (MtpDevParams) may become compile-time
// constants of a fixed-shape instantiation of the kernel (mtp_kernels_fixed.hip).
//
// A candidate field is decided by the potential's table structure (the alpha_* tables, the species count, R) and by
// the LDS plan (mtp_plan.hpp, plan_launch), never by the fit, the system or the call.  A shape is a struct with one static
// constexpr member per field it fixes (and a name and the kernel's template arguments); a field it does not list stays a
// read of the argument block.  The three lists below are the only enumeration of the candidates: the kernel's accessor
// (SHF / SHA / SHT, mtp_wave_body.hpp), the launcher's field-by-field match (mtp_shape_matches) and the generator of
// mtp_fixed_shapes.hpp (mtp_plan_fixed_fields -> scripts/gen_fixed_shapes.py) are all expanded from them.
#pragma once

#include <type_traits>

#include "mtp_device.hpp"

// int fields
#define MTP_SHAPE_INT_FIELDS(X)                                                                                       \
  X(Sp) X(R) X(Mu) X(P) X(A) X(B) X(T) X(S) X(C) X(nslot) X(nlevels) X(nseed) X(Am) X(Ad) X(Se) X(nfb)                \
  X(coef_total) X(coef_dense) X(blob_bytes) X(off_rows) X(off_level) X(off_slot) X(off_radial) X(off_seed_idx)        \
  X(off_seed_val) X(off_map) X(off_lin) X(off_pack) X(off_fwd) X(off_smu) X(off_coef) X(off_leaf_cf) X(off_leaf_cb)   \
  X(off_seg_fwd) X(off_seg_bwd) X(rows_in_lds) X(tgt_in_lds) X(scalars_in_lds) X(dg_mode) X(fp_row) X(pow_row)        \
  X(dg_off) X(w_m) X(w_d) X(w_coef) X(w_nb) X(tab_rows) X(ov_doubles) X(m_doubles) X(d_doubles)                     \
  X(slot_mu_lo) X(slot_mu_hi)
// int fields of tables that no launch copies into LDS (they sit behind every prefix of the blob): matched, read and
// generated like the fields above; a list of its own because the list above is also the record of what the LDS plan
// decides (tests/plan_dump.cpp)
#define MTP_SHAPE_EXT_FIELDS(X) X(nfb5) X(off_fwd5)
// int[MTP_PSTRIDE + 2] fields (a shape gives them as static constexpr int f(int k))
#define MTP_SHAPE_ARR_FIELDS(X) X(deg_first) X(deg_coef) X(level_rows)
#define MTP_SHAPE_ARR_LEN (MTP_PSTRIDE + 2)
// signed char[MTP_SLOT_ROWS_MU * MTP_PSTRIDE] fields, indexed mu * MTP_PSTRIDE + nu (a shape gives them like the arrays)
#define MTP_SHAPE_TAB_FIELDS(X) X(slot_row)
#define MTP_SHAPE_TAB_LEN (MTP_SLOT_ROWS_MU * MTP_PSTRIDE)

// the generic shape: nothing fixed
struct ShapeGeneric {
  static constexpr const char *name = "";
};

namespace mtp_shape {

#define MTP_X(f)                                                                    \
  template <class SH, class = void> struct has_##f : std::false_type {};            \
  template <class SH> struct has_##f<SH, std::void_t<decltype(&SH::f)>> : std::true_type {};
MTP_SHAPE_INT_FIELDS(MTP_X)
MTP_SHAPE_EXT_FIELDS(MTP_X)
MTP_SHAPE_ARR_FIELDS(MTP_X)
MTP_SHAPE_TAB_FIELDS(MTP_X)
#undef MTP_X

// the launch's values equal the shape's over exactly the fields the shape fixes
template <class SH> bool matches(const MtpDevParams &p)
{
  bool ok = true;
#define MTP_X(f) \
  if constexpr (has_##f<SH>::value) ok = ok && p.f == SH::f;
  MTP_SHAPE_INT_FIELDS(MTP_X)
  MTP_SHAPE_EXT_FIELDS(MTP_X)
#undef MTP_X
#define MTP_X(f)                    \
  if constexpr (has_##f<SH>::value) \
    for (int k = 0; k < MTP_SHAPE_ARR_LEN; k++) ok = ok && p.f[k] == SH::f(k);
  MTP_SHAPE_ARR_FIELDS(MTP_X)
#undef MTP_X
#define MTP_X(f)                    \
  if constexpr (has_##f<SH>::value) \
    for (int k = 0; k < MTP_SHAPE_TAB_LEN; k++) ok = ok && p.f[k] == SH::f(k);
  MTP_SHAPE_TAB_FIELDS(MTP_X)
#undef MTP_X
  return ok;
}

}   // namespace mtp_shape

// mtp_kernels_fixed.hip: the name of the first compiled shape whose template arguments and fixed fields all equal the
// launch's, or nullptr (host only: needs no device)
const char *mtp_fixed_shape_match(const MtpDevParams &p);
// launches that shape's kernel; *used receives its name, or nullptr when no shape matches (nothing is launched then)
hipError_t mtp_launch_wave_kernel_fixed(const MtpDevParams &p, int grid, int wpb, size_t lds, hipStream_t st, const char **used);
