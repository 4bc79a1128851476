// Fixed-shape instantiations of the force kernel (gfx950): the statements of mtp_wave_kernel (mtp_wave_kernel_body.hpp) with the
// fields of the argument block that a shape of mtp_fixed_shapes.hpp fixes as compile-time constants.  Trip counts
// (slots per rank, seeds, energy entries, product levels) are then known, row and coefficient offsets fold into the
// immediates of the LDS instructions, and the layout / table-home branches go.  A translation unit of its own, so that
// it compiles beside mtp_kernels.hip.
//
// A launch takes one of these kernels only when its template arguments and EVERY field the shape fixes equal the
// launch's values (mtp_shape::matches, expanded from the same field list as the constants); everything else runs the
// generic kernels.  Nothing here is keyed on a file name, a level number, the coefficients or the system.
#include <hip/hip_runtime.h>

#include "mtp_device.hpp"

#include "mtp_wave_body.hpp"

#include "mtp_fixed_shapes.hpp"

namespace {

template <int KL, int NB, int PITCH, bool GRADE, int DEG, int WPS, class SH>
__global__ void __launch_bounds__(WPS == 3 ? 768 : 512, WPS) mtp_wave_kernel_fixed(const MtpDevParams p_arg)
{
  (void) p_arg;   // read through the kernarg segment pointer
#include "mtp_wave_kernel_body.hpp"
}

// the launcher's rule for the template arguments (mtp_kernels.hip, launch_pitch / launch_grade), then the fields
template <class SH> bool selects(const MtpDevParams &p)
{
  int KL = 0, NB = 0;
  if (mtp_pick_fwd_shape(p.nfb, &KL, &NB) != 0 || p.NT != 32) return false;
  const int deg = mtp_wave_kernel_deg(KL, p.P);
  const int wps = deg == mtp_wave_kernel_dlow(KL) && KL <= 32 && NB == 1 && p.wps == 3 ? 3 : 2;
  // a shape that takes the five-factor blocks gives every block a lane of the grid (the count itself is matched below)
  if constexpr (mtp_shape::has_nfb5<SH>::value)
    if (p.nfb5 > KL * NB) return false;
  return KL == SH::kKL && NB == SH::kNB && MTP_PITCH == SH::kPITCH && (p.grade_flag != 0) == SH::kGRADE && deg == SH::kDEG &&
      wps == SH::kWPS && mtp_shape::matches<SH>(p);
}

template <class SH> hipError_t launch_shape(const MtpDevParams &p, int grid, int wpb, size_t lds, hipStream_t st)
{
  static std::atomic<unsigned long long> attr_mask{0};
  auto *fn = &mtp_wave_kernel_fixed<SH::kKL, SH::kNB, SH::kPITCH, SH::kGRADE, SH::kDEG, SH::kWPS, SH>;
  const hipError_t e = mtp_raise_lds_limit(reinterpret_cast<const void *>(fn), attr_mask);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * wpb), lds, st, p);
  return hipGetLastError();
}

}   // namespace

const char *mtp_fixed_shape_match(const MtpDevParams &p)
{
#define MTP_X(SH) \
  if (selects<SH>(p)) return SH::name;
  MTP_FIXED_SHAPES(MTP_X)
#undef MTP_X
  (void) p;
  return nullptr;
}

hipError_t mtp_launch_wave_kernel_fixed(const MtpDevParams &p, int grid, int wpb, size_t lds, hipStream_t st, const char **used)
{
  *used = nullptr;
  if (wpb < 1 || wpb > (p.wps == 3 ? 12 : 8)) return hipErrorInvalidValue;
#define MTP_X(SH)                                \
  if (selects<SH>(p)) {                          \
    *used = SH::name;                            \
    return launch_shape<SH>(p, grid, wpb, lds, st); \
  }
  MTP_FIXED_SHAPES(MTP_X)
#undef MTP_X
  (void) grid;
  (void) lds;
  (void) st;
  return hipSuccess;
}
