// Context (one GPU) and the extern "C" entry points of libmtp_mi355x (include/mtp_mi355x.h).
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "../../include/mtp_mi355x.h"
#include "mtp_device.hpp"
#include "mtp_shape_fields.hpp"
#include "mtp_plan.hpp"
#include "mtp_potential.hpp"

using namespace mtp_plan;

namespace {

struct HipFail {
  hipError_t e;
  const char *what;
};
#define HIP_CHECK(call)                                   \
  do {                                                    \
    hipError_t _e = (call);                               \
    if (_e != hipSuccess) throw HipFail{_e, #call};       \
  } while (0)

template <class T> struct DevBuf {
  T *ptr = nullptr;
  size_t cap = 0;
  void reserve(size_t n)
  {
    if (n <= cap) return;
    if (ptr) (void) hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ptr), std::max<size_t>(n, 1) * sizeof(T)));
    cap = n;
  }
  void upload(const T *src, size_t n, hipStream_t st)
  {
    reserve(n);
    if (n) HIP_CHECK(hipMemcpyAsync(ptr, src, n * sizeof(T), hipMemcpyHostToDevice, st));
  }
  void upload(const std::vector<T> &v, hipStream_t st) { upload(v.data(), v.size(), st); }
  ~DevBuf()
  {
    if (ptr) (void) hipFree(ptr);
  }
};

void copy_err(const std::string &s, char *err, int errlen)
{
  if (err && errlen > 0) std::snprintf(err, (size_t) errlen, "%s", s.c_str());
}

}   // namespace

struct mtp_context {
  const mtp_potential *pot = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string last_error;
  int variant = MTP_VARIANT_AUTO;
  int num_cus = 256;
  BlobSizes blob_sizes;   // the four prefixes of the table blob a launch plan may copy (mtp_plan.hpp)
  bool xcd_map = true;   // MTP_XCD_MAP=0 (tuning override) turns the XCD-aware atom map off
  // potential tables
  DevBuf<double> d_species;
  DevBuf<MtpRow8> d_rows, d_prog_fwd, d_prog_bwd;
  DevBuf<unsigned char> d_blob;
  DevBuf<int32_t> d_seed_idx, d_map, d_map_all, d_tgt;
  DevBuf<double> d_seed_val, d_lin, d_leaf_cf, d_leaf_cb;
  // neighbour list
  DevBuf<int> d_ilist, d_first, d_neigh;
  DevBuf<int> d_nb_scratch, d_nb_info;   // device neighbour-list build
  hipStream_t list_stream = nullptr;     // stream the context-owned list was last written on
  DevBuf<unsigned char> d_nb_tmp;
  DevBuf<double> d_nb_xs;
  const int *ilist = nullptr, *first = nullptr, *neigh = nullptr;   // active (owned or caller's)
  int inum = 0, nall = 0, max_numneigh = 0;
  bool have_list = false;
  // host-path staging
  DevBuf<double> d_x, d_f, d_eatom, d_vatom, d_grades, d_coeff;
  DevBuf<int> d_type;
  std::vector<double> h_tmp;
  // workspaces
  DevBuf<double> d_ev_slots, d_ev, d_maxg;
  DevBuf<long long> d_fq;      // deterministic mode: fixed-point force accumulators, kept zeroed between calls
  bool deterministic = false;
  DevBuf<int> d_err;
  DevBuf<unsigned long long> d_stamps;
  // launch geometry
  LaunchPlan lp[3];   // [0] force calls, [1] candidate-vector kernel of grade calls, [2] the grade instantiation (mtp_plan.hpp)
  DevBuf<double> d_cvec, d_ainv_pad, d_ainv_tiled, d_dbasic;
  DevBuf<double> d_csum;   // mtp_batch_cfg_grades: [ncfg][cpad] candidate vectors summed per configuration
  DevBuf<int> d_ident;     // and the identity ilist its grade launch reads them by
  DevBuf<double> d_maxvol;   // mtp_maxvol_select: the stacked matrix [W^T ; G] and the small state around it, kept between calls
  int cpad = 0, dpad = 0;
  int cvec_rows = 0;       // rows [0, cvec_rows) of the installed list all hold candidate vectors of grade calls on it
  // device-resident outputs of mtp_compute_resident (the /kk styles' DualViews): which of them the last call filled
  bool res_valid = false;
  int res_eflag = 0, res_vflag = 0, res_grade = 0;
  DevBuf<double> d_res_tot;   // [8 + 1 + C]: ev[8] | max grade | coeff_ders[C], zeroed by one launch per step
  // timing
  bool timing = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;

  // design rows and training gradient (mtp_design_rows_device, mtp_train_*_device): the one structural table of the
  // kernels with a workgroup per centre, built and uploaded by the first call of either kind
  bool centre_ready = false;
  DevBuf<MtpRow8> d_centre_rows;
  DevBuf<int32_t> d_centre_ints;     // level offsets | basic descriptors | scalar map | force map | basics by mu | mu offsets
  DevBuf<double> d_design_radial;
  MtpCentreParams centre{};          // shape and table; the system fields are bound per call (centre_bind)
  const int *centre_fmap = nullptr, *centre_bymu = nullptr, *centre_mufirst = nullptr;
  int train_rc = MTP_OK;             // what the training formulas say to this table (mtp_build_train_table, the packed basics)
  std::string train_msg;

  // The context's own values (include/mtp_mi355x.h, "installing ..."): initialised from the potential, replaced by the
  // installs, and the only source of values for what the context does after its creation -- `pot` is read for structure.
  std::vector<double> h_radial, h_species, h_moments, h_active_set, h_inverse;

  MtpDevParams base{};
  const char *last_shape = "";   // name of the fixed-shape kernel the last force launch ran ("": a generic kernel)

  int plan();   // the plans of the installed list; MTP_ERR_LIMIT and last_error when it does not fit
};

int mtp_context::plan()
{
  if (plan_launch(*pot, blob_sizes, num_cus, inum, max_numneigh, variant, lp, base)) return MTP_OK;
  last_error = NO_FIT;
  return MTP_ERR_LIMIT;
}

namespace {

bool set_device(mtp_context *c)
{
  if (hipSetDevice(c->device) == hipSuccess) return true;
  c->last_error = "hipSetDevice failed";
  return false;
}

int fail(mtp_context *c, int rc, const std::string &msg)   // a refusal: the code, and the message for mtp_last_error
{
  c->last_error = msg;
  return rc;
}

int device_fail(mtp_context *c, const HipFail &f)
{
  c->last_error = std::string(f.what) + ": " + hipGetErrorString(f.e);
  return MTP_ERR_DEVICE;
}

// W [C][C] zero padded to [cpad][cpad] for the MFMA grade kernel, and the same matrix in MFMA operand order for the
// LDS-staged grade kernel: [tile][k-step][lane], lane (j = l & 15, k = l >> 4) <- Ainv[16 tile + j][4 kstep + k]
void pad_and_tile(const double *W, int C, int cpad, std::vector<double> &pad, std::vector<double> &tiled)
{
  pad.assign((size_t) cpad * cpad, 0.0);
  for (int r = 0; r < C; r++) std::memcpy(&pad[(size_t) r * cpad], &W[(size_t) r * C], (size_t) C * sizeof(double));
  tiled.assign((size_t) cpad * cpad, 0.0);
  const int ks_n = cpad / 4;
  for (int t = 0; t < cpad / 16; t++)
    for (int ks = 0; ks < ks_n; ks++)
      for (int l = 0; l < 64; l++)
        tiled[((size_t) t * ks_n + ks) * 64 + l] = pad[(size_t) (16 * t + (l & 15)) * cpad + 4 * ks + (l >> 4)];
}

// calculate_extrapolation_grade for configuration mode (mtp_cfg_grade, mtp_context_cfg_grade)
double cfg_grade_of(const double *W, int C, const double *c)
{
  double mx = 0.0;
  for (int i = 0; i < C; i++) {
    const double *row = &W[(size_t) i * C];
    double g = 0.0;
    for (int j = 0; j < C; j++) g += c[j] * row[j];
    mx = std::max(mx, g < 0 ? -g : g);
  }
  return mx;
}

bool all_finite(const double *v, size_t n)   // (a null array is an argument left out)
{
  for (size_t i = 0; v && i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}   // namespace

extern "C" {

int mtp_potential_load(const char *path, int want_selection, mtp_potential **out, char *err, int errlen)
{
  if (!path || !out) return MTP_ERR_ARG;
  *out = nullptr;
  mtp_potential *p = new (std::nothrow) mtp_potential();
  if (!p) return MTP_ERR_ARG;
  std::string msg;
  int rc = mtp_parse_file(path, want_selection != 0, *p, msg);
  if (rc != MTP_OK) {
    copy_err(msg, err, errlen);
    delete p;
    return rc;
  }
  *out = p;
  return MTP_OK;
}

void mtp_potential_free(mtp_potential *pot) { delete pot; }

int mtp_potential_get_info(const mtp_potential *p, mtp_potential_info *info)
{
  if (!p || !info) return MTP_ERR_ARG;
  info->species_count = p->species_count;
  info->radial_basis_size = p->radial_basis_size;
  info->radial_func_count = p->radial_func_count;
  info->alpha_moment_count = p->alpha_moment_count;
  info->alpha_index_basic_count = p->alpha_index_basic_count;
  info->alpha_index_times_count = p->alpha_index_times_count;
  info->alpha_scalar_count = p->alpha_scalar_count;
  info->max_alpha_index_basic = p->max_alpha_index_basic;
  info->coeff_count = p->coeff_count;
  info->has_selection = p->has_selection;
  info->configuration_mode = p->configuration_mode;
  info->product_levels = p->normal_levels;
  info->scaling = p->scaling;
  info->min_cutoff = p->min_cutoff;
  info->max_cutoff = p->max_cutoff;
  return MTP_OK;
}

int mtp_potential_kernel_shape(const mtp_potential *p, int32_t *fwd_blocks, int32_t *block_lanes,
                               int32_t *blocks_per_lane, int32_t *max_degree)
{
  if (!p) return MTP_ERR_ARG;
  if (fwd_blocks) *fwd_blocks = p->fwd_block_count;
  int KL = 0, NB = 0;
  if (mtp_pick_fwd_shape(p->fwd_block_count, &KL, &NB) != 0) return MTP_ERR_LIMIT;
  if (block_lanes) *block_lanes = KL;
  if (blocks_per_lane) *blocks_per_lane = NB;
  if (max_degree) *max_degree = mtp_wave_kernel_deg(KL, p->max_alpha_index_basic);
  return MTP_OK;
}

int mtp_potential_moment_blocks(const mtp_potential *p, int five, int32_t *blocks, int cap_blocks, int32_t *basic_pack)
{
  if (!p || cap_blocks < 0) return MTP_ERR_ARG;
  const std::vector<int32_t> &v = five ? p->fwd5_blocks : p->fwd_blocks;
  const int n = five ? p->fwd5_block_count : p->fwd_block_count;
  if (blocks) {
    if (cap_blocks < n) return MTP_ERR_ARG;
    if (n) std::memcpy(blocks, v.data(), (size_t) n * 8 * sizeof(int32_t));
  }
  if (basic_pack && !p->basic_pack_lds.empty())
    std::memcpy(basic_pack, p->basic_pack_lds.data(), p->basic_pack_lds.size() * sizeof(int32_t));
  return n;
}

int mtp_potential_get_tables(const mtp_potential *p, int32_t *aib, int32_t *ait, int32_t *map, double *rc,
                             double *sc, double *mc, double *inv)
{
  if (!p) return MTP_ERR_ARG;
  auto cp = [](auto *dst, const auto &v) {
    if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
  };
  cp(aib, p->alpha_index_basic);
  cp(ait, p->alpha_index_times);
  cp(map, p->alpha_moment_mapping);
  cp(rc, p->radial_basis_coeffs);
  cp(sc, p->species_coeffs);
  cp(mc, p->linear_coeffs);
  if (inv) {
    if (!p->has_selection) return MTP_ERR_STATE;
    cp(inv, p->inverse_active_set);
  }
  return MTP_OK;
}

int mtp_potential_get_active_set(const mtp_potential *p, double *active_set)
{
  if (!p || !active_set) return MTP_ERR_ARG;
  if (!p->has_selection) return MTP_ERR_STATE;
  std::memcpy(active_set, p->active_set.data(), p->active_set.size() * sizeof(double));
  return MTP_OK;
}

int mtp_potential_write_selection(const char *src_path, const char *dst_path, const double *active_set,
                                  const double *inverse_active_set, int coeff_count, char *err, int errlen)
{
  if (!src_path || !dst_path || !active_set || !inverse_active_set) {
    copy_err("mtp_potential_write_selection: null argument", err, errlen);
    return MTP_ERR_ARG;
  }
  mtp_potential src;
  std::string msg;
  const int rc = mtp_parse_file(src_path, true, src, msg);
  if (rc != MTP_OK) {
    copy_err(msg, err, errlen);
    return rc;
  }
  if (coeff_count != src.coeff_count) {
    copy_err("mtp_potential_write_selection: coeff_count is " + std::to_string(coeff_count) + ", the file's is " +
                 std::to_string(src.coeff_count),
             err, errlen);
    return MTP_ERR_ARG;
  }
  // the text of the source up to and including the '#' of the raw blocks, byte for byte, then the two blocks
  std::vector<char> head((size_t) src.selection_offset);
  FILE *in = std::fopen(src_path, "rb");
  const bool got = in && std::fread(head.data(), 1, head.size(), in) == head.size();
  if (in) std::fclose(in);
  if (!got) {
    copy_err(std::string("Cannot read potential file ") + src_path, err, errlen);
    return MTP_ERR_IO;
  }
  const std::string tmp = std::string(dst_path) + ".tmp" + std::to_string((long) getpid());
  FILE *out = std::fopen(tmp.c_str(), "wb");
  if (!out) {
    copy_err("Cannot open " + tmp + " for writing: " + std::strerror(errno), err, errlen);
    return MTP_ERR_IO;
  }
  const size_t n = (size_t) coeff_count * coeff_count;
  bool ok = std::fwrite(head.data(), 1, head.size(), out) == head.size() &&
            std::fwrite(active_set, sizeof(double), n, out) == n &&
            std::fwrite(inverse_active_set, sizeof(double), n, out) == n;
  int why = ok ? 0 : errno;   // of the call that failed, not of one after it
  if (std::fclose(out) != 0 && ok) {
    ok = false;
    why = errno;
  }
  if (ok && std::rename(tmp.c_str(), dst_path) != 0) {
    ok = false;
    why = errno;
  }
  if (!ok) {
    copy_err(std::string("Cannot write potential file ") + dst_path + ": " + std::strerror(why), err, errlen);
    std::remove(tmp.c_str());
    return MTP_ERR_IO;
  }
  return MTP_OK;
}

int mtp_cfg_grade(const mtp_potential *p, const double *c, double *grade)
{
  if (!p || !c || !grade) return MTP_ERR_ARG;
  if (!p->has_selection) return MTP_ERR_STATE;
  *grade = cfg_grade_of(p->inverse_active_set.data(), p->coeff_count, c);
  return MTP_OK;
}

int mtp_context_create(const mtp_potential *pot, int device_id, mtp_context **out, char *err, int errlen)
{
  if (!pot || !out) return MTP_ERR_ARG;
  *out = nullptr;
  mtp_context *c = nullptr;
  try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      copy_err("no HIP device is visible: libmtp_mi355x has no CPU fallback", err, errlen);
      return MTP_ERR_DEVICE;
    }
    if (device_id < 0 || device_id >= ndev) {
      copy_err("device id out of range", err, errlen);
      return MTP_ERR_ARG;
    }
    HIP_CHECK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      copy_err(std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only", err,
               errlen);
      return MTP_ERR_DEVICE;
    }
    c = new mtp_context();
    c->pot = pot;
    c->h_radial = pot->radial_basis_coeffs;
    c->h_species = pot->species_coeffs;
    c->h_moments = pot->linear_coeffs;
    if (pot->has_selection) {
      c->h_active_set = pot->active_set;
      c->h_inverse = pot->inverse_active_set;
    }
    c->device = device_id;
    c->num_cus = prop.multiProcessorCount;
    if (const char *e = std::getenv("MTP_XCD_MAP")) c->xcd_map = std::atoi(e) != 0;
    HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    hipStream_t st = c->stream;
    c->d_species.upload(pot->species_coeffs, st);
    // packed rows (8 B each): moment ids in 16 bits, multiplicity in a signed 16 bits
    if (pot->alpha_moment_count > 8191) {   // (packed rows hold 16-bit byte offsets; 8192 moments are 128 KB of LDS anyway)
      copy_err("alpha_moments_count above 8191 is not supported by this build", err, errlen);
      delete c;
      return MTP_ERR_LIMIT;
    }
    std::vector<MtpRow8> rows8, fwd8, bwd8;
    const char *refusal = pack_rows(pot->rows_by_level, rows8);
    if (!refusal) refusal = pack_rows(pot->prog_fwd, fwd8);
    if (!refusal) refusal = pack_rows(pot->prog_bwd, bwd8);
    if (refusal) {
      copy_err(refusal, err, errlen);
      delete c;
      return MTP_ERR_LIMIT;
    }
    c->d_rows.upload(rows8, st);
    c->d_prog_fwd.upload(fwd8, st);
    c->d_prog_bwd.upload(bwd8, st);
    // table blob copied into LDS by every workgroup
    MtpDevParams &bb = c->base;
    std::vector<unsigned char> blob;
    build_blob(*pot, rows8, read_tuning(), bb, c->blob_sizes, blob);
    c->d_seed_idx.upload(pot->seed_idx, st);
    c->d_seed_val.upload(pot->seed_val, st);
    c->d_map.upload(pot->e_map, st);
    c->d_lin.upload(pot->e_lin, st);
    c->d_map_all.upload(pot->mapping_lds, st);
    c->d_leaf_cf.upload(pot->leaf_cf, st);
    c->d_leaf_cb.upload(pot->leaf_cb, st);
    bb.g_seed_idx = c->d_seed_idx.ptr;
    bb.g_seed_val = c->d_seed_val.ptr;
    bb.g_map = c->d_map.ptr;
    bb.g_lin = c->d_lin.ptr;
    bb.g_map_all = c->d_map_all.ptr;
    bb.leaf_cf = c->d_leaf_cf.ptr;
    bb.leaf_cb = c->d_leaf_cb.ptr;
    c->d_tgt.upload(pot->basic_tgt, st);
    bb.g_tgt = c->d_tgt.ptr;
    c->d_blob.upload(blob.data(), blob.size(), st);
    if (pot->has_selection) {   // inverse active set zero padded to a multiple of 16 for the MFMA grade kernel
      const int C = pot->coeff_count;
      c->cpad = (C + 15) / 16 * 16;
      std::vector<double> pad, tiled;
      pad_and_tile(pot->inverse_active_set.data(), C, c->cpad, pad, tiled);
      c->d_ainv_pad.upload(pad, st);
      c->d_ainv_tiled.upload(tiled, st);
      HIP_CHECK(hipStreamSynchronize(st));
    }
    c->d_ev_slots.reserve((size_t) MTP_EV_SLOTS * 8);
    HIP_CHECK(hipMemsetAsync(c->d_ev_slots.ptr, 0, (size_t) MTP_EV_SLOTS * 8 * sizeof(double), st));
    c->d_ev.reserve(8);
    c->d_maxg.reserve(1);
    c->d_err.reserve(1);
    HIP_CHECK(hipMemsetAsync(c->d_err.ptr, 0, sizeof(int), st));
#ifdef MTP_STAMPS
    constexpr size_t stamp_words = 16 + MTP_TRACE_WORDS;   // the phase sums, then the per-wavefront trace
#else
    constexpr size_t stamp_words = 16;
#endif
    c->d_stamps.reserve(stamp_words);
    HIP_CHECK(hipMemsetAsync(c->d_stamps.ptr, 0, stamp_words * sizeof(unsigned long long), st));
    HIP_CHECK(hipStreamSynchronize(st));

    MtpDevParams &b = c->base;
    fill_sizes(*pot, b);
    b.rmin = pot->min_cutoff;
    b.rmax = pot->max_cutoff;
    b.scaling = pot->scaling;
    b.cutsq = pot->max_cutoff * pot->max_cutoff;   // pair_mtp.cpp:449,456
    b.inv_span = 1.0 / (pot->max_cutoff - pot->min_cutoff);
    b.inv_rmax = 1.0 / pot->max_cutoff;
    b.blob = c->d_blob.ptr;
    b.rows = c->d_rows.ptr;
    b.prog_fwd = c->d_prog_fwd.ptr;
    b.prog_bwd = c->d_prog_bwd.ptr;
    b.species_coeffs = c->d_species.ptr;
    b.inv_mu = 1.0f / (float) pot->radial_func_count;
    b.ev_slots = c->d_ev_slots.ptr;
    b.err_flag = c->d_err.ptr;
    b.stamps = c->d_stamps.ptr;
    int kl_ = 0, kb_ = 0;
    if (mtp_pick_fwd_shape(pot->fwd_block_count, &kl_, &kb_) != 0) {
      copy_err("more than 256 head x tail blocks of basic moments are not supported by this build", err, errlen);
      delete c;
      return MTP_ERR_LIMIT;
    }
    if (mtp_pick_shape(pot->alpha_index_basic_count, &kl_, &kb_) != 0) {
      copy_err("alpha_index_basic_count above 640 is not supported by this build", err, errlen);
      delete c;
      return MTP_ERR_LIMIT;
    }
  } catch (const HipFail &f) {
    copy_err(std::string(f.what) + ": " + hipGetErrorString(f.e), err, errlen);
    delete c;
    return MTP_ERR_DEVICE;
  }
  *out = c;
  return MTP_OK;
}

void mtp_context_destroy(mtp_context *c)
{
  if (!c) return;
  (void) hipSetDevice(c->device);
  if (c->ev0) (void) hipEventDestroy(c->ev0);
  if (c->ev1) (void) hipEventDestroy(c->ev1);
  if (c->stream) {
    (void) hipStreamSynchronize(c->stream);
    (void) hipStreamDestroy(c->stream);
  }
  delete c;
}

const char *mtp_last_error(const mtp_context *c) { return c ? c->last_error.c_str() : "null context"; }

int mtp_context_set_variant(mtp_context *c, int variant)
{
  if (!c || variant < MTP_VARIANT_AUTO || variant > MTP_VARIANT_SMALL) return MTP_ERR_ARG;
  c->variant = variant;
  if (c->have_list) return c->plan();
  return MTP_OK;
}

static int finish_list(mtp_context *c, int inum, int nall, int max_numneigh)
{
  c->inum = inum;
  c->nall = nall;
  c->max_numneigh = max_numneigh;
  c->have_list = true;
  c->cvec_rows = 0;
  const int rc = c->plan();
  if (rc != MTP_OK) {
    c->have_list = false;
    return rc;
  }
  try {
    if (c->pot->has_selection && inum > 0) {   // candidate vectors, zero padded rows of cpad doubles
      const size_t n = (size_t) inum * c->cpad;
      if (n > c->d_cvec.cap) {
        c->d_cvec.reserve(n);
        HIP_CHECK(hipMemset(c->d_cvec.ptr, 0, n * sizeof(double)));
      }
      int kl_ = 16, kb_ = 1;
      (void) mtp_pick_shape(c->pot->alpha_index_basic_count, &kl_, &kb_);
      c->dpad = kl_ * kb_;
      c->d_dbasic.reserve((size_t) inum * c->dpad);
    }
  } catch (const HipFail &f) {
    c->last_error = f.what;
    c->have_list = false;
    return MTP_ERR_DEVICE;
  }
  return MTP_OK;
}

int mtp_set_neighbors_csr(mtp_context *c, int inum, const int *ilist, const int *first, const int *neigh,
                          int nall)
{
  if (!c || inum < 0 || nall < inum || (inum > 0 && (!ilist || !first))) return MTP_ERR_ARG;
  try {
    HIP_CHECK(hipSetDevice(c->device));
    int mx = 0;
    for (int ii = 0; ii < inum; ii++) mx = std::max(mx, first[ii + 1] - first[ii]);
    const int total = inum > 0 ? first[inum] : 0;
    if (total > 0 && !neigh) return MTP_ERR_ARG;
    c->d_ilist.upload(ilist, (size_t) inum, c->stream);
    std::vector<int> z(1, 0);
    c->d_first.upload(inum > 0 ? first : z.data(), (size_t) inum + 1, c->stream);
    c->d_neigh.upload(neigh, (size_t) total, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ilist = c->d_ilist.ptr;
    c->first = c->d_first.ptr;
    c->neigh = c->d_neigh.ptr;
    return finish_list(c, inum, nall, mx);
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
}

int mtp_set_neighbors(mtp_context *c, int inum, const int *ilist, const int *numneigh,
                      const int *const *firstneigh, int nall)
{
  if (!c || inum < 0 || (inum > 0 && (!ilist || !numneigh || !firstneigh))) return MTP_ERR_ARG;
  std::vector<int> first((size_t) inum + 1, 0);
  long long total = 0;
  for (int ii = 0; ii < inum; ii++) total += numneigh[ilist[ii]];
  if (total > 2147483647LL) return fail(c, MTP_ERR_LIMIT, "neighbour list has more than 2^31-1 entries on this rank");
  for (int ii = 0; ii < inum; ii++) first[ii + 1] = first[ii] + numneigh[ilist[ii]];
  std::vector<int> neigh((size_t) first[inum]);
  for (int ii = 0; ii < inum; ii++) {
    const int i = ilist[ii];
    std::copy(firstneigh[i], firstneigh[i] + numneigh[i], neigh.begin() + first[ii]);
  }
  return mtp_set_neighbors_csr(c, inum, ilist, first.data(), neigh.data(), nall);
}

int mtp_set_neighbors_device(mtp_context *c, int inum, const int *d_ilist, const int *d_first,
                             const int *d_neigh, int nall, int max_numneigh)
{
  if (!c || inum < 0 || nall < inum || max_numneigh < 0 || (inum > 0 && (!d_ilist || !d_first))) return MTP_ERR_ARG;
  (void) hipSetDevice(c->device);
  c->ilist = d_ilist;
  c->first = d_first;
  c->neigh = d_neigh;
  return finish_list(c, inum, nall, max_numneigh);
}

int mtp_build_neighbors_device(mtp_context *c, void *stream, const double *d_x, int inum, int nall,
                               double list_cutoff, const double lo[3], const double hi[3],
                               const int **d_first_out, const int **d_neigh_out, long long *total_out,
                               int *max_numneigh_out)
{
  if (!c || inum < 0 || nall < inum || !lo || !hi || !(list_cutoff > 0.0) || (nall > 0 && !d_x)) return MTP_ERR_ARG;
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  int n3[3];
  long long ncell = 1;
  for (int a = 0; a < 3; a++) {
    if (!(hi[a] >= lo[a])) return MTP_ERR_ARG;
    n3[a] = std::max(1, (int) std::ceil((hi[a] - lo[a]) / list_cutoff));
    ncell *= n3[a];
  }
  if (ncell > (1ll << 26))
    return fail(c, MTP_ERR_LIMIT, "neighbour build: more than 2^26 cells (box much larger than the atoms it holds?)");
  try {
    const size_t scan_n = (size_t) std::max<long long>(ncell, inum) + 1;
    const size_t cub_bytes = mtp_neighbor_scan_bytes((int) scan_n, nall);
    c->d_nb_tmp.reserve(std::max<size_t>(cub_bytes, 16));
    c->d_nb_scratch.reserve((size_t) 4 * nall + 2 * (size_t) ncell + 2 + (size_t) inum + 1);
    c->d_nb_info.reserve(2);
    c->d_nb_xs.reserve((size_t) 3 * std::max(nall, 1));
    c->d_ilist.reserve((size_t) std::max(inum, 1));
    c->d_first.reserve((size_t) inum + 1);
    HIP_CHECK(mtp_launch_neighbor_build(d_x, inum, nall, list_cutoff, lo, n3, c->d_nb_scratch.ptr, c->d_nb_xs.ptr,
                                        c->d_nb_tmp.ptr, c->d_nb_tmp.cap, c->d_ilist.ptr, c->d_first.ptr, nullptr,
                                        c->d_nb_info.ptr, st));
    int info[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(info, c->d_nb_info.ptr, sizeof(info), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (info[0] < 0 || (long long) inum * info[1] > 0x7fffffffll)
      return fail(c, MTP_ERR_LIMIT, "neighbour list has more than 2^31-1 entries on this rank");
    c->d_neigh.reserve((size_t) std::max(info[0], 1));
    HIP_CHECK(mtp_launch_neighbor_build(d_x, inum, nall, list_cutoff, lo, n3, c->d_nb_scratch.ptr, c->d_nb_xs.ptr,
                                        c->d_nb_tmp.ptr, c->d_nb_tmp.cap, c->d_ilist.ptr, c->d_first.ptr, c->d_neigh.ptr,
                                        c->d_nb_info.ptr, st));
    c->ilist = c->d_ilist.ptr;
    c->first = c->d_first.ptr;
    c->neigh = c->d_neigh.ptr;
    c->list_stream = st;
    if (d_first_out) *d_first_out = c->d_first.ptr;
    if (d_neigh_out) *d_neigh_out = c->d_neigh.ptr;
    if (total_out) *total_out = info[0];
    if (max_numneigh_out) *max_numneigh_out = info[1];
    return finish_list(c, inum, nall, info[1]);
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
}

int mtp_set_neighbors_device_2d(mtp_context *c, void *stream, int inum, const int *d_ilist, const int *d_numneigh,
                                const int *d_neighbors, long long stride_i, long long stride_jj, int max_neighs, int nall)
{
  if (!c || inum < 0 || nall < inum || max_neighs < 0 || (inum > 0 && (!d_ilist || !d_numneigh)) || stride_i < 0 || stride_jj < 0)
    return MTP_ERR_ARG;
  if (inum > 0 && max_neighs > 0 && (!d_neighbors || (stride_i != 1 && stride_jj != 1)))
    return fail(c, MTP_ERR_ARG, "mtp_set_neighbors_device_2d: one of the two strides must be 1 (LayoutLeft or LayoutRight view)");
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  try {
    const size_t cub_bytes = mtp_neighbor_scan_bytes(inum + 1, 1);
    c->d_nb_tmp.reserve(std::max<size_t>(cub_bytes, 16));
    c->d_nb_scratch.reserve((size_t) inum + 1);
    c->d_nb_info.reserve(4);
    c->d_first.reserve((size_t) inum + 1);
    HIP_CHECK(mtp_launch_list_from_2d(inum, d_ilist, d_numneigh, d_neighbors, stride_i, stride_jj, max_neighs,
                                      c->d_nb_scratch.ptr, c->d_nb_tmp.ptr, c->d_nb_tmp.cap, c->d_first.ptr, nullptr,
                                      c->d_nb_info.ptr, st));
    int info[3] = {0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(info, c->d_nb_info.ptr, sizeof(info), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));   // one read-back per re-neighbouring sizes the entry array and the LDS plan
    if (info[2])
      return fail(c, MTP_ERR_ARG,
                  "mtp_set_neighbors_device_2d: a d_numneigh entry is negative or exceeds the view's second extent");
    if (info[0] < 0) return fail(c, MTP_ERR_LIMIT, "neighbour list has more than 2^31-1 entries on this rank");
    c->d_neigh.reserve((size_t) std::max(info[0], 1));
    HIP_CHECK(mtp_launch_list_from_2d(inum, d_ilist, d_numneigh, d_neighbors, stride_i, stride_jj, max_neighs,
                                      c->d_nb_scratch.ptr, c->d_nb_tmp.ptr, c->d_nb_tmp.cap, c->d_first.ptr, c->d_neigh.ptr,
                                      c->d_nb_info.ptr, st));
    c->ilist = d_ilist;   // the caller's (KOKKOS') d_ilist stays in use: it must remain valid until the next list
    c->first = c->d_first.ptr;
    c->neigh = c->d_neigh.ptr;
    c->list_stream = st;
    return finish_list(c, inum, nall, info[1]);
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
}

// ---- device-resident step (include/mtp_mi355x.h, "device-resident step") ------------------------------------------
int mtp_compute_resident(mtp_context *c, void *stream, const double *d_x, const int *d_type, double *d_f, int eflag, int vflag,
                         int grade_flag)
{
  if (!c || !d_x || !d_type || !d_f) return MTP_ERR_ARG;
  if (!c->have_list) return fail(c, MTP_ERR_STATE, "mtp_compute before mtp_set_neighbors");
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  const size_t nall = (size_t) c->nall, C = (size_t) c->pot->coeff_count;
  const bool want_ea = (eflag & MTP_ENERGY_ATOM) != 0, want_va = (vflag & MTP_VIRIAL_ATOM) != 0;
  const bool cfg = c->pot->configuration_mode != 0;
  c->res_valid = false;
  try {
    // totals: one allocation, padded to an even count, zeroed by ONE launch on the caller's stream
    const size_t ntot = (8 + 1 + C + 1) / 2 * 2;
    c->d_res_tot.reserve(ntot);
    HIP_CHECK(mtp_launch_zero(c->d_res_tot.ptr, ntot, st));
    if (want_ea) {   // eatom[i] is assigned for i in ilist; every other row reads 0 (LAMMPS zeroes eatom in ev_setup)
      c->d_eatom.reserve(nall + (nall & 1));
      HIP_CHECK(mtp_launch_zero(c->d_eatom.ptr, nall + (nall & 1), st));
    }
    if (want_va) {
      c->d_vatom.reserve(6 * nall);
      HIP_CHECK(mtp_launch_zero(c->d_vatom.ptr, 6 * nall, st));
    }
    if (grade_flag && !cfg) {   // grown, never shrunk; rows outside ilist keep their last value (pair_mtp_extrapolation.cpp:91-94)
      if (c->d_grades.cap < nall) {
        c->d_grades.reserve(nall + (nall & 1));
        HIP_CHECK(mtp_launch_zero(c->d_grades.ptr, nall + (nall & 1), st));
      }
    }
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  double *tot = c->d_res_tot.ptr;
  const int rc = mtp_compute_device(c, reinterpret_cast<void *>(st), d_x, d_type, eflag, vflag, grade_flag, d_f,
                                    want_ea ? c->d_eatom.ptr : nullptr, want_va ? c->d_vatom.ptr : nullptr, tot,
                                    grade_flag && !cfg ? c->d_grades.ptr : nullptr, grade_flag ? tot + 8 : nullptr,
                                    grade_flag && cfg ? tot + 9 : nullptr);
  if (rc != MTP_OK) return rc;
  c->res_valid = true;
  c->res_eflag = eflag;
  c->res_vflag = vflag;
  c->res_grade = grade_flag ? 1 : 0;
  return MTP_OK;
}

int mtp_resident_totals(mtp_context *c, void *stream, double *ev7, double *max_grade, double *coeff_ders)
{
  if (!c) return MTP_ERR_ARG;
  if (!c->res_valid) return fail(c, MTP_ERR_STATE, "mtp_resident_totals before mtp_compute_resident");
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  const size_t C = (size_t) c->pot->coeff_count, n = 9 + (coeff_ders && c->res_grade ? C : 0);
  c->h_tmp.resize(std::max<size_t>(c->h_tmp.size(), 9 + C));
  if (hipSetDevice(c->device) != hipSuccess ||
      hipMemcpyAsync(c->h_tmp.data(), c->d_res_tot.ptr, n * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess) {
    c->last_error = "resident totals: copy failed";
    return MTP_ERR_DEVICE;
  }
  const int rc = mtp_synchronize(c, reinterpret_cast<void *>(st));   // the one wait of the step; reports the atom-type error
  if (rc != MTP_OK) return rc;
  if (ev7)
    for (int q = 0; q < 7; q++) ev7[q] = c->h_tmp[q];
  if (max_grade) *max_grade = c->res_grade ? c->h_tmp[8] : 0.0;
  if (coeff_ders && c->res_grade)
    for (size_t q = 0; q < C; q++) coeff_ders[q] = c->h_tmp[9 + q];
  return MTP_OK;
}

static int resident_array(mtp_context *c, int what, const double **ptr, int *ncol)
{
  if (!c->res_valid) return fail(c, MTP_ERR_STATE, "per-atom outputs asked for before mtp_compute_resident");
  switch (what) {
    case MTP_PERATOM_EATOM:
      if (!(c->res_eflag & MTP_ENERGY_ATOM)) break;
      *ptr = c->d_eatom.ptr;
      *ncol = 1;
      return MTP_OK;
    case MTP_PERATOM_VATOM:
      if (!(c->res_vflag & MTP_VIRIAL_ATOM)) break;
      *ptr = c->d_vatom.ptr;
      *ncol = 6;
      return MTP_OK;
    case MTP_PERATOM_GRADES:
      if (!c->d_grades.ptr || c->pot->configuration_mode) break;
      *ptr = c->d_grades.ptr;
      *ncol = 1;
      return MTP_OK;
    default:
      return MTP_ERR_ARG;
  }
  c->last_error = "this per-atom output was not produced by the last mtp_compute_resident call";
  return MTP_ERR_STATE;
}

int mtp_resident_peratom_device(mtp_context *c, int what, const double **d_ptr, int *ncol)
{
  if (!c || !d_ptr) return MTP_ERR_ARG;
  int nc = 0;
  const int rc = resident_array(c, what, d_ptr, &nc);
  if (rc == MTP_OK && ncol) *ncol = nc;
  return rc;
}

int mtp_resident_peratom_host(mtp_context *c, void *stream, int what, double *host)
{
  if (!c || !host) return MTP_ERR_ARG;
  const double *src = nullptr;
  int nc = 0;
  const int rc = resident_array(c, what, &src, &nc);
  if (rc != MTP_OK) return rc;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  if (hipSetDevice(c->device) != hipSuccess ||
      hipMemcpyAsync(host, src, (size_t) c->nall * nc * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    c->last_error = "resident per-atom output: copy failed";
    return MTP_ERR_DEVICE;
  }
  return MTP_OK;
}

int mtp_copy_to_host(mtp_context *c, void *stream, void *host, const void *d_src, size_t bytes)
{
  if (!c || (bytes > 0 && (!host || !d_src))) return MTP_ERR_ARG;
  if (bytes == 0) return MTP_OK;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  if (hipSetDevice(c->device) != hipSuccess || hipMemcpyAsync(host, d_src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    c->last_error = "mtp_copy_to_host failed";
    return MTP_ERR_DEVICE;
  }
  return MTP_OK;
}

const char *mtp_build_flags(void)
{
  // compile-time switches that differ from the shipped defaults; "" for a release build (tests assert exactly that)
  static const std::string flags = [] {
    std::string f;
#ifdef MTP_STAMPS
    f += "MTP_STAMPS ";
#endif
    f += mtp_kernel_build_flags();
    f += mtp_maxvol_build_flags();
    f += mtp_normal_build_flags();
    if (!f.empty() && f.back() == ' ') f.pop_back();
    return f;
  }();
  return flags.c_str();
}

int mtp_copy_neighbors_to_host(mtp_context *c, int *first, int *neigh)
{
  if (!c || !first) return MTP_ERR_ARG;
  if (!c->have_list || c->first != c->d_first.ptr || c->neigh != c->d_neigh.ptr) {
    if (c) c->last_error = "the current neighbour list is not owned by the context";
    return MTP_ERR_STATE;
  }
  (void) hipSetDevice(c->device);
  // the list was written on list_stream (a non-blocking stream: the copies below do not wait for it by themselves)
  if (hipStreamSynchronize(c->list_stream ? c->list_stream : c->stream) != hipSuccess) return MTP_ERR_DEVICE;
  if (hipMemcpy(first, c->d_first.ptr, sizeof(int) * ((size_t) c->inum + 1), hipMemcpyDeviceToHost) != hipSuccess)
    return MTP_ERR_DEVICE;
  if (neigh && first[c->inum] > 0 &&
      hipMemcpy(neigh, c->d_neigh.ptr, sizeof(int) * (size_t) first[c->inum], hipMemcpyDeviceToHost) != hipSuccess)
    return MTP_ERR_DEVICE;
  return MTP_OK;
}

int mtp_compute_device_rows(mtp_context *c, void *stream, int row_begin, int row_count, int finish_tallies,
                            const double *d_x, const int *d_type, int eflag, int vflag, int grade_flag, double *d_f,
                            double *d_eatom, double *d_vatom, double *d_ev, double *d_grades, double *d_max_grade,
                            double *d_coeff_ders)
{
  if (!c) return MTP_ERR_ARG;
  if (row_begin < 0 || row_count < 0 || (c->have_list && row_begin + row_count > c->inum))
    return fail(c, MTP_ERR_ARG, "row range outside the neighbour list");
  if (!c->have_list) return fail(c, MTP_ERR_STATE, "mtp_compute before mtp_set_neighbors");
  if (!d_x || !d_type || !d_f) return MTP_ERR_ARG;
  if (const int grc = mtp_internal_check_grade_args(c, grade_flag, d_grades, d_coeff_ders)) return grc;
  const bool cfg = c->pot->configuration_mode;
  if (((eflag & MTP_ENERGY_GLOBAL) || vflag) && finish_tallies && !d_ev) return MTP_ERR_ARG;
  if (c->inum == 0) return MTP_OK;
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  MtpDevParams p = c->base;
  p.inum = row_count;      // rows of THIS launch: [row0, row0 + inum) of the installed list
  p.row0 = row_begin;
  p.nall = c->nall;
  p.ilist = c->ilist;
  p.first = c->first;
  p.neigh = c->neigh;
  p.x = d_x;
  p.type = d_type;
  p.f = d_f;
  p.fq = nullptr;
  p.eatom = d_eatom;
  p.vatom = d_vatom;
  p.eflag = eflag;
  p.vflag = vflag;
  p.grade_flag = grade_flag ? 1 : 0;
  p.xcd_map = c->xcd_map && row_count >= 8 * 64 ? 1 : 0;
  const LaunchPlan &L = c->lp[grade_flag ? 2 : 0];
  const RowRange rr = plan_row_range(L, c->num_cus, row_count);
  apply_plan(p, L, *c->pot, grade_flag != 0);
  p.cvec = grade_flag ? c->d_cvec.ptr : nullptr;
  p.cpad = c->cpad;
  // the force kernel writes the radial block of the candidate vectors itself for the common table shape; other
  // shapes leave the adjoints of the basics in HBM for mtp_cvec_kernel
  const bool fused = grade_flag && c->pot->radial_basis_size == 8 && c->pot->radial_func_count <= 4 &&
      c->pot->species_count <= 2 && std::getenv("MTP_GRADE_UNFUSED") == nullptr;
  p.grade_fused = fused ? 1 : 0;
  p.dbasic = grade_flag && !fused ? c->d_dbasic.ptr : nullptr;
  p.dpad = c->dpad;
  try {
    if (c->timing) {
      if (!c->ev0) {
        HIP_CHECK(hipEventCreate(&c->ev0));
        HIP_CHECK(hipEventCreate(&c->ev1));
      }
      HIP_CHECK(hipEventRecord(c->ev0, st));
    }
    if (c->deterministic && row_count > 0) {
      const size_t n3 = 3 * (size_t) c->nall;
      if (c->d_fq.cap < n3) {
        c->d_fq.reserve(n3);
        HIP_CHECK(hipMemsetAsync(c->d_fq.ptr, 0, n3 * sizeof(long long), st));
      }
      p.fq = c->d_fq.ptr;
    }
    if (row_count > 0) {
      const char *used = nullptr;
      HIP_CHECK(mtp_launch_wave_kernel(p, rr.grid, rr.wpb, rr.lds_bytes, st, &used));
      c->last_shape = used ? used : "";
    }
    if (p.fq) HIP_CHECK(mtp_launch_fixed_to_force(p.fq, d_f, c->nall, st));
    if (c->timing) {
      HIP_CHECK(hipEventRecord(c->ev1, st));
      c->timed = true;
    }
    // the per-wavefront tally slots keep accumulating over the launches of a step; the last one folds them
    if (finish_tallies && ((eflag & MTP_ENERGY_GLOBAL) || vflag)) HIP_CHECK(mtp_launch_ev_finish(c->d_ev_slots.ptr, d_ev, st));
    if (grade_flag && row_count > 0) {
      if (!fused) {
        MtpDevParams pc = p;   // radial block of the candidate vectors from the adjoints left in HBM
        pc.blob_bytes = c->blob_sizes.norows;
        pc.rows_in_lds = 0;
        pc.wave_doubles = c->lp[1].wave_doubles;
        pc.tab_rows = c->lp[1].tab_rows;
        const RowRange rc1 = plan_cvec_range(c->lp[1], row_count);
        HIP_CHECK(mtp_launch_cvec_kernel(pc, rc1.grid, rc1.wpb, rc1.lds_bytes, st));
      }
      const double *cv = c->d_cvec.ptr + (size_t) row_begin * c->cpad;
      if (row_begin <= c->cvec_rows) c->cvec_rows = std::max(c->cvec_rows, row_begin + row_count);   // (no gap below)
      if (cfg)
        HIP_CHECK(mtp_launch_colsum_kernel(cv, c->cpad, c->pot->coeff_count, row_count, d_coeff_ders, st));
      else
        HIP_CHECK(mtp_launch_grade_kernel(cv, c->d_ainv_pad.ptr, c->d_ainv_tiled.ptr, c->cpad, c->pot->coeff_count, row_count,
                                          c->ilist + row_begin, d_grades, d_max_grade, st));
    }
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

int mtp_compute_device(mtp_context *c, void *stream, const double *d_x, const int *d_type, int eflag, int vflag,
                       int grade_flag, double *d_f, double *d_eatom, double *d_vatom, double *d_ev,
                       double *d_grades, double *d_max_grade, double *d_coeff_ders)
{
  if (!c) return MTP_ERR_ARG;
  return mtp_compute_device_rows(c, stream, 0, c->inum, 1, d_x, d_type, eflag, vflag, grade_flag, d_f, d_eatom, d_vatom,
                                 d_ev, d_grades, d_max_grade, d_coeff_ders);
}

// ---- batched configurations (include/mtp_mi355x.h) ----------------------------------------------------------------
int mtp_batch_reduce(void *stream, int ncfg, const int *d_cfg_first, const double *d_eatom, const double *d_vatom,
                     const double *d_grades, double *d_energy, double *d_virial, double *d_cfg_grade)
{
  if (ncfg < 0 || (ncfg > 0 && !d_cfg_first) || (d_energy && !d_eatom) || (d_virial && !d_vatom) || (d_cfg_grade && !d_grades))
    return MTP_ERR_ARG;
  if (!stream) return MTP_ERR_ARG;   // no context here: NULL is not mapped to anything (include/mtp_mi355x.h, "Streams")
  if (ncfg == 0) return MTP_OK;
  return mtp_launch_batch_reduce(ncfg, d_cfg_first, d_energy ? d_eatom : nullptr, d_virial ? d_vatom : nullptr,
                                 d_cfg_grade ? d_grades : nullptr, d_energy, d_virial, d_cfg_grade,
                                 reinterpret_cast<hipStream_t>(stream)) == hipSuccess
      ? MTP_OK
      : MTP_ERR_DEVICE;
}

int mtp_batch_cfg_grades(mtp_context *c, void *stream, int ncfg, const int *d_cfg_first, int nrows, double *d_cfg_grade)
{
  if (!c) return MTP_ERR_ARG;
  if (ncfg < 0 || nrows < 0 || (ncfg > 0 && (!d_cfg_first || !d_cfg_grade))) return MTP_ERR_ARG;
  if (!c->pot->has_selection || !c->pot->configuration_mode)
    return fail(c, MTP_ERR_STATE, "mtp_batch_cfg_grades: the potential carries no configuration-mode selection state");
  if (!c->have_list || nrows > c->inum || (size_t) nrows * c->cpad > c->d_cvec.cap)
    return fail(c, MTP_ERR_STATE,
                "mtp_batch_cfg_grades: no candidate vectors for these rows (call after a grade call on the installed list)");
  if (ncfg == 0) return MTP_OK;
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  try {
    c->d_csum.reserve((size_t) ncfg * c->cpad);
    c->d_ident.reserve((size_t) ncfg);
    HIP_CHECK(mtp_launch_batch_colsum(c->d_cvec.ptr, c->cpad, ncfg, d_cfg_first, c->d_csum.ptr, c->d_ident.ptr, st));
    HIP_CHECK(mtp_launch_grade_kernel(c->d_csum.ptr, c->d_ainv_pad.ptr, c->d_ainv_tiled.ptr, c->cpad, c->pot->coeff_count, ncfg,
                                      c->d_ident.ptr, d_cfg_grade, nullptr, st));
    HIP_CHECK(mtp_launch_batch_grade_scale(ncfg, d_cfg_first, d_cfg_grade, st));
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

// ---- design rows of the linear refit (include/mtp_mi355x.h) ----------------------------------------------------------
// builds and uploads the table of both kinds of call; `train`: the call is a training call (a design call succeeds on a
// table the training formulas refuse; a training call is refused every time, with the same code and message)
static int centre_prepare(mtp_context *c, hipStream_t st, bool train)
{
  if (!c->centre_ready) {
    const mtp_potential &pot = *c->pot;
    const std::string who = train ? "training gradient" : "design rows";
    mtp_train_table built;   // (its design part is filled either way)
    std::string tmsg;
    int trc = mtp_build_train_table(pot, built, tmsg);
    const mtp_train_table &t = built;
    const mtp_design_table &dt = t.design;
    if (train && trc != MTP_OK) {
      c->last_error = tmsg;
      return trc;
    }
    if (dt.A > 8191)
      return fail(c, MTP_ERR_LIMIT, who + ": alpha_moments_count above 8191 is not supported by the packed times rows");
    if (trc == MTP_OK && (pot.radial_func_count > 16 || pot.max_alpha_index_basic > 16)) {
      trc = MTP_ERR_LIMIT;
      tmsg = "training gradient: radial_funcs_count or a basic index above 16 does not fit the packed basics";
      if (train) {
        c->last_error = tmsg;
        return trc;
      }
    }
    std::vector<MtpRow8> rows8;
    if (pack_rows(dt.rows, rows8))
      return fail(c, MTP_ERR_LIMIT, who + ": a multiplicity of alpha_index_times does not fit 16 bits");
    std::vector<int32_t> ints(dt.level_offset);
    for (const std::vector<int32_t> *v : {&dt.basic_pack, &dt.scalar_map, &dt.force_map, &t.bymu, &t.mufirst})
      ints.insert(ints.end(), v->begin(), v->end());
    c->d_centre_rows.upload(rows8, st);
    c->d_centre_ints.upload(ints, st);
    c->d_design_radial.upload(c->h_radial, st);   // (the context's values: an install may precede the first call)
    HIP_CHECK(hipStreamSynchronize(st));   // (the staging vectors go out of scope)
    MtpCentreParams &d = c->centre;
    d = MtpCentreParams{};
    d.Sp = pot.species_count;
    d.R = pot.radial_basis_size;
    d.Mu = pot.radial_func_count;
    d.P = pot.max_alpha_index_basic;
    d.A = dt.A;
    d.B = dt.B;
    d.S = dt.S;
    d.nblocks = dt.nblocks;
    d.rmin = pot.min_cutoff;
    d.rmax = pot.max_cutoff;
    d.scaling = pot.scaling;
    d.cutsq = pot.max_cutoff * pot.max_cutoff;
    d.inv_span = 1.0 / (pot.max_cutoff - pot.min_cutoff);
    d.rows = c->d_centre_rows.ptr;
    d.level = c->d_centre_ints.ptr;
    d.pack = d.level + dt.level_offset.size();
    d.map = d.pack + dt.B;
    c->centre_fmap = d.map + dt.S;
    c->centre_bymu = c->centre_fmap + dt.S;
    c->centre_mufirst = c->centre_bymu + dt.B;
    d.err_flag = c->d_err.ptr;
    c->train_rc = trc;
    c->train_msg = tmsg;
    c->centre_ready = true;
  }
  if (train && c->train_rc != MTP_OK) c->last_error = c->train_msg;
  return train ? c->train_rc : MTP_OK;
}

// the table and the system of one call
static void centre_bind(const mtp_context *c, MtpCentreParams &p, const double *d_x, const int *d_type, int row_begin, int row_count,
                        const int *d_owner, int nowned, int ld)
{
  p = c->centre;
  p.row0 = row_begin;
  p.nrows = row_count;
  p.nowned = nowned;
  p.nall = c->nall;
  p.ld = ld;
  p.cj_cap = std::max(c->max_numneigh, 1);
  p.ilist = c->ilist;
  p.first = c->first;
  p.neigh = c->neigh;
  p.type = d_type;
  p.owner = d_owner;
  p.x = d_x;
}

// the workgroups of a launch whose LDS image takes `lds` bytes, or the refusal of an image beyond the CU's 160 KB: `fixed`
// gives the caller's sentence for an image that is too large without the list's ids
static int centre_grid(mtp_context *c, const std::string &who, size_t lds, int cj_cap, int row_count, int *grid,
                       const std::function<std::string()> &fixed)
{
  if (lds > CU_LDS_BYTES) {
    c->last_error = who + ": the workgroup's LDS image needs " + std::to_string(lds) + " of 163840 bytes: " +
        (lds - (size_t) cj_cap * sizeof(int) > CU_LDS_BYTES
             ? fixed()
             : "the list's longest row, max_numneigh = " + std::to_string(c->max_numneigh) + ", is too large");
    return MTP_ERR_LIMIT;
  }
  const int per_cu = (int) std::max<size_t>(1, std::min<size_t>(8, CU_LDS_BYTES / lds));
  *grid = std::max(1, std::min(row_count, c->num_cus * per_cu));
  return MTP_OK;
}

int mtp_design_rows_device(mtp_context *c, void *stream, const double *d_x, const int *d_type, int row_begin, int row_count,
                           const int *d_owner, int ld, double *d_basis, double *d_force, int nowned, double *d_virial_atom)
{
  if (!c) return MTP_ERR_ARG;
  if (!c->have_list) return fail(c, MTP_ERR_STATE, "mtp_design_rows_device before a neighbour list is installed");
  const int cols = c->pot->species_count + c->pot->alpha_scalar_count;
  if (ld < cols || (ld & 1))
    return fail(c, MTP_ERR_ARG,
                "mtp_design_rows_device: ld = " + std::to_string(ld) + " must be even and at least Sp + S = " + std::to_string(cols));
  if (row_begin < 0 || row_count < 0 || row_begin + row_count > c->inum || nowned < 0)
    return fail(c, MTP_ERR_ARG, "mtp_design_rows_device: row range outside the neighbour list, or nowned < 0");
  if (row_count > 0 && (!d_x || !d_type || !d_force))
    return fail(c, MTP_ERR_ARG, "mtp_design_rows_device: positions, types and the force rows are required");
  if (row_count == 0) return MTP_OK;
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  try {
    int rc = centre_prepare(c, st, false), grid = 0;
    if (rc != MTP_OK) return rc;
    MtpDesignParams p{};
    centre_bind(c, p, d_x, d_type, row_begin, row_count, d_owner, nowned, ld);
    p.fmap = c->centre_fmap;
    p.radial = c->d_design_radial.ptr;
    p.basis = d_basis;
    p.force = d_force;
    p.virial = d_virial_atom;
    const size_t lds = mtp_design_lds_layout(p);
    rc = centre_grid(c, "mtp_design_rows_device", lds, p.cj_cap, row_count, &grid, [&] {
      return std::to_string(MTP_DESIGN_WAVES + 1) + " moment images of alpha_moments_count = " + std::to_string(p.A) +
          " doubles and nine rows of alpha_scalar_moments = " + std::to_string(p.S) + " are too large";
    });
    if (rc != MTP_OK) return rc;
    HIP_CHECK(mtp_launch_design_kernel(p, grid, lds, st));
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

int mtp_batch_design_reduce(void *stream, int ncfg, const int *d_cfg_first, int ld, const double *d_basis,
                            const double *d_virial_atom, double *d_energy, double *d_virial)
{
  if (ncfg < 0 || ld < 1 || (ncfg > 0 && !d_cfg_first) || (d_energy && !d_basis) || (d_virial && !d_virial_atom)) return MTP_ERR_ARG;
  if (!stream) return MTP_ERR_ARG;   // no context here: NULL is not mapped to anything (include/mtp_mi355x.h, "Streams")
  if (ncfg == 0 || (!d_energy && !d_virial)) return MTP_OK;
  return mtp_launch_batch_design_reduce(ncfg, d_cfg_first, ld, d_basis, d_virial_atom, d_energy, d_virial,
                                        reinterpret_cast<hipStream_t>(stream)) == hipSuccess
      ? MTP_OK
      : MTP_ERR_DEVICE;
}

// ---- training gradient (include/mtp_mi355x.h) -------------------------------------------------------------------------
// the checks and the launch both training calls share; `who` names the call in messages
static int train_launch(mtp_context *c, const char *who, bool vjp, void *stream, const double *d_x, const int *d_type, int row_begin,
                        int row_count, const int *d_owner, const double *d_theta, int nowned, MtpTrainParams io, int ld)
{
  if (!c) return MTP_ERR_ARG;
  const std::string w(who);
  if (!c->have_list) return fail(c, MTP_ERR_STATE, w + " before a neighbour list is installed");
  const mtp_potential &pot = *c->pot;
  const int cols = pot.species_count * pot.species_count * pot.radial_func_count * pot.radial_basis_size + pot.species_count +
      pot.alpha_scalar_count;
  if (vjp && (ld < cols || (ld & 1)))
    return fail(c, MTP_ERR_ARG, w + ": ld = " + std::to_string(ld) + " must be even and at least C = " + std::to_string(cols));
  if (row_begin < 0 || row_count < 0 || row_begin + row_count > c->inum || nowned < 0)
    return fail(c, MTP_ERR_ARG, w + ": row range outside the neighbour list, or nowned < 0");
  if (row_count > 0 && (!d_x || !d_type || !d_theta || (vjp ? !io.grad : !io.force)))
    return fail(c, MTP_ERR_ARG,
                w + ": positions, types, theta and " + (vjp ? "the gradient rows" : "the force array") + " are required");
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  try {
    int rc = centre_prepare(c, st, true), grid = 0;   // (a refused table is reported even for an empty row range)
    if (rc != MTP_OK) return rc;
    if (row_count == 0) return MTP_OK;
    MtpTrainParams p = io;   // (the caller's outputs and cotangents)
    centre_bind(c, p, d_x, d_type, row_begin, row_count, d_owner, nowned, ld);
    p.bymu = c->centre_bymu;
    p.mufirst = c->centre_mufirst;
    p.theta = d_theta;
    const size_t lds = mtp_train_lds_layout(p);
    rc = centre_grid(c, w, lds, p.cj_cap, row_count, &grid, [&] {
      return "four moment images of alpha_moments_count = " + std::to_string(p.A) + " doubles and " + std::to_string(p.tab_rows) +
          " table rows are too large";
    });
    if (rc != MTP_OK) return rc;
    HIP_CHECK(mtp_launch_train_kernel(p, vjp, grid, lds, st));
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

int mtp_train_value_device(mtp_context *c, void *stream, const double *d_x, const int *d_type, int row_begin, int row_count,
                           const int *d_owner, const double *d_theta, double *d_eatom, double *d_force, int nowned,
                           double *d_vatom)
{
  MtpTrainParams io{};
  io.eatom = d_eatom;
  io.force = d_force;
  io.vatom = d_vatom;
  return train_launch(c, "mtp_train_value_device", false, stream, d_x, d_type, row_begin, row_count, d_owner, d_theta, nowned, io, 0);
}

int mtp_train_vjp_device(mtp_context *c, void *stream, const double *d_x, const int *d_type, int row_begin, int row_count,
                         const int *d_owner, const double *d_theta, const double *d_ebar, const double *d_fbar, int nowned,
                         const double *d_vbar, int ld, double *d_grad_rows)
{
  MtpTrainParams io{};
  io.ebar = d_ebar;
  io.fbar = d_fbar;
  io.vbar = d_vbar;
  io.grad = d_grad_rows;
  return train_launch(c, "mtp_train_vjp_device", true, stream, d_x, d_type, row_begin, row_count, d_owner, d_theta, nowned, io, ld);
}

// ---- MaxVol selection (include/mtp_mi355x.h) -------------------------------------------------------------------------
int mtp_context_candidates_device(const mtp_context *c, const double **d_rows, int *nrows, int *ld)
{
  if (!c || !d_rows || !nrows || !ld) return MTP_ERR_ARG;
  if (!c->pot->has_selection || !c->have_list || c->cvec_rows <= 0 || (size_t) c->cvec_rows * c->cpad > c->d_cvec.cap)
    return MTP_ERR_STATE;   // (const context: no message) no grade call on the installed list yet
  *d_rows = c->d_cvec.ptr;
  *nrows = c->cvec_rows;
  *ld = c->cpad;
  return MTP_OK;
}

int mtp_batch_cfg_candidates(mtp_context *c, void *stream, int ncfg, const int *d_cfg_first, int nrows, const double **d_rows,
                             int *ld)
{
  if (!c) return MTP_ERR_ARG;
  if (ncfg < 0 || nrows < 0 || !d_rows || !ld || (ncfg > 0 && !d_cfg_first)) return MTP_ERR_ARG;
  if (!c->pot->has_selection) return fail(c, MTP_ERR_STATE, "mtp_batch_cfg_candidates: the potential carries no selection state");
  if (!c->have_list || nrows > c->cvec_rows || (size_t) nrows * c->cpad > c->d_cvec.cap)
    return fail(c, MTP_ERR_STATE,
                "mtp_batch_cfg_candidates: no candidate vectors for these rows (call after a grade call on the installed list)");
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  try {
    c->d_csum.reserve((size_t) std::max(ncfg, 1) * c->cpad);
    c->d_ident.reserve((size_t) std::max(ncfg, 1));
    if (ncfg > 0) {
      HIP_CHECK(mtp_launch_batch_colsum(c->d_cvec.ptr, c->cpad, ncfg, d_cfg_first, c->d_csum.ptr, c->d_ident.ptr, st));
      HIP_CHECK(mtp_launch_maxvol_scale_rows(c->d_csum.ptr, c->cpad, ncfg, d_cfg_first, st));
    }
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  *d_rows = c->d_csum.ptr;
  *ld = c->cpad;
  return MTP_OK;
}

int mtp_maxvol_select(mtp_context *c, void *stream, const double *d_rows, long long nrows, int ld, double threshold,
                      int max_swaps, int refresh, double *active_set, double *inverse_active_set, int *slot_source,
                      int *swap_rows, int *swap_slots, double *swap_pivots, int *nswaps, int *converged,
                      double *log_volume_gain, double *max_grade_after)
{
  if (!c) return MTP_ERR_ARG;
  const mtp_potential &p = *c->pot;
  if (!p.has_selection) return fail(c, MTP_ERR_STATE, "mtp_maxvol_select: the potential carries no selection state");
  const int C = p.coeff_count;
  if (!(threshold >= 1.0) || !std::isfinite(threshold) || nrows < 0 || ld < C || max_swaps < 0 || refresh < 1 ||
      (nrows > 0 && !d_rows) || !active_set || !inverse_active_set || !slot_source || !nswaps || !converged ||
      (max_swaps > 0 && (!swap_rows || !swap_slots || !swap_pivots))) {
    c->last_error = "mtp_maxvol_select: needs threshold >= 1, ld >= coeff_count, max_swaps >= 0, refresh >= 1 and its outputs";
    return MTP_ERR_ARG;
  }
  if (nrows * (long long) C > (1ll << 62) / C) return fail(c, MTP_ERR_LIMIT, "mtp_maxvol_select: too many rows");
  double mg = 0.0;
  int bad = 0;
  *nswaps = 0;
  *converged = 1;
  if (nrows == 0) {   // nothing to select from: the context's own blocks (the potential's until an install), bit for bit
    std::memcpy(active_set, c->h_active_set.data(), c->h_active_set.size() * sizeof(double));
    std::memcpy(inverse_active_set, c->h_inverse.data(), c->h_inverse.size() * sizeof(double));
    for (int j = 0; j < C; j++) slot_source[j] = -1;
  } else {
    if (!set_device(c)) return MTP_ERR_DEVICE;
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    hipError_t e = hipSuccess;
    try {   // the arena is the context's and is kept: a selection loop allocates once
      c->d_maxvol.reserve(mtp_maxvol_arena_doubles(c->num_cus, C, nrows, max_swaps));
      e = mtp_maxvol_run(st, c->num_cus, c->d_maxvol.ptr, C, c->h_active_set.data(), c->h_inverse.data(), d_rows, nrows,
                         ld, threshold, max_swaps, refresh, active_set, inverse_active_set, slot_source, swap_rows, swap_slots,
                         swap_pivots, nswaps, converged, &mg, &bad);
    } catch (const HipFail &f) {
      e = f.e;
    } catch (const std::bad_alloc &) {
      c->last_error = "mtp_maxvol_select: out of host memory";
      return MTP_ERR_LIMIT;
    }
    if (e != hipSuccess) {
      c->last_error = std::string("mtp_maxvol_select: ") + hipGetErrorString(e);
      return e == hipErrorOutOfMemory ? MTP_ERR_LIMIT : MTP_ERR_DEVICE;
    }
  }
  double gain = 0.0;
  for (int k = 0; k < *nswaps; k++) gain += std::log(std::fabs(swap_pivots[k]));
  if (log_volume_gain) *log_volume_gain = gain;
  if (max_grade_after) *max_grade_after = mg;
  if (bad) return fail(c, MTP_ERR_ARG, "mtp_maxvol_select: a candidate vector (or a grade computed from it) is not finite");
  return MTP_OK;
}

// ---- installs into a live context (include/mtp_mi355x.h) ----------------------------------------------------------------
namespace {

// the checks of an install of coefficients, with nothing written: the tables a context of these values reads
int check_coeffs(mtp_context *c, const char *who, const double *radial, const double *species, const double *moments,
                 mtp_coeff_tables &t)
{
  const mtp_potential &p = *c->pot;
  if (!all_finite(radial, p.radial_basis_coeffs.size()) || !all_finite(species, p.species_coeffs.size()) ||
      !all_finite(moments, p.linear_coeffs.size())) {
    c->last_error = std::string(who) + ": a coefficient is not finite";
    return MTP_ERR_ARG;
  }
  mtp_build_coeff_tables(p, radial ? radial : c->h_radial.data(), species ? species : c->h_species.data(),
                         moments ? moments : c->h_moments.data(), t);
  if (c->base.off_leaf_cb == c->base.off_leaf_cf && t.leaf_cb != t.leaf_cf) {
    c->last_error = std::string(who) + ": the context was created on values whose leaf rows have one constant for the energy and "
        "the adjoint, and its table blob holds one table for both; the new moment coefficients make them differ (two scalars on "
        "one leaf moment): load the file instead";
    return MTP_ERR_UNSUPPORTED;
  }
  return MTP_OK;
}

int check_selection(mtp_context *c, const char *who, const double *active_set, const double *inverse_active_set, int coeff_count)
{
  const mtp_potential &p = *c->pot;
  if (!p.has_selection)
    return fail(c, MTP_ERR_STATE, std::string(who) + ": the context's potential was loaded without its selection state");
  if (!active_set || !inverse_active_set || coeff_count != p.coeff_count)
    return fail(c, MTP_ERR_ARG, std::string(who) + ": needs both blocks, and coeff_count = " + std::to_string(p.coeff_count));
  const size_t n = (size_t) p.coeff_count * p.coeff_count;
  if (!all_finite(active_set, n) || !all_finite(inverse_active_set, n))
    return fail(c, MTP_ERR_ARG, std::string(who) + ": an entry of the active set or of its inverse is not finite");
  return MTP_OK;
}

// An install in three steps, so that one call waits ONCE however much it installs: queue_* issue the copies into every
// device copy of the tables from staging memory the caller keeps alive, the caller drains the stream, and
// commit_* replace the context's host copies.  queue_* throw HipFail.
void queue_coeffs(mtp_context *c, hipStream_t st, const mtp_coeff_tables &t)
{
  auto put = [&](void *dst, const std::vector<double> &v) {
    if (!v.empty()) HIP_CHECK(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, st));
  };
  const MtpDevParams &b = c->base;
  unsigned char *blob = c->d_blob.ptr;
  put(blob + b.off_radial, t.radial);
  if (b.scalars_in_lds) {
    put(blob + b.off_seed_val, t.seed_val);
    put(blob + b.off_lin, t.e_lin);
  }
  put(blob + b.off_leaf_cf, t.leaf_cf);
  if (b.off_leaf_cb != b.off_leaf_cf) put(blob + b.off_leaf_cb, t.leaf_cb);
  put(c->d_seed_val.ptr, t.seed_val);
  put(c->d_lin.ptr, t.e_lin);
  put(c->d_leaf_cf.ptr, t.leaf_cf);
  put(c->d_leaf_cb.ptr, t.leaf_cb);
  put(c->d_species.ptr, t.species);
  if (c->centre_ready) put(c->d_design_radial.ptr, t.radial);
}

void commit_coeffs(mtp_context *c, const mtp_coeff_tables &t, const double *moments)
{
  c->h_radial = t.radial;
  c->h_species = t.species;
  if (moments) c->h_moments.assign(moments, moments + c->h_moments.size());
}

struct StagedSelection {
  std::vector<double> pad, tiled;
};

void queue_selection(mtp_context *c, hipStream_t st, const double *inverse_active_set, StagedSelection &stage)
{
  pad_and_tile(inverse_active_set, c->pot->coeff_count, c->cpad, stage.pad, stage.tiled);
  HIP_CHECK(hipMemcpyAsync(c->d_ainv_pad.ptr, stage.pad.data(), stage.pad.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(c->d_ainv_tiled.ptr, stage.tiled.data(), stage.tiled.size() * sizeof(double), hipMemcpyHostToDevice, st));
}

void commit_selection(mtp_context *c, const double *active_set, const double *inverse_active_set)
{
  const size_t n = (size_t) c->pot->coeff_count * c->pot->coeff_count;
  c->h_active_set.assign(active_set, active_set + n);
  c->h_inverse.assign(inverse_active_set, inverse_active_set + n);
}

}   // namespace

int mtp_context_install_coeffs(mtp_context *c, void *stream, const double *radial_coeffs, const double *species_coeffs,
                               const double *moment_coeffs)
{
  if (!c) return MTP_ERR_ARG;
  mtp_coeff_tables t;
  const int rc = check_coeffs(c, "mtp_context_install_coeffs", radial_coeffs, species_coeffs, moment_coeffs, t);
  if (rc != MTP_OK) return rc;
  if (!set_device(c)) return MTP_ERR_DEVICE;
  try {
    hipStream_t st = reinterpret_cast<hipStream_t>(mtp_internal_resolve_stream(c, stream));
    queue_coeffs(c, st, t);
    HIP_CHECK(hipStreamSynchronize(st));   // the one wait: earlier work on the stream and these copies
    commit_coeffs(c, t, moment_coeffs);
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

int mtp_context_install_selection(mtp_context *c, void *stream, const double *active_set, const double *inverse_active_set,
                                  int coeff_count)
{
  if (!c) return MTP_ERR_ARG;
  const int rc = check_selection(c, "mtp_context_install_selection", active_set, inverse_active_set, coeff_count);
  if (rc != MTP_OK) return rc;
  if (!set_device(c)) return MTP_ERR_DEVICE;
  try {
    hipStream_t st = reinterpret_cast<hipStream_t>(mtp_internal_resolve_stream(c, stream));
    StagedSelection stage;
    queue_selection(c, st, inverse_active_set, stage);
    HIP_CHECK(hipStreamSynchronize(st));
    commit_selection(c, active_set, inverse_active_set);
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

int mtp_context_install_file(mtp_context *c, void *stream, const char *path)
{
  if (!c || !path) return MTP_ERR_ARG;
  const mtp_potential &p = *c->pot;
  // the gate is mtp_potential_compatible's: one text parse, no schedule.  A file with NO #MVS tail at all (what the
  // coefficient writers leave) still installs its coefficients into a context that has a selection state; a tail that is
  // there but does not read (wrong version, a weight line missing, short blocks) is the parser's error.
  mtp_potential file;
  std::string msg;
  bool with_selection = p.has_selection;
  int rc = mtp_parse_text_file(path, with_selection, file, msg);
  if (rc == MTP_ERR_SELECTION && with_selection && file.selection_absent) {   // (a damaged tail stays an error)
    with_selection = false;
    file = mtp_potential();
    msg.clear();
    rc = mtp_parse_text_file(path, false, file, msg);
  }
  if (rc == MTP_OK) rc = mtp_check_compatible(p, file, with_selection, msg);
  if (rc != MTP_OK) {
    c->last_error = "mtp_context_install_file: " + msg;
    return rc;
  }
  mtp_coeff_tables t;
  rc = check_coeffs(c, "mtp_context_install_file", file.radial_basis_coeffs.data(), file.species_coeffs.data(),
                    file.linear_coeffs.data(), t);
  if (rc == MTP_OK && with_selection)
    rc = check_selection(c, "mtp_context_install_file", file.active_set.data(), file.inverse_active_set.data(), file.coeff_count);
  if (rc != MTP_OK) return rc;
  if (!set_device(c)) return MTP_ERR_DEVICE;
  try {
    hipStream_t st = reinterpret_cast<hipStream_t>(mtp_internal_resolve_stream(c, stream));
    StagedSelection stage;
    queue_coeffs(c, st, t);
    if (with_selection) queue_selection(c, st, file.inverse_active_set.data(), stage);
    HIP_CHECK(hipStreamSynchronize(st));   // one wait for both
    commit_coeffs(c, t, file.linear_coeffs.data());
    if (with_selection) commit_selection(c, file.active_set.data(), file.inverse_active_set.data());
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

int mtp_context_get_coeffs(const mtp_context *c, double *radial_coeffs, double *species_coeffs, double *moment_coeffs)
{
  if (!c) return MTP_ERR_ARG;
  auto cp = [](double *dst, const std::vector<double> &v) {
    if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(double));
  };
  cp(radial_coeffs, c->h_radial);
  cp(species_coeffs, c->h_species);
  cp(moment_coeffs, c->h_moments);
  return MTP_OK;
}

int mtp_context_get_selection(const mtp_context *c, double *active_set, double *inverse_active_set)
{
  if (!c) return MTP_ERR_ARG;
  if (!c->pot->has_selection) return MTP_ERR_STATE;
  if (active_set) std::memcpy(active_set, c->h_active_set.data(), c->h_active_set.size() * sizeof(double));
  if (inverse_active_set) std::memcpy(inverse_active_set, c->h_inverse.data(), c->h_inverse.size() * sizeof(double));
  return MTP_OK;
}

int mtp_context_cfg_grade(const mtp_context *c, const double *coeff_ders, double *grade)
{
  if (!c || !coeff_ders || !grade) return MTP_ERR_ARG;
  if (!c->pot->has_selection) return MTP_ERR_STATE;
  *grade = cfg_grade_of(c->h_inverse.data(), c->pot->coeff_count, coeff_ders);
  return MTP_OK;
}

int mtp_context_coeff_tables_device(mtp_context *c, void *stream, int32_t *counts, double *blob_radial, double *blob_seed_val,
                                    double *blob_e_lin, double *blob_leaf_cf, double *blob_leaf_cb, double *hbm_seed_val,
                                    double *hbm_e_lin, double *hbm_leaf_cf, double *hbm_leaf_cb, double *species,
                                    double *design_radial, double *ainv_pad, double *ainv_tiled)
{
  if (!c) return MTP_ERR_ARG;
  const mtp_potential &p = *c->pot;
  const MtpDevParams &b = c->base;
  const size_t n_rad = p.radial_basis_coeffs.size(), n_seed = p.seed_val.size(), n_lin = p.e_lin.size(), n_leaf = p.leaf_cf.size();
  const size_t n_w = p.has_selection ? (size_t) c->cpad * c->cpad : 0;
  if (counts) {
    const size_t v[10] = {n_rad, n_seed, n_lin, n_leaf, n_leaf, p.species_coeffs.size(), c->centre_ready ? n_rad : 0, n_w, n_w,
                          (size_t) (b.scalars_in_lds ? 1 : 0)};
    for (int k = 0; k < 10; k++) counts[k] = (int32_t) v[k];
  }
  if (!set_device(c)) return MTP_ERR_DEVICE;
  hipStream_t st = reinterpret_cast<hipStream_t>(mtp_internal_resolve_stream(c, stream));
  try {
    auto get = [&](double *dst, const void *src, size_t n) {
      if (dst && n) HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, st));
    };
    const unsigned char *blob = c->d_blob.ptr;
    get(blob_radial, blob + b.off_radial, n_rad);
    if (b.scalars_in_lds) {
      get(blob_seed_val, blob + b.off_seed_val, n_seed);
      get(blob_e_lin, blob + b.off_lin, n_lin);
    }
    get(blob_leaf_cf, blob + b.off_leaf_cf, n_leaf);
    get(blob_leaf_cb, blob + b.off_leaf_cb, n_leaf);
    get(hbm_seed_val, c->d_seed_val.ptr, n_seed);
    get(hbm_e_lin, c->d_lin.ptr, n_lin);
    get(hbm_leaf_cf, c->d_leaf_cf.ptr, n_leaf);
    get(hbm_leaf_cb, c->d_leaf_cb.ptr, n_leaf);
    get(species, c->d_species.ptr, p.species_coeffs.size());
    if (c->centre_ready) get(design_radial, c->d_design_radial.ptr, n_rad);
    get(ainv_pad, c->d_ainv_pad.ptr, n_w);
    get(ainv_tiled, c->d_ainv_tiled.ptr, n_w);
    HIP_CHECK(hipStreamSynchronize(st));
  } catch (const HipFail &f) {
    return device_fail(c, f);
  }
  return MTP_OK;
}

int mtp_synchronize(mtp_context *c, void *stream)
{
  if (!c) return MTP_ERR_ARG;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  int flag = 0;
  hipError_t e = hipMemcpyAsync(&flag, c->d_err.ptr, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(c, MTP_ERR_DEVICE, std::string("synchronize: ") + hipGetErrorString(e));
  if (flag) {
    (void) hipMemsetAsync(c->d_err.ptr, 0, sizeof(int), st);
    (void) hipStreamSynchronize(st);
    if (flag == 2)
      return fail(c, MTP_ERR_LIMIT, "a neighbour list row holds more in-cutoff neighbours than the declared max_numneigh");
    if (flag == 3)
      return fail(c, MTP_ERR_ARG, "design rows: a centre or an owner outside [0, nowned), or a list entry outside [0, nall)");
    c->last_error = "Too few species count in the MTP potential!";   // pair_mtp.cpp:92-93
    return MTP_ERR_SPECIES;
  }
  return MTP_OK;
}

int mtp_compute(mtp_context *c, const double *x, const int *type, int eflag, int vflag, int grade_flag,
                double *f, double *eatom, double *vatom, double *energy, double *virial, double *grades,
                double *max_grade, double *coeff_ders)
{
  if (!c || !x || !type || !f) return MTP_ERR_ARG;
  if (!c->have_list) return fail(c, MTP_ERR_STATE, "mtp_compute before mtp_set_neighbors");
  const size_t nall = (size_t) c->nall;
  try {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    c->d_x.upload(x, 3 * nall, st);
    c->d_type.upload(type, nall, st);
    c->d_f.reserve(3 * nall);
    HIP_CHECK(hipMemsetAsync(c->d_f.ptr, 0, 3 * nall * sizeof(double), st));
    const bool want_ea = (eflag & MTP_ENERGY_ATOM) && eatom;
    const bool want_va = (vflag & MTP_VIRIAL_ATOM) && vatom;
    if (want_ea) c->d_eatom.upload(eatom, nall, st);   // keeps entries of atoms outside ilist
    if (want_va) {
      c->d_vatom.reserve(6 * nall);
      HIP_CHECK(hipMemsetAsync(c->d_vatom.ptr, 0, 6 * nall * sizeof(double), st));
    }
    HIP_CHECK(hipMemsetAsync(c->d_ev.ptr, 0, 8 * sizeof(double), st));
    if (grade_flag) {
      c->d_grades.reserve(nall);
      c->d_coeff.reserve((size_t) c->pot->coeff_count);
      HIP_CHECK(hipMemsetAsync(c->d_grades.ptr, 0, nall * sizeof(double), st));
      HIP_CHECK(hipMemsetAsync(c->d_coeff.ptr, 0, (size_t) c->pot->coeff_count * sizeof(double), st));
      HIP_CHECK(hipMemsetAsync(c->d_maxg.ptr, 0, sizeof(double), st));
    }
    int rc = mtp_compute_device(c, st, c->d_x.ptr, c->d_type.ptr, eflag, vflag, grade_flag, c->d_f.ptr,
                                want_ea ? c->d_eatom.ptr : nullptr, want_va ? c->d_vatom.ptr : nullptr,
                                c->d_ev.ptr, grade_flag ? c->d_grades.ptr : nullptr,
                                grade_flag ? c->d_maxg.ptr : nullptr, grade_flag ? c->d_coeff.ptr : nullptr);
    if (rc != MTP_OK) return rc;
    c->h_tmp.resize(std::max<size_t>(6 * nall, 16));
    HIP_CHECK(hipMemcpyAsync(c->h_tmp.data(), c->d_f.ptr, 3 * nall * sizeof(double), hipMemcpyDeviceToHost, st));
    rc = mtp_synchronize(c, st);
    if (rc != MTP_OK) return rc;
    for (size_t q = 0; q < 3 * nall; q++) f[q] += c->h_tmp[q];
    if (want_ea) HIP_CHECK(hipMemcpy(eatom, c->d_eatom.ptr, nall * sizeof(double), hipMemcpyDeviceToHost));
    if (want_va) {
      HIP_CHECK(hipMemcpy(c->h_tmp.data(), c->d_vatom.ptr, 6 * nall * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t q = 0; q < 6 * nall; q++) vatom[q] += c->h_tmp[q];
    }
    double ev[8];
    HIP_CHECK(hipMemcpy(ev, c->d_ev.ptr, 8 * sizeof(double), hipMemcpyDeviceToHost));
    if ((eflag & MTP_ENERGY_GLOBAL) && energy) *energy += ev[0];
    if (vflag && virial)
      for (int q = 0; q < 6; q++) virial[q] += ev[1 + q];
    if (grade_flag) {
      if (grades) HIP_CHECK(hipMemcpy(grades, c->d_grades.ptr, nall * sizeof(double), hipMemcpyDeviceToHost));
      if (max_grade) HIP_CHECK(hipMemcpy(max_grade, c->d_maxg.ptr, sizeof(double), hipMemcpyDeviceToHost));
      if (coeff_ders)
        HIP_CHECK(hipMemcpy(coeff_ders, c->d_coeff.ptr, (size_t) c->pot->coeff_count * sizeof(double),
                            hipMemcpyDeviceToHost));
    }
  } catch (const HipFail &fl) {
    return device_fail(c, fl);
  }
  return MTP_OK;
}

int mtp_context_launch_info(const mtp_context *c, int32_t *lds_bytes_per_wave, int32_t *waves_per_block,
                            int32_t *grid_blocks, int32_t *neighbor_tile)
{
  if (!c || !c->have_list) return MTP_ERR_STATE;
  const LaunchPlan &L = c->lp[0];
  if (lds_bytes_per_wave) *lds_bytes_per_wave = L.wave_doubles * 8;   // per atom image
  if (waves_per_block) *waves_per_block = L.wpb;
  if (grid_blocks) *grid_blocks = L.grid;
  if (neighbor_tile) *neighbor_tile = c->base.NT;
  return MTP_OK;
}

int mtp_context_plan_info(const mtp_context *c, int32_t *waves_per_simd, int32_t *rebuild_tables)
{
  if (!c || !c->have_list) return MTP_ERR_STATE;
  if (waves_per_simd) *waves_per_simd = c->lp[0].wps;
  if (rebuild_tables) *rebuild_tables = c->lp[0].rebuild ? 1 : 0;
  return MTP_OK;
}

int mtp_context_layout_mode(const mtp_context *c, int32_t *mode)
{
  if (!c || !c->have_list) return MTP_ERR_STATE;
  if (mode) *mode = c->lp[0].layout.mode;
  return MTP_OK;
}

// diagnostic builds only: read and clear the per-phase cycle sums (not part of the public ABI)
int mtp_debug_read_stamps(mtp_context *c, unsigned long long *out16)
{
  if (!c || !out16) return MTP_ERR_ARG;
  if (hipMemcpy(out16, c->d_stamps.ptr, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return MTP_ERR_DEVICE;
  (void) hipMemset(c->d_stamps.ptr, 0, 16 * sizeof(unsigned long long));
  return MTP_OK;
}

#ifdef MTP_STAMPS
// the per-wavefront phase trace of the last force launch (mtp_device.hpp, MTP_TRACE_*): `words` must be MTP_TRACE_WORDS
int mtp_debug_read_trace(mtp_context *c, unsigned long long *out, int words)
{
  if (!c || !out || words != MTP_TRACE_WORDS) return MTP_ERR_ARG;
  if (hipMemcpy(out, c->d_stamps.ptr + 16, (size_t) words * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
    return MTP_ERR_DEVICE;
  return MTP_OK;
}
#endif

}   // extern "C"

// ---- the plan without a device (mtp_plan.cpp; the name of a fixed-shape kernel belongs to the kernel unit) --------------
extern "C" {

int mtp_plan_fixed_shape(const mtp_potential *pot, int num_cus, int inum, int max_numneigh, int variant, int grade,
                         char *name, int namelen)
{
  MtpDevParams p;
  int rc = plan_params(pot, num_cus, inum, max_numneigh, variant, grade, p);
  if (rc != MTP_OK) return rc;
  if (!name || namelen <= 0) return MTP_ERR_ARG;
  const char *m = mtp_fixed_shape_match(p);
  std::snprintf(name, (size_t) namelen, "%s", m ? m : "");
  return MTP_OK;
}

int mtp_context_last_shape(const mtp_context *c, char *name, int namelen)
{
  if (!c || !name || namelen <= 0) return MTP_ERR_ARG;
  std::snprintf(name, (size_t) namelen, "%s", c->last_shape);
  return MTP_OK;
}

}   // extern "C"

void *mtp_internal_resolve_stream(mtp_context *c, void *stream)
{
  return stream ? stream : (c ? reinterpret_cast<void *>(c->stream) : nullptr);
}

int mtp_internal_installed_rows(const mtp_context *c) { return c && c->have_list ? c->inum : -1; }

int mtp_internal_check_grade_args(mtp_context *c, int grade_flag, const double *d_grades, const double *d_coeff_ders)
{
  if (!c) return MTP_ERR_ARG;
  if (!grade_flag) return MTP_OK;
  if (!c->pot->has_selection)
    return fail(c, MTP_ERR_STATE, "extrapolation grades requested but the potential has no #MVS_v1.1 selection state");
  const bool cfg = c->pot->configuration_mode;
  if (!cfg && !d_grades) return fail(c, MTP_ERR_ARG, "neighbourhood-mode grades need a grades array");
  if (cfg && !d_coeff_ders) return fail(c, MTP_ERR_ARG, "configuration-mode grades need a coeff_ders array");
  if (c->pot->species_count * c->pot->radial_func_count * c->pot->radial_basis_size > 256)
    return fail(c, MTP_ERR_LIMIT, "Sp*Mu*R above 256 is not supported by the grade kernels of this build");
  return MTP_OK;
}

int mtp_internal_finish_unpack(mtp_context *c, void *stream, int eflag, int vflag, double *d_ev, double *d_f, const int *d_idx,
                               const double *d_frecv, int n3)
{
  if (!c || !d_f || n3 < 0) return MTP_ERR_ARG;
  const int fold = ((eflag & MTP_ENERGY_GLOBAL) || vflag) ? 1 : 0;
  if (fold && !d_ev) return MTP_ERR_ARG;
  if (!fold && n3 == 0) return MTP_OK;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  return mtp_launch_ev_finish_unpack(c->d_ev_slots.ptr, d_ev, fold, d_f, d_idx, d_frecv, n3, st) == hipSuccess ? MTP_OK
                                                                                                                : MTP_ERR_DEVICE;
}

extern "C" {

int mtp_zero_async(void *stream, double *d_p, long long n)
{
  if (n < 0 || (n > 0 && !d_p) || (reinterpret_cast<uintptr_t>(d_p) & 15u)) return MTP_ERR_ARG;
  if (!stream) return MTP_ERR_ARG;   // no context here: NULL is not mapped to anything (include/mtp_mi355x.h, "Streams")
  return mtp_launch_zero(d_p, (size_t) n, reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? MTP_OK : MTP_ERR_DEVICE;
}

int mtp_context_set_deterministic(mtp_context *c, int enable)
{
  if (!c) return MTP_ERR_ARG;
  c->deterministic = enable != 0;
  return MTP_OK;
}

int mtp_context_set_timing(mtp_context *c, int enable)
{
  if (!c) return MTP_ERR_ARG;
  c->timing = enable != 0;
  c->timed = false;
  return MTP_OK;
}

int mtp_context_last_kernel_ms(mtp_context *c, float *ms)
{
  if (!c || !ms) return MTP_ERR_ARG;
  if (!c->timed) return MTP_ERR_STATE;
  hipError_t e = hipEventSynchronize(c->ev1);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, c->ev0, c->ev1);
  if (e != hipSuccess) return fail(c, MTP_ERR_DEVICE, std::string("event timing: ") + hipGetErrorString(e));
  return MTP_OK;
}

}   // extern "C"
