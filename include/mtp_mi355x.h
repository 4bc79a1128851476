/* libmtp_mi355x -- C ABI of the MI355X-native MTP pair-style compute path.
 *
 * This is the drop-in boundary: plain C types, opaque handles, int status
 * returns, no exceptions across the boundary.  Each entry point names the reference
 * interface (file:line relative to /root/reference) it stands in for; INTEGRATION.md
 * shows the LAMMPS `Pair` subclass / plugin stub that binds them.
 *
 * Threading: one context per rank/GPU; calls on one context must be serialised by the
 * caller (the reference is not re-entrant either: member scratch buffers,
 * LAMMPS/ML-MTP/pair_mtp.h:70-83).
 *
 * Streams.  Device work is ordered on the `stream` (a hipStream_t) given to an entry point.  ONE rule for NULL:
 *   - entry points that take a context (mtp_compute_device[_rows], mtp_build_neighbors_device,
 *     mtp_set_neighbors_device_2d, mtp_synchronize, mtp_halo_force_step, mtp_ghosts_reverse_finish,
 *     mtp_batch_cfg_grades, mtp_batch_cfg_candidates, mtp_maxvol_select, mtp_design_rows_device, the installs and
 *     mtp_context_coeff_tables_device): NULL means the
 *     context's own stream, resolved once per call -- every launch and RCCL group of that call runs on it;
 *   - entry points without a context (the other mtp_halo_*, mtp_ghosts_*, mtp_nve_* calls, mtp_zero_async,
 *     mtp_batch_reduce, mtp_ghosts_owner_device, mtp_batch_design_reduce, the mtp_sample_* calls, mtp_relax_step, the
 *     mtp_relax_cell_* calls, mtp_neb_step,
 *     mtp_normal_clear, mtp_normal_accumulate, mtp_normal_get, mtp_normal_set): NULL is
 *     rejected with MTP_ERR_ARG -- there is no stream to map it to, and the legacy null stream is never used.
 * The context's stream is created NON-BLOCKING: it does not synchronise with the legacy default stream, so a caller
 * whose other GPU work runs on the default stream (PyTorch's default) must pass a real stream handle that its own
 * work is ordered on, or synchronise around the calls.
 *
 * Installs (mtp_context_install_coeffs, mtp_context_install_selection, mtp_context_install_file) rewrite, IN PLACE, device
 * tables that every launch of the context reads.  Their ordering contract:
 *   - an install is ordered after all earlier work on `stream` (NULL: the context's own stream, as above);
 *   - it returns after that stream has drained -- ONE hipStreamSynchronize per call, whatever it installs -- so every later
 *     launch of the context, on any stream, reads the new values;
 *   - the caller's arrays are free on return;
 *   - the caller must have NO launch of this context in flight on ANOTHER stream while it installs: nothing orders such a
 *     launch against the copies, and it would read tables half old, half new.  A caller whose force calls are queued on
 *     its own stream installs on that stream (or synchronises first); NULL is right only for work that ran on the
 *     context's stream.
 */
#ifndef MTP_MI355X_H
#define MTP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTP_MI355X_ABI_VERSION 11

/* status codes (the reference aborts through error->one/all, pair_mtp.cpp:92,354-358;
 * the adapter turns a non-zero status + mtp_last_error() into error->all) */
enum {
  MTP_OK = 0,
  MTP_ERR_IO = -2,          /* cannot open / short read */
  MTP_ERR_EOF = -3,
  MTP_ERR_FORMAT = -4,      /* not "MTP" / wrong version */
  MTP_ERR_PARSE = -5,       /* keyword or number missing */
  MTP_ERR_UNSUPPORTED = -6, /* magnetic basis, unknown radial basis */
  MTP_ERR_TABLE = -7,       /* inconsistent alpha tables */
  MTP_ERR_SELECTION = -8,   /* #MVS block missing or malformed */
  MTP_ERR_MODE = -9,        /* energy_weight + site_en_weight > 1 */
  MTP_ERR_ARG = -20,
  MTP_ERR_DEVICE = -21,     /* HIP runtime failure, no device, wrong architecture */
  MTP_ERR_SPECIES = -22,    /* atom type outside the potential (pair_mtp.cpp:91-93,116-118) */
  MTP_ERR_STATE = -23,      /* e.g. compute before set_neighbors, grades without #MVS */
  MTP_ERR_LIMIT = -24       /* table or neighbour count beyond what one wave's LDS holds */
};

/* eflag / vflag bits follow LAMMPS (pair.h: ENERGY_GLOBAL 1, ENERGY_ATOM 2,
 * VIRIAL_PAIR 1, VIRIAL_FDOTR 2, VIRIAL_ATOM 4).  PairMTP::compute tests the raw vflag
 * (pair_mtp.cpp:257): any non-zero vflag tallies the global virial, bit 4 also vatom. */
#define MTP_ENERGY_GLOBAL 1
#define MTP_ENERGY_ATOM 2
#define MTP_VIRIAL_ATOM 4

/* kernel variant: the reference exposes two GPU styles, `mtp/kk` (thread-parallel,
 * KOKKOS/pair_mtp_kokkos.h:20-22) and `mtp/small/kk` (block-parallel,
 * KOKKOS/pair_mtps_kokkos.h:20-22).  Both map onto one wavefront-per-atom design here;
 * the variant only picks how many wavefronts share a workgroup. */
enum { MTP_VARIANT_AUTO = 0, MTP_VARIANT_LARGE = 1, MTP_VARIANT_SMALL = 2 };

typedef struct mtp_potential mtp_potential; /* parsed MLIP-3 file: PairMTP model state, pair_mtp.h:47-83 */
typedef struct mtp_context mtp_context;     /* one GPU: device tables, neighbour list, workspaces */

typedef struct mtp_potential_info {
  int32_t species_count;
  int32_t radial_basis_size;       /* R  */
  int32_t radial_func_count;       /* Mu */
  int32_t alpha_moment_count;      /* A  */
  int32_t alpha_index_basic_count; /* B  */
  int32_t alpha_index_times_count; /* T  */
  int32_t alpha_scalar_count;      /* S  */
  int32_t max_alpha_index_basic;   /* P  */
  int32_t coeff_count;             /* C = Sp^2 Mu R + Sp + S (pair_mtp_extrapolation.cpp:533) */
  int32_t has_selection;           /* a #MVS_v1.1 block was read */
  int32_t configuration_mode;      /* energy_weight == 1 (pair_mtp_extrapolation.cpp:605) */
  int32_t product_levels;          /* dependency levels of the times table (native schedule) */
  double scaling;
  double min_cutoff;
  double max_cutoff;               /* what PairMTP::init_one returns, pair_mtp.cpp:325-330 */
} mtp_potential_info;

/* PairMTP::read_file (pair_mtp.cpp:335-570) + RadialMTPBasis::ReadBasisProperties
 * (mtp_radial_basis.cpp:59-102); with want_selection != 0 also
 * PairMTPExtrapolation::read_file (pair_mtp_extrapolation.cpp:528-612).  Host only. */
int mtp_potential_load(const char *path, int want_selection, mtp_potential **out, char *err, int errlen);
void mtp_potential_free(mtp_potential *pot);
int mtp_potential_get_info(const mtp_potential *pot, mtp_potential_info *info);
/* copies of the parsed tables for inspection (sizes from get_info); any pointer may be NULL */
int mtp_potential_get_tables(const mtp_potential *pot, int32_t *alpha_index_basic /*[B][4]*/,
                             int32_t *alpha_index_times /*[T][4]*/, int32_t *alpha_moment_mapping /*[S]*/,
                             double *radial_coeffs /*[Sp*Sp*Mu*R]*/, double *species_coeffs /*[Sp]*/,
                             double *moment_coeffs /*[S]*/, double *inverse_active_set /*[C*C]*/);
/* the force kernel instantiation a context of this potential launches (host only): head x tail blocks of the
 * basic-moment pass, its lane grid (block lanes x blocks per lane) and the highest tensor rank of the unrolled force
 * phase.  MTP_ERR_LIMIT (fwd_blocks still written) when no instantiation fits; any pointer may be NULL */
int mtp_potential_kernel_shape(const mtp_potential *pot, int32_t *fwd_blocks, int32_t *block_lanes,
                               int32_t *blocks_per_lane, int32_t *max_degree);
/* the blocks of the basic-moment pass as the kernels read them (host only), 8 ints a block: the 3 x 3 head x tail blocks
 * of the generic kernels (five == 0) or the five-factor blocks of the fixed-shape kernels (five != 0).  Returns the
 * number of blocks, or a negative error; `blocks` (may be NULL) must hold cap_blocks >= that many.  basic_pack (may be
 * NULL) receives, for the basic at each LDS number, slot | a << 8 | b << 12 | c << 16 | mu << 20. */
int mtp_potential_moment_blocks(const mtp_potential *pot, int five, int32_t *blocks /*[cap_blocks][8]*/, int cap_blocks,
                                int32_t *basic_pack /*[B]*/);

/* The device copies made in PairMTPKokkos::settings (KOKKOS/pair_mtp_kokkos.cpp:108-174).
 * Fails with MTP_ERR_DEVICE when no gfx950 device is usable: there is no CPU fallback. */
int mtp_context_create(const mtp_potential *pot, int device_id, mtp_context **out, char *err, int errlen);
void mtp_context_destroy(mtp_context *ctx);
const char *mtp_last_error(const mtp_context *ctx);
int mtp_context_set_variant(mtp_context *ctx, int variant);

/* The neighbour list PairMTP::compute reads (pair_mtp.cpp:81-85): call after every
 * LAMMPS re-neighbouring.  `firstneigh[i]` is indexed by atom index i = ilist[ii], as in
 * LAMMPS; entries are masked with NEIGHMASK on the device. */
int mtp_set_neighbors(mtp_context *ctx, int inum, const int *ilist, const int *numneigh,
                      const int *const *firstneigh, int nall);
/* Same list in CSR form: neighbours of ilist[ii] are neigh[first[ii] .. first[ii+1]). */
int mtp_set_neighbors_csr(mtp_context *ctx, int inum, const int *ilist, const int *first, const int *neigh,
                          int nall);
/* CSR arrays already resident in HBM (no copy; must stay valid until replaced). */
int mtp_set_neighbors_device(mtp_context *ctx, int inum, const int *d_ilist, const int *d_first,
                             const int *d_neigh, int nall, int max_numneigh);
/* The list as LAMMPS-KOKKOS holds it on the device: the `/kk` styles of the reference read k_list->d_ilist(ii),
 * d_numneigh(i) and the padded 2-D view d_neighbors(i, jj) (KOKKOS/pair_mtp_kokkos.cpp:236-239, pair_mtp_kokkos.h:115;
 * `FindMaxNumNeighs`, pair_mtp_kokkos.cpp:177-191, 254-256).  Element (i, jj) is d_neighbors[i * stride_i + jj *
 * stride_jj] -- LayoutLeft (the GPU default): stride_i = 1, stride_jj = extent(0); LayoutRight: stride_i = extent(1),
 * stride_jj = 1 -- rows are indexed by atom index i = d_ilist[ii], max_neighs = extent(1).  Two device kernels and a
 * scan compact the view into the context's CSR arrays (special-bond bits are kept and masked with NEIGHMASK in the
 * force kernel, pair_mtp.cpp:114); d_ilist is used in place and must stay valid until the next list is installed.
 * Nothing passes through the host except one 12-byte read-back (entry count, longest row), which synchronises
 * `stream` once per re-neighbouring. */
int mtp_set_neighbors_device_2d(mtp_context *ctx, void *stream, int inum, const int *d_ilist, const int *d_numneigh,
                                const int *d_neighbors, long long stride_i, long long stride_jj, int max_neighs,
                                int nall);
/* Builds that list on the GPU from positions resident in HBM (what LAMMPS' Neighbor class
 * does ahead of the pair style, REQ_FULL at pair_mtp.cpp:317-318): a full list for atoms [0, inum) over all
 * nall atoms (owned first, then explicit ghosts -- no periodic images are invented), entries j != i with
 * |x_j - x_i|^2 <= list_cutoff^2.  lo / hi bound the positions of all nall atoms.  The list stays in the
 * context (ilist = 0..inum-1) and is installed as by mtp_set_neighbors_device; d_first_out / d_neigh_out (may be
 * null) receive device pointers to the CSR arrays, total_out / max_numneigh_out their sizes.  Synchronises the
 * stream once (to size the entry array). */
int mtp_build_neighbors_device(mtp_context *ctx, void *stream, const double *d_x, int inum, int nall,
                               double list_cutoff, const double lo[3], const double hi[3],
                               const int **d_first_out, const int **d_neigh_out, long long *total_out,
                               int *max_numneigh_out);
/* Copies the CSR arrays of the list the context owns (uploaded by mtp_set_neighbors[_csr] or built by
 * mtp_build_neighbors_device) back to the host: first[inum + 1], neigh[first[inum]].  MTP_ERR_STATE when the
 * current list lives in caller memory (mtp_set_neighbors_device). */
int mtp_copy_neighbors_to_host(mtp_context *ctx, int *first, int *neigh);

/* PairMTP::compute (pair_mtp.cpp:72-280) and, with grade_flag != 0,
 * PairMTPExtrapolation::compute (pair_mtp_extrapolation.cpp:68-382), on host arrays laid
 * out as LAMMPS lays them out: x, f [nall][3]; type [nall] 1-based; eatom [nall];
 * vatom [nall][6].  f, virial and vatom ACCUMULATE, eatom[i] is assigned for i in ilist,
 * *energy accumulates (eng_vdwl), exactly as in the reference.  grades[i] (neighbourhood
 * mode) is assigned for i in ilist; *max_grade is this rank's maximum (neighbourhood) or
 * is left to mtp_cfg_grade (configuration mode, where coeff_ders[C] receives this rank's
 * sum_i dE_i/dtheta for the caller to all-reduce, pair_mtp_extrapolation.cpp:369).
 * Unused outputs may be NULL.  Copies go over PCIe; use the _device form to avoid them. */
int mtp_compute(mtp_context *ctx, const double *x, const int *type, int eflag, int vflag, int grade_flag,
                double *f, double *eatom, double *vatom, double *energy, double *virial /*[6]*/,
                double *grades, double *max_grade, double *coeff_ders);

/* Same, device pointers, asynchronous on `stream` (a hipStream_t, NULL = context stream).
 * d_ev[7] accumulates {energy, virial xx,yy,zz,xy,xz,yz}; d_max_grade[1] is max-updated
 * (caller zeroes); d_coeff_ders[C] accumulates.  The atom-type error is reported by the next
 * mtp_synchronize(). */
int mtp_compute_device(mtp_context *ctx, void *stream, const double *d_x, const int *d_type, int eflag,
                       int vflag, int grade_flag, double *d_f, double *d_eatom, double *d_vatom,
                       double *d_ev, double *d_grades, double *d_max_grade, double *d_coeff_ders);
/* The same on rows [row_begin, row_begin + row_count) of the installed list only (rows = positions in ilist).  A
 * domain-decomposed step splits its owned atoms into those whose list holds no ghost and the rest, so that the
 * former are computed while the ghost positions are still in flight (what LAMMPS-KOKKOS does with its
 * interior / boundary kernels; reference anchor for the semantics: pair_mtp.cpp:252-254, 315).  Energy and virial
 * keep accumulating in the context's tally slots over the launches of a step; the launch with finish_tallies != 0
 * folds them into d_ev (the others may pass d_ev = NULL).  Grades / candidate vectors of the rows are produced
 * per launch. */
int mtp_compute_device_rows(mtp_context *ctx, void *stream, int row_begin, int row_count, int finish_tallies,
                            const double *d_x, const int *d_type, int eflag, int vflag, int grade_flag,
                            double *d_f, double *d_eatom, double *d_vatom, double *d_ev, double *d_grades,
                            double *d_max_grade, double *d_coeff_ders);
int mtp_synchronize(mtp_context *ctx, void *stream);

/* ---- device-resident step: what the reference's /kk styles do around their kernels --------------------------------
 * PairMTPKokkos::compute (KOKKOS/pair_mtp_kokkos.cpp:197-399) and PairMTPExtrapolationKokkos::compute
 * (KOKKOS/pair_mtp_extrapolation_kokkos.cpp:274-610) read x / type and write f through LAMMPS-KOKKOS device views
 * (:231-240) and keep every other output -- eng_vdwl / virial (`ev`), d_eatom, d_vatom, the grades -- in device views
 * that are copied to the host only when something asks (k_eatom / k_vatom sync :379-388; grades :223-243).  Here those
 * views belong to the context:
 *   mtp_compute_resident   zeroes the totals and the requested per-atom arrays on `stream`, then runs the force call of
 *                          mtp_compute_device (same flags, same accumulate / assign semantics) into them; nothing
 *                          crosses PCIe and nothing waits;
 *   mtp_resident_totals    the ONE wait of a step: ev7 = {energy, virial xx,yy,zz,xy,xz,yz} of that call, this rank's
 *                          maximum grade (neighbourhood mode) and, in configuration mode, sum_i dE_i/dtheta (C doubles,
 *                          may be NULL); reports the atom-type error like mtp_synchronize;
 *   mtp_resident_peratom_device / _host   the per-atom arrays of that call -- eatom [nall], vatom [nall][6], grades
 *                          [nall] -- as a device pointer (valid until the next call that grows them) or copied to the
 *                          host on request (what `fix pair` / `dump` trigger through extract_peratom,
 *                          pair_mtp_extrapolation.cpp:641-652). */
enum { MTP_PERATOM_EATOM = 0, MTP_PERATOM_VATOM = 1, MTP_PERATOM_GRADES = 2 };
int mtp_compute_resident(mtp_context *ctx, void *stream, const double *d_x, const int *d_type, double *d_f, int eflag,
                         int vflag, int grade_flag);
int mtp_resident_totals(mtp_context *ctx, void *stream, double *ev7, double *max_grade, double *coeff_ders);
int mtp_resident_peratom_device(mtp_context *ctx, int what, const double **d_ptr, int *ncol);
int mtp_resident_peratom_host(mtp_context *ctx, void *stream, int what, double *host);
/* `bytes` from a device array to the host, ordered on `stream` and waited for (atomKK->sync(Host, ...) for the few
 * rows a .cfg record needs, pair_mtp_extrapolation.cpp:401-479, when positions live on the device) */
int mtp_copy_to_host(mtp_context *ctx, void *stream, void *host, const void *d_src, size_t bytes);

/* PairMTPExtrapolation::calculate_extrapolation_grade (pair_mtp_extrapolation.cpp:347-358)
 * for configuration mode: max_i |sum_j coeff_ders[j] A^-1[i][j]| on the host (C^2 flops,
 * once per step after the cross-rank sum). */
int mtp_cfg_grade(const mtp_potential *pot, const double *coeff_ders, double *grade);

/* Compile-time switches of this build that differ from the shipped defaults, space separated ("" for a release
 * build: tests assert that the library they load carries none -- diagnostic variants are never shipped). */
const char *mtp_build_flags(void);
/* introspection for benchmarks: LDS bytes per wavefront, wavefronts per workgroup, grid */
int mtp_context_launch_info(const mtp_context *ctx, int32_t *lds_bytes_per_wave, int32_t *waves_per_block,
                            int32_t *grid_blocks, int32_t *neighbor_tile);
/* d_p[0, n) = 0.0 in one kernel launch on `stream` (d_p 16-byte aligned): the "zero the force array" that precedes
 * every force call (LAMMPS: Verlet::force_clear) without hipMemsetAsync's two fill kernels. */
int mtp_zero_async(void *stream, double *d_p, long long n);
/* Deterministic force sums (tests, reproducible goldens; SURVEY.md section 5 "deterministic-reduction mode"): the
 * scatter f_j -= F_ij and the per-atom totals are accumulated as 64-bit fixed-point integers (2^-40 eV/A, |f| < 2^23)
 * and converted once, so two calls on the same input return the same bits; energy and virial are folded in a fixed
 * order in either mode.  Default off: native fp64 HBM atomics, whose sums depend on arrival order in the last bits
 * (as the reference's own Kokkos atomics do, KOKKOS/pair_mtp_kokkos.cpp:602-605). */
int mtp_context_set_deterministic(mtp_context *ctx, int enable);
/* register build the planner chose (2 or 3 wavefronts per SIMD) and whether the per-atom LDS image uses the
 * "rebuild" layout (radial tables built twice, moments overlaying them) */
int mtp_context_plan_info(const mtp_context *ctx, int32_t *waves_per_simd, int32_t *rebuild_tables);
/* per-atom LDS layout of the force calls' plan (after a set_neighbors call): 0 keep, 1 lean (no dg rows),
 * 2 rebuild, 3 rebuild without dg rows (MTP_LAYOUT = keep | lean | rebuild | rebuild-nodg forces one) */
int mtp_context_layout_mode(const mtp_context *ctx, int32_t *mode);
/* The launch plan without a device (host only).  For a list of `inum` rows with at most `max_numneigh` entries each on a
 * GPU of `num_cus` compute units, `variant` as in mtp_context_set_variant, `grade` = a call with grades:
 * mtp_plan_fixed_fields writes, as "name=value" lines, the force kernel's template arguments (KL NB PITCH GRADE DEG WPS)
 * and every field of the kernel's argument block that the potential's table structure and the plan decide -- the
 * fields a fixed-shape instantiation of the kernel may hold as compile-time constants (csrc/mtp_shape_fields.hpp);
 * mtp_plan_fixed_shape writes the name of the compiled fixed-shape kernel such a launch runs, or "" when it runs a
 * generic one.  A launch runs a fixed-shape kernel only when every field that shape fixes equals the launch's value. */
int mtp_plan_fixed_fields(const mtp_potential *pot, int num_cus, int inum, int max_numneigh, int variant, int grade,
                          char *buf, int buflen);
int mtp_plan_fixed_shape(const mtp_potential *pot, int num_cus, int inum, int max_numneigh, int variant, int grade,
                         char *name, int namelen);
/* name of the fixed-shape kernel the context's last force launch ran, "" for a generic kernel (MTP_FIXED_SHAPE=0 in
 * the environment, read at every launch, keeps all launches on the generic kernels: tests and A/B runs) */
int mtp_context_last_shape(const mtp_context *ctx, char *name, int namelen);
/* last kernel time of the dominant kernel in ms, measured with HIP events on the launch
 * stream (enable with mtp_context_set_timing(ctx, 1); costs one event pair per call) */
int mtp_context_set_timing(mtp_context *ctx, int enable);
int mtp_context_last_kernel_ms(mtp_context *ctx, float *ms);

/* ---- multi-GPU halo: spatial domain decomposition, one process per GPU, RCCL over xGMI ------------------------
 *
 * The reference leaves the ghost-atom exchange to LAMMPS' Comm class (forward_comm of x before Pair::compute,
 * reverse_comm of f after it); it only relies on it: forces are written onto ghosts (pair_mtp.cpp:252-254) and
 * newton_pair must be on (pair_mtp.cpp:315).  A standalone driver (or a KOKKOS-resident LAMMPS that hands over
 * device views) gets the same two exchanges from the library: device pack / unpack kernels around ONE grouped
 * RCCL exchange per direction (ncclGroupStart, ncclSend / ncclRecv to every peer, ncclGroupEnd) on the halo's own
 * stream, ordered with the caller's stream by events, so interior force work overlaps the exchange.
 *
 * Layout contract: atoms [0, nlocal) are owned, ghosts follow, grouped by the rank that owns them, in rank order
 * (recv_counts[q] ghosts from rank q).  send_idx lists, grouped by destination rank in rank order (send_counts[q]
 * entries for rank q), the owned atoms each peer holds as ghosts, in the order that peer stores them; send_shift
 * is the periodic shift added to their coordinates on the way.  A rank may be its own peer (periodic images).
 */
typedef struct mtp_halo mtp_halo;
#define MTP_HALO_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
enum { MTP_REDUCE_SUM = 0, MTP_REDUCE_MAX = 1 };

/* ncclGetUniqueId: called on one rank; the caller passes the bytes to every rank (MPI_Bcast, a TCP store, a file) */
int mtp_halo_get_unique_id(void *id_out /*[MTP_HALO_ID_BYTES]*/);
/* Host only, no device: the per-peer segment tables mtp_halo_create derives from the layout contract above -- peer q's
 * segment starts at atom send_off[q] of the packed send buffer and at ghost recv_off[q]; arrays of nranks + 1 entries
 * (last = totals) -- with the same checks (counts add up, send_idx inside the owned atoms).  These are the offsets the
 * grouped ncclSend / ncclRecv of a direction use (the counterpart of LAMMPS' Comm sendlist / firstrecv bookkeeping
 * the reference relies on, pair_mtp.cpp:252-254, 315). */
int mtp_halo_layout(int nranks, int nlocal, int nghost, const int *send_idx, const int *send_counts,
                    const int *recv_counts, int *send_off /*[nranks+1]*/, int *recv_off /*[nranks+1]*/, char *err,
                    int errlen);
/* ncclCommInitRank + device copies of the index lists: collective over all nranks processes.  unique_id == NULL
 * creates the halo WITHOUT a communicator (no collective call): it packs, unpacks and answers mtp_halo_get_layout,
 * and its segments are moved by mtp_halo_local_exchange or by the caller; the RCCL entry points (mtp_halo_forward_begin,
 * mtp_halo_forward, mtp_halo_reverse_begin, mtp_halo_reverse, mtp_halo_force_step, mtp_halo_allreduce) then return
 * MTP_ERR_STATE before anything is launched. */
int mtp_halo_create(int device_id, int nranks, int rank, const void *unique_id, int nlocal, int nghost,
                    const int *send_idx /*[sum send_counts]*/, const double *send_shift /*[sum send_counts][3]*/,
                    const int *send_counts /*[nranks]*/, const int *recv_counts /*[nranks]*/, mtp_halo **out,
                    char *err, int errlen);
void mtp_halo_destroy(mtp_halo *halo);
const char *mtp_halo_last_error(const mtp_halo *halo);
/* what RCCL itself reports for the communicator (ncclCommCount, ncclCommUserRank, ncclGetVersion) */
int mtp_halo_comm_count(const mtp_halo *halo, int *nranks, int *rank, int *rccl_version);
/* Comm::forward_comm: d_x[nlocal + k] <- owner's x + shift.  begin: pack on `stream`, exchange on the halo's
 * stream; end: `stream` waits for the exchange.  Work queued on `stream` in between overlaps it.  A halo without a
 * communicator: MTP_ERR_STATE from begin, before the pack (likewise mtp_halo_reverse_begin). */
int mtp_halo_forward_begin(mtp_halo *halo, void *stream, double *d_x /*[nall][3]*/);
int mtp_halo_forward_end(mtp_halo *halo, void *stream);
int mtp_halo_forward(mtp_halo *halo, void *stream, double *d_x);
/* Comm::reverse_comm: ghost rows of d_f are sent back and added onto their owners (fp64 atomics).  begin: the
 * exchange starts once `stream` has reached this point (every launch that writes ghost forces must precede it);
 * end: `stream` waits, then adds the received rows into d_f[0, nlocal). */
int mtp_halo_reverse_begin(mtp_halo *halo, void *stream, const double *d_f /*[nall][3]*/);
int mtp_halo_reverse_end(mtp_halo *halo, void *stream, double *d_f);
int mtp_halo_reverse(mtp_halo *halo, void *stream, double *d_f);
/* One domain-decomposed force call (Comm::forward_comm, Pair::compute, Comm::reverse_comm of a LAMMPS step,
 * pair_mtp.cpp:252-254, 315): zero d_f, ghost positions in, forces of the rows_a + rows_b + rows_c = inum rows, ghost
 * forces back onto their owners, tallies folded into d_ev by the last force launch.  Default schedule: everything
 * on `stream` -- pack, forward group, one launch over all rows, reverse group, unpack (measured faster on MI355X than
 * the overlapped one at every domain size tried).  mtp_halo_set_overlap(halo, 1): both exchanges overlapped -- the
 * installed list must then be ordered interior | boundary | interior (interior = no ghost in the atom's list): forward
 * halo || rows [0, rows_a), boundary rows, reverse halo || the last rows_c rows, on `stream` and the halo's stream.
 * Every refusal comes before the first launch, so a refused call has written neither d_f nor d_x and issued no group:
 * MTP_ERR_ARG for a misaligned d_f, a negative row count, rows_a + rows_b + rows_c != inum of the installed list, or a
 * NULL d_ev when (eflag & MTP_ENERGY_GLOBAL) || vflag; MTP_ERR_STATE for a halo without a communicator or a context
 * without a list; and the grade refusals of mtp_compute_device_rows (no selection state: MTP_ERR_STATE, no d_grades /
 * d_coeff_ders array for the potential's mode: MTP_ERR_ARG, Sp*Mu*R > 256: MTP_ERR_LIMIT; text in mtp_last_error(ctx),
 * the others' in mtp_halo_last_error).  Only a failure of the device or of RCCL can end the call later. */
int mtp_halo_force_step(mtp_halo *halo, mtp_context *ctx, void *stream, int rows_a, int rows_b, int rows_c,
                        double *d_x, const int *d_type, int eflag, int vflag, int grade_flag, double *d_f,
                        double *d_eatom, double *d_vatom, double *d_ev, double *d_grades, double *d_max_grade,
                        double *d_coeff_ders);
int mtp_halo_set_overlap(mtp_halo *halo, int enable);
int mtp_halo_get_overlap(const mtp_halo *halo);
/* The kernels either side of an exchange on their own: sendbuf[k] = d_x[send_idx[k]] + send_shift[k] (what
 * mtp_halo_forward_begin launches ahead of its group) and d_f[send_idx[k]] += frecv[k] (what mtp_halo_reverse_end
 * launches behind its group). */
int mtp_halo_pack_forward(mtp_halo *halo, void *stream, const double *d_x);
int mtp_halo_unpack_reverse(mtp_halo *halo, void *stream, double *d_f);
/* the tables of this halo as the exchange uses them (arrays of nranks + 1 / nranks entries; any may be NULL) */
int mtp_halo_get_layout(const mtp_halo *halo, int *nsend, int *send_off, int *send_counts, int *recv_off,
                        int *recv_counts);
/* Single-process rehearsal of an n-rank exchange: halos[r] = rank r of ONE n-rank decomposition, all on one device
 * (created with or without a communicator).  direction 0 = forward: after mtp_halo_pack_forward on every rank, copies
 * every (source q, destination r) segment into the ghost rows of d_arrays[r] (= rank r's positions [nall_r][3]);
 * direction 1 = reverse: copies the ghost rows of d_arrays[r] (= rank r's forces) into the owners' receive buffers,
 * to be folded by mtp_halo_unpack_reverse.  Device-to-device copies on `stream`, addressed with the same per-peer
 * offset tables the RCCL groups use; fails when the two sides of a segment disagree on its length. */
int mtp_halo_local_exchange(mtp_halo *const *halos, int n, void *stream, int direction, double *const *d_arrays);
/* in-place ncclAllReduce of `count` doubles: energy / virial and the configuration-mode candidate vector (SUM,
 * pair_mtp_extrapolation.cpp:369), the neighbourhood-mode maximum grade (MAX, :379) */
int mtp_halo_allreduce(mtp_halo *halo, void *stream, double *d_buf, int count, int op);

/* ---- standalone MD support: LAMMPS-core work either side of Pair::compute, on the device ------
 *
 * For drivers that keep the whole step in HBM (bench.py's whole-step number, lammps_mtp_kokkos_amd/md.py): the
 * periodic ghost images of ONE GPU's own atoms (Comm::borders / forward_comm / reverse_comm of a single rank; the
 * pair style needs them because it writes forces onto ghosts, pair_mtp.cpp:252-254, 315) and the two halves of a
 * velocity-Verlet step (fix nve).  mtp_ghosts_build: orthogonal box [0, box), every edge >= rghost (the fast path the
 * whole-step benchmark runs); mtp_ghosts_build_cell: any periodic cell, smaller than rghost included.
 */
typedef struct mtp_ghosts mtp_ghosts;
int mtp_ghosts_create(int device_id, mtp_ghosts **out);
void mtp_ghosts_destroy(mtp_ghosts *g);
const char *mtp_ghosts_last_error(const mtp_ghosts *g);
/* Re-neighbouring: wraps d_x[0, nlocal) into the box, finds every periodic image within rghost of the box (atom
 * order, then lexicographic shift order: deterministic) and writes their positions behind the owned atoms.
 * *nall_out = nlocal + ghosts; MTP_ERR_LIMIT (nothing written beyond the wrap) when that exceeds `capacity` rows.
 * Synchronises the stream once (the ghost count sizes the caller's arrays and the neighbour list). */
int mtp_ghosts_build(mtp_ghosts *g, void *stream, double *d_x /*[capacity][3]*/, int nlocal, int capacity,
                     const double box[3], double rghost, int *nall_out);
/* The same for any periodic cell.  cell[9]: rows are the lattice vectors a, b, c (any right-handed, non-degenerate
 * cell; LAMMPS' restricted triclinic is the lower-triangular case, an orthogonal box the diagonal one); origin at 0.
 * With fractional coordinates s = x . cell^-1, the owned atoms are wrapped to s in [0, 1)^3 and written back as
 * s . cell.  With plane spacings d_a = V / |cell_b x cell_c| (cyclic) and margins m_a = rghost / d_a, the image of
 * atom i under the integer shift n != 0 is a ghost iff -m_a <= s_a + n_a < 1 + m_a for a = 0, 1, 2 (the slab
 * criterion of LAMMPS' triclinic ghost cutoffs: a superset of "within rghost of the cell", separable per direction).
 * Any number of images per direction, no lower limit on the cell size.  Ghost order, capacity protocol, the single
 * stream synchronisation and the NULL-stream rule as for mtp_ghosts_build; shift[k] = n . cell.  MTP_ERR_ARG for a
 * cell with det <= 0 or non-finite entries (nothing is launched); MTP_ERR_LIMIT, *nall_out = INT_MAX, when owned +
 * ghost atoms do not fit an int (never wrapped).  nlocal == 0: MTP_OK, *nall_out = 0, nothing is launched and the
 * stream is not synchronised (as in mtp_ghosts_build_batch).  mtp_ghosts_forward / reverse / reverse_finish / types
 * then work on the handle unchanged. */
int mtp_ghosts_build_cell(mtp_ghosts *g, void *stream, double *d_x /*[capacity][3]*/, int nlocal, int capacity,
                          const double cell[9], double rghost, int *nall_out);
/* Host arithmetic only: bounds of every position mtp_ghosts_build_cell can write for this cell and rghost (the lo / hi
 * that mtp_build_neighbors_device wants), the cell volume, and the images taken per direction and sign (ceil(m_a)).
 * Any output may be NULL. */
int mtp_ghosts_cell_bounds(const double cell[9], double rghost, double lo[3], double hi[3], double *volume,
                           int nimage[3]);
int mtp_ghosts_forward(mtp_ghosts *g, void *stream, double *d_x);   /* ghost rows <- owner + shift            */
int mtp_ghosts_reverse(mtp_ghosts *g, void *stream, double *d_f);   /* owner rows += ghost rows (fp64 atomics) */
/* The same together with the energy / virial fold of a force call made through mtp_compute_device_rows(...,
 * finish_tallies = 0, ...): one launch instead of two (d_ev as in mtp_compute_device; eflag / vflag of that call). */
int mtp_ghosts_reverse_finish(mtp_ghosts *g, mtp_context *ctx, void *stream, int eflag, int vflag, double *d_f, double *d_ev);
int mtp_ghosts_types(mtp_ghosts *g, void *stream, int *d_type);     /* ghost types <- owner types              */
/* fix nve (metal units: dtf = 0.5 dt ftm2v): v += dtf f / m; x += dt v   and   v += dtf f / m; masses per type */
int mtp_nve_initial(void *stream, int nlocal, double *d_x, double *d_v, const double *d_f, const int *d_type,
                    const double *d_inv_mass, double dtf, double dt);
int mtp_nve_final(void *stream, int nlocal, double *d_v, const double *d_f, const int *d_type,
                  const double *d_inv_mass, double dtf);
/* d_out2[0] = max_i |x_i - x_ref_i|^2 (the half-skin re-neighbouring test), d_out2[1] = sum_i m_i v_i^2 */
int mtp_nve_monitor(void *stream, int nlocal, const double *d_x, const double *d_x_ref, const double *d_v,
                    const int *d_type, const double *d_mass, double *d_out2);

/* ---- batched configurations: many small periodic cells in one device pass ------------------------------------------
 *
 * Training and candidate configurations (1 to 200 atoms, each with its own lattice, thousands at a time) are what the
 * reference evaluates one `run 0` at a time: one PairMTP::compute (pair_mtp.cpp:72-280) or
 * PairMTPExtrapolation::compute (pair_mtp_extrapolation.cpp:68-382) per configuration, each with its own Comm::borders
 * and Neighbor build.  Here one pass serves the whole batch: every configuration gets a slot of its own in one large
 * box (mtp_batch_layout), one ghost build takes a different cell per atom (mtp_ghosts_build_batch), the stock
 * mtp_build_neighbors_device and ONE force call with MTP_ENERGY_ATOM | MTP_VIRIAL_ATOM run over all rows, and the
 * per-atom outputs are reduced per configuration (mtp_batch_reduce, mtp_batch_cfg_grades).  Owned atoms of
 * configuration k are rows [cfg_first[k], cfg_first[k + 1]) of every per-atom array; cfg_first[0] = 0, non-decreasing,
 * empty configurations allowed.
 */
/* Host arithmetic only.  cells[ncfg][9] (rows = lattice vectors, as for mtp_ghosts_build_cell).  The ghost
 * parallelepiped of configuration k (what mtp_ghosts_cell_bounds reports for its cell and rghost) is translated by
 * origins[k] into slot k of a 3-D grid of uniform slots, sized by the largest extents in the batch and centred on the
 * origin; two slots are at least `gap` apart along some axis, so with gap >= the list cutoff (required: gap >= rghost) no
 * atom or image of one configuration lies within the list cutoff of another and the stock neighbour build keeps them
 * apart.  lo / hi bound every position of the batch (what mtp_build_neighbors_device wants), *ncells is the number of
 * list cells (edge rghost) that box implies.  MTP_ERR_ARG for a cell with det <= 0 or non-finite entries: err names the
 * configuration.  MTP_ERR_LIMIT when the batch would need more than 2^26 list cells (the builder's limit) or a
 * coordinate beyond 2048 A in magnitude (translation costs bits of the interatomic distances): err names
 * the first configuration that does not fit and *nfit is the number of leading configurations that do -- the caller
 * splits the batch there.  On success *nfit = ncfg.  ncells and nfit may be NULL. */
int mtp_batch_layout(int ncfg, const double *cells /*[ncfg][9]*/, double rghost, double gap, double *origins /*[ncfg][3]*/,
                     double lo[3], double hi[3], long long *ncells, int *nfit, char *err, int errlen);
/* mtp_ghosts_build_cell with the cell looked up per atom (Comm::borders of every configuration at once).  cfg_first
 * [ncfg + 1], cells [ncfg][9] and origins [ncfg][3] are HOST arrays (copied to the device by the call).  Atom i of
 * configuration k is wrapped into cell k exactly as mtp_ghosts_build_cell wraps it, then translated by origins[k]; its
 * images are found by the same slab criterion with cell k's margins.  Ghost order as ever: all owned atoms first, then
 * the ghosts in atom order, then in lexicographic shift order, shift[k] = n . cell of the owner's configuration -- so
 * mtp_ghosts_forward / reverse / reverse_finish / types work on the handle unchanged.  Capacity protocol, 64-bit total,
 * the single stream synchronisation and the NULL-stream rule as for mtp_ghosts_build_cell.  MTP_ERR_ARG, nothing
 * launched, for a cfg_first that does not start at 0 or decreases and for a bad cell (the error names the
 * configuration). */
int mtp_ghosts_build_batch(mtp_ghosts *g, void *stream, double *d_x /*[capacity][3]*/, int ncfg, const int *cfg_first,
                           const double *cells, const double *origins, int capacity, double rghost, int *nall_out);
/* Per-configuration totals of a force call made with MTP_ENERGY_ATOM | MTP_VIRIAL_ATOM: d_energy[k] = sum of d_eatom,
 * d_virial[k][6] = sum of d_vatom over the owned rows of configuration k (the reference tallies vatom on the central
 * atom, pair_mtp.cpp:268-276: ghost rows carry none), same sign and component order as d_ev; d_cfg_grade[k] = max of
 * d_grades over those rows (neighbourhood mode: pair_mtp_extrapolation.cpp:333-335 per configuration).  Each output
 * with its input may be NULL.  One wavefront per configuration (its workgroup for segments longer than 256 rows), rows
 * read coalesced and combined in a fixed order without atomics: a configuration's result does not depend on the rest of
 * the batch.  An empty configuration gets zeros.  d_cfg_first [ncfg + 1] is a device array.  No context: NULL stream is
 * rejected. */
int mtp_batch_reduce(void *stream, int ncfg, const int *d_cfg_first, const double *d_eatom, const double *d_vatom,
                     const double *d_grades, double *d_energy, double *d_virial, double *d_cfg_grade);
/* Configuration-mode grades per configuration, after a grade call (grade_flag != 0) over the nrows = cfg_first[ncfg] rows
 * of the installed list: the context's candidate vectors are summed per configuration (the MPI_Allreduce of
 * pair_mtp_extrapolation.cpp:369 with one "world" per configuration), graded by the same MFMA kernel as the
 * neighbourhood grades (calculate_extrapolation_grade, :347-358) and divided by the configuration's atom count, 0 for an
 * empty one (:373-376).  NULL stream = the context's. */
int mtp_batch_cfg_grades(mtp_context *ctx, void *stream, int ncfg, const int *d_cfg_first, int nrows, double *d_cfg_grade);

/* ---- batched sampling: finite-temperature MD of a whole batch of cells, grades watched on the device ----------------
 *
 * The step of the active-learning loop that PRODUCES candidate configurations: MD under the current potential that
 * watches the extrapolation grade (the reference does it inside LAMMPS: pair_style mtp/extrapolation ... threshold_select /
 * threshold_break, pair_mtp_extrapolation.cpp:389-399, under fix langevin + fix nve).  These are the integrator pieces
 * over the layout of the batched configurations: per-atom arrays hold the owned rows [cfg_first[k], cfg_first[k + 1]) of
 * configuration k, positions are in SLOT coordinates (cell coordinates + origins[k], as mtp_ghosts_build_batch leaves them)
 * between re-neighbourings, and the force / grade call in the middle of a step is the stock one over all rows.  Per
 * configuration, device arrays [ncfg]: the target temperature, a 64-bit noise key chosen by the caller, frozen (0 / 1) and
 * last_capture (a step; start it at -2^30).  Every array is the caller's; no context: NULL stream is rejected.  A step is
 *   mtp_sample_initial -> mtp_ghosts_forward -> force call -> mtp_ghosts_reverse[_finish] -> mtp_sample_final
 * and, on a grade step, the per-configuration grades (mtp_batch_reduce / mtp_batch_cfg_grades) -> mtp_sample_capture.
 */
/* d_row_cfg[i] = the configuration of owned row i, i < nrows = cfg_first[ncfg] (device arrays).  Once per pass: the three
 * per-step kernels read it instead of searching cfg_first. */
int mtp_sample_row_map(void *stream, int ncfg, const int *d_cfg_first, int nrows, int *d_row_cfg);
/* fix nve, first half (metal units, dtf = 0.5 dt ftm2v): v += dtf f / m; x += dt v for the rows of unfrozen configurations
 * -- bit for bit what mtp_nve_initial does to them; rows of a frozen configuration are not written. */
int mtp_sample_initial(void *stream, int nrows, const int *d_row_cfg, const int *d_frozen, double *d_x, double *d_v,
                       const double *d_f, const int *d_type, const double *d_inv_mass, double dtf, double dt);
/* fix langevin (post_force, its default uniform noise) and then fix nve's second half, in that order, one launch:
 *     gamma1 = -m / t_damp / ftm2v,   gamma2 = sqrt(m) sqrt(24 kB T[k] / t_damp / dt / mvv2e) / ftm2v
 *     f += gamma1 v + gamma2 (u - 0.5)     (stored back: the next first half kicks with it, as in LAMMPS)
 *     v += dtf f / m
 * for the rows of unfrozen configurations.  u per atom, step and component is counter-based: Philox4x32-10 with the counter
 * (step, index of the atom within its configuration, low word of key[k], high word of key[k]) and the key (low word of
 * seed, high word of seed); output words 0, 1, 2 give x, y, z as u = (w + 0.5) 2^-32, so u - 0.5 is exact, symmetric and
 * never at an end point.  A configuration's noise therefore does not depend on the batch it sits in or where.  t_damp <= 0
 * or non-finite: no thermostat -- nothing drawn, f not written, v bit for bit mtp_nve_final's (d_mass, d_temperature, d_key
 * may then be NULL).  masses per type; 0 <= step < 2^31. */
int mtp_sample_final(void *stream, int nrows, const int *d_row_cfg, const int *d_cfg_first, const int *d_frozen, double *d_v,
                     double *d_f, const int *d_type, const double *d_mass, const double *d_inv_mass,
                     const double *d_temperature, const unsigned long long *d_key, unsigned long long seed, int step, double dtf,
                     double dt, double t_damp);
/* Per configuration d_mv2[k] = sum m v^2 over its rows (an empty one: 0) and d_d2[k] = the largest |x - x_ref|^2 of its
 * rows, 0 for a frozen configuration; one wavefront per configuration (its workgroup above 256 rows, as mtp_batch_reduce),
 * fixed order, no atomics.  Then d_block4 = {max_k d_d2[k], frozen, captured, dropped} with the three counts taken from
 * d_counts (mtp_sample_capture's): the one thing a driver reads between re-neighbourings. */
int mtp_sample_monitor(void *stream, int ncfg, const int *d_cfg_first, const int *d_frozen, const double *d_x,
                       const double *d_x_ref, const double *d_v, const int *d_type, const double *d_mass, const int *d_counts,
                       double *d_mv2, double *d_d2, double *d_block4);
/* The capture decisions of a grade step at `step`, from the per-configuration grades g = d_cfg_grade[k], on the device:
 *   - configuration k wants a slot if it is neither frozen nor empty, !(g < threshold_select) and
 *     step - last_capture[k] >= capture_gap (a NaN grade therefore captures);
 *   - slots of the candidate buffer go out in ascending (step, configuration) order: slot = the number of configurations
 *     that wanted one before it (an exclusive scan over the configurations, any ncfg; no atomic counter);
 *   - a slot below max_candidates is filled: d_rec[slot] = {k, step}, d_rec_grade[slot] = g, last_capture[k] = step,
 *     d_cand_x[slot][j][3] = x - origins[k] of its j-th owned row (`stride` rows a slot, stride >= the largest
 *     configuration), and the configuration freezes if !(g < threshold_break);
 *   - otherwise NOTHING of it is written, it is counted as dropped and it does not freeze.
 * d_counts[3] = {captured, dropped, frozen} accumulate over the calls of a run (zero them first); d_slot [ncfg] is scratch
 * (the slot of each configuration at this step, -1 for none). */
int mtp_sample_capture(void *stream, int ncfg, const int *d_cfg_first, int nrows, const int *d_row_cfg,
                       const double *d_cfg_grade, int step, double threshold_select, double threshold_break, int capture_gap,
                       const double *d_x, const double *d_origins /*[ncfg][3]*/, int *d_frozen, int *d_last_capture, int *d_slot,
                       int max_candidates, int stride, double *d_cand_x, int *d_rec /*[max_candidates][2]*/, double *d_rec_grade,
                       int *d_counts);
/* x -= origins[row_cfg]: slot coordinates back to cell coordinates, in front of a re-neighbouring --
 * mtp_ghosts_build_batch wraps cell coordinates and translates them again. */
int mtp_sample_to_cell(void *stream, int nrows, const int *d_row_cfg, const double *d_origins, double *d_x);

/* ---- batched relaxation: FIRE minimisation of a whole batch of cells, convergence decided on the device -------------
 *
 * The other producer of configurations: relaxing many small cells to their local minima under the current potential while
 * the extrapolation grade is watched (MLIP's `relax`).  The layout, the slot coordinates, the force / grade call, the
 * capture and the monitor block are those of the batched sampling; the minimiser is FIRE (Bitzek et al., PRL 97, 170201)
 * with the per-step displacement cap of LAMMPS' min_style fire, one state machine per configuration.  A step s = 0, 1, ... is
 *   mtp_ghosts_forward -> force call -> mtp_ghosts_reverse[_finish]
 *   -> on a grade step: the per-configuration grades -> mtp_sample_capture   (BEFORE the minimiser: a configuration over
 *      threshold_break freezes at the positions that were graded)
 *   -> mtp_relax_step(s)
 * d_frozen[k] is the status of configuration k: 0 running, 1 frozen by mtp_sample_capture, 2 converged, 3 failed (non-finite
 * forces).  Any non-zero status means that no row of the configuration is written again, by this call or by the mtp_sample_*
 * ones; d_counts[2] (mtp_sample_capture's, and what mtp_sample_monitor reports as "frozen") counts all three.
 */
typedef struct mtp_relax_params {
  double ftol;        /* >= 0: converged when the largest |f_i| of the configuration is <= ftol [eV/A] */
  double dt_max;      /* > 0: the largest time step [ps] */
  double dmax;        /* > 0: the largest displacement of a coordinate in one step [A] */
  double f_inc;       /* >= 1 */
  double f_dec;       /* in (0, 1) */
  double alpha_start; /* in [0, 1] */
  double f_alpha;     /* in (0, 1] */
  int n_min;          /* >= 0: downhill steps before dt grows */
} mtp_relax_params;
/* One FIRE step of every non-empty configuration k with d_frozen[k] == 0, from the folded forces d_f of its rows (metal
 * units; masses per type as 1 / m in d_inv_mass).  One launch; a workgroup of four wavefronts owns four consecutive
 * configurations, a wavefront serves a segment of up to 256 rows and the whole workgroup a longer one (as mtp_batch_reduce),
 * every sum in a fixed order without floating-point atomics: a configuration's result depends on its own rows only.
 *   1. P = sum f.v, vv = sum v.v, ff = sum f.f, fmax2 = max_i |f_i|^2;  d_fmax[k] = sqrt(fmax2)
 *   2. ff not finite:       d_frozen[k] = 3, d_done_step[k] = step, ++d_counts[2]; no row is written
 *      fmax2 <= ftol^2:     d_frozen[k] = 2, d_done_step[k] = step, ++d_counts[2]; its rows of v are set to 0, x is not written
 *      (with `last` != 0 the call ends here: it only decides; neither the state nor a row of a running configuration is written)
 *   3. P > 0:   a = 1 - alpha, b = alpha sqrt(vv / ff), ++npos; if npos > n_min: dt = min(dt f_inc, dt_max), alpha *= f_alpha
 *      else:    a = b = 0, npos = 0, alpha = alpha_start; dt *= f_dec only if vv > 0 (a configuration at rest, as at step 0,
 *               is not punished)
 *   4. v' = a v + b f;  vmax = the largest |v'| component of the configuration;  dtv = dt, or dmax / vmax if dt vmax > dmax;
 *      x += dtv v';  v = v' + (dtv ftm2v / m) f
 * d_dt, d_alpha, d_npos [ncfg] are the state (the caller starts them at dt, alpha_start and 0; velocities at 0).  d_fmax and
 * d_done_step of a configuration that is empty or already frozen are not written.  ncfg == 0 launches nothing.  MTP_ERR_ARG,
 * nothing launched, for a NULL stream (no context), ncfg < 0, step < 0, a missing array or parameters that are not finite
 * or outside the ranges above. */
int mtp_relax_step(void *stream, int ncfg, const int *d_cfg_first, const mtp_relax_params *params, int step, int last,
                   double *d_x, double *d_v, const double *d_f, const int *d_type, const double *d_inv_mass, double *d_dt,
                   double *d_alpha, int *d_npos, int *d_frozen, int *d_done_step, double *d_fmax, int *d_counts /*[3]*/);

/* ---- batched variable-cell relaxation: the cells relax with their atoms, under a pressure ----------------------------
 *
 * mtp_relax_step with the cell among the degrees of freedom.  Row-vector convention throughout: a cell h has the lattice
 * vectors as rows, x = s . h, and the virial is W = -dE/d(eps) for x -> x (I + eps), components xx yy zz xy xz yz (what
 * mtp_batch_reduce leaves per configuration from a force call with MTP_VIRIAL_ATOM).  Per configuration k:
 *   h0 [9]     the cell given;  D [9], starting at I: the current cell is h = h0 . D
 *   xt [n][3]  reference-frame positions: x - origin = xt . D
 *   the generalised coordinates are the n rows of xt and the three rows of L D, L [A] = cell_factor (times the
 *   configuration's atom count with factor_per_atom != 0); the generalised velocities are vt [n][3] and vq [9] [A/ps].
 * Generalised forces from the folded forces f and the virial W:
 *   ft_i = f_i . D^T
 *   W'   = (W - p V I) o mask,  V = det h, mask the symmetric 0/1 matrix of cell_mask[6] (order as W);
 *          isotropic != 0:  W' <- (tr W' / 3) I
 *   G    = D^-T . W' / L        [eV/A]  (= -d(E + p V)/d(L D) when the mask is all ones)
 * `pressure` is in eV/A^3 (1 GPa = 1 / 160.21766 eV/A^3).  A step s is
 *   mtp_ghosts_forward -> force call with per-atom virial -> mtp_ghosts_reverse_finish -> mtp_batch_reduce (W)
 *   -> on a grade step: the grades -> mtp_sample_capture -> mtp_relax_cell_capture_cells
 *   -> mtp_relax_cell_step(s) -> mtp_ghosts_deform
 * and a re-neighbouring reads d_h back, builds ghosts and list for those cells and calls mtp_relax_cell_rebase.
 */
typedef struct mtp_relax_cell_params {
  mtp_relax_params fire; /* as for mtp_relax_step; dmax caps every generalised component: |dD_ab| <= dmax / L a step */
  double stol;           /* >= 0: converged needs max_ab |W'_ab| / V <= stol [eV/A^3] as well */
  double pressure;       /* finite [eV/A^3] */
  double cell_factor;    /* > 0, finite: L [A], or L per atom */
  double cell_mass;      /* > 0, finite: the mass of the cell coordinates [g/mol] */
  int cell_mask[6];      /* 0 or 1 each: which components of W' drive the cell (xx yy zz xy xz yz) */
  int isotropic;         /* != 0: the cell changes its volume only */
  int factor_per_atom;   /* != 0: L = cell_factor times the atom count of the configuration */
} mtp_relax_cell_params;
/* The device arrays of mtp_relax_cell_step: per owned row, per atom type, per configuration.  All are the caller's. */
typedef struct mtp_relax_cell_arrays {
  const int *cfg_first;   /* [ncfg + 1] */
  double *x;              /* [n][3] slot coordinates: written as origin + xt . D for the rows that move */
  double *xt, *vt;        /* [n][3] */
  const double *f;        /* [n][3] folded forces */
  const int *type;        /* [n] */
  const double *inv_mass; /* per type */
  const double *virial;   /* [ncfg][6] W */
  const double *h0;       /* [ncfg][9] */
  const double *origins;  /* [ncfg][3] */
  double *D, *vq;         /* [ncfg][9] */
  const double *Dbinv;    /* [ncfg][9] inverse of D at the last rebuild (mtp_relax_cell_rebase; I at the start) */
  const double *href;     /* [ncfg][9] the cell at the last rebuild */
  const int *nimg;        /* [ncfg][3] images per direction and sign at the last rebuild (mtp_ghosts_cell_bounds) */
  double *dt, *alpha;     /* [ncfg] FIRE state, as for mtp_relax_step */
  int *npos, *frozen, *done_step;
  double *fmax, *smax;    /* [ncfg] */
  double *gcell;          /* [ncfg][9] G */
  double *h;              /* [ncfg][9] the current cell: start it at h0 */
  double *T;              /* [ncfg][9] Dbinv . D after the move: what mtp_ghosts_deform takes */
  double *cellmove;       /* [ncfg] the list-validity measure of the cell, below */
  int *counts;            /* [3] mtp_sample_capture's */
} mtp_relax_cell_arrays;
/* One FIRE step over the extended degrees of freedom of every non-empty configuration with frozen[k] == 0.  One launch, the
 * layout, the wavefront / workgroup split and the fixed-order reductions of mtp_relax_step:
 *   1. P, vv, ff over the n + 3 generalised rows (ft, vt; then G, vq: the cell rows are added to the atom total, entry by
 *      entry in storage order) and fmax2 = max_i |f_i|^2 over the TRUE forces
 *   2. smax = max_ab |W'_ab| / V;  fmax[k] = sqrt(fmax2), smax[k], gcell[k] = G, h[k] = h0 . D are written
 *   3. ff, a component of W, V or det D not finite, or det D <= 0:  frozen[k] = 3 (failed), as in mtp_relax_step
 *   4. fmax2 <= ftol^2 and smax <= stol:  frozen[k] = 2 (converged); vt and vq are set to 0, nothing else is written
 *   5. with `last` != 0 the call ends here
 *   6. the FIRE rules of mtp_relax_step (a, b, npos, dt, alpha), vmax and ONE dtv with the dmax cap over all generalised
 *      components
 *   7. xt += dtv vt';  D += dtv vq' / L;  vt = vt' + (dtv ftm2v / m_i) ft;  vq = vq' + (dtv ftm2v / cell_mass) G;
 *      x = origin + xt . D (the new ones);  h[k] = h0 . D and T[k] = Dbinv . D for the new D
 *   8. cellmove[k] = sum_a (nimg[k][a] + 1) |h_a - href_a|  [A], rows a of the new cell: an image that is not a ghost of the
 *      last build has |n_a| <= nimg_a + 1 (or lies a whole plane spacing further out) and moves by n . (h - href) against
 *      its owner, so a pair distance changes by at most two atom displacements plus cellmove.
 * MTP_ERR_ARG, nothing launched: as mtp_relax_step, and stol < 0, pressure / cell_factor / cell_mass not finite,
 * cell_factor <= 0, cell_mass <= 0, a mask entry that is neither 0 nor 1, a missing array. */
int mtp_relax_cell_step(void *stream, int ncfg, const mtp_relax_cell_params *params, int step, int last,
                        const mtp_relax_cell_arrays *arrays);
/* After a re-neighbouring (which wrapped d_x and translated it to d_origins): xt = (x - origin) . D^-1 for every owned row
 * and Dbinv[k] = D[k]^-1, for the configurations with det D > 0 (the others are left as they are). */
int mtp_relax_cell_rebase(void *stream, int ncfg, int nrows, const int *d_row_cfg, const double *d_origins, const double *d_x,
                          const double *d_D, double *d_xt, double *d_Dbinv);
/* Right after mtp_sample_capture: d_cand_cell[slot[k]][9] = d_h[k] for 0 <= slot[k] < max_candidates, so that a candidate
 * carries the cell it was graded in. */
int mtp_relax_cell_capture_cells(void *stream, int ncfg, const int *d_slot, int max_candidates, const double *d_h,
                                 double *d_cand_cell);
/* Ghosts that follow a deforming cell between re-neighbourings: shift[k] = shift_at_build[k] . T[cfg(owner[k])] with
 * d_row_cfg [nlocal] (mtp_sample_row_map) and d_T [ncfg][9] (T = D_build^-1 . D_now, written by mtp_relax_cell_step).  The
 * handle keeps a copy of the shifts of the last build (made by the first call after it), so rounding does not accumulate
 * over the steps; mtp_ghosts_forward / reverse / reverse_finish / types work unchanged. */
int mtp_ghosts_deform(mtp_ghosts *g, void *stream, const int *d_row_cfg, const double *d_T /*[ncfg][9]*/);

/* ---- batched constant-pressure sampling: Langevin MD of a whole batch of cells at a target pressure (NPT) -------------
 *
 * The batched sampling with the cell moved by stochastic cell rescaling, a first-order stochastic barostat in the spirit of
 * Bernetti & Bussi, J. Chem. Phys. 153, 114107 (2020).  Conventions of the variable-cell relaxation above: rows of h are the
 * lattice vectors, x - origin = s . h, W [eV] is the configurational virial for x -> x (I + eps) (xx yy zz xy xz yz, what
 * mtp_batch_reduce leaves from a force call with MTP_VIRIAL_ATOM), pressure in eV/A^3.  Per configuration k, V = det h and
 * kT = kB T[k]:
 *   Kt_ab = mvv2e sum_i m_i v_ia v_ib   the kinetic tensor [eV];   Wt = W + Kt
 *   M     = compressibility / (3 tau_p V0),  V0 the volume of the cell AS GIVEN [1 / (eV ps)]: a constant of the run, so no
 *           mobility-gradient term arises
 * One barostat move over a time dt is the symmetric log-strain
 *   A = M dt [(Wt - p V I + kT I) o mask] + sqrt(2 kT M dt) N o mask,     N_aa = xi_aa,  N_ab = N_ba = xi_ab / sqrt(2)
 *   isotropic != 0:  A <- (tr A / 3) I  (the three diagonal mask entries must be 1)
 *   every |A_ab| is capped at strain_max, keeping its sign; capped[k] counts the steps at which a component was
 *   E = I + A + A^2/2 + A^3/6 + A^4/24,  Einv the same series in -A.  strain_max <= 0.05 is required; at the default 0.01 the
 *       truncation is below |3 A|^5 / 120 < 3e-10, far under the step's own O(dt) error
 *   x - origin <- (x - origin) . E,  v <- v . Einv,  h <- h . E,  T <- T . E
 * Where the + kT I comes from.  At fixed scaled positions and scaled momenta the flow h -> h exp(t S), S symmetric, preserves
 * the Haar measure dh / V^3 of the cells.  The target exp(-beta (K + U + p V)) V^-2 dh (isotropic: dV) has the density
 * rho = exp(-beta (K + U + p V)) V against that measure, and the logarithmic derivative of rho along the generator S is
 * beta (Wt - p V I) : S + tr S (the momenta scale with Einv, hence Kt beside W).  The move is one Euler-Maruyama step of the
 * overdamped Langevin equation dA = M kT grad(log rho) dt + sqrt(2 M kT) dB in the Frobenius metric of the symmetric
 * matrices, of which rho is the stationary density.  Flexible cells also rotate slowly (symmetric strains do not commute);
 * energies, forces and virials are invariant under it and nothing removes it.
 * Noise: xi = sqrt(12) (u - 0.5), u = (w + 0.5) 2^-32 from Philox4x32-10 as in mtp_sample_final -- uniform with zero mean, unit
 * variance and zero third moment, all a weak first-order scheme needs (and what fix langevin does); no transcendental function.
 * Key: `seed`; counter (step, 0x80000000 + j, low word of key[k], high word of key[k]): call j = 0 gives xx, yy, zz from the
 * words 0, 1, 2, call j = 1 xy, xz, yz.  Atom indices stay below 2^31, so these counters never meet an atom's.
 * A step s = 1, 2, ... is
 *   mtp_sample_cell_step(s) -> mtp_ghosts_deform(T) -> force call with per-atom virial -> mtp_ghosts_reverse_finish
 *   -> mtp_batch_reduce (W) -> mtp_sample_final -> on a grade step: mtp_sample_capture -> mtp_relax_cell_capture_cells
 * so that the forces of a kick are always those of the positions and the cell they were computed in, while the W that drives
 * the cell at step s is the one of the force call of step s - 1: a one-step lag, an O(dt) error of the same order as the
 * Euler-Maruyama move itself.
 */
typedef struct mtp_sample_cell_params {
  double dt;              /* > 0, finite [ps] */
  double dtf;             /* finite: 0.5 dt ftm2v, as for mtp_sample_initial */
  double tau_p;           /* [ps]; not finite or <= 0: the barostat is off */
  double compressibility; /* > 0, finite [A^3/eV]: an estimate; it sets the time scale only */
  double pressure;        /* finite [eV/A^3] */
  double strain_max;      /* in (0, 0.05] */
  int cell_mask[6];       /* 0 or 1 each (xx yy zz xy xz yz); all 0: the barostat is off */
  int isotropic;          /* != 0: the cell changes its volume only */
  unsigned long long seed;
} mtp_sample_cell_params;
/* The device arrays of mtp_sample_cell_step: per owned row, per atom type, per configuration.  All are the caller's. */
typedef struct mtp_sample_cell_arrays {
  const int *cfg_first;          /* [ncfg + 1] */
  double *x, *v;                 /* [n][3] slot coordinates, velocities */
  const double *f;               /* [n][3] folded forces (with the thermostat's, as mtp_sample_final left them) */
  const int *type;               /* [n] */
  const double *inv_mass, *mass; /* per type */
  const double *virial;          /* [ncfg][6] W of the previous force call */
  const double *temperature;     /* [ncfg] */
  const unsigned long long *key; /* [ncfg] */
  const double *origins;         /* [ncfg][3] */
  const double *V0;              /* [ncfg] */
  double *h;                     /* [ncfg][9] the current cell: start it at the cell given */
  double *T;                     /* [ncfg][9] the deformation since the last rebuild: what mtp_ghosts_deform takes (start: I) */
  const double *href;            /* [ncfg][9] the cell at the last rebuild */
  const int *nimg;               /* [ncfg][3] as for mtp_relax_cell_step */
  int *frozen, *done_step;       /* [ncfg] */
  double *cellmove;              /* [ncfg] mtp_relax_cell_step's list-validity measure */
  int *capped;                   /* [ncfg] */
  double *press;                 /* [ncfg] tr Wt / (3 V) of the last step [eV/A^3] */
  int *counts;                   /* [3] mtp_sample_capture's */
} mtp_sample_cell_arrays;
/* The first half step of every non-empty configuration with frozen[k] == 0, with its barostat move.  One launch; the work
 * split, the segment rule (a wavefront up to 256 rows, the workgroup above) and the fixed-order reductions without
 * floating-point atomics of mtp_relax_cell_step:
 *   1. kick: v += dtf f / m  (mtp_sample_initial's expression);  the six components of Kt from the kicked velocities
 *   2. a component of W or Kt, V or V0 not finite, V <= 0 or V0 <= 0:  frozen[k] = 3 (failed), done_step[k] = step,
 *      ++counts[2]; none of its rows or cell state is written
 *   3. press[k] = tr Wt / (3 V)
 *   4. barostat off (tau_p, or an all-zero mask):  x += dt v -- rows come out bit for bit as mtp_sample_initial leaves them;
 *      h, T, cellmove and capped are not written, nothing is drawn
 *   5. otherwise A, E, Einv as above from V = det h and the W given;  x = origin + ((x - origin) + dt v) . E;  v = v . Einv;
 *      h = h . E, T = T . E;  cellmove[k] as mtp_relax_cell_step (8.) defines it
 * MTP_ERR_ARG, nothing launched: a NULL stream (no context), ncfg < 0, step < 0, a missing array, dt not positive or not
 * finite, dtf / pressure / compressibility not finite, compressibility <= 0, strain_max outside (0, 0.05], a mask entry that
 * is neither 0 nor 1, isotropic with a diagonal mask entry of 0. */
int mtp_sample_cell_step(void *stream, int ncfg, const mtp_sample_cell_params *params, int step,
                         const mtp_sample_cell_arrays *arrays);

/* ---- batched nudged elastic band: minimum-energy paths of a whole batch of bands, decided on the device --------------
 *
 * What follows the minima: the path between two of them and its barrier.  A band is a run of M >= 3 CONSECUTIVE
 * configurations (its images) of the batched layout with the same atom count, the same types and the same, fixed cell; band b
 * is the configurations [band_first[b], band_first[b + 1]).  Its first and last image are never moved.  The bands of a batch
 * are independent; the images of a band are not -- this is the one kernel of the batched family that couples configurations.
 * The method is the climbing-image NEB with the improved tangent (Henkelman & Jonsson, J. Chem. Phys. 113, 9978; Henkelman,
 * Uberuaga & Jonsson, ibid. 9901), minimised by the FIRE state machine of mtp_relax_step, ONE per band.  Layout, slot
 * coordinates, force / grade call, capture and monitor block are those of the batched relaxation; a step s = 0, 1, ... is
 *   mtp_ghosts_forward -> force call with MTP_ENERGY_ATOM -> mtp_ghosts_reverse[_finish]
 *   -> on a grade step: the per-configuration grades -> mtp_sample_capture
 *   -> mtp_neb_step(s)
 * Re-neighbouring wraps every image into the cell on its own, so neighbouring images may differ by lattice vectors: all
 * differences between images go through the minimum image mic(d) = d - rint(d . h^-1) . h (row vectors, rint to even), which
 * is the true difference as long as no atom moves more than a quarter of the smallest cell height between two images.
 */
#define MTP_NEB_MAX_IMAGES 64 /* the image energies and the per-image totals of a band live in LDS */
typedef struct mtp_neb_params {
  mtp_relax_params fire; /* as for mtp_relax_step; ftol bounds the largest |F_neb| of a row */
  double spring;         /* > 0, finite: the spring constant between neighbouring images [eV/A^2] */
  int climb_step;        /* the first step with a climbing image; < 0: never */
} mtp_neb_params;
/* The device arrays of mtp_neb_step.  All are the caller's. */
typedef struct mtp_neb_arrays {
  const int *band_first;   /* [nband + 1] configuration indices: the device copy of the host table given to the call */
  const int *cfg_first;    /* [ncfg + 1] */
  double *x, *v;           /* [n][3] slot coordinates, velocities (start: 0) */
  const double *f;         /* [n][3] folded forces */
  const double *eatom;     /* [n] per-atom energies of the same force call */
  const int *type;         /* [n] */
  const double *inv_mass;  /* per type */
  const double *origins;   /* [ncfg][3] */
  const double *cell;      /* [nband][9] h, rows = lattice vectors */
  const double *cell_inv;  /* [nband][9] h^-1 */
  double *fneb;            /* [n][3] F_neb */
  double *energy;          /* [ncfg] E_i */
  double *dt, *alpha;      /* [nband] FIRE state, as for mtp_relax_step */
  int *npos, *done_step;   /* [nband] */
  double *fmax;            /* [nband] */
  int *climber;            /* [nband] the climbing image of the last step looked at (its index within the band), -1: none */
  int *band_status;        /* [nband] 0 running, 1 stopped by a capture, 2 converged, 3 failed */
  int *frozen;             /* [ncfg] mtp_sample_capture's and mtp_sample_monitor's: every image of a stopped band is set */
  int *counts;             /* [3] mtp_sample_capture's */
} mtp_neb_arrays;
/* One NEB step of every band with band_status[b] == 0.  One launch, one workgroup of 256 threads per band: an image is served
 * by one wavefront (the four of the workgroup take the images in turn), the FIRE sweeps over the interior rows -- consecutive
 * rows -- by the whole workgroup.  Every floating-point sum has a fixed order (the reductions of mtp_relax_step; per-image
 * totals are added in image order) and there are no floating-point atomics: a band's result depends on its own rows only,
 * whatever the batch around it.  The one atomic is the integer count counts[2].  Images are i = 0 ... M - 1, rows of image i
 * are those of configuration band_first[b] + i; "interior" is 0 < i < M - 1.
 *   1. capture check: if frozen[k] != 0 for an image of the band (mtp_sample_capture froze it), band_status[b] = 1,
 *      done_step[b] = step, every image still at 0 gets frozen[k] = 1 and is added to counts[2]; NOTHING else is written
 *   2. E_i = the sum of the image's rows of eatom;  energy[k] = E_i
 *   3. tangents, for every interior image and each of its atoms j, on cell coordinates c = x - origins[k]:
 *        D+ = mic(c_{i+1} - c_i),  D- = mic(c_i - c_{i-1})
 *        E_{i+1} > E_i > E_{i-1}:  tau = D+;    E_{i+1} < E_i < E_{i-1}:  tau = D-;    otherwise, with
 *        big / small = the larger / smaller of |E_{i+1} - E_i| and |E_{i-1} - E_i|:
 *        tau = big D+ + small D- if E_{i+1} > E_{i-1}, else small D+ + big D-
 *      |tau| = sqrt(sum over atoms and components of tau^2);  |tau| zero or not finite: the band fails (5.)
 *   4. F.t = (sum F tau) / |tau|;  |D+|, |D-| the norms over the whole image;
 *        F_neb = F + g tau,  g = (spring (|D+| - |D-|) - F.t) / |tau|      (= F - (F.t) t + spring (|D+| - |D-|) t)
 *      from step >= climb_step >= 0 the interior image of the highest E_i (the lowest index on a tie) climbs instead:
 *        g = -2 F.t / |tau|                                                  (= F - 2 (F.t) t)
 *      climber[b] = its index, -1 before that step;  fneb = F_neb for the interior rows, 0 for the rows of both end images
 *   5. FIRE, rules 1 to 4 of mtp_relax_step over the interior rows of the WHOLE band with F_neb in place of f:
 *      P = sum F_neb.v, vv, ff, fmax2 = the largest |F_neb|^2 of a row;  fmax[b] = sqrt(fmax2)
 *      ff not finite (or 3. failed; or an E_i that is not finite, after which nothing of 3. and 4. is written, fmax[b] = 0 and
 *      climber[b] = -1; or images of different atom counts, for which nothing of 2. to 4. is written either):
 *                           band_status[b] = 3, frozen[k] = 3 for ALL its images, done_step[b] = step, counts[2] += M
 *      fmax2 <= ftol^2:     band_status[b] = 2, frozen[k] = 2 for all its images, done_step[b] = step, counts[2] += M;
 *                           the interior rows of v are set to 0, x is not written
 *      (with `last` != 0 the call ends here: it only decides, and has written fneb, energy, fmax and climber)
 *      then a, b, npos, dt, alpha by rule 3 of mtp_relax_step from the band's dt[b], alpha[b], npos[b];  v' = a v + b F_neb;
 *      vmax over the interior rows;  dtv = dt, or dmax / vmax if dt vmax > dmax;  x += dtv v';  v = v' + (dtv ftm2v / m) F_neb
 *      No row of the two end images is written, ever.
 *   6. MTP_ERR_ARG, nothing launched: a NULL stream (no context), nband < 0, ncfg < 0, step < 0, a missing array (nband > 0),
 *      FIRE parameters outside the ranges of mtp_relax_params, spring not finite or <= 0, and a band table -- the HOST copy
 *      band_first [nband + 1], the only thing the check can read without waiting for the device -- that starts below 0, ends
 *      above ncfg or has a band of fewer than 3 or more than MTP_NEB_MAX_IMAGES images.  (A band for which the device copy
 *      says so is skipped by the kernel.)  Equal atom counts and types within a band are the caller's to check on the host.
 * nband == 0 launches nothing.  The caller starts dt, alpha, npos as for mtp_relax_step, done_step and climber at -1,
 * band_status and v at 0. */
int mtp_neb_step(void *stream, int nband, const int *band_first /* host */, int ncfg, const mtp_neb_params *params, int step,
                 int last, const mtp_neb_arrays *arrays);

/* ---- batched force constants: the Hessian of every configuration of a batch by central differences ----------------------
 *
 * What follows the stationary points: their second derivatives (is a minimum a minimum, has a saddle one unstable mode, the
 * harmonic prefactor of a rate, Gamma-point phonons).  H = -dF/dx by central differences of the forces with a step h that is
 * far inside the skin: ONE ghost build and ONE list serve all the force calls of a pass, and nothing is read back between
 * them.  Layout, slot coordinates and force call are those of the batched relaxation.
 *
 * Selection: configuration j differentiates with respect to m_j <= n_j of its owned atoms, sel[sel_first[j] ...
 * sel_first[j + 1]) -- ROW numbers of the batch, each within the configuration's own rows, none repeated.
 * H_j is [3 m_j][3 m_j], row-major, at H + h_first[j], h_first[j] = sum_{i < j} (3 m_i)^2.  Row c = 3 a + d is the displaced
 * coordinate (selected atom a, direction d), column r = 3 b + e the responding one (the force on selected atom b along e).
 *
 * A pass is K + 1 launches of mtp_hess_step, K = 6 sel_max with sel_max >= every m_j, around K + 1 force calls:
 *   x0 = x;  for k = 0 ... K:  mtp_ghosts_forward -> force call with MTP_ENERGY_ATOM -> mtp_ghosts_reverse[_finish]
 *                               -> mtp_hess_step(k)
 *   mtp_hess_finish
 * Displacement k < K moves the selected atom a = k / 6 of every configuration with m_j > a along d = (k % 6) / 2, by +h for
 * even k and by -h for odd k.  Launch k, for a configuration with status[j] == 0 (any other is skipped: nothing of it is
 * written) and at least one row:
 *   1. k == 0: f0 = f on its owned rows, fmax[j] = sqrt(the largest |f0|^2 of a row), energy[j] = the sum of its rows of
 *      eatom.  A component of f0 that is not finite -- or a selection that is longer than the configuration or sel_max or
 *      names a row outside the configuration -- sets status[j] = MTP_HESS_FAILED; no displacement is made.
 *   2. k >= 1, m_j > a' (a', d' of displacement k - 1, row c = 3 a' + d'): f holds the forces of that displacement.  After a
 *      +h call the row is parked, H[c][r] = f[sel b][e]; after the -h call H[c][r] = (f[sel b][e] - H[c][r]) * inv2h with
 *      inv2h = 1 / (2 h) computed once on the host in double -- this expression and no other.  If one of the 3 m_j components
 *      is not finite, nothing of the row is written and status[j] = MTP_HESS_FAILED.
 *   3. k >= 1, m_j > a': the moved coordinate is put back from the saved copy, x[row][d'] = x0[row][d'] (a failed
 *      configuration too: after the pass x == x0 to the bit).
 *   4. k < K, m_j > a, not failed: x[row][d] = x0[row][d] + h, or x0[row][d] - h.
 * Segments of up to 256 rows are served by a wavefront, longer ones by the workgroup (the split of mtp_relax_step); every
 * floating-point sum has a fixed order and every expression is evaluated as written (no fused multiply-add): a
 * configuration's result depends on its own rows only, whatever the batch around it.
 * MTP_ERR_ARG, nothing launched: a NULL stream, ncfg < 0, sel_max < 0 or above MTP_HESS_MAX_SELECTED, k outside
 * [0, 6 sel_max], h not finite or <= 0, a missing array (ncfg > 0).  ncfg == 0 launches nothing.  The caller starts status,
 * fmax and energy at 0. */
#define MTP_HESS_FAILED 1
#define MTP_HESS_MAX_SELECTED (1 << 28)
int mtp_hess_step(void *stream, int ncfg, const int *d_cfg_first, const int *d_sel_first, const int *d_sel, int sel_max, int k,
                  double h, double *d_x, const double *d_x0, const double *d_f, const double *d_eatom, const long long *d_h_first,
                  double *d_H, double *d_f0, double *d_fmax, double *d_energy, int *d_status);
/* The end of a pass, one launch, for every configuration with status[j] == 0 and m_j > 0 (a wavefront for up to 256 selected
 * atoms, the workgroup for more):
 *   1. diag[j][0] = asymmetry = max |H_cr - H_rc| of the matrix as harvested (an O(h^2) truncation quantity)
 *   2. diag[j][1] = sum_rule = max_{c, e} |sum_b H[c][3 b + e]|, also of the matrix as harvested, the sum over b = 0 ...
 *      m_j - 1 in that order: the total force that displacement c left on the selected atoms, over 2 h -- the
 *      translation-invariance residual of the force call, of rounding size when m_j = n_j and meaningless otherwise.  (The
 *      column sums, and with them the row sums of the symmetrised matrix, vanish only to O(h^2).)
 *   3. H <- 0.5 (H + H^T): a pair is read once and both members are written by the same thread
 *   4. mass_weight != 0: H[c][r] *= 1 / sqrt(M_a M_b), M = d_mass[d_type[row] - 1]
 * MTP_ERR_ARG, nothing launched: a NULL stream, ncfg < 0, a missing array (ncfg > 0). */
int mtp_hess_finish(void *stream, int ncfg, const int *d_sel_first, const int *d_sel, const int *d_type, const double *d_mass,
                    int mass_weight, const long long *d_h_first, double *d_H, double *d_diag /* [ncfg][2] */,
                    const int *d_status);

/* ---- batched elastic constants: the second derivatives of every configuration of a batch with respect to its cell ------
 *
 * What the force constants leave out: the Hessian of the cell degrees of freedom.  Stress-strain coefficients by central
 * differences of the stress, and the force-strain coupling by central differences of the forces, over the twelve homogeneous
 * strains x -> x (I +- h E_w), h far inside the skin over the list cutoff: ONE ghost build and ONE list serve the thirteen
 * force calls of a pass, and nothing is read back between them.  Layout, slot coordinates and the force call with per-atom
 * virials are those of the batched variable-cell relaxation: the cell h0 has the lattice vectors as rows, W = -dE/d(eps) for
 * x -> x (I + eps) is what mtp_batch_reduce leaves per configuration, components xx yy zz xy xz yz everywhere.
 *
 * Definitions, per configuration j of n_j atoms, N = 3 n_j:
 *   strain k = 0 ... 11: component w = k / 2, amplitude s = +h (k even) or -h (k odd), D = I + s E_w; E_w has a 1 on the
 *     diagonal for w < 3 and 0.5 on BOTH off-diagonal entries otherwise (engineering shear).  The atoms move at fixed scaled
 *     coordinates, x[r][b] = origin[b] + ((xt[r][0] D[0][b] + xt[r][1] D[1][b]) + xt[r][2] D[2][b]), and the ghosts follow
 *     through mtp_ghosts_deform with T = D.
 *   stress: sigma_v = -(W_v / V), V = det(h0) * det(D) (both by cofactors along the first row), the Cauchy stress [eV/A^3]
 *   Bt [6][6]:       Bt[w][v] = (sigma_v(+h E_w) - sigma_v(-h E_w)) * inv2h, inv2h = 1 / (2 h) computed once on the host
 *   coupling [6][N]: Lambda[w][3 i + d] = (f_id(+h E_w) - f_id(-h E_w)) * inv2h, at c_first[j] = 18 * cfg_first[j]
 * A pass is thirteen launches of mtp_elastic_step around thirteen force calls:
 *   x0 = x;  for k = 0 ... 12:  mtp_ghosts_forward -> force call with MTP_ENERGY_ATOM and MTP_VIRIAL_ATOM ->
 *                                mtp_ghosts_reverse_finish -> mtp_batch_reduce (W) -> mtp_elastic_step(k) -> mtp_ghosts_deform(T)
 *   mtp_elastic_finish [-> the pass of mtp_hess_step at D = I -> mtp_hess_finish -> mtp_elastic_relax]
 * Launch k, for a configuration with status[j] == 0 (any other is skipped: nothing of it is written) and at least one row:
 *   1. k == 0: f0 = f on its rows, fmax[j] = sqrt(the largest |f0|^2 of a row), energy[j] = the sum of its rows of eatom,
 *      stress0[j][v] = -(W_v / V0), V0 = det(h0).  A component of f0 or of W that is not finite, or V0 that is not a positive
 *      finite number, sets status[j] = MTP_ELASTIC_FAILED.
 *   2. k >= 1 harvests strain k - 1 (w', its sign): after the +h call the six stresses and the N forces are parked in row w'
 *      of Bt and of the coupling; after the -h call out = (parked - now) * inv2h -- this expression and no other.  If one of
 *      the 6 + N numbers is not finite, nothing of the two rows is written and status[j] = MTP_ELASTIC_FAILED.
 *   3. the geometry of strain k: k < 12: T[j] = D_k and x as above; k == 12: x = x0 from the saved copy, to the bit, and
 *      T[j] = I.  A configuration that failed in 1. or 2. is returned to x0 and T[j] = I by the launch that failed it.
 * Segments of up to 256 rows are served by a wavefront, longer ones by the workgroup (the split of mtp_relax_step); every
 * floating-point sum has a fixed order and every expression is evaluated as written (no fused multiply-add): a
 * configuration's result depends on its own rows only, whatever the batch around it.
 * MTP_ERR_ARG, nothing launched: a NULL stream, ncfg < 0, k outside [0, 12], h not finite or <= 0, a missing array
 * (ncfg > 0).  ncfg == 0 launches nothing.  The caller starts status, fmax and energy at 0. */
#define MTP_ELASTIC_FAILED 1
#define MTP_ELASTIC_UNSTABLE 2
int mtp_elastic_step(void *stream, int ncfg, const int *d_cfg_first, int k, double h, double *d_x, const double *d_x0,
                     const double *d_xt, const double *d_origins, const double *d_h0 /* [ncfg][9] */, const double *d_f,
                     const double *d_eatom, const double *d_virial /* [ncfg][6] */, double *d_T /* [ncfg][9] */,
                     double *d_Bt /* [ncfg][36] */, double *d_coupling, const long long *d_c_first, double *d_f0, double *d_fmax,
                     double *d_energy, double *d_stress0 /* [ncfg][6] */, int *d_status);
/* The end of a pass, one launch, one wavefront for every configuration with status[j] == 0 and at least one row:
 *   1. K[v][w] = 0.5 * ((((d_ik s_jl + d_jk s_il) + d_il s_jk) + d_jl s_ik) - 2 d_kl s_ij) with v = (i, j), w = (k, l),
 *      s = stress0 and d the Kronecker delta as 0.0 / 1.0: Wallace's relation between the stress-strain coefficients under a
 *      residual stress and the second derivatives of the energy with respect to Lagrangian strain
 *   2. B[v][w] = Bt[w][v]: stress component v, strain component w.  NOT symmetric under stress:
 *      B - B^T = d s^T - s d^T + O(h^2), d = (1, 1, 1, 0, 0, 0)
 *   3. M = B - K; diag[j][0] = asymmetry = max_{v < w} |M[v][w] - M[w][v]| (an O(h^2) truncation quantity);
 *      C[v][w] = C[w][v] = 0.5 * (M[v][w] + M[w][v]): a pair is read once and both members are written by one lane
 *   4. diag[j][1] = sum_rule = max_{w, d} |sum_i Lambda[w][3 i + d]|, the sum over the atoms i = 0 ... n_j - 1 in that order:
 *      the translation-invariance residual of the force call, of rounding size
 * MTP_ERR_ARG, nothing launched: a NULL stream, ncfg < 0, a missing array (ncfg > 0). */
int mtp_elastic_finish(void *stream, int ncfg, const int *d_cfg_first, const long long *d_c_first, const double *d_coupling,
                       const double *d_stress0, const double *d_Bt, double *d_B /* [ncfg][36] */, double *d_C /* [ncfg][36] */,
                       double *d_diag /* [ncfg][2] */, const int *d_status);
/* Relaxed ions, one launch per LDS tier, one workgroup for every configuration with status[j] == 0 and 0 < N <=
 * MTP_ELASTIC_RELAX_MAX_N (a larger one is left as it is: the caller solves it on the host).  H_j [N][N] at H + h_first[j]
 * is the symmetrised, NOT mass-weighted Hessian of a full selection in the order of the rows (mtp_hess_finish).
 *   1. A = H + tau sum_d t_d t_d^T with the three normalised translations t_d: A[r][c] = H[r][c] + (tau / n) where
 *      r % 3 == c % 3, tau = trace(H) / N.  Lambda^T is orthogonal to the t_d (the sum rule), so A^-1 Lambda^T is the
 *      pseudo-inverse H^+ Lambda^T where H is positive semi-definite with the translations as its only null vectors.
 *   2. A = L L^T in LDS, fp64, packed lower triangle, column by column; a pivot that is <= 0 or not finite sets status[j] =
 *      MTP_ELASTIC_UNSTABLE, and U, B_rel and C_rel of the configuration become NaN (B and C stay)
 *   3. U [6][N] at U + c_first[j]: A U[w] = Lambda'[w], the internal-strain displacements per unit strain, with
 *      Lambda'[w][3 i + d] = Lambda[w][3 i + d] - (sum_i Lambda[w][3 i + d]) / n: what rounding left of a translation is taken out
 *   4. R[v][w] = sum_c Lambda'[v][c] U[w][c] over c = 0 ... N - 1 in that order;
 *      B_rel[v][w] = B[v][w] - R[v][w] / V0,  C_rel[v][w] = C[v][w] - (0.5 * (R[v][w] + R[w][v])) / V0,  V0 = vol[j]
 * A configuration of one atom has the translations as its only degrees of freedom: U = 0, B_rel = B, C_rel = C.
 * This is exact where the forces vanish; d sigma_v / d u_c = -Lambda[v][c] / V has a correction of size |f0| / V otherwise.
 * The tiers: N <= 48, <= 96 and <= 192 take 12, 42 and 154 KiB of LDS a workgroup.
 * MTP_ERR_ARG, nothing launched: a NULL stream, ncfg < 0, a missing array (ncfg > 0). */
#define MTP_ELASTIC_TIER_SMALL 48
#define MTP_ELASTIC_TIER_MIDDLE 96
#define MTP_ELASTIC_RELAX_MAX_N 192
int mtp_elastic_relax(void *stream, int ncfg, const int *d_cfg_first, const long long *d_h_first, const double *d_H,
                      const long long *d_c_first, const double *d_coupling, const double *d_vol, const double *d_B,
                      const double *d_C, double *d_U, double *d_B_rel, double *d_C_rel, int *d_status);


/* ---- batched symmetric eigen-solver: eigenvalues and eigenvectors of every matrix of a ragged batch, in LDS -----------------
 *
 * What follows mtp_hess_finish: the normal modes of a whole batch of force-constant matrices without a copy to the host.  One
 * launch per LDS tier, one workgroup of MTP_BATCH_BLOCK threads per matrix; cyclic two-sided Jacobi in fp64.  Matrix j is
 * [N_j][N_j], row-major, at A + a_first[j] (the blocks of mtp_hess_finish: h_first can be handed over as it is) and is only
 * read; its eigenvalues go ascending to W + w_first[j], its eigenvectors, if d_V is given, to V + a_first[j], row-major, column
 * i belonging to W[i]; info[j] = (sweeps made, off-diagonal Frobenius norm at the end).  A matrix with status[j] != 0 on entry
 * is skipped, nothing of it is written (the status of a Hessian pass can be passed straight in); N_j == 0 writes nothing.
 * Every sum runs in index order or through the fixed-order workgroup total, and no expression is contracted: the results do
 * not depend on the batch a matrix is in.  Per matrix, in this order:
 *   1. a_rc = 0.5 * (x + y) with x = A_rc / (root_r * root_c), y = A_cr / (root_c * root_r), root = d_root + w_first[j] (the
 *      square roots of the masses, one per coordinate), or x = A_rc, y = A_cr without d_root
 *   2. with project (N a multiple of 3): A <- P A P, P = I - sum_d t_d t_d^T, t_d[i] = root_i (or 1) where i % 3 == d,
 *      normalised: tau_i = root_i / sqrt(sum_{k % 3 == i % 3} root_k^2), u[r][d] = sum_{i % 3 == d} a_ri tau_i,
 *      g[d][e] = sum_{i % 3 == d} tau_i u[i][e] (all sums over ascending i), and for r >= c
 *      a_rc <- ((a_rc - tau_r u[c][r % 3]) - u[r][c % 3] tau_c) + (tau_r g[r % 3][c % 3]) tau_c
 *   3. norm = |A|_F: thread t adds a_rc^2 for r N + c = t, t + MTP_BATCH_BLOCK, ..., then the workgroup total.  A norm or a root
 *      that is not finite, or project with N % 3 != 0, fails the matrix: W, V and info become NaN, status[j] = MTP_EIGH_FAILED.
 *      thr = (norm * 2^-53) / N
 *   4. sweeps in the parallel round-robin order: with Ne = N rounded up to even and M = Ne - 1, step s = 0 ... M - 1 rotates
 *      the pairs (M, s) and ((s + i) mod M, (s - i) mod M), i = 1 ... Ne / 2 - 1, each taken as (p, q), p < q; a pair with the
 *      padding index of an odd N is idle.  A pair rotates iff |a_pq| > thr: zeta = (a_qq - a_pp) / (2 a_pq),
 *      t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (t = 1 at zeta = 0), c = 1 / sqrt(1 + t^2), s = t c; a_pp <- a_pp - t a_pq,
 *      a_qq <- a_qq + t a_pq, a_pq <- 0 exactly.  All rotations of a step are computed from the diagonal 2 x 2 blocks first and
 *      parked in LDS; after a barrier the 2 x 2 block B where pairs k1 > k2 of the step meet becomes J1^T B J2 (the rows first:
 *      x_p. = c1 b_p. - s1 b_q., x_q. = s1 b_p. + c1 b_q.; then the columns: b_.p = c2 x_.p - s2 x_.q, b_.q = s2 x_.p + c2 x_.q)
 *      and the columns of V: v_rp <- c v_rp - s v_rq, v_rq <- s v_rp + c v_rq.  A block whose two pairs have s = 0 and the
 *      columns of a pair with s = 0 are left as they are.  Every element is written once per step, from old values.
 *      The solve ends after the first sweep without a rotation, or after max_sweeps sweeps: then status[j] =
 *      MTP_EIGH_NOT_CONVERGED and the state reached is still sorted and written.
 *   5. the diagonal ascending by rank, ties by index: W, the permuted columns of V, info.
 * The tiers: N <= 48 and <= 96 hold A (a packed lower triangle) and V in LDS, 30 and 113 KiB a workgroup (12 and 41 KiB
 * without d_V); N <= 192 holds A alone (153 KiB) and serves d_V == NULL only.  A matrix above its limit -- MTP_EIGH_MAX_N_VECTORS
 * with d_V, MTP_EIGH_MAX_N without -- gets status[j] = MTP_EIGH_TOO_LARGE and nothing else of it is written: the caller solves
 * it on the host.
 * MTP_ERR_ARG, nothing launched: a NULL stream, nmat < 0, max_sweeps < 1, a missing array (nmat > 0; d_root and d_V may be NULL). */
#define MTP_EIGH_FAILED 1          /* a non-finite entry, mass root or norm; or project != 0 with N % 3 != 0 */
#define MTP_EIGH_NOT_CONVERGED 2   /* max_sweeps sweeps and the last one still rotated */
#define MTP_EIGH_TOO_LARGE 3       /* N above the tier that can serve it; nothing else of it is written */
#define MTP_EIGH_TIER_SMALL 48
#define MTP_EIGH_MAX_N_VECTORS 96
#define MTP_EIGH_MAX_N 192
int mtp_eigh_batched(void *stream, int nmat, const int *d_n, const long long *d_a_first, const double *d_A,
                     const long long *d_w_first, const double *d_root /* [sum N_j] or NULL */, int project, int max_sweeps,
                     double *d_W, double *d_V /* or NULL */, double *d_info /* [nmat][2] */, int *d_status);


/* ---- MaxVol selection: which candidate vectors enter the active set ------------------------------------------------
 *
 * The step of the active-learning loop that consumes the grades (MLIP's select-add; the reference only grades,
 * pair_mtp_extrapolation.cpp:347-358, and writes the pre-selected configurations, :401-479).
 *
 * Convention.  The reference grades a candidate vector c with gamma_i = sum_j W[i][j] c_j, W being the second raw block
 * of the #MVS_v1.1 tail read row-major (:347-358, :608-611).  Call the first block S.  This library takes the COLUMNS of
 * S to be the selected candidate vectors and W = S^-1: the only reading under which a member of the active set grades
 * exactly e_j with the reference's formula, and one every potential file of this project satisfies.  Whether files
 * written by MLIP-3 itself follow it depends on how MLIP orders the blocks in memory; nothing here
 * depends on that.  A swap puts pool row i into slot j: S[:, j] <- v_i.  With G[n, :] = W v_n and the pivot p = G[i][j],
 * every row r of the stacked matrix [W^T ; G] is updated as r <- r - r[j] u, u = (G[i, :] - e_j) / p, and |det S| grows
 * by the factor |p|.
 */
/* copy of the first raw block S (mtp_potential_get_tables returns the second, W); MTP_ERR_STATE without a selection block */
int mtp_potential_get_active_set(const mtp_potential *pot, double *active_set /*[C*C]*/);
/* Writes a potential file that is src_path with the two raw blocks replaced: the bytes of src_path up to and including
 * the '#' in front of the raw blocks (pair_mtp_extrapolation.cpp:607), then active_set and inverse_active_set, C * C
 * doubles each.  Host only; written under a temporary name beside dst_path and renamed.  MTP_ERR_SELECTION for a source
 * without an #MVS tail, MTP_ERR_ARG for a coeff_count that is not the file's, otherwise the parser's codes. */
int mtp_potential_write_selection(const char *src_path, const char *dst_path, const double *active_set,
                                  const double *inverse_active_set, int coeff_count, char *err, int errlen);
/* The per-atom candidate vectors dE_i/dtheta of the grade calls on the installed list (what
 * PairMTPExtrapolation::compute accumulates per atom, :97-98, 240-252): row ii belongs to list row ii, *ld doubles apart,
 * the first C of them used.  *nrows counts the rows from 0 that the grade calls on this list have covered without a gap:
 * a call over a row range that starts above them (mtp_compute_device_rows) does not extend it.  The storage is the
 * context's own: valid until the next list is installed.  MTP_ERR_STATE before a grade call that covers row 0. */
int mtp_context_candidates_device(const mtp_context *ctx, const double **d_rows, int *nrows, int *ld);
/* Per-configuration candidate vectors after a grade call over nrows = cfg_first[ncfg] rows (arguments as for
 * mtp_batch_cfg_grades): the sums of the rows of each configuration divided by its atom count, so that a row's grade is
 * the configuration grade mtp_batch_cfg_grades reports (:369-376); an empty configuration is a zero row.  The storage is
 * the context's own, shared with mtp_batch_cfg_grades: valid until the next call of either.  NULL stream = the context's. */
int mtp_batch_cfg_candidates(mtp_context *ctx, void *stream, int ncfg, const int *d_cfg_first, int nrows,
                             const double **d_rows, int *ld);
/* MaxVol over a pool of nrows candidate vectors d_rows[nrows][ld] (device, the first C of each row used), starting from
 * the context's S and W (the potential's until an install): while some |G[i][j]| exceeds `threshold`, the largest one (ties to the smaller n * C + j) is
 * swapped in.  Per swap one pivot kernel and one pass over the (C + nrows) x cpad stacked matrix run on `stream`; the host
 * reads a 16-byte status once per 16 swaps.  Every `refresh` swaps, and always before the call ends, G is recomputed from
 * the pool and the current W: *converged = 1 only when freshly computed grades hold no entry above the threshold, and
 * *max_grade_after is their maximum -- what a later grade call with the new set reports.  The context's own inverse
 * is NOT changed by the call: selection is followed by mtp_context_install_selection, or by a reload of the written file.
 *   active_set, inverse_active_set [C*C]  S' and W' (host); every changed column of S' is a pool row bit for bit
 *   slot_source [C]                      the pool row now in slot j, -1 where the original column was kept
 *   swap_rows, swap_slots, swap_pivots   [max_swaps] the log: swap k put row i into slot j with pivot p
 *   log_volume_gain                      sum log |p| = log |det S'| - log |det S|
 * NULL stream = the context's.  MTP_ERR_STATE without a selection block; MTP_ERR_ARG for threshold < 1, ld < C,
 * max_swaps < 0, refresh < 1 (nothing launched), and for a non-finite candidate: the outputs then describe the state
 * before the offending pivot.  nrows == 0 is valid: zero swaps, outputs equal to the context's blocks bit for bit.
 * Reaching max_swaps is no error: *converged = 0 and the outputs are the state reached.  The device memory of a call
 * ((C + nrows) x cpad doubles and a little more) is the context's and is kept for the next one; MTP_ERR_LIMIT when it
 * cannot be had. */
int mtp_maxvol_select(mtp_context *ctx, void *stream, const double *d_rows, long long nrows, int ld, double threshold,
                      int max_swaps, int refresh, double *active_set /*[C*C] host*/,
                      double *inverse_active_set /*[C*C] host*/, int *slot_source /*[C]*/, int *swap_rows, int *swap_slots,
                      double *swap_pivots /*[max_swaps]*/, int *nswaps, int *converged, double *log_volume_gain,
                      double *max_grade_after);

/* ---- linear refit: design rows of energy, force and virial ---------------------------------------------------------
 *
 * The model is linear in the species coefficients and in moment_coeffs xi: E = sum_i (species[t_i] + sum_a xi_a B_a(i)),
 * and so are the forces and the virial PairMTP::compute returns (pair_mtp.cpp:204-276).  A refit of these Sp + S numbers
 * with the radial coefficients fixed -- MLIP's linear regression, the "retrain" step of the active-learning loop -- needs
 * the design matrix: per configuration one energy row, 3 N force rows and six virial rows over the columns
 * [species (Sp) | moments (S)], the order of the last Sp + S entries of a candidate vector.  The rows are produced in
 * forward mode: per centre atom i and direction d = (neighbour n, component c), dM_k = d m_k(n) / d u_{n,c} for the basics
 * (the expressions of pair_mtp.cpp:163-191), dM[a3] += mult (dM[a0] M[a1] + M[a0] dM[a1]) through the times rows, and
 * G_a(i, n, c) = dM[alpha_moment_mapping[a]].  Nothing here depends on xi or on the species coefficients.
 */
/* Design rows over rows [row_begin, row_begin + row_count) of the INSTALLED list (rows = positions in ilist, as for
 * mtp_compute_device_rows).  All arrays are device arrays of the caller, leading dimension ld >= Sp + S, even.
 *   d_basis  [row_count][ld] or NULL   row ii - row_begin: one-hot on the centre's type, then B_a(i); columns up to ld
 *                                     zero.  Assigned, once per row: the site-energy design rows.
 *   d_force  [3 nowned][ld]            ACCUMULATED (the caller zeroes it, mtp_zero_async): F[3 owner(n) + c][Sp + a] -= G
 *                                     and F[3 i + c][Sp + a] += G, the sign for which F . theta is the force the force
 *                                     calls return after the ghost fold; the species columns are never touched (they
 *                                     are zero).  The own-row term is summed over the centre's directions on chip first;
 *                                     a neighbour that is an image of the centre itself contributes to neither (the two
 *                                     terms cancel exactly).  fp64 atomic adds: sums depend on arrival order in the
 *                                     last bits.
 *   d_owner  [nall] or NULL            owner(j): the owned row a list entry j is an image of (mtp_ghosts_owner_device);
 *                                     NULL = identity.  No array with ghost rows is ever written.
 *   d_virial_atom [row_count][6][ld] or NULL   assigned: the rows for which V . theta is the per-atom virial vatom[i]
 *                                     (xx, yy, zz, xy, xz, yz; sign and symmetrisation of pair_mtp.cpp:257-276); their
 *                                     sum over a configuration is its virial row block (mtp_batch_design_reduce).
 * A scalar whose moment a LATER scalar is mapped to as well has zero force and virial columns: the reference seeds the
 * adjoint by assignment (pair_mtp.cpp:217-218).  One workgroup of four wavefronts per centre atom; the kernel's table is
 * built and uploaded by the first call on a context.  MTP_ERR_STATE before a list is installed; MTP_ERR_ARG for ld < Sp + S,
 * an odd ld, a row range outside the list, nowned < 0 or a NULL d_force with row_count > 0; MTP_ERR_LIMIT when the
 * workgroup's LDS image does not fit (mtp_last_error names the quantity).  Reported by the next mtp_synchronize: an atom
 * type outside the potential (MTP_ERR_SPECIES), a row with more in-cutoff neighbours than the list's max_numneigh
 * (MTP_ERR_LIMIT), a centre or an owner outside [0, nowned) or a list entry outside [0, nall) (MTP_ERR_ARG; such terms
 * are skipped, never written).  A centre that is refused this way is skipped as a whole: its d_basis and d_virial_atom
 * rows are NOT assigned and keep what the caller's buffers held, and after any of these errors no output of the call may
 * be used. */
int mtp_design_rows_device(mtp_context *ctx, void *stream, const double *d_x, const int *d_type, int row_begin,
                           int row_count, const int *d_owner, int ld, double *d_basis, double *d_force, int nowned,
                           double *d_virial_atom);
/* The owner map of the last build on a ghost handle, for all rows: identity on the owned rows, the owner behind them
 * (*nall entries).  The handle keeps the owners of its ghosts only; the full map is completed by one small launch on
 * `stream` into storage of the handle and is valid until the next build. */
int mtp_ghosts_owner_device(mtp_ghosts *g, void *stream, const int **d_owner, int *nall);
/* Per-configuration design rows from the per-atom ones: d_energy[k][0, ld) = sum of d_basis over rows [cfg_first[k],
 * cfg_first[k + 1]), d_virial[k][6][ld] the same of d_virial_atom (either pair may be NULL).  One workgroup per
 * configuration and row kind, columns over the lanes, rows added in order without atomics: a configuration's rows do not
 * depend on the rest of the batch; an empty one gets zeros.  d_cfg_first [ncfg + 1] is a device array. */
int mtp_batch_design_reduce(void *stream, int ncfg, const int *d_cfg_first, int ld, const double *d_basis,
                            const double *d_virial_atom, double *d_energy, double *d_virial);
/* The tangent kernel's table as the host builds it from the native schedule (host only, for inspection): counts[4] =
 * {rows (padded), level blocks, A, B}; rows [counts[0]][4] = {a0, a1, mult, a3} in dependency-level order, the leaf
 * block last, over an image with a slot for every moment; level_offset [counts[1] + 1]; scalar_map / force_map [S]
 * (force_map: -1 where a later scalar is mapped to the same moment); basic_pack [B] = slot | a << 8 | b << 12 | c << 16 |
 * mu << 20.  Any pointer may be NULL. */
int mtp_potential_design_table(const mtp_potential *pot, int32_t *counts, int32_t *rows, int32_t *level_offset,
                               int32_t *scalar_map, int32_t *force_map, int32_t *basic_pack);
/* Writes src_path with new linear coefficients to dst_path (host only; temporary file beside dst_path, then rename): the
 * species_coeffs line (kept when species_coeffs == NULL) and the moment_coeffs line are replaced, numbers with 17
 * significant digits; every other byte in front of the selection tail is kept.  The radial block of a candidate vector
 * depends on moment_coeffs, so an #MVS tail of the source no longer describes the new potential: the written file ENDS
 * BEFORE THE TAIL and the call returns MTP_WROTE_WITHOUT_SELECTION (> 0) instead of MTP_OK.  The written file is read
 * back before the rename: the reference sizes its reader's line buffer from the table (T * 32 + 20 characters), and where
 * a coefficient line does not come back bit for bit the call fails with MTP_ERR_LIMIT and writes nothing.  MTP_ERR_ARG
 * for counts that are not the file's (species_count is not looked at when species_coeffs == NULL) and for non-finite
 * coefficients, otherwise the parser's codes. */
#define MTP_WROTE_WITHOUT_SELECTION 1
int mtp_potential_write_coeffs(const char *src_path, const char *dst_path, const double *species_coeffs /*[Sp] or NULL*/,
                               const double *moment_coeffs /*[S]*/, int species_count, int scalar_count, char *err,
                               int errlen);

/* ---- linear refit without the design matrix: double-double normal equations ----------------------------------------
 *
 * The state (opaque handle mtp_normal) holds, per kind of row (0 energy, 1 force, 2 virial), the augmented Gram matrix
 * G = B^T B of n = ncols + 1 columns as two [n][n] fp64 planes hi and lo -- the entry is the unevaluated sum hi + lo, about
 * 106 bits (csrc/mtp_dd.hpp) -- and the number of rows that entered.  Column ncols of B is the target.  For a call with
 * rows [nrows][ld], scale [nrows] and target [nrows]
 *     b[i][c] = fl(scale[i] * rows[i][c]) for c < ncols,   b[i][ncols] = fl(scale[i] * target[i])
 * (ONE fp64 multiply), and sum_i b[i][j] b[i][k] is added to entry (j, k).  A row with scale[i] == 0 is skipped by a test
 * on scale (it may hold NaN) and is not counted; columns [ncols, ld) of rows are never read.  Neither the weights of a fit
 * nor its starting coefficients enter a state, so it can be kept between rounds and extended by new rows only.
 *
 * Sum order: rows are taken in slices of a compile-time length (mtp_normal_sizes), every slice is summed in row order in
 * registers and the slices are added to the state in slice order.  Both triangles are written from one value, so entry
 * (j, k) equals entry (k, j) bit for bit, and the result is the same on any device, for any workspace size and however a
 * row range is split into calls at multiples of the slice length.  No atomics; fp64 VALU arithmetic only. */
typedef struct mtp_normal mtp_normal;
/* tile edge of the kernel, rows of an LDS panel, rows of a slice and the fixed cap of a state's workspace in bytes (any
 * pointer may be NULL); host only */
int mtp_normal_sizes(int *tile, int *panel, int *slice, long long *workspace_cap_bytes);
/* A zeroed state for ncols columns on a device, with its workspace of partial tiles: workspace_bytes (0: the cap) is
 * rounded down to whole rounds of slices -- at least one slice, at most the cap and 256 slices.  A call with more slices
 * than the workspace holds runs several rounds; the result does not depend on that.  Nothing is allocated after this. */
int mtp_normal_create(int device, int ncols, long long workspace_bytes, mtp_normal **out);
void mtp_normal_destroy(mtp_normal *h);
const char *mtp_normal_last_error(const mtp_normal *h);
/* ncols, the slices one round holds, the workspace's and the state's device bytes (any pointer may be NULL) */
int mtp_normal_info(const mtp_normal *h, int *ncols, int *round_slices, long long *workspace_bytes, long long *state_bytes);
/* fewer slices a round than the workspace holds (a diagnostic: the result must not change); MTP_ERR_ARG for more */
int mtp_normal_set_round_slices(mtp_normal *h, int slices);
/* zeroes the three matrices and the row counts, one launch */
int mtp_normal_clear(mtp_normal *h, void *stream);
/* Adds the rows of one kind.  Device arrays of the caller; nothing waits on the host.  MTP_ERR_ARG (the state is left as
 * it was) for a NULL stream, ld < ncols, a kind outside 0..2, nrows < 0 or a NULL array with nrows > 0; nrows == 0
 * launches nothing. */
int mtp_normal_accumulate(mtp_normal *h, void *stream, int kind, long long nrows, int ld, const double *d_rows,
                          const double *d_scale, const double *d_target);
/* Host copies: hi and lo are [3][n][n] (kind, row, column), counts [3].  Both synchronise on `stream`; get: any pointer may
 * be NULL. */
int mtp_normal_get(mtp_normal *h, void *stream, double *hi, double *lo, long long counts[3]);
int mtp_normal_set(mtp_normal *h, void *stream, const double *hi, const double *lo, const long long counts[3]);
/* The solve's first half (HOST ONLY, no device): G = sum_k weights[k] G_k in double-double (hi[k] / lo[k] [n][n]; a kind
 * with weight 0 or hi[k] == NULL is left out), then a Cholesky factorisation with diagonal pivoting over the first
 * ncols = n - 1 columns, the target column riding along.  The pivot of a step is the remaining column with the largest
 * (remaining diagonal) / (original diagonal); the factorisation stops when that ratio is <= drop, and a column with a zero
 * diagonal is dropped at once.  Outputs, rounded to fp64 at the end:
 *   R [ncols][ncols]     rows [0, *rank): the factor in the ORIGINAL column order, zero where a column was eliminated
 *                        by an earlier row (R^T R = G on the kept part; R has the singular values of the weighted matrix)
 *   q [ncols]            entries [0, *rank): Q^T y - R theta0, formed in double-double
 *   pivot_order [ncols]  entries [0, *rank): the column each row eliminated
 *   dropped [ncols]      entries [0, *ndropped): the columns left out, *rank + *ndropped = ncols
 *   pivot_ratios [ncols] the ratio of every kept pivot, then that of every dropped column in the order of `dropped`
 * (pivot_order, dropped, ndropped and pivot_ratios may be NULL).  lstsq(R, q) is the change of the coefficients that
 * lstsq(A_w, y_w - A_w theta0) gives.  MTP_ERR_ARG for non-finite input, a negative weight, no kind with a positive
 * weight or a diagonal entry below zero; MTP_ERR_LIMIT when the host is out of memory. */
int mtp_normal_factor(int n, const double *const hi[3], const double *const lo[3], const double weights[3], const double *theta0,
                      double drop, double *R, double *q, int *rank, int *pivot_order, int *dropped, int *ndropped,
                      double *pivot_ratios);
/* y^T y - 2 theta^T g + theta^T G theta of ONE kind, evaluated in double-double and clamped at 0: the sum of squared
 * (scaled) residuals at theta (host only).  MTP_ERR_ARG for non-finite input. */
int mtp_normal_quadratic(int n, const double *hi, const double *lo, const double *theta, double *out);

/* ---- training gradient: loss derivatives for ALL coefficients -------------------------------------------------------
 *
 * theta [C] holds every coefficient in candidate-vector order: radial [Sp][Sp][Mu][R] | species [Sp] | moments [S],
 * C = Sp^2 Mu R + Sp + S.  It is a device vector of the caller's and is read by every call: a trainer steps theta without
 * reloading a potential, and the context's force tables keep their coefficients until mtp_context_install_coeffs.  The model is not linear in the
 * radial block, so the gradient is produced in reverse: for cotangents ebar (per atom), fbar (per owned atom) and vbar
 * (per atom, six components)
 *     grad = d/dtheta [ sum_i ebar_i eatom_i + sum_j fbar_j . F_j + sum_i vbar_i . vatom_i ],   F the folded force,
 * which, summed over centre atoms, is the derivative of each centre's candidate vector along ONE displacement field
 * du_n = fbar_owner(i) - fbar_owner(n) - Vs u_n (Vs: the symmetric matrix of vbar_i with halved off-diagonals) plus ebar_i
 * times the candidate vector itself.  One workgroup of four wavefronts per centre atom; the structural
 * table is built and uploaded by the first training call on a context.
 *
 * Tables the formulas do not cover are refused with MTP_ERR_UNSUPPORTED before anything is launched (mtp_last_error names
 * the row or the scalar): a row of alpha_index_times that reads a moment which the same or a later row still adds to, and
 * two scalars mapped to one moment.  For both the reference's forces are not the gradient of its energy.
 *
 * Arguments, the NULL-stream rule and the deferred reports are those of mtp_design_rows_device: MTP_ERR_STATE before a
 * list is installed; MTP_ERR_ARG for a row range outside the list, nowned < 0, a missing required array, and in vjp mode
 * ld < C or an odd ld; MTP_ERR_LIMIT when the workgroup's LDS image (four moment images, the tile tables, the list's
 * longest row) exceeds 160 KB.  Reported by the next mtp_synchronize: an atom type outside the potential, a row longer
 * than max_numneigh, a centre or an owner outside [0, nowned) or a list entry outside [0, nall); a refused centre is
 * skipped as a whole and its rows are not assigned. */
/* value: d_eatom [row_count] and d_vatom [row_count][6] (either may be NULL) are ASSIGNED per row ii - row_begin; d_force
 * [nowned][3] is ACCUMULATED straight onto owner rows with fp64 atomic adds (the caller zeroes it): +t on the centre, -t on
 * owner(n).  Semantics, signs and cutoff test are those of PairMTP::compute (pair_mtp.cpp:196-276). */
int mtp_train_value_device(mtp_context *ctx, void *stream, const double *d_x, const int *d_type, int row_begin,
                           int row_count, const int *d_owner, const double *d_theta, double *d_eatom, double *d_force,
                           int nowned, double *d_vatom);
/* vjp: d_ebar [row_count], d_fbar [nowned][3], d_vbar [row_count][6] -- any of them may be NULL, meaning zero.
 * d_grad_rows [row_count][ld] is ASSIGNED, columns [C, ld) zero; no atomics to global memory.  Per-configuration sums of
 * the rows: mtp_batch_design_reduce (d_basis = d_grad_rows). */
int mtp_train_vjp_device(mtp_context *ctx, void *stream, const double *d_x, const int *d_type, int row_begin, int row_count,
                         const int *d_owner, const double *d_theta, const double *d_ebar, const double *d_fbar, int nowned,
                         const double *d_vbar, int ld, double *d_grad_rows);
/* The training kernel's structural table (host only, for inspection): counts[6] = {rows (padded), level blocks, A, B, Mu,
 * C}; the rows, level offsets, scalar map and basic descriptors are those of mtp_potential_design_table; bymu [B]: the
 * basics ordered by mu, mufirst [Mu + 1] its offsets; refused[2] = {first row of alpha_index_times, in file order, that
 * reads a moment which the same or a later row still adds to, first scalar mapped to a moment an earlier scalar is mapped
 * to as well}, -1 for none.  Returns MTP_ERR_UNSUPPORTED and a message in err when either is set.  Any pointer may be
 * NULL. */
int mtp_potential_train_table(const mtp_potential *pot, int32_t *counts, int32_t *bymu, int32_t *mufirst, int32_t *refused,
                              char *err, int errlen);
/* mtp_potential_write_coeffs with the radial block as well: the lines between the radial_coeffs line and the
 * alpha_moments_count line are replaced by every t1-t2 pair in row-major order, Mu brace lines of R numbers each, 17
 * significant digits, indented as the source's first pair line and first brace line (radial_coeffs == NULL keeps the
 * block).  The read-back through the text parser must return all three arrays bit for bit, or nothing is written. */
int mtp_potential_write_all_coeffs(const char *src_path, const char *dst_path, const double *radial_coeffs /*[Sp^2 Mu R] or NULL*/,
                                   const double *species_coeffs /*[Sp] or NULL*/, const double *moment_coeffs /*[S]*/,
                                   int radial_count, int species_count, int scalar_count, char *err, int errlen);

/* ---- installing new coefficients and a new active set into a LIVE context ------------------------------------------
 *
 * The native schedule of a potential (dependency levels, LDS numbering, gather programs, head x tail blocks) is a
 * function of its alpha tables only; the coefficient values enter a context through a handful of small device arrays
 * (DESIGN.md 5.3.3).  A context keeps its own host copy of {radial, species, moment coefficients, S, W}, initialised from
 * the potential it was created on, and from then on that copy is the only source of values for what the context does; the
 * potential itself is const, may be shared by several contexts and is never written.  An install rewrites every device
 * copy of the values and nothing else: no re-plan, no allocation of launch state, the same kernels afterwards.
 *
 * All arguments of an install are validated before the first byte is written: a refused install leaves the context
 * exactly as it was.  The ordering contract of an install (after earlier work on `stream`, one wait, the caller's arrays
 * free on return, no launch of the context in flight on another stream) stands in the Streams paragraph at the top.
 *
 * A coefficient change makes the columns of the installed active set stale (candidate vectors depend on the
 * coefficients); rebuilding the set is the caller's selection step, not something an install does.
 */
/* The coefficient-dependent tables of the native schedule for a (radial, species, moment) triple on the FIXED structure of
 * `pot` (host only): arrays in the sizes and order of mtp_potential_write_all_coeffs, NULL = the potential's own values.
 * counts[6] = lengths of radial_out, species_out, seed_val, e_lin, leaf_cf, leaf_cb (seed_val: the last scalar mapped to a
 * stored moment; e_lin: the scalars of stored moments; leaf_cf / leaf_cb: per leaf row mult x the sum of the coefficients
 * mapped to the leaf moment, respectively the last one).  Any output may be NULL.  MTP_ERR_ARG for non-finite input. */
int mtp_potential_coeff_tables(const mtp_potential *pot, const double *radial_coeffs, const double *species_coeffs,
                               const double *moment_coeffs, int32_t *counts /*[6]*/, double *radial_out, double *species_out,
                               double *seed_val, double *e_lin, double *leaf_cf, double *leaf_cb);
/* MTP_OK when the file at `path` (read by the text parser: no schedule is built) equals `pot` in everything the schedule
 * and the kernels' argument block were built from: scaling, both cutoffs, species_count, radial_basis_size,
 * radial_funcs_count, every alpha count and the three alpha tables entry by entry (the parser accepts one radial basis
 * type only) and, with want_selection != 0, coeff_count and the selection mode.  Otherwise MTP_ERR_UNSUPPORTED, err names the
 * first difference; the parser's codes for a file that does not read. */
int mtp_potential_compatible(const mtp_potential *pot, const char *path, int want_selection, char *err, int errlen);
/* New coefficients (HOST arrays; NULL keeps that block): the radial block and the scalar-side tables in the LDS table blob,
 * in place at their recorded offsets, their HBM / L2 copies, the species coefficients and, if a design call has uploaded
 * it, the design kernel's radial block.  MTP_ERR_ARG for non-finite values.  MTP_ERR_UNSUPPORTED when the context was
 * created on values for which every leaf row's energy and adjoint constants are equal -- the blob then holds ONE table for
 * both -- and the new values make them differ (two scalars on one leaf moment whose first coefficient was zero). */
int mtp_context_install_coeffs(mtp_context *ctx, void *stream, const double *radial_coeffs /*[Sp^2 Mu R] or NULL*/,
                               const double *species_coeffs /*[Sp] or NULL*/, const double *moment_coeffs /*[S] or NULL*/);
/* New S and W = S^-1 ([C*C] host arrays, both required): the padded and the MFMA-ordered copy of W on the device, and the
 * context's S, W.  MTP_ERR_STATE when the context's potential was loaded without its selection state, MTP_ERR_ARG for a
 * coeff_count that is not the potential's and for non-finite entries. */
int mtp_context_install_selection(mtp_context *ctx, void *stream, const double *active_set, const double *inverse_active_set,
                                  int coeff_count);
/* The gate of mtp_potential_compatible, then the file's coefficients and -- one wait for both -- the file's selection.  The
 * file is read with the context's selection wish; where the context has a selection state and the file has NO #MVS tail at
 * all (what the coefficient writers leave), the coefficients alone are installed and the context keeps its set.  A tail
 * that is there but does not read (wrong version, a weight line missing, short blocks) is MTP_ERR_SELECTION / MTP_ERR_IO
 * and nothing is installed. */
int mtp_context_install_file(mtp_context *ctx, void *stream, const char *path);
/* the context's current values (host copies; any pointer may be NULL); get_selection: MTP_ERR_STATE without one */
int mtp_context_get_coeffs(const mtp_context *ctx, double *radial_coeffs, double *species_coeffs, double *moment_coeffs);
int mtp_context_get_selection(const mtp_context *ctx, double *active_set, double *inverse_active_set);
/* What the kernels will read, copied back from DEVICE memory (ordered on `stream`, waited for).  counts[10] = doubles of
 * {radial, seed_val, e_lin, leaf_cf, leaf_cb, species, design radial, ainv_pad, ainv_tiled, scalars_in_lds}: the radial
 * block and the four scalar-side tables as they stand in the blob (blob_seed_val / blob_e_lin: only when scalars_in_lds,
 * else nothing is written), the same four from the separate HBM copies, d_species, the design kernel's radial block (count
 * 0 before the first design call) and the two copies of W (0 without a selection state).  With every output NULL the call
 * only fills counts. */
int mtp_context_coeff_tables_device(mtp_context *ctx, void *stream, int32_t *counts /*[10]*/, double *blob_radial,
                                    double *blob_seed_val, double *blob_e_lin, double *blob_leaf_cf, double *blob_leaf_cb,
                                    double *hbm_seed_val, double *hbm_e_lin, double *hbm_leaf_cf, double *hbm_leaf_cb,
                                    double *species, double *design_radial, double *ainv_pad, double *ainv_tiled);
/* mtp_cfg_grade on the context's W */
int mtp_context_cfg_grade(const mtp_context *ctx, const double *coeff_ders, double *grade);

#ifdef __cplusplus
}
#endif
#endif
