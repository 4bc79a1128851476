"""ctypes binding of libmtp_mi355x.so (include/mtp_mi355x.h) for tests, bench and the
multi-GPU driver.  There is no fallback: a missing library or a missing gfx950 device
raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTP_LIB", os.path.join(_HERE, "libmtp_mi355x.so"))   # MTP_LIB: diagnostic builds

MTP_OK = 0
ERR_NAMES = {-2: "IO", -3: "EOF", -4: "FORMAT", -5: "PARSE", -6: "UNSUPPORTED", -7: "TABLE",
             -8: "SELECTION", -9: "MODE", -20: "ARG", -21: "DEVICE", -22: "SPECIES", -23: "STATE",
             -24: "LIMIT"}
VARIANT_AUTO, VARIANT_LARGE, VARIANT_SMALL = 0, 1, 2

EXPORTS = [
    "mtp_potential_load", "mtp_potential_free", "mtp_potential_get_info", "mtp_potential_get_tables",
    "mtp_context_create", "mtp_context_destroy", "mtp_last_error", "mtp_context_set_variant",
    "mtp_set_neighbors", "mtp_set_neighbors_csr", "mtp_set_neighbors_device", "mtp_compute",
    "mtp_compute_device", "mtp_synchronize", "mtp_cfg_grade", "mtp_context_launch_info",
    "mtp_context_set_timing", "mtp_context_last_kernel_ms", "mtp_build_neighbors_device",
    "mtp_copy_neighbors_to_host", "mtp_compute_device_rows", "mtp_context_plan_info",
    "mtp_halo_get_unique_id", "mtp_halo_create", "mtp_halo_destroy", "mtp_halo_last_error", "mtp_halo_comm_count",
    "mtp_halo_forward_begin", "mtp_halo_forward_end", "mtp_halo_forward", "mtp_halo_reverse_begin",
    "mtp_halo_reverse_end", "mtp_halo_reverse", "mtp_halo_allreduce", "mtp_halo_force_step", "mtp_halo_set_overlap",
    "mtp_halo_get_overlap", "mtp_halo_layout", "mtp_halo_pack_forward", "mtp_halo_unpack_reverse", "mtp_halo_get_layout",
    "mtp_halo_local_exchange", "mtp_set_neighbors_device_2d", "mtp_build_flags", "mtp_compute_resident",
    "mtp_resident_totals", "mtp_resident_peratom_device", "mtp_resident_peratom_host", "mtp_copy_to_host",
    "mtp_ghosts_create", "mtp_ghosts_destroy", "mtp_ghosts_last_error", "mtp_ghosts_build", "mtp_ghosts_forward",
    "mtp_ghosts_reverse", "mtp_ghosts_reverse_finish", "mtp_ghosts_types", "mtp_nve_initial", "mtp_nve_final", "mtp_nve_monitor",
    "mtp_context_set_deterministic", "mtp_zero_async", "mtp_potential_kernel_shape", "mtp_context_layout_mode",
    "mtp_ghosts_build_cell", "mtp_ghosts_cell_bounds",
    "mtp_plan_fixed_fields", "mtp_plan_fixed_shape", "mtp_context_last_shape", "mtp_potential_moment_blocks",
    "mtp_batch_layout", "mtp_ghosts_build_batch", "mtp_batch_reduce", "mtp_batch_cfg_grades",
    "mtp_potential_get_active_set", "mtp_potential_write_selection", "mtp_context_candidates_device",
    "mtp_batch_cfg_candidates", "mtp_maxvol_select",
    "mtp_design_rows_device", "mtp_ghosts_owner_device", "mtp_batch_design_reduce", "mtp_potential_design_table",
    "mtp_potential_write_coeffs",
    "mtp_train_value_device", "mtp_train_vjp_device", "mtp_potential_train_table", "mtp_potential_write_all_coeffs",
    "mtp_potential_coeff_tables", "mtp_potential_compatible", "mtp_context_install_coeffs", "mtp_context_install_selection",
    "mtp_context_install_file", "mtp_context_get_coeffs", "mtp_context_get_selection", "mtp_context_coeff_tables_device",
    "mtp_context_cfg_grade",
    "mtp_sample_row_map", "mtp_sample_initial", "mtp_sample_final", "mtp_sample_monitor", "mtp_sample_capture",
    "mtp_sample_to_cell", "mtp_relax_step",
    "mtp_relax_cell_step", "mtp_relax_cell_rebase", "mtp_relax_cell_capture_cells", "mtp_ghosts_deform",
    "mtp_sample_cell_step", "mtp_neb_step", "mtp_hess_step", "mtp_hess_finish",
    "mtp_elastic_step", "mtp_elastic_finish", "mtp_elastic_relax", "mtp_eigh_batched",
    "mtp_normal_sizes", "mtp_normal_create", "mtp_normal_destroy", "mtp_normal_last_error", "mtp_normal_info",
    "mtp_normal_set_round_slices", "mtp_normal_clear", "mtp_normal_accumulate", "mtp_normal_get", "mtp_normal_set",
    "mtp_normal_factor", "mtp_normal_quadratic",
]
WROTE_WITHOUT_SELECTION = 1   # mtp_potential_write_coeffs: the source's #MVS tail was left out
# mtp_batch_reduce: segments of up to BATCH_WAVE_ROWS rows are reduced by one wavefront (64 lanes), longer ones by a
# workgroup of BATCH_BLOCK threads; the grade kernel behind mtp_batch_cfg_grades takes GRADE_ROWS_PER_BLOCK rows a workgroup
BATCH_WAVE_LANES, BATCH_WAVE_ROWS, BATCH_BLOCK, GRADE_ROWS_PER_BLOCK = 64, 256, 256, 128
BATCH_MAX_COORD, BATCH_MAX_CELLS = 2048.0, 2 ** 26
HALO_ID_BYTES = 128
REDUCE_SUM, REDUCE_MAX = 0, 1


class MtpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmtp_mi355x: %s (%d): %s" % (ERR_NAMES.get(code, "?"), code, msg))
        self.code = code


class PotentialInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "species_count", "radial_basis_size", "radial_func_count", "alpha_moment_count",
        "alpha_index_basic_count", "alpha_index_times_count", "alpha_scalar_count",
        "max_alpha_index_basic", "coeff_count", "has_selection", "configuration_mode",
        "product_levels")] + [("scaling", C.c_double), ("min_cutoff", C.c_double), ("max_cutoff", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        # torch bundles its own libamdhip64.so.7; importing it first makes this library bind to
        # that same HIP runtime (one runtime per process) instead of loading /opt/rocm's beside it
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for n in EXPORTS:
            getattr(L, n)           # AttributeError if the ABI drifted
        for n in EXPORTS:
            getattr(L, n).restype = C.c_int
        L.mtp_last_error.restype = C.c_char_p
        L.mtp_build_flags.restype = C.c_char_p
        L.mtp_halo_last_error.restype = C.c_char_p
        L.mtp_ghosts_last_error.restype = C.c_char_p
        L.mtp_normal_last_error.restype = C.c_char_p
        L.mtp_normal_destroy.restype = None
        L.mtp_ghosts_destroy.restype = None
        L.mtp_potential_free.restype = None
        L.mtp_context_destroy.restype = None
        L.mtp_halo_destroy.restype = None
        _lib = L
    return _lib


def kernel_source_hash():
    """sha256 over the sources of the force / grade kernels, their planner and the table builder: ties committed
    rocprofv3 counters to the build they came from.  The neighbour-list, halo and integrator kernels are other launches
    (their sources do not enter the counted kernels) and are left out, so that work on them does not orphan the counters."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(_HERE, "csrc")
    other_launches = ("mtp_neighbor_kernels.hip", "mtp_halo.hip", "mtp_md.hip", "mtp_sample.hip", "mtp_relax.hip",
                      "mtp_relax_cell.hip", "mtp_batch_step.hpp", "mtp_sample_cell.hip", "mtp_philox.hpp", "mtp_neb.hip",
                      "mtp_hess.hip", "mtp_elastic.hip", "mtp_eigh.hip")
    for n in sorted(os.listdir(src)):
        if n.endswith((".hip", ".hpp", ".cpp")) and n not in other_launches:
            h.update(n.encode())
            h.update(open(os.path.join(src, n), "rb").read())
    return h.hexdigest()


def build_flags():
    """compile-time switches of the loaded library that differ from the shipped defaults ("" for a release build)"""
    return lib().mtp_build_flags().decode()


def halo_layout(plan):
    """(send_off, recv_off) as the C side derives them from a plan's counts (host only: mtp_halo_layout)."""
    idx = np.ascontiguousarray(plan.send_idx, np.int32)
    sc = np.ascontiguousarray(plan.send_counts, np.int32)
    rc_ = np.ascontiguousarray(plan.recv_counts, np.int32)
    so = np.zeros(plan.nranks + 1, np.int32)
    ro = np.zeros(plan.nranks + 1, np.int32)
    err = C.create_string_buffer(512)
    rc = lib().mtp_halo_layout(int(plan.nranks), int(plan.nlocal), int(plan.nghost), _np(idx, C.c_int), _np(sc, C.c_int),
                               _np(rc_, C.c_int), _np(so, C.c_int), _np(ro, C.c_int), err, 512)
    if rc:
        raise MtpError(rc, err.value.decode())
    return so, ro


def use_private_torch_stream(device):
    """PyTorch's default stream is the legacy null stream (handle 0), and a null handle asks this library for the
    context's own NON-BLOCKING stream -- torch work and the library's kernels would then not be ordered with respect
    to each other.  Drivers that mix both call this once: it makes a real stream current for torch and returns its
    handle for the library's `stream` arguments (collectives issued from torch follow the current stream too)."""
    import torch
    s = torch.cuda.Stream(device=device)
    torch.cuda.set_stream(s)
    return s


def _np(a, ty):
    return None if a is None else a.ctypes.data_as(C.POINTER(ty))


def _ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


class Potential:
    def __init__(self, path, selection=False):
        self.h = C.c_void_p()
        self.path = os.fspath(path)
        err = C.create_string_buffer(512)
        rc = lib().mtp_potential_load(os.fsencode(path), int(selection), C.byref(self.h), err, 512)
        if rc:
            raise MtpError(rc, err.value.decode())
        self.info = PotentialInfo()
        lib().mtp_potential_get_info(self.h, C.byref(self.info))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.mtp_potential_free(self.h)
            self.h = None

    @property
    def sizes(self):
        i = self.info
        return dict(Sp=i.species_count, R=i.radial_basis_size, Mu=i.radial_func_count, A=i.alpha_moment_count,
                    B=i.alpha_index_basic_count, T=i.alpha_index_times_count, S=i.alpha_scalar_count,
                    P=i.max_alpha_index_basic, C=i.coeff_count, levels=i.product_levels)

    def tables(self):
        """copies of the parsed tables (mtp_potential_get_tables) and, since the linear refit, three scalars of get_info
        beside them -- scaling, min_cutoff, max_cutoff -- so that the dict is all driver.design_twin needs"""
        i = self.info
        out = dict(
            alpha_index_basic=np.zeros((i.alpha_index_basic_count, 4), np.int32),
            alpha_index_times=np.zeros((i.alpha_index_times_count, 4), np.int32),
            alpha_moment_mapping=np.zeros(i.alpha_scalar_count, np.int32),
            radial_coeffs=np.zeros(i.species_count ** 2 * i.radial_func_count * i.radial_basis_size),
            species_coeffs=np.zeros(i.species_count), moment_coeffs=np.zeros(i.alpha_scalar_count))
        inv = np.zeros((i.coeff_count, i.coeff_count)) if i.has_selection else None
        rc = lib().mtp_potential_get_tables(
            self.h, _np(out["alpha_index_basic"], C.c_int32), _np(out["alpha_index_times"], C.c_int32),
            _np(out["alpha_moment_mapping"], C.c_int32), _np(out["radial_coeffs"], C.c_double),
            _np(out["species_coeffs"], C.c_double), _np(out["moment_coeffs"], C.c_double), _np(inv, C.c_double))
        if rc:
            raise MtpError(rc, "get_tables")
        if inv is not None:
            out["inverse_active_set"] = inv
        out.update(scaling=float(i.scaling), min_cutoff=float(i.min_cutoff), max_cutoff=float(i.max_cutoff))
        return out

    def active_set(self):
        """the first raw block S of the selection state, [C, C]: its columns are the selected candidate vectors and the
        second block (tables()["inverse_active_set"]) is its inverse (mtp_potential_get_active_set)"""
        C_ = self.info.coeff_count
        S = np.zeros((C_, C_))
        rc = lib().mtp_potential_get_active_set(self.h, _np(S, C.c_double))
        if rc:
            raise MtpError(rc, "get_active_set: the potential carries no selection state")
        return S

    def design_table(self):
        """the tangent (design-row) kernel's own table as the host builds it (mtp_potential_design_table): dict(rows
        [n, 4] = {a0, a1, mult, a3} in dependency-level order over an image with a slot for every moment, level_offset,
        scalar_map, force_map [S], basic_pack [B], A, B)"""
        cnt = np.zeros(4, np.int32)
        rc = lib().mtp_potential_design_table(self.h, _np(cnt, C.c_int32), None, None, None, None, None)
        if rc:
            raise MtpError(rc, "design_table")
        S = self.info.alpha_scalar_count
        out = dict(rows=np.zeros((int(cnt[0]), 4), np.int32), level_offset=np.zeros(int(cnt[1]) + 1, np.int32),
                   scalar_map=np.zeros(S, np.int32), force_map=np.zeros(S, np.int32), basic_pack=np.zeros(int(cnt[3]), np.int32))
        rc = lib().mtp_potential_design_table(self.h, None, _np(out["rows"], C.c_int32), _np(out["level_offset"], C.c_int32),
                                              _np(out["scalar_map"], C.c_int32), _np(out["force_map"], C.c_int32),
                                              _np(out["basic_pack"], C.c_int32))
        if rc:
            raise MtpError(rc, "design_table")
        out.update(A=int(cnt[2]), B=int(cnt[3]))
        return out

    def train_table(self):
        """the training kernel's structural table as the host builds it (mtp_potential_train_table): dict(rows (padded),
        levels, A, B, Mu, C, bymu [B], mufirst [Mu + 1], late_row, dup_scalar (-1: none), supported, message).  A table the
        gradient formulas do not cover is reported here (supported = False, message names the row or the scalar) and
        refused by the training calls with MtpError(UNSUPPORTED)."""
        cnt = np.zeros(6, np.int32)
        lib().mtp_potential_train_table(self.h, _np(cnt, C.c_int32), None, None, None, None, 0)
        bymu, mufirst = np.zeros(int(cnt[3]), np.int32), np.zeros(int(cnt[4]) + 1, np.int32)
        refused = np.zeros(2, np.int32)
        err = C.create_string_buffer(512)
        rc = lib().mtp_potential_train_table(self.h, None, _np(bymu, C.c_int32), _np(mufirst, C.c_int32),
                                             _np(refused, C.c_int32), err, 512)
        if rc not in (0, -6):
            raise MtpError(rc, "train_table")
        return dict(rows=int(cnt[0]), levels=int(cnt[1]), A=int(cnt[2]), B=int(cnt[3]), Mu=int(cnt[4]), C=int(cnt[5]),
                    bymu=bymu, mufirst=mufirst, late_row=int(refused[0]), dup_scalar=int(refused[1]), supported=rc == 0,
                    message=err.value.decode())

    def theta(self):
        """the file's coefficients as one [C] vector in candidate-vector order [radial | species | moments]"""
        t = self.tables()
        return np.concatenate([t["radial_coeffs"], t["species_coeffs"], t["moment_coeffs"]])

    def coeff_tables(self, radial_coeffs=None, species_coeffs=None, moment_coeffs=None):
        """the coefficient-dependent tables of the native schedule for the given blocks on this potential's structure (None:
        the file's own values), host only: dict(radial, species, seed_val, e_lin, leaf_cf, leaf_cb) -- what a context
        created on a file with these values uploads (mtp_potential_coeff_tables).  Non-finite input: MtpError(ARG)."""
        i = self.info
        want = (i.species_count ** 2 * i.radial_func_count * i.radial_basis_size, i.species_count, i.alpha_scalar_count)
        arrs = []
        for a, n, name in zip((radial_coeffs, species_coeffs, moment_coeffs), want, ("radial", "species", "moment")):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
            if a is not None and len(a) != n:
                raise MtpError(-20, "coeff_tables: %d %s coefficients given, the potential has %d" % (len(a), name, n))
            arrs.append(a)
        cnt = np.zeros(6, np.int32)
        rc = lib().mtp_potential_coeff_tables(self.h, *[_np(a, C.c_double) for a in arrs], _np(cnt, C.c_int32),
                                              None, None, None, None, None, None)
        if rc:
            raise MtpError(rc, "coeff_tables: a coefficient is not finite")
        names = ("radial", "species", "seed_val", "e_lin", "leaf_cf", "leaf_cb")
        out = {n: np.zeros(int(k)) for n, k in zip(names, cnt)}
        rc = lib().mtp_potential_coeff_tables(self.h, *[_np(a, C.c_double) for a in arrs], None,
                                              *[_np(out[n], C.c_double) for n in names])
        if rc:
            raise MtpError(rc, "coeff_tables")
        return out

    def compatible(self, path, selection=None):
        """None when the file at `path` has this potential's structure -- everything the native schedule and the kernels'
        argument block were built from -- so that a context of this potential can install it; otherwise the message that
        names the first difference (mtp_potential_compatible).  selection (default: as this potential was loaded) also
        compares coeff_count and the selection mode.  A file that does not parse raises."""
        sel = bool(self.info.has_selection) if selection is None else bool(selection)
        err = C.create_string_buffer(512)
        rc = lib().mtp_potential_compatible(self.h, os.fsencode(path), int(sel), err, 512)
        if rc == -6:
            return err.value.decode()
        if rc:
            raise MtpError(rc, err.value.decode())
        return None

    def kernel_shape(self):
        """the force kernel instantiation a context of this potential launches (mtp_potential_kernel_shape)"""
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        rc = lib().mtp_potential_kernel_shape(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        if rc:
            raise MtpError(rc, "%d head x tail blocks: no force kernel instantiation fits" % a.value)
        return dict(fwd_blocks=a.value, block_lanes=b.value, blocks_per_lane=c.value, max_degree=d.value)

    def moment_blocks(self, five=False):
        """the blocks of the basic-moment pass as the kernels read them (mtp_potential_moment_blocks): (blocks [n][8] int32,
        pack [B] int32 = slot | a << 8 | b << 12 | c << 16 | mu << 20 of the basic at each LDS number).  five=False: the
        3 x 3 head x tail blocks, five=True: the five-factor blocks of the fixed-shape kernels"""
        n = lib().mtp_potential_moment_blocks(self.h, int(bool(five)), None, 0, None)
        if n < 0:
            raise MtpError(n, "moment_blocks")
        blocks = np.zeros((n, 8), dtype=np.int32)
        pack = np.zeros(self.sizes["B"], dtype=np.int32)
        rc = lib().mtp_potential_moment_blocks(self.h, int(bool(five)), _np(blocks, C.c_int32), n, _np(pack, C.c_int32))
        if rc != n:
            raise MtpError(rc, "moment_blocks")
        return blocks, pack

    def plan_fixed_fields(self, num_cus, inum, max_numneigh, variant=VARIANT_AUTO, grade=False):
        """the force kernel's template arguments and the fields of its argument block that the table structure and the
        launch plan decide, without a device (mtp_plan_fixed_fields): {name: int, or list of ints}, in the library's order"""
        buf = C.create_string_buffer(8192)
        rc = lib().mtp_plan_fixed_fields(self.h, int(num_cus), int(inum), int(max_numneigh), int(variant), int(bool(grade)),
                                         buf, 8192)
        if rc:
            raise MtpError(rc, "plan_fixed_fields")
        out = {}
        for line in buf.value.decode().splitlines():
            k, v = line.split("=")
            out[k] = [int(x) for x in v.split(",")] if "," in v else int(v)
        return out

    def plan_fixed_shape(self, num_cus, inum, max_numneigh, variant=VARIANT_AUTO, grade=False):
        """name of the fixed-shape kernel such a launch would run, "" for a generic one (no device needed)"""
        buf = C.create_string_buffer(128)
        rc = lib().mtp_plan_fixed_shape(self.h, int(num_cus), int(inum), int(max_numneigh), int(variant), int(bool(grade)),
                                        buf, 128)
        if rc:
            raise MtpError(rc, "plan_fixed_shape")
        return buf.value.decode()

    def cfg_grade(self, coeff_ders):
        g = C.c_double(0)
        c = np.ascontiguousarray(coeff_ders, dtype=np.float64)
        rc = lib().mtp_cfg_grade(self.h, _np(c, C.c_double), C.byref(g))
        if rc:
            raise MtpError(rc, "cfg_grade")
        return g.value


class Context:
    """One GPU context.  Host-array path: set_neighbors + compute.  Device path:
    set_neighbors_device + compute_device with torch tensors."""

    def __init__(self, pot: Potential, device=0):
        self.pot = pot
        self.h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = lib().mtp_context_create(pot.h, int(device), C.byref(self.h), err, 512)
        if rc:
            raise MtpError(rc, err.value.decode())
        self._keep = []

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.mtp_context_destroy(self.h)
            self.h = None

    def _check(self, rc):
        if rc:
            raise MtpError(rc, lib().mtp_last_error(self.h).decode())

    def set_variant(self, v):
        self._check(lib().mtp_context_set_variant(self.h, int(v)))

    def set_neighbors(self, ilist, first, neigh, nall):
        ilist = np.ascontiguousarray(ilist, np.int32)
        first = np.ascontiguousarray(first, np.int32)
        neigh = np.ascontiguousarray(neigh, np.int32)
        self.nall = int(nall)
        self._check(lib().mtp_set_neighbors_csr(self.h, len(ilist), _np(ilist, C.c_int), _np(first, C.c_int),
                                                _np(neigh, C.c_int), int(nall)))

    def set_neighbors_lammps(self, ilist, numneigh, rows, nall):
        """LAMMPS form: numneigh[i], firstneigh[i] indexed by atom id (rows: list of int32 arrays)."""
        ilist = np.ascontiguousarray(ilist, np.int32)
        numneigh = np.ascontiguousarray(numneigh, np.int32)
        rows = [np.ascontiguousarray(r, np.int32) for r in rows]
        arr = (C.POINTER(C.c_int) * len(rows))(*[_np(r, C.c_int) for r in rows])
        self.nall = int(nall)
        self._check(lib().mtp_set_neighbors(self.h, len(ilist), _np(ilist, C.c_int), _np(numneigh, C.c_int), arr,
                                            int(nall)))

    def set_neighbors_device_2d(self, ilist_t, numneigh_t, neighbors_t, stride_i, stride_jj, max_neighs, nall, stream=None):
        """LAMMPS-KOKKOS form: d_ilist(ii), d_numneigh(i), padded 2-D view d_neighbors(i, jj) with the given strides."""
        self._keep = [ilist_t, numneigh_t, neighbors_t]
        self.nall = int(nall)
        self._inum = int(ilist_t.numel())
        self._check(lib().mtp_set_neighbors_device_2d(self.h, C.c_void_p(stream) if stream else None, int(ilist_t.numel()),
                                                      _ptr(ilist_t), _ptr(numneigh_t), _ptr(neighbors_t),
                                                      C.c_longlong(stride_i), C.c_longlong(stride_jj), int(max_neighs),
                                                      int(nall)))

    def set_neighbors_device(self, ilist_t, first_t, neigh_t, nall, max_numneigh):
        self._keep = [ilist_t, first_t, neigh_t]
        self.nall = int(nall)
        self._check(lib().mtp_set_neighbors_device(self.h, int(ilist_t.numel()), _ptr(ilist_t), _ptr(first_t),
                                                   _ptr(neigh_t), int(nall), int(max_numneigh)))

    def compute(self, x, types, eflag=3, vflag=4, grade=False):
        x = np.ascontiguousarray(x, np.float64)
        types = np.ascontiguousarray(types, np.int32)
        nall = x.shape[0]
        assert nall == self.nall
        f = np.zeros((nall, 3))
        eatom = np.zeros(nall)
        vatom = np.zeros((nall, 6))
        virial = np.zeros(6)
        e = C.c_double(0)
        mg = C.c_double(0)
        grades = np.zeros(nall) if grade else None
        cd = np.zeros(self.pot.info.coeff_count) if grade else None
        self._check(lib().mtp_compute(self.h, _np(x, C.c_double), _np(types, C.c_int), int(eflag), int(vflag),
                                      int(bool(grade)), _np(f, C.c_double), _np(eatom, C.c_double),
                                      _np(vatom, C.c_double), C.byref(e), _np(virial, C.c_double),
                                      _np(grades, C.c_double), C.byref(mg), _np(cd, C.c_double)))
        out = dict(energy=e.value, eatom=eatom, f=f, virial=virial, vatom=vatom)
        if grade:
            out.update(grades=grades, max_grade=mg.value, coeff_ders=cd)
        return out

    def build_neighbors_device(self, x_t, inum, nall, list_cutoff, lo, hi, stream=None):
        """Full neighbour list built on the GPU from device-resident positions; returns
        (entries, longest row).  The list stays in the context."""
        lo3 = (C.c_double * 3)(*[float(v) for v in lo])
        hi3 = (C.c_double * 3)(*[float(v) for v in hi])
        total, mx = C.c_longlong(0), C.c_int32(0)
        st = C.c_void_p(stream) if stream else None
        self._check(lib().mtp_build_neighbors_device(self.h, st, _ptr(x_t), int(inum), int(nall), C.c_double(list_cutoff),
                                                     lo3, hi3, None, None, C.byref(total), C.byref(mx)))
        self._inum = int(inum)
        self.nall = int(nall)
        return total.value, mx.value

    def neighbors_to_host(self, inum=None, total=None):
        """(first, neigh) of the list the context owns, as numpy arrays."""
        inum = self._inum if inum is None else inum
        first = np.zeros(inum + 1, dtype=np.int32)
        self._check(lib().mtp_copy_neighbors_to_host(self.h, _np(first, C.c_int32), None))
        neigh = np.zeros(max(int(first[-1]), 1), dtype=np.int32)
        self._check(lib().mtp_copy_neighbors_to_host(self.h, _np(first, C.c_int32), _np(neigh, C.c_int32)))
        return first, neigh[: int(first[-1])]

    def compute_device(self, x_t, type_t, f_t, eflag=0, vflag=0, grade=False, eatom_t=None, vatom_t=None,
                       ev_t=None, grades_t=None, maxg_t=None, coeff_t=None, stream=None):
        st = C.c_void_p(stream) if stream else None
        self._check(lib().mtp_compute_device(self.h, st, _ptr(x_t), _ptr(type_t), int(eflag), int(vflag),
                                             int(bool(grade)), _ptr(f_t), _ptr(eatom_t), _ptr(vatom_t),
                                             _ptr(ev_t), _ptr(grades_t), _ptr(maxg_t), _ptr(coeff_t)))

    def compute_device_rows(self, row_begin, row_count, finish, x_t, type_t, f_t, eflag=0, vflag=0, grade=False,
                            eatom_t=None, vatom_t=None, ev_t=None, grades_t=None, maxg_t=None, coeff_t=None, stream=None):
        """Rows [row_begin, row_begin + row_count) of the installed list; `finish` folds the energy / virial tallies."""
        st = C.c_void_p(stream) if stream else None
        self._check(lib().mtp_compute_device_rows(self.h, st, int(row_begin), int(row_count), int(bool(finish)),
                                                  _ptr(x_t), _ptr(type_t), int(eflag), int(vflag), int(bool(grade)),
                                                  _ptr(f_t), _ptr(eatom_t), _ptr(vatom_t), _ptr(ev_t),
                                                  _ptr(grades_t), _ptr(maxg_t), _ptr(coeff_t)))

    def design_rows(self, row_begin, row_count, x_t, type_t, force_t, nowned, ld, basis_t=None, virial_t=None, owner=None,
                    stream=None):
        """Design rows of rows [row_begin, row_begin + row_count) of the installed list (mtp_design_rows_device): force_t
        [3 nowned, ld] is accumulated into (zero it first), basis_t [row_count, ld] and virial_t [row_count, 6, ld] are
        assigned; `owner` is the device pointer of the owner map (Ghosts.owner) or None for the identity."""
        self._check(lib().mtp_design_rows_device(self.h, C.c_void_p(stream) if stream else None, _ptr(x_t), _ptr(type_t),
                                                 int(row_begin), int(row_count), C.c_void_p(owner) if owner else None, int(ld),
                                                 _ptr(basis_t), _ptr(force_t), int(nowned), _ptr(virial_t)))

    def train_value(self, row_begin, row_count, x_t, type_t, theta_t, force_t, nowned, eatom_t=None, vatom_t=None, owner=None,
                    stream=None):
        """Energies, forces and virials at the coefficients theta_t [C] (device, candidate-vector order) for rows [row_begin,
        row_begin + row_count) of the installed list (mtp_train_value_device): force_t [nowned, 3] is accumulated into (zero
        it first), eatom_t [row_count] and vatom_t [row_count, 6] are assigned; `owner` as for design_rows."""
        self._check(lib().mtp_train_value_device(self.h, C.c_void_p(stream) if stream else None, _ptr(x_t), _ptr(type_t),
                                                 int(row_begin), int(row_count), C.c_void_p(owner) if owner else None,
                                                 _ptr(theta_t), _ptr(eatom_t), _ptr(force_t), int(nowned), _ptr(vatom_t)))

    def train_vjp(self, row_begin, row_count, x_t, type_t, theta_t, grad_t, nowned, ld, ebar_t=None, fbar_t=None, vbar_t=None,
                  owner=None, stream=None):
        """Per-atom rows of the gradient with respect to all C coefficients (mtp_train_vjp_device): grad_t [row_count, ld]
        is assigned, row i = d/dtheta of ebar_i eatom_i + the centre's share of fbar . F and vbar_i . vatom_i; ebar_t
        [row_count], fbar_t [nowned, 3], vbar_t [row_count, 6], None = zero."""
        self._check(lib().mtp_train_vjp_device(self.h, C.c_void_p(stream) if stream else None, _ptr(x_t), _ptr(type_t),
                                               int(row_begin), int(row_count), C.c_void_p(owner) if owner else None,
                                               _ptr(theta_t), _ptr(ebar_t), _ptr(fbar_t), int(nowned), _ptr(vbar_t), int(ld),
                                               _ptr(grad_t)))

    def synchronize(self, stream=None):
        self._check(lib().mtp_synchronize(self.h, C.c_void_p(stream) if stream else None))

    def batch_cfg_grades(self, cfg_first_t, nrows, cfg_grade_t, stream=None):
        """configuration-mode grade of every configuration (rows [cfg_first[k], cfg_first[k + 1]) of the grade call just
        made over `nrows` rows) into cfg_grade_t [ncfg]: mtp_batch_cfg_grades"""
        self._check(lib().mtp_batch_cfg_grades(self.h, C.c_void_p(stream) if stream else None, int(cfg_first_t.numel()) - 1,
                                               _ptr(cfg_first_t), int(nrows), _ptr(cfg_grade_t)))

    def candidates(self):
        """per-atom candidate vectors of the grade calls on the installed list as a torch view [list rows, ld] of the
        context's own storage (the first C columns are used): mtp_context_candidates_device"""
        d, n, ld = C.c_void_p(), C.c_int(), C.c_int()
        rc = lib().mtp_context_candidates_device(self.h, C.byref(d), C.byref(n), C.byref(ld))
        if rc:                                               # (a const context keeps no message of its own)
            raise MtpError(rc, "no candidate vectors: call after a grade call on the installed list")
        return _device_view(d.value, n.value, ld.value)

    def batch_cfg_candidates(self, cfg_first_t, nrows, stream=None):
        """per-configuration candidate vectors (sums over the configuration's rows / its atom count) of the grade call just
        made over `nrows` rows, as a torch view [ncfg, ld] of the context's own storage: mtp_batch_cfg_candidates"""
        d, ld = C.c_void_p(), C.c_int()
        ncfg = int(cfg_first_t.numel()) - 1
        self._check(lib().mtp_batch_cfg_candidates(self.h, C.c_void_p(stream) if stream else None, ncfg, _ptr(cfg_first_t),
                                                   int(nrows), C.byref(d), C.byref(ld)))
        return _device_view(d.value, ncfg, ld.value)

    def maxvol_select(self, rows_t, threshold, max_swaps=None, refresh=64, stream=None):
        """MaxVol over the pool rows_t [N, ld] (fp64 device tensor, rows ld >= C doubles apart, the first C used), starting
        from the context's active set (the potential's until install_selection): mtp_maxvol_select.  max_swaps defaults to 4 C.  Returns dict(active_set,
        inverse_active_set [C, C], slot_source [C], swaps [(row, slot, pivot)], nswaps, converged, log_volume_gain,
        max_grade_after).  A non-finite candidate raises MtpError(ARG) whose .result is that dict for the state before the
        offending pivot."""
        C_ = int(self.pot.info.coeff_count)
        max_swaps = 4 * C_ if max_swaps is None else int(max_swaps)
        n = int(rows_t.shape[0])
        ld = int(rows_t.stride(0)) if n > 0 else max(C_, int(rows_t.shape[1]) if rows_t.dim() > 1 else C_)
        if n > 0 and (rows_t.dim() != 2 or rows_t.stride(1) != 1 or str(rows_t.dtype) != "torch.float64"):
            raise ValueError("maxvol_select: the pool must be an fp64 matrix with contiguous rows")
        if n > 0 and rows_t.shape[1] < C_:
            ld = -1                              # (refused by the library: rows shorter than C)
        S, W = np.zeros((C_, C_)), np.zeros((C_, C_))
        src = np.zeros(C_, np.int32)
        m = max(max_swaps, 1)
        si, sj, sp = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m)
        ns, conv, gain, mg = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
        rc = lib().mtp_maxvol_select(self.h, C.c_void_p(stream) if stream else None, _ptr(rows_t) if n > 0 else None,
                                     C.c_longlong(n), int(ld), C.c_double(threshold), int(max_swaps), int(refresh),
                                     _np(S, C.c_double), _np(W, C.c_double), _np(src, C.c_int), _np(si, C.c_int),
                                     _np(sj, C.c_int), _np(sp, C.c_double), C.byref(ns), C.byref(conv), C.byref(gain),
                                     C.byref(mg))
        k = ns.value
        out = dict(active_set=S, inverse_active_set=W, slot_source=src,
                   swaps=[(int(si[q]), int(sj[q]), float(sp[q])) for q in range(k)], nswaps=k, converged=bool(conv.value),
                   log_volume_gain=gain.value, max_grade_after=mg.value)
        if rc:
            e = MtpError(rc, lib().mtp_last_error(self.h).decode())
            e.result = out
            raise e
        return out

    # ---- installs: new values into this live context (include/mtp_mi355x.h, "installing ...") -------------------------
    # The ordering contract of all three (include/mtp_mi355x.h, "Streams"): an install is ordered after all earlier work on
    # `stream` (None: the context's own non-blocking stream); it returns after that stream has drained (one wait per call);
    # the arrays handed over are free on return; and the caller must have NO launch of this context in flight on ANOTHER
    # stream -- nothing orders such a launch against the in-place copies.  With torch work queued on a stream of the
    # caller's, pass that stream's handle (or synchronise first).
    def _sizes3(self):
        i = self.pot.info
        return (i.species_count ** 2 * i.radial_func_count * i.radial_basis_size, i.species_count, i.alpha_scalar_count)

    def install_coeffs(self, radial_coeffs=None, species_coeffs=None, moment_coeffs=None, stream=None):
        """New coefficients (host arrays in the file's order, any shape; None keeps that block) into every device table the
        kernels read; no re-plan, the same kernels afterwards: mtp_context_install_coeffs.  Ordered after earlier work on
        `stream`, returns after it has drained, the arrays are free on return; no launch of this context may be in flight
        on another stream (the contract above).  All arguments are checked before anything is written: wrong lengths and
        non-finite values raise MtpError(ARG) and leave the context as it was.  The installed active set's columns were
        candidate vectors of the OLD coefficients: rebuilding it is a select_cells call, not part of an install."""
        arrs = []
        for a, n, name in zip((radial_coeffs, species_coeffs, moment_coeffs), self._sizes3(), ("radial", "species", "moment")):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
            if a is not None and len(a) != n:
                raise MtpError(-20, "install_coeffs: %d %s coefficients given, the potential has %d" % (len(a), name, n))
            arrs.append(a)
        self._check(lib().mtp_context_install_coeffs(self.h, C.c_void_p(stream) if stream else None,
                                                     *[_np(a, C.c_double) for a in arrs]))

    def install_selection(self, active_set, inverse_active_set, stream=None):
        """A new active set S and its inverse W ([C, C] host arrays) into the grade kernels' two copies of W and the start of
        the next maxvol_select: mtp_context_install_selection.  Stream ordering as for install_coeffs: after earlier work
        on `stream`, one wait, arrays free on return, no launch of this context in flight on another stream.  MtpError(STATE) when the potential was loaded without its
        selection state, MtpError(ARG) for a wrong size or non-finite entries; the context is then unchanged."""
        S = np.ascontiguousarray(active_set, dtype=np.float64)
        W = np.ascontiguousarray(inverse_active_set, dtype=np.float64)
        C_ = int(self.pot.info.coeff_count)
        n = int(S.shape[0]) if S.ndim == 2 and S.shape[0] == S.shape[1] and W.shape == S.shape else -1
        if n < 0 and self.pot.info.has_selection:
            raise MtpError(-20, "install_selection: active_set and inverse_active_set must be [%d, %d]" % (C_, C_))
        self._check(lib().mtp_context_install_selection(self.h, C.c_void_p(stream) if stream else None, _np(S, C.c_double),
                                                        _np(W, C.c_double), n))

    def install_file(self, path, stream=None):
        """The coefficients of the file at `path` and, if this context has a selection state and the file carries one, its
        active set, with one wait for both: mtp_context_install_file.  Stream ordering as for install_coeffs (no launch of
        this context in flight on another stream).  A file with no #MVS tail at all installs its coefficients only; a tail
        that does not read is the parser's error and nothing is installed.  MtpError(UNSUPPORTED) naming the first difference when the file's structure
        (Potential.compatible) is not this potential's -- such a file needs a new Potential and Context."""
        self._check(lib().mtp_context_install_file(self.h, C.c_void_p(stream) if stream else None, os.fsencode(path)))

    def coeffs(self):
        """the context's current coefficients: dict(radial_coeffs, species_coeffs, moment_coeffs), flat host arrays"""
        out = [np.zeros(n) for n in self._sizes3()]
        self._check(lib().mtp_context_get_coeffs(self.h, *[_np(a, C.c_double) for a in out]))
        return dict(radial_coeffs=out[0], species_coeffs=out[1], moment_coeffs=out[2])

    def theta(self):
        """the context's current coefficients as one [C] vector in candidate-vector order [radial | species | moments]: the
        file's until an install (Potential.theta() stays the file's)"""
        c = self.coeffs()
        return np.concatenate([c["radial_coeffs"], c["species_coeffs"], c["moment_coeffs"]])

    def selection(self):
        """the context's current (active_set S, inverse_active_set W), [C, C] each: mtp_context_get_selection"""
        C_ = int(self.pot.info.coeff_count)
        S, W = np.zeros((C_, C_)), np.zeros((C_, C_))
        rc = lib().mtp_context_get_selection(self.h, _np(S, C.c_double), _np(W, C.c_double))
        if rc:
            raise MtpError(rc, "selection: the potential was loaded without its selection state")
        return S, W

    def cfg_grade(self, coeff_ders):
        """configuration-mode grade max_i |sum_j W[i][j] c_j| on the context's W: mtp_context_cfg_grade"""
        g = C.c_double(0)
        c = np.ascontiguousarray(coeff_ders, dtype=np.float64)
        rc = lib().mtp_context_cfg_grade(self.h, _np(c, C.c_double), C.byref(g))
        if rc:
            raise MtpError(rc, "cfg_grade")
        return g.value

    def coeff_tables_device(self, stream=None):
        """what the kernels will read, copied back from device memory (mtp_context_coeff_tables_device): dict of host arrays
        blob_radial, blob_seed_val, blob_e_lin (None unless scalars_in_lds), blob_leaf_cf, blob_leaf_cb, hbm_seed_val,
        hbm_e_lin, hbm_leaf_cf, hbm_leaf_cb, species, design_radial (None before the first design call), ainv_pad, ainv_tiled
        (None without a selection state), plus scalars_in_lds"""
        st = C.c_void_p(stream) if stream else None
        cnt = np.zeros(10, np.int32)
        self._check(lib().mtp_context_coeff_tables_device(self.h, st, _np(cnt, C.c_int32), *([None] * 13)))
        n_rad, n_seed, n_lin, n_cf, n_cb, n_sp, n_dr, n_pad, n_til, in_lds = [int(v) for v in cnt]
        names = ("blob_radial", "blob_seed_val", "blob_e_lin", "blob_leaf_cf", "blob_leaf_cb", "hbm_seed_val", "hbm_e_lin",
                 "hbm_leaf_cf", "hbm_leaf_cb", "species", "design_radial", "ainv_pad", "ainv_tiled")
        sizes = (n_rad, n_seed if in_lds else None, n_lin if in_lds else None, n_cf, n_cb, n_seed, n_lin, n_cf, n_cb, n_sp,
                 n_dr or None, n_pad or None, n_til or None)
        out = {n: (None if k is None else np.zeros(k)) for n, k in zip(names, sizes)}
        self._check(lib().mtp_context_coeff_tables_device(self.h, st, None, *[_np(out[n], C.c_double) for n in names]))
        out["scalars_in_lds"] = bool(in_lds)
        return out

    def save(self, dst):
        """Writes the potential file of the context's CURRENT state to `dst` through the existing writers: the source file
        (Potential.path) supplies the structure, write_all_coeffs the three coefficient blocks and, for a potential loaded
        with its selection state, write_selection the two raw blocks behind the source's #MVS header lines.  A Context
        created on `dst` holds bit for bit the tables this one holds."""
        c = self.coeffs()
        dst = os.fspath(dst)
        if not self.pot.info.has_selection:
            write_all_coeffs(self.pot.path, dst, c["moment_coeffs"], c["species_coeffs"], c["radial_coeffs"])
            return
        S, W = self.selection()
        tmp_sel, tmp_txt = dst + ".sel%d" % os.getpid(), dst + ".txt%d" % os.getpid()
        try:
            write_selection(self.pot.path, tmp_sel, S, W)           # the source's text, '#', the new blocks
            write_all_coeffs(tmp_sel, tmp_txt, c["moment_coeffs"], c["species_coeffs"], c["radial_coeffs"])   # new text, no tail
            data = open(tmp_sel, "rb").read()
            k = data.find(b"#MVS_v1.1")
            k = data.rfind(b"\n", 0, k) + 1                         # (the writer ends its file at the start of that line)
            with open(tmp_txt, "ab") as f:
                f.write(data[k:])
            os.replace(tmp_txt, dst)
        finally:
            for t in (tmp_sel, tmp_txt):
                if os.path.exists(t):
                    os.remove(t)

    def last_shape(self):
        """name of the fixed-shape kernel the last force launch ran, "" for a generic kernel"""
        buf = C.create_string_buffer(128)
        self._check(lib().mtp_context_last_shape(self.h, buf, 128))
        return buf.value.decode()

    def plan_info(self):
        a, b = C.c_int32(), C.c_int32()
        self._check(lib().mtp_context_plan_info(self.h, C.byref(a), C.byref(b)))
        return dict(waves_per_simd=a.value, rebuild_tables=b.value)

    def layout_mode(self):
        """per-atom LDS layout of the force plan: 0 keep, 1 lean, 2 rebuild, 3 rebuild-nodg"""
        m = C.c_int32()
        self._check(lib().mtp_context_layout_mode(self.h, C.byref(m)))
        return m.value

    def launch_info(self):
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(lib().mtp_context_launch_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(lds_bytes_per_wave=a.value, waves_per_block=b.value, grid_blocks=c.value,
                    neighbor_tile=d.value)

    def set_deterministic(self, on=True):
        self._check(lib().mtp_context_set_deterministic(self.h, int(on)))

    def set_timing(self, on=True):
        self._check(lib().mtp_context_set_timing(self.h, int(on)))

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(lib().mtp_context_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value


def _device_view(ptr, nrows, ld):
    """torch view [nrows, ld] (fp64) of device memory the library owns -- no copy; the caller keeps the owner alive"""
    import torch

    class _Span:
        pass
    span = _Span()
    span.__cuda_array_interface__ = dict(shape=(int(nrows), int(ld)), typestr="<f8", data=(int(ptr), False), version=2,
                                         strides=None)
    if nrows == 0:
        return torch.zeros((0, int(ld)), dtype=torch.float64, device="cuda")
    return torch.as_tensor(span, device="cuda")


def write_selection(src, dst, active_set, inverse_active_set):
    """`src` with its two raw selection blocks replaced by active_set (S: columns = selected candidate vectors) and
    inverse_active_set (W = S^-1), written to `dst` through a temporary file: mtp_potential_write_selection (host only)"""
    S = np.ascontiguousarray(active_set, dtype=np.float64)
    W = np.ascontiguousarray(inverse_active_set, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or W.shape != S.shape:
        raise ValueError("write_selection: active_set and inverse_active_set must be square matrices of one size")
    err = C.create_string_buffer(512)
    rc = lib().mtp_potential_write_selection(os.fsencode(src), os.fsencode(dst), _np(S, C.c_double), _np(W, C.c_double),
                                             int(S.shape[0]), err, 512)
    if rc:
        raise MtpError(rc, err.value.decode())


def zero_async(t, stream=None):
    """t[...] = 0 on `stream` in one kernel launch (fp64 tensor)"""
    rc = lib().mtp_zero_async(C.c_void_p(stream) if stream else None, _ptr(t), C.c_longlong(t.numel()))
    if rc:
        raise MtpError(rc, "mtp_zero_async")


def halo_unique_id():
    """ncclGetUniqueId (one rank calls this and hands the bytes to every rank)."""
    buf = C.create_string_buffer(HALO_ID_BYTES)
    rc = lib().mtp_halo_get_unique_id(buf)
    if rc:
        raise MtpError(rc, "ncclGetUniqueId failed")
    return buf.raw


class Halo:
    """The library's RCCL halo (include/mtp_mi355x.h, "multi-GPU halo") for one rank of a decomposition
    (domain.HaloPlan).  Creation is collective over all ranks -- unless unique_id is None: the halo then has no
    communicator (pack / unpack / layout only; segments move through Halo.local_exchange)."""

    def __init__(self, plan, device, unique_id):
        self.plan = plan
        self.h = C.c_void_p()
        idx = np.ascontiguousarray(plan.send_idx, np.int32)
        shift = np.ascontiguousarray(plan.send_shift, np.float64).reshape(-1, 3)
        sc = np.ascontiguousarray(plan.send_counts, np.int32)
        rc_ = np.ascontiguousarray(plan.recv_counts, np.int32)
        assert (unique_id is None or len(unique_id) == HALO_ID_BYTES) and len(sc) == plan.nranks == len(rc_)
        err = C.create_string_buffer(512)
        rc = lib().mtp_halo_create(int(device), int(plan.nranks), int(plan.rank), unique_id, int(plan.nlocal),
                                   int(plan.nghost), _np(idx, C.c_int), _np(shift, C.c_double), _np(sc, C.c_int),
                                   _np(rc_, C.c_int), C.byref(self.h), err, 512)
        if rc:
            raise MtpError(rc, err.value.decode())

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.mtp_halo_destroy(self.h)
            self.h = None

    def _check(self, rc):
        if rc:
            raise MtpError(rc, lib().mtp_halo_last_error(self.h).decode())

    def comm_count(self):
        n, r, v = C.c_int(), C.c_int(), C.c_int()
        self._check(lib().mtp_halo_comm_count(self.h, C.byref(n), C.byref(r), C.byref(v)))
        return dict(nranks=n.value, rank=r.value, rccl_version=v.value)

    @staticmethod
    def _st(stream):
        return C.c_void_p(stream) if stream else None

    def forward_begin(self, x_t, stream=None):
        self._check(lib().mtp_halo_forward_begin(self.h, self._st(stream), _ptr(x_t)))

    def forward_end(self, stream=None):
        self._check(lib().mtp_halo_forward_end(self.h, self._st(stream)))

    def forward(self, x_t, stream=None):
        self._check(lib().mtp_halo_forward(self.h, self._st(stream), _ptr(x_t)))

    def reverse_begin(self, f_t, stream=None):
        self._check(lib().mtp_halo_reverse_begin(self.h, self._st(stream), _ptr(f_t)))

    def reverse_end(self, f_t, stream=None):
        self._check(lib().mtp_halo_reverse_end(self.h, self._st(stream), _ptr(f_t)))

    def reverse(self, f_t, stream=None):
        self._check(lib().mtp_halo_reverse(self.h, self._st(stream), _ptr(f_t)))

    def force_step(self, ctx, rows, x_t, type_t, f_t, eflag=0, vflag=0, grade=False, eatom_t=None, vatom_t=None, ev_t=None,
                   grades_t=None, maxg_t=None, coeff_t=None, stream=None):
        """One decomposed force call (one C call).  Default: zero f + pack, forward exchange, all rows in one launch,
        reverse exchange, unpack, on one stream; after set_overlap(True): forward halo || interior rows, boundary rows,
        reverse halo || interior rows (rows = (nA, nB, nC) of domain.overlap_order)."""
        na, nb, nc = rows
        rc = lib().mtp_halo_force_step(self.h, ctx.h, self._st(stream), int(na), int(nb), int(nc), _ptr(x_t), _ptr(type_t),
                                       int(eflag), int(vflag), int(bool(grade)), _ptr(f_t), _ptr(eatom_t), _ptr(vatom_t),
                                       _ptr(ev_t), _ptr(grades_t), _ptr(maxg_t), _ptr(coeff_t))
        if rc:
            msg = lib().mtp_halo_last_error(self.h).decode() or lib().mtp_last_error(ctx.h).decode()
            raise MtpError(rc, msg)

    def pack_forward(self, x_t, stream):
        self._check(lib().mtp_halo_pack_forward(self.h, self._st(stream), _ptr(x_t)))

    def unpack_reverse(self, f_t, stream):
        self._check(lib().mtp_halo_unpack_reverse(self.h, self._st(stream), _ptr(f_t)))

    def layout(self):
        n = self.plan.nranks
        ns = C.c_int()
        so, sc, ro, rc_ = (np.zeros(n + 1, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int32), np.zeros(n, np.int32))
        self._check(lib().mtp_halo_get_layout(self.h, C.byref(ns), _np(so, C.c_int), _np(sc, C.c_int), _np(ro, C.c_int),
                                              _np(rc_, C.c_int)))
        return dict(nsend=ns.value, send_off=so, send_counts=sc, recv_off=ro, recv_counts=rc_)

    @staticmethod
    def local_exchange(halos, direction, arrays, stream):
        """All ranks' exchange of one direction (0 forward: arrays = positions, 1 reverse: arrays = forces) between the
        halo objects of one decomposition living in this process (mtp_halo_local_exchange)."""
        n = len(halos)
        hs = (C.c_void_p * n)(*[h.h for h in halos])
        ps = (C.c_void_p * n)(*[t.data_ptr() for t in arrays])
        rc = lib().mtp_halo_local_exchange(hs, n, C.c_void_p(stream), int(direction), ps)
        if rc:
            raise MtpError(rc, lib().mtp_halo_last_error(halos[0].h).decode())

    def set_overlap(self, enable):
        self._check(lib().mtp_halo_set_overlap(self.h, int(bool(enable))))

    @property
    def overlap(self):
        return bool(lib().mtp_halo_get_overlap(self.h))

    def allreduce(self, buf_t, op=REDUCE_SUM, stream=None):
        self._check(lib().mtp_halo_allreduce(self.h, self._st(stream), _ptr(buf_t), int(buf_t.numel()), int(op)))


class Ghosts:
    """Periodic ghost images of one GPU's own atoms, kept on the device (mtp_ghosts_*)."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib().mtp_ghosts_create(int(device), C.byref(self.h))
        if rc:
            raise MtpError(rc, "mtp_ghosts_create")
        self.nall = 0

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.mtp_ghosts_destroy(self.h)
            self.h = None

    def _check(self, rc):
        if rc:
            raise MtpError(rc, lib().mtp_ghosts_last_error(self.h).decode())

    def build(self, x_t, nlocal, box, rghost, stream=None):
        """Wraps x_t[:nlocal] and writes the ghost positions behind them; returns nall.  x_t must have room:
        raises MtpError(LIMIT) otherwise, with self.nall set to the size needed."""
        b3 = (C.c_double * 3)(*[float(v) for v in box])
        nall = C.c_int(0)
        rc = lib().mtp_ghosts_build(self.h, C.c_void_p(stream) if stream else None, _ptr(x_t), int(nlocal),
                                    int(x_t.shape[0]), b3, C.c_double(rghost), C.byref(nall))
        self.nall = nall.value
        self._check(rc)
        return nall.value

    def build_cell(self, x_t, nlocal, cell, rghost, stream=None):
        """The same for any periodic cell (rows of the 3x3 `cell` are the lattice vectors; smaller than rghost is fine):
        mtp_ghosts_build_cell.  Same capacity protocol as build()."""
        c9 = (C.c_double * 9)(*[float(v) for v in np.asarray(cell, dtype=np.float64).reshape(9)])
        nall = C.c_int(0)
        rc = lib().mtp_ghosts_build_cell(self.h, C.c_void_p(stream) if stream else None, _ptr(x_t), int(nlocal),
                                         int(x_t.shape[0]), c9, C.c_double(rghost), C.byref(nall))
        self.nall = nall.value
        self._check(rc)
        return nall.value

    def build_batch(self, x_t, cfg_first, cells, origins, rghost, stream=None):
        """The same for many cells at once (mtp_ghosts_build_batch): owned atoms of configuration k are rows
        [cfg_first[k], cfg_first[k + 1]) of x_t, wrapped into cells[k] and translated by origins[k] (host arrays; the origins
        come from batch_layout).  Same capacity protocol as build()."""
        cf = np.ascontiguousarray(cfg_first, dtype=np.int32)
        ncfg = len(cf) - 1
        c9 = np.ascontiguousarray(cells, dtype=np.float64).reshape(ncfg, 9)
        o3 = np.ascontiguousarray(origins, dtype=np.float64).reshape(ncfg, 3)
        nall = C.c_int(0)
        rc = lib().mtp_ghosts_build_batch(self.h, C.c_void_p(stream) if stream else None, _ptr(x_t), ncfg, _np(cf, C.c_int),
                                          _np(c9, C.c_double), _np(o3, C.c_double), int(x_t.shape[0]), C.c_double(rghost),
                                          C.byref(nall))
        self.nall = nall.value
        self._check(rc)
        return nall.value

    def forward(self, x_t, stream=None):
        self._check(lib().mtp_ghosts_forward(self.h, C.c_void_p(stream) if stream else None, _ptr(x_t)))

    def reverse(self, f_t, stream=None):
        self._check(lib().mtp_ghosts_reverse(self.h, C.c_void_p(stream) if stream else None, _ptr(f_t)))

    def reverse_finish(self, ctx, f_t, ev_t, eflag=0, vflag=0, stream=None):
        """ghost forces onto their owners + the tally fold of a force call made with finish_tallies=False, one launch"""
        self._check(lib().mtp_ghosts_reverse_finish(self.h, ctx.h, C.c_void_p(stream) if stream else None, int(eflag), int(vflag),
                                                    _ptr(f_t), _ptr(ev_t)))

    def types(self, type_t, stream=None):
        self._check(lib().mtp_ghosts_types(self.h, C.c_void_p(stream) if stream else None, _ptr(type_t)))

    def deform(self, row_cfg_t, T_t, stream=None):
        """the ghosts follow a deforming cell: shift = (shift of the last build) . T_t[configuration of the owner], T_t
        [ncfg, 3, 3] as relax_cell_step leaves it (mtp_ghosts_deform)"""
        self._check(lib().mtp_ghosts_deform(self.h, C.c_void_p(stream) if stream else None, _ptr(row_cfg_t), _ptr(T_t)))

    def owner(self, stream=None):
        """(device pointer, nall) of the owner map of the last build over ALL rows -- identity on the owned rows -- in
        storage of the handle, valid until the next build (mtp_ghosts_owner_device)"""
        d, n = C.c_void_p(), C.c_int(0)
        self._check(lib().mtp_ghosts_owner_device(self.h, C.c_void_p(stream) if stream else None, C.byref(d), C.byref(n)))
        return d.value, n.value


def ghosts_cell_bounds(cell, rghost):
    """Host arithmetic (no device): dict(lo, hi, volume, nimage) -- the bounds of every position Ghosts.build_cell can
    write for this cell (what build_neighbors_device wants), the cell volume, the images per direction and sign."""
    c9 = (C.c_double * 9)(*[float(v) for v in np.asarray(cell, dtype=np.float64).reshape(9)])
    lo, hi, vol, nim = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(0), (C.c_int * 3)()
    rc = lib().mtp_ghosts_cell_bounds(c9, C.c_double(rghost), lo, hi, C.byref(vol), nim)
    if rc:
        raise MtpError(rc, "mtp_ghosts_cell_bounds: the cell must be finite with det > 0, rghost > 0")
    return dict(lo=np.array(lo[:]), hi=np.array(hi[:]), volume=vol.value, nimage=np.array(nim[:], dtype=np.int64))


def batch_layout(cells, rghost, gap=None):
    """Host arithmetic (no device): one slot per configuration in one box, any two at least `gap` (default rghost, the list
    cutoff) apart -- mtp_batch_layout.  cells [ncfg, 3, 3].  Returns dict(origins [ncfg, 3], lo, hi, ncells); raises
    MtpError with .nfit = the number of leading configurations that do fit when the batch is beyond the layout's limits."""
    c9 = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 9)
    ncfg = len(c9)
    org = np.zeros((ncfg, 3))
    lo, hi, nc, nfit = (C.c_double * 3)(), (C.c_double * 3)(), C.c_longlong(0), C.c_int(0)
    err = C.create_string_buffer(512)
    rc = lib().mtp_batch_layout(ncfg, _np(c9, C.c_double), C.c_double(rghost), C.c_double(rghost if gap is None else gap),
                                _np(org, C.c_double), lo, hi, C.byref(nc), C.byref(nfit), err, 512)
    if rc:
        e = MtpError(rc, err.value.decode())
        e.nfit = nfit.value
        raise e
    return dict(origins=org, lo=np.array(lo[:]), hi=np.array(hi[:]), ncells=nc.value)


def batch_reduce(cfg_first_t, eatom_t=None, vatom_t=None, grades_t=None, energy_t=None, virial_t=None, cfg_grade_t=None,
                 stream=None):
    """per-configuration sums of eatom / vatom and maxima of grades over rows [cfg_first[k], cfg_first[k + 1]), all device
    tensors (mtp_batch_reduce)"""
    rc = lib().mtp_batch_reduce(C.c_void_p(stream) if stream else None, int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t),
                                _ptr(eatom_t), _ptr(vatom_t), _ptr(grades_t), _ptr(energy_t), _ptr(virial_t), _ptr(cfg_grade_t))
    if rc:
        raise MtpError(rc, "mtp_batch_reduce: needs a stream, and an input for every output")


def batch_design_reduce(cfg_first_t, ld, basis_t=None, virial_atom_t=None, energy_t=None, virial_t=None, stream=None):
    """per-configuration design rows: sums of the per-atom basis rows [rows, ld] into energy_t [ncfg, ld] and of the
    per-atom virial rows [rows, 6, ld] into virial_t [ncfg, 6, ld] over rows [cfg_first[k], cfg_first[k + 1]), all device
    tensors (mtp_batch_design_reduce)"""
    rc = lib().mtp_batch_design_reduce(C.c_void_p(stream) if stream else None, int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t),
                                       int(ld), _ptr(basis_t), _ptr(virial_atom_t), _ptr(energy_t), _ptr(virial_t))
    if rc:
        raise MtpError(rc, "mtp_batch_design_reduce: needs a stream, and an input for every output")


def write_coeffs(src, dst, moment_coeffs, species_coeffs=None):
    """`src` with its moment_coeffs (and, unless None, species_coeffs) replaced, 17 significant digits, written to `dst`
    through a temporary file: mtp_potential_write_coeffs (host only).  Returns 0, or WROTE_WITHOUT_SELECTION when `src`
    carries an #MVS selection tail: the tail describes the old coefficients and is left out of `dst`."""
    m = np.ascontiguousarray(moment_coeffs, dtype=np.float64).reshape(-1)
    sp = None if species_coeffs is None else np.ascontiguousarray(species_coeffs, dtype=np.float64).reshape(-1)
    err = C.create_string_buffer(512)
    rc = lib().mtp_potential_write_coeffs(os.fsencode(src), os.fsencode(dst), _np(sp, C.c_double), _np(m, C.c_double),
                                          -1 if sp is None else len(sp), len(m), err, 512)
    if rc < 0:
        raise MtpError(rc, err.value.decode())
    return rc


def write_all_coeffs(src, dst, moment_coeffs, species_coeffs=None, radial_coeffs=None):
    """write_coeffs with the radial block as well ([Sp, Sp, Mu, R] in any shape of that order; None keeps the source's):
    mtp_potential_write_all_coeffs (host only).  Returns 0 or WROTE_WITHOUT_SELECTION."""
    m = np.ascontiguousarray(moment_coeffs, dtype=np.float64).reshape(-1)
    sp = None if species_coeffs is None else np.ascontiguousarray(species_coeffs, dtype=np.float64).reshape(-1)
    ra = None if radial_coeffs is None else np.ascontiguousarray(radial_coeffs, dtype=np.float64).reshape(-1)
    err = C.create_string_buffer(512)
    rc = lib().mtp_potential_write_all_coeffs(os.fsencode(src), os.fsencode(dst), _np(ra, C.c_double), _np(sp, C.c_double),
                                              _np(m, C.c_double), -1 if ra is None else len(ra), -1 if sp is None else len(sp),
                                              len(m), err, 512)
    if rc < 0:
        raise MtpError(rc, err.value.decode())
    return rc


def nve_initial(nlocal, x_t, v_t, f_t, type_t, inv_mass_t, dtf, dt, stream=None):
    rc = lib().mtp_nve_initial(C.c_void_p(stream) if stream else None, int(nlocal), _ptr(x_t), _ptr(v_t), _ptr(f_t),
                               _ptr(type_t), _ptr(inv_mass_t), C.c_double(dtf), C.c_double(dt))
    if rc:
        raise MtpError(rc, "mtp_nve_initial")


def nve_final(nlocal, v_t, f_t, type_t, inv_mass_t, dtf, stream=None):
    rc = lib().mtp_nve_final(C.c_void_p(stream) if stream else None, int(nlocal), _ptr(v_t), _ptr(f_t), _ptr(type_t),
                             _ptr(inv_mass_t), C.c_double(dtf))
    if rc:
        raise MtpError(rc, "mtp_nve_final")


def nve_monitor(nlocal, x_t, x_ref_t, v_t, type_t, mass_t, out2_t, stream=None):
    rc = lib().mtp_nve_monitor(C.c_void_p(stream) if stream else None, int(nlocal), _ptr(x_t), _ptr(x_ref_t), _ptr(v_t),
                               _ptr(type_t), _ptr(mass_t), _ptr(out2_t))
    if rc:
        raise MtpError(rc, "mtp_nve_monitor")


# ---- batched sampling (include/mtp_mi355x.h): all arguments are device tensors in the layout of the batched configurations

def _st(stream):
    return C.c_void_p(stream) if stream else None


def sample_row_map(cfg_first_t, row_cfg_t, stream=None):
    """row_cfg_t[i] = the configuration of owned row i, for all rows of row_cfg_t: mtp_sample_row_map"""
    rc = lib().mtp_sample_row_map(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), int(row_cfg_t.numel()),
                                  _ptr(row_cfg_t))
    if rc:
        raise MtpError(rc, "mtp_sample_row_map")


def sample_initial(nrows, row_cfg_t, frozen_t, x_t, v_t, f_t, type_t, inv_mass_t, dtf, dt, stream=None):
    """first half step of the unfrozen configurations: mtp_sample_initial"""
    rc = lib().mtp_sample_initial(_st(stream), int(nrows), _ptr(row_cfg_t), _ptr(frozen_t), _ptr(x_t), _ptr(v_t), _ptr(f_t),
                                  _ptr(type_t), _ptr(inv_mass_t), C.c_double(dtf), C.c_double(dt))
    if rc:
        raise MtpError(rc, "mtp_sample_initial")


def sample_final(nrows, row_cfg_t, cfg_first_t, frozen_t, v_t, f_t, type_t, mass_t, inv_mass_t, temperature_t, key_t, seed, step,
                 dtf, dt, t_damp, stream=None):
    """fix langevin's force (Philox4x32-10 noise keyed by key_t [ncfg] int64 and `seed`) and the second half step of the
    unfrozen configurations in one launch; t_damp <= 0 or infinite: the second half step alone.  mtp_sample_final"""
    rc = lib().mtp_sample_final(_st(stream), int(nrows), _ptr(row_cfg_t), _ptr(cfg_first_t), _ptr(frozen_t), _ptr(v_t), _ptr(f_t),
                                _ptr(type_t), _ptr(mass_t), _ptr(inv_mass_t), _ptr(temperature_t), _ptr(key_t),
                                C.c_ulonglong(int(seed) & (2 ** 64 - 1)), int(step), C.c_double(dtf), C.c_double(dt),
                                C.c_double(t_damp))
    if rc:
        raise MtpError(rc, "mtp_sample_final")


def sample_monitor(cfg_first_t, frozen_t, x_t, x_ref_t, v_t, type_t, mass_t, counts_t, mv2_t, d2_t, block_t, stream=None):
    """mv2_t[k] = sum m v^2, d2_t[k] = largest squared displacement from x_ref_t (0 where frozen), block_t [4] = (max d2,
    frozen, captured, dropped): mtp_sample_monitor"""
    rc = lib().mtp_sample_monitor(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), _ptr(frozen_t), _ptr(x_t),
                                  _ptr(x_ref_t), _ptr(v_t), _ptr(type_t), _ptr(mass_t), _ptr(counts_t), _ptr(mv2_t), _ptr(d2_t),
                                  _ptr(block_t))
    if rc:
        raise MtpError(rc, "mtp_sample_monitor")


def sample_capture(cfg_first_t, nrows, row_cfg_t, cfg_grade_t, step, threshold_select, threshold_break, capture_gap, x_t,
                   origins_t, frozen_t, last_capture_t, slot_t, max_candidates, stride, cand_x_t, rec_t, rec_grade_t, counts_t,
                   stream=None):
    """the capture and freeze decisions of a grade step with their snapshots, on the device: mtp_sample_capture.  cand_x_t
    [max_candidates, stride, 3], rec_t [max_candidates, 2] int32 (configuration, step), rec_grade_t [max_candidates],
    counts_t [3] int32 (captured, dropped, frozen; accumulated)"""
    rc = lib().mtp_sample_capture(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), int(nrows), _ptr(row_cfg_t),
                                  _ptr(cfg_grade_t), int(step), C.c_double(threshold_select), C.c_double(threshold_break),
                                  int(capture_gap), _ptr(x_t), _ptr(origins_t), _ptr(frozen_t), _ptr(last_capture_t), _ptr(slot_t),
                                  int(max_candidates), int(stride), _ptr(cand_x_t), _ptr(rec_t), _ptr(rec_grade_t), _ptr(counts_t))
    if rc:
        raise MtpError(rc, "mtp_sample_capture")


def sample_to_cell(nrows, row_cfg_t, origins_t, x_t, stream=None):
    """slot coordinates back to cell coordinates in front of a re-neighbouring: mtp_sample_to_cell"""
    rc = lib().mtp_sample_to_cell(_st(stream), int(nrows), _ptr(row_cfg_t), _ptr(origins_t), _ptr(x_t))
    if rc:
        raise MtpError(rc, "mtp_sample_to_cell")


# ---- batched relaxation (include/mtp_mi355x.h): device tensors in the layout of the batched configurations

RELAX_STATUS = ("running", "captured-frozen", "converged", "failed")       # frozen_t[k] = 0, 1, 2, 3


class RelaxParams(C.Structure):
    """mtp_relax_params"""
    _fields_ = [(n, C.c_double) for n in ("ftol", "dt_max", "dmax", "f_inc", "f_dec", "alpha_start", "f_alpha")] + [("n_min", C.c_int)]


def relax_step(cfg_first_t, params, step, x_t, v_t, f_t, type_t, inv_mass_t, dt_t, alpha_t, npos_t, frozen_t, done_step_t, fmax_t,
               counts_t, last=False, stream=None):
    """one FIRE step of every running configuration, with the convergence decision, in one launch: mtp_relax_step.  `params`
    is a RelaxParams; dt_t, alpha_t, fmax_t [ncfg] float64 and npos_t, frozen_t, done_step_t [ncfg] int32 are per configuration,
    counts_t [3] int32 is sample_capture's.  last=True only decides."""
    rc = lib().mtp_relax_step(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), C.byref(params), int(step), int(bool(last)),
                              _ptr(x_t), _ptr(v_t), _ptr(f_t), _ptr(type_t), _ptr(inv_mass_t), _ptr(dt_t), _ptr(alpha_t),
                              _ptr(npos_t), _ptr(frozen_t), _ptr(done_step_t), _ptr(fmax_t), _ptr(counts_t))
    if rc:
        raise MtpError(rc, "mtp_relax_step")


# ---- batched variable-cell relaxation (include/mtp_mi355x.h)

GPA = 1.0 / 160.21766                                                       # 1 GPa in eV/A^3


class RelaxCellParams(C.Structure):
    """mtp_relax_cell_params"""
    _fields_ = [("fire", RelaxParams)] + [(n, C.c_double) for n in ("stol", "pressure", "cell_factor", "cell_mass")] + \
               [("cell_mask", C.c_int * 6), ("isotropic", C.c_int), ("factor_per_atom", C.c_int)]


RELAX_CELL_ARRAYS = ("cfg_first", "x", "xt", "vt", "f", "type", "inv_mass", "virial", "h0", "origins", "D", "vq", "Dbinv", "href",
                     "nimg", "dt", "alpha", "npos", "frozen", "done_step", "fmax", "smax", "gcell", "h", "T", "cellmove", "counts")


class RelaxCellArrays(C.Structure):
    """mtp_relax_cell_arrays: device pointers, in the order of RELAX_CELL_ARRAYS"""
    _fields_ = [(n, C.c_void_p) for n in RELAX_CELL_ARRAYS]


def relax_cell_params(fire, stol, pressure, cell_factor, cell_mass, cell_mask=(1, 1, 1, 1, 1, 1), isotropic=False,
                      factor_per_atom=False):
    """a RelaxCellParams from a RelaxParams and the cell arguments (no check: mtp_relax_cell_step makes them)"""
    return RelaxCellParams(fire, float(stol), float(pressure), float(cell_factor), float(cell_mass),
                           (C.c_int * 6)(*[int(m) for m in cell_mask]), int(bool(isotropic)), int(bool(factor_per_atom)))


def relax_cell_step(ncfg, params, step, arrays, last=False, stream=None):
    """one FIRE step over atoms and cell of every running configuration, in one launch: mtp_relax_cell_step.  `params` is a
    RelaxCellParams, `arrays` a dict of device tensors with the keys RELAX_CELL_ARRAYS (float64; type, nimg, npos, frozen,
    done_step, counts and cfg_first int32)."""
    A = RelaxCellArrays(*[_ptr(arrays.get(n)) for n in RELAX_CELL_ARRAYS])
    rc = lib().mtp_relax_cell_step(_st(stream), int(ncfg), C.byref(params), int(step), int(bool(last)), C.byref(A))
    if rc:
        raise MtpError(rc, "mtp_relax_cell_step")


def relax_cell_rebase(ncfg, row_cfg_t, origins_t, x_t, D_t, xt_t, Dbinv_t, stream=None):
    """after a re-neighbouring: xt = (x - origin) . D^-1 for every owned row, Dbinv = D^-1: mtp_relax_cell_rebase"""
    rc = lib().mtp_relax_cell_rebase(_st(stream), int(ncfg), int(row_cfg_t.numel()), _ptr(row_cfg_t), _ptr(origins_t), _ptr(x_t),
                                     _ptr(D_t), _ptr(xt_t), _ptr(Dbinv_t))
    if rc:
        raise MtpError(rc, "mtp_relax_cell_rebase")


def relax_cell_capture_cells(slot_t, max_candidates, h_t, cand_cell_t, stream=None):
    """cand_cell_t[slot] = h_t[k] for the configurations sample_capture just gave a slot: mtp_relax_cell_capture_cells"""
    rc = lib().mtp_relax_cell_capture_cells(_st(stream), int(slot_t.numel()), _ptr(slot_t), int(max_candidates), _ptr(h_t),
                                            _ptr(cand_cell_t))
    if rc:
        raise MtpError(rc, "mtp_relax_cell_capture_cells")


# ---- batched constant-pressure sampling (include/mtp_mi355x.h)

class SampleCellParams(C.Structure):
    """mtp_sample_cell_params"""
    _fields_ = [(n, C.c_double) for n in ("dt", "dtf", "tau_p", "compressibility", "pressure", "strain_max")] + \
               [("cell_mask", C.c_int * 6), ("isotropic", C.c_int), ("seed", C.c_ulonglong)]


SAMPLE_CELL_ARRAYS = ("cfg_first", "x", "v", "f", "type", "inv_mass", "mass", "virial", "temperature", "key", "origins", "V0", "h", "T",
                      "href", "nimg", "frozen", "done_step", "cellmove", "capped", "press", "counts")


class SampleCellArrays(C.Structure):
    """mtp_sample_cell_arrays: device pointers, in the order of SAMPLE_CELL_ARRAYS"""
    _fields_ = [(n, C.c_void_p) for n in SAMPLE_CELL_ARRAYS]


def sample_cell_params(dt, dtf, tau_p, compressibility, pressure, strain_max=0.01, cell_mask=(1, 1, 1, 1, 1, 1), isotropic=False,
                       seed=0):
    """a SampleCellParams (no check: mtp_sample_cell_step makes them); tau_p None: the barostat is off"""
    return SampleCellParams(float(dt), float(dtf), 0.0 if tau_p is None else float(tau_p), float(compressibility), float(pressure),
                            float(strain_max), (C.c_int * 6)(*[int(m) for m in cell_mask]), int(bool(isotropic)),
                            int(seed) & (2 ** 64 - 1))


def sample_cell_step(ncfg, params, step, arrays, stream=None):
    """the first half step of every running configuration with its barostat move, in one launch: mtp_sample_cell_step.  `params`
    is a SampleCellParams, `arrays` a dict of device tensors with the keys SAMPLE_CELL_ARRAYS (float64; key int64; type, nimg,
    frozen, done_step, capped, counts and cfg_first int32)."""
    A = SampleCellArrays(*[_ptr(arrays.get(n)) for n in SAMPLE_CELL_ARRAYS])
    rc = lib().mtp_sample_cell_step(_st(stream), int(ncfg), C.byref(params), int(step), C.byref(A))
    if rc:
        raise MtpError(rc, "mtp_sample_cell_step")


# ---- batched nudged elastic band (include/mtp_mi355x.h)

NEB_STATUS = ("running", "captured-frozen", "converged", "failed")         # band_status[b] = 0, 1, 2, 3
NEB_MAX_IMAGES = 64


class NebParams(C.Structure):
    """mtp_neb_params: NebParams(RelaxParams, spring, climb_step); climb_step < 0: no image ever climbs"""
    _fields_ = [("fire", RelaxParams), ("spring", C.c_double), ("climb_step", C.c_int)]


NEB_ARRAYS = ("band_first", "cfg_first", "x", "v", "f", "eatom", "type", "inv_mass", "origins", "cell", "cell_inv", "fneb", "energy",
              "dt", "alpha", "npos", "done_step", "fmax", "climber", "band_status", "frozen", "counts")


class NebArrays(C.Structure):
    """mtp_neb_arrays: device pointers, in the order of NEB_ARRAYS"""
    _fields_ = [(n, C.c_void_p) for n in NEB_ARRAYS]


def neb_step(band_first, ncfg, params, step, arrays, last=False, stream=None):
    """one climbing-image NEB step of every running band, with the convergence decision, in one launch: mtp_neb_step.
    `band_first` [nband + 1] is the HOST band table (int32 numpy; the argument check reads it), arrays["band_first"] its copy on
    the device; `params` is a NebParams, `arrays` a dict of device tensors with the keys NEB_ARRAYS (float64; band_first,
    cfg_first, type, npos, done_step, climber, band_status, frozen and counts int32).  last=True only decides."""
    bf = np.ascontiguousarray(band_first, dtype=np.int32)
    A = NebArrays(*[_ptr(arrays.get(n)) for n in NEB_ARRAYS])
    rc = lib().mtp_neb_step(_st(stream), len(bf) - 1, _np(bf, C.c_int), int(ncfg), C.byref(params), int(step), int(bool(last)),
                            C.byref(A))
    if rc:
        raise MtpError(rc, "mtp_neb_step")


# ---- batched force constants (include/mtp_mi355x.h)

HESS_STATUS = ("ok", "failed")                                              # status_t[j] = 0, 1
HESS_MAX_SELECTED = 2 ** 28


def hess_step(cfg_first_t, sel_first_t, sel_t, sel_max, k, h, x_t, x0_t, f_t, eatom_t, h_first_t, H_t, f0_t, fmax_t, energy_t,
              status_t, stream=None):
    """launch k = 0 ... 6 sel_max of a pass of central differences: harvest displacement k - 1 into its row of H, put the moved
    coordinate back from x0_t, make displacement k: mtp_hess_step.  sel_first_t [ncfg + 1], sel_t (row numbers) and status_t
    [ncfg] are int32, h_first_t [ncfg] int64; H_t holds the [3 m][3 m] matrices one after another; f0_t [n, 3], fmax_t and
    energy_t [ncfg] are written by launch 0."""
    rc = lib().mtp_hess_step(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), _ptr(sel_first_t), _ptr(sel_t), int(sel_max),
                             int(k), C.c_double(h), _ptr(x_t), _ptr(x0_t), _ptr(f_t), _ptr(eatom_t), _ptr(h_first_t), _ptr(H_t),
                             _ptr(f0_t), _ptr(fmax_t), _ptr(energy_t), _ptr(status_t))
    if rc:
        raise MtpError(rc, "mtp_hess_step")


def hess_finish(sel_first_t, sel_t, type_t, mass_t, mass_weight, h_first_t, H_t, diag_t, status_t, stream=None):
    """the end of a pass: diag_t [ncfg, 2] = (asymmetry, sum_rule), H <- 0.5 (H + H^T), with mass_weight divided by
    sqrt(M_a M_b) (mass_t per type): mtp_hess_finish"""
    rc = lib().mtp_hess_finish(_st(stream), int(sel_first_t.numel()) - 1, _ptr(sel_first_t), _ptr(sel_t), _ptr(type_t), _ptr(mass_t),
                               int(bool(mass_weight)), _ptr(h_first_t), _ptr(H_t), _ptr(diag_t), _ptr(status_t))
    if rc:
        raise MtpError(rc, "mtp_hess_finish")


# ---- batched elastic constants (include/mtp_mi355x.h)

ELASTIC_STATUS = ("ok", "failed", "unstable")                               # status_t[j] = 0, 1, 2
ELASTIC_TIERS = (48, 96, 192)                                               # the LDS tiers of mtp_elastic_relax: N = 3 n up to ...
ELASTIC_RELAX_MAX_N = ELASTIC_TIERS[-1]


def elastic_step(cfg_first_t, k, h, x_t, x0_t, xt_t, origins_t, h0_t, f_t, eatom_t, virial_t, T_t, Bt_t, coupling_t, c_first_t,
                 f0_t, fmax_t, energy_t, stress0_t, status_t, stream=None):
    """launch k = 0 ... 12 of a pass of central differences over the strains x -> x (I +- h E_w): harvest strain k - 1 into row
    (k - 1) / 2 of Bt_t [ncfg, 6, 6] and of coupling_t (the [6][3 n] blocks one after another, c_first_t [ncfg] int64 = 18
    cfg_first), then lay x_t and T_t [ncfg, 9] out for strain k (k = 12: back to x0_t): mtp_elastic_step.  f0_t [n, 3], fmax_t,
    energy_t [ncfg] and stress0_t [ncfg, 6] are written by launch 0; status_t [ncfg] int32."""
    rc = lib().mtp_elastic_step(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), int(k), C.c_double(h), _ptr(x_t),
                                _ptr(x0_t), _ptr(xt_t), _ptr(origins_t), _ptr(h0_t), _ptr(f_t), _ptr(eatom_t), _ptr(virial_t),
                                _ptr(T_t), _ptr(Bt_t), _ptr(coupling_t), _ptr(c_first_t), _ptr(f0_t), _ptr(fmax_t), _ptr(energy_t),
                                _ptr(stress0_t), _ptr(status_t))
    if rc:
        raise MtpError(rc, "mtp_elastic_step")


def elastic_finish(cfg_first_t, c_first_t, coupling_t, stress0_t, Bt_t, B_t, C_t, diag_t, status_t, stream=None):
    """the end of a pass: B_t [ncfg, 6, 6] = Bt^T, C_t = sym(B - K(stress0)), diag_t [ncfg, 2] = (asymmetry, sum_rule):
    mtp_elastic_finish"""
    rc = lib().mtp_elastic_finish(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), _ptr(c_first_t), _ptr(coupling_t),
                                  _ptr(stress0_t), _ptr(Bt_t), _ptr(B_t), _ptr(C_t), _ptr(diag_t), _ptr(status_t))
    if rc:
        raise MtpError(rc, "mtp_elastic_finish")


def elastic_relax(cfg_first_t, h_first_t, H_t, c_first_t, coupling_t, vol_t, B_t, C_t, U_t, B_rel_t, C_rel_t, status_t, stream=None):
    """relaxed ions for the configurations of up to ELASTIC_RELAX_MAX_N coordinates: U_t (laid out like coupling_t) =
    (H + tau sum t t^T)^-1 Lambda^T by Cholesky in LDS, B_rel_t = B - R / V, C_rel_t = C - sym(R) / V with R = Lambda U^T;
    status_t[j] = 2 ("unstable") where a pivot is not positive: mtp_elastic_relax.  H_t: the symmetrised full Hessians of
    hess_finish without mass weights."""
    rc = lib().mtp_elastic_relax(_st(stream), int(cfg_first_t.numel()) - 1, _ptr(cfg_first_t), _ptr(h_first_t), _ptr(H_t),
                                 _ptr(c_first_t), _ptr(coupling_t), _ptr(vol_t), _ptr(B_t), _ptr(C_t), _ptr(U_t), _ptr(B_rel_t),
                                 _ptr(C_rel_t), _ptr(status_t))
    if rc:
        raise MtpError(rc, "mtp_elastic_relax")


# ---- batched symmetric eigen-solver (include/mtp_mi355x.h)

EIGH_STATUS = ("ok", "failed", "not converged", "too large")                # status_t[j] = 0, 1, 2, 3
EIGH_MAX_N, EIGH_MAX_N_VECTORS = 192, 96                                    # the largest N without and with eigenvectors


def eigh_batched(n_t, a_first_t, A_t, w_first_t, root_t, project, max_sweeps, W_t, V_t, info_t, status_t, stream=None):
    """eigenvalues (and, with V_t, eigenvectors) of the matrices [N_j, N_j] at A_t + a_first_t[j] by Jacobi sweeps in LDS:
    mtp_eigh_batched.  n_t and status_t [nmat] are int32, a_first_t and w_first_t [nmat] int64; root_t (one per coordinate, laid
    out like W_t) divides A_rc by root_r root_c, or None; project takes the three translations out (N a multiple of 3); W_t holds
    the eigenvalues ascending from w_first_t[j], V_t (or None) the eigenvectors like A_t, column i to W[i]; info_t [nmat, 2] =
    (sweeps, off-diagonal norm).  status_t[j] != 0 on entry skips the matrix; 1, 2, 3 on return: EIGH_STATUS."""
    rc = lib().mtp_eigh_batched(_st(stream), int(n_t.numel()), _ptr(n_t), _ptr(a_first_t), _ptr(A_t), _ptr(w_first_t), _ptr(root_t),
                                int(bool(project)), int(max_sweeps), _ptr(W_t), _ptr(V_t), _ptr(info_t), _ptr(status_t))
    if rc:
        raise MtpError(rc, "mtp_eigh_batched")


# ---- linear refit without the design matrix: double-double normal equations (include/mtp_mi355x.h) -------------------------
NORMAL_KINDS = ("energy", "force", "virial")


def normal_sizes():
    """dict(tile, panel, slice, workspace_cap) of the loaded build's accumulate kernel: the tile edge, the rows of an LDS
    panel, the rows of a slice (the unit of the sum order) and the fixed cap of a state's workspace in bytes"""
    t, p, s, w = C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
    lib().mtp_normal_sizes(C.byref(t), C.byref(p), C.byref(s), C.byref(w))
    return dict(tile=t.value, panel=p.value, slice=s.value, workspace_cap=w.value)


class Normal:
    """The device-side state of the normal equations (mtp_normal_*): per kind of row (0 energy, 1 force, 2 virial) the
    augmented Gram matrix of ncols + 1 columns in double-double and the number of rows that entered."""

    def __init__(self, ncols, device=0, workspace_bytes=0):
        self.h = C.c_void_p()
        rc = lib().mtp_normal_create(int(device), int(ncols), C.c_longlong(int(workspace_bytes)), C.byref(self.h))
        if rc:
            raise MtpError(rc, "mtp_normal_create(ncols = %d)" % ncols)
        self.ncols, self.n, self.device = int(ncols), int(ncols) + 1, int(device)

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.mtp_normal_destroy(self.h)
            self.h = None

    def _check(self, rc):
        if rc:
            raise MtpError(rc, lib().mtp_normal_last_error(self.h).decode())

    def info(self):
        """dict(ncols, round_slices, workspace_bytes, state_bytes)"""
        a, b, c, d = C.c_int(0), C.c_int(0), C.c_longlong(0), C.c_longlong(0)
        self._check(lib().mtp_normal_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(ncols=a.value, round_slices=b.value, workspace_bytes=c.value, state_bytes=d.value)

    def set_round_slices(self, slices):
        """fewer slices a round than the workspace holds: several rounds of accumulate + fold, the same bits"""
        rc = lib().mtp_normal_set_round_slices(self.h, int(slices))
        if rc:
            raise MtpError(rc, "mtp_normal_set_round_slices: between 1 and what the workspace holds")

    def clear(self, stream=None):
        self._check(lib().mtp_normal_clear(self.h, _st(stream)))

    def accumulate(self, kind, nrows, ld, rows_t, scale_t, target_t, stream=None):
        """adds sum_i b[i][j] b[i][k], b = scale[:, None] * [rows[:, :ncols] | target], of nrows rows of leading dimension
        ld to the matrix of `kind` (device tensors; rows of scale 0 are skipped and not counted)"""
        self._check(lib().mtp_normal_accumulate(self.h, _st(stream), int(kind), C.c_longlong(int(nrows)), int(ld), _ptr(rows_t),
                                                _ptr(scale_t), _ptr(target_t)))

    def get(self, stream=None):
        """host copies (hi [3, n, n], lo [3, n, n], counts [3]); synchronises on `stream`"""
        hi, lo = np.zeros((3, self.n, self.n)), np.zeros((3, self.n, self.n))
        cnt = (C.c_longlong * 3)()
        self._check(lib().mtp_normal_get(self.h, _st(stream), _np(hi, C.c_double), _np(lo, C.c_double), cnt))
        return hi, lo, np.array(cnt[:], dtype=np.int64)

    def set(self, hi, lo, counts, stream=None):
        hi, lo = (np.ascontiguousarray(a, dtype=np.float64) for a in (hi, lo))
        if hi.shape != (3, self.n, self.n) or lo.shape != hi.shape or len(counts) != 3:
            raise MtpError(-20, "Normal.set: hi and lo must be [3, %d, %d], counts [3]" % (self.n, self.n))
        cnt = (C.c_longlong * 3)(*[int(c) for c in counts])
        self._check(lib().mtp_normal_set(self.h, _st(stream), _np(hi, C.c_double), _np(lo, C.c_double), cnt))


def normal_factor(hi, lo, weights, theta0, drop=2.0 ** -80):
    """mtp_normal_factor (host only): hi, lo [3, n, n].  Returns dict(R [rank, ncols], q [rank], rank, pivot_order [rank],
    dropped_columns, pivot_ratios [ncols]: the kept pivots' ratios, then those of the dropped columns)."""
    hi, lo = (np.ascontiguousarray(a, dtype=np.float64) for a in (hi, lo))
    n = int(hi.shape[-1])
    if hi.shape != (3, n, n) or lo.shape != hi.shape:
        raise MtpError(-20, "normal_factor: hi and lo must be [3, n, n]")
    ncols = n - 1
    theta0 = np.ascontiguousarray(theta0, dtype=np.float64).reshape(-1)
    if len(theta0) != ncols:
        raise MtpError(-20, "normal_factor: theta0 must have %d entries" % ncols)
    P = C.POINTER(C.c_double)
    hp = (P * 3)(*[hi[k].ctypes.data_as(P) for k in range(3)])
    lp = (P * 3)(*[lo[k].ctypes.data_as(P) for k in range(3)])
    w = (C.c_double * 3)(*[float(x) for x in weights])
    R, q, ratios = np.zeros((ncols, ncols)), np.zeros(ncols), np.zeros(ncols)
    order, dropped = np.zeros(ncols, np.int32), np.zeros(ncols, np.int32)
    rank, nd = C.c_int(0), C.c_int(0)
    rc = lib().mtp_normal_factor(n, hp, lp, w, _np(theta0, C.c_double), C.c_double(drop), _np(R, C.c_double), _np(q, C.c_double),
                                 C.byref(rank), _np(order, C.c_int), _np(dropped, C.c_int), C.byref(nd), _np(ratios, C.c_double))
    if rc:
        raise MtpError(rc, "mtp_normal_factor: needs finite input, weights >= 0 (one of them positive) and no negative diagonal")
    r = rank.value
    return dict(R=R[:r].copy(), q=q[:r].copy(), rank=r, pivot_order=order[:r].copy(), dropped_columns=dropped[:nd.value].copy(),
                pivot_ratios=ratios)


def normal_quadratic(hi, lo, theta):
    """mtp_normal_quadratic (host only): the sum of squared scaled residuals of ONE kind (hi, lo [n, n]) at theta"""
    hi, lo = (np.ascontiguousarray(a, dtype=np.float64) for a in (hi, lo))
    theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
    n = int(hi.shape[-1])
    if hi.shape != (n, n) or lo.shape != hi.shape or len(theta) != n - 1:
        raise MtpError(-20, "normal_quadratic: hi and lo must be [n, n], theta [n - 1]")
    out = C.c_double(0.0)
    rc = lib().mtp_normal_quadratic(n, _np(hi, C.c_double), _np(lo, C.c_double), _np(theta, C.c_double), C.byref(out))
    if rc:
        raise MtpError(rc, "mtp_normal_quadratic: non-finite input")
    return out.value
