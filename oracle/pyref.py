"""ctypes loader for the COMPILED REFERENCE (oracle/_ref/libmtp_ref.so): the reference's own `mtp` and
`mtp/extrapolation` pair styles, built unchanged by `make -C oracle ref` against stand-in LAMMPS headers
(tests/cpp/lammps_mock) with oracle/ref_driver.cpp around them.

TEST INFRASTRUCTURE ONLY, like pyoracle: `Reference` has the constructor, the compute() signature and the result keys
of pyoracle.Oracle, so a test can swap judges.  The library exists only where the reference's sources are (or where a
build elsewhere left it in oracle/_ref/, which is git-ignored): ask available() first.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, "_ref", "libmtp_ref.so")
_LIB = None
_N = 4096


def reference_dir():
    return os.environ.get("MTP_REFERENCE_DIR", "/root/reference/LAMMPS/ML-MTP")


def have_sources():
    return os.path.isfile(os.path.join(reference_dir(), "pair_mtp.cpp"))


def build():
    """make -C oracle ref (needs the reference's sources)"""
    import sys
    subprocess.check_call(["make", "-s", "-C", _HERE, "ref", "MTP_REFERENCE_DIR=" + reference_dir(),
                           "PYTHON=" + sys.executable])


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(_PATH)
        L.mtp_ref_open.restype = C.c_void_p
        L.mtp_ref_open.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                   C.c_char_p, C.c_int]
        L.mtp_ref_close.argtypes = [C.c_void_p]
        L.mtp_ref_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.mtp_ref_init_one.restype = C.c_double
        L.mtp_ref_init_one.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.mtp_ref_set_extrapolation_flag.argtypes = [C.c_void_p, C.c_int]
        L.mtp_ref_extract_peratom.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
        L.mtp_ref_compute.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_long] + \
            [C.c_void_p] * 9 + [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        L.mtp_ref_write_config.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_long,
                                           C.c_void_p]
        _LIB = L
    return _LIB


def available():
    """True when oracle/_ref/libmtp_ref.so can be loaded"""
    if not os.path.exists(_PATH):
        return False
    try:
        lib()
        return True
    except OSError:
        return False


class ReferenceError_(RuntimeError):
    """what the reference's error->one / error->all (or a C++ exception of its reader) said"""


def _a(a):
    return None if a is None else a.ctypes.data


class Reference:
    """One potential file in the reference's pair style; `selection` chooses `mtp/extrapolation`.
    mlip3 = (cfg_path, select_threshold, break_threshold) as strings gives the four-argument MLIP-3 form."""

    def __init__(self, path, selection=False, mlip3=None):
        self.log = ""
        self.h = None
        log, err = C.create_string_buffer(_N), C.create_string_buffer(_N)
        style = 2 if mlip3 else (1 if selection else 0)
        a = [os.fsencode(v) for v in mlip3] if mlip3 else [None, None, None]
        self.selection = bool(selection or mlip3)
        self.mlip3 = bool(mlip3)
        h = lib().mtp_ref_open(style, os.fsencode(path), a[0], a[1], a[2], log, _N, err, _N)
        self.log = log.value.decode()
        if not h:
            raise ReferenceError_(err.value.decode())
        self.h = h
        iv, dv = (C.c_int * 10)(), (C.c_double * 3)()
        lib().mtp_ref_sizes(h, iv, dv)
        self._sizes = dict(zip(("Sp", "R", "Mu", "A", "B", "T", "S", "P", "C"), list(iv)[:9]))
        if not self.selection:
            s = self._sizes
            s["C"] = s["Sp"] * s["Sp"] * s["Mu"] * s["R"] + s["Sp"] + s["S"]
        self.configuration_mode = iv[9] if self.selection else 0
        self.scaling, self.min_cutoff, self.max_cutoff = dv[0], dv[1], dv[2]

    def __del__(self):
        try:
            if self.h:
                lib().mtp_ref_close(self.h)
                self.h = None
        except Exception:
            pass

    close = __del__

    @property
    def sizes(self):
        return dict(self._sizes)

    def init_one(self, i, j):
        err = C.create_string_buffer(_N)
        v = lib().mtp_ref_init_one(self.h, i, j, err, _N)
        if err.value:
            raise ReferenceError_(err.value.decode())
        return v

    def set_extrapolation_flag(self, on):
        """what `fix pair` does through extract("extrapolation_flag"); False when the style has no such flag"""
        return bool(lib().mtp_ref_set_extrapolation_flag(self.h, int(on)))

    def extract_peratom(self):
        """ncol of extract_peratom("extrapolation"); None when the style has none; raises what the style raises"""
        ncol, err = C.c_int(-1), C.create_string_buffer(_N)
        rc = lib().mtp_ref_extract_peratom(self.h, C.byref(ncol), err, _N)
        if rc < 0:
            raise ReferenceError_(err.value.decode())
        return None if rc else ncol.value

    def compute(self, x, types, ilist, first, neigh, eflag=3, vflag=4, extrapolation=False, natoms=0, prefill=0.0,
                domain=None):
        """As pyoracle.Oracle.compute.  prefill: what energy, eatom, virial and vatom hold when the style is called (it
        zeroes what it tallies)."""
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        types = np.ascontiguousarray(types, dtype=np.int32)
        ilist = np.ascontiguousarray(ilist, dtype=np.int32)
        first = np.ascontiguousarray(first, dtype=np.int32)
        neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        nall = x.shape[0]
        f = np.zeros((nall, 3))
        eatom = np.full(nall, float(prefill))
        vatom = np.full((nall, 6), float(prefill))
        virial = np.full(6, float(prefill))
        e = np.full(1, float(prefill))
        grades = np.zeros(nall)
        mg = np.zeros(1)
        cd = np.zeros(max(1, self._sizes["C"]))
        dom = None if domain is None else np.ascontiguousarray(domain, dtype=np.float64)
        if self.selection:
            self.set_extrapolation_flag(bool(extrapolation))
        elif extrapolation:
            raise ValueError("opened without selection")
        log, err = C.create_string_buffer(_N), C.create_string_buffer(_N)
        rc = lib().mtp_ref_compute(self.h, nall, len(ilist), _a(ilist), _a(first), _a(neigh), _a(x), _a(types),
                                   eflag, vflag, int(natoms), _a(dom), _a(f), _a(e), _a(eatom), _a(virial), _a(vatom),
                                   _a(grades), _a(mg), _a(cd), log, _N, err, _N)
        self.log = log.value.decode()
        self.error = err.value.decode()
        if rc and not (self.mlip3 and "Exceeded Break Threshold" in self.error):
            raise ReferenceError_(self.error)
        out = dict(energy=float(e[0]), eatom=eatom, f=f, virial=virial, vatom=vatom)
        if extrapolation or self.mlip3:
            out.update(grades=grades, max_grade=float(mg[0]), coeff_ders=cd[:self._sizes["C"]].copy(),
                       pvector0=float(mg[0]))
        return out

    def write_config(self, x, types, grades, max_grade, natoms, domain):
        """one .cfg record from prescribed grades through the style's own write_config (MLIP-3 form)"""
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        types = np.ascontiguousarray(types, dtype=np.int32)
        grades = np.ascontiguousarray(grades, dtype=np.float64)
        dom = np.ascontiguousarray(domain, dtype=np.float64)
        if lib().mtp_ref_write_config(self.h, len(x), _a(x), _a(types), _a(grades), float(max_grade), int(natoms), _a(dom)):
            raise ReferenceError_("no preselected file")


def run_mlip3(path, cfg_path, select, brk, domain, x, types, ilist, first, neigh, eflag=3, vflag=4, natoms=None):
    """The MLIP-3 form end to end: settings with four arguments, thresholds, Domain fields, one compute.
    Returns dict(cfg=bytes of the preselected file, log=settings + compute log text, error=message or "", out=results)."""
    r = Reference(path, mlip3=(cfg_path, str(select), str(brk)))
    log = r.log
    out = r.compute(x, types, ilist, first, neigh, eflag, vflag, extrapolation=True,
                    natoms=len(ilist) if natoms is None else natoms, domain=domain)
    log += r.log
    error = r.error
    r.close()
    with open(cfg_path, "rb") as fh:
        cfg = fh.read()
    return dict(cfg=cfg, log=log, error=error, out=out)
