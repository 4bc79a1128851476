"""One randomised GPU-vs-oracle parity case: random level, species count, density (one to three 32-neighbour
tiles), ragged subset lists, grade calls and all three LDS layouts.  Shared by tests/test_gpu_fuzz.py (fixed seeds, part
of `pytest -m gpu`) and scripts/fuzz_parity.py (open-ended sweeps).  fuzz_star_case is the same along the geometry axis:
disjoint stars (tests/_stars.py) with a random multiset of (in-cutoff count, row length)."""
import os

import numpy as np

from lammps_mtp_kokkos_amd import capi, mtpgen
from lammps_mtp_kokkos_amd.driver import periodic_system


def fuzz_case(rng, tmpdir, tag="p"):
    """Runs one case; returns (description, dict of relative errors F / E / V / G)."""
    from oracle.pyoracle import Oracle
    level = int(rng.choice([6, 8, 10, 12, 14, 16, 18]))
    species = int(rng.integers(1, 4))
    a = float(rng.choice([3.165, 2.9, 2.6, 2.3]))
    cells = tuple(int(v) for v in rng.integers(2, 5, 3))
    grade = bool(rng.integers(0, 2)) and species <= 2
    plan = str(rng.choice(["keep", "lean", "rebuild"]))
    tab = mtpgen.level8_template() if level == 8 else mtpgen.build_table(level)
    pot_d = mtpgen.random_potential(tab, species, int(rng.integers(1, 10 ** 6)))
    if grade:
        mtpgen.add_selection_state(pot_d, "nbh", seed=int(rng.integers(1, 1000)))
    path = os.path.join(str(tmpdir), "%s.almtp" % tag)
    mtpgen.write_mtp(pot_d, path)
    pos, box = mtpgen.bcc_lattice(*cells, a=a, jitter=0.08, seed=int(rng.integers(1, 10 ** 6)))
    types = rng.integers(1, species + 1, len(pos)).astype(np.int32)
    s = periodic_system(pos, box, types, 6.5)
    # ragged: a random subset of the owned atoms as ilist, their full rows
    keep = np.sort(rng.choice(s.nlocal, max(1, int(s.nlocal * rng.uniform(0.5, 1.0))), replace=False)).astype(np.int32)
    first = np.zeros(len(keep) + 1, np.int32)
    first[1:] = np.cumsum(s.first[keep + 1] - s.first[keep])
    neigh = np.concatenate([s.neigh[s.first[i]:s.first[i + 1]] for i in keep]) if len(keep) else np.zeros(0, np.int32)
    wps = str(rng.choice([2, 3]))          # register build (3 only exists for the narrow lane grids: ignored elsewhere)
    old, old_w = os.environ.get("MTP_LAYOUT"), os.environ.get("MTP_WPS")
    os.environ["MTP_LAYOUT"] = plan
    os.environ["MTP_WPS"] = wps
    try:
        pot = capi.Potential(path, selection=grade)
        ctx = capi.Context(pot, 0)
        ctx.set_neighbors(keep, first, neigh, s.nall)
        got = ctx.compute(s.x, s.types, eflag=3, vflag=4, grade=grade)
    finally:
        for k, v in (("MTP_LAYOUT", old), ("MTP_WPS", old_w)):
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    want = Oracle(path, selection=grade).compute(s.x, s.types, keep, first, neigh, extrapolation=grade,
                                                 natoms=len(keep))
    scale = max(1.0, np.abs(want["f"]).max())
    err = dict(F=np.abs(got["f"] - want["f"]).max() / scale,
               E=abs(got["energy"] - want["energy"]) / max(1.0, abs(want["energy"])),
               V=np.abs(got["virial"] - want["virial"]).max() / max(1.0, np.abs(want["virial"]).max()),
               G=0.0)
    if grade:
        err["G"] = np.abs(got["grades"][keep] - want["grades"][keep]).max() / max(1.0, np.abs(want["grades"][keep]).max())
    mx = int(np.diff(first).max()) if len(keep) else 0
    desc = "level %2d species %d a %.3f cells %s rows %4d maxrow %3d grade %d layout %s wps %s" % (
        level, species, a, cells, len(keep), mx, grade, plan, wps)
    return desc, err


def fuzz_star_case(rng, tmpdir, tag="s"):
    """One case on disjoint stars: random (K, L) multiset around the tile and sweep edges, row order, shell range, level,
    layout, register build and grade call, compared per star (_stars.per_star_check asserts the tolerance).  Returns
    (description, dict of worst error / per-star tolerance)."""
    from oracle.pyoracle import Oracle
    import _stars
    level = int(rng.choice([6, 8, 10, 12, 14, 16, 18, 20]))
    species = int(rng.integers(1, 3))
    grade = bool(rng.integers(0, 2))
    plan = str(rng.choice(["keep", "lean", "rebuild"]))
    wps = str(rng.choice([2, 3]))
    order = str(rng.choice(_stars.ORDERS))
    rlo = float(rng.choice([1.0, 1.6, 2.1, 3.0]))
    special = "edge" if rng.integers(0, 3) == 0 else None
    tab = mtpgen.level8_template() if level == 8 else mtpgen.build_table(level)
    pot_d = mtpgen.random_potential(tab, species, int(rng.integers(1, 10 ** 6)))
    if grade:
        mtpgen.add_selection_state(pot_d, "nbh", seed=int(rng.integers(1, 1000)))
    path = os.path.join(str(tmpdir), "%s.almtp" % tag)
    mtpgen.write_mtp(pot_d, path)
    nstar = int(rng.integers(40, 400))
    near = np.array([0, 32, 64, 96, 128])
    K = np.where(rng.random(nstar) < 0.6, np.abs(rng.choice(near, nstar) + rng.integers(-2, 6, nstar)), rng.integers(0, 131, nstar))
    extra = np.where(rng.random(nstar) < 0.5, rng.choice([0, 1, 2], nstar), rng.integers(0, 180, nstar))
    L = np.where(rng.random(nstar) < 0.3, np.maximum(K, rng.choice([64, 127, 128, 129, 256, 257], nstar)), K + extra)
    KL = [(int(k), int(l)) for k, l in zip(K, L)]
    st = _stars.stars(KL, rng, species=species, rin=(rlo, 5.0), order=order, special=special)
    assert _stars.counts(st) == KL
    old, old_w = os.environ.get("MTP_LAYOUT"), os.environ.get("MTP_WPS")
    os.environ["MTP_LAYOUT"] = plan
    os.environ["MTP_WPS"] = wps
    try:
        pot = capi.Potential(path, selection=grade)
        ctx = capi.Context(pot, 0)
        ctx.set_neighbors(st.ilist, st.first, st.neigh, st.nall)
        got = ctx.compute(st.x, st.types, eflag=3, vflag=4, grade=grade)
    finally:
        for k, v in (("MTP_LAYOUT", old), ("MTP_WPS", old_w)):
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    want = Oracle(path, selection=grade).compute(st.x, st.types, st.ilist, st.first, st.neigh, extrapolation=grade,
                                                 natoms=len(KL))
    desc = "stars %3d level %2d species %d order %-8s shell from %.1f %s grade %d layout %s wps %s" % (
        nstar, level, species, order, rlo, "exact-cutoff" if special else "plain", grade, plan, wps)
    return desc, _stars.per_star_check(st, got, want, grade, False, desc)
