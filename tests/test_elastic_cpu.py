"""Batched elastic constants, the host side (md.elastic_cells, md.relax_ions, md.moduli, md.stress_correction, md.to_voigt;
include/mtp_mi355x.h, "batched elastic constants"): the numpy twin of tests/_elastic.py on two analytic solids, the host-only
functions against closed forms, the ionic term on a chain of alternating springs, and the refusals that must come before a
pointer or the device is touched.  No GPU."""
import ctypes as C
import types

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi, md

import _cells
import _elastic

CELL = np.array([[6.4, 0.0, 0.0], [2.1, 5.9, 0.0], [-1.7, 1.3, 6.2]])


# ---- the twin on analytic solids ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [0.005, 0.02])
def test_the_twin_recovers_a_solid_whose_stress_is_linear_in_the_strain(h):
    """two configurations (5 and 70 atoms) and an empty one between them, each with its own C, sigma, Lambda and slot origin:
    stress, birch = C + K(sigma), elastic = C and the coupling come back to rounding over h, the B - B^T identity holds to
    rounding, and after the pass the positions are the saved ones to the bit"""
    solids = [_elastic.LinearSolid(5, 1, CELL), None, _elastic.LinearSolid(70, 2, 2.0 * CELL)]
    sizes = [5, 0, 70]
    first = np.concatenate([[0], np.cumsum(sizes)])
    origins = np.array([[3.0, -2.0, 1.0], [0.0, 0.0, 0.0], [40.0, 7.0, -11.0]])
    h0 = np.array([CELL.reshape(9), np.eye(3).reshape(9), (2.0 * CELL).reshape(9)])
    x = np.concatenate([s.pos + origins[j] for j, s in enumerate(solids) if s is not None])

    def model(x):
        e, f, W = np.zeros(len(x)), np.zeros((len(x), 3)), np.zeros((3, 6))
        for j, s in enumerate(solids):
            if s is not None:
                a, b = first[j], first[j + 1]
                e[a:b], f[a:b], W[j] = s(x[a:b], origins[j])
        return e, f, W

    x_before = x.copy()
    twin = _elastic.Twin(first, h).run(x, origins, h0, model)
    assert np.array_equal(x, x_before) and not twin.status.any()
    assert np.array_equal(twin.T[[0, 2]], np.tile(np.eye(3).reshape(9), (2, 1))) and not twin.T[1].any()   # (an empty one is skipped)
    for j in (0, 2):
        s = solids[j]
        tol = 1e-12 * np.abs(s.B).max() / h
        err = dict(stress=np.abs(twin.stress0[j] - s.sigma).max(), birch=np.abs(twin.B[j] - s.B).max(),
                   elastic=np.abs(twin.C[j] - s.C).max(), coupling=np.abs(twin.lam(j) - s.Lam).max(),
                   identity=np.abs((twin.B[j] - twin.B[j].T) - (np.outer(_elastic.DVEC, s.sigma) - np.outer(s.sigma, _elastic.DVEC))).max())
        print("h %g, configuration %d: %s, asymmetry %.3e, sum rule %.3e (tolerance %.3e)"
              % (h, j, ", ".join("%s %.2e" % kv for kv in err.items()), twin.diag[j, 0], twin.diag[j, 1], tol))
        assert max(err.values()) <= tol and twin.diag[j, 0] <= 2.0 * tol and twin.diag[j, 1] <= 70 * tol
        assert np.abs(twin.B[j] - twin.B[j].T).max() > 0.1                # (the raw asymmetry is no rounding matter)
        assert np.abs(twin.f0[first[j]: first[j + 1]] - s.f0).max() <= 1e-12 and twin.energy[j] != 0.0
    assert not twin.B[1].any() and not twin.diag[1].any() and twin.fmax[1] == 0.0


def test_the_elastic_constants_are_the_second_derivatives_with_respect_to_lagrangian_strain():
    """a solid whose energy is EXACTLY quadratic in the Lagrangian strain, E = V0 (S : eta + eta : C : eta / 2): its Cauchy stress
    is not linear in the small strain, so B carries an O(h^2) error -- but `elastic` must converge to the given C and `stress` to
    S, which is what Wallace's correction and its sign are for.  The error falls by four when h is halved."""
    Cm, S = _elastic.random_constants(5)
    V0 = float(np.linalg.det(CELL))
    pos = np.random.default_rng(0).random((4, 3)) @ CELL
    errs = []
    for h in (0.004, 0.002):
        calls = [0]

        def model(x):
            k = calls[0] - 1
            calls[0] += 1
            D = np.eye(3) if k < 0 or k >= 12 else _elastic.strain_of(k, h)[2]
            return np.zeros(4), np.zeros((4, 3)), _elastic.hyperelastic_virial(Cm, S, V0, D)[None]

        twin = _elastic.Twin([0, 4], h).run(pos.copy(), np.zeros((1, 3)), CELL.reshape(1, 9), model)
        assert np.abs(twin.stress0[0] - S).max() <= 1e-14 * np.abs(S).max() * 10
        errs.append(float(np.abs(twin.C[0] - Cm).max()))
        # without the correction the matrix is off by the stress itself
        assert np.abs(0.5 * (twin.B[0] + twin.B[0].T) - Cm).max() > 0.1 * np.abs(S).max()
    print("|elastic - C| at h = 0.004, 0.002: %.3e, %.3e (|C|max %.2f, |S|max %.2f)" % (errs[0], errs[1], np.abs(Cm).max(), np.abs(S).max()))
    assert errs[0] < 1e-3 * np.abs(Cm).max() and 3.5 < errs[0] / errs[1] < 4.5


def test_a_poisoned_number_fails_its_configuration_only_in_the_twin():
    solids = [_elastic.LinearSolid(4, 3, CELL), _elastic.LinearSolid(6, 4, CELL)]
    first, origins, h0 = np.array([0, 4, 10]), np.array([[0.0, 0.0, 0.0], [30.0, 0.0, 0.0]]), np.tile(CELL.reshape(9), (2, 1))

    def model(x):
        parts = [s(x[first[j]: first[j + 1]], origins[j]) for j, s in enumerate(solids)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.array([p[2] for p in parts])

    x = np.concatenate([s.pos + origins[j] for j, s in enumerate(solids)])
    clean = _elastic.Twin(first, 0.01).run(x.copy(), origins, h0, model)
    for nan_at in ((0, "w", 1, 2), (3, "f", 5, 0), (4, "w", 1, 5)):
        xx = x.copy()
        twin = _elastic.Twin(first, 0.01).run(xx, origins, h0, model, nan_at=nan_at)
        assert list(twin.status) == [0, _elastic.FAILED] and np.array_equal(xx, x)
        assert np.array_equal(twin.B[0], clean.B[0]) and np.array_equal(twin.C[0], clean.C[0]) and not twin.B[1].any()
        done = {0: 0, 3: 1, 4: 1}[nan_at[0]]                                   # rows completed before the failure
        assert not twin.Bt[1, done + 1:].any() and all(twin.Bt[1, w].any() for w in range(done))


# ---- host-only functions ----------------------------------------------------------------------------------------------------

def test_stress_correction_and_to_voigt():
    s = np.array([0.11, -0.23, 0.31, 0.05, -0.07, 0.13])
    K = md.stress_correction(s)
    assert np.array_equal(K, _elastic.correction(s))
    d = _elastic.DVEC
    assert np.abs((K - K.T) - (np.outer(d, s) - np.outer(s, d))).max() <= 1e-16
    # hydrostatic stress sigma = -p I: K = p (d d^T - 2 I_eng), the textbook B_ijkl = C_ijkl + p (d_ij d_kl - d_ik d_jl - d_il d_jk)
    p = 0.37
    want = p * np.outer(d, d) - p * np.diag([2.0, 2.0, 2.0, 1.0, 1.0, 1.0])
    assert np.abs(md.stress_correction(-p * d) - want).max() <= 1e-16
    assert md.VOIGT == (0, 1, 2, 5, 4, 3)
    assert np.array_equal(md.to_voigt(np.arange(6.0)), [0, 1, 2, 5, 4, 3])
    M = np.arange(36.0).reshape(6, 6)
    V = md.to_voigt(M)
    assert V[3, 3] == M[5, 5] and V[5, 5] == M[3, 3] and V[0, 3] == M[0, 5] and V[4, 4] == M[4, 4] and V[3, 5] == M[5, 3]
    for bad in (np.zeros(5), np.zeros((6, 5)), np.zeros((3, 3))):
        with pytest.raises(ValueError, match="to_voigt"):
            md.to_voigt(bad)
    with pytest.raises(ValueError, match="stress_correction"):
        md.stress_correction(np.zeros((3, 3)))


def test_moduli_against_closed_forms_and_its_refusals():
    lam, mu = 1.3, 0.7                                                         # isotropic: Voigt = Reuss = Hill
    Ci = np.zeros((6, 6))
    Ci[:3, :3] = lam
    Ci[range(3), range(3)] += 2.0 * mu
    Ci[range(3, 6), range(3, 6)] = mu
    m = md.moduli(Ci)
    for key, want in (("bulk_voigt", lam + 2.0 * mu / 3.0), ("bulk_reuss", lam + 2.0 * mu / 3.0), ("bulk_hill", lam + 2.0 * mu / 3.0),
                      ("shear_voigt", mu), ("shear_reuss", mu), ("shear_hill", mu), ("compressibility", 1.0 / (lam + 2.0 * mu / 3.0))):
        assert abs(m[key] - want) <= 1e-14 * want, key
    assert m["born_stable"] is True and abs(m["min_eigenvalue"] - mu) <= 1e-14
    c11, c12, c44 = 3.26, 1.26, 1.0                                            # cubic
    Cc = np.zeros((6, 6))
    Cc[:3, :3] = c12
    Cc[range(3), range(3)] = c11
    Cc[range(3, 6), range(3, 6)] = c44
    m = md.moduli(Cc)
    K = (c11 + 2.0 * c12) / 3.0
    gv, gr = (c11 - c12 + 3.0 * c44) / 5.0, 5.0 * (c11 - c12) * c44 / (4.0 * c44 + 3.0 * (c11 - c12))
    for key, want in (("bulk_voigt", K), ("bulk_reuss", K), ("shear_voigt", gv), ("shear_reuss", gr), ("shear_hill", 0.5 * (gv + gr)),
                      ("compressibility", 1.0 / K)):
        assert abs(m[key] - want) <= 1e-14 * want, key
    assert m["born_stable"] and gr < gv
    assert md.moduli(md.to_voigt(Cc)) == m                                     # (the same in either order)
    Cu = Cc.copy()
    Cu[range(3), range(3)] = 1.0                                               # c11 < c12: the tetragonal shear is unstable
    assert md.moduli(Cu)["born_stable"] is False
    nan = Cc.copy()
    nan[2, 3] = np.nan
    for bad in (nan, np.zeros((6, 5)), np.zeros(6), np.zeros((6, 6))):
        with pytest.raises(ValueError, match="moduli"):
            md.moduli(bad)


def _chain(k1, k2, cells=3, a=2.0):
    """a periodic chain along x of 2 * cells atoms at spacing a / 2 with springs k1, k2 in turn (and weak ties along y and z so
    that only the translations are null): H, the coupling of the strain xx, the clamped C11 and the volume (unit cross-section)"""
    n = 2 * cells
    H = np.zeros((3 * n, 3 * n))
    Lam = np.zeros((6, 3 * n))
    b = 0.5 * a
    for i in range(n):
        j, k = (i + 1) % n, (k1 if i % 2 == 0 else k2)
        for d, kd in ((0, k), (1, 0.3), (2, 0.2)):
            H[3 * i + d, 3 * i + d] += kd
            H[3 * j + d, 3 * j + d] += kd
            H[3 * i + d, 3 * j + d] -= kd
            H[3 * j + d, 3 * i + d] -= kd
        # a strain eps stretches bond (i, j) by b eps: the force on i is +k b eps, on j it is -k b eps
        Lam[0, 3 * i] += k * b
        Lam[0, 3 * j] -= k * b
    V = cells * a
    C = np.zeros((6, 6))
    C[0, 0] = n * 0.5 * (k1 + k2) * b * b / V                                  # sum over the bonds of k b^2, per volume
    return H, Lam, C, V


def test_relax_ions_on_a_chain_of_alternating_springs():
    """clamped, every bond takes the strain: the stiffness is that of the mean spring (k1 + k2) / 2.  Relaxed, the two bonds of a
    cell are in series: 2 k1 k2 / (k1 + k2)."""
    k1, k2 = 3.0, 0.5
    H, Lam, C, V = _chain(k1, k2)
    assert abs(C[0, 0] - 0.5 * (k1 + k2)) <= 1e-15                             # (n b^2 / V = b = 1 with a = 2)
    r = md.relax_ions(C, C, Lam, H, V)
    want = 2.0 * k1 * k2 / (k1 + k2)
    print("clamped %.6f, relaxed %.6f (series value %.6f)" % (C[0, 0], r["elastic_relaxed"][0, 0], want))
    assert r["status"] == "ok" and abs(r["elastic_relaxed"][0, 0] - want) <= 1e-13
    assert abs(r["birch_relaxed"][0, 0] - want) <= 1e-13 and np.abs(r["elastic_relaxed"][1:, 1:]).max() <= 1e-14
    assert np.abs(r["internal_strain"].reshape(6, -1, 3).sum(1)).max() <= 1e-13     # no net translation
    assert np.abs(H @ r["internal_strain"][0] - Lam[0]).max() <= 1e-13              # H U = Lambda^T on the complement
    # equal springs: nothing relaxes
    H1, L1, C1, V1 = _chain(1.7, 1.7)
    r1 = md.relax_ions(C1, C1, L1, H1, V1)
    assert np.abs(r1["elastic_relaxed"] - C1).max() <= 1e-14 and np.abs(r1["internal_strain"]).max() <= 1e-14
    # the translations are projected: a rigid shift in the right-hand sides changes nothing
    shift = Lam + np.tile([0.4, -0.2, 0.1], Lam.shape[1] // 3)[None, :] * np.arange(1, 7)[:, None]
    r2 = md.relax_ions(C, C, shift, H, V)
    U0 = r["internal_strain"]
    assert np.abs(r2["internal_strain"] - U0).max() <= 1e-13 and np.abs(r2["elastic_relaxed"] - r["elastic_relaxed"]).max() <= 1e-13
    # a given U is used as it is
    r3 = md.relax_ions(C, C, Lam, H, V, internal_strain=U0)
    assert np.array_equal(r3["elastic_relaxed"], r["elastic_relaxed"])
    # a negative mode
    Hn = H.copy()
    Hn[1, 1] -= 2.0
    Hn[4, 4] -= 2.0
    Hn[1, 4] += 2.0
    Hn[4, 1] += 2.0
    rn = md.relax_ions(C, C, Lam, Hn, V)
    assert rn["status"] == "unstable" and np.isnan(rn["elastic_relaxed"]).all() and np.isnan(rn["internal_strain"]).all()
    for kw in (dict(B=np.zeros((6, 5))), dict(coupling=Lam[:, :-1]), dict(hessian=H[:-3, :-3]), dict(volume=0.0), dict(volume=float("nan"))):
        a = dict(B=C, C=C, coupling=Lam, hessian=H, volume=V)
        a.update(kw)
        with pytest.raises(ValueError, match="relax_ions"):
            md.relax_ions(**a)


# ---- refusals before a device is touched -------------------------------------------------------------------------------------

def test_the_entry_points_refuse_bad_arguments_before_touching_a_pointer():
    """every pointer is a made-up address: a call that got past the checks would crash here"""
    L = capi.lib()
    assert all(n in capi.EXPORTS for n in ("mtp_elastic_step", "mtp_elastic_finish", "mtp_elastic_relax"))
    assert capi.ELASTIC_STATUS == ("ok", "failed", "unstable") and capi.ELASTIC_RELAX_MAX_N >= 162
    p = C.c_void_p(4096)

    def step(stream=p, ncfg=3, k=0, h=0.005, null=None):
        ptrs = [None if i == null else p for i in range(18)]
        return L.mtp_elastic_step(stream, ncfg, ptrs[0], k, C.c_double(h), *ptrs[1:])

    def finish(stream=p, ncfg=3, null=None):
        return L.mtp_elastic_finish(stream, ncfg, *[None if i == null else p for i in range(9)])

    def relax(stream=p, ncfg=3, null=None):
        return L.mtp_elastic_relax(stream, ncfg, *[None if i == null else p for i in range(12)])

    for fn in (step, finish, relax):
        assert fn(stream=None) == -20 and fn(ncfg=-1) == -20 and fn(ncfg=0) == 0
    for h in (0.0, -0.005, float("nan"), float("inf")):
        assert step(h=h) == -20
    assert step(k=-1) == -20 and step(k=13) == -20 and step(ncfg=0, k=12) == 0
    for fn, count in ((step, 18), (finish, 9), (relax, 12)):
        for i in range(count):
            assert fn(null=i) == -20, (fn.__name__, i)


def _stub(max_cutoff=5.0):
    """what elastic_cells reads of a context before it plans: anything past the host checks fails on it with AttributeError"""
    return types.SimpleNamespace(pot=types.SimpleNamespace(info=types.SimpleNamespace(max_cutoff=max_cutoff)))


def test_elastic_cells_refuses_before_it_touches_the_device():
    cfg = _cells.tilted5_cell()
    cases = {
        "h 0": dict(h=0.0), "h < 0": dict(h=-0.005), "h nan": dict(h=float("nan")), "h inf": dict(h=float("inf")),
        "h at half the skin over the cutoff": dict(h=1.0 / 7.0), "h above it": dict(h=0.2),
        "h_atoms 0": dict(h_atoms=0.0), "h_atoms nan": dict(h_atoms=float("nan")), "h_atoms at half the skin": dict(h_atoms=1.0),
    }
    for what, kw in cases.items():
        with pytest.raises(ValueError, match="elastic_cells") as ei:
            md.elastic_cells(_stub(), [cfg], **kw)
        print(what, "->", ei.value)
    with pytest.raises(ValueError, match="configuration 0"):
        md.elastic_cells(_stub(), [cfg], relax_ions=True, max_hessian_bytes=8 * 15 * 15 - 1)
    for kw in (dict(h=0.1428), dict(h_atoms=0.999), dict(relax_ions=True, max_hessian_bytes=8 * 15 * 15)):   # just inside
        with pytest.raises(AttributeError):
            md.elastic_cells(_stub(), [cfg], **kw)
