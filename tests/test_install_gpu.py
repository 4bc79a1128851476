"""Installing new coefficients and a new active set into a LIVE context (include/mtp_mi355x.h, "installing ...").

Context A is created on the committed file and then installed into; context B is created on the file that carries the
same values (capi.write_all_coeffs / capi.write_selection / Context.save) -- the reload route.  The exact check is
Context.coeff_tables_device(): what the kernels will read, copied back from device memory, A against B bit for bit.
Outputs are compared A against B and against the CPU oracle on the written file, per quantity within the project's
parity bound 1e-9 + 1e-10 max(1, max |reference|) (tests/_install.py, bound); tests/test_install_cpu.py asserts that the
perturbation moves the forces by at least 1e3 times that bound, so stale tables cannot pass.  Grades: the bound of the
existing grade tests (tests/test_gpu_baseline_configs.py), 1e-9 + 1e-9 max(1, max |reference|)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _batch   # noqa: E402
import _cells   # noqa: E402
from _cells import LIST_CUTOFF   # noqa: E402
from _install import POT, ROOT, bound, golden_cell, perturb, potential, write_perturbed   # noqa: E402

pytestmark = pytest.mark.gpu

_TMP = tempfile.TemporaryDirectory(prefix="install_")
ALL3 = ("radial", "species", "moments")
QUANTITIES = ("energy", "eatom", "f", "virial", "vatom")


@functools.lru_cache(maxsize=None)
def _written(name, blocks=ALL3):
    """(path, radial, species, moments): `name` with the blocks perturbed, written once and shared"""
    dst = os.path.join(_TMP.name, "%s_%s.mtp" % (name.split(".")[0], "_".join(blocks)))
    return (dst,) + write_perturbed(os.path.join(POT, name), dst, blocks=blocks)


@functools.lru_cache(maxsize=None)
def _oracle_on(path, name):
    """the oracle's outputs on the golden cell of `name` with the potential file `path` (computed once; read only)"""
    from oracle.pyoracle import Oracle
    s = golden_cell(name)
    return Oracle(path).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4)


def _same_tables(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray) or isinstance(b[k], np.ndarray):
            assert a[k] is not None and b[k] is not None and np.array_equal(a[k], b[k]), "%s %s" % (what, k)
        else:
            assert a[k] == b[k], "%s %s" % (what, k)


def _within(got, ref, what):
    for q in QUANTITIES:
        err = float(np.abs(np.asarray(got[q]) - np.asarray(ref[q])).max())
        print("%s %s: max abs err %.3e, bound %.3e" % (what, q, err, bound(ref[q])))
        assert err <= bound(ref[q]), "%s %s: %.3e > %.3e" % (what, q, err, bound(ref[q]))


def _listed(path, name, selection=False):
    s = golden_cell(name)
    ctx = capi.Context(potential(path, selection), 0)
    ctx.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    return ctx, s


# ---- 5. the tables, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalars_lds", ["0", "1"])
@pytest.mark.parametrize("name", ["W_L8.mtp", "W_L16.mtp", "WRe_L20.mtp"])
def test_installed_tables_equal_a_context_of_the_written_file(monkeypatch, name, scalars_lds):
    """level 8; level 16 (leaves, rows and scalars in LDS); level 20 (two species, gather form, leaf constants behind the
    rows) -- with the scalar-side tables forced out of and into the blob"""
    monkeypatch.setenv("MTP_SCALARS_LDS", scalars_lds)
    path, ra, sp, mo = _written(name)
    pot = potential(os.path.join(POT, name))
    th_file = pot.theta()
    a = capi.Context(pot, 0)
    before = a.coeff_tables_device()
    assert before["scalars_in_lds"] == (scalars_lds == "1") and (before["blob_seed_val"] is not None) == (scalars_lds == "1")
    host = pot.coeff_tables()
    for k in ("seed_val", "e_lin", "leaf_cf", "leaf_cb"):     # what creation uploaded is what the host tables say, in both copies
        assert np.array_equal(before["hbm_" + k], host[k])
        assert before["blob_" + k] is None or np.array_equal(before["blob_" + k], host[k])
    a.install_coeffs(ra, sp, mo)
    b = capi.Context(potential(path), 0)
    ta, tb = a.coeff_tables_device(), b.coeff_tables_device()
    _same_tables(ta, tb, name)
    assert not np.array_equal(ta["blob_radial"], before["blob_radial"]) and not np.array_equal(ta["hbm_leaf_cf"], before["hbm_leaf_cf"])
    assert np.array_equal(a.theta(), np.concatenate([ra, sp, mo])) and np.array_equal(b.theta(), a.theta())
    assert np.array_equal(pot.theta(), th_file) and not np.array_equal(a.theta(), th_file)   # the potential is not written
    # the file route into a live context, and Context.save as the writer
    a2 = capi.Context(pot, 0)
    a2.install_file(path)
    _same_tables(a2.coeff_tables_device(), tb, name + " install_file")
    if scalars_lds == "1":                                   # (one more load of the file: once per potential)
        saved = os.path.join(_TMP.name, "saved_%s" % name)
        a.save(saved)
        _same_tables(capi.Context(capi.Potential(saved), 0).coeff_tables_device(), tb, name + " save")


# ---- 6. outputs of A against B and against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", [None, "core", "tgt", "norows", "rows"])
@pytest.mark.parametrize("name", ["W_L16.mtp", "WRe_L20.mtp"])
def test_outputs_after_an_install_under_every_blob_prefix(monkeypatch, name, prefix):
    """each copy of the leaf constants and the scalar tables is the one a launch reads under at least one prefix"""
    if prefix is not None:
        monkeypatch.setenv("MTP_BLOB_PREFIX", prefix)
    _check_outputs(name)


def test_outputs_after_an_install_level8():
    _check_outputs("W_L8.mtp")


def _check_outputs(name, deterministic=False):
    path, ra, sp, mo = _written(name)
    a, s = _listed(os.path.join(POT, name), name)
    b, _ = _listed(path, name)
    if deterministic:
        a.set_deterministic(True)
        b.set_deterministic(True)
    old = a.compute(s.x, s.types)
    shape, plan, launch = a.last_shape(), a.plan_info(), a.launch_info()
    a.install_coeffs(ra, sp, mo)
    got, ref = a.compute(s.x, s.types), b.compute(s.x, s.types)
    assert (a.last_shape(), a.plan_info(), a.launch_info()) == (shape, plan, launch)
    assert (b.last_shape(), b.plan_info()) == (shape, plan)
    _within(got, ref, name + " A vs B")
    _within(got, _oracle_on(path, name), name + " A vs oracle")
    assert float(np.abs(got["f"] - old["f"]).max()) >= 1e3 * bound(ref["f"])          # (the install did change the forces)
    if deterministic:                                        # fixed-point force sums: two calls, and A and B, agree to the bit
        assert np.array_equal(a.compute(s.x, s.types)["f"], got["f"]) and np.array_equal(got["f"], ref["f"])
    return a, b, s, got


@pytest.mark.parametrize("name", ["W_L16.mtp", "WRe_L20.mtp"])
def test_outputs_after_an_install_deterministic_and_resident(name):
    import torch
    a, b, s, got = _check_outputs(name, deterministic=True)
    # the device-resident step (mtp_compute_resident) on A: totals and per-atom arrays of the installed values
    a.set_deterministic(False)
    dev = torch.device("cuda:0")
    st = capi.use_private_torch_stream(dev).cuda_stream
    x_t, t_t = torch.from_numpy(s.x).to(dev), torch.from_numpy(s.types).to(dev)
    f_t = torch.zeros((s.nall, 3), dtype=torch.float64, device=dev)
    L = capi.lib()
    a._check(L.mtp_compute_resident(a.h, C.c_void_p(st), capi._ptr(x_t), capi._ptr(t_t), capi._ptr(f_t), 3, 4, 0))
    ev7 = np.zeros(7)
    a._check(L.mtp_resident_totals(a.h, C.c_void_p(st), capi._np(ev7, C.c_double), None, None))
    eatom, vatom = np.zeros(s.nall), np.zeros((s.nall, 6))
    a._check(L.mtp_resident_peratom_host(a.h, C.c_void_p(st), 0, capi._np(eatom, C.c_double)))
    a._check(L.mtp_resident_peratom_host(a.h, C.c_void_p(st), 1, capi._np(vatom, C.c_double)))
    res = dict(energy=ev7[0], virial=ev7[1:], eatom=eatom, vatom=vatom, f=f_t.cpu().numpy())
    path = _written(name)[0]
    _within(res, b.compute(s.x, s.types), name + " resident A vs B")
    _within(res, _oracle_on(path, name), name + " resident A vs oracle")


# ---- 7. partial installs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", ALL3)
@pytest.mark.parametrize("name", ["W_L16.mtp", "WRe_L20.mtp"])
def test_one_block_installed_equals_the_file_with_that_block(name, block):
    path, ra, sp, mo = _written(name, (block,))
    a, s = _listed(os.path.join(POT, name), name)
    a.install_coeffs(**{"radial_coeffs": ra} if block == "radial" else {"species_coeffs": sp} if block == "species" else
                     {"moment_coeffs": mo})
    b, _ = _listed(path, name)
    _same_tables(a.coeff_tables_device(), b.coeff_tables_device(), "%s %s" % (name, block))
    assert np.array_equal(a.theta(), b.theta())
    got = a.compute(s.x, s.types)
    _within(got, b.compute(s.x, s.types), "%s %s A vs B" % (name, block))
    _within(got, _oracle_on(path, name), "%s %s A vs oracle" % (name, block))


# ---- 8. design and train after an install ---------------------------------------------------------------------------------------
def _small_cells(species=1):
    return [_cells.cubic2_cell(), _cells.tilted5_cell(species), _batch.sheared8_cell(species)]


def test_design_and_train_read_the_installed_radial_block():
    from lammps_mtp_kokkos_amd.md import design_cells, evaluate_cells, loss_cells
    name = "W_L16.mtp"
    path, ra, sp, mo = _written(name, ("radial",))
    cells = _small_cells()
    a = capi.Context(potential(os.path.join(POT, name)), 0)
    d_old = design_cells(a, cells, list_cutoff=LIST_CUTOFF)                # uploads the design kernel's radial block
    assert a.coeff_tables_device()["design_radial"] is not None
    a.install_coeffs(radial_coeffs=ra)
    b = capi.Context(potential(path), 0)
    da, db = design_cells(a, cells, list_cutoff=LIST_CUTOFF), design_cells(b, cells, list_cutoff=LIST_CUTOFF)
    _same_tables(a.coeff_tables_device(), b.coeff_tables_device(), "after design calls")
    for k in ("energy", "force", "virial"):
        xa, xb, xo = da[k].cpu().numpy(), db[k].cpu().numpy(), d_old[k].cpu().numpy()
        err = float(np.abs(xa - xb).max())
        print("design %s: max abs err %.3e, bound %.3e, moved by %.3e" % (k, err, bound(xb), np.abs(xa - xo).max()))
        assert err <= bound(xb) and float(np.abs(xa - xo).max()) >= 1e3 * bound(xb)
    labels = [dict(energy=r["energy"] + 0.01 * len(r["f"]), f=r["f"] + 0.02, virial=r["virial"] * 1.01)
              for r in evaluate_cells(b, cells, list_cutoff=LIST_CUTOFF)]
    la, lb = loss_cells(a, cells, labels, list_cutoff=LIST_CUTOFF), loss_cells(b, cells, labels, list_cutoff=LIST_CUTOFF)
    assert abs(la["loss"] - lb["loss"]) <= bound(lb["loss"])
    assert float(np.abs(la["grad"] - lb["grad"]).max()) <= bound(lb["grad"])
    stale = loss_cells(a, cells, labels, theta=a.pot.theta(), list_cutoff=LIST_CUTOFF)      # (the file's theta is another loss)
    assert abs(stale["loss"] - lb["loss"]) >= 1e3 * bound(lb["loss"])


# ---- 9. selection ------------------------------------------------------------------------------------------------------------------
def _grade_close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, tol = float(np.abs(got - want).max()), 1e-9 + 1e-9 * max(1.0, float(np.abs(want).max()))
    print("%s: max abs err %.3e, bound %.3e" % (what, err, tol))
    assert err <= tol, what


def _pool_cells(species):
    return [_cells.cubic2_cell(), _cells.tilted5_cell(species), _batch.sheared8_cell(species), _batch.carved(11, species)]


def _c622_file():
    """WRe_L20.mtp with a synthetic neighbourhood-mode selection state, made as tests/test_gpu_baseline_configs.py makes it"""
    dst = os.path.join(_TMP.name, "WRe_L20_nbh.almtp")
    if not os.path.exists(dst):
        rng = np.random.default_rng(17)
        S = 2.0 * np.eye(622) + 0.05 * rng.uniform(-1, 1, size=(622, 622))
        tail = ["#MVS_v1.1", "energy_weight = 0", "force_weight = 0", "stress_weight = 0", "site_en_weight = 1", "weight_scaling = 1"]
        data = open(os.path.join(POT, "WRe_L20.mtp"), "rb").read()
        data += ("\n".join(tail) + "\n").encode() + b"#" + S.astype("<f8").tobytes() + np.linalg.inv(S).astype("<f8").tobytes()
        open(dst, "wb").write(data)
    return dst


@pytest.mark.parametrize("which", ["W_L16_nbh.almtp", "WRe_L10_cfg.almtp", "c622"])
def test_installed_selection_grades_like_a_context_of_the_written_file(monkeypatch, which):
    """neighbourhood mode at cpad 160 (the LDS-staged MFMA grade kernel, the tiled copy), configuration mode, and C = 622
    (the generic grade kernel, the padded copy)"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, select_cells
    from oracle.pyoracle import Oracle
    if which == "c622":                                      # three level-20 loads: without the LDS-bank search (another numbering
        monkeypatch.setenv("MTP_NO_RENUMBER", "1")           # of the moments, the same results; read when a file is loaded)
    src = _c622_file() if which == "c622" else os.path.join(POT, which)
    pot = capi.Potential(src, selection=True)
    cfg_mode, C_ = bool(pot.info.configuration_mode), int(pot.info.coeff_count)
    cells = _pool_cells(int(pot.info.species_count))
    a = capi.Context(pot, 0)
    S0, W0 = a.selection()
    assert np.array_equal(S0, pot.active_set()) and np.array_equal(W0, pot.tables()["inverse_active_set"])
    sel = select_cells(a, cells, threshold=1.1, list_cutoff=LIST_CUTOFF, max_swaps=6 if which == "c622" else None)
    assert sel["nswaps"] >= 1
    t0 = a.coeff_tables_device()
    a.install_selection(sel["active_set"], sel["inverse_active_set"])
    out = os.path.join(_TMP.name, "sel_%s.almtp" % which)
    a.save(out)
    b = capi.Context(capi.Potential(out, selection=True), 0)
    ta = a.coeff_tables_device()
    _same_tables(ta, b.coeff_tables_device(), which)
    assert not np.array_equal(ta["ainv_pad"], t0["ainv_pad"]) and not np.array_equal(ta["ainv_tiled"], t0["ainv_tiled"])
    # nrows == 0: the installed blocks bit for bit
    import torch
    none = a.maxvol_select(torch.zeros((0, C_), dtype=torch.float64, device="cuda"), 1.1)
    assert np.array_equal(none["active_set"], sel["active_set"]) and np.array_equal(none["inverse_active_set"], sel["inverse_active_set"])
    # grades on A against B and against the oracle with the new W, fused and unfused
    orc = Oracle(out, selection=True)
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("MTP_GRADE_UNFUSED", "1")
        ga, gb = evaluate_cells(a, cells, list_cutoff=LIST_CUTOFF, grades=True), evaluate_cells(b, cells, list_cutoff=LIST_CUTOFF, grades=True)
        for k, (ra_, rb_, cell) in enumerate(zip(ga, gb, cells)):
            ow = _cells.oracle_cell(orc, *cell, list_cutoff=LIST_CUTOFF, extrapolation=True, natoms=len(cell[0]))[3]
            tag = "%s cfg %d%s" % (which, k, " unfused" if unfused else "")
            if cfg_mode:                                     # mtp_batch_cfg_grades; the oracle's max_grade is the configuration's
                _grade_close(ra_["cfg_grade"], rb_["cfg_grade"], tag + " cfg_grade A vs B")
                _grade_close(ra_["cfg_grade"], ow["max_grade"], tag + " cfg_grade A vs oracle")
            else:
                _grade_close(ra_["grades"], rb_["grades"], tag + " grades A vs B")
                _grade_close(ra_["grades"], ow["grades"][: len(cell[0])], tag + " grades A vs oracle")
    if cfg_mode:                                             # mtp_context_cfg_grade follows the new W, mtp_cfg_grade the file's
        s = golden_cell(which)
        a.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
        cd = a.compute(s.x, s.types, grade=True)["coeff_ders"]
        want = float(np.abs(sel["inverse_active_set"] @ cd).max())
        _grade_close(a.cfg_grade(cd), want, which + " context cfg_grade")
        _grade_close(pot.cfg_grade(cd), float(np.abs(W0 @ cd).max()), which + " potential cfg_grade")
        assert abs(a.cfg_grade(cd) - pot.cfg_grade(cd)) > 1e-6 * want
    # a second selection on A starts from the installed set, as on B: the same swap log
    again = _batch.mixed_batch(int(pot.info.species_count))[:5] if which != "c622" else cells[:2]
    sa = select_cells(a, again, threshold=1.05, list_cutoff=LIST_CUTOFF, max_swaps=4)
    sb = select_cells(b, again, threshold=1.05, list_cutoff=LIST_CUTOFF, max_swaps=4)
    assert [(i, j) for i, j, _ in sa["swaps"]] == [(i, j) for i, j, _ in sb["swaps"]]
    assert np.array_equal(sa["active_set"], sb["active_set"])


# ---- 10. refusals leave the context alone -----------------------------------------------------------------------------------------
def test_refused_installs_change_nothing():
    pot = potential(os.path.join(POT, "W_L16_nbh.almtp"), True)
    a = capi.Context(pot, 0)
    t0, th0, (S0, W0) = a.coeff_tables_device(), a.theta(), a.selection()
    t = pot.tables()
    C_ = pot.info.coeff_count

    def refused(code, call, *args, **kw):
        with pytest.raises(capi.MtpError) as e:
            call(*args, **kw)
        assert e.value.code == code, e.value
        _same_tables(a.coeff_tables_device(), t0, "after a refusal")
        assert np.array_equal(a.theta(), th0) and np.array_equal(a.selection()[0], S0) and np.array_equal(a.selection()[1], W0)

    for key in ("radial_coeffs", "species_coeffs", "moment_coeffs"):
        refused(-20, a.install_coeffs, **{key: np.zeros(t[key].size + 1)})
        for bad in (np.nan, np.inf):
            v = t[key].copy().reshape(-1)
            v[-1] = bad
            refused(-20, a.install_coeffs, **{key: v})
            # a good block beside a bad one: nothing of the good one may land
            good = {"radial_coeffs": t["radial_coeffs"] * 1.5}
            if key != "radial_coeffs":
                refused(-20, a.install_coeffs, **dict(good, **{key: v}))
    bad_W = W0.copy()
    bad_W[3, 4] = np.nan
    refused(-20, a.install_selection, S0, bad_W)
    refused(-20, a.install_selection, bad_W, W0)
    refused(-20, a.install_selection, S0[:-1, :-1], W0[:-1, :-1])
    refused(-20, a.install_selection, np.zeros((C_ + 1, C_ + 1)), np.zeros((C_ + 1, C_ + 1)))
    refused(-6, a.install_file, os.path.join(POT, "W_L8.mtp"))
    refused(-6, a.install_file, os.path.join(POT, "WRe_L10_cfg.almtp"))
    refused(-2, a.install_file, os.path.join(_TMP.name, "no_such_file.mtp"))
    nan_file = os.path.join(_TMP.name, "nan.almtp")          # a compatible file whose values are refused: nothing lands
    data = open(os.path.join(POT, "W_L16_nbh.almtp"), "rb").read()
    k = data.index(b"moment_coeffs = {") + len(b"moment_coeffs = {")
    open(nan_file, "wb").write(data[:k] + b"nan, " + data[data.index(b",", k) + 1:])
    refused(-20, a.install_file, nan_file)
    # a tail that is there but does not read is the parser's error: no quiet install of the coefficients alone
    k = data.index(b"#MVS_v1.1")
    new_text = open(_written("W_L16.mtp")[0], "rb").read()     # other coefficients, the structure of this potential
    for tag, tail in (("version", data[k:].replace(b"#MVS_v1.1", b"#MVS_v1.0", 1)),
                      ("weight", data[k:].replace(b"stress_weight", b"stres_weight", 1)),
                      ("short", data[k: k + 300])):
        path = os.path.join(_TMP.name, "damaged_%s.almtp" % tag)
        open(path, "wb").write(new_text + tail)
        refused(-2 if tag == "short" else -8, a.install_file, path)
    # ... while a file with no tail at all installs its coefficients and keeps the set
    a3 = capi.Context(pot, 0)
    a3.install_file(_written("W_L16.mtp")[0])
    assert np.array_equal(a3.theta(), np.concatenate(_written("W_L16.mtp")[1:]))
    assert np.array_equal(a3.selection()[1], W0) and np.array_equal(a3.coeff_tables_device()["ainv_pad"], t0["ainv_pad"])
    # a selection into a context whose potential was loaded without its selection state
    plain = capi.Context(capi.Potential(os.path.join(POT, "W_L16_nbh.almtp")), 0)
    p0 = plain.coeff_tables_device()
    with pytest.raises(capi.MtpError) as e:
        plain.install_selection(S0, W0)
    assert e.value.code == -23
    with pytest.raises(capi.MtpError) as e:
        plain.selection()
    assert e.value.code == -23
    _same_tables(plain.coeff_tables_device(), p0, "plain")
    assert p0["ainv_pad"] is None and p0["ainv_tiled"] is None


# ---- 10b. two scalars on one leaf moment: the two-table blob layout and the refusal of the one-table layout ------------------------
def test_leaf_constants_of_a_shared_scalar_moment(tmp_path):
    """tests/_mutate.py, dup_mapping: the last scalar is mapped onto the moment of the first never-read scalar, so
    leaf_cf = mult (c_first + c_last) and leaf_cb = mult c_last.  A context created on such a file holds TWO leaf tables in
    its blob and an install writes both; one created on the file with c_first = 0 holds ONE table for both (the values are
    equal), and an install that makes them differ is refused with MTP_ERR_UNSUPPORTED and changes nothing."""
    from _mutate import mutate_mtp
    from oracle.pyoracle import Oracle
    name = "W_L16.mtp"
    mut = str(tmp_path / "dup.mtp")
    info = mutate_mtp(os.path.join(POT, name), mut, late_writer=False, dup_mapping=True)
    pot = capi.Potential(mut)
    t = pot.tables()
    first = int(np.flatnonzero(t["alpha_moment_mapping"] == info["dup_moment"])[0])
    assert first < len(t["alpha_moment_mapping"]) - 1 and t["alpha_moment_mapping"][-1] == info["dup_moment"]
    ra, sp, mo = perturb(t)
    new = str(tmp_path / "dup_new.mtp")
    capi.write_all_coeffs(mut, new, mo, sp, ra)
    s = golden_cell(name)
    # two tables: installed against a context of the written file and the oracle
    a, b = capi.Context(pot, 0), capi.Context(capi.Potential(new), 0)
    ta0 = a.coeff_tables_device()
    assert not np.array_equal(ta0["blob_leaf_cf"], ta0["blob_leaf_cb"]) and not np.array_equal(ta0["hbm_leaf_cf"], ta0["hbm_leaf_cb"])
    a.install_coeffs(ra, sp, mo)
    ta = a.coeff_tables_device()
    _same_tables(ta, b.coeff_tables_device(), "dup_mapping")
    assert not np.array_equal(ta["blob_leaf_cf"], ta["blob_leaf_cb"]) and not np.array_equal(ta["blob_leaf_cb"], ta0["blob_leaf_cb"])
    for c in (a, b):
        c.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
    got = a.compute(s.x, s.types)
    _within(got, b.compute(s.x, s.types), "dup_mapping A vs B")
    _within(got, Oracle(new).compute(s.x, s.types, s.ilist, s.first, s.neigh, eflag=3, vflag=4), "dup_mapping A vs oracle")
    # one table: the same file with a zero first coefficient
    mo_zero = t["moment_coeffs"].copy()
    mo_zero[first] = 0.0
    zero = str(tmp_path / "dup_zero.mtp")
    capi.write_all_coeffs(mut, zero, mo_zero, t["species_coeffs"], t["radial_coeffs"])
    z = capi.Context(capi.Potential(zero), 0)
    tz = z.coeff_tables_device()
    assert np.array_equal(tz["blob_leaf_cf"], tz["blob_leaf_cb"]) and np.array_equal(tz["hbm_leaf_cf"], tz["hbm_leaf_cb"])
    th = z.theta()
    with pytest.raises(capi.MtpError) as e:
        z.install_coeffs(ra, sp, mo)                           # c_first != 0: the two constants would differ
    assert e.value.code == -6
    _same_tables(z.coeff_tables_device(), tz, "after the refusal")
    assert np.array_equal(z.theta(), th)
    keep = mo.copy()                                         # values that keep the two constants equal are installed
    keep[first] = 0.0
    z.install_coeffs(ra, sp, keep)
    kept = str(tmp_path / "dup_keep.mtp")
    capi.write_all_coeffs(mut, kept, keep, sp, ra)
    _same_tables(z.coeff_tables_device(), capi.Context(capi.Potential(kept), 0).coeff_tables_device(), "zero first coefficient")


# ---- 11. two contexts on one Potential ----------------------------------------------------------------------------------------------
def test_an_install_stays_in_its_context():
    name = "W_L16.mtp"
    path, ra, sp, mo = _written(name)
    pot = potential(os.path.join(POT, name))
    s = golden_cell(name)
    a, other = capi.Context(pot, 0), capi.Context(pot, 0)
    for c in (a, other):
        c.set_neighbors(s.ilist, s.first, s.neigh, s.nall)
        c.set_deterministic(True)
    t0, th0, out0 = other.coeff_tables_device(), pot.theta(), other.compute(s.x, s.types)
    a.install_coeffs(ra, sp, mo)
    _same_tables(other.coeff_tables_device(), t0, "the other context")
    out1 = other.compute(s.x, s.types)
    for q in QUANTITIES:
        assert np.array_equal(out1[q], out0[q]) if q == "f" else np.abs(np.asarray(out1[q]) - np.asarray(out0[q])).max() <= bound(out0[q]), q
    assert np.array_equal(pot.theta(), th0) and np.array_equal(other.theta(), th0) and not np.array_equal(a.theta(), th0)
    _within(a.compute(s.x, s.types), _oracle_on(path, name), "the installed context")


# ---- 12. the loop without a reload ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radial_installed", [False, True])
def test_fit_linear_installs_its_result(tmp_path, radial_installed):
    """radial_installed: teacher and student run on a radial block that is not the file's, so fit_linear's out_path has to
    carry the CONTEXT's radial block (capi.write_all_coeffs) for the written file to be the refitted model"""
    from lammps_mtp_kokkos_amd.md import evaluate_cells, fit_linear
    src = os.path.join(POT, "W_L8.mtp")
    cells = [_cells.cubic2_cell(), _cells.tilted5_cell(1), _batch.sheared8_cell(), _batch.carved(16)]
    assert [len(c[0]) for c in cells] == [2, 5, 8, 16]
    pot = capi.Potential(src)
    teacher, student = capi.Context(pot, 0), capi.Context(pot, 0)
    radial = pot.tables()["radial_coeffs"]
    if radial_installed:
        radial = perturb(pot.tables(), seed=9, rel=0.05)[0]
        teacher.install_coeffs(radial_coeffs=radial)
        student.install_coeffs(radial_coeffs=radial)
    want = evaluate_cells(teacher, cells, list_cutoff=LIST_CUTOFF)
    labels = [dict(energy=r["energy"], f=r["f"], virial=r["virial"]) for r in want]
    t = pot.tables()
    _, sp, mo = perturb(t, seed=5, rel=0.05)
    student.install_coeffs(species_coeffs=sp, moment_coeffs=mo)
    off = evaluate_cells(student, cells, list_cutoff=LIST_CUTOFF)
    assert max(float(np.abs(o["f"] - w["f"]).max()) for o, w in zip(off, want)) > 1e-3
    out = str(tmp_path / "refit.mtp")
    res = fit_linear(student, cells, labels, out_path=out, list_cutoff=LIST_CUTOFF, install=True)
    assert res["wrote"] == 0                                  # (no #MVS tail in the source: nothing was left out, by either writer)
    assert np.array_equal(student.theta(), np.concatenate([radial.reshape(-1), res["species_coeffs"], res["moment_coeffs"]]))
    back = capi.Potential(out).tables()                      # the written file is the student's model, radial block included
    assert np.array_equal(back["radial_coeffs"], radial.reshape(-1)) and np.array_equal(back["moment_coeffs"], res["moment_coeffs"])
    assert np.array_equal(back["radial_coeffs"], t["radial_coeffs"]) == (not radial_installed)
    got = evaluate_cells(student, cells, list_cutoff=LIST_CUTOFF)
    reload_ = evaluate_cells(capi.Context(capi.Potential(out), 0), cells, list_cutoff=LIST_CUTOFF)
    rm = res["rmse_after"]
    print("rmse after", rm, "before", res["rmse_before"])
    for g, w, r, c in zip(got, want, reload_, cells):
        n = len(c[0])
        # the residual solve_linear reports is an rms over the labelled rows: no single row exceeds rms x sqrt(rows)
        assert abs(g["energy"] - w["energy"]) / n <= rm["energy"] * np.sqrt(len(cells)) + bound(w["energy"])
        assert float(np.abs(g["f"] - w["f"]).max()) <= rm["force"] * np.sqrt(3 * 31) + bound(w["f"])
        assert float(np.abs(g["virial"] - w["virial"]).max()) / n <= rm["virial"] * np.sqrt(6 * len(cells)) + bound(w["virial"])
        for q in ("energy", "f", "virial"):                  # ... and the reload route gives the same numbers
            assert float(np.abs(np.asarray(g[q]) - np.asarray(r[q])).max()) <= bound(r[q]), q
    ts, tr = student.coeff_tables_device(), capi.Context(capi.Potential(out), 0).coeff_tables_device()
    assert np.array_equal(ts.pop("design_radial"), ts["blob_radial"]) and tr.pop("design_radial") is None   # (only the student made a design call)
    _same_tables(ts, tr, "refit")


# ---- 13. the host mirror: pair_style re-issued on a running mirror ------------------------------------------------------------------
def _write_system(path, s):
    assert np.array_equal(s.ilist, np.arange(s.nlocal))
    with open(path, "w") as fh:
        fh.write("%d %d 0 0 0\n" % (s.nlocal, s.nall))
        for (x, y, z), t in zip(s.x, s.types):
            fh.write("%.17g %.17g %.17g %d\n" % (x, y, z, t))
        for i in range(s.nlocal):
            row = s.neigh[s.first[i]:s.first[i + 1]]
            fh.write("%d %s\n" % (len(row), " ".join(map(str, row))))


def _read_snapshots(path, nall):
    lines = open(path).read().split("\n")
    head = [float(v) for v in lines[0].split()]
    out = []
    for k in range(2):
        rows = lines[1 + k * (nall + 1): 1 + (k + 1) * (nall + 1)]
        tot = np.array([float(v) for v in rows[0].split()])
        per = np.array([[float(v) for v in r.split()] for r in rows[1:]])
        out.append(dict(energy=tot[0], virial=tot[1:7], pv=tot[7], f=per[:, :3], eatom=per[:, 3], vatom=per[:, 4:10]))
    return head, out[0], out[1]


@pytest.mark.parametrize("mode", ["plain", "ext"])
def test_pair_style_reissued_installs_a_compatible_file(tmp_path, mode):
    """settings -> init_style -> compute -> settings with a retrained file -> compute: the same context object, no new
    neighbour list, the numbers of a mirror freshly constructed on that file; for the extrapolation style pvector[0]
    follows the new W.  A file of another structure takes the full load."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_pair_install")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lammps_mtp_kokkos_amd", "host"), "pair_install"])
    if mode == "plain":
        name, src = "W_L16.mtp", os.path.join(POT, "W_L16.mtp")
        new, other = _written(name)[0], os.path.join(POT, "W_L8.mtp")
    else:
        name, src = "WRe_L10_cfg.almtp", os.path.join(POT, "WRe_L10_cfg.almtp")
        C_ = capi.Potential(src).info.coeff_count
        rng = np.random.default_rng(23)
        S = 2.0 * np.eye(C_) + 0.3 * rng.uniform(-1, 1, (C_, C_))
        new, other = str(tmp_path / "new_set.almtp"), os.path.join(POT, "W_L16_nbh.almtp")
        capi.write_selection(src, new, S, np.linalg.inv(S))
    s = golden_cell(name)
    sysfile, out = str(tmp_path / "system.txt"), str(tmp_path / "out.txt")
    _write_system(sysfile, s)
    r = subprocess.run([exe, mode, sysfile, out, src, new, other], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # the reference's two log lines on every read: three reads by the first mirror, one by the fresh one
    assert r.stdout.count("The scaling is") == 4 and r.stdout.count(" species.") == 4, r.stdout
    head, installed, fresh = _read_snapshots(out, s.nall)
    same, installs, ctx_after, installs_after, computed, pv_before = head
    assert same == 1 and installs == 1                       # the context handle is the same object
    assert ctx_after == 0 and installs_after == 1 and computed == 0      # the full load: a new context, a new list needed
    for q in QUANTITIES:
        err = float(np.abs(installed[q] - fresh[q]).max())
        print("%s %s: installed vs fresh %.3e, bound %.3e" % (mode, q, err, bound(fresh[q])))
        assert err <= bound(fresh[q]), q
    if mode == "plain":
        ref = _oracle_on(new, name)
        for q in QUANTITIES:
            assert float(np.abs(installed[q] - np.asarray(ref[q])).max()) <= bound(ref[q]), q
    else:
        _grade_close(installed["pv"], fresh["pv"], "pvector[0] installed vs fresh")
        assert abs(installed["pv"] - pv_before) > 1e-6 * abs(fresh["pv"])         # pvector[0] follows the new W
