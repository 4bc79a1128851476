"""mtp_halo_force_step -- the call a multi-GPU driver makes once per MD step -- at the size, parity, image-count, split and
flag edges of tests/_halo_step.py, through the RCCL self-exchange of one rank whose only peer is itself.

The reference is the oracle on x_all = [x_own, x_own[send_idx] + send_shift] with the ghost forces folded by np.add.at
(tests/test_halo_step_cpu.py checks that model against the single-box route).  Tolerances are the suite's own
(tests/test_gpu_halo.py, tests/test_gpu_shapes.py::_check).  Every call runs on one private stream; each geometry has one
halo (one communicator), destroyed when the module is through."""
import functools
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi

import _halo_step as hs
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POT = os.path.join(ROOT, "potentials")
NAN = float("nan")
SENTINEL = -7.25e11            # what a buffer nobody may write holds
PAD = 4                        # sentinel doubles behind the 3 nall of f


class Rig:
    """one geometry: plan, halo with a communicator of its own, the module's stream"""
    stream = None

    def __init__(self, name):
        import torch
        self.name = name
        self.plan = hs.plan(name)
        self.dev = torch.device("cuda:0")
        if Rig.stream is None:
            Rig.stream = capi.use_private_torch_stream(self.dev)
        self.st = self.stream.cuda_stream
        self.halo = capi.Halo(self.plan, 0, capi.halo_unique_id())
        self.x_own = hs.positions(self.plan)
        self.types = torch.from_numpy(self.plan.types).to(self.dev)

    def close(self):
        self.stream.synchronize()
        capi.lib().mtp_halo_destroy(self.halo.h)
        self.halo.h = None


_rigs = {}


@pytest.fixture(scope="module", autouse=True)
def _halos_are_destroyed():
    yield
    for r in _rigs.values():
        r.close()
    _rigs.clear()


@pytest.fixture
def rig(request):
    """the rig of one geometry (indirect parameter), made when first asked for and kept until the module is through"""
    if request.param not in _rigs:
        _rigs[request.param] = Rig(request.param)
    return _rigs[request.param]


def on(*names):
    return pytest.mark.parametrize("rig", list(names), indirect=True)


_pots = {}


def _pot(name, grade=False):
    if (name, grade) not in _pots:
        _pots[name, grade] = capi.Potential(os.path.join(POT, name), selection=grade)
    return _pots[name, grade]


@functools.lru_cache(maxsize=None)
def _want(name, potential, eflag=3, vflag=1, grade=False):
    """the model of the step for a geometry at its standard positions: computed once, shared, read-only"""
    from oracle.pyoracle import Oracle
    p = hs.plan(name)
    return hs.model_step(Oracle(os.path.join(POT, potential), selection=grade), p, hs.positions(p), eflag, vflag, grade)


def _context(rig, potential, order="natural", grade=False, deterministic=False):
    """a context with the plan's list installed in the given row order -> (ctx, (na, nb, nc))"""
    import torch
    p = rig.plan
    ctx = capi.Context(_pot(potential, grade), 0)
    if deterministic:
        ctx.set_deterministic(True)
    ilist, first, neigh, split = hs.order_of(p, order)
    il, fi, ne = (torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(rig.dev) for a in (ilist, first, neigh))
    ctx.set_neighbors_device(il, fi, ne, p.nall, int(np.diff(first).max()))
    return ctx, split


class Buffers:
    """x with stale (NaN) ghost rows, f with PAD sentinel doubles behind it, eatom, ev"""

    def __init__(self, rig):
        import torch
        p, dev = rig.plan, rig.dev
        self.rig = rig
        self.x = torch.from_numpy(np.concatenate([rig.x_own, np.full((p.nghost, 3), NAN)])).to(dev)
        self.fbuf = torch.full((3 * p.nall + PAD,), SENTINEL, dtype=torch.float64, device=dev)
        self.f = self.fbuf[: 3 * p.nall].view(p.nall, 3)
        self.ea = torch.full((p.nall,), SENTINEL, dtype=torch.float64, device=dev)
        self.ev = torch.zeros(8, dtype=torch.float64, device=dev)

    def stale(self):
        """before EACH call: NaN in all of f and in the ghost rows of x, the sentinel in eatom"""
        self.f.fill_(NAN)
        self.x[self.rig.plan.nlocal:] = NAN
        self.ea.fill_(SENTINEL)

    def forces(self):
        """f after a call, with everything around it checked: ghost positions bit-equal to owner + shift, owned
        positions untouched, no NaN in f, the doubles behind f untouched"""
        p = self.rig.plan
        self.rig.stream.synchronize()
        x = self.x.cpu().numpy()
        assert np.array_equal(x[: p.nlocal], self.rig.x_own)
        assert np.array_equal(x[p.nlocal:], hs.ghosts_of(p, self.rig.x_own))
        fb = self.fbuf.cpu().numpy()
        assert np.array_equal(fb[3 * p.nall:], np.full(PAD, SENTINEL)), "the zeroing ran past 3 nall"
        f = fb[: 3 * p.nall].reshape(p.nall, 3)
        assert np.isfinite(f).all(), "%d entries of f are not finite" % int((~np.isfinite(f)).sum())
        return f


def _force_tol(F):
    return 1e-9 + 1e-10 * max(1.0, float(np.abs(F).max()))


def _check_forces(p, f, want, what):
    err = float(np.abs(f[: p.nlocal] - want["f"]).max())
    # the ghost rows of f hold what the force kernel left there (the reverse halo reads them, it does not clear them)
    gerr = float(np.abs(f[p.nlocal:] - want["f_all"][p.nlocal:]).max()) if p.nghost else 0.0
    print("%s: forces %.3e, ghost rows %.3e (bound %.3e)" % (what, err, gerr, _force_tol(want["f"])))
    assert err <= _force_tol(want["f"]) and gerr <= _force_tol(want["f"]), what


def _check_ev(p, ev, want, times, what):
    """ev[0] and ev[1:7] against `times` x the reference (the tallies accumulate over calls)"""
    E, V = times * want["energy"], times * want["virial"]
    de, dv = abs(ev[0] - E), float(np.abs(ev[1:7] - V).max())
    print("%s: energy %.3e, virial %.3e" % (what, de, dv))
    assert de <= 1e-10 * p.nlocal * max(1.0, abs(E) / p.nlocal), what
    assert dv <= 1e-8 + 1e-10 * np.abs(V).max(), what
    assert ev[7] == 0.0


def _check_eatom(p, ea, want):
    assert np.abs(ea[: p.nlocal] - want["eatom"][: p.nlocal]).max() <= 1e-10
    assert np.array_equal(ea[p.nlocal:], np.full(p.nghost, SENTINEL))      # per-atom energies are the centre's


ALL = ("pack_odd_tiny", "pack_even_tiny", "pack_even_two_species", "pack_odd_split", "zero_odd", "zero_even") + hs.CLUSTERS
TWO_SPECIES = {"pack_even_two_species": "WRe_L20.mtp"}


# ---- (a) every geometry, both schedules ---------------------------------------------------------------------------


def _values(rig, potential, overlap):
    p = rig.plan
    rig.halo.set_overlap(overlap)
    assert rig.halo.overlap == overlap
    ctx, split = _context(rig, potential)
    want = _want(rig.name, potential)
    b = Buffers(rig)
    for call in (1, 2):                       # the second call on the same buffers, ev NOT zeroed in between
        b.stale()
        rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, eatom_t=b.ea, ev_t=b.ev, stream=rig.st)
        f = b.forces()
        what = "%s %s overlap=%d call %d" % (rig.name, potential, overlap, call)
        _check_forces(p, f, want, what)
        _check_eatom(p, b.ea.cpu().numpy(), want)
        _check_ev(p, b.ev.cpu().numpy(), want, call, what)


@pytest.mark.parametrize("overlap", [False, True])
@on(*ALL)
def test_step_against_the_oracle(rig, overlap):
    """W_L8 (the two-species box: WRe_L20) on every geometry: f is NaN, the ghost rows of x are NaN and eatom holds a
    sentinel before each of two calls; owned forces, ghost forces, eatom, energy and virial equal the reference, the
    tallies of the second call add onto the first's, the ghost positions are bit-equal to owner + shift, and the four
    doubles behind f are untouched."""
    _values(rig, TWO_SPECIES.get(rig.name, "W_L8.mtp"), overlap)


@pytest.mark.parametrize("overlap", [False, True])
@on("pack_even_tiny", "zero_even")
def test_step_against_the_oracle_level_16(rig, overlap):
    _values(rig, "W_L16.mtp", overlap)


# ---- (b) split edges of the overlapped schedule -------------------------------------------------------------------


SPLITS = [("pack_odd_tiny", "natural"), ("pack_even_tiny", "natural"), ("pack_odd_split", "empty_first"),
          ("pack_odd_split", "empty_last"), ("no_ghosts_even", "empty_middle"), ("no_ghosts_odd", "empty_middle")]


@pytest.mark.parametrize("rig,order", SPLITS, indirect=["rig"])
def test_overlapped_split_edges(rig, order):
    """Overlapped schedule with an empty launch somewhere: (0, n, 0) of the tiny boxes (every owned atom has a ghost in
    its row: the middle launch folds the tallies), boundary | interior (empty first launch), interior | boundary (empty
    last launch) and, on the clusters, where no row has a ghost in it, (n/2, 0, n - n/2) (empty middle launch).  A
    boundary row cannot go into the first or the last launch -- they run beside the exchanges -- so the empty middle
    launch needs a plan without boundary rows.  Same values as the one-stream schedule (forces 1e-11, ev 1e-8, as
    tests/test_gpu_halo.py compares its two schedules), and the oracle's."""
    p = rig.plan
    ctx, split = _context(rig, "W_L8.mtp", order)
    assert 0 in split
    want = _want(rig.name, "W_L8.mtp")
    got = {}
    for overlap in (False, True):
        rig.halo.set_overlap(overlap)
        b = Buffers(rig)
        b.stale()
        rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, eatom_t=b.ea, ev_t=b.ev, stream=rig.st)
        f = b.forces()
        what = "%s %s %s overlap=%d" % (rig.name, order, split, overlap)
        _check_forces(p, f, want, what)
        _check_ev(p, b.ev.cpu().numpy(), want, 1, what)
        _check_eatom(p, b.ea.cpu().numpy(), want)
        got[overlap] = (f, b.ev.cpu().numpy())
    assert np.abs(got[True][0] - got[False][0]).max() < 1e-11 and np.abs(got[True][1] - got[False][1]).max() < 1e-8


# ---- (c) the unpack with up to 26 images of one owner -------------------------------------------------------------


@on("pack_even_tiny", "pack_odd_tiny")
def test_reverse_adds_every_image_onto_its_owner(rig):
    """halo.reverse on random f: 17 (4x4x5 cells) and 26 (4x4x4) ghost rows land on one address.  Against np.add.at only
    the order of an owner's m + 1 additions differs, so each component agrees to (m + 1) 2^-53 sum |terms|; the ghost
    rows stay as they were, bit for bit.  (The fused fold of the step is checked by test_step_against_the_oracle.)"""
    import torch
    p = rig.plan
    f_np = np.random.default_rng(4).normal(size=(p.nall, 3))
    f = torch.from_numpy(f_np.copy()).to(rig.dev)
    rig.halo.reverse(f, rig.st)
    rig.stream.synchronize()
    got = f.cpu().numpy()
    err, bound = np.abs(got[: p.nlocal] - hs.fold(p, f_np)), hs.unpack_bound(p, f_np)
    print("%s: %d images at most, worst err / bound %.3f" % (rig.name, hs.images(p).max(), (err / bound).max()))
    assert (err <= bound).all()
    assert np.array_equal(got[p.nlocal:], f_np[p.nlocal:])


# ---- (d) flags ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("overlap", [False, True])
@on("pack_even_two_species", "zero_odd")
def test_flags_through_the_step(rig, overlap):
    """eflag = vflag = 0 without an ev array (fold = 0 in mtp_ev_finish_unpack), eflag = 2 alone, vflag = 4 with per-atom
    virials, then the 3 / 1 call again: the tallies it folds hold one call's worth, whatever ran before.  The two-species
    box has random types, the ghosts' from the plan."""
    import torch
    p = rig.plan
    potential = TWO_SPECIES.get(rig.name, "W_L8.mtp")
    rig.halo.set_overlap(overlap)
    ctx, split = _context(rig, potential)
    want = _want(rig.name, potential)
    b = Buffers(rig)
    kw = dict(stream=rig.st)
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, eatom_t=b.ea, ev_t=b.ev, **kw)
    f31 = b.forces()
    _check_forces(p, f31, want, "3/1")
    _check_ev(p, b.ev.cpu().numpy(), want, 1, "3/1")
    # no global energy, no virial, no ev array: the forces of the 3/1 call, and the ev of that call is left alone
    b.ev.fill_(SENTINEL)
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=0, vflag=0, **kw)
    f00 = b.forces()
    assert np.abs(f00 - f31).max() < 1e-11
    assert np.array_equal(b.ev.cpu().numpy(), np.full(8, SENTINEL))
    assert np.array_equal(b.ea.cpu().numpy(), np.full(p.nall, SENTINEL))
    # per-atom energies alone
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=2, vflag=0, eatom_t=b.ea, **kw)
    f20 = b.forces()
    assert np.abs(f20 - f31).max() < 1e-11
    _check_eatom(p, b.ea.cpu().numpy(), want)
    assert np.array_equal(b.ev.cpu().numpy(), np.full(8, SENTINEL))
    # per-atom virials: the reference tallies on the central atom, so ghost rows stay zero
    want4 = _want(rig.name, potential, 0, 4)
    va = torch.zeros((p.nall, 6), dtype=torch.float64, device=rig.dev)
    b.ev.zero_()
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=0, vflag=4, vatom_t=va, ev_t=b.ev, **kw)
    f04 = b.forces()
    assert np.abs(f04 - f31).max() < 1e-11
    vah = va.cpu().numpy()
    _close(vah[: p.nlocal], want4["vatom"][: p.nlocal], "vatom")
    assert not vah[p.nlocal:].any() and not want4["vatom"][p.nlocal:].any()
    evh = b.ev.cpu().numpy()
    assert evh[0] == 0.0 and np.abs(evh[1:7] - want4["virial"]).max() <= 1e-8 + 1e-10 * np.abs(want4["virial"]).max()
    # ... and nothing of the calls above is left in the tally slots
    b.ev.zero_()
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, eatom_t=b.ea, ev_t=b.ev, **kw)
    _check_forces(p, b.forces(), want, "3/1 again")
    _check_ev(p, b.ev.cpu().numpy(), want, 1, "3/1 again")


# ---- (e) grades through the step ----------------------------------------------------------------------------------


@on("pack_odd_tiny")
def test_neighbourhood_grades_through_the_step(rig):
    """W_L16_nbh on the (0, n, 0) box in both schedules: grades of the owned atoms and max_grade against the oracle"""
    import torch
    p = rig.plan
    potential = "W_L16_nbh.almtp"
    ctx, split = _context(rig, potential, grade=True)
    assert split == (0, p.nlocal, 0)
    want = _want(rig.name, potential, 3, 1, True)
    for overlap in (False, True):
        rig.halo.set_overlap(overlap)
        b = Buffers(rig)
        gr = torch.full((p.nall,), SENTINEL, dtype=torch.float64, device=rig.dev)
        mg = torch.zeros(1, dtype=torch.float64, device=rig.dev)
        b.stale()
        rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, grade=True, eatom_t=b.ea, ev_t=b.ev, grades_t=gr,
                            maxg_t=mg, stream=rig.st)
        _check_forces(p, b.forces(), want, "grades overlap=%d" % overlap)
        _check_ev(p, b.ev.cpu().numpy(), want, 1, "grades overlap=%d" % overlap)
        g = gr.cpu().numpy()
        scale = max(1.0, want["max_grade"])
        assert np.abs(g[: p.nlocal] - want["grades"][: p.nlocal]).max() <= 1e-9 * scale
        assert np.array_equal(g[p.nlocal:], np.full(p.nghost, SENTINEL))
        assert abs(float(mg.item()) - want["max_grade"]) <= 1e-9 * scale


@on("pack_odd_split")
def test_configuration_coeff_ders_through_the_step(rig):
    """WRe_L10_cfg: coeff_ders, zeroed before the call, is the oracle's with natoms = nlocal -- from one launch in the
    one-stream schedule, summed over three in the overlapped one (4 | 242 | 4 rows)"""
    import torch
    p = rig.plan
    potential = "WRe_L10_cfg.almtp"
    ctx, split = _context(rig, potential, grade=True)
    assert min(split) > 0
    want = _want(rig.name, potential, 3, 1, True)
    got = {}
    for overlap in (False, True):
        rig.halo.set_overlap(overlap)
        b = Buffers(rig)
        cd = torch.zeros(_pot(potential, True).info.coeff_count, dtype=torch.float64, device=rig.dev)
        b.stale()
        rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, grade=True, eatom_t=b.ea, ev_t=b.ev, coeff_t=cd,
                            stream=rig.st)
        _check_forces(p, b.forces(), want, "cfg overlap=%d" % overlap)
        got[overlap] = cd.cpu().numpy()
        _close(got[overlap], want["coeff_ders"], "coeff_ders overlap=%d" % overlap, atol=1e-9, rtol=1e-10)
    _close(got[True], got[False], "coeff_ders of three launches against one", atol=1e-9, rtol=1e-10)
    assert np.abs(want["coeff_ders"]).max() > 1.0


# ---- (f) deterministic context ------------------------------------------------------------------------------------


@pytest.mark.parametrize("overlap", [False, True])
@on("bcc8_cut7", "pack_even_tiny")
def test_deterministic_context(rig, overlap):
    """Deterministic mode converts its fixed-point scratch after every row launch and the unpack then adds on top.  The
    step's forces are within the force tolerance of a plain deterministic call on x_all folded on the host, and a plain
    deterministic call on the step's context afterwards is bit-equal to one on a fresh context: the step left the
    scratch clean.  Two force_step calls are NOT asked to agree bit for bit: the unpack's atomic adds onto an owner with
    several images land in any order."""
    import torch
    p = rig.plan
    rig.halo.set_overlap(overlap)
    ctx, split = _context(rig, "W_L16.mtp", deterministic=True)
    fresh, _ = _context(rig, "W_L16.mtp", deterministic=True)
    xa = torch.from_numpy(hs.x_all(p, rig.x_own)).to(rig.dev)
    plain = {}
    b = Buffers(rig)
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, ev_t=b.ev, stream=rig.st)
    f = b.forces()
    for key, c in (("step", ctx), ("fresh", fresh)):
        fp = torch.zeros((p.nall, 3), dtype=torch.float64, device=rig.dev)
        c.compute_device(xa, rig.types, fp, stream=rig.st)
        c.synchronize(rig.st)
        plain[key] = fp.cpu().numpy()
    assert np.array_equal(plain["step"], plain["fresh"])
    F = hs.fold(p, plain["fresh"])
    err = float(np.abs(f[: p.nlocal] - F).max())
    print("%s overlap=%d: step against the folded plain call %.3e" % (rig.name, overlap, err))
    assert err <= _force_tol(F)
    _check_forces(p, f, _want(rig.name, "W_L16.mtp"), "deterministic")


# ---- (g) a rank without ghosts ------------------------------------------------------------------------------------


@pytest.mark.parametrize("overlap", [False, True])
@on(*hs.CLUSTERS)
def test_rank_without_ghosts(rig, overlap):
    """nsend = nghost = 0 (both parities of 3 nlocal): two empty RCCL groups, no unpack work; the step is the plain call,
    and forward / reverse change nothing"""
    import torch
    p = rig.plan
    rig.halo.set_overlap(overlap)
    ctx, split = _context(rig, "W_L8.mtp")
    want = _want(rig.name, "W_L8.mtp")
    b = Buffers(rig)
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, eatom_t=b.ea, ev_t=b.ev, stream=rig.st)
    f = b.forces()
    _check_forces(p, f, want, rig.name)
    _check_ev(p, b.ev.cpu().numpy(), want, 1, rig.name)
    fp = torch.zeros((p.nall, 3), dtype=torch.float64, device=rig.dev)
    ctx.compute_device(b.x, rig.types, fp, stream=rig.st)
    ctx.synchronize(rig.st)
    assert np.abs(f - fp.cpu().numpy()).max() < 1e-11
    before_x, before_f = b.x.clone(), b.f.clone()
    rig.halo.forward(b.x, rig.st)
    rig.halo.reverse(b.f, rig.st)
    rig.stream.synchronize()
    assert torch.equal(b.x, before_x) and torch.equal(b.f, before_f)


# ---- (h) refusals launch nothing ----------------------------------------------------------------------------------


def _refused(call, code, f, text=None):
    """`call` raises MtpError `code` and the sentinel-filled f is bit-unchanged: nothing was launched"""
    import torch
    torch.cuda.synchronize()
    with pytest.raises(capi.MtpError) as e:
        call()
    torch.cuda.synchronize()
    assert e.value.code == code, str(e.value)
    if text:
        assert text in str(e.value)
    assert bool((f == SENTINEL).all()), "a refused call wrote f"


REFUSALS = ["misaligned_f", "negative_rows", "null_type", "short_split", "long_split", "energy_without_ev", "virial_without_ev",
            "vatom_without_ev", "no_list", "grades_without_selection", "nbh_grades_without_array", "cfg_without_coeff_ders"]
GRADE_CASES = {"nbh_grades_without_array": "W_L16_nbh.almtp", "cfg_without_coeff_ders": "WRe_L10_cfg.almtp"}


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("case", REFUSALS)
@on("pack_odd_tiny")
def test_refusals_launch_nothing(rig, case, overlap):
    """The step refuses ahead of its first launch: a misaligned f, a negative row count, no type array, a split that does
    not add up to the installed list's rows (short or long), a call that needs the tally fold without an ev array, a
    context without a list, and the grade refusals of the force call (no selection state, neighbourhood grades without a
    grades array, configuration mode without coeff_ders).  f keeps its sentinel, the ghost rows of x stay stale, ev
    stays zero, the message says what was wrong, and a correct call on the same objects goes through afterwards."""
    import torch
    p, n = rig.plan, rig.plan.nlocal
    rig.halo.set_overlap(overlap)
    potential = GRADE_CASES.get(case, "W_L8.mtp")
    grade = case in GRADE_CASES
    ctx, split = _context(rig, potential, grade=grade)
    want = _want(rig.name, potential, 3, 1, grade)
    b = Buffers(rig)
    b.f.fill_(SENTINEL)
    step = rig.halo.force_step
    kw = dict(eflag=3, vflag=1, eatom_t=b.ea, ev_t=b.ev, stream=rig.st)
    no_ev = dict(eatom_t=b.ea, stream=rig.st)
    gr = torch.zeros(p.nall, dtype=torch.float64, device=rig.dev)
    mg = torch.zeros(1, dtype=torch.float64, device=rig.dev)
    cd = torch.zeros(_pot(potential, grade).info.coeff_count, dtype=torch.float64, device=rig.dev)
    good = dict(kw)
    if case == "nbh_grades_without_array":
        good.update(grade=True, grades_t=gr, maxg_t=mg)
    elif case == "cfg_without_coeff_ders":
        good.update(grade=True, coeff_t=cd)
    if case == "misaligned_f":
        off = torch.full((3 * p.nall + 2,), SENTINEL, dtype=torch.float64, device=rig.dev)
        f_off = off[1: 1 + 3 * p.nall].view(p.nall, 3)
        assert f_off.data_ptr() % 16 == 8
        _refused(lambda: step(ctx, split, b.x, rig.types, f_off, **kw), -20, off, "not 16-byte aligned")
    elif case == "negative_rows":
        _refused(lambda: step(ctx, (-1, n + 1, 0), b.x, rig.types, b.f, **kw), -20, b.fbuf, "negative row count")
    elif case == "null_type":
        _refused(lambda: step(ctx, split, b.x, None, b.f, **kw), -20, b.fbuf, "must not be NULL")
    elif case == "short_split":
        _refused(lambda: step(ctx, (0, n - 1, 0), b.x, rig.types, b.f, **kw), -20, b.fbuf, "row count of the installed list")
    elif case == "long_split":
        _refused(lambda: step(ctx, (0, n, 1), b.x, rig.types, b.f, **kw), -20, b.fbuf, "row count of the installed list")
    elif case == "energy_without_ev":
        _refused(lambda: step(ctx, split, b.x, rig.types, b.f, eflag=1, vflag=0, **no_ev), -20, b.fbuf, "without d_ev")
    elif case == "virial_without_ev":
        _refused(lambda: step(ctx, split, b.x, rig.types, b.f, eflag=0, vflag=1, **no_ev), -20, b.fbuf, "without d_ev")
    elif case == "vatom_without_ev":
        _refused(lambda: step(ctx, split, b.x, rig.types, b.f, eflag=2, vflag=4, **no_ev), -20, b.fbuf, "without d_ev")
    elif case == "no_list":
        bare = capi.Context(_pot("W_L8.mtp"), 0)
        _refused(lambda: step(bare, split, b.x, rig.types, b.f, **kw), -23, b.fbuf, "before mtp_set_neighbors")
    elif case == "grades_without_selection":
        _refused(lambda: step(ctx, split, b.x, rig.types, b.f, grade=True, grades_t=gr, maxg_t=mg, coeff_t=cd, **kw), -23, b.fbuf,
                 "no #MVS_v1.1 selection state")
    elif case == "nbh_grades_without_array":
        _refused(lambda: step(ctx, split, b.x, rig.types, b.f, grade=True, maxg_t=mg, coeff_t=cd, **kw), -20, b.fbuf,
                 "need a grades array")
    elif case == "cfg_without_coeff_ders":
        _refused(lambda: step(ctx, split, b.x, rig.types, b.f, grade=True, grades_t=gr, maxg_t=mg, **kw), -20, b.fbuf,
                 "need a coeff_ders array")
    assert bool((b.fbuf == SENTINEL).all()) and torch.isnan(b.x[n:]).all() and not b.ev.any()
    assert not gr.any() and not mg.any() and not cd.any()
    b.stale()
    step(ctx, split, b.x, rig.types, b.f, **good)
    _check_forces(p, b.forces(), want, "after the refusal")
    _check_ev(p, b.ev.cpu().numpy(), want, 1, "after the refusal")
    if case == "nbh_grades_without_array":
        assert abs(float(mg.item()) - want["max_grade"]) <= 1e-9 * max(1.0, want["max_grade"])
    elif case == "cfg_without_coeff_ders":
        _close(cd.cpu().numpy(), want["coeff_ders"], "coeff_ders after the refusal", atol=1e-9, rtol=1e-10)


NO_COMM = ["force_step", "forward", "forward_begin", "reverse", "reverse_begin"]


@pytest.mark.parametrize("entry", NO_COMM)
@on("pack_odd_tiny")
def test_halo_without_a_communicator_refuses_before_it_packs(rig, entry):
    """unique_id = None: force_step, forward and reverse answer MTP_ERR_STATE, as mtp_halo_allreduce does, with nothing
    launched; the pack kernel of such a halo still runs, and the rig's own halo still steps"""
    import torch
    p = rig.plan
    bare = capi.Halo(p, 0, None)
    ctx, split = _context(rig, "W_L8.mtp")
    b = Buffers(rig)
    b.f.fill_(SENTINEL)
    text = "created without a communicator"
    if entry == "force_step":
        _refused(lambda: bare.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, ev_t=b.ev, stream=rig.st), -23, b.fbuf,
                 text)
    else:
        arg = b.x if entry.startswith("forward") else b.f
        _refused(lambda: getattr(bare, entry)(arg, rig.st), -23, b.fbuf, text)
    assert torch.isnan(b.x[p.nlocal:]).all()
    bare.pack_forward(b.x, rig.st)
    rig.stream.synchronize()
    rig.halo.set_overlap(False)
    b.stale()
    rig.halo.force_step(ctx, split, b.x, rig.types, b.f, eflag=3, vflag=1, eatom_t=b.ea, ev_t=b.ev, stream=rig.st)
    _check_forces(p, b.forces(), _want(rig.name, "W_L8.mtp"), "after the refusal")
