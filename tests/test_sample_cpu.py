"""The numpy twin of the batched sampler (tests/_sample.py) on its own -- Philox4x32-10 against its published vectors, the
thermostat on free particles, the capture rules -- and the argument errors md.sample_cells raises without a device."""
import numpy as np
import pytest

import _sample
from _sample import KB, MVV2E, FTM2V


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(counter, key, want):
    got = _sample.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(w) for w in got] == list(want)
    # ... and as one row of a batch of counters
    many = _sample.philox4x32_10(np.array([(1, 2, 3, 4), counter, (5, 6, 7, 8)], dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(w) for w in many[1]] == list(want)


def test_noise_is_exact_symmetric_and_keyed_by_configuration_not_position():
    idx = np.arange(1000)
    a = _sample.noise(7, idx, np.uint64(0x123456789abcdef0), seed=99)
    assert a.shape == (1000, 3) and (np.abs(a) < 0.5).all() and (a != 0.0).all()
    assert np.array_equal((a + 0.5) * 2.0 ** 32 - 0.5, np.round((a + 0.5) * 2.0 ** 32 - 0.5))        # u = (w + 0.5) 2^-32 exactly
    assert abs(a.mean()) < 0.02 and abs(a.var() - 1.0 / 12.0) < 0.005
    b = _sample.noise(7, idx[500:], np.uint64(0x123456789abcdef0), seed=99)                          # the same atoms, asked for alone
    assert np.array_equal(a[500:], b)
    for other in (_sample.noise(8, idx, np.uint64(0x123456789abcdef0), 99), _sample.noise(7, idx, np.uint64(0x123456789abcdef1), 99),
                  _sample.noise(7, idx, np.uint64(0x123456789abcdef0), 98), _sample.noise(7, idx, np.uint64(0x023456789abcdef0), 99),
                  _sample.noise(7, idx, np.uint64(0x123456789abcdef0), 99 + 2 ** 32)):
        assert not np.array_equal(a, other)


def test_twin_thermostat_holds_free_particles_at_the_target_temperature():
    """512 free atoms (f = 0) of mass 183.84 from rest, 300 K, dt = 1 fs, t_damp = 0.1 ps, 4000 steps: the mean kinetic
    temperature after the first 500 steps (five damping times) is within 5 % of the target"""
    n, mass, T, dt, t_damp, steps = 512, 183.84, 300.0, 1e-3, 0.1, 4000
    m, inv_m = np.full(n, mass), np.full(n, 1.0 / mass)
    x, v = np.zeros((n, 3)), np.zeros((n, 3))
    idx, key, moving = np.arange(n), np.full(n, 12345, dtype=np.uint64), np.ones(n, dtype=bool)
    T_row = np.full(n, T)
    dtf = 0.5 * dt * FTM2V
    f = np.zeros((n, 3))
    _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, 0.0, 0, idx, key, 5, moving)
    temps = []
    for step in range(1, steps + 1):
        _sample.first_half(x, v, f, inv_m, dtf, dt, moving)
        f = np.zeros((n, 3))
        _sample.second_half(v, f, m, inv_m, T_row, t_damp, dt, dtf, step, idx, key, 5, moving)
        temps.append(MVV2E * (m[:, None] * v * v).sum() / (3 * n * KB))
    mean = float(np.mean(temps[500:]))
    print("mean kinetic temperature %.2f K" % mean)
    assert abs(mean - T) <= 0.05 * T


def test_twin_nve_mode_draws_nothing_and_frozen_rows_are_not_written():
    rng = np.random.default_rng(0)
    n = 10
    x, v, f = rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    m = np.full(n, 50.0)
    moving = np.arange(n) % 2 == 0
    x0, v0, f0 = x.copy(), v.copy(), f.copy()
    _sample.first_half(x, v, f, 1.0 / m, 0.3, 0.01, moving)
    _sample.second_half(v, f, m, 1.0 / m, np.full(n, 300.0), 0.0, 0.01, 0.3, 1, np.arange(n), np.zeros(n, dtype=np.uint64), 0, moving)
    assert np.array_equal(f, f0) and np.array_equal(x[~moving], x0[~moving]) and np.array_equal(v[~moving], v0[~moving])
    assert np.allclose(v[moving], v0[moving] + 2 * 0.3 / 50.0 * f0[moving], rtol=1e-14, atol=0)
    assert np.allclose(x[moving], x0[moving] + 0.01 * (v0[moving] + 0.3 / 50.0 * f0[moving]), rtol=1e-14, atol=0)


def test_twin_capture_rules():
    natoms = [3, 0, 2, 5, 1]
    # slot order is (step, configuration); an empty configuration is never captured, whatever its grade
    c = _sample.Capture(natoms, select=2.0, brk=10.0, gap=0, max_candidates=100)
    assert c.step(0, [1.0, 50.0, 2.0, 1.9, 3.0]) == [2, 4]
    assert c.step(4, [2.5, 0.0, 1.0, 11.0, 2.0]) == [0, 3, 4]
    assert c.records == [(2, 0, 2.0), (4, 0, 3.0), (0, 4, 2.5), (3, 4, 11.0), (4, 4, 2.0)]
    assert list(c.frozen) == [False, False, False, True, False] and c.dropped == 0
    # a frozen configuration is never captured again
    assert c.step(8, [0.0, 0.0, 0.0, 99.0, 0.0]) == [] and len(c.records) == 5
    # capture_gap: a configuration is captured again only gap steps after its last capture
    c = _sample.Capture(natoms, 2.0, 10.0, gap=8, max_candidates=100)
    assert c.step(0, [3, 0, 0, 0, 0]) == [0] and c.step(4, [3, 0, 3, 0, 0]) == [2] and c.step(8, [3, 0, 3, 0, 0]) == [0]
    assert c.step(12, [3, 0, 3, 0, 0]) == [2] and [r[:2] for r in c.records] == [(0, 0), (2, 4), (0, 8), (2, 12)]
    # a full buffer drops whole snapshots, counts them, and does not freeze what it dropped
    c = _sample.Capture(natoms, 2.0, 10.0, 0, max_candidates=2)
    assert c.step(0, [20.0, 0, 3.0, 30.0, 4.0]) == [0, 2] and c.dropped == 2
    assert list(c.frozen) == [True, False, False, False, False]
    assert c.step(1, [20.0, 0, 3.0, 30.0, 4.0]) == [] and c.dropped == 5 and len(c.records) == 2
    # a NaN grade captures and freezes
    c = _sample.Capture(natoms, 2.0, 10.0, 0, 100)
    assert c.step(0, [np.nan, np.nan, 1.0, 1.0, 1.0]) == [0] and list(c.frozen) == [True, False, False, False, False]
    assert np.isnan(c.records[0][2])


def test_sample_cells_argument_errors_are_raised_before_anything_touches_the_device():
    """ctx is never looked at: None stands in for it"""
    from lammps_mtp_kokkos_amd.md import sample_cells
    cfgs = [(np.zeros((1, 3)), 5.0 * np.eye(3), None), (np.array([[0.0, 0, 0], [2.5, 2.5, 2.5]]), 5.0 * np.eye(3), [1, 2])]
    with pytest.raises(ValueError, match="threshold_select"):
        sample_cells(None, cfgs, 300.0, 10, 1e-3, threshold_select=3.0, threshold_break=2.0)
    for dt in (0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError, match="dt"):
            sample_cells(None, cfgs, 300.0, 10, dt)
    for keys in ([1], [1, 2, 3]):
        with pytest.raises(ValueError, match="keys"):
            sample_cells(None, cfgs, 300.0, 10, 1e-3, keys=keys)
    with pytest.raises(ValueError, match="temperature"):
        sample_cells(None, cfgs, [300.0, 200.0, 100.0], 10, 1e-3)
    with pytest.raises(ValueError, match="masses"):
        sample_cells(None, cfgs, 300.0, 10, 1e-3, masses=[183.84, -186.2])
    with pytest.raises(ValueError, match="velocities"):
        sample_cells(None, cfgs, 300.0, 10, 1e-3, velocities=[np.zeros((1, 3)), np.zeros((3, 3))])


def test_maxwell_boltzmann_is_per_configuration_and_has_no_net_momentum():
    from lammps_mtp_kokkos_amd.md import maxwell_boltzmann
    rng = np.random.default_rng(1)
    items = [(rng.normal(size=(n, 3)), rng.integers(1, 3, n)) for n in (400, 0, 1, 300)]
    masses = np.array([183.84, 186.2])
    v = maxwell_boltzmann(items, masses, np.array([300.0, 300.0, 300.0, 600.0]), 7, [10, 11, 12, 13])
    alone = maxwell_boltzmann(items[3:], masses, np.array([600.0]), 7, [13])
    assert np.array_equal(v[3], alone[0]) and v[1].shape == (0, 3) and not v[2].any()
    for k in (0, 3):
        m = masses[items[k][1] - 1]
        assert np.abs((m[:, None] * v[k]).sum(0)).max() < 1e-9
        T = MVV2E * (m[:, None] * v[k] ** 2).sum() / (3 * len(m) * KB)
        assert abs(T - (300.0, 0, 0, 600.0)[k]) < 0.12 * (300.0, 0, 0, 600.0)[k]


@pytest.mark.parametrize("kw,answers,want,s_want", [
    (dict(steps=5, every=3, check_every=2), (), "F H0 | I1 F H1 | I2 M F H2 | I3 M B F H3 | I4 F H4 | I5 M F H5", 5),
    (dict(steps=5, every=3, check_every=2), [(True, False)], "F H0 | I1 F H1 | I2 M", 1),
    (dict(steps=5, every=3, check_every=2, grade_every=2), [(True, False)], "F H0 C0 M", 0),
    (dict(steps=1, every=3, check_every=2, thermostat=False), (), "F | I1 F H1", 1),
    (dict(steps=3, every=3, check_every=1), [(False, True)], "F H0 | I1 M B F H1 | I2 M F H2 | I3 M F H3", 3),
    (dict(steps=2, every=3, check_every=0, grade_every=2), (), "F H0 C0 M | I1 F H1 | I2 F H2 C2", 2),
], ids=["cadence", "all-frozen-at-a-read", "frozen-at-graded-step-0", "nve", "stale", "graded"])
@pytest.mark.parametrize("recording", [False, True], ids=["", "record"])
def test_the_sampler_loop_asks_the_run_in_the_order_of_sample_cells(kw, answers, want, s_want, recording):
    """md._sample_pass, the step loop of sample_cells and sample_cells_npt, with a run that has no device behind it (the twin of
    the test of md._minimise_pass in tests/test_relax_cpu.py).  F forces, H<s> second half, I<s> first half, C<s> capture, M read,
    B rebuild; the sequences are read off the loop sample_cells had of its own:

      case                     steps every check_every grade_every thermostat reads              sequence                          returns
      cadence                  5     3     2           0           on         (False, False)...  F H0 | I1 F H1 | I2 M F H2 |      5
                                                                                                 I3 M B F H3 | I4 F H4 | I5 M F H5
      all frozen at a read     5     3     2           0           on         first (True, -)    F H0 | I1 F H1 | I2 M             1
      frozen at graded step 0  5     3     2           2           on         first (True, -)    F H0 C0 M                         0
      NVE                      1     3     2           0           off        (False, False)...  F | I1 F H1                       1
      stale                    3     3     1           0           on         first (-, True)    F H0 | I1 M B F H1 | I2 M F H2 |  3
                                                                                                 I3 M F H3
      graded                   2     3     0           2           on         (False, False)...  F H0 C0 M | I1 F H1 | I2 F H2 C2  2

    Step 0 is forces, the thermostat's setup call (no kick) and, graded, the capture and one read.  Then per step: the first
    half, since += 1, the read at since >= every and at since % check_every == 0, the all-frozen break -- the step whose first
    half wrote nothing is not counted --, the rebuild when due or stale (since = 0), forces, the second half, the capture.  The
    forces are graded exactly on the grade steps, and record follows every completed step, step 0 included."""
    from lammps_mtp_kokkos_amd import md
    from _stub_run import StubRun
    run = StubRun(answers)
    ge = kw.get("grade_every", 0)
    s = md._sample_pass(run, kw["steps"], lambda step: bool(ge) and step % ge == 0, kw["every"], kw["check_every"], run.first_half,
                        run.second_half, run.record if recording else None, thermostat=kw.get("thermostat", True))
    assert " ".join(run.log) == want.replace(" |", "")
    assert s == s_want and run.log.count("B") == want.count("B")
    assert run.graded_forces == [bool(ge) and q % ge == 0 for q in range(s + 1)]
    assert run.recorded == (list(range(s + 1)) if recording else [])
    assert run.moves == 0                                                            # (what follows a move is the first half's)
