"""MaxVol selection without a GPU: the file writer (mtp_potential_write_selection) against the library's own parser, the
CPU oracle and, where it was built, the compiled reference; its error cases; and the numpy twin
(driver.maxvol_select_numpy) on its own.  Convention (include/mtp_mi355x.h): the columns of the first raw block S are the
selected candidate vectors, the second block is W = S^-1, a candidate c grades W c."""
import ctypes
import os

import numpy as np
import pytest

from lammps_mtp_kokkos_amd import capi
from lammps_mtp_kokkos_amd.driver import maxvol_select_numpy, periodic_system_cell

import _batch
import _maxvol
from _cells import POT, LIST_CUTOFF


def _new_state(C, seed):
    """a selection state that differs from every committed one: the twin's result on a small random pool"""
    S, W = _maxvol.random_state(C, seed=seed)
    S1, W1, swaps, _ = maxvol_select_numpy(_maxvol.random_pool(C, 40, seed=seed + 1), S, W, 2.0, 4 * C)
    assert swaps
    return S1, W1


@pytest.mark.parametrize("fname", ["W_L16_nbh.almtp", "WRe_L10_cfg.almtp"])
def test_written_file_round_trips_bit_for_bit_in_both_selection_modes(fname, tmp_path):
    src = os.path.join(POT, fname)
    old = capi.Potential(src, selection=True)
    C = old.info.coeff_count
    S1, W1 = _new_state(C, 5)
    dst = str(tmp_path / ("new_" + fname))
    capi.write_selection(src, dst, S1, W1)
    new = capi.Potential(dst, selection=True)
    assert new.info.configuration_mode == old.info.configuration_mode and new.info.coeff_count == C
    assert np.array_equal(new.active_set(), S1) and np.array_equal(new.tables()["inverse_active_set"], W1)
    a, b = open(src, "rb").read(), open(dst, "rb").read()
    text = len(a) - 2 * 8 * C * C                            # everything up to and including the '#' of the raw blocks
    assert len(b) == len(a) and b[:text] == a[:text] and a[text - 1:text] == b"#"
    assert b[text:] == S1.tobytes() + W1.tobytes()
    assert os.listdir(tmp_path) == ["new_" + fname]          # the temporary file is gone
    # the source's own blocks come back through the same two getters
    assert np.array_equal(np.frombuffer(a[text:text + 8 * C * C]).reshape(C, C), old.active_set())
    assert np.abs(old.tables()["inverse_active_set"] @ old.active_set() - np.eye(C)).max() < 1e-13
    # a file of the writer is a source of the writer
    again = str(tmp_path / "again.almtp")
    capi.write_selection(dst, again, old.active_set(), old.tables()["inverse_active_set"])
    assert open(again, "rb").read() == a


def test_the_oracle_and_the_reference_grade_with_the_written_blocks(tmp_path):
    from oracle import pyoracle, pyref
    src = os.path.join(POT, "W_L16_nbh.almtp")
    C = capi.Potential(src, selection=True).info.coeff_count
    S1, W1 = _new_state(C, 11)
    dst = str(tmp_path / "new.almtp")
    capi.write_selection(src, dst, S1, W1)
    orc = pyoracle.Oracle(dst, selection=True)
    assert np.array_equal(orc.arr("inverse_active_set", C * C).reshape(C, C), W1)
    assert np.array_equal(orc.arr("active_set", C * C).reshape(C, C), S1)
    grade = pyoracle.lib().mtp_oracle_grade
    for c in list(_maxvol.random_pool(C, 3, seed=2)) + [S1[:, 7].copy()]:
        got = grade(ctypes.byref(orc.m), c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        want = np.abs(W1 @ c)
        assert abs(got - want.max()) <= 1e-12 * max(1.0, want.max())
    assert abs(np.abs(W1 @ S1[:, 7]).max() - 1.0) < 1e-12      # a member of the set grades e_j
    # per-atom grades of a real cell: the oracle on the written file against W' . c_i, with c_i what an extrapolation call
    # over atom i alone leaves in coeff_ders (neighbourhood mode clears it per atom) -- on the SOURCE file, whose W differs
    pos, cell, types = _batch.sheared8_cell()
    s = periodic_system_cell(pos, cell, types, LIST_CUTOFF)
    new = orc.compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=s.nlocal)
    assert new["max_grade"] == new["grades"][: s.nlocal].max() > 0.0
    old_orc = pyoracle.Oracle(src, selection=True)
    for ii in range(s.nlocal):
        lo, hi = int(s.first[ii]), int(s.first[ii + 1])
        one = old_orc.compute(s.x, s.types, s.ilist[ii:ii + 1], np.array([0, hi - lo], dtype=np.int32), s.neigh[lo:hi],
                              extrapolation=True, natoms=1)
        want = np.abs(W1 @ one["coeff_ders"]).max()
        got = new["grades"][s.ilist[ii]]
        assert abs(got - want) <= 1e-12 * max(1.0, want), (ii, got, want)
    if pyref.available():
        ref = pyref.Reference(dst, selection=True)
        want = ref.compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True, natoms=s.nlocal)
        _batch.close(new["grades"][: s.nlocal], want["grades"][: s.nlocal], "oracle against the compiled reference on the written file",
                     atol=1e-9, rtol=1e-9)
        old = pyref.Reference(src, selection=True).compute(s.x, s.types, s.ilist, s.first, s.neigh, extrapolation=True,
                                                           natoms=s.nlocal)
        assert np.abs(old["grades"][: s.nlocal] - want["grades"][: s.nlocal]).max() > 1e-3   # (the blocks did change)


def test_writer_error_cases(tmp_path):
    src = os.path.join(POT, "W_L16_nbh.almtp")
    pot = capi.Potential(src, selection=True)
    C = pot.info.coeff_count
    S, W = pot.active_set(), pot.tables()["inverse_active_set"]
    dst = str(tmp_path / "out.almtp")
    with pytest.raises(capi.MtpError) as ei:                  # no #MVS tail in the source
        capi.write_selection(os.path.join(POT, "W_L16.mtp"), dst, S, W)
    assert ei.value.code == -8
    with pytest.raises(capi.MtpError) as ei:                  # blocks of another potential's size
        capi.write_selection(src, dst, S[:26, :26].copy(), W[:26, :26].copy())
    assert ei.value.code == -20 and "149" in str(ei.value)
    with pytest.raises(capi.MtpError) as ei:
        capi.write_selection(str(tmp_path / "missing.almtp"), dst, S, W)
    assert ei.value.code == -2
    with pytest.raises(capi.MtpError) as ei:                  # the destination's directory does not exist
        capi.write_selection(src, str(tmp_path / "nowhere" / "out.almtp"), S, W)
    assert ei.value.code == -2
    with pytest.raises(ValueError):
        capi.write_selection(src, dst, S, W[:, :5])
    assert os.listdir(tmp_path) == []                         # no refused call left a file behind
    with pytest.raises(capi.MtpError) as ei:                  # and a potential loaded without its tail has no active set
        capi.Potential(os.path.join(POT, "W_L16.mtp")).active_set()
    assert ei.value.code == -23
    rc = capi.lib().mtp_potential_write_selection(None, None, None, None, C, None, 0)
    assert rc == -20


@pytest.mark.parametrize("C,N", [(26, 300), (115, 1000)])
@pytest.mark.parametrize("threshold", [2.0, 1.1, 1.0 + 1e-6])
def test_the_twin_on_its_own(C, N, threshold):
    r = _maxvol.twin_run(C, N, threshold)
    S, W, V, S1, W1, swaps, G = (r[k] for k in ("S", "W", "V", "S1", "W1", "swaps", "G"))
    assert 0 < len(swaps) <= 1.03 * C + 1                    # converged well inside the 4 C budget
    fresh = V @ W1.T
    print("C = %d N = %d threshold %.7g: %d swaps, drift %.3e, |W'S' - I| %.3e" % (
        C, N, threshold, len(swaps), np.abs(G - fresh).max(), np.abs(W1 @ S1 - np.eye(C)).max()))
    # the twin stops on its rank-1-updated G (<= threshold exactly); freshly computed grades differ from it by the drift,
    # which fp64 rounding of at most ~C rank-1 updates of entries <= max |G| keeps orders below 1e-11 at these sizes
    drift = float(np.abs(G - fresh).max())
    assert np.abs(G).max() <= threshold and drift <= 1e-11 and np.abs(W1 @ S1 - np.eye(C)).max() <= 1e-11
    assert np.abs(fresh).max() <= threshold + drift
    gain = sum(np.log(abs(p)) for _, _, p in swaps)
    assert abs(gain - (np.linalg.slogdet(S1)[1] - np.linalg.slogdet(S)[1])) <= 1e-9
    assert all(abs(p) > threshold for _, _, p in swaps)
    src = _maxvol.slot_source_of(swaps, C)
    for j in range(C):                                        # column provenance, bit for bit
        assert np.array_equal(S1[:, j], S[:, j] if src[j] < 0 else V[src[j]])
    assert (src >= 0).any() and np.array_equal(r["S"], _maxvol.random_state(C)[0])   # (the shared inputs were not written to)


def test_the_twin_breaks_ties_towards_the_smaller_linear_index_and_respects_max_swaps():
    C = 26
    S, W = _maxvol.random_state(C)
    V = _maxvol.random_pool(C, 50)
    V[31] = V[12]                                             # two bit-identical rows
    G0 = V @ W.T
    i0, j0 = divmod(int(np.argmax(np.abs(G0))), C)
    V[40] = V[i0]                                             # ... and a copy of the row that holds the global maximum
    _, _, swaps, _ = maxvol_select_numpy(V, S, W, 1.1, 4 * C)
    assert swaps[0][:2] == (min(i0, 40), j0)
    S3, W3, three, _ = maxvol_select_numpy(V, S, W, 1.1, 3)
    assert three == swaps[:3] and np.abs(W3 @ S3 - np.eye(C)).max() < 1e-12
    S0, W0, none, G = maxvol_select_numpy(V[:0], S, W, 1.1, 4 * C)
    assert none == [] and np.array_equal(S0, S) and np.array_equal(W0, W) and G.shape == (0, C)
