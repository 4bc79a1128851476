"""More than one pass through md.sample_cells, md.relax_cells and md.relax_cells_vc (tests/test_sample_gpu.py,
tests/test_relax_gpu.py, tests/test_relax_vc_gpu.py): the batch of _batch.mixed_batch -- 1, 2, 5, 0, 8 and 54 atoms -- run whole,
with max_atoms_per_pass = 1 (six passes of one configuration, one of them without an atom) and with max_atoms_per_pass = 8
(passes (0, 4) (4, 5) (5, 6): the empty configuration inside a pass of several).  A pass is a complete run of its
configurations, so a split run is compared with the whole run and, for what a pass does on its own -- its list builds, the
step it ends at --, with runs of the passes' configurations alone."""
import numpy as np

from lammps_mtp_kokkos_amd.md import plan_cell_passes

import _sample

SPLITS = {1: [(k, k + 1) for k in range(6)], 8: [(0, 4), (4, 5), (5, 6)]}


def assert_split_runs_are_the_whole_run(run, batch, list_cutoff, same_final, trace_tol, x_tol, same_cell=None):
    """run(first, end, max_atoms_per_pass) -> what the driver returns for batch[first:end] (trace=True); same_final(got, want,
    config) asserts on one entry of `final`; trace_tol = {trace column: bound}; same_cell(got, want, given, step) asserts on a
    candidate's cell (default: bitwise the cell given).  Returns (the whole run, {max_atoms_per_pass: the split run})."""
    ncfg = len(batch)
    natoms = np.array([len(c[0]) for c in batch])
    cells = np.array([c[1] for c in batch])
    whole = run(0, ncfg, None)
    assert [(a, b) for a, b, _ in plan_cell_passes(cells, natoms, list_cutoff)[0]] == [(0, ncfg)]
    assert whole["dropped"] == 0
    rows = whole["steps_done"] + 1
    out = {}
    for cap, passes in SPLITS.items():
        assert [(a, b) for a, b, _ in plan_cell_passes(cells, natoms, list_cutoff, cap)[0]] == passes
        got = out[cap] = run(0, ncfg, cap)
        parts = [run(a, b, None) for a, b in passes]
        print("max_atoms_per_pass %d: steps_done %d (whole %d, passes %r), builds %d (whole %d, passes %r)"
              % (cap, got["steps_done"], whole["steps_done"], [p["steps_done"] for p in parts], got["builds"], whole["builds"],
                 [p["builds"] for p in parts]))
        assert got["steps_done"] == whole["steps_done"] == max(p["steps_done"] for p in parts)
        assert got["builds"] == sum(p["builds"] for p in parts)
        assert sorted(got["trace"]) == sorted(trace_tol)
        for (a, b), part in zip(passes, parts):
            done = part["steps_done"] if natoms[a:b].sum() else -1       # (a pass without an atom records nothing)
            for name, tol in trace_tol.items():
                col, ref = got["trace"][name], whole["trace"][name]
                assert col.shape == ref.shape == (rows, ncfg), name
                err = float(np.abs(col[: done + 1, a:b] - ref[: done + 1, a:b]).max(initial=0.0))
                print("  pass (%d, %d), ended at step %d: trace %s differs by %.3e" % (a, b, done, name, err))
                assert err < tol, (cap, a, b, name)
                assert not col[done + 1:, a:b].any(), (cap, a, b, name)  # rows after the pass's own end stay zero
        for k in range(ncfg):
            same_final(got["final"][k], whole["final"][k], batch[k])
        if "frozen" in whole:
            assert np.array_equal(got["frozen"], whole["frozen"])
        # records and candidates: by pass in the split run, by (step, configuration) in the whole run; configuration numbers
        # are those of the batch
        order = sorted(range(len(got["records"])), key=lambda i: (got["records"][i][1], got["records"][i][0]))
        assert [got["records"][i][:2] for i in order] == [r[:2] for r in whole["records"]]
        assert got["dropped"] == 0 and len(got["candidates"]) == len(got["records"])
        for i, (k, s, g), (pos, cell, types) in zip(order, whole["records"], whole["candidates"]):
            g1, (pos1, cell1, types1) = got["records"][i][2], got["candidates"][i]
            assert abs(g1 - g) <= 1e-9 * max(1.0, abs(g)), (cap, k, s, g1, g)
            assert pos1.shape == batch[k][0].shape and np.array_equal(types1, batch[k][2])
            assert _sample.wrapped_diff(pos1, pos, cell) < x_tol, (cap, k, s)
            if same_cell is None:
                assert np.array_equal(cell1, batch[k][1]) and np.array_equal(cell, batch[k][1])
            else:
                same_cell(cell1, cell, batch[k][1], s)
    return whole, out
