"""Device-resident velocity-Verlet (NVE) driver around the MTP force call -- the standalone counterpart of what
LAMMPS' Verlet / Comm / Neighbor classes do around `Pair::compute`.  Positions,
velocities, forces, ghost maps and the neighbour list stay in HBM between steps; every piece of the step is one of
the library's HIP kernels (include/mtp_mi355x.h, "standalone MD support"):

  per step      mtp_nve_initial (kick + drift) -> mtp_ghosts_forward (ghosts follow their owners) -> force call
                (mtp_compute_device) -> mtp_ghosts_reverse (ghost forces onto owners: newton_pair on,
                /root/reference/LAMMPS/ML-MTP/pair_mtp.cpp:252-254, 315) -> mtp_nve_final (kick)
  every `every` steps (or when an atom moved more than half the skin: mtp_nve_monitor, one 16-byte read-back)
                mtp_ghosts_build (wrap + periodic images, on the device) and mtp_build_neighbors_device

`box` is a 3-vector (orthogonal box with every edge >= the list cutoff: mtp_ghosts_build, the path the whole-step
benchmark times) or a 3x3 cell whose rows are the lattice vectors (any periodic cell, triclinic or smaller than the
cutoff: mtp_ghosts_build_cell, list bounds from mtp_ghosts_cell_bounds).  evaluate_cell is one such evaluation
without the integrator; evaluate_cells does many of them -- training or candidate configurations, each with its own
cell -- in one device pass (include/mtp_mi355x.h, "batched configurations").  sample_cells is the integrator over that
batch layout: Langevin (or NVE) MD of all the cells at once with the extrapolation grade watched, and the extrapolating
configurations captured, on the device (include/mtp_mi355x.h, "batched sampling"); sample_cells_npt does the same at constant
pressure, the cells moved by a stochastic barostat ("batched constant-pressure sampling").  relax_cells and relax_cells_vc take
the batch to its minima ("batched relaxation"), neb_cells connects minima by climbing-image nudged elastic bands ("batched
nudged elastic band").

torch only allocates the arrays and provides the stream; the host sees the ghost count and the list size at a
re-neighbouring (they size arrays) and nothing else.
"""
from __future__ import annotations

import collections

import numpy as np

from . import capi

MVV2E = 1.0364269e-4          # (g/mol)(A/ps)^2 -> eV     (LAMMPS metal units)
FTM2V = 1.0 / MVV2E           # eV/A / (g/mol) -> A/ps^2
KB = 8.617343e-5              # eV/K


class DeviceNVE:
    def __init__(self, ctx, pos, box, rc, types=None, mass=183.84, list_cutoff=7.0, device=None, every=10,
                 check_every=4, vflag=0):
        import torch
        self.torch = torch
        self.ctx = ctx
        self.dev = device or torch.device("cuda:0")
        # torch's default stream is the null stream, which the library maps to its own non-blocking stream: use one
        # real stream for the allocations' fills and the library's kernels so that they are ordered
        if torch.cuda.current_stream(self.dev).cuda_stream == 0:
            capi.use_private_torch_stream(self.dev)
        self.st = torch.cuda.current_stream(self.dev).cuda_stream
        self.box_np = np.asarray(box, dtype=np.float64)
        if self.box_np.shape not in ((3,), (3, 3)):
            raise ValueError("box: a 3-vector (orthogonal box) or a 3x3 cell (rows = lattice vectors)")
        self.is_cell = self.box_np.shape == (3, 3)
        self.n = len(pos)
        types_np = np.ones(self.n, dtype=np.int32) if types is None else np.asarray(types, dtype=np.int32)
        masses = np.atleast_1d(np.asarray(mass, dtype=np.float64))
        if len(masses) < int(types_np.max()):
            masses = np.full(int(types_np.max()), float(masses[0]))
        self.mass_t = torch.from_numpy(masses).to(self.dev)
        self.inv_mass_t = torch.from_numpy(1.0 / masses).to(self.dev)
        self.cut = float(list_cutoff)
        self.rc = float(rc)                # potential cutoff: skin = list_cutoff - rc
        self.every = int(every)
        self.check_every = int(check_every)
        self.vflag = int(vflag)          # 1: the global virial is tallied too (as in the headline benchmark)
        self.ghosts = capi.Ghosts(self.dev.index or 0)
        self.cap = 0
        self._alloc(int(self.n * 1.6) + 1024, pos, types_np)
        self.v = torch.zeros((self.n, 3), dtype=torch.float64, device=self.dev)
        self.mon = torch.zeros(2, dtype=torch.float64, device=self.dev)
        self.x_ref = torch.empty((self.n, 3), dtype=torch.float64, device=self.dev)
        self.steps_since_build = 0
        self.builds = 0
        self._reneighbor()
        self._forces()

    @property
    def x(self):
        """owned atoms (wrapped into the box at the last re-neighbouring)"""
        return self.xall[: self.n]

    @property
    def f(self):
        return self.fall[: self.n]

    def _alloc(self, cap, pos=None, types_np=None):
        torch = self.torch
        xall = torch.zeros((cap, 3), dtype=torch.float64, device=self.dev)
        tall = torch.ones(cap, dtype=torch.int32, device=self.dev)
        if pos is not None:
            xall[: self.n] = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64)).to(self.dev)
            tall[: self.n] = torch.from_numpy(types_np).to(self.dev)
        else:
            xall[: self.n] = self.xall[: self.n]
            tall[: self.n] = self.types_all[: self.n]
        self.xall, self.types_all = xall, tall
        # forces and the energy / virial totals share one allocation, so that one launch zeroes both every step
        self.fbuf = torch.zeros(3 * cap + 8, dtype=torch.float64, device=self.dev)
        self.fall = self.fbuf[: 3 * cap].view(cap, 3)
        self.ev = self.fbuf[3 * cap:]
        self.cap = cap

    # ---- ghosts + list (re-neighbouring), all on the device ----------------------------------------------------
    def _reneighbor(self):
        build = self.ghosts.build_cell if self.is_cell else self.ghosts.build
        try:
            self.nall = build(self.xall, self.n, self.box_np, self.cut, stream=self.st)
        except capi.MtpError as e:
            if e.code != -24 or self.ghosts.nall <= self.cap or self.ghosts.nall >= 2 ** 31 - 1:
                raise
            self._alloc(int(self.ghosts.nall * 1.2) + 1024)
            self.nall = build(self.xall, self.n, self.box_np, self.cut, stream=self.st)
        self.ghosts.types(self.types_all, stream=self.st)
        if self.is_cell:
            b = capi.ghosts_cell_bounds(self.box_np, self.cut)
            lo, hi = b["lo"], b["hi"]
        else:
            lo = [-self.cut - 1.0] * 3
            hi = self.box_np + self.cut + 1.0
        self.entries, self.max_row = self.ctx.build_neighbors_device(self.xall, self.n, self.nall, self.cut, lo, hi,
                                                                     stream=self.st)
        self.x_ref.copy_(self.xall[: self.n])
        self.steps_since_build = 0
        self.builds += 1

    def _forces(self):
        self.ghosts.forward(self.xall, stream=self.st)
        capi.zero_async(self.fbuf, stream=self.st)      # f (all rows of the allocation) and ev in one launch
        # (finish_tallies=False: the energy / virial fold rides in the launch that folds the ghost forces)
        self.ctx.compute_device_rows(0, self.n, False, self.xall, self.types_all, self.fall, eflag=1, vflag=self.vflag,
                                     ev_t=self.ev, stream=self.st)
        self.ghosts.reverse_finish(self.ctx, self.fall, self.ev, eflag=1, vflag=self.vflag, stream=self.st)

    # ---- one velocity-Verlet step ------------------------------------------------------------------------------
    def step(self, dt):
        dtf = 0.5 * dt * FTM2V
        capi.nve_initial(self.n, self.xall, self.v, self.fall, self.types_all, self.inv_mass_t, dtf, dt, stream=self.st)
        self.steps_since_build += 1
        need = self.steps_since_build >= self.every
        if not need and self.check_every and self.steps_since_build % self.check_every == 0:   # half-skin criterion
            capi.nve_monitor(self.n, self.xall, self.x_ref, self.v, self.types_all, self.mass_t, self.mon, stream=self.st)
            need = bool(self.mon[0].item() > (0.5 * (self.cut - self.rc)) ** 2)
        if need:
            self._reneighbor()
        self._forces()
        capi.nve_final(self.n, self.v, self.fall, self.types_all, self.inv_mass_t, dtf, stream=self.st)

    def total_energy(self):
        capi.nve_monitor(self.n, self.xall, self.x_ref, self.v, self.types_all, self.mass_t, self.mon, stream=self.st)
        m = self.mon.cpu().numpy()
        return float(self.ev[0].item()) + 0.5 * MVV2E * float(m[1])


def _torch_stream(dev):
    import torch
    if torch.cuda.current_stream(dev).cuda_stream == 0:      # see DeviceNVE.__init__
        capi.use_private_torch_stream(dev)
    return torch.cuda.current_stream(dev).cuda_stream


def evaluate_cell(ctx, pos, cell, types=None, list_cutoff=7.0, vflag=1, grades=False, device=None):
    """One device-resident evaluation of a periodic cell of any shape and size (rows of `cell` = lattice vectors):
    ghost images (mtp_ghosts_build_cell), the full list (mtp_build_neighbors_device), the force call and the fold of the
    ghost forces onto their owners, all in HBM.  Returns dict(energy, f [n, 3] in the order of `pos`, virial [6]
    (xx, yy, zz, xy, xz, yz; pair-style sign: virial_ab = sum r_a f_b, zeros when vflag = 0), volume, x [n, 3] the
    positions wrapped into the cell) and, with grades=True (a potential loaded with its selection state,
    neighbourhood mode), grades [n] and max_grade."""
    import torch
    dev = device or torch.device("cuda:0")
    st = _torch_stream(dev)
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    n = len(pos)
    types_np = np.ones(n, dtype=np.int32) if types is None else np.ascontiguousarray(types, dtype=np.int32)
    bounds = capi.ghosts_cell_bounds(cell, list_cutoff)
    ghosts = capi.Ghosts(dev.index or 0)

    def alloc(cap):
        x = torch.zeros((cap, 3), dtype=torch.float64, device=dev)
        x[:n] = torch.from_numpy(pos).to(dev)
        return x

    xall = alloc(n)                                          # the first call only counts: it reports the size needed
    try:
        nall = ghosts.build_cell(xall, n, cell, list_cutoff, stream=st)
    except capi.MtpError as e:
        if e.code != -24 or ghosts.nall <= n or ghosts.nall >= 2 ** 31 - 1:
            raise
        xall = alloc(ghosts.nall)
        nall = ghosts.build_cell(xall, n, cell, list_cutoff, stream=st)
    tall = torch.ones(xall.shape[0], dtype=torch.int32, device=dev)
    tall[:n] = torch.from_numpy(types_np).to(dev)
    ghosts.types(tall, stream=st)
    ctx.build_neighbors_device(xall, n, nall, list_cutoff, bounds["lo"], bounds["hi"], stream=st)
    fbuf = torch.zeros(3 * xall.shape[0] + 8, dtype=torch.float64, device=dev)
    fall, ev = fbuf[: 3 * xall.shape[0]].view(-1, 3), fbuf[3 * xall.shape[0]:]
    g_t = torch.zeros(nall, dtype=torch.float64, device=dev) if grades else None
    mg_t = torch.zeros(1, dtype=torch.float64, device=dev) if grades else None
    ctx.compute_device_rows(0, n, False, xall, tall, fall, eflag=1, vflag=int(vflag), grade=bool(grades), ev_t=ev,
                            grades_t=g_t, maxg_t=mg_t, stream=st)
    ghosts.reverse_finish(ctx, fall, ev, eflag=1, vflag=int(vflag), stream=st)
    ctx.synchronize(stream=st)                               # an atom type outside the potential is reported here
    evh = ev.cpu().numpy()
    out = dict(energy=float(evh[0]), f=fall[:n].cpu().numpy(), virial=evh[1:7].copy(), volume=bounds["volume"],
               x=xall[:n].cpu().numpy())
    if grades:
        out.update(grades=g_t[:n].cpu().numpy(), max_grade=float(mg_t.item()))
    return out


class _BatchBuffers:
    """device (and pinned host) arrays of evaluate_cells, grown as needed and reused across its passes"""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev
        self.cap = self.cap_cfg = self.cap_work = self.cap_out = 0

    def reserve(self, cap, ncfg, work, out):
        torch, dev = self.torch, self.dev
        if cap > self.cap:
            self.cap = int(cap * 1.1) + 1024
            self.xall = torch.empty((self.cap, 3), dtype=torch.float64, device=dev)
            self.tall = torch.empty(self.cap, dtype=torch.int32, device=dev)
            self.grades = torch.empty(self.cap, dtype=torch.float64, device=dev)
        if ncfg > self.cap_cfg:
            self.cap_cfg = int(ncfg * 1.1) + 16
            self.res = torch.empty(8 * self.cap_cfg, dtype=torch.float64, device=dev)
        if work > self.cap_work:
            self.cap_work = int(work * 1.1) + 1024
            self.work = torch.empty(self.cap_work, dtype=torch.float64, device=dev)
        if out > self.cap_out:
            self.cap_out = int(out * 1.1) + 1024
            self.out_host = torch.empty(self.cap_out, dtype=torch.float64, pin_memory=True)


def plan_cell_passes(cells, natoms, list_cutoff, max_atoms_per_pass=None):
    """Host arithmetic only: the passes evaluate_cells makes over a batch.  cells [ncfg, 3, 3], natoms [ncfg].  A pass is
    a run of consecutive configurations; a new one starts where the owned atoms would exceed `max_atoms_per_pass` (a
    configuration is never split), where owned + ghost atoms could approach 2^31, and where mtp_batch_layout says the
    batch no longer fits its limits (2^26 list cells, coordinates within 2048 A).  Returns ([(first, end, layout)], the
    cell volumes, the most rows -- owned + ghost atoms -- every configuration can need)."""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    natoms = np.asarray(natoms, dtype=np.int64)
    cut = float(list_cutoff)
    # volumes and margins m_a = rghost / d_a of all cells at once (driver.cell_margins); every atom has at most
    # floor(1 + 2 m_a) + 1 shifts per direction, which bounds the rows a configuration can need
    with np.errstate(all="ignore"):
        cross = np.stack([np.cross(cells[:, 1], cells[:, 2]), np.cross(cells[:, 2], cells[:, 0]),
                          np.cross(cells[:, 0], cells[:, 1])], axis=1)
        volume = (cells[:, 0] * cross[:, 0]).sum(1)
        margins = cut * np.sqrt((cross * cross).sum(2)) / volume[:, None]
        bad = ~(np.isfinite(cells).all((1, 2)) & (volume > 0.0) & np.isfinite(margins).all(1))
    if bad.any():
        raise capi.MtpError(-20, "configuration %d: the cell must be finite, right-handed and non-degenerate (det > 0)"
                            % int(np.nonzero(bad)[0][0]))
    max_rows = natoms * np.prod(np.floor(1.0 + 2.0 * margins) + 1.0, axis=1)
    queue, begin, atoms, rows = [], 0, 0, 0.0
    for k in range(len(cells)):
        n = int(natoms[k])
        if k > begin and ((max_atoms_per_pass is not None and atoms + n > max_atoms_per_pass)
                          or rows + max_rows[k] > 2.0 ** 31 - 2.0 ** 20):
            queue.append((begin, k))
            begin, atoms, rows = k, 0, 0.0
        atoms, rows = atoms + n, rows + max_rows[k]
    if begin < len(cells):
        queue.append((begin, len(cells)))
    queue.reverse()
    passes = []
    while queue:
        k0, k1 = queue.pop()
        try:
            passes.append((k0, k1, capi.batch_layout(cells[k0:k1], cut, cut)))
        except capi.MtpError as e:
            if e.code != -24 or not 0 < e.nfit < k1 - k0:      # a configuration that does not fit on its own
                raise
            queue.append((k0 + e.nfit, k1))
            queue.append((k0, k0 + e.nfit))
    return passes, volume, max_rows


def evaluate_cells(ctx, configs, list_cutoff=7.0, vflag=1, grades=False, max_atoms_per_pass=None, device=None):
    """evaluate_cell for many small periodic cells in one device pass.  `configs` is a sequence of (pos, cell, types)
    (types may be None; a configuration may be empty).  Every configuration gets a slot of its own in one large box
    (mtp_batch_layout: no atom or image of one lies within the list cutoff of another), and one pass is one ghost build
    with the cell looked up per atom (mtp_ghosts_build_batch), one list build, one force launch over all rows, the ghost
    fold, the per-configuration reductions (mtp_batch_reduce, mtp_batch_cfg_grades) and one copy back, with one wait
    each for the ghost count and the list size and one at the end.  The batch is split into passes by
    `max_atoms_per_pass` (owned atoms; a configuration is never split), by the layout's limits (2^26 list cells,
    coordinates within 2048 A) and where owned + ghost atoms would approach 2^31.

    Returns a list of dicts in input order, each with the keys of evaluate_cell: energy, f [n, 3] in the order of `pos`,
    virial [6], volume, x [n, 3] (wrapped into the cell, without the slot origin); with grades=True also grades [n] and
    max_grade (neighbourhood mode) or cfg_grade (configuration mode: the grade of the configuration as a whole,
    pair_mtp_extrapolation.cpp:369-376).  An atom type outside the potential is reported at the final synchronise of
    its pass; the message names the pass."""
    return _cell_passes(ctx, configs, list_cutoff, vflag, grades, max_atoms_per_pass, device, None)


def _cell_passes(ctx, configs, list_cutoff, vflag, grades, max_atoms_per_pass, device, on_pass):
    """the passes of evaluate_cells, shared with select_cells: `on_pass(k0, k1, cf, cf_t, n, stream)` (or None) is called
    once per non-empty pass, after its device work is queued and before the copy back, while the context still holds that
    pass's candidate vectors"""
    import torch
    dev = device or torch.device("cuda:0")
    st = _torch_stream(dev)
    cut = float(list_cutoff)
    cfg_mode = bool(grades) and bool(ctx.pot.info.configuration_mode)
    C = int(ctx.pot.info.coeff_count)
    items, all_cells, natoms = _batch_items(configs)
    passes, volume, max_rows = plan_cell_passes(all_cells, natoms, cut, max_atoms_per_pass)
    ghosts = capi.Ghosts(dev.index or 0)
    buf = _BatchBuffers(torch, dev)
    results = [None] * len(items)
    npass = 0
    na = lambda nall: nall + (nall & 1)
    for k0, k1, lay in passes:
        npass += 1
        ncfg = k1 - k0
        counts = natoms[k0:k1]
        cf = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        n = int(cf[-1])
        if n == 0:
            for k in range(k0, k1):
                results[k] = _empty_result(float(volume[k]), grades, cfg_mode)
            continue
        cf_t = torch.from_numpy(cf).to(dev)
        nall = _pass_ghosts_and_list(ctx, ghosts, buf, items[k0:k1], cf, all_cells[k0:k1], lay, cut, n + int(max_rows[k0:k1].sum()),
                                     lambda rows, first: buf.reserve(rows, ncfg, 10 * na(rows) + 10 + C + (C & 1),
                                                                     7 * n + 8 * ncfg if first else 0), st)
        # f | ev | eatom | vatom | max grade | coeff_ders: one allocation, zeroed by one launch
        m = na(nall)
        work = buf.work[: 10 * m + 10 + C + (C & 1)]
        fall, ev = work[: 3 * nall].view(nall, 3), work[3 * m: 3 * m + 8]
        eatom, vatom = work[3 * m + 8: 4 * m + 8], work[4 * m + 8: 10 * m + 8]
        maxg, coeff = work[10 * m + 8: 10 * m + 9], work[10 * m + 10: 10 * m + 10 + C]
        capi.zero_async(work, stream=st)
        vf = 4 if vflag else 0
        ctx.compute_device_rows(0, n, False, buf.xall, buf.tall, fall, eflag=3, vflag=vf, grade=bool(grades), eatom_t=eatom,
                                vatom_t=vatom if vf else None, ev_t=ev, grades_t=buf.grades if grades and not cfg_mode else None,
                                maxg_t=maxg if grades else None, coeff_t=coeff if cfg_mode else None, stream=st)
        ghosts.reverse_finish(ctx, fall, ev, eflag=3, vflag=vf, stream=st)
        res = buf.res[: 8 * ncfg]
        e_t, v_t, g_t = res[:ncfg], res[ncfg: 7 * ncfg], res[7 * ncfg:]
        if not vf or not grades:
            res.zero_()
        capi.batch_reduce(cf_t, eatom_t=eatom, vatom_t=vatom if vf else None, grades_t=buf.grades if grades and not cfg_mode else None,
                          energy_t=e_t, virial_t=v_t if vf else None, cfg_grade_t=g_t if grades and not cfg_mode else None, stream=st)
        if cfg_mode:
            ctx.batch_cfg_grades(cf_t, n, g_t, stream=st)
        if on_pass is not None:
            on_pass(k0, k1, cf, cf_t, n, st)
        pieces = [buf.xall[:n].reshape(-1), fall[:n].reshape(-1), res] + ([buf.grades[:n]] if grades and not cfg_mode else [])
        nout = sum(int(p.numel()) for p in pieces)
        out = buf.out_host[:nout]
        out.copy_(torch.cat(pieces), non_blocking=True)       # the one copy back, waited for below
        try:
            ctx.synchronize(stream=st)                        # an atom type outside the potential is reported here
        except capi.MtpError as e:
            raise capi.MtpError(e.code, "pass %d (configurations %d to %d): %s" % (npass, k0, k1 - 1, e)) from e
        h = out.numpy()
        xh = h[: 3 * n].reshape(n, 3) - np.repeat(lay["origins"], counts, axis=0)
        fh = h[3 * n: 6 * n].reshape(n, 3).copy()
        eh, vh = h[6 * n: 6 * n + ncfg].copy(), h[6 * n + ncfg: 6 * n + 7 * ncfg].reshape(ncfg, 6).copy()
        ch, gh = h[6 * n + 7 * ncfg: 6 * n + 8 * ncfg].copy(), h[6 * n + 8 * ncfg:].copy()
        for j in range(ncfg):
            a, b = int(cf[j]), int(cf[j + 1])
            r = dict(energy=float(eh[j]), f=fh[a:b], virial=vh[j], volume=float(volume[k0 + j]), x=xh[a:b])
            if grades and cfg_mode:
                r["cfg_grade"] = float(ch[j])
            elif grades:
                r["grades"], r["max_grade"] = gh[a:b], float(ch[j])
            results[k0 + j] = r
    return results


def _batch_items(configs):
    """[(pos [n, 3], types [n])], cells [ncfg, 3, 3] and atom counts of a sequence of (pos, cell, types) configurations"""
    items = []
    for k, c in enumerate(configs):
        pos = np.ascontiguousarray(c[0], dtype=np.float64).reshape(-1, 3)
        types = c[2] if len(c) > 2 else None
        types = np.ones(len(pos), dtype=np.int32) if types is None else np.ascontiguousarray(types, dtype=np.int32).reshape(-1)
        if len(types) != len(pos):
            raise ValueError("configuration %d: %d types for %d atoms" % (k, len(types), len(pos)))
        items.append((pos, types))
    all_cells = np.array([np.asarray(c[1], dtype=np.float64).reshape(3, 3) for c in configs], dtype=np.float64).reshape(-1, 3, 3)
    natoms = np.array([len(it[0]) for it in items], dtype=np.int64)
    return items, all_cells, natoms


def _pass_ghosts_and_list(ctx, ghosts, buf, part, cf, cells, lay, cut, cap, reserve, st):
    """the ghost and list part of one pass over a batch of cells (shared by evaluate_cells / select_cells and design_cells):
    owned positions and types into buf.xall / buf.tall, the ghost build with the cell looked up per atom, ghost types and
    the full list, installed in the context.  `reserve(rows, first)` sizes the caller's buffers for `rows` owned + ghost
    rows (`cap` is an upper bound; the capacity protocol grows them once more if it has to).  Returns nall."""
    torch, dev = buf.torch, buf.dev
    n = int(cf[-1])
    reserve(cap, True)
    buf.xall[:n] = torch.from_numpy(np.concatenate([it[0] for it in part])).to(dev)
    buf.tall[:n] = torch.from_numpy(np.concatenate([it[1] for it in part])).to(dev)
    try:
        nall = ghosts.build_batch(buf.xall, cf, cells, lay["origins"], cut, stream=st)
    except capi.MtpError as e:                            # (the capacity protocol; `cap` is an upper bound)
        if e.code != -24 or ghosts.nall <= buf.cap or ghosts.nall >= 2 ** 31 - 1:
            raise
        keep = buf.xall[:n].clone()
        reserve(ghosts.nall, False)
        buf.xall[:n] = keep
        buf.tall[:n] = torch.from_numpy(np.concatenate([it[1] for it in part])).to(dev)
        nall = ghosts.build_batch(buf.xall, cf, cells, lay["origins"], cut, stream=st)
    ghosts.types(buf.tall, stream=st)
    ctx.build_neighbors_device(buf.xall, n, nall, cut, lay["lo"], lay["hi"], stream=st)
    return nall


def _empty_result(volume, grades, cfg_mode):
    r = dict(energy=0.0, f=np.zeros((0, 3)), virial=np.zeros(6), volume=volume, x=np.zeros((0, 3)))
    if grades and cfg_mode:
        r.update(cfg_grade=0.0)
    elif grades:
        r.update(grades=np.zeros(0), max_grade=0.0)
    return r


def select_cells(ctx, configs, threshold=1.1, out_path=None, list_cutoff=7.0, max_swaps=None, max_pool_bytes=2 ** 31,
                 max_atoms_per_pass=None, device=None, install=False):
    """The selection step of the active-learning loop over a batch of candidate configurations: the passes of
    evaluate_cells(grades=True), every pass's candidate vectors copied into one pool on the device (one row per atom in
    neighbourhood mode, one per configuration -- the sum over its atoms divided by their number -- in configuration mode),
    ONE MaxVol selection over that pool starting from the context's active set (Context.maxvol_select), and, with
    `out_path`, the potential file with the new active set and its inverse (capi.write_selection: the source's text, so
    its coefficients are the file's).  The new set reaches a context by either of two routes: install=True puts it into
    `ctx` (Context.install_selection, after any out_path write) -- plan, list and buffers are kept --, or a new Potential
    and Context are loaded from the written file.  The pool is selected as a whole, because later swaps
    change earlier grades: ValueError when it would exceed `max_pool_bytes` (the selection needs as much again for its
    grade matrix).

    Returns dict(selected: indices of the configurations that own a row now in the active set, ascending; nswaps,
    converged, log_volume_gain = log |det S'| - log |det S|; grade_before [ncfg]: every configuration's grade against the
    old set; max_grade_after: the largest grade of the pool against the new set; active_set, inverse_active_set [C, C];
    slot_source [C]: per slot the configuration whose vector it now holds -- (configuration, atom) in neighbourhood mode --
    or None where the original column was kept; swaps: the log [(pool row, slot, pivot)])."""
    import torch
    dev = device or torch.device("cuda:0")
    _torch_stream(dev)                                       # the pool is filled on this stream
    info = ctx.pot.info
    if not info.has_selection:
        raise capi.MtpError(-23, "select_cells: the potential was loaded without its selection state")
    cfg_mode = bool(info.configuration_mode)
    C = int(info.coeff_count)
    cpad = (C + 15) // 16 * 16
    natoms = np.array([len(np.asarray(c[0], dtype=np.float64).reshape(-1, 3)) for c in configs], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(natoms)])
    nrows = len(natoms) if cfg_mode else int(first[-1])
    if nrows * cpad * 8 > max_pool_bytes:
        raise ValueError("select_cells: a pool of %d candidate vectors needs %d bytes, max_pool_bytes is %d; a pool has to be "
                         "selected as a whole" % (nrows, nrows * cpad * 8, max_pool_bytes))
    pool = torch.zeros((nrows, cpad), dtype=torch.float64, device=dev)

    def on_pass(k0, k1, cf, cf_t, n, st):
        if cfg_mode:
            pool[k0:k1] = ctx.batch_cfg_candidates(cf_t, n, stream=st)
        else:
            pool[int(first[k0]): int(first[k0]) + n] = ctx.candidates()[:n]

    res = _cell_passes(ctx, configs, list_cutoff, 0, True, max_atoms_per_pass, dev, on_pass)
    st = torch.cuda.current_stream(dev).cuda_stream
    sel = ctx.maxvol_select(pool, threshold, max_swaps=max_swaps, stream=st)
    if out_path is not None:
        capi.write_selection(ctx.pot.path, out_path, sel["active_set"], sel["inverse_active_set"])
    if install:
        ctx.install_selection(sel["active_set"], sel["inverse_active_set"], stream=st)
    owner = [None if r < 0 else (int(r) if cfg_mode else int(np.searchsorted(first, r, side="right") - 1))
             for r in sel["slot_source"]]
    source = [None if k is None else (k if cfg_mode else (k, int(r - first[k]))) for k, r in zip(owner, sel["slot_source"])]
    return dict(selected=sorted({k for k in owner if k is not None}), nswaps=sel["nswaps"], converged=sel["converged"],
                log_volume_gain=sel["log_volume_gain"],
                grade_before=np.array([r["cfg_grade"] if cfg_mode else r["max_grade"] for r in res]),
                max_grade_after=sel["max_grade_after"], active_set=sel["active_set"],
                inverse_active_set=sel["inverse_active_set"], slot_source=source, swaps=sel["swaps"])


def _design_passes(ctx, configs, list_cutoff, virial, max_atoms_per_pass, device, begin):
    """The passes design_cells and normal_cells share: ghost build, list build, the design call with the ghost owner map,
    the per-configuration sums (capi.batch_design_reduce) and the synchronise that reports an atom type outside the
    potential.  `begin(plan)` is called once, after the planning and before anything is allocated, with plan = dict(dev,
    stream, cols, ld, natoms, first, passes, pass_atoms, pass_cfgs: the atoms and configurations of the largest pass); it
    raises where the caller's byte bound is exceeded and returns (rows_of, on_pass).  rows_of(k0, k1) gives the ZEROED
    destination (force [3 n, ld], energy [k1 - k0, ld], virial [k1 - k0, 6, ld] or None) of a pass;
    on_pass(k0, k1, force, energy, virial, stream) (or None) runs after the sums are queued, before the synchronise.
    Returns the plan."""
    import torch
    dev = device or torch.device("cuda:0")
    st = _torch_stream(dev)
    cut = float(list_cutoff)
    info = ctx.pot.info
    cols = int(info.species_count + info.alpha_scalar_count)
    ld = cols + (cols & 1)
    items, all_cells, natoms = _batch_items(configs)
    first = np.concatenate([[0], np.cumsum(natoms)]).astype(np.int64)
    passes, _, max_rows = plan_cell_passes(all_cells, natoms, cut, max_atoms_per_pass)
    plan = dict(dev=dev, stream=st, cols=cols, ld=ld, natoms=natoms, first=first, passes=passes,
                pass_atoms=max([int(first[k1] - first[k0]) for k0, k1, _ in passes], default=0),
                pass_cfgs=max([k1 - k0 for k0, k1, _ in passes], default=0))
    rows_of, on_pass = begin(plan)
    ghosts = capi.Ghosts(dev.index or 0)
    buf = _BatchBuffers(torch, dev)
    npass = 0
    for k0, k1, lay in passes:
        npass += 1
        cf = (first[k0:k1 + 1] - first[k0]).astype(np.int32)
        n = int(cf[-1])
        if n == 0:
            continue
        cf_t = torch.from_numpy(cf).to(dev)
        # per-atom rows of the pass: basis [n, ld] | virial [n, 6, ld]
        nall = _pass_ghosts_and_list(ctx, ghosts, buf, items[k0:k1], cf, all_cells[k0:k1], lay, cut, n + int(max_rows[k0:k1].sum()),
                                     lambda rows, first_: buf.reserve(rows, 0, (7 if virial else 1) * n * ld, 0), st)
        basis = buf.work[: n * ld].view(n, ld)
        vatom = buf.work[n * ld: 7 * n * ld].view(n, 6, ld) if virial else None
        owner, nown = ghosts.owner(stream=st)
        assert nown == nall
        force, energy, vir = rows_of(k0, k1)
        ctx.design_rows(0, n, buf.xall, buf.tall, force, n, ld, basis_t=basis, virial_t=vatom, owner=owner, stream=st)
        capi.batch_design_reduce(cf_t, ld, basis_t=basis, virial_atom_t=vatom, energy_t=energy,
                                 virial_t=vir if virial else None, stream=st)
        if on_pass is not None:
            on_pass(k0, k1, force, energy, vir, st)
        try:
            ctx.synchronize(stream=st)                        # an atom type outside the potential is reported here
        except capi.MtpError as e:
            raise capi.MtpError(e.code, "pass %d (configurations %d to %d): %s" % (npass, k0, k1 - 1, e)) from e
    torch.cuda.current_stream(dev).synchronize()
    return plan


def design_cells(ctx, configs, list_cutoff=7.0, virial=True, max_design_bytes=2 ** 31, max_atoms_per_pass=None, device=None):
    """The design matrix of the linear refit over a batch of configurations (include/mtp_mi355x.h, "linear refit"): the
    passes of evaluate_cells -- ghost build, list build -- with the design call (Context.design_rows, the ghost owner
    map folding every neighbour's term onto its owned row) in place of the force call, then the per-configuration sums
    (capi.batch_design_reduce).  Columns are [species (Sp) | moments (S)]; with theta = the context's species_coeffs and
    moment_coeffs (Context.coeffs), energy @ theta, force @ theta and virial @ theta are what evaluate_cells returns.

    Returns dict(energy [ncfg, Sp + S], force [3 sum n, Sp + S] (row 3 (cfg_first[k] + a) + c: atom a of configuration k,
    component c, atoms in the order of `pos`), virial [ncfg, 6, Sp + S] (None with virial=False), cfg_first [ncfg + 1],
    columns = Sp + S) as DEVICE tensors (views of allocations whose rows are `ld` = columns rounded up to even apart),
    plus natoms.  ValueError when these three matrices together with the per-atom basis and virial rows of the largest
    pass (7 n ld doubles for a pass of n atoms; `max_atoms_per_pass` bounds them) would exceed `max_design_bytes`: the caller
    shards the training set, or fits through normal_cells, which keeps no matrix.  An atom type outside the potential is
    reported at the synchronise of its pass; the message names it."""
    import torch
    out = {}

    def begin(plan):
        dev, ld, first = plan["dev"], plan["ld"], plan["first"]
        ncfg_all, ntot, pass_atoms = len(plan["natoms"]), int(first[-1]), plan["pass_atoms"]
        # the three matrices and, beside them, the per-atom basis and virial rows of the largest pass
        need = 8 * ld * (ncfg_all + 3 * ntot + (6 * ncfg_all if virial else 0) + (7 if virial else 1) * pass_atoms)
        if need > max_design_bytes:
            raise ValueError("design_cells: the design matrix of %d configurations with %d atoms (and the per-atom rows of its "
                             "largest pass, %d atoms) needs %d bytes, max_design_bytes is %d; shard the training set, or lower "
                             "max_atoms_per_pass" % (ncfg_all, ntot, pass_atoms, need, max_design_bytes))
        energy = torch.zeros((ncfg_all, ld), dtype=torch.float64, device=dev)
        force = torch.zeros((3 * ntot, ld), dtype=torch.float64, device=dev)
        vir = torch.zeros((ncfg_all, 6, ld), dtype=torch.float64, device=dev) if virial else None
        out.update(energy=energy, force=force, vir=vir)
        return (lambda k0, k1: (force[3 * int(first[k0]): 3 * int(first[k1])], energy[k0:k1], vir[k0:k1] if virial else None)), None

    plan = _design_passes(ctx, configs, list_cutoff, virial, max_atoms_per_pass, device, begin)
    cols = plan["cols"]
    return dict(energy=out["energy"][:, :cols], force=out["force"][:, :cols], virial=out["vir"][:, :, :cols] if virial else None,
                cfg_first=torch.from_numpy(plan["first"].astype(np.int32)).to(plan["dev"]), columns=cols, natoms=plan["natoms"])


def fit_linear(ctx, configs, labels, weights=(1.0, 0.01, 0.001), rcond=1e-12, out_path=None, list_cutoff=7.0,
               max_design_bytes=2 ** 31, max_atoms_per_pass=None, device=None, install=False, method="svd", state=None):
    """The linear refit: species_coeffs and moment_coeffs fitted to reference energies, forces and virials with the radial
    coefficients fixed.  labels[k] = dict(energy=float or None, f=[n, 3] or None, virial=[6] or None) for configs[k]
    (virial in the sign and order evaluate_cells returns).  With N_k atoms in configuration k the rows of design_cells
    and their labels are scaled by sqrt(w_e) / N_k (energy), sqrt(w_f) (forces) and sqrt(w_s) / N_k (virial), weights =
    (w_e, w_f, w_s) -- this project's definition, not pinned to MLIP's --, rows without a label are dropped, and the
    solve is for the CHANGE of the coefficients: delta = lstsq(A_w, y_w - A_w theta_0, rcond), theta = theta_0 + delta,
    theta_0 the context's current coefficients (Context.coeffs: the file's until an install), so that directions the data do not determine (the complete tables are
    rank deficient by construction) keep their values.  The weighted matrix is copied to the host and solved with
    numpy.linalg.lstsq (SVD); it is bounded by max_design_bytes and the fit runs once per round.

    method="normal" keeps no design matrix: normal_cells adds every pass's rows to the double-double normal equations on
    the device (max_design_bytes is its max_bytes and bounds one pass, the state and its workspace), and solve_normal
    factors them on the host and hands the triangular factor to the same SVD solve -- the same coefficients from cols^2
    numbers instead of rows x cols.  `state` (a NormalState of an earlier call, method="normal" only) is extended by these
    configurations, so that a round costs its new configurations only; the state is returned under "state", with
    "dropped_columns" and "pivot_ratios" beside the keys below.

    Returns dict(species_coeffs, moment_coeffs, rank, singular_values, rmse_before, rmse_after: dicts energy (per atom),
    force, virial (per atom) over the labelled rows, None for a kind without labels) and, with out_path, writes the
    potential file: through capi.write_coeffs while the context's radial block is the file's, through
    capi.write_all_coeffs with the context's radial block once an install has made them differ (the written file is always
    the context's model).  "wrote" is the return value of the writer used; both return 0, or
    capi.WROTE_WITHOUT_SELECTION where the source's #MVS tail was left out.  The result reaches a context by either of two routes: install=True puts it
    into `ctx` (Context.install_coeffs, after any out_path write), or a new Potential and Context are loaded from the written
    file.  Either way the active set's columns are candidate vectors of the OLD coefficients and are stale: rebuilding the
    set is the caller's select_cells call, not something an install does."""
    if len(labels) != len(configs):
        raise ValueError("fit_linear: %d labels for %d configurations" % (len(labels), len(configs)))
    if method not in ("svd", "normal") or (state is not None and method != "normal"):
        raise ValueError("fit_linear: method is 'svd' or 'normal', and a state goes with 'normal' only")
    want_v = float(weights[2]) > 0.0 and any(l.get("virial") is not None for l in labels)
    t = ctx.coeffs()
    theta0 = np.concatenate([t["species_coeffs"], t["moment_coeffs"]])
    if method == "normal":
        state = normal_cells(ctx, configs, labels, state=state, list_cutoff=list_cutoff, virial=want_v, max_bytes=max_design_bytes,
                             max_atoms_per_pass=max_atoms_per_pass, device=device)
        res = solve_normal(state, theta0, weights, rcond)
        res["state"] = state
    else:
        d = design_cells(ctx, configs, list_cutoff=list_cutoff, virial=want_v, max_design_bytes=max_design_bytes,
                         max_atoms_per_pass=max_atoms_per_pass, device=device)
        res = solve_linear(d["energy"].cpu().numpy(), d["force"].cpu().numpy(), d["virial"].cpu().numpy() if want_v else None,
                           d["natoms"], labels, theta0, weights, rcond)
    Sp = int(ctx.pot.info.species_count)
    theta = res.pop("theta")
    res.update(species_coeffs=theta[:Sp].copy(), moment_coeffs=theta[Sp:].copy())
    if out_path is not None:
        if np.array_equal(t["radial_coeffs"], ctx.pot.tables()["radial_coeffs"]):
            res["wrote"] = capi.write_coeffs(ctx.pot.path, out_path, res["moment_coeffs"], res["species_coeffs"])
        else:                                                   # (an installed radial block: the file's is not the context's)
            res["wrote"] = capi.write_all_coeffs(ctx.pot.path, out_path, res["moment_coeffs"], res["species_coeffs"], t["radial_coeffs"])
    if install:                                                 # (design_cells ended in a synchronise of the current stream)
        ctx.install_coeffs(species_coeffs=res["species_coeffs"], moment_coeffs=res["moment_coeffs"])
    return res


def solve_linear(energy, force, virial, natoms, labels, theta0, weights=(1.0, 0.01, 0.001), rcond=1e-12):
    """The host part of fit_linear (numpy only): energy [ncfg, cols], force [3 sum n, cols], virial [ncfg, 6, cols] or None
    are the design matrices of design_cells, natoms [ncfg].  Labelled rows are scaled as fit_linear documents, and
    delta = lstsq(A_w, y_w - A_w theta0, rcond) (SVD).  Returns dict(theta = theta0 + delta, rank, singular_values,
    rmse_before, rmse_after)."""
    w_e, w_f, w_s = (float(w) for w in weights)
    natoms = np.asarray(natoms, dtype=np.int64)
    ncfg = len(natoms)
    first = np.concatenate([[0], np.cumsum(natoms)])
    cols = energy.shape[1]
    e_rows = [k for k in range(ncfg) if labels[k].get("energy") is not None and natoms[k] > 0 and w_e > 0.0]
    f_cfg = [k for k in range(ncfg) if labels[k].get("f") is not None and natoms[k] > 0 and w_f > 0.0]
    v_cfg = [k for k in range(ncfg) if virial is not None and w_s > 0.0 and labels[k].get("virial") is not None and natoms[k] > 0]
    blocks, ys, scales, kinds = [], [], [], []
    if e_rows:
        blocks.append(energy[e_rows])
        ys.append(np.array([float(labels[k]["energy"]) for k in e_rows]))
        scales.append(np.sqrt(w_e) / natoms[e_rows])
        kinds.append(("energy", w_e))
    if f_cfg:
        for k in f_cfg:
            if np.shape(labels[k]["f"]) != (natoms[k], 3):
                raise ValueError("fit_linear: labels[%d]['f'] must be [%d, 3]" % (k, natoms[k]))
        rows = np.concatenate([np.arange(3 * first[k], 3 * first[k + 1]) for k in f_cfg])
        blocks.append(force[rows])
        ys.append(np.concatenate([np.asarray(labels[k]["f"], dtype=np.float64).reshape(-1) for k in f_cfg]))
        scales.append(np.full(len(rows), np.sqrt(w_f)))
        kinds.append(("force", w_f))
    if v_cfg:
        blocks.append(virial[v_cfg].reshape(-1, cols))
        ys.append(np.concatenate([np.asarray(labels[k]["virial"], dtype=np.float64).reshape(6) for k in v_cfg]))
        scales.append(np.repeat(np.sqrt(w_s) / natoms[v_cfg], 6))
        kinds.append(("virial", w_s))
    if not blocks:
        raise ValueError("fit_linear: no labelled rows with a positive weight")
    scale = np.concatenate(scales)
    Aw = np.concatenate(blocks) * scale[:, None]
    yw = np.concatenate(ys) * scale
    theta0 = np.asarray(theta0, dtype=np.float64)
    resid0 = yw - Aw @ theta0
    delta, _, rank, sv = np.linalg.lstsq(Aw, resid0, rcond=rcond)
    theta = theta0 + delta
    resid1 = yw - Aw @ theta

    def rmse(resid):
        # per kind, with the weight taken out: energy and virial per atom, forces per component
        out, at = dict(energy=None, force=None, virial=None), 0
        for (kind, w), sc in zip(kinds, scales):
            out[kind] = float(np.sqrt(np.mean((resid[at:at + len(sc)] / np.sqrt(w)) ** 2)))
            at += len(sc)
        return out

    return dict(theta=theta, rank=int(rank), singular_values=sv, rmse_before=rmse(resid0), rmse_after=rmse(resid1))


# ---- the same fit without the design matrix: double-double normal equations (include/mtp_mi355x.h) -----------------------
def design_fingerprint(ctx, list_cutoff=7.0):
    """sha256 over everything the design matrix of a configuration depends on: the context's CURRENT radial coefficients,
    scaling, the cutoffs, the species count, the alpha tables and the list cutoff.  The linear coefficients do not enter:
    a NormalState stays valid across installs of species_coeffs / moment_coeffs and goes stale with the radial block."""
    import hashlib
    t, i = ctx.pot.tables(), ctx.pot.info
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(ctx.coeffs()["radial_coeffs"], dtype=np.float64).tobytes())
    h.update(np.array([i.scaling, i.min_cutoff, i.max_cutoff, float(list_cutoff)], dtype=np.float64).tobytes())
    h.update(np.array([i.species_count, i.radial_basis_size, i.radial_func_count], dtype=np.int64).tobytes())
    for key in ("alpha_index_basic", "alpha_index_times", "alpha_moment_mapping"):
        h.update(np.ascontiguousarray(t[key], dtype=np.int32).tobytes())
    return h.hexdigest()


class NormalState:
    """The normal equations of a training set on the device: `normal` (capi.Normal: per kind the augmented Gram matrix in
    double-double and its row count), ncols and the fingerprint (design_fingerprint; None for a state that
    normal_from_design made from bare matrices) of what the rows depended on.  Neither weights nor coefficients enter, so a
    state is extended round by round (normal_cells(state=...)) and solved for any weights (solve_normal)."""

    def __init__(self, normal, fingerprint, device):
        self.normal, self.fingerprint, self.device = normal, fingerprint, device
        self.ncols = normal.ncols

    def arrays(self):
        """host copies (hi [3, n, n], lo [3, n, n], counts [3]) after a synchronise of the current stream"""
        return self.normal.get(stream=_torch_stream(self.device))

    @property
    def counts(self):
        """rows that entered per kind: dict(energy, force, virial)"""
        return dict(zip(capi.NORMAL_KINDS, (int(c) for c in self.normal.get(stream=_torch_stream(self.device))[2])))

    @staticmethod
    def write_arrays(path, hi, lo, counts, fingerprint):
        """the file of save(): an .npz at exactly `path` (host only)"""
        with open(path, "wb") as f:
            np.savez(f, hi=np.asarray(hi, dtype=np.float64), lo=np.asarray(lo, dtype=np.float64),
                     counts=np.asarray(counts, dtype=np.int64), fingerprint=np.array("" if fingerprint is None else fingerprint))

    @staticmethod
    def read_arrays(path):
        """(hi, lo, counts, fingerprint or None) of a file of save() (host only)"""
        with np.load(path) as z:
            return z["hi"], z["lo"], z["counts"], str(z["fingerprint"]) or None

    def save(self, path):
        """hi, lo, counts and the fingerprint as an .npz, bit for bit"""
        NormalState.write_arrays(path, *self.arrays(), self.fingerprint)

    @staticmethod
    def load(path, device=None, workspace_bytes=0):
        import torch
        dev = device or torch.device("cuda:0")
        hi, lo, counts, fp = NormalState.read_arrays(path)
        normal = capi.Normal(hi.shape[-1] - 1, dev.index or 0, workspace_bytes)
        normal.set(hi, lo, counts, stream=_torch_stream(dev))
        return NormalState(normal, fp, dev)


def _normal_labels(labels, natoms):
    """scale and target of every row of the three kinds (the rules of _label_arrays; no weights): energy rows 1 / N_k and
    E_k, force rows 1 and f, virial rows 1 / N_k and the six components; scale 0 where there is no label or no atom"""
    first, e_ref, e_on, f_ref, f_on, v_ref, v_on = _label_arrays(labels, natoms, (1.0, 1.0, 1.0))
    inv = np.where(natoms > 0, 1.0 / np.maximum(natoms, 1), 0.0)
    return first, (e_on * inv, e_ref), (np.repeat(f_on, 3), f_ref.reshape(-1)), (np.repeat(v_on * inv, 6), v_ref.reshape(-1))


def _normal_state(state, ncols, fingerprint, dev, budget, who):
    """the state to extend, or a new one whose workspace takes at most a quarter of `budget` bytes"""
    if state is None:
        return NormalState(capi.Normal(ncols, dev.index or 0, max(1, int(budget) // 4)), fingerprint, dev)
    if state.ncols != ncols or state.fingerprint != fingerprint:
        raise ValueError("%s: the state was accumulated for %d columns with fingerprint %s, these rows have %d columns and "
                         "fingerprint %s (a state is stale once the radial coefficients, the cutoffs or the tables changed)"
                         % (who, state.ncols, state.fingerprint, ncols, fingerprint))
    return state


def normal_cells(ctx, configs, labels, state=None, list_cutoff=7.0, virial=True, max_bytes=2 ** 31, max_atoms_per_pass=None,
                 device=None):
    """The normal equations of the linear refit over a batch of configurations, WITHOUT the design matrix: the passes of
    design_cells with the three matrices of one pass only, and after each pass's sums three Normal.accumulate calls --
    energy rows with scale 1 / N_k and target E_k, force rows with scale 1 and target f, virial rows with scale 1 / N_k,
    six per configuration.  The scale is 0 (the row is skipped) where the label is None or the configuration is empty;
    the weights of a fit are NOT applied here (solve_normal applies them).  labels as for fit_linear.

    `max_bytes` bounds the rows of one pass (8 ld (7 cfgs + 10 atoms) with virials), the state (48 n^2, n = columns + 1) and
    its workspace together; nothing grows with the number of configurations.  With max_atoms_per_pass=None the passes are
    sized to fit.  ValueError when a single pass cannot fit, when labels are malformed, or when `state` (a NormalState to
    extend by these rows) carries another fingerprint (design_fingerprint).  Returns the NormalState."""
    import torch
    if len(labels) != len(configs):
        raise ValueError("normal_cells: %d labels for %d configurations" % (len(labels), len(configs)))
    dev = device or torch.device("cuda:0")
    info = ctx.pot.info
    cols = int(info.species_count + info.alpha_scalar_count)
    ld = cols + (cols & 1)
    per_atom, per_cfg = 8 * ld * (3 + (7 if virial else 1)) + 48, 8 * ld * (7 if virial else 1) + 112
    state = _normal_state(state, cols, design_fingerprint(ctx, list_cutoff), dev, max_bytes, "normal_cells")
    ninfo = state.normal.info()
    fixed = ninfo["state_bytes"] + ninfo["workspace_bytes"]
    if max_atoms_per_pass is None:
        max_atoms_per_pass = max(1, (int(max_bytes) - fixed) // (per_atom + per_cfg))
    natoms = np.array([len(np.asarray(c[0], dtype=np.float64).reshape(-1, 3)) for c in configs], dtype=np.int64)
    first, (e_sc, e_tg), (f_sc, f_tg), (v_sc, v_tg) = _normal_labels(labels, natoms)
    buf = {}

    def begin(plan):
        need = fixed + per_atom * plan["pass_atoms"] + per_cfg * plan["pass_cfgs"]
        if need > max_bytes:
            raise ValueError("normal_cells: the state (%d bytes), its workspace (%d) and the rows of the largest pass (%d atoms "
                             "in %d configurations) need %d bytes, max_bytes is %d; lower max_atoms_per_pass"
                             % (ninfo["state_bytes"], ninfo["workspace_bytes"], plan["pass_atoms"], plan["pass_cfgs"], need, max_bytes))
        z = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        buf.update(force=z(3 * plan["pass_atoms"], ld), energy=z(plan["pass_cfgs"], ld),
                   vir=z(plan["pass_cfgs"], 6, ld) if virial else None)

        def rows_of(k0, k1):
            n, ncfg = int(first[k1] - first[k0]), k1 - k0
            force = buf["force"][: 3 * n]
            capi.zero_async(force, stream=plan["stream"])      # (the design call accumulates into its force rows)
            return force, buf["energy"][:ncfg], buf["vir"][:ncfg] if virial else None

        def on_pass(k0, k1, force, energy, vir, st):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            a, b = int(first[k0]), int(first[k1])
            state.normal.accumulate(0, k1 - k0, ld, energy, up(e_sc[k0:k1]), up(e_tg[k0:k1]), stream=st)
            state.normal.accumulate(1, 3 * (b - a), ld, force, up(f_sc[3 * a: 3 * b]), up(f_tg[3 * a: 3 * b]), stream=st)
            if virial:
                state.normal.accumulate(2, 6 * (k1 - k0), ld, vir, up(v_sc[6 * k0: 6 * k1]), up(v_tg[6 * k0: 6 * k1]), stream=st)

        return rows_of, on_pass

    _design_passes(ctx, configs, list_cutoff, virial, max_atoms_per_pass, dev, begin)
    return state


def normal_from_design(d, labels, state=None):
    """The accumulation of normal_cells from the DEVICE tensors design_cells returned (`d`), so that both solvers can be
    handed the same rows.  A new state carries no fingerprint (None): normal_cells does not extend it."""
    natoms = np.asarray(d["natoms"], dtype=np.int64)
    if len(labels) != len(natoms):
        raise ValueError("normal_from_design: %d labels for %d configurations" % (len(labels), len(natoms)))
    e, f, v = d["energy"], d["force"], d["virial"]
    dev, cols, ld = e.device, int(d["columns"]), int(e.stride(0))
    st = _torch_stream(dev)
    state = _normal_state(state, cols, None if state is None else state.fingerprint, dev, 2 ** 30, "normal_from_design")
    _, e_l, f_l, v_l = _normal_labels(labels, natoms)
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    state.normal.accumulate(0, len(natoms), ld, e, up(e_l[0]), up(e_l[1]), stream=st)
    state.normal.accumulate(1, int(f.shape[0]), ld, f, up(f_l[0]), up(f_l[1]), stream=st)
    if v is not None:
        state.normal.accumulate(2, 6 * len(natoms), ld, v, up(v_l[0]), up(v_l[1]), stream=st)
    torch.cuda.current_stream(dev).synchronize()
    return state


def solve_normal(state, theta0, weights=(1.0, 0.01, 0.001), rcond=1e-12, drop=2.0 ** -80):
    """The host part of fit_linear(method="normal"): `state` is a NormalState, or host arrays (hi [3, n, n], lo [3, n, n],
    counts [3]).  capi.normal_factor forms G = sum_k w_k G_k and its diagonally pivoted Cholesky factor R in double-double
    -- a column is dropped when its pivot falls to `drop` times its original diagonal --, then delta = lstsq(R, q, rcond)
    (SVD) with q = Q^T y - R theta0: R has the singular values of the weighted design matrix, and delta is what solve_linear
    computes from that matrix.  Other weights cost this call only.

    Returns the keys of solve_linear -- theta = theta0 + delta, rank, singular_values (of R), rmse_before, rmse_after: per
    kind sqrt(capi.normal_quadratic / rows), None for a kind without rows or with weight 0 -- and dropped_columns,
    pivot_ratios (the kept pivots' ratios in elimination order, then the dropped columns')."""
    hi, lo, counts = state.arrays() if isinstance(state, NormalState) else state
    w = [float(x) for x in weights]
    theta0 = np.asarray(theta0, dtype=np.float64).reshape(-1)
    live = [k for k in range(3) if w[k] > 0.0 and int(counts[k]) > 0]
    if min(w) < 0.0 or not live:
        raise ValueError("fit_linear: no labelled rows with a positive weight")
    f = capi.normal_factor(hi, lo, [w[k] if k in live else 0.0 for k in range(3)], theta0, drop)
    delta, _, rank, sv = np.linalg.lstsq(f["R"], f["q"], rcond=rcond)
    theta = theta0 + delta

    def rmse(th):
        return {name: float(np.sqrt(capi.normal_quadratic(hi[k], lo[k], th) / int(counts[k]))) if k in live else None
                for k, name in enumerate(capi.NORMAL_KINDS)}

    return dict(theta=theta, rank=int(rank), singular_values=sv, rmse_before=rmse(theta0), rmse_after=rmse(theta),
                dropped_columns=f["dropped_columns"], pivot_ratios=f["pivot_ratios"])


def _label_arrays(labels, natoms, weights):
    """host arrays of the labels and the masks of the labelled kinds (the rules of solve_linear: a kind counts where its
    label is not None, its weight positive and the configuration not empty)"""
    w_e, w_f, w_s = (float(w) for w in weights)
    ncfg = len(natoms)
    first = np.concatenate([[0], np.cumsum(natoms)]).astype(np.int64)
    e_ref, e_on = np.zeros(ncfg), np.zeros(ncfg)
    f_ref, f_on = np.zeros((int(first[-1]), 3)), np.zeros(int(first[-1]))
    v_ref, v_on = np.zeros((ncfg, 6)), np.zeros(ncfg)
    for k, l in enumerate(labels):
        if natoms[k] == 0:
            continue
        if l.get("energy") is not None and w_e > 0.0:
            e_ref[k], e_on[k] = float(l["energy"]), 1.0
        if l.get("f") is not None and w_f > 0.0:
            if np.shape(l["f"]) != (natoms[k], 3):
                raise ValueError("loss_cells: labels[%d]['f'] must be [%d, 3]" % (k, natoms[k]))
            f_ref[first[k]:first[k + 1]], f_on[first[k]:first[k + 1]] = np.asarray(l["f"], dtype=np.float64), 1.0
        if l.get("virial") is not None and w_s > 0.0:
            v_ref[k], v_on[k] = np.asarray(l["virial"], dtype=np.float64).reshape(6), 1.0
    return first, e_ref, e_on, f_ref, f_on, v_ref, v_on


def loss_cells(ctx, configs, labels, theta=None, weights=(1.0, 0.01, 0.001), grad=True, list_cutoff=7.0, max_atoms_per_pass=None,
               device=None):
    """The training loss and its gradient with respect to ALL coefficients (include/mtp_mi355x.h, "training gradient").
    `theta` [C] in candidate-vector order [radial | species | moments] (None: the context's own, Context.theta()); the
    context's force tables are not involved.  The loss is the objective fit_linear minimises, with N_k atoms in
    configuration k and weights = (w_e, w_f, w_s):
        L = sum_k [ w_e ((E_k - E*_k) / N_k)^2 + w_f sum |F - F*|^2 + w_s sum_6 ((V_k - V*_k) / N_k)^2 ]  over the labelled kinds.
    The passes are those of evaluate_cells and design_cells (ghost build, list build, the ghost owner map).  Per pass: the
    value kernel (Context.train_value), per-configuration totals (capi.batch_reduce), residuals and cotangents
    ebar_i = 2 w_e (E_k - E*_k) / N_k^2, fbar_j = 2 w_f (F_j - F*_j), vbar_i = 2 w_s (V_k - V*_k) / N_k^2 (torch, on the
    device), the vjp kernel (Context.train_vjp) and the per-configuration sums of its rows (capi.batch_design_reduce).

    Returns dict(loss, grad [C] host float64 (None with grad=False), grad_cfg [ncfg, C] device (None with grad=False), rmse:
    dict energy (per atom), force, virial (per atom) over the labelled rows as fit_linear reports them, None for a kind
    without labels; energy [ncfg], forces [sum n, 3] in the order of `pos`, virial [ncfg, 6] as host arrays)."""
    import torch
    if len(labels) != len(configs):
        raise ValueError("loss_cells: %d labels for %d configurations" % (len(labels), len(configs)))
    dev = device or torch.device("cuda:0")
    st = _torch_stream(dev)
    cut = float(list_cutoff)
    info = ctx.pot.info
    C = int(info.species_count ** 2 * info.radial_func_count * info.radial_basis_size + info.species_count + info.alpha_scalar_count)
    ld = C + (C & 1)
    theta_h = ctx.theta() if theta is None else np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
    if len(theta_h) != C:
        raise ValueError("loss_cells: theta has %d entries, the potential has C = %d coefficients" % (len(theta_h), C))
    w_e, w_f, w_s = (float(w) for w in weights)
    items, all_cells, natoms = _batch_items(configs)
    ncfg_all = len(items)
    first, e_ref, e_on, f_ref, f_on, v_ref, v_on = _label_arrays(labels, natoms, weights)
    ntot = int(first[-1])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    theta_t = to(theta_h)
    e_ref_t, e_on_t, f_ref_t, f_on_t, v_ref_t, v_on_t = to(e_ref), to(e_on), to(f_ref), to(f_on), to(v_ref), to(v_on)
    inv_n = to(1.0 / np.maximum(natoms, 1).astype(np.float64))
    counts_t = to(natoms)
    energy = torch.zeros(ncfg_all, dtype=torch.float64, device=dev)
    virial = torch.zeros((ncfg_all, 6), dtype=torch.float64, device=dev)
    forces = torch.zeros((ntot, 3), dtype=torch.float64, device=dev)
    grad_cfg = torch.zeros((ncfg_all, ld), dtype=torch.float64, device=dev) if grad else None
    passes, _, max_rows = plan_cell_passes(all_cells, natoms, cut, max_atoms_per_pass)
    ghosts = capi.Ghosts(dev.index or 0)
    buf = _BatchBuffers(torch, dev)
    npass = 0
    for k0, k1, lay in passes:
        npass += 1
        cf = (first[k0:k1 + 1] - first[k0]).astype(np.int32)
        n = int(cf[-1])
        if n == 0:
            continue
        a0, a1 = int(first[k0]), int(first[k1])
        cf_t = torch.from_numpy(cf).to(dev)
        nall = _pass_ghosts_and_list(ctx, ghosts, buf, items[k0:k1], cf, all_cells[k0:k1], lay, cut, n + int(max_rows[k0:k1].sum()),
                                     lambda rows, first_: buf.reserve(rows, 0, 0, 0), st)
        owner, nown = ghosts.owner(stream=st)
        assert nown == nall
        eatom = torch.empty(n, dtype=torch.float64, device=dev)
        vatom = torch.empty((n, 6), dtype=torch.float64, device=dev)
        f_pass = forces[a0:a1]                                # (zero: accumulated into)
        ctx.train_value(0, n, buf.xall, buf.tall, theta_t, f_pass, n, eatom_t=eatom, vatom_t=vatom, owner=owner, stream=st)
        capi.batch_reduce(cf_t, eatom_t=eatom, vatom_t=vatom, energy_t=energy[k0:k1], virial_t=virial[k0:k1], stream=st)
        if grad:
            reps = counts_t[k0:k1]
            ebar = torch.repeat_interleave(2.0 * w_e * (energy[k0:k1] - e_ref_t[k0:k1]) * e_on_t[k0:k1] * inv_n[k0:k1] ** 2, reps)
            vbar = torch.repeat_interleave(2.0 * w_s * (virial[k0:k1] - v_ref_t[k0:k1]) * (v_on_t[k0:k1] * inv_n[k0:k1] ** 2)[:, None],
                                           reps, dim=0).contiguous()
            fbar = (2.0 * w_f * (f_pass - f_ref_t[a0:a1]) * f_on_t[a0:a1, None]).contiguous()
            rows = torch.empty((n, ld), dtype=torch.float64, device=dev)
            ctx.train_vjp(0, n, buf.xall, buf.tall, theta_t, rows, n, ld, ebar_t=ebar, fbar_t=fbar, vbar_t=vbar, owner=owner,
                          stream=st)
            capi.batch_design_reduce(cf_t, ld, basis_t=rows, energy_t=grad_cfg[k0:k1], stream=st)
        try:
            ctx.synchronize(stream=st)                        # an atom type outside the potential is reported here
        except capi.MtpError as e:
            raise capi.MtpError(e.code, "pass %d (configurations %d to %d): %s" % (npass, k0, k1 - 1, e)) from e
    re = (energy - e_ref_t) * e_on_t * inv_n
    rf = (forces - f_ref_t) * f_on_t[:, None]
    rv = (virial - v_ref_t) * (v_on_t * inv_n)[:, None]
    sums = torch.stack([(re * re).sum(), (rf * rf).sum(), (rv * rv).sum()]).cpu().numpy()
    torch.cuda.current_stream(dev).synchronize()
    loss = float(w_e * sums[0] + w_f * sums[1] + w_s * sums[2])
    nrow = (e_on.sum(), 3.0 * f_on.sum(), 6.0 * v_on.sum())
    rmse = {k: (float(np.sqrt(s / m)) if m > 0 else None) for k, s, m in zip(("energy", "force", "virial"), sums, nrow)}
    return dict(loss=loss, grad=grad_cfg.sum(0)[:C].cpu().numpy() if grad else None, grad_cfg=grad_cfg[:, :C] if grad else None,
                rmse=rmse, energy=energy.cpu().numpy(), forces=forces.cpu().numpy(), virial=virial.cpu().numpy())


def minimize_lbfgs(fun, theta0, mask=None, max_iter=200, history_size=20, tolerance_grad=1e-10, tolerance_change=0.0, max_ls=25):
    """The optimiser of fit_full on its own (host only): torch.optim.LBFGS with the strong-Wolfe line search on a CPU
    float64 tensor, one L-BFGS iteration (with up to max_ls line-search evaluations) per outer step so that the loss at the
    start of every iteration is recorded; the optimiser's state (curvature pairs, step length) carries over between them.
    fun(theta [C] numpy) -> (loss, grad [C] numpy); entries of the gradient where `mask` is False are zeroed (those
    coefficients do not move).  Stops after max_iter iterations, or when the largest gradient entry at the start of an
    iteration is at most tolerance_grad, or when the loss changed by at most tolerance_change over the last iteration.
    Returns (theta [C], history: the loss at the start of every iteration and the loss at the returned theta)."""
    import torch
    p = torch.tensor(np.asarray(theta0, dtype=np.float64).reshape(-1), dtype=torch.float64, requires_grad=True)
    keep = None if mask is None else torch.from_numpy(np.asarray(mask, dtype=np.float64))
    opt = torch.optim.LBFGS([p], lr=1.0, max_iter=1, max_eval=int(max_ls) + 1, history_size=history_size, tolerance_grad=0.0,
                            tolerance_change=0.0, line_search_fn="strong_wolfe")
    seen = []                                                 # (loss, largest gradient entry) of this step's evaluations

    def closure():
        opt.zero_grad()
        loss, g = fun(p.detach().numpy().copy())
        g = torch.from_numpy(np.asarray(g, dtype=np.float64).reshape(-1).copy())
        p.grad = g if keep is None else g * keep
        seen.append((float(loss), float(p.grad.abs().max())))
        return torch.tensor(float(loss), dtype=torch.float64)

    history = []
    for _ in range(int(max_iter)):
        del seen[:]
        history.append(float(opt.step(closure)))
        if seen[0][1] <= tolerance_grad or (len(history) > 1 and abs(history[-2] - history[-1]) <= tolerance_change):
            break
    theta = p.detach().numpy().copy()
    history.append(float(fun(theta)[0]))
    return theta, history


def fit_full(ctx, configs, labels, weights=(1.0, 0.01, 0.001), theta0=None, fit=("radial", "species", "moments"), max_iter=200,
             out_path=None, list_cutoff=7.0, max_atoms_per_pass=None, history_size=20, tolerance_grad=1e-10, tolerance_change=0.0,
             device=None, install=False):
    """Non-linear training: ALL coefficients -- the radial block included -- fitted to reference energies, forces and
    virials by L-BFGS (minimize_lbfgs) on the loss of loss_cells, whose closure is one loss_cells call on the device.
    labels and weights as for fit_linear; theta0 [C] in candidate-vector order (None: the context's coefficients); `fit`
    names the blocks that move, the gradient of the others is zeroed.

    Returns dict(theta [C], radial_coeffs [Sp, Sp, Mu, R], species_coeffs, moment_coeffs, history: the loss at the start of
    every iteration and at the end, rmse_before, rmse_after) and, with out_path, writes the potential file through
    capi.write_all_coeffs ("wrote" = its return value).  The two routes into a context are those of fit_linear: install=True
    (Context.install_coeffs on `ctx`, after any out_path write) or a load of the written file; the active set is stale
    afterwards either way."""
    unknown = set(fit) - {"radial", "species", "moments"}
    if unknown:
        raise ValueError("fit_full: unknown block(s) %s" % sorted(unknown))
    info = ctx.pot.info
    Sp, S = int(info.species_count), int(info.alpha_scalar_count)
    Mu, R = int(info.radial_func_count), int(info.radial_basis_size)
    nrad = Sp * Sp * Mu * R
    theta0 = ctx.theta() if theta0 is None else np.ascontiguousarray(theta0, dtype=np.float64).reshape(-1)
    mask = np.concatenate([np.full(nrad, "radial" in fit), np.full(Sp, "species" in fit), np.full(S, "moments" in fit)])
    kw = dict(weights=weights, list_cutoff=list_cutoff, max_atoms_per_pass=max_atoms_per_pass, device=device)
    before = loss_cells(ctx, configs, labels, theta=theta0, grad=False, **kw)

    def fun(theta):
        r = loss_cells(ctx, configs, labels, theta=theta, **kw)
        return r["loss"], r["grad"]

    theta, history = minimize_lbfgs(fun, theta0, mask, max_iter, history_size, tolerance_grad, tolerance_change)
    after = loss_cells(ctx, configs, labels, theta=theta, grad=False, **kw)
    res = dict(theta=theta, radial_coeffs=theta[:nrad].reshape(Sp, Sp, Mu, R).copy(), species_coeffs=theta[nrad:nrad + Sp].copy(),
               moment_coeffs=theta[nrad + Sp:].copy(), history=history, rmse_before=before["rmse"], rmse_after=after["rmse"])
    if out_path is not None:
        res["wrote"] = capi.write_all_coeffs(ctx.pot.path, out_path, res["moment_coeffs"], res["species_coeffs"], res["radial_coeffs"])
    if install:
        ctx.install_coeffs(res["radial_coeffs"], res["species_coeffs"], res["moment_coeffs"])
    return res


def maxwell_boltzmann(items, mass_of_type, temperature, seed, keys):
    """Host only: Maxwell-Boltzmann velocities [A/ps] per configuration of `items` = [(pos, types)], each from a generator
    of its own seeded by (seed, keys[k]) -- a configuration's draw does not depend on the batch around it -- with the
    configuration's centre-of-mass velocity removed."""
    out = []
    for k, (pos, types) in enumerate(items):
        rng = np.random.default_rng([int(seed) & (2 ** 64 - 1), int(keys[k]) & (2 ** 64 - 1)])
        m = mass_of_type[types - 1]
        v = rng.normal(size=(len(pos), 3)) * np.sqrt(KB * float(temperature[k]) / (m * MVV2E))[:, None]
        if len(pos) == 1:                                     # (its own centre of mass: at rest exactly)
            v[:] = 0.0
        elif len(pos):
            v -= (m[:, None] * v).sum(0) / m.sum()
        out.append(v)
    return out


_Capture = collections.namedtuple("_Capture", "select brk gap max_candidates grade_every thresholds_named")


class _RunSetup:
    """What the batched drivers (`who`) share around their passes.  The prologue: the grade steps (and the refusal of thresholds
    without selection state) before anything touches the device, then the stream, the plan of the passes, ghosts, buffers and
    masses.  The harness of one pass (each_pass).  And what the passes add up to: candidates, records, final, dropped,
    steps_done, builds and the host trace [len(trace_names), steps + 1, ncfg].  `batch`: _batch_items' triple; `capture`: the
    _Capture of _run_arguments, None without grade steps; `replan(plan)`: the passes a driver wants in place of the plan's."""

    def __init__(self, who, ctx, batch, mass_of_type, *, list_cutoff, max_atoms_per_pass, device, capture=None, steps=0, every=1,
                 check_every=0, trace_names=(), replan=None):
        info, (items, all_cells, natoms) = ctx.pot.info, batch
        self.capture = capture = capture or _Capture(2.0, 10.0, 0, 0, 0, False)     # (None: nothing is ever graded or captured)
        self.grade_every = int(capture.grade_every or 0)
        if not info.has_selection:
            if capture.thresholds_named:
                raise capi.MtpError(-23, who + ": thresholds need a potential loaded with its selection state")
            self.grade_every = 0
        import torch
        self.torch, self.dev = torch, device or torch.device("cuda:0")
        self.st = _torch_stream(self.dev)
        self.who, self.ctx, self.items, self.all_cells, self.natoms = who, ctx, items, all_cells, natoms
        self.steps, self.every, self.check_every, self.cut = int(steps), int(every), int(check_every or 0), float(list_cutoff)
        self.skin = self.cut - float(info.max_cutoff)
        self.cfg_mode = bool(self.grade_every) and bool(info.configuration_mode)
        plan, self.volume, self.max_rows = plan_cell_passes(all_cells, natoms, self.cut, max_atoms_per_pass)
        self.plan = plan if replan is None else replan(plan)
        self.ghosts = capi.Ghosts(self.dev.index or 0)
        self.buf = _BatchBuffers(torch, self.dev)
        self.mass_t, self.inv_mass_t = self.to(mass_of_type), self.to(1.0 / mass_of_type)
        self.candidates, self.records, self.final = [], [], [None] * len(items)
        self.dropped = self.steps_done = self.npass = self.builds = 0
        self.trace_names = tuple(trace_names)
        self.trace = np.zeros((len(self.trace_names), self.steps + 1, len(items))) if self.trace_names else None

    def to(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def zeros(self, *shape):
        return self.torch.zeros(shape, dtype=self.torch.float64, device=self.dev)

    def graded(self, step):
        return bool(self.grade_every) and step % self.grade_every == 0

    def each_pass(self, body, empty_final, run_type, final_monitor=False):
        """The passes, one complete run each.  A pass without an atom only fills final[k] = empty_final(k).  Any other gets a
        run (`run_type`: the first ghost and list build; run.trace [len(trace_names), steps + 1, ncfg] on the device) and the
        driver's body(run) -> (s: the last step made, final), then the final energies (and, for the kinetic energy, the monitor),
        the synchronise that names the pass, x without the slot origins, final[k0:k1] = final(x, energies) -- one dict per
        configuration, rows run.rows[j] of x --, the harvest of what was captured and the scatter of the trace."""
        for k0, k1, lay in self.plan:
            self.npass += 1
            counts = self.natoms[k0:k1]
            if int(counts.sum()) == 0:
                for k in range(k0, k1):
                    self.final[k] = empty_final(k)
                continue
            run = run_type(self, k0, k1, lay)
            self.builds += 1
            e_t = self.zeros(k1 - k0)
            run.trace = self.zeros(len(self.trace_names), self.steps + 1, k1 - k0) if self.trace_names else None
            s, final = body(run)
            self.steps_done = max(self.steps_done, s)
            run.energies(e_t)
            if final_monitor:
                run.monitor()
            run.synchronize(self.npass, k0, k1)
            xh = run.x[:run.n].cpu().numpy() - np.repeat(run.lay["origins"], counts, axis=0)
            self.final[k0:k1] = final(xh, e_t.cpu().numpy())
            self.dropped += run.harvest(k0, self.records, self.candidates)
            if self.trace_names:
                self.trace[:, : s + 1, k0:k1] = run.trace.cpu().numpy()[:, : s + 1]

    def result(self, **more):
        """the returned dict (`more`: the driver's own keys, after `dropped`)"""
        out = dict(candidates=self.candidates, records=self.records, dropped=self.dropped, **more, final=self.final,
                   steps_done=self.steps_done, builds=self.builds)
        if self.trace_names:
            out["trace"] = {name: self.trace[i, : self.steps_done + 1] for i, name in enumerate(self.trace_names)}
        return out


class _CellRun:
    """One pass of sample_cells / relax_cells -- a batch of cells that stays on the device for a whole run: the first ghost and
    list build, the per-configuration arrays every such run keeps (frozen, the capture state and its candidate buffer, the
    monitor block) and the launches around the integrator or minimiser: the force call with the ghost fold, the capture, the
    monitor and its one read, the re-neighbouring in slot coordinates, the energies, and the harvest of what was captured.
    The driver sets `v`, the velocities the monitor looks at.  _DeformingCellRun is the same for cells that change."""

    vflag = 0                                                 # 4: per-atom virials (the work layout of evaluate_cells)

    def __init__(self, setup, k0, k1, lay):
        torch, dev, to = setup.torch, setup.dev, setup.to
        self.per_row = 10 if self.vflag else 4
        self.setup, self.k0, self.k1, self.lay = setup, k0, k1, lay
        self.ctx, self.ghosts, self.buf = setup.ctx, setup.ghosts, setup.buf
        self.cut, self.cfg_mode, self.st = setup.cut, setup.cfg_mode, setup.st
        self.items, self.cells, self.counts = setup.items[k0:k1], setup.all_cells[k0:k1], setup.natoms[k0:k1]
        self.room = max(setup.capture.max_candidates - len(setup.records), 0)     # what earlier passes left of the candidate buffer
        self.C = C = int(self.ctx.pot.info.coeff_count)
        self.ncfg = ncfg = k1 - k0
        self.nonempty = int((self.counts > 0).sum())
        self.cf = cf = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.n = n = int(cf[-1])
        self.rows = [(int(cf[j]), int(cf[j + 1])) for j in range(ncfg)]
        self.stride = int(self.counts.max())
        self.cf_t, self.org_t = to(cf), to(lay["origins"])
        na = lambda rows: rows + (rows & 1)
        self.work_size = lambda rows: self.per_row * na(rows) + 10 + C + (C & 1)
        buf = self.buf
        nall = _pass_ghosts_and_list(self.ctx, self.ghosts, buf, self.items, cf, self.cells, lay, self.cut,
                                     n + int(setup.max_rows[k0:k1].sum()),
                                     lambda rows, first: buf.reserve(rows, ncfg, self.work_size(rows), 0), self.st)
        self.x = buf.xall
        self.row_cfg = torch.empty(n, dtype=torch.int32, device=dev)
        capi.sample_row_map(self.cf_t, self.row_cfg, stream=self.st)
        self.x_ref = self.x[:n].clone()
        self.frozen = torch.zeros(ncfg, dtype=torch.int32, device=dev)
        self.last_capture = torch.full((ncfg,), -2 ** 30, dtype=torch.int32, device=dev)
        self.slot = torch.full((ncfg,), -1, dtype=torch.int32, device=dev)
        self.counts_t = torch.zeros(3, dtype=torch.int32, device=dev)    # captured, dropped, frozen
        self.g_t = torch.zeros(ncfg, dtype=torch.float64, device=dev)
        mon = torch.zeros((3 if self.vflag else 2) * ncfg + 4, dtype=torch.float64, device=dev)
        self.mv2, self.d2, self.block = mon[:ncfg], mon[ncfg: 2 * ncfg], mon[2 * ncfg: 2 * ncfg + 4]
        self.cellmove, self.monitor_read = mon[2 * ncfg + 4:], mon[ncfg:]     # (vflag: d2 | block | cellmove is ONE read)
        self.cand_x = torch.zeros((max(self.room, 1), self.stride, 3), dtype=torch.float64, device=dev)
        self.cand_cell = None                                 # (fixed cells: a candidate's cell is the one given)
        self.rec = torch.zeros((max(self.room, 1), 2), dtype=torch.int32, device=dev)
        self.rec_grade = torch.zeros(max(self.room, 1), dtype=torch.float64, device=dev)
        self.layout(nall)

    def layout(self, rows):
        # f | ev | eatom | (vatom) | max grade | coeff_ders: one allocation, zeroed by one launch every step
        m, C, p = rows + (rows & 1), self.C, self.per_row
        w = self.buf.work[: self.work_size(rows)]
        self.work, self.f, self.ev, self.eatom = w, w[: 3 * rows].view(rows, 3), w[3 * m: 3 * m + 8], w[3 * m + 8: 4 * m + 8]
        self.vatom = w[4 * m + 8: p * m + 8]
        self.maxg, self.coeff = w[p * m + 8: p * m + 9], w[p * m + 10: p * m + 10 + C]

    def forces(self, grade):
        ctx, buf, st, n, vf = self.ctx, self.buf, self.st, self.n, self.vflag
        nbh, cfg = grade and not self.cfg_mode, grade and self.cfg_mode
        self.ghosts.forward(self.x, stream=st)
        capi.zero_async(self.work, stream=st)
        ctx.compute_device_rows(0, n, False, self.x, buf.tall, self.f, eflag=3, vflag=vf, grade=grade, eatom_t=self.eatom,
                                vatom_t=self.vatom if vf else None, ev_t=self.ev, grades_t=buf.grades if nbh else None,
                                maxg_t=self.maxg if grade else None, coeff_t=self.coeff if cfg else None, stream=st)
        self.ghosts.reverse_finish(ctx, self.f, self.ev, eflag=3, vflag=vf, stream=st)
        if vf:                                                # the virial per configuration and, in the SAME launch, the grades
            capi.batch_reduce(self.cf_t, vatom_t=self.vatom, grades_t=buf.grades if nbh else None, virial_t=self.virial,
                              cfg_grade_t=self.g_t if nbh else None, stream=st)
        elif nbh:
            capi.batch_reduce(self.cf_t, grades_t=buf.grades, cfg_grade_t=self.g_t, stream=st)
        if cfg:
            ctx.batch_cfg_grades(self.cf_t, n, self.g_t, stream=st)

    def capture(self, step):
        c = self.setup.capture
        capi.sample_capture(self.cf_t, self.n, self.row_cfg, self.g_t, step, c.select, c.brk, c.gap, self.x, self.org_t, self.frozen,
                            self.last_capture, self.slot, self.room, self.stride, self.cand_x, self.rec, self.rec_grade,
                            self.counts_t, stream=self.st)

    def moved(self):
        """after the positions were moved (fixed cells: nothing follows)"""

    def monitor(self, mv2_t=None):
        capi.sample_monitor(self.cf_t, self.frozen, self.x, self.x_ref, self.v, self.buf.tall, self.setup.mass_t, self.counts_t,
                            self.mv2 if mv2_t is None else mv2_t, self.d2, self.block, stream=self.st)

    def read(self):
        """the monitor and the one host read between rebuilds: (nothing is running any more, the lists are stale: an atom of a
        running configuration moved more than half the skin)"""
        self.monitor()
        b = self.block.cpu().numpy()
        return b[1] >= self.nonempty, b[0] > (0.5 * self.setup.skin) ** 2

    def energies(self, out_t):
        capi.batch_reduce(self.cf_t, eatom_t=self.eatom, energy_t=out_t, stream=self.st)

    def reneighbor(self):
        self.rebuild()
        self.setup.builds += 1

    def rebuild(self):
        x, n, lay, st = self.x, self.n, self.lay, self.st
        capi.sample_to_cell(n, self.row_cfg, self.org_t, x, stream=st)
        rows = self.ghosts.build_batch(x, self.cf, self.cells, lay["origins"], self.cut, stream=st)
        self.ghosts.types(self.buf.tall, stream=st)
        self.ctx.build_neighbors_device(x, n, rows, self.cut, lay["lo"], lay["hi"], stream=st)
        self.layout(rows)
        self.x_ref.copy_(x[:n])

    def synchronize(self, npass, k0, k1):
        try:
            self.ctx.synchronize(stream=self.st)              # an atom type outside the potential is reported here
        except capi.MtpError as e:
            raise capi.MtpError(e.code, "pass %d (configurations %d to %d): %s" % (npass, k0, k1 - 1, e)) from e

    def harvest(self, k0, records, candidates):
        """appends this pass's records (configuration numbers from k0) and candidates; returns the number dropped.  self.cand_cell
        [slots, 9]: the cell every candidate was captured in, where cells change during the run"""
        ch = self.counts_t.cpu().numpy()
        ncap = int(ch[0])
        rh, gh, snap = self.rec[:ncap].cpu().numpy(), self.rec_grade[:ncap].cpu().numpy(), self.cand_x[:ncap].cpu().numpy()
        ch9 = None if self.cand_cell is None else self.cand_cell[:ncap].cpu().numpy().reshape(ncap, 3, 3)
        for j in range(ncap):
            k = int(rh[j, 0])
            records.append((k0 + k, int(rh[j, 1]), float(gh[j])))
            cell = self.cells[k] if ch9 is None else ch9[j]
            candidates.append((snap[j, : int(self.counts[k])].copy(), cell.copy(), self.items[k][1].copy()))
        return int(ch[1])


class _DeformingCellRun(_CellRun):
    """_CellRun for cells that change during the run (relax_cells_vc, sample_cells_npt): forces with
    per-atom virials and the virial per configuration, the geometry h = h0 . D, x = origin + xt . D in the arrays `A`
    (mtp_relax_cell_arrays; the driver adds its minimiser's state and sets v = A["vt"] -- sample_cells_npt moves h itself and
    adds the arrays of mtp_sample_cell_arrays: D stays I and xt is not read), ghosts that follow the cell after a
    move, the stale rule with the cell's own movement in it, candidates with the cell of their graded step, and a rebuild that
    lays the pass out again for the cells as they are."""

    vflag = 4

    def __init__(self, setup, k0, k1, lay):
        super().__init__(setup, k0, k1, lay)
        to, zeros, ncfg, n = setup.to, setup.zeros, self.ncfg, self.n
        self.eye = eye = setup.torch.eye(3, dtype=setup.torch.float64, device=setup.dev).reshape(1, 9).repeat(ncfg, 1)
        h0_t = to(self.cells.reshape(ncfg, 9))
        self.virial = zeros(ncfg, 6)
        self.A = A = dict(cfg_first=self.cf_t, x=self.x, xt=zeros(n, 3), f=self.f, type=self.buf.tall, inv_mass=setup.inv_mass_t,
                          virial=self.virial, h0=h0_t, origins=self.org_t, D=eye.clone(), Dbinv=eye.clone(), href=h0_t.clone(),
                          nimg=to(_cell_images(self.cells, self.cut)), frozen=self.frozen, h=h0_t.clone(), T=eye.clone(),
                          cellmove=self.cellmove, counts=self.counts_t)
        capi.relax_cell_rebase(ncfg, self.row_cfg, self.org_t, self.x, A["D"], A["xt"], A["Dbinv"], stream=self.st)   # xt = x - origin
        self.cand_cell = zeros(max(self.room, 1), 9)

    def capture(self, step):
        super().capture(step)
        capi.relax_cell_capture_cells(self.slot, self.room, self.A["h"], self.cand_cell, stream=self.st)

    def moved(self):
        self.ghosts.deform(self.row_cfg, self.A["T"], stream=self.st)

    def read(self):
        self.monitor()
        ncfg = self.ncfg
        m = self.monitor_read.cpu().numpy()                   # d2 [ncfg] | block [4] | cellmove [ncfg]
        return m[ncfg + 1] >= self.nonempty, cell_list_stale(m[:ncfg], m[ncfg + 4:], self.setup.skin)

    def rebuild(self):
        A, buf, ghosts, st, n, ncfg, cut, to = self.A, self.buf, self.ghosts, self.st, self.n, self.ncfg, self.cut, self.setup.to
        hh = A["h"].cpu().numpy().reshape(ncfg, 3, 3)                 # the cells the atoms sit in now
        with np.errstate(all="ignore"):
            bad = ~(np.isfinite(hh).all((1, 2)) & (_det3(hh) > 0.0))
        hh[bad] = self.cells[bad]                                     # (such a configuration fails at its next step)
        capi.sample_to_cell(n, self.row_cfg, self.org_t, self.x, stream=st)     # with the OLD origins
        try:
            new = capi.batch_layout(hh, cut, cut)
        except capi.MtpError as e:
            if e.code != -24:
                raise
            raise capi.MtpError(-24, "%s: pass %d: configuration %d no longer fits the pass with its relaxed cell: %s"
                                % (self.setup.who, self.setup.npass, self.k0 + int(getattr(e, "nfit", 0)), e)) from e
        org_t = to(new["origins"])
        try:
            rows = ghosts.build_batch(self.x, self.cf, hh, new["origins"], cut, stream=st)
        except capi.MtpError as e:                                    # (the capacity protocol: a shrinking cell has more images)
            if e.code != -24 or ghosts.nall <= buf.cap or ghosts.nall >= 2 ** 31 - 1:
                raise
            keep_x, keep_t = self.x[:n].clone(), buf.tall[:n].clone()
            buf.reserve(ghosts.nall, ncfg, self.work_size(ghosts.nall), 0)
            buf.xall[:n], buf.tall[:n] = keep_x, keep_t
            self.x = buf.xall
            capi.sample_to_cell(n, self.row_cfg, org_t, self.x, stream=st)     # (the refused build wrapped and translated already)
            rows = ghosts.build_batch(self.x, self.cf, hh, new["origins"], cut, stream=st)
        ghosts.types(buf.tall, stream=st)
        self.ctx.build_neighbors_device(self.x, n, rows, cut, new["lo"], new["hi"], stream=st)
        buf.reserve(0, ncfg, self.work_size(rows), 0)                 # (rows may exceed what the work array was sized for)
        self.layout(rows)
        self.x_ref.copy_(self.x[:n])
        self.cells, self.lay, self.org_t = hh, new, org_t
        A.update(x=self.x, f=self.f, type=buf.tall, origins=org_t, href=to(hh.reshape(ncfg, 9)), nimg=to(_cell_images(hh, cut)))
        A["T"].copy_(self.eye)
        self.cellmove.zero_()
        capi.relax_cell_rebase(ncfg, self.row_cfg, org_t, self.x, A["D"], A["xt"], A["Dbinv"], stream=st)


def _minimise_pass(run, steps, graded, step, every, check_every):
    """The step loop relax_cells and relax_cells_vc share, s = 0 ... steps: forces (graded on a grade step) -> on a grade step
    the capture, BEFORE the minimiser -> step(s, last): the driver's one minimiser launch (and its trace) -> what follows a
    move -> every `check_every` steps since the last rebuild, after step 0 and at a rebuild the one read: (nothing runs any
    more, the lists are stale) -> the rebuild.  After step `steps` no move is made.  Returns the last step made."""
    s, since = 0, 0
    while True:
        grade = graded(s)
        run.forces(grade)
        if grade:
            run.capture(s)
        step(s, s == steps)
        if s == steps:
            break
        run.moved()
        since += 1
        need = since >= every
        if s == 0 or need or (check_every and since % check_every == 0):   # the one read between rebuilds, and one at a rebuild
            done, stale = run.read()
            if done:                                          # nothing is running any more: this step moved nothing
                break
            need = need or stale
        if need:
            run.reneighbor()
            since = 0
        s += 1
    return s


def _sample_pass(run, steps, graded, every, check_every, first_half, second_half, record=None, thermostat=True):
    """The step loop sample_cells and sample_cells_npt share.  Step 0: forces (graded on a grade step) -> with `thermostat`
    second_half(0, False), fix langevin's setup: the thermostat force, no kick -> on a grade step the capture and one read.
    Step s = 1 ... steps: first_half(s), the driver's launch and what follows its move -> the reads and rebuilds of
    _minimise_pass, without the read after step 0 -> forces -> second_half(s, True) -> on a grade step the capture.  record(s)
    (or None) follows every step made, step 0 included.  Returns the last step made: a first half wrote nothing if the read
    after it finds nothing running, and is not counted."""
    record = record or (lambda step: None)
    run.forces(graded(0))
    if thermostat:
        second_half(0, False)
    stop = False
    if graded(0):
        run.capture(0)
        stop = run.read()[0]
    record(0)
    s, since = 0, 0
    while s < steps and not stop:
        s += 1
        first_half(s)
        since += 1
        need = since >= every
        if need or (check_every and since % check_every == 0):   # the one read between rebuilds, and one at a rebuild
            done, stale = run.read()
            if done:                                          # nothing is running any more: this first half wrote nothing
                s -= 1
                break
            need = need or stale
        if need:
            run.reneighbor()
            since = 0
        grade = graded(s)
        run.forces(grade)
        second_half(s, True)
        if grade:
            run.capture(s)
        record(s)
    return s


def _mass_of_type(who, items, masses):
    """the masses per atom type; ValueError unless the types count from 1 and `masses` is one positive mass or one per type"""
    ntypes = max([int(t.max()) for _, t in items if len(t)], default=1)
    if min([int(t.min()) for _, t in items if len(t)], default=1) < 1:
        raise ValueError("%s: atom types count from 1" % who)
    mass_of_type = np.atleast_1d(np.asarray(masses, dtype=np.float64)).reshape(-1)
    if len(mass_of_type) == 1:
        mass_of_type = np.full(ntypes, float(mass_of_type[0]))
    if len(mass_of_type) < ntypes or not (mass_of_type > 0.0).all():
        raise ValueError("%s: masses is one positive mass, or one per atom type (%d)" % (who, ntypes))
    return mass_of_type


def _run_arguments(who, items, masses, threshold_select, threshold_break, capture_gap, max_candidates, grade_every, every,
                   check_every):
    """the host-side checks sample_cells and relax_cells (`who`) share: thresholds, atom types and masses, the capture and
    list arguments.  Returns (mass_of_type, the _Capture that _RunSetup takes)."""
    select = 2.0 if threshold_select is None else float(threshold_select)
    brk = 10.0 if threshold_break is None else float(threshold_break)
    if select > brk:
        raise ValueError("%s: threshold_select (%g) is above threshold_break (%g)" % (who, select, brk))
    mass_of_type = _mass_of_type(who, items, masses)
    if int(capture_gap) < 0 or int(grade_every or 0) < 0 or int(every) < 1 or int(check_every or 0) < 0:
        raise ValueError("%s: capture_gap, grade_every and check_every must not be negative, every at least 1" % who)
    max_candidates = 4 * len(items) if max_candidates is None else int(max_candidates)
    if max_candidates < 0:
        raise ValueError("%s: max_candidates must not be negative" % who)
    return mass_of_type, _Capture(select, brk, int(capture_gap), max_candidates, grade_every,
                                  threshold_select is not None or threshold_break is not None)


def _sample_arguments(configs, temperature, steps, dt, keys, masses, threshold_select, threshold_break, capture_gap,
                      max_candidates, velocities, grade_every, every, check_every, who="sample_cells"):
    """the host-side checks of sample_cells and sample_cells_npt (`who`; nothing here touches the device); returns the normalised
    arguments"""
    items, all_cells, natoms = _batch_items(configs)
    ncfg = len(items)
    if not (float(dt) > 0.0 and np.isfinite(float(dt))):
        raise ValueError(who + ": dt must be positive and finite, got %r" % (dt,))
    if int(steps) < 0 or int(steps) >= 2 ** 30:
        raise ValueError(who + ": steps must be in [0, 2^30)")
    mass_of_type, capture = _run_arguments(who, items, masses, threshold_select, threshold_break, capture_gap, max_candidates,
                                           grade_every, every, check_every)
    if keys is None:
        keys = np.arange(ncfg, dtype=np.uint64)
    else:
        if len(keys) != ncfg:
            raise ValueError(who + ": %d keys for %d configurations" % (len(keys), ncfg))
        keys = np.array([int(q) & (2 ** 64 - 1) for q in keys], dtype=np.uint64)
    temperature = np.asarray(temperature, dtype=np.float64)
    if temperature.ndim == 0:
        temperature = np.full(ncfg, float(temperature))
    if temperature.shape != (ncfg,) or not (np.isfinite(temperature).all() and (temperature >= 0.0).all()):
        raise ValueError(who + ": temperature is a non-negative scalar or one per configuration (%d)" % ncfg)
    if velocities is not None:
        if len(velocities) != ncfg:
            raise ValueError(who + ": %d velocity arrays for %d configurations" % (len(velocities), ncfg))
        velocities = [np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]
        for k, v in enumerate(velocities):
            if len(v) != natoms[k]:
                raise ValueError(who + ": velocities[%d] must be [%d, 3]" % (k, natoms[k]))
    return (items, all_cells, natoms), capture, keys, temperature, mass_of_type, velocities


def sample_cells(ctx, configs, temperature, steps, dt, t_damp=0.1, seed=0, keys=None, masses=183.84, grade_every=10,
                 threshold_select=None, threshold_break=None, capture_gap=0, max_candidates=None, velocities=None,
                 list_cutoff=7.0, every=10, check_every=4, max_atoms_per_pass=None, device=None, trace=False):
    """The sampling step of the active-learning loop: finite-temperature MD of a whole batch of independent periodic cells
    under the context's potential, device-resident, with the extrapolation grade checked every `grade_every` steps and the
    extrapolating configurations captured on the device (what LAMMPS does one cell at a time with pair_style
    mtp/extrapolation ... threshold_select threshold_break under fix langevin + fix nve).  `configs` as for evaluate_cells;
    the passes are planned by plan_cell_passes and run one after another, every pass a complete run of `steps`.

    One step (metal units, dt in ps) is mtp_sample_initial (kick + drift) -> ghosts follow -> ONE force call over all rows
    -> ghost fold -> mtp_sample_final (fix langevin's force with t_damp [ps] and the target `temperature` [K], a scalar or
    one per configuration, then the second kick).  t_damp <= 0, None or infinite: plain NVE.  The noise is Philox4x32-10 on
    the counter (step, atom within its configuration, keys[k]) and the key `seed` (include/mtp_mi355x.h): the trajectory of
    a configuration depends on its keys[k] (default: its index in `configs`), not on the batch around it.  As in LAMMPS the
    thermostat force is also applied to the forces of step 0 (fix langevin's setup).  velocities=None draws Maxwell-Boltzmann
    velocities per configuration on the host (maxwell_boltzmann: from seed and keys[k], centre-of-mass velocity removed);
    otherwise a list of [n, 3] arrays in A/ps.  masses: one, or one per atom type [g/mol].

    Lists are rebuilt every `every` steps, or when an atom of an unfrozen configuration moved more than half the skin
    (list_cutoff - the potential's cutoff) -- seen in the 32-byte block mtp_sample_monitor leaves, which is read every
    `check_every` steps since the last rebuild, and once at every rebuild, and is the only thing the host reads between
    rebuilds.

    Grade steps (0, grade_every, 2 grade_every, ...; a potential loaded with its selection state) take the grade of every
    configuration -- the largest per-atom grade in neighbourhood mode, the configuration's grade in configuration mode --
    and mtp_sample_capture decides on the device: a non-empty, unfrozen configuration with !(grade < threshold_select) (default 2)
    whose last capture is at least capture_gap steps back is captured -- a snapshot of its positions in the next slot of the
    candidate buffer, slots in ascending (step, configuration) order -- and then frozen (it no longer moves) if
    !(grade < threshold_break) (default 10).  With the buffer (max_candidates slots, default 4 per configuration) full, a
    configuration is dropped: counted, nothing of it written, not frozen.  A potential without selection state skips the
    grade steps; naming a threshold then raises MtpError(-23), as select_cells does.  The run ends early once every non-empty
    configuration of the pass is frozen, which is seen at the next read of the monitor block (so at the latest at the next
    rebuild; frozen configurations do not move in between, and steps_done counts the steps up to that read).

    Returns dict(candidates: [(pos, cell, types)] in capture order (by pass, then step, then configuration), ready for
    select_cells; records: [(configuration, step, grade)]; dropped; frozen [ncfg] bool; final: per configuration dict(x [n, 3]
    cell coordinates, wrapped at the last rebuild; v [n, 3]; energy: the potential energy; temperature = sum m v^2 / (3 n kB));
    steps_done: the steps made (the largest over the passes); builds: the list builds of all passes) and, with the diagnostic trace=True
    (two more launches a step), trace: dict(energy, kinetic [steps_done
    + 1, ncfg]) -- potential and kinetic energy per configuration after every step, step 0 first."""
    batch, capture, keys, temperature, mass_of_type, velocities = _sample_arguments(
        configs, temperature, steps, dt, keys, masses, threshold_select, threshold_break, capture_gap, max_candidates, velocities,
        grade_every, every, check_every)
    setup = _RunSetup("sample_cells", ctx, batch, mass_of_type, capture=capture, steps=steps, every=every, check_every=check_every,
                      trace_names=("energy", "kinetic") if trace else (), list_cutoff=list_cutoff,
                      max_atoms_per_pass=max_atoms_per_pass, device=device)
    to, st, buf, mass_t, inv_mass_t = setup.to, setup.st, setup.buf, setup.mass_t, setup.inv_mass_t
    dt, seed = float(dt), int(seed) & (2 ** 64 - 1)
    t_damp = 0.0 if t_damp is None or not np.isfinite(float(t_damp)) or float(t_damp) <= 0.0 else float(t_damp)
    dtf = 0.5 * dt * FTM2V
    if velocities is None:
        velocities = maxwell_boltzmann(setup.items, mass_of_type, temperature, seed, keys)
    frozen_all = np.zeros(len(setup.items), dtype=bool)

    def one_pass(run):
        k0, k1, n, cf_t, row_cfg, x, frozen = run.k0, run.k1, run.n, run.cf_t, run.row_cfg, run.x, run.frozen
        run.v = v = to(np.concatenate(velocities[k0:k1]))
        temp_t = to(temperature[k0:k1])
        key_t = to(keys[k0:k1].view(np.int64))

        def second_half(step, kick):
            capi.sample_final(n, row_cfg, cf_t, frozen, v, run.f, buf.tall, mass_t, inv_mass_t, temp_t, key_t, seed, step,
                              dtf if kick else 0.0, dt, t_damp, stream=st)

        def record(step):
            run.energies(run.trace[0, step])
            run.monitor(run.trace[1, step])

        s = _sample_pass(run, setup.steps, setup.graded, setup.every, setup.check_every,
                         lambda step: capi.sample_initial(n, row_cfg, frozen, x, v, run.f, buf.tall, inv_mass_t, dtf, dt, stream=st),
                         second_half, record if trace else None, thermostat=t_damp > 0.0)

        def final(xh, eh):                                    # (the harness ran the monitor once more: sum m v^2 at the end)
            vh, mh = v.cpu().numpy(), run.mv2.cpu().numpy()
            frozen_all[k0:k1] = frozen.cpu().numpy() != 0
            return [dict(x=xh[a:b], v=vh[a:b], energy=float(eh[j]),
                         temperature=float(mh[j]) * MVV2E / (3.0 * (b - a) * KB) if b > a else 0.0)
                    for j, (a, b) in enumerate(run.rows)]

        return s, final

    setup.each_pass(one_pass, lambda k: dict(x=np.zeros((0, 3)), v=np.zeros((0, 3)), energy=0.0, temperature=0.0), _CellRun,
                    final_monitor=True)
    out = setup.result(frozen=frozen_all)
    if trace:
        out["trace"]["kinetic"] = 0.5 * MVV2E * out["trace"]["kinetic"]
    return out


def _relax_arguments(configs, steps, ftol, dt, dt_max, dmax, n_min, f_inc, f_dec, alpha_start, f_alpha, masses, threshold_select,
                     threshold_break, capture_gap, max_candidates, grade_every, every, check_every, who="relax_cells"):
    """the host-side checks of relax_cells and relax_cells_vc (`who`; nothing here touches the device); returns the normalised
    arguments"""
    items, all_cells, natoms = _batch_items(configs)
    if int(steps) < 0 or int(steps) >= 2 ** 30:
        raise ValueError(who + ": steps must be in [0, 2^30)")
    num = dict(ftol=ftol, dt=dt, dt_max=dt_max, dmax=dmax, f_inc=f_inc, f_dec=f_dec, alpha_start=alpha_start, f_alpha=f_alpha)
    num = {k: float(q) for k, q in num.items()}
    for k, q in num.items():
        if not np.isfinite(q):
            raise ValueError("%s: %s must be finite, got %r" % (who, k, q))
    if not (num["ftol"] >= 0.0 and num["dt"] > 0.0 and num["dt_max"] > 0.0 and num["dmax"] > 0.0):
        raise ValueError(who + ": ftol >= 0, dt > 0, dt_max > 0 and dmax > 0 are required")
    if not (num["f_inc"] >= 1.0 and 0.0 < num["f_dec"] < 1.0 and 0.0 <= num["alpha_start"] <= 1.0 and 0.0 < num["f_alpha"] <= 1.0):
        raise ValueError(who + ": f_inc >= 1, f_dec in (0, 1), alpha_start in [0, 1] and f_alpha in (0, 1] are required")
    if int(n_min) < 0:
        raise ValueError(who + ": n_min must not be negative")
    mass_of_type, capture = _run_arguments(who, items, masses, threshold_select, threshold_break, capture_gap, max_candidates,
                                           grade_every, every, check_every)
    params = capi.RelaxParams(num["ftol"], num["dt_max"], num["dmax"], num["f_inc"], num["f_dec"], num["alpha_start"], num["f_alpha"],
                              int(n_min))
    return (items, all_cells, natoms), capture, mass_of_type, params, num["dt"]


def relax_cells(ctx, configs, steps, ftol=1e-3, dt=1e-3, dt_max=1e-2, dmax=0.1, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1,
                f_alpha=0.99, masses=183.84, grade_every=0, threshold_select=None, threshold_break=None, capture_gap=0,
                max_candidates=None, list_cutoff=7.0, every=10, check_every=4, max_atoms_per_pass=None, device=None, trace=False):
    """The relaxation step of the active-learning loop: every cell of a batch of independent periodic cells is taken to its
    local minimum under the context's potential (fixed cells), device-resident, with FIRE (Bitzek et al., PRL 97, 170201)
    and the per-step displacement cap of LAMMPS' min_style fire -- one state machine per configuration, run by
    mtp_relax_step -- while the extrapolation grade is watched as in sample_cells (what MLIP's `relax` does one cell at a
    time).  `configs`, the passes, the lists (`list_cutoff`, `every`, `check_every`: rebuilt every `every` steps or when an atom
    of a running configuration moved more than half the skin, seen in the monitor block) and the capture arguments
    (`grade_every`, here 0 = never by default, `threshold_select`, `threshold_break`, `capture_gap`, `max_candidates`) are
    those of sample_cells.

    Velocities start at 0, the time step at `dt` [ps].  Step s = 0 ... steps is: ONE force call over all rows (graded on
    grade steps) -> ghost fold -> on a grade step mtp_sample_capture, BEFORE the minimiser, so that a configuration over
    threshold_break freezes at the positions that were graded -> mtp_relax_step(s), which reduces P = sum f.v, sum v.v,
    sum f.f and the largest |f_i| per configuration and decides on the device: non-finite forces -> "failed"; largest
    |f_i| <= ftol [eV/A] -> "converged" (its velocities are set to 0); otherwise the FIRE update of dt and alpha (dt_max,
    n_min, f_inc, f_dec, alpha_start, f_alpha), the mixed velocity, a move of at most `dmax` [A] per coordinate and the kick
    (masses: one, or one per atom type [g/mol]).  A frozen, converged or failed configuration is not written again.  After
    step `steps` no move is made: the last launch only decides.  The run of a pass ends early once every non-empty
    configuration is frozen, converged or failed, seen at the next read of the monitor block (after step 0, every
    `check_every` steps since the last rebuild, and at every rebuild).

    Returns dict(final: per configuration dict(x [n, 3] cell coordinates, wrapped at the last rebuild; energy: the potential
    energy at x; fmax: the largest |f_i| at the last step the minimiser looked at it (0 if it never did); status: "running",
    "captured-frozen", "converged" or "failed"; step: the step of convergence or failure, -1 otherwise; dt: its time step);
    candidates, records, dropped: as sample_cells; steps_done: the last step whose forces were computed (the largest over the
    passes); builds) and, with trace=True (one more launch and a copy a step), trace: dict(energy, fmax [steps_done + 1, ncfg]) --
    per configuration and step, step 0 first, fmax as in `final`."""
    batch, capture, mass_of_type, params, dt = _relax_arguments(
        configs, steps, ftol, dt, dt_max, dmax, n_min, f_inc, f_dec, alpha_start, f_alpha, masses, threshold_select, threshold_break,
        capture_gap, max_candidates, grade_every, every, check_every)
    setup = _RunSetup("relax_cells", ctx, batch, mass_of_type, capture=capture, steps=steps, every=every, check_every=check_every,
                      trace_names=("energy", "fmax") if trace else (), list_cutoff=list_cutoff,
                      max_atoms_per_pass=max_atoms_per_pass, device=device)
    torch, dev, st, buf = setup.torch, setup.dev, setup.st, setup.buf

    def one_pass(run):
        ncfg = run.ncfg
        run.v = v = setup.zeros(run.n, 3)
        state = setup.zeros(3, ncfg)
        dt_t, alpha_t, fmax_t = state[0], state[1], state[2]
        dt_t.fill_(dt)
        alpha_t.fill_(params.alpha_start)
        npos_t = torch.zeros(ncfg, dtype=torch.int32, device=dev)
        done_t = torch.full((ncfg,), -1, dtype=torch.int32, device=dev)

        def step(s, last):
            capi.relax_step(run.cf_t, params, s, run.x, v, run.f, buf.tall, setup.inv_mass_t, dt_t, alpha_t, npos_t, run.frozen,
                            done_t, fmax_t, run.counts_t, last=last, stream=st)
            if trace:
                run.energies(run.trace[0, s])
                run.trace[1, s].copy_(fmax_t)

        s = _minimise_pass(run, setup.steps, setup.graded, step, setup.every, setup.check_every)

        def final(xh, eh):
            sh, fh, dh = state.cpu().numpy(), run.frozen.cpu().numpy(), done_t.cpu().numpy()
            return [dict(x=xh[a:b], energy=float(eh[j]), fmax=float(sh[2, j]), status=capi.RELAX_STATUS[int(fh[j])],
                         step=int(dh[j]), dt=float(sh[0, j])) for j, (a, b) in enumerate(run.rows)]

        return s, final

    setup.each_pass(one_pass, lambda k: dict(x=np.zeros((0, 3)), energy=0.0, fmax=0.0, status=capi.RELAX_STATUS[0], step=-1, dt=dt),
                    _CellRun)
    return setup.result()


def cell_list_stale(d2, cellmove, skin):
    """Host arithmetic: the rebuild rule of relax_cells_vc.  d2 [ncfg]: the largest squared displacement of an atom of each
    configuration since the last rebuild; cellmove [ncfg]: mtp_relax_cell_step's sum_a (nimg_a + 1) |h_a - href_a|; skin =
    list_cutoff - the potential's cutoff.  A pair changes its distance by at most two atom displacements plus |n . (h - href)|,
    and an image that was no ghost at the last build has |n_a| <= nimg_a + 1 (or lies a whole plane spacing further out): the
    lists are stale once max_k (2 sqrt(d2[k]) + cellmove[k]) > skin.  With cellmove = 0 this is the half-skin test."""
    d2, cellmove = np.asarray(d2, dtype=np.float64), np.asarray(cellmove, dtype=np.float64)
    return bool(d2.size) and bool(np.max(2.0 * np.sqrt(d2) + cellmove) > float(skin))


def _relax_vc_arguments(natoms, mass_of_type, pressure, stol, cell_mask, isotropic, cell_factor, cell_mass):
    """the host-side checks of relax_cells_vc's own arguments (nothing here touches the device); returns (stol, pressure,
    cell_factor, cell_mass, cell_mask [6], factor_per_atom)"""
    stol, pressure = float(stol), float(pressure)
    if not (np.isfinite(stol) and stol >= 0.0):
        raise ValueError("relax_cells_vc: stol must be finite and not negative, got %r" % (stol,))
    if not np.isfinite(pressure):
        raise ValueError("relax_cells_vc: pressure must be finite, got %r" % (pressure,))
    per_atom = cell_factor is None
    cell_factor = 1.0 if per_atom else float(cell_factor)
    if not (np.isfinite(cell_factor) and cell_factor > 0.0):
        raise ValueError("relax_cells_vc: cell_factor must be positive and finite, got %r" % (cell_factor,))
    cell_mass = float(np.mean(mass_of_type)) if cell_mass is None else float(cell_mass)
    if not (np.isfinite(cell_mass) and cell_mass > 0.0):
        raise ValueError("relax_cells_vc: cell_mass must be positive and finite, got %r" % (cell_mass,))
    return stol, pressure, cell_factor, cell_mass, _cell_mask("relax_cells_vc", cell_mask), per_atom


def _cell_mask(who, cell_mask):
    """cell_mask as a list of six 0 / 1, or ValueError"""
    try:
        mask = [int(m) for m in cell_mask]
        exact = all(float(m) == q for m, q in zip(cell_mask, mask))
    except (TypeError, ValueError):
        mask, exact = [], False
    if len(mask) != 6 or not exact or any(m not in (0, 1) for m in mask):
        raise ValueError("%s: cell_mask is six entries 0 or 1 (xx yy zz xy xz yz), got %r" % (who, cell_mask))
    return mask


def _cell_images(cells, rghost):
    """mtp_ghosts_cell_bounds' nimage of many cells at once, int32 [ncfg, 3]: ceil(rghost / plane spacing) per direction, the
    margins of plan_cell_passes (a rebuild of relax_cells_vc needs them for every cell of the pass)"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    cross = np.stack([np.cross(cells[:, 1], cells[:, 2]), np.cross(cells[:, 2], cells[:, 0]), np.cross(cells[:, 0], cells[:, 1])], axis=1)
    volume = (cells[:, 0] * cross[:, 0]).sum(1)
    m = float(rghost) * np.sqrt((cross * cross).sum(2)) / volume[:, None]
    return np.minimum(np.ceil(m), 2147483647.0).astype(np.int32)


def _det3(h):
    """determinants of [..., 3, 3] arrays or tensors, elementwise products (no factorisation)"""
    return (h[..., 0, 0] * (h[..., 1, 1] * h[..., 2, 2] - h[..., 1, 2] * h[..., 2, 1])
            - h[..., 0, 1] * (h[..., 1, 0] * h[..., 2, 2] - h[..., 1, 2] * h[..., 2, 0])
            + h[..., 0, 2] * (h[..., 1, 0] * h[..., 2, 1] - h[..., 1, 1] * h[..., 2, 0]))


def relax_cells_vc(ctx, configs, steps, pressure=0.0, stol=1e-4, cell_mask=(1, 1, 1, 1, 1, 1), isotropic=False, cell_factor=None,
                   cell_mass=None, ftol=1e-3, dt=1e-3, dt_max=1e-2, dmax=0.1, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1,
                   f_alpha=0.99, masses=183.84, grade_every=0, threshold_select=None, threshold_break=None, capture_gap=0,
                   max_candidates=None, list_cutoff=7.0, every=10, check_every=4, max_atoms_per_pass=None, device=None,
                   trace=False):
    """relax_cells with the cell among the degrees of freedom: every cell of the batch is taken, together with its atoms, to a
    local minimum of the enthalpy E + p V under the context's potential, device-resident, one state machine per configuration
    run by mtp_relax_cell_step (include/mtp_mi355x.h, "batched variable-cell relaxation").  Every argument of relax_cells has
    its meaning there.  `pressure` [eV/A^3; 1 GPa = capi.GPA = 1 / 160.21766 eV/A^3]; `stol` [eV/A^3]: a configuration has
    converged when its largest |f_i| <= ftol AND the largest |W'_ab| / V <= stol, W' = (W - p V I) o mask the virial that drives
    the cell.  `cell_mask` (xx yy zz xy xz yz; 0 or 1): which components do; all 0 keeps the cells fixed.  `isotropic`: the cell
    changes its volume only.  `cell_factor` [A]: the length L that turns the deformation D (the cell is h = h0 . D, the atoms sit
    at x = xt . D) into the coordinates L D the minimiser moves -- default the configuration's atom count -- and `cell_mass`
    [g/mol] their mass, default the mean of `masses`.  `dmax` caps every generalised coordinate: |dD_ab| <= dmax / L per step.

    Step s = 0 ... steps: ghosts follow (their shifts deformed with the cell by mtp_ghosts_deform after every move) -> ONE force
    call with per-atom energies and virials -> ghost fold -> the virial per configuration (mtp_batch_reduce) -> on a grade step
    the grades, mtp_sample_capture and the cells of the captured (a candidate is positions, the cell AT the graded step, types)
    -> mtp_relax_cell_step(s).  The lists are rebuilt every `every` steps or when max_k (2 sqrt(d2[k]) + cellmove[k]) exceeds the
    skin (cell_list_stale), seen in the one read of the monitor: its block, d2 and cellmove.  A rebuild reads the cells back,
    lays the pass out again for them -- MtpError(-24) naming the configuration if they no longer fit one pass -- and builds
    ghosts and lists for them.

    Returns what relax_cells returns; final[k] also has cell [3, 3], virial [6] (W at x and cell), volume, enthalpy = energy +
    pressure * volume and smax (as fmax: at the last step the minimiser looked at it), and trace=True adds smax and volume
    [steps_done + 1, ncfg] (volume: of the cell the step's forces were taken in)."""
    who = "relax_cells_vc"
    batch, capture, mass_of_type, fire, dt = _relax_arguments(
        configs, steps, ftol, dt, dt_max, dmax, n_min, f_inc, f_dec, alpha_start, f_alpha, masses, threshold_select, threshold_break,
        capture_gap, max_candidates, grade_every, every, check_every, who)
    stol, pressure, cell_factor, cell_mass, mask, per_atom = _relax_vc_arguments(batch[2], mass_of_type, pressure, stol, cell_mask,
                                                                                 isotropic, cell_factor, cell_mass)
    params = capi.relax_cell_params(fire, stol, pressure, cell_factor, cell_mass, mask, isotropic, per_atom)
    setup = _RunSetup(who, ctx, batch, mass_of_type, capture=capture, steps=steps, every=every, check_every=check_every,
                      trace_names=("energy", "fmax", "smax", "volume") if trace else (), list_cutoff=list_cutoff,
                      max_atoms_per_pass=max_atoms_per_pass, device=device)
    torch, dev, st, zeros = setup.torch, setup.dev, setup.st, setup.zeros

    def one_pass(run):
        ncfg, A = run.ncfg, run.A
        A.update(vt=zeros(run.n, 3), vq=zeros(ncfg, 9), dt=torch.full((ncfg,), dt, dtype=torch.float64, device=dev),
                 alpha=torch.full((ncfg,), fire.alpha_start, dtype=torch.float64, device=dev),
                 npos=torch.zeros(ncfg, dtype=torch.int32, device=dev),
                 done_step=torch.full((ncfg,), -1, dtype=torch.int32, device=dev), fmax=zeros(ncfg), smax=zeros(ncfg),
                 gcell=zeros(ncfg, 9))
        run.v = A["vt"]

        def step(s, last):
            if trace:
                run.trace[3, s].copy_(_det3(A["h"].view(ncfg, 3, 3)))
            capi.relax_cell_step(ncfg, params, s, A, last=last, stream=st)
            if trace:
                run.energies(run.trace[0, s])
                run.trace[1, s].copy_(A["fmax"])
                run.trace[2, s].copy_(A["smax"])

        s = _minimise_pass(run, setup.steps, setup.graded, step, setup.every, setup.check_every)

        def final(xh, eh):
            fh, dh = run.frozen.cpu().numpy(), A["done_step"].cpu().numpy()
            hh, wh = A["h"].cpu().numpy().reshape(ncfg, 3, 3), A["virial"].cpu().numpy()
            dth, fmh, smh = A["dt"].cpu().numpy(), A["fmax"].cpu().numpy(), A["smax"].cpu().numpy()
            with np.errstate(all="ignore"):
                vol = _det3(hh)
            return [dict(x=xh[a:b], energy=float(eh[j]), fmax=float(fmh[j]), status=capi.RELAX_STATUS[int(fh[j])], step=int(dh[j]),
                         dt=float(dth[j]), cell=hh[j].copy(), virial=wh[j].copy(), volume=float(vol[j]),
                         enthalpy=float(eh[j]) + pressure * float(vol[j]), smax=float(smh[j])) for j, (a, b) in enumerate(run.rows)]

        return s, final

    def empty_final(k):
        return dict(x=np.zeros((0, 3)), energy=0.0, fmax=0.0, status=capi.RELAX_STATUS[0], step=-1, dt=dt,
                    cell=setup.all_cells[k].copy(), virial=np.zeros(6), volume=float(setup.volume[k]),
                    enthalpy=pressure * float(setup.volume[k]), smax=0.0)

    setup.each_pass(one_pass, empty_final, _DeformingCellRun)
    return setup.result()


def _npt_arguments(pressure, compressibility, tau_p, t_damp, cell_mask, isotropic, strain_max):
    """the host-side checks of sample_cells_npt's own arguments (nothing here touches the device); returns (pressure,
    compressibility, tau_p or None: the barostat is off, t_damp, cell_mask [6], strain_max)"""
    who = "sample_cells_npt"
    pressure, compressibility, strain_max = float(pressure), float(compressibility), float(strain_max)
    if not np.isfinite(pressure):
        raise ValueError("%s: pressure must be finite, got %r" % (who, pressure))
    if not (np.isfinite(compressibility) and compressibility > 0.0):
        raise ValueError("%s: compressibility must be positive and finite, got %r" % (who, compressibility))
    if t_damp is None or not (np.isfinite(float(t_damp)) and float(t_damp) > 0.0):
        raise ValueError("%s: t_damp must be positive and finite (the barostat's noise is at the thermostat's temperature), got %r"
                         % (who, t_damp))
    if not 0.0 < strain_max <= 0.05:
        raise ValueError("%s: strain_max must be in (0, 0.05], got %r" % (who, strain_max))
    mask = _cell_mask(who, cell_mask)
    if isotropic and mask[:3] != [1, 1, 1]:
        raise ValueError("%s: isotropic needs the three diagonal entries of cell_mask to be 1, got %r" % (who, cell_mask))
    if tau_p is not None:
        tau_p = float(tau_p)
        if not (np.isfinite(tau_p) and tau_p > 0.0):
            tau_p = None
    return pressure, compressibility, tau_p, float(t_damp), mask, strain_max


def sample_cells_npt(ctx, configs, temperature, pressure, steps, dt, *, compressibility, tau_p=1.0, t_damp=0.1,
                     cell_mask=(1, 1, 1, 1, 1, 1), isotropic=False, strain_max=0.01, seed=0, keys=None, masses=183.84, grade_every=10,
                     threshold_select=None, threshold_break=None, capture_gap=0, max_candidates=None, velocities=None,
                     list_cutoff=7.0, every=10, check_every=4, max_atoms_per_pass=None, device=None, trace=False):
    """sample_cells at constant pressure: Langevin MD of a whole batch of independent periodic cells at the target `temperature`
    [K] and `pressure` [eV/A^3; 1 GPa = capi.GPA], device-resident, the cell of every configuration moved by stochastic cell
    rescaling -- a first-order stochastic barostat in the spirit of Bernetti & Bussi, J. Chem. Phys. 153, 114107 (2020), one
    state machine per configuration run by mtp_sample_cell_step (include/mtp_mi355x.h, "batched constant-pressure sampling":
    the move, its noise and where its terms come from).  Every argument of sample_cells has its meaning there; grade watching
    and capture are sample_cells', and a candidate carries the cell of its graded step.

    `compressibility` [A^3/eV] is an estimate of the isothermal compressibility and `tau_p` [ps] the barostat's time: together
    they set how fast the cell answers (M = compressibility / (3 tau_p V0), V0 the volume given), not where it ends up.
    tau_p None, not finite or not positive, or a `cell_mask` (xx yy zz xy xz yz; 0 or 1) of zeros: the cells stay as given, and
    the trajectory is sample_cells'.  `isotropic`: the cell changes its volume only.  `strain_max` (at most 0.05) caps every
    component of the log-strain of one step; final[k]["capped"] counts the steps at which it did.  A finite positive `t_damp`
    is required: the barostat's noise is at the thermostat's temperature.  A flexible cell also rotates slowly (symmetric
    strains do not commute); energies, forces and virials are invariant under it and nothing removes it.

    Step 0 is sample_cells' step 0 with the virial tallied.  Step s = 1 ... steps: mtp_sample_cell_step(s) (kick, the kinetic
    tensor, the barostat move from the virial of the PREVIOUS force call, drift) -> ghosts follow the cell (mtp_ghosts_deform)
    -> ONE force call with per-atom virials -> ghost fold -> the virial per configuration -> mtp_sample_final -> on a grade
    step mtp_sample_capture and the cells of the captured.  Lists are rebuilt as in relax_cells_vc: every `every` steps or when
    cell_list_stale says so at the one read of the monitor (every `check_every` steps since the last rebuild); a rebuild lays
    the pass out again for the cells as they are.  A configuration whose virial, kinetic tensor or volume is not finite (or
    whose volume is not positive) fails: it is not written again.

    Returns what sample_cells returns (frozen [ncfg]: True for every configuration that no longer moves); final[k] also has
    cell [3, 3], volume, virial [6] (W at x and cell), pressure = tr (W + Kt) / (3 V) [eV/A^3], capped, status ("running",
    "captured-frozen" or "failed") and step (of the failure, -1 otherwise); trace=True adds volume (of the cell the step's
    forces were taken in) and pressure [steps_done + 1, ncfg]."""
    who = "sample_cells_npt"
    batch, capture, keys, temperature, mass_of_type, velocities = _sample_arguments(
        configs, temperature, steps, dt, keys, masses, threshold_select, threshold_break, capture_gap, max_candidates, velocities,
        grade_every, every, check_every, who)
    pressure, compressibility, tau_p, t_damp, mask, strain_max = _npt_arguments(pressure, compressibility, tau_p, t_damp, cell_mask,
                                                                                isotropic, strain_max)
    setup = _RunSetup(who, ctx, batch, mass_of_type, capture=capture, steps=steps, every=every, check_every=check_every,
                      trace_names=("energy", "kinetic", "volume", "pressure") if trace else (), list_cutoff=list_cutoff,
                      max_atoms_per_pass=max_atoms_per_pass, device=device)
    torch, dev, to, st, zeros = setup.torch, setup.dev, setup.to, setup.st, setup.zeros
    dt, seed = float(dt), int(seed) & (2 ** 64 - 1)
    dtf = 0.5 * dt * FTM2V
    barostat = tau_p is not None and any(mask)
    params = capi.sample_cell_params(dt, dtf, tau_p, compressibility, pressure, strain_max, mask, isotropic, seed)
    if velocities is None:
        velocities = maxwell_boltzmann(setup.items, mass_of_type, temperature, seed, keys)
    frozen_all = np.zeros(len(setup.items), dtype=bool)

    def one_pass(run):
        k0, k1, n, ncfg, A = run.k0, run.k1, run.n, run.ncfg, run.A
        run.v = v = to(np.concatenate(velocities[k0:k1]))
        A.update(v=v, mass=setup.mass_t, temperature=to(temperature[k0:k1]), key=to(keys[k0:k1].view(np.int64)),
                 V0=to(setup.volume[k0:k1]), done_step=torch.full((ncfg,), -1, dtype=torch.int32, device=dev),
                 capped=torch.zeros(ncfg, dtype=torch.int32, device=dev), press=zeros(ncfg))

        def first_half(step):
            capi.sample_cell_step(ncfg, params, step, A, stream=st)
            if barostat:
                run.moved()

        def second_half(step, kick):
            capi.sample_final(n, run.row_cfg, run.cf_t, run.frozen, v, run.f, run.buf.tall, setup.mass_t, setup.inv_mass_t,
                              A["temperature"], A["key"], seed, step, dtf if kick else 0.0, dt, t_damp, stream=st)

        def record(step):                                     # (pressure: tr W + 2 K over 3 V, from the monitor's sum m v^2)
            run.energies(run.trace[0, step])
            run.monitor(run.trace[1, step])
            vol = _det3(A["h"].view(ncfg, 3, 3))
            run.trace[2, step].copy_(vol)
            run.trace[3, step].copy_((run.virial[:, :3].sum(1) + MVV2E * run.trace[1, step]) / (3.0 * vol))

        s = _sample_pass(run, setup.steps, setup.graded, setup.every, setup.check_every, first_half, second_half,
                         record if trace else None)

        def final(xh, eh):                                    # (the harness ran the monitor once more: sum m v^2 at the end)
            vh, mh, fh = v.cpu().numpy(), run.mv2.cpu().numpy(), run.frozen.cpu().numpy()
            hh, wh = A["h"].cpu().numpy().reshape(ncfg, 3, 3), run.virial.cpu().numpy()
            dh, ch = A["done_step"].cpu().numpy(), A["capped"].cpu().numpy()
            frozen_all[k0:k1] = fh != 0
            with np.errstate(all="ignore"):
                vol = _det3(hh)
                press = (wh[:, :3].sum(1) + MVV2E * mh) / (3.0 * vol)
            return [dict(x=xh[a:b], v=vh[a:b], energy=float(eh[j]),
                         temperature=float(mh[j]) * MVV2E / (3.0 * (b - a) * KB) if b > a else 0.0, cell=hh[j].copy(),
                         volume=float(vol[j]), virial=wh[j].copy(), pressure=float(press[j]) if b > a else 0.0, capped=int(ch[j]),
                         status=capi.RELAX_STATUS[int(fh[j])], step=int(dh[j])) for j, (a, b) in enumerate(run.rows)]

        return s, final

    def empty_final(k):
        return dict(x=np.zeros((0, 3)), v=np.zeros((0, 3)), energy=0.0, temperature=0.0, cell=setup.all_cells[k].copy(),
                    volume=float(setup.volume[k]), virial=np.zeros(6), pressure=0.0, capped=0, status=capi.RELAX_STATUS[0], step=-1)

    setup.each_pass(one_pass, empty_final, _DeformingCellRun, final_monitor=True)
    out = setup.result(frozen=frozen_all)
    if trace:
        out["trace"]["kinetic"] = 0.5 * MVV2E * out["trace"]["kinetic"]
    return out


def _minimum_image(d, cell, cell_inv):
    """d - rint(d . h^-1) . h, rows of `cell` the lattice vectors: what mtp_neb_step applies to every difference of two images"""
    return d - np.rint(d @ cell_inv) @ cell


def interpolate_band(pos_a, pos_b, cell, nimages):
    """Host only: `nimages` >= 2 images from pos_a to pos_b [n, 3], linear in the minimum-image difference of the two under
    `cell` (rows = lattice vectors) -- an atom that crosses a periodic boundary between the two takes the short way.  The first
    image is pos_a, the last pos_a + mic(pos_b - pos_a): pos_b up to lattice vectors.  The images are continuous (not wrapped)."""
    a = np.asarray(pos_a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(pos_b, dtype=np.float64).reshape(-1, 3)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    if a.shape != b.shape:
        raise ValueError("interpolate_band: %d and %d atoms" % (len(a), len(b)))
    if int(nimages) < 2:
        raise ValueError("interpolate_band: at least 2 images")
    d = _minimum_image(b - a, cell, np.linalg.inv(cell))
    return [a + d * (i / (int(nimages) - 1.0)) for i in range(int(nimages))]


def plan_band_passes(cells, natoms, band_first, list_cutoff, max_atoms_per_pass=None):
    """Host arithmetic only: plan_cell_passes for a batch whose configurations [band_first[b], band_first[b + 1]) form bands
    that must stay together.  A boundary of plan_cell_passes that falls inside a band moves to the band's start, and so does a
    split the layout's limits ask for; a band that does not fit a pass alone raises MtpError(-24) and names the band.  The pass
    that follows a moved boundary gains the images that were in front of it: it may hold more owned atoms than
    `max_atoms_per_pass` (and more rows than plan_cell_passes' guard of 2^31 - 2^20), by less than one band's worth -- as a
    single configuration above the cap does in plan_cell_passes; only the layout's limits are checked again.  Returns what
    plan_cell_passes returns."""
    band_first = np.asarray(band_first, dtype=np.int64)
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    cut = float(list_cutoff)
    passes, volume, max_rows = plan_cell_passes(cells, natoms, cut, max_atoms_per_pass)
    band_start = lambda k: int(band_first[np.searchsorted(band_first, k, side="right") - 1])
    starts = sorted({band_start(k0) for k0, _, _ in passes})
    queue = [(a, b) for a, b in zip(starts, starts[1:] + [len(cells)])]
    queue.reverse()
    out = []
    while queue:
        k0, k1 = queue.pop()
        try:
            out.append((k0, k1, capi.batch_layout(cells[k0:k1], cut, cut)))
        except capi.MtpError as e:
            if e.code != -24:
                raise
            mid = band_start(k0 + int(getattr(e, "nfit", 0)))
            if mid <= k0:
                raise capi.MtpError(-24, "neb_cells: band %d (configurations %d to %d) does not fit a pass on its own: %s"
                                    % (int(np.searchsorted(band_first, k0, side="right")) - 1, k0,
                                       int(band_first[np.searchsorted(band_first, k0, side="right")]) - 1, e)) from e
            queue.append((mid, k1))
            queue.append((k0, mid))
    return out, volume, max_rows


def _neb_arguments(bands, spring, climb_after):
    """the host-side checks neb_cells adds to those of relax_cells (nothing here touches the device).  Returns the images of all
    bands as configurations, the band table and the climb step."""
    configs, band_first = [], [0]
    if not (np.isfinite(float(spring)) and float(spring) > 0.0):
        raise ValueError("neb_cells: spring must be positive and finite, got %r" % (spring,))
    if climb_after is not None and int(climb_after) < 0:
        raise ValueError("neb_cells: climb_after is a number of steps, or None for no climbing image")
    for b, band in enumerate(bands):
        images, cell = band[0], np.asarray(band[1], dtype=np.float64).reshape(3, 3)
        types = band[2] if len(band) > 2 else None
        images = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3) for p in images]
        if not 3 <= len(images) <= capi.NEB_MAX_IMAGES:
            raise ValueError("neb_cells: band %d has %d images: 3 to %d are possible" % (b, len(images), capi.NEB_MAX_IMAGES))
        if len({len(p) for p in images}) != 1 or len(images[0]) == 0:
            raise ValueError("neb_cells: band %d: every image needs the same, non-zero number of atoms, got %s"
                             % (b, [len(p) for p in images]))
        with np.errstate(all="ignore"):
            cross = np.stack([np.cross(cell[1], cell[2]), np.cross(cell[2], cell[0]), np.cross(cell[0], cell[1])])
            volume = float(cell[0] @ cross[0])
            heights = volume / np.sqrt((cross * cross).sum(1))
        if not (np.isfinite(cell).all() and volume > 0.0):
            raise ValueError("neb_cells: band %d: the cell must be finite, right-handed and non-degenerate (det > 0)" % b)
        inv = np.linalg.inv(cell)
        for i in range(len(images) - 1):
            d = _minimum_image(images[i + 1] - images[i], cell, inv)
            far = float(np.sqrt((d * d).sum(1)).max())
            if not far <= 0.25 * float(heights.min()):
                raise ValueError("neb_cells: band %d: an atom moves %.3f A between images %d and %d, more than a quarter of the "
                                 "smallest cell height (%.3f A): the minimum image is not exact, use more images or a larger cell"
                                 % (b, far, i, i + 1, float(heights.min())))
        configs += [(p, cell, types) for p in images]
        band_first.append(len(configs))
    return configs, np.array(band_first, dtype=np.int32), -1 if climb_after is None else int(climb_after)


def neb_cells(ctx, bands, steps, spring=5.0, climb_after=None, ftol=1e-3, dt=1e-3, dt_max=1e-2, dmax=0.1, n_min=5, f_inc=1.1,
              f_dec=0.5, alpha_start=0.1, f_alpha=0.99, masses=183.84, grade_every=0, threshold_select=None, threshold_break=None,
              capture_gap=0, max_candidates=None, list_cutoff=7.0, every=10, check_every=4, max_atoms_per_pass=None, device=None,
              trace=False):
    """What follows relax_cells in the active-learning loop: the minimum-energy paths between minima and their barriers, for a
    whole batch of independent bands at once, device-resident -- the climbing-image nudged elastic band with the improved
    tangent (Henkelman & Jonsson, JCP 113, 9978; Henkelman, Uberuaga & Jonsson, JCP 113, 9901), one FIRE state machine per band,
    run by mtp_neb_step -- while the extrapolation grade is watched as in sample_cells: the transition state is where a
    potential extrapolates most.  `bands` is a sequence of (images: [pos [n, 3], ...], cell, types): 3 to 64 images of the same
    atoms in the same, fixed cell (interpolate_band makes a first guess).  The first and the last image are never moved.

    The images of all bands are the configurations of one batch (passes, lists and capture arguments as relax_cells; a band is
    never split between passes: plan_band_passes).  Step s = 0 ... steps is: ONE force call over all rows -> ghost fold -> on a
    grade step mtp_sample_capture -> mtp_neb_step(s): image energies, tangents and spring forces under the minimum image (a
    re-neighbouring wraps every image on its own), F_neb = F - (F.t) t + spring (|D+| - |D-|) t, from step `climb_after` on
    (None: never) F - 2 (F.t) t for the interior image of highest energy, then FIRE over the interior rows of the band (the
    FIRE arguments are those of relax_cells; `ftol` bounds the largest |F_neb| of an atom).  A band stops as "converged",
    "failed" (a non-finite force or energy, or a vanishing tangent) or "captured-frozen" (one of its images went over threshold_break;
    the band stops at the next mtp_neb_step); all its images are then frozen.  After step `steps` no move is made.

    Refused on the host before anything touches the device (ValueError): fewer than 3 or more than 64 images, differing or zero
    atom counts, a spring that is not positive, and a band in which an atom moves more than a quarter of the smallest cell
    height between two neighbouring images, after minimum image -- up to there the minimum image is the true difference.

    Returns dict(bands: per band dict(images: [M] positions [n, 3], made continuous along the band on the host -- the first as
    wrapped at the last rebuild, each next one unwrapped against the one before; energies [M]; barrier_forward, barrier_backward:
    the highest image energy minus that of the first and of the last image; highest: the index of that image; fmax: the largest
    |F_neb| at the last step the band was looked at; status: "running", "captured-frozen", "converged" or "failed"; step: the
    step at which it stopped, -1 otherwise; dt); candidates, records, dropped: as sample_cells, configuration numbers counting
    the images of all bands in order; final: per image dict(x, energy); steps_done; builds) and, with trace=True (one more
    launch and a copy a step), trace: dict(energy [steps_done + 1, number of images], fmax [steps_done + 1, number of bands])."""
    configs, band_first, climb_step = _neb_arguments(bands, spring, climb_after)
    batch, capture, mass_of_type, fire, dt = _relax_arguments(
        configs, steps, ftol, dt, dt_max, dmax, n_min, f_inc, f_dec, alpha_start, f_alpha, masses, threshold_select, threshold_break,
        capture_gap, max_candidates, grade_every, every, check_every, who="neb_cells")
    params = capi.NebParams(fire, float(spring), climb_step)
    setup = _RunSetup("neb_cells", ctx, batch, mass_of_type, capture=capture, steps=steps, every=every, check_every=check_every,
                      trace_names=("energy", "fmax") if trace else (), list_cutoff=list_cutoff, max_atoms_per_pass=max_atoms_per_pass,
                      device=device, replan=lambda plan: plan_band_passes(batch[1], batch[2], band_first, list_cutoff, max_atoms_per_pass)[0])
    torch, dev, st = setup.torch, setup.dev, setup.st
    results = [None] * len(bands)

    def one_pass(run):
        b0, b1 = int(np.searchsorted(band_first, run.k0)), int(np.searchsorted(band_first, run.k1))
        nband, ncfg = b1 - b0, run.ncfg
        bf = (band_first[b0: b1 + 1] - run.k0).astype(np.int32)
        cells = run.cells[bf[:-1]]
        run.v = v = setup.zeros(run.n, 3)
        state = setup.zeros(3, nband)
        state[0].fill_(dt)
        state[1].fill_(fire.alpha_start)
        ints = torch.zeros((4, nband), dtype=torch.int32, device=dev)      # npos, done_step, climber, band_status
        ints[1:3].fill_(-1)
        first_t = setup.to(bf[:-1].astype(np.int64))
        A = dict(band_first=setup.to(bf), cfg_first=run.cf_t, v=v, type=run.buf.tall, inv_mass=setup.inv_mass_t, origins=run.org_t,
                 cell=setup.to(cells.reshape(nband, 9)), cell_inv=setup.to(np.linalg.inv(cells).reshape(nband, 9)),
                 fneb=setup.zeros(run.n, 3), energy=setup.zeros(ncfg), dt=state[0], alpha=state[1], fmax=state[2], npos=ints[0],
                 done_step=ints[1], climber=ints[2], band_status=ints[3], frozen=run.frozen, counts=run.counts_t)

        def step(s, last):
            A.update(x=run.x, f=run.f, eatom=run.eatom)           # (a rebuild lays the work array out again)
            capi.neb_step(bf, ncfg, params, s, A, last=last, stream=st)
            if trace:
                run.energies(run.trace[0, s])
                run.trace[1, s].index_copy_(0, first_t, state[2])     # (a band's fmax sits at its first image)

        s = _minimise_pass(run, setup.steps, setup.graded, step, setup.every, setup.check_every)

        def final(xh, eh):
            sh, ih = state.cpu().numpy(), ints.cpu().numpy()
            for j in range(nband):
                k0, k1 = int(bf[j]), int(bf[j + 1])
                inv = np.linalg.inv(cells[j])
                images = [xh[slice(*run.rows[k0])].copy()]
                for k in range(k0 + 1, k1):
                    images.append(images[-1] + _minimum_image(xh[slice(*run.rows[k])] - images[-1], cells[j], inv))
                e = eh[k0:k1].copy()
                top = int(np.argmax(e))
                results[b0 + j] = dict(images=images, energies=e, barrier_forward=float(e[top] - e[0]),
                                       barrier_backward=float(e[top] - e[-1]), highest=top, fmax=float(sh[2, j]),
                                       status=capi.NEB_STATUS[int(ih[3, j])], step=int(ih[1, j]), dt=float(sh[0, j]))
            return [dict(x=xh[a:b], energy=float(eh[j])) for j, (a, b) in enumerate(run.rows)]

        return s, final

    setup.each_pass(one_pass, lambda k: dict(x=np.zeros((0, 3)), energy=0.0), _CellRun)
    out = setup.result(bands=results)
    if trace:
        out["trace"]["fmax"] = out["trace"]["fmax"][:, band_first[:-1].astype(np.int64)]
    return out


def _hessian_selections(atoms, natoms):
    """the selected atoms of every configuration as int64 index arrays (None: all of them, in order); out of range or repeated
    entries raise"""
    if atoms is None:
        atoms = [None] * len(natoms)
    if len(atoms) != len(natoms):
        raise ValueError("hessian_cells: atoms is None or one entry per configuration (%d), got %d" % (len(natoms), len(atoms)))
    out = []
    for k, a in enumerate(atoms):
        n = int(natoms[k])
        a = np.arange(n, dtype=np.int64) if a is None else np.asarray(a, dtype=np.int64).reshape(-1)
        if len(a) and (a.min() < 0 or a.max() >= n):
            raise ValueError("hessian_cells: configuration %d: atoms must be in [0, %d)" % (k, n))
        if len(np.unique(a)) != len(a):
            raise ValueError("hessian_cells: configuration %d: an atom is selected more than once" % k)
        out.append(a)
    return out


def _hessian_sizes(nsel, max_hessian_bytes):
    """the bytes of every configuration's Hessian, (3 m_j)^2 * 8; one above `max_hessian_bytes` on its own raises, named"""
    size = 8 * (3 * np.asarray(nsel, dtype=np.int64)) ** 2
    over = np.nonzero(size > int(max_hessian_bytes))[0]
    if len(over):
        raise ValueError("hessian_cells: configuration %d: its Hessian of %d selected atoms takes %d bytes, above max_hessian_bytes "
                         "(%d)" % (int(over[0]), int(nsel[over[0]]), int(size[over[0]]), int(max_hessian_bytes)))
    return size


def cut_hessian_passes(plan, cells, nsel, list_cutoff, max_hessian_bytes=2 ** 31):
    """Host arithmetic only: the passes `plan` of plan_cell_passes cut further so that the Hessians of a pass, sum (3 m_j)^2 * 8
    bytes with m_j = nsel[j] selected atoms, stay within `max_hessian_bytes` (a configuration is never split; one that is above
    the limit on its own raises, named).  A pass that is cut gets the layouts of its pieces."""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    size, limit = _hessian_sizes(nsel, max_hessian_bytes), int(max_hessian_bytes)
    cut, out = float(list_cutoff), []
    for k0, k1, lay in plan:
        pieces, begin, used = [], k0, 0
        for k in range(k0, k1):
            if k > begin and used + int(size[k]) > limit:
                pieces.append((begin, k))
                begin, used = k, 0
            used += int(size[k])
        pieces.append((begin, k1))
        out += [(k0, k1, lay)] if len(pieces) == 1 else [(a, b, capi.batch_layout(cells[a:b], cut, cut)) for a, b in pieces]
    return out


def _positive_step(who, name, value):
    """the difference step `name` of driver `who` as a float, or ValueError"""
    if not (float(value) > 0.0 and np.isfinite(float(value))):
        raise ValueError("%s: %s must be positive and finite, got %r" % (who, name, float(value)))
    return float(value)


def _displacement_in_skin(who, name, value, ctx, list_cutoff):
    """an atom displaced by `value` [A] keeps its list: ValueError unless it is below half the skin"""
    skin = float(list_cutoff) - float(ctx.pot.info.max_cutoff)
    if not value < 0.5 * skin:
        raise ValueError("%s: %s (%g A) must stay below half the skin (list_cutoff - cutoff = %g A): the list has to "
                         "hold for every displaced copy" % (who, name, value, skin))


def _hessian_pass(run, setup, selections, h, mass_weight, status):
    """The difference loop of hessian_cells and of the ionic arm of elastic_cells.  `selections`: per configuration of the pass
    the indices, into the configuration, of its differentiated atoms (None: all); `status` [ncfg] int32 on the device: a configuration that
    has failed is skipped, one that fails here is marked.  Saves x and runs 6 max_j m_j + 1 times "forces, mtp_hess_step", then
    mtp_hess_finish.  Returns dict(H: the blocks [3 m_j, 3 m_j], from h_first[j]; f0 [n, 3]; state [2, ncfg]: fmax, energy; diag
    [ncfg, 2]: asymmetry, sum rule; blocks(): after the synchronise, the blocks on the host, NaN where status says failed).
    The last element of `sel` only keeps the table from being empty: no kernel reads it, whatever it holds."""
    to, zeros, ncfg, n = setup.to, setup.zeros, run.ncfg, run.n
    m = run.counts.astype(np.int64) if selections is None else np.array([len(a) for a in selections], dtype=np.int64)
    rows = [np.arange(n)] if selections is None else [run.rows[j][0] + selections[j] for j in range(ncfg)]
    sel = np.concatenate(rows + [np.zeros(1, dtype=np.int64)])
    first = np.concatenate([[0], np.cumsum((3 * m) ** 2)])
    sel_first_t, sel_t = to(np.concatenate([[0], np.cumsum(m)]).astype(np.int32)), to(sel.astype(np.int32))
    h_first_t = to(first[:-1].astype(np.int64))
    H, x0, sel_max = zeros(max(int(first[-1]), 1)), run.x[:n].clone(), int(m.max())
    f0, state, diag = zeros(n, 3), zeros(2, ncfg), zeros(ncfg, 2)
    for k in range(6 * sel_max + 1):
        run.forces(False)
        capi.hess_step(run.cf_t, sel_first_t, sel_t, sel_max, k, h, run.x, x0, run.f, run.eatom, h_first_t, H, f0, state[0], state[1],
                       status, stream=run.st)
    capi.hess_finish(sel_first_t, sel_t, run.buf.tall, setup.mass_t, mass_weight, h_first_t, H, diag, status, stream=run.st)

    def blocks():
        Hh, failed = H.cpu().numpy(), status.cpu().numpy() == 1
        return [np.full((N, N), np.nan) if bad else Hh[at: at + N * N].reshape(N, N).copy()
                for N, at, bad in zip(3 * m, first, failed)]

    return dict(H=H, h_first=h_first_t, f0=f0, state=state, diag=diag, blocks=blocks)


def hessian_cells(ctx, configs, h=0.01, atoms=None, mass_weight=False, masses=183.84, list_cutoff=7.0, max_atoms_per_pass=None,
                  max_hessian_bytes=2 ** 31, device=None, modes=False, project_translations=None, zero_tol=1e-3, vectors=False):
    """What follows relax_cells and neb_cells: the second derivatives at their stationary points, for a whole batch of
    independent periodic cells at once, device-resident -- force constants by central differences of the forces with the step
    `h` [A].  `configs` and the passes are those of evaluate_cells (`list_cutoff`, `max_atoms_per_pass`); a displacement of `h`
    is far inside the skin (list_cutoff - the potential's cutoff; h >= half of it raises), so ONE ghost build and ONE list serve
    all the force calls of a pass: 6 max_j m_j + 1 of them, each followed by ONE launch of mtp_hess_step, which harvests the
    forces of the displacement just made into its row of H, restores the coordinate from the saved copy and makes the next
    displacement.  Nothing is read back before the end of the pass, where mtp_hess_finish measures the asymmetry and the sum rule
    and symmetrises.

    `atoms`: None (every atom), or one entry per configuration: None, or the indices (into its `pos`) of the m atoms whose
    coordinates are differentiated -- the others stay where they are, and H is the [3 m, 3 m] block of those atoms in the order
    given.  Entries out of range or repeated raise.  mass_weight=True divides H[3a+d, 3b+e] by sqrt(M_a M_b) on the device
    (`masses`: one, or one per atom type [g/mol]).  The passes are cut further so that the Hessians of one pass stay within
    `max_hessian_bytes` (cut_hessian_passes; a single configuration above it raises, named).

    Returns one dict per configuration: hessian [3 m, 3 m] (symmetrised; eV/A^2, or eV/(A^2 g/mol) when mass-weighted; row
    3 a + d is the displaced coordinate, column 3 b + e the responding one), atoms [m], energy and f0 [n, 3] (in the order of
    `pos`) at the undisplaced positions, fmax = the largest |f0_i|, asymmetry = max |H_cr - H_rc| before symmetrising (an
    O(h^2) truncation quantity), sum_rule = max |sum_b H[c, 3 b + e]| (below), status: "ok" or "failed" (a force that was not
    finite: the Hessian is then NaN; the other configurations are not affected).  An empty configuration, or an empty
    selection, gives a (0, 0) Hessian.

    sum_rule is taken from the matrix AS HARVESTED, before it is symmetrised, like the asymmetry -- not from the returned
    `hessian`.  Row c of the harvested matrix holds the forces that displacement c left on the selected atoms, over 2 h; summed
    over all atoms they vanish to rounding (Newton's third law in the force call), so for a full selection sum_rule is the
    translation-invariance residual of the force path and stays within 3 n times the force parity bound over h.  The column
    sums, and with them the row sums of the symmetrised `hessian`, vanish only to O(h^2) and have no such bound; that is why
    modes() projects the translations out instead of relying on them.

    modes=True: the normal modes of every Hessian of a pass are solved on the device (mtp_eigh_batched) from the blocks
    mtp_hess_finish left, before anything is copied back; the masses of the selected atoms weight a Hessian that is not yet
    mass-weighted.  The dicts gain the keys of modes() -- frequencies, eigenvalues, eigenvectors (None unless `vectors`),
    n_unstable, n_zero (`zero_tol`) -- and modes_status (capi.EIGH_STATUS; "failed" with NaN frequencies where the Hessian failed)
    and solver: "device", or "host" for a matrix above the solver's size (capi.EIGH_MAX_N coordinates, capi.EIGH_MAX_N_VECTORS
    with `vectors`), which goes through modes().  project_translations: None projects the translations out of the full selections
    only; True or False decides for all.  `hessian` is returned as without modes."""
    batch = items, all_cells, natoms = _batch_items(configs)
    h = _positive_step("hessian_cells", "h", h)
    mass_of_type = _mass_of_type("hessian_cells", items, masses)
    selections = _hessian_selections(atoms, natoms)
    nsel = np.array([len(a) for a in selections], dtype=np.int64)
    if modes and not (float(zero_tol) >= 0.0):
        raise ValueError("hessian_cells: zero_tol must not be negative")
    project = (nsel == natoms) if project_translations is None else np.full(len(nsel), bool(project_translations))
    _displacement_in_skin("hessian_cells", "h", h, ctx, list_cutoff)
    _hessian_sizes(nsel, max_hessian_bytes)                   # (a configuration too large raises before anything is set up)
    setup = _RunSetup("hessian_cells", ctx, batch, mass_of_type, list_cutoff=list_cutoff, max_atoms_per_pass=max_atoms_per_pass,
                      device=device, replan=lambda plan: cut_hessian_passes(plan, all_cells, nsel, list_cutoff, max_hessian_bytes))

    def empty(k):
        out = dict(hessian=np.zeros((0, 0)), atoms=selections[k], energy=0.0, f0=np.zeros((0, 3)), fmax=0.0, asymmetry=0.0,
                   sum_rule=0.0, status=capi.HESS_STATUS[0])
        if modes:
            out.update(_hessian_modes_keys(_modes_dict(np.zeros(0), np.zeros((0, 0)) if vectors else None, zero_tol, 0, 0, "device")))
        return out

    def one_pass(run):
        k0 = run.k0
        status = setup.torch.zeros(run.ncfg, dtype=setup.torch.int32, device=setup.dev)
        hp = _hessian_pass(run, setup, selections[k0: run.k1], h, mass_weight, status)
        if modes:     # solved from the blocks on the device; a Hessian that failed is skipped and stays "failed"
            sel, root = selections[k0: run.k1], None
            if not mass_weight:
                root = [np.repeat(np.sqrt(mass_of_type[items[k0 + j][1][a] - 1]), 3) for j, a in enumerate(sel)]
            solve = _eigh_device(setup.torch, setup.dev, run.st, 3 * nsel[k0: run.k1], hp["h_first"], hp["H"], root, project[k0: run.k1],
                                 30, vectors, status)

        def final(xh, eh):
            fh, sh, dh, th = hp["f0"].cpu().numpy(), hp["state"].cpu().numpy(), hp["diag"].cpu().numpy(), status.cpu().numpy()
            Hh, out = hp["blocks"](), []
            found = solve(zero_tol) if modes else None
            for j, (a, b) in enumerate(run.rows):
                if b == a:
                    out.append(empty(k0 + j))
                    continue
                out.append(dict(hessian=Hh[j], atoms=selections[k0 + j], energy=float(sh[1, j]), f0=fh[a:b],
                                fmax=float(sh[0, j]), asymmetry=float(dh[j, 0]), sum_rule=float(dh[j, 1]),
                                status=capi.HESS_STATUS[int(th[j])]))
                if modes:
                    if found[j] is None:     # above the solver's size: the host routine, on the Hessian as returned
                        M = None if mass_weight else mass_of_type[items[k0 + j][1][selections[k0 + j]] - 1]
                        found[j] = _host_modes(Hh[j], M, bool(project[k0 + j]), zero_tol, vectors)
                    out[-1].update(_hessian_modes_keys(found[j]))
            return out

        return 0, final

    setup.each_pass(one_pass, empty, _CellRun)
    return setup.final


def modes(hessian, masses_of_atoms, project_translations=True, zero_tol=1e-3):
    """Host only: the normal modes of one Hessian of hessian_cells.  `hessian` [3 m, 3 m] in eV/A^2 with `masses_of_atoms` [m]
    (or one mass) in g/mol -- it is mass-weighted here, D = H / sqrt(M_a M_b) --, or already mass-weighted with
    masses_of_atoms=None (then the translations are taken as uniform).  With `project_translations` the three uniform
    translations are projected out of D first (they come out as zero modes to rounding); this is meaningful for a FULL selection
    only: pass False for the block of a partial one.  numpy's eigh, eigenvalues lambda ascending.

    Returns dict(frequencies [3 m] in THz, nu = sign(lambda) sqrt(|lambda| FTM2V) / (2 pi): unstable modes come out NEGATIVE, the
    convention of phonon codes; eigenvectors [3 m, 3 m], column i the mass-weighted mode of frequencies[i]; eigenvalues [3 m] in
    eV/(A^2 g/mol); n_unstable: the modes with nu < -zero_tol; n_zero: those with |nu| <= zero_tol [THz])."""
    H = np.array(hessian, dtype=np.float64)
    if H.ndim != 2 or H.shape[0] != H.shape[1] or H.shape[0] % 3:
        raise ValueError("modes: the Hessian must be [3 m, 3 m], got %r" % (H.shape,))
    if not np.isfinite(H).all():
        raise ValueError("modes: the Hessian is not finite (a failed configuration?)")
    if not (float(zero_tol) >= 0.0):
        raise ValueError("modes: zero_tol must not be negative")
    m = H.shape[0] // 3
    if masses_of_atoms is None:
        root = np.ones(3 * m)
    else:
        M = np.asarray(masses_of_atoms, dtype=np.float64).reshape(-1)
        M = np.full(m, M[0]) if len(M) == 1 else M
        if len(M) != m or not ((M > 0.0).all() and np.isfinite(M).all()):
            raise ValueError("modes: masses_of_atoms is one positive mass, or one per atom (%d)" % m)
        root = np.repeat(np.sqrt(M), 3)
        H = H / np.outer(root, root)
    H = 0.5 * (H + H.T)
    if project_translations and m:
        T = np.zeros((3 * m, 3))
        for d in range(3):
            T[d::3, d] = root[d::3]
        T /= np.linalg.norm(T, axis=0)
        P = np.eye(3 * m) - T @ T.T
        H = P @ H @ P
        H = 0.5 * (H + H.T)
    lam, vec = np.linalg.eigh(H) if m else (np.zeros(0), np.zeros((0, 0)))
    nu = np.sign(lam) * np.sqrt(np.abs(lam) * FTM2V) / (2.0 * np.pi)
    return dict(frequencies=nu, eigenvectors=vec, eigenvalues=lam, n_unstable=int((nu < -zero_tol).sum()),
                n_zero=int((np.abs(nu) <= zero_tol).sum()))


def _modes_dict(lam, vec, zero_tol, status, sweeps, solver):
    """the dict of modes() from eigenvalues (the same expression of lambda for the frequencies), with status, sweeps and solver"""
    nu = np.sign(lam) * np.sqrt(np.abs(lam) * FTM2V) / (2.0 * np.pi)
    return dict(frequencies=nu, eigenvectors=vec, eigenvalues=lam, n_unstable=int((nu < -zero_tol).sum()),
                n_zero=int((np.abs(nu) <= zero_tol).sum()), status=capi.EIGH_STATUS[int(status)], sweeps=int(sweeps), solver=solver)


def _host_modes(hessian, masses_of_atoms, project, zero_tol, vectors):
    """a matrix the device does not take: modes(), in the dict of the device path"""
    out = modes(hessian, masses_of_atoms, project, zero_tol)
    out.update(eigenvectors=out["eigenvectors"] if vectors else None, status=capi.EIGH_STATUS[0], sweeps=0, solver="host")
    return out


def _hessian_modes_keys(found):
    """what hessian_cells takes over from a dict of the solver: its status becomes modes_status"""
    out = {k: found[k] for k in ("frequencies", "eigenvalues", "eigenvectors", "n_unstable", "n_zero", "solver")}
    out["modes_status"] = found["status"]
    return out


def _eigh_device(torch, dev, st, sizes, first_t, A_t, roots, project, max_sweeps, vectors, status_t):
    """What modes_cells and hessian_cells(modes=True) share: mtp_eigh_batched over the matrices [N_j, N_j] that lie on the device
    at A_t + first_t[j] (sizes [nmat]), with `roots` (None, or per matrix the square roots of the masses, one per coordinate)
    and per matrix `project`; a matrix with status_t[j] != 0 is skipped (status_t itself is not written).  The kernel takes one
    projection flag a launch, so a batch that mixes both is solved in two, each skipping the other's matrices.  Nothing is
    copied back here: the returned function read(zero_tol) does that (the copies wait for the stream) and gives, per matrix, the
    dict of _modes_dict, or None where the device did not take the matrix (status "too large")."""
    sizes, project = np.asarray(sizes, dtype=np.int64), np.asarray(project, dtype=bool)
    nmat, w_first = len(sizes), np.concatenate([[0], np.cumsum(sizes)])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = lambda count: torch.full((max(int(count), 1),), float("nan"), dtype=torch.float64, device=dev)
    n_t, w_first_t = to(sizes.astype(np.int32)), to(w_first[:-1].astype(np.int64))
    root_t = None if roots is None else to(np.concatenate(list(roots) + [np.ones(1)]).astype(np.float64))
    W, V, info = full(w_first[-1]), (full((sizes ** 2).sum()) if vectors else None), full(2 * nmat).view(-1, 2)
    done = status_t.clone()
    for flag in (False, True):
        pick = project == flag
        if not pick.any():
            continue
        if pick.all():
            capi.eigh_batched(n_t, first_t, A_t, w_first_t, root_t, flag, max_sweeps, W, V, info, done, stream=st)
            continue
        pick_t = to(pick)
        mine = torch.where(pick_t, done, torch.full_like(done, -1))
        capi.eigh_batched(n_t, first_t, A_t, w_first_t, root_t, flag, max_sweeps, W, V, info, mine, stream=st)
        done = torch.where(pick_t, mine, done)

    def read(zero_tol):
        Wh, ih, sh = W.cpu().numpy(), info.cpu().numpy(), done.cpu().numpy()
        Vh, at = (V.cpu().numpy(), first_t.cpu().numpy()) if vectors else (None, None)
        out = []
        for j, N in enumerate(sizes):
            if sh[j] == 3:
                out.append(None)
                continue
            lam = Wh[w_first[j]: w_first[j + 1]].copy()
            vec = Vh[at[j]: at[j] + N * N].reshape(N, N).copy() if vectors else None
            out.append(_modes_dict(lam, vec, zero_tol, sh[j], 0 if np.isnan(ih[j, 0]) else ih[j, 0], "device"))
        return out

    return read


def modes_cells(hessians, masses_of_atoms=None, project_translations=True, zero_tol=1e-3, vectors=False, max_sweeps=30, device=None):
    """modes() for a whole list of Hessians [3 m_j, 3 m_j] at once, solved on the device: mtp_eigh_batched, cyclic Jacobi in
    LDS, one workgroup a matrix.  `masses_of_atoms`: None (the Hessians are mass-weighted already), one number, or one entry per
    matrix with the meaning it has in modes() (None, one mass, or one per atom).  `project_translations`, `zero_tol`: as in
    modes().  Wrong shapes and masses, and a Hessian that is not finite, raise before the device is touched.

    Returns one dict per matrix with the keys of modes() -- frequencies from the same expression of the eigenvalues, eigenvectors
    None unless `vectors` -- and status (capi.EIGH_STATUS: "not converged" after `max_sweeps` sweeps that all rotated, with the
    state reached), sweeps, and solver: "device", or "host" for a matrix of more than capi.EIGH_MAX_N coordinates
    (capi.EIGH_MAX_N_VECTORS with `vectors`), which goes through modes()."""
    if not (float(zero_tol) >= 0.0):
        raise ValueError("modes_cells: zero_tol must not be negative")
    if int(max_sweeps) < 1:
        raise ValueError("modes_cells: max_sweeps must be at least 1")
    mats = [np.array(H, dtype=np.float64) for H in hessians]
    if masses_of_atoms is None or np.isscalar(masses_of_atoms):
        per = [masses_of_atoms] * len(mats)
    elif len(masses_of_atoms) == len(mats):
        per = list(masses_of_atoms)
    else:
        raise ValueError("modes_cells: masses_of_atoms is None, one number, or one entry per matrix (%d), got %d"
                         % (len(mats), len(masses_of_atoms)))
    roots = []
    for j, (H, M) in enumerate(zip(mats, per)):
        if H.ndim != 2 or H.shape[0] != H.shape[1] or H.shape[0] % 3:
            raise ValueError("modes_cells: matrix %d: the Hessian must be [3 m, 3 m], got %r" % (j, H.shape))
        if not np.isfinite(H).all():
            raise ValueError("modes_cells: matrix %d: the Hessian is not finite (a failed configuration?)" % j)
        m = H.shape[0] // 3
        if M is None:
            roots.append(np.ones(3 * m))
            continue
        M = np.asarray(M, dtype=np.float64).reshape(-1)
        M = np.full(m, M[0]) if len(M) == 1 else M
        if len(M) != m or not ((M > 0.0).all() and np.isfinite(M).all()):
            raise ValueError("modes_cells: matrix %d: masses_of_atoms is one positive mass, or one per atom (%d)" % (j, m))
        roots.append(np.repeat(np.sqrt(M), 3))
    if not mats:
        return []
    import torch
    dev = device or torch.device("cuda:0")
    st = _torch_stream(dev)
    sizes = np.array([len(H) for H in mats], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(sizes ** 2)])
    A_t = torch.from_numpy(np.concatenate([H.reshape(-1) for H in mats] + [np.zeros(1)])).to(dev)
    first_t = torch.from_numpy(first[:-1].astype(np.int64)).to(dev)
    status_t = torch.zeros(len(mats), dtype=torch.int32, device=dev)
    weighted = any(M is not None for M in per)
    found = _eigh_device(torch, dev, st, sizes, first_t, A_t, roots if weighted else None, np.full(len(mats), bool(project_translations)),
                         int(max_sweeps), bool(vectors), status_t)(zero_tol)
    return [_host_modes(mats[j], per[j], bool(project_translations), zero_tol, vectors) if f is None else f
            for j, f in enumerate(found)]


def vineyard_prefactor(freq_min, freq_saddle, zero_tol=1e-3):
    """Host only: the harmonic transition-state prefactor of Vineyard (J. Phys. Chem. Solids 3, 121), nu* = prod nu_min /
    prod' nu_saddle over the stable, non-zero modes (nu > zero_tol) of modes() at the minimum and at the saddle, in the unit of
    the frequencies (THz); the rate is nu* exp(-barrier / kB T).  Evaluated through sums of logarithms.  Raises unless the
    minimum has no unstable mode, the saddle exactly one (nu < -zero_tol), and the saddle one stable mode fewer than the
    minimum."""
    lo, hi = np.asarray(freq_min, dtype=np.float64).reshape(-1), np.asarray(freq_saddle, dtype=np.float64).reshape(-1)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("vineyard_prefactor: the frequencies must be finite")
    if int((lo < -zero_tol).sum()):
        raise ValueError("vineyard_prefactor: the minimum has %d unstable modes: it is no minimum" % int((lo < -zero_tol).sum()))
    if int((hi < -zero_tol).sum()) != 1:
        raise ValueError("vineyard_prefactor: the saddle has %d unstable modes, a first-order saddle has exactly one"
                         % int((hi < -zero_tol).sum()))
    stable_lo, stable_hi = lo[lo > zero_tol], hi[hi > zero_tol]
    if len(stable_hi) != len(stable_lo) - 1:
        raise ValueError("vineyard_prefactor: %d stable modes at the minimum, %d at the saddle: the saddle must have one fewer"
                         % (len(stable_lo), len(stable_hi)))
    return float(np.exp(np.log(stable_lo).sum() - np.log(stable_hi).sum()))


# ---- elastic constants: the second derivatives with respect to the cell -------------------------------------------------------

VOIGT = (0, 1, 2, 5, 4, 3)    # Voigt's 11 22 33 23 13 12 in the project's order xx yy zz xy xz yz
_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
_COMPONENT = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 0): 3, (0, 2): 4, (2, 0): 4, (1, 2): 5, (2, 1): 5}


def to_voigt(M):
    """Host only: a [6] vector or [6, 6] matrix in the project's component order xx yy zz xy xz yz, reordered to Voigt's
    11 22 33 23 13 12 (a permutation; the engineering-shear convention is the same in both)"""
    M = np.asarray(M, dtype=np.float64)
    if M.shape == (6,):
        return M[list(VOIGT)].copy()
    if M.shape != (6, 6):
        raise ValueError("to_voigt: a [6] vector or a [6, 6] matrix, got %r" % (M.shape,))
    return M[np.ix_(VOIGT, VOIGT)].copy()


def stress_correction(stress):
    """Host only: K [6, 6] of Wallace's relation for the Cauchy stress `stress` [6] (xx yy zz xy xz yz),
    K_ijkl = (d_ik s_jl + d_jk s_il + d_il s_jk + d_jl s_ik - 2 d_kl s_ij) / 2 with row (i, j) and column (k, l): the
    stress-strain coefficients B of a stressed state and the second derivatives C of its energy with respect to Lagrangian strain,
    per volume, differ by it, C = B - K.  K - K^T = d s^T - s d^T with d = (1, 1, 1, 0, 0, 0)."""
    s = np.asarray(stress, dtype=np.float64)
    if s.shape != (6,):
        raise ValueError("stress_correction: the stress is [6] (xx yy zz xy xz yz), got %r" % (s.shape,))
    sg = lambda a, b: s[_COMPONENT[(a, b)]]
    dl = lambda a, b: 1.0 if a == b else 0.0
    K = np.zeros((6, 6))
    for v, (i, j) in enumerate(_PAIRS):
        for w, (k, l) in enumerate(_PAIRS):
            K[v, w] = 0.5 * ((((dl(i, k) * sg(j, l) + dl(j, k) * sg(i, l)) + dl(i, l) * sg(j, k)) + dl(j, l) * sg(i, k))
                             - 2.0 * dl(k, l) * sg(i, j))
    return K


def moduli(C):
    """Host only: the polycrystalline moduli of one matrix of elastic constants `C` [6, 6] (eV/A^3, engineering shears; the
    project's order or Voigt's: every quantity here is the same for both).  Returns dict(bulk_voigt, bulk_reuss, bulk_hill,
    shear_voigt, shear_reuss, shear_hill [eV/A^3]; compressibility = 1 / bulk_reuss [A^3/eV], what sample_cells_npt takes;
    born_stable: the smallest eigenvalue of sym(C) is positive; min_eigenvalue).  A matrix that is not [6, 6], not finite or
    singular raises."""
    C = np.asarray(C, dtype=np.float64)
    if C.shape != (6, 6):
        raise ValueError("moduli: the elastic constants are [6, 6], got %r" % (C.shape,))
    if not np.isfinite(C).all():
        raise ValueError("moduli: the elastic constants are not finite (a failed configuration?)")
    C = 0.5 * (C + C.T)
    lam = np.linalg.eigvalsh(C)
    if not np.abs(lam).min() > 0.0:
        raise ValueError("moduli: the matrix of elastic constants is singular")
    S = np.linalg.inv(C)
    n3, s3 = slice(0, 3), slice(3, 6)
    dia = lambda M: float(np.trace(M[n3, n3]))
    off = lambda M: float(M[0, 1] + M[0, 2] + M[1, 2])
    shr = lambda M: float(np.trace(M[s3, s3]))
    kv, gv = (dia(C) + 2.0 * off(C)) / 9.0, (dia(C) - off(C) + 3.0 * shr(C)) / 15.0
    kr, gr = 1.0 / (dia(S) + 2.0 * off(S)), 15.0 / (4.0 * dia(S) - 4.0 * off(S) + 3.0 * shr(S))
    return dict(bulk_voigt=kv, bulk_reuss=kr, bulk_hill=0.5 * (kv + kr), shear_voigt=gv, shear_reuss=gr, shear_hill=0.5 * (gv + gr),
                compressibility=1.0 / kr, born_stable=bool(lam[0] > 0.0), min_eigenvalue=float(lam[0]))


def relax_ions(B, C, coupling, hessian, volume, internal_strain=None):
    """Host only: the ionic term of the elastic constants, by the algorithm of mtp_elastic_relax in numpy (elastic_cells uses it
    for the configurations above capi.ELASTIC_RELAX_MAX_N coordinates).  `B`, `C` [6, 6]: the clamped birch and elastic of
    elastic_cells; `coupling` [6, 3 n] = Lambda; `hessian` [3 n, 3 n] of hessian_cells for ALL atoms, not mass-weighted (it is
    symmetrised here); `volume` V0.  A = H + tau sum_d t_d t_d^T with the three normalised translations t_d and tau =
    trace(H) / 3 n, factorised by Cholesky; U = A^-1 Lambda^T (Lambda^T, with the mean over the atoms taken out of every row, is
    orthogonal to the translations, so this is H^+ Lambda^T at a minimum), R = Lambda U^T.  With `internal_strain` [6, 3 n] given, that U is used and nothing is solved.
    Returns dict(internal_strain=U [6, 3 n], birch_relaxed = B - R / V0, elastic_relaxed = C - sym(R) / V0, status "ok" or
    "unstable": A is not positive definite -- the configuration is no minimum -- and the three are NaN)."""
    B, C = np.asarray(B, dtype=np.float64), np.asarray(C, dtype=np.float64)
    Lam, H = np.asarray(coupling, dtype=np.float64), np.asarray(hessian, dtype=np.float64)
    N = Lam.shape[1] if Lam.ndim == 2 else -1
    if B.shape != (6, 6) or C.shape != (6, 6) or Lam.ndim != 2 or Lam.shape[0] != 6 or N % 3 or H.shape != (N, N):
        raise ValueError("relax_ions: B and C are [6, 6], coupling [6, 3 n] and hessian [3 n, 3 n], got %r, %r, %r, %r"
                         % (B.shape, C.shape, Lam.shape, H.shape))
    V0 = float(volume)
    if not (V0 > 0.0 and np.isfinite(V0)):
        raise ValueError("relax_ions: the volume must be positive and finite, got %r" % (volume,))
    status = capi.ELASTIC_STATUS[0]
    if N:                                                     # what rounding left of a translation in Lambda is taken out
        Lam = (Lam.reshape(6, N // 3, 3) - Lam.reshape(6, N // 3, 3).mean(1, keepdims=True)).reshape(6, N)
    if internal_strain is not None:
        U = np.asarray(internal_strain, dtype=np.float64)
        if U.shape != Lam.shape:
            raise ValueError("relax_ions: internal_strain is [6, 3 n] like the coupling, got %r" % (U.shape,))
    elif N <= 3:                                              # one atom: only the translations, nothing relaxes
        U = np.zeros((6, N))
    else:
        A = 0.5 * (H + H.T)
        tau = float(np.trace(A)) / N
        for d in range(3):
            A[d::3, d::3] += tau / (N // 3)
        try:
            if not np.isfinite(A).all():
                raise np.linalg.LinAlgError("not finite")
            L = np.linalg.cholesky(A)
            U = np.linalg.solve(L.T, np.linalg.solve(L, Lam.T)).T
        except np.linalg.LinAlgError:
            nan = np.full((6, 6), np.nan)
            return dict(internal_strain=np.full((6, N), np.nan), birch_relaxed=nan, elastic_relaxed=nan.copy(),
                        status=capi.ELASTIC_STATUS[2])
    R = Lam @ U.T
    return dict(internal_strain=U, birch_relaxed=B - R / V0, elastic_relaxed=C - 0.5 * (R + R.T) / V0, status=status)


_relax_ions_on_host = relax_ions                              # (elastic_cells has a parameter of the public name)


def elastic_cells(ctx, configs, h=0.005, relax_ions=False, h_atoms=0.01, list_cutoff=7.0, max_atoms_per_pass=None,
                  max_hessian_bytes=2 ** 31, device=None):
    """What hessian_cells leaves out: the second derivatives with respect to the CELL -- elastic constants -- for a whole batch of
    independent periodic cells at once, device-resident.  `configs` and the passes are those of evaluate_cells.  A pass makes ONE
    ghost build and ONE list and runs 13 force calls with per-atom virials on them, at zero strain and at x -> x (I +- h E_w) for
    the six components w (order xx yy zz xy xz yz; a shear E_w has 1/2 on both off-diagonal entries: engineering shear), the
    atoms at fixed scaled coordinates and the ghosts following through mtp_ghosts_deform; mtp_elastic_step harvests between the
    calls and mtp_elastic_finish ends the pass (include/mtp_mi355x.h, "batched elastic constants").  Nothing is read back before
    the end of the pass.  `h` must stay below half the skin over the list cutoff: a pair inside the cutoff after the strain was
    inside the list before it.

    Returns one dict per configuration (eV, A; to_voigt reorders to 11 22 33 23 13 12):
      stress [6]       the Cauchy stress sigma = -W / V at zero strain [eV/A^3]
      birch [6, 6]     B[v][w] = d sigma_v / d eps_w by central differences, as harvested.  NOT symmetric under residual stress:
                       B - B^T = d sigma^T - sigma d^T + O(h^2), d = (1, 1, 1, 0, 0, 0)
      elastic [6, 6]   C = sym(B - K(sigma)), K = stress_correction(stress) (Wallace): the second derivatives of the energy with
                       respect to Lagrangian strain, per volume; moduli(C) gives bulk and shear moduli and the compressibility
      asymmetry        max |(B - K) - (B - K)^T| before symmetrising, an O(h^2) truncation quantity
      coupling [6, 3n] Lambda[w][3 i + d] = d f_id / d eps_w at fixed scaled coordinates;  sum_rule = max |sum_i Lambda[w][3 i + d]|,
                       the translation-invariance residual, of rounding size
      energy, f0 [n, 3], fmax, volume, status: "ok", "failed" (a force or virial that was not finite: the matrices are NaN; the
      other configurations are not affected) or "unstable" (below)
    All of these are for CLAMPED ions.  relax_ions=True goes on, in the same pass, with the force constants of all atoms
    (hessian_cells' loop, displacement `h_atoms` [A], 6 n + 1 more force calls; the passes are then cut by cut_hessian_passes to
    `max_hessian_bytes`) and mtp_elastic_relax, and adds
      hessian [3n, 3n], internal_strain [6, 3n] = U = H^+ Lambda^T (the displacements per unit strain),
      birch_relaxed = B - Lambda U^T / V, elastic_relaxed = C - sym(Lambda U^T) / V
    "unstable": the Hessian has a negative mode, the relaxed matrices are NaN, the clamped ones stay.  The ionic term is exact
    only where the forces vanish -- d sigma_v / d u_c = -Lambda[v][c] / V has a correction of size |f0| / V otherwise -- so relax
    with relax_cells or relax_cells_vc first and look at the `fmax` returned here.  An empty configuration gives zeros of the
    right shapes."""
    who = "elastic_cells"
    batch = items, all_cells, natoms = _batch_items(configs)
    h, h_atoms = _positive_step(who, "h", h), _positive_step(who, "h_atoms", h_atoms)
    skin = float(list_cutoff) - float(ctx.pot.info.max_cutoff)
    if not h < 0.5 * skin / float(list_cutoff):
        raise ValueError("elastic_cells: h (%g) must stay below half the skin over the list cutoff (%g / %g / 2 = %g): the list has to "
                         "hold for every strained copy" % (h, skin, float(list_cutoff), 0.5 * skin / float(list_cutoff)))
    _displacement_in_skin(who, "h_atoms", h_atoms, ctx, list_cutoff)
    ionic = bool(relax_ions)
    if ionic:
        _hessian_sizes(natoms, max_hessian_bytes)
    setup = _RunSetup(who, ctx, batch, _mass_of_type(who, items, 1.0), list_cutoff=list_cutoff, max_atoms_per_pass=max_atoms_per_pass,
                      device=device,
                      replan=(lambda plan: cut_hessian_passes(plan, all_cells, natoms, list_cutoff, max_hessian_bytes)) if ionic else None)
    torch, dev, st, to, zeros = setup.torch, setup.dev, setup.st, setup.to, setup.zeros

    def empty(k):
        z = lambda *s: np.zeros(s)
        out = dict(stress=z(6), birch=z(6, 6), elastic=z(6, 6), coupling=z(6, 0), asymmetry=0.0, sum_rule=0.0, energy=0.0,
                   f0=z(0, 3), fmax=0.0, volume=float(setup.volume[k]), status=capi.ELASTIC_STATUS[0])
        if ionic:
            out.update(hessian=z(0, 0), internal_strain=z(6, 0), birch_relaxed=z(6, 6), elastic_relaxed=z(6, 6))
        return out

    def one_pass(run):
        k0, ncfg, n, A = run.k0, run.ncfg, run.n, run.A
        cf = run.cf.astype(np.int64)
        c_first_t = to(18 * cf[:-1])
        x0 = run.x[:n].clone()
        f0, state, diag = zeros(n, 3), zeros(2, ncfg), zeros(ncfg, 2)
        stress0, Bt, B, Cm, coupling = zeros(ncfg, 6), zeros(ncfg, 36), zeros(ncfg, 36), zeros(ncfg, 36), zeros(max(18 * n, 1))
        status = torch.zeros(ncfg, dtype=torch.int32, device=dev)
        for k in range(13):
            run.forces(False)
            capi.elastic_step(run.cf_t, k, h, run.x, x0, A["xt"], run.org_t, A["h0"], run.f, run.eatom, run.virial, A["T"], Bt,
                              coupling, c_first_t, f0, state[0], state[1], stress0, status, stream=st)
            run.moved()
        capi.elastic_finish(run.cf_t, c_first_t, coupling, stress0, Bt, B, Cm, diag, status, stream=st)
        if ionic:                                             # (the strain loop left x = x0, and its failures in `status`)
            U, B_rel, C_rel = zeros(max(18 * n, 1)), zeros(ncfg, 36), zeros(ncfg, 36)
            hp = _hessian_pass(run, setup, None, h_atoms, False, status)
            capi.elastic_relax(run.cf_t, hp["h_first"], hp["H"], c_first_t, coupling, to(setup.volume[k0: run.k1]), B, Cm, U, B_rel,
                               C_rel, status, stream=st)

        def final(xh, eh):
            fh, sh, dh, th = f0.cpu().numpy(), state.cpu().numpy(), diag.cpu().numpy(), status.cpu().numpy()
            s0, Bh, Ch, Lh = stress0.cpu().numpy(), B.cpu().numpy(), Cm.cpu().numpy(), coupling.cpu().numpy()
            if ionic:
                Hh, Uh, Brh, Crh = hp["blocks"](), U.cpu().numpy(), B_rel.cpu().numpy(), C_rel.cpu().numpy()
            out = []
            for j, (a, b) in enumerate(run.rows):
                if b == a:
                    out.append(empty(k0 + j))
                    continue
                N, code = 3 * (b - a), int(th[j])
                r = dict(stress=s0[j].copy(), birch=Bh[j].reshape(6, 6).copy(), elastic=Ch[j].reshape(6, 6).copy(),
                         coupling=Lh[18 * a: 18 * b].reshape(6, N).copy(), asymmetry=float(dh[j, 0]), sum_rule=float(dh[j, 1]),
                         energy=float(sh[1, j]), f0=fh[a:b], fmax=float(sh[0, j]), volume=float(setup.volume[k0 + j]))
                if code == 1:
                    for key in ("birch", "elastic", "coupling"):
                        r[key][:] = np.nan
                if ionic:
                    r["hessian"] = Hh[j]
                    if code == 1:
                        r.update(internal_strain=np.full((6, N), np.nan), birch_relaxed=np.full((6, 6), np.nan),
                                 elastic_relaxed=np.full((6, 6), np.nan))
                    elif N > capi.ELASTIC_RELAX_MAX_N:                # above the largest LDS tier: the same algorithm on the host
                        more = _relax_ions_on_host(r["birch"], r["elastic"], r["coupling"], r["hessian"], r["volume"])
                        code = capi.ELASTIC_STATUS.index(more.pop("status"))
                        r.update(more)
                    else:
                        r.update(internal_strain=Uh[18 * a: 18 * b].reshape(6, N).copy(), birch_relaxed=Brh[j].reshape(6, 6).copy(),
                                 elastic_relaxed=Crh[j].reshape(6, 6).copy())
                r["status"] = capi.ELASTIC_STATUS[code]
                out.append(r)
            return out

        return 0, final

    setup.each_pass(one_pass, empty, _DeformingCellRun)
    return setup.final
