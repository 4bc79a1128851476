// The statements of the force kernel, included INSIDE the body of a __global__ function template with the parameters
// <int KL, int NB, int PITCH, bool GRADE, int DEG, int WPS> and a type SH in scope (no include guard: mtp_kernels.hip
// includes it into mtp_wave_kernel with SH = ShapeGeneric, mtp_kernels_fixed.hip into mtp_wave_kernel_fixed with SH =
// its Shape parameter).  Textual inclusion, not a device function the kernels call: the generic kernels then compile
// exactly as they did when the statements stood in mtp_wave_kernel itself (with the body wrapped in an inlined device
// function, <64,2,33,false,11,2> spilled 89 VGPR dwords where profiles/r05_code_objects.txt records 87).
//
// WPS = wavefronts per SIMD the register budget is sized for: 2 (<= 256 VGPRs, workgroups of up to 8 wavefronts) or
// 3 (<= 168 VGPRs, workgroups of up to 12: one workgroup per CU puts three wavefronts on every SIMD)
//
// SH (mtp_shape_fields.hpp) is the shape of the launch: the fields of the argument block it fixes are compile-time
// constants here (SHF / SHA), the others are read from the block.  ShapeGeneric fixes none.
  constexpr int NT = 32;                 // neighbours per tile
  // Product passes: the wide lane grids (KL = 64: level 18 and up, thousands of times rows that live in HBM / L2 either
  // way) run the gather programs -- measured at level 20: 2.02 -> 1.93 ms; the narrow grids keep the row-per-lane passes
  // with the rows in LDS -- at level 16 the gather programs (27 KB, so in L2) were 2.3 % slower (0.523 vs 0.511 ms).
  constexpr bool GATHER = KL == 64;
  // The 3-per-SIMD build is planned with the dg-free layouts only (its table shapes have Mu <= 4), so the dg paths are
  // compiled out of it; the 2-per-SIMD build takes either (uniform flag).
  constexpr bool NODG_CT = WPS == 3;
  // f' of the force phase from registers: the dg-free build of a shape that fixes the slot -> mu map (mtp_wave_body.hpp)
  constexpr bool FP_REGS = NODG_CT && fp_regs_ct<SH>;
  constexpr bool PHASE_PRIO = phase_prio_ct<SH>;   // s_setprio by phase (mtp_wave_body.hpp)
  constexpr int NG = 64 / KL;            // neighbour groups in the wavefront
  constexpr int NPG = NT / NG;           // neighbours per group per tile
  static_assert(NT == 32, "the force phase maps lanes to (32 neighbours) x (2 halves)");

  // the argument block is the kernel's only argument: it starts the kernarg segment
  KP kp = (KP) __builtin_amdgcn_kernarg_segment_ptr();
#ifdef MTP_STAMPS
  const unsigned long long st_entry = __builtin_amdgcn_s_memtime();
#endif
  kernarg_touch<(int) sizeof(MtpDevParams)>(kp);
  extern __shared__ double lds[];
  unsigned char *sh = reinterpret_cast<unsigned char *>(lds);
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction: tell the compiler, so per-atom state lives in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wpb = blockDim.x >> 6;

  // XCD-aware atom map: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so workgroup b works
  // for XCD b % 8; giving every XCD one contiguous eighth of ilist (callers keep atoms roughly in spatial order:
  // LAMMPS sorts them, the bench lattice is cell-major) keeps the position gathers and the force atomics of a slab in
  // ONE L2 instead of spreading every slab over all eight.
  int ii_beg, ii_end, ii_step;
  if (kp->xcd_map && (gridDim.x & 7) == 0) {
    const int chunk = (kp->inum + 7) >> 3, xcd = blockIdx.x & 7;
    // Rounds of (workgroups x wpb) atoms: when the last round is only partly filled, the wavefronts are numbered
    // wave-major, so that its atoms land on a few wavefronts of EVERY workgroup instead of on all wavefronts of a few
    // (65 536 atoms over 3 072 wavefronts = 21.33 rounds: -2.4 %); with whole rounds the block-major numbering keeps
    // neighbouring atoms on one CU (level 20, 32 rounds exactly: 0.3 % better).
    const int nb8 = gridDim.x >> 3;
    if (chunk % (nb8 * wpb) != 0) ii_beg = kp->row0 + xcd * chunk + wave * nb8 + (blockIdx.x >> 3);
    else ii_beg = kp->row0 + xcd * chunk + (blockIdx.x >> 3) * wpb + wave;
    ii_end = kp->row0 + min(kp->inum, (xcd + 1) * chunk);
    ii_step = (gridDim.x >> 3) * wpb;
  } else {
    ii_step = gridDim.x * wpb;
    if (kp->inum % ii_step != 0) ii_beg = kp->row0 + wave * gridDim.x + blockIdx.x;
    else ii_beg = kp->row0 + blockIdx.x * wpb + wave;
    ii_end = kp->row0 + kp->inum;
  }
  // The head of an atom's list row {ilist, first} is requested one atom ahead and carried in SGPRs: two dependent memory
  // round trips per atom instead of three, and the first atom's ride on the table copy below (what a 2,048-atom call
  // is made of: one atom per wavefront, every load a miss).
  int hd_i = 0, hd_b = 0, hd_e = 0;
  if (ii_beg < ii_end) {   // (uniform)
    hd_i = kp->ilist[ii_beg];
    hd_b = kp->first[ii_beg];
    hd_e = kp->first[ii_beg + 1];
  }
  // ---- 0. workgroup-shared tables ---------------------------------------------------------
  for (int o = threadIdx.x * 16; o < SHF(blob_bytes); o += blockDim.x * 16)
    *reinterpret_cast<uint4 *>(sh + o) = *reinterpret_cast<const uint4 *>(kp->blob + o);
  __syncthreads();
  BlockTables bt;
  bt.rows = reinterpret_cast<const MtpRow8 *>(sh + SHF(off_rows));
  bt.level = reinterpret_cast<const int *>(sh + SHF(off_level));
  bt.seg_fwd = reinterpret_cast<const int *>(sh + SHF(off_seg_fwd));
  bt.seg_bwd = reinterpret_cast<const int *>(sh + SHF(off_seg_bwd));
  bt.slot = reinterpret_cast<const int *>(sh + SHF(off_slot));
  bt.radial = reinterpret_cast<const double *>(sh + SHF(off_radial));
  bt.seed_idx = reinterpret_cast<const int *>(sh + SHF(off_seed_idx));
  bt.seed_val = reinterpret_cast<const double *>(sh + SHF(off_seed_val));
  bt.map = reinterpret_cast<const int *>(sh + SHF(off_map));
  bt.lin = reinterpret_cast<const double *>(sh + SHF(off_lin));
  bt.pack = reinterpret_cast<const int *>(sh + SHF(off_pack));
  bt.coef = reinterpret_cast<const int *>(sh + SHF(off_coef));
  bt.smu = reinterpret_cast<const int *>(sh + SHF(off_smu));
  bt.fwd = reinterpret_cast<const int *>(sh + SHF(off_fwd));
  bt.leaf_cf = reinterpret_cast<const double *>(sh + SHF(off_leaf_cf));   // (behind the rows: valid when rows_in_lds)
  bt.leaf_cb = reinterpret_cast<const double *>(sh + SHF(off_leaf_cb));
  const bool rows_lds = SHF(rows_in_lds) != 0;
  // row_regs_ct: the packed rows of the short product levels, this lane's row of each of their blocks
  constexpr bool ROW_REGS = !GATHER && MTP_PU >= ROW_KEEP_LEVEL && row_regs_ct<SH>;   // (the gather passes have no rows per level)
  MtpRow8 krow[kept_count<SH>()];
  if constexpr (ROW_REGS) load_kept_rows<SH, 0>(bt.rows, krow, lane);
  // row_keep_l1_ct: and its row of the first blocks of the first level (whole trips of the passes)
  constexpr bool KEEP_L1 = ROW_REGS && ROW_KEEP_L1 % MTP_PU == 0 && row_keep_l1_ct<SH>;
  MtpRow8 krow1[kept_l1_count<SH>()];
  if constexpr (KEEP_L1) load_kept_l1_rows<SH>(bt.rows, krow1, lane);
  // (not in the KL = 16 grade build: there the SGPR pair costs a twelfth spilled VGPR dword)
  constexpr bool MU_PACKED = WPS == 3 && !(GRADE && KL == 16);
  SlotMu<MU_PACKED> smu{bt.smu, 0ull};
  if constexpr (MU_PACKED && slot_mu_ct<SH>) {   // the shape's constant
    smu.bits = slot_mu_bits<SH>();
  } else if constexpr (MU_PACKED) {   // lane s holds mu(s): bit 0 of every slot by one ballot, bit 1 by another, interleaved
    const int mu_l = lane < min(SHF(nslot), 32) ? bt.smu[lane] : 0;
    const unsigned long long b0 = __ballot((mu_l & 1) != 0), b1 = __ballot((mu_l & 2) != 0);
    auto spread = [](unsigned long long x) {   // bit k -> bit 2 k (k < 32)
      x = (x | (x << 16)) & 0x0000ffff0000ffffull;
      x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
      x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
      x = (x | (x << 2)) & 0x3333333333333333ull;
      return (x | (x << 1)) & 0x5555555555555555ull;
    };
    smu.bits = spread(b0) | (spread(b1) << 1);
  }

  const int kl = lane & (KL - 1), q = lane / KL;
  const unsigned wave_off = (SHF(blob_bytes) >> 3) + wave * kp->wave_doubles;   // doubles
  const unsigned lds0 = (unsigned) (size_t) (lds_cdouble *) lds;            // static cast of the array itself
  const WaveLds<PITCH> w(lds + wave_off, lds0 + 8u * wave_off, kp, SH{});
  const int P = SHF(P);

  // Basic-moment pass in 3 x 3 register blocks (built on the host, mtp_potential.cpp): lane (q, kl) owns the blocks
  // kl + KL t; a block is 3 heads (slot s, exponent a: head value g_s x^a) times 3 tails (b, c: tail value y^b z^c)
  // with b + c = nu_s - a for all of them, i.e. nine basics from twelve table rows.  Per block: LDS byte addresses of
  // the rows for this lane's neighbour column q.
  unsigned hg[NB][3], hx[NB][3], ty[NB][3], tz[NB][3];
  bool bval[NB];
  // (2-per-SIMD build: formed once per kernel; 3-per-SIMD build: once per atom, so that the twelve registers are free
  // outside the basic-moment pass)
  auto block_addresses = [&](int kl_) {
#pragma unroll
    for (int t = 0; t < NB; t++) {
      const int blk = kl_ + KL * t;
      bval[t] = blk < SHF(nfb);
      const int *bd = bt.fwd + 8 * (bval[t] ? blk : 0);
      const unsigned w0 = (unsigned) bd[0], w1 = (unsigned) bd[1], w2 = (unsigned) bd[2];
#pragma unroll
      for (int h = 0; h < 3; h++) {
        const unsigned tq = w.addr(w.tab + q);
        hg[t][h] = tq + (unsigned) mul24((int) ((w0 >> (8 * h)) & 255u), 8 * PITCH);
        hx[t][h] = tq + (unsigned) mul24(SHF(pow_row) + (int) ((w1 >> (4 * h)) & 15u), 8 * PITCH);
        ty[t][h] = tq + (unsigned) mul24(SHF(pow_row) + P + (int) ((w1 >> (12 + 4 * h)) & 15u), 8 * PITCH);
        tz[t][h] = tq + (unsigned) mul24(SHF(pow_row) + 2 * P + (int) ((w2 >> (4 * h)) & 15u), 8 * PITCH);
        // one finished address per register: stops the optimiser from re-splitting them into
        // base + row offset (which costs a v_add per LDS read in the inner loops)
        asm volatile("" : "+v"(hg[t][h]), "+v"(hx[t][h]), "+v"(ty[t][h]), "+v"(tz[t][h]));
      }
    }
  };
  if constexpr (WPS != 3) block_addresses(kl);
  // block_regs_ct: the row byte offsets of this lane's block, {g | x power} and {y power | z power} of head / tail h as
  // the 16-bit halves of bpk[h] and bpk[3 + h], decoded once per wavefront; block_offsets_to_addresses() per atom
  constexpr bool BLOCK_REGS = WPS == 3 && NB == 1 && block_regs_ct<SH>;
  unsigned bpk[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  // fwd5_ct (mtp_wave_body.hpp): the pass in five-factor blocks, lane (q, kl) owns block kl.  The block's eight words are
  // read from the blob in HBM / L2 once per wavefront (the table is in no LDS prefix) and stay in registers as
  // block_regs_ct keeps the 3 x 3 offsets: bpk5[f] = row byte offsets of factor f as 16-bit halves, kk5[] = the six
  // int16 basic indices in pairs, shape5 = the lanes whose factor 2 is a head (3 x 2 block), a lane mask in an SGPR
  // pair.  fa[f] / fb[f]: LDS byte addresses of the two rows of factor f for this lane's neighbour column, per atom.
  constexpr bool FWD5 = BLOCK_REGS && fwd5_ct<SH>;
  constexpr int NACC = FWD5 ? 6 : 9;   // products of a block
  // the trims of the five-factor force shape (mtp_wave_body.hpp: sum_t_ct, cnt_sgpr_ct)
  constexpr bool SUM_T = FWD5 && NG == 2 && sum_t_ct<SH>, CNT_SGPR = FWD5 && cnt_sgpr_ct<SH>;
  unsigned fa[5], fb[5];
  unsigned bpk5[5] = {0u, 0u, 0u, 0u, 0u}, kk5[3] = {0u, 0u, 0u};
  unsigned long long shape5 = 0ull;
  auto block5_addresses = [&]() {
    bval[0] = kl < SHF(nfb5);
    const unsigned tq = w.addr(w.tab + q);
#pragma unroll
    for (int f = 0; f < 5; f++) {
      asm volatile("" : "+v"(bpk5[f]));   // opaque per atom: the adds stay inside the loop
      fa[f] = tq + (bpk5[f] & 0xffffu);
      fb[f] = tq + (bpk5[f] >> 16);
      asm volatile("" : "+v"(fa[f]), "+v"(fb[f]));   // one finished address per register (block_addresses)
    }
  };
  if constexpr (FWD5) {
    const uint4 *bd = reinterpret_cast<const uint4 *>(kp->blob + SHF(off_fwd5)) + 2 * (kl < SHF(nfb5) ? kl : 0);
    const uint4 lo = bd[0], hi = bd[1];
    const unsigned wd[5] = {lo.x, lo.y, lo.z, lo.w, hi.x};
    if constexpr (SUM_T) {   // the indices of products 3 q + 0..2 in kk5[0..1]
      kk5[0] = q ? (hi.z >> 16) | (hi.w << 16) : hi.y;
      kk5[1] = q ? hi.w >> 16 : hi.z & 0xffffu;
    } else {
      kk5[0] = hi.y;
      kk5[1] = hi.z;
      kk5[2] = hi.w;
    }
    const bool head2 = (wd[2] >> 31) != 0u;
    shape5 = __ballot(head2);
#pragma unroll
    for (int f = 0; f < 5; f++) {   // a head {slot s, x^a} or a tail {y^b, z^c}: factor 2 by the block's shape
      const int r0 = (int) (wd[f] & 0xffffu), r1 = (int) ((wd[f] >> 16) & 0x7fffu);
      const bool head = f < 2 || (f == 2 && head2);
      const unsigned o0 = (unsigned) mul24(head ? r0 : SHF(pow_row) + P + r0, 8 * PITCH);
      const unsigned o1 = (unsigned) mul24(SHF(pow_row) + (head ? 0 : 2 * P) + r1, 8 * PITCH);
      bpk5[f] = o0 | (o1 << 16);
    }
  } else if constexpr (BLOCK_REGS) {
    const int *bd = bt.fwd + 8 * (kl < SHF(nfb) ? kl : 0);
    const unsigned w0 = (unsigned) bd[0], w1 = (unsigned) bd[1], w2 = (unsigned) bd[2];
#pragma unroll
    for (int h = 0; h < 3; h++) {
      const unsigned og = (unsigned) mul24((int) ((w0 >> (8 * h)) & 255u), 8 * PITCH);
      const unsigned ox = (unsigned) mul24(SHF(pow_row) + (int) ((w1 >> (4 * h)) & 15u), 8 * PITCH);
      const unsigned oy = (unsigned) mul24(SHF(pow_row) + P + (int) ((w1 >> (12 + 4 * h)) & 15u), 8 * PITCH);
      const unsigned oz = (unsigned) mul24(SHF(pow_row) + 2 * P + (int) ((w2 >> (4 * h)) & 15u), 8 * PITCH);
      bpk[h] = og | (ox << 16);
      bpk[3 + h] = oy | (oz << 16);
    }
  }
  auto block_offsets_to_addresses = [&]() {
    bval[0] = kl < SHF(nfb);
    const unsigned tq = w.addr(w.tab + q);
#pragma unroll
    for (int h = 0; h < 3; h++) {
      asm volatile("" : "+v"(bpk[h]), "+v"(bpk[3 + h]));   // opaque per atom: the adds stay inside the loop
      hg[0][h] = tq + (bpk[h] & 0xffffu);
      hx[0][h] = tq + (bpk[h] >> 16);
      ty[0][h] = tq + (bpk[3 + h] & 0xffffu);
      tz[0][h] = tq + (bpk[3 + h] >> 16);
      asm volatile("" : "+v"(hg[0][h]), "+v"(hx[0][h]), "+v"(ty[0][h]), "+v"(tz[0][h]));
    }
  };

  double tally = 0.0;   // lane 9: energy, lanes 3..8: virial components of this wave's atoms
  // Global-only tallies need no per-atom reduction: the per-lane partial sums of the virial (and of the energy) run
  // across the wavefront's atoms and cross the lanes once, after the atom loop.  Per-atom outputs (vatom: vflag & 4,
  // eatom: eflag & 2) keep the per-atom reductions.
  double vacc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, eacc = 0.0;
  // (Only in the 2-per-SIMD build: at 168 VGPRs the six virial accumulators spill 10 dwords, and deferring the energy
  // alone was measured equal -- 0.4044 against 0.4044 ms; when that build still spilled, all seven cost more than the
  // per-atom reductions: 0.514 against 0.500 ms.)
  const bool v_per_atom = WPS == 3 ? kp->vflag != 0 : (kp->vflag & 4) != 0;
  const bool e_per_atom = WPS == 3 ? true : (kp->eflag & 2) != 0;
#ifdef MTP_STAMPS
  unsigned long long st_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long st_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long st_prologue = st_prev - st_entry;   // argument block, table copy, barrier, first list head
  // the trace record of this wavefront (workgroups 0..7: one per XCD), and the atom it is at
  unsigned long long *st_trace = nullptr;
  int st_atom = 0;
  if (kp->stamps && blockIdx.x < MTP_TRACE_WGS && wave < MTP_MAX_WPB)
    st_trace = kp->stamps + 16 + (size_t) (blockIdx.x * MTP_MAX_WPB + wave) * MTP_TRACE_WAVE_WORDS;
  if (st_trace && lane == 0) {
    st_trace[0] = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_ID: wave slot [3:0], SIMD [5:4], CU [11:8], SE [15:13]
    st_trace[1] = __builtin_amdgcn_s_getreg(20 | (31 << 11));   // XCC_ID
    st_trace[2] = ii_beg < ii_end ? (unsigned long long) ((ii_end - ii_beg + ii_step - 1) / ii_step) : 0ull;
    st_trace[3] = st_entry;
    st_trace[4] = st_prev;
    st_trace[5] = __builtin_amdgcn_s_memtime();   // the first atom starts here
  }
  st_prev = __builtin_amdgcn_s_memtime();
#endif

  auto store_seeds = [&]() {   // D[seed_idx[k]] = seed_val[k]: the adjoints of the stored scalars
    if (SHF(scalars_in_lds))
      for (int k = lane; k < SHF(nseed); k += 64) w.D[bt.seed_idx[k]] = bt.seed_val[k];
    else
      for (int k = lane; k < SHF(nseed); k += 64) w.D[kp->g_seed_idx[k]] = kp->g_seed_val[k];
  };

  int nx_i = __builtin_amdgcn_readfirstlane(hd_i), nx_b = __builtin_amdgcn_readfirstlane(hd_b);
  int nx_n = __builtin_amdgcn_readfirstlane(hd_e) - nx_b;
  for (int ii = ii_beg; ii < ii_end; ii += ii_step) {
    phase_prio<PHASE_PRIO, MTP_PRIO_CHAIN>();   // loop head and compaction: dependent memory round trips
    // ii is wave-uniform, so is everything loaded through it: keep it in SGPRs.  Two dependent memory round trips per
    // atom: {type_i, x_i, the row's first 128 neighbour ids; the NEXT atom's ilist, first} -> {x_j, type_j}: every load
    // of a stage is requested before the first wait, and before the type check branches.
    const int i = nx_i, jbeg = nx_b, jnum = nx_n;
    {
      const int iin = min(ii + ii_step, ii_end - 1);   // (the last atom asks for its own row again: no branch)
      hd_i = kp->ilist[iin];
      hd_b = kp->first[iin];
      hd_e = kp->first[iin + 1];
    }
    int jpre[2] = {0, 0};   // neighbour ids of the first chunk
    if (jnum > 0) {         // (uniform)
#pragma unroll
      for (int u = 0; u < 2; u++) jpre[u] = kp->neigh[jbeg + min(64 * u + lane, jnum - 1)];
    }
    const int itype_raw = kp->type[i];
    const double *xi_p = kp->x + 3 * (size_t) i;   // (i in SGPRs: scalar arithmetic)
    const double x0_raw = xi_p[0], x1_raw = xi_p[1], x2_raw = xi_p[2];
    asm volatile("" : "+v"(jpre[0]), "+v"(jpre[1]));   // (pins the first use of the ids behind the requests above)
    const int itype = __builtin_amdgcn_readfirstlane(itype_raw) - 1;
    const double xi0 = uniform_f64(x0_raw), xi1 = uniform_f64(x1_raw), xi2 = uniform_f64(x2_raw);
    nx_i = __builtin_amdgcn_readfirstlane(hd_i);   // (requested ahead of the loads above: here by now)
    nx_b = __builtin_amdgcn_readfirstlane(hd_b);
    nx_n = __builtin_amdgcn_readfirstlane(hd_e) - nx_b;
    if (itype < 0 || itype >= SHF(Sp)) {   // pair_mtp.cpp:91-93
      if (lane == 0) atomicExch(kp->err_flag, 1);
      continue;
    }

    STAMP(0);   // loop head: ilist/type/x/first loads issue
    // ---- 1. compaction (the first NT survivors go straight into the tile arrays) --------
    int cnt = 0;
    const int cj_last = kp->cj_cap - 1;
    for (int c0 = 0; c0 < jnum; c0 += 128) {
      // two list entries per lane; the loads of both are in flight together (clamped indices, no branches)
      int j2[2], jt2[2];
      double d2[2][3];
      bool ok2[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int jj = c0 + 64 * u + lane;
        ok2[u] = jj < jnum;
        j2[u] = (c0 == 0 ? jpre[u] : kp->neigh[jbeg + min(jj, jnum - 1)]) & MTP_NEIGHMASK;   // (uniform select)
      }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        jt2[u] = kp->type[j2[u]] - 1;
        const double *xj = row3(kp->x, j2[u]);
        d2[u][0] = xj[0];
        d2[u][1] = xj[1];
        d2[u][2] = xj[2];
      }
      // (no branch on the loaded values ahead of the arithmetic: the compiler otherwise sinks the position loads of the
      // first entry behind its type check -- one more dependent memory round trip per atom)
      bool bad = false;
#pragma unroll
      for (int u = 0; u < 2; u++) bad = bad || (ok2[u] && (jt2[u] < 0 || jt2[u] >= SHF(Sp)));
      if (__ballot(bad) != 0ull) {   // pair_mtp.cpp:116-118 (uniform, never taken with a valid type array)
        if (bad) atomicExch(kp->err_flag, 1);
      }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (u == 1 && c0 + 64 >= jnum) break;   // uniform
        const int j = j2[u], jt = jt2[u];
        const double dx = d2[u][0] - xi0, dy = d2[u][1] - xi1, dz = d2[u][2] - xi2;
        const double r2 = dx * dx + dy * dy + dz * dz;
        const bool in = ok2[u] && jt >= 0 && jt < SHF(Sp) && !(r2 > kp->cutsq);   // pair_mtp.cpp:123
        const unsigned long long m = __ballot(in);
        if (in) {
          const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
          w.cj[min(pos, cj_last)] = j;   // a list longer than the declared max_numneigh is reported below
          if (pos < NT) {
            double r, inv;
            sqrt_and_inverse(r2, r, inv);
            w.nbx[pos] = dx;
            w.nby[pos] = dy;
            w.nbz[pos] = dz;
            w.nbr[pos] = r;
            w.nbi[pos] = inv;
            w.nbj[pos] = j;
            w.nbjt[pos] = jt;
          }
        }
        cnt += __builtin_amdgcn_readfirstlane(__popcll(m));
      }
    }
    if (cnt > kp->cj_cap) {   // the caller's max_numneigh sized the id array: refuse instead of overrunning LDS
      if (lane == 0) atomicExch(kp->err_flag, 2);
      cnt = kp->cj_cap;
    }
    if constexpr (CNT_SGPR) cnt = __builtin_amdgcn_readfirstlane(cnt);   // (cnt_sgpr_ct: the merge above left it in a VGPR)
    {   // dummy neighbours pad tile 0 to a multiple of NG
      const int pos = cnt + lane;
      if (cnt < NT && lane < NG && pos < ((min(cnt, NT) + NG - 1) / NG) * NG) {
        w.nbx[pos] = 0.0;
        w.nby[pos] = 0.0;
        w.nbz[pos] = 0.0;
        w.nbr[pos] = kp->rmax;
        w.nbi[pos] = kp->inv_rmax;
        w.nbj[pos] = i;
        w.nbjt[pos] = itype;
      }
    }
    wave_fence();

    STAMP(1);   // compaction
    phase_prio<PHASE_PRIO, MTP_PRIO_BURST>();   // tile tables and basic moments: bursts
    // ---- 2+3. tiles: tables, then basic moments in registers ------------------------------
    double acc[NB][NACC];
#pragma unroll
    for (int t = 0; t < NB; t++)
#pragma unroll
      for (int e = 0; e < NACC; e++) acc[t][e] = 0.0;
    if constexpr (FWD5) {
      block5_addresses();
    } else if constexpr (BLOCK_REGS) {
      block_offsets_to_addresses();
    } else if constexpr (WPS == 3) {
      int kl_o = kl;
      asm volatile("" : "+v"(kl_o));   // opaque per atom: keeps the address arithmetic inside the loop
      block_addresses(kl_o);
    }
    const int ntiles = (cnt + NT - 1) / NT;
    const bool nodg = NODG_CT || (SHF(dg_mode) & 1) != 0, rebuild = (SHF(dg_mode) & 2) != 0;
    double park[MTP_PARK] = {0.0, 0.0};   // nodg layouts: f'_mu(r) of this lane's neighbour, mu = half, half + 2
    for (int tile = 0; tile < ntiles; tile++) {
      const int t0 = tile * NT, nt = min(NT, cnt - t0), ntp = ((nt + NG - 1) / NG) * NG;
      build_tile<PITCH, SH>(kp, bt, w, t0, cnt, ntp, tile > 0, true, !nodg && !rebuild, nodg, park, xi0, xi1, xi2, i, itype, lane);
      STAMP(2);   // tile tables
#pragma unroll
      for (int m = 0; m < NPG; m++) {
        if (m * NG < ntp) {
          // the 12 reads of a block issue back to back (one LDS latency), then 6 products and 9 FMAs; the barriers
          // keep the scheduler from either splitting the burst or hoisting every column's reads (register blow-up)
          if constexpr (FWD5) {
            // five-factor block: ten reads, five factor values, the third factor's two partners by the block's shape,
            // six FMAs.  A product is (row x row) x (row x row) with both inner products rounded first, as in the
            // 3 x 3 pass (and fma(u, v, c) = fma(v, u, c)): the basics keep their bits
            double Ra[5], Rb[5];
#pragma unroll
            for (int f = 0; f < 5; f++) {
              Ra[f] = lds_ld(fa[f], m * NG);
              Rb[f] = lds_ld(fb[f], m * NG);
            }
            __builtin_amdgcn_sched_barrier(0);
            double F[5];
#pragma unroll
            for (int f = 0; f < 5; f++) F[f] = Ra[f] * Rb[f];
            const double p4 = select_f64(shape5, F[0], F[3]), p5 = select_f64(shape5, F[1], F[4]);
            acc[0][0] = fma(F[0], F[3], acc[0][0]);
            acc[0][1] = fma(F[0], F[4], acc[0][1]);
            acc[0][2] = fma(F[1], F[3], acc[0][2]);
            acc[0][3] = fma(F[1], F[4], acc[0][3]);
            acc[0][4] = fma(F[2], p4, acc[0][4]);
            acc[0][5] = fma(F[2], p5, acc[0][5]);
            __builtin_amdgcn_sched_barrier(0);
          } else {
#pragma unroll
          for (int t = 0; t < NB; t++) {
            double G[3], X[3], Y[3], Z[3];
#pragma unroll
            for (int h = 0; h < 3; h++) {
              G[h] = lds_ld(hg[t][h], m * NG);
              X[h] = lds_ld(hx[t][h], m * NG);
              Y[h] = lds_ld(ty[t][h], m * NG);
              Z[h] = lds_ld(tz[t][h], m * NG);
            }
            __builtin_amdgcn_sched_barrier(0);
            double hd[3], tl[3];
#pragma unroll
            for (int h = 0; h < 3; h++) {
              hd[h] = G[h] * X[h];
              tl[h] = Y[h] * Z[h];
            }
#pragma unroll
            for (int h = 0; h < 3; h++)
#pragma unroll
              for (int u = 0; u < 3; u++) acc[t][3 * h + u] = fma(hd[h], tl[u], acc[t][3 * h + u]);
            __builtin_amdgcn_sched_barrier(0);
          }
          }
        }
      }
      if (ntiles > 1) wave_fence();
    }
    STAMP(3);   // basic moments
    phase_prio<PHASE_PRIO, MTP_PRIO_CHAIN>();   // product passes, leaf sweep, energy: a few instructions between LDS round trips
    // sum over the neighbour groups, then moments + adjoints into LDS
    if constexpr (SUM_T) {   // total e in half 0, total e + 3 in half 1
#pragma unroll
      for (int e = 0; e < 3; e++) acc[0][e] = pair_sum32_t(acc[0][e], acc[0][e + 3]);
    } else {
#pragma unroll
    for (int t = 0; t < NB; t++)
#pragma unroll
      for (int e = 0; e < NACC; e++) {
        if (NG >= 4) acc[t][e] = pair_sum16(acc[t][e]);   // KL = 16: groups differ in lane bits 4 and 5
        if (NG >= 2) acc[t][e] = pair_sum32(acc[t][e]);
      }
    }
    for (int m = SHF(B) + lane; m < SHF(Am); m += 64) w.M[m] = 0.0;
    for (int m = lane; m < SHF(Ad); m += 64) w.D[m] = 0.0;
    // adjoint seeds (atom-invariant) behind the zeros, in the same program order: the leaf sweep adds onto them
    store_seeds();
    // the first 64 energy-table entries, requested ahead of the product passes: the energy then costs one LDS round trip
    int emap0 = 0;
    double elin0 = 0.0;
    if (lane < SHF(Se)) {
      if (SHF(scalars_in_lds)) {
        emap0 = bt.map[lane];
        elin0 = bt.lin[lane];
      } else {
        emap0 = kp->g_map[lane];
        elin0 = kp->g_lin[lane];
      }
    }
    if constexpr (SUM_T) {
      if (bval[0]) {
        // the lane's three int16 basic indices, products 3 q + 0..2 (-1: no such basic), from the registers
#pragma unroll
        for (int e = 0; e < 3; e++) {
          asm volatile("" : "+v"(kk5[e >> 1]));   // (opaque per atom: the unpacked indices are not kept across the loop)
          const int k = (int) (short) (kk5[e >> 1] >> (16 * (e & 1)));
          if (k >= 0) w.M[k] = acc[0][e];
        }
      }
    } else if constexpr (FWD5) {
      if (q == 0 && bval[0]) {
        // the block's six int16 basic indices in product order (-1: no such basic), from the registers
#pragma unroll
        for (int e = 0; e < 6; e++) {
          asm volatile("" : "+v"(kk5[e >> 1]));   // (opaque per atom: the unpacked indices are not kept across the loop)
          const int k = (int) (short) (kk5[e >> 1] >> (16 * (e & 1)));
          if (k >= 0) w.M[k] = acc[0][e];
        }
      }
    } else if (q == 0) {
#pragma unroll
      for (int t = 0; t < NB; t++)
        if (bval[t]) {
          // nine int16 basic indices of the block (-1: no such basic), 20 bytes after the three descriptor words
          const short *kk = reinterpret_cast<const short *>(bt.fwd + 8 * (kl + KL * t) + 3);
#pragma unroll
          for (int e = 0; e < 9; e++) {
            const int k = kk[e];
            if (k >= 0) w.M[k] = acc[t][e];
          }
        }
    }
    wave_fence();

    // ---- 4a. products, level by level (pair_mtp.cpp:196-201) -----------------------------
    if constexpr (GATHER) {
      gather_pass(kp->prog_fwd, bt.seg_fwd, SHF(nlevels), w.M, w.M, w.M, lane);
    } else {
      if constexpr (ROW_REGS) forward_levels_kept<MTP_PU, SH, 0, KEEP_L1>(bt.rows, krow, krow1, w.M, lane);
      else if (rows_lds) products_forward<MTP_PU, SH>(kp, bt.rows, bt.level, w.M, lane);
      else products_forward<MTP_PU, SH>(kp, kp->rows, bt.level, w.M, lane);
    }
    // ---- site energy (pair_mtp.cpp:204-212): the leaf rows' share first ------------------------------------
    double e = 0.0;
    // (two code paths per table home, LDS blob or HBM/L2: no pointer selects between address spaces, see below)
    // (bounds from the blob's level table or the shape's constants: level_row, mtp_wave_body.hpp)
    const int leaf_beg = level_row<SH>(bt.level, SHF(nlevels));
    const int leaf_nit = (level_row<SH>(bt.level, SHF(nlevels) + 1) - leaf_beg) >> 6;
    if (rows_lds) e = leaf_forward<MTP_PU, GRADE, false>(bt.rows, bt.leaf_cf, bt.leaf_cb, leaf_beg, leaf_nit, w.M, w.D, lane);
    else e = leaf_forward<MTP_PU, GRADE, true>(kp->rows, kp->leaf_cf, kp->leaf_cb, leaf_beg, leaf_nit, w.M, w.D, lane);
    STAMP(4);   // products forward
    // ---- candidate vector, species and linear blocks (pair_mtp_extrapolation.cpp:235-252) ----
    if (GRADE) {
      double *crow = kp->cvec + (size_t) ii * kp->cpad + SHF(Sp) * SHF(Sp) * SHF(Mu) * SHF(R);
      for (int k = lane; k < SHF(Sp); k += 64) crow[k] = k == itype ? 1.0 : 0.0;
      for (int k = lane; k < SHF(S); k += 64) crow[SHF(Sp) + k] = w.M[kp->g_map_all[k]];
    }
    if (lane < SHF(Se)) e += elin0 * w.M[emap0];
    if (SHF(scalars_in_lds))
      for (int k = lane + 64; k < SHF(Se); k += 64) e += bt.lin[k] * w.M[bt.map[k]];
    else
      for (int k = lane + 64; k < SHF(Se); k += 64) e += kp->g_lin[k] * w.M[kp->g_map[k]];
    if (e_per_atom) {
      e = wave_sum(e) + kp->species_coeffs[itype];
      if (lane == 9) {   // (lane 9 carries the energy tally; nothing of e stays live into the force phase)
        if ((kp->eflag & 2) && kp->eatom) kp->eatom[i] = e;
        if (kp->eflag & 1) tally += e;
      }
    } else {
      eacc += e + (lane == 0 ? kp->species_coeffs[itype] : 0.0);
    }
    // ---- 4b. adjoints (pair_mtp.cpp:217-233) ----------------------------------------------
    STAMP(5);   // energy
    if constexpr (GATHER) {
      gather_pass(kp->prog_bwd, bt.seg_bwd, SHF(nlevels), w.D, w.M, w.D, lane);
    } else {
      if constexpr (ROW_REGS) backward_levels_kept<MTP_PU, SH, 0, KEEP_L1>(bt.rows, krow, krow1, w.M, w.D, lane);
      else if (rows_lds) products_backward<MTP_PU, SH>(kp, bt.rows, bt.level, w.M, w.D, lane);
      else products_backward<MTP_PU, SH>(kp, kp->rows, bt.level, w.M, w.D, lane);
    }

    STAMP(6);   // products backward
    phase_prio<PHASE_PRIO, MTP_PRIO_BURST>();   // coefficient blocks and forces: bursts
    // ---- 5. forces ---------------------------------------------------------------------------
    // the (now free) moment region receives the coefficient blocks of the derivative polynomials:
    // basic k = (slot s; a, b, c) puts a D_k at the d/dx coefficient of x^(a-1) y^b z^c, b D_k and c D_k alike
    if (!SHF(coef_dense)) {   // monomials the potential does not list
      for (int k = lane; k < SHF(coef_total); k += 64) w.coef[k] = 0.0;
      wave_fence();
    }
    for (int k0 = 0; k0 < (GRADE && kp->dbasic ? max(kp->dpad, SHF(B)) : SHF(B)); k0 += 192) {
      constexpr int ROUNDS = 3;   // 192 basics per trip: all reads first, one LDS round trip
      double dd[ROUNDS];
      int2 tg[ROUNDS];
      if (SHF(tgt_in_lds)) {   // (uniform; two loops, not a pointer select between address spaces)
#pragma unroll
        for (int u = 0; u < ROUNDS; u++) tg[u] = reinterpret_cast<const int2 *>(bt.coef)[min(k0 + lane + 64 * u, SHF(B) - 1)];
      } else {
#pragma unroll
        for (int u = 0; u < ROUNDS; u++) tg[u] = reinterpret_cast<const int2 *>(kp->g_tgt)[min(k0 + lane + 64 * u, SHF(B) - 1)];
      }
#pragma unroll
      for (int u = 0; u < ROUNDS; u++) dd[u] = w.D[min(k0 + lane + 64 * u, SHF(B) - 1)];
#pragma unroll
      for (int u = 0; u < ROUNDS; u++) {
        const int k = k0 + lane + 64 * u;
        const bool ok = k < SHF(B);
        if (GRADE && kp->dbasic && k < kp->dpad) kp->dbasic[(size_t) ii * kp->dpad + k] = ok ? dd[u] : 0.0;   // read back by mtp_cvec_kernel
        if (ok) {
          const unsigned t0 = (unsigned) tg[u].x, t1 = (unsigned) tg[u].y;
          const unsigned tx = t0 & 0xffffu, ty_ = t0 >> 16, tz_ = t1 & 0xffffu;
          if (tx != 0xffffu) w.coef[tx] = dd[u] * (double) ((t1 >> 16) & 15u);
          if (ty_ != 0xffffu) w.coef[ty_] = dd[u] * (double) ((t1 >> 20) & 15u);
          if (tz_ != 0xffffu) w.coef[tz_] = dd[u] * (double) ((t1 >> 24) & 15u);
        }
      }
    }
    wave_fence();
    STAMP(9);   // coefficient blocks
    {
      const int n = lane & 31, part = lane >> 5;
      unsigned pcol = w.addr(w.tab + n);
      asm volatile("" : "+v"(pcol));
      double crad = 0.0;
      for (int tile = 0; tile < ntiles; tile++) {
        const int t0 = tile * NT, nt = min(NT, cnt - t0), ntp = ((nt + NG - 1) / NG) * NG;
        if (ntiles > 1 || rebuild)   // (single-tile atoms in the persistent layouts: the g rows and park[] of the tile build stand)
          build_tile<PITCH, SH>(kp, bt, w, t0, cnt, ntp, ntiles > 1, false, !nodg, nodg, park, xi0, xi1, xi2, i, itype, lane);
        // f' of the tile: the Mu rows behind the coefficient blocks, or all four in registers of both halves (fp_regs_ct)
        double Fp[MTP_FP_N] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (FP_REGS) fp_exchange(park, Fp);
        else if (nodg) fp_from_parked<PITCH, SH>(kp, w, ntp, park, lane);
        // columns past ntp hold stale (finite or not) data: their lanes are masked at the end
        const double x = w.nbx[n], y = w.nby[n], z = w.nbz[n], inv = w.nbi[n];
        double UA = 0.0, VA = 0.0, UB = 0.0, VB = 0.0, S0 = 0.0;
        double Wm[4] = {0.0, 0.0, 0.0, 0.0};
        const bool fused = GRADE && kp->grade_fused;
        const unsigned pcoef = w.addr(w.coef), pcoef_l = pcoef + 8u * (unsigned) (lane & 15);
        {   // rank 0: P_s = D_k, no gradient; dg_s = f'_mu (nodg: its row fp_row + mu; else the slot's dg row)
          const unsigned cg0 = pcol + 8u * (unsigned) (nodg ? SHF(fp_row) * PITCH : SHF(dg_off));
          const int n0 = SHA(deg_first, 1);
          // four slots per per-lane read: lane i of each row holds D_{s4 + i} (poly_eval_dpp)
          for (int s4 = 0; s4 < n0; s4 += 4) {
            const double c = lds_ld(pcoef_l + 8u * (unsigned) (SHA(deg_coef, 0) + s4), 0);
            auto term = [&](auto I) {
              constexpr int i = decltype(I)::value;
              const int sidx = s4 + i;
              if (i == 0 || sidx < n0) {   // (uniform)
                const int mu = nodg ? smu.template uniform<true, GRADE>(sidx) : smu.template uniform<false, GRADE>(sidx);
                if constexpr (FP_REGS) fmac_row_bcast1<i>(S0, c, fp_pick(Fp, slot_mu_of<SH>(sidx)));
                else fmac_row_bcast1<i>(S0, c, lds_ld(cg0 + 8u * (unsigned) ((nodg ? mu : sidx) * PITCH), 0));
                if (GRADE) {
                  const double dk = row_bcast<i>(c);
#pragma unroll
                  for (int v = 0; v < 4; v++) Wm[v] += (mu == v && part == 0) ? dk : 0.0;
                }
              }
            };
            term(std::integral_constant<int, 0>());
            term(std::integral_constant<int, 1>());
            term(std::integral_constant<int, 2>());
            term(std::integral_constant<int, 3>());
          }
        }
        double mono[DEG * (DEG + 1) / 2];
        mono[0] = 1.0;
        if (nodg) {
          force_degree<1, DEG, PITCH, GRADE, true, SH, SlotMu<MU_PACKED>, FP_REGS>(kp, pcol, pcoef, pcoef_l, part, x, y, z, mono, UA, VA, UB, VB, smu, inv, inv, Wm, Fp);
          // dg_s / nu = f'_mu r^-nu / nu - g_s / r: the second term of every slot at once
          VA = fma(-inv, UA, VA);
          VB = fma(-inv, UB, VB);
        } else if constexpr (!NODG_CT) {
          force_degree<1, DEG, PITCH, GRADE, false, SH>(kp, pcol, pcoef, pcoef_l, part, x, y, z, mono, UA, VA, UB, VB, smu, inv, inv, Wm, Fp);
        }
        if (fused) {
          // c[jt][mu][ri] += sum_n [type_n = jt] Q_ri(r_n) W_mu(n)  (pair_mtp_extrapolation.cpp:193-198, 323-329):
          // half h of the wavefront reduces the 32 (mu, ri) entries of jt = h over its 32 neighbour lanes
          double qv[8];
          {
            const double r = w.nbr[n], d = r - kp->rmax;
            const double ksi = (2.0 * r - (kp->rmin + kp->rmax)) * kp->inv_span;
            qv[0] = kp->scaling * (d * d);
            qv[1] = kp->scaling * (ksi * d * d);
#pragma unroll
            for (int ri = 2; ri < 8; ri++) qv[ri] = 2.0 * ksi * qv[ri - 1] - qv[ri - 2];
          }
          const bool mine = n < nt && w.nbjt[n] == part;
          double ent[32];
#pragma unroll
          for (int v = 0; v < 4; v++) {
            const double wt = pair_sum32(Wm[v]);   // every lane takes part in the exchange; masked afterwards
#pragma unroll
            for (int ri = 0; ri < 8; ri++) ent[8 * v + ri] = mine ? qv[ri] * wt : 0.0;
          }
          Butterfly<32>::run(ent, lane);
          crad += ent[0];   // lane (h, e): entry e = mu R + ri of block jt = h
        }
        // sum_s dg_s P_s = r . sum_s (dg_s / nu) grad P_s  (+ rank 0), shared by both halves
        // (the contraction is spelled out: left to the compiler, a * b + c * d fused one product in the generic kernels and
        // the other in the fixed-shape ones, and the forces differed in the last bit)
        double S = fma(y, VB, (part ? z : x) * VA) + (part ? 0.0 : S0);
        S = pair_sum32(S);
        UB = pair_sum32(UB);
        const double sr = S * inv;
        const bool valid = n < nt;
        const double Fa = valid ? fma(sr, part ? z : x, UA) : 0.0;   // half 0: F_x, half 1: F_z
        const double Fy = valid && part == 0 ? fma(sr, y, UB) : 0.0;
        const double Fx = part ? 0.0 : Fa, Fz = part ? Fa : 0.0;
        if (valid) {
          const size_t j = (size_t) w.nbj[n];
          unsigned j2 = (unsigned) j << 1;
          asm volatile("" : "+v"(j2));
          const size_t j3 = (size_t) (j2 + (unsigned) j);   // 3 j without a quarter-rate multiply
          force_add(kp, j3 + (part ? 2 : 0), -Fa);   // pair_mtp.cpp:252-254
          if (part == 0) force_add(kp, j3 + 1, -Fy);
        }
        // ---- totals of this tile over the 64 lanes: force on i (3), virial (6); lane v < 9 ends up with value v.
        // Per tile, not per atom: nine running sums carried across the tile loop would be live through the whole
        // force phase (18 VGPRs the 168-VGPR build does not have); atoms with more than 32 neighbours pay one more
        // reduction per extra tile.
        double v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0;
        if (kp->vflag && valid) {   // pair_mtp.cpp:257-277 (linear in F: each half tallies its components)
          v0 = -Fx * x;
          v1 = -Fy * y;
          v2 = -Fz * z;
          v3 = -(Fx * y + Fy * x) * 0.5;
          v4 = -(Fx * z + Fz * x) * 0.5;
          v5 = -(Fy * z + Fz * y) * 0.5;
        }
        double tot;
        if (kp->vflag && !v_per_atom) {
          vacc[0] += v0;
          vacc[1] += v1;
          vacc[2] += v2;
          vacc[3] += v3;
          vacc[4] += v4;
          vacc[5] += v5;
        }
        if (v_per_atom) {
          double part9[9] = {Fx, Fy, Fz, v0, v1, v2, v3, v4, v5};
          butterfly9(part9, lane);
          tot = part9[0];
        } else {
          // the mirror partners flip the low lane bits too, so they go first (while every lane still holds
          // all entries); the quad butterfly then leaves entry (lane & 3) summed over the row
          double part4[4] = {Fx, Fy, Fz, 0.0};
#pragma unroll
          for (int u = 0; u < 3; u++) {
            part4[u] += partner_f64<8>(part4[u]);
            part4[u] += partner_f64<4>(part4[u]);
          }
          Butterfly<4>::run(part4, lane);
          tot = part4[0];
        }
        tot = pair_sum32(pair_sum16(tot));
        if (lane < 9) {
          if (lane < 3) {
            force_add(kp, 3 * (size_t) i + lane, tot);   // pair_mtp.cpp:248-250
          } else if (v_per_atom) {
            tally += tot;
            if ((kp->vflag & 4) && kp->vatom) kp->vatom[6 * (size_t) i + (lane - 3)] += tot;
          }
        }
        if (ntiles > 1) wave_fence();
      }
      if (GRADE && kp->grade_fused) {   // radial block of the row: block (itype, jt), zeros elsewhere
        const int MuR = SHF(Mu) * 8, SMR = SHF(Sp) * MuR;
        double *crow = kp->cvec + (size_t) ii * kp->cpad;
        for (int e = lane; e < SHF(Sp) * SMR; e += 64)
          if (e / SMR != itype) crow[e] = 0.0;
        if (part < SHF(Sp) && n < MuR) crow[(itype * SHF(Sp) + part) * MuR + n] = crad;
      }
    }
    STAMP(7);   // forces
    wave_fence();
    STAMP(8);   // per-atom totals
#ifdef MTP_STAMPS
    st_atom++;
#endif
  }
  phase_prio<PHASE_PRIO, MTP_PRIO_BURST>();
#ifdef MTP_STAMPS
  if (lane == 0 && kp->stamps)
    for (int k = 0; k < 10; k++) atomicAdd(kp->stamps + k, st_acc[k]);
  if (lane == 0 && kp->stamps) {
    atomicAdd(kp->stamps + 10, st_prologue);
    atomicAdd(kp->stamps + 11, __builtin_amdgcn_s_memtime() - st_entry);   // the wavefront's life up to here
    atomicAdd(kp->stamps + 12, 1ull);                                        // wavefronts
  }
#endif
  if (kp->vflag && !v_per_atom) {   // the deferred virial: one transpose-reduce for all atoms of the wavefront
    double part16[16] = {0.0, 0.0, 0.0, vacc[0], vacc[1], vacc[2], vacc[3], vacc[4], vacc[5], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    Butterfly<16>::run(part16, lane);
    const double tot = pair_sum32(pair_sum16(part16[0]));
    if (lane >= 3 && lane < 9) tally += tot;
  }
  if ((kp->eflag & 1) && !e_per_atom) {
    const double et = wave_sum(eacc);
    if (lane == 9) tally += et;
  }
  if (lane >= 3 && lane <= 9 && tally != 0.0) {
    // quantity-major slots [8][MTP_EV_SLOTS]: the fold reads each quantity's slots as one contiguous run
    double *slot = kp->ev_slots + (size_t) ((blockIdx.x * wpb + wave) % MTP_EV_SLOTS);
    unsafeAtomicAdd(&slot[(size_t) (lane == 9 ? 0 : lane - 2) * MTP_EV_SLOTS], tally);
  }
