  // The body of an interpreter block (engine.hip: k_run, k_run_batch).  The including kernel
  // provides KArgs k, the names VF, MODE, TIER and KG, and the macros MG_VB (the block's id within
  // its launch) and MG_VGRID (that launch's grid size).  k_run_seeded also defines MG_SEEDED and
  // provides SeedArgs sd (MODE_SEEDED, KG = 1).  k_run_scored defines both MG_SEEDED and MG_SCORED
  // and also provides ScoreArgs sc (MODE_SCORED, KG = 1).
  VF vf0(mg_lds, k, MG_VB);
  // the generator constants into LDS behind the value file (one wave per block: its own later
  // reads see the writes, LDS runs a wave's operations in order)
  if (MODE != MODE_EVAL && k.lds_g != kNoLds)
    for (uint32_t i = threadIdx.x; i < k.n_gconsts; i += kWave) mg_lds[k.lds_g + i] = cst(k.gconsts)[i];
  // EVAL sweeps rows [0, count); GEN / SEARCH sweep the aligned 64-index groups that
  // cover [start, start + count), one group per wave (the GEN3 group key is per wave)
  const uint64_t a0 = (MODE == MODE_EVAL) ? 0ull : (k.start & ~63ull);
  const uint64_t end = k.start + k.count;
  const uint64_t total = (MODE == MODE_EVAL) ? k.count : (end - a0);
  // KG groups per wave per pass (run_program): a wave's pass covers KG * 64 consecutive indices
  const uint64_t step = (uint64_t)MG_VGRID * kWave * KG;
  const bool early = (MODE == MODE_SEARCH || MODE == MODE_SEEDED || MODE == MODE_SCORED) && (k.flags & MG_SEARCH_EARLY_EXIT);
  uint64_t wave_best = ~0ull, wave_hits = 0;  // wave-uniform; published once per wave
  // idx & 63 == threadIdx.x & 63 below (a0 and base are multiples of 64): the lane half of
  // the GEN3 lane key is fixed per thread
  const uint64_t lk = (MODE == MODE_EVAL) ? 0ull : gen_lane_key(threadIdx.x & 63u, k.sk);
  // Warm the scalar cache with the program and the generator specs, 64-byte lines eight loads at a
  // time: a wave reads them with dependent scalar loads, one instruction (32 B) or spec ahead, so a
  // cold cache costs it an L2 round trip every other instruction — the floor of an easy query's time
  // to first model, which one wave's pass over the program is.
  if (k.flags & kFlagPrefetch) {
    uint32_t acc = 0;
    auto warm = [&acc](const uint32_t* base, uint32_t lines) {
      const auto* b = cst(base);
      for (uint32_t l = 0; l < lines; l += 8) {
        uint32_t x[8];
#pragma unroll
        for (int q = 0; q < 8; q++) x[q] = (l + q < lines) ? b[16u * (l + q)] : 0u;
#pragma unroll
        for (int q = 0; q < 8; q++) acc ^= x[q];
      }
    };
    warm((const uint32_t*)k.code, min((k.n_instr + 2u) / 2u, 512u));
    if (MODE != MODE_EVAL && k.specs) warm((const uint32_t*)k.specs, min((k.n_specs + 1u) / 2u, 512u));
    if (acc == 0x5EED1E55u && k.count == ~0ull) k.hits[0] = acc;  // never true: keeps the loads
  }
  // the hoisted literals: their slots are never reused, so once per thread is enough
  for (uint32_t pc = 0; pc < k.pc0; pc++) {
    const Instr in = ld_instr(k, pc);
    const uint32_t L = (in.wd + 31) >> 5;
    const auto* c = cst(k.consts) + in.p0;
    MG_FOR_G(MG_LIMBS(L, vf.at(in.dst + j) = c[j];););
  }
#ifdef MG_SCORED
  // the sweep walks the window like every other mode; the model launch (sc.fetch) runs one group,
  // that of slot MG_VB's winner, with only the winner's lane active
  uint64_t base0 = (uint64_t)MG_VB * kWave, win = ~0ull;
  if (sc.fetch) {
    const unsigned long long w = sc.slots[(uint64_t)MG_VB * kSlotStride];
    win = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(w >> 32)) << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)w);
    if (win == ~0ull) return;  // an empty slot: its row stays as the caller left it
    win = k.start + (win & kSlotIndexMask);
    base0 = (win & ~63ull) - a0;
  }
  for (uint64_t base = base0; base < total; base += step) {
#else
  for (uint64_t base = (uint64_t)MG_VB * kWave * KG; base < total; base += step) {
#endif
    bool active[KG];
    uint64_t i[KG];
    GKeys key[KG];
#pragma unroll
    for (int g = 0; g < KG; g++) {
      const uint64_t off = base + (uint64_t)g * kWave + threadIdx.x;
      const uint64_t idx = a0 + off;  // candidate index (GEN / SEARCH)
      active[g] = (MODE == MODE_EVAL) ? off < total : (idx >= k.start && idx < end);
      // EVAL: SoA row; GEN: output row (only written by active lanes)
      i[g] = (MODE == MODE_EVAL) ? (active[g] ? off : total - 1) : (idx - k.start);
#ifdef MG_SCORED
      if (sc.fetch) active[g] = idx == win;
#endif
    }
    uint64_t cur_u = ~0ull;  // the hit word as this group starts (early exit only)
    if (early) {
      // every candidate below the current first hit is still evaluated, so the
      // final minimum is exact; waves entirely above it stop
      const unsigned long long cur = read_first_hit(k.first_hit, k.flags);
      // readfirstlane returns int: widen through uint32_t, or a low word with bit 31 set would
      // sign-extend over the high word
      cur_u = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(cur >> 32)) << 32) |
              (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)cur);
      if (a0 + base >= cur_u) break;
    }
    // each group's key from its base (a0 + base + 64 g, a multiple of 64: idx >> 6 is the same for
    // every lane), so the compiler sees G as wave-uniform: the MIXED alternatives are scalar branches
    // and the generator specs scalar loads (from idx, G looked per-lane: divergent branches, vector loads)
#pragma unroll
    for (int g = 0; g < KG; g++) key[g] = MODE != MODE_EVAL ? gen_keys_lk(a0 + base + (uint64_t)g * kWave, lk, k.sg) : GKeys{};
    uint32_t v[KG];
#ifdef MG_SEEDED
    // group number n of the seeded index space: seed n mod n_seeds, round n / n_seeds (wave-uniform,
    // like every per-group choice of GEN3); KG = 1
    SeedGroup sgrp[1];
    {
      const uint64_t n = (a0 + base) >> 6;
      const uint32_t ns = sd.n_seeds ? sd.n_seeds : 1u;
      sgrp[0].s = sd;
      sgrp[0].m = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(n % ns));
      sgrp[0].replay = n < ns;
    }
#ifdef MG_SCORED
    uint32_t viol[1];
    run_program<VF, MODE, TIER, KG>(k, vf0, i, key, early, active, v, MG_VB, sgrp, viol);
    if (sc.fetch) return;  // the winner's rows are stored (K_WATCH); nothing to reduce
    {
      // the group's best candidate: the minimum of viol << 6 | lane over the active lanes (lowest
      // violations, then lowest index), six cross-lane steps
      uint32_t best = active[0] ? (viol[0] << 6) | (threadIdx.x & 63u) : ~0u;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o));
      if (threadIdx.x == 0 && best != ~0u) {
        const unsigned long long w =
            ((unsigned long long)(best >> 6) << 48) | ((a0 + base + (uint64_t)(best & 63u)) - k.start);
        unsigned long long* sw = sc.slots + (((a0 + base) >> 6) & (MG_SCORED_SLOTS - 1u)) * kSlotStride;
        // read first, atomicMin only when lower (as the first-hit word)
        if (w < __hip_atomic_load(sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(sw, w);
      }
    }
#else
    run_program<VF, MODE, TIER, KG>(k, vf0, i, key, early, active, v, MG_VB, sgrp);
#endif
#else
    run_program<VF, MODE, TIER, KG>(k, vf0, i, key, early, active, v, MG_VB);
#endif
#pragma unroll
    for (int g = 0; g < KG; g++) {
      v[g] = active[g] ? v[g] : 0u;
      if (MODE == MODE_SEEDED && k.verdict && active[g]) k.verdict[i[g]] = (uint8_t)v[g];
      if (MODE == MODE_SEARCH || MODE == MODE_SEEDED || MODE == MODE_SCORED) {
        const unsigned long long m = __ballot(v[g] != 0);
        if (m) {
          const uint64_t first = a0 + base + (uint64_t)g * kWave + (uint64_t)(__ffsll((long long)m) - 1);
          wave_hits += (uint64_t)__popcll(m);
          if (first < wave_best) {
            wave_best = first;
            // (a hit at or above the word read as the group started cannot lower it: no atomic)
            if (early && threadIdx.x == 0 && first < cur_u) {
              atomicMin(k.first_hit, (unsigned long long)first);
              publish_peers(k.first_hit, (unsigned long long)first);
            }
          }
        }
      } else if (active[g]) {
        k.verdict[i[g]] = (uint8_t)v[g];
      }
    }
  }
  if ((MODE == MODE_SEARCH || MODE == MODE_SEEDED || MODE == MODE_SCORED) && threadIdx.x == 0) {
    // a first hit that cannot lower the current minimum is not published; the count goes to the
    // block's stripe (kHitStripes)
    if (wave_best != ~0ull &&
        wave_best < read_first_hit(k.first_hit, k.flags))
      atomicMin(k.first_hit, (unsigned long long)wave_best);
    if (wave_hits) atomicAdd(k.hits + kHitStride * (1u + (MG_VB % kHitStripes)) - 1u, (unsigned long long)wave_hits);
  }
