// The body of the ragged verify's vector kernel, symbols and stored chunk bytes
// alike: #include-d INSIDE the two __global__ definitions (rs_verify_ragged.hip,
// rs_bytes_ragged.hip), which differ in one kernel argument.  A shared
// __device__ function would be the plain way to write this; inlining one into
// the kernels changed the machine code of every instantiation, and these
// kernels are held to their bytes.  In scope where it is included: the
// template parameters K, W, R, UB, C, NC, DYN, PIPE, SET, the kernel
// arguments of SLIME_RVERIFY_PARAMS plus `ticket`, and a constexpr bool
// BYTES (false: `mapping` is a null constant that nothing reads).
// rs_verify_ragged.hip's header comment describes the scheme.
  static_assert(K > 0 && K <= 16 && NC > 0 && NC <= 64, "compile-time k only");
  static_assert(W >= 1 && W <= UB, "a step is at most a tile");
  static_assert(PIPE || !DYN, "the dynamic walk is double-buffered");
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  UnitWalk<C, NC, DYN> w(ticket, units, descs, nunits, lane, wave, gridDim.x * kWaves);
  Tally t(lane);
  // The walk's current object, plan and mapping: read when a step's loads are issued, never by a compare.
  const uint8_t* sb[K];
  const uint8_t* rb[R];
  const uint8_t* cb = nullptr;
  uint64_t cshard = 0, res = 0;
  PlanRows cur{coeff, out_idx, rows};
  uint32_t cur_m = 0;
  uint32_t st = 0, ns = 0, t0 = 0, tend = 0;  // the step inside the current tile, the tile's steps and vectors
  auto bases = [&]() {
    u32x16 idx;
    if constexpr (SET) {
      const PlanRef pl = ragged::load_plan(coeff, descs, w.obj);
      cur.rows = block_rows(pl.rows, r0);
      // No row in this block: the unit is passed over, and sb / rb keep the bases of the last
      // object that had loads (the prefetch past a wave's last step re-reads through them).
      if (cur.rows == 0) return;
      cur.coeff = coeff + pl.coeff_off + r0 * kCoeffStride;
      cur.oidx = coeff + pl.out_off + r0;
      idx = *reinterpret_cast<const u32x16*>(coeff + pl.in_off);  // K <= 16: one line
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) idx[j] = in_idx[j];
    }
    if constexpr (BYTES) cur_m = mapping[w.obj];  // wave-uniform: one scalar load
#pragma unroll
    for (int j = 0; j < K; ++j) sb[j] = in + ((w.d.src_off + (uint64_t)idx[j] * w.d.src_shard) << 2);
    cb = cmp + (w.d.dst_off << 2);
    cshard = w.d.dst_shard << 2;
    res = (uint64_t)w.obj * res_stride;
    row_bases<R>(rb, cb, cur.oidx, cshard, 0, cur.rows);
  };
  // After the walk moved: the new object's bases, units without a row in this block passed over,
  // and the steps of the tile the walk stands on.
  auto settle = [&]() {
    while (w.live) {
      if (w.fresh) bases();
      if (!SET || cur.rows != 0) break;
      w.advance();
    }
    if (w.live) {
      t0 = w.tile() * (64 * UB);
      tend = w.d.nvec - t0 < 64u * UB ? w.d.nvec : t0 + 64 * UB;  // the host lists tiles below nvec only
      ns = (tend - t0 + 64 * W - 1) / (64 * W);
      st = 0;
    }
  };
  auto next = [&]() {
    if (++st < ns) return;
    w.advance();
    settle();
  };
  auto here = [&]() { return StepRef{cb, cshard, mism + res, first + res, cur, cur_m, t0 + st * (64 * W), tend}; };
  auto load = [&](uint4(&x)[W][K], uint4(&s)[R][W], const StepRef& r) {
    load_tile<K, W, R, uint32_t>(x, s, sb, rb, r.tb + lane, r.v1);
  };
  // The step's OWN object, plan and mapping (r), whatever the walk has moved on to.  BYTES: check_tile
  // turns the raw inputs into symbols first and compares BE(computed ^ m) with the stored words.
  auto check = [&](uint4(&x)[W][K], uint4(&s)[R][W], const StepRef& r) {
    if (r.mism != t.mism) {
      t.flush();
      t.begin(r.mism, r.fst);
    }
    check_tile<K, W, R, BYTES, uint32_t>(t, x, s, r.cb, r.pl.coeff, r.pl.oidx, r.cshard, r.pl.rows, BYTES ? r.m : 0u,
                                         r.tb, r.v1);
  };
  settle();
  if constexpr (PIPE) {
    if (w.live) {
      uint4 xa[W][K], xb[W][K], sa[R][W], sc[R][W];
      StepRef ra = here(), rc = ra;
      load(xa, sa, ra);
      for (;;) {
        next();
        // Past the last step the prefetch re-reads the current one (unconditional loads, see load_tile).
        rc = ra;
        if (w.live) rc = here();
        load(xb, sc, rc);
        check(xa, sa, ra);
        if (!w.live) break;
        next();
        ra = rc;
        if (w.live) ra = here();
        load(xa, sa, ra);
        check(xb, sc, rc);
        if (!w.live) break;
      }
    }
  } else {
    while (w.live) {
      uint4 x[W][K], s[R][W];
      const StepRef r = here();
      load(x, s, r);
      check(x, s, r);
      next();
    }
  }
  t.flush();
  w.finish();
  verify_tails<K, SET, BYTES>(SLIME_RVERIFY_PASS);
