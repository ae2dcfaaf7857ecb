// lcp_primal_step.inc - the body-space PDIPM step kernel (see lcp_primal.hip for the derivation); included, inside
// namespace lcp::primal, by the translation units that instantiate it (lcp_primal.hip: EQC = 4; lcp_primal_chain.hip: EQC = 24).
// NCOL: capacity of the system (nz + neq <= NCOL <= 64): pivots are visited in groups of eight up to the scene's size, so a capacity
//       that is not a multiple of 8 (30: the ten free bodies of BASELINE config 5 in the pinned form) just ends its last group early
// DENSE: the same solve behind the dense LCPFunction boundary (lcp.py:22-64): the scene's (Q, p, G, h, A, b, F) is read instead of
//        a contact list - scenes lcp_classify_big marked 3: the mixed contact LCP of engines.py:50-74 with a diagonal Q whose
//        Jacobian rows touch at most two bodies -, the outputs are x, y, z, s (forward) or the seven dense gradients of
//        lcp.py:52-61 (backward).
// PIN:   the caller promised (LCP_HINT_PINNED) that the equality rows of every scene pin the leading coordinates: A = [I 0], and b = 0
//        from a contact list (engines.py:74).  Then x_p = 0 throughout (dx_p = -ry_p = -x_p), the columns of the pinned coordinates
//        only ever multiply zeros and the equality rows need no pivots: the system that is formed and factored is the
//        (nz - neq)-square S_ff = (Q + G^T M^-1 G)_ff - 30 x 30 instead of 36 x 36 on BASELINE config 5, 32 columns instead of 40.
//        The ROWS of the pinned coordinates are still formed (over the live columns): they ride along in the backward sweep and
//        leave dy_p = rhs_p - (S dx)_p on their lanes, so y lives on the pinned lanes, not on lanes nz .. nz + neq - 1.  A scene
//        that breaks the promise is not solved (NaN velocities, LCP_ST_NAN), as in lcp_quad.hip.  NCOL >= nz - neq here.
//        PIN = neq at compile time (3: one pinned body): the pivot lanes k + neq of the broadcasts must be immediates - v_readlane
//        with its lane select in a scalar register measured 40 % slower in the LU (100 k -> 141 k cycles per scene at 24 columns).
template <int NCOL, bool BWD, bool DENSE, int EQC, int PIN = 0>
__global__ void __launch_bounds__(64, (NCOL <= 24 ? 2 : (NCOL <= 40 ? LCP_PRIMAL_OCC40 : 1))) lcp_primal_kernel(StepArgs SP, StepBwdArgs Gd, DenseIO DN) {
  static_assert(!(PIN && EQC > 4), "the pinned form serves up to four equality rows");
  // row stride of the matrix image.  Entry (r, c) sits in bank pair (r LDK + c) mod 32: with LDK = -1 (mod 32) the diagonal blocks of
  // ALL bodies fall on the same few banks (c - r) and the ds_add_f64 of the formation serialise - measured at LDK = 31: formation
  // 86 k -> 156 k cycles per scene, and every other LDS phase of the CU's wavefronts behind it
  constexpr int LDK = ((NCOL + 1) % 32 == 31) ? NCOL + 3 : NCOL + 1;
  // LU layout of factor(): the lane grid in the kernels of the pinned form (round 3: backward kernels only - in the forward the first
  // grid form's longer dependent chain per pivot cost more than its instructions saved, 0.4099 -> 0.4163 ms; round 4's second form
  // - half the issue slots per pivot, the pivot's dependent chain taken off the critical path - wins there too: config 5 forward
  // 0.366 -> 0.326 ms, LU 150 k -> 125 k cycles per scene; profiles/r04_ab_config5.txt), row per lane otherwise
  constexpr bool GRID = PIN != 0 && NCOL <= 32 && (BWD ? LCP_PRIMAL_GRIDLU != 0 : LCP_PRIMAL_GRIDLU == 2);
  constexpr int NROW = NCOL + PIN;                                  // rows of the image: the pinned coordinates keep theirs
  // Triangular sweeps in BLOCK layout (round 4, behind the second form of the lane-grid LU; lcp_primal_bsweep.h): the live rows on three
  // DPP rows of BS lanes, PIN lanes behind each block for the partial sums of the pinned coordinates' rows.  The factors are read
  // from the image by the sweeps (it stays live between factor() and the solves: one more - zero - row for the lanes without a
  // row, the affine direction is parked in its own 4 KB)
  constexpr bool BSW = GRID && LCP_PRIMAL_GRIDLU_V2 != 0 && LCP_PRIMAL_BSWEEP != 0;
  constexpr int BS = (NCOL + 2) / 3;
  static_assert(!BSW || (BS + PIN <= 16 && 3 * BS <= LDK && BS <= 12), "block layout of the sweeps");
  constexpr int KROWS = NROW + (BSW ? 1 : 0);
  constexpr int KSZ = (KROWS * LDK > 11 * LX) ? KROWS * LDK : 11 * LX;    // (the dense backward stages 144 + 8 nc <= 656 doubles here; the forward parks 512)
  __shared__ __attribute__((aligned(16))) double Kl[KSZ];          // image of the system matrix (formation); backward: staging
  __shared__ double park[(BSW && !BWD) ? 8 * LX : 1];
  __shared__ double xv[LX];                                        // x-space exchange / accumulation
  constexpr int ASZ = (EQC <= 4) ? EQC * LX : at_cap(NCOL, EQC);    // the A image: rows of 64 (few rows) or packed e x nz (many rows)
  __shared__ float At[ASZ];
  __shared__ int B12[2 * LX];
  __shared__ double gx[(GRID && LCP_PRIMAL_GRIDLU_V2) ? 2 * LX : 1];   // lane-grid LU: the multipliers of a pivot, handed from the pivot column's DPP row to the others
  double* const stash = (BSW && !BWD) ? park : Kl;                 // the affine direction, parked during the corrector solve: 8 x 64 doubles
                                                                   // (row-per-lane sweeps: the image is only live inside factor(), which no solve straddles)
  const int scene = blockIdx.x, lane = threadIdx.x;
  if (!BWD && blockIdx.x == 0 && lane == 0 && SP.tag) *SP.tag = SP.tag_value;   // workspace trailer: which kernel family laid it out
  if (DENSE && DN.cls[scene] != (PIN ? 4 : 3)) return;                     // (another family / the other form serves the scene: lcp_classify_big)
  const int nb = SP.nb, nz = 3 * nb, ncap = SP.nc, e = PIN ? PIN : SP.e;
  constexpr int clo = PIN;                                                   // first live column (PIN: e == PIN, checked by the launcher)
  const int n = PIN ? nz - e : nz + e;                                       // pivots
  const int AST = (EQC <= 4) ? LX : nz;                                      // row stride of the A image
  double* Wg = (double*)SP.ws + (size_t)scene * (DENSE ? DN.ws_scene / sizeof(double) : (size_t)WsLayout::TOTAL);
  double* Wit = Wg + WsLayout::IT;
  // Round 6 (profiles/r06_ab_bwd_split.txt, item 3): what the prologue reads at addresses that depend on the lane alone is asked for HERE, without
  // lane predicates (the address is clamped, the value masked where it is used) - a load under `if (lane < ...)` is waited for at the join of
  // its branch, and the kernel used to make 17 .. 38 such round trips one after the other in front of its first multiplication
  const int lx = lane < nz ? lane : 0;                                     // (nz <= 64: an entry that exists)
  float md_l = 0.f, vv_l = 0.f, ff_l = 0.f;
  if constexpr (!DENSE) {
    md_l = ((const float*)SP.Mdiag)[(size_t)scene * nz + lx]; vv_l = ((const float*)SP.v)[(size_t)scene * nz + lx];
    ff_l = BWD ? 0.f : ((const float*)SP.f)[(size_t)scene * nz + lx];
  }
  double wx_l = 0, wz_l[4] = {1, 1, 1, 1}, ws_l[4] = {1, 1, 1, 1}, wmu_l = 0, wqd_l = 0;
  constexpr bool HOIST_IT = BWD && (!DENSE || LCP_PRIMAL_HOIST_DENSE_BWD);   // (A/B: profiles/r06_ab_dense_bwd_hoist.txt)
  if constexpr (HOIST_IT) {                                                // the iterate the forward kept (64 entries per field: any lane's slot exists)
    wx_l = Wit[lane];
    static_for<4>([&](auto Q_) LCP_INL { wz_l[Q_] = Wit[ZO + Q_ * LX + lane]; ws_l[Q_] = Wit[ZO + (4 + Q_) * LX + lane]; });
    if constexpr (DENSE) { wmu_l = Wit[ZO + 8 * LX + lane]; wqd_l = Wit[ZO + 9 * LX + lane]; }
  }
  int ncs = ncap;
  if (BWD) ncs = (int)Wg[0];                                               // the count the forward solved with
  else if (SP.c_count) ncs = SP.c_count[scene];
  const int truncated = (ncs > ncap) ? LCP_ST_TRUNCATED : 0;               // more contacts found than the list holds
  ncs = ncs < 0 ? 0 : (ncs > ncap ? ncap : ncs);
  if (!BWD && lane == 0) Wg[0] = (double)ncs;
  // contact of this lane.  Contacts of one pair of bodies sit next to each other in a list (world.py:119-142 walks the pairs) and
  // hit the same 36 entries of the matrix image: dealt round-robin to the four 16-lane rows they meet in different passes of a
  // ds_add_f64 instead of serialising in one
  const int ci = (LCP_PRIMAL_CPERM && ncap > 16) ? (4 * (lane & 15) + (lane >> 4)) : lane;    // (lists of up to 16 contacts stay in one row)
  const bool vc = ci < ncs;                                                // this lane owns a live contact
  const bool vx = lane < nz;                                               // ... an x entry,
  const bool ve = PIN ? lane < e : (lane >= nz && lane < nz + e);          // ... an equality multiplier (PIN: on the pinned coordinate's lane)
  const bool vf = PIN ? (vx && !ve) : vx;                                  // ... a free x entry
  const int ya = PIN ? lane : lane - nz;                                   // (an equality lane's row)

  // ---- assembly (engines.py:31-32,50-74; world.py:144-234) ----------------------------------------------------------
  const float* vv = DENSE ? nullptr : (const float*)SP.v + (size_t)scene * nz;
  float jn[6] = {0, 0, 0, 0, 0, 0}, jf[6] = {0, 0, 0, 0, 0, 0};            // (fp32 inputs: exact, half the registers)
  int c0 = 0, c1 = 0;                                                      // first columns of the contact's two bodies
  double mu_c = 0, hn = 0;
  double qd = 0, p = 0, b_in = 0;
  for (int i = lane; i < ASZ; i += 64) At[i] = 0.0f;
  wsync();
  if constexpr (DENSE) {
    // dense boundary: G = [Jc; Jf; 0] with Jf rows (+jt, -jt) (engines.py:67-68, world.py:191-192), F[3nc + c][c] = mu_c
    // (engines.py:71), h = [h_n; 0; 0] (:74), at most two bodies per contact - all verified per scene by lcp_classify_big
    // (round 5: lcp_classify_big, the one pass over the dense tensors, left the contact's record in the workspace block - its six
    //  entries of Jc / Jt on its two bodies, the bodies' first columns, mu_c, h_n - component-major, 16 x ncap floats)
    if (vc) {
      const float* rec = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(Wg) + DENSE_EXTRACT_OFF);
#pragma unroll
      for (int q = 0; q < 6; ++q) { jn[q] = rec[q * ncap + ci]; jf[q] = rec[(6 + q) * ncap + ci]; }
      c0 = __float_as_int(rec[12 * ncap + ci]); c1 = __float_as_int(rec[13 * ncap + ci]);
      if (BWD) mu_c = HOIST_IT ? wmu_l : Wit[ZO + 8 * LX + lane];                                              // (as the contact-list backward: from the iterate block)
      else { mu_c = (double)rec[14 * ncap + ci]; hn = (double)rec[15 * ncap + ci]; }
    }
    if (BWD) { if (vx) qd = HOIST_IT ? wqd_l : Wit[ZO + 9 * LX + lane]; }
    else {
      if (vx) { qd = (double)DN.Q[(size_t)scene * nz * nz + (size_t)lane * nz + lane]; p = (double)DN.p[(size_t)scene * nz + lane]; }
      if (ve) b_in = (double)DN.b[(size_t)scene * e + ya];
      Wit[ZO + 8 * LX + lane] = mu_c; Wit[ZO + 9 * LX + lane] = qd;
    }
    for (int i = lane; i < e * nz; i += 64) { const int a = i / nz, k = i - a * nz; At[a * AST + k] = DN.A[(size_t)scene * e * nz + i]; }
  } else {
    if (vc) {
      const ContactRows<float> r = make_contact<float>((const float*)SP.c_n + (size_t)scene * ncap * 2, (const float*)SP.c_p1 + (size_t)scene * ncap * 2,
                                                       (const float*)SP.c_p2 + (size_t)scene * ncap * 2, SP.c_i1 + (size_t)scene * ncap,
                                                       SP.c_i2 + (size_t)scene * ncap, (const float*)SP.rest + (size_t)scene * nb,
                                                       (const float*)SP.fric + (size_t)scene * nb, vv, ci);
#pragma unroll
      for (int q = 0; q < 6; ++q) { jn[q] = r.jn[q]; jf[q] = r.jf[q]; }
      c0 = 3 * r.b1; c1 = 3 * r.b2;
      mu_c = (double)r.mu; hn = (double)r.h;
    }
    if (vx) {
      qd = (double)md_l;
      p = (double)momentum_entry<float>(md_l, vv_l, (float)SP.dt, ff_l);                      // engines.py:32
    }
    for (int i = lane; i < e * nz; i += 64) { const int a = i / nz, k = i - a * nz; At[a * AST + k] = ((const float*)SP.Je)[(size_t)scene * e * nz + i]; }
  }
  auto colq = [&](int q) { return q < 3 ? c0 + q : c1 + (q - 3); };
  wsync();
  bool broken = false;                                                     // LCP_HINT_PINNED on a scene whose rows are not [I 0]
  if constexpr (PIN) {
    bool okl = true;
#pragma unroll
    for (int a = 0; a < EQC; ++a) { if (a < e) okl = okl && (!vx || At[a * AST + lane] == ((lane == a) ? 1.0f : 0.0f)); }
    broken = !__all(okl);
    if (!BWD && broken) {
      if (vx) ((float*)SP.v_new)[(size_t)scene * nz + lane] = nan_of<float>();
      if (lane == 0) { if (SP.iters) SP.iters[scene] = 0; if (SP.status) SP.status[scene] = LCP_ST_NAN; }
      return;
    }
  }
  int status = truncated;
  if (__any(vx && !(qd != 0.0))) status |= LCP_ST_SINGULAR_Q;
  // the lane's column / row of A: x lanes hold A[:, lane], the equality lane nz + a holds nothing extra (its row is read from At)
  auto acol = [&](int a) -> double { return (EQC <= 4 || lane < nz) ? (double)At[a * AST + lane] : 0.0; };    // (zero beyond nz: At is cleared)

  // ---- products ------------------------------------------------------------------------------------------------------
  auto Gv = [&](double v, double& gn, double& gt) {                       // m-space <- x-space (v on the x lanes)
    xv[lane] = vx ? v : 0.0; wsync();
    gn = 0; gt = 0;
    if (vc) {
#pragma unroll
      for (int q = 0; q < 6; ++q) { const double xq = xv[colq(q)]; gn = fma((double)jn[q], xq, gn); gt = fma((double)jf[q], xq, gt); }
    }
    wsync();
  };
  auto Gtw = [&](double wn, double wt) -> double {                        // x-space <- m-space (Jc^T wn + Jt^T wt)
    xv[lane] = 0.0; wsync();
    if (vc) {
#pragma unroll
      for (int q = 0; q < 6; ++q) lds_add(&xv[colq(q)], fma((double)jf[q], wt, (double)jn[q] * wn));
    }
    wsync();
    const double r = vx ? xv[lane] : 0.0;
    wsync();
    return r;
  };
  auto Av = [&](double v) -> double {                                     // equality lanes <- x lanes
    double out = 0;
    if constexpr (EQC <= 4) {
#pragma unroll
      for (int a = 0; a < EQC; ++a) { if (a < e) { const double sm = wave_sum(acol(a) * (vx ? v : 0.0)); if (lane == nz + a) out = sm; } }
    } else {                                                              // many rows (chains of joints): every equality lane sums its own row
      xv[lane] = vx ? v : 0.0; wsync();
      if (ve) { const float* ar = At + (lane - nz) * AST; for (int k = 0; k < nz; ++k) out = fma((double)ar[k], xv[k], out); }
      wsync();
    }
    return out;
  };
  auto Aty = [&](double y) -> double {                                    // x lanes <- equality lanes
    double acc = 0;
    if constexpr (EQC <= 4) {
#pragma unroll
      for (int a = 0; a < EQC; ++a) { if (a < e) acc = fma(acol(a), bcast_lane(y, nz + a), acc); }
    } else {
      for (int a = 0; a < e; ++a) acc = fma(acol(a), bcast_lane(y, nz + a), acc);
    }
    return acc;
  };

  // ---- the contact's 4 x 4 block M = F_c + diag(s / z), inverted in closed form ------------------------------------------------
  double idn = 1, i1 = 1, i2 = 1, kap = 1.0 / 3.0;                         // 1 / Dn, 1 / D1, 1 / D2, 1 / (Dg + 1 / D1 + 1 / D2)
  double b00 = 0, b10 = 0, b11 = 0;                                        // the 2 x 2 matrix of G^T M^-1 G in (Jc, Jt) coordinates
  auto block_setup = [&](const M4<double>& D) {                           // D = 1 / d = s / z
#if LCP_PRIMAL_RCP_STEP
    idn = fast_rcp(D.n); i1 = fast_rcp(D.f1); i2 = fast_rcp(D.f2);         // (v_rcp_f64 + two Newton steps, as factor_pq of lcp_quad_kernels.inc)
    kap = fast_rcp(D.g + (i1 + i2));
#else
    idn = 1.0 / D.n; i1 = 1.0 / D.f1; i2 = 1.0 / D.f2;
    kap = 1.0 / (D.g + (i1 + i2));
#endif
    b00 = idn;
    b10 = kap * (i1 - i2) * (mu_c * idn);
    b11 = kap * fma(i1 + i2, D.g, 4.0 * (i1 * i2));                        // = (i1 + i2) - kap (i1 - i2)^2, without the cancellation
  };
  auto minv = [&](const M4<double>& t) -> M4<double> {                    // M^-1 t
    M4<double> o;
    o.n = idn * t.n;
    o.g = kap * ((t.g - mu_c * o.n) + fma(i1, t.f1, i2 * t.f2));
    o.f1 = i1 * (t.f1 - o.g);
    o.f2 = i2 * (t.f2 - o.g);
    return o;
  };

#ifdef LCP_PRIMAL_PROFILE
  long long pc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tk = clock64();
#endif
  // ---- formation + LU of K = [[Q + G^T M^-1 G, A^T], [A, 0]]: row `lane` in t[], 1 / U[lane][lane] in udinv ---------------------
  double t[NCOL];
  double udinv = 1.0;
  bool singular = false;
  // block layout of the sweeps (BSW): this lane's DPP row / position, its row of the image, the diagonal block of its row split into
  // the part below the diagonal (forward sweep) and above it (backward sweep; the pinned rows' entries on the partial lanes)
  const int br = lane >> 4, bl = lane & 15;
  const int brow = br * BS + bl;
  const bool blive = BSW && br < 3 && bl < BS && brow < NCOL, bpart = BSW && br < 3 && bl >= BS && bl < BS + PIN;
  const double* irow = Kl + (blive ? clo + brow : NROW) * LDK;              // (partial and idle lanes: the zero row - their off-diagonal blocks)
  double dgL[BSW ? BS : 1], dgU[BSW ? BS : 1], udb = 1.0;
  // lane selects of the two permutations (ds_bpermute: bytes): coordinate layout -> block layout and back; lane 63 holds a zero
  const int a_in = 4 * (blive ? clo + brow : ((bpart && br == 0) ? bl - BS : 63));
  const int a_o1 = 4 * ((lane >= clo && lane - clo < NCOL) ? 16 * ((lane - clo) / BS) + (lane - clo) % BS : (lane < clo ? BS + lane : 63));
  auto bperm = [&](double v, int a) -> double {
    return __hiloint2double(__builtin_amdgcn_ds_bpermute(a, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(a, __double2loint(v)));
  };
  auto factor = [&]() LCP_INL {
    // (the lane compares below are invariant over the PDIPM loop: hoisted, their ~100 masks overflow the scalar file and come
    //  back through v_readlane spills - an opaque copy of the lane index keeps them local to the factorisation)
    int ln = lane - clo; asm volatile("" : "+v"(ln));                       // the lane's pivot index (negative: a pinned coordinate's row)
    for (int i = lane; i < KROWS * LDK; i += 64) Kl[i] = 0.0;
    wsync();
    if constexpr (PIN) { if (ln >= 0 && ln < NCOL) Kl[lane * LDK + ln] = vx ? qd : 1.0; }
    else if (lane < NCOL) Kl[lane * LDK + lane] = vx ? qd : (ve ? 0.0 : 1.0);   // rows beyond the system: identity
    if (!PIN && vx) {
      if constexpr (EQC <= 4) {
#pragma unroll
        for (int a = 0; a < EQC; ++a) { if (a < e) { const double av = acol(a); Kl[lane * LDK + nz + a] = av; Kl[(nz + a) * LDK + lane] = av; } }
      } else {
        for (int a = 0; a < e; ++a) { const double av = acol(a); Kl[lane * LDK + nz + a] = av; Kl[(nz + a) * LDK + lane] = av; }
      }
    }
    wsync();
    if (vc) {
      double p0[6], p1[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) { p0[q] = b00 * (double)jn[q]; p1[q] = fma(b10, (double)jn[q], b11 * (double)jf[q]); }
#pragma unroll
      for (int pq = 0; pq < 6; ++pq) {
        double* row = Kl + colq(pq) * LDK - clo;
#pragma unroll
        for (int q = 0; q < 6; ++q) { if (!PIN || colq(q) >= clo) lds_add(row + colq(q), fma((double)jf[pq], p1[q], (double)jn[pq] * p0[q])); }
      }
    }
    wsync();
    PR_TICK(1)
    if constexpr (GRID && LCP_PRIMAL_GRIDLU_V2) {
      // ---- LU on a 4 x 16 lane grid, second form (round 4).  Same layout, same elimination order and the same products as the first
      // form below - bit for bit its factors -, with what a pivot costs beside its multiply-adds cut down: the LU is bound by the
      // VALU issue slots of its wavefront (row per lane: two v_readlane + one FMA per entry, ~1700 slots per factorisation; first
      // grid form: ~1400, of which 460 multiply-adds as v_mov_b64_dpp + v_fma pairs and ~30 per pivot around them).
      //   * trailing update: ONE asm block of v_fmac_f64_dpp ... row_newbcast per pivot (lcp_primal_gridlu.h): the broadcast rides
      //     in the multiply-add, half the slots;
      //   * the multipliers of a pivot live in the DPP row that holds the pivot column; the other rows get them through LDS - every
      //     lane stores its candidate (one ds_write_b64, no compare), every lane reads the slot of the pivot column's row back (one
      //     ds_read_b64 at a compile-time offset): no v_permlane swaps, no VALU slot at all (the first form: ~8 per multiplier);
      //   * lane masks (rows below the pivot, the pivot column's DPP row) are COMPILE-TIME 64-bit constants moved into vcc inside the
      //     v_cndmask statements (keep_lanes / take_lanes): no v_cmp, no mask registers; "only the rows right of the pivot column" is
      //     the multiply-add's own row_mask;
      //   * zero / NaN pivots are looked for once, on the finished diagonal, not per pivot.
      constexpr int NJ = (NCOL + 3) / 4, NA = (NCOL + 15) / 16;
      static_assert(NA <= 2, "the lane grid holds two row slots");
      int l16 = lane & 15, r4 = lane >> 4;
      asm volatile("" : "+v"(l16)); asm volatile("" : "+v"(r4));
      double a0[NJ], a1[NJ];
      {
        const int i0 = l16 < NCOL ? l16 : NCOL - 1, i1 = l16 + 16 < NCOL ? l16 + 16 : NCOL - 1;   // (rows beyond the system: a copy that is never written back)
        static_for<NJ>([&](auto J_) LCP_INL {
          constexpr int J = J_;
          const int c = 4 * J + r4;
          a0[J] = (c < NCOL) ? Kl[(clo + i0) * LDK + c] : 0.0;
          a1[J] = (NA > 1 && c < NCOL) ? Kl[(clo + i1) * LDK + c] : 0.0;
        });
      }
      double* const gxw = gx + lane;                                        // this lane's candidate slot: gx[A][lane]
      const double* const gxr = gx + l16;                                   // + 64 A + 16 rk: the pivot column's row
#if LCP_PRIMAL_GRIDLU_V2 == 2
      // Software-pipelined form: the multipliers of pivot k + 1 are computed - and their LDS round trip started - as soon as pivot k
      // has updated the column slot of column k + 1; the bulk of pivot k's trailing update then runs while they travel (the
      // reciprocal's dependent chain and the LDS latency leave the critical path; same operations on the same values: bit for bit
      // the factors of the forms above)
      double u0 = 0, u1 = 0;                                                // multipliers of the CURRENT pivot, as every DPP row sees them
      auto prep = [&](auto K_) LCP_INL {                                    // pivot K_: reciprocal, multipliers into the factors, LDS hand-over started
        constexpr int k = K_, rk = k % 4, jk = k / 4, lk = k % 16, ak = k / 16;
        constexpr unsigned long long ROW = 0xFFFFull << (16 * rk);
        constexpr unsigned long long B0 = grid_below(k, 0), B1 = grid_below(k, 1);
        const double piv = q16::bc<lk>(ak == 0 ? a0[jk] : a1[jk]);
        #if LCP_PRIMAL_EXP_RCP1
        double inv = __builtin_amdgcn_rcp(piv); inv = fma(fma(-piv, inv, 1.0), inv, inv);   // (experiment: ONE Newton step, ~2^-46)
#else
        const double inv = fast_rcp(piv);
#endif
#if LCP_PRIMAL_GRIDLU_XROW
        // the multipliers cross the DPP rows by lane swaps (four dependent VALU operations per half) instead of an LDS round trip:
        // more issue slots, a shorter dependent chain per pivot (A/B: profiles/r04_ab_config5.txt)
        if constexpr (ak == 0) {
          const double l0 = keep_lanes<B0>(a0[jk] * inv);
          if constexpr ((B0 & ROW) != 0) a0[jk] = take_lanes<(B0 & ROW)>(a0[jk], l0);
          u0 = rows_bcast<rk>(l0);
        }
        if constexpr (NA > 1) {
          const double l1 = keep_lanes<B1>(a1[jk] * inv);
          if constexpr ((B1 & ROW) != 0) a1[jk] = take_lanes<(B1 & ROW)>(a1[jk], l1);
          u1 = rows_bcast<rk>(l1);
        }
#else
        if constexpr (ak == 0) {
          const double l0 = keep_lanes<B0>(a0[jk] * inv);
          if constexpr ((B0 & ROW) != 0) a0[jk] = take_lanes<(B0 & ROW)>(a0[jk], l0);
          gxw[0] = l0;
        }
        if constexpr (NA > 1) {
          const double l1 = keep_lanes<B1>(a1[jk] * inv);
          if constexpr ((B1 & ROW) != 0) a1[jk] = take_lanes<(B1 & ROW)>(a1[jk], l1);
          gxw[LX] = l1;
        }
        wsync();
        if constexpr (ak == 0) u0 = gxr[16 * rk];
        if constexpr (NA > 1) u1 = gxr[LX + 16 * rk];
#endif
      };
      prep(std::integral_constant<int, 0>{});
      static_for<NCOL - 1>([&](auto K_) LCP_INL {
        constexpr int k = K_, rk = k % 4, jk = k / 4, lk = k % 16, ak = k / 16;
        constexpr int RM = (0xf << (rk + 1)) & 0xf;                         // DPP rows whose column of slot jk lies right of column k (none behind the last row)
        constexpr int JN = (k + 1) / 4;                                     // the slot of column k + 1: jk, or jk + 1 behind the last DPP row
        constexpr int RA = (JN == jk) ? RM : 0xf;                           // (slot jk: the rows right of the pivot column only - the instruction's row_mask)
        const double c0 = u0, c1 = u1;                                      // (this pivot's multipliers; prep() below overwrites u0 / u1)
        // first the slot of the next pivot column ...
        if constexpr (ak == 0 && NA > 1) grid_two<lk, JN, (JN < NJ ? 1 : 0), RA>(a0, a1, c0, c1);
        else if constexpr (ak == 0) grid_one<lk, JN, (JN < NJ ? 1 : 0), RA>(a0, c0);
        else grid_one<lk, JN, (JN < NJ ? 1 : 0), RA>(a1, c1);
        // ... then the next pivot's multipliers set off ...
#ifdef LCP_PRIMAL_EXP_PREP_EVERY
        // EXPERIMENT ONLY (wrong factors!): the per-pivot chain - reciprocal, multipliers, masks, hand-over across the DPP rows - only for
        // every LCP_PRIMAL_EXP_PREP_EVERY-th pivot, the multiply-adds of all of them: what pivots in blocks could save AT MOST (they
        // would still pay a closed-form block inverse and the block's multipliers) - tools/experiments/block_pivot_bound.py
        if constexpr (k + 1 < NCOL - 1 && ((K_ + 1) % LCP_PRIMAL_EXP_PREP_EVERY) == 0) prep(std::integral_constant<int, K_ + 1>{});
#else
        if constexpr (k + 1 < NCOL - 1) prep(std::integral_constant<int, K_ + 1>{});
#endif
        // ... and the rest of this pivot's update runs meanwhile
        if constexpr (ak == 0 && NA > 1) grid_two<lk, JN + 1, (NJ - JN - 1 > 0 ? NJ - JN - 1 : 0), 0xf>(a0, a1, c0, c1);
        else if constexpr (ak == 0) grid_one<lk, JN + 1, (NJ - JN - 1 > 0 ? NJ - JN - 1 : 0), 0xf>(a0, c0);
        else grid_one<lk, JN + 1, (NJ - JN - 1 > 0 ? NJ - JN - 1 : 0), 0xf>(a1, c1);
      });
#else
      static_for<NCOL - 1>([&](auto K_) LCP_INL {
        constexpr int k = K_, rk = k % 4, jk = k / 4, lk = k % 16, ak = k / 16;
        constexpr unsigned long long ROW = 0xFFFFull << (16 * rk);           // lanes of the DPP row that holds column k
        constexpr int RM = (0xf << (rk + 1)) & 0xf;                         // DPP rows whose column of slot jk lies right of column k: the row_mask of that slot's update
        constexpr unsigned long long B0 = grid_below(k, 0), B1 = grid_below(k, 1);   // rows of slot 0 / slot 1 below the pivot row
        constexpr int JF = (rk == 3) ? jk + 1 : jk, NF = NJ - JF;           // column slots the update visits (the pivot column's own slot: rows right of it only)
        const double piv = q16::bc<lk>(ak == 0 ? a0[jk] : a1[jk]);           // (the pivot: valid in DPP row rk)
        const double inv = fast_rcp(piv);
        if constexpr (ak == 0 && NA > 1) {
          const double l0 = keep_lanes<B0>(a0[jk] * inv), l1 = keep_lanes<B1>(a1[jk] * inv);
          if constexpr ((B0 & ROW) != 0) a0[jk] = take_lanes<(B0 & ROW)>(a0[jk], l0);
          a1[jk] = take_lanes<(B1 & ROW)>(a1[jk], l1);
          gxw[0] = l0; gxw[LX] = l1;
          wsync();
          const double u0 = gxr[16 * rk], u1 = gxr[LX + 16 * rk];
          wsync();
          grid_two<lk, JF, NF, (JF == jk ? RM : 0xf)>(a0, a1, u0, u1);
        } else if constexpr (ak == 0) {                                      // (at most 16 columns: one row slot)
          const double l0 = keep_lanes<B0>(a0[jk] * inv);
          if constexpr ((B0 & ROW) != 0) a0[jk] = take_lanes<(B0 & ROW)>(a0[jk], l0);
          gxw[0] = l0;
          wsync();
          const double u0 = gxr[16 * rk];
          wsync();
          grid_one<lk, JF, NF, (JF == jk ? RM : 0xf)>(a0, u0);
        } else {
          const double l1 = keep_lanes<B1>(a1[jk] * inv);
          if constexpr ((B1 & ROW) != 0) a1[jk] = take_lanes<(B1 & ROW)>(a1[jk], l1);
          gxw[LX] = l1;
          wsync();
          const double u1 = gxr[LX + 16 * rk];
          wsync();
          grid_one<lk, JF, NF, (JF == jk ? RM : 0xf)>(a1, u1);
        }
      });
#endif
      {
        const int i0 = l16, i1 = l16 + 16;
        static_for<NJ>([&](auto J_) LCP_INL {
          constexpr int J = J_;
          const int c = 4 * J + r4;
          if (i0 < NCOL && c < NCOL) Kl[(clo + i0) * LDK + c] = a0[J];
          if (NA > 1 && i1 < NCOL && c < NCOL) Kl[(clo + i1) * LDK + c] = a1[J];
        });
      }
      wsync();
      if constexpr (BSW) {
        // the sweeps' registers: the diagonal block of the lane's row, masked once here (compile-time lane masks), and 1 / U[row][row]
        const double* dptr = (blive ? irow : Kl + (bpart ? bl - BS : NROW) * LDK) + ((blive || bpart) ? br * BS : 0);
        static_for<BS>([&](auto K_) LCP_INL {
          constexpr int k = K_;
          const double v = dptr[k];
          dgL[k] = keep_lanes<bs_mask_lower(k, BS, NCOL)>(v);
          dgU[k] = keep_lanes<bs_mask_upper(k, BS, NCOL, PIN)>(v);
        });
        const double dg = irow[blive ? brow : 0];
        udb = blive ? fast_rcp(dg) : 1.0;
        singular = __any(blive && (!(dg != 0.0) || (dg != dg)));             // a zero / NaN pivot
        // the backward sweep runs on the UNIT upper factor D^-1 U (one multiply-add per step on its dependent chain, not a multiply
        // and a multiply-add): the diagonal block of the lane's row is scaled here, once per factorisation; the blocks right of it
        // stay as they are in the image and their sums are scaled as they enter (BsUpdate's `sc`).  The partial lanes keep the
        // pinned rows as they are: udb = 1.  (Measured and dropped: scaling those blocks IN the image - 40 LDS operations per lane
        // and factorisation: LU phase 109 k -> 125 k cycles per scene, the CU's eight wavefronts queue on the LDS.)
        static_for<BS>([&](auto K_) LCP_INL { dgU[K_] *= udb; });
        return;                                                             // (the image stays: the sweeps read the off-diagonal blocks from it)
      }
      {
        const double* row = Kl + (lane < NROW ? lane : 0) * LDK;
        static_for<NCOL>([&](auto J) LCP_INL { t[J] = row[J]; });
        if (lane >= NROW) static_for<NCOL>([&](auto J) LCP_INL { t[J] = 0.0; });
        bool bad = false;
        if (ln >= 0 && ln < NCOL) { const double dg = row[ln]; udinv = fast_rcp(dg); bad = !(dg != 0.0) || (dg != dg); }   // 1 / U[row][row]; a zero / NaN pivot
        singular = __any(bad);
      }
      wsync();
      return;
    }
    if constexpr (GRID) {
      // ---- LU on a 4 x 16 lane grid (pinned form, <= 32 columns).  Lane (r = lane / 16, l = lane % 16) holds the live rows l and
      // l + 16 of the columns 4 j + r: the pivot row arrives inside the DPP row with the multiply-add (row_newbcast, no
      // v_readlane), the two multipliers of a lane's rows cross the DPP rows through lane swaps.  Same elimination order and the
      // same products as the row-per-lane form below: bit for bit its factors (A/B: LCP_PRIMAL_GRIDLU = 0).  The pinned
      // coordinates' rows stay in the image untouched.  tools/experiments/lu_micro.hip: 22 k cycles per factorisation at two
      // waves per SIMD against 30 k.
      constexpr int NJ = (NCOL + 3) / 4, NA = (NCOL + 15) / 16;
      int l16 = lane & 15, r4 = lane >> 4;
      asm volatile("" : "+v"(l16)); asm volatile("" : "+v"(r4));
      double a[NA][NJ];
      static_for<NA>([&](auto A_) LCP_INL {
        constexpr int A = A_;
        const int i = l16 + 16 * A, ic = i < NCOL ? i : NCOL - 1;          // (rows beyond the system: a copy that is never written back)
        static_for<NJ>([&](auto J_) LCP_INL { constexpr int J = J_; const int c = 4 * J + r4; a[A][J] = (c < NCOL) ? Kl[(clo + ic) * LDK + c] : 0.0; });
      });
      bool bad = false;
      static_for<NCOL>([&](auto K_) LCP_INL {
        constexpr int k = K_, rk = k % 4, jk = k / 4, lk = k % 16, ak = k / 16;
        const double piv = q16::bc<lk>(a[ak][jk]);                           // (the pivot: valid in DPP row rk)
        const double inv = fast_rcp(piv);
        bad = bad || (r4 == rk && (!(piv != 0.0) || (piv != piv)));
        double b[NA];
        static_for<NA - ak>([&](auto AA) LCP_INL {
          constexpr int A = ak + AA;
          const bool below = l16 + 16 * A > k;
          const double mlt = q16::keep_if(a[A][jk] * inv, below);
          if (r4 == rk && below) a[A][jk] = mlt;
          b[A] = rows_bcast<rk>(mlt);
        });
        static_for<NJ - jk>([&](auto JJ) LCP_INL {
          constexpr int jj = jk + JJ;
          static_for<NA - ak>([&](auto AA) LCP_INL {
            constexpr int A = ak + AA;
            double u = b[A];
            if constexpr (jj == jk) u = q16::keep_if(u, r4 > rk);             // (this slot's columns <= k are finished)
            q16::fnmac_bc<lk>(a[A][jj], a[ak][jj], u);
          });
        });
      });
      singular = __any(bad);
      static_for<NA>([&](auto A_) LCP_INL {
        constexpr int A = A_;
        const int i = l16 + 16 * A;
        static_for<NJ>([&](auto J_) LCP_INL { constexpr int J = J_; const int c = 4 * J + r4; if (i < NCOL && c < NCOL) Kl[(clo + i) * LDK + c] = a[A][J]; });
      });
      wsync();
      {
        const double* row = Kl + (lane < NROW ? lane : 0) * LDK;
        static_for<NCOL>([&](auto J) LCP_INL { t[J] = row[J]; });
        if (lane >= NROW) static_for<NCOL>([&](auto J) LCP_INL { t[J] = 0.0; });
        if (ln >= 0 && ln < NCOL) udinv = fast_rcp(row[ln]);                 // 1 / U[row][row], as the row-per-lane form keeps it
      }
      wsync();
      return;
    }
    {
      const double* row = Kl + (lane < NROW ? lane : 0) * LDK;
      static_for<NCOL>([&](auto J) LCP_INL { t[J] = row[J]; });
      if (lane >= NROW) static_for<NCOL>([&](auto J) LCP_INL { t[J] = 0.0; });
    }
    wsync();
    singular = false;
    static_for<(NCOL + 7) / 8>([&](auto G8) LCP_INL {
      if (8 * G8 < n) {
        static_for<(NCOL - 8 * G8 < 8 ? NCOL - 8 * G8 : 8)>([&](auto KK) LCP_INL {
          constexpr int k = 8 * G8 + KK;
          const double pk = bcast_lane(t[k], k + clo);
          singular = singular || !(pk != 0.0) || (pk != pk);
          const double inv = fast_rcp(pk);
          if (ln == k) udinv = inv;
          const double l = (ln > k) ? t[k] * inv : 0.0;
          if (ln > k) t[k] = l;
          // pivot-row entries in batches of 8 scalar pairs, then the 8 FMAs: back to back, every v_readlane -> v_fma pair
          // costs two wait states more and the pairs serialise on one scalar register.  (Measured and dropped: the pivot row
          // through LDS - lane k stores it with ds_write_b128, every lane reads it back at a uniform address.  Fewer
          // instructions, but every read moves 1 KB through the CU's one LDS port and eight waves share it: 3.8 M against
          // 6.5 M sim steps/s on config 5.  Also measured and dropped: skipping the 3 x 3 column blocks a pivot row cannot reach
          // - block masks from the contact graph, symbolic elimination on scalars, bodies in reverse order to keep the fill
          // low (31 of 66 block visits on a config-5 pile) - with scalar branches between batches of three columns: the
          // shorter batches and the branches cost more than the skipped work saves, 6.3 M against 6.5 M; towers gained 3-5 %.)
          constexpr int NJ = NCOL - 1 - k;
          static_for<(NJ + 7) / 8>([&](auto C8) LCP_INL {
            constexpr int j0 = k + 1 + 8 * C8, nj = (NJ - 8 * C8) < 8 ? (NJ - 8 * C8) : 8;
            double pv[8];
            static_for<nj>([&](auto I) LCP_INL { pv[I] = bcast_lane(t[j0 + I], k + clo); });
            static_for<nj>([&](auto I) LCP_INL { sgpr_pin(pv[I]); });
            static_for<nj>([&](auto I) LCP_INL { t[j0 + I] = fma(-l, pv[I], t[j0 + I]); });
          });
        });
      }
    });
  };
  // K^-1 w (w: entry `lane` of the right-hand side)
  // (measured and dropped, round 4: the multiply-add of a sweep step under a compile-time EXECUTION mask (s_mov exec, v_fma, restore)
  //  instead of v_cmp + v_cndmask on the multiplier - fewer VALU slots, but every exec write stalls the VALU pipeline: solve_kkt
  //  72 k -> 96 k cycles per scene on config 5; masking the multiplier with one v_cndmask on a vcc immediate needs a temporary pair per
  //  step and tips this 255-register kernel into 73 spills - profiles/r04_ab_config5.txt)
  auto ksolve = [&](double w) -> double {
    if constexpr (BSW) {
      // Block layout (lcp_primal_bsweep.h).  L = [[L00, 0, 0], [L10, L11, 0], [L20, L21, L22]] by blocks of BS rows, one block per DPP
      // row: solve a diagonal block inside its row (the entry a step needs comes with the multiply-add), hand the block's solution to
      // the rows below / above (rows_bcast: lane swaps), subtract its off-diagonal blocks there (entries read from the image, issued
      // a stage ahead) - the same multiply-adds in the same order per row as the row-per-lane sweeps, ~150 VALU slots instead of ~390.
      // The pinned coordinates' rows ride along in the backward sweep as before: one partial sum per block, added on the way out.
      double wb = bperm(w, a_in);
      double o[BS];
      static_for<BS>([&](auto J) LCP_INL { o[J] = irow[J]; });                                   // L(., block 0)
      BsSolveL<BS - 1, 0x1>::run(wb, dgL);
      double c = rows_bcast<0>(wb);
      BsUpdate<BS, 0x6, true>::run(wb, c, 1.0, o);
      static_for<BS>([&](auto J) LCP_INL { o[J] = irow[BS + J]; });                              // L(., block 1)
      BsSolveL<BS - 1, 0x2>::run(wb, dgL);
      c = rows_bcast<1>(wb);
      BsUpdate<BS, 0x4, true>::run(wb, c, 1.0, o);
      static_for<BS>([&](auto J) LCP_INL { o[J] = irow[2 * BS + J]; });                          // U(., block 2) (columns beyond the system: the image's zero padding)
      BsSolveL<BS - 1, 0x4>::run(wb, dgL);
      wb *= udb;                                                                                 // D^-1 y (unit upper factor)
      BsSolveU<BS, BS - 1, 0x4>::run(wb, dgU);
      c = rows_bcast<2>(wb);
      BsUpdate<BS, 0x3, false>::run(wb, c, udb, o);
      static_for<BS>([&](auto J) LCP_INL { o[J] = irow[BS + J]; });                              // U(., block 1)
      BsSolveU<BS, BS - 1, 0x2>::run(wb, dgU);
      c = rows_bcast<1>(wb);
      BsUpdate<BS, 0x1, false>::run(wb, c, udb, o);
      BsSolveU<BS, BS - 1, 0x1>::run(wb, dgU);
      const double xb = wb;
      // back to the coordinate layout; a pinned coordinate's lane adds its three partial sums
      const int a_o2 = lane < clo ? a_o1 + 64 : 252, a_o3 = lane < clo ? a_o1 + 128 : 252;
      return (bperm(xb, a_o1) + bperm(xb, a_o2)) + bperm(xb, a_o3);
    }
    int ln = lane - clo; asm volatile("" : "+v"(ln));
    static_for<(NCOL + 7) / 8>([&](auto G8) LCP_INL {
      if (8 * G8 < n) {
        static_for<(NCOL - 8 * G8 < 8 ? NCOL - 8 * G8 : 8)>([&](auto KK) LCP_INL {
          constexpr int k = 8 * G8 + KK;
          const double yk = bcast_lane(w, k + clo);
          w = fma(-((ln > k) ? t[k] : 0.0), yk, w);
        });
      }
    });
    static_for<(NCOL + 7) / 8>([&](auto GR) LCP_INL {
      constexpr int g8 = (NCOL + 7) / 8 - 1 - GR, gk = (NCOL - 8 * g8 < 8 ? NCOL - 8 * g8 : 8);
      if (8 * g8 < n) {
        static_for<gk>([&](auto KR) LCP_INL {
          constexpr int k = 8 * g8 + gk - 1 - KR;
          const double xk = bcast_lane(w * udinv, k + clo);
          w = fma(-((ln < k) ? t[k] : 0.0), xk, w);                           // (PIN: the pinned rows, ln < 0, collect -(S dx)_p)
        });
      }
    });
    return w * udinv;
  };

  // solve_kkt (pdipm.py:325-354) in body space; di = 1 / d.  rx / ox: x lanes, ry / oy: equality lanes
  auto solve_kkt = [&](const M4<double>& di, double rx, const M4<double>& rs, const M4<double>& rz, double ry,
                       double& ox, M4<double>& os, M4<double>& oz, double& oy) {
    M4<double> q = m4<double>(rs.n * di.n - rz.n, rs.f1 * di.f1 - rz.f1, rs.f2 * di.f2 - rz.f2, rs.g * di.g - rz.g);
    if (!vc) q = m4<double>(0, 0, 0, 0);
    const M4<double> u = minv(q);
    const double gu = Gtw(vc ? u.n : 0.0, vc ? u.f1 - u.f2 : 0.0);
    const double rhs = vx ? (gu - rx) : (ve ? -ry : 0.0);                   // (PIN: ve lanes are x lanes - rhs_p = (gu - rx)_p, -ry_p = 0)
#ifdef LCP_PRIMAL_PROFILE
    const long long ks0 = clock64();
#endif
    const double sol = ksolve(rhs);
#ifdef LCP_PRIMAL_PROFILE
    pc[6] += clock64() - ks0;                                               // (the triangular sweeps alone, inside solve_kkt's pc[4])
#endif
    ox = vf ? sol : 0.0; oy = ve ? sol : 0.0;                               // (PIN: dx_p = 0, dy_p = rhs_p - (S dx)_p from the sweep)
    double gn, gt;
    Gv(ox, gn, gt);
    oz = minv(m4<double>(gn - q.n, gt - q.f1, -gt - q.f2, -q.g));
    if (!vc) oz = m4<double>(0, 0, 0, 0);
    os = m4<double>((-rs.n - oz.n) * di.n, (-rs.f1 - oz.f1) * di.f1, (-rs.f2 - oz.f2) * di.f2, (-rs.g - oz.g) * di.g);   // :347,350
    if (!vc) os = m4<double>(0, 0, 0, 0);
  };

#if !LCP_PRIMAL_RCP_STEP
  // get_step for (z, dz), (s, ds) (pdipm.py:182-186), NaN semantics as in lcp_quad.hip step_pair_q
  auto step_pair = [&](const M4<double>& z, const M4<double>& dz, const M4<double>& s, const M4<double>& ds) -> double {
    const double ninf = -inf_of<double>(), pinf = inf_of<double>();
    const M4<double> az = m4<double>(-z.n / dz.n, -z.f1 / dz.f1, -z.f2 / dz.f2, -z.g / dz.g);
    const M4<double> as = m4<double>(-s.n / ds.n, -s.f1 / ds.f1, -s.f2 / ds.f2, -s.g / ds.g);
    auto key4 = [&](const M4<double>& a) { return umax(umax(nan_key(a.n), nan_key(a.f1)), umax(nan_key(a.f2), nan_key(a.g))); };
    auto max4 = [&](const M4<double>& a) { return __builtin_fmax(__builtin_fmax(a.n, a.f1), __builtin_fmax(a.f2, a.g)); };
    auto min4 = [&](const M4<double>& a) { return __builtin_fmin(__builtin_fmin(a.n, a.f1), __builtin_fmin(a.f2, a.g)); };
    {
      // the fill max(1, a.max()) is at least every entry: where both vectors have an entry it does not replace (dv <= 0) and nothing
      // is NaN, a.min() is the minimum over those entries and the fill's four reductions drop out (lcp_quad_kernels.inc, step_pair_q:
      // the same value, bit for bit; the general form below otherwise)
      const bool oz = !(dz.n > 0.0) || !(dz.f1 > 0.0) || !(dz.f2 > 0.0) || !(dz.g > 0.0);
      const bool os = !(ds.n > 0.0) || !(ds.f1 > 0.0) || !(ds.f2 > 0.0) || !(ds.g > 0.0);
      const bool nn = key_is_nan(umax(key4(az), key4(as)));
      const uint32_t fz_ = wave_umax(vc ? (nn ? 8u : (oz ? 1u : 0u)) : 0u), fs_ = wave_umax((vc && os) ? 1u : 0u);   // (a NaN anywhere: 8)
      if (fz_ == 1u && fs_ == 1u) {
        auto open = [&](double dv, double a) { return (dv > 0.0) ? pinf : a; };
        const double l4 = __builtin_fmin(__builtin_fmin(__builtin_fmin(open(dz.n, az.n), open(dz.f1, az.f1)), __builtin_fmin(open(dz.f2, az.f2), open(dz.g, az.g))),
                                         __builtin_fmin(__builtin_fmin(open(ds.n, as.n), open(ds.f1, as.f1)), __builtin_fmin(open(ds.f2, as.f2), open(ds.g, as.g))));
        return wave_min(vc ? l4 : pinf);
      }
    }
    const uint32_t kmz = wave_umax(vc ? key4(az) : 0u), kms = wave_umax(vc ? key4(as) : 0u);
    const double mz = wave_max(vc ? max4(az) : ninf), ms = wave_max(vc ? max4(as) : ninf);
    const double fz = key_is_nan(kmz) ? 1.0 : __builtin_fmax(mz, 1.0), fs = key_is_nan(kms) ? 1.0 : __builtin_fmax(ms, 1.0);
    auto pick = [&](double dv, double a, double fill) { return (dv > 0.0) ? fill : a; };
    const M4<double> pz = m4<double>(pick(dz.n, az.n, fz), pick(dz.f1, az.f1, fz), pick(dz.f2, az.f2, fz), pick(dz.g, az.g, fz));
    const M4<double> ps = m4<double>(pick(ds.n, as.n, fs), pick(ds.f1, as.f1, fs), pick(ds.f2, as.f2, fs), pick(ds.g, as.g, fs));
    const uint32_t kl = wave_umax(vc ? umax(key4(pz), key4(ps)) : 0u);
    const double l = wave_min(vc ? __builtin_fmin(min4(pz), min4(ps)) : pinf);
    return key_is_nan(kl) ? nan_of<double>() : l;
  };

#else
  // get_step through reciprocals (LCP_PRIMAL_RCP_STEP; see step_pair_rcp in lcp_quad_kernels.inc): with t_i = dv_i / v_i the step length
  // is -1 / min_i t_i over ALL entries wherever both vectors have a decreasing entry and no t_i is zero, NaN or infinite (the product of
  // the eight tells); any other case evaluates the exact form of lcp_device.h (step_flags / step_from_flags) - no quotient per entry
  // there either, so the kernel no longer carries the IEEE-quotient form.  The reciprocals are formed where they are used and die there
  // (v_rcp_f64 + two Newton steps: 5 instructions against the 12 of a division): this kernel lives at its register limit.
  auto step_pair_rcp = [&](const M4<double>& z, const M4<double>& dz, const M4<double>& s, const M4<double>& ds) -> double {
    const M4<double> tz = m4<double>(dz.n * fast_rcp(z.n), dz.f1 * fast_rcp(z.f1), dz.f2 * fast_rcp(z.f2), dz.g * fast_rcp(z.g));
    const M4<double> ts = m4<double>(ds.n * fast_rcp(s.n), ds.f1 * fast_rcp(s.f1), ds.f2 * fast_rcp(s.f2), ds.g * fast_rcp(s.g));
    const double mz = __builtin_fmin(__builtin_fmin(tz.n, tz.f1), __builtin_fmin(tz.f2, tz.g));
    const double ms = __builtin_fmin(__builtin_fmin(ts.n, ts.f1), __builtin_fmin(ts.f2, ts.g));
    const double prod = ((tz.n * tz.f1) * (tz.f2 * tz.g)) * ((ts.n * ts.f1) * (ts.f2 * ts.g));
    const bool bad = __builtin_amdgcn_class(prod, 0x2F7);                    // NaN, +-inf, +-0, +-denormal
    // (flags over the wave through the execution-mask compares: no reduction)
#if LCP_PRIMAL_EXP_STEP == 1
    if (false)                                                               // (experiment: the exact form always)
#elif LCP_PRIMAL_EXP_STEP == 2
    if (true)                                                                // (experiment: the fast form always - wrong on degenerate vectors)
#elif LCP_PRIMAL_EXP_STEP == 3
    if (!__any(vc && bad) && __any(vc && mz < 0.0) && __any(vc && ms < 0.0))
#else
    if (__builtin_expect(!__any(vc && bad) && __any(vc && mz < 0.0) && __any(vc && ms < 0.0), 1))
#endif
      return -fast_rcp(wave_min(vc ? __builtin_fmin(mz, ms) : inf_of<double>()));
    auto wave_or5 = [&](uint32_t w) -> uint32_t {                            // OR over the wave of a five-bit word, bit by bit
      return (__any((w & 1u) != 0u) ? 1u : 0u) | (__any((w & 2u) != 0u) ? 2u : 0u) | (__any((w & 4u) != 0u) ? 4u : 0u) | (__any((w & 8u) != 0u) ? 8u : 0u) |
             (__any((w & 16u) != 0u) ? 16u : 0u);
    };
    const uint32_t gz = wave_or5(vc ? (step_flags(tz.n) | step_flags(tz.f1) | step_flags(tz.f2) | step_flags(tz.g)) : 0u);
    const uint32_t gs = wave_or5(vc ? (step_flags(ts.n) | step_flags(ts.f1) | step_flags(ts.f2) | step_flags(ts.g)) : 0u);
    return pmin(step_from_flags(gz, wave_min(vc ? mz : inf_of<double>())), step_from_flags(gs, wave_min(vc ? ms : inf_of<double>())));
  };

#endif
  if (BWD) {
    // ---- backward: d(loss)/d(v_new) -> d(loss)/d(Mdiag, v, f, rest, fric, contact normal / arms) ----------------------------
    double x = vx ? (HOIST_IT ? wx_l : Wit[lane]) : 0.0, dx = 0, dnu = 0;
    M4<double> z = m4<double>(1, 1, 1, 1), s = z, dinv = z, ds, dl;
    if (vc) {
      if constexpr (HOIST_IT) {
        z = m4<double>(wz_l[0], wz_l[1], wz_l[2], wz_l[3]);
        s = m4<double>(ws_l[0], ws_l[1], ws_l[2], ws_l[3]);
      } else {
        z = m4<double>(Wit[ZO + lane], Wit[ZO + LX + lane], Wit[ZO + 2 * LX + lane], Wit[ZO + 3 * LX + lane]);
        s = m4<double>(Wit[ZO + 4 * LX + lane], Wit[ZO + 5 * LX + lane], Wit[ZO + 6 * LX + lane], Wit[ZO + 7 * LX + lane]);
      }
      dinv = m4<double>(s.n / z.n, s.f1 / z.f1, s.f2 / z.f2, s.g / z.g);                 // 1 / d, d = z / s (lcp.py:44)
    }
    // At a converged iterate the ratios D = s / z of the active rows underflow against Q (1e-12 and below), and Q + G^T M^-1 G
    // would lose Q.  The factorisation therefore uses D floored at BWD_FLOOR x (the row's effective inverse mass
    // j Q^-1 j^T) - a perturbation of 1e-9 of the diagonal of the contact-space matrix - and one step of iterative refinement on
    // the UNREDUCED equations (residuals formed with M, not M^-1) takes the perturbation out again: 1e-8 of the natural scale
    // |g| / min Q against the contact-space solve (tools/experiments/primal_numerics.py).  The forward needs neither: its
    // right-hand sides keep the error of the stiff directions benign (same experiment).
    constexpr double BWD_FLOOR = 1e-9;
    M4<double> dfl = dinv;
    {
      xv[lane] = vx ? 1.0 / qd : 0.0; wsync();
      double wn = 0, wt = 0;
      if (vc) {
#pragma unroll
        for (int q = 0; q < 6; ++q) { const double qi = xv[colq(q)]; wn = fma((double)jn[q] * (double)jn[q], qi, wn); wt = fma((double)jf[q] * (double)jf[q], qi, wt); }
        dfl.n = __builtin_fmax(dinv.n, BWD_FLOOR * wn);
        dfl.f1 = __builtin_fmax(dinv.f1, BWD_FLOOR * wt);
        dfl.f2 = __builtin_fmax(dinv.f2, BWD_FLOOR * wt);
      }
      wsync();
    }
    block_setup(dfl);
    factor();                                                               // lcp.py:46
    // v_new = -x (engines.py:76-77)  =>  d(loss)/dx = -d(loss)/d(v_new)
    double g = !vx ? 0.0 : (DENSE ? (double)DN.dl_dx[(size_t)scene * nz + lane] : -(double)((const float*)Gd.dl_dv)[(size_t)scene * nz + lane]);
    if ((SP.tag && *SP.tag != SP.tag_value) || broken) g = nan_of<double>();   // (another family's workspace, or a broken LCP_HINT_PINNED promise: NaN gradients instead of a misread)
    const M4<double> zero = m4<double>(0, 0, 0, 0);
    solve_kkt(dfl, g, zero, zero, 0.0, dx, ds, dl, dnu);                     // lcp.py:47-50
    {
      // residuals of  Q dx + G^T dl + A^T dnu = -g ,  G dx - M dl = 0 ,  A dx = 0  with the TRUE D
      double r1 = -g - (qd * dx + Gtw(vc ? dl.n : 0.0, vc ? dl.f1 - dl.f2 : 0.0));
      if (e > 0) r1 -= PIN ? dnu : Aty(dnu);                                  // (PIN: A^T dnu is dnu on the pinned lanes, zero elsewhere)
      if (!vx) r1 = 0.0;
      double gn, gt;
      Gv(dx, gn, gt);
      M4<double> r3 = m4<double>(-(gn - dinv.n * dl.n), -(gt - (dinv.f1 * dl.f1 + dl.g)), -(-gt - (dinv.f2 * dl.f2 + dl.g)),
                                 (mu_c * dl.n - (dl.f1 + dl.f2)) + dinv.g * dl.g);
      if (!vc) r3 = zero;
      const double r2 = (e > 0 && !PIN) ? -Av(dx) : 0.0;                      // (PIN: A dx = dx_p = 0)
      double cx, cnu;
      M4<double> cs, cl;
      solve_kkt(dfl, -r1, zero, m4<double>(-r3.n, -r3.f1, -r3.f2, -r3.g), -r2, cx, cs, cl, cnu);
      dx += cx; dnu += cnu;
      dl = m4<double>(dl.n + cl.n, dl.f1 + cl.f1, dl.f2 + cl.f2, dl.g + cl.g);
    }
    if constexpr (DENSE) {
      // ---- LCPFunction.backward (lcp.py:52-61): the outer products of (x, dx), (nu, dnu), (lam, dlam) --------------------------------
      double *X = Kl, *DX = Kl + 64, *NU = Kl + 128, *DNU = Kl + 136, *LAM = Kl + 144, *DLAM = Kl + 144 + 4 * LX;
      const int m = 4 * ncap;
      wsync();
      X[lane] = x; DX[lane] = vx ? dx : 0.0;
      if (lane < 8) { NU[lane] = (lane < e) ? Wit[64 + lane] : 0.0; DNU[lane] = 0.0; }
      wsync();
      if (ve) DNU[ya] = dnu;
      if (ci < ncap) {                                                      // dense row order: [normal | friction pairs | cone]
        LAM[ci] = z.n; LAM[ncap + 2 * ci] = z.f1; LAM[ncap + 2 * ci + 1] = z.f2; LAM[3 * ncap + ci] = z.g;
        DLAM[ci] = dl.n; DLAM[ncap + 2 * ci] = dl.f1; DLAM[ncap + 2 * ci + 1] = dl.f2; DLAM[3 * ncap + ci] = dl.g;
      }
      wsync();
      if (DN.dp) for (int j = lane; j < nz; j += 64) DN.dp[(size_t)scene * nz + j] = (float)DX[j];                            // lcp.py:52
      if (DN.dh) for (int i = lane; i < m; i += 64) DN.dh[(size_t)scene * m + i] = (float)(-DLAM[i]);                          // :56
      if (DN.db) for (int a = lane; a < e; a += 64) DN.db[(size_t)scene * e + a] = (float)(-DNU[a]);                           // :58
      if (DN.dQ) for (int i = lane; i < nz * nz; i += 64) { const int j = i / nz, k = i - j * nz;
        DN.dQ[(size_t)scene * nz * nz + i] = (float)(0.5 * (DX[j] * X[k] + X[j] * DX[k])); }                                  // :59-60
      if (DN.dA) for (int i = lane; i < e * nz; i += 64) { const int a = i / nz, k = i - a * nz;
        DN.dA[(size_t)scene * e * nz + i] = (float)(DNU[a] * X[k] + NU[a] * DX[k]); }                                         // :57
      // dG and dF - 290 of the 302 KB a pile's gradients take - leave as 16-byte stores: four consecutive entries per lane (m is a multiple
      // of four: the four entries of a dF store share their row; a dG store may straddle two rows - nz is odd - and looks each entry up)
      if (DN.dG) { float4* o4 = reinterpret_cast<float4*>(DN.dG + (size_t)scene * m * nz);
        for (int i4 = lane; i4 < (m * nz) >> 2; i4 += 64) {
          float w[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) { const int i = 4 * i4 + t, r = i / nz, k = i - r * nz; w[t] = (float)(DLAM[r] * X[k] + LAM[r] * DX[k]); }   // :53
          o4[i4] = make_float4(w[0], w[1], w[2], w[3]);
        } }
      if (DN.dF) { float4* o4 = reinterpret_cast<float4*>(DN.dF + (size_t)scene * m * m);
        const int q4 = m >> 2;
        for (int i4 = lane; i4 < m * q4; i4 += 64) { const int r = i4 / q4, c = 4 * (i4 - r * q4); const double dl_r = -DLAM[r];
          o4[i4] = make_float4((float)(dl_r * LAM[c]), (float)(dl_r * LAM[c + 1]), (float)(dl_r * LAM[c + 2]), (float)(dl_r * LAM[c + 3])); } }   // :54
      return;
    }
    // x-space vectors to LDS so that a contact lane can read the entries of its two bodies
    double* X = Kl; double* DX = Kl + LX; double* CR = Kl + 2 * LX; double* CF = Kl + 3 * LX;
    X[lane] = x; DX[lane] = dx; wsync();
    double gh_rbar = 0;
    {
      double cr = 0, cf = 0, dnx = 0, dny = 0, d1x = 0, d1y = 0, d2x = 0, d2y = 0;
      int b1 = 0, b2 = 0;
      if (vc) {
        const size_t cb = (size_t)scene * ncap + ci;
        const double nx = ((const float*)SP.c_n)[cb * 2], ny = ((const float*)SP.c_n)[cb * 2 + 1];
        const double p1x = ((const float*)SP.c_p1)[cb * 2], p1y = ((const float*)SP.c_p1)[cb * 2 + 1];
        const double p2x = ((const float*)SP.c_p2)[cb * 2], p2y = ((const float*)SP.c_p2)[cb * 2 + 1];
        b1 = SP.c_i1[cb]; b2 = SP.c_i2[cb];
        const double rbar = 0.5 * ((double)((const float*)SP.rest)[(size_t)scene * nb + b1] + (double)((const float*)SP.rest)[(size_t)scene * nb + b2]);
        const double jnd[6] = {p1x * ny - p1y * nx, nx, ny, -(p2x * ny - p2y * nx), -nx, -ny};     // world.py:177-183
        const double gh = -dl.n;                                              // dh = -dlam (lcp.py:56)
        const double af = dl.f1 - dl.f2, lf = z.f1 - z.f2;                    // Jf rows are +jt, -jt (world.py:191-192)
        double gjn[6], gjf[6], jnv = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const int col = (q < 3) ? 3 * b1 + q : 3 * b2 + (q - 3);
          const double xq = X[col], dxq = DX[col], vq = (double)vv[col];
          jnv = fma(jnd[q], vq, jnv);
          gjn[q] = dl.n * xq + z.n * dxq + gh * rbar * vq;                    // dG row n (lcp.py:53) + h = (Jc v) rbar
          gjf[q] = af * xq + lf * dxq;
        }
        gh_rbar = gh * rbar;
        cr = 0.5 * gh * jnv;                                                  // rbar = (rest_b1 + rest_b2) / 2 (world.py:144-151)
        cf = 0.5 * (-dl.g * z.n);                                             // dF[gamma_c, n_c] = -dlam_g lam_n (lcp.py:54), F = mu there
        dnx = -gjn[0] * p1y + gjn[1] + gjn[3] * p2y - gjn[4] - gjf[0] * p1x - gjf[2] + gjf[3] * p2x + gjf[5];
        dny = gjn[0] * p1x + gjn[2] - gjn[3] * p2x - gjn[5] - gjf[0] * p1y + gjf[1] + gjf[3] * p2y - gjf[4];
        d1x = gjn[0] * ny - gjf[0] * nx; d1y = -gjn[0] * nx - gjf[0] * ny;
        d2x = -gjn[3] * ny + gjf[3] * nx; d2y = gjn[3] * nx + gjf[3] * ny;
      }
      wsync();
      CR[ci] = cr; CF[ci] = cf; B12[ci] = b1; B12[LX + ci] = b2;             // (by contact: the per-body sums below run in list order)
      if (ci < ncap) {
        const size_t cb = (size_t)scene * ncap + ci;
        if (Gd.dcn) { ((float*)Gd.dcn)[cb * 2] = (float)dnx; ((float*)Gd.dcn)[cb * 2 + 1] = (float)dny; }
        if (Gd.dcp1) { ((float*)Gd.dcp1)[cb * 2] = (float)d1x; ((float*)Gd.dcp1)[cb * 2 + 1] = (float)d1y; }
        if (Gd.dcp2) { ((float*)Gd.dcp2)[cb * 2] = (float)d2x; ((float*)Gd.dcp2)[cb * 2 + 1] = (float)d2y; }
      }
    }
    const double dv_h = Gtw(gh_rbar, 0.0);                                   // Jc^T (dh rbar)
    if (vx) {
      const size_t o = (size_t)scene * nz + lane;
      const double md = (double)md_l, v = (double)vv_l;
      if (Gd.dMdiag) ((float*)Gd.dMdiag)[o] = (float)(dx * x + dx * v);      // Q = diag(M) (dQ, lcp.py:59-60) and p = M v + dt f
      if (Gd.dv) ((float*)Gd.dv)[o] = (float)(dx * md + dv_h);
      if (Gd.df) ((float*)Gd.df)[o] = (float)(dx * (double)SP.dt);
    }
    if (Gd.dJe && e > 0) {                                                    // dA = dnu (x) x + nu (x) dx (lcp.py:57; A = Je)
      float* o = (float*)Gd.dJe + (size_t)scene * e * nz;
      for (int a = 0; a < e; ++a) {
        const double dn = bcast_lane(dnu, PIN ? a : nz + a), nu = Wit[64 + a];
        if (vx) o[a * nz + lane] = (float)(dn * x + nu * dx);
      }
    }
    if (lane < nb) {                                                          // per-body sums over the contacts, fixed order
      double ar = 0, af = 0;
      for (int c = 0; c < ncs; ++c) {
        const double w = ((B12[c] == lane) ? 1.0 : 0.0) + ((B12[LX + c] == lane) ? 1.0 : 0.0);
        if (w != 0.0) { ar += w * CR[c]; af += w * CF[c]; }
      }
      if (Gd.drest) ((float*)Gd.drest)[(size_t)scene * nb + lane] = (float)ar;
      if (Gd.dfric) ((float*)Gd.dfric)[(size_t)scene * nb + lane] = (float)af;
    }
    return;
  }

  // ---- the PDIPM loop (pdipm.py:49-179) -----------------------------------------------------------------------------------
  const int max_iter = SP.max_iter, lim = SP.lim;
  const double eps = SP.eps;
  const double mf = (double)(4 * ncs);
  double x = 0, y = 0;                                                       // x on the x lanes, y on the equality lanes
  M4<double> s = m4<double>(1, 1, 1, 1), z = s, dinv = s;
  // the best iterate lives in the workspace block the backward reads (18 doubles per lane that would otherwise hold
  // registers for the whole loop): stored when an iterate improves, read back once for the outputs
  auto keep_best = [&](double x_, double y_, const M4<double>& z_, const M4<double>& s_) {
    if (vx) Wit[lane] = x_;
    if (ve) Wit[64 + ya] = y_;
    Wit[ZO + lane] = z_.n; Wit[ZO + LX + lane] = z_.f1; Wit[ZO + 2 * LX + lane] = z_.f2; Wit[ZO + 3 * LX + lane] = z_.g;
    Wit[ZO + 4 * LX + lane] = s_.n; Wit[ZO + 5 * LX + lane] = s_.f1; Wit[ZO + 6 * LX + lane] = s_.f2; Wit[ZO + 7 * LX + lane] = s_.g;
  };
  double best_resid = inf_of<double>();
  bool have_best = false, done = false;
  int n_not = 0, iters = 0;
#if LCP_PRIMAL_PEEL_INIT
  // (the initialisation pass - it = -1 - as its own copy of the loop body: LCP_Q_PEEL_INIT in lcp_quad_kernels.inc)
  auto iteration = [&](auto INIT_, const int it) LCP_INL -> bool {
    constexpr bool INIT = decltype(INIT_)::value;
    __builtin_assume(INIT == (it < 0));
#define LCP_PRIMAL_BREAK return false
#else
  for (int it = -1; it < max_iter; ++it) {
#define LCP_PRIMAL_BREAK break
#endif
    double rx = 0, ry = 0, mu = 0, resid = 0, szsum = 0;
    M4<double> rs = m4<double>(0, 0, 0, 0), rz = rs;
    if (it < 0) {                                                           // init: (p, 0, -h, -b), d = 1 (:57-63); b = 0 from a contact list (engines.py:74)
      rx = p; ry = -b_in; rz = m4<double>(-hn, 0, 0, 0); dinv = m4<double>(1, 1, 1, 1);
    } else {                                                                // residuals (:82-96)
      rx = Gtw(vc ? z.n : 0.0, vc ? z.f1 - z.f2 : 0.0) + qd * x + p;
      if (e > 0) rx += PIN ? y : Aty(y);
      if (!vx) rx = 0.0;
      rs = z;
      double gn, gt;
      Gv(x, gn, gt);
      rz = m4<double>(gn + s.n - hn, gt + s.f1 - z.g, -gt + s.f2 - z.g, s.g - (mu_c * z.n - (z.f1 + z.f2)));
      if (!vc) rz = m4<double>(0, 0, 0, 0);
      ry = (e > 0 && !PIN) ? Av(x) - b_in : 0.0;                            // (PIN: A x - b = x_p = 0)
      const double n_rx = wave_sum(rx * rx);
      const double n_rz = wave_sum(rz.n * rz.n + rz.f1 * rz.f1 + rz.f2 * rz.f2 + rz.g * rz.g);
      const double n_ry = PIN ? 0.0 : wave_sum(ry * ry);                    // (PIN: ry = x_p is identically zero)
      const double sz = wave_sum(vc ? (s.n * z.n + s.f1 * z.f1) + (s.f2 * z.f2 + s.g * z.g) : 0.0);
      szsum = sz;
      mu = sz / mf; mu = mu < 0 ? -mu : mu;                                 // (:91)
      resid = sqrt(n_rz) + sqrt(n_ry) + sqrt(n_rx) + mf * mu;               // (:92-96)
#if LCP_PRIMAL_RCP_STEP
      dinv = vc ? m4<double>(s.n * fast_rcp(z.n), s.f1 * fast_rcp(z.f1), s.f2 * fast_rcp(z.f2), s.g * fast_rcp(z.g)) : m4<double>(1, 1, 1, 1);
#else
      dinv = vc ? m4<double>(s.n / z.n, s.f1 / z.f1, s.f2 / z.f2, s.g / z.g) : m4<double>(1, 1, 1, 1);   // 1 / d, d = z / s (:98)
#endif
    }
    block_setup(dinv);
    PR_TICK(0)                                                              // residuals
    factor();                                                               // (:99-100)
    PR_TICK(2)                                                              // LU
#ifdef LCP_PRIMAL_DEBUG_DUMP
    // (round 6 root-cause aid, profiles/r06_chain_rootcause.txt: the factors and the first solve of the initialisation pass, 80 doubles per lane behind the scenes' blocks)
    double* const dbg = (double*)SP.ws + (size_t)SP.B * WsLayout::TOTAL + ((size_t)scene * 64 + lane) * 80;
    if (it < 0) {
      if constexpr (!GRID && (LCP_PRIMAL_DEBUG_DUMP & 1) != 0) { static_for<NCOL>([&](auto J) LCP_INL { dbg[J] = t[J]; }); }
      if constexpr ((LCP_PRIMAL_DEBUG_DUMP & 2) != 0) {
      dbg[56] = udinv; dbg[57] = rx; dbg[58] = ry; dbg[59] = rz.n; dbg[60] = qd; dbg[61] = p; dbg[62] = idn; dbg[63] = kap; dbg[64] = b00; dbg[65] = b10; dbg[66] = b11; }
    }
#endif
    if (it >= 0 && !done) {
      ++iters;
      if (singular && it > 0) { status |= LCP_ST_SINGULAR_T; done = true; }   // except: return best (:99-102)
      else {
        const bool improved = !have_best || (resid < best_resid);             // (:107-132)
        if (improved) { best_resid = resid; n_not = 0; have_best = true; keep_best(x, y, z, s); }
        else ++n_not;
        if (n_not == lim || best_resid < eps || mu > mu_limit<double>()) done = true;   // (:133)
      }
    }
    // (the iterate the last pass would produce is never evaluated - pdipm.py:176-179 - so its solves are skipped)
    if (it >= 0 && it == max_iter - 1) done = true;
    if (done) LCP_PRIMAL_BREAK;
    double ax = 0, ay = 0;
    M4<double> as_ = m4<double>(0, 0, 0, 0), az = as_;
    const int npass = (it < 0) ? 1 : 2;
#if LCP_PRIMAL_UNROLL_PASS
    // (the two solves of an iteration as two copies of the code, `pass` a compile-time constant - as LCP_Q_UNROLL_PASS in lcp_quad_kernels.inc)
    auto one_pass = [&](auto PASS_) LCP_INL {
      constexpr int pass = PASS_;
#else
    for (int pass = 0; pass < npass; ++pass) {
#endif
      double ox, oy;
      M4<double> os, oz;
      PR_TICK(3)
      solve_kkt(dinv, rx, rs, rz, ry, ox, os, oz, oy);
      PR_TICK(4)                                                            // solve_kkt
#ifdef LCP_PRIMAL_DEBUG_DUMP
      if ((LCP_PRIMAL_DEBUG_DUMP & 4) != 0 && it < 0) { dbg[67] = ox; dbg[68] = oy; dbg[69] = os.n; dbg[70] = os.f1; dbg[71] = os.f2; dbg[72] = os.g; dbg[73] = oz.n; dbg[74] = oz.f1; dbg[75] = oz.f2; dbg[76] = oz.g; }
#endif
      if (it < 0) {
        x = ox; s = os; z = oz; y = oy;                                     // (:60-63)
        auto min4 = [&](const M4<double>& a) { return pmin(pmin(a.n, a.f1), pmin(a.f2, a.g)); };
        const uint32_t ks = wave_umax(vc ? umax(umax(nan_key(s.n), nan_key(s.f1)), umax(nan_key(s.f2), nan_key(s.g))) : 0u);
        const uint32_t kz = wave_umax(vc ? umax(umax(nan_key(z.n), nan_key(z.f1)), umax(nan_key(z.f2), nan_key(z.g))) : 0u);
        double smin = wave_min(vc ? min4(s) : inf_of<double>()), zmin = wave_min(vc ? min4(z) : inf_of<double>());
        if (key_is_nan(ks)) smin = nan_of<double>();
        if (key_is_nan(kz)) zmin = nan_of<double>();
        if (smin <= 0.0) { const double sh = 1.0 - smin; s = m4<double>(s.n + sh, s.f1 + sh, s.f2 + sh, s.g + sh); }   // (:66-75)
        if (zmin <= 0.0) { const double sh = 1.0 - zmin; z = m4<double>(z.n + sh, z.f1 + sh, z.f2 + sh, z.g + sh); }
        if (!vc) { s = m4<double>(1, 1, 1, 1); z = s; }
        if (ncs == 0) { keep_best(x, y, z, s); done = true; }               // engines.py:36-50: x = P^-1 u, no LCP
      } else if (pass == 0) {
        ax = ox; ay = oy; as_ = os; az = oz;                                // affine direction (:138-139)
#if LCP_PRIMAL_RCP_STEP
        const double alpha = pmin(step_pair_rcp(z, az, s, as_), 1.0);
#else
        const double alpha = pmin(step_pair(z, az, s, as_), 1.0);          // (:142-144)
#endif
        auto sc = [&](double sv, double dsv, double zv, double dzv) { return (sv + alpha * dsv) * (zv + alpha * dzv); };
        const double t3 = wave_sum(vc ? (sc(s.n, as_.n, z.n, az.n) + sc(s.f1, as_.f1, z.f1, az.f1)) + (sc(s.f2, as_.f2, z.f2, az.f2) + sc(s.g, as_.g, z.g, az.g)) : 0.0);
        const double t4 = szsum;                                            // sum(s z) of this iterate: formed with the residuals (:91)
        const double r3 = t3 / t4, sig = r3 * r3 * r3;                      // (:146-150)
        const double ms = -mu * sig;
        rx = 0; ry = 0; rz = m4<double>(0, 0, 0, 0);
#if LCP_PRIMAL_RCP_STEP
        rs = vc ? m4<double>((ms + as_.n * az.n) * fast_rcp(s.n), (ms + as_.f1 * az.f1) * fast_rcp(s.f1), (ms + as_.f2 * az.f2) * fast_rcp(s.f2),
                             (ms + as_.g * az.g) * fast_rcp(s.g))
                : m4<double>(0, 0, 0, 0);
#else
        rs = vc ? m4<double>((ms + as_.n * az.n) / s.n, (ms + as_.f1 * az.f1) / s.f1, (ms + as_.f2 * az.f2) / s.f2, (ms + as_.g * az.g) / s.g)
                : m4<double>(0, 0, 0, 0);                                   // (:153)
#endif
        stash[lane] = as_.n; stash[LX + lane] = as_.f1; stash[2 * LX + lane] = as_.f2; stash[3 * LX + lane] = as_.g;
        stash[4 * LX + lane] = az.n; stash[5 * LX + lane] = az.f1; stash[6 * LX + lane] = az.f2; stash[7 * LX + lane] = az.g;
      } else {
        const double cx = ox + ax, cy = oy + ay;                            // (:160-163)
        as_ = m4<double>(stash[lane], stash[LX + lane], stash[2 * LX + lane], stash[3 * LX + lane]);
        az = m4<double>(stash[4 * LX + lane], stash[5 * LX + lane], stash[6 * LX + lane], stash[7 * LX + lane]);
        const M4<double> cs = m4<double>(os.n + as_.n, os.f1 + as_.f1, os.f2 + as_.f2, os.g + as_.g);
        const M4<double> cz = m4<double>(oz.n + az.n, oz.f1 + az.f1, oz.f2 + az.f2, oz.g + az.g);
#if LCP_PRIMAL_RCP_STEP
        const double alpha = pmin(0.999 * step_pair_rcp(z, cz, s, cs), 1.0);
#else
        const double alpha = pmin(0.999 * step_pair(z, cz, s, cs), 1.0);   // (:164-166)
#endif
        x += alpha * cx; y += alpha * cy;                                   // (:171-174)
        if (vc) {
          s = m4<double>(s.n + alpha * cs.n, s.f1 + alpha * cs.f1, s.f2 + alpha * cs.f2, s.g + alpha * cs.g);
          z = m4<double>(z.n + alpha * cz.n, z.f1 + alpha * cz.f1, z.f2 + alpha * cz.f2, z.g + alpha * cz.g);
        }
      }
      PR_TICK(5)                                                            // step lengths, update
#if LCP_PRIMAL_UNROLL_PASS
    };
    one_pass(std::integral_constant<int, 0>{});
    if (npass > 1) one_pass(std::integral_constant<int, 1>{});
#else
    }
#endif
    if (done) LCP_PRIMAL_BREAK;
#if LCP_PRIMAL_PEEL_INIT
    return true;
  };
  if (iteration(std::true_type{}, -1)) {
#pragma unroll 1
    for (int it = 0; it < max_iter; ++it) { if (!iteration(std::false_type{}, it)) break; }
  }
#else
  }
#endif
#undef LCP_PRIMAL_BREAK

  // ---- outputs (row layout of a capacity-sized LCP, padded slots 0) ---------------------------------------------------------
  if (!have_best && ncs > 0) keep_best(x, y, z, s);                         // (max_iter = 0: the initial point)
  const double bx = vx ? Wit[lane] : 0.0, by = ve ? Wit[64 + ya] : 0.0;
  const M4<double> bz = m4<double>(Wit[ZO + lane], Wit[ZO + LX + lane], Wit[ZO + 2 * LX + lane], Wit[ZO + 3 * LX + lane]);
  const M4<double> bs = m4<double>(Wit[ZO + 4 * LX + lane], Wit[ZO + 5 * LX + lane], Wit[ZO + 6 * LX + lane], Wit[ZO + 7 * LX + lane]);
  bool bad = vx && (bx != bx);
  if (vc) bad = bad || (bz.n != bz.n) || (bs.n != bs.n) || (bz.f1 != bz.f1) || (bz.f2 != bz.f2) || (bz.g != bz.g) ||
                (bs.f1 != bs.f1) || (bs.f2 != bs.f2) || (bs.g != bs.g);
  if (__any(bad)) status |= LCP_ST_NAN;
  const int m = 4 * ncap;
  if (ci < ncap) {
    const float k = vc ? 1.0f : 0.0f;
    if (SP.z) { float* o = (float*)SP.z + (size_t)scene * m; o[ci] = k * (float)bz.n; o[ncap + 2 * ci] = k * (float)bz.f1; o[ncap + 2 * ci + 1] = k * (float)bz.f2; o[3 * ncap + ci] = k * (float)bz.g; }
    if (SP.s) { float* o = (float*)SP.s + (size_t)scene * m; o[ci] = k * (float)bs.n; o[ncap + 2 * ci] = k * (float)bs.f1; o[ncap + 2 * ci + 1] = k * (float)bs.f2; o[3 * ncap + ci] = k * (float)bs.g; }
  }
  if (ve && SP.y) ((float*)SP.y)[(size_t)scene * e + ya] = (float)by;
  if (vx) {
    const double nv = DENSE ? bx : -bx;                                               // engines.py:76-77 (dense boundary: zhats = x itself, lcp.py:35)
    ((float*)SP.v_new)[(size_t)scene * nz + lane] = (float)nv;
    if (!DENSE && SP.p_new) ((float*)SP.p_new)[(size_t)scene * nz + lane] = (float)((double)((const float*)SP.pos)[(size_t)scene * nz + lane] + nv * SP.dt);   // bodies.py:81
  }
  if (lane == 0) { if (SP.iters) SP.iters[scene] = iters; if (SP.status) SP.status[scene] = status; }
#ifdef LCP_PRIMAL_PROFILE
  __builtin_amdgcn_s_waitcnt(0);
  if (lane == 0 && SP.s) { float* o = (float*)SP.s + (size_t)scene * 4 * ncap + (4 * ncap - 8); for (int i = 0; i < 7; ++i) o[i] = (float)pc[i]; }
#endif
}


