// lcp_primal_wg_poststab.hip - PdipmEngine.post_stabilization (engines.py:80-116) and its backward in body space beyond one
// wavefront: ONE WORKGROUP of 256 threads per scene, the fp64 system in LDS - the mapping and the machinery of lcp_primal_wg.hip on
// the frictionless LCP of lcp_primal_poststab.hip (Q = M, p = 0, G = Jc, h = (Jc v)(1 - rbar), A = Je, b = Je v, F = 0: one
// inequality row per contact, the block M is the scalar s / z).  General form only: nz + neq <= 128 pivots with neq <= 4 (41 bodies
// on a three-row floor), at most 256 contacts; the pinned form of the step kernel needs b = 0, which a moving floor breaks.
//
// Thread c = contact c, thread r < nz + neq = entry r of x / y.  Formation by ds_add_f64 wave by wave (a barrier between the
// passes: every entry receives its additions in one order on every launch and at every batch position), right-looking LU without
// pivoting with one barrier per pivot, the triangular sweeps in wave 0, scene-wide reductions per wave by DPP and combined in a
// fixed order.  Those pieces - sizes, reductions, LU, sweeps, the products with the A image - are lcp_primal_wg_common.h, shared
// with lcp_primal_wg.hip.
#include "lcp_primal_wg_common.h"

namespace lcp {
namespace pwp {

using namespace wgc;

// workspace per scene (doubles): [0] contact count | x [IT, IT + 136) | y [YO, YO + 8) | z [ncap] | s [ncap]
__host__ __device__ constexpr size_t ws_doubles(int ncap) { return wgc::ws_doubles(ncap, 2); }

template <bool BWD>
__global__ void __launch_bounds__(NT, 1) lcp_poststab_wg_kernel(StepArgs SP, StepBwdArgs Gd) {
  __shared__ __attribute__((aligned(16))) double Kl[CAP * LDK];        // the system image; backward: staging behind the solves
  __shared__ double xv[NT];                                            // x-space exchange / accumulation
  __shared__ double rv[NT];                                            // right-hand sides / solutions of the sweeps
  __shared__ float At[4 * AST];                                        // the A image: e rows of nz
  __shared__ int B12[2 * MAXC];
  __shared__ double redd[4];
  __shared__ uint32_t redu[4];

  const int scene = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  if (!BWD && scene == 0 && tid == 0 && SP.tag) *SP.tag = SP.tag_value;     // workspace trailer: which kernel family laid it out
  const int nb = SP.nb, nz = 3 * nb, ncap = SP.nc, e = SP.e;
  const int n = nz + e;                                                   // pivots
  double* const Wg = (double*)SP.ws + (size_t)scene * ws_doubles(ncap);

  // ---- scene-wide reductions: per wave by DPP, then the four wave results in a fixed order ------------------------------------
  const BlockReduce br{redd, redu, wv, lane};
  auto bsum = [&](double v) LCP_INL -> double { return br.sum(v); };
  auto bmin = [&](double v) LCP_INL -> double { return br.min(v); };
  auto bmax = [&](double v) LCP_INL -> double { return br.max(v); };
  auto bumax = [&](uint32_t v) LCP_INL -> uint32_t { return br.umax(v); };
  auto bor = [&](uint32_t v) LCP_INL -> uint32_t { return br.or_<3>(v); };          // OR of a three-bit word
  auto bany = [&](bool b) LCP_INL -> bool { return br.any(b); };

  const int lx = tid < nz ? tid : 0;
  const float md_l = ((const float*)SP.Mdiag)[(size_t)scene * nz + lx], vv_l = ((const float*)SP.v)[(size_t)scene * nz + lx];
  int ncs = ncap;
  if (BWD) ncs = (int)Wg[0];                                              // the count the forward solved with
  else if (SP.c_count) ncs = SP.c_count[scene];
  const int truncated = (ncs > ncap) ? LCP_ST_TRUNCATED : 0;
  ncs = ncs < 0 ? 0 : (ncs > ncap ? ncap : ncs);
  if (!BWD && tid == 0) Wg[0] = (double)ncs;
  const int ci = tid;
  const bool vc = ci < ncs;                                               // this thread owns a live contact
  const bool vx = tid < nz;                                               // ... an x entry,
  const bool ve = tid >= nz && tid < n;                                   // ... an equality multiplier
  const int ya = tid - nz;

  // ---- assembly (engines.py:84-91; world.py:144-183) ----------------------------------------------------------------------------
  const float* vv = (const float*)SP.v + (size_t)scene * nz;
  float jn[6] = {0, 0, 0, 0, 0, 0};
  int c0 = 0, c1 = 0;
  double hn = 0;
  for (int i = tid; i < 4 * AST; i += NT) At[i] = 0.0f;
  bsync();
  if (vc) {
    const ContactRows<float> r = make_contact<float>((const float*)SP.c_n + (size_t)scene * ncap * 2, (const float*)SP.c_p1 + (size_t)scene * ncap * 2,
                                                     (const float*)SP.c_p2 + (size_t)scene * ncap * 2, SP.c_i1 + (size_t)scene * ncap,
                                                     SP.c_i2 + (size_t)scene * ncap, (const float*)SP.rest + (size_t)scene * nb,
                                                     (const float*)SP.rest + (size_t)scene * nb, vv, ci);
#pragma unroll
    for (int q = 0; q < 6; ++q) jn[q] = r.jn[q];
    c0 = 3 * r.b1; c1 = 3 * r.b2;
    hn = (double)r.jv + (double)r.jv * -(double)r.rbar;                   // engines.py:87-89
  }
  const double qd = vx ? (double)md_l : 0.0;
  for (int i = tid; i < e * nz; i += NT) { const int a = i / nz, k = i - a * nz; At[a * AST + k] = ((const float*)SP.Je)[(size_t)scene * e * nz + i]; }
  auto colq = [&](int q) LCP_INL { return q < 3 ? c0 + q : c1 + (q - 3); };
  bsync();
  int status = truncated;
  if (bany(vx && !(qd != 0.0))) status |= LCP_ST_SINGULAR_Q;

  // ---- products ------------------------------------------------------------------------------------------------------------
  auto Gv = [&](double v) LCP_INL -> double {                                     // (Jc v)_c
    xv[tid] = vx ? v : 0.0; bsync();
    double gn = 0;
    if (vc) {
#pragma unroll
      for (int q = 0; q < 6; ++q) gn = fma((double)jn[q], xv[colq(q)], gn);
    }
    bsync();
    return gn;
  };
  auto Gtw = [&](double wn) LCP_INL -> double {                                   // (Jc^T w)_j: the waves add in turn (fixed order)
    xv[tid] = 0.0; bsync();
    for (int w = 0; w < 4; ++w) {
      if (wv == w && vc) {
#pragma unroll
        for (int q = 0; q < 6; ++q) lds_add_wg(&xv[colq(q)], (double)jn[q] * wn);
      }
      bsync();
    }
    const double r = vx ? xv[tid] : 0.0;
    bsync();
    return r;
  };
  auto Av = [&](double v) LCP_INL -> double { return wgc::Av(At, xv, v, tid, nz, vx, ve, ya); };        // equality threads <- x threads
  auto Aty = [&](double y) LCP_INL -> double { return wgc::Aty(At, xv, y, tid, nz, e, vx, ve); };      // x threads <- equality threads
  const double b_in = (e > 0) ? Av((double)vv_l) : 0.0;                   // ge = Je v (engines.py:86), on the equality threads

  // ---- formation + LU of K = [[M + Jc^T diag(z / s) Jc, A^T], [A, 0]] ---------------------------------------------------------
  double idn = 0.0;                                                       // z / s of this thread's contact (0: no contact)
  bool singular = false;
  auto factor = [&]() LCP_INL {
    for (int i = tid; i < n * LDK; i += NT) Kl[i] = 0.0;
    bsync();
    if (vx) {
      Kl[tid * LDK + tid] = qd;
      for (int a = 0; a < e; ++a) { const double av = (double)At[a * AST + tid]; Kl[tid * LDK + nz + a] = av; Kl[(nz + a) * LDK + tid] = av; }
    }
    bsync();
    for (int w = 0; w < 4; ++w) {
      if (wv == w && vc) {
#pragma unroll
        for (int pq = 0; pq < 6; ++pq) {
          double* row = Kl + colq(pq) * LDK;
          const double a = idn * (double)jn[pq];
#pragma unroll
          for (int q = 0; q < 6; ++q) lds_add_wg(row + colq(q), a * (double)jn[q]);
        }
      }
      bsync();
    }
    singular = lu_factor(Kl, n, 0, wv, lane);                             // right-looking LU, one barrier per pivot
  };
  // K^-1 w (w: entry `tid` of the right-hand side; the solution comes back the same way)
  auto ksolve = [&](double w) LCP_INL -> double {
    rv[tid] = w;
    bsync();
    if (wv == 0) lu_sweeps(Kl, rv, n, 0, lane);
    bsync();
    const double out = rv[tid];
    bsync();
    return out;
  };

  // solve_kkt (pdipm.py:325-354) in body space: q = rs / d - rz, K [dx; dy] = [-rx + Jc^T (q / D); -ry], dz = (Jc dx - q) / D
  auto solve_kkt = [&](double di, double rx, double rs, double rz, double ry, double& ox, double& os, double& oz, double& oy) LCP_INL {
    const double q = vc ? rs * di - rz : 0.0;
    const double gu = Gtw(vc ? idn * q : 0.0);
    const double sol = ksolve(vx ? (gu - rx) : (ve ? -ry : 0.0));
    ox = vx ? sol : 0.0; oy = ve ? sol : 0.0;
    const double gx = Gv(ox);
    oz = vc ? idn * (gx - q) : 0.0;
    os = vc ? (-rs - oz) * di : 0.0;                                        // :347,350
  };
  // get_step for (z, dz), (s, ds) (pdipm.py:182-186) with its NaN, zero and fill semantics, as lcp_poststab_primal_kernel's
  auto step_pair = [&](double z, double dz, double s, double ds) LCP_INL -> double {
    const double ninf = -inf_of<double>(), pinf = inf_of<double>();
    const double az = -z / dz, as = -s / ds;
    {
      // (the fill cannot be the minimum where both vectors keep an entry and nothing is NaN - same value)
      const bool nn = key_is_nan(umax(nan_key(az), nan_key(as)));
      const uint32_t f = bor(vc ? ((nn ? 1u : 0u) | (!(dz > 0.0) ? 2u : 0u) | (!(ds > 0.0) ? 4u : 0u)) : 0u);
      if (f == 6u) return bmin(vc ? __builtin_fmin((dz > 0.0) ? pinf : az, (ds > 0.0) ? pinf : as) : pinf);
    }
    const uint32_t kmz = bumax(vc ? nan_key(az) : 0u), kms = bumax(vc ? nan_key(as) : 0u);
    const double mz = bmax(vc ? az : ninf), ms = bmax(vc ? as : ninf);
    const double fz = key_is_nan(kmz) ? 1.0 : __builtin_fmax(mz, 1.0), fs = key_is_nan(kms) ? 1.0 : __builtin_fmax(ms, 1.0);
    const double pz = (dz > 0.0) ? fz : az, ps = (ds > 0.0) ? fs : as;
    const uint32_t kl = bumax(vc ? umax(nan_key(pz), nan_key(ps)) : 0u);
    const double l = bmin(vc ? __builtin_fmin(pz, ps) : pinf);
    return key_is_nan(kl) ? nan_of<double>() : l;
  };

  if (BWD) {
    // ---- backward: d(loss)/d(dp) -> d(loss)/d(Mdiag, v, rest, contact normal / arms, Je): lcp.py:37-64 on the frictionless LCP,
    // contracted through h = gc = (Jc v)(1 - rbar), b = ge = Je v, G = Jc (engines.py:84-112) ---------------------------------
    const double x = vx ? Wg[IT + tid] : 0.0;
    double z = 1, s = 1, dinv = 1;
    if (vc) { z = Wg[ZO + ci]; s = Wg[ZO + ncap + ci]; dinv = s / z; }    // 1 / d, d = z / s (lcp.py:44)
    constexpr double BWD_FLOOR = 1e-9;                                     // (floored D + one refinement step with the true D)
    double dfl = dinv;
    {
      xv[tid] = vx ? 1.0 / qd : 0.0; bsync();
      double wn = 0;
      if (vc) {
#pragma unroll
        for (int q = 0; q < 6; ++q) wn = fma((double)jn[q] * (double)jn[q], xv[colq(q)], wn);
        dfl = __builtin_fmax(dinv, BWD_FLOOR * wn);
      }
      bsync();
    }
    idn = vc ? 1.0 / dfl : 0.0;
    factor();                                                               // lcp.py:46
    double g = vx ? -(double)((const float*)Gd.dl_dv)[(size_t)scene * nz + tid] : 0.0;     // dp = -x (engines.py:115)
    if (SP.tag && *SP.tag != SP.tag_value) g = nan_of<double>();           // (another family's workspace: NaN gradients instead of a misread)
    double dx, ds, dl, dnu;
    solve_kkt(dfl, g, 0.0, 0.0, 0.0, dx, ds, dl, dnu);                      // lcp.py:47-50
    if (ncs > 0) {                                                          // refinement on the unreduced equations, true D
      double r1 = -g - (qd * dx + Gtw(vc ? dl : 0.0));
      if (e > 0) r1 -= Aty(dnu);
      if (!vx) r1 = 0.0;
      const double gx = Gv(dx);
      const double r3 = vc ? -(gx - dinv * dl) : 0.0;
      const double r2 = (e > 0) ? -Av(dx) : 0.0;
      double cx, cs, cl, cnu;
      solve_kkt(dfl, -r1, 0.0, -r3, -r2, cx, cs, cl, cnu);
      dx += cx; dnu += cnu; dl += cl;
    }
    // x-space vectors to LDS (the image is free now) so that a contact thread can read the entries of its two bodies
    double* X = Kl; double* DX = Kl + NT; double* CR = Kl + 2 * NT; double* DNU = Kl + 3 * NT;
    X[tid] = x; DX[tid] = vx ? dx : 0.0;
    if (ve) DNU[ya] = dnu;
    bsync();
    double djv = 0;
    {
      double cr = 0, dnx = 0, dny = 0, d1x = 0, d1y = 0, d2x = 0, d2y = 0;
      int b1 = 0, b2 = 0;
      if (vc) {
        const size_t cb = (size_t)scene * ncap + ci;
        const double nx = ((const float*)SP.c_n)[cb * 2], ny = ((const float*)SP.c_n)[cb * 2 + 1];
        const double p1x = ((const float*)SP.c_p1)[cb * 2], p1y = ((const float*)SP.c_p1)[cb * 2 + 1];
        const double p2x = ((const float*)SP.c_p2)[cb * 2], p2y = ((const float*)SP.c_p2)[cb * 2 + 1];
        b1 = SP.c_i1[cb]; b2 = SP.c_i2[cb];
        const double rbar = 0.5 * ((double)((const float*)SP.rest)[(size_t)scene * nb + b1] + (double)((const float*)SP.rest)[(size_t)scene * nb + b2]);
        const double jnd[6] = {p1x * ny - p1y * nx, nx, ny, -(p2x * ny - p2y * nx), -nx, -ny};     // world.py:177-183
        const double gh = -dl;                                                // dh = -dlam (lcp.py:56)
        djv = gh * (1.0 - rbar);                                              // h = (Jc v) + (Jc v) * -rbar (engines.py:89)
        double gjn[6], jnv = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const int col = (q < 3) ? 3 * b1 + q : 3 * b2 + (q - 3);
          const double xq = X[col], dxq = DX[col], vq = (double)vv[col];
          jnv = fma(jnd[q], vq, jnv);
          gjn[q] = dl * xq + z * dxq + djv * vq;                              // dG row (lcp.py:53) + h through Jc
        }
        cr = 0.5 * (-gh * jnv);                                               // rbar = (rest_b1 + rest_b2) / 2 (world.py:144-151)
        dnx = -gjn[0] * p1y + gjn[1] + gjn[3] * p2y - gjn[4];
        dny = gjn[0] * p1x + gjn[2] - gjn[3] * p2x - gjn[5];
        d1x = gjn[0] * ny; d1y = -gjn[0] * nx;
        d2x = -gjn[3] * ny; d2y = gjn[3] * nx;
      }
      CR[ci] = cr; B12[ci] = b1; B12[MAXC + ci] = b2;                        // (by contact: the per-body sums below run in list order)
      if (ci < ncap) {                                                       // (padded slots: 0)
        const size_t cb = (size_t)scene * ncap + ci;
        if (Gd.dcn) { ((float*)Gd.dcn)[cb * 2] = (float)dnx; ((float*)Gd.dcn)[cb * 2 + 1] = (float)dny; }
        if (Gd.dcp1) { ((float*)Gd.dcp1)[cb * 2] = (float)d1x; ((float*)Gd.dcp1)[cb * 2 + 1] = (float)d1y; }
        if (Gd.dcp2) { ((float*)Gd.dcp2)[cb * 2] = (float)d2x; ((float*)Gd.dcp2)[cb * 2 + 1] = (float)d2y; }
      }
    }
    // v enters through gc = (1 - rbar) Jc v and ge = Je v: dv = Jc^T djv + Je^T db, db = -dnu (lcp.py:58)
    double dv = Gtw(vc ? djv : 0.0);                                         // (its barriers publish CR / B12)
    if (e > 0) dv += Aty(ve ? -dnu : 0.0);
    if (vx) {
      const size_t o = (size_t)scene * nz + tid;
      if (Gd.dMdiag) ((float*)Gd.dMdiag)[o] = (float)(dx * x);               // Q = diag(M): dQ_jj = dx_j x_j (lcp.py:59-60); p = 0
      if (Gd.dv) ((float*)Gd.dv)[o] = (float)dv;
    }
    if (Gd.dJe && e > 0 && vx) {                                              // dA = dnu (x) x + nu (x) dx (lcp.py:57) + db (x) v
      float* o = (float*)Gd.dJe + (size_t)scene * e * nz;
      const double vl = (double)vv_l;
      for (int a = 0; a < e; ++a) { const double dn = DNU[a]; o[a * nz + tid] = (float)(dn * x + Wg[YO + a] * dx - dn * vl); }
    }
    if (tid < nb && Gd.drest) {                                               // per-body sums over the contacts, fixed order
      double ar = 0;
      for (int c = 0; c < ncs; ++c) {
        const double w = ((B12[c] == tid) ? 1.0 : 0.0) + ((B12[MAXC + c] == tid) ? 1.0 : 0.0);
        if (w != 0.0) ar += w * CR[c];
      }
      ((float*)Gd.drest)[(size_t)scene * nb + tid] = (float)ar;
    }
    return;
  }

  // ---- the PDIPM loop (pdipm.py:49-179) --------------------------------------------------------------------------------------
  const int max_iter = SP.max_iter, lim = SP.lim;
  const double eps = SP.eps;
  const double mf = (double)ncs;
  double x = 0, y = 0, s = 1, z = 1, dinv = 1;
  auto keep_best = [&](double x_, double y_, double z_, double s_) LCP_INL {
    if (vx) Wg[IT + tid] = x_;
    if (ve) Wg[YO + ya] = y_;
    if (ci < ncap) { Wg[ZO + ci] = vc ? z_ : 1.0; Wg[ZO + ncap + ci] = vc ? s_ : 1.0; }
  };
  double best_resid = inf_of<double>();
  bool have_best = false, done = false;
  int n_not = 0, iters = 0;
  for (int it = -1; it < max_iter; ++it) {
    double rx = 0, ry = 0, rs = 0, rz = 0, mu = 0, resid = 0, szsum = 0;
    if (it < 0) {                                                           // init: (p, 0, -h, -b), d = 1 (:57-63); p = 0
      rx = 0.0; ry = -b_in; rz = vc ? -hn : 0.0; dinv = 1.0;
    } else {                                                                // residuals (:82-96), F = 0
      rx = Gtw(vc ? z : 0.0) + qd * x;
      if (e > 0) rx += Aty(y);
      if (!vx) rx = 0.0;
      rs = z;
      const double gx = Gv(x);
      rz = vc ? gx + s - hn : 0.0;
      ry = (e > 0) ? Av(x) - b_in : 0.0;
      const double n_rx = bsum(rx * rx), n_rz = bsum(rz * rz), n_ry = bsum(ry * ry);
      const double sz = bsum(vc ? s * z : 0.0);
      szsum = sz;
      mu = sz / mf; mu = mu < 0 ? -mu : mu;                                 // (:91)
      resid = sqrt(n_rz) + sqrt(n_ry) + sqrt(n_rx) + mf * mu;               // (:92-96)
      dinv = vc ? s / z : 1.0;
    }
    idn = vc ? 1.0 / dinv : 0.0;
    factor();                                                               // (:99-100)
    if (it >= 0 && !done) {
      ++iters;
      if (singular && it > 0) { status |= LCP_ST_SINGULAR_T; done = true; }   // except: return best (:99-102)
      else {
        const bool improved = !have_best || (resid < best_resid);             // (:107-132; a NaN residual never improves)
        if (improved) { best_resid = resid; n_not = 0; have_best = true; keep_best(x, y, z, s); }
        else ++n_not;
        if (n_not == lim || best_resid < eps || mu > mu_limit<double>()) done = true;   // (:133)
      }
    }
    if (it >= 0 && it == max_iter - 1) done = true;                         // (the last pass's iterate is never evaluated: :176-179)
    if (done) break;
    double ax = 0, ay = 0, as_ = 0, az = 0;
    const int npass = (it < 0) ? 1 : 2;
    for (int pass = 0; pass < npass; ++pass) {
      double ox, oy, os, oz;
      solve_kkt(dinv, rx, rs, rz, ry, ox, os, oz, oy);
      if (it < 0) {
        x = ox; s = os; z = oz; y = oy;                                     // (:60-63)
        const uint32_t ks = bumax(vc ? nan_key(s) : 0u), kz = bumax(vc ? nan_key(z) : 0u);
        double smin = bmin(vc ? s : inf_of<double>()), zmin = bmin(vc ? z : inf_of<double>());
        if (key_is_nan(ks)) smin = nan_of<double>();
        if (key_is_nan(kz)) zmin = nan_of<double>();
        if (smin <= 0.0) s += 1.0 - smin;                                   // (:66-75)
        if (zmin <= 0.0) z += 1.0 - zmin;
        if (!vc) { s = 1.0; z = 1.0; }
        if (ncs == 0) { keep_best(x, y, z, s); have_best = true; done = true; }   // engines.py:92-103: the direct solve, no LCP
      } else if (pass == 0) {
        ax = ox; ay = oy; as_ = os; az = oz;                                // affine direction (:138-139)
        const double alpha = pmin(step_pair(z, az, s, as_), 1.0);          // (:142-144)
        const double t3 = bsum(vc ? (s + alpha * as_) * (z + alpha * az) : 0.0);
        const double r3 = t3 / szsum, sig = r3 * r3 * r3;                   // (:146-150)
        rx = 0; ry = 0; rz = 0;
        rs = vc ? (-mu * sig + as_ * az) / s : 0.0;                         // (:153)
      } else {
        const double cx = ox + ax, cy = oy + ay, cs = os + as_, cz = oz + az;   // (:160-163)
        const double alpha = pmin(0.999 * step_pair(z, cz, s, cs), 1.0);    // (:164-166)
        x += alpha * cx; y += alpha * cy;                                   // (:171-174)
        if (vc) { s += alpha * cs; z += alpha * cz; }
      }
    }
    if (done) break;
  }

  // ---- outputs ---------------------------------------------------------------------------------------------------------------
  if (!have_best) keep_best(0.0, 0.0, 1.0, 1.0);                            // (max_iter = 0: dp = 0, as lcp_poststab_primal_kernel)
  __threadfence_block();
  bsync();
  const double dp = vx ? -Wg[IT + tid] : 0.0;                               // engines.py:115
  if (bany(vx && (dp != dp))) status |= LCP_ST_NAN;
  if (vx) {
    ((float*)SP.v_new)[(size_t)scene * nz + tid] = (float)dp;
    if (SP.p_out64) {                                                       // world.py:110-117: dp /= 2 ; body.move(dt)
      const double dts = SP.dt_scene ? SP.dt_scene[scene] : SP.dt;
      SP.p_out64[(size_t)scene * nz + tid] = SP.pos64[(size_t)scene * nz + tid] + (dp * 0.5) * dts;
    }
  }
  if (tid == 0) { if (SP.iters) SP.iters[scene] = iters; if (SP.status) SP.status[scene] = status; }
}

}  // namespace pwp

// sizes: the general form of lcp_primal_wg.hip - at most 128 pivots (nz + neq, neq <= 4), at most 256 contacts
bool primal_wg_poststab_supported(int nz, int m, int e) {
  return m > 0 && wgc::general_form_fits(nz, m, e);
}
size_t primal_wg_poststab_ws_bytes(int m) { return sizeof(double) * pwp::ws_doubles(m / 4); }

template <bool BWD>
static int wg_poststab_launch(const StepArgs& SP, const StepBwdArgs& Gd, void* stream) {
  hipLaunchKernelGGL(pwp::lcp_poststab_wg_kernel<BWD>, dim3(SP.B), dim3(wgc::NT), 0, (hipStream_t)stream, SP, Gd);
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}
int primal_wg_post_stab(const StepArgs& SP, void* stream) { StepBwdArgs Gd = {}; return wg_poststab_launch<false>(SP, Gd, stream); }
int primal_wg_post_stab_backward(const StepArgs& SP, const StepBwdArgs& Gd, void* stream) { return wg_poststab_launch<true>(SP, Gd, stream); }

}  // namespace lcp
