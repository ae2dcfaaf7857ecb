// lcp_primal_wg.hip - the body-space PDIPM step (lcp_primal.hip has the derivation) for systems beyond one wavefront: ONE
// WORKGROUP of 256 threads (four waves) per scene, the fp64 system in LDS.  Serves up to 128 pivots (nz - 3 under LCP_HINT_PINNED:
// 43 bodies; nz + neq with neq <= 4 otherwise: 41 bodies) and up to 256 contacts - the sizes that used to fall to the contact-space
// generic kernels (lcp_generic.hip: T = 4 nc square, in HBM once it outgrows the LDS).
//
// Mapping: thread c = contact c (its compressed rows of Jc / Jt and the four inequality components of every m-space vector in
// registers, as a lane of lcp_primal_kernel); thread r < nz + neq = entry r of the x / y vectors.  The n x LDK image of the system
// lives in LDS for the whole solve:
//   * formation: Q (diagonal), A / A^T, then each contact's 6 x 6 block of G^T M^-1 G by ds_add_f64 - the four waves in four passes
//     with a barrier between them, so every entry receives its additions in the same order on every launch and at every batch
//     position (bitwise reproducible);
//   * LU without pivoting (x rows first, the equality rows last), right-looking: pivot k's row sits in registers (lane j: columns
//     k + 1 + j and k + 65 + j), wave w updates the rows k + 1 + w, k + 5 + w, ...; one barrier per pivot;
//   * the triangular sweeps run in wave 0 (two pivots per lane, the solution entries broadcast by v_readlane, no barrier per step);
//     the pinned coordinates' rows give dy_p = rhs_p - (S dx)_p afterwards;
//   * reductions over the scene: per wave by DPP, the four partial results combined in a fixed order through LDS.
// Sizes, reductions, LU, sweeps and the products with the A image are lcp_primal_wg_common.h, shared with lcp_primal_wg_poststab.hip.
// PDIPM semantics are lcp_primal_kernel's (pdipm.py:49-179): init shift, best iterate, NaN never improving, `lim` strikes, 0.999,
// step lengths through reciprocals with the exact cold path of lcp_device.h; the backward re-forms the system at the kept iterate
// with the floored D and one step of iterative refinement on the unreduced equations (lcp_primal_step.inc).
#include "lcp_primal_wg_common.h"

namespace lcp {
namespace pwg {

using namespace wgc;

constexpr int RCAP = CAP + 1;           // rows of the image (pinned form: the three pinned coordinates' rows + at most 126 pivots)
// workspace per scene (doubles): [0] contact count | x [IT, IT + 136) | y [YO, YO + 8) | z, s: 4 ncap each, component-major
__host__ __device__ constexpr size_t ws_doubles(int ncap) { return wgc::ws_doubles(ncap, 8); }

template <bool BWD>
__global__ void __launch_bounds__(NT, 1) lcp_primal_wg_kernel(StepArgs SP, StepBwdArgs Gd, int pin) {
  __shared__ __attribute__((aligned(16))) double Kl[RCAP * LDK];       // the system image; backward: staging behind the solves
  __shared__ double xv[NT];                                            // x-space exchange / accumulation
  __shared__ double rv[NT];                                            // right-hand sides / solutions of the sweeps
  __shared__ float At[4 * AST];                                        // the A image: e rows of nz
  __shared__ int B12[2 * MAXC];
  __shared__ double redd[4];
  __shared__ uint32_t redu[4];

  const int scene = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  if (!BWD && scene == 0 && tid == 0 && SP.tag) *SP.tag = SP.tag_value;     // workspace trailer: which kernel family laid it out
  const int nb = SP.nb, nz = 3 * nb, ncap = SP.nc, e = SP.e;
  const int clo = pin ? e : 0;                                            // first live column (pinned form: e == 3, checked by the launcher)
  const int n = pin ? nz - e : nz + e;                                    // pivots
  double* const Wg = (double*)SP.ws + (size_t)scene * ws_doubles(ncap);

  // ---- scene-wide reductions: per wave by DPP, then the four wave results in a fixed order ------------------------------------
  const BlockReduce br{redd, redu, wv, lane};
  auto bsum = [&](double v) LCP_INL -> double { return br.sum(v); };
  auto bmin = [&](double v) LCP_INL -> double { return br.min(v); };
  auto bumax = [&](uint32_t v) LCP_INL -> uint32_t { return br.umax(v); };
  auto bor = [&](uint32_t v) LCP_INL -> uint32_t { return br.or_<5>(v); };          // OR of a five-bit word
  auto bany = [&](bool b) LCP_INL -> bool { return br.any(b); };

  const int lx = tid < nz ? tid : 0;
  const float md_l = ((const float*)SP.Mdiag)[(size_t)scene * nz + lx], vv_l = ((const float*)SP.v)[(size_t)scene * nz + lx];
  const float ff_l = BWD ? 0.f : ((const float*)SP.f)[(size_t)scene * nz + lx];
  int ncs = ncap;
  if (BWD) ncs = (int)Wg[0];                                              // the count the forward solved with
  else if (SP.c_count) ncs = SP.c_count[scene];
  const int truncated = (ncs > ncap) ? LCP_ST_TRUNCATED : 0;
  ncs = ncs < 0 ? 0 : (ncs > ncap ? ncap : ncs);
  if (!BWD && tid == 0) Wg[0] = (double)ncs;
  const int ci = tid;
  const bool vc = ci < ncs;                                               // this thread owns a live contact
  const bool vx = tid < nz;                                               // ... an x entry,
  const bool ve = pin ? tid < e : (tid >= nz && tid < nz + e);            // ... an equality multiplier (pinned form: on the pinned coordinate)
  const bool vf = pin ? (vx && !ve) : vx;                                 // ... a free x entry
  const int ya = pin ? tid : tid - nz;

  // ---- assembly (engines.py:31-32,50-74; world.py:144-234) ----------------------------------------------------------------
  const float* vv = (const float*)SP.v + (size_t)scene * nz;
  float jn[6] = {0, 0, 0, 0, 0, 0}, jf[6] = {0, 0, 0, 0, 0, 0};
  int c0 = 0, c1 = 0;
  double mu_c = 0, hn = 0, qd = 0, p = 0;
  for (int i = tid; i < 4 * AST; i += NT) At[i] = 0.0f;
  bsync();
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
    p = (double)momentum_entry<float>(md_l, vv_l, (float)SP.dt, ff_l);    // engines.py:32
  }
  for (int i = tid; i < e * nz; i += NT) { const int a = i / nz, k = i - a * nz; At[a * AST + k] = ((const float*)SP.Je)[(size_t)scene * e * nz + i]; }
  auto colq = [&](int q) LCP_INL { return q < 3 ? c0 + q : c1 + (q - 3); };
  bsync();
  bool broken = false;                                                    // LCP_HINT_PINNED on a scene whose rows are not [I 0]
  if (pin) {
    bool okl = true;
    for (int a = 0; a < e; ++a) okl = okl && (!vx || At[a * AST + tid] == ((tid == a) ? 1.0f : 0.0f));
    broken = bany(!okl);
    if (!BWD && broken) {
      if (vx) ((float*)SP.v_new)[(size_t)scene * nz + tid] = nan_of<float>();
      if (tid == 0) { if (SP.iters) SP.iters[scene] = 0; if (SP.status) SP.status[scene] = LCP_ST_NAN; }
      return;                                                             // (uniform over the workgroup)
    }
  }
  int status = truncated;
  if (bany(vx && !(qd != 0.0))) status |= LCP_ST_SINGULAR_Q;

  // ---- products ------------------------------------------------------------------------------------------------------------
  auto Gv = [&](double v, double& gn, double& gt) LCP_INL {                       // m-space <- x-space
    xv[tid] = vx ? v : 0.0; bsync();
    gn = 0; gt = 0;
    if (vc) {
#pragma unroll
      for (int q = 0; q < 6; ++q) { const double xq = xv[colq(q)]; gn = fma((double)jn[q], xq, gn); gt = fma((double)jf[q], xq, gt); }
    }
    bsync();
  };
  auto Gtw = [&](double wn, double wt) LCP_INL -> double {                        // x-space <- m-space: the waves add in turn (fixed order)
    xv[tid] = 0.0; bsync();
    for (int w = 0; w < 4; ++w) {
      if (wv == w && vc) {
#pragma unroll
        for (int q = 0; q < 6; ++q) lds_add_wg(&xv[colq(q)], fma((double)jf[q], wt, (double)jn[q] * wn));
      }
      bsync();
    }
    const double r = vx ? xv[tid] : 0.0;
    bsync();
    return r;
  };
  auto Av = [&](double v) LCP_INL -> double { return wgc::Av(At, xv, v, tid, nz, vx, ve, ya); };        // equality threads <- x threads (unpinned form)
  auto Aty = [&](double y) LCP_INL -> double { return wgc::Aty(At, xv, y, tid, nz, e, vx, ve); };      // x threads <- equality threads (unpinned form)

  // ---- the contact's 4 x 4 block M = F_c + diag(s / z), inverted in closed form (lcp_primal_step.inc) ------------------------
  double idn = 1, i1 = 1, i2 = 1, kap = 1.0 / 3.0, b00 = 0, b10 = 0, b11 = 0;
  auto block_setup = [&](const M4<double>& D) LCP_INL {
    idn = fast_rcp(D.n); i1 = fast_rcp(D.f1); i2 = fast_rcp(D.f2);
    kap = fast_rcp(D.g + (i1 + i2));
    b00 = idn;
    b10 = kap * (i1 - i2) * (mu_c * idn);
    b11 = kap * fma(i1 + i2, D.g, 4.0 * (i1 * i2));
  };
  auto minv = [&](const M4<double>& t) LCP_INL -> M4<double> {
    M4<double> o;
    o.n = idn * t.n;
    o.g = kap * ((t.g - mu_c * o.n) + fma(i1, t.f1, i2 * t.f2));
    o.f1 = i1 * (t.f1 - o.g);
    o.f2 = i2 * (t.f2 - o.g);
    return o;
  };

  // ---- formation + LU of K = [[Q + G^T M^-1 G, A^T], [A, 0]] (pinned form: S_ff, the pinned rows formed beside it) --------------
  const int nrows = n + clo;
  bool singular = false;
  auto factor = [&]() LCP_INL {
    for (int i = tid; i < nrows * LDK; i += NT) Kl[i] = 0.0;
    bsync();
    if (pin) { if (vx && tid >= clo) Kl[tid * LDK + tid - clo] = qd; }
    else if (vx) {
      Kl[tid * LDK + tid] = qd;
      for (int a = 0; a < e; ++a) { const double av = (double)At[a * AST + tid]; Kl[tid * LDK + nz + a] = av; Kl[(nz + a) * LDK + tid] = av; }
    }
    bsync();
    double p0[6], p1[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { p0[q] = b00 * (double)jn[q]; p1[q] = fma(b10, (double)jn[q], b11 * (double)jf[q]); }
    for (int w = 0; w < 4; ++w) {
      if (wv == w && vc) {
#pragma unroll
        for (int pq = 0; pq < 6; ++pq) {
          double* row = Kl + colq(pq) * LDK - clo;
#pragma unroll
          for (int q = 0; q < 6; ++q) { if (colq(q) >= clo) lds_add_wg(row + colq(q), fma((double)jf[pq], p1[q], (double)jn[pq] * p0[q])); }
        }
      }
      bsync();
    }
    singular = lu_factor(Kl, n, clo, wv, lane);                           // right-looking LU, one barrier per pivot
  };
  // K^-1 w (w: entry `tid` of the right-hand side, coordinate layout; the solution comes back the same way)
  auto ksolve = [&](double w) LCP_INL -> double {
    rv[tid] = w;
    bsync();
    if (wv == 0) lu_sweeps(Kl, rv, n, clo, lane);
    bsync();
    double out = rv[tid];
    if (pin && tid < clo) {                                               // dy_p = rhs_p - (S dx)_p on the pinned coordinates' rows
      const double* prow = Kl + tid * LDK;
      for (int k = 0; k < n; ++k) out = fma(-prow[k], rv[k + clo], out);
    }
    bsync();
    return out;
  };

  // solve_kkt (pdipm.py:325-354) in body space; di = 1 / d
  auto solve_kkt = [&](const M4<double>& di, double rx, const M4<double>& rs, const M4<double>& rz, double ry,
                       double& ox, M4<double>& os, M4<double>& oz, double& oy) LCP_INL {
    M4<double> q = m4<double>(rs.n * di.n - rz.n, rs.f1 * di.f1 - rz.f1, rs.f2 * di.f2 - rz.f2, rs.g * di.g - rz.g);
    if (!vc) q = m4<double>(0, 0, 0, 0);
    const M4<double> u = minv(q);
    const double gu = Gtw(vc ? u.n : 0.0, vc ? u.f1 - u.f2 : 0.0);
    const double rhs = vx ? (gu - rx) : (ve ? -ry : 0.0);
    const double sol = ksolve(rhs);
    ox = vf ? sol : 0.0; oy = ve ? sol : 0.0;
    double gn, gt;
    Gv(ox, gn, gt);
    oz = minv(m4<double>(gn - q.n, gt - q.f1, -gt - q.f2, -q.g));
    if (!vc) oz = m4<double>(0, 0, 0, 0);
    os = m4<double>((-rs.n - oz.n) * di.n, (-rs.f1 - oz.f1) * di.f1, (-rs.f2 - oz.f2) * di.f2, (-rs.g - oz.g) * di.g);
    if (!vc) os = m4<double>(0, 0, 0, 0);
  };
  // get_step through reciprocals (step_pair_rcp of lcp_primal_step.inc): the fast form where both vectors decrease somewhere and no t_i
  // is zero / NaN / infinite / denormal, the exact form of lcp_device.h otherwise
  auto step_pair_rcp = [&](const M4<double>& z, const M4<double>& dz, const M4<double>& s, const M4<double>& ds) LCP_INL -> double {
    const M4<double> tz = m4<double>(dz.n * fast_rcp(z.n), dz.f1 * fast_rcp(z.f1), dz.f2 * fast_rcp(z.f2), dz.g * fast_rcp(z.g));
    const M4<double> ts = m4<double>(ds.n * fast_rcp(s.n), ds.f1 * fast_rcp(s.f1), ds.f2 * fast_rcp(s.f2), ds.g * fast_rcp(s.g));
    const double mz = __builtin_fmin(__builtin_fmin(tz.n, tz.f1), __builtin_fmin(tz.f2, tz.g));
    const double ms = __builtin_fmin(__builtin_fmin(ts.n, ts.f1), __builtin_fmin(ts.f2, ts.g));
    const double prod = ((tz.n * tz.f1) * (tz.f2 * tz.g)) * ((ts.n * ts.f1) * (ts.f2 * ts.g));
    const bool bad = __builtin_amdgcn_class(prod, 0x2F7);                    // NaN, +-inf, +-0, +-denormal
    const uint32_t fl = (vc && bad ? 1u : 0u) | (vc && mz < 0.0 ? 2u : 0u) | (vc && ms < 0.0 ? 4u : 0u);
    const uint32_t f = bor(fl);
    if (f == 6u) return -fast_rcp(bmin(vc ? __builtin_fmin(mz, ms) : inf_of<double>()));
    const uint32_t gz = bor(vc ? (step_flags(tz.n) | step_flags(tz.f1) | step_flags(tz.f2) | step_flags(tz.g)) : 0u);
    const uint32_t gs = bor(vc ? (step_flags(ts.n) | step_flags(ts.f1) | step_flags(ts.f2) | step_flags(ts.g)) : 0u);
    return pmin(step_from_flags(gz, bmin(vc ? mz : inf_of<double>())), step_from_flags(gs, bmin(vc ? ms : inf_of<double>())));
  };

  if (BWD) {
    // ---- backward: d(loss)/d(v_new) -> d(loss)/d(Mdiag, v, f, rest, fric, contact normal / arms, Je) -------------------------
    double x = vx ? Wg[IT + tid] : 0.0, dx = 0, dnu = 0;
    M4<double> z = m4<double>(1, 1, 1, 1), s = z, dinv = z, ds, dl;
    if (vc) {
      z = m4<double>(Wg[ZO + ci], Wg[ZO + ncap + ci], Wg[ZO + 2 * ncap + ci], Wg[ZO + 3 * ncap + ci]);
      s = m4<double>(Wg[ZO + 4 * ncap + ci], Wg[ZO + 5 * ncap + ci], Wg[ZO + 6 * ncap + ci], Wg[ZO + 7 * ncap + ci]);
      dinv = m4<double>(s.n / z.n, s.f1 / z.f1, s.f2 / z.f2, s.g / z.g);     // 1 / d, d = z / s (lcp.py:44)
    }
    // D floored at BWD_FLOOR x the row's effective inverse mass, one step of refinement with the true D (lcp_primal_step.inc)
    constexpr double BWD_FLOOR = 1e-9;
    M4<double> dfl = dinv;
    {
      xv[tid] = vx ? 1.0 / qd : 0.0; bsync();
      double wn = 0, wt = 0;
      if (vc) {
#pragma unroll
        for (int q = 0; q < 6; ++q) { const double qi = xv[colq(q)]; wn = fma((double)jn[q] * (double)jn[q], qi, wn); wt = fma((double)jf[q] * (double)jf[q], qi, wt); }
        dfl.n = __builtin_fmax(dinv.n, BWD_FLOOR * wn);
        dfl.f1 = __builtin_fmax(dinv.f1, BWD_FLOOR * wt);
        dfl.f2 = __builtin_fmax(dinv.f2, BWD_FLOOR * wt);
      }
      bsync();
    }
    block_setup(dfl);
    factor();                                                               // lcp.py:46
    double g = !vx ? 0.0 : -(double)((const float*)Gd.dl_dv)[(size_t)scene * nz + tid];   // v_new = -x
    if ((SP.tag && *SP.tag != SP.tag_value) || broken) g = nan_of<double>();   // (another family's workspace / a broken promise: NaN gradients)
    const M4<double> zero = m4<double>(0, 0, 0, 0);
    solve_kkt(dfl, g, zero, zero, 0.0, dx, ds, dl, dnu);                     // lcp.py:47-50
    {
      double r1 = -g - (qd * dx + Gtw(vc ? dl.n : 0.0, vc ? dl.f1 - dl.f2 : 0.0));
      if (e > 0) r1 -= pin ? dnu : Aty(dnu);
      if (!vx) r1 = 0.0;
      double gn, gt;
      Gv(dx, gn, gt);
      M4<double> r3 = m4<double>(-(gn - dinv.n * dl.n), -(gt - (dinv.f1 * dl.f1 + dl.g)), -(-gt - (dinv.f2 * dl.f2 + dl.g)),
                                 (mu_c * dl.n - (dl.f1 + dl.f2)) + dinv.g * dl.g);
      if (!vc) r3 = zero;
      const double r2 = (e > 0 && !pin) ? -Av(dx) : 0.0;
      double cx, cnu;
      M4<double> cs, cl;
      solve_kkt(dfl, -r1, zero, m4<double>(-r3.n, -r3.f1, -r3.f2, -r3.g), -r2, cx, cs, cl, cnu);
      dx += cx; dnu += cnu;
      dl = m4<double>(dl.n + cl.n, dl.f1 + cl.f1, dl.f2 + cl.f2, dl.g + cl.g);
    }
    // x-space vectors to LDS (the image is free now) so that a contact thread can read the entries of its two bodies
    double* X = Kl; double* DX = Kl + NT; double* CR = Kl + 2 * NT; double* CF = Kl + 3 * NT; double* DNU = Kl + 4 * NT;
    X[tid] = x; DX[tid] = dx;
    if (ve) DNU[ya] = dnu;
    bsync();
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
        const double af = dl.f1 - dl.f2, lf = z.f1 - z.f2;
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
        cr = 0.5 * gh * jnv;
        cf = 0.5 * (-dl.g * z.n);                                             // dF[gamma_c, n_c] = -dlam_g lam_n (lcp.py:54)
        dnx = -gjn[0] * p1y + gjn[1] + gjn[3] * p2y - gjn[4] - gjf[0] * p1x - gjf[2] + gjf[3] * p2x + gjf[5];
        dny = gjn[0] * p1x + gjn[2] - gjn[3] * p2x - gjn[5] - gjf[0] * p1y + gjf[1] + gjf[3] * p2y - gjf[4];
        d1x = gjn[0] * ny - gjf[0] * nx; d1y = -gjn[0] * nx - gjf[0] * ny;
        d2x = -gjn[3] * ny + gjf[3] * nx; d2y = gjn[3] * nx + gjf[3] * ny;
      }
      CR[ci] = cr; CF[ci] = cf; B12[ci] = b1; B12[MAXC + ci] = b2;           // (by contact: the per-body sums below run in list order)
      if (ci < ncap) {                                                       // (padded slots: 0)
        const size_t cb = (size_t)scene * ncap + ci;
        if (Gd.dcn) { ((float*)Gd.dcn)[cb * 2] = (float)dnx; ((float*)Gd.dcn)[cb * 2 + 1] = (float)dny; }
        if (Gd.dcp1) { ((float*)Gd.dcp1)[cb * 2] = (float)d1x; ((float*)Gd.dcp1)[cb * 2 + 1] = (float)d1y; }
        if (Gd.dcp2) { ((float*)Gd.dcp2)[cb * 2] = (float)d2x; ((float*)Gd.dcp2)[cb * 2 + 1] = (float)d2y; }
      }
    }
    const double dv_h = Gtw(gh_rbar, 0.0);                                   // Jc^T (dh rbar)   (its barriers publish CR / CF / B12)
    if (vx) {
      const size_t o = (size_t)scene * nz + tid;
      const double md = (double)md_l, v = (double)vv_l;
      if (Gd.dMdiag) ((float*)Gd.dMdiag)[o] = (float)(dx * x + dx * v);      // Q = diag(M) and p = M v + dt f
      if (Gd.dv) ((float*)Gd.dv)[o] = (float)(dx * md + dv_h);
      if (Gd.df) ((float*)Gd.df)[o] = (float)(dx * (double)SP.dt);
    }
    if (Gd.dJe && e > 0 && vx) {                                              // dA = dnu (x) x + nu (x) dx (lcp.py:57; A = Je)
      float* o = (float*)Gd.dJe + (size_t)scene * e * nz;
      for (int a = 0; a < e; ++a) o[a * nz + tid] = (float)(DNU[a] * x + Wg[YO + a] * dx);
    }
    if (tid < nb) {                                                           // per-body sums over the contacts, fixed order
      double ar = 0, af = 0;
      for (int c = 0; c < ncs; ++c) {
        const double w = ((B12[c] == tid) ? 1.0 : 0.0) + ((B12[MAXC + c] == tid) ? 1.0 : 0.0);
        if (w != 0.0) { ar += w * CR[c]; af += w * CF[c]; }
      }
      if (Gd.drest) ((float*)Gd.drest)[(size_t)scene * nb + tid] = (float)ar;
      if (Gd.dfric) ((float*)Gd.dfric)[(size_t)scene * nb + tid] = (float)af;
    }
    return;
  }

  // ---- the PDIPM loop (pdipm.py:49-179) --------------------------------------------------------------------------------------
  const int max_iter = SP.max_iter, lim = SP.lim;
  const double eps = SP.eps;
  const double mf = (double)(4 * ncs);
  double x = 0, y = 0;
  M4<double> s = m4<double>(1, 1, 1, 1), z = s, dinv = s, as_ = m4<double>(0, 0, 0, 0), az = as_;
  auto keep_best = [&](double x_, double y_, const M4<double>& z_, const M4<double>& s_) LCP_INL {
    if (vx) Wg[IT + tid] = x_;
    if (ve) Wg[YO + ya] = y_;
    if (ci < ncap) {
      Wg[ZO + ci] = z_.n; Wg[ZO + ncap + ci] = z_.f1; Wg[ZO + 2 * ncap + ci] = z_.f2; Wg[ZO + 3 * ncap + ci] = z_.g;
      Wg[ZO + 4 * ncap + ci] = s_.n; Wg[ZO + 5 * ncap + ci] = s_.f1; Wg[ZO + 6 * ncap + ci] = s_.f2; Wg[ZO + 7 * ncap + ci] = s_.g;
    }
  };
  double best_resid = inf_of<double>();
  bool have_best = false, done = false;
  int n_not = 0, iters = 0;
  for (int it = -1; it < max_iter; ++it) {
    double rx = 0, ry = 0, mu = 0, resid = 0, szsum = 0;
    M4<double> rs = m4<double>(0, 0, 0, 0), rz = rs;
    if (it < 0) {                                                           // init: (p, 0, -h, -b), d = 1 (:57-63); b = 0 (engines.py:74)
      rx = p; ry = 0.0; rz = m4<double>(-hn, 0, 0, 0); dinv = m4<double>(1, 1, 1, 1);
      if (!vc) rz = m4<double>(0, 0, 0, 0);
    } else {                                                                // residuals (:82-96)
      rx = Gtw(vc ? z.n : 0.0, vc ? z.f1 - z.f2 : 0.0) + qd * x + p;
      if (e > 0) rx += pin ? y : Aty(y);
      if (!vx) rx = 0.0;
      rs = z;
      double gn, gt;
      Gv(x, gn, gt);
      rz = m4<double>(gn + s.n - hn, gt + s.f1 - z.g, -gt + s.f2 - z.g, s.g - (mu_c * z.n - (z.f1 + z.f2)));
      if (!vc) rz = m4<double>(0, 0, 0, 0);
      ry = (e > 0 && !pin) ? Av(x) : 0.0;
      const double n_rx = bsum(rx * rx);
      const double n_rz = bsum(rz.n * rz.n + rz.f1 * rz.f1 + rz.f2 * rz.f2 + rz.g * rz.g);
      const double n_ry = pin ? 0.0 : bsum(ry * ry);
      const double sz = bsum(vc ? (s.n * z.n + s.f1 * z.f1) + (s.f2 * z.f2 + s.g * z.g) : 0.0);
      szsum = sz;
      mu = sz / mf; mu = mu < 0 ? -mu : mu;                                 // (:91)
      resid = sqrt(n_rz) + sqrt(n_ry) + sqrt(n_rx) + mf * mu;               // (:92-96)
      dinv = vc ? m4<double>(s.n * fast_rcp(z.n), s.f1 * fast_rcp(z.f1), s.f2 * fast_rcp(z.f2), s.g * fast_rcp(z.g)) : m4<double>(1, 1, 1, 1);
    }
    block_setup(dinv);
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
    double ax = 0, ay = 0;
    const int npass = (it < 0) ? 1 : 2;
    for (int pass = 0; pass < npass; ++pass) {
      double ox, oy;
      M4<double> os, oz;
      solve_kkt(dinv, rx, rs, rz, ry, ox, os, oz, oy);
      if (it < 0) {
        x = ox; s = os; z = oz; y = oy;                                     // (:60-63)
        auto min4 = [&](const M4<double>& a) LCP_INL { return pmin(pmin(a.n, a.f1), pmin(a.f2, a.g)); };
        const uint32_t ks = bumax(vc ? umax(umax(nan_key(s.n), nan_key(s.f1)), umax(nan_key(s.f2), nan_key(s.g))) : 0u);
        const uint32_t kz = bumax(vc ? umax(umax(nan_key(z.n), nan_key(z.f1)), umax(nan_key(z.f2), nan_key(z.g))) : 0u);
        double smin = bmin(vc ? min4(s) : inf_of<double>()), zmin = bmin(vc ? min4(z) : inf_of<double>());
        if (key_is_nan(ks)) smin = nan_of<double>();
        if (key_is_nan(kz)) zmin = nan_of<double>();
        if (smin <= 0.0) { const double sh = 1.0 - smin; s = m4<double>(s.n + sh, s.f1 + sh, s.f2 + sh, s.g + sh); }   // (:66-75)
        if (zmin <= 0.0) { const double sh = 1.0 - zmin; z = m4<double>(z.n + sh, z.f1 + sh, z.f2 + sh, z.g + sh); }
        if (!vc) { s = m4<double>(1, 1, 1, 1); z = s; }
        if (ncs == 0) { keep_best(x, y, z, s); done = true; }               // engines.py:36-50: x = P^-1 u, no LCP
      } else if (pass == 0) {
        ax = ox; ay = oy; as_ = os; az = oz;                                // affine direction (:138-139)
        const double alpha = pmin(step_pair_rcp(z, az, s, as_), 1.0);      // (:142-144)
        auto sc = [&](double sv, double dsv, double zv, double dzv) LCP_INL { return (sv + alpha * dsv) * (zv + alpha * dzv); };
        const double t3 = bsum(vc ? (sc(s.n, as_.n, z.n, az.n) + sc(s.f1, as_.f1, z.f1, az.f1)) + (sc(s.f2, as_.f2, z.f2, az.f2) + sc(s.g, as_.g, z.g, az.g)) : 0.0);
        const double r3 = t3 / szsum, sig = r3 * r3 * r3;                   // (:146-150)
        const double ms = -mu * sig;
        rx = 0; ry = 0; rz = m4<double>(0, 0, 0, 0);
        rs = vc ? m4<double>((ms + as_.n * az.n) * fast_rcp(s.n), (ms + as_.f1 * az.f1) * fast_rcp(s.f1), (ms + as_.f2 * az.f2) * fast_rcp(s.f2),
                             (ms + as_.g * az.g) * fast_rcp(s.g))
                : m4<double>(0, 0, 0, 0);                                   // (:153)
      } else {
        const double cx = ox + ax, cy = oy + ay;                            // (:160-163)
        const M4<double> cs = m4<double>(os.n + as_.n, os.f1 + as_.f1, os.f2 + as_.f2, os.g + as_.g);
        const M4<double> cz = m4<double>(oz.n + az.n, oz.f1 + az.f1, oz.f2 + az.f2, oz.g + az.g);
        const double alpha = pmin(0.999 * step_pair_rcp(z, cz, s, cs), 1.0);   // (:164-166)
        x += alpha * cx; y += alpha * cy;                                   // (:171-174)
        if (vc) {
          s = m4<double>(s.n + alpha * cs.n, s.f1 + alpha * cs.f1, s.f2 + alpha * cs.f2, s.g + alpha * cs.g);
          z = m4<double>(z.n + alpha * cz.n, z.f1 + alpha * cz.f1, z.f2 + alpha * cz.f2, z.g + alpha * cz.g);
        }
      }
    }
    if (done) break;
  }

  // ---- outputs (row layout of a capacity-sized LCP, padded slots 0) ---------------------------------------------------------
  if (!have_best && ncs > 0) keep_best(x, y, z, s);                         // (max_iter = 0: the initial point)
  __threadfence_block();
  bsync();
  const double bx = vx ? Wg[IT + tid] : 0.0, by = ve ? Wg[YO + ya] : 0.0;
  M4<double> bz = m4<double>(0, 0, 0, 0), bs = bz;
  if (ci < ncap) {
    bz = m4<double>(Wg[ZO + ci], Wg[ZO + ncap + ci], Wg[ZO + 2 * ncap + ci], Wg[ZO + 3 * ncap + ci]);
    bs = m4<double>(Wg[ZO + 4 * ncap + ci], Wg[ZO + 5 * ncap + ci], Wg[ZO + 6 * ncap + ci], Wg[ZO + 7 * ncap + ci]);
  }
  bool bad = vx && (bx != bx);
  if (vc) bad = bad || (bz.n != bz.n) || (bs.n != bs.n) || (bz.f1 != bz.f1) || (bz.f2 != bz.f2) || (bz.g != bz.g) ||
                (bs.f1 != bs.f1) || (bs.f2 != bs.f2) || (bs.g != bs.g);
  if (bany(bad)) status |= LCP_ST_NAN;
  const int m = 4 * ncap;
  if (ci < ncap) {
    const float k = vc ? 1.0f : 0.0f;
    if (SP.z) { float* o = (float*)SP.z + (size_t)scene * m; o[ci] = k * (float)bz.n; o[ncap + 2 * ci] = k * (float)bz.f1; o[ncap + 2 * ci + 1] = k * (float)bz.f2; o[3 * ncap + ci] = k * (float)bz.g; }
    if (SP.s) { float* o = (float*)SP.s + (size_t)scene * m; o[ci] = k * (float)bs.n; o[ncap + 2 * ci] = k * (float)bs.f1; o[ncap + 2 * ci + 1] = k * (float)bs.f2; o[3 * ncap + ci] = k * (float)bs.g; }
  }
  if (ve && SP.y) ((float*)SP.y)[(size_t)scene * e + ya] = (float)by;
  if (vx) {
    const double nv = -bx;                                                  // engines.py:76-77
    ((float*)SP.v_new)[(size_t)scene * nz + tid] = (float)nv;
    if (SP.p_new) ((float*)SP.p_new)[(size_t)scene * nz + tid] = (float)((double)((const float*)SP.pos)[(size_t)scene * nz + tid] + nv * SP.dt);   // bodies.py:81
  }
  if (tid == 0) { if (SP.iters) SP.iters[scene] = iters; if (SP.status) SP.status[scene] = status; }
}

}  // namespace pwg

// sizes: at most 128 pivots (pinned form: nz - 3; otherwise nz + neq with neq <= 4), at most 256 contacts
bool primal_wg_supported(int nz, int m, int e, bool pinned) {
  if (pinned && e == 3) return wgc::sizes_ok(nz, m, e) && nz - e <= wgc::CAP && nz <= pwg::RCAP;
  return wgc::general_form_fits(nz, m, e);
}
size_t primal_wg_ws_bytes(int m) { return sizeof(double) * pwg::ws_doubles(m / 4); }

template <bool BWD>
static int wg_launch(const StepArgs& SP, const StepBwdArgs& Gd, bool pinned, void* stream) {
  const int pin = (pinned && SP.e == 3) ? 1 : 0;
  hipLaunchKernelGGL(pwg::lcp_primal_wg_kernel<BWD>, dim3(SP.B), dim3(wgc::NT), 0, (hipStream_t)stream, SP, Gd, pin);
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}
int primal_wg_step(const StepArgs& SP, void* stream, bool pinned) { StepBwdArgs Gd = {}; return wg_launch<false>(SP, Gd, pinned, stream); }
int primal_wg_step_backward(const StepArgs& SP, const StepBwdArgs& Gd, void* stream, bool pinned) { return wg_launch<true>(SP, Gd, pinned, stream); }

}  // namespace lcp
