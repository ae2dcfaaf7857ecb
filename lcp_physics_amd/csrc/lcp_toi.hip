// lcp_toi.hip - continuous collision: the time of impact of body pairs along the engine's own move, and the backward of the times.
//
// include/lcp_hip.h ("time of impact") states the rule and why no iterate passes the first touch.  d(t) is the distance rule of the
// proximity queries at pose(t) = p + t (double)v, and this file follows that rule comparison by comparison:
//   circle - circle   lcp_proximity.hip:99-105 (evaluate)
//   circle - hull     hull_sd, lcp_render_common.h:103-133: h > m keeps the first edge of the largest h, d2 < d2min the first nearest
//   hull - hull       scan(), lcp_proximity.hip:54-77, and its use in evaluate(), :116-139: face when max(sep_A, sep_B) <= 0, A's face
//                     when sep_A >= sep_B; apart, A's edges first and a strict < for B's
//   the features and witnesses   lcp_proximity.hip:141-148
// What differs is where the geometry comes from.  The staged scene of lcp_render_common.h holds world vertices at ONE pose; here every
// pair looks at its two bodies at its own time, so what is staged is what does not move - kind, radius, offsets, the body-frame
// vertices (at most 16 KB), rho, p and v - and a lane turns the vertices it needs itself: one sincos per body and evaluation, world
// vertices, edges and normals formed on the fly (at()).
//
// Forward: one workgroup per scene, lane = pair, the pairs walked 256 at a time.  The validity test and the cull come before a pair's
// loop; lanes run different iteration counts, so the loop holds no workgroup barrier.  Every lane keeps the smallest (toi, pair) of
// the HIT / UNCONVERGED pairs it saw; one butterfly per wavefront and four LDS slots make first_toi / first_pair.
//
// Backward: one workgroup per scene.  Every live pair is evaluated once more, at pose(toi), and leaves its terms in LDS (104 bytes a
// pair): the force +-a = -+(g_toi / ddot) n on its two witnesses, the torque of it about either centre, and the force turned into
// either body's frame at the pair's own time.  Then every body is owned by ONE wavefront (body b by wavefront b mod 4), which walks
// the pairs in order; lane j owns vertex j of the body, the body's sums are formed alike in every lane.  No atomics, no cross-lane
// sums: two runs give the same bits whichever outputs are asked for.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_contacts_wide.h"
#include "lcp_kernels.h"

namespace lcp {
namespace toi {

constexpr int MAXB = ctw::MAXB;
constexpr int TT = 256;                    // threads per workgroup (four wavefronts)
constexpr int WAVES = TT / 64;
constexpr int MAXP = 1024;                 // pairs per scene
constexpr int T_BIT = 0x100;               // in a feature: the pair's t belongs to this edge (without it: the vertex of that index)
constexpr int MISS = 0, HIT = 1, TOUCHING = 2, UNCONVERGED = 3;

// what does not move, in LDS
struct Still {
  int* kind; int* off; int* ok;            // ok: a circle, or a hull of at least three vertices
  double *rad, *rho, *pose, *vel;          // pose, vel: [nb][3] (rot, x, y), (w, vx, vy)
  double2* vl;                             // the packed body-frame vertices
};

#define LCP_TOI_TABLES(S, dyn)                                                                                                  \
  __shared__ int s_kind[MAXB], s_off[MAXB + 1], s_ok[MAXB];                                                                     \
  __shared__ double s_rad[MAXB], s_rho[MAXB], s_pose[MAXB * 3], s_vel[MAXB * 3];                                                \
  Still S;                                                                                                                      \
  S.kind = s_kind; S.off = s_off; S.ok = s_ok; S.rad = s_rad; S.rho = s_rho; S.pose = s_pose; S.vel = s_vel;                    \
  S.vl = reinterpret_cast<double2*>(dyn)

// Stages scene `scene`; false (for the whole workgroup) when its hull vertices exceed vmax: such a scene is not queried.
__device__ __forceinline__ bool stage(const Still& S, int scene, int nb, int cap, int vmax, const int32_t* kind, const double* radius,
                                      const double* verts_local, const int32_t* nverts, const double* p, const float* v) {
  const int tid = threadIdx.x;
  const int total = ctw::stage_bodies(scene, nb, cap, kind, nverts, radius, S.kind, S.off, S.rad);
  for (int idx = tid; idx < nb * 3; idx += TT) {
    S.pose[idx] = p[(size_t)scene * nb * 3 + idx];
    S.vel[idx] = (double)v[(size_t)scene * nb * 3 + idx];
  }
  __syncthreads();
  if (total > vmax) return false;
  for (int idx = tid; idx < nb * cap; idx += TT) {
    const int b = idx / cap, k = idx - b * cap;
    const int o = S.off[b];
    if (k < S.off[b + 1] - o)                                                            // (vertex slots >= nverts are never read)
      S.vl[o + k] = *reinterpret_cast<const double2*>(verts_local + (((size_t)scene * nb + b) * cap + k) * 2);
  }
  __syncthreads();
  if (tid < nb) {
    const int o = S.off[tid], nvb = S.off[tid + 1] - o;
    const bool hull = S.kind[tid] != 0;
    double r = 0.0;
    if (hull)
      for (int k = 0; k < nvb; ++k) r = fmax(r, sqrt(S.vl[o + k].x * S.vl[o + k].x + S.vl[o + k].y * S.vl[o + k].y));
    S.rho[tid] = r;
    S.ok[tid] = !hull || nvb >= 3;
  }
  __syncthreads();
  return true;
}

// a pair of two different bodies of the scene, neither a hull of fewer than three vertices (the proximity rule's own definition)
__device__ __forceinline__ bool valid_pair(const Still& S, int nb, int k1, int k2) {
  if (k1 == k2 || k1 < 0 || k1 >= nb || k2 < 0 || k2 >= nb) return false;
  return S.ok[k1] && S.ok[k2];
}

// body k at time t
struct Body {
  bool circ; int o, nv;
  double cx, cy, sn, cs, r;
};

__device__ __forceinline__ Body at(const Still& S, int k, double t) {
  Body b;
  b.circ = S.kind[k] == 0; b.o = S.off[k]; b.nv = S.off[k + 1] - b.o; b.r = S.rad[k];
  sincos(S.pose[3 * k] + t * S.vel[3 * k], &b.sn, &b.cs);
  b.cx = S.pose[3 * k + 1] + t * S.vel[3 * k + 1];
  b.cy = S.pose[3 * k + 2] + t * S.vel[3 * k + 2];
  return b;
}

__device__ __forceinline__ double2 wv(const Still& S, const Body& b, int j) {            // utils.py:105-112
  const double2 l = S.vl[b.o + j];
  return make_double2(b.cx + (b.cs * l.x - b.sn * l.y), b.cy + (b.sn * l.x + b.cs * l.y));
}

struct Edge { double2 w, e, n; double il; };

__device__ __forceinline__ Edge edge_of(const Still& S, const Body& b, int i) {
  Edge E;
  E.w = wv(S, b, i);
  const double2 c = wv(S, b, i + 1 == b.nv ? 0 : i + 1);
  E.e = make_double2(c.x - E.w.x, c.y - E.w.y);
  E.il = 1.0 / sqrt(E.e.x * E.e.x + E.e.y * E.e.y);
  E.n = make_double2(E.e.y * E.il, -E.e.x * E.il);                                       // left_orthogonal(e) / |e|, contacts.py:229-231
  return E;
}

// hull_sd (lcp_render_common.h:103-133) of hull H at x: the selected edge only; the caller forms d, t and u from it
__device__ __forceinline__ int hull_edge(const Still& S, const Body& H, double px, double py, bool& inside) {
  double m = -1e308, d2min = 1e308;
  int im = 0, io = 0;
  for (int i = 0; i < H.nv; ++i) {
    const Edge E = edge_of(S, H, i);
    const double qx = px - E.w.x, qy = py - E.w.y;
    const double h = E.n.x * qx + E.n.y * qy;
    if (h > m) { m = h; im = i; }
    const double s = (qx * E.e.x + qy * E.e.y) * E.il * E.il;
    const double tc = fmin(fmax(s, 0.0), 1.0);
    const double rx = qx - tc * E.e.x, ry = qy - tc * E.e.y;
    const double d2 = rx * rx + ry * ry;
    if (d2 < d2min) { d2min = d2; io = i; }
  }
  inside = m <= 0.0;
  return inside ? im : io;
}

// scan() (lcp_proximity.hip:54-77): the edges of hull A against the vertices of hull V, the visit of j starting at `skew`
__device__ __forceinline__ void scan(const Still& S, const Body& A, const Body& V, int skew, double& sep, int& si, int& sj, double& d2m,
                                     int& di, int& dj) {
  const double INF = __builtin_inf();
  sep = -INF; si = 0; sj = 0; d2m = INF; di = 0; dj = 0;
  for (int i = 0; i < A.nv; ++i) {
    const Edge E = edge_of(S, A, i);
    const double il2 = E.il * E.il;
    double m = INF;
    int mj = 0, j = skew;
    for (int jj = 0; jj < V.nv; ++jj) {
      const double2 x = wv(S, V, j);
      const double qx = x.x - E.w.x, qy = x.y - E.w.y;
      const double h = E.n.x * qx + E.n.y * qy;
      if (h < m || (h == m && j < mj)) { m = h; mj = j; }
      const double s = (qx * E.e.x + qy * E.e.y) * il2;
      const double tc = fmin(fmax(s, 0.0), 1.0);
      const double rx = qx - tc * E.e.x, ry = qy - tc * E.e.y;
      const double d2 = rx * rx + ry * ry;
      if (d2 < d2m || (d2 == d2m && di == i && j < dj)) { d2m = d2; di = i; dj = j; }
      j = j + 1 == V.nv ? 0 : j + 1;
    }
    if (m > sep) { sep = m; si = i; sj = mj; }
  }
}

// What a valid pair evaluates to at time t (evaluate(), lcp_proximity.hip:94-149, without its cutoff).
struct Ev {
  int f1, f2;                              // the feature of body 1 / 2: -1 its centre, else its edge (| T_BIT: at parameter t) or vertex
  double dist, nx, ny, w1x, w1y, w2x, w2y, t;
  Body b1, b2;
};

__device__ __forceinline__ Ev evaluate(const Still& S, int k1, int k2, double time) {
  Ev Q;
  Q.b1 = at(S, k1, time); Q.b2 = at(S, k2, time);
  const Body &B1 = Q.b1, &B2 = Q.b2;
  Q.f1 = Q.f2 = -1; Q.t = 0.0;
  if (B1.circ && B2.circ) {
    const double qx = B2.cx - B1.cx, qy = B2.cy - B1.cy;
    const double len = sqrt(qx * qx + qy * qy);
    const double id = len > 0.0 ? 1.0 / len : 0.0;
    Q.dist = len - B1.r - B2.r;
    Q.nx = qx * id; Q.ny = qy * id;
    Q.w1x = B1.cx + B1.r * Q.nx; Q.w1y = B1.cy + B1.r * Q.ny;
    Q.w2x = B2.cx - B2.r * Q.nx; Q.w2y = B2.cy - B2.r * Q.ny;
    return Q;
  }
  bool edge_first, face;                                                                 // the edge is body 1's; a face (else a segment)
  int edge, pf = -1;
  double px, py, rad = 0.0;
  if (B1.circ || B2.circ) {
    const Body& C = B1.circ ? B1 : B2;
    edge_first = B2.circ;
    px = C.cx; py = C.cy; rad = C.r;
    edge = hull_edge(S, B1.circ ? B2 : B1, px, py, face);
  } else {
    const int lane = threadIdx.x & 63;
    double sa, sb, da, db;
    int sai, saj, sbj, sbi, dai, daj, dbj, dbi;
    scan(S, B1, B2, lane % B2.nv, sa, sai, saj, da, dai, daj);                           // A's edges i, B's vertices j
    scan(S, B2, B1, lane % B1.nv, sb, sbj, sbi, db, dbj, dbi);                           // B's edges j, A's vertices i
    face = fmax(sa, sb) <= 0.0;
    edge_first = face ? sa >= sb : !(db < da);                                           // (apart: A's set comes first, a strict <)
    int v;
    if (edge_first) { edge = face ? sai : dai; v = face ? saj : daj; }
    else { edge = face ? sbj : dbj; v = face ? sbi : dbi; }
    pf = v;
    const double2 x = wv(S, edge_first ? B2 : B1, v);
    px = x.x; py = x.y;
  }
  const Edge E = edge_of(S, edge_first ? B1 : B2, edge);
  const double ex = px - E.w.x, ey = py - E.w.y;
  const double s = (ex * E.e.x + ey * E.e.y) * E.il * E.il;
  const double tc = fmin(fmax(s, 0.0), 1.0);
  const double rx = ex - tc * E.e.x, ry = ey - tc * E.e.y;
  const double dout = sqrt(rx * rx + ry * ry);
  const double id = dout > 0.0 ? 1.0 / dout : 0.0;
  const double d = face ? E.n.x * ex + E.n.y * ey : dout;
  const double ux = face ? E.n.x : rx * id, uy = face ? E.n.y : ry * id;
  const double sg = edge_first ? 1.0 : -1.0;
  const double wpx = px - rad * ux, wpy = py - rad * uy, wex = px - d * ux, wey = py - d * uy;
  Q.dist = d - rad;
  Q.nx = sg * ux; Q.ny = sg * uy; Q.t = face ? s : tc;
  Q.w1x = edge_first ? wex : wpx; Q.w1y = edge_first ? wey : wpy;
  Q.w2x = edge_first ? wpx : wex; Q.w2y = edge_first ? wpy : wey;
  Q.f1 = edge_first ? (edge | T_BIT) : pf;
  Q.f2 = edge_first ? pf : (edge | T_BIT);
  return Q;
}

struct Args {
  int nb, cap, vmax, P;
  const int32_t* kind; const double* radius; const double* verts_local; const int32_t* nverts;
  const double* p; const float* v;
  const int32_t* first; const int32_t* second;
};

// the smaller of two (toi, pair), the smaller pair on ties
__device__ __forceinline__ void take_first(double& bt, int& bi, double t, int i) {
  if (t < bt || (t == bt && i < bi)) { bt = t; bi = i; }
}

__global__ void __launch_bounds__(TT) lcp_time_of_impact_kernel(Args A, const double* margin, const double* horizon, double tol,
                                                               int max_iter, double* toi, int32_t* status, double* normal,
                                                               double* first_toi, int32_t* first_pair) {
  extern __shared__ double2 s_dyn[];
  LCP_TOI_TABLES(S, s_dyn);
  __shared__ double s_bt[WAVES];
  __shared__ int s_bi[WAVES];
  const int scene = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = A.nb, P = A.P;
  const bool fits = stage(S, scene, nb, A.cap, A.vmax, A.kind, A.radius, A.verts_local, A.nverts, A.p, A.v);
  const double hz = horizon[scene];
  const bool ok = fits && hz > 0.0;                                                      // (a NaN horizon: not queried)
  const double miss = hz > 0.0 ? hz : 0.0;                                               // max(horizon, 0), 0 for a NaN
  const int NONE = 0x7fffffff;
  double bt = __builtin_inf();
  int bi = NONE;
  for (int r = tid; r < P; r += TT) {
    const size_t i = (size_t)scene * P + r;
    const int k1 = A.first[i], k2 = A.second[i];
    const double mg = margin[i];
    int st = MISS;
    double t = 0.0, te = 0.0, nx = 0.0, ny = 0.0;
    bool run = ok && valid_pair(S, nb, k1, k2);
    double dvx = 0.0, dvy = 0.0, turn = 0.0;
    if (run) {
      dvx = S.vel[3 * k2 + 1] - S.vel[3 * k1 + 1]; dvy = S.vel[3 * k2 + 2] - S.vel[3 * k1 + 2];
      turn = fabs(S.vel[3 * k1]) * S.rho[k1] + fabs(S.vel[3 * k2]) * S.rho[k2];
      // the cull: bounding circles (a circle's radius, a hull's rho) farther apart than the pair can close within the horizon.  Then
      // d(0) - margin > tol and t_1 >= horizon: the rule's own first iteration says MISS.  (The slack covers the rounding of the gap.)
      const double qx = S.pose[3 * k2 + 1] - S.pose[3 * k1 + 1], qy = S.pose[3 * k2 + 2] - S.pose[3 * k1 + 2];
      const double len = sqrt(qx * qx + qy * qy);
      const double R1 = S.kind[k1] == 0 ? S.rad[k1] : S.rho[k1], R2 = S.kind[k2] == 0 ? S.rad[k2] : S.rho[k2];
      const double gap = len - R1 - R2 - mg;
      const double slack = 1e-9 * (len + R1 + R2 + mg);
      if (gap - slack >= hz * (sqrt(dvx * dvx + dvy * dvy) + turn) && gap - slack > tol) run = false;
    }
    if (run) {
      st = UNCONVERGED;
      for (int k = 0; k < max_iter; ++k) {
        const Ev Q = evaluate(S, k1, k2, t);
        te = t;
        const double g = Q.dist - mg;
        if (g <= tol) { st = k == 0 ? TOUCHING : HIT; nx = Q.nx; ny = Q.ny; break; }
        const double a = -(Q.nx * dvx + Q.ny * dvy) + turn;
        if (!(a > 0.0)) { st = MISS; break; }
        t = te + g / a;
        if (!(t < hz)) { st = MISS; break; }
      }
    }
    const double out = st == MISS ? miss : te;                                           // (TOUCHING: te = 0)
    if (toi) toi[i] = out;
    if (status) status[i] = st;
    if (normal) { normal[2 * i] = nx; normal[2 * i + 1] = ny; }
    if (st == HIT || st == UNCONVERGED) take_first(bt, bi, out, r);
  }
  if (!first_toi && !first_pair) return;                                                 // (uniform)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) take_first(bt, bi, __shfl_xor(bt, o, 64), __shfl_xor(bi, o, 64));
  if (lane == 0) { s_bt[wave] = bt; s_bi[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w) take_first(bt, bi, s_bt[w], s_bi[w]);
    if (first_toi) first_toi[scene] = bi == NONE ? miss : bt;
    if (first_pair) first_pair[scene] = bi == NONE ? -1 : bi;
  }
}

// the per-pair terms of the backward, behind the vertices in the dynamic LDS: P slots each
struct Terms {
  double *ax, *ay, *g, *t, *toi, *rot1, *rot2, *l1x, *l1y, *l2x, *l2y;
  int *b1, *b2, *f1, *f2;                  // the two bodies (-1: no gradient) and their features
};
constexpr int TERM_DOUBLES = 11, TERM_INTS = 4;

static size_t terms_lds(int P) { return (size_t)P * (TERM_DOUBLES * sizeof(double) + TERM_INTS * sizeof(int)); }

__global__ void __launch_bounds__(TT) lcp_time_of_impact_backward_kernel(Args A, const double* toi, const int32_t* status,
                                                                        const double* g_toi, double* g_p, double* g_v, double* g_radius,
                                                                        double* g_verts_local, double* g_margin) {
  extern __shared__ double2 s_dyn[];
  LCP_TOI_TABLES(S, s_dyn);
  const int nb = A.nb, P = A.P, cap = A.cap;
  Terms T;
  T.ax = reinterpret_cast<double*>(S.vl + A.vmax); T.ay = T.ax + P; T.g = T.ay + P; T.t = T.g + P; T.toi = T.t + P;
  T.rot1 = T.toi + P; T.rot2 = T.rot1 + P; T.l1x = T.rot2 + P; T.l1y = T.l1x + P; T.l2x = T.l1y + P; T.l2y = T.l2x + P;
  T.b1 = reinterpret_cast<int*>(T.l2y + P); T.b2 = T.b1 + P; T.f1 = T.b2 + P; T.f2 = T.f1 + P;
  const int scene = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool ok = stage(S, scene, nb, cap, A.vmax, A.kind, A.radius, A.verts_local, A.nverts, A.p, A.v);
  // ---- every pair: one evaluation at pose(toi), its terms
  for (int r = tid; r < P; r += TT) {
    const size_t i = (size_t)scene * P + r;
    const int k1 = A.first[i], k2 = A.second[i];
    bool live = ok && status[i] == HIT && valid_pair(S, nb, k1, k2);
    double G = 0.0;
    T.b1[r] = -1; T.b2[r] = -1;
    if (live) {
      const double time = toi[i];
      const Ev Q = evaluate(S, k1, k2, time);
      const double r1x = Q.w1x - Q.b1.cx, r1y = Q.w1y - Q.b1.cy, r2x = Q.w2x - Q.b2.cx, r2y = Q.w2y - Q.b2.cy;
      const double w1 = S.vel[3 * k1], w2 = S.vel[3 * k2];
      // the witness points' velocities V_i = vlin_i + w_i perp(W_i - c_i), perp(x, y) = (-y, x)
      const double vx = (S.vel[3 * k2 + 1] - w2 * r2y) - (S.vel[3 * k1 + 1] - w1 * r1y);
      const double vy = (S.vel[3 * k2 + 2] + w2 * r2x) - (S.vel[3 * k1 + 2] + w1 * r1x);
      const double ddot = Q.nx * vx + Q.ny * vy;
      live = ddot < 0.0;
      if (live) {
        G = g_toi[i] / ddot;
        const double ax = -G * Q.nx, ay = -G * Q.ny;                                     // body 2 receives +a at W_2, body 1 -a at W_1
        T.ax[r] = ax; T.ay[r] = ay; T.g[r] = -G; T.t[r] = Q.t; T.toi[r] = time;
        T.rot1[r] = -(r1x * ay - r1y * ax); T.rot2[r] = r2x * ay - r2y * ax;             // dW/drot = perp(W - c)
        T.l1x[r] = -(Q.b1.cs * ax + Q.b1.sn * ay); T.l1y[r] = -(-Q.b1.sn * ax + Q.b1.cs * ay);     // R(rot + w toi)^T (-+a)
        T.l2x[r] = Q.b2.cs * ax + Q.b2.sn * ay; T.l2y[r] = -Q.b2.sn * ax + Q.b2.cs * ay;
        T.b1[r] = k1; T.b2[r] = k2; T.f1[r] = Q.f1; T.f2[r] = Q.f2;
      }
    }
    if (g_margin) g_margin[i] = G;
  }
  __syncthreads();
  // ---- every body: owned by one wavefront, the pairs in order
  for (int b = wave; b < nb; b += WAVES) {
    const bool hull = S.kind[b] != 0;
    const int nv = ok ? S.off[b + 1] - S.off[b] : 0;
    double gr = 0.0, gx = 0.0, gy = 0.0, hr = 0.0, hx = 0.0, hy = 0.0, grad = 0.0, ux = 0.0, uy = 0.0;
    for (int r0 = 0; r0 < P; r0 += 64) {
      const int rl = r0 + lane;
      unsigned long long todo = __ballot(rl < P && (T.b1[rl] == b || T.b2[rl] == b));
      while (todo) {                                                                     // (uniform: every lane walks the same pairs)
        const int r = r0 + __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const bool second = T.b2[r] == b;
        const double sg = second ? 1.0 : -1.0, time = T.toi[r];
        const double fx = sg * T.ax[r], fy = sg * T.ay[r], fr = second ? T.rot2[r] : T.rot1[r];
        gr += fr; gx += fx; gy += fy;
        hr += time * fr; hx += time * fx; hy += time * fy;
        if (!hull) { grad -= T.g[r]; continue; }
        const int f = second ? T.f2[r] : T.f1[r];
        const int edge = f & (T_BIT - 1), e1 = edge + 1 >= nv ? 0 : edge + 1;
        const double t = (f & T_BIT) ? T.t[r] : 0.0;
        const double lx = second ? T.l2x[r] : T.l1x[r], ly = second ? T.l2y[r] : T.l1y[r];
        if (lane == edge) { ux += (1.0 - t) * lx; uy += (1.0 - t) * ly; }
        if (lane == e1) { ux += t * lx; uy += t * ly; }
      }
    }
    const size_t body = (size_t)scene * nb + b;
    if (g_verts_local && lane < cap) {                                                   // (cap <= 64: one pass; slots >= nverts, circles: zeros)
      const bool mine = hull && lane < nv;
      *reinterpret_cast<double2*>(g_verts_local + (body * cap + lane) * 2) = make_double2(mine ? ux : 0.0, mine ? uy : 0.0);
    }
    if (lane == 0) {
      if (g_p) { g_p[body * 3] = gr; g_p[body * 3 + 1] = gx; g_p[body * 3 + 2] = gy; }
      if (g_v) { g_v[body * 3] = hr; g_v[body * 3 + 1] = hx; g_v[body * 3 + 2] = hy; }
      if (g_radius) g_radius[body] = hull ? 0.0 : grad;
    }
  }
}

static size_t still_lds(int vmax) { return (size_t)vmax * sizeof(double2); }

// (the static tables of either kernel take less than 8 KB; beyond 64 KB in all the dynamic part is opted in to)
static int launch(const void* fn, long long blocks, size_t lds, void* stream, void** args) {
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
  if (lds + 8 * 1024 > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return LCP_E_LAUNCH;
  if (hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(TT), args, lds, (hipStream_t)stream) != hipSuccess) return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace toi

bool time_of_impact_supported(int nb, int nvcap, int scene_verts_max, int P) {
  return render_supported(nb, nvcap, scene_verts_max) && P >= 1 && P <= toi::MAXP;
}

int time_of_impact_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                          const double* verts_local, const int32_t* nverts, const double* p, const float* v, const int32_t* pair_first,
                          const int32_t* pair_second, const double* margin, const double* horizon, double tol, int max_iter, double* toi_out,
                          int32_t* status, double* normal, double* first_toi, int32_t* first_pair, void* stream) {
  using namespace toi;
  if (!time_of_impact_supported(nb, nvcap, scene_verts_max, P)) return LCP_E_TOOLARGE;
  Args A{nb, nvcap, ctw::vmax_of(scene_verts_max), P, kind, radius, verts_local, nverts, p, v, pair_first, pair_second};
  void* args[] = {&A, &margin, &horizon, &tol, &max_iter, &toi_out, &status, &normal, &first_toi, &first_pair};
  return launch(reinterpret_cast<const void*>(lcp_time_of_impact_kernel), B, still_lds(A.vmax), stream, args);
}

int time_of_impact_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                   const double* verts_local, const int32_t* nverts, const double* p, const float* v,
                                   const int32_t* pair_first, const int32_t* pair_second, const double* toi_in, const int32_t* status,
                                   const double* g_toi, double* g_p, double* g_v, double* g_radius, double* g_verts_local, double* g_margin,
                                   void* stream) {
  using namespace toi;
  if (!time_of_impact_supported(nb, nvcap, scene_verts_max, P)) return LCP_E_TOOLARGE;
  Args A{nb, nvcap, ctw::vmax_of(scene_verts_max), P, kind, radius, verts_local, nverts, p, v, pair_first, pair_second};
  void* args[] = {&A, &toi_in, &status, &g_toi, &g_p, &g_v, &g_radius, &g_verts_local, &g_margin};
  return launch(reinterpret_cast<const void*>(lcp_time_of_impact_backward_kernel), B, still_lds(A.vmax) + terms_lds(P), stream, args);
}

}  // namespace lcp
