// lcp_proximity.hip - proximity queries: the signed distance between body pairs with its normal and witness points, and the backward
// of the distances.
//
// include/lcp_hip.h ("proximity queries") states the rule; this file follows it comparison by comparison.  Every pair that involves a
// hull comes down to ONE point x (a circle's centre with its radius r, or a hull's vertex with r = 0) against ONE edge i of the other
// body, either as a face (overlapping: d = n_i . (x - w_i), u = n_i, t unclamped) or as a segment (apart: d = |x - foot|, u = (x -
// foot) / d, t clamped):
//   dist = d - r,  the witness on the point's body x - r u, on the edge's body x - d u,  n = u if the edge is body 1's, else -u
//   circle - hull   hull_sd (lcp_render_common.h) at the centre
//   hull - hull     scan(): the edges of one hull against the vertices of the other, sep = max_i min_j h and the smallest squared
//                   segment distance, both with their (i, j) and the first (i, j) on ties; A's edges first, then B's
//
// Forward: one workgroup per (scene, 256 pairs), the scene staged in LDS by stage_scene; lane = pair; the validity test and the
// bounding-circle cull (wanted()) come before the pair's loops.  A lane's inner loop over the other hull's vertices starts at vertex
// (lane mod nv) and wraps: the lanes of a wavefront read different bodies at the same step, and bodies of 16 vertices lie 256 bytes
// apart, which is every LDS bank again - the rotation spreads a 16-lane group of a 16-byte read over all 64 banks.  Ties are broken
// by the index, not by the order of the visit, so the rotation changes no result.
//
// Backward: one workgroup per scene.  Every pair is recomputed (the same function) and leaves in LDS g n, g, t, its two bodies and the
// feature of either (48 bytes a pair).  With d(dist) = n . (dW2 - dW1) - dr1 - dr2, body 2 receives +g n and body 1 -g n at its
// witness: a circle at its centre (and -g for its radius), a hull (1 - t) and t of it at the two world vertices of the edge (a
// vertex: all of it there).  Then every body is owned by ONE wavefront (body b by wavefront b mod 4), which walks the pairs in order,
// 64 at a time, exactly as lcp_sensors.hip walks the rays: per-lane sums in pair order, the hull's vertices through an LDS accumulator
// of the wavefront, one butterfly per output.  No atomics: two runs give the same bits.
#include "lcp_render_common.h"

namespace lcp {
namespace proximity {

using render::MAXB;
using render::RD_T;
using render::RD_WAVES;
using render::Scene;
using render::wave_sum;

constexpr int MAXP = 1024;                 // pairs per scene
constexpr int T_BIT = 0x100;               // in a feature: the pair's t belongs to this edge (without it: the edge's first vertex)

struct Pairs {
  int P;
  const int32_t* first; const int32_t* second; const double* max_dist;
};

// What a pair evaluates to.  live = false: invalid, culled or clamped - dist = max_dist, everything else 0, no gradient.
struct Prox {
  bool live;
  int f1, f2;                              // the feature of body 1 / 2: -1 its centre, else its edge (| T_BIT: at parameter t)
  double dist, nx, ny, w1x, w1y, w2x, w2y, t;
};

// The edges of hull [oe, oe + ne) against the vertices of hull [ov, ov + nv): sep = max_i min_j n_i . (v_j - w_i) with its (i, j),
// the first i on ties of the max and the first j on ties of the min; and the smallest squared point-to-segment distance with its
// (i, j), the first in the order (i outer, j inner).  The visit of j starts at `skew` and wraps.
__device__ __forceinline__ void scan(const Scene& S, int oe, int ne, int ov, int nv, int skew, double& sep, int& si, int& sj,
                                     double& d2m, int& di, int& dj) {
  const double INF = __builtin_inf();
  sep = -INF; si = 0; sj = 0; d2m = INF; di = 0; dj = 0;
  for (int i = 0; i < ne; ++i) {
    const double2 vw = S.vw[oe + i], ve = S.ve[oe + i], vn = S.vn[oe + i];
    const double il = S.vil[oe + i], il2 = il * il;
    double m = INF;
    int mj = 0, j = skew;
    for (int jj = 0; jj < nv; ++jj) {
      const double2 x = S.vw[ov + j];
      const double qx = x.x - vw.x, qy = x.y - vw.y;
      const double h = vn.x * qx + vn.y * qy;
      if (h < m || (h == m && j < mj)) { m = h; mj = j; }
      const double s = (qx * ve.x + qy * ve.y) * il2;
      const double tc = fmin(fmax(s, 0.0), 1.0);
      const double rx = qx - tc * ve.x, ry = qy - tc * ve.y;
      const double d2 = rx * rx + ry * ry;
      if (d2 < d2m || (d2 == d2m && di == i && j < dj)) { d2m = d2; di = i; dj = j; }
      j = j + 1 == nv ? 0 : j + 1;
    }
    if (m > sep) { sep = m; si = i; sj = mj; }
  }
}

// Whether a pair is evaluated at all (ok: the scene is queried): a pair of two different bodies of the scene, neither a hull of fewer
// than three vertices, whose bounding circles are less than md apart (the cull: beyond it the true distance is >= md too).
__device__ __forceinline__ bool wanted(const Scene& S, int nb, bool ok, int k1, int k2, double md) {
  if (!ok || k1 == k2 || k1 < 0 || k1 >= nb || k2 < 0 || k2 >= nb) return false;
  const double reach1 = S.reach[k1], reach2 = S.reach[k2];
  if (reach1 < 0.0 || reach2 < 0.0) return false;
  const double qx = S.cx[k2] - S.cx[k1], qy = S.cy[k2] - S.cy[k1];
  return !(sqrt(qx * qx + qy * qy) - reach1 - reach2 >= md);
}

// The rule of the header for one pair against the staged scene (ok: the scene is queried at all).
__device__ __forceinline__ Prox evaluate(const Scene& S, int nb, bool ok, int k1, int k2, double md) {
  Prox R;
  R.live = false; R.f1 = R.f2 = -1; R.dist = md; R.nx = R.ny = R.w1x = R.w1y = R.w2x = R.w2y = R.t = 0.0;
  if (!wanted(S, nb, ok, k1, k2, md)) return R;
  const double c1x = S.cx[k1], c1y = S.cy[k1], c2x = S.cx[k2], c2y = S.cy[k2];
  const double qx = c2x - c1x, qy = c2y - c1y;
  const double len = sqrt(qx * qx + qy * qy);
  const bool circ1 = S.kind[k1] == 0, circ2 = S.kind[k2] == 0;
  Prox Q = R;
  if (circ1 && circ2) {
    const double r1 = S.rad[k1], r2 = S.rad[k2];
    const double id = len > 0.0 ? 1.0 / len : 0.0;
    Q.dist = len - r1 - r2;
    Q.nx = qx * id; Q.ny = qy * id;
    Q.w1x = c1x + r1 * Q.nx; Q.w1y = c1y + r1 * Q.ny;
    Q.w2x = c2x - r2 * Q.nx; Q.w2y = c2y - r2 * Q.ny;
  } else {
    bool edge_first;                                                                     // the edge is body 1's
    int edge, pf = -1;                                                                   // the edge (in its hull), the point's feature
    double px, py, rad = 0.0, d, t, ux, uy;
    if (circ1 || circ2) {
      const int kh = circ1 ? k2 : k1, kc = circ1 ? k1 : k2;
      edge_first = circ2;
      px = S.cx[kc]; py = S.cy[kc]; rad = S.rad[kc];
      d = render::hull_sd(S, S.off[kh], S.off[kh + 1] - S.off[kh], px, py, edge, t, ux, uy);
    } else {
      const int oa = S.off[k1], na = S.off[k1 + 1] - oa, ob = S.off[k2], nbv = S.off[k2 + 1] - ob;
      const int lane = threadIdx.x & 63;
      double sa, sb, da, db;
      int sai, saj, sbj, sbi, dai, daj, dbj, dbi;
      scan(S, oa, na, ob, nbv, lane % nbv, sa, sai, saj, da, dai, daj);                  // A's edges i, B's vertices j
      scan(S, ob, nbv, oa, na, lane % na, sb, sbj, sbi, db, dbj, dbi);                   // B's edges j, A's vertices i
      const bool face = fmax(sa, sb) <= 0.0;
      edge_first = face ? sa >= sb : !(db < da);                                         // (apart: A's set comes first, a strict <)
      int oe, ov, v;
      if (edge_first) { oe = oa; ov = ob; edge = face ? sai : dai; v = face ? saj : daj; }
      else { oe = ob; ov = oa; edge = face ? sbj : dbj; v = face ? sbi : dbi; }
      pf = v;
      px = S.vw[ov + v].x; py = S.vw[ov + v].y;
      const double2 vw = S.vw[oe + edge], ve = S.ve[oe + edge], vn = S.vn[oe + edge];
      const double il = S.vil[oe + edge];
      const double ex = px - vw.x, ey = py - vw.y;
      const double s = (ex * ve.x + ey * ve.y) * il * il;
      const double tc = fmin(fmax(s, 0.0), 1.0);
      const double rx = ex - tc * ve.x, ry = ey - tc * ve.y;
      const double dout = sqrt(rx * rx + ry * ry);
      const double id = dout > 0.0 ? 1.0 / dout : 0.0;
      d = face ? vn.x * ex + vn.y * ey : dout;
      t = face ? s : tc;
      ux = face ? vn.x : rx * id; uy = face ? vn.y : ry * id;
    }
    const double sg = edge_first ? 1.0 : -1.0;
    const double wpx = px - rad * ux, wpy = py - rad * uy, wex = px - d * ux, wey = py - d * uy;
    Q.dist = d - rad;
    Q.nx = sg * ux; Q.ny = sg * uy; Q.t = t;
    Q.w1x = edge_first ? wex : wpx; Q.w1y = edge_first ? wey : wpy;
    Q.w2x = edge_first ? wpx : wex; Q.w2y = edge_first ? wpy : wey;
    Q.f1 = edge_first ? (edge | T_BIT) : pf;
    Q.f2 = edge_first ? pf : (edge | T_BIT);
  }
  if (!(Q.dist < md)) return R;                                                          // the clamp
  Q.live = true;
  return Q;
}

__global__ void __launch_bounds__(RD_T) lcp_pair_distance_kernel(int nb, int cap, int vmax, int chunks, Pairs pairs, const int32_t* kind,
                                                                const double* radius, const double* verts_local, const int32_t* nverts,
                                                                const double* p, double* dist, double* normal, double* w1, double* w2) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  const int scene = blockIdx.x / chunks, chunk = blockIdx.x - scene * chunks;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  const int r = chunk * RD_T + threadIdx.x;
  if (r >= pairs.P) return;
  const size_t i = (size_t)scene * pairs.P + r;
  const Prox Q = evaluate(S, nb, ok, pairs.first[i], pairs.second[i], pairs.max_dist[i]);
  if (dist) dist[i] = Q.dist;
  if (normal) { normal[2 * i] = Q.nx; normal[2 * i + 1] = Q.ny; }
  if (w1) { w1[2 * i] = Q.w1x; w1[2 * i + 1] = Q.w1y; }
  if (w2) { w2[2 * i] = Q.w2x; w2[2 * i + 1] = Q.w2y; }
}

// the per-pair terms of the backward, behind the scene's arrays in the dynamic LDS: P slots each
struct Terms {
  double *ax, *ay, *g, *t;                 // g n, g, the edge parameter
  int *b1, *b2, *f1, *f2;                  // the two bodies (-1: no gradient) and their features
};

static size_t terms_lds(int P) { return (size_t)P * (4 * sizeof(double) + 4 * sizeof(int)); }

__global__ void __launch_bounds__(RD_T) lcp_pair_distance_backward_kernel(int nb, int cap, int vmax, Pairs pairs, const int32_t* kind,
                                                                         const double* radius, const double* verts_local,
                                                                         const int32_t* nverts, const double* p, const double* g_dist,
                                                                         double* g_p, double* g_radius, double* g_verts_local) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  __shared__ double2 s_acc[RD_WAVES][ctw::NV];             // per wavefront: the gradient of each world vertex of the body it owns
  const int P = pairs.P;
  Terms T;
  T.ax = S.vil + vmax; T.ay = T.ax + P; T.g = T.ay + P; T.t = T.g + P;
  T.b1 = reinterpret_cast<int*>(T.t + P); T.b2 = T.b1 + P; T.f1 = T.b2 + P; T.f2 = T.f1 + P;
  const int scene = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  // ---- every pair: its features again, its terms
  for (int r = tid; r < P; r += RD_T) {
    const size_t i = (size_t)scene * P + r;
    const int k1 = pairs.first[i], k2 = pairs.second[i];
    const Prox Q = evaluate(S, nb, ok, k1, k2, pairs.max_dist[i]);
    const double g = Q.live ? g_dist[i] : 0.0;
    T.ax[r] = g * Q.nx; T.ay[r] = g * Q.ny; T.g[r] = g; T.t[r] = Q.t;
    T.b1[r] = Q.live ? k1 : -1; T.b2[r] = Q.live ? k2 : -1; T.f1[r] = Q.f1; T.f2[r] = Q.f2;
  }
  __syncthreads();
  // ---- every body: owned by one wavefront, the pairs in order
  for (int b = wave; b < nb; b += RD_WAVES) {
    const bool hull = S.kind[b] != 0;
    const int o = S.off[b], nv = ok ? S.off[b + 1] - o : 0;               // (a scene that is not queried has no staged vertices)
    s_acc[wave][lane] = make_double2(0.0, 0.0);            // (ctw::NV = 64: one slot per lane, the wavefront's own)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double gx = 0.0, gy = 0.0, grot = 0.0, grad = 0.0;
    for (int r0 = 0; r0 < P; r0 += 64) {
      const int r = r0 + lane;
      const bool valid = r < P;
      const bool second = valid && T.b2[r] == b, mine = second || (valid && T.b1[r] == b);
      if (!__any(mine)) continue;
      const double sg = second ? 1.0 : -1.0;               // body 2 receives +g n, body 1 -g n
      const double ax = mine ? sg * T.ax[r] : 0.0, ay = mine ? sg * T.ay[r] : 0.0;
      if (!hull) {
        if (mine) { gx += ax; gy += ay; grad -= T.g[r]; }
      } else {
        const int f = mine ? (second ? T.f2[r] : T.f1[r]) : 0;
        const int edge = mine ? (f & (T_BIT - 1)) : -1;
        const double t = mine && (f & T_BIT) ? T.t[r] : 0.0;
        // the lane's rank among the lanes whose witness lies on the same edge, and the largest such group: lanes of one rank hold
        // pairwise different edges, so they add without meeting - rank by rank, the edge's first vertex, then its second
        int rank = 0, depth = 0;
        unsigned long long todo = __ballot(mine);
        while (todo) {
          const int e = __shfl(edge, __ffsll((long long)todo) - 1, 64);
          const bool same = mine && edge == e;
          const unsigned long long m = __ballot(same);
          if (same) rank = __popcll(m & ((1ull << lane) - 1));
          depth = max(depth, (int)__popcll(m));
          todo &= ~m;
        }
        const int e1 = edge + 1 >= nv ? 0 : edge + 1;
        for (int j = 0; j < depth; ++j) {
          if (mine && rank == j) {
            double2 u = s_acc[wave][edge];
            u.x += (1.0 - t) * ax; u.y += (1.0 - t) * ay;
            s_acc[wave][edge] = u;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (mine && rank == j) {
            double2 v = s_acc[wave][e1];
            v.x += t * ax; v.y += t * ay;
            s_acc[wave][e1] = v;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
      }
    }
    // the world-vertex gradients turned back into the body frame, and what they give the pose
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < cap) {                                      // (cap <= 64: one pass)
      double wx = 0.0, wy = 0.0;
      if (hull && lane < nv) {
        wx = s_acc[wave][lane].x; wy = s_acc[wave][lane].y;
        const double rx = S.vw[o + lane].x - S.cx[b], ry = S.vw[o + lane].y - S.cy[b];
        gx += wx; gy += wy; grot += wy * rx - wx * ry;     // dw/drot = left turn of (w - c)
      }
      if (g_verts_local) {
        const double sn = S.sn[b], cs = S.cs[b];
        double2 out = make_double2(cs * wx + sn * wy, -sn * wx + cs * wy);      // (slots >= nverts, circles: zeros)
        *reinterpret_cast<double2*>(g_verts_local + (((size_t)scene * nb + b) * cap + lane) * 2) = out;
      }
    }
    const double sr = wave_sum(grot), sx = wave_sum(gx), sy = wave_sum(gy), sa = wave_sum(grad);
    if (lane == 0) {
      const size_t body = (size_t)scene * nb + b;
      if (g_p) { g_p[body * 3] = sr; g_p[body * 3 + 1] = sx; g_p[body * 3 + 2] = sy; }
      if (g_radius) g_radius[body] = hull ? 0.0 : sa;
    }
  }
}

// (the static tables of either kernel take less than 12 KB; beyond 64 KB in all the dynamic part is opted in to)
static int launch(const void* fn, long long blocks, size_t lds, void* stream, void** args) {
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
  if (lds + 12 * 1024 > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return LCP_E_LAUNCH;
  if (hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(RD_T), args, lds, (hipStream_t)stream) != hipSuccess) return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace proximity

bool pair_distance_supported(int nb, int nvcap, int scene_verts_max, int P) {
  return render_supported(nb, nvcap, scene_verts_max) && P >= 1 && P <= proximity::MAXP;
}

int pair_distance_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                         const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                         const int32_t* pair_second, const double* pair_max_dist, double* dist, double* normal, double* w1, double* w2,
                         void* stream) {
  using namespace proximity;
  if (!pair_distance_supported(nb, nvcap, scene_verts_max, P)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  int chunks = (P + RD_T - 1) / RD_T;
  Pairs pairs{P, pair_first, pair_second, pair_max_dist};
  void* args[] = {&nb, &nvcap, &vmax, &chunks, &pairs, &kind, &radius, &verts_local, &nverts, &p, &dist, &normal, &w1, &w2};
  return launch(reinterpret_cast<const void*>(lcp_pair_distance_kernel), (long long)B * chunks, render::scene_lds(vmax), stream, args);
}

int pair_distance_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                  const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                                  const int32_t* pair_second, const double* pair_max_dist, const double* g_dist, double* g_p,
                                  double* g_radius, double* g_verts_local, void* stream) {
  using namespace proximity;
  if (!pair_distance_supported(nb, nvcap, scene_verts_max, P)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  Pairs pairs{P, pair_first, pair_second, pair_max_dist};
  void* args[] = {&nb, &nvcap, &vmax, &pairs, &kind, &radius, &verts_local, &nverts, &p, &g_dist, &g_p, &g_radius, &g_verts_local};
  return launch(reinterpret_cast<const void*>(lcp_pair_distance_backward_kernel), B, render::scene_lds(vmax) + terms_lds(P), stream, args);
}

}  // namespace lcp
