// lcp_points.hip - point probes: the signed distance from query points to the scene, and the backward of the distances.
//
// include/lcp_hip.h ("point probes") states the rule; this file follows it comparison by comparison.  A point is mounted on a body m
// (or on the world frame): x = c_m + R(rot_m) xy.  Per candidate body k (k != m; the target alone when one is named; a hull of fewer
// than three vertices never): (d_k, u_k, edge, t) = body_sd of lcp_render_common.h at x - the rule of the drawing and of the
// "circle 1 - hull 2" pair.  Per point: the smallest d_k, the smallest k on ties; none, or d >= max_dist: a void point (dist =
// max_dist, body = -1, normal = 0).
//
// Forward: one workgroup per (scene, 256 points), the scene staged in LDS by stage_scene; lane = point, a loop over the bodies, and a
// body whose bounding circle lies at or beyond min(best so far, max_dist) for every point of the wavefront is skipped by the whole
// wavefront.  The bounding circle only under-estimates d_k (the hull lies inside it, and `reach` carries a rounding slack), so a body
// that is skipped could not have become the selection of a live point: a finite cutoff leaves a live point's bits what +inf gives.
//
// Backward: one workgroup per scene.  Every point recomputes its selection (the same function) and leaves its terms in LDS:
//   dd = u . (dx - dX) - dr,  A = g_dist u
// so the selected body receives -A (a circle at its centre, with -g_dist for the radius; a hull -(1 - t) A and -t A at the two world
// vertices of the edge) and the mounting body +A at x, that is A . perp(x - c_m) for its angle.  g_pt_xy is the point's own.  The terms
// are separate arrays of doubles and ints indexed by the point: lane-consecutive 8-byte and 4-byte accesses, no bank is met twice
// within a half-wavefront.  Then every body is owned by ONE wavefront (body b by wavefront b mod 4), which walks the points in order,
// 64 at a time, exactly as lcp_sensors.hip walks the rays: per-lane sums in point order, the hull's vertices through an LDS
// accumulator of the wavefront (the lanes that selected the same edge add one after the other in lane order), then one butterfly per
// output.  No atomics: two runs give the same bits.
#include "lcp_render_common.h"

namespace lcp {
namespace points {

using render::MAXB;
using render::RD_T;
using render::RD_WAVES;
using render::Scene;
using render::wave_sum;

constexpr int MAXN = 1024;                 // points per scene

struct Points {
  int N;
  const int32_t* body; const double* xy; const int32_t* target; const double* max_dist;
};

// one point in the world frame; ok = false: a void point (a mounting body outside [0, nb) other than -1)
struct Pt {
  bool ok; int mount, target;
  double x, y, md;
};

struct Sel {
  int k, edge;                             // k = -1: a void point (d = max_dist then)
  double d, ux, uy, t;
};

__device__ __forceinline__ Pt load_point(const Scene& S, const Points& pts, int scene, int r, int nb, bool valid) {
  Pt q;
  q.ok = false; q.mount = -1; q.target = -2; q.x = q.y = 0.0; q.md = 0.0;
  if (!valid) return q;
  const size_t i = (size_t)scene * pts.N + r;
  const int m = pts.body[i];
  const double lx = pts.xy[2 * i], ly = pts.xy[2 * i + 1];
  q.md = pts.max_dist[i];
  q.target = pts.target[i];
  q.mount = m;
  if (m == -1) {
    q.ok = true; q.x = lx; q.y = ly;
  } else if (m >= 0 && m < nb) {
    const double sn = S.sn[m], cs = S.cs[m];
    q.ok = true;
    q.x = S.cx[m] + (cs * lx - sn * ly); q.y = S.cy[m] + (sn * lx + cs * ly);
  }
  return q;
}

// The rule of the header for one point against the staged scene.  Uniform control flow over the bodies; `live` masks the lane.
__device__ __forceinline__ Sel select(const Scene& S, int nb, bool live, const Pt& q) {
  Sel H;
  H.k = -1; H.edge = 0; H.d = q.md; H.ux = H.uy = H.t = 0.0;
  double best = __builtin_inf();
  for (int k = 0; k < nb; ++k) {
    const double reach = S.reach[k];
    bool near = live && k != q.mount && reach >= 0.0 && (q.target == -1 || q.target == k);
    if (near) {
      // the bounding circle against what could still change the result: d_k >= |x - c_k| - reach
      const double dx = q.x - S.cx[k], dy = q.y - S.cy[k];
      near = !(sqrt(dx * dx + dy * dy) - reach >= fmin(best, q.md));
    }
    if (!__any(near)) continue;
    int edge; double t, ux, uy;
    const double d = render::body_sd(S, k, q.x, q.y, edge, t, ux, uy);
    if (near && d < best) { best = d; H.k = k; H.edge = edge; H.d = d; H.ux = ux; H.uy = uy; H.t = t; }
  }
  if (H.k < 0 || !(H.d < q.md)) { H.k = -1; H.edge = 0; H.d = q.md; H.ux = H.uy = H.t = 0.0; }
  return H;
}

__global__ void __launch_bounds__(RD_T) lcp_point_distance_kernel(int nb, int cap, int vmax, int chunks, Points pts, const int32_t* kind,
                                                                 const double* radius, const double* verts_local, const int32_t* nverts,
                                                                 const double* p, double* dist, int32_t* body, double* normal) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  const int scene = blockIdx.x / chunks, chunk = blockIdx.x - scene * chunks;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  const int r = chunk * RD_T + threadIdx.x;
  const bool valid = r < pts.N;
  const Pt q = load_point(S, pts, scene, r, nb, valid);
  const Sel H = select(S, nb, ok && q.ok, q);
  if (valid) {
    const size_t i = (size_t)scene * pts.N + r;
    if (dist) dist[i] = H.d;
    if (body) body[i] = H.k;
    if (normal) { normal[2 * i] = H.ux; normal[2 * i + 1] = H.uy; }
  }
}

// the per-point terms of the backward, behind the scene's arrays in the dynamic LDS: N slots each
struct Terms {
  double *ax, *ay, *g, *t, *mrot;          // A = g u, g, the edge parameter, the mounting body's angle term
  int *k, *edge, *mount;                   // selected body (-1: no gradient), its edge, mounting body (-1: none)
};

static size_t terms_lds(int N) { return (size_t)N * (5 * sizeof(double) + 3 * sizeof(int)); }

__global__ void __launch_bounds__(RD_T) lcp_point_distance_backward_kernel(int nb, int cap, int vmax, Points pts, const int32_t* kind,
                                                                          const double* radius, const double* verts_local,
                                                                          const int32_t* nverts, const double* p, const double* g_dist,
                                                                          double* g_p, double* g_radius, double* g_verts_local,
                                                                          double* g_pt_xy) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  __shared__ double2 s_acc[RD_WAVES][ctw::NV];             // per wavefront: the gradient of each world vertex of the body it owns
  const int N = pts.N;
  Terms T;
  T.ax = S.vil + vmax; T.ay = T.ax + N; T.g = T.ay + N; T.t = T.g + N; T.mrot = T.t + N;
  T.k = reinterpret_cast<int*>(T.mrot + N); T.edge = T.k + N; T.mount = T.edge + N;
  const int scene = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  // ---- every point: its selection again, its own gradient, its terms
  for (int r = tid; r - tid < N; r += RD_T) {              // (uniform trip count: select() votes across the wavefront)
    const bool valid = r < N;
    const Pt q = load_point(S, pts, scene, r, nb, valid);
    const Sel H = select(S, nb, ok && q.ok, q);
    if (!valid) continue;
    const size_t i = (size_t)scene * N + r;
    const bool live = H.k >= 0;
    const int m = live && q.mount >= 0 && q.mount < nb ? q.mount : -1;
    const double g = live ? g_dist[i] : 0.0;
    const double ax = g * H.ux, ay = g * H.uy;
    double gx = ax, gy = ay, mrot = 0.0;
    if (m >= 0) {
      const double rx = q.x - S.cx[m], ry = q.y - S.cy[m], sn = S.sn[m], cs = S.cs[m];
      mrot = ay * rx - ax * ry;                                                          // dx/drot = perp(x - c_m)
      gx = cs * ax + sn * ay; gy = -sn * ax + cs * ay;                                   // into the mounting frame
    }
    if (g_pt_xy) { g_pt_xy[2 * i] = gx; g_pt_xy[2 * i + 1] = gy; }
    T.ax[r] = ax; T.ay[r] = ay; T.g[r] = g; T.t[r] = H.t; T.mrot[r] = mrot;
    T.k[r] = H.k; T.edge[r] = H.edge; T.mount[r] = m;
  }
  __syncthreads();
  if (!g_p && !g_radius && !g_verts_local) return;
  // ---- every body: owned by one wavefront, the points in order
  for (int b = wave; b < nb; b += RD_WAVES) {
    const bool hull = S.kind[b] != 0;
    const int o = S.off[b], nv = ok ? S.off[b + 1] - o : 0;               // (a scene that is not probed has no staged vertices)
    s_acc[wave][lane] = make_double2(0.0, 0.0);            // (ctw::NV = 64: one slot per lane, the wavefront's own)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double gx = 0.0, gy = 0.0, grot = 0.0, grad = 0.0;
    for (int r0 = 0; r0 < N; r0 += 64) {
      const int r = r0 + lane;
      const bool valid = r < N;
      const bool struck = valid && T.k[r] == b, mounted = valid && T.mount[r] == b;
      if (!__any(struck || mounted)) continue;
      const double ax = valid ? T.ax[r] : 0.0, ay = valid ? T.ay[r] : 0.0;
      if (mounted) { gx += ax; gy += ay; grot += T.mrot[r]; }
      if (!hull) {
        if (struck) { gx -= ax; gy -= ay; grad -= T.g[r]; }
      } else {
        const int edge = struck ? T.edge[r] : -1;
        const double t = struck ? T.t[r] : 0.0;
        // the lane's rank among the lanes that selected the same edge, and the largest such group: lanes of one rank selected
        // pairwise different edges, so they add without meeting - rank by rank, the edge's first vertex, then its second
        int rank = 0, depth = 0;
        unsigned long long todo = __ballot(struck);
        while (todo) {
          const int e = __shfl(edge, __ffsll((long long)todo) - 1, 64);
          const bool mine = struck && edge == e;
          const unsigned long long m = __ballot(mine);
          if (mine) rank = __popcll(m & ((1ull << lane) - 1));
          depth = max(depth, (int)__popcll(m));
          todo &= ~m;
        }
        const int e1 = edge + 1 >= nv ? 0 : edge + 1;
        for (int j = 0; j < depth; ++j) {
          if (struck && rank == j) {
            double2 u = s_acc[wave][edge];
            u.x -= (1.0 - t) * ax; u.y -= (1.0 - t) * ay;
            s_acc[wave][edge] = u;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (struck && rank == j) {
            double2 v = s_acc[wave][e1];
            v.x -= t * ax; v.y -= t * ay;
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

}  // namespace points

bool point_distance_supported(int nb, int nvcap, int scene_verts_max, int N) {
  return render_supported(nb, nvcap, scene_verts_max) && N >= 1 && N <= points::MAXN;
}

int point_distance_launch(int B, int nb, int nvcap, int scene_verts_max, int N, const int32_t* kind, const double* radius,
                          const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pt_body,
                          const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist, double* dist, int32_t* body,
                          double* normal, void* stream) {
  using namespace points;
  if (!point_distance_supported(nb, nvcap, scene_verts_max, N)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  int chunks = (N + RD_T - 1) / RD_T;
  Points pts{N, pt_body, pt_xy, pt_target, pt_max_dist};
  void* args[] = {&nb, &nvcap, &vmax, &chunks, &pts, &kind, &radius, &verts_local, &nverts, &p, &dist, &body, &normal};
  return launch(reinterpret_cast<const void*>(lcp_point_distance_kernel), (long long)B * chunks, render::scene_lds(vmax), stream, args);
}

int point_distance_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int N, const int32_t* kind, const double* radius,
                                   const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pt_body,
                                   const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist, const double* g_dist,
                                   double* g_p, double* g_radius, double* g_verts_local, double* g_pt_xy, void* stream) {
  using namespace points;
  if (!point_distance_supported(nb, nvcap, scene_verts_max, N)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  Points pts{N, pt_body, pt_xy, pt_target, pt_max_dist};
  void* args[] = {&nb, &nvcap, &vmax, &pts, &kind, &radius, &verts_local, &nverts, &p, &g_dist, &g_p, &g_radius, &g_verts_local,
                  &g_pt_xy};
  return launch(reinterpret_cast<const void*>(lcp_point_distance_backward_kernel), B, render::scene_lds(vmax) + terms_lds(N), stream, args);
}

}  // namespace lcp
