// lcp_sensors.hip - range sensors: rays cast against every scene's geometry, and the backward of the distances.
//
// include/lcp_hip.h ("range sensors") states the rule; this file follows it comparison by comparison.  A ray is mounted on a body m
// (or on the world frame): o = c_m + R(rot_m) origin, u = (cos, sin)(rot_m + angle).  Per body k != m:
//   circle   q = o - c, b = q . u, cc = q . q - r^2:  cc <= 0: s = 0;  else miss if b >= 0 or b^2 - cc < 0;
//            else s = -b - sqrt(b^2 - cc), n = (o + s u - c) / r
//   hull     h_i = n_i . (o - w_i), den_i = n_i . u over the world vertices, edges and outward normals of the drawing
//            (lcp_render_common.h):  all h_i <= 0: s = 0;  den_i == 0 and h_i > 0: miss;  s_in = max -h_i / den_i over den_i < 0 (first
//            i on ties), s_out = min -h_i / den_i over den_i > 0;  hit iff 0 <= s_in <= s_out: s = s_in, n = n_i,
//            t = (o + s u - w_i) . e_i / |e_i|^2
//   ray      the smallest s_k, the smallest k on ties; none, or s >= range: dist = range, hit = -1, normal = 0
//
// Forward: one workgroup per (scene, 256 rays), the scene staged in LDS by stage_scene; lane = ray, a loop over the bodies, and a body
// whose bounding circle none of the wavefront's rays can reach within their range is skipped by the whole wavefront (beyond it the
// rule gives a miss or s >= range, so the result does not depend on the skip).
//
// Backward: one workgroup per scene.  Every ray recomputes its hit (the same function) and leaves its terms in LDS:
//   ds = (n . dX + dr - n . (do + s du)) / (n . u),  a = g_dist / (n . u),  A = a n
// so the struck body receives +A (a circle at its centre, with a for the radius; a hull (1 - t) A and t A at the two world vertices
// of the edge) and the mounting body -A at o and -s A . perp(u) for its angle.  g_ray_origin and g_ray_angle are the ray's own.
// Then every body is owned by ONE wavefront (body b by wavefront b mod 4), which walks the rays in order, 64 at a time: per-lane
// sums in ray order, the hull's vertices through an LDS accumulator of the wavefront (the lanes that struck the same edge add one after
// the other in lane order, lanes that struck different edges together), then one butterfly per output.  No atomics: two runs give the
// same bits.
#include "lcp_render_common.h"

namespace lcp {
namespace sensors {

using render::MAXB;
using render::RD_T;
using render::RD_WAVES;
using render::Scene;
using render::wave_sum;

constexpr int MAXR = 1024;                 // rays per scene

struct Rays {
  int R;
  const int32_t* body; const double* origin; const double* angle; const double* range;
};

// one ray in the world frame; ok = false: it misses everything (a mounting body outside [0, nb) other than -1)
struct Ray {
  bool ok; int mount;
  double ox, oy, ux, uy, range;
};

struct Hit {
  int k, edge;                             // k = -1: a miss or clamped at the range (s = range then)
  double s, nx, ny, t;
};

// (the direction from the angle p holds, not from the staged sine and cosine)
__device__ __forceinline__ Ray load_ray(const Scene& S, const Rays& rays, const double* p, int scene, int r, int nb, bool valid) {
  Ray y;
  y.ok = false; y.mount = -1; y.ox = y.oy = 0.0; y.ux = 1.0; y.uy = 0.0; y.range = 0.0;
  if (!valid) return y;
  const size_t i = (size_t)scene * rays.R + r;
  const int m = rays.body[i];
  const double lx = rays.origin[2 * i], ly = rays.origin[2 * i + 1], ang = rays.angle[i];
  y.range = rays.range[i];
  y.mount = m;
  if (m == -1) {
    y.ok = true; y.ox = lx; y.oy = ly; y.ux = cos(ang); y.uy = sin(ang);
  } else if (m >= 0 && m < nb) {
    const double sn = S.sn[m], cs = S.cs[m], a = p[((size_t)scene * nb + m) * 3] + ang;
    y.ok = true;
    y.ox = S.cx[m] + (cs * lx - sn * ly); y.oy = S.cy[m] + (sn * lx + cs * ly);
    y.ux = cos(a); y.uy = sin(a);
  }
  return y;
}

// The rule of the header for one ray against the staged scene.  Uniform control flow over the bodies; `live` masks the lane.
__device__ __forceinline__ Hit cast(const Scene& S, int nb, bool live, const Ray& y) {
  Hit H;
  H.k = -1; H.edge = 0; H.s = y.range; H.nx = H.ny = H.t = 0.0;
  const double INF = __builtin_inf();
  double best = INF;
  for (int k = 0; k < nb; ++k) {
    const double reach = S.reach[k];
    bool near = live && k != y.mount && reach >= 0.0;
    if (near) {
      // the bounding circle against the ray's line, its start and its range
      const double qx = S.cx[k] - y.ox, qy = S.cy[k] - y.oy;
      const double along = qx * y.ux + qy * y.uy, across = qx * y.uy - qy * y.ux;
      near = !(across * across > reach * reach) && !(along < -reach) && !(along - reach >= y.range);
    }
    if (!__any(near)) continue;
    double s = -1.0, nx = 0.0, ny = 0.0, t = 0.0;
    int edge = 0;
    bool hit = false;
    if (S.kind[k] == 0) {
      const double r = S.rad[k];
      const double qx = y.ox - S.cx[k], qy = y.oy - S.cy[k];
      const double b = qx * y.ux + qy * y.uy, cc = qx * qx + qy * qy - r * r;
      const double disc = b * b - cc;
      if (cc <= 0.0) { hit = true; s = 0.0; }
      else if (!(b >= 0.0) && !(disc < 0.0)) {
        hit = true;
        s = -b - sqrt(disc);
        nx = (qx + s * y.ux) / r; ny = (qy + s * y.uy) / r;
      }
    } else {
      const int o = S.off[k], nv = S.off[k + 1] - o;
      bool inside = true, miss = false;
      double s_in = -INF, s_out = INF;
      for (int i = 0; i < nv; ++i) {
        const double2 vw = S.vw[o + i], vn = S.vn[o + i];
        const double h = vn.x * (y.ox - vw.x) + vn.y * (y.oy - vw.y), den = vn.x * y.ux + vn.y * y.uy;
        inside = inside && h <= 0.0;
        miss = miss || (den == 0.0 && h > 0.0);
        const double c = -h / den;
        if (den < 0.0 && c > s_in) { s_in = c; edge = i; }
        if (den > 0.0 && c < s_out) s_out = c;
      }
      if (inside) { hit = true; s = 0.0; }
      else if (!miss && 0.0 <= s_in && s_in <= s_out) {
        hit = true;
        s = s_in;
        const double2 vw = S.vw[o + edge], ve = S.ve[o + edge], vn = S.vn[o + edge];
        const double il = S.vil[o + edge];
        nx = vn.x; ny = vn.y;
        t = ((y.ox + s * y.ux - vw.x) * ve.x + (y.oy + s * y.uy - vw.y) * ve.y) * il * il;
      }
    }
    if (near && hit && s < best) { best = s; H.k = k; H.edge = edge; H.s = s; H.nx = nx; H.ny = ny; H.t = t; }
  }
  if (H.k < 0 || H.s >= y.range) { H.k = -1; H.edge = 0; H.s = y.range; H.nx = H.ny = H.t = 0.0; }
  else if (H.s == 0.0) { H.nx = H.ny = H.t = 0.0; }
  return H;
}

__global__ void __launch_bounds__(RD_T) lcp_cast_rays_kernel(int nb, int cap, int vmax, int chunks, Rays rays, const int32_t* kind,
                                                            const double* radius, const double* verts_local, const int32_t* nverts,
                                                            const double* p, double* dist, int32_t* hit, double* normal) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  const int scene = blockIdx.x / chunks, chunk = blockIdx.x - scene * chunks;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  const int r = chunk * RD_T + threadIdx.x;
  const bool valid = r < rays.R;
  const Ray y = load_ray(S, rays, p, scene, r, nb, valid);
  const Hit H = cast(S, nb, ok && y.ok, y);
  if (valid) {
    const size_t i = (size_t)scene * rays.R + r;
    if (dist) dist[i] = H.s;
    if (hit) hit[i] = H.k;
    if (normal) { normal[2 * i] = H.nx; normal[2 * i + 1] = H.ny; }
  }
}

// the per-ray terms of the backward, behind the scene's arrays in the dynamic LDS: R slots each
struct Terms {
  double *ax, *ay, *a, *t, *mrot;          // A, a, the edge parameter, the mounting body's angle term
  int *k, *edge, *mount;                   // struck body (-1: no gradient), its edge, mounting body (-1: none)
};

static size_t terms_lds(int R) { return (size_t)R * (5 * sizeof(double) + 3 * sizeof(int)); }

__global__ void __launch_bounds__(RD_T) lcp_cast_rays_backward_kernel(int nb, int cap, int vmax, Rays rays, const int32_t* kind,
                                                                     const double* radius, const double* verts_local,
                                                                     const int32_t* nverts, const double* p, const double* g_dist,
                                                                     double* g_p, double* g_radius, double* g_verts_local,
                                                                     double* g_ray_origin, double* g_ray_angle) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  __shared__ double2 s_acc[RD_WAVES][ctw::NV];             // per wavefront: the gradient of each world vertex of the body it owns
  const int R = rays.R;
  Terms T;
  T.ax = S.vil + vmax; T.ay = T.ax + R; T.a = T.ay + R; T.t = T.a + R; T.mrot = T.t + R;
  T.k = reinterpret_cast<int*>(T.mrot + R); T.edge = T.k + R; T.mount = T.edge + R;
  const int scene = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  // ---- every ray: its hit again, its own gradients, its terms
  for (int r = tid; r - tid < R; r += RD_T) {              // (uniform trip count: cast() votes across the wavefront)
    const bool valid = r < R;
    const Ray y = load_ray(S, rays, p, scene, r, nb, valid);
    const Hit H = cast(S, nb, ok && y.ok, y);
    if (!valid) continue;
    const size_t i = (size_t)scene * R + r;
    const bool active = H.k >= 0 && H.s > 0.0;
    double ax = 0.0, ay = 0.0, a = 0.0, go_x = 0.0, go_y = 0.0, gang = 0.0, mrot = 0.0;
    const int m = y.mount >= 0 && y.mount < nb ? y.mount : -1;
    if (active) {
      a = g_dist[i] / (H.nx * y.ux + H.ny * y.uy);
      ax = a * H.nx; ay = a * H.ny;
      gang = -H.s * (ay * y.ux - ax * y.uy);                                             // -s A . perp(u), perp(u) = (-u.y, u.x)
      go_x = -ax; go_y = -ay;
      if (m >= 0) {
        const double rx = y.ox - S.cx[m], ry = y.oy - S.cy[m], sn = S.sn[m], cs = S.cs[m];
        mrot = -(ay * rx - ax * ry) + gang;                                              // do/drot = perp(o - c_m), du/drot = perp(u)
        const double wx = go_x, wy = go_y;
        go_x = cs * wx + sn * wy; go_y = -sn * wx + cs * wy;                             // into the mounting frame
      }
    }
    if (g_ray_origin) { g_ray_origin[2 * i] = go_x; g_ray_origin[2 * i + 1] = go_y; }
    if (g_ray_angle) g_ray_angle[i] = gang;
    T.ax[r] = ax; T.ay[r] = ay; T.a[r] = a; T.t[r] = H.t; T.mrot[r] = mrot;
    T.k[r] = active ? H.k : -1; T.edge[r] = H.edge; T.mount[r] = active ? m : -1;
  }
  __syncthreads();
  if (!g_p && !g_radius && !g_verts_local) return;
  // ---- every body: owned by one wavefront, the rays in order
  for (int b = wave; b < nb; b += RD_WAVES) {
    const bool hull = S.kind[b] != 0;
    const int o = S.off[b], nv = ok ? S.off[b + 1] - o : 0;               // (a scene that is not sensed has no staged vertices)
    s_acc[wave][lane] = make_double2(0.0, 0.0);            // (ctw::NV = 64: one slot per lane, the wavefront's own)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double gx = 0.0, gy = 0.0, grot = 0.0, grad = 0.0;
    for (int r0 = 0; r0 < R; r0 += 64) {
      const int r = r0 + lane;
      const bool valid = r < R;
      const bool struck = valid && T.k[r] == b, mounted = valid && T.mount[r] == b;
      if (!__any(struck || mounted)) continue;
      const double ax = valid ? T.ax[r] : 0.0, ay = valid ? T.ay[r] : 0.0;
      if (mounted) { gx -= ax; gy -= ay; grot += T.mrot[r]; }
      if (!hull) {
        if (struck) { gx += ax; gy += ay; grad += T.a[r]; }
      } else {
        const int edge = struck ? T.edge[r] : -1;
        const double t = struck ? T.t[r] : 0.0;
        // the lane's rank among the lanes that struck the same edge, and the largest such group: lanes of one rank struck pairwise
        // different edges, so they add without meeting - rank by rank, the edge's first vertex, then its second
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
            u.x += (1.0 - t) * ax; u.y += (1.0 - t) * ay;
            s_acc[wave][edge] = u;
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (struck && rank == j) {
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

}  // namespace sensors

bool cast_rays_supported(int nb, int nvcap, int scene_verts_max, int R) {
  return render_supported(nb, nvcap, scene_verts_max) && R >= 1 && R <= sensors::MAXR;
}

int cast_rays_launch(int B, int nb, int nvcap, int scene_verts_max, int R, const int32_t* kind, const double* radius,
                     const double* verts_local, const int32_t* nverts, const double* p, const int32_t* ray_body,
                     const double* ray_origin, const double* ray_angle, const double* ray_range, double* dist, int32_t* hit,
                     double* normal, void* stream) {
  using namespace sensors;
  if (!cast_rays_supported(nb, nvcap, scene_verts_max, R)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  int chunks = (R + RD_T - 1) / RD_T;
  Rays rays{R, ray_body, ray_origin, ray_angle, ray_range};
  void* args[] = {&nb, &nvcap, &vmax, &chunks, &rays, &kind, &radius, &verts_local, &nverts, &p, &dist, &hit, &normal};
  return launch(reinterpret_cast<const void*>(lcp_cast_rays_kernel), (long long)B * chunks, render::scene_lds(vmax), stream, args);
}

int cast_rays_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int R, const int32_t* kind, const double* radius,
                              const double* verts_local, const int32_t* nverts, const double* p, const int32_t* ray_body,
                              const double* ray_origin, const double* ray_angle, const double* ray_range, const double* g_dist,
                              double* g_p, double* g_radius, double* g_verts_local, double* g_ray_origin, double* g_ray_angle,
                              void* stream) {
  using namespace sensors;
  if (!cast_rays_supported(nb, nvcap, scene_verts_max, R)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  Rays rays{R, ray_body, ray_origin, ray_angle, ray_range};
  void* args[] = {&nb, &nvcap, &vmax, &rays, &kind, &radius, &verts_local, &nverts, &p, &g_dist, &g_p, &g_radius, &g_verts_local,
                  &g_ray_origin, &g_ray_angle};
  return launch(reinterpret_cast<const void*>(lcp_cast_rays_backward_kernel), B, render::scene_lds(vmax) + terms_lds(R), stream, args);
}

}  // namespace lcp
