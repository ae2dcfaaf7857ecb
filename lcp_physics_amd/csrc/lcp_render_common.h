// lcp_render_common.h - what the drawing kernels share (lcp_render.hip: bodies; lcp_render_marks.hip: bodies with their marks and the
// joints' markers): the camera, the scene staged in LDS over the packed vertex list, the signed distances with their derivative data,
// the coverage ramp and the wavefront sum.  include/lcp_hip.h ("drawing") has the formulas.
#ifndef LCP_RENDER_COMMON_H
#define LCP_RENDER_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_contacts_wide.h"
#include "lcp_kernels.h"

namespace lcp {
namespace render {

constexpr int RD_T = 256;                  // threads per workgroup (four wavefronts)
constexpr int RD_WAVES = RD_T / 64;
constexpr int TILE_W = 64, TILE_H = 16;    // forward tile: lane = column, four rows per wavefront
constexpr int MAXB = ctw::MAXB;

struct Cam {
  int H, W, C;
  double x0, y0, ppm, w;
};

// The scene in LDS: the body tables (static) and the packed per-vertex arrays (dynamic, vmax slots each).
struct Scene {
  int* kind; int* off; double* rad;                      // stage_bodies (lcp_contacts_wide.h)
  double *cx, *cy, *sn, *cs, *reach, *thick;             // pose, bounding radius grown by w / 2 (< 0: not drawn), thickness
  float* col;                                            // [MAXB][4], channels >= C zero
  double2 *vw, *ve, *vn; double* vil;                    // world vertex, edge vector, outward normal, 1 / |edge|
};

#define LCP_RD_SCENE_TABLES(S, dyn, vmax)                                                                                      \
  __shared__ int s_kind[MAXB], s_off[MAXB + 1];                                                                                 \
  __shared__ double s_rad[MAXB], s_cx[MAXB], s_cy[MAXB], s_sn[MAXB], s_cs[MAXB], s_reach[MAXB], s_thick[MAXB];                  \
  __shared__ float s_col[MAXB * 4];                                                                                             \
  Scene S;                                                                                                                      \
  S.kind = s_kind; S.off = s_off; S.rad = s_rad; S.cx = s_cx; S.cy = s_cy; S.sn = s_sn; S.cs = s_cs; S.reach = s_reach;         \
  S.thick = s_thick; S.col = s_col;                                                                                             \
  S.vw = reinterpret_cast<double2*>(dyn); S.ve = S.vw + (vmax); S.vn = S.ve + (vmax);                                           \
  S.vil = reinterpret_cast<double*>(S.vn + (vmax))

static size_t scene_lds(int vmax) { return (size_t)vmax * (3 * sizeof(double2) + sizeof(double)); }

// Stages scene `scene`; false (for the whole workgroup) when its hull vertices exceed vmax: such a scene is not drawn.
__device__ __forceinline__ bool stage_scene(const Scene& S, int scene, int nb, int cap, int vmax, int C, const int32_t* kind,
                                            const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                            const float* colors, const double* thickness, double w) {
  const int tid = threadIdx.x;
  const int total = ctw::stage_bodies(scene, nb, cap, kind, nverts, radius, S.kind, S.off, S.rad);
  if (tid < nb) {
    const double* pose = p + ((size_t)scene * nb + tid) * 3;
    const double rot = pose[0];
    S.cx[tid] = pose[1]; S.cy[tid] = pose[2];
    S.sn[tid] = sin(rot); S.cs[tid] = cos(rot);
    S.thick[tid] = thickness ? thickness[(size_t)scene * nb + tid] : 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) S.col[tid * 4 + c] = c < C ? colors[((size_t)scene * nb + tid) * C + c] : 0.0f;
  }
  __syncthreads();
  if (total > vmax) return false;
  for (int idx = tid; idx < nb * cap; idx += RD_T) {
    const int b = idx / cap, k = idx - b * cap;
    const int o = S.off[b], nvb = S.off[b + 1] - o;
    if (k < nvb) {                                                                      // (vertex slots >= nverts are never read)
      const double* vl = verts_local + ((size_t)scene * nb + b) * cap * 2;
      const int k1 = k + 1 == nvb ? 0 : k + 1;
      const double2 a = *reinterpret_cast<const double2*>(vl + 2 * k), c = *reinterpret_cast<const double2*>(vl + 2 * k1);
      const double sn = S.sn[b], cs = S.cs[b];
      const double ax = S.cx[b] + (cs * a.x - sn * a.y), ay = S.cy[b] + (sn * a.x + cs * a.y);     // utils.py:105-112
      const double bx = S.cx[b] + (cs * c.x - sn * c.y), by = S.cy[b] + (sn * c.x + cs * c.y);
      const double ex = bx - ax, ey = by - ay;
      const double il = 1.0 / sqrt(ex * ex + ey * ey);
      S.vw[o + k] = make_double2(ax, ay);
      S.ve[o + k] = make_double2(ex, ey);
      S.vn[o + k] = make_double2(ey * il, -ex * il);                                     // left_orthogonal(e) / |e|, contacts.py:229-231
      S.vil[o + k] = il;
    }
  }
  __syncthreads();
  if (tid < nb) {
    double r = S.rad[tid];
    const int o = S.off[tid], nvb = S.off[tid + 1] - o;
    bool drawn = true;
    if (S.kind[tid] != 0) {
      drawn = nvb >= 3;
      r = 0.0;
      for (int k = 0; k < nvb; ++k) {
        const double dx = S.vw[o + k].x - S.cx[tid], dy = S.vw[o + k].y - S.cy[tid];
        r = fmax(r, sqrt(dx * dx + dy * dy));
      }
    }
    // the slack covers the rounding of the distances compared with it (relative to the coordinates they are formed from)
    const double slack = 1e-9 * (fabs(S.cx[tid]) + fabs(S.cy[tid]) + r + w);
    S.reach[tid] = drawn ? r + 0.5 * w + slack : -1.0;
  }
  __syncthreads();
  return true;
}

// Signed distance of hull [o, o + nv) at x, and where it is attained: edge `edge` at parameter t with unit direction u = dd/dx
// (dd/dw_edge = -(1 - t) u, dd/dw_edge+1 = -t u).
__device__ __forceinline__ double hull_sd(const Scene& S, int o, int nv, double px, double py, int& edge, double& t, double& ux,
                                          double& uy) {
  double m = -1e308, d2min = 1e308;
  int im = 0, io = 0;
  for (int i = 0; i < nv; ++i) {
    const double2 vw = S.vw[o + i], ve = S.ve[o + i], vn = S.vn[o + i];
    const double il = S.vil[o + i];
    const double qx = px - vw.x, qy = py - vw.y;
    const double h = vn.x * qx + vn.y * qy;
    if (h > m) { m = h; im = i; }
    const double s = (qx * ve.x + qy * ve.y) * il * il;
    const double tc = fmin(fmax(s, 0.0), 1.0);
    const double rx = qx - tc * ve.x, ry = qy - tc * ve.y;
    const double d2 = rx * rx + ry * ry;
    if (d2 < d2min) { d2min = d2; io = i; }
  }
  const bool inside = m <= 0.0;
  edge = inside ? im : io;
  const double2 vw = S.vw[o + edge], ve = S.ve[o + edge], vn = S.vn[o + edge];
  const double il = S.vil[o + edge];
  const double qx = px - vw.x, qy = py - vw.y;
  const double s = (qx * ve.x + qy * ve.y) * il * il;
  const double tc = fmin(fmax(s, 0.0), 1.0);
  const double rx = qx - tc * ve.x, ry = qy - tc * ve.y;
  const double dout = sqrt(d2min);
  const double id = dout > 0.0 ? 1.0 / dout : 0.0;
  t = inside ? s : tc;
  ux = inside ? vn.x : rx * id;
  uy = inside ? vn.y : ry * id;
  return inside ? m : dout;
}

// Signed distance of body k at x with its derivative data (a circle: u = (x - c) / |x - c|, 0 at the centre as torch.norm has it).
__device__ __forceinline__ double body_sd(const Scene& S, int k, double px, double py, int& edge, double& t, double& ux, double& uy) {
  if (S.kind[k] != 0) return hull_sd(S, S.off[k], S.off[k + 1] - S.off[k], px, py, edge, t, ux, uy);
  const double dx = px - S.cx[k], dy = py - S.cy[k];
  const double len = sqrt(dx * dx + dy * dy);
  const double id = len > 0.0 ? 1.0 / len : 0.0;
  edge = 0; t = 0.0; ux = dx * id; uy = dy * id;
  return len - S.rad[k];
}

__device__ __forceinline__ double cov(double d, double iw) { return fmin(fmax(0.5 - d * iw, 0.0), 1.0); }
__device__ __forceinline__ double alpha_of(double d, double th, double iw) {
  const double c0 = cov(d, iw);
  return th > 0.0 ? c0 - cov(d + th, iw) : c0;
}
// d cov / dd: -1 / w strictly inside the ramp, else 0
__device__ __forceinline__ double dcov(double d, double iw) {
  const double a = 0.5 - d * iw;
  return a > 0.0 && a < 1.0 ? -iw : 0.0;
}

// whether pixel x can see body k at all: outside the grown bounding circle alpha is exactly 0 and d > 0
__device__ __forceinline__ bool within_reach(const Scene& S, int k, double px, double py) {
  const double dx = px - S.cx[k], dy = py - S.cy[k], r = S.reach[k];
  return !(dx * dx + dy * dy > r * r);
}

// alpha and d of body k at the pixels of this wavefront (0 and +1 beyond its reach; the skip is per wavefront)
__device__ __forceinline__ double body_alpha(const Scene& S, int k, double px, double py, bool valid, double iw, double& d) {
  d = 1.0;
  const bool near = valid && within_reach(S, k, px, py);
  if (!__any(near)) return 0.0;
  int edge; double t, ux, uy;
  const double dk = body_sd(S, k, px, py, edge, t, ux, uy);
  if (!near) return 0.0;
  d = dk;
  return alpha_of(dk, S.thick[k], iw);
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

}  // namespace render
}  // namespace lcp
#endif
