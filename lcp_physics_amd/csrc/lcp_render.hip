// lcp_render.hip - the reference's drawing on the device: frames and segmentation masks of every scene, and their backward.
//
// What Body.draw (physics/bodies.py:140-150 circles, :237-250 hulls) and the paint loop of run_world (world.py:279-280) put on
// the screen, restated so that it can be differentiated: pixel = pos * pixels_per_meter, x to the right, y downward, bodies
// painted in list order, thickness 0 = filled, > 0 = an outline of that width.  Pixel (i, j) is sampled at the world point
// x = (x0 + (j + 1/2) / ppm, y0 + (i + 1/2) / ppm).
//   signed distance   circle |x - c| - r;  hull: w_i = c + R(rot) v_i (utils.py:105-112), e_i = w_i+1 - w_i,
//                     n_i = left_orthogonal(e_i) / |e_i| (contacts.py:229-231), h_i = n_i . (x - w_i), m = max h_i;
//                     d = m where m <= 0, else the distance to the nearest edge segment
//   coverage          cov(d) = clamp(1/2 - d / w, 0, 1);  alpha = cov(d), or cov(d) - cov(d + thickness) for an outline
//   image             I = background;  for k = 0 .. nb-1:  I = I (1 - alpha_k) + alpha_k colour_k
//   mask              the largest k with d_k <= 0, or -1
// fp64 arithmetic, the image stored as fp32.  Not drawn: a hull of fewer than three vertices.  The circle's spoke, the hull's centre
// dot, the rect's diagonals and the joints' markers are lcp_render_marks.hip's, over the same bodies (lcp_render_common.h).
//
// Forward: one workgroup per (scene, tile of 16 x 64 pixels).  The scene's world vertices, edge vectors, normals and inverse edge
// lengths are staged in LDS once (the packed vertex list of lcp_contacts_wide.hip: <= 64 bodies, capacity 8..64, <= 1024 hull
// vertices).  A body whose bounding circle, grown by w / 2, misses the tile is skipped: there alpha is exactly 0 and d > 0, so
// the output does not depend on the cull.  Lane = column, so a wavefront writes 256 contiguous bytes of an image row.
//
// Backward: one workgroup per (scene, body), walking the body's pixel box (clamped to the image in floating point, before any
// conversion to an integer).  At each pixel the compositing state is recomputed from the bodies whose grown bounding circles meet
// this body's: T_k = prod_{j > k} (1 - alpha_j) and the colour below.  Every output element is owned by one workgroup; the sums
// run over registers in pixel order, then xor butterflies, then the four wavefronts in order: no atomics, the same bits every run.
// The vertex gradients go through per-wavefront LDS accumulators: the lanes of a wavefront that hit the same edge are summed by a
// butterfly and lane 0 adds the sum, edge by edge in lane order.
#include "lcp_render_common.h"

namespace lcp {
namespace render {

__global__ void __launch_bounds__(RD_T) lcp_render_kernel(int nb, int cap, int vmax, int tiles, Cam cam, const int32_t* kind, const double* radius,
                                                         const double* verts_local, const int32_t* nverts, const double* p,
                                                         const float* colors, const float* background, const double* thickness,
                                                         float* image, int32_t* ids) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  __shared__ unsigned long long s_mask;
  const int scene = blockIdx.x / tiles, tile = blockIdx.x - scene * tiles;
  const int tiles_x = (cam.W + TILE_W - 1) / TILE_W;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ok = stage_scene(S, scene, nb, cap, vmax, cam.C, kind, radius, verts_local, nverts, p, colors, thickness, cam.w);
  const int i0 = ty * TILE_H, j0 = tx * TILE_W;
  const int i1 = min(i0 + TILE_H, cam.H) - 1, j1 = min(j0 + TILE_W, cam.W) - 1;      // the tile's last row and column
  if (threadIdx.x < 64) {
    // the bodies that can reach the rectangle of this tile's pixel centres
    bool vis = false;
    if (ok && lane < nb && S.reach[lane] >= 0.0) {
      const double xa = cam.x0 + (j0 + 0.5) / cam.ppm, xb = cam.x0 + (j1 + 0.5) / cam.ppm;
      const double ya = cam.y0 + (i0 + 0.5) / cam.ppm, yb = cam.y0 + (i1 + 0.5) / cam.ppm;
      const double dx = fmax(fmax(xa - S.cx[lane], S.cx[lane] - xb), 0.0), dy = fmax(fmax(ya - S.cy[lane], S.cy[lane] - yb), 0.0);
      vis = !(dx * dx + dy * dy > S.reach[lane] * S.reach[lane]);
    }
    const unsigned long long m = __ballot(vis);
    if (lane == 0) s_mask = m;
  }
  __syncthreads();
  const unsigned long long mask = s_mask;
  const double iw = 1.0 / cam.w;
  const int j = j0 + lane;
  const double px = cam.x0 + (j + 0.5) / cam.ppm;
  double bg[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bg[c] = image && c < cam.C ? (double)background[c] : 0.0;
#pragma unroll 1
  for (int r = 0; r < TILE_H / RD_WAVES; ++r) {
    const int i = i0 + wave + RD_WAVES * r;
    const bool valid = i < cam.H && j < cam.W;
    const double py = cam.y0 + (i + 0.5) / cam.ppm;
    double I[4] = {bg[0], bg[1], bg[2], bg[3]};
    int top = -1;
    for (unsigned long long m = mask; m; m &= m - 1) {
      const int k = __ffsll((long long)m) - 1;
      double d;
      const double a = body_alpha(S, k, px, py, valid, iw, d);
      if (d <= 0.0) top = k;
#pragma unroll
      for (int c = 0; c < 4; ++c) I[c] = I[c] * (1.0 - a) + a * (double)S.col[k * 4 + c];
    }
    if (valid) {
      if (image) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < cam.C) image[(((size_t)scene * cam.C + c) * cam.H + i) * cam.W + j] = (float)I[c];
      }
      if (ids) ids[((size_t)scene * cam.H + i) * cam.W + j] = top;
    }
  }
}

__global__ void __launch_bounds__(RD_T) lcp_render_backward_kernel(int nb, int cap, int vmax, Cam cam, const int32_t* kind,
                                                                  const double* radius, const double* verts_local,
                                                                  const int32_t* nverts, const double* p, const float* colors,
                                                                  const float* background, const double* thickness,
                                                                  const float* g_image, double* g_p, double* g_radius,
                                                                  double* g_verts_local, float* g_colors) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  __shared__ unsigned long long s_mask;
  __shared__ double2 s_acc[RD_WAVES][ctw::NV];             // per wavefront: the gradient of each world vertex of this body
  __shared__ double s_red[RD_WAVES][8];
  const int scene = blockIdx.x / nb, k = blockIdx.x - scene * nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool ok = stage_scene(S, scene, nb, cap, vmax, cam.C, kind, radius, verts_local, nverts, p, colors, thickness, cam.w);
  const bool drawn = ok && S.reach[k] >= 0.0;
  if (tid < 64) {
    bool ov = false;
    if (drawn && lane < nb && S.reach[lane] >= 0.0) {
      const double dx = S.cx[lane] - S.cx[k], dy = S.cy[lane] - S.cy[k], r = S.reach[lane] + S.reach[k];
      ov = !(dx * dx + dy * dy > r * r);
    }
    const unsigned long long m = __ballot(ov);
    if (lane == 0) s_mask = m;
  }
  for (int v = lane; v < ctw::NV; v += 64) s_acc[wave][v] = make_double2(0.0, 0.0);
  __syncthreads();
  const unsigned long long mask = s_mask;
  const unsigned long long below = mask & ((1ull << k) - 1), above = k == 63 ? 0ull : mask & ~((2ull << k) - 1);
  const bool hull = S.kind[k] != 0;
  const int o = S.off[k], nv = S.off[k + 1] - o;
  const double iw = 1.0 / cam.w, th = S.thick[k];
  // the pixel box of the grown bounding circle, clamped to the image while still in floating point (a body at 1e15, a non-finite
  // bound: an empty box or the whole image, never an index outside it)
  const double reach = drawn ? S.reach[k] : -1.0;
  const double fj0 = fmin(fmax(floor((S.cx[k] - reach - cam.x0) * cam.ppm - 0.5) - 1.0, 0.0), (double)cam.W);
  const double fj1 = fmin(fmax(ceil((S.cx[k] + reach - cam.x0) * cam.ppm - 0.5) + 1.0, -1.0), (double)cam.W - 1.0);
  const double fi0 = fmin(fmax(floor((S.cy[k] - reach - cam.y0) * cam.ppm - 0.5) - 1.0, 0.0), (double)cam.H);
  const double fi1 = fmin(fmax(ceil((S.cy[k] + reach - cam.y0) * cam.ppm - 0.5) + 1.0, -1.0), (double)cam.H - 1.0);
  const int jlo = (int)fj0, jhi = drawn ? (int)fj1 : -1, ilo = (int)fi0, ihi = drawn ? (int)fi1 : -1;
  double colk[4], bg[4], gcol[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 4; ++c) { colk[c] = (double)S.col[k * 4 + c]; bg[c] = c < cam.C ? (double)background[c] : 0.0; }
  double acc_r = 0.0, acc_x = 0.0, acc_y = 0.0;            // circle: radius and centre
#pragma unroll 1
  for (int ib = ilo; ib <= ihi; ib += RD_WAVES) {
    const int i = ib + wave;
    const double py = cam.y0 + (i + 0.5) / cam.ppm;
#pragma unroll 1
    for (int jb = jlo; jb <= jhi; jb += 64) {
      const int j = jb + lane;
      const bool valid = i <= ihi && j <= jhi;
      const double px = cam.x0 + (j + 0.5) / cam.ppm;
      const bool near = valid && within_reach(S, k, px, py);
      if (!__any(near)) continue;
      int edge; double t, ux, uy;
      const double d = body_sd(S, k, px, py, edge, t, ux, uy);
      const double alpha = alpha_of(d, th, iw);
      const double dadd = th > 0.0 ? dcov(d, iw) - dcov(d + th, iw) : dcov(d, iw);
      const bool active = near && (alpha != 0.0 || dadd != 0.0);
      if (!__any(active)) continue;
      double T = 1.0;
      for (unsigned long long m = above; m; m &= m - 1) {
        double dj;
        T *= 1.0 - body_alpha(S, __ffsll((long long)m) - 1, px, py, active, iw, dj);
      }
      const bool geo = active && dadd != 0.0;
      double I[4] = {bg[0], bg[1], bg[2], bg[3]};
      if (__any(geo)) {
        for (unsigned long long m = below; m; m &= m - 1) {
          const int jj = __ffsll((long long)m) - 1;
          double dj;
          const double a = body_alpha(S, jj, px, py, geo, iw, dj);
#pragma unroll
          for (int c = 0; c < 4; ++c) I[c] = I[c] * (1.0 - a) + a * (double)S.col[jj * 4 + c];
        }
      }
      double gal = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < cam.C) {
          const double g = active ? (double)g_image[(((size_t)scene * cam.C + c) * cam.H + i) * cam.W + j] : 0.0;
          gcol[c] += g * (alpha * T);
          gal += g * (colk[c] - I[c]);
        }
      }
      const double gd = geo ? gal * T * dadd : 0.0;
      const double Gx = gd * ux, Gy = gd * uy;
      if (!hull) {
        acc_r -= gd; acc_x -= Gx; acc_y -= Gy;
      } else {
        const bool pend = geo && gd != 0.0;
        unsigned long long todo = __ballot(pend);
        while (todo) {
          const int e = __shfl(edge, __ffsll((long long)todo) - 1, 64);
          const bool mine = pend && edge == e;
          const double ax = wave_sum(mine ? -(1.0 - t) * Gx : 0.0), ay = wave_sum(mine ? -(1.0 - t) * Gy : 0.0);
          const double bx = wave_sum(mine ? -t * Gx : 0.0), by = wave_sum(mine ? -t * Gy : 0.0);
          if (lane == 0) {
            const int e1 = e + 1 >= nv ? 0 : e + 1;
            double2 a = s_acc[wave][e];
            a.x += ax; a.y += ay;
            s_acc[wave][e] = a;
            double2 b = s_acc[wave][e1];
            b.x += bx; b.y += by;
            s_acc[wave][e1] = b;
          }
          todo &= ~__ballot(mine);
        }
      }
    }
  }
  __syncthreads();
  // the world-vertex gradients (the four wavefronts in order) turned back into the body frame, and what they give the pose
  double vx = 0.0, vy = 0.0, vr = 0.0;
  if (tid < 64) {
    for (int v = lane; v < cap; v += 64) {                 // (cap <= 64: one pass)
      double gx = 0.0, gy = 0.0;
      if (hull && drawn && v < nv) {
#pragma unroll
        for (int q = 0; q < RD_WAVES; ++q) { gx += s_acc[q][v].x; gy += s_acc[q][v].y; }
        const double rx = S.vw[o + v].x - S.cx[k], ry = S.vw[o + v].y - S.cy[k];
        vx = gx; vy = gy; vr = gy * rx - gx * ry;          // dw/drot = left turn of (w - c)
      }
      if (g_verts_local) {
        const double sn = S.sn[k], cs = S.cs[k];
        double2 out = make_double2(cs * gx + sn * gy, -sn * gx + cs * gy);      // (slots >= nverts, circles: zeros)
        *reinterpret_cast<double2*>(g_verts_local + (((size_t)scene * nb + k) * cap + v) * 2) = out;
      }
    }
  }
  double part[8] = {hull ? vr : 0.0, hull ? vx : acc_x, hull ? vy : acc_y, acc_r, gcol[0], gcol[1], gcol[2], gcol[3]};
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const double s = wave_sum(part[q]);
    if (lane == 0) s_red[wave][q] = s;
  }
  __syncthreads();
  if (tid < 8) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < RD_WAVES; ++q) s += s_red[q][tid];
    const size_t body = (size_t)scene * nb + k;
    if (tid < 3) { if (g_p) g_p[body * 3 + tid] = s; }
    else if (tid == 3) { if (g_radius) g_radius[body] = hull ? 0.0 : s; }
    else if (tid - 4 < cam.C) { if (g_colors) g_colors[body * cam.C + (tid - 4)] = (float)s; }
  }
}

// (the static tables of either kernel take less than 12 KB; beyond 64 KB in all the dynamic part is opted in to)
static int launch(const void* fn, long long blocks, size_t lds, void* stream, void** args) {
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
  const dim3 grid((unsigned)blocks);
  if (lds + 12 * 1024 > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return LCP_E_LAUNCH;
  if (hipLaunchKernel(fn, grid, dim3(RD_T), args, lds, (hipStream_t)stream) != hipSuccess) return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace render

bool render_supported(int nb, int nvcap, int scene_verts_max) { return contacts_wide_supported(nb, nvcap, scene_verts_max); }

int render_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind, const double* radius,
                  const double* verts_local, const int32_t* nverts, const double* p, const float* colors, const float* background,
                  const double* thickness, double x0, double y0, double ppm, double w, float* image, int32_t* ids, void* stream) {
  using namespace render;
  if (!render_supported(nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  const long long tiles = (long long)((W + TILE_W - 1) / TILE_W) * ((H + TILE_H - 1) / TILE_H);
  if (tiles > 0x7fffffffLL) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  int ntiles = (int)tiles;
  Cam cam{H, W, C, x0, y0, ppm, w};
  void* args[] = {&nb, &nvcap, &vmax, &ntiles, &cam, &kind, &radius, &verts_local, &nverts, &p, &colors, &background, &thickness, &image, &ids};
  return launch(reinterpret_cast<const void*>(lcp_render_kernel), tiles * B, scene_lds(vmax), stream, args);
}

int render_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind,
                           const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                           const float* colors, const float* background, const double* thickness, double x0, double y0, double ppm,
                           double w, const float* g_image, double* g_p, double* g_radius, double* g_verts_local, float* g_colors,
                           void* stream) {
  using namespace render;
  if (!render_supported(nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  Cam cam{H, W, C, x0, y0, ppm, w};
  void* args[] = {&nb, &nvcap, &vmax, &cam, &kind, &radius, &verts_local, &nverts, &p, &colors, &background, &thickness, &g_image,
                  &g_p, &g_radius, &g_verts_local, &g_colors};
  return launch(reinterpret_cast<const void*>(lcp_render_backward_kernel), (long long)B * nb, scene_lds(vmax), stream, args);
}

}  // namespace lcp
