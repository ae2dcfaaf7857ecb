// lcp_render_marks.hip - the rest of the reference's paint loop on the device: the bodies of lcp_render.hip with the marks Body.draw
// puts on them (the circle's spoke, bodies.py:144-147; the hull's centre dot, :245-247; the rect's diagonals, :295-296) and the joints'
// markers (constraints.py:51-53, 89-92, 117-119, 144-146, 171-173, 202-206; painted after the bodies, world.py:281-282), and their
// backward.  include/lcp_hip.h ("drawing") has the formulas; the bodies' arithmetic is lcp_render_common.h's, shared with lcp_render.hip.
//   segment (A, B, width s)     d = dist(x, AB) - s / 2, alpha = cov(d); A == B: the point A (parameter 0, no division)
//   disc (A, r)                 d = |x - A| - r, alpha = cov(d);  ring of thickness t: alpha = cov(d) - cov(d + t)
//   a frame                     for each body k its GROUP: body k and its mark (order 0: spoke / diagonals under the body, centre dot
//                               over it; order 1: the mark over the body), then the joints' markers, joint 0 first
// Every group lies inside one circle around the body's centre (the body's bounding radius or the mark's, grown by w / 2 and the
// rounding slack), every joint's marker inside one around its own centre: a layer is skipped only where its alpha is exactly 0.
//
// Forward: lcp_render_kernel's mapping (one workgroup per (scene, tile of 16 x 64 pixels), lane = column) with one 64-bit mask of the
// groups and one of the joints that reach the tile.
//
// Backward: ONE launch of workgroups with two roles.  Block (scene, body k) owns body k and its mark, over the group's pixel box:
// g_p, g_radius, g_verts_local, g_colors, g_mark_colors of that body.  Block (scene, joint j) owns joint j's marker over its own box:
// g_joint_colors, g_jrot1, g_jr1 of that joint and its pull on its two bodies, which goes to the caller's workspace g_p_joints[B,nj,2,3].
// Each recomputes the transmittance of everything above and the colour below from the groups and joints whose circles meet its own.  A
// second, stream-ordered launch (one thread per body) adds the workspace's slots to g_p joint by joint.  No atomics; every output
// element is owned by one workgroup; register sums in pixel order, xor butterflies, the four wavefronts in order: the same bits every
// run.
#include "lcp_render_common.h"

namespace lcp {
namespace render {

constexpr int MAXJ = 64;                                   // joints per scene
constexpr int MARK_SPOKE = 1, MARK_CENTRE = 2, MARK_DIAGONALS = 3;
constexpr int JT_JOINT = 1, JT_FIXED = 2, JT_XCON = 3, JT_YCON = 4, JT_ROTCON = 5, JT_TOTAL = 6;      // physics/joints.py
constexpr int PR_NONE = 0, PR_LINE = 1, PR_DOT = 2, PR_JLINE = 3, PR_RING = 4;      // segment of line_w, disc of dot_r, segment of joint_w, ring

struct MarkArgs {
  int nj, order;
  double line_w, dot_r, joint_w, joint_r;
  const int32_t* mark; const float* mark_colors;
  const int32_t *jtype, *jb1, *jb2; const double *jr1, *jrot1; const float* joint_colors;
};

// The marks and markers of a scene in LDS: per body two primitives (type, A, B) and a colour, per joint three.
struct Marks {
  int* mcode; int* mtype; double4* mseg; float* mcol; double* greach;       // [MAXB], [MAXB][2], [MAXB][2], [MAXB][4], the group's reach
  int* jkind; int* jtype; double4* jseg; float* jcol;                        // [MAXJ], [MAXJ][3], [MAXJ][3], [MAXJ][4]
  double *jcx, *jcy, *jreach;                                                // the marker's circle (reach < 0: not drawn)
};

#define LCP_RD_MARK_TABLES(M)                                                                                                   \
  __shared__ int s_mcode[MAXB], s_mtype[MAXB * 2], s_jkind[MAXJ], s_jtype[MAXJ * 3];                                            \
  __shared__ double4 s_mseg[MAXB * 2], s_jseg[MAXJ * 3];                                                                        \
  __shared__ float s_mcol[MAXB * 4], s_jcol[MAXJ * 4];                                                                          \
  __shared__ double s_greach[MAXB], s_jcx[MAXJ], s_jcy[MAXJ], s_jreach[MAXJ];                                                   \
  Marks M;                                                                                                                      \
  M.mcode = s_mcode; M.mtype = s_mtype; M.mseg = s_mseg; M.mcol = s_mcol; M.greach = s_greach;                                  \
  M.jkind = s_jkind; M.jtype = s_jtype; M.jseg = s_jseg; M.jcol = s_jcol; M.jcx = s_jcx; M.jcy = s_jcy; M.jreach = s_jreach

// After stage_scene: the primitives of every body's mark (lanes of wavefront 0) and of every joint's marker (wavefront 1).  A code
// that does not fit its body, a FIXED joint without a second body, a body index outside the scene: no primitive.
__device__ __forceinline__ void stage_marks(const Scene& S, const Marks& M, const MarkArgs& A, bool ok, int scene, int nb, int C, double w) {
  const int tid = threadIdx.x;
  if (tid < nb) {
    const int k = tid;
    int code = ok && A.mark ? A.mark[(size_t)scene * nb + k] : 0;
    const bool hull = S.kind[k] != 0;
    const int o = S.off[k], nv = S.off[k + 1] - o;
    if (code == MARK_SPOKE ? hull : code == MARK_DIAGONALS ? !(hull && nv == 4) : code != MARK_CENTRE) code = 0;
    const double cx = S.cx[k], cy = S.cy[k];
    int t0 = PR_NONE, t1 = PR_NONE;
    double4 g0 = make_double4(0.0, 0.0, 0.0, 0.0), g1 = g0;
    double ext = -1.0;
    if (code == MARK_SPOKE) {
      const double r = S.rad[k];
      t0 = PR_LINE; g0 = make_double4(cx, cy, cx + r * S.cs[k], cy + r * S.sn[k]);
      ext = fabs(r) + 0.5 * A.line_w;
    } else if (code == MARK_CENTRE) {
      t0 = PR_DOT; g0 = make_double4(cx, cy, cx, cy);
      ext = A.dot_r;
    } else if (code == MARK_DIAGONALS) {
      const double2 w0 = S.vw[o], w1 = S.vw[o + 1], w2 = S.vw[o + 2], w3 = S.vw[o + 3];
      t0 = PR_LINE; g0 = make_double4(w0.x, w0.y, w2.x, w2.y);
      t1 = PR_LINE; g1 = make_double4(w1.x, w1.y, w3.x, w3.y);
      double r = 0.0;
      for (int q = 0; q < 4; ++q) { const double dx = S.vw[o + q].x - cx, dy = S.vw[o + q].y - cy; r = fmax(r, sqrt(dx * dx + dy * dy)); }
      ext = r + 0.5 * A.line_w;
    }
    M.mcode[k] = code; M.mtype[2 * k] = t0; M.mtype[2 * k + 1] = t1; M.mseg[2 * k] = g0; M.mseg[2 * k + 1] = g1;
#pragma unroll
    for (int c = 0; c < 4; ++c) M.mcol[k * 4 + c] = code != 0 && c < C ? A.mark_colors[((size_t)scene * nb + k) * C + c] : 0.0f;
    double reach = S.reach[k];
    if (ext >= 0.0) reach = fmax(reach, ext + 0.5 * w + 1e-9 * (fabs(cx) + fabs(cy) + ext + w));
    M.greach[k] = reach;
  }
  if (tid >= 64 && tid < 64 + MAXJ) {
    const int j = tid - 64;
    int kind = 0;
    int t[3] = {PR_NONE, PR_NONE, PR_NONE};
    double4 g[3];
    g[0] = g[1] = g[2] = make_double4(0.0, 0.0, 0.0, 0.0);
    double cx = 0.0, cy = 0.0, ext = -1.0;
    if (ok && j < A.nj) {
      const size_t jo = (size_t)scene * A.nj + j;
      const int jt = A.jtype[jo], b1 = A.jb1[jo], b2 = A.jb2[jo];
      if (b1 >= 0 && b1 < nb) {
        const double x1 = S.cx[b1], y1 = S.cy[b1], R = A.joint_r;
        const double4 hor = make_double4(x1 - R, y1, x1 + R, y1), ver = make_double4(x1, y1 - R, x1, y1 + R), at = make_double4(x1, y1, x1, y1);
        cx = x1; cy = y1;
        if (jt == JT_JOINT) {
          const double r1 = A.jr1[jo], th = A.jrot1[jo];
          cx = x1 + r1 * cos(th); cy = y1 + r1 * sin(th);
          kind = jt; t[0] = PR_DOT; g[0] = make_double4(cx, cy, cx, cy); ext = A.dot_r;
        } else if (jt == JT_FIXED) {
          if (b2 >= 0 && b2 < nb) {
            const double x2 = S.cx[b2], y2 = S.cy[b2];
            kind = jt; t[0] = PR_JLINE; g[0] = make_double4(x1, y1, x2, y2);
            cx = 0.5 * (x1 + x2); cy = 0.5 * (y1 + y2);
            const double dx = x2 - x1, dy = y2 - y1;
            ext = 0.5 * sqrt(dx * dx + dy * dy) + 0.5 * A.joint_w;
          }
        } else if (jt == JT_YCON) {
          kind = jt; t[0] = PR_JLINE; g[0] = hor; ext = R + 0.5 * A.joint_w;
        } else if (jt == JT_XCON) {
          kind = jt; t[0] = PR_JLINE; g[0] = ver; ext = R + 0.5 * A.joint_w;
        } else if (jt == JT_ROTCON) {
          kind = jt; t[0] = PR_RING; g[0] = at; ext = R;
        } else if (jt == JT_TOTAL) {
          kind = jt; t[0] = PR_RING; g[0] = at; t[1] = PR_JLINE; g[1] = hor; t[2] = PR_JLINE; g[2] = ver; ext = R + 0.5 * A.joint_w;
        }
      }
    }
    M.jkind[j] = kind;
#pragma unroll
    for (int q = 0; q < 3; ++q) { M.jtype[3 * j + q] = t[q]; M.jseg[3 * j + q] = g[q]; }
#pragma unroll
    for (int c = 0; c < 4; ++c) M.jcol[j * 4 + c] = kind != 0 && c < C ? A.joint_colors[((size_t)scene * A.nj + j) * C + c] : 0.0f;
    M.jcx[j] = cx; M.jcy[j] = cy;
    M.jreach[j] = kind != 0 ? ext + 0.5 * w + 1e-9 * (fabs(cx) + fabs(cy) + ext + w) : -1.0;
  }
  __syncthreads();
}

// alpha of a primitive at x with its derivative data: dadd = d alpha / dd, u = dd/dx (0 where the distance is 0), t = the segment's
// parameter (dd/dA = -(1 - t) u, dd/dB = -t u)
__device__ __forceinline__ double prim_alpha(int type, double4 g, const MarkArgs& A, double px, double py, double iw, double& dadd,
                                             double& ux, double& uy, double& t) {
  const double qx = px - g.x, qy = py - g.y;
  double rx = qx, ry = qy;
  t = 0.0;
  if (type == PR_LINE || type == PR_JLINE) {
    const double ex = g.z - g.x, ey = g.w - g.y;
    const double l2 = ex * ex + ey * ey;
    const double s = l2 > 0.0 ? (qx * ex + qy * ey) / l2 : 0.0;
    t = fmin(fmax(s, 0.0), 1.0);
    rx = qx - t * ex; ry = qy - t * ey;
  }
  const double len = sqrt(rx * rx + ry * ry);
  const double id = len > 0.0 ? 1.0 / len : 0.0;
  ux = rx * id; uy = ry * id;
  const double d = len - (type == PR_LINE ? 0.5 * A.line_w : type == PR_JLINE ? 0.5 * A.joint_w : type == PR_DOT ? A.dot_r : A.joint_r);
  if (type == PR_RING) {
    dadd = dcov(d, iw) - dcov(d + A.line_w, iw);
    return cov(d, iw) - cov(d + A.line_w, iw);
  }
  dadd = dcov(d, iw);
  return cov(d, iw);
}

__device__ __forceinline__ bool within(double cx, double cy, double r, double px, double py) {
  const double dx = px - cx, dy = py - cy;
  return !(dx * dx + dy * dy > r * r);
}

__device__ __forceinline__ void over(double I[4], double a, const float* col) {
#pragma unroll
  for (int c = 0; c < 4; ++c) I[c] = I[c] * (1.0 - a) + a * (double)col[c];
}

// whether the mark of body k lies under it
__device__ __forceinline__ bool mark_under(const Marks& M, const MarkArgs& A, int k) { return A.order == 0 && M.mcode[k] != MARK_CENTRE; }

// Group k (body k and its mark, in the frame's order) painted over I at the pixels of this wavefront; T is multiplied by the group's
// transmittance, top becomes k where the body's silhouette covers the pixel.  The skips are per wavefront.
__device__ __forceinline__ void group_over(const Scene& S, const Marks& M, const MarkArgs& A, int k, double px, double py, bool valid,
                                           double iw, double I[4], double& T, int& top) {
  const bool near = valid && within(S.cx[k], S.cy[k], M.greach[k], px, py);
  if (!__any(near)) return;
  double ab = 0.0;
  const bool bnear = near && S.reach[k] >= 0.0 && within_reach(S, k, px, py);
  if (__any(bnear)) {
    int edge; double t, ux, uy;
    const double dk = body_sd(S, k, px, py, edge, t, ux, uy);
    if (bnear) {
      ab = alpha_of(dk, S.thick[k], iw);
      if (dk <= 0.0) top = k;
    }
  }
  double am[2] = {0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int type = M.mtype[2 * k + q];
    if (type != PR_NONE) {
      double dadd, ux, uy, t;
      const double a = prim_alpha(type, M.mseg[2 * k + q], A, px, py, iw, dadd, ux, uy, t);
      am[q] = near ? a : 0.0;
    }
  }
  const bool under = mark_under(M, A, k);
  if (under) { over(I, am[0], M.mcol + 4 * k); over(I, am[1], M.mcol + 4 * k); }
  over(I, ab, S.col + 4 * k);
  if (!under) { over(I, am[0], M.mcol + 4 * k); over(I, am[1], M.mcol + 4 * k); }
  T *= (1.0 - ab) * ((1.0 - am[0]) * (1.0 - am[1]));
}

// Joint j's marker painted over I; T is multiplied by its transmittance.
__device__ __forceinline__ void joint_over(const Marks& M, const MarkArgs& A, int j, double px, double py, bool valid, double iw,
                                           double I[4], double& T) {
  const bool near = valid && within(M.jcx[j], M.jcy[j], M.jreach[j], px, py);
  if (!__any(near)) return;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int type = M.jtype[3 * j + q];
    if (type == PR_NONE) break;
    double dadd, ux, uy, t;
    double a = prim_alpha(type, M.jseg[3 * j + q], A, px, py, iw, dadd, ux, uy, t);
    a = near ? a : 0.0;
    over(I, a, M.jcol + 4 * j);
    T *= 1.0 - a;
  }
}

// the circles (centre, reach; reach < 0: nothing) that reach the rectangle [xa, xb] x [ya, yb] / that meet the circle (x, y, r)
__device__ __forceinline__ bool reaches_box(double cx, double cy, double r, double xa, double xb, double ya, double yb) {
  const double dx = fmax(fmax(xa - cx, cx - xb), 0.0), dy = fmax(fmax(ya - cy, cy - yb), 0.0);
  return r >= 0.0 && !(dx * dx + dy * dy > r * r);
}
__device__ __forceinline__ bool meets(double cx, double cy, double r, double x, double y, double r2) {
  const double dx = cx - x, dy = cy - y, s = r + r2;
  return r >= 0.0 && !(dx * dx + dy * dy > s * s);
}

__global__ void __launch_bounds__(RD_T) lcp_render_marks_kernel(int nb, int cap, int vmax, int tiles, Cam cam, MarkArgs A, const int32_t* kind,
                                                               const double* radius, const double* verts_local, const int32_t* nverts,
                                                               const double* p, const float* colors, const float* background,
                                                               const double* thickness, float* image, int32_t* ids) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  LCP_RD_MARK_TABLES(M);
  __shared__ unsigned long long s_mask[2];
  const int scene = blockIdx.x / tiles, tile = blockIdx.x - scene * tiles;
  const int tiles_x = (cam.W + TILE_W - 1) / TILE_W;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ok = stage_scene(S, scene, nb, cap, vmax, cam.C, kind, radius, verts_local, nverts, p, colors, thickness, cam.w);
  stage_marks(S, M, A, ok, scene, nb, cam.C, cam.w);
  const int i0 = ty * TILE_H, j0 = tx * TILE_W;
  const int i1 = min(i0 + TILE_H, cam.H) - 1, j1 = min(j0 + TILE_W, cam.W) - 1;      // the tile's last row and column
  if (threadIdx.x < 128) {
    // wavefront 0: the groups, wavefront 1: the joints that can reach the rectangle of this tile's pixel centres
    const double xa = cam.x0 + (j0 + 0.5) / cam.ppm, xb = cam.x0 + (j1 + 0.5) / cam.ppm;
    const double ya = cam.y0 + (i0 + 0.5) / cam.ppm, yb = cam.y0 + (i1 + 0.5) / cam.ppm;
    bool vis = false;
    if (wave == 0) vis = ok && lane < nb && reaches_box(S.cx[lane], S.cy[lane], M.greach[lane], xa, xb, ya, yb);
    else vis = ok && lane < A.nj && reaches_box(M.jcx[lane], M.jcy[lane], M.jreach[lane], xa, xb, ya, yb);
    const unsigned long long m = __ballot(vis);
    if (lane == 0) s_mask[wave] = m;
  }
  __syncthreads();
  const unsigned long long mask = s_mask[0], jmask = s_mask[1];
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
    double T = 1.0;
    int top = -1;
    for (unsigned long long m = mask; m; m &= m - 1) group_over(S, M, A, __ffsll((long long)m) - 1, px, py, valid, iw, I, T, top);
    if (image)
      for (unsigned long long m = jmask; m; m &= m - 1) joint_over(M, A, __ffsll((long long)m) - 1, px, py, valid, iw, I, T);
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

struct MarkGrads {
  double *g_p, *g_radius, *g_verts_local; float *g_colors, *g_mark_colors, *g_joint_colors; double *g_jrot1, *g_jr1, *g_p_joints;
};

// the pixel box of the circle (cx, cy, reach), clamped to the image while still in floating point (a centre at 1e15, a non-finite
// bound: an empty box or the whole image, never an index outside it); reach < 0: empty
__device__ __forceinline__ void pixel_box(const Cam& cam, double cx, double cy, double reach, int& jlo, int& jhi, int& ilo, int& ihi) {
  const bool drawn = reach >= 0.0;
  const double fj0 = fmin(fmax(floor((cx - reach - cam.x0) * cam.ppm - 0.5) - 1.0, 0.0), (double)cam.W);
  const double fj1 = fmin(fmax(ceil((cx + reach - cam.x0) * cam.ppm - 0.5) + 1.0, -1.0), (double)cam.W - 1.0);
  const double fi0 = fmin(fmax(floor((cy - reach - cam.y0) * cam.ppm - 0.5) - 1.0, 0.0), (double)cam.H);
  const double fi1 = fmin(fmax(ceil((cy + reach - cam.y0) * cam.ppm - 0.5) + 1.0, -1.0), (double)cam.H - 1.0);
  jlo = drawn ? (int)fj0 : 0; jhi = drawn ? (int)fj1 : -1; ilo = drawn ? (int)fi0 : 0; ihi = drawn ? (int)fi1 : -1;
}

// blocks [0, body_blocks): (scene, body); the rest: (scene, joint)
__global__ void __launch_bounds__(RD_T) lcp_render_marks_backward_kernel(int nb, int cap, int vmax, int body_blocks, Cam cam, MarkArgs A,
                                                                        const int32_t* kind, const double* radius,
                                                                        const double* verts_local, const int32_t* nverts, const double* p,
                                                                        const float* colors, const float* background,
                                                                        const double* thickness, const float* g_image, MarkGrads G) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  LCP_RD_MARK_TABLES(M);
  __shared__ unsigned long long s_mask[2];
  __shared__ double2 s_acc[RD_WAVES][ctw::NV];             // per wavefront: the gradient of each world vertex of this body
  __shared__ double s_red[RD_WAVES][12];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool body_role = (int)blockIdx.x < body_blocks;
  const int unit = body_role ? blockIdx.x : blockIdx.x - body_blocks;
  const int per = body_role ? nb : A.nj;
  const int scene = unit / per, k = unit - scene * per;    // k: the body, or the joint
  const bool ok = stage_scene(S, scene, nb, cap, vmax, cam.C, kind, radius, verts_local, nverts, p, colors, thickness, cam.w);
  stage_marks(S, M, A, ok, scene, nb, cam.C, cam.w);
  const double ocx = body_role ? S.cx[k] : M.jcx[k], ocy = body_role ? S.cy[k] : M.jcy[k];
  const double oreach = !ok ? -1.0 : body_role ? M.greach[k] : M.jreach[k];
  if (tid < 128) {
    // the groups (wavefront 0) and the joints (wavefront 1) whose circles meet this unit's
    bool ov = false;
    if (oreach >= 0.0) {
      if (wave == 0) ov = lane < nb && meets(S.cx[lane], S.cy[lane], M.greach[lane], ocx, ocy, oreach);
      else ov = lane < A.nj && meets(M.jcx[lane], M.jcy[lane], M.jreach[lane], ocx, ocy, oreach);
    }
    const unsigned long long m = __ballot(ov);
    if (lane == 0) s_mask[wave] = m;
  }
  for (int v = lane; v < ctw::NV; v += 64) s_acc[wave][v] = make_double2(0.0, 0.0);
  __syncthreads();
  const unsigned long long gmask = s_mask[0], jmask = s_mask[1];
  const unsigned long long lower = (1ull << k) - 1, upper = k == 63 ? 0ull : ~((2ull << k) - 1);
  const double iw = 1.0 / cam.w;
  int jlo, jhi, ilo, ihi;
  pixel_box(cam, ocx, ocy, oreach, jlo, jhi, ilo, ihi);
  double bg[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bg[c] = c < cam.C ? (double)background[c] : 0.0;

  if (body_role) {
    const unsigned long long below = gmask & lower, above = gmask & upper;
    const bool body_drawn = S.reach[k] >= 0.0;
    const bool hull = S.kind[k] != 0;
    const int o = S.off[k], nv = S.off[k + 1] - o;
    const double th = S.thick[k];
    const int code = M.mcode[k];
    const bool under = mark_under(M, A, k);
    const int type0 = M.mtype[2 * k], type1 = M.mtype[2 * k + 1];
    const double4 seg0 = M.mseg[2 * k], seg1 = M.mseg[2 * k + 1];
    const double sn = S.sn[k], cs = S.cs[k], rad = S.rad[k];
    double colk[4], colm[4], gcol[4] = {0.0, 0.0, 0.0, 0.0}, gmcol[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) { colk[c] = (double)S.col[k * 4 + c]; colm[c] = (double)M.mcol[k * 4 + c]; }
    double acc_r = 0.0, acc_x = 0.0, acc_y = 0.0, acc_rot = 0.0;          // what does not go through the vertices: circle, spoke, dot
    double2 dg[4];                                                         // the diagonals' pull on the four world vertices
#pragma unroll
    for (int q = 0; q < 4; ++q) dg[q] = make_double2(0.0, 0.0);
#pragma unroll 1
    for (int ib = ilo; ib <= ihi; ib += RD_WAVES) {
      const int i = ib + wave;
      const double py = cam.y0 + (i + 0.5) / cam.ppm;
#pragma unroll 1
      for (int jb = jlo; jb <= jhi; jb += 64) {
        const int j = jb + lane;
        const bool valid = i <= ihi && j <= jhi;
        const double px = cam.x0 + (j + 0.5) / cam.ppm;
        const bool near = valid && within(ocx, ocy, oreach, px, py);
        if (!__any(near)) continue;
        // this group's own layers: the body, then the mark's primitives
        int edge = 0; double t = 0.0, ux = 0.0, uy = 0.0, ab = 0.0, dab = 0.0;
        const bool bnear = near && body_drawn && within_reach(S, k, px, py);
        if (__any(bnear)) {
          const double d = body_sd(S, k, px, py, edge, t, ux, uy);
          if (bnear) {
            ab = alpha_of(d, th, iw);
            dab = th > 0.0 ? dcov(d, iw) - dcov(d + th, iw) : dcov(d, iw);
          }
        }
        double a0 = 0.0, da0 = 0.0, u0x = 0.0, u0y = 0.0, t0 = 0.0, a1 = 0.0, da1 = 0.0, u1x = 0.0, u1y = 0.0, t1 = 0.0;
        if (type0 != PR_NONE) {
          a0 = prim_alpha(type0, seg0, A, px, py, iw, da0, u0x, u0y, t0);
          if (!near) { a0 = 0.0; da0 = 0.0; }
        }
        if (type1 != PR_NONE) {
          a1 = prim_alpha(type1, seg1, A, px, py, iw, da1, u1x, u1y, t1);
          if (!near) { a1 = 0.0; da1 = 0.0; }
        }
        const bool active = near && (ab != 0.0 || dab != 0.0 || a0 != 0.0 || da0 != 0.0 || a1 != 0.0 || da1 != 0.0);
        if (!__any(active)) continue;
        double T = 1.0, dump[4] = {0.0, 0.0, 0.0, 0.0};
        int top;
        for (unsigned long long m = above; m; m &= m - 1) group_over(S, M, A, __ffsll((long long)m) - 1, px, py, active, iw, dump, T, top);
        for (unsigned long long m = jmask; m; m &= m - 1) joint_over(M, A, __ffsll((long long)m) - 1, px, py, active, iw, dump, T);
        const bool geo = active && (dab != 0.0 || da0 != 0.0 || da1 != 0.0);
        double I[4] = {bg[0], bg[1], bg[2], bg[3]};
        if (__any(geo)) {
          double Tb = 1.0;
          for (unsigned long long m = below; m; m &= m - 1) group_over(S, M, A, __ffsll((long long)m) - 1, px, py, geo, iw, I, Tb, top);
        }
        // transmittance above and colour below each own layer, in the group's order
        double Tbody, T0, T1, Ib[4], I0[4], I1[4];
        if (under) {
          Tbody = T; T1 = T * (1.0 - ab); T0 = T1 * (1.0 - a1);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            I0[c] = I[c]; I1[c] = I0[c] * (1.0 - a0) + a0 * colm[c]; Ib[c] = I1[c] * (1.0 - a1) + a1 * colm[c];
          }
        } else {
          T1 = T; T0 = T * (1.0 - a1); Tbody = T0 * (1.0 - a0);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            Ib[c] = I[c]; I0[c] = Ib[c] * (1.0 - ab) + ab * colk[c]; I1[c] = I0[c] * (1.0 - a0) + a0 * colm[c];
          }
        }
        double galb = 0.0, gal0 = 0.0, gal1 = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < cam.C) {
            const double g = active ? (double)g_image[(((size_t)scene * cam.C + c) * cam.H + i) * cam.W + j] : 0.0;
            gcol[c] += g * (ab * Tbody);
            gmcol[c] += g * (a0 * T0 + a1 * T1);
            galb += g * (colk[c] - Ib[c]);
            gal0 += g * (colm[c] - I0[c]);
            gal1 += g * (colm[c] - I1[c]);
          }
        }
        const double gd = geo && dab != 0.0 ? galb * Tbody * dab : 0.0;
        const double gd0 = geo && da0 != 0.0 ? gal0 * T0 * da0 : 0.0;
        const double gd1 = geo && da1 != 0.0 ? gal1 * T1 * da1 : 0.0;
        // the mark
        if (code == MARK_SPOKE) {                          // A = c, B = c + rad (cos rot, sin rot)
          const double bx = -t0 * gd0 * u0x, by = -t0 * gd0 * u0y;
          acc_x -= gd0 * u0x; acc_y -= gd0 * u0y;
          acc_rot += rad * (cs * by - sn * bx);
          acc_r += cs * bx + sn * by;
        } else if (code == MARK_CENTRE) {
          acc_x -= gd0 * u0x; acc_y -= gd0 * u0y;
        } else if (code == MARK_DIAGONALS) {               // w0 - w2 and w1 - w3
          dg[0].x -= (1.0 - t0) * gd0 * u0x; dg[0].y -= (1.0 - t0) * gd0 * u0y;
          dg[2].x -= t0 * gd0 * u0x; dg[2].y -= t0 * gd0 * u0y;
          dg[1].x -= (1.0 - t1) * gd1 * u1x; dg[1].y -= (1.0 - t1) * gd1 * u1y;
          dg[3].x -= t1 * gd1 * u1x; dg[3].y -= t1 * gd1 * u1y;
        }
        // the body
        const double Gx = gd * ux, Gy = gd * uy;
        if (!hull) {
          acc_r -= gd; acc_x -= Gx; acc_y -= Gy;
        } else {
          const bool pend = gd != 0.0;
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
    if (code == MARK_DIAGONALS) {                          // (a hull of exactly four vertices; uniform over the workgroup)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double sx = wave_sum(dg[q].x), sy = wave_sum(dg[q].y);
        if (lane == 0) { double2 a = s_acc[wave][q]; a.x += sx; a.y += sy; s_acc[wave][q] = a; }
      }
    }
    __syncthreads();
    // the world-vertex gradients (the four wavefronts in order) turned back into the body frame, and what they give the pose
    double vx = 0.0, vy = 0.0, vr = 0.0;
    if (tid < 64) {
      for (int v = lane; v < cap; v += 64) {               // (cap <= 64: one pass)
        double gx = 0.0, gy = 0.0;
        if (hull && ok && v < nv) {
#pragma unroll
          for (int q = 0; q < RD_WAVES; ++q) { gx += s_acc[q][v].x; gy += s_acc[q][v].y; }
          const double rx = S.vw[o + v].x - S.cx[k], ry = S.vw[o + v].y - S.cy[k];
          vx = gx; vy = gy; vr = gy * rx - gx * ry;        // dw/drot = left turn of (w - c)
        }
        if (G.g_verts_local) {
          double2 out = make_double2(cs * gx + sn * gy, -sn * gx + cs * gy);        // (slots >= nverts, circles: zeros)
          *reinterpret_cast<double2*>(G.g_verts_local + (((size_t)scene * nb + k) * cap + v) * 2) = out;
        }
      }
    }
    double part[12] = {vr + acc_rot, vx + acc_x, vy + acc_y, acc_r, gcol[0], gcol[1], gcol[2], gcol[3], gmcol[0], gmcol[1], gmcol[2], gmcol[3]};
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      const double s = wave_sum(part[q]);
      if (lane == 0) s_red[wave][q] = s;
    }
    __syncthreads();
    if (tid < 12) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < RD_WAVES; ++q) s += s_red[q][tid];
      const size_t body = (size_t)scene * nb + k;
      if (tid < 3) { if (G.g_p) G.g_p[body * 3 + tid] = s; }
      else if (tid == 3) { if (G.g_radius) G.g_radius[body] = hull ? 0.0 : s; }
      else if (tid < 8) { if (G.g_colors && tid - 4 < cam.C) G.g_colors[body * cam.C + (tid - 4)] = (float)s; }
      else if (G.g_mark_colors && tid - 8 < cam.C) G.g_mark_colors[body * cam.C + (tid - 8)] = (float)s;
    }
    return;
  }

  // ---- the joint's role ----
  {
    const unsigned long long below = jmask & lower, above = jmask & upper;
    const int jt = M.jkind[k];
    int type[3]; double4 seg[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { type[q] = M.jtype[3 * k + q]; seg[q] = M.jseg[3 * k + q]; }
    const size_t jo = (size_t)scene * A.nj + k;
    double r1 = 0.0, sn = 0.0, cs = 0.0;
    if (jt == JT_JOINT) { r1 = A.jr1[jo]; const double thj = A.jrot1[jo]; sn = sin(thj); cs = cos(thj); }
    double colj[4], gcol[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) colj[c] = (double)M.jcol[k * 4 + c];
    double g1x = 0.0, g1y = 0.0, g2x = 0.0, g2y = 0.0, gjr = 0.0, gjrot = 0.0;
#pragma unroll 1
    for (int ib = ilo; ib <= ihi; ib += RD_WAVES) {
      const int i = ib + wave;
      const double py = cam.y0 + (i + 0.5) / cam.ppm;
#pragma unroll 1
      for (int jb = jlo; jb <= jhi; jb += 64) {
        const int j = jb + lane;
        const bool valid = i <= ihi && j <= jhi;
        const double px = cam.x0 + (j + 0.5) / cam.ppm;
        const bool near = valid && within(ocx, ocy, oreach, px, py);
        if (!__any(near)) continue;
        double a[3] = {0.0, 0.0, 0.0}, da[3] = {0.0, 0.0, 0.0}, ux[3] = {0.0, 0.0, 0.0}, uy[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (type[q] != PR_NONE) {
            a[q] = prim_alpha(type[q], seg[q], A, px, py, iw, da[q], ux[q], uy[q], t[q]);
            if (!near) { a[q] = 0.0; da[q] = 0.0; }
          }
        }
        const bool active = near && (a[0] != 0.0 || da[0] != 0.0 || a[1] != 0.0 || da[1] != 0.0 || a[2] != 0.0 || da[2] != 0.0);
        if (!__any(active)) continue;
        double T = 1.0, dump[4] = {0.0, 0.0, 0.0, 0.0};
        for (unsigned long long m = above; m; m &= m - 1) joint_over(M, A, __ffsll((long long)m) - 1, px, py, active, iw, dump, T);
        const bool geo = active && (da[0] != 0.0 || da[1] != 0.0 || da[2] != 0.0);
        double I[4] = {bg[0], bg[1], bg[2], bg[3]};
        if (__any(geo)) {
          double Tb = 1.0;
          int top;
          for (unsigned long long m = gmask; m; m &= m - 1) group_over(S, M, A, __ffsll((long long)m) - 1, px, py, geo, iw, I, Tb, top);
          for (unsigned long long m = below; m; m &= m - 1) joint_over(M, A, __ffsll((long long)m) - 1, px, py, geo, iw, I, Tb);
        }
        double Tq[3], gal[3] = {0.0, 0.0, 0.0};
        Tq[2] = T; Tq[1] = Tq[2] * (1.0 - a[2]); Tq[0] = Tq[1] * (1.0 - a[1]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c < cam.C) {
            const double g = active ? (double)g_image[(((size_t)scene * cam.C + c) * cam.H + i) * cam.W + j] : 0.0;
            const double I0 = I[c], I1 = I0 * (1.0 - a[0]) + a[0] * colj[c], I2 = I1 * (1.0 - a[1]) + a[1] * colj[c];
            gcol[c] += g * (a[0] * Tq[0] + a[1] * Tq[1] + a[2] * Tq[2]);
            gal[0] += g * (colj[c] - I0); gal[1] += g * (colj[c] - I1); gal[2] += g * (colj[c] - I2);
          }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double gd = geo && da[q] != 0.0 ? gal[q] * Tq[q] * da[q] : 0.0;
          const double Gx = -gd * ux[q], Gy = -gd * uy[q];                      // the pull on the whole primitive
          if (jt == JT_FIXED) {                                                 // A = c_b1, B = c_b2
            g1x += (1.0 - t[q]) * Gx; g1y += (1.0 - t[q]) * Gy;
            g2x += t[q] * Gx; g2y += t[q] * Gy;
          } else {
            g1x += Gx; g1y += Gy;
            if (jt == JT_JOINT) { gjr += cs * Gx + sn * Gy; gjrot += r1 * (cs * Gy - sn * Gx); }
          }
        }
      }
    }
    double part[10] = {g1x, g1y, g2x, g2y, gjrot, gjr, gcol[0], gcol[1], gcol[2], gcol[3]};
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      const double s = wave_sum(part[q]);
      if (lane == 0) s_red[wave][q] = s;
    }
    __syncthreads();
    if (tid < 10) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < RD_WAVES; ++q) s += s_red[q][tid];
      if (tid < 4) {
        if (G.g_p_joints) {
          double* slot = G.g_p_joints + (jo * 2 + (tid >> 1)) * 3;
          slot[1 + (tid & 1)] = s;
          if ((tid & 1) == 0) slot[0] = 0.0;                                    // (no marker turns with a body)
        }
      }
      else if (tid == 4) { if (G.g_jrot1) G.g_jrot1[jo] = s; }
      else if (tid == 5) { if (G.g_jr1) G.g_jr1[jo] = s; }
      else if (G.g_joint_colors && tid - 6 < cam.C) G.g_joint_colors[jo * cam.C + (tid - 6)] = (float)s;
    }
  }
}

// g_p[b,k] += the slots of the joints that hold body k, joint by joint: one thread per body
__global__ void __launch_bounds__(RD_T) lcp_render_marks_gather_kernel(long long bodies, int nb, int nj, const int32_t* jb1, const int32_t* jb2,
                                                                      const double* g_p_joints, double* g_p) {
  const long long body = (long long)blockIdx.x * RD_T + threadIdx.x;
  if (body >= bodies) return;
  const long long scene = body / nb;
  const int k = (int)(body - scene * nb);
  double s0 = g_p[body * 3], s1 = g_p[body * 3 + 1], s2 = g_p[body * 3 + 2];
  for (int j = 0; j < nj; ++j) {
    const size_t jo = (size_t)scene * nj + j;
    const int b[2] = {jb1[jo], jb2[jo]};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (b[q] == k) {
        const double* slot = g_p_joints + (jo * 2 + q) * 3;
        s0 += slot[0]; s1 += slot[1]; s2 += slot[2];
      }
    }
  }
  g_p[body * 3] = s0; g_p[body * 3 + 1] = s1; g_p[body * 3 + 2] = s2;
}

// (the static tables of either kernel take less than 32 KB; beyond 64 KB in all the dynamic part is opted in to)
static int launch(const void* fn, long long blocks, size_t lds, void* stream, void** args) {
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
  const dim3 grid((unsigned)blocks);
  if (lds + 32 * 1024 > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return LCP_E_LAUNCH;
  if (hipLaunchKernel(fn, grid, dim3(RD_T), args, lds, (hipStream_t)stream) != hipSuccess) return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace render

int render_marks_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind, const double* radius,
                        const double* verts_local, const int32_t* nverts, const double* p, const float* colors, const float* background,
                        const double* thickness, double x0, double y0, double ppm, double w, const RenderMarks& mk, float* image,
                        int32_t* ids, void* stream) {
  using namespace render;
  if (!render_supported(nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  const long long tiles = (long long)((W + TILE_W - 1) / TILE_W) * ((H + TILE_H - 1) / TILE_H);
  if (tiles > 0x7fffffffLL) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  int ntiles = (int)tiles;
  Cam cam{H, W, C, x0, y0, ppm, w};
  MarkArgs A{mk.nj, mk.order, mk.line_w, mk.dot_r, mk.joint_w, mk.joint_r, mk.mark, mk.mark_colors, mk.jtype, mk.jb1, mk.jb2, mk.jr1, mk.jrot1,
             mk.joint_colors};
  void* args[] = {&nb, &nvcap, &vmax, &ntiles, &cam, &A, &kind, &radius, &verts_local, &nverts, &p, &colors, &background, &thickness, &image, &ids};
  return launch(reinterpret_cast<const void*>(lcp_render_marks_kernel), tiles * B, scene_lds(vmax), stream, args);
}

int render_marks_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind,
                                 const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                 const float* colors, const float* background, const double* thickness, double x0, double y0, double ppm,
                                 double w, const RenderMarks& mk, const float* g_image, double* g_p, double* g_radius,
                                 double* g_verts_local, float* g_colors, float* g_mark_colors, float* g_joint_colors, double* g_jrot1,
                                 double* g_jr1, double* g_p_joints, void* stream) {
  using namespace render;
  if (!render_supported(nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  Cam cam{H, W, C, x0, y0, ppm, w};
  MarkArgs A{mk.nj, mk.order, mk.line_w, mk.dot_r, mk.joint_w, mk.joint_r, mk.mark, mk.mark_colors, mk.jtype, mk.jb1, mk.jb2, mk.jr1, mk.jrot1,
             mk.joint_colors};
  MarkGrads G{g_p, g_radius, g_verts_local, g_colors, g_mark_colors, g_joint_colors, g_jrot1, g_jr1, g_p_joints};
  // the roles that own a requested output
  const bool bodies = g_p || g_radius || g_verts_local || g_colors || g_mark_colors;
  const bool joints = mk.nj > 0 && (g_p || g_joint_colors || g_jrot1 || g_jr1);
  const long long nbody = bodies ? (long long)B * nb : 0, njoint = joints ? (long long)B * mk.nj : 0;
  if (nbody + njoint == 0) return 0;
  if (nbody > 0x7fffffffLL) return LCP_E_TOOLARGE;
  int body_blocks = (int)nbody;
  void* args[] = {&nb, &nvcap, &vmax, &body_blocks, &cam, &A, &kind, &radius, &verts_local, &nverts, &p, &colors, &background, &thickness,
                  &g_image, &G};
  const int rc = launch(reinterpret_cast<const void*>(lcp_render_marks_backward_kernel), nbody + njoint, scene_lds(vmax), stream, args);
  if (rc != 0 || !(g_p && mk.nj > 0)) return rc;
  long long nbodies = (long long)B * nb;
  int nj = mk.nj;
  const int32_t *jb1 = mk.jb1, *jb2 = mk.jb2;
  const double* ws = g_p_joints;
  void* gargs[] = {&nbodies, &nb, &nj, &jb1, &jb2, &ws, &g_p};
  return launch(reinterpret_cast<const void*>(lcp_render_marks_gather_kernel), (nbodies + RD_T - 1) / RD_T, 0, stream, gargs);
}

}  // namespace lcp
