// lcp_overlap.hip - overlap queries: the area of the intersection of body pairs, and its backward.
//
// include/lcp_hip.h ("overlap queries") states the rule; this file follows it comparison by comparison.  No intersection polygon is
// built: by Green's theorem the area is a sum over the pieces of either boundary that lie inside the other shape, and its differential
// is the integral of the boundary's normal motion over the same pieces.
//   hull - hull     clip(): an edge against the other hull's half-planes (Cyrus-Beck), closed for body 1 and open for body 2, so that a
//                   piece of boundary the two share counts once; a piece [t0, t1] of edge i adds (t1 - t0) cross(w_i - c1, e_i) / 2.
//                   The terms are about c1, not about the overlap, so two pieces that should cancel or complement each other must end
//                   in the SAME point: edge_pair() forms what an edge of body 1 and an edge of body 2 share - parallel or not, the
//                   height, the crossing - once, in one way, for both bodies
//   circle - hull   cuts(): an edge split where it crosses the circle; a piece inside adds its triangle about the circle's centre, a
//                   piece outside the sector it subtends
//   circle - circle the lens
//
// Forward: one workgroup per (scene, 256 pairs), the scene staged in LDS by stage_scene; lane = pair; the validity test and the
// bounding-circle cull (wanted()) come before the pair's loops.  Per-lane state is scalars: the running [t0, t1], the sum, the loop
// indices.
//
// Backward: one workgroup per scene.  A body's gradient comes from its OWN boundary alone, so nothing per pair is staged: every body is
// owned by ONE wavefront (body b by wavefront b mod 4), which looks at the pairs 64 at a time, lane = pair, and then takes the pairs the
// body is part of one by one in pair order, lane = edge: a hull's lane clips its own edge against the partner and keeps the two vertex
// terms of its piece in registers; a circle's lane takes an edge of the hull partner (lane 0 alone a circle partner).  After the last
// pair the term for w_i+1 moves to the next lane and one butterfly per output gives the pose.  No atomics: two runs give the same bits.
#include "lcp_render_common.h"

namespace lcp {
namespace overlap {

using render::MAXB;
using render::RD_T;
using render::RD_WAVES;
using render::Scene;
using render::wave_sum;

constexpr int MAXP = 1024;                 // pairs per scene
constexpr double PI = 3.14159265358979323846;

struct Pairs {
  int P;
  const int32_t* first; const int32_t* second;
};

// a x b from two rounded products (no fused multiply-add): two vectors of equal bits give exactly 0
__device__ __forceinline__ double cross_rn(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
  const double l = ax * by, r = ay * bx;
  return l - r;
}

// Whether a pair is evaluated at all (ok: the scene is queried): a pair of two different bodies of the scene, neither a hull of fewer
// than three vertices, whose bounding circles meet (the cull: otherwise the area is 0).
__device__ __forceinline__ bool wanted(const Scene& S, int nb, bool ok, int k1, int k2) {
  if (!ok || k1 == k2 || k1 < 0 || k1 >= nb || k2 < 0 || k2 >= nb) return false;
  const double reach1 = S.reach[k1], reach2 = S.reach[k2];
  if (reach1 < 0.0 || reach2 < 0.0) return false;
  const double qx = S.cx[k2] - S.cx[k1], qy = S.cy[k2] - S.cy[k1];
  return !(sqrt(qx * qx + qy * qy) - reach1 - reach2 > 0.0);
}

// What an edge of body 1 (a1, e1) and an edge of body 2 (b2, e2; n2 its normal, il2 = 1 / |e2|) have to do with each other,
// formed ONCE in one way whichever of the two edges is being clipped, so that both bodies decide and cut alike:
//   c = e1 x e2;   h = n2 . (a1 - b2), the height of a1 over body 2's line
//   par: the edges count as parallel, |c| <= TAU |e1| |e2|; then h stands for the whole edge and is compared with +-eps, a few
//        roundings of the coordinates it is formed from
//   otherwise the two LINES cross at X = a1 + tx e1, tx = -h / (c il2); body 2's parameter is X projected onto its edge
constexpr double TAU = 1e-12, EPS_H = 64 * 2.220446049250313e-16;
struct EdgePair {
  bool par, same;                          // same: the edges run in the same direction (e1 . e2 > 0)
  double c, h, eps, tx;
};
__device__ __forceinline__ EdgePair edge_pair(double2 a1, double2 e1, double2 b2, double2 e2, double2 n2, double il2) {
#pragma clang fp contract(off)
  EdgePair R;
  R.c = cross_rn(e1.x, e1.y, e2.x, e2.y);
  const double qx = a1.x - b2.x, qy = a1.y - b2.y;
  const double hx = n2.x * qx, hy = n2.y * qy;
  R.h = hx + hy;
  const double l1 = e1.x * e1.x + e1.y * e1.y, l2 = e2.x * e2.x + e2.y * e2.y;
  R.par = R.c * R.c <= (TAU * TAU) * (l1 * l2);
  R.same = e1.x * e2.x + e1.y * e2.y > 0.0;
  R.eps = EPS_H * (fabs(a1.x) + fabs(a1.y) + fabs(b2.x) + fabs(b2.y));
  R.tx = R.par ? 0.0 : -R.h / (R.c * il2);
  return R;
}

// Edge `io` (an index into the staged arrays) against the half-planes of hull [og, og + ng): false when nothing of it is left, else the
// piece [t0, t1].  first: the edge is body 1's (the closed form: a piece of length 0 stays, and so does an edge along a line of body
// 2 that runs in its direction); else body 2's (the open form).  Parallel edges: body 1's is out above the line, and on it when the two
// run against each other (the bodies touch from outside); body 2's is out unless it lies strictly inside - below body 1's line, which
// is h > eps when the two run alike and h < -eps when they run against each other.  Of two edges on one line that run alike exactly
// one stays, of two that run against each other both or none.
__device__ __forceinline__ bool clip(const Scene& S, int io, int og, int ng, bool first, double& t0, double& t1) {
  const double2 a0 = S.vw[io], e = S.ve[io], n = S.vn[io];
  const double il = S.vil[io];
  t0 = 0.0; t1 = 1.0;
  for (int j = 0; j < ng; ++j) {
    const double2 b = S.vw[og + j], eg = S.ve[og + j];
    if (first) {
      const EdgePair Q = edge_pair(a0, e, b, eg, S.vn[og + j], S.vil[og + j]);
      if (Q.par) {
        if (Q.h > Q.eps || (Q.h >= -Q.eps && !Q.same)) return false;
      } else if (Q.c > 0.0) t1 = fmin(t1, Q.tx);                                         // (n2 . e1 = c il2 > 0: the edge leaves)
      else t0 = fmax(t0, Q.tx);
      if (t0 > t1) return false;                                                         // (t0 only grows, t1 only shrinks)
    } else {
      const EdgePair Q = edge_pair(b, eg, a0, e, n, il);
      if (Q.par) {
        if (Q.same ? !(Q.h > Q.eps) : !(Q.h < -Q.eps)) return false;
      } else {
        const double xx = b.x + Q.tx * eg.x - a0.x, xy = b.y + Q.tx * eg.y - a0.y;
        const double t = (xx * e.x + xy * e.y) * il * il;
        if (Q.c > 0.0) t0 = fmax(t0, t);                                                 // (n1 . e2 = -c il1 < 0: the edge enters)
        else t1 = fmin(t1, t);
      }
      if (t0 >= t1) return false;
    }
  }
  return true;
}

// Where the edge u + t e (u relative to the circle's centre) crosses the circle of squared radius r2: the pieces are [0, ta],
// [ta, tb] and [tb, 1]; a root outside (0, 1) leaves its end at 0 or 1 (a piece of no length).
__device__ __forceinline__ void cuts(double ux, double uy, double2 e, double r2, double& ta, double& tb) {
  const double a = e.x * e.x + e.y * e.y, bq = ux * e.x + uy * e.y, cq = ux * ux + uy * uy - r2;
  const double disc = bq * bq - a * cq;
  ta = 0.0; tb = 1.0;
  if (disc > 0.0) {
    const double sq = sqrt(disc);
    const double r0 = (-bq - sq) / a, r1 = (-bq + sq) / a;
    if (r0 > 0.0 && r0 < 1.0) ta = r0;
    if (r1 > 0.0 && r1 < 1.0) tb = r1;
  }
}

// whether the piece [t0, t1] (t1 > t0) of the edge lies in the circle: its midpoint does
__device__ __forceinline__ bool piece_within(double ux, double uy, double2 e, double r2, double t0, double t1) {
  const double tm = 0.5 * (t0 + t1);
  const double mx = ux + tm * e.x, my = uy + tm * e.y;
  return mx * mx + my * my <= r2;
}

// the angle the piece [t0, t1] subtends at the circle's centre
__device__ __forceinline__ double piece_angle(double ux, double uy, double2 e, double t0, double t1) {
  const double px = ux + t0 * e.x, py = uy + t0 * e.y, qx = ux + t1 * e.x, qy = uy + t1 * e.y;
  return atan2(px * qy - py * qx, px * qx + py * qy);
}

__device__ __forceinline__ double hull_hull_area(const Scene& S, int k1, int k2) {
  const int oa = S.off[k1], na = S.off[k1 + 1] - oa, ob = S.off[k2], nbv = S.off[k2 + 1] - ob;
  const double ox = S.cx[k1], oy = S.cy[k1];
  double sum = 0.0, t0, t1;
  for (int i = 0; i < na; ++i) {
    const double2 a0 = S.vw[oa + i], e = S.ve[oa + i];
    if (clip(S, oa + i, ob, nbv, true, t0, t1)) sum += (t1 - t0) * ((a0.x - ox) * e.y - (a0.y - oy) * e.x);
  }
  for (int j = 0; j < nbv; ++j) {
    const double2 b0 = S.vw[ob + j], e = S.ve[ob + j];
    if (clip(S, ob + j, oa, na, false, t0, t1)) sum += (t1 - t0) * ((b0.x - ox) * e.y - (b0.y - oy) * e.x);
  }
  return 0.5 * sum;
}

__device__ __forceinline__ double circle_hull_area(const Scene& S, int kc, int kh) {
  const int o = S.off[kh], nv = S.off[kh + 1] - o;
  const double cx = S.cx[kc], cy = S.cy[kc], r = S.rad[kc], r2 = r * r;
  double sum = 0.0;
  bool within = false, centre_in = true;
  for (int i = 0; i < nv; ++i) {
    const double2 w = S.vw[o + i], e = S.ve[o + i], n = S.vn[o + i];
    const double ux = w.x - cx, uy = w.y - cy;
    centre_in = centre_in && n.x * (cx - w.x) + n.y * (cy - w.y) <= 0.0;
    double ta, tb;
    cuts(ux, uy, e, r2, ta, tb);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double t0 = k == 0 ? 0.0 : (k == 1 ? ta : tb), t1 = k == 0 ? ta : (k == 1 ? tb : 1.0);
      if (!(t1 > t0)) continue;
      if (piece_within(ux, uy, e, r2, t0, t1)) { sum += 0.5 * (t1 - t0) * (ux * e.y - uy * e.x); within = true; }
      else sum += 0.5 * r2 * piece_angle(ux, uy, e, t0, t1);
    }
  }
  if (!within) return centre_in ? PI * r2 : 0.0;           // nothing of the hull's boundary in the circle: all of the circle or none
  return sum;
}

__device__ __forceinline__ double circle_circle_area(const Scene& S, int k1, int k2) {
  const double qx = S.cx[k2] - S.cx[k1], qy = S.cy[k2] - S.cy[k1], r1 = S.rad[k1], r2 = S.rad[k2];
  const double d2 = qx * qx + qy * qy, d = sqrt(d2);
  if (d >= r1 + r2) return 0.0;
  if (d <= fabs(r1 - r2)) { const double rm = r1 <= r2 ? r1 : r2; return PI * rm * rm; }
  const double x1 = fmin(fmax((d2 + r1 * r1 - r2 * r2) / (2.0 * d * r1), -1.0), 1.0);
  const double x2 = fmin(fmax((d2 + r2 * r2 - r1 * r1) / (2.0 * d * r2), -1.0), 1.0);
  const double k = (-d + r1 + r2) * (d + r1 - r2) * (d - r1 + r2) * (d + r1 + r2);
  return r1 * r1 * acos(x1) + r2 * r2 * acos(x2) - 0.5 * sqrt(k);
}

// The rule of the header for one pair against the staged scene (ok: the scene is queried at all).
__device__ __forceinline__ double evaluate(const Scene& S, int nb, bool ok, int k1, int k2) {
  if (!wanted(S, nb, ok, k1, k2)) return 0.0;
  const bool circ1 = S.kind[k1] == 0, circ2 = S.kind[k2] == 0;
  const double a = circ1 && circ2 ? circle_circle_area(S, k1, k2)
                   : circ1        ? circle_hull_area(S, k1, k2)
                   : circ2        ? circle_hull_area(S, k2, k1)
                                  : hull_hull_area(S, k1, k2);
  return a > 0.0 ? a : 0.0;                                // (a sum that rounds below 0 is 0)
}

__global__ void __launch_bounds__(RD_T) lcp_pair_overlap_kernel(int nb, int cap, int vmax, int chunks, Pairs pairs, const int32_t* kind,
                                                               const double* radius, const double* verts_local, const int32_t* nverts,
                                                               const double* p, double* area) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  const int scene = blockIdx.x / chunks, chunk = blockIdx.x - scene * chunks;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  const int r = chunk * RD_T + threadIdx.x;
  if (r >= pairs.P) return;
  const size_t i = (size_t)scene * pairs.P + r;
  area[i] = evaluate(S, nb, ok, pairs.first[i], pairs.second[i]);
}

__global__ void __launch_bounds__(RD_T) lcp_pair_overlap_backward_kernel(int nb, int cap, int vmax, Pairs pairs, const int32_t* kind,
                                                                        const double* radius, const double* verts_local,
                                                                        const int32_t* nverts, const double* p, const double* g_area,
                                                                        double* g_p, double* g_radius, double* g_verts_local) {
  extern __shared__ double2 s_dyn[];
  LCP_RD_SCENE_TABLES(S, s_dyn, vmax);
  const int P = pairs.P;
  const int scene = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool ok = render::stage_scene(S, scene, nb, cap, vmax, 0, kind, radius, verts_local, nverts, p, nullptr, nullptr, 0.0);
  for (int b = wave; b < nb; b += RD_WAVES) {
    const bool hull = S.kind[b] != 0;
    const int o = S.off[b], nv = ok ? S.off[b + 1] - o : 0;               // (a scene that is not queried has no staged vertices)
    const double bx = S.cx[b], by = S.cy[b], rb = S.rad[b];
    const bool edge = hull && lane < nv;                                   // a hull's lane: its own edge
    const double2 a0 = edge ? S.vw[o + lane] : make_double2(0.0, 0.0), ea = edge ? S.ve[o + lane] : make_double2(0.0, 0.0);
    double fx = 0.0, fy = 0.0, nx = 0.0, ny = 0.0;                         // a hull: what w_lane and w_lane+1 receive; a circle: fx, fy its centre
    double grad = 0.0;                                                     // a circle: its radius
    for (int r0 = 0; r0 < P; r0 += 64) {
      const int r = r0 + lane;
      const size_t i = (size_t)scene * P + (r < P ? r : 0);
      const int k1 = r < P ? pairs.first[i] : -1, k2 = r < P ? pairs.second[i] : -1;
      const bool mine = (k1 == b || k2 == b) && wanted(S, nb, ok, k1, k2);
      const double g = mine ? g_area[i] : 0.0;
      unsigned long long todo = __ballot(mine);
      while (todo) {                                                       // the body's pairs, in pair order
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const bool first = __shfl(k1, l, 64) == b;
        const int q = first ? __shfl(k2, l, 64) : __shfl(k1, l, 64);       // the partner
        const double gg = __shfl(g, l, 64);
        const bool qhull = S.kind[q] != 0;
        const int oq = S.off[q], nq = S.off[q + 1] - oq;
        const double qx = S.cx[q], qy = S.cy[q], rq = S.rad[q];
        if (hull) {
          // the pieces of the own edge inside the partner: |e| n = (e.y, -e.x) times ((t1 - t0) - s) for w_i and s for w_i+1
          double len = 0.0, s = 0.0;
          if (edge && qhull) {
            double t0, t1;
            if (clip(S, o + lane, oq, nq, first, t0, t1)) { len = t1 - t0; s = 0.5 * (t1 * t1 - t0 * t0); }
          } else if (edge) {
            const double ux = a0.x - qx, uy = a0.y - qy, r2 = rq * rq;
            double ta, tb;
            cuts(ux, uy, ea, r2, ta, tb);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const double t0 = k == 0 ? 0.0 : (k == 1 ? ta : tb), t1 = k == 0 ? ta : (k == 1 ? tb : 1.0);
              if (t1 > t0 && piece_within(ux, uy, ea, r2, t0, t1)) { len += t1 - t0; s += 0.5 * (t1 * t1 - t0 * t0); }
            }
          }
          const double wx = gg * ea.y, wy = -gg * ea.x;
          fx += (len - s) * wx; fy += (len - s) * wy;
          nx += s * wx; ny += s * wy;
        } else if (qhull) {
          // a circle against a hull, lane = the hull's edge: the centre receives minus what the hull's pieces in the circle give the
          // hull (translation invariance), the radius r times the angle of the circle's arc inside the hull
          const bool has = lane < nq;
          double phi = 0.0;
          bool within = false, centre_in = true;
          if (has) {
            const double2 w = S.vw[oq + lane], e = S.ve[oq + lane], n = S.vn[oq + lane];
            const double ux = w.x - bx, uy = w.y - by, r2 = rb * rb;
            centre_in = n.x * (bx - w.x) + n.y * (by - w.y) <= 0.0;
            double ta, tb;
            cuts(ux, uy, e, r2, ta, tb);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const double t0 = k == 0 ? 0.0 : (k == 1 ? ta : tb), t1 = k == 0 ? ta : (k == 1 ? tb : 1.0);
              if (!(t1 > t0)) continue;
              if (piece_within(ux, uy, e, r2, t0, t1)) { fx -= gg * e.y * (t1 - t0); fy += gg * e.x * (t1 - t0); within = true; }
              else phi += piece_angle(ux, uy, e, t0, t1);
            }
          }
          if (__any(within)) grad += gg * rb * phi;
          else if (__all(centre_in) && lane == 0) grad += gg * 2.0 * PI * rb;            // all of the circle inside the hull
        } else if (lane == 0) {
          const double dx = qx - bx, dy = qy - by, d2 = dx * dx + dy * dy, d = sqrt(d2);
          if (d >= rb + rq) {
          } else if (d <= fabs(rb - rq)) {
            if (first ? rb <= rq : rb < rq) grad += gg * 2.0 * PI * rb;                  // the smaller circle's own area (a tie: body 1's)
          } else {
            const double x = fmin(fmax((d2 + rb * rb - rq * rq) / (2.0 * d * rb), -1.0), 1.0);
            const double chord = 2.0 * rb * sqrt(fmax(1.0 - x * x, 0.0));
            fx += gg * chord * dx / d; fy += gg * chord * dy / d;
            grad += gg * 2.0 * acos(x) * rb;
          }
        }
      }
    }
    // a hull: the term for w_i+1 moves to the next lane; the world-vertex gradients turned back into the body frame, and the pose
    const int src = lane == 0 ? (nv > 0 ? nv - 1 : 0) : lane - 1;
    const double mx = __shfl(nx, src, 64), my = __shfl(ny, src, 64);
    double gx = 0.0, gy = 0.0, grot = 0.0;
    if (hull) {
      double wx = 0.0, wy = 0.0;
      if (edge) {
        wx = fx + mx; wy = fy + my;
        const double rx = a0.x - bx, ry = a0.y - by;
        gx = wx; gy = wy; grot = wy * rx - wx * ry;                        // dw/drot = left turn of (w - c)
      }
      if (g_verts_local && lane < cap) {                                   // (cap <= 64: one pass; slots >= nverts: zeros)
        const double sn = S.sn[b], cs = S.cs[b];
        *reinterpret_cast<double2*>(g_verts_local + (((size_t)scene * nb + b) * cap + lane) * 2) =
            make_double2(cs * wx + sn * wy, -sn * wx + cs * wy);
      }
    } else {
      gx = fx; gy = fy;
      if (g_verts_local && lane < cap)
        *reinterpret_cast<double2*>(g_verts_local + (((size_t)scene * nb + b) * cap + lane) * 2) = make_double2(0.0, 0.0);
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

}  // namespace overlap

bool pair_overlap_supported(int nb, int nvcap, int scene_verts_max, int P) {
  return render_supported(nb, nvcap, scene_verts_max) && P >= 1 && P <= overlap::MAXP;
}

int pair_overlap_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                        const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                        const int32_t* pair_second, double* area, void* stream) {
  using namespace overlap;
  if (!pair_overlap_supported(nb, nvcap, scene_verts_max, P)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  int chunks = (P + RD_T - 1) / RD_T;
  Pairs pairs{P, pair_first, pair_second};
  void* args[] = {&nb, &nvcap, &vmax, &chunks, &pairs, &kind, &radius, &verts_local, &nverts, &p, &area};
  return launch(reinterpret_cast<const void*>(lcp_pair_overlap_kernel), (long long)B * chunks, render::scene_lds(vmax), stream, args);
}

int pair_overlap_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                 const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                                 const int32_t* pair_second, const double* g_area, double* g_p, double* g_radius,
                                 double* g_verts_local, void* stream) {
  using namespace overlap;
  if (!pair_overlap_supported(nb, nvcap, scene_verts_max, P)) return LCP_E_TOOLARGE;
  int vmax = ctw::vmax_of(scene_verts_max);
  Pairs pairs{P, pair_first, pair_second};
  void* args[] = {&nb, &nvcap, &vmax, &pairs, &kind, &radius, &verts_local, &nverts, &p, &g_area, &g_p, &g_radius, &g_verts_local};
  return launch(reinterpret_cast<const void*>(lcp_pair_overlap_backward_kernel), B, render::scene_lds(vmax), stream, args);
}

}  // namespace lcp
