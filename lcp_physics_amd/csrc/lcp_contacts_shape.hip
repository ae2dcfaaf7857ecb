// lcp_contacts_shape.hip - backward of the contact frame with respect to the SHAPE of the bodies: the radii of the circles and the
// body-frame vertices of the hulls.
//
// In the reference every operation of DiffContactHandler (physics/contacts.py:57-352) is a torch op on Circle.rad (bodies.py:121)
// and on Hull.verts (bodies.py:168-171, turned by rotate_verts, bodies.py:211-214), so a loss after a roll-out reaches them.
// Here the same geometry code (lcp_contacts_geom.inc) runs on dual numbers, as in lcp_contact_frame_backward_wide_kernel, with
// seeds that are shape coordinates.  What differs from the pose derivative: a seeded vertex moves alone, so the two edges that
// end in it change their length and their normal (ShapeRef / ShapeLen below; with respect to the pose the lengths were constants
// and the normals only turned).
//
// A pair's records depend on few shape coordinates: the two radii, the two vertices of the reference edge (hull / hull; for
// circle / hull the GJK simplex's one or two vertices, or the SAT edge's two) and the two vertices of the incident edge - ten seeds
// at most, whatever the hulls' vertex counts.  One workgroup per scene:
//   1. the work units = the distinct pairs among the first min(count, maxc) records (stage_frame_scene, as in the pose kernel);
//   2. one lane per unit runs collide_pair with no seed and keeps the vertices LCP_GEOM_TRACE names (on dual numbers too, so
//      that this pass and the next take their branches in the same code);
//   3. one lane per (unit, seed) re-runs collide_pair with that seed and keeps its term g . d(n, p1, p2) in LDS;
//   4. the terms are summed per output coordinate in record order (no atomics: the result does not depend on timing), the
//      world-frame vertex gradient turned back by R(rot)^T into verts_local coordinates.  Every output element is written.
// LDS: static 3.4 KB (pose, radii, sin / cos, kinds, offsets); dynamic 40 B per vertex of the scene's packed list (rotated
// vertices, edge normals, edge lengths) + 112 B per contact slot (ten terms, four traced vertices, the reference body, the
// unit's first record and two bodies) + 4 B: 152 KB at most, checked on the host before the launch (LCP_E_TOOLARGE).
// Limits as for lcp_contacts_wide.hip: nb <= 64, 8 <= nvcap <= 64, at most 1024 vertices per scene.
#include "lcp_contacts_wide.h"

namespace lcp {
namespace ctw {
namespace shp {

constexpr int SB_T = 256;       // threads per workgroup (one scene)
constexpr int NSEED = 10;       // radius of body 1, of body 2, then x, y of the traced vertices tr0, tr1, ti0, ti1

using ad::Dual;

// Vertex k of a body, or (with `nrm` set) the outward unit normal of its edge (k, k + 1): the value staged in LDS, the
// derivative with respect to coordinate (sx, sy) = e_x or e_y of vertex `ks` of that body (-1: no seed in this body).
template <class V>
struct ShapeRef {
  const double2* vts;
  const double2* nrm;
  int n, ks;
  double sx, sy;
  __device__ __forceinline__ V operator[](int k) const {
    V r;
    if (!nrm) {
      const double2 u = vts[k];
      const bool on = k == ks;
      r.x = Dual(u.x, on ? sx : 0.0); r.y = Dual(u.y, on ? sy : 0.0);
      return r;
    }
    const double2 nv = nrm[k];
    const int k1 = k + 1 == n ? 0 : k + 1;
    r.x = Dual(nv.x); r.y = Dual(nv.y);
    if (k == ks || k1 == ks) {                                          // contacts.py:229-231: normal = left_orthogonal(edge) / |edge|
      const double sg = k1 == ks ? 1.0 : -1.0;
      const double2 a = vts[k], c = vts[k1];
      const Dual ex(c.x - a.x, sg * sx), ey(c.y - a.y, sg * sy);
      const Dual inv = Dual(1.0) / sqrt(ex * ex + ey * ey);
      r.x.d = (ey * inv).d; r.y.d = (-ex * inv).d;
    }
    return r;
  }
};
// the length of edge (k, k + 1)
struct ShapeLen {
  const double2* vts;
  const double* len;
  int n, ks;
  double sx, sy;
  __device__ __forceinline__ Dual operator[](int k) const {
    const int k1 = k + 1 == n ? 0 : k + 1;
    Dual r(len[k]);
    if (k == ks || k1 == ks) {
      const double sg = k1 == ks ? 1.0 : -1.0;
      const double2 a = vts[k], c = vts[k1];
      r.d = sg * ((c.x - a.x) * sx + (c.y - a.y) * sy) / r.v;
    }
    return r;
  }
};
#define LCP_S Dual
#define LCP_GEOM_VREF ShapeRef<V2>
#define LCP_GEOM_SREF ShapeLen
#define LCP_GEOM_TRACE
#include "lcp_contacts_geom.inc"
#undef LCP_GEOM_TRACE
#undef LCP_GEOM_SREF
#undef LCP_GEOM_VREF
#undef LCP_S

// body `bb` of the scene with the radius seed `drad` and the vertex seed (ks, c): ks = -1 none, c = 0 x, 1 y
__device__ __forceinline__ Body make_body(int bb, double drad, int ks, int c, const int* s_kind, const int* s_off, const double* s_rad,
                                          const double* s_pose, const double2* s_verts, const double2* s_nrm, const double* s_elen) {
  Body b;
  const int o = s_off[bb];
  b.kind = s_kind[bb];
  b.rad = Dual(s_rad[bb], drad);
  b.nv = s_off[bb + 1] - o;
  b.pos = v2(Dual(s_pose[bb * 3 + 1]), Dual(s_pose[bb * 3 + 2]));
  const double sx = c == 0 ? 1.0 : 0.0, sy = c == 0 ? 0.0 : 1.0;
  b.verts.vts = s_verts + o; b.verts.nrm = nullptr; b.verts.n = b.nv; b.verts.ks = ks; b.verts.sx = sx; b.verts.sy = sy;
  b.nrm.vts = s_verts + o; b.nrm.nrm = s_nrm + o; b.nrm.n = b.nv; b.nrm.ks = ks; b.nrm.sx = sx; b.nrm.sy = sy;
  b.elen.vts = s_verts + o; b.elen.len = s_elen + o; b.elen.n = b.nv; b.elen.ks = ks; b.elen.sx = sx; b.elen.sy = sy;
  return b;
}

__global__ void __launch_bounds__(SB_T) lcp_contact_frame_backward_shape_kernel(int nb, int maxc, int nvcap, int vmax, const int32_t* kind,
                                                                              const double* radius, const double* verts_local,
                                                                              const int32_t* nverts, const double* p, double eps,
                                                                              const int32_t* count, const int32_t* c_i1,
                                                                              const int32_t* c_i2, const float* g_n,
                                                                              const float* g_p1, const float* g_p2,
                                                                              double* d_radius, double* d_verts_local) {
  extern __shared__ double2 s_dyn[];
  double2* s_verts = s_dyn;
  double2* s_nrm = s_verts + vmax;
  double* s_elen = reinterpret_cast<double*>(s_nrm + vmax);
  double* s_term = s_elen + vmax;                                         // [maxc][NSEED]
  int* s_uv = reinterpret_cast<int*>(s_term + (size_t)maxc * NSEED);     // [maxc][4] traced vertices in the packed list, -1: none
  int* s_uref = s_uv + (size_t)maxc * 4;                                  // [maxc] 0 / 1: the body of the unit that owns tr0, tr1
  int* s_ustart = s_uref + maxc;                                          // [maxc + 1]
  int* s_ub1 = s_ustart + maxc + 1;                                       // [maxc]
  int* s_ub2 = s_ub1 + maxc;                                              // [maxc]
  __shared__ double s_pose[MAXB * 3];
  __shared__ double s_rad[MAXB];
  __shared__ double2 s_sc[MAXB];
  __shared__ int s_kind[MAXB], s_off[MAXB + 1];
  __shared__ int s_nunits;
  const int tid = threadIdx.x;
  const int scene = blockIdx.x;
  double* out_r = d_radius ? d_radius + (size_t)scene * nb : nullptr;
  double* out_v = d_verts_local ? d_verts_local + (size_t)scene * nb * nvcap * 2 : nullptr;
  const int vtot = stage_bodies(scene, nb, nvcap, kind, nverts, radius, s_kind, s_off, s_rad);   // (uniform over the workgroup)
  if (vtot > vmax) {                                                      // scene_verts_max too small: no derivative
    if (out_r) for (int i = tid; i < nb; i += SB_T) out_r[i] = 0.0;
    if (out_v) for (int i = tid; i < nb * nvcap * 2; i += SB_T) out_v[i] = 0.0;
    return;
  }
  const int nunits = stage_frame_scene<SB_T>(scene, nb, maxc, nvcap, verts_local, p, count, c_i1, c_i2, s_off, s_pose, s_sc, s_verts, s_nrm,
                                             s_elen, s_ustart, s_ub1, s_ub2, &s_nunits);
  // the vertices each unit's records were built from
  for (int u = tid; u < nunits; u += SB_T) {
    const int bi = s_ub1[u], bj = s_ub2[u];
    const Body b1 = make_body(bi, 0.0, -1, 0, s_kind, s_off, s_rad, s_pose, s_verts, s_nrm, s_elen);
    const Body b2 = make_body(bj, 0.0, -1, 0, s_kind, s_off, s_rad, s_pose, s_verts, s_nrm, s_elen);
    Pt pt0, pt1;
    pt0.tref = 0; pt0.tr0 = -1; pt0.tr1 = -1; pt0.ti0 = -1; pt0.ti1 = -1;
    const int cnt = collide_pair(b1, b2, eps, pt0, pt1);
    const int ro = s_off[pt0.tref ? bj : bi], io = s_off[pt0.tref ? bi : bj];
    const bool hit = cnt > 0;
    s_uref[u] = pt0.tref;
    s_uv[u * 4 + 0] = hit && pt0.tr0 >= 0 ? ro + pt0.tr0 : -1;
    s_uv[u * 4 + 1] = hit && pt0.tr1 >= 0 ? ro + pt0.tr1 : -1;
    s_uv[u * 4 + 2] = hit && pt0.ti0 >= 0 ? io + pt0.ti0 : -1;
    s_uv[u * 4 + 3] = hit && pt0.ti1 >= 0 ? io + pt0.ti1 : -1;
  }
  __syncthreads();
  for (int w = tid; w < nunits * NSEED; w += SB_T) {
    const int u = w / NSEED, s = w - u * NSEED;
    const int r0 = s_ustart[u], nrec = s_ustart[u + 1] - r0;
    const int bi = s_ub1[u], bj = s_ub2[u];
    int ks1 = -1, ks2 = -1, c = 0;
    double dr1 = 0.0, dr2 = 0.0;
    bool active;
    if (s < 2) {
      active = s_kind[s == 0 ? bi : bj] == 0;                           // (a hull's radius is not read)
      dr1 = s == 0 ? 1.0 : 0.0; dr2 = 1.0 - dr1;
    } else {
      const int j = (s - 2) >> 1;
      const int pid = s_uv[u * 4 + j];
      c = (s - 2) & 1;
      active = pid >= 0;
      const int owner = j < 2 ? s_uref[u] : 1 - s_uref[u];               // 0: body i1, 1: body i2
      if (owner == 0) ks1 = pid - s_off[bi]; else ks2 = pid - s_off[bj];
    }
    double acc = 0.0;
    if (active) {
      const Body b1 = make_body(bi, dr1, ks1, c, s_kind, s_off, s_rad, s_pose, s_verts, s_nrm, s_elen);
      const Body b2 = make_body(bj, dr2, ks2, c, s_kind, s_off, s_rad, s_pose, s_verts, s_nrm, s_elen);
      Pt pt0, pt1;
      const int c2 = collide_pair(b1, b2, eps, pt0, pt1);
      for (int q = 0; q < c2 && q < nrec; ++q) {
        const Pt& pt = q == 0 ? pt0 : pt1;
        const size_t o = ((size_t)scene * maxc + r0 + q) * 2;
        acc += (double)g_n[o] * pt.n.x.d + (double)g_n[o + 1] * pt.n.y.d + (double)g_p1[o] * pt.p1.x.d + (double)g_p1[o + 1] * pt.p1.y.d
             + (double)g_p2[o] * pt.p2.x.d + (double)g_p2[o + 1] * pt.p2.y.d;
      }
    }
    s_term[w] = acc;
  }
  __syncthreads();
  // per output coordinate, the terms in record order
  if (out_r) {
    for (int b = tid; b < nb; b += SB_T) {
      double sum = 0.0;
      for (int u = 0; u < nunits; ++u) {
        if (s_ub1[u] == b) sum += s_term[u * NSEED];
        if (s_ub2[u] == b) sum += s_term[u * NSEED + 1];
      }
      out_r[b] = sum;
    }
  }
  if (out_v) {
    for (int i = tid; i < nb * nvcap; i += SB_T) {
      const int b = i / nvcap, k = i - b * nvcap;
      const int o = s_off[b];
      double lx = 0.0, ly = 0.0;
      if (k < s_off[b + 1] - o) {
        const int pid = o + k;
        double gx = 0.0, gy = 0.0;
        for (int u = 0; u < nunits; ++u) {
          if (s_ub1[u] != b && s_ub2[u] != b) continue;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (s_uv[u * 4 + j] == pid) { gx += s_term[u * NSEED + 2 + 2 * j]; gy += s_term[u * NSEED + 3 + 2 * j]; }
        }
        const double sn = s_sc[b].x, cs = s_sc[b].y;                    // u = R v_local, so d/d(v_local) = R^T d/du
        lx = cs * gx + sn * gy; ly = cs * gy - sn * gx;
      }
      out_v[2 * i] = lx; out_v[2 * i + 1] = ly;
    }
  }
}

static size_t shape_bwd_lds(int vmax, int maxc) {
  return (size_t)vmax * (2 * sizeof(double2) + sizeof(double)) + (size_t)maxc * NSEED * sizeof(double) + (size_t)(8 * maxc + 1) * sizeof(int);
}

}  // namespace shp
}  // namespace ctw

int contact_frame_backward_shape_launch(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind,
                                        const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                        double eps, const int32_t* count, const int32_t* c_i1, const int32_t* c_i2,
                                        const float* g_n, const float* g_p1, const float* g_p2, double* d_radius,
                                        double* d_verts_local, void* stream) {
  if (!contacts_wide_supported(nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  const int vmax = ctw::vmax_of(scene_verts_max);
  const size_t lds = ctw::shp::shape_bwd_lds(vmax, maxc);
  if (lds > ctw::LDS_LIMIT) return LCP_E_TOOLARGE;
  return ctw::launch_per_scene(ctw::shp::lcp_contact_frame_backward_shape_kernel, B, ctw::shp::SB_T, lds, stream, nb, maxc, nvcap, vmax, kind,
                               radius, verts_local, nverts, p, eps, count, c_i1, c_i2, g_n, g_p1, g_p2, d_radius, d_verts_local);
}

}  // namespace lcp
