// lcp_contacts_wide.hip - the narrow phase of lcp_contacts.hip for hulls of up to 64 vertices and scenes of up to 64 bodies.
//
// Same job, same semantics, same geometry code (lcp_contacts_geom.inc) as lcp_move_find_contacts_kernel and
// lcp_contact_frame_backward_kernel (see lcp_contacts.hip for the map to the reference); what differs is the staging:
//   * the vertices of a scene are ONE packed list in LDS (body b owns [off[b], off[b] + nverts[b]), off = prefix sum of the
//     nverts), sized at launch from the batch's largest per-scene vertex total - the reference's Hull takes any number of
//     vertices (bodies.py:154-250) and World.find_contacts any number of bodies (world.py:139-142);
//   * the geometry is included in a namespace of its own whose NV is 64, so the GJK iteration cap (4 NV) covers the largest
//     hull (the reference loops `while True`, contacts.py:88);
//   * the frame backward runs one lane per (contacting pair, pose coordinate) instead of one thread per scene, and forms the
//     dual vertices / normals on read from the values staged once (d/d(rot) of R(rot) v is the 90-degree turn of the value;
//     edge lengths do not depend on the pose).
// Limits (checked on the host before a launch, lcp_api.cpp): nb <= 64, 8 <= nvcap <= 64 (verts_local[B,nb,nvcap,2]),
// hulls of 3..nvcap vertices, at most 1024 vertices per scene.
// The detection kernel is also the one behind lcp_move_find_contacts_bp_f64: instantiated with BP it culls the body pairs before the
// narrow phase (lcp_contacts_bp.hip, included below: the cull, its LDS and why it loses nothing).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_contacts_wide.h"
#include "lcp_contacts_bp.hip"

namespace lcp {
namespace ctw {

constexpr int FB_T = 256;       // threads per workgroup (one scene) of the frame backward

#define LCP_S double
#include "lcp_contacts_geom.inc"
#undef LCP_S

// ---- forward-mode derivative over ad::Dual (lcp_contacts_wide.h) ---------------------------------------------------------
namespace ad {
// A rotated vertex (or edge normal) u = R(rot) u_local of a body whose rotation carries the seed dr (1 or 0): the value from
// LDS, the derivative d u / d rot * dr = dr (-u.y, u.x).  Translation seeds do not reach it (vertices are relative to pos).
template <class V>
struct TurnRef {
  const double2* val;
  double dr;
  __device__ __forceinline__ V operator[](int k) const {
    const double2 u = val[k];
    V r; r.x = Dual(u.x, -u.y * dr); r.y = Dual(u.y, u.x * dr);
    return r;
  }
};
// an edge length: invariant under the pose
struct ConstRef {
  const double* val;
  __device__ __forceinline__ Dual operator[](int k) const { return Dual(val[k]); }
};
#define LCP_S Dual
#define LCP_GEOM_VREF TurnRef<V2>
#define LCP_GEOM_SREF ConstRef
#include "lcp_contacts_geom.inc"
#undef LCP_GEOM_SREF
#undef LCP_GEOM_VREF
#undef LCP_S
}  // namespace ad

// ---------------------------------------------------------------- detection: World.step_dt's move / detect / halve loop
// One wavefront per scene, lane = body pair (i < j, lexicographic), the up to 2016 pairs walked 64 at a time; the contacts are
// compacted in pair order with a wave prefix sum.  Dynamic LDS: 4 arrays over the scene's packed vertex list (V = the host's
// scene_verts_max): local and rotated vertices, edge normals (V2) and edge lengths, and the owning body of each vertex.
// DTS: every scene's loop starts from P.dt_in[scene] (compile-time, as in lcp_contacts.hip: the scalar-dt kernel stays the code it was)
// BP: the broadphase of lcp_contacts_bp.hip - every trial pose culls the pairs into a candidate list (static LDS of its own, which the
// other instantiations do not allocate) and the lanes walk that list instead of all pairs; candidates[B] or NULL: its length at the
// accepted pose.  Every barrier and the __all(done) exit are wave-uniform in every instantiation.
template <bool DTS, bool BP>
__global__ void __launch_bounds__(64) lcp_move_find_contacts_wide_kernel(ContactArgs P, int nvcap, int vmax, int32_t* candidates) {
  extern __shared__ double2 s_dyn[];
  V2* s_vloc = reinterpret_cast<V2*>(s_dyn);
  V2* s_verts = s_vloc + vmax;
  V2* s_nrm = s_verts + vmax;
  double* s_elen = reinterpret_cast<double*>(s_nrm + vmax);
  int* s_vbody = reinterpret_cast<int*>(s_elen + vmax);
  __shared__ double s_pose[MAXB * 3];
  __shared__ V2 s_sc[MAXB];
  __shared__ double s_rad[MAXB];
  __shared__ int s_kind[MAXB], s_off[MAXB + 1];
  __shared__ bp::CullLds<V2> s_cull;                       // (BP only)
  const int ll = threadIdx.x;
  const int scene = blockIdx.x;
  const int nb = P.nb;
  const int npairs = nb * (nb - 1) / 2;
  const int vtot = stage_bodies(scene, nb, nvcap, P.kind, P.nverts, P.radius, s_kind, s_off, s_rad);
  if (vtot > vmax) {                                      // the caller's scene_verts_max is too small: no detection, count = -1
    pad_records(P, scene, ll, 0);
    if (ll == 0) { P.count[scene] = -1; if (BP && candidates) candidates[scene] = 0; }
    return;
  }
  __syncthreads();
  // geometry does not change over the trials: stage it in LDS once
  for (int b = 0; b < nb; ++b) {
    const int o = s_off[b], n = s_off[b + 1] - o;
    const double* vl = P.verts_local + ((size_t)scene * nb + b) * nvcap * 2;
    for (int k = ll; k < n; k += 64) { s_vloc[o + k] = v2(vl[2 * k], vl[2 * k + 1]); s_vbody[o + k] = b; }
  }
  if constexpr (BP) {
    __syncthreads();
    bp::bound_radii(nb, s_kind, s_off, s_rad, s_vloc, s_cull.bound);
  }
  double dt = DTS ? P.dt_in[scene] : P.dt;                  // per-scene starting dt (World.step(fixed_dt=True), world.py:72-80)
  const bool finished = DTS && dt <= 0.0;                      // the scene has reached its end_t: it stays where it is (one trial, no move)
  int base = 0, trial = 0, nwork = npairs;                  // nwork: the pairs the narrow phase walks
  double maxpen = -1e300;
  for (;;) {
    // bodies.py:80-82 (p <- p_start + v dt) and the vertex rotation of bodies.py:211-214
    for (int idx = ll; idx < nb * 3; idx += 64) {
      double pv = P.p_start[(size_t)scene * nb * 3 + idx];
      if (P.v && !finished) pv += (double)P.v[(size_t)scene * nb * 3 + idx] * dt;
      s_pose[idx] = pv;
    }
    __syncthreads();
    for (int b = ll; b < nb; b += 64) { const double rot = s_pose[b * 3]; s_sc[b] = v2(sin(rot), cos(rot)); }
    __syncthreads();
    for (int idx = ll; idx < vtot; idx += 64) s_verts[idx] = turned<V2>(s_sc[s_vbody[idx]], s_vloc[idx].x, s_vloc[idx].y);
    __syncthreads();
    // edge normals and lengths of every hull, once per trial pose
    for (int idx = ll; idx < vtot; idx += 64) {
      const int bdy = s_vbody[idx], o = s_off[bdy];
      edge_normal(s_verts + o, s_off[bdy + 1] - o, idx - o, s_nrm[idx], s_elen[idx]);
    }
    __syncthreads();
    if constexpr (BP) {
      nwork = bp::cull_pairs(P, scene, s_cull, s_kind, s_off, s_rad, s_pose, s_verts, s_nrm);
      __syncthreads();
    }
    base = 0; maxpen = -1e300;
    for (int w0 = 0; w0 < nwork; w0 += 64) {
      const int w = w0 + ll;
      int cnt = 0, bi = 0, bj = 1;
      Pt pt0, pt1;
      pt0.n = v2(0, 0); pt0.p1 = pt0.n; pt0.p2 = pt0.n; pt0.pen = 0; pt1 = pt0;
      bool run = w < nwork;
      if (run) {
        if constexpr (BP) {                                     // (the cull has looked at no_contact)
          const int code = s_cull.cand[w];
          bi = code >> 8; bj = code & 255;
        } else {
          pair_of(w, nb, bi, bj);
          run = !(P.no_contact && P.no_contact[((size_t)scene * nb + bi) * nb + bj]);
        }
      }
      if (run) {
        Body b1, b2;
        b1.kind = s_kind[bi]; b2.kind = s_kind[bj];
        b1.pos = v2(s_pose[bi * 3 + 1], s_pose[bi * 3 + 2]); b2.pos = v2(s_pose[bj * 3 + 1], s_pose[bj * 3 + 2]);
        b1.rad = s_rad[bi]; b2.rad = s_rad[bj];
        const int o1 = s_off[bi], o2 = s_off[bj];
        b1.nv = s_off[bi + 1] - o1; b2.nv = s_off[bj + 1] - o2;
        b1.verts = s_verts + o1; b2.verts = s_verts + o2;
        b1.nrm = s_nrm + o1; b2.nrm = s_nrm + o2; b1.elen = s_elen + o1; b2.elen = s_elen + o2;
        cnt = collide_pair(b1, b2, P.eps, pt0, pt1);
      }
      base += store_records(P, scene, ll, base, cnt, bi, bj, pt0, pt1, maxpen);
    }
    maxpen = scene_max(maxpen);
    ++trial;
    const bool done = accept_or_halve(P, base, maxpen, trial, finished, dt);
    if (__all(done)) break;
    __syncthreads();
  }
  scene_outputs(P, scene, ll, s_pose, base, maxpen, dt, trial, finished);
  if (BP && ll == 0 && candidates) candidates[scene] = nwork;       // pairs that passed the cull at the accepted pose
}

// ---------------------------------------------------------------- backward of the contact frame
// d(loss)/d(pose_b,q) = sum over the records of g_n . dn/d(pose_b,q) + g_p1 . dp1/d(..) + g_p2 . dp2/d(..)   (lcp_contacts.hip)
// One workgroup per scene.  The work units are the distinct pairs among the first min(count, maxc) records (a pair's records
// are consecutive in the list); lane w = (unit w / 6, pose coordinate w % 6 of the pair: rot, x, y of body i1, then of i2)
// re-runs collide_pair on dual numbers with that seed and keeps its term in LDS; the terms are then summed per pose
// coordinate in record order (the existing kernel's order; no atomics, so the result does not depend on timing).
// Dynamic LDS: rotated vertices, edge normals (V2) and edge lengths of the packed vertex list (vmax), then per unit
// (maxc): its six terms, its first record and its two bodies.
__global__ void __launch_bounds__(FB_T) lcp_contact_frame_backward_wide_kernel(int nb, int maxc, int nvcap, int vmax, const int32_t* kind,
                                                                             const double* radius, const double* verts_local,
                                                                             const int32_t* nverts, const double* p, double eps,
                                                                             const int32_t* count, const int32_t* c_i1,
                                                                             const int32_t* c_i2, const float* g_n,
                                                                             const float* g_p1, const float* g_p2, double* dp) {
  extern __shared__ double2 s_dyn[];
  double2* s_verts = s_dyn;
  double2* s_nrm = s_verts + vmax;
  double* s_elen = reinterpret_cast<double*>(s_nrm + vmax);
  double* s_term = s_elen + vmax;                                     // [maxc][6]
  int* s_ustart = reinterpret_cast<int*>(s_term + (size_t)maxc * 6); // [maxc + 1]
  int* s_ub1 = s_ustart + maxc + 1;                                   // [maxc]
  int* s_ub2 = s_ub1 + maxc;                                          // [maxc]
  __shared__ double s_pose[MAXB * 3];
  __shared__ double s_rad[MAXB];
  __shared__ double2 s_sc[MAXB];
  __shared__ int s_kind[MAXB], s_off[MAXB + 1];
  __shared__ int s_nunits;
  const int tid = threadIdx.x;
  const int scene = blockIdx.x;
  double* out = dp + (size_t)scene * nb * 3;
  const int vtot = stage_bodies(scene, nb, nvcap, kind, nverts, radius, s_kind, s_off, s_rad);   // (uniform over the workgroup)
  if (vtot > vmax) {                                                  // scene_verts_max too small: no derivative
    for (int i = tid; i < nb * 3; i += FB_T) out[i] = 0.0;
    return;
  }
  const int nunits = stage_frame_scene<FB_T>(scene, nb, maxc, nvcap, verts_local, p, count, c_i1, c_i2, s_off, s_pose, s_sc, s_verts, s_nrm,
                                             s_elen, s_ustart, s_ub1, s_ub2, &s_nunits);
  for (int w = tid; w < nunits * 6; w += FB_T) {
    using ad::Dual;
    const int u = w / 6, s = w - u * 6;
    const int r0 = s_ustart[u], nrec = s_ustart[u + 1] - r0;
    const int bi = s_ub1[u], bj = s_ub2[u];
    ad::Body b[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int bb = q == 0 ? bi : bj;
      const int seed = (s / 3 == q) ? s % 3 : -1;                   // 0 rot, 1 x, 2 y; -1: none
      const int o = s_off[bb];
      b[q].kind = s_kind[bb];
      b[q].rad = Dual(s_rad[bb]);
      b[q].nv = s_off[bb + 1] - o;
      b[q].pos = ad::v2(Dual(s_pose[bb * 3 + 1], seed == 1 ? 1.0 : 0.0), Dual(s_pose[bb * 3 + 2], seed == 2 ? 1.0 : 0.0));
      const double dr = seed == 0 ? 1.0 : 0.0;
      b[q].verts.val = s_verts + o; b[q].verts.dr = dr;
      b[q].nrm.val = s_nrm + o; b[q].nrm.dr = dr;
      b[q].elen.val = s_elen + o;
    }
    ad::Pt pt0, pt1;
    const int c2 = ad::collide_pair(b[0], b[1], eps, pt0, pt1);
    double acc = 0.0;
    for (int c = 0; c < c2 && c < nrec; ++c) {
      const ad::Pt& pt = c == 0 ? pt0 : pt1;
      const size_t o = ((size_t)scene * maxc + r0 + c) * 2;
      acc += (double)g_n[o] * pt.n.x.d + (double)g_n[o + 1] * pt.n.y.d + (double)g_p1[o] * pt.p1.x.d + (double)g_p1[o + 1] * pt.p1.y.d
           + (double)g_p2[o] * pt.p2.x.d + (double)g_p2[o + 1] * pt.p2.y.d;
    }
    s_term[w] = acc;
  }
  __syncthreads();
  // per pose coordinate, the terms in record order
  for (int i = tid; i < nb * 3; i += FB_T) {
    const int bd = i / 3, c = i - bd * 3;
    double sum = 0.0;
    for (int u = 0; u < nunits; ++u) {
      if (s_ub1[u] == bd) sum += s_term[u * 6 + c];
      if (s_ub2[u] == bd) sum += s_term[u * 6 + 3 + c];
    }
    out[i] = sum;
  }
}

static size_t frame_bwd_lds(int vmax, int maxc) {
  return (size_t)vmax * (2 * sizeof(double2) + sizeof(double)) + (size_t)maxc * 6 * sizeof(double) + (size_t)(3 * maxc + 1) * sizeof(int);
}

}  // namespace ctw

bool contacts_wide_supported(int nb, int nvcap, int scene_verts_max) {
  return nb >= 1 && nb <= ctw::MAXB && nvcap >= 8 && nvcap <= ctw::NV && scene_verts_max >= 0 &&
         scene_verts_max <= CONTACTS_WIDE_MAX_SCENE_VERTS;
}

int contacts_wide_launch(const ContactArgs& P, int nvcap, int scene_verts_max, void* stream) {
  if (!contacts_wide_supported(P.nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  const int vmax = ctw::vmax_of(scene_verts_max);
  const auto kernel = P.dt_in ? ctw::lcp_move_find_contacts_wide_kernel<true, false> : ctw::lcp_move_find_contacts_wide_kernel<false, false>;
  return ctw::launch_per_scene(kernel, P.B, 64, ctw::detect_lds(vmax), stream, P, nvcap, vmax, (int32_t*)nullptr);
}

int contacts_bp_launch(const ContactArgs& P, int nvcap, int scene_verts_max, int32_t* candidates, void* stream) {
  if (!contacts_wide_supported(P.nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  const int vmax = ctw::vmax_of(scene_verts_max);
  const auto kernel = P.dt_in ? ctw::lcp_move_find_contacts_wide_kernel<true, true> : ctw::lcp_move_find_contacts_wide_kernel<false, true>;
  return ctw::launch_per_scene(kernel, P.B, 64, ctw::detect_lds(vmax), stream, P, nvcap, vmax, candidates);
}

int contact_frame_backward_wide_launch(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind,
                                       const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                       double eps, const int32_t* count, const int32_t* c_i1, const int32_t* c_i2,
                                       const float* g_n, const float* g_p1, const float* g_p2, double* dp, void* stream) {
  if (!contacts_wide_supported(nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  const int vmax = ctw::vmax_of(scene_verts_max);
  const size_t lds = ctw::frame_bwd_lds(vmax, maxc);
  if (lds > ctw::LDS_LIMIT) return LCP_E_TOOLARGE;
  return ctw::launch_per_scene(ctw::lcp_contact_frame_backward_wide_kernel, B, ctw::FB_T, lds, stream, nb, maxc, nvcap, vmax, kind, radius,
                               verts_local, nverts, p, eps, count, c_i1, c_i2, g_n, g_p1, g_p2, dp);
}

}  // namespace lcp
