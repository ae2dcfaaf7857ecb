// lcp_contacts_bp.hip - the detection loop of lcp_contacts_wide.hip with a broadphase in front of the narrow phase.
//
// The reference never hands every pair to its contact handler: World.find_contacts (world.py:139-142) runs the geoms through ODE's
// HashSpace over bounding spheres padded by the margin (bodies.py:_create_geom), and only the surviving pairs reach
// DiffContactHandler.  lcp_move_find_contacts_wide_kernel walks all nb (nb - 1) / 2 pairs instead, 64 per pass, and a pass costs
// what its slowest lane costs - a full SAT + clip as soon as one lane's pair touches.  Here every trial pose first culls the pairs
// by bounding circle and bounding box (both widened by what the narrow phase's own gates allow, below), compacts the survivors IN PAIR ORDER into an LDS list, and the narrow phase walks that
// list: about one candidate per body on piles, i.e. one narrow pass where all pairs need up to 32.
//
// Same staging, mapping, move / detect / halve loop, padding and outputs as the wide kernel (one wave per scene, the scene's packed
// vertex list in dynamic LDS, lcp_contacts_geom.inc in a namespace of its own with NV = 64); every output is bitwise the wide
// kernel's, because a culled pair is one that collide_pair reports no point for (below) and the survivors keep their order.
//
// The cull rule is a relaxation of the gates collide_pair itself applies, so it drops nothing.  Per body b (convex, counter-clockwise,
// not degenerate: the contract of the geometry):
//   R_b        bounding radius about the position: the radius of a circle, max |verts_local| of a hull (once per launch);
//   box_b      (min, max) of the rotated vertices, relative to the position (a circle: -+ radius), at every trial pose;
//   mitre_b    (min, max) over the vertices k of m_k = (n_{k-1} + n_k) / (1 + n_{k-1} . n_k), n the outward unit edge normals: the
//              outward offset of the hull by r, as the intersection of its edges' half-planes moved out by r, has the vertices
//              v_k + r m_k (a circle: -+ 1);   kappa_b = max_k |m_k| = 1 / sin(smallest interior angle / 2) (a circle: 1).
// For the ordered pair (a, b), r = R_b + eps, S = R_a + kappa_a r and d = pos_b - pos_a, the test T(a, b) is
//     |d|^2 <= S^2 (1 + 4e-9)   and   box_a.min + r mitre_a.min - 1e-9 S <= d <= box_a.max + r mitre_a.max + 1e-9 S  on both axes;
// a pair i < j survives iff no_contact[i][j] is not set and T(i, j) and T(j, i) hold.
// Why nothing is lost.  hull / hull reports a point only after test_separations passed in both directions (hull_hull returns 0
// otherwise, before the clip): for every edge k of a, min over the vertices v of b of n_k . (v + d - v_k) <= eps.  Every vertex of b has
// n_k . v >= -R_b, so n_k . d - n_k . v_k <= R_b + eps for every k: d lies in the offset of hull a by r, a convex polygon whose vertices
// v_k + r m_k lie within R_a + kappa_a r of the origin and within the box above - that is T(a, b).  (The distance between the hulls
// is NOT bounded by eps: the separation is only tested along edge normals - two corners pass it up to eps / sin(angle / 2) apart -
// and the clip can then report an extrapolated point; kappa and the mitres account for exactly that.)  circle / hull reports a point
// only for a point of the hull (a convex combination of its vertices) within rad + eps of the centre, or, with the centre inside
// the hull, after the same edge test with R_b = rad: the centre lies in the same offset; in the other order S >= R_hull + rad + eps
// and the box is the disc's.  circle / circle returns 0 for |d| > r_a + r_b + eps, and T is that test and its box.
// The 1e-9 S slack only has to exceed the fp64 rounding of either side: a few ulp of coordinates of order 1e3, about 1e-12, against
// a slack of at least 1e-8 for bodies of size 10 and up.
//
// Every loop is bounded: the cull takes at most 32 iterations, the narrow pass ceil(candidates / 64) <= 32, the trials stop at
// max_trials; the barriers and the __all(done) exit are wave-uniform as in the wide kernel.
// Limits (checked on the host before a launch): those of lcp_contacts_wide.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_contacts_wide.h"

namespace lcp {
namespace ctw {
namespace bp {

constexpr int MAXPAIRS = MAXB * (MAXB - 1) / 2;      // 2016 candidates at most: (i << 8) | j in 16 bits, 4 KB

#define LCP_S double
#include "lcp_contacts_geom.inc"
#undef LCP_S

// DTS: every scene's loop starts from P.dt_in[scene] (compile-time, as in lcp_contacts_wide.hip)
template <bool DTS>
__global__ void __launch_bounds__(64) lcp_move_find_contacts_bp_kernel(ContactArgs P, int nvcap, int vmax, int32_t* candidates) {
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
  __shared__ double s_bound[MAXB];                          // R_b
  __shared__ V2 s_lo[MAXB], s_hi[MAXB];                     // box_b at the trial pose, relative to the position
  __shared__ V2 s_mlo[MAXB], s_mhi[MAXB];                   // mitre_b at the trial pose
  __shared__ double s_kap[MAXB];                            // kappa_b
  __shared__ uint16_t s_cand[MAXPAIRS];
  const int ll = threadIdx.x;
  const int scene = blockIdx.x;
  const int nb = P.nb;
  const int npairs = nb * (nb - 1) / 2;
  const int vtot = stage_bodies(scene, nb, nvcap, P.kind, P.nverts, P.radius, s_kind, s_off, s_rad);
  if (vtot > vmax) {                                      // the caller's scene_verts_max is too small: no detection, count = -1
    for (int slot = ll; slot < P.maxc; slot += 64) {
      const size_t o = (size_t)scene * P.maxc + slot;
      P.c_n[o * 2] = 0; P.c_n[o * 2 + 1] = 0; P.c_p1[o * 2] = 0; P.c_p1[o * 2 + 1] = 0; P.c_p2[o * 2] = 0; P.c_p2[o * 2 + 1] = 0;
      if (P.c_pen) P.c_pen[o] = 0;
      P.c_i1[o] = 0; P.c_i2[o] = 0;
    }
    if (ll == 0) { P.count[scene] = -1; if (candidates) candidates[scene] = 0; }
    return;
  }
  __syncthreads();
  // geometry does not change over the trials: stage it in LDS once
  for (int b = 0; b < nb; ++b) {
    const int o = s_off[b], n = s_off[b + 1] - o;
    const double* vl = P.verts_local + ((size_t)scene * nb + b) * nvcap * 2;
    for (int k = ll; k < n; k += 64) { s_vloc[o + k] = v2(vl[2 * k], vl[2 * k + 1]); s_vbody[o + k] = b; }
  }
  __syncthreads();
  // bounding radius about the body's position: pose-independent, one lane per body
  for (int b = ll; b < nb; b += 64) {
    double r = s_rad[b];
    if (s_kind[b] != 0) {
      const int o = s_off[b], n = s_off[b + 1] - o;
      double r2 = 0.0;
      for (int k = 0; k < n; ++k) { const double lx = s_vloc[o + k].x, ly = s_vloc[o + k].y; const double q = lx * lx + ly * ly; r2 = q > r2 ? q : r2; }
      r = sqrt(r2);
    }
    s_bound[b] = r;
  }
  double dt = DTS ? P.dt_in[scene] : P.dt;                  // per-scene starting dt (World.step(fixed_dt=True), world.py:72-80)
  const bool finished = DTS && dt <= 0.0;                      // the scene has reached its end_t: it stays where it is (one trial, no move)
  int base = 0, trial = 0, ncand = 0;
  double maxpen = -1e300;
  bool done = false;
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
    for (int idx = ll; idx < vtot; idx += 64) {
      const int bdy = s_vbody[idx];
      const double sn = s_sc[bdy].x, cs = s_sc[bdy].y;
      const double lx = s_vloc[idx].x, ly = s_vloc[idx].y;
      s_verts[idx] = v2(cs * lx - sn * ly, sn * lx + cs * ly);                      // utils.py:105-112
    }
    __syncthreads();
    // edge normals and lengths of every hull, once per trial pose
    for (int idx = ll; idx < vtot; idx += 64) {
      const int bdy = s_vbody[idx], o = s_off[bdy], nvb = s_off[bdy + 1] - o, k = idx - o;
      const V2 edge = s_verts[o + (k + 1) % nvb] - s_verts[idx];
      const double en = norm(edge);
      s_elen[idx] = en;
      s_nrm[idx] = left_orth(edge) * (1.0 / en);
    }
    __syncthreads();
    // box, mitre extents and kappa of every body at this pose (one lane per body; a hull without vertices is its position)
    for (int b = ll; b < nb; b += 64) {
      double x0 = -s_rad[b], x1 = s_rad[b], y0 = x0, y1 = x1;
      double mx0 = -1.0, mx1 = 1.0, my0 = -1.0, my1 = 1.0, k2 = 1.0;
      if (s_kind[b] != 0) {
        const int o = s_off[b], n = s_off[b + 1] - o;
        x0 = x1 = y0 = y1 = 0.0;
        if (n > 0) { x0 = x1 = s_verts[o].x; y0 = y1 = s_verts[o].y; mx0 = my0 = 1e300; mx1 = my1 = -1e300; k2 = 0.0; }
        for (int k = 0; k < n; ++k) {
          const double x = s_verts[o + k].x, y = s_verts[o + k].y;
          x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
          const V2 nc = s_nrm[o + k], np = s_nrm[o + (k + n - 1) % n];
          const double inv = 1.0 / (1.0 + (np.x * nc.x + np.y * nc.y));
          const double mx = (np.x + nc.x) * inv, my = (np.y + nc.y) * inv;
          mx0 = mx < mx0 ? mx : mx0; mx1 = mx > mx1 ? mx : mx1; my0 = my < my0 ? my : my0; my1 = my > my1 ? my : my1;
          const double q = mx * mx + my * my;
          k2 = q > k2 ? q : k2;
        }
      }
      s_lo[b] = v2(x0, y0); s_hi[b] = v2(x1, y1); s_mlo[b] = v2(mx0, my0); s_mhi[b] = v2(mx1, my1); s_kap[b] = sqrt(k2);
    }
    __syncthreads();
    // cull: all pairs in lexicographic order, the survivors compacted in that order
    ncand = 0;
    for (int p0 = 0; p0 < npairs; p0 += 64) {
      const int pr = p0 + ll;
      int bi = 0, bj = 1;
      bool keep = false;
      if (pr < npairs) {
        int rem = pr;                                           // pair index -> (i, j), i < j, lexicographic
        while (rem >= nb - 1 - bi) { rem -= nb - 1 - bi; ++bi; }
        bj = bi + 1 + rem;
        const bool skip = P.no_contact && P.no_contact[((size_t)scene * nb + bi) * nb + bj];
        double dx = s_pose[bj * 3 + 1] - s_pose[bi * 3 + 1], dy = s_pose[bj * 3 + 2] - s_pose[bi * 3 + 2];
        const double d2 = dx * dx + dy * dy;
        keep = !skip;
#pragma unroll
        for (int q = 0; q < 2; ++q) {                           // T(i, j), then T(j, i)
          const int a = q == 0 ? bi : bj, b = q == 0 ? bj : bi;
          const double r = s_bound[b] + P.eps;
          const double S = s_bound[a] + s_kap[a] * r;
          const double sl = 1e-9 * S;
          const V2 lo = s_lo[a], hi = s_hi[a], mlo = s_mlo[a], mhi = s_mhi[a];
          keep = keep && d2 <= S * S * (1.0 + 4e-9)
                 && dx <= hi.x + r * mhi.x + sl && dx >= lo.x + r * mlo.x - sl && dy <= hi.y + r * mhi.y + sl && dy >= lo.y + r * mlo.y - sl;
          dx = -dx; dy = -dy;
        }
      }
      const uint64_t mask = __ballot(keep);
      if (keep) s_cand[ncand + __popcll(mask & ((1ull << ll) - 1))] = (uint16_t)((bi << 8) | bj);
      ncand += __popcll(mask);
    }
    __syncthreads();
    base = 0; maxpen = -1e300;
    for (int c0 = 0; c0 < ncand; c0 += 64) {
      const int ci = c0 + ll;
      int cnt = 0, bi = 0, bj = 1;
      Pt pt0, pt1;
      pt0.n = v2(0, 0); pt0.p1 = pt0.n; pt0.p2 = pt0.n; pt0.pen = 0; pt1 = pt0;
      if (ci < ncand) {
        const int code = s_cand[ci];
        bi = code >> 8; bj = code & 255;
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
      // exclusive prefix sum of cnt over the wave (candidate order = pair order = the reference's contact order)
      int incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (ll >= off) incl += o; }
      const int excl = incl - cnt;
      const int total = __shfl(incl, 63, 64);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const Pt& pt = q == 0 ? pt0 : pt1;
        const int slot = base + excl + q;
        if (q < cnt && slot < P.maxc) {
          const size_t o = (size_t)scene * P.maxc + slot;
          P.c_n[o * 2] = (float)pt.n.x; P.c_n[o * 2 + 1] = (float)pt.n.y;
          P.c_p1[o * 2] = (float)pt.p1.x; P.c_p1[o * 2 + 1] = (float)pt.p1.y;
          P.c_p2[o * 2] = (float)pt.p2.x; P.c_p2[o * 2 + 1] = (float)pt.p2.y;
          if (P.c_pen) P.c_pen[o] = pt.pen;
          P.c_i1[o] = bi; P.c_i2[o] = bj;
        }
        if (q < cnt) maxpen = pt.pen > maxpen ? pt.pen : maxpen;
      }
      base += total;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(maxpen, off, 64); maxpen = o > maxpen ? o : maxpen; }
    ++trial;
    // world.py:95-101
    const bool ok = !(base > 0 && maxpen > P.tol);
    if (ok || (!P.strict && dt < P.dt_floor) || trial >= P.max_trials || !P.v || finished) done = true;   // (max_trials: the reference would spin)
    else dt *= 0.5;
    if (__all(done)) break;
    __syncthreads();
  }
  // pad the unused contact slots with a harmless record (no normal, bodies 0/0)
  const int nfill = base < P.maxc ? base : P.maxc;
  for (int slot = nfill + ll; slot < P.maxc; slot += 64) {
    const size_t o = (size_t)scene * P.maxc + slot;
    P.c_n[o * 2] = 0; P.c_n[o * 2 + 1] = 0; P.c_p1[o * 2] = 0; P.c_p1[o * 2 + 1] = 0; P.c_p2[o * 2] = 0; P.c_p2[o * 2 + 1] = 0;
    if (P.c_pen) P.c_pen[o] = 0;
    P.c_i1[o] = 0; P.c_i2[o] = 0;
  }
  if (P.p_out) for (int idx = ll; idx < nb * 3; idx += 64) P.p_out[(size_t)scene * nb * 3 + idx] = s_pose[idx];
  if (ll == 0) {
    P.count[scene] = base;                                  // may exceed maxc: the caller checks
    if (P.max_pen) P.max_pen[scene] = base > 0 ? maxpen : 0.0;
    if (P.dt_used) P.dt_used[scene] = finished ? 0.0 : dt;
    if (P.t && !finished) P.t[scene] += dt;                              // world.py:122
    if (P.trials) P.trials[scene] = trial;
    if (candidates) candidates[scene] = ncand;              // pairs that passed the cull at the accepted pose
  }
}

}  // namespace bp
}  // namespace ctw

int contacts_bp_launch(const ContactArgs& P, int nvcap, int scene_verts_max, int32_t* candidates, void* stream) {
  if (!contacts_wide_supported(P.nb, nvcap, scene_verts_max)) return LCP_E_TOOLARGE;
  const int vmax = ctw::vmax_of(scene_verts_max);
  const auto kernel = P.dt_in ? ctw::bp::lcp_move_find_contacts_bp_kernel<true> : ctw::bp::lcp_move_find_contacts_bp_kernel<false>;
  return ctw::launch_per_scene(kernel, P.B, 64, ctw::detect_lds(vmax), stream, P, nvcap, vmax, candidates);
}

}  // namespace lcp
