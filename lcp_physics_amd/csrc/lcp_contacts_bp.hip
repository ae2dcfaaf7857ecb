// lcp_contacts_bp.hip - the broadphase in front of the narrow phase: what the BP instantiations of the detection kernel of
// lcp_contacts_wide.hip (lcp_move_find_contacts_wide_kernel<DTS, true>, behind lcp_move_find_contacts_bp_f64) add to its trial loop.
// Not a unit of its own: lcp_contacts_wide.hip includes it, so that there is one trial loop and one instantiation of the geometry.
//
// The reference never hands every pair to its contact handler: World.find_contacts (world.py:139-142) runs the geoms through ODE's
// HashSpace over bounding spheres padded by the margin (bodies.py:_create_geom), and only the surviving pairs reach
// DiffContactHandler.  Without the broadphase the detection kernel walks all nb (nb - 1) / 2 pairs instead, 64 per pass, and a pass costs
// what its slowest lane costs - a full SAT + clip as soon as one lane's pair touches.  Here every trial pose first culls the pairs
// by bounding circle and bounding box (both widened by what the narrow phase's own gates allow, below), compacts the survivors IN PAIR ORDER into an LDS list, and the narrow phase walks that
// list: about one candidate per body on piles, i.e. one narrow pass where all pairs need up to 32.
//
// Staging, mapping, move / detect / halve loop, padding and outputs are the kernel's own, whichever way it is instantiated; every
// output is bitwise that of the instantiation without the broadphase, because a culled pair is one that collide_pair reports no point
// for (below) and the survivors keep their order.
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
// Every loop is bounded: the cull takes at most 32 iterations, the narrow pass ceil(candidates / 64) <= 32; the barrier inside
// cull_pairs is reached by the whole wave.
#ifndef LCP_CONTACTS_BP_HIP
#define LCP_CONTACTS_BP_HIP
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_contacts_wide.h"

namespace lcp {
namespace ctw {
namespace bp {

constexpr int MAXPAIRS = MAXB * (MAXB - 1) / 2;      // 2016 candidates at most: (i << 8) | j in 16 bits, 4 KB

// static LDS of the cull (V2: the geometry's vector of two doubles); only the BP instantiations name it
template <class V2>
struct CullLds {
  double bound[MAXB];                          // R_b
  V2 lo[MAXB], hi[MAXB];                       // box_b at the trial pose, relative to the position
  V2 mlo[MAXB], mhi[MAXB];                     // mitre_b at the trial pose
  double kap[MAXB];                            // kappa_b
  uint16_t cand[MAXPAIRS];                     // the surviving pairs (i << 8) | j, in pair order
};

// R_b, the bounding radius about the body's position: pose-independent, one lane per body (once per launch, after the body-frame
// vertices s_vloc are staged)
template <class V2>
__device__ __forceinline__ void bound_radii(int nb, const int* s_kind, const int* s_off, const double* s_rad, const V2* s_vloc,
                                            double* s_bound) {
  for (int b = threadIdx.x; b < nb; b += 64) {
    double r = s_rad[b];
    if (s_kind[b] != 0) {
      const int o = s_off[b], n = s_off[b + 1] - o;
      double r2 = 0.0;
      for (int k = 0; k < n; ++k) { const double lx = s_vloc[o + k].x, ly = s_vloc[o + k].y; const double q = lx * lx + ly * ly; r2 = q > r2 ? q : r2; }
      r = sqrt(r2);
    }
    s_bound[b] = r;
  }
}

// The cull at one trial pose (the rotated vertices and edge normals staged and a barrier passed): box, mitre extents and kappa of
// every body, a barrier, then T over all pairs in lexicographic order, the survivors compacted into L.cand in that order.
// Returns the number of survivors (the same on every lane); the caller's barrier comes before L.cand is read.
template <class V2>
__device__ __forceinline__ int cull_pairs(const ContactArgs& P, int scene, CullLds<V2>& L, const int* s_kind, const int* s_off,
                                          const double* s_rad, const double* s_pose, const V2* s_verts, const V2* s_nrm) {
  const int ll = threadIdx.x;
  const int nb = P.nb;
  const int npairs = nb * (nb - 1) / 2;
  // (one lane per body; a hull without vertices is its position)
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
    L.lo[b].x = x0; L.lo[b].y = y0; L.hi[b].x = x1; L.hi[b].y = y1;
    L.mlo[b].x = mx0; L.mlo[b].y = my0; L.mhi[b].x = mx1; L.mhi[b].y = my1;
    L.kap[b] = sqrt(k2);
  }
  __syncthreads();
  int ncand = 0;
  for (int p0 = 0; p0 < npairs; p0 += 64) {
    const int pr = p0 + ll;
    int bi = 0, bj = 1;
    bool keep = false;
    if (pr < npairs) {
      pair_of(pr, nb, bi, bj);
      const bool skip = P.no_contact && P.no_contact[((size_t)scene * nb + bi) * nb + bj];
      double dx = s_pose[bj * 3 + 1] - s_pose[bi * 3 + 1], dy = s_pose[bj * 3 + 2] - s_pose[bi * 3 + 2];
      const double d2 = dx * dx + dy * dy;
      keep = !skip;
#pragma unroll
      for (int q = 0; q < 2; ++q) {                           // T(i, j), then T(j, i)
        const int a = q == 0 ? bi : bj, b = q == 0 ? bj : bi;
        const double r = L.bound[b] + P.eps;
        const double S = L.bound[a] + L.kap[a] * r;
        const double sl = 1e-9 * S;
        const V2 lo = L.lo[a], hi = L.hi[a], mlo = L.mlo[a], mhi = L.mhi[a];
        keep = keep && d2 <= S * S * (1.0 + 4e-9)
               && dx <= hi.x + r * mhi.x + sl && dx >= lo.x + r * mlo.x - sl && dy <= hi.y + r * mhi.y + sl && dy >= lo.y + r * mlo.y - sl;
        dx = -dx; dy = -dy;
      }
    }
    const uint64_t mask = __ballot(keep);
    if (keep) L.cand[ncand + __popcll(mask & ((1ull << ll) - 1))] = (uint16_t)((bi << 8) | bj);
    ncand += __popcll(mask);
  }
  return ncand;
}

}  // namespace bp
}  // namespace ctw
}  // namespace lcp
#endif
