// lcp_contacts_wide.h - what the contact kernels share.  All of them (lcp_contacts.hip too): the dual number of the forward-mode
// derivatives and the parts of the detection loop that do not depend on how a scene is staged.  The kernels over a scene's packed
// vertex list (lcp_contacts_wide.hip: detection, with the broadphase of lcp_contacts_bp.hip or without, and the frame backward with
// respect to the pose; lcp_contacts_shape.hip: the frame backward with respect to the shape): the size limits, the per-scene body
// table, the edge-normal pass, the scene staging of the two backward kernels and the host-side LDS helpers.
#ifndef LCP_CONTACTS_WIDE_H
#define LCP_CONTACTS_WIDE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_kernels.h"

namespace lcp {
namespace ctw {

constexpr int NV = 64;          // max vertices of a hull (GJK iteration cap of the geometry code: 4 NV)
constexpr int MAXB = 64;        // max bodies per scene (one lane per body in the offset scan)

// ---- forward-mode derivative: value + ONE directional derivative (every comparison looks at the values only) ----------------
namespace ad {
struct Dual {
  double v, d;
  __device__ __forceinline__ Dual() {}
  __device__ __forceinline__ Dual(double a) : v(a), d(0.0) {}
  __device__ __forceinline__ Dual(double a, double b) : v(a), d(b) {}
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual(a.v - b.v, a.d - b.d); }
__device__ __forceinline__ Dual operator-(Dual a) { return Dual(-a.v, -a.d); }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return Dual(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) { const double q = a.v / b.v; return Dual(q, (a.d - q * b.d) / b.v); }
__device__ __forceinline__ Dual sqrt(Dual a) { const double r = ::sqrt(a.v); return Dual(r, 0.5 * a.d / r); }
__device__ __forceinline__ bool operator<(Dual a, Dual b) { return a.v < b.v; }
__device__ __forceinline__ bool operator<=(Dual a, Dual b) { return a.v <= b.v; }
__device__ __forceinline__ bool operator>(Dual a, Dual b) { return a.v > b.v; }
__device__ __forceinline__ bool operator>=(Dual a, Dual b) { return a.v >= b.v; }
__device__ __forceinline__ bool operator==(Dual a, Dual b) { return a.v == b.v; }
}  // namespace ad

// ---- the parts of the detection loop (World.step_dt's move / detect / halve loop, world.py:88-101) of a kernel with one wave per
// scene, ll = the lane.  (lcp_move_find_contacts_kernel of lcp_contacts.hip, the kernel of the benchmarked small worlds with 16 or 64
// lanes per scene, states the same parts in its own text: with any of these in their place its instruction stream is no longer the
// one that was measured - profiles/contacts_shared_staging.json.)

// pair index -> (i, j), i < j, lexicographic
__device__ __forceinline__ void pair_of(int pr, int nb, int& bi, int& bj) {
  int rem = pr;
  bi = 0;
  while (rem >= nb - 1 - bi) { rem -= nb - 1 - bi; ++bi; }
  bj = bi + 1 + rem;
}

// the harmless record (no normal, bodies 0/0) in the contact slots [from, maxc) of a scene
__device__ __forceinline__ void pad_records(const ContactArgs& P, int scene, int ll, int from) {
  for (int slot = from + ll; slot < P.maxc; slot += 64) {
    const size_t o = (size_t)scene * P.maxc + slot;
    P.c_n[o * 2] = 0; P.c_n[o * 2 + 1] = 0; P.c_p1[o * 2] = 0; P.c_p1[o * 2 + 1] = 0; P.c_p2[o * 2] = 0; P.c_p2[o * 2 + 1] = 0;
    if (P.c_pen) P.c_pen[o] = 0;
    P.c_i1[o] = 0; P.c_i2[o] = 0;
  }
}

// One pass of the pair loop: every lane brings the cnt (0..2) points pt0, pt1 of its pair (bi, bj).  The records go to the slots
// base + (exclusive prefix sum of cnt over the wave) - lane order = pair order = the reference's contact order - while they fit in
// maxc; maxpen takes the lane's deepest penetration.  Returns the pass's number of records.
template <class Pt>
__device__ __forceinline__ int store_records(const ContactArgs& P, int scene, int ll, int base, int cnt, int bi, int bj,
                                             const Pt& pt0, const Pt& pt1, double& maxpen) {
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
  return total;
}

// the deepest penetration over the lanes of the scene
__device__ __forceinline__ double scene_max(double maxpen) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(maxpen, off, 64); maxpen = o > maxpen ? o : maxpen; }
  return maxpen;
}

// world.py:95-101 after trial number `trial` (counted from 1) found `base` records: true = the scene keeps this trial's pose and dt,
// false = dt was halved for another trial.  (max_trials: the reference would spin)
__device__ __forceinline__ bool accept_or_halve(const ContactArgs& P, int base, double maxpen, int trial, bool finished, double& dt) {
  const bool ok = !(base > 0 && maxpen > P.tol);
  if (ok || (!P.strict && dt < P.dt_floor) || trial >= P.max_trials || !P.v || finished) return true;
  dt *= 0.5;
  return false;
}

// what a scene leaves behind: the unused contact slots padded, the accepted pose, and the per-scene outputs
__device__ __forceinline__ void scene_outputs(const ContactArgs& P, int scene, int ll, const double* s_pose, int base, double maxpen,
                                              double dt, int trial, bool finished) {
  pad_records(P, scene, ll, base < P.maxc ? base : P.maxc);
  if (P.p_out) for (int idx = ll; idx < P.nb * 3; idx += 64) P.p_out[(size_t)scene * P.nb * 3 + idx] = s_pose[idx];
  if (ll == 0) {
    P.count[scene] = base;                                  // may exceed maxc: the caller checks
    if (P.max_pen) P.max_pen[scene] = base > 0 ? maxpen : 0.0;
    if (P.dt_used) P.dt_used[scene] = finished ? 0.0 : dt;
    if (P.t && !finished) P.t[scene] += dt;                              // world.py:122
    if (P.trials) P.trials[scene] = trial;
  }
}

// Per-scene body table in LDS (static) and the packed vertex offsets: lane b of the (first) wave scans nverts.  A hull
// contributes min(max(nverts, 0), nvcap) vertices, a circle none.  Returns the scene's vertex total (all lanes).
__device__ __forceinline__ int stage_bodies(int scene, int nb, int nvcap, const int32_t* kind, const int32_t* nverts,
                                            const double* radius, int* s_kind, int* s_off, double* s_rad) {
  const int lane = threadIdx.x & 63;
  int nvb = 0;
  if (lane < nb) {
    const int k = kind[(size_t)scene * nb + lane];
    int n = nverts[(size_t)scene * nb + lane];
    n = n < 0 ? 0 : (n > nvcap ? nvcap : n);
    nvb = k != 0 ? n : 0;
    if (threadIdx.x < 64) { s_kind[lane] = k; s_rad[lane] = radius[(size_t)scene * nb + lane]; }
  }
  int incl = nvb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
  if (threadIdx.x < 64 && lane < nb) { s_off[lane + 1] = incl; if (lane == 0) s_off[0] = 0; }
  return __shfl(incl, 63, 64);
}

// ---- a scene's rotated geometry: the ONE arithmetic of the detection kernel and of the two frame-backward kernels.  The backward
// kernels re-run collide_pair from these values and must take the branches the detection took; V = the geometry's V2 or double2. ----
// vertex (lx, ly) of the body frame turned by the rotation whose (sin, cos) is sc                       utils.py:105-112
template <class V, class SC>
__device__ __forceinline__ V turned(SC sc, double lx, double ly) {
  const double sn = sc.x, cs = sc.y;
  V r; r.x = cs * lx - sn * ly; r.y = sn * lx + cs * ly;
  return r;
}
// edge (k, k + 1) of the hull with the n rotated vertices v[0..n): its length, and left_orth(edge) / |edge|, the outward unit normal
template <class V>
__device__ __forceinline__ void edge_normal(const V* v, int n, int k, V& nrm, double& len) {
  const V a = v[k], c = v[(k + 1) % n];
  const double ex = c.x - a.x, ey = c.y - a.y;
  const double en = ::sqrt(ex * ex + ey * ey);
  const double inv = 1.0 / en;
  len = en;
  nrm.x = ey * inv; nrm.y = -ex * inv;
}

// What the two frame-backward kernels (T threads, one workgroup per scene) stage after stage_bodies: the pose; the work units = the
// distinct pairs among the first min(count, maxc) records (a pair's records are consecutive: unit u covers the records
// [s_ustart[u], s_ustart[u + 1]) of the bodies s_ub1[u], s_ub2[u]); (sin, cos) of every rotation; the rotated vertices, edge normals
// and edge lengths of the packed vertex list.  Ends with a barrier; returns the number of units.
template <int T>
__device__ __forceinline__ int stage_frame_scene(int scene, int nb, int maxc, int nvcap, const double* verts_local, const double* p,
                                                 const int32_t* count, const int32_t* c_i1, const int32_t* c_i2, const int* s_off,
                                                 double* s_pose, double2* s_sc, double2* s_verts, double2* s_nrm, double* s_elen,
                                                 int* s_ustart, int* s_ub1, int* s_ub2, int* s_nunits) {
  const int tid = threadIdx.x;
  int ntot = count[scene];
  ntot = ntot < 0 ? 0 : (ntot > maxc ? maxc : ntot);
  for (int i = tid; i < nb * 3; i += T) s_pose[i] = p[(size_t)scene * nb * 3 + i];
  // the work units: wave 0 flags the records that start a pair and compacts their indices with a ballot
  if (tid < 64) {
    int nu = 0;
    for (int r0 = 0; r0 < ntot; r0 += 64) {
      const int r = r0 + tid;
      int i1 = 0, i2 = 0;
      bool start = false;
      if (r < ntot) {
        const size_t o = (size_t)scene * maxc + r;
        i1 = c_i1[o]; i2 = c_i2[o];
        start = r == 0 || i1 != c_i1[o - 1] || i2 != c_i2[o - 1];
        i1 = i1 < 0 ? 0 : (i1 >= nb ? nb - 1 : i1); i2 = i2 < 0 ? 0 : (i2 >= nb ? nb - 1 : i2);   // (body indices stay in the table)
      }
      const uint64_t m = __ballot(start);
      if (start) {
        const int u = nu + __popcll(m & ((1ull << tid) - 1));
        s_ustart[u] = r; s_ub1[u] = i1; s_ub2[u] = i2;
      }
      nu += __popcll(m);
    }
    if (tid == 0) { s_ustart[nu] = ntot; *s_nunits = nu; }
  }
  __syncthreads();
  for (int b = tid; b < nb; b += T) { const double rot = s_pose[b * 3]; s_sc[b] = make_double2(sin(rot), cos(rot)); }
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int o = s_off[b], n = s_off[b + 1] - o;
    const double* vl = verts_local + ((size_t)scene * nb + b) * nvcap * 2;
    for (int k = tid; k < n; k += T) s_verts[o + k] = turned<double2>(s_sc[b], vl[2 * k], vl[2 * k + 1]);
  }
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int o = s_off[b], n = s_off[b + 1] - o;
    for (int k = tid; k < n; k += T) edge_normal(s_verts + o, n, k, s_nrm[o + k], s_elen[o + k]);
  }
  __syncthreads();
  return *s_nunits;
}

// ---- host side: what the launchers of these kernels share (the size limits themselves: contacts_wide_supported) -----------
constexpr size_t LDS_LIMIT = 160 * 1024 - 8 * 1024;    // (the static tables of the kernels take less than 8 KB)

// the `vmax` the kernels carve their dynamic arrays by: the caller's scene_verts_max, at least one slot
static int vmax_of(int scene_verts_max) { return scene_verts_max < 1 ? 1 : scene_verts_max; }

// dynamic LDS of the detection kernel (lcp_contacts_wide.hip, with the broadphase and without): local and rotated vertices and edge normals
// (V2 = two doubles), edge lengths, owning bodies
static size_t detect_lds(int vmax) { return (size_t)vmax * (3 * sizeof(double2) + sizeof(double) + sizeof(int)); }

// One workgroup of `threads` per scene with `lds` bytes of dynamic LDS (opted in to beyond the 64 KB every kernel may have)
template <typename K, typename... A>
static int launch_per_scene(K kernel, int B, int threads, size_t lds, void* stream, A... args) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return LCP_E_LAUNCH;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(threads), lds, (hipStream_t)stream, args...);
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace ctw
}  // namespace lcp
#endif
