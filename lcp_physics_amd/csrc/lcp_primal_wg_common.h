// lcp_primal_wg_common.h - what the two workgroup-per-scene units share (lcp_primal_wg.hip: the contact-list step;
// lcp_primal_wg_poststab.hip: post-stabilisation): ONE WORKGROUP of 256 threads per scene, the fp64 system in LDS.  Sizes and the
// head of the workspace, the scene-wide reductions, the right-looking LU with one barrier per pivot, the triangular sweeps of wave 0
// and the products with the A image.  Everything here is inlined into the kernels: the device code of both units is what it was when
// each carried these pieces itself (profiles/wg_shared_header.json).  The PDIPM loop, the per-contact block algebra, solve_kkt and
// the step lengths differ between the two LCPs and stay in the units.
#pragma once
#include "lcp_primal_common.h"

namespace lcp {
namespace wgc {

using namespace w64;
using namespace wsc;

constexpr int NT = 256;                 // threads per scene
constexpr int CAP = 128;                // pivots
// row stride: entry (r, c) in bank pair (r LDK + c) mod 32 - LDK = 1 (mod 32) spreads the diagonal blocks of the bodies over the banks
// (formation) and puts the entries of one column in different banks (the sweeps read a column across the lanes)
constexpr int LDK = CAP + 1;
constexpr int AST = 132;                // row stride of the A image (nz <= 129)
constexpr int MAXC = 256;               // contacts
// workspace per scene (doubles): [0] contact count | x [IT, IT + 136) | y [YO, YO + 8) | z, s from ZO: `per_contact` doubles a contact
constexpr int IT = 8, YO = IT + 136, ZO = YO + 8;
__host__ __device__ constexpr size_t ws_doubles(int ncap, int per_contact) { return (size_t)ZO + (size_t)per_contact * (size_t)ncap; }

// sizes every form takes: whole bodies, whole contacts (four rows each), at most MAXC of them
inline bool sizes_ok(int nz, int m, int e) { return nz > 0 && (nz % 3) == 0 && (m % 4) == 0 && m / 4 <= MAXC && e >= 0; }
// the general form: at most CAP pivots nz + neq, neq <= 4
inline bool general_form_fits(int nz, int m, int e) { return sizes_ok(nz, m, e) && e <= 4 && nz + e <= CAP; }

__device__ __forceinline__ void bsync() { __syncthreads(); }
__device__ __forceinline__ void lds_add_wg(double* p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // ds_add_f64 (no return)
}

// ---- scene-wide reductions: per wave by DPP, then the four wave results in a fixed order (r0 . r1) . (r2 . r3) ------------------
struct BlockReduce {
  double* redd;
  uint32_t* redu;
  int wv, lane;
  __device__ __forceinline__ double sum(double v) const {
    const double w = wave_sum(v);
    bsync(); if (lane == 0) redd[wv] = w; bsync();
    return (redd[0] + redd[1]) + (redd[2] + redd[3]);
  }
  __device__ __forceinline__ double min(double v) const {                          // NaN-ignoring, as wave_min
    const double w = wave_min(v);
    bsync(); if (lane == 0) redd[wv] = w; bsync();
    return __builtin_fmin(__builtin_fmin(redd[0], redd[1]), __builtin_fmin(redd[2], redd[3]));
  }
  __device__ __forceinline__ double max(double v) const {                          // NaN-ignoring, as wave_max
    const double w = wave_max(v);
    bsync(); if (lane == 0) redd[wv] = w; bsync();
    return __builtin_fmax(__builtin_fmax(redd[0], redd[1]), __builtin_fmax(redd[2], redd[3]));
  }
  __device__ __forceinline__ uint32_t umax(uint32_t v) const {
    const uint32_t w = wave_umax(v);
    bsync(); if (lane == 0) redu[wv] = w; bsync();
    return wsc::umax(wsc::umax(redu[0], redu[1]), wsc::umax(redu[2], redu[3]));
  }
  // OR of a word of BITS (3 or 5) bits.  One term per bit, written out: a loop over the bits reorders the scalar selects.
  template <int BITS> __device__ __forceinline__ uint32_t or_(uint32_t v) const {
    static_assert(BITS == 3 || BITS == 5, "three or five flag bits");
    uint32_t w = (__any((v & 1u) != 0u) ? 1u : 0u) | (__any((v & 2u) != 0u) ? 2u : 0u) | (__any((v & 4u) != 0u) ? 4u : 0u);
    if constexpr (BITS == 5) w = w | (__any((v & 8u) != 0u) ? 8u : 0u) | (__any((v & 16u) != 0u) ? 16u : 0u);
    bsync(); if (lane == 0) redu[wv] = w; bsync();
    return (redu[0] | redu[1]) | (redu[2] | redu[3]);
  }
  __device__ __forceinline__ bool any(bool b) const { return umax(b ? 1u : 0u) != 0u; }
};

// ---- right-looking LU without pivoting of the n x n system whose row i is row i + clo of the image (clo: the pinned coordinates'
// rows in front, 0 otherwise), one barrier per pivot: the pivot row in registers (lane j: columns k + 1 + j and k + 65 + j), wave w
// takes the rows k + 1 + w + 4 i.  Returns whether a pivot was zero or NaN (uniform: every thread read every pivot).
__device__ __forceinline__ bool lu_factor(double* Kl, int n, int clo, int wv, int lane) {
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    const double* prow = Kl + (k + clo) * LDK;
    const double piv = prow[k];
    bad = bad || !(piv != 0.0) || (piv != piv);
    const double inv = fast_rcp(piv);
    const int j0 = k + 1 + lane, j1 = j0 + 64;
    const double u0 = j0 < n ? prow[j0] : 0.0, u1 = j1 < n ? prow[j1] : 0.0;
    for (int i = k + 1 + wv; i < n; i += 4) {
      double* row = Kl + (i + clo) * LDK;
      const double l = row[k] * inv;
      if (j0 < n) row[j0] = fma(-l, u0, row[j0]);
      if (j1 < n) row[j1] = fma(-l, u1, row[j1]);
      if (lane == 0) row[k] = l;                                        // (after every lane's read of it: LDS serves a wave in order)
    }
    bsync();
  }
  return bad;
}

// ---- the triangular sweeps behind lu_factor, for wave 0 alone: lane l owns pivots l and l + 64, the solution entries travel by
// v_readlane, no barrier per step.  rv[clo, clo + n): the right-hand side in, the solution out.  The caller stores the right-hand
// side and puts a barrier in front and behind.
__device__ __forceinline__ void lu_sweeps(const double* Kl, double* rv, int n, int clo, int lane) {
  const int i0 = lane, i1 = lane + 64;
  const bool l0 = i0 < n, l1 = i1 < n;
  const double* r0p = Kl + ((l0 ? i0 : 0) + clo) * LDK;
  const double* r1p = Kl + ((l1 ? i1 : 0) + clo) * LDK;
  double r0 = l0 ? rv[i0 + clo] : 0.0, r1 = l1 ? rv[i1 + clo] : 0.0;
  // forward: unit lower factor, eight columns' entries asked for ahead of their steps
  for (int k0 = 0; k0 < n; k0 += 8) {
    double a0[8], a1[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) { const int k = k0 + kk < n ? k0 + kk : n - 1; a0[kk] = r0p[k]; a1[kk] = r1p[k]; }
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = k0 + kk;
      if (k < n) {
        const double yk = bcast_lane(k < 64 ? r0 : r1, k & 63);
        if (l0 && i0 > k) r0 = fma(-a0[kk], yk, r0);
        if (l1 && i1 > k) r1 = fma(-a1[kk], yk, r1);
      }
    }
  }
  const double ud0 = l0 ? fast_rcp(r0p[i0]) : 1.0, ud1 = l1 ? fast_rcp(r1p[i1]) : 1.0;
  // backward: upper factor, x_k = r_k / U[k][k]
  for (int k0 = n - 1; k0 >= 0; k0 -= 8) {
    double a0[8], a1[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) { const int k = k0 - kk >= 0 ? k0 - kk : 0; a0[kk] = r0p[k]; a1[kk] = r1p[k]; }
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = k0 - kk;
      if (k >= 0) {
        const double xk = bcast_lane(k < 64 ? r0 * ud0 : r1 * ud1, k & 63);
        if (l0 && i0 < k) r0 = fma(-a0[kk], xk, r0);
        if (l1 && i1 < k) r1 = fma(-a1[kk], xk, r1);
      }
    }
  }
  if (l0) rv[i0 + clo] = r0 * ud0;
  if (l1) rv[i1 + clo] = r1 * ud1;
}

// ---- products with the A image (e rows of nz floats, stride AST) through the exchange vector xv; general form: the equality
// multipliers sit on the threads nz .. nz + e - 1 (ve), row ya = tid - nz -------------------------------------------------------
__device__ __forceinline__ double Av(const float* At, double* xv, double v, int tid, int nz, bool vx, bool ve, int ya) {   // equality threads <- x threads
  xv[tid] = vx ? v : 0.0; bsync();
  double out = 0;
  if (ve) { const float* ar = At + ya * AST; for (int k = 0; k < nz; ++k) out = fma((double)ar[k], xv[k], out); }
  bsync();
  return out;
}
__device__ __forceinline__ double Aty(const float* At, double* xv, double y, int tid, int nz, int e, bool vx, bool ve) {   // x threads <- equality threads
  xv[tid] = ve ? y : 0.0; bsync();
  double acc = 0;
  if (vx) for (int a = 0; a < e; ++a) acc = fma((double)At[a * AST + tid], xv[nz + a], acc);
  bsync();
  return acc;
}

}  // namespace wgc
}  // namespace lcp
