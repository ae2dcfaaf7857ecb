// lcp_contacts_wide.h - what the kernels over a scene's packed vertex list share (lcp_contacts_wide.hip: detection and the frame
// backward with respect to the pose; lcp_contacts_shape.hip: the frame backward with respect to the shape): the size limits, the
// dual number of the forward-mode derivatives, the per-scene body table and the host-side LDS helpers.
#ifndef LCP_CONTACTS_WIDE_H
#define LCP_CONTACTS_WIDE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_kernels.h"

namespace lcp {
namespace ctw {

constexpr int NV = 64;          // max vertices of a hull (GJK iteration cap of the geometry code: 4 NV)
constexpr int MAXB = 64;        // max bodies per scene (one lane per body in the offset scan)

// ---- forward-mode derivative (value + one directional derivative), as in lcp_contacts.hip ------------------------------
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

// ---- host side: what the launchers of these kernels share (the size limits themselves: contacts_wide_supported) -----------
constexpr size_t LDS_LIMIT = 160 * 1024 - 8 * 1024;    // (the static tables of the kernels take less than 8 KB)

// the `vmax` the kernels carve their dynamic arrays by: the caller's scene_verts_max, at least one slot
static int vmax_of(int scene_verts_max) { return scene_verts_max < 1 ? 1 : scene_verts_max; }

// dynamic LDS of the detection kernels (lcp_contacts_wide.hip, lcp_contacts_bp.hip): local and rotated vertices and edge normals
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
