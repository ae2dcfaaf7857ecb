// lcp_report.hip - contact reports: the impulses a solve applied, per body, per body pair and per joint.
//
// include/lcp_hip.h ("contact reports") states the rule: at a solution M (v_new - v) - dt f = G^T z + Je^T y, and this unit evaluates
// the two terms on the right from the multipliers a solve wrote and the records it consumed.
//
// Mapping (that of lcp_forces.hip).  A group of G lanes serves one scene, G the power of two >= max(nb, min(maxc, 256)), at most 256; a
// workgroup has max(64, G) threads and so holds 64 / G scenes where G < 64: 4 bodies x 16 contacts are four scenes in one wavefront.
//   phase 1, lane = record (stride G): the record's impulse j = zn n + zt d, its torques about the two bodies' centres, zn and the two
//            bodies into LDS, 48 bytes a record, 48 KB at maxc = 1024 (one scene per workgroup there); only the scene's first
//            min(c_count, maxc) records are staged, and none of an inactive scene
//   phase 2, lane = body: it walks the scene's staged records IN RECORD ORDER and adds what is addressed to it, in fp64; one rounding at
//            the store.  The walk reads one LDS address per group (a broadcast).
//   phase 3, lane = pair (stride G): the same walk, keeping the records between the pair's two bodies
//   phase 4, lane = body coordinate (stride G): the column sum of Je^T y over the rows in order; consecutive lanes read consecutive
//            columns of a row
// Every output element belongs to one lane: no atomics, the same bits every run.  Phases 2 to 4 only read LDS, so one barrier suffices.
#include <hip/hip_runtime.h>

#include "lcp_kernels.h"

namespace lcp {
namespace report {

constexpr int MAXB = 64, MAXC = 1024, MAXP = 1024;
constexpr size_t SLOT_BYTES = 5 * sizeof(double) + 2 * sizeof(int);    // t1, t2, jx, jy, zn, i1, i2

struct Outputs {
  float *body_impulse, *body_normal;
  int32_t* body_touching;
  float *joint_impulse, *pair_impulse, *pair_normal;
  int32_t* pair_contacts;
};

// `shift`: log2 of the lanes a scene has (G); the workgroup holds blockDim.x >> shift scenes
__global__ void __launch_bounds__(256) lcp_contact_report_kernel(int B, int nb, int maxc, int e, int P, int shift, const int32_t* c_count,
                                                                 const int32_t* active, const float* c_n, const float* c_p1,
                                                                 const float* c_p2, const int32_t* c_i1, const int32_t* c_i2,
                                                                 const float* z, const float* y, const float* Je,
                                                                 const int32_t* pair_first, const int32_t* pair_second,
                                                                 double min_impulse, Outputs out) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int G = 1 << shift;
  const int slots = ((int)blockDim.x >> shift) * maxc;
  double *s_t1 = s_dyn, *s_t2 = s_t1 + slots, *s_jx = s_t2 + slots, *s_jy = s_jx + slots, *s_zn = s_jy + slots;
  int *s_i1 = reinterpret_cast<int*>(s_zn + slots), *s_i2 = s_i1 + slots;
  const int sub = (int)threadIdx.x >> shift, gl = (int)threadIdx.x & (G - 1);
  const long long scene = (long long)blockIdx.x * ((int)blockDim.x >> shift) + sub;
  const bool ok = scene < B;
  const bool on = ok && (!active || active[scene] != 0);
  int n = 0;                                                                               // the records of this scene
  if (on) {
    n = c_count ? c_count[scene] : maxc;
    n = n < 0 ? 0 : (n > maxc ? maxc : n);
  }
  const int base = sub * maxc;
  // ---- phase 1: lane = record
  if (n > 0) {
    const float* zs = z + (size_t)scene * 4 * maxc;
    for (int c = gl; c < n; c += G) {
      const size_t r = (size_t)scene * maxc + c;
      const double zn = (double)zs[c], zt = (double)zs[maxc + 2 * c] - (double)zs[maxc + 2 * c + 1];
      const double nx = (double)c_n[2 * r], ny = (double)c_n[2 * r + 1];
      const double jx = zn * nx + zt * ny, jy = zn * ny - zt * nx;                         // d = left_orthogonal(n) = (ny, -nx)
      const double p1x = (double)c_p1[2 * r], p1y = (double)c_p1[2 * r + 1], p2x = (double)c_p2[2 * r], p2y = (double)c_p2[2 * r + 1];
      const int j = base + c;
      s_t1[j] = p1x * jy - p1y * jx;                                                       // cross_2d(c_p1, j)
      s_t2[j] = -(p2x * jy - p2y * jx);                                                    // -cross_2d(c_p2, j)
      s_jx[j] = jx; s_jy[j] = jy; s_zn[j] = zn;
      s_i1[j] = c_i1[r]; s_i2[j] = c_i2[r];
    }
  }
  __syncthreads();
  if (!ok) return;
  // ---- phase 2: lane = body
  if (gl < nb) {
    const int b = gl;
    double st = 0.0, sx = 0.0, sy = 0.0, sn = 0.0;
    int touching = 0;
    for (int c = 0; c < n; ++c) {
      const int j = base + c;
      const bool first = s_i1[j] == b, second = s_i2[j] == b;
      if (first) { st += s_t1[j]; sx += s_jx[j]; sy += s_jy[j]; }
      if (second) { st += s_t2[j]; sx -= s_jx[j]; sy -= s_jy[j]; }
      if (first || second) { sn += s_zn[j]; touching += s_zn[j] > min_impulse ? 1 : 0; }
    }
    const size_t o = (size_t)scene * nb + b;
    if (out.body_impulse) { out.body_impulse[3 * o] = (float)st; out.body_impulse[3 * o + 1] = (float)sx; out.body_impulse[3 * o + 2] = (float)sy; }
    if (out.body_normal) out.body_normal[o] = (float)sn;
    if (out.body_touching) out.body_touching[o] = touching;
  }
  // ---- phase 3: lane = pair
  if (out.pair_impulse || out.pair_normal || out.pair_contacts) {
    for (int q = gl; q < P; q += G) {
      const size_t o = (size_t)scene * P + q;
      const int f = pair_first[o], s = pair_second[o];
      double st = 0.0, sx = 0.0, sy = 0.0, sn = 0.0;
      int contacts = 0;
      if (f != s && f >= 0 && f < nb && s >= 0 && s < nb) {
        for (int c = 0; c < n; ++c) {
          const int j = base + c;
          const int i1 = s_i1[j], i2 = s_i2[j];
          const bool fwd = i1 == f && i2 == s, rev = i1 == s && i2 == f;
          if (fwd) { st += s_t1[j]; sx += s_jx[j]; sy += s_jy[j]; }
          if (rev) { st += s_t2[j]; sx -= s_jx[j]; sy -= s_jy[j]; }
          if (fwd || rev) { sn += s_zn[j]; contacts += s_zn[j] > min_impulse ? 1 : 0; }
        }
      }
      if (out.pair_impulse) { out.pair_impulse[3 * o] = (float)st; out.pair_impulse[3 * o + 1] = (float)sx; out.pair_impulse[3 * o + 2] = (float)sy; }
      if (out.pair_normal) out.pair_normal[o] = (float)sn;
      if (out.pair_contacts) out.pair_contacts[o] = contacts;
    }
  }
  // ---- phase 4: lane = body coordinate
  if (out.joint_impulse) {
    const int nz = 3 * nb;
    const bool joints = on && e > 0 && y && Je;
    const float* ys = joints ? y + (size_t)scene * e : nullptr;
    const float* Js = joints ? Je + (size_t)scene * e * nz : nullptr;
    for (int k = gl; k < nz; k += G) {
      double s = 0.0;
      if (joints)
        for (int r = 0; r < e; ++r) s += (double)Js[(size_t)r * nz + k] * (double)ys[r];
      out.joint_impulse[(size_t)scene * nz + k] = (float)s;
    }
  }
}

}  // namespace report

bool contact_report_supported(int nb, int maxc, int P) {
  return nb >= 1 && nb <= report::MAXB && maxc >= 1 && maxc <= report::MAXC && P >= 0 && P <= report::MAXP;
}

int contact_report_launch(int B, int nb, int maxc, int e, int P, const int32_t* c_count, const int32_t* active, const float* c_n,
                          const float* c_p1, const float* c_p2, const int32_t* c_i1, const int32_t* c_i2, const float* z, const float* y,
                          const float* Je, const int32_t* pair_first, const int32_t* pair_second, double min_impulse, float* body_impulse,
                          float* body_normal, int32_t* body_touching, float* joint_impulse, float* pair_impulse, float* pair_normal,
                          int32_t* pair_contacts, void* stream) {
  using namespace report;
  if (!contact_report_supported(nb, maxc, P)) return LCP_E_TOOLARGE;
  const int need = nb > (maxc < 256 ? maxc : 256) ? nb : (maxc < 256 ? maxc : 256);
  int shift = 0;
  while ((1 << shift) < need && shift < 8) ++shift;
  const int threads = (1 << shift) < 64 ? 64 : (1 << shift);
  const int scenes = threads >> shift;
  const long long blocks = ((long long)B + scenes - 1) / scenes;
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
  const size_t lds = SLOT_BYTES * (size_t)maxc * scenes;                                   // (at most 48 KB: no opt-in)
  Outputs out{body_impulse, body_normal, body_touching, joint_impulse, pair_impulse, pair_normal, pair_contacts};
  void* args[] = {&B, &nb, &maxc, &e, &P, &shift, &c_count, &active, &c_n, &c_p1, &c_p2, &c_i1, &c_i2, &z, &y, &Je, &pair_first,
                  &pair_second, &min_impulse, &out};
  if (hipLaunchKernel(reinterpret_cast<const void*>(lcp_contact_report_kernel), dim3((unsigned)blocks), dim3(threads), args, lds,
                      (hipStream_t)stream) != hipSuccess)
    return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace lcp
