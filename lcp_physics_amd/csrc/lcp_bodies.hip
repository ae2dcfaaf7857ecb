// lcp_bodies.hip - the reference's body constructors on the device: mass properties and gravity from shape and mass.
//
// What Circle / Hull / Rect.__init__ (physics/bodies.py:15-290) and Gravity.set_body (forces.py:64-67) compute from the RAW
// description of a body - the radius, or the vertices relative to the reference point in the reference's order, and the mass:
//   circle   centroid 0, I = m r^2 / 2                                                    (bodies.py:125-126)
//   hull     c = 1/6 sum x_i (v_i + v_i+1) / sum x_i / 2,  x_i = cross_2d(v_i+1, v_i)       (bodies.py:216-226, utils.py:93-96)
//            u_i = v_i - c                                                                (bodies.py:171)
//            I = 1/6 m sum |x(u_i+1, u_i)| (u_i.u_i + u_i.u_i+1 + u_i+1.u_i+1) / sum |x(u_i+1, u_i)|     (bodies.py:179-189)
//   M = diag(I, m, m) (bodies.py:44-47),  f_gravity = (0, 0, m g).
// In the reference all of this is inside autograd; lcp_body_properties_backward_kernel is its chain rule, recomputing c and u from
// the raw inputs (no saved state).
//
// Mapping: a streaming kernel, 16 B per vertex in and out.  A body owns L = cap rounded up to a power of two consecutive lanes,
// lane = edge (vertex e and its successor): 8 bodies per wavefront at cap 8, one at cap 64, so a wavefront's vertex loads and
// stores are contiguous.  The successor / predecessor values come through cross-lane shuffles inside the body's lanes, the sums
// are xor butterflies over the L lanes (no LDS, no atomics): lanes >= nv, circles and the tail bodies of the last wavefront add
// exact zeros, every lane of a body ends with the same bits, and the order of the additions depends on nv and cap only, not on
// where the body lies in the batch.  Control flow around the shuffles is uniform; kinds are told apart by selects.
// Vertex slots >= nv are never read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_kernels.h"

namespace lcp {
namespace bodies {

constexpr int BD_T = 256;       // threads per workgroup (four wavefronts)

template <int L>
__device__ __forceinline__ double seg_sum(double s) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);     // (o < L: the partner is a lane of the same body)
  return s;
}
template <int L>
__device__ __forceinline__ bool seg_any(bool f, int lane) {
  const uint64_t m = __ballot(f);
  const uint64_t seg = L == 64 ? ~0ull : (((1ull << (L & 63)) - 1) << (lane & ~(L - 1)));
  return (m & seg) != 0;
}
__device__ __forceinline__ double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }   // utils.py:93-96

// What both kernels need of a body: its raw vertex e and the successor, the centroid and the recentred pair.
struct Edge {
  bool hull, live;              // a hull body; lane e < nv of one
  int nv, next, prev;           // vertices read (0 for a circle, a tail body and a bad count), cyclic neighbours as lanes of the wave
  double vx, vy, wx, wy;        // v_e, v_e+1 (zeros on a lane that is not live)
  double xv, A;                 // x(v_e+1, v_e) and its sum
  double cx, cy;                // centroid
  double ux, uy, tx, ty;        // u_e, u_e+1
};

template <int L>
__device__ __forceinline__ Edge load_edge(long long body, long long nbody, int e, int lane, int cap, const int32_t* kind,
                                          const int32_t* nverts, const double* verts_raw, int& nv_given) {
  Edge E;
  const bool in = body < nbody;
  const int k = in ? kind[body] : 0;
  nv_given = in && k != 0 ? nverts[body] : 0;
  E.hull = in && k != 0;
  E.nv = nv_given < 0 ? 0 : (nv_given > cap ? cap : nv_given);
  E.live = e < E.nv;
  E.vx = 0.0; E.vy = 0.0;
  if (E.live) {
    const double2 v = *reinterpret_cast<const double2*>(verts_raw + ((size_t)body * cap + e) * 2);
    E.vx = v.x; E.vy = v.y;
  }
  const int base = lane & ~(L - 1);
  E.next = base + (e + 1 >= E.nv ? 0 : e + 1);
  E.prev = base + (e == 0 ? (E.nv > 0 ? E.nv - 1 : 0) : e - 1);
  E.wx = __shfl(E.vx, E.next, 64); E.wy = __shfl(E.vy, E.next, 64);
  E.xv = E.live ? cross2(E.wx, E.wy, E.vx, E.vy) : 0.0;
  const double sx = E.vx + E.wx, sy = E.vy + E.wy;
  E.A = seg_sum<L>(E.xv);
  const double nx = seg_sum<L>(E.live ? E.xv * sx : 0.0), ny = seg_sum<L>(E.live ? E.xv * sy : 0.0);
  const double den = 0.5 * E.A;                                          // bodies.py:225: the sum of cross / 2
  E.cx = E.hull ? (1.0 / 6.0) * nx / den : 0.0;                           // bodies.py:226
  E.cy = E.hull ? (1.0 / 6.0) * ny / den : 0.0;
  E.ux = E.live ? E.vx - E.cx : 0.0; E.uy = E.live ? E.vy - E.cy : 0.0;
  E.tx = E.live ? E.wx - E.cx : 0.0; E.ty = E.live ? E.wy - E.cy : 0.0;
  return E;
}

__device__ __forceinline__ bool finite(double x) { return (x - x) == 0.0; }

template <int L>
__global__ void __launch_bounds__(BD_T) lcp_body_properties_kernel(long long nbody, int cap, const int32_t* kind, const double* radius,
                                                                  const double* verts_raw, const int32_t* nverts, const double* mass,
                                                                  double g, double* centroid, double* verts_local, double* inertia,
                                                                  float* Mdiag, float* f_gravity, int32_t* status) {
  const long long gid = (long long)blockIdx.x * BD_T + threadIdx.x;
  const long long body = gid / L;
  const int e = (int)(gid & (L - 1)), lane = threadIdx.x & 63;
  int nv_given;
  const Edge E = load_edge<L>(body, nbody, e, lane, cap, kind, nverts, verts_raw, nv_given);
  const bool in = body < nbody;
  // the orientation test of bodies.py:228-235 and the turn of each pair of consecutive edges
  const double cw = seg_sum<L>(E.live ? (E.wx - E.vx) * (E.wy + E.vy) : 0.0);
  const double zx = __shfl(E.wx, E.next, 64), zy = __shfl(E.wy, E.next, 64);          // v_e+2
  const double turn = cross2(E.wx - E.vx, E.wy - E.vy, zx - E.wx, zy - E.wy);
  const bool against = seg_any<L>(E.live && turn * E.A > 0.0, lane);                 // (a convex polygon of either orientation: turn A < 0)
  // bodies.py:179-189 on the recentred vertices
  const double w = E.live ? fabs(cross2(E.tx, E.ty, E.ux, E.uy)) : 0.0;
  const double q = E.ux * E.ux + E.uy * E.uy + (E.ux * E.tx + E.uy * E.ty) + (E.tx * E.tx + E.ty * E.ty);
  const double num = seg_sum<L>(w * q), den = seg_sum<L>(w);
  if (!in) return;
  const double m = mass[body], r = radius[body];
  const double I = E.hull ? (1.0 / 6.0) * m * num / den : m * r * r / 2;               // bodies.py:189, :126
  if (verts_local && e < cap) {
    double2 o; o.x = E.ux; o.y = E.uy;                                                // (slots >= nv and circles: zeros)
    *reinterpret_cast<double2*>(verts_local + ((size_t)body * cap + e) * 2) = o;
  }
  if (e != 0) return;
  if (centroid) { centroid[body * 2] = E.cx; centroid[body * 2 + 1] = E.cy; }
  if (inertia) inertia[body] = I;
  if (Mdiag) { Mdiag[body * 3] = (float)I; Mdiag[body * 3 + 1] = (float)m; Mdiag[body * 3 + 2] = (float)m; }
  if (f_gravity) { f_gravity[body * 3] = 0.0f; f_gravity[body * 3 + 1] = 0.0f; f_gravity[body * 3 + 2] = (float)(m * g); }
  if (status) {
    int st = 0;
    if (!E.hull) {
      if (!finite(r) || !finite(m)) st = LCP_BODY_ST_DEGENERATE;
    } else if (nv_given < 3 || nv_given > cap) {
      st = LCP_BODY_ST_COUNT;
    } else if (!(E.A != 0.0) || !finite(E.A) || !finite(m)) {
      st = LCP_BODY_ST_DEGENERATE;
    } else {
      if (cw >= 0.0) st |= LCP_BODY_ST_ORIENTATION;
      if (against) st |= LCP_BODY_ST_NONCONVEX;
    }
    status[body] = st;
  }
}

template <int L>
__global__ void __launch_bounds__(BD_T) lcp_body_properties_backward_kernel(long long nbody, int cap, const int32_t* kind,
                                                                           const double* radius, const double* verts_raw,
                                                                           const int32_t* nverts, const double* mass, double g,
                                                                           const double* g_centroid, const double* g_verts_local,
                                                                           const double* g_inertia, const float* g_Mdiag,
                                                                           const float* g_f, double* g_verts_raw, double* g_radius,
                                                                           double* g_mass) {
  const long long gid = (long long)blockIdx.x * BD_T + threadIdx.x;
  const long long body = gid / L;
  const int e = (int)(gid & (L - 1)), lane = threadIdx.x & 63;
  int nv_given;
  const Edge E = load_edge<L>(body, nbody, e, lane, cap, kind, nverts, verts_raw, nv_given);
  const bool in = body < nbody;
  double m = 0.0, gI = 0.0, gcx = 0.0, gcy = 0.0, gux = 0.0, guy = 0.0;
  if (in) {
    m = mass[body];
    if (g_inertia) gI = g_inertia[body];
    if (g_Mdiag) gI += (double)g_Mdiag[body * 3];
    if (g_centroid && E.hull) { gcx = g_centroid[body * 2]; gcy = g_centroid[body * 2 + 1]; }
    if (g_verts_local && E.live) {
      const double2 t = *reinterpret_cast<const double2*>(g_verts_local + ((size_t)body * cap + e) * 2);
      gux = t.x; guy = t.y;
    }
  }
  // I = 1/6 m Num / Den, Num = sum w q, Den = sum w, w = |x(u_e+1, u_e)|: edge e gives P to vertex e and Q to vertex e + 1
  const double xu = E.live ? cross2(E.tx, E.ty, E.ux, E.uy) : 0.0;
  const double w = fabs(xu);
  const double q = E.ux * E.ux + E.uy * E.uy + (E.ux * E.tx + E.uy * E.ty) + (E.tx * E.tx + E.ty * E.ty);
  const double num = seg_sum<L>(w * q), den = seg_sum<L>(w);
  const double ratio = num / den;                                                     // (6 I / m)
  const double k6 = E.live ? gI * (1.0 / 6.0) * m / den : 0.0;
  const double a = k6 * (q - ratio) * (xu > 0.0 ? 1.0 : (xu < 0.0 ? -1.0 : 0.0));    // d|x| = sign(x) dx
  const double b = k6 * w;
  const double px = a * -E.ty + b * (2.0 * E.ux + E.tx), py = a * E.tx + b * (2.0 * E.uy + E.ty);
  const double qx = a * E.uy + b * (E.ux + 2.0 * E.tx), qy = a * -E.ux + b * (E.uy + 2.0 * E.ty);
  gux += px + __shfl(qx, E.prev, 64); guy += py + __shfl(qy, E.prev, 64);
  if (!E.live) { gux = 0.0; guy = 0.0; }
  // u = v - c: the centroid takes g_centroid - sum of the u gradients; c = N / (3 A), N = sum x (v_e + v_e+1), A = sum x
  const double hx = gcx - seg_sum<L>(gux), hy = gcy - seg_sum<L>(guy);
  const double i3a = 1.0 / (3.0 * E.A);
  const double kc = E.live ? (hx * (E.vx + E.wx - 3.0 * E.cx) + hy * (E.vy + E.wy - 3.0 * E.cy)) * i3a : 0.0;
  const double dir = E.live ? E.xv * i3a : 0.0;
  const double pcx = kc * -E.wy + dir * hx, pcy = kc * E.wx + dir * hy;
  const double qcx = kc * E.vy + dir * hx, qcy = kc * -E.vx + dir * hy;
  double gvx = gux + pcx + __shfl(qcx, E.prev, 64), gvy = guy + pcy + __shfl(qcy, E.prev, 64);
  if (!E.live) { gvx = 0.0; gvy = 0.0; }
  if (!in) return;
  if (g_verts_raw && e < cap) {
    double2 o; o.x = gvx; o.y = gvy;                                                  // (slots >= nv and circles: zeros)
    *reinterpret_cast<double2*>(g_verts_raw + ((size_t)body * cap + e) * 2) = o;
  }
  if (e != 0) return;
  const double r = radius[body];
  if (g_radius) g_radius[body] = E.hull ? 0.0 : gI * m * r;
  if (g_mass) {
    double gm = gI * (E.hull ? (1.0 / 6.0) * ratio : r * r / 2);                      // dI/dm = I / m
    if (g_Mdiag) gm += (double)g_Mdiag[body * 3 + 1] + (double)g_Mdiag[body * 3 + 2];
    if (g_f) gm += g * (double)g_f[body * 3 + 2];
    g_mass[body] = gm;
  }
}

static int lanes_per_body(int cap) { return cap <= 8 ? 8 : cap <= 16 ? 16 : cap <= 32 ? 32 : 64; }

}  // namespace bodies

int body_properties_launch(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                           const int32_t* nverts, const double* mass, double g, double* centroid, double* verts_local,
                           double* inertia, float* Mdiag, float* f_gravity, int32_t* status, void* stream) {
  const long long nbody = (long long)B * nb;
  const int L = bodies::lanes_per_body(cap);
  const long long blocks = (nbody * L + bodies::BD_T - 1) / bodies::BD_T;
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
#define LCP_BD_LAUNCH(LL)                                                                                                      \
  hipLaunchKernelGGL(bodies::lcp_body_properties_kernel<LL>, dim3((unsigned)blocks), dim3(bodies::BD_T), 0, (hipStream_t)stream, \
                     nbody, cap, kind, radius, verts_raw, nverts, mass, g, centroid, verts_local, inertia, Mdiag, f_gravity, status)
  switch (L) {
    case 8: LCP_BD_LAUNCH(8); break;
    case 16: LCP_BD_LAUNCH(16); break;
    case 32: LCP_BD_LAUNCH(32); break;
    default: LCP_BD_LAUNCH(64); break;
  }
#undef LCP_BD_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

int body_properties_backward_launch(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                                    const int32_t* nverts, const double* mass, double g, const double* g_centroid,
                                    const double* g_verts_local, const double* g_inertia, const float* g_Mdiag, const float* g_f,
                                    double* g_verts_raw, double* g_radius, double* g_mass, void* stream) {
  const long long nbody = (long long)B * nb;
  const int L = bodies::lanes_per_body(cap);
  const long long blocks = (nbody * L + bodies::BD_T - 1) / bodies::BD_T;
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
#define LCP_BD_LAUNCH(LL)                                                                                                     \
  hipLaunchKernelGGL(bodies::lcp_body_properties_backward_kernel<LL>, dim3((unsigned)blocks), dim3(bodies::BD_T), 0,          \
                     (hipStream_t)stream, nbody, cap, kind, radius, verts_raw, nverts, mass, g, g_centroid, g_verts_local,     \
                     g_inertia, g_Mdiag, g_f, g_verts_raw, g_radius, g_mass)
  switch (L) {
    case 8: LCP_BD_LAUNCH(8); break;
    case 16: LCP_BD_LAUNCH(16); break;
    case 32: LCP_BD_LAUNCH(32); break;
    default: LCP_BD_LAUNCH(64); break;
  }
#undef LCP_BD_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace lcp
