// lcp_forces.hip - force elements: springs / dampers, PD motors and viscous drag as a function of the state, and their backward.
//
// include/lcp_hip.h ("force elements") states the rule; evaluate() follows it line by line and gradients() is its derivative.
//
// Mapping.  A group of G lanes serves one scene, G the power of two >= max(nb, E), at most 256; a workgroup has max(64, G) threads
// and so holds 64 / G scenes where G < 64.  The common world has 3 to 12 bodies and a handful of elements: with a 256-thread workgroup
// per scene all but a few of its lanes would idle and 4096 scenes would be 16384 wavefronts; this way 4 bodies x 4 elements are 16
// scenes in one wavefront (256 wavefronts), 48 bodies x 256 elements one workgroup of 256 per scene, one element per lane.
//   phase 1, lane = element (stride G): the element's wrench on either body into LDS - the torque on body 1, the torque on body 2,
//            the force on body 1 (body 2 receives its negative) and the two bodies, 40 bytes an element, 40 KB at E = 1024
//   phase 2, lane = body: it walks the scene's staged elements IN ELEMENT ORDER and adds what is addressed to it, in fp64, onto
//            f_base; one rounding at the store.  A body's sum is one lane's, so one wavefront's: no atomics, the same bits every run.
//            The walk reads one LDS address per group (a broadcast).
// The backward has the same two phases in chunks of 512 elements (72 bytes an element: 36 KB): lane = element writes the element's
// own gradients (k, c, x0, w0, a1, a2) to memory and stages what the two bodies receive - because positions and velocities enter a
// spring only through P2 - P1 and V2 - V1, the translation parts of body 2 are minus body 1's and are staged once; lane = body adds
// them in element order over the chunks and writes g_p and g_v at the end.  Nothing is saved by the forward: every element is
// evaluated again.
#include <hip/hip_runtime.h>

#include "lcp_kernels.h"

namespace lcp {
namespace forces {

constexpr int MAXE = 1024, MAXB = 64;
constexpr int CHUNK = 512;                 // elements the backward stages at a time
constexpr int NOBODY = -2;                 // in a staged slot: nothing is addressed to a body (-1 is the world, which receives nothing either)
enum { KIND_SPRING = 1, KIND_MOTOR = 2, KIND_DRAG = 3 };

struct Elements {
  int E;
  const int32_t *kind, *b1, *b2;
  const double *a1, *a2, *k, *c, *x0, *w0, *limit;
};

// One end of an element: a body's anchor, or (body < 0) a point of the world at rest.
struct End {
  bool body;
  double sn, cs, w, rx, ry, Px, Py, Vx, Vy;
};

__device__ __forceinline__ End end_of(int b, double ax, double ay, const double* p, const float* v) {
  End e;
  e.body = b >= 0;
  e.sn = 0.0; e.cs = 1.0; e.w = 0.0; e.rx = e.ry = 0.0; e.Px = ax; e.Py = ay; e.Vx = e.Vy = 0.0;
  if (e.body) {
    sincos(p[3 * b], &e.sn, &e.cs);
    e.w = (double)v[3 * b];
    e.rx = e.cs * ax - e.sn * ay; e.ry = e.sn * ax + e.cs * ay;                          // utils.py:105-112
    e.Px = p[3 * b + 1] + e.rx; e.Py = p[3 * b + 2] + e.ry;
    e.Vx = (double)v[3 * b + 1] - e.w * e.ry; e.Vy = (double)v[3 * b + 2] + e.w * e.rx;   // V = v + w perp(r)
  }
  return e;
}

// What an element evaluates to.  kind 0: nothing (invalid, or a spring of length 0).  The wrench: torque t1 and force (fx, fy) on b1,
// torque t2 and force -(fx, fy) on b2.
struct Eval {
  int kind, b1, b2;
  bool sat;                                // the clamp is active: no gradient
  double t1, t2, fx, fy;
  double k, c, x0, w0;
  End e1, e2;                              // spring
  double L, ux, uy, Ldot, s;               // spring: length, direction, rate, the (clamped) tension
  double th, om;                           // motor
  double w, vx, vy;                        // drag: body 1's velocity
};

__device__ __forceinline__ Eval evaluate(const Elements& el, size_t i, int nb, const double* p, const float* v) {
  Eval R;
  R.kind = 0; R.b1 = R.b2 = NOBODY; R.sat = false; R.t1 = R.t2 = R.fx = R.fy = 0.0;
  const int kind = el.kind[i], b1 = el.b1[i], b2 = el.b2[i];
  R.k = el.k[i]; R.c = el.c[i]; R.x0 = el.x0[i]; R.w0 = el.w0[i];
  const double limit = el.limit[i];
  if (kind == KIND_DRAG) {
    if (b1 < 0 || b1 >= nb) return R;
    R.w = (double)v[3 * b1]; R.vx = (double)v[3 * b1 + 1]; R.vy = (double)v[3 * b1 + 2];
    R.kind = kind; R.b1 = b1;
    R.t1 = -R.c * R.w; R.fx = -R.k * R.vx; R.fy = -R.k * R.vy;
    return R;
  }
  if (kind != KIND_SPRING && kind != KIND_MOTOR) return R;
  if (b1 < -1 || b1 >= nb || b2 < -1 || b2 >= nb || b1 == b2) return R;                    // (b1 == b2 covers both ends the world)
  if (kind == KIND_MOTOR) {
    R.th = (b2 >= 0 ? p[3 * b2] : 0.0) - (b1 >= 0 ? p[3 * b1] : 0.0);
    R.om = (b2 >= 0 ? (double)v[3 * b2] : 0.0) - (b1 >= 0 ? (double)v[3 * b1] : 0.0);
    const double tau = R.k * (R.x0 - R.th) + R.c * (R.w0 - R.om);
    R.sat = fabs(tau) >= limit;
    const double t = R.sat ? copysign(limit, tau) : tau;
    R.kind = kind; R.b1 = b1; R.b2 = b2;
    R.t1 = -t; R.t2 = t;
    return R;
  }
  R.e1 = end_of(b1, el.a1[2 * i], el.a1[2 * i + 1], p, v);
  R.e2 = end_of(b2, el.a2[2 * i], el.a2[2 * i + 1], p, v);
  const double dx = R.e2.Px - R.e1.Px, dy = R.e2.Py - R.e1.Py;
  R.L = sqrt(dx * dx + dy * dy);
  if (!(R.L > 0.0)) return R;                                                              // L == 0: no force, no gradient
  R.ux = dx / R.L; R.uy = dy / R.L;
  R.Ldot = R.ux * (R.e2.Vx - R.e1.Vx) + R.uy * (R.e2.Vy - R.e1.Vy);
  const double s = R.k * (R.L - R.x0) + R.c * R.Ldot;
  R.sat = fabs(s) >= limit;
  R.s = R.sat ? copysign(limit, s) : s;
  R.kind = kind; R.b1 = b1; R.b2 = b2;
  R.fx = R.s * R.ux; R.fy = R.s * R.uy;
  R.t1 = R.e1.rx * R.fy - R.e1.ry * R.fx;                                                  // cross(r1, s u)
  R.t2 = -(R.e2.rx * R.fy - R.e2.ry * R.fx);                                               // cross(r2, -s u)
  return R;
}

// The gradients of one element: its own parameters, and what its two bodies receive - body 1 (rot1, -x, -y) of the pose and
// (w1, -vx, -vy) of the velocity, body 2 (rot2, x, y) and (w2, vx, vy).  b1 / b2: the bodies that receive anything (else NOBODY).
struct Grad {
  int b1, b2;
  double k, c, x0, w0, a1x, a1y, a2x, a2y;
  double rot1, rot2, x, y, w1, w2, vx, vy;
};

// g_f of a body as (torque, fx, fy); the world has none
__device__ __forceinline__ void cotangent(int b, const float* g_f, double& t, double& x, double& y) {
  t = x = y = 0.0;
  if (b >= 0) { t = (double)g_f[3 * b]; x = (double)g_f[3 * b + 1]; y = (double)g_f[3 * b + 2]; }
}

__device__ __forceinline__ Grad gradients(const Eval& R, const float* g_f) {
  Grad D;
  D.b1 = D.b2 = NOBODY;
  D.k = D.c = D.x0 = D.w0 = D.a1x = D.a1y = D.a2x = D.a2y = 0.0;
  D.rot1 = D.rot2 = D.x = D.y = D.w1 = D.w2 = D.vx = D.vy = 0.0;
  if (R.kind == 0 || R.sat) return D;
  double gt1, g1x, g1y, gt2, g2x, g2y;
  cotangent(R.b1, g_f, gt1, g1x, g1y);
  cotangent(R.b2, g_f, gt2, g2x, g2y);
  D.b1 = R.b1 >= 0 ? R.b1 : NOBODY;
  D.b2 = R.b2 >= 0 ? R.b2 : NOBODY;
  if (R.kind == KIND_DRAG) {                                                               // (-c w, -k vx, -k vy) on b1
    D.c = -gt1 * R.w;
    D.k = -(g1x * R.vx + g1y * R.vy);
    D.w1 = -R.c * gt1;
    D.vx = R.k * g1x; D.vy = R.k * g1y;                                                    // (body 1 receives the negative)
    return D;
  }
  if (R.kind == KIND_MOTOR) {                                                              // tau = k (x0 - th) + c (w0 - om), +tau on b2
    const double q = gt2 - gt1;
    D.k = q * (R.x0 - R.th); D.x0 = q * R.k;
    D.c = q * (R.w0 - R.om); D.w0 = q * R.c;
    D.rot2 = -q * R.k; D.rot1 = q * R.k;
    D.w2 = -q * R.c; D.w1 = q * R.c;
    return D;
  }
  // spring: the loss sees F . q with F = s u and q = g1 - g2 + gt1 perp(r1) - gt2 perp(r2)
  const End &e1 = R.e1, &e2 = R.e2;
  const double qx = (g1x - g2x) - gt1 * e1.ry + gt2 * e2.ry, qy = (g1y - g2y) + gt1 * e1.rx - gt2 * e2.rx;
  const double qu = qx * R.ux + qy * R.uy;
  const double Vrx = e2.Vx - e1.Vx, Vry = e2.Vy - e1.Vy;
  const double iL = 1.0 / R.L;
  D.k = qu * (R.L - R.x0); D.x0 = -qu * R.k; D.c = qu * R.Ldot;
  // d = P2 - P1 and Vr = V2 - V1
  const double gdx = qu * R.k * R.ux + (qu * R.c * (Vrx - R.ux * R.Ldot) + R.s * (qx - R.ux * qu)) * iL;
  const double gdy = qu * R.k * R.uy + (qu * R.c * (Vry - R.uy * R.Ldot) + R.s * (qy - R.uy * qu)) * iL;
  const double gvx = qu * R.c * R.ux, gvy = qu * R.c * R.uy;
  D.x = gdx; D.y = gdy; D.vx = gvx; D.vy = gvy;
  const double Fx = R.s * R.ux, Fy = R.s * R.uy;
  if (e2.body) {
    // r2 through P2, through V2 = v2 + w2 perp(r2) and through the torque cross(r2, -F)
    const double grx = gdx + e2.w * gvy - gt2 * Fy, gry = gdy - e2.w * gvx + gt2 * Fx;
    D.rot2 = gry * e2.rx - grx * e2.ry;                                                    // dr/drot = perp(r)
    D.w2 = gvy * e2.rx - gvx * e2.ry;
    D.a2x = e2.cs * grx + e2.sn * gry; D.a2y = -e2.sn * grx + e2.cs * gry;                 // R(rot)^T
  } else {
    D.a2x = gdx; D.a2y = gdy;
  }
  if (e1.body) {
    const double grx = -gdx - e1.w * gvy + gt1 * Fy, gry = -gdy + e1.w * gvx - gt1 * Fx;
    D.rot1 = gry * e1.rx - grx * e1.ry;
    D.w1 = -(gvy * e1.rx - gvx * e1.ry);
    D.a1x = e1.cs * grx + e1.sn * gry; D.a1y = -e1.sn * grx + e1.cs * gry;
  } else {
    D.a1x = -gdx; D.a1y = -gdy;
  }
  return D;
}

// `shift`: log2 of the lanes a scene has (G); the workgroup holds blockDim.x >> shift scenes
__global__ void __launch_bounds__(256) lcp_force_elements_kernel(int B, int nb, int shift, Elements el, const double* p, const float* v,
                                                                 const float* f_base, float* f_out) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int E = el.E, G = 1 << shift;
  const int slots = ((int)blockDim.x >> shift) * E;
  double *s_t1 = s_dyn, *s_t2 = s_t1 + slots, *s_fx = s_t2 + slots, *s_fy = s_fx + slots;
  int *s_b1 = reinterpret_cast<int*>(s_fy + slots), *s_b2 = s_b1 + slots;
  const int sub = (int)threadIdx.x >> shift, gl = (int)threadIdx.x & (G - 1);
  const long long scene = (long long)blockIdx.x * ((int)blockDim.x >> shift) + sub;
  const bool ok = scene < B;
  const double* ps = p + (ok ? (size_t)scene * nb * 3 : 0);
  const float* vs = v + (ok ? (size_t)scene * nb * 3 : 0);
  if (ok) {
    for (int e = gl; e < E; e += G) {
      const Eval R = evaluate(el, (size_t)scene * E + e, nb, ps, vs);
      const int j = sub * E + e;
      s_t1[j] = R.t1; s_t2[j] = R.t2; s_fx[j] = R.fx; s_fy[j] = R.fy;
      s_b1[j] = R.b1; s_b2[j] = R.b2;
    }
  }
  __syncthreads();
  if (!ok || gl >= nb) return;
  const int b = gl;
  const size_t o = ((size_t)scene * nb + b) * 3;
  float base[3] = {0.0f, 0.0f, 0.0f};
  if (f_base) { base[0] = f_base[o]; base[1] = f_base[o + 1]; base[2] = f_base[o + 2]; }    // (read before the store: f_out may be f_base)
  double st = (double)base[0], sx = (double)base[1], sy = (double)base[2];
  bool touched = false;
  for (int e = 0; e < E; ++e) {
    const int j = sub * E + e;
    if (s_b1[j] == b) { st += s_t1[j]; sx += s_fx[j]; sy += s_fy[j]; touched = true; }
    if (s_b2[j] == b) { st += s_t2[j]; sx -= s_fx[j]; sy -= s_fy[j]; touched = true; }
  }
  // a body no element touches: f_base's bits
  f_out[o] = touched ? (float)st : base[0];
  f_out[o + 1] = touched ? (float)sx : base[1];
  f_out[o + 2] = touched ? (float)sy : base[2];
}

__global__ void __launch_bounds__(256) lcp_force_elements_backward_kernel(int B, int nb, int shift, int chunk, Elements el,
                                                                          const double* p, const float* v, const float* g_f, double* g_p,
                                                                          double* g_v, double* g_k, double* g_c, double* g_x0,
                                                                          double* g_w0, double* g_a1, double* g_a2) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int E = el.E, G = 1 << shift;
  const int slots = ((int)blockDim.x >> shift) * chunk;
  double *s_rot1 = s_dyn, *s_rot2 = s_rot1 + slots, *s_x = s_rot2 + slots, *s_y = s_x + slots;
  double *s_w1 = s_y + slots, *s_w2 = s_w1 + slots, *s_vx = s_w2 + slots, *s_vy = s_vx + slots;
  int *s_b1 = reinterpret_cast<int*>(s_vy + slots), *s_b2 = s_b1 + slots;
  const int sub = (int)threadIdx.x >> shift, gl = (int)threadIdx.x & (G - 1);
  const long long scene = (long long)blockIdx.x * ((int)blockDim.x >> shift) + sub;
  const bool ok = scene < B;
  const size_t so = ok ? (size_t)scene * nb * 3 : 0;
  const double* ps = p + so;
  const float *vs = v + so, *gs = g_f + so;
  const int b = gl;
  double arot = 0.0, ax = 0.0, ay = 0.0, aw = 0.0, avx = 0.0, avy = 0.0;                   // body b's sums
  for (int e0 = 0; e0 < E; e0 += chunk) {
    const int n = min(chunk, E - e0);
    if (ok) {
      for (int jj = gl; jj < n; jj += G) {
        const size_t i = (size_t)scene * E + e0 + jj;
        const Grad D = gradients(evaluate(el, i, nb, ps, vs), gs);
        if (g_k) g_k[i] = D.k;
        if (g_c) g_c[i] = D.c;
        if (g_x0) g_x0[i] = D.x0;
        if (g_w0) g_w0[i] = D.w0;
        if (g_a1) { g_a1[2 * i] = D.a1x; g_a1[2 * i + 1] = D.a1y; }
        if (g_a2) { g_a2[2 * i] = D.a2x; g_a2[2 * i + 1] = D.a2y; }
        const int j = sub * chunk + jj;
        s_rot1[j] = D.rot1; s_rot2[j] = D.rot2; s_x[j] = D.x; s_y[j] = D.y;
        s_w1[j] = D.w1; s_w2[j] = D.w2; s_vx[j] = D.vx; s_vy[j] = D.vy;
        s_b1[j] = D.b1; s_b2[j] = D.b2;
      }
    }
    __syncthreads();
    if (ok && b < nb) {
      for (int jj = 0; jj < n; ++jj) {
        const int j = sub * chunk + jj;
        if (s_b1[j] == b) { arot += s_rot1[j]; ax -= s_x[j]; ay -= s_y[j]; aw += s_w1[j]; avx -= s_vx[j]; avy -= s_vy[j]; }
        if (s_b2[j] == b) { arot += s_rot2[j]; ax += s_x[j]; ay += s_y[j]; aw += s_w2[j]; avx += s_vx[j]; avy += s_vy[j]; }
      }
    }
    __syncthreads();                                                                       // (the next chunk overwrites the slots)
  }
  if (!ok || b >= nb) return;
  const size_t o = so + (size_t)b * 3;
  if (g_p) { g_p[o] = arot; g_p[o + 1] = ax; g_p[o + 2] = ay; }
  if (g_v) { g_v[o] = aw; g_v[o + 1] = avx; g_v[o + 2] = avy; }
}

// lanes per scene as a shift: the power of two >= max(nb, E), at most 256
static int group_shift(int nb, int E) {
  int shift = 0;
  while ((1 << shift) < (nb > E ? nb : E) && shift < 8) ++shift;
  return shift;
}

static int launch(const void* fn, int B, int shift, size_t lds_per_scene, void* stream, void** args) {
  const int threads = (1 << shift) < 64 ? 64 : (1 << shift);
  const int scenes = threads >> shift;
  const long long blocks = ((long long)B + scenes - 1) / scenes;
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
  const size_t lds = lds_per_scene * scenes;                                               // (at most 40 KB: no opt-in)
  if (hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(threads), args, lds, (hipStream_t)stream) != hipSuccess) return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace forces

bool force_elements_supported(int nb, int E) { return nb >= 1 && nb <= forces::MAXB && E >= 1 && E <= forces::MAXE; }

int force_elements_launch(int B, int nb, int E, const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1,
                          const double* a2, const double* k, const double* c, const double* x0, const double* w0, const double* limit,
                          const double* p, const float* v, const float* f_base, float* f_out, void* stream) {
  using namespace forces;
  if (!force_elements_supported(nb, E)) return LCP_E_TOOLARGE;
  Elements el{E, kind, b1, b2, a1, a2, k, c, x0, w0, limit};
  int shift = group_shift(nb, E);
  void* args[] = {&B, &nb, &shift, &el, &p, &v, &f_base, &f_out};
  return launch(reinterpret_cast<const void*>(lcp_force_elements_kernel), B, shift, (size_t)E * (4 * sizeof(double) + 2 * sizeof(int)),
                stream, args);
}

int force_elements_backward_launch(int B, int nb, int E, const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1,
                                   const double* a2, const double* k, const double* c, const double* x0, const double* w0,
                                   const double* limit, const double* p, const float* v, const float* g_f, double* g_p, double* g_v,
                                   double* g_k, double* g_c, double* g_x0, double* g_w0, double* g_a1, double* g_a2, void* stream) {
  using namespace forces;
  if (!force_elements_supported(nb, E)) return LCP_E_TOOLARGE;
  Elements el{E, kind, b1, b2, a1, a2, k, c, x0, w0, limit};
  int shift = group_shift(nb, E);
  int chunk = E < CHUNK ? E : CHUNK;
  void* args[] = {&B, &nb, &shift, &chunk, &el, &p, &v, &g_f, &g_p, &g_v, &g_k, &g_c, &g_x0, &g_w0, &g_a1, &g_a2};
  return launch(reinterpret_cast<const void*>(lcp_force_elements_backward_kernel), B, shift,
                (size_t)chunk * (8 * sizeof(double) + 2 * sizeof(int)), stream, args);
}

}  // namespace lcp
