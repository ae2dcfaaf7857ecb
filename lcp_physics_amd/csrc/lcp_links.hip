// lcp_links.hip - mechanism links: the equality rows of rods, slots and sliders as a function of the pose, and their backward.
//
// include/lcp_hip.h ("mechanism links") states the rule; evaluate() follows it line by line and gradients() is its derivative.
//
// Mapping (that of lcp_forces.hip).  A group of G lanes serves one scene, G the power of two >= max(nb, L), at most 256; a workgroup has
// max(64, G) threads and so holds 64 / G scenes where G < 64: 4 bodies x 4 links are 16 scenes in one wavefront, 48 bodies x 64 links
// one wavefront per scene.
//   forward   phase 0, lane = link: the rows the link's kind has, into LDS (a link's first row is the sum over the links before it)
//             phase 1, lane = link: the link's (at most six) entries and the two columns they start at, staged per ROW in LDS, 32 bytes
//                      a row; a row no link fills keeps the columns -1
//             phase 2, the scenes of a workgroup are ONE contiguous range of Je: its threads walk that range with consecutive addresses
//                      (whole-line stores whatever G is), a base row copied from Je_base, a link row zero but for the staged entries.
//                      Every element of Je is written once, by one thread: nothing orders a zero fill against the entries.
//   backward  phase 0 as above; phase 1, lane = link: the link's own gradients (a1, a2, phi) to memory, what its two bodies receive
//             into LDS (40 bytes a link: the translation part of the second body is minus the first's, a link sees the positions only
//             through their difference); phase 2, lane = body: it walks the staged links IN LINK ORDER and adds what is addressed to it.
//             A body's sum is one lane's: no atomics, the same bits every run; a body no link names keeps exact zeros.
// The kind switch is per lane: evaluate() shares the anchors' turn between the kinds and each arm is a dozen lines.
#include <hip/hip_runtime.h>

#include "lcp_kernels.h"

namespace lcp {
namespace links {

constexpr int MAXL = 256, MAXB = 64, MAXE0 = 65536;
constexpr int NOBODY = -2;                 // in a staged slot: nothing is addressed to a body (-1 is the world, which receives nothing either)
constexpr double COINCIDENT = 1e-12;       // a rod between anchors closer than this has no direction: a row of zeros
enum { KIND_DISTANCE = 1, KIND_SLOT = 2, KIND_PRISMATIC = 3 };

struct Links {
  int L;
  const int32_t *kind, *first, *second;
  const double *a1, *a2, *phi;
};

__device__ __forceinline__ int rows_of(int kind) {
  return kind == KIND_PRISMATIC ? 2 : (kind == KIND_DISTANCE || kind == KIND_SLOT) ? 1 : 0;
}

// What a link evaluates to.  kind 0: its rows are zero (an index out of range, first == second, a rod without a direction).
// (dx, dy): the rod's w_2 - w_1; the slot's r_2 + d = w_1 - c_2 (second a body; unused for the world).  (nx, ny): the rod's n, the slot's t.
struct Eval {
  int kind, b1, b2;
  double sn1, cs1, sn2, cs2, r1x, r1y, r2x, r2y;
  double dx, dy, len, nx, ny;
};

__device__ __forceinline__ Eval evaluate(const Links& ln, size_t i, int nb, const double* p) {
  Eval R;
  R.kind = 0; R.b1 = R.b2 = NOBODY;
  R.sn1 = R.sn2 = 0.0; R.cs1 = R.cs2 = 1.0; R.r1x = R.r1y = R.r2x = R.r2y = 0.0;
  R.dx = R.dy = R.nx = R.ny = 0.0; R.len = 1.0;
  const int kind = ln.kind[i], b1 = ln.first[i], b2 = ln.second[i];
  if (rows_of(kind) == 0) return R;
  if (b1 < 0 || b1 >= nb || b2 < -1 || b2 >= nb || b1 == b2) return R;
  const double a1x = ln.a1[2 * i], a1y = ln.a1[2 * i + 1], a2x = ln.a2[2 * i], a2y = ln.a2[2 * i + 1];
  sincos(p[3 * b1], &R.sn1, &R.cs1);
  R.r1x = R.cs1 * a1x - R.sn1 * a1y; R.r1y = R.sn1 * a1x + R.cs1 * a1y;
  const double w1x = p[3 * b1 + 1] + R.r1x, w1y = p[3 * b1 + 2] + R.r1y;
  double c2x = 0.0, c2y = 0.0, w2x = a2x, w2y = a2y;                                      // the world: w_2 = a_2, rotation 0
  if (b2 >= 0) {
    sincos(p[3 * b2], &R.sn2, &R.cs2);
    R.r2x = R.cs2 * a2x - R.sn2 * a2y; R.r2y = R.sn2 * a2x + R.cs2 * a2y;
    c2x = p[3 * b2 + 1]; c2y = p[3 * b2 + 2];
    w2x = c2x + R.r2x; w2y = c2y + R.r2y;
  }
  if (kind == KIND_DISTANCE) {
    R.dx = w2x - w1x; R.dy = w2y - w1y;
    R.len = sqrt(R.dx * R.dx + R.dy * R.dy);
    if (!(R.len >= COINCIDENT)) return R;                                                  // (a NaN too)
    R.nx = R.dx / R.len; R.ny = R.dy / R.len;
  } else {
    double sp, cp;
    sincos(ln.phi[i], &sp, &cp);
    R.nx = -(R.cs2 * sp + R.sn2 * cp); R.ny = -R.sn2 * sp + R.cs2 * cp;                    // t = R(rot_2) (-sin phi, cos phi)
    R.dx = w1x - c2x; R.dy = w1y - c2y;
  }
  R.kind = kind; R.b1 = b1; R.b2 = b2;
  return R;
}

// The link's first row: three entries from column 3 b1, three from column 3 b2.
__device__ __forceinline__ void entries(const Eval& R, double* e) {
  const double nx = R.nx, ny = R.ny;
  if (R.kind == KIND_DISTANCE) {
    e[0] = -(R.r1x * ny - R.r1y * nx); e[1] = -nx; e[2] = -ny;
    e[3] = R.r2x * ny - R.r2y * nx; e[4] = nx; e[5] = ny;
  } else {
    e[0] = R.r1x * ny - R.r1y * nx; e[1] = nx; e[2] = ny;
    e[3] = -(R.dx * ny - R.dy * nx); e[4] = -nx; e[5] = -ny;
  }
}

// The gradients of one link: its own parameters, and what its two bodies receive - body 1 (rot1, x, y), body 2 (rot2, -x, -y).
struct Grad {
  int b1, b2;
  double a1x, a1y, a2x, a2y, phi;
  double rot1, rot2, x, y;
};

// `g`: the cotangent of the link's first row (nz floats)
__device__ __forceinline__ Grad gradients(const Eval& R, const float* g) {
  Grad D;
  D.b1 = D.b2 = NOBODY;
  D.a1x = D.a1y = D.a2x = D.a2y = D.phi = D.rot1 = D.rot2 = D.x = D.y = 0.0;
  if (R.kind == 0) return D;
  const bool body2 = R.b2 >= 0;
  const double g1r = (double)g[3 * R.b1], g1x = (double)g[3 * R.b1 + 1], g1y = (double)g[3 * R.b1 + 2];
  const double g2r = body2 ? (double)g[3 * R.b2] : 0.0, g2x = body2 ? (double)g[3 * R.b2 + 1] : 0.0,
               g2y = body2 ? (double)g[3 * R.b2 + 2] : 0.0;
  D.b1 = R.b1; D.b2 = body2 ? R.b2 : NOBODY;
  const double nx = R.nx, ny = R.ny;
  double gr1x, gr1y, gr2x = 0.0, gr2y = 0.0;                                               // what reaches the arms r_1, r_2
  if (R.kind == KIND_DISTANCE) {
    // the row is (-cross(r1, n), -n | cross(r2, n), n): through n = d / |d|, d = w2 - w1, and through the arms
    const double gnx = (g2x - g1x) + g1r * R.r1y - g2r * R.r2y, gny = (g2y - g1y) - g1r * R.r1x + g2r * R.r2x;
    const double dot = nx * gnx + ny * gny;
    const double gdx = (gnx - nx * dot) / R.len, gdy = (gny - ny * dot) / R.len;
    D.x = -gdx; D.y = -gdy;
    gr1x = -g1r * ny - gdx; gr1y = g1r * nx - gdy;
    gr2x = g2r * ny + gdx; gr2y = -g2r * nx + gdy;
    if (!body2) { D.a2x = gdx; D.a2y = gdy; }                                              // the world point itself
  } else {
    // the row is (cross(r1, t), t | -cross(u, t), -t) with u = r2 + d = w1 - c2: a2 does not enter it
    const double gtx = -g1r * R.r1y + (g1x - g2x) + g2r * R.dy, gty = g1r * R.r1x + (g1y - g2y) - g2r * R.dx;
    const double gux = -g2r * ny, guy = g2r * nx;
    D.x = gux; D.y = guy;
    gr1x = g1r * ny + gux; gr1y = -g1r * nx + guy;
    const double gth = -gtx * ny + gty * nx;                                               // dt / d(rot2 + phi) = perp(t)
    D.phi = gth;
    if (body2) D.rot2 = gth;
  }
  D.rot1 = gr1y * R.r1x - gr1x * R.r1y;                                                    // dr / drot = perp(r)
  D.a1x = R.cs1 * gr1x + R.sn1 * gr1y; D.a1y = -R.sn1 * gr1x + R.cs1 * gr1y;               // R(rot)^T
  if (body2 && R.kind == KIND_DISTANCE) {
    D.rot2 = gr2y * R.r2x - gr2x * R.r2y;
    D.a2x = R.cs2 * gr2x + R.sn2 * gr2y; D.a2y = -R.sn2 * gr2x + R.cs2 * gr2y;
  }
  return D;
}

// the first row of link l of the group's scene (the rows of the links before it), from the staged row counts
__device__ __forceinline__ int first_row(const int* s_rows, int l) {
  int off = 0;
  for (int q = 0; q < l; ++q) off += s_rows[q];
  return off;
}

// `shift`: log2 of the lanes a scene has (G); the workgroup holds blockDim.x >> shift scenes
__global__ void __launch_bounds__(256) lcp_link_jacobian_kernel(int B, int nb, int shift, int e0, int el, Links ln, const double* p,
                                                                const float* Je_base, float* Je) {
  extern __shared__ __attribute__((aligned(16))) float s_dynf[];
  const int L = ln.L, G = 1 << shift, S = (int)blockDim.x >> shift;
  float* s_val = s_dynf;                                                                   // [S el][6]
  int* s_col = reinterpret_cast<int*>(s_val + (size_t)S * el * 6);                         // [S el][2]
  int* s_rows = s_col + (size_t)S * el * 2;                                                // [S L]
  const int sub = (int)threadIdx.x >> shift, gl = (int)threadIdx.x & (G - 1);
  const long long scene0 = (long long)blockIdx.x * S;
  const long long scene = scene0 + sub;
  const bool ok = scene < B;
  if (ok)
    for (int l = gl; l < L; l += G) s_rows[sub * L + l] = rows_of(ln.kind[(size_t)scene * L + l]);
  for (int r = gl; r < el; r += G) { s_col[2 * (sub * el + r)] = -1; s_col[2 * (sub * el + r) + 1] = -1; }
  __syncthreads();
  if (ok) {
    const double* ps = p + (size_t)scene * nb * 3;
    for (int l = gl; l < L; l += G) {
      const int n = s_rows[sub * L + l], off = first_row(s_rows + sub * L, l);
      if (n == 0 || off + n > el) continue;                                                // (a scene with more rows than `el`: dropped)
      const Eval R = evaluate(ln, (size_t)scene * L + l, nb, ps);
      if (R.kind == 0) continue;
      double e[6];
      entries(R, e);
      int j = sub * el + off;
      const int c1 = 3 * R.b1, c2 = R.b2 >= 0 ? 3 * R.b2 : -1;
      s_col[2 * j] = c1; s_col[2 * j + 1] = c2;
      for (int q = 0; q < 6; ++q) s_val[6 * j + q] = (float)e[q];
      if (n == 2) {                                                                        // rot_1 - rot_2
        ++j;
        s_col[2 * j] = c1; s_col[2 * j + 1] = c2;
        s_val[6 * j] = 1.0f; s_val[6 * j + 1] = 0.0f; s_val[6 * j + 2] = 0.0f;
        s_val[6 * j + 3] = -1.0f; s_val[6 * j + 4] = 0.0f; s_val[6 * j + 5] = 0.0f;
      }
    }
  }
  __syncthreads();
  // the workgroup's scenes are one contiguous range of Je: thread t owns elements t, t + blockDim, ... of it, as (scene, row, column)
  const unsigned nz = 3u * (unsigned)nb, rows = (unsigned)(e0 + el);
  const unsigned ns = (unsigned)((long long)B - scene0 < S ? (long long)B - scene0 : S);
  const unsigned per = rows * nz, total = ns * per, stride = blockDim.x;
  const unsigned dcol = stride % nz, drow = (stride / nz) % rows, dscene = (stride / nz) / rows;
  unsigned s = threadIdx.x / per, w = threadIdx.x % per;
  unsigned r = w / nz, c = w % nz;
  float* out = Je + (size_t)scene0 * per;
  const float* base = Je_base ? Je_base + (size_t)scene0 * e0 * nz : nullptr;
  for (unsigned i = threadIdx.x; i < total; i += stride) {
    float val = 0.0f;
    if (r < (unsigned)e0) {
      val = base[((size_t)s * e0 + r) * nz + c];
    } else {
      const int j = (int)s * el + (int)(r - (unsigned)e0), c1 = s_col[2 * j], c2 = s_col[2 * j + 1];
      if (c1 >= 0 && c - (unsigned)c1 < 3u) val = s_val[6 * j + (int)(c - (unsigned)c1)];
      else if (c2 >= 0 && c - (unsigned)c2 < 3u) val = s_val[6 * j + 3 + (int)(c - (unsigned)c2)];
    }
    out[i] = val;
    c += dcol; r += drow; s += dscene;
    if (c >= nz) { c -= nz; ++r; }
    if (r >= rows) { r -= rows; ++s; }
  }
}

__global__ void __launch_bounds__(256) lcp_link_jacobian_backward_kernel(int B, int nb, int shift, int e0, int el, Links ln,
                                                                         const double* p, const float* gJe, double* g_p, double* g_a1,
                                                                         double* g_a2, double* g_phi) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int L = ln.L, G = 1 << shift;
  const int slots = ((int)blockDim.x >> shift) * L;
  double *s_rot1 = s_dyn, *s_rot2 = s_rot1 + slots, *s_x = s_rot2 + slots, *s_y = s_x + slots;
  int *s_b1 = reinterpret_cast<int*>(s_y + slots), *s_b2 = s_b1 + slots, *s_rows = s_b2 + slots;
  const int sub = (int)threadIdx.x >> shift, gl = (int)threadIdx.x & (G - 1);
  const long long scene = (long long)blockIdx.x * ((int)blockDim.x >> shift) + sub;
  const bool ok = scene < B;
  if (ok)
    for (int l = gl; l < L; l += G) s_rows[sub * L + l] = rows_of(ln.kind[(size_t)scene * L + l]);
  __syncthreads();
  const int nz = 3 * nb;
  if (ok) {
    const double* ps = p + (size_t)scene * nb * 3;
    const float* gs = gJe + ((size_t)scene * (e0 + el) + e0) * nz;                         // the cotangent of the scene's link rows
    for (int l = gl; l < L; l += G) {
      const size_t i = (size_t)scene * L + l;
      const int n = s_rows[sub * L + l], off = first_row(s_rows + sub * L, l);
      Eval R;
      R.kind = 0;
      if (n != 0 && off + n <= el) R = evaluate(ln, i, nb, ps);
      Grad D;
      if (R.kind != 0) {
        D = gradients(R, gs + (size_t)off * nz);
      } else {
        D.b1 = D.b2 = NOBODY;
        D.a1x = D.a1y = D.a2x = D.a2y = D.phi = D.rot1 = D.rot2 = D.x = D.y = 0.0;
      }
      if (g_a1) { g_a1[2 * i] = D.a1x; g_a1[2 * i + 1] = D.a1y; }
      if (g_a2) { g_a2[2 * i] = D.a2x; g_a2[2 * i + 1] = D.a2y; }
      if (g_phi) g_phi[i] = D.phi;
      const int j = sub * L + l;
      s_rot1[j] = D.rot1; s_rot2[j] = D.rot2; s_x[j] = D.x; s_y[j] = D.y;
      s_b1[j] = D.b1; s_b2[j] = D.b2;
    }
  }
  __syncthreads();
  if (!ok || gl >= nb || !g_p) return;
  const int b = gl;
  double arot = 0.0, ax = 0.0, ay = 0.0;
  for (int l = 0; l < L; ++l) {
    const int j = sub * L + l;
    if (s_b1[j] == b) { arot += s_rot1[j]; ax += s_x[j]; ay += s_y[j]; }
    if (s_b2[j] == b) { arot += s_rot2[j]; ax -= s_x[j]; ay -= s_y[j]; }
  }
  const size_t o = ((size_t)scene * nb + b) * 3;
  g_p[o] = arot; g_p[o + 1] = ax; g_p[o + 2] = ay;
}

// lanes per scene as a shift: the power of two >= max(nb, L), at most 256
static int group_shift(int nb, int L) {
  int shift = 0;
  while ((1 << shift) < (nb > L ? nb : L) && shift < 8) ++shift;
  return shift;
}

static int launch(const void* fn, int B, int shift, size_t lds_per_scene, void* stream, void** args) {
  const int threads = (1 << shift) < 64 ? 64 : (1 << shift);
  const int scenes = threads >> shift;
  const long long blocks = ((long long)B + scenes - 1) / scenes;
  if (blocks > 0x7fffffffLL) return LCP_E_TOOLARGE;
  const size_t lds = lds_per_scene * scenes;                                               // (at most 17 KB: no opt-in)
  if (hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(threads), args, lds, (hipStream_t)stream) != hipSuccess) return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace links

bool link_jacobian_supported(int nb, int L, int e0) {
  return nb >= 1 && nb <= links::MAXB && L >= 1 && L <= links::MAXL && e0 >= 0 && e0 <= links::MAXE0;
}

int link_jacobian_launch(int B, int nb, int L, int e0, int el, const int32_t* kind, const int32_t* first, const int32_t* second,
                         const double* a1, const double* a2, const double* phi, const double* p, const float* Je_base, float* Je,
                         void* stream) {
  using namespace links;
  if (!link_jacobian_supported(nb, L, e0) || el < 0 || el > 2 * L) return LCP_E_TOOLARGE;
  Links ln{L, kind, first, second, a1, a2, phi};
  int shift = group_shift(nb, L);
  void* args[] = {&B, &nb, &shift, &e0, &el, &ln, &p, &Je_base, &Je};
  return launch(reinterpret_cast<const void*>(lcp_link_jacobian_kernel), B, shift,
                (size_t)el * (6 * sizeof(float) + 2 * sizeof(int)) + (size_t)L * sizeof(int), stream, args);
}

int link_jacobian_backward_launch(int B, int nb, int L, int e0, int el, const int32_t* kind, const int32_t* first, const int32_t* second,
                                  const double* a1, const double* a2, const double* phi, const double* p, const float* gJe, double* g_p,
                                  double* g_a1, double* g_a2, double* g_phi, void* stream) {
  using namespace links;
  if (!link_jacobian_supported(nb, L, e0) || el < 0 || el > 2 * L) return LCP_E_TOOLARGE;
  Links ln{L, kind, first, second, a1, a2, phi};
  int shift = group_shift(nb, L);
  void* args[] = {&B, &nb, &shift, &e0, &el, &ln, &p, &gJe, &g_p, &g_a1, &g_a2, &g_phi};
  return launch(reinterpret_cast<const void*>(lcp_link_jacobian_backward_kernel), B, shift,
                (size_t)L * (4 * sizeof(double) + 3 * sizeof(int)), stream, args);
}

}  // namespace lcp
