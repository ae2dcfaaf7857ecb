// lcp_substep.hip - the bookkeeping around one sub-step of World.step(fixed_dt=True) for B scenes.
//
//   reference (physics/world.py)                                                here
//   :72-80  step(fixed_dt=True): end_t = t + dt; while t < end_t:              lcp_substep_begin_kernel  (dt_k, active)
//           step_dt(end_t - t)
//   engines.py:31-32  u = M v + dt_k f(t)                                       lcp_substep_begin_kernel  (f_eff = (float)dt_k * f)
//   :87     set_v(new_v) - only for a scene that is still stepping             lcp_substep_commit_kernel
//
// The scenes of a batch need different numbers of sub-steps (the penetration test of step_dt halves dt per scene), so every
// sub-step runs the whole batch and a scene that has reached its end_t is masked: dt_k = 0 (the detection kernels leave such
// a scene where it is), contact count 0 (the solve takes its no-contact branch) and its velocities are put back afterwards.
// The solve kernels form u = md * v + dt * f in fp32 with contraction off (lcp_device.h momentum_entry): with dt = 1 and
// f_eff = fl((float)dt_k * f) that is bit for bit md * v + (float)dt_k * f, so they need no per-scene dt of their own.
// Element-wise, no atomics, nothing data dependent in the launch: capturable into a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_kernels.h"

namespace lcp {
namespace sub {

constexpr int T = 256;

// one thread per entry of f[B, nb, 3]; the thread of a scene's first entry also writes the scene's dt_k, active and count_eff
__global__ void __launch_bounds__(T) lcp_substep_begin_kernel(int B, int per, const double* t, const double* end_t, const float* f,
                                                              const int32_t* count, double* dt_k, int32_t* active, int32_t* count_eff,
                                                              float* f_eff) {
  const size_t i = (size_t)blockIdx.x * T + threadIdx.x;
  if (i >= (size_t)B * per) return;
  const int scene = (int)(i / per);
  const double tk = t[scene], te = end_t[scene];
  const bool on = tk < te;                                    // world.py:76 `while self.t < end_t`
  const double d = on ? te - tk : 0.0;                        // world.py:77 exactly this subtraction, in fp64
  f_eff[i] = (float)d * f[i];                                 // one fp32 product
  if (i == (size_t)scene * per) {
    dt_k[scene] = d;
    active[scene] = on ? 1 : 0;
    count_eff[scene] = on ? count[scene] : 0;
  }
}

// v_new = active ? v_new : v_old, in place: one thread per entry of v[B, nb, 3]
__global__ void __launch_bounds__(T) lcp_substep_commit_kernel(int B, int per, const int32_t* active, const float* v_old, float* v_new) {
  const size_t i = (size_t)blockIdx.x * T + threadIdx.x;
  if (i >= (size_t)B * per) return;
  if (!active[i / per]) v_new[i] = v_old[i];
}

}  // namespace sub

int substep_begin_launch(int B, int nb, const double* t, const double* end_t, const float* f, const int32_t* count, double* dt_k,
                         int32_t* active, int32_t* count_eff, float* f_eff, void* stream) {
  const size_t n = (size_t)B * nb * 3;
  hipLaunchKernelGGL(sub::lcp_substep_begin_kernel, dim3((unsigned)((n + sub::T - 1) / sub::T)), dim3(sub::T), 0, (hipStream_t)stream, B, nb * 3, t,
                     end_t, f, count, dt_k, active, count_eff, f_eff);
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

int substep_commit_launch(int B, int nb, const int32_t* active, const float* v_old, float* v_new, void* stream) {
  const size_t n = (size_t)B * nb * 3;
  hipLaunchKernelGGL(sub::lcp_substep_commit_kernel, dim3((unsigned)((n + sub::T - 1) / sub::T)), dim3(sub::T), 0, (hipStream_t)stream, B, nb * 3,
                     active, v_old, v_new);
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace lcp
