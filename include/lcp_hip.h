/*
 * lcp_hip.h - C ABI of the MI355X-native batched LCP contact solver (liblcp_hip.so).
 *
 * This is the drop-in boundary for the hot path of locuslab/lcp-physics.  The reference
 * is pure Python and has no FFI of its own; each entry point below names the reference
 * interface it replaces (paths relative to /root/reference/lcp_physics).  The reference-
 * side binding a maintainer would add (a ctypes stub inside lcp/lcp.py and
 * physics/engines.py) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless stated otherwise; all tensors are
 *    row-major, contiguous, batch-major ([B, rows, cols]);
 *  - the caller owns every buffer, including the workspace (`lcp_workspace_bytes`);
 *    nothing is allocated, freed or synchronised inside; launches are ordered on `stream`
 *    (a hipStream_t passed as void*, NULL = the default stream);
 *  - return value: 0 = launched, <0 = invalid arguments / unsupported size (LCP_E_*);
 *    numerical trouble is NOT an error (the reference returns its best iterate silently,
 *    lcp/solvers/pdipm.py:99-102,133-136,176-179): it is reported per scene in `status`;
 *  - sizes: nz = number of primal variables, m = nineq (rows of G), e = neq (rows of A,
 *    may be 0: then A, b, y and their gradients may be NULL).
 *  - `compute`: arithmetic type used inside the kernels.  LCP_COMPUTE_F64 is the parity
 *    path (fp32 I/O, fp64 arithmetic); LCP_COMPUTE_F32 computes everything in fp32.
 *  - threading: the library holds no process-global mutable state.  Every launch is planned from its own arguments and
 *    ordered on the caller's stream of the CURRENT device, so host threads may drive different streams / devices
 *    concurrently; the two lcp_debug_* settings are per calling thread.
 */
#ifndef LCP_HIP_H
#define LCP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LCP_COMPUTE_F32 0
#define LCP_COMPUTE_F64 1
/* May be OR-ed into the `compute` argument of lcp_pdipm_backward_f32: the workspace was left by a CONTACT-LIST forward
 * (lcp_step_fused_f32 / lcp_solve_dynamics_f32, sizes of the four-scenes-per-wave kernels: nz <= 16, <= 16 contacts, neq <= 4)
 * called with this same `compute` word - the dense backward (lcp.py:37-64) of a fused step.  One launch; it factors in body
 * space when that forward did (the workspace then holds no contact-space matrix at all). */
#define LCP_HINT_ALL_CONTACT 0x100
/* May be OR-ed into any `compute` argument: serve this call from the generic workgroup-per-scene kernels whatever the
 * sizes (A/B and debugging aid; a backward must carry the same flag as its forward - they share the workspace layout). */
#define LCP_PATH_GENERIC 0x200
/* Likewise (A/B aids): the contact-space kernels where the default is a body-space one; one wave per scene (lcp_primal) at every
 * size.  The kernel family of a call is a function of its sizes and its `compute` WORD: pass the word of the forward to the
 * backward and both plan the same workspace layout on any host threads.  The forward also leaves a layout tag in the workspace;
 * a backward planned for another layout returns NaN gradients instead of misreading it. */
#define LCP_PATH_CONTACT_SPACE 0x2000
#define LCP_PATH_PRIMAL 0x4000
/* Likewise: the contact-list step on one workgroup per scene in body space (lcp_primal_wg.hip) wherever its sizes allow - at most 128
 * pivots (3 nb - 3 under LCP_HINT_PINNED with e = 3, else 3 nb + e with e <= 4), at most 256 contacts, fp64 arithmetic - also where
 * another family would serve the call by default (A/B aid; the backward must carry the same bit).  lcp_post_stabilization_f32 and its
 * backward follow the bit too (lcp_primal_wg_poststab.hip: 3 nb + e <= 128 with e <= 4, at most 256 contacts). */
#define LCP_PATH_PRIMAL_WG 0x80000
/* Contact-list forwards of the four-scenes-per-wave sizes choose by batch size between four scenes per wavefront (lcp_quad.hip) and
 * one scene per wavefront (lcp_solo.hip, small batches); these force one of the two (A/B aids; same workspace layout, any backward
 * follows either). */
#define LCP_PATH_QUAD 0x8000
#define LCP_PATH_SOLO 0x10000
/* May be OR-ed into the `compute` argument of the contact-list forwards (lcp_step_fused_f32, lcp_solve_dynamics_f32): the caller
 * asserts that the equality rows of EVERY scene pin the leading coordinates - Je = [I 0], the TotalConstraint that fixes the floor of
 * the reference's demo worlds (physics/constraints.py:175-192) - or that there are none.  The four-scenes-per-wave family then skips
 * the launch that serves scenes with other equality rows (it finds nothing to do on such batches and costs 2-5 us); the
 * one-wave-per-scene family (17..64 contacts) forms and factors the free coordinates' system only (three pinned rows: 30 pivots
 * instead of 36 on BASELINE config 5).  The word travels with the op: the backward entry points take the same hint.  A scene that
 * breaks the promise is NOT solved: its new velocities are NaN and LCP_ST_NAN is set. */
#define LCP_HINT_PINNED 0x20000
/* OR-ed into the `compute` argument of lcp_workspace_bytes by callers of the fp64-I/O entry points (lcp_pdipm_forward_f64 /
 * lcp_pdipm_backward_f64): their workspace also keeps an fp64 copy of F. */
#define LCP_IO_F64 0x400

/* May be OR-ed into the `compute` argument of lcp_pdipm_backward_f32 / _f64 (round 6; SURVEY.md §0.5: "offer the adjoint-correct
 * backward as an opt-in flag, never as default"): solve with K^T instead of K.  The reference's LCPFunction.backward (lcp/lcp.py:46-50)
 * solves the KKT system itself - exact only where the LCP matrix F is symmetric, and the contact LCP's F is not (engines.py:69-73: +mu in
 * the cone rows, +1 / -1 between friction and cone rows).  K^T is K with F^T in place of F (every other block sits symmetrically), so the
 * transposed solve factors T^T = R^T + diag(s / z) from the R = G Q^-1 G^T - ... + F the forward left in the workspace.  Served by the
 * generic kernels only: the forward of such a call must have run with LCP_PATH_GENERIC (any other workspace layout returns NaN gradients
 * through the layout tag, as every mismatch does).  lcp_physics_amd.lcp.LCPFunction(adjoint_backward=True) sets both bits. */
#define LCP_BWD_ADJOINT 0x40000

#define LCP_E_BADARG   (-1)   /* null pointer / non-positive size                     */
#define LCP_E_TOOLARGE (-2)   /* problem does not fit the kernels' LDS/workspace plan (the generic kernels keep the matrices in the
                               * workspace when 160 KB of LDS do not hold them: e.g. 32 bodies x 128 contacts in fp64 plan; the limit
                               * is the vectors, ~(8 nz + 15 nineq + 9 neq) numbers in LDS)                                   */
#define LCP_E_LAUNCH   (-3)   /* hipLaunchKernel reported an error                     */

/* per-scene status bits written to `status[B]` */
#define LCP_ST_SINGULAR_Q   1  /* zero/NaN pivot while inverting Q   (pdipm.py:361-368 raises) */
#define LCP_ST_SINGULAR_S11 2  /* zero/NaN pivot in A Q^-1 A^T                                  */
#define LCP_ST_SINGULAR_T   4  /* exact zero pivot in LU(T): best iterate returned (pdipm.py:99-102) */
#define LCP_ST_NAN          8  /* the returned iterate contains NaN                             */
#define LCP_ST_TRUNCATED   16  /* c_count[k] > maxc: the scene was solved with its first maxc contacts only (the reference's
                                  list is unbounded, world.py:139-142) - enlarge maxc and redo the step      */

/* Library / build identification: returns a static string such as
 * "lcp_hip 0.1.0 gfx950".  Host-only, never touches the GPU. */
const char* lcp_version(void);

/* Bytes of workspace the forward/backward pair needs for a batch (caller allocates,
 * 256-byte aligned).  Holds what the reference keeps on the op instance between forward
 * and backward (lcp/lcp.py:28-29: Q_LU, S_LU, R, nus, lams, slacks): R, Q^-1, G Q^-1 A^T,
 * (A Q^-1 A^T)^-1 and the best iterate in compute precision.  Host-only. */
size_t lcp_workspace_bytes(int B, int nz, int m, int e, int compute);

/* Replaces LCPFunction.forward (lcp/lcp.py:22-35) = pdipm.pre_factor_kkt
 * (lcp/solvers/pdipm.py:357-408) + pdipm.forward (pdipm.py:49-179) with factor_kkt
 * (:414-454), solve_kkt (:325-354) and get_step (:182-186), per-scene (batch-1) semantics.
 *   in : Q[B,nz,nz] p[B,nz] G[B,m,nz] h[B,m] A[B,e,nz] b[B,e] F[B,m,m]
 *   out: x[B,nz] (zhats)  y[B,e] (nus)  z[B,m] (lams)  s[B,m] (slacks)
 *        iters[B]  (PDIPM loop iterations executed = factorisations inside the loop)
 *        status[B] (LCP_ST_* bits)
 * eps / max_iter / not_improved_lim: lcp/lcp.py:12-13 (1e-12, 10, 3). */
int lcp_pdipm_forward_f32(int B, int nz, int m, int e,
                          const float* Q, const float* p, const float* G, const float* h,
                          const float* A, const float* b, const float* F,
                          double eps, int max_iter, int not_improved_lim, int compute,
                          float* x, float* y, float* z, float* s,
                          int32_t* iters, int32_t* status, void* ws, void* stream);

/* Same, fp64 I/O and fp64 arithmetic (the reference's default dtype, physics/utils.py:34). */
int lcp_pdipm_forward_f64(int B, int nz, int m, int e,
                          const double* Q, const double* p, const double* G, const double* h,
                          const double* A, const double* b, const double* F,
                          double eps, int max_iter, int not_improved_lim,
                          double* x, double* y, double* z, double* s,
                          int32_t* iters, int32_t* status, void* ws, void* stream);

/* Replaces LCPFunction.backward (lcp/lcp.py:37-64): d = lams/slacks, factor_kkt, one
 * solve_kkt with rhs (dl_dx, 0, 0, 0), then the outer products.  Uses the workspace left
 * by the matching forward call (same B, nz, m, e, compute).  The reference solves with K,
 * not K^T (exact only for symmetric F); that formula is reproduced.
 *   in : G[B,m,nz] A[B,e,nz] dl_dx[B,nz]
 *   out: dQ[B,nz,nz] dp[B,nz] dG[B,m,nz] dh[B,m] dA[B,e,nz] db[B,e] dF[B,m,m]
 *        (any output pointer may be NULL to skip that gradient)
 * At an iterate that converged to rounding (d_i = lams_i / slacks_i of 1e16 and more) the matrix of lcp.py:46 is singular to working
 * precision wherever contact points are redundant; an elimination that meets a pivot of rounding noise there (or an exact zero) is
 * repeated with slacks_i / lams_i floored at 1e-12 x the row's diagonal of G Q^-1 G^T - the body-space kernels floor always and refine
 * once - so that dl/dp, dQ, dA, db stay the gradients of the converged solution instead of the cancellation error of multipliers of
 * 1e15 (the reference's own pivoted LU has that exposure; tests/parity.py::own_iterate_backward is the gate).
 * Alignment (m of 65 .. 256 rows, the dense route of 17 .. 64 contacts): scenes the forward classified as contact LCPs with at most two
 * bodies per contact are served by kernels that move F, dG and dF in 16-byte pieces.  The forward only hands that class out when F and G
 * are 16-byte aligned (torch allocations are; a view with an odd storage offset is not - such a call is solved by the contact-space
 * kernels instead); the backward of a forward that did returns LCP_E_BADARG for a dG or dF that is not 16-byte aligned.  For those scenes
 * the backward reads the Jacobian rows from the records the forward left in the workspace: the G passed here must be the forward's G. */
int lcp_pdipm_backward_f32(int B, int nz, int m, int e,
                           const float* G, const float* A, const float* dl_dx, int compute,
                           float* dQ, float* dp, float* dG, float* dh,
                           float* dA, float* db, float* dF,
                           void* ws, void* stream);

int lcp_pdipm_backward_f64(int B, int nz, int m, int e,
                           const double* G, const double* A, const double* dl_dx,
                           double* dQ, double* dp, double* dG, double* dh,
                           double* dA, double* db, double* dF,
                           void* ws, void* stream);

/* Replaces the contact branch of PdipmEngine.solve_dynamics (physics/engines.py:26-78)
 * for B independent scenes: assembles u = M v + dt f (engines.py:31-32), Jc / Jf / mu / E /
 * restitutions (physics/world.py:144-234) into the dense (Q,p,G,h,A,b,F) the reference hands
 * to LCPFunction (engines.py:67-76).  nb bodies (3 DoF each, nz = 3 nb), nc contacts
 * (m = 4 nc, two friction directions), e joint rows.
 *   in : Mdiag[B,nb,3] v[B,nb,3] f[B,nb,3] rest[B,nb] fric[B,nb]
 *        c_n[B,nc,2] c_p1[B,nc,2] c_p2[B,nc,2] c_i1[B,nc] c_i2[B,nc] (int32)  Je[B,e,nz]
 *   out: Q[B,nz,nz] p[B,nz] G[B,m,nz] h[B,m] A[B,e,nz] b[B,e] F[B,m,m] */
int lcp_assemble_contacts_f32(int B, int nb, int nc, int e,
                              const float* Mdiag, const float* v, const float* f,
                              const float* rest, const float* fric,
                              const float* c_n, const float* c_p1, const float* c_p2,
                              const int32_t* c_i1, const int32_t* c_i2, const float* Je, float dt,
                              float* Q, float* p, float* G, float* h, float* A, float* b, float* F,
                              void* stream);

/* One fused simulation step for B scenes in a single launch: the assembly above, the LCP
 * solve (as lcp_pdipm_forward_f32), new_v = -x (engines.py:76-77) and the semi-implicit
 * integrator p <- p + new_v dt of Body.move (physics/bodies.py:80-82).  Dense LCP data
 * never leaves the chip.  Leaves the same workspace as the forward so that
 * lcp_pdipm_backward_f32 can follow (with G from lcp_assemble_contacts_f32).
 *   out: v_new[B,nb,3]  p_new[B,nb,3]  z[B,m]  s[B,m]  y[B,e]  iters[B]  status[B]
 *        z, s, y may be NULL: the multipliers are then not written out (the reference's step returns new_v only, engines.py:76-77;
 *        the backward reads them, in fp64, from the workspace either way).
 * Sizes and kernel families as lcp_solve_dynamics_f32 (every scene at nc contacts). */
int lcp_step_fused_f32(int B, int nb, int nc, int e,
                       const float* pos, const float* Mdiag, const float* v, const float* f,
                       const float* rest, const float* fric,
                       const float* c_n, const float* c_p1, const float* c_p2,
                       const int32_t* c_i1, const int32_t* c_i2, const float* Je, float dt,
                       double eps, int max_iter, int not_improved_lim, int compute,
                       float* v_new, float* p_new, float* z, float* s, float* y,
                       int32_t* iters, int32_t* status, void* ws, void* stream);

/* Backward of lcp_step_fused_f32 / lcp_solve_dynamics_f32 with respect to the PHYSICAL inputs of the step: what the
 * reference obtains by autograd through PdipmEngine.solve_dynamics (physics/engines.py:31-32,50-77) and the World
 * Jacobian builders (physics/world.py:144-234) on top of LCPFunction.backward (lcp/lcp.py:37-64).  The rank-1 LCP
 * gradients (dQ, dp, dG, dh, dF of lcp.py:52-61) are contracted on chip and never written.  Must follow the forward on
 * the same stream with the same workspace and the same (unchanged) inputs.
 *   in : the inputs of the forward, dl_dv[B,nb,3] = d(loss)/d(v_new)
 *   out: dMdiag[B,nb,3] dv[B,nb,3] df[B,nb,3] drest[B,nb] dfric[B,nb] dc_n[B,nc,2] dc_p1[B,nc,2] dc_p2[B,nc,2]
 *        (any may be NULL; padded contact slots get 0).  The joint Jacobian Je is treated as a constant here: see
 *        lcp_step_backward_je_f32 for its gradient.
 * Sizes: 3 nb <= 16, nc <= 16, e <= 4 after either forward; 3 nb <= 32 with nc <= 16, and up to nc <= 64, 3 nb <= 43,
 * e <= 4 (fp64 arithmetic), after lcp_solve_dynamics_f32 only (its kernels own the workspace layout); 5 <= e <= 24 equality rows
 * (chains of joints) with nc <= 64 and 3 nb + e <= 56, or e <= 4 with 3 nb + e <= 64 (18 .. 20 bodies; round 6) (fp64 arithmetic) after either
 * forward; beyond those, up to 128 pivots (3 nb - 3 under LCP_HINT_PINNED with e = 3: 43 bodies; else 3 nb + e, e <= 4: 41 bodies)
 * and up to 256 contacts (fp64 arithmetic) on the workgroup-per-scene body-space kernel (lcp_primal_wg.hip) after either forward;
 * every other size the generic
 * kernels step forward - more than 64 contacts, 3 nb + e > 56, fp32 arithmetic beyond 16 contacts: lcp_step_bwd_kernel on the iterate
 * lcp_step_kernel leaves, each scene at its own contact count - after either forward, in either arithmetic.  LCP_E_TOOLARGE only for
 * the wave64 step family (fp32 arithmetic, 3 nb <= 16, 5 <= e <= 8: its kernel keeps no iterate) and beyond the generic plan. */
int lcp_step_backward_f32(int B, int nb, int nc, int e,
                          const float* Mdiag, const float* v, const float* f,
                          const float* rest, const float* fric,
                          const float* c_n, const float* c_p1, const float* c_p2,
                          const int32_t* c_i1, const int32_t* c_i2, const float* Je, float dt,
                          const float* dl_dv, int compute,
                          float* dMdiag, float* dv, float* df, float* drest, float* dfric,
                          float* dc_n, float* dc_p1, float* dc_p2, void* ws, void* stream);

/* Host-only: 1 when lcp_step_backward_f32 / _je_f32 can follow a contact-list forward (lcp_step_fused_f32,
 * lcp_solve_dynamics_f32) called with these sizes and this `compute` word - since round 6 every size the forward itself accepts
 * except the wave64 step family (fp32 arithmetic, 3 nb <= 16, 5 <= e <= 8) -, else 0: the backward entry points return
 * LCP_E_TOOLARGE there.  The reference differentiates any size through LCPFunction.backward (lcp/lcp.py:37-64): the dense boundary
 * (lcp_physics_amd/physics/dense_step.py) is what the host falls back on for a 0. */
int lcp_step_has_backward(int nb, int maxc, int e, int compute);

/* The same with the gradient of the joint Jacobian as a ninth output: dJe[B,e,3 nb] = dnu (x) x + nu (x) dx (lcp.py:57, A = Je
 * in engines.py:75) - what the reference back-propagates into Joint.J() / FixedJoint.J() (constraints.py:26-36, 64-73: the
 * anchor arms follow the bodies' poses) when a world with joints is differentiated through its steps.  dJe may be NULL. */
int lcp_step_backward_je_f32(int B, int nb, int nc, int e,
                             const float* Mdiag, const float* v, const float* f,
                             const float* rest, const float* fric,
                             const float* c_n, const float* c_p1, const float* c_p2,
                             const int32_t* c_i1, const int32_t* c_i2, const float* Je, float dt,
                             const float* dl_dv, int compute,
                             float* dMdiag, float* dv, float* df, float* drest, float* dfric,
                             float* dc_n, float* dc_p1, float* dc_p2, float* dJe, void* ws, void* stream);

/* Replaces PdipmEngine.solve_dynamics (physics/engines.py:26-78) for B scenes whose contact lists have
 * DIFFERENT lengths (what contact detection produces): scene k uses the first c_count[k] <= maxc records of
 * its padded contact list and solves the mixed LCP of exactly that size (nineq = 4 c_count[k], engines.py:51-76);
 * a scene without contacts takes the direct KKT solve of engines.py:36-50.  One launch, no position update
 * (that is lcp_move_find_contacts_f64).  Arguments as lcp_step_fused_f32; z, s use the row layout of a
 * maxc-contact LCP ([normal | friction pairs | gamma] blocks of maxc, 2 maxc, maxc rows), padded slots are 0.
 * Served by the four-scenes-per-wave kernel when 3 nb <= 32, maxc <= 16, e <= 4: the workspace it leaves then feeds
 * lcp_step_backward_f32 (padded slots get zero gradients) and, for 3 nb <= 16, lcp_pdipm_backward_f32 (m = 4 maxc).
 * Larger scenes - maxc <= 64 with 3 nb + e <= 56 and e <= 24 (chains of joints: two rows per revolute joint), with 3 nb + e <= 64 and
 * e <= 4 (up to 20 bodies on a pinned floor: the 64-row instantiation, every lane of the wave a row; round 6), or 3 nb <= 43,
 * e <= 4 - run (fp64 arithmetic) on the wave-per-scene body-space kernel (BASELINE config 5) or the workgroup-per-scene
 * contact-space kernel, and can be followed by lcp_step_backward_f32 (not by the dense backward).  Beyond those, systems of up to 128
 * pivots (3 nb - 3 under LCP_HINT_PINNED with e = 3: up to 43 bodies; 3 nb + e with e <= 4 otherwise: up to 41 bodies) with up to 256
 * contacts run (fp64 arithmetic) on the workgroup-per-scene BODY-space kernel (lcp_primal_wg.hip: one workgroup of 256 threads per
 * scene, the system in LDS), followed by lcp_step_backward_f32 as well (not by the dense backward); anything else - more pivots,
 * 5 .. 24 equality rows beyond 56 rows, fp32 arithmetic - runs on the generic kernels (LCP_E_TOOLARGE beyond their LDS / workspace plan), which keep each scene's iterate and its contact count for
 * lcp_step_backward_f32 as well (round 6).
 *   out: v_new[B,nb,3]  z[B,4 maxc]  s[B,4 maxc]  y[B,e]  iters[B]  status[B] */
int lcp_solve_dynamics_f32(int B, int nb, int maxc, int e, const int32_t* c_count,
                           const float* Mdiag, const float* v, const float* f,
                           const float* rest, const float* fric,
                           const float* c_n, const float* c_p1, const float* c_p2,
                           const int32_t* c_i1, const int32_t* c_i2, const float* Je, float dt,
                           double eps, int max_iter, int not_improved_lim, int compute,
                           float* v_new, float* z, float* s, float* y,
                           int32_t* iters, int32_t* status, void* ws, void* stream);

/* Replaces PdipmEngine.post_stabilization (physics/engines.py:80-116) and the correction move World.step_dt makes with
 * its result (physics/world.py:109-117), for B scenes in one launch.  Per scene the frictionless LCP
 *   Q = M, p = 0, G = Jc (world.py:172-184), h = gc = Jc v + Jc v * -restitutions (:87-89), A = Je, b = ge = Je v (:86),
 *   F = 0 (:110), solver defaults (lcp.py:12-13: pass eps = 1e-12, max_iter = 10, not_improved_lim = 3)
 * over the first c_count[k] entries of the padded contact list; dp = -x (:115).  A scene without contacts takes the
 * direct solve [[M, -Je^T], [Je, 0]]^-1 [0; ge] (:92-103).  `v` are the velocities AFTER the dynamics solve and the
 * contacts those found after the move (world.py:87-94).  When p / p_out are given, p_out = p + (dp / 2) dt_k with
 * dt_k = dt_scene[k] (the dt the scene's step ended up using; NULL: the scalar `dt`) - world.py:110-117; the caller
 * re-detects contacts at p_out (world.py:121: lcp_move_find_contacts_f64 with v = NULL); p_out may be p itself.
 * Runs on the wave-per-scene body-space kernel (fp64 arithmetic, maxc <= 64, e <= 24, 3 nb + e <= 56, or e <= 4 with 3 nb + e <= 64; it leaves its best
 * iterate in the workspace for lcp_post_stabilization_backward_f32); beyond those sizes on the workgroup-per-scene BODY-space kernel
 * (lcp_primal_wg_poststab.hip: fp64 arithmetic, 3 nb + e <= 128 with e <= 4 - 41 bodies on a three-row floor -, maxc <= 256; one
 * workgroup of 256 threads per scene, the system in LDS, its own workspace layout and tag) where the capacity is at least three
 * contact slots per two bodies (4 maxc >= 6 nb: below that the generic kernels are as fast) or LCP_PATH_PRIMAL_WG asks for it; else on
 * the workgroup-per-scene generic kernels (any size their plan takes: LCP_E_TOOLARGE beyond); workspace of
 * lcp_workspace_bytes(B, 3 nb, 4 maxc, e, compute).
 *   out: dp[B,nb,3]  p_out[B,nb,3] (optional)  iters[B]  status[B] */
int lcp_post_stabilization_f32(int B, int nb, int maxc, int e, const int32_t* c_count,
                               const float* Mdiag, const float* v, const float* rest,
                               const float* c_n, const float* c_p1, const float* c_p2,
                               const int32_t* c_i1, const int32_t* c_i2, const float* Je,
                               double eps, int max_iter, int not_improved_lim, int compute,
                               const double* p, const double* dt_scene, double dt, double* p_out,
                               float* dp, int32_t* iters, int32_t* status, void* ws, void* stream);

/* Backward of lcp_post_stabilization_f32 with respect to its physical inputs - what the reference obtains by autograd
 * through PdipmEngine.post_stabilization (engines.py:80-116: ge = Je v, gc = Jc v + Jc v * -restitutions, the LCPFunction
 * call and its backward lcp.py:37-64, dp = -x) when a World with post_stab=True is differentiated (experiments/inference.py).
 * Must follow the forward on the same stream with the same workspace and unchanged inputs.  Body-space kernel where the forward
 * ran there (fp64 arithmetic, maxc <= 64, e <= 24, 3 nb + e <= 56, or e <= 4 with 3 nb + e <= 64: one wave per scene; beyond them
 * 3 nb + e <= 128 with e <= 4 and maxc <= 256: one workgroup per scene, lcp_primal_wg_poststab.hip - the same `compute` word picks
 * the same family), else (round 6) the generic kernels on the iterate
 * lcp_post_stab_kernel keeps - any size of their plan, either arithmetic; LCP_E_TOOLARGE beyond it.
 *   in : the forward's inputs, dl_ddp[B,nb,3] = d(loss)/d(dp)
 *   out: dMdiag[B,nb,3] dv[B,nb,3] drest[B,nb] dc_n[B,maxc,2] dc_p1[B,maxc,2] dc_p2[B,maxc,2] dJe[B,e,3nb]
 *        (any may be NULL; padded contact slots get 0) */
int lcp_post_stabilization_backward_f32(int B, int nb, int maxc, int e,
                                        const float* Mdiag, const float* v, const float* rest,
                                        const float* c_n, const float* c_p1, const float* c_p2,
                                        const int32_t* c_i1, const int32_t* c_i2, const float* Je,
                                        const float* dl_ddp, int compute,
                                        float* dMdiag, float* dv, float* drest,
                                        float* dc_n, float* dc_p1, float* dc_p2, float* dJe,
                                        void* ws, void* stream);

/* Host-only: 1 when lcp_post_stabilization_backward_f32 can follow lcp_post_stabilization_f32 at these sizes and this `compute`
 * word - every size the forward accepts, since round 6 -, else 0 (the host would then differentiate the correction through the dense
 * boundary, the way engines.py:80-116 itself does: lcp_physics_amd/physics/dense_step.py). */
int lcp_post_stabilization_has_backward(int nb, int maxc, int e, int compute);

/* Replaces the position update of World.step_dt (physics/world.py:88-101,122) together with the
 * contact generation it calls, for B independent scenes in one launch:
 *   Body.move (physics/bodies.py:80-82)         p_try = p_start + v dt
 *   World.find_contacts (world.py:139-142)      all body pairs i < j (the reference delegates the
 *                                               broadphase to ODE; `no_contact[B,nb,nb]` != 0 skips a pair)
 *   DiffContactHandler.__call__ (physics/contacts.py:57-205) circle/circle, circle/hull (GJK + SAT),
 *                                               hull/hull (SAT, incident edge, clipping), with its helpers
 *                                               (contacts.py:207-352) and rotate_verts (bodies.py:211-214)
 *   the penetration test and dt halving (world.py:95-101): while any contact penetrates by more than
 *   `tol`, dt <- dt / 2 and retry from p_start; `strict` = strict_no_penetration, `dt_floor` = world.dt / 4
 *   (non-strict worlds accept once dt < dt_floor).  The loop is per scene and runs on the device;
 *   `max_trials` bounds it (the reference would spin forever on a pose that penetrates at dt -> 0).
 * Geometry and poses are fp64 (tol = 1e-6 against coordinates of several hundred cannot be resolved in
 * fp32); the contact frame handed to the LCP kernels is fp32.
 *   in : kind[B,nb] (0 circle, 1 hull)  radius[B,nb]  verts_local[B,nb,8,2] (body frame, CCW as the
 *        reference's Hull.verts; lcp_move_find_contacts_nv_f64 takes other capacities)  nverts[B,nb]  p_start[B,nb,3]
 *        (rot,x,y)  v[B,nb,3] (NULL: detect at p_start)
 *   out: p_out[B,nb,3]  c_n/c_p1/c_p2[B,maxc,2]  c_pen[B,maxc]  c_i1/c_i2[B,maxc]  count[B] (contacts found,
 *        in the reference's order; > maxc means the list was truncated)  max_pen[B]  dt_used[B]
 *        t[B] (+= dt_used)  trials[B]   (c_pen, max_pen, dt_used, t, trials, p_out may be NULL)
 * nb <= 32, hulls of <= 8 vertices (LCP_E_TOOLARGE beyond; larger scenes: lcp_move_find_contacts_nv_f64). */
int lcp_move_find_contacts_f64(int B, int nb, int maxc,
                               const int32_t* kind, const double* radius, const double* verts_local,
                               const int32_t* nverts, const uint8_t* no_contact,
                               const double* p_start, const float* v,
                               double dt, double dt_floor, int strict, int max_trials,
                               double eps, double tol,
                               double* p_out, float* c_n, float* c_p1, float* c_p2, double* c_pen,
                               int32_t* c_i1, int32_t* c_i2, int32_t* count, double* max_pen,
                               double* dt_used, double* t, int32_t* trials, void* stream);

/* Replaces World.Je (physics/world.py:156-170) over the joints' J() (physics/constraints.py:13-217) and Joint.move /
 * update_pos (constraints.py:39-50) for B scenes: joints whose Jacobian follows the pose.
 *   jtype[B,nj]: 1 Joint (revolute, 2 rows)  2 FixedJoint (3 rows)  3 XConstraint  4 YConstraint  5 RotConstraint (1 row each)
 *                6 TotalConstraint (3 rows)  0 empty;   jb1 / jb2 [B,nj] body indices (jb2 = -1: no second body)
 *   jr1 / jrot1 [B,nj]: polar coordinates of a Joint's anchor relative to body 1 (cart_to_polar with the positive-angle rule,
 *                utils.py:75-82); jrot1 is state: with `v` != NULL it is first advanced by vscale * v[body1][0] * dt_k,
 *                dt_k = dt_scene[k] (NULL: `dt`) - the dt the scene's step accepted (world.py:88-107 restores the joints before
 *                every retry); vscale = 1 for the dynamics move, 0.5 for the post-stabilisation move (world.py:112).
 *   p[B,nb,3] the pose the Jacobian is wanted at;  out: Je[B,e,3 nb] float32, e = the rows the joint list adds up to. */
int lcp_joint_jacobian_f64(int B, int nb, int nj, int e,
                           const int32_t* jtype, const int32_t* jb1, const int32_t* jb2,
                           const double* jr1, double* jrot1, const double* p,
                           const float* v, const double* dt_scene, double dt, double vscale,
                           float* Je, void* stream);

/* Backward of lcp_joint_jacobian_f64 with respect to the pose and the revolute joints' angles: what the reference obtains by autograd
 * through Joint.J() / FixedJoint.J() with update_pos (physics/constraints.py:26-50, 64-85) when a roll-out with joints is
 * back-propagated (experiments/inference.py:55-61).  jrot1[B,nj]: the angles the Jacobian was evaluated at (a copy taken then - the
 * forward advances its jrot1 in place);  gJe[B,e,3 nb] float32 = d(loss)/dJe (lcp_step_backward_je_f32's dJe).
 *   out: g_p[B,nb,3] float64 (written, not accumulated; only the x / y columns of the joints' bodies are non-zero), g_rot[B,nj]. */
int lcp_joint_jacobian_backward_f64(int B, int nb, int nj, int e,
                                    const int32_t* jtype, const int32_t* jb1, const int32_t* jb2,
                                    const double* jr1, const double* jrot1, const float* gJe,
                                    double* g_p, double* g_rot, void* stream);

/* Backward of the state update that ends a differentiable step - Body.move (physics/bodies.py:80-82), the vertex turn it skips for a
 * zero rotation increment (bodies.py:199-202) and Joint.move (constraints.py:39-43) - with respect to the velocities moved by:
 *   p_new = p + scale v dt_k (cotangent g_p);  the pose the geometry is differentiated at, geo_new = p_geo + the same increment where
 *   it is non-zero or the coordinate is x / y (cotangent g_g);  rot_new = rot + scale v[body1][0] dt_k for revolute joints (g_rot).
 * g_p / g_g [B,nb,3] float64 and g_rot [B,nj] float64 may be NULL (no such cotangent);  v[B,nb,3] float32 the velocities of the move
 * (new_v, or the post-stabilisation dp with scale = 0.5, world.py:112);  dt_scene[B] >= 0 the dt each scene's step accepted (0: a scene that
 * was finished in a sub-step of fixed-interval stepping and did not move - its g_v is exactly 0);
 * jtype / jb1 [B,nj] as in lcp_joint_jacobian_f64 (needed with g_rot).   out: g_v[B,nb,3] float32 = d(loss)/dv. */
int lcp_state_update_backward_f64(int B, int nb, int nj,
                                  const double* g_p, const double* g_g, const double* g_rot,
                                  const float* v, const double* dt_scene, double scale,
                                  const int32_t* jtype, const int32_t* jb1, float* g_v, void* stream);

/* Backward of the contact frame with respect to the poses: what the reference obtains by autograd through
 * DiffContactHandler (physics/contacts.py:57-352 - every operation of the contact tuple is a differentiable torch op,
 * including the rotated hull vertices of bodies.py:211-214), needed to back-propagate through a roll-out
 * (demos/grad_demo.py:45-50, experiments/inference.py:55-61).  Every record type: circle / circle, circle / hull (GJK or
 * SAT), hull / hull (SAT, incident edge, clipping); the derivative follows the branches the detection took (as autograd does).
 *   in : the geometry and the pose `p` lcp_move_find_contacts_f64 detected the contact list at (its p_out), its `eps`,
 *        count[B], and g_n / g_p1 / g_p2 [B,maxc,2] = d(loss)/d(c_n, c_p1, c_p2) (what lcp_step_backward_f32 returns)
 *   out: dp[B,nb,3] = d(loss)/d(pose) through the contact frame (overwritten).   nb <= 32, hulls of <= 8 vertices
 *   (LCP_E_TOOLARGE beyond; larger scenes: lcp_contact_frame_backward_nv_f64). */
int lcp_contact_frame_backward_f64(int B, int nb, int maxc,
                                   const int32_t* kind, const double* radius, const double* verts_local,
                                   const int32_t* nverts, const uint8_t* no_contact,
                                   const double* p, double eps, const int32_t* count,
                                   const float* g_n, const float* g_p1, const float* g_p2,
                                   double* dp, void* stream);

/* lcp_move_find_contacts_f64 for hulls of up to 64 vertices and scenes of up to 64 bodies (the reference's Hull takes any
 * number of vertices, bodies.py:154-250; World.find_contacts any number of bodies, world.py:139-142).  Same arguments, same
 * semantics and outputs (pair order i < j, no_contact, count > maxc reported, padding, p_out / max_pen / dt_used / t / trials), plus
 *   nvcap            the vertex capacity of verts_local[B,nb,nvcap,2], 8 <= nvcap <= 64 (hulls of 3 .. nvcap vertices)
 *   scene_verts_max  an upper bound of sum(nverts) over the hulls of any one scene, <= 1024 (it sizes the LDS: 60 B per vertex)
 * LCP_E_TOOLARGE for nb > 64, nvcap outside [8, 64] or scene_verts_max > 1024 (checked before any launch); a scene whose
 * vertices exceed scene_verts_max gets count = -1 and no records.  Same double-precision geometry in the same order as
 * lcp_move_find_contacts_f64: on the sizes both take, the outputs are bitwise the same (lcp_contacts_wide.hip). */
int lcp_move_find_contacts_nv_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max,
                                  const int32_t* kind, const double* radius, const double* verts_local,
                                  const int32_t* nverts, const uint8_t* no_contact,
                                  const double* p_start, const float* v,
                                  double dt, double dt_floor, int strict, int max_trials,
                                  double eps, double tol,
                                  double* p_out, float* c_n, float* c_p1, float* c_p2, double* c_pen,
                                  int32_t* c_i1, int32_t* c_i2, int32_t* count, double* max_pen,
                                  double* dt_used, double* t, int32_t* trials, void* stream);

/* The move / detect / halve loop of World.step_dt (physics/world.py:88-101) when World.step(fixed_dt=True) drives it
 * (world.py:72-80: `while self.t < end_t: self.step_dt(end_t - self.t)`): every scene starts its loop from a dt of its own.
 * The arguments, semantics and outputs of lcp_move_find_contacts_nv_f64, plus
 *   dt_scene[B]  (required) the dt each scene's loop starts from; the scalar `dt` is not read.  A scene with dt_scene <= 0 has
 *                reached its end_t: it makes one trial without moving and is done whatever the penetration test says -
 *                p_out = p_start bitwise, the records of that pose, dt_used = 0, t unchanged, trials = 1.
 * `dt_floor` stays the caller's (world.py:98 compares with self.dt / 4, the world's dt, not the sub-step's).
 * nb <= 32 with nvcap == 8 runs the kernels of lcp_move_find_contacts_f64, anything else those of the _nv_ entry; the size
 * errors are the _nv_ entry's (LCP_E_TOOLARGE for nb > 64, nvcap outside [8, 64], scene_verts_max > 1024), checked before
 * any launch.  With all dt_scene equal to a positive dt the outputs are bitwise those of the scalar entries. */
int lcp_move_find_contacts_dts_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max,
                                   const int32_t* kind, const double* radius, const double* verts_local,
                                   const int32_t* nverts, const uint8_t* no_contact,
                                   const double* p_start, const float* v,
                                   double dt, double dt_floor, int strict, int max_trials,
                                   double eps, double tol,
                                   double* p_out, float* c_n, float* c_p1, float* c_p2, double* c_pen,
                                   int32_t* c_i1, int32_t* c_i2, int32_t* count, double* max_pen,
                                   double* dt_used, double* t, int32_t* trials,
                                   const double* dt_scene, void* stream);

/* Detection with a broadphase in front of the narrow phase (lcp_contacts_bp.hip).  The reference's World.find_contacts
 * (physics/world.py:139-142) collides its geoms through ODE's HashSpace over bounding spheres padded by the margin
 * (physics/bodies.py:_create_geom), so only nearby pairs reach the contact handler; the _nv_ / _dts_ entries hand it all
 * nb (nb - 1) / 2 pairs.  This entry culls at every trial pose first.  Per body b: R_b the bounding radius about its position (the
 * radius of a circle, max |verts_local| of a hull), box_b the (min, max) of its rotated vertices relative to the position, mitre_b the
 * (min, max) over its vertices of m_k = (n_{k-1} + n_k) / (1 + n_{k-1} . n_k) with n the outward unit edge normals, kappa_b = max |m_k|
 * (a circle: box -+ radius, mitre -+ 1, kappa 1).  For the ordered pair (a, b), r = R_b + eps, S = R_a + kappa_a r, d = pos_b - pos_a:
 *   T(a, b):  |d|^2 <= S^2 (1 + 4e-9)  and  box_a.min + r mitre_a.min - 1e-9 S <= d <= box_a.max + r mitre_a.max + 1e-9 S on both axes.
 * A pair i < j reaches the narrow phase iff no_contact[i][j] is not set and T(i, j) and T(j, i) hold.  T relaxes the gates of the
 * narrow phase itself: hull / hull reports a point only after the separation along every edge normal of both hulls is <= eps, which
 * puts pos_b inside hull a offset outwards by r (vertices v_k + r m_k) - the DISTANCE between two hulls with a record can exceed eps
 * (two corners: up to eps / sin(angle / 2)), which kappa and the mitres cover; circle / hull and circle / circle report a point
 * only within eps.  So no record is lost, for convex, counter-clockwise, non-degenerate hulls, and the survivors keep the pair order.
 * The arguments of lcp_move_find_contacts_dts_f64 in the same order, then
 *   dt_scene[B]    or NULL.  NULL: every scene starts from the scalar `dt` (lcp_move_find_contacts_nv_f64); otherwise the
 *                  per-scene dt and the finished scenes of lcp_move_find_contacts_dts_f64.
 *   candidates[B]  or NULL: the number of pairs that passed the cull at the accepted trial pose (p_out).
 * Sizes and errors are those of the _nv_ entry, checked before any launch: nb <= 64, 8 <= nvcap <= 64, scene_verts_max <= 1024
 * (LCP_E_TOOLARGE beyond) - one kernel for all of them, nb <= 32 at capacity 8 included, so scene_verts_max is always read.
 * A scene whose vertices exceed scene_verts_max gets count = -1, padded records and candidates = 0.
 * Contract: every other output is bitwise that of lcp_move_find_contacts_nv_f64 (dt_scene NULL) / lcp_move_find_contacts_dts_f64
 * on the same inputs. */
int lcp_move_find_contacts_bp_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max,
                                  const int32_t* kind, const double* radius, const double* verts_local,
                                  const int32_t* nverts, const uint8_t* no_contact,
                                  const double* p_start, const float* v,
                                  double dt, double dt_floor, int strict, int max_trials,
                                  double eps, double tol,
                                  double* p_out, float* c_n, float* c_p1, float* c_p2, double* c_pen,
                                  int32_t* c_i1, int32_t* c_i2, int32_t* count, double* max_pen,
                                  double* dt_used, double* t, int32_t* trials,
                                  const double* dt_scene, int32_t* candidates, void* stream);

/* The head of one sub-step of World.step(fixed_dt=True) (physics/world.py:76-78) for B scenes, element-wise:
 *   in : t[B], end_t[B] float64 (the scenes' clocks and the time their step ends at)  f[B,nb,3] float32 (the forces at t)
 *        count[B] (the contacts of the current pose)
 *   out: dt_k[B] float64 = end_t - t where t < end_t, else 0 (world.py:77, that subtraction in fp64)
 *        active[B] int32 = t < end_t (world.py:76)
 *        count_eff[B] = count where active, else 0 (a finished scene takes the no-contact branch of the solve, engines.py:36-50)
 *        f_eff[B,nb,3] float32 = (float)dt_k * f, one fp32 product: lcp_solve_dynamics_f32 with dt = 1 and f_eff forms
 *        u = M v + dt_k f (engines.py:31-32) bit for bit as it would with a dt of dt_k per scene.
 * All outputs are required; none may alias an input. */
int lcp_substep_begin_f64(int B, int nb, const double* t, const double* end_t, const float* f,
                          const int32_t* count, double* dt_k, int32_t* active, int32_t* count_eff,
                          float* f_eff, void* stream);

/* The tail of the solve of one sub-step (physics/world.py:87 `set_v(new_v)`, which a finished scene never reaches):
 * v_new[B,nb,3] = active[B] ? v_new : v_old, in place (only the entries of finished scenes are written). */
int lcp_substep_commit_f32(int B, int nb, const int32_t* active, const float* v_old, float* v_new, void* stream);

/* lcp_contact_frame_backward_f64 at the sizes of lcp_move_find_contacts_nv_f64 (nb <= 64, verts_local[B,nb,nvcap,2] with
 * 8 <= nvcap <= 64, scene_verts_max <= 1024), plus the records' body indices c_i1 / c_i2 [B,maxc] of that detection: the
 * work is one lane per (contacting pair, pose coordinate) over the first min(count, maxc) records, summed per coordinate in
 * record order (deterministic).  no_contact is accepted for symmetry and not read (a masked pair has no records).
 * LCP_E_TOOLARGE beyond those sizes or when the LDS (40 B per vertex + 52 B per contact slot) exceeds 152 KB. */
int lcp_contact_frame_backward_nv_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max,
                                      const int32_t* kind, const double* radius, const double* verts_local,
                                      const int32_t* nverts, const uint8_t* no_contact,
                                      const double* p, double eps, const int32_t* count,
                                      const int32_t* c_i1, const int32_t* c_i2,
                                      const float* g_n, const float* g_p1, const float* g_p2,
                                      double* dp, void* stream);

/* Backward of the contact frame with respect to the SHAPE of the bodies: what the reference obtains by autograd when
 * Circle.rad (physics/bodies.py:121) or Hull.verts (bodies.py:168-171, turned by rotate_verts, bodies.py:211-214) are leaves -
 * every operation of DiffContactHandler (physics/contacts.py:57-352) is a torch op on those tensors, edge lengths and edge
 * normals included.  Same inputs and sizes as lcp_contact_frame_backward_nv_f64 (nb <= 64, 8 <= nvcap <= 64, scene_verts_max <=
 * 1024; nvcap = 8 is the layout of the lcp_move_find_contacts_f64 family, so this one entry serves both), every record type,
 * along the branches the detection took.
 *   out: d_radius[B,nb] and d_verts_local[B,nb,nvcap,2] (body frame: the world-frame term turned back by R(rot)^T), either may
 *        be NULL; written, not accumulated: circles get zero vertex gradient, hulls zero radius gradient, vertex slots >= nverts
 *        zero, and a scene whose vertices exceed scene_verts_max zeros throughout.
 * One lane per (contacting pair, shape coordinate its records were built from: two radii, the reference edge's and the incident
 * edge's or GJK simplex's vertices - at most 10) over the first min(count, maxc) records, summed in record order (no atomics:
 * deterministic).  LCP_E_TOOLARGE beyond those sizes or when the LDS (40 B per vertex + 112 B per contact slot) exceeds 152 KB. */
int lcp_contact_frame_backward_shape_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max,
                                         const int32_t* kind, const double* radius, const double* verts_local,
                                         const int32_t* nverts, const double* p, double eps, const int32_t* count,
                                         const int32_t* c_i1, const int32_t* c_i2,
                                         const float* g_n, const float* g_p1, const float* g_p2,
                                         double* d_radius, double* d_verts_local, void* stream);

/* ---- bodies: mass properties and gravity from shape and mass ----
 * Per-body status bits of lcp_body_properties_f64.  A hull gets the first that applies of COUNT and DEGENERATE alone (nothing
 * else can be said of it), otherwise ORIENTATION and / or NONCONVEX; a circle only DEGENERATE (non-finite radius or mass). */
#define LCP_BODY_ST_COUNT        1  /* nverts < 3 or nverts > cap                        (bodies.py:169 `len(verts) > 2`)          */
#define LCP_BODY_ST_ORIENTATION  2  /* sum (x2 - x1)(y2 + y1) >= 0: not the reference's vertex order (bodies.py:228-235)            */
#define LCP_BODY_ST_NONCONVEX    4  /* two consecutive edges turn against the polygon's orientation                               */
#define LCP_BODY_ST_DEGENERATE   8  /* sum cross_2d(v_i+1, v_i) == 0 (no area), or a non-finite vertex, radius or mass            */

/* What the reference's body constructors compute, for B x nb bodies in one launch (lcp_bodies.hip): Circle.__init__ /
 * _get_ang_inertia (physics/bodies.py:116-126), Hull.__init__ (bodies.py:162-177: `_get_centroid` :216-226, the recentred
 * `verts` :171, `pos = ref_point + centroid` :173, `_is_clockwise` :228-235), Hull._get_ang_inertia (:179-189, on the recentred
 * vertices), Body.M (:44-47) and Gravity.set_body (forces.py:64-67).  A Rect is the hull of its four vertices (bodies.py:260-262).
 *   in (all required): kind[B,nb] i32 (0 circle, otherwise hull), radius[B,nb] f64 (circles), verts_raw[B,nb,cap,2] f64 relative
 *       to the body's reference point in the reference's vertex order (slots >= nverts are never read), nverts[B,nb] i32
 *       (hulls), mass[B,nb] f64; g: the gravity constant.  8 <= cap <= 64, else LCP_E_BADARG; B or nb of 0: success, no launch.
 *   out (each optional, NULL = skipped, at least one; written, never accumulated):
 *       centroid[B,nb,2] f64 (circle: 0), verts_local[B,nb,cap,2] f64 = verts_raw - centroid (slots >= nverts and circles: 0),
 *       inertia[B,nb] f64, Mdiag[B,nb,3] f32 = (I, m, m), f_gravity[B,nb,3] f32 = (0, 0, m g), status[B,nb] i32 (LCP_BODY_ST_*).
 * A flagged body still has every output written (possibly NaN); nothing is read beyond min(nverts, cap) vertices.
 * fp64 arithmetic; cap rounded up to a power of two lanes per body (8 bodies per wavefront at cap 8), sums by cross-lane
 * butterflies: the result of a body depends on its own inputs and cap only, not on its place in the batch. */
int lcp_body_properties_f64(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                            const int32_t* nverts, const double* mass, double g,
                            double* centroid, double* verts_local, double* inertia, float* Mdiag, float* f_gravity,
                            int32_t* status, void* stream);

/* Backward of lcp_body_properties_f64: what the reference's autograd gives the raw vertices handed to Hull (through the centroid
 * bodies.py:216-226, the recentred vertices :171 and the inertia :179-189), Circle.rad (:125-126) and the mass (:44-47,
 * forces.py:67).  Same raw inputs (all required), centroid and recentred vertices are recomputed: no saved state.
 *   cotangents in (each optional, NULL = zero): g_centroid[B,nb,2] f64, g_verts_local[B,nb,cap,2] f64 (slots >= nverts are not
 *       read), g_inertia[B,nb] f64, g_Mdiag[B,nb,3] f32, g_f[B,nb,3] f32.
 *   out (each optional, at least one; written, never accumulated): g_verts_raw[B,nb,cap,2] f64 (slots >= nverts and circles:
 *       0), g_radius[B,nb] f64 (hulls: 0), g_mass[B,nb] f64.
 * |cross| differentiates to its sign.  Same sizes, mapping and error codes as the forward. */
int lcp_body_properties_backward_f64(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                                     const int32_t* nverts, const double* mass, double g,
                                     const double* g_centroid, const double* g_verts_local, const double* g_inertia,
                                     const float* g_Mdiag, const float* g_f,
                                     double* g_verts_raw, double* g_radius, double* g_mass, void* stream);

/* ---- drawing: frames and segmentation masks of every scene, differentiable ----
 * What Body.draw paints (physics/bodies.py:140-150 circles, :237-250 hulls: pixel = pos * pixels_per_meter, x to the right, y
 * downward, thickness 0 = filled, > 0 = an outline) in the order of the paint loop of run_world (world.py:279-280: list order,
 * later over earlier), for B scenes in one launch (lcp_render.hip) - what Recorder (utils.py:54-72) and
 * run_world(screen=, recorder=) (world.py:246-320) need of the world state, as tensors.  Not drawn: a hull of fewer than three
 * vertices.  The circle's spoke, the hull's centre dot, the rect's diagonals and the joints' markers: lcp_render_marks_f64 below.
 *   camera: H x W pixels, pixel (i, j) sampled at x = (x0 + (j + 1/2) / ppm, y0 + (i + 1/2) / ppm); w > 0: the width of the edge
 *       ramp in world units (one pixel: 1 / ppm).
 *   signed distance d_k(x): circle |x - c| - r; hull with w_i = c + R(rot) v_i (utils.py:105-112), e_i = w_i+1 - w_i,
 *       n_i = left_orthogonal(e_i) / |e_i| (contacts.py:229-231), h_i = n_i . (x - w_i), m = max h_i: d = m where m <= 0, else
 *       the distance to the nearest edge segment.  cov(d) = clamp(1/2 - d / w, 0, 1); alpha_k = cov(d_k) for thickness_k == 0,
 *       cov(d_k) - cov(d_k + thickness_k) for thickness_k > 0.
 *   in: kind[B,nb] i32, radius[B,nb] f64, verts_local[B,nb,nvcap,2] f64 (slots >= nverts are never read), nverts[B,nb] i32,
 *       p[B,nb,3] f64 (rot, x, y), colors[B,nb,C] f32, background[C] f32 - all required; thickness[B,nb] f64, NULL = all filled.
 *   out (each optional, at least one; written, never accumulated):
 *       image[B,C,H,W] f32: I = background, then I = I (1 - alpha_k) + alpha_k colors[b,k] for k = 0 .. nb-1;
 *       ids[B,H,W] i32: the largest k with d_k <= 0 (the filled silhouette, whatever the thickness), or -1.
 * Sizes: 1 <= nb <= 64, 8 <= nvcap <= 64, 0 <= scene_verts_max <= 1024 (as lcp_move_find_contacts_nv_f64; a scene with more hull
 * vertices than scene_verts_max is not drawn: background and -1), B, H, W >= 1, 1 <= C <= 4, B C H W < 2^31, w > 0, ppm > 0 -
 * anything else is LCP_E_BADARG before any launch.  fp64 arithmetic.  One workgroup per (scene, tile of 16 x 64 pixels); a body
 * whose bounding circle grown by w / 2 misses the tile is skipped, where its alpha is exactly 0.  No allocation, no
 * synchronisation, no global state. */
int lcp_render_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C,
                   const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                   const double* p, const float* colors, const float* background, const double* thickness,
                   double x0, double y0, double ppm, double w,
                   float* image, int32_t* ids, void* stream);

/* Backward of the image of lcp_render_f64: what autograd gives the pose, Circle.rad, Hull.verts and the colours when the
 * drawing of Body.draw (bodies.py:140-150, 237-250) in the order of world.py:279-280 is written as tensor operations.  Same
 * inputs and checks; nothing is saved by the forward, the compositing state is recomputed per pixel.
 *   in: g_image[B,C,H,W] f32 (required).
 *   out (each optional, at least one; written, never accumulated): g_p[B,nb,3] f64, g_radius[B,nb] f64 (hulls: 0),
 *       g_verts_local[B,nb,nvcap,2] f64 (body frame; circles and slots >= nverts: 0), g_colors[B,nb,C] f32.
 * cov differentiates to -1 / w strictly inside its ramp and to 0 elsewhere; at |x - c| = 0 the circle's direction is 0.
 * One workgroup per (scene, body) over the body's pixel box, clamped to the image in floating point; sums in a fixed order, no
 * atomics: two runs give the same bits. */
int lcp_render_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C,
                            const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                            const double* p, const float* colors, const float* background, const double* thickness,
                            double x0, double y0, double ppm, double w, const float* g_image,
                            double* g_p, double* g_radius, double* g_verts_local, float* g_colors, void* stream);

/* The same frames with the marks Body.draw puts on the bodies and the joints' markers, the rest of run_world's paint loop
 * (world.py:279-282), in one launch (lcp_render_marks.hip).  Every convention of lcp_render_f64 holds: pixel centres, cov, the
 * compositing I = I (1 - alpha) + alpha colour back to front, fp64 arithmetic, fp32 image.  A frame is an ordered list of LAYERS:
 * the bodies' are exactly those of lcp_render_f64, the new ones are built from two primitives:
 *   segment (A, B, width s): d = dist(x, segment AB) - s / 2, alpha = cov(d).  A == B is the point A: the projection parameter is
 *       0 and nothing is divided by |AB|^2.  Where dist = 0 the direction dd/dx is 0 (as at a circle's centre).
 *   disc / ring (A, radius r, thickness t): d = |x - A| - r; filled: alpha = cov(d); ring: alpha = cov(d) - cov(d + t).
 * Body marks, mark[B,nb] i32 (NULL: none), colours mark_colors[B,nb,C] f32 (required with mark):
 *       0 none
 *       1 SPOKE      segment c -> c + rad (cos rot, sin rot), width line_w            circles only        bodies.py:144-147
 *       2 CENTRE     filled disc at c, radius dot_r                                   any kind            bodies.py:245-247
 *       3 DIAGONALS  segments w0 - w2 and w1 - w3 of the world vertices, width line_w hulls, nverts == 4  bodies.py:295-296
 *   A code that does not fit its body (a spoke on a hull, diagonals on a hull of nverts != 4, any other code) is not drawn:
 *   alpha = 0 and no gradient.
 * Joint markers, painted after all bodies, joint 0 first; jtype, jb1, jb2 [B,nj] i32, jr1, jrot1 [B,nj] f64 (the layout of
 * lcp_joint_jacobian_f64, read per scene), joint_colors[B,nj,C] f32; 0 <= nj <= 64, every joint pointer may be NULL when nj == 0:
 *       JOINT   filled disc, radius dot_r, at c_b1 + jr1 (cos jrot1, sin jrot1)                      constraints.py:44-53
 *       FIXED   segment c_b1 -> c_b2, width joint_w; not drawn when jb2 < 0                          constraints.py:89-92
 *       YCON    horizontal tick c_b1 -+ (joint_r, 0), width joint_w                                  constraints.py:117-119
 *       XCON    vertical tick c_b1 -+ (0, joint_r), width joint_w                                    constraints.py:144-146
 *       ROTCON  ring at c_b1, radius joint_r, thickness line_w                                       constraints.py:171-173
 *       TOTAL   that ring, then the horizontal tick, then the vertical tick                          constraints.py:202-206
 *   A joint of any other type, or whose body index lies outside [0, nb), is not drawn.  The lengths are world lengths (the
 *   reference's pixel constants divided by pixels_per_meter: line_w 1, dot_r 2, joint_w 2, joint_r 5 pixels).
 * order = 0, the reference's: for each body k its SPOKE or DIAGONALS under body k, then body k, then its CENTRE over it; then the
 *       joints.  order = 1: for each body k the body, then its mark whatever the code; then the joints (a filled body hides a
 *       mark painted under it, as pygame would).
 * ids is unchanged by marks and markers: the topmost filled body silhouette.
 * Not reproduced: the reference's one-pixel offset of the TOTAL marker's ring (constraints.py:203); its integer pixel rounding
 * of every coordinate; a hull of fewer than three vertices (its CENTRE mark is drawn).
 * Sizes and checks of lcp_render_f64, and: 0 <= nj <= 64, order in {0, 1}, line_w > 0, joint_w > 0, dot_r >= 0, joint_r >= 0,
 * mark_colors with mark, every joint array with nj > 0 - anything else is LCP_E_BADARG before any launch.  The tile mapping of
 * lcp_render_f64; every layer is culled by a bounding circle grown by w / 2 and the rounding slack, where its alpha is exactly 0.
 * No allocation, no synchronisation, no global state. */
int lcp_render_marks_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C,
                         const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                         const double* p, const float* colors, const float* background, const double* thickness,
                         double x0, double y0, double ppm, double w,
                         const int32_t* mark, const float* mark_colors,
                         int nj, const int32_t* jtype, const int32_t* jb1, const int32_t* jb2, const double* jr1, const double* jrot1,
                         const float* joint_colors,
                         int order, double line_w, double dot_r, double joint_w, double joint_r,
                         float* image, int32_t* ids, void* stream);

/* Backward of the image of lcp_render_marks_f64.  Same inputs and checks; nothing is saved by the forward.
 *   in: g_image[B,C,H,W] f32 (required).
 *   out (each optional, at least one; written, never accumulated): g_p[B,nb,3] f64, g_radius[B,nb] f64 (hulls: 0),
 *       g_verts_local[B,nb,nvcap,2] f64 (body frame; circles and slots >= nverts: 0), g_colors[B,nb,C] f32,
 *       g_mark_colors[B,nb,C] f32 (undrawn marks: 0), g_joint_colors[B,nj,C] f32, g_jrot1[B,nj] f64, g_jr1[B,nj] f64 (joints other
 *       than JOINT: 0).
 *   workspace: g_p_joints[B,nj,2,3] f64, required when g_p is asked for and nj > 0 (LCP_E_BADARG without it): every joint's pull
 *       on its two bodies, written by the first launch and added to g_p, body by body in joint order, by a second one.
 * The spoke reaches rot, c and radius; the diagonals verts_local, rot and c; the centre dot c; the markers the positions of jb1 /
 * jb2, jrot1 and jr1.  One workgroup per (scene, body) owns the body and its mark over the group's pixel box, one per (scene, joint)
 * the joint's marker over its own, in ONE launch; the second launch (one thread per body) only when g_p is asked for and nj > 0.
 * No atomics, sums in a fixed order: two runs give the same bits. */
int lcp_render_marks_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C,
                                  const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                                  const double* p, const float* colors, const float* background, const double* thickness,
                                  double x0, double y0, double ppm, double w,
                                  const int32_t* mark, const float* mark_colors,
                                  int nj, const int32_t* jtype, const int32_t* jb1, const int32_t* jb2, const double* jr1,
                                  const double* jrot1, const float* joint_colors,
                                  int order, double line_w, double dot_r, double joint_w, double joint_r,
                                  const float* g_image,
                                  double* g_p, double* g_radius, double* g_verts_local, float* g_colors, float* g_mark_colors,
                                  float* g_joint_colors, double* g_jrot1, double* g_jr1, double* g_p_joints, void* stream);

/* ---- range sensors: rays cast against every scene's geometry, differentiable ----
 * A fan of rays mounted on a body (or on the world frame), each returning the distance to the first surface it meets, for B scenes
 * in one launch (lcp_sensors.hip).  The scene inputs, their limits and the world vertices w_i, edges e_i = w_i+1 - w_i and outward
 * normals n_i are exactly those of lcp_render_f64 (utils.py:105-112, contacts.py:229-231); a scene with more hull vertices than
 * scene_verts_max is not sensed (every ray misses), a hull of fewer than three vertices is never hit.
 *   rays, R per scene: ray_body[B,R] i32 (the mounting body m; -1: the world frame; any other value outside [0, nb): the ray misses),
 *       ray_origin[B,R,2] f64 and ray_angle[B,R] f64 in the mounting frame, ray_range[B,R] f64 > 0.
 *       o = c_m + R(rot_m) origin, u = (cos, sin)(rot_m + angle); world frame: o = origin, the angle as it is.  A ray never tests its
 *       own mounting body.
 *   per body k:
 *       circle  q = o - c, b = q . u, cc = q . q - r^2.  cc <= 0: s = 0 (the origin inside or on it).  Otherwise a miss if b >= 0 or
 *               b^2 - cc < 0; otherwise s = -b - sqrt(b^2 - cc), n = (o + s u - c) / r.
 *       hull    h_i = n_i . (o - w_i), den_i = n_i . u.  All h_i <= 0: s = 0 (inside).  An edge with den_i == 0 and h_i > 0: a miss.
 *               s_in = max of -h_i / den_i over the edges with den_i < 0 (the first i on ties), s_out = min of -h_i / den_i over those
 *               with den_i > 0.  A hit iff 0 <= s_in <= s_out: s = s_in, n = that edge's normal, t = (o + s u - w_i) . e_i / |e_i|^2.
 *   per ray: the smallest s_k, on ties the smallest k.  None, or s >= ray_range: dist = ray_range, hit = -1, normal = 0.
 *   out (each optional, at least one; written, never accumulated): dist[B,R] f64, hit[B,R] i32, normal[B,R,2] f64 (0 for a miss and
 *       for s = 0).
 * Sizes: those of lcp_render_f64 (1 <= nb <= 64, 8 <= nvcap <= 64, 0 <= scene_verts_max <= 1024), 1 <= R <= 1024, B >= 0; a NULL
 * scene or ray array, no output - anything else is LCP_E_BADARG before any launch.  B == 0: success, no launch.  fp64 arithmetic.  One
 * workgroup per (scene, 256 rays), lane = ray; a body whose bounding circle none of a wavefront's rays can reach within their range is
 * skipped by that wavefront, where the rule gives a miss or s >= ray_range.  No allocation, no synchronisation, no global state. */
int lcp_cast_rays_f64(int B, int nb, int nvcap, int scene_verts_max, int R,
                      const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                      const int32_t* ray_body, const double* ray_origin, const double* ray_angle, const double* ray_range,
                      double* dist, int32_t* hit, double* normal, void* stream);

/* Backward of dist of lcp_cast_rays_f64.  Same inputs and checks; nothing is saved by the forward, every ray's hit is recomputed.
 *   in: g_dist[B,R] f64 (required).
 *   out (each optional, at least one; written, never accumulated): g_p[B,nb,3] f64, g_radius[B,nb] f64 (hulls: 0),
 *       g_verts_local[B,nb,nvcap,2] f64 (body frame; circles and slots >= nverts: 0), g_ray_origin[B,R,2] f64, g_ray_angle[B,R] f64.
 * A hit with 0 < s < ray_range differentiates by
 *       ds = (n . dX + dr - n . (do + s du)) / (n . u)
 *   dX: the motion of the material surface point - a circle: dc; a hull: (1 - t) dw_i + t dw_i+1 with
 *       dw = dc + drot perp(w - c) + R(rot) dv_local;  dr: the circle's radius (a hull: 0);
 *   do = dc_m + drot_m perp(o - c_m) + R(rot_m) d(origin),  du = (drot_m + d(angle)) perp(u),  perp(x, y) = (-y, x).
 * Misses, rays clamped at their range and hits with s = 0 have zero gradient.  A body collects from every ray that hits it and from
 * every ray mounted on it: one workgroup per scene, the rays' terms staged in LDS, every body owned by one wavefront that sums over
 * the rays in order - no atomics, two runs give the same bits. */
int lcp_cast_rays_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int R,
                               const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                               const double* p,
                               const int32_t* ray_body, const double* ray_origin, const double* ray_angle, const double* ray_range,
                               const double* g_dist,
                               double* g_p, double* g_radius, double* g_verts_local, double* g_ray_origin, double* g_ray_angle,
                               void* stream);

/* ---- proximity queries: the signed distance between body pairs, differentiable ----
 * How far apart two bodies are - negative when they overlap - with the unit normal from the first towards the second and a witness
 * point on either surface, for P pairs per scene and B scenes in one launch (lcp_proximity.hip).  Where the contact list has a record
 * (within eps of touching) dist is minus the largest penetration of the pair's records; the query continues it to pairs that are
 * apart.  The scene inputs, their limits and the world vertices w_i, edges e_i = w_i+1 - w_i and outward unit normals n_i are exactly
 * those of lcp_render_f64 / lcp_cast_rays_f64.  no_contact is not consulted: a query is explicit.
 *   pairs, P per scene: pair_first[B,P] i32 (body 1), pair_second[B,P] i32 (body 2), pair_max_dist[B,P] f64 > 0 (+inf allowed).
 *   per pair: dist, n (unit, from body 1 towards body 2), w1 on body 1's surface, w2 on body 2's, world frame; dist = n . (w2 - w1).
 *       circle - circle   q = c2 - c1, dist = |q| - r1 - r2, n = q / |q| (0 when |q| == 0), w1 = c1 + r1 n, w2 = c2 - r2 n.
 *       circle 1 - hull 2 (d, edge, t, u) = the signed distance of hull 2 at c1 with its derivative data: outside, the nearest edge
 *               (the smallest squared point-to-segment distance, the first on ties) with t clamped to [0, 1] and u = (c1 - foot) / d;
 *               inside (max_i h_i <= 0, h_i = n_i . (c1 - w_i)) the edge of largest h_i, the first i on ties, u = n_i, d = h_i, t =
 *               (c1 - w_i) . e_i / |e_i|^2 unclamped.  dist = d - r1, n = -u, w1 = c1 - r1 u, w2 = c1 - d u.
 *       hull 1 - circle 2 the mirror image with n = u.
 *       hull A (1) - hull B (2)   sep_A = max_i min_j n^A_i . (b_j - a_i), the first i on ties of the max and the first j on ties of
 *               the min; sep_B likewise with the roles swapped.
 *               max(sep_A, sep_B) <= 0 (overlapping or touching): dist is that maximum; A's face wins when sep_A >= sep_B.  A's face i
 *                   with its support vertex b_j: n = n^A_i, w2 = b_j, w1 = b_j - dist n, t = (b_j - a_i) . e_i / |e_i|^2 (unclamped);
 *                   B's face j with a_i: n = -n^B_j, w1 = a_i, w2 = a_i + dist n, t on B's edge.
 *               otherwise (apart): dist is the smallest point-to-segment distance over two sets, in this order: every b_j against every
 *                   edge i of A (i outer, j inner), then every a_i against every edge j of B (j outer, i inner); squared distances
 *                   are compared and a strict < keeps the first on ties.  The witness on the edge's body is the foot point at the
 *                   clamped t, the witness on the other body is the vertex, n = (w2 - w1) / dist.  dist > 0 here.
 *   invalid: pair_first == pair_second, an index outside [0, nb), or a hull of fewer than three vertices: dist = max_dist.
 *   clamp:   any dist >= max_dist is returned as max_dist with n = w1 = w2 = 0 and no gradient.
 *   cull:    a pair whose bounding circles (the staged ones, which only over-estimate) are max_dist or more apart is not evaluated;
 *            its true distance is at least max_dist too, so no result depends on the cull.
 *   a scene with more hull vertices than scene_verts_max is not queried: every pair returns max_dist.
 *   out (each optional, at least one; written, never accumulated): dist[B,P] f64, normal[B,P,2] f64, w1[B,P,2] f64, w2[B,P,2] f64.
 * Sizes: those of lcp_cast_rays_f64 (1 <= nb <= 64, 8 <= nvcap <= 64, 0 <= scene_verts_max <= 1024), 1 <= P <= 1024, B >= 0; a NULL
 * scene or pair array, no output - anything else is LCP_E_BADARG before any launch.  B == 0: success, no launch.  fp64 arithmetic.
 * One workgroup per (scene, 256 pairs), lane = pair, the cull decided before the pair's loops.  No allocation, no synchronisation, no
 * global state. */
int lcp_pair_distance_f64(int B, int nb, int nvcap, int scene_verts_max, int P,
                          const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                          const double* p,
                          const int32_t* pair_first, const int32_t* pair_second, const double* pair_max_dist,
                          double* dist, double* normal, double* w1, double* w2, void* stream);

/* Backward of dist of lcp_pair_distance_f64.  Same inputs and checks; nothing is saved by the forward, every pair is recomputed.
 *   in: g_dist[B,P] f64 (required).
 *   out (each optional, at least one; written, never accumulated): g_p[B,nb,3] f64, g_radius[B,nb] f64 (hulls: 0),
 *       g_verts_local[B,nb,nvcap,2] f64 (body frame; circles and slots >= nverts: 0).
 * A pair with dist < max_dist differentiates by
 *       d(dist) = n . (dW2 - dW1) - dr1 - dr2
 *   dW: the motion of the material witness point - a circle: dc; a hull's vertex: dw; a point of a hull's edge: (1 - t) dw_i + t dw_i+1
 *       with dw = dc + drot perp(w - c) + R(rot) dv_local, perp(x, y) = (-y, x);  dr: a circle's radius (a hull: 0).
 * Invalid, culled and clamped pairs have zero gradient.  One workgroup per scene, the pairs' terms staged in LDS behind the scene
 * (48 bytes a pair), every body owned by one wavefront that sums over the pairs in order - no atomics, two runs give the same bits. */
int lcp_pair_distance_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int P,
                                   const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                                   const double* p,
                                   const int32_t* pair_first, const int32_t* pair_second, const double* pair_max_dist,
                                   const double* g_dist,
                                   double* g_p, double* g_radius, double* g_verts_local, void* stream);

/* ---- overlap queries: the area of the intersection of body pairs, differentiable ----
 * How much two bodies overlap, as an area, for P pairs per scene and B scenes in one launch (lcp_overlap.hip).  The area of the
 * intersection of two convex shapes is C1 in the pose, 0 where the bodies are apart, and grows smoothly from the first touch;
 * lcp_pair_distance_f64 answers an overlapping pair with the depth of one feature pair, which is only piecewise smooth.  The scene
 * inputs, their limits and the world vertices w_i, edges e_i = w_i+1 - w_i and outward unit normals n_i are exactly those of
 * lcp_pair_distance_f64, and so are the pairs: pair_first[B,P] i32 (body 1), pair_second[B,P] i32 (body 2).  The pair set's cutoff
 * (pair_max_dist) is not an argument and is not consulted: an area needs none.  no_contact is not consulted.
 *   per pair: area[B,P] f64 >= 0, the area of body 1 n body 2 (a sum that rounds below 0 is returned as 0).
 *       circle - circle   d = |c2 - c1|.  d >= r1 + r2: 0.  d <= |r1 - r2|: pi min(r1, r2)^2.  Otherwise the lens
 *               r1^2 acos((d^2 + r1^2 - r2^2) / (2 d r1)) + r2^2 acos((d^2 + r2^2 - r1^2) / (2 d r2))
 *                   - sqrt((-d + r1 + r2)(d + r1 - r2)(d - r1 + r2)(d + r1 + r2)) / 2,  the acos arguments clamped to [-1, 1].
 *       hull A (1) - hull B (2)   Green's theorem over the pieces of either boundary that lie inside the other shape; no intersection
 *               polygon is built.  Every edge a_i + t e_i of A is clipped against B's half-planes h_j(x) = n^B_j . (x - b_j)
 *               (Cyrus-Beck), starting from [t0, t1] = [0, 1], and a piece that is left adds cross(p - o, q - o) / 2 = (t1 - t0)
 *               cross(a_i - o, e_i) / 2 with p = a(t0), q = a(t1) and o = c1, body 1's centre: the terms stay of the bodies' own size
 *               at coordinates of several hundred.  Then B's edges against A's half-planes.  The terms are about c1, not about the
 *               overlap, so pieces of the two boundaries that cancel or complement each other have to end in the same point; what
 *               an edge i of A and an edge j of B have to do with each other is therefore formed ONCE, in one way, whichever of the
 *               two is being clipped:
 *                   c = cross(e_i, e^B_j) (two rounded products, no fused multiply-add);  h = n^B_j . (a_i - b_j);
 *                   parallel: |c| <= 1e-12 |e_i| |e^B_j|;  eps = 64 * 2^-52 (|a_i.x| + |a_i.y| + |b_j.x| + |b_j.y|).
 *               Not parallel: the two lines cross at X = a_i + tx e_i, tx = -h / (c / |e^B_j|).  A's edge: c > 0: t1 = min(t1, tx),
 *                   c < 0: t0 = max(t0, tx).  B's edge: t = (X - b_j) . e^B_j / |e^B_j|^2; c > 0: t0 = max(t0, t), c < 0: t1 = min(t1, t).
 *               Parallel (h stands for the whole edge): A's edge is out when h > eps, and when |h| <= eps and e_i . e^B_j <= 0 (the
 *                   edges lie on one line and run against each other: the bodies touch from outside there).  B's edge is out unless it
 *                   lies strictly inside A's half-plane: unless h > eps when e_i . e^B_j > 0, unless h < -eps otherwise.
 *               A's edge is out when t0 > t1 (closed), B's when t0 >= t1 (open).  Of two edges on one line that run in the same
 *               direction exactly one is counted - a body inside another with an edge on one of its edges, two identical bodies at
 *               one pose - and of two that run against each other both or none, at any rotation.  Within the two bands the area is
 *               off by at most eps or 1e-12 |e| times the edge's length (1e-9 at edges of 30 and coordinates of 500); it is
 *               continuous across them to the same amount.
 *       circle - hull, in either order   the sum over the hull's edges: u = w_i - c, the edge u + t e_i split at its crossings of the
 *               circle, the roots in (0, 1) of |u + t e_i|^2 = r^2, used only when the discriminant is > 0.  A piece whose midpoint
 *               is within r (<=) adds cross(p, q) / 2, a piece outside adds r^2 atan2(cross(p, q), p . q) / 2 (p, q its ends).  When
 *               no piece of any edge is within r the area is pi r^2 if the centre lies in the hull (n_i . (c - w_i) <= 0 for every
 *               i) and exactly 0 otherwise.
 *   invalid: pair_first == pair_second, an index outside [0, nb), or a hull of fewer than three vertices: area = 0.
 *   cull:    a pair whose bounding circles (the staged ones, which only over-estimate) do not meet is not evaluated and returns
 *            exactly 0, which is what the rule gives it; no result depends on the cull.
 *   a scene with more hull vertices than scene_verts_max is not queried: every pair returns 0.
 *   out: area[B,P] f64, required; written, never accumulated.
 * Sizes: those of lcp_pair_distance_f64 (1 <= nb <= 64, 8 <= nvcap <= 64, 0 <= scene_verts_max <= 1024, 1 <= P <= 1024), B >= 0; a
 * NULL scene or pair array, no output - anything else is LCP_E_BADARG before any launch.  B == 0: success, no launch.  fp64
 * arithmetic.  One workgroup per (scene, 256 pairs), lane = pair, the cull decided before the pair's loops; a hull pair costs
 * 2 nA nB half-plane tests and no per-lane arrays.  No allocation, no synchronisation, no global state. */
int lcp_pair_overlap_f64(int B, int nb, int nvcap, int scene_verts_max, int P,
                         const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                         const double* p,
                         const int32_t* pair_first, const int32_t* pair_second,
                         double* area, void* stream);

/* Backward of lcp_pair_overlap_f64.  Same inputs and checks; nothing is saved by the forward, every pair is recomputed.
 *   in: g_area[B,P] f64 (required).
 *   out (each optional, at least one; written, never accumulated): g_p[B,nb,3] f64, g_radius[B,nb] f64 (hulls: 0),
 *       g_verts_local[B,nb,nvcap,2] f64 (body frame; circles and slots >= nverts: 0).
 * Only the pieces of a body's own boundary that lie inside the other body move the area:
 *       d(area) = sum over the pieces of  integral n . dW ds
 *   a piece [t0, t1] of a hull's edge i (the pieces of the forward):  |e_i| n_i . [((t1 - t0) - s) dw_i + s dw_i+1], s = (t1^2 - t0^2) / 2,
 *       with dw = dc + drot perp(w - c) + R(rot) dv_local, perp(x, y) = (-y, x), the material motion of "proximity queries";
 *   a circle against a hull: by translation invariance its centre receives minus what the pieces of the hull's edges within r give
 *       the hull's translation, -sum |e_i| n_i (t1 - t0); its radius r times the angle of its arc inside the hull, the sum of the
 *       atan2 terms of the pieces outside (2 pi when the whole circle lies in the hull);
 *   circle - circle (the lens): with alpha_k the acos of circle k and nhat = (c2 - c1) / d, d(area)/dc1 = chord nhat = -d(area)/dc2,
 *       chord = 2 r1 sin alpha_1, and d(area)/dr_k = 2 alpha_k r_k; one circle inside the other: 2 pi r for the smaller one (body 1
 *       when the radii are equal), nothing else.
 * The motion of the clip parameters cancels between the two pieces that meet in a crossing.  A pair whose bodies are apart has zero
 * gradient (the forward returns a sum that rounds below 0 as 0; the backward does not look at the sum).
 * Where a piece of one boundary lies exactly in the other's the area has a kink and this is one of its one-sided differentials.
 * One workgroup per scene; a body's gradient comes from its own boundary alone, so nothing per pair is staged: every body is owned by
 * one wavefront that takes the pairs the body is part of in pair order, lane = the body's edge (a circle: the partner's edge), and
 * sums in registers - no atomics, two runs give the same bits. */
int lcp_pair_overlap_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int P,
                                  const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                                  const double* p,
                                  const int32_t* pair_first, const int32_t* pair_second,
                                  const double* g_area,
                                  double* g_p, double* g_radius, double* g_verts_local, void* stream);

/* ---- point probes: the signed distance from query points to the scene, differentiable ----
 * How far a point is from the scene - negative inside a body - and from which body, for N points per scene and B scenes in one
 * launch (lcp_points.hip).  A point is mounted on a body (or on the world frame) and tests every other body or one target body.  The
 * scene inputs, their limits and the world vertices w_i, edges e_i = w_i+1 - w_i and outward unit normals n_i are exactly those of
 * lcp_render_f64 / lcp_cast_rays_f64; a scene with more hull vertices than scene_verts_max is not probed (every point is void), a
 * hull of fewer than three vertices is never a candidate.  no_contact is not consulted.
 *   points, N per scene: pt_body[B,N] i32 (the mounting body m; -1: the world frame; any other value outside [0, nb): the point is
 *       void), pt_xy[B,N,2] f64 in the mounting frame, pt_target[B,N] i32 (-1: every body is tested; k in [0, nb): body k alone; any
 *       other value: no candidate), pt_max_dist[B,N] f64 > 0 (+inf allowed).
 *       x = c_m + R(rot_m) xy; world frame: x = xy.  A point never tests its own mounting body: target == m gives no candidate.
 *   per candidate body k: (d_k, u_k, edge, t)
 *       circle  q = x - c, d = |q| - r, u = q / |q| (exactly 0 when |q| == 0).
 *       hull    the signed distance of the hull at x with its derivative data ("circle 1 - hull 2" above with r1 = 0): outside, the
 *               edge of smallest squared point-to-segment distance (the first on ties), t clamped to [0, 1], d = |x - foot|,
 *               u = (x - foot) / d; inside (max_i h_i <= 0, h_i = n_i . (x - w_i)) the edge of largest h_i (the first i on ties),
 *               d = h_i, u = n_i, t = (x - w_i) . e_i / |e_i|^2 unclamped.
 *   per point: the smallest d_k, on ties the smallest k.  None, or d >= pt_max_dist: dist = pt_max_dist, body = -1, normal = 0 - a
 *       void point, without a gradient.  Otherwise dist = d (negative inside), body = k, normal = u = d(dist)/dx.
 *   out (each optional, at least one; written everywhere, never accumulated): dist[B,N] f64, body[B,N] i32, normal[B,N,2] f64.
 * Sizes: those of lcp_cast_rays_f64 (1 <= nb <= 64, 8 <= nvcap <= 64, 0 <= scene_verts_max <= 1024), 1 <= N <= 1024, B >= 0; a NULL
 * scene or point array, no output - anything else is LCP_E_BADARG before any launch.  B == 0: success, no launch.  fp64 arithmetic.
 * One workgroup per (scene, 256 points), lane = point; a body whose bounding circle lies at or beyond min(the best distance so far,
 * pt_max_dist) for every point of a wavefront is skipped by that wavefront, where the rule gives no change: a finite cutoff leaves
 * the bits of every live point what +inf gives.  No allocation, no synchronisation, no global state. */
int lcp_point_distance_f64(int B, int nb, int nvcap, int scene_verts_max, int N,
                           const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                           const double* p,
                           const int32_t* pt_body, const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist,
                           double* dist, int32_t* body, double* normal, void* stream);

/* Backward of dist of lcp_point_distance_f64.  Same inputs and checks; nothing is saved by the forward, every point's selection is
 * recomputed.
 *   in: g_dist[B,N] f64 (required).
 *   out (each optional, at least one; written, never accumulated): g_p[B,nb,3] f64, g_radius[B,nb] f64 (hulls: exactly 0),
 *       g_verts_local[B,nb,nvcap,2] f64 (body frame; circles and slots >= nverts: exactly 0), g_pt_xy[B,N,2] f64 (mounting frame).
 * A live point differentiates by
 *       dd = u . (dx - dX) - dr
 *   dx = dc_m + drot_m perp(x - c_m) + R(rot_m) d(xy)   (world frame: d(xy)),  perp(x, y) = (-y, x);
 *   dX = dc_k (a circle; dr: its radius' change)
 *      = (1 - t) dw_i + t dw_i+1 with dw = dc_k + drot_k perp(w - c_k) + R(rot_k) dv_local   (a hull; dr = 0).
 * Inside a hull t is unclamped, which makes the face term exact: the normal's rotation contributes -t n . (dw_i+1 - dw_i).  Void
 * points have zero gradient.  A body collects from every point whose `body` it is and from every point mounted on it: one workgroup
 * per scene, the points' terms staged in LDS behind the scene (52 bytes a point), every body owned by one wavefront that sums over
 * the points in order - no atomics, two runs give the same bits.  g_pt_xy is the point's own. */
int lcp_point_distance_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int N,
                                    const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                                    const double* p,
                                    const int32_t* pt_body, const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist,
                                    const double* g_dist,
                                    double* g_p, double* g_radius, double* g_verts_local, double* g_pt_xy, void* stream);

/* ---- time of impact: when body pairs first touch along the engine's move, differentiable ----
 * A step accepts a move whose END pose does not penetrate; a body that travels more than an obstacle's thickness in one dt lands
 * beyond it without a record.  This query says when P pairs per scene first come within a margin of each other along the move, for
 * B scenes in one launch (lcp_toi.hip).  The scene inputs and their limits are those of lcp_pair_distance_f64.
 *   motion:  pose_b(t) = p_b + t (double)v_b in all three coordinates (bodies.py:80-82) for 0 <= t <= horizon; p[B,nb,3] f64 (rot, x,
 *            y), v[B,nb,3] f32 (w, vx, vy).  d(t): dist of lcp_pair_distance_f64 for the pair at pose(t), without a cutoff; n(t): its
 *            unit normal from body 1 towards body 2.
 *   pairs, P per scene: pair_first[B,P] i32, pair_second[B,P] i32, margin[B,P] f64 >= 0;  per scene: horizon[B] f64;
 *            tol > 0 (a distance), 1 <= max_iter <= 1024 (evaluations of d).
 *   conservative advancement: t_0 = 0; for k = 0, 1, ...
 *            d_k = d(t_k), n_k = n(t_k)
 *            d_k - margin <= tol:   TOUCHING with toi = 0 when k == 0, else HIT with toi = t_k
 *            a_k = -n_k . (vlin_2 - vlin_1) + |w_1| rho_1 + |w_2| rho_2     rho: 0 for a circle, max_j |verts_local_j| for a hull
 *            a_k <= 0:              MISS
 *            t_k+1 = t_k + (d_k - margin) / a_k;   t_k+1 >= horizon:  MISS
 *            after max_iter evaluations without an exit: UNCONVERGED, toi = the last evaluated t_k.
 *       Why no iterate passes the first touch: for separated convex bodies n_k is a separating direction - at t_k body 1 lies in
 *       {x : n_k . x <= s} and body 2 in {x : n_k . x >= s + d_k}.  Along n_k a point of body i moves at n_k . vlin_i plus at most
 *       |w_i| rho_i (it turns about the centre at a distance of at most rho_i; a circle's surface does not move when it turns).  So
 *       after s - t_k more time the gap between the two half planes, and with it the distance, is at least d_k - (s - t_k) a_k:
 *               d(s) >= d_k - (s - t_k) a_k   for every s >= t_k,
 *       which stays above margin until t_k+1.  By induction no t_k lies beyond the first time d reaches margin: a HIT has
 *       margin <= d <= margin + tol at a time no later than the first touch, an UNCONVERGED toi is a true lower bound of it, and a
 *       MISS (a_k <= 0: the gap cannot shrink; t_k+1 >= horizon) has no touch before the horizon.
 *   results: MISS returns toi = horizon.  status: LCP_TOI_MISS 0, LCP_TOI_HIT 1, LCP_TOI_TOUCHING 2, LCP_TOI_UNCONVERGED 3.
 *   invalid: pair_first == pair_second, an index outside [0, nb), or a hull of fewer than three vertices: MISS without evaluation.
 *   a scene with more hull vertices than scene_verts_max, or with a horizon that is <= 0 or NaN, is not queried: every pair is a MISS
 *            with toi = max(horizon, 0) (0 for a NaN), and first_toi is that value.
 *   cull:    a pair whose bounding circles (a circle's radius; a hull's rho about its centre) are at least
 *            margin + horizon (|vlin_2 - vlin_1| + |w_1| rho_1 + |w_2| rho_2) apart, and more than margin + tol, is a MISS without
 *            evaluation: then d_0 - margin > tol and t_1 >= horizon, the rule's own first iteration.  No result depends on the cull.
 *   out (each optional, at least one; written, never accumulated): toi[B,P] f64, status[B,P] i32, normal[B,P,2] f64 (n at toi for HIT
 *            and TOUCHING, else 0), and per scene first_toi[B] f64, first_pair[B] i32: the smallest toi over the pairs with status HIT
 *            or UNCONVERGED and its pair, the smallest pair index on ties; none: horizon and -1.  (TOUCHING pairs are left out on
 *            purpose: they are in the contact list already.)
 * Sizes: those of lcp_pair_distance_f64 (1 <= nb <= 64, 8 <= nvcap <= 64, 0 <= scene_verts_max <= 1024, 1 <= P <= 1024), B >= 0; a NULL
 * input array, no output, tol or max_iter outside their range - anything else is LCP_E_BADARG before any launch.  B == 0: success, no
 * launch.  fp64 arithmetic.  One workgroup per scene, lane = pair, 256 pairs at a time; staged in LDS is what does not move (the
 * body-frame vertices, rho, p, v), every evaluation turns the two bodies to the lane's own time.  No allocation, no synchronisation, no
 * global state. */
#define LCP_TOI_MISS 0
#define LCP_TOI_HIT 1
#define LCP_TOI_TOUCHING 2
#define LCP_TOI_UNCONVERGED 3
int lcp_time_of_impact_f64(int B, int nb, int nvcap, int scene_verts_max, int P,
                           const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                           const double* p, const float* v,
                           const int32_t* pair_first, const int32_t* pair_second, const double* margin, const double* horizon,
                           double tol, int max_iter,
                           double* toi, int32_t* status, double* normal, double* first_toi, int32_t* first_pair, void* stream);

/* Backward of toi of lcp_time_of_impact_f64.  The forward is iterative; the backward needs ONE evaluation, at pose(toi).
 *   in: the scene, v and the pairs as above; toi[B,P] f64 and status[B,P] i32 as the forward wrote them; g_toi[B,P] f64 (all required).
 *   out (each optional, at least one; f64, written everywhere, never accumulated): g_p[B,nb,3], g_v[B,nb,3], g_radius[B,nb] (hulls: 0),
 *       g_verts_local[B,nb,nvcap,2] (body frame; circles and slots >= nverts: 0), g_margin[B,P].
 * A pair is live when its status is HIT and ddot < 0, ddot = n . (V_2(W_2) - V_1(W_1)) with V_i(W) = vlin_i + w_i perp(W - c_i) the
 * velocities of the witness points W_1, W_2 of the distance rule at pose(toi), perp(x, y) = (-y, x).  From d(pose(toi)) = margin:
 *       d(toi) = (d(margin) - [n . (dW_2 - dW_1) - dr_1 - dr_2]) / ddot
 *   dW: as in lcp_pair_distance_backward_f64 but at the advanced pose: dW = dc + toi dvlin + (drot + toi dw) perp(W - c)
 *       + R(rot + w toi) dv_local (an edge's point: (1 - t) and t of it at the edge's two vertices).  So g_v is, pair by pair, toi times
 *       the pair's g_p terms.  Pairs that are not live give exactly 0 to every output.
 * One workgroup per scene, the live pairs' terms staged in LDS (104 bytes a pair), every body owned by one wavefront that walks the
 * pairs in order - no atomics, two runs give the same bits whichever outputs are asked for. */
int lcp_time_of_impact_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int P,
                                    const int32_t* kind, const double* radius, const double* verts_local, const int32_t* nverts,
                                    const double* p, const float* v,
                                    const int32_t* pair_first, const int32_t* pair_second,
                                    const double* toi, const int32_t* status, const double* g_toi,
                                    double* g_p, double* g_v, double* g_radius, double* g_verts_local, double* g_margin, void* stream);

/* ---- force elements: springs, motors and drag as a function of the state, differentiable ----
 * Forces that depend on the state of the scene - a spring or damper between two anchors, a PD servo on a relative angle, viscous
 * drag - for E elements per scene and B scenes in one launch (lcp_forces.hip), added onto an optional base force.
 *   state:   p[B,nb,3] f64 (rot, x, y); v[B,nb,3] f32 (w, vx, vy).  A wrench is (torque, fx, fy), the order of p and v.
 *            cross(a, b) = ax by - ay bx, perp(x, y) = (-y, x), R(rot) = [[cos, -sin], [sin, cos]] (utils.py:105-112).
 *   elements, [B,E] each (scenes may differ in every array): kind i32 (0 none, 1 spring, 2 motor, 3 drag), b1, b2 i32,
 *            a1, a2 [B,E,2] f64 (anchors), k, c, x0, w0, limit f64 (limit > 0, +inf allowed).
 *   spring / damper (1): either body may be -1, the world: its anchor is then in world coordinates and at rest.
 *            r_i = R(rot_i) a_i, P_i = c_i + r_i, V_i = (vx, vy)_i + w_i perp(r_i)       (the world: P_i = a_i, V_i = 0)
 *            d = P_2 - P_1, L = |d|, u = d / L, Ldot = u . (V_2 - V_1)
 *            s = k (L - x0) + c Ldot, clamped to [-limit, limit]
 *            body 1 receives (cross(r_1, s u), s u), body 2 (cross(r_2, -s u), -s u).  L == 0: no force, zero gradient.
 *   motor (2): a PD servo on the relative angle; b1 is the base, b2 the driven body; either may be -1 (the world: angle 0, at rest).
 *            th = rot_2 - rot_1 (no wrapping: rot accumulates), om = w_2 - w_1
 *            tau = k (x0 - th) + c (w0 - om), clamped to [-limit, limit]; +tau on b2's rotation, -tau on b1's.
 *   drag (3): body b1 receives (-c w, -k vx, -k vy); b2, the anchors, x0, w0 and limit are ignored (b2 is not even checked).
 *   invalid: kind 0 or unknown; spring or motor with an index outside [-1, nb) or b1 == b2 (which covers both ends the world);
 *            drag with b1 outside [0, nb).  An invalid element produces nothing and has zero gradient.
 *   a saturated element (|s| or |tau| >= limit) acts with +-limit and has zero gradient with respect to everything; limit has none.
 *   out: f_out[B,nb,3] f32 = f_base + the sum of the elements' wrenches on the body.  f_base[B,nb,3] f32 is optional (NULL: 0) and
 *            f_out may alias it.  Every entry is accumulated in fp64, starting from f_base, over the elements IN ELEMENT ORDER and
 *            rounded once at the store; a body that no element touches gets f_base's bits.
 * Sizes: 1 <= nb <= 64, 1 <= E <= 1024, B >= 0; a NULL element array, p, v or f_out - anything else is LCP_E_BADARG before any
 * launch.  B == 0: success, no launch.  A group of lanes per scene (the power of two >= max(nb, E), at most 256; several scenes share
 * a wavefront below 64), the elements' wrenches staged in LDS (40 bytes an element), every body's sum owned by one lane: no atomics,
 * two runs give the same bits.  No allocation, no synchronisation, no global state. */
int lcp_force_elements_f64(int B, int nb, int E,
                           const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1, const double* a2,
                           const double* k, const double* c, const double* x0, const double* w0, const double* limit,
                           const double* p, const float* v, const float* f_base, float* f_out, void* stream);

/* Backward of lcp_force_elements_f64.  Same inputs and checks; nothing is saved by the forward, every element is evaluated again.
 *   in: g_f[B,nb,3] f32 (required), the cotangent of f_out.  (The cotangent of f_base is g_f itself.)
 *   out (each optional, at least one; written everywhere, never accumulated; all f64): g_p[B,nb,3], g_v[B,nb,3], g_k, g_c, g_x0,
 *       g_w0 [B,E], g_a1, g_a2 [B,E,2].  Invalid and saturated elements and springs with L == 0: exactly 0.  A world-anchored end's
 *       g_a is the gradient of its world point.  A drag's k is its linear and c its angular coefficient.
 * Every body's sums are owned by one lane that walks the elements in order (staged 512 at a time, 72 bytes an element): no atomics,
 * two runs give the same bits, whichever outputs are asked for. */
int lcp_force_elements_backward_f64(int B, int nb, int E,
                                    const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1, const double* a2,
                                    const double* k, const double* c, const double* x0, const double* w0, const double* limit,
                                    const double* p, const float* v, const float* g_f,
                                    double* g_p, double* g_v, double* g_k, double* g_c, double* g_x0, double* g_w0,
                                    double* g_a1, double* g_a2, void* stream);

/* ---- mechanism links: rods, slots and sliders between bodies, differentiable ----
 * Equality rows that are a pure function of the pose, for L links per scene and B scenes in one launch (lcp_links.hip), written
 * below an optional block of base rows into ONE matrix Je[B, e0 + el, 3 nb] - what the step entries take as `Je`.  Every link is a
 * position-level function C(p) of the poses p = (rot, x, y); its rows are the exact gradient dC/dp, and the solvers hold Je v = 0.
 *   pose:    p[B,nb,3] f64.  cross(a, b) = ax by - ay bx, perp(x, y) = (-y, x), R(rot) = [[cos, -sin], [sin, cos]].
 *   links, [B,L] each (bodies, anchors and angles may differ per scene; the kinds are expected to be the same list in every scene):
 *            kind i32 (0 none, 1 distance, 2 slot, 3 prismatic), first i32 in [0, nb), second i32 in [-1, nb) (-1: the world),
 *            a1, a2 [B,L,2] f64 (anchors in the bodies' frames; the world's is a world point), phi f64.
 *            r_k = R(rot_k) a_k, w_k = c_k + r_k; the world: w_2 = a_2, rot_2 = 0, no columns.
 *   distance (1), 1 row:  C = |w_2 - w_1| - length, n = (w_2 - w_1) / |w_2 - w_1|
 *            columns of first (-cross(r_1, n), -n_x, -n_y), of second (cross(r_2, n), n_x, n_y); |w_2 - w_1| < 1e-12: a row of zeros.
 *   slot (2), 1 row: first's anchor stays on a line fixed in second.  d = w_1 - w_2, t = R(rot_2) (-sin phi, cos phi), C = t . d
 *            columns of first (cross(r_1, t), t_x, t_y), of second (-cross(r_2 + d, t), -t_x, -t_y).
 *   prismatic (3), 2 rows: the slot's row, then rot_1 - rot_2 - const: (1, 0, 0) and (-1, 0, 0).
 *   A link's first row is e0 + the rows of the links before it in ITS scene; a link whose rows would pass `el` is dropped.  kind 0 or
 *   unknown: no rows.  A link with an index out of range or first == second keeps its rows, all zero.  Rows no link fills are zero.
 *   out: Je[B, e0 + el, 3 nb] f32, every element written once: rows [0, e0) are Je_base's bits (Je_base[B,e0,3 nb] f32, required when
 *            e0 > 0, must not overlap Je), link rows are exact zeros but for the six entries, computed in fp64 and rounded once.
 * Sizes: 1 <= nb <= 64, 1 <= L <= 256, 0 <= e0 <= 65536 (LCP_E_TOOLARGE beyond the upper limits), 0 <= el <= 2 L, B >= 0; a NULL link
 * array, p or Je, Je_base NULL with e0 > 0 - anything else is LCP_E_BADARG before any launch.  B == 0 or e0 + el == 0: success, no
 * launch.  A group of lanes per scene (the power of two >= max(nb, L); several scenes share a wavefront below 64), the entries staged
 * per row in LDS (32 bytes a row), the matrix stored by the whole workgroup with consecutive addresses.  No allocation, no
 * synchronisation, no global state. */
int lcp_link_jacobian_f64(int B, int nb, int L, int e0, int el,
                          const int32_t* kind, const int32_t* first, const int32_t* second,
                          const double* a1, const double* a2, const double* phi,
                          const double* p, const float* Je_base, float* Je, void* stream);

/* Backward of the LINK rows of lcp_link_jacobian_f64 (the cotangent of the base rows is gJe's first e0 rows: the caller's slice).
 * Same inputs and checks; nothing is saved by the forward.
 *   in: gJe[B, e0 + el, 3 nb] f32 (required), the cotangent of Je.
 *   out (each optional, at least one; written everywhere, never accumulated; all f64): g_p[B,nb,3], g_a1, g_a2 [B,L,2], g_phi[B,L].
 *       It includes the derivative of n (distance) and of t and d (slot).  A slot's row does not depend on a2; a distance on phi; the
 *       second row of a prismatic link is constant.  Links that wrote zeros or nothing: exactly 0.  A body no link names: exactly 0.
 * Every body's sum is owned by one lane that walks the links in order (staged in LDS, 40 bytes a link): no atomics, two runs give
 * the same bits, whichever outputs are asked for. */
int lcp_link_jacobian_backward_f64(int B, int nb, int L, int e0, int el,
                                   const int32_t* kind, const int32_t* first, const int32_t* second,
                                   const double* a1, const double* a2, const double* phi,
                                   const double* p, const float* gJe,
                                   double* g_p, double* g_a1, double* g_a2, double* g_phi, void* stream);

/* ---- contact reports: the impulses of a solve per body, per body pair and per joint ----
 * Which bodies touch and how hard, from the multipliers a solve wrote (z, y of lcp_solve_dynamics_f32 / lcp_step_fused_f32) and the
 * contact records it consumed, for B scenes in one launch (lcp_report.hip).  The reference's residual is
 * rx = A^T y + G^T z + Q x + p (lcp/solvers/pdipm.py:82-85) with Q = M, p = M v + dt f, x = -new_v, A = Je and G = [Jc; Jf; 0]
 * (physics/engines.py:31-32,52-76), so at a solution
 *            M (v_new - v) - dt f  =  G^T z  +  Je^T y
 * the first term the CONTACT impulse on every body coordinate, the second the JOINT impulse.  An impulse is (torque, x, y), the order
 * of p and v.  With the row blocks of physics/world.py:172-211, cross_2d(a, b) = ax by - ay bx and left_orthogonal(n) = (ny, -nx)
 * (physics/utils.py:93-102), record c of a scene contributes
 *            zn = z[c], zt = z[maxc + 2c] - z[maxc + 2c + 1], n = c_n[c], d = left_orthogonal(n), j = zn n + zt d
 *            body c_i1[c] receives (cross_2d(c_p1[c], j), j), body c_i2[c] receives (-cross_2d(c_p2[c], j), -j).
 *   in:  the records c_n, c_p1, c_p2 [B,maxc,2] f32, c_i1, c_i2 [B,maxc] i32; z [B,4 maxc] f32; c_count [B] i32 or NULL (every scene has
 *        maxc records: the fused step); active [B] i32 or NULL (all active).  A scene's records are its first min(c_count, maxc); an
 *        inactive scene (active == 0) has none, and no joint impulse either.  y [B,e] f32 and Je [B,e,3 nb] f32: either NULL, or
 *        e == 0, leaves joint_impulse zero.  pair_first, pair_second [B,P] i32 (required when P > 0); min_impulse: the threshold of
 *        the two counts.
 *   out (each optional, at least one; written everywhere, never accumulated):
 *        body_impulse[B,nb,3] f32   what the body receives from all its contacts
 *        body_normal[B,nb] f32      the sum of zn over the records that name the body on either side (a record counts once)
 *        body_touching[B,nb] i32    how many of those records have (double)zn > min_impulse
 *        joint_impulse[B,nb,3] f32  sum_r Je[r, 3 b + q] y[r], rows in order
 *        pair_impulse[B,P,3] f32    what `first` receives from `second`: records with (i1, i2) = (first, second) give
 *                                   (cross_2d(c_p1, j), j), records with (i1, i2) = (second, first) give (-cross_2d(c_p2, j), -j);
 *                                   the torque is about `first`'s centre
 *        pair_normal[B,P] f32       the sum of zn over those records
 *        pair_contacts[B,P] i32     how many of them have (double)zn > min_impulse
 *   Every float sum is taken in fp64 in record (or row) order and rounded once at the store.  A record index outside [0, nb) gives
 *   nothing to that side; a pair with first == second or an index outside [0, nb) is all zeros.
 * Sizes: 1 <= nb <= 64, 1 <= maxc <= 1024, 0 <= P <= 1024, e >= 0 (LCP_E_TOOLARGE beyond the upper limits); B < 0, a size below its
 * lower limit, a NULL record array or z, a NULL pair array with P > 0, or no output at all are LCP_E_BADARG; a refusal writes nothing.
 * B == 0: success, no launch.  A group of lanes per scene (the power of two >= max(nb, min(maxc, 256)), at most 256; several scenes
 * share a wavefront below 64), the records' impulses staged in LDS (48 bytes a record), every output element owned by one lane: no
 * atomics, two runs give the same bits.  No allocation, no synchronisation, no global state. */
int lcp_contact_report_f32(int B, int nb, int maxc, int e, int P, const int32_t* c_count, const int32_t* active,
                           const float* c_n, const float* c_p1, const float* c_p2, const int32_t* c_i1, const int32_t* c_i2,
                           const float* z, const float* y, const float* Je,
                           const int32_t* pair_first, const int32_t* pair_second, double min_impulse,
                           float* body_impulse, float* body_normal, int32_t* body_touching, float* joint_impulse,
                           float* pair_impulse, float* pair_normal, int32_t* pair_contacts, void* stream);

/* ---- the breakout encoder: frames -> paddle, blocks and ball of every scene ----
 * What extract_params (experiments/breakout/encoder.py:63-133, with remove_rect :136-137 and get_pos_dims :140-145) reads off
 * an Atari Breakout frame, for B frames in one launch (lcp_encoder.hip).  The reference reads channel 0 only (`frame[..., 0]`):
 * the KEY PLANE k(i, j) = frame[b stride_b + i stride_row + j stride_col], bytes, every comparison on bytes.  "Removed" stands
 * for what the reference paints black (remove_rect) before it searches on.
 *   layout: a HOST pointer to LCP_ENC_LAYOUT_WORDS int32 words, copied into the kernel's arguments (defaults: encoder.py:28-52):
 *       [0] paddle_line 189  [1] paddle_h 4  [2] paddle_w 16  [3] paddle_key 200  [4] ball_w 2  [5] nrows 6 (0 .. 8)
 *       [6] band_top 57  [7] band_h 6  [8..15] row_key 200 198 180 162 72 66  [16..19] erase rect, inclusive corners (top, left,
 *       bottom, right) 189 152 194 160  [20] ball_key 200
 *   paddle (:67-82): px = the first column holding the maximum of row paddle_line; if k(paddle_line, px + ball_w + 1) !=
 *       paddle_key, the first column >= px + ball_w + 1 holding the maximum of the rest of the row (the ball can sit in that row,
 *       left of the paddle); r = the first column >= px that is not paddle_key (none, or r == px: W), at most px + paddle_w.
 *       Corners (paddle_line, px, paddle_line + paddle_h, r); removed: rows paddle_line .. paddle_line + paddle_h, columns
 *       px .. r, both inclusive, clipped.  px + ball_w + 1 >= W (the reference raises): the first px is kept,
 *       LCP_ENC_ST_PADDLE_PROBE.
 *   blocks (:91-101): band i has top = band_top + i band_h; the maximal runs [left, right) of k(top, .) == row_key[i], left to
 *       right, give corners (top, left, top + band_h, right) and remove rows top .. top + band_h - 1, columns left .. right - 1.
 *       A run that starts at column 0 ends the band's list: it and what follows it there are neither listed nor removed
 *       (`while left > 0`).  A run that reaches column W - 1 (the reference never returns) ends the band's list the same way:
 *       LCP_ENC_ST_RUN_AT_EDGE.  Order: by band, then left to right.  nblocks is the true total; the first max_blocks are
 *       stored, more set LCP_ENC_ST_TRUNCATED; the removal covers every listed run whatever max_blocks.
 *   erase rect (:104-105): removed, inclusive, clipped.
 *   ball (:107-121): (i, j) = the first pixel in raster order with k == ball_key that is not removed; right = the first column
 *       >= j of row i that is removed or not ball_key (none: j), bottom likewise down column j (none: i).  Corners (i, j, bottom,
 *       right).  No such pixel: LCP_ENC_ST_NO_BALL and zeros.
 *   in: frame (device) with stride_b, stride_row, stride_col > 0 in bytes (gym's [B,H,W,C]: stride_col = C; [B,C,H,W]: 1).  Of
 *       each row only the bytes from its first to its last key byte are read, nothing before or after; rows with stride_col <= 4
 *       are read as whole 16-byte lines (any alignment), other strides byte by byte.
 *   out (each optional, NULL = skipped, at least one; written, never accumulated): paddle[B,4] i32, blocks[B,max_blocks,4] i32
 *       (slots >= the count: 0), nblocks[B] i32, ball[B,4] i32, status[B] i32 (LCP_ENC_ST_*), and the get_pos_dims form
 *       (x, y, w, h) = ((right + left) / 2, (bottom + top) / 2, right - left, bottom - top) in f64: paddle_params[B,4],
 *       block_params[B,max_blocks,4] (slots >= the count: the reference's placeholder (1000, 60, 1, 1), run_breakout.py:56),
 *       ball_params[B,3] = (x, y, min(min(w, h) / 2, 1)), without a ball (W / 2, 100 H, 1) (:125-129).
 * LCP_E_BADARG before any launch: a NULL frame or layout, no output, B < 0, H outside 1 .. 2^20, W outside 1 .. 1024, max_blocks
 * outside 1 .. 256, a stride < 1, a key outside 1 .. 255, nrows outside 0 .. 8, band_h < 1, paddle_w < 1, paddle_h < 0, ball_w < 0,
 * paddle_line or band_top outside the image, band_top + nrows band_h > paddle_line, an erase rect with a negative or reversed
 * corner.  B == 0: success, no launch.  One workgroup of 256 threads per scene; no allocation, no synchronisation, no global
 * state, no atomics on global memory: two runs give the same bits. */
#define LCP_ENC_LAYOUT_WORDS 21
#define LCP_ENC_ST_NO_BALL       1  /* no pixel of ball_key is left once paddle, blocks and the erase rect are removed           */
#define LCP_ENC_ST_TRUNCATED     2  /* nblocks > max_blocks: the list is cut, nothing else                                         */
#define LCP_ENC_ST_RUN_AT_EDGE   4  /* a band's run reaches column W - 1: the reference loops forever (encoder.py:96-101)          */
#define LCP_ENC_ST_PADDLE_PROBE  8  /* px + ball_w + 1 >= W: the reference raises IndexError (encoder.py:69)                       */
int lcp_extract_params_u8(int B, int H, int W, const uint8_t* frame, int64_t stride_b, int64_t stride_row, int64_t stride_col,
                          const int32_t* layout, int max_blocks,
                          int32_t* paddle, int32_t* blocks, int32_t* nblocks, int32_t* ball, int32_t* status,
                          double* paddle_params, double* block_params, double* ball_params, void* stream);

/* ---- debugging / A-B aids (not part of the drop-in surface) ----
 * lcp_debug_set_trace: when non-NULL, the dense forward writes trace[B, max_iter, 4] =
 *   (resid, mu, sigma, alpha) per PDIPM iteration (device pointer to doubles).
 * lcp_debug_set_path : 0 = automatic kernel selection, 1 = generic (workgroup-per-scene) kernels only,
 *   2 = wave-per-scene kernels whenever the sizes allow (the default behaviour of 0 today),
 *   3 = contact-space factorisation everywhere: lcp_big.hip instead of lcp_primal.hip for 17..64 contacts, the 32-row reduced
 *       system instead of the body-space one in lcp_quad.hip's contact-list forward (the formulation of pdipm.py:325-454;
 *       same answers).  A forward and its backward must run under the same setting.
 *   4 = lcp_primal.hip (one wave per scene) also where lcp_quad.hip would serve (A/B: small batches).
 * Both settings are thread_local: they affect the calls of the thread that made them, nobody else's. */
void lcp_debug_set_trace(double* device_trace);
/* LCP_BWD_ADJOINT for lcp_pdipm_backward_f64 (that entry has no `compute` word): per calling thread, like the two settings above;
 * non-zero = the next fp64-I/O backward calls of this thread solve with K^T.  Reset it to 0 afterwards. */
void lcp_set_backward_adjoint(int on);
void lcp_debug_set_path(int path);

#ifdef __cplusplus
}
#endif
#endif /* LCP_HIP_H */
