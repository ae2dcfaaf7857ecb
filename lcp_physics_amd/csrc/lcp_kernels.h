// lcp_kernels.h - internal launch-argument structs shared by the kernel translation units and
// the C-ABI layer (lcp_api.cpp).  Plain C++: no HIP types, no torch types.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lcp_hip.h"

namespace lcp {

struct Plan {
  int ok;            // fits the LDS budget
  int ldT;           // leading dimension of T
  int t_in_lds;      // where the matrices live (lcp_generic.hip carve()): 1 = all in LDS, 0 = T = R + diag(s/z) and the prefactor scratch in the workspace, 2 = Q, Q^-1, G there too
  size_t lds_bytes;  // dynamic LDS per workgroup
  size_t ws_stride;  // workspace elements (compute precision) per scene
};

struct FwdArgs {
  int B, nz, m, e;
  const void *Q, *p, *G, *h, *A, *b, *F;
  void *x, *y, *z, *s;
  int32_t* iters;
  int32_t* status;
  void* ws;
  size_t ws_stride;
  double eps;
  int max_iter, lim;
  int ldT, t_in_lds;
  double* trace;     // optional [B, max_iter, 4] (resid, mu, sigma, alpha) - debugging aid
  const int32_t* cls;  // optional per-scene class (lcp_classify_big): the generic kernels leave scenes of class 2 alone
  int32_t* tag;        // workspace trailer word: every forward kernel writes `tag_value` (kernel family + layout) there
  int tag_value;
};

struct BwdArgs {
  int B, nz, m, e;
  const void *G, *A, *dl_dx;
  void *dQ, *dp, *dG, *dh, *dA, *db, *dF;
  void* ws;
  size_t ws_stride;
  int ldT, t_in_lds;
  const int32_t* cls;  // as FwdArgs::cls
  const int32_t* tag;  // workspace trailer word the forward left; a backward that finds another value than `tag_value` (a workspace
  int tag_value;       // laid out by another kernel family) returns NaN gradients instead of reading it
  int skip_tag;        // 0, or the tag of the OTHER kernel family the forward may have fallen back on (wave64 step -> generic step
                       // when contact counts are given): a backward that finds it leaves without writing, its partner serves the call
  int adjoint;         // LCP_BWD_ADJOINT (generic kernels): factor T^T - the solve with K^T instead of the reference's K
  int split;           // lcp_bwd_quad<..., BODY> (round 6): 1 = leave dG and dF to lcp_bwd_stream_quad - the solve kernel hands (x, dx, lam, dlam)
                       // over in the scene's workspace block and writes the small gradients only
};

// dense (Q, p, G, h, A, b, F) boundary of lcp_big.hip: LCPFunction sizes beyond the wave-per-scene kernels (nineq <= 256)
// where lcp_classify_big leaves the per-contact records of a contact-structured dense scene for the body-space kernels (bytes into the
// scene's workspace block; behind lcp_primal's 6.3 KB iterate block, 4 KB long at 64 contacts - the block is at least 32 KB at these sizes)
constexpr size_t DENSE_EXTRACT_OFF = 8192;

struct DenseIO {
  int nz, m;
  int32_t* tag;                                     // workspace trailer word (see FwdArgs::tag)
  int tag_value;
  const float *Q, *p, *G, *h, *A, *b, *F;           // forward inputs
  float *x, *y, *z, *s;                             // forward outputs
  int32_t *iters, *status;
  int32_t* cls;                                     // [B] class per scene (2 = contact-structured with diagonal Q)
  size_t ws_scene;                                  // workspace bytes per scene (common to the kernel families of a batch)
  const float* dl_dx;                               // backward: cotangent, then the seven gradients (any may be NULL)
  float *dQ, *dp, *dG, *dh, *dA, *db, *dF;
};
inline DenseIO dense_io(const FwdArgs& P, int32_t* cls, size_t ws_scene) {
  DenseIO DN = {};
  DN.nz = P.nz; DN.m = P.m; DN.cls = cls; DN.ws_scene = ws_scene;
  DN.Q = (const float*)P.Q; DN.p = (const float*)P.p; DN.G = (const float*)P.G; DN.h = (const float*)P.h;
  DN.A = (const float*)P.A; DN.b = (const float*)P.b; DN.F = (const float*)P.F;
  return DN;
}
inline DenseIO dense_io(const BwdArgs& P, int32_t* cls, size_t ws_scene) {
  DenseIO DN = {};
  DN.nz = P.nz; DN.m = P.m; DN.cls = cls; DN.ws_scene = ws_scene;
  DN.G = (const float*)P.G; DN.A = (const float*)P.A; DN.dl_dx = (const float*)P.dl_dx;
  DN.dQ = (float*)P.dQ; DN.dp = (float*)P.dp; DN.dG = (float*)P.dG; DN.dh = (float*)P.dh; DN.dA = (float*)P.dA; DN.db = (float*)P.db; DN.dF = (float*)P.dF;
  return DN;
}

struct StepArgs {
  int B, nb, nc, e;
  const void *pos, *Mdiag, *v, *f, *rest, *fric, *c_n, *c_p1, *c_p2;
  const int32_t *c_i1, *c_i2;
  const int32_t* c_count;   // per-scene live contacts (<= nc) or NULL = nc everywhere
  const void* Je;
  double dt;
  double eps;
  int max_iter, lim;
  void *v_new, *p_new, *z, *s, *y;
  int32_t* iters;
  int32_t* status;
  void* ws;
  size_t ws_stride;
  int ldT, t_in_lds;
  // post-stabilisation (generic_post_stab only): pose before / after the correction move and the dt every scene used
  const double* pos64;
  const double* dt_scene;
  double* p_out64;
  int32_t* tag;             // workspace trailer word (see FwdArgs::tag): written by the forward kernels, compared by the backward ones
  int tag_value;
};
// the contact-list arguments of a dense call on the contact-structured kernels (lcp_big.hip, lcp_primal.hip); `nb`: the bodies the
// unit's kernels see in nz columns
inline StepArgs dense_step_args(const FwdArgs& P, int nb) {
  StepArgs SP = {};
  SP.B = P.B; SP.nb = nb; SP.nc = P.m / 4; SP.e = P.e; SP.ws = P.ws;
  SP.eps = P.eps; SP.max_iter = P.max_iter; SP.lim = P.lim;
  SP.v_new = P.x; SP.z = P.z; SP.s = P.s; SP.y = P.y; SP.iters = P.iters; SP.status = P.status;
  SP.tag = P.tag; SP.tag_value = P.tag_value;
  return SP;
}
inline StepArgs dense_step_args(const BwdArgs& P, int nb) {
  StepArgs SP = {};
  SP.B = P.B; SP.nb = nb; SP.nc = P.m / 4; SP.e = P.e; SP.ws = P.ws;
  SP.tag = (int32_t*)P.tag; SP.tag_value = P.tag_value;
  return SP;
}

struct StepBwdArgs {
  const void* dl_dv;                                   // [B, nb, 3]  d(loss)/d(v_new)
  void *dMdiag, *dv, *df, *drest, *dfric, *dcn, *dcp1, *dcp2;
  void* dJe;                                           // [B, e, 3 nb]  d(loss)/d(Je) = dnu (x) x + nu (x) dx (lcp.py:57), or NULL
};

struct ContactArgs {
  int B, nb, maxc;
  const int32_t *kind, *nverts;         // [B, nb]  0 = circle, 1 = hull ; vertex count of a hull
  const double *radius, *verts_local;   // [B, nb], [B, nb, nvcap, 2] (body frame; nvcap = 8 on the kernels of lcp_contacts.hip)
  const uint8_t* no_contact;            // [B, nb, nb] pairs to skip, or NULL
  const double* p_start;                // [B, nb, 3] (rot, x, y)
  const float* v;                       // [B, nb, 3] or NULL (detect at p_start)
  double dt, dt_floor, eps, tol;
  const double* dt_in;                  // [B] the dt each scene's loop starts from, or NULL = `dt` everywhere; <= 0: the scene is finished
  int strict, max_trials;
  double* p_out;
  float *c_n, *c_p1, *c_p2;
  double* c_pen;
  int32_t *c_i1, *c_i2, *count;
  double *max_pen, *dt_used, *t;
  int32_t* trials;
};

// generic (any size) path - lcp_generic.hip
Plan make_plan(int nz, int m, int e, int csize);
int generic_forward(const FwdArgs& P, int io_f64, int compute, size_t lds, void* stream);
int generic_backward(const BwdArgs& P, int io_f64, int compute, size_t lds, void* stream);
int generic_step_backward(const StepArgs& P, const StepBwdArgs& Gd, int compute, size_t lds, void* stream);   // lcp_step_backward_f32 at any size of the generic plan (round 6)
int generic_post_stab_backward(const StepArgs& P, const StepBwdArgs& Gd, int compute, size_t lds, void* stream);   // lcp_post_stabilization_backward_f32, same sizes
int generic_post_stab(const StepArgs& P, int compute, size_t lds, void* stream);
int generic_step(const StepArgs& P, int compute, size_t lds, void* stream);
int generic_assemble(const StepArgs& P, float* Q, float* p, float* G, float* h, float* A, float* b,
                     float* F, void* stream);

// wave-per-scene register-resident path (nz <= 16, nineq <= 64, neq <= 8, fp32 I/O) - lcp_wave64.hip
bool wave64_supported(int nz, int m, int e);
size_t wave64_ws_bytes(int compute, int io_f64 = 0);
int wave64_forward(const FwdArgs& P, int compute, void* stream, int io_f64 = 0, int body_space = 0);   // body_space: see quad_forward
int wave64_backward(const BwdArgs& P, int compute, bool all_quad, void* stream, int io_f64 = 0, int body_space = 0);
int wave64_step(const StepArgs& P, int compute, void* stream);

// body-space (primal) contact-structured path: one wave per scene, <= 64 contacts, nz + neq <= 64 - lcp_primal.hip
bool primal_supported(int nz, int m, int e);          // contact-list entry points: up to 24 equality rows (nz + neq <= 56), up to 64 rows with at most 4 (round 6)
bool primal_poststab_supported(int nz, int m, int e); // post-stabilisation: the sizes of primal_supported
bool primal_dense_supported(int nz, int m, int e);    // dense boundary: up to 4 equality rows, nz + neq <= 56
size_t primal_ws_bytes();
int primal_step(const StepArgs& P, void* stream, bool pinned = false);      // pinned: LCP_HINT_PINNED (lcp_primal_pin.hip)
int primal_step_backward(const StepArgs& P, const StepBwdArgs& G, void* stream, bool pinned = false);
bool primal_pin_supported(int nz, int e);             // lcp_primal_pin.hip: nz - neq pivots when the equality rows pin the leading coordinates
int primal_pin_launch(const StepArgs& P, const StepBwdArgs& G, int backward, void* stream);
int primal_pin_dense_launch(const StepArgs& P, const DenseIO& DN, int backward, void* stream);   // dense boundary, scenes of class 4
int primal_chain_launch(const StepArgs& P, const StepBwdArgs& G, int backward, void* stream);   // lcp_primal_chain.hip: 5 .. 24 equality rows
int primal_post_stab_backward(const StepArgs& P, const StepBwdArgs& G, void* stream);   // lcp.py:37-64 on that LCP, contracted through engines.py:84-112
int primal_post_stab(const StepArgs& P, void* stream);                                         // engines.py:80-116 in body space
int primal_dense_forward(const FwdArgs& P, int32_t* cls, size_t ws_scene, void* stream);      // scenes of class 3 (and 4: the pinned form)
int primal_dense_backward(const BwdArgs& P, int32_t* cls, size_t ws_scene, void* stream);

// body-space contact-list step beyond one wavefront: one workgroup of 256 threads per scene, the fp64 system in LDS - lcp_primal_wg.hip
bool primal_wg_supported(int nz, int m, int e, bool pinned);   // <= 128 pivots (pinned: nz - 3; otherwise nz + neq, neq <= 4), <= 256 contacts
size_t primal_wg_ws_bytes(int m);                              // per scene: contact count, best iterate (x, y, z, s)
int primal_wg_step(const StepArgs& P, void* stream, bool pinned = false);
int primal_wg_step_backward(const StepArgs& P, const StepBwdArgs& G, void* stream, bool pinned = false);
// post-stabilisation on the same mapping (general form only) - lcp_primal_wg_poststab.hip
bool primal_wg_poststab_supported(int nz, int m, int e);       // nz + neq <= 128 with neq <= 4, <= 256 contacts
size_t primal_wg_poststab_ws_bytes(int m);                     // per scene: contact count, best iterate (x, y, z, s: one row per contact)
int primal_wg_post_stab(const StepArgs& P, void* stream);
int primal_wg_post_stab_backward(const StepArgs& P, const StepBwdArgs& G, void* stream);

// four-scenes-per-wave contact-structured path (nc <= 16, neq <= 4, diagonal Q; nz <= 16, or nz <= 32 from a contact
// list) - lcp_quad.hip
// `accept`: classification flag value (workspace meta[0]) the launch serves
bool quad_post_supported(int nz, int m, int e);        // post-stabilisation on this mapping (m = 4 maxc as everywhere; the LCP has maxc rows)
int quad_post_stab(const StepArgs& P, void* stream);
bool quad_supported(int nz, int m, int e);
bool quad_step_supported(int nz, int m, int e);   // contact-list entry points: nz <= 32
int quad_forward(const FwdArgs& P, int compute, int accept, void* stream, int io_f64 = 0, int body_space = 0);   // body_space: the dense boundary on the body-space kernels (fp32 tensors, fp64 arithmetic)
bool quad_dense_is_body_space(int io_f64, int compute, int body_space);   // does quad_forward run the body-space kernels for these arguments ?
int quad_backward(const BwdArgs& P, int compute, int accept, void* stream, int io_f64 = 0, int body = 0, bool pinned = false);   // body: workspace of a body-space forward; pinned: LCP_HINT_PINNED
int quad_step(const StepArgs& P, int compute, void* stream, int body_space = 1, int solo = -1, bool pinned = false);   // solo: -1 by batch size, 0 never, 1 always; pinned: LCP_HINT_PINNED
// one scene per wavefront, small batches (the body-space sizes with nz <= 16) - lcp_solo.hip
bool solo_supported(int nz, int m, int e);
int solo_step(const StepArgs& P, void* stream, bool pinned = false);
int quad_step_backward(const StepArgs& P, const StepBwdArgs& G, int compute, void* stream, int body_space = 1, bool pinned = false);
bool quad_step_is_body_space(int nz, int compute, int body_space);   // does quad_step run the body-space kernels for these arguments ?

// workgroup-per-scene contact-structured forward for up to 64 contacts (fused step, forward only) - lcp_big.hip
bool big_supported(int nz, int m, int e);
size_t big_ws_bytes(int m);
int big_step(const StepArgs& P, void* stream);
int big_step_backward(const StepArgs& P, const StepBwdArgs& G, void* stream);
// dense boundary (lcp_pdipm_forward_f32 / _backward_f32) for 16 < nineq / 4 <= 64 contacts: classification, then the same kernel
bool big_dense_supported(int nz, int m, int e);
int big_dense_forward(const FwdArgs& P, int32_t* cls, size_t ws_scene, int primal_ok, void* stream);   // (classifies: 0 / 2 / 3 / 4; primal_ok: bit 0 = lcp_primal sizes, bit 1 = pinned sizes)
int big_dense_backward(const BwdArgs& P, int32_t* cls, size_t ws_scene, void* stream);

// narrow-phase contact generation + position update - lcp_contacts.hip
bool contacts_small_supported(int nb, int nvcap);     // <= 32 bodies, hulls of capacity 8 (detection and the frame backward)
int contacts_launch(const ContactArgs& P, void* stream);
int joint_jacobian_launch(int B, int nb, int nj, int e, const int32_t* jtype, const int32_t* jb1, const int32_t* jb2, const double* jr1,
                          double* jrot1, const double* p, const float* v, const double* dt_scene, double dt, double vscale, float* Je,
                          void* stream);
int joint_jacobian_backward_launch(int B, int nb, int nj, int e, const int32_t* jtype, const int32_t* jb1, const int32_t* jb2,
                                   const double* jr1, const double* jrot1, const float* gJe, double* g_p, double* g_rot, void* stream);
int state_update_backward_launch(int B, int nb, int nj, const double* g_p, const double* g_g, const double* g_rot, const float* v,
                                 const double* dt_scene, double scale, const int32_t* jtype, const int32_t* jb1, float* g_v, void* stream);
int contact_frame_backward_launch(int B, int nb, int maxc, const int32_t* kind, const double* radius, const double* verts_local,
                                  const int32_t* nverts, const uint8_t* no_contact, const double* p, double eps,
                                  const int32_t* count, const float* g_n, const float* g_p1, const float* g_p2, double* dp,
                                  void* stream);
// the element-wise kernels around the sub-steps of World.step(fixed_dt=True) (world.py:72-80) - lcp_substep.hip
int substep_begin_launch(int B, int nb, const double* t, const double* end_t, const float* f, const int32_t* count, double* dt_k,
                         int32_t* active, int32_t* count_eff, float* f_eff, void* stream);
int substep_commit_launch(int B, int nb, const int32_t* active, const float* v_old, float* v_new, void* stream);
// the same for hulls of up to 64 vertices (verts_local[B,nb,nvcap,2], 8 <= nvcap <= 64), up to 64 bodies and
// CONTACTS_WIDE_MAX_SCENE_VERTS vertices per scene (packed per-scene vertex lists in LDS) - lcp_contacts_wide.hip
constexpr int CONTACTS_WIDE_MAX_SCENE_VERTS = 1024;
bool contacts_wide_supported(int nb, int nvcap, int scene_verts_max);   // the sizes of every kernel over the packed vertex list
int contacts_wide_launch(const ContactArgs& P, int nvcap, int scene_verts_max, void* stream);
int contact_frame_backward_wide_launch(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind,
                                       const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                       double eps, const int32_t* count, const int32_t* c_i1, const int32_t* c_i2,
                                       const float* g_n, const float* g_p1, const float* g_p2, double* dp, void* stream);
// the detection loop of contacts_wide_launch with a broadphase (bounding circle + box, survivors compacted in pair order) in front
// of the narrow phase; candidates[B] or NULL: the pairs that passed at the accepted pose - lcp_contacts_wide.hip (the cull: lcp_contacts_bp.hip)
int contacts_bp_launch(const ContactArgs& P, int nvcap, int scene_verts_max, int32_t* candidates, void* stream);
// the reference's body constructors (bodies.py:15-290, forces.py:51-67): centroid, recentred vertices, inertia, mass matrix
// diagonal and gravity from the raw shape and the mass, and their chain rule - lcp_bodies.hip (cap rounded up to a power of two
// lanes per body, segmented cross-lane sums; sizes checked by the caller: 8 <= cap <= 64)
int body_properties_launch(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                           const int32_t* nverts, const double* mass, double g, double* centroid, double* verts_local,
                           double* inertia, float* Mdiag, float* f_gravity, int32_t* status, void* stream);
int body_properties_backward_launch(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                                    const int32_t* nverts, const double* mass, double g, const double* g_centroid,
                                    const double* g_verts_local, const double* g_inertia, const float* g_Mdiag, const float* g_f,
                                    double* g_verts_raw, double* g_radius, double* g_mass, void* stream);

// lcp_render.hip: frames and masks of every scene (Body.draw, bodies.py:140-150, 237-250; world.py:279-280) and their backward
bool render_supported(int nb, int nvcap, int scene_verts_max);          // the sizes of the packed vertex list (contacts_wide_supported)
int render_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind, const double* radius,
                  const double* verts_local, const int32_t* nverts, const double* p, const float* colors, const float* background,
                  const double* thickness, double x0, double y0, double ppm, double w, float* image, int32_t* ids, void* stream);
int render_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind,
                           const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                           const float* colors, const float* background, const double* thickness, double x0, double y0, double ppm,
                           double w, const float* g_image, double* g_p, double* g_radius, double* g_verts_local, float* g_colors,
                           void* stream);

// lcp_render_marks.hip: the same frames with the bodies' marks (spoke, centre dot, diagonals) and the joints' markers
// (bodies.py:144-147, 245-247, 295-296; constraints.py:51-206; world.py:281-282) and their backward; arguments checked by the caller
struct RenderMarks {
  const int32_t* mark; const float* mark_colors;                     // [B,nb], [B,nb,C]; mark NULL: none
  int nj; const int32_t *jtype, *jb1, *jb2; const double *jr1, *jrot1; const float* joint_colors;      // the JointSet layout, [B,nj]
  int order; double line_w, dot_r, joint_w, joint_r;
};
int render_marks_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind, const double* radius,
                        const double* verts_local, const int32_t* nverts, const double* p, const float* colors, const float* background,
                        const double* thickness, double x0, double y0, double ppm, double w, const RenderMarks& mk, float* image,
                        int32_t* ids, void* stream);
int render_marks_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind,
                                 const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                 const float* colors, const float* background, const double* thickness, double x0, double y0, double ppm,
                                 double w, const RenderMarks& mk, const float* g_image, double* g_p, double* g_radius,
                                 double* g_verts_local, float* g_colors, float* g_mark_colors, float* g_joint_colors, double* g_jrot1,
                                 double* g_jr1, double* g_p_joints, void* stream);

// lcp_sensors.hip: rays cast against every scene's geometry (include/lcp_hip.h, "range sensors") and the backward of the distances;
// arguments checked by the caller
bool cast_rays_supported(int nb, int nvcap, int scene_verts_max, int R);          // render_supported and 1 <= R <= 1024
int cast_rays_launch(int B, int nb, int nvcap, int scene_verts_max, int R, const int32_t* kind, const double* radius,
                     const double* verts_local, const int32_t* nverts, const double* p, const int32_t* ray_body,
                     const double* ray_origin, const double* ray_angle, const double* ray_range, double* dist, int32_t* hit,
                     double* normal, void* stream);
int cast_rays_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int R, const int32_t* kind, const double* radius,
                              const double* verts_local, const int32_t* nverts, const double* p, const int32_t* ray_body,
                              const double* ray_origin, const double* ray_angle, const double* ray_range, const double* g_dist,
                              double* g_p, double* g_radius, double* g_verts_local, double* g_ray_origin, double* g_ray_angle,
                              void* stream);

// lcp_proximity.hip: the signed distance between body pairs (include/lcp_hip.h, "proximity queries") and the backward of the
// distances; arguments checked by the caller
bool pair_distance_supported(int nb, int nvcap, int scene_verts_max, int P);      // render_supported and 1 <= P <= 1024
int pair_distance_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                         const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                         const int32_t* pair_second, const double* pair_max_dist, double* dist, double* normal, double* w1, double* w2,
                         void* stream);
int pair_distance_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                  const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                                  const int32_t* pair_second, const double* pair_max_dist, const double* g_dist, double* g_p,
                                  double* g_radius, double* g_verts_local, void* stream);

// lcp_overlap.hip: the area of the intersection of body pairs (include/lcp_hip.h, "overlap queries") and its backward; arguments
// checked by the caller
bool pair_overlap_supported(int nb, int nvcap, int scene_verts_max, int P);       // render_supported and 1 <= P <= 1024
int pair_overlap_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                        const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                        const int32_t* pair_second, double* area, void* stream);
int pair_overlap_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                 const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                                 const int32_t* pair_second, const double* g_area, double* g_p, double* g_radius,
                                 double* g_verts_local, void* stream);

// lcp_points.hip: the signed distance from query points to the scene (include/lcp_hip.h, "point probes") and the backward of the
// distances; arguments checked by the caller
bool point_distance_supported(int nb, int nvcap, int scene_verts_max, int N);     // render_supported and 1 <= N <= 1024
int point_distance_launch(int B, int nb, int nvcap, int scene_verts_max, int N, const int32_t* kind, const double* radius,
                          const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pt_body,
                          const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist, double* dist, int32_t* body,
                          double* normal, void* stream);
int point_distance_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int N, const int32_t* kind, const double* radius,
                                   const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pt_body,
                                   const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist, const double* g_dist,
                                   double* g_p, double* g_radius, double* g_verts_local, double* g_pt_xy, void* stream);

// lcp_toi.hip: the time of impact of body pairs along the move p + t v (include/lcp_hip.h, "time of impact") and the backward of the
// times; arguments checked by the caller
bool time_of_impact_supported(int nb, int nvcap, int scene_verts_max, int P);     // render_supported and 1 <= P <= 1024
int time_of_impact_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                          const double* verts_local, const int32_t* nverts, const double* p, const float* v, const int32_t* pair_first,
                          const int32_t* pair_second, const double* margin, const double* horizon, double tol, int max_iter, double* toi,
                          int32_t* status, double* normal, double* first_toi, int32_t* first_pair, void* stream);
int time_of_impact_backward_launch(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                   const double* verts_local, const int32_t* nverts, const double* p, const float* v,
                                   const int32_t* pair_first, const int32_t* pair_second, const double* toi, const int32_t* status,
                                   const double* g_toi, double* g_p, double* g_v, double* g_radius, double* g_verts_local, double* g_margin,
                                   void* stream);

// lcp_forces.hip: the force elements (include/lcp_hip.h, "force elements") and their backward; arguments checked by the caller
bool force_elements_supported(int nb, int E);                                     // 1 <= nb <= 64 and 1 <= E <= 1024
int force_elements_launch(int B, int nb, int E, const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1,
                          const double* a2, const double* k, const double* c, const double* x0, const double* w0, const double* limit,
                          const double* p, const float* v, const float* f_base, float* f_out, void* stream);
int force_elements_backward_launch(int B, int nb, int E, const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1,
                                   const double* a2, const double* k, const double* c, const double* x0, const double* w0,
                                   const double* limit, const double* p, const float* v, const float* g_f, double* g_p, double* g_v,
                                   double* g_k, double* g_c, double* g_x0, double* g_w0, double* g_a1, double* g_a2, void* stream);

// lcp_links.hip: the rows of the mechanism links (include/lcp_hip.h, "mechanism links") and their backward; arguments checked by the caller
bool link_jacobian_supported(int nb, int L, int e0);                              // 1 <= nb <= 64, 1 <= L <= 256, 0 <= e0 <= 65536
int link_jacobian_launch(int B, int nb, int L, int e0, int el, const int32_t* kind, const int32_t* first, const int32_t* second,
                         const double* a1, const double* a2, const double* phi, const double* p, const float* Je_base, float* Je,
                         void* stream);
int link_jacobian_backward_launch(int B, int nb, int L, int e0, int el, const int32_t* kind, const int32_t* first, const int32_t* second,
                                  const double* a1, const double* a2, const double* phi, const double* p, const float* gJe, double* g_p,
                                  double* g_a1, double* g_a2, double* g_phi, void* stream);

// lcp_report.hip: the contact report (include/lcp_hip.h, "contact reports"); arguments checked by the caller
bool contact_report_supported(int nb, int maxc, int P);                           // 1 <= nb <= 64, 1 <= maxc <= 1024, 0 <= P <= 1024
int contact_report_launch(int B, int nb, int maxc, int e, int P, const int32_t* c_count, const int32_t* active, const float* c_n,
                          const float* c_p1, const float* c_p2, const int32_t* c_i1, const int32_t* c_i2, const float* z, const float* y,
                          const float* Je, const int32_t* pair_first, const int32_t* pair_second, double min_impulse, float* body_impulse,
                          float* body_normal, int32_t* body_touching, float* joint_impulse, float* pair_impulse, float* pair_normal,
                          int32_t* pair_contacts, void* stream);

// lcp_encoder.hip: the breakout encoder (experiments/breakout/encoder.py:63-145), one workgroup per frame; arguments checked by
// the caller, `layout` the LCP_ENC_LAYOUT_WORDS host words
int extract_params_launch(int B, int H, int W, const uint8_t* frame, long long stride_b, long long stride_row, long long stride_col,
                          const int32_t* layout, int max_blocks, int32_t* paddle, int32_t* blocks, int32_t* nblocks, int32_t* ball,
                          int32_t* status, double* paddle_params, double* block_params, double* ball_params, void* stream);

// backward of the contact frame with respect to the SHAPE (radii, body-frame hull vertices) at the same sizes: one lane per
// (contacting pair, shape coordinate the pair's records were built from) - lcp_contacts_shape.hip
int contact_frame_backward_shape_launch(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind,
                                        const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                        double eps, const int32_t* count, const int32_t* c_i1, const int32_t* c_i2,
                                        const float* g_n, const float* g_p1, const float* g_p2, double* d_radius,
                                        double* d_verts_local, void* stream);

}  // namespace lcp
