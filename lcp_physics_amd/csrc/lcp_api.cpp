// lcp_api.cpp - the C ABI declared in include/lcp_hip.h: argument checking, launch planning and
// dispatch to the kernel translation units.  No torch types, no allocation, no synchronisation.
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "lcp_kernels.h"

namespace {

// The library keeps NO process-global mutable state: launches are planned from their arguments alone and ordered on the
// caller's stream, so any number of host threads may drive any number of streams / devices concurrently.  The two
// debugging aids below are per calling thread (thread_local), and the kernel family can also be forced per call with
// the LCP_PATH_* bits of the `compute` word.
thread_local double* g_trace = nullptr;   // debugging aid, see lcp_debug_set_trace
thread_local int g_adjoint = 0;           // lcp_set_backward_adjoint: LCP_BWD_ADJOINT for the fp64-I/O backward (it has no `compute` word)
thread_local int g_path = 0;              // lcp_debug_set_path: this thread's DEFAULT kernel path for calls whose `compute` word names
                                          // none, a value of enum Path below (any other value: automatic, except that
                                          // post-stabilisation then runs on the generic kernels)

constexpr int FLAG_BITS = LCP_BWD_ADJOINT | LCP_PATH_GENERIC | LCP_HINT_ALL_CONTACT | LCP_IO_F64 | LCP_PATH_CONTACT_SPACE | LCP_PATH_PRIMAL | LCP_PATH_QUAD | LCP_PATH_SOLO |
                          LCP_HINT_PINNED | LCP_PATH_PRIMAL_WG;

// Forced kernel path; the values are those of lcp_debug_set_path
enum Path : int { P_AUTO = 0, P_GENERIC = 1, P_CONTACT_SPACE = 3, P_PRIMAL = 4, P_PRIMAL_WG = 5 };
// lcp_quad.hip or lcp_solo.hip at the four-scenes-per-wave sizes (same workspace layout either way: forward only)
enum Solo { SOLO_AUTO = -1, SOLO_NEVER = 0, SOLO_ALWAYS = 1 };

// The `compute` word of an entry point, parsed once per call.  The path is a function of the WORD whenever the word names one
// (LCP_PATH_*): a forward and its backward that carry the same word pick the same kernel family on any two host threads.  Only a
// word without path bits falls back on the calling thread's lcp_debug_set_path default.
struct Word {
  int arith;          // LCP_COMPUTE_F32 / LCP_COMPUTE_F64 (anything else: LCP_E_BADARG)
  bool io_f64;        // fp64 tensors (lcp_pdipm_*_f64; LCP_IO_F64 for lcp_workspace_bytes)
  Path path;
  Solo solo;
  bool pinned, all_contact, adjoint;
  bool ok() const { return arith == LCP_COMPUTE_F32 || arith == LCP_COMPUTE_F64; }
  bool f64() const { return arith == LCP_COMPUTE_F64; }
};
inline Word parse(int compute, bool io_f64 = false) {
  Word w;
  w.arith = compute & ~FLAG_BITS;
  w.io_f64 = io_f64;
  w.path = (compute & LCP_PATH_GENERIC) ? P_GENERIC : (compute & LCP_PATH_CONTACT_SPACE) ? P_CONTACT_SPACE
         : (compute & LCP_PATH_PRIMAL) ? P_PRIMAL : (compute & LCP_PATH_PRIMAL_WG) ? P_PRIMAL_WG : (Path)g_path;
  w.solo = (compute & LCP_PATH_SOLO) ? SOLO_ALWAYS : (compute & LCP_PATH_QUAD) ? SOLO_NEVER : SOLO_AUTO;
  w.pinned = (compute & LCP_HINT_PINNED) != 0;
  w.all_contact = (compute & LCP_HINT_ALL_CONTACT) != 0;
  w.adjoint = (compute & LCP_BWD_ADJOINT) != 0 || (io_f64 && g_adjoint);
  return w;
}

// Workspace trailer (one 256-byte block behind the scene blocks and the class words): tag[0] = which forward laid the workspace
// out.  Every forward kernel writes it, every backward kernel compares it with what ITS launch plan expects and returns NaN
// gradients on a mismatch (a backward planned for another kernel family would otherwise misread the layout silently).
enum WsTag {
  TAG_DENSE_WAVE = 1, TAG_DENSE_BIG = 2, TAG_DENSE_GENERIC = 3,                       // lcp_pdipm_forward_*
  TAG_STEP_QUAD_BODY = 4, TAG_STEP_QUAD_CS = 5, TAG_STEP_PRIMAL = 6, TAG_STEP_BIG = 7, TAG_STEP_WAVE64 = 8, TAG_STEP_GENERIC = 9,
  TAG_POSTSTAB_PRIMAL = 10, TAG_POSTSTAB_GENERIC = 11,
  TAG_DENSE_WAVE_BODY = 12,                                                           // lcp_pdipm_forward_f32, class-2 scenes solved in body space (no W)
  TAG_STEP_PRIMAL_WG = 13,                                                            // contact-list step, one workgroup per scene in body space
  TAG_POSTSTAB_PRIMAL_WG = 14                                                         // post-stabilisation, one workgroup per scene in body space
};
constexpr size_t TRAILER_BYTES = 256;

// Per-scene workspace bytes: the largest layout of the families that can serve the sizes, so that every call of one op (any word,
// forward or backward) agrees on the stride.  `pl`: the generic plan of the sizes (plan_of).
inline lcp::Plan plan_of(int nz, int m, int e, const Word& w) { return lcp::make_plan(nz, m, e, (w.io_f64 || w.f64()) ? 8 : 4); }
inline size_t scene_bytes(int nz, int m, int e, const Word& w, const lcp::Plan& pl) {
  size_t per_scene = pl.ws_stride * ((w.io_f64 || w.f64()) ? 8 : 4);
  if (lcp::wave64_supported(nz, m, e) || lcp::quad_step_supported(nz, m, e)) {   // (lcp_quad.hip uses the wave64 layout)
    const size_t b = lcp::wave64_ws_bytes(w.io_f64 ? LCP_COMPUTE_F64 : w.arith, w.io_f64);
    if (b > per_scene) per_scene = b;
  }
  if (!lcp::quad_step_supported(nz, m, e) && lcp::big_supported(nz, m, e) && lcp::big_ws_bytes(m) > per_scene)
    per_scene = lcp::big_ws_bytes(m);      // (the sizes the quad kernel takes never reach lcp_big.hip)
  if (lcp::primal_supported(nz, m, e) && lcp::primal_ws_bytes() > per_scene) per_scene = lcp::primal_ws_bytes();
  return (per_scene + 15) & ~(size_t)15;
}
inline size_t cls_bytes_of(int B) { return (((size_t)B * sizeof(int32_t)) + 255) & ~(size_t)255; }
inline int32_t* trailer_of(void* ws, int B, size_t per_scene) { return (int32_t*)((unsigned char*)ws + (size_t)B * per_scene + cls_bytes_of(B)); }

// The routing decision of one call: which kernel family serves it, the workspace layout that family leaves (tag, stride) and
// whether a backward can read it - computed once, before any launch, and read by the forward, its backward and the queries.
enum Family { FAM_QUAD, FAM_PRIMAL, FAM_BIG, FAM_PRIMAL_WG, FAM_WAVE64, FAM_GENERIC };
struct Route {
  Family fam;
  int tag;               // workspace tag the forward of this family leaves
  size_t ws_scene;       // per-scene workspace bytes (scene_bytes)
  lcp::Plan plan;        // the generic kernels' plan (plan.ok = 0: they cannot take the sizes)
  bool has_backward;
  int counts_tag;        // step: the tag the forward leaves when given per-scene contact counts, where that changes the family
                         // (FAM_WAVE64 -> the generic step), else 0
  // dense entries (lcp_pdipm_*): FAM_WAVE64 = the wave-per-scene kernels, FAM_BIG = per-scene classes (lcp_classify_big) for lcp_big.hip,
  // lcp_primal.hip and the generic kernels, FAM_GENERIC = the generic kernels alone
  bool dense_body;       // FAM_WAVE64: the contact-structured scenes on the four-scenes-per-wave kernels in body space
  bool primal_dense;     // FAM_BIG: the sizes of lcp_primal.hip's dense kernels (classes 3 / 4)
  int primal_ok;         // FAM_BIG: what the forward may classify 3 (bit 0) / 4 (bit 1), before it checks F and G for 16-byte alignment
};

inline Route route_base(int nz, int m, int e, const Word& w) {
  Route r = {};
  r.plan = plan_of(nz, m, e, w);
  r.ws_scene = scene_bytes(nz, m, e, w, r.plan);
  return r;
}

// Contact-list entry points (lcp_step_fused_f32, lcp_solve_dynamics_f32, lcp_step_backward_*): nz = 3 nb, m = 4 maxc.
// `has_counts`: per-scene contact counts (lcp_solve_dynamics_f32); a backward cannot tell and routes without.
inline Route route_step(int nz, int m, int e, const Word& w, bool has_counts) {
  Route r = route_base(nz, m, e, w);
  const bool cs = w.path == P_CONTACT_SPACE;
  // lcp_primal_wg.hip: its sizes, fp64 arithmetic, and its per-scene block within the stride the workspace already has there (so
  // that lcp_workspace_bytes stays what it was); automatic mode also only where the generic plan holds the size (no size gains or
  // loses LCP_E_TOOLARGE, lcp_step_has_backward answers as before)
  auto wg_ok = [&] { return w.f64() && lcp::primal_wg_supported(nz, m, e, w.pinned) && lcp::primal_wg_ws_bytes(m) <= r.ws_scene; };
  if (w.path == P_GENERIC) r.fam = FAM_GENERIC;
  else if (w.path == P_PRIMAL && w.f64() && lcp::primal_supported(nz, m, e)) r.fam = FAM_PRIMAL;   // (A/B: one wave per scene at every size)
  else if (w.path == P_PRIMAL_WG && wg_ok()) r.fam = FAM_PRIMAL_WG;        // (A/B: one workgroup per scene wherever it fits)
  else if (lcp::quad_step_supported(nz, m, e)) r.fam = FAM_QUAD;          // <= 16 contacts, <= 10 bodies, e <= 4
  else if (w.f64() && !cs && lcp::primal_supported(nz, m, e)) r.fam = FAM_PRIMAL;   // <= 64 contacts, body-space systems
  else if (w.f64() && lcp::big_supported(nz, m, e)) r.fam = FAM_BIG;      // <= 64 contacts (fp64 arithmetic)
  else if (!cs && wg_ok() && r.plan.ok) r.fam = FAM_PRIMAL_WG;            // <= 128 pivots, <= 256 contacts
  else if (lcp::wave64_supported(nz, m, e) && !has_counts) r.fam = FAM_WAVE64;   // nz <= 16, e 5..8 (its kernel takes full lists only)
  else r.fam = FAM_GENERIC;
  switch (r.fam) {
    case FAM_QUAD: r.tag = lcp::quad_step_is_body_space(nz, w.arith, !cs) ? TAG_STEP_QUAD_BODY : TAG_STEP_QUAD_CS; break;   // (two layouts: with and without W)
    case FAM_PRIMAL: r.tag = TAG_STEP_PRIMAL; break;
    case FAM_BIG: r.tag = TAG_STEP_BIG; break;
    case FAM_PRIMAL_WG: r.tag = TAG_STEP_PRIMAL_WG; break;
    case FAM_WAVE64: r.tag = TAG_STEP_WAVE64; r.counts_tag = TAG_STEP_GENERIC; break;
    default: r.tag = TAG_STEP_GENERIC;
  }
  r.has_backward = r.fam == FAM_GENERIC ? r.plan.ok : r.fam != FAM_WAVE64;   // (the wave64 step kernel keeps no workspace a backward can read)
  return r;
}

// lcp_post_stabilization_*: body space where the sizes allow (lcp_quad.hip in automatic mode where it takes them, lcp_primal.hip
// otherwise - one layout, one tag, one backward; beyond one wavefront lcp_primal_wg_poststab.hip with a layout and a tag of its
// own), the generic kernels everywhere else
inline Route route_poststab(int nz, int m, int e, const Word& w) {
  Route r = route_base(nz, m, e, w);
  const bool body = (w.path == P_AUTO || w.path == P_PRIMAL) && w.f64() && lcp::primal_poststab_supported(nz, m, e);
  // lcp_primal_wg_poststab.hip: its sizes, fp64 arithmetic, its per-scene block within the stride the workspace already has there
  // and only where the generic plan holds the size (lcp_workspace_bytes, lcp_post_stabilization_has_backward and LCP_E_TOOLARGE
  // stay what they were).  Its time follows the bodies alone, the generic kernels' (one row per contact: T is maxc x maxc) the
  // contacts: automatic mode takes it from three contact slots per two bodies on (m >= 2 nz), where it measured 1.4 x - 29 x
  // faster; at one slot per body the two are within 20 % of each other, either way (profiles/r09_poststab_wg_sweep.json).
  // LCP_PATH_PRIMAL_WG takes it wherever it fits, the sizes of the one-wave kernels included (A/B)
  const bool wg_fits = w.f64() && lcp::primal_wg_poststab_supported(nz, m, e) && lcp::primal_wg_poststab_ws_bytes(m) <= r.ws_scene && r.plan.ok;
  const bool wg = !body && wg_fits && (w.path == P_PRIMAL_WG || (w.path == P_AUTO && m >= 2 * nz));
  r.fam = wg ? FAM_PRIMAL_WG : !body ? FAM_GENERIC : (w.path == P_AUTO && lcp::quad_post_supported(nz, m, e)) ? FAM_QUAD : FAM_PRIMAL;
  r.tag = wg ? TAG_POSTSTAB_PRIMAL_WG : body ? TAG_POSTSTAB_PRIMAL : TAG_POSTSTAB_GENERIC;
  r.has_backward = body || r.plan.ok;
  return r;
}

// lcp_pdipm_forward_* / lcp_pdipm_backward_*
inline Route route_dense(int nz, int m, int e, const Word& w) {
  Route r = route_base(nz, m, e, w);
  const bool generic = w.path == P_GENERIC;
  if (!generic && lcp::wave64_supported(nz, m, e)) {          // (fp64 I/O runs the same kernels with fp64 loads / stores)
    // the contact-structured scenes go to the four-scenes-per-wave kernels: in body space unless the word asks for the contact-space
    // formulation (LCP_PATH_CONTACT_SPACE)
    r.fam = FAM_WAVE64;
    r.dense_body = w.path != P_CONTACT_SPACE && lcp::quad_supported(nz, m, e) && lcp::quad_dense_is_body_space(w.io_f64, w.arith, 1);
    r.tag = r.dense_body ? TAG_DENSE_WAVE_BODY : TAG_DENSE_WAVE;
  } else if (!generic && !w.io_f64 && w.f64() && lcp::big_dense_supported(nz, m, e)) {
    // 17 .. 64 contacts (nineq <= 256): lcp_big.hip where the scene has the contact structure (classified per scene on the device),
    // the generic kernels for the other scenes of the batch, on ONE per-scene stride; the classes live behind the B scene blocks
    r.fam = FAM_BIG;
    r.tag = TAG_DENSE_BIG;
    r.primal_dense = (nz % 3) == 0 && lcp::primal_dense_supported(nz, m, e);
    // (the body-space kernels read lcp_classify_big's per-contact records - 16 floats per contact, DENSE_EXTRACT_OFF into the
    //  scene's block: a precondition of that route)
    const bool rec_fits = lcp::DENSE_EXTRACT_OFF + (size_t)16 * (m / 4) * sizeof(float) <= r.ws_scene;
    r.primal_ok = (w.path != P_CONTACT_SPACE && rec_fits && r.primal_dense) ? (1 | (lcp::primal_pin_supported(nz, e) ? 2 : 0)) : 0;
  } else {
    r.fam = FAM_GENERIC;
    r.tag = TAG_DENSE_GENERIC;
  }
  r.has_backward = r.fam == FAM_WAVE64 || r.plan.ok;        // (forward too: every family but wave64 runs the generic kernels as well)
  return r;
}

// lcp_move_find_contacts_*: which kernels serve a detection call of these sizes.  The limits themselves are the two predicates'
// (lcp_contacts.hip: <= 32 bodies, capacity 8; lcp_contacts_wide.hip: <= 64 bodies, capacity 8..64, <= 1024 vertices per scene).
enum DetectEntry { DETECT_F64, DETECT_NV, DETECT_DTS, DETECT_BP };      // lcp_move_find_contacts_f64, _nv_f64, _dts_f64, _bp_f64
enum DetectKernels { DETECT_NONE, DETECT_SMALL, DETECT_WIDE, DETECT_BROADPHASE };   // lcp_contacts.hip, lcp_contacts_wide.hip, lcp_contacts_bp.hip
inline DetectKernels route_contacts(DetectEntry entry, int nb, int nvcap, int scene_verts_max) {
  const bool small = lcp::contacts_small_supported(nb, nvcap);
  const bool wide = lcp::contacts_wide_supported(nb, nvcap, scene_verts_max);
  switch (entry) {
    case DETECT_F64: return small ? DETECT_SMALL : DETECT_NONE;
    // the wide kernel at every size it accepts, the sizes of the small kernels included (callers compare the two there)
    case DETECT_NV: return wide ? DETECT_WIDE : DETECT_NONE;
    // the limits of lcp_move_find_contacts_nv_f64, whichever kernel serves the call
    case DETECT_DTS: return !wide ? DETECT_NONE : small ? DETECT_SMALL : DETECT_WIDE;
    default: return wide ? DETECT_BROADPHASE : DETECT_NONE;
  }
}

}  // namespace

extern "C" {

const char* lcp_version(void) { return "lcp_hip 0.2.0 gfx950"; }

size_t lcp_workspace_bytes(int B, int nz, int m, int e, int compute) {
  if (B <= 0 || nz <= 0 || m <= 0 || e < 0) return 0;
  Word w = parse(compute, (compute & LCP_IO_F64) != 0);
  if (w.io_f64) w.arith = LCP_COMPUTE_F64;
  // scene blocks | per-scene classes of the dense lcp_big path | trailer (the layout tag)
  return (size_t)B * scene_bytes(nz, m, e, w, plan_of(nz, m, e, w)) + cls_bytes_of(B) + TRAILER_BYTES;
}

// Debugging / A-B aid: the calling thread's default path for calls whose `compute` word carries no LCP_PATH_* bit (enum Path:
// 0 automatic, 1 generic kernels, 3 contact-space kernels, 4 one wave per scene, 5 one workgroup per scene in body space).  Prefer
// the per-call bits: they travel with the word from a forward to its backward, whatever threads the two run on.
void lcp_debug_set_path(int path) { g_path = path; }

// Debugging aid (not part of the drop-in surface): when set, the dense forward writes
// trace[B, max_iter, 4] = (resid, mu, sigma, alpha) per PDIPM iteration.  Pass NULL to disable.
void lcp_debug_set_trace(double* device_trace) { g_trace = device_trace; }
void lcp_set_backward_adjoint(int on) { g_adjoint = on ? 1 : 0; }

static int forward_common(int io_f64, int B, int nz, int m, int e, const void* Q, const void* p, const void* G,
                          const void* h, const void* A, const void* b, const void* F, double eps, int max_iter,
                          int lim, int compute, void* x, void* y, void* z, void* s, int32_t* iters,
                          int32_t* status, void* ws, void* stream) {
  if (B <= 0 || nz <= 0 || m <= 0 || e < 0 || max_iter < 0) return LCP_E_BADARG;
  if (!Q || !p || !G || !h || !F || !x || !z || !s || !ws) return LCP_E_BADARG;
  if (e > 0 && (!A || !b)) return LCP_E_BADARG;
  const Word w = parse(compute, io_f64);
  if (!w.ok()) return LCP_E_BADARG;
  const Route r = route_dense(nz, m, e, w);
  if (!r.has_backward) return LCP_E_TOOLARGE;                              // (nor a forward)
  lcp::FwdArgs P;
  memset(&P, 0, sizeof(P));
  P.tag = trailer_of(ws, B, r.ws_scene);
  P.tag_value = r.tag;
  P.B = B; P.nz = nz; P.m = m; P.e = e;
  P.Q = Q; P.p = p; P.G = G; P.h = h; P.A = A; P.b = b; P.F = F;
  P.x = x; P.y = y; P.z = z; P.s = s; P.iters = iters; P.status = status;
  P.ws = ws; P.ws_stride = r.plan.ws_stride; P.eps = eps; P.max_iter = max_iter; P.lim = lim;
  P.ldT = r.plan.ldT; P.t_in_lds = r.plan.t_in_lds; P.trace = g_trace;
  if (r.fam == FAM_WAVE64) return lcp::wave64_forward(P, w.arith, stream, io_f64, r.dense_body);
  if (r.fam == FAM_BIG) {
    int32_t* cls = (int32_t*)((unsigned char*)ws + (size_t)B * r.ws_scene);
    // classes per scene: 4 = as 3 with equality rows that pin the leading coordinates (lcp_primal_pin.hip); 3 = contact structure, at
    // most two bodies per contact, sizes of lcp_primal.hip; 2 = contact structure (lcp_big.hip); 0 = anything else (the generic kernels)
    // (the body-space kernels move F, dG, dF with 16-byte accesses: without that alignment the scenes stay with the contact-space /
    //  generic kernels, which make no such assumption)
    const bool aligned16 = (((uintptr_t)F | (uintptr_t)G) & 15) == 0;
    const int primal_ok = aligned16 ? r.primal_ok : 0;
    int rc = lcp::big_dense_forward(P, cls, r.ws_scene, primal_ok, stream);
    if (rc) return rc;
    if (primal_ok) { rc = lcp::primal_dense_forward(P, cls, r.ws_scene, stream); if (rc) return rc; }
    P.cls = cls; P.ws_stride = r.ws_scene / sizeof(double);                 // the rest of the batch, same stride (fp64 arithmetic)
  }
  return lcp::generic_forward(P, io_f64, w.arith, r.plan.lds_bytes, stream);
}

int lcp_pdipm_forward_f32(int B, int nz, int m, int e, const float* Q, const float* p, const float* G,
                          const float* h, const float* A, const float* b, const float* F, double eps,
                          int max_iter, int not_improved_lim, int compute, float* x, float* y, float* z,
                          float* s, int32_t* iters, int32_t* status, void* ws, void* stream) {
  return forward_common(0, B, nz, m, e, Q, p, G, h, A, b, F, eps, max_iter, not_improved_lim, compute, x, y,
                        z, s, iters, status, ws, stream);
}

int lcp_pdipm_forward_f64(int B, int nz, int m, int e, const double* Q, const double* p, const double* G,
                          const double* h, const double* A, const double* b, const double* F, double eps,
                          int max_iter, int not_improved_lim, double* x, double* y, double* z, double* s,
                          int32_t* iters, int32_t* status, void* ws, void* stream) {
  return forward_common(1, B, nz, m, e, Q, p, G, h, A, b, F, eps, max_iter, not_improved_lim,
                        LCP_COMPUTE_F64, x, y, z, s, iters, status, ws, stream);
}

static int backward_common(int io_f64, int B, int nz, int m, int e, const void* G, const void* A,
                           const void* dl_dx, int compute, void* dQ, void* dp, void* dG, void* dh, void* dA,
                           void* db, void* dF, void* ws, void* stream) {
  if (B <= 0 || nz <= 0 || m <= 0 || e < 0) return LCP_E_BADARG;
  if (!G || !dl_dx || !ws) return LCP_E_BADARG;
  if (e > 0 && !A) return LCP_E_BADARG;
  Word w = parse(compute, io_f64);       // (the forward's word: LCP_HINT_PINNED's promise holds for the backward too)
  if (w.adjoint) {                       // opt-in: solve with K^T (generic kernels; the forward ran with LCP_PATH_GENERIC)
    if (w.all_contact) return LCP_E_BADARG;
    w.path = P_GENERIC;
  }
  if (!w.ok()) return LCP_E_BADARG;
  const Route r = route_dense(nz, m, e, w);
  if (!r.has_backward) return LCP_E_TOOLARGE;
  lcp::BwdArgs P;
  memset(&P, 0, sizeof(P));
  P.tag = trailer_of(ws, B, r.ws_scene);
  P.tag_value = r.tag;
  P.B = B; P.nz = nz; P.m = m; P.e = e; P.G = G; P.A = A; P.dl_dx = dl_dx;
  P.dQ = dQ; P.dp = dp; P.dG = dG; P.dh = dh; P.dA = dA; P.db = db; P.dF = dF;
  P.ws = ws; P.ws_stride = r.plan.ws_stride; P.ldT = r.plan.ldT; P.t_in_lds = r.plan.t_in_lds;
  P.adjoint = w.adjoint ? 1 : 0;
  if (w.all_contact) {
    // LCP_HINT_ALL_CONTACT: the workspace was left by a contact-list forward (lcp_step_fused_f32 / lcp_solve_dynamics_f32) called with
    // this `compute` word.  Three of its kernel families keep a workspace a dense backward can read - the four-scenes-per-wave one
    // (in body space, no W in it: lcp_bwd_quad<..., BODY>, or in contact space, exactly as that forward decided), the wave64 step
    // kernel and the generic one (their dense layouts) -, the tag says which one it was.
    if (io_f64) return LCP_E_BADARG;
    const Route st = route_step(nz, m, e, w, false);
    P.tag_value = st.tag;
    switch (st.fam) {
      case FAM_QUAD:
        if (!lcp::quad_supported(nz, m, e)) return LCP_E_TOOLARGE;             // (nz 17..32: the physical backward only)
        return lcp::quad_backward(P, w.arith, 2, stream, 0, st.tag == TAG_STEP_QUAD_BODY, w.pinned);
      case FAM_WAVE64: {
        // the word cannot tell whether the forward had contact counts (then it ran the generic step), the tag it left can: both
        // backwards are launched, the one whose family did not run the forward finds its partner's tag and leaves without writing
        P.skip_tag = st.counts_tag;
        const int rc = lcp::wave64_backward(P, w.arith, false, stream, 0);
        if (rc || !st.plan.ok) return rc;                                      // (no generic plan: the generic step cannot have run either)
        P.tag_value = st.counts_tag; P.skip_tag = st.tag;
        return lcp::generic_backward(P, io_f64, w.arith, st.plan.lds_bytes, stream);
      }
      case FAM_GENERIC: return lcp::generic_backward(P, io_f64, w.arith, st.plan.lds_bytes, stream);
      default: return LCP_E_TOOLARGE;                                          // (lcp_primal / lcp_big / lcp_primal_wg: lcp_step_backward_f32 is their backward)
    }
  }
  if (r.fam == FAM_WAVE64) return lcp::wave64_backward(P, w.arith, false, stream, io_f64, r.dense_body);
  if (r.fam == FAM_BIG) {
    // (classes 3 / 4 - the forward only hands them out for 16-byte aligned F and G - write dG and dF with 16-byte stores)
    if (r.primal_dense && ((((uintptr_t)dG) | ((uintptr_t)dF)) & 15) != 0) return LCP_E_BADARG;
    int32_t* cls = (int32_t*)((unsigned char*)ws + (size_t)B * r.ws_scene);
    int rc = lcp::big_dense_backward(P, cls, r.ws_scene, stream);           // (the classes the forward left behind the scene blocks)
    if (rc) return rc;
    if (r.primal_dense) { rc = lcp::primal_dense_backward(P, cls, r.ws_scene, stream); if (rc) return rc; }
    P.cls = cls; P.ws_stride = r.ws_scene / sizeof(double);
  }
  return lcp::generic_backward(P, io_f64, w.arith, r.plan.lds_bytes, stream);
}

int lcp_pdipm_backward_f32(int B, int nz, int m, int e, const float* G, const float* A, const float* dl_dx,
                           int compute, float* dQ, float* dp, float* dG, float* dh, float* dA, float* db,
                           float* dF, void* ws, void* stream) {
  return backward_common(0, B, nz, m, e, G, A, dl_dx, compute, dQ, dp, dG, dh, dA, db, dF, ws, stream);
}

int lcp_pdipm_backward_f64(int B, int nz, int m, int e, const double* G, const double* A,
                           const double* dl_dx, double* dQ, double* dp, double* dG, double* dh, double* dA,
                           double* db, double* dF, void* ws, void* stream) {
  return backward_common(1, B, nz, m, e, G, A, dl_dx, LCP_COMPUTE_F64, dQ, dp, dG, dh, dA, db, dF, ws,
                         stream);
}

static int fill_step(lcp::StepArgs& P, int B, int nb, int nc, int e, const float* pos, const float* Mdiag,
                     const float* v, const float* f, const float* rest, const float* fric, const float* c_n,
                     const float* c_p1, const float* c_p2, const int32_t* c_i1, const int32_t* c_i2,
                     const float* Je, float dt) {
  if (B <= 0 || nb <= 0 || nc <= 0 || e < 0) return LCP_E_BADARG;
  if (!Mdiag || !v || !f || !rest || !fric || !c_n || !c_p1 || !c_p2 || !c_i1 || !c_i2) return LCP_E_BADARG;
  if (e > 0 && !Je) return LCP_E_BADARG;
  memset(&P, 0, sizeof(P));
  P.B = B; P.nb = nb; P.nc = nc; P.e = e;
  P.pos = pos; P.Mdiag = Mdiag; P.v = v; P.f = f; P.rest = rest; P.fric = fric;
  P.c_n = c_n; P.c_p1 = c_p1; P.c_p2 = c_p2; P.c_i1 = c_i1; P.c_i2 = c_i2; P.Je = Je; P.dt = dt;
  return 0;
}

// the workspace of a contact-list call: its trailer word and, on the generic kernels, their plan (the other families keep layouts
// of their own)
static void place(lcp::StepArgs& P, const Route& r) {
  P.tag = trailer_of(P.ws, P.B, r.ws_scene);
  P.tag_value = r.tag;
  if (r.fam == FAM_GENERIC) { P.ws_stride = r.plan.ws_stride; P.ldT = r.plan.ldT; P.t_in_lds = r.plan.t_in_lds; }
}

int lcp_assemble_contacts_f32(int B, int nb, int nc, int e, const float* Mdiag, const float* v, const float* f,
                              const float* rest, const float* fric, const float* c_n, const float* c_p1,
                              const float* c_p2, const int32_t* c_i1, const int32_t* c_i2, const float* Je,
                              float dt, float* Q, float* p, float* G, float* h, float* A, float* b, float* F,
                              void* stream) {
  lcp::StepArgs P;
  int rc = fill_step(P, B, nb, nc, e, nullptr, Mdiag, v, f, rest, fric, c_n, c_p1, c_p2, c_i1, c_i2, Je, dt);
  if (rc) return rc;
  if (!Q || !p || !G || !h || !F) return LCP_E_BADARG;
  if (e > 0 && (!A || !b)) return LCP_E_BADARG;
  return lcp::generic_assemble(P, Q, p, G, h, A, b, F, stream);
}

// forward of the contact-list entry points, by family
static int launch_step(lcp::StepArgs& P, const Word& w, void* stream) {
  const Route r = route_step(3 * P.nb, 4 * P.nc, P.e, w, P.c_count != nullptr);
  place(P, r);
  switch (r.fam) {
    case FAM_QUAD: return lcp::quad_step(P, w.arith, stream, w.path != P_CONTACT_SPACE, w.solo, w.pinned);
    case FAM_PRIMAL: return lcp::primal_step(P, stream, w.pinned);
    case FAM_BIG: return lcp::big_step(P, stream);
    case FAM_PRIMAL_WG: return lcp::primal_wg_step(P, stream, w.pinned);
    case FAM_WAVE64: return lcp::wave64_step(P, w.arith, stream);
    default: return r.plan.ok ? lcp::generic_step(P, w.arith, r.plan.lds_bytes, stream) : LCP_E_TOOLARGE;
  }
}

int lcp_step_fused_f32(int B, int nb, int nc, int e, const float* pos, const float* Mdiag, const float* v,
                       const float* f, const float* rest, const float* fric, const float* c_n,
                       const float* c_p1, const float* c_p2, const int32_t* c_i1, const int32_t* c_i2,
                       const float* Je, float dt, double eps, int max_iter, int not_improved_lim, int compute,
                       float* v_new, float* p_new, float* z, float* s, float* y, int32_t* iters,
                       int32_t* status, void* ws, void* stream) {
  const Word w = parse(compute);
  if (!w.ok()) return LCP_E_BADARG;
  lcp::StepArgs P;
  int rc = fill_step(P, B, nb, nc, e, pos, Mdiag, v, f, rest, fric, c_n, c_p1, c_p2, c_i1, c_i2, Je, dt);
  if (rc) return rc;
  if (!pos || !v_new || !p_new || !ws || max_iter < 0) return LCP_E_BADARG;
  P.eps = eps; P.max_iter = max_iter; P.lim = not_improved_lim;
  P.v_new = v_new; P.p_new = p_new; P.z = z; P.s = s; P.y = y; P.iters = iters; P.status = status;
  P.ws = ws;
  return launch_step(P, w, stream);
}

int lcp_step_backward_f32(int B, int nb, int nc, int e, const float* Mdiag, const float* v, const float* f,
                          const float* rest, const float* fric, const float* c_n, const float* c_p1,
                          const float* c_p2, const int32_t* c_i1, const int32_t* c_i2, const float* Je, float dt,
                          const float* dl_dv, int compute, float* dMdiag, float* dv, float* df, float* drest,
                          float* dfric, float* dc_n, float* dc_p1, float* dc_p2, void* ws, void* stream) {
  return lcp_step_backward_je_f32(B, nb, nc, e, Mdiag, v, f, rest, fric, c_n, c_p1, c_p2, c_i1, c_i2, Je, dt, dl_dv, compute, dMdiag,
                                  dv, df, drest, dfric, dc_n, dc_p1, dc_p2, nullptr, ws, stream);
}

int lcp_step_backward_je_f32(int B, int nb, int nc, int e, const float* Mdiag, const float* v, const float* f,
                             const float* rest, const float* fric, const float* c_n, const float* c_p1,
                             const float* c_p2, const int32_t* c_i1, const int32_t* c_i2, const float* Je, float dt,
                             const float* dl_dv, int compute, float* dMdiag, float* dv, float* df, float* drest,
                             float* dfric, float* dc_n, float* dc_p1, float* dc_p2, float* dJe, void* ws, void* stream) {
  const Word w = parse(compute);
  if (!w.ok()) return LCP_E_BADARG;
  lcp::StepArgs P;
  int rc = fill_step(P, B, nb, nc, e, nullptr, Mdiag, v, f, rest, fric, c_n, c_p1, c_p2, c_i1, c_i2, Je, dt);
  if (rc) return rc;
  if (!dl_dv || !ws) return LCP_E_BADARG;
  P.ws = ws;
  lcp::StepBwdArgs G;
  G.dl_dv = dl_dv; G.dMdiag = dMdiag; G.dv = dv; G.df = df; G.drest = drest; G.dfric = dfric;
  G.dcn = dc_n; G.dcp1 = dc_p1; G.dcp2 = dc_p2; G.dJe = (e > 0) ? dJe : nullptr;
  // the forward's route (the kernels check the tag it left in the workspace trailer)
  const Route r = route_step(3 * nb, 4 * nc, e, w, false);
  if (!r.has_backward) return LCP_E_TOOLARGE;
  place(P, r);
  switch (r.fam) {
    case FAM_QUAD: return lcp::quad_step_backward(P, G, w.arith, stream, w.path != P_CONTACT_SPACE, w.pinned);
    case FAM_PRIMAL: return lcp::primal_step_backward(P, G, stream, w.pinned);
    case FAM_BIG: return lcp::big_step_backward(P, G, stream);
    case FAM_PRIMAL_WG: return lcp::primal_wg_step_backward(P, G, stream, w.pinned);
    default: return lcp::generic_step_backward(P, G, w.arith, r.plan.lds_bytes, stream);   // (lcp_step_bwd_kernel on the iterate lcp_step_kernel kept)
  }
}

int lcp_step_has_backward(int nb, int maxc, int e, int compute) {
  if (nb <= 0 || maxc <= 0 || e < 0) return 0;
  const Word w = parse(compute);
  return w.ok() && route_step(3 * nb, 4 * maxc, e, w, false).has_backward ? 1 : 0;
}

int lcp_solve_dynamics_f32(int B, int nb, int maxc, int e, const int32_t* c_count, const float* Mdiag,
                           const float* v, const float* f, const float* rest, const float* fric,
                           const float* c_n, const float* c_p1, const float* c_p2, const int32_t* c_i1,
                           const int32_t* c_i2, const float* Je, float dt, double eps, int max_iter,
                           int not_improved_lim, int compute, float* v_new, float* z, float* s, float* y,
                           int32_t* iters, int32_t* status, void* ws, void* stream) {
  const Word w = parse(compute);
  if (!w.ok()) return LCP_E_BADARG;
  lcp::StepArgs P;
  int rc = fill_step(P, B, nb, maxc, e, nullptr, Mdiag, v, f, rest, fric, c_n, c_p1, c_p2, c_i1, c_i2, Je, dt);
  if (rc) return rc;
  if (!c_count || !v_new || !ws || max_iter < 0) return LCP_E_BADARG;
  P.c_count = c_count;
  P.eps = eps; P.max_iter = max_iter; P.lim = not_improved_lim;
  P.v_new = v_new; P.p_new = nullptr; P.z = z; P.s = s; P.y = y; P.iters = iters; P.status = status;
  P.ws = ws;
  return launch_step(P, w, stream);
}

int lcp_post_stabilization_f32(int B, int nb, int maxc, int e, const int32_t* c_count, const float* Mdiag,
                               const float* v, const float* rest, const float* c_n, const float* c_p1,
                               const float* c_p2, const int32_t* c_i1, const int32_t* c_i2, const float* Je,
                               double eps, int max_iter, int not_improved_lim, int compute, const double* p,
                               const double* dt_scene, double dt, double* p_out, float* dp, int32_t* iters,
                               int32_t* status, void* ws, void* stream) {
  const Word w = parse(compute);
  if (!w.ok()) return LCP_E_BADARG;
  lcp::StepArgs P;
  // (forces and friction do not enter this LCP: engines.py:80-116 reads M, v, Je, Jc and the restitutions only)
  int rc = fill_step(P, B, nb, maxc, e, nullptr, Mdiag, v, /*f*/ v, rest, /*fric*/ rest, c_n, c_p1, c_p2, c_i1, c_i2, Je,
                     (float)dt);
  if (rc) return rc;
  if (!c_count || !dp || !ws || max_iter < 0) return LCP_E_BADARG;
  if ((p_out != nullptr) != (p != nullptr)) return LCP_E_BADARG;
  P.c_count = c_count;
  P.dt = dt;
  P.eps = eps; P.max_iter = max_iter; P.lim = not_improved_lim;
  P.v_new = dp; P.iters = iters; P.status = status;
  P.pos64 = p; P.dt_scene = dt_scene; P.p_out64 = p_out;
  P.ws = ws;                                                                // (lcp_primal.hip leaves the best iterate there for the backward)
  const Route r = route_poststab(3 * nb, 4 * maxc, e, w);
  place(P, r);
  switch (r.fam) {
    case FAM_QUAD: return lcp::quad_post_stab(P, stream);
    case FAM_PRIMAL: return lcp::primal_post_stab(P, stream);
    case FAM_PRIMAL_WG: return lcp::primal_wg_post_stab(P, stream);
    default: return r.plan.ok ? lcp::generic_post_stab(P, w.arith, r.plan.lds_bytes, stream) : LCP_E_TOOLARGE;
  }
}

int lcp_post_stabilization_has_backward(int nb, int maxc, int e, int compute) {
  if (nb <= 0 || maxc <= 0 || e < 0) return 0;
  const Word w = parse(compute);
  return w.ok() && route_poststab(3 * nb, 4 * maxc, e, w).has_backward ? 1 : 0;
}

int lcp_post_stabilization_backward_f32(int B, int nb, int maxc, int e, const float* Mdiag, const float* v,
                                        const float* rest, const float* c_n, const float* c_p1, const float* c_p2,
                                        const int32_t* c_i1, const int32_t* c_i2, const float* Je, const float* dl_ddp,
                                        int compute, float* dMdiag, float* dv, float* drest, float* dc_n, float* dc_p1,
                                        float* dc_p2, float* dJe, void* ws, void* stream) {
  const Word w = parse(compute);
  if (!w.ok()) return LCP_E_BADARG;
  lcp::StepArgs P;
  int rc = fill_step(P, B, nb, maxc, e, nullptr, Mdiag, v, /*f*/ v, rest, /*fric*/ rest, c_n, c_p1, c_p2, c_i1, c_i2, Je, 0.0f);
  if (rc) return rc;
  if (!dl_ddp || !ws) return LCP_E_BADARG;
  // the forward's route: the body-space kernels where they ran (one wave or one workgroup per scene, each on its own layout),
  // lcp_step_bwd_kernel<.., POST> on the iterate lcp_post_stab_kernel kept otherwise
  const Route r = route_poststab(3 * nb, 4 * maxc, e, w);
  if (!r.has_backward) return LCP_E_TOOLARGE;
  P.ws = ws;
  place(P, r);
  lcp::StepBwdArgs G = {};
  G.dl_dv = dl_ddp; G.dMdiag = dMdiag; G.dv = dv; G.drest = drest; G.dcn = dc_n; G.dcp1 = dc_p1; G.dcp2 = dc_p2;
  G.dJe = (e > 0) ? dJe : nullptr;
  switch (r.fam) {
    case FAM_GENERIC: return lcp::generic_post_stab_backward(P, G, w.arith, r.plan.lds_bytes, stream);
    case FAM_PRIMAL_WG: return lcp::primal_wg_post_stab_backward(P, G, stream);
    default: return lcp::primal_post_stab_backward(P, G, stream);        // (lcp_quad.hip's forward leaves the one-wave layout)
  }
}

// What the four detection entries share: the checks of their common arguments and the one fill of the kernel argument.
// `dt_scene`: the dt each scene's loop starts from, or NULL = `dt` everywhere.
static int fill_contacts(lcp::ContactArgs& P, int B, int nb, int maxc, const int32_t* kind, const double* radius,
                         const double* verts_local, const int32_t* nverts, const uint8_t* no_contact, const double* p_start,
                         const float* v, double dt, double dt_floor, int strict, int max_trials, double eps, double tol,
                         double* p_out, float* c_n, float* c_p1, float* c_p2, double* c_pen, int32_t* c_i1, int32_t* c_i2,
                         int32_t* count, double* max_pen, double* dt_used, double* t, int32_t* trials, const double* dt_scene) {
  if (B <= 0 || nb <= 0 || maxc <= 0 || max_trials <= 0) return LCP_E_BADARG;
  if (!kind || !radius || !verts_local || !nverts || !p_start) return LCP_E_BADARG;
  if (!c_n || !c_p1 || !c_p2 || !c_i1 || !c_i2 || !count) return LCP_E_BADARG;
  memset(&P, 0, sizeof(P));
  P.B = B; P.nb = nb; P.maxc = maxc; P.kind = kind; P.nverts = nverts; P.radius = radius;
  P.verts_local = verts_local; P.no_contact = no_contact; P.p_start = p_start; P.v = v;
  P.dt = dt; P.dt_floor = dt_floor; P.eps = eps; P.tol = tol; P.strict = strict; P.max_trials = max_trials;
  P.p_out = p_out; P.c_n = c_n; P.c_p1 = c_p1; P.c_p2 = c_p2; P.c_pen = c_pen; P.c_i1 = c_i1; P.c_i2 = c_i2;
  P.count = count; P.max_pen = max_pen; P.dt_used = dt_used; P.t = t; P.trials = trials;
  P.dt_in = dt_scene;
  return 0;
}

// a detection call on the kernels route_contacts gives it (after every LCP_E_BADARG check of the entry)
static int launch_contacts(DetectEntry entry, const lcp::ContactArgs& P, int nvcap, int scene_verts_max, int32_t* candidates,
                           void* stream) {
  switch (route_contacts(entry, P.nb, nvcap, scene_verts_max)) {
    case DETECT_SMALL: return lcp::contacts_launch(P, stream);
    case DETECT_WIDE: return lcp::contacts_wide_launch(P, nvcap, scene_verts_max, stream);
    case DETECT_BROADPHASE: return lcp::contacts_bp_launch(P, nvcap, scene_verts_max, candidates, stream);
    default: return LCP_E_TOOLARGE;
  }
}

// (verts_local [B, nb, 8, 2]: this entry has no capacity argument)
int lcp_move_find_contacts_f64(int B, int nb, int maxc, const int32_t* kind, const double* radius,
                               const double* verts_local, const int32_t* nverts, const uint8_t* no_contact,
                               const double* p_start, const float* v, double dt, double dt_floor, int strict,
                               int max_trials, double eps, double tol, double* p_out, float* c_n, float* c_p1,
                               float* c_p2, double* c_pen, int32_t* c_i1, int32_t* c_i2, int32_t* count,
                               double* max_pen, double* dt_used, double* t, int32_t* trials, void* stream) {
  lcp::ContactArgs P;
  const int rc = fill_contacts(P, B, nb, maxc, kind, radius, verts_local, nverts, no_contact, p_start, v, dt, dt_floor, strict, max_trials, eps, tol,
                               p_out, c_n, c_p1, c_p2, c_pen, c_i1, c_i2, count, max_pen, dt_used, t, trials, nullptr);
  return rc ? rc : launch_contacts(DETECT_F64, P, /*nvcap*/ 8, 0, nullptr, stream);
}

int lcp_joint_jacobian_f64(int B, int nb, int nj, int e, const int32_t* jtype, const int32_t* jb1, const int32_t* jb2,
                           const double* jr1, double* jrot1, const double* p, const float* v, const double* dt_scene, double dt,
                           double vscale, float* Je, void* stream) {
  if (B <= 0 || nb <= 0 || nj <= 0 || e <= 0) return LCP_E_BADARG;
  if (!jtype || !jb1 || !jb2 || !jr1 || !jrot1 || !p || !Je) return LCP_E_BADARG;
  return lcp::joint_jacobian_launch(B, nb, nj, e, jtype, jb1, jb2, jr1, jrot1, p, v, dt_scene, dt, vscale, Je, stream);
}

int lcp_joint_jacobian_backward_f64(int B, int nb, int nj, int e, const int32_t* jtype, const int32_t* jb1, const int32_t* jb2,
                                    const double* jr1, const double* jrot1, const float* gJe, double* g_p, double* g_rot, void* stream) {
  if (B <= 0 || nb <= 0 || nj <= 0 || e <= 0) return LCP_E_BADARG;
  if (!jtype || !jb1 || !jb2 || !jr1 || !jrot1 || !gJe || !g_p || !g_rot) return LCP_E_BADARG;
  return lcp::joint_jacobian_backward_launch(B, nb, nj, e, jtype, jb1, jb2, jr1, jrot1, gJe, g_p, g_rot, stream);
}

int lcp_state_update_backward_f64(int B, int nb, int nj, const double* g_p, const double* g_g, const double* g_rot, const float* v,
                                  const double* dt_scene, double scale, const int32_t* jtype, const int32_t* jb1, float* g_v, void* stream) {
  if (B <= 0 || nb <= 0 || nj < 0) return LCP_E_BADARG;
  if (!v || !dt_scene || !g_v) return LCP_E_BADARG;
  if (g_rot && (nj <= 0 || !jtype || !jb1)) return LCP_E_BADARG;
  return lcp::state_update_backward_launch(B, nb, nj, g_p, g_g, g_rot, v, dt_scene, scale, jtype, jb1, g_v, stream);
}

// what the three contact-frame backward entries share: sizes, geometry, pose, and the records' counts and cotangents
static bool frame_args_ok(int B, int nb, int maxc, const int32_t* kind, const double* radius, const double* verts_local,
                          const int32_t* nverts, const double* p, const int32_t* count, const float* g_n, const float* g_p1,
                          const float* g_p2) {
  return B > 0 && nb > 0 && maxc > 0 && kind && radius && verts_local && nverts && p && count && g_n && g_p1 && g_p2;
}

int lcp_contact_frame_backward_f64(int B, int nb, int maxc, const int32_t* kind, const double* radius, const double* verts_local,
                                   const int32_t* nverts, const uint8_t* no_contact, const double* p, double eps,
                                   const int32_t* count, const float* g_n, const float* g_p1, const float* g_p2, double* dp,
                                   void* stream) {
  if (!frame_args_ok(B, nb, maxc, kind, radius, verts_local, nverts, p, count, g_n, g_p1, g_p2) || !dp) return LCP_E_BADARG;
  return lcp::contact_frame_backward_launch(B, nb, maxc, kind, radius, verts_local, nverts, no_contact, p, eps, count, g_n, g_p1, g_p2,
                                            dp, stream);
}

int lcp_move_find_contacts_nv_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind, const double* radius,
                                  const double* verts_local, const int32_t* nverts, const uint8_t* no_contact,
                                  const double* p_start, const float* v, double dt, double dt_floor, int strict,
                                  int max_trials, double eps, double tol, double* p_out, float* c_n, float* c_p1,
                                  float* c_p2, double* c_pen, int32_t* c_i1, int32_t* c_i2, int32_t* count,
                                  double* max_pen, double* dt_used, double* t, int32_t* trials, void* stream) {
  if (scene_verts_max < 0) return LCP_E_BADARG;
  lcp::ContactArgs P;
  const int rc = fill_contacts(P, B, nb, maxc, kind, radius, verts_local, nverts, no_contact, p_start, v, dt, dt_floor, strict, max_trials, eps, tol,
                               p_out, c_n, c_p1, c_p2, c_pen, c_i1, c_i2, count, max_pen, dt_used, t, trials, nullptr);
  return rc ? rc : launch_contacts(DETECT_NV, P, nvcap, scene_verts_max, nullptr, stream);
}

// World.step(fixed_dt=True) (world.py:72-80): step_dt(end_t - t) with a dt of its own per scene
int lcp_move_find_contacts_dts_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind, const double* radius,
                                   const double* verts_local, const int32_t* nverts, const uint8_t* no_contact,
                                   const double* p_start, const float* v, double dt, double dt_floor, int strict,
                                   int max_trials, double eps, double tol, double* p_out, float* c_n, float* c_p1,
                                   float* c_p2, double* c_pen, int32_t* c_i1, int32_t* c_i2, int32_t* count,
                                   double* max_pen, double* dt_used, double* t, int32_t* trials, const double* dt_scene, void* stream) {
  if (scene_verts_max < 0 || !dt_scene) return LCP_E_BADARG;
  lcp::ContactArgs P;
  const int rc = fill_contacts(P, B, nb, maxc, kind, radius, verts_local, nverts, no_contact, p_start, v, dt, dt_floor, strict, max_trials, eps, tol,
                               p_out, c_n, c_p1, c_p2, c_pen, c_i1, c_i2, count, max_pen, dt_used, t, trials, dt_scene);
  return rc ? rc : launch_contacts(DETECT_DTS, P, nvcap, scene_verts_max, nullptr, stream);
}

// the same loop with a broadphase in front of the narrow phase (lcp_contacts_bp.hip); dt_scene NULL: the scalar dt
int lcp_move_find_contacts_bp_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind, const double* radius,
                                  const double* verts_local, const int32_t* nverts, const uint8_t* no_contact,
                                  const double* p_start, const float* v, double dt, double dt_floor, int strict,
                                  int max_trials, double eps, double tol, double* p_out, float* c_n, float* c_p1,
                                  float* c_p2, double* c_pen, int32_t* c_i1, int32_t* c_i2, int32_t* count,
                                  double* max_pen, double* dt_used, double* t, int32_t* trials, const double* dt_scene,
                                  int32_t* candidates, void* stream) {
  if (scene_verts_max < 0) return LCP_E_BADARG;
  lcp::ContactArgs P;
  const int rc = fill_contacts(P, B, nb, maxc, kind, radius, verts_local, nverts, no_contact, p_start, v, dt, dt_floor, strict, max_trials, eps, tol,
                               p_out, c_n, c_p1, c_p2, c_pen, c_i1, c_i2, count, max_pen, dt_used, t, trials, dt_scene);
  return rc ? rc : launch_contacts(DETECT_BP, P, nvcap, scene_verts_max, candidates, stream);
}

// the bookkeeping of world.py:72-80 around one sub-step (lcp_substep.hip)
int lcp_substep_begin_f64(int B, int nb, const double* t, const double* end_t, const float* f, const int32_t* count, double* dt_k,
                          int32_t* active, int32_t* count_eff, float* f_eff, void* stream) {
  if (B <= 0 || nb <= 0) return LCP_E_BADARG;
  if (!t || !end_t || !f || !count || !dt_k || !active || !count_eff || !f_eff) return LCP_E_BADARG;
  return lcp::substep_begin_launch(B, nb, t, end_t, f, count, dt_k, active, count_eff, f_eff, stream);
}

int lcp_substep_commit_f32(int B, int nb, const int32_t* active, const float* v_old, float* v_new, void* stream) {
  if (B <= 0 || nb <= 0) return LCP_E_BADARG;
  if (!active || !v_old || !v_new) return LCP_E_BADARG;
  return lcp::substep_commit_launch(B, nb, active, v_old, v_new, stream);
}

int lcp_contact_frame_backward_nv_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind, const double* radius,
                                      const double* verts_local, const int32_t* nverts, const uint8_t* no_contact, const double* p,
                                      double eps, const int32_t* count, const int32_t* c_i1, const int32_t* c_i2, const float* g_n,
                                      const float* g_p1, const float* g_p2, double* dp, void* stream) {
  (void)no_contact;                                            // (the records name the pairs; a masked pair has none)
  if (!frame_args_ok(B, nb, maxc, kind, radius, verts_local, nverts, p, count, g_n, g_p1, g_p2)) return LCP_E_BADARG;
  if (scene_verts_max < 0 || !c_i1 || !c_i2 || !dp) return LCP_E_BADARG;
  return lcp::contact_frame_backward_wide_launch(B, nb, maxc, nvcap, scene_verts_max, kind, radius, verts_local, nverts, p, eps, count,
                                                 c_i1, c_i2, g_n, g_p1, g_p2, dp, stream);
}

int lcp_contact_frame_backward_shape_f64(int B, int nb, int maxc, int nvcap, int scene_verts_max, const int32_t* kind, const double* radius,
                                         const double* verts_local, const int32_t* nverts, const double* p, double eps,
                                         const int32_t* count, const int32_t* c_i1, const int32_t* c_i2, const float* g_n,
                                         const float* g_p1, const float* g_p2, double* d_radius, double* d_verts_local, void* stream) {
  if (!frame_args_ok(B, nb, maxc, kind, radius, verts_local, nverts, p, count, g_n, g_p1, g_p2)) return LCP_E_BADARG;
  if (scene_verts_max < 0 || !c_i1 || !c_i2) return LCP_E_BADARG;
  if (!d_radius && !d_verts_local) return LCP_E_BADARG;         // (nothing asked for)
  return lcp::contact_frame_backward_shape_launch(B, nb, maxc, nvcap, scene_verts_max, kind, radius, verts_local, nverts, p, eps, count,
                                                  c_i1, c_i2, g_n, g_p1, g_p2, d_radius, d_verts_local, stream);
}

int lcp_body_properties_f64(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                            const int32_t* nverts, const double* mass, double g, double* centroid, double* verts_local,
                            double* inertia, float* Mdiag, float* f_gravity, int32_t* status, void* stream) {
  if (B < 0 || nb < 0 || cap < 8 || cap > 64) return LCP_E_BADARG;
  if (!kind || !radius || !verts_raw || !nverts || !mass) return LCP_E_BADARG;
  if (!centroid && !verts_local && !inertia && !Mdiag && !f_gravity && !status) return LCP_E_BADARG;   // (nothing asked for)
  if (B == 0 || nb == 0) return 0;
  return lcp::body_properties_launch(B, nb, cap, kind, radius, verts_raw, nverts, mass, g, centroid, verts_local, inertia, Mdiag,
                                     f_gravity, status, stream);
}

int lcp_body_properties_backward_f64(int B, int nb, int cap, const int32_t* kind, const double* radius, const double* verts_raw,
                                     const int32_t* nverts, const double* mass, double g, const double* g_centroid,
                                     const double* g_verts_local, const double* g_inertia, const float* g_Mdiag, const float* g_f,
                                     double* g_verts_raw, double* g_radius, double* g_mass, void* stream) {
  if (B < 0 || nb < 0 || cap < 8 || cap > 64) return LCP_E_BADARG;
  if (!kind || !radius || !verts_raw || !nverts || !mass) return LCP_E_BADARG;
  if (!g_verts_raw && !g_radius && !g_mass) return LCP_E_BADARG;                                       // (nothing asked for)
  if (B == 0 || nb == 0) return 0;
  return lcp::body_properties_backward_launch(B, nb, cap, kind, radius, verts_raw, nverts, mass, g, g_centroid, g_verts_local,
                                              g_inertia, g_Mdiag, g_f, g_verts_raw, g_radius, g_mass, stream);
}

// what both render entries refuse before any launch: sizes outside the packed vertex list's, a camera without pixels or scale, an
// image whose element index leaves 31 bits, a missing required pointer (thickness is optional: NULL = every body filled)
static bool render_args_ok(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const void* kind, const void* radius,
                           const void* verts_local, const void* nverts, const void* p, const void* colors, const void* background,
                           double ppm, double w) {
  if (B < 1 || !lcp::render_supported(nb, nvcap, scene_verts_max)) return false;
  if (C < 1 || C > 4 || H < 1 || W < 1) return false;
  if ((long long)B * C * H * W >= (1LL << 31)) return false;
  if (!(w > 0.0) || !(ppm > 0.0)) return false;                      // (a NaN fails both)
  return kind && radius && verts_local && nverts && p && colors && background;
}

int lcp_render_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind, const double* radius,
                   const double* verts_local, const int32_t* nverts, const double* p, const float* colors, const float* background,
                   const double* thickness, double x0, double y0, double ppm, double w, float* image, int32_t* ids, void* stream) {
  if (!render_args_ok(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors, background, ppm, w))
    return LCP_E_BADARG;
  if (!image && !ids) return LCP_E_BADARG;                            // (nothing asked for)
  return lcp::render_launch(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors, background, thickness,
                            x0, y0, ppm, w, image, ids, stream);
}

int lcp_render_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind,
                            const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                            const float* colors, const float* background, const double* thickness, double x0, double y0, double ppm,
                            double w, const float* g_image, double* g_p, double* g_radius, double* g_verts_local, float* g_colors,
                            void* stream) {
  if (!render_args_ok(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors, background, ppm, w))
    return LCP_E_BADARG;
  if (!g_image || (!g_p && !g_radius && !g_verts_local && !g_colors)) return LCP_E_BADARG;
  return lcp::render_backward_launch(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors, background,
                                     thickness, x0, y0, ppm, w, g_image, g_p, g_radius, g_verts_local, g_colors, stream);
}

// what the two entries with marks and markers refuse on top of render_args_ok: a joint count outside 0..64, an order other than 0 / 1,
// a width that is not positive, a negative radius (a NaN fails either), marks without colours, joints without one of their arrays
static bool render_marks_ok(const int32_t* mark, const float* mark_colors, int nj, const void* jtype, const void* jb1, const void* jb2,
                            const void* jr1, const void* jrot1, const void* joint_colors, int order, double line_w, double dot_r,
                            double joint_w, double joint_r) {
  if (nj < 0 || nj > 64 || (order != 0 && order != 1)) return false;
  if (!(line_w > 0.0) || !(joint_w > 0.0) || !(dot_r >= 0.0) || !(joint_r >= 0.0)) return false;
  if (mark && !mark_colors) return false;
  return nj == 0 || (jtype && jb1 && jb2 && jr1 && jrot1 && joint_colors);
}

int lcp_render_marks_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind, const double* radius,
                         const double* verts_local, const int32_t* nverts, const double* p, const float* colors, const float* background,
                         const double* thickness, double x0, double y0, double ppm, double w, const int32_t* mark,
                         const float* mark_colors, int nj, const int32_t* jtype, const int32_t* jb1, const int32_t* jb2, const double* jr1,
                         const double* jrot1, const float* joint_colors, int order, double line_w, double dot_r, double joint_w,
                         double joint_r, float* image, int32_t* ids, void* stream) {
  if (!render_args_ok(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors, background, ppm, w))
    return LCP_E_BADARG;
  if (!render_marks_ok(mark, mark_colors, nj, jtype, jb1, jb2, jr1, jrot1, joint_colors, order, line_w, dot_r, joint_w, joint_r))
    return LCP_E_BADARG;
  if (!image && !ids) return LCP_E_BADARG;                            // (nothing asked for)
  const lcp::RenderMarks mk{mark, mark_colors, nj, jtype, jb1, jb2, jr1, jrot1, joint_colors, order, line_w, dot_r, joint_w, joint_r};
  return lcp::render_marks_launch(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors, background,
                                  thickness, x0, y0, ppm, w, mk, image, ids, stream);
}

int lcp_render_marks_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int H, int W, int C, const int32_t* kind,
                                  const double* radius, const double* verts_local, const int32_t* nverts, const double* p,
                                  const float* colors, const float* background, const double* thickness, double x0, double y0, double ppm,
                                  double w, const int32_t* mark, const float* mark_colors, int nj, const int32_t* jtype, const int32_t* jb1,
                                  const int32_t* jb2, const double* jr1, const double* jrot1, const float* joint_colors, int order,
                                  double line_w, double dot_r, double joint_w, double joint_r, const float* g_image, double* g_p,
                                  double* g_radius, double* g_verts_local, float* g_colors, float* g_mark_colors, float* g_joint_colors,
                                  double* g_jrot1, double* g_jr1, double* g_p_joints, void* stream) {
  if (!render_args_ok(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors, background, ppm, w))
    return LCP_E_BADARG;
  if (!render_marks_ok(mark, mark_colors, nj, jtype, jb1, jb2, jr1, jrot1, joint_colors, order, line_w, dot_r, joint_w, joint_r))
    return LCP_E_BADARG;
  if (!g_image || (!g_p && !g_radius && !g_verts_local && !g_colors && !g_mark_colors && !g_joint_colors && !g_jrot1 && !g_jr1))
    return LCP_E_BADARG;
  if (g_p && nj > 0 && !g_p_joints) return LCP_E_BADARG;              // (the joints' pull on their bodies needs its workspace)
  const lcp::RenderMarks mk{mark, mark_colors, nj, jtype, jb1, jb2, jr1, jrot1, joint_colors, order, line_w, dot_r, joint_w, joint_r};
  return lcp::render_marks_backward_launch(B, nb, nvcap, scene_verts_max, H, W, C, kind, radius, verts_local, nverts, p, colors,
                                           background, thickness, x0, y0, ppm, w, mk, g_image, g_p, g_radius, g_verts_local, g_colors,
                                           g_mark_colors, g_joint_colors, g_jrot1, g_jr1, g_p_joints, stream);
}

// what both ray entries refuse before any launch: a negative batch, sizes outside the packed vertex list's, a ray count outside
// 1..1024, a missing scene or ray array
static bool cast_rays_args_ok(int B, int nb, int nvcap, int scene_verts_max, int R, const void* kind, const void* radius,
                              const void* verts_local, const void* nverts, const void* p, const void* ray_body, const void* ray_origin,
                              const void* ray_angle, const void* ray_range) {
  if (B < 0 || !lcp::cast_rays_supported(nb, nvcap, scene_verts_max, R)) return false;
  return kind && radius && verts_local && nverts && p && ray_body && ray_origin && ray_angle && ray_range;
}

int lcp_cast_rays_f64(int B, int nb, int nvcap, int scene_verts_max, int R, const int32_t* kind, const double* radius,
                      const double* verts_local, const int32_t* nverts, const double* p, const int32_t* ray_body,
                      const double* ray_origin, const double* ray_angle, const double* ray_range, double* dist, int32_t* hit,
                      double* normal, void* stream) {
  if (!cast_rays_args_ok(B, nb, nvcap, scene_verts_max, R, kind, radius, verts_local, nverts, p, ray_body, ray_origin, ray_angle, ray_range))
    return LCP_E_BADARG;
  if (!dist && !hit && !normal) return LCP_E_BADARG;                  // (nothing asked for)
  if (B == 0) return 0;
  return lcp::cast_rays_launch(B, nb, nvcap, scene_verts_max, R, kind, radius, verts_local, nverts, p, ray_body, ray_origin, ray_angle,
                               ray_range, dist, hit, normal, stream);
}

int lcp_cast_rays_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int R, const int32_t* kind, const double* radius,
                               const double* verts_local, const int32_t* nverts, const double* p, const int32_t* ray_body,
                               const double* ray_origin, const double* ray_angle, const double* ray_range, const double* g_dist,
                               double* g_p, double* g_radius, double* g_verts_local, double* g_ray_origin, double* g_ray_angle,
                               void* stream) {
  if (!cast_rays_args_ok(B, nb, nvcap, scene_verts_max, R, kind, radius, verts_local, nverts, p, ray_body, ray_origin, ray_angle, ray_range))
    return LCP_E_BADARG;
  if (!g_dist || (!g_p && !g_radius && !g_verts_local && !g_ray_origin && !g_ray_angle)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::cast_rays_backward_launch(B, nb, nvcap, scene_verts_max, R, kind, radius, verts_local, nverts, p, ray_body, ray_origin,
                                        ray_angle, ray_range, g_dist, g_p, g_radius, g_verts_local, g_ray_origin, g_ray_angle, stream);
}

// what both proximity entries refuse before any launch: a negative batch, sizes outside the packed vertex list's, a pair count
// outside 1..1024, a missing scene or pair array
static bool pair_distance_args_ok(int B, int nb, int nvcap, int scene_verts_max, int P, const void* kind, const void* radius,
                                  const void* verts_local, const void* nverts, const void* p, const void* pair_first,
                                  const void* pair_second, const void* pair_max_dist) {
  if (B < 0 || !lcp::pair_distance_supported(nb, nvcap, scene_verts_max, P)) return false;
  return kind && radius && verts_local && nverts && p && pair_first && pair_second && pair_max_dist;
}

int lcp_pair_distance_f64(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                          const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                          const int32_t* pair_second, const double* pair_max_dist, double* dist, double* normal, double* w1, double* w2,
                          void* stream) {
  if (!pair_distance_args_ok(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first, pair_second, pair_max_dist))
    return LCP_E_BADARG;
  if (!dist && !normal && !w1 && !w2) return LCP_E_BADARG;            // (nothing asked for)
  if (B == 0) return 0;
  return lcp::pair_distance_launch(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first, pair_second,
                                   pair_max_dist, dist, normal, w1, w2, stream);
}

int lcp_pair_distance_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                   const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                                   const int32_t* pair_second, const double* pair_max_dist, const double* g_dist, double* g_p,
                                   double* g_radius, double* g_verts_local, void* stream) {
  if (!pair_distance_args_ok(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first, pair_second, pair_max_dist))
    return LCP_E_BADARG;
  if (!g_dist || (!g_p && !g_radius && !g_verts_local)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::pair_distance_backward_launch(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first,
                                            pair_second, pair_max_dist, g_dist, g_p, g_radius, g_verts_local, stream);
}

// what both overlap entries refuse before any launch: what the proximity entries refuse, without a cutoff among the pair arrays
static bool pair_overlap_args_ok(int B, int nb, int nvcap, int scene_verts_max, int P, const void* kind, const void* radius,
                                 const void* verts_local, const void* nverts, const void* p, const void* pair_first,
                                 const void* pair_second) {
  if (B < 0 || !lcp::pair_overlap_supported(nb, nvcap, scene_verts_max, P)) return false;
  return kind && radius && verts_local && nverts && p && pair_first && pair_second;
}

int lcp_pair_overlap_f64(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                         const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                         const int32_t* pair_second, double* area, void* stream) {
  if (!pair_overlap_args_ok(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first, pair_second))
    return LCP_E_BADARG;
  if (!area) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::pair_overlap_launch(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first, pair_second, area,
                                  stream);
}

int lcp_pair_overlap_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                  const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pair_first,
                                  const int32_t* pair_second, const double* g_area, double* g_p, double* g_radius,
                                  double* g_verts_local, void* stream) {
  if (!pair_overlap_args_ok(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first, pair_second))
    return LCP_E_BADARG;
  if (!g_area || (!g_p && !g_radius && !g_verts_local)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::pair_overlap_backward_launch(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, pair_first,
                                           pair_second, g_area, g_p, g_radius, g_verts_local, stream);
}

// what both point-probe entries refuse before any launch: a negative batch, sizes outside the packed vertex list's, a point count
// outside 1..1024, a missing scene or point array
static bool point_distance_args_ok(int B, int nb, int nvcap, int scene_verts_max, int N, const void* kind, const void* radius,
                                   const void* verts_local, const void* nverts, const void* p, const void* pt_body, const void* pt_xy,
                                   const void* pt_target, const void* pt_max_dist) {
  if (B < 0 || !lcp::point_distance_supported(nb, nvcap, scene_verts_max, N)) return false;
  return kind && radius && verts_local && nverts && p && pt_body && pt_xy && pt_target && pt_max_dist;
}

int lcp_point_distance_f64(int B, int nb, int nvcap, int scene_verts_max, int N, const int32_t* kind, const double* radius,
                           const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pt_body,
                           const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist, double* dist, int32_t* body,
                           double* normal, void* stream) {
  if (!point_distance_args_ok(B, nb, nvcap, scene_verts_max, N, kind, radius, verts_local, nverts, p, pt_body, pt_xy, pt_target, pt_max_dist))
    return LCP_E_BADARG;
  if (!dist && !body && !normal) return LCP_E_BADARG;                 // (nothing asked for)
  if (B == 0) return 0;
  return lcp::point_distance_launch(B, nb, nvcap, scene_verts_max, N, kind, radius, verts_local, nverts, p, pt_body, pt_xy, pt_target,
                                    pt_max_dist, dist, body, normal, stream);
}

int lcp_point_distance_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int N, const int32_t* kind, const double* radius,
                                    const double* verts_local, const int32_t* nverts, const double* p, const int32_t* pt_body,
                                    const double* pt_xy, const int32_t* pt_target, const double* pt_max_dist, const double* g_dist,
                                    double* g_p, double* g_radius, double* g_verts_local, double* g_pt_xy, void* stream) {
  if (!point_distance_args_ok(B, nb, nvcap, scene_verts_max, N, kind, radius, verts_local, nverts, p, pt_body, pt_xy, pt_target, pt_max_dist))
    return LCP_E_BADARG;
  if (!g_dist || (!g_p && !g_radius && !g_verts_local && !g_pt_xy)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::point_distance_backward_launch(B, nb, nvcap, scene_verts_max, N, kind, radius, verts_local, nverts, p, pt_body, pt_xy,
                                             pt_target, pt_max_dist, g_dist, g_p, g_radius, g_verts_local, g_pt_xy, stream);
}

// what both time-of-impact entries refuse before any launch: what the proximity entries refuse, with the velocities among the scene arrays
static bool time_of_impact_args_ok(int B, int nb, int nvcap, int scene_verts_max, int P, const void* kind, const void* radius,
                                   const void* verts_local, const void* nverts, const void* p, const void* v, const void* pair_first,
                                   const void* pair_second) {
  if (B < 0 || !lcp::time_of_impact_supported(nb, nvcap, scene_verts_max, P)) return false;
  return kind && radius && verts_local && nverts && p && v && pair_first && pair_second;
}

int lcp_time_of_impact_f64(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                           const double* verts_local, const int32_t* nverts, const double* p, const float* v, const int32_t* pair_first,
                           const int32_t* pair_second, const double* margin, const double* horizon, double tol, int max_iter, double* toi,
                           int32_t* status, double* normal, double* first_toi, int32_t* first_pair, void* stream) {
  if (!time_of_impact_args_ok(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, v, pair_first, pair_second))
    return LCP_E_BADARG;
  if (!margin || !horizon || !(tol > 0.0) || max_iter < 1 || max_iter > 1024) return LCP_E_BADARG;      // (a NaN tol fails too)
  if (!toi && !status && !normal && !first_toi && !first_pair) return LCP_E_BADARG;                     // (nothing asked for)
  if (B == 0) return 0;
  return lcp::time_of_impact_launch(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, v, pair_first, pair_second,
                                    margin, horizon, tol, max_iter, toi, status, normal, first_toi, first_pair, stream);
}

int lcp_time_of_impact_backward_f64(int B, int nb, int nvcap, int scene_verts_max, int P, const int32_t* kind, const double* radius,
                                    const double* verts_local, const int32_t* nverts, const double* p, const float* v,
                                    const int32_t* pair_first, const int32_t* pair_second, const double* toi, const int32_t* status,
                                    const double* g_toi, double* g_p, double* g_v, double* g_radius, double* g_verts_local,
                                    double* g_margin, void* stream) {
  if (!time_of_impact_args_ok(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, v, pair_first, pair_second))
    return LCP_E_BADARG;
  if (!toi || !status || !g_toi || (!g_p && !g_v && !g_radius && !g_verts_local && !g_margin)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::time_of_impact_backward_launch(B, nb, nvcap, scene_verts_max, P, kind, radius, verts_local, nverts, p, v, pair_first,
                                             pair_second, toi, status, g_toi, g_p, g_v, g_radius, g_verts_local, g_margin, stream);
}

// what both force-element entries refuse before any launch: a negative batch, sizes outside the limits, a missing element or state array
static bool force_elements_args_ok(int B, int nb, int E, const void* kind, const void* b1, const void* b2, const void* a1, const void* a2,
                                   const void* k, const void* c, const void* x0, const void* w0, const void* limit, const void* p,
                                   const void* v) {
  if (B < 0 || !lcp::force_elements_supported(nb, E)) return false;
  return kind && b1 && b2 && a1 && a2 && k && c && x0 && w0 && limit && p && v;
}

int lcp_force_elements_f64(int B, int nb, int E, const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1,
                           const double* a2, const double* k, const double* c, const double* x0, const double* w0, const double* limit,
                           const double* p, const float* v, const float* f_base, float* f_out, void* stream) {
  if (!force_elements_args_ok(B, nb, E, kind, b1, b2, a1, a2, k, c, x0, w0, limit, p, v) || !f_out) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::force_elements_launch(B, nb, E, kind, b1, b2, a1, a2, k, c, x0, w0, limit, p, v, f_base, f_out, stream);
}

int lcp_force_elements_backward_f64(int B, int nb, int E, const int32_t* kind, const int32_t* b1, const int32_t* b2, const double* a1,
                                    const double* a2, const double* k, const double* c, const double* x0, const double* w0,
                                    const double* limit, const double* p, const float* v, const float* g_f, double* g_p, double* g_v,
                                    double* g_k, double* g_c, double* g_x0, double* g_w0, double* g_a1, double* g_a2, void* stream) {
  if (!force_elements_args_ok(B, nb, E, kind, b1, b2, a1, a2, k, c, x0, w0, limit, p, v)) return LCP_E_BADARG;
  if (!g_f || (!g_p && !g_v && !g_k && !g_c && !g_x0 && !g_w0 && !g_a1 && !g_a2)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::force_elements_backward_launch(B, nb, E, kind, b1, b2, a1, a2, k, c, x0, w0, limit, p, v, g_f, g_p, g_v, g_k, g_c, g_x0,
                                             g_w0, g_a1, g_a2, stream);
}

// what both link entries refuse before any launch (0: nothing): sizes below their lower limits or a missing array (LCP_E_BADARG), sizes
// beyond the upper limits (LCP_E_TOOLARGE), more link rows than the kinds can have (LCP_E_BADARG)
static int link_jacobian_args(int B, int nb, int L, int e0, int el, const void* kind, const void* first, const void* second,
                              const void* a1, const void* a2, const void* phi, const void* p) {
  if (B < 0 || nb < 1 || L < 1 || e0 < 0 || el < 0) return LCP_E_BADARG;
  if (!kind || !first || !second || !a1 || !a2 || !phi || !p) return LCP_E_BADARG;
  if (!lcp::link_jacobian_supported(nb, L, e0)) return LCP_E_TOOLARGE;
  return el > 2 * L ? LCP_E_BADARG : 0;
}

int lcp_link_jacobian_f64(int B, int nb, int L, int e0, int el, const int32_t* kind, const int32_t* first, const int32_t* second,
                          const double* a1, const double* a2, const double* phi, const double* p, const float* Je_base, float* Je,
                          void* stream) {
  if (int rc = link_jacobian_args(B, nb, L, e0, el, kind, first, second, a1, a2, phi, p)) return rc;
  if (!Je || (e0 > 0 && !Je_base)) return LCP_E_BADARG;
  if (B == 0 || e0 + el == 0) return 0;
  return lcp::link_jacobian_launch(B, nb, L, e0, el, kind, first, second, a1, a2, phi, p, Je_base, Je, stream);
}

int lcp_link_jacobian_backward_f64(int B, int nb, int L, int e0, int el, const int32_t* kind, const int32_t* first,
                                   const int32_t* second, const double* a1, const double* a2, const double* phi, const double* p,
                                   const float* gJe, double* g_p, double* g_a1, double* g_a2, double* g_phi, void* stream) {
  if (int rc = link_jacobian_args(B, nb, L, e0, el, kind, first, second, a1, a2, phi, p)) return rc;
  if (!gJe || (!g_p && !g_a1 && !g_a2 && !g_phi)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::link_jacobian_backward_launch(B, nb, L, e0, el, kind, first, second, a1, a2, phi, p, gJe, g_p, g_a1, g_a2, g_phi, stream);
}

int lcp_contact_report_f32(int B, int nb, int maxc, int e, int P, const int32_t* c_count, const int32_t* active, const float* c_n,
                           const float* c_p1, const float* c_p2, const int32_t* c_i1, const int32_t* c_i2, const float* z, const float* y,
                           const float* Je, const int32_t* pair_first, const int32_t* pair_second, double min_impulse,
                           float* body_impulse, float* body_normal, int32_t* body_touching, float* joint_impulse, float* pair_impulse,
                           float* pair_normal, int32_t* pair_contacts, void* stream) {
  if (B < 0 || nb < 1 || maxc < 1 || e < 0 || P < 0) return LCP_E_BADARG;
  if (!c_n || !c_p1 || !c_p2 || !c_i1 || !c_i2 || !z) return LCP_E_BADARG;
  if (P > 0 && (!pair_first || !pair_second)) return LCP_E_BADARG;
  if (!body_impulse && !body_normal && !body_touching && !joint_impulse && !pair_impulse && !pair_normal && !pair_contacts)
    return LCP_E_BADARG;
  if (!lcp::contact_report_supported(nb, maxc, P)) return LCP_E_TOOLARGE;
  if (B == 0) return 0;
  return lcp::contact_report_launch(B, nb, maxc, e, P, c_count, active, c_n, c_p1, c_p2, c_i1, c_i2, z, y, Je, pair_first, pair_second,
                                    min_impulse, body_impulse, body_normal, body_touching, joint_impulse, pair_impulse, pair_normal,
                                    pair_contacts, stream);
}

// the layout words of lcp_extract_params_u8 against an H x W image (include/lcp_hip.h lists what is refused)
static bool encoder_layout_ok(const int32_t* w, int H, int W) {
  const int paddle_line = w[0], paddle_h = w[1], paddle_w = w[2], paddle_key = w[3], ball_w = w[4], nrows = w[5], band_top = w[6],
            band_h = w[7], ball_key = w[20];
  auto key = [](int k) { return k >= 1 && k <= 255; };
  if (!key(paddle_key) || !key(ball_key) || nrows < 0 || nrows > 8) return false;
  for (int i = 0; i < nrows; ++i)
    if (!key(w[8 + i])) return false;
  if (band_h < 1 || paddle_w < 1 || paddle_h < 0 || ball_w < 0) return false;
  if (paddle_line < 0 || paddle_line >= H || band_top < 0 || band_top >= H) return false;
  if ((long long)band_top + (long long)nrows * band_h > paddle_line) return false;          // (every top line lies above it)
  if (paddle_h > (1 << 20) || paddle_w > (1 << 20) || ball_w > (1 << 20)) return false;      // (sums with a column stay in 31 bits)
  return w[16] >= 0 && w[17] >= 0 && w[18] >= w[16] && w[19] >= w[17];
}

int lcp_extract_params_u8(int B, int H, int W, const uint8_t* frame, int64_t stride_b, int64_t stride_row, int64_t stride_col,
                          const int32_t* layout, int max_blocks, int32_t* paddle, int32_t* blocks, int32_t* nblocks, int32_t* ball,
                          int32_t* status, double* paddle_params, double* block_params, double* ball_params, void* stream) {
  if (B < 0 || H < 1 || H > (1 << 20) || W < 1 || W > 1024 || max_blocks < 1 || max_blocks > 256) return LCP_E_BADARG;
  if (!frame || !layout || stride_b < 1 || stride_row < 1 || stride_col < 1) return LCP_E_BADARG;
  if (!paddle && !blocks && !nblocks && !ball && !status && !paddle_params && !block_params && !ball_params) return LCP_E_BADARG;
  if (!encoder_layout_ok(layout, H, W)) return LCP_E_BADARG;
  if (B == 0) return 0;
  return lcp::extract_params_launch(B, H, W, frame, stride_b, stride_row, stride_col, layout, max_blocks, paddle, blocks, nblocks, ball,
                                    status, paddle_params, block_params, ball_params, stream);
}

}  // extern "C"
