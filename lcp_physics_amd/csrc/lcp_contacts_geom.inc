// lcp_contacts_geom.inc - the narrow-phase geometry of DiffContactHandler (physics/contacts.py:57-352), written once over
// the scalar type LCP_S and included twice by lcp_contacts.hip: with LCP_S = double (the detection kernel) and with
// LCP_S = Dual (value + one directional derivative: the forward-mode derivative of the contact frame with respect to a
// pose coordinate, for lcp_contact_frame_backward_f64).  Branches are taken on the VALUES, so the derivative is the one
// autograd gives the reference: along the branch the forward pass took.
// A body's vertex / normal / edge-length arrays are read through the types VRef and SRef: plain pointers unless the includer
// defines LCP_GEOM_VREF / LCP_GEOM_SREF (types with operator[](int) returning V2 / LCP_S; lcp_contacts_wide.hip forms the dual
// vertices of its frame backward on read from staged values that way).
// With LCP_GEOM_TRACE defined, the first record of a pair also names the vertices it was built from (lcp_contacts_shape.hip
// seeds its derivative with respect to the shape with them); nothing else changes, and without the macro nothing at all.
struct V2 { LCP_S x, y; };
__device__ __forceinline__ V2 v2(LCP_S x, LCP_S y) { V2 r; r.x = x; r.y = y; return r; }
__device__ __forceinline__ V2 operator+(V2 a, V2 b) { return v2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ V2 operator-(V2 a, V2 b) { return v2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ V2 operator-(V2 a) { return v2(-a.x, -a.y); }
__device__ __forceinline__ V2 operator*(V2 a, LCP_S s) { return v2(a.x * s, a.y * s); }
__device__ __forceinline__ V2 operator*(LCP_S s, V2 a) { return v2(a.x * s, a.y * s); }
__device__ __forceinline__ LCP_S dot(V2 a, V2 b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ LCP_S norm(V2 a) { return sqrt(a.x * a.x + a.y * a.y); }
__device__ __forceinline__ V2 left_orth(V2 v) { return v2(v.y, -v.x); }              // utils.py:99-102

#ifdef LCP_GEOM_VREF
typedef LCP_GEOM_VREF VRef;
#else
typedef const V2* VRef;
#endif
#ifdef LCP_GEOM_SREF
typedef LCP_GEOM_SREF SRef;
#else
typedef const LCP_S* SRef;
#endif

struct Body {             // world frame
  int kind;               // 0 circle, 1 hull
  V2 pos;
  LCP_S rad;
  int nv;
  VRef verts;             // hull vertices relative to pos, rotated (LDS)
  VRef nrm;               // outward unit normal of edge k = (verts[k], verts[k+1])  (LDS, formed once per trial pose)
  SRef elen;              // length of edge k
};

#ifdef LCP_GEOM_TRACE
// tref: the body of the pair (0 / 1) that owns the vertices tr0, tr1 (the reference edge of hull / hull; the GJK simplex or the
// SAT edge of the hull of circle / hull); ti0, ti1: the incident edge's vertices, on the other body.  -1: none.
struct Pt { V2 n, p1, p2; LCP_S pen; int tref, tr0, tr1, ti0, ti1; };
#define LCP_TRACE(pt, b, r0, r1, i0, i1) do { (pt).tref = (b); (pt).tr0 = (r0); (pt).tr1 = (r1); (pt).ti0 = (i0); (pt).ti1 = (i1); } while (0)
#else
struct Pt { V2 n, p1, p2; LCP_S pen; };
#define LCP_TRACE(pt, b, r0, r1, i0, i1) do { } while (0)
#endif

// contacts.py:207-217 (`>=`: last maximiser wins)
__device__ __forceinline__ int support(VRef pts, int n, V2 dir) {
  int best = -1; LCP_S bn = -1.0;
  for (int i = 0; i < n; ++i) { const LCP_S c = dot(pts[i], dir); if (c >= bn) { bn = c; best = i; } }
  return best;
}

__device__ __forceinline__ int circle_circle(const Body& b1, const Body& b2, double eps, Pt& out0) {   // contacts.py:68-79
  const LCP_S r = b1.rad + b2.rad;
  V2 n = b1.pos - b2.pos;
  const LCP_S dist = norm(n);
  const LCP_S pen = r - dist;
  if (pen < -eps) return 0;
  n = n * (1.0 / dist);
  out0.n = n; out0.p1 = -n * (b1.rad - pen / 2); out0.p2 = n * (b2.rad - pen / 2); out0.pen = pen;
  LCP_TRACE(out0, 0, -1, -1, -1, -1);
  return 1;
}

__device__ __forceinline__ void bary2(V2 p, V2 a, V2 b, LCP_S& u, LCP_S& v) {        // contacts.py:334-340
  const V2 d = b - a;
  const LCP_S n = norm(d);
  const V2 nd = d * (1.0 / n);
  u = dot(b - p, nd) / n; v = dot(p - a, nd) / n;
}
__device__ __forceinline__ void bary3(V2 p, V2 a, V2 b, V2 c, LCP_S& u, LCP_S& v, LCP_S& w) {   // contacts.py:341-350
  // inverse of [[ax,bx,cx],[ay,by,cy],[1,1,1]] applied to (px,py,1)
  const LCP_S det = a.x * (b.y - c.y) - b.x * (a.y - c.y) + c.x * (a.y - b.y);
  const LCP_S id = 1.0 / det;
  u = ((b.y - c.y) * p.x + (c.x - b.x) * p.y + (b.x * c.y - c.x * b.y)) * id;
  v = ((c.y - a.y) * p.x + (a.x - c.x) * p.y + (c.x * a.y - a.x * c.y)) * id;
  w = ((a.y - b.y) * p.x + (b.x - a.x) * p.y + (a.x * b.y - b.x * a.y)) * id;
}

// (no private arrays anywhere below: dynamically indexed locals live in scratch memory on this target, and a scratch
//  round trip costs as much as the whole arithmetic of a pair - the simplex, clip and manifold buffers are named scalars)
struct Simplex { V2 a, b, c; int ia, ib, ic; int n; };     // up to 3 points with their vertex indices

// contacts.py:295-330: closest point of the simplex to p; `keep` = the sub-simplex that supports it (the reference's
// `ids_used`, in its order), keep.n == 3 means p is inside the triangle
__device__ __forceinline__ V2 closest(V2 p, const Simplex& sx, Simplex& keep) {
  keep = sx;
  if (sx.n == 1) return sx.a;
  if (sx.n == 2) {
    LCP_S u, v; bary2(p, sx.a, sx.b, u, v);
    if (u <= 0) { keep.a = sx.b; keep.ia = sx.ib; keep.n = 1; return sx.b; }
    if (v <= 0) { keep.n = 1; return sx.a; }
    return u * sx.a + v * sx.b;
  }
  LCP_S uAB, vAB, uBC, vBC, uCA, vCA, uABC, vABC, wABC;
  bary2(p, sx.a, sx.b, uAB, vAB); bary2(p, sx.b, sx.c, uBC, vBC); bary2(p, sx.c, sx.a, uCA, vCA);
  bary3(p, sx.a, sx.b, sx.c, uABC, vABC, wABC);
  if (vAB <= 0 && uCA <= 0) { keep.n = 1; return sx.a; }
  if (vBC <= 0 && uAB <= 0) { keep.a = sx.b; keep.ia = sx.ib; keep.n = 1; return sx.b; }
  if (vCA <= 0 && uBC <= 0) { keep.a = sx.c; keep.ia = sx.ic; keep.n = 1; return sx.c; }
  if (uAB > 0 && vAB > 0 && wABC <= 0) { keep.n = 2; return uAB * sx.a + vAB * sx.b; }
  if (uBC > 0 && vBC > 0 && uABC <= 0) { keep.a = sx.b; keep.ia = sx.ib; keep.b = sx.c; keep.ib = sx.ic; keep.n = 2; return uBC * sx.b + vBC * sx.c; }
  if (uCA > 0 && vCA > 0 && vABC <= 0) { keep.a = sx.c; keep.ia = sx.ic; keep.b = sx.a; keep.ib = sx.ia; keep.n = 2; return uCA * sx.c + vCA * sx.a; }
  return p;                                                      // inside (the reference raises if nothing matched)
}

// contacts.py:80-141: `circ` plays b1, `hull` b2
__device__ __forceinline__ int circle_hull(const Body& circ, const Body& hull, double eps, bool circle_is_g2, Pt& out0) {
  const VRef verts = hull.verts;
  const int nv = hull.nv;
  const V2 tp = circ.pos - hull.pos;
  Simplex sx, keep;
  sx.a = verts[0]; sx.ia = 0; sx.b = sx.a; sx.c = sx.a; sx.ib = -1; sx.ic = -1; sx.n = 1;
  keep = sx;
  V2 cl = sx.a;
  for (int iter = 0; iter < 4 * NV; ++iter) {
    cl = closest(tp, sx, keep);
    if (keep.n == 3) break;
    V2 sd;
    if (keep.n == 2) {
      sd = left_orth(keep.a - keep.b);
      if (dot(sd, tp - keep.a) < 0) sd = -sd;
    } else {
      sd = tp - cl;
    }
    if (sd.x == 0 && sd.y == 0) break;
    const int si = support(verts, nv, sd);
    const bool in_simplex = (si == sx.ia) || (sx.n > 1 && si == sx.ib) || (sx.n > 2 && si == sx.ic);
    if (in_simplex) break;
    sx = keep;                                                   // the used points, then the new support point
    if (keep.n == 1) { sx.b = verts[si]; sx.ib = si; } else { sx.c = verts[si]; sx.ic = si; }
    sx.n = keep.n + 1;
  }
  V2 bn, bp1, bp2; LCP_S bd;
  LCP_TRACE(out0, circle_is_g2 ? 0 : 1, keep.ia, keep.n == 2 ? keep.ib : -1, -1, -1);
  if (keep.n < 3) {
    bp2 = cl;
    const V2 cw = cl + hull.pos;
    bp1 = cw - circ.pos;
    bd = norm(cw - circ.pos) - circ.rad;
    if (bd > eps) return 0;
    bn = -bp1 * (1.0 / norm(bp1));
  } else {                                     // centre inside the hull: SAT, contacts.py:114-137
    bd = -1e10; bn = v2(0, 0); bp1 = bn; bp2 = bn;
    for (int idx = 0; idx < nv; ++idx) {
      const V2 nrm = hull.nrm[idx];
      const V2 center = circ.pos - hull.pos;
      const LCP_S dist = dot(nrm, center - verts[idx]) - circ.rad;
      if (dist > bd) {
        if (dist > eps) return 0;
        bd = dist; bn = nrm;
        bp2 = center + nrm * -(dist + circ.rad);
        bp1 = bp2 + hull.pos - circ.pos;
        LCP_TRACE(out0, circle_is_g2 ? 0 : 1, idx, (idx + 1) % nv, -1, -1);
      }
    }
  }
  if (circle_is_g2) { bn = -bn; const V2 t = bp1; bp1 = bp2; bp2 = t; }
  out0.n = bn; out0.p1 = bp1; out0.p2 = bp2; out0.pen = -bd;
  return 1;
}

struct Sep { LCP_S dist; V2 normal; int vertex; LCP_S edge_norm; int edge; };

__device__ __forceinline__ Sep test_separations(const Body& h1, const Body& h2, double eps) {      // contacts.py:220-250
  Sep best; best.dist = -1e10; best.normal = v2(0, 0); best.vertex = -1; best.edge_norm = 0; best.edge = 0;
  for (int idx = 0; idx < h1.nv; ++idx) {
    const LCP_S en = h1.elen[idx];
    const V2 nrm = h1.nrm[idx];
    const int si = support(h2.verts, h2.nv, -nrm);
    const V2 sp = h2.verts[si] + h2.pos - h1.pos;
    const LCP_S dist = dot(nrm, sp - h1.verts[idx]);
    if (dist > best.dist) {
      if (dist > eps) { best.dist = dist; best.edge = idx; return best; }
      best.dist = dist; best.normal = -nrm; best.vertex = si; best.edge_norm = en; best.edge = idx;
    }
  }
  return best;
}

__device__ __forceinline__ int incident_edge(V2 ref_normal, const Body& inc, int inc_vertex) {      // contacts.py:253-268
  LCP_S min_dot = 1e10; int best = -1;
  const int e0 = (inc_vertex - 1 + inc.nv) % inc.nv;
  for (int q = 0; q < 2; ++q) {
    const int i = q == 0 ? e0 : inc_vertex;
    const V2 inrm = inc.nrm[i];
    const LCP_S d = dot(ref_normal, inrm);
    if (d < min_dot) { min_dot = d; best = i; }
  }
  return best;
}

__device__ __forceinline__ int clip(V2 in0, V2 in1, V2 nrm, LCP_S offset, V2& o0, V2& o1) {       // contacts.py:270-292
  int n = 0;
  const LCP_S d0 = dot(nrm, in0) + offset, d1 = dot(nrm, in1) + offset;
  o0 = in0; o1 = in1;
  if (d0 >= 0.0) { o0 = in0; n = 1; }
  if (d1 >= 0.0) { if (n == 0) o0 = in1; else o1 = in1; ++n; }
  if (d0 * d1 < 0.0 || n < 2) {
    const LCP_S interp = d0 / (d0 - d1);
    const V2 x = in0 + interp * (in1 - in0);
    if (n == 0) o0 = x; else if (n == 1) o1 = x;             // (never a third point: two kept vertices imply d0 d1 >= 0)
    ++n;
  }
  return n;
}

__device__ __forceinline__ int hull_hull(const Body& b1, const Body& b2, double eps, Pt& out0, Pt& out1) {  // contacts.py:142-201
  const Sep c1 = test_separations(b1, b2, eps);
  if (c1.dist > eps) return 0;
  const Sep c2 = test_separations(b2, b1, eps);
  if (c2.dist > eps) return 0;
  const bool ref_is_b2 = c2.dist > c1.dist;
  const Body& ref = ref_is_b2 ? b2 : b1;
  const Body& inc = ref_is_b2 ? b1 : b2;
  const Sep& c = ref_is_b2 ? c2 : c1;
  const V2 nrm = -c.normal;
  const LCP_S half_edge = c.edge_norm / 2;
  const int ie = incident_edge(nrm, inc, c.vertex);
  const V2 iv0 = inc.verts[ie] + inc.pos - ref.pos;
  const V2 iv1 = inc.verts[(ie + 1) % inc.nv] + inc.pos - ref.pos;
  const V2 plane = left_orth(nrm);
  V2 a0, a1, q0, q1;
  const int n1 = clip(iv0, iv1, plane, half_edge, a0, a1);
  if (n1 < 2) return 0;
  const int n2 = clip(a0, a1, -plane, half_edge, q0, q1);
  int n = 0;
  const V2 refv = ref.verts[c.edge];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const V2 cq = q == 0 ? q0 : q1;
    const LCP_S dist = dot(nrm, cq - refv);
    if (q < n2 && dist <= eps) {
      const V2 pt1 = cq + nrm * -dist;
      const V2 pt2 = pt1 + ref.pos - inc.pos;
      Pt r;
      if (ref_is_b2) { r.n = nrm; r.p1 = pt2; r.p2 = pt1; }                        // contacts.py:170-175
      else { r.n = -nrm; r.p1 = pt1; r.p2 = pt2; }                                 // contacts.py:198-201
      r.pen = -dist;
      if (n == 0) out0 = r; else out1 = r;
      ++n;
    }
  }
  if (n > 0) LCP_TRACE(out0, ref_is_b2 ? 1 : 0, c.edge, (c.edge + 1) % ref.nv, ie, (ie + 1) % inc.nv);
  return n;
}

__device__ __forceinline__ int collide_pair(const Body& b1, const Body& b2, double eps, Pt& out0, Pt& out1) {   // contacts.py:57-205
  const bool c1 = b1.kind == 0, c2 = b2.kind == 0;
  if (c1 && c2) return circle_circle(b1, b2, eps, out0);
  if (c1) return circle_hull(b1, b2, eps, false, out0);
  if (c2) return circle_hull(b2, b1, eps, true, out0);
  return hull_hull(b1, b2, eps, out0, out1);
}
#undef LCP_TRACE
