"""Time the drawing with marks and joint markers (lcp_render_marks.hip through `physics.render.render(marks=, joints=)`) against
(b) the plain drawing of the same scene without them (lcp_render.hip), in the same process, and (c) the same formulas
(include/lcp_hip.h, "drawing") as vectorised torch operations on the same device with torch's autograd as their backward - the
comparison partner of tools/bench_render.py with the marks' and markers' layers added the way a user would write them (kinds, codes
and joint types known on the host, one pass per layer).

    python tools/bench_render_marks.py [--out profiles/render_marks.json]                 # needs the GPU
    python tools/bench_render_marks.py --resources-only [--parent-asm FILE] [--out ...]   # no GPU: (re)fill the kernels' register /
                                                   # scratch / LDS use from lcp_physics_amd/csrc/asm/lcp_render_marks.fixed.s and,
                                                   # with --parent-asm, whether asm/lcp_render.fixed.s is byte for byte that file

The two shapes of profiles/render.json (C = 3): A - 4096 scenes x 64 x 64 of a floor, two boxes and a circle, a mark on every body
and three joints (the floor's TOTAL, a revolute joint on a box, a weld of the other box and the circle); B - 256 scenes x 210 x 160 of
the breakout layout, a mark on every one of the 40 bodies, no joints.  Marks over their bodies (the bodies are filled).  Forward
(into a preallocated tensor) and forward + backward (a random cotangent; all the gradients each route has), HIP events around
windows of at least 0.2 s after a spin-up, the three routes alternating, the median of 7 windows and their spread.  Before anything
is timed the routes are checked against each other: (a) against (c) in values and gradients, (a) without marks and joints against
(b) bit for bit.
"""
import argparse
import hashlib
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_render as BR                                                 # noqa: E402  (shapes, windows, the bodies' torch formulas)

ASM_DIR = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm")
F64 = torch.float64
SPOKE, CENTRE, DIAGONALS = 1, 2, 3
JOINT, FIXED, XCON, YCON, ROTCON, TOTAL = 1, 2, 3, 4, 5, 6


def _segment(ax, ay, bx, by, X, Y):
    """Distance from the segment A -> B ([B] each) at every pixel, [B,H,W] (A != B in these shapes)."""
    e = lambda t: t.reshape(-1, 1, 1)
    qx, qy, ex, ey = X - e(ax), Y - e(ay), e(bx - ax), e(by - ay)
    t = ((qx * ex + qy * ey) / (ex * ex + ey * ey)).clamp(0.0, 1.0)
    return torch.sqrt((qx - t * ex) ** 2 + (qy - t * ey) ** 2)


def torch_render_marks(nvs, thick, codes, joints, sizes, radius, verts, p, colors, mcol, jcol, jr1, jrot1, background, X, Y, w):
    """bench_render.torch_render with, over every body, its mark, and then the joints' markers: the comparison partner."""
    B, C = p.shape[0], colors.shape[-1]
    line_w, dot_r, joint_w, joint_r = sizes
    cov = lambda d: (0.5 - d / w).clamp(0.0, 1.0)
    e = lambda t: t.reshape(B, 1, 1)
    state = {"img": background.to(F64).reshape(1, C, 1, 1).expand(B, C, *X.shape)}

    def paint(a, col):
        a = a.unsqueeze(1)
        state["img"] = state["img"] * (1 - a) + a * col.to(F64).reshape(B, C, 1, 1)

    for k, nv in enumerate(nvs):
        cx, cy = p[:, k, 1], p[:, k, 2]
        sn, cs = torch.sin(p[:, k, 0]), torch.cos(p[:, k, 0])
        if nv == 0:
            d = torch.sqrt((X - e(cx)) ** 2 + (Y - e(cy)) ** 2) - e(radius[:, k])
        else:
            vx, vy = verts[:, k, :nv, 0], verts[:, k, :nv, 1]
            wx, wy = cx.unsqueeze(1) + (cs.unsqueeze(1) * vx - sn.unsqueeze(1) * vy), cy.unsqueeze(1) + (sn.unsqueeze(1) * vx + cs.unsqueeze(1) * vy)
            ex, ey = torch.roll(wx, -1, 1) - wx, torch.roll(wy, -1, 1) - wy
            L = torch.sqrt(ex * ex + ey * ey)
            e4 = lambda t: t.reshape(B, 1, 1, nv)
            qx, qy = X.unsqueeze(-1) - e4(wx), Y.unsqueeze(-1) - e4(wy)
            m = (e4(ey / L) * qx - e4(ex / L) * qy).max(-1).values
            t = ((qx * e4(ex) + qy * e4(ey)) / e4(L * L)).clamp(0.0, 1.0)
            dist = torch.sqrt((qx - t * e4(ex)) ** 2 + (qy - t * e4(ey)) ** 2).min(-1).values
            d = torch.where(m <= 0, m, dist)
        paint(cov(d) - cov(d + thick[k]) if thick[k] > 0 else cov(d), colors[:, k])
        if codes[k] == SPOKE and nv == 0:
            paint(cov(_segment(cx, cy, cx + radius[:, k] * cs, cy + radius[:, k] * sn, X, Y) - line_w / 2), mcol[:, k])
        elif codes[k] == CENTRE:
            paint(cov(torch.sqrt((X - e(cx)) ** 2 + (Y - e(cy)) ** 2) - dot_r), mcol[:, k])
        elif codes[k] == DIAGONALS and nv == 4:
            for a, b in ((0, 2), (1, 3)):
                paint(cov(_segment(wx[:, a], wy[:, a], wx[:, b], wy[:, b], X, Y) - line_w / 2), mcol[:, k])
    for j, (jt, b1, b2) in enumerate(joints):
        x1, y1 = p[:, b1, 1], p[:, b1, 2]
        tick = lambda ax, ay, bx, by: paint(cov(_segment(ax, ay, bx, by, X, Y) - joint_w / 2), jcol[:, j])

        def ring():
            d = torch.sqrt((X - e(x1)) ** 2 + (Y - e(y1)) ** 2) - joint_r
            paint(cov(d) - cov(d + line_w), jcol[:, j])

        if jt == JOINT:
            ax, ay = x1 + jr1[:, j] * torch.cos(jrot1[:, j]), y1 + jr1[:, j] * torch.sin(jrot1[:, j])
            paint(cov(torch.sqrt((X - e(ax)) ** 2 + (Y - e(ay)) ** 2) - dot_r), jcol[:, j])
        elif jt == FIXED:
            tick(x1, y1, p[:, b2, 1], p[:, b2, 2])
        if jt in (ROTCON, TOTAL):
            ring()
        if jt in (YCON, TOTAL):
            tick(x1 - joint_r, y1, x1 + joint_r, y1)
        if jt in (XCON, TOTAL):
            tick(x1, y1 - joint_r, x1, y1 + joint_r)
    return state["img"].to(torch.float32)


def measure(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.joints import JointSet
    from lcp_physics_amd.physics.render import render
    ins, info = BR.make_shape(name, dev)
    geom, cam, B, chunk, nb = ins["geom"], ins["cam"], info["B"], ins["chunk"], info["nb"]
    ppm = cam.pixels_per_meter
    sizes = (1.0 / ppm, 2.0 / ppm, 2.0 / ppm, 5.0 / ppm)                       # the reference's pixel sizes
    codes = [SPOKE if nv == 0 else DIAGONALS for nv in ins["nvs"]]
    joints = [(TOTAL, 0, -1), (JOINT, 1, -1), (FIXED, 2, 3)] if name.startswith("A_") else []
    nj = len(joints)
    rng = np.random.default_rng(9)
    t = lambda a, dt_: torch.tensor(np.asarray(a), dtype=dt_, device=dev).contiguous()
    marks = t(np.broadcast_to(np.asarray(codes, np.int32), (B, nb)).copy(), torch.int32)
    mcol, jcol = t(rng.uniform(0, 1, (B, nb, 3)), torch.float32), t(rng.uniform(0, 1, (B, nj, 3)), torch.float32)
    jr1, jrot1 = t(rng.uniform(10.0, 14.0, (B, nj)), F64), t(rng.uniform(0.0, 6.0, (B, nj)), F64)
    col = lambda q: t(np.broadcast_to(np.asarray([jn[q] for jn in joints], np.int32), (B, nj)).copy(), torch.int32)
    kw = dict(background=ins["background"], thickness=ins["thickness"])
    out = torch.empty(B, 3, info["H"], info["W"], dtype=torch.float32, device=dev)
    leaves = [x.clone().requires_grad_(True) for x in (ins["p"], geom.radius, geom.verts_local, ins["colors"], mcol, jcol, jrot1, jr1)]
    lgeom = GeometryBatch(geom.kind, leaves[1], leaves[2], geom.nverts, None, geom.scene_verts_max)

    def mk(jr, jrot, jc, mc):
        d = dict(kw, marks=marks, mark_colors=mc, marks_over=True)
        if nj:
            d.update(joints=JointSet(col(0), col(1), col(2), jr, jrot.detach().clone(), 0), jrot1=jrot, joint_colors=jc)
        return d

    mkw, lkw = mk(jr1, jrot1, jcol, mcol), mk(leaves[7], leaves[6], leaves[5], leaves[4])

    def t_part(x, s):
        p, radius, verts, colors, mc, jc, jrot, jr = x
        return torch_render_marks(ins["nvs"], ins["thick"], codes, joints, sizes, radius[s], verts[s], p[s], colors[s], mc[s], jc[s], jr[s],
                                  jrot[s], ins["background"], ins["X"], ins["Y"], ins["w"])

    const = (ins["p"], geom.radius, geom.verts_local, ins["colors"], mcol, jcol, jrot1, jr1)

    def fwd(route):
        with torch.no_grad():
            if route == "marks":
                return render(geom, ins["p"], cam, ins["colors"], out=out, **mkw)
            if route == "plain":
                return render(geom, ins["p"], cam, ins["colors"], out=out, **kw)
            for lo in range(0, B, chunk):
                out[lo:lo + chunk] = t_part(const, slice(lo, lo + chunk))
            return out

    def both(route):
        for x in leaves:
            x.grad = None
        if route == "marks":
            render(lgeom, leaves[0], cam, leaves[3], **lkw).backward(ins["g"])
        elif route == "plain":
            render(lgeom, leaves[0], cam, leaves[3], **kw).backward(ins["g"])
        else:
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                t_part(leaves, s).backward(ins["g"][s])

    # the routes compute the same thing (values and gradients) before anything is timed
    live = [i for i, x in enumerate(leaves) if x.numel()]
    ki, ti = fwd("marks").clone(), fwd("torch").clone()
    both("marks")
    kg = [leaves[i].grad.clone() for i in live]
    both("torch")
    tg = [leaves[i].grad.clone() for i in live]
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1.0))
    agree = max([rel(ki, ti)] + [rel(a, b) for a, b in zip(kg, tg)])
    assert agree < 1e-5, "the routes disagree: %g" % agree
    pi = fwd("plain").clone()
    with torch.no_grad():
        bare = render(geom, ins["p"], cam, ins["colors"], marks=torch.zeros_like(marks), **kw)
    assert torch.equal(bare, pi), "the marks kernel without marks is not the plain drawing"
    changed = int(((ki - pi).abs().amax(1) > 1e-3).sum())
    assert changed > 0
    torch.cuda.synchronize()
    fns = {}
    for r in ("marks", "plain", "torch"):
        fns[r + "_forward"] = (lambda r=r: fwd(r))
        fns[r + "_forward_backward"] = (lambda r=r: both(r))
    for fn in fns.values():                                                             # spin-up: clocks, code objects, allocator
        BR.window(fn, 0.3)
    runs = {k: [] for k in fns}
    for _ in range(7):                                                                  # alternating
        for k, fn in fns.items():
            runs[k].append(BR.window(fn))
    res = dict(info, nj=nj, marks_over=True, routes_agree_rel=agree, pixels_changed_by_marks=changed)
    for k, v in runs.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        res[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    for what in ("forward", "forward_backward"):
        res["marks_over_plain_" + what] = round(res["marks_%s_us" % what] / res["plain_%s_us" % what], 4)
        res["marks_over_torch_" + what] = round(res["marks_%s_us" % what] / res["torch_%s_us" % what], 5)
    return res


def kernel_resources():
    """Registers, scratch and static LDS of the kernels of lcp_render_marks.hip, from the metadata of the assembly the build left."""
    path = os.path.join(ASM_DIR, "lcp_render_marks.fixed.s")
    if not os.path.exists(path):
        return None
    keys = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
            "group_segment_fixed_size")
    blocks = []
    for line in open(path):
        m = re.match(r"  (- | {2})\.(\w+):\s+(\S+)", line)                # a kernel's metadata: "  - .first_key:" then "    .key:" lines
        if not m:
            continue
        if m.group(1) == "- ":
            blocks.append({})
        if blocks:
            blocks[-1][m.group(2)] = m.group(3)
    out = {}
    for b in blocks:
        n = b.get("name", "")
        if "lcp_render_marks" in n:
            out["gather" if "gather" in n else "backward" if "backward" in n else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


def asm_identity(parent):
    """Whether the build's asm/lcp_render.fixed.s is byte for byte `parent` (the same unit built from the parent commit at the same
    path: the compilation-unit id in the assembly is a hash of path and options)."""
    mine = os.path.join(ASM_DIR, "lcp_render.fixed.s")
    sha = lambda f: hashlib.sha256(open(f, "rb").read()).hexdigest()
    return {"unit": "lcp_render.hip", "sha256": sha(mine), "parent_sha256": sha(parent), "byte_identical_to_parent": sha(mine) == sha(parent)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_marks.json"))
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--parent-asm", default=None)
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if not a.resources_only:
        assert torch.cuda.is_available(), "bench_render_marks.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc.update({"device": torch.cuda.get_device_name(0),
                    "shapes": {n: measure(n, dev) for n in ("A_4096x64x64_4bodies", "B_256x210x160_breakout40")}})
    res = kernel_resources()
    if res is not None or "kernels" not in doc:
        doc["kernels"] = res
    if a.parent_asm:
        doc["lcp_render_asm"] = asm_identity(a.parent_asm)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
