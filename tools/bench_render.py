"""Time the drawing (lcp_render.hip through `physics.render.render`) against the route a user had before it existed: the same
formulas (include/lcp_hip.h, "drawing") as vectorised torch operations on the same device, with torch's autograd as their backward.
The torch composition exists here only as the comparison partner; it is written the way a user would write it - one pass per body
over [scenes, H, W, vertices] tensors, the kind and vertex count of each body known on the host (no masks) - and runs over the
scenes in chunks where the intermediates of the whole batch would not fit the device.

    python tools/bench_render.py [--out profiles/render.json]        # needs the GPU
    python tools/bench_render.py --resources-only [--out ...]        # no GPU: (re)fill the kernels' register / scratch / LDS use
                                                                     # from lcp_physics_amd/csrc/asm/lcp_render.fixed.s

Shapes (C = 3): A - 4096 scenes x 64 x 64 of a floor, two boxes and a circle; B - 256 scenes x 210 x 160 of the breakout layout of
the reference's experiments/breakout/encoder.py (ball, paddle, two walls, roof, two stoppers and 33 blocks in six rows: 40 bodies),
every pose jittered per scene.  Forward (image only, into a preallocated tensor) and forward + backward (a random cotangent;
gradients of pose, radii, vertices and colours), HIP events around windows of at least 0.2 s after a spin-up, the two routes
alternating, the median of 7 windows and their spread.  Bytes: the image the forward has to write, over the kernel route's time,
as a fraction of 8 TB/s - the floor of the forward.
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12
ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_render.fixed.s")
F64 = torch.float64


def torch_render(nvs, thick, radius, verts, p, colors, background, X, Y, w):
    """The formulas as batched torch operations (differentiable by autograd): the comparison partner.  nvs[k]: the vertex count of
    body k (0: a circle), thick[k]: its thickness - host values, the same in every scene."""
    B = p.shape[0]
    C = colors.shape[-1]
    cov = lambda d: (0.5 - d / w).clamp(0.0, 1.0)
    img = background.to(F64).reshape(1, C, 1, 1).expand(B, C, *X.shape)
    for k, nv in enumerate(nvs):
        cx, cy = p[:, k, 1].reshape(B, 1, 1), p[:, k, 2].reshape(B, 1, 1)
        if nv == 0:
            d = torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2) - radius[:, k].reshape(B, 1, 1)
        else:
            sn, cs = torch.sin(p[:, k, 0:1]), torch.cos(p[:, k, 0:1])
            vx, vy = verts[:, k, :nv, 0], verts[:, k, :nv, 1]
            wx, wy = p[:, k, 1:2] + (cs * vx - sn * vy), p[:, k, 2:3] + (sn * vx + cs * vy)
            ex, ey = torch.roll(wx, -1, 1) - wx, torch.roll(wy, -1, 1) - wy
            L = torch.sqrt(ex * ex + ey * ey)
            e4 = lambda t: t.reshape(B, 1, 1, nv)
            qx, qy = X.unsqueeze(-1) - e4(wx), Y.unsqueeze(-1) - e4(wy)
            m = (e4(ey / L) * qx - e4(ex / L) * qy).max(-1).values
            t = ((qx * e4(ex) + qy * e4(ey)) / e4(L * L)).clamp(0.0, 1.0)
            dist = torch.sqrt((qx - t * e4(ex)) ** 2 + (qy - t * e4(ey)) ** 2).min(-1).values
            d = torch.where(m <= 0, m, dist)
        a = (cov(d) - cov(d + thick[k]) if thick[k] > 0 else cov(d)).unsqueeze(1)
        img = img * (1 - a) + a * colors[:, k].to(F64).reshape(B, C, 1, 1)
    return img.to(torch.float32)


def _rect(wd, ht):
    return [[wd / 2, ht / 2], [-wd / 2, ht / 2], [-wd / 2, -ht / 2], [wd / 2, -ht / 2]]          # bodies.py:260-262


def layout(name):
    """(B, H, W, camera, bodies, torch-route chunk): bodies = [(kind, (rot, x, y), radius or vertices, thickness)]."""
    if name == "A_4096x64x64_4bodies":
        bodies = [("rect", (0.0, 484.0, 500.0), _rect(900.0, 10.0), 0.0), ("rect", (0.2, 505.0, 478.0), _rect(30.0, 30.0), 0.0),
                  ("rect", (-0.4, 498.0, 446.0), _rect(26.0, 22.0), 3.0), ("circle", (0.0, 458.0, 472.0), 20.0, 0.0)]
        return 4096, 64, 64, (420.0, 400.0, 0.5), bodies, 1024
    # experiments/breakout/encoder.py:28-51, 148-227 (pixel units, ppm = 1)
    SW, WALL, ROOF, STOP_LINE, STOP_H, BH = 160.0, 8.0, 31.0, 189.0, 6.0, 6.0
    bodies = [("circle", (0.0, 80.0, 120.0), 1.0, 0.0), ("rect", (0.0, 72.0, 191.0), _rect(16.0, 4.0), 0.0),
              ("rect", (0.0, WALL / 2, STOP_LINE / 2), _rect(WALL, STOP_LINE), 0.0),
              ("rect", (0.0, SW - WALL / 2, (STOP_LINE + STOP_H) / 2), _rect(WALL, STOP_LINE + STOP_H), 0.0),
              ("rect", (0.0, SW / 2, ROOF / 2), _rect(SW - 2 * WALL, ROOF), 0.0),
              ("rect", (0.0, WALL / 2, STOP_LINE + STOP_H / 2), _rect(WALL, STOP_H), 0.0),
              ("rect", (0.0, SW + WALL / 2, STOP_LINE + STOP_H / 2), _rect(WALL, STOP_H), 0.0)]
    for row, n in enumerate((6, 6, 6, 5, 5, 5)):                          # 33 blocks between columns 8 and 152, rows 57 .. 93
        bw = (SW - 2 * WALL) / n
        bodies += [("rect", (0.0, WALL + (i + 0.5) * bw, 57.0 + (row + 0.5) * BH), _rect(bw, BH), 0.0) for i in range(n)]
    return 256, 210, 160, (0.0, 0.0, 1.0), bodies, 16


def make_shape(name, dev):
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.render import Camera
    B, H, W, (x0, y0, ppm), bodies, chunk = layout(name)
    nb, cap = len(bodies), 8
    rng = np.random.default_rng(5)
    kind, nverts, radius = np.zeros((B, nb), np.int32), np.zeros((B, nb), np.int32), np.zeros((B, nb))
    verts, thick = np.zeros((B, nb, cap, 2)), np.zeros((B, nb))
    pose = np.zeros((B, nb, 3))
    for k, (what, ps, shape, th) in enumerate(bodies):
        pose[:, k] = np.asarray(ps) + rng.uniform(-1, 1, (B, 3)) * np.array([0.05 if what == "rect" and ps[0] != 0.0 else 0.0, 0.45, 0.45]) / ppm
        thick[:, k] = th
        if what == "circle":
            radius[:, k] = shape
        else:
            kind[:, k], nverts[:, k] = 1, len(shape)
            verts[:, k, :len(shape)] = np.asarray(shape)
    t = lambda a, dt_: torch.tensor(a, dtype=dt_, device=dev).contiguous()
    geom = GeometryBatch(t(kind, torch.int32), t(radius, F64), t(verts, F64), t(nverts, torch.int32), None, int(nverts[0].sum()))
    cam = Camera(H, W, origin=(x0, y0), pixels_per_meter=ppm)
    X = x0 + (torch.arange(W, dtype=F64, device=dev) + 0.5) / ppm
    Y = y0 + (torch.arange(H, dtype=F64, device=dev) + 0.5) / ppm
    gen = torch.Generator(device="cpu").manual_seed(3)
    ins = dict(geom=geom, p=t(pose, F64), cam=cam, colors=t(rng.uniform(0, 1, (B, nb, 3)), torch.float32),
               background=t(rng.uniform(0, 1, 3), torch.float32), thickness=t(thick, F64), w=1.0 / ppm,
               X=X.reshape(1, W).expand(H, W), Y=Y.reshape(H, 1).expand(H, W), nvs=[int(n) for n in nverts[0]],
               thick=[float(x) for x in thick[0]], chunk=chunk,
               g=torch.randn(B, 3, H, W, generator=gen, dtype=torch.float32).to(dev))
    info = dict(B=B, H=H, W=W, C=3, nb=nb, cap=cap, torch_route_scenes_per_chunk=chunk, bytes_forward=B * 3 * H * W * 4)
    return ins, info


def window(fn, seconds=0.2):
    """Mean time of one call of `fn` over a window of at least `seconds`, by HIP events."""
    n = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= seconds * 1e3:
            return ms * 1e-3 / n
        n = max(n * 2, int(n * seconds * 1.2e3 / max(ms, 1e-3)))


def measure(name, dev):
    from lcp_physics_amd.physics.render import render
    ins, info = make_shape(name, dev)
    geom, cam, B, chunk = ins["geom"], ins["cam"], info["B"], ins["chunk"]
    kw = dict(background=ins["background"], thickness=ins["thickness"])
    out = torch.empty(B, 3, info["H"], info["W"], dtype=torch.float32, device=dev)
    leaves = [t.clone().requires_grad_(True) for t in (ins["p"], geom.radius, geom.verts_local, ins["colors"])]
    from lcp_physics_amd.physics.contacts import GeometryBatch
    lgeom = GeometryBatch(geom.kind, leaves[1], leaves[2], geom.nverts, None, geom.scene_verts_max)

    def t_part(p, radius, verts, colors, s):
        return torch_render(ins["nvs"], ins["thick"], radius[s], verts[s], p[s], colors[s], ins["background"], ins["X"], ins["Y"], ins["w"])

    def k_fwd():
        with torch.no_grad():
            return render(geom, ins["p"], cam, ins["colors"], out=out, **kw)

    def t_fwd():
        with torch.no_grad():
            for lo in range(0, B, chunk):
                out[lo:lo + chunk] = t_part(ins["p"], geom.radius, geom.verts_local, ins["colors"], slice(lo, lo + chunk))
        return out

    def both(route):
        for x in leaves:
            x.grad = None
        if route == "kernel":
            render(lgeom, leaves[0], cam, leaves[3], **kw).backward(ins["g"])
        else:
            for lo in range(0, B, chunk):
                s = slice(lo, lo + chunk)
                t_part(leaves[0], leaves[1], leaves[2], leaves[3], s).backward(ins["g"][s])

    # the two routes compute the same thing (values and gradients) before anything is timed
    ki = k_fwd().clone()
    ti = t_fwd().clone()
    both("kernel")
    kg = [x.grad.clone() for x in leaves]
    both("torch")
    tg = [x.grad.clone() for x in leaves]
    torch.cuda.synchronize()
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1.0))
    agree = max([rel(ki, ti)] + [rel(a, b) for a, b in zip(kg, tg)])
    assert agree < 1e-5, "the routes disagree: %g" % agree
    fns = {"kernel_forward": k_fwd, "torch_forward": t_fwd, "kernel_forward_backward": lambda: both("kernel"),
           "torch_forward_backward": lambda: both("torch")}
    for fn in fns.values():                                                             # spin-up: clocks, code objects, allocator
        window(fn, 0.3)
    runs = {k: [] for k in fns}
    for _ in range(7):                                                                  # alternating
        for k, fn in fns.items():
            runs[k].append(window(fn))
    res = dict(info, routes_agree_rel=agree)
    for k, v in runs.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e6, 2)
        res[k + "_spread_us"] = [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)]
    res["forward_fraction_of_peak_bandwidth"] = round(info["bytes_forward"] / (res["kernel_forward_us"] * 1e-6) / PEAK_BYTES_PER_S, 4)
    res["kernel_over_torch_forward"] = round(res["kernel_forward_us"] / res["torch_forward_us"], 5)
    res["kernel_over_torch_forward_backward"] = round(res["kernel_forward_backward_us"] / res["torch_forward_backward_us"], 5)
    return res


def kernel_resources():
    """Registers, scratch and static LDS of the two kernels of lcp_render.hip, from the metadata of the assembly the build left."""
    if not os.path.exists(ASM):
        return None
    keys = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
    blocks = []
    for line in open(ASM):
        m = re.match(r"  (- | {2})\.(\w+):\s+(\S+)", line)                # a kernel's metadata: "  - .first_key:" then "    .key:" lines
        if not m:
            continue
        if m.group(1) == "- ":
            blocks.append({})
        if blocks:
            blocks[-1][m.group(2)] = m.group(3)
    out = {}
    for b in blocks:
        if "lcp_render" in b.get("name", ""):
            out["backward" if "backward" in b["name"] else "forward"] = {k: int(b[k]) for k in keys if k in b}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        assert torch.cuda.is_available(), "bench_render.py measures on the GPU; there is no CPU timing"
        dev = torch.device("cuda:0")
        doc = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S,
               "shapes": {n: measure(n, dev) for n in ("A_4096x64x64_4bodies", "B_256x210x160_breakout40")}}
    res = kernel_resources()
    if res is not None or "kernels" not in doc:
        doc["kernels"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
