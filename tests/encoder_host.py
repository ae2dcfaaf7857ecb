"""The breakout encoder of lcp_encoder.hip (include/lcp_hip.h, "the breakout encoder") restated in numpy on the CPU, and the
synthesiser of the frames it is tested on: the yardstick of tests/test_hip_encoder.py, shared with
tools/gen_breakout_golden.py.  Not a test.

    out = extract_host(key, layout)            # key [H,W] uint8: channel 0 of a frame
    out["paddle"], out["blocks"] [n,4], out["nblocks"], out["ball"], out["status"], out["*_params"]

The reference (experiments/breakout/encoder.py:63-133) paints what it has found black and searches again; the restatement keeps a
boolean `removed` image instead, which is the form the kernel uses.  tests/test_encoder_fixture.py holds it to the unmodified
reference, on the committed frames and live."""
import numpy as np

ST_NO_BALL, ST_TRUNCATED, ST_RUN_AT_EDGE, ST_PADDLE_PROBE = 1, 2, 4, 8
PLACEHOLDER = (1000.0, 60.0, 1.0, 1.0)                       # run_breakout.py:56

# encoder.py:28-52 (keys: channel 0 of the ATARI_* colours, :18-26)
ATARI = dict(paddle_line=189, paddle_h=4, paddle_w=16, paddle_key=200, ball_w=2, nrows=6, band_top=57, band_h=6,
             row_key=(200, 198, 180, 162, 72, 66), erase=(189, 152, 194, 160), ball_key=200)
ATARI_H, ATARI_W = 210, 160


def layout_words(L):
    """The LCP_ENC_LAYOUT_WORDS int32 words of include/lcp_hip.h."""
    keys = list(L["row_key"]) + [0] * (8 - len(L["row_key"]))
    return [L["paddle_line"], L["paddle_h"], L["paddle_w"], L["paddle_key"], L["ball_w"], L["nrows"], L["band_top"], L["band_h"],
            *keys, *L["erase"], L["ball_key"]]


def pos_dims(c):
    """get_pos_dims (encoder.py:140-145) of corners (top, left, bottom, right): (x, y, w, h)."""
    top, left, bottom, right = (float(v) for v in c)
    return ((right + left) / 2.0, (bottom + top) / 2.0, right - left, bottom - top)


def extract_host(key, L=ATARI, max_blocks=None):
    """`blocks` is the whole list; with `max_blocks` it is cut / padded to that many slots as the kernel stores it."""
    k = np.asarray(key)
    assert k.ndim == 2 and k.dtype == np.uint8
    H, W = k.shape
    removed = np.zeros((H, W), dtype=bool)
    status = 0
    # paddle, encoder.py:67-82
    pl = L["paddle_line"]
    row = k[pl]
    px = int(np.argmax(row))
    probe = px + L["ball_w"] + 1
    if probe >= W:
        status |= ST_PADDLE_PROBE                            # (:69 raises IndexError)
    elif row[probe] != L["paddle_key"]:
        px = int(np.argmax(row[probe:])) + probe             # :71
    other = np.flatnonzero(row[px:] != L["paddle_key"])
    r = int(other[0]) + px if other.size else px             # :75 (np.argmin of all-True is 0)
    r = r if r != px else W                                  # :77
    r = min(r, px + L["paddle_w"])                           # :78
    paddle = (pl, px, pl + L["paddle_h"], r)
    removed[pl:pl + L["paddle_h"] + 1, px:r + 1] = True      # :89, :137 (inclusive corners)
    # blocks, encoder.py:91-101
    blocks = []
    for i in range(L["nrows"]):
        top = L["band_top"] + i * L["band_h"]
        eq = (k[top] == L["row_key"][i]).astype(np.int8)
        d = np.diff(np.concatenate([[0], eq, [0]]))
        for left, right in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
            if left == 0:                                    # `while left > 0`
                break
            if right == W:                                   # np.argmin gives 0: a rect of no width, found again for ever
                status |= ST_RUN_AT_EDGE
                break
            blocks.append((top, int(left), top + L["band_h"], int(right)))
            removed[top:top + L["band_h"], left:right] = True            # :100 (pos[1] - [1, 1], inclusive)
    # the red stopper, encoder.py:104-105
    e = L["erase"]
    removed[e[0]:e[2] + 1, e[1]:e[3] + 1] = True
    # ball, encoder.py:107-121
    hit = (k == L["ball_key"]) & ~removed
    idx = np.flatnonzero(hit)
    if idx.size:
        i, j = divmod(int(idx[0]), W)
        stop = np.flatnonzero(~hit[i, j:])
        right = j + int(stop[0]) if stop.size else j
        stop = np.flatnonzero(~hit[i:, j])
        bottom = i + int(stop[0]) if stop.size else i
        ball = (i, j, bottom, right)
        x, y, w, h = pos_dims(ball)
        ball_params = (x, y, min(min(w, h) / 2.0, 1.0))      # :125
    else:
        status |= ST_NO_BALL
        ball = (0, 0, 0, 0)
        ball_params = (W / 2.0, H * 100.0, 1.0)              # :129
    n = len(blocks)
    stored = blocks
    if max_blocks is not None:
        if n > max_blocks:
            status |= ST_TRUNCATED
        stored = blocks[:max_blocks] + [(0, 0, 0, 0)] * max(0, max_blocks - n)
    bp = [pos_dims(c) for c in blocks]
    if max_blocks is not None:
        bp = bp[:max_blocks] + [PLACEHOLDER] * max(0, max_blocks - n)
    return dict(paddle=np.array(paddle, dtype=np.int32), blocks=np.array(stored, dtype=np.int32).reshape(-1, 4),
                nblocks=n, ball=np.array(ball, dtype=np.int32), status=status,
                paddle_params=np.array(pos_dims(paddle)), block_params=np.array(bp, dtype=np.float64).reshape(-1, 4),
                ball_params=np.array(ball_params), removed=removed)


def extract_host_batch(keys, L=ATARI, max_blocks=8):
    """The kernel's outputs for keys [B,H,W]: a dict of stacked arrays."""
    outs = [extract_host(k, L, max_blocks) for k in keys]
    return dict(paddle=np.stack([o["paddle"] for o in outs]), blocks=np.stack([o["blocks"] for o in outs]),
                nblocks=np.array([o["nblocks"] for o in outs], dtype=np.int32), ball=np.stack([o["ball"] for o in outs]),
                status=np.array([o["status"] for o in outs], dtype=np.int32),
                paddle_params=np.stack([o["paddle_params"] for o in outs]), block_params=np.stack([o["block_params"] for o in outs]),
                ball_params=np.stack([o["ball_params"] for o in outs]))


# ------------------------------------------------------------------------------------------------ frames

def scaled_layout(H, W):
    """A small layout in the proportions of the Atari one for an H x W image (H >= 40, W >= 40)."""
    band_h = max(2, H // 35)
    band_top = H // 4
    nrows = 4
    paddle_line = H - max(6, H // 10)
    ww = max(2, W // 20)
    return dict(paddle_line=paddle_line, paddle_h=2, paddle_w=max(4, W // 10), paddle_key=200, ball_w=2, nrows=nrows,
                band_top=band_top, band_h=band_h, row_key=(200, 198, 180, 162), erase=(paddle_line, W - ww, paddle_line + 3, W),
                ball_key=200)


def synth(rng, L=ATARI, H=ATARI_H, W=ATARI_W, p_missing=0.3, ball="free", paddle_x=None, strays=0, run_at_zero=None,
          stray_top=None, long_paddle=False, keep=None):
    """The key plane [H,W] uint8 of a Breakout-like frame of layout `L`: grey walls and roof (142), the stoppers (66 left, 200
    right, under the erase rect), bricks of a twentieth of the width with probability `p_missing` of a gap, a paddle, a ball.
      ball: "free" (anywhere below the bands, off the paddle's rows), "none", "paddle_row" (in the paddle's row, left of the paddle),
            "gap_top" (in a gap of band 0, across its top line), "under_paddle" (right of the paddle, overlapping its removed rect),
            or (i, j) its top-left corner
      strays: isolated ball_key pixels below the ball;  stray_top: a band whose top line gets a one-pixel run in a gap
      run_at_zero: a band that gets a brick flush with column 0;  long_paddle: a paddle_key run longer than paddle_w
      keep: only the first `keep` bricks that survive are drawn (a frame of few blocks)"""
    k = np.zeros((H, W), dtype=np.uint8)
    ww = max(2, W // 20)                                     # wall and brick width
    pl, ph, pw = L["paddle_line"], L["paddle_h"], L["paddle_w"]
    roof0, roof1 = max(1, L["band_top"] // 3), max(2, L["band_top"] // 2)
    k[roof0:pl + ph + 2, :ww] = 142
    k[roof0:pl + ph + 2, W - ww:] = 142
    k[roof0:roof1, :] = 142
    k[2:roof0 - 1, W // 5:W // 5 + 3] = 142                  # a score digit
    k[pl:pl + ph + 2, :ww] = 66
    e = L["erase"]
    k[e[0]:e[2] + 1, e[1]:min(e[3] + 1, W)] = 200            # the red stopper
    nbrick = (W - 2 * ww) // ww
    drawn = 0
    gaps = {}
    for i in range(L["nrows"]):
        top = L["band_top"] + i * L["band_h"]
        present = rng.random(nbrick) >= p_missing
        present[rng.integers(nbrick)] = False                # at least one gap per band
        for c in range(nbrick):
            if present[c] and (keep is None or drawn < keep):
                k[top:top + L["band_h"], ww + c * ww:ww + (c + 1) * ww] = L["row_key"][i]
                drawn += 1
            else:
                present[c] = False
        gaps[i] = [c for c in range(nbrick) if not present[c] and (c == 0 or not present[c - 1]) and (c == nbrick - 1 or not present[c + 1])]
        if not gaps[i]:
            gaps[i] = [c for c in range(nbrick) if not present[c]]
    if run_at_zero is not None:
        top = L["band_top"] + run_at_zero * L["band_h"]
        k[top:top + L["band_h"], :ww] = L["row_key"][run_at_zero]
    if stray_top is not None:
        top = L["band_top"] + stray_top * L["band_h"]
        c = gaps[stray_top][0]
        k[top, ww + c * ww + ww // 2] = L["row_key"][stray_top]
    run = pw + 3 if long_paddle else pw
    if paddle_x is None:
        paddle_x = int(rng.integers(ww + 6, W - ww - run - 4))
    k[pl:pl + ph, paddle_x:paddle_x + run] = L["paddle_key"]
    bh, bw = 4, L["ball_w"]
    lo = L["band_top"] + L["nrows"] * L["band_h"] + 2
    if ball == "free":
        ball = (int(rng.integers(lo, pl - bh - 1)), int(rng.integers(ww, W - ww - bw)))
    elif ball == "paddle_row":
        ball = (pl - 1, int(rng.integers(ww, paddle_x - bw - 2)))
    elif ball == "gap_top":
        c = gaps[0][0]
        ball = (L["band_top"] - 2, ww + c * ww + 1)
    elif ball == "under_paddle":
        ball = (pl - 3, paddle_x + run)
    if ball != "none":
        k[ball[0]:ball[0] + bh, ball[1]:ball[1] + bw] = L["ball_key"]
        for _ in range(strays):
            k[int(rng.integers(min(ball[0] + bh + 1, pl - 2), pl - 1)), int(rng.integers(ww, W - ww))] = L["ball_key"]
    return k


def random_frame(rng, L=ATARI, H=ATARI_H, W=ATARI_W):
    """A frame with every feature of `synth` drawn at random (block counts from a handful to several dozen)."""
    kinds = ["free"] * 5 + ["none", "paddle_row", "gap_top", "under_paddle"]
    nrows = L["nrows"]
    return synth(rng, L, H, W, p_missing=float(rng.choice([0.05, 0.3, 0.5, 0.7])), ball=kinds[int(rng.integers(len(kinds)))],
                 strays=int(rng.integers(0, 3)), run_at_zero=int(rng.integers(nrows)) if rng.random() < 0.2 else None,
                 stray_top=int(rng.integers(nrows)) if rng.random() < 0.3 else None, long_paddle=bool(rng.random() < 0.2),
                 keep=int(rng.integers(1, 9)) if rng.random() < 0.25 else None)


def to_frame(key, C, rng, channels_first=False):
    """A C-channel frame whose channel 0 is `key` [..,H,W]; the other channels hold random bytes, which nobody may read."""
    key = np.asarray(key)
    f = rng.integers(0, 256, size=key.shape + (C,), dtype=np.uint8)
    f[..., 0] = key
    return np.ascontiguousarray(np.moveaxis(f, -1, -3)) if channels_first else f


def load_reference_experiment():
    """The reference's `encoder` and `run_breakout` modules (experiments/breakout), unmodified: `run_breakout.py` imports `gym`
    and `mpc.mpc` at module level and uses neither in `simulate_breakout` / `to_vector` / `from_vector`, so empty stand-in modules
    carrying the three imported names are placed in `sys.modules`.  Needs the reference tree (oracle/ref_shim.py)."""
    import os
    import sys
    import types
    from oracle import ref_shim
    ref_shim.load_reference()
    for name, attrs in (("gym", ()), ("mpc", ()), ("mpc.mpc", ("GradMethods", "QuadCost", "MPC"))):
        if name not in sys.modules:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[name] = m
    d = os.path.join(ref_shim.REFERENCE_ROOT, "experiments", "breakout")
    if d not in sys.path:
        sys.path.insert(0, d)
    import encoder
    import run_breakout
    return encoder, run_breakout


def render_case(outs, L, H, W, nslots):
    """What the encoder read off B frames (`outs`: a list of `extract_host` results, at most `nslots` blocks each) as a scene for
    the drawing (the dict of tests/render_host.py: CPU tensors): per scene a grey wall, `nslots` block rects (absent slots at the
    placeholder pose, outside the image), the paddle and a ball_w x (bottom - top) rect as ball - axis-aligned, integer corners,
    one pixel per unit, the ramp one pixel wide: every edge falls between two pixel centres, so coverage is exactly 0 or 1."""
    import torch
    B, nb = len(outs), nslots + 3
    kind = torch.ones(B, nb, dtype=torch.int32)
    nverts = torch.full((B, nb), 4, dtype=torch.int32)
    verts = torch.zeros(B, nb, 8, 2, dtype=torch.float64)
    p = torch.zeros(B, nb, 3, dtype=torch.float64)
    colors = torch.zeros(B, nb, 3, dtype=torch.float32)
    corner = torch.tensor([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]], dtype=torch.float64)      # bodies.py:260-262
    for b, o in enumerate(outs):
        ww = max(2, W // 20)
        rects = [((ww / 2.0, H / 2.0, float(ww), float(H - 10)), (142, 142, 142))]
        for s in range(nslots):
            if s < o["nblocks"]:
                x, y, w, h = o["block_params"][s]
                band = int((y - h / 2 - L["band_top"]) // L["band_h"])
                rects.append(((x, y, w, h), (L["row_key"][band], 90, 60)))
            else:
                rects.append((PLACEHOLDER, (L["row_key"][0], 90, 60)))
        rects.append((tuple(o["paddle_params"]), (L["paddle_key"], 72, 72)))
        rects.append((pos_dims(o["ball"]), (L["ball_key"], 72, 72)))
        for k, ((x, y, w, h), col) in enumerate(rects):
            p[b, k, 1], p[b, k, 2] = x, y
            verts[b, k, :4] = corner * torch.tensor([w / 2.0, h / 2.0], dtype=torch.float64)
            colors[b, k] = torch.tensor(col, dtype=torch.float32) / 255.0
    return dict(kind=kind, radius=torch.zeros(B, nb, dtype=torch.float64), verts_local=verts, nverts=nverts, p=p, colors=colors,
                background=torch.zeros(3, dtype=torch.float32), thickness=torch.zeros(B, nb, dtype=torch.float64), H=H, W=W, x0=0.0, y0=0.0,
                ppm=1.0, w=1.0, per_scene_colors=True)
