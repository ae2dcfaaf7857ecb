"""Worlds from pixels, on the device: the reference's Breakout experiment (`experiments/breakout/encoder.py`,
`run_breakout.py:27-69`) for B frames at once.

    params = extract_params(frames)                        # [B,210,160,3] uint8 on the GPU -> paddle, blocks, ball: ONE launch
    state = to_vector(params)                              # [B, 4 + 4 max_blocks + 3] f64 (run_breakout.py:47-60)
    bw = make_world(params, ball_vel)                      # encoder.py:148-227: 7 + max_blocks bodies per scene
    state = simulate_breakout(bw, action, vx, vy, differentiable=True)       # run_breakout.py:27-44
    (state[:, :4] ** 2).mean().backward()                  # reaches vx, vy (learn_params.py)

`extract_params` is `lcp_extract_params_u8` (lcp_encoder.hip; include/lcp_hip.h has the rule): it reads channel 0 of the frames in
place, through their strides, and finds the paddle, the runs of every band of blocks and the ball.  `render` closes the loop the
other way (`to_uint8` is `FrameRecorder`'s quantisation).  The world is a `ContactWorld` built from `BodyBatch.from_raw` on device
tensors; the pinned bodies (walls, roof, stoppers, blocks) come first, so their TotalConstraints are Je = [I 0].  Not here: the
MPC controller and gym (`run_breakout.py:72-245`).  No CPU fallback.
"""
import ctypes
from dataclasses import dataclass, field

import torch

from .. import _lib
from .bodies import BodyBatch
from .contacts import CIRCLE, HULL, NV

ST_NO_BALL, ST_TRUNCATED, ST_RUN_AT_EDGE, ST_PADDLE_PROBE = 1, 2, 4, 8           # LCP_ENC_ST_* (include/lcp_hip.h)
_ST_NAMES = ((ST_TRUNCATED, "more blocks than max_blocks"), (ST_RUN_AT_EDGE, "a run of blocks reaches the last column (encoder.py:96-101 never returns)"),
             (ST_PADDLE_PROBE, "the paddle probe leaves the image (encoder.py:69 raises)"))
PLACEHOLDER = (1000.0, 60.0, 1.0, 1.0)       # run_breakout.py:56: the block outside the screen that stands for "no block"
MAX_ROWS, MAX_BLOCKS = 8, 256


@dataclass(frozen=True)
class FrameLayout:
    """Where the encoder looks (the LCP_ENC_LAYOUT_WORDS of include/lcp_hip.h) and what `make_world` builds around it; the defaults
    are the constants of encoder.py:17-60.  Keys are values of channel 0; colours are RGB in 0..255."""
    height: int = 210                        # :28
    width: int = 160                         # :29
    paddle_line: int = 189                   # :31
    paddle_h: int = 4                        # :33
    paddle_w: int = 16                       # :34
    paddle_key: int = 200                    # :35, :18
    ball_w: int = 2                          # :38
    nrows: int = 6                           # :44
    band_top: int = 57                       # :42
    band_h: int = 6                          # :41
    row_key: tuple = (200, 198, 180, 162, 72, 66)            # :44, :18-23
    erase: tuple = (189, 152, 194, 160)      # :104-105 (top, left, bottom, right), inclusive: the red stopper
    ball_key: int = 200                      # :39
    wall_w: float = 8.0                      # :46
    roof_line: float = 31.0                  # :48
    stopper_line: float = 189.0              # :49
    stopper_w: float = 8.0                   # :50
    stopper_h: float = 6.0                   # :51
    dt: float = 1.0                          # :56
    fric: float = 0.0                        # :57
    ball_mass: float = 1.0                   # :58
    restitution: float = 1.0                 # :59
    stopper_restitution: float = -1.0        # :60
    row_colors: tuple = ((200, 72, 72), (198, 108, 58), (180, 122, 48), (162, 162, 42), (72, 160, 72), (66, 72, 200))   # :18-23, :44
    paddle_color: tuple = (200, 72, 72)      # :35
    ball_color: tuple = (200, 72, 72)        # :39
    wall_color: tuple = (142, 142, 142)      # :47
    left_stopper_color: tuple = (66, 158, 130)               # :52
    right_stopper_color: tuple = (142, 142, 142)             # :203 (drawn in the wall's colour)

    @staticmethod
    def atari():
        return FrameLayout()

    def words(self):
        """The int32 words `lcp_extract_params_u8` takes."""
        if not 0 <= self.nrows <= MAX_ROWS or len(self.row_key) < self.nrows or len(self.erase) != 4:
            raise ValueError("a layout has 0..%d bands, a key for each, and an erase rect of four corners" % MAX_ROWS)
        keys = [int(k) for k in self.row_key[:self.nrows]] + [0] * (MAX_ROWS - self.nrows)
        return [self.paddle_line, self.paddle_h, self.paddle_w, self.paddle_key, self.ball_w, self.nrows, self.band_top, self.band_h,
                *keys, *[int(c) for c in self.erase], self.ball_key]

    def validate(self, H, W, max_blocks):
        """What the entry refuses with LCP_E_BADARG, with the reason."""
        key = lambda k: 1 <= int(k) <= 255
        w = self.words()
        if not 1 <= W <= 1024 or H < 1:
            raise ValueError("frames must be 1 .. 1024 pixels wide and at least one high (got %d x %d)" % (H, W))
        if not 1 <= int(max_blocks) <= MAX_BLOCKS:
            raise ValueError("max_blocks must lie in 1 .. %d (got %d)" % (MAX_BLOCKS, max_blocks))
        if not (key(self.paddle_key) and key(self.ball_key) and all(key(k) for k in w[8:8 + self.nrows])):
            raise ValueError("keys are bytes other than 0")
        if self.band_h < 1 or self.paddle_w < 1 or self.paddle_h < 0 or self.ball_w < 0:
            raise ValueError("band_h and paddle_w must be positive, paddle_h and ball_w not negative")
        if not (0 <= self.paddle_line < H and 0 <= self.band_top < H):
            raise ValueError("paddle_line and band_top must lie inside the image")
        if self.band_top + self.nrows * self.band_h > self.paddle_line:
            raise ValueError("the bands must end at or above paddle_line")
        if min(self.erase) < 0 or self.erase[2] < self.erase[0] or self.erase[3] < self.erase[1]:
            raise ValueError("the erase rect is (top, left, bottom, right) with top <= bottom and left <= right, none negative")


@dataclass
class BreakoutParams:
    """What the encoder read off B frames, on the device: corners are (top, left, bottom, right) int32; `*_params` the
    `get_pos_dims` form (encoder.py:140-145) in float64 - paddle (x, y, w, h), blocks (x, y, w, h) with the placeholder
    (1000, 60, 1, 1) in slots >= `nblocks`, ball (x, y, radius)."""
    paddle: torch.Tensor
    blocks: torch.Tensor
    nblocks: torch.Tensor
    ball: torch.Tensor
    status: torch.Tensor
    paddle_params: torch.Tensor
    block_params: torch.Tensor
    ball_params: torch.Tensor

    _FIELDS = (("paddle", torch.int32, (4,)), ("blocks", torch.int32, (-1, 4)), ("nblocks", torch.int32, ()), ("ball", torch.int32, (4,)),
               ("status", torch.int32, ()), ("paddle_params", torch.float64, (4,)), ("block_params", torch.float64, (-1, 4)),
               ("ball_params", torch.float64, (3,)))

    @staticmethod
    def empty(B, max_blocks, device):
        """Preallocated outputs for `extract_params(out=...)`."""
        shape = lambda s: (B,) + tuple(max_blocks if d < 0 else d for d in s)
        return BreakoutParams(*[torch.empty(shape(s), dtype=dt_, device=device) for _, dt_, s in BreakoutParams._FIELDS])

    @property
    def max_blocks(self):
        return self.blocks.shape[1]

    def raise_on_status(self):
        """RuntimeError naming the first frame the reference would not have returned from, or whose block list was cut (synchronises)."""
        st = self.status.cpu()
        bad = (st & (ST_TRUNCATED | ST_RUN_AT_EDGE | ST_PADDLE_PROBE)).nonzero()
        if bad.numel():
            k = int(bad[0])
            word = int(st[k])
            raise RuntimeError("frame %d: %s (status %d)" % (k, "; ".join(t for bit, t in _ST_NAMES if word & bit), word))


def to_uint8(image):
    """`FrameRecorder`'s quantisation of a rendered image (float in [0, 1]) to bytes: round(clamp(x, 0, 1) * 255)."""
    return torch.round(image.detach().clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def extract_params(frames, layout=None, max_blocks=32, channels_first=False, out=None, check=None):
    """encoder.py:63-133 for B frames in one launch.  `frames`: uint8 on the GPU, [B,H,W,C] (gym's) or [B,H,W], or with
    `channels_first` [B,C,H,W] (`FrameRecorder`'s); any strides - a view is read in place, only channel 0 is touched.
    `max_blocks`: the slots of the block list (1 .. 256; the true count is `nblocks`, more set ST_TRUNCATED).
    `out`: a `BreakoutParams.empty(B, max_blocks, device)` to write into; the call is then the one launch and nothing else, so it
    can be captured in a `torch.cuda.graph` (`max_blocks` is taken from it).  `check=True` reads `status` once (one host
    synchronisation) and raises on TRUNCATED, RUN_AT_EDGE or PADDLE_PROBE; False leaves it on the device (None: True unless `out`
    is given)."""
    check = out is None if check is None else bool(check)
    layout = FrameLayout.atari() if layout is None else layout
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise RuntimeError("frames must live on a GPU (got %s); the HIP path has no CPU fallback"
                           % (frames.device if isinstance(frames, torch.Tensor) else type(frames).__name__))
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
        raise RuntimeError("frames must be uint8 [B,H,W,C], [B,C,H,W] or [B,H,W] (got %s %s)" % (frames.dtype, tuple(frames.shape)))
    plane = frames if frames.dim() == 3 else (frames[:, 0] if channels_first else frames[..., 0])
    B, H, W = plane.shape
    if out is not None:
        max_blocks = out.max_blocks
    layout.validate(H, W, max_blocks)
    # a dimension of one element has no stride to speak of; the entry wants them positive
    sb, sr, sc = (max(int(s), 1) if n == 1 else int(s) for s, n in zip(plane.stride(), plane.shape))
    if min(sb, sr, sc) < 1:
        raise RuntimeError("frames must have positive strides (an expanded view has none)")
    dev = frames.device
    if out is None:
        out = BreakoutParams.empty(B, max_blocks, dev)
    else:
        for name, dt_, s in BreakoutParams._FIELDS:
            t = _lib.require_gpu_tensor(getattr(out, name), "out." + name, dt_)
            if t.shape != (B,) + tuple(max_blocks if d < 0 else d for d in s):
                raise ValueError("out.%s has shape %s for %d frames and %d block slots" % (name, tuple(t.shape), B, max_blocks))
    words = (ctypes.c_int32 * len(layout.words()))(*layout.words())
    P = _lib.ptr
    lib = _lib.load()
    with _lib.on_device(dev):
        rc = lib.lcp_extract_params_u8(B, H, W, ctypes.c_void_p(plane.data_ptr()), sb, sr, sc, ctypes.cast(words, ctypes.c_void_p),
                                       int(max_blocks), P(out.paddle), P(out.blocks), P(out.nblocks), P(out.ball), P(out.status),
                                       P(out.paddle_params), P(out.block_params), P(out.ball_params), _lib.stream_ptr(dev))
    _lib.check(rc, "lcp_extract_params_u8")
    if check:
        out.raise_on_status()
    return out


def to_vector(params):
    """run_breakout.py:47-60, batched: [B, 4 + 4 max_blocks + 3] f64 = paddle (pos, dims), blocks (pos, dims) with the placeholder
    in absent slots, ball (pos, rad)."""
    B = params.paddle_params.shape[0]
    return torch.cat([params.paddle_params, params.block_params.reshape(B, -1), params.ball_params], dim=1)


def from_vector(state, max_blocks=None):
    """run_breakout.py:63-69, batched: state [B, 4 + 4 max_blocks + 3] -> (paddle_params [B,4], block_params [B,max_blocks,4],
    ball_params [B,3]), views of `state`."""
    n = state.shape[1] - 7
    if n < 4 or n % 4 or (max_blocks is not None and n != 4 * max_blocks):
        raise ValueError("a state has 4 + 4 max_blocks + 3 columns (got %d%s)" % (state.shape[1], "" if max_blocks is None else
                                                                                  " for max_blocks = %d" % max_blocks))
    return state[:, :4], state[:, 4:4 + n].reshape(state.shape[0], n // 4, 4), state[:, 4 + n:]


@dataclass
class BreakoutWorld:
    """`world`: the `ContactWorld`; `ball`, `paddle`: body indices; `blocks`: the indices of the block slots (a `range`); `present`
    [B,max_blocks] bool: the slots that hold a block; `dims` [B,nb,2] f64: the rects' (w, h) and, for the ball, (radius, radius);
    `colors` [nb,3] float32 in [0, 1] for `render` (block slots in the colour of the first band: a slot's band varies by scene -
    `scene_colors` [B,nb,3] has every block in its band's colour)."""
    world: object
    ball: int
    paddle: int
    blocks: range
    present: torch.Tensor
    dims: torch.Tensor
    colors: torch.Tensor
    scene_colors: torch.Tensor
    layout: FrameLayout = field(default_factory=FrameLayout)


def make_world(params_or_state, ball_vel, layout=None, **world_kw):
    """encoder.py:148-227 for B scenes: walls, roof and stoppers of the layout, `max_blocks` block slots, the ball (a circle) and
    the paddle, as a `ContactWorld` with dt = 1, restitution 1 (-1 on the stoppers), friction 0, TotalConstraints on everything but
    ball and paddle, and the reference's `add_no_contact` pairs.  A slot without a block sits at the placeholder pose and collides
    with nothing.  `params_or_state`: `BreakoutParams`, or a state [B, 4 + 4 max_blocks + 3] f64 (`to_vector`; a slot that holds
    exactly the placeholder is absent).  `ball_vel`: (vx, vy) or [B,2].  Body order: left wall, right wall, roof, left stopper,
    right stopper, the blocks, ball, paddle.  `world_kw` goes to `ContactWorld` (maxc, check, ...).  Device work only, except for what
    `ContactWorld` itself checks on the host (`check=False` turns that off)."""
    layout = FrameLayout.atari() if layout is None else layout
    f64 = torch.float64
    if isinstance(params_or_state, BreakoutParams):
        pp, bp, lp = params_or_state.paddle_params, params_or_state.block_params, params_or_state.ball_params
        mb = bp.shape[1]
        present = torch.arange(mb, device=bp.device).unsqueeze(0) < params_or_state.nblocks.unsqueeze(1)
    else:
        state = _lib.require_gpu_tensor(params_or_state.detach(), "state", f64)
        pp, bp, lp = from_vector(state)
        mb = bp.shape[1]
        present = ~(bp == bp.new_tensor(PLACEHOLDER)).all(dim=2)
    dev = pp.device
    if not pp.is_cuda:
        raise RuntimeError("the parameters must live on a GPU (got %s); the HIP path has no CPU fallback" % dev)
    B = pp.shape[0]
    nfix = 5 + mb
    nb = nfix + 2
    ball, paddle = nfix, nfix + 1
    L = layout
    Wd, ww, sl, sw, sh = float(L.width), L.wall_w, L.stopper_line, L.stopper_w, L.stopper_h
    # (x, y, w, h) of the five fixed rects, encoder.py:171-205
    fixed = torch.tensor([[ww / 2, sl / 2, ww, sl], [Wd - ww / 2, (sl + sh) / 2, ww, sl + sh], [Wd / 2, L.roof_line / 2, Wd - 2 * ww, L.roof_line],
                          [sw / 2, sl + sh / 2, sw, sh], [Wd + sw / 2, sl + sh / 2, sw, sh]], dtype=f64, device=dev)
    rects = torch.cat([fixed.unsqueeze(0).expand(B, 5, 4), bp, bp.new_zeros(B, 1, 4), pp.unsqueeze(1)], dim=1)       # [B,nb,4]; the ball's row unused
    half = rects[:, :, 2:] / 2
    corner = torch.tensor([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0]], dtype=f64, device=dev)               # bodies.py:260-262
    verts = torch.zeros(B, nb, NV, 2, dtype=f64, device=dev)
    verts[:, :, :4] = half.unsqueeze(2) * corner
    verts[:, ball] = 0.0
    kind = torch.full((B, nb), HULL, dtype=torch.int32, device=dev)
    kind[:, ball] = CIRCLE
    nverts = torch.full((B, nb), 4, dtype=torch.int32, device=dev)
    nverts[:, ball] = 0
    radius = torch.zeros(B, nb, dtype=f64, device=dev)
    radius[:, ball] = lp[:, 2]
    ref = torch.zeros(B, nb, 3, dtype=f64, device=dev)
    ref[:, :, 1:] = rects[:, :, :2]
    ref[:, ball, 1:] = lp[:, :2]
    v0 = torch.zeros(B, nb, 3, dtype=torch.float32, device=dev)
    v0[:, ball, 1:] = torch.as_tensor(ball_vel, dtype=torch.float32, device=dev).expand(B, 2)
    mass = torch.ones(B, nb, dtype=f64, device=dev)
    mass[:, ball] = L.ball_mass
    rest = torch.full((B, nb), L.restitution, dtype=torch.float32, device=dev)
    rest[:, 3:5] = L.stopper_restitution
    fric = torch.full((B, nb), L.fric, dtype=torch.float32, device=dev)
    raw = {"kind": kind, "radius": radius, "verts_raw": verts, "nverts": nverts, "mass": mass, "ref": ref, "v0": v0, "rest": rest, "fric": fric}
    bodies = BodyBatch.from_raw(raw, g=None, check=False, scene_verts_max=4 * (nb - 1))
    # add_no_contact, encoder.py:175-225 (symmetric, bodies.py:104-106)
    LW, RW, ROOF, LS, RS = range(5)
    nc = torch.zeros(nb, nb, dtype=torch.bool, device=dev)
    pairs = [(LW, paddle), (paddle, RW), (ROOF, paddle), (ROOF, LW), (ROOF, RW), (LS, LW), (LS, ball), (RS, RW), (RS, ball)]
    for i, j in pairs:
        nc[i, j] = nc[j, i] = True
    nc[5:nfix, LW] = nc[LW, 5:nfix] = True
    nc[5:nfix, RW] = nc[RW, 5:nfix] = True
    nc[5:nfix, 5:nfix] = True
    absent = torch.zeros(B, nb, dtype=torch.bool, device=dev)
    absent[:, 5:nfix] = ~present
    nc = nc.unsqueeze(0) | absent.unsqueeze(1) | absent.unsqueeze(2)
    nc = nc & ~torch.eye(nb, dtype=torch.bool, device=dev)
    bodies.geom.no_contact = nc.to(torch.uint8).contiguous()
    # TotalConstraint (constraints.py:176-192: J = I) on the leading 5 + max_blocks bodies
    e = 3 * nfix
    Je = torch.zeros(B, e, 3 * nb, dtype=torch.float32, device=dev)
    Je[:, :, :e] = torch.eye(e, dtype=torch.float32, device=dev)
    world_kw.setdefault("dt", L.dt)
    world = bodies.world(Je=Je, **world_kw)
    dims = rects[:, :, 2:].clone()
    dims[:, ball] = lp[:, 2:3]
    # colours: a block's band from its top line, encoder.py:214
    c255 = lambda c: torch.tensor(c, dtype=torch.float32, device=dev) / 255.0
    rows = c255(L.row_colors[:max(L.nrows, 1)])
    level = ((bp[:, :, 1] - bp[:, :, 3] / 2 - L.band_top) / L.band_h).floor().long().clamp(0, rows.shape[0] - 1)
    scene_colors = torch.cat([torch.stack([c255(L.wall_color), c255(L.wall_color), c255(L.wall_color), c255(L.left_stopper_color),
                                           c255(L.right_stopper_color)]).unsqueeze(0).expand(B, 5, 3), rows[level],
                              c255(L.ball_color).expand(B, 1, 3), c255(L.paddle_color).expand(B, 1, 3)], dim=1).contiguous()
    colors = scene_colors[0].clone()
    colors[5:nfix] = rows[0]
    return BreakoutWorld(world, ball, paddle, range(5, nfix), present, dims, colors, scene_colors, L)


def step_breakout(bw, action, paddle_vel_x, paddle_vel_y, differentiable=False):
    """encoder.py:299-307: the velocities detached and copied, the paddle's two translation components set to
    `paddle_vel * action` (`action` [B] or a number; the speeds numbers or tensors, which the gradient reaches), one
    `step(fixed_dt=True)`."""
    w = bw.world
    dev = w.p.device
    v = w.v.detach().clone()
    act = torch.as_tensor(action, dtype=torch.float32, device=dev).expand(w.B)
    as_t = lambda s: s.to(device=dev, dtype=torch.float32) if isinstance(s, torch.Tensor) else torch.tensor(float(s), dtype=torch.float32, device=dev)
    k = bw.paddle
    row = torch.stack([v[:, k, 0], (as_t(paddle_vel_x) * act).expand(w.B), (as_t(paddle_vel_y) * act).expand(w.B)], dim=1)      # [B,3]
    w.v = torch.cat([v[:, :k], row.unsqueeze(1), v[:, k + 1:]], dim=1)
    return w.step(fixed_dt=True, differentiable=differentiable)


def breakout_state(bw):
    """The state vector of the world's current pose (run_breakout.py:30-34): paddle (pos, dims), blocks, ball (pos, rad)."""
    p = bw.world.p
    B = p.shape[0]
    dims = bw.dims.to(p.dtype)
    body = lambda i: torch.cat([p[:, i, 1:], dims[:, i]], dim=1)
    blocks = torch.cat([p[:, bw.blocks.start:bw.blocks.stop, 1:], dims[:, bw.blocks.start:bw.blocks.stop]], dim=2).reshape(B, -1)
    return torch.cat([body(bw.paddle), blocks, p[:, bw.ball, 1:], dims[:, bw.ball, :1]], dim=1)


def simulate_breakout(bw, action, paddle_vel_x, paddle_vel_y, differentiable=False):
    """run_breakout.py:27-44: `step_breakout`, the new state [B, 4 + 4 max_blocks + 3], and the rotation of ball, paddle and blocks
    put back to 0 by assigning the pose (contacts are not detected again, as in the reference)."""
    step_breakout(bw, action, paddle_vel_x, paddle_vel_y, differentiable=differentiable)
    state = breakout_state(bw)
    w = bw.world
    keep = torch.ones(w.nb, 3, dtype=w.p.dtype, device=w.p.device)
    keep[bw.blocks.start:, 0] = 0.0                                    # blocks, ball, paddle: the trailing bodies
    if differentiable:
        w.p = w.p * keep
    else:
        w.p.mul_(keep)
    return state
