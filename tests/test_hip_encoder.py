"""GPU: the breakout encoder on the device (lcp_encoder.hip: `lcp_extract_params_u8`, through
`lcp_physics_amd.physics.breakout.extract_params`) against the unmodified reference's answers (tests/golden/breakout.npz) and its
numpy restatement (tests/encoder_host.py, which tests/test_encoder_fixture.py holds to the reference).  Everything is compared
exactly: the corners are integers, the `*_params` halves of integers."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from tests import encoder_host as EH

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "breakout.npz")
FIELDS = ("paddle", "blocks", "nblocks", "ball", "status", "paddle_params", "block_params", "ball_params")


def _layout(L, H, W):
    from lcp_physics_amd.physics.breakout import FrameLayout
    return dataclasses.replace(FrameLayout.atari(), height=H, width=W, **L)


def _host(p):
    return {n: getattr(p, n).cpu().numpy() for n in FIELDS}


def _assert_same(got, want, what):
    for n in FIELDS:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n, got[n].dtype, got[n].shape)
        bad = np.argwhere(got[n] != want[n])
        assert bad.size == 0, (what, n, "first difference at", bad[0].tolist(), got[n][tuple(bad[0])], want[n][tuple(bad[0])])


@functools.lru_cache(None)
def _random64():
    """64 seeded random frames (block counts from a handful to dozens side by side) and the restatement's answers, shared."""
    rng = np.random.default_rng(64)
    keys = np.stack([EH.random_frame(rng) for _ in range(64)])
    want = EH.extract_host_batch(keys, max_blocks=40)
    assert int(want["nblocks"].min()) <= 8 and int(want["nblocks"].max()) >= 30 and (want["status"] & EH.ST_NO_BALL).any()
    return keys, want


def test_the_committed_frames_give_the_reference_s_answers():
    from lcp_physics_amd.physics.breakout import extract_params
    g = np.load(GOLDEN)
    keys = g["a_key"]
    nmax = g["a_block_params"].shape[1]
    rng = np.random.default_rng(0)
    p = extract_params(torch.from_numpy(EH.to_frame(keys, 3, rng)).to(DEV), max_blocks=nmax)
    got = _host(p)
    assert np.array_equal(got["nblocks"], g["a_nblocks"])
    assert np.array_equal(got["paddle_params"], g["a_paddle_params"]) and np.array_equal(got["block_params"], g["a_block_params"])
    assert np.array_equal(got["ball_params"], g["a_ball_params"])
    _assert_same(got, EH.extract_host_batch(keys, max_blocks=nmax), "fixture")          # the integers: the restatement's


def test_64_random_frames_in_one_launch_match_the_restatement_in_every_layout_of_the_frame():
    """gym's [B,H,W,3], RGBA [B,H,W,4], FrameRecorder's [B,3,H,W] and a bare plane: the same answers, other channels random."""
    from lcp_physics_amd.physics.breakout import extract_params
    keys, want = _random64()
    rng = np.random.default_rng(1)
    for C, cf in ((3, False), (4, False), (3, True), (1, False)):
        frames = torch.from_numpy(EH.to_frame(keys, C, rng, channels_first=cf)).to(DEV)
        _assert_same(_host(extract_params(frames, max_blocks=40, channels_first=cf, check=False)), want, (C, cf))
    plane = torch.from_numpy(keys).to(DEV)
    _assert_same(_host(extract_params(plane, max_blocks=40, check=False)), want, "plane")
    # any positive strides: a column stride of 7 bytes (gathered, not read by lines) and a view with padded rows
    wide = torch.from_numpy(EH.to_frame(keys[:8], 7, rng)).to(DEV)
    _assert_same(_host(extract_params(wide, max_blocks=40, check=False)), {n: v[:8] for n, v in want.items()}, "stride 7")
    padded = torch.zeros(8, 210, 171, 3, dtype=torch.uint8, device=DEV)
    padded[:, :, 5:165] = torch.from_numpy(EH.to_frame(keys[:8], 3, rng)).to(DEV)
    _assert_same(_host(extract_params(padded[:, :, 5:165], max_blocks=40, check=False)), {n: v[:8] for n, v in want.items()}, "padded rows")


@pytest.mark.parametrize("W", [40, 64, 65, 160, 200])
def test_small_layouts_at_widths_around_the_64_column_pass(W):
    """Below one pass of 64 columns, exactly one, one over, 2.5 passes, 3.1 passes; with C = 3 rows of 3 W bytes start at every
    alignment (W = 65: 195 bytes per row), with C = 1 rows of W bytes."""
    from lcp_physics_amd.physics.breakout import extract_params
    H = 50
    L = EH.scaled_layout(H, W)
    rng = np.random.default_rng(W)
    keys = np.stack([EH.random_frame(rng, L, H, W) for _ in range(12)])
    keys[3, L["band_top"] + L["band_h"], W - 3:] = L["row_key"][1]                      # a run that reaches the last column
    want = EH.extract_host_batch(keys, L, max_blocks=24)
    assert want["status"][3] & EH.ST_RUN_AT_EDGE and int(want["nblocks"].max()) > 4
    for C in (3, 1, 4):
        frames = torch.from_numpy(EH.to_frame(keys, C, rng)).to(DEV)
        _assert_same(_host(extract_params(frames, _layout(L, H, W), max_blocks=24, check=False)), want, (W, C))
    # an odd byte offset of the whole batch: no row starts on a 16-byte line
    flat = torch.zeros(keys.size * 3 + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = torch.from_numpy(EH.to_frame(keys, 3, rng)).to(DEV).reshape(-1)
    _assert_same(_host(extract_params(flat[1:].view(12, H, W, 3), _layout(L, H, W), max_blocks=24, check=False)), want, (W, "offset 1"))


def test_a_short_block_list_is_cut_and_nothing_else():
    from lcp_physics_amd.physics.breakout import extract_params
    keys, want = _random64()
    frames = torch.from_numpy(EH.to_frame(keys, 3, np.random.default_rng(2))).to(DEV)
    got = _host(extract_params(frames, max_blocks=6, check=False))
    cut = want["nblocks"] > 6
    assert cut.any() and (~cut).any()
    assert np.array_equal(got["nblocks"], want["nblocks"])                              # the true count
    assert np.array_equal(got["status"] & EH.ST_TRUNCATED != 0, cut)
    assert np.array_equal(got["status"] & ~EH.ST_TRUNCATED, want["status"])
    assert np.array_equal(got["blocks"], want["blocks"][:, :6]) and np.array_equal(got["block_params"], want["block_params"][:, :6])
    assert np.array_equal(got["ball"], want["ball"]) and np.array_equal(got["ball_params"], want["ball_params"])
    assert np.array_equal(got["paddle"], want["paddle"])
    with pytest.raises(RuntimeError, match="max_blocks"):
        extract_params(frames, max_blocks=6, check=True)


def test_frames_the_reference_does_not_return_from_come_back_flagged():
    from lcp_physics_amd.physics.breakout import extract_params
    rng = np.random.default_rng(3)
    L = EH.ATARI
    keys = np.stack([EH.synth(rng, p_missing=0.5) for _ in range(3)])
    keys[1, L["band_top"] + 2 * L["band_h"], 150:] = L["row_key"][2]                    # a run to the last column
    keys[2, L["paddle_line"]] = 0
    keys[2, L["paddle_line"], 158:] = 255                                               # the maximum two columns from the edge
    want = EH.extract_host_batch(keys, max_blocks=40)
    assert want["status"].tolist() == [0, EH.ST_RUN_AT_EDGE, EH.ST_PADDLE_PROBE]
    frames = torch.from_numpy(EH.to_frame(keys, 3, rng)).to(DEV)
    _assert_same(_host(extract_params(frames, max_blocks=40, check=False)), want, "flagged")
    with pytest.raises(RuntimeError, match="frame 1"):
        extract_params(frames, max_blocks=40)


def test_graph_capture_replays_the_same_bits():
    from lcp_physics_amd.physics.breakout import BreakoutParams, extract_params
    keys, want = _random64()
    rng = np.random.default_rng(4)
    frames = torch.from_numpy(EH.to_frame(keys, 3, rng)).to(DEV)
    out = BreakoutParams.empty(64, 40, DEV)
    extract_params(frames, out=out)                                                     # (warm-up: the library is loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        extract_params(frames, out=out)
    for n in FIELDS:
        getattr(out, n).fill_(-5)
    graph.replay()
    torch.cuda.synchronize()
    _assert_same(_host(out), want, "replay")
    frames.copy_(torch.from_numpy(EH.to_frame(keys[::-1].copy(), 3, rng)).to(DEV))      # new pixels, the same launch
    graph.replay()
    torch.cuda.synchronize()
    _assert_same(_host(out), {n: v[::-1] for n, v in want.items()}, "replay on new frames")


def test_round_trip_with_render():
    """The encoder's answer drawn by `render` (integer-cornered rects at one pixel per unit, a ball_w x 4 rect as ball; crisp: see
    tests/test_encoder_fixture.py), quantised by `to_uint8` and extracted again: paddle, blocks and ball come back exactly."""
    from lcp_physics_amd.physics.breakout import extract_params, to_uint8
    from lcp_physics_amd.physics.contacts import GeometryBatch
    from lcp_physics_amd.physics.render import Camera, render
    rng = np.random.default_rng(5)
    keys = np.stack([EH.synth(rng, p_missing=pm) for pm in (0.5, 0.3, 0.7)])
    outs = [EH.extract_host(k) for k in keys]
    nslots = max(o["nblocks"] for o in outs) + 1
    want = EH.extract_host_batch(keys, max_blocks=nslots)
    c = EH.render_case(outs, EH.ATARI, EH.ATARI_H, EH.ATARI_W, nslots)
    t = lambda k: c[k].to(DEV).contiguous()
    geom = GeometryBatch(t("kind"), t("radius"), t("verts_local"), t("nverts"), None, None)
    image = render(geom, t("p"), Camera(EH.ATARI_H, EH.ATARI_W), t("colors"))
    back = _host(extract_params(to_uint8(image), max_blocks=nslots, channels_first=True))
    for n in ("paddle", "blocks", "nblocks", "ball", "status"):
        assert np.array_equal(back[n], want[n]), n
    assert int(want["nblocks"].min()) > 0
