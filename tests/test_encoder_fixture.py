"""CPU: the numpy restatement of the breakout encoder (tests/encoder_host.py) against the unmodified reference - on the committed
frames of tests/golden/breakout.npz (tools/gen_breakout_golden.py) and, where the reference tree exists, live on 200 seeded random
frames -, the layout's validation and the refusal of host tensors."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_shim
from tests import encoder_host as EH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "breakout.npz")


def test_the_restatement_reproduces_the_reference_on_the_committed_frames():
    g = np.load(GOLDEN)
    keys = g["a_key"]
    assert keys.shape == (48, EH.ATARI_H, EH.ATARI_W) and keys.dtype == np.uint8
    nmax = g["a_block_params"].shape[1]
    for k in range(len(keys)):
        host = EH.extract_host(keys[k], max_blocks=nmax)
        assert host["nblocks"] == int(g["a_nblocks"][k]), k
        assert np.array_equal(host["paddle_params"], g["a_paddle_params"][k]), k
        assert np.array_equal(host["block_params"], g["a_block_params"][k]), k
        assert np.array_equal(host["ball_params"], g["a_ball_params"][k]), k
        # the corners are the params read backwards (get_pos_dims, encoder.py:140-145)
        x, y, w, h = g["a_paddle_params"][k]
        assert host["paddle"].tolist() == [y - h / 2, x - w / 2, y + h / 2, x + w / 2], k
    assert int(g["a_nblocks"].min()) <= 5 and int(g["a_nblocks"].max()) >= 30


def test_the_layout_defaults_are_the_constants_of_the_reference():
    from lcp_physics_amd.physics.breakout import FrameLayout
    g = np.load(GOLDEN)
    L = FrameLayout.atari()
    assert L.words() == EH.layout_words(EH.ATARI)
    w = lambda n: g["w_" + n]
    assert (L.height, L.width, L.paddle_line, L.paddle_h, L.paddle_w, L.ball_w, L.band_h) == tuple(
        int(w(n)) for n in ("SCREEN_HEIGHT", "SCREEN_WIDTH", "PADDLE_TOP_LINE", "PADDLE_HEIGHT", "PADDLE_WIDTH", "BALL_WIDHT", "BLOCK_HEIGHT"))
    assert L.band_top == int(w("BLOCKS_TOP_LEFT")[0]) and L.nrows == len(w("BLOCK_COLORS"))
    assert list(L.row_key) == w("BLOCK_COLORS")[:, 0].tolist() and [list(c) for c in L.row_colors] == w("BLOCK_COLORS").tolist()
    assert L.paddle_key == int(w("PADDLE_COLOR")[0]) and L.ball_key == int(w("BALL_COLOR")[0])
    assert (L.wall_w, L.roof_line, L.stopper_line, L.stopper_w, L.stopper_h, L.dt, L.fric, L.ball_mass, L.restitution, L.stopper_restitution) == tuple(
        float(w(n)) for n in ("WALL_WIDTH", "ROOF_LINE", "STOPPER_LINE", "STOPPER_WIDTH", "STOPPER_HEIGHT", "DT", "FRIC_COEFF", "BALL_MASS",
                              "STD_RESTITUTION", "STOPPER_RESTITUTION"))
    # encoder.py:104-105: the erase rect is the red stopper
    assert L.erase == (int(w("STOPPER_LINE")), int(w("SCREEN_WIDTH") - w("STOPPER_WIDTH")), int(w("STOPPER_LINE") + w("STOPPER_HEIGHT") - 1),
                       int(w("SCREEN_WIDTH")))
    assert list(L.wall_color) == w("WALL_COLOR").tolist() and list(L.left_stopper_color) == w("LEFT_STOPPER_COLOR").tolist()


@pytest.mark.skipif(not ref_shim.reference_available(), reason="needs the reference tree")
def test_the_restatement_reproduces_the_reference_live_on_200_random_frames():
    enc, _ = EH.load_reference_experiment()
    rng = np.random.default_rng(1234)
    counts = []
    for k in range(200):
        key = EH.random_frame(rng)
        host = EH.extract_host(key)
        assert host["status"] & ~EH.ST_NO_BALL == 0, k            # (frames the reference returns from)
        paddle, blocks, ball = enc.extract_params(EH.to_frame(key, 3, rng))
        flat = lambda pd: [float(pd[0][0]), float(pd[0][1]), float(pd[1][0]), float(pd[1][1])]
        assert flat(paddle) == host["paddle_params"].tolist(), k
        assert [flat(b) for b in blocks] == host["block_params"].tolist(), k
        assert [float(ball[0][0]), float(ball[0][1]), float(ball[1])] == host["ball_params"].tolist(), k
        counts.append(len(blocks))
    assert min(counts) <= 5 and max(counts) >= 30


def test_the_restatement_flags_what_the_reference_does_not_return_from():
    rng = np.random.default_rng(5)
    key = EH.synth(rng, p_missing=0.5)
    top = EH.ATARI["band_top"] + 2 * EH.ATARI["band_h"]
    edge = key.copy()
    edge[top, 150:] = EH.ATARI["row_key"][2]
    a, b = EH.extract_host(key), EH.extract_host(edge)
    assert b["status"] & EH.ST_RUN_AT_EDGE and not a["status"] & EH.ST_RUN_AT_EDGE
    assert b["nblocks"] <= a["nblocks"] and np.array_equal(a["paddle"], b["paddle"])
    probe = key.copy()
    probe[EH.ATARI["paddle_line"]] = 0
    probe[EH.ATARI["paddle_line"], 158:] = 255
    assert EH.extract_host(probe)["status"] & EH.ST_PADDLE_PROBE
    assert EH.extract_host(key, max_blocks=2)["status"] & EH.ST_TRUNCATED


@pytest.mark.parametrize("change", [dict(paddle_key=0), dict(ball_key=256), dict(row_key=(200, 0, 180, 162, 72, 66)), dict(paddle_line=210),
                                    dict(band_top=-1), dict(band_top=160), dict(nrows=9), dict(band_h=0), dict(paddle_w=0),
                                    dict(erase=(189, 152, 188, 160)), dict(erase=(189, -1, 194, 160))])
def test_layout_validation(change):
    import dataclasses
    from lcp_physics_amd.physics.breakout import FrameLayout
    FrameLayout.atari().validate(210, 160, 32)
    with pytest.raises(ValueError):
        dataclasses.replace(FrameLayout.atari(), **change).validate(210, 160, 32)


@pytest.mark.parametrize("H,W,mb", [(210, 0, 8), (210, 1025, 8), (189, 160, 8), (210, 160, 0), (210, 160, 257)])
def test_sizes_outside_the_entry_s_limits_are_refused(H, W, mb):
    from lcp_physics_amd.physics.breakout import FrameLayout
    with pytest.raises(ValueError):
        FrameLayout.atari().validate(H, W, mb)


def test_host_frames_raise():
    from lcp_physics_amd.physics.breakout import extract_params
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract_params(torch.zeros(2, 210, 160, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        extract_params(np.zeros((2, 210, 160, 3), dtype=np.uint8))


def test_state_vector_round_trip():
    from lcp_physics_amd.physics.breakout import BreakoutParams, from_vector, to_vector
    p = BreakoutParams.empty(3, 5, "cpu")
    gen = torch.Generator().manual_seed(0)
    p.paddle_params.copy_(torch.rand(3, 4, generator=gen, dtype=torch.float64))
    p.block_params.copy_(torch.rand(3, 5, 4, generator=gen, dtype=torch.float64))
    p.ball_params.copy_(torch.rand(3, 3, generator=gen, dtype=torch.float64))
    s = to_vector(p)
    assert s.shape == (3, 4 + 4 * 5 + 3)
    a, b, c = from_vector(s, 5)
    assert torch.equal(a, p.paddle_params) and torch.equal(b, p.block_params) and torch.equal(c, p.ball_params)
    with pytest.raises(ValueError):
        from_vector(s, 4)


def test_a_rendered_scene_of_integer_rects_is_crisp_and_reads_back():
    """What tests/test_hip_encoder.py relies on for its round trip with `render`, confirmed on the CPU with the drawing's
    restatement: rects with integer corners at one pixel per unit have coverage 0 or 1 everywhere, and the encoder's restatement
    reads paddle, blocks and ball back from the quantised image."""
    from tests import render_host as RH
    H, W = 60, 64
    L = EH.scaled_layout(H, W)
    rng = np.random.default_rng(9)
    outs = [EH.extract_host(EH.synth(rng, L, H, W, p_missing=0.5), L) for _ in range(2)]
    nslots = max(o["nblocks"] for o in outs) + 1
    image, _, _ = RH.render_host(EH.render_case(outs, L, H, W, nslots))
    # every pixel centre is half a pixel from the nearest edge, where the one-pixel ramp ends: coverage is 0 or 1 (to rounding)
    # and every pixel holds a body's colour or the background, a whole number of 255ths
    off = float((image * 255.0 - torch.round(image * 255.0)).abs().max())
    assert off < 1e-4, off                                       # (the colours are float32: 255 x 2^-24 relative)
    frames = torch.round(image.clamp(0.0, 1.0) * 255.0).to(torch.uint8).numpy()
    for b, o in enumerate(outs):
        back = EH.extract_host(frames[b, 0], L)
        assert back["status"] == 0 and back["nblocks"] == o["nblocks"] > 0
        assert np.array_equal(back["paddle"], o["paddle"]) and np.array_equal(back["blocks"], o["blocks"])
        assert np.array_equal(back["ball"], o["ball"])
