"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of lcp_extract_params_u8: guard bands
around every buffer, the frame bitwise unchanged, each optional output NULL in turn, nothing read outside the key plane - the frame
buffer ENDS with the last key byte of the last row, so with stride_col = 3 the two bytes a whole pixel would still have are guard
bytes, 0xFF in one run and 0x00 in the other: a kernel that read them (255 beats every key in the paddle line's maximum) would
give different answers -, outputs written and not accumulated, refusals that write nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import encoder_host as EH
from tests.test_hip_buffer_contract import F64, I32, U8, Call, Case, R, _check, _run, _same

pytestmark = pytest.mark.gpu
OUTS = ("paddle", "blocks", "nblocks", "ball", "enc_status", "paddle_params", "block_params", "ball_params")
HOST = ("paddle", "blocks", "nblocks", "ball", "status", "paddle_params", "block_params", "ball_params")


def _case(H, W, sc, B=3, max_blocks=12, pad_row=0, twice=False, seed=0):
    """B random frames of the scaled layout as a byte buffer with column stride `sc`, `pad_row` bytes of 0xFF between rows, cut
    after the last key byte; the other channels' bytes are random."""
    L = EH.scaled_layout(H, W) if (H, W) != (EH.ATARI_H, EH.ATARI_W) else EH.ATARI
    rng = np.random.default_rng(1000 * W + 10 * sc + seed)
    keys = np.stack([EH.random_frame(rng, L, H, W) for _ in range(B)])
    sr = W * sc + pad_row
    sb = H * sr
    raw = rng.integers(0, 256, size=(B, H, sr), dtype=np.uint8)
    raw[:, :, W * sc:] = 255
    raw[:, :, 0:W * sc:sc] = keys
    nbytes = (B - 1) * sb + (H - 1) * sr + (W - 1) * sc + 1
    frame = torch.from_numpy(raw.reshape(-1)[:nbytes].copy())
    words = (ctypes.c_int32 * 21)(*EH.layout_words(L))
    bufs = [("frame", U8, (nbytes,), "in", frame),
            ("paddle", I32, (B, 4), "out", None), ("blocks", I32, (B, max_blocks, 4), "out", None), ("nblocks", I32, (B,), "out", None),
            ("ball", I32, (B, 4), "out", None), ("enc_status", I32, (B,), "out", None), ("paddle_params", F64, (B, 4), "out", None),
            ("block_params", F64, (B, max_blocks, 4), "out", None), ("ball_params", F64, (B, 3), "out", None)]
    args = [B, H, W, R("frame"), sb, sr, sc, ctypes.cast(words, ctypes.c_void_p), max_blocks] + [R(n) for n in OUTS]
    want = EH.extract_host_batch(keys, L, max_blocks)

    def post(outs):
        for n, h in zip(OUTS, HOST):
            assert np.array_equal(outs[n].numpy(), want[h]), n

    case = Case(B, bufs, [Call("lcp_extract_params_u8", args, OUTS)] * (2 if twice else 1), nulls=[{n} for n in OUTS], post=post)
    case.keep = words                                                              # (the host words outlive the calls)
    return case, args


@pytest.mark.parametrize("H,W,sc,pad_row", [(50, 65, 3, 0), (50, 40, 1, 0), (50, 64, 4, 0), (50, 65, 3, 7), (50, 65, 5, 0), (210, 160, 3, 0)])
def test_guards_optional_outputs_and_nothing_read_outside_the_key_plane(H, W, sc, pad_row):
    """Guards intact, the frame const, every output element written, the restatement's answers, the same bits with the arena
    carved in reverse and zero-filled (the bytes after the last key byte are guards), and with each output NULL in turn.
    65 x 3: rows of 195 bytes start at every alignment; stride 5: the gathered path; 7 bytes of 0xFF between rows."""
    _check(_case(H, W, sc, pad_row=pad_row)[0])


def test_outputs_are_overwritten_not_accumulated():
    once, _, _ = _run(_case(50, 65, 3)[0])
    twice, _, _ = _run(_case(50, 65, 3, twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_an_empty_batch_is_success_without_a_launch():
    case, args = _case(50, 65, 3)
    case.steps = [Call("lcp_extract_params_u8", [0] + args[1:], ())]
    outs, _, _ = _run(case)
    for n in OUTS:
        assert bool((outs[n].view(-1).view(U8) == 0xFF).all()), n


def test_refusals_write_nothing():
    """Sizes outside the limits, a missing frame or layout, no output, a stride of 0, a bad layout: LCP_E_BADARG, nothing touched."""
    case, args = _case(50, 65, 3)
    L = EH.scaled_layout(50, 65)
    with_arg = lambda k, v: args[:k] + [v] + args[k + 1:]
    bad = [with_arg(0, -1), with_arg(1, 0), with_arg(2, 0), with_arg(2, 1025), with_arg(3, R("frame_missing")), with_arg(4, 0), with_arg(5, 0),
           with_arg(6, 0), with_arg(6, -3), with_arg(7, None), with_arg(8, 0), with_arg(8, 257), args[:9] + [None] * 8]
    keep = []
    for change in (dict(paddle_key=0), dict(ball_key=256), dict(paddle_line=50), dict(band_top=45), dict(nrows=9), dict(band_h=0),
                   dict(erase=(44, 3, 43, 9)), dict(row_key=(200, 0, 180, 162))):
        words = (ctypes.c_int32 * 21)(*EH.layout_words(dict(L, **change)))
        keep.append(words)
        bad.append(with_arg(7, ctypes.cast(words, ctypes.c_void_p)))
    case.steps = [Call("lcp_extract_params_u8", a, OUTS, rc=-1) for a in bad]
    _run(case)
