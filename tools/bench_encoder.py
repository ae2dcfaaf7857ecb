"""Time the breakout encoder (lcp_encoder.hip through `physics.breakout.extract_params`) on a batch of frames.

    python tools/bench_encoder.py [--out profiles/encoder.json]        # needs the GPU
    python tools/bench_encoder.py --resources-only [--out ...]         # no GPU: (re)fill the kernel's register / scratch / LDS use
                                                                       # from lcp_physics_amd/csrc/asm/lcp_encoder.fixed.s

Shapes: 4096 frames of 210 x 160 x 3 as gym hands them out ([B,H,W,C]: the key plane has a column stride of 3 bytes, so every
16-byte line of the rows read is touched) and as `FrameRecorder` keeps them ([B,C,H,W]: the key plane is contiguous, a third of the
bytes).  The frames are 256 synthetic ones (tests/encoder_host.py `random_frame`) repeated; the answers are checked against the
numpy restatement before anything is timed.  One call = one launch into preallocated outputs; HIP events around windows of at
least 0.2 s after a spin-up, the two shapes alternating, the median of 7 windows and their spread.

Bytes: `frame_bytes` is the whole frame (HWC) or the whole key plane (CHW); `bytes_read` what the kernel actually stages - the
paddle line, the bands' top lines and the blocks of 16 rows down to the one that holds the ball (the scan leaves there), computed
from the answers.  Both over the call time as a fraction of the 8 TB/s peak.  The only comparator that exists on the machine that
runs this is the numpy restatement on its CPU (time per frame over 64 frames); the one condition is that the batch call beats it
over the same batch.
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import encoder_host as EH  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
ASM = os.path.join(ROOT, "lcp_physics_amd", "csrc", "asm", "lcp_encoder.fixed.s")
B, DISTINCT, MAXB, SCAN_ROWS = 4096, 256, 40, 16


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


def measure(dev):
    from lcp_physics_amd.physics.breakout import BreakoutParams, extract_params
    rng = np.random.default_rng(2026)
    keys = np.stack([EH.random_frame(rng) for _ in range(DISTINCT)])
    t0 = time.perf_counter()
    want = EH.extract_host_batch(keys[:64], max_blocks=MAXB)
    host_per_frame = (time.perf_counter() - t0) / 64
    want = EH.extract_host_batch(keys, max_blocks=MAXB)
    H, W = keys.shape[1:]
    rep = B // DISTINCT
    hwc = torch.from_numpy(EH.to_frame(keys, 3, rng)).to(dev).repeat(rep, 1, 1, 1).contiguous()
    chw = hwc.permute(0, 3, 1, 2).contiguous()
    outs = {"HWC": BreakoutParams.empty(B, MAXB, dev), "CHW": BreakoutParams.empty(B, MAXB, dev)}
    fns = {"HWC": lambda: extract_params(hwc, out=outs["HWC"]), "CHW": lambda: extract_params(chw, channels_first=True, out=outs["CHW"])}
    for name, fn in fns.items():                                                       # the answers first
        fn()
        torch.cuda.synchronize()
        for n, v in want.items():
            got = getattr(outs[name], n).cpu().numpy()
            assert np.array_equal(got, np.concatenate([v] * rep)), (name, n)
    # rows staged per frame: the bands' top lines and the paddle line, then blocks of SCAN_ROWS rows down to the ball's
    ball_row = np.where(want["status"] & EH.ST_NO_BALL, H - 1, want["ball"][:, 0])
    rows = EH.ATARI["nrows"] + 1 + np.minimum((ball_row // SCAN_ROWS + 1) * SCAN_ROWS, H)
    rows_mean = float(rows.mean())
    for fn in fns.values():                                                            # spin-up
        window(fn, 0.3)
    runs = {k: [] for k in fns}
    for _ in range(7):                                                                 # alternating
        for k, fn in fns.items():
            runs[k].append(window(fn))
    res = {"B": B, "H": int(H), "W": int(W), "C": 3, "max_blocks": MAXB, "distinct_frames": DISTINCT, "rows_staged_mean": round(rows_mean, 2),
           "blocks_per_frame": [int(want["nblocks"].min()), int(want["nblocks"].max())],
           "host_restatement_us_per_frame": round(host_per_frame * 1e6, 1),
           "host_restatement_s_per_batch": round(host_per_frame * B, 3)}
    for k, v in runs.items():
        sc = 3 if k == "HWC" else 1
        t = float(np.median(v))
        frame_bytes, read = B * H * W * sc, B * rows_mean * W * sc
        res[k] = {"call_us": round(t * 1e6, 2), "call_spread_us": [round(min(v) * 1e6, 2), round(max(v) * 1e6, 2)],
                  "ns_per_frame": round(t * 1e9 / B, 2), "frame_bytes": int(frame_bytes), "bytes_read": int(read),
                  "frame_bytes_fraction_of_peak_bandwidth": round(frame_bytes / t / PEAK_BYTES_PER_S, 4),
                  "bytes_read_fraction_of_peak_bandwidth": round(read / t / PEAK_BYTES_PER_S, 4),
                  "host_restatement_over_call": round(host_per_frame * B / t, 1)}
        assert t < host_per_frame * B, "the batch call must beat the host restatement over the same batch"
    return res


def kernel_resources():
    """Registers, scratch and static LDS of lcp_extract_params_kernel, from the metadata of the assembly the build left, and whether
    the kernel makes a call."""
    if not os.path.exists(ASM):
        return None
    keys = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
    blocks, calls = [], 0
    for line in open(ASM):
        calls += bool(re.match(r"\s+s_(swappc|call)_b64", line))
        m = re.match(r"  (- | {2})\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "- ":
            blocks.append({})
        if blocks:
            blocks[-1][m.group(2)] = m.group(3)
    for b in blocks:
        if "lcp_extract_params_kernel" in b.get("name", ""):
            out = {k: int(b[k]) for k in keys if k in b}
            out["calls"] = calls
            out["dynamic_lds_bytes_210x160x3"] = 16 * 496 + 1280        # 16 rows of 31 lines and the tables (extract_params_launch)
            return out
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    else:
        assert torch.cuda.is_available(), "bench_encoder.py measures on the GPU; there is no CPU timing"
        doc = {"device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_BYTES_PER_S, "shape_4096x210x160x3": measure(torch.device("cuda:0")),
               "reference_extract_params_ms_per_frame_cpu_single_rough_run_elsewhere": 9.0}
    res = kernel_resources()
    if res is not None or "kernel" not in doc:
        doc["kernel"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
