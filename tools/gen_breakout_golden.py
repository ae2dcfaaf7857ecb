"""Generate tests/golden/breakout.npz from the UNMODIFIED reference experiment (experiments/breakout/encoder.py,
run_breakout.py).  TEST INFRASTRUCTURE ONLY; needs the reference tree (oracle/ref_shim.py) and runs on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_breakout_golden.py

`run_breakout.py` imports `gym` and `mpc.mpc` at module level and uses neither in `simulate_breakout` / `to_vector` /
`from_vector`: empty stand-in modules carrying the three imported names are placed in `sys.modules`, no reference file is touched.

(a) `a_*`: 48 synthetic frames (tests/encoder_host.py `synth`; only channel 0, the key plane, is stored) and what the reference's
    `extract_params` returns for them: paddle (pos, dims), blocks (pos, dims; padded with the placeholder of run_breakout.py:56),
    their number, ball (pos, rad).  Asserted: every special case of the rule occurs at least once.
(b) `r_*`: three roll-outs through the reference's `make_world` + `simulate_breakout` on frames of at most 8 blocks: per step the
    state vector, the clock, the number of sub-steps and of contacts; d(mean squared state[:, :4] of the last step) /
    d(paddle_vel_x, paddle_vel_y) from the reference's autograd.  Asserted: one bounces off a block, one off the paddle with a step
    of more than one sub-step, one off a wall; a second run reproduces counts and clocks; the initial ball moved by 1e-7 changes no
    count (a roll-out that sits on a halving tie is not a fixture).
(c) `w_*`: the constants of encoder.py:17-60 as the reference module holds them.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from tests import encoder_host as EH  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "breakout.npz")
MAXB = 8                                          # block slots of the roll-outs' state vectors


load_experiment = EH.load_reference_experiment


def reference_params(enc, key, rng):
    """`extract_params` of the unmodified reference on a 3-channel frame whose channel 0 is `key`, flattened."""
    paddle, blocks, ball = enc.extract_params(EH.to_frame(key, 3, rng))
    flat = lambda pd: [float(pd[0][0]), float(pd[0][1]), float(pd[1][0]), float(pd[1][1])]
    return (np.array(flat(paddle)), np.array([flat(b) for b in blocks]).reshape(-1, 4),
            np.array([float(ball[0][0]), float(ball[0][1]), float(ball[1])]))


def frames_a():
    """(key, tags) of the 48 frames; tags name the special cases a frame was built for."""
    rng = np.random.default_rng(20260)
    out = []
    add = lambda tags, **kw: out.append((EH.synth(rng, **kw), tags))
    add({"paddle_row"}, ball="paddle_row", p_missing=0.3)
    add({"paddle_row"}, ball="paddle_row", p_missing=0.6, paddle_x=100)
    add({"gap_top"}, ball="gap_top", p_missing=0.4)
    add({"gap_top"}, ball="gap_top", p_missing=0.7)
    add({"under_rect", "clipped"}, ball="under_paddle", p_missing=0.3)
    add({"under_rect", "clipped"}, ball="under_paddle", p_missing=0.5, paddle_x=20)
    add({"no_ball"}, ball="none", p_missing=0.3)
    add({"no_ball"}, ball="none", p_missing=0.8)
    add({"clipped"}, long_paddle=True)
    add({"stray_top"}, stray_top=2, p_missing=0.4)
    add({"stray_top"}, stray_top=0, p_missing=0.5)
    add({"run_at_zero"}, run_at_zero=1, p_missing=0.5)
    add({"run_at_zero"}, run_at_zero=4, p_missing=0.3)
    add({"few"}, keep=5, p_missing=0.5)
    add({"few"}, keep=8, p_missing=0.5)
    add({"many"}, p_missing=0.5)
    add({"many"}, p_missing=0.45, strays=2)
    while len(out) < 48:
        out.append((EH.random_frame(rng), set()))
    return out


def fixture_a(enc):
    rng = np.random.default_rng(7)
    frames = frames_a()
    keys = np.stack([k for k, _ in frames])
    P, BL, N, BA = [], [], [], []
    seen = set()
    for key, tags in frames:
        paddle, blocks, ball = reference_params(enc, key, rng)
        host = EH.extract_host(key)
        assert np.array_equal(paddle, host["paddle_params"]) and np.array_equal(blocks, host["block_params"]) \
            and np.array_equal(ball, host["ball_params"]), "the restatement of tests/encoder_host.py differs from the reference"
        P.append(paddle); BL.append(blocks); N.append(len(blocks)); BA.append(ball)
        # what the frame exercises, read off the reference's answer and the frame itself
        L = EH.ATARI
        row = key[L["paddle_line"]]
        first = int(np.argmax(row))
        if row[first + L["ball_w"] + 1] != L["paddle_key"] and "paddle_row" in tags:
            assert paddle[0] - paddle[2] / 2 > first, "second argmax"
            seen.add("paddle_row")
        if "gap_top" in tags:
            assert any(b[2] == L["ball_w"] and b[1] == L["band_top"] + L["band_h"] / 2 for b in blocks), "the ball became a block"
            assert host["ball"][2] == L["band_top"], "the ball ends where the block's rect begins"
            seen.add("gap_top")
        if "under_rect" in tags:
            assert host["removed"][host["ball"][2], host["ball"][1]] and key[host["ball"][2], host["ball"][1]] == L["ball_key"]
            seen.add("under_rect")
        if host["status"] & EH.ST_NO_BALL:
            assert ball[1] == 100 * EH.ATARI_H
            seen.add("no_ball")
        px = int(host["paddle"][1])
        if paddle[2] == L["paddle_w"] and row[px + L["paddle_w"]] == L["paddle_key"]:
            seen.add("clipped")
        if any(b[2] == 1 for b in blocks):
            seen.add("stray_top")
        for i in range(L["nrows"]):
            eq = key[L["band_top"] + i * L["band_h"]] == L["row_key"][i]
            if eq[0] and np.flatnonzero(np.diff(eq.astype(np.int8)) == 1).size:
                assert not any(b[1] == L["band_top"] + i * L["band_h"] + L["band_h"] / 2 for b in blocks), "a band that starts at column 0 lists nothing"
                seen.add("run_at_zero")
        assert host["status"] & ~EH.ST_NO_BALL == 0
    want = {"paddle_row", "gap_top", "under_rect", "no_ball", "clipped", "stray_top", "run_at_zero"}
    assert seen == want, ("special cases missing", want - seen)
    assert min(N) <= 5 and max(N) >= 30, ("block counts", min(N), max(N))
    nmax = max(N)
    blocks = np.tile(np.array(EH.PLACEHOLDER), (len(frames), nmax, 1))
    for k, b in enumerate(BL):
        blocks[k, :len(b)] = b
    print("(a) %d frames, blocks per frame %d .. %d, special cases %s" % (len(frames), min(N), max(N), sorted(seen)))
    return dict(a_key=keys, a_paddle_params=np.stack(P), a_block_params=blocks, a_nblocks=np.array(N, dtype=np.int32), a_ball_params=np.stack(BA))


# the three roll-outs: (name, synth arguments, ball velocity, actions, paddle speeds - exactly representable in fp32)
ROLLOUTS = (
    ("block", dict(keep=4, p_missing=0.5, paddle_x=90, ball=(70, 0)), (0.5, -3.0), (1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0), (3.75, 0.5)),
    ("paddle", dict(keep=6, p_missing=0.5, paddle_x=60, ball=(172, 66)), (1.0, 5.0), (-1.0, 1.0, -1.0, -1.0, 1.0, -1.0, 1.0, 1.0), (0.5, 3.75)),
    ("wall", dict(keep=8, p_missing=0.5, paddle_x=100, ball=(130, 16)), (-5.0, 1.0), (-1.0, 1.0, 1.0, -1.0, 1.0, 1.0), (3.75, 0.5)),
)


def rollout_frame(name, kw):
    rng = np.random.default_rng({"block": 11, "paddle": 12, "wall": 13}[name])
    kw = dict(kw)
    if name == "block":
        # under the first brick of band 0 that is drawn
        probe = EH.synth(np.random.default_rng(11), **dict(kw, ball="none"))
        cols = np.flatnonzero(probe[EH.ATARI["band_top"]] == EH.ATARI["row_key"][0])
        kw["ball"] = (kw["ball"][0], int(cols[0]) + 3)
    return EH.synth(rng, **kw)


def run_rollout(enc, rb, key, ball_vel, actions, paddle_vel, shift=0.0):
    """The reference's loop: extract_params -> to_vector -> from_vector -> make_world, then simulate_breakout per action."""
    rng = np.random.default_rng(3)
    s = rb.to_vector(*enc.extract_params(EH.to_frame(key, 3, rng)))
    if shift:
        s = s.clone()
        s[-3:-1] += shift
    world, ball, paddle, blocks, paddle_idx = enc.make_world(*rb.from_vector(s), torch.tensor(ball_vel, dtype=torch.float64))
    vx = torch.tensor(paddle_vel[0], dtype=torch.float64, requires_grad=True)
    vy = torch.tensor(paddle_vel[1], dtype=torch.float64, requires_grad=True)
    inner, calls = world.step_dt, []

    def step_dt(dt):
        inner(dt)
        calls.append(float(dt))
    world.step_dt = step_dt
    S, T, NS, NC, BV = [s.detach().numpy().copy()], [float(world.t)], [], [], []
    sn = None
    for a in actions:
        before = len(calls)
        sn = rb.simulate_breakout(a, world, ball, paddle, blocks, paddle_idx, paddle_vel_x=vx, paddle_vel_y=vy)
        S.append(sn.detach().numpy().reshape(-1).copy()); T.append(float(world.t)); NS.append(len(calls) - before)
        NC.append(len(world.contacts)); BV.append(ball.v.detach().numpy().copy())
    loss = (sn[:, :4] ** 2).mean()
    loss.backward()
    return dict(state=np.stack(S), t=np.array(T), nsub=np.array(NS), ncontacts=np.array(NC), ball_v=np.stack(BV),
                loss=float(loss), grad=np.array([float(vx.grad), float(vy.grad)]), nblocks=len(blocks))


def fixture_b(enc, rb):
    out = {}
    nsteps = max(len(r[3]) for r in ROLLOUTS)
    keys, recs = [], []
    for name, kw, ball_vel, actions, pv in ROLLOUTS:
        key = rollout_frame(name, kw)
        rec = run_rollout(enc, rb, key, ball_vel, actions, pv)
        again = run_rollout(enc, rb, key, ball_vel, actions, pv)
        assert np.array_equal(rec["nsub"], again["nsub"]) and np.array_equal(rec["t"], again["t"]) \
            and np.array_equal(rec["ncontacts"], again["ncontacts"]), (name, "not reproducible")
        for shift in (1e-7, -1e-7):
            moved = run_rollout(enc, rb, key, ball_vel, actions, pv, shift=shift)
            assert np.array_equal(rec["nsub"], moved["nsub"]) and np.array_equal(rec["ncontacts"], moved["ncontacts"]), \
                (name, "sits on a tie: the ball moved by %g changes a count" % shift, rec["nsub"], moved["nsub"], rec["ncontacts"], moved["ncontacts"])
        assert 1 <= rec["nblocks"] <= MAXB
        assert np.abs(rec["t"] - np.arange(len(rec["t"]))).max() < 1e-12, (name, "clock off the grid")
        v = rec["ball_v"]                                              # (rot, x, y) per step
        v0 = np.array([0.0, *ball_vel])
        flips = lambda c: bool((np.sign(v[:, c]) == -np.sign(v0[c])).any())
        bx, by = rec["state"][:, -3], rec["state"][:, -2]
        if name == "block":
            assert flips(2) and by.min() < 70 and by.min() > 60, (name, "no bounce off the block", by, v)
        if name == "paddle":
            assert flips(2) and int(rec["nsub"].max()) > 1 and by.max() > 180, (name, "no bounce off the paddle / no halving", by, rec["nsub"])
        if name == "wall":
            assert flips(1) and bx.min() < 12, (name, "no bounce off the wall", bx, v)
        assert np.isfinite(rec["grad"]).all() and np.abs(rec["grad"]).max() > 0
        print("(b) %-6s blocks %d  sub-steps %s  contacts %s  loss %.4f  grad %s" % (name, rec["nblocks"], rec["nsub"].tolist(),
                                                                                     rec["ncontacts"].tolist(), rec["loss"], rec["grad"]))
        keys.append(key); recs.append(rec)
    ns = 4 + 4 * MAXB + 3
    state = np.zeros((len(recs), nsteps + 1, ns))
    pad = lambda a, fill: np.concatenate([a, np.full(nsteps - len(a), fill, dtype=a.dtype)])
    for k, r in enumerate(recs):
        n = r["nblocks"]
        s = r["state"]
        full = np.concatenate([s[:, :4 + 4 * n], np.tile(np.array(EH.PLACEHOLDER), (len(s), MAXB - n)), s[:, -3:]], axis=1)
        state[k, :len(s)] = full
    out.update(r_names=np.array([r[0] for r in ROLLOUTS]), r_key=np.stack(keys), r_ball_vel=np.array([r[2] for r in ROLLOUTS]),
               r_actions=np.stack([pad(np.array(r[3]), 0.0) for r in ROLLOUTS]), r_nsteps=np.array([len(r[3]) for r in ROLLOUTS]),
               r_paddle_vel=np.array([r[4] for r in ROLLOUTS]), r_state=state, r_nblocks=np.array([r["nblocks"] for r in recs]),
               r_t=np.stack([pad(r["t"][1:], -1.0) for r in recs]), r_nsub=np.stack([pad(r["nsub"], -1) for r in recs]),
               r_ncontacts=np.stack([pad(r["ncontacts"], -1) for r in recs]), r_loss=np.array([r["loss"] for r in recs]),
               r_grad=np.stack([r["grad"] for r in recs]))
    return out


def constants(enc):
    names = ("SCREEN_HEIGHT", "SCREEN_WIDTH", "PADDLE_TOP_LINE", "PADDLE_HEIGHT", "PADDLE_WIDTH", "BALL_WIDHT", "BLOCK_HEIGHT", "WALL_WIDTH",
             "ROOF_LINE", "STOPPER_LINE", "STOPPER_WIDTH", "STOPPER_HEIGHT", "DT", "FRIC_COEFF", "BALL_MASS", "STD_RESTITUTION",
             "STOPPER_RESTITUTION")
    out = {"w_" + n: np.float64(getattr(enc, n)) for n in names}
    out.update(w_BLOCKS_TOP_LEFT=np.array(enc.BLOCKS_TOP_LEFT), w_BLOCK_COLORS=np.array(enc.BLOCK_COLORS), w_PADDLE_COLOR=np.array(enc.PADDLE_COLOR),
               w_BALL_COLOR=np.array(enc.BALL_COLOR), w_WALL_COLOR=np.array(enc.WALL_COLOR), w_LEFT_STOPPER_COLOR=np.array(enc.LEFT_STOPPER_COLOR))
    return out


def main():
    enc, rb = load_experiment()
    torch.set_default_dtype(torch.float64)
    flat = fixture_a(enc)
    flat.update(fixture_b(enc, rb))
    flat.update(constants(enc))
    np.savez_compressed(OUT, **flat)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    assert size < 150 * 1024, "the fixture must stay below 150 KB"


if __name__ == "__main__":
    main()
