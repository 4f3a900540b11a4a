"""The oracle's pinned max-pool (critic_apply(picks=...), oracle/hourglass_ref.py), its chunked phase-2 step and the decoders of the
kernels' argmax buffers (tests/pool_picks.py).  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hourglass_ref as orc
import pool_picks

torch.set_num_threads(4)


def own_picks(P, X, p=0.0, masks=None):
    """max_pool2d's own indices, as window positions, of the forward critic_apply makes on X (training-mode dropout with ``masks``)."""
    out, h = [], X
    with torch.no_grad():
        for i, key in enumerate(orc.ENC_CONV_KEYS):
            y = F.relu(F.conv2d(h, P[key + ".weight"], P[key + ".bias"], padding=1))
            h, idx = F.max_pool2d(y, 2, return_indices=True)
            W = y.shape[-1]
            out.append((idx // W % 2) * 2 + idx % W % 2)
            if i >= 2 and masks is not None:
                h = orc._drop(h, p, True, masks[i - 2])
    return out


def _problem(chfak, n, seed, p=0.3, dtype=torch.float32):
    rs = np.random.RandomState(seed)
    pc = {k: v.to(dtype) for k, v in orc.seeded_params(orc.critic_shapes(chfak), 21).items()}
    pm = {k: v.to(dtype) for k, v in orc.seeded_params(orc.masker_shapes(chfak), 22).items()}
    A = orc.u8_to_nchw(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)).to(dtype)
    B = orc.u8_to_nchw(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)).to(dtype)
    Y = torch.from_numpy(rs.rand(n)).to(dtype)
    d2, d3, nb = 8 * chfak, 16 * chfak, 32 * chfak
    masks = [[torch.from_numpy((rs.rand(*s) >= p).astype(np.float32)).to(dtype) for s in ((n, d2, 8, 8), (n, d3, 4, 4), (n, nb))]
             for _ in range(4)]
    return pc, pm, A, B, Y, masks


def _phase2_own_picks(pc, pm, A, B, Y, masks, p):
    """Each pass's own max_pool2d picks: the mixes are formed from the unpinned step's Z exactly as phase2_loss forms them."""
    with torch.no_grad():
        _, _, Z, _ = orc.phase2_loss(pc, pm, A, B, Y, p=p, training=True, masks=masks)
    return [own_picks(pc, X, p, m) for X, m in zip((A, B, A * (1 - Z) + Z * B, B * (1 - Z) + Z * A), masks)]


def _assert_records_equal(r0, r1):
    assert r0["total"] == r1["total"] and r0["parts"] == r1["parts"]
    assert torch.equal(r0["Z"], r1["Z"]) and torch.equal(r0["pred"], r1["pred"])
    for grp in ("grads_c", "grads_m", "params_c", "params_m"):
        for k, v in r0[grp].items():
            assert torch.equal(v, r1[grp][k]), f"{grp} {k}"


@pytest.mark.parametrize("chfak", [1, 5])
def test_pinned_to_max_pool_indices_is_bitwise_the_oracle(chfak):
    """picks = max_pool2d's own indices: loss, pred, Z, every gradient and the parameters after Adam bitwise as without picks
    (phase 2 with dropout masks, and phase 1)."""
    n, p = 3, 0.3
    pc, pm, A, B, Y, masks = _problem(chfak, n, 5 + chfak, p)
    picks = _phase2_own_picks(pc, pm, A, B, Y, masks, p)
    batch = [(A, B, Y)]
    r0 = orc.train_phase2(pc, pm, batch, steps=1, p=p, training=True, masks=masks)[0]
    r1 = orc.train_phase2(pc, pm, batch, steps=1, p=p, training=True, masks=masks, picks=picks)[0]
    _assert_records_equal(r0, r1)
    q0 = orc.train_phase1(pc, [(A, Y)], steps=1, p=p, masks=masks[0])[0]
    q1 = orc.train_phase1(pc, [(A, Y)], steps=1, p=p, masks=masks[0], picks=picks[0])[0]
    assert q0["loss"] == q1["loss"] and torch.equal(q0["pred"], q1["pred"])
    for k in q0["grads"]:
        assert torch.equal(q0["grads"][k], q1["grads"][k]) and torch.equal(q0["params"][k], q1["params"][k]), k


def test_moving_one_pick_moves_that_windows_dy_to_the_new_pixel():
    """A window of features.0 whose four candidates tie exactly (a flat patch): moving its pick from position 0 to 3 leaves every value
    and every gradient above that stage bitwise as it was, and moves the window's dy to exactly the new pixel -- the image gradient
    changes by that dy pushed back through features.0 from the new pixel minus from the old one."""
    P = {k: v.double() for k, v in orc.seeded_params(orc.critic_shapes(1), 21).items()}
    rs = np.random.RandomState(3)
    x = rs.randint(0, 256, (2, 64, 64, 3)).astype(np.uint8)
    x[1, 16:32, 16:32] = (200, 40, 90)                               # flat patch: windows 9..14 of image 1 tie four ways
    X = orc.u8_to_nchw(x).double()
    cot = torch.from_numpy(rs.randn(2)).double()
    w0 = P["features.0.weight"]
    pre = F.relu(F.conv2d(X, w0, P["features.0.bias"], padding=1))
    win = pre[1, :, 20:22, 20:22].reshape(8, 4)                      # window (10, 10) of image 1
    assert (win == win[:, :1]).all()
    c0 = int(win[:, 0].argmax())
    assert float(win[c0, 0]) > 0

    def run(pk):
        Pl = orc.leafify(P)
        Xl = X.clone().requires_grad_(True)
        pred, emb = orc.critic_apply(Pl, Xl, collect=True, picks=pk)
        for e in emb:
            e.retain_grad()
        (pred[:, 0] * cot).sum().backward()
        return pred.detach(), emb, Pl, Xl.grad

    base = own_picks(P, X)
    assert int(base[0][1, c0, 10, 10]) == 0                          # max_pool2d's first index
    moved = [t.clone() for t in base]
    moved[0][1, c0, 10, 10] = 3
    p0, e0, P0, gx0 = run(base)
    p1, e1, P1, gx1 = run(moved)
    assert torch.equal(p0, p1)
    for a, b in zip(e0, e1):
        assert torch.equal(a, b) and torch.equal(a.grad, b.grad)
    for k in P:
        if not k.startswith("features.0."):
            assert torch.equal(P0[k].grad, P1[k].grad), k
    g = float(e0[0].grad[1, c0, 10, 10])
    assert g != 0.0
    D = torch.zeros_like(pre)
    D[1, c0, 20, 20], D[1, c0, 21, 21] = -g, g                       # the old pixel (0,0) loses dy, the new one (1,1) gains it
    want = F.conv_transpose2d(D, w0, padding=1)
    torch.testing.assert_close(gx1 - gx0, want, rtol=1e-9, atol=1e-12 * float(gx0.abs().max()))
    assert float((gx1 - gx0)[0].abs().max()) == 0.0                   # the other image is untouched


def test_chunked_phase2_step_equals_the_whole_batch():
    """train_phase2(chunk=k): slices of k images with each slice's loss weighted by its share of the batch -- the whole-batch step
    (float64, ragged last slice, dropout masks and pinned picks sliced along)."""
    n, p = 8, 0.3
    pc, pm, A, B, Y, masks = _problem(1, n, 9, p, dtype=torch.float64)
    picks = _phase2_own_picks(pc, pm, A, B, Y, masks, p)
    batch = [(A, B, Y)]
    whole = orc.train_phase2(pc, pm, batch, steps=1, p=p, training=True, masks=masks, picks=picks)[0]
    part = orc.train_phase2(pc, pm, batch, steps=1, p=p, training=True, masks=masks, picks=picks, chunk=3)[0]
    assert part["total"] == pytest.approx(whole["total"], rel=1e-13)
    for k, v in whole["parts"].items():
        assert part["parts"][k] == pytest.approx(v, rel=1e-13), k
    torch.testing.assert_close(part["Z"], whole["Z"], rtol=1e-13, atol=0)
    torch.testing.assert_close(part["pred"], whole["pred"], rtol=1e-13, atol=0)
    for grp in ("grads_c", "grads_m", "params_c", "params_m"):
        for k, v in whole[grp].items():
            torch.testing.assert_close(part[grp][k], v, rtol=1e-11, atol=1e-14 * float(v.abs().max()), msg=f"{grp} {k}")


def _hand_codes(rs, n, co, hp, wp):
    pick = torch.from_numpy(rs.randint(0, 4, (n, co, hp, wp)))
    dead = torch.from_numpy(rs.rand(n, co, hp, wp) < 0.3)
    dead[0, :, 0, 0] = True                                          # a word whose nibbles are all 0xF (-1 as int32)
    dead[0, :, 0, 1] = False
    return pick, dead


def test_nibble_decoder_round_trips():
    """int32 [n, hp, wp, co/8], channel c at bits 4 (c % 8) of word c // 8, 0xF = dead -- words built by hand (the sign bit included)."""
    rs = np.random.RandomState(1)
    n, co, hp, wp = 3, 16, 4, 5
    pick, dead = _hand_codes(rs, n, co, hp, wp)
    code = np.where(dead.numpy(), 15, pick.numpy()).astype(np.int64)          # [n, co, hp, wp]
    words = np.zeros((n, hp, wp, co // 8), np.int64)
    for c in range(co):
        words[..., c // 8] |= code[:, c] << (4 * (c % 8))
    am = torch.from_numpy(words.astype(np.uint32).view(np.int32))
    assert (am < 0).any()
    got_pick, got_dead = pool_picks.decode_nibbles(am)
    assert torch.equal(got_dead, dead)
    assert torch.equal(got_pick, pick.masked_fill(dead, 0)) and got_pick.dtype == torch.int64
    assert torch.equal(pool_picks.decode(am)[0], got_pick)
    assert int(am[0, 0, 0, 0]) == -1 and int(am[0, 0, 1, 0]) != -1


def test_byte_decoder_round_trips():
    """uint8 [n, hp, wp, co], one pick per byte, any value >= 4 dead (the kernels write 0xFF)."""
    rs = np.random.RandomState(2)
    n, co, hp, wp = 2, 40, 3, 4
    pick, dead = _hand_codes(rs, n, co, hp, wp)
    marker = torch.from_numpy(rs.choice([4, 7, 0xFF], size=dead.shape))
    code = torch.where(dead, marker, pick).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    got_pick, got_dead = pool_picks.decode_bytes(code)
    assert torch.equal(got_dead, dead)
    assert torch.equal(got_pick, pick.masked_fill(dead, 0))
    assert torch.equal(pool_picks.decode(code)[0], got_pick)


def test_oracle_order_and_check_picks_on_the_oracles_own_picks():
    """Slot order [B | A | rep | inj] -> [A, B, rep, inj]; check_picks passes max_pool2d's own picks with no flip and rejects a pick
    moved on a window whose candidates are clearly apart, and one moved off max_pool2d's first index on an exact tie."""
    t = torch.arange(8).reshape(8, 1)
    order = pool_picks.oracle_order([t, t, t, t], 2)
    assert [o[0][:, 0].tolist() for o in order] == [[2, 3], [0, 1], [4, 5], [6, 7]]
    assert len(pool_picks.oracle_order([t[:6]] * 4, 2)) == 3           # no injected pass
    P = orc.seeded_params(orc.critic_shapes(1), 21)
    rs = np.random.RandomState(4)
    x = rs.randint(0, 256, (2, 64, 64, 3)).astype(np.uint8)
    x[1, 16:32, 16:32] = (200, 40, 90)
    X = orc.u8_to_nchw(x)
    picks = own_picks(P, X)
    inputs, dead, h = [torch.from_numpy(x)], [], X
    for i, key in enumerate(orc.ENC_CONV_KEYS):
        y = F.relu(F.conv2d(h, P[key + ".weight"], P[key + ".bias"], padding=1))
        h = F.max_pool2d(y, 2)
        dead.append(h <= 0)
        inputs.append(h.permute(0, 2, 3, 1))
    flips = pool_picks.check_picks(P, inputs[:4], [q.masked_fill(d, 0) for q, d in zip(picks, dead)], dead)
    assert pool_picks.report(flips, "oracle's own picks") <= 2
    pre = F.conv2d(X.double(), P["features.0.weight"].double(), P["features.0.bias"].double(), padding=1)
    top2 = pool_picks._windows(pre).topk(2, dim=-1).values
    clear = ((top2[..., 0] > 0) & (top2[..., 0] - top2[..., 1] > 1e-2 * top2[..., 0])).nonzero()[0].tolist()
    tied = ((top2[..., 0] > 0) & (top2[..., 0] - top2[..., 1] <= pool_picks.TIE * top2[..., 0]) & (picks[0] == 0)).nonzero()[0].tolist()
    assert tied[0] == 1                                               # (in the flat patch of image 1)
    for cell, what in ((clear, "argmax"), (tied, "exactly tied")):
        bad = [q.clone() for q in picks]
        bad[0][tuple(cell)] = (int(picks[0][tuple(cell)]) + 1) % 4
        with pytest.raises(AssertionError, match=what):
            pool_picks.check_picks(P, inputs[:4], bad, dead)
