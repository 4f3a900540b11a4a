"""GPU parity of the HIP kernels (through the C ABI) against the CPU oracle, layer family by layer family.
Tolerance: fp32, 1e-3 relative (BASELINE.json north_star) -- checked as |got-ref| <= 1e-3*|ref| + atol with a
small atol scaled to each tensor's magnitude."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import hourglass_ref as orc
import pool_picks


REL_REPORT = {}       # what -> worst PURE relative error over the elements above 1 % of the tensor's maximum (summary test below)


def rel_close(got, ref, what, rtol=1e-3, atol_scale=2e-5):
    """|got - ref| <= rtol |ref| + atol_scale max|ref| elementwise.  The absolute term only covers values near zero; the worst
    pure-relative error of the elements that carry the tensor (>= 1 % of its maximum) is recorded (for the summary of
    test_zz_rel_summary.py) and shown on failure."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    mx = max(1e-12, float(np.abs(ref).max()))
    atol = atol_scale * mx
    err = np.abs(got - ref)
    big = np.abs(ref) >= 1e-2 * mx
    worst_rel = float((err[big] / np.abs(ref[big])).max()) if big.any() else 0.0
    REL_REPORT[what] = max(REL_REPORT.get(what, 0.0), worst_rel)
    bad = err > (rtol * np.abs(ref) + atol)
    assert not bad.any(), (f"{what}: {bad.sum()}/{bad.size} outside tol; max err {err.max():.3e} "
                           f"(ref max {np.abs(ref).max():.3e}) at {np.unravel_index(err.argmax(), err.shape)}; "
                           f"worst pure-relative error over |ref| >= 1% of max: {worst_rel:.3e}")


def nhwc(t):  # device NHWC tensor -> numpy NCHW
    return t.detach().float().cpu().permute(0, 3, 1, 2).numpy()


@pytest.fixture(scope="module")
def ctx(g1):
    import cgs_amd
    from cgs_amd import hourglass as hg, spec
    dev = torch.device("cuda:0")
    pc, pm = g1
    lc, lm = spec.critic_layout(), spec.masker_layout()
    fc = torch.empty(lc.total, device=dev)
    fm = torch.empty(lm.total, device=dev)
    lc.flatten({k: v.to(dev) for k, v in pc.items()}, fc)
    lm.flatten({k: v.to(dev) for k, v in pm.items()}, fm)
    return dict(hg=hg, spec=spec, dev=dev, pc=pc, pm=pm, lc=lc, lm=lm, fc=fc, fm=fm)


def test_layout_roundtrip(ctx):
    back = ctx["lc"].unflatten(ctx["fc"])
    for k, v in ctx["pc"].items():
        np.testing.assert_array_equal(back[k].cpu().numpy(), v.numpy())
    back = ctx["lm"].unflatten(ctx["fm"])
    for k, v in ctx["pm"].items():
        np.testing.assert_array_equal(back[k].cpu().numpy(), v.numpy())


def tie_frames(n, seed):
    """Frames like real first-person views have: flat patches.  Constant-colour 8x8 blocks (every 2x2 pool window inside a
    block is a 4-way tie of equal conv outputs), images made of rows repeated four times (vertical ties), one flat image."""
    rs = np.random.RandomState(seed)
    blocks = rs.randint(0, 256, (n, 8, 8, 3)).astype(np.uint8)
    x = np.repeat(np.repeat(blocks, 8, axis=1), 8, axis=2)
    rows = rs.randint(0, 256, (n, 16, 64, 3)).astype(np.uint8)
    x[2::3] = np.repeat(rows, 4, axis=1)[2::3]
    x[-1] = 200
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("n,kind", [(8, "noise"), (5, "noise"), (37, "noise"), (13, "ties")])
def test_forward_matches_oracle(ctx, golden, n, kind):
    hg, dev = ctx["hg"], ctx["dev"]
    x_u8 = np.random.RandomState(10 + n).randint(0, 256, (n, 64, 64, 3)).astype(np.uint8) if kind == "noise" else tie_frames(n, 7)
    X = orc.u8_to_nchw(x_u8)
    with torch.no_grad():
        pred, embeds = orc.critic_apply(ctx["pc"], X, collect=True)
        Z, inter = orc.masker_apply(ctx["pm"], X, embeds, return_all=True)
    xd = torch.from_numpy(x_u8).to(dev)
    c = hg.critic_forward(ctx["fc"], ctx["lc"], xd, n)
    m = hg.masker_forward(ctx["fm"], ctx["lm"], xd, [c["e0"], c["e1"], c["e2"], c["e3"], c["e4"]], n)
    torch.cuda.synchronize()
    for i in range(4):
        rel_close(nhwc(c[f"e{i}"]), embeds[i].numpy(), f"e{i}")
    rel_close(c["e4"].cpu().numpy(), embeds[4].flatten(1).numpy(), "e4")
    rel_close(c["pred"].cpu().numpy(), pred[:, 0].numpy(), "pred")
    rel_close(m["o4"].cpu().numpy(), inter["o4"].flatten(1).numpy(), "o4")
    for k in ("o3", "o2", "o1", "o0", "hm"):
        rel_close(nhwc(m[k]), inter[k].numpy(), k)
    rel_close(m["Z"].cpu().numpy(), Z[:, 0].numpy(), "Z")
    # same through the fp32 image path (the replaced / injected passes use it)
    xf = (xd.float() / 255.0).contiguous()
    c2 = hg.critic_forward(ctx["fc"], ctx["lc"], xf, n)
    rel_close(c2["pred"].cpu().numpy(), pred[:, 0].numpy(), "pred(f32 input)")
    rel_close(nhwc(c2["e0"]), embeds[0].numpy(), "e0(f32 input)")


def test_golden_eval_fixture(ctx, golden):
    """The committed reference capture itself (not just the oracle) on the GPU path."""
    hg, dev = ctx["hg"], ctx["dev"]
    g = golden("g2_eval.npz")
    xd = torch.from_numpy(g["X"]).to(dev)
    c = hg.critic_forward(ctx["fc"], ctx["lc"], xd, 8)
    m = hg.masker_forward(ctx["fm"], ctx["lm"], xd, [c[f"e{i}"] for i in range(5)], 8)
    rel_close(c["pred"].cpu().numpy(), g["pred"][:, 0], "pred")
    rel_close(m["Z"].cpu().numpy(), g["Z"][:, 0], "Z")
    for i in range(4):
        rel_close(nhwc(c[f"e{i}"]), g[f"e{i}"], f"e{i}")


def test_pool_argmax_mask(ctx):
    """amask nibble = first maximum of the 2x2 window, 0xF where the pooled value is <= 0."""
    hg, dev = ctx["hg"], ctx["dev"]
    x_u8 = np.random.RandomState(3).randint(0, 256, (3, 64, 64, 3)).astype(np.uint8)
    with torch.no_grad():
        X = orc.u8_to_nchw(x_u8)
        pre = torch.relu(torch.nn.functional.conv2d(X, ctx["pc"]["features.0.weight"], ctx["pc"]["features.0.bias"], padding=1))
        pooled, idx = torch.nn.functional.max_pool2d(pre, 2, return_indices=True)
    c = hg.critic_forward(ctx["fc"], ctx["lc"], torch.from_numpy(x_u8).to(dev), 3)
    am = c["am0"].cpu().numpy().astype(np.uint32)[..., 0]  # [n,32,32]
    yy, xx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    for ch in range(8):
        nib = (am >> (4 * ch)) & 15
        ref_pos = ((idx[:, ch].numpy() // 64) - 2 * yy) * 2 + ((idx[:, ch].numpy() % 64) - 2 * xx)
        dead = pooled[:, ch].numpy() <= 0
        assert (nib[dead] == 15).all()
        # ties between equal positive values are measure-zero for random inputs
        assert (nib[~dead] == ref_pos[~dead]).mean() > 0.9999


def test_pool_argmax_first_index_on_ties(ctx):
    """max_pool2d keeps the FIRST maximum of a window (row-major); on frames with flat patches equal positive conv outputs
    tie constantly.  Every nibble of all four pooling stages must equal the reference index wherever the pooled value is
    positive -- checked where the window's two largest values are exactly equal (a true tie) or clearly apart (positions a
    last-bit rounding difference between the CPU and GPU convolutions cannot reorder)."""
    hg, dev = ctx["hg"], ctx["dev"]
    n = 13
    x_u8 = tie_frames(n, 7)
    F = torch.nn.functional
    c = hg.critic_forward(ctx["fc"], ctx["lc"], torch.from_numpy(x_u8).to(dev), n)
    torch.cuda.synchronize()
    keys = ["features.0", "features.3", "features.6", "features.10"]
    h = orc.u8_to_nchw(x_u8)
    ties_total = 0
    with torch.no_grad():
        for i, key in enumerate(keys):
            pre = torch.relu(F.conv2d(h, ctx["pc"][key + ".weight"], ctx["pc"][key + ".bias"], padding=1))
            pooled, idx = F.max_pool2d(pre, 2, return_indices=True)
            hw = pre.shape[-1]
            win = pre.unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, pre.shape[1], hw // 2, hw // 2, 4)
            top2 = win.topk(2, dim=-1).values
            gap = (top2[..., 0] - top2[..., 1]).numpy()
            exact_tie = gap == 0
            clear = gap > 1e-4 * max(float(pre.max()), 1e-6)
            am = c[f"am{i}"].cpu().numpy().astype(np.uint32)            # [n, hp, wp, co/8]
            yy, xx = np.meshgrid(np.arange(hw // 2), np.arange(hw // 2), indexing="ij")
            for ch in range(pre.shape[1]):
                nib = (am[..., ch // 8] >> (4 * (ch % 8))) & 15
                ii = idx[:, ch].numpy()
                ref_pos = ((ii // hw) - 2 * yy) * 2 + ((ii % hw) - 2 * xx)
                pos = pooled[:, ch].numpy() > 0
                assert (nib[~pos] == 15).all(), f"{key} ch{ch}: dead windows must carry 0xF"
                chk = pos & (exact_tie[:, ch] | clear[:, ch])
                assert (nib[chk] == ref_pos[chk]).all(), f"{key} ch{ch}: argmax differs from max_pool2d's first index"
                ties_total += int((pos & exact_tie[:, ch]).sum())
            h = pooled
    assert ties_total > 5000, f"the tie set exercised only {ties_total} positive ties"


def _oracle_grads(ctx, x_u8, cot_pred, cot_embeds, cot_Z, f32_input=False, picks=None):
    pc = orc.leafify(ctx["pc"])
    pm = orc.leafify(ctx["pm"])
    X = orc.u8_to_nchw(x_u8).requires_grad_(f32_input)
    pred, embeds = orc.critic_apply(pc, X, collect=True, picks=picks)
    Z, inter = orc.masker_apply(pm, X.detach(), embeds, return_all=True)
    loss = (pred[:, 0] * cot_pred).sum() + (Z[:, 0] * cot_Z).sum()
    for e, c in zip(embeds, cot_embeds):
        loss = loss + (e * c).sum()
    loss.backward()
    return pc, pm, X, Z


@pytest.mark.parametrize("n,kind", [(8, "noise"), (21, "noise"), (13, "ties")])
def test_backward_matches_oracle_autograd(ctx, n, kind):
    """critic + masker backward with random cotangents on every output, vs torch autograd on the oracle, every image.
    kind = ties: flat-patch frames, where the pooling gradient must follow max_pool2d's first-index rule.
    The oracle follows the kernels' 2x2 max-pool picks (the argmax nibbles critic_forward writes for all four stages): where a window's
    two largest values are a near-tie fp32 and float64 may pick different pixels; check_picks asserts that this is the only way the
    picks differ (an exact tie must take max_pool2d's first index) and the count stays small."""
    hg, dev, lc, lm = ctx["hg"], ctx["dev"], ctx["lc"], ctx["lm"]
    rs = np.random.RandomState(n)
    x_u8 = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8) if kind == "noise" else tie_frames(n, 7)
    cot_pred = torch.from_numpy(rs.randn(n).astype(np.float32))
    cot_Z = torch.from_numpy(rs.randn(n, 64, 64).astype(np.float32) * 0.1)
    shapes = [(n, 8, 32, 32), (n, 8, 16, 16), (n, 8, 8, 8), (n, 16, 4, 4), (n, 32, 1, 1)]
    cot_e = [torch.from_numpy(rs.randn(*s).astype(np.float32) * 0.05) for s in shapes]

    xd = torch.from_numpy(x_u8).to(dev)
    xf = (xd.float() / 255.0).contiguous()   # fp32 image path so that the image gradient can be checked too
    c = hg.critic_forward(ctx["fc"], lc, xf, n)
    picks, dead = pool_picks.buffer_picks(c, n)
    flips = pool_picks.check_picks(ctx["pc"], [xf, c["e0"], c["e1"], c["e2"]], picks, dead, what=f"{kind} n={n}")
    nflip = pool_picks.report(flips, f"critic_forward {kind} n={n}")
    assert nflip <= max(1, n // 10), f"pool picks differ from float64 on {nflip} near-tied cells: {flips}"
    pc, pm, X, Z = _oracle_grads(ctx, x_u8, cot_pred, cot_e, cot_Z, f32_input=True, picks=picks)
    embeds = [c[f"e{i}"] for i in range(5)]
    m = hg.masker_forward(ctx["fm"], lm, xf, embeds, n)
    Zd = m["Z"]
    dzpre = (cot_Z.to(dev) * Zd * (1 - Zd)).contiguous()
    plan_m = hg.SlabPlan()
    d_emb = hg.masker_backward(ctx["fm"], lm, xf, embeds, n, m, dzpre, plan_m)
    gm = torch.zeros(lm.total, device=dev)
    plan_m.build(gm).run()
    # the cotangents on the embeds join the decoder's skip gradients
    for i in range(4):
        d_emb[i] += cot_e[i].to(dev).permute(0, 2, 3, 1).contiguous()
    d_emb[4] += cot_e[4].to(dev).flatten(1)
    plan_c = hg.SlabPlan()
    dx = torch.empty((n, 64, 64, 3), device=dev)
    hg.critic_backward(ctx["fc"], lc, xf, n, c, cot_pred.to(dev), plan_c, d_embeds=d_emb, n_add=n, dx=dx, dx_from=0)
    gc = torch.zeros(lc.total, device=dev)
    plan_c.build(gc).run()
    torch.cuda.synchronize()
    for k, v in lm.unflatten(gm).items():
        rel_close(v.cpu().numpy(), pm[k].grad.numpy(), f"masker grad {k}")
    for k, v in lc.unflatten(gc).items():
        rel_close(v.cpu().numpy(), pc[k].grad.numpy(), f"critic grad {k}")
    rel_close(nhwc(dx), X.grad.numpy(), "image gradient")


def test_u8_and_f32_wgrad_agree(ctx):
    """The uint8 loader (A images) and the fp32 loader (mixes) feed the same arithmetic."""
    hg, dev, lc = ctx["hg"], ctx["dev"], ctx["lc"]
    n = 6
    rs = np.random.RandomState(5)
    xd = torch.from_numpy(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)).to(dev)
    xf = (xd.float() / 255.0).contiguous()
    dp = torch.from_numpy(rs.randn(n).astype(np.float32)).to(dev)
    outs = []
    for x in (xd, xf):
        c = hg.critic_forward(ctx["fc"], lc, x, n)
        plan = hg.SlabPlan()
        hg.critic_backward(ctx["fc"], lc, x, n, c, dp, plan)
        g = torch.zeros(lc.total, device=dev)
        plan.build(g).run()
        outs.append(g.cpu().numpy())
    rel_close(outs[0], outs[1], "u8 vs f32 critic grads", rtol=1e-4)


def test_dropout_masks_statistics_and_step(ctx):
    from cgs_amd import _lib
    import ctypes as C
    dev = ctx["dev"]
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty(1 << 20, device=dev)
    masks = []
    for s in (0, 1):
        step.fill_(s)
        d = _lib.Dropout(0.3, 1, 1234, step.data_ptr())
        _lib.call("cgs_dropout_mask", d, out.numel(), C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        masks.append(out.cpu().numpy().copy())
    keep = masks[0] != 0
    assert abs(keep.mean() - 0.7) < 3e-3
    np.testing.assert_allclose(masks[0][keep], 1 / 0.7, rtol=1e-6)
    assert (masks[0] != masks[1]).mean() > 0.3          # a new step draws a new mask
    # lag-1 independence
    assert abs(np.corrcoef(keep[:-1], keep[1:])[0, 1]) < 5e-3


def test_forward_backward_with_dropout_vs_oracle_masks(ctx):
    """Train-mode dropout (p=0.3): export the Philox keep-masks the kernels used and feed the SAME masks to
    the oracle; forward values and every gradient must agree."""
    from cgs_amd import _lib
    import ctypes as C
    hg, dev, lc = ctx["hg"], ctx["dev"], ctx["lc"]
    n, p = 9, 0.3
    rs = np.random.RandomState(77)
    x_u8 = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    step = torch.full((1,), 5, dtype=torch.int64, device=dev)
    drop = hg.DropState(p, 99, step)
    xd = torch.from_numpy(x_u8).to(dev)
    c = hg.critic_forward(ctx["fc"], lc, xd, n, drop)
    dp = torch.from_numpy(rs.randn(n).astype(np.float32))
    plan = hg.SlabPlan()
    hg.critic_backward(ctx["fc"], lc, xd, n, c, dp.to(dev), plan, drop)
    g = torch.zeros(lc.total, device=dev)
    plan.build(g).run()
    masks = []
    for site, shape in ((0, (n, 8, 8, 8)), (1, (n, 4, 4, 16)), (2, (n, 32))):
        out = torch.empty(int(np.prod(shape)), device=dev)
        _lib.call("cgs_dropout_mask", drop.desc(site), out.numel(), C.c_void_p(out.data_ptr()),
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        mk = (out.cpu().reshape(shape) != 0).float()
        masks.append(mk.permute(0, 3, 1, 2).contiguous() if len(shape) == 4 else mk)
    pc = orc.leafify(ctx["pc"])
    pred = orc.critic_apply(pc, orc.u8_to_nchw(x_u8), p=p, training=True, masks=masks)
    (pred[:, 0] * dp).sum().backward()
    rel_close(c["pred"].cpu().numpy(), pred[:, 0].detach().numpy(), "pred with dropout")
    for k, v in lc.unflatten(g).items():
        rel_close(v.cpu().numpy(), pc[k].grad.numpy(), f"critic grad {k} (dropout)")


@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_ragged_batches_forward_backward(ctx, n):
    """Batch sizes that do not fill a workgroup's image group (padding lanes, partial tiles)."""
    hg, dev, lc, lm = ctx["hg"], ctx["dev"], ctx["lc"], ctx["lm"]
    rs = np.random.RandomState(100 + n)
    x_u8 = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    cot_pred = torch.from_numpy(rs.randn(n).astype(np.float32))
    cot_Z = torch.from_numpy(rs.randn(n, 64, 64).astype(np.float32) * 0.1)
    zeros = [torch.zeros(s) for s in [(n, 8, 32, 32), (n, 8, 16, 16), (n, 8, 8, 8), (n, 16, 4, 4), (n, 32, 1, 1)]]
    pc, pm, X, Z = _oracle_grads(ctx, x_u8, cot_pred, zeros, cot_Z)
    xd = torch.from_numpy(x_u8).to(dev)
    c = hg.critic_forward(ctx["fc"], lc, xd, n)
    embeds = [c[f"e{i}"] for i in range(5)]
    m = hg.masker_forward(ctx["fm"], lm, xd, embeds, n)
    rel_close(m["Z"].cpu().numpy(), Z[:, 0].detach().numpy(), "Z")
    dzpre = (cot_Z.to(dev) * m["Z"] * (1 - m["Z"])).contiguous()
    plan_m, plan_c = hg.SlabPlan(), hg.SlabPlan()
    d_emb = hg.masker_backward(ctx["fm"], lm, xd, embeds, n, m, dzpre, plan_m)
    hg.critic_backward(ctx["fc"], lc, xd, n, c, cot_pred.to(dev), plan_c, d_embeds=d_emb, n_add=n)
    gm, gc = torch.zeros(lm.total, device=dev), torch.zeros(lc.total, device=dev)
    plan_m.build(gm).run()
    plan_c.build(gc).run()
    for k, v in lm.unflatten(gm).items():
        rel_close(v.cpu().numpy(), pm[k].grad.numpy(), f"masker grad {k} (n={n})")
    for k, v in lc.unflatten(gc).items():
        rel_close(v.cpu().numpy(), pc[k].grad.numpy(), f"critic grad {k} (n={n})")


def test_empty_batch_and_bad_arguments(ctx):
    """n = 0 is a no-op; unsupported shapes and null pointers are reported through the return code."""
    from cgs_amd import _lib
    import ctypes as C
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(64, device=ctx["dev"])
    p = C.c_void_p(buf.data_ptr())
    d0 = _lib.ConvDesc(0, 64, 64, 3, 0, 8, _lib.SRC_U8, 2, _lib.ACT_RELU, 1, _lib.Dropout())
    assert lib.cgs_conv3x3_fwd(C.byref(d0), p, None, p, p, p, None, st) == _lib.OK
    assert lib.cgs_head_fwd(0, p, p, p, p, p, p, p, _lib.Dropout(), _lib.Dropout(), p, p, p, None, None, None, st) == _lib.OK
    bad = _lib.ConvDesc(4, 48, 48, 3, 0, 8, _lib.SRC_U8, 2, _lib.ACT_RELU, 1, _lib.Dropout())
    assert lib.cgs_conv3x3_fwd(C.byref(bad), p, None, p, p, p, None, st) == _lib.ERR_UNSUPPORTED
    ok = _lib.ConvDesc(4, 64, 64, 3, 0, 8, _lib.SRC_U8, 2, _lib.ACT_RELU, 1, _lib.Dropout())
    assert lib.cgs_conv3x3_fwd(C.byref(ok), None, None, p, p, p, None, st) == _lib.ERR_BADARG
    assert lib.cgs_conv3x3_bwd_data(C.byref(ok), p, None, p, None, 0, None, 0, p, None, st) == _lib.ERR_BADARG  # pool needs amask
    assert lib.cgs_pointwise_fwd(4, 16, 32, p, p, p, p, st) == _lib.ERR_UNSUPPORTED
    assert lib.cgs_mix_fwd(1, 4095, p, p, p, 1, p, p, st) == _lib.ERR_BADARG
    with pytest.raises(_lib.CgsError, match="CGS_ERR_UNSUPPORTED"):
        _lib.call("cgs_conv3x3_fwd", C.byref(bad), p, None, p, p, p, None, st)
    torch.cuda.synchronize()


def test_shared_launch_backward_equals_separate_launches(ctx):
    """cgs_conv3x3_bwd_both runs the same device code as bwd_weight + bwd_data: identical bits."""
    from cgs_amd import _lib
    import ctypes as C
    hg, dev, lc = ctx["hg"], ctx["dev"], ctx["lc"]
    lib = _lib.load()
    n = 24
    rs = np.random.RandomState(8)
    e0 = torch.from_numpy(rs.rand(n, 32, 32, 8).astype(np.float32)).to(dev)
    de1 = torch.from_numpy(rs.randn(n, 16, 16, 8).astype(np.float32)).to(dev)
    am = torch.from_numpy(rs.randint(0, 2 ** 31, (n, 16, 16, 1)).astype(np.int32)).to(dev)   # arbitrary nibbles (incl. invalid ones)
    w = C.c_void_p(ctx["fc"].data_ptr() + 4 * lc.off("features.3.weight"))
    d = hg.conv_desc(n, 32, 8, 0, 8, False, 2, "relu", 1, _lib.Dropout())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    ns1 = lib.cgs_conv3x3_bwd_weight_slabs(C.byref(d))
    s1 = torch.zeros(ns1, 584, device=dev); dx1 = torch.empty(n, 32, 32, 8, device=dev)
    _lib.call("cgs_conv3x3_bwd_weight", C.byref(d), P(e0), None, P(de1), P(am), P(s1), st)
    _lib.call("cgs_conv3x3_bwd_data", C.byref(d), P(de1), P(am), w, None, _lib.ACT_NONE, None, 0, P(dx1), None, st)
    ns2 = lib.cgs_conv3x3_bwd_both_slabs(C.byref(d))
    s2 = torch.zeros(ns2, 584, device=dev); dx2 = torch.empty_like(dx1)
    _lib.call("cgs_conv3x3_bwd_both", C.byref(d), P(e0), None, P(de1), P(am), w, None, 0, P(dx2), None, P(s2), st)
    torch.cuda.synchronize()
    assert torch.equal(dx1, dx2)
    np.testing.assert_allclose(s1.sum(0).cpu().numpy(), s2.sum(0).cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("n,u8", [(3, False), (16, True), (130, False)])
def test_mask_head_backward_vs_torch_fp32(ctx, n, u8):
    """cgs_mask_head_bwd (masker.2 dgrad rebuilt on the fly, upsample folded into the masker.0 weights, MFMA; masker.2 and
    masker.0 weight gradients riding along) against a plain torch autograd (fp64) of nets.py:488-491 on the same tensors."""
    from cgs_amd import _lib
    import ctypes as C
    import torch.nn.functional as F
    dev, lm, pm = ctx["dev"], ctx["lm"], ctx["pm"]
    lib = _lib.load()
    rs = np.random.RandomState(40 + n)
    img_u8 = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    img = img_u8.astype(np.float32) / np.float32(255.0) if u8 else rs.rand(n, 64, 64, 3).astype(np.float32)
    o0 = rs.randn(n, 8, 32, 32).astype(np.float32)
    dz = (rs.randn(n, 64, 64) * 1e-3).astype(np.float32)
    w0t = pm["masker.0.weight"].double().requires_grad_(True); b0t = pm["masker.0.bias"].double().requires_grad_(True)
    w2t = pm["masker.2.weight"].double().requires_grad_(True); b2t = pm["masker.2.bias"].double().requires_grad_(True)
    o0t = torch.from_numpy(o0).double().requires_grad_(True)
    cat = torch.cat([torch.from_numpy(img).double().permute(0, 3, 1, 2), F.interpolate(o0t, scale_factor=2, mode="nearest")], 1)
    hpre = F.conv2d(cat, w0t, b0t, padding=1)
    hpre.retain_grad()                    # the kernel's d_h is the gradient w.r.t. the masker.0 conv output (pre-LeakyReLU)
    h = F.leaky_relu(hpre, 0.01)
    zpre = F.conv2d(h, w2t, b2t, padding=1)
    zpre.backward(torch.from_numpy(dz).double()[:, None])

    hd = h.detach().float().permute(0, 2, 3, 1).contiguous().to(dev)
    xd = torch.from_numpy(img_u8 if u8 else img).to(dev)
    o0d = torch.from_numpy(o0).permute(0, 2, 3, 1).contiguous().to(dev)
    dzd = torch.from_numpy(dz).to(dev)
    nan = float("nan")
    dh = torch.full((n, 64, 64, 16), nan, device=dev)
    do0 = torch.full((n, 32, 32, 8), nan, device=dev)
    nsl = lib.cgs_mask_head_bwd_slabs(n)
    assert nsl > 0
    slab2 = torch.full((nsl, 145), nan, device=dev)
    slab0 = torch.full((nsl, 1600), nan, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    fm = ctx["fm"]
    w2p = C.c_void_p(fm.data_ptr() + 4 * lm.off("masker.2.weight"))
    w0p = C.c_void_p(fm.data_ptr() + 4 * lm.off("masker.0.weight"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kind = _lib.SRC_U8 if u8 else _lib.SRC_F32
    _lib.call("cgs_mask_head_bwd", n, kind, P(xd), P(o0d), P(dzd), P(hd), w2p, w0p, P(dh), P(do0), P(slab2), P(slab0), st)
    torch.cuda.synchronize()
    rel_close(nhwc(dh), hpre.grad.numpy(), "d h")
    rel_close(nhwc(do0), o0t.grad.numpy(), "d o0", atol_scale=5e-5)
    g = slab2.sum(0).cpu().numpy()
    rel_close(g[:144].reshape(3, 3, 16), w2t.grad[0].permute(1, 2, 0).numpy(), "d masker.2.weight", atol_scale=1e-4)
    rel_close(g[144:], b2t.grad.numpy(), "d masker.2.bias", atol_scale=1e-4)
    g = slab0.sum(0).cpu().numpy()
    rel_close(g[:1584].reshape(3, 3, 11, 16), w0t.grad.permute(2, 3, 1, 0).numpy(), "d masker.0.weight", atol_scale=1e-4)
    rel_close(g[1584:], b0t.grad.numpy(), "d masker.0.bias", atol_scale=1e-4)
    # every subset of the optional outputs gives the same bits for what it does produce
    do0b = torch.empty_like(do0); s2b = torch.empty_like(slab2)
    _lib.call("cgs_mask_head_bwd", n, kind, None, None, P(dzd), P(hd), w2p, w0p, None, P(do0b), P(s2b), None, st)
    dhc, do0c = torch.empty_like(dh), torch.empty_like(do0)
    _lib.call("cgs_mask_head_bwd", n, 0, None, None, P(dzd), P(hd), w2p, w0p, P(dhc), P(do0c), None, None, st)
    torch.cuda.synchronize()
    assert torch.equal(do0, do0b) and torch.equal(do0, do0c) and torch.equal(dh, dhc) and torch.equal(slab2, s2b)
    # argument errors are return codes, not faults
    assert lib.cgs_mask_head_bwd(n, kind, None, None, P(dzd), P(hd), w2p, w0p, None, P(do0), P(slab2), P(slab0), st) < 0
    assert lib.cgs_mask_head_bwd(n, 7, P(xd), P(o0d), P(dzd), P(hd), w2p, w0p, None, P(do0), P(slab2), P(slab0), st) < 0


def test_bottleneck_conv_inside_head_kernels_equals_standalone(ctx):
    """cgs_head_fwd(..., w_pw, b_pw, o4) == cgs_pointwise_fwd on its e4, and cgs_head_bwd(..., d_o4, w_pw, slab_pw) ==
    cgs_pointwise_bwd followed by cgs_head_bwd(d_e4_extra = its dx): same d_e3, same head slab, same dec_model.4 gradient."""
    from cgs_amd import _lib
    from cgs_amd.hourglass import HEAD_SLAB, PW_SLAB
    import ctypes as C
    dev, lc, lm, fc, fm = ctx["dev"], ctx["lc"], ctx["lm"], ctx["fc"], ctx["fm"]
    lib = _lib.load()
    n, n_extra = 21, 13
    rs = np.random.RandomState(77)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(dev)
    e3 = T(np.maximum(rs.randn(n, 4, 4, 16), 0))
    P = lambda t: C.c_void_p(t.data_ptr())
    wc = lambda k: C.c_void_p(fc.data_ptr() + 4 * lc.off(k))
    wm = lambda k: C.c_void_p(fm.data_ptr() + 4 * lm.off(k))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nd = _lib.Dropout()
    mk = lambda *s: torch.full(s, float("nan"), device=dev)
    e4, h1, pred, o4 = mk(n, 32), mk(n, 32), mk(n), mk(n, 32)
    _lib.call("cgs_head_fwd", n, P(e3), wc("features.14.weight"), wc("features.14.bias"), wc("crit.1.weight"), wc("crit.1.bias"),
              wc("crit.4.weight"), wc("crit.4.bias"), nd, nd, P(e4), P(h1), P(pred), wm("dec_model.4.weight"),
              wm("dec_model.4.bias"), P(o4), st)
    o4_ref = mk(n, 32)
    _lib.call("cgs_pointwise_fwd", n, 32, 32, P(e4), wm("dec_model.4.weight"), wm("dec_model.4.bias"), P(o4_ref), st)
    torch.cuda.synchronize()
    np.testing.assert_allclose(o4.cpu().numpy(), o4_ref.cpu().numpy(), rtol=1e-5, atol=1e-6)
    # backward
    dpred = T(rs.randn(n) * 0.1)
    d_o4 = T(rs.randn(n_extra, 32) * 0.1)
    d_e3x = T(rs.randn(n_extra, 4, 4, 16) * 0.1)
    nsl = lib.cgs_head_bwd_slabs(n)
    # (a) stand-alone 1x1 backward, then the head with d_e4_extra
    nsp = lib.cgs_pointwise_bwd_slabs(n_extra)
    dx, slab_pw_a = mk(n_extra, 32), mk(nsp, PW_SLAB)
    _lib.call("cgs_pointwise_bwd", n_extra, 32, 32, P(e4), P(d_o4), wm("dec_model.4.weight"), P(dx), P(slab_pw_a), st)
    de3_a, slab_a = mk(n, 4, 4, 16), mk(nsl, HEAD_SLAB)
    _lib.call("cgs_head_bwd", n, P(e3), P(e4), P(h1), P(pred), P(dpred), P(dx), P(d_e3x), n_extra, wc("features.14.weight"),
              wc("crit.1.weight"), wc("crit.4.weight"), nd, nd, P(de3_a), P(slab_a), None, None, None, st)
    # (b) everything in the head kernel
    de3_b, slab_b, slab_pw_b = mk(n, 4, 4, 16), mk(nsl, HEAD_SLAB), mk(nsl, PW_SLAB)
    _lib.call("cgs_head_bwd", n, P(e3), P(e4), P(h1), P(pred), P(dpred), None, P(d_e3x), n_extra, wc("features.14.weight"),
              wc("crit.1.weight"), wc("crit.4.weight"), nd, nd, P(de3_b), P(slab_b), P(d_o4), wm("dec_model.4.weight"),
              P(slab_pw_b), st)
    torch.cuda.synchronize()
    rel_close(de3_b.cpu().numpy(), de3_a.cpu().numpy(), "d e3", rtol=1e-4)
    rel_close(slab_b.sum(0).cpu().numpy(), slab_a.sum(0).cpu().numpy(), "head slab", rtol=1e-4)
    rel_close(slab_pw_b.sum(0).cpu().numpy(), slab_pw_a.sum(0).cpu().numpy(), "dec_model.4 slab", rtol=1e-4)
    # argument errors are return codes
    assert lib.cgs_head_bwd(n, P(e3), P(e4), P(h1), P(pred), P(dpred), None, None, 0, wc("features.14.weight"), wc("crit.1.weight"),
                            wc("crit.4.weight"), nd, nd, P(de3_b), P(slab_b), P(d_o4), None, None, st) < 0


@pytest.mark.parametrize("n,u8", [(5, True), (37, False)])
def test_fused_inference_mask_head_matches_oracle_and_two_kernel_form(ctx, n, u8):
    """cgs_mask_infer_fwd (masker.0 into an LDS tile + masker.2 + sigmoid, the 16-channel intermediate never stored) vs the
    oracle's masker and vs the two cgs_conv3x3_fwd launches of the training path."""
    from cgs_amd import _lib
    import ctypes as C
    hg, dev, lm, fm = ctx["hg"], ctx["dev"], ctx["lm"], ctx["fm"]
    lib = _lib.load()
    x_u8 = np.random.RandomState(60 + n).randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    X = orc.u8_to_nchw(x_u8)
    with torch.no_grad():
        _, embeds = orc.critic_apply(ctx["pc"], X, collect=True)
        Z = orc.masker_apply(ctx["pm"], X, embeds)
    xd = torch.from_numpy(x_u8).to(dev)
    xin = xd if u8 else (xd.float() / 255.0).contiguous()
    c = hg.critic_forward(ctx["fc"], ctx["lc"], xin, n)
    emb = [c[f"e{i}"] for i in range(5)]
    m2 = hg.masker_forward(fm, lm, xin, emb, n)                       # two-kernel form (keeps hm)
    m1 = hg.masker_forward(fm, lm, xin, emb, n, keep_hm=False)        # one kernel
    torch.cuda.synchronize()
    assert "hm" not in m1 and "hm" in m2
    rel_close(m1["Z"].cpu().numpy(), Z[:, 0].numpy(), "Z (fused inference)")
    np.testing.assert_allclose(m1["Z"].cpu().numpy(), m2["Z"].cpu().numpy(), rtol=2e-5, atol=2e-6)
    # round 5: the one-kernel form IS the training forward's kernel storing nothing but Z -- bit-identical to cgs_mask_train_fwd's Z; the earlier
    # tile kernel (cgs_mask_infer_fwd_tile) computes the same mask in another summation order
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    off = lambda k: C.c_void_p(fm.data_ptr() + 4 * lm.off(k))
    wargs = (off("masker.0.weight"), off("masker.0.bias"), off("masker.2.weight"), off("masker.2.bias"))
    src = _lib.SRC_U8 if u8 else _lib.SRC_F32
    h_t = torch.empty((n, 64, 64, 16), device=dev); z_t = torch.empty((n, 64, 64), device=dev); zp = torch.empty(2 * n, device=dev)
    assert lib.cgs_mask_train_fwd(n, src, P(xin), P(m2["o0"]), *wargs, P(h_t), P(z_t), P(zp), st) == 0
    z_tile = torch.empty((n, 64, 64), device=dev)
    assert lib.cgs_mask_infer_fwd_tile(n, src, P(xin), P(m2["o0"]), *wargs, P(z_tile), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(m1["Z"], z_t)
    np.testing.assert_allclose(z_tile.cpu().numpy(), m1["Z"].cpu().numpy(), rtol=2e-5, atol=2e-6)
    rel_close(z_tile.cpu().numpy(), Z[:, 0].numpy(), "Z (tile kernel)")
    p = C.c_void_p(xin.data_ptr())
    assert lib.cgs_mask_infer_fwd(n, 7, p, p, p, p, p, p, p, st) < 0
    assert lib.cgs_mask_infer_fwd_tile(n, 7, p, p, p, p, p, p, p, st) < 0


def test_fp16_operand_inference_mask_head_within_1e3_abs(ctx):
    """BASELINE config 4: the opt-in fp16-operand masker.0 GEMM (fp32 accumulate, fp32 masker.2).  Tolerance is the one
    SURVEY 8d states for fp16 inference: ~1e-3 ABSOLUTE in Z against the fp32 oracle (checked: max 2e-3, mean 3e-4)."""
    hg, dev, lm, fm = ctx["hg"], ctx["dev"], ctx["lm"], ctx["fm"]
    n = 33
    x_u8 = np.random.RandomState(71).randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    X = orc.u8_to_nchw(x_u8)
    with torch.no_grad():
        _, embeds = orc.critic_apply(ctx["pc"], X, collect=True)
        Z = orc.masker_apply(ctx["pm"], X, embeds)[:, 0].numpy()
    for u8 in (True, False):
        xd = torch.from_numpy(x_u8).to(dev)
        xin = xd if u8 else (xd.float() / 255.0).contiguous()
        c = hg.critic_forward(ctx["fc"], ctx["lc"], xin, n)
        m = hg.masker_forward(fm, lm, xin, [c[f"e{i}"] for i in range(5)], n, keep_hm=False, fp16_mask_head=True)
        torch.cuda.synchronize()
        err = np.abs(m["Z"].cpu().numpy() - Z)
        assert err.max() <= 2e-3 and err.mean() <= 3e-4, (err.max(), err.mean())
    with pytest.raises(Exception):
        hg.masker_forward(fm, lm, xin, [c[f"e{i}"] for i in range(5)], n, keep_hm=True, fp16_mask_head=True)


@pytest.mark.parametrize("inject,wgrad", [(True, True), (False, True), (True, False)])
def test_enc0_backward_with_mix_backward_equals_two_launches(ctx, inject, wgrad):
    """cgs_enc0_bwd_mix == cgs_conv3x3_bwd_both (features.0 on the fp32 mixes) followed by cgs_mix_bwd: identical dzpre bits
    and identical weight-gradient slabs; the image gradients are never stored."""
    from cgs_amd import _lib
    import ctypes as C
    hg, dev, lc, fc = ctx["hg"], ctx["dev"], ctx["lc"], ctx["fc"]
    lib = _lib.load()
    n_a = 11
    n_mix = 2 * n_a if inject else n_a
    rs = np.random.RandomState(5 + inject + 2 * wgrad)
    A = torch.from_numpy(rs.randint(0, 256, (n_a, 64, 64, 3)).astype(np.uint8)).to(dev)
    B = torch.from_numpy(rs.randint(0, 256, (n_a, 64, 64, 3)).astype(np.uint8)).to(dev)
    Z = torch.from_numpy(rs.rand(n_a, 64, 64).astype(np.float32)).to(dev)
    mixed = torch.from_numpy(rs.rand(n_mix, 64, 64, 3).astype(np.float32)).to(dev)
    dy = torch.from_numpy(rs.randn(n_mix, 32, 32, 8).astype(np.float32)).to(dev)
    am = torch.from_numpy(rs.randint(0, 2 ** 31, (n_mix, 32, 32, 1)).astype(np.int32)).to(dev)
    w = C.c_void_p(fc.data_ptr() + 4 * lc.off("features.0.weight"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    l1s, l2s = 0.5 / (n_a * 4096), 0.1 / (n_a * 4096)
    d = hg.conv_desc(n_mix, 64, 3, 0, 8, False, 2, "relu", 1, _lib.Dropout())
    # reference: two launches
    dmix = torch.empty(n_mix, 64, 64, 3, device=dev)
    if wgrad:
        ns = lib.cgs_conv3x3_bwd_both_slabs(C.byref(d))
        s_ref = torch.zeros(ns, 224, device=dev)
        _lib.call("cgs_conv3x3_bwd_both", C.byref(d), P(mixed), None, P(dy), P(am), w, None, 0, P(dmix), None, P(s_ref), st)
    else:
        _lib.call("cgs_conv3x3_bwd_data", C.byref(d), P(dy), P(am), w, None, _lib.ACT_NONE, None, 0, P(dmix), None, st)
    dz_ref = torch.empty(n_a, 64, 64, device=dev)
    _lib.call("cgs_mix_bwd", n_a, 4096, P(A), P(B), P(Z), P(dmix), int(inject), l1s, l2s, P(dz_ref), st)
    # one launch
    dz = torch.full((n_a, 64, 64), float("nan"), device=dev)
    slab = None
    if wgrad:
        assert lib.cgs_enc0_bwd_mix_slabs(n_mix) == ns
        slab = torch.zeros(ns, 224, device=dev)
    _lib.call("cgs_enc0_bwd_mix", n_a, int(inject), P(mixed) if wgrad else None, P(dy), P(am), w, P(A), P(B), P(Z), l1s, l2s, None,
              P(dz), P(slab), st)
    torch.cuda.synchronize()
    # one data-gradient pass over the DIFFERENCE tile (conv_bwd_both.hip DEnc0D): same sums in another order
    scale = float(dz_ref.abs().max()) + 1e-30
    assert float((dz - dz_ref).abs().max()) <= 2e-5 * scale, float((dz - dz_ref).abs().max()) / scale
    if wgrad:
        assert torch.equal(slab, s_ref)
    assert lib.cgs_enc0_bwd_mix(n_a, 1, P(mixed), P(dy), P(am), w, P(A), P(B), P(Z), l1s, l2s, None, P(dz), None, st) < 0


def test_virtual_mixes_equal_materialised_mixes(ctx):
    """CGS_SRC_MIX: features.0 forward (and its weight gradient inside cgs_enc0_bwd_mix with mixed=NULL) on the mixes computed
    in the tile loader == the same kernels on the output of cgs_mix_fwd; the mask layer's z partial sums == cgs_mix_fwd's."""
    from cgs_amd import _lib
    import ctypes as C
    hg, dev, lc, fc = ctx["hg"], ctx["dev"], ctx["lc"], ctx["fc"]
    lib = _lib.load()
    n_a = 9
    rs = np.random.RandomState(123)
    A = torch.from_numpy(rs.randint(0, 256, (n_a, 64, 64, 3)).astype(np.uint8)).to(dev)
    B = torch.from_numpy(rs.randint(0, 256, (n_a, 64, 64, 3)).astype(np.uint8)).to(dev)
    Z = torch.from_numpy(rs.rand(n_a, 64, 64).astype(np.float32)).to(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    mixed = torch.empty(2 * n_a, 64, 64, 3, device=dev)
    zp = torch.empty(2 * lib.cgs_mix_fwd_partials(n_a, 4096), device=dev)
    _lib.call("cgs_mix_fwd", n_a, 4096, P(A), P(B), P(Z), 1, P(mixed), P(zp), st)
    # forward
    c_ref = hg.critic_forward(fc, lc, mixed, 2 * n_a)
    c_vir = hg.critic_forward(fc, lc, hg.MixInput(A, B, Z), 2 * n_a)
    torch.cuda.synchronize()
    np.testing.assert_allclose(c_vir["e0"].cpu().numpy(), c_ref["e0"].cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(c_vir["pred"].cpu().numpy(), c_ref["pred"].cpu().numpy(), rtol=1e-5, atol=1e-7)
    # weight gradient inside the fused backward
    dy = torch.from_numpy(rs.randn(2 * n_a, 32, 32, 8).astype(np.float32)).to(dev)
    am = c_ref["am0"]
    w = C.c_void_p(fc.data_ptr() + 4 * lc.off("features.0.weight"))
    ns = lib.cgs_enc0_bwd_mix_slabs(2 * n_a)
    s_ref, s_vir = torch.zeros(ns, 224, device=dev), torch.zeros(ns, 224, device=dev)
    dz_ref, dz_vir = torch.empty(n_a, 64, 64, device=dev), torch.empty(n_a, 64, 64, device=dev)
    _lib.call("cgs_enc0_bwd_mix", n_a, 1, P(mixed), P(dy), P(am), w, P(A), P(B), P(Z), 1e-6, 0.0, None, P(dz_ref), P(s_ref), st)
    _lib.call("cgs_enc0_bwd_mix", n_a, 1, None, P(dy), P(am), w, P(A), P(B), P(Z), 1e-6, 0.0, None, P(dz_vir), P(s_vir), st)
    torch.cuda.synchronize()
    assert torch.equal(dz_ref, dz_vir)
    rel_close(s_vir.sum(0).cpu().numpy(), s_ref.sum(0).cpu().numpy(), "features.0 weight gradient on virtual mixes", rtol=1e-4)
    # z partial sums out of the mask layer
    h = torch.from_numpy(rs.randn(n_a, 64, 64, 16).astype(np.float32)).to(dev)
    lm, fm = ctx["lm"], ctx["fm"]
    d = hg.conv_desc(n_a, 64, 16, 0, 1, False, 2, "sigmoid", 0, _lib.Dropout())
    zout, zpart = torch.empty(n_a, 64, 64, device=dev), torch.full((4 * n_a, 2), float("nan"), device=dev)
    _lib.call("cgs_conv3x3_fwd", C.byref(d), P(h), None, C.c_void_p(fm.data_ptr() + 4 * lm.off("masker.2.weight")),
              C.c_void_p(fm.data_ptr() + 4 * lm.off("masker.2.bias")), P(zout), P(zpart), st)
    torch.cuda.synchronize()
    zz = zout.double()
    np.testing.assert_allclose(zpart[:, 0].double().sum().item(), zz.abs().sum().item(), rtol=1e-5)
    np.testing.assert_allclose(zpart[:, 1].double().sum().item(), (zz * zz).sum().item(), rtol=1e-5)


def rel_kind(what):
    """Category of a comparison by its label: parameters after optimiser steps (Adam divides by sqrt(v): a gradient error near a
    zero gradient is amplified), gradients, or forward tensors."""
    w = what.lower()
    if " after " in w or "parameters" in w or w.endswith(" flat") or w.endswith(" m") or w.endswith(" v"):
        return "param"
    if "grad" in w or w.startswith("d") or "slab" in w or "dw" in w or "bwd" in w or "backward" in w:
        return "grad"
    return "fwd"


# "param": a weight after Adam steps.  The first update is lr g / (|g| + eps): ill-conditioned where |g| ~ eps, so a weight of 1 % of its tensor's maximum
# moves with the summation ORDER of its gradient (measured worst 5.4e-3 of such a weight = 3e-6 absolute = 0.3 % of one update step, after the Linear
# layers' GEMM changed its k order; 3.3e-3 before) -- the bound is a fraction of an update step, not a statement about the gradient (that is "grad").
REL_LIMIT = {"fwd": 1e-3, "grad": 2e-3, "param": 1e-2}
