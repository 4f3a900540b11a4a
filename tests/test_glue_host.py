"""The float64 references of tests/glue_ref.py, checked on the CPU.

1. Against the objective itself: float64 torch autograd of the loss arrangement exactly as oracle/hourglass_ref.py
   (phase2_loss) and tests/golden/make_golden.py write it -- F.mse_loss, F.binary_cross_entropy, F.l1_loss(valuefak * Z, 0),
   F.mse_loss(valuefak * Z, 0) with valuefak = 1 - pred.detach() -- so the GPU tests of tests/test_gpu_glue.py compare the kernels
   with the training objective and not with a restatement of the kernels.
2. A guard on the fixture of the GPU test: on that test's own n = 257 inputs, partial sums that are NOT per image (the capped
   grid-stride layout cgs_mix_fwd had) must miss the reference by at least 1000 x the GPU test's tolerance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as gr
from glue_ref import LFAK, L1, L2, LOSS_RTOL      # the GPU test's own loss weights and tolerance

RTOL = 1e-12            # both sides are float64


def rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max()) if ref.size else 0.0


def objective(pred, zpre, A, B, Y, dmixed, n, lfak, L1, L2, live, inject, bce, staticnorm):
    """phase2_loss of oracle/hourglass_ref.py with the critic's four outputs as the leaf `pred` = [B | A | replaced | injected]
    and the mask as sigmoid(zpre); `dmixed` stands for the gradient arriving at the mixes from the critic's passes over them."""
    negpred, p = pred[:n].detach(), pred[n:2 * n]
    rv, iv = pred[2 * n:3 * n], pred[3 * n:4 * n]
    Z = torch.sigmoid(zpre)                                   # [n,1,h,w]
    parts = {}
    total = 0
    if live:
        cl = F.binary_cross_entropy(p, Y) if bce else F.mse_loss(p, Y)
        total = total + lfak * cl
        parts["critic"] = cl
    rl = F.mse_loss(rv, negpred.detach())
    total = total + rl
    parts["replace"] = rl
    replaced = A * (1 - Z) + Z * B
    mixes = [replaced]
    if inject:
        il = F.mse_loss(iv, p.detach())
        total = total + il
        parts["inject"] = il
        mixes.append(B * (1 - Z) + Z * A)
    valuefak = 1 if staticnorm else 1 - p.detach().view(-1, 1, 1, 1)
    if L1:
        nl = L1 * F.l1_loss(valuefak * Z, torch.zeros_like(Z))
        total = total + nl
        parts["norm"] = nl
    if L2:
        nl2 = L2 * F.mse_loss(valuefak * Z, torch.zeros_like(Z))
        total = total + nl2
        parts["norm2"] = nl2
    through_critic = (torch.cat(mixes) * dmixed).sum()
    return total, parts, Z, through_critic


CASES = [(live, inject, bce, staticnorm, L1, L2)
         for live in (True, False) for inject in (True, False) for bce in (True, False) for staticnorm in (True, False)
         for (L1, L2) in ((0.5, 0.0), (0.0, 0.3), (0.5, 0.3))]


@pytest.mark.parametrize("live,inject,bce,staticnorm,L1,L2", CASES)
def test_reference_is_the_objective_and_its_gradient(live, inject, bce, staticnorm, L1, L2):
    n, h, w, lfak = 3, 4, 8, 5.0
    hw = h * w
    rs = np.random.RandomState(7 + 8 * live + 4 * inject + 2 * bce + staticnorm)
    A_u8 = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    B_u8 = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    zpre_np = rs.randn(n, hw) * 2
    pred_np = rs.uniform(0.05, 0.95, 4 * n)
    if bce:
        y_np = np.array([1.0, 0.0, 1.0])
        pred_np[n], pred_np[n + 1] = 0.0, 1.0               # both log clamps and the 1e-12 denominator
    else:
        y_np = rs.randn(n)
    n_mix = 2 * n if inject else n
    dmixed_np = rs.randn(n_mix, h, w, 3)

    nchw = lambda x: torch.from_numpy(x.astype(np.float64) / 255.0).permute(0, 3, 1, 2)
    pred = torch.from_numpy(pred_np).requires_grad_(True)
    zpre = torch.from_numpy(zpre_np.reshape(n, 1, h, w)).requires_grad_(True)
    total, parts, Z, through = objective(pred, zpre, nchw(A_u8), nchw(B_u8), torch.from_numpy(y_np),
                                         torch.from_numpy(dmixed_np).permute(0, 3, 1, 2), n, lfak, L1, L2, live, inject, bce, staticnorm)
    (total + through).backward()

    Znp = Z.detach().numpy().reshape(n, hw)
    flags = gr.LIVE * live | gr.INJECT * inject | gr.BCE * bce | gr.WEIGHTED * (not staticnorm)
    mixed, zsum = gr.mix_fwd(A_u8, B_u8, Znp, inject)
    losses, dpred = gr.phase2(pred_np if inject else pred_np[:3 * n], y_np, zsum, n, lfak, L1, L2, flags, n * hw)
    want = [float(parts[k].detach()) if k in parts else 0.0 for k in ("critic", "replace", "inject", "norm", "norm2")] + [float(total.detach())]
    for k in range(6):
        assert abs(losses[k] - want[k]) <= RTOL * abs(want[k]), (k, losses[k], want[k])
    g = pred.grad.numpy()
    assert np.all(g[:n] == 0) and np.all(dpred[:n] == 0)
    assert rel(dpred, g[:dpred.size]) <= RTOL
    if not inject:
        assert np.all(g[3 * n:] == 0)
    # the mixes themselves, then the chain through them and through the sigmoid
    ref_mixed = torch.cat([nchw(A_u8) * (1 - Z) + Z * nchw(B_u8)] + ([nchw(B_u8) * (1 - Z) + Z * nchw(A_u8)] if inject else []))
    assert rel(mixed.reshape(n_mix, h, w, 3), ref_mixed.detach().permute(0, 2, 3, 1).numpy()) <= RTOL
    vf_pred = None if staticnorm else pred_np[n:2 * n]
    dz, bound = gr.mix_bwd(A_u8, B_u8, Znp, dmixed_np, inject, L1 / (n * hw), L2 / (n * hw), vf_pred)
    err = np.abs(dz - zpre.grad.numpy().reshape(n, hw))
    assert np.all(err <= RTOL * bound), float((err / bound).max())
    assert np.all(bound >= np.abs(dz))


def test_phase1_reference_is_the_objective_and_its_gradient():
    rs = np.random.RandomState(3)
    for bce in (False, True):
        n = 3
        p_np = rs.uniform(0.05, 0.95, n)
        y_np = np.array([1.0, 0.0, 1.0]) if bce else rs.randn(n)
        if bce:
            p_np[0], p_np[1] = 0.0, 1.0
        p = torch.from_numpy(p_np).requires_grad_(True)
        loss = F.binary_cross_entropy(p, torch.from_numpy(y_np)) if bce else F.mse_loss(p, torch.from_numpy(y_np))
        loss.backward()
        got, dp = gr.phase1(p_np, y_np, bce)
        assert abs(got - loss.item()) <= RTOL * abs(loss.item())
        assert rel(dp, p.grad.numpy()) <= RTOL


def test_sign_of_zero_is_zero_and_weights_are_per_image():
    A = np.zeros((2, 1, 4, 3), np.uint8)
    Z = np.array([[0.0, 0.5, -0.5, 1.0], [0.25, 0.25, 0.25, 0.25]])
    dm = np.zeros((2, 4, 3))
    dz, _ = gr.mix_bwd(A, A, Z, dm, 0, 1.0, 0.0, vf_pred=np.array([0.0, 1.0]))
    np.testing.assert_array_equal(dz[0], [0.0, 0.25, -1.0 * -0.5 * 1.5, 0.0])
    np.testing.assert_array_equal(dz[1], 0.0)                 # valuefak = 1 - 1


def test_adam_reference_is_torch_adam():
    rs = np.random.RandomState(11)
    p0, g = rs.randn(50), rs.randn(2, 50)
    p = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([p])
    m, v, q = np.zeros(50), np.zeros(50), p0
    for t in (1, 2):
        p.grad = torch.from_numpy(g[t - 1].copy())
        opt.step()
        st = gr.adam(q, g[t - 1] * 2, m, v, t, 1e-3, 0.9, 0.999, 1e-8, gscale=0.5)
        q, m, v = st.p, st.m, st.v
        np.testing.assert_allclose(q, p.detach().numpy(), rtol=1e-13, atol=0)
        assert np.all(st.m_bound >= np.abs(st.m)) and np.all(st.update_bound >= np.abs(st.update))


def test_reduce_reference():
    slab = np.arange(24, dtype=np.float32) - 7
    s, mag = gr.reduce(slab, 3, 8, 5)
    np.testing.assert_array_equal(s, slab.reshape(3, 8)[:, :5].astype(np.float64).sum(0))
    np.testing.assert_array_equal(mag, np.abs(slab.reshape(3, 8)[:, :5]).astype(np.float64).sum(0))
    s2, mag2 = gr.reduce(slab, 3, 8, 5, dst0=np.full(8, -2.0, np.float32), accumulate=True)
    np.testing.assert_array_equal(s2, s - 2)
    np.testing.assert_array_equal(mag2, mag + 2)


# ------------------------------------------------------------------------------------------------
# guard: the GPU test's inputs tell per-image partials from partials that straddle images
# ------------------------------------------------------------------------------------------------
def straddling_partials(Z, n, hw):
    """(sum |Z|, sum Z^2) per workgroup of a grid capped at 1024 workgroups of 256 four-pixel groups that grid-strides over
    ALL images' groups: above 256 images of 64x64 a workgroup's sums mix pixels of several images."""
    groups = n * hw // 4
    blocks = min((groups + 255) // 256, 1024)
    blk = (np.arange(groups) // 256) % blocks
    zg = Z.astype(np.float64).reshape(groups, 4)
    return np.stack([np.bincount(blk, np.abs(zg).sum(1), blocks), np.bincount(blk, (zg * zg).sum(1), blocks)], axis=1)


def weighted_like_the_loss_kernel(parts, pred, n, l1, l2, nz):
    """phase2_losses_kernel's flag-8 weighting: partial i belongs to image i / (partials / n)."""
    per_img = parts.shape[0] // n
    vf = 1 - pred.astype(np.float64)[n + np.arange(parts.shape[0]) // per_img]
    return l1 * (vf * parts[:, 0]).sum() / nz, l2 * (vf * vf * parts[:, 1]).sum() / nz


@pytest.mark.parametrize("n,hw", [(257, 4096), (300, 4096)])
@pytest.mark.parametrize("bce", [False, True])
def test_gpu_fixture_tells_per_image_partials_from_straddling_ones(n, hw, bce):
    Z = gr.mask_inputs(n, hw)
    pred, y = gr.loss_inputs(n, bce)
    zsum = gr.mask_sums(Z)
    flags = gr.LIVE | gr.INJECT | gr.WEIGHTED | (gr.BCE if bce else 0)
    losses, _ = gr.phase2(pred, y, zsum, n, LFAK, L1, L2, flags, n * hw)
    got = weighted_like_the_loss_kernel(straddling_partials(Z, n, hw), pred, n, L1, L2, n * hw)
    for k in (0, 1):
        miss = abs(got[k] - losses[3 + k]) / losses[3 + k]
        assert miss >= 1000 * LOSS_RTOL, (k, miss)
    # the same model below the cap is per image, and then it IS the reference
    m = 5
    Zs, (ps, ys) = gr.mask_inputs(m, hw), gr.loss_inputs(m, bce)
    zs = gr.mask_sums(Zs)
    ls, _ = gr.phase2(ps, ys, zs, m, LFAK, L1, L2, flags, m * hw)
    gs = weighted_like_the_loss_kernel(straddling_partials(Zs, m, hw), ps, m, L1, L2, m * hw)
    assert abs(gs[0] - ls[3]) <= 1e-12 * ls[3] and abs(gs[1] - ls[4]) <= 1e-12 * ls[4]
