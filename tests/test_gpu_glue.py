"""The training step's glue kernels (csrc/elementwise.hip), each through the C ABI against the float64 references of
tests/glue_ref.py (which tests/test_glue_host.py ties to the objective itself).  Every output buffer is NaN before the launch,
every size comes from the library's own count functions, every call's return code is checked (_lib.call raises), and each test
synchronises once after its launches.

Tolerances count float32 roundings; eps = 2^-24 (glue_ref.EPS).  Two bounds are stated against a MAGNITUDE (the expression
with every term replaced by its absolute value) where terms of either sign are added, because an error of eps per term is
relative to the terms, not to what is left after they cancel:
  * the mix backward (glue_ref.mix_bwd's bound);
  * Adam's first moment m = b1 m + (1 - b1) g: m and g of opposite sign cancel, so `4 eps relative` is taken of
    |b1 m| + |(1 - b1) g| (= |m| itself wherever the two agree in sign), and the 64 eps of the parameter's update likewise of the
    update formed with that magnitude (glue_ref.adam's m_bound / update_bound).  v's terms are non-negative: 4 eps of v itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import glue_ref as gr
from glue_ref import EPS, LFAK, L1, L2, LOSS_RTOL

pytestmark = pytest.mark.gpu

def _mods():
    from cgs_amd import _lib
    return _lib, _lib.load()


def DEV():
    return torch.device("cuda:0")


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV())


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV(), dtype=torch.float32)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.int32)


def worst(err, tol, what):
    """Largest err / tol (printed: the margin is part of the record), asserted <= 1.  tol == 0 demands err == 0."""
    err, tol = np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    assert not np.isnan(err).any(), f"{what}: NaN left in the output"
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    w = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: worst err/tol {w:.3f}")
    assert w <= 1.0, f"{what}: err/tol {w:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"


def mix_inputs(n, hw, seed, negatives=False):
    """uint8 frames with the bytes 0 and 255, Z in [0, 1) with exact 0 and exact 1 (and, for the backward, a few negative values)."""
    rs = np.random.RandomState(seed)
    A = rs.randint(0, 256, (n, hw, 3)).astype(np.uint8)
    B = rs.randint(0, 256, (n, hw, 3)).astype(np.uint8)
    A[0, :3] = [[0, 255, 0], [255, 255, 255], [0, 0, 0]]
    B[0, :3] = [[255, 0, 0], [0, 0, 255], [255, 255, 255]]
    Z = rs.rand(n, hw).astype(np.float32)
    Z[0, 0], Z[0, 1], Z[-1, -1], Z[-1, -2] = 0.0, 1.0, 1.0, 0.0
    if negatives:
        Z[0, 4:8] = [-0.25, -0.5, -1.0, -0.125]
        Z[-1, hw // 2] = -0.75
    return A, B, Z


# ------------------------------------------------------------------------------------------------
# cgs_mix_fwd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inject", [0, 1])
@pytest.mark.parametrize("n,hw", [(1, 4096), (5, 4096), (257, 4096), (65, 16384)])
def test_mix_fwd(n, hw, inject):
    """mixed within 8 eps absolute (values in [0, 1], at most 6 roundings); image k's partials sum to its float64
    (sum |Z|, sum Z^2) within 64 eps relative (non-negative terms: at most 8 serial adds, then the wave and workgroup tree)."""
    _lib, lib = _mods()
    A, B, Z = mix_inputs(n, hw, 100 + n + inject)
    Ad, Bd, Zd = dev(A), dev(B), dev(Z)
    cnt = lib.cgs_mix_fwd_partials(n, hw)
    assert cnt > 0 and cnt % n == 0
    mixed, zp, zp_only = nan(2 * n, hw, 3), nan(cnt, 2), nan(cnt, 2)
    _lib.call("cgs_mix_fwd", n, hw, P(Ad), P(Bd), P(Zd), inject, P(mixed), P(zp), S())
    _lib.call("cgs_mix_fwd", n, hw, None, None, P(Zd), inject, None, P(zp_only), S())
    torch.cuda.synchronize()
    ref, zsum = gr.mix_fwd(A, B, Z, inject)
    got = host(mixed)
    n_mix = n * (1 + inject)
    worst(np.abs(got[:n_mix] - ref), np.full(ref.shape, 8 * EPS), "mixed")
    if not inject:
        assert np.isnan(got[n:]).all(), "inject = 0 wrote the injected slots"
    per_image = host(zp).astype(np.float64).reshape(n, cnt // n, 2).sum(1)
    worst(np.abs(per_image - zsum), 64 * EPS * zsum, "per-image partial sums")
    assert np.array_equal(bits(zp), bits(zp_only)), "mixed = NULL partials differ from the partials with mixed given"


# ------------------------------------------------------------------------------------------------
# cgs_mix_bwd / cgs_mix_bwd_weighted / cgs_enc0_bwd_mix(vf_pred)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inject", [0, 1])
@pytest.mark.parametrize("n,hw", [(1, 4096), (5, 4096), (2, 16384)])
def test_mix_bwd_and_weighted(n, hw, inject):
    """|err| <= 16 eps x the magnitude bound, for every regulariser combination, with and without valuefak; cgs_mix_bwd is
    cgs_mix_bwd_weighted(vf_pred = NULL) bit for bit.  The scales are of order one so that the regulariser terms weigh as much
    as the gradient through the mixes."""
    _lib, lib = _mods()
    A, B, Z = mix_inputs(n, hw, 200 + n + inject, negatives=True)
    rs = np.random.RandomState(300 + n + inject)
    n_mix = n * (1 + inject)
    dmixed = rs.randn(n_mix, hw, 3).astype(np.float32)
    vfp = rs.rand(n).astype(np.float32)
    vfp[0] = 1.0
    vfp[-1] = 0.0 if n > 1 else 1.0
    vfp0 = np.zeros(n, np.float32)                  # (n = 1 sees both ends over the two vectors)
    Ad, Bd, Zd, dmd = dev(A), dev(B), dev(Z), dev(dmixed)
    a, b = gr.f32(0.75), gr.f32(0.4)
    runs, keep = [], []
    for l1s, l2s in ((0.0, 0.0), (a, 0.0), (0.0, b), (a, b)):
        out, out_w = nan(n, hw), nan(n, hw)
        _lib.call("cgs_mix_bwd", n, hw, P(Ad), P(Bd), P(Zd), P(dmd), inject, l1s, l2s, P(out), S())
        _lib.call("cgs_mix_bwd_weighted", n, hw, P(Ad), P(Bd), P(Zd), P(dmd), inject, l1s, l2s, None, P(out_w), S())
        runs.append((l1s, l2s, None, out, out_w))
        for vf in (vfp, vfp0):
            vd, o = dev(vf), nan(n, hw)
            _lib.call("cgs_mix_bwd_weighted", n, hw, P(Ad), P(Bd), P(Zd), P(dmd), inject, l1s, l2s, P(vd), P(o), S())
            runs.append((l1s, l2s, vf, o, None))
            keep.append(vd)
    torch.cuda.synchronize()
    for l1s, l2s, vf, out, out_w in runs:
        ref, bound = gr.mix_bwd(A, B, Z, dmixed, inject, l1s, l2s, vf)
        worst(np.abs(host(out) - ref), 16 * EPS * bound, f"dzpre l1s {l1s} l2s {l2s} vf {'none' if vf is None else vf[0]}")
        if out_w is not None:
            assert np.array_equal(bits(out), bits(out_w)), "cgs_mix_bwd != cgs_mix_bwd_weighted(NULL)"


def test_enc0_bwd_mix_with_valuefak(g1):
    """cgs_enc0_bwd_mix with a vf_pred argument == glue_ref.mix_bwd applied to what cgs_conv3x3_bwd_data produces, to the
    tolerance of test_enc0_backward_with_mix_backward_equals_two_launches (2e-5 of the largest element: the fused kernel
    forms the same sums in another order)."""
    _lib, lib = _mods()
    from cgs_amd import hourglass as hg, spec
    lc = spec.critic_layout()
    fc = torch.empty(lc.total, device=DEV())
    lc.flatten({k: v.to(DEV()) for k, v in g1[0].items()}, fc)
    n_a, n_mix = 5, 10
    rs = np.random.RandomState(77)
    A, B, Z = mix_inputs(n_a, 4096, 78)
    dy = rs.randn(n_mix, 32, 32, 8).astype(np.float32)
    am = rs.randint(0, 2 ** 31, (n_mix, 32, 32, 1)).astype(np.int32)
    vfp = rs.rand(n_a).astype(np.float32)
    vfp[0], vfp[-1] = 0.0, 1.0
    l1s, l2s = gr.f32(0.3), gr.f32(0.2)
    Ad, Bd, Zd, dyd, amd, vd = dev(A), dev(B), dev(Z), dev(dy), dev(am), dev(vfp)
    w = C.c_void_p(fc.data_ptr() + 4 * lc.off("features.0.weight"))
    d = hg.conv_desc(n_mix, 64, 3, 0, 8, False, 2, "relu", 1, _lib.Dropout())
    dmix, dz = nan(n_mix, 64, 64, 3), nan(n_a, 64, 64)
    _lib.call("cgs_conv3x3_bwd_data", C.byref(d), P(dyd), P(amd), w, None, _lib.ACT_NONE, None, 0, P(dmix), None, S())
    _lib.call("cgs_enc0_bwd_mix", n_a, 1, None, P(dyd), P(amd), w, P(Ad), P(Bd), P(Zd), l1s, l2s, P(vd), P(dz), None, S())
    torch.cuda.synchronize()
    ref, _ = gr.mix_bwd(A, B, Z, host(dmix).reshape(n_mix, 4096, 3), 1, l1s, l2s, vfp)
    unweighted, _ = gr.mix_bwd(A, B, Z, host(dmix).reshape(n_mix, 4096, 3), 1, l1s, l2s, None)
    tol = 2e-5 * np.abs(ref).max()
    assert np.abs(unweighted - ref).max() > 100 * tol           # (dropping the weighting would miss by far more than the tolerance)
    worst(np.abs(host(dz).reshape(n_a, 4096) - ref), np.full(ref.shape, tol), "enc0_bwd_mix dzpre with valuefak")


# ------------------------------------------------------------------------------------------------
# cgs_phase1_loss / cgs_phase2_losses / the loss values of cgs_reduce_adam
# ------------------------------------------------------------------------------------------------
def mask_partials(n, hw):
    """Enqueues cgs_mix_fwd(mixed = NULL) on the shared n-image mask (the caller's one synchronise covers it): (device partials,
    their count, float64 per-image sums, the device mask to keep alive)."""
    _lib, lib = _mods()
    Z = gr.mask_inputs(n, hw)
    cnt = lib.cgs_mix_fwd_partials(n, hw)
    Zd, zp = dev(Z), nan(cnt, 2)
    _lib.call("cgs_mix_fwd", n, hw, None, None, P(Zd), 0, None, P(zp), S())
    return zp, cnt, gr.mask_sums(Z), Zd


def check_losses(got, ref, what):
    worst(np.abs(got[:6] - ref), LOSS_RTOL * np.abs(ref), what)


PHASE2_SHAPES = [(n, 4096, f) for n in (1, 63, 64, 65, 255, 256, 257, 300) for f in range(16)] + [(65, 16384, f) for f in range(8, 16)]


@pytest.mark.parametrize("n,hw,flags", PHASE2_SHAPES)
def test_phase2_losses(n, hw, flags):
    """Each loss within 1e-5 relative (sums of non-negative terms; the margin covers logf and the rounding of 1 - p); dpred
    within 16 eps purely relative and exactly 0 where the reference is 0 (the whole B slot; the A slot of a frozen critic).
    The partials are cgs_mix_fwd's, so flag 8 above 256 images of 64x64 (64 of 128x128) needs them to be per image.
    Under bce the A slot holds an exact 0 at every n and an exact 1 from n = 2 on (glue_ref.loss_inputs): n = 1 does not
    reach the clamp of log(1 - p) at p = 1."""
    _lib, lib = _mods()
    inject, bce = bool(flags & gr.INJECT), bool(flags & gr.BCE)
    zp, cnt, zsum, Zd = mask_partials(n, hw)
    pred, y = gr.loss_inputs(n, bce)
    pd, yd = dev(pred), dev(y)
    losses, dpred = nan(8), nan(4 * n)
    _lib.call("cgs_phase2_losses", n, P(pd), P(yd), P(zp), cnt, LFAK, L1, L2, flags, n * hw, P(losses), P(dpred), S())
    torch.cuda.synchronize()
    ref_l, ref_d = gr.phase2(pred if inject else pred[:3 * n], y, zsum, n, LFAK, L1, L2, flags, n * hw)
    got_l, got_d = host(losses).astype(np.float64), host(dpred).astype(np.float64)
    check_losses(got_l, ref_l, f"losses n {n} flags {flags}")
    assert got_l[6] == 0 and got_l[7] == 0
    worst(np.abs(got_d[:ref_d.size] - ref_d), 16 * EPS * np.abs(ref_d), "dpred")
    assert not got_d[:n].any()
    if not inject:
        assert np.isnan(got_d[3 * n:]).all(), "inject = 0 wrote the injected slot of dpred"


@pytest.mark.parametrize("bce", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 300])
def test_phase1_loss(n, bce):
    _lib, lib = _mods()
    pred4, y = gr.loss_inputs(n, bce)
    pred = pred4[n:2 * n].copy()                      # the A slot: exact 0 and exact 1 under bce
    pd, yd = dev(pred), dev(y)
    loss, dpred = nan(8), nan(n + 8)
    _lib.call("cgs_phase1_loss", n, P(pd), P(yd), bce, P(loss), P(dpred), S())
    torch.cuda.synchronize()
    ref_l, ref_d = gr.phase1(pred, y, bce)
    got_l, got_d = host(loss).astype(np.float64), host(dpred).astype(np.float64)
    worst(abs(got_l[0] - ref_l), LOSS_RTOL * abs(ref_l), f"phase-1 loss n {n} bce {bce}")
    worst(np.abs(got_d[:n] - ref_d), 16 * EPS * np.abs(ref_d), "dpred")
    assert np.isnan(got_d[n:]).all() and np.isnan(got_l[1:]).all()


def job_table(rows):
    """Device table of cgs_reduce_job entries (slab pointer, dst pointer, nslab, stride, count, accumulate), as SlabPlan.build makes it."""
    _lib, _ = _mods()
    arr = (_lib.ReduceJob * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = _lib.ReduceJob(*r)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV())


@pytest.mark.parametrize("flags", [3, 11, 15])
@pytest.mark.parametrize("n", [5, 257])
def test_fused_tail_loss_values(n, flags):
    """cgs_reduce_adam (one trivial reduction job, param = NULL): losses[0..5] equal cgs_phase2_losses' on the same inputs to
    8 eps relative (the same terms summed by 512 threads instead of 256) and the float64 reference to 1e-5."""
    _lib, lib = _mods()
    hw = 4096
    zp, cnt, zsum, Zd = mask_partials(n, hw)
    pred, y = gr.loss_inputs(n, bool(flags & gr.BCE))
    pd, yd = dev(pred), dev(y)
    slab, dst = dev(np.array([3.0], np.float32)), nan(1)
    jobs = job_table([(slab.data_ptr(), dst.data_ptr(), 1, 1, 1, 0)])
    step = torch.full((1,), 7, dtype=torch.int64, device=DEV())
    ticket = torch.zeros(3, dtype=torch.int32, device=DEV())
    fused, plain, dpred = nan(8), nan(8), nan(4 * n)
    _lib.call("cgs_reduce_adam", P(jobs), 1, 1, P(step), None, P(dst), None, None, 1e-3, 0.9, 0.999, 1e-8, P(ticket), n, P(pd), P(yd),
              P(zp), cnt, LFAK, L1, L2, flags, n * hw, P(fused), S())
    _lib.call("cgs_phase2_losses", n, P(pd), P(yd), P(zp), cnt, LFAK, L1, L2, flags, n * hw, P(plain), P(dpred), S())
    torch.cuda.synchronize()
    ref_l, _ = gr.phase2(pred, y, zsum, n, LFAK, L1, L2, flags, n * hw)
    f, p = host(fused).astype(np.float64), host(plain).astype(np.float64)
    check_losses(f, ref_l, f"fused losses n {n} flags {flags}")
    worst(np.abs(f[:6] - p[:6]), 8 * EPS * np.abs(p[:6]), "fused against cgs_phase2_losses")
    assert f[6] == 0 and f[7] == 0
    assert int(step.item()) == 8 and not host(ticket).any() and float(dst.item()) == 3.0


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
LR, B1, B2, ADAM_EPS = gr.f32(1e-3), gr.f32(0.9), gr.f32(0.999), gr.f32(1e-8)


def adam_state(count, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(count).astype(np.float32), (rs.randn(count) * 0.1).astype(np.float32),
            (rs.rand(count) * 0.01).astype(np.float32))                    # p, m, v (v >= 0)


def check_adam(got_p, got_m, got_v, st, p_before, what):
    """m, v within 4 eps relative (m: of its terms' magnitude, see the module docstring); p within eps |p| + 64 eps |update|: the bias
    corrections (double pow, or the expm1f form of the fused kernel) carry at most 8 eps, the rest is a handful of float operations."""
    worst(np.abs(got_m - st.m), 4 * EPS * st.m_bound, what + " m")
    worst(np.abs(got_v - st.v), 4 * EPS * np.abs(st.v), what + " v")
    worst(np.abs(got_p - st.p), EPS * np.abs(p_before) + 64 * EPS * st.update_bound, what + " p")


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("t", [1, 10, 100000])
@pytest.mark.parametrize("count", [1, 255, 257, 1000])
def test_adam_flat(count, t, gscale):
    """cgs_adam_flat reads the already ticked step counter t."""
    _lib, lib = _mods()
    p0, m0, v0 = adam_state(count, 400 + count)
    g = (np.random.RandomState(count + t).randn(count) * 0.3).astype(np.float32)
    pad = 8                                            # the floats after `count` must stay as they are
    bufs = [dev(np.concatenate([x, np.full(pad, 9.0, np.float32)])) for x in (p0, m0, v0)]
    gd = dev(g)
    step = torch.full((1,), t, dtype=torch.int64, device=DEV())
    _lib.call("cgs_adam_flat", count, P(bufs[0]), P(gd), P(bufs[1]), P(bufs[2]), P(step), LR, B1, B2, ADAM_EPS, gscale, S())
    torch.cuda.synchronize()
    st = gr.adam(p0, g, m0, v0, t, LR, B1, B2, ADAM_EPS, gscale)
    gp, gm, gv = (host(b).astype(np.float64) for b in bufs)
    check_adam(gp[:count], gm[:count], gv[:count], st, p0, f"adam_flat count {count} t {t}")
    assert (gp[count:] == 9).all() and (gm[count:] == 9).all() and (gv[count:] == 9).all()
    assert int(step.item()) == t


@pytest.mark.parametrize("step0", [0, 9, 99999])
@pytest.mark.parametrize("count", [1, 255, 257, 1000])
def test_reduce_adam_two_steps(count, step0):
    """Two launches back to back (another gradient in the slab for the second): both steps match float64 Adam on the reduced
    gradient the kernel leaves in dst, the counter rises by one per launch, the ticket words are zero after each, and only the
    elements the job's dst addresses move."""
    _lib, lib = _mods()
    nslab, off, total = 3, 8, count + 16
    rs = np.random.RandomState(500 + count + step0)
    slabs = [(rs.randn(nslab, count) * 0.3).astype(np.float32) for _ in range(2)]
    state = [np.concatenate([np.full(off, 9.0, np.float32), x, np.full(total - off - count, 9.0, np.float32)]) for x in adam_state(count, 600 + count)]
    p, m, v = (dev(x) for x in state)
    grad = nan(total)
    slab = dev(slabs[0])
    nxt = dev(slabs[1])
    jobs = job_table([(slab.data_ptr(), grad.data_ptr() + 4 * off, nslab, count, count, 0)])
    step = torch.full((1,), step0, dtype=torch.int64, device=DEV())
    ticket = torch.zeros(3, dtype=torch.int32, device=DEV())
    snaps = []
    for k in range(2):
        _lib.call("cgs_reduce_adam", P(jobs), 1, count, P(step), P(p), P(grad), P(m), P(v), LR, B1, B2, ADAM_EPS, P(ticket), 0, None, None,
                  None, 0, 0.0, 0.0, 0.0, 0, 0, None, S())
        snaps.append([t.clone() for t in (p, m, v, grad, step, ticket)])
        if k == 0:
            slab.copy_(nxt)
    torch.cuda.synchronize()
    before = state
    for k in range(2):
        gp, gm, gv, gg, gs, gt = (host(t) for t in snaps[k])
        assert int(gs[0]) == step0 + k + 1 and not gt.any()
        red, mag = gr.reduce(slabs[k], nslab, count, count)
        worst(np.abs(gg[off:off + count] - red), 64 * EPS * mag, f"step {k} reduced gradient")
        assert np.isnan(gg[:off]).all() and np.isnan(gg[off + count:]).all()
        st = gr.adam(before[0][off:off + count], gg[off:off + count], before[1][off:off + count], before[2][off:off + count],
                     step0 + k + 1, LR, B1, B2, ADAM_EPS)
        check_adam(gp[off:off + count].astype(np.float64), gm[off:off + count].astype(np.float64), gv[off:off + count].astype(np.float64),
                   st, before[0][off:off + count], f"reduce_adam count {count} step {step0 + k + 1}")
        for got in (gp, gm, gv):
            assert (got[:off] == 9).all() and (got[off + count:] == 9).all()
        before = [gp, gm, gv]


# ------------------------------------------------------------------------------------------------
# slab reduction
# ------------------------------------------------------------------------------------------------
REDUCE_JOBS = [(1, 1, 1), (31, 3, 3), (33, 127, 127), (512, 128, 128), (513, 129, 132), (2048, 131, 131), (100, 260, 264)]   # (nslab, count, stride)


def up4(x):
    return (x + 3) // 4 * 4


def reduce_setup(accumulate, seed):
    """One slab buffer and one gradient buffer holding every job at a 16-byte aligned offset; a job's dst region is `stride`
    floats of which only the first `count` may change."""
    rs = np.random.RandomState(seed)
    slab_np, dst_np, rows, so, do = [], [], [], 0, 0
    for nslab, count, stride in REDUCE_JOBS:
        s = rs.randn(up4(nslab * stride)).astype(np.float32)
        d = rs.randn(up4(stride)).astype(np.float32)
        rows.append((so, do, nslab, stride, count, s, d))
        slab_np.append(s); dst_np.append(d)
        so += s.size; do += d.size
    slab, dst = dev(np.concatenate(slab_np)), dev(np.concatenate(dst_np))
    assert slab.data_ptr() % 16 == 0
    table = job_table([(slab.data_ptr() + 4 * a, dst.data_ptr() + 4 * b, ns, st, c, int(accumulate)) for a, b, ns, st, c, _, _ in rows])
    return slab, dst, rows, table


def check_reduced(dst, rows, accumulate, what):
    got = host(dst)
    for so, do, nslab, stride, count, s, d in rows:
        ref, mag = gr.reduce(s, nslab, stride, count, d, accumulate)
        worst(np.abs(got[do:do + count] - ref), 64 * EPS * mag, f"{what} job {(nslab, count, stride)}")
        assert np.array_equal(got[do + count:do + d.size].view(np.int32), d[count:].view(np.int32)), "columns at and after count changed"


@pytest.mark.parametrize("accumulate", [0, 1])
def test_reduce_slabs(accumulate):
    """Several jobs in one launch, max_count the largest count (short jobs see idle workgroups): |err| <= 64 eps sum |terms| per
    column, the columns at and after count untouched, the step word one higher."""
    _lib, lib = _mods()
    slab, dst, rows, table = reduce_setup(accumulate, 700 + accumulate)
    step = torch.full((1,), 41, dtype=torch.int64, device=DEV())
    _lib.call("cgs_reduce_slabs", P(table), len(rows), max(r[4] for r in rows), P(step), S())
    torch.cuda.synchronize()
    check_reduced(dst, rows, accumulate, "reduce_slabs")
    assert int(step.item()) == 42


@pytest.mark.parametrize("accumulate", [0, 1])
def test_reduce_adam_reduction(accumulate):
    """The same jobs through cgs_reduce_adam (param = NULL: reduction and tick only)."""
    _lib, lib = _mods()
    slab, dst, rows, table = reduce_setup(accumulate, 710 + accumulate)
    step = torch.full((1,), 41, dtype=torch.int64, device=DEV())
    ticket = torch.zeros(len(rows) + 2, dtype=torch.int32, device=DEV())
    _lib.call("cgs_reduce_adam", P(table), len(rows), max(r[4] for r in rows), P(step), None, P(dst), None, None, LR, B1, B2, ADAM_EPS,
              P(ticket), 0, None, None, None, 0, 0.0, 0.0, 0.0, 0, 0, None, S())
    torch.cuda.synchronize()
    check_reduced(dst, rows, accumulate, "reduce_adam")
    assert int(step.item()) == 42 and not host(ticket).any()


def test_reduce_slabs_step_word_and_null_step():
    """*step rises by one per launch that is given it, and a launch with step = NULL leaves it alone."""
    _lib, lib = _mods()
    slab, dst = dev(np.array([0.5], np.float32)), dev(np.array([1.0], np.float32))
    table = job_table([(slab.data_ptr(), dst.data_ptr(), 1, 1, 1, 1)])
    step = torch.full((1,), 99999, dtype=torch.int64, device=DEV())
    seen = []
    for sp in (step, None, step):
        _lib.call("cgs_reduce_slabs", P(table), 1, 1, P(sp), S())
        seen.append(step.clone())
    torch.cuda.synchronize()
    assert [int(s.item()) for s in seen] == [100000, 100000, 100001]
    assert float(dst.item()) == 2.5


def test_reduce_slabs_vector_rows_equal_scalar_rows_bitwise():
    """A 16-byte aligned job with stride % 4 == 0 (one 16-byte load per four columns) and the same rows at a slab pointer one
    float further (one column per pass) give the same bits: every column's sum is formed in the same order either way."""
    _lib, lib = _mods()
    nslab, count, stride = 513, 129, 132
    data = np.random.RandomState(720).randn(nslab * stride).astype(np.float32)
    aligned = dev(data)
    shifted = dev(np.concatenate([np.zeros(1, np.float32), data, np.zeros(3, np.float32)]))
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
    d0, d1 = nan(stride), nan(stride)
    table = job_table([(aligned.data_ptr(), d0.data_ptr(), nslab, stride, count, 0), (shifted.data_ptr() + 4, d1.data_ptr(), nslab, stride, count, 0)])
    _lib.call("cgs_reduce_slabs", P(table), 2, count, None, S())
    torch.cuda.synchronize()
    ref, mag = gr.reduce(data, nslab, stride, count)
    worst(np.abs(host(d0)[:count] - ref), 64 * EPS * mag, "aligned job")
    assert np.array_equal(bits(d0)[:count], bits(d1)[:count])
    assert np.isnan(host(d0)[count:]).all() and np.isnan(host(d1)[count:]).all()
