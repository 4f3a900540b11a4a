"""features.0's sparse weight gradient (csrc/wgrad_sparse.h, SpCfg<64, 3, *>) through its three entry points, at the smallest shapes
where the tile staging can go wrong: 8 tiles (strips of 8 rows) per image, so the first and the last strip (halo rows outside the
image), columns 0 and 63, and the half-filled third store pass of every tile; n = 1, 2, 3 frames and n_a = 1, 2 for the mixes, plus
one batch of each kind in which some workgroups take two tiles (both prefetch stages).

Frames: every byte differs from its neighbours in the row, the column and the channel (a seeded permutation of 0..255 walked with a
skew per row and per image), so that a wrong lane-to-pixel map cannot cancel.  Pooled gradients on a dyadic grid (k / 8, |k| <= 16),
argmax nibbles uniform over the four window positions and the dead codes 4..15.  The reference is the definition in float64
    dW[ky][kx][ci][co] = sum X[y + ky - 1][x + kx - 1][ci] dE[cell][co]   over the cells and their argmax pixel (y, x),  db[co] = sum dE
on X = byte / 255 (or the mix a (1 - z) + z b of two such frames).  With dyadic gradients the kernel's sums differ from it by the fp32
rounding of byte / 255 and of the mix only; the tolerance is the one the existing weight-gradient tests of this layer use
(tests/test_gpu_kernels.py rel_close: rtol 1e-4 as for the virtual mixes, absolute term 2e-5 of the largest element)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL_SCALE = 1e-4, 2e-5


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_frames(n, seed):
    perm = np.random.RandomState(seed).permutation(256).astype(np.uint8)
    i = np.arange(n * 64 * 64 * 3, dtype=np.int64)
    return perm[(i + 7 * (i // 192) + 31 * (i // 12288)) % 256].reshape(n, 64, 64, 3)


def make_grad(n, seed):
    rs = np.random.RandomState(seed)
    dy = (rs.randint(-16, 17, size=(n, 32, 32, 8)) / 8.0).astype(np.float32)
    nib = rs.randint(0, 5, size=(n, 32, 32, 8))                      # 0..3: argmax position, 4: dead ...
    nib = np.where(nib == 4, rs.randint(4, 16, size=nib.shape), nib)  # ... as any of the codes 4..15
    words = np.zeros((n, 32, 32), dtype=np.uint64)
    for co in range(8):
        words |= nib[..., co].astype(np.uint64) << np.uint64(4 * co)
    return dy, nib, words.astype(np.uint32).view(np.int32).reshape(n, 32, 32, 1)


def reference(x64, dy, nib):
    """[28][8] in float64: rows (ky, kx, ci) then the bias row."""
    n = x64.shape[0]
    dense = np.zeros((n, 64, 64, 8), dtype=np.float64)
    ni, cy, cx, co = np.nonzero(nib < 4)
    p = nib[ni, cy, cx, co]
    dense[ni, 2 * cy + (p >> 1), 2 * cx + (p & 1), co] = dy[ni, cy, cx, co]
    xp = np.zeros((n, 66, 66, 3), dtype=np.float64)
    xp[:, 1:65, 1:65] = x64
    out = np.zeros((28, 8), dtype=np.float64)
    for ky in range(3):
        for kx in range(3):
            out[(ky * 3 + kx) * 3:(ky * 3 + kx) * 3 + 3] = np.einsum("nyxc,nyxo->co", xp[:, ky:ky + 64, kx:kx + 64], dense)
    out[27] = dense.sum((0, 1, 2))
    return out


def close(got, ref, what):
    got = np.asarray(got, dtype=np.float64).reshape(28, 8)
    err = np.abs(got - ref)
    bound = RTOL * np.abs(ref) + ATOL_SCALE * np.abs(ref).max()
    print(f"{what}: max |err| {err.max():.3e}, max |ref| {np.abs(ref).max():.3e}, worst err / bound {(err / bound).max():.3e}")
    assert np.abs(ref).max() > 1 and np.isfinite(got).all() and np.all(err <= bound), f"{what}: {(err / bound).max()} of the bound"


@pytest.fixture(scope="module")
def env():
    from cgs_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    return dict(L=_lib, lib=lib, dev=dev, cache={})


def case(env, n):
    """Frames A (and B for the mixes), gradient, nibbles and the float64 reference of n frames, computed once."""
    if n not in env["cache"]:
        a, b = make_frames(n, 11 + n), make_frames(n, 211 + n)
        dy, nib, words = make_grad(n, 411 + n)
        T = lambda v: torch.from_numpy(v).to(env["dev"])
        env["cache"][n] = dict(a=a, b=b, dy=dy, nib=nib, A=T(a), B=T(b), DY=T(dy), AM=T(words), ref=reference(a.astype(np.float64) / 255.0, dy, nib))
    return env["cache"][n]


def desc(env, n, src):
    L = env["L"]
    return L.ConvDesc(n, 64, 64, 3, 0, 8, src, 2, L.ACT_RELU, 1, L.Dropout())


def run_bwd_weight(env, n, src, x, dy, am):
    L, lib = env["L"], env["lib"]
    d = desc(env, n, src)
    ns = lib.cgs_conv3x3_bwd_weight_slabs(C.byref(d))
    assert 0 < ns <= 8 * n
    slab = torch.full((ns, 224), float("nan"), device=env["dev"])
    L.call("cgs_conv3x3_bwd_weight", C.byref(d), P(x), None, P(dy), P(am), P(slab), stream())
    torch.cuda.synchronize()
    return slab


def run_with_head(env, n, x, dy, am):
    L, lib, dev = env["L"], env["lib"], env["dev"]
    ns = lib.cgs_conv3x3_bwd_weight_slabs(C.byref(desc(env, n, L.SRC_U8)))
    slab = torch.full((ns, 224), float("nan"), device=dev)
    rs = np.random.RandomState(5)
    hvec = torch.from_numpy(rs.randn(n, 384).astype(np.float32)).to(dev)
    e4 = torch.from_numpy(rs.randn(n, 32).astype(np.float32)).to(dev)
    sh = torch.zeros(lib.cgs_tail_head_wgrad_slabs(n), 9313, device=dev)
    L.call("cgs_enc0_wgrad_u8_with_head", n, P(x), P(dy), P(am), P(slab), n, P(hvec), P(e4), None, 0, 0, None, None, None, 0, P(sh), None, stream())
    torch.cuda.synchronize()
    return slab


def run_mix(env, n_a, inject, A, B, Z, dy, am, mixed=None):
    L, lib, dev = env["L"], env["lib"], env["dev"]
    n_mix = 2 * n_a if inject else n_a
    ns = lib.cgs_enc0_bwd_mix_slabs(n_mix)
    assert ns > 0
    slab = torch.full((ns, 224), float("nan"), device=dev)
    w = torch.from_numpy(np.random.RandomState(6).randn(3, 3, 3, 8).astype(np.float32)).to(dev)
    dz = torch.empty(n_a, 64, 64, device=dev)
    L.call("cgs_enc0_bwd_mix", n_a, int(inject), P(mixed), P(dy), P(am), P(w), P(A), P(B), P(Z), 0.0, 0.0, None, P(dz), P(slab), stream())
    torch.cuda.synchronize()
    return slab


def as_f32_frames(a):
    return a.astype(np.float32) * np.float32(1.0 / 255.0)      # the kernel's own expression: one fp32 product per byte


@pytest.mark.parametrize("n", [1, 2, 3, 113])      # 113: 904 tiles on 896 workgroups, eight of them with two tiles
def test_frames_weight_gradient(env, n):
    """cgs_conv3x3_bwd_weight on uint8 and on fp32 frames, cgs_enc0_wgrad_u8_with_head: each against float64, and bit-identical slabs."""
    L = env["L"]
    c = case(env, n)
    s_u8 = run_bwd_weight(env, n, L.SRC_U8, c["A"], c["DY"], c["AM"])
    xf = torch.from_numpy(as_f32_frames(c["a"])).to(env["dev"])
    s_f32 = run_bwd_weight(env, n, L.SRC_F32, xf, c["DY"], c["AM"])
    s_head = run_with_head(env, n, c["A"], c["DY"], c["AM"])
    for name, s in (("uint8", s_u8), ("fp32", s_f32), ("with_head", s_head)):
        close(s.double().sum(0).cpu().numpy(), c["ref"], f"features.0 weight gradient, {name} frames, n = {n}")
    assert s_u8.shape == s_f32.shape == s_head.shape
    assert torch.equal(s_u8, s_f32) and torch.equal(s_u8, s_head)


@pytest.mark.parametrize("n_a,inject", [(1, False), (1, True), (2, False), (2, True), (33, True)])      # 33: 528 tiles on 512 workgroups
def test_mix_weight_gradient(env, n_a, inject):
    """cgs_enc0_bwd_mix on the virtual mixes (a, b, z in the tile loader) against float64; with z = 0 the mixes ARE the frames
    [A | B]: bit-identical to the uint8 path on those frames, and to the materialised fp32 mixes."""
    L, dev = env["L"], env["dev"]
    n_mix = 2 * n_a if inject else n_a
    c, g = case(env, n_a), case(env, n_mix)
    A, B, a, b = c["A"], c["B"], c["a"], c["b"]
    z = (np.random.RandomState(7 + n_a).randint(0, 17, size=(n_a, 64, 64)) / 16.0).astype(np.float32)
    a64, b64, z64 = a.astype(np.float64) / 255.0, b.astype(np.float64) / 255.0, z.astype(np.float64)[..., None]
    mixes = [a64 * (1 - z64) + z64 * b64] + ([b64 * (1 - z64) + z64 * a64] if inject else [])
    ref = reference(np.concatenate(mixes), g["dy"], g["nib"])
    s = run_mix(env, n_a, inject, A, B, torch.from_numpy(z).to(dev), g["DY"], g["AM"])
    close(s.double().sum(0).cpu().numpy(), ref, f"features.0 weight gradient, virtual mixes, n_a = {n_a}, inject = {inject}")
    # z = 0: the same image through the three sources
    z0 = torch.zeros(n_a, 64, 64, device=dev)
    s_vir = run_mix(env, n_a, inject, A, B, z0, g["DY"], g["AM"])
    frames = np.concatenate([a, b]) if inject else a
    s_mat = run_mix(env, n_a, inject, A, B, z0, g["DY"], g["AM"], mixed=torch.from_numpy(as_f32_frames(frames)).to(dev))
    s_u8 = run_bwd_weight(env, n_mix, L.SRC_U8, torch.from_numpy(frames).to(dev), g["DY"], g["AM"])
    assert torch.equal(s_vir, s_mat)
    if s_u8.shape == s_vir.shape:      # one tile per slab in both launches: the same partition of the sum
        assert torch.equal(s_vir, s_u8) and torch.equal(s_vir.sum(0), s_u8.sum(0))
    else:
        assert n_a == 33
    close(s_vir.double().sum(0).cpu().numpy(), reference(frames.astype(np.float64) / 255.0, g["dy"], g["nib"]), f"mixes at z = 0, n_a = {n_a}, inject = {inject}")
