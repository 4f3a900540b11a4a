"""The dyadic 64x64 fixture of tests/exact64_ref.py, checked on the CPU: its conditions hold for every draw and batch size that
test_gpu_exact64_forward.py uses, the loader facts the exactness rests on hold in fp32, the draws cover every weight element of
features.0 / masker.0 / masker.2, the reference restates oracle/hourglass_ref.py, a float32 torch evaluation equals it bit for bit
wherever exactness is claimed, every planted mutation moves a compared tensor, and a denser variant fails the conditions."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact64_ref as E
from oracle import hourglass_ref as orc

N = 3
MUT_DRAWS = tuple(range(0, 36, 5))      # 0, 5, .. 35: every residue mod 9 but 4, so every tap position of masker.2 (its four non-zeros share one)


@pytest.fixture(scope="module")
def fix():
    """draw -> fixture at n = 3, computed once and left unchanged."""
    return {d: E.fixture(d, N) for d in range(E.N_DRAWS)}


def test_conditions_hold_for_every_draw(fix):
    for d, f in fix.items():
        try:
            E.check_exactness64(f)
        except AssertionError as e:
            raise AssertionError(f"draw {d}: {e}")


@pytest.mark.parametrize("n", [1, E.N_DISTINCT])
def test_conditions_hold_for_draw_0_at_the_other_batch_sizes(n):
    """(A large batch of the GPU tests is the n = 8 images repeated: big_order.)"""
    E.check_exactness64(E.fixture(0, n))


def test_big_order_holds_every_distinct_image_and_is_not_periodic():
    for n in (257, 1025, 1100, 2049):
        idx = E.big_order(n)
        assert idx.shape == (n,) and set(idx.tolist()) == set(range(E.N_DISTINCT))
        assert all(not np.array_equal(idx[p:], idx[:-p]) for p in range(1, 65))


def test_a_denser_variant_fails_the_conditions(monkeypatch):
    """The conditions are real constraints: with every weight element non-zero the sums and the logits leave the exact range."""
    monkeypatch.setattr(E, "weight_mask", lambda key, shape, draw: np.ones(shape, dtype=bool))
    bad = 0
    for d in range(6):
        try:
            E.check_exactness64(E.fixture(d, N))
        except AssertionError:
            bad += 1
    assert bad == 6, bad


def test_chained_references_stay_exact_in_fp32(fix):
    """The two forms that chain into exact_ref's layers: the one-launch critic forward (exact_ref's chain on this file's e0) and the fused
    decoder + mask head (this file's mask head on exact_ref's o0) keep every sum of absolute terms below 2^22 quanta, in every draw."""
    import exact_ref as X
    small = []
    for d, f in fix.items():
        P = X.dyadic_params(d)
        for key in ("e0_u8", "e0_mix"):
            r = E.critic_chain(P, f[key])
            assert np.array_equal(r["e1"].astype(np.float32).astype(np.float64), r["e1"]) and np.abs(r["logit"]).max() < 64
        g = E.dec_mask_fixture(d, N, P)
        assert (g["mh_u8M"]["pre"] < 0).mean() > 0.1 and np.isfinite(g["Z_bound"]).all() and (g["Z_bound"] > 0).all()
        small.append(E.dec_mask_fixture(d, N, P, scale=E.DEC_SMALL)["unsaturated"])
    # with exact_ref's own o0 most of Z is saturated (masker.2 weakly checked); with the decoder's inputs scaled down it is not
    assert sum(u >= 0.25 for u in small) >= E.N_DRAWS - 1 and np.median(small) > 0.9, small
    for n in (1, E.N_DISTINCT):
        E.dec_mask_fixture(0, n, X.dyadic_params(0))
        E.dec_mask_fixture(0, n, X.dyadic_params(0), scale=E.DEC_SMALL)
    fb = E.dec_mask_fixture(0, 2, X.dyadic_params(0), scale=E.DEC_SMALL, fullbyte=True)
    assert fb["unsaturated"] > 0.9 and fb["Z_bound"].max() < 1e-3 and fb["bounds"]["hM"].max() < 1e-4


# ---- the loader facts ----
def test_fact_uint8_scaling_is_exact_for_0_and_255_only():
    v = E.u8_values(np.arange(256, dtype=np.uint8))
    assert v[0] == 0.0 and v[255] == 1.0 and np.float32(255) * (np.float32(1) / np.float32(255)) == np.float32(1)
    rest = v[1:255]
    assert (rest.astype(np.float16).astype(np.float64) != rest).all(), "a byte in 1..254 scales to an fp16 number"


def test_fact_mix_is_exact_under_any_contraction():
    f32 = np.float32
    for av in (0.0, 1.0):
        for bv in (0.0, 1.0):
            for z in (0.0, 0.25, 0.5, 0.75, 1.0):
                exact = av * (1 - z) + z * bv
                omz = f32(1) - f32(z)
                plain = f32(f32(av) * omz) + f32(f32(z) * f32(bv))
                fma_l = f32(float(f32(av)) * float(omz) + float(f32(f32(z) * f32(bv))))        # fma(av, 1 - z, z * bv): one rounding
                fma_r = f32(float(f32(z)) * float(f32(bv)) + float(f32(f32(av) * omz)))
                assert float(plain) == float(fma_l) == float(fma_r) == exact and exact * 4 == round(exact * 4)


def test_fact_leaky_relu_is_one_fp32_multiply():
    v = (np.arange(-2048, 2049) / 4.0).astype(np.float32)
    slope = np.float32(0.01)
    sel = np.where(v > 0, v, slope * v)                      # cgs_common.h
    mx = np.maximum(v, slope * v)                            # mask_fwd_body.h
    assert sel.dtype == np.float32 and np.array_equal(sel, mx)
    assert np.array_equal(E.lrelu32(v.astype(np.float64)), sel.astype(np.float64))
    t = F.leaky_relu(torch.from_numpy(v), 0.01).numpy()
    assert np.array_equal(t, sel), "torch's float32 LeakyReLU is another rule"
    neg = sel[v < 0].astype(np.float64)
    not16 = neg.astype(np.float16).astype(np.float64) != neg      # (float32(0.01) * -25 k rounds to -k / 4: those are fp16 numbers)
    assert not16.mean() > 0.9 and (neg * 4 != np.round(neg * 4)).mean() > 0.9, "negative-branch h values are dyadic"


def test_fact_sigmoid_bound_in_float32():
    x = np.arange(-13, 65, dtype=np.float64) / 4.0           # the range check_exactness64 allows
    assert x.min() == -E.LOGIT_MIN_ABS
    ref = 1.0 / (1.0 + np.exp(-x))
    x32 = x.astype(np.float32)
    got = (np.float32(1) / (np.float32(1) + np.exp(-x32))).astype(np.float64)
    assert (np.abs(got - ref) <= E.SIG_ULPS * 2.0 ** -23 * ref).all()
    assert np.array_equal(E.sig_bound(x, ref), E.SIG_ULPS * 2.0 ** -23 * ref), "sig_bound is family P's bound on the fixture's range"
    assert (E.sig_bound(np.array([-8.0]), ref[:1]) > E.SIG_ULPS * 2.0 ** -23 * ref[:1]).all()


def test_draws_cover_every_weight_element():
    for fam in E.FAMILIES:
        P = [E.params(d, fam) for d in range(E.N_DRAWS)]
        for name, shp in E.SHAPES.items():
            union = np.zeros(shp, dtype=bool)
            for p in P:
                w = p[name + ".weight"]
                assert set(np.unique(w)) <= {-1.0, 0.0, 1.0}
                k = E.nnz(w)
                assert (k >= 4).all() and (k <= 5).all(), f"{name}: {k} non-zeros per output channel"
                union |= w != 0
            assert union.all(), f"{name} ({fam}): {union.size - union.sum()} elements are zero in every draw"
    assert any((E.params(d, "M")["masker.0.weight"] < 0).any() for d in range(E.N_DRAWS))


# ---- the reference restates the model ----
def test_reference_agrees_with_the_oracle_on_ordinary_weights():
    n = 2
    rs = np.random.RandomState(5)
    pc = {k: v.double() for k, v in orc.seeded_params(orc.critic_shapes(), 11).items()}
    pm = {k: v.double() for k, v in orc.seeded_params(orc.masker_shapes(), 12).items()}
    A = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    B = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    a, b = A / 255.0, B / 255.0
    nchw = lambda x: torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
    p = {k: v.numpy() for k, v in list(pc.items()) + list(pm.items())}
    with torch.no_grad():
        _, emb = orc.critic_apply(pc, nchw(a), collect=True)
        Z, al = orc.masker_apply(pm, nchw(a), emb, return_all=True)
    e0, _, _ = E.features0(a, p)
    np.testing.assert_allclose(e0, nhwc(emb[0]), rtol=0, atol=1e-12)
    r = E.mask_head(a, nhwc(al["o0"]), p, lrelu=lambda v: np.where(v > 0, v, 0.01 * v))
    np.testing.assert_allclose(r["h"], nhwc(al["hm"]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["Z"], Z[:, 0].numpy(), rtol=0, atol=1e-12)
    z = Z[:, 0].numpy()
    m = E.mix(a, b, z, 1)
    zz = z[..., None]
    np.testing.assert_allclose(m[:n], a * (1 - zz) + zz * b, rtol=0, atol=1e-15)       # main.py:395,406 as oracle.phase2_loss writes them
    np.testing.assert_allclose(m[n:], b * (1 - zz) + zz * a, rtol=0, atol=1e-15)
    with torch.no_grad():
        _, emb_r = orc.critic_apply(pc, nchw(m), collect=True)
    np.testing.assert_allclose(E.features0(m, p)[0], nhwc(emb_r[0]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(E.zpart(z), np.stack((np.abs(z).reshape(n, -1).sum(1), (z ** 2).reshape(n, -1).sum(1)), 1), rtol=1e-14)


# ---- order independence shown: torch's float32 operators give the float64 numbers ----
def t32(x):
    return torch.from_numpy(np.ascontiguousarray(x)).float()


def torch_features0(x, p):
    pre = F.relu(F.conv2d(t32(x).permute(0, 3, 1, 2), t32(p["features.0.weight"]), t32(p["features.0.bias"]), padding=1))
    e, idx = F.max_pool2d(pre, 2, return_indices=True)
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
    pos = (idx // 64 - 2 * yy) * 2 + (idx % 64 - 2 * xx)
    nib = torch.where(e > 0, pos, torch.full_like(pos, 15)).permute(0, 2, 3, 1).numpy().astype(np.uint32)
    am = np.zeros(nib.shape[:3] + (1,), dtype=np.uint32)
    for ch in range(8):
        am[..., 0] |= nib[..., ch] << np.uint32(4 * ch)
    assert e.dtype == torch.float32
    return e.permute(0, 2, 3, 1).numpy(), am


def torch_mask_head(x, o0, p):
    up = F.interpolate(t32(o0).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    pre = F.conv2d(torch.cat((t32(x).permute(0, 3, 1, 2), up), 1), t32(p["masker.0.weight"]), t32(p["masker.0.bias"]), padding=1)
    h = F.leaky_relu(pre, 0.01)
    logit = F.conv2d(h, t32(p["masker.2.weight"]), t32(p["masker.2.bias"]), padding=1)
    assert logit.dtype == torch.float32
    return pre.permute(0, 2, 3, 1).numpy(), h.permute(0, 2, 3, 1).numpy(), logit[:, 0].numpy()


def test_float32_torch_evaluation_is_bit_identical(fix):
    for d in range(0, E.N_DRAWS, 5):
        f = fix[d]
        a, b = E.u8_values(f["A"]), E.u8_values(f["B"])
        za, zb, zz = t32(a), t32(b), t32(f["Zin"])[..., None]
        m32 = torch.cat((za * (1 - zz) + zz * zb, zb * (1 - zz) + zz * za)).numpy()
        assert m32.dtype == np.float32 and np.array_equal(m32.astype(np.float64), f["mix1"]), f"draw {d}: mix"
        for k, x in (("u8", a), ("f32", f["F"]), ("mix", f["mix1"])):
            e, am = torch_features0(x, f["pP"])
            assert np.array_equal(e.astype(np.float64), f["e0_" + k]) and np.array_equal(am, f["am0_" + k]), f"draw {d}: features.0 on {k}"
        for fam in E.FAMILIES:
            for k, x in (("u8", a), ("f32", f["F"])):
                r = f["mh_" + k + fam]
                pre, h, logit = torch_mask_head(x, f["o0" + fam], f["p" + fam])
                assert np.array_equal(pre.astype(np.float64), r["pre"]), f"draw {d} {fam} {k}: masker.0"
                assert np.array_equal(h.astype(np.float64), r["h"]), f"draw {d} {fam} {k}: h"
                if fam == "P":
                    assert np.array_equal(logit.astype(np.float64), r["logit"]), f"draw {d} P {k}: logit"
                else:
                    assert (np.abs(logit - r["logit"]) <= 146 * E.U * r["S"]).all(), f"draw {d} M {k}: logit bound"


# ---- the fixture reacts to the planted mutations ----
def compared(f, mut=None, groups=("mix", "enc", "head", "m2")):
    """The tensors the GPU tests compare (those of `groups`), recomputed from the fixture's inputs with `mut` planted in the reference."""
    a, b = E.u8_values(f["A"]), E.u8_values(f["B"])
    out = {}
    if "mix" in groups:
        out["mix1"] = E.mix(a, b, f["Zin"], 1, mut)
    if "enc" in groups:
        for k, x in (("u8", a), ("f32", f["F"]), ("mix", f["mix1"])):
            out["e0_" + k], out["am0_" + k], _ = E.features0(x, f["pP"], mut)
    if "head" in groups:
        for fam in E.FAMILIES:
            for k, x in (("u8", a), ("f32", f["F"])):
                r = E.mask_head(x, f["o0" + fam], f["p" + fam], mut)
                out[f"h_{k}{fam}"], out[f"Z_{k}{fam}"] = r["h"], r["Z"]
    if "m2" in groups:
        out["Z_m2"] = E.masker2(f["hin"], f["pP"], mut)[2]
    return out


def test_compared_restates_the_fixture(fix):
    f = fix[0]
    c = compared(f)
    assert np.array_equal(c["mix1"], f["mix1"]) and np.array_equal(c["e0_mix"], f["e0_mix"]) and np.array_equal(c["am0_u8"], f["am0_u8"])
    assert np.array_equal(c["h_u8M"], f["mh_u8M"]["h"]) and np.array_equal(c["Z_f32P"], f["mh_f32P"]["Z"]) and np.array_equal(c["Z_m2"], f["m2"]["Z"])


EXPECT = {      # mutation -> tensors that must move in at least one of MUT_DRAWS (each is compared by a GPU test)
    "tie_last": ("am0_u8", "am0_f32", "am0_mix"),
    "halo_col": ("e0_u8", "e0_f32", "e0_mix", "h_u8P", "h_f32M", "Z_m2"),
    "halo_row": ("e0_u8", "e0_f32", "e0_mix", "h_u8P", "h_f32M", "Z_m2"),
    "up_shift": ("h_u8P", "h_u8M", "h_f32P", "h_f32M", "Z_u8P"),
    "swap_rb": ("e0_u8", "e0_f32", "mix1", "h_u8P", "h_f32M"),
    "pixel_shift": ("e0_u8", "e0_f32", "mix1", "h_u8P", "h_f32M"),
    "inject_swapped": ("mix1",),
    "cat_order": ("h_u8P", "h_u8M", "h_f32P", "h_f32M"),
}


GROUP_OF = {"mix": ("mix1",), "enc": ("e0_", "am0_"), "head": ("h_", "Z_u8", "Z_f32"), "m2": ("Z_m2",)}


@pytest.mark.parametrize("mut", E.MUTATIONS)
def test_planted_reference_mutation_is_seen(fix, mut):
    assert set(EXPECT) == set(E.MUTATIONS)
    moved = set()
    groups = {g for g, keys in GROUP_OF.items() if any(k.startswith(keys) for k in EXPECT[mut])}
    for d in MUT_DRAWS:
        base, m = compared(fix[d], None, groups), compared(fix[d], mut, groups)
        moved |= {k for k in base if not np.array_equal(base[k], m[k])}
        if mut == "tie_last":                                  # a tie picks an EQUAL value: only the argmax words can move
            assert moved <= {"am0_u8", "am0_f32", "am0_mix"}, moved
    missing = [k for k in EXPECT[mut] if k not in moved]
    assert not missing, f"{mut}: {missing} do not move in any of the draws {MUT_DRAWS}"


def test_fullbyte_frames_hold_every_value_at_every_byte_position():
    x = E.frames_fullbyte(2).reshape(2, 1024, 12)
    for i in range(2):
        for p in range(12):
            assert len(np.unique(x[i, :, p])) == 256
