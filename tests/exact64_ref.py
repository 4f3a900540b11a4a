"""Float64 reference of the 64x64 forward layers on DYADIC frames and masks, for the exact-arithmetic tests of the 64x64 kernels
(tests/test_exact64_host.py on the CPU, tests/test_gpu_exact64_forward.py on the GPU).  The 32x32-and-smaller layers are
tests/exact_ref.py's; this file follows it and reuses its weight pattern, biases, pooling and upsampling.  numpy only.

Layers (NHWC; layer order of oracle/hourglass_ref.py):
  frames [n,64,64,3] -features.0, ReLU, pool-> e0 [n,32,32,8] + am0 (argmax nibbles, [n,32,32,1])
  mix: replaced = A (1 - Z) + Z B, injected = B (1 - Z) + Z A; zpart = per-image (sum |Z|, sum Z^2)
  h [n,64,64,16] = LeakyReLU_0.01(masker.0(cat(frames, up2(o0 [n,32,32,8]))));  Z [n,64,64] = sigmoid(masker.2(h))

What is exact (test_exact64_host.py asserts each fact on the CPU):
  * a uint8 loader computes b * (1.f / 255.f) in fp32: exactly 0 and 1 for b in {0, 255}; other bytes are not dyadic;
  * fp32 frames are k/4 (k in 0..4), Z inputs of the mixes are multiples of 1/4 in [0, 1], so av (1 - z) + z bv is exact under any
    contraction; weights are sparse and +-1, biases multiples of 1/4, every sum of absolute terms stays below 512: e0, the mixes and
    masker.0's pre-activation are exact in fp32 in any summation order;
  * LeakyReLU is ONE fp32 multiply on the negative branch: h = float32(float32(0.01) * float32(v)) bit for bit -- but not dyadic.
Hence two FAMILIES of mask head draws:
  P  masker.0 weights +1, biases >= 0, o0 >= 0: every pre-activation is >= 0, h is dyadic, masker.2's logit is exact and Z is
     within the sigmoid bound |Z - ref| <= 4 * 2^-23 * ref (SIG_ULPS);
  M  mixed signs, at least a quarter of h on the negative branch: h is compared bit for bit with the rule above; masker.2 then sums
     145 terms (144 products with +-1 / 0, exact, and the bias) of which the negative-branch ones are not dyadic: 145 additions in
     any order and one output rounding, |logit - ref| <= 146 * 2^-24 * S with S the per-pixel sum of the absolute terms on the
     reference's fp32 h, and |Z - sigmoid(ref)| <= 0.25 * that + 4 * 2^-23 * sigmoid(ref) (sigmoid' <= 1/4).
The sigmoid bound is derived for the kernels' 1 / (1 + __expf(-x)): the argument x * log2(e) carries the constant's and the
product's rounding (1.22 * 2^-24 relative, |x| times that in the result), v_exp_f32 1 ulp (2 * 2^-24), the add and the correctly
rounded division 2^-24 each, and the error of e^-x reaches Z scaled by e^-x / (1 + e^-x) <= 1: (1.22 |x| + 4) * 2^-24 <= 4 * 2^-23
for x >= -LOGIT_MIN_ABS = -3.25 (and for every x >= 0); check_exactness64 asserts that range.  sig_bound() is the same derivation
without the range, for logits the fixture does not choose (the fused decoder + mask head test, the full-byte case).

The FULL-BYTE case (not exact): frames over all 256 byte values, each at each of the 12 byte positions of a 4-pixel group -- the
{0, 255} frames cannot see a wrong byte mask or shift.  The reference takes float32(b) * float32(1/255) as input VALUES and goes on
in float64; a conv output with k non-zero +-1 weights is k additions of exact products (the bias included) and rounds at most k
times on partial sums below S: |got - ref| <= (k + 2) * 2^-24 * S."""
import numpy as np

import exact_ref as X
from exact_ref import BIASES, LIMIT, P_PLUS, pool, up, weight_mask

N_DRAWS = 36                                   # masker.2's stride (144 / 4): the largest of the three layers' strides
SHAPES = {"features.0": (8, 3, 3, 3), "masker.0": (16, 11, 3, 3), "masker.2": (1, 16, 3, 3)}         # fan-in 27, 99, 144
FAMILIES = ("P", "M")
P_PLUS_0 = P_PLUS["features.3"]                # features.0 sits in front of a ReLU like features.3
P_PLUS_M2 = 0.85                               # masker.2: mostly +1, so that few logits fall below -LOGIT_MIN_ABS
LOGIT_MIN_ABS = 3.25
SIG_ULPS = 4.0                                 # in units of 2^-23 * ref
U = 2.0 ** -24
FP32_QUANTA = 2.0 ** 22                        # fp32 holds 2^24 quanta exactly: the chained references below stay 4x under it
N_DISTINCT = 8                                 # a large batch is 8 distinct images repeated in a non-periodic order
# Seeds of a draw: base + draw + 1000 * attempt, attempt 0 except for the draws listed here, whose attempt-0 tensors miss one of
# check_exactness64's conditions (found once by running it at n = 1, 3, 8; test_exact64_host.py asserts the conditions again).
ATTEMPT = {5: 1, 17: 1, 18: 1, 30: 2, 34: 1}
MUTATIONS = ("tie_last", "halo_col", "halo_row", "up_shift", "swap_rb", "pixel_shift", "inject_swapped", "cat_order")
S255 = np.float32(1.0) / np.float32(255.0)
SLOPE = np.float32(0.01)


def _rs(base, draw):
    return np.random.RandomState(base + draw + 1000 * ATTEMPT.get(draw, 0))


def params(draw, fam):
    """name -> float64 array (reference OIHW convention) of features.0, masker.0 (family `fam`) and masker.2; features.0 and masker.2
    are the same in both families."""
    rs = _rs(17000, draw)
    p = {}

    def layer(name, plus, biases):
        shp = SHAPES[name]
        p[name + ".weight"] = np.where(rs.rand(*shp) < plus, 1.0, -1.0) * weight_mask(name, shp, draw)
        p[name + ".bias"] = np.asarray(biases)[rs.randint(0, len(biases), size=shp[0])]
    layer("features.0", P_PLUS_0, BIASES)
    layer("masker.2", P_PLUS_M2, BIASES)
    if fam == "M":
        rs.rand(1000)                          # another stretch of the stream
        layer("masker.0", 0.5, BIASES)
    else:
        layer("masker.0", 2.0, [b for b in BIASES if b >= 0])
    return p


def _patches(rs, x, draw, vals_of):
    """Flat patches at 8-aligned positions as exact_ref.dyadic_e0 (16x16 blocks here are 8x8 pooled): whole pool windows tie."""
    n = x.shape[0]
    for img, side in (((draw + 1) % n, 16), (draw % n, (32, 48, 64)[draw % 3])):
        y0, x0 = (8 * rs.randint(0, (64 - side) // 8 + 1, size=2)).tolist()
        x[img, y0:y0 + side, x0:x0 + side, :] = vals_of(rs)
    return x


def frames_u8(draw, n, which="A"):
    """uint8 [n,64,64,3] in {0, 255}."""
    rs = _rs({"A": 19000, "B": 21000}[which], draw)
    x = (rs.rand(n, 64, 64, 3) < 0.5).astype(np.uint8) * np.uint8(255)
    return _patches(rs, x, draw, lambda r: np.array([255, 0, 255], dtype=np.uint8)[r.permutation(3)])


def frames_f32(draw, n):
    """float64 [n,64,64,3]: k/4, k in 0..4."""
    rs = _rs(23000, draw)
    x = rs.randint(0, 5, size=(n, 64, 64, 3)) / 4.0
    return _patches(rs, x, draw, lambda r: np.array([1.0, 0.25, 0.75])[r.permutation(3)])


def frames_fullbyte(n):
    """uint8 [n,64,64,3]: byte position p (0..11) of 4-pixel group g of image i holds (g + 37 p + 101 i) mod 256 -- every value at every position."""
    i, g, p = np.meshgrid(np.arange(n), np.arange(1024), np.arange(12), indexing="ij")
    return ((g + 37 * p + 101 * i) % 256).astype(np.uint8).reshape(n, 64, 64, 3)


def u8_values(x):
    """What a uint8 loader makes of the bytes: float32(b) * float32(1/255), as float64."""
    return (x.astype(np.float32) * S255).astype(np.float64)


def o0_dyadic(draw, n, fam):
    """float64 [n,32,32,8], multiples of 1/4: family P in {0, 1/4}, family M in {-1/4, 0, 1/4} (small, so that the
    logits stay in the range of the sigmoid bound)."""
    rs = _rs(25000 if fam == "P" else 27000, draw)
    if fam == "P":
        return (rs.rand(n, 32, 32, 8) < 0.6) / 4.0
    return rs.randint(-1, 2, size=(n, 32, 32, 8)) / 4.0


def z_dyadic(draw, n):
    """float64 [n,64,64] in {0, 1/4, 1/2, 3/4, 1}."""
    return _rs(29000, draw).randint(0, 5, size=(n, 64, 64)) / 4.0


def h_dyadic(draw, n):
    """float64 [n,64,64,16] in {-1/4, 0, 1/4, 1/2}: masker.2's input when the layer is tested on its own (any sum of four +-h and a
    bias stays inside [-2.5, 2.5])."""
    return _rs(31000, draw).randint(-1, 3, size=(n, 64, 64, 16)) / 4.0


def big_order(n):
    """Image i of a batch of n > 8 is distinct image big_order(n)[i]: the first 8 in order, then a fixed random sequence."""
    idx = np.random.RandomState(4242).randint(0, N_DISTINCT, size=n)
    idx[:N_DISTINCT] = np.arange(N_DISTINCT)
    return idx


# ---- layers (float64; `mut` plants one of MUTATIONS) ----
def _image(x, mut):
    if mut == "swap_rb":
        x = x[..., ::-1]
    if mut == "pixel_shift":                                   # pixel j of a 4-pixel group read from pixel j + 1 of that group
        n, h, w, c = x.shape
        x = x.reshape(n, h, w // 4, 4, c)[:, :, :, [1, 2, 3, 0], :].reshape(n, h, w, c)
    return x


def conv3x3(x, w, b, mut=None):
    """x NHWC, w OIHW, pad 1, term by term over the non-zero weights (any weights give the right sum)."""
    n, h, wd, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    if mut == "halo_col":
        xp[:, :, 0, :] = xp[:, :, 1, :]                        # halo column 0 taken from column 1 (must be zero)
    if mut == "halo_row":
        xp[:, -1, :, :] = xp[:, -2, :, :]                      # the halo row below the image taken from the last row
    xp = np.ascontiguousarray(xp.transpose(3, 0, 1, 2))
    out = np.zeros((w.shape[0], n, h, wd)) + np.reshape(b, (-1, 1, 1, 1))
    for o, c, ky, kx in np.argwhere(w != 0):
        out[o] += w[o, c, ky, kx] * xp[c, :, ky:ky + h, kx:kx + wd]
    return np.ascontiguousarray(out.transpose(1, 2, 3, 0))


def features0(x, p, mut=None):
    """x: frame or mix VALUES [n,64,64,3] -> e0 [n,32,32,8], am0 uint32 [n,32,32,1], the pool windows [n,32,32,8,4]."""
    pre = conv3x3(_image(x, mut), p["features.0.weight"], p["features.0.bias"], mut)
    return pool(np.maximum(pre, 0.0), mut)


def mix(a, b, z, inject, mut=None):
    """a, b: frame values [n,64,64,3], z [n,64,64] -> [n or 2n,64,64,3]: replaced | injected."""
    a, b = _image(a, mut), _image(b, mut)
    if mut == "inject_swapped":
        a, b = b, a
    zz = z[..., None]
    rep = a * (1.0 - zz) + zz * b
    return np.concatenate((rep, b * (1.0 - zz) + zz * a)) if inject else rep


def zpart(z):
    """[n,2]: per-image (sum |Z|, sum Z^2) in float64."""
    return np.stack((np.abs(z).sum((1, 2)), (z * z).sum((1, 2))), axis=1)


def cat_in(x, o0, mut=None):
    u = up(o0, 2)
    if mut == "up_shift":                                      # the upsampled map one pixel to the right, zeros entering at column 0
        u = np.concatenate((np.zeros_like(u[:, :, :1]), u[:, :, :-1]), axis=2)
    return np.concatenate((u, _image(x, mut)) if mut == "cat_order" else (_image(x, mut), u), axis=-1)


def lrelu32(pre):
    """The kernels' LeakyReLU on an fp32-exact pre-activation: the value itself, or ONE fp32 multiply by float32(0.01)."""
    v = pre.astype(np.float32)
    return np.where(v > 0, v, SLOPE * v).astype(np.float64)


def masker0(x, o0, p, mut=None, lrelu=lrelu32):
    """-> pre [n,64,64,16] (float64, exact) and h = lrelu32(pre) (fp32 values as float64).  (lrelu: another LeakyReLU, for the
    comparison with the oracle on ordinary weights, where pre is no fp32 number.)"""
    pre = conv3x3(cat_in(x, o0, mut), p["masker.0.weight"], p["masker.0.bias"], mut)
    return pre, lrelu(pre)


def masker2(h, p, mut=None):
    """-> logit [n,64,64] (float64 on the given h), S = per-pixel sum of the absolute terms, Z = sigmoid(logit)."""
    w, b = p["masker.2.weight"], p["masker.2.bias"]
    logit = conv3x3(h, w, b, mut)[..., 0]
    S = conv3x3(np.abs(h), np.abs(w), np.abs(b))[..., 0]
    return logit, S, 1.0 / (1.0 + np.exp(-logit))


def mask_head(x, o0, p, mut=None, lrelu=lrelu32):
    r = {}
    r["pre"], r["h"] = masker0(x, o0, p, mut, lrelu)
    r["logit"], r["S"], r["Z"] = masker2(r["h"], p, mut)
    r["zpart"] = zpart(r["Z"])
    return r


def abs_sum(x, w, b):
    return conv3x3(np.abs(x), np.abs(w), np.abs(b))


# ---- bounds ----
def sig_bound(logit, ref):
    """|Z - ref| of 1 / (1 + __expf(-x)) with an exact x (module docstring): family P's 4 * 2^-23 * ref wherever x >= -3.25."""
    return np.maximum(SIG_ULPS * 2.0 ** -23, (1.22 * np.maximum(-logit, 0.0) + 4.0) * U) * ref + 2.0 ** -126     # (below fp32's normal range: flushed)


def z_bound(r, exact_h):
    """Bound of |Z - r['Z']| for a kernel whose h equals r['h'] bit for bit: exact_h (family P, h dyadic) the sigmoid bound alone."""
    sb = SIG_ULPS * 2.0 ** -23 * r["Z"]
    return sb if exact_h else 0.25 * 146 * U * r["S"] + sb


ZPART_DEPTH = 40


def zpart_bound(z):
    """|zpart - float64 sums of the kernel's OWN fp32 Z|, from the kernels' summation: a thread adds its own pixels one after the other (at
    most 16: 4096 pixels of an image on 256 threads), wave_sum is a 6-level butterfly, the waves of a workgroup (at most 16) are added one
    after the other, and the rows of an image are summed here in float64.  So every element passes through at most 16 + 6 + 16 = 38
    additions, and its square is rounded once: (1 + 2^-24)^39 - 1 < 40 * 2^-24 relative to the sum of the (non-negative) terms.  One
    average pixel is 1/4096 of the sum, a hundred times that.  (Dyadic Z, the mixes: zpart is exact instead.)"""
    return ZPART_DEPTH * U * zpart(z)


def zpart_ref_bound(z_ref, zb):
    """|sums of a Z within zb of z_ref - zpart(z_ref)|: sum zb for sum |Z| (Z > 0), sum (2 z_ref + zb) zb for sum Z^2."""
    return np.stack((zb.sum((1, 2)), ((2 * z_ref + zb) * zb).sum((1, 2))), axis=1)


def nnz(w):
    """Non-zero weights of each output channel."""
    return (w != 0).reshape(w.shape[0], -1).sum(1)


# ---- the fixture of one draw ----
INPUTS = ("A", "B", "F", "Zin", "hin", "o0P", "o0M")


def inputs(draw, n):
    """name -> input tensor of one (draw, n <= 8): uint8 frames A / B, fp32 frames F, the mixes' mask Zin, masker.2's own input hin,
    and o0 of the two families."""
    f = {"A": frames_u8(draw, n, "A"), "B": frames_u8(draw, n, "B"), "F": frames_f32(draw, n), "Zin": z_dyadic(draw, n), "hin": h_dyadic(draw, n)}
    for fam in FAMILIES:
        f["o0" + fam] = o0_dyadic(draw, n, fam)
    return f


def inputs_fullbyte(draw, n=2):
    """The inputs of `draw` with the full-byte frames in place of A and B (B: the images of A in reverse order, bytes complemented)."""
    f = inputs(draw, n)
    f["A"] = frames_fullbyte(n)
    f["B"] = (255 - f["A"][::-1]).astype(np.uint8)
    return f


GROUPS = ("mix", "enc", "head", "m2")


def evaluate(inp, pP, pM, mut=None, exact=True, groups=GROUPS, fams=FAMILIES):
    """The inputs and the reference tensors of `groups` (mix: mix1, zpart_in; enc: e0 / am0 / win of the three sources; head: mh_<src><fam>
    of `fams`; m2: masker.2 on hin).  exact=False (the full-byte case): LeakyReLU in float64, since masker.0's pre-activation is no fp32
    number there."""
    f = dict(inp, pP=pP, pM=pM)
    lrelu = lrelu32 if exact else (lambda v: np.where(v > 0, v, float(SLOPE) * v))
    a, b = u8_values(f["A"]), u8_values(f["B"])
    if "mix" in groups:
        f["mix1"] = mix(a, b, f["Zin"], 1, mut)
        f["zpart_in"] = zpart(f["Zin"])
    if "enc" in groups:
        for k, x in (("u8", a), ("f32", f["F"]), ("mix", mix(a, b, f["Zin"], 1, mut if mut == "inject_swapped" else None))):
            f["e0_" + k], f["am0_" + k], f["win_" + k] = features0(x, pP, mut)
    if "head" in groups:
        for fam in fams:
            f["mh_u8" + fam] = mask_head(a, f["o0" + fam], f["p" + fam], mut, lrelu)
            f["mh_f32" + fam] = mask_head(f["F"], f["o0" + fam], f["p" + fam], mut, lrelu)
    if "m2" in groups:
        f["m2"] = dict(zip(("logit", "S", "Z"), masker2(f["hin"], pP, mut)))
        f["m2"]["zpart"] = zpart(f["m2"]["Z"])
    return f


def fixture(draw, n):
    """Everything the tests of one (draw, n <= 8) need, inputs and references, computed once."""
    f = evaluate(inputs(draw, n), params(draw, "P"), params(draw, "M"))
    f["draw"], f["n"] = draw, n
    return f


def critic_chain(xparams, e0):
    """exact_ref's chain (features.3 .. pred, o4) on an e0 of THIS file, for the one-launch critic forward.  Such an e0 reaches 5.5, not
    exact_ref's 1/2, so the sums leave the fp16 range -- but every tensor of that kernel is fp32: asserted here is that every layer's sum
    of absolute terms stays below 2^22 quanta (1/4; 1/16 behind crit.1, 2^-10 for the logit)."""
    r = X.forward(xparams, e0)
    for layer, s in X.abs_sums(r, xparams, e0).items():
        q = {"crit.1": 0.0625, "crit.4": 2.0 ** -10}.get(layer, 0.25)
        assert s.max() / q < FP32_QUANTA, f"{layer}: sum of absolute terms {s.max()}"
    return r


DEC_SMALL = 2.0 ** -6


def decoder(pm, e0, e1, e2, e3, o4, a=lambda v: v):
    """exact_ref.forward's decoder lines on given inputs (a = np.abs: the sums of absolute terms)."""
    W = lambda k: (a(pm[k + ".weight"]), a(pm[k + ".bias"]))
    cat = lambda skip, low, f: np.concatenate((a(skip), X.up(a(low), f)), axis=-1)
    r = {}
    r["o3"] = X.conv3x3(cat(e3, o4.reshape(-1, 1, 1, 32), 4), *W("dec_model.3"))
    r["o2"] = X.conv3x3(cat(e2, r["o3"], 2), *W("dec_model.2"))
    r["o1"] = X.conv3x3(cat(e1, r["o2"], 2), *W("dec_model.1"))
    r["o0"] = X.conv3x3(cat(e0, r["o1"], 2), *W("dec_model.0"))
    return r


def dec_mask_fixture(draw, n, xparams, scale=1.0, fullbyte=False):
    """The fused decoder + mask head: exact_ref's e0 .. o4 of (draw, n) times `scale` as x_<name>, the decoder's o3 .. o0 on them as
    references (scale 1: exact_ref's own, asserted), and the mask head of family M on the uint8 frames of this file and THAT o0 (as o0M).
    scale 1: |o0| reaches a few hundred -- masker.0's sums leave the fp16 range but stay below 2^22 quanta (asserted), so h keeps its
    bit-exact rule; most logits are far outside [-3.25, 16], Z's bound takes sig_bound() and most of Z is saturated: masker.2 is checked
    only weakly there.  scale DEC_SMALL = 2^-6 (the decoder is linear: its inputs are then multiples of 2^-8, the biases stay): o0 stays
    of the biases' size, and the logits inside (-10, 10) are at least a tenth in every draw (asserted here) and at least a quarter in all
    draws but one (draw 1, whose masker.2 weights are all +1; test_exact64_host.py): the case that checks masker.2 and the sigmoid in this form.  fullbyte: the full-byte frames as x; h and Z then get fullbyte_bounds on that o0."""
    q0 = 0.25 * scale
    xin = {k: v * scale for k, v in dict(X.forward(xparams, X.dyadic_e0(draw, n)), e0=X.dyadic_e0(draw, n)).items() if k in ("e0", "e1", "e2", "e3", "o4")}
    pm = xparams[1]
    r = decoder(pm, **xin)
    if scale == 1.0:
        full = X.forward(xparams, xin["e0"])
        assert all(np.array_equal(r[k], full[k]) for k in r)
    for k, s in decoder(pm, a=np.abs, **xin).items():
        assert s.max() / q0 < FP32_QUANTA and np.array_equal(r[k] / q0, np.round(r[k] / q0)), k
    inp = dict(inputs_fullbyte(draw, n) if fullbyte else inputs(draw, n), o0M=r["o0"])
    f = evaluate(inp, params(draw, "P"), params(draw, "M"), exact=not fullbyte, groups=("head",), fams=("M",))
    q, m = f["pM"], f["mh_u8M"]
    s0 = abs_sum(cat_in(u8_values(f["A"]), r["o0"]), q["masker.0.weight"], q["masker.0.bias"])
    assert s0.max() / q0 < FP32_QUANTA and m["S"].max() / q0 < FP32_QUANTA
    if not fullbyte:
        assert np.array_equal(m["pre"].astype(np.float32).astype(np.float64), m["pre"]) and np.array_equal(m["pre"] / q0, np.round(m["pre"] / q0))
    f.update({"x_" + k: v for k, v in list(xin.items()) + list(r.items())})
    if fullbyte:
        f["bounds"] = fullbyte_bounds(f, groups=("head",), fams=("M",))
        f["Z_bound"] = f["bounds"]["ZM"]
    else:
        f["Z_bound"] = 0.25 * 146 * U * m["S"] + sig_bound(m["logit"], m["Z"])
    f["unsaturated"] = float((np.abs(m["logit"]) < 10).mean())
    if scale != 1.0:
        assert f["unsaturated"] >= 0.1, f"only {f['unsaturated']:.2f} of the logits inside (-10, 10)"
    return f


def image_of(inp, i):
    """The inputs restricted to image i (a batch of one)."""
    return {k: inp[k][i:i + 1] for k in INPUTS}


def fullbyte_bounds(f, groups=GROUPS, fams=FAMILIES):
    """Bounds of the full-byte case for a run f = evaluate(inputs_fullbyte(..), .., exact=False): name -> array shaped like the
    tensor.  pre-activations: (k + 2) * 2^-24 * S per output channel (module docstring); pooled maxima: the largest bound of the window
    (each of the four values moves by at most its own); the mixes: two products, one sum, k = 2; features.0 on the mixes: the
    mixes' own error through the +-1 weights in addition; h: LeakyReLU is 1-Lipschitz and rounds once on the negative branch; the
    logit: h's bounds through masker.2's +-1 weights and its own 146 * 2^-24 * S; Z: sigmoid' <= 1/4 and sig_bound."""
    pP = f["pP"]
    a, b = u8_values(f["A"]), u8_values(f["B"])
    out = {}
    zz = f["Zin"][..., None]
    s_mix = np.concatenate((a * (1 - zz) + zz * b, b * (1 - zz) + zz * a))              # all terms are >= 0: S is the value
    out["mix1"] = 4 * U * s_mix
    w0, b0 = pP["features.0.weight"], pP["features.0.bias"]
    k0 = nnz(w0)
    if "enc" not in groups:
        return dict(out, **_head_bounds(f, a, fams))

    def pooled(bound):
        n, h, w, c = bound.shape
        return bound.reshape(n, h // 2, 2, w // 2, 2, c).max((2, 4))
    for k, x, extra in (("u8", a, None), ("mix", f["mix1"], out["mix1"])):
        pre_b = (k0 + 2) * U * abs_sum(x, w0, b0)
        if extra is not None:
            pre_b = pre_b + abs_sum(extra, w0, 0 * b0)
        out["e0_" + k] = pooled(pre_b)
    return dict(out, **_head_bounds(f, a, fams)) if "head" in groups else out


def _head_bounds(f, a, fams):
    out = {}
    for fam in fams:
        q = f["p" + fam]
        r = f["mh_u8" + fam]
        w, bb = q["masker.0.weight"], q["masker.0.bias"]
        hb = (nnz(w) + 2) * U * abs_sum(cat_in(a, f["o0" + fam]), w, bb) + U * np.abs(r["h"])
        w2, b2 = q["masker.2.weight"], q["masker.2.bias"]
        lb = abs_sum(hb, w2, 0 * b2)[..., 0] + 146 * U * abs_sum(np.abs(r["h"]) + hb, w2, b2)[..., 0]
        out["h" + fam] = hb
        out["Z" + fam] = 0.25 * lb + sig_bound(r["logit"] - lb, r["Z"]) * (1 + 1e-3)
    return out


def check_exactness64(f):
    """Raises AssertionError unless the fixture satisfies the conditions under which the kernels must reproduce it as the module
    docstring says: (a) fp16 round-trip, (b) absolute sums below 512, (c) quanta and the logit range, (d) density, ties, families."""
    f16 = lambda x: x.astype(np.float16).astype(np.float64)
    quarter = lambda x: np.array_equal(x * 4, np.round(x * 4))
    dense = lambda x: np.count_nonzero(x) >= 0.5 * x.size
    p = f["pP"]
    a, b = u8_values(f["A"]), u8_values(f["B"])
    assert set(np.unique(f["A"])) <= {0, 255} and set(np.unique(f["B"])) <= {0, 255}
    assert set(np.unique(a)) <= {0.0, 1.0}, "(c) bytes 0 / 255 are not exactly 0 / 1"
    assert set(np.unique(f["Zin"])) == {0.0, 0.25, 0.5, 0.75, 1.0}
    tensors = {"F": f["F"], "mix1": f["mix1"], "hin": f["hin"], "e0_u8": f["e0_u8"], "e0_f32": f["e0_f32"], "e0_mix": f["e0_mix"],
               "o0P": f["o0P"], "o0M": f["o0M"], "h(P,u8)": f["mh_u8P"]["h"], "h(P,f32)": f["mh_f32P"]["h"],
               "pre(M,u8)": f["mh_u8M"]["pre"], "pre(M,f32)": f["mh_f32M"]["pre"]}
    for k, x in tensors.items():
        assert np.array_equal(f16(x), x), f"(a) {k} is not fp16-exact"
        assert quarter(x), f"(c) {k} is not a multiple of 1/4"
        assert dense(x), f"(d) {k}: only {np.count_nonzero(x) / x.size:.2f} non-zero"
    assert (f["F"] >= 0).all() and f["F"].max() <= 1 and (f["mix1"] >= 0).all() and f["mix1"].max() <= 1
    for k, x in (("u8", a), ("f32", f["F"]), ("mix", f["mix1"])):
        s = abs_sum(x, p["features.0.weight"], p["features.0.bias"])
        assert s.max() < LIMIT, f"(b) features.0 on {k}: {s.max()}"
        win = f["win_" + k]
        mx = win.max(-1, keepdims=True)
        ties = int((((win == mx).sum(-1) >= 2) & (mx[..., 0] > 0)).sum())
        assert ties >= 20, f"(d) features.0 on {k}: {ties} exact positive ties"
    for fam in FAMILIES:
        q = f["p" + fam]
        for k, x in (("u8", a), ("f32", f["F"])):
            r = f["mh_" + k + fam]
            s = abs_sum(cat_in(x, f["o0" + fam]), q["masker.0.weight"], q["masker.0.bias"])
            assert s.max() < LIMIT, f"(b) masker.0 {fam} on {k}: {s.max()}"
            assert r["S"].max() < LIMIT, f"(b) masker.2 {fam} on {k}: {r['S'].max()}"
            assert np.array_equal(r["pre"].astype(np.float32).astype(np.float64), r["pre"])
            neg = (r["pre"] < 0).mean()
            if fam == "P":
                assert neg == 0, f"(d) family P on {k}: {neg:.3f} of the pre-activations are negative"
                assert np.array_equal(r["h"], r["pre"]) and quarter(r["logit"]), "(c) family P: h and the logit are dyadic"
            else:
                assert neg >= 0.25, f"(d) family M on {k}: only {neg:.3f} of h on the negative branch"
            assert r["logit"].min() >= -LOGIT_MIN_ABS and r["logit"].max() <= 16, \
                f"(c) {fam} on {k}: logits in [{r['logit'].min()}, {r['logit'].max()}]"
    m2 = f["m2"]
    assert m2["S"].max() < LIMIT and quarter(m2["logit"]) and m2["logit"].min() >= -LOGIT_MIN_ABS and m2["logit"].max() <= 16
