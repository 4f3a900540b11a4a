"""Float64 reference of the 32x32-and-smaller forward layers on DYADIC data, for the exact-arithmetic forward tests.

Activations are non-negative multiples of 1/4, weights are sparse and in {-1, +1} (features.6 also +-2, crit.1 +-{1/4, 1/2},
crit.4 +-{1/16, 1/8}), biases are multiples of 1/4, and in every layer the sum of the ABSOLUTE values of all terms stays below
512 = 2048 quanta of 1/4.  Then every partial sum is an exact fp16 and fp32 number whatever the summation order or the matrix
instruction, so a kernel has to reproduce this reference bit for bit in every tensor it writes (check_exactness asserts the
conditions; they are conditions on the reference alone).  numpy only: nothing here imports the GPU package.

Chain (layer order of oracle/hourglass_ref.py: critic_apply from e0 on, then masker_apply up to o0), NHWC:
  e0 [n,32,32,8] -features.3, ReLU, pool-> e1 [n,16,16,8] -features.6-> e2 [n,8,8,8] -features.10-> e3 [n,4,4,16]
  -features.14 (4x4 valid), ReLU-> e4 [n,32] -crit.1, ReLU-> h1 [n,32] -crit.4-> logit [n] -sigmoid-> pred [n]
  e4 -dec_model.4 (1x1)-> o4 [n,32]; o3 = dec_model.3(cat(e3, up4(o4))) [n,4,4,16]; o2 = dec_model.2(cat(e2, up2(o3))) [n,8,8,8];
  o1 = dec_model.1(cat(e1, up2(o2))) [n,16,16,8]; o0 = dec_model.0(cat(e0, up2(o1))) [n,32,32,8]   (decoder trunk linear)
"""
import numpy as np

from oracle.hourglass_ref import critic_shapes, masker_shapes

N_DRAWS = 108                      # dec_model.3's stride (432 / 4): the largest of the layers' strides
# layer -> the magnitudes its non-zero weights take
LAYERS = {
    "features.3": (1.0,), "features.6": (1.0, 1.0, 1.0, 2.0), "features.10": (1.0,), "features.14": (1.0,),
    "crit.1": (0.25, 0.5), "crit.4": (0.0625, 0.125),
    "dec_model.4": (1.0,), "dec_model.3": (1.0,), "dec_model.2": (1.0,), "dec_model.1": (1.0,), "dec_model.0": (1.0,),
}
# share of positive signs: above 1/2 in front of a ReLU, so that at least half of every tensor is non-zero in every draw
P_PLUS = {"features.3": 0.6, "features.6": 0.6, "features.10": 0.6, "features.14": 0.65, "crit.1": 0.65}
BIASES = (0.0, 0.25, -0.25, 0.5, -0.5)
KMAX = 2                           # e0 = k / 4, k in 0..KMAX
LIMIT = 512.0                      # 2048 quanta of 1/4: an fp16 significand holds them exactly
# The seeds of a draw are 7000 / 9000 + draw + 1000 * attempt: the attempt is 0 except for the draws listed here, whose attempt-0
# tensors miss one of check_exactness's conditions (a sum of absolute terms above 512, a logit above 8, a tensor less than half
# non-zero).  Found once by running check_exactness at every batch size the tests use; the tests assert the conditions again.
ATTEMPT = {1: 1, 17: 1, 36: 1, 37: 1, 41: 1, 42: 1, 48: 3, 49: 2, 64: 1, 69: 2, 77: 1, 83: 2, 85: 1, 89: 1, 104: 2}
MUTATIONS = ("tie_last", "up_shift", "halo_col", "swap45")


def weight_mask(key, shape, draw):
    """Non-zero pattern of a layer's weight (reference OIHW / [o][k] shape) in a draw: (flat index + draw + 5 o) % (fan_in / 4) == 0 with
    o the output channel, i.e. four non-zeros per output channel at positions that move from channel to channel; over `stride`
    consecutive draws every element is non-zero exactly once."""
    fan_in = int(np.prod(shape[1:]))
    stride = fan_in // 4
    flat = np.arange(int(np.prod(shape)))
    o = flat // fan_in
    return ((flat + draw + 5 * o) % stride == 0).reshape(shape)


def dyadic_params(draw):
    """(critic, masker) parameter dicts (float64 numpy, the key / shape convention of critic_shapes() / masker_shapes())."""
    rs = np.random.RandomState(7000 + draw + 1000 * ATTEMPT.get(draw, 0))
    out = []
    for shapes in (critic_shapes(), masker_shapes()):
        p = {}
        for key, shp in shapes:
            layer, kind = key.rsplit(".", 1)
            if layer not in LAYERS:                        # features.0, masker.*: not used here, any finite values
                p[key] = rs.uniform(-0.1, 0.1, size=shp)
            elif kind == "weight":
                mags = np.asarray(LAYERS[layer])
                w = np.where(rs.rand(*shp) < P_PLUS.get(layer, 0.5), 1.0, -1.0) * mags[rs.randint(0, len(mags), size=shp)]
                p[key] = w * weight_mask(key, shp, draw)
            else:
                p[key] = np.asarray(BIASES)[rs.randint(0, len(BIASES), size=shp)]
        out.append(p)
    return out[0], out[1]


def dyadic_e0(draw, n):
    """fp16-exact NHWC [n,32,32,8] float64: k/4 with k in 0..4, about half zero.  Image draw % n carries a flat patch (channels
    constant over a block of 16x16 or more at an 8-aligned position), image (draw + 1) % n a flat 8x8 block: whole pool
    windows tie there, through all three pooled stages."""
    rs = np.random.RandomState(9000 + draw + 1000 * ATTEMPT.get(draw, 0))
    k = rs.randint(0, KMAX + 1, size=(n, 32, 32, 8)) * (rs.rand(n, 32, 32, 8) < 0.75)
    e0 = k / 4.0
    for img, side in (((draw + 1) % n, 8), (draw % n, (16, 24, 32)[draw % 3])):   # the large patch last: at n = 1 it stays
        y0, x0 = (8 * rs.randint(0, (32 - side) // 8 + 1, size=2)).tolist()
        vals = rs.randint(0, KMAX + 1, size=8) / 4.0
        vals[rs.randint(0, 8)] = KMAX / 4.0                        # never an all-zero patch
        e0[img, y0:y0 + side, x0:x0 + side, :] = vals
    return e0


# ---- layers (float64; `mut` plants one of MUTATIONS, for the tests that show the fixture reacts to them) ----
def _pad(x, mut):
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    if mut == "halo_col":
        xp[:, :, 0, :] = xp[:, :, 1, :]                    # halo column 0 taken from column 1 (must be zero)
    return xp


def conv3x3(x, w, b, mut=None):
    """x NHWC, w OIHW, pad 1."""
    n, h, wd, _ = x.shape
    xp = _pad(x, mut)
    xp = np.ascontiguousarray(xp.transpose(3, 0, 1, 2))    # channel planes
    out = np.zeros((w.shape[0], n, h, wd)) + np.reshape(b, (-1, 1, 1, 1))
    for o, c, ky, kx in np.argwhere(w != 0):               # term by term: the weights are sparse (any weights give the right sum)
        out[o] += w[o, c, ky, kx] * xp[c, :, ky:ky + h, kx:kx + wd]
    return np.ascontiguousarray(out.transpose(1, 2, 3, 0))


def pool(x, mut=None):
    """2x2 max-pool of relu'd x NHWC -> (pooled, amask uint32 [n,h/2,w/2,c/8], windows [n,h/2,w/2,c,4])."""
    n, h, w, c = x.shape
    win = x.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    idx = win.argmax(-1) if mut != "tie_last" else 3 - win[..., ::-1].argmax(-1)      # numpy's argmax: the first maximum
    pooled = np.take_along_axis(win, idx[..., None], -1)[..., 0]
    nib = np.where(pooled > 0, idx, 15).astype(np.uint32)
    am = np.zeros((n, h // 2, w // 2, c // 8), dtype=np.uint32)
    for ch in range(c):
        am[..., ch // 8] |= nib[..., ch] << np.uint32(4 * (ch % 8))
    return pooled, am, win


def up(x, f, mut=None):
    u = np.repeat(np.repeat(x, f, axis=1), f, axis=2)
    if mut == "up_shift":
        u = np.roll(u, 1, axis=2)
    return u


def enc_stage(x, w, b, mut=None):
    return pool(np.maximum(conv3x3(x, w, b, mut), 0.0), mut)


def forward(params, e0, mut=None):
    pc, pm = params
    W = lambda p, k: (p[k + ".weight"], p[k + ".bias"])
    r = {}
    r["e1"], r["am1"], _ = enc_stage(e0, *W(pc, "features.3"), mut)
    r["e2"], r["am2"], _ = enc_stage(r["e1"], *W(pc, "features.6"), mut)
    r["e3"], r["am3"], _ = enc_stage(r["e2"], *W(pc, "features.10"), mut)
    n = e0.shape[0]
    w14, b14 = W(pc, "features.14")                                           # OIHW [32,16,4,4] on NHWC [n,4,4,16]
    r["e4"] = np.maximum(r["e3"].reshape(n, -1) @ w14.transpose(2, 3, 1, 0).reshape(256, 32) + b14, 0.0)
    r["h1"] = np.maximum(r["e4"] @ pc["crit.1.weight"].T + pc["crit.1.bias"], 0.0)
    r["logit"] = r["h1"] @ pc["crit.4.weight"][0] + pc["crit.4.bias"][0]
    r["pred"] = 1.0 / (1.0 + np.exp(-r["logit"]))
    r["o4"] = r["e4"] @ pm["dec_model.4.weight"][:, :, 0, 0].T + pm["dec_model.4.bias"]
    cat = lambda skip, low, f: np.concatenate((skip, up(low, f, mut)), axis=-1)  # torch.cat((skip, upsampled), 1)
    r["o3"] = conv3x3(cat(r["e3"], r["o4"].reshape(n, 1, 1, 32), 4), *W(pm, "dec_model.3"), mut)
    c2 = cat(r["e2"], r["o3"], 2)
    if mut == "swap45":
        c2[..., [4, 5]] = c2[..., [5, 4]]
    r["o2"] = conv3x3(c2, *W(pm, "dec_model.2"), mut)
    r["o1"] = conv3x3(cat(r["e1"], r["o2"], 2), *W(pm, "dec_model.1"), mut)
    r["o0"] = conv3x3(cat(e0, r["o1"], 2), *W(pm, "dec_model.0"), mut)
    return r


def abs_sums(r, params, e0):
    """layer -> conv(|x|, |w|) + |b| of that layer on the reference's own inputs (no activation)."""
    pc, pm = params
    A = lambda p, k: (np.abs(p[k + ".weight"]), np.abs(p[k + ".bias"]))
    n = e0.shape[0]
    a = np.abs
    cat = lambda skip, low, f: np.concatenate((a(skip), up(a(low), f)), axis=-1)
    w14, b14 = A(pc, "features.14")
    return {
        "features.3": conv3x3(a(e0), *A(pc, "features.3")),
        "features.6": conv3x3(a(r["e1"]), *A(pc, "features.6")),
        "features.10": conv3x3(a(r["e2"]), *A(pc, "features.10")),
        "features.14": a(r["e3"]).reshape(n, -1) @ w14.transpose(2, 3, 1, 0).reshape(256, 32) + b14,
        "crit.1": a(r["e4"]) @ a(pc["crit.1.weight"]).T + a(pc["crit.1.bias"]),
        "crit.4": a(r["h1"]) @ a(pc["crit.4.weight"][0]) + a(pc["crit.4.bias"][0]),
        "dec_model.4": a(r["e4"]) @ a(pm["dec_model.4.weight"][:, :, 0, 0]).T + a(pm["dec_model.4.bias"]),
        "dec_model.3": conv3x3(cat(r["e3"], r["o4"].reshape(n, 1, 1, 32), 4), *A(pm, "dec_model.3")),
        "dec_model.2": conv3x3(cat(r["e2"], r["o3"], 2), *A(pm, "dec_model.2")),
        "dec_model.1": conv3x3(cat(r["e1"], r["o2"], 2), *A(pm, "dec_model.1")),
        "dec_model.0": conv3x3(cat(e0, r["o1"], 2), *A(pm, "dec_model.0")),
    }


def positive_ties(params, e0, r):
    """stage -> number of pool windows whose maximum is positive and taken by two or more of the four elements."""
    pc = params[0]
    out = {}
    for key, src in (("features.3", e0), ("features.6", r["e1"]), ("features.10", r["e2"])):
        _, _, win = enc_stage(src, pc[key + ".weight"], pc[key + ".bias"])
        mx = win.max(-1, keepdims=True)
        out[key] = int((((win == mx).sum(-1) >= 2) & (mx[..., 0] > 0)).sum())
    return out


TENSORS = ("e1", "e2", "e3", "e4", "h1", "o4", "o3", "o2", "o1", "o0")
# quantum of each tensor: 1/4 everywhere except behind crit.1, whose weights are multiples of 1/4 themselves
QUANTUM = {k: 0.25 for k in TENSORS}
QUANTUM["h1"] = 0.0625


def check_exactness(r, params, e0):
    """Raises AssertionError unless the reference run `r` = forward(params, e0) satisfies the conditions under which every kernel
    must reproduce it exactly: (a) fp16 round-trip of every tensor, (b) absolute sums below 512, (c) the quanta, (d) density and ties."""
    f16 = lambda x: x.astype(np.float16).astype(np.float64)
    assert np.array_equal(f16(e0), e0) and (e0 >= 0).all() and np.array_equal(e0 * 4, np.round(e0 * 4))
    for k in TENSORS:
        assert np.array_equal(f16(r[k]), r[k]), f"(a) {k} is not fp16-exact"
        q = r[k] / QUANTUM[k]
        assert np.array_equal(q, np.round(q)), f"(c) {k} is not a multiple of {QUANTUM[k]}"
        assert np.count_nonzero(r[k]) >= 0.5 * r[k].size, f"(d) {k}: only {np.count_nonzero(r[k]) / r[k].size:.2f} non-zero"
    for layer, s in abs_sums(r, params, e0).items():
        assert s.max() < LIMIT, f"(b) {layer}: sum of absolute terms {s.max()} >= {LIMIT}"
    lq = r["logit"] * 1024
    assert np.array_equal(lq, np.round(lq)) and np.abs(r["logit"]).max() <= 8, "(c) logit"
    for key, cnt in positive_ties(params, e0, r).items():
        assert cnt >= 20, f"(d) {key}: {cnt} exact positive ties"
