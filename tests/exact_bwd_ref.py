"""Float64 reference of the BACKWARD of tests/exact_ref.py's chain on dyadic data, for the exact-arithmetic backward tests.

Free inputs: dy_o0 [n,32,32,8] = k/4 with k in -2..2 (about one quarter non-zero), the saved pred = 1/2 for every image, and
dpred in +-{64, 128}, so that d logit = dpred pred (1 - pred) is +-16 or +-32.  With crit.4's 1/16 and crit.1's 1/4 weights every data
gradient is a multiple of 1/4 and every weight gradient a multiple of 1/16 (activations are multiples of 1/4; h1 of 1/16, but it
meets only d logit, a multiple of 16).  When, for every output element, the sum of the ABSOLUTE values of all its terms stays below
2^22 quanta, every partial sum is an exact fp32 number in any order, on any partition of the images over workgroups and slab rows:
a kernel has to reproduce this reference bit for bit (check_exactness_bwd asserts the conditions on the reference alone).
Dropout, where used, has p = 1/2: the keep multiplier is exactly 2.  numpy only.

Everything is NHWC; weight gradients come in the kernels' slab layout: HWIO [ky][kx][ci][co] flat, then the bias gradient; the
head's [features.14 w 8192 (k = (y 4 + x) 16 + c major) | b 32 | crit.1 w 1024 (k-major) | b 32 | crit.4 w 32 | b 1]; dec_model.4's
[w 1024 (k-major) | b 32].  hvec [n,384] as include/cgs_hip.h documents it:
[0,256) dropout(e3) | [256,288) dz4 | [288,320) dh1 | [320,352) dz2 h1 mask | [352] dz2, the rest unused (zero here)."""
import numpy as np

import exact_ref as X

Q_DATA, Q_WEIGHT = 0.25, 0.0625
LIMIT_QUANTA = 2.0 ** 22            # a factor 4 under fp32's 2^24
# the second seeds of the cotangents (as exact_ref.ATTEMPT): draws whose attempt-0 cotangents miss one of check_exactness_bwd's conditions
ATTEMPT_BWD = {}
DROP_DRAWS = (0, 1, 2, 3)           # the group of draws that also runs with Dropout p = 1/2 at all three sites
TARGET_SCALES = (64.0, 128.0)       # |d loss / d pred| of the tail kernels' target modes, by draw parity (one loss_scale per launch)
MUTATIONS = ("tie_last", "up_shift", "halo_col", "swap45", "last_image", "drop_weight")
ENC = (("features.3", 1), ("features.6", 2), ("features.10", 3))
DEC = (("dec_model.0", 0), ("dec_model.1", 1), ("dec_model.2", 2), ("dec_model.3", 3))
DATA = ("dE0", "do1", "dE1", "do2", "dE2", "do3", "dE3", "d_o4", "de4_dec", "de3", "de2", "de1", "de0", "hvec")
SLABS = {"dec_model.0": "g_dec0", "dec_model.1": "g_dec1", "dec_model.2": "g_dec2", "dec_model.3": "g_dec3", "dec_model.4": "g_pw",
         "features.3": "g_enc1", "features.6": "g_enc2", "features.10": "g_enc3", "head": "g_head"}
TENSORS = DATA + tuple(SLABS.values())


def cotangents(draw, n, carry=None):
    """(dy_o0 [n,32,32,8], dpred [n]).  carry: the images that carry non-zero cotangents (default: all); the others get exact zeros."""
    rs = np.random.RandomState(11000 + draw + 1000 * ATTEMPT_BWD.get(draw, 0))
    m = n if carry is None else len(carry)
    k = np.asarray((-2, -1, 1, 2))[rs.randint(0, 4, size=(m, 32, 32, 8))] * (rs.rand(m, 32, 32, 8) < 0.25)
    dp = np.asarray((64.0, 128.0))[rs.randint(0, 2, size=m)] * np.where(rs.rand(m) < 0.5, 1.0, -1.0)
    if carry is None:
        return k / 4.0, dp
    dy, dpred = np.zeros((n, 32, 32, 8)), np.zeros(n)
    dy[list(carry)], dpred[list(carry)] = k / 4.0, dp
    return dy, dpred


def target_dpred(draw, dpred):
    """The cotangent of pred that the tail kernels' target modes derive for this draw: target = (dpred < 0), pred = 1/2 and
    loss_scale S (MSE: 2 S (pred - target)) or S / 2 (BCE: S/2 (pred - target) / (pred (1 - pred))) both give sign(dpred) S."""
    return np.sign(dpred) * TARGET_SCALES[draw % 2]


def standin_masks(draw, n):
    """Dropout multipliers (0 or 2) of the three sites for the CPU tests; the GPU tests export the kernels' own with cgs_dropout_mask."""
    rs = np.random.RandomState(13000 + draw)
    return tuple(2.0 * (rs.rand(*s) < 0.5) for s in ((n, 8, 8, 8), (n, 4, 4, 16), (n, 32)))


def forward(params, e0, masks=None, mut=None):
    """exact_ref.forward with Dropout multipliers masks = (m_e2, m_e3, m_h1) in front of features.10, features.14 and crit.4 (None: none),
    as the training forward applies them: the saved e2 / e3 / h1 are the values BEFORE Dropout, the decoder reads those."""
    if masks is None:
        r = X.forward(params, e0, mut=mut)
        r["e0"] = e0
        return r
    pc, pm = params
    W = lambda p, k: (p[k + ".weight"], p[k + ".bias"])
    n = e0.shape[0]
    r = {"e0": e0}
    r["e1"], r["am1"], _ = X.enc_stage(e0, *W(pc, "features.3"), mut)
    r["e2"], r["am2"], _ = X.enc_stage(r["e1"], *W(pc, "features.6"), mut)
    r["e3"], r["am3"], _ = X.enc_stage(r["e2"] * masks[0], *W(pc, "features.10"), mut)
    w14, b14 = W(pc, "features.14")
    r["e4"] = np.maximum((r["e3"] * masks[1]).reshape(n, -1) @ w14.transpose(2, 3, 1, 0).reshape(256, 32) + b14, 0.0)
    r["h1"] = np.maximum(r["e4"] @ pc["crit.1.weight"].T + pc["crit.1.bias"], 0.0)
    r["logit"] = (r["h1"] * masks[2]) @ pc["crit.4.weight"][0] + pc["crit.4.bias"][0]
    r["o4"] = r["e4"] @ pm["dec_model.4.weight"][:, :, 0, 0].T + pm["dec_model.4.bias"]
    cat = lambda skip, low, f: np.concatenate((skip, X.up(low, f)), axis=-1)
    r["o3"] = X.conv3x3(cat(r["e3"], r["o4"].reshape(n, 1, 1, 32), 4), *W(pm, "dec_model.3"))
    r["o2"] = X.conv3x3(cat(r["e2"], r["o3"], 2), *W(pm, "dec_model.2"))
    r["o1"] = X.conv3x3(cat(r["e1"], r["o2"], 2), *W(pm, "dec_model.1"))
    r["o0"] = X.conv3x3(cat(e0, r["o1"], 2), *W(pm, "dec_model.0"))
    return r


# ---- layers ----
def conv_bwd_data(dy, w, mut=None):
    """dy NHWC [n,h,w,co], w OIHW -> gradient at the (concatenated) input [n,h,w,ci]: dx[y,x,c] = sum dy[y+1-ky, x+1-kx, o] w[o,c,ky,kx]."""
    n, h, wd, _ = dy.shape
    dyp = np.pad(dy, ((0, 0), (1, 1), (1, 1), (0, 0)))
    if mut == "halo_col":
        dyp[:, :, 0, :] = dyp[:, :, 1, :]                  # halo column 0 taken from column 1 (must be zero)
    dyp = np.ascontiguousarray(dyp.transpose(3, 0, 1, 2))
    out = np.zeros((w.shape[1], n, h, wd))
    nz = np.argwhere(w != 0)
    if mut == "drop_weight":
        nz = nz[1:]                                        # the first non-zero weight of the layer is left out
    for o, c, ky, kx in nz:
        out[c] += w[o, c, ky, kx] * dyp[o][:, 2 - ky:2 - ky + h, 2 - kx:2 - kx + wd]
    return np.ascontiguousarray(out.transpose(1, 2, 3, 0))


def conv_bwd_weight(x, dy, mut=None):
    """x NHWC [n,h,w,ci] (the concatenated input), dy [n,h,w,co] -> slab row [9 ci co + co]: HWIO, then the bias gradient."""
    if mut == "last_image":
        x, dy = x[:-1], dy[:-1]
    n, h, wd, ci = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    g = np.stack([np.einsum("nyxc,nyxo->co", xp[:, ky:ky + h, kx:kx + wd], dy) for ky in range(3) for kx in range(3)])
    return np.concatenate((g.reshape(-1), dy.sum((0, 1, 2))))


def cell_sum(d, f, mut=None):
    """Backward of the nearest upsample by f: the sum over each f x f cell."""
    if mut == "up_shift":
        d = np.roll(d, 1, axis=2)
    n, h, w, c = d.shape
    return d.reshape(n, h // f, f, w // f, f, c).sum((2, 4))


def unpool(dp, am):
    """Gradient at the pooled, ReLU'd map -> gradient at the convolution's output, by the argmax nibbles (0xF: zero)."""
    n, h, w, c = dp.shape
    out = np.zeros((n, h, 2, w, 2, c))
    for ch in range(c):
        nib = (am[..., ch // 8] >> np.uint32(4 * (ch % 8))) & np.uint32(15)
        for pos in range(4):
            out[:, :, pos >> 1, :, pos & 1, ch] = np.where(nib == pos, dp[..., ch], 0.0)
    return out.reshape(n, 2 * h, 2 * w, c)


def backward(params, r, dy_o0, dpred, masks=None, mut=None, absolute=None, pred=0.5):
    """Every tensor the backward kernels write, from the forward run r = forward(params, e0, masks) and the cotangents.
    absolute = the gradients of a plain call: every LAYER's sums are then formed over |x|, |w|, |dy| with the same routing (pool nibbles,
    ReLU masks, Dropout) and with the plain call's tensors as that layer's inputs: for every output element the sum of the absolute values
    of the terms a kernel adds up (a kernel's inputs, and the tensors between the layers of a fused kernel, are exact numbers)."""
    a = np.abs if absolute is not None else (lambda v: v)
    act = (lambda name, v: np.abs(absolute[name])) if absolute is not None else (lambda name, v: v)
    pm = params[1]
    n = dy_o0.shape[0]
    cat = lambda skip, low, f: np.concatenate((a(skip), X.up(a(low), f)), axis=-1)
    g = {}
    # ---- decoder ----
    dy = a(dy_o0)
    lows = {0: r["o1"], 1: r["o2"], 2: r["o3"], 3: r["o4"].reshape(n, 1, 1, 32)}
    for key, i in DEC:
        skip = r[f"e{i}"]
        f = 4 if i == 3 else 2
        g[SLABS[key]] = conv_bwd_weight(cat(skip, lows[i], f), dy, mut)
        d = conv_bwd_data(dy, a(pm[key + ".weight"]), mut)
        cs = skip.shape[-1]
        if mut == "swap45" and i == 2:
            d[..., [4, 5]] = d[..., [5, 4]]
        g[f"dE{i}"] = d[..., :cs]
        dy = cell_sum(d[..., cs:], f, mut)
        name = "d_o4" if i == 3 else f"do{i + 1}"
        g[name] = dy.reshape(n, 32) if i == 3 else dy
        dy = act(name, dy).reshape(dy.shape)
    d_o4 = act("d_o4", g["d_o4"])
    wpw = a(pm["dec_model.4.weight"][:, :, 0, 0])                       # [o][k]
    g["de4_dec"] = d_o4 @ wpw
    g["g_pw"] = pw_slab(a(r["e4"]), d_o4, mut)
    g.update(encoder(params, r, dpred, g, masks, mut, absolute, pred))
    return g


def pw_slab(e4, d_o4, mut=None):
    """dec_model.4's slab row [w 1024 k-major | b 32] over the images of d_o4 (the first len(d_o4) rows of e4)."""
    k = len(d_o4) - (1 if mut == "last_image" else 0)
    return np.concatenate(((e4[:k].T @ d_o4[:k]).reshape(-1), d_o4[:k].sum(0)))


def encoder(params, r, dpred, skips, masks=None, mut=None, absolute=None, pred=0.5, head_only=False):
    """The critic's half: head, features.10, features.6, features.3.  skips: the gradients that arrive from the decoder, dE0..dE3 at the
    embeds and de4_dec at e4 (a missing entry: none); a test zeroes them for the images that get none.  head_only: stop at de3."""
    a = np.abs if absolute is not None else (lambda v: v)
    act = (lambda name, v: np.abs(absolute[name])) if absolute is not None else (lambda name, v: v)
    pc = params[0]
    n = dpred.shape[0]
    m_e2, m_e3, m_h1 = masks if masks is not None else (1.0, 1.0, 1.0)
    sub = slice(0, n - 1) if mut == "last_image" else slice(0, n)
    skip = lambda name: act(name, skips[name]) if name in skips else 0.0
    g = {}
    e4 = a(r["e4"])
    dz2 = a(dpred) * pred * (1.0 - pred)
    h1m = a(r["h1"]) * m_h1
    dh1 = (r["h1"] > 0) * dz2[:, None] * a(pc["crit.4.weight"][0])[None, :] * m_h1
    de4 = dh1 @ a(pc["crit.1.weight"]) + skip("de4_dec")
    dz4 = (r["e4"] > 0) * de4
    e3d = (a(r["e3"]) * m_e3).reshape(n, 256)
    w14 = a(pc["features.14.weight"]).transpose(2, 3, 1, 0).reshape(256, 32)
    hv = np.zeros((n, 384))
    hv[:, :256], hv[:, 256:288], hv[:, 288:320], hv[:, 320:352], hv[:, 352] = e3d, dz4, dh1, dz2[:, None] * h1m, dz2
    g["hvec"] = hv
    if absolute is not None:
        dz4, dh1 = np.abs(absolute["hvec"][:, 256:288]), np.abs(absolute["hvec"][:, 288:320])
    g["g_head"] = np.concatenate(((e3d[sub].T @ dz4[sub]).reshape(-1), dz4[sub].sum(0), (e4[sub].T @ dh1[sub]).reshape(-1), dh1[sub].sum(0),
                                  (dz2[sub, None] * h1m[sub]).sum(0), dz2[sub].sum(keepdims=True)))
    d = (dz4 @ w14.T).reshape(n, 4, 4, 16) * m_e3 + skip("dE3")
    g["de3"] = d
    if head_only:
        return g
    for (key, i), m in zip(reversed(ENC), (m_e2, 1.0, 1.0)):
        x = a(r[f"e{i - 1}"]) * m
        pre = unpool(act(f"de{i}", d), r[f"am{i}"])
        g[SLABS[key]] = conv_bwd_weight(x, pre, mut)
        d = conv_bwd_data(pre, a(pc[key + ".weight"]), mut) * m + skip(f"dE{i - 1}")
        g[f"de{i - 1}"] = d
    return g


def run(draw, n, masks=None, mut=None, carry=None):
    """(params, forward run, gradients) of a draw."""
    P = X.dyadic_params(draw)
    r = forward(P, X.dyadic_e0(draw, n), masks, mut="tie_last" if mut == "tie_last" else None)
    dy, dp = cotangents(draw, n, carry)
    r["dy_o0"], r["dpred"] = dy, dp
    return P, r, backward(P, r, dy, dp, masks, mut)


def tie_counts(params, r, g, masks=None):
    """stage -> number of pool windows that are exact positive ties AND carry a non-zero gradient."""
    pc = params[0]
    out = {}
    for key, i in ENC:
        src = r[f"e{i - 1}"] * (masks[0] if (masks is not None and i == 3) else 1.0)
        _, _, win = X.enc_stage(src, pc[key + ".weight"], pc[key + ".bias"])
        mx = win.max(-1, keepdims=True)
        tie = ((win == mx).sum(-1) >= 2) & (mx[..., 0] > 0)
        out[key] = int((tie & (g[f"de{i}"] != 0)).sum())
    return out


def check_exactness_bwd(params, r, g, masks=None, min_ties=20):
    """Raises AssertionError unless the reference gradients g = backward(params, r, ...) satisfy the conditions under which every
    backward kernel must reproduce them exactly in fp32: (a) the quanta, (b) sums of absolute terms below 2^22 quanta, (c) density,
    (d) gradient-carrying tied pool windows."""
    ab = backward(params, r, r["dy_o0"], r["dpred"], masks, absolute=g)
    for k in TENSORS:
        q = Q_WEIGHT if k.startswith("g_") else Q_DATA
        v = g[k] / q
        assert np.array_equal(v, np.round(v)), f"(a) {k} is not a multiple of {q}"
        assert ab[k].max() < LIMIT_QUANTA * q, f"(b) {k}: sum of absolute terms {ab[k].max()} >= 2^22 quanta of {q}"
        assert (np.abs(g[k]) <= ab[k]).all(), k
        assert np.array_equal(g[k].astype(np.float32).astype(np.float64), g[k]), f"{k} is not fp32-exact"
        body = g[k][:, :353] if k == "hvec" else g[k]
        assert np.count_nonzero(body) >= 0.25 * body.size, f"(c) {k}: only {np.count_nonzero(body) / body.size:.3f} non-zero"
    for key, cnt in tie_counts(params, r, g, masks).items():
        assert cnt >= min_ties, f"(d) {key}: {cnt} gradient-carrying exact positive ties"
