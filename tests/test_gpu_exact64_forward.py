"""Every hand-written forward form that reads a 64x64 frame or writes a 64x64 map, called through the C ABI on the dyadic fixture of
tests/exact64_ref.py and compared with its float64 reference: BIT FOR BIT wherever nothing rounds (e0 and its argmax words from uint8,
fp32 and mixed frames; the materialised mixes and their mask sums; masker.0's h in both families), and within the two DERIVED bounds
where something must (Z: the sigmoid bound in family P, the 146 * 2^-24 * S logit bound on top of it in family M; exact64_ref's
docstring derives both, tests/test_exact64_host.py asserts the fixture's conditions).  No tolerance is measured anywhere.

Each form gets REFERENCE tensors as inputs, so each is tested on its own -- a form-against-form comparison passes when both forms
share one wrong loader.  One test function covers one form: all 36 draws at n = 3 (over the draws every weight element of
features.0, masker.0 and masker.2 is non-zero at least once), draw 0 at n = 1, and draw 0 at one batch just above each grid cap of
the form's launcher; a large batch is 8 distinct images in a non-periodic order (the reference is computed for 8 images), and three
of its images are also run alone and must give the same bits.  Every output sits between two guard bands of 256 sentinel elements
and is pre-filled with the sentinel.  One more, NOT exact, case per form that reads uint8 frames (cgs_conv3x3_fwd features.0 uint8 and
mix, cgs_critic_fwd_fused uint8 and mix -- e0 / am0 only there --, cgs_mix_fwd, masker.0 uint8, the five fused mask heads on uint8
frames, cgs_dec_mask_fwd): full-byte frames (every byte value at each of the 12 byte positions of a 4-pixel group) within
(k + 2) * 2^-24 * S, pool picks compared where the window's two largest values differ by more.
The mask heads' zpart is compared twice: with the float64 sums of the kernel's own Z within 40 * 2^-24 of the sum (the kernels' summation
depth, exact64_ref.zpart_bound: a hundredth of one average pixel), and with the reference's sums within what Z's bound allows.  A failure
prints the first differing element, the reference's terms there (weight x input value at every non-zero weight) and which planted
mutation or single dropped weight reproduces the kernel's value.

Inventory of the C ABI entries that read a 64x64 frame or write a 64x64 map in the forward direction (include/cgs_hip.h):
  tested here
    cgs_conv3x3_fwd           features.0 with CGS_SRC_U8 / CGS_SRC_F32 / CGS_SRC_MIX (n_a replaced; 2 n_a replaced | injected) -> e0, am0;
                              masker.0 with CGS_SRC_U8 / CGS_SRC_F32 -> h (grid cap 2048 workgroups = 256 images: n = 257);
                              masker.2 on a dyadic h -> Z, zpart through `amask`.  (features.0 on the MATERIALISED mix is the
                              CGS_SRC_F32 form on other data: both equal the reference, so they equal each other.)
    cgs_mix_fwd (+ _partials) inject 0 / 1 and mixed = NULL -> mixed, zpart; mix_wg_per_img gives 4, 3, 2, 1 workgroups per image
                              from n = 1, 257, 342, 513 on (1024 workgroups in all; one pixel group per thread up to 256 images)
    cgs_mask_train_fwd, cgs_mask_train_fwd_packed (the operand packed by cgs_tail_dec_fwd_pack, as masker_forward does)  -> h, Z, zpart
    cgs_mask_infer_fwd, cgs_mask_infer_fwd_packed -> Z (the training kernel storing Z alone); one workgroup per image and no cap in
                              the launcher: n = 257, more workgroups than the chip has compute units
    cgs_mask_infer_fwd_tile   -> Z (the tile kernel; grid cap 1024 workgroups = 128 images: n = 129)
    cgs_dec_mask_fwd          -> o3, o2, o1, o0 against exact_ref's decoder, h / Z / zpart against exact64_ref's mask head on that o0, on
                              exact_ref's own inputs (large o0: h exact, Z mostly saturated, masker.2 weakly checked) AND on those inputs
                              times 2^-6 (small o0, unsaturated logits: the check of masker.2 in this form); n > 1024 and fp32 frames:
                              CGS_ERR_UNSUPPORTED and nothing written
    cgs_critic_fwd_fused      uint8 frames and the in-loader mixes -> e0, am0 (and e1 .. pred, o4 against exact_ref's chain on that e0; pred
                              within exact_ref's 4 * 2^-23 * ref: the critic head calls the precise expf, not the mask head's __expf)
  left out
    cgs_critic_fwd_fused_pack   the same launch plus the weight-packing workgroup, whose output the packed mask head tests consume
                                through cgs_tail_dec_fwd_pack's identical packer (test_gpu_dec_mask_fused.py compares the two byte for byte)
    cgs_f16_enc0_fwd, cgs_mask_infer_fwd_f16, cgs_mask_infer_fwd_f16o   scale bytes by 1/1024 and fold 1024/255 into fp16 weights: nothing
                                about them is exact; they keep their measured-distribution tests (test_gpu_generic.py, test_gpu_kernels.py)
    cgs_gen_enc0_fwd, cgs_gen_conv3x3_fwd(_folded), cgs_gen16_* / cgs_genbf16_*   the generic chfak 2..5 path, not the chfak-1 hot path
    cgs_bf16_*                  config 5 (128x128 frames; bf16 operands)
    cgs_sheet_compose, cgs_vis_compose, cgs_video_compose, cgs_overlay_compose, cgs_fit_*, cgs_temporal_*, cgs_dense_crf2, cgs_objects_*,
    cgs_boundary_score, cgs_saliency_sweep, cgs_iou_*, cgs_gather_*   read frames or masks, but are no network layers (own float64 / integer suites)
    every backward entry (cgs_mask_head_bwd, cgs_enc0_bwd_mix*, cgs_enc0_wgrad_u8_*, cgs_mix_bwd*, the bf16 hwgrad family): next"""
import ctypes as C

import numpy as np
import pytest
import torch

import exact64_ref as E
import exact_ref as X
from test_gpu_exact_forward import F32, U32, Guarded, load_params, stream, wc, wm

pytestmark = pytest.mark.gpu

U8 = torch.uint8
N_SMALL = 3


class Store:
    """(draw, n) -> fixture, (draw, family) -> full (critic, masker) parameter dicts; computed once, on demand, and left unchanged."""

    def __init__(self):
        self.fix, self.params, self.xp, self.xrun = {}, {}, {}, {}

    def f(self, d, n):
        if (d, n) not in self.fix:
            self.fix[(d, n)] = E.fixture(d, n)
        return self.fix[(d, n)]

    def xparams(self, d):
        if d not in self.xp:
            self.xp[d] = X.dyadic_params(d)
        return self.xp[d]

    def load(self, env, d, fam):
        """exact_ref's dyadic parameters of draw d with features.0 / masker.0 (family) / masker.2 of exact64_ref."""
        if (d, fam) not in self.params:
            pc, pm = (dict(q) for q in self.xparams(d))
            q = E.params(d, fam)
            for k in ("weight", "bias"):
                pc["features.0." + k] = q["features.0." + k]
                pm["masker.0." + k], pm["masker.2." + k] = q["masker.0." + k], q["masker.2." + k]
            self.params[(d, fam)] = (pc, pm)
        load_params(env, (d, fam))


@pytest.fixture(scope="module")
def env():
    from cgs_amd import _lib, spec
    from cgs_amd import hourglass as hg
    dev = torch.device("cuda:0")
    lc, lm = spec.critic_layout(), spec.masker_layout()
    e = dict(lib=_lib, hg=hg, dev=dev, lc=lc, lm=lm, refs=Store(), fc=torch.zeros(lc.total, device=dev), fm=torch.zeros(lm.total, device=dev),
             fc_host=torch.zeros(lc.total), fm_host=torch.zeros(lm.total))
    _lib.load()
    return e


def dev_t(env, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=env["dev"], dtype=dtype)


def ptr(t):
    return C.c_void_p(t.data_ptr())


# ---- cases ----
def cases(env, fam, big=(), draws=range(E.N_DRAWS)):
    """dicts d, fam, n, f (fixture of the distinct images), idx (batch image -> fixture image), big."""
    st = env["refs"]
    for d in draws:
        yield dict(d=d, fam=fam, n=N_SMALL, f=st.f(d, N_SMALL), idx=np.arange(N_SMALL), big=False)
    yield dict(d=0, fam=fam, n=1, f=st.f(0, 1), idx=np.arange(1), big=False)
    for n in big:
        yield dict(d=0, fam=fam, n=n, f=st.f(0, E.N_DISTINCT), idx=E.big_order(n), big=True)


def fullbyte_case(env, d=0, n=2):
    f = E.evaluate(E.inputs_fullbyte(d, n), E.params(d, "P"), E.params(d, "M"), exact=False)
    f["bounds"] = E.fullbyte_bounds(f)
    return dict(d=d, fam="M", n=n, f=f, idx=np.arange(n), big=False, fullbyte=True)


def pick(f, path):
    for k in path:
        f = f[k]
    return f


# ---- failure reports ----
LAYER_OF = {"e0": "features.0", "am0": "features.0", "h": "masker.0", "Z": "masker.2", "mix1": None}


def explain(case, path, got, ref, at, within=None):
    """The reference's contributing terms at the first differing element `at`, and which planted mutation of the reference, or ONE dropped
    weight of the layer, gives the kernel's value there (within: a bound array instead of equality)."""
    f, n = case["f"], case["n"]
    block, img = divmod(at[0], n) if got.shape[0] != n else (0, at[0])
    fi = int(case["idx"][img])
    lines = [f"first at (image, y, x, channel ...) = {at}: kernel {got[at]!r}, reference {ref[at]!r}; batch image {img} is fixture image {fi}"]
    name = path[-1].split("_")[0]
    layer = LAYER_OF.get(name)
    pP, pM = f["pP"], f["pM"]
    pw = pM if (len(path) == 2 and path[0].endswith("M")) else pP
    if layer and not name.startswith("am"):
        w = pw[layer + ".weight"]
        o = at[-1] if name != "Z" else 0
        lines.append(f"{layer}: output channel {o} reads weights (in-channel, ky, kx) -> w: "
                     + ", ".join(f"{tuple(int(i) for i in ix)} -> {w[o][tuple(ix)]}" for ix in np.argwhere(w[o] != 0)) + f"; bias {pw[layer + '.bias'][o]}")
    inp = E.image_of(f, fi)
    local = (block,) + tuple(at[1:])
    exact = not case.get("fullbyte")
    if layer and not name.startswith("am"):
        lines += terms(f, inp, path, layer, pw, local, exact)

    def same(pp, pm, mut=None):
        t = pick(E.evaluate(inp, pp, pm, mut, exact), path)
        v = t[local]
        return abs(float(got[at]) - float(v)) <= within[at] if within is not None else np.asarray(v).astype(got.dtype) == got[at]
    hits = [m for m in E.MUTATIONS if same(pP, pM, m)]
    if layer:
        w = pw[layer + ".weight"]
        for ix in np.argwhere(w != 0):
            q = dict(pw)
            q[layer + ".weight"] = w.copy()
            q[layer + ".weight"][tuple(ix)] = 0.0
            if same(q if pw is pP else pP, q if pw is pM else pM):
                hits.append(f"{layer}.weight{tuple(int(i) for i in ix)} dropped")
    lines.append("reference mutations that reproduce the kernel's value: " + (", ".join(hits) if hits else "none of those tried"))
    return "\n".join(lines)


def terms(f, inp, path, layer, pw, local, exact):
    """The reference's contributing terms of one output element: weight x input value at every non-zero weight (for a pooled element, at
    each of the window's four pixels)."""
    a = E.u8_values(inp["A"])
    if layer == "features.0":
        src = path[-1].split("_")[1]
        x = {"u8": a, "f32": inp["F"], "mix": E.mix(a, E.u8_values(inp["B"]), inp["Zin"], 1)}[src]
        pixels = [(2 * local[1] + dy, 2 * local[2] + dx) for dy in (0, 1) for dx in (0, 1)]
        o = local[3]
    elif layer == "masker.0":
        x = E.cat_in(a if "u8" in path[0] else inp["F"], inp["o0" + path[0][-1]])
        pixels, o = [(local[1], local[2])], local[3]
    else:
        x = inp["hin"] if path[0] == "m2" else pick(E.evaluate(inp, f["pP"], f["pM"], None, exact, groups=("head",)), path[:-1])["h"]
        pixels, o = [(local[1], local[2])], 0
    xp = np.pad(x[local[0]], ((1, 1), (1, 1), (0, 0)))
    w, out = pw[layer + ".weight"][o], []
    for y, xx in pixels:
        t = [f"{w[tuple(ix)]:+g} * {xp[y + ix[1], xx + ix[2], ix[0]]!r}" for ix in np.argwhere(w != 0)]
        total = sum(w[tuple(ix)] * xp[y + ix[1], xx + ix[2], ix[0]] for ix in np.argwhere(w != 0)) + pw[layer + ".bias"][o]
        out.append(f"  input pixel {(y, xx)}: " + " ".join(t) + f" + bias = {total!r}")
    return out


# ---- rules: how one output is compared ----
def r_exact(path, f=None):
    """f: another fixture dict than the case's (a half of [replaced | injected], references of exact_ref added)."""
    def rule(case, what, got, all_got):
        case = case if f is None else dict(case, f=f)
        ref = pick(case["f"], path)
        ref = ref[case["idx"]] if ref.shape[0] == len(case["f"]["A"]) else np.concatenate([h[case["idx"]] for h in np.split(ref, 2)])
        ref = ref if ref.dtype == np.uint32 else ref.astype(got.dtype)
        assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
        if not np.array_equal(got, ref):
            bad = np.argwhere(got != ref)
            at = tuple(int(i) for i in bad[0])
            raise AssertionError(f"{what} is not bit-identical to the float64 reference: {len(bad)}/{got.size} elements differ\n"
                                 + explain(case, path, got, ref, at))
    return rule


def r_bound(path, bound_of, f=None, scan=True):
    def rule(case, what, got, all_got):
        case = case if f is None else dict(case, f=f)
        idx = case["idx"]
        ref, bound = pick(case["f"], path), bound_of(case["f"])
        if ref.shape[0] != len(case["f"]["A"]):
            idx = np.concatenate([idx, idx + len(case["f"]["A"])])
        ref, bound = ref[idx], bound[idx]
        assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
        err = np.abs(got.astype(np.float64) - ref)
        worst = (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0      # (bound 0: a sum of zeros, err must be 0)
        print(f"{what}: worst |got - ref| / bound = {worst:.3f}")
        if not (err <= bound).all():
            at = tuple(int(i) for i in np.argwhere(err > bound)[0])
            raise AssertionError(f"{what}: {(err > bound).sum()}/{got.size} elements outside the derived bound, worst |got - ref| / bound = "
                                 f"{worst:.2f}\n" + (explain(case, path, got, ref, at, within=bound) if scan else f"first at {at}"))
    return rule


def r_am_gap(src):
    """Full-byte case: argmax nibbles where the reference decides them -- the window's two largest values further apart than twice the
    window's bound, and the largest further from zero than the bound."""
    def rule(case, what, got, all_got):
        f = case["f"]
        win, pb, ref = f["win_" + src], f["bounds"]["e0_" + src], f["am0_" + src]
        top = np.sort(win, axis=-1)
        decided = (top[..., 3] - top[..., 2] > 2 * pb) & (np.abs(top[..., 3]) > pb)
        nib = lambda am: np.stack([(am[..., 0] >> np.uint32(4 * c)) & np.uint32(15) for c in range(8)], axis=-1)
        assert decided.mean() > 0.5, f"{what}: only {decided.mean():.2f} of the picks are decided"
        bad = decided & (nib(got) != nib(ref))
        assert not bad.any(), f"{what}: {bad.sum()} decided pool picks differ, first at {tuple(np.argwhere(bad)[0])}"
    return rule


def r_zsum_exact(rows_of):
    """zpart rows of an image summed in float64 == the exact sums of the dyadic mask."""
    def rule(case, what, got, all_got):
        n, k = case["n"], rows_of(case["n"])
        assert got.shape == (n * k, 2), f"{what}: shape {got.shape}, {k} rows per image"
        sums = got.astype(np.float64).reshape(n, k, 2).sum(1)
        ref = case["f"]["zpart_in"][case["idx"]]
        assert np.array_equal(sums, ref), f"{what}: per-image (sum |Z|, sum Z^2) differ from the exact sums at images {np.argwhere(sums != ref)[:4, 0]}"
    return rule


def r_zsum_own(zname, k, path, bound_of):
    """zpart rows of an image summed in float64: against the float64 sums of the kernel's OWN Z within zpart_bound (the kernels' summation
    depth: sees a single dropped or doubled pixel), and against the reference's sums within what Z's own bound (bound_of) allows."""
    def rule(case, what, got, all_got):
        n = case["n"]
        assert got.shape == (n * k, 2), f"{what}: shape {got.shape}"
        sums = got.astype(np.float64).reshape(n, k, 2).sum(1)
        z = all_got[zname].astype(np.float64)
        own, bound = E.zpart(z), E.zpart_bound(z)
        assert (np.abs(sums - own) <= bound).all(), f"{what}: worst |zpart - sums of Z| / bound = {(np.abs(sums - own) / bound).max():.2f}"
        zr, zb = pick(case["f"], path)[case["idx"]], bound_of(case["f"])[case["idx"]]
        ref, rb = E.zpart(zr), E.zpart_ref_bound(zr, zb) + E.zpart_bound(zr + zb)
        assert (np.abs(sums - ref) <= rb).all(), f"{what}: worst |zpart - reference sums| / bound = {(np.abs(sums - ref) / rb).max():.2f}"
    return rule


# ---- the runner ----
def run(env, form, case_list, build):
    """build(case) -> (inputs: name -> (array with the batch's images, dtype), outputs: name -> (shape, dtype, layout), launch(n, I, O),
    rules: name -> rule).  layout: how the rows of image i alone map into the batch -- 'img' [i], 'block' [i, n + i] ([replaced | injected]),
    'rows' k consecutive rows per image, None: not compared between the batch and the image alone."""
    dev, st = env["dev"], env["refs"]

    def once(case):
        inputs, outputs, launch, rules = build(case)
        I = {k: dev_t(env, a, dt) for k, (a, dt) in inputs.items()}
        O = {k: Guarded(shape, dt, dev) for k, (shape, dt, _) in outputs.items()}
        for g in O.values():
            g.reset()
        launch(case["n"], {k: ptr(t) for k, t in I.items()}, {k: g.ptr for k, g in O.items()})
        torch.cuda.synchronize()
        what = f"{form} draw {case['d']} family {case['fam']} n={case['n']}" + (" full-byte" if case.get("fullbyte") else "")
        got = {k: O[k].read(f"{what}: {k}") for k in O}
        return outputs, rules, got, what

    for case in case_list:
        st.load(env, case["d"], case["fam"])
        outputs, rules, got, what = once(case)
        for k, rule in rules.items():
            rule(case, f"{what}: {k}", got[k], got)
        if case["big"]:                                   # the same images alone: same bits, whichever workgroup and round took them
            n = case["n"]
            for i in (0, n // 2, n - 1):
                _, _, alone, _ = once(dict(case, n=1, idx=case["idx"][i:i + 1], big=False))
                for k, (_, _, layout) in outputs.items():
                    if layout is None:
                        continue
                    m = alone[k].shape[0]
                    rows = [i] if layout == "img" else [i, n + i][:m] if layout == "block" else list(range(i * m, i * m + m))
                    assert np.array_equal(alone[k], got[k][rows]), f"{what}: {k} of image {i} differs between the batch and n=1"


def frames(case, key):
    return case["f"][key][case["idx"]]


def conv_desc(L, n, ca, cb, co, src, act, pool):
    return L.ConvDesc(n, 64, 64, ca, cb, co, src, 2, act, pool, L.Dropout())


# ---- features.0 ----
@pytest.mark.parametrize("src", ["u8", "f32"])
def test_conv3x3_fwd_features0(env, src):
    L = env["lib"]
    kind, key, dt = (L.SRC_U8, "A", U8) if src == "u8" else (L.SRC_F32, "F", F32)

    def build(case):
        n = case["n"]

        def launch(n, I, O):
            d = conv_desc(L, n, 3, 0, 8, kind, L.ACT_RELU, 1)
            L.call("cgs_conv3x3_fwd", C.byref(d), I["x"], None, wc(env, "features.0.weight"), wc(env, "features.0.bias"), O["e0"], O["am0"], stream())
        if case.get("fullbyte"):
            rules = {"e0": r_bound(("e0_u8",), lambda f: f["bounds"]["e0_u8"]), "am0": r_am_gap("u8")}
        else:
            rules = {"e0": r_exact(("e0_" + src,)), "am0": r_exact(("am0_" + src,))}
        return ({"x": (frames(case, key), dt)}, {"e0": ((n, 32, 32, 8), F32, "img"), "am0": ((n, 32, 32, 1), U32, "img")}, launch, rules)
    run(env, f"cgs_conv3x3_fwd(features.0, {src})", list(cases(env, "P")) + ([fullbyte_case(env)] if src == "u8" else []), build)


def mix_src(L, I, n_a):
    m = L.MixSrc(I["a"].value, I["b"].value, I["z"].value, n_a, 0)
    return m, C.cast(C.pointer(m), C.c_void_p)


def mix_inputs(case):
    return {"a": (frames(case, "A"), U8), "b": (frames(case, "B"), U8), "z": (frames(case, "Zin"), F32)}


def mix_rules(case, inject):
    """inject 0: the replaced half of the fixture's [replaced | injected] tensors."""
    f = case["f"]
    nf = len(f["A"])
    if not inject:
        f = dict(f, e0_mix=f["e0_mix"][:nf], am0_mix=f["am0_mix"][:nf], win_mix=f["win_mix"][:nf])
        if case.get("fullbyte"):
            f["bounds"] = dict(f["bounds"], e0_mix=f["bounds"]["e0_mix"][:nf])
    if case.get("fullbyte"):
        return {"e0": r_bound(("e0_mix",), lambda g: g["bounds"]["e0_mix"], f=f), "am0": lambda c, w, g, a: r_am_gap("mix")(dict(c, f=f), w, g, a)}
    return {"e0": r_exact(("e0_mix",), f=f), "am0": r_exact(("am0_mix",), f=f)}


@pytest.mark.parametrize("inject", [0, 1])
def test_conv3x3_fwd_features0_mix(env, inject):
    """CGS_SRC_MIX: the mixes are formed in the tile loader.  inject 0: n = n_a images (replaced); 1: n = 2 n_a (replaced | injected)."""
    L = env["lib"]

    def build(case):
        n_a = case["n"]
        n = (1 + inject) * n_a

        def launch(n_a, I, O):
            m, mp = mix_src(L, I, n_a)
            d = conv_desc(L, (1 + inject) * n_a, 3, 0, 8, L.SRC_MIX, L.ACT_RELU, 1)
            L.call("cgs_conv3x3_fwd", C.byref(d), mp, None, wc(env, "features.0.weight"), wc(env, "features.0.bias"), O["e0"], O["am0"], stream())
        return (mix_inputs(case), {"e0": ((n, 32, 32, 8), F32, "block"), "am0": ((n, 32, 32, 1), U32, "block")}, launch, mix_rules(case, inject))
    run(env, f"cgs_conv3x3_fwd(features.0, mix, inject={inject})", list(cases(env, "P")) + [fullbyte_case(env)], build)


@pytest.mark.parametrize("x_is_mix", [0, 1])
def test_critic_fwd_fused(env, x_is_mix):
    """The whole critic forward of an image in one workgroup: e0 / am0 against exact64_ref, the rest against exact_ref's chain on that e0
    (all fp32 tensors; the sums of absolute terms stay far inside fp32's exact range: exact64_ref.critic_chain).  One workgroup per image and no
    cap in the launcher: n = 257.  The full-byte case compares e0 / am0 (the pipelined uint8 loader and the mix loader of THIS kernel)."""
    L, st = env["lib"], env["refs"]
    nd = L.Dropout()
    e0k, amk = ("e0_mix", "am0_mix") if x_is_mix else ("e0_u8", "am0_u8")
    TAIL = {"e1": ((16, 16, 8), F32), "am1": ((16, 16, 1), U32), "e2": ((8, 8, 8), F32), "am2": ((8, 8, 1), U32), "e3": ((4, 4, 16), F32),
            "am3": ((4, 4, 2), U32), "e4": ((32,), F32), "h1": ((32,), F32), "pred": ((), F32), "o4": ((32,), F32)}

    def chain(case):
        """The case's fixture + exact_ref's chain on its e0 as x_<name>."""
        f = case["f"]
        key = ("crit", case["d"], len(f["A"]), x_is_mix)
        if key not in st.xrun:
            r = E.critic_chain(st.xparams(case["d"]), f[e0k])
            st.xrun[key] = dict(f, **{"x_" + k: v for k, v in r.items()})
        return st.xrun[key]

    def build(case):
        n_a = case["n"]
        n = (1 + x_is_mix) * n_a
        fb = case.get("fullbyte")
        f = case["f"] if fb else chain(case)
        nf = len(f["A"])

        def launch(n_a, I, O):
            tw = env["hg"].tail_enc_weights(env["fc"], env["lc"], pw=(wm(env, "dec_model.4.weight").value, wm(env, "dec_model.4.bias").value))
            if x_is_mix:
                launch.m, x = mix_src(L, I, n_a)
            else:
                x = I["a"]
            L.call("cgs_critic_fwd_fused", (1 + x_is_mix) * n_a, C.byref(tw), x, x_is_mix, wc(env, "features.0.weight"), wc(env, "features.0.bias"),
                   O["e0"], O["am0"], wc(env, "features.3.weight"), wc(env, "features.3.bias"), O["e1"], O["am1"], O["e2"], O["am2"], O["e3"], O["am3"],
                   O["e4"], O["h1"], O["pred"], O["o4"], nd, nd, nd, stream())
        lay = "block" if x_is_mix else "img"
        outs = {"e0": ((n, 32, 32, 8), F32, lay), "am0": ((n, 32, 32, 1), U32, lay)}
        outs.update({k: ((n,) + s, dt, lay) for k, (s, dt) in TAIL.items()})
        if fb:       # e0 / am0 alone: the layers below get a non-dyadic e0 there (they are written between their guard bands all the same)
            src = "mix" if x_is_mix else "u8"
            rules = {"e0": r_bound((e0k,), lambda g: g["bounds"]["e0_" + src]), "am0": r_am_gap(src)}
        else:
            rules = {"e0": r_exact((e0k,)), "am0": r_exact((amk,))}
            for k in TAIL:
                rules[k] = r_exact_plain("x_" + k, nf, f)
            # exact_ref's bound for pred: the critic head calls the precise expf (csrc/tail.hip), within 1 ulp for any argument -- not the
            # mask head's __expf, whose bound (exact64_ref.sig_bound) grows with |logit|
            rules["pred"] = r_bound(("x_pred",), lambda g: 4 * 2.0 ** -23 * g["x_pred"], f=f, scan=False)
        inputs = mix_inputs(case) if x_is_mix else {"a": (frames(case, "A"), U8)}
        return inputs, outs, launch, rules
    run(env, f"cgs_critic_fwd_fused(mix={x_is_mix})", list(cases(env, "P", big=(257,))) + [fullbyte_case(env)], build)


def r_exact_plain(key, nf, f=None):
    """Bit-identity with a reference tensor that is no tensor of exact64_ref (no mutation report): rows by image, or [replaced | injected]."""
    def rule(case, what, got, all_got):
        ref = (f or case["f"])[key]
        idx = case["idx"] if ref.shape[0] == nf else np.concatenate([case["idx"], case["idx"] + nf])
        ref = ref[idx] if ref.dtype == np.uint32 else ref[idx].astype(got.dtype)
        assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
        bad = np.argwhere(got != ref)
        assert not len(bad), (f"{what} is not bit-identical to exact_ref's float64 chain: {len(bad)}/{got.size} elements differ, first at "
                              f"{tuple(bad[0])}: kernel {got[tuple(bad[0])]!r}, reference {ref[tuple(bad[0])]!r}")
    return rule


# ---- the materialised mix ----
@pytest.mark.parametrize("mode", ["replaced", "replaced+injected", "sums only"])
def test_mix_fwd(env, mode):
    L = env["lib"]
    inject = int(mode == "replaced+injected")
    lib = L.load()

    def build(case):
        n = case["n"]
        k = lib.cgs_mix_fwd_partials(n, 4096) // n
        assert k == min(4, max(1, 1024 // n)), (n, k)

        def launch(n, I, O):
            L.call("cgs_mix_fwd", n, 4096, I["a"], I["b"], I["z"], inject, O.get("mixed"), O["zpart"], stream())
        outs = {"zpart": ((n * k, 2), F32, None)}
        rules = {"zpart": r_zsum_exact(lambda n: k)}
        if mode != "sums only":
            outs["mixed"] = (((1 + inject) * n, 64, 64, 3), F32, "block")
            f = case["f"]
            nf = len(f["A"])
            if not inject:
                f = dict(f, mix1=f["mix1"][:nf])
                if case.get("fullbyte"):
                    f["bounds"] = dict(f["bounds"], mix1=f["bounds"]["mix1"][:nf])
            rules["mixed"] = r_bound(("mix1",), lambda g: g["bounds"]["mix1"], f=f) if case.get("fullbyte") else r_exact(("mix1",), f=f)
        return mix_inputs(case), outs, launch, rules
    extra = [fullbyte_case(env)] if mode != "sums only" else []
    run(env, f"cgs_mix_fwd({mode})", list(cases(env, "P", big=(257, 342, 513))) + extra, build)


# ---- the mask head, layer by layer ----
def head_cases(env, big):
    """Both families over all draws; the large batches in family M (the code path does not depend on the family)."""
    return list(cases(env, "P")) + list(cases(env, "M", big=big))


def head_inputs(case, src):
    return {"x": (frames(case, "A" if src == "u8" else "F"), U8 if src == "u8" else F32), "o0": (frames(case, "o0" + case["fam"]), F32)}


def head_rules(case, src, names):
    if case.get("fullbyte"):
        mh, zb = ("mh_u8M",), (lambda f: f["bounds"]["ZM"])
        r = {"h": r_bound(mh + ("h",), lambda f: f["bounds"]["hM"])}
    else:
        mh, zb = ("mh_" + src + case["fam"],), (lambda f: E.z_bound(pick(f, mh), case["fam"] == "P"))
        r = {"h": r_exact(mh + ("h",))}
    r["Z"] = r_bound(mh + ("Z",), zb)
    r["zpart"] = r_zsum_own("Z", 1, mh + ("Z",), zb)
    return {k: r[k] for k in names}


@pytest.mark.parametrize("src", ["u8", "f32"])
def test_conv3x3_fwd_masker0(env, src):
    L = env["lib"]

    def build(case):
        n = case["n"]

        def launch(n, I, O):
            d = conv_desc(L, n, 3, 8, 16, L.SRC_U8 if src == "u8" else L.SRC_F32, L.ACT_LRELU, 0)
            L.call("cgs_conv3x3_fwd", C.byref(d), I["x"], I["o0"], wm(env, "masker.0.weight"), wm(env, "masker.0.bias"), O["h"], None, stream())
        return head_inputs(case, src), {"h": ((n, 64, 64, 16), F32, "img")}, launch, head_rules(case, src, ("h",))
    run(env, f"cgs_conv3x3_fwd(masker.0, {src})", head_cases(env, (257,)) + ([fullbyte_case(env)] if src == "u8" else []), build)


def test_conv3x3_fwd_masker2(env):
    """masker.2 + sigmoid on a dyadic h (the logit is exact: the sigmoid bound alone); zpart [4 n][2] through the `amask` argument."""
    L = env["lib"]

    def build(case):
        n = case["n"]

        def launch(n, I, O):
            d = conv_desc(L, n, 16, 0, 1, L.SRC_F32, L.ACT_SIGMOID, 0)
            L.call("cgs_conv3x3_fwd", C.byref(d), I["h"], None, wm(env, "masker.2.weight"), wm(env, "masker.2.bias"), O["Z"], O["zpart"], stream())
        zb = lambda f: E.SIG_ULPS * 2.0 ** -23 * f["m2"]["Z"]
        rules = {"Z": r_bound(("m2", "Z"), zb), "zpart": r_zsum_own("Z", 4, ("m2", "Z"), zb)}
        return {"h": (frames(case, "hin"), F32)}, {"Z": ((n, 64, 64), F32, "img"), "zpart": ((4 * n, 2), F32, "rows")}, launch, rules
    run(env, "cgs_conv3x3_fwd(masker.2)", cases(env, "P"), build)


# ---- the fused mask heads ----
def build_pack(env):
    """masker.0's weight registers [40 * 64] the way masker_forward gets them: from the spare workgroup of cgs_tail_dec_fwd_pack."""
    L, dev = env["lib"], env["dev"]
    pack = torch.full((40 * 64,), -7.0, device=dev)
    z = {k: torch.zeros(s, device=dev) for k, s in (("e1", 16 * 16 * 8), ("e2", 8 * 8 * 8), ("e3", 4 * 4 * 16), ("o4", 32), ("o3", 256), ("o2", 512), ("o1", 2048))}
    td = env["hg"].tail_dec_weights(env["fm"], env["lm"])
    L.call("cgs_tail_dec_fwd_pack", 1, C.byref(td), ptr(z["e1"]), ptr(z["e2"]), ptr(z["e3"]), ptr(z["o4"]), ptr(z["o3"]), ptr(z["o2"]), ptr(z["o1"]),
           wm(env, "masker.0.weight"), ptr(pack), stream())
    return pack


def mask_head_form(env, entry, src, names, big):
    L = env["lib"]
    kind = L.SRC_U8 if src == "u8" else L.SRC_F32
    shapes = {"h": ((64, 64, 16), "img"), "Z": ((64, 64), "img"), "zpart": ((2,), "img")}

    def build(case):
        n = case["n"]

        def launch(n, I, O):
            w = (wm(env, "masker.0.weight"), wm(env, "masker.0.bias"), wm(env, "masker.2.weight"), wm(env, "masker.2.bias"))
            outs = tuple(O[k] for k in names)
            extra = ()
            if entry.endswith("_packed"):
                launch.pack = build_pack(env)                     # (kept alive until the synchronize that follows the launch)
                extra = (ptr(launch.pack),)
            L.call(entry, n, kind, I["x"], I["o0"], *w, *outs, *extra, stream())
        return (head_inputs(case, src), {k: ((n,) + shapes[k][0], F32, shapes[k][1]) for k in names}, launch, head_rules(case, src, names))
    run(env, f"{entry}({src})", head_cases(env, big) + ([fullbyte_case(env)] if src == "u8" else []), build)


@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("entry", ["cgs_mask_train_fwd", "cgs_mask_train_fwd_packed"])
def test_mask_train_fwd(env, entry, src):
    mask_head_form(env, entry, src, ("h", "Z", "zpart"), (257,))


@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("entry", ["cgs_mask_infer_fwd", "cgs_mask_infer_fwd_packed"])
def test_mask_infer_fwd(env, entry, src):
    mask_head_form(env, entry, src, ("Z",), (257,))


@pytest.mark.parametrize("src", ["u8", "f32"])
def test_mask_infer_fwd_tile(env, src):
    mask_head_form(env, "cgs_mask_infer_fwd_tile", src, ("Z",), (129,))


# ---- decoder + mask head in one launch ----
DEC_IN = ("e0", "e1", "e2", "e3", "o4")
DEC_OUT = {"o3": (4, 4, 16), "o2": (8, 8, 8), "o1": (16, 16, 8), "o0": (32, 32, 8)}


def dec_mask_args(env, n, I, O, src, pack):
    td = env["hg"].tail_dec_weights(env["fm"], env["lm"])
    return (n, C.byref(td), I["e0"], I["e1"], I["e2"], I["e3"], I["o4"], O["o3"], O["o2"], O["o1"], wm(env, "dec_model.0.weight"), wm(env, "dec_model.0.bias"),
            O["o0"], src, I["x"], wm(env, "masker.0.bias"), wm(env, "masker.2.weight"), wm(env, "masker.2.bias"), O["h"], O["Z"], O["zpart"], ptr(pack), stream())


def test_dec_mask_fwd(env):
    """o3 .. o0 against the float64 decoder (exact_ref's, on its e0 .. o4 as inputs), h / Z / zpart against exact64_ref's mask head (family M)
    on THAT o0 (exact64_ref.dec_mask_fixture).  Two groups of cases over all draws.  'full': exact_ref's own tensors -- |o0| reaches a few
    hundred, h is still bit-exact (fp32 holds the sums), but most logits are saturated: masker.2 and the sigmoid are checked only weakly
    there (Z: 0.25 * 146 * 2^-24 * S + sig_bound).  'small': the same inputs times 2^-6 (the decoder is linear), so that o0 stays of the
    biases' size and most logits lie inside (-10, 10): the group that checks masker.2 in this instantiation.  One full-byte case (small
    inputs): this kernel has its own instantiation of the uint8 frame loader, with the first strip's fetch hoisted in front of the decoder."""
    L, st = env["lib"], env["refs"]

    def fixture_of(d, n, scale=1.0, fullbyte=False):
        key = ("dm", d, n, scale, fullbyte)
        if key not in st.xrun:
            st.xrun[key] = E.dec_mask_fixture(d, n, st.xparams(d), scale, fullbyte)
        return st.xrun[key]

    def dm_cases():
        for scale in (1.0, E.DEC_SMALL):
            for d in range(E.N_DRAWS):
                yield dict(d=d, fam="M", n=N_SMALL, f=fixture_of(d, N_SMALL, scale), idx=np.arange(N_SMALL), big=False)
            yield dict(d=0, fam="M", n=1, f=fixture_of(0, 1, scale), idx=np.arange(1), big=False)
        yield dict(d=0, fam="M", n=257, f=fixture_of(0, E.N_DISTINCT), idx=E.big_order(257), big=True)
        yield dict(d=0, fam="M", n=2, f=fixture_of(0, 2, E.DEC_SMALL, True), idx=np.arange(2), big=False, fullbyte=True)

    def build(case):
        n, f = case["n"], case["f"]
        nf = len(f["A"])

        def launch(n, I, O):
            launch.pack = build_pack(env)
            rc = L.load().cgs_dec_mask_fwd(*dec_mask_args(env, n, I, O, L.SRC_U8, launch.pack))
            assert rc == L.OK, rc
        inputs = {k: (f["x_" + k][case["idx"]], F32) for k in DEC_IN}
        inputs["x"] = (frames(case, "A"), U8)
        outs = {k: ((n,) + s, F32, "img") for k, s in DEC_OUT.items()}
        outs.update(h=((n, 64, 64, 16), F32, "img"), Z=((n, 64, 64), F32, "img"), zpart=((n, 2), F32, "img"))
        rules = {k: r_exact_plain("x_" + k, nf) for k in DEC_OUT}
        mh, zb = ("mh_u8M",), (lambda f: f["Z_bound"])
        rules["h"] = r_bound(mh + ("h",), lambda f: f["bounds"]["hM"]) if case.get("fullbyte") else r_exact(mh + ("h",))
        rules["Z"] = r_bound(mh + ("Z",), zb)
        rules["zpart"] = r_zsum_own("Z", 1, mh + ("Z",), zb)
        return inputs, outs, launch, rules
    # (explain() re-evaluates from case['f'], which here carries the decoder's o0 as o0M)
    run(env, "cgs_dec_mask_fwd", dm_cases(), build)


@pytest.mark.parametrize("why", ["n = 1025", "fp32 frames"])
def test_dec_mask_fwd_answers_unsupported_beyond_its_limits(env, why):
    """Beyond the documented limits (n <= 1024, uint8 frames): CGS_ERR_UNSUPPORTED and nothing written.  Every buffer has the size the call
    would need, so that a launcher that lost the check fails the assertions below and writes nowhere else."""
    L, dev = env["lib"], env["dev"]
    env["refs"].load(env, 0, "M")
    n, src = (1025, L.SRC_U8) if why == "n = 1025" else (3, L.SRC_F32)
    IN = {"e0": 32 * 32 * 8, "e1": 16 * 16 * 8, "e2": 8 * 8 * 8, "e3": 4 * 4 * 16, "o4": 32}
    I = {k: torch.zeros(n * s, device=dev) for k, s in IN.items()}
    I["x"] = torch.zeros(n * 64 * 64 * 3, device=dev, dtype=U8 if src == L.SRC_U8 else F32)
    OUT = dict({k: int(np.prod(s)) for k, s in DEC_OUT.items()}, h=64 * 64 * 16, Z=64 * 64, zpart=2)
    O = {k: torch.full((n * s,), -12345.0, device=dev) for k, s in OUT.items()}
    pack = build_pack(env)
    rc = L.load().cgs_dec_mask_fwd(*dec_mask_args(env, n, {k: ptr(t) for k, t in I.items()}, {k: ptr(t) for k, t in O.items()}, src, pack))
    torch.cuda.synchronize()
    assert rc == L.ERR_UNSUPPORTED
    for k, t in O.items():
        assert bool((t == -12345.0).all()), f"{k} was written by a call that answered CGS_ERR_UNSUPPORTED"
