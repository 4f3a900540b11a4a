"""Every hand-written forward form of the layers from e0 (32x32x8) down to the bottleneck and back up to o0, called through the C
ABI on the dyadic fixture of tests/exact_ref.py and compared BIT FOR BIT with its float64 reference.

On that fixture nothing rounds (activations are multiples of 1/4, every sum of absolute terms stays below 512: exact in fp16 and
fp32 in any order, on any matrix instruction; tests/test_exact_host.py asserts the conditions), so there is no tolerance: every
tensor a form writes equals the reference cast to its dtype, pool-argmax words included.  The one exception is pred: its logit is
exact, expf is within 1 ulp, the add within 1/2 ulp, the correctly rounded division within 1/2 ulp -- under 2 ulp; the bound is
twice that, |pred - ref| <= 4 * 2^-23 * ref with ref = 1 / (1 + exp(-logit)) in float64.

Each form gets REFERENCE tensors as inputs, so each is tested on its own.  One test function covers one form over all 108 draws at
n = 3 (over the draws every weight element of every layer is non-zero at least once), and draw 0 at n = 1 and n = 1100 (more images
than any tail launcher's persistent-workgroup cap; three images of that batch are also run alone and must give the same bits).
Every output sits between two guard bands of 256 sentinel elements inside one allocation; the bands must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_ref as X

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL = {torch.float32: -12345.0, torch.float16: -1234.0, torch.int32: -0x5A5A5A5B}
NP = {torch.float32: np.float32, torch.float16: np.float16, torch.int32: np.uint32}
F32, F16, U32 = torch.float32, torch.float16, torch.int32
ORDER = ("e1", "am1", "e2", "am2", "e3", "am3", "e4", "h1", "pred", "o4", "o3", "o2", "o1", "o0")     # chain order: first mismatch first
N_BIG = 1100


class Refs:
    """(draw, n) -> the float64 reference (with its e0), computed once and left unchanged; params of a draw likewise."""

    def __init__(self):
        self.params = {d: X.dyadic_params(d) for d in range(X.N_DRAWS)}
        self.runs = {}
        for d in range(X.N_DRAWS):
            self._add(d, 3)
        self._add(0, 1)
        self._add(0, N_BIG)

    def _add(self, d, n):
        e0 = X.dyadic_e0(d, n)
        r = X.forward(self.params[d], e0)
        r["e0"] = e0
        self.runs[(d, n)] = r

    def get(self, d, n, first=None):
        r = self.runs[(d, n)]
        return r if first is None else {k: v[:first] for k, v in r.items()}


@pytest.fixture(scope="module")
def env():
    from cgs_amd import _lib, spec
    from cgs_amd import hourglass as hg
    dev = torch.device("cuda:0")
    lc, lm = spec.critic_layout(), spec.masker_layout()
    e = dict(lib=_lib, hg=hg, dev=dev, lc=lc, lm=lm, refs=Refs(), fc=torch.zeros(lc.total, device=dev), fm=torch.zeros(lm.total, device=dev),
             fc_host=torch.zeros(lc.total), fm_host=torch.zeros(lm.total))
    _lib.load()
    return e


def load_params(env, d):
    """The draw's reference-convention (OIHW) parameters through spec's layout conversion into the flat kernel-layout buffers."""
    pc, pm = env["refs"].params[d]
    env["lc"].flatten({k: torch.from_numpy(v) for k, v in pc.items()}, env["fc_host"])
    env["lm"].flatten({k: torch.from_numpy(v) for k, v in pm.items()}, env["fm_host"])
    env["fc"].copy_(env["fc_host"])
    env["fm"].copy_(env["fm_host"])


class Guarded:
    """An output tensor inside one larger allocation, 256 sentinel elements on each side (and the sentinel in the body before a launch)."""

    def __init__(self, shape, dtype, dev):
        self.shape, self.dtype = tuple(shape), dtype
        self.numel = int(np.prod(shape))
        self.base = torch.empty(self.numel + 2 * GUARD, dtype=dtype, device=dev)
        self.ptr = C.c_void_p(self.base.data_ptr() + GUARD * self.base.element_size())

    def reset(self):
        self.base.fill_(SENTINEL[self.dtype])

    def read(self, what):
        a = self.base.cpu().numpy()
        s = np.asarray(SENTINEL[self.dtype], dtype=a.dtype)
        lo, hi = a[:GUARD], a[GUARD + self.numel:]
        assert (lo == s).all(), f"{what}: {(lo != s).sum()} elements of the guard band BELOW the tensor were written"
        assert (hi == s).all(), f"{what}: {(hi != s).sum()} elements of the guard band ABOVE the tensor were written"
        return a[GUARD:GUARD + self.numel].reshape(self.shape).view(NP[self.dtype])


def explain(env, name, got, ref, d, r):
    """First differing element of `name`, the reference's contributing terms, and which planted mutation of the reference (a
    wrong tie rule / upsample shift / halo column / channel pair, or ONE weight of that layer dropped) gives the kernel's value."""
    bad = np.argwhere(got != ref)
    at = tuple(int(i) for i in bad[0])
    lines = [f"{len(bad)}/{got.size} elements differ; first at (image, y, x, channel ...) = {at}: kernel {got[at]!r}, reference {ref[at]!r}"]
    params, e0 = env["refs"].params[d], r["e0"]
    layer = {"e1": "features.3", "am1": "features.3", "e2": "features.6", "am2": "features.6", "e3": "features.10", "am3": "features.10",
             "e4": "features.14", "h1": "crit.1", "pred": "crit.4", "o4": "dec_model.4", "o3": "dec_model.3", "o2": "dec_model.2",
             "o1": "dec_model.1", "o0": "dec_model.0"}[name]
    which = 0 if layer.startswith(("features", "crit")) else 1
    w = params[which][layer + ".weight"]
    if not name.startswith("am") and name != "pred":
        o = at[-1]
        lines.append(f"{layer}: output channel {o} reads weights (in-channel, ky, kx) -> w: "
                     + ", ".join(f"{tuple(int(i) for i in ix)} -> {w[o][tuple(ix)]}" for ix in np.argwhere(w[o] != 0))
                     + f"; bias {params[which][layer + '.bias'][o]}")
    img = slice(at[0], at[0] + 1)
    e0i = e0[img]
    local = (0,) + at[1:]
    cast = lambda v: v if name.startswith("am") else v.astype(got.dtype)
    hits = []
    for mut in X.MUTATIONS:
        if cast(X.forward(params, e0i, mut=mut)[name])[local] == got[at]:
            hits.append(mut)
    for ix in np.argwhere(w != 0):
        q = (dict(params[0]), dict(params[1]))
        q[which][layer + ".weight"] = w.copy()
        q[which][layer + ".weight"][tuple(ix)] = 0.0
        if cast(X.forward(q, e0i)[name])[local] == got[at]:
            hits.append(f"{layer}.weight{tuple(int(i) for i in ix)} dropped")
    lines.append("reference mutations that reproduce the kernel's value: " + (", ".join(hits) if hits else "none of those tried"))
    return "\n".join(lines)


def compare(env, name, got, r, d, n, form):
    what = f"{form} draw {d} n={n}: {name}"
    if name == "pred":
        ref = r["pred"]
        err = np.abs(got.astype(np.float64) - ref)
        bound = 4 * 2.0 ** -23 * ref
        assert (err <= bound).all(), f"{what}: worst |pred - ref| / ref = {(err / ref).max() / 2.0 ** -23:.2f} x 2^-23 (bound 4)"
        return
    ref = r[name] if name.startswith("am") else r[name].astype(got.dtype)        # exact: check_exactness (a)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    if not np.array_equal(got, ref):
        raise AssertionError(f"{what} is not bit-identical to the float64 reference\n" + explain(env, name, got, ref, d, r))


def run_form(env, form, inputs, outputs, launch, big=N_BIG):
    """inputs: name -> dtype (reference tensors uploaded as that type); outputs: name -> dtype (guarded, compared).
    launch(n, I, O): the C ABI call(s), I / O = name -> c_void_p."""
    dev, refs = env["dev"], env["refs"]
    groups = [(3, list(range(X.N_DRAWS)), None), (1, [0], None), (big, [0], None if big == N_BIG else big)]
    single = {}                                       # (image of the big batch) -> its outputs when run alone
    for n, draws, first in groups:
        out = {k: Guarded((n,) + shape_of(k)[1:], dt, dev) for k, dt in outputs.items()}
        for d in draws:
            r = refs.get(d, n if first is None else N_BIG, first)
            load_params(env, d)
            I = {k: torch.from_numpy(r[k]).to(device=dev, dtype=dt).contiguous() for k, dt in inputs.items()}
            for g in out.values():
                g.reset()
            launch(n, {k: C.c_void_p(t.data_ptr()) for k, t in I.items()}, {k: g.ptr for k, g in out.items()})
            torch.cuda.synchronize()
            got = {k: out[k].read(f"{form} draw {d} n={n}: {k}") for k in ORDER if k in out}
            for k, v in got.items():
                compare(env, k, v, r, d, n, form)
            if n >= 1024:                             # the same images alone: same bits, whichever workgroup and round took them
                one = {k: Guarded((1,) + shape_of(k)[1:], dt, dev) for k, dt in outputs.items()}
                for i in (0, n // 2, n - 1):
                    Ii = {k: t[i:i + 1].contiguous() for k, t in I.items()}
                    for g in one.values():
                        g.reset()
                    launch(1, {k: C.c_void_p(t.data_ptr()) for k, t in Ii.items()}, {k: g.ptr for k, g in one.items()})
                    torch.cuda.synchronize()
                    for k, g in one.items():
                        alone = g.read(f"{form} image {i} alone: {k}")
                        assert np.array_equal(alone[0], got[k][i]), f"{form}: {k} of image {i} differs between the n={n} batch and n=1"


SHAPES = {"e0": (0, 32, 32, 8), "e1": (0, 16, 16, 8), "am1": (0, 16, 16, 1), "e2": (0, 8, 8, 8), "am2": (0, 8, 8, 1), "e3": (0, 4, 4, 16),
          "am3": (0, 4, 4, 2), "e4": (0, 32), "h1": (0, 32), "pred": (0,), "o4": (0, 32), "o3": (0, 4, 4, 16), "o2": (0, 8, 8, 8),
          "o1": (0, 16, 16, 8), "o0": (0, 32, 32, 8)}


def shape_of(k):
    return SHAPES[k]


def test_reference_shapes_are_the_kernels(env):
    r = env["refs"].get(0, 3)
    for k, s in SHAPES.items():
        assert r[k].shape == (3,) + s[1:], (k, r[k].shape)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def wc(env, key):
    return C.c_void_p(env["fc"].data_ptr() + 4 * env["lc"].off(key))


def wm(env, key):
    return C.c_void_p(env["fm"].data_ptr() + 4 * env["lm"].off(key))


def enc_w(env):
    return env["hg"].tail_enc_weights(env["fc"], env["lc"], pw=(wm(env, "dec_model.4.weight").value, wm(env, "dec_model.4.bias").value))


def dec_w(env):
    return env["hg"].tail_dec_weights(env["fm"], env["lm"])


ENC_OUT = {"e2": F32, "am2": U32, "e3": F32, "am3": U32, "e4": F32, "h1": F32, "pred": F32, "o4": F32}
DEC_IN = {"e1": F32, "e2": F32, "e3": F32, "o4": F32}
DEC_OUT = {"o3": F32, "o2": F32, "o1": F32}


def test_conv3x3_fwd_features3(env):
    L = env["lib"]

    def launch(n, I, O):
        d = L.ConvDesc(n, 32, 32, 8, 0, 8, L.SRC_F32, 2, L.ACT_RELU, 1, L.Dropout())
        L.call("cgs_conv3x3_fwd", C.byref(d), I["e0"], None, wc(env, "features.3.weight"), wc(env, "features.3.bias"), O["e1"], O["am1"], stream())
    run_form(env, "cgs_conv3x3_fwd(features.3)", {"e0": F32}, {"e1": F32, "am1": U32}, launch)


def test_conv3x3_fwd_dec_model0(env):
    L = env["lib"]

    def launch(n, I, O):
        d = L.ConvDesc(n, 32, 32, 8, 8, 8, L.SRC_F32, 2, L.ACT_NONE, 0, L.Dropout())
        L.call("cgs_conv3x3_fwd", C.byref(d), I["e0"], I["o1"], wm(env, "dec_model.0.weight"), wm(env, "dec_model.0.bias"), O["o0"], None, stream())
    run_form(env, "cgs_conv3x3_fwd(dec_model.0)", {"e0": F32, "o1": F32}, {"o0": F32}, launch)


def test_enc1_tail_fwd(env):
    L = env["lib"]
    nd = L.Dropout()

    def launch(n, I, O):
        tw = enc_w(env)
        L.call("cgs_enc1_tail_fwd", n, C.byref(tw), I["e0"], wc(env, "features.3.weight"), wc(env, "features.3.bias"), O["e1"], O["am1"],
               O["e2"], O["am2"], O["e3"], O["am3"], O["e4"], O["h1"], O["pred"], O["o4"], nd, nd, nd, stream())
    run_form(env, "cgs_enc1_tail_fwd", {"e0": F32}, dict(ENC_OUT, e1=F32, am1=U32), launch)


@pytest.mark.parametrize("with_o4", [True, False])
def test_tail_enc_fwd(env, with_o4):
    L = env["lib"]
    nd = L.Dropout()
    outs = {k: v for k, v in ENC_OUT.items() if with_o4 or k != "o4"}

    def launch(n, I, O):
        tw = enc_w(env)
        L.call("cgs_tail_enc_fwd", n, C.byref(tw), I["e1"], O["e2"], O["am2"], O["e3"], O["am3"], O["e4"], O["h1"], O["pred"], O.get("o4"),
               nd, nd, nd, stream())
    run_form(env, f"cgs_tail_enc_fwd(o4={with_o4})", {"e1": F32}, outs, launch)


@pytest.mark.parametrize("entry", ["cgs_tail_dec_fwd", "cgs_tail_dec_fwd_pack"])
def test_tail_dec_fwd(env, entry):
    L = env["lib"]

    def launch(n, I, O):
        td = dec_w(env)
        extra = (None, None) if entry == "cgs_tail_dec_fwd_pack" else ()          # w_m0, m0_pack = NULL
        L.call(entry, n, C.byref(td), I["e1"], I["e2"], I["e3"], I["o4"], O["o3"], O["o2"], O["o1"], *extra, stream())
    run_form(env, entry, DEC_IN, DEC_OUT, launch)


def test_tail_dec_fwd_dec0(env):
    """One workgroup per image up to the documented limit of 1024 images; beyond it CGS_ERR_UNSUPPORTED and nothing written."""
    L = env["lib"]

    def launch(n, I, O):
        td = dec_w(env)
        L.call("cgs_tail_dec_fwd_dec0", n, C.byref(td), I["e0"], I["e1"], I["e2"], I["e3"], I["o4"], O["o3"], O["o2"], O["o1"],
               wm(env, "dec_model.0.weight"), wm(env, "dec_model.0.bias"), O["o0"], None, None, stream())
    run_form(env, "cgs_tail_dec_fwd_dec0", dict(DEC_IN, e0=F32), dict(DEC_OUT, o0=F32), launch, big=1024)
    buf = torch.zeros(64, device=env["dev"])
    p = C.c_void_p(buf.data_ptr())
    td = dec_w(env)
    rc = L.load().cgs_tail_dec_fwd_dec0(N_BIG, C.byref(td), p, p, p, p, p, p, p, p, p, p, p, None, None, stream())
    torch.cuda.synchronize()
    assert rc == L.ERR_UNSUPPORTED and not buf.any()


def test_f16_enc1_fwd(env):
    L = env["lib"]

    def launch(n, I, O):
        L.call("cgs_f16_enc1_fwd", n, I["e0"], wc(env, "features.3.weight"), wc(env, "features.3.bias"), O["e1"], stream())
    run_form(env, "cgs_f16_enc1_fwd", {"e0": F16}, {"e1": F32}, launch)


def test_f16_dec0_fwd(env):
    L = env["lib"]

    def launch(n, I, O):
        L.call("cgs_f16_dec0_fwd", n, I["e0"], I["o1"], wm(env, "dec_model.0.weight"), wm(env, "dec_model.0.bias"), O["o0"], stream())
    run_form(env, "cgs_f16_dec0_fwd", {"e0": F16, "o1": F32}, {"o0": F16}, launch)


@pytest.mark.parametrize("decoder", [True, False])
def test_tail_infer_h16(env, decoder):
    L = env["lib"]
    outs = {"pred": F32, "o1": F32} if decoder else {"pred": F32}

    def launch(n, I, O):
        tw, td = enc_w(env), dec_w(env)
        L.call("cgs_tail_infer_h16", n, C.byref(tw), C.byref(td) if decoder else None, I["e1"], O["pred"], O.get("o1"), stream())
    run_form(env, f"cgs_tail_infer_h16(decoder={decoder})", {"e1": F32}, outs, launch)
