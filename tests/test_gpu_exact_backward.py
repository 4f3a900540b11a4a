"""Every hand-written BACKWARD form of the layers from o0 / pred back to e0 (32x32x8), called through the C ABI on the dyadic fixture of
tests/exact_ref.py with the cotangents of tests/exact_bwd_ref.py, and compared BIT FOR BIT with the float64 backward reference.

On that fixture nothing rounds in fp32 (every data gradient is a multiple of 1/4, every weight gradient of 1/16, every sum of absolute
terms stays below 2^22 quanta; tests/test_exact_bwd_host.py asserts the conditions and that the reference equals float64 autograd), so
there is no tolerance: whatever a form's summation order, its partition of the images over workgroups and slab rows, or its launch form,
every tensor it writes equals the reference cast to fp32.  Each form gets REFERENCE tensors as inputs, so each is tested on its own.

Weight gradients are checked three ways: every slab row the form's *_slabs(n) function reports was written (no sentinel left), the float64
sum of the rows equals the reference, and cgs_reduce_slabs over the rows gives the reference's fp32 bits.

Cases of every form: all 108 draws at n = 3 (over the draws every weight element is non-zero at least once); draws 0..3 at n = 3 with Dropout
p = 1/2 at all three sites (keep scale exactly 2; the kernels' own masks, exported with cgs_dropout_mask, go into the reference); draw 0 at
n = 1, n = 600 (above the 512-image cap of the one-workgroup-per-image decoder form) and n = 1100 (above the 768-workgroup cap of the tail
kernels).  In the large batches at most eight images carry non-zero cotangents -- images 0, n - 1 and s - 1, s, s + 1 for every slab count
s < n the form reports -- so the n = 3 bounds hold; all other images have real activations and zero cotangents: every image's share must
arrive, an idle image must contribute exactly zero.  Three images of a large batch are also run alone (n = 1) against the reference of that
image alone; their data gradients are the same rows of the same reference, so batch and single run have the same bits.
The target modes of the tail kernels (d loss / d pred derived in the kernel) give every image a non-zero cotangent, so they run at n <= 3.
The n = 3 cases rotate through a form's variants by their position; the variants of the large batches are chosen by name (big_i,
BIG_TAIL_ENC).  The references of a large batch are computed on its carrying images alone and scattered into zeros.
Every output sits between two guard bands of 256 sentinel elements inside one allocation; outputs and slab rows are pre-filled with the
sentinel; the bands must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_ref as X
import exact_bwd_ref as B

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = -12345.0
N_BIG = 1100
BIG = (600, N_BIG)
HEAD_SLAB, PW_SLAB = 9313, 1056
SHAPE = {"de0": (32, 32, 8), "dE0": (32, 32, 8), "de1": (16, 16, 8), "dE1": (16, 16, 8), "do1": (16, 16, 8), "de2": (8, 8, 8), "dE2": (8, 8, 8),
         "do2": (8, 8, 8), "de3": (4, 4, 16), "dE3": (4, 4, 16), "do3": (4, 4, 16), "d_o4": (32,), "de4_dec": (32,), "hvec": (384,)}


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Buf:
    """An fp32 output inside one larger allocation, 256 sentinel elements on each side (and the sentinel in the body before a launch)."""

    def __init__(self, shape, dev):
        self.shape = tuple(int(s) for s in shape)
        self.numel = int(np.prod(self.shape))
        self.base = torch.empty(self.numel + 2 * GUARD, dtype=torch.float32, device=dev)
        self.t = self.base[GUARD:GUARD + self.numel].view(self.shape)
        self.ptr = C.c_void_p(self.t.data_ptr())
        self.base.fill_(SENT)

    def read(self, what):
        a = self.base.cpu().numpy()
        lo, hi = a[:GUARD], a[GUARD + self.numel:]
        assert (lo == SENT).all(), f"{what}: {(lo != SENT).sum()} elements of the guard band BELOW the tensor were written"
        assert (hi == SENT).all(), f"{what}: {(hi != SENT).sum()} elements of the guard band ABOVE the tensor were written"
        return a[GUARD:GUARD + self.numel].reshape(self.shape)


def scatter(gs, idx, n, e3):
    """The gradients gs of the carrying images idx as those of the n-image batch: the data rows of every other image are zero (hvec keeps
    their activations e3), the weight gradients are the carrying images' own."""
    g = {}
    for k, v in gs.items():
        if k.startswith("g_"):
            g[k] = v
        else:
            g[k] = np.zeros((n,) + v.shape[1:])
            g[k][idx] = v
    if "hvec" in g:
        g["hvec"][:, :256] = e3.reshape(n, 256)
    return g


class Case:
    """One (draw, batch) of the fixture: forward tensors r, gradients g (float64, left unchanged), Dropout masks, device copies on demand.
    sub = (idx, case of the images idx alone): a large batch whose cotangents sit on the images idx only."""

    def __init__(self, env, d, n, r, g, masks=None, drops=None, tag="", explainable=True, sub=None):
        self.env, self.d, self.n, self.r, self.g, self.masks, self.tag, self.sub = env, d, n, r, g, masks, tag, sub
        self.drops = drops if drops is not None else (env["lib"].Dropout(),) * 3
        self.explainable = explainable
        self._dev, self._mut, self._hold = {}, {}, []

    def hold(self, t):
        """Keeps a temporary device tensor alive until the case's launches have run (a pointer alone does not)."""
        self._hold.append(t)
        return t

    def release(self):
        """Drops the device copies (a large batch is built for one test and not kept)."""
        self._hold.clear()
        self._dev.clear()

    def carrying(self, k):
        """The images < k that can have a non-zero gradient."""
        return np.arange(k) if self.sub is None else self.sub[0][self.sub[0] < k]

    def __str__(self):
        return f"draw {self.d} n={self.n}{self.tag}"

    def f(self, name):
        """r[name] / g[name] as a device tensor (fp32; the argmax words as int32)."""
        if name not in self._dev:
            v = self.r[name] if name in self.r else self.g[name]
            t = torch.from_numpy(v.view(np.int32)) if v.dtype == np.uint32 else torch.from_numpy(v).float()
            self._dev[name] = t.to(self.env["dev"]).contiguous()
        return self._dev[name]

    def up(self, v):
        return self.hold(torch.from_numpy(np.ascontiguousarray(v)).float().to(self.env["dev"]))

    def mutated(self, mut):
        """(r, g) of the reference with a planted mutation (None: the reference), on the same inputs; for explain()."""
        if mut is None:
            return self.r, self.g
        if mut not in self._mut:
            r = self.r
            if mut == "tie_last":
                r = B.forward(self.env["refs"].params[self.d], self.r["e0"], self.masks, mut=mut)
            self._mut[mut] = (r, B.backward(self.env["refs"].params[self.d], r, self.r["dy_o0"], self.r["dpred"], self.masks, mut=mut))
        return self._mut[mut]

    def enc(self, mut=None, n_add=None, keys=("dE0", "dE1", "dE2", "dE3", "de4_dec"), dpred=None, head_only=False):
        """The critic half with the decoder's gradients `keys` arriving for images < n_add only."""
        n_add = self.n if n_add is None else n_add
        if self.sub is not None:                                                   # the carrying images alone, scattered into zeros
            idx, s = self.sub
            assert mut is None and dpred is None
            return scatter(s.enc(None, int(np.searchsorted(idx, n_add)), keys, head_only=head_only), idx, self.n, self.r["e3"])
        r, g = self.mutated(mut)
        sk = {}
        for k in keys:
            sk[k] = g[k].copy()
            sk[k][n_add:] = 0.0
        return B.encoder(self.env["refs"].params[self.d], r, self.r["dpred"] if dpred is None else dpred, sk, self.masks, mut, head_only=head_only)


class Refs:
    """The float64 references, computed once and left unchanged."""

    def __init__(self, env):
        self.env = env
        self.params = {d: X.dyadic_params(d) for d in range(X.N_DRAWS)}
        self.small = []
        for d in range(X.N_DRAWS):
            _, r, g = B.run(d, 3)
            self.small.append(Case(env, d, 3, r, g))
        L, hg, dev = env["lib"], env["hg"], env["dev"]
        self.step = torch.full((1,), 7, dtype=torch.int64, device=dev)
        for d in B.DROP_DRAWS:
            drops, masks = [], []
            for site, shape in ((hg.DROP_SITE_E2, (3, 8, 8, 8)), (hg.DROP_SITE_E3, (3, 4, 4, 16)), (hg.DROP_SITE_H1, (3, 32))):
                dd = L.Dropout(0.5, site, 4321 + d, self.step.data_ptr(), 0, 0)
                out = torch.empty(int(np.prod(shape)), device=dev)
                L.call("cgs_dropout_mask", dd, out.numel(), P(out), stream())
                m = out.cpu().numpy().astype(np.float64).reshape(shape)
                assert set(np.unique(m)) <= {0.0, 2.0}, "p = 1/2: the keep multiplier is exactly 2"
                drops.append(dd)
                masks.append(m)
            _, r, g = B.run(d, 3, masks=tuple(masks))
            B.check_exactness_bwd(self.params[d], r, g, tuple(masks))          # (the CPU test checks stand-in masks; these are the kernels' own)
            rt = dict(r, dpred=B.target_dpred(d, r["dpred"]))                  # and with the cotangent the target modes derive
            B.check_exactness_bwd(self.params[d], rt, B.backward(self.params[d], rt, rt["dy_o0"], rt["dpred"], tuple(masks)), tuple(masks))
            self.small.append(Case(env, d, 3, r, g, tuple(masks), tuple(drops), tag=" dropout"))
        _, r, g = B.run(0, 1)
        self.small.append(Case(env, 0, 1, r, g))
        self.rbig = B.forward(self.params[0], X.dyadic_e0(0, N_BIG))
        self._big = {}

    def big(self, n, carry):
        """(the n-image case whose cotangents sit on `carry`, three of its images as single-image cases).  Only the carrying images'
        reference is kept; the n-image tensors are built for the caller, who drops them after use."""
        carry = tuple(sorted(list(dict.fromkeys(c for c in carry if 0 <= c < n))[:8]))
        env, Pm, idx = self.env, self.params[0], list(carry)
        if (n, carry) not in self._big:
            rs = {k: v[idx] for k, v in self.rbig.items()}
            rs["dy_o0"], rs["dpred"] = B.cotangents(0, len(idx))
            gs = B.backward(Pm, rs, rs["dy_o0"], rs["dpred"])
            B.check_exactness_bwd(Pm, rs, gs)                                      # the carrying images alone are an n <= 8 batch
            singles = []
            for j in sorted({0, len(idx) // 2, len(idx) - 1}):
                r1 = {k: v[j:j + 1] for k, v in rs.items()}
                singles.append(Case(env, 0, 1, r1, B.backward(Pm, r1, r1["dy_o0"], r1["dpred"]), tag=f" (image {idx[j]} of the n={n} batch alone)"))
            self._big[(n, carry)] = (Case(env, 0, len(idx), rs, gs, tag=f" (images {idx} of the n={n} batch)"), singles)
        sub, singles = self._big[(n, carry)]
        r = {k: v[:n] for k, v in self.rbig.items()}
        r["dy_o0"], r["dpred"] = np.zeros((n, 32, 32, 8)), np.zeros(n)
        r["dy_o0"][idx], r["dpred"][idx] = sub.r["dy_o0"], sub.r["dpred"]
        g = scatter(sub.g, idx, n, r["e3"])                                        # an idle image still has its activations in hvec
        return Case(env, 0, n, r, g, tag=f" cotangents on images {idx}", explainable=False, sub=(np.asarray(idx), sub)), singles


@pytest.fixture(scope="module")
def env():
    from cgs_amd import _lib, spec
    from cgs_amd import hourglass as hg
    dev = torch.device("cuda:0")
    lc, lm = spec.critic_layout(), spec.masker_layout()
    e = dict(lib=_lib, hg=hg, dev=dev, lc=lc, lm=lm, fc=torch.zeros(lc.total, device=dev), fm=torch.zeros(lm.total, device=dev),
             fc_host=torch.zeros(lc.total), fm_host=torch.zeros(lm.total), red=torch.zeros(HEAD_SLAB, device=dev), loaded=None)
    _lib.load()
    e["refs"] = Refs(e)
    return e


def load_params(env, d):
    """The draw's reference-convention (OIHW) parameters through spec's layout conversion into the flat kernel-layout buffers."""
    if env["loaded"] == d:
        return
    pc, pm = env["refs"].params[d]
    env["lc"].flatten({k: torch.from_numpy(v) for k, v in pc.items()}, env["fc_host"])
    env["lm"].flatten({k: torch.from_numpy(v) for k, v in pm.items()}, env["fm_host"])
    env["fc"].copy_(env["fc_host"])
    env["fm"].copy_(env["fm_host"])
    env["loaded"] = d


def wc(env, key):
    return C.c_void_p(env["fc"].data_ptr() + 4 * env["lc"].off(key))


def wm(env, key):
    return C.c_void_p(env["fm"].data_ptr() + 4 * env["lm"].off(key))


def explain(got, ref, ref_of_mut, c):
    """First differing element, and which planted mutation of the reference gives the kernel's value there."""
    bad = np.argwhere(got != ref)
    at = tuple(int(i) for i in bad[0])
    lines = [f"{len(bad)}/{got.size} elements differ; first at index (image / slab position first) {at}: kernel {got[at]!r}, reference {ref[at]!r}"]
    if ref_of_mut is not None and c.explainable:
        hits = []
        for mut in B.MUTATIONS:
            m = ref_of_mut(mut)
            if m is not None and m.shape == ref.shape and np.float32(m[at]) == got[at]:
                hits.append(mut)
        lines.append("reference mutations that reproduce the kernel's value: " + (", ".join(hits) if hits else "none of those tried"))
    return "\n".join(lines)


def expect(c, form, name, buf, ref, ref_of_mut=None):
    """A data tensor: bit-identical to the reference cast to fp32 (exact: the CPU test asserts the cast loses nothing)."""
    what = f"{form} {c}: {name}"
    got = buf.read(what)
    ref = np.asarray(ref).reshape(got.shape)
    if not np.array_equal(got, ref.astype(np.float32)):
        rm = (lambda mut: np.asarray(ref_of_mut(mut)).reshape(got.shape)) if ref_of_mut is not None else None
        raise AssertionError(f"{what} is not bit-identical to the float64 reference\n" + explain(got, ref.astype(np.float32), rm, c))


def expect_untouched(c, form, name, buf):
    assert (buf.read(f"{form} {c}: {name}") == SENT).all(), f"{form} {c}: {name} was written"


def expect_slab(c, form, name, buf, ref, ref_of_mut=None):
    """buf [rows reported by the form][count]: all rows written, their float64 sum is the reference, cgs_reduce_slabs gives its fp32 bits."""
    env = c.env
    what = f"{form} {c}: {name}"
    rows = buf.read(what)
    left = np.argwhere(rows == SENT)
    assert len(left) == 0, f"{what}: {len(left)} elements of the {rows.shape[0]} reported rows still hold the sentinel, first (row, element) {left[0].tolist()}"
    tot = rows.astype(np.float64).sum(0)
    if not np.array_equal(tot, ref):
        raise AssertionError(f"{what}: the float64 sum of the {rows.shape[0]} slab rows is not the reference\n" + explain(tot, ref, ref_of_mut, c))
    plan = env["hg"].SlabPlan()
    plan.add(buf.t, rows.shape[0], rows.shape[1], 0)
    env["red"].fill_(SENT)
    plan.build(env["red"]).run()
    torch.cuda.synchronize()
    red = env["red"].cpu().numpy()[:rows.shape[1]]
    assert np.array_equal(red, ref.astype(np.float32)), f"{what}: cgs_reduce_slabs over the rows differs from the reference at {np.argwhere(red != ref.astype(np.float32))[:3].tolist()}"


def run_form(env, fn, slab_counts=None, big=BIG, big_i=None):
    """fn(case, i): launches and assertions of one form on one case; i selects among the form's variants.  The small cases rotate through
    them by position; the large batch big[j] runs variant big_i[j] (default 0), its single images the variants 0, 1, 2.  slab_counts(n): the
    slab counts the form reports at n (they place the cotangent-carrying images of the large batches)."""
    refs = env["refs"]
    for i, c in enumerate(refs.small):
        load_params(env, c.d)
        fn(c, i)
        c._hold.clear()
    load_params(env, 0)
    for j, n in enumerate(big):
        s = [int(x) for x in (slab_counts(n) if slab_counts else ()) if 0 < int(x) < n]
        carry = [0, n - 1] + [x + k for x in s for k in (-1, 0, 1)]          # at most eight: the first and last image, then the counts in the order given
        case, singles = refs.big(n, carry)
        fn(case, big_i[j] if big_i else 0)
        case.release()
        del case
        for k, c in enumerate(singles):
            fn(c, k)
            c._hold.clear()


def sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# stand-alone convolution backward
# ---------------------------------------------------------------------------------------------------------------------------------
ENC_I = {"features.3": 1, "features.6": 2, "features.10": 3}
DEC_I = {"dec_model.0": 0, "dec_model.1": 1, "dec_model.2": 2, "dec_model.3": 3}
CONV_LAYERS = tuple(ENC_I) + tuple(DEC_I)


def layer_row(env, key):
    """hourglass' table row of a layer: (key, hw, ca, cb, co, upsample, activation, pool, dropout site)."""
    return env["hg"].ENC_LAYERS[ENC_I[key]] if key in ENC_I else env["hg"].DEC_LAYERS[3 - DEC_I[key]]


def layer_desc(env, key, n, drop=None):
    _k, hw, ca, cb, co, ups, act, pool, _site = layer_row(env, key)
    return env["hg"].conv_desc(n, hw, ca, cb, co, False, ups, act, pool, drop if drop is not None else env["lib"].Dropout())


class ConvLayer:
    """Descriptor, inputs and expected outputs of one layer's stand-alone backward on a case."""

    def __init__(self, env, c, key):
        L = env["lib"]
        self.key, self.enc = key, key in ENC_I
        n = c.n
        _k, hw, ca, cb, co, ups, act, pool, site = layer_row(env, key)
        if self.enc:
            i = self.i = ENC_I[key]
            drop = c.drops[0] if site is not None else L.Dropout()
            self.src_a, self.src_b, self.dy, self.am = c.f(f"e{i - 1}"), None, c.f(f"de{i}"), c.f(f"am{i}")
            self.w = wc(env, key + ".weight")
            self.da_name, self.db_name, self.add_name = f"de{i - 1}", None, f"dE{i - 1}"
        else:
            i = self.i = DEC_I[key]
            drop = L.Dropout()
            self.src_a, self.src_b = c.f(f"e{i}"), c.f(("o1", "o2", "o3", "o4")[i])
            self.dy, self.am = c.f(("dy_o0", "do1", "do2", "do3")[i]), None
            self.w = wm(env, key + ".weight")
            self.da_name, self.db_name, self.add_name = f"dE{i}", ("do1", "do2", "do3", "d_o4")[i], f"e{i}"
        self.desc = layer_desc(env, key, n, drop)
        self.count = 9 * (ca + cb) * co + co
        self.slab_name = B.SLABS[key]
        self.a_shape = (n, hw, hw, ca)
        self.b_shape = (n, 32) if ups == 4 else (n, hw // 2, hw // 2, cb)

    def expected_a(self, c, n_add, mut=None):
        """d_a with the addend arriving for images < n_add (encoder: the decoder's skip gradient; decoder layers: the skip activation)."""
        r, g = c.mutated(mut)
        if self.enc:
            add = g[self.add_name].copy()
            conv = g[self.da_name] - add
        else:
            add = r[self.add_name].copy()
            conv = g[self.da_name]
        add[n_add:] = 0.0
        return conv + add


def n_add_of(n, i):
    return (n, n - 1, 0)[i % 3]


@pytest.mark.parametrize("key", CONV_LAYERS)
def test_conv3x3_bwd_data(env, key):
    L = env["lib"]

    def fn(c, i):
        cl = ConvLayer(env, c, key)
        form = f"cgs_conv3x3_bwd_data({key})"
        n_add = n_add_of(c.n, i)
        alias = (i // 3) % 2 == 1
        which = "both" if cl.enc else ("both", "a", "b")[(i // 2) % 3]
        add_src = c.f(cl.add_name)
        da = Buf(cl.a_shape, c.env["dev"]) if which != "b" else None
        db = Buf(cl.b_shape, c.env["dev"]) if (cl.db_name and which != "a") else None
        addend = None
        if da is not None:
            if alias:
                da.t.copy_(add_src)
                addend = da.ptr
            else:
                addend = P(add_src) if n_add > 0 else None
        L.call("cgs_conv3x3_bwd_data", C.byref(cl.desc), P(cl.dy), P(cl.am), cl.w, None, L.ACT_NONE, addend, n_add if da is not None else 0,
               da.ptr if da else None, db.ptr if db else None, stream())
        sync()
        v = f" n_addend={n_add} alias={alias} outputs={which}"
        if da is not None:
            expect(c, form + v, cl.da_name, da, cl.expected_a(c, n_add), lambda mut: cl.expected_a(c, n_add, mut))
        if db is not None:
            expect(c, form + v, cl.db_name, db, c.g[cl.db_name], lambda mut: c.mutated(mut)[1][cl.db_name])
    run_form(env, fn, big_i=(1, 3))          # n = 600: n_addend = n - 1, both outputs; n = 1100: n_addend = n aliasing d_a, d_a only (decoder layers)


@pytest.mark.parametrize("key", CONV_LAYERS)
def test_conv3x3_bwd_weight(env, key):
    L = env["lib"]

    def fn(c, i):
        cl = ConvLayer(env, c, key)
        nsl = L.load().cgs_conv3x3_bwd_weight_slabs(C.byref(cl.desc))
        assert nsl > 0
        slab = Buf((nsl, cl.count), c.env["dev"])
        L.call("cgs_conv3x3_bwd_weight", C.byref(cl.desc), P(cl.src_a), P(cl.src_b), P(cl.dy), P(cl.am), slab.ptr, stream())
        sync()
        expect_slab(c, f"cgs_conv3x3_bwd_weight({key})", cl.slab_name, slab, c.g[cl.slab_name], lambda mut: c.mutated(mut)[1][cl.slab_name])
    run_form(env, fn, lambda n: [L.load().cgs_conv3x3_bwd_weight_slabs(C.byref(layer_desc(env, key, n)))])


@pytest.mark.parametrize("key", CONV_LAYERS)
def test_conv3x3_bwd_both(env, key):
    L = env["lib"]

    def fn(c, i):
        cl = ConvLayer(env, c, key)
        form = f"cgs_conv3x3_bwd_both({key})"
        nsl = L.load().cgs_conv3x3_bwd_both_slabs(C.byref(cl.desc))
        assert nsl > 0
        n_add = n_add_of(c.n, i) if cl.enc else 0
        slab, da = Buf((nsl, cl.count), c.env["dev"]), Buf(cl.a_shape, c.env["dev"])
        db = Buf(cl.b_shape, c.env["dev"]) if cl.db_name else None
        L.call("cgs_conv3x3_bwd_both", C.byref(cl.desc), P(cl.src_a), P(cl.src_b), P(cl.dy), P(cl.am), cl.w, P(c.f(cl.add_name)) if n_add > 0 else None,
               n_add, da.ptr, db.ptr if db else None, slab.ptr, stream())
        sync()
        expect(c, form + f" n_addend={n_add}", cl.da_name, da, cl.expected_a(c, n_add), lambda mut: cl.expected_a(c, n_add, mut))
        if db is not None:
            expect(c, form, cl.db_name, db, c.g[cl.db_name], lambda mut: c.mutated(mut)[1][cl.db_name])
        expect_slab(c, form, cl.slab_name, slab, c.g[cl.slab_name], lambda mut: c.mutated(mut)[1][cl.slab_name])
    run_form(env, fn, lambda n: [L.load().cgs_conv3x3_bwd_both_slabs(C.byref(layer_desc(env, key, n)))], big_i=(1, 0))      # n_addend = n - 1 at 600, n at 1100


# ---------------------------------------------------------------------------------------------------------------------------------
# head and 1x1 convolution
# ---------------------------------------------------------------------------------------------------------------------------------
def pred_half(c):
    return c.hold(torch.full((c.n,), 0.5, device=c.env["dev"]))


HEAD_VARIANTS = ("plain", "d_e3_extra", "d_e3_extra aliasing d_e3", "d_e4_extra", "d_o4 + w_pw + slab_pw")


@pytest.mark.parametrize("variant", HEAD_VARIANTS)
def test_head_bwd(env, variant):
    L = env["lib"]
    vi = HEAD_VARIANTS.index(variant)

    def fn(c, i):
        form = f"cgs_head_bwd[{variant}]"
        n_x = 0 if vi == 0 else (c.n, c.n - 1)[i % 2]
        keys = ((), ("dE3",), ("dE3",), ("de4_dec",), ("de4_dec",))[vi]
        ref = lambda mut=None: c.enc(mut, n_x, keys, head_only=True)
        e = ref()
        nsl = L.load().cgs_head_bwd_slabs(c.n)
        de3, slab = Buf((c.n, 4, 4, 16), c.env["dev"]), Buf((nsl, HEAD_SLAB), c.env["dev"])
        slab_pw = Buf((nsl, PW_SLAB), c.env["dev"]) if vi == 4 else None
        x3 = x4 = do4 = None
        if vi == 1 and n_x > 0:
            x3 = P(c.f("dE3"))
        if vi == 2:
            de3.t.copy_(c.f("dE3"))
            x3 = de3.ptr
        if vi == 3 and n_x > 0:
            x4 = P(c.f("de4_dec"))
        if vi == 4:
            do4 = P(c.f("d_o4"))
        L.call("cgs_head_bwd", c.n, P(c.f("e3")), P(c.f("e4")), P(c.f("h1")), P(pred_half(c)), P(c.f("dpred")), x4, x3, n_x,
               wc(env, "features.14.weight"), wc(env, "crit.1.weight"), wc(env, "crit.4.weight"), c.drops[1], c.drops[2], de3.ptr, slab.ptr,
               do4, wm(env, "dec_model.4.weight") if vi == 4 else None, slab_pw.ptr if slab_pw else None, stream())
        sync()
        v = f"{form} n_extra={n_x}"
        expect(c, v, "de3", de3, e["de3"], lambda mut: ref(mut)["de3"])
        expect_slab(c, v, "g_head", slab, e["g_head"], lambda mut: ref(mut)["g_head"])
        if slab_pw is not None:
            expect_slab(c, v, "g_pw", slab_pw, B.pw_slab(c.r["e4"], c.g["d_o4"][:n_x]), lambda mut: B.pw_slab(c.r["e4"], c.mutated(mut)[1]["d_o4"][:n_x], mut))
    run_form(env, fn, lambda n: [L.load().cgs_head_bwd_slabs(n)], big_i=(0, 1))          # extras for all n images at 600, for n - 1 at 1100


def test_pointwise_bwd(env):
    L = env["lib"]

    def fn(c, i):
        nsl = L.load().cgs_pointwise_bwd_slabs(c.n)
        dx, slab = Buf((c.n, 32), c.env["dev"]), Buf((nsl, PW_SLAB), c.env["dev"])
        L.call("cgs_pointwise_bwd", c.n, 32, 32, P(c.f("e4")), P(c.f("d_o4")), wm(env, "dec_model.4.weight"), dx.ptr, slab.ptr, stream())
        sync()
        expect(c, "cgs_pointwise_bwd", "de4_dec", dx, c.g["de4_dec"], lambda mut: c.mutated(mut)[1]["de4_dec"])
        expect_slab(c, "cgs_pointwise_bwd", "g_pw", slab, c.g["g_pw"], lambda mut: c.mutated(mut)[1]["g_pw"])
    run_form(env, fn, lambda n: [L.load().cgs_pointwise_bwd_slabs(n)])


# ---------------------------------------------------------------------------------------------------------------------------------
# encoder tail
# ---------------------------------------------------------------------------------------------------------------------------------
# (loss: dpred given | MSE target | BCE target; n_add index into (n, n - 1, 0); d_o4; slabs; rider: None | (n_r: n or n - 1, rows: all 4 n_r, one,
# or a count); for _enc1, where given: s1 = slab1 formed in the kernel (else NULL), na0 = index of features.3's own addend count)
BIG_TAIL_ENC = (          # the large batches run these two, whatever the number of small cases
    dict(loss="dpred", na=0, pw=True, slabs=True, rider=("n", "all"), s1=True, na0=0),       # the step's own form: slab1 in the kernel, 4 n_r rider rows
    dict(loss="dpred", na=1, pw=True, slabs=True, rider=("n-1", 256), s1=False, na0=2),      # 256 rider rows as the step launches them: several tiles each
)
TAIL_ENC_VARIANTS = (
    dict(loss="dpred", na=0, pw=True, slabs=True, rider=None),
    dict(loss="mse", na=1, pw=True, slabs=True, rider=("n", "all")),
    dict(loss="bce", na=2, pw=False, slabs=True, rider=("n-1", "one")),
    dict(loss="dpred", na=1, pw=False, slabs=False, rider=("n", "one")),
    dict(loss="mse", na=0, pw=False, slabs=True, rider=("n-1", "all")),
    dict(loss="bce", na=1, pw=True, slabs=False, rider=None),
    dict(loss="dpred", na=2, pw=True, slabs=True, rider=("n-1", "all")),
    dict(loss="dpred", na=0, pw=False, slabs=True, rider=("n", "all")),
)


def tail_enc_case(env, c, v, enc1, i, entry):
    """One launch of cgs_tail_enc_bwd / _rider / _enc1 in variant v and its assertions."""
    L, hg, dev = env["lib"], env["hg"], c.env["dev"]
    n = c.n
    loss = v["loss"] if n <= 3 and "alone" not in c.tag else "dpred"          # the target modes give EVERY image a cotangent
    n_add = n_add_of(n, v["na"])
    pw = v["pw"] and n_add > 0
    dpred, target, scale, bce, dp_ref = P(c.f("dpred")), None, 0.0, 0, None
    if loss != "dpred":
        S = B.TARGET_SCALES[c.d % 2]
        dp_ref = B.target_dpred(c.d, c.r["dpred"])                              # pred = 1/2: MSE 2 s (pred - t) = -+s, BCE s (pred - t) / (1/4) = -+2 s;
        target, dpred = c.up((c.r["dpred"] < 0).astype(np.float64)), None       # check_exactness_bwd holds for it (CPU test; Refs for the Dropout group)
        scale, bce = (S, 0) if loss == "mse" else (S / 2, 1)
    keys = tuple(k for k in ("dE0", "dE1", "dE2", "dE3") if enc1 or k != "dE0") + (("de4_dec",) if pw else ())
    n_add0 = n_add_of(n, v.get("na0", i // 3)) if enc1 else 0                     # features.3's own addend count (the ABI takes it separately)
    with_s1 = v.get("s1", i % 2 == 0)

    def ref(mut=None):
        if dp_ref is None and n_add == n and pw:                                   # the step's own form: the case's reference as it stands
            e = dict(c.mutated(mut)[1])                                            # (without enc1, dE0 reaches none of the tensors compared)
        else:
            e = c.enc(mut, n_add, keys, dpred=dp_ref)
        if enc1 and n_add0 != n_add:                                              # de0 = convolution part + dE0 for images < n_add0, not < n_add
            lo, hi = sorted((n_add, n_add0))
            e["de0"] = e["de0"].copy()
            e["de0"][lo:hi] += (1.0 if n_add0 > n_add else -1.0) * c.mutated(mut)[1]["dE0"][lo:hi]
        return e
    e = ref()
    nsl = L.load().cgs_tail_enc_bwd_slabs(n)
    de1, hvec = Buf((n, 16, 16, 8), dev), Buf((n, 384), dev)
    s10 = Buf((nsl, 1168), dev) if v["slabs"] else None
    s6 = Buf((nsl, 584), dev) if v["slabs"] else None
    tw = hg.tail_enc_weights(env["fc"], env["lc"], pw=(wm(env, "dec_model.4.weight").value, wm(env, "dec_model.4.bias").value) if pw else None)
    rider = v["rider"] if entry != "cgs_tail_enc_bwd" else None
    rargs, sr, n_r = (0, None, None, None, None, 0), None, 0
    if rider is not None:
        n_r = n if (rider[0] == "n" or n == 1) else n - 1
        rows = {"all": 4 * n_r, "one": 1}.get(rider[1]) or min(rider[1], 4 * n_r)
        sr = Buf((rows, 1160), dev)
        rargs = (n_r, P(c.f("e0")), P(c.f("o1")), P(c.f("dy_o0")), sr.ptr, rows)
    args = [n, C.byref(tw), P(c.f("e1")), P(c.f("e2")), P(c.f("am2")), P(c.f("e3")), P(c.f("am3")), P(c.f("e4")), P(c.f("h1")), P(pred_half(c)),
            dpred, P(target), scale, bce, P(c.f("dE1")) if n_add else None, P(c.f("dE2")) if n_add else None, P(c.f("dE3")) if n_add else None,
            P(c.f("d_o4")) if pw else None, n_add, de1.ptr, hvec.ptr if v["slabs"] else None, s10.ptr if s10 else None, s6.ptr if s6 else None,
            c.drops[0], c.drops[1], c.drops[2]]
    de0 = s1 = None
    if entry == "cgs_tail_enc_bwd":
        args += [stream()]
    else:
        args += list(rargs)
        if enc1:
            de0 = Buf((n, 32, 32, 8), dev)
            s1 = Buf((nsl, 584), dev) if (v["slabs"] and with_s1) else None
            args += [P(c.f("am1")), wc(env, "features.3.weight"), P(c.f("dE0")) if n_add0 else None, n_add0, de0.ptr,
                     P(c.f("e0")) if s1 else None, s1.ptr if s1 else None]
        args += [stream()]
    L.call(entry, *args)
    sync()
    form = f"{entry}[loss={loss} n_add={n_add} d_o4={pw} slabs={v['slabs']} rider={rider}" + (f" n_addend0={n_add0} slab1={'in kernel' if s1 else 'NULL'}]" if enc1 else "]")
    expect(c, form, "de1", de1, e["de1"], lambda mut: ref(mut)["de1"])
    if v["slabs"]:
        got = hvec.read(f"{form} {c}: hvec")[:, :353]
        if not np.array_equal(got, e["hvec"][:, :353].astype(np.float32)):
            raise AssertionError(f"{form} {c}: hvec[:, :353] is not bit-identical to the reference\n"
                                 + explain(got, e["hvec"][:, :353].astype(np.float32), lambda mut: ref(mut)["hvec"][:, :353], c))
        expect_slab(c, form, "g_enc3 (slab10)", s10, e["g_enc3"], lambda mut: ref(mut)["g_enc3"])
        expect_slab(c, form, "g_enc2 (slab6)", s6, e["g_enc2"], lambda mut: ref(mut)["g_enc2"])
    if sr is not None:
        sel = c.carrying(n_r)                                                    # (dy_o0 of every other image is zero)
        cat, dy_r = np.concatenate((c.r["e0"][sel], X.up(c.r["o1"][sel], 2)), axis=-1), c.r["dy_o0"][sel]
        expect_slab(c, form, "g_dec0 (rider)", sr, B.conv_bwd_weight(cat, dy_r), lambda mut: B.conv_bwd_weight(cat, dy_r, mut))
    if de0 is not None:
        expect(c, form, "de0", de0, e["de0"], lambda mut: ref(mut)["de0"])
    if s1 is not None:
        expect_slab(c, form, "g_enc1 (slab1)", s1, e["g_enc1"], lambda mut: ref(mut)["g_enc1"])


@pytest.mark.parametrize("entry", ["cgs_tail_enc_bwd", "cgs_tail_enc_bwd_rider", "cgs_tail_enc_bwd_enc1"])
def test_tail_enc_bwd(env, entry):
    L = env["lib"]

    def fn(c, i):
        if c.sub is not None:
            vs = BIG_TAIL_ENC
        else:
            vs = [TAIL_ENC_VARIANTS[v] for v in {0, 1 + i % (len(TAIL_ENC_VARIANTS) - 1)}]          # the step's own form on every case, the others in rotation
        for v in vs:
            tail_enc_case(env, c, v, entry.endswith("enc1"), i, entry)
    run_form(env, fn, lambda n: [L.load().cgs_tail_enc_bwd_slabs(n)])


# ---------------------------------------------------------------------------------------------------------------------------------
# head weight gradients: stand-alone and as riders of the features.0 launches
# ---------------------------------------------------------------------------------------------------------------------------------
def head_ranges(c, i):
    """(images in the first range, with d_o4): one range on even i, two on odd (the second is empty at n = 1); d_o4 for i = 0, 1 mod 4."""
    two = i % 2 == 1
    k = c.n if not two else (c.n + 1) // 2
    with_o4 = (i // 2) % 2 == 0
    return k, with_o4


def head_args(c, k, with_o4):
    n = c.n
    hv, e4, do4 = c.f("hvec"), c.f("e4"), c.f("d_o4")
    r0 = (k, P(hv[:k]), P(e4[:k]), P(do4[:k]) if with_o4 else None, k if with_o4 else 0)
    r1 = (n - k, P(hv[k:]), P(e4[k:]), P(do4[k:]) if with_o4 else None, (n - k) if with_o4 else 0) if n > k else (0, None, None, None, 0)
    return list(r0) + list(r1)


def expect_head(c, form, sh, spw, with_o4):
    expect_slab(c, form, "g_head", sh, c.g["g_head"], lambda mut: c.mutated(mut)[1]["g_head"])
    if with_o4:
        expect_slab(c, form, "g_pw", spw, c.g["g_pw"], lambda mut: c.mutated(mut)[1]["g_pw"])


def test_tail_head_wgrad(env):
    L = env["lib"]

    def fn(c, i):
        k, with_o4 = head_ranges(c, i)
        nsl = L.load().cgs_tail_head_wgrad_slabs(c.n)
        sh, spw = Buf((nsl, HEAD_SLAB), c.env["dev"]), Buf((nsl, PW_SLAB), c.env["dev"])
        L.call("cgs_tail_head_wgrad", *head_args(c, k, with_o4), sh.ptr, spw.ptr if with_o4 else None, stream())
        sync()
        expect_head(c, f"cgs_tail_head_wgrad[ranges {k}+{c.n - k} d_o4={with_o4}]", sh, spw, with_o4)
        if not with_o4:
            expect_untouched(c, "cgs_tail_head_wgrad", "slab_pw (not passed)", spw)
    run_form(env, fn, lambda n: [L.load().cgs_tail_head_wgrad_slabs(n)], big_i=(0, 1))          # one range at 600, two at 1100, both with d_o4


def frames(c, seed):
    rs = np.random.RandomState(seed)
    return c.hold(torch.from_numpy(rs.randint(0, 256, size=(c.n, 64, 64, 3)).astype(np.uint8)).to(c.env["dev"]))


def am0_words(c, n):
    return c.hold(torch.full((n, 32, 32, 1), 0x3210F123, dtype=torch.int32, device=c.env["dev"]))


@pytest.mark.parametrize("entry", ["cgs_enc0_wgrad_u8_with_head", "cgs_enc0_wgrad_u8_with_head_enc1"])
def test_enc0_wgrad_u8_with_head(env, entry):
    """The head GEMM and features.3's rider slab are exact; the features.0 part gets real uint8 frames and dy = 0:
    its slab must be exactly zero (features.0's input is not dyadic: its non-zero gradients are out of scope here)."""
    L, hg = env["lib"], env["hg"]
    d0 = lambda n: hg.conv_desc(n, 64, 3, 0, 8, True, 2, "relu", 1, L.Dropout())

    def fn(c, i):
        dev, n = c.env["dev"], c.n
        k, with_o4 = head_ranges(c, i)
        ns0 = L.load().cgs_conv3x3_bwd_weight_slabs(C.byref(d0(n)))
        assert ns0 > 0
        s0 = Buf((ns0, 224), dev)
        sh, spw = Buf((L.load().cgs_tail_head_wgrad_slabs(n), HEAD_SLAB), dev), Buf((L.load().cgs_tail_head_wgrad_slabs(n), PW_SLAB), dev)
        args = [n, P(frames(c, 5)), P(c.hold(torch.zeros(n, 32, 32, 8, device=dev))), P(am0_words(c, n)), s0.ptr] + head_args(c, k, with_o4) + [sh.ptr, spw.ptr if with_o4 else None]
        s1 = None
        if entry != "cgs_enc0_wgrad_u8_with_head":
            ns1 = L.load().cgs_enc1_wgrad_rider_slabs(n)
            s1 = Buf((ns1, 584), dev)
            args += [n, P(c.f("e0")), P(c.f("de1")), P(c.f("am1")), s1.ptr, ns1]
        L.call(entry, *args, stream())
        sync()
        form = f"{entry}[ranges {k}+{n - k} d_o4={with_o4}]"
        z = s0.read(f"{form} {c}: features.0 slab")
        assert not z.any(), f"{form} {c}: features.0's slab is not exactly zero for dy = 0 ({np.count_nonzero(z)} elements, {(z == SENT).sum()} of them unwritten)"
        expect_head(c, form, sh, spw, with_o4)
        if s1 is not None:
            expect_slab(c, form, "g_enc1 (rider)", s1, c.g["g_enc1"], lambda mut: c.mutated(mut)[1]["g_enc1"])
    run_form(env, fn, lambda n: [L.load().cgs_tail_head_wgrad_slabs(n), L.load().cgs_enc1_wgrad_rider_slabs(n),
                                 L.load().cgs_conv3x3_bwd_weight_slabs(C.byref(d0(n)))], big_i=(0, 1))          # one range at 600, two at 1100, with d_o4


def test_enc0_bwd_mix_enc1(env):
    """slab1 (features.3's weight gradient, riding) is exact.  With dy = 0 and both regulariser scales 0 the features.0 slab and dzpre must be
    exactly zero: dzpre = [sum_c (B - A)(d_rep - d_inj) + l1 sign(z) + 2 l2 z] z (1 - z) is a pure function of those inputs (conv_bwd_both.hip)."""
    L = env["lib"]

    def fn(c, i):
        dev, n = c.env["dev"], c.n
        inject = 1 if n % 2 == 0 else 0
        n_a = n // 2 if inject else n
        a8, b8 = frames(c, 6)[:n_a], frames(c, 7)[:n_a]
        z = c.hold(torch.from_numpy(np.random.RandomState(8).uniform(0.05, 0.95, size=(n_a, 64, 64))).float().to(dev))
        ns0, ns1 = L.load().cgs_enc0_bwd_mix_slabs(n), L.load().cgs_enc1_wgrad_rider_slabs(n)
        s0, s1, dz = Buf((ns0, 224), dev), Buf((ns1, 584), dev), Buf((n_a, 64, 64), dev)
        L.call("cgs_enc0_bwd_mix_enc1", n_a, inject, None, P(c.hold(torch.zeros(n, 32, 32, 8, device=dev))), P(am0_words(c, n)), wc(env, "features.0.weight"),
               P(a8), P(b8), P(z), 0.0, 0.0, None, dz.ptr, s0.ptr, P(c.f("e0")), P(c.f("de1")), P(c.f("am1")), s1.ptr, stream())
        sync()
        form = f"cgs_enc0_bwd_mix_enc1[n_a={n_a} inject={inject}]"
        for name, b in (("features.0 slab", s0), ("dzpre", dz)):
            v = b.read(f"{form} {c}: {name}")
            assert not v.any(), f"{form} {c}: {name} is not exactly zero for dy = 0 ({np.count_nonzero(v)} elements, {(v == SENT).sum()} of them unwritten)"
        expect_slab(c, form, "g_enc1 (rider)", s1, c.g["g_enc1"], lambda mut: c.mutated(mut)[1]["g_enc1"])
    run_form(env, fn, lambda n: [L.load().cgs_enc0_bwd_mix_slabs(n), L.load().cgs_enc1_wgrad_rider_slabs(n)])


# ---------------------------------------------------------------------------------------------------------------------------------
# decoder tail
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["cgs_tail_dec_bwd", "cgs_dec0_tail_dec_bwd"])
def test_tail_dec_bwd(env, entry):
    """cgs_dec0_tail_dec_bwd: one workgroup and one slab row per image up to the documented limit (cgs_tail_dec_bwd_slabs' cap, 512);
    beyond it CGS_ERR_UNSUPPORTED and nothing written.  So besides n = 600 and 1100 there is a batch AT the limit, n = 512: the largest at
    which this form computes anything, and the one the benchmark runs."""
    L, hg = env["lib"], env["hg"]
    dec0 = entry != "cgs_tail_dec_bwd"

    def fn(c, i):
        dev, n = c.env["dev"], c.n
        nsl = L.load().cgs_tail_dec_bwd_slabs(n)
        td = hg.tail_dec_weights(env["fm"], env["lm"])
        outs = {k: Buf((n,) + SHAPE[k], dev) for k in ("dE1", "dE2", "dE3", "d_o4")}
        sl = {3: Buf((nsl, 6928), dev), 2: Buf((nsl, 1736), dev), 1: Buf((nsl, 1160), dev)}
        if dec0:
            outs["dE0"], outs["do1"] = Buf((n, 32, 32, 8), dev), Buf((n, 16, 16, 8), dev)
            args = [n, C.byref(td), P(c.f("dy_o0")), wm(env, "dec_model.0.weight"), outs["dE0"].ptr, P(c.f("e1")), P(c.f("e2")), P(c.f("e3")), P(c.f("o4")),
                    P(c.f("o3")), P(c.f("o2")), outs["do1"].ptr, outs["dE1"].ptr, outs["dE2"].ptr, outs["dE3"].ptr, outs["d_o4"].ptr, sl[3].ptr, sl[2].ptr, sl[1].ptr]
        else:
            args = [n, C.byref(td), P(c.f("e1")), P(c.f("e2")), P(c.f("e3")), P(c.f("o4")), P(c.f("o3")), P(c.f("o2")), P(c.f("do1")),
                    outs["dE1"].ptr, outs["dE2"].ptr, outs["dE3"].ptr, outs["d_o4"].ptr, sl[3].ptr, sl[2].ptr, sl[1].ptr]
        rc = getattr(L.load(), entry)(*args, stream())
        sync()
        form = entry
        if dec0 and n > nsl:
            assert rc == L.ERR_UNSUPPORTED, f"{form} {c}: return code {rc}"
            for k, b in list(outs.items()) + [(f"slab{j}", s) for j, s in sl.items()]:
                expect_untouched(c, form, k, b)
            return
        L.check(rc, entry)
        for k, b in outs.items():
            expect(c, form, k, b, c.g[k], lambda mut, k=k: c.mutated(mut)[1][k])
        for j, s in sl.items():
            expect_slab(c, form, f"g_dec{j}", s, c.g[f"g_dec{j}"], lambda mut, j=j: c.mutated(mut)[1][f"g_dec{j}"])
    run_form(env, fn, lambda n: [L.load().cgs_tail_dec_bwd_slabs(n)], big=(512,) + BIG)
