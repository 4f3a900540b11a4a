"""The decoder forward and the training mask head forward of an image in one workgroup (cgs_dec_mask_fwd, csrc/tail.hip: dec_mask_fwd_kernel)
against the two launches it replaces (cgs_tail_dec_fwd_dec0 + cgs_mask_train_fwd_packed).

The fused kernel runs the two kernels' own bodies -- same operands, same order of every sum -- so every comparison here is bit for bit:
there is no tolerance anywhere in this file.  Inputs are random with the golden chfak-1 weights; the frames include flat patches, an
all-black and an all-white image (exact ties, saturated bytes)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEC_IN = (("e0", (32, 32, 8)), ("e1", (16, 16, 8)), ("e2", (8, 8, 8)), ("e3", (4, 4, 16)), ("o4", (32,)))
OUTS = (("o3", (4, 4, 16)), ("o2", (8, 8, 8)), ("o1", (16, 16, 8)), ("o0", (32, 32, 8)), ("h", (64, 64, 16)), ("Z", (64, 64)), ("zpart", (2,)))


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def frames_u8(rs, n):
    """Random uint8 frames; every second image carries flat 8x8 patches (exact ties between neighbouring pixels), image 0 is all black,
    image 1 (if any) all white."""
    x = rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)
    for i in range(0, n, 2):
        for _ in range(12):
            y0, x0 = rs.randint(0, 57, 2)
            x[i, y0:y0 + 8, x0:x0 + 8] = rs.randint(0, 256, 3).astype(np.uint8)
    x[0] = 0
    if n > 1:
        x[1] = 255
    return x


@pytest.fixture(scope="module")
def env(g1):
    from cgs_amd import _lib, spec
    from cgs_amd import hourglass as hg
    dev = torch.device("cuda:0")
    pc, pm = g1
    lc, lm = spec.critic_layout(), spec.masker_layout()
    fc, fm = torch.zeros(lc.total, device=dev), torch.zeros(lm.total, device=dev)
    lc.flatten({k: v.to(dev) for k, v in pc.items()}, fc)
    lm.flatten({k: v.to(dev) for k, v in pm.items()}, fm)
    _lib.load()
    return dict(lib=_lib, hg=hg, dev=dev, lc=lc, lm=lm, fc=fc, fm=fm, g1=g1)


def inputs(env, n, seed, fp32_frames=False):
    rs = np.random.RandomState(seed)
    I = {k: torch.from_numpy(rs.standard_normal((n,) + s).astype(np.float32)).to(env["dev"]) for k, s in DEC_IN}
    x = frames_u8(rs, n)
    I["x"] = torch.from_numpy(x.astype(np.float32) / 255.0 if fp32_frames else x).to(env["dev"])
    return I


def outputs(env, n, fill):
    return {k: torch.full((n,) + s, fill, dtype=torch.float32, device=env["dev"]) for k, s in OUTS}


def wp(env, key):
    return C.c_void_p(env["fm"].data_ptr() + 4 * env["lm"].off(key))


def two_launches(env, n, I, O, pack, src):
    L, hg = env["lib"], env["hg"]
    td = hg.tail_dec_weights(env["fm"], env["lm"])
    L.call("cgs_tail_dec_fwd_dec0", n, C.byref(td), p(I["e0"]), p(I["e1"]), p(I["e2"]), p(I["e3"]), p(I["o4"]), p(O["o3"]), p(O["o2"]), p(O["o1"]),
           wp(env, "dec_model.0.weight"), wp(env, "dec_model.0.bias"), p(O["o0"]), wp(env, "masker.0.weight"), p(pack), stream())
    L.call("cgs_mask_train_fwd_packed", n, src, p(I["x"]), p(O["o0"]), wp(env, "masker.0.weight"), wp(env, "masker.0.bias"),
           wp(env, "masker.2.weight"), wp(env, "masker.2.bias"), p(O["h"]), p(O["Z"]), p(O["zpart"]), p(pack), stream())


def fused_rc(env, n, I, O, pack, src):
    td = env["hg"].tail_dec_weights(env["fm"], env["lm"])
    return env["lib"].load().cgs_dec_mask_fwd(n, C.byref(td), p(I["e0"]), p(I["e1"]), p(I["e2"]), p(I["e3"]), p(I["o4"]), p(O["o3"]), p(O["o2"]),
                                              p(O["o1"]), wp(env, "dec_model.0.weight"), wp(env, "dec_model.0.bias"), p(O["o0"]), src, p(I["x"]),
                                              wp(env, "masker.0.bias"), wp(env, "masker.2.weight"), wp(env, "masker.2.bias"), p(O["h"]), p(O["Z"]),
                                              p(O["zpart"]), p(pack), stream())


@pytest.mark.parametrize("n", [1, 2, 3, 37])
def test_fused_kernel_equals_the_two_launches_bit_for_bit(env, n):
    """n = 1: a single workgroup; 2 / 3: a full and a ragged pair; 37: several CUs.  o3, o2, o1, o0, h, Z and zpart are torch.equal (the
    outputs of the two forms start from different fill values, so equality comes from what the kernels wrote)."""
    L = env["lib"]
    I = inputs(env, n, 100 + n)
    pack = torch.zeros(40 * 64, device=env["dev"])
    ref, got = outputs(env, n, 1.0), outputs(env, n, 2.0)
    two_launches(env, n, I, ref, pack, L.SRC_U8)
    rc = fused_rc(env, n, I, got, pack, L.SRC_U8)
    torch.cuda.synchronize()
    assert rc == L.OK
    for k, _ in OUTS:
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], ref[k]), f"{k} (n={n}): {int((got[k] != ref[k]).sum())} of {got[k].numel()} elements differ"


@pytest.mark.parametrize("n", [1, 5])
def test_m0pack_from_the_critic_launch_equals_the_decoder_launch_s(env, n):
    """The spare workgroup of cgs_critic_fwd_fused_pack (through hourglass.critic_forward) builds the same 40 x 64 floats as the spare workgroup
    of cgs_tail_dec_fwd_dec0, byte for byte -- and the critic's own outputs do not change with the rider."""
    hg, L = env["hg"], env["lib"]
    I = inputs(env, n, 200 + n)
    pack_dec = torch.full((40 * 64,), 3.0, device=env["dev"])
    two_launches(env, n, I, outputs(env, n, 0.0), pack_dec, L.SRC_U8)
    pack_crit = torch.full((40 * 64,), 4.0, device=env["dev"])
    with_rider = hg.critic_forward(env["fc"], env["lc"], I["x"], n, m0=(wp(env, "masker.0.weight"), pack_crit))
    without = hg.critic_forward(env["fc"], env["lc"], I["x"], n)
    torch.cuda.synchronize()
    assert torch.equal(pack_crit.view(torch.int32), pack_dec.view(torch.int32))
    for k in without:
        assert torch.equal(with_rider[k], without[k]), k


@pytest.mark.parametrize("n", [160, 224])
def test_step_is_bit_identical_with_the_fused_launch_on_and_off(env, monkeypatch, n):
    """Two phase-2 steps at dropout 0.3 through the engine's own selection: losses, parameters and Adam moments with DEC_MASK_FWD_FUSED on
    and off; the captured graph of the fused form (step 2 of a use_graph engine is a replay) against the eager steps.  n = 160 is the
    smallest batch that takes the one-kernel mask head forward, hence the fused launch."""
    from cgs_amd import engine
    hg = env["hg"]
    pc, pm = env["g1"]
    dev = env["dev"]
    rs = np.random.RandomState(31 + n)
    A = torch.from_numpy(frames_u8(rs, n)).to(dev)
    B = torch.from_numpy(rs.randint(0, 256, (n, 64, 64, 3)).astype(np.uint8)).to(dev)
    Y = torch.from_numpy(rs.rand(n).astype(np.float32)).to(dev)
    taken = []
    inner = hg.masker_forward

    def spy(*a, **kw):
        taken.append(bool(kw.get("m0pack_done")))
        return inner(*a, **kw)

    monkeypatch.setattr(hg, "masker_forward", spy)

    def run(use_graph):
        e = engine.HourglassEngine(n, device=dev, dropout=0.3, use_graph=use_graph)
        e.load_state(pc, pm)
        for _ in range(2):
            e.phase2_step(A, B, Y)
        torch.cuda.synchronize()
        return [t.clone() for t in (e.losses, e.flat, e.m, e.v)]

    monkeypatch.setattr(hg, "DEC_MASK_FWD_FUSED", True)
    on = run(False)
    assert taken and all(taken), "the fused launch was not selected"
    graph = run(True)
    del taken[:]
    monkeypatch.setattr(hg, "DEC_MASK_FWD_FUSED", False)
    off = run(False)
    assert taken and not any(taken), "the switch did not switch the fused launch off"
    for a, b, c, what in zip(on, off, graph, ("losses", "parameters", "m", "v")):
        assert torch.isfinite(a).all(), what
        assert torch.equal(a, b), f"{what} differ between DEC_MASK_FWD_FUSED on and off (n={n})"
        assert torch.equal(c, a), f"{what}: the replayed graph of the fused form differs from the eager steps (n={n})"


def test_fp32_frames_keep_the_two_launches(env, monkeypatch):
    """The entry point answers CGS_ERR_UNSUPPORTED for fp32 frames (and writes nothing); hourglass.masker_forward with fp32 frames -- asked the
    same way as for uint8 frames -- runs the two launches and equals them bit for bit."""
    hg, L = env["hg"], env["lib"]
    n = 3
    monkeypatch.setattr(hg, "MASK_TRAIN_FUSED_MIN_N", 0)
    monkeypatch.setattr(hg, "DEC_MASK_FWD_FUSED", True)
    I = inputs(env, n, 300, fp32_frames=True)
    pack = torch.zeros(40 * 64, device=env["dev"])
    ref = outputs(env, n, 1.0)
    two_launches(env, n, I, ref, pack, L.SRC_F32)
    got = outputs(env, n, 2.0)
    rc = fused_rc(env, n, I, got, pack, L.SRC_F32)
    torch.cuda.synchronize()
    assert rc == L.ERR_UNSUPPORTED
    for k, _ in OUTS:
        assert bool((got[k] == 2.0).all()), f"{k} was written by a call that answered CGS_ERR_UNSUPPORTED"
    assert not hg.dec_mask_fwd_fused(n, False) and hg.dec_mask_fwd_fused(n, True)
    o = {"o4": I["o4"], "m0pack": pack.clone()}
    zpart = torch.full((hg.zpart_count(n), 2), 2.0, device=env["dev"])
    hg.masker_forward(env["fm"], env["lm"], I["x"], [I["e0"], I["e1"], I["e2"], I["e3"], None], n, out=o, o4_done=True, zpart=zpart, m0pack_done=True)
    torch.cuda.synchronize()
    for k, _ in OUTS:
        g = zpart if k == "zpart" else o["hm" if k == "h" else k]
        assert torch.equal(g, ref[k]), f"{k}: masker_forward with fp32 frames differs from the two launches"
