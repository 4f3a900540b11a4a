"""The float64 backward reference of the exact-arithmetic backward tests (tests/exact_bwd_ref.py), checked on the CPU: it equals torch's
float64 autograd of the same chain bit for bit, its exactness conditions hold for every (draw, n) test_gpu_exact_backward.py uses, a cast
to fp32 loses nothing, and every planted mutation moves at least one tensor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
import exact_bwd_ref as B


@pytest.fixture(scope="module")
def runs():
    """(draw, n, dropout) -> (params, forward, gradients, masks), computed once and left unchanged."""
    out = {}
    for d in range(X.N_DRAWS):
        for n in (3, 1):
            out[(d, n, False)] = B.run(d, n) + (None,)
    for d in B.DROP_DRAWS:
        mk = B.standin_masks(d, 3)
        out[(d, 3, True)] = B.run(d, 3, masks=mk) + (mk,)
    return out


def autograd(P, r, masks):
    """The same chain in torch float64 (conv2d, max_pool2d, interpolate, linear) and its autograd; the cotangent of pred enters as
    d logit = dpred pred (1 - pred) with the saved pred = 1/2.  Returns the tensors of exact_bwd_ref.backward (NHWC, slab layout)."""
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double()
    nchw = lambda v: t(v).permute(0, 3, 1, 2).contiguous()
    pc, pm = ({k: t(v).requires_grad_(True) for k, v in p.items() if k.rsplit(".", 1)[0] in X.LAYERS} for p in P)
    n = r["e0"].shape[0]
    mk = [nchw(masks[0]), nchw(masks[1]), t(masks[2])] if masks is not None else [1.0, 1.0, 1.0]
    keep = {}

    def tap(name, v):
        v = v * 1.0                 # an identity node: its .grad is the gradient that arrives on THIS edge only
        v.retain_grad()
        keep[name] = v
        return v

    e = [tap("de0", nchw(r["e0"]).requires_grad_(True))]
    pre = []
    for i, key in ((1, "features.3"), (2, "features.6"), (3, "features.10")):
        src = e[-1] * (mk[0] if i == 3 else 1.0)
        z = F.conv2d(src, pc[key + ".weight"], pc[key + ".bias"], padding=1)
        pre.append(z)
        e.append(tap(f"de{i}", F.max_pool2d(F.relu(z), 2)))
    z4 = tap("dz4", F.conv2d(e[3] * mk[1], pc["features.14.weight"], pc["features.14.bias"]).flatten(1))
    e4 = tap("de4", F.relu(z4))
    z1 = tap("dh1", F.linear(e4, pc["crit.1.weight"], pc["crit.1.bias"]))
    logit = F.linear(F.relu(z1) * mk[2], pc["crit.4.weight"], pc["crit.4.bias"])[:, 0]
    up2 = lambda v: F.interpolate(v, scale_factor=2, mode="nearest")
    o4 = tap("d_o4", F.conv2d(tap("de4_dec", e4).reshape(n, 32, 1, 1), pm["dec_model.4.weight"], pm["dec_model.4.bias"]))
    o3 = tap("do3", F.conv2d(torch.cat((tap("dE3", e[3]), up2(up2(o4))), 1), pm["dec_model.3.weight"], pm["dec_model.3.bias"], padding=1))
    o2 = tap("do2", F.conv2d(torch.cat((tap("dE2", e[2]), up2(o3)), 1), pm["dec_model.2.weight"], pm["dec_model.2.bias"], padding=1))
    o1 = tap("do1", F.conv2d(torch.cat((tap("dE1", e[1]), up2(o2)), 1), pm["dec_model.1.weight"], pm["dec_model.1.bias"], padding=1))
    o0 = F.conv2d(torch.cat((tap("dE0", e[0]), up2(o1)), 1), pm["dec_model.0.weight"], pm["dec_model.0.bias"], padding=1)
    for k in ("e1", "e2", "e3"):
        assert np.array_equal(e[int(k[1])].detach().permute(0, 2, 3, 1).numpy(), r[k]), k
    assert np.array_equal(o0.detach().permute(0, 2, 3, 1).numpy(), r["o0"]) and np.array_equal(logit.detach().numpy(), r["logit"])
    dz2 = t(r["dpred"]) * 0.25
    ((o0 * nchw(r["dy_o0"])).sum() + (logit * dz2).sum()).backward()
    g = {}
    for k, v in keep.items():
        a = v.grad
        g[k] = (a.permute(0, 2, 3, 1) if a.dim() == 4 else a).numpy()
    g["d_o4"] = g["d_o4"].reshape(n, 32)
    slab = lambda p, k: np.concatenate((p[k + ".weight"].grad.permute(2, 3, 1, 0).reshape(-1).numpy(), p[k + ".bias"].grad.numpy()))
    for key, name in B.SLABS.items():
        if key == "head":
            g[name] = np.concatenate((slab(pc, "features.14"), pc["crit.1.weight"].grad.T.reshape(-1).numpy(), pc["crit.1.bias"].grad.numpy(),
                                      pc["crit.4.weight"].grad[0].numpy(), pc["crit.4.bias"].grad.numpy()))
        else:
            g[name] = slab(pc if key.startswith("features") else pm, key)
    h1m = r["h1"] * (masks[2] if masks is not None else 1.0)
    hv = np.zeros((n, 384))
    hv[:, :256] = (r["e3"] * (masks[1] if masks is not None else 1.0)).reshape(n, 256)
    hv[:, 256:288], hv[:, 288:320], hv[:, 320:352], hv[:, 352] = g.pop("dz4"), g.pop("dh1"), dz2.numpy()[:, None] * h1m, dz2.numpy()
    g["hvec"] = hv
    return g


def test_reference_equals_torch_float64_autograd(runs):
    for (d, n, drop), (P, r, g, mk) in runs.items():
        t = autograd(P, r, mk)
        for k in B.TENSORS:
            assert t[k].shape == g[k].shape, (d, n, k, t[k].shape, g[k].shape)
            assert np.array_equal(t[k], g[k]), f"draw {d} n={n} dropout={drop}: {k} differs from autograd at {np.argwhere(t[k] != g[k])[:3].tolist()}"


def test_conditions_hold_for_every_case_the_gpu_tests_use(runs):
    """n = 3: all draws (and the Dropout group); n = 1: draw 0.  The large batches of the GPU tests carry cotangents on at most eight
    images, whose gradients are those of an n <= 8 batch; the test there asserts the conditions on the carrying images again.
    The target modes of the tail kernels replace |dpred| by the draw's loss scale (target_dpred): the conditions hold for those cotangents too."""
    for (d, n, drop), (P, r, g, mk) in runs.items():
        if n == 1 and d != 0:
            continue
        try:
            B.check_exactness_bwd(P, r, g, mk, min_ties=20)
            rt = dict(r, dpred=B.target_dpred(d, r["dpred"]))
            B.check_exactness_bwd(P, rt, B.backward(P, rt, rt["dy_o0"], rt["dpred"], mk), mk, min_ties=20)
        except AssertionError as e:
            raise AssertionError(f"draw {d} n={n} dropout={drop}: {e}")


def test_fp32_cast_loses_nothing(runs):
    for key, (P, r, g, mk) in runs.items():
        for k in B.TENSORS + ("dy_o0", "dpred"):
            v = g[k] if k in g else r[k]
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v), (key, k)


MUT_DRAWS = tuple(range(0, X.N_DRAWS, 9))


@pytest.mark.parametrize("mut", B.MUTATIONS)
def test_planted_mutation_moves_a_tensor(runs, mut):
    for d in MUT_DRAWS:
        g = runs[(d, 3, False)][2]
        m = B.run(d, 3, mut=mut)[2]
        moved = [k for k in B.TENSORS if not np.array_equal(m[k], g[k])]
        assert moved, f"{mut}: no tensor moves in draw {d}"
