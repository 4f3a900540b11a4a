"""The dyadic fixture of the exact-arithmetic forward tests (tests/exact_ref.py), checked on the CPU: its conditions hold for every
draw and batch size test_gpu_exact_forward.py uses, its draws cover every weight element, a float32 evaluation through torch's own
convolution / max-pool / upsample equals it bit for bit, and it reacts to single wrong weights and to four planted index errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X

N = 3
WATCH = ("pred", "o1", "o0")


@pytest.fixture(scope="module")
def runs():
    """draw -> (params, e0, reference) at n = 3, computed once and left unchanged."""
    out = {}
    for d in range(X.N_DRAWS):
        P, e0 = X.dyadic_params(d), X.dyadic_e0(d, N)
        out[d] = (P, e0, X.forward(P, e0))
    return out


def test_conditions_hold_for_every_draw(runs):
    for d, (P, e0, r) in runs.items():
        try:
            X.check_exactness(r, P, e0)
        except AssertionError as e:
            raise AssertionError(f"draw {d}: {e}")


@pytest.mark.parametrize("n", [1, 1100])
def test_conditions_hold_for_draw_0_at_the_other_batch_sizes(n):
    """(The n = 1024 case of cgs_tail_dec_fwd_dec0 is the first 1024 images of the n = 1100 batch.)"""
    P, e0 = X.dyadic_params(0), X.dyadic_e0(0, n)
    X.check_exactness(X.forward(P, e0), P, e0)


def test_a_denser_variant_fails_the_conditions(monkeypatch):
    """The conditions are real constraints: with e0 = k/4, k in 0..8, the sums leave the exact range."""
    monkeypatch.setattr(X, "KMAX", 8)
    bad = 0
    for d in range(12):
        P, e0 = X.dyadic_params(d), X.dyadic_e0(d, N)
        try:
            X.check_exactness(X.forward(P, e0), P, e0)
        except AssertionError:
            bad += 1
    assert bad >= 6, bad


def test_draws_cover_every_weight_element(runs):
    for which in (0, 1):
        for key, w in runs[0][0][which].items():
            if not key.endswith(".weight") or key.rsplit(".", 1)[0] not in X.LAYERS:
                continue
            union = np.zeros(w.shape, dtype=bool)
            for d in range(X.N_DRAWS):
                nz = runs[d][0][which][key] != 0
                assert (nz.reshape(w.shape[0], -1).sum(1) == 4).all(), f"{key} draw {d}: four non-zeros per output channel"
                union |= nz
            assert union.all(), f"{key}: {union.size - union.sum()} elements are zero in every draw"


def torch_f32_chain(P, e0):
    """The same chain through torch's float32 CPU operators (conv2d, max_pool2d with indices, interpolate, linear), NCHW."""
    pc, pm = ({k: torch.from_numpy(v).float() for k, v in p.items()} for p in P)
    h = torch.from_numpy(e0).float().permute(0, 3, 1, 2)
    r, emb = {}, [h]
    for i, key in ((1, "features.3"), (2, "features.6"), (3, "features.10")):
        pre = F.relu(F.conv2d(h, pc[key + ".weight"], pc[key + ".bias"], padding=1))
        h, idx = F.max_pool2d(pre, 2, return_indices=True)
        hw = pre.shape[-1]
        yy, xx = torch.meshgrid(torch.arange(hw // 2), torch.arange(hw // 2), indexing="ij")
        pos = (idx // hw - 2 * yy) * 2 + (idx % hw - 2 * xx)
        nib = torch.where(h > 0, pos, torch.full_like(pos, 15)).permute(0, 2, 3, 1).numpy().astype(np.uint32)
        am = np.zeros(nib.shape[:3] + (nib.shape[3] // 8,), dtype=np.uint32)
        for ch in range(nib.shape[3]):
            am[..., ch // 8] |= nib[..., ch] << np.uint32(4 * (ch % 8))
        r[f"e{i}"], r[f"am{i}"] = h, am
        emb.append(h)
    e4 = F.relu(F.conv2d(h, pc["features.14.weight"], pc["features.14.bias"]))
    r["e4"] = e4.flatten(1)
    r["h1"] = F.relu(F.linear(r["e4"], pc["crit.1.weight"], pc["crit.1.bias"]))
    r["logit"] = F.linear(r["h1"], pc["crit.4.weight"], pc["crit.4.bias"])[:, 0]
    up2 = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
    o4 = F.conv2d(e4, pm["dec_model.4.weight"], pm["dec_model.4.bias"])
    r["o4"] = o4.flatten(1)
    r["o3"] = F.conv2d(torch.cat((emb[3], up2(up2(o4))), 1), pm["dec_model.3.weight"], pm["dec_model.3.bias"], padding=1)
    r["o2"] = F.conv2d(torch.cat((emb[2], up2(r["o3"])), 1), pm["dec_model.2.weight"], pm["dec_model.2.bias"], padding=1)
    r["o1"] = F.conv2d(torch.cat((emb[1], up2(r["o2"])), 1), pm["dec_model.1.weight"], pm["dec_model.1.bias"], padding=1)
    r["o0"] = F.conv2d(torch.cat((emb[0], up2(r["o1"])), 1), pm["dec_model.0.weight"], pm["dec_model.0.bias"], padding=1)
    out = {}
    for k, v in r.items():
        if isinstance(v, torch.Tensor):
            assert v.dtype == torch.float32
            v = (v.permute(0, 2, 3, 1) if v.dim() == 4 else v).numpy()
        out[k] = v
    return out


def test_float32_torch_evaluation_is_bit_identical(runs):
    """Order independence shown, not asserted: torch's float32 kernels sum in their own order and give the float64 numbers."""
    for d in range(0, X.N_DRAWS, 11):                      # 10 draws
        P, e0, r = runs[d]
        t = torch_f32_chain(P, e0)
        for k, v in t.items():
            assert v.shape == r[k].shape, (d, k, v.shape, r[k].shape)
            assert np.array_equal(v.astype(r[k].dtype), r[k]), f"draw {d}: {k} differs between torch float32 and the float64 chain"


def changed(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in WATCH)


PER_LAYER = 30


def weight_candidates():
    """30 non-zero elements of each of the eleven layers, 330 in all, by a rule that looks at no output: element (3 j) mod count of
    draw (7 j) mod 108, j = 0..29.  crit.1 is sampled in the rows whose output crit.4 reads in that draw (crit.4 has four non-zeros:
    the other 28 rows of crit.1 reach h1, which the encoder forms store, but none of pred / o1 / o0)."""
    for which, shapes in ((0, X.critic_shapes()), (1, X.masker_shapes())):
        for key, _ in shapes:
            layer = key.rsplit(".", 1)[0]
            if key.endswith(".weight") and layer in X.LAYERS:
                for j in range(PER_LAYER):
                    yield which, key, (7 * j) % X.N_DRAWS, j


def test_single_weight_elements_are_seen_in_the_final_outputs(runs):
    """Zeroing ONE non-zero weight element moves at least one element of (pred, o1, o0) of its draw: for at least 200 of the 330
    candidates, and for at least half of the candidates of every layer.  It cannot hold for every candidate: behind a ReLU a unit
    that is off in all three images hides its weights (e4 and h1 are about 3/4 non-zero), and so does a feature channel whose four
    weights leave it off everywhere; those elements show in the intermediate tensors that the fp32 and h16 forms store and that
    the GPU tests compare too.  The candidates are fixed by a rule, the ones that are seen are counted."""
    seen, total = {}, {}
    for which, key, d, j in weight_candidates():
        P, e0, r = runs[d]
        w = P[which][key]
        nz = w != 0
        if key == "crit.1.weight":
            nz = nz & (P[0]["crit.4.weight"][0] != 0)[:, None]
        idx = np.argwhere(nz)
        at = tuple(idx[(3 * j) % len(idx)])
        Q = (dict(P[0]), dict(P[1]))
        Q[which][key] = w.copy()
        Q[which][key][at] = 0.0
        total[key] = total.get(key, 0) + 1
        seen[key] = seen.get(key, 0) + int(changed(X.forward(Q, e0), r))
    print({k: f"{seen[k]}/{total[k]}" for k in total})
    assert len(total) == 11 and all(v == PER_LAYER for v in total.values())
    assert sum(seen.values()) >= 200, seen
    assert all(2 * seen[k] >= total[k] for k in total), seen


def test_last_index_tie_rule_is_seen_in_the_argmax_words(runs):
    """A tie that takes the last index instead of the first picks an EQUAL value: no tensor value can move (asserted), only the
    argmax nibbles do, and they do in every pooled stage of every draw tried -- which is why the GPU tests compare am1 / am2 / am3."""
    for d in range(0, X.N_DRAWS, 9):
        P, e0, r = runs[d]
        m = X.forward(P, e0, mut="tie_last")
        assert not changed(m, r) and all(np.array_equal(m[k], r[k]) for k in X.TENSORS)
        for k in ("am1", "am2", "am3"):
            assert not np.array_equal(m[k], r[k]), f"draw {d}: {k} does not react to the tie rule"


@pytest.mark.parametrize("mut", [m for m in X.MUTATIONS if m != "tie_last"])
def test_planted_reference_mutation_is_seen(runs, mut):
    hit = [d for d in range(0, X.N_DRAWS, 9) if changed(X.forward(runs[d][0], runs[d][1], mut=mut), runs[d][2])]
    assert hit, f"{mut}: none of {WATCH} moves in any of the draws tried"
