"""CPU checks of the dense-CRF restatement (tests/crf_ref.py) and of the -crf plumbing that needs no GPU."""
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import crf_ref  # noqa: E402
import cgs_amd  # noqa: E402
from cgs_amd import _lib  # noqa: E402


def _naive_q1(frame, p1, params, iterations):
    """Per-pair double loop of the two-label mean field in its softmax form (both labels carried, no shortcut)."""
    w1, alpha, beta, w2, gamma, _ = params
    h, w = p1.shape
    pix = [(x, y) for y in range(h) for x in range(w)]
    N = len(pix)
    col = frame.reshape(-1, 3).astype(np.float64)
    kB = np.zeros((N, N))
    kG = np.zeros((N, N))
    for i, (xi, yi) in enumerate(pix):
        for j, (xj, yj) in enumerate(pix):
            dp = (xi - xj) ** 2 + (yi - yj) ** 2
            dc = sum((col[i, c] - col[j, c]) ** 2 for c in range(3))
            kB[i, j] = math.exp(-dp / (2 * alpha * alpha) - dc / (2 * beta * beta))
            kG[i, j] = math.exp(-dp / (2 * gamma * gamma))
    nB = [1.0 / math.sqrt(sum(kB[i]) + 1e-20) for i in range(N)]
    nG = [1.0 / math.sqrt(sum(kG[i]) + 1e-20) for i in range(N)]
    P1 = p1.astype(np.float32).ravel()
    P0 = np.float32(1.0) - P1
    U = [[float(-np.log(P0[i])), float(-np.log(P1[i]))] for i in range(N)]

    def softmax(a):
        m = max(a)
        e = [math.exp(v - m) for v in a]
        return [v / sum(e) for v in e]
    Q = [softmax([-U[i][0], -U[i][1]]) for i in range(N)]
    for _ in range(iterations):
        new = []
        for i in range(N):
            a = []
            for lab in range(2):
                mB = sum(kB[i, j] * nB[j] * Q[j][lab] for j in range(N))
                mG = sum(kG[i, j] * nG[j] * Q[j][lab] for j in range(N))
                a.append(-U[i][lab] + w1 * nB[i] * mB + w2 * nG[i] * mG)
            new.append(softmax(a))
        Q = new
    return np.array([q[1] for q in Q]).reshape(h, w)


def _frame(h, w, seed):
    rs = np.random.RandomState(seed)
    frame = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    frame[: h // 2, : w // 2] = (40, 200, 90)             # a flat block: pairs with kB near the spatial kernel alone
    p1 = rs.uniform(0.05, 0.95, (h, w)).astype(np.float32)
    return frame, p1


def test_restatement_equals_naive_double_loop():
    frame, p1 = _frame(6, 5, 0)
    for params in [(22, 12, 3.1, 8, 1.8, 0), (5, 3, 40, 3, 1.0, 0)]:
        F = crf_ref.Frame(frame, p1, params)
        for it in range(4):
            want = _naive_q1(frame, p1, params, it)
            _, got, _ = F.run(it)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_zero_iterations_and_zero_weights_give_the_argmax_of_p():
    frame, p1 = _frame(7, 9, 1)
    p1[0, 0] = 0.5                                          # a tie goes to label 0
    want = (p1 > np.float32(1.0) - p1).astype(np.uint8)
    lab0, _, _ = crf_ref.Frame(frame, p1, (22, 12, 3.1, 8, 1.8, 0)).run()
    np.testing.assert_array_equal(lab0, want)
    labw, _, _ = crf_ref.Frame(frame, p1, (0, 12, 3.1, 0, 1.8, 5)).run()
    np.testing.assert_array_equal(labw, want)


def test_probability_one_pins_label_one():
    frame, p1 = _frame(8, 8, 2)
    p1[:] = 0.001
    p1[3, 4] = 1.0
    p1[6, 1] = 0.0
    for params in [(22, 12, 3.1, 8, 1.8, 10), (1000, 50, 100, 1000, 5, 5)]:
        lab, q, _ = crf_ref.Frame(frame, p1, params).run()
        assert lab[3, 4] == 1 and q[3, 4] == 1.0
        assert lab[6, 1] == 0 and q[6, 1] == 0.0


def test_dense_crf2_is_declared_in_header_and_signatures():
    with open(os.path.join(REPO, "include", "cgs_hip.h")) as fp:
        text = fp.read()
    assert re.search(r"\bint cgs_dense_crf2\s*\(", text)
    assert re.search(r"\}\s*cgs_crf_params;", text)
    assert "cgs_dense_crf2" in _lib.SIGNATURES
    assert [f for f, _ in _lib.CrfParams._fields_] == ["w_bilateral", "alpha", "beta", "w_gaussian", "gamma", "iterations"]


def test_reference_params_match_the_reference_grid():
    # main.py:1230-1235: w1 = [22], alpha = [12], beta = [3.1], w2 = [8], gamma = [1.8], it = [10]
    assert tuple(cgs_amd.crf.REFERENCE_PARAMS) == (22, 12, 3.1, 8, 1.8, 10)
