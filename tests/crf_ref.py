"""float64 numpy restatement of the two-label dense CRF that cgs_dense_crf2 computes (include/cgs_hip.h, csrc/crf.hip), the checker of
tests/test_crf_host.py and tests/test_gpu_crf.py.  Exact fully-connected mean field, Potts compatibility, symmetric normalisation:

  kB(i,j) = exp(-|p_i-p_j|^2 / 2 alpha^2 - |c_i-c_j|^2 / 2 beta^2),  kG(i,j) = exp(-|p_i-p_j|^2 / 2 gamma^2)   (j = i included)
  n_i = (sum_j k(i,j) + 1e-20)^-1/2,  U_l = -ln P_l in fp32 (P_0 = 1 - P_1 in fp32),  Q1 = sigmoid(d) with
  d = a_1 - a_0 = (U_0 - U_1) + sum_k w_k n_i (2 sum_j k(i,j) n_j Q1(j) - S_i),   S_i = sum_j k(i,j) n_j.

The bilateral kernel is applied blockwise (rows of K at a time), so 128 x 128 frames fit in memory; the spatial one is separable."""
import numpy as np

_BLOCK_ELEMS = 1 << 22          # pair entries per block of K_B rows


def unary_diff(p1):
    """U_0 - U_1 in float64 from the fp32 unaries (+-inf where P_1 is exactly 1 / 0)."""
    p1 = np.asarray(p1, dtype=np.float32)
    p0 = np.float32(1.0) - p1
    with np.errstate(divide="ignore"):
        u0, u1 = -np.log(p0), -np.log(p1)
    return u0.astype(np.float64) - u1.astype(np.float64)


def sigmoid(d):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-d))


class Frame:
    """One frame [h,w,3] uint8 with its P_1 [h,w] and parameters (w1, alpha, beta, w2, gamma, it)."""

    def __init__(self, frame_u8, p1, params):
        self.h, self.w = p1.shape
        self.w1, alpha, beta, self.w2, gamma, self.it = params
        self.p1 = np.asarray(p1, dtype=np.float32)
        ys, xs = np.mgrid[0:self.h, 0:self.w]
        self.pos = np.stack([xs.ravel(), ys.ravel()], -1).astype(np.float64)
        self.col = np.asarray(frame_u8, dtype=np.float64).reshape(-1, 3)
        self.a2, self.b2 = 2.0 * alpha * alpha, 2.0 * beta * beta
        ax = lambda n: np.exp(-np.subtract.outer(np.arange(n), np.arange(n)).astype(np.float64) ** 2 / (2.0 * gamma * gamma))
        self.gx, self.gy = ax(self.w), ax(self.h)
        self.dU = unary_diff(self.p1).ravel()
        self.nB = 1.0 / np.sqrt(self.kb(np.ones((self.h * self.w, 1)))[:, 0] + 1e-20)
        self.nG = 1.0 / np.sqrt(self.kg(np.ones(self.h * self.w)) + 1e-20)
        self.sB = self.kb(self.nB[:, None])[:, 0]
        self.sG = self.kg(self.nG)

    def kb(self, V):
        """K_B @ V for V [N, m], rows of K_B a block at a time."""
        out = np.empty_like(V, dtype=np.float64)
        block = max(16, _BLOCK_ELEMS // len(V))
        for lo in range(0, len(V), block):
            hi = min(len(V), lo + block)
            dp = ((self.pos[lo:hi, None, :] - self.pos[None, :, :]) ** 2).sum(-1)
            dc = ((self.col[lo:hi, None, :] - self.col[None, :, :]) ** 2).sum(-1)
            out[lo:hi] = np.exp(-dp / self.a2 - dc / self.b2) @ V
        return out

    def kg(self, v):
        return (self.gy @ v.reshape(self.h, self.w) @ self.gx.T).ravel()

    def start(self):
        """Q1 after zero iterations: softmax(-U)."""
        return sigmoid(self.dU).reshape(self.h, self.w)

    def step_d(self, q1):
        """a_1 - a_0 of one mean-field step from the state Q1 [h,w]."""
        q = np.asarray(q1, dtype=np.float64).ravel()
        tB = self.kb((self.nB * q)[:, None])[:, 0]
        tG = self.kg(self.nG * q)
        d = self.dU + self.w1 * self.nB * (2.0 * tB - self.sB) + self.w2 * self.nG * (2.0 * tG - self.sG)
        return d.reshape(self.h, self.w)

    def step(self, q1):
        return sigmoid(self.step_d(q1))

    def run(self, iterations=None):
        """(labels uint8 [h,w], Q1 [h,w], final a_1 - a_0 [h,w] or None at zero iterations)."""
        it = self.it if iterations is None else iterations
        q, d = self.start(), None
        for _ in range(it):
            d = self.step_d(q)
            q = sigmoid(d)
        if d is None:
            return (self.p1 > np.float32(1.0) - self.p1).astype(np.uint8), q, None
        return (d > 0).astype(np.uint8), q, d
