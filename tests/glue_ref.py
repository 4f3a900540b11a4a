"""float64 numpy references of the training step's glue kernels (csrc/elementwise.hip): the mask mix and its backward with the
L1/L2 mask regularisers, the phase-1 / phase-2 losses and their dpred, flat Adam and the slab reduction.  No torch, no GPU.
Every input is the kernel's exact float32 / uint8 input promoted to float64, so a kernel differs from these functions by its own
rounding only.  Scalars a kernel receives as C floats go through f32() first for the same reason.

The builders at the end make the inputs that tests/test_gpu_glue.py feeds the loss kernels; tests/test_glue_host.py checks on
the same arrays that they tell per-image partial sums from partial sums that straddle images."""
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -24            # unit roundoff of float32

LIVE, INJECT, BCE, WEIGHTED = 1, 2, 4, 8      # flag bits of cgs_phase2_losses / cgs_reduce_adam
BCE_DENOM_MIN = float(np.float32(1e-12))      # the kernels' 1e-12f; torch.binary_cross_entropy's backward clamps at the same float


def f32(x):
    """The value a C float argument takes, as a Python float."""
    return float(np.float32(x))


def _d(x):
    return np.asarray(x, dtype=np.float64)


def _frames(A_u8, n):
    assert A_u8.dtype == np.uint8
    return _d(A_u8).reshape(n, -1, 3) / 255.0


def mask_sums(Z):
    """Per-image (sum |Z|, sum Z^2) [n, 2] of Z [n, ...]."""
    z = _d(Z).reshape(Z.shape[0], -1)
    return np.stack([np.abs(z).sum(1), (z * z).sum(1)], axis=1)


def mix_fwd(A_u8, B_u8, Z, inject):
    """replaced = A(1-Z) + ZB, injected = B(1-Z) + ZA.  Returns mixed [n or 2n, hw, 3] in slot order [replaced | injected] and the
    per-image sums [n, 2] = (sum |Z|, sum Z^2)."""
    n = Z.shape[0]
    z = _d(Z).reshape(n, -1, 1)
    a, b = _frames(A_u8, n), _frames(B_u8, n)
    rep = a * (1 - z) + z * b
    mixed = np.concatenate([rep, b * (1 - z) + z * a]) if inject else rep
    return mixed, mask_sums(Z)


def mix_bwd(A_u8, B_u8, Z, dmixed, inject, l1s, l2s, vf_pred=None):
    """dzpre = [ sum_c (B-A)_c (dRep_c - dInj_c) + l1s vf sign(Z) + 2 l2s vf^2 Z ] Z (1-Z), sign(0) = 0, vf = 1 - vf_pred[image]
    (1 without vf_pred).  Returns (dzpre [n, hw], bound [n, hw]): the bound is the same expression with every term replaced by
    its absolute value (A and B separately: the kernel forms B - A from two rounded values)."""
    n = Z.shape[0]
    z = _d(Z).reshape(n, -1)
    a, b = _frames(A_u8, n), _frames(B_u8, n)
    dm = _d(dmixed).reshape(-1, z.shape[1], 3)
    dr = dm[:n]
    di = dm[n:2 * n] if inject else np.zeros_like(dr)
    vf = np.ones((n, 1)) if vf_pred is None else (1 - _d(vf_pred)).reshape(n, 1)
    d = ((b - a) * (dr - di)).sum(2) + l1s * vf * np.sign(z) + 2 * l2s * vf * vf * z
    mag = ((a + b) * (np.abs(dr) + np.abs(di))).sum(2) + np.abs(l1s * vf * np.sign(z)) + np.abs(2 * l2s * vf * vf * z)
    return d * z * (1 - z), mag * np.abs(z) * (1 + np.abs(z))


def _bce(p, y):
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log(1 - p), -100.0)
    return -(y * lp + (1 - y) * lq), (p - y) / np.maximum((1 - p) * p, BCE_DENOM_MIN)


def phase1(pred, y, bce):
    """mean squared error or (log clamped at -100) binary cross entropy of pred [n] against y [n].  Returns (loss, dpred [n])."""
    p, y = _d(pred), _d(y)
    n = p.shape[0]
    if bce:
        terms, g = _bce(p, y)
        return terms.sum() / n, g / n
    return ((p - y) ** 2).sum() / n, 2 * (p - y) / n


def phase2(pred, y, zsum_per_image, n, lfak, l1, l2, flags, nz):
    """The phase-2 objective on the critic values pred = [B | A | replaced | injected] (4n, or 3n without inject), targets y [n]
    and the per-image (sum |Z|, sum Z^2) [n, 2]; nz = mask elements.  Returns losses[6] = (critic, replace, inject, l1, l2, total)
    and dpred = d total / d pred (3n entries without inject).  flags: LIVE | INJECT | BCE | WEIGHTED (valuefak = 1 - pred_A,
    detached, on the regularisers)."""
    live, inject, bce, weighted = bool(flags & LIVE), bool(flags & INJECT), bool(flags & BCE), bool(flags & WEIGHTED)
    p, y, zs = _d(pred), _d(y), _d(zsum_per_image)
    pb, pa, pr = p[:n], p[n:2 * n], p[2 * n:3 * n]
    dpred = np.zeros(4 * n if inject else 3 * n)
    c = 0.0
    if live:
        c, g = phase1(pa, y, bce)
        dpred[n:2 * n] = lfak * g
    r = ((pr - pb) ** 2).sum() / n
    dpred[2 * n:3 * n] = 2 * (pr - pb) / n
    i = 0.0
    if inject:
        pi = p[3 * n:4 * n]
        i = ((pi - pa) ** 2).sum() / n
        dpred[3 * n:] = 2 * (pi - pa) / n
    vf = 1 - pa if weighted else np.ones(n)
    n1 = l1 * (vf * zs[:, 0]).sum() / nz
    n2 = l2 * (vf * vf * zs[:, 1]).sum() / nz
    total = (lfak * c if live else 0.0) + r + i + n1 + n2
    return np.array([c, r, i, n1, n2, total]), dpred


AdamStep = namedtuple("AdamStep", "p m v update m_bound update_bound")


def adam(p, g, m, v, t, lr, b1, b2, eps, gscale=1.0):
    """torch.optim.Adam's step number t (defaults: no weight decay, no amsgrad) on gradient g * gscale, bias corrections in
    float64.  update = p_before - p_after.  m_bound = |b1 m| + |(1-b1) g| (the two terms of m may cancel; those of v cannot) and
    update_bound = the update with m_bound in place of m: what a float32 rounding of m's terms is relative to."""
    p, g, m, v = _d(p), _d(g) * gscale, _d(m), _d(v)
    m1 = b1 * m + (1 - b1) * g
    mb = np.abs(b1 * m) + np.abs((1 - b1) * g)
    v1 = b2 * v + (1 - b2) * g * g
    c1, c2 = 1 - b1 ** float(t), 1 - b2 ** float(t)
    denom = np.sqrt(v1) / np.sqrt(c2) + eps
    upd = (lr / c1) * (m1 / denom)
    return AdamStep(p - upd, m1, v1, upd, mb, (lr / c1) * (mb / denom))


def reduce(slab, nslab, stride, count, dst0=None, accumulate=False):
    """dst[i] (+)= sum_{b < nslab} slab[b * stride + i], i < count.  Returns (sums [count], sum of |terms| [count])."""
    s = _d(slab).ravel()
    idx = np.arange(nslab)[:, None] * stride + np.arange(count)[None, :]
    rows = s[idx]
    tot, mag = rows.sum(0), np.abs(rows).sum(0)
    if accumulate:
        tot, mag = tot + _d(dst0)[:count], mag + np.abs(_d(dst0)[:count])
    return tot, mag


# ------------------------------------------------------------------------------------------------
# shared inputs of the loss tests
# ------------------------------------------------------------------------------------------------
LFAK, L1, L2 = 5.0, 0.5, 0.25       # the loss weights of the loss tests (exact in float32)
LOSS_RTOL = 1e-5                    # tests/test_gpu_glue.py: every loss value within 1e-5 relative of the reference


def mask_inputs(n, hw):
    """Z [n, hw] float32 in [0, 1) with a per-image scale log-uniform in [1e-3, 1]: the images' sums differ by orders of
    magnitude, so a partial sum credited to the wrong image shows."""
    rs = np.random.RandomState(1000 + n + hw)
    scale = 10.0 ** rs.uniform(-3, 0, size=(n, 1))
    return (rs.rand(n, hw) * scale).astype(np.float32)


def loss_inputs(n, bce):
    """pred [4n] float32 uniform in (0, 1), slots [B | A | replaced | injected], and y [n]: randn, or 0/1 under bce, where the
    A slot also holds an exact 0 (first image) and, from two images on, an exact 1 (last image)."""
    rs = np.random.RandomState(2000 + 2 * n + int(bool(bce)))
    pred = rs.uniform(0.02, 0.98, size=4 * n).astype(np.float32)
    if bce:
        y = rs.randint(0, 2, size=n).astype(np.float32)
        pred[n] = 0.0
        if n > 1:
            pred[2 * n - 1] = 1.0
    else:
        y = rs.randn(n).astype(np.float32)
    return pred, y
