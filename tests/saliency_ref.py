"""Numpy restatement of the saliency sweep (cgs_amd.saliency / cgs_saliency_sweep): the masks are Handler._saliency_post's own, one call per
threshold, counted with `&` / `|`; the normaliser is restated from that function's two lines.  Used by tests/test_saliency_host.py and
tests/test_gpu_saliency.py."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from cgs_amd import handler  # noqa: E402


def hard(sal, preds, t, salglobal):
    """uint8 [n,64,64]: _saliency_post's thresholded map.  t goes in as a Python float, as argparse hands --salience-thresh over."""
    with np.errstate(all="ignore"):                          # inf / inf, 0 * inf, x / tiny overflowing: NaN and inf are the point
        return handler.Handler._saliency_post(sal[:, None], preds, float(t), bool(salglobal))[1][:, 0]


def scale(sal, t, salglobal):
    """float32 [n]: the normaliser _saliency_post builds before it adds `tiny`."""
    n = sal.shape[0]
    with np.errstate(all="ignore"):
        if salglobal:
            s = np.where(sal >= 0, sal, 0.0).mean() * float(t)
            assert s.dtype == np.float32
            return np.full(n, s, dtype=np.float32)
        return np.sort(sal.reshape(n, -1), axis=-1)[:, int(sal.shape[-1] * sal.shape[-2] * float(t))]


def sweep(sal, preds, truth, thresholds, salglobal):
    """(inter int64 [T], union int64 [T], scale float32 [n,T], masks uint8 [T,n,64,64]) in the order of `thresholds`."""
    truth = np.asarray(truth).astype(bool)
    masks = np.stack([hard(sal, preds, t, salglobal) for t in thresholds])
    inter = np.array([np.count_nonzero(truth & m.astype(bool)) for m in masks], dtype=np.int64)
    union = np.array([np.count_nonzero(truth | m.astype(bool)) for m in masks], dtype=np.int64)
    return inter, union, np.stack([scale(sal, t, salglobal) for t in thresholds], axis=1), masks
