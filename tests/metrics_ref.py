"""The direct form of the evaluation counts that cgs_iou_curve / cgs_iou_counts compute (include/cgs_hip.h), the checker of
tests/test_metrics_host.py and tests/test_gpu_metrics.py: per threshold one numpy compare of the float32 array with a float32 scalar,
one `&` and one `|` -- what Handler.get_iou does today (main.py:1265-1270), and nothing of the kernel's histogram formulation."""
import numpy as np


def curve(v, truth, thresholds, inclusive=False):
    """(inter [T], union [T]) int64, thresholds in the order given."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    truth = np.asarray(truth).reshape(-1) != 0
    inter, union = [], []
    with np.errstate(invalid="ignore"):
        for t in np.asarray(thresholds, dtype=np.float32).reshape(-1):
            on = (v >= np.float32(t)) if inclusive else (v > np.float32(t))
            inter.append(np.count_nonzero(truth & on))
            union.append(np.count_nonzero(truth | on))
    return np.array(inter, dtype=np.int64), np.array(union, dtype=np.int64)


def counts(labels, truth):
    """[K, 2] int64 = (intersection, union) of each of the K stacks of labels with truth."""
    truth = np.asarray(truth).reshape(-1) != 0
    labels = np.asarray(labels).reshape(-1, truth.size) != 0
    return np.array([[np.count_nonzero(truth & m), np.count_nonzero(truth | m)] for m in labels], dtype=np.int64)
