"""Binary ranking metrics of device tensors: sklearn.metrics.roc_auc_score / average_precision_score for binary labels, computed on
the GPU (tlc_binary_rank_metrics in csrc/lp_metrics.hip through ops.binary_rank_metrics).

sklearn's binary semantics with pos_label 1: scores in descending order, equal scores one threshold.  ROC-AUC is the Mann-Whitney
count divided by 2 P N with one rounding (sklearn's trapezoid area in exact arithmetic); AP is sklearn's
-sum(diff(recall) * precision[:-1]).  One class only: AUC NaN, AP 0.0 without positives / 1.0 without negatives, with the warnings
sklearn 1.7 gives.

Differences from sklearn: the labels must be 0 or 1 (sklearn also accepts any two values, e.g. {0, 2}, and takes the larger as
the positive class); scores must be float32 / float64 and labels bool / uint8 / int64 / float32 CUDA tensors.  NaN or infinite
scores, an empty input and labels outside {0, 1} raise ValueError.  These functions return Python floats, so they wait for the
device; ops.binary_rank_metrics is the asynchronous form.  There is no CPU fallback.
"""
import warnings

from . import ops


class UndefinedMetricWarning(UserWarning):
    """A metric is undefined for the input (sklearn.exceptions.UndefinedMetricWarning)."""


def check_status(status, what="y_true / y_score"):
    """Raise ValueError for the status bits of ops.binary_rank_metrics (host ints), as sklearn does for such input."""
    if status & ops.RANK_EMPTY:
        raise ValueError("%s: found an empty segment (0 samples); a minimum of 1 is required" % what)
    if status & ops.RANK_NONFINITE:
        raise ValueError("%s: y_score contains NaN or infinity" % what)
    if status & ops.RANK_BAD_LABEL:
        raise ValueError("%s: y_true must hold only 0 and 1 (binary labels, pos_label 1)" % what)


def warn_single_class(n_pos, n_neg):
    """The warnings sklearn 1.7 gives for one class only (the values are already NaN / 0.0 / 1.0)."""
    if n_pos == 0 or n_neg == 0:
        warnings.warn("Only one class is present in y_true. ROC AUC score is not defined in that case.", UndefinedMetricWarning,
                      stacklevel=3)
    if n_pos == 0:
        warnings.warn("No positive class found in y_true, recall is set to one for all thresholds.", UserWarning, stacklevel=3)


def roc_auc_ap(y_true, y_score):
    """(ROC-AUC, average precision) of one binary problem from one sort on the device -> two Python floats."""
    import torch
    auc, ap, n_pos, n_neg, status = ops.binary_rank_metrics(y_score, y_true)
    # one copy to the host: the counts (< 2^31) and the status word are exact in float64
    v = torch.cat([auc, ap, n_pos.double(), n_neg.double(), status.double()]).cpu().tolist()
    check_status(int(v[4]))
    warn_single_class(int(v[2]), int(v[3]))
    return float(v[0]), float(v[1])


def roc_auc_score(y_true, y_score):
    """sklearn.metrics.roc_auc_score(y_true, y_score) for binary 0/1 labels, on the device.  NaN for one class only."""
    auc, _ = _quiet(y_true, y_score, ap=False)
    return auc


def average_precision_score(y_true, y_score):
    """sklearn.metrics.average_precision_score(y_true, y_score) for binary 0/1 labels, on the device."""
    _, ap = _quiet(y_true, y_score, ap=True)
    return ap


def _quiet(y_true, y_score, ap):
    # each single metric gives only its own warning, as sklearn does
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        auc, apv = roc_auc_ap(y_true, y_score)
    for w in caught:
        if (w.category is UndefinedMetricWarning) != ap:
            warnings.warn(w.message, w.category, stacklevel=3)
    return auc, apv
