"""Literal fp64 numpy oracle of the validation scalars (test infrastructure): test_sample_depth of the reference
(train_rcmvsnet.py:449-499) = cas_mvsnet_loss (models/modules.py:527-546), AbsDepthError_metrics and Thres_metrics
(utils.py:139-159), restated with boolean-mask indexing as they are written there -- except that every sum is fp64.  The
difference ``est - gt`` is the one fp32 subtraction the reference's tensors make; everything after it is fp64."""
import numpy as np

SCALAR_KEYS = ("loss", "depth_loss", "abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error",
               "thres2mm_accu", "thres4mm_accu", "thres8mm_accu", "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror")


def _mean(x):
    return float(np.sum(x, dtype=np.float64) / x.size) if x.size else float("nan")      # torch.mean of nothing is NaN


def _error(est, gt, mask):
    est, gt = np.asarray(est, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    m = np.asarray(mask, dtype=np.float32) > 0.5
    with np.errstate(invalid="ignore"):
        return (est[m] - gt[m]).astype(np.float64)


def smooth_l1(est, gt, mask):
    """F.smooth_l1_loss(est[mask], gt[mask], reduction='mean'), beta = 1 -> (sum, count)"""
    d = _error(est, gt, mask)
    e = np.abs(d)
    with np.errstate(invalid="ignore"):
        terms = np.where(e < 1.0, 0.5 * d * d, e - 0.5)
    return float(np.sum(terms, dtype=np.float64)), int(d.size)


def thres_metrics(est, gt, mask, thres):
    e = np.abs(_error(est, gt, mask))
    with np.errstate(invalid="ignore"):
        return _mean((e > thres).astype(np.float64))


def abs_depth_error(est, gt, mask, thres=None):
    e = np.abs(_error(est, gt, mask))
    if thres is not None:
        with np.errstate(invalid="ignore"):
            e = e[(e >= float(thres[0])) & (e <= float(thres[1]))]
        if e.shape[0] == 0:
            return 0.0
    return _mean(e)


def record(triples, dlossw=None):
    """triples: [(est, gt, mask)] of the three stages -> the 12 scalars plus the raw sums and counts (validation.SUM_KEYS /
    COUNT_KEYS names)"""
    w = [1.0, 1.0, 1.0] if dlossw is None else [float(x) for x in dlossw]
    out, loss = {}, 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, (est, gt, mask) in enumerate(triples):
            s, n = smooth_l1(est, gt, mask)
            out["sl1_stage%d" % (k + 1)], out["n_stage%d" % (k + 1)] = s, n
            depth_loss = np.float64(s) / np.float64(n)
            loss = loss + w[k] * depth_loss
    est, gt, mask = triples[-1]
    e = np.abs(_error(est, gt, mask))
    out.update(loss=float(loss), depth_loss=float(depth_loss), abs_depth_error=abs_depth_error(est, gt, mask),
               sum_abs_error=float(np.sum(e, dtype=np.float64)))
    for t, (lo, hi) in zip((2, 4, 8), ((0.0, 2.0), (2.0, 4.0), (4.0, 8.0))):
        err = thres_metrics(est, gt, mask, t)
        out["thres%dmm_error" % t], out["thres%dmm_accu" % t] = err, 1.0 - err
        out["thres%dmm_abserror" % t] = abs_depth_error(est, gt, mask, [lo, hi])
        with np.errstate(invalid="ignore"):
            out["count_gt%dmm" % t] = int(np.sum(e > t))
            band = e[(e >= lo) & (e <= hi)]
        out["band%dmm_sum" % t], out["band%dmm_count" % t] = float(np.sum(band, dtype=np.float64)), int(band.size)
    return out
