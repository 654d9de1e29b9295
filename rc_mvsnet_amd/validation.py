"""The validation pass of the reference's training script (train_rcmvsnet.py:229-258 after every epoch, :262-275 as
``--mode test``, ``test_sample_depth`` at :449-499): the estimated depth of the train-variant ``CascadeMVSNet`` in eval mode
against the DTU ground-truth depth maps of ``mvs_dataset.DTUValDataset``.

Per item the reference forms 12 scalars -- the supervised multi-stage smooth-L1 loss (``cas_mvsnet_loss``), the mean absolute
depth error, the 2 / 4 / 8 mm error and accuracy rates and their band-wise absolute errors -- with about a dozen boolean-mask
indexings, each a ``nonzero`` with a blocking read-back.  Here they are ONE launch (csrc/depth_metrics.hip,
``rcmvs_depth_metrics``) that writes the item's record into a row of an fp64 table on the device; ``validate`` reads the table
every ``summary_freq`` items and at the end, never per item.  DESIGN.md section 4, "Validation".

``cas_mvsnet_loss``, ``Thres_metrics`` and ``AbsDepthError_metrics`` carry the reference's names and signatures (models/modules.py,
utils.py) over the same kernel.  No CPU path: tensors must be on the GPU.
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib, mvs_dataset
from .ops import _chk, _stream

SCALAR_KEYS = ("loss", "depth_loss", "abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error",
               "thres2mm_accu", "thres4mm_accu", "thres8mm_accu", "thres2mm_abserror", "thres4mm_abserror", "thres8mm_abserror")
SUM_KEYS = ("sl1_stage1", "sl1_stage2", "sl1_stage3", "sum_abs_error", "band2mm_sum", "band4mm_sum", "band8mm_sum")
COUNT_KEYS = ("n_stage1", "n_stage2", "n_stage3", "count_gt2mm", "count_gt4mm", "count_gt8mm", "band2mm_count", "band4mm_count",
              "band8mm_count")
RECORD = _lib.CONSTANTS["RCMVS_DM_RECORD"]      # doubles per table row = the 12 scalars, the 16 raw sums / counts, 4 zeros
RAW = _lib.CONSTANTS["RCMVS_DM_RAW"]            # column of the first raw sum
DLOSSW = (0.5, 1.0, 2.0)        # --dlossw default, train_rcmvsnet.py:61
STAGES = ("stage1", "stage2", "stage3")
THRESHOLDS = (2.0, 4.0, 8.0)
BANDS = ((0.0, 2.0), (2.0, 4.0), (4.0, 8.0))

MAX_WORKSPACES = 8
_WORKSPACES = {}        # (device, stage sizes) -> workspace; validate() holds one entry, the reference-named wrappers bypass it


def _new_workspace(device, sizes):
    nbytes = _lib.load().rcmvs_depth_metrics_workspace_bytes(*sizes)
    if nbytes <= 0:
        raise _lib.RcmvsError(f"depth_metrics: empty stage among sizes {sizes}")
    raw = torch.zeros(nbytes + 128, dtype=torch.uint8, device=device)
    at = -raw.data_ptr() % 128                                      # the ticket and every partial on a 128-byte line of their own
    return raw[at:at + nbytes]


def _workspace(device, sizes):
    """The kernel's ticket + per-block partials for these stage sizes: zero-filled once, left ready by every call that completes.
    A call that does NOT complete (a failed launch, a fault elsewhere on the device while it is in flight) can leave the ticket
    part-drawn, after which the wrong block of a later call (or none) takes itself for the last one and the record is wrong or missing:
    ``_launch`` drops the workspace when the library reports a failure, ``reset_workspaces`` drops them all (``validate`` does so
    at the start of every pass), and the next call starts from a fresh zero-filled one."""
    key = (str(device), sizes)
    ws = _WORKSPACES.get(key)
    if ws is None:
        if len(_WORKSPACES) >= MAX_WORKSPACES:                      # many shapes in one process: start over rather than grow
            _WORKSPACES.clear()
        ws = _WORKSPACES[key] = _new_workspace(device, sizes)
    return ws


def reset_workspaces():
    """Forget every cached workspace (see ``_workspace``)."""
    _WORKSPACES.clear()


def _plane(t, name):
    if t.dim() != 3:
        raise _lib.RcmvsError(f"depth_metrics: {name} must be (1,h,w), got {tuple(t.shape)}")
    if t.shape[0] != 1:
        raise _lib.RcmvsError(f"depth_metrics: {name} has batch {t.shape[0]}; the limit is batch 1 (the reference validates at batch size 1)")
    return t


def _launch(triples, dlossw, table, slot, images, events=None, cached=True):
    """triples: three (est, gt, mask) of (1,h,w) fp32 tensors.  -> (row, images or None).  cached=False: a workspace of its own
    (callers with arbitrary plane sizes, which would otherwise grow the cache without bound)."""
    for k, (est, gt, mask) in enumerate(triples):
        for t, name in ((est, "depth"), (gt, "depth_gt"), (mask, "mask")):
            _plane(t, f"{name} of stage {k + 1}")
        if not (est.shape == gt.shape == mask.shape):
            raise _lib.RcmvsError(f"depth_metrics: stage {k + 1}: depth {tuple(est.shape)}, depth_gt {tuple(gt.shape)} and mask {tuple(mask.shape)} differ")
    device = triples[2][0].device
    sizes = tuple(int(t[0].numel()) for t in triples)
    if table is None:
        table = torch.empty((slot + 1, RECORD), dtype=torch.float64, device=device)
    if table.dim() != 2 or table.shape[1] != RECORD or not 0 <= slot < table.shape[0]:
        raise _lib.RcmvsError(f"depth_metrics: row {slot} of a table of shape {tuple(table.shape)}: expected (rows > slot, {RECORD})")
    w = None
    if dlossw is not None:
        if len(dlossw) != 3:
            raise _lib.RcmvsError(f"depth_metrics: dlossw needs one weight per stage, got {list(dlossw)}")
        w = (ctypes.c_double * 3)(*[float(x) for x in dlossw])
    out = None
    if images:
        out = {"depth_est": torch.empty_like(triples[2][0]), "errormap": torch.empty_like(triples[2][0])}
    ws = _workspace(device, sizes) if cached else _new_workspace(device, sizes)      # held until the launch is enqueued
    args = []
    for est, gt, mask in triples:
        args += [_chk(est, "depth"), _chk(gt, "depth_gt"), _chk(mask, "mask"), est.numel()]
    args += [ctypes.cast(w, ctypes.c_void_p) if w is not None else ctypes.c_void_p(0), _chk(table, "table", torch.float64), slot,
             _chk(out["depth_est"], "depth_est") if out else ctypes.c_void_p(0), _chk(out["errormap"], "errormap") if out else ctypes.c_void_p(0),
             _chk(ws, "workspace", torch.uint8)]
    stream = _stream()
    try:
        if events is None:
            _lib.call("rcmvs_depth_metrics", *args, stream)
        else:
            _lib.call("rcmvs_depth_metrics_timed", *args, ctypes.c_void_p(events[0].cuda_event), ctypes.c_void_p(events[1].cuda_event), stream)
    except _lib.RcmvsError:
        _WORKSPACES.pop((str(device), sizes), None)                 # its ticket may be part-drawn: never reuse it
        raise
    return table[slot], out


def depth_metrics(outputs, depth_gt_ms, mask_ms, dlossw=None, table=None, slot=0, images=False, events=None):
    """Every scalar of test_sample_depth for one item, in one launch and without a host read.

    outputs: the model's output dict (``outputs["stageK"]["depth"]`` (1,h,w)); depth_gt_ms / mask_ms: the reference's ``depth``
    and ``mask`` stage dicts as (1,h,w) fp32 tensors on the GPU; dlossw: three stage weights (None = 1, 1, 1, as cas_mvsnet_loss).
    Row ``slot`` of ``table`` ((rows, RECORD) fp64 on the device; None = a fresh one) receives the record; returned as a device
    tensor (``record_to_dict`` reads it).  images=True: -> (row, {"depth_est": est * mask, "errormap": |est - gt| * mask}) of
    the last stage, written by the same launch.  events: two recorded torch.cuda.Event that receive the kernel's own start / stop."""
    triples = [(outputs[k]["depth"], depth_gt_ms[k], mask_ms[k]) for k in STAGES]
    row, out = _launch(triples, dlossw, table, slot, images, events)
    return (row, out) if images else row


def record_to_dict(row):
    """A table row (device or host tensor, or array of RECORD doubles) -> {SCALAR_KEYS: float, SUM_KEYS: float, COUNT_KEYS: int}.
    This is the host read."""
    r = row.detach().cpu().numpy() if isinstance(row, torch.Tensor) else np.asarray(row, dtype=np.float64)
    if r.shape != (RECORD,):
        raise _lib.RcmvsError(f"record_to_dict: expected {RECORD} doubles, got shape {r.shape}")
    rec = {k: float(r[i]) for i, k in enumerate(SCALAR_KEYS)}
    rec.update({k: float(r[RAW + i]) for i, k in enumerate(SUM_KEYS)})
    rec.update({k: int(r[RAW + len(SUM_KEYS) + i]) for i, k in enumerate(COUNT_KEYS)})
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# the reference's names (models/modules.py:527-546, utils.py:139-159)
# ---------------------------------------------------------------------------------------------------------------------
def cas_mvsnet_loss(inputs, depth_gt_ms, mask_ms, **kwargs):
    """-> (total_loss, depth_loss of the last stage), 0-d fp32 tensors on the device"""
    row = depth_metrics(inputs, depth_gt_ms, mask_ms, dlossw=kwargs.get("dlossw", None))
    return row[0].to(torch.float32), row[1].to(torch.float32)


def _last_stage_row(depth_est, depth_gt, mask):
    """the record of one (est, gt, mask) triple as the last stage; the first two stages read four of its pixels"""
    if mask.dtype == torch.bool:                                   # the reference passes ``mask > 0.5``
        mask = mask.to(torch.float32)
    head = tuple(t.reshape(1, 1, -1)[:, :, :min(4, t.numel())] for t in (depth_est, depth_gt, mask))
    return _launch([head, head, (depth_est, depth_gt, mask)], None, None, 0, False, cached=False)[0]


def Thres_metrics(depth_est, depth_gt, mask, thres):
    """fraction of the mask's pixels with |est - gt| > thres; thres is 2, 4 or 8 (the ones the kernel counts)"""
    assert isinstance(thres, (int, float))
    if float(thres) not in THRESHOLDS:
        raise _lib.RcmvsError(f"Thres_metrics: thres {thres} is not one of {THRESHOLDS}")
    return _last_stage_row(depth_est, depth_gt, mask)[3 + THRESHOLDS.index(float(thres))].to(torch.float32)


def AbsDepthError_metrics(depth_est, depth_gt, mask, thres=None):
    """mean |est - gt| over the mask, or over its pixels with thres[0] <= error <= thres[1] (0 when there is none);
    thres is None, [0, 2], [2, 4] or [4, 8]"""
    row = _last_stage_row(depth_est, depth_gt, mask)
    if thres is None:
        return row[2].to(torch.float32)
    band = (float(thres[0]), float(thres[1]))
    if band not in BANDS:
        raise _lib.RcmvsError(f"AbsDepthError_metrics: band {list(thres)} is not one of {BANDS}")
    return row[9 + BANDS.index(band)].to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
def item_inputs(item):
    """an item of DTUValDataset -> (imgs (1,V,3,H,W), proj_matrices, depth_values (1,D)) on the item's device"""
    return item["imgs"][None], item["proj_dev"], item["depth_values_dev"]


def mean_record(records):
    """DictAverageMeter.mean (utils.py:103-122): the mean over ITEMS of the per-item scalars, not a pooled mean over pixels"""
    return {k: sum(r[k] for r in records) / len(records) for k in SCALAR_KEYS} if records else {}


def validate(model, dataset, dlossw=DLOSSW, indices=None, workers=4, summary_freq=10, out=None, on_summary=None, forward_fn=None,
             image_dir=None, stats=None):
    """One pass over ``dataset`` (a DTUValDataset) -> (records, mean): ``records[i]`` = record_to_dict of item ``indices[i]``,
    ``mean`` = mean_record(records).

    model: the train-variant CascadeMVSNet; run in eval mode under no_grad, its previous ``training`` flag is restored.
    Per item: one forward and one depth_metrics launch into row i of one (n, RECORD) table -- no host synchronisation; the
    table's new rows are read when ``i % summary_freq == 0`` and at the end.  At each such read of item i, ``on_summary(i, record)``
    is called and, with ``out``, one line is printed.  forward_fn(model, imgs, proj, depth_values) -> outputs (default:
    ``model(...)[0]``).  image_dir: write the last stage's masked depth and error map of every summary item as PFM files.
    stats: a dict that receives ``loader_wait_s`` (time spent waiting for items) and ``items``."""
    from .data_io import save_pfm
    idx = list(range(len(dataset))) if indices is None else list(indices)
    n = len(idx)
    forward_fn = forward_fn or (lambda m, *a: m(*a)[0])
    was_training = model.training
    reset_workspaces()                                                           # a pass never inherits a ticket of an earlier, possibly lost, launch
    model.eval()
    records, wait = [], 0.0
    try:
        with torch.no_grad():
            table = torch.zeros((max(n, 1), RECORD), dtype=torch.float64, device=dataset.device)
            items = mvs_dataset.prefetch(dataset, indices=idx, workers=workers, depth=2 * max(1, workers))
            for i in range(n):
                t0 = time.perf_counter()
                item = next(items)
                wait += time.perf_counter() - t0
                summary = i % summary_freq == 0
                outputs = forward_fn(model, *item_inputs(item))
                want = summary and image_dir is not None
                got = depth_metrics(outputs, item["depth_dev"], item["mask_dev"], dlossw=dlossw, table=table, slot=i, images=want)
                if summary or i == n - 1:
                    host = table[len(records):i + 1].cpu()                       # the host read: once per summary_freq items
                    records += [record_to_dict(row) for row in host]
                if summary:
                    if want:
                        os.makedirs(image_dir, exist_ok=True)
                        for name, img in got[1].items():
                            save_pfm(os.path.join(image_dir, "{:0>6}_{}.pfm".format(idx[i], name)), img[0].cpu().numpy())
                    if on_summary is not None:
                        on_summary(i, records[i])
                    if out is not None:
                        r = records[i]
                        print("Iter {}/{}, test loss = {:.3f}, depth loss = {:.3f}, thres2mm_accu = {:.3f}, thres4mm_accu = {:.3f}, "
                              "thres8mm_accu = {:.3f}".format(i, n, r["loss"], r["depth_loss"], r["thres2mm_accu"], r["thres4mm_accu"],
                                                              r["thres8mm_accu"]), file=out, flush=True)
    finally:
        model.train(was_training)
    if stats is not None:
        stats.update(loader_wait_s=wait, items=n)
    return records, mean_record(records)
