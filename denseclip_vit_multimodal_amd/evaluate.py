"""On-device validation: class maps, mIoU / pixel accuracy, depth errors and the validation losses,
from the heads' low-res outputs, without materialising the resized (B, 19, H, W) logits.

The reference's validate() (train_denseclip.py:294-684) resizes both heads to the label size, then
takes argmax -> confusion matrix / accuracy (denseclip/utils.py:109-139, compute_segmentation_metrics),
the depth errors (utils/depth_metrics.py:12-88, compute_depth_errors), the masked RMSE (:589-593)
and the validation CE / SILog (:497, :524).  Here one fused kernel per head (csrc/headeval.hip,
torch.ops.dclip_eval.*) reads the low-res map and the labels / targets once and adds into running
device-resident sums; `Evaluator.compute()` is the only call that synchronises with the host.

    ev = Evaluator()
    for img, seg, depth, mask in loader:
        out = model.forward_lowres(img)
        ev.update(out['seg'], out['depth'], seg, depth, mask)
    metrics = ev.compute()

The depth figures are POOLED over every evaluated pixel of every update.  The reference's
DepthMetricsAggregator (utils/depth_metrics.py:122-163) instead averages the per-call results of
compute_depth_errors, which weights a call with few valid pixels like one with many;
`update(..., per_call=True)` returns the call's own sums (`metrics_from_sums` turns them into that
call's figures) for callers who want that average.

Multi-scale + flip test-time augmentation (the reference's test.py --aug-test) runs on the same
footing: `forward_views` keeps the low-res maps of every view, and `predict_tta` /
`Evaluator.update_views` / `validate(..., tta=dict(...))` hand them to one fused kernel per head
(csrc/headensemble.hip) that averages the resized, mirrored-back views in registers.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _torch_ops

DEPTH_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
TTA_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)  # the reference's --aug-test ratios (test.py:93-96)
AVERAGES = ("logits", "probs")
_LAB_DTYPES = (torch.int64, torch.int32, torch.uint8)


def _E():
    """torch.ops.dclip_eval (loads libdclip_torch.so on first use; raises if it is missing)."""
    _torch_ops.load()
    return torch.ops.dclip_eval


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"evaluate: {what} must be a GPU tensor (the MI355X path has no CPU fallback)")


def _hw(t):
    return int(t.shape[-2]), int(t.shape[-1])


def upsample_argmax(logits, size):
    """argmax over the classes of the bilinear (align_corners=False) resize of `logits` (B, K, h, w)
    to `size`: uint8 (B, H, W), the lowest class index among equal maxima (torch.argmax's rule)."""
    _need_gpu(logits, "logits")
    return _E().upsample_argmax(logits.detach().contiguous(), int(size[0]), int(size[1]))


def predict(model, img, size=None):
    """{'seg': uint8 (B, H, W) class map, 'depth': fp32 (B, 1, H, W)} of `model` on `img`, resized
    to `size` (default: the image size); either is None for a model without that head."""
    from . import ops
    size = tuple(img.shape[-2:]) if size is None else (int(size[0]), int(size[1]))
    with torch.no_grad():
        low = model.forward_lowres(img)
        seg, depth = low["seg"], low["depth"]
        return {"seg": upsample_argmax(seg, size) if seg is not None else None,
                "depth": ops.upsample(depth, size) if depth is not None else None}


def _probs(average):
    """the `probs` flag of the ensemble ops from the averaging rule's name"""
    if average not in AVERAGES:
        raise ValueError(f"average={average!r}: 'logits' (the mean of the views' resized logits, the reference's "
                         "aug_test) or 'probs' (the mean of their softmax, mmseg's rule)")
    return average == "probs"


def tta_views(img, scales=TTA_SCALES, flip=True):
    """Yield (view_img, flipped) for every scale, each followed by its horizontal mirror when `flip`:
    F.interpolate(bilinear, align_corners=False) of the normalised image `img` (B, 3, H, W) to
    (int(H s + 0.5), int(W s + 0.5)); scale 1 passes `img` through untouched.  This is torch's resize
    of the float image, not cv2's 8-bit resize of the decoded one, which mmcv's MultiScaleFlipAug
    uses: parity with that is not pinned."""
    H, W = _hw(img)
    for s in scales:
        size = (int(H * s + 0.5), int(W * s + 0.5))
        view = img if size == (H, W) else F.interpolate(img, size=size, mode="bilinear", align_corners=False)
        yield view, False
        if flip:
            yield view.flip(-1), True


def forward_views(model, img, scales=TTA_SCALES, flip=True):
    """`model.forward_lowres` on every view of `tta_views`, one view at a time under no_grad, keeping
    only the low-res maps: (seg_views, depth_views, flips), a list per head (None for a model
    without that head) and the views' flip flags."""
    segs, depths, flips = [], [], []
    with torch.no_grad():
        for view, flipped in tta_views(img, scales, flip):
            low = model.forward_lowres(view)
            if low["seg"] is not None:
                segs.append(low["seg"].detach().contiguous())
            if low["depth"] is not None:
                depths.append(low["depth"].detach().contiguous())
            flips.append(int(flipped))
    return segs or None, depths or None, flips


def predict_tta(model, img, scales=TTA_SCALES, flip=True, average="logits", size=None):
    """`predict` under multi-scale + flip test-time augmentation: {'seg': uint8 (B, H, W), 'depth':
    fp32 (B, 1, H, W)} from the mean over the views of the resized, mirrored-back outputs
    (csrc/headensemble.hip: no per-view full-size tensor).  `average`: 'logits' or 'probs' for the
    class map (the depth is always the mean of the predictions)."""
    probs = _probs(average)
    H, W = _hw(img) if size is None else (int(size[0]), int(size[1]))
    segs, depths, flips = forward_views(model, img, scales, flip)
    E = _E()
    return {"seg": E.ensemble_argmax(segs, flips, H, W, probs) if segs else None,
            "depth": E.ensemble_depth(depths, flips, H, W) if depths else None}


def metrics_from_sums(cm=None, ce_sums=None, depth_sums=None, lambd=0.5):
    """The reference's formulas on host copies of an Evaluator's state (any of them may be None)."""
    out = {}
    if cm is not None:
        cm = np.asarray(cm, dtype=np.int64)
        diag = np.diag(cm).astype(np.float64)
        total = float(cm.sum())
        union = (cm.sum(0) + cm.sum(1)).astype(np.float64) - diag
        iou = diag / (union + 1e-8)
        out.update(accuracy=float(diag.sum()) / (total + 1e-5), class_iou=iou, mean_iou=float(np.nanmean(iou)),
                   confusion_matrix=cm)
    if ce_sums is not None:
        s, n = float(ce_sums[0]), float(ce_sums[1])
        out["loss_seg"] = s / n if n > 0 else None
    if depth_sums is not None:
        d = [float(v) for v in depth_sums]
        n = d[0]
        if n > 0:
            out.update(abs_rel=d[3] / n, sq_rel=d[4] / n, rmse=math.sqrt(d[1] / n), rmse_log=math.sqrt(d[2] / n),
                       a1=d[5] / n, a2=d[6] / n, a3=d[7] / n)
        else:
            out.update({k: None for k in DEPTH_KEYS})
        T = d[8]
        out["rmse_masked"] = math.sqrt(d[9] / T) if T > 0 else None
        # SILogLoss (losses.py): sum d^2 / T - lambd (sum d)^2 / T^2, 0 on an empty mask
        out["loss_silog"] = d[11] / T - lambd * d[10] ** 2 / T ** 2 if T > 0 else 0.0
    return out


class Evaluator:
    """Running validation state on the device: `cm` (int64 K x K, row = target, column =
    prediction), `ce_sums` (float64[2]: CE sum, #valid pixels) and `depth_sums` (float64[12],
    include/dclip.h: dclip_upsample_eval_depth).  `update` launches the fused kernels on the current
    stream and neither synchronises nor returns a new tensor, so it can be captured after
    `forward_lowres` in one HIP graph; `compute` is the only call that synchronises."""

    def __init__(self, num_classes=19, ignore_index=255, min_depth=1e-3, max_depth=80.0, clamp_pred=True,
                 device=None, lambd=0.5, eps=1e-6):
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.num_classes, self.ignore_index = int(num_classes), int(ignore_index)
        self.min_depth, self.max_depth, self.clamp_pred = float(min_depth), float(max_depth), bool(clamp_pred)
        self.lambd, self.eps = float(lambd), float(eps)
        self.device = torch.device(device)
        self.cm = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=self.device)
        self.ce_sums = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.depth_sums = torch.zeros(12, dtype=torch.float64, device=self.device)

    def reset(self):
        for t in (self.cm, self.ce_sums, self.depth_sums):
            t.zero_()

    def update(self, seg_lowres=None, depth_lowres=None, seg_target=None, depth_target=None, depth_mask=None,
               per_call=False):
        """Add one batch: `seg_lowres` (B, K, h, w) with `seg_target` (B, H, W) int64 / int32 / uint8,
        `depth_lowres` (B, 1, h, w) with `depth_target` (B, [1,] H, W) and `depth_mask` (same shape,
        bool / uint8, None = all valid).  Returns None, or with per_call=True the call's own
        {'cm', 'ce_sums', 'depth_sums'} (device tensors, also added to the running state)."""
        E = _E()
        own = None
        if per_call:
            own = {"cm": torch.zeros_like(self.cm), "ce_sums": torch.zeros_like(self.ce_sums),
                   "depth_sums": torch.zeros_like(self.depth_sums)}
        if seg_lowres is not None and seg_target is not None:
            _need_gpu(seg_lowres, "seg_lowres")
            if seg_lowres.shape[1] != self.num_classes:
                raise ValueError(f"Evaluator: {seg_lowres.shape[1]} classes, built for {self.num_classes}")
            lab = seg_target.reshape(seg_target.shape[0], *_hw(seg_target))
            if lab.dtype not in _LAB_DTYPES:
                lab = lab.long()
            cm, ce = (own["cm"], own["ce_sums"]) if per_call else (self.cm, self.ce_sums)
            E.seg_update(seg_lowres.detach().contiguous(), lab.contiguous(), self.ignore_index, cm, ce, False)
            if per_call:
                self.cm += cm
                self.ce_sums += ce
        if depth_lowres is not None and depth_target is not None:
            _need_gpu(depth_lowres, "depth_lowres")
            B = depth_target.shape[0]
            tg = depth_target.detach().reshape(B, *_hw(depth_target)).float().contiguous()
            mk = None
            if depth_mask is not None:
                mk = depth_mask.reshape(B, *_hw(depth_mask)).to(torch.uint8).contiguous()
            sums = own["depth_sums"] if per_call else self.depth_sums
            E.depth_update(depth_lowres.detach().contiguous(), tg, mk, self.min_depth, self.max_depth,
                           self.clamp_pred, self.eps, sums, False)
            if per_call:
                self.depth_sums += sums
        return own

    def update_views(self, seg_views=None, depth_views=None, flips=(), seg_target=None, depth_target=None,
                     depth_mask=None, average="logits", per_call=False):
        """`update` on the ensemble of one batch's views (`forward_views`): lists of low-res maps
        (B, K, h_v, w_v) / (B, 1, h_v, w_v) and the views' flip flags; the metrics are taken from the
        mean over the views of the resized, mirrored-back outputs (`average`: 'logits' or 'probs'
        for the class map and the CE).  Same contract as `update`: no host synchronisation, no new
        tensor besides the workspace, added to the running state; per_call=True returns the call's
        own sums."""
        probs = _probs(average)
        E = _E()
        flips = [int(f) for f in flips]
        own = None
        if per_call:
            own = {"cm": torch.zeros_like(self.cm), "ce_sums": torch.zeros_like(self.ce_sums),
                   "depth_sums": torch.zeros_like(self.depth_sums)}
        if seg_views and seg_target is not None:
            for v in seg_views:
                _need_gpu(v, "seg_views")
                if v.shape[1] != self.num_classes:
                    raise ValueError(f"Evaluator: {v.shape[1]} classes, built for {self.num_classes}")
            lab = seg_target.reshape(seg_target.shape[0], *_hw(seg_target))
            if lab.dtype not in _LAB_DTYPES:
                lab = lab.long()
            cm, ce = (own["cm"], own["ce_sums"]) if per_call else (self.cm, self.ce_sums)
            E.ensemble_seg_update([v.detach().contiguous() for v in seg_views], flips, lab.contiguous(),
                                  self.ignore_index, probs, cm, ce, False)
            if per_call:
                self.cm += cm
                self.ce_sums += ce
        if depth_views and depth_target is not None:
            for v in depth_views:
                _need_gpu(v, "depth_views")
            B = depth_target.shape[0]
            tg = depth_target.detach().reshape(B, *_hw(depth_target)).float().contiguous()
            mk = None
            if depth_mask is not None:
                mk = depth_mask.reshape(B, *_hw(depth_mask)).to(torch.uint8).contiguous()
            sums = own["depth_sums"] if per_call else self.depth_sums
            E.ensemble_depth_update([v.detach().contiguous() for v in depth_views], flips, tg, mk, self.min_depth,
                                    self.max_depth, self.clamp_pred, self.eps, sums, False)
            if per_call:
                self.depth_sums += sums
        return own

    def all_reduce(self, group=None):
        """Sum the state over the ranks of `group`: one all_reduce per state tensor."""
        import torch.distributed as dist
        for t in (self.cm, self.ce_sums, self.depth_sums):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        """The metrics of everything added so far, with the reference's formulas: `accuracy` =
        correct / (total + 1e-5), `class_iou` = diag / (union + 1e-8), `mean_iou` = nanmean;
        `abs_rel`, `sq_rel`, `rmse`, `rmse_log`, `a1`, `a2`, `a3` pooled over the evaluated pixels (None
        when there are none); `rmse_masked` (the trainer's RMSE on the mask); `loss_seg` (mean CE);
        `loss_silog`; the raw `confusion_matrix`.  Synchronises (three small copies to the host)."""
        return metrics_from_sums(self.cm.cpu().numpy(), self.ce_sums.cpu().numpy(), self.depth_sums.cpu().numpy(),
                                 self.lambd)


def validate(model, batches, evaluator=None, tta=None, **loss_cfg):
    """Evaluate `model` over `batches` of (img, seg, depth, mask) (train.synth_batch's layout) in
    eval mode under no_grad, restore the model's mode, and return `evaluator.compute()`.  Under an
    initialised process group the state is summed over the ranks first.  `tta`: None (one forward
    per batch), or dict(scales=..., flip=..., average=...) (each optional: TTA_SCALES, True,
    'logits') for multi-scale + flip test-time augmentation (`forward_views` + `update_views`).
    `loss_cfg`: Evaluator keywords (lambd, eps, min_depth, ...) for the default evaluator."""
    import torch.distributed as dist
    if tta is not None:
        unknown = set(tta) - {"scales", "flip", "average"}
        if unknown:
            raise ValueError(f"validate: unknown tta keys {sorted(unknown)} (scales, flip, average)")
        scales, flip = tta.get("scales", TTA_SCALES), tta.get("flip", True)
        average = tta.get("average", "logits")
        _probs(average)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for img, seg, depth, mask in batches:
                if evaluator is None:
                    evaluator = Evaluator(device=img.device, **loss_cfg)
                if tta is not None:
                    segs, depths, flips = forward_views(model, img, scales, flip)
                    evaluator.update_views(segs, depths, flips, seg, depth, mask, average=average)
                    continue
                low = model.forward_lowres(img)
                evaluator.update(low["seg"], low["depth"], seg, depth, mask)
    finally:
        model.train(was_training)
    if evaluator is None:
        evaluator = Evaluator(**loss_cfg)
    if dist.is_available() and dist.is_initialized():
        evaluator.all_reduce()
    return evaluator.compute()
