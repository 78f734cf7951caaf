"""On-device validation: class maps, mIoU / pixel accuracy, depth errors and the validation losses,
from the heads' low-res outputs, without materialising the resized (B, K, H, W) logits.

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

Sliding-window inference (test_cfg mode='slide' of the reference's ViT configs, mmseg's
slide_inference) likewise: `forward_windows` runs the model on the overlapping crops of
`slide_windows` and keeps their low-res maps, and `predict_slide` / `Evaluator.update_windows` /
`validate(..., slide=dict(crop_size=..., stride=...))` hand them to one fused kernel per head
(csrc/headslide.hip) that averages, per pixel, the windows that cover it.

The two combine as in mmseg's aug_test over slide_inference, the evaluation the reference's ViT
configs run under --aug-test: `forward_view_windows` runs the windows of every scaled / mirrored view
(`view_windows`), and `predict_slide_tta` / `Evaluator.update_view_windows` /
`validate(..., slide_tta=dict(crop_size=..., stride=...))` hand all of them to one fused kernel per
head (csrc/headslidetta.hip): per output pixel and view, up to four taps of the view's slide result,
each the mean of its covering windows, with no per-view tensor.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _torch_ops
from ._native import CLASSES_MAX, ENSEMBLE_MAX_VIEWS, SLIDE_MAX_WINDOWS, SLIDE_TTA_MAX_WINDOWS

DEPTH_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
TTA_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)  # the reference's --aug-test ratios (test.py:93-96)
AVERAGES = ("logits", "probs")
_LAB_DTYPES = (torch.int64, torch.int32, torch.uint8)
CITYSCAPES_K = 19  # the class count of the register-resident kernels; any other K <= CLASSES_MAX is chunked


def _check_classes(K, what):
    """True when K takes the chunked kernels (csrc/classes.hip), False for the 19-class ones"""
    K = int(K)
    if K < 1 or K > CLASSES_MAX:
        raise ValueError(f"{what}: {K} classes (the fused evaluation takes 1 to {CLASSES_MAX})")
    return K != CITYSCAPES_K


def _only_cityscapes(K, what):
    """the ensemble / sliding-window kernels are built for 19 classes"""
    if K is not None and int(K) != CITYSCAPES_K:
        raise NotImplementedError(f"{what}: {int(K)} classes: the multi-scale / flip and sliding-window evaluation "
                                  f"kernels are built for {CITYSCAPES_K} classes; only the plain path (predict, "
                                  "Evaluator.update, validate without tta / slide) takes another class count")


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
    if _check_classes(logits.shape[1], "upsample_argmax"):
        return _E().upsample_argmax_classes(logits.detach().contiguous(), int(size[0]), int(size[1]))
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
    _only_cityscapes(getattr(model, "num_classes", None), "predict_tta")
    H, W = _hw(img) if size is None else (int(size[0]), int(size[1]))
    segs, depths, flips = forward_views(model, img, scales, flip)
    _only_cityscapes(segs[0].shape[1] if segs else None, "predict_tta")
    E = _E()
    return {"seg": E.ensemble_argmax(segs, flips, H, W, probs) if segs else None,
            "depth": E.ensemble_depth(depths, flips, H, W) if depths else None}


def _pair(v, what):
    """(a, b) of positive ints from an int or a pair"""
    try:
        a, b = (v, v) if isinstance(v, int) else v
        a, b = int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError(f"slide: {what}={v!r}: a positive int or a pair of them") from None
    if a <= 0 or b <= 0:
        raise ValueError(f"slide: {what}={v!r} must be positive")
    return a, b


def slide_windows(H, W, crop_size, stride):
    """The windows of mmseg's slide_inference on an H x W image: ((wh, ww), [(y0, x0), ...]), row by
    row.  With crop_size (ch, cw) and stride (sh, sw) (ints or pairs) there are
    max(H - ch + sh - 1, 0) // sh + 1 rows of windows (columns likewise); window (i, j) ends at
    y2 = min(i sh + ch, H) and starts at max(y2 - ch, 0), so every window is min(ch, H) x min(cw, W)
    and the last of a row or column is shifted back, not shrunk."""
    return _slide_grid(H, W, crop_size, stride, SLIDE_MAX_WINDOWS)


def _slide_grid(H, W, crop_size, stride, limit):
    """`slide_windows` with the table's limit as an argument"""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"slide: image size {H} x {W} must be positive")
    (ch, cw), (sh, sw) = _pair(crop_size, "crop_size"), _pair(stride, "stride")
    h_grids = max(H - ch + sh - 1, 0) // sh + 1
    w_grids = max(W - cw + sw - 1, 0) // sw + 1
    if h_grids * w_grids > limit:
        raise ValueError(f"slide: {h_grids} x {w_grids} = {h_grids * w_grids} windows on a {H} x {W} image with "
                         f"crop_size={(ch, cw)}, stride={(sh, sw)} (at most {limit})")
    origins = []
    for i in range(h_grids):
        for j in range(w_grids):
            y2, x2 = min(i * sh + ch, H), min(j * sw + cw, W)
            origins.append((max(y2 - ch, 0), max(x2 - cw, 0)))
    return (min(ch, H), min(cw, W)), origins


def slide_from_test_cfg(test_cfg):
    """validate's `slide` keywords from a model's test_cfg: dict(crop_size=..., stride=...) for
    dict(mode='slide', crop_size=..., stride=...) (the reference's ViT configs), None for any other mode
    ('whole', or no test_cfg)."""
    if not isinstance(test_cfg, dict) or test_cfg.get("mode") != "slide":
        return None
    if "crop_size" not in test_cfg or "stride" not in test_cfg:
        raise ValueError(f"test_cfg={test_cfg!r}: mode='slide' needs crop_size and stride")
    return {"crop_size": test_cfg["crop_size"], "stride": test_cfg["stride"]}


def forward_windows(model, img, crop_size, stride, windows_per_forward=None):
    """`model.forward_lowres` on every window of `slide_windows` under no_grad, keeping only the
    low-res maps: (seg_lows, depth_lows, (wh, ww), origins), a list of (B, K, h, w) / (B, 1, h, w)
    maps per head (None for a model without that head) in the order of `origins`.  One window (all B
    images) per forward by default; `windows_per_forward` = n runs n windows concatenated along the
    batch."""
    H, W = _hw(img)
    (wh, ww), origins = slide_windows(H, W, crop_size, stride)
    segs, depths = _forward_crops(model, img, (wh, ww), origins, windows_per_forward)
    return segs or None, depths or None, (wh, ww), origins


def _forward_crops(model, img, size, origins, windows_per_forward):
    """the low-res maps (seg list, depth list) of `model` on the crops of `img` of `size` at `origins`"""
    wh, ww = size
    n = 1 if windows_per_forward is None else int(windows_per_forward)
    if n <= 0:
        raise ValueError(f"slide: windows_per_forward={windows_per_forward!r} must be positive")
    B = img.shape[0]
    segs, depths = [], []
    with torch.no_grad():
        for i in range(0, len(origins), n):
            crops = [img[:, :, y0:y0 + wh, x0:x0 + ww] for y0, x0 in origins[i:i + n]]
            low = model.forward_lowres(crops[0].contiguous() if len(crops) == 1 else torch.cat(crops, 0))
            for head, out in ((low["seg"], segs), (low["depth"], depths)):
                if head is not None:
                    out.extend(c.contiguous() for c in head.detach().split(B, 0))
    return segs, depths


def _flat(origins):
    return [int(c) for o in origins for c in o]


def predict_slide(model, img, crop_size, stride, windows_per_forward=None):
    """`predict` under sliding-window inference (mmseg's test_cfg mode='slide'): {'seg': uint8
    (B, H, W), 'depth': fp32 (B, 1, H, W)} from the mean, over the windows that cover a pixel, of the
    windows' outputs resized to the window size (csrc/headslide.hip: no image-sized accumulator)."""
    _only_cityscapes(getattr(model, "num_classes", None), "predict_slide")
    H, W = _hw(img)
    segs, depths, (wh, ww), origins = forward_windows(model, img, crop_size, stride, windows_per_forward)
    _only_cityscapes(segs[0].shape[1] if segs else None, "predict_slide")
    E = _E()
    return {"seg": E.slide_argmax(segs, _flat(origins), wh, ww, H, W) if segs else None,
            "depth": E.slide_depth(depths, _flat(origins), wh, ww, H, W) if depths else None}


def view_windows(H, W, crop_size, stride, scales=TTA_SCALES, flip=True):
    """The windows of every view of mmseg's aug_test over slide_inference on an H x W image: a list,
    in `tta_views` order, of (Hv, Wv, flipped, (wh, ww), origins) with (Hv, Wv) = (int(H s + 0.5),
    int(W s + 0.5)) and `slide_windows(Hv, Wv, crop_size, stride)` in the view's own coordinates (a
    mirrored view has the windows of the plain one: they are cut from the mirrored image).  At most
    ENSEMBLE_MAX_VIEWS views and SLIDE_TTA_MAX_WINDOWS windows in all."""
    H, W = int(H), int(W)
    out = []
    for s in scales:
        Hv, Wv = int(H * s + 0.5), int(W * s + 0.5)
        size, origins = _slide_grid(Hv, Wv, crop_size, stride, SLIDE_TTA_MAX_WINDOWS)
        out.append((Hv, Wv, False, size, list(origins)))
        if flip:
            out.append((Hv, Wv, True, size, list(origins)))
    total = sum(len(v[4]) for v in out)
    if not out or len(out) > ENSEMBLE_MAX_VIEWS:
        raise ValueError(f"slide_tta: {len(out)} views (1 .. {ENSEMBLE_MAX_VIEWS})")
    if total > SLIDE_TTA_MAX_WINDOWS:
        raise ValueError(f"slide_tta: {total} windows over {len(out)} views of a {H} x {W} image with "
                         f"crop_size={crop_size!r}, stride={stride!r} (at most {SLIDE_TTA_MAX_WINDOWS})")
    return out


def forward_view_windows(model, img, crop_size, stride, scales=TTA_SCALES, flip=True, windows_per_forward=None):
    """`model.forward_lowres` on every window (`view_windows`) of every view (`tta_views`) of `img` under
    no_grad, one view's image at a time, keeping only the low-res maps: (seg_lows, depth_lows, views,
    origins) with one list of (B, K, h_v, w_v) / (B, 1, h_v, w_v) maps per head over all views in view
    order (None for a model without that head), views = [(Hv, Wv, flipped, wh, ww, nwin), ...] and
    origins = [(y0, x0), ...] per window in its view's coordinates."""
    H, W = _hw(img)
    table = view_windows(H, W, crop_size, stride, scales, flip)
    segs, depths, views, origins = [], [], [], []
    for (view, flipped), (Hv, Wv, fl, size, orig) in zip(tta_views(img, scales, flip), table):
        assert _hw(view) == (Hv, Wv) and flipped == fl
        s, d = _forward_crops(model, view, size, orig, windows_per_forward)
        segs.extend(s)
        depths.extend(d)
        views.append((Hv, Wv, int(flipped), size[0], size[1], len(orig)))
        origins.extend(orig)
    return segs or None, depths or None, views, origins


def predict_slide_tta(model, img, crop_size, stride, scales=TTA_SCALES, flip=True, average="probs",
                      windows_per_forward=None):
    """`predict` under multi-scale + flip test-time augmentation with every view evaluated by sliding
    windows (mmseg's aug_test over slide_inference): {'seg': uint8 (B, H, W), 'depth': fp32
    (B, 1, H, W)} from the mean over the views of their slide results resized to the image and
    mirrored back (csrc/headslidetta.hip: no per-view tensor).  `average`: 'probs' (mmseg's rule) or
    'logits' for the class map; the depth is always the mean of the predictions."""
    probs = _probs(average)
    _only_cityscapes(getattr(model, "num_classes", None), "predict_slide_tta")
    H, W = _hw(img)
    segs, depths, views, origins = forward_view_windows(model, img, crop_size, stride, scales, flip,
                                                        windows_per_forward)
    _only_cityscapes(segs[0].shape[1] if segs else None, "predict_slide_tta")
    E = _E()
    return {"seg": E.slide_tta_argmax(segs, _flat(views), _flat(origins), H, W, probs) if segs else None,
            "depth": E.slide_tta_depth(depths, _flat(views), _flat(origins), H, W) if depths else None}


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
        self.chunked = _check_classes(self.num_classes, "Evaluator")  # K != 19: csrc/classes.hip
        self._seg_ws = {}  # the chunked kernel's workspace per (device, bytes): allocated once, reused by every update
        self.min_depth, self.max_depth, self.clamp_pred = float(min_depth), float(max_depth), bool(clamp_pred)
        self.lambd, self.eps = float(lambd), float(eps)
        self.device = torch.device(device)
        self.cm = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=self.device)
        self.ce_sums = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.depth_sums = torch.zeros(12, dtype=torch.float64, device=self.device)

    def reset(self):
        for t in (self.cm, self.ce_sums, self.depth_sums):
            t.zero_()

    def _own(self, per_call):
        """the call's own zeroed sums (per_call=True), or None: the fused ops add to the running state"""
        if not per_call:
            return None
        return {"cm": torch.zeros_like(self.cm), "ce_sums": torch.zeros_like(self.ce_sums),
                "depth_sums": torch.zeros_like(self.depth_sums)}

    def _add_back(self, own, *keys):
        """the call's own sums into the running state"""
        if own is not None:
            for k in keys:
                getattr(self, k).add_(own[k])

    def _seg_args(self, maps, what, seg_target, own):
        """(contiguous low-res maps, labels (B, H, W) in a dtype the kernels read, cm, ce_sums)"""
        for v in maps:
            _need_gpu(v, what)
            if v.shape[1] != self.num_classes:
                raise ValueError(f"Evaluator: {v.shape[1]} classes, built for {self.num_classes}")
        lab = seg_target.reshape(seg_target.shape[0], *_hw(seg_target))
        if lab.dtype not in _LAB_DTYPES:
            lab = lab.long()
        cm, ce = (self.cm, self.ce_sums) if own is None else (own["cm"], own["ce_sums"])
        return [v.detach().contiguous() for v in maps], lab.contiguous(), cm, ce

    def _depth_args(self, maps, what, depth_target, depth_mask, own):
        """(contiguous low-res maps, target (B, H, W) fp32, mask (B, H, W) uint8 or None, sums)"""
        for v in maps:
            _need_gpu(v, what)
        B = depth_target.shape[0]
        tg = depth_target.detach().reshape(B, *_hw(depth_target)).float().contiguous()
        mk = None
        if depth_mask is not None:
            mk = depth_mask.reshape(B, *_hw(depth_mask)).to(torch.uint8).contiguous()
        return [v.detach().contiguous() for v in maps], tg, mk, self.depth_sums if own is None else own["depth_sums"]

    def _classes_ws(self, low):
        """the chunked kernel's scratch for maps of this shape, sized by dclip_upsample_eval_seg_classes_ws_bytes"""
        n = int(_E().seg_classes_ws_bytes(int(low.shape[0]), self.num_classes, int(low.shape[2]), int(low.shape[3])))
        key = (low.device, n)  # images of many sizes (ADE20K's) share one buffer as long as the size agrees
        ws = self._seg_ws.get(key)
        if ws is None:
            ws = self._seg_ws[key] = torch.empty(n, dtype=torch.uint8, device=low.device)
        return ws

    def update(self, seg_lowres=None, depth_lowres=None, seg_target=None, depth_target=None, depth_mask=None,
               per_call=False):
        """Add one batch: `seg_lowres` (B, K, h, w) with `seg_target` (B, H, W) int64 / int32 / uint8,
        `depth_lowres` (B, 1, h, w) with `depth_target` (B, [1,] H, W) and `depth_mask` (same shape,
        bool / uint8, None = all valid).  Returns None, or with per_call=True the call's own
        {'cm', 'ce_sums', 'depth_sums'} (device tensors, also added to the running state)."""
        E = _E()
        own = self._own(per_call)
        if seg_lowres is not None and seg_target is not None:
            (low,), lab, cm, ce = self._seg_args([seg_lowres], "seg_lowres", seg_target, own)
            if self.chunked:
                E.seg_update_classes(low, lab, self.ignore_index, cm, ce, False, self._classes_ws(low))
            else:
                E.seg_update(low, lab, self.ignore_index, cm, ce, False)
            self._add_back(own, "cm", "ce_sums")
        if depth_lowres is not None and depth_target is not None:
            (low,), tg, mk, sums = self._depth_args([depth_lowres], "depth_lowres", depth_target, depth_mask, own)
            E.depth_update(low, tg, mk, self.min_depth, self.max_depth, self.clamp_pred, self.eps, sums, False)
            self._add_back(own, "depth_sums")
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
        _only_cityscapes(self.num_classes, "Evaluator.update_views")
        E = _E()
        flips = [int(f) for f in flips]
        own = self._own(per_call)
        if seg_views and seg_target is not None:
            lows, lab, cm, ce = self._seg_args(seg_views, "seg_views", seg_target, own)
            E.ensemble_seg_update(lows, flips, lab, self.ignore_index, probs, cm, ce, False)
            self._add_back(own, "cm", "ce_sums")
        if depth_views and depth_target is not None:
            lows, tg, mk, sums = self._depth_args(depth_views, "depth_views", depth_target, depth_mask, own)
            E.ensemble_depth_update(lows, flips, tg, mk, self.min_depth, self.max_depth, self.clamp_pred, self.eps,
                                    sums, False)
            self._add_back(own, "depth_sums")
        return own

    def update_windows(self, seg_lows=None, depth_lows=None, window_size=None, origins=(), seg_target=None,
                       depth_target=None, depth_mask=None, per_call=False):
        """`update` on one batch's sliding windows (`forward_windows`): lists of low-res maps
        (B, K, h, w) / (B, 1, h, w), the windows' size (wh, ww) at the image's resolution and their
        origins [(y0, x0), ...]; the metrics are taken from the mean, over the windows that cover a
        pixel, of the windows' outputs resized to (wh, ww).  Same contract as `update`: no host
        synchronisation, no new tensor besides the workspace, added to the running state;
        per_call=True returns the call's own sums."""
        _only_cityscapes(self.num_classes, "Evaluator.update_windows")
        E = _E()
        wh, ww = int(window_size[0]), int(window_size[1])
        flat = _flat(origins)
        own = self._own(per_call)
        if seg_lows and seg_target is not None:
            lows, lab, cm, ce = self._seg_args(seg_lows, "seg_lows", seg_target, own)
            E.slide_seg_update(lows, flat, wh, ww, lab, self.ignore_index, cm, ce, False)
            self._add_back(own, "cm", "ce_sums")
        if depth_lows and depth_target is not None:
            lows, tg, mk, sums = self._depth_args(depth_lows, "depth_lows", depth_target, depth_mask, own)
            E.slide_depth_update(lows, flat, wh, ww, tg, mk, self.min_depth, self.max_depth, self.clamp_pred,
                                 self.eps, sums, False)
            self._add_back(own, "depth_sums")
        return own

    def update_view_windows(self, seg_lows=None, depth_lows=None, views=(), origins=(), seg_target=None,
                            depth_target=None, depth_mask=None, average="probs", per_call=False):
        """`update` on one batch's windows of every view (`forward_view_windows`): lists of low-res maps
        over all views in view order, views = [(Hv, Wv, flipped, wh, ww, nwin), ...] and the windows'
        origins [(y0, x0), ...] in their view's coordinates; the metrics are taken from the mean over
        the views of their slide results resized to the target's size and mirrored back (`average`:
        'probs' or 'logits' for the class map and the CE).  Same contract as `update`: no host
        synchronisation, no new tensor besides the workspace, added to the running state;
        per_call=True returns the call's own sums."""
        probs = _probs(average)
        _only_cityscapes(self.num_classes, "Evaluator.update_view_windows")
        E = _E()
        vflat, oflat = _flat(views), _flat(origins)
        own = self._own(per_call)
        if seg_lows and seg_target is not None:
            lows, lab, cm, ce = self._seg_args(seg_lows, "seg_lows", seg_target, own)
            E.slide_tta_seg_update(lows, vflat, oflat, lab, self.ignore_index, probs, cm, ce, False)
            self._add_back(own, "cm", "ce_sums")
        if depth_lows and depth_target is not None:
            lows, tg, mk, sums = self._depth_args(depth_lows, "depth_lows", depth_target, depth_mask, own)
            E.slide_tta_depth_update(lows, vflat, oflat, tg, mk, self.min_depth, self.max_depth, self.clamp_pred,
                                     self.eps, sums, False)
            self._add_back(own, "depth_sums")
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


_SLIDE_TTA_KEYS = ("crop_size", "stride", "scales", "flip", "average", "windows_per_forward")


def validate(model, batches, evaluator=None, tta=None, slide=None, slide_tta=None, **loss_cfg):
    """Evaluate `model` over `batches` of (img, seg, depth, mask) (train.synth_batch's layout) in
    eval mode under no_grad, restore the model's mode, and return `evaluator.compute()`.  Under an
    initialised process group the state is summed over the ranks first.  `tta`: None (one forward
    per batch), or dict(scales=..., flip=..., average=...) (each optional: TTA_SCALES, True,
    'logits') for multi-scale + flip test-time augmentation (`forward_views` + `update_views`).
    `slide`: None, dict(crop_size=..., stride=...[, windows_per_forward=...]) for sliding-window
    inference (`forward_windows` + `update_windows`), or True to take crop_size and stride from
    `model.test_cfg` (which must then be dict(mode='slide', crop_size=..., stride=...)); `slide` and
    `tta` do not combine: `slide_tta` is their combination, mmseg's aug_test over slide_inference
    (`forward_view_windows` + `update_view_windows`): dict(crop_size=..., stride=...[, scales=...,
    flip=..., average=..., windows_per_forward=...]) (TTA_SCALES, True, 'probs'), or True to take
    crop_size and stride from `model.test_cfg`; it excludes both `slide` and `tta`.  `loss_cfg`: Evaluator keywords (lambd, eps, min_depth, ...) for the default
    evaluator."""
    import torch.distributed as dist
    if slide_tta is not None and slide_tta is not False:
        if tta is not None or (slide is not None and slide is not False):
            raise ValueError("validate: slide_tta is sliding windows over multi-scale + flip views by itself; it does "
                             "not combine with slide or tta")
        if slide_tta is True:
            slide_tta = slide_from_test_cfg(getattr(model, "test_cfg", None))
            if slide_tta is None:
                raise ValueError(f"validate: slide_tta=True needs model.test_cfg = dict(mode='slide', crop_size=..., "
                                 f"stride=...), got {getattr(model, 'test_cfg', None)!r}")
        unknown = set(slide_tta) - set(_SLIDE_TTA_KEYS)
        if unknown:
            raise ValueError(f"validate: unknown slide_tta keys {sorted(unknown)} ({', '.join(_SLIDE_TTA_KEYS)})")
        if "crop_size" not in slide_tta or "stride" not in slide_tta:
            raise ValueError("validate: slide_tta needs crop_size and stride")
        _pair(slide_tta["crop_size"], "crop_size"), _pair(slide_tta["stride"], "stride")
        slide_tta = dict(slide_tta)
        st_average = slide_tta.pop("average", "probs")
        _probs(st_average)
    else:
        slide_tta = None
    if tta is not None:
        unknown = set(tta) - {"scales", "flip", "average"}
        if unknown:
            raise ValueError(f"validate: unknown tta keys {sorted(unknown)} (scales, flip, average)")
        scales, flip = tta.get("scales", TTA_SCALES), tta.get("flip", True)
        average = tta.get("average", "logits")
        _probs(average)
    if slide is not None and slide is not False:
        if tta is not None:
            raise ValueError("validate: slide and tta do not combine (sliding windows over multi-scale + flip views "
                             "are validate(slide_tta=dict(crop_size=..., stride=..., ...)))")
        if slide is True:
            slide = slide_from_test_cfg(getattr(model, "test_cfg", None))
            if slide is None:
                raise ValueError(f"validate: slide=True needs model.test_cfg = dict(mode='slide', crop_size=..., "
                                 f"stride=...), got {getattr(model, 'test_cfg', None)!r}")
        unknown = set(slide) - {"crop_size", "stride", "windows_per_forward"}
        if unknown:
            raise ValueError(f"validate: unknown slide keys {sorted(unknown)} (crop_size, stride, "
                             "windows_per_forward)")
        if "crop_size" not in slide or "stride" not in slide:
            raise ValueError("validate: slide needs crop_size and stride")
        _pair(slide["crop_size"], "crop_size"), _pair(slide["stride"], "stride")
    else:
        slide = None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for img, seg, depth, mask in batches:
                if evaluator is None:
                    if "num_classes" not in loss_cfg and getattr(model, "num_classes", None):
                        loss_cfg["num_classes"] = int(model.num_classes)
                    evaluator = Evaluator(device=img.device, **loss_cfg)
                if slide_tta is not None:
                    segs, depths, views, origins = forward_view_windows(model, img, **slide_tta)
                    evaluator.update_view_windows(segs, depths, views, origins, seg, depth, mask, average=st_average)
                    continue
                if tta is not None:
                    segs, depths, flips = forward_views(model, img, scales, flip)
                    evaluator.update_views(segs, depths, flips, seg, depth, mask, average=average)
                    continue
                if slide is not None:
                    segs, depths, size, origins = forward_windows(model, img, **slide)
                    evaluator.update_windows(segs, depths, size, origins, seg, depth, mask)
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
