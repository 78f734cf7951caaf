"""SILog depth loss (reference seg/denseclip/losses.py:7-78), the depth loss as a weighted sum of SILog, L1
and BerHu, and the segmentation cross-entropy with class weights, label smoothing and online hard example
mining."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class SILogLoss(nn.Module):
    def __init__(self, lambd=0.5, eps=1e-6, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError(f"Invalid reduction type: {reduction}. Must be 'mean' or 'sum'.")
        self.lambd = lambd
        self.eps = eps
        self.reduction = reduction

    def forward(self, prediction, target, mask=None):
        d = torch.log(torch.clamp(prediction, min=self.eps)) - torch.log(torch.clamp(target, min=self.eps))
        if mask is not None:
            if mask.shape != d.shape:
                if mask.dim() == d.dim() - 1:
                    mask = mask.unsqueeze(1)
                else:
                    raise ValueError(f"Mask shape {mask.shape} incompatible with log_diff shape {d.shape}")
            d = torch.where(mask, d, torch.zeros_like(d))
            T = mask.sum()
        else:
            T = torch.tensor(float(d.numel()), device=d.device)
        # T as a device tensor: no host sync (the reference calls .item() here)
        Tf = T.to(d.dtype).clamp(min=1)
        loss = (d ** 2).sum() / Tf - self.lambd * d.sum() ** 2 / Tf ** 2
        return torch.where(T > 0, loss, torch.zeros_like(loss))


class DepthLoss(nn.Module):
    """The depth loss as a weighted sum of the terms the reference's trainer chooses between
    (configs/denseclip_multitask_cityscapes.yaml:67-70 LOSS_TYPE 'silog', 'berhu' or 'l1' with
    BERHU_THRESHOLD 0.2; train_denseclip.py:1276-1312 "the sum of depth components"):
        silog * SILog(lambd, eps) + l1 * L1 + berhu * BerHu(berhu_threshold)
    on the mask M (every pixel without one), r = prediction - target, e = |r|, T = #M:
        L1    = sum_M e / T
        BerHu = sum_M b(e) / T,  b(e) = e if e <= c, else (e^2 + c^2) / (2 c),  c = berhu_threshold * max_M e
    c is a constant (Laina et al.): it is detached, no gradient flows through the maximum.  It is the
    maximum of THIS call's pixels, hence per rank and per micro-batch under data parallelism or gradient
    accumulation.  An empty mask gives 0.  Weights finite and >= 0, at least one > 0.

    forward(prediction, target, mask) is the materialised formulation on a prediction already at the
    target's size: plain torch, differentiable, no host synchronisation; it runs anywhere.
    fused(pred_lowres, target, mask) is the same loss from the low-res prediction through
    ops.upsample_depth_loss: the resized prediction never exists."""

    def __init__(self, silog=1.0, l1=0.0, berhu=0.0, lambd=0.5, eps=1e-6, berhu_threshold=0.2):
        super().__init__()
        ws = [float(silog), float(l1), float(berhu)]
        if not all(math.isfinite(v) and v >= 0.0 for v in ws) or not any(v > 0.0 for v in ws):
            raise ValueError(f"DepthLoss: weights silog={silog}, l1={l1}, berhu={berhu} "
                             "(finite, >= 0, at least one > 0)")
        if not 0.0 < float(berhu_threshold) <= 1.0:
            raise ValueError(f"DepthLoss: berhu_threshold={berhu_threshold} (0 < berhu_threshold <= 1)")
        self.silog, self.l1, self.berhu = ws
        self.lambd, self.eps = lambd, eps
        self.berhu_threshold = float(berhu_threshold)

    def forward(self, prediction, target, mask=None):
        if mask is not None and mask.shape != prediction.shape:
            if mask.dim() == prediction.dim() - 1:
                mask = mask.unsqueeze(1)
            else:
                raise ValueError(f"Mask shape {mask.shape} incompatible with prediction shape {prediction.shape}")
        if mask is not None and mask.dtype != torch.bool:
            mask = mask != 0  # a mask byte counts as valid when non-zero
        loss = 0.0
        if self.silog > 0:
            loss = self.silog * SILogLoss(self.lambd, self.eps)(prediction, target, mask)
        if self.l1 > 0 or self.berhu > 0:
            r = prediction - target
            if mask is not None:
                r = torch.where(mask, r, torch.zeros_like(r))  # masked-out targets may hold anything
                T = mask.sum()
            else:
                T = torch.tensor(float(r.numel()), device=r.device)
            e = r.abs()
            Tf = T.to(r.dtype).clamp(min=1)
            if self.l1 > 0:
                loss = loss + self.l1 * (e.sum() / Tf)
            if self.berhu > 0:
                # amax keeps a NaN, as the kernels' select does; the masked-out pixels hold e = 0 <= c
                c = self.berhu_threshold * e.detach().amax()
                safe = torch.where(c > 0, c, torch.ones_like(c))
                b = torch.where(e <= c, e, (e * e + c * c) / (2 * safe))
                loss = loss + self.berhu * (b.sum() / Tf)
            loss = torch.where(T > 0, loss, torch.zeros_like(loss))
        return loss

    def fused(self, pred_lowres, target, mask=None):
        from . import ops
        return ops.upsample_depth_loss(pred_lowres, target, mask, silog=self.silog, l1=self.l1, berhu=self.berhu,
                                       lambd=self.lambd, eps=self.eps, berhu_threshold=self.berhu_threshold)


class L1DepthLoss(DepthLoss):
    """mean |prediction - target| on the mask (the reference's LOSS_TYPE 'l1')"""

    def __init__(self):
        super().__init__(silog=0.0, l1=1.0)


class BerHuLoss(DepthLoss):
    """the reverse Huber loss on the mask (the reference's LOSS_TYPE 'berhu', BERHU_THRESHOLD 0.2)"""

    def __init__(self, threshold=0.2):
        super().__init__(silog=0.0, berhu=1.0, berhu_threshold=threshold)


def ohem_keep(p_t, valid, thresh, batch_kept):
    """The keep mask of online hard example mining (mmseg's OHEMPixelSampler rule): with p_t the
    softmax probability of the target at every pixel and `valid` the pixels that have one,
        threshold = max(sorted_ascending(p_t[valid])[min(batch_kept, n_valid - 1)], thresh)
    and a pixel is kept iff it is valid and p_t < threshold.  Everything stays on p_t's device:
    the invalid pixels sort last (+inf) and the index is clamped with the device-side count, so
    there is no host synchronisation.  No valid pixel: nothing is kept."""
    flat = torch.where(valid, p_t, torch.full_like(p_t, float("inf"))).reshape(-1)
    idx = torch.clamp(valid.sum() - 1, min=0, max=int(batch_kept))
    kth = torch.sort(flat).values.gather(0, idx.reshape(1))
    threshold = torch.clamp(kth, min=float(thresh))
    return valid & (p_t < threshold)


class SegCrossEntropy(nn.Module):
    """The segmentation loss with the options people train with: class weights, label smoothing
    and OHEM (ohem = dict(thresh=0.7, min_kept=100000): the loss is averaged over the pixels
    `ohem_keep` keeps, min_kept per image).

    forward(up_logits, labels) is the materialised formulation on logits already at the label
    size: F.cross_entropy with the same arguments, the OHEM rule in torch; it runs anywhere.
    fused(lowres_logits, labels) is the same loss from the low-res logits through
    ops.upsample_cross_entropy: the resized logits never exist."""

    def __init__(self, weight=None, label_smoothing=0.0, ignore_index=255, ohem=None):
        super().__init__()
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"SegCrossEntropy: label_smoothing={label_smoothing} (0 <= label_smoothing < 1)")
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32).clone())
        self.label_smoothing = float(label_smoothing)
        self.ignore_index = int(ignore_index)
        self.ohem = None
        if ohem is not None:
            self.ohem = {"thresh": float(ohem.get("thresh", 0.7)), "min_kept": int(ohem.get("min_kept", 100000))}
            if not 0.0 < self.ohem["thresh"] <= 1.0 or self.ohem["min_kept"] < 0:
                raise ValueError(f"SegCrossEntropy: ohem={ohem} (0 < thresh <= 1, min_kept >= 0)")

    def _weight_on(self, device):
        """the class weights where the logits are; the module itself stays where its owner put it (place it
        with .to(device) beforehand: a copy made here costs a transfer per call and cannot be captured)"""
        w = self.weight
        return w if w is None or w.device == device else w.to(device)

    def _valid(self, labels, K):
        return (labels != self.ignore_index) & (labels >= 0) & (labels < K)

    def forward(self, up_logits, labels):
        w = self._weight_on(up_logits.device)
        labels = labels.long()
        if self.ohem is None:
            return F.cross_entropy(up_logits, labels, weight=w, ignore_index=self.ignore_index,
                                   label_smoothing=self.label_smoothing)
        K = up_logits.shape[1]
        valid = self._valid(labels, K)
        t = torch.where(valid, labels, torch.zeros_like(labels))
        with torch.no_grad():
            x = up_logits.detach()  # selected in the logits' own precision, fp32 at the least
            x = x.float() if x.dtype in (torch.float16, torch.bfloat16) else x
            p_t = F.softmax(x, dim=1).gather(1, t[:, None]).squeeze(1)
            keep = ohem_keep(p_t, valid, self.ohem["thresh"], self.ohem["min_kept"] * labels.shape[0])
        l = F.cross_entropy(up_logits, labels, weight=w, ignore_index=self.ignore_index,
                            label_smoothing=self.label_smoothing, reduction="none")
        q = keep.to(l.dtype)
        w_t = q if w is None else q * w.to(l.dtype)[t]
        return (l * q).sum() / w_t.sum()

    def fused(self, lowres_logits, labels):
        from . import ops
        w = self._weight_on(lowres_logits.device)
        if self.ohem is None:
            return ops.upsample_cross_entropy(lowres_logits, labels, self.ignore_index, w, self.label_smoothing)
        with torch.no_grad():  # the selection: the plain per-pixel loss, forward only
            nll = ops.upsample_cross_entropy(lowres_logits.detach(), labels, self.ignore_index, reduction="none")
            keep = ohem_keep(torch.exp(-nll), self._valid(labels, lowres_logits.shape[1]), self.ohem["thresh"],
                             self.ohem["min_kept"] * labels.shape[0])
        return ops.upsample_cross_entropy(lowres_logits, labels, self.ignore_index, w, self.label_smoothing,
                                          pixel_weight=keep.to(torch.float32))
