"""Shared inputs and CPU references of the sliding-windows-under-TTA tests (test_slide_tta_cpu.py,
test_gpu_slide_tta.py): the cases (image, crop, stride, views, patch size of the low-res maps), the
windows of every view by slide_ref's restated rule, seeded low-res maps per window (a low-frequency
scene shared by all views plus noise, so that the views agree as real ones do), the fp64 reference
(per view slide_ref.slide, eval_ref.resize to the image unless the view has its size, .flip(-1) for a
flipped view, softmax under 'probs', then the mean), the ambiguity threshold, and the measurement of
the reference's own fp32 departure (`python tests/slide_tta_ref.py` prints the table
test_gpu_slide_tta.py holds as REF_FP32_DEPARTURE, taken with torch's scalar CPU kernels so that
every machine prints the same figures).  Labels, targets and masks are eval_ref's."""
import functools
import math

import torch

import eval_ref as R
import slide_ref as S
from tta_ref import AMBIGUOUS_CAP, LAB_OF_LOW, LOWS, RULES, ce_sum, check_class_map, mask_of  # noqa: F401

K = R.K
# name -> (B, H, W, crop_size, stride, [(Hv, Wv, flip), ...], p); a window's low-res map is
# (ceil(wh / p), ceil(ww / p))
CASES = {
    # the reference geometry (1024 x 2048, crop 640, stride 426, ratios 0.5 / 1 / 1.75) at 1/16: a view
    # smaller than the crop, the identity view, a downscaled view; 4 + 20 + 64 windows
    "city16": (1, 64, 128, (40, 40), (27, 27), [(hv, 2 * hv, f) for hv in (32, 64, 112) for f in (0, 1)], 8),
    # odd origins, W % 4 != 0, non-integer ratios both ways
    "odd": (2, 43, 301, (20, 131), (13, 87), [(43, 301, 0), (32, 226, 1), (54, 376, 0), (54, 376, 1)], 4),
    # x1.75 downscale over pixels covered by up to 4 windows
    "down_dense": (1, 24, 40, (16, 16), (8, 8), [(42, 70, 0), (42, 70, 1)], 4),
    # no resize, no overlap
    "identity_pair": (1, 32, 64, (16, 32), (16, 32), [(32, 64, 0), (32, 64, 1)], 4),
    # one window per view, x2 upscale after the slide
    "small_views": (1, 40, 100, (32, 64), (21, 42), [(20, 50, 0), (20, 50, 1)], 4),
    # W past a 128-column tile, window edges inside tiles
    "two_tiles": (2, 24, 528, (24, 300), (24, 228), [(24, 528, 0), (18, 396, 1)], 8),
    # 440 windows: the device table written in several chunks
    "many": (1, 16, 32, (8, 8), (5, 5), [(28, 56, i % 2) for i in range(8)], 2),
}
N_WINDOWS = {"city16": 88, "odd": 47, "down_dense": 80, "identity_pair": 8, "small_views": 2, "two_tiles": 4,
             "many": 440}
# (case, low dtype, mask kind, clamp) of the depth test
DEPTH_CASES = [(c, low, "mask", 1) for c in ("city16", "odd", "down_dense") for low in LOWS] + \
              [(c, torch.float32, m, k) for c in ("city16", "odd", "down_dense")
               for m, k in (("mask", 0), ("none", 0), ("none", 1))]


def geometry(case):
    """(B, H, W, views) of a case; views = [(Hv, Wv, flip, (wh, ww), origins, (h, w)), ...]"""
    B, H, W, crop, stride, vs, p = CASES[case]
    views = []
    for Hv, Wv, flip in vs:
        (wh, ww), origins = S.windows(Hv, Wv, crop, stride)
        views.append((Hv, Wv, flip, (wh, ww), origins, (-(-wh // p), -(-ww // p))))
    return B, H, W, views


@functools.lru_cache(maxsize=None)
def _scene(B):
    gen = torch.Generator().manual_seed(99)
    a = 3 * torch.rand(K, generator=gen, dtype=torch.float64)
    b = 5 * torch.rand(K, generator=gen, dtype=torch.float64)
    ph = torch.rand(B, K, generator=gen, dtype=torch.float64)
    return a, b, ph


@functools.lru_cache(maxsize=None)
def seg_low(case, vi, g, dtype=torch.float32):
    """window g of view vi: the scene at the window's low-res pixel centres (in the un-mirrored image's
    normalised coordinates) plus unit noise"""
    B, H, W, views = geometry(case)
    Hv, Wv, flip, (wh, ww), origins, (h, w) = views[vi]
    y0, x0 = origins[g]
    a, b, ph = _scene(B)
    ny = (y0 + (torch.arange(h, dtype=torch.float64) + 0.5) * wh / h) / Hv
    nx = (x0 + (torch.arange(w, dtype=torch.float64) + 0.5) * ww / w) / Wv
    if flip:
        nx = 1 - nx
    arg = a.view(1, K, 1, 1) * ny.view(1, 1, h, 1) + b.view(1, K, 1, 1) * nx.view(1, 1, 1, w) + ph.view(B, K, 1, 1)
    gen = torch.Generator().manual_seed(6000 + 100 * vi + g)
    return ((4 * torch.cos(2 * math.pi * arg)).float() + torch.randn(B, K, h, w, generator=gen)).to(dtype)


@functools.lru_cache(maxsize=None)
def depth_low(case, vi, g, dtype=torch.float32):
    B, H, W, views = geometry(case)
    h, w = views[vi][5]
    gen = torch.Generator().manual_seed(7000 + 100 * vi + g)
    return (0.5 + 59.5 * torch.rand(B, 1, h, w, generator=gen)).to(dtype)


def seg_lows(case, low):
    """per view, the list of its windows' maps"""
    return [[seg_low(case, vi, g, low) for g in range(len(v[4]))] for vi, v in enumerate(geometry(case)[3])]


def depth_lows(case, low):
    return [[depth_low(case, vi, g, low) for g in range(len(v[4]))] for vi, v in enumerate(geometry(case)[3])]


def slide_tta(maps, views, H, W, probs=False, dtype=torch.float64, view_order=None, window_order=None):
    """(mean, [S_v], [cmax_v]): per view (in `view_order`) slide_ref.slide of its windows (in
    `window_order(vi)`), the resize to H x W unless the view has that size, .flip(-1) for a flipped
    view, softmax over dim 1 under 'probs', then the mean; in `dtype` throughout"""
    outs, slides, cmax = [], [], []
    for vi in (range(len(views)) if view_order is None else view_order):
        Hv, Wv, flip, size, origins, hw = views[vi]
        s, cnt = S.slide(maps[vi], origins, size, Hv, Wv, dtype=dtype,
                         order=None if window_order is None else window_order(vi))
        slides.append(s)
        cmax.append(int(cnt.max()))
        u = s if (Hv, Wv) == (H, W) else R.resize(s, H, W, dtype)
        if flip:
            u = u.flip(-1)
        outs.append(torch.softmax(u, dim=1) if probs else u)
    return torch.stack(outs).mean(0), slides, cmax


def tau_of(maps, views, slides, cmax, mean, rule, H, W):
    """Per view slide_ref.tau_of, plus for a resized view the second stage's fp32 summation order and
    source-coordinate rounding on a map whose slope per view pixel is 1 / p_v of the low-res map's
    (eval_ref.tau's form at Hv / p_v[0] + Wv / p_v[1]); then tta_ref.tau_of's rule over the views."""
    t = 0.0
    for m, (Hv, Wv, flip, (wh, ww), origins, (h, w)), s, c in zip(maps, views, slides, cmax):
        tv = S.tau_of(m, (h, w), s, c)
        if (Hv, Wv) != (H, W):
            tv += 2.0 ** -24 * float(s.abs().max()) * (32 + 8 * (Hv / (wh / h) + Wv / (ww / w)))
        t += tv
    t /= len(views)
    if rule == "probs":
        return t / 4 + 2.0 ** -20
    return t + 2.0 ** -24 * (len(views) + 1) * float(mean.abs().max())


def reference(maps, views, H, W, rule):
    """(mean fp64, tau) of any maps / views"""
    mean, slides, cmax = slide_tta(maps, views, H, W, probs=rule == "probs")
    return mean, tau_of(maps, views, slides, cmax, mean, rule, H, W)


@functools.lru_cache(maxsize=None)
def seg_reference(case, low, rule):
    B, H, W, views = geometry(case)
    return reference(seg_lows(case, low), views, H, W, rule)


@functools.lru_cache(maxsize=None)
def depth_reference(case, low):
    B, H, W, views = geometry(case)
    return reference(depth_lows(case, low), views, H, W, "logits")


def measure_fp32_departure():
    """The largest relative departure, over the inputs the GPU tests use, of the reference's own fp32
    path (the same torch sequence in fp32) from its fp64 evaluation: the CE sum under each rule and
    every floating depth sum.  Also the ambiguous share per case and rule, the worst fp32-vs-fp64
    distance of the mean in units of tau and the unambiguous pixels on which the fp32 argmax differs."""
    dep = {"ce_logits": 0.0, "ce_probs": 0.0}
    amb, dist, wrong = {}, 0.0, 0
    for case in CASES:
        B, H, W, views = geometry(case)
        for low in LOWS:
            lab = R.labels(B, H, W, LAB_OF_LOW[low])
            for rule in RULES:
                u64, tau = seg_reference(case, low, rule)
                u32 = slide_tta(seg_lows(case, low), views, H, W, probs=rule == "probs", dtype=torch.float32)[0]
                dep["ce_" + rule] = max(dep["ce_" + rule], R.rel(ce_sum(u32, lab, rule), ce_sum(u64, lab, rule)))
                top = u64.topk(2, dim=1).values
                a = (top[:, 0] - top[:, 1]) < tau
                amb[case, rule] = max(amb.get((case, rule), 0.0), float(a.float().mean()))
                dist = max(dist, float((u32.double() - u64).abs().max()) / tau)
                wrong += int(((u32.argmax(1) != u64.argmax(1)) & ~a).sum())
    for case, low, kind, clamp in DEPTH_CASES:
        B, H, W, views = geometry(case)
        u64, _ = depth_reference(case, low)
        u32 = slide_tta(depth_lows(case, low), views, H, W, dtype=torch.float32)[0]
        gt, mask = R.depth_target(B, H, W), mask_of(kind, B, H, W)
        s64, s32 = R.depth_sums(u64, gt, mask, clamp=bool(clamp)), R.depth_sums(u32, gt, mask, clamp=bool(clamp))
        for i in R.FLOAT_SUMS:
            n = R.SUM_NAMES[i]
            dep[n] = max(dep.get(n, 0.0), R.rel(s32[i], s64[i]))
    return dep, amb, dist, wrong


if __name__ == "__main__":
    import os
    import subprocess
    import sys
    # torch's vectorised CPU kernels round differently per instruction set; the table is taken with the
    # scalar kernels, which give every CPU the same figures (as slide_ref.py does)
    if os.environ.get("ATEN_CPU_CAPABILITY") != "default":
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)],
                                 env=dict(os.environ, ATEN_CPU_CAPABILITY="default")))
    print("CPU capability:", torch.backends.cpu.get_cpu_capability())
    dep, amb, dist, wrong = measure_fp32_departure()
    print("REF_FP32_DEPARTURE = {" + ", ".join(f'"{k}": {v:.2e}' for k, v in dep.items()) + "}")
    print("ambiguous share:", {f"{c}/{r}": f"{v:.2e}" for (c, r), v in amb.items()})
    print(f"fp32 mean vs fp64, in tau: {dist:.3f}")
    print("unambiguous pixels where the fp32 argmax differs:", wrong)
