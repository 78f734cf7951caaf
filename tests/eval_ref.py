"""Shared inputs and CPU references of the evaluation tests (test_eval_cpu.py, test_gpu_eval.py,
golden/gen_eval_golden.py): seeded low-res maps and targets, the fp64 resize, the ambiguity
threshold of the class map, and the depth / CE sums of include/dclip.h (dclip_upsample_eval_*)
evaluated with torch in a chosen precision."""
import functools

import torch
import torch.nn.functional as F

K = 19
IGNORE = 255
# (B, h, w, H, W): the workload's x16; a non-integer scale with w crossing a 32-column chunk; W past
# one 128-column tile; a wide flat map; a single low-res pixel; the identity; a scale near 1 on a map
# so large that the kernel halves its tile width to fit the low-res patch in LDS
SHAPES = [(2, 8, 16, 128, 256), (1, 5, 37, 43, 301), (2, 4, 33, 64, 528), (1, 3, 70, 17, 1000), (1, 1, 1, 7, 9),
          (1, 6, 6, 6, 6), (1, 11, 66, 12, 68)]
SHAPE_IDS = ["x16", "odd", "two_tiles", "wide", "one_pixel", "identity", "narrow_tile"]
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
SUM_NAMES = ("n", "sq", "log_sq", "abs_rel", "sq_rel", "a1", "a2", "a3", "n_mask", "mask_sq", "d", "d_sq")
FLOAT_SUMS = (1, 2, 3, 4, 9, 10, 11)


@functools.lru_cache(maxsize=None)
def logits(B, h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(1234)
    return (torch.randn(B, K, h, w, generator=g) * 3).to(dtype)


@functools.lru_cache(maxsize=None)
def labels(B, H, W, dtype=torch.int64):
    """~10 % ignore (255), ~0.5 % in 19..254; the wider dtypes also hold negatives and values past 255"""
    g = torch.Generator().manual_seed(1235)
    lab = torch.randint(0, K, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    lab[r < 0.1] = IGNORE
    odd = (r >= 0.1) & (r < 0.105)
    lab[odd] = torch.randint(K, 255, (B, H, W), generator=g)[odd]
    if dtype != torch.uint8:
        wide = (r >= 0.105) & (r < 0.11)
        lab[wide] = torch.tensor([-1, 256, 1000, -300])[torch.randint(0, 4, (B, H, W), generator=g)][wide]
    return lab.to(dtype)


@functools.lru_cache(maxsize=None)
def depth_low(B, h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(1236)
    return (0.5 + 59.5 * torch.rand(B, 1, h, w, generator=g)).to(dtype)


@functools.lru_cache(maxsize=None)
def depth_target(B, H, W):
    g = torch.Generator().manual_seed(1237)
    t = 90 * torch.rand(B, H, W, generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.05] = 0.0
    return t


@functools.lru_cache(maxsize=None)
def depth_mask(B, H, W):
    g = torch.Generator().manual_seed(1238)
    return (torch.rand(B, H, W, generator=g) >= 0.2).to(torch.uint8)


def resize(x, H, W, dtype=torch.float64):
    """F.interpolate(bilinear, align_corners=False) of the map's VALUES (whatever dtype holds them) in `dtype`"""
    return F.interpolate(x.to(dtype), size=(H, W), mode="bilinear", align_corners=False)


def tau(low, h, w):
    """fp32 summation order plus the rounding of the fp32 source coordinate, for a map of this size"""
    return 2.0 ** -24 * float(low.abs().max()) * (32 + 8 * (h + w))


def valid_labels(lab):
    lab = lab.long()
    return (lab != IGNORE) & (lab >= 0) & (lab < K)


def ce_sum(up, lab):
    """sum over the valid pixels of -log softmax(up)[label] in up's dtype (F.cross_entropy, as the trainer)"""
    lab = lab.long()
    lab = torch.where(valid_labels(lab), lab, torch.full_like(lab, IGNORE))
    return float(F.cross_entropy(up, lab, ignore_index=IGNORE, reduction="sum"))


def depth_sums(up, gt, mask, dmin=1e-3, dmax=80.0, clamp=True, eps=1e-6, thr_scale=1.0):
    """The 12 sums of dclip_upsample_eval_depth from a resized prediction `up` (B, 1, H, W), in up's
    dtype throughout (fp64: the reference; fp32: the formulas as compute_depth_errors / SILogLoss
    run them).  thr_scale scales the three thresholds."""
    dt = up.dtype
    up = up[:, 0]
    gt = gt.to(dt)
    m = torch.ones_like(gt, dtype=torch.bool) if mask is None else mask.bool()
    ev = m & (gt >= dmin) & (gt <= dmax)
    g, p = gt[ev], up[ev]
    if clamp:
        p = p.clamp(min=dmin, max=dmax)
    thr = torch.maximum(g / p, p / g)
    diff = g - p
    dlog = torch.log(g) - torch.log(p)
    gm, pm = gt[m], up[m]
    d = torch.log(pm.clamp(min=eps)) - torch.log(gm.clamp(min=eps))
    return [float(ev.sum()), float((diff ** 2).sum()), float((dlog ** 2).sum()), float((diff.abs() / g).sum()),
            float((diff ** 2 / g).sum())] + [float((thr < t * thr_scale).sum()) for t in THRESHOLDS] + \
           [float(m.sum()), float(((gm - pm) ** 2).sum()), float(d.sum()), float((d ** 2).sum())]


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)
