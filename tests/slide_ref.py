"""Shared inputs and CPU references of the sliding-window tests (test_slide_cpu.py,
test_gpu_slide.py): the window rule of mmseg's slide_inference restated on its own, seeded low-res
maps per window, the fp64 reference (per window F.interpolate of the values in fp64 to the window
size, added into an image-sized accumulator beside a count map, then the division), the ambiguity
threshold of the class map, and the measurement of the reference's own fp32 departure
(`python tests/slide_ref.py` prints the table test_gpu_slide.py holds as REF_FP32_DEPARTURE, taken
with torch's scalar CPU kernels so that every machine prints the same figures).
Labels, targets and masks are eval_ref's."""
import functools

import torch

import eval_ref as R
from tta_ref import AMBIGUOUS_CAP, LAB_OF_LOW, LOWS, check_class_map, mask_of  # noqa: F401

K = R.K
# name -> (B, H, W, crop_size, stride, (h, w) of a window's low-res map)
CASES = {
    # the Cityscapes geometry (1024 x 2048, crop 512 x 1024, stride 341 x 683) at 1/16: 9 windows at
    # y {0, 21, 32}, x {0, 42, 64}, the last row / column shifted back, counts 1, 2 and 4, the x16 resize
    "thirds": (1, 64, 128, (32, 64), (21, 42), (2, 4)),
    # odd origins (13, 23; 87, 170), W % 4 != 0, a non-integer scale, window edges inside the tiles
    "odd": (2, 43, 301, (20, 131), (13, 87), (5, 37)),
    # 12 windows, up to 9 on a pixel
    "dense": (1, 40, 96, (24, 48), (8, 16), (3, 6)),
    # no overlap: every count 1
    "exact": (2, 32, 64, (16, 32), (16, 32), (4, 8)),
    # the image smaller than the crop: one 20 x 50 window
    "small_image": (1, 20, 50, (32, 64), (21, 42), (5, 12)),
    # two windows whose edges (228, 300) fall inside 128-column tiles
    "straddle": (2, 24, 528, (24, 300), (24, 228), (4, 33)),
    # the half-width-tile path (the patch of a 128-column tile past 48 KiB), origins x {0, 34, 68}
    "narrow_tile": (4, 12, 136, (12, 68), (12, 34), (11, 66)),
}
# (case, low dtype, mask kind, clamp) of the depth test
DEPTH_CASES = [(c, low, "mask", 1) for c in ("thirds", "odd", "narrow_tile") for low in LOWS] + \
              [(c, torch.float32, m, k) for c in ("thirds", "odd", "narrow_tile")
               for m, k in (("mask", 0), ("none", 0), ("none", 1))]


def windows(H, W, crop, stride):
    """((wh, ww), [(y0, x0), ...]) by the rule, written out independently of evaluate.slide_windows"""
    (ch, cw), (sh, sw) = crop, stride
    origins = []
    for i in range(max(H - ch + sh - 1, 0) // sh + 1):
        for j in range(max(W - cw + sw - 1, 0) // sw + 1):
            y2, x2 = min(i * sh + ch, H), min(j * sw + cw, W)
            origins.append((max(y2 - ch, 0), max(x2 - cw, 0)))
    return (min(ch, H), min(cw, W)), origins


def geometry(case):
    """(B, H, W, (wh, ww), origins, (h, w)) of a case"""
    B, H, W, crop, stride, low = CASES[case]
    size, origins = windows(H, W, crop, stride)
    return B, H, W, size, origins, low


@functools.lru_cache(maxsize=None)
def seg_low(g, B, h, w, dtype=torch.float32):
    """eval_ref.logits' recipe, one seed per window"""
    gen = torch.Generator().manual_seed(4000 + g)
    return (torch.randn(B, K, h, w, generator=gen) * 3).to(dtype)


@functools.lru_cache(maxsize=None)
def depth_low(g, B, h, w, dtype=torch.float32):
    """eval_ref.depth_low's recipe, one seed per window"""
    gen = torch.Generator().manual_seed(5000 + g)
    return (0.5 + 59.5 * torch.rand(B, 1, h, w, generator=gen)).to(dtype)


def seg_lows(case, low):
    B, H, W, size, origins, (h, w) = geometry(case)
    return [seg_low(g, B, h, w, low) for g in range(len(origins))]


def depth_lows(case, low):
    B, H, W, size, origins, (h, w) = geometry(case)
    return [depth_low(g, B, h, w, low) for g in range(len(origins))]


def slide(maps, origins, size, H, W, dtype=torch.float64, order=None):
    """(result, count): every window's map resized to `size` in `dtype` and added into an H x W
    accumulator at its origin (in `order`, default as given), a count map, the division."""
    wh, ww = size
    B, C = maps[0].shape[:2]
    acc = torch.zeros(B, C, H, W, dtype=dtype)
    cnt = torch.zeros(1, 1, H, W, dtype=dtype)
    for g in (range(len(maps)) if order is None else order):
        y0, x0 = origins[g]
        acc[:, :, y0:y0 + wh, x0:x0 + ww] += R.resize(maps[g], wh, ww, dtype)
        cnt[:, :, y0:y0 + wh, x0:x0 + ww] += 1
    assert bool((cnt > 0).all())
    return acc / cnt, cnt


def tau_of(maps, low_hw, result, cmax):
    """the largest resize error of a window (eval_ref.tau: fp32 summation order plus the rounding of
    the fp32 source coordinate; a mean of such values errs by no more) plus the cmax + 1 roundings of
    the fp32 sum and division"""
    h, w = low_hw
    return max(R.tau(m.float(), h, w) for m in maps) + 2.0 ** -24 * (cmax + 1) * float(result.abs().max())


@functools.lru_cache(maxsize=None)
def seg_reference(case, low):
    """(result fp64 (B, K, H, W), tau) of the case's windows as the low dtype holds them"""
    B, H, W, size, origins, hw = geometry(case)
    maps = seg_lows(case, low)
    u, cnt = slide(maps, origins, size, H, W)
    return u, tau_of(maps, hw, u, int(cnt.max()))


@functools.lru_cache(maxsize=None)
def depth_reference(case, low):
    """(result fp64 (B, 1, H, W), tau) of the case's depth windows"""
    B, H, W, size, origins, hw = geometry(case)
    maps = depth_lows(case, low)
    u, cnt = slide(maps, origins, size, H, W)
    return u, tau_of(maps, hw, u, int(cnt.max()))


def measure_fp32_departure():
    """The largest relative departure, over the inputs the GPU tests use, of the reference's own fp32
    path (the same torch sequence in fp32) from its fp64 evaluation: the CE sum and every floating
    depth sum.  Also the largest ambiguous share, the worst fp32-vs-fp64 distance of the result in
    units of tau and the number of unambiguous pixels on which the fp32 argmax differs."""
    dep = {"ce": 0.0}
    amb, dist, wrong = {}, 0.0, 0
    for case in CASES:
        B, H, W, size, origins, hw = geometry(case)
        for low in LOWS:
            lab = R.labels(B, H, W, LAB_OF_LOW[low])
            u64, tau = seg_reference(case, low)
            u32, _ = slide(seg_lows(case, low), origins, size, H, W, dtype=torch.float32)
            dep["ce"] = max(dep["ce"], R.rel(R.ce_sum(u32, lab), R.ce_sum(u64, lab)))
            top = u64.topk(2, dim=1).values
            a = (top[:, 0] - top[:, 1]) < tau
            amb[case] = max(amb.get(case, 0.0), float(a.float().mean()))
            dist = max(dist, float((u32.double() - u64).abs().max()) / tau)
            wrong += int(((u32.argmax(1) != u64.argmax(1)) & ~a).sum())
    for case, low, kind, clamp in DEPTH_CASES:
        B, H, W, size, origins, hw = geometry(case)
        u64, _ = depth_reference(case, low)
        u32, _ = slide(depth_lows(case, low), origins, size, H, W, dtype=torch.float32)
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
    # scalar kernels, which give every CPU the same figures (as tta_ref.py does)
    if os.environ.get("ATEN_CPU_CAPABILITY") != "default":
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)],
                                 env=dict(os.environ, ATEN_CPU_CAPABILITY="default")))
    print("CPU capability:", torch.backends.cpu.get_cpu_capability())
    dep, amb, dist, wrong = measure_fp32_departure()
    print("REF_FP32_DEPARTURE = {" + ", ".join(f'"{k}": {v:.2e}' for k, v in dep.items()) + "}")
    print("ambiguous share:", {k: f"{v:.2e}" for k, v in amb.items()})
    print(f"fp32 result vs fp64, in tau: {dist:.3f}")
    print("unambiguous pixels where the fp32 argmax differs:", wrong)
