"""Shared inputs and CPU references of the test-time-ensembling tests (test_tta_cpu.py,
test_gpu_tta.py): seeded views, the fp64 ensemble (per view F.interpolate of the values in fp64,
.flip(-1) for a flipped view, softmax under the 'probs' rule, then the mean), the ambiguity
thresholds of the class map, and the measurement of the reference's own fp32 departure
(`python tests/tta_ref.py` prints the table test_gpu_tta.py holds as REF_FP32_DEPARTURE, taken with
torch's scalar CPU kernels so that every machine prints the same figures).
Labels, targets and masks are eval_ref's."""
import functools

import torch
import torch.nn.functional as F

import eval_ref as R

K = R.K
# name -> (B, H, W, [(h, w, flip), ...])
CASES = {
    # the reference's six ratios of a 4 x 8 map, each plain and flipped
    "ms_flip": (1, 64, 128, [(h, 2 * h, f) for h in range(2, 8) for f in (0, 1)]),
    "odd": (2, 43, 301, [(5, 37, 0), (5, 37, 1), (7, 53, 0), (3, 19, 1)]),
    "two_tiles": (2, 64, 528, [(4, 33, 0), (4, 33, 1), (6, 50, 1)]),
    "single": (1, 43, 301, [(5, 37, 0)]),
    "single_flip": (1, 43, 301, [(5, 37, 1)]),
    "identity_pair": (1, 6, 6, [(6, 6, 0), (6, 6, 1)]),
    # the half-width-tile path, forced by the first view alone
    "narrow_tile": (4, 12, 68, [(11, 66, 0), (9, 50, 1)]),
    "x16_pair": (2, 128, 256, [(8, 16, 0), (8, 16, 1)]),
}
LOWS = [torch.bfloat16, torch.float16, torch.float32]
LABS = [torch.int64, torch.int32, torch.uint8]
LAB_OF_LOW = dict(zip(LOWS, LABS))  # one label dtype per low dtype: every label path, no extra cases
RULES = ["logits", "probs"]
AMBIGUOUS_CAP = 2e-3
# (case, low dtype, mask kind, clamp) of the depth test
DEPTH_CASES = [(c, low, "mask", 1) for c in ("ms_flip", "odd", "narrow_tile") for low in LOWS] + \
              [(c, torch.float32, m, k) for c in ("ms_flip", "odd", "narrow_tile")
               for m, k in (("mask", 0), ("none", 0), ("none", 1))]


@functools.lru_cache(maxsize=None)
def seg_view(i, B, h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(2000 + i)
    return (torch.randn(B, K, h, w, generator=g) * 3).to(dtype)


@functools.lru_cache(maxsize=None)
def depth_view(i, B, h, w, dtype=torch.float32):
    """eval_ref.depth_low's recipe, one seed per view"""
    g = torch.Generator().manual_seed(3000 + i)
    return (0.5 + 59.5 * torch.rand(B, 1, h, w, generator=g)).to(dtype)


def seg_views(case, low):
    B, H, W, views = CASES[case]
    return [seg_view(i, B, h, w, low) for i, (h, w, f) in enumerate(views)]


def depth_views(case, low):
    B, H, W, views = CASES[case]
    return [depth_view(i, B, h, w, low) for i, (h, w, f) in enumerate(views)]


def ensemble(maps, flips, H, W, probs=False, dtype=torch.float64, order=None):
    """The mean over the views (in `order`, default as given) of the resized, mirrored-back maps,
    through a softmax over dim 1 first under the 'probs' rule, in `dtype` throughout."""
    outs = []
    for i in (range(len(maps)) if order is None else order):
        u = R.resize(maps[i], H, W, dtype)
        if flips[i]:
            u = u.flip(-1)
        outs.append(torch.softmax(u, dim=1) if probs else u)
    return torch.stack(outs).mean(0)


def flips_of(case):
    return [f for _, _, f in CASES[case][3]]


@functools.lru_cache(maxsize=None)
def seg_reference(case, low, rule):
    """(mean fp64 (B, K, H, W), tau) of the case's views as the low dtype holds them"""
    B, H, W, views = CASES[case]
    maps = seg_views(case, low)
    u = ensemble(maps, flips_of(case), H, W, probs=rule == "probs")
    return u, tau_of(maps, views, u, rule)


@functools.lru_cache(maxsize=None)
def depth_reference(case, low):
    """(mean fp64 (B, 1, H, W), tau) of the case's depth views"""
    B, H, W, views = CASES[case]
    maps = depth_views(case, low)
    u = ensemble(maps, flips_of(case), H, W)
    return u, tau_of(maps, views, u, "logits")


def tau_of(maps, views, mean, rule):
    """logits: the views' mean resize error (eval_ref.tau: fp32 summation order plus the rounding of
    the fp32 source coordinate) plus the V + 1 roundings of the fp32 mean.  probs: a quarter of the
    views' mean resize error (a softmax output p moves by p (1 - p) <= 1/4 per unit of its input)
    plus 2^-20 for the fp32 exponentials, the division and the mean."""
    t = sum(R.tau(m.float(), h, w) for m, (h, w, _) in zip(maps, views)) / len(maps)
    if rule == "probs":
        return t / 4 + 2.0 ** -20
    return t + 2.0 ** -24 * (len(maps) + 1) * float(mean.abs().max())


def check_class_map(pred, u, tau, cap=AMBIGUOUS_CAP):
    """pred (B, H, W) uint8 on the CPU against the fp64 ensemble `u`: every pixel whose top-2 gap is
    at least tau equals argmax u, an ambiguous one picks a class within tau of the maximum, and at
    most `cap` of the pixels are ambiguous.  Returns the ambiguous pixels' mask."""
    top = u.topk(2, dim=1).values
    amb = (top[:, 0] - top[:, 1]) < tau
    frac = float(amb.float().mean())
    print(f"ambiguous {frac:.2e} (tau {tau:.3e})")
    assert frac <= cap, frac
    p = pred.long()
    wrong = (p != u.argmax(1)) & ~amb
    assert not bool(wrong.any()), f"{int(wrong.sum())} unambiguous pixels differ from argmax of the fp64 ensemble"
    picked = u.gather(1, p.unsqueeze(1))[:, 0]
    assert bool((top[:, 0] - picked <= tau).all()), "an ambiguous pixel picked a class further than tau from the maximum"
    return amb


def ce_sum(mean, lab, rule):
    """sum over the valid pixels of -log softmax(mean)[label] (logits) or -log mean[label] (probs),
    in mean's dtype"""
    if rule == "logits":
        return R.ce_sum(mean, lab)
    lab = lab.long()
    lab = torch.where(R.valid_labels(lab), lab, torch.full_like(lab, R.IGNORE))
    return float(F.nll_loss(torch.log(mean), lab, ignore_index=R.IGNORE, reduction="sum"))


def mask_of(kind, B, H, W):
    return {"mask": R.depth_mask(B, H, W), "none": None}[kind]


def measure_fp32_departure():
    """The largest relative departure, over the inputs the GPU tests use, of the reference's own fp32
    path (the same torch sequence in fp32) from its fp64 evaluation: the CE sum under each rule and
    every floating depth sum.  Also the ambiguous share per rule and the worst fp32-vs-fp64 distance
    of the mean in units of tau."""
    dep = {"ce_logits": 0.0, "ce_probs": 0.0}
    amb = {"logits": 0.0, "probs": 0.0}
    dist = {"logits": 0.0, "probs": 0.0}
    wrong = 0
    for case, (B, H, W, views) in CASES.items():
        for low in LOWS:
            lab = R.labels(B, H, W, LAB_OF_LOW[low])
            for rule in RULES:
                u64, tau = seg_reference(case, low, rule)
                u32 = ensemble(seg_views(case, low), flips_of(case), H, W, probs=rule == "probs", dtype=torch.float32)
                dep["ce_" + rule] = max(dep["ce_" + rule], R.rel(ce_sum(u32, lab, rule), ce_sum(u64, lab, rule)))
                top = u64.topk(2, dim=1).values
                a = (top[:, 0] - top[:, 1]) < tau
                amb[rule] = max(amb[rule], float(a.float().mean()))
                dist[rule] = max(dist[rule], float((u32.double() - u64).abs().max()) / tau)
                wrong += int(((u32.argmax(1) != u64.argmax(1)) & ~a).sum())
    for case, low, kind, clamp in DEPTH_CASES:
        B, H, W, views = CASES[case]
        u64, _ = depth_reference(case, low)
        u32 = ensemble(depth_views(case, low), flips_of(case), H, W, dtype=torch.float32)
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
    # torch's vectorised CPU kernels (softmax, log, the resize) round differently per instruction set:
    # the probs-rule CE departure comes out as 1.68e-7 under one AVX2 build and 1.10e-7 under an
    # AVX-512 one.  The table is taken with the scalar kernels, which give every CPU the same figures
    # (and, for both CE sums, the smallest: the tightest bound).
    if os.environ.get("ATEN_CPU_CAPABILITY") != "default":
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)],
                                 env=dict(os.environ, ATEN_CPU_CAPABILITY="default")))
    print("CPU capability:", torch.backends.cpu.get_cpu_capability())
    dep, amb, dist, wrong = measure_fp32_departure()
    print("REF_FP32_DEPARTURE = {" + ", ".join(f'"{k}": {v:.2e}' for k, v in dep.items()) + "}")
    print("ambiguous share:", {k: f"{v:.2e}" for k, v in amb.items()})
    print("fp32 mean vs fp64, in tau:", {k: f"{v:.3f}" for k, v in dist.items()})
    print("unambiguous pixels where the fp32 argmax differs:", wrong)
