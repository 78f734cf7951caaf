"""Time one validation update of the two heads, fused against unfused, in one process.

    python tools/bench_eval.py [--batch 8] [--rounds 12] [--inner 5] [--dtype bf16]

At B x (19 | 1) x 64 x 128 heads -> 1024 x 2048 labels (the benchmark's shapes), interleaved ABBA:
  (A) the unfused path built only from what the package had before evaluate.py: ops.upsample of both
      heads (the (B, 19, H, W) fp32 logits are materialised), argmax, a bincount confusion matrix and
      the depth errors / masked RMSE / SILog sums as masked torch reductions;
  (A+CE) the same plus F.cross_entropy(reduction='sum') on the resized logits, which (B) also computes;
  (B) one Evaluator.update (csrc/headeval.hip).
Every arm ends in a device synchronise; times are device-event times of `inner` back-to-back calls.
Prints per-arm median / min / max over the rounds, the ratios, the separate times of (B)'s two
kernels' ops, and (B)'s achieved bytes/s against the bytes it has to move (labels, depth target,
mask and the low-res maps, computed from the shapes), then one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from denseclip_vit_multimodal_amd import ops  # noqa: E402
from denseclip_vit_multimodal_amd.evaluate import Evaluator, _E  # noqa: E402
from denseclip_vit_multimodal_amd.train import synth_batch  # noqa: E402

K = 19


def unfused(seg_low, depth_low, seg, depth, mask, size, with_ce=False, dmin=1e-3, dmax=80.0, eps=1e-6):
    up = ops.upsample(seg_low, size)
    pred = up.argmax(1)
    valid = (seg != 255) & (seg >= 0) & (seg < K)
    idx = torch.where(valid, seg * K + pred, torch.full_like(seg, K * K))
    cm = torch.bincount(idx.view(-1), minlength=K * K + 1)[:K * K].view(K, K)
    out = [cm]
    if with_ce:
        out.append(F.cross_entropy(up, seg, ignore_index=255, reduction="sum"))
    d = ops.upsample(depth_low, size)
    m = mask.bool()
    ev = m & (depth >= dmin) & (depth <= dmax)
    p = d.clamp(min=dmin, max=dmax)
    g = torch.where(ev, depth, torch.ones_like(depth))
    p = torch.where(ev, p, torch.ones_like(p))
    thr = torch.maximum(g / p, p / g)
    diff = g - p
    dlog = torch.log(g) - torch.log(p)
    z = torch.zeros_like(d)
    dm = torch.where(m, depth - d, z)
    sd = torch.where(m, torch.log(d.clamp(min=eps)) - torch.log(depth.clamp(min=eps)), z)
    out += [ev.sum(), (diff ** 2).sum(), (dlog ** 2).sum(), (diff.abs() / g).sum(), (diff ** 2 / g).sum(),
            (ev & (thr < 1.25)).sum(), (ev & (thr < 1.25 ** 2)).sum(), (ev & (thr < 1.25 ** 3)).sum(), m.sum(),
            (dm ** 2).sum(), sd.sum(), (sd ** 2).sum()]
    return out


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs a GPU (no CPU fallback, no timing without one)")
    dev = torch.device("cuda")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    B, H, W = a.batch, a.height, a.width
    h, w = H // 16, W // 16
    g = torch.Generator().manual_seed(1234)
    seg_low = (torch.randn(B, K, h, w, generator=g) * 3).to(dev).to(dt)
    depth_low = (0.5 + 59.5 * torch.rand(B, 1, h, w, generator=g)).to(dev).to(dt)
    _, seg, depth, mask = synth_batch(B, H, W, dev, image_dtype=torch.float32)
    mask_u8 = mask.to(torch.uint8)
    ev = Evaluator(device=dev)
    E = _E()
    tg, mk = depth.reshape(B, H, W), mask_u8.reshape(B, H, W)

    arms = {
        "A": lambda: unfused(seg_low, depth_low, seg, depth, mask, (H, W)),
        "A+CE": lambda: unfused(seg_low, depth_low, seg, depth, mask, (H, W), with_ce=True),
        "B": lambda: ev.update(seg_low, depth_low, seg, depth, mask_u8),
        "B.seg": lambda: E.seg_update(seg_low, seg, 255, ev.cm, ev.ce_sums, False),
        "B.depth": lambda: E.depth_update(depth_low, tg, mk, 1e-3, 80.0, True, 1e-6, ev.depth_sums, False),
    }
    # the two paths agree before anything is timed
    ref = unfused(seg_low, depth_low, seg, depth, mask, (H, W), with_ce=True)
    ev.update(seg_low, depth_low, seg, depth, mask_u8)
    torch.cuda.synchronize()
    cm_diff = int((ev.cm - ref[0]).abs().sum())
    ce_rel = abs(float(ev.ce_sums[0]) - float(ref[1])) / abs(float(ref[1]))
    sums_rel = max(abs(float(ev.depth_sums[i]) - float(ref[2 + i])) / max(abs(float(ref[2 + i])), 1e-30)
                   for i in range(12))
    print(f"agreement: confusion-matrix L1 difference {cm_diff} of {int(ev.cm.sum())} pixels, CE sum rel {ce_rel:.2e}, "
          f"depth sums max rel {sums_rel:.2e} (the unfused sums are fp32 reductions)")

    for fn in arms.values():  # warm every arm
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for r in range(a.rounds):
        order = ["A", "B", "B", "A"] if r % 2 == 0 else ["B", "A", "A", "B"]
        for k in order + ["A+CE", "B.seg", "B.depth"]:
            times[k].append(timed(arms[k], a.inner))
    stat = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}
    for k, s in stat.items():
        print(f"{k:8s} median {s['median_ms']:8.3f} ms   min {s['min_ms']:8.3f}   max {s['max_ms']:8.3f}   "
              f"({len(times[k])} x {a.inner} calls)")
    px = B * H * W
    low_bytes = (seg_low.numel() + depth_low.numel()) * seg_low.element_size()
    bytes_b = px * (seg.element_size() + 4 + 1) + low_bytes
    bytes_a = px * (K * 4 * 3 + 8 * 3 + 4 * 2) + low_bytes  # logits written, read by argmax and CE; labels; depth map
    res = {"shape": [B, K, h, w, H, W], "dtype": a.dtype, "times": stat,
           "ratio_A_over_B": stat["A"]["median_ms"] / stat["B"]["median_ms"],
           "ratio_A+CE_over_B": stat["A+CE"]["median_ms"] / stat["B"]["median_ms"],
           "B_bytes": bytes_b, "B_GBps": bytes_b / stat["B"]["median_ms"] / 1e6,
           "A_bytes_at_least": bytes_a, "cm_l1_diff": cm_diff, "ce_rel": ce_rel, "depth_sums_rel": sums_rel}
    print(f"(B) moves {bytes_b / 1e9:.3f} GB by its shapes: {res['B_GBps']:.0f} GB/s achieved; "
          f"A / B = {res['ratio_A_over_B']:.2f}, (A+CE) / B = {res['ratio_A+CE_over_B']:.2f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
