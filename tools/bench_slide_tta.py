"""Time sliding-window inference inside multi-scale + flip ensembling of one validation update, fused
against unfused, in one process.

    python tools/bench_slide_tta.py [--batch 1] [--rounds 6] [--inner 2] [--dtype bf16] [--average probs]

At batch x 1024 x 2048 with the reference's ViT test_cfg (crop 640, stride 426) under its --aug-test
ratios 0.5 .. 1.75 plus flip (evaluate.view_windows: 12 views, 196 windows), on synthetic low-res maps
of the size the benchmark model (heads at 1/16 of the crop) gives them; no model forwards.
Interleaved ABBA:
  (A) the unfused torch sequence on those maps, mmseg's aug_test over slide_inference: per view a
      (B, 19, Hv, Wv) fp32 accumulator and a count map filled window by window (F.interpolate to the
      window size), the division, F.interpolate to the image, .flip(-1), softmax, added into the
      running sum over the views; then argmax, a bincount confusion matrix and the CE sum; likewise
      the depth, then the 12 sums as masked torch reductions;
  (B) one Evaluator.update_view_windows (csrc/headslidetta.hip: one fused launch per head).
Every arm ends in a device synchronise; times are device-event times of `inner` back-to-back calls.
Prints per-arm median / min / max over the rounds, the ratio, (B)'s two ops on their own and the peak
memory each arm allocates on top of its inputs (torch.cuda.max_memory_allocated).  Ends with one JSON
line.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from denseclip_vit_multimodal_amd.evaluate import TTA_SCALES, Evaluator, _E, view_windows  # noqa: E402
from denseclip_vit_multimodal_amd.train import synth_batch  # noqa: E402

K = 19
PATCH = 16


def view_mean(lows, view, size, probs):
    """mmseg's slide_inference of one view on its windows' low-res maps, resized to the image and
    mirrored back (inference + aug_test's per-view part)"""
    Hv, Wv, flip, (wh, ww), origins = view
    B, C = lows[0].shape[:2]
    acc = torch.zeros(B, C, Hv, Wv, device=lows[0].device)
    cnt = torch.zeros(1, 1, Hv, Wv, device=lows[0].device)
    for low, (y0, x0) in zip(lows, origins):
        acc[:, :, y0:y0 + wh, x0:x0 + ww] += F.interpolate(low.float(), size=(wh, ww), mode="bilinear",
                                                           align_corners=False)
        cnt[:, :, y0:y0 + wh, x0:x0 + ww] += 1
    u = acc / cnt
    if (Hv, Wv) != tuple(size):
        u = F.interpolate(u, size=tuple(size), mode="bilinear", align_corners=False)
    if flip:
        u = u.flip(-1)
    return torch.softmax(u, dim=1) if probs else u


def ensemble(lows, table, size, probs):
    total, at = None, 0
    for view in table:
        n = len(view[4])
        u = view_mean(lows[at:at + n], view, size, probs)
        total = u if total is None else total.add_(u)
        at += n
    return total / len(table)


def unfused(seg_lows, depth_lows, table, seg, depth, mask, size, probs, dmin=1e-3, dmax=80.0, eps=1e-6):
    up = ensemble(seg_lows, table, size, probs)
    pred = up.argmax(1)
    valid = (seg != 255) & (seg >= 0) & (seg < K)
    idx = torch.where(valid, seg * K + pred, torch.full_like(seg, K * K))
    cm = torch.bincount(idx.view(-1), minlength=K * K + 1)[:K * K].view(K, K)
    if probs:
        ce = F.nll_loss(torch.log(up), seg, ignore_index=255, reduction="sum")
    else:
        ce = F.cross_entropy(up, seg, ignore_index=255, reduction="sum")
    d = ensemble(depth_lows, table, size, False)
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
    sums = [ev.sum(), (diff ** 2).sum(), (dlog ** 2).sum(), (diff.abs() / g).sum(), (diff ** 2 / g).sum(),
            (ev & (thr < 1.25)).sum(), (ev & (thr < 1.25 ** 2)).sum(), (ev & (thr < 1.25 ** 3)).sum(), m.sum(),
            (dm ** 2).sum(), sd.sum(), (sd ** 2).sum()]
    return pred, cm, ce, sums


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def peak_extra(fn):
    """bytes the call allocates at its peak on top of what is allocated on entry"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--crop", type=int, nargs=2, default=(640, 640))
    ap.add_argument("--stride", type=int, nargs=2, default=(426, 426))
    ap.add_argument("--scales", type=float, nargs="+", default=TTA_SCALES)
    ap.add_argument("--no-flip", action="store_true")
    ap.add_argument("--average", choices=["logits", "probs"], default="probs")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_slide_tta needs a GPU (no CPU fallback, no timing without one)")
    dev = torch.device("cuda")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    B, H, W = a.batch, a.height, a.width
    crop, stride, probs = tuple(a.crop), tuple(a.stride), a.average == "probs"
    table = view_windows(H, W, crop, stride, tuple(a.scales), not a.no_flip)
    views = [(Hv, Wv, int(f), wh, ww, len(o)) for Hv, Wv, f, (wh, ww), o in table]
    origins = [xy for v in table for xy in v[4]]
    vflat, oflat = [c for v in views for c in v], [c for o in origins for c in o]
    g = torch.Generator().manual_seed(1234)
    seg_lows, depth_lows = [], []
    for Hv, Wv, f, (wh, ww), o in table:
        h, w = -(-wh // PATCH), -(-ww // PATCH)
        seg_lows += [(torch.randn(B, K, h, w, generator=g) * 3).to(dev).to(dt) for _ in o]
        depth_lows += [(0.5 + 59.5 * torch.rand(B, 1, h, w, generator=g)).to(dev).to(dt) for _ in o]
    _, seg, depth, mask = synth_batch(B, H, W, dev, image_dtype=torch.float32)
    mask_u8 = mask.to(torch.uint8)
    tg, mk = depth.reshape(B, H, W), mask_u8.reshape(B, H, W)
    ev = Evaluator(device=dev)
    E = _E()
    print(f"{len(table)} views, {len(origins)} windows: " +
          ", ".join(f"{Hv}x{Wv}{'f' if f else ''}:{len(o)}" for Hv, Wv, f, s, o in table) + f"; average {a.average}")

    arms = {
        "A": lambda: unfused(seg_lows, depth_lows, table, seg, depth, mask, (H, W), probs),
        "B": lambda: ev.update_view_windows(seg_lows, depth_lows, views, origins, seg, depth, mask_u8,
                                            average=a.average),
        "B.seg": lambda: E.slide_tta_seg_update(seg_lows, vflat, oflat, seg, 255, probs, ev.cm, ev.ce_sums, False),
        "B.depth": lambda: E.slide_tta_depth_update(depth_lows, vflat, oflat, tg, mk, 1e-3, 80.0, True, 1e-6,
                                                    ev.depth_sums, False),
    }
    # the two paths agree before anything is timed
    pred_a, cm_a, ce_a, sums_a = arms["A"]()
    pred_b = E.slide_tta_argmax(seg_lows, vflat, oflat, H, W, probs)
    ev.update_view_windows(seg_lows, depth_lows, views, origins, seg, depth, mask_u8, average=a.average)
    torch.cuda.synchronize()
    px = B * H * W
    map_diff = int((pred_a != pred_b).sum())
    cm_diff = int((ev.cm - cm_a).abs().sum())
    ce_rel = abs(float(ev.ce_sums[0]) - float(ce_a)) / abs(float(ce_a))
    sums_rel = max(abs(float(ev.depth_sums[i]) - float(sums_a[i])) / max(abs(float(sums_a[i])), 1e-30)
                   for i in range(12))
    print(f"agreement: {map_diff} of {px} class ids differ, confusion-matrix L1 difference {cm_diff}, CE sum rel "
          f"{ce_rel:.2e}, depth sums max rel {sums_rel:.2e} (the unfused sums are fp32 reductions)")
    del pred_a, cm_a, ce_a, sums_a, pred_b
    ev.reset()

    peaks = {k: peak_extra(arms[k]) for k in ("A", "B")}
    for fn in arms.values():  # warm every arm
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for r in range(a.rounds):
        order = ["A", "B", "B", "A"] if r % 2 == 0 else ["B", "A", "A", "B"]
        for k in order + ["B.seg", "B.depth"]:
            times[k].append(timed(arms[k], a.inner))
    stat = {k: stats(v) for k, v in times.items()}
    for k, s in stat.items():
        print(f"{k:8s} median {s['median_ms']:8.3f} ms   min {s['min_ms']:8.3f}   max {s['max_ms']:8.3f}   "
              f"({len(times[k])} x {a.inner} calls)")
    res = {"shape": [B, H, W], "crop_size": crop, "stride": stride, "scales": list(a.scales), "flip": not a.no_flip,
           "average": a.average, "views": views, "windows": len(origins), "dtype": a.dtype, "times": stat,
           "ratio_A_over_B": stat["A"]["median_ms"] / stat["B"]["median_ms"], "peak_extra_bytes": peaks,
           "class_ids_differ": map_diff, "cm_l1_diff": cm_diff, "ce_rel": ce_rel, "depth_sums_rel": sums_rel}
    print(f"A / B = {res['ratio_A_over_B']:.2f}; peak memory on top of the inputs: A {peaks['A'] / 2 ** 20:.1f} MiB, "
          f"B {peaks['B'] / 2 ** 20:.1f} MiB")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
