"""Time sliding-window inference of one validation update, fused against unfused, in one process.

    python tools/bench_slide.py [--batch 1] [--rounds 10] [--inner 3] [--dtype bf16] [--no-model]

At batch x 1024 x 2048 with windows of 512 x 1024 at stride (341, 683) (evaluate.slide_windows: nine
windows, up to four on a pixel), whose low-res maps have the size the benchmark model (ViT-B/16, heads
at 1/16 of the crop) gives them, 32 x 64, random values.  Interleaved ABBA:
  (A) the unfused torch sequence on those maps, mmseg's slide_inference: per window F.interpolate to
      the window size (a (B, 19, 512, 1024) fp32 tensor), added into a (B, 19, H, W) fp32 accumulator at
      the window's origin, +1 into a count map, the division, argmax, a bincount confusion matrix and
      the CE sum; likewise the depth, then the 12 sums as masked torch reductions;
  (B) one Evaluator.update_windows (csrc/headslide.hip: one fused launch per head).
Every arm ends in a device synchronise; times are device-event times of `inner` back-to-back calls.
Prints per-arm median / min / max over the rounds, the ratio, (B)'s two ops on their own, the peak
memory each arm allocates on top of its inputs, and, unless --no-model, for the benchmark model on one
image: the nine window forwards (evaluate.forward_windows) beside one forward of the whole image,
and a whole evaluate.predict_slide beside the time of its two slide ops alone.  Ends with one JSON
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

from denseclip_vit_multimodal_amd.evaluate import (Evaluator, _E, forward_windows, predict_slide,  # noqa: E402
                                                   slide_windows)
from denseclip_vit_multimodal_amd.train import synth_batch  # noqa: E402

K = 19
PATCH = 16


def full_size_mean(lows, origins, window, size):
    """mmseg's slide_inference on the windows' low-res maps: accumulator, count map, division"""
    (wh, ww), (H, W) = window, size
    B, C = lows[0].shape[:2]
    acc = torch.zeros(B, C, H, W, device=lows[0].device)
    cnt = torch.zeros(1, 1, H, W, device=lows[0].device)
    for low, (y0, x0) in zip(lows, origins):
        acc[:, :, y0:y0 + wh, x0:x0 + ww] += F.interpolate(low.float(), size=(wh, ww), mode="bilinear",
                                                           align_corners=False)
        cnt[:, :, y0:y0 + wh, x0:x0 + ww] += 1
    return acc / cnt


def unfused(seg_lows, depth_lows, origins, window, seg, depth, mask, size, dmin=1e-3, dmax=80.0, eps=1e-6):
    up = full_size_mean(seg_lows, origins, window, size)
    pred = up.argmax(1)
    valid = (seg != 255) & (seg >= 0) & (seg < K)
    idx = torch.where(valid, seg * K + pred, torch.full_like(seg, K * K))
    cm = torch.bincount(idx.view(-1), minlength=K * K + 1)[:K * K].view(K, K)
    ce = F.cross_entropy(up, seg, ignore_index=255, reduction="sum")
    d = full_size_mean(depth_lows, origins, window, size)
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
    ap.add_argument("--crop", type=int, nargs=2, default=(512, 1024))
    ap.add_argument("--stride", type=int, nargs=2, default=(341, 683))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--no-model", action="store_true", help="skip the whole-model timings")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_slide needs a GPU (no CPU fallback, no timing without one)")
    dev = torch.device("cuda")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    B, H, W = a.batch, a.height, a.width
    crop, stride = tuple(a.crop), tuple(a.stride)
    window, origins = slide_windows(H, W, crop, stride)
    flat = [c for o in origins for c in o]
    h, w = window[0] // PATCH, window[1] // PATCH
    g = torch.Generator().manual_seed(1234)
    seg_lows = [(torch.randn(B, K, h, w, generator=g) * 3).to(dev).to(dt) for _ in origins]
    depth_lows = [(0.5 + 59.5 * torch.rand(B, 1, h, w, generator=g)).to(dev).to(dt) for _ in origins]
    _, seg, depth, mask = synth_batch(B, H, W, dev, image_dtype=torch.float32)
    mask_u8 = mask.to(torch.uint8)
    tg, mk = depth.reshape(B, H, W), mask_u8.reshape(B, H, W)
    ev = Evaluator(device=dev)
    E = _E()
    print(f"windows {window[0]} x {window[1]} from {h} x {w} maps at {origins}")

    arms = {
        "A": lambda: unfused(seg_lows, depth_lows, origins, window, seg, depth, mask, (H, W)),
        "B": lambda: ev.update_windows(seg_lows, depth_lows, window, origins, seg, depth, mask_u8),
        "B.seg": lambda: E.slide_seg_update(seg_lows, flat, *window, seg, 255, ev.cm, ev.ce_sums, False),
        "B.depth": lambda: E.slide_depth_update(depth_lows, flat, *window, tg, mk, 1e-3, 80.0, True, 1e-6,
                                                ev.depth_sums, False),
    }
    # the two paths agree before anything is timed
    pred_a, cm_a, ce_a, sums_a = arms["A"]()
    pred_b = E.slide_argmax(seg_lows, flat, *window, H, W)
    ev.update_windows(seg_lows, depth_lows, window, origins, seg, depth, mask_u8)
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
        for _ in range(2):
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
    low_bytes = sum(v.numel() * v.element_size() for v in seg_lows + depth_lows)
    bytes_b = px * (seg.element_size() + 4 + 1) + low_bytes
    res = {"shape": [B, H, W], "crop_size": crop, "stride": stride, "window": window, "origins": origins,
           "low": [h, w], "dtype": a.dtype, "times": stat,
           "ratio_A_over_B": stat["A"]["median_ms"] / stat["B"]["median_ms"],
           "peak_extra_bytes": peaks, "B_bytes": bytes_b, "B_GBps": bytes_b / stat["B"]["median_ms"] / 1e6,
           "class_ids_differ": map_diff, "cm_l1_diff": cm_diff, "ce_rel": ce_rel, "depth_sums_rel": sums_rel}
    print(f"A / B = {res['ratio_A_over_B']:.2f}; peak memory on top of the inputs: A {peaks['A'] / 2 ** 20:.1f} MiB, "
          f"B {peaks['B'] / 2 ** 20:.1f} MiB; (B) moves {bytes_b / 1e6:.1f} MB by its shapes: "
          f"{res['B_GBps']:.0f} GB/s achieved")

    if not a.no_model:
        from denseclip_vit_multimodal_amd.config import build_model, load_yaml
        model = build_model(load_yaml("denseclip_cityscapes.yaml"), clip_path_override="").to(dev).eval()
        img = synth_batch(1, H, W, dev, image_dtype=torch.bfloat16)[0]
        segs, depths, win, org = forward_windows(model, img, crop, stride)
        fl = [c for o in org for c in o]
        print(f"model windows: {len(segs)} x seg {tuple(segs[0].shape)} {segs[0].dtype}")
        arms_m = {
            "one_forward": lambda: model.forward_lowres(img),
            "window_forwards": lambda: forward_windows(model, img, crop, stride),
            "window_forwards_3": lambda: forward_windows(model, img, crop, stride, windows_per_forward=3),
            "predict_slide": lambda: predict_slide(model, img, crop, stride),
        }
        tail = lambda: (E.slide_argmax(segs, fl, *win, H, W), E.slide_depth(depths, fl, *win, H, W))  # noqa: E731
        for fn in list(arms_m.values()) + [tail]:
            fn()
        torch.cuda.synchronize()
        tm = {k: [] for k in arms_m}
        tt = []
        for _ in range(max(3, a.rounds // 2)):
            for k, fn in arms_m.items():
                tm[k].append(timed(fn, 1))
            tt.append(timed(tail, a.inner))
        res["model"] = {k: stats(v) for k, v in tm.items()}
        res["model"]["slide_ops"] = stats(tt)
        med = {k: statistics.median(v) for k, v in tm.items()}
        res["model"]["windows_over_one_forward"] = med["window_forwards"] / med["one_forward"]
        res["model"]["slide_ops_share"] = statistics.median(tt) / med["predict_slide"]
        print(f"forward (1 x {H} x {W}): one forward of the whole image median {med['one_forward']:.1f} ms; the "
              f"{len(org)} window forwards {med['window_forwards']:.1f} ms one at a time "
              f"({res['model']['windows_over_one_forward']:.2f} x), {med['window_forwards_3']:.1f} ms three per forward")
        print(f"predict_slide: median {med['predict_slide']:.1f} ms, of which the two slide ops "
              f"{statistics.median(tt):.3f} ms ({100 * res['model']['slide_ops_share']:.2f} %)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
