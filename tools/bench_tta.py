"""Time the multi-scale + flip ensemble of one validation update, fused against unfused, in one process.

    python tools/bench_tta.py [--batch 1] [--rounds 10] [--inner 3] [--dtype bf16] [--average logits] [--no-model]

At batch x 1024 x 2048 with the 12 views of evaluate.TTA_SCALES + flip, whose low-res maps have the
sizes the benchmark model (ViT-B/16, heads at 1/16 of the view) gives them: 32x64, 48x96, 64x128,
80x160, 96x192 and 112x224, each plain and flipped, random values.  Interleaved ABBA:
  (A) the unfused torch sequence on those maps: per view ops.upsample to the label size and .flip(-1)
      for a flipped view (a full-size fp32 tensor per view), torch.stack, .mean(0) (a softmax per view
      first under --average probs), argmax, a bincount confusion matrix and the CE sum; likewise the
      depth: per-view ops.upsample + flip, stack, mean, then the 12 sums as masked torch reductions;
  (B) one Evaluator.update_views (csrc/headensemble.hip: one fused launch per head).
Every arm ends in a device synchronise; times are device-event times of `inner` back-to-back calls.
Prints per-arm median / min / max over the rounds, the ratio, (B)'s two ops on their own, the peak
memory each arm allocates on top of its inputs, and, unless --no-model, the time of a whole
evaluate.predict_tta of the benchmark model on one image beside the time of its ensemble ops alone
(the view forwards are the rest).  Ends with one JSON line.
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
from denseclip_vit_multimodal_amd.evaluate import TTA_SCALES, Evaluator, _E, forward_views, predict_tta  # noqa: E402
from denseclip_vit_multimodal_amd.train import synth_batch  # noqa: E402

K = 19
PATCH = 16


def full_size_mean(views, flips, size, probs=False):
    outs = []
    for v, f in zip(views, flips):
        u = ops.upsample(v, size)
        if f:
            u = u.flip(-1)
        outs.append(torch.softmax(u, dim=1) if probs else u)
    return torch.stack(outs).mean(0)


def unfused(seg_views, depth_views, flips, seg, depth, mask, size, probs, dmin=1e-3, dmax=80.0, eps=1e-6):
    up = full_size_mean(seg_views, flips, size, probs)
    pred = up.argmax(1)
    valid = (seg != 255) & (seg >= 0) & (seg < K)
    idx = torch.where(valid, seg * K + pred, torch.full_like(seg, K * K))
    cm = torch.bincount(idx.view(-1), minlength=K * K + 1)[:K * K].view(K, K)
    if probs:
        ce = F.nll_loss(torch.log(up), seg, ignore_index=255, reduction="sum")
    else:
        ce = F.cross_entropy(up, seg, ignore_index=255, reduction="sum")
    d = full_size_mean(depth_views, flips, size)
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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--average", choices=["logits", "probs"], default="logits")
    ap.add_argument("--no-model", action="store_true", help="skip the whole-model predict_tta timing")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta needs a GPU (no CPU fallback, no timing without one)")
    dev = torch.device("cuda")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    B, H, W = a.batch, a.height, a.width
    probs = a.average == "probs"
    geo = [(int(H * s + 0.5) // PATCH, int(W * s + 0.5) // PATCH, f) for s in TTA_SCALES for f in (0, 1)]
    flips = [f for _, _, f in geo]
    g = torch.Generator().manual_seed(1234)
    seg_views = [(torch.randn(B, K, h, w, generator=g) * 3).to(dev).to(dt) for h, w, _ in geo]
    depth_views = [(0.5 + 59.5 * torch.rand(B, 1, h, w, generator=g)).to(dev).to(dt) for h, w, _ in geo]
    _, seg, depth, mask = synth_batch(B, H, W, dev, image_dtype=torch.float32)
    mask_u8 = mask.to(torch.uint8)
    tg, mk = depth.reshape(B, H, W), mask_u8.reshape(B, H, W)
    ev = Evaluator(device=dev)
    E = _E()
    print(f"views (h, w, flip): {geo}")

    arms = {
        "A": lambda: unfused(seg_views, depth_views, flips, seg, depth, mask, (H, W), probs),
        "B": lambda: ev.update_views(seg_views, depth_views, flips, seg, depth, mask_u8, average=a.average),
        "B.seg": lambda: E.ensemble_seg_update(seg_views, flips, seg, 255, probs, ev.cm, ev.ce_sums, False),
        "B.depth": lambda: E.ensemble_depth_update(depth_views, flips, tg, mk, 1e-3, 80.0, True, 1e-6, ev.depth_sums,
                                                   False),
    }
    # the two paths agree before anything is timed
    pred_a, cm_a, ce_a, sums_a = arms["A"]()
    pred_b = E.ensemble_argmax(seg_views, flips, H, W, probs)
    ev.update_views(seg_views, depth_views, flips, seg, depth, mask_u8, average=a.average)
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
    low_bytes = sum(v.numel() * v.element_size() for v in seg_views + depth_views)
    bytes_b = px * (seg.element_size() + 4 + 1) + low_bytes
    res = {"shape": [B, H, W], "views": geo, "dtype": a.dtype, "average": a.average, "times": stat,
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
        segs, depths, fl = forward_views(model, img)
        print(f"model views: seg {[tuple(s.shape[-2:]) for s in segs]} {segs[0].dtype}")
        whole = lambda: predict_tta(model, img, average=a.average)  # noqa: E731
        tail = lambda: (E.ensemble_argmax(segs, fl, H, W, probs), E.ensemble_depth(depths, fl, H, W))  # noqa: E731
        for fn in (whole, tail):
            fn()
        torch.cuda.synchronize()
        tw, tt = [], []
        for _ in range(max(3, a.rounds // 2)):
            tw.append(timed(whole, 1))
            tt.append(timed(tail, a.inner))
        res["predict_tta"] = {"whole": stats(tw), "ensemble_ops": stats(tt),
                              "ensemble_share": statistics.median(tt) / statistics.median(tw)}
        print(f"predict_tta (1 x {H} x {W}, 12 views): median {statistics.median(tw):.1f} ms, of which the two "
              f"ensemble ops {statistics.median(tt):.3f} ms ({100 * res['predict_tta']['ensemble_share']:.2f} %)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
