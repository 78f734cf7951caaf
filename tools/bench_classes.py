"""Time the fused head paths at K = 150 classes against the torch sequence they replace, in one process.

    python tools/bench_classes.py [--rounds 10] [--inner 20] [--dtype bf16] [--classes 150]

At two shapes, B = 8, 32 x 32 -> 512 x 512 (ADE20K's crop) and B = 2, 64 x 128 -> 1024 x 2048, with
alternating arms (ABBA / BAAB by round):
  CE    (A) F.interpolate + F.cross_entropy + backward on the low-res logits held in fp32 (cast outside
            the timed calls; the (B, K, H, W) fp32 logits and their gradient are materialised);
        (B) ops.UpsampleCEFn forward + backward (csrc/classes.hip, dclip_upsample_ce_classes);
  eval  (A) F.interpolate + argmax + bincount confusion matrix + F.cross_entropy(sum);
        (B) Evaluator(num_classes=K).update (dclip_upsample_eval_seg_classes).
Every timing is a device-event time of `inner` back-to-back calls that ends in a device synchronise;
every arm is warmed at its shape first and the two arms are checked against each other before anything
is timed.  Peak scratch is torch's peak allocated bytes over one call above what was allocated before
it (inputs excluded, outputs and workspaces included).  Prints per-arm median / min / max over the
rounds and the ratios, then one JSON line.  Reads nothing outside the repository; fixes no threshold.
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
from denseclip_vit_multimodal_amd.evaluate import Evaluator  # noqa: E402

SHAPES = [(8, 32, 32, 512, 512), (2, 64, 128, 1024, 2048)]


def ce_unfused(low32, lab):
    x = low32.detach().requires_grad_(True)
    loss = F.cross_entropy(F.interpolate(x, size=lab.shape[-2:], mode="bilinear", align_corners=False), lab,
                           ignore_index=255)
    loss.backward()
    return loss.detach(), x.grad


def ce_fused(low, lab):
    x = low.detach().requires_grad_(True)
    loss = ops.UpsampleCEFn.apply(x, lab, 255)
    loss.backward()
    return loss.detach(), x.grad


def eval_unfused(low32, lab, K):
    up = F.interpolate(low32, size=lab.shape[-2:], mode="bilinear", align_corners=False)
    pred = up.argmax(1)
    valid = (lab != 255) & (lab >= 0) & (lab < K)
    idx = torch.where(valid, lab * K + pred, torch.full_like(lab, K * K))
    cm = torch.bincount(idx.view(-1), minlength=K * K + 1)[:K * K].view(K, K)
    return cm, F.cross_entropy(up, lab, ignore_index=255, reduction="sum")


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def peak_scratch(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classes needs a GPU (no CPU fallback, no timing without one)")
    dev = torch.device("cuda")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    K = a.classes
    results = []
    for (B, h, w, H, W) in SHAPES:
        g = torch.Generator().manual_seed(1234)
        low = (torch.randn(B, K, h, w, generator=g) * 3).to(dev).to(dt)
        g = torch.Generator().manual_seed(1235)
        lab = torch.randint(0, K, (B, H, W), generator=g)
        lab[torch.rand(B, H, W, generator=g) < 0.1] = 255
        lab = lab.to(dev)
        low32 = low.float()  # arm A's input: the unfused heads hand fp32 logits to the resize
        ev = Evaluator(num_classes=K, device=dev)

        def eval_fused():
            with torch.no_grad():
                ev.update(low, None, lab)

        def eval_a():
            with torch.no_grad():
                return eval_unfused(low32, lab, K)

        # the arms agree before anything is timed
        (la, ga), (lb, gb) = ce_unfused(low32, lab), ce_fused(low, lab)
        ce_loss_rel = abs(float(la) - float(lb)) / abs(float(la))
        ce_grad_rel = float((ga.double() - gb.double()).norm() / ga.double().norm())
        cm_a, sum_a = eval_a()
        eval_fused()
        torch.cuda.synchronize()
        cm_diff = int((ev.cm - cm_a).abs().sum())
        sum_rel = abs(float(ev.ce_sums[0]) - float(sum_a)) / abs(float(sum_a))
        print(f"[{B} x {K} x {h} x {w} -> {H} x {W}] agreement: CE loss rel {ce_loss_rel:.2e}, gradient rel "
              f"{ce_grad_rel:.2e}; confusion-matrix L1 difference {cm_diff} of {int(ev.cm.sum())} pixels, CE sum rel "
              f"{sum_rel:.2e}")
        del la, ga, lb, gb, cm_a, sum_a
        arms = {"ce.A": lambda: ce_unfused(low32, lab), "ce.B": lambda: ce_fused(low, lab), "eval.A": eval_a,
                "eval.B": eval_fused}
        for fn in arms.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        scratch = {k: peak_scratch(fn) for k, fn in arms.items()}
        times = {k: [] for k in arms}
        for r in range(a.rounds):
            for pair in ("ce", "eval"):
                order = ["A", "B", "B", "A"] if r % 2 == 0 else ["B", "A", "A", "B"]
                for arm in order:
                    times[f"{pair}.{arm}"].append(timed(arms[f"{pair}.{arm}"], a.inner))
        stat = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                    "peak_scratch_MiB": scratch[k] / 2 ** 20} for k, v in times.items()}
        for k, s in stat.items():
            print(f"  {k:7s} median {s['median_ms']:9.3f} ms   min {s['min_ms']:9.3f}   max {s['max_ms']:9.3f}   "
                  f"peak scratch {s['peak_scratch_MiB']:9.1f} MiB   ({len(times[k])} x {a.inner} calls)")
        res = {"shape": [B, K, h, w, H, W], "dtype": a.dtype, "times": stat,
               "ce_A_over_B": stat["ce.A"]["median_ms"] / stat["ce.B"]["median_ms"],
               "eval_A_over_B": stat["eval.A"]["median_ms"] / stat["eval.B"]["median_ms"],
               "ce_loss_rel": ce_loss_rel, "ce_grad_rel": ce_grad_rel, "cm_l1_diff": cm_diff, "ce_sum_rel": sum_rel}
        print(f"  CE A / B = {res['ce_A_over_B']:.2f}, eval A / B = {res['eval_A_over_B']:.2f}")
        results.append(res)
        del low, low32, lab, ev
        torch.cuda.empty_cache()
    print(json.dumps({"classes": K, "results": results}))


if __name__ == "__main__":
    main()
