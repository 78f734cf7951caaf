"""Time the optimizer step of the ViT-B/16 DenseCLIP parameter set, native against torch, in one process.

    python tools/bench_optim.py [--rounds 12] [--inner 10] [--mode F] [--max-norm 1.0]

One small-image train step (2 x 256 x 512, bf16) populates the gradients and the 16-bit weight
caches; then, on those gradients, interleaved ABBA, with and without clipping:
  (A) the sequence the package ran before train.FusedAdamW for the same semantics: torch's fused
      AdamW through train.step_unless_nonfinite, followed by ops.refresh_weight_copies (the
      optimizer-step hook); with clipping also torch.nn.utils.clip_grad_norm_ (a norm pass and a
      multiply pass over every gradient) and the gradients' inf-norm pass (check_grads=True);
  (B) train.FusedAdamW through the same train.step_unless_nonfinite: the norm pass (with clipping
      only) and the update pass of csrc/optim.hip, which writes the weight copies itself.
Both optimizers step the same parameters on the same gradients (the values drift; the work does
not).  Times are device-event times of `inner` back-to-back steps ending in a device synchronise, so
they hold whichever of the host's issue time and the device's run time is longer.  Prints per-arm
median / min / max over the rounds, the byte model from the shapes (28 B per parameter for the
update's fp32 reads and writes + 2 B per copy element — about 32 B per parameter in all — and 4 B per
parameter for the norm pass) and those bytes over (B)'s step time, then one JSON line.  That rate is
a whole-step figure, not a kernel's bandwidth: no kernel trace separates host from device time here.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from denseclip_vit_multimodal_amd import ops, train  # noqa: E402


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
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--mode", choices=["F", "R"], default="F")
    ap.add_argument("--max-norm", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim needs a GPU (no CPU fallback, no timing without one)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.make_model(dev, a.mode).train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt_a = train.make_optimizer(params)
    opt_ac = train.make_optimizer(params)
    opt_b = train.FusedAdamW(params, lr=2e-5, weight_decay=0.01)
    opt_bc = train.FusedAdamW(params, lr=2e-5, weight_decay=0.01, max_norm=a.max_norm)
    batch = train.synth_batch(2, 256, 512, dev, 0, image_dtype=torch.bfloat16)
    loss = train.train_step(model, opt_a, batch)  # gradients, weight caches, the refresh descriptor
    torch.cuda.synchronize()
    stepped = [p for p in params if p.grad is not None]
    n = sum(p.numel() for p in stepped)
    copies = sum(v.numel() for items in ops.collect_weight_copies(stepped).values()
                 for it in items for v in (it[3], it[4]) if v is not None)

    def arm_a():
        train.step_unless_nonfinite(opt_a, loss, check_grads=False)

    def arm_a_clip():
        torch.nn.utils.clip_grad_norm_(stepped, a.max_norm)
        train.step_unless_nonfinite(opt_ac, loss, check_grads=True)

    def arm_b():
        train.step_unless_nonfinite(opt_b, loss, check_grads=False)

    def arm_b_clip():
        train.step_unless_nonfinite(opt_bc, loss, check_grads=True)

    arms = {"A": arm_a, "B": arm_b, "A.clip": arm_a_clip, "B.clip": arm_b_clip}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for r in range(a.rounds):
        for pair in (("A", "B"), ("A.clip", "B.clip")):
            x, y = pair if r % 2 == 0 else pair[::-1]
            for k in (x, y, y, x):
                times[k].append(timed(arms[k], a.inner))
    stat = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}
    print(f"{len(stepped)} parameters with gradients, {n / 1e6:.1f} M elements, {copies / 1e6:.1f} M copy elements; "
          f"mode {a.mode}, total_norm {float(opt_bc.last_total_norm):.4g}, steps {float(opt_bc.step_count):.0f}")
    for k, s in stat.items():
        print(f"{k:7s} median {s['median_ms']:8.3f} ms   min {s['min_ms']:8.3f}   max {s['max_ms']:8.3f}   "
              f"({len(times[k])} x {a.inner} steps)")
    upd_bytes, norm_bytes = 28 * n + 2 * copies, 4 * n  # p, g, m, v read + p, m, v written; the copies; g read
    res = {"mode": a.mode, "params": len(stepped), "elements": n, "copy_elements": copies, "times": stat,
           "ratio_A_over_B": stat["A"]["median_ms"] / stat["B"]["median_ms"],
           "ratio_Aclip_over_Bclip": stat["A.clip"]["median_ms"] / stat["B.clip"]["median_ms"],
           "B_bytes": upd_bytes, "B_GBps": upd_bytes / stat["B"]["median_ms"] / 1e6,
           "Bclip_bytes": upd_bytes + norm_bytes,
           "Bclip_GBps": (upd_bytes + norm_bytes) / stat["B.clip"]["median_ms"] / 1e6}
    print(f"(B) moves {upd_bytes / 1e9:.3f} GB by its shapes ({res['B_GBps']:.0f} GB/s over the step's time), with "
          f"clipping {(upd_bytes + norm_bytes) / 1e9:.3f} GB ({res['Bclip_GBps']:.0f} GB/s); A / B = "
          f"{res['ratio_A_over_B']:.2f}, A.clip / B.clip = {res['ratio_Aclip_over_Bclip']:.2f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
