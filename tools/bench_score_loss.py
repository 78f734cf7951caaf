"""Time the identity-head branch: the score map's backward (csrc/scoregrad.hip) alone, the whole branch forward
+ backward, and one mode-F train step with the head on and off, in one process.

    python tools/bench_score_loss.py [--rounds 8] [--inner 5] [--no-step]

At B = 8, h x w = 64 x 128, C = 512 (the pixel embeddings of 1024 x 2048 images at patch 16), labels 1024 x
2048, tau = 0.07, for K = 19 and K = 150:
  bwd        ops.score_map_bwd alone (bf16 v, bf16 dv, ds f32): the three launches of dclip_score_map_bwd;
  bwd.torch  what replaces it in torch: autograd's backward of F.normalize x2 + einsum on an f32 copy of v (the
             backward only: the forward graph is built outside the timed region);
  branch     ops.ScoreMapFn(scale 1 / tau) + ops.upsample_cross_entropy, forward + backward;
  torch      normalize x2, einsum, / tau, F.interpolate(bilinear), F.cross_entropy, forward + backward, on f32.
Then one mode-F train step of ViT-B/16 at the headline shape (8 x 1024 x 2048, bf16 images, fused head losses)
with the identity head off and on (eager steps, the same batch).
Every timing is a device-event time of `inner` back-to-back calls that ends in a device synchronise; every arm
is warmed first, the HIP and torch arms are checked against each other before anything is timed (on as many
images as keep torch's resized logits below 2^31 elements, which its kernels need: 6 of the 8 at K = 150, where
the timed torch arm's values are therefore not to be trusted, only its time), and the arms run in an order that
reverses every round.  Prints per-arm median / min / max, then one JSON line.  Reads
nothing outside the repository; fixes no threshold.
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

B, H_LOW, W_LOW, C, H, W, TAU = 8, 64, 128, 512, 1024, 2048, 0.07


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def run_arms(arms, rounds, inner):
    for fn in arms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for r in range(rounds):
        order = list(arms) if r % 2 == 0 else list(arms)[::-1]
        for k in order + order[::-1]:
            times[k].append(timed(arms[k], inner))
    out = {k: stats(v) for k, v in times.items()}
    for k, s in out.items():
        print(f"  {k:10s} median {s['median_ms']:9.3f} ms   min {s['min_ms']:9.3f}   max {s['max_ms']:9.3f}   "
              f"({len(times[k])} x {inner} calls)")
    return out


def branch_case(K, dev, rounds, inner):
    HW = H_LOW * W_LOW
    g = torch.Generator().manual_seed(1234 + K)
    v = torch.randn(B * HW, C, generator=g).to(dev).to(torch.bfloat16)
    vmap = v.view(B, H_LOW, W_LOW, C).permute(0, 3, 1, 2)
    text = (torch.randn(B, K, C, generator=g) * 0.5).to(dev)
    ds = (torch.randn(B, K, HW, generator=g) * 1e-6).to(dev)
    lab = torch.randint(0, K, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = 255
    lab = lab.to(dev)
    v32 = vmap.float().contiguous()

    def torch_score(x, t):
        return torch.einsum("bchw,bkc->bkhw", F.normalize(x, dim=1, p=2), F.normalize(t, dim=2, p=2))

    def hip_branch():
        x, t = vmap.detach().requires_grad_(True), text.detach().requires_grad_(True)
        loss = ops.upsample_cross_entropy(ops.ScoreMapFn.apply(x, t, 1e-12, 1.0 / TAU), lab, ignore_index=255)
        loss.backward()
        return loss.detach(), x.grad, t.grad

    def torch_branch():
        x, t = v32.detach().requires_grad_(True), text.detach().requires_grad_(True)
        up = F.interpolate(torch_score(x, t) / TAU, size=(H, W), mode="bilinear", align_corners=False)
        loss = F.cross_entropy(up, lab, ignore_index=255)
        loss.backward()
        return loss.detach(), x.grad, t.grad

    # the torch backward of the score map alone: a fresh graph per call, built outside the timed region
    graphs = []

    def prime(n):
        for _ in range(n):
            x, t = v32.detach().requires_grad_(True), text.detach().requires_grad_(True)
            graphs.append((torch_score(x, t), x, t))

    def torch_bwd():
        s, x, t = graphs.pop()
        s.backward(ds.view(B, K, H_LOW, W_LOW))

    # the arms agree before anything is timed: on as many images as keep the resized logits below 2^31 elements
    # (torch's resize / cross-entropy kernels index with 32 bits; 8 x 150 x 1024 x 2048 is 2.5e9)
    nb = max(1, min(B, (2 ** 31 - 1) // (K * H * W)))

    def sub(fn):
        nonlocal vmap, v32, text, lab
        keep = (vmap, v32, text, lab)
        vmap, v32, text, lab = vmap[:nb], v32[:nb], text[:nb], lab[:nb]
        try:
            return fn()
        finally:
            vmap, v32, text, lab = keep

    (lh, gvh, gth), (lt, gvt, gtt) = sub(hip_branch), sub(torch_branch)
    agree = (abs(float(lh) - float(lt)) / abs(float(lt)),
             float((gvh.double() - gvt.double()).norm() / gvt.double().norm()),
             float((gth.double() - gtt.double()).norm() / gtt.double().norm()))
    print(f"[K = {K}] branch agreement HIP vs torch f32 on {nb} image(s) (loss rel, d map rel, d text rel; the HIP "
          f"forward rounds the text rows to bf16 for its MFMA and stores d map in bf16): "
          f"{agree[0]:.2e} {agree[1]:.2e} {agree[2]:.2e}")
    del lh, gvh, gth, lt, gvt, gtt
    arms = {"bwd": lambda: ops.score_map_bwd(v, text, ds, B, HW), "branch": hip_branch,
            "torch": torch_branch}
    res = run_arms(arms, rounds, inner)
    # the torch backward alone, its graphs primed per timing
    tb = []
    for _ in range(2 * rounds):
        prime(inner)
        torch.cuda.synchronize()
        tb.append(timed(torch_bwd, inner))
    res["bwd.torch"] = stats(tb)
    s = res["bwd.torch"]
    print(f"  {'bwd.torch':10s} median {s['median_ms']:9.3f} ms   min {s['min_ms']:9.3f}   max {s['max_ms']:9.3f}")
    moved = (B * HW * C * 2 * 2) / 2 ** 20  # one read of v, one write of dv, bf16
    print(f"  bwd: {moved:.0f} MiB of v + dv -> {moved * 2 ** 20 / (res['bwd']['median_ms'] * 1e-3) / 1e12:.2f} TB/s "
          f"if it were one read and one write; torch / HIP: bwd {res['bwd.torch']['median_ms'] / res['bwd']['median_ms']:.2f}, "
          f"branch {res['torch']['median_ms'] / res['branch']['median_ms']:.2f}")
    return {"K": K, "times": res, "agreement": agree}


def step_case(dev, rounds):
    from denseclip_vit_multimodal_amd.config import build_model, load_yaml
    from denseclip_vit_multimodal_amd.train import (freeze_for_mode, identity_loss_weight, make_optimizer, synth_batch,
                                                    train_step)
    batch = synth_batch(B, H, W, dev, 0)
    out = {}
    for name in ("head_off", "head_on"):
        cfg = load_yaml("denseclip_cityscapes.yaml")
        if name == "head_on":
            cfg["model"]["identity_head"] = dict(type="IdentityHead", loss_weight=0.4)
        torch.manual_seed(0)
        m = build_model(cfg, clip_path_override="").to(dev).train()
        m.fused_head_loss = True
        opt = make_optimizer(freeze_for_mode(m, "F"))
        wt = identity_loss_weight(m)
        for _ in range(3):
            train_step(m, opt, batch, identity_weight=wt)
        torch.cuda.synchronize()
        t = [timed(lambda: train_step(m, opt, batch, identity_weight=wt), 2) for _ in range(rounds)]
        out[name] = stats(t)
        s = out[name]
        print(f"  step {name:9s} median {s['median_ms']:9.3f} ms   min {s['min_ms']:9.3f}   max {s['max_ms']:9.3f}")
        del m, opt
        torch.cuda.empty_cache()
    out["delta_ms"] = out["head_on"]["median_ms"] - out["head_off"]["median_ms"]
    print(f"  head on - head off = {out['delta_ms']:+.3f} ms per step")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the two train-step timings")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score_loss needs a GPU (no CPU fallback, no timing without one)")
    dev = torch.device("cuda")
    results = {"branch": [branch_case(K, dev, a.rounds, a.inner) for K in (19, 150)]}
    torch.cuda.empty_cache()
    if not a.no_step:
        print(f"[mode F train step, ViT-B/16, {B} x {H} x {W} bf16]")
        results["step"] = step_case(dev, a.rounds)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
