"""Time the ADE20K batch preparation (csrc/dataade.hip) on the GPU and the same samples through PIL on the host.

    python tools/bench_ade20k_prep.py [--warmup 20] [--iters 100] [--dtype bf16] [--seed 0]

8 synthetic samples of ADE20K-like sizes (683x512, 512x384, 256x341, ... as W x H) to 512 x 512 crops with
parameters from `ade20k_params(RandomState(seed))`:
  (gpu)       torch.ops.dclip_data.ade20k_prepare on planes already on the device: `warmup` calls, then `iters`
              calls between two HIP events, one synchronise at the end;
  (gpu+h2d)   data.prepare_ade20k_batch from the host arrays (packing, the three uploads, the op), wall clock
              around `iters` calls that end in a synchronise;
  (pil)       the reference's per-sample work on the host with PIL itself (resize, resize, crop, label map,
              normalise, as datasets/ade20k.py:74-185 with the drawn parameters), wall clock, where PIL is
              importable (skipped, and said so, where it is not);
the GPU result is first checked against the PIL one (labels equal, image within 1e-6 in f32).  Prints the
figures, then one JSON line.  Reads nothing outside the repository; fixes no threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from denseclip_vit_multimodal_amd import _torch_ops, data  # noqa: E402

SIZES_WH = [(683, 512), (512, 384), (256, 341), (512, 683), (640, 480), (384, 512), (500, 375), (341, 256)]
CROP = (512, 512)


def samples(seed):
    g = np.random.RandomState(seed)
    out = []
    for W, H in SIZES_WH:
        out.append((g.randint(0, 256, (H, W, 3)).astype(np.uint8), g.randint(0, 151, (H, W)).astype(np.uint8)))
    return out


def pil_sample(img, lab, prm, mean, std):
    from PIL import Image
    H1, W1, H2, W2, y0, x0, _ = prm
    a, b = Image.fromarray(img).resize((W1, H1), Image.BILINEAR), Image.fromarray(lab).resize((W1, H1), Image.NEAREST)
    if (H2, W2) != (H1, W1):
        a, b = a.resize((W2, H2), Image.BILINEAR), b.resize((W2, H2), Image.NEAREST)
    box = (x0, y0, x0 + CROP[1], y0 + CROP[0])
    a, b = a.crop(box), b.crop(box)
    lb = np.array(b).astype(np.int64)
    valid = lb > 0
    lb[valid] -= 1
    lb[~valid] = 255
    x = (np.array(a).astype(np.float32) / 255.0 - mean) / std
    return torch.from_numpy(x.transpose(2, 0, 1)), torch.from_numpy(lb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    dev = torch.device("cuda")
    _torch_ops.load()
    smp = samples(a.seed)
    sizes = [s[1].shape for s in smp]
    prm = data.ade20k_params(sizes, CROP, rng=np.random.RandomState(a.seed))
    geom_host, _, _ = data.ade20k_geometry(sizes, prm, CROP)
    img = torch.from_numpy(np.concatenate([s[0].reshape(-1) for s in smp])).to(dev)
    lab = torch.from_numpy(np.concatenate([s[1].reshape(-1) for s in smp])).to(dev)
    geom = geom_host.to(dev)
    mean, std = list(data.IMAGENET_MEAN), list(data.IMAGENET_STD)
    op = torch.ops.dclip_data.ade20k_prepare
    res = {"metric": "ade20k_prepare_ms_per_batch", "B": len(smp), "crop": list(CROP), "dtype": a.dtype,
           "params": prm.tolist(), "ws_bytes": int(torch.ops.dclip_data.ade20k_ws_bytes(geom_host, *CROP))}

    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
        print("PIL is not importable: the host arm and the check against it are skipped")
    if have_pil:
        m, s = np.array(mean), np.array(std)
        ref = [pil_sample(i, l, p, m, s) for (i, l), p in zip(smp, prm.tolist())]
        out, seg = op(img, lab, geom, geom_host, *CROP, mean, std, 255, torch.float32)
        err = float((out.double().cpu() - torch.stack([r[0] for r in ref])).abs().max())
        assert torch.equal(seg.cpu(), torch.stack([r[1] for r in ref])), "labels differ from PIL"
        assert err <= 1e-6, err
        print(f"check against PIL: labels equal, image max abs err {err:.2e}")
        res["pil_version"] = PIL.__version__

    for _ in range(a.warmup):
        op(img, lab, geom, geom_host, *CROP, mean, std, 255, dt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        op(img, lab, geom, geom_host, *CROP, mean, std, 255, dt)
    e1.record()
    torch.cuda.synchronize()
    res["gpu_ms"] = e0.elapsed_time(e1) / a.iters
    print(f"gpu (planes on the device, HIP events): {res['gpu_ms']:.4f} ms per batch of {len(smp)}")

    for _ in range(3):
        data.prepare_ade20k_batch(smp, CROP, prm, dev, out_dtype=dt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        data.prepare_ade20k_batch(smp, CROP, prm, dev, out_dtype=dt)
    torch.cuda.synchronize()
    res["gpu_h2d_ms"] = (time.perf_counter() - t0) * 1e3 / a.iters
    print(f"gpu + packing + upload (wall clock): {res['gpu_h2d_ms']:.4f} ms per batch")

    if have_pil:
        n = max(1, a.iters // 10)
        pil_sample(*smp[0], prm[0].tolist(), m, s)
        t0 = time.perf_counter()
        for _ in range(n):
            for (i, l), p in zip(smp, prm.tolist()):
                pil_sample(i, l, p, m, s)
        res["pil_ms"] = (time.perf_counter() - t0) * 1e3 / n
        print(f"PIL {PIL.__version__} on one host core (wall clock, {n} rounds): {res['pil_ms']:.3f} ms per batch")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
