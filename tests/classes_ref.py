"""Shared inputs and CPU references of the any-class-count tests (test_classes_cpu.py,
test_gpu_classes.py): eval_ref.py's generators with the class count as an argument (eval_ref has
K = 19 at module level), the fp64 resize and the ambiguity threshold taken from it unchanged.

    python tests/classes_ref.py      prints the departure of torch's fp32 evaluation of the CE sum from
                                     the fp64 one over the GPU test's cases (REF_FP32_DEPARTURE_CE)
"""
import functools

import torch
import torch.nn.functional as F

import eval_ref

IGNORE = 255
KS = (2, 33, 150, 256)
# (B, h, w, H, W): the workload's x16; an odd scale where w crosses a 32-column chunk and W spans three
# tiles; wide; one low-res pixel; the identity; a scale near 1 whose K-channel patch does not fit LDS
SHAPES = [(2, 8, 16, 128, 256), (1, 5, 37, 43, 301), (1, 3, 70, 17, 1000), (1, 1, 1, 7, 9), (1, 6, 6, 6, 6),
          (1, 11, 66, 12, 68)]
SHAPE_IDS = ["x16", "odd", "wide", "one_pixel", "identity", "near_one"]
LOWS = (torch.bfloat16, torch.float16, torch.float32)
LABS = (torch.int64, torch.uint8)

resize = eval_ref.resize
tau = eval_ref.tau
rel = eval_ref.rel


@functools.lru_cache(maxsize=None)
def logits(B, K, h, w, dtype=torch.float32):
    g = torch.Generator().manual_seed(1234)
    return (torch.randn(B, K, h, w, generator=g) * 3).to(dtype)


@functools.lru_cache(maxsize=None)
def labels(B, K, H, W, dtype=torch.int64):
    """~10 % ignore (255), ~0.5 % in K..254 (where K < 255); the wider dtypes also hold negatives and
    values past 255, as eval_ref.labels"""
    g = torch.Generator().manual_seed(1235)
    lab = torch.randint(0, K, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    lab[r < 0.1] = IGNORE
    if K < 255:
        odd = (r >= 0.1) & (r < 0.105)
        lab[odd] = torch.randint(K, 255, (B, H, W), generator=g)[odd]
    if dtype != torch.uint8:
        wide = (r >= 0.105) & (r < 0.11)
        lab[wide] = torch.tensor([-1, 256, 1000, -300])[torch.randint(0, 4, (B, H, W), generator=g)][wide]
    return lab.to(dtype)


def valid_labels(lab, K, ignore=IGNORE):
    lab = lab.long()
    return (lab != ignore) & (lab >= 0) & (lab < K)


def ce_sum(up, lab, K, ignore=IGNORE):
    """sum over the valid pixels of -log softmax(up)[label] in up's dtype (F.cross_entropy, as the trainer)"""
    lab = lab.long()
    lab = torch.where(valid_labels(lab, K, ignore), lab, torch.full_like(lab, -100))
    return float(F.cross_entropy(up, lab, ignore_index=-100, reduction="sum"))


def fp32_departure(ks=KS, shapes=SHAPES, lows=LOWS, labs=LABS):
    """max over the cases of |CE sum of the fp32 resize in fp32 - CE sum of the fp64 resize in fp64| / the latter"""
    worst = 0.0
    for K in ks:
        for (B, h, w, H, W) in shapes:
            for low in lows:
                L = logits(B, K, h, w, low)
                u64, u32 = resize(L, H, W), resize(L, H, W, torch.float32)
                for labdt in labs:
                    lab = labels(B, K, H, W, labdt)
                    worst = max(worst, rel(ce_sum(u32, lab, K), ce_sum(u64, lab, K)))
    return worst


if __name__ == "__main__":
    torch.set_num_threads(8)
    print(f"REF_FP32_DEPARTURE_CE = {fp32_departure():.4e}")
