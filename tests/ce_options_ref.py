"""Shared inputs and fp64 references of the optioned fused CE's tests (test_ce_options_cpu.py,
test_gpu_ce_options.py): classes_ref's logits and labels, seeded class weights in [0.25, 4], a seeded
per-pixel weight with negatives, and F.interpolate + F.cross_entropy (weight, label_smoothing,
reduction="none") with autograd as the reference, in any dtype.

    python tests/ce_options_ref.py    prints the departures of torch's own fp32 evaluation from the fp64
                                      one over the GPU test's cases (the REF_FP32_* constants of
                                      test_ce_options_cpu.py) and the OHEM cases' kept / ambiguous shares
"""
import functools

import torch
import torch.nn.functional as F

import classes_ref as R

IGNORE = R.IGNORE
EPS = 0.1
KS = (19, 2, 33, 150, 256)
SHAPE_IDS = ["x16", "odd", "one_pixel", "identity", "near_one"]
SHAPES = [R.SHAPES[R.SHAPE_IDS.index(s)] for s in SHAPE_IDS]
# every K x shape at bf16 / int64; the three low dtypes with uint8 labels on x16 and odd only
CASES = [(K, s, torch.bfloat16, torch.int64) for K in KS for s in range(len(SHAPES))] + \
        [(K, s, low, torch.uint8) for K in KS for s in (0, 1) for low in R.LOWS]
# the option sets of the fp64 comparison: (class weights, smoothing, pixel weights)
OPTIONS = {"weights": (True, 0.0, False), "smooth": (False, EPS, False), "all": (True, EPS, True)}


def case_id(K, si, low, labdt):
    return f"K{K}-{SHAPE_IDS[si]}-{str(low)[6:]}-{str(labdt)[6:]}"


@functools.lru_cache(maxsize=None)
def class_weight(K):
    g = torch.Generator().manual_seed(1240 + K)
    return 0.25 + 3.75 * torch.rand(K, generator=g)


@functools.lru_cache(maxsize=None)
def pixel_weight(B, H, W):
    """any finite float: N(0.5, 1), about 30 % negative"""
    g = torch.Generator().manual_seed(1241)
    return 0.5 + torch.randn(B, H, W, generator=g)


def inputs(K, si, low, labdt, options="all"):
    """(logits, labels, class weights or None, smoothing, pixel weights or None) of a case"""
    B, h, w, H, W = SHAPES[si]
    cw, eps, pw = OPTIONS[options] if isinstance(options, str) else options
    return (R.logits(B, K, h, w, low), R.labels(B, K, H, W, labdt), class_weight(K) if cw else None, eps,
            pixel_weight(B, H, W) if pw else None)


def reference(L, lab, weight=None, eps=0.0, q=None, dtype=torch.float64, grad=True):
    """{sum0: sum q l, sum1: sum q w_t, count, pixel_loss (B, H, W), grad of sum0 wrt the low-res logits} of
    F.cross_entropy(F.interpolate(L), ...) evaluated in `dtype` on the values L holds; a label that is
    the ignore index or outside [0, K) is not valid"""
    K = L.shape[1]
    x = L.detach().to(dtype).clone().requires_grad_(grad)
    up = F.interpolate(x, size=lab.shape[-2:], mode="bilinear", align_corners=False)
    valid = R.valid_labels(lab, K)
    t = torch.where(valid, lab.long(), torch.full_like(lab.long(), -100))
    w = None if weight is None else weight.to(dtype)
    pl = F.cross_entropy(up, t, weight=w, ignore_index=-100, label_smoothing=eps, reduction="none")
    qq = torch.ones_like(pl) if q is None else q.to(dtype)
    wt = valid.to(dtype) if w is None else w[t.clamp(min=0)] * valid
    s0 = (qq * pl).sum()
    if grad:
        s0.backward()
    return {"sum0": float(s0.detach()), "sum1": float((qq * wt).sum()), "count": int(valid.sum()),
            "pixel_loss": pl.detach(), "grad": x.grad, "valid": valid}


def target_prob(L, lab, dtype=torch.float64):
    """softmax(up(L))[label] at the valid pixels (1 elsewhere): OHEM's p_t, from the plain loss"""
    return torch.exp(-reference(L, lab, dtype=dtype, grad=False)["pixel_loss"])


# ----------------------------------------------------------------------------- OHEM
# (thresh, min_kept per image as a share of the image's pixels): the threshold is `thresh` itself; the
# k-th smallest p_t decides
OHEM_RULES = {"thresh": (0.7, 0.0005), "kth": (0.05, 0.35)}
OHEM_KS = (19, 150)
OHEM_SHAPES = (0, 1, 4)  # x16, odd, near_one
OHEM_SCALE = 2.0         # the logits are scaled by this: the fp64 reference then keeps 10 % .. 90 %


@functools.lru_cache(maxsize=None)
def ohem_inputs(K, si, low=torch.bfloat16):
    """(logits, labels): the labels are the argmax of the fp64 resize on about 70 % of the valid pixels"""
    B, h, w, H, W = SHAPES[si]
    L = (R.logits(B, K, h, w) * OHEM_SCALE).to(low)
    lab = R.labels(B, K, H, W).clone()
    u = F.interpolate(L.double(), size=(H, W), mode="bilinear", align_corners=False)
    g = torch.Generator().manual_seed(1242)
    pick = R.valid_labels(lab, K) & (torch.rand(B, H, W, generator=g) < 0.7)
    lab[pick] = u.argmax(1)[pick]
    return L, lab


def ohem_rule(rule, si):
    B, h, w, H, W = SHAPES[si]
    thresh, share = OHEM_RULES[rule]
    return thresh, max(1, int(share * H * W))


def ohem_literal(p_t, valid, thresh, batch_kept):
    """the rule restated with a host-side sort: (keep mask, threshold)"""
    vals = sorted(p_t[valid].tolist())
    if not vals:
        return torch.zeros_like(valid), None
    threshold = max(vals[min(batch_kept, len(vals) - 1)], thresh)
    return valid & (p_t < threshold), threshold


def departures():
    """(loss sum, relative), (pixel loss, max abs / the case's largest pixel loss), (exp(-l) against p_t, abs),
    (gradient of sum q l wrt the low-res logits, norm-wise relative) of torch's fp32 evaluation from the
    fp64 one, maximised over CASES x OPTIONS"""
    d_sum = d_pix = d_p = d_grad = 0.0
    for K, si, low, labdt in CASES:
        for name in OPTIONS:
            L, lab, cw, eps, q = inputs(K, si, low, labdt, name)
            r64, r32 = reference(L, lab, cw, eps, q), reference(L, lab, cw, eps, q, torch.float32)
            d_sum = max(d_sum, R.rel(r32["sum0"], r64["sum0"]), R.rel(r32["sum1"], r64["sum1"]))
            d_pix = max(d_pix, float((r32["pixel_loss"].double() - r64["pixel_loss"]).abs().max())
                        / float(r64["pixel_loss"].max()))
            d_grad = max(d_grad, float((r32["grad"].double() - r64["grad"]).norm() / r64["grad"].norm()))
        L, lab = R.logits(*SHAPES[si][:1], K, *SHAPES[si][1:3], low), R.labels(SHAPES[si][0], K, *SHAPES[si][3:], labdt)
        d_p = max(d_p, float((target_prob(L, lab, torch.float32).double() - target_prob(L, lab)).abs().max()))
    for K in OHEM_KS:
        for si in OHEM_SHAPES:
            L, lab = ohem_inputs(K, si)
            d_p = max(d_p, float((target_prob(L, lab, torch.float32).double() - target_prob(L, lab)).abs().max()))
    return d_sum, d_pix, d_p, d_grad


if __name__ == "__main__":
    torch.set_num_threads(8)
    d_sum, d_pix, d_p, d_grad = departures()
    print(f"REF_FP32_DEPARTURE_SUM = {d_sum:.4e}\nREF_FP32_DEPARTURE_PIXEL = {d_pix:.4e}\n"
          f"REF_FP32_DEPARTURE_PT = {d_p:.4e}\nREF_FP32_DEPARTURE_GRAD = {d_grad:.4e}")
    for K in OHEM_KS:
        for si in OHEM_SHAPES:
            L, lab = ohem_inputs(K, si)
            p, valid = target_prob(L, lab), R.valid_labels(lab, K)
            for rule in OHEM_RULES:
                thresh, kept = ohem_rule(rule, si)
                keep, th = ohem_literal(p, valid, thresh, kept * L.shape[0])
                amb = ((p - th).abs() <= 4 * d_p) & valid
                print(f"K{K} {SHAPE_IDS[si]} {rule}: threshold {th:.6f}, kept {float(keep.sum()) / float(valid.sum()):.3f} "
                      f"of the valid pixels, ambiguous {float(amb.sum()) / float(valid.sum()):.2e}")
