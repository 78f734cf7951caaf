"""Shared inputs and CPU references of the identity-head tests (test_score_loss_cpu.py,
test_gpu_score_loss.py): the score map's backward (csrc/scoregrad.hip) and the branch it closes.

  reference   fp64 torch autograd of the reference's own lines (denseclip.py:672-675: F.normalize of the
              pixel embeddings over channels, F.normalize of the text embeddings, einsum
              'bchw,bkc->bkhw'), then / tau, F.interpolate(bilinear, align_corners=False) and
              F.cross_entropy(ignore_index=255) for the whole branch.
  emulation   the kernel rounds nowhere to 16 bits before its stores (f32 products on the VALU, the norms
              and the projection in f64, the 16-bit v widened exactly), so its emulation is the same
              sequence evaluated in fp32 on the same 16-bit-representable v; a 16-bit dv is the fp32
              result rounded once.
  closed form the arithmetic of include/dclip.h (dclip_score_map_bwd), in any dtype.

    python tests/score_loss_ref.py     prints the emulation's worst absolute error per case and output
                                       (the table committed in test_gpu_score_loss.py)
"""
import functools

import torch
import torch.nn.functional as F

EPS = 1e-12
IGNORE = 255
TAU = 0.07
# (B, h, w, C, K): HW no multiple of the pixel span or of a wave's pixel group; the workload's widths; many
# spans in the dt fold; K on both sides of the 16- and 32-class chunk boundaries and of the forward's two
# kernels; the smallest shape; the two wider slab variants of the kernel (512 < C <= 1024: ViT-L/14's text width,
# and C > 1024, where phase B's threads take a second channel unit and the fold its upper channel slots)
SHAPES = [(2, 5, 7, 48, 19), (2, 8, 16, 512, 19), (1, 17, 61, 64, 19), (2, 4, 9, 64, 1), (2, 4, 9, 64, 32),
          (2, 4, 9, 64, 33), (2, 4, 9, 64, 150), (2, 4, 9, 64, 256), (1, 1, 1, 16, 2), (1, 3, 5, 768, 19),
          (1, 2, 3, 2048, 33), (2, 3, 3, 1040, 19)]
V_DTS = (torch.bfloat16, torch.float16)
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def case_id(shape, v_dt):
    return "x".join(str(s) for s in shape) + ("-bf16" if v_dt == torch.bfloat16 else "-f16")


def cases():
    return [(s, dt) for s in SHAPES for dt in V_DTS]


@functools.lru_cache(maxsize=None)
def inputs(shape, v_dt):
    """v (B, HW, C) in v_dt, t (B, K, C) f32, ds (B, K, HW) f32: seeded, ordinary magnitudes"""
    B, h, w, C, K = shape
    g = torch.Generator().manual_seed(4242 + 7 * B + 11 * h + 13 * w + 17 * C + 19 * K)
    v = (torch.randn(B, h * w, C, generator=g) * 1.5).to(v_dt)
    t = torch.randn(B, K, C, generator=g) * 0.5
    ds = torch.randn(B, K, h * w, generator=g) * 0.1
    return v, t, ds


def score(v, t, eps=EPS):
    """reference lines 672-675 on (B, HW, C) pixel rows: (B, K, HW) in the inputs' dtype"""
    vn = F.normalize(v, dim=2, p=2, eps=eps)
    tn = F.normalize(t, dim=2, p=2, eps=eps)
    return torch.einsum("bpc,bkc->bkp", vn, tn)


def autograd_grads(v, t, ds, dtype, scale=1.0, eps=EPS):
    """(dv, dt) of sum(score * ds * scale) by torch autograd in `dtype`"""
    v = v.to(dtype).clone().requires_grad_(True)
    t = t.to(dtype).clone().requires_grad_(True)
    (score(v, t, eps) * (ds.to(dtype) * scale)).sum().backward()
    return v.grad, t.grad


def closed_form(v, t, ds, dtype, scale=1.0, eps=EPS):
    """dclip_score_map_bwd's arithmetic (include/dclip.h) in `dtype`"""
    v, t, ds = v.to(dtype), t.to(dtype), ds.to(dtype) * scale
    nv = v.norm(dim=2, keepdim=True)
    nt = t.norm(dim=2, keepdim=True)
    rv, rt = 1 / nv.clamp_min(eps), 1 / nt.clamp_min(eps)
    av, at = (nv >= eps).to(dtype), (nt >= eps).to(dtype)
    vn, tn = v * rv, t * rt
    dvn = torch.einsum("bkp,bkc->bpc", ds, tn)
    dtn = torch.einsum("bkp,bpc->bkc", ds, vn)
    dv = rv * (dvn - av * vn * (vn * dvn).sum(2, keepdim=True))
    dt = rt * (dtn - at * tn * (tn * dtn).sum(2, keepdim=True))
    return dv, dt


@functools.lru_cache(maxsize=None)
def reference(shape, v_dt):
    """the fp64 (dv, dt) of a case; computed once, shared, never modified"""
    v, t, ds = inputs(shape, v_dt)
    return autograd_grads(v, t, ds, torch.float64)


def emulate(shape, v_dt, dv_dt=torch.float32):
    """what an implementation with the kernel's rounding points gives: fp32 autograd, dv stored in dv_dt"""
    v, t, ds = inputs(shape, v_dt)
    dv, dt = autograd_grads(v, t, ds, torch.float32)
    return dv.to(dv_dt).float(), dt


def emulated_errors(shape, v_dt):
    """max |emulation - fp64| of (dv in f32, dv in v_dt, dt)"""
    rv, rt = reference(shape, v_dt)
    e32, et = emulate(shape, v_dt, torch.float32)
    e16, _ = emulate(shape, v_dt, v_dt)
    return (float((e32.double() - rv).abs().max()), float((e16.double() - rv).abs().max()),
            float((et.double() - rt).abs().max()))


def bound(emulated, out_dt, ref):
    """the GPU test's rule: 1.5 x the emulated error + one unit roundoff of the output dtype x max |ref|"""
    return 1.5 * emulated + UNIT[out_dt] * float(ref.abs().max())


# ---------------------------------------------------------------- the whole branch
def labels(B, H, W, K, seed=99):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, K, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    return lab


def branch_loss(vmap, text, lab, tau=TAU, eps=EPS):
    """CE(interpolate(score / tau)) of a (B, C, h, w) map and (B, K, C) text in their dtype: reference lines
    672-675, / tau, the resize to the labels' size and the plain cross-entropy"""
    vn = F.normalize(vmap, dim=1, p=2, eps=eps)
    tn = F.normalize(text, dim=2, p=2, eps=eps)
    logits = torch.einsum("bchw,bkc->bkhw", vn, tn) / tau
    up = F.interpolate(logits, size=lab.shape[-2:], mode="bilinear", align_corners=False)
    return F.cross_entropy(up, lab, ignore_index=IGNORE), logits


# ---------------------------------------------------------------- a model without the head
PARENT_STEP = "score_loss_parent_step.npz"  # under tests/golden: seeded_step() as the commit before the head gave it
SAMPLES = 64


def seeded_step(dev="cuda"):
    """{"loss": f32[1], "<parameter>": up to 64 evenly spaced f32 elements of its gradient} of one training
    forward + loss + backward of ViT-B/16 (CITYSCAPES_CFG, the deterministic spec weights, no identity head),
    every parameter trainable but the text encoder's, fused head losses, dropout off, the seeded synthetic batch
    at 2 x 256 x 512 in bf16.  Width 768: every fold of the step has a fixed order, so two runs are bitwise equal."""
    import numpy as np
    from helpers import CITYSCAPES_CFG, CITYSCAPES_CLASSES, spec_state_dict
    from denseclip_vit_multimodal_amd import DenseCLIP
    from denseclip_vit_multimodal_amd.train import freeze_for_mode, loss_fn, synth_batch
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **CITYSCAPES_CFG)
    m.load_state_dict(spec_state_dict("cityscapes"))
    m = m.to(dev).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    freeze_for_mode(m, "F")
    m.fused_head_loss = True
    img, seg, depth, mask = synth_batch(2, 256, 512, torch.device(dev), 0)
    out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
    loss = loss_fn(out, seg, depth, mask)
    loss.backward()
    res = {"loss": loss.detach().float().reshape(1).cpu().numpy(), "out_keys": np.array(sorted(out))}
    for n, p in m.named_parameters():
        if p.grad is not None:
            g = p.grad.detach().float().reshape(-1)
            res[n] = g[::max(1, g.numel() // SAMPLES)][:SAMPLES].cpu().numpy()
    return res


if __name__ == "__main__":
    torch.set_num_threads(8)
    print(f"{'case':28s} {'dv f32':>10s} {'dv 16-bit':>10s} {'dt':>10s}")
    for shape, v_dt in cases():
        a, b, c = emulated_errors(shape, v_dt)
        print(f"    {case_id(shape, v_dt)!r}: ({a:.3e}, {b:.3e}, {c:.3e}),")
