"""CPU checks of the identity-head branch: the closed form of dclip_score_map_bwd (include/dclip.h) against fp64
autograd of the reference's lines, zero rows included; the new symbols declared, bound and exported, their host
checks; the op registered with a fake implementation and refusing CPU tensors; the trainer's weight lookup and
YAML parsing; gradless_parameter_names with the head on and off, with and without a context decoder; loss_fn's
materialised path; a model without the head keeps today's outputs."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import score_loss_ref as R
from helpers import CITYSCAPES_CLASSES, MID_CFG, ROOT, TINY_CTX_CFG
from denseclip_vit_multimodal_amd import _native as N

NEW = ["dclip_score_map_bwd", "dclip_score_map_bwd_ws_floats"]
HEAD = dict(type="IdentityHead", loss_weight=0.4)
P = ctypes.c_void_p(0x1000)


@pytest.mark.parametrize("shape,v_dt", [(R.SHAPES[0], torch.bfloat16), (R.SHAPES[5], torch.float16),
                                        (R.SHAPES[8], torch.bfloat16)], ids=["odd", "K33", "smallest"])
def test_closed_form_equals_fp64_autograd(shape, v_dt):
    v, t, ds = (x.clone() for x in R.inputs(shape, v_dt))
    for zero_rows in (False, True):
        if zero_rows:
            v[0, 0] = 0
            t[0, -1] = 0
        for scale in (1.0, 1.0 / R.TAU):
            a = R.autograd_grads(v, t, ds, torch.float64, scale)
            c = R.closed_form(v, t, ds, torch.float64, scale)
            for x, y in zip(a, c):
                # relative to each row's size: a clamped row's gradient is dvn / eps ~ 1e11
                rows = y.abs().amax(dim=2, keepdim=True).clamp_min(1e-30)
                assert float(((x - y).abs() / rows).max()) < 1e-12
            if zero_rows:
                assert bool(torch.isfinite(c[0].float()).all()) and float(c[0][0, 0].abs().max()) > 1e6
                tn = F.normalize(t.double(), dim=2, eps=R.EPS)
                want = torch.einsum("k,kc->c", ds[0, :, 0].double() * scale, tn[0]) / R.EPS
                assert torch.allclose(c[0][0, 0], want, rtol=1e-12, atol=0)


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", f.read(), re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert lib.dclip_score_map_bwd_ws_floats.restype is ctypes.c_int64
    assert len(N._SIGS["dclip_score_map_bwd"]) == 21


def _bwd(L, K=19, v_dt=2, dv_dt=0, C=64, B=1, HW=8, v=P, t=P, ds=P, dv=P, dt=P, ws=P, dv_ld=None):
    return L.dclip_score_map_bwd(v, v_dt, HW * C, 0, C, t, ds, 1.0, dv, dv_dt, HW * C, 0, dv_ld or C, dt, ws, B, HW, C, K,
                                 1e-12, None)


@pytest.mark.parametrize("kw,needle", [
    (dict(K=0), "K=0"), (dict(K=257), "K=257"), (dict(v_dt=0), "f16/bf16"), (dict(dv_dt=1), "dv_dt=1"),
    (dict(C=72), "C % 16"), (dict(C=4096), "C <= 2048"), (dict(B=70000), "65535"), (dict(HW=0), "empty"),
    (dict(v=None), "required"), (dict(dv=None), "required"), (dict(dt=None), "required"), (dict(ws=None), "ws"),
    (dict(ws=ctypes.c_void_p(0x1004)), "ws"), (dict(dv_ld=68), "dv needs"), (dict(v=ctypes.c_void_p(0x1008)), "16-byte"),
], ids=["K0", "K257", "v_dt", "dv_dt", "C16", "Cmax", "B", "HW0", "v", "dv", "dt", "ws", "ws_align", "dv_ld", "v_align"])
def test_host_checks_reject_before_any_launch(kw, needle):
    L = N.load()
    assert _bwd(L, **kw) == -1
    assert needle in L.dclip_last_error().decode()


def test_workspace_is_a_function_of_the_shapes():
    L = N.load()
    q = L.dclip_score_map_bwd_ws_floats
    # tn (B K C) + one dt partial (K C) per image and span of 256 pixels
    for B, HW, C, K in [(8, 8192, 512, 19), (1, 1, 16, 2), (2, 257, 64, 150), (1, 1037, 2048, 256)]:
        assert q(B, HW, C, K) == B * K * C * (1 + (HW + 255) // 256)
    for bad in [(0, 8, 64, 19), (1, 0, 64, 19), (1, 8, 0, 19), (1, 8, 4096, 19), (1, 8, 64, 0), (1, 8, 64, 257)]:
        assert q(*bad) == 0


@pytest.fixture(scope="module")
def loaded():
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    return torch.ops


def test_op_registered_with_a_fake_and_refuses_cpu_tensors(loaded):
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = loaded.dclip_classes.score_map_bwd
    B, HW, C, K = 2, 40, 64, 150
    with FakeTensorMode():
        v = torch.empty(B * HW, C, device="cuda", dtype=torch.bfloat16)
        t = torch.empty(B, K, C, device="cuda")
        ds = torch.empty(B, K, HW, device="cuda")
        dv, dt = op(v, HW * C, 0, C, t, ds, 1.0, B, HW, 1e-12, torch.float32)
        assert dv.shape == (B * HW, C) and dv.dtype == torch.float32 and dt.shape == (B, K, C) and dt.dtype == torch.float32
        tok = torch.empty(B * (HW + 1), C, device="cuda", dtype=torch.float16)
        dv, _ = op(tok, (HW + 1) * C, 1, C, t, ds, 1.0, B, HW, 1e-12, torch.float16)
        assert dv.shape == (B * HW, C) and dv.dtype == torch.float16  # dense rows from a token buffer
    with pytest.raises(NotImplementedError, match="CPU"):
        op(torch.randn(B * HW, C).bfloat16(), HW * C, 0, C, torch.randn(B, K, C), torch.randn(B, K, HW), 1.0, B, HW, 1e-12,
           torch.float32)
    # the pinned dclip:: namespace is as it was: the new op lives beside score_map in dclip_classes
    names = {n for n in torch._C._dispatch_get_all_op_names() if n.startswith("dclip_classes::")}
    assert "dclip_classes::score_map_bwd" in names and "dclip::score_map_bwd" not in torch._C._dispatch_get_all_op_names()


def test_identity_loss_weight_and_yaml():
    from denseclip_vit_multimodal_amd import DenseCLIP
    from denseclip_vit_multimodal_amd.config import load_yaml, model_kwargs
    from denseclip_vit_multimodal_amd.train import identity_loss_weight, loss_config
    cfg = load_yaml("denseclip_cityscapes.yaml")
    assert identity_loss_weight(cfg) is None and identity_loss_weight(None) is None
    before = loss_config(cfg)[:2]
    cfg["model"]["identity_head"] = dict(type="IdentityHead", in_channels=19, channels=19, num_classes=19,
                                         dropout_ratio=0.1, align_corners=False)
    assert identity_loss_weight(cfg) == 0.4  # the published configs' weight
    cfg["model"]["identity_head"]["loss_weight"] = 0.25
    assert identity_loss_weight(cfg) == 0.25
    cfg["model"]["identity_head"]["loss_decode"] = dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.3)
    assert identity_loss_weight(cfg) == 0.3  # loss_decode takes precedence
    cfg["training"]["loss_weights"]["identity"] = 0.5
    assert identity_loss_weight(cfg) == 0.5  # the trainer's own override
    assert loss_config(cfg)[:2] == before  # its return value does not change
    assert model_kwargs(cfg, clip_path_override="")["identity_head"]["loss_decode"]["loss_weight"] == 0.3
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(MID_CFG, identity_head=cfg["model"]["identity_head"]))
    assert m.with_identity_head and m.identity_loss_weight == 0.3 and identity_loss_weight(m) == 0.3
    assert sum(p.numel() for p in m.identity_head.parameters()) == 0
    m0 = DenseCLIP(class_names=CITYSCAPES_CLASSES, **MID_CFG)
    assert not m0.with_identity_head and identity_loss_weight(m0) is None and m0.identity_head is None
    assert m.state_dict().keys() == m0.state_dict().keys()
    with pytest.raises(ValueError, match="identity_head type"):
        DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(MID_CFG, identity_head=dict(type="FCNHead")))
    with pytest.raises(NotImplementedError, match="align_corners"):
        DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(MID_CFG, identity_head=dict(HEAD, align_corners=True)))


def test_gradless_parameter_names_follow_the_head():
    from denseclip_vit_multimodal_amd import DenseCLIP
    from denseclip_vit_multimodal_amd.train import gradless_parameter_names

    def names(**kw):
        return set(gradless_parameter_names(DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(MID_CFG, **kw))))

    ctx = TINY_CTX_CFG["context_decoder"]
    today = {"backbone.proj", "contexts", "gamma", "vis_proj.weight", "vis_proj.bias", "global_proj.weight",
             "global_proj.bias"}
    assert names() == today
    off_ctx = names(context_decoder=ctx)
    assert today < off_ctx and any(n.startswith("context_decoder.") for n in off_ctx)
    assert all(n in today or n.startswith("context_decoder.") for n in off_ctx)
    # head on, no decoder: the contexts and vis_proj train; the pooled feature feeds nothing
    assert names(identity_head=HEAD) == {"backbone.proj", "gamma", "global_proj.weight", "global_proj.bias"}
    # head on, decoder over [pooled; pixels]: everything but the unused CLIP projection trains
    assert names(identity_head=HEAD, context_decoder=ctx) == {"backbone.proj"}
    # head on, decoder over the pixels alone: global_proj stays dead
    assert names(identity_head=HEAD, context_decoder=ctx, context_feature="backbone") == \
        {"backbone.proj", "global_proj.weight", "global_proj.bias"}
    # a frozen parameter is not listed
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(MID_CFG, identity_head=HEAD))
    m.gamma.requires_grad_(False)
    assert "gamma" not in gradless_parameter_names(m)


def test_shipped_yaml_with_the_head_enabled():
    from denseclip_vit_multimodal_amd.config import load_yaml, model_kwargs
    from denseclip_vit_multimodal_amd.train import _dead_names
    cfg = load_yaml("denseclip_cityscapes.yaml")
    cfg["model"]["identity_head"] = dict(HEAD)
    kw = model_kwargs(copy.deepcopy(cfg), clip_path_override="")
    assert kw["identity_head"] == HEAD and not kw.get("context_decoder")

    class Shell:  # the two attributes the rule reads, without building ViT-B/16 on the CPU
        with_identity_head, context_decoder, context_feature = True, None, kw["context_feature"]

    assert _dead_names(Shell) == (("backbone.proj", "gamma"), ("global_proj.",))


def test_loss_fn_materialised_path_adds_the_identity_term():
    from denseclip_vit_multimodal_amd.losses import SILogLoss
    from denseclip_vit_multimodal_amd.train import loss_fn
    g = torch.Generator().manual_seed(5)
    B, K, H, W = 2, 19, 12, 20
    main = torch.randn(B, K, H, W, generator=g, requires_grad=True)
    ident = torch.randn(B, K, H, W, generator=g, requires_grad=True)
    depth_out = 1 + torch.rand(B, 1, H, W, generator=g)
    seg = R.labels(B, H, W, K)
    depth = 1 + 79 * torch.rand(B, 1, H, W, generator=g)
    mask = torch.rand(B, 1, H, W, generator=g) > 0.2
    out = {"main_output": main, "depth_output": depth_out, "aux_losses": {"identity_head": ident}}
    plain = {"main_output": main, "depth_output": depth_out, "aux_losses": {}}
    base = loss_fn(plain, seg, depth, mask, seg_weight=0.7, silog_weight=0.2)
    want = 0.7 * F.cross_entropy(main, seg, ignore_index=255) + 0.2 * SILogLoss()(depth_out, depth, mask)
    assert torch.equal(base, want)  # without the keyword: today's loss
    got = loss_fn(out, seg, depth, mask, seg_weight=0.7, silog_weight=0.2, identity_weight=0.4)
    assert torch.equal(got, want + 0.4 * F.cross_entropy(ident, seg, ignore_index=255))
    got.backward()
    assert ident.grad is not None and float(ident.grad.abs().sum()) > 0
    with pytest.raises(ValueError, match="identity"):
        loss_fn({"main_output": main, "depth_output": None, "aux_losses": {}}, seg, depth, mask, identity_weight=0.4)
    # logits without a weight: refused (the head's parameters are listed as alive, so they must get a gradient)
    with pytest.raises(ValueError, match="no identity_weight"):
        loss_fn(out, seg, depth, mask)
    with pytest.raises(ValueError, match="no identity_weight"):
        loss_fn({"main_output_lowres": main, "identity_output_lowres": ident}, seg, depth, mask)


def test_the_branch_refuses_a_cpu_map_in_training():
    from denseclip_vit_multimodal_amd import DenseCLIP
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(MID_CFG, identity_head=HEAD)).train()
    maps = [torch.zeros(1, 128, 2, 4)] * 2
    with pytest.raises(RuntimeError, match="identity_head"):
        m._process_features(maps)


def test_keywords_reach_every_step_function():
    import inspect
    from denseclip_vit_multimodal_amd import train
    for fn in (train.loss_fn, train.train_step, train.train_step_accum, train.CapturedTrainStep.__init__):
        p = inspect.signature(fn).parameters
        assert "identity_weight" in p and p["identity_weight"].default is None, fn


def test_a_model_without_the_head_returns_todays_keys(monkeypatch):
    """the forward's result dicts, with the backbone, the score branch and the heads stubbed out (no GPU)"""
    from denseclip_vit_multimodal_amd import DenseCLIP, ops
    seg, depth = torch.zeros(1, 19, 2, 4), torch.zeros(1, 1, 2, 4)
    img, gt = torch.zeros(1, 3, 32, 64), torch.zeros(1, 32, 64, dtype=torch.long)
    monkeypatch.setattr(ops, "upsample", lambda x, size: F.interpolate(x, size=size, mode="bilinear"))
    for head in (None, HEAD):
        m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **(MID_CFG if head is None else dict(MID_CFG, identity_head=head)))
        logits = torch.ones(1, 19, 2, 4)
        monkeypatch.setattr(m, "extract_feat", lambda x: [torch.zeros(1, 128, 2, 4)] * 2)
        monkeypatch.setattr(m, "_process_features", lambda f: (None, f, logits, f))
        monkeypatch.setattr(m, "_heads", lambda maps: (seg, depth))
        monkeypatch.setattr(m, "neck", None)
        m.train()
        out = m(img, gt_semantic_seg=gt, return_loss=True)
        assert set(out) == {"main_output", "depth_output", "aux_losses"}
        assert set(out["aux_losses"]) == (set() if head is None else {"identity_head"})
        if head is not None:
            assert out["aux_losses"]["identity_head"].shape == (1, 19, 32, 64)
        m.fused_head_loss = True
        out = m(img, gt_semantic_seg=gt, return_loss=True)
        today = {"main_output", "depth_output", "aux_losses", "main_output_lowres", "depth_output_lowres"}
        assert set(out) == (today if head is None else today | {"identity_output_lowres"})
        assert out["aux_losses"] == {}
        with torch.no_grad():  # no gradients: the branch is not part of a graph, nothing extra is returned
            assert set(m(img, gt_semantic_seg=gt, return_loss=True)) == today
        m.eval()
        assert set(m(img, return_loss=False)) == {"seg", "depth"}
