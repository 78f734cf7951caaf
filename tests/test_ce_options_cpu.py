"""CPU checks of the optioned fused CE (csrc/celossopt.hip, torch.ops.dclip_loss, ops.upsample_cross_entropy,
losses.SegCrossEntropy, train.seg_loss_config): the entry points are declared, bound and exported; the
host checks reject bad arguments before any launch; the op has a fake implementation and refuses CPU
tensors; the config parser, the materialised loss and the OHEM selection rule.

The REF_FP32_* constants: the departure of torch's own fp32 evaluation (F.interpolate -> F.cross_entropy
with the options, fp32) from the fp64 evaluation of the same values, maximised over ce_options_ref.CASES
and its three option sets; recorded from `python tests/ce_options_ref.py` (8 threads).  The GPU test allows
the kernel 4x these figures:
    REF_FP32_DEPARTURE_SUM    sum q l and sum q w_t, relative
    REF_FP32_DEPARTURE_PIXEL  the per-pixel loss, max abs error over the case's largest pixel loss
    REF_FP32_DEPARTURE_PT     exp(-l) of the plain loss against the fp64 p_t, absolute (OHEM's tau / 4)
    REF_FP32_DEPARTURE_GRAD   the gradient of sum q l wrt the low-res logits, norm-wise relative.  The worst case
                              carries the pixel weights (30 % negative, so the folded sums cancel).  The
                              16-bit gradient bound 1e-2 is more than 4x this; the f32 bound 1e-5 is not
                              (4x is 1.6e-5): it is kept as it stands, stricter than torch's own fp32
                              evaluation would warrant."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import ce_options_ref as C
import classes_ref as R
from helpers import ROOT
from denseclip_vit_multimodal_amd import _native as N

REF_FP32_DEPARTURE_SUM = 2.6382e-7
REF_FP32_DEPARTURE_PIXEL = 4.0249e-6
REF_FP32_DEPARTURE_PT = 1.5673e-5
REF_FP32_DEPARTURE_GRAD = 4.0592e-6
NEW = ["dclip_upsample_ce_opt", "dclip_upsample_ce_opt_ws_floats"]
P = ctypes.c_void_p(0x1000)  # a non-null pointer the host checks never dereference


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", f.read(), re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert lib.dclip_upsample_ce_opt_ws_floats.restype is ctypes.c_int64
    for K in (1, 19, 150, 256):
        assert lib.dclip_upsample_ce_opt_ws_floats(2, K, 5, 37) > 0
    for bad in [(0, 19, 4, 4), (1, 0, 4, 4), (1, 257, 4, 4), (1, 19, 0, 4), (1, 19, 4, 0)]:
        assert lib.dclip_upsample_ce_opt_ws_floats(*bad) == 0


def _opt(L, K=150, B=1, h=4, w=8, H=64, W=128, logits=P, labels=P, cw=P, eps=0.1, pw=P, pl=P, sums=P, count=P, grad=P,
         ws=P, low_dt=0, lab_dt=0):
    return L.dclip_upsample_ce_opt(low_dt, logits, B, K, h, w, labels, lab_dt, H, W, 255, cw, eps, pw, pl, sums, count,
                                   grad, ws, None)


@pytest.mark.parametrize("call,needle", [
    (lambda L: _opt(L, K=0), "K=0"),
    (lambda L: _opt(L, K=257), "K=257"),
    (lambda L: _opt(L, h=0), "bad sizes"),
    (lambda L: _opt(L, W=-1), "bad sizes"),
    (lambda L: _opt(L, low_dt=7), "low_dt=7"),
    (lambda L: _opt(L, lab_dt=3), "lab_dt=3"),
    (lambda L: _opt(L, logits=None), "logits and labels required"),
    (lambda L: _opt(L, labels=None), "logits and labels required"),
    (lambda L: _opt(L, ws=None), "ws"),
    (lambda L: _opt(L, ws=ctypes.c_void_p(0x1004)), "ws"),
    (lambda L: _opt(L, eps=-0.1), "label_smoothing"),
    (lambda L: _opt(L, eps=1.0), "label_smoothing"),
    (lambda L: _opt(L, eps=float("nan")), "label_smoothing"),
    (lambda L: _opt(L, grad=None, pl=None, sums=None, count=None), "no output"),
    (lambda L: _opt(L, sums=None), "both or neither"),
    (lambda L: _opt(L, count=None), "both or neither"),
    (lambda L: _opt(L, B=8, H=16384, W=16384), "below 2^31"),
], ids=["K0", "K257", "h0", "W_negative", "dtype", "label_dtype", "null_logits", "null_labels", "null_ws",
        "misaligned_ws", "eps_negative", "eps_one", "eps_nan", "no_output", "sums_without_count", "count_without_sums",
        "2^31"])
def test_host_checks_reject_before_any_launch(call, needle):
    L = N.load()
    assert call(L) == -1
    assert needle in L.dclip_last_error().decode()


@pytest.fixture(scope="module")
def loaded():
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    return torch.ops


def test_op_registered_with_a_fake(loaded):
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = loaded.dclip_loss.upsample_ce
    rets = [str(r.type) for r in op.default._schema.returns]
    assert rets == ["Tensor", "Tensor", "Optional[Tensor]", "Optional[Tensor]"]
    with FakeTensorMode():
        lg = torch.empty(2, 150, 8, 16, device="cuda", dtype=torch.bfloat16)
        lab = torch.empty(2, 128, 256, device="cuda", dtype=torch.uint8)
        cw = torch.empty(150, device="cuda")
        pw = torch.empty(2, 128, 256, device="cuda")
        s, n, g, pl = op(lg, lab, 255, cw, 0.1, pw, True, True)
        assert s.shape == (2,) and s.dtype == torch.float64 and n.shape == (1,) and n.dtype == torch.int32
        assert g.shape == lg.shape and g.dtype == torch.float32 and g.device.type == "cuda"
        assert pl.shape == lab.shape and pl.dtype == torch.float32
        s, n, g, pl = op(lg, lab, 255, None, 0.0, None, False, True)
        assert pl is None and g.shape == lg.shape
        s, n, g, pl = op(lg, lab, 255, None, 0.0, None, True, False)
        assert g is None and pl.shape == lab.shape


def test_cpu_tensors_are_refused(loaded):
    lg, lab = torch.randn(1, 150, 4, 4), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="CPU"):
        loaded.dclip_loss.upsample_ce(lg, lab, 255, None, 0.1, None, False, True)
    from denseclip_vit_multimodal_amd import ops
    for red in ("mean", "none"):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            ops.upsample_cross_entropy(lg, lab, weight=torch.ones(150), reduction=red)


def test_upsample_cross_entropy_argument_checks_and_neutral_dispatch(monkeypatch):
    from denseclip_vit_multimodal_amd import ops
    lg, lab = torch.zeros(1, 19, 2, 2), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="reduction"):
        ops.upsample_cross_entropy(lg, lab, reduction="batchmean")
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.upsample_cross_entropy(lg, lab, label_smoothing=1.0)
    seen = []
    monkeypatch.setattr(ops.UpsampleCEFn, "apply", lambda *a: seen.append(a) or "plain")
    n0 = ops.STATS.get("upsample_ce_opt", 0)
    assert ops.upsample_cross_entropy(lg, lab) == "plain" and seen[0][2] == 255
    assert ops.STATS.get("upsample_ce_opt", 0) == n0


# ----------------------------------------------------------------------------- train.seg_loss_config
def test_seg_loss_config_parses_and_raises():
    from denseclip_vit_multimodal_amd.losses import SegCrossEntropy
    from denseclip_vit_multimodal_amd.train import loss_config, seg_loss_config
    assert seg_loss_config({}, 19) is None and seg_loss_config(None, 19) is None
    assert seg_loss_config({"training": {"loss_weights": {"seg": 1.0}}}, 19) is None
    assert len(loss_config({"training": {"seg_loss": {}}})) == 3
    sl = seg_loss_config({"training": {"seg_loss": {}}}, 19)
    assert isinstance(sl, SegCrossEntropy) and sl.weight is None and sl.label_smoothing == 0.0 and sl.ohem is None
    cw = [0.5 + 0.1 * i for i in range(19)]
    sl = seg_loss_config({"training": {"seg_loss": {"class_weight": cw, "label_smoothing": 0.1,
                                                     "ohem": {"thresh": 0.7, "min_kept": 1000}}}}, 19)
    assert torch.equal(sl.weight, torch.tensor(cw)) and "weight" in dict(sl.named_buffers())
    assert sl.label_smoothing == 0.1 and sl.ohem == {"thresh": 0.7, "min_kept": 1000} and sl.ignore_index == 255
    assert seg_loss_config({"training": {"seg_loss": {"ohem": {}}}}, 19).ohem == {"thresh": 0.7, "min_kept": 100000}
    for bad in ({"class_weight": cw[:18]}, {"class_weight": [-1.0] + cw[1:]}, {"label_smoothing": -0.01},
                {"label_smoothing": 1.0}, {"ohem": {"thresh": 0.0}}, {"ohem": {"thresh": 1.5}},
                {"ohem": {"min_kept": -1}}):
        with pytest.raises(ValueError):
            seg_loss_config({"training": {"seg_loss": bad}}, 19)
    assert seg_loss_config({"training": {"seg_loss": {"ohem": {"thresh": 1.0, "min_kept": 0}}}}, 19) is not None


# ----------------------------------------------------------------------------- losses.SegCrossEntropy
@pytest.mark.parametrize("K", [2, 19, 150])
def test_seg_cross_entropy_forward_is_torch_cross_entropy(K):
    from denseclip_vit_multimodal_amd.losses import SegCrossEntropy
    B, h, w, H, W = C.SHAPES[1]
    up = F.interpolate(R.logits(B, K, h, w).double(), size=(H, W), mode="bilinear", align_corners=False)
    lab = R.labels(B, K, H, W, torch.uint8).long()  # F.cross_entropy refuses labels outside [0, K) but the ignored
    lab[(lab >= K) & (lab != 255)] = 255
    cw = C.class_weight(K).double()
    for weight, eps in ((None, 0.0), (cw, 0.0), (None, 0.1), (cw, 0.1)):
        got = SegCrossEntropy(weight=weight, label_smoothing=eps).double()(up, lab)
        want = F.cross_entropy(up, lab, weight=weight, ignore_index=255, label_smoothing=eps)
        assert torch.equal(got, want), (weight is not None, eps)


def test_seg_cross_entropy_forward_with_ohem_averages_over_the_kept_pixels():
    from denseclip_vit_multimodal_amd.losses import SegCrossEntropy
    K, si = 19, 1
    L, lab = C.ohem_inputs(K, si)
    thresh, kept = C.ohem_rule("kth", si)
    cw = C.class_weight(K)
    up = F.interpolate(L.double(), size=lab.shape[-2:], mode="bilinear", align_corners=False).requires_grad_(True)
    lab = torch.where(R.valid_labels(lab, K), lab, torch.full_like(lab, 255))
    loss = SegCrossEntropy(weight=cw, label_smoothing=0.1, ohem={"thresh": thresh, "min_kept": kept}).double()(up, lab)
    keep, _ = C.ohem_literal(C.target_prob(L, lab), lab != 255, thresh, kept * L.shape[0])
    assert 0.1 < float(keep.sum()) / float((lab != 255).sum()) < 0.9
    ref = C.reference(L, lab, cw, 0.1, keep.double(), grad=False)
    assert abs(float(loss.detach()) - ref["sum0"] / ref["sum1"]) <= 1e-12 * abs(float(loss.detach()))
    loss.backward()
    # no gradient reaches a pixel that was not kept
    assert int(torch.count_nonzero(up.grad.abs().sum(1)[~keep])) == 0 and float(up.grad.abs().sum()) > 0


def _ohem_cases():
    g = torch.Generator().manual_seed(3)
    p = torch.rand(2, 9, 13, generator=g, dtype=torch.float64)
    valid = torch.rand(2, 9, 13, generator=g) < 0.8
    tied = (p * 8).floor() / 8  # many equal values, so the k-th value has ties on both sides
    n = int(valid.sum())
    yield "thresh_decides", p, valid, 0.7, 5
    yield "kth_decides", p, valid, 0.05, n // 2
    yield "n_valid_le_batch_kept", p, valid, 0.3, n
    yield "n_valid_lt_batch_kept", p, valid, 0.3, 10 * n
    yield "all_ignored", p, torch.zeros_like(valid), 0.7, 5
    yield "ties_at_the_threshold", tied, valid, 0.01, n // 2
    yield "ties_at_thresh", tied, valid, 0.5, 3
    yield "nothing_kept_but_zero", p, valid, 0.01, 0
    yield "one_valid", p, (torch.arange(p.numel()) == 17).view(p.shape), 0.5, 100


@pytest.mark.parametrize("name,p,valid,thresh,kept", list(_ohem_cases()), ids=[c[0] for c in _ohem_cases()])
def test_ohem_keep_equals_the_literal_rule(name, p, valid, thresh, kept):
    from denseclip_vit_multimodal_amd.losses import ohem_keep
    want, threshold = C.ohem_literal(p, valid, thresh, kept)
    got = ohem_keep(p, valid, thresh, kept)
    assert got.dtype == torch.bool and torch.equal(got, want), (name, threshold)
    assert not bool((got & ~valid).any())
    if name == "all_ignored":
        assert not bool(got.any())
    if name.startswith("ties"):
        assert bool(((p == threshold) & valid).any()) and not bool(got[p == threshold].any())
    assert torch.equal(ohem_keep(p.float(), valid, thresh, kept), C.ohem_literal(p.float(), valid, thresh, kept)[0])


# ----------------------------------------------------------------------------- train.loss_fn
def test_loss_fn_without_a_seg_loss_is_todays_value():
    from denseclip_vit_multimodal_amd.losses import SegCrossEntropy
    from denseclip_vit_multimodal_amd.train import loss_fn
    g = torch.Generator().manual_seed(9)
    out = {"main_output": torch.randn(2, 19, 16, 24, generator=g), "depth_output": 1 + torch.rand(2, 1, 16, 24, generator=g)}
    seg = torch.randint(0, 19, (2, 16, 24), generator=g)
    seg[torch.rand(2, 16, 24, generator=g) < 0.1] = 255
    depth, mask = 1 + 79 * torch.rand(2, 1, 16, 24, generator=g), torch.rand(2, 1, 16, 24, generator=g) > 0.2
    from denseclip_vit_multimodal_amd.losses import SILogLoss
    today = 1.0 * F.cross_entropy(out["main_output"], seg, ignore_index=255) \
        + 0.1 * SILogLoss()(out["depth_output"], depth, mask)
    assert torch.equal(loss_fn(out, seg, depth, mask), today)
    assert torch.equal(loss_fn(out, seg, depth, mask, seg_loss=None), today)
    # a neutral configured loss is the same formula; a weighted one is torch's weighted CE in its place
    assert torch.allclose(loss_fn(out, seg, depth, mask, seg_loss=SegCrossEntropy()), today, rtol=1e-6, atol=0)
    cw = C.class_weight(19)
    want = F.cross_entropy(out["main_output"], seg, weight=cw, ignore_index=255, label_smoothing=0.1) \
        + 0.1 * SILogLoss()(out["depth_output"], depth, mask)
    assert torch.equal(loss_fn(out, seg, depth, mask, seg_loss=SegCrossEntropy(cw, 0.1)), want)


def test_reference_formulas_are_the_issues():
    """the closed forms the kernels implement against autograd through F.cross_entropy, fp64"""
    K, si = 33, 1
    L, lab, cw, eps, q = C.inputs(K, si, torch.float32, torch.int64)
    ref = C.reference(L, lab, cw, eps, q)
    u = F.interpolate(L.double(), size=lab.shape[-2:], mode="bilinear", align_corners=False).requires_grad_(True)
    valid = ref["valid"]
    t = torch.where(valid, lab, torch.zeros_like(lab))
    logp = F.log_softmax(u, 1)
    w = cw.double()
    l = (1 - eps) * w[t] * -logp.gather(1, t[:, None])[:, 0] + eps / K * (-(logp * w[None, :, None, None])).sum(1)
    l = torch.where(valid, l, torch.zeros_like(l))
    assert float((l - ref["pixel_loss"]).abs().max()) <= 1e-12
    (q.double() * l).sum().backward()
    P_ = logp.exp().detach()
    onehot = F.one_hot(t, K).permute(0, 3, 1, 2).double()
    d = (1 - eps) * w[t][:, None] * (P_ - onehot) + eps / K * (P_ * w.sum() - w[None, :, None, None])
    d = d * (q.double() * valid)[:, None]
    assert float((d - u.grad).abs().max()) <= 1e-12 * float(u.grad.abs().max()) + 1e-15
