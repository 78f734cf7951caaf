"""The optioned fused resize + CE (csrc/celossopt.hip -> torch.ops.dclip_loss -> ops.upsample_cross_entropy ->
losses.SegCrossEntropy -> train.loss_fn) on the GPU: class weights, label smoothing, pixel weights, the
per-pixel loss map and OHEM, at K in {19 (register-resident), 2, 33, 150, 256 (chunked)}.

C-ABI calls run on guard-banded buffers (abi_guard.run_poisoned): pixel_loss and the workspace pre-filled
with 0xFF and then 0x3C must give equal results, guards intact; sums, count and grad accumulate from
non-zero starts.

Against fp64 (F.interpolate + F.cross_entropy with the same options on the values the low dtype holds):
sums and grad with test_upsample_ce_vs_torch's bounds (1e-5 relative on the sums; gradient rel_err 1e-5
for f32, 1e-2 for bf16 / f16), which are more than 4x REF_FP32_DEPARTURE_SUM (test_ce_options_cpu.py);
count exact; the pixel loss within 4x REF_FP32_DEPARTURE_PIXEL of the case's largest pixel loss, exactly 0
at a pixel that is not valid.

Identities are bitwise (torch.equal): neutral options against the plain kernels, an all-ones pixel weight
against none, a zero pixel weight against an ignored label, forward-only against the full call, two runs.

OHEM: a pixel is ambiguous when its fp64 p_t lies within TAU = 4x REF_FP32_DEPARTURE_PT of the fp64
threshold; every other pixel's keep bit must equal the fp64 rule's, the ambiguous share is capped at 2e-3
(the fp64 reference alone: at most 1.4e-3, one pixel of 728 on near_one; `python tests/ce_options_ref.py`),
and the loss and gradient are compared against fp64 under the kernel path's own keep mask.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ce_options_ref as C
import classes_ref as R
from abi_guard import bitwise_equal, guarded, guarded_copy, run_poisoned
from helpers import MID_CFG, CITYSCAPES_CLASSES, rel_err, spec_state_dict
from test_ce_options_cpu import (REF_FP32_DEPARTURE_GRAD, REF_FP32_DEPARTURE_PIXEL, REF_FP32_DEPARTURE_PT,
                                 REF_FP32_DEPARTURE_SUM)
from test_gpu_classes import build_150, run_ce

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOW_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
LAB_DT = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
TAU = 4 * REF_FP32_DEPARTURE_PT
AMBIGUOUS_MAX = 2e-3
# the issue's bounds against 4x torch's own fp32 departure over the same cases: the sums' 1e-5 and the 16-bit
# gradient's 1e-2 exceed it; the f32 gradient's 1e-5 does not (4 x 4.06e-6) and is kept, the stricter of the two
assert 1e-5 >= 4 * REF_FP32_DEPARTURE_SUM and 1e-2 >= 4 * REF_FP32_DEPARTURE_GRAD


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def _call(name, *args):
    from denseclip_vit_multimodal_amd import _native as N
    return N.call(name, *args)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_opt(L, lab, cw=None, eps=0.0, q=None, want_pl=True, want_grad=True, start=(1.5, 2.5, 3, 0.25)):
    """dclip_upsample_ce_opt through run_poisoned: {sum0, sum1, count, grad, pixel_loss} minus the start values"""
    from denseclip_vit_multimodal_amd import _native as N
    B, K, h, w = L.shape
    H, W = lab.shape[-2:]
    a, b = guarded_copy(L.to(DEV)), guarded_copy(lab.to(DEV))
    gw = None if cw is None else guarded_copy(cw.float().to(DEV))
    gq = None if q is None else guarded_copy(q.float().to(DEV))
    sums, cnt = guarded(2, torch.float64), guarded(1, torch.int32)
    grad = guarded((B, K, h, w), torch.float32) if want_grad else None
    pl = guarded((B, H, W), torch.float32) if want_pl else None
    ws = guarded(int(N.lib().dclip_upsample_ce_opt_ws_floats(B, K, h, w)), torch.float32)
    ptr = lambda g: None if g is None else g.ptr()  # noqa: E731

    def fn():
        sums.t[0] = start[0]; sums.t[1] = start[1]; cnt.t.fill_(start[2])  # noqa: E702
        if grad is not None:
            grad.t.fill_(start[3])
        _call("dclip_upsample_ce_opt", LOW_DT[L.dtype], a.ptr(), B, K, h, w, b.ptr(), LAB_DT[lab.dtype], H, W, C.IGNORE,
              ptr(gw), float(eps), ptr(gq), ptr(pl), sums.ptr(), cnt.ptr(), ptr(grad), ws.ptr(), _stream())

    present = lambda *gs: [g for g in gs if g is not None]  # noqa: E731
    out = run_poisoned(fn, inputs=present(a, b, gw, gq), outputs=present(pl), scratch=[ws],
                       accum=present(sums, cnt, grad))
    res = {}
    if want_pl:
        res["pixel_loss"] = out.pop(0).cpu()
    s, n = out[0].cpu(), out[1].cpu()
    res.update(sum0=float(s[0]) - start[0], sum1=float(s[1]) - start[1], count=int(n) - start[2])
    if want_grad:
        res["grad"] = out[2].double().cpu() - start[3]
    return res


def check_against_fp64(got, ref, low, what):
    e0, e1 = R.rel(got["sum0"], ref["sum0"]), R.rel(got["sum1"], ref["sum1"])
    eg = rel_err(got["grad"], ref["grad"])
    top = float(ref["pixel_loss"].max())
    ep = float((got["pixel_loss"].double() - ref["pixel_loss"]).abs().max()) / top if top > 0 else 0.0
    print(f"{what}: sum q l rel {e0:.2e}, sum q w_t rel {e1:.2e}, gradient rel_err {eg:.2e}, pixel loss {ep:.2e} of "
          f"the largest ({top:.3f})")
    assert got["count"] == ref["count"]
    assert e0 <= 1e-5 and e1 <= 1e-5, (e0, e1)
    assert eg <= (1e-5 if low == torch.float32 else 1e-2), eg
    assert ep <= 4 * REF_FP32_DEPARTURE_PIXEL, ep
    assert int(torch.count_nonzero(got["pixel_loss"][~ref["valid"]])) == 0, "pixel_loss at a pixel that is not valid"


@pytest.mark.parametrize("K,si,low,labdt", C.CASES, ids=[C.case_id(*c) for c in C.CASES])
def test_optioned_ce_against_fp64_on_poisoned_buffers(K, si, low, labdt):
    for name in C.OPTIONS:
        L, lab, cw, eps, q = C.inputs(K, si, low, labdt, name)
        got = run_opt(L, lab, cw, eps, q)
        check_against_fp64(got, C.reference(L, lab, cw, eps, q), low, name)


# the C-ABI matrix of the fp64 comparison: every K x shape at bf16 / int64, the three low dtypes with uint8
# labels on x16 and odd (each low dtype is an instantiation of its own)
IDENTITY_IDS = [C.case_id(*c) for c in C.CASES]


@pytest.mark.parametrize("K,si,low,labdt", C.CASES + [(K, si, torch.float32, torch.int64) for K in C.KS for si in (1, 4)],
                         ids=IDENTITY_IDS + [C.case_id(K, si, torch.float32, torch.int64) for K in C.KS for si in (1, 4)])
def test_neutral_options_give_the_plain_kernels_results_bitwise(K, si, low, labdt):
    """All-ones class weights (and none), no smoothing, no pixel weight: sums[0], count and grad of
    dclip_upsample_ce (K = 19) / dclip_upsample_ce_classes, bit for bit, and sums[1] == count.  The
    optioned kernels are separate functions, so this also holds their compiled arithmetic to the plain
    kernels' (which products are fused into multiply-adds: csrc/celossopt.hip, lerp_rounded)."""
    B, h, w, H, W = C.SHAPES[si]
    L, lab = R.logits(B, K, h, w, low), R.labels(B, K, H, W, labdt)
    zero = (0.0, 0.0, 0, 0.0)
    entry = "dclip_upsample_ce" if K == 19 else "dclip_upsample_ce_classes"
    ls, n, g = run_ce(K, (h, w), (H, W), low, L.to(DEV), lab.to(DEV), entry=entry, start=(0.0, 0, 0.0))
    for cw in (torch.ones(K), None):
        neutral = run_opt(L, lab, cw, 0.0, None, start=zero)
        print(f"neutral against {entry}: loss sum {neutral['sum0']!r} / {ls!r} (rel {R.rel(neutral['sum0'], ls):.1e}), "
              f"{int((neutral['grad'] != g.cpu()).sum())} of {g.numel()} gradient elements differ "
              f"(rel_err {rel_err(neutral['grad'], g):.1e})")
        assert neutral["count"] == n and neutral["sum1"] == float(n)
        assert neutral["sum0"] == ls
        assert torch.equal(neutral["grad"], g.cpu())


@pytest.mark.parametrize("K,si,low,labdt", C.CASES, ids=IDENTITY_IDS)
def test_identities_are_bitwise(K, si, low, labdt):
    B, h, w, H, W = C.SHAPES[si]
    L, lab = R.logits(B, K, h, w, low), R.labels(B, K, H, W, labdt)
    zero = (0.0, 0.0, 0, 0.0)
    # an all-ones pixel weight is none
    cw = C.class_weight(K)
    full = run_opt(L, lab, cw, C.EPS, None, start=zero)
    ones = run_opt(L, lab, cw, C.EPS, torch.ones(B, H, W), start=zero)
    for k in ("sum0", "sum1", "count"):
        assert ones[k] == full[k], k
    assert torch.equal(ones["grad"], full["grad"]) and bitwise_equal(ones["pixel_loss"], full["pixel_loss"])
    # a zero pixel weight on 30 % of the pixels is those labels ignored (sums and gradient; the count is the labels')
    g_ = torch.Generator().manual_seed(1243)
    drop = torch.rand(B, H, W, generator=g_) < 0.3
    masked = run_opt(L, lab, cw, C.EPS, (~drop).float(), start=zero)
    ignored = run_opt(L, torch.where(drop, torch.full_like(lab, C.IGNORE), lab), cw, C.EPS, None, start=zero)
    assert masked["sum0"] == ignored["sum0"] and masked["sum1"] == ignored["sum1"]
    assert torch.equal(masked["grad"], ignored["grad"])
    assert masked["count"] == full["count"]
    # forward only: the same sums, count and pixel loss
    fwd = run_opt(L, lab, cw, C.EPS, C.pixel_weight(B, H, W), want_grad=False, start=zero)
    both = run_opt(L, lab, cw, C.EPS, C.pixel_weight(B, H, W), start=zero)
    for k in ("sum0", "sum1", "count"):
        assert fwd[k] == both[k], k
    assert bitwise_equal(fwd["pixel_loss"], both["pixel_loss"])
    # two runs
    again = run_opt(L, lab, cw, C.EPS, C.pixel_weight(B, H, W), start=zero)
    assert again["sum0"] == both["sum0"] and again["sum1"] == both["sum1"] and again["count"] == both["count"]
    assert bitwise_equal(again["grad"], both["grad"]) and bitwise_equal(again["pixel_loss"], both["pixel_loss"])
    # gradient only (no sums, no pixel loss) is accepted and gives the same gradient
    from denseclip_vit_multimodal_amd import _native as N
    a, b, gw = L.to(DEV), lab.to(DEV), cw.to(DEV)
    q = C.pixel_weight(B, H, W).to(DEV)
    grad = torch.zeros(B, K, h, w, device=DEV)
    ws = torch.empty(int(N.lib().dclip_upsample_ce_opt_ws_floats(B, K, h, w)), device=DEV)
    _call("dclip_upsample_ce_opt", LOW_DT[low], a.data_ptr(), B, K, h, w, b.data_ptr(), LAB_DT[labdt], H, W, C.IGNORE, gw.data_ptr(), C.EPS,
          q.data_ptr(), None, None, None, grad.data_ptr(), ws.data_ptr(), _stream())
    assert torch.equal(grad.double().cpu(), both["grad"])


# ----------------------------------------------------------------------------- autograd level
@pytest.mark.parametrize("low", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("K", [19, 150])
def test_upsample_cross_entropy_against_fp64_autograd(K, low):
    from denseclip_vit_multimodal_amd import ops
    si = 1
    B, h, w, H, W = C.SHAPES[si]
    L, lab, cw, eps, q = C.inputs(K, si, low, torch.int64)
    gtol = 1e-5 if low == torch.float32 else 1e-2
    g_ = torch.Generator().manual_seed(1244)
    upstream = torch.randn(B, H, W, generator=g_)
    for red, pw in (("mean", None), ("mean", q), ("sum", None), ("sum", q), ("none", None), ("none", q)):
        ref = C.reference(L, lab, cw, eps, pw if red != "none" else (upstream if pw is None else upstream * pw))
        x = L.to(DEV).requires_grad_(True)
        n0 = ops.STATS.get("upsample_ce_opt", 0)
        out = ops.upsample_cross_entropy(x, lab.to(DEV), C.IGNORE, cw.to(DEV), eps, None if pw is None else pw.to(DEV), red)
        if red == "none":
            assert out.shape == (B, H, W) and out.dtype == torch.float32
            want = ref["pixel_loss"] if pw is None else ref["pixel_loss"] * pw.double()
            err = float((out.double().cpu() - want).abs().max()) / float(ref["pixel_loss"].max())
            assert err <= 4 * REF_FP32_DEPARTURE_PIXEL * max(1.0, float(pw.abs().max()) if pw is not None else 1.0), err
            (out * upstream.to(DEV)).sum().backward()
            assert ops.STATS.get("upsample_ce_opt", 0) == n0 + 2
            scale = 1.0
        else:
            scale = ref["sum1"] if red == "mean" else 1.0
            err = R.rel(float(out), ref["sum0"] / scale)
            assert out.shape == () and err <= 1e-5, (red, err)
            out.backward()
            assert ops.STATS.get("upsample_ce_opt", 0) == n0 + 1
        eg = rel_err(x.grad.float(), ref["grad"] / scale)
        print(f"{red}, pixel weight {pw is not None}: value err {err:.2e}, gradient rel_err {eg:.2e}")
        assert x.grad.dtype == low and eg <= gtol, (red, eg)


def test_neutral_call_takes_the_plain_kernels_and_all_ignored_gives_nan():
    from denseclip_vit_multimodal_amd import ops
    B, h, w, H, W = C.SHAPES[1]
    for K, stat in ((19, None), (33, "upsample_ce_classes")):
        L, lab = R.logits(B, K, h, w).to(DEV), R.labels(B, K, H, W).to(DEV)
        n0, c0 = ops.STATS.get("upsample_ce_opt", 0), ops.STATS.get("upsample_ce_classes", 0)
        a = ops.upsample_cross_entropy(L, lab)
        assert ops.STATS.get("upsample_ce_opt", 0) == n0
        assert ops.STATS.get("upsample_ce_classes", 0) == c0 + (stat is not None)
        assert bitwise_equal(a, ops.UpsampleCEFn.apply(L, lab, 255))
        x = L.clone().requires_grad_(True)
        loss = ops.upsample_cross_entropy(x, torch.full_like(lab, 255), weight=C.class_weight(K).to(DEV), label_smoothing=0.1)
        loss.backward()
        assert bool(torch.isnan(loss)) and int(torch.count_nonzero(x.grad)) == 0


def test_opcheck_and_argument_checks():
    from denseclip_vit_multimodal_amd import ops
    op = ops.DL().upsample_ce
    K = 33
    B, h, w, H, W = C.SHAPES[1]
    L, lab = R.logits(B, K, h, w, torch.bfloat16).to(DEV), R.labels(B, K, H, W, torch.uint8).to(DEV)
    cw, q = C.class_weight(K).to(DEV), C.pixel_weight(B, H, W).to(DEV)
    utils = ("test_schema", "test_faketensor", "test_aot_dispatch_dynamic")
    torch.library.opcheck(op, (L, lab, 255, cw, 0.1, q, True, True), test_utils=utils)
    torch.library.opcheck(op, (L, lab, 255, None, 0.0, None, True, False), test_utils=utils)
    torch.library.opcheck(op, (L, lab, 255, cw, 0.0, None, False, True), test_utils=utils)
    for bad, needle in (((L, lab, 255, cw[:-1], 0.1, q, True, True), "class_weight"),
                        ((L, lab, 255, cw.double(), 0.1, q, True, True), "float32"),
                        ((L, lab, 255, cw, 0.1, q[:, :-1], True, True), "pixel_weight"),
                        ((L, lab, 255, cw, 0.1, q.half(), True, True), "float32"),
                        ((L, lab, 255, cw, 0.1, q.transpose(1, 2), True, True), "pixel_weight"),
                        ((L, lab, 255, cw.cpu(), 0.1, q, True, True), "GPU"),
                        ((L, lab, 255, cw, 0.1, q.cpu(), True, True), "GPU"),
                        ((L, lab, 255, cw, 1.0, q, True, True), "label_smoothing"),
                        ((L.transpose(2, 3), lab, 255, cw, 0.1, q, True, True), "contiguous")):
        with pytest.raises(RuntimeError, match=needle):
            op(*bad)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- OHEM
OHEM_CASES = [(K, si, rule) for K in C.OHEM_KS for si in C.OHEM_SHAPES for rule in C.OHEM_RULES]


@pytest.mark.parametrize("K,si,rule", OHEM_CASES, ids=[f"K{K}-{C.SHAPE_IDS[si]}-{r}" for K, si, r in OHEM_CASES])
def test_ohem_selection_and_loss(K, si, rule):
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.losses import SegCrossEntropy, ohem_keep
    L, lab = C.ohem_inputs(K, si)
    B = L.shape[0]
    thresh, kept = C.ohem_rule(rule, si)
    cw = C.class_weight(K)
    valid = R.valid_labels(lab, K)
    p64 = C.target_prob(L, lab)
    keep64, threshold = C.ohem_literal(p64, valid, thresh, kept * B)
    share = float(keep64.sum()) / float(valid.sum())
    amb = ((p64 - threshold).abs() <= TAU) & valid
    amb_share = float(amb.sum()) / float(valid.sum())
    print(f"fp64: threshold {threshold:.6f} ({'thresh' if threshold == thresh else 'k-th value'}), kept {share:.3f}, "
          f"ambiguous {amb_share:.2e} (tau {TAU:.2e})")
    assert 0.1 <= share <= 0.9 and amb_share <= AMBIGUOUS_MAX
    assert (threshold == thresh) == (rule == "thresh")
    crit = SegCrossEntropy(cw, C.EPS, ohem={"thresh": thresh, "min_kept": kept}).to(DEV)
    x, labd, validd = L.to(DEV).requires_grad_(True), lab.to(DEV), valid.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit.fused(x, labd)
        loss.backward()
        # the kernel path's own selection, as fused computes it
        with torch.no_grad():
            nll = ops.upsample_cross_entropy(x.detach(), labd, C.IGNORE, reduction="none")
            keep = ohem_keep(torch.exp(-nll), validd, thresh, kept * B)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    keep = keep.cpu()
    wrong = (keep != keep64) & ~amb
    assert not bool(wrong.any()), f"{int(wrong.sum())} unambiguous pixels' keep bits differ from the fp64 rule's"
    assert not bool((keep & ~valid).any())
    ref = C.reference(L, lab, cw, C.EPS, keep.double())
    el, eg = R.rel(float(loss), ref["sum0"] / ref["sum1"]), rel_err(x.grad.float(), ref["grad"] / ref["sum1"])
    print(f"kept {float(keep.sum()) / float(valid.sum()):.3f}; loss rel {el:.2e}, gradient rel_err {eg:.2e}")
    assert el <= 1e-5 and eg <= 1e-2, (el, eg)


# ----------------------------------------------------------------------------- training level
def build_19(cfg, name, cdt=torch.bfloat16):
    from denseclip_vit_multimodal_amd import DenseCLIP
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **cfg)
    m.load_state_dict(spec_state_dict(name))
    m.backbone.compute_dtype = cdt
    return m.to(DEV).eval()


def _trainable(m):
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def _seg_losses(K, H, W):
    from denseclip_vit_multimodal_amd.train import seg_loss_config
    cw = [float(v) for v in C.class_weight(K)]
    plain = {"class_weight": cw, "label_smoothing": 0.1}
    # the k-th smallest p_t decides: a third of each image's pixels are kept
    ohem = dict(plain, ohem={"thresh": 1e-4, "min_kept": H * W // 3})
    return {"weights_smoothing": seg_loss_config({"training": {"seg_loss": plain}}, K).to(DEV),
            "ohem": seg_loss_config({"training": {"seg_loss": ohem}}, K).to(DEV)}


@pytest.mark.parametrize("K", [19, 150])
def test_fused_seg_loss_matches_materialised(K):
    """test_fused_head_loss_matches_materialised with a configured segmentation loss, its tolerances"""
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.train import loss_fn, synth_batch
    H, W = 128, 256
    torch.manual_seed(0)
    m = _trainable(build_19(MID_CFG, "mid") if K == 19 else build_150(MID_CFG, "mid"))
    img, seg, depth, mask = synth_batch(1, H, W, torch.device(DEV), image_dtype=torch.float32, num_classes=K)
    for name, seg_loss in _seg_losses(K, H, W).items():
        res = []
        for fused in (False, True):
            m.fused_head_loss = fused
            m.zero_grad(set_to_none=True)
            n0 = ops.STATS.get("upsample_ce_opt", 0)
            out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
            loss = loss_fn(out, seg, depth, mask, seg_loss=seg_loss)
            loss.backward()
            assert ops.STATS.get("upsample_ce_opt", 0) == n0 + int(fused) * (2 if name == "ohem" else 1)
            res.append((float(loss.detach()),
                        {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
        (l0, g0), (l1, g1) = res
        print(f"K {K} {name}: materialised {l0!r}, fused {l1!r}")
        assert abs(l0 - l1) < 1e-4 * abs(l0), (name, l0, l1)
        assert g0.keys() == g1.keys() and len(g0) > 20
        for k in g0:
            assert rel_err(g1[k], g0[k]) < (2e-2 if k.startswith("backbone.") else 2e-3), (name, k)


def test_captured_train_step_with_a_seg_loss_replays_and_none_is_todays_loss():
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.train import (CapturedTrainStep, freeze_for_mode, loss_fn, make_optimizer,
                                                    synth_batch, train_step)
    H, W = 128, 256
    batch = synth_batch(1, H, W, torch.device(DEV), image_dtype=torch.float32)
    img, seg, depth, mask = batch
    m = _trainable(build_19(MID_CFG, "mid"))
    m.fused_head_loss = True
    # seg_loss=None: the parent's loss, bit for bit, through the plain kernels
    with torch.no_grad():
        out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
        n0 = ops.STATS.get("upsample_ce_opt", 0)
        today = 1.0 * ops.UpsampleCEFn.apply(out["main_output_lowres"], seg, 255) \
            + 0.1 * ops.UpsampleSILogFn.apply(out["depth_output_lowres"], depth, mask, 0.5, 1e-6)
        assert bitwise_equal(loss_fn(out, seg, depth, mask), today)
        assert bitwise_equal(loss_fn(out, seg, depth, mask, seg_loss=None), today)
        assert ops.STATS.get("upsample_ce_opt", 0) == n0
    seg_loss = _seg_losses(19, H, W)["ohem"]

    def make():
        torch.manual_seed(0)
        mm = _trainable(build_19(MID_CFG, "mid"))
        mm.fused_head_loss = True
        return mm, make_optimizer(freeze_for_mode(mm, "F"), capturable=True)

    ma, oa = make()
    eager = [float(train_step(ma, oa, batch, seg_loss=seg_loss)) for _ in range(5)]
    mb, ob = make()
    cap = CapturedTrainStep(mb, ob, batch, seg_loss=seg_loss)
    replays = [float(cap()), float(cap())]
    torch.cuda.synchronize()
    print(f"eager {eager}, captured {replays}")
    assert all(v == v and abs(v) != float("inf") for v in eager + replays)
    assert replays == eager[3:], (replays, eager)
