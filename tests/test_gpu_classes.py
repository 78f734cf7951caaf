"""The any-class-count paths (csrc/classes.hip -> torch.ops.dclip_classes / dclip_eval -> ops.py,
evaluate.py) on the GPU, at K in {2, 33, 150, 256} (below one chunk, two 32-row score tiles plus one
class, ADE20K's count, the limit) and at K = 19 against the 19-class kernels.

C-ABI calls run on guard-banded buffers (abi_guard.run_poisoned): outputs and workspace pre-filled
with 0xFF and then 0x3C must give equal results, guards intact, accumulators checked from a non-zero
start.

Class map: as test_gpu_eval.py, against the fp64 resize u of the logits' values: a pixel is ambiguous
when its top-2 gap in u is below tau = eval_ref.tau; every other pixel must equal argmax u, an
ambiguous one must pick a class within tau of the maximum.  The ambiguous share is capped at 3e-3: with
these seeds the fp64 reference alone gives at most 2.2e-3 (K = 256, bf16, the wide shape) and 1.2e-3
(one pixel of 816) on the near-one shape, so test_gpu_eval.py's 1e-3 would not hold here.

CE sum: within 4x REF_FP32_DEPARTURE_CE (test_classes_cpu.py: torch's own fp32 evaluation departs
from the fp64 one by that much over these cases) of the fp64 value.

Fused CE (ops.UpsampleCEFn) against F.cross_entropy(F.interpolate(...)) in fp64 on the same values,
with test_upsample_ce_vs_torch's bounds: loss 1e-5 relative, gradient rel_err 1e-5 (f32) / 1e-2 (bf16).
Score map against fp32 torch with test_score_map_and_row_mean's bounds: 4e-3 bf16, 1e-3 f16.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import classes_ref as R
from abi_guard import bitwise_equal, guarded, guarded_copy, guarded_rows_copy, run_poisoned
from helpers import MID_CFG, TINY_CFG, CITYSCAPES_CLASSES, images, rel_err, spec_state_dict
from test_classes_cpu import REF_FP32_DEPARTURE_CE

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOW_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
LAB_DT = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
AMBIGUOUS_MAX = 3e-3
_name = lambda d: str(d).replace("torch.", "")  # noqa: E731


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def _call(name, *args):
    from denseclip_vit_multimodal_amd import _native as N
    return N.call(name, *args)


def _lib():
    from denseclip_vit_multimodal_amd import _native as N
    return N.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- evaluation
@functools.lru_cache(maxsize=2)
def seg_reference(K, shape, low):
    """(u fp64 (B, K, H, W), tau, top-2 values) of the case's logits as the low dtype holds them"""
    B, h, w, H, W = shape
    L = R.logits(B, K, h, w, low)
    u = R.resize(L, H, W)
    return u, R.tau(L.float(), h, w), u.topk(min(2, K), dim=1).values


def check_class_map(pred, K, shape, low, identity=False):
    """pred (B, H, W) uint8 on the CPU against the fp64 resize; returns the ambiguous pixels' mask"""
    B, h, w, H, W = shape
    u, tau, top = seg_reference(K, shape, low)
    amb = (top[:, 0] - top[:, 1]) < tau
    p = pred.long()
    if identity:
        assert torch.equal(p, R.logits(B, K, h, w, low).float().argmax(1)), "identity resize: argmax of the input"
        return amb
    frac = float(amb.float().mean())
    print(f"ambiguous {frac:.2e} (tau {tau:.3e})")
    assert frac <= AMBIGUOUS_MAX, frac
    wrong = (p != u.argmax(1)) & ~amb
    assert not bool(wrong.any()), f"{int(wrong.sum())} unambiguous pixels differ from argmax of the fp64 resize"
    picked = u.gather(1, p.unsqueeze(1))[:, 0]
    assert bool((top[:, 0] - picked <= tau).all()), "an ambiguous pixel picked a class further than tau from the maximum"
    return amb


def run_seg(K, shape, low, labdt, start=(5, 1.5, 3), ignore=R.IGNORE, entry="dclip_upsample_eval_seg_classes",
            logits=None, labels=None):
    """an eval_seg entry point through run_poisoned; (pred, cm, loss_sum, count) minus the start values"""
    B, h, w, H, W = shape
    lg = guarded_copy((R.logits(B, K, h, w, low) if logits is None else logits).to(DEV))
    lab = guarded_copy((R.labels(B, K, H, W, labdt) if labels is None else labels).to(DEV))
    pred = guarded((B, H, W), torch.uint8)
    cm, loss, cnt = guarded((K, K), torch.int64), guarded(1, torch.float64), guarded(1, torch.int64)
    query = entry.replace("_seg_classes", "_seg_classes_ws_bytes") if "classes" in entry else "dclip_upsample_eval_ws_bytes"
    ws = guarded(int(getattr(_lib(), query)(B, K, h, w)))

    def fn():
        cm.t.fill_(start[0]); loss.t.fill_(start[1]); cnt.t.fill_(start[2])  # noqa: E702
        _call(entry, LOW_DT[low], lg.ptr(), B, K, h, w, lab.ptr(), LAB_DT[labdt], H, W, ignore, pred.ptr(), cm.ptr(),
              loss.ptr(), cnt.ptr(), ws.ptr(), _stream())

    p, c, ls, n = run_poisoned(fn, inputs=[lg, lab], outputs=[pred], scratch=[ws], accum=[cm, loss, cnt])
    return p.cpu(), c.cpu() - start[0], float(ls.cpu()) - start[1], int(n.cpu()) - start[2]


SEG_CASES = [(K, s, low, lab) for K in R.KS for s in range(len(R.SHAPES)) for low in R.LOWS for lab in R.LABS]


@pytest.mark.parametrize("K,si,low,labdt", SEG_CASES,
                         ids=[f"K{K}-{R.SHAPE_IDS[s]}-{_name(lo)}-{_name(la)}" for K, s, lo, la in SEG_CASES])
def test_seg_class_map_confusion_matrix_count_and_ce(K, si, low, labdt):
    shape = R.SHAPES[si]
    B, h, w, H, W = shape
    pred, cm, loss, count = run_seg(K, shape, low, labdt)
    check_class_map(pred, K, shape, low, identity=(h, w) == (H, W))
    lab = R.labels(B, K, H, W, labdt)
    valid = R.valid_labels(lab, K)
    assert int(valid.sum()) < lab.numel()  # ignore / out-of-range labels are present ...
    want = torch.bincount((lab.long() * K + pred.long())[valid], minlength=K * K).view(K, K)
    assert torch.equal(cm, want)  # ... and contribute nothing; the kernel's own class map otherwise, exactly
    assert count == int(valid.sum())
    u, _, _ = seg_reference(K, shape, low)
    ce64 = R.ce_sum(u, lab, K)
    err = R.rel(loss, ce64)
    print(f"CE sum {loss!r} vs fp64 {ce64!r}: rel {err:.2e}")
    assert err <= 4 * REF_FP32_DEPARTURE_CE, err


@pytest.mark.parametrize("K", [33, 150, 256])
@pytest.mark.parametrize("si", [0, 1, 4], ids=["x16", "odd", "identity"])
def test_tie_takes_the_lower_class(K, si):
    """two channels identical everywhere and above every other, one in the first class chunk and one
    in the last: the lower index everywhere"""
    from denseclip_vit_multimodal_amd.evaluate import upsample_argmax
    B, h, w, H, W = R.SHAPES[si]
    L = R.logits(B, K, h, w).clone()
    L[:, K - 1] = L[:, 4] = L.amax(1) + 1.0
    pred = upsample_argmax(L.to(DEV), (H, W))
    assert pred.dtype == torch.uint8 and bool((pred == 4).all())


@pytest.mark.parametrize("K", [33, 150])
@pytest.mark.parametrize("si", [0, 1], ids=["x16", "odd"])
def test_labels_null_gives_the_same_class_map(K, si):
    shape = R.SHAPES[si]
    B, h, w, H, W = shape
    low = torch.bfloat16
    lg = guarded_copy(R.logits(B, K, h, w, low).to(DEV))
    pred = guarded((B, H, W), torch.uint8)

    def fn():
        _call("dclip_upsample_eval_seg_classes", LOW_DT[low], lg.ptr(), B, K, h, w, None, 0, H, W, R.IGNORE, pred.ptr(),
              None, None, None, None, _stream())

    (p,) = run_poisoned(fn, inputs=[lg], outputs=[pred])
    check_class_map(p.cpu(), K, shape, low)
    from denseclip_vit_multimodal_amd.evaluate import _E
    E = _E()
    cm = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ce = torch.zeros(2, dtype=torch.float64, device=DEV)
    lab = R.labels(B, K, H, W).to(DEV)
    with_labels = E.seg_update_classes(lg.t, lab, R.IGNORE, cm, ce, True)
    assert torch.equal(E.upsample_argmax_classes(lg.t, H, W), with_labels) and torch.equal(with_labels, p)
    assert E.seg_update_classes(lg.t, lab, R.IGNORE, cm, ce, False) is None
    assert int(cm.sum()) == 2 * int(R.valid_labels(lab, K).sum()) == int(ce[1])


@pytest.mark.parametrize("ignore", [255, -100])
def test_256_classes_and_the_ignore_index(ignore):
    """K = 256: with ignore 255 the label 255 is skipped although it is a class; with ignore -100 it counts"""
    K, shape = 256, R.SHAPES[1]
    B, h, w, H, W = shape
    g = torch.Generator().manual_seed(77)
    lab = torch.randint(0, K, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.2] = 255
    assert int((lab == 255).sum()) > 100
    pred, cm, loss, count = run_seg(K, shape, torch.float32, torch.int64, ignore=ignore, labels=lab)
    valid = R.valid_labels(lab, K, ignore)
    assert count == int(valid.sum()) == (lab.numel() - (int((lab == 255).sum()) if ignore == 255 else 0))
    want = torch.bincount((lab * K + pred.long())[valid], minlength=K * K).view(K, K)
    assert torch.equal(cm, want)
    assert (int(cm[255].sum()) == 0) == (ignore == 255)
    u, _, _ = seg_reference(K, shape, torch.float32)
    assert R.rel(loss, R.ce_sum(u, lab, K, ignore)) <= 4 * REF_FP32_DEPARTURE_CE


@pytest.mark.parametrize("K", [33, 256])
def test_two_runs_are_bitwise_equal_and_updates_add(K):
    shape, low = R.SHAPES[0], torch.bfloat16
    a = run_seg(K, shape, low, torch.int64)
    b = run_seg(K, shape, low, torch.int64, start=(0, 0.0, 0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[3] == b[3]
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    B, h, w, H, W = shape
    lg, lab = R.logits(B, K, h, w, low).to(DEV), R.labels(B, K, H, W).to(DEV)
    one, two = Evaluator(num_classes=K, device=DEV), Evaluator(num_classes=K, device=DEV)
    one.update(lg, None, lab)
    two.update(lg, None, lab)
    again = Evaluator(num_classes=K, device=DEV)
    again.update(lg, None, lab)
    assert bitwise_equal(one.ce_sums, again.ce_sums) and torch.equal(one.cm, again.cm)
    assert torch.equal(one.cm.cpu(), b[1]) and float(one.ce_sums[0]) == b[2]
    two.update(lg, None, lab)
    assert torch.equal(two.cm, 2 * one.cm) and int(two.ce_sums[1]) == 2 * int(one.ce_sums[1])
    assert float(two.ce_sums[0]) == 2 * float(one.ce_sums[0])  # x + x is exact
    assert len(two._seg_ws) == 1


@pytest.mark.parametrize("low", R.LOWS, ids=_name)
@pytest.mark.parametrize("si", [0, 1, 5], ids=["x16", "odd", "near_one"])
def test_at_19_classes_the_new_entry_point_agrees_with_the_old(si, low):
    K, shape = 19, R.SHAPES[si]
    new = run_seg(K, shape, low, torch.int64)
    old = run_seg(K, shape, low, torch.int64, entry="dclip_upsample_eval_seg")
    amb = check_class_map(new[0], K, shape, low)
    check_class_map(old[0], K, shape, low)
    assert new[3] == old[3]
    assert torch.equal(new[0][~amb], old[0][~amb])
    B, h, w, H, W = shape
    lab = R.labels(B, K, H, W)
    keep = R.valid_labels(lab, K) & ~amb
    cells = lambda p: torch.bincount((lab * K + p.long())[keep], minlength=K * K).view(K, K)  # noqa: E731
    moved = lambda p: torch.bincount((lab * K + p.long())[R.valid_labels(lab, K) & amb], minlength=K * K).view(K, K)  # noqa: E731
    assert torch.equal(new[1] - moved(new[0]), cells(new[0])) and torch.equal(cells(new[0]), cells(old[0]))
    assert torch.equal(old[1] - moved(old[0]), cells(old[0]))
    u, _, _ = seg_reference(K, shape, low)
    ce64 = R.ce_sum(u, lab, K)
    assert R.rel(new[2], ce64) <= 4 * REF_FP32_DEPARTURE_CE and R.rel(old[2], ce64) <= 4 * REF_FP32_DEPARTURE_CE


# ----------------------------------------------------------------------------- fused CE
CE_SHAPES = [((8, 16), (128, 256)), ((7, 9), (20, 13)), ((5, 33), (41, 100)), ((16, 40), (12, 25))]  # the last: down
# scales above x16: low-res column (row) 0 also owns the outputs whose source is clamped at 0, about
# 1.5 W / w of them, the widest band a thread walks: x32, x25 / x26.2 with odd sizes, one low-res pixel
CE_WIDE = [((2, 3), (64, 96)), ((4, 5), (100, 131)), ((1, 1), (40, 50))]


def ce_inputs(K, hw, HW, ldt):
    g = torch.Generator().manual_seed(5)
    B = 2
    lg = (torch.randn(B, K, *hw, generator=g) * 3).to(ldt)
    lab = torch.randint(0, K, (B, *HW), generator=g)
    lab[torch.rand(B, *HW, generator=g) < 0.1] = 255
    return lg.to(DEV), lab.to(DEV)


def ce_reference(lg, lab):
    """(mean CE, its gradient wrt the low-res logits) in fp64 on the logits' values"""
    lr = lg.detach().double().requires_grad_(True)
    ref = F.cross_entropy(F.interpolate(lr, size=lab.shape[-2:], mode="bilinear", align_corners=False), lab,
                          ignore_index=255)
    ref.backward()
    return float(ref.detach()), lr.grad


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("hw,HW", CE_SHAPES + CE_WIDE)
@pytest.mark.parametrize("ldt", [torch.float32, torch.bfloat16], ids=_name)
def test_upsample_ce_vs_fp64_and_repeats_bitwise(K, hw, HW, ldt):
    from denseclip_vit_multimodal_amd import ops
    lg, lab = ce_inputs(K, hw, HW, ldt)
    ref, gref = ce_reference(lg, lab)
    runs = []
    for _ in range(2):
        x = lg.clone().requires_grad_(True)
        n0 = ops.STATS.get("upsample_ce_classes", 0)
        loss = ops.UpsampleCEFn.apply(x, lab, 255)
        assert ops.STATS.get("upsample_ce_classes", 0) == n0 + 1
        loss.backward()
        runs.append((loss.detach(), x.grad))
    (l0, g0), (l1, g1) = runs
    err_l, err_g = abs(float(l0) - ref) / abs(ref), rel_err(g0.float(), gref)
    print(f"loss {float(l0)!r} vs fp64 {ref!r}: rel {err_l:.2e}; gradient rel_err {err_g:.2e}")
    assert err_l <= 1e-5, err_l
    assert err_g <= (1e-5 if ldt == torch.float32 else 1e-2), err_g
    assert bitwise_equal(l0, l1) and bitwise_equal(g0, g1)


def run_ce(K, hw, HW, ldt, lg, lab, entry="dclip_upsample_ce_classes", start=(1.5, 3, 0.25)):
    """a CE entry point through run_poisoned: (loss_sum, count, grad) minus the start values"""
    B, (h, w), (H, W) = lg.shape[0], hw, HW
    a, b = guarded_copy(lg), guarded_copy(lab)
    loss, cnt, grad = guarded(1, torch.float64), guarded(1, torch.int32), guarded((B, K, h, w), torch.float32)
    query = "dclip_upsample_ce_classes_ws_floats" if "classes" in entry else "dclip_upsample_ws_floats"
    ws = guarded(int(getattr(_lib(), query)(B, K, h, w)), torch.float32)

    def fn():
        loss.t.fill_(start[0]); cnt.t.fill_(start[1]); grad.t.fill_(start[2])  # noqa: E702
        _call(entry, LOW_DT[ldt], a.ptr(), B, K, h, w, b.ptr(), LAB_DT[lab.dtype], H, W, 255, loss.ptr(), cnt.ptr(),
              grad.ptr(), ws.ptr(), _stream())

    ls, n, g = run_poisoned(fn, inputs=[a, b], scratch=[ws], accum=[loss, cnt, grad])
    return float(ls.cpu()) - start[0], int(n.cpu()) - start[1], g.double() - start[2]


@pytest.mark.parametrize("K", [33, 150])
@pytest.mark.parametrize("hw,HW", [CE_SHAPES[0], CE_SHAPES[2], CE_WIDE[0]])
def test_ce_accumulates_on_poisoned_buffers(K, hw, HW):
    lg, lab = ce_inputs(K, hw, HW, torch.float32)
    ls, n, g = run_ce(K, hw, HW, torch.float32, lg, lab)
    ref, gref = ce_reference(lg, lab)
    valid = int((lab != 255).sum())
    assert n == valid
    assert abs(ls / valid - ref) <= 1e-5 * abs(ref)
    # adding onto the start value 0.25 rounds each f32 element once more: 2^-24 (|g| + 0.25) at most
    slack = 2.0 ** -24 * (float(g.norm()) + 0.25 * g.numel() ** 0.5) / valid
    assert float((g / valid - gref).norm()) <= 1e-5 * float(gref.norm()) + slack


@pytest.mark.parametrize("K", [2, 150])
def test_all_labels_ignored_gives_nan_loss_and_zero_gradient(K):
    from denseclip_vit_multimodal_amd import ops
    lg, lab = ce_inputs(K, (5, 33), (41, 100), torch.float32)
    x = lg.clone().requires_grad_(True)
    loss = ops.UpsampleCEFn.apply(x, torch.full_like(lab, 255), 255)
    loss.backward()
    assert bool(torch.isnan(loss)) and int(torch.count_nonzero(x.grad)) == 0


@pytest.mark.parametrize("ldt", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("hw,HW", CE_SHAPES + CE_WIDE)
def test_ce_at_19_classes_agrees_with_the_19_class_kernel(hw, HW, ldt):
    K = 19
    lg, lab = ce_inputs(K, hw, HW, ldt)
    new = run_ce(K, hw, HW, ldt, lg, lab, start=(0.0, 0, 0.0))
    old = run_ce(K, hw, HW, ldt, lg, lab, entry="dclip_upsample_ce", start=(0.0, 0, 0.0))
    assert new[1] == old[1]
    assert abs(new[0] - old[0]) <= 1e-5 * abs(old[0])
    assert rel_err(new[2], old[2]) <= (1e-5 if ldt == torch.float32 else 1e-2)


# ----------------------------------------------------------------------------- score map
SCORE_CASES = [(2, 333, 512, 33, False), (2, 40, 512, 150, True), (1, 31, 64, 256, False), (1, 64, 1024, 171, True)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize("B,HW,C,K,tok", SCORE_CASES)
def test_score_map_classes(dt, B, HW, C, K, tok):
    """plain pixel rows and token-buffer rows (a NaN CLS row first in every image) against fp32 torch on the
    same 16-bit values; one all-zero pixel row; class rows past K never written; bitwise repeatable"""
    g = torch.Generator().manual_seed(11)
    v = torch.randn(B, HW, C, generator=g).to(dt)
    v[B - 1, HW // 2] = 0
    t = torch.randn(B, K, C, generator=g)
    off = 1 if tok else 0
    rows, bstride = guarded_rows_copy(v.to(DEV), C, off)
    gt = guarded_copy(t.to(DEV))
    score = guarded((B, K, HW), torch.float32)

    def fn():
        _call("dclip_score_map_classes", rows.ptr(), LOW_DT[dt], bstride, off, C, gt.ptr(), score.ptr(), B, HW, C, K,
              1e-12, _stream())

    (s,) = run_poisoned(fn, inputs=[rows, gt], outputs=[score])
    ref = torch.einsum("bpc,bkc->bkp", F.normalize(v.float(), dim=2), F.normalize(t, dim=2))
    err = rel_err(s, ref)
    print(f"score map rel_err {err:.2e}")
    assert err < (4e-3 if dt == torch.bfloat16 else 1e-3)
    assert int(torch.count_nonzero(s[B - 1, :, HW // 2])) == 0  # exactly 0 in every class tile
    from denseclip_vit_multimodal_amd import ops
    n0 = ops.STATS.get("score_map_classes", 0)
    again = ops.score_map(rows.t.view(-1, C), gt.t, B, HW, row_off=off, bstride=bstride)
    assert ops.STATS.get("score_map_classes", 0) == n0 + 1 and bitwise_equal(again.view(B, K, HW), s)


def test_score_map_classes_equals_the_32_class_kernel_on_its_range():
    B, HW, C, K = 2, 77, 512, 32
    g = torch.Generator().manual_seed(12)
    v = torch.randn(B * HW, C, generator=g).to(torch.bfloat16).to(DEV)
    t = torch.randn(B, K, C, generator=g).to(DEV)
    ops = torch.ops
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    old = ops.dclip.score_map(v, HW * C, 0, C, t, B, HW, 1e-12)
    new = ops.dclip_classes.score_map(v, HW * C, 0, C, t, B, HW, 1e-12)
    assert rel_err(new, old) < 1e-6


# ----------------------------------------------------------------------------- model
NAMES_150 = [CITYSCAPES_CLASSES[i % len(CITYSCAPES_CLASSES)] for i in range(150)]


def build_150(cfg, name, depth=True, cdt=torch.bfloat16):
    """`cfg` with 150 classes (the Cityscapes names cycled), the spec weights wherever the shapes allow
    (the classifier is resized, so it keeps its seeded initialisation)"""
    from denseclip_vit_multimodal_amd import DenseCLIP
    torch.manual_seed(0)
    cfg = dict(cfg, decode_head=dict(cfg["decode_head"], num_classes=150))
    if not depth:
        cfg.pop("depth_head")
    m = DenseCLIP(class_names=NAMES_150, **cfg)
    own = m.state_dict()
    sd = {k: v for k, v in spec_state_dict(name).items() if k in own and own[k].shape == v.shape}
    assert len(sd) > 20
    m.load_state_dict(sd, strict=False)
    m.backbone.compute_dtype = cdt
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def mid150():
    return build_150(MID_CFG, "mid")


def unfused(model, img, size):
    """(low-res logits, torch's class map of their fp32 resize, ambiguous pixels of the fp64 resize)"""
    with torch.no_grad():
        low = model.forward_lowres(img)["seg"].float()
    h, w = low.shape[-2:]
    up = F.interpolate(low, size=size, mode="bilinear", align_corners=False)
    u = R.resize(low.cpu(), *size)
    top = u.topk(2, dim=1).values
    amb = (top[:, 0] - top[:, 1]) < R.tau(low.cpu(), h, w)
    return low, up, amb.to(DEV)


def test_predict_and_validate_match_the_unfused_sequence(mid150):
    from denseclip_vit_multimodal_amd import evaluate, ops
    from denseclip_vit_multimodal_amd.train import synth_batch
    img, seg, depth, mask = synth_batch(1, 128, 256, torch.device(DEV), image_dtype=torch.float32, num_classes=150)
    n0 = ops.STATS.get("score_map_classes", 0)
    out = evaluate.predict(mid150, img)
    assert ops.STATS.get("score_map_classes", 0) == n0 + 1
    low, up, amb = unfused(mid150, img, (128, 256))
    assert low.shape[1] == 150 and out["seg"].dtype == torch.uint8 and out["seg"].shape == (1, 128, 256)
    # the comparison below takes the kernel's pick on the ambiguous pixels, so they must stay few: these
    # seeded weights and images give 1.8e-4 (6 of 32768 pixels); capped at the kernel tests' 3e-3
    print(f"ambiguous {float(amb.float().mean()):.2e}")
    assert float(amb.float().mean()) <= AMBIGUOUS_MAX
    want = up.argmax(1)
    assert torch.equal(out["seg"].long()[~amb], want[~amb])
    assert out["depth"].shape == (1, 1, 128, 256)
    got = evaluate.validate(mid150, [(img, seg, depth, mask)])
    # compute_segmentation_metrics' counts from torch's class map, the kernel's pick on the ambiguous pixels
    pred = torch.where(amb, out["seg"].long(), want)
    valid = (seg != 255) & (seg >= 0) & (seg < 150)
    cm = torch.bincount((seg * 150 + pred)[valid], minlength=150 * 150).view(150, 150).cpu()
    assert torch.equal(torch.as_tensor(got["confusion_matrix"]), cm)
    ref = evaluate.metrics_from_sums(cm=cm.numpy())
    assert abs(got["mean_iou"] - ref["mean_iou"]) <= 1e-6 and abs(got["accuracy"] - ref["accuracy"]) <= 1e-6
    ce = float(F.cross_entropy(F.interpolate(low.double(), size=(128, 256), mode="bilinear", align_corners=False), seg,
                               ignore_index=255))
    assert abs(got["loss_seg"] - ce) <= 1e-6 * abs(ce)
    assert got["rmse"] is not None


def test_fused_head_loss_matches_materialised_at_150_classes():
    """test_gpu_parity.test_fused_head_loss_matches_materialised at K = 150, with its tolerances"""
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.train import loss_fn, synth_batch
    m = build_150(TINY_CFG, "tiny")
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    for p in m.parameters():
        p.requires_grad_(True)
    img, seg, depth, mask = synth_batch(2, 64, 128, DEV, image_dtype=torch.float32, num_classes=150)
    res = []
    for fused in (False, True):
        m.fused_head_loss = fused
        m.zero_grad(set_to_none=True)
        n0 = ops.STATS.get("upsample_ce_classes", 0)
        out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
        loss = loss_fn(out, seg, depth, mask)
        assert ops.STATS.get("upsample_ce_classes", 0) == n0 + int(fused)
        loss.backward()
        res.append((float(loss.detach()), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = res
    assert abs(l0 - l1) < 1e-4 * abs(l0), (l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 20
    for k in g0:
        assert rel_err(g1[k], g0[k]) < (2e-2 if k.startswith("backbone.") else 2e-3), k


def test_seg_only_model_trains_validates_and_replays():
    """no depth head, no depth targets (the ADE20K case): two steps on one batch with a finite loss
    that does not rise, validate without depth targets, and CapturedEval's replay"""
    from denseclip_vit_multimodal_amd import evaluate
    from denseclip_vit_multimodal_amd.serve import CapturedEval
    from denseclip_vit_multimodal_amd.train import freeze_for_mode, make_optimizer, synth_batch, train_step
    m = build_150(MID_CFG, "mid", depth=False)
    assert m.depth_head is None
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    m.fused_head_loss = True
    opt = make_optimizer(freeze_for_mode(m, "F"))
    img, seg, _, _ = synth_batch(1, 128, 256, torch.device(DEV), image_dtype=torch.float32, num_classes=150)
    batch = (img, seg, None, None)
    losses = [float(train_step(m, opt, batch)) for _ in range(2)]
    print(f"losses {losses}")
    assert all(map(lambda v: v == v and abs(v) != float("inf"), losses)) and losses[1] <= losses[0], losses
    got = evaluate.validate(m, [batch])
    assert got["loss_seg"] is not None and 0.0 <= got["mean_iou"] <= 1.0 and "rmse" in got and got["rmse"] is None
    m.eval()
    want = evaluate.predict(m, img)
    assert want["depth"] is None
    cap = CapturedEval(m, img)
    other = images(1, 128, 256, seed=4321).to(DEV)
    first = cap(other)["seg"].clone()
    assert torch.equal(cap(img)["seg"], want["seg"]) and cap(img)["depth"] is None
    assert torch.equal(first, evaluate.predict(m, other)["seg"])


def test_seg_only_captured_train_step_equals_eager():
    """train.CapturedTrainStep on batches (img, seg, None, None) of the seg-only 150-class model: three
    warm-up steps and two replays give the losses of five eager steps (the fused CE repeats bit for bit)"""
    from denseclip_vit_multimodal_amd.train import (CapturedTrainStep, freeze_for_mode, make_optimizer, synth_batch,
                                                    train_step)

    def make():
        m = build_150(MID_CFG, "mid", depth=False).train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        m.fused_head_loss = True
        return m, make_optimizer(freeze_for_mode(m, "F"), capturable=True)

    batches = []
    for rank in (0, 1):
        img, seg, _, _ = synth_batch(1, 128, 256, torch.device(DEV), rank, image_dtype=torch.float32, num_classes=150)
        batches.append((img, seg, None, None))
    b1, b2 = batches
    ma, oa = make()
    la = [float(train_step(ma, oa, b)) for b in (b1, b1, b1, b2, b1)]
    mb, ob = make()
    cap = CapturedTrainStep(mb, ob, b1)
    lb = [float(cap(b2)), float(cap(b1))]
    torch.cuda.synchronize()
    print(f"eager {la}, captured {lb}")
    assert lb == la[3:], (lb, la)
    with pytest.raises(ValueError, match="absent"):
        cap((b1[0], b1[1], torch.zeros(1, 1, 128, 256, device=DEV), None))
