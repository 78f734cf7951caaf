"""The fused on-device validation path (csrc/headeval.hip -> torch.ops.dclip_eval -> evaluate.py) on
the GPU.  C-ABI calls run on guard-banded buffers (abi_guard.run_poisoned): outputs and workspace
pre-filled with 0xFF and then 0x3C must give equal results, guards intact, and the accumulating
arguments are checked from a non-zero start.

Class map: the reference u is F.interpolate of the logits' values in fp64 on the CPU.  A pixel is
ambiguous when its top-2 gap in u is below tau = 2^-24 max|L| (32 + 8 (h + w)) (fp32 summation order
plus the rounding of the fp32 source coordinate; torch's own fp32 CPU resize stays within 0.14 tau of
u on these shapes and disagrees with the fp64 argmax on no pixel).  Every other pixel must equal
argmax u, an ambiguous one must pick a class within tau of the maximum, and at most 0.1 % of a case's
pixels may be ambiguous (the inputs alone give at most 5.4e-4; the identity case is excluded: there
the map must equal argmax of the input exactly).

Floating sums: measured on the CPU over these inputs (the first six shapes of eval_ref.SHAPES, every
low dtype, mask and clamp setting below; the seventh shape, added for the kernel's narrow-tile path,
only raises the figures and is held to the same ones), the reference's own fp32 path (F.interpolate fp32 -> the formulas of compute_depth_errors /
SILogLoss / F.cross_entropy in fp32) departs from the fp64 evaluation of the same formulas by at most
    CE sum 1.04e-7, sum (gt-p)^2 1.07e-7, sum (log gt - log p)^2 2.72e-7, sum |gt-p|/gt 1.47e-7,
    sum (gt-p)^2/gt 1.98e-7, masked sum (gt-up)^2 9.09e-8, sum d 2.29e-7, sum d^2 1.48e-7
relative (REF_FP32_DEPARTURE).  The kernel keeps fp32 per-pixel terms but sums in f64 and is allowed
4x these figures.  Threshold counts must lie between the fp64 counts at t (1 - 1e-5) and t (1 + 1e-5).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import eval_ref as R
from abi_guard import guarded, guarded_copy, run_poisoned
from helpers import MID_CFG, CITYSCAPES_CLASSES, ROOT, images, spec_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = R.K
REF_FP32_DEPARTURE = {"ce": 1.04e-7, "sq": 1.07e-7, "log_sq": 2.72e-7, "abs_rel": 1.47e-7, "sq_rel": 1.98e-7,
                      "mask_sq": 9.09e-8, "d": 2.29e-7, "d_sq": 1.48e-7}
LOW_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
LAB_DT = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
LOWS = [torch.bfloat16, torch.float16, torch.float32]
LABS = [torch.int64, torch.int32, torch.uint8]
_name = lambda d: str(d).replace("torch.", "")  # noqa: E731


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def _call(name, *args):
    from denseclip_vit_multimodal_amd import _native as N
    return N.call(name, *args)


def _ws(B, k, h, w):
    from denseclip_vit_multimodal_amd import _native as N
    return guarded(int(N.lib().dclip_upsample_eval_ws_bytes(B, k, h, w)))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def seg_reference(shape, low):
    """(u fp64 (B, K, H, W), tau) of the case's logits as the low dtype holds them"""
    B, h, w, H, W = shape
    L = R.logits(B, h, w, low)
    return R.resize(L, H, W), R.tau(L.float(), h, w)


def check_class_map(pred, shape, low, identity=False):
    """pred (B, H, W) uint8 on the CPU against the fp64 resize; returns the ambiguous pixels' mask"""
    B, h, w, H, W = shape
    u, tau = seg_reference(shape, low)
    top = u.topk(2, dim=1).values
    amb = (top[:, 0] - top[:, 1]) < tau
    p = pred.long()
    if identity:
        assert torch.equal(p, R.logits(B, h, w, low).float().argmax(1)), "identity resize: argmax of the input"
        return amb
    frac = float(amb.float().mean())
    print(f"ambiguous {frac:.2e} (tau {tau:.3e})")
    assert frac <= 1e-3, frac
    want = u.argmax(1)
    wrong = (p != want) & ~amb
    assert not bool(wrong.any()), f"{int(wrong.sum())} unambiguous pixels differ from argmax of the fp64 resize"
    picked = u.gather(1, p.unsqueeze(1))[:, 0]
    assert bool((top[:, 0] - picked <= tau).all()), "an ambiguous pixel picked a class further than tau from the maximum"
    return amb


def run_seg(shape, low, labdt, start=(5, 1.5, 3)):
    """dclip_upsample_eval_seg through run_poisoned; returns (pred, cm, loss_sum, count) minus the start values"""
    B, h, w, H, W = shape
    lg = guarded_copy(R.logits(B, h, w, low).to(DEV))
    lab = guarded_copy(R.labels(B, H, W, labdt).to(DEV))
    pred = guarded((B, H, W), torch.uint8)
    cm, loss, cnt = guarded((K, K), torch.int64), guarded(1, torch.float64), guarded(1, torch.int64)
    ws = _ws(B, K, h, w)

    def fn():
        cm.t.fill_(start[0]); loss.t.fill_(start[1]); cnt.t.fill_(start[2])  # noqa: E702
        _call("dclip_upsample_eval_seg", LOW_DT[low], lg.ptr(), B, K, h, w, lab.ptr(), LAB_DT[labdt], H, W, R.IGNORE,
              pred.ptr(), cm.ptr(), loss.ptr(), cnt.ptr(), ws.ptr(), _stream())

    p, c, ls, n = run_poisoned(fn, inputs=[lg, lab], outputs=[pred], scratch=[ws], accum=[cm, loss, cnt])
    return p.cpu(), c.cpu() - start[0], float(ls.cpu()) - start[1], int(n.cpu()) - start[2]


@pytest.mark.parametrize("labdt", LABS, ids=_name)
@pytest.mark.parametrize("low", LOWS, ids=_name)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_seg_class_map_confusion_matrix_count_and_ce(shape, low, labdt):
    B, h, w, H, W = shape
    pred, cm, loss, count = run_seg(shape, low, labdt)
    check_class_map(pred, shape, low, identity=(h, w) == (H, W))
    lab = R.labels(B, H, W, labdt)
    valid = R.valid_labels(lab)
    assert int(valid.sum()) < lab.numel()  # ignore / out-of-range labels are present ...
    want = torch.bincount((lab.long() * K + pred.long())[valid], minlength=K * K).view(K, K)
    assert torch.equal(cm, want)  # ... and contribute nothing; the kernel's own class map otherwise, exactly
    assert count == int(valid.sum())
    u, _ = seg_reference(shape, low)
    ce64 = R.ce_sum(u, lab)
    err = R.rel(loss, ce64)
    print(f"CE sum {loss!r} vs fp64 {ce64!r}: rel {err:.2e}")
    assert err <= 4 * REF_FP32_DEPARTURE["ce"], err


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[1], R.SHAPES[5]], ids=["x16", "odd", "identity"])
def test_tie_takes_the_lower_class(shape):
    """two channels identical everywhere and above every other: the lower index everywhere"""
    from denseclip_vit_multimodal_amd.evaluate import upsample_argmax
    B, h, w, H, W = shape
    L = R.logits(B, h, w).clone()
    L[:, 11] = L[:, 4] = L.amax(1) + 1.0
    pred = upsample_argmax(L.to(DEV), (H, W))
    assert pred.dtype == torch.uint8 and bool((pred == 4).all())


@pytest.mark.parametrize("low", LOWS, ids=_name)
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[1]], ids=["x16", "odd"])
def test_labels_null_gives_the_same_class_map(shape, low):
    B, h, w, H, W = shape
    lg = guarded_copy(R.logits(B, h, w, low).to(DEV))
    pred = guarded((B, H, W), torch.uint8)

    def fn():
        _call("dclip_upsample_eval_seg", LOW_DT[low], lg.ptr(), B, K, h, w, None, 0, H, W, R.IGNORE, pred.ptr(), None,
              None, None, None, _stream())

    (p,) = run_poisoned(fn, inputs=[lg], outputs=[pred])
    check_class_map(p.cpu(), shape, low)
    from denseclip_vit_multimodal_amd.evaluate import _E
    E = _E()
    cm = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ce = torch.zeros(2, dtype=torch.float64, device=DEV)
    lab = R.labels(B, H, W).to(DEV)
    with_labels = E.seg_update(lg.t, lab, R.IGNORE, cm, ce, True)
    assert torch.equal(E.upsample_argmax(lg.t, H, W), with_labels) and torch.equal(with_labels, p)
    assert E.seg_update(lg.t, lab, R.IGNORE, cm, ce, False) is None
    assert int(cm.sum()) == 2 * int(R.valid_labels(lab).sum()) == int(ce[1])


def check_depth_sums(got, up64, gt, mask, clamp, dmin=1e-3, dmax=80.0):
    want = R.depth_sums(up64, gt, mask, dmin, dmax, clamp)
    lo = R.depth_sums(up64, gt, mask, dmin, dmax, clamp, thr_scale=1 - 1e-5)
    hi = R.depth_sums(up64, gt, mask, dmin, dmax, clamp, thr_scale=1 + 1e-5)
    assert got[0] == want[0] and got[8] == want[8], (got[0], want[0], got[8], want[8])
    for i in (5, 6, 7):
        assert lo[i] <= got[i] <= hi[i], (R.SUM_NAMES[i], lo[i], got[i], hi[i])
    for i in R.FLOAT_SUMS:
        err = R.rel(got[i], want[i]) if want[i] != 0 else abs(got[i])
        print(f"{R.SUM_NAMES[i]}: {got[i]!r} vs fp64 {want[i]!r}: rel {err:.2e}")
        assert err <= 4 * REF_FP32_DEPARTURE[R.SUM_NAMES[i]], (R.SUM_NAMES[i], err)


def run_depth(shape, low, mask, clamp, start=2.0, dmin=1e-3, dmax=80.0):
    B, h, w, H, W = shape
    lo = guarded_copy(R.depth_low(B, h, w, low).to(DEV))
    gt = guarded_copy(R.depth_target(B, H, W).to(DEV))
    mk = guarded_copy(mask.to(DEV)) if mask is not None else None
    up, sums, ws = guarded((B, H, W), torch.float32), guarded(12, torch.float64), _ws(B, 1, h, w)

    def fn():
        sums.t.fill_(start)
        _call("dclip_upsample_eval_depth", LOW_DT[low], lo.ptr(), B, h, w, gt.ptr(), mk.ptr() if mk else None, H, W,
              dmin, dmax, int(clamp), 1e-6, up.ptr(), sums.ptr(), ws.ptr(), _stream())

    u, s = run_poisoned(fn, inputs=[lo, gt] + ([mk] if mk else []), outputs=[up], scratch=[ws], accum=[sums])
    return u.cpu(), [float(v) - start for v in s.cpu()]


DEPTH_CASES = [(s, low, "mask", 1) for s in R.SHAPES for low in LOWS] + \
              [(s, torch.float32, m, c) for s in R.SHAPES[:2] for m, c in (("mask", 0), ("none", 0), ("none", 1),
                                                                           ("empty", 1), ("empty", 0))]


@pytest.mark.parametrize("shape,low,mask_kind,clamp", DEPTH_CASES,
                         ids=[f"{R.SHAPE_IDS[R.SHAPES.index(s)]}-{_name(d)}-{m}-clamp{c}" for s, d, m, c in DEPTH_CASES])
def test_depth_sums_and_resized_map(shape, low, mask_kind, clamp):
    B, h, w, H, W = shape
    mask = {"mask": R.depth_mask(B, H, W), "none": None, "empty": torch.zeros(B, H, W, dtype=torch.uint8)}[mask_kind]
    up, sums = run_depth(shape, low, mask, clamp)
    D = R.depth_low(B, h, w, low)
    u64 = R.resize(D, H, W)
    dev = float((up.double() - u64[:, 0]).abs().max())
    tau = R.tau(D.float(), h, w)
    print(f"up: max |up - u| {dev:.3e} (tau {tau:.3e})")
    assert dev <= tau
    if mask_kind == "empty":
        assert sums == [0.0] * 12
        return
    check_depth_sums(sums, u64, R.depth_target(B, H, W), mask, bool(clamp))


def test_depth_nan_prediction_reaches_the_silog_sums():
    """One NaN in the low-res prediction under the mask: sums[10] (sum d) and sums[11] (sum d^2), d as in
    dclip_upsample_silog, must not be finite -- torch.clamp in SILogLoss keeps the NaN, and a clamp
    that returns eps for it would report a finite validation loss for a diverged depth head.  The
    sliding-window and ensemble paths score through the same epilogue (eval_tile.h)."""
    shape = R.SHAPES[0]
    B, h, w, H, W = shape
    low = R.depth_low(B, h, w, torch.float32).clone()
    low.view(B, -1)[0, (h // 2) * w + w // 2] = float("nan")
    mask = R.depth_mask(B, H, W)
    u = R.resize(low, H, W)[:, 0]
    assert int((torch.isnan(u) & (mask != 0)).sum()) > 0, "no masked-in pixel reads the NaN element"
    lo, gt, mk = guarded_copy(low.to(DEV)), guarded_copy(R.depth_target(B, H, W).to(DEV)), guarded_copy(mask.to(DEV))
    up, sums, ws = guarded((B, H, W), torch.float32), guarded(12, torch.float64), _ws(B, 1, h, w)
    ws.fill(0xFF)
    _call("dclip_upsample_eval_depth", LOW_DT[torch.float32], lo.ptr(), B, h, w, gt.ptr(), mk.ptr(), H, W, 1e-3, 80.0, 1,
          1e-6, up.ptr(), sums.ptr(), ws.ptr(), _stream())
    s = sums.t.cpu()
    for g in (lo, gt, mk, up, sums, ws):
        g.check()
    print(f"NaN prediction under the mask: sum d {float(s[10])!r}, sum d^2 {float(s[11])!r}, n_mask {float(s[8])!r}")
    assert float(s[8]) == float((mask != 0).sum())
    assert not bool(torch.isfinite(s[10])) and not bool(torch.isfinite(s[11]))


def _evaluator_on_fixture():
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
    t = {k: torch.from_numpy(g[k]).to(DEV) for k in ("logits", "depth", "labels", "depth_target", "depth_mask")}
    ev = Evaluator(device=DEV)
    return g, t, ev


def test_fixture_end_to_end():
    """Evaluator.update on the fixture's inputs, compute() against the reference's recorded metrics:
    the floating metrics within 4x REF_FP32_DEPARTURE of the recorded value (the metric's sum; a root
    halves the relative error, the same bound is kept), a1..a3 by the threshold-count rule, the
    confusion matrix different from the recorded one only at ambiguous pixels."""
    from denseclip_vit_multimodal_amd.evaluate import upsample_argmax
    g, t, ev = _evaluator_on_fixture()
    assert ev.update(t["logits"], t["depth"], t["labels"], t["depth_target"], t["depth_mask"]) is None
    m = ev.compute()
    shape = R.SHAPES[0]
    assert torch.equal(t["logits"].cpu(), R.logits(*shape[:3]))  # the generator's inputs are eval_ref's
    amb = check_class_map(upsample_argmax(t["logits"], shape[3:]).cpu(), shape, torch.float32)
    l1 = int(np.abs(m["confusion_matrix"] - g["confusion_matrix"]).sum())
    assert l1 <= 2 * int(amb.sum()), (l1, int(amb.sum()))
    assert int(m["confusion_matrix"].sum()) == int(g["confusion_matrix"].sum())
    for key, src in (("loss_seg", "ce"), ("rmse", "sq"), ("rmse_log", "log_sq"), ("abs_rel", "abs_rel"),
                     ("sq_rel", "sq_rel"), ("rmse_masked", "mask_sq")):
        err = R.rel(m[key], float(g[key]))
        print(f"{key}: {m[key]!r} vs recorded {float(g[key])!r}: rel {err:.2e}")
        assert err <= 4 * REF_FP32_DEPARTURE[src], (key, err)
    if l1 == 0:
        for key in ("accuracy", "mean_iou"):
            assert R.rel(m[key], float(g[key])) <= 1e-6, key
    u64 = R.resize(R.depth_low(*shape[:3]), *shape[3:])
    gt, mask = R.depth_target(shape[0], *shape[3:]), R.depth_mask(shape[0], *shape[3:])
    n = R.depth_sums(u64, gt, mask)[0]
    lo, hi = (R.depth_sums(u64, gt, mask, thr_scale=s) for s in (1 - 1e-5, 1 + 1e-5))
    for i, key in ((5, "a1"), (6, "a2"), (7, "a3")):
        assert lo[i] / n <= m[key] <= hi[i] / n, key
        assert abs(m[key] - float(g[key])) <= (hi[i] - lo[i] + 1) / n, key


def test_updates_are_deterministic_and_additive():
    g, t, ev = _evaluator_on_fixture()
    args = (t["logits"], t["depth"], t["labels"], t["depth_target"], t["depth_mask"])
    ev.update(*args)
    one = [x.clone() for x in (ev.cm, ev.ce_sums, ev.depth_sums)]
    ev.reset()
    ev.update(*args)
    for a, b in zip(one, (ev.cm, ev.ce_sums, ev.depth_sums)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))  # bitwise, the floating sums too
    own = ev.update(*args, per_call=True)
    assert torch.equal(ev.cm, 2 * one[0]) and float(ev.ce_sums[1]) == 2 * float(one[1][1])
    for i in (0, 5, 6, 7, 8):
        assert float(ev.depth_sums[i]) == 2 * float(one[2][i])
    for a, b in zip(one, (own["cm"], own["ce_sums"], own["depth_sums"])):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.fixture(scope="module")
def mid_model():
    from denseclip_vit_multimodal_amd import DenseCLIP
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **MID_CFG)
    m.load_state_dict(spec_state_dict("mid"))
    m.backbone.compute_dtype = torch.float16
    return m.to(DEV).eval()


def test_model_predict_and_forward_lowres(mid_model):
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.evaluate import predict
    x = images(1, 128, 256).to(DEV)
    with torch.no_grad():
        full = mid_model(x, return_loss=False)
        low = mid_model.forward_lowres(x)
        assert low["seg"].shape[1] == K and low["depth"].shape[1] == 1 and low["seg"].shape[-1] < 256
        for k in ("seg", "depth"):
            assert torch.equal(ops.upsample(low[k], (128, 256)), full[k]), k
    out = predict(mid_model, x)
    assert out["seg"].dtype == torch.uint8 and out["seg"].shape == (1, 128, 256)
    assert torch.equal(out["depth"], full["depth"])
    h, w = low["seg"].shape[-2:]
    tau = R.tau(low["seg"].float().cpu(), h, w)
    top = full["seg"].topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) >= tau
    assert float(clear.float().mean()) > 0.9
    assert torch.equal(out["seg"].long()[clear], full["seg"].argmax(1)[clear])


def test_captured_eval_matches_eager_predict(mid_model):
    from denseclip_vit_multimodal_amd.evaluate import predict
    from denseclip_vit_multimodal_amd.serve import CapturedEval
    x1, x2 = images(1, 128, 256, seed=1).to(DEV), images(1, 128, 256, seed=2).to(DEV)
    e1, e2 = ({k: v.clone() for k, v in predict(mid_model, x).items()} for x in (x1, x2))
    assert not torch.equal(e1["depth"], e2["depth"])
    ce = CapturedEval(mid_model, x1)
    for x, e in ((x2, e2), (x1, e1)):
        out = ce(x)
        torch.cuda.synchronize()
        assert out["seg"].dtype == torch.uint8 and out["depth"].dtype == torch.float32
        for k in ("seg", "depth"):
            assert torch.equal(out[k], e[k]), k
    with pytest.raises(ValueError):
        ce(torch.cat([x1, x2]))


def test_validate_equals_evaluator_fed_by_hand(mid_model):
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, validate
    from denseclip_vit_multimodal_amd.train import synth_batch
    batches = [synth_batch(1, 128, 256, torch.device(DEV), rank=r, image_dtype=torch.float32) for r in (0, 1)]
    mid_model.train()
    got = validate(mid_model, batches)
    assert mid_model.training
    mid_model.eval()
    ev = Evaluator(device=DEV)
    with torch.no_grad():
        for img, seg, depth, mask in batches:
            low = mid_model.forward_lowres(img)
            ev.update(low["seg"], low["depth"], seg, depth, mask)
    want = ev.compute()
    assert int(want["confusion_matrix"].sum()) == sum(int((b[1] != 255).sum()) for b in batches)
    for k, v in want.items():  # NaN where an untrained depth head goes negative: equal as NaN
        if v is None:
            assert got[k] is None, k
        else:
            assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=np.asarray(v).dtype.kind == "f"), k
