"""The fused multi-scale + flip ensemble (csrc/headensemble.hip -> torch.ops.dclip_eval.ensemble_* ->
evaluate.py) on the GPU.  C-ABI calls run on guard-banded buffers (abi_guard.run_poisoned): outputs
and workspace pre-filled with 0xFF and then 0x3C must give equal results, guards intact, and the
accumulating arguments are checked from a non-zero start.

Reference (tta_ref.ensemble): fp64 on the CPU; per view F.interpolate of the values, .flip(-1) for a
flipped view, a softmax under the 'probs' rule, then the mean.

Class map: a pixel is ambiguous when its top-2 gap in the fp64 mean is below
    tau_logits = mean_v 2^-24 max|L_v| (32 + 8 (h_v + w_v)) + 2^-24 (V + 1) max|mean|
    tau_probs  = mean_v 2^-24 max|L_v| (32 + 8 (h_v + w_v)) / 4 + 2^-20.
Every other pixel must equal the fp64 argmax, an ambiguous one must pick a class within tau of the
maximum, and at most 2e-3 of a case's pixels may be ambiguous.  Measured on the CPU over these inputs
(`python tests/tta_ref.py`; every case, low dtype and rule): the ambiguous share is at most 9.19e-4
(logits) and 1.53e-3 (probs); torch's own fp32 path stays within 0.115 tau (logits) and 0.068 tau
(probs) of the fp64 mean and disagrees with the fp64 argmax on no unambiguous pixel.  The script runs
torch's scalar CPU kernels (ATEN_CPU_CAPABILITY=default), so it prints the same figures on every
machine: the vectorised kernels round differently per instruction set (the probs-rule CE departure
below comes out as 1.68e-7 under one AVX2 build and 1.10e-7 under an AVX-512 one), and for both CE
sums the scalar figure is the smallest of them, the tightest bound.

Floating sums: measured the same way (the CE sum over every case, low dtype and rule with the label
dtype paired to the low dtype; the depth sums over tta_ref.DEPTH_CASES), the reference's own fp32
path (the same torch sequence in fp32) departs from its fp64 evaluation by at most
    CE sum 9.60e-8 (logits) and 1.01e-7 (probs), sum (gt-p)^2 1.49e-7, sum (log gt - log p)^2 1.47e-7,
    sum |gt-p|/gt 2.41e-7, sum (gt-p)^2/gt 2.09e-7, masked sum (gt-up)^2 9.00e-8, sum d 6.86e-8,
    sum d^2 1.38e-7
relative (REF_FP32_DEPARTURE).  The kernel keeps fp32 per-pixel terms but sums in f64 and is allowed
4x these figures.  Threshold counts must lie between the fp64 counts at t (1 - 1e-5) and t (1 + 1e-5).
The mean depth map must agree with the fp64 mean to within tau_logits of the depth views.
"""
import ctypes

import numpy as np
import pytest
import torch

import eval_ref as R
import tta_ref as T
from abi_guard import bitwise_equal, guarded, guarded_copy, run_poisoned
from helpers import MID_CFG, CITYSCAPES_CLASSES, images, spec_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = R.K
REF_FP32_DEPARTURE = {"ce_logits": 9.60e-8, "ce_probs": 1.01e-7, "sq": 1.49e-7, "log_sq": 1.47e-7, "abs_rel": 2.41e-7,
                      "sq_rel": 2.09e-7, "mask_sq": 9.00e-8, "d": 6.86e-8, "d_sq": 1.38e-7}
LOW_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
LAB_DT = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
AVG = {"logits": 0, "probs": 1}
_name = lambda d: str(d).replace("torch.", "")  # noqa: E731


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def _N():
    from denseclip_vit_multimodal_amd import _native as N
    return N


def _call(name, *args):
    return _N().call(name, *args)


def _ws(B, k, nviews):
    return guarded(int(_N().lib().dclip_ensemble_eval_ws_bytes(B, k, nviews)))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(bufs, views, order):
    return _N().view_table([(bufs[i].ptr(), views[i][0], views[i][1], views[i][2]) for i in order])


def run_seg(case, low, rule, labdt=None, order=None, maps=None, start=(5, 1.5, 3)):
    """dclip_ensemble_eval_seg through run_poisoned; (pred, cm, loss_sum, count) minus the start values"""
    B, H, W, views = T.CASES[case]
    labdt = T.LAB_OF_LOW[low] if labdt is None else labdt
    order = list(range(len(views))) if order is None else order
    bufs = [guarded_copy(m.to(DEV)) for m in (T.seg_views(case, low) if maps is None else maps)]
    tab = _table(bufs, views, order)
    lab = guarded_copy(R.labels(B, H, W, labdt).to(DEV))
    pred = guarded((B, H, W), torch.uint8)
    cm, loss, cnt = guarded((K, K), torch.int64), guarded(1, torch.float64), guarded(1, torch.int64)
    ws = _ws(B, K, len(order))

    def fn():
        cm.t.fill_(start[0]); loss.t.fill_(start[1]); cnt.t.fill_(start[2])  # noqa: E702
        _call("dclip_ensemble_eval_seg", LOW_DT[low], tab, len(order), B, K, AVG[rule], lab.ptr(), LAB_DT[labdt], H, W,
              R.IGNORE, pred.ptr(), cm.ptr(), loss.ptr(), cnt.ptr(), ws.ptr(), _stream())

    p, c, ls, n = run_poisoned(fn, inputs=bufs + [lab], outputs=[pred], scratch=[ws], accum=[cm, loss, cnt])
    return p.cpu(), c.cpu() - start[0], float(ls.cpu()) - start[1], int(n.cpu()) - start[2]


def run_depth(case, low, mask_kind="mask", clamp=1, order=None, target=True, start=2.0, dmin=1e-3, dmax=80.0):
    """dclip_ensemble_eval_depth through run_poisoned; (up, sums minus the start value); target=False:
    prediction only (null target, mask, sums and workspace), sums None"""
    B, H, W, views = T.CASES[case]
    order = list(range(len(views))) if order is None else order
    bufs = [guarded_copy(m.to(DEV)) for m in T.depth_views(case, low)]
    tab = _table(bufs, views, order)
    up = guarded((B, H, W), torch.float32)
    if not target:
        def fn():
            _call("dclip_ensemble_eval_depth", LOW_DT[low], tab, len(order), B, None, None, H, W, dmin, dmax,
                  int(clamp), 1e-6, up.ptr(), None, None, _stream())

        (u,) = run_poisoned(fn, inputs=bufs, outputs=[up])
        return u.cpu(), None
    mask = T.mask_of(mask_kind, B, H, W)
    gt = guarded_copy(R.depth_target(B, H, W).to(DEV))
    mk = guarded_copy(mask.to(DEV)) if mask is not None else None
    sums, ws = guarded(12, torch.float64), _ws(B, 1, len(order))

    def fn():
        sums.t.fill_(start)
        _call("dclip_ensemble_eval_depth", LOW_DT[low], tab, len(order), B, gt.ptr(), mk.ptr() if mk else None, H, W,
              dmin, dmax, int(clamp), 1e-6, up.ptr(), sums.ptr(), ws.ptr(), _stream())

    u, s = run_poisoned(fn, inputs=bufs + [gt] + ([mk] if mk else []), outputs=[up], scratch=[ws], accum=[sums])
    return u.cpu(), [float(v) - start for v in s.cpu()]


# ----------------------------------------------------------------------------- 1. cases x dtypes x rules
@pytest.mark.parametrize("rule", T.RULES)
@pytest.mark.parametrize("low", T.LOWS, ids=_name)
@pytest.mark.parametrize("case", list(T.CASES))
def test_seg_class_map_confusion_matrix_count_and_ce(case, low, rule):
    B, H, W, views = T.CASES[case]
    pred, cm, loss, count = run_seg(case, low, rule)
    u, tau = T.seg_reference(case, low, rule)
    T.check_class_map(pred, u, tau)
    lab = R.labels(B, H, W, T.LAB_OF_LOW[low])
    valid = R.valid_labels(lab)
    assert int(valid.sum()) < lab.numel()  # ignore / out-of-range labels are present ...
    want = torch.bincount((lab.long() * K + pred.long())[valid], minlength=K * K).view(K, K)
    assert torch.equal(cm, want)  # ... and contribute nothing; the kernel's own class map otherwise, exactly
    assert count == int(valid.sum())
    ce64 = T.ce_sum(u, lab, rule)
    err = R.rel(loss, ce64)
    print(f"CE sum {loss!r} vs fp64 {ce64!r}: rel {err:.2e}")
    assert err <= 4 * REF_FP32_DEPARTURE["ce_" + rule], err


# ----------------------------------------------------------------------------- 2. one plain view
@pytest.mark.parametrize("low", T.LOWS, ids=_name)
def test_single_plain_view_seg_equals_the_single_view_kernel(low):
    """one plain view under the logits rule: the class map, the confusion matrix and the count of
    dclip_upsample_eval_seg, bitwise (the CE sums are printed: the segmentation kernel fixes one
    fusion of the interpolation for every pixel slot, the single-view kernel leaves it to the compiler,
    and the sums need not be bitwise equal)"""
    B, H, W, ((h, w, _),) = T.CASES["single"]
    labdt = T.LAB_OF_LOW[low]
    pred, cm, loss, count = run_seg("single", low, "logits", start=(0, 0.0, 0))
    N = _N()
    lg = T.seg_view(0, B, h, w, low).to(DEV)
    lab = R.labels(B, H, W, labdt).to(DEV)
    p1 = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
    cm1 = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ls1, n1 = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    ws1 = torch.empty(int(N.lib().dclip_upsample_eval_ws_bytes(B, K, h, w)), dtype=torch.uint8, device=DEV)
    _call("dclip_upsample_eval_seg", LOW_DT[low], lg.data_ptr(), B, K, h, w, lab.data_ptr(), LAB_DT[labdt], H, W,
          R.IGNORE, p1.data_ptr(), cm1.data_ptr(), ls1.data_ptr(), n1.data_ptr(), ws1.data_ptr(), _stream())
    assert torch.equal(pred, p1.cpu()) and torch.equal(cm, cm1.cpu()) and count == int(n1)
    print(f"CE sum {loss!r} vs single-view {float(ls1)!r}: rel {R.rel(loss, float(ls1)):.2e}")


@pytest.mark.parametrize("low", T.LOWS, ids=_name)
def test_single_plain_view_depth_equals_the_single_view_kernel(low):
    """one plain view: `up` and the 12 sums of dclip_upsample_eval_depth, bitwise.

    headeval.hip leaves the fusion of Y.l0 (X.l0 a00 + X.l1 a01) + Y.l1 (...) to the compiler, whose
    gfx950 code does not fuse a thread's four pixels alike; headensemble.hip spells out the same
    fused multiply-adds per pixel slot (bilerp_depth).  A failure here with differences of an ulp or
    two means headeval.hip compiles to other fusions than bilerp_depth states."""
    B, H, W, ((h, w, _),) = T.CASES["single"]
    N = _N()
    up, sums = run_depth("single", low, start=0.0)
    d = T.depth_view(0, B, h, w, low).to(DEV)
    gt, mk = R.depth_target(B, H, W).to(DEV), R.depth_mask(B, H, W).to(DEV)
    up1 = torch.empty(B, H, W, device=DEV)
    s1 = torch.zeros(12, dtype=torch.float64, device=DEV)
    wsd = torch.empty(int(N.lib().dclip_upsample_eval_ws_bytes(B, 1, h, w)), dtype=torch.uint8, device=DEV)
    _call("dclip_upsample_eval_depth", LOW_DT[low], d.data_ptr(), B, h, w, gt.data_ptr(), mk.data_ptr(), H, W, 1e-3,
          80.0, 1, 1e-6, up1.data_ptr(), s1.data_ptr(), wsd.data_ptr(), _stream())
    up1, s1 = up1.cpu(), [float(v) for v in s1.cpu()]
    ulp = (up.view(torch.int32).long() - up1.view(torch.int32).long()).abs()
    print(f"up: {int((ulp > 0).sum())} of {ulp.numel()} values differ, by at most {int(ulp.max())} ulp")
    print("sums rel:", {R.SUM_NAMES[i]: f"{R.rel(sums[i], s1[i]) if s1[i] else abs(sums[i]):.2e}" for i in range(12)})
    assert bitwise_equal(up, up1)
    assert sums == s1  # from a zero start on both sides: bitwise


# ----------------------------------------------------------------------------- 3. the flip is the mirror
@pytest.mark.parametrize("rule", T.RULES)
@pytest.mark.parametrize("low", T.LOWS, ids=_name)
def test_single_flipped_view_is_the_column_mirror(low, rule):
    """the same map as `single`, flagged flipped: the same arithmetic at column W-1-x"""
    assert torch.equal(T.seg_views("single", low)[0], T.seg_views("single_flip", low)[0])
    plain = run_seg("single", low, rule)[0]
    flipped = run_seg("single_flip", low, rule)[0]
    assert torch.equal(flipped, plain.flip(-1))
    assert not torch.equal(flipped, plain)
    up_plain, up_flipped = run_depth("single", low)[0], run_depth("single_flip", low)[0]
    assert bitwise_equal(up_flipped, up_plain.flip(-1).contiguous())


@pytest.mark.parametrize("W", [301, 302, 303, 304])
def test_flipped_depth_is_the_mirror_at_every_width_residue(W):
    """the depth kernel keeps a source column in the pixel slot column % 4, flipped or not, and which
    slot that is depends on W % 4: every residue, through the op"""
    from denseclip_vit_multimodal_amd.evaluate import _E
    d = [T.depth_view(0, 1, 5, 37).to(DEV)]
    plain, flipped = _E().ensemble_depth(d, [0], 43, W), _E().ensemble_depth(d, [1], 43, W)
    assert bitwise_equal(flipped, plain.flip(-1).contiguous()) and not torch.equal(flipped, plain)


# ----------------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("rule", T.RULES)
@pytest.mark.parametrize("case", ["ms_flip", "odd", "identity_pair", "narrow_tile"])
def test_tie_takes_the_lower_class(case, rule):
    """two channels identical in every view and above every other: the lower index everywhere"""
    from denseclip_vit_multimodal_amd.evaluate import _E
    B, H, W, views = T.CASES[case]
    maps = []
    for m in T.seg_views(case, torch.float32):
        m = m.clone()
        m[:, 11] = m[:, 4] = m.amax(1) + 1.0
        maps.append(m.to(DEV))
    pred = _E().ensemble_argmax(maps, T.flips_of(case), H, W, rule == "probs")
    assert pred.dtype == torch.uint8 and pred.shape == (B, H, W) and bool((pred == 4).all())


# ----------------------------------------------------------------------------- 5. view order, determinism
@pytest.mark.parametrize("rule", T.RULES)
@pytest.mark.parametrize("case", ["ms_flip", "odd"])
def test_view_order_moves_only_ambiguous_pixels_and_runs_repeat_bitwise(case, rule):
    low = torch.bfloat16
    B, H, W, views = T.CASES[case]
    u, tau = T.seg_reference(case, low, rule)
    first = run_seg(case, low, rule)
    again = run_seg(case, low, rule)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert first[2] == again[2] and first[3] == again[3]  # the CE sum bitwise, from the same start
    order = list(reversed(range(len(views))))
    perm = run_seg(case, low, rule, order=order)
    amb = T.check_class_map(perm[0], u, tau)
    moved = perm[0] != first[0]
    assert not bool((moved & ~amb).any()), f"{int((moved & ~amb).sum())} unambiguous pixels changed with the order"
    assert perm[3] == first[3]
    d1, d2 = run_depth(case, low), run_depth(case, low)
    assert bitwise_equal(d1[0], d2[0]) and d1[1] == d2[1]
    dp = run_depth(case, low, order=order)
    _, dtau = T.depth_reference(case, low)
    assert float((dp[0] - d1[0]).abs().max()) <= 2 * dtau


# ----------------------------------------------------------------------------- 6. depth
def check_depth_sums(got, up64, gt, mask, clamp, dmin=1e-3, dmax=80.0):
    want = R.depth_sums(up64, gt, mask, dmin, dmax, clamp)
    lo = R.depth_sums(up64, gt, mask, dmin, dmax, clamp, thr_scale=1 - 1e-5)
    hi = R.depth_sums(up64, gt, mask, dmin, dmax, clamp, thr_scale=1 + 1e-5)
    assert got[0] == want[0] and got[8] == want[8], (got[0], want[0], got[8], want[8])
    for i in (5, 6, 7):
        assert lo[i] <= got[i] <= hi[i], (R.SUM_NAMES[i], lo[i], got[i], hi[i])
    worst = []
    for i in R.FLOAT_SUMS:
        err = R.rel(got[i], want[i]) if want[i] != 0 else abs(got[i])
        print(f"{R.SUM_NAMES[i]}: {got[i]!r} vs fp64 {want[i]!r}: rel {err:.2e}")
        if err > 4 * REF_FP32_DEPARTURE[R.SUM_NAMES[i]]:
            worst.append((R.SUM_NAMES[i], err))
    assert not worst, worst


@pytest.mark.parametrize("case,low,mask_kind,clamp", T.DEPTH_CASES,
                         ids=[f"{c}-{_name(d)}-{m}-clamp{k}" for c, d, m, k in T.DEPTH_CASES])
def test_depth_sums_and_mean_map(case, low, mask_kind, clamp):
    B, H, W, views = T.CASES[case]
    up, sums = run_depth(case, low, mask_kind, clamp)
    u64, tau = T.depth_reference(case, low)
    dev = float((up.double() - u64[:, 0]).abs().max())
    print(f"up: max |up - mean| {dev:.3e} (tau {tau:.3e})")
    assert dev <= tau
    check_depth_sums(sums, u64, R.depth_target(B, H, W), T.mask_of(mask_kind, B, H, W), bool(clamp))


@pytest.mark.parametrize("low", T.LOWS, ids=_name)
@pytest.mark.parametrize("case", ["ms_flip", "odd", "narrow_tile"])
def test_depth_prediction_only_equals_the_map_of_the_run_with_a_target(case, low):
    with_target = run_depth(case, low)[0]
    alone, sums = run_depth(case, low, target=False)
    assert sums is None and bitwise_equal(alone, with_target)


# ----------------------------------------------------------------------------- 7. ops
def _op_inputs(case="odd", low=torch.bfloat16, labdt=torch.uint8):
    B, H, W, views = T.CASES[case]
    return dict(segs=[m.to(DEV) for m in T.seg_views(case, low)], depths=[m.to(DEV) for m in T.depth_views(case, low)],
                flips=T.flips_of(case), lab=R.labels(B, H, W, labdt).to(DEV), gt=R.depth_target(B, H, W).to(DEV),
                mk=R.depth_mask(B, H, W).to(DEV), size=(H, W))


def test_opcheck_ensemble_ops():
    from denseclip_vit_multimodal_amd.evaluate import _E
    E = _E()
    a = _op_inputs()
    H, W = a["size"]
    utils = ("test_schema", "test_faketensor", "test_aot_dispatch_dynamic")
    # the two *_update ops mutate their accumulators and return `Tensor?`: torch's functionalisation
    # of custom ops does not take an optional return beside mutated arguments (as for the single-view
    # seg_update / depth_update, whose schemas these follow), so they are checked for schema and
    # mutation annotations and for fake-vs-real outputs, not traced through AOT dispatch
    mut_utils = ("test_schema", "test_faketensor")
    cm = lambda: torch.zeros(K, K, dtype=torch.int64, device=DEV)  # noqa: E731
    ce = lambda: torch.zeros(2, dtype=torch.float64, device=DEV)  # noqa: E731
    sums = lambda: torch.zeros(12, dtype=torch.float64, device=DEV)  # noqa: E731
    for probs in (False, True):
        torch.library.opcheck(E.ensemble_argmax, (a["segs"], a["flips"], H, W, probs), test_utils=utils)
        for want in (False, True):
            torch.library.opcheck(E.ensemble_seg_update, (a["segs"], a["flips"], a["lab"], R.IGNORE, probs, cm(), ce(),
                                                          want), test_utils=mut_utils)
    torch.library.opcheck(E.ensemble_depth, (a["depths"], a["flips"], H, W), test_utils=utils)
    for want, mk in ((False, a["mk"]), (True, None)):
        torch.library.opcheck(E.ensemble_depth_update, (a["depths"], a["flips"], a["gt"], mk, 1e-3, 80.0, True, 1e-6,
                                                        sums(), want), test_utils=mut_utils)


@pytest.mark.parametrize("rule", T.RULES)
def test_update_views_equals_the_c_abi_and_per_call_adds_up(rule):
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, _E
    case, low, labdt = "odd", torch.bfloat16, torch.uint8
    a = _op_inputs(case, low, labdt)
    pred, cm, loss, count = run_seg(case, low, rule, labdt=labdt, start=(0, 0.0, 0))
    up, sums = run_depth(case, low, start=0.0)
    ev = Evaluator(device=DEV)
    assert ev.update_views(a["segs"], a["depths"], a["flips"], a["lab"], a["gt"], a["mk"], average=rule) is None
    assert torch.equal(ev.cm.cpu(), cm)
    assert [float(v) for v in ev.ce_sums.cpu()] == [loss, float(count)]
    assert [float(v) for v in ev.depth_sums.cpu()] == sums
    E = _E()
    assert torch.equal(E.ensemble_argmax(a["segs"], a["flips"], *a["size"], rule == "probs").cpu(), pred)
    assert bitwise_equal(E.ensemble_depth(a["depths"], a["flips"], *a["size"]).cpu()[:, 0], up)
    one = [t.clone() for t in (ev.cm, ev.ce_sums, ev.depth_sums)]
    own = ev.update_views(a["segs"], a["depths"], a["flips"], a["lab"], a["gt"], a["mk"], average=rule, per_call=True)
    for x, y in zip(one, (own["cm"], own["ce_sums"], own["depth_sums"])):
        assert bitwise_equal(x, y)  # the call's own sums: those of the first call, from zero
    for x, y in zip(one, (ev.cm, ev.ce_sums, ev.depth_sums)):
        assert bitwise_equal(x + x, y)  # and the running state holds both


def test_update_views_captured_in_a_graph_accumulates_per_replay():
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    a = _op_inputs()
    args = (a["segs"], a["depths"], a["flips"], a["lab"], a["gt"], a["mk"])
    eager = Evaluator(device=DEV)
    for _ in range(2):
        eager.update_views(*args)
    ev = Evaluator(device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # allocator pools, library handles
            ev.update_views(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert ev.update_views(*args) is None
    ev.reset()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ev.cm.sum()) == 2 * int(R.valid_labels(a["lab"]).sum())
    for x, y in zip((eager.cm, eager.ce_sums, eager.depth_sums), (ev.cm, ev.ce_sums, ev.depth_sums)):
        assert bitwise_equal(x, y)


# ----------------------------------------------------------------------------- 8. model
@pytest.fixture(scope="module")
def mid_model():
    from denseclip_vit_multimodal_amd import DenseCLIP
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **MID_CFG)
    m.load_state_dict(spec_state_dict("mid"))
    m.backbone.compute_dtype = torch.float16
    return m.to(DEV).eval()


SCALES = (0.5, 1.0, 1.5)


@pytest.mark.parametrize("rule", T.RULES)
def test_model_predict_tta_against_the_fp64_ensemble_of_its_views(mid_model, rule):
    from denseclip_vit_multimodal_amd.evaluate import forward_views, predict_tta
    x = images(1, 128, 256).to(DEV)
    H, W = 128, 256
    segs, depths, flips = forward_views(mid_model, x, SCALES, True)
    assert flips == [0, 1] * 3 and len(segs) == len(depths) == 6
    assert len({tuple(s.shape[-2:]) for s in segs}) == 3 and all(s.shape[-1] <= W for s in segs)
    out = predict_tta(mid_model, x, scales=SCALES, flip=True, average=rule)
    assert out["seg"].dtype == torch.uint8 and out["seg"].shape == (1, H, W)
    assert out["depth"].dtype == torch.float32 and out["depth"].shape == (1, 1, H, W)
    maps = [s.cpu() for s in segs]
    geo = [(s.shape[-2], s.shape[-1], f) for s, f in zip(maps, flips)]
    u = T.ensemble(maps, flips, H, W, probs=rule == "probs")
    T.check_class_map(out["seg"].cpu(), u, T.tau_of(maps, geo, u, rule))
    dmaps = [d.cpu() for d in depths]
    d64 = T.ensemble(dmaps, flips, H, W)
    dtau = T.tau_of(dmaps, geo, d64, "logits")
    dev = float((out["depth"].cpu().double() - d64).abs().max())
    print(f"depth: max |up - mean| {dev:.3e} (tau {dtau:.3e})")
    assert dev <= dtau


def _same_metrics(got, want):
    for k, v in want.items():  # NaN where an untrained depth head goes negative: equal as NaN
        if v is None:
            assert got[k] is None, k
        else:
            assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=np.asarray(v).dtype.kind == "f"), k


def test_validate_with_and_without_tta_equals_an_evaluator_fed_by_hand(mid_model):
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, forward_views, validate
    from denseclip_vit_multimodal_amd.train import synth_batch
    batches = [synth_batch(1, 128, 256, torch.device(DEV), rank=r, image_dtype=torch.float32) for r in (0, 1)]
    total = sum(int((b[1] != 255).sum()) for b in batches)
    for rule in T.RULES:
        mid_model.train()
        got = validate(mid_model, batches, tta=dict(scales=SCALES, flip=True, average=rule))
        assert mid_model.training
        mid_model.eval()
        ev = Evaluator(device=DEV)
        for img, seg, depth, mask in batches:
            segs, depths, flips = forward_views(mid_model, img, SCALES, True)
            ev.update_views(segs, depths, flips, seg, depth, mask, average=rule)
        want = ev.compute()
        assert int(want["confusion_matrix"].sum()) == total
        _same_metrics(got, want)
    # without tta: today's code path, one forward_lowres + update per batch
    got = validate(mid_model, batches)
    ev = Evaluator(device=DEV)
    with torch.no_grad():
        for img, seg, depth, mask in batches:
            low = mid_model.forward_lowres(img)
            ev.update(low["seg"], low["depth"], seg, depth, mask)
    _same_metrics(got, ev.compute())
