"""Sliding-window inference fused into the evaluation (csrc/headslide.hip ->
torch.ops.dclip_eval.slide_* -> evaluate.py) on the GPU.  C-ABI calls run on guard-banded buffers
(abi_guard.run_poisoned): outputs and workspace pre-filled with 0xFF and then 0x3C must give equal
results, guards intact, and the accumulating arguments are checked from a non-zero start.

Reference (slide_ref.slide): fp64 on the CPU; per window F.interpolate of the values to the window
size, added into an image-sized accumulator at the window's origin beside a count map, then the
division (mmseg's slide_inference).

Class map: a pixel is ambiguous when its top-2 gap in the fp64 result is below
    tau = max_g 2^-24 max|L_g| (32 + 8 (h + w)) + 2^-24 (cmax + 1) max|result|,
cmax the largest number of windows on a pixel.  Every other pixel must equal the fp64 argmax, an
ambiguous one must pick a class within tau of the maximum, and at most 2e-3 of a case's pixels may be
ambiguous.  Measured on the CPU over these inputs (`python tests/slide_ref.py`, torch's scalar CPU
kernels, so the figures are the same on every machine; every case and low dtype): the ambiguous share
is at most 7.66e-4 (narrow_tile); torch's own fp32 sequence stays within 0.086 tau of the fp64 result
and disagrees with the fp64 argmax on no unambiguous pixel.

Floating sums: measured the same way (the CE sum over every case and low dtype with the label dtype
paired to the low dtype; the depth sums over slide_ref.DEPTH_CASES), the reference's own fp32 path
(the same torch sequence in fp32) departs from its fp64 evaluation by at most
    CE sum 1.82e-7, sum (gt-p)^2 9.20e-8, sum (log gt - log p)^2 2.02e-7, sum |gt-p|/gt 4.50e-7,
    sum (gt-p)^2/gt 6.24e-7, masked sum (gt-up)^2 1.03e-7, sum d 9.11e-8, sum d^2 1.02e-7
relative (REF_FP32_DEPARTURE).  The kernel keeps fp32 per-pixel terms but sums in f64 and is allowed
4x these figures.  Threshold counts must lie between the fp64 counts at t (1 - 1e-5) and t (1 + 1e-5).
The depth map must agree with the fp64 result to within the depth windows' tau.
"""
import ctypes

import numpy as np
import pytest
import torch

import eval_ref as R
import slide_ref as S
from abi_guard import bitwise_equal, guarded, guarded_copy, run_poisoned
from helpers import MID_CFG, CITYSCAPES_CLASSES, images, spec_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = R.K
REF_FP32_DEPARTURE = {"ce": 1.82e-07, "sq": 9.20e-08, "log_sq": 2.02e-07, "abs_rel": 4.50e-07, "sq_rel": 6.24e-07,
                      "mask_sq": 1.03e-07, "d": 9.11e-08, "d_sq": 1.02e-07}
LOW_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
LAB_DT = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
_name = lambda d: str(d).replace("torch.", "")  # noqa: E731


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def _N():
    from denseclip_vit_multimodal_amd import _native as N
    return N


def _call(name, *args):
    return _N().call(name, *args)


def _ws(B, k, nwin):
    return guarded(int(_N().lib().dclip_slide_eval_ws_bytes(B, k, nwin)))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(bufs, origins, order):
    return _N().window_table([(bufs[g].ptr(), origins[g][0], origins[g][1]) for g in order])


def _flat(origins):
    return [c for o in origins for c in o]


def run_seg(case, low, labdt=None, order=None, labels=True, start=(5, 1.5, 3), geom=None, maps=None):
    """dclip_slide_eval_seg through run_poisoned; (pred, cm, loss_sum, count) minus the start values;
    labels=False: the class map only (null labels, cm, loss_sum, count and workspace)"""
    B, H, W, (wh, ww), origins, (h, w) = S.geometry(case) if geom is None else geom
    labdt = S.LAB_OF_LOW[low] if labdt is None else labdt
    order = list(range(len(origins))) if order is None else order
    bufs = [guarded_copy(m.to(DEV)) for m in (S.seg_lows(case, low) if maps is None else maps)]
    tab = _table(bufs, origins, order)
    pred = guarded((B, H, W), torch.uint8)
    if not labels:
        def fn():
            _call("dclip_slide_eval_seg", LOW_DT[low], tab, len(order), B, K, h, w, wh, ww, None, 0, H, W, R.IGNORE,
                  pred.ptr(), None, None, None, None, _stream())

        (p,) = run_poisoned(fn, inputs=bufs, outputs=[pred])
        return p.cpu(), None, None, None
    lab = guarded_copy(R.labels(B, H, W, labdt).to(DEV))
    cm, loss, cnt = guarded((K, K), torch.int64), guarded(1, torch.float64), guarded(1, torch.int64)
    ws = _ws(B, K, len(order))

    def fn():
        cm.t.fill_(start[0]); loss.t.fill_(start[1]); cnt.t.fill_(start[2])  # noqa: E702
        _call("dclip_slide_eval_seg", LOW_DT[low], tab, len(order), B, K, h, w, wh, ww, lab.ptr(), LAB_DT[labdt], H, W,
              R.IGNORE, pred.ptr(), cm.ptr(), loss.ptr(), cnt.ptr(), ws.ptr(), _stream())

    p, c, ls, n = run_poisoned(fn, inputs=bufs + [lab], outputs=[pred], scratch=[ws], accum=[cm, loss, cnt])
    return p.cpu(), c.cpu() - start[0], float(ls.cpu()) - start[1], int(n.cpu()) - start[2]


def run_depth(case, low, mask_kind="mask", clamp=1, order=None, target=True, start=2.0, dmin=1e-3, dmax=80.0, geom=None,
              maps=None):
    """dclip_slide_eval_depth through run_poisoned; (up, sums minus the start value); target=False:
    prediction only (null target, mask, sums and workspace), sums None"""
    B, H, W, (wh, ww), origins, (h, w) = S.geometry(case) if geom is None else geom
    order = list(range(len(origins))) if order is None else order
    bufs = [guarded_copy(m.to(DEV)) for m in (S.depth_lows(case, low) if maps is None else maps)]
    tab = _table(bufs, origins, order)
    up = guarded((B, H, W), torch.float32)
    if not target:
        def fn():
            _call("dclip_slide_eval_depth", LOW_DT[low], tab, len(order), B, h, w, wh, ww, None, None, H, W, dmin, dmax,
                  int(clamp), 1e-6, up.ptr(), None, None, _stream())

        (u,) = run_poisoned(fn, inputs=bufs, outputs=[up])
        return u.cpu(), None
    mask = S.mask_of(mask_kind, B, H, W)
    gt = guarded_copy(R.depth_target(B, H, W).to(DEV))
    mk = guarded_copy(mask.to(DEV)) if mask is not None else None
    sums, ws = guarded(12, torch.float64), _ws(B, 1, len(order))

    def fn():
        sums.t.fill_(start)
        _call("dclip_slide_eval_depth", LOW_DT[low], tab, len(order), B, h, w, wh, ww, gt.ptr(),
              mk.ptr() if mk else None, H, W, dmin, dmax, int(clamp), 1e-6, up.ptr(), sums.ptr(), ws.ptr(), _stream())

    u, s = run_poisoned(fn, inputs=bufs + [gt] + ([mk] if mk else []), outputs=[up], scratch=[ws], accum=[sums])
    return u.cpu(), [float(v) - start for v in s.cpu()]


def check_seg(case, low, pred, cm, loss, count):
    B, H, W = S.CASES[case][:3]
    u, tau = S.seg_reference(case, low)
    amb = S.check_class_map(pred, u, tau)
    lab = R.labels(B, H, W, S.LAB_OF_LOW[low])
    valid = R.valid_labels(lab)
    assert int(valid.sum()) < lab.numel()  # ignore / out-of-range labels are present ...
    want = torch.bincount((lab.long() * K + pred.long())[valid], minlength=K * K).view(K, K)
    assert torch.equal(cm, want)  # ... and contribute nothing; the kernel's own class map otherwise, exactly
    assert count == int(valid.sum())
    ce64 = R.ce_sum(u, lab)
    err = R.rel(loss, ce64)
    print(f"CE sum {loss!r} vs fp64 {ce64!r}: rel {err:.2e}")
    assert err <= 4 * REF_FP32_DEPARTURE["ce"], err
    return amb


# ----------------------------------------------------------------------------- 1. cases x dtypes
@pytest.mark.parametrize("low", S.LOWS, ids=_name)
@pytest.mark.parametrize("case", list(S.CASES))
def test_seg_class_map_confusion_matrix_count_and_ce(case, low):
    check_seg(case, low, *run_seg(case, low))


# ----------------------------------------------------------------------------- 2. depth
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


@pytest.mark.parametrize("case,low,mask_kind,clamp", S.DEPTH_CASES,
                         ids=[f"{c}-{_name(d)}-{m}-clamp{k}" for c, d, m, k in S.DEPTH_CASES])
def test_depth_sums_and_mean_map(case, low, mask_kind, clamp):
    B, H, W = S.CASES[case][:3]
    up, sums = run_depth(case, low, mask_kind, clamp)
    u64, tau = S.depth_reference(case, low)
    dev = float((up.double() - u64[:, 0]).abs().max())
    print(f"up: max |up - result| {dev:.3e} (tau {tau:.3e})")
    assert dev <= tau
    check_depth_sums(sums, u64, R.depth_target(B, H, W), S.mask_of(mask_kind, B, H, W), bool(clamp))


@pytest.mark.parametrize("low", S.LOWS, ids=_name)
@pytest.mark.parametrize("case", ["thirds", "odd", "narrow_tile"])
def test_depth_prediction_only_equals_the_map_of_the_run_with_a_target(case, low):
    with_target = run_depth(case, low)[0]
    alone, sums = run_depth(case, low, target=False)
    assert sums is None and bitwise_equal(alone, with_target)


# ----------------------------------------------------------------------------- 3. one window over the image
def _one_window(which):
    """a geometry with a single window that is the whole image"""
    if which == "small_image":
        return S.geometry("small_image")
    B, H, W = S.CASES["thirds"][:3]  # thirds' image under a crop no smaller than the image
    size, origins = S.windows(H, W, (64, 200), (21, 42))
    return B, H, W, size, origins, S.CASES["thirds"][5]


@pytest.mark.parametrize("low", S.LOWS, ids=_name)
@pytest.mark.parametrize("which", ["small_image", "thirds_large_crop"])
def test_one_window_over_the_image_equals_one_plain_view_of_the_ensemble(which, low):
    """class map, confusion matrix, count, `up` and the 12 depth sums of dclip_ensemble_eval_* with one
    plain view of the same map, bitwise: the window-local arithmetic at origin (0, 0) is the view's,
    and a count of 1 divides nothing"""
    geom = _one_window(which)
    B, H, W, size, origins, (h, w) = geom
    assert size == (H, W) and origins == [(0, 0)]
    N = _N()
    labdt = S.LAB_OF_LOW[low]
    seg, dep = S.seg_low(0, B, h, w, low), S.depth_low(0, B, h, w, low)
    pred, cm, loss, count = run_seg(None, low, start=(0, 0.0, 0), geom=geom, maps=[seg])
    up, sums = run_depth(None, low, start=0.0, geom=geom, maps=[dep])
    lg, d = seg.to(DEV), dep.to(DEV)
    lab = R.labels(B, H, W, labdt).to(DEV)
    p1 = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
    cm1 = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    ls1, n1 = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    ws1 = torch.empty(int(N.lib().dclip_ensemble_eval_ws_bytes(B, K, 1)), dtype=torch.uint8, device=DEV)
    _call("dclip_ensemble_eval_seg", LOW_DT[low], N.view_table([(lg.data_ptr(), h, w, 0)]), 1, B, K, 0, lab.data_ptr(),
          LAB_DT[labdt], H, W, R.IGNORE, p1.data_ptr(), cm1.data_ptr(), ls1.data_ptr(), n1.data_ptr(), ws1.data_ptr(),
          _stream())
    assert torch.equal(pred, p1.cpu()) and torch.equal(cm, cm1.cpu()) and count == int(n1)
    print(f"CE sum {loss!r} vs one view {float(ls1)!r}: rel {R.rel(loss, float(ls1)):.2e}")
    gt, mk = R.depth_target(B, H, W).to(DEV), R.depth_mask(B, H, W).to(DEV)
    up1 = torch.empty(B, H, W, device=DEV)
    s1 = torch.zeros(12, dtype=torch.float64, device=DEV)
    wsd = torch.empty(int(N.lib().dclip_ensemble_eval_ws_bytes(B, 1, 1)), dtype=torch.uint8, device=DEV)
    _call("dclip_ensemble_eval_depth", LOW_DT[low], N.view_table([(d.data_ptr(), h, w, 0)]), 1, B, gt.data_ptr(),
          mk.data_ptr(), H, W, 1e-3, 80.0, 1, 1e-6, up1.data_ptr(), s1.data_ptr(), wsd.data_ptr(), _stream())
    assert bitwise_equal(up, up1.cpu())
    assert sums == [float(v) for v in s1.cpu()]  # from a zero start on both sides: bitwise


# ----------------------------------------------------------------------------- 4. translation
@pytest.mark.parametrize("low", S.LOWS, ids=_name)
def test_disjoint_windows_are_the_single_view_results_translated(low):
    """`exact`: no overlap, so every window's region of the class map is upsample_argmax of its map at
    the window size, and its region of `up` is, bitwise, the single-view kernel's resize of its depth
    map (the origins are multiples of 4: the window-local pixel slots are the image's)"""
    from denseclip_vit_multimodal_amd.evaluate import _E, upsample_argmax
    B, H, W, (wh, ww), origins, (h, w) = S.geometry("exact")
    assert len(origins) == 4 and all(y % 4 == 0 and x % 4 == 0 for y, x in origins)
    pred = run_seg("exact", low)[0]
    up = run_depth("exact", low)[0]
    zeros, sums = torch.zeros(B, wh, ww, device=DEV), torch.zeros(12, dtype=torch.float64, device=DEV)
    for g, (y0, x0) in enumerate(origins):
        own = upsample_argmax(S.seg_low(g, B, h, w, low).to(DEV), (wh, ww)).cpu()
        assert torch.equal(pred[:, y0:y0 + wh, x0:x0 + ww], own), g
        one = _E().depth_update(S.depth_low(g, B, h, w, low).to(DEV), zeros, None, 1e-3, 80.0, True, 1e-6, sums, True)
        assert bitwise_equal(up[:, y0:y0 + wh, x0:x0 + ww].contiguous(), one.cpu()[:, 0].contiguous()), g


@pytest.mark.parametrize("x0", [1, 2, 3])
def test_depth_window_at_an_odd_origin_is_its_own_resize(x0):
    """a window's depth values follow its window-local columns: where it alone covers a pixel, the
    value is, bitwise, the single-view kernel's resize of its map, whatever the origin mod 4"""
    from denseclip_vit_multimodal_amd.evaluate import _E
    B, h, w, wh, ww, H = 1, 5, 12, 20, 50, 20
    W = x0 + ww
    maps = [S.depth_low(g, B, h, w).to(DEV) for g in range(2)]
    up = _E().slide_depth(maps, [0, 0, 0, x0], wh, ww, H, W)
    zeros, sums = torch.zeros(B, wh, ww, device=DEV), torch.zeros(12, dtype=torch.float64, device=DEV)
    own = [_E().depth_update(m, zeros, None, 1e-3, 80.0, True, 1e-6, sums, True) for m in maps]
    assert bitwise_equal(up[..., :x0].contiguous(), own[0][..., :x0].contiguous())  # the first window alone
    assert bitwise_equal(up[..., ww:].contiguous(), own[1][..., ww - x0:].contiguous())  # the second alone
    mean = (own[0][..., x0:] + own[1][..., :ww - x0]) / 2  # both: one rounded add, one division
    assert bitwise_equal(up[..., x0:ww].contiguous(), mean.contiguous())


# ----------------------------------------------------------------------------- 5. order, determinism
@pytest.mark.parametrize("case", ["thirds", "odd", "dense"])
def test_window_order_moves_only_ambiguous_pixels_and_runs_repeat_bitwise(case):
    low = torch.bfloat16
    B, H, W, size, origins, hw = S.geometry(case)
    first = run_seg(case, low)
    again = run_seg(case, low)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert first[2] == again[2] and first[3] == again[3]  # the CE sum bitwise, from the same start
    order = list(reversed(range(len(origins))))
    perm = run_seg(case, low, order=order)
    amb = check_seg(case, low, *perm)  # the same checks as in table order
    moved = perm[0] != first[0]
    assert not bool((moved & ~amb).any()), f"{int((moved & ~amb).sum())} unambiguous pixels changed with the order"
    d1, d2 = run_depth(case, low), run_depth(case, low)
    assert bitwise_equal(d1[0], d2[0]) and d1[1] == d2[1]
    dp = run_depth(case, low, order=order)
    u64, dtau = S.depth_reference(case, low)
    assert float((dp[0].double() - u64[:, 0]).abs().max()) <= dtau
    check_depth_sums(dp[1], u64, R.depth_target(B, H, W), S.mask_of("mask", B, H, W), True)


# ----------------------------------------------------------------------------- 6. class map alone
@pytest.mark.parametrize("low", S.LOWS, ids=_name)
@pytest.mark.parametrize("case", ["thirds", "odd", "narrow_tile"])
def test_prediction_only_gives_the_class_map_of_the_run_with_labels(case, low):
    alone = run_seg(case, low, labels=False)
    assert alone[1] is None and torch.equal(alone[0], run_seg(case, low)[0])


def test_tie_takes_the_lower_class():
    """two channels identical in every window and above every other: the lower index everywhere"""
    from denseclip_vit_multimodal_amd.evaluate import _E
    B, H, W, (wh, ww), origins, hw = S.geometry("odd")
    maps = []
    for m in S.seg_lows("odd", torch.float32):
        m = m.clone()
        m[:, 11] = m[:, 4] = m.amax(1) + 1.0
        maps.append(m.to(DEV))
    pred = _E().slide_argmax(maps, _flat(origins), wh, ww, H, W)
    assert pred.dtype == torch.uint8 and pred.shape == (B, H, W) and bool((pred == 4).all())


# ----------------------------------------------------------------------------- 7. ops, capture
def _op_inputs(case="odd", low=torch.bfloat16, labdt=torch.uint8):
    B, H, W, size, origins, hw = S.geometry(case)
    return dict(segs=[m.to(DEV) for m in S.seg_lows(case, low)], depths=[m.to(DEV) for m in S.depth_lows(case, low)],
                size=size, origins=origins, lab=R.labels(B, H, W, labdt).to(DEV), gt=R.depth_target(B, H, W).to(DEV),
                mk=R.depth_mask(B, H, W).to(DEV), image=(H, W))


def test_opcheck_slide_ops():
    from denseclip_vit_multimodal_amd.evaluate import _E
    E = _E()
    a = _op_inputs()
    (wh, ww), (H, W), flat = a["size"], a["image"], _flat(a["origins"])
    utils = ("test_schema", "test_faketensor", "test_aot_dispatch_dynamic")
    # the two *_update ops mutate their accumulators and return `Tensor?`: as for the ensemble ops they
    # are checked for schema and mutation annotations and for fake-vs-real outputs, not through AOT dispatch
    mut_utils = ("test_schema", "test_faketensor")
    cm = lambda: torch.zeros(K, K, dtype=torch.int64, device=DEV)  # noqa: E731
    ce = lambda: torch.zeros(2, dtype=torch.float64, device=DEV)  # noqa: E731
    sums = lambda: torch.zeros(12, dtype=torch.float64, device=DEV)  # noqa: E731
    torch.library.opcheck(E.slide_argmax, (a["segs"], flat, wh, ww, H, W), test_utils=utils)
    for want in (False, True):
        torch.library.opcheck(E.slide_seg_update, (a["segs"], flat, wh, ww, a["lab"], R.IGNORE, cm(), ce(), want),
                              test_utils=mut_utils)
    torch.library.opcheck(E.slide_depth, (a["depths"], flat, wh, ww, H, W), test_utils=utils)
    for want, mk in ((False, a["mk"]), (True, None)):
        torch.library.opcheck(E.slide_depth_update, (a["depths"], flat, wh, ww, a["gt"], mk, 1e-3, 80.0, True, 1e-6,
                                                     sums(), want), test_utils=mut_utils)


def test_update_windows_equals_the_c_abi_and_per_call_adds_up():
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, _E
    case, low, labdt = "odd", torch.bfloat16, torch.uint8
    a = _op_inputs(case, low, labdt)
    pred, cm, loss, count = run_seg(case, low, labdt=labdt, start=(0, 0.0, 0))
    up, sums = run_depth(case, low, start=0.0)
    ev = Evaluator(device=DEV)
    args = (a["segs"], a["depths"], a["size"], a["origins"], a["lab"], a["gt"], a["mk"])
    assert ev.update_windows(*args) is None
    assert torch.equal(ev.cm.cpu(), cm)
    assert [float(v) for v in ev.ce_sums.cpu()] == [loss, float(count)]
    assert [float(v) for v in ev.depth_sums.cpu()] == sums
    E = _E()
    assert torch.equal(E.slide_argmax(a["segs"], _flat(a["origins"]), *a["size"], *a["image"]).cpu(), pred)
    assert bitwise_equal(E.slide_depth(a["depths"], _flat(a["origins"]), *a["size"], *a["image"]).cpu()[:, 0], up)
    one = [t.clone() for t in (ev.cm, ev.ce_sums, ev.depth_sums)]
    own = ev.update_windows(*args, per_call=True)
    for x, y in zip(one, (own["cm"], own["ce_sums"], own["depth_sums"])):
        assert bitwise_equal(x, y)  # the call's own sums: those of the first call, from zero
    for x, y in zip(one, (ev.cm, ev.ce_sums, ev.depth_sums)):
        assert bitwise_equal(x + x, y)  # and the running state holds both


def test_update_windows_captured_in_a_graph_accumulates_per_replay():
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    a = _op_inputs()
    args = (a["segs"], a["depths"], a["size"], a["origins"], a["lab"], a["gt"], a["mk"])
    eager = Evaluator(device=DEV)
    eager.update_windows(*args)
    ev = Evaluator(device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # allocator pools, library handles
            ev.update_windows(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert ev.update_windows(*args) is None
    ev.reset()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ev.cm.sum()) == 2 * int(R.valid_labels(a["lab"]).sum())
    assert torch.equal(ev.cm, 2 * eager.cm)  # exactly twice the integer state of one eager call
    for i in (0, 5, 6, 7, 8):  # the depth counts
        assert float(ev.depth_sums[i]) == 2 * float(eager.depth_sums[i]), i
    assert float(ev.ce_sums[1]) == 2 * float(eager.ce_sums[1])
    twice = Evaluator(device=DEV)
    for _ in range(2):
        twice.update_windows(*args)
    for x, y in zip((twice.cm, twice.ce_sums, twice.depth_sums), (ev.cm, ev.ce_sums, ev.depth_sums)):
        assert bitwise_equal(x, y)  # and the floating sums are those of two eager calls


# ----------------------------------------------------------------------------- 8. model
@pytest.fixture(scope="module")
def mid_model():
    from denseclip_vit_multimodal_amd import DenseCLIP
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **MID_CFG)
    m.load_state_dict(spec_state_dict("mid"))
    m.backbone.compute_dtype = torch.float16
    return m.to(DEV).eval()


CROP, STRIDE = (32, 64), (21, 42)  # `thirds` on a 64 x 128 image


def test_model_predict_slide_against_the_fp64_sequence_on_its_windows(mid_model):
    from denseclip_vit_multimodal_amd.evaluate import forward_windows, predict_slide
    H, W = 64, 128
    x = images(2, H, W).to(DEV)
    segs, depths, size, origins = forward_windows(mid_model, x, CROP, STRIDE)
    assert (size, origins) == S.windows(H, W, CROP, STRIDE) and len(segs) == len(depths) == 9
    assert all(s.shape == segs[0].shape and s.shape[0] == 2 for s in segs) and segs[0].shape[-1] <= size[1]
    # several windows per forward: the same windows through a larger batch
    segs3, depths3, _, _ = forward_windows(mid_model, x, CROP, STRIDE, windows_per_forward=4)
    assert len(segs3) == 9 and all(a.shape == b.shape for a, b in zip(segs, segs3))
    out = predict_slide(mid_model, x, CROP, STRIDE)
    assert out["seg"].dtype == torch.uint8 and out["seg"].shape == (2, H, W)
    assert out["depth"].dtype == torch.float32 and out["depth"].shape == (2, 1, H, W)
    maps = [s.cpu() for s in segs]
    hw = tuple(maps[0].shape[-2:])
    u, cnt = S.slide(maps, origins, size, H, W)
    assert int(cnt.max()) == 4 and int(cnt.min()) == 1
    S.check_class_map(out["seg"].cpu(), u, S.tau_of(maps, hw, u, 4))
    dmaps = [d.cpu() for d in depths]
    d64, _ = S.slide(dmaps, origins, size, H, W)
    dtau = S.tau_of(dmaps, hw, d64, 4)
    dev = float((out["depth"].cpu().double() - d64).abs().max())
    print(f"depth: max |up - result| {dev:.3e} (tau {dtau:.3e})")
    assert dev <= dtau


def _same_metrics(got, want):
    for k, v in want.items():  # NaN where an untrained depth head goes negative: equal as NaN
        if v is None:
            assert got[k] is None, k
        else:
            assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=np.asarray(v).dtype.kind == "f"), k


def test_validate_slide_against_the_fp64_sequence_and_unchanged_without_slide(mid_model):
    """validate(slide=...) against metrics_from_sums of the fp64 sequence on the windows' maps.
    The confusion matrix may differ from the fp64 one only by the ambiguous pixels (each moves one
    count between two cells).  The floating metrics are ratios (and square roots) of sums that each
    sit within 4x REF_FP32_DEPARTURE of fp64, at most 4 * 6.24e-7 = 2.5e-6: a metric of two such sums
    is held to 5e-6 relative; a1..a3 to the counts bracketed at t (1 -+ 1e-5)."""
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, forward_windows, metrics_from_sums, validate
    from denseclip_vit_multimodal_amd.train import synth_batch
    H, W = 64, 128
    batches = [synth_batch(1, H, W, torch.device(DEV), rank=r, image_dtype=torch.float32) for r in (0, 1)]
    mid_model.train()
    got = validate(mid_model, batches, slide=dict(crop_size=CROP, stride=STRIDE))
    assert mid_model.training
    mid_model.eval()
    # slide=True reads the model's test_cfg
    mid_model.test_cfg = dict(mode="slide", crop_size=CROP, stride=STRIDE)
    try:
        _same_metrics(validate(mid_model, batches, slide=True), got)
    finally:
        mid_model.test_cfg = None
    cm = torch.zeros(K, K, dtype=torch.int64)
    ce, n_amb = 0.0, 0
    sums, lo, hi = np.zeros(12), np.zeros(12), np.zeros(12)
    ev = Evaluator(device=DEV)
    for img, seg, depth, mask in batches:
        segs, depths, size, origins = forward_windows(mid_model, img, CROP, STRIDE)
        ev.update_windows(segs, depths, size, origins, seg, depth, mask)
        maps, dmaps = [s.cpu() for s in segs], [d.cpu() for d in depths]
        u, cnt = S.slide(maps, origins, size, H, W)
        top = u.topk(2, dim=1).values
        n_amb += int(((top[:, 0] - top[:, 1]) < S.tau_of(maps, tuple(maps[0].shape[-2:]), u, int(cnt.max()))).sum())
        lab = seg.cpu().reshape(1, H, W)
        valid = R.valid_labels(lab)
        cm += torch.bincount((lab.long() * K + u.argmax(1))[valid], minlength=K * K).view(K, K)
        ce += R.ce_sum(u, lab)
        d64, _ = S.slide(dmaps, origins, size, H, W)
        gt, mk = depth.cpu().reshape(1, H, W), mask.cpu().reshape(1, H, W).to(torch.uint8)
        sums += np.asarray(R.depth_sums(d64, gt, mk))
        lo += np.asarray(R.depth_sums(d64, gt, mk, thr_scale=1 - 1e-5))
        hi += np.asarray(R.depth_sums(d64, gt, mk, thr_scale=1 + 1e-5))
    _same_metrics(got, ev.compute())  # validate is forward_windows + update_windows per batch
    want = metrics_from_sums(cm.numpy(), [ce, float(cm.sum())], sums)
    gcm = torch.from_numpy(got["confusion_matrix"])
    print(f"ambiguous pixels {n_amb}, confusion matrix L1 distance {int((gcm - cm).abs().sum())}")
    assert int(gcm.sum()) == int(cm.sum()) and int((gcm - cm).abs().sum()) <= 2 * n_amb
    if n_amb == 0:
        assert got["accuracy"] == want["accuracy"] and got["mean_iou"] == want["mean_iou"]
    for k in ("loss_seg", "abs_rel", "sq_rel", "rmse", "rmse_log", "rmse_masked", "loss_silog"):
        assert got[k] is not None and np.isfinite(want[k]), (k, got[k], want[k])
        err = R.rel(got[k], want[k])
        print(f"{k}: {got[k]!r} vs fp64 {want[k]!r}: rel {err:.2e}")
        assert err <= 5e-6, (k, err)
    n = sums[0]
    for i, k in ((5, "a1"), (6, "a2"), (7, "a3")):
        assert lo[i] / n <= got[k] <= hi[i] / n, k
    # without slide: today's code path, one forward_lowres + update per batch
    got = validate(mid_model, batches)
    ev = Evaluator(device=DEV)
    with torch.no_grad():
        for img, seg, depth, mask in batches:
            low = mid_model.forward_lowres(img)
            ev.update(low["seg"], low["depth"], seg, depth, mask)
    _same_metrics(got, ev.compute())
