"""dclip_upsample_depth_stats / dclip_upsample_depth_finish (csrc/depthlossopt.hip: depth_band_kernel PASS 0, 1
and 2, depth_stats_fold_kernel, depth_bsum_fold_kernel, ce_band.h's merge), the depth loss as a weighted sum
of SILog, L1 and BerHu, behind the C ABI on guard-banded, poisoned buffers (abi_guard.py), both passes
against an fp64 reference: every stats slot to its bound, sum b(e) to its bound, the gradient per low-res
element (depth_loss_check.py: the cases, the reference, the bounds and why they hold).

What the cases cover, over silog_check's nine shapes x three prediction dtypes x three masks x four term
configurations (L1 alone, BerHu alone at theta 0.2 and 0.9, all three terms at weights 1, 0.5, 0.25):
  * the workspace at the library's own size, entered as 0xFF, then as 0x3C (run_poisoned);
  * accumulators that start from non-zero values: the stats at (1.5, 2.5, 3.0, 4.5, 0.125, 7.0), sum b(e)
    at 0.75, the gradient at 0.25 and at zero; the slots the terms do not select come back as they went in;
  * the finish pass on its own: from the stats a separate stats pass wrote, which it must leave bitwise
    unchanged and which the reference takes as they are (c = theta x the handed maximum);
  * a mask without a valid pixel (every sum exactly its start, the gradient exactly its start), mask bytes
    other than 0 / 1, NaN in every masked-out target, h == 1, w == 1, a second chunk of one column, bands
    and low-res elements that own no pixel (bound 0);
  * BerHu at theta = 1 (no pixel above c) is L1 bit for bit; pred == target gives a zero maximum, a zero
    loss, an untouched gradient and nothing non-finite;
  * NaN: one in the resized prediction or in a target under the mask makes sum e, the maximum and sum b(e)
    non-finite while T stays exact; one under masked-out pixels alone changes nothing;
  * two runs of both passes are bitwise equal.
Above the ABI, ops.UpsampleDepthLossFn (eager, under opcheck and replayed from a captured graph),
train.loss_fn, the fused train step against the materialised one and CapturedTrainStep(depth_loss=...).
At the end the module prints, per dtype, the worst figure over its cases as a fraction of its bound.

The kernels on the MI355X over all 324 cases (362 tests, 8.8 s), next to the f32 emulation, worst figure /
bound (f32 | bf16 | fp16 predictions); reports, not thresholds:
    output                          kernels                  emulation
    stats[0] = sum d                0.110 | 0.044 | 0.069    0.015 | 0.029 | 0.085
    stats[1] = sum d^2              0.297 | 0.212 | 0.238    0.061 | 0.132 | 0.252
    stats[2] = T, unselected slots  exact                    exact
    stats[3] = sum e                0.053 | 0.005 | 0.019    the same
    stats[4] = max e                0.152 | 0.160 | 0.122    the same
    sum b(e)                        0.040 | 0.028 | 0.033    0.048 | 0.041 | 0.036
    grad onto 0.25                  0.965 | 0.986 | 0.980    the same   (the rounding of the add onto 0.25)
    grad onto zero ("grad0")        0.210 | 0.197 | 0.211    0.198 | 0.198 | 0.198
ops.UpsampleDepthLossFn's loss sat at 0.001 - 0.055 of its bound, train.loss_fn's at 0.005 - 0.117; the fused
MID_CFG step gave the materialised step's loss to the last f32 bit (7.101263 bf16, 7.100945 fp16) and every
gradient within 1.8e-7 (backbone) / 4.7e-7 (the rest) of it, against 2e-2 / 2e-3 allowed.  Everything passed
as first written.
"""
import pytest
import torch

import depth_loss_check as DC
import misc_check as MC
from abi_guard import bitwise_equal, guarded, guarded_copy, run_poisoned
from helpers import MID_CFG, CITYSCAPES_CLASSES, rel_err, spec_state_dict
from misc_check import BF16, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
WORST = {}  # dtype name -> {output: worst figure / bound} over this session
CASES = DC.cases()


@pytest.fixture(autouse=True)
def _need(hip):
    pass


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key, w in sorted(WORST.items()):
        print(f"\ndepth loss contract dclip_upsample_depth_* {key}: worst figure / bound "
              + ", ".join(f"{n} {v:.3f}" for n, v in sorted(w.items())), end="")


def NT():
    from denseclip_vit_multimodal_amd import _native
    return _native


def code(dt):
    return {F16: NT().F16, BF16: NT().BF16, F32: NT().F32}[dt]


def stream():
    return torch.cuda.current_stream().cuda_stream


def find(**want):
    hits = [c for c in CASES if all(c[k] == v for k, v in want.items())]
    assert hits, want
    return hits[0]


class Buffers:
    """one case's operands in guarded device buffers, the workspace at the library's own size"""

    def __init__(self, c, inp, weights=None, theta=None):
        self.c, (B, h, w, H, W) = c, DC.dims(c)
        self.weights = DC.weights(c) if weights is None else weights
        self.theta = DC.theta(c) if theta is None else theta
        self.terms = sum(bit for bit, v in zip((DC.SILOG, DC.L1, DC.BERHU), self.weights) if v > 0)
        self.pred = guarded_copy(inp["pred"].reshape(B, 1, h, w).to(DEV))
        self.target = guarded_copy(inp["target"].to(DEV))
        self.mask = None if inp["mask"] is None else guarded_copy(inp["mask"].to(DEV))
        self.ws = guarded(int(NT().lib().dclip_upsample_depth_loss_ws_floats(B, h, w)), F32)
        self.inputs = [g for g in (self.pred, self.target, self.mask) if g is not None]

    def call_stats(self, stats):
        B, h, w, H, W = DC.dims(self.c)
        NT().call("dclip_upsample_depth_stats", code(self.c["dt"]), self.pred.ptr(), B, h, w, self.target.ptr(),
                  None if self.mask is None else self.mask.ptr(), H, W, DC.EPS, self.terms, stats.ptr(),
                  self.ws.ptr(), stream())

    def call_finish(self, stats, bsum, grad):
        B, h, w, H, W = DC.dims(self.c)
        NT().call("dclip_upsample_depth_finish", code(self.c["dt"]), self.pred.ptr(), B, h, w, self.target.ptr(),
                  None if self.mask is None else self.mask.ptr(), H, W, DC.EPS, DC.LAMBD, self.terms,
                  *self.weights, self.theta, stats.ptr(), None if bsum is None else bsum.ptr(),
                  None if grad is None else grad.ptr(), self.ws.ptr(), stream())

    def stats(self, start):
        """the six f64 (on the host) after a poisoned stats pass onto `start`"""
        stats, first = guarded(6, F64), torch.tensor(start, dtype=F64, device=DEV)

        def fn():
            stats.t.copy_(first)
            self.call_stats(stats)

        s, = run_poisoned(fn, inputs=self.inputs, scratch=[self.ws], accum=[stats])
        return s.cpu()

    def finish(self, given, grad_start, bsum_start=DC.BSUM_START, want_grad=True):
        """(sum b(e) or None, the gradient (B, h, w) or None) after a poisoned finish pass from `given` onto the
        starts; `given` is an input: guarded, and bitwise unchanged afterwards"""
        B, h, w, H, W = DC.dims(self.c)
        gst = guarded_copy(given.to(DEV))
        grad = guarded((B, h, w), F32) if want_grad else None
        bsum = guarded(1, F64) if self.terms & DC.BERHU else None

        def fn():
            if grad is not None:
                grad.t.fill_(grad_start)
            if bsum is not None:
                bsum.t.fill_(bsum_start)
            self.call_finish(gst, bsum, grad)

        outs = run_poisoned(fn, inputs=self.inputs + [gst], scratch=[self.ws],
                            accum=[g for g in (bsum, grad) if g is not None])
        assert bitwise_equal(gst.t.cpu(), given), "the finish pass wrote to its stats"
        outs = [o.cpu() for o in outs]
        return (outs.pop(0) if bsum is not None else None), (outs.pop(0) if grad is not None else None)


@pytest.mark.parametrize("c", CASES, ids=[DC.case_id(c) for c in CASES])
def test_both_passes(c):
    """the stats onto non-zero starts and from zero; the finish pass from the latter's stats onto 0.75 / 0.25
    and onto zero; its forward-only form gives the same sum b(e) bit for bit"""
    inp = DC.inputs(c)
    buf = Buffers(c, inp)
    raw = buf.stats(DC.STATS_START)
    given = buf.stats((0.0,) * 6)
    bsum, grad = buf.finish(given, DC.GRAD_START)
    bsum0, grad0 = buf.finish(given, 0.0, bsum_start=0.0)
    outs = dict(DC.split_stats(raw), grad=grad, grad0=grad0)
    if bsum is not None:
        outs["Sb"] = bsum - DC.BSUM_START
        fwd_only, none = buf.finish(given, 0.0, bsum_start=0.0, want_grad=False)
        assert none is None and bitwise_equal(fwd_only, bsum0), "the forward-only form's sum b(e) differs"
    if c["mask"] == "empty":
        assert bitwise_equal(raw, torch.tensor(DC.STATS_START, dtype=F64)), "the stats moved without a valid pixel"
        assert bitwise_equal(given, torch.zeros(6, dtype=F64))
        assert bitwise_equal(grad, torch.full_like(grad, DC.GRAD_START)), "the gradient moved without a valid pixel"
        assert bitwise_equal(grad0, torch.zeros_like(grad0))
        assert bsum is None or (float(bsum) == DC.BSUM_START and float(bsum0) == 0.0)
    MC.hold(f"depth loss {DC.case_id(c)}", DC.items(c, inp, given, DC.shared_ref(c)), outs,
            WORST.setdefault(MC.NAME[c["dt"]], {}))


SEAM = dict(shape="x16_seam", mask="random")


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "fp16"])
def test_berhu_at_theta_one_is_l1(dt):
    """c is the maximum itself: no pixel lies above it, sum b(e) is sum e and the gradient L1's, bit for bit"""
    c = find(cfg="l1", dt=dt, **SEAM)
    inp = DC.inputs(c)
    l1 = Buffers(c, inp)
    bh = Buffers(c, inp, weights=(0.0, 0.0, 1.0), theta=1.0)
    s1, sb = l1.stats((0.0,) * 6), bh.stats((0.0,) * 6)
    assert bitwise_equal(s1[:4], sb[:4]) and float(s1[4]) == 0.0 and float(sb[4]) > 0.0
    _, g1 = l1.finish(s1, 0.0)
    bsum, gb = bh.finish(sb, 0.0, bsum_start=0.0)
    assert bitwise_equal(bsum.reshape(()), sb[3]), (float(bsum), float(sb[3]))
    assert bitwise_equal(gb, g1), int((gb != g1).sum())


@pytest.mark.parametrize("cfg", list(DC.CONFIGS))
def test_prediction_equal_to_target(cfg):
    """the identity shape with pred == target: r = 0 everywhere, sign(0) = 0 and c = 0 never divides"""
    c = find(shape="identity", dt=F32, mask="none", cfg=cfg)
    inp = DC.inputs(c)
    inp["target"] = inp["pred"].float().abs() + 1.0
    inp["pred"] = inp["target"].clone()
    buf = Buffers(c, inp)
    st = buf.stats((0.0,) * 6)
    bsum, grad = buf.finish(st, DC.GRAD_START, bsum_start=0.0)
    print(f"pred == target {cfg}: stats {st.tolist()}, sum b {None if bsum is None else float(bsum)}")
    assert float(st[2]) == 36 and float(st[3]) == 0.0 and float(st[4]) == 0.0
    assert float(st[0]) == 0.0 and float(st[1]) == 0.0  # d = log p - log p
    assert bsum is None or float(bsum) == 0.0
    assert bitwise_equal(grad, torch.full_like(grad, DC.GRAD_START)), "a gradient at r = 0"


@pytest.mark.parametrize("cfg", ["berhu0.2", "all"])
def test_two_runs_are_bitwise_equal(cfg):
    c = find(cfg=cfg, dt=BF16, **SEAM)
    inp = DC.inputs(c)
    runs = []
    for _ in range(2):
        buf = Buffers(c, inp)
        st = buf.stats((0.0,) * 6)
        runs.append((st,) + buf.finish(st, 0.0, bsum_start=0.0))
    for a, b in zip(*runs):
        assert bitwise_equal(a, b)


# ----------------------------------------------------------------------------- NaN
def raw_passes(c, inp):
    """both passes from zero on a 0xFF workspace, without run_poisoned (which demands finite results)"""
    B, h, w, H, W = DC.dims(c)
    buf = Buffers(c, inp)
    stats, grad = guarded(6, F64), guarded((B, h, w), F32)
    bsum = guarded(1, F64) if buf.terms & DC.BERHU else None
    buf.ws.fill(0xFF)
    buf.call_stats(stats)
    buf.ws.fill(0xFF)
    buf.call_finish(stats, bsum, grad)
    out = stats.t.cpu(), (torch.zeros(1, dtype=F64) if bsum is None else bsum.t.cpu()), grad.t.cpu()
    for g in buf.inputs + [buf.ws, stats, grad] + ([] if bsum is None else [bsum]):
        g.check()
    return out


def readers(c, b, i, j):
    """the high-res pixels (B, H, W) bool whose resized value reads low-res element (b, i, j), by index"""
    B, h, w, H, W = DC.dims(c)
    y0, y1, _, _ = MC.lerp(h, H)
    x0, x1, _, _ = MC.lerp(w, W)
    r = torch.zeros(B, H, W, dtype=torch.bool)
    r[b] = ((y0 == i) | (y1 == i))[:, None] & ((x0 == j) | (x1 == j))[None, :]
    return r


@pytest.mark.parametrize("cfg", list(DC.CONFIGS))
def test_nan_prediction_under_the_mask(cfg):
    c = find(cfg=cfg, dt=F32, **SEAM)
    inp = DC.inputs(c)
    b, i, j = 1, 1, 32  # the one column of the second chunk
    assert int((readers(c, b, i, j) & DC.in_mask(inp)).sum()) > 0
    inp["pred"][b, i, j] = float("nan")
    stats, bsum, _ = raw_passes(c, inp)
    print(f"NaN prediction under the mask {cfg}: stats {stats.tolist()}, sum b {bsum.tolist()}")
    assert DC.nan_verdict(c, stats, bsum, DC.in_mask(inp).sum()) == []


@pytest.mark.parametrize("cfg", list(DC.CONFIGS))
def test_nan_target_under_the_mask(cfg):
    c = find(cfg=cfg, dt=F32, **SEAM)
    inp = DC.inputs(c)
    b, y, x = DC.in_mask(inp).nonzero()[1234].tolist()
    inp["target"][b, y, x] = float("nan")
    stats, bsum, _ = raw_passes(c, inp)
    print(f"NaN target under the mask {cfg}: stats {stats.tolist()}, sum b {bsum.tolist()}")
    assert DC.nan_verdict(c, stats, bsum, DC.in_mask(inp).sum()) == []


@pytest.mark.parametrize("cfg", ["berhu0.9", "all"])
def test_nan_prediction_under_masked_out_pixels_changes_nothing(cfg):
    """every pixel that reads the NaN element is masked out: both passes are those of the reference, which
    never sees the element (it holds 0 there)"""
    c = find(cfg=cfg, dt=F32, **SEAM)
    inp = DC.inputs(c)
    b, i, j = 0, 1, 5
    r = readers(c, b, i, j)
    inp["mask"][r] = 0
    inp["target"][r] = float("nan")
    clean = dict(inp, pred=inp["pred"].clone())
    clean["pred"][b, i, j] = 0.0
    assert not bool((r & DC.in_mask(inp)).any())
    inp["pred"][b, i, j] = float("nan")
    stats, bsum, grad = raw_passes(c, inp)
    f = DC.forward_ref(c, clean)
    outs = dict(DC.split_stats(stats, (0.0,) * 6), grad=grad, Sb=bsum)
    its = DC.stats_items(c, clean, (0.0,) * 6, f) + DC.finish_items(c, clean, stats, 0.0, fwd=f)
    MC.hold(f"depth loss NaN under masked-out pixels {cfg}", its, outs)


# ----------------------------------------------------------------------------- above the ABI
OPS_CASES = [find(shape=s, dt=dt, mask=m, cfg=k)
             for s, dt, m, k in (("x16_seam", BF16, "random", "all"), ("x16_seam", F16, "none", "berhu0.2"),
                                 ("odd", F32, "random", "berhu0.9"), ("odd", BF16, "none", "l1"),
                                 ("flat", F16, "random", "all"), ("down", BF16, "random", "berhu0.2"),
                                 ("two_chunks", BF16, "random", "l1"))]


def op_inputs(c, inp):
    B, h, w, H, W = DC.dims(c)
    pred = inp["pred"].reshape(B, 1, h, w).to(DEV).requires_grad_(True)
    mask = None if inp["mask"] is None else (inp["mask"] != 0).reshape(B, 1, H, W).to(DEV)
    return pred, inp["target"].reshape(B, 1, H, W).to(DEV), mask


def op_loss(c, pred, target, mask):
    from denseclip_vit_multimodal_amd import ops
    w_s, w_1, w_b = DC.weights(c)
    return ops.upsample_depth_loss(pred, target, mask, silog=w_s, l1=w_1, berhu=w_b, lambd=DC.LAMBD, eps=DC.EPS,
                                   berhu_threshold=DC.theta(c))


@pytest.mark.parametrize("c", OPS_CASES, ids=[DC.case_id(c) for c in OPS_CASES])
def test_ops_loss_and_gradient(c):
    """ops.UpsampleDepthLossFn: the loss within what the sums' bounds allow, the gradient in the prediction's
    dtype and exactly the ABI's finish pass (from zero) times the incoming 0.1, rounded once; a call
    captured in a graph and replayed gives the same bits; under no_grad the same loss"""
    from denseclip_vit_multimodal_amd import ops
    inp = DC.inputs(c)
    pred, target, mask = op_inputs(c, inp)
    n0 = ops.STATS.get("upsample_depth_loss", 0)
    loss = op_loss(c, pred, target, mask)
    assert ops.STATS.get("upsample_depth_loss", 0) == n0 + 1, "the depth-loss kernels did not run"
    assert loss.dtype == F32 and loss.dim() == 0
    buf = Buffers(c, inp)
    given = buf.stats((0.0,) * 6)
    ref, bound = DC.loss_ref(c, inp, given, DC.shared_ref(c))
    err = abs(float(loss.detach()) - ref)
    print(f"ops {DC.case_id(c)}: loss {float(loss.detach())!r} vs fp64 {ref!r}: |err| / bound {err / bound:.3f}")
    assert err <= bound
    (loss * 0.1).backward()
    assert pred.grad.dtype == c["dt"] and pred.grad.shape == pred.shape
    _, g0 = buf.finish(given, 0.0, bsum_start=0.0)
    want = (g0 * torch.tensor(0.1, dtype=F32)).to(c["dt"]).reshape(pred.shape)
    assert bitwise_equal(pred.grad.cpu(), want), int((pred.grad.cpu() != want).sum())
    with torch.no_grad():
        assert bitwise_equal(op_loss(c, pred, target, mask), loss.detach()), "the forward-only form's loss differs"
    # captured and replayed
    static = pred.detach().clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op_loss(c, static, target, mask).backward()
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl = op_loss(c, static, target, mask)
        (gl * 0.1).backward()
    for _ in range(2):
        static.grad.zero_()
        graph.replay()
        assert bitwise_equal(gl.detach(), loss.detach()) and bitwise_equal(static.grad, pred.grad)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "fp16"])
def test_ops_empty_mask(dt):
    c = find(shape="x16_seam", dt=dt, mask="empty", cfg="all")
    pred, target, mask = op_inputs(c, DC.inputs(c))
    assert mask.dtype == torch.bool and not bool(mask.any())
    loss = op_loss(c, pred, target, mask)
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert pred.grad.dtype == dt and bool((pred.grad == 0).all())


def test_silog_alone_runs_todays_kernels():
    """only silog > 0: UpsampleSILogFn times the weight, the new kernels stay out of it"""
    from denseclip_vit_multimodal_amd import ops
    c = find(shape="odd", dt=BF16, mask="random", cfg="all")
    pred, target, mask = op_inputs(c, DC.inputs(c))
    n0 = ops.STATS.get("upsample_depth_loss", 0)
    loss = ops.upsample_depth_loss(pred, target, mask, silog=0.5)
    assert ops.STATS.get("upsample_depth_loss", 0) == n0
    want = 0.5 * ops.UpsampleSILogFn.apply(pred.detach(), target, mask, 0.5, 1e-6)
    assert bitwise_equal(loss.detach(), want)


def test_opcheck():
    from denseclip_vit_multimodal_amd import ops
    c = find(shape="odd", dt=BF16, mask="random", cfg="all")
    B, h, w, H, W = DC.dims(c)
    inp = DC.inputs(c)
    pred = inp["pred"].reshape(B, 1, h, w).to(DEV)
    target, mask = inp["target"].to(DEV), inp["mask"].to(DEV)
    DL = ops.DL()
    utils = ("test_schema", "test_faketensor", "test_aot_dispatch_dynamic")  # as the other ops' opchecks
    for mk in (mask, None):
        tg = target if mk is not None else torch.nan_to_num(target, nan=1.0)
        torch.library.opcheck(DL.upsample_depth_stats, (pred, tg, mk, DC.EPS, 7), test_utils=utils)
        stats = DL.upsample_depth_stats(pred, tg, mk, DC.EPS, 7)
        for want_grad in (True, False):
            torch.library.opcheck(DL.upsample_depth_finish,
                                  (pred, tg, mk, stats, DC.EPS, DC.LAMBD, 7, 1.0, 0.5, 0.25, 0.2, want_grad),
                                  test_utils=utils)
    for bad, needle in (((pred[:, 0], tg, mk, DC.EPS, 7), "pred"), ((pred, tg.double(), mk, DC.EPS, 7), "target"),
                        ((pred, tg[:, :-1], mask, DC.EPS, 7), "mask"), ((pred, tg, mask.bool(), DC.EPS, 7), "mask"),
                        ((pred.cpu(), tg, mk, DC.EPS, 7), "GPU"), ((pred, tg, mk, DC.EPS, 0), "a non-empty set"),
                        ((pred, tg, mk, DC.EPS, 8), "a non-empty set")):
        with pytest.raises(RuntimeError, match=needle):
            DL.upsample_depth_stats(*bad)
    fin = (DC.EPS, DC.LAMBD, 7, 1.0, 0.5, 0.25, 0.2, True)
    for bad, needle in (((pred, tg, mk, stats[:5]) + fin, "stats"), ((pred, tg, mk, stats.float()) + fin, "stats"),
                        ((pred, tg, mk, stats.cpu()) + fin, "GPU"),
                        ((pred, tg, mk, stats, DC.EPS, DC.LAMBD, 3, 1.0, 0.5, 0.25, 0.2, True), "not built for"),
                        ((pred, tg, mk, stats, DC.EPS, DC.LAMBD, 7, 1.0, -0.5, 0.25, 0.2, True), "finite and >= 0"),
                        ((pred, tg, mk, stats, DC.EPS, DC.LAMBD, 7, 1.0, 0.5, 0.25, 1.5, True), "0 < threshold"),
                        ((pred, tg, mk, stats, DC.EPS, DC.LAMBD, 7, 1.0, 0.5, 0.0, 0.2, False), "nothing to compute")):
        with pytest.raises(RuntimeError, match=needle):
            DL.upsample_depth_finish(*bad)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mask_kind", ["random", "none"])
@pytest.mark.parametrize("cfg", ["l1", "all"])
def test_train_loss_fn_depth_term(cfg, mask_kind):
    """train.loss_fn on a model output that holds the two low-res maps only, seg_weight = 0: 0.1 x the
    configured depth loss"""
    from denseclip_vit_multimodal_amd import train
    from denseclip_vit_multimodal_amd.losses import DepthLoss
    c = find(shape="x16_seam", dt=BF16, mask=mask_kind, cfg=cfg)
    B, h, w, H, W = DC.dims(c)
    inp = DC.inputs(c)
    pred, target, mask = op_inputs(c, inp)
    g = MC.gen(77)
    logits = MC.randn(g, B, 19, h, w).to(DEV)
    seg = torch.full((B, H, W), 255, dtype=torch.int64)
    seg[:, ::3, ::5] = torch.randint(0, 19, seg[:, ::3, ::5].shape, generator=g)  # some valid labels: a finite CE
    out = {"main_output_lowres": logits, "depth_output_lowres": pred}
    w_s, w_1, w_b = DC.weights(c)
    dl = DepthLoss(silog=w_s, l1=w_1, berhu=w_b, lambd=DC.LAMBD, eps=DC.EPS, berhu_threshold=DC.theta(c))
    loss = train.loss_fn(out, seg.to(DEV), target, mask, seg_weight=0.0, depth_loss=dl)
    given = Buffers(c, inp).stats((0.0,) * 6)
    ref, bound = DC.loss_ref(c, inp, given, DC.shared_ref(c))
    # 0.1 as the double the trainer multiplies by, the f32 product's rounding on top
    err = abs(float(loss.detach()) - 0.1 * ref)
    allowed = 0.1 * bound + 2 * DC.U * abs(0.1 * ref)
    print(f"loss_fn {DC.case_id(c)}: {float(loss.detach())!r} vs 0.1 x fp64 {0.1 * ref!r}: |err| / bound {err / allowed:.3f}")
    assert err <= allowed


# ----------------------------------------------------------------------------- training level
def _model(cdt):
    from denseclip_vit_multimodal_amd import DenseCLIP
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **MID_CFG)
    m.load_state_dict(spec_state_dict("mid"))
    m.backbone.compute_dtype = cdt
    m = m.to(DEV).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    for p in m.parameters():
        p.requires_grad_(True)
    return m


def _depth_loss():
    from denseclip_vit_multimodal_amd.train import depth_loss_config
    return depth_loss_config({"training": {"depth_loss": {"terms": {"silog": 1.0, "l1": 0.5, "berhu": 0.25}}}})


@pytest.mark.parametrize("cdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fused_depth_loss_matches_materialised(cdt):
    """test_gpu_parity.py::test_fused_head_loss_matches_materialised with a configured depth loss, its
    tolerances (loss 1e-4 relative; gradients rel_err 2e-3, 2e-2 behind the ViT's 16-bit backward).  The fp16
    steps take exact gradient scales: the delayed ones carry state from one backward into the next."""
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.train import loss_fn, synth_batch
    torch.manual_seed(0)
    m = _model(cdt)
    img, seg, depth, mask = synth_batch(1, 128, 256, torch.device(DEV), image_dtype=torch.float32)
    dl = _depth_loss()
    saved = ops.FP16_DELAYED_SCALE
    ops.FP16_DELAYED_SCALE = False
    try:
        res = []
        for fused in (False, True):
            m.fused_head_loss = fused
            m.zero_grad(set_to_none=True)
            n0 = ops.STATS.get("upsample_depth_loss", 0)
            out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
            loss = loss_fn(out, seg, depth, mask, depth_loss=dl)
            loss.backward()
            assert ops.STATS.get("upsample_depth_loss", 0) == n0 + int(fused)
            res.append((float(loss.detach()),
                        {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
    finally:
        ops.FP16_DELAYED_SCALE = saved
    (l0, g0), (l1, g1) = res
    worst = {True: 0.0, False: 0.0}
    for k in g0:
        worst[k.startswith("backbone.")] = max(worst[k.startswith("backbone.")], rel_err(g1[k], g0[k]))
    print(f"materialised {l0!r}, fused {l1!r}; worst gradient rel_err: backbone {worst[True]:.2e}, other {worst[False]:.2e}")
    assert abs(l0 - l1) < 1e-4 * abs(l0), (l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 20
    for k in g0:
        assert rel_err(g1[k], g0[k]) < (2e-2 if k.startswith("backbone.") else 2e-3), k


def test_captured_train_step_with_a_depth_loss_replays_and_none_is_todays_loss():
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.train import (CapturedTrainStep, freeze_for_mode, loss_fn, make_optimizer,
                                                    synth_batch, train_step)
    batch = synth_batch(1, 128, 256, torch.device(DEV), image_dtype=torch.float32)
    img, seg, depth, mask = batch
    m = _model(torch.bfloat16)
    m.fused_head_loss = True
    # depth_loss=None: the parent's loss, bit for bit, through the plain kernels
    with torch.no_grad():
        out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
        n0 = ops.STATS.get("upsample_depth_loss", 0)
        today = 1.0 * ops.UpsampleCEFn.apply(out["main_output_lowres"], seg, 255) \
            + 0.1 * ops.UpsampleSILogFn.apply(out["depth_output_lowres"], depth, mask, 0.5, 1e-6)
        assert bitwise_equal(loss_fn(out, seg, depth, mask), today)
        assert bitwise_equal(loss_fn(out, seg, depth, mask, depth_loss=None), today)
        assert ops.STATS.get("upsample_depth_loss", 0) == n0
    dl = _depth_loss()

    def make():
        torch.manual_seed(0)
        mm = _model(torch.bfloat16)
        mm.fused_head_loss = True
        return mm, make_optimizer(freeze_for_mode(mm, "F"), capturable=True)

    ma, oa = make()
    eager = [float(train_step(ma, oa, batch, depth_loss=dl)) for _ in range(5)]
    mb, ob = make()
    cap = CapturedTrainStep(mb, ob, batch, depth_loss=dl)
    replays = [float(cap()), float(cap())]
    torch.cuda.synchronize()
    print(f"eager {eager}, captured {replays}")
    assert all(v == v and abs(v) != float("inf") for v in eager + replays)
    assert replays == eager[3:], (replays, eager)
