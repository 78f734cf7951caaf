"""dclip_upsample_silog (csrc/headloss.hip: band_fold_kernel MODE 1 and MODE 2, band_sums_kernel,
band_merge_kernel), the depth half of every training step, behind the C ABI on guard-banded, poisoned
buffers (abi_guard.py), both passes against an fp64 reference: the three sums each to its bound, the
gradient per low-res element (silog_check.py: the cases, the reference, the bounds and why they hold).

What test_upsample_silog_vs_reference cannot see, going through ops.py, f32 predictions and one norm
over the whole gradient:
  * bf16 and fp16 predictions, which is what the model hands the kernel;
  * one pixel, one chunk-seam column or one band row missing from the fold: every low-res element
    has its own bound and none is excluded (test_silog_contract_emulation_cpu.py plants them);
  * a workspace or an output that already holds the answer: the workspace enters as 0xFF, then as
    0x3C (run_poisoned), at the size dclip_upsample_ws_floats gives, never more;
  * accumulators that start from non-zero values: the sums at (1.5, 2.5, 3.0), the gradient at 0.25;
  * pass 1 on its own: from the sums a separate pass 0 wrote, which it must leave bitwise unchanged
    and which the reference takes as they are;
  * a mask without a valid pixel (sums exactly zero, the gradient exactly its start), mask bytes
    other than 0 / 1, targets below eps, NaN in every masked-out target, h == 1, w == 1, a second
    chunk of one column, bands and low-res elements that own no pixel (bound 0: back as they went in);
  * NaN: one in the resized prediction or in a target under the mask makes sums[0..1] NaN, as
    torch.clamp in losses.SILogLoss does (the trainer then skips the step); one under masked-out pixels
    alone changes nothing.
Above the ABI, ops.UpsampleSILogFn and train.loss_fn are held to the same reference.
At the end the module prints, per dtype, the worst figure over its cases as a fraction of its bound.

The kernels on the MI355X over all 162 cases (177 tests, 4.6 s), next to the f32 emulation, worst
figure / bound (f32 | bf16 | fp16 predictions); reports, not thresholds:
    output                          kernels                  emulation
    sums[0] = sum d                 0.110 | 0.050 | 0.069    0.042 | 0.049 | 0.085
    sums[1] = sum d^2               0.297 | 0.212 | 0.238    0.065 | 0.132 | 0.252
    sums[2] = T                     exact                    exact
    grad onto 0.25                  0.988 | 0.979 | 0.983    the same   (the rounding of the add onto 0.25)
    grad onto zero ("grad0")        0.267 | 0.246 | 0.266    0.146 | 0.136 | 0.145
The gradient is also run from zero because next to 0.25 the last add's rounding (u / 4) is a thousand
times a typical element's own bound; from zero the fold itself is what the bound weighs.
As first written, with logf(fmaxf(x, eps)), the kernel failed the two NaN tests (sums of -3071.19 /
1037854.04 with a NaN prediction, 10072.78 / 834453.66 with a NaN target: fmaxf returns eps for a
NaN) and passed everything else with the figures above; the clamp is now the select x < eps ? eps : x.
"""
import pytest
import torch

import misc_check as MC
import silog_check as SC
from abi_guard import bitwise_equal, guarded, guarded_copy, run_poisoned
from misc_check import BF16, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
WORST = {}  # dtype name -> {output: worst figure / bound} over this session
CASES = SC.cases()


@pytest.fixture(autouse=True)
def _need(hip):
    pass


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key, w in sorted(WORST.items()):
        print(f"\nsilog contract dclip_upsample_silog {key}: worst figure / bound "
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

    def __init__(self, c, inp):
        self.c, (B, h, w, H, W) = c, SC.dims(c)
        self.pred = guarded_copy(inp["pred"].reshape(B, 1, h, w).to(DEV))
        self.target = guarded_copy(inp["target"].to(DEV))
        self.mask = None if inp["mask"] is None else guarded_copy(inp["mask"].to(DEV))
        self.ws = guarded(int(NT().lib().dclip_upsample_ws_floats(B, 1, h, w)), F32)
        self.inputs = [g for g in (self.pred, self.target, self.mask) if g is not None]

    def call(self, npass, sums, grad):
        B, h, w, H, W = SC.dims(self.c)
        NT().call("dclip_upsample_silog", npass, code(self.c["dt"]), self.pred.ptr(), B, h, w, self.target.ptr(),
                  None if self.mask is None else self.mask.ptr(), H, W, self.c["eps"], self.c["lambd"], sums.ptr(),
                  None if grad is None else grad.ptr(), self.ws.ptr(), stream())

    def pass0(self, start):
        """sums (f64[3], on the host) after a poisoned pass 0 onto `start`"""
        sums, first = guarded(3, F64), torch.tensor(start, dtype=F64, device=DEV)

        def fn():
            sums.t.copy_(first)
            self.call(0, sums, None)

        s, = run_poisoned(fn, inputs=self.inputs, scratch=[self.ws], accum=[sums])
        return s.cpu()

    def pass1(self, given, start):
        """the gradient (B, h, w) after a poisoned pass 1 from `given` onto `start`; `given` is an
        input: guarded, and bitwise unchanged afterwards"""
        B, h, w, H, W = SC.dims(self.c)
        gsum, grad = guarded_copy(given.to(DEV)), guarded((B, h, w), F32)

        def fn():
            grad.t.fill_(start)
            self.call(1, gsum, grad)

        g, = run_poisoned(fn, inputs=self.inputs + [gsum], scratch=[self.ws], accum=[grad])
        assert bitwise_equal(gsum.t.cpu(), given), "pass 1 wrote to its sums"
        return g.cpu()


@pytest.mark.parametrize("c", CASES, ids=[SC.case_id(c) for c in CASES])
def test_both_passes(c):
    """pass 0 onto (1.5, 2.5, 3.0), pass 1 onto 0.25 and onto zero from the sums of a separate pass 0 that started at zero"""
    inp = SC.inputs(c)
    buf = Buffers(c, inp)
    start = torch.tensor(SC.SUMS_START, dtype=F64)
    raw = buf.pass0(SC.SUMS_START)
    given = buf.pass0((0.0, 0.0, 0.0))
    grad = buf.pass1(given, SC.GRAD_START)
    s = raw - start
    outs = {"S0": s[0:1], "S1": s[1:2], "T": s[2:3], "grad": grad, "grad0": buf.pass1(given, 0.0)}
    if c["mask"] == "empty":
        assert bitwise_equal(raw, start), "the sums moved without a valid pixel"
        assert bitwise_equal(given, torch.zeros(3, dtype=F64))
        assert bitwise_equal(grad, torch.full_like(grad, SC.GRAD_START)), "the gradient moved without a valid pixel"
        assert bitwise_equal(outs["grad0"], torch.zeros_like(grad))
    MC.hold(f"silog {SC.case_id(c)}", SC.items(c, inp, given), outs, WORST.setdefault(MC.NAME[c["dt"]], {}))


# ----------------------------------------------------------------------------- NaN
NAN_CASE = dict(shape="x16_seam", dt=F32, eps=1e-6, lambd=0.5, mask="random")


def raw_pass0(c, inp):
    """pass 0 from zero on a 0xFF workspace, without run_poisoned (which demands finite results)"""
    buf = Buffers(c, inp)
    sums = guarded(3, F64)
    buf.ws.fill(0xFF)
    buf.call(0, sums, None)
    out = sums.t.cpu()
    for g in buf.inputs + [buf.ws, sums]:
        g.check()
    return out


def readers(c, b, i, j):
    """the high-res pixels (B, H, W) bool whose resized value reads low-res element (b, i, j): by
    index, whatever the weight -- at the clamped first rows and columns l1 = 0 multiplies row / column
    1, and 0 x NaN is NaN here as it is in F.interpolate"""
    B, h, w, H, W = SC.dims(c)
    y0, y1, _, _ = MC.lerp(h, H)
    x0, x1, _, _ = MC.lerp(w, W)
    r = torch.zeros(B, H, W, dtype=torch.bool)
    r[b] = ((y0 == i) | (y1 == i))[:, None] & ((x0 == j) | (x1 == j))[None, :]
    return r


def test_nan_prediction_under_the_mask_reaches_the_sums():
    c = find(**NAN_CASE)
    inp = SC.inputs(c)
    b, i, j = 1, 1, 32  # the one column of the second chunk
    assert int((readers(c, b, i, j) & SC.in_mask(inp)).sum()) > 0
    inp["pred"][b, i, j] = float("nan")
    sums = raw_pass0(c, inp)
    print(f"NaN prediction under the mask: sums {sums.tolist()}")
    assert not bool(torch.isfinite(sums[0])) and not bool(torch.isfinite(sums[1]))
    assert float(sums[2]) == float(SC.in_mask(inp).sum())


def test_nan_target_under_the_mask_reaches_the_sums():
    c = find(**NAN_CASE)
    inp = SC.inputs(c)
    b, y, x = SC.in_mask(inp).nonzero()[1234].tolist()
    inp["target"][b, y, x] = float("nan")
    sums = raw_pass0(c, inp)
    print(f"NaN target under the mask: sums {sums.tolist()}")
    assert not bool(torch.isfinite(sums[0])) and not bool(torch.isfinite(sums[1]))
    assert float(sums[2]) == float(SC.in_mask(inp).sum())


def test_nan_prediction_under_masked_out_pixels_changes_nothing():
    """every pixel that reads the NaN element is masked out: the sums are those of the reference, which
    never sees the element (it holds 0 there and asserts that no pixel of the mask reads it)"""
    c = find(**NAN_CASE)
    inp = SC.inputs(c)
    b, i, j = 0, 1, 5
    r = readers(c, b, i, j)
    inp["mask"][r] = 0
    inp["target"][r] = float("nan")
    clean = dict(inp, pred=inp["pred"].clone())
    clean["pred"][b, i, j] = 0.0
    assert not bool((r & SC.in_mask(inp)).any())
    inp["pred"][b, i, j] = float("nan")
    sums = raw_pass0(c, inp)
    outs = {"S0": sums[0:1], "S1": sums[1:2], "T": sums[2:3]}
    MC.hold("silog NaN under masked-out pixels", SC.sums_items(c, clean), outs)


# ----------------------------------------------------------------------------- above the ABI
OPS_CASES = [find(shape=s, dt=dt, eps=1e-6, lambd=0.5, mask=m)
             for s, dt, m in (("x16_seam", BF16, "random"), ("x16_seam", F16, "none"), ("odd", F32, "random"),
                              ("odd", BF16, "none"), ("flat", F16, "random"), ("down", BF16, "random"))]
OPS_CASES.append(find(shape="two_chunks", dt=BF16, eps=0.5, lambd=0.85, mask="random"))


def op_inputs(c, inp):
    B, h, w, H, W = SC.dims(c)
    pred = inp["pred"].reshape(B, 1, h, w).to(DEV).requires_grad_(True)
    mask = None if inp["mask"] is None else (inp["mask"] != 0).reshape(B, 1, H, W).to(DEV)
    return pred, inp["target"].reshape(B, 1, H, W).to(DEV), mask


@pytest.mark.parametrize("c", OPS_CASES, ids=[SC.case_id(c) for c in OPS_CASES])
def test_ops_loss_and_gradient(c):
    """ops.UpsampleSILogFn: the loss within what the sums' bounds allow, the gradient in the
    prediction's dtype and exactly the ABI's pass 1 (from zero) times the incoming 0.1, rounded once"""
    from denseclip_vit_multimodal_amd import ops
    inp = SC.inputs(c)
    pred, target, mask = op_inputs(c, inp)
    loss = ops.UpsampleSILogFn.apply(pred, target, mask, c["lambd"], c["eps"])
    assert loss.dtype == F32 and loss.dim() == 0
    ref, bound = SC.loss_ref(c, inp)
    err = abs(float(loss.detach()) - ref)
    print(f"ops {SC.case_id(c)}: loss {float(loss.detach())!r} vs fp64 {ref!r}: |err| / bound {err / bound:.3f}")
    assert err <= bound
    (loss * 0.1).backward()
    assert pred.grad.dtype == c["dt"] and pred.grad.shape == pred.shape
    buf = Buffers(c, inp)
    given = buf.pass0((0.0, 0.0, 0.0))
    g0 = buf.pass1(given, 0.0)
    MC.hold(f"silog from zero {SC.case_id(c)}", SC.grad_items(c, inp, given, init=0.0), {"grad": g0})
    want = (g0 * torch.tensor(0.1, dtype=F32)).to(c["dt"]).reshape(pred.shape)
    assert bitwise_equal(pred.grad.cpu(), want), int((pred.grad.cpu() != want).sum())


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "fp16"])
def test_ops_empty_mask(dt):
    from denseclip_vit_multimodal_amd import ops
    c = find(shape="x16_seam", dt=dt, eps=1e-6, lambd=0.5, mask="empty")
    pred, target, mask = op_inputs(c, SC.inputs(c))
    assert mask.dtype == torch.bool and not bool(mask.any())
    loss = ops.UpsampleSILogFn.apply(pred, target, mask, c["lambd"], c["eps"])
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert pred.grad.dtype == dt and bool((pred.grad == 0).all())


@pytest.mark.parametrize("mask_kind", ["random", "none"])
def test_train_loss_fn_depth_term(mask_kind):
    """train.loss_fn on a model output that holds the two low-res maps only, seg_weight = 0: 0.1 x SILog"""
    from denseclip_vit_multimodal_amd import train
    from denseclip_vit_multimodal_amd.losses import SILogLoss
    c = find(shape="x16_seam", dt=BF16, eps=0.5, lambd=0.85, mask=mask_kind)
    B, h, w, H, W = SC.dims(c)
    inp = SC.inputs(c)
    pred, target, mask = op_inputs(c, inp)
    g = MC.gen(77)
    logits = MC.randn(g, B, 19, h, w).to(DEV)
    seg = torch.full((B, H, W), 255, dtype=torch.int64)
    seg[:, ::3, ::5] = torch.randint(0, 19, seg[:, ::3, ::5].shape, generator=g)  # some valid labels: a finite CE
    out = {"main_output_lowres": logits, "depth_output_lowres": pred}
    loss = train.loss_fn(out, seg.to(DEV), target, mask, silog=SILogLoss(lambd=c["lambd"], eps=c["eps"]), seg_weight=0.0)
    ref, bound = SC.loss_ref(c, inp)
    # 0.1 as the double the trainer multiplies by, the f32 product's rounding on top
    err = abs(float(loss.detach()) - 0.1 * ref)
    allowed = 0.1 * bound + 2 * SC.U * abs(0.1 * ref)
    print(f"loss_fn {SC.case_id(c)}: {float(loss.detach())!r} vs 0.1 x fp64 {0.1 * ref!r}: |err| / bound {err / allowed:.3f}")
    assert err <= allowed
