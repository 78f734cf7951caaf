"""The identity-head branch on the GPU: dclip_score_map_bwd (csrc/scoregrad.hip) against fp64 on poisoned,
guard-banded buffers, the op layer (torch.ops.dclip_classes.score_map_bwd, ops.ScoreMapFn), and the model /
trainer wiring (one train step, its loss and gradients, the captured step, the refusals).

Bounds.  The kernel rounds nowhere before its stores, so its emulation (tests/score_loss_ref.py) is the fp32
evaluation of the reference's lines.  Every output is held to

    max |hip - fp64|  <=  1.5 x EMULATED[case][output]  +  unit roundoff(output dtype) x max |fp64|

(test_gpu_grad_parity.py's rule; the 1.5 covers the summation order).  EMULATED is the table that
`python tests/score_loss_ref.py` prints (max |fp32 autograd - fp64 autograd| of dv stored in f32, dv stored
in v's dtype, dt), recorded here:
"""
import ctypes

import pytest
import torch

import score_loss_ref as R
from abi_guard import GuardedStrided, bitwise_equal, guarded, guarded_copy, guarded_rows_copy, run_poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
EMULATED = {
    '2x5x7x48x19-bf16': (5.878e-09, 6.011e-05, 1.777e-08),
    '2x5x7x48x19-f16': (4.055e-09, 7.615e-06, 1.802e-08),
    '2x8x16x512x19-bf16': (6.963e-10, 7.517e-06, 7.973e-09),
    '2x8x16x512x19-f16': (7.438e-10, 9.539e-07, 7.643e-09),
    '1x17x61x64x19-bf16': (4.052e-09, 6.101e-05, 1.382e-07),
    '1x17x61x64x19-f16': (4.258e-09, 7.625e-06, 1.285e-07),
    '2x4x9x64x1-bf16': (5.456e-10, 1.488e-05, 5.070e-09),
    '2x4x9x64x1-f16': (6.793e-10, 1.822e-06, 5.951e-09),
    '2x4x9x64x32-bf16': (6.080e-09, 6.054e-05, 1.616e-08),
    '2x4x9x64x32-f16': (4.801e-09, 7.112e-06, 1.460e-08),
    '2x4x9x64x33-bf16': (5.413e-09, 5.811e-05, 1.730e-08),
    '2x4x9x64x33-f16': (4.964e-09, 7.353e-06, 1.614e-08),
    '2x4x9x64x150-bf16': (2.313e-08, 1.203e-04, 2.037e-08),
    '2x4x9x64x150-f16': (2.505e-08, 1.480e-05, 2.145e-08),
    '2x4x9x64x256-bf16': (3.915e-08, 1.217e-04, 2.386e-08),
    '2x4x9x64x256-f16': (3.790e-08, 2.153e-05, 1.989e-08),
    '1x1x1x16x2-bf16': (5.945e-10, 3.487e-06, 5.076e-09),
    '1x1x1x16x2-f16': (1.077e-09, 1.901e-06, 3.966e-09),
    '1x3x5x768x19-bf16': (3.471e-10, 3.783e-06, 1.642e-09),
    '1x3x5x768x19-f16': (3.431e-10, 4.767e-07, 8.900e-10),
    '1x2x3x2048x33-bf16': (2.672e-10, 1.905e-06, 3.840e-10),
    '1x2x3x2048x33-f16': (1.750e-10, 2.374e-07, 2.577e-10),
    '2x3x3x1040x19-bf16': (3.494e-10, 3.780e-06, 6.460e-10),
    '2x3x3x1040x19-f16': (2.242e-10, 4.336e-07, 4.867e-10),
}


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def _N():
    from denseclip_vit_multimodal_amd import _native as N
    return N


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_bwd(v, t, ds, dv_dt, token=False, scale=1.0, eps=R.EPS):
    """dclip_score_map_bwd through run_poisoned: v (B, HW, C) 16-bit, t (B, K, C), ds (B, K, HW) on the CPU.
    token: v and dv as token buffers (row_off 1, bstride (HW + 1) C; v's CLS rows hold NaN, dv's must come back
    untouched).  dt and the workspace start from 0xFF (then 0x3C): dt is fully overwritten and nothing is read
    before it is written.  Returns (dv (B, HW, C), dt (B, K, C)) on the CPU."""
    N = _N()
    B, HW, C = v.shape
    K = t.shape[1]
    off = 1 if token else 0
    gv, bstride = guarded_rows_copy(v.to(DEV), C, off)
    gt, gds = guarded_copy(t.to(DEV)), guarded_copy(ds.to(DEV))
    gdv = GuardedStrided((B, HW, C), (bstride, C, 1), dv_dt, 0, off * C)
    gdt = guarded((B, K, C), torch.float32)
    nws = int(N.lib().dclip_score_map_bwd_ws_floats(B, HW, C, K))
    assert nws > 0
    gws = guarded(nws, torch.float32)

    def fn():
        N.call("dclip_score_map_bwd", gv.ptr(), DT[v.dtype], bstride, off, C, gt.ptr(), gds.ptr(), float(scale),
               gdv.ptr(), DT[dv_dt], bstride, off, C, gdt.ptr(), gws.ptr(), B, HW, C, K, float(eps), _stream())

    dv, dt = run_poisoned(fn, inputs=[gv, gt, gds], outputs=[gdv, gdt], scratch=[gws])
    return dv.cpu(), dt.cpu()


def check_case(shape, v_dt, dv_dt, token):
    cid = R.case_id(shape, v_dt)
    v, t, ds = R.inputs(shape, v_dt)
    rdv, rdt = R.reference(shape, v_dt)
    dv, dt = run_bwd(v, t, ds, dv_dt, token=token)
    e32, e16, et = EMULATED[cid]
    err_v = float((dv.double() - rdv).abs().max())
    err_t = float((dt.double() - rdt).abs().max())
    bv = R.bound(e32 if dv_dt == torch.float32 else e16, dv_dt, rdv)
    bt = R.bound(et, torch.float32, rdt)
    print(f"{cid} dv_dt={dv_dt} token={token}: dv err {err_v:.3e} (bound {bv:.3e}), dt err {err_t:.3e} (bound {bt:.3e})")
    assert err_v <= bv, (cid, err_v, bv)
    assert err_t <= bt, (cid, err_t, bt)


@pytest.mark.parametrize("dv16", [False, True], ids=["dv_f32", "dv_16"])
@pytest.mark.parametrize("shape,v_dt", R.cases(), ids=[R.case_id(s, d) for s, d in R.cases()])
def test_kernel_against_fp64(shape, v_dt, dv16):
    check_case(shape, v_dt, v_dt if dv16 else torch.float32, token=False)


@pytest.mark.parametrize("dv16", [False, True], ids=["dv_f32", "dv_16"])
@pytest.mark.parametrize("shape,v_dt", [(R.SHAPES[0], torch.bfloat16), (R.SHAPES[2], torch.float16),
                                        (R.SHAPES[6], torch.bfloat16), (R.SHAPES[9], torch.bfloat16),
                                        (R.SHAPES[11], torch.float16)],
                         ids=["odd", "spans", "K150", "C768", "C1040"])
def test_token_buffer_addressing(shape, v_dt, dv16):
    """v and dv as token buffers: NaN CLS rows in v reach no output, dv's CLS rows (0xFF, then 0x3C) and every
    guard band come back untouched (run_poisoned), and the result meets the dense layout's bounds"""
    check_case(shape, v_dt, v_dt if dv16 else torch.float32, token=True)


def test_clamped_rows():
    """an all-zero pixel row and an all-zero text row with non-zero ds: dvn / eps and dtn / eps, finite in f32"""
    shape, v_dt = R.SHAPES[0], torch.bfloat16
    v, t, ds = (x.clone() for x in R.inputs(shape, v_dt))
    v[1, 9] = 0
    t[0, 4] = 0
    dv, dt = run_bwd(v, t, ds, torch.float32)
    rdv, rdt = R.closed_form(v, t, ds, torch.float64)
    assert bool(torch.isfinite(dv).all()) and bool(torch.isfinite(dt).all())
    # dvn / eps = sum_k ds tn_k / eps (the text row that is zero contributes nothing)
    tn = torch.nn.functional.normalize(t.double(), dim=2, eps=R.EPS)
    want_v = torch.einsum("k,kc->c", ds[1, :, 9].double(), tn[1]) / R.EPS
    vn = torch.nn.functional.normalize(v.double(), dim=2, eps=R.EPS)
    want_t = torch.einsum("p,pc->c", ds[0, 4].double(), vn[0]) / R.EPS
    rel_v = float((dv[1, 9].double() - want_v).abs().max() / want_v.abs().max())
    rel_t = float((dt[0, 4].double() - want_t).abs().max() / want_t.abs().max())
    print(f"clamped rows: rel err dv {rel_v:.3e} dt {rel_t:.3e}; max |dv| {float(dv.abs().max()):.3e}")
    # f32 sums of K = 19 (HW = 35) terms of ordinary size: 1e-5 relative is 2 orders above their rounding
    assert float(want_v.abs().max()) > 1e9 and rel_v < 1e-5 and rel_t < 1e-5
    # the other rows are what they are without the zero rows' help
    mask = torch.ones(v.shape[:2], dtype=torch.bool)
    mask[1, 9] = False
    assert float((dv[mask].double() - rdv[mask]).abs().max()) < 1e-6


def test_bitwise_and_scale():
    shape, v_dt = R.SHAPES[2], torch.bfloat16
    v, t, ds = R.inputs(shape, v_dt)
    a = run_bwd(v, t, ds, torch.float32)
    b = run_bwd(v, t, ds, torch.float32)
    assert bitwise_equal(a[0], b[0]) and bitwise_equal(a[1], b[1])
    scale = 1.0 / R.TAU
    s = run_bwd(v, t, ds, torch.float32, scale=scale)
    p = run_bwd(v, t, ds * scale, torch.float32)  # the same product, rounded to f32 once in either form
    assert bitwise_equal(s[0], p[0]) and bitwise_equal(s[1], p[1])


def test_host_checks():
    N = _N()
    L = N.lib()
    P = ctypes.c_void_p(0x1000)

    def call(K=19, v_dt=2, dv_dt=0, C=64, B=1, HW=8, v=P, t=P, ds=P, dv=P, dt=P, ws=P, dv_ld=None):
        return L.dclip_score_map_bwd(v, v_dt, HW * C, 0, C, t, ds, 1.0, dv, dv_dt, HW * C, 0, dv_ld or C, dt, ws, B, HW,
                                     C, K, 1e-12, None)

    for kw, needle in ((dict(K=0), "K=0"), (dict(K=257), "K=257"), (dict(v_dt=0), "f16/bf16"),
                       (dict(dv_dt=1), "dv_dt=1"), (dict(C=72), "C % 16"), (dict(C=4096), "C <= 2048"),
                       (dict(B=70000), "65535"), (dict(dv=None), "required"), (dict(ws=None), "ws"),
                       (dict(ws=ctypes.c_void_p(0x1004)), "ws"), (dict(dv_ld=68), "dv needs"), (dict(HW=0), "empty")):
        assert call(**kw) == -1, kw
        assert needle in L.dclip_last_error().decode(), (kw, L.dclip_last_error().decode())
    assert L.dclip_score_map_bwd_ws_floats(0, 8, 64, 19) == 0 and L.dclip_score_map_bwd_ws_floats(1, 8, 64, 257) == 0


# ----------------------------------------------------------------------------- op layer
def test_opcheck_and_scoremapfn():
    from denseclip_vit_multimodal_amd import ops
    shape, v_dt = R.SHAPES[0], torch.bfloat16
    B, h, w, C, K = shape
    v, t, ds = R.inputs(shape, v_dt)
    vd, td, dsd = v.to(DEV).view(B * h * w, C), t.to(DEV), ds.to(DEV)
    ops.D()
    op = torch.ops.dclip_classes.score_map_bwd
    torch.library.opcheck(op, (vd, h * w * C, 0, C, td, dsd, 1.0, B, h * w, R.EPS, torch.float32),
                          test_utils=("test_schema", "test_faketensor"))
    # ScoreMapFn on a channels-last map: forward bit-identical to ops.score_map, gradients within test 1's bounds
    vmap = vd.view(B, h, w, C).permute(0, 3, 1, 2).requires_grad_(True)
    tx = td.clone().requires_grad_(True)
    out = ops.ScoreMapFn.apply(vmap, tx)
    assert bitwise_equal(out.view(B, K, h * w), ops.score_map(vd, td, B, h * w))
    out.backward(dsd.view(B, K, h, w))
    rdv, rdt = R.reference(shape, v_dt)
    e32, e16, et = EMULATED[R.case_id(shape, v_dt)]
    gv = vmap.grad.permute(0, 2, 3, 1).reshape(B, h * w, C).cpu()
    assert vmap.grad.dtype == v_dt and float((gv.double() - rdv).abs().max()) <= R.bound(e16, v_dt, rdv)
    assert float((tx.grad.cpu().double() - rdt).abs().max()) <= R.bound(et, torch.float32, rdt)
    # scale: out = score / tau, the gradients those of ds / tau
    vmap2 = vmap.detach().requires_grad_(True)
    out2 = ops.ScoreMapFn.apply(vmap2, tx.detach(), R.EPS, 1.0 / R.TAU)
    assert torch.equal(out2, out.detach() * (1.0 / R.TAU))
    # a read-out map over its token buffer is read in place
    buf = torch.zeros(B, h * w + 1, C, dtype=v_dt, device=DEV)
    buf[:, 0] = float("nan")
    buf[:, 1:] = v.to(DEV)
    tmap = buf.view(-1).as_strided((B, C, h, w), ((h * w + 1) * C, 1, w * C, C), C).requires_grad_(True)
    assert ops.token_rows(tmap) is not None
    out3 = ops.ScoreMapFn.apply(tmap, td)
    assert bitwise_equal(out3, out.detach())
    out3.backward(dsd.view(B, K, h, w))
    assert bitwise_equal(tmap.grad.permute(0, 2, 3, 1).reshape(B, h * w, C).cpu(), gv)
    with pytest.raises(NotImplementedError, match="CPU"):
        op(v.view(-1, C), h * w * C, 0, C, t, ds, 1.0, B, h * w, R.EPS, torch.float32)


# ----------------------------------------------------------------------------- model and trainer
H_IMG, W_IMG = 128, 256
HEAD = dict(type="IdentityHead", loss_weight=0.4, in_channels=32, channels=32, num_classes=19, dropout_ratio=0.0,
            align_corners=False)


def build(cfg, name, head=HEAD, cdt=torch.bfloat16):
    from denseclip_vit_multimodal_amd import DenseCLIP
    from helpers import CITYSCAPES_CLASSES, spec_state_dict
    kw = {} if head is None else {"identity_head": head}
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(cfg, **kw))
    m.load_state_dict(spec_state_dict(name))
    m.backbone.compute_dtype = cdt
    m = m.to(DEV).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m.fused_head_loss = True
    return m


def _batch(B=1):
    from denseclip_vit_multimodal_amd.train import synth_batch
    return synth_batch(B, H_IMG, W_IMG, torch.device(DEV), image_dtype=torch.float32)


def test_train_step_trains_the_score_branch():
    """one train_step with the head on: vis_proj and the contexts get gradients (None on a tree without the
    identity head's wiring), and the loss it returns is seg CE + 0.1 SILog + 0.4 identity CE of the step's own
    low-res outputs (a forward hook keeps them), recomputed in fp64, within the fused CE's tolerance (1e-5
    relative, test_gpu_ce_options.py)"""
    import torch.nn.functional as F
    from denseclip_vit_multimodal_amd import losses, ops
    from denseclip_vit_multimodal_amd.train import (freeze_for_mode, gradless_parameter_names, identity_loss_weight,
                                                    loss_fn, make_optimizer, train_step)
    from helpers import MID_CFG
    m = build(MID_CFG, "mid")
    assert identity_loss_weight(m) == 0.4
    opt = make_optimizer(freeze_for_mode(m, "F"))
    batch = _batch()
    img, seg, depth, mask = batch
    n0 = ops.STATS.get("score_map_bwd", 0)
    kept = {}
    hook = m.register_forward_hook(lambda mod, args, out: kept.update(out=out))  # the step's own outputs
    loss = train_step(m, opt, batch, identity_weight=identity_loss_weight(m))
    hook.remove()
    assert ops.STATS.get("score_map_bwd", 0) == n0 + 1
    for p in (m.vis_proj.weight, m.vis_proj.bias, m.contexts):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
    # exactly the parameters gradless_parameter_names lists got no gradient
    dead = set(gradless_parameter_names(m))
    got = {n for n, p in m.named_parameters() if p.requires_grad and p.grad is None}
    assert got == dead, (sorted(got ^ dead))
    assert dead == {"backbone.proj", "gamma", "global_proj.weight", "global_proj.bias"}
    # the loss train_step returned against fp64 on the low-res outputs of that same forward
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in kept["out"].items()}
    got_loss = float(loss)
    # a model that returns identity logits needs the weight: its parameters are counted as alive
    with pytest.raises(ValueError, match="identity_weight"):
        loss_fn(out, seg, depth, mask)
    assert out["identity_output_lowres"].shape == (1, 19, H_IMG // 16, W_IMG // 16)
    assert out["identity_output_lowres"].dtype == torch.float32

    def up(t):
        return F.interpolate(t.double().cpu(), size=(H_IMG, W_IMG), mode="bilinear", align_corners=False)

    ce = float(F.cross_entropy(up(out["main_output_lowres"]), seg.cpu(), ignore_index=255))
    ce_id = float(F.cross_entropy(up(out["identity_output_lowres"]), seg.cpu(), ignore_index=255))
    sil = float(losses.SILogLoss()(up(out["depth_output_lowres"]), depth.double().cpu(), mask.cpu()))
    want = 1.0 * ce + 0.1 * sil + 0.4 * ce_id
    print(f"step loss {got_loss!r} vs fp64 {want!r} (ce {ce:.6f}, silog {sil:.6f}, identity ce {ce_id:.6f})")
    assert abs(got_loss - want) <= 1e-5 * (abs(ce) + 0.1 * abs(sil) + 0.4 * abs(ce_id))
    assert bool(torch.isfinite(loss))


def test_branch_gradients_against_fp64():
    """only the identity term weighted: the gradient at the last read-out map (a tensor hook) and vis_proj's
    weight gradient against the fp64 restatement of the branch (reference lines 672-675, / tau, resize, CE) run on
    the same 16-bit map values.  Bounds by test 1's rule from the branch's own emulation: the fp32 evaluation of
    the same lines with the pixel embeddings and their gradient stored in bf16, as vis_proj's GEMMs store them."""
    import torch.nn.functional as F
    from denseclip_vit_multimodal_amd.train import loss_fn
    from helpers import MID_CFG
    m = build(MID_CFG, "mid")
    for p in m.parameters():
        p.requires_grad_(True)
    img, seg, depth, mask = _batch()
    grabbed = {}
    orig = m._score_branch_train

    def spy(visual, cdt):
        grabbed["map"] = visual.detach().float().cpu()

        def keep(g):
            grabbed["dmap"] = g.detach().float().cpu()

        visual.register_hook(keep)
        text, logits = orig(visual, cdt)
        grabbed["text"] = text.detach().double().cpu()
        return text, logits

    m._score_branch_train = spy
    out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
    loss = loss_fn(out, seg, depth, mask, seg_weight=0.0, silog_weight=0.0, identity_weight=1.0)
    # the main heads' terms carry weight 0: what reaches the map through the neck is exactly 0
    loss.backward()
    W, b = m.vis_proj.weight.detach().cpu(), m.vis_proj.bias.detach().cpu()

    def branch(dtype, store16):
        x = grabbed["map"].to(dtype).requires_grad_(True)
        w = W.to(torch.bfloat16).to(dtype).requires_grad_(True) if store16 else W.to(dtype).requires_grad_(True)
        v = F.conv2d(x, w, b.to(dtype))
        if store16:
            v = _Round16.apply(v)
        l, _ = R.branch_loss(v, grabbed["text"].to(dtype), seg.cpu(), tau=m.tau)
        l.backward()
        return x.grad.double(), w.grad.double()

    rx, rw = branch(torch.float64, False)
    ex, ew = branch(torch.float32, True)
    ex = ex.to(torch.bfloat16).double()  # the input-gradient GEMM stores bf16
    gx, gw = grabbed["dmap"].double(), m.vis_proj.weight.grad.detach().cpu().double()
    for name, hip, emu, ref, odt in (("d map", gx, ex, rx, torch.bfloat16), ("d vis_proj.weight", gw, ew, rw, torch.float32)):
        e_hip, e_emu = float((hip - ref).abs().max()), float((emu - ref).abs().max())
        bound = R.bound(e_emu, odt, ref)
        print(f"{name}: hip err {e_hip:.3e}, emulated {e_emu:.3e}, bound {bound:.3e}, max |ref| {float(ref.abs().max()):.3e}")
        assert e_hip <= bound, (name, e_hip, bound)


class _Round16(torch.autograd.Function):
    """bf16 storage of a value and of its gradient (tests/emulation16.py's Round)"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def test_fp16_compute_is_refused():
    from helpers import MID_CFG
    m = build(MID_CFG, "mid", cdt=torch.float16)
    img, seg, depth, mask = _batch()
    with pytest.raises(NotImplementedError, match="fp16"):
        m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)


def test_materialised_mode_and_eval_are_untouched():
    from helpers import MID_CFG
    m = build(MID_CFG, "mid")
    m.fused_head_loss = False
    img, seg, depth, mask = _batch()
    out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
    assert set(out) == {"main_output", "depth_output", "aux_losses"}
    assert out["aux_losses"]["identity_head"].shape == (1, 19, H_IMG, W_IMG)
    low = m.forward_lowres(img)  # training mode, head on: the two maps, nothing kept on the module
    assert set(low) == {"seg", "depth"} and not hasattr(m, "_last_score")
    m = build(MID_CFG, "mid").eval()  # a fresh one: the training forward above moved the BN statistics
    with torch.no_grad():
        ev = m(img, return_loss=False)
    m0 = build(MID_CFG, "mid", head=None).eval()
    with torch.no_grad():
        ev0 = m0(img, return_loss=False)
    assert set(ev) == {"seg", "depth"} and bitwise_equal(ev["seg"], ev0["seg"]) and bitwise_equal(ev["depth"], ev0["depth"])
    m0.train()
    m0.fused_head_loss = True
    out0 = m0(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
    assert set(out0) == {"main_output", "depth_output", "aux_losses", "main_output_lowres", "depth_output_lowres"}
    assert out0["aux_losses"] == {}


def test_context_decoder_trains_too():
    """with a context decoder the text side is alive: gamma, the decoder and global_proj get gradients"""
    from denseclip_vit_multimodal_amd.train import freeze_for_mode, gradless_parameter_names, loss_fn
    from helpers import MID_CFG, TINY_CTX_CFG
    cfg = dict(MID_CFG, context_decoder=TINY_CTX_CFG["context_decoder"])
    from denseclip_vit_multimodal_amd import DenseCLIP
    from helpers import CITYSCAPES_CLASSES, spec_state_dict
    torch.manual_seed(3)
    m = DenseCLIP(class_names=CITYSCAPES_CLASSES, **dict(cfg, identity_head=HEAD))
    m.load_state_dict(spec_state_dict("mid"), strict=False)
    m.backbone.compute_dtype = torch.bfloat16
    m = m.to(DEV).train()
    with torch.no_grad():
        m.gamma.fill_(0.5)
    m.fused_head_loss = True
    freeze_for_mode(m, "F")
    img, seg, depth, mask = _batch()
    out = m(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
    loss_fn(out, seg, depth, mask, identity_weight=0.4).backward()
    dead = set(gradless_parameter_names(m))
    got = {n for n, p in m.named_parameters() if p.requires_grad and p.grad is None}
    assert dead == {"backbone.proj"} and got == dead, sorted(got ^ dead)
    for p in (m.gamma, m.global_proj.weight, m.contexts, next(m.context_decoder.parameters())):
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0


def test_captured_step_replays_and_equals_eager():
    """ViT-B/16 from the shipped YAML with the head on (width 768: every fold of the step has a fixed order, the
    narrow test widths' LayerNorm bias sums do not), mode F, bf16 images at 2 x 256 x 512: three replays after the
    three warm-up steps against six eager steps, losses and every parameter bit for bit"""
    from denseclip_vit_multimodal_amd.config import build_model, load_yaml
    from denseclip_vit_multimodal_amd.train import (CapturedTrainStep, freeze_for_mode, gradless_parameter_names,
                                                    identity_loss_weight, make_optimizer, synth_batch, train_step)
    batch = synth_batch(2, 256, 512, torch.device(DEV), 0)
    cfg = load_yaml("denseclip_cityscapes.yaml")
    cfg["model"]["identity_head"] = dict(type="IdentityHead", loss_weight=0.4)
    wt = identity_loss_weight(cfg)
    assert wt == 0.4

    def make():
        torch.manual_seed(0)
        mm = build_model(cfg, clip_path_override="").to(DEV).train()
        for mod in mm.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        mm.fused_head_loss = True
        return mm, make_optimizer(freeze_for_mode(mm, "F"), capturable=True)

    ma, oa = make()
    # the shipped config has no context decoder: exactly these stay without a gradient
    assert set(gradless_parameter_names(ma)) == {"backbone.proj", "gamma", "global_proj.weight", "global_proj.bias"}
    start = ma.contexts.detach().clone()
    eager = [float(train_step(ma, oa, batch, identity_weight=wt)) for _ in range(6)]
    mb, ob = make()
    cap = CapturedTrainStep(mb, ob, batch, identity_weight=wt)  # three eager warm-up steps
    replays = [float(cap()), float(cap()), float(cap())]
    torch.cuda.synchronize()
    print(f"eager {eager}, captured {replays}")
    assert all(v == v and abs(v) != float("inf") for v in eager + replays)
    assert replays == eager[3:]
    pa = dict(ma.named_parameters())
    diff = [n for n, p in mb.named_parameters() if not torch.equal(p, pa[n])]
    assert not diff, (len(diff), diff[:8])
    assert float((mb.contexts.detach() - start).abs().sum()) > 0 and mb.vis_proj.weight.grad is not None  # the branch trained


def test_a_model_without_the_head_computes_what_it_did():
    """one seeded training forward + loss + backward of the head-less ViT-B/16 (score_loss_ref.seeded_step): the
    loss and 64 samples of every parameter's gradient, bit for bit what the commit before the identity head gave
    (tests/golden/score_loss_parent_step.npz, recorded from that commit's build with the same function), and the
    same set of parameters with a gradient"""
    import os
    import numpy as np
    from helpers import GOLDEN
    want = np.load(os.path.join(GOLDEN, R.PARENT_STEP))
    got = R.seeded_step(DEV)
    assert sorted(got) == sorted(want.files)
    assert list(got["out_keys"]) == list(want["out_keys"])
    assert got["loss"].tobytes() == want["loss"].tobytes(), (got["loss"], want["loss"])
    diff = [k for k in want.files if k != "out_keys" and got[k].tobytes() != want[k].tobytes()]
    assert not diff, (len(diff), diff[:8])
    assert "vis_proj.weight" not in got and "contexts" not in got and len(got) > 150
