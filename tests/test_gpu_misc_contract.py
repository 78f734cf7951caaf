"""Every kernel of csrc/misc.hip behind the C ABI (im2col, token assembly, positional-embedding and
bilinear resize, transposes, the row mean, the pixel-text score map, score concatenation, casts,
BatchNorm; not dclip_weight_refresh, nor the fp16-scaling entry points: test_gpu_norm_contract.py
holds those to the same kind of contract) on
guard-banded, poisoned, strided buffers (abi_guard.py), every output against an fp64 reference per
element or bit for bit (misc_check.py: the cases, the references, the bounds and why they hold).

What test_gpu_kernels.py cannot see, going through ops.py and one norm over the whole tensor:
  * one wrong row, column or channel: every element has its own bound, none is excluded;
  * an output or workspace that already holds the answer: outputs and scratch enter as 0xFF, then
    as 0x3C (run_poisoned), must be finite and bitwise the same after both, workspaces have the
    size the library's query (or the header's formula) gives, never more;
  * reads past the last valid element: NaN follows every input's last element, fills the columns
    between its width and its leading dimension, the CLS rows of a token layout, the rows before
    r0 of a transpose and the pixels beyond im2col's floor grid;
  * writes outside the output: guard bands, and the gap columns of a strided output;
  * accumulating arguments (dpos, dcls, colsum, the accumulate = 1 output, the running statistics)
    that start from non-zero values;
  * dclip_bn_bwd on its own: it is fed the mean / rstd dclip_bn_fwd wrote, and the reference uses
    those same values.
The CPU emulation of the kernels goes through the same checker at the same cases in
test_misc_contract_emulation_cpu.py.  At the end the module prints, per entry point and dtype, the
worst figure over its cases as a fraction of its bound (bitwise outputs: the number of differing
elements, 0).

The kernels on the MI355X over all 234 cases (4.4 s), next to the f32 emulation, worst figure / bound
(fp16 | bf16 where both run); every bitwise output differs in 0 elements:
    entry point / output            kernels         emulation
    bilinear_fwd out  f32->f32      0.257           0.292
                      fp16->f32     0.266           0.303
                      bf16->bf16    0.992           0.992     (the output's own rounding)
    bilinear_bwd din  f32 | bf16    0.185 | 0.192   0.185 | 0.192
    pos_interp_fwd out              0.313           0.315
    pos_interp_bwd dpos             0.207           0.183
    score_concat score              0.992 | 0.995   0.992 | 0.995
    tokens_bwd dcls, dpos           0.366, 0.437    0.366, 0.437
    transpose colsum (inexact case) 0.024           0.010
    row_mean out                    0.006 | 0.006   0.006 | 0.006
    score_map score                 0.300 | 0.333   0.300 | 0.333
    bn_fwd mean                     0.224 | 0.225   0.224 | 0.225
           rstd                     0.230 | 0.230   0.175 | 0.175
           running mean, var        0.332, 0.215 | 0.270, 0.295      0.332, 0.380 | 0.270, 0.345
           y                        0.978 | 0.992   0.978 | 0.992
    bn_eval y                       0.999 | 0.996   0.999 | 0.996
    bn_bwd dw, db                   0.207, 0.006 | 0.225, 0.007      the same
           dx                       0.987 | 0.994   0.987 | 0.994
With row 0 six standard deviations out (700 x 64) the worst error of the mean is 5.5 x (fp16) / 5.7 x
(bf16) the centred case's and the worst relative error of rstd 27 x / 13 x, at 1.2e-5 and less: the
bound grows with Q / n + md^2 as the error does.
"""
import pytest
import torch

import misc_check as MC
from abi_guard import (GuardedMatrix, GuardedStrided, bits, guarded, guarded_copy, guarded_matrix_copy,
                       guarded_rows_copy, guarded_strided_copy, run_poisoned)
from misc_check import BF16, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}  # (family, dtypes) -> {output: worst figure / bound} over this session
# output name -> entry point, for the report
ENTRY = {"pos_interp": {"out[0]": "dclip_pos_interp_fwd", "out": "dclip_pos_interp_fwd", "dpos": "dclip_pos_interp_bwd"},
         "tokens": {"x": "dclip_tokens_fwd", "dpatch": "dclip_tokens_bwd", "dcls": "dclip_tokens_bwd",
                    "dpos": "dclip_tokens_bwd"},
         "bn": {"mean": "dclip_bn_fwd", "rstd": "dclip_bn_fwd", "rm": "dclip_bn_fwd", "rv": "dclip_bn_fwd",
                "y": "dclip_bn_fwd", "y_eval": "dclip_bn_eval", "dx": "dclip_bn_bwd", "dw": "dclip_bn_bwd",
                "db": "dclip_bn_bwd"}}
BN_ERR = {}  # (rows, C, dtype, outlier) -> (worst |mean - ref|, worst |rstd - ref| / rstd)


@pytest.fixture(autouse=True)
def _need(hip):
    pass


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (family, key), w in sorted(WORST.items()):
        by_entry = {}
        for name, v in sorted(w.items()):
            by_entry.setdefault(ENTRY.get(family, {}).get(name, "dclip_" + family), []).append(f"{name} {v:.3f}")
        for entry, figures in sorted(by_entry.items()):
            print(f"\nmisc contract {entry} {key}: worst figure / bound " + ", ".join(figures), end="")


def NT():
    from denseclip_vit_multimodal_amd import _native
    return _native


def code(dt):
    return {F16: NT().F16, BF16: NT().BF16, F32: NT().F32}[dt]


def stream():
    return torch.cuda.current_stream().cuda_stream


def gcopy(t):
    """a CPU tensor's values in a guarded device buffer; None stays None"""
    return None if t is None else guarded_copy(t.to(DEV))


def ptr(g):
    return None if g is None else g.ptr()


def scalar(v):
    return guarded_copy(torch.tensor([v], dtype=F32, device=DEV))


def accum(values):
    """a contiguous accumulating argument with non-zero entry values: (buffer, values) for run_poisoned's inout"""
    v = values.to(DEV).reshape(1, -1) if values.dim() == 1 else values.to(DEV)
    return GuardedMatrix(v.shape[0], v.shape[1], v.shape[1], v.dtype), v


def pixel_rows(x, token):
    """(B, rows, C) as strided pixel rows: a token buffer (row_off 1, ld C; the CLS rows hold NaN) or a
    channel slice (row_off 0, ld C + 8); returns (buffer, bstride, row_off, ld)"""
    ld, row_off = (x.shape[2], 1) if token else (x.shape[2] + 8, 0)
    g, bstride = guarded_rows_copy(x.to(DEV), ld, row_off)
    return g, bstride, row_off, ld


def check(family, c, inp, outs):
    outs = {k: v.cpu() for k, v in outs.items()}
    MC.check_case(family, c, inp, outs, WORST.setdefault((family, MC.dtype_key(c)), {}))
    return outs


def cases(family):
    cs = MC.FAMILIES[family][0]()
    return pytest.mark.parametrize("c", cs, ids=[MC.case_id(c) for c in cs])


# ----------------------------------------------------------------------------- resampling
@cases("bilinear_fwd")
def test_bilinear_fwd(c):
    """bilinear_fwd_kernel: 1024-column segments, 16-byte stores when Wo % 4 == 0, the clamped x of a ragged segment"""
    inp = MC.bilinear_fwd_inputs(c)
    (Hi, Wi), (Ho, Wo), NC = c["i"], c["o"], c["NC"]
    gx, out = gcopy(inp["x"]), guarded((NC, Ho, Wo), c["odt"])
    o, = run_poisoned(lambda: NT().call("dclip_bilinear_fwd", gx.ptr(), code(c["idt"]), out.ptr(), code(c["odt"]), NC,
                                        Hi, Wi, Ho, Wo, stream()), inputs=[gx], outputs=[out])
    check("bilinear_fwd", c, inp, {"out": o})


@cases("bilinear_bwd")
def test_bilinear_bwd(c):
    """bilinear_bwd_w_kernel + bilinear_bwd_h_kernel through the (NC, Ho, Wi) scratch the header names"""
    inp = MC.bilinear_bwd_inputs(c)
    (Hi, Wi), (Ho, Wo), NC = c["i"], c["o"], c["NC"]
    gd, din, ws = gcopy(inp["dout"]), guarded((NC, Hi, Wi), F32), guarded((NC, Ho, Wi), F32)
    o, = run_poisoned(lambda: NT().call("dclip_bilinear_bwd", gd.ptr(), code(c["gdt"]), din.ptr(), ws.ptr(), NC, Hi, Wi,
                                        Ho, Wo, stream()), inputs=[gd], outputs=[din], scratch=[ws])
    check("bilinear_bwd", c, inp, {"din": o})


@cases("pos_interp")
def test_pos_interp(c):
    """pos_interp_fwd_kernel and pos_interp_bwd_kernel (dpos += from non-zero values), g up- and downsampled"""
    inp = MC.pos_interp_inputs(c)
    g, C, H, W = c["g"], c["C"], c["H"], c["W"]
    gpos, out = gcopy(inp["pos"]), guarded((H * W + 1, C), F32)
    o, = run_poisoned(lambda: NT().call("dclip_pos_interp_fwd", gpos.ptr(), out.ptr(), g, C, H, W, stream()),
                      inputs=[gpos], outputs=[out])
    gd, (dpos, dpos0) = gcopy(inp["dout"]), accum(inp["dpos0"])
    d, = run_poisoned(lambda: NT().call("dclip_pos_interp_bwd", gd.ptr(), dpos.ptr(), g, C, H, W, stream()),
                      inputs=[gd], inout=[(dpos, dpos0)])
    check("pos_interp", c, inp, {"out": o, "dpos": d})


@cases("score_concat")
def test_score_concat(c):
    """score_concat_kernel: the C copied channels bit for bit, the K resized score channels to the bound"""
    inp = MC.score_concat_inputs(c)
    B, h, w, C, K = c["B"], c["h"], c["w"], c["C"], c["K"]
    rows, bstride, row_off, ld = pixel_rows(inp["rows"], c["token"])
    gs, out = gcopy(inp["score"]), guarded((B * h * w, C + K), c["dt"])
    o, = run_poisoned(lambda: NT().call("dclip_score_concat", rows.ptr(), code(c["dt"]), bstride, row_off, ld, C,
                                        gs.ptr(), K, c["hs"], c["ws"], out.ptr(), B, h, w, stream()),
                      inputs=[rows, gs], outputs=[out])
    check("score_concat", c, inp, {"out": o})


# ----------------------------------------------------------------------------- layout ops
@cases("im2col")
def test_im2col(c):
    """im2col_kernel (p % 4 == 0) and im2col_any_kernel: values and the zero padding K .. ldo - 1, bit for bit"""
    inp = MC.im2col_inputs(c)
    B, p = c["B"], c["p"]
    rows = B * (c["Hin"] // p) * (c["Win"] // p)
    gi, out = gcopy(inp["img"]), guarded((rows, c["ldo"]), c["odt"])
    o, = run_poisoned(lambda: NT().call("dclip_im2col", gi.ptr(), code(c["idt"]), out.ptr(), code(c["odt"]), c["ldo"], B,
                                        c["Cin"], c["Hin"], c["Win"], p, stream()), inputs=[gi], outputs=[out])
    check("im2col", c, inp, {"out": o})


@cases("tokens")
def test_tokens(c):
    """tokens_fwd_kernel bit for bit; tokens_bwd_kernel: dpatch bit for bit (host scale times a device
    scale), dcls / dpos accumulated onto non-zero values, each of the three null in one case"""
    inp = MC.tokens_inputs(c)
    B, Pn, C, dt = c["B"], c["P"], c["C"], c["dt"]
    gp, gc, gpos, x = gcopy(inp["patch"]), gcopy(inp["cls"]), gcopy(inp["pos"]), guarded((B * (Pn + 1), C), F32)
    xo, = run_poisoned(lambda: NT().call("dclip_tokens_fwd", gp.ptr(), code(dt), gc.ptr(), gpos.ptr(), x.ptr(), B, Pn, C,
                                         stream()), inputs=[gp, gc, gpos], outputs=[x])
    gdx = gcopy(inp["dx"])
    dpatch = None if c["null"] == "dpatch" else guarded((B * Pn, C), dt)
    dcls = None if c["null"] == "dcls" else accum(inp["dcls0"])
    dpos = None if c["null"] == "dpos" else accum(inp["dpos0"])
    sp = scalar(MC.TOKENS_SCALE_PTR) if c["ptr"] else None
    inout = [a for a in (dcls, dpos) if a is not None]
    res = run_poisoned(lambda: NT().call("dclip_tokens_bwd", gdx.ptr(), ptr(dpatch), code(dt), MC.TOKENS_SCALE, ptr(sp),
                                         ptr(dcls and dcls[0]), ptr(dpos and dpos[0]), B, Pn, C, stream()),
                       inputs=[gdx] + ([sp] if sp else []), outputs=[dpatch] if dpatch else [], inout=inout)
    names = (["dpatch"] if dpatch else []) + (["dcls"] if dcls else []) + (["dpos"] if dpos else [])
    outs = dict(zip(names, res), x=xo)
    if "dcls" in outs:
        outs["dcls"] = outs["dcls"][0]
    check("tokens", c, inp, outs)


@cases("transpose")
def test_transpose(c):
    """transpose_kernel (batches, r0, rows_pad, accumulate, colsum) and transpose_f32_fast_kernel on
    strided inputs and outputs.  The last case is the fast kernel's (64, 128) with out_ld % 8 != 0: it
    takes the generic kernel and is held to the same bits."""
    inp = MC.transpose_inputs(c)
    rows, cols, rows_pad, r0, batch = c["rows"], c["cols"], c["rows_pad"], c["r0"], c["batch"]
    in_ld, out_ld = c["in_ld"], c["out_ld"]
    in_bs, out_bs = (r0 + rows) * in_ld + c["bgap"], cols * out_ld + c["bgap"]
    full = torch.cat([torch.full((batch, r0, cols), float("nan")).to(c["idt"]), inp["in"]], 1)  # NaN before r0
    gi = guarded_strided_copy(full.to(DEV), (in_bs, in_ld, 1))
    out = GuardedStrided((batch, cols, rows_pad), (out_bs, out_ld, 1), c["odt"])
    cs = accum(inp["colsum0"]) if c["colsum"] else None
    # the condition under which dclip_transpose takes transpose_f32_fast_kernel (misc.hip)
    fast = (not c["acc"] and cs is None and batch == 1 and r0 == 0 and c["idt"] == F32 and c["odt"] in (F16, BF16)
            and rows == rows_pad and rows % 64 == 0 and cols % 64 == 0 and in_ld % 4 == 0 and out_ld % 8 == 0
            and (gi.ptr() | out.ptr()) % 16 == 0)
    assert fast == c["fast"], "the case does not take the kernel it is meant for"
    inout = ([(out, inp["out0"].to(DEV))] if c["acc"] else []) + ([cs] if cs else [])
    res = run_poisoned(lambda: NT().call("dclip_transpose", gi.ptr(), code(c["idt"]), in_bs, in_ld, r0, out.ptr(),
                                         code(c["odt"]), out_bs, out_ld, batch, rows, rows_pad, cols, c["acc"],
                                         ptr(cs and cs[0]), stream()),
                       inputs=[gi], outputs=[] if c["acc"] else [out], inout=inout)
    outs = {"out": res[0]}
    if cs:
        outs["colsum"] = res[-1][0]
    check("transpose", c, inp, outs)


@cases("cast")
def test_cast(c):
    """cast_kernel: 4 elements per thread and the scalar tail, bit for bit (misc_check.CAST_SECOND_PASS_N
    says why no case reaches a second pass of the grid-stride loop)"""
    inp = MC.cast_inputs(c)
    s, sp = MC.cast_scale(c)
    gi, out, gsp = gcopy(inp["in"]), guarded(c["n"], c["odt"]), (scalar(sp) if sp is not None else None)
    o, = run_poisoned(lambda: NT().call("dclip_cast", gi.ptr(), code(c["idt"]), out.ptr(), code(c["odt"]), c["n"], s,
                                        ptr(gsp), stream()), inputs=[gi] + ([gsp] if gsp else []), outputs=[out])
    check("cast", c, inp, {"out": o})


# ----------------------------------------------------------------------------- reductions
@cases("row_mean")
def test_row_mean(c):
    """row_mean_part_kernel (8 predicated loads in flight, 256 / (C / 8) row phases, idle threads) +
    row_mean_final_kernel, the workspace at the size dclip_row_mean_workspace gives"""
    inp = MC.row_mean_inputs(c)
    B, rows, C = c["B"], c["rows"], c["C"]
    x, bstride, row_off, ld = pixel_rows(inp["x"], c["token"])
    ws = guarded(int(NT().lib().dclip_row_mean_workspace(B, rows, C)), F32)
    out = guarded((B, C), F32)
    o, = run_poisoned(lambda: NT().call("dclip_row_mean", x.ptr(), code(c["dt"]), bstride, row_off, ld, B, rows, C,
                                        ws.ptr(), out.ptr(), stream()), inputs=[x], outputs=[out], scratch=[ws])
    check("row_mean", c, inp, {"out": o})


@cases("score_map")
def test_score_map(c):
    """score_map_kernel: 1 to 128 MFMA steps over 4 waves, ragged 32-pixel groups, K < 32, an all-zero
    pixel row and class row (exactly 0)"""
    inp = MC.score_map_inputs(c)
    B, HW, C, K = c["B"], c["HW"], c["C"], c["K"]
    v, bstride, row_off, ld = pixel_rows(inp["v"], c["token"])
    gt, score = gcopy(inp["t"]), guarded((B, K, HW), F32)
    o, = run_poisoned(lambda: NT().call("dclip_score_map", v.ptr(), code(c["dt"]), bstride, row_off, ld, gt.ptr(),
                                        score.ptr(), B, HW, C, K, MC.SCORE_EPS, stream()),
                      inputs=[v, gt], outputs=[score])
    check("score_map", c, inp, {"score": o})


# ----------------------------------------------------------------------------- batch norm
@cases("bn")
def test_bn(c):
    """dclip_bn_fwd (statistics per channel, running statistics from non-trivial values, y per
    element), dclip_bn_eval, and dclip_bn_bwd from the mean / rstd the forward wrote (dw / db per
    channel, dx per element, the ReLU mask asserted unambiguous, *gscale = 2^-13 exactly)"""
    inp = MC.bn_inputs(c)
    rows, C, ld, dt, relu = c["rows"], c["C"], c["ld"], c["dt"], c["relu"]
    nws = int(NT().lib().dclip_bn_workspace(rows, C))
    assert nws == 512 * 2 * C + 5 * C  # the header's formula
    gx, gdy = guarded_matrix_copy(inp["x"].to(DEV), ld), guarded_matrix_copy(inp["dy"].to(DEV), ld)
    gw, gb = gcopy(inp["w"]), gcopy(inp["b"])
    ws, mean, rstd = guarded(nws, F32), guarded(C, F32), guarded(C, F32)
    y = GuardedMatrix(rows, C, ld, dt)
    run = [] if c["null"] else [accum(inp["rm0"]), accum(inp["rv0"])]
    res = run_poisoned(lambda: NT().call("dclip_bn_fwd", code(dt), gx.ptr(), rows, C, ld, ptr(gw), ptr(gb), MC.BN_EPS,
                                         MC.BN_MOMENTUM, ptr(run[0][0] if run else None), ptr(run[1][0] if run else None), ws.ptr(),
                                         mean.ptr(), rstd.ptr(), y.ptr(), relu, stream()),
                       inputs=[g for g in (gx, gw, gb) if g], outputs=[mean, rstd, y], scratch=[ws], inout=run)
    outs = dict(zip(["mean", "rstd", "y"], res))
    if run:
        outs["rm"], outs["rv"] = res[3][0], res[4][0]

    erm, erv, ye = gcopy(inp["erm"]), gcopy(inp["erv"]), GuardedMatrix(rows, C, ld, dt)
    outs["y_eval"], = run_poisoned(lambda: NT().call("dclip_bn_eval", code(dt), gx.ptr(), rows, C, ld, ptr(gw), ptr(gb),
                                                     MC.BN_EPS, erm.ptr(), erv.ptr(), ws.ptr(), ye.ptr(), relu, stream()),
                                   inputs=[g for g in (gx, gw, gb, erm, erv) if g], outputs=[ye], scratch=[ws])

    gmean, grstd = guarded_copy(outs["mean"]), guarded_copy(outs["rstd"])
    dx = GuardedMatrix(rows, C, ld, dt)
    dw, db = (None, None) if c["null"] else (guarded(C, F32), guarded(C, F32))
    gs = scalar(MC.BN_GSCALE) if relu else None

    def bwd(dw, db, gs):
        return lambda: NT().call("dclip_bn_bwd", code(dt), gdy.ptr(), gx.ptr(), rows, C, ld, ptr(gw), ptr(gb),
                                 gmean.ptr(), grstd.ptr(), ws.ptr(), dx.ptr(), ptr(dw), ptr(db), relu, ptr(gs), stream())

    res = run_poisoned(bwd(dw, db, gs), inputs=[g for g in (gdy, gx, gw, gb, gmean, grstd, gs) if g],
                       outputs=[dx] + ([dw, db] if dw else []), scratch=[ws])
    outs["dx"] = res[0]
    if dw:
        outs["dw"], outs["db"] = res[1], res[2]
    if gs and dw:  # a power-of-two *gscale is exact: the unscaled gradients times 2^-13, bit for bit
        dw1, db1 = guarded(C, F32), guarded(C, F32)
        r1 = run_poisoned(bwd(dw1, db1, None), outputs=[dx, dw1, db1], scratch=[ws])
        assert torch.equal(bits(r1[1] * MC.BN_GSCALE), bits(outs["dw"])), "dw is not exactly *gscale times the unscaled dw"
        assert torch.equal(bits(r1[2] * MC.BN_GSCALE), bits(outs["db"])), "db is not exactly *gscale times the unscaled db"
        assert torch.equal(bits(r1[0]), bits(outs["dx"])), "dx depends on *gscale"
    outs = check("bn", c, inp, outs)

    # by how much the statistics' error grows when row 0, the shift of the sums, is an outlier
    if rows != 700 or relu:
        return
    items = {n: r for n, r, _ in MC.bn_refs(c, inp, outs) if n in ("mean", "rstd")}
    err = (float((outs["mean"].double() - items["mean"]).abs().max()),
           float(((outs["rstd"].double() - items["rstd"]).abs() / items["rstd"]).max()))
    BN_ERR[rows, C, dt, c["outlier"]] = err
    centred = BN_ERR.get((rows, C, dt, False))
    if c["outlier"] and centred:
        print(f"bn {rows} x {C} {MC.NAME[dt]}, row 0 six standard deviations out: worst |mean - ref| {err[0]:.2e} "
              f"({err[0] / max(centred[0], 1e-300):.1f} x the centred case's), worst relative rstd error {err[1]:.2e} "
              f"({err[1] / max(centred[1], 1e-300):.1f} x)")
