"""The other family of gemm.hip through the C ABI on guard-banded, poisoned, STRIDED buffers
(abi_guard.py): dclip_conv3x3 (conv_nt_kernel, forward and input gradient), dclip_conv3x3_wgrad
(conv_wgrad_kernel and its two combines) and dclip_gemm_tn's SPLITK (the weight-gradient kernels),
every output against an fp64 reference per 32 x 64 block and per element (conv_check.py: the
references as matrix products; gemm_check.py: the bounds and why they hold — nothing is added to them).

What the op-layer tests of test_gpu_kernels.py / test_gpu_torch_ops.py cannot see:
  * outputs that do not already hold the answer: every output and workspace enters as 0xFF, then as
    0x3C (run_poisoned), the weight gradient's workspace is exactly splits * Nout * 9 Cin floats;
  * out-of-image taps that leak: the input's pixels are written through a strided view into a
    buffer of 0xFF, so the CLS row a y = -1 tap would wrongly read, the columns between Cin and x_ld,
    whatever lies before the first pixel and behind the last are NaN, in three layouts: contiguous,
    a token buffer (bstride (1 + H W) ld, off ld) and a channel slice (ld = C + 64, off 64);
  * the edges of the 256-pixel x 128-column tile with 64-channel K-steps (conv_check.GEOMETRIES;
    Nout 8, 72, 128, 136; Cin 64, 128, 192), accumulate = 1, an f32 output, out_ld = Nout + 8 (the gap
    columns come back bit for bit) and the mapped output (out_gap 1, out_off 1) into a token-shaped
    buffer whose row 0 of every image comes back bit for bit, in both poison runs;
  * the weight gradient's pixel splits, one of them empty (3 splits at 80 pixels: 64 + 16 + 0), both
    output layouts, *alpha_ptr, ldy = Nout + 8 and the builtin-staging variant (DCLIP_OPT_GEMM_TN_TILE 5);
    where every tap of a column block is out of the image the reference block is exactly zero and
    the blocked check demands exact zeros;
  * dclip_gemm_tn SPLITK on lda = M + 8, ldb = N + 16, ldc = N + 8 per block and per element, with
    DCLIP_OPT_GEMM_TN_TILE 0 - 5, DCLIP_OPT_GEMM_KLOOP 1, a ragged K (24, 70, 200), splits 1 - 3 (K = 24
    or 70 with 3 splits: splits that hold no row), the combine's bias, alpha * *alpha_ptr, and colsum_a
    on the 256 x 256 and on the small-tile path, held to
        |cs - ref| <= 2^-24 |ref| + (K + 4) 2^-24 |alpha| sum_k |A|
    and to bitwise equality between run_poisoned's two runs (it is summed in a fixed order on every
    path: colsum_kernel reduces in LDS and the combine adds the per-split partials in split order).

conv_nt_kernel's pointer staging (an input extent of 2^32 - 4096 bytes or more, which no workload shape
reaches) runs once per mode, on two images 2^31 elements apart.

The CPU emulation of the kernels (test_conv_contract_emulation_cpu.py) through the same checker, and
the kernels on the MI355X over all rows of this file (worst figure / bound, fp16 | bf16 operands):
    form               emulation blk    emulation el     kernels blk      kernels el
    conv store16       0.109 | 0.146    0.772 | 0.943    0.120 | 0.156    0.725 | 0.931
    conv store32       0.062 | 0.027    0.007 | 0.003    0.022 | 0.020    0.003 | 0.002
    conv resid         0.043 | 0.019    0.007 | 0.003    0.019 | 0.018    0.003 | 0.002
    conv store16, pointer staging (bf16 only)                  - | 0.143        - | 0.936
    wgrad              0.031 | 0.013    0.047 | 0.022    0.012 | 0.010    0.016 | 0.014
    wgrad, OIHW        0.030 | 0.012    0.047 | 0.022    0.009 | 0.008    0.019 | 0.018
    gemm_tn SPLITK                                       0.010 | 0.008    0.277 | 0.261
    gemm_tn STORE, tiles 2 and 3                         0.006 | 0.005    0.019 | 0.018
    gemm_tn colsum_a                                                      0.013 | 0.009
(a 16-bit output rounded by half an ulp just above a power of two is at 2^-p |ref| by itself; the
f32 outputs are far from their bounds; SPLITK's elementwise figure is set by K = 24, where the
bound's accumulation term is smallest.)

What this file found: with DCLIP_OPT_GEMM_TN_TILE 2 or 3 on the 256 x 256 path and colsum_a given,
dclip_gemm_tn took the sums for fused, but those two kernel variants have none: SPLITK's combine
then read per-split partials nobody had written (test_gemm_tn_splitk_strided[*-tile2-*] and
[*-tile3-*] with colsum_a: 256 non-finite values after the 0xFF run) and STORE left colsum_a
untouched.  They take the separate pass now.
"""
import pytest
import torch

import conv_check as CC
import gemm_check as GC
from abi_guard import (FINITE, POISON, Guarded, GuardedMatrix, bits, guarded, guarded_copy, guarded_matrix,
                       guarded_matrix_copy, option_scope, run_poisoned)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
F32 = torch.float32
WORST = {}  # (form, dtype) -> {(output, check): worst figure / bound} over this session
GEO = dict(zip("ABCDE", CC.GEOMETRIES))  # A 2x9x17, B 3x5x7, C 2x1x40, D 2x40x1, E 1x1x1


@pytest.fixture(autouse=True)
def _need(hip):
    pass


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (form, dt), w in sorted(WORST.items(), key=str):
        print(f"\nconv contract {form} {dt}: worst figure / bound "
              + ", ".join(f"{n} {c} {v:.3f}" for (n, c), v in sorted(w.items())), end="")


def NT():
    from denseclip_vit_multimodal_amd import _native
    return _native


def code(dt):
    return {torch.float16: NT().F16, torch.bfloat16: NT().BF16, torch.float32: NT().F32}[dt]


def stream():
    return torch.cuda.current_stream().cuda_stream


def dt_id(dt):
    return DT_IDS[DTS.index(dt)]


# ----------------------------------------------------------------------------- buffers
def pixel_buffer(x, layout):
    """The pixels x (B, H, W, C) written through a strided view into a guarded buffer of 0xFF that
    ends at the last pixel's last channel; returns (buffer, x_bstride, x_off, x_ld) in elements."""
    B, H, W, C = x.shape
    HW = H * W
    if layout == "contiguous":
        ld, off, bstride = C, 0, HW * C
    elif layout == "token":  # a ViT token buffer: row 0 of every image is the CLS row
        ld, off = C, C
        bstride = (1 + HW) * ld
    elif layout == "slice":  # channels [64, 64 + C) of a wider channels-last buffer
        ld, off = C + 64, 64
        bstride = HW * ld
    else:
        raise KeyError(layout)
    g = Guarded((B - 1) * bstride + off + (HW - 1) * ld + C, x.dtype, POISON)
    g.t.as_strided((B, HW, C), (bstride, ld, 1), g.t.storage_offset() + off).copy_(x.reshape(B, HW, C))
    return g, bstride, off, ld


class MappedOutput(GuardedMatrix):
    """A token-shaped output (B * (1 + HW) rows of `cols`, pitch `ld`) that dclip_conv3x3 writes with
    out_gap 1, out_off 1: `m` is the B x HW x cols view of the rows it maps, and `gap` everything else
    of the payload — the columns between cols and ld and row 0 of every image — which run_poisoned
    demands back bit for bit after both runs."""

    def __init__(self, B, HW, cols, ld, dtype, fill=0):
        super().__init__(B * (1 + HW), cols, ld, dtype, fill)  # sets gap (through the setter) to the gap columns
        self.m = self.t.as_strided((B, HW, cols), ((1 + HW) * ld, ld, 1), self.t.storage_offset() + ld)
        self.row0 = self.t.as_strided((B, cols), ((1 + HW) * ld, 1), self.t.storage_offset())

    @property
    def gap(self):  # a fresh tensor on every access
        return torch.cat([self._gapcols.reshape(-1), self.row0.reshape(-1)])

    @gap.setter
    def gap(self, v):
        self._gapcols = v


# ----------------------------------------------------------------------------- dclip_conv3x3
# (geometry, input layout, Cin, Nout, form, out_ld - Nout, mapped output); mode and dtype are parametrised
# on top, so each value of each axis meets both modes and both dtypes
CONV_ROWS = [
    ("A", "contiguous", 64, 136, "store16", 0, False),
    ("A", "token", 128, 72, "store32", 8, True),
    ("A", "slice", 192, 128, "resid", 8, False),
    ("A", "token", 64, 8, "resid", 0, True),
    ("A", "slice", 128, 136, "store16", 8, True),
    ("B", "token", 192, 72, "store16", 8, True),
    ("B", "slice", 64, 136, "store32", 0, False),
    ("B", "contiguous", 128, 8, "resid", 8, False),
    ("C", "slice", 128, 136, "store16", 8, False),
    ("C", "token", 64, 128, "store32", 0, True),
    ("C", "contiguous", 192, 72, "resid", 0, False),
    ("D", "token", 128, 128, "store16", 0, True),
    ("D", "contiguous", 192, 8, "store32", 8, False),
    ("D", "slice", 64, 72, "resid", 8, True),
    ("E", "token", 64, 8, "store16", 8, True),
    ("E", "contiguous", 128, 136, "store32", 0, False),
    ("E", "slice", 192, 72, "resid", 0, False),
]


def test_conv_rows_cover_every_axis():
    for i, values in enumerate([set("ABCDE"), {"contiguous", "token", "slice"}, {64, 128, 192}, {8, 72, 128, 136},
                                {"store16", "store32", "resid"}, {0, 8}, {False, True}]):
        assert {r[i] for r in CONV_ROWS} == values, i


@pytest.mark.parametrize("row", CONV_ROWS, ids=["-".join(str(v) for v in r) for r in CONV_ROWS])
@pytest.mark.parametrize("mode", [0, 1], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_conv3x3(dt, mode, row):
    """conv_nt_kernel: mode 0 with Wt[co][tap * Cin + ci], mode 1 with X = dOut and Wd[ci][tap * Cout +
    co] (the kernel's Cin is then Cout and its Nout the true Cin): out = conv_cols(X, +-1) @ W^T"""
    geo, layout, Cin, Nout, form, ldgap, mapped = row
    L = NT()
    B, H, W = GEO[geo]
    HW, M = H * W, B * H * W
    o = CC.operands(B, H, W, Cin, Nout, dt, 1000 * mode + CONV_ROWS.index(row), DEV)
    gx, bstride, off, ld = pixel_buffer(o["X"], layout)
    gw = guarded_copy(o["Wm"])
    out_dt = dt if form == "store16" else F32
    out_ld = Nout + ldgap
    fill = POISON if form == "resid" else 0
    gout = (MappedOutput(B, HW, Nout, out_ld, out_dt, fill) if mapped
            else guarded_matrix(M, Nout, out_ld, out_dt, fill))
    untouched = []  # per run: row 0 of every image of a mapped output still holds what it entered with

    def fn():
        entry = bits(gout.row0.clone()) if mapped else None  # a copy: contiguous() of one row would alias it
        L.call("dclip_conv3x3", mode, code(dt), gx.ptr(), bstride, off, ld, B, H, W, Cin, gw.ptr(), Nout, gout.ptr(),
               code(out_dt), out_ld, 1 if mapped else 0, 1 if mapped else 0, 1 if form == "resid" else 0, stream())
        if mapped:
            untouched.append((bits(gout.row0) == entry).all())

    if form == "resid":  # the prior contents: read and overwritten in place (aux == out)
        res = o["res"].view(B, HW, Nout) if mapped else o["res"]
        y = run_poisoned(fn, inputs=[gx, gw], inout=[(gout, res)])[0]
    else:
        y = run_poisoned(fn, inputs=[gx, gw], outputs=[gout])[0]
    if mapped:
        assert len(untouched) == 2
        for ok, byte in zip(untouched, (POISON, FINITE)):
            assert bool(ok), f"row 0 of an image of the mapped output was written (0x{byte:02X} run)"
        if form != "resid":  # after the second run those rows hold its fill, byte for byte
            assert bool((gout.row0.contiguous().view(torch.uint8) == FINITE).all())
    acc, absacc = CC.conv_ref(o["X"], o["Wm"], 1 if mode == 0 else -1)
    refs = GC.references(form, dt, 9 * Cin, acc, absacc, 1.0, res=o["res"])
    what = (f"conv3x3 mode {mode} {dt_id(dt)} {B}x{H}x{W} {layout} Cin={Cin} Nout={Nout} {form} out_ld={out_ld}"
            + (" mapped" if mapped else ""))
    GC.check(what, refs, {"C": y.reshape(M, Nout)}, WORST.setdefault(("conv " + form, dt_id(dt)), {}))


# ----------------------------------------------------------------------------- dclip_conv3x3_wgrad
# (geometry, input layout, Cin, Nout, splits, oihw, alpha_ptr, DCLIP_OPT_GEMM_TN_TILE)
WGRAD_ROWS = [
    ("A", "contiguous", 128, 136, 1, 0, False, 0),
    ("A", "token", 256, 72, 2, 1, True, 0),
    ("A", "slice", 128, 8, 4, 1, False, 0),
    ("A", "token", 128, 72, 4, 0, False, 0),
    ("A", "contiguous", 256, 136, 2, 1, True, 0),
    ("A", "token", 128, 136, 2, 0, False, 5),
    ("C", "token", 128, 136, 3, 1, True, 0),
    ("C", "slice", 256, 8, 3, 0, False, 0),
    ("D", "token", 256, 72, 3, 0, False, 0),
    ("D", "contiguous", 128, 136, 3, 1, False, 0),
    ("B", "slice", 128, 72, 2, 0, False, 0),
    ("B", "token", 256, 8, 1, 1, True, 0),
    ("E", "token", 128, 8, 2, 1, False, 0),
    ("E", "contiguous", 256, 136, 1, 0, False, 0),
]


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=["-".join(str(v) for v in r) for r in WGRAD_ROWS])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_conv3x3_wgrad(dt, row):
    """conv_wgrad_kernel's per-split slabs in a poisoned workspace of exactly splits * Nout * 9 Cin
    floats, then splitk_reduce_kernel (oihw 0) or conv_wgrad_reduce_oihw_kernel (oihw 1, times
    *alpha_ptr = 2^-9): dW = dY^T conv_cols(X, +1).  With 3 splits at 80 pixels the third holds no
    pixel and its slab must still be written (zeros)."""
    geo, layout, Cin, Nout, splits, oihw, scaled, tile = row
    L = NT()
    B, H, W = GEO[geo]
    Kpix, N = B * H * W, 9 * Cin
    if splits == 3 and Kpix == 80:
        kp = (Kpix + 64 * splits - 1) // (64 * splits) * 64
        assert kp == 64 and 2 * kp >= Kpix  # the pixel rows per split of dclip_conv3x3_wgrad: the last split is empty
    o = CC.operands(B, H, W, Cin, Nout, dt, 5000 + WGRAD_ROWS.index(row), DEV)
    gx, bstride, off, ld = pixel_buffer(o["X"], layout)
    gdy = guarded_matrix_copy(o["dY"], Nout + 8)
    alpha = 2.0 ** -9 if scaled else 1.0
    galpha = guarded_copy(torch.tensor([alpha], device=DEV))
    gdw = guarded((Nout, N), F32)
    ws = guarded(splits * Nout * N, F32)

    def fn():
        L.call("dclip_conv3x3_wgrad", code(dt), gdy.ptr(), Nout + 8, Nout, gx.ptr(), bstride, off, ld, B, H, W, Cin,
               gdw.ptr(), ws.ptr(), splits, oihw, galpha.ptr() if scaled else None, stream())

    with option_scope() as set_option:
        if tile:
            set_option(L.OPT_GEMM_TN_TILE, tile)
        y = run_poisoned(fn, inputs=[gx, gdy, galpha], outputs=[gdw], scratch=[ws])[0]
    acc, absacc = CC.wgrad_ref(o["dY"], o["X"], bool(oihw))
    if geo in "CD":  # six of the nine taps never meet the image: whole column blocks of exact zeros
        assert int((acc == 0).all(0).sum()) == 6 * Cin
    refs = GC.references("store32", dt, Kpix, acc, absacc, alpha)
    what = (f"conv3x3_wgrad {dt_id(dt)} {B}x{H}x{W} {layout} Cin={Cin} Nout={Nout} splits {splits} oihw {oihw} "
            f"alpha {alpha} tile {tile}")
    GC.check(what, refs, {"C": y}, WORST.setdefault(("wgrad oihw" if oihw else "wgrad", dt_id(dt)), {}))


# ----------------------------------------------------------------------------- dclip_gemm_tn, SPLITK
_TN = {}


def tn_operands(M, N, K, dt):
    """A (K, M), B (K, N) on lda = M + 8, ldb = N + 16 in guarded buffers, the side inputs and the fp64
    products: computed once per (M, N, K, dtype), read-only"""
    key = (M, N, K, dt)
    if key not in _TN:
        g = torch.Generator(device=DEV).manual_seed(13 * M + 7 * N + K)
        A = torch.randn(K, M, device=DEV, generator=g).to(dt)
        Bm = (torch.randn(K, N, device=DEV, generator=g) * K ** -0.5).to(dt)
        bias = torch.randn(N, device=DEV, generator=g)
        A64, B64 = A.double(), Bm.double()
        _TN[key] = {"gA": guarded_matrix_copy(A, M + 8), "gB": guarded_matrix_copy(Bm, N + 16), "bias": bias,
                    "gbias": guarded_copy(bias), "galpha": guarded_copy(torch.tensor([0.25], device=DEV)),
                    "acc": A64.t() @ B64, "absacc": A64.abs().t() @ B64.abs(), "colsum": A64.sum(0),
                    "abscolsum": A64.abs().sum(0)}
    return _TN[key]


def colsum_figure(what, cs, t, alpha, K, dt):
    """worst |cs - ref| / (2^-24 |ref| + (K + 4) 2^-24 |alpha| sum_k |A|) of colsum_a, printed and recorded"""
    ref = alpha * t["colsum"]
    bound = GC.U32 * ref.abs() + (K + 4) * GC.U32 * abs(alpha) * t["abscolsum"]
    figure = float(((cs.double() - ref).abs() / bound.clamp(min=1e-300)).max())
    print(f"{what} colsum_a: worst |cs - ref| / bound {figure:.3f}")
    w = WORST.setdefault(("gemm_tn colsum", dt_id(dt)), {})
    w["cs", "element"] = max(w.get(("cs", "element"), 0.0), figure)
    return figure


# option rows: (DCLIP_OPT_GEMM_TN_TILE, DCLIP_OPT_GEMM_KLOOP)
TN_BIG_ROWS = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (0, 1)]
TN_CASES = ([(M, N, t, kl) for (M, N) in [(256, 264), (264, 256)] for (t, kl) in TN_BIG_ROWS]
            + [(136, 72, 1, 0)])


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("K", [24, 70, 200])
@pytest.mark.parametrize("M,N,tile,kloop", TN_CASES,
                         ids=[f"{M}x{N}-tile{t}" + ("-kloop1" if kl else "") for M, N, t, kl in TN_CASES])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_gemm_tn_splitk_strided(dt, M, N, tile, kloop, K, splits):
    """C = alpha A^T B (+ bias) through the per-split slabs of a poisoned workspace of exactly
    splits * (M N + M) floats and the combine, into ldc = N + 8; K is no multiple of 64, K_pad is K
    rounded up to 64 * splits (K = 24 with 2 or 3 splits, 70 with 3: splits without a row).  The bias
    in half of the rows, alpha = 0.5 with *alpha_ptr = 0.25 in half, colsum_a in two of three."""
    L = NT()
    t = tn_operands(M, N, K, dt)
    ti, ki = TN_CASES.index((M, N, tile, kloop)), [24, 70, 200].index(K)
    idx = 9 * ti + 3 * ki + splits - 1
    # per option row and split count: colsum_a at two of the three K, null at the third
    with_bias, scaled, with_cs = bool(idx & 1), bool(idx & 2), (ti + ki + splits) % 3 != 0
    alpha = 0.125 if scaled else 1.0
    k_pad = (K + 64 * splits - 1) // (64 * splits) * 64 * splits
    out = guarded_matrix(M, N, N + 8, F32)
    ws = guarded(splits * (M * N + M), F32)
    cs = [guarded(M, F32)] if with_cs else []

    def fn():
        L.call("dclip_gemm_tn", L.EPI_SPLITK, code(dt), t["gA"].ptr(), M + 8, t["gB"].ptr(), N + 16, M, N, K, k_pad,
               splits, 0.5 if scaled else 1.0, t["galpha"].ptr() if scaled else None,
               t["gbias"].ptr() if with_bias else None, ws.ptr(), out.ptr(), N + 8, cs[0].ptr() if with_cs else None,
               stream())

    with option_scope() as set_option:
        set_option(L.OPT_GEMM_TN_TILE, tile)
        if kloop:
            set_option(L.OPT_GEMM_KLOOP, kloop)
        # run_poisoned: colsum_a (accumulated, so zeroed before each run) bitwise equal between the runs
        res = run_poisoned(fn, inputs=[t["gA"], t["gB"], t["gbias"], t["galpha"]], outputs=[out], scratch=[ws],
                           accum=cs)
    what = (f"gemm_tn SPLITK {dt_id(dt)} M={M} N={N} K={K} splits {splits} tile {tile} kloop {kloop} alpha {alpha} "
            f"bias {'set' if with_bias else 'null'}")
    figure = colsum_figure(what, res[1], t, alpha, K, dt) if with_cs else 0.0  # printed before anything is asserted
    refs = GC.references("splitk", dt, K, t["acc"], t["absacc"], alpha, t["bias"] if with_bias else None)
    GC.check(what, refs, {"C": res[0]}, WORST.setdefault(("gemm_tn splitk", dt_id(dt)), {}))
    assert figure <= 1.0, (what, "colsum_a", figure)


@pytest.mark.parametrize("tile", [2, 3])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_gemm_tn_store_colsum_without_fused_sums(dt, tile):
    """The STORE epilogue on the 32-row K-step variants of the 256 x 256 kernel, which have no fused
    column sums: colsum_a must come from the separate pass (it was left untouched)"""
    L = NT()
    M, N, K = 256, 264, 70
    t = tn_operands(M, N, K, dt)
    out = guarded_matrix(M, N, N + 8, F32)
    cs = guarded(M, F32)

    def fn():
        L.call("dclip_gemm_tn", L.EPI_STORE, code(dt), t["gA"].ptr(), M + 8, t["gB"].ptr(), N + 16, M, N, K, 128, 1,
               0.5, t["galpha"].ptr(), None, None, out.ptr(), N + 8, cs.ptr(), stream())

    with option_scope() as set_option:
        set_option(L.OPT_GEMM_TN_TILE, tile)
        res = run_poisoned(fn, inputs=[t["gA"], t["gB"], t["galpha"]], outputs=[out], accum=[cs])
    what = f"gemm_tn STORE {dt_id(dt)} M={M} N={N} K={K} tile {tile} alpha 0.125"
    figure = colsum_figure(what, res[1], t, 0.125, K, dt)
    refs = GC.references("store32", dt, K, t["acc"], t["absacc"], 0.125)
    GC.check(what, refs, {"C": res[0]}, WORST.setdefault(("gemm_tn store", dt_id(dt)), {}))
    assert figure <= 1.0, (what, "colsum_a", figure)


# ----------------------------------------------------------------------------- conv_nt_kernel, pointer staging
@pytest.mark.parametrize("mode", [0, 1], ids=["fwd", "dgrad"])
def test_conv3x3_pointer_staging(mode):
    """dclip_conv3x3 stages the input with buffer loads while its extent stays below 2^32 - 4096
    bytes, and with per-lane pointers and the zero row beyond (no workload shape does that).  Two
    images 2^31 elements apart in one allocation reach it; only the images (token layout: a CLS row
    in front) and 1 MiB of 0xFF around each are ever written or read."""
    L = NT()
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip("less than 16 GiB of device memory free")
    dt, (B, H, W), Cin, Nout = torch.bfloat16, GEO["A"], 64, 72
    HW, M, ld, off, bstride = H * W, B * H * W, Cin, Cin, 1 << 31
    assert ((B - 1) * bstride + off + HW * ld) * 2 >= (1 << 32) - 4096  # dclip_conv3x3's switch
    o = CC.operands(B, H, W, Cin, Nout, dt, 9000 + mode, DEV)
    band = 1 << 20
    raw = torch.empty(band + ((B - 1) * bstride + off + HW * ld) * 2 + band, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    for b in range(B):
        lo = band + b * bstride * 2  # byte offset of image b's CLS row
        raw[lo - band:lo + (off + HW * ld) * 2 + band] = POISON
        raw[lo + off * 2:lo + (off + HW * ld) * 2].view(dt).view(HW, ld).copy_(o["X"][b].reshape(HW, Cin))
    gw = guarded_copy(o["Wm"])
    gout = guarded_matrix(M, Nout, Nout + 8, dt)
    y = run_poisoned(lambda: L.call("dclip_conv3x3", mode, code(dt), raw.data_ptr() + band, bstride, off, ld, B, H, W,
                                    Cin, gw.ptr(), Nout, gout.ptr(), code(dt), Nout + 8, 0, 0, 0, stream()),
                     inputs=[gw], outputs=[gout])[0]
    del raw
    torch.cuda.empty_cache()
    acc, absacc = CC.conv_ref(o["X"], o["Wm"], 1 if mode == 0 else -1)
    refs = GC.references("store16", dt, 9 * Cin, acc, absacc, 1.0)
    GC.check(f"conv3x3 mode {mode} bf16 pointer staging", refs, {"C": y},
             WORST.setdefault(("conv store16 (pointer staging)", dt_id(dt)), {}))
