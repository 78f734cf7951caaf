"""The attention entry points (and the two other hot-path workspaces: the split-K TN GEMM and the
LayerNorm backward) called through the C ABI on guard-banded, poisoned buffers (abi_guard.py).

What the per-kernel tests cannot see, because the op layer's at::empty hands a second call the
first call's freed — and correct — block:
  * a row or a workspace partial that is never written, or read before it is written (outputs and
    workspaces enter as 0xFF = NaN, then as 0x3C; the results must be finite and bitwise equal);
  * a write outside a buffer, a read past an input's last element that reaches a result (every
    buffer lies between two 1 MiB bands of NaN);
  * one wrong tile hidden in a norm over the whole tensor: forward and gradients are compared with
    fp64 autograd of softmax(q k^T d^-0.5) v per BLOCK of 32 rows of an image (a shorter last block
    merged into its predecessor) x one head's 64 columns x q / k / v part, against the bounds the
    suite already uses for the whole tensor (TOL[dt] for o, 1e-2 absolute for lse, 4 TOL[dt] for
    the gradients; error = ||y - ref|| / max(||ref||, floor), floor = the existing 1e-3 ||dout||
    scaled by sqrt(block elements / all elements); o takes no floor).  The project's 16-bit
    emulation (emulation16.Attn16, output rounded to dt) at these shapes over 5 seeds has its worst
    block at 4.6e-3 (bf16, bound 4.8e-2) and 6.3e-4 (fp16, bound 8e-3);
  * the option x entry point matrix: every dispatch row of dclip_attn_bwd and dclip_attn_bwd_fp8 at
    N = 65 (generic), 257 (one key block), 290 (N - 1 = 256 + 33: partial key block and partial
    64-tile), 449 (N - 1 = 256 + 192) and 513, B = 2, H = 3 (both > 1, H odd: a swapped b / h index
    shows), with the workspace sized by the library's own query — its trailing guard is the
    workspace contract's check.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from abi_guard import bitwise_equal, guarded, guarded_copy, option_scope, run_poisoned
from helpers import rel_err
from test_gpu_fp8 import make_qkv
from test_gpu_kernels import TOL, prescale

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 2, 3
C = 64 * H
SCALE = 64 ** -0.5
NS = [65, 257, 290, 449, 513]
DTS = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def NT():
    from denseclip_vit_multimodal_amd import _native
    return _native


def code(dt):
    return {torch.float16: NT().F16, torch.bfloat16: NT().BF16, torch.float32: NT().F32}[dt]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def under():
    """under(opts, fn): fn() with the (option id, value) pairs set; every option is back at 0 when
    fn returns or raises, and again at teardown."""
    seen = []

    def run(opts, fn):
        with option_scope() as set_option:
            for o, v in opts:
                seen.append(o)
                set_option(o, v)
            return fn()

    try:
        yield run
    finally:
        for o in seen:
            NT().call("dclip_set_option", o, 0)


# ----------------------------------------------------------------------------- references (computed once)
def exact(qkv, dout, N):
    """fp64 autograd of softmax(q k^T d^-0.5) v on the GPU from the kernels' rounded inputs:
    (o (B*N, C), lse log2-domain (B*H*N), d qkv (B*N, 3C)) — read-only for every test"""
    r = qkv.double()
    r[:, :C] /= SCALE * math.log2(math.e)  # the unscaled q the log2-domain contract implies
    r.requires_grad_(True)
    q, k, v = r.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * SCALE
    o = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * N, C)
    o.backward(dout.double())
    lse = (torch.logsumexp(s, -1) / math.log(2)).reshape(-1)
    return o.detach(), lse.detach(), r.grad


_CASES = {}


def case(N, dt):
    """prescale((randn * 1.5).to(dt)) inputs in guarded buffers, the fp64 reference, and the default
    forward's (o, lse) — the backward's inputs — computed on poisoned buffers"""
    if (N, dt) not in _CASES:
        torch.manual_seed(1000 + N)
        qkv, _ = prescale((torch.randn(B * N, 3 * C, device=DEV) * 1.5).to(dt), H)
        dout = torch.randn(B * N, C, device=DEV).to(dt)
        c = {"key": ("16", N, dt), "N": N, "dt": dt, "qkv": guarded_copy(qkv), "dout": guarded_copy(dout)}
        c["oref"], c["lref"], c["gref"] = exact(qkv, dout, N)
        o, lse = fwd(c, "dclip_attn_fwd")
        c["o"], c["lse"] = guarded_copy(o), guarded_copy(lse)
        _CASES[N, dt] = c
    return _CASES[N, dt]


_CASES8 = {}


def case8(N, dt):
    """test_fp8_backward_kernel's setting: make_qkv(spread=1.0), the fp8 forward's (o, lse)"""
    if (N, dt) not in _CASES8:
        torch.manual_seed(2000 + N)
        qkv = make_qkv(B, N, H, dt, spread=1.0)
        dout = torch.randn(B * N, C, device=DEV).to(dt)
        c = {"key": ("8", N, dt), "N": N, "dt": dt, "qkv": guarded_copy(qkv), "dout": guarded_copy(dout)}
        _, _, c["gref"] = exact(qkv, dout, N)
        o, lse = fwd(c, "dclip_attn_fwd_fp8")
        c["o"], c["lse"] = guarded_copy(o), guarded_copy(lse)
        _CASES8[N, dt] = c
    return _CASES8[N, dt]


def fwd(c, entry):
    """(o, lse) of dclip_attn_fwd / dclip_attn_fwd_fp8 under the options in force, run poisoned"""
    L = NT()
    N, dt = c["N"], c["dt"]
    go, gl = guarded((B * N, C), dt), guarded((B * H * N,), torch.float32)
    if entry == "dclip_attn_fwd":
        return run_poisoned(lambda: L.call(entry, code(dt), c["qkv"].ptr(), go.ptr(), gl.ptr(), B, N, H, 64, SCALE,
                                           stream()), inputs=[c["qkv"]], outputs=[go, gl])
    ws = guarded(L.lib().dclip_attn_fwd_fp8_workspace(B, N, H), torch.uint8)  # bytes; the payload is 256-B aligned
    return run_poisoned(lambda: L.call(entry, code(dt), c["qkv"].ptr(), go.ptr(), gl.ptr(), ws.ptr(), B, N, H, 64,
                                       stream()), inputs=[c["qkv"]], outputs=[go, gl], scratch=[ws])


_BWD = {}


def bwd(under, c, entry, opts):
    """dqkv of dclip_attn_bwd / dclip_attn_bwd_fp8 under `opts`, run poisoned with the workspace the
    library's own query gives under those options; computed once per (inputs, entry, options)"""
    key = (c["key"], entry, tuple(opts))
    if key not in _BWD:
        L = NT()
        N, dt = c["N"], c["dt"]

        def run():
            ws = guarded(getattr(L.lib(), entry + "_workspace")(B, N, H), torch.float32)
            gd = guarded((B * N, 3 * C), dt)
            ins = [c["qkv"], c["o"], c["dout"], c["lse"]]
            return run_poisoned(lambda: L.call(entry, code(dt), c["qkv"].ptr(), c["o"].ptr(), c["dout"].ptr(),
                                               c["lse"].ptr(), ws.ptr(), gd.ptr(), B, N, H, 64, SCALE, stream()),
                                inputs=ins, outputs=[gd], scratch=[ws])[0]

        _BWD[key] = under(opts, run)
    return _BWD[key]


# ----------------------------------------------------------------------------- blocked error
def blocked_err(y, ref, N, floor_all=0.0, all_elems=1):
    """y, ref (B*N, G*64): the worst ||y - ref|| / max(||ref||, floor) over blocks of 32 rows of an image
    (a shorter last block merged into its predecessor) x 64 columns; the floor of a block is floor_all
    sqrt(block elements / all_elems).  Returns (error, (image, first row, column group))."""
    G = y.shape[1] // 64
    d2 = (y.double() - ref).view(B, N, G, 64).pow(2).sum(-1)
    r2 = ref.view(B, N, G, 64).pow(2).sum(-1)
    nb = N // 32
    edges = (list(range(0, 32 * nb, 32)) if nb else [0]) + [N]
    lo, hi = torch.tensor(edges[:-1], device=y.device), torch.tensor(edges[1:], device=y.device)

    def blocks(x):
        cs = torch.cat([torch.zeros_like(x[:, :1]), x.cumsum(1)], 1)
        return (cs[:, hi] - cs[:, lo]).clamp(min=0)

    floor = floor_all * torch.sqrt((hi - lo).double() * 64 / all_elems).view(1, -1, 1)
    err = blocks(d2).sqrt() / torch.maximum(blocks(r2).sqrt(), floor.expand(B, -1, G)).clamp(min=1e-300)
    i = int(err.argmax())
    b, rest = divmod(i, err.shape[1] * G)
    blk, g = divmod(rest, G)
    return float(err.max()), (b, edges[blk], g)


def check_grads(c, dqkv, what):
    """blocked dq / dk / dv against fp64 autograd at 4 TOL[dt]"""
    N, dt = c["N"], c["dt"]
    floor = 1e-3 * float(c["dout"].t.double().norm())
    worst = []
    for part, name in enumerate("qkv"):
        sl = slice(part * C, (part + 1) * C)
        e, where = blocked_err(dqkv[:, sl], c["gref"][:, sl], N, floor, B * N * C)
        worst.append((name, e, where))
    print(f"{what} N={N} {dt}: worst 32-row x head block d" + ", d".join(f"{n} {e:.3e} at {w}" for n, e, w in worst)
          + f" (bound {4 * TOL[dt]:.1e})")
    for n, e, w in worst:
        assert e < 4 * TOL[dt], (n, e, w)


# ----------------------------------------------------------------------------- 1. dclip_attn_fwd
@pytest.mark.parametrize("kernel,waves", [(0, 0), (0, 4), (1, 0), (2, 0), (3, 0), (4, 0)])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_attn_fwd_poisoned_blocked(dt, N, kernel, waves, under):
    c = case(N, dt)
    o, lse = under([(NT().OPT_ATTN_FWD_KERNEL, kernel), (NT().OPT_ATTN_FWD_WAVES, waves)],
                   lambda: fwd(c, "dclip_attn_fwd"))
    e, where = blocked_err(o, c["oref"], N)
    el = float((lse.double() - c["lref"]).abs().max())
    print(f"attn_fwd kernel {kernel} waves {waves} N={N} {dt}: worst block o {e:.3e} at {where} "
          f"(bound {TOL[dt]:.1e}), lse {el:.3e} (bound 1e-2)")
    assert e < TOL[dt], (e, where)
    assert el < 1e-2, el


# ----------------------------------------------------------------------------- 2. dclip_attn_fwd_fp8
@pytest.mark.parametrize("qk", [0, 1])
@pytest.mark.parametrize("N", [65, 257, 290])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_attn_fwd_fp8_poisoned(dt, N, qk, under):
    """the poison checks only (run_poisoned): the fp8 forward's accuracy is test_gpu_fp8.py's"""
    c = case8(N, dt)
    under([(NT().OPT_ATTN_FP8_QK, qk)], lambda: fwd(c, "dclip_attn_fwd_fp8"))


# ----------------------------------------------------------------------------- 3. dclip_attn_bwd
def bwd_rows():
    n = NT()
    blk = lambda v: [(n.OPT_ATTN_BWD_BLOCK, v)]  # noqa: E731
    rows = {"default": []}
    rows.update({f"block{v}": blk(v) for v in (1, 5, 6, 7, 8, 9, 10)})
    rows.update({
        "kernel1": [(n.OPT_ATTN_BWD_KERNEL, 1)],
        "dqw4": [(n.OPT_ATTN_DQ_WAVES, 4)],
        "dqw4_block6": [(n.OPT_ATTN_DQ_WAVES, 4)] + blk(6),
        "dkdvw8_block1": [(n.OPT_ATTN_DKDV_WAVES, 8)] + blk(1),
        "qs128_kernel1": [(n.OPT_ATTN_DKDV_QS, 128), (n.OPT_ATTN_BWD_KERNEL, 1)],
        "rows64_block6": [(n.OPT_ATTN_DQ_ROWS, 64)] + blk(6),
        "defer_block6": [(n.OPT_ATTN_DQ_DEFER, 1)] + blk(6),
        "issue_block6": [(n.OPT_ATTN_DQ_ISSUE, 1)] + blk(6),
        "reduce": [(n.OPT_ATTN_DQ_REDUCE, 1)],
        "prep_order": [(n.OPT_ATTN_PREP_ORDER, 1)],
    })
    return rows


BWD_ROW_IDS = ["default", "block1", "block5", "block6", "block7", "block8", "block9", "block10", "kernel1", "dqw4",
               "dqw4_block6", "dkdvw8_block1", "qs128_kernel1", "rows64_block6", "defer_block6", "issue_block6",
               "reduce", "prep_order"]
# the bitwise relations the suite claims (test_attention_dkdv7_bitwise_dkdv6,
# test_attention_onepass_dq_reduce_lds_bitwise, option 10 = the default), where stale memory cannot fake them
BWD_BITWISE = {"block7": "block6", "block8": "block6", "reduce": "default", "prep_order": "default",
               "block10": "default"}


@pytest.mark.parametrize("row", BWD_ROW_IDS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_attn_bwd_poisoned_blocked(dt, N, row, under):
    rows = bwd_rows()
    assert sorted(rows) == sorted(BWD_ROW_IDS)
    c = case(N, dt)
    dqkv = bwd(under, c, "dclip_attn_bwd", rows[row])
    check_grads(c, dqkv, f"attn_bwd {row}")
    if row in BWD_BITWISE:
        assert bitwise_equal(dqkv, bwd(under, c, "dclip_attn_bwd", rows[BWD_BITWISE[row]])), (row, BWD_BITWISE[row])


# ----------------------------------------------------------------------------- 4. dclip_attn_bwd_fp8
FP8_ROW_IDS = ["block0", "block1", "block5", "block6", "block7", "block8", "block9", "block10", "dqw4", "kernel1"]


@pytest.mark.parametrize("row", FP8_ROW_IDS)
@pytest.mark.parametrize("N", [65, 257, 290, 513])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_attn_bwd_fp8_poisoned_options(dt, N, row, under):
    """dclip_attn_bwd_fp8's contract (include/dclip.h): on the CLS-split path (N >= 257, not
    DCLIP_OPT_ATTN_BWD_KERNEL 1, not a ragged N - 1 with DCLIP_OPT_ATTN_DQ_WAVES 4) every
    DCLIP_OPT_ATTN_BWD_BLOCK value gives option 0's result bit for bit, dQ and the key-0 rows are the
    two-pass dclip_attn_bwd's (option 6) bit for bit, and option 0's dK / dV are within the e4m3
    bound 5e-2 (norm-wise, test_fp8_backward_kernel) of fp64 autograd; elsewhere the whole output is
    dclip_attn_bwd's under the same options, bit for bit."""
    n = NT()
    opts = {"dqw4": [(n.OPT_ATTN_DQ_WAVES, 4)], "kernel1": [(n.OPT_ATTN_BWD_KERNEL, 1)]}.get(row)
    if opts is None:
        opts = [(n.OPT_ATTN_BWD_BLOCK, int(row[5:]))]
    c = case8(N, dt)
    d8 = bwd(under, c, "dclip_attn_bwd_fp8", opts)
    split = N >= 257 and row != "kernel1" and not (row == "dqw4" and (N - 1) % 256 != 0)
    if not split:
        assert bitwise_equal(d8, bwd(under, c, "dclip_attn_bwd", opts))
        return
    if row.startswith("block"):
        assert bitwise_equal(d8, bwd(under, c, "dclip_attn_bwd_fp8", [(n.OPT_ATTN_BWD_BLOCK, 0)]))
    two_pass = [(n.OPT_ATTN_DQ_WAVES, 4)] if row == "dqw4" else []
    d16 = bwd(under, c, "dclip_attn_bwd", two_pass + [(n.OPT_ATTN_BWD_BLOCK, 6)])
    assert bitwise_equal(d8[:, :C], d16[:, :C])  # dQ: the 16-bit dQ pass
    k0 = torch.arange(B, device=DEV) * N  # key 0 of every image: the 16-bit fold merge
    assert bitwise_equal(d8[k0], d16[k0])
    if row == "block0":
        e8 = [rel_err(d8[:, s].float(), c["gref"][:, s]) for s in (slice(C, 2 * C), slice(2 * C, 3 * C))]
        print(f"attn_bwd_fp8 N={N} {dt}: dK / dV rel err vs fp64 {e8} (bound 5e-2)")
        assert max(e8) < 5e-2, e8


# ----------------------------------------------------------------------------- D. dclip_gemm_tn, SPLITK
@pytest.mark.parametrize("forced", [0, 3], ids=["plan", "splits3"])
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("K,M,N", [(70, 264, 520), (1000, 256, 384)])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_gemm_tn_splitk_poisoned(dt, K, M, N, tile, forced, under):
    """C = A^T B through the split-K slabs of a poisoned workspace; K is not a multiple of 64, so
    K_pad > K and the rows >= K that "contribute zero" lie in the NaN band behind A and B.  splits
    from dclip_gemm_tn_plan, and forced to 3 with its K_pad (K = 70: the last split holds no row
    at all).  colsum_a is given here on the 256x256 kernel only, from the time the small-tile path
    was thought to add it with atomics; it does not: colsum_kernel reduces each split's rows in LDS in
    a fixed order and the combine adds the per-split partials in split order, so colsum_a repeats
    bit for bit on every path (include/dclip.h says so now).  The small-tile path, and the 256x256
    tiles without fused sums (DCLIP_OPT_GEMM_TN_TILE 2, 3), are held to an fp64 reference and to
    bitwise equality between the two poison runs by test_gpu_conv_contract.py's
    test_gemm_tn_splitk_strided."""
    import ctypes
    L = NT()
    torch.manual_seed(5)
    A = guarded_copy(torch.randn(K, M, device=DEV).to(dt))
    Bm = guarded_copy(torch.randn(K, N, device=DEV).to(dt))
    ref = A.t.double().t() @ Bm.t.double()

    def run():
        if forced:
            splits, k_pad = forced, (K + 64 * forced - 1) // (64 * forced) * 64 * forced
        else:
            sp, kp = ctypes.c_int(0), ctypes.c_int64(0)
            L.call("dclip_gemm_tn_plan", M, N, K, ctypes.byref(sp), ctypes.byref(kp))
            splits, k_pad = sp.value, kp.value
        assert k_pad > K
        big = tile != 1 and M >= 256 and N >= 256
        ws = guarded(splits * (M * N + M), torch.float32)
        out = guarded((M, N), torch.float32)
        cs = [guarded(M, torch.float32)] if big else []
        res = run_poisoned(lambda: L.call("dclip_gemm_tn", L.EPI_SPLITK, code(dt), A.ptr(), M, Bm.ptr(), N, M, N, K,
                                          k_pad, splits, 1.0, None, None, ws.ptr(), out.ptr(), N,
                                          cs[0].ptr() if big else None, stream()),
                           inputs=[A, Bm], outputs=[out], scratch=[ws], accum=cs)
        return res, splits

    res, splits = under([(L.OPT_GEMM_TN_TILE, tile)], run)
    e = rel_err(res[0], ref)
    print(f"gemm_tn SPLITK K={K} M={M} N={N} {dt} tile {tile} splits {splits}: rel err {e:.3e} (bound 1e-5)")
    assert e < 1e-5, e
    if len(res) > 1:
        ec = rel_err(res[1], A.t.double().sum(0))
        assert ec < 1e-5, ec


# ----------------------------------------------------------------------------- D. dclip_layernorm_bwd_res
@pytest.mark.parametrize("lpdt", [None, torch.bfloat16], ids=["nolp", "lp_bf16"])
@pytest.mark.parametrize("dydt", [torch.bfloat16, torch.float32], ids=["dy_bf16", "dy_f32"])
@pytest.mark.parametrize("cols", [512, 768, 1024])
def test_layernorm_bwd_res_poisoned(cols, dydt, lpdt):
    """dx = res + LN^T(dy), its 16-bit copy, dw and db through the per-workgroup partials of a
    poisoned dclip_layernorm_bwd_ws_floats workspace, against fp64 autograd at the existing 1e-5."""
    L = NT()
    rows = 517
    torch.manual_seed(7)
    x = torch.randn(rows, cols, device=DEV) * 2
    w = torch.randn(cols, device=DEV)
    dy = torch.randn(rows, cols, device=DEV).to(dydt)
    res = torch.randn(rows, cols, device=DEV)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = torch.zeros(cols, device=DEV, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x64, (cols,), w64, b64, 1e-5).backward(dy.double())
    mean = x.double().mean(1).float()
    rstd = torch.rsqrt(x.double().var(1, unbiased=False) + 1e-5).float()
    ins = [guarded_copy(t) for t in (dy, x, w, mean, rstd, res)]
    gdy, gx, gw, gm, gr, gres = ins
    nws = L.lib().dclip_layernorm_bwd_ws_floats(rows, cols)
    assert nws > 0
    ws = guarded(nws, torch.float32)
    dx = guarded((rows, cols), torch.float32)
    lp = guarded((rows, cols), lpdt) if lpdt is not None else None
    dw, db = guarded(cols, torch.float32), guarded(cols, torch.float32)
    out = run_poisoned(lambda: L.call("dclip_layernorm_bwd_res", gdy.ptr(), code(dydt), None, 0, gx.ptr(), L.F32,
                                      gw.ptr(), gm.ptr(), gr.ptr(), gres.ptr(), dx.ptr(),
                                      lp.ptr() if lp is not None else None, code(lpdt) if lp is not None else 0,
                                      dw.ptr(), db.ptr(), ws.ptr(), rows, cols, stream()),
                       inputs=ins, outputs=[dx] + ([lp] if lp is not None else []), scratch=[ws], accum=[dw, db])
    e = [rel_err(out[0], res.double() + x64.grad), rel_err(out[-2], w64.grad), rel_err(out[-1], b64.grad)]
    print(f"layernorm_bwd_res cols {cols} dy {dydt} lp {lpdt}: dx, dw, db rel err {e} (bound 1e-5)")
    assert max(e) < 1e-5, e
    if lp is not None:
        assert bitwise_equal(out[1], out[0].to(lpdt))
