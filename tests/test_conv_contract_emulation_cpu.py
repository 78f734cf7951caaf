"""Before any kernel meets test_gpu_conv_contract.py's references, they are checked themselves, on CPU:

  * conv_check.conv_cols and the two weight layouts against fp64 F.conv2d and its autograd
    gradients (forward, input gradient, weight gradient and its OIHW permutation) at the five
    geometries of the GPU file: max |difference| below 1e-11;
  * a plain emulation of the kernels (f32 F.conv2d, or an f32 matmul for the weight gradient, on the
    operands as rounded to their 16-bit dtype, the output rounded to its dtype) through
    gemm_check.references / gemm_check.check, for both dtypes and every form.  A bound this
    emulation misses would be a wrong bound, not a strict one.

Worst figure / bound of the emulation over the five geometries x (Cin, Nout) in {(64, 72), (128, 136)},
forward and input gradient together (fp16 | bf16 operands):
    form                 blocked          element
    store16              0.109 | 0.146    0.772 | 0.943
    store32              0.062 | 0.027    0.007 | 0.003
    resid                0.043 | 0.019    0.007 | 0.003
    wgrad                0.031 | 0.013    0.047 | 0.022
    wgrad, OIHW          0.030 | 0.012    0.047 | 0.022
(a 16-bit output rounded by half an ulp just above a power of two is at 2^-p |ref| by itself; the
f32 outputs sit far below their bounds because K is at most 1152 here.)
"""
import pytest
import torch
import torch.nn.functional as F

import conv_check as CC
import gemm_check as GC

DTS = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
CHANNELS = [(64, 72), (128, 136)]  # (Cin, Nout); the weight gradient needs Cin % 128 == 0 on the GPU, not here


# ----------------------------------------------------------------------------- the references against torch, fp64
@pytest.mark.parametrize("B,H,W", CC.GEOMETRIES, ids=["x".join(map(str, g)) for g in CC.GEOMETRIES])
def test_conv_cols_vs_conv2d_fp64(B, H, W):
    Cin, Cout = 16, 24
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    x = torch.randn(B, H, W, Cin, dtype=torch.float64, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g) * (9 * Cin) ** -0.5
    dy = torch.randn(B * H * W, Cout, dtype=torch.float64, generator=g)
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wn = w.clone().requires_grad_(True)
    y = F.conv2d(xn, wn, padding=1)
    y.backward(dy.view(B, H, W, Cout).permute(0, 3, 1, 2))
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * W, -1)  # noqa: E731
    fwd, _ = CC.conv_ref(x, CC.weights_fwd(w), 1)
    dgrad, _ = CC.conv_ref(dy.view(B, H, W, Cout), CC.weights_dgrad(w), -1)
    wg, _ = CC.wgrad_ref(dy, x)
    wg_oihw, _ = CC.wgrad_ref(dy, x, as_oihw=True)
    errs = {"forward": (fwd - rows(y.detach())).abs().max(), "dgrad": (dgrad - rows(xn.grad)).abs().max(),
            "wgrad": (wg - CC.weights_fwd(wn.grad)).abs().max(),
            "oihw": (wg_oihw - wn.grad.reshape(Cout, Cin * 9)).abs().max()}
    print(f"conv_cols {B}x{H}x{W}: " + ", ".join(f"{k} {float(v):.2e}" for k, v in errs.items()) + " (bound 1e-11)")
    for k, v in errs.items():
        assert float(v) < 1e-11, (k, float(v))


def test_out_of_image_taps_are_exact_zeros():
    """W = 1: the columns of the six taps with dx != 0 are exactly zero, so the weight gradient's
    reference blocks there are exactly zero (the blocked check then demands exact zeros)"""
    x = torch.randn(2, 40, 1, 8, dtype=torch.float64)
    cols = CC.conv_cols(x, 1).view(80, 9, 8)
    for tap in range(9):
        assert bool((cols[:, tap] == 0).all()) == (tap % 3 != 1)


# ----------------------------------------------------------------------------- the emulation through the checker
@pytest.mark.parametrize("form", ["store16", "store32", "resid"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_conv_emulation_stays_under_the_bounds(dt, form):
    worst = {}
    for gi, (B, H, W) in enumerate(CC.GEOMETRIES):
        for ci, (Cin, Nout) in enumerate(CHANNELS):
            for d in (1, -1):
                o = CC.operands(B, H, W, Cin, Nout, dt, 10 * gi + ci, "cpu")
                outs = CC.emulate_conv(form, dt, o["X"], o["Wm"], d, o["res"])
                acc, absacc = CC.conv_ref(o["X"], o["Wm"], d)
                refs = GC.references(form, dt, 9 * Cin, acc, absacc, 1.0, res=o["res"])
                GC.check(f"emulation conv {form} {dt} d={d} {B}x{H}x{W} Cin={Cin} Nout={Nout}", refs, outs, worst)
    print(f"emulation conv {form} {dt}: worst figure / bound "
          + ", ".join(f"{n} {c} {v:.3f}" for (n, c), v in sorted(worst.items())))


@pytest.mark.parametrize("as_oihw", [False, True], ids=["tapmajor", "oihw"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_wgrad_emulation_stays_under_the_bounds(dt, as_oihw):
    worst = {}
    for gi, (B, H, W) in enumerate(CC.GEOMETRIES):
        for ci, (Cin, Nout) in enumerate(CHANNELS):
            o = CC.operands(B, H, W, Cin, Nout, dt, 10 * gi + ci, "cpu")
            splits = (1, 2, 4, 3, 3)[gi]
            alpha = 2.0 ** -9 if as_oihw and ci else 1.0
            outs = CC.emulate_wgrad(o["dY"], o["X"], splits, as_oihw, alpha)
            acc, absacc = CC.wgrad_ref(o["dY"], o["X"], as_oihw)
            refs = GC.references("store32", dt, B * H * W, acc, absacc, alpha)
            GC.check(f"emulation wgrad {dt} {B}x{H}x{W} Cin={Cin} Nout={Nout} splits {splits} oihw {as_oihw}",
                     refs, outs, worst)
    print(f"emulation wgrad {'oihw' if as_oihw else 'tapmajor'} {dt}: worst figure / bound "
          + ", ".join(f"{n} {c} {v:.3f}" for (n, c), v in sorted(worst.items())))
