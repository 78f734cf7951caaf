"""The fp64 references of the 3x3 implicit-GEMM convolution (dclip_conv3x3, dclip_conv3x3_wgrad) as
plain matrix products, on whatever device the tensors live on, in the form gemm_check.references /
gemm_check.check take unchanged (test_gpu_conv_contract.py; test_conv_contract_emulation_cpu.py sends
a CPU emulation of the kernels through the very same path first).

conv_cols(x, d) is the im2col matrix of a channels-last (B, H, W, C) image: row p = (b, y, x), column
tap * C + c holds x[b][(y, x) + d * delta(tap)][c] with delta(tap) = (tap // 3 - 1, tap % 3 - 1), and
zero outside the image.  It is built from F.pad and nine slices: no double-precision convolution is
relied on, and the same matrix of |x| gives the |A| |B| term of the elementwise bound.

  forward   acc = conv_cols(X, +1) @ Wt^T        Wt[co][tap * Cin + ci]  = w[co][ci][tap]   K = 9 Cin
  dgrad     acc = conv_cols(dOut, -1) @ Wd^T     Wd[ci][tap * Cout + co] = w[co][ci][tap]   K = 9 Cout
  wgrad     acc = dY^T @ conv_cols(X, +1)        [co][tap * Cin + ci]                       K = B H W
            and its (Cout, Cin, 3, 3) permutation (oihw), times a power of two (*alpha_ptr)

with `absacc` the same product of the absolute values.  The forms of gemm_check: store16 (a 16-bit
output), store32 (an f32 one, and the weight gradient), resid (accumulate = 1).  The elementwise bound
holds for any summation order, so the pixel split of the weight gradient needs no extra term.
"""
import torch
import torch.nn.functional as F

# (B, H, W): two pixel tiles of 256 with a ragged last one and an image boundary inside the first; one
# ragged tile; every vertical tap out of the image; every horizontal one; a single pixel
GEOMETRIES = [(2, 9, 17), (3, 5, 7), (2, 1, 40), (2, 40, 1), (1, 1, 1)]


def conv_cols(x, d):
    """(B, H, W, C) -> (B*H*W, 9*C): column tap*C + c = x[p + d*delta(tap)][c], zero outside the image"""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))  # one zero pixel around W and H
    taps = []
    for tap in range(9):
        dy, dx = d * (tap // 3 - 1), d * (tap % 3 - 1)
        taps.append(xp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W, :])
    return torch.cat(taps, dim=-1).reshape(B * H * W, 9 * C)


def weights_fwd(w):
    """torch's (Cout, Cin, 3, 3) -> Wt (Cout, 9*Cin), Wt[co][tap*Cin + ci]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9 * w.shape[1])


def weights_dgrad(w):
    """torch's (Cout, Cin, 3, 3) -> Wd (Cin, 9*Cout), Wd[ci][tap*Cout + co]"""
    return w.permute(1, 2, 3, 0).reshape(w.shape[1], 9 * w.shape[0])


def oihw(dw):
    """(Cout, 9*Cin) in (tap, ci) order -> (Cout, Cin*9): torch's (Cout, Cin, 3, 3), flattened"""
    co, k = dw.shape
    return dw.view(co, 9, k // 9).permute(0, 2, 1).reshape(co, k)


def conv_ref(x, wmat, d):
    """(acc, absacc) of out[p][n] = sum_k conv_cols(x, d)[p][k] wmat[n][k]: forward (d = +1, Wt) and
    input gradient (d = -1, x = dOut, Wd); x (B, H, W, C) and wmat as rounded to their 16-bit dtype"""
    cols, w64 = conv_cols(x.double(), d), wmat.double()
    return cols @ w64.t(), cols.abs() @ w64.abs().t()


def wgrad_ref(dy, x, as_oihw=False):
    """(acc, absacc) of dW[co][tap*Cin + ci] = sum_p dY[p][co] X[p + delta(tap)][ci]; dy (B*H*W, Cout)"""
    cols, dy64 = conv_cols(x.double(), 1), dy.double()
    acc, absacc = dy64.t() @ cols, dy64.abs().t() @ cols.abs()
    return (oihw(acc), oihw(absacc)) if as_oihw else (acc, absacc)


def operands(B, H, W, Cin, Nout, dt, seed, device):
    """randn rounded to dt: X (B, H, W, Cin); Wm (Nout, 9*Cin) scaled by (9 Cin)^-0.5; dY (B*H*W, Nout)
    scaled by (B H W)^-0.5; res (B*H*W, Nout) f32; fixed seed"""
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, device=device, generator=g)

    M = B * H * W
    return {"X": randn(B, H, W, Cin).to(dt), "Wm": (randn(Nout, 9 * Cin) * (9 * Cin) ** -0.5).to(dt),
            "dY": (randn(M, Nout) * M ** -0.5).to(dt), "res": randn(M, Nout)}


# ----------------------------------------------------------------------------- what the kernels are meant to compute
def emulate_conv(form, dt, x, wmat, d, res=None):
    """f32 F.conv2d of the rounded operands (d = +1: the forward conv of Wt; d = -1: the input
    gradient of Wd through torch's own conv2d_input), the epilogue in f32, the output rounded"""
    B, H, W, C = x.shape
    n = wmat.shape[0]
    x32 = x.float().permute(0, 3, 1, 2)
    if d == 1:
        w = wmat.float().view(n, 3, 3, C).permute(0, 3, 1, 2)  # (Cout = n, Cin = C, 3, 3)
        y = F.conv2d(x32, w, padding=1)
    else:
        w = wmat.float().view(n, 3, 3, C).permute(3, 0, 1, 2)  # Wd[ci = n][tap][co = C] -> (Cout, Cin, 3, 3)
        y = torch.nn.grad.conv2d_input((B, n, H, W), w, x32, padding=1)
    v = y.permute(0, 2, 3, 1).reshape(B * H * W, n)
    if form == "store16":
        return {"C": v.to(dt)}
    if form == "store32":
        return {"C": v}
    if form == "resid":
        return {"C": v + res}
    raise KeyError(form)


def emulate_wgrad(dy, x, splits=1, as_oihw=False, alpha=1.0):
    """the f32 product of the rounded operands in `splits` pixel chunks of a multiple of 64 rows,
    added in order, then the layout and the factor"""
    cols = conv_cols(x.float(), 1)
    K = cols.shape[0]
    kp = (K + 64 * splits - 1) // (64 * splits) * 64
    v = torch.zeros(dy.shape[1], cols.shape[1], dtype=torch.float32, device=dy.device)
    for s in range(splits):
        v = v + dy[s * kp:(s + 1) * kp].float().t() @ cols[s * kp:(s + 1) * kp]
    if as_oihw:
        v = oihw(v)
    return {"C": v * torch.tensor(alpha, dtype=torch.float32, device=dy.device)}
