"""The cases, inputs, fp64 reference, bounds and plain-torch emulation of test_gpu_silog_contract.py
(dclip_upsample_silog: csrc/headloss.hip, band_fold_kernel MODE 1 and MODE 2, band_sums_kernel,
band_merge_kernel), on CPU tensors, so that the emulation goes through the very same checker
(test_silog_contract_emulation_cpu.py) before any kernel does.  Conventions of misc_check.py: the
reference in fp64 from the values the storage dtype holds, u = 2^-24, an item is (output name,
reference, bound), no element is ever excluded, a bound of zero demands the exact value.

The operation (include/dclip.h), X the low-res prediction (B, h, w), gt the target and M the mask
(a non-zero byte; all pixels without a mask) at (B, H, W), eps and lambd as the f32 the ABI takes:
    p = Wy X Wx^T                      the resize of misc_check (interpolation matrices from f32 weights)
    d = log(max(p, eps)) - log(max(gt, eps))                                        on M
    sums = (S0, S1, T) = (sum d, sum d^2, #M)                                       pass 0
    gd = (2 d / T' - 2 lambd S0 / T'^2) / p  where p >= eps and on M, else 0;  T' = T, 1 if T = 0
    grad = Wy^T gd Wx                                                               pass 1
Pass 1 is judged on its own: S0 and T are the very f64 values of the `sums` buffer it was handed
(as dclip_bn_bwd is checked from the statistics dclip_bn_fwd wrote).

Why each bound holds, a = |Wy| |X| |Wx|^T, P = max(p, eps), G = max(gt, eps):
dp    u |p| + 8 u a: the forward resize bound of misc_check (T + 4 = 8 roundings), an f32 output.
dd    2 dp / max(p, eps) [p >= eps] + 2 u (|log P| + |log G|) + u |d|.  log(p + e) - log p = e / p to
      first order, the factor 2 covers the rest (dp / p < 2^-16 in every case); a clamped p is eps
      itself, without error, as long as no pixel sits on the clamp (below).  logf is within 1 ulp <=
      2 u |log| of each logarithm; the subtraction is one rounding.
S0    sum dd + 2^-50 sum |d|: the terms are f32, the sum is f64 in some fixed order.
S1    sum (2 |d| dd + dd^2): (d + e)^2 - d^2; the square and the sum are f64.
T     exact.
gd    mag = (|2 d / T'| + |2 lambd S0 / T'^2|) / |p|, dgd = 2 dd / (T' |p|) + 8 u mag + mag dp / |p|: the
      kernel's own d (dd) through 2 d / T'; 8 roundings, each relative to a term that mag bounds (S0 to
      f32, the lambd product, T'^2, two divisions, the subtraction, 1 / p, the last product: 2 x and T
      to f32 are exact, T < 2^24); 1 / p from a p that is off by dp.  Both are zero where gd is
      (outside M, p < eps).
grad  u |ref| + (Tt + 4) u |Wy|^T mag |Wx| + |Wy|^T dgd |Wx|,  Tt = touch(Wy) touch(Wx): misc_check's
      gradient bound (any order of Tt terms, the weight products) plus the per-pixel error carried
      through the fold.  An accumulating start adds u (|init| + |ref|) for the one f32 add
      -- at the elements at least one pixel with a gradient reaches.  Everywhere else (a low-res
      element no pixel reads when downsampling, every element when T = 0 or p < eps throughout) the
      kernel adds an exact zero, the bound is 0 and the element must come back as it went in.

A pixel is "on the clamp" when it is in M and |p - eps| <= dp: there the kernel and the reference may
take different branches.  forward_ref() asserts that no case has one (a seed that produces one is changed,
the pixel is never excluded).
"""
import zlib

import torch

import misc_check as MC
from misc_check import BF16, F16, F32, NAME, U

F64 = torch.float64
SHAPES = {  # (B, h, w, H, W): the smallest that reach each branch (32 columns per chunk, 8 column slices, 8 rows per load group)
    "x16_seam": (2, 3, 33, 48, 528),   # integer scale, two chunks, the second holding one column, B > 1
    "two_chunks": (1, 2, 64, 8, 256),  # w % 32 == 0: chunk 0 has a 33rd column, chunk 1 none
    "odd": (1, 5, 70, 43, 301),        # three chunks, non-integer scales
    "one_pixel": (1, 1, 1, 7, 9),      # i1 == i and j1 == jj everywhere
    "identity": (1, 6, 6, 6, 6),
    "down": (1, 16, 40, 12, 25),       # low-res elements that no pixel reads: bound 0
    "near_one": (1, 11, 66, 12, 68),
    "tall": (1, 3, 2, 100, 5),         # more than 8 rows per band, fewer than 8 columns per low-res column
    "flat": (1, 1, 40, 9, 500),        # h == 1 with two chunks
}
PARAMS = [(1e-6, 0.5), (0.5, 0.85)]
MASKS = ["none", "random", "empty"]
SUMS_START = (1.5, 2.5, 3.0)
GRAD_START = 0.25
JW = 32  # band_fold_kernel's low-res columns per chunk


def cases():
    return [dict(shape=s, dt=dt, eps=eps, lambd=lambd, mask=m) for s in SHAPES for dt in (F32, BF16, F16)
            for eps, lambd in PARAMS for m in MASKS]


def case_id(c):
    return f"{c['shape']}-{NAME[c['dt']]}-eps{c['eps']:g}-lambd{c['lambd']:g}-{c['mask']}"


def dims(c):
    return SHAPES[c["shape"]]


def f32_of(v):
    """a host float as the ABI receives it"""
    return float(torch.tensor(v, dtype=F32))


def inputs(c):
    """pred (B, h, w) in its dtype, about 8 % below eps; target (B, H, W) f32 in [1, 80] with 5 % zeros;
    mask None or (B, H, W) u8 with valid bytes from {1, 2, 255}; NaN in the masked-out targets"""
    B, h, w, H, W = dims(c)
    g = MC.gen(zlib.crc32(case_id(c).encode()))
    pred = (torch.rand(B, h, w, generator=g) * 60 - 5).to(c["dt"])
    target = 1 + 79 * torch.rand(B, H, W, generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.05] = 0.0
    valid = torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (B, H, W), generator=g)]
    keep = torch.rand(B, H, W, generator=g) < 0.8
    mask = {"none": None, "random": torch.where(keep, valid, torch.zeros_like(valid)),
            "empty": torch.zeros(B, H, W, dtype=torch.uint8)}[c["mask"]]
    if mask is not None:
        target[mask == 0] = float("nan")
    return {"pred": pred, "target": target, "mask": mask}


def in_mask(inp):
    m = inp["mask"]
    return torch.ones_like(inp["target"], dtype=torch.bool) if m is None else m != 0


# ----------------------------------------------------------------------------- the fp64 reference
def forward_ref(c, inp):
    """everything pass 0 and pass 1 share: p, dp, d, dd (0 outside M), M, the sums and their bounds"""
    B, h, w, H, W = dims(c)
    eps = f32_of(c["eps"])
    M = in_mask(inp)
    p, a = MC.resize_ref(inp["pred"], H, W)
    dp = U * p.abs() + 8 * U * a
    on_clamp = M & ((p - eps).abs() <= dp)
    assert not bool(on_clamp.any()), f"{case_id(c)}: {int(on_clamp.sum())} pixels on the clamp: change the seed"
    zero = torch.zeros_like(p)
    logP = torch.log(p.clamp(min=eps))
    logG = torch.where(M, torch.log(inp["target"].double().clamp(min=eps)), zero)
    d = torch.where(M, logP - logG, zero)
    dd = 2 * dp / p.clamp(min=eps) * (p >= eps) + 2 * U * (logP.abs() + logG.abs()) + U * d.abs()
    dd = torch.where(M, dd, zero)
    S0, S1, T = d.sum(), d.pow(2).sum(), M.sum().double()
    return dict(p=p, dp=dp, d=d, dd=dd, M=M, S0=S0, S1=S1, T=T,
                eS0=dd.sum() + 2.0 ** -50 * d.abs().sum(), eS1=(2 * d.abs() * dd + dd.pow(2)).sum())


def sums_items(c, inp, fwd=None):
    """pass 0's three sums (each as a 1-element tensor), the accumulator's start already subtracted"""
    f = fwd or forward_ref(c, inp)
    one = lambda v: torch.as_tensor(v, dtype=F64).reshape(1)  # noqa: E731
    return [("S0", one(f["S0"]), one(f["eS0"])), ("S1", one(f["S1"]), one(f["eS1"])), ("T", one(f["T"]), one(0.0))]


def grad_items(c, inp, sums, init=GRAD_START, fwd=None):
    """pass 1 from the f64 `sums` it was given, accumulated onto `init`"""
    B, h, w, H, W = dims(c)
    eps, lambd = f32_of(c["eps"]), f32_of(c["lambd"])
    f = fwd or forward_ref(c, inp)
    p, d, dd, dp = f["p"], f["d"], f["dd"], f["dp"]
    S0, T = float(sums[0]), float(sums[2])
    Tp = T if T > 0 else 1.0
    live = f["M"] & (p >= eps)
    zero = torch.zeros_like(p)
    gd = torch.where(live, (2 * d / Tp - 2 * lambd * S0 / Tp ** 2) / p, zero)
    mag = torch.where(live, ((2 * d / Tp).abs() + abs(2 * lambd * S0 / Tp ** 2)) / p.abs(), zero)
    dgd = torch.where(live, 2 * dd / (Tp * p.abs()) + 8 * U * mag + mag * dp / p.abs(), zero)
    Wy, Wx = MC.lerp_matrix(h, H), MC.lerp_matrix(w, W)
    fold = lambda t: Wy.abs().t() @ t @ Wx.abs()  # noqa: E731
    ref = Wy.t() @ gd @ Wx
    Tt = MC.touch(Wy) * MC.touch(Wx)
    fmag = fold(mag)
    bound = U * ref.abs() + (Tt + 4) * U * fmag + fold(dgd)
    init = torch.as_tensor(init, dtype=F64).expand_as(ref)
    bound = bound + U * (init.abs() + ref.abs()) * (fmag > 0)
    return [("grad", init + ref, bound)]


def loss_ref(c, inp, fwd=None):
    """SILogLoss's value from the reference sums, with lambd as the host double ops.UpsampleSILogFn
    uses, and the bound the sums' bounds imply plus the result's rounding to f32"""
    f = fwd or forward_ref(c, inp)
    S0, S1, T, lambd = float(f["S0"]), float(f["S1"]), float(f["T"]), float(c["lambd"])
    if T == 0:
        return 0.0, 0.0
    e0, e1 = float(f["eS0"]), float(f["eS1"])
    loss = S1 / T - lambd * S0 ** 2 / T ** 2
    bound = (e1 / T + lambd * (2 * abs(S0) * e0 + e0 ** 2) / T ** 2 + U * abs(loss)
             + 2.0 ** -50 * (S1 / T + lambd * S0 ** 2 / T ** 2))
    return loss, bound


# ----------------------------------------------------------------------------- the f32 emulation
def emu_pixels(c, inp):
    """p, d (f32, d zero outside the mask) and the mask, as band_fold_kernel computes them per pixel"""
    B, h, w, H, W = dims(c)
    eps = torch.tensor(c["eps"], dtype=F32)
    M = in_mask(inp)
    p = MC.emu_resize(inp["pred"], H, W)
    d = torch.log(torch.where(p < eps, eps, p)) - torch.log(torch.where(inp["target"] < eps, eps, inp["target"]))
    assert p.dtype == d.dtype == F32
    return p, torch.where(M, d, torch.zeros_like(d)), M


def emu_sums(d, M, start=(0.0, 0.0, 0.0)):
    """sums += (sum d, sum d^2, T): f32 terms, f64 sums"""
    dm = d.double()[M]
    return torch.tensor(start, dtype=F64) + torch.stack([dm.sum(), dm.pow(2).sum(), M.sum().double()])


def emu_gd(c, p, d, M, sums, zero_below_eps=True, clamp_T=True):
    """the per-pixel gradient as the kernel writes it: S and T cast to f32"""
    eps, lambd = torch.tensor(c["eps"], dtype=F32), torch.tensor(c["lambd"], dtype=F32)
    gS, gT = sums[0].to(F32), sums[2].to(F32)
    if clamp_T:
        gT = gT if float(gT) > 0 else torch.tensor(1.0, dtype=F32)
    inv = torch.where(p >= eps, 1 / p, torch.zeros_like(p)) if zero_below_eps else 1 / p
    gd = (2 * d / gT - 2 * lambd * gS / (gT * gT)) * inv
    assert gd.dtype == F32
    return torch.where(M, gd, torch.zeros_like(gd))


def emu_fold(c, gd, init=GRAD_START):
    B, h, w, H, W = dims(c)
    return torch.full((B, h, w), init, dtype=F32) + MC.emu_resize_grad(gd, h, w)


def emulate(c, inp, sums_start=SUMS_START, grad_start=GRAD_START):
    """both passes as the GPU test runs them: pass 0 onto `sums_start` (the start subtracted again in
    fp64), pass 1 onto `grad_start` and onto zero from a pass 0 of its own that started at zero;
    returns (outputs by name, that pass 0's sums)"""
    p, d, M = emu_pixels(c, inp)
    s = emu_sums(d, M, sums_start) - torch.tensor(sums_start, dtype=F64)
    given = emu_sums(d, M)
    gd = emu_gd(c, p, d, M, given)
    return {"S0": s[0:1], "S1": s[1:2], "T": s[2:3], "grad": emu_fold(c, gd, grad_start), "grad0": emu_fold(c, gd, 0.0)}, given


def items(c, inp, given, grad_start=GRAD_START):
    """the sums, the gradient accumulated onto `grad_start` and, as "grad0", onto zero: next to 0.25 the
    rounding of the last add is a thousand times a typical element's own bound, so the run from zero
    is the one that weighs the fold"""
    f = forward_ref(c, inp)
    (_, ref0, bound0), = grad_items(c, inp, given, 0.0, f)
    return sums_items(c, inp, f) + grad_items(c, inp, given, grad_start, f) + [("grad0", ref0, bound0)]
