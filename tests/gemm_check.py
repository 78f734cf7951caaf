"""The reference, the bounds and the checks of test_gpu_gemm_contract.py, on whatever device the
tensors live on, so that a CPU emulation of the kernels goes through the very same checker
(test_gemm_contract_emulation_cpu.py) before any kernel does.

An NT GEMM output is y = epilogue(alpha * A B^T): `acc` = A B^T and `absacc` = |A| |B|^T are computed
in fp64 from the operands as rounded to their 16-bit dtype.  Two checks per output, in this order:

  blocked   ||y - ref|| / ||ref|| per block of 32 rows x 64 columns (a shorter last block merged into
            its neighbour), under the bound the suite already uses for the whole tensor: TOL[dt] for a
            16-bit output, 1e-5 for f32.  One wrong 16-row x 64-byte store piece is a whole block
            here and 1e-3 of a 11016 x 3072 output's norm.
  element   for the outputs that are linear in the accumulator (STORE, STORE_SCALED, RESIDUAL's C and
            C2, SPLITK, GELU's z), with no excluded share:
                |y - ref| <= 2^-p |ref| + (K + 4) 2^-24 |alpha| (|A| |B|^T) |scale|
                             [+ 2^-24 (|res| + |ref|) for RESIDUAL]
            p = 11 (fp16), 8 (bf16), 24 (f32): rounding to nearest of the output, plus the standard
            dot-product bound gamma_K |a|.|b| in f32, which holds for any summation order (so for
            every tile shape, K split and MFMA accumulation order), with 4 more roundings for alpha,
            the bias, the column scale and a split-K combine.
h = z sigmoid(1.702 z) and GELU_BWD = acc * quick_gelu'(z) take the activation factor in fp64 from
the z the kernel wrote (or was given) and are held to the blocked check only; z itself is held to
both.
"""
import torch

TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2, torch.float32: 1e-5}  # test_gpu_kernels.TOL
P = {torch.float16: 11, torch.bfloat16: 8, torch.float32: 24}
U32 = 2.0 ** -24

# the epilogue forms of dclip_gemm under test: name -> outputs, in the order they are checked
FORMS = {
    "store32": ("C",), "store16": ("C",), "scaled": ("C",), "gelu": ("C", "C2"), "gelu_h": ("C2",),
    "resid": ("C",), "resid_lp": ("C", "C2"), "resid_inplace": ("C",), "gelu_bwd": ("C",), "splitk": ("C",),
}


def quick_gelu(z):
    return z * torch.sigmoid(1.702 * z)


def quick_gelu_grad(z):
    s = torch.sigmoid(1.702 * z)
    return s + 1.702 * z * s * (1 - s)


def _fold(x, b, dim):
    """sums of x over runs of b along dim; a shorter last run is added to its predecessor"""
    x = x.movedim(dim, 0)
    n = x.shape[0]
    if n < b:
        return x.sum(0, keepdim=True).movedim(0, dim)
    nb = n // b
    s = x[:nb * b].reshape(nb, b, *x.shape[1:]).sum(1)
    if n > nb * b:
        s[-1] += x[nb * b:].sum(0)
    return s.movedim(0, dim)


def blocked_err(y, ref, rows=32, cols=64):
    """worst ||y - ref|| / ||ref|| over blocks of rows x cols; returns (error, (first row, first column))"""
    d2 = _fold(_fold((y.double() - ref).pow(2), rows, 0), cols, 1)
    r2 = _fold(_fold(ref.pow(2), rows, 0), cols, 1)
    err = d2.sqrt() / r2.sqrt().clamp(min=1e-300)
    i = int(err.argmax())
    return float(err.reshape(-1)[i]), (i // err.shape[1] * rows, i % err.shape[1] * cols)


def element_ratio(y, ref, bound):
    """worst |y - ref| / bound; returns (ratio, (row, column))"""
    r = (y.double() - ref).abs() / bound.clamp(min=1e-300)
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), (i // r.shape[1], i % r.shape[1])


def references(form, dt, K, acc, absacc, alpha, bias=None, scale=None, res=None, z0=None, outs=None):
    """[(output name, ref fp64, tolerance of the blocked check, elementwise bound or None)] of one call.
    acc, absacc: A B^T and |A| |B|^T in fp64; alpha: the effective factor (alpha * *alpha_ptr);
    bias (N), scale (N), res (M, N), z0 (M, N): the side inputs of the form; outs: the call's outputs
    by name (GELU's h is held to the z the kernel wrote)."""
    lin = acc * alpha
    if bias is not None and form != "gelu_bwd":
        lin = lin + bias.double()
    kterm = (K + 4) * U32 * abs(alpha) * absacc

    def rnd(t):
        return 2.0 ** -P[t]

    if form in ("store32", "splitk"):
        return [("C", lin, TOL[torch.float32], rnd(torch.float32) * lin.abs() + kterm)]
    if form == "store16":
        return [("C", lin, TOL[dt], rnd(dt) * lin.abs() + kterm)]
    if form == "scaled":
        s = scale.double()
        ref = lin * s
        return [("C", ref, TOL[dt], rnd(dt) * ref.abs() + kterm * s.abs())]
    if form == "gelu":
        return [("C", lin, TOL[dt], rnd(dt) * lin.abs() + kterm),
                ("C2", quick_gelu(outs["C"].double()), TOL[dt], None)]
    if form == "gelu_h":  # no z is written: the activation of the exact z
        return [("C2", quick_gelu(lin), TOL[dt], None)]
    if form in ("resid", "resid_lp", "resid_inplace"):
        r = res.double()
        ref = r + lin
        extra = U32 * (r.abs() + ref.abs())
        out = [("C", ref, TOL[torch.float32], rnd(torch.float32) * ref.abs() + kterm + extra)]
        if form == "resid_lp":
            out.append(("C2", ref, TOL[dt], rnd(dt) * ref.abs() + kterm + extra))
        return out
    if form == "gelu_bwd":
        return [("C", lin * quick_gelu_grad(z0.double()), TOL[dt], None)]
    raise KeyError(form)


def check(what, refs, outs, worst=None):
    """every output of `refs` against `outs`: the figures are printed before they are asserted;
    `worst`, when given, collects max(figure / bound) per (output, check)"""
    figures = []
    for name, ref, tol, bound in refs:
        y = outs[name]
        assert y.shape == ref.shape, (what, name, y.shape, ref.shape)
        e, where = blocked_err(y, ref)
        line = f"{what} {name}: worst 32 x 64 block {e:.3e} at {where} (bound {tol:.1e})"
        r, rwhere = (None, None)
        if bound is not None:
            r, rwhere = element_ratio(y, ref, bound)
            line += f", worst |y - ref| / elementwise bound {r:.3f} at {rwhere}"
        print(line)
        figures.append((name, e, where, tol, r, rwhere))
        if worst is not None:
            worst[name, "blocked"] = max(worst.get((name, "blocked"), 0.0), e / tol)
            if r is not None:
                worst[name, "element"] = max(worst.get((name, "element"), 0.0), r)
    for name, e, where, tol, r, rwhere in figures:
        assert e < tol, (what, name, "blocked", e, where)
        if r is not None:
            assert r <= 1.0, (what, name, "elementwise", r, rwhere)


def emulate(form, dt, A, B, alpha, bias=None, scale=None, res=None, z0=None, splits=1):
    """What the kernels are meant to compute, in plain torch: the f32 product of the rounded
    operands (`splits` K chunks, each times alpha, added in order), the epilogue in f32, the outputs
    rounded to their dtype."""
    a32 = torch.tensor(alpha, dtype=torch.float32, device=A.device)
    kc = A.shape[1] // splits
    v = None
    for s in range(splits):
        part = (A[:, s * kc:(s + 1) * kc].float() @ B[:, s * kc:(s + 1) * kc].float().t()) * a32
        v = part if v is None else v + part
    if bias is not None and form != "gelu_bwd":
        v = v + bias
    if form in ("store32", "splitk"):
        return {"C": v}
    if form == "store16":
        return {"C": v.to(dt)}
    if form == "scaled":
        return {"C": (v * scale).to(dt)}
    if form in ("gelu", "gelu_h"):
        z = v.to(dt)
        h = quick_gelu(z.float()).to(dt)
        return {"C": z, "C2": h} if form == "gelu" else {"C2": h}
    if form in ("resid", "resid_lp", "resid_inplace"):
        v = v + res
        return {"C": v, "C2": v.to(dt)} if form == "resid_lp" else {"C": v}
    if form == "gelu_bwd":
        return {"C": (v * quick_gelu_grad(z0.float())).to(dt)}
    raise KeyError(form)


def operands(M, N, K, dt, seed, device):
    """randn rounded to dt, B scaled by K^-0.5, and the side inputs of every form; fixed seed"""
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, device=device, generator=g)

    return {"A": randn(M, K).to(dt), "B": (randn(N, K) * K ** -0.5).to(dt), "bias": randn(N),
            "scale": torch.rand(N, device=device, generator=g) + 0.5, "res": randn(M, N), "z0": randn(M, N).to(dt)}
