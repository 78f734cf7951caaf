"""The cases, references, bounds and plain-torch emulations of test_gpu_misc_contract.py (every kernel
of csrc/misc.hip but dclip_weight_refresh and the fp16-scaling entry points dclip_grad_scale,
dclip_add_readout_cast / _amax / _cast_scaled and dclip_row_scale_add, which norm_check.py and
test_gpu_norm_contract.py hold to the same kind of contract), on CPU tensors, so
that the emulation goes through the very same checker (test_misc_contract_emulation_cpu.py) before
any kernel does.  Conventions of gemm_check.py: every reference in fp64 from the operands as
rounded to their storage dtype, p = 11 / 8 / 24 for fp16 / bf16 / f32 outputs, u = 2^-24, no share
of elements ever excluded; "2^-p |ref|" for an fp16 output is max(2^-11 |ref|, 2^-25), fp16's spacing
below 2^-14 being 2^-24 whatever the value (rounding()).  An item of a family's refs() is (output name, reference, bound); bound
None means bitwise (+0 and -0 differ).  A bound of zero at an element demands the exact value.

Every family is FAMILIES[name] = (cases, inputs, emulate, refs): `cases` the list of the GPU test's
cases (dicts), inputs(case) the operands (CPU, fixed seed, rounded to their dtype), emulate(case,
inputs) the outputs by name in f32 torch arithmetic rounded to the output dtype, refs(case, inputs,
outputs) the items.  Why each bound holds:

bitwise    im2col, transpose (a copy through f32, one RNE cast; with accumulate one f32 add, which
           is the RNE of the exact sum and so has one possible result), the copied channels of
           score_concat, tokens_fwd (one f32 add), cast and dpatch of tokens_bwd (one f32 multiply,
           one RNE cast), row 0 of pos_interp_fwd, a resize whose sizes are equal (l1 = 0, l0 = 1).
resize     Wy (Ho x Hi), Wx (Wo x Wi): l0 at i0 and l1 at i1 of the header's index formula in f32
           (scale = in / out, src = max(scale (dst + .5) - .5, 0), i0 = (int) src, i1 = i0 + (i0 <
           in - 1), l1 = src - i0, l0 = 1 - l1), taken to fp64: the weights themselves are then
           exact, ref = Wy X Wx^T is linear in X and absacc = |Wy| |X| |Wx|^T.  scale (dst + .5) - .5
           is one fused multiply-add, rounded once: that is how hipcc contracts lerp_index (misc.hip)
           and how PyTorch's own CPU kernel evaluates it -- with the product rounded separately src
           moves by an ulp at 221 of 1028 columns of 5 -> 1028, and F.interpolate then misses the
           bound below by a factor of 3.4 (test_misc_contract_emulation_cpu.py shows both).
             |y - ref| <= 2^-p |ref| + (T + 4) u absacc
           forward: l0 (l0' a + l1' b) + l1 (l0' c + l1' d) puts at most T = 4 roundings on the path
           of any operand (product, inner sum, product, outer sum), each relative to a partial sum
           that |.| bounds; the 4 more are headroom (l0 = 1 - l1 is rounded in W as in the kernel).
           gradients: an element of din / dpos sums w_y w_x g over the T outputs that touch it (T =
           the largest column count of non-zeros of Wy times that of Wx; the two-pass bilinear
           backward has Ty + Tx <= T + 1 terms): any order of T terms costs (T - 1) u, the weight
           product and the two multiplies 3 u.  An accumulating argument (+=) adds u and |init| to
           absacc.
row_mean   a sum of `rows` exact f32 values in any order, (rows - 1) u sum|x|, one division:
             |y - ref| <= (rows + 4) u mean_r |x|
tokens_bwd dcls / dpos: init + sum over B:  (B + 2) u (|init| + sum_b |dx|)
colsum     init + sum over batch * rows, float atomics (any order):
             (batch rows + 2) u (|init| + sum |in|)
score_map  v^ = v / max(|v|, eps), t^ = t / max(|t|, eps) in fp64, ref = <v^, t^>:
             |y - ref| <= (2^-p(dt) + (C + 8) u) sum_c |v^_c t^_c|
           t^ is rounded to nearest in the operand dtype: 2^-(p+1) per term, half of the first
           term.  The other half (2^-12 >= 4096 u at fp16) covers the two f32 sums of squares:
           sums of positive terms, so relative errors of C u, C u / 2 each after the root, C u in
           all for C <= 2048.  The dot product is f32 in any order (C u); the roots, reciprocals and
           products are the 8.  A zero pixel row or class row has bound 0: exactly 0.
batchnorm  see bn_refs: the kernel's shifted sums S = sum(x - x0), Q = sum(x - x0)^2 (x0 = row 0),
           errors (rows + 2) u sum|x - x0| and (rows + 4) u Q, propagated through md = S / n, var =
           Q / n - md^2 (so the bound scales with Q / n + md^2, not with var), rsqrt, the running
           statistics, scale / shift and the output's rounding.
"""
import torch

from gemm_check import P, U32

U = U32
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
LOW = [F16, BF16]
NAME = {F32: "f32", F16: "fp16", BF16: "bf16"}


def eps_of(dt):
    return 2.0 ** -P[dt]


def rounding(dt, ref):
    """the rounding of `ref` to dt: 2^-p |ref|, and below fp16's smallest normal (2^-14), where the
    spacing is 2^-24 whatever the value, half of that"""
    r = eps_of(dt) * ref.abs()
    return r.clamp(min=2.0 ** -25) if dt == F16 else r


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def dyadic(g, *shape):
    """multiples of 1/8 in [-4, 4]: exact in every dtype, and so is any f32 sum of fewer than 2^18"""
    return torch.randint(-32, 33, shape, generator=g).float() / 8


# ----------------------------------------------------------------------------- the checker
def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def ratio(y, ref, bound):
    """worst |y - ref| / bound over all elements (0 / 0 = 0, x / 0 = inf, NaN = inf) and where"""
    d = (y.double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(d)
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))
    if r.numel() == 0:
        return 0.0, ()
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def hold(what, items, outs, worst=None):
    """every item against `outs`: the figures are printed before anything is asserted; `worst`
    collects, per output, max |y - ref| / bound (bitwise outputs: the number of differing elements)"""
    figures = []
    for name, ref, bound in items:
        y = outs[name]
        assert tuple(y.shape) == tuple(ref.shape), (what, name, tuple(y.shape), tuple(ref.shape))
        if bound is None:
            assert y.dtype == ref.dtype, (what, name, y.dtype, ref.dtype)
            bad = int((bits(y) != bits(ref)).sum())
            print(f"{what} {name}: {bad} of {y.numel()} elements differ bitwise")
            figures.append((name, float(bad), None, True))
        else:
            r, where = ratio(y, ref, bound)
            print(f"{what} {name}: worst |y - ref| / bound {r:.3f} at {where}")
            figures.append((name, r, where, False))
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), figures[-1][1])
    for name, r, where, bitwise in figures:
        if bitwise:
            assert r == 0, (what, name, "bitwise", r)
        else:
            assert r <= 1.0, (what, name, "bound", r, where)


def passes(what, items, outs):
    try:
        hold(what, items, outs)
    except AssertionError:
        return False
    return True


def old_rel_err(y, ref):
    """the norm-wise criterion of test_gpu_kernels.py (helpers.rel_err)"""
    return float((y.double() - ref.double()).norm() / ref.double().norm().clamp(min=1e-30))


# ----------------------------------------------------------------------------- resampling
def lerp(n_in, n_out, fused=True):
    """(i0, i1, l0, l1) of every output index: the header's formula in f32, scale (dst + .5) - .5 as
    ONE fused multiply-add (the exact f32 x f32 product and the subtraction in fp64, rounded to f32
    once), every other step a torch op in f32.  fused=False rounds the product on its own, for the
    CPU test that shows the difference."""
    scale = torch.tensor(float(n_in), dtype=F32) / torch.tensor(float(n_out), dtype=F32)
    dst = torch.arange(n_out, dtype=F32)
    if fused:
        src = (scale.double() * (dst + 0.5).double() - 0.5).to(F32).clamp(min=0)
    else:
        src = (scale * (dst + 0.5) - 0.5).clamp(min=0)
    i0 = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(F32)
    l0 = 1 - l1
    assert scale.dtype == dst.dtype == src.dtype == l1.dtype == l0.dtype == F32
    return i0, i1, l0, l1


def lerp_matrix(n_in, n_out, fused=True):
    """(n_out, n_in) fp64: l0 at i0 plus l1 at i1, the f32 weights exactly"""
    i0, i1, l0, l1 = lerp(n_in, n_out, fused)
    W = torch.zeros(n_out, n_in, dtype=torch.float64)
    rows = torch.arange(n_out)
    W.index_put_((rows, i0), l0.double(), accumulate=True)
    W.index_put_((rows, i1), l1.double(), accumulate=True)
    return W


def touch(W):
    """the largest number of outputs that touch one source element"""
    return int((W != 0).sum(0).max())


def resize_ref(x, Ho, Wo):
    """x (N, Hi, Wi) -> ref, absacc (N, Ho, Wo) in fp64"""
    Wy, Wx = lerp_matrix(x.shape[1], Ho), lerp_matrix(x.shape[2], Wo)
    x = x.double()
    return Wy @ x @ Wx.t(), Wy.abs() @ x.abs() @ Wx.abs().t()


def resize_grad_ref(g, Hi, Wi):
    """g (N, Ho, Wo) -> ref, absacc (N, Hi, Wi) in fp64, and T"""
    Wy, Wx = lerp_matrix(Hi, g.shape[1]), lerp_matrix(Wi, g.shape[2])
    g = g.double()
    return Wy.t() @ g @ Wx, Wy.abs().t() @ g.abs() @ Wx.abs(), touch(Wy) * touch(Wx)


def emu_resize(x, Ho, Wo):
    """the kernels' gather form in f32: ly.l0 (lx.l0 v00 + lx.l1 v01) + ly.l1 (lx.l0 v10 + lx.l1 v11)"""
    y0, y1, ly0, ly1 = lerp(x.shape[1], Ho)
    x0, x1, lx0, lx1 = lerp(x.shape[2], Wo)
    x = x.float()
    top = lx0 * x[:, y0][:, :, x0] + lx1 * x[:, y0][:, :, x1]
    bot = lx0 * x[:, y1][:, :, x0] + lx1 * x[:, y1][:, :, x1]
    return ly0[:, None] * top + ly1[:, None] * bot


def emu_resize_grad(g, Hi, Wi):
    """two f32 passes (over x, then over y) with the f32 weights"""
    Wy, Wx = lerp_matrix(Hi, g.shape[1]).float(), lerp_matrix(Wi, g.shape[2]).float()
    return Wy.t() @ (g.float() @ Wx)


GEOMETRIES = [((3, 5), (7, 1028)), ((4, 6), (5, 1027)), ((7, 9), (20, 13)), ((10, 10), (5, 7)), ((1, 1), (3, 4)),
              ((5, 4), (5, 4)), ((2, 3), (1, 1))]


def bilinear_fwd_cases():
    return [dict(NC=nc, i=i, o=o, idt=idt, odt=odt) for (i, o) in GEOMETRIES for nc in (1, 3)
            for idt, odt in ((F32, F32), (BF16, BF16), (F16, F32))]


def bilinear_fwd_inputs(c):
    g = gen(11 + 7 * c["NC"] + c["i"][0] + 3 * c["o"][1])
    return {"x": randn(g, c["NC"], *c["i"]).to(c["idt"])}


def bilinear_fwd_emulate(c, inp):
    return {"out": emu_resize(inp["x"], *c["o"]).to(c["odt"])}


def bilinear_fwd_refs(c, inp, outs):
    if c["i"] == c["o"]:  # the identity: exact
        return [("out", inp["x"].to(c["odt"]), None)]
    ref, absacc = resize_ref(inp["x"], *c["o"])
    return [("out", ref, rounding(c["odt"], ref) + (4 + 4) * U * absacc)]


def bilinear_bwd_cases():
    return [dict(NC=nc, i=i, o=o, gdt=gdt) for (i, o) in GEOMETRIES + [((1, 1), (64, 64))] for nc in (1, 3)
            for gdt in (F32, BF16)]


def bilinear_bwd_inputs(c):
    g = gen(13 + 7 * c["NC"] + c["i"][0] + 3 * c["o"][1])
    return {"dout": randn(g, c["NC"], *c["o"]).to(c["gdt"])}


def bilinear_bwd_emulate(c, inp):
    return {"din": emu_resize_grad(inp["dout"], *c["i"])}


def bilinear_bwd_refs(c, inp, outs):
    ref, absacc, T = resize_grad_ref(inp["dout"], *c["i"])
    return [("din", ref, eps_of(F32) * ref.abs() + (T + 4) * U * absacc)]


def pos_interp_cases():
    return [dict(g=g, C=C, H=H, W=W) for g in (1, 2, 7) for C in (4, 20)
            for H, W in ((1, 1), (3, 5), (16, 9), (5, 14))]


def pos_interp_inputs(c):
    g = gen(17 + c["g"] + 5 * c["C"] + 11 * c["H"])
    return {"pos": randn(g, c["g"] ** 2 + 1, c["C"]), "dout": randn(g, c["H"] * c["W"] + 1, c["C"]),
            "dpos0": randn(g, c["g"] ** 2 + 1, c["C"])}


def _planes(rows, h, w):
    """(h w, C) channels-last rows -> (C, h, w)"""
    return rows.t().reshape(rows.shape[1], h, w)


def _rows(planes):
    return planes.reshape(planes.shape[0], -1).t()


def pos_interp_emulate(c, inp):
    g, H, W = c["g"], c["H"], c["W"]
    out = torch.cat([inp["pos"][:1], _rows(emu_resize(_planes(inp["pos"][1:], g, g), H, W))])
    grad = torch.cat([inp["dout"][:1], _rows(emu_resize_grad(_planes(inp["dout"][1:], H, W), g, g))])
    return {"out": out.contiguous(), "dpos": inp["dpos0"] + grad}


def pos_interp_refs(c, inp, outs):
    g, H, W = c["g"], c["H"], c["W"]
    ref, absacc = resize_ref(_planes(inp["pos"][1:], g, g), H, W)
    gref, gabs, T = resize_grad_ref(_planes(inp["dout"][1:], H, W), g, g)
    init = inp["dpos0"].double()
    dref = init + torch.cat([inp["dout"][:1].double(), _rows(gref)])
    dabs = init.abs() + torch.cat([inp["dout"][:1].double().abs(), _rows(gabs)])
    return [("out[0]", inp["pos"][0], None),
            ("out", _rows(ref), eps_of(F32) * _rows(ref).abs() + (4 + 4) * U * _rows(absacc)),
            ("dpos", dref, eps_of(F32) * dref.abs() + (T + 4 + 1) * U * dabs)]


def pos_interp_split(outs):
    """the names the items refer to, from the entry points' two outputs"""
    return {"out[0]": outs["out"][0], "out": outs["out"][1:], "dpos": outs["dpos"]}


def score_concat_cases():
    shapes = [(1, 1, 1, 8, 1, 1, 1), (2, 7, 9, 72, 19, 13, 5), (2, 12, 20, 64, 64, 6, 10)]
    return [dict(B=B, h=h, w=w, C=C, K=K, hs=hs, ws=ws, dt=dt, token=token)
            for (B, h, w, C, K, hs, ws) in shapes for dt in LOW for token in (False, True)]


def score_concat_inputs(c):
    g = gen(19 + c["h"] + 3 * c["K"])
    return {"rows": randn(g, c["B"], c["h"] * c["w"], c["C"]).to(c["dt"]),
            "score": randn(g, c["B"], c["K"], c["hs"], c["ws"])}


def score_concat_emulate(c, inp):
    B, K, h, w = c["B"], c["K"], c["h"], c["w"]
    s = emu_resize(inp["score"].reshape(B * K, c["hs"], c["ws"]), h, w).reshape(B, K, h * w).transpose(1, 2)
    return {"out": torch.cat([inp["rows"], s.to(c["dt"])], 2).reshape(B * h * w, -1)}


def score_concat_refs(c, inp, outs):
    B, K, h, w = c["B"], c["K"], c["h"], c["w"]
    ref, absacc = resize_ref(inp["score"].reshape(B * K, c["hs"], c["ws"]), h, w)
    ref = ref.reshape(B, K, h * w).transpose(1, 2).reshape(B * h * w, K)
    absacc = absacc.reshape(B, K, h * w).transpose(1, 2).reshape(B * h * w, K)
    return [("copied", inp["rows"].reshape(B * h * w, -1), None),
            ("score", ref, rounding(c["dt"], ref) + (4 + 4) * U * absacc)]


def score_concat_split(c, outs):
    return {"copied": outs["out"][:, :c["C"]], "score": outs["out"][:, c["C"]:]}


# ----------------------------------------------------------------------------- layout ops
def im2col_cases():
    geo = [dict(B=2, Cin=3, Hin=9, Win=14, p=4, ldo=64),     # vector path, floor grid 2 x 3, K = 48 padded
           dict(B=2, Cin=3, Hin=30, Win=45, p=14, ldo=640),  # K = 588 padded
           dict(B=2, Cin=3, Hin=7, Win=10, p=3, ldo=28),     # K = 27 rounded up to 4
           dict(B=2, Cin=3, Hin=8, Win=12, p=4, ldo=48)]     # gw * p == Win: the last patch ends the image
    return [dict(g, idt=idt, odt=odt) for g in geo for idt, odt in ((F32, BF16), (BF16, BF16), (F32, F32))]


def im2col_inputs(c):
    img = randn(gen(23 + c["p"] + c["Win"]), c["B"], c["Cin"], c["Hin"], c["Win"]).to(c["idt"])
    gh, gw = c["Hin"] // c["p"], c["Win"] // c["p"]
    img[:, :, gh * c["p"]:] = float("nan")  # the pixels beyond the floor grid are not read
    img[:, :, :, gw * c["p"]:] = float("nan")
    return {"img": img}


def im2col_emulate(c, inp):
    B, Cin, p = c["B"], c["Cin"], c["p"]
    gh, gw = c["Hin"] // p, c["Win"] // p
    x = inp["img"][:, :, :gh * p, :gw * p].reshape(B, Cin, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5)
    out = torch.zeros(B * gh * gw, c["ldo"], dtype=c["odt"])
    out[:, :Cin * p * p] = x.reshape(B * gh * gw, Cin * p * p).float().to(c["odt"])
    return {"out": out}


def im2col_refs(c, inp, outs):
    return [("out", im2col_emulate(c, inp)["out"], None)]


def tokens_cases():
    cases = [dict(B=B, P=Pn, C=C, dt=dt, null=None, ptr=(i + j) % 2 == 1)
             for i, (B, Pn, C) in enumerate(((1, 1, 4), (3, 5, 20), (2, 64, 768))) for j, dt in enumerate((F32, F16, BF16))]
    return cases + [dict(B=3, P=5, C=20, dt=BF16, null=n, ptr=False) for n in ("dcls", "dpos", "dpatch")]


TOKENS_SCALE, TOKENS_SCALE_PTR = 0.5, 0.125  # both powers of two: their f32 product is exact


def tokens_inputs(c):
    B, Pn, C = c["B"], c["P"], c["C"]
    g = gen(29 + B + 3 * Pn + C)
    return {"patch": randn(g, B * Pn, C).to(c["dt"]), "cls": randn(g, C), "pos": randn(g, Pn + 1, C),
            "dx": randn(g, B, Pn + 1, C), "dcls0": randn(g, C), "dpos0": randn(g, Pn + 1, C)}


def tokens_scale(c):
    return TOKENS_SCALE * (TOKENS_SCALE_PTR if c["ptr"] else 1.0)


def tokens_emulate(c, inp):
    B, Pn, C = c["B"], c["P"], c["C"]
    x = torch.cat([inp["cls"].expand(B, 1, C), inp["patch"].float().reshape(B, Pn, C)], 1) + inp["pos"]
    outs = {"x": x.reshape(B * (Pn + 1), C)}
    acc = torch.zeros(Pn + 1, C)
    for b in range(B):
        acc = acc + inp["dx"][b]
    if c["null"] != "dpatch":
        outs["dpatch"] = (inp["dx"][:, 1:] * torch.tensor(tokens_scale(c), dtype=F32)).to(c["dt"]).reshape(B * Pn, C)
    if c["null"] != "dcls":
        outs["dcls"] = inp["dcls0"] + acc[0]
    if c["null"] != "dpos":
        outs["dpos"] = inp["dpos0"] + acc
    return outs


def tokens_refs(c, inp, outs):
    B = c["B"]
    emu = tokens_emulate(c, inp)
    items = [("x", emu["x"], None)]
    if c["null"] != "dpatch":
        items.append(("dpatch", emu["dpatch"], None))
    s, a = inp["dx"].double().sum(0), inp["dx"].double().abs().sum(0)
    if c["null"] != "dcls":
        i0 = inp["dcls0"].double()
        items.append(("dcls", i0 + s[0], (B + 2) * U * (i0.abs() + a[0])))
    if c["null"] != "dpos":
        i0 = inp["dpos0"].double()
        items.append(("dpos", i0 + s, (B + 2) * U * (i0.abs() + a)))
    return items


def transpose_cases():
    def case(rows, cols, idt, odt, rows_pad=None, r0=0, batch=1, acc=0, colsum=False, in_gap=0, out_gap=0,
             bgap=0, fast=False, random=False):
        return dict(rows=rows, cols=cols, idt=idt, odt=odt, rows_pad=rows_pad or rows, r0=r0, batch=batch, acc=acc,
                    colsum=colsum, in_ld=cols + in_gap, out_ld=(rows_pad or rows) + out_gap, bgap=bgap, fast=fast,
                    random=random)

    return [case(1, 1, F32, BF16),
            case(65, 63, BF16, BF16, colsum=True, in_gap=9, out_gap=5),
            case(65, 63, F32, F16, in_gap=1, out_gap=3),
            # one row block, one batch: a single atomic add per column, so inexact sums repeat bit for bit
            case(60, 70, F32, BF16, colsum=True, in_gap=2, out_gap=4, random=True),
            case(300, 72, F32, F16, rows_pad=384, colsum=True, in_gap=8),
            case(64, 64, BF16, F32, r0=3, batch=3, colsum=True, in_gap=8, out_gap=8, bgap=40),
            case(65, 63, F16, F32, batch=2, acc=1, colsum=True, in_gap=1, out_gap=3, bgap=7),
            case(64, 128, F32, BF16, in_gap=4, out_gap=8, fast=True),
            case(128, 64, F32, F16, in_gap=4, out_gap=8, fast=True),
            case(64, 128, F32, BF16, in_gap=4, out_gap=6)]  # out_ld % 8 != 0: the generic kernel, the same values


def transpose_inputs(c):
    g = gen(31 + c["rows"] + c["cols"] + c["batch"])
    # colsum over several row blocks or batches: exact sums, so that the float atomics' order cannot
    # show between run_poisoned's two runs
    assert not c["random"] or (c["rows"] <= 64 and c["batch"] == 1)
    make = dyadic if c["colsum"] and not c["random"] else randn
    x = make(g, c["batch"], c["rows"], c["cols"]).to(c["idt"])
    return {"in": x, "out0": randn(g, c["batch"], c["cols"], c["rows_pad"]),
            "colsum0": (randn if c["random"] else dyadic)(g, c["cols"])}


def transpose_emulate(c, inp):
    out = torch.zeros(c["batch"], c["cols"], c["rows_pad"], dtype=c["odt"])
    t = inp["in"].float().transpose(1, 2)
    if c["acc"]:
        assert c["rows_pad"] == c["rows"]
        out = inp["out0"] + t
    else:
        out[:, :, :c["rows"]] = t.to(c["odt"])
    outs = {"out": out}
    if c["colsum"]:
        outs["colsum"] = inp["colsum0"] + inp["in"].float().sum((0, 1))
    return outs


def transpose_refs(c, inp, outs):
    items = [("out", transpose_emulate(c, inp)["out"], None)]
    if c["colsum"]:
        i0, x = inp["colsum0"].double(), inp["in"].double()
        items.append(("colsum", i0 + x.sum((0, 1)), (c["batch"] * c["rows"] + 2) * U * (i0.abs() + x.abs().sum((0, 1)))))
    return items


# 65536 workgroups x 256 threads x 4 elements = 2^26 elements per pass of cast_kernel's grid-stride
# loop: a second iteration needs n > 2^26, at least 2 x 2 x 2^26 bytes = 256 MiB of 16-bit buffers,
# above the 64 MiB this suite allows one test.  The largest n stays 262147.
CAST_SECOND_PASS_N = 65536 * 256 * 4 + 1
CAST_SCALES = ("one", "pow2_ptr", "0.37")


def cast_cases():
    return ([dict(n=n, idt=F32, odt=BF16, scale=CAST_SCALES[i % 3]) for i, n in enumerate((1, 3, 4, 262147))]
            + [dict(n=n, idt=F16, odt=F32, scale=CAST_SCALES[(i + 1) % 3]) for i, n in enumerate((1, 3, 4, 262147))]
            + [dict(n=1023, idt=idt, odt=odt, scale=s) for idt in (F32, F16, BF16) for odt in (F32, F16, BF16)
               for s in CAST_SCALES])


def cast_scale(c):
    """(the scale argument, *scale_ptr or None)"""
    return {"one": (1.0, None), "pow2_ptr": (2.0, 2.0 ** -7), "0.37": (0.37, None)}[c["scale"]]


def cast_inputs(c):
    return {"in": (randn(gen(37 + c["n"]), c["n"]) * 3).to(c["idt"])}


def cast_emulate(c, inp):
    s, sp = cast_scale(c)
    scale = torch.tensor(s, dtype=F32) * (torch.tensor(sp, dtype=F32) if sp is not None else 1)
    return {"out": (inp["in"].float() * scale).to(c["odt"])}


def cast_refs(c, inp, outs):
    return [("out", cast_emulate(c, inp)["out"], None)]


# ----------------------------------------------------------------------------- reductions
def row_mean_cases():
    return [dict(B=B, rows=rows, C=C, dt=dt, token=token)
            for (B, rows, C) in ((1, 1, 8), (2, 127, 768), (2, 129, 2048), (3, 300, 64)) for dt in LOW
            for token in (False, True)]


def row_mean_inputs(c):
    return {"x": (randn(gen(41 + c["rows"]), c["B"], c["rows"], c["C"]) + 0.25).to(c["dt"])}


def row_mean_emulate(c, inp):
    return {"out": inp["x"].float().sum(1) / c["rows"]}


def row_mean_refs(c, inp, outs):
    x = inp["x"].double()
    return [("out", x.mean(1), (c["rows"] + 4) * U * x.abs().mean(1))]


SCORE_EPS = 1e-12  # F.normalize's default


def score_map_cases():
    return [dict(B=B, HW=HW, C=C, K=K, dt=dt, token=token, zeros=(HW == 33))
            for (B, HW, C, K) in ((1, 1, 16, 1), (2, 33, 48, 19), (2, 31, 512, 32), (1, 64, 2048, 5)) for dt in LOW
            for token in (False, True)]


def score_map_inputs(c):
    g = gen(43 + c["HW"] + c["K"])
    v, t = randn(g, c["B"], c["HW"], c["C"]).to(c["dt"]), randn(g, c["B"], c["K"], c["C"])
    if c["zeros"]:
        v[1, 32] = 0  # the last pixel of a ragged group
        v[0, 7] = 0
        t[1, 3] = 0
    return {"v": v, "t": t}


def score_map_emulate(c, inp, raw_class=None):
    v, t = inp["v"].float(), inp["t"]
    tn = t * (1 / t.pow(2).sum(2, keepdim=True).sqrt().clamp(min=SCORE_EPS))
    if raw_class is not None:  # a planted defect: this class is not normalised
        tn[:, raw_class] = t[:, raw_class]
    tn = tn.to(c["dt"]).float()
    inv = 1 / v.pow(2).sum(2).sqrt().clamp(min=SCORE_EPS)
    return {"score": (tn @ v.transpose(1, 2)) * inv[:, None, :]}


def score_map_refs(c, inp, outs):
    v, t = inp["v"].double(), inp["t"].double()
    vn = v / v.norm(dim=2, keepdim=True).clamp(min=SCORE_EPS)
    tn = t / t.norm(dim=2, keepdim=True).clamp(min=SCORE_EPS)
    return [("score", tn @ vn.transpose(1, 2), (eps_of(c["dt"]) + (c["C"] + 8) * U) * (tn.abs() @ vn.abs().transpose(1, 2)))]


# ----------------------------------------------------------------------------- batch norm
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
BN_GSCALE = 2.0 ** -13


def bn_cases():
    shapes = [(1, 8, 8), (3, 8, 16), (37, 768, 776), (1030, 2048, 2048), (700, 64, 1536)]
    cases = [dict(rows=r, C=C, ld=ld, dt=dt, relu=relu, null=False, outlier=False)
             for (r, C, ld) in shapes for dt in LOW for relu in (0, 1)]
    cases += [dict(rows=37, C=768, ld=776, dt=BF16, relu=0, null=True, outlier=False)]
    cases += [dict(rows=700, C=64, ld=1536, dt=dt, relu=0, null=False, outlier=True) for dt in LOW]
    return cases


def _ulp16(x, dt):
    """the spacing of dt at |x| (f32)"""
    e = torch.floor(torch.log2(x.float().abs().clamp(min=2.0 ** -14)))
    return torch.pow(2.0, e - (P[dt] - 1))


def bn_mask_margin(x, sc, sh):
    """min over all elements of |x sc + sh| / (|x sc| + |sh|) in fp64 (1 where both are zero)"""
    a, b = x.double() * sc, sh.expand_as(x)
    den = a.abs() + b.abs()
    return torch.where(den == 0, torch.ones_like(den), (a + b).abs() / den)


def bn_stats64(x):
    x = x.double()
    mean = x.mean(0)
    var = (x - mean).pow(2).mean(0)
    return mean, var, 1 / torch.sqrt(var + float(torch.tensor(BN_EPS, dtype=F32)))


def bn_inputs(c):
    rows, C = c["rows"], c["C"]
    g = gen(47 + rows + C + 2 * c["relu"])
    x = randn(g, rows, C) * (0.5 + torch.rand(C, generator=g)) + randn(g, C) * 0.5
    if rows == 1:
        x = x * 2.0 ** -12  # mean = x and sh = b - x sc: keep |x sc| below |b|, so that y = b has an unambiguous sign
    if c["outlier"]:
        x[0] += 6 * x.std(0)  # row 0, the shift of the kernel's sums, 6 standard deviations out
    x = x.to(c["dt"])
    w = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    b = randn(g, C) * 0.5
    inp = {"w": None if c["null"] else w, "b": None if c["null"] else b,
           "rm0": None if c["null"] else randn(g, C) * 0.3, "rv0": None if c["null"] else 0.5 + torch.rand(C, generator=g),
           "dy": randn(g, rows, C).to(c["dt"]),
           "erm": randn(g, C) * 0.3, "erv": 0.5 + torch.rand(C, generator=g)}  # dclip_bn_eval's statistics
    if c["relu"]:
        # the backward recomputes the ReLU mask from x sc + sh in f32: move the few elements whose
        # sign is within reach of its rounding one 16-bit ulp at a time, away from the zero
        for _ in range(32):
            mean, var, rstd = bn_stats64(x)
            sc = w.double() * rstd
            sh = b.double() - mean * sc
            bad = bn_mask_margin(x, sc, sh) < 2.0 ** -9
            if not bool(bad.any()):
                break
            t = x.double() * sc + sh
            away = torch.where(t >= 0, 1.0, -1.0) * torch.where(sc >= 0, 1.0, -1.0)
            x = torch.where(bad, x.float() + away.float() * _ulp16(x, c["dt"]), x.float()).to(c["dt"])
    inp["x"] = x
    return inp


def _opt(t, fill, C):
    return torch.full((C,), fill) if t is None else t


def bn_emulate(c, inp, biased_running_var=False):
    rows, C, dt = c["rows"], c["C"], c["dt"]
    x = inp["x"].float()
    w, b = _opt(inp["w"], 1.0, C), _opt(inp["b"], 0.0, C)
    n = torch.tensor(float(rows), dtype=F32)
    eps, mom = torch.tensor(BN_EPS, dtype=F32), torch.tensor(BN_MOMENTUM, dtype=F32)
    d = x - x[0]
    S, Q = d.sum(0), (d * d).sum(0)
    md = S / n
    var = (Q / n - md * md).clamp(min=0)
    mu = x[0] + md
    rs = torch.rsqrt(var + eps)
    sc = w * rs
    sh = b - mu * sc
    y = x * sc + sh
    outs = {"mean": mu, "rstd": rs, "y": (y.clamp(min=0) if c["relu"] else y).to(dt)}
    if inp["rm0"] is not None:
        unb = var if (biased_running_var or rows == 1) else var * (n / (n - 1))
        outs["rm"] = (1 - mom) * inp["rm0"] + mom * mu
        outs["rv"] = (1 - mom) * inp["rv0"] + mom * unb
    esc = w / torch.sqrt(inp["erv"] + eps)
    ey = x * esc + (b - inp["erm"] * esc)
    outs["y_eval"] = (ey.clamp(min=0) if c["relu"] else ey).to(dt)
    outs.update(bn_bwd_emulate(c, inp, mu, rs))
    return outs


def bn_bwd_emulate(c, inp, mean, rstd):
    """dclip_bn_bwd in f32 from the given mean / rstd"""
    rows, C, dt = c["rows"], c["C"], c["dt"]
    x, dy = inp["x"].float(), inp["dy"].float()
    w, b = _opt(inp["w"], 1.0, C), _opt(inp["b"], 0.0, C)
    n = torch.tensor(float(rows), dtype=F32)
    g = dy
    if c["relu"]:
        sc = w * rstd
        g = torch.where(x * sc + (b - mean * sc) > 0, dy, torch.zeros_like(dy))
    S, Q = g.sum(0), (g * (x - mean)).sum(0)
    ga = BN_GSCALE if c["relu"] else 1.0
    k1 = w * rstd
    k2 = -w * rstd * rstd * rstd * (Q / n)
    k3 = -k1 * (S / n) - k2 * mean
    outs = {"dx": (g * k1 + x * k2 + k3).to(dt)}
    if not c["null"]:
        outs["dw"], outs["db"] = Q * rstd * ga, S * ga
    return outs


def bn_refs(c, inp, outs):
    """The forward's statistics, per channel, n = rows, x0 = row 0, d = x - x0 (one rounding: both
    are 16-bit), S = sum d, Q = sum d^2 in fp64:
        eS = (n + 2) u sum|d|                  d's rounding, any summation order
        eQ = (n + 4) u Q                       d's rounding twice, the square, any order
        e_md = eS / n + u |md|                 md = S / n
        e_mean = e_md + u |mean|               mean = x0 + md
        e_var = eQ / n + 2 |md| e_md + e_md^2 + 3 u (Q / n + md^2)     var = Q / n - md^2
        e_rstd = e_var / (2 (var + eps - e_var)^1.5) + 4 u rstd        the add, rsqrt to 1 ulp
        e_rm = m e_mean + 4 u ((1 - m)|rm0| + m |mean|)
        e_rv = m n / (n - 1) (e_var + 2 u var) + 4 u ((1 - m)|rv0| + m var n / (n - 1))
    The maps: sc = w rstd, sh = b - mean sc, y = x sc + sh rounded to dt:
        e_sc = |w| e_rstd + u |sc|,  e_sh = |mean| e_sc + |sc| e_mean + 2 u |mean sc| + u |sh|
        e_y = 2^-p |y| + |x| e_sc + e_sh + 2 u (|x sc| + |sh|)         (ReLU is 1-Lipschitz)
    dclip_bn_eval: the same with e_mean = 0 and e_sc = 4 u |sc| (add, sqrt, division).
    The backward, from the mean / rstd it was given (those the forward wrote, taken as exact), g =
    dy masked where x sc + sh <= 0 (asserted unambiguous), S = sum g, Q = sum g (x - mean):
        db = S ga, dw = Q rstd ga:  (n + 4) u sum|g| ga,  (n + 4) u sum|g (x - mean)| rstd ga
        k1 = w rstd, k2 = -w rstd^3 Q / n, k3 = -k1 S / n - k2 mean, dx = k1 g + k2 x + k3:
        e_k1 = u |k1|, e_k2 = |w| rstd^3 eQ / n + 5 u |k2|  (eQ = (n + 3) u sum|g (x - mean)|),
        e_k3 = |k1| eS / n + |mean| e_k2 + 4 u (|k1 S / n| + |k2 mean|)  (eS = (n + 2) u sum|g|),
        e_dx = 2^-p |dx| + |g| e_k1 + |x| e_k2 + e_k3 + 3 u (|k1 g| + |k2 x| + |k3|)"""
    rows, C, dt = c["rows"], c["C"], c["dt"]
    x, dy = inp["x"].double(), inp["dy"].double()
    w, b = _opt(inp["w"], 1.0, C).double(), _opt(inp["b"], 0.0, C).double()
    n = float(rows)
    eps, m = float(torch.tensor(BN_EPS, dtype=F32)), float(torch.tensor(BN_MOMENTUM, dtype=F32))
    mean, var, rstd = bn_stats64(x)
    d = x - x[0]
    S, Q = d.sum(0), d.pow(2).sum(0)
    md = S / n
    eS, eQ = (n + 2) * U * d.abs().sum(0), (n + 4) * U * Q
    e_md = eS / n + U * md.abs()
    e_mean = e_md + U * mean.abs()
    e_var = eQ / n + 2 * md.abs() * e_md + e_md ** 2 + 3 * U * (Q / n + md ** 2)
    assert bool((e_var < 0.5 * (var + eps)).all())
    e_rstd = e_var / (2 * (var + eps - e_var).pow(1.5)) + 4 * U * rstd
    items = [("mean", mean, e_mean), ("rstd", rstd, e_rstd)]
    if inp["rm0"] is not None:
        unb = var * (n / (n - 1)) if rows > 1 else var
        f = n / (n - 1) if rows > 1 else 1.0
        rm0, rv0 = inp["rm0"].double(), inp["rv0"].double()
        items.append(("rm", (1 - m) * rm0 + m * mean, m * e_mean + 4 * U * ((1 - m) * rm0.abs() + m * mean.abs())))
        items.append(("rv", (1 - m) * rv0 + m * unb, m * f * (e_var + 2 * U * var) + 4 * U * ((1 - m) * rv0.abs() + m * unb)))

    def affine(sc, e_sc, mu, e_mu):
        sh = b - mu * sc
        e_sh = mu.abs() * e_sc + sc.abs() * e_mu + 2 * U * (mu * sc).abs() + U * sh.abs()
        y = x * sc + sh
        e_y = x.abs() * e_sc + e_sh + 2 * U * ((x * sc).abs() + sh.abs())
        if c["relu"]:
            y = y.clamp(min=0)
        return y, rounding(dt, y) + e_y

    sc = w * rstd
    items.append(("y",) + affine(sc, w.abs() * e_rstd + U * sc.abs(), mean, e_mean))
    erm, erv = inp["erm"].double(), inp["erv"].double()
    esc = w / torch.sqrt(erv + eps)
    items.append(("y_eval",) + affine(esc, 4 * U * esc.abs(), erm, torch.zeros_like(erm)))

    # the backward, judged on its own: from the mean / rstd the forward under test wrote
    mu, rs = outs["mean"].double(), outs["rstd"].double()
    g = dy
    if c["relu"]:
        ksc = w * rs
        ksh = b - mu * ksc
        margin = bn_mask_margin(x, ksc, ksh)
        assert float(margin.min()) >= 2.0 ** -10, ("ambiguous ReLU mask", float(margin.min()))
        g = torch.where(x * ksc + ksh > 0, dy, torch.zeros_like(dy))
    ga = BN_GSCALE if c["relu"] else 1.0
    xc = x - mu
    S, Q = g.sum(0), (g * xc).sum(0)
    aS, aQ = g.abs().sum(0), (g * xc).abs().sum(0)
    if not c["null"]:
        items.append(("dw", Q * rs * ga, (n + 4) * U * aQ * rs * ga))
        items.append(("db", S * ga, (n + 4) * U * aS * ga))
    eS, eQ = (n + 2) * U * aS, (n + 3) * U * aQ
    k1 = w * rs
    k2 = -w * rs.pow(3) * (Q / n)
    k3 = -k1 * (S / n) - k2 * mu
    e_k1 = U * k1.abs()
    e_k2 = w.abs() * rs.pow(3) * eQ / n + 5 * U * k2.abs()
    e_k3 = k1.abs() * eS / n + mu.abs() * e_k2 + 4 * U * ((k1 * S / n).abs() + (k2 * mu).abs())
    dx = k1 * g + k2 * x + k3
    e_dx = rounding(dt, dx) + g.abs() * e_k1 + x.abs() * e_k2 + e_k3 + 3 * U * ((k1 * g).abs() + (k2 * x).abs() + k3.abs())
    items.append(("dx", dx, e_dx))
    return items


def _same(c, outs):
    return outs


FAMILIES = {
    "bilinear_fwd": (bilinear_fwd_cases, bilinear_fwd_inputs, bilinear_fwd_emulate, bilinear_fwd_refs, _same),
    "bilinear_bwd": (bilinear_bwd_cases, bilinear_bwd_inputs, bilinear_bwd_emulate, bilinear_bwd_refs, _same),
    "pos_interp": (pos_interp_cases, pos_interp_inputs, pos_interp_emulate, pos_interp_refs,
                   lambda c, outs: pos_interp_split(outs)),
    "score_concat": (score_concat_cases, score_concat_inputs, score_concat_emulate, score_concat_refs, score_concat_split),
    "im2col": (im2col_cases, im2col_inputs, im2col_emulate, im2col_refs, _same),
    "tokens": (tokens_cases, tokens_inputs, tokens_emulate, tokens_refs, _same),
    "transpose": (transpose_cases, transpose_inputs, transpose_emulate, transpose_refs, _same),
    "cast": (cast_cases, cast_inputs, cast_emulate, cast_refs, _same),
    "row_mean": (row_mean_cases, row_mean_inputs, row_mean_emulate, row_mean_refs, _same),
    "score_map": (score_map_cases, score_map_inputs, score_map_emulate, score_map_refs, _same),
    "bn": (bn_cases, bn_inputs, bn_emulate, bn_refs, _same),
}


def case_id(c):
    def s(v):
        if isinstance(v, torch.dtype):
            return NAME[v]
        if isinstance(v, tuple):
            return "x".join(str(e) for e in v)
        return str(v)
    return "-".join(f"{k}{s(v)}" for k, v in c.items() if v not in (None, False, 0) or k in ("relu",))


def dtype_key(c):
    """the dtypes of a case, for the per-entry-point report"""
    return "/".join(NAME[v] for v in c.values() if isinstance(v, torch.dtype)) or "f32"


def check_case(family, c, inp, outs, worst=None):
    """hold the outputs of one case (by the entry points' names) to the family's items"""
    _, _, _, refs, split = FAMILIES[family]
    hold(f"{family} {case_id(c)}", refs(c, inp, outs), split(c, outs), worst)
