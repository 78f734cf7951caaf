"""The cases, references, bounds and plain-torch emulations of test_gpu_norm_contract.py: every entry
point of csrc/layernorm.hip and the fp16 gradient-scale entry points of csrc/misc.hip
(dclip_grad_scale, dclip_add_readout_cast / _amax / _cast_scaled, dclip_row_scale_add), on CPU
tensors, so that the emulation goes through the very same checker
(test_norm_contract_emulation_cpu.py) before any kernel does.  Conventions of misc_check.py: every
reference in fp64 from the operands as rounded to their storage dtype, p = 11 / 8 / 24, u = 2^-24, no
share of elements ever excluded, an item of refs() is (output name, reference, bound), bound None
means bitwise.  FAMILIES[name] = (cases, inputs, emulate, refs, split) as there; the families in
SEQUENCES are driven through run_sequence(): uses 1 .. 5 of ONE delayed-scale state.

All bounds are first-order in u with the products of two error terms covered by counting one more
rounding than occurs; n = cols, sums "in any order" cost (n - 1) u sum|terms| (the kernels' row sums
are lane-serial over n / 64 values and six butterfly levels: depth n / 64 + 6, which this does not
pin).  A contraction of a + b s into one FMA removes a rounding: every bound is that of the unfused form.

forward    x in fp64, mu = mean x, var = mean (x - mu)^2, v = var + eps, r = v^-1/2:
             e_mu = (n + 2) u mean|x|          the sum in any order, 1 / n rounded, the product
             e_v  = (n + 5) u var + e_mu^2 + u v
                    sum (x - mu^)^2 = n var + n (mu - mu^)^2 exactly, so the mean's error enters
                    squared; d = x - mu^ is rounded (2 u on d^2), the square (1), the sum in any
                    order (n - 1), 1 / n and its product (2), one more for the second-order terms:
                    n + 5; the addition of eps u v
             e_r  = e_v / (2 (v - e_v)^1.5) + RSQRT_U u r      (asserted: e_v < v / 2)
             e_y  = 2^-p |y| + |w| ((r + e_r) e_mu + |x - mu| e_r) + 4 u (|(x - mu) r w| + |b|)
                    (the subtraction, two products, the addition: 4)
           rsqrtf: no accuracy statement for it is installed with the device library here, so, as
           the contract demands then, torch.rsqrt (f32, CPU) was measured against fp64 over 6e6
           arguments in [1e-13, 1e6]: 1.50 u at worst (test_rsqrt_allowance_was_measured repeats
           it); the GPU is given twice that, RSQRT_U = 3.  A constant row has var = 0, y = b within
           |w| r e_mu, rstd = eps^-1/2 within e_r.
backward   from the f32 mean / rstd it is given (those the forward wrote: taken as exact, the
           dclip_bn_bwd convention), x^ = (x - mean) rstd, dy' = dy (*dy_scale) with the rows r %
           dy_ntok == 0 as 0 (*dy_scale is a power of two here, asserted: dy' is exact), g = dy' w:
             e_mg  = (n + 2) u mean|g|          g's rounding, the sum, 1 / n and its product
             e_mgx = (n + 5) u mean|g x^|       x^: 2, g: 1, the product, the sum, 1 / n: n + 5
             A = rstd (|g| + |mg| + |x^ mgx|),  B = A + |res| + |add' add_scale|
             e_dx = 2^-24 |dx| + rstd (e_mg + |x^| e_mgx) + 8 u B
                    at most 5 roundings on the path of any of the three terms (x^ mgx: 2 + product +
                    subtraction + rstd), one for each of the two optional additions, one for add'
                    times add_scale: 8
             dw: (rows + 4) u (|init| + sum_r |dy' x^|), db: (rows + 4) u (|init| + sum_r |dy'|)
                    any order over the rows and the entry value (the atomic paths fix none), x^: 2,
                    the product: 1
bitwise    lp against (lp_dt) of the dx that was written, with a delayed scale (f16)(dx s), s a power
           of two; dclip_layernorm_bwd_add against dclip_layernorm_bwd_res + dclip_add_readout_cast
           and the second of two calls on the table path (GPU test); dclip_add_readout_cast's sum (one
           f32 addition: one possible result) and lp (scale a power of two); dclip_row_scale_add with
           s in {0, 1 / keep}, keep a power of two (the product is exact, so fused or not the sum is
           rounded once); every word of a scale state.
read-out   sum = a + b' bs (amax, cast_scaled):  2^-24 |sum| + 2 u (|a| + |b' bs|)
scale      s = 2^clamp(floor(log2(target / m)), -60, 60) in exact terms: m the largest |.| bit
           pattern of the f32 output the kernel ITSELF wrote (read back; a maximum is exact), the
           exponent by frexp of the fp64 quotient of two f32 values (which cannot round onto a power
           of two it does not equal); m = 0 or m >= 0x7f800000: s = 1 (dclip_grad_scale, _amax) or
           the scale the previous use used (delayed scale).  A delayed-scale state after use k: spair
           = (s, 1 / s), st[192 + k % 3] = s, the maximum over shards k % 3 = m (which shard a
           workgroup joins is not fixed), shards (k + 1) % 3 all zero, every other word unchanged.
"""
import math

import torch

from misc_check import (BF16, F16, F32, NAME, bits, case_id, dtype_key, eps_of, gen, hold, old_rel_err,  # noqa: F401
                        passes, randn, ratio, rounding)
from misc_check import U

RSQRT_U = 3.0            # twice the 1.50 u measured for torch.rsqrt on the CPU (see above)
RSQRT_CPU_MEASURED = 1.50  # torch 2.10 for ROCm 7.0, x86-64
RSQRT_CPU_MARGIN = 0.25    # what the CPU test lets another torch build differ by; the allowance does not move
LN_EPS = 1e-5            # the statistics the backward cases are fed
DY_SCALE = 2.0 ** -7
ADD_SCALE = 2.0 ** -9
TARGET = 256.0
S0 = 16.0                # the seed: st[0] = TARGET / S0, st[192] = S0
DS_SHARDS, DS_FLOATS = 64, 196
USES = (1, 2, 3, 4, 5)
USE_MULT = {1: 1.0, 2: 64.0, 3: 0.0, 4: 1.0, 5: 1.0}  # use 2: 2^6 times larger, use 3: all zero
INF_USE = 4              # this use's dy (LayerNorm) / a (read-out) holds one inf
SEQUENCES = ("ln_bwd_scaled", "readout_scaled")


def f32(v):
    return float(torch.tensor(v, dtype=F32))


def fbits(v):
    """the bit pattern of the f32 value v"""
    return int(torch.tensor([v], dtype=F32).view(torch.int32)[0])


def bfloat(b):
    return float(torch.tensor([b], dtype=torch.int32).view(F32)[0])


def maxbits(t):
    """the largest |.| bit pattern of an f32 tensor (0 when empty): NaN / inf sort above every finite value"""
    return int((bits(t.float()) & 0x7FFFFFFF).max()) if t.numel() else 0


def scale_exponent(target, m, nearest=False):
    """clamp(floor(log2(target / m)), -60, 60) of the bit pattern m, None when m is 0 or not finite"""
    if m == 0 or m >= 0x7F800000:
        return None
    q = f32(target) / bfloat(m)
    e = round(math.log2(q)) if nearest else math.frexp(q)[1] - 1
    return max(-60, min(60, e))


def pair_words(target, m):
    """dclip_grad_scale's ws after a call: (s, 1 / s, 0, 0) as int32 words"""
    e = scale_exponent(target, m) or 0
    return torch.tensor([fbits(2.0 ** e), fbits(2.0 ** -e), 0, 0], dtype=torch.int32)


def mask_rows(t, ntok):
    """t with the rows r % ntok == 0 as 0 (whatever they hold), ntok > 0"""
    drop = (torch.arange(t.shape[0]) % ntok == 0)[:, None]
    return torch.where(drop, torch.zeros_like(t), t)


def signed_weight(g, cols):
    return (0.5 + torch.rand(cols, generator=g)) * torch.where(torch.rand(cols, generator=g) < 0.25, -1.0, 1.0)


# ----------------------------------------------------------------------------- delayed scale
def ds_seed():
    st = torch.zeros(DS_FLOATS, dtype=torch.int32)
    st[0], st[3 * DS_SHARDS] = fbits(TARGET / S0), fbits(S0)
    return st


def ds_scale(st, use, nearest=False):
    """the scale use `use` casts with, from the state on entry"""
    row = (use + 2) % 3
    e = scale_exponent(TARGET, int(st[row * DS_SHARDS:(row + 1) * DS_SHARDS].max()), nearest)
    return bfloat(int(st[3 * DS_SHARDS + row])) if e is None else 2.0 ** e


def ds_apply(st, use, m, s=None, clear=True):
    """the state after use `use` joined the maximum m (into shard 0) having cast with s"""
    s = ds_scale(st, use) if s is None else s
    out = st.clone()
    if clear:
        out[((use + 1) % 3) * DS_SHARDS:((use + 1) % 3 + 1) * DS_SHARDS] = 0
    out[3 * DS_SHARDS + use % 3] = fbits(s)
    out[(use % 3) * DS_SHARDS] = max(int(out[(use % 3) * DS_SHARDS]), m)
    return out, torch.tensor([s, 1.0 / s], dtype=F32)


def ds_kept(use):
    """the words of a state use `use` must not change"""
    row = (use + 2) % 3
    return list(range(row * DS_SHARDS, (row + 1) * DS_SHARDS)) + [3 * DS_SHARDS + k for k in range(4) if k != use % 3]


def ds_items(st0, use, m):
    s = ds_scale(st0, use)
    cur = st0[(use % 3) * DS_SHARDS:(use % 3 + 1) * DS_SHARDS]
    return s, [("spair", torch.tensor([s, 1.0 / s], dtype=F32), None),
               ("st_used", torch.tensor([fbits(s)], dtype=torch.int32), None),
               ("st_max", torch.tensor([max(int(cur.max()), m)], dtype=torch.int32), None),
               ("st_cleared", torch.zeros(DS_SHARDS, dtype=torch.int32), None),
               ("st_kept", st0[ds_kept(use)], None)]


def ds_split(use, outs):
    st = outs["st"]
    return {"spair": outs["spair"], "st_used": st[3 * DS_SHARDS + use % 3].reshape(1),
            "st_max": st[(use % 3) * DS_SHARDS:(use % 3 + 1) * DS_SHARDS].max().reshape(1),
            "st_cleared": st[((use + 1) % 3) * DS_SHARDS:((use + 1) % 3 + 1) * DS_SHARDS], "st_kept": st[ds_kept(use)]}


def times(t, m):
    """t * m, and for m = 0 zeros of one sign: +0 (a product with 0 keeps the sign of its other factor)"""
    return torch.zeros_like(t) if m == 0 else t * m


def inf_row(c):
    return min(3, c["rows"] - 1)


def finite_rows(c, t):
    """t without the row that holds use INF_USE's inf"""
    if c.get("use") != INF_USE:
        return t
    keep = torch.arange(t.shape[0]) != inf_row(c)
    return t[keep]


def nonfinite_flag(c, t):
    """1 where the inf's row of t is not finite"""
    return (~torch.isfinite(t[inf_row(c)].float())).to(torch.uint8)


# ----------------------------------------------------------------------------- LayerNorm forward
def ln_fwd_cases():
    def case(rows, cols, xdt=F32, ydt=F32, data="centred", eps=1e-5, null=None):
        return dict(rows=rows, cols=cols, xdt=xdt, ydt=ydt, data=data, eps=eps, null=null)

    EPS, cs, k = (1e-5, 1e-12, 1e-2), [], 0
    shapes = [(r, c) for c in (4, 252, 260, 1028, 2044, 2048) for r in (1, 3, 5, 517)]  # ln_fwd_kernel
    shapes += [(r, c) for c in (512, 768, 1024) for r in (1, 7, 8197)]                  # ln_fwd_fast, wrapped walk
    for rows, cols in shapes:
        for ydt in (F32, BF16):
            cs.append(case(rows, cols, F32, ydt, ("centred", "offset")[(k // 2) % 2], EPS[k % 3]))
            k += 1
    for rows, cols in ((517, 260), (7, 768)):  # every x_dt x y_dt
        for xdt in (F32, F16, BF16):
            for ydt in (F32, F16, BF16):
                c = case(rows, cols, xdt, ydt, "offset", EPS[k % 3])
                k += 1
                if not any(all(o[f] == c[f] for f in c) for o in cs):
                    cs.append(c)
    for rows, cols in ((5, 260), (7, 768)):
        cs += [case(rows, cols, F32, BF16, "centred", 1e-5, null) for null in ("mean", "rstd")]
    return cs


def ln_fwd_inputs(c):
    rows, cols = c["rows"], c["cols"]
    g = gen(101 + rows + 3 * cols)
    x = randn(g, rows, cols)
    if c["data"] == "offset":
        x = x + 100.0  # every row 100 standard deviations from zero
    if rows >= 3:
        x[1] = 3 * 2.0 ** -12  # a constant row: var = 0
        x[2] = 0
    return {"x": x.to(c["xdt"]), "w": signed_weight(g, cols), "b": randn(g, cols) * 0.5}


def ln_fwd_emulate(c, inp, unbiased=False, no_eps=False):
    x, n = inp["x"].float(), c["cols"]
    mu = x.sum(1, keepdim=True) / n
    d = x - mu
    var = (d * d).sum(1, keepdim=True) / (n - 1 if unbiased else n)
    rs = torch.rsqrt(var if no_eps else var + torch.tensor(c["eps"], dtype=F32))
    outs = {"y": (d * rs * inp["w"] + inp["b"]).to(c["ydt"]), "mean": mu[:, 0].clone(), "rstd": rs[:, 0].clone()}
    if c["null"]:
        del outs[c["null"]]
    return outs


def ln_fwd_stats64(x, eps):
    x = x.double()
    mu = x.mean(1, keepdim=True)
    var = (x - mu).pow(2).mean(1, keepdim=True)
    return mu, var, (var + f32(eps)).rsqrt()


def ln_fwd_refs(c, inp, outs):
    x, w, b, n = inp["x"].double(), inp["w"].double(), inp["b"].double(), c["cols"]
    mu, var, r = ln_fwd_stats64(inp["x"], c["eps"])
    v, d = var + f32(c["eps"]), x - mu
    e_mu = (n + 2) * U * x.abs().mean(1, keepdim=True)
    e_v = (n + 5) * U * var + e_mu ** 2 + U * v
    assert bool((e_v < 0.5 * v).all()), "the variance's error is not small against var + eps: the case is ill-posed"
    e_r = e_v / (2 * (v - e_v).pow(1.5)) + RSQRT_U * U * r
    y = d * r * w + b
    e_y = rounding(c["ydt"], y) + w.abs() * ((r + e_r) * e_mu + d.abs() * e_r) + 4 * U * ((d * r * w).abs() + b.abs())
    items = [("y", y, e_y)]
    if c["null"] != "mean":
        items.append(("mean", mu[:, 0], e_mu[:, 0]))
    if c["null"] != "rstd":
        items.append(("rstd", r[:, 0], e_r[:, 0]))
    return items


# ----------------------------------------------------------------------------- LayerNorm backward
def bwd_ref(dyp, x, w, mu, rs, res, addt, dw0, db0):
    """fp64: (dx, e_dx, dw, e_dw, db, e_db); addt = add' add_scale or None, dw0 / db0 the entry values or None"""
    rows, n = x.shape
    mu, rs = mu.double()[:, None], rs.double()[:, None]
    xh, g = (x - mu) * rs, dyp * w
    mg, mgx = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = rs * (g - mg - xh * mgx)
    B = rs * (g.abs() + mg.abs() + (xh * mgx).abs())
    e = rs * ((n + 2) * U * g.abs().mean(1, keepdim=True) + xh.abs() * (n + 5) * U * (g * xh).abs().mean(1, keepdim=True))
    for t in (res, addt):
        if t is not None:
            dx, B = dx + t, B + t.abs()
    e_dx = eps_of(F32) * dx.abs() + e + 8 * U * B
    out = [dx, e_dx]
    for init, t in ((dw0, dyp * xh), (db0, dyp)):
        if init is None:
            out += [None, None]
        else:
            out += [init.double() + t.sum(0), (rows + 4) * U * (init.double().abs() + t.abs().sum(0))]
    return out


def bwd_emu(dyp, x, w, mu, rs, res, addt, dw0, db0, drop_mgx_row=None, dw_rows=None):
    """the kernels' arithmetic in f32 torch: (dx before res / add, dx, dw, db)"""
    n = x.shape[1]
    mu, rs = mu[:, None], rs[:, None]
    xh, g = (x - mu) * rs, dyp * w
    mg, mgx = g.sum(1, keepdim=True) / n, (g * xh).sum(1, keepdim=True) / n
    if drop_mgx_row is not None:  # a planted defect
        mgx[drop_mgx_row] = 0
    core = rs * (g - mg - xh * mgx)
    dx = core
    if res is not None:
        dx = dx + res
    if addt is not None:
        dx = dx + addt
    sel = slice(None) if dw_rows is None else dw_rows
    dw = None if dw0 is None else dw0 + (dyp * xh)[sel].sum(0)
    db = None if db0 is None else db0 + dyp.sum(0)
    return core, dx, dw, db


def ln_stats(x):
    """the f32 emulation's mean / rstd of x at LN_EPS (the GPU test replaces them by dclip_layernorm_fwd's)"""
    x = x.float()
    mu = x.sum(1, keepdim=True) / x.shape[1]
    d = x - mu
    return mu[:, 0].clone(), torch.rsqrt((d * d).sum(1) / x.shape[1] + torch.tensor(LN_EPS, dtype=F32))


def ln_bwd_cases():
    def case(rows, cols, dydt=F32, xdt=F32, res=None, lp=None, ws=True, null=None, dsc=False, ntok=0):
        fast = cols in (512, 768, 1024)
        if res in ("acc", "plain"):  # dclip_layernorm_bwd, accumulate = 1 / 0: no lp, no table, no dy_scale / dy_ntok
            lp, ws, dsc, ntok = None, False, False, 0
        if not fast:
            ws, dsc, ntok = False, False, 0
        if dsc:
            dydt = F16
        return dict(rows=rows, cols=cols, dydt=dydt, xdt=xdt, res=res, lp=lp, ws=ws, null=null, dsc=dsc, ntok=ntok)

    RES, LP, DT, NULL = (None, "sep", "alias", "acc"), (None, F16, BF16), (F32, F16, BF16), (None, "dw", None, "db", "both")
    cs = []
    shapes = [(r, c) for c in (4, 260, 2048) for r in (1, 5, 4101)]          # ln_bwd_kernel: 1024 blocks x 4 rows wrap
    shapes += [(r, c) for c in (512, 768, 1024) for r in (1, 7, 9, 4107)]    # ln_bwd_fast: 512 blocks x 8 rows wrap
    for i, (rows, cols) in enumerate(shapes):
        cs.append(case(rows, cols, DT[i % 3], DT[(i // 3) % 3], RES[i % 4], LP[(i + 1) % 3], ws=i % 2 == 0,
                       null=NULL[i % 5], dsc=i % 4 == 1, ntok=(0, 5, rows)[i % 3]))
    cs += [case(9, 768, F32, F32, "sep", BF16, ws=True, null="both"),         # the table is not touched
           case(4107, 512, BF16, F16, "alias", F16, ws=False),                # 512 atomic adds per address
           case(9, 512, F32, BF16, None, None, ws=True, null="dw"),
           case(9, 1024, F16, F32, "sep", F16, ws=True, null="db"),
           case(4107, 768, F16, F32, "sep", F16, ws=True, dsc=True, ntok=5),
           case(7, 1024, F32, F32, "alias", BF16, ws=True, ntok=7),           # dy_ntok = rows: only row 0 masked
           case(4101, 260, F16, BF16, "acc"),
           case(5, 260, F32, F16, "plain"),                                   # accumulate = 0: dx is written, never read
           case(9, 768, BF16, F32, "plain", null="db"),
           case(4107, 1024, F16, BF16, "plain"),
           case(5, 2048, BF16, F32, "alias", F16, null="db")]
    return cs


def ln_bwd_inputs(c):
    rows, cols = c["rows"], c["cols"]
    g = gen(211 + rows + 3 * cols + 7 * bool(c["dsc"]) + c["ntok"])
    x = (randn(g, rows, cols) + 0.3).to(c["xdt"])
    dy = randn(g, rows, cols)
    if c["dsc"]:
        dy = dy / DY_SCALE  # dy arrives on the scale 1 / *dy_scale
    dy = dy.to(c["dydt"])
    if c["ntok"]:
        dy[torch.arange(rows) % c["ntok"] == 0] = float("nan")  # masked rows are not to be read, or to be overwritten
    mean, rstd = ln_stats(x)
    return {"x": x, "dy": dy, "w": signed_weight(g, cols),
            "res": randn(g, rows, cols) if c["res"] not in (None, "plain") else None,
            "dw0": randn(g, cols), "db0": randn(g, cols), "mean": mean, "rstd": rstd}


def dy_prime(c, dy, scale=DY_SCALE):
    assert math.frexp(scale)[0] == 0.5  # a power of two: dy' is exact
    dyp = dy * scale if c.get("dsc") else dy
    return mask_rows(dyp, c["ntok"]) if c.get("ntok") and "adt" not in c else dyp


def inits(c, inp):
    return (None if c["null"] in ("dw", "both") else inp["dw0"]), (None if c["null"] in ("db", "both") else inp["db0"])


def ln_bwd_emulate(c, inp, **defect):
    dw0, db0 = inits(c, inp)
    _, dx, dw, db = bwd_emu(dy_prime(c, inp["dy"].float()), inp["x"].float(), inp["w"], inp["mean"], inp["rstd"],
                            inp["res"], None, dw0, db0, **defect)
    outs = {"dx": dx}
    if c["lp"]:
        outs["lp"] = dx.to(c["lp"])
    if dw is not None:
        outs["dw"] = dw
    if db is not None:
        outs["db"] = db
    return outs


def ln_bwd_refs(c, inp, outs):
    dw0, db0 = inits(c, inp)
    res = None if inp["res"] is None else inp["res"].double()
    dx, e_dx, dw, e_dw, db, e_db = bwd_ref(dy_prime(c, inp["dy"].double()), inp["x"].double(), inp["w"].double(),
                                           inp["mean"], inp["rstd"], res, None, dw0, db0)
    items = [("dx", dx, e_dx)]
    if c["lp"]:
        items.append(("lp", outs["dx"].to(c["lp"]), None))
    if dw is not None:
        items.append(("dw", dw, e_dw))
    if db is not None:
        items.append(("db", db, e_db))
    return items


# dclip_layernorm_bwd_add, and the delayed-scale forms dclip_layernorm_bwd_scaled / _scaled_add
FUSED_SHAPES = [(10, 512), (4107, 512), (10, 768), (10, 1024), (4107, 768), (4107, 1024)]


def ln_bwd_add_cases():
    return [dict(rows=rows, cols=cols, ntok=(5, 197)[i % 2], dydt=(F32, BF16)[i % 2], adt=BF16, lp=(BF16, F16)[(i // 2) % 2],
                 res="sep" if i % 3 else None, ws=i % 3 != 2, null=(None, None, "dw", "both")[i % 4], use=1)
            for i, (rows, cols) in enumerate(FUSED_SHAPES)]


def ln_bwd_scaled_cases():
    """both forms at all six shapes.  A width and a dy type make one instantiation of ln_bwd_fast
    each; of the wrapped walks (4107 rows) _scaled_add takes f16 dy on dy_scale at 512 and 1024 and
    f32 at 768, _scaled f16 dy on dy_scale at 768 and f32 at 512 and 1024"""
    cs = [dict(entry="scaled_add", rows=rows, cols=cols, ntok=(5, 197)[i % 2], dydt=F16 if i % 2 else F32,
               dsc=i % 2 == 1, adt=(F16, BF16)[(i // 2) % 2], asc=i % 3 != 0, res="sep" if i % 3 != 1 else None,
               ws=i % 3 != 2, null=None) for i, (rows, cols) in enumerate(FUSED_SHAPES)]
    cs += [dict(entry="scaled", rows=rows, cols=cols, ntok=0, dydt=F16 if i % 2 == 0 else F32, dsc=i % 2 == 0, adt=None,
                asc=False, res="alias" if i % 2 else "sep", ws=i % 3 != 0, null=(None, "db", "dw")[i % 3])
           for i, (rows, cols) in enumerate(FUSED_SHAPES)]
    return cs


def fused_inputs(c):
    rows, cols, use = c["rows"], c["cols"], c["use"]
    g = gen(307 + rows + 3 * cols + 11 * use + c["ntok"])
    m = USE_MULT[use]
    x = randn(g, rows, cols) + 0.3
    dy = times(randn(g, rows, cols), m)
    if c.get("dsc"):
        dy = dy / DY_SCALE
    dy = dy.to(c["dydt"])
    if use == INF_USE and "entry" in c:
        dy[inf_row(c), 5] = float("inf")
    add = None
    if c["adt"] is not None:
        add = times(randn(g, rows, cols), m * (1 / ADD_SCALE if c.get("asc") else 1.0) * 0.25).to(c["adt"])
        add[torch.arange(rows) % c["ntok"] == 0] = float("nan")  # the CLS rows read as 0
    mean, rstd = ln_stats(x)
    return {"x": x, "dy": dy, "w": signed_weight(g, cols), "res": times(randn(g, rows, cols), m) if c["res"] else None,
            "add": add, "dw0": randn(g, cols), "db0": randn(g, cols), "mean": mean, "rstd": rstd}


def fused_null(c):
    """use INF_USE runs without dw / db: a column sum over an inf says nothing"""
    return "both" if c["use"] == INF_USE and "entry" in c else c["null"]


def add_term(c, add, keep_cls=False):
    if add is None:
        return None
    t = add * ADD_SCALE if c.get("asc") else add
    return t if keep_cls else mask_rows(t, c["ntok"])


def fused_emulate(c, inp, keep_cls=False, s=None, clear=True, **defect):
    cn = dict(c, null=fused_null(c))
    dw0, db0 = inits(cn, inp)
    core, dx, dw, db = bwd_emu(dy_prime(c, inp["dy"].float()), inp["x"], inp["w"], inp["mean"], inp["rstd"], inp["res"],
                               add_term(c, None if inp["add"] is None else inp["add"].float(), keep_cls), dw0, db0, **defect)
    outs = {"dx": dx}
    if "entry" in c:
        s = ds_scale(inp["st"], c["use"]) if s is None else s
        outs["lp"] = (dx * s).to(F16)
        outs["st"], outs["spair"] = ds_apply(inp["st"], c["use"], maxbits(dx), s, clear)
    else:
        outs["lp"] = dx.to(c["lp"])
    if dw is not None:
        outs["dw"] = dw
    if db is not None:
        outs["db"] = db
    return outs


def fused_refs(c, inp, outs):
    cn = dict(c, null=fused_null(c))
    dw0, db0 = inits(cn, inp)
    res = None if inp["res"] is None else inp["res"].double()
    dx, e_dx, dw, e_dw, db, e_db = bwd_ref(dy_prime(c, inp["dy"].double()), inp["x"].double(), inp["w"].double(),
                                           inp["mean"], inp["rstd"], res,
                                           add_term(c, None if inp["add"] is None else inp["add"].double()), dw0, db0)
    items = [("dx", finite_rows(c, dx), finite_rows(c, e_dx))]
    if "entry" in c:
        s, ds = ds_items(inp["st"], c["use"], maxbits(outs["dx"]))
        items.append(("lp", finite_rows(c, (outs["dx"] * s).to(F16)), None))
        items += ds
        if c["use"] == INF_USE:
            ones = torch.ones(c["cols"], dtype=torch.uint8)
            items += [("dx_inf_row", ones, None), ("lp_inf_row", ones, None)]
    else:
        items.append(("lp", outs["dx"].to(c["lp"]), None))
    if dw is not None:
        items.append(("dw", dw, e_dw))
    if db is not None:
        items.append(("db", db, e_db))
    return items


def fused_split(c, outs):
    o = dict(outs, dx=finite_rows(c, outs["dx"]), lp=finite_rows(c, outs["lp"]))
    if "entry" in c:
        o.update(ds_split(c["use"], outs))
        if c["use"] == INF_USE:
            o["dx_inf_row"], o["lp_inf_row"] = nonfinite_flag(c, outs["dx"]), nonfinite_flag(c, outs["lp"])
    return o


# ----------------------------------------------------------------------------- read-out folds
READOUT_SHAPES = [(r, c) for c in (8, 768) for r in (1, 6, 1030)]


def readout_cast_cases():
    return [dict(rows=rows, cols=cols, ntok=(1, 3, 197)[(i + j) % 3], bdt=bdt, lp=(F16, BF16)[(i + j) % 2], alias=(i + j) % 2 == 1,
                 scale=(1.0, 1024.0)[(i // 2 + j) % 2], use=1)
            for i, (rows, cols) in enumerate(READOUT_SHAPES) for j, bdt in enumerate((F32, F16, BF16))]


def readout_amax_cases():
    return [dict(rows=rows, cols=cols, ntok=(3, 197, 1)[(i + j) % 3], bdt=bdt, alias=(i + j) % 2 == 0, asc=(i + j) % 3 != 0, use=1)
            for i, (rows, cols) in enumerate(READOUT_SHAPES) for j, bdt in enumerate((F32, F16, BF16))]


def readout_scaled_cases():
    """rows = 1029 at cols = 8: n8 = 1029 chunks, odd, so the second chunk of the last iteration is absent"""
    shapes = READOUT_SHAPES + [(1029, 8)]
    cs = [dict(rows=rows, cols=cols, ntok=(197, 3, 1)[i % 3], bdt=(F32, F16, BF16)[i % 3], alias=i % 2 == 1, asc=i % 2 == 0,
               bnull=False) for i, (rows, cols) in enumerate(shapes)]
    return cs + [dict(rows=6, cols=768, ntok=3, bdt=F32, alias=False, asc=False, bnull=True)]


def readout_inputs(c):
    rows, cols, use = c["rows"], c["cols"], c["use"]
    g = gen(401 + rows + 3 * cols + 11 * use + c["ntok"])
    m = USE_MULT[use]
    a = times(randn(g, rows, cols), m)
    if use == INF_USE and "bnull" in c:
        a[inf_row(c), 5] = float("inf")
    b = times(randn(g, rows, cols), m * (1 / ADD_SCALE if c.get("asc") else 1.0) * 0.25).to(c["bdt"])
    b[torch.arange(rows) % c["ntok"] == 0] = float("nan")
    return {"a": a, "b": None if c.get("bnull") else b}


def readout_sum(c, a, b, keep_cls=False):
    if b is None:
        return a
    return a + add_term(c, b, keep_cls)


def readout_cast_emulate(c, inp, keep_cls=False):
    s = readout_sum(c, inp["a"], inp["b"].float(), keep_cls)
    return {"sum": s, "lp": (s * torch.tensor(c["scale"], dtype=F32)).to(c["lp"])}


def readout_cast_refs(c, inp, outs):
    assert math.frexp(c["scale"])[0] == 0.5
    return [("sum", readout_cast_emulate(c, inp)["sum"], None),  # one f32 addition: one possible result
            ("lp", (outs["sum"] * torch.tensor(c["scale"], dtype=F32)).to(c["lp"]), None)]


def readout_bound(c, inp):
    a = inp["a"].double()
    t = torch.zeros_like(a) if inp["b"] is None else add_term(c, inp["b"].double())
    return a + t, eps_of(F32) * (a + t).abs() + 2 * U * (a.abs() + t.abs())


def readout_amax_emulate(c, inp):
    s = readout_sum(c, inp["a"], inp["b"].float())
    return {"sum": s, "ws": pair_words(TARGET, maxbits(s))}


def readout_amax_refs(c, inp, outs):
    ref, bound = readout_bound(c, inp)
    return [("sum", ref, bound), ("ws", pair_words(TARGET, maxbits(outs["sum"])), None)]


def readout_scaled_emulate(c, inp, s=None, clear=True):
    x = readout_sum(c, inp["a"], None if inp["b"] is None else inp["b"].float())
    s = ds_scale(inp["st"], c["use"]) if s is None else s
    outs = {"lp": (x * s).to(F16)}
    if inp["b"] is not None:
        outs["sum"] = x
    outs["st"], outs["spair"] = ds_apply(inp["st"], c["use"], maxbits(x), s, clear)
    return outs


def readout_scaled_refs(c, inp, outs):
    written = inp["a"] if inp["b"] is None else outs["sum"]  # b = NULL: sum is not written, lp is a's cast
    s, ds = ds_items(inp["st"], c["use"], maxbits(written))
    lp = (written * s).to(F16)
    items = [("lp", lp, None)] + ds  # an inf (not a NaN) has one bit pattern: lp is held whole
    if inp["b"] is not None:
        ref, bound = readout_bound(c, inp)
        items.append(("sum", finite_rows(c, ref), finite_rows(c, bound)))
    if c["use"] == INF_USE and inp["b"] is not None:  # the inf reaches sum at its own element and nowhere else
        items.append(("sum_inf_row", (~torch.isfinite(inp["a"][inf_row(c)])).to(torch.uint8), None))
    return items


def readout_scaled_split(c, outs):
    o = dict(outs)
    o.update(ds_split(c["use"], outs))
    if "sum" in outs:
        o["sum"] = finite_rows(c, outs["sum"])
        if c["use"] == INF_USE:
            o["sum_inf_row"] = nonfinite_flag(c, outs["sum"])
    return o


# ----------------------------------------------------------------------------- dclip_grad_scale
# 512 workgroups x 256 threads x 4 loads of 4 elements: the unrolled loop needs n / 4 > 3 x 131072,
# which 2^21 + 4003 reaches (with a remainder for the single-load loop and a scalar tail of 3)
GRAD_SCALE_N = (0, 1, 3, 4, 1027, 2 ** 20 + 3, 2 ** 21 + 4003)
GRAD_SCALE_KINDS = ("normal", "zero", "nan", "inf", "target", "denormal", "3e38")


def grad_scale_positions(n):
    pos = {"first": 0, "last": n - 1}
    if n >= 8:
        pos["body"] = (n // 4) * 2 + 1
    if n % 4:
        pos["tail"] = 4 * (n // 4)
    return pos


def grad_scale_cases():
    cs = [dict(n=0, place="first", kind="zero")]
    for n in GRAD_SCALE_N[1:]:
        for place in grad_scale_positions(n):
            cs.append(dict(n=n, place=place, kind="normal"))
    for i, kind in enumerate(GRAD_SCALE_KINDS[1:]):
        for n in (3, 1027):
            cs.append(dict(n=n, place=("tail", "body", "last", "first")[i % 4] if n == 1027 else "tail", kind=kind))
    return cs


def grad_scale_inputs(c):
    n, kind = c["n"], c["kind"]
    g = randn(gen(503 + n), n) * 0.1
    if kind in ("zero", "denormal"):
        g = torch.zeros(n)
    if n and kind != "zero":
        g[grad_scale_positions(n)[c["place"]]] = {"normal": -37.5, "nan": float("nan"), "inf": float("-inf"), "target": TARGET,
                                                  "denormal": 1e-40, "3e38": 3e38}[kind]
    return {"g": g, "g2": g * 4 + 0.001}  # a second call on the same ws, other data


def grad_scale_emulate(c, inp, skip_tail=False, nearest=False):
    outs = {}
    for name, g in (("ws", inp["g"]), ("ws2", inp["g2"])):
        m = maxbits(g[:4 * (c["n"] // 4)] if skip_tail else g)
        e = scale_exponent(TARGET, m, nearest) or 0
        outs[name] = torch.tensor([fbits(2.0 ** e), fbits(2.0 ** -e), 0, 0], dtype=torch.int32)
    return outs


def grad_scale_refs(c, inp, outs):
    return [("ws", pair_words(TARGET, maxbits(inp["g"])), None), ("ws2", pair_words(TARGET, maxbits(inp["g2"])), None)]


# ----------------------------------------------------------------------------- dclip_row_scale_add
KEEP = 0.5


def row_scale_add_cases():
    return [dict(ntok=ntok, B=B, cols=cols, x=x) for ntok in (1, 5) for B in (1, 3) for cols in (4, 772)
            for x in (None, "sep", "alias")]


def row_scale_add_inputs(c):
    ntok, rows = c["ntok"], c["ntok"] * c["B"]
    g = gen(601 + rows + c["cols"])
    s = torch.where(torch.arange(ntok) % 2 == (c["B"] == 1), 0.0, 1 / KEEP)  # zeros and 1 / keep
    return {"x": randn(g, rows, c["cols"]) if c["x"] else None, "y": randn(g, rows, c["cols"]), "s": s.float()}


def row_scale_add_emulate(c, inp):
    v = inp["y"] * inp["s"].repeat(c["B"])[:, None]
    return {"out": v if inp["x"] is None else v + inp["x"]}


def row_scale_add_refs(c, inp, outs):
    assert all(v == 0 or math.frexp(v)[0] == 0.5 for v in inp["s"].tolist())
    return [("out", row_scale_add_emulate(c, inp)["out"], None)]


def _same(c, outs):
    return outs


FAMILIES = {
    "ln_fwd": (ln_fwd_cases, ln_fwd_inputs, ln_fwd_emulate, ln_fwd_refs, _same),
    "ln_bwd": (ln_bwd_cases, ln_bwd_inputs, ln_bwd_emulate, ln_bwd_refs, _same),
    "ln_bwd_add": (ln_bwd_add_cases, fused_inputs, fused_emulate, fused_refs, fused_split),
    "ln_bwd_scaled": (ln_bwd_scaled_cases, fused_inputs, fused_emulate, fused_refs, fused_split),
    "readout_cast": (readout_cast_cases, readout_inputs, readout_cast_emulate, readout_cast_refs, _same),
    "readout_amax": (readout_amax_cases, readout_inputs, readout_amax_emulate, readout_amax_refs, _same),
    "readout_scaled": (readout_scaled_cases, readout_inputs, readout_scaled_emulate, readout_scaled_refs, readout_scaled_split),
    "grad_scale": (grad_scale_cases, grad_scale_inputs, grad_scale_emulate, grad_scale_refs, _same),
    "row_scale_add": (row_scale_add_cases, row_scale_add_inputs, row_scale_add_emulate, row_scale_add_refs, _same),
}


def norm_case_id(c):
    return case_id({k: (f"{v:g}" if isinstance(v, float) else v) for k, v in c.items()})


def check_case(family, c, inp, outs, worst=None):
    """hold the outputs of one case (by the entry points' names) to the family's items"""
    _, _, _, refs, split = FAMILIES[family]
    hold(f"{family} {norm_case_id(c)}", refs(c, inp, outs), split(c, outs), worst)


def run_sequence(family, base, step, worst=None, uses=USES):
    """uses 1 .. 5 of one delayed-scale state seeded as the header describes: step(case, inputs) ->
    outputs (with the state after the use as "st", int32 words), each use held to the family's items"""
    _, inputs, _, _, _ = FAMILIES[family]
    st = ds_seed()
    for use in uses:
        c = dict(base, use=use)
        inp = inputs(c)
        inp["st"] = st
        outs = step(c, inp)
        check_case(family, c, inp, outs, worst)
        st = outs["st"].clone()
    return st
