"""The cases, inputs, fp64 reference, bounds and plain-torch emulation of test_gpu_depth_loss_contract.py
(dclip_upsample_depth_stats / dclip_upsample_depth_finish: csrc/depthlossopt.hip, depth_band_kernel PASS 0,
1 and 2, depth_stats_fold_kernel, depth_bsum_fold_kernel and ce_band.h's merge), on CPU tensors, so that
the emulation goes through the very same checker (test_depth_loss_contract_emulation_cpu.py) before any
kernel does.  Conventions of silog_check.py / misc_check.py: the reference in fp64 from the values the
storage dtype holds, u = 2^-24, an item is (output name, reference, bound), no element is ever excluded, a
bound of zero demands the exact value.

The operation (include/dclip.h), X the low-res prediction (B, h, w), gt the target and M the mask (a
non-zero byte; all pixels without a mask) at (B, H, W); eps, lambd, the weights w_s, w_1, w_b and theta as
the f32 the ABI takes:
    p = Wy X Wx^T, d                         the resize and the log difference of silog_check
    r = p - gt, e = |r|                                                             on M
    stats = (S0, S1, T, Se, mx) = (sum d, sum d^2, #M, sum e, max e)                the stats pass
    c = theta mx;  b(e) = e if e <= c else (e^2 + c^2) / (2 c);  Sb = sum b(e)      the finish pass
    gd = w_s silog'(d, S0, T) + w_1 sign(r) / T' + w_b (sign(r) / T' if e <= c else r / (c T'));  T' = max(T, 1)
    grad = Wy^T gd Wx
The finish pass is judged on its own: S0, T and mx are the very f64 values of the `stats` buffer it was
handed (as silog_check judges pass 1), so c is theta times the handed maximum.

Why each bound holds; dp, dd, S0, S1 and the SILog gradient's (mag, dgd) are silog_check's:
dr    dp + u (|r| + dp): p is off by dp, the subtraction is one rounding of a value within dp of r.
Se    sum dr + 2^-50 sum e: ||a| - |b|| <= |a - b|; the terms are f32, the sum is f64 in some fixed order.
mx    max_M dr: |max a - max b| <= max |a - b|.  It is an f32 value held exactly in its f64 slot.
T     exact.  A slot the terms do not select comes back as it went in: bound 0 on (slot - start).
c     dc = u c: one f32 product of theta and the handed maximum (itself an f32).
b     e where e <= c: dr.  Above c: (e / c) dr + |e^2 - c^2| / (2 c^2) dc, the two first derivatives, times
      (1 + 2^-20) for the mixed second-order term, + dr^2 / (2 c) (the second derivative in e; the one in c
      is e^2 / c^3 dc^2 <= 2 u^2 b), + 5 u b: the four roundings of e e, c c, their sum and the division
      (2 c is exact), (1 + u)^4 - 1 < 5 u.
Sb    sum db + 2^-50 sum b.
gd    w_s silog': w_s dgd + u w_s mag, the product with the weight being one more rounding.
      w_1 sign(r) / T': u |g|, the one rounding of w_1 / T' (T < 2^24 is exact in f32; the sign is exact off
      the kink, below).
      w_b sign(r) / T' where e <= c: the same.  Above c: w_b dr / (c T') for the kernel's own r, + 5 u |g|:
      c's rounding (|g| dc / c = u |g|), the product c T', the division w_b / (c T'), the product with r,
      and the second-order terms of the four.
      The sum of the up to three terms: two additions, each rounding a partial sum that mag = w_s mag_s +
      |g_1| + |g_b| bounds: 2 u mag.
grad  silog_check.grad_items's fold: u |ref| + (Tt + 4) u fold(mag) + fold(dgd), plus u (|init| + |ref|) for
      the accumulating start's one add where a pixel with a gradient reaches, and 0 elsewhere (every
      element when T = 0): the element must come back as it went in.

Two conditions replace any exclusion, as "on the clamp" does in silog_check:
  * no in-mask pixel lies within dr of the kink r = 0 (the kernel's sign could differ);
  * with a BerHu weight, no in-mask pixel lies within dr + dc of the threshold e = c (the kernel and the
    reference could take different branches).
The reference asserts both; a seed that trips either is changed through RESEED, a pixel is never dropped.
The inputs are silog_check's recipe per (shape, dtype, mask), shared by the term configurations.
theta 0.9 is there because both branches must be populated: the share of in-mask pixels above c is 56-89 %
at theta 0.2 and 0.15-17 % at theta 0.9.
"""
import functools
import zlib

import torch

import misc_check as MC
import silog_check as SC
from misc_check import BF16, F16, F32, NAME, U

F64 = torch.float64
SHAPES = SC.SHAPES
MASKS = SC.MASKS
EPS, LAMBD = 1e-6, 0.5
CONFIGS = {  # (w_silog, w_l1, w_berhu), theta
    "l1": ((0.0, 1.0, 0.0), 0.2),
    "berhu0.2": ((0.0, 0.0, 1.0), 0.2),
    "berhu0.9": ((0.0, 0.0, 1.0), 0.9),
    "all": ((1.0, 0.5, 0.25), 0.2),
}
SILOG, L1, BERHU = 1, 2, 4  # DCLIP_DEPTH_*
STATS_START = (1.5, 2.5, 3.0, 4.5, 0.125, 7.0)
GRAD_START = SC.GRAD_START
BSUM_START = 0.75
# (shape, dtype name, mask) -> a suffix to the seed's text, for the inputs that put a pixel inside the
# threshold band of one configuration
RESEED = {("x16_seam", "bf16", "none"): "#1"}  # one pixel within dr + dc of e = c at theta 0.2 with the plain seed


def cases():
    return [dict(shape=s, dt=dt, mask=m, cfg=k) for s in SHAPES for dt in (F32, BF16, F16) for m in MASKS
            for k in CONFIGS]


def case_id(c):
    return f"{c['shape']}-{NAME[c['dt']]}-{c['mask']}-{c['cfg']}"


def base(c):
    """the silog_check case whose recipe, resize and SILog reference this case shares"""
    return dict(shape=c["shape"], dt=c["dt"], eps=EPS, lambd=LAMBD, mask=c["mask"])


def dims(c):
    return SHAPES[c["shape"]]


def weights(c):
    return CONFIGS[c["cfg"]][0]


def theta(c):
    return CONFIGS[c["cfg"]][1]


def terms(c):
    w_s, w_1, w_b = weights(c)
    return (SILOG if w_s > 0 else 0) | (L1 if w_1 > 0 else 0) | (BERHU if w_b > 0 else 0)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dt, mask):
    """silog_check.inputs's recipe, the seed from the same text plus RESEED's suffix"""
    c = dict(shape=shape, dt=dt, eps=EPS, lambd=LAMBD, mask=mask)
    B, h, w, H, W = SHAPES[shape]
    g = MC.gen(zlib.crc32((SC.case_id(c) + RESEED.get((shape, NAME[dt], mask), "")).encode()))
    pred = (torch.rand(B, h, w, generator=g) * 60 - 5).to(dt)
    target = 1 + 79 * torch.rand(B, H, W, generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.05] = 0.0
    valid = torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (B, H, W), generator=g)]
    keep = torch.rand(B, H, W, generator=g) < 0.8
    m = {"none": None, "random": torch.where(keep, valid, torch.zeros_like(valid)),
         "empty": torch.zeros(B, H, W, dtype=torch.uint8)}[mask]
    if m is not None:
        target[m == 0] = float("nan")
    return pred, target, m


def inputs(c):
    """pred (B, h, w) in its dtype, target (B, H, W) f32 with NaN in the masked-out pixels, mask None or u8:
    fresh copies, a test may write to them"""
    pred, target, m = _inputs(c["shape"], c["dt"], c["mask"])
    return {"pred": pred.clone(), "target": target.clone(), "mask": None if m is None else m.clone()}


in_mask = SC.in_mask
f32_of = SC.f32_of


# ----------------------------------------------------------------------------- the fp64 reference
def forward_ref(c, inp):
    """what both passes share: silog_check's forward reference plus r, e, dr (0 outside M), the two further
    stats and their bounds"""
    f = dict(SC.forward_ref(base(c), inp))
    M, p, dp = f["M"], f["p"], f["dp"]
    zero = torch.zeros_like(p)
    r = torch.where(M, p - torch.where(M, inp["target"].double(), zero), zero)
    e = r.abs()
    dr = torch.where(M, dp + U * (e + dp), zero)
    on_kink = M & (e <= dr)
    assert not bool(on_kink.any()), f"{case_id(c)}: {int(on_kink.sum())} pixels on the kink r = 0: change the seed"
    any_px = bool(M.any())
    f.update(r=r, e=e, dr=dr, Se=e.sum(), eSe=dr.sum() + 2.0 ** -50 * e.sum(),
             mx=e[M].max() if any_px else zero.sum(), emx=dr[M].max() if any_px else zero.sum())
    return f


@functools.lru_cache(maxsize=None)
def _shared_ref(shape, dt, mask):
    c = dict(shape=shape, dt=dt, mask=mask, cfg="l1")
    return forward_ref(c, inputs(c))


def shared_ref(c):
    """forward_ref of the case's unmodified inputs, computed once per (shape, dtype, mask)"""
    return _shared_ref(c["shape"], c["dt"], c["mask"])


def one(v):
    return torch.as_tensor(v, dtype=F64).reshape(1)


def stats_items(c, inp, start=STATS_START, fwd=None):
    """the six slots after the stats pass onto `start`: "S0", "S1", "T", "Se" with the start subtracted,
    "mx" and "spare" as they stand; a slot the terms do not select holds its start"""
    f = fwd or forward_ref(c, inp)
    t = terms(c)
    s = t & SILOG != 0
    se = t & (L1 | BERHU) != 0
    mx = t & BERHU != 0
    return [("S0", one(f["S0"] if s else 0.0), one(f["eS0"] if s else 0.0)),
            ("S1", one(f["S1"] if s else 0.0), one(f["eS1"] if s else 0.0)),
            ("T", one(f["T"]), one(0.0)),
            ("Se", one(f["Se"] if se else 0.0), one(f["eSe"] if se else 0.0)),
            ("mx", one(max(float(f["mx"]), start[4]) if mx else start[4]), one(f["emx"] if mx else 0.0)),
            ("spare", one(start[5]), one(0.0))]


def split_stats(raw, start=STATS_START):
    """the outputs stats_items names, from the six f64 the stats pass left"""
    raw, st = raw.double().cpu(), torch.tensor(start, dtype=F64)
    s = raw - st
    return {"S0": s[0:1], "S1": s[1:2], "T": s[2:3], "Se": s[3:4], "mx": raw[4:5], "spare": raw[5:6]}


def finish_ref(c, inp, given, fwd=None):
    """the finish pass from the f64 `given` stats: c, the per-pixel b and gd with their bounds and gd's
    magnitude"""
    f = fwd or forward_ref(c, inp)
    eps, lambd, th = f32_of(EPS), f32_of(LAMBD), f32_of(theta(c))
    w_s, w_1, w_b = (f32_of(v) for v in weights(c))
    M, p, dp, d, dd, r, e, dr = (f[k] for k in ("M", "p", "dp", "d", "dd", "r", "e", "dr"))
    S0, T, mx = float(given[0]), float(given[2]), float(given[4])
    Tp = T if T > 0 else 1.0
    zero = torch.zeros_like(p)
    gd, mag, dgd = zero.clone(), zero.clone(), zero.clone()
    sign = torch.sign(r)
    out = {}
    if w_s > 0:
        live = M & (p >= eps)
        g = torch.where(live, (2 * d / Tp - 2 * lambd * S0 / Tp ** 2) / p, zero)
        m = torch.where(live, ((2 * d / Tp).abs() + abs(2 * lambd * S0 / Tp ** 2)) / p.abs(), zero)
        dg = torch.where(live, 2 * dd / (Tp * p.abs()) + 8 * U * m + m * dp / p.abs(), zero)
        gd, mag, dgd = gd + w_s * g, mag + w_s * m, dgd + w_s * dg + U * w_s * m
    if w_1 > 0:
        g = torch.where(M, w_1 * sign / Tp, zero)
        gd, mag, dgd = gd + g, mag + g.abs(), dgd + U * g.abs()
    if w_b > 0:
        cc = th * mx
        dc = U * cc
        near = M & ((e - cc).abs() <= dr + dc)
        assert not bool(near.any()), \
            f"{case_id(c)}: {int(near.sum())} pixels within dr + dc of the threshold e = c: change the seed (RESEED)"
        above = M & (e > cc)
        safe = cc if cc > 0 else 1.0
        b = torch.where(above, (e * e + cc * cc) / (2 * safe), e)
        db = torch.where(above, ((e / safe) * dr + (e * e - cc * cc).abs() / (2 * safe * safe) * dc) * (1 + 2.0 ** -20)
                         + dr * dr / (2 * safe) + 5 * U * b, dr)
        g = torch.where(above, w_b * r / (safe * Tp), torch.where(M, w_b * sign / Tp, zero))
        dg = torch.where(above, w_b * dr / (safe * Tp) + 5 * U * g.abs(), U * g.abs())
        gd, mag, dgd = gd + g, mag + g.abs(), dgd + dg
        out.update(c=cc, above=above, Sb=b.sum(), eSb=db.sum() + 2.0 ** -50 * b.sum())
    dgd = dgd + 2 * U * mag
    out.update(gd=gd, mag=mag, dgd=dgd)
    return out


def finish_items(c, inp, given, init=GRAD_START, bsum_start=BSUM_START, fwd=None, name="grad"):
    """"Sb" (the start subtracted; with a BerHu weight only) and the gradient accumulated onto `init`"""
    B, h, w, H, W = dims(c)
    f = fwd or forward_ref(c, inp)
    fr = finish_ref(c, inp, given, f)
    Wy, Wx = MC.lerp_matrix(h, H), MC.lerp_matrix(w, W)
    fold = lambda t: Wy.abs().t() @ t @ Wx.abs()  # noqa: E731
    ref = Wy.t() @ fr["gd"] @ Wx
    Tt = MC.touch(Wy) * MC.touch(Wx)
    fmag = fold(fr["mag"])
    bound = U * ref.abs() + (Tt + 4) * U * fmag + fold(fr["dgd"])
    init = torch.as_tensor(init, dtype=F64).expand_as(ref)
    bound = bound + U * (init.abs() + ref.abs()) * (fmag > 0)
    its = [(name, init + ref, bound)]
    if "Sb" in fr:
        its.insert(0, ("Sb", one(fr["Sb"]), one(fr["eSb"])))
    return its


def items(c, inp, given, fwd=None):
    """everything test_both_passes holds: the stats onto STATS_START, Sb, the gradient onto GRAD_START and, as
    "grad0", onto zero (next to 0.25 the last add's rounding hides the fold, as in silog_check)"""
    f = fwd or forward_ref(c, inp)
    fin = finish_items(c, inp, given, GRAD_START, fwd=f)
    return stats_items(c, inp, fwd=f) + fin + [finish_items(c, inp, given, 0.0, fwd=f, name="grad0")[-1]]


def loss_ref(c, inp, given, fwd=None):
    """the loss ops.UpsampleDepthLossFn forms (the weights and lambd as host doubles) from the reference sums,
    Sb from the `given` stats' c as the finish pass takes it, and the bound the sums' bounds imply plus the
    result's rounding to f32"""
    f = fwd or forward_ref(c, inp)
    T = float(f["T"])
    if T == 0:
        return 0.0, 0.0
    w_s, w_1, w_b = weights(c)
    loss = bound = size = 0.0
    if w_s > 0:
        S0, S1, e0, e1 = float(f["S0"]), float(f["S1"]), float(f["eS0"]), float(f["eS1"])
        loss += w_s * (S1 / T - LAMBD * S0 ** 2 / T ** 2)
        bound += w_s * (e1 / T + LAMBD * (2 * abs(S0) * e0 + e0 ** 2) / T ** 2)
        size += w_s * (S1 / T + LAMBD * S0 ** 2 / T ** 2)
    if w_1 > 0:
        loss += w_1 * float(f["Se"]) / T
        bound += w_1 * float(f["eSe"]) / T
        size += w_1 * float(f["Se"]) / T
    if w_b > 0:
        fr = finish_ref(c, inp, given, f)
        loss += w_b * float(fr["Sb"]) / T
        bound += w_b * float(fr["eSb"]) / T
        size += w_b * float(fr["Sb"]) / T
    return loss, bound + U * abs(loss) + 2.0 ** -48 * size


# ----------------------------------------------------------------------------- NaN
def nan_verdict(c, stats, bsum, T):
    """What a NaN among the in-mask resized predictions or targets must do (include/dclip.h): sum e, the
    maximum and sum b(e) non-finite for the terms that have them, T exact.  Returns the list of violations."""
    t, bad = terms(c), []
    if t & (L1 | BERHU) and bool(torch.isfinite(stats[3])):
        bad.append(f"sum e = {float(stats[3])} is finite")
    if t & BERHU and bool(torch.isfinite(stats[4])):
        bad.append(f"max e = {float(stats[4])} is finite: the maximum dropped the NaN")
    if t & BERHU and bool(torch.isfinite(bsum).all()):
        bad.append(f"sum b(e) = {float(bsum.reshape(-1)[0])} is finite")
    if float(stats[2]) != float(T):
        bad.append(f"T = {float(stats[2])}, not {float(T)}")
    return bad


# ----------------------------------------------------------------------------- the f32 emulation
def emu_pixels(c, inp):
    """p, d, r (f32; d and r zero outside the mask) and the mask, as depth_band_kernel computes them"""
    p, d, M = SC.emu_pixels(base(c), inp)
    r = torch.where(M, p - inp["target"], torch.zeros_like(p))
    assert r.dtype == F32
    return p, d, r, M


def emu_stats(c, d, r, M, start=(0.0,) * 6, keep_nan=True):
    """the six f64 after the stats pass onto `start`; keep_nan=False is fmaxf's maximum, which drops a NaN"""
    t, s = terms(c), torch.tensor(start, dtype=F64)
    e = r.abs().double()[M]
    if t & SILOG:
        dm = d.double()[M]
        s[0] += dm.sum()
        s[1] += dm.pow(2).sum()
    s[2] += M.sum().double()
    if t & (L1 | BERHU):
        s[3] += e.sum()
    if t & BERHU:
        if keep_nan:
            m = torch.cat([e, s[4:5]]).max()  # torch.max keeps a NaN
        else:
            m = torch.cat([e[~torch.isnan(e)], s[4:5]]).max()
        s[4] = m
    return s


def emu_finish(c, p, d, r, M, given, init=GRAD_START, bsum_start=BSUM_START, **defect):
    """(sum b(e) onto bsum_start or None, the gradient onto init) as PASS 2 computes them"""
    bsum, gd = emu_gd(c, p, d, r, M, given, bsum_start, **defect)
    return bsum, SC.emu_fold(base(c), gd, init)


def emu_gd(c, p, d, r, M, given, bsum_start=BSUM_START, branch="right", through_max=False, drop=None):
    """(sum b(e) onto bsum_start or None, the per-pixel gradient) as PASS 2 computes them: the call's constants
    from the handed stats in f32.  Planted defects: branch="linear" takes sign(r) / T' above c too,
    through_max adds the gradient of c = theta max e at the pixel that holds the maximum, drop=(b, y, x)
    leaves one pixel out of the fold."""
    w_s, w_1, w_b = (torch.tensor(v, dtype=F32) for v in weights(c))
    eps, lambd, th = (torch.tensor(v, dtype=F32) for v in (EPS, LAMBD, theta(c)))
    gS, gT, mx = given[0].to(F32), given[2].to(F32), given[4].to(F32)
    gT = gT if float(gT) > 0 else torch.tensor(1.0, dtype=F32)
    zero = torch.zeros_like(p)
    e, sg = r.abs(), torch.sign(r)
    gd, bsum = zero.clone(), None
    if float(w_s) > 0:
        inv = torch.where(p >= eps, 1 / p, zero)
        gd = w_s * ((2 * d / gT - 2 * lambd * gS / (gT * gT)) * inv)
    if float(w_1) > 0:
        gd = gd + sg * (w_1 / gT)
    if float(w_b) > 0:
        cc = th * mx
        lin = e <= cc
        b = torch.where(lin, e, (e * e + cc * cc) / (2 * cc))
        bsum = torch.tensor([bsum_start], dtype=F64) + b.double()[M].sum()
        kc = w_b / (cc * gT) if float(cc) > 0 else torch.tensor(0.0, dtype=F32)
        gb = torch.where(lin, sg * (w_b / gT), r * kc)
        if branch == "linear":
            gb = sg * (w_b / gT)
        gd = gd + gb
        if through_max:
            above = M & ~lin
            dSb_dc = ((cc * cc - e * e) / (2 * cc * cc))[above].sum()
            at = (e * M).reshape(-1).argmax()
            gd.reshape(-1)[at] += (w_b / gT) * dSb_dc * th * sg.reshape(-1)[at]
    assert gd.dtype == F32
    gd = torch.where(M, gd, zero)
    if drop is not None:
        gd[drop] = 0
    return bsum, gd


def emulate(c, inp):
    """both passes as the GPU test runs them: the stats onto STATS_START, the finish pass onto BSUM_START /
    GRAD_START and onto zero from a stats pass of its own that started at zero; (outputs by name, those stats)"""
    p, d, r, M = emu_pixels(c, inp)
    outs = split_stats(emu_stats(c, d, r, M, STATS_START))
    given = emu_stats(c, d, r, M)
    bsum, grad = emu_finish(c, p, d, r, M, given)
    _, grad0 = emu_finish(c, p, d, r, M, given, init=0.0)
    outs.update(grad=grad, grad0=grad0)
    if bsum is not None:
        outs["Sb"] = bsum - BSUM_START
    return outs, given
