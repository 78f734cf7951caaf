"""Every entry point of csrc/layernorm.hip (dclip_layernorm_fwd, _bwd, _bwd_res, _bwd_add, _bwd_scaled,
_bwd_scaled_add, _bwd_ws_floats) and the fp16 gradient-scale entry points of csrc/misc.hip
(dclip_grad_scale, dclip_add_readout_cast / _amax / _cast_scaled, dclip_row_scale_add) behind the C
ABI on guard-banded, poisoned buffers (abi_guard.py), every output against an fp64 reference per
element or bit for bit (norm_check.py: the cases, the references, the bounds and why they hold).

What test_gpu_kernels.py and test_gpu_fp16.py cannot see, with one norm over the whole tensor, an
fp32 reference computed by the GPU, or one kernel compared with another:
  * one wrong row: the last row, the first row of a wrapped persistent walk (forward above 8192
    rows, backward above 4096, the generic backward above 4096), a wave without a row;
  * the generic kernels above 256 columns, at widths that are no multiple of 256, and at 2048;
  * a constant row, a zero row, rows 100 standard deviations from zero, eps from 1e-12 to 1e-2;
  * NaN in the rows dy_ntok and ntok drop, which must reach no output and no dw / db;
  * lp as the cast of the dx that was WRITTEN, res aliasing dx, dw / db accumulating onto non-zero
    values on the table path, the atomic path and the generic kernel's, each of them NULL;
  * the dw / db partials table at exactly the queried size, poisoned, and untouched without dw / db;
  * the backward on its own: it is fed the mean / rstd dclip_layernorm_fwd wrote, and the
    reference uses those same values;
  * the delayed-scale protocol through uses 1 .. 5 of ONE state, every word of it bit for bit: a
    use 2^6 times larger, an all-zero use (the scale is kept), a use with an inf (lp carries it, the
    next scale is kept); dclip_grad_scale's scalar tail, clamps and reset words.
The CPU emulation goes through the same checker at the same cases in
test_norm_contract_emulation_cpu.py.  At the end the module prints, per entry point and dtypes, the
worst figure over its cases as a fraction of its bound (bitwise outputs: the number of differing
elements, 0) and the module's run time.

The kernels on the MI355X over all 243 tests (12.6 s for the module, the fp64 references on the CPU
included; the slowest, five uses at 4107 x 1024, 2.1 s), next to the f32 emulation, worst figure /
bound over an entry point's cases; every bitwise output differs in 0 elements (lp, dclip_add_readout_cast's
sum, dclip_row_scale_add, dclip_grad_scale's and dclip_add_readout_amax's ws, spair and all five
groups of state words after each of five uses, dclip_layernorm_bwd_add against the two passes in dx,
lp and, on the table path, dw and db):
    entry point / output                   kernels                emulation
    layernorm_fwd mean, rstd               0.267, 0.263           0.267, 0.278
                  y  f32 | fp16 | bf16     0.265 | 0.970 | 0.994  0.266 | 0.970 | 0.994  (16-bit: the output's own rounding)
    layernorm_bwd(_res) dx, dw, db         0.175, 0.451, 0.200    0.175, 0.451, 0.225
    layernorm_bwd_add   dx, dw, db         0.025, 0.128, 0.128    0.029, 0.149, 0.152
    layernorm_bwd_scaled      dx, dw, db   0.031, 0.229, 0.161    0.035, 0.205, 0.175 (both scaled forms)
    layernorm_bwd_scaled_add  dx, dw, db   0.024, 0.267, 0.159
    add_readout_amax, _cast_scaled sum     0.333                  0.333
dx stays far below 1 in both columns because its bound charges every row sum n roundings in the
worst order while the kernels (lane-serial, then a butterfly) and torch (pairwise) sum at depth n / 64
+ 6 and log2 n; the 0.175 is at 4 columns (4101 x 4), where little of the bound is summation.  rstd's
0.263 is the zero row of the eps = 1e-5 cases, where only the addition of eps and rsqrtf round: about
1 u of the (1 + 3) u allowed there; the emulation's 0.278 is an ordinary row.

NOT pinned: the sign of a zero in a delayed-scale lp.  For (f16)(x * s) hipcc emits v_fma_mixlo_f16 /
v_fma_mixhi_f16 x, s, 0 for some elements of a lane's eight and a packed f32 multiply followed by a
conversion for the others (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S csrc/layernorm.hip,
the ln_bwd_fast kernels with a delayed scale), and -0 * s + (+0) is +0: a dx of -0 gives an lp of +0
in the former and of -0 in the latter.  The values are equal and lp only feeds GEMMs.  So that lp can
be held bit for bit at every other element, the all-zero use feeds zeros of one sign (+0,
norm_check.times) and no -0 reaches dx there; at the other uses a dx of exactly -0 does not occur in
the random data.  It follows that this contract does not notice a change that makes -0 appear in dx,
or that moves the sign of a zero in lp: it compares lp with the cast of the dx that was written only
where that dx is not -0.
"""
import time

import pytest
import torch

import norm_check as NC
from abi_guard import FINITE, POISON, GuardedMatrix, guarded, guarded_copy, run_poisoned
from norm_check import BF16, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}  # (entry point, dtypes) -> {output: worst figure / bound} over this session
ENTRY = {"ln_fwd": "dclip_layernorm_fwd", "ln_bwd": "dclip_layernorm_bwd(_res)", "ln_bwd_add": "dclip_layernorm_bwd_add",
         "scaled": "dclip_layernorm_bwd_scaled", "scaled_add": "dclip_layernorm_bwd_scaled_add",
         "readout_cast": "dclip_add_readout_cast", "readout_amax": "dclip_add_readout_amax",
         "readout_scaled": "dclip_add_readout_cast_scaled", "grad_scale": "dclip_grad_scale",
         "row_scale_add": "dclip_row_scale_add"}
INT = {4: torch.int32, 2: torch.int16}


@pytest.fixture(autouse=True)
def _need(hip):
    pass


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    for (entry, key), w in sorted(WORST.items()):
        print(f"\nnorm contract {entry} {key}: worst figure / bound " + ", ".join(f"{n} {v:.3f}" for n, v in sorted(w.items())),
              end="")
    print(f"\nnorm contract: {time.time() - t0:.1f} s for the module")


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


def io(values, as_int=False):
    """an argument the entry point reads and writes, with its entry values: (buffer, values) for
    run_poisoned's inout; as_int: held as integer words, for a result that may hold an inf or NaN"""
    v = values.to(DEV)
    v = v.reshape(1, -1) if v.dim() == 1 else v
    if as_int:
        v = v.view(INT[v.element_size()])
    return GuardedMatrix(v.shape[0], v.shape[1], v.shape[1], v.dtype), v


def out(shape, dt, as_int=False):
    return guarded(shape, INT[torch.empty((), dtype=dt).element_size()] if as_int else dt)


def typed(t, dt):
    return t if t.dtype == dt else t.view(dt)


def worst_of(family, c):
    return WORST.setdefault((ENTRY[c.get("entry", family)], NC.dtype_key(c)), {})


def check(family, c, inp, outs):
    outs = {k: v.cpu() for k, v in outs.items()}
    NC.check_case(family, c, inp, outs, worst_of(family, c))
    return outs


def cases(family):
    cs = NC.FAMILIES[family][0]()
    return pytest.mark.parametrize("c", cs, ids=[NC.norm_case_id(c) for c in cs])


def rejected(name, *args, why):
    """the entry point returns DCLIP_ERR_ARG before any launch and leaves the message of the check
    that the changed argument is to trip: `why` is a part of that message"""
    lib = NT().lib()
    assert getattr(lib, name)(*args) == -1, (name, "accepted", args)
    msg = lib.dclip_last_error().decode(errors="replace")
    assert name in msg and why in msg, (name, "rejected for another reason", msg)


def still(g, byte):
    """every byte of a guarded payload is still `byte`"""
    return bool((g.raw[g.off:g.off + g.nbytes] == byte).all())


def gpu_stats(inp):
    """the mean / rstd dclip_layernorm_fwd writes for inp["x"] at LN_EPS, into inp (the backward is
    judged on its own: the reference uses the same values)"""
    x = inp["x"]
    rows, cols = x.shape
    gx, gw, gb = gcopy(x), gcopy(torch.ones(cols)), gcopy(torch.zeros(cols))
    y, mean, rstd = guarded((rows, cols), BF16), guarded(rows, F32), guarded(rows, F32)
    NT().call("dclip_layernorm_fwd", gx.ptr(), code(x.dtype), gw.ptr(), gb.ptr(), y.ptr(), code(BF16), mean.ptr(),
              rstd.ptr(), rows, cols, NC.LN_EPS, stream())
    inp["mean"], inp["rstd"] = mean.t.cpu(), rstd.t.cpu()
    assert bool(torch.isfinite(inp["mean"]).all() and torch.isfinite(inp["rstd"]).all())
    return gcopy(inp["mean"]), gcopy(inp["rstd"])


# ----------------------------------------------------------------------------- forward
@cases("ln_fwd")
def test_layernorm_fwd(c):
    """ln_fwd_kernel (1 .. 8 column groups of 256, the last one ragged) and ln_fwd_fast (a wave's walk
    over rows, wrapped at 8197): y per element, mean and rstd per row, either of them NULL"""
    inp = NC.ln_fwd_inputs(c)
    rows, cols = c["rows"], c["cols"]
    gx, gw, gb = gcopy(inp["x"]), gcopy(inp["w"]), gcopy(inp["b"])
    y = guarded((rows, cols), c["ydt"])
    mean = None if c["null"] == "mean" else guarded(rows, F32)
    rstd = None if c["null"] == "rstd" else guarded(rows, F32)
    named = [(n, g) for n, g in (("y", y), ("mean", mean), ("rstd", rstd)) if g is not None]
    res = run_poisoned(lambda: NT().call("dclip_layernorm_fwd", gx.ptr(), code(c["xdt"]), gw.ptr(), gb.ptr(), y.ptr(),
                                         code(c["ydt"]), ptr(mean), ptr(rstd), rows, cols, c["eps"], stream()),
                       inputs=[gx, gw, gb], outputs=[g for _, g in named])
    check("ln_fwd", c, inp, dict(zip([n for n, _ in named], res)))


def test_layernorm_fwd_arguments():
    """rows = 0 writes nothing; cols in {0, 6, 2052} and rows = -1 are rejected with a message"""
    d = guarded(16384, F32)
    y = guarded(16384, F32, fill=POISON)
    p = d.ptr()
    NT().call("dclip_layernorm_fwd", p, code(F32), p, p, y.ptr(), code(F32), y.ptr(), y.ptr(), 0, 768, 1e-5, stream())
    torch.cuda.synchronize()
    assert still(y, POISON) and bool(y.intact())
    for rows, cols, why in ((2, 0, "must be a multiple of 4"), (2, 6, "must be a multiple of 4"), (2, 2052, "<= 2048"),
                            (-1, 768, "rows < 0")):
        rejected("dclip_layernorm_fwd", p, code(F32), p, p, y.ptr(), code(F32), None, None, rows, cols, 1e-5, stream(),
                 why=why)


# ----------------------------------------------------------------------------- backward
def bwd_blocks(rows, cols):
    return min((rows + 7) // 8, 512) if cols in (512, 768, 1024) else min((rows + 3) // 4, 1024)


class Backward:
    """the buffers of one LayerNorm backward case and its call through run_poisoned.  dw / db are
    in-out arguments with non-zero entry values; where several workgroups add to them atomically the
    order of the additions is free, so the two poisoned runs need not agree bit for bit: those are
    reset by the call itself, read after the second run and held to the any-order bound only."""

    def __init__(self, c, inp, nonfinite=False, with_lp=True, null=None):
        rows, cols = c["rows"], c["cols"]
        self.c, self.rows, self.cols = c, rows, cols
        null = c["null"] if null is None else null
        self.gdy, self.gx, self.gw = gcopy(inp["dy"]), gcopy(inp["x"]), gcopy(inp["w"])
        self.gmean, self.grstd = gpu_stats(inp)
        self.inputs = [self.gdy, self.gx, self.gw, self.gmean, self.grstd]
        self.outputs, self.inout, self.names_out, self.names_io, self.manual = [], [], [], [], []
        self.res = None
        if c["res"] in ("alias", "acc"):
            self.dx = self.add_io("dx", inp["res"], nonfinite)
            self.res = self.dx
        else:
            self.dx = self.add_out("dx", (rows, cols), F32, nonfinite)
            if c["res"] == "sep":
                self.res = gcopy(inp["res"])
                self.inputs.append(self.res)
        lp_dt = c.get("lp", F16)  # the delayed-scale forms: always fp16
        self.lp = self.add_out("lp", (rows, cols), lp_dt, nonfinite) if (with_lp and lp_dt) else None
        fast = cols in (512, 768, 1024)
        self.ws = None
        if c["ws"] and fast:
            n = int(NT().lib().dclip_layernorm_bwd_ws_floats(rows, cols))
            assert n == bwd_blocks(rows, cols) * 2 * cols  # the header's formula, and not a float more
            self.ws = guarded(n, F32)
        table = self.ws is not None
        self.ordered = table or bwd_blocks(rows, cols) == 1
        self.dw = self.dw_db("dw", inp["dw0"]) if null not in ("dw", "both") else None
        self.db = self.dw_db("db", inp["db0"]) if null not in ("db", "both") else None

    def add_out(self, name, shape, dt, as_int=False):
        g = out(shape, dt, as_int)
        self.outputs.append(g)
        self.names_out.append((name, dt))
        return g

    def add_io(self, name, values, as_int=False):
        g, v = io(values, as_int)
        self.inout.append((g, v))
        self.names_io.append((name, values.dtype))
        return g

    def dw_db(self, name, init):
        if self.ordered:
            return self.add_io(name, init)
        g, v = io(init)
        self.manual.append((name, g, v))
        self.inputs.append(g)  # its guard bands are checked with the inputs'
        return g

    def run(self, call, extra_inputs=(), extra_io=()):
        """extra_io: (name, dtype, (buffer, values)) in-out arguments of the fused forms (the scale state)"""
        def fn():
            for _, g, v in self.manual:
                g.fill(POISON)
                g.m.copy_(v)
            call()

        res = run_poisoned(fn, inputs=self.inputs + list(extra_inputs), outputs=self.outputs,
                           scratch=[self.ws] if self.ws else [], inout=self.inout + [e[2] for e in extra_io])
        names = self.names_out + self.names_io + [(n, dt) for n, dt, _ in extra_io]
        outs = {n: typed(t, dt) for (n, dt), t in zip(names, res)}
        for name, g, _ in self.manual:
            outs[name] = g.m.clone()
        for k in ("dw", "db", "st"):
            if k in outs:
                outs[k] = outs[k][0]
        return outs


@cases("ln_bwd")
def test_layernorm_bwd(c):
    """ln_bwd_kernel and ln_bwd_fast through dclip_layernorm_bwd_res (res none / separate / aliasing
    dx, lp, dy_scale, dy_ntok with NaN in the masked rows of dy, the partials table or atomics) and
    dclip_layernorm_bwd (accumulate = 1 onto dx's entry values, accumulate = 0 onto a poisoned dx)"""
    inp = NC.ln_bwd_inputs(c)
    rows, cols = c["rows"], c["cols"]
    b = Backward(c, inp)
    gs = scalar(NC.DY_SCALE) if c["dsc"] else None
    if c["res"] in ("acc", "plain"):
        def call():
            NT().call("dclip_layernorm_bwd", b.gdy.ptr(), code(c["dydt"]), b.gx.ptr(), code(c["xdt"]), b.gw.ptr(),
                      b.gmean.ptr(), b.grstd.ptr(), b.dx.ptr(), int(c["res"] == "acc"), ptr(b.dw), ptr(b.db), rows, cols,
                      stream())
    else:
        def call():
            NT().call("dclip_layernorm_bwd_res", b.gdy.ptr(), code(c["dydt"]), ptr(gs), c["ntok"], b.gx.ptr(), code(c["xdt"]),
                      b.gw.ptr(), b.gmean.ptr(), b.grstd.ptr(), ptr(b.res), b.dx.ptr(), ptr(b.lp),
                      code(c["lp"]) if c["lp"] else 0, ptr(b.dw), ptr(b.db), ptr(b.ws), rows, cols, stream())
    outs = b.run(call, [gs] if gs else [])
    if b.ws is not None and c["null"] == "both":
        assert still(b.ws, FINITE), "the partials table was written though neither dw nor db was asked for"
    check("ln_bwd", c, inp, outs)


def test_layernorm_bwd_arguments():
    lib, d = NT().lib(), guarded(16384, F32)
    p = d.ptr()
    for cols in (512, 768, 1024):
        for rows in (1, 7, 8, 9, 4095, 4096, 4097, 4107, 100000):
            assert int(lib.dclip_layernorm_bwd_ws_floats(rows, cols)) == min(-(-rows // 8), 512) * 2 * cols
        assert int(lib.dclip_layernorm_bwd_ws_floats(0, cols)) == 0 and int(lib.dclip_layernorm_bwd_ws_floats(-3, cols)) == 0
    for cols in (4, 256, 260, 2048):
        assert int(lib.dclip_layernorm_bwd_ws_floats(64, cols)) == 0

    def res(dy_scale, dy_ntok, lp, lp_dt, cols, why):
        rejected("dclip_layernorm_bwd_res", p, code(F32), dy_scale, dy_ntok, p, code(F32), p, p, p, None, p, lp, lp_dt, None,
                 None, None, 2, cols, stream(), why=why)

    res(p, 0, None, 0, 260, "dy_scale / dy_ntok need cols")
    res(None, 5, None, 0, 260, "dy_scale / dy_ntok need cols")
    res(None, -1, None, 0, 768, "dy_ntok < 0")
    res(None, 0, p, code(F32), 768, "lp_dt must be")

    def scaled(why, rows=2, cols=768, target=NC.TARGET, use=1, lp=p):
        """one argument of a call that passes every check changed.  use, target and lp share one
        check and one message, which names all three"""
        rejected("dclip_layernorm_bwd_scaled", p, code(F32), None, p, code(F32), p, p, p, None, p, lp, None, None, None, rows,
                 cols, target, p, use, p, stream(), why=why)
        rejected("dclip_layernorm_bwd_scaled_add", p, code(F32), None, p, p, p, p, None, p, code(BF16), None, 5, p, lp, None,
                 None, None, rows, cols, target, p, use, p, stream(), why=why)

    scaled("use >= 1", use=0)
    scaled("target > 0", target=0.0)
    scaled(": lp, ", lp=None)
    scaled("cols must be", cols=256)
    scaled("rows must be > 0", rows=0)
    for cols, lp, why in ((256, p, "cols must be"), (768, None, "lp (F16 or BF16) is required")):
        rejected("dclip_layernorm_bwd_add", p, code(F32), p, p, p, p, None, p, 5, p, lp, code(BF16), None, None, None, 2, cols,
                 stream(), why=why)


@cases("ln_bwd_add")
def test_layernorm_bwd_add(c):
    """dclip_layernorm_bwd_add to the bounds, NaN in add's CLS rows, and bit for bit what
    dclip_layernorm_bwd_res followed by dclip_add_readout_cast give (dw / db too where their order is fixed)"""
    inp = NC.fused_inputs(c)
    rows, cols, ntok = c["rows"], c["cols"], c["ntok"]
    b = Backward(c, inp)
    gadd = gcopy(inp["add"])
    outs = b.run(lambda: NT().call("dclip_layernorm_bwd_add", b.gdy.ptr(), code(c["dydt"]), b.gx.ptr(), b.gw.ptr(),
                                   b.gmean.ptr(), b.grstd.ptr(), ptr(b.res), gadd.ptr(), ntok, b.dx.ptr(), b.lp.ptr(),
                                   code(c["lp"]), ptr(b.dw), ptr(b.db), ptr(b.ws), rows, cols, stream()), [gadd])
    outs = check("ln_bwd_add", c, inp, outs)

    two = Backward(c, dict(inp, mean=inp["mean"], rstd=inp["rstd"]), with_lp=False)
    lp2 = guarded((rows, cols), c["lp"])

    def passes():
        NT().call("dclip_layernorm_bwd_res", two.gdy.ptr(), code(c["dydt"]), None, 0, two.gx.ptr(), code(F32), two.gw.ptr(),
                  two.gmean.ptr(), two.grstd.ptr(), ptr(two.res), two.dx.ptr(), None, 0, ptr(two.dw), ptr(two.db),
                  ptr(two.ws), rows, cols, stream())
        NT().call("dclip_add_readout_cast", two.dx.ptr(), gadd.ptr(), code(BF16), two.dx.ptr(), lp2.ptr(), code(c["lp"]), rows,
                  cols, ntok, 1.0, stream())

    two.outputs.append(lp2)
    two.names_out.append(("lp", c["lp"]))
    ref = {k: v.cpu() for k, v in two.run(passes, [gadd]).items()}
    names = ["dx", "lp"] + ([k for k in ("dw", "db") if k in ref] if b.ordered else [])
    NC.hold(f"ln_bwd_add {NC.norm_case_id(c)} against the two passes", [(k, ref[k], None) for k in names], outs,
            WORST.setdefault((ENTRY["ln_bwd_add"] + " = two passes", NC.dtype_key(c)), {}))


@cases("ln_bwd_scaled")
def test_layernorm_bwd_scaled(c):
    """dclip_layernorm_bwd_scaled and _scaled_add: uses 1 .. 5 of one delayed-scale state, dx to the
    bounds, lp = (f16)(dx s) and every word of the state and of spair bit for bit after each use"""
    def step(cu, inp):
        rows, cols = cu["rows"], cu["cols"]
        nonfinite = cu["use"] == NC.INF_USE
        b = Backward(cu, inp, nonfinite, null=NC.fused_null(cu))
        gs = scalar(NC.DY_SCALE) if cu["dsc"] else None
        gadd, gasc = gcopy(inp["add"]), (scalar(NC.ADD_SCALE) if cu["asc"] else None)
        spair = b.add_out("spair", 2, F32)
        st = io(inp["st"])
        if cu["entry"] == "scaled":
            def call():
                NT().call("dclip_layernorm_bwd_scaled", b.gdy.ptr(), code(cu["dydt"]), ptr(gs), b.gx.ptr(), code(F32),
                          b.gw.ptr(), b.gmean.ptr(), b.grstd.ptr(), ptr(b.res), b.dx.ptr(), b.lp.ptr(), ptr(b.dw), ptr(b.db),
                          ptr(b.ws), rows, cols, NC.TARGET, st[0].ptr(), cu["use"], spair.ptr(), stream())
        else:
            def call():
                NT().call("dclip_layernorm_bwd_scaled_add", b.gdy.ptr(), code(cu["dydt"]), ptr(gs), b.gx.ptr(), b.gw.ptr(),
                          b.gmean.ptr(), b.grstd.ptr(), ptr(b.res), gadd.ptr(), code(cu["adt"]), ptr(gasc), cu["ntok"],
                          b.dx.ptr(), b.lp.ptr(), ptr(b.dw), ptr(b.db), ptr(b.ws), rows, cols, NC.TARGET, st[0].ptr(),
                          cu["use"], spair.ptr(), stream())
        outs = b.run(call, [g for g in (gs, gadd, gasc) if g], [("st", torch.int32, st)])
        return {k: v.cpu() for k, v in outs.items()}

    NC.run_sequence("ln_bwd_scaled", c, step, worst_of("ln_bwd_scaled", c))


# ----------------------------------------------------------------------------- read-out folds
def readout_buffers(c, inp, nonfinite=False):
    """a, b and sum (aliasing a or not): (a's pointer, b, sum, outputs, in-out arguments)"""
    gb = gcopy(inp["b"])
    if c["alias"]:
        s = io(inp["a"], nonfinite)
        return s[0].ptr(), gb, s[0], [gb], [], [s]
    ga = gcopy(inp["a"])
    s = out(inp["a"].shape, F32, nonfinite)
    return ga.ptr(), gb, s, [ga, gb], [s], []


@cases("readout_cast")
def test_add_readout_cast(c):
    """add_readout_cast_kernel: sum (one f32 addition) and lp bit for bit, NaN in b's CLS rows, sum aliasing a"""
    inp = NC.readout_inputs(c)
    rows, cols = c["rows"], c["cols"]
    pa, gb, s, inputs, outputs, inout = readout_buffers(c, inp)
    lp = guarded((rows, cols), c["lp"])
    res = run_poisoned(lambda: NT().call("dclip_add_readout_cast", pa, gb.ptr(), code(c["bdt"]), s.ptr(), lp.ptr(),
                                         code(c["lp"]), rows, cols, c["ntok"], c["scale"], stream()),
                       inputs=inputs, outputs=outputs + [lp], inout=inout)
    check("readout_cast", c, inp, {"sum": res[1] if c["alias"] else res[0], "lp": res[0] if c["alias"] else res[1]})


@cases("readout_amax")
def test_add_readout_amax(c):
    """add_readout_amax_kernel: sum to its bound, ws = (s, 1 / s, 0, 0) of the sum that was written, bit for bit"""
    inp = NC.readout_inputs(c)
    rows, cols = c["rows"], c["cols"]
    pa, gb, s, inputs, outputs, inout = readout_buffers(c, inp)
    gasc = scalar(NC.ADD_SCALE) if c["asc"] else None
    ws = io(torch.zeros(4, dtype=torch.int32))
    res = run_poisoned(lambda: NT().call("dclip_add_readout_amax", pa, gb.ptr(), code(c["bdt"]), ptr(gasc), s.ptr(), rows,
                                         cols, c["ntok"], NC.TARGET, ws[0].ptr(), stream()),
                       inputs=inputs + ([gasc] if gasc else []), outputs=outputs, inout=inout + [ws])
    check("readout_amax", c, inp, {"sum": res[0], "ws": res[-1][0]})


@cases("readout_scaled")
def test_add_readout_cast_scaled(c):
    """add_readout_cast_ds_kernel through uses 1 .. 5 of one state (an odd chunk count at rows = 1029);
    b = NULL: sum is not written (it stays poisoned) and lp is a's cast"""
    def step(cu, inp):
        rows, cols = cu["rows"], cu["cols"]
        nonfinite = cu["use"] == NC.INF_USE
        gasc = scalar(NC.ADD_SCALE) if cu["asc"] else None
        lp, spair, st = out((rows, cols), F16, nonfinite), guarded(2, F32), io(inp["st"])
        if cu["bnull"]:
            ga, s = gcopy(inp["a"]), guarded((rows, cols), F32, fill=POISON)
            pa, pb, inputs, outputs, inout = ga.ptr(), None, [ga, s], [], []
        else:
            pa, gb, s, inputs, outputs, inout = readout_buffers(cu, inp, nonfinite)
            pb = gb.ptr()
        res = run_poisoned(lambda: NT().call("dclip_add_readout_cast_scaled", pa, pb, code(cu["bdt"]), ptr(gasc), s.ptr(),
                                             lp.ptr(), rows, cols, cu["ntok"], NC.TARGET, st[0].ptr(), cu["use"], spair.ptr(),
                                             stream()),
                           inputs=inputs + ([gasc] if gasc else []), outputs=outputs + [lp, spair], inout=inout + [st])
        outs = {"lp": typed(res[len(outputs)], F16), "spair": res[len(outputs) + 1], "st": res[-1][0]}
        if cu["bnull"]:
            assert still(s, POISON), "sum was written though b is NULL"
        else:
            outs["sum"] = typed(res[-2] if cu["alias"] else res[0], F32)
        return {k: v.cpu() for k, v in outs.items()}

    NC.run_sequence("readout_scaled", c, step, worst_of("readout_scaled", c))


def test_add_readout_arguments():
    d = guarded(16384, F32)
    p, st = d.ptr(), stream()
    # cols % 8, a pointer 4 bytes off, ntok = 0 (which shares the check, and the message, of cols)
    for cols, q, ntok, why in ((12, p, 3, "cols"), (8, p + 4, 3, "unaligned"), (8, p, 0, "cols")):
        rejected("dclip_add_readout_cast", q, p, code(F32), p, p, code(F16), 2, cols, ntok, 1.0, st, why=why)
        rejected("dclip_add_readout_amax", q, p, code(F32), None, p, 2, cols, ntok, NC.TARGET, p, st, why=why)
        rejected("dclip_add_readout_cast_scaled", q, p, code(F32), None, p, p, 2, cols, ntok, NC.TARGET, p, 1, p, st, why=why)


# ----------------------------------------------------------------------------- gradient scale, stochastic depth
@cases("grad_scale")
def test_grad_scale(c):
    """grad_scale_kernel: the unrolled loop, the single-load loop and block 0's scalar tail, the
    maximum in each of them; ws bit for bit after a call and after a second one on the same ws"""
    inp = NC.grad_scale_inputs(c)
    n = c["n"]
    pad = torch.full((max(n, 4),), float("nan"))  # n = 0 still passes a valid pointer
    g1, g2 = pad.clone(), pad.clone()
    g1[:n], g2[:n] = inp["g"], inp["g2"]
    g1, g2 = gcopy(g1), gcopy(g2)
    ws = io(torch.zeros(4, dtype=torch.int32))
    res = run_poisoned(lambda: NT().call("dclip_grad_scale", g1.ptr(), n, NC.TARGET, ws[0].ptr(), stream()),
                       inputs=[g1], inout=[ws])
    NT().call("dclip_grad_scale", g2.ptr(), n, NC.TARGET, ws[0].ptr(), stream())  # ws[2], ws[3] as the first call left them
    assert bool(ws[0].intact())
    check("grad_scale", c, inp, {"ws": res[0][0], "ws2": ws[0].m[0].clone()})


def test_grad_scale_arguments():
    d = guarded(64, F32)
    p, st = d.ptr(), stream()
    rejected("dclip_grad_scale", p + 4, 8, NC.TARGET, p, st, why="16-byte aligned")
    rejected("dclip_grad_scale", p, 8, 0.0, p, st, why="bad arguments")
    rejected("dclip_grad_scale", p, 8, -1.0, p, st, why="bad arguments")
    rejected("dclip_grad_scale", p, 8, NC.TARGET, None, st, why="bad arguments")


@cases("row_scale_add")
def test_row_scale_add(c):
    """row_scale_add_kernel with s in {0, 1 / keep}: bit for bit, x NULL, separate or aliasing out"""
    inp = NC.row_scale_add_inputs(c)
    rows, cols = c["ntok"] * c["B"], c["cols"]
    gy, gs = gcopy(inp["y"]), gcopy(inp["s"])
    if c["x"] == "alias":
        o = io(inp["x"])
        px, po, inputs, outputs, inout = o[0].ptr(), o[0].ptr(), [gy, gs], [], [o]
    else:
        gx, o = gcopy(inp["x"]), guarded((rows, cols), F32)
        px, po, inputs, outputs, inout = ptr(gx), o.ptr(), [g for g in (gx, gy, gs) if g], [o], []
    res = run_poisoned(lambda: NT().call("dclip_row_scale_add", px, gy.ptr(), gs.ptr(), c["ntok"], po, rows, cols, stream()),
                       inputs=inputs, outputs=outputs, inout=inout)
    check("row_scale_add", c, inp, {"out": res[0]})


def test_row_scale_add_arguments():
    d = guarded(4096, F32)
    p, st = d.ptr(), stream()
    rejected("dclip_row_scale_add", None, p, p, 5, p, 10, 6, st, why="cols % 4 == 0")
    rejected("dclip_row_scale_add", None, p, p, 5, p, 12, 8, st, why="rows a multiple of ntok")
