"""dclip_gemm (and dclip_gemm_tn's STORE epilogue) through the C ABI on guard-banded, poisoned,
STRIDED buffers (abi_guard.py), every output against an fp64 reference per 32 x 64 block and per
element (gemm_check.py: the reference, the bounds and why they hold).

What test_gpu_kernels.py cannot see:
  * the persistent kernel away from the workload's own size.  launch_pers (gemm.hip) takes a shape
    only with N % 256 == 0, an M tail of <= 64 rows and >= 2 x CU count full 256 x 256 tiles; P1 and
    P2 below are the smallest such shapes on 256 CUs at N = 3072 (streaming stores) and N = 768 (plain
    stores), K = 128, and every persistent case asserts those conditions before it runs;
  * the three M-tail paths and their boundaries: tails 0, 1, 8, 16, 17, 64 and 65 rows, and the K
    that select gemm_tail16x16_kernel (64, 768, 3072), gemm_tail16_kernel (4096) and the split-K
    scratch + tail_combine_kernel (3200; any K for 17 .. 64 rows), each with every epilogue, with
    alpha = 0.5 * *alpha_ptr (0.25) in half of the cases and bias == NULL in half;
  * leading dimensions: lda = K + 8, ldb = K + 16, ldc = N + 8, ldc2 = N + 16, ld_aux = N + 24.  The
    gap columns of an input hold NaN, those of an output must come back untouched, and every
    matrix ends at its last valid element, against a 1 MiB band of NaN;
  * outputs that do not already hold the answer: every output and workspace enters as 0xFF, then as
    0x3C (run_poisoned);
  * one wrong piece in a large output: blocks of 32 x 64 and single elements, not one norm.
Options move one at a time from the default on P1 (8 tail rows) and P2 (24 tail rows), every row
against the fp64 reference; the grid kernels (tiles 1-5) run at ragged edges, launch_big's own
M-tail split at the smallest shape that takes it per tile, and dclip_gemm's SPLITK with 1, 2 and 4
splits.

The CPU emulation of the kernels (test_gemm_contract_emulation_cpu.py: torch's f32 product, f32
epilogue, outputs rounded; 4 small shapes x 5 seeds) through the same checker has its worst figures
at these fractions of the bounds: blocked, f32 outputs 0.036 (fp16 operands) / 0.015 (bf16), 16-bit
outputs 0.12 (fp16) / 0.16 (bf16), h of the z-less GELU form (held to the exact z) 0.19 / 0.24;
elementwise, f32 outputs 0.15 / 0.12, 16-bit outputs 0.99 / 0.995 (a value just above a power of
two, rounded by half an ulp, is at 2^-p |ref| by itself; the accumulation term is the headroom).
The kernels on the MI355X over all rows of this file, next to that emulation (worst figure / bound,
fp16 | bf16 operands; "blk" the blocked check, "el" the elementwise one):
    form            output   kernels blk    emulation blk   kernels el     emulation el
    store32         C        0.046 | 0.045  0.036 | 0.015   0.125 | 0.124  0.055 | 0.048
    store16         C        0.119 | 0.160  0.111 | 0.147   0.997 | 0.996  0.989 | 0.995
    scaled          C        0.123 | 0.163  0.112 | 0.151   0.994 | 0.995  0.988 | 0.992
    gelu            C (z)    0.121 | 0.160  0.110 | 0.146   0.993 | 0.995  0.985 | 0.994
    gelu            C2 (h)   0.126 | 0.169  0.119 | 0.159
    gelu_h          C2 (h)   0.196 | 0.269  0.187 | 0.241
    resid           C        0.029 | 0.028  0.026 | 0.011   0.177 | 0.173  0.122 | 0.083
    resid_lp        C        0.032 | 0.032  0.025 | 0.011   0.101 | 0.114  0.125 | 0.098
    resid_lp        C2       0.114 | 0.150  0.109 | 0.149   0.997 | 0.996  0.984 | 0.995
    resid_inplace   C        0.032 | 0.032  0.026 | 0.011   0.101 | 0.114  0.147 | 0.124
    gelu_bwd        C        0.116 | 0.155  0.111 | 0.149
    splitk          C        0.016 | 0.014  0.036 | 0.015   0.009 | 0.009  0.066 | 0.053
    gemm_tn STORE   C        0.010 | 0.008                  0.017 | 0.018
(the f32 outputs sit higher on the kernels than in the emulation because these shapes are larger and
K reaches 4096; every figure is far from its bound except the 16-bit rounding itself).
"""
import collections

import pytest
import torch

import gemm_check as GC
from abi_guard import (guarded, guarded_copy, guarded_matrix, guarded_matrix_copy, option_scope, run_poisoned)
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
F32 = torch.float32
NT_FORMS = [f for f in GC.FORMS if f != "splitk"]  # SPLITK never takes the persistent path: its own test
# the smallest shapes launch_pers takes on 256 CUs: (full rows, N); K = 128 unless a test says otherwise
PERS = {"P1": (43 * 256, 3072),   # 43 x 12 = 516 tiles; N >= 2048: streaming stores
        "P2": (171 * 256, 768)}   # 171 x 3 = 513 tiles; plain stores
WORST = {}  # (form, dtype) -> {(output, check): worst figure / bound} over this session


@pytest.fixture(autouse=True)
def _need(hip):
    pass


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (form, dt), w in sorted(WORST.items(), key=str):
        print(f"\ngemm contract {form} {dt}: worst figure / bound "
              + ", ".join(f"{n} {c} {v:.3f}" for (n, c), v in sorted(w.items())), end="")


def NT():
    from denseclip_vit_multimodal_amd import _native
    return _native


def code(dt):
    return {torch.float16: NT().F16, torch.bfloat16: NT().BF16, torch.float32: NT().F32}[dt]


def stream():
    return torch.cuda.current_stream().cuda_stream


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_launch_pers(M, N, takes_tail=True):
    """The conditions under which launch_pers (gemm.hip) takes a shape, asserted before a case that
    is meant to run the persistent kernel; with takes_tail False, that it declines for the tail alone
    (> 64 rows: the grid kernel).  Skips when the CU count makes the shape too small."""
    G = cu_count()
    full, tail = (M // 256) * (N // 256), M % 256
    if full < 2 * G:
        pytest.skip(f"{full} full tiles < 2 x {G} CUs: launch_pers declines this shape on this part")
    assert N % 256 == 0 and full >= 2 * G
    assert (tail <= 64) == takes_tail, (M, tail)


# ----------------------------------------------------------------------------- operands and references (computed once)
class Master:
    """The operands of one (Mmax, N, K, dtype) in guarded buffers, strided and contiguous, and
    A B^T and |A| |B|^T in fp64 — read-only; a case with M <= Mmax rows uses their first M rows."""

    def __init__(self, Mmax, N, K, dt):
        self.Mmax, self.N, self.K, self.dt = Mmax, N, K, dt
        self.o = o = GC.operands(Mmax, N, K, dt, 7 * Mmax + 3 * N + K, DEV)
        A64, B64 = o["A"].double(), o["B"].double()
        self.acc = A64 @ B64.t()
        self.absacc = A64.abs() @ B64.abs().t()
        self.gB = {True: guarded_matrix_copy(o["B"], K + 16), False: guarded_copy(o["B"])}
        self.gbias, self.gscale = guarded_copy(o["bias"]), guarded_copy(o["scale"])
        self.galpha = guarded_copy(torch.tensor([0.25], device=DEV))
        self._a = {}

    def a(self, M, strided):
        if (M, strided) not in self._a:
            rows = self.o["A"][:M]
            self._a[M, strided] = guarded_matrix_copy(rows, self.K + 8) if strided else guarded_copy(rows)
        return self._a[M, strided]


_MASTERS = collections.OrderedDict()


def master(Mmax, N, K, dt):
    key = (Mmax, N, K, dt)
    if key in _MASTERS:
        _MASTERS.move_to_end(key)
    else:
        while len(_MASTERS) >= 3:  # a few hundred MB each
            _MASTERS.popitem(last=False)
        _MASTERS[key] = Master(Mmax, N, K, dt)
    return _MASTERS[key]


class Call:
    """One dclip_gemm call of `form` on the first M rows of a Master: its guarded buffers, fn() (the
    call on the current stream) and finish(results) (the checks against fp64).  `case` picks alpha
    (odd: 0.5 with alpha_ptr -> 0.25, even: 1 and NULL) and the bias (bit 1 set: given, else NULL)."""

    def __init__(self, ms, M, form, case, strided=True, splits=1):
        L = NT()
        dt, N, K = ms.dt, ms.N, ms.K
        self.ms, self.M, self.form = ms, M, form
        pad = (lambda n: n) if strided else (lambda n: 0)
        lda, ldb, ldc, ldc2, ld_aux = K + pad(8), K + pad(16), N + pad(8), N + pad(16), N + pad(24)
        self.alpha = 0.125 if case & 1 else 1.0
        self.bias = ms.o["bias"] if case & 2 else None
        gA, gB = ms.a(M, strided), ms.gB[strided]
        self.inputs = [gA, gB, ms.gbias, ms.gscale, ms.galpha]
        self.outputs, self.scratch, self.inout, self.names = [], [], [], []
        res, z0 = ms.o["res"][:M], ms.o["z0"][:M]
        C = C2 = aux = None
        aux_dt, c_dt = L.F32, code(dt)

        def out(name, odt, ld):
            g = guarded_matrix(M, N, ld, odt)
            self.outputs.append(g)
            self.names.append(name)
            return g

        if form == "store32":
            epi, C, c_dt = L.EPI_STORE, out("C", F32, ldc), L.F32
        elif form == "store16":
            epi, C = L.EPI_STORE, out("C", dt, ldc)
        elif form == "scaled":
            epi, C, aux, ld_aux = L.EPI_STORE_SCALED, out("C", dt, ldc), ms.gscale, N
        elif form == "gelu":
            epi, C, C2 = L.EPI_GELU, out("C", dt, ldc), out("C2", dt, ldc2)
        elif form == "gelu_h":
            epi, C2 = L.EPI_GELU, out("C2", dt, ldc2)
        elif form in ("resid", "resid_lp"):
            epi, c_dt = L.EPI_RESIDUAL, L.F32
            aux = guarded_matrix_copy(res, ld_aux)
            self.inputs.append(aux)
            C = out("C", F32, ldc)
            if form == "resid_lp":
                C2 = out("C2", dt, ldc2)
        elif form == "resid_inplace":  # aux aliases C: C is an input, set before each run, never poisoned
            epi, c_dt = L.EPI_RESIDUAL, L.F32
            C = aux = guarded_matrix(M, N, ldc, F32, 0xFF)
            ld_aux = ldc
            self.inout.append((C, res))
        elif form == "gelu_bwd":
            epi, aux_dt = L.EPI_GELU_BWD, code(dt)
            aux = guarded_matrix_copy(z0, ld_aux)
            self.inputs.append(aux)
            C = out("C", dt, ldc)
        elif form == "splitk":
            epi, c_dt = L.EPI_SPLITK, L.F32
            aux = guarded(splits * M * N, F32)
            self.scratch.append(aux)
            C = out("C", F32, ldc)
        else:
            raise KeyError(form)
        if form == "resid_inplace":
            self.names.append("C")
        ptr = lambda g: g.ptr() if g is not None else None  # noqa: E731
        args = (epi, code(dt), gA.ptr(), lda, gB.ptr(), ldb, M, N, K, splits,
                0.5 if case & 1 else 1.0, ms.galpha.ptr() if case & 1 else None,
                ms.gbias.ptr() if self.bias is not None else None, ptr(aux), aux_dt, ld_aux,
                ptr(C), c_dt, ldc, ptr(C2), ldc2)
        self.fn = lambda: L.call("dclip_gemm", *args, stream())
        self.what = (f"{form} M={M} N={N} K={K} {DT_IDS[DTS.index(dt)]} alpha {self.alpha} "
                     f"bias {'set' if self.bias is not None else 'null'} {'strided' if strided else 'contiguous'}"
                     + (f" splits {splits}" if form == "splitk" else ""))

    def run(self):
        return run_poisoned(self.fn, inputs=self.inputs, outputs=self.outputs, scratch=self.scratch,
                            inout=self.inout)

    def finish(self, results, what=""):
        ms, M = self.ms, self.M
        outs = dict(zip(self.names, results))
        refs = GC.references(self.form, ms.dt, ms.K, ms.acc[:M], ms.absacc[:M], self.alpha, self.bias,
                             ms.o["scale"], ms.o["res"][:M], ms.o["z0"][:M], outs)
        GC.check(what + self.what, refs, outs, WORST.setdefault((self.form, DT_IDS[DTS.index(ms.dt)]), {}))


def run_form(ms, M, form, case, strided=True, splits=1, what=""):
    c = Call(ms, M, form, case, strided, splits)
    c.finish(c.run(), what)


def pers_master(shape, K, dt):
    """P1 with up to 65 tail rows, P2 with up to 24: one Master per (shape, K, dtype) for every test"""
    mfull, N = PERS[shape]
    return master(mfull + (65 if shape == "P1" else 24), N, K, dt)


# ----------------------------------------------------------------------------- the tail scratch regrows
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_tail_scratch_regrowth(dt):
    """A 24-row tail at N = 768 (P2), a 64-row tail at N = 3072 (P1: eight times the scratch, so the
    library's tail scratch is freed and regrown unless an earlier test already grew it) and the first
    again, back to back on one stream, eager: all three against fp64.  First in the file, so that
    the scratch is as small as the session allows."""
    calls = []
    for i, (shape, tail) in enumerate([("P2", 24), ("P1", 64), ("P2", 24)]):
        mfull, N = PERS[shape]
        assert_launch_pers(mfull + tail, N)
        calls.append(Call(pers_master(shape, 128, dt), mfull + tail, "resid_lp", 3 * i + 1))
    results = run_poisoned(lambda: [c.fn() for c in calls], inputs=[g for c in calls for g in c.inputs],
                           outputs=[g for c in calls for g in c.outputs])
    for i, c in enumerate(calls):
        c.finish(results[2 * i:2 * i + 2], f"regrowth call {i}: ")


# ----------------------------------------------------------------------------- persistent kernel, every tail
TAIL_ROWS = [("P1", t, True) for t in (0, 1, 8, 16, 17, 64, 65)] + [("P2", 8, True), ("P2", 24, True),
                                                                    ("P1", 8, False)]  # the last: contiguous control


@pytest.mark.parametrize("form", NT_FORMS)
@pytest.mark.parametrize("shape,tail,strided", TAIL_ROWS,
                         ids=[f"{s}-tail{t}" + ("" if st else "-contiguous") for s, t, st in TAIL_ROWS])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_persistent_tails(dt, shape, tail, strided, form):
    """gemm_nt_pers_kernel on its smallest shapes with every M tail: none, gemm_tail16x16_kernel (1, 8,
    16 rows), the scratch path (17, 24, 64) and 65 rows, which launch_pers declines (the 256 x 256
    grid kernel must be as right)."""
    mfull, N = PERS[shape]
    assert_launch_pers(mfull + tail, N, takes_tail=tail <= 64)
    ms = pers_master(shape, 128, dt)
    run_form(ms, mfull + tail, form, TAIL_ROWS.index((shape, tail, strided)) + NT_FORMS.index(form), strided)


# ----------------------------------------------------------------------------- which tail kernel
@pytest.mark.parametrize("form", NT_FORMS)
@pytest.mark.parametrize("tail", [8, 16])
@pytest.mark.parametrize("K", [64, 768, 3072, 4096, 3200])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_tail_kernel_selection(dt, K, tail, form):
    """P1's geometry with the K that pick each tail kernel for <= 16 rows (launch_pers, tail16x16_plan):
    64 (2 waves x 1 step; also below the K >= 128 gates of the claim counters and of options 8 / 9),
    768 (12 x 2), 3072 (16 x 6): gemm_tail16x16_kernel; 4096 (no plan, K % 256 == 0):
    gemm_tail16_kernel; 3200 (no plan, K % 256 != 0): split-K scratch + tail_combine_kernel."""
    mfull, N = PERS["P1"]
    assert_launch_pers(mfull + tail, N)
    run_form(pers_master("P1", K, dt), mfull + tail, form, tail // 8 + K // 64 + NT_FORMS.index(form))


# ----------------------------------------------------------------------------- one option at a time
def option_rows():
    n = NT()
    rows = {f"tile{v}": (n.OPT_GEMM_TILE, v) for v in (0, 6, 7, 8, 9)}
    rows.update({f"epi{v}": (n.OPT_GEMM_EPI, v) for v in (1, 2, 3)})
    rows["sched1"] = (n.OPT_GEMM_SCHED, 1)
    rows.update({f"kloop{v}": (n.OPT_GEMM_KLOOP, v) for v in (1, 2)})
    rows.update({f"tail{v}": (n.OPT_GEMM_TAIL, v) for v in (1, 2)})
    return rows


OPTION_IDS = ["tile0", "tile6", "tile7", "tile8", "tile9", "epi1", "epi2", "epi3", "sched1", "kloop1", "kloop2",
              "tail1", "tail2"]


@pytest.mark.parametrize("form", NT_FORMS)
@pytest.mark.parametrize("row", OPTION_IDS)
@pytest.mark.parametrize("shape,tail", [("P1", 8), ("P2", 24)], ids=["P1-tail8", "P2-tail24"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_persistent_option_sweep(dt, shape, tail, row, form):
    """Every DCLIP_OPT_GEMM_* value that changes the persistent path, one at a time from the default,
    against fp64 (not against another variant): tiles 6-9, the three other epilogue store variants,
    the work-conserving walk, the K-loop schedules and the tail kernels."""
    rows = option_rows()
    assert sorted(rows) == sorted(OPTION_IDS)
    mfull, N = PERS[shape]
    assert_launch_pers(mfull + tail, N)
    ms = pers_master(shape, 128, dt)
    with option_scope() as set_option:
        set_option(*rows[row])
        run_form(ms, mfull + tail, form, OPTION_IDS.index(row) + NT_FORMS.index(form), what=f"{row}: ")


@pytest.mark.parametrize("form", ["store16", "gelu", "resid_lp"])
@pytest.mark.parametrize("K", [192, 256])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_work_conserving_walk_short_k(dt, K, form):
    """DCLIP_OPT_GEMM_SCHED 1 publishes the next tile's claim behind K-step nk - 3, or before the loop
    when nk == 2 (K = 128: the sweep above).  nk = 3 makes that K-step the tile's first, beside the
    round-0 ownership word; nk = 4 is the first with a K-step before it."""
    mfull, N = PERS["P1"]
    assert_launch_pers(mfull + 8, N)
    with option_scope() as set_option:
        set_option(NT().OPT_GEMM_SCHED, 1)
        run_form(pers_master("P1", K, dt), mfull + 8, form, K // 64 + NT_FORMS.index(form), what="sched1: ")


# ----------------------------------------------------------------------------- grid kernels at ragged edges
@pytest.mark.parametrize("form", NT_FORMS)
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("M,N,K", [(65, 72, 64), (257, 264, 128), (300, 200, 192)])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_grid_kernels_ragged(dt, M, N, K, tile, form):
    """gemm_nt_kernel (1), gemm_nt_big_kernel 256x256 / 256x128 / k32x4 (2, 3, 4) and gemm_nt_pp_kernel
    (5) with a partial last tile in both directions"""
    with option_scope() as set_option:
        set_option(NT().OPT_GEMM_TILE, tile)
        run_form(master(M, N, K, dt), M, form, tile + M + NT_FORMS.index(form), what=f"tile{tile}: ")


@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("M,N,K,strided", [(257, 264, 256, True), (300, 200, 512, True), (257, 264, 256, False)],
                         ids=["257-264-256", "300-200-512", "257-264-256-contiguous"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_gemm_splitk(dt, M, N, K, strided, tile, splits):
    """dclip_gemm's own EPI_SPLITK: the partial slabs in a poisoned workspace, then
    splitk_reduce_kernel with the bias and ldc = N + 8 (and one contiguous control)"""
    with option_scope() as set_option:
        set_option(NT().OPT_GEMM_TILE, tile)
        # bit 1 of the case (the bias) set for two of every three rows, alpha alternating
        run_form(master(M, N, K, dt), M, "splitk", (2 if (tile + splits) % 3 else 0) + (tile & 1), strided, splits,
                 what=f"tile{tile}: ")


# ----------------------------------------------------------------------------- launch_big's M-tail split
# launch_big (gemm.hip) splits a tail of <= 64 rows off when K >= 1536 and the tail's row of tiles adds a
# round of 256 workgroups: full_rows * tiles_n <= 256 < (full_rows + 1) * tiles_n.  Smallest shapes with
# a 24-row tail at N = 3072: 256 x 256 tiles (options 2, 4, 5, and 6-9 / 0 falling back): tiles_n = 12,
# 21 full rows (252 <= 256 < 264); 256 x 128 tiles (option 3): tiles_n = 24, 10 full rows (240 <= 256 < 264).
BIG_TAIL = {0: (21, 256), 2: (21, 256), 3: (10, 128), 4: (21, 256), 5: (21, 256)}


@pytest.mark.parametrize("form", NT_FORMS)
@pytest.mark.parametrize("tile", sorted(BIG_TAIL))
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_launch_big_tail_split(dt, tile, form):
    full_rows, tbn = BIG_TAIL[tile]
    M, N, K, tail = full_rows * 256 + 24, 3072, 1536, 24
    tiles_n = N // tbn
    assert K >= 1536 and tail <= 64 and full_rows * tiles_n <= 256 < (full_rows + 1) * tiles_n  # launch_big
    if tile == 0:  # automatic: the persistent choice, which must decline (launch_pers) for the grid kernel
        if full_rows * (N // 256) >= 2 * cu_count():
            pytest.skip(f"launch_pers takes {full_rows} x {N // 256} tiles on {cu_count()} CUs")
        assert M >= 4096
    with option_scope() as set_option:
        set_option(NT().OPT_GEMM_TILE, tile)
        run_form(master(M, N, K, dt), M, form, tile + NT_FORMS.index(form), what=f"tile{tile}: ")


# ----------------------------------------------------------------------------- dclip_gemm_tn, STORE
@pytest.mark.parametrize("colsum", [False, True], ids=["nocolsum", "colsum"])
@pytest.mark.parametrize("K,M,N", [(70, 136, 72), (200, 256, 264)])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_gemm_tn_store_strided(dt, K, M, N, colsum):
    """C = alpha A^T B with the STORE epilogue straight into a strided C (ldc = N + 8), lda = M + 8,
    ldb = N + 16: the small-tile kernel with K no multiple of 64 (70: the rows >= K of the last
    K-tile lie behind A's and B's last elements, in NaN) and the 256 x 256 kernel (200); colsum_a
    (accumulated: zeroed before each run; one block row over all of K, so in a fixed order) set
    and null."""
    L = NT()
    g = torch.Generator(device=DEV).manual_seed(11 * K + M)
    A = torch.randn(K, M, device=DEV, generator=g).to(dt)
    Bm = (torch.randn(K, N, device=DEV, generator=g) * K ** -0.5).to(dt)
    gA, gB = guarded_matrix_copy(A, M + 8), guarded_matrix_copy(Bm, N + 16)
    galpha = guarded_copy(torch.tensor([0.25], device=DEV))
    scaled = bool(colsum) == (K == 70)
    alpha = 0.125 if scaled else 1.0
    out = guarded_matrix(M, N, N + 8, F32)
    cs = [guarded(M, F32)] if colsum else []
    k_pad = (K + 63) // 64 * 64
    assert k_pad > K
    res = run_poisoned(lambda: L.call("dclip_gemm_tn", L.EPI_STORE, code(dt), gA.ptr(), M + 8, gB.ptr(), N + 16, M, N,
                                      K, k_pad, 1, 0.5 if scaled else 1.0, galpha.ptr() if scaled else None, None,
                                      None, out.ptr(), N + 8, cs[0].ptr() if colsum else None, stream()),
                       inputs=[gA, gB, galpha], outputs=[out], accum=cs)
    A64, B64 = A.double(), Bm.double()
    refs = GC.references("store32", dt, K, A64.t() @ B64, A64.abs().t() @ B64.abs(), alpha)
    GC.check(f"gemm_tn STORE K={K} M={M} N={N} {dt} alpha {alpha}", refs, {"C": res[0]},
             WORST.setdefault(("tn_store", DT_IDS[DTS.index(dt)]), {}))
    if colsum:
        ec = rel_err(res[1], alpha * A64.sum(0))
        print(f"gemm_tn STORE colsum rel err {ec:.3e} (bound 1e-5)")
        assert ec < 1e-5, ec
