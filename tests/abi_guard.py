"""Guard-banded, poisoned buffers for tests that call the C ABI directly (test_gpu_abi_contract.py,
test_gpu_gemm_contract.py, test_gpu_conv_contract.py, test_gpu_misc_contract.py,
test_gpu_norm_contract.py, test_gpu_silog_contract.py, test_gpu_ade20k.py,
test_gpu_cityscapes_contract.py).

The op layer allocates every output and workspace with at::empty, and the caching allocator hands a
second call the block the first one just freed — still holding the first call's (correct) result.
A row a kernel never writes, or a workspace partial it reads before writing, then looks right.
Here every buffer is a slice of one flat uint8 allocation

    [ 1 MiB guard | payload | 1 MiB guard ]

with both guards filled with 0xFF (NaN as f32, f16 and bf16) and the payload with a byte of the
caller's choice, so that
  * an input is followed (and preceded) by NaN: a tile that reads past the last row and multiplies
    what it read by zero gives NaN instead of 0;
  * an out-of-bounds write of up to 1 MiB lands in a guard, harmlessly, and is seen by check();
  * run_poisoned() runs an entry point on outputs / workspaces pre-filled with 0xFF and again with
    0x3C (finite in every dtype): NaN after the first run means something was read before it was
    written, a difference between the runs means an output depends on what the buffers held.
Workspaces are sized by the library's own queries, never smaller.
A matrix with a leading dimension larger than its width (guarded_matrix) ends at its last valid
element; its gap columns hold NaN when it is an input and must come back untouched when it is an
output.  GuardedStrided is the same for any strided view: batches of matrices, strided pixel rows.
"""
import contextlib

import torch

DEV = "cuda"
GUARD = 1 << 20
POISON, FINITE = 0xFF, 0x3C


class Guarded:
    """A typed tensor `t` of `shape` inside [1 MiB 0xFF | payload | 1 MiB 0xFF]: the payload starts
    256-B aligned and the trailing guard at the first byte after its last element."""

    def __init__(self, shape, dtype, fill=0):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.empty(GUARD + 256 + self.nbytes + GUARD, dtype=torch.uint8, device=DEV)
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.raw.fill_(POISON)
        self.t = self.raw[self.off:self.off + self.nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % 256 == 0 and self.t.data_ptr() == self.raw.data_ptr() + self.off
        self.fill(fill)

    def fill(self, byte):
        self.raw[self.off:self.off + self.nbytes] = byte

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        """0-d bool tensor (no synchronisation): both guards still all 0xFF"""
        return (self.raw[:self.off] == POISON).all() & (self.raw[self.off + self.nbytes:] == POISON).all()

    def check(self):
        assert bool(self.intact()), "a guard band was written: out-of-bounds write"


def guarded(nbytes_or_shape, dtype=torch.uint8, fill=0):
    return Guarded(nbytes_or_shape, dtype, fill)


def guarded_copy(t):
    """`t`'s values in a guarded buffer: NaN follows the last element"""
    g = Guarded(t.shape, t.dtype)
    g.t.copy_(t)
    return g


class GuardedMatrix(Guarded):
    """A (rows, cols) matrix with leading dimension `ld` >= cols in a guarded payload of exactly
    (rows - 1) * ld + cols elements, so the trailing guard starts at the first byte after the last
    valid element.  `t`: the whole payload (flat); `m`: the (rows, cols) strided view; `gap`: the gap
    columns [cols, ld) of rows 0 .. rows - 2.  The whole payload, gaps included, is filled with
    `fill`: 0xFF for an input (write its values through `m`), so that a kernel that reads `ld`
    elements of a row instead of `cols` poisons its result."""

    def __init__(self, rows, cols, ld, dtype, fill=0):
        rows, cols, ld = int(rows), int(cols), int(ld)
        assert rows >= 1 and ld >= cols >= 1
        super().__init__((rows - 1) * ld + cols, dtype, fill)
        self.rows, self.cols, self.ld = rows, cols, ld
        self.m = self.t.as_strided((rows, cols), (ld, 1))
        self.gap = self.t[:(rows - 1) * ld].view(rows - 1, ld)[:, cols:]


def guarded_matrix(rows, cols, ld, dtype, fill=0):
    return GuardedMatrix(rows, cols, ld, dtype, fill)


def guarded_matrix_copy(t, ld):
    """the 2-d tensor `t`'s values with leading dimension `ld`, NaN in the gaps and behind the last element"""
    g = GuardedMatrix(t.shape[0], t.shape[1], ld, t.dtype, POISON)
    g.m.copy_(t)
    return g


class GuardedStrided(Guarded):
    """A tensor of `shape` with arbitrary non-overlapping `strides` (in elements) starting `offset`
    elements into a guarded payload that ends at the view's last element: a batch of matrices with a
    batch stride and a leading dimension, or the library's strided pixel rows (guarded_rows_copy).
    `t`: the whole payload (flat), filled with `fill` throughout (0xFF for an input: whatever lies
    between the valid elements holds NaN); `m`: the strided view; `gap`: the payload's elements
    outside `m` (a copy, in order), which an output must bring back untouched."""

    def __init__(self, shape, strides, dtype, fill=0, offset=0):
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        assert len(shape) == len(strides) and min(shape) >= 1 and min(strides) >= 1 and offset >= 0
        super().__init__(int(offset) + sum((n - 1) * s for n, s in zip(shape, strides)) + 1, dtype, fill)
        self.m = self.t.as_strided(shape, strides, self.t.storage_offset() + int(offset))  # absolute in the storage
        outside = torch.ones(self.t.shape, dtype=torch.bool, device=self.t.device)
        outside.as_strided(shape, strides, int(offset)).fill_(False)
        assert int(outside.numel() - outside.sum()) == self.m.numel(), "overlapping strides"
        self._outside = outside

    @property
    def gap(self):
        return self.t[self._outside]


def guarded_strided_copy(t, strides, offset=0):
    """`t`'s values at `strides` from `offset`, NaN everywhere else and behind the last element"""
    g = GuardedStrided(t.shape, strides, t.dtype, POISON, offset)
    g.m.copy_(t)
    return g


def guarded_rows_copy(t, ld, row_off):
    """The (batch, rows, cols) tensor `t` as the library's strided pixel rows: row r of image b at
    b * bstride + (row_off + r) * ld, bstride = (row_off + rows) * ld.  row_off = 1, ld = cols is a
    ViT token buffer whose CLS rows are skipped (they hold NaN here); row_off = 0, ld > cols a
    channel slice of a wider map.  Returns (buffer, bstride); the layout's base is buffer.ptr()."""
    bstride = (row_off + t.shape[1]) * ld
    return guarded_strided_copy(t, (bstride, ld, 1), row_off * ld), bstride


def valid(g):
    """the elements of a guarded buffer a kernel may write: the matrix view, or the whole payload"""
    return getattr(g, "m", g.t)


def bits(t):
    """integer view for bitwise comparisons (NaN == NaN, -0 != +0)"""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def bitwise_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def run_poisoned(fn, inputs=(), outputs=(), scratch=(), accum=(), inout=()):
    """Call `fn()` (one entry point through _native.call, on the current stream) twice on the same
    inputs: with `outputs` and `scratch` (Guarded) filled with 0xFF, then with 0x3C; `accum`
    (accumulating arguments the caller initialises by contract) zeroed before each; `inout`, pairs
    (GuardedMatrix, values) of arguments the entry point reads and overwrites (an aliased side
    input), set to `values` before each with 0xFF in the gaps.  Then, in this order: every guard of
    every buffer intact, the 0xFF run's outputs all finite, the two runs' outputs bitwise equal, and
    the gap columns of every GuardedMatrix among them bitwise what they were on entry, after both
    runs.  Returns the outputs' (then the accumulators', then the in-out arguments') valid elements."""
    runs, gaps = [], []
    written = tuple(outputs) + tuple(accum) + tuple(g for g, _ in inout)
    for byte in (POISON, FINITE):
        for g in tuple(outputs) + tuple(scratch):
            g.fill(byte)
        for g in accum:
            g.fill(0)
        for g, values in inout:
            g.fill(POISON)
            g.m.copy_(values)
        entry = [bits(g.gap) if hasattr(g, "gap") else None for g in written]
        fn()
        runs.append([valid(g).clone() for g in written])
        gaps.append([(bits(g.gap) == e).all() if e is not None else None for g, e in zip(written, entry)])
    ok = [g.intact() for g in tuple(inputs) + tuple(outputs) + tuple(scratch) + tuple(accum)
          + tuple(g for g, _ in inout)]
    torch.cuda.synchronize()
    broken = [i for i, v in enumerate(ok) if not bool(v)]
    assert not broken, f"out-of-bounds write: guard bands of buffers {broken} (inputs, outputs, scratch, accum) changed"
    for i, t in enumerate(runs[0]):
        assert bool(torch.isfinite(t).all()), \
            f"output {i}: {int((~torch.isfinite(t)).sum())} non-finite values after the 0xFF run (read before written)"
    for i, (a, b) in enumerate(zip(*runs)):
        assert bitwise_equal(a, b), \
            f"output {i} depends on the buffers' contents on entry ({int((bits(a) != bits(b)).sum())} elements differ)"
    for run, byte in zip(gaps, (POISON, FINITE)):
        for i, v in enumerate(run):
            assert v is None or bool(v), \
                f"output {i}: the columns between its width and its leading dimension were written (0x{byte:02X} run)"
    return runs[0]


@contextlib.contextmanager
def option_scope():
    """yields set(option id, value); every option touched is back at 0 on exit"""
    from denseclip_vit_multimodal_amd import _native as NT
    touched = []

    def set_option(opt, value):
        touched.append(opt)
        NT.call("dclip_set_option", opt, int(value))

    try:
        yield set_option
    finally:
        for opt in touched:
            NT.call("dclip_set_option", opt, 0)
