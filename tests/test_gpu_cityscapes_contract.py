"""The four entry points of csrc/data.hip (dclip_cityscapes_prepare, dclip_cityscapes_augment,
dclip_color_jitter, dclip_normalize_u8) through the C ABI on guard-banded, poisoned buffers
(abi_guard.run_poisoned), against oracle/data_oracle.py BIT FOR BIT: the pipeline is integer work plus
correctly rounded f32 steps in the reference's order, so there is no tolerance anywhere in this file.  A
16-bit image is the oracle's f32 result cast with torch.Tensor.to(dtype).  The cases, and what each is
there for, are in cityscapes_check.py; test_cityscapes_contract_emulation_cpu.py shows that each of
thirteen plausible slips, planted in the oracle, changes the expectation of at least one of them.

Then the op layer: torch.library.opcheck on torch.ops.dclip.cityscapes_prepare in its three forms, the
arguments it must refuse (every malformed tensor at least as large in bytes as the well-formed one, so that
a missing check gives wrong values, never an out-of-bounds read), and data.prepare_batch with ColorJitter
and an fp16 image.

Not covered: the grid-stride loops of prepare, augment and normalize_u8 are capped at 65536 blocks and
start only above 16.7M output pixels, which no small shape reaches; test_augment_full_resolution_batch
(test_gpu_data.py) remains the largest run of them.  The gray-mean reduction's loop (1024 blocks) does run
here, at 520 x 520."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cityscapes_check as C
from abi_guard import bitwise_equal, guarded, guarded_copy, guarded_matrix, run_poisoned
from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16, BF16, U8 = torch.float32, torch.float16, torch.bfloat16, torch.uint8
_name = lambda d: str(d).replace("torch.", "")  # noqa: E731


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def N():
    from denseclip_vit_multimodal_amd import _native
    return _native


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
    return {F32: N().F32, F16: N().F16, BF16: N().BF16, U8: N().U8}[dtype]


def _f3(v):
    return (ctypes.c_float * 3)(*v)


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """the oracle's outputs of a case, computed once and shared"""
    return C.expected(next(c for c in C.ALL_CASES if c["id"] == case_id))


def same_rows(what, got, want, row_ids):
    """bitwise per batch row; every row that differs is named before the assertion"""
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = [(row_ids[b], int((got[b].contiguous().view(torch.uint8) != want[b].contiguous().view(torch.uint8)).sum()))
           for b in range(len(want)) if not bitwise_equal(got[b], want[b])]
    print(f"{what}: {len(bad)} of {len(want)} rows differ bitwise {bad[:6]}")
    assert not bad, (what, bad)


def image_as(img_f32, dtype):
    return torch.from_numpy(img_f32).to(dtype)


class Prep:
    """a PREP case as guarded device buffers for direct calls of prepare / augment"""

    def __init__(self, case, norm=C.CLIP):
        self.case, self.norm = case, norm
        s = C.prep_samples(case)
        self.B, self.H, self.W, self.h, self.w = len(case["rows"]), case["H"], case["W"], case["h"], case["w"]
        assert len(s) == self.B
        self.img = guarded_copy(torch.from_numpy(np.stack([x[0] for x in s])).to(DEV))
        self.ids = guarded_copy(torch.from_numpy(np.stack([x[1] for x in s])).to(DEV))
        self.disp = guarded_copy(torch.from_numpy(np.stack([x[2] for x in s]).view(np.int16)).to(DEV))
        self.prm = guarded_copy(torch.tensor(case["rows"], dtype=torch.int32).to(DEV))
        self.seg = guarded((self.B, self.h, self.w), torch.int64)
        self.depth = guarded((self.B, self.h, self.w), F32)
        self.mask = guarded((self.B, self.h, self.w), U8)
        self.mean, self.std = _f3(norm[0]), _f3(norm[1])

    def run(self, dtype, entry=None, prm=None):
        """(image, seg, depth, mask) of one poisoned double run"""
        entry = entry or ("dclip_cityscapes_augment" if self.case["kind"] == "augment" else "dclip_cityscapes_prepare")
        prm = prm or self.prm
        shape = (self.B, self.h, self.w, 3) if dtype == U8 else (self.B, 3, self.h, self.w)
        out = guarded(shape, dtype)
        args = (self.img.ptr(), self.ids.ptr(), self.disp.ptr(), self.B, self.H, self.W, prm.ptr(), self.h, self.w,
                self.mean, self.std, self.case["bf"], self.case["depth_max"], out.ptr(), _dt(dtype), self.seg.ptr(),
                self.depth.ptr(), self.mask.ptr())
        return run_poisoned(lambda: N().call(entry, *args, _stream()), inputs=[self.img, self.ids, self.disp, prm],
                            outputs=[out, self.seg, self.depth, self.mask])

    def hold(self, outs, dtype, what):
        e, ids = expected(self.case["id"]), self.case["row_ids"]
        img, seg, depth, mask = outs
        same_rows(f"{what} image {_name(dtype)}", img, torch.from_numpy(e["u8"]) if dtype == U8 else image_as(e["img"], dtype), ids)
        same_rows(f"{what} seg", seg, e["seg"], ids)
        same_rows(f"{what} depth", depth, e["depth"], ids)
        same_rows(f"{what} mask", mask, e["mask"], ids)
        assert bool(((mask == 0) | (mask == 1)).all())


# ----------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("dtype", [F32, BF16, F16, U8], ids=_name)
@pytest.mark.parametrize("case", C.GEOM7, ids=lambda c: c["id"])
def test_augment_geometry(case, dtype):
    p = Prep(case)
    outs = p.run(dtype)
    p.hold(outs, dtype, case["id"])
    # PadIfNeeded: the normalised zero (the byte 0 for the uint8 crop), 255, 255.0 and mask 1
    img, seg, depth, mask = (t.cpu() for t in outs)
    pad = torch.from_numpy(C.padded(case))
    assert int(pad.sum()) > 0
    if dtype == U8:
        assert bool((img[pad] == 0).all())
    else:
        m = np.asarray(C.CLIP[0], np.float32) * np.float32(255)
        r = np.float32(1) / (np.asarray(C.CLIP[1], np.float32) * np.float32(255))
        zero = torch.from_numpy((np.float32(0) - m) * r).to(dtype)
        assert bitwise_equal(img.permute(0, 2, 3, 1)[pad], zero.expand(int(pad.sum()), 3).contiguous())
    assert bool((seg[pad] == 255).all()) and bool((depth[pad] == 255.0).all()) and bool((mask[pad] == 1).all())


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=_name)
@pytest.mark.parametrize("case", C.GEOM3, ids=lambda c: c["id"])
def test_prepare_windows_and_their_identity_in_augment(case, dtype):
    p = Prep(case)
    outs = p.run(dtype)
    p.hold(outs, dtype, case["id"])
    # identity parameters in augment = prepare, bit for bit
    ident = guarded_copy(torch.tensor([(case["H"], case["W"], 0, 0) + tuple(r) for r in case["rows"]], dtype=torch.int32).to(DEV))
    again = p.run(dtype, entry="dclip_cityscapes_augment", prm=ident)
    for name, a, b in zip(("image", "seg", "depth", "mask"), again, outs):
        same_rows(f"{case['id']} augment(identity) {name}", a, b.cpu(), case["row_ids"])


# ----------------------------------------------------------------------------- value domains
@pytest.mark.parametrize("case", C.DOMAINS, ids=lambda c: c["id"])
def test_every_label_id_and_every_disparity(case):
    from oracle import data_oracle as D
    p = Prep(case)
    dtype = U8 if case["kind"] == "augment" else F32
    outs = p.run(dtype)
    p.hold(outs, dtype, case["id"])
    (_, ids, disp), = C.domain_sample()
    seg, depth, mask = (t.cpu()[0] for t in outs[1:])
    assert torch.equal(seg, torch.from_numpy(D.map_labels(ids).astype(np.int64)))
    d, _ = D.disparity_to_depth(disp, case["bf"], case["depth_max"])
    assert bitwise_equal(depth, torch.from_numpy(d)) and torch.equal(mask, torch.from_numpy((d > 0).astype(np.uint8)))
    # the reference's own recorded depth of every disparity (index = disparity = 256 y + x)
    tag = f"{int(case['bf'])}_{int(case['depth_max'])}"
    g = golden("disparity_all")
    if case["depth_max"] in (80.0, 40.0):
        assert bitwise_equal(depth.reshape(-1), g["depth_" + tag])
        assert torch.equal(mask.reshape(-1), (g["depth_" + tag] > 0).to(U8))
        assert int((g["valid_" + tag] != mask.reshape(-1)).sum()) == 1  # d = 1: 'valid' with depth 0
    else:
        assert float(depth.reshape(-1)[1281]) == case["depth_max"] and int(mask.reshape(-1)[1281]) == 1


# ----------------------------------------------------------------------------- ColorJitter
@pytest.mark.parametrize("case", C.JITTER, ids=lambda c: c["id"])
def test_color_jitter(case):
    img = C.jitter_images(case)
    B, h, w, _ = img.shape
    values = torch.from_numpy(img).reshape(B * h * w, 3).to(DEV)
    buf = guarded_matrix(B * h * w, 3, 3, U8)
    prm = guarded_copy(torch.tensor(case["params"], dtype=torch.float64).to(DEV))
    ws = guarded((B,), torch.int64)  # poisoned on entry: the entry point zeroes it itself
    out, = run_poisoned(lambda: N().call("dclip_color_jitter", buf.ptr(), B, h, w, prm.ptr(), ws.ptr(), _stream()),
                        inputs=[prm], scratch=[ws], inout=[(buf, values)])
    same_rows(case["id"], out.view(B, h, w, 3), expected(case["id"])["img"], case["row_ids"])
    for b, p in enumerate(case["params"]):
        if tuple(p[:4]) == C.IDENT:
            assert torch.equal(out.view(B, h, w, 3)[b].cpu(), torch.from_numpy(img[b])), "the identity touched its bytes"


def test_color_jitter_order_entry_outside_the_table_is_skipped():
    """data.prepare_batch refuses such a table; a direct caller's bad entry must not index outside its row: that
    position is skipped and the other three run"""
    from oracle import data_oracle as D
    img = C._random_images(3, 20, 28, 61)
    rows = [C._row(C.ACTIVE, (0, 7, 2, 3)), C._row(C.ACTIVE, (-3, 1, 2, 3)), C._row(C.ACTIVE, (0, 1, 2, 11))]
    remaining = [(0, 2, 3), (1, 2, 3), (0, 1, 2)]
    values = torch.from_numpy(img).reshape(-1, 3).to(DEV)
    buf = guarded_matrix(values.shape[0], 3, 3, U8)
    prm = guarded_copy(torch.tensor(rows, dtype=torch.float64).to(DEV))
    ws = guarded((3,), torch.int64)
    out, = run_poisoned(lambda: N().call("dclip_color_jitter", buf.ptr(), 3, 20, 28, prm.ptr(), ws.ptr(), _stream()),
                        inputs=[prm], scratch=[ws], inout=[(buf, values)])
    want = np.stack([D.color_jitter(img[b], list(C.ACTIVE) + list(remaining[b])) for b in range(3)])
    same_rows("bad order entries", out.view(3, 20, 28, 3), want, ["entry 7", "entry -3", "entry 11"])


# ----------------------------------------------------------------------------- Normalize
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=_name)
@pytest.mark.parametrize("case", C.NORMALISE, ids=lambda c: c["id"])
def test_normalize_u8(case, dtype):
    img = C.normalise_image()
    B, h, w, _ = img.shape
    src = guarded_copy(torch.from_numpy(img).to(DEV))
    out = guarded((B, 3, h, w), dtype)
    mean, std = _f3(case["norm"][0]), _f3(case["norm"][1])
    got, = run_poisoned(lambda: N().call("dclip_normalize_u8", src.ptr(), B, h, w, mean, std, out.ptr(), _dt(dtype), _stream()),
                        inputs=[src], outputs=[out])
    same_rows(f"{case['id']} {_name(dtype)}", got, image_as(C.normalise_expected(case), dtype), ["image0", "image1"])


# ----------------------------------------------------------------------------- the op layer and prepare_batch
def _op_args(case, jitter=None, dtype=BF16):
    s = C.prep_samples(case)
    img = torch.from_numpy(np.stack([x[0] for x in s])).to(DEV)
    ids = torch.from_numpy(np.stack([x[1] for x in s])).to(DEV)
    disp = torch.from_numpy(np.stack([x[2] for x in s]).view(np.int16)).to(DEV)
    crop = torch.tensor(case["rows"], dtype=torch.int32, device=DEV)
    args = [img, ids, disp, crop, case["h"], case["w"], list(C.CLIP[0]), list(C.CLIP[1]), case["bf"], case["depth_max"], dtype]
    return args + ([jitter] if jitter is not None else [])


def _jitter_rows(B):
    return [C._row(C.ACTIVE, C.ORDERS[(5 * b + 3) % 24]) for b in range(B - 1)] + [C._row(C.IDENT)]


def _op():
    from denseclip_vit_multimodal_amd import ops
    return ops.D().cityscapes_prepare


def test_opcheck_cityscapes_prepare():
    utils = ("test_schema", "test_faketensor", "test_aot_dispatch_dynamic")
    g3, g7 = C.GEOM3[0], C.GEOM7[0]
    jit = torch.tensor(_jitter_rows(len(g7["rows"])), dtype=torch.float64, device=DEV)
    torch.library.opcheck(_op(), tuple(_op_args(g3)), test_utils=utils)
    torch.library.opcheck(_op(), tuple(_op_args(g7)), test_utils=utils)
    torch.library.opcheck(_op(), tuple(_op_args(g7, jit)), test_utils=utils)


def test_prepare_batch_with_jitter_and_fp16_image():
    from oracle import data_oracle as D
    from denseclip_vit_multimodal_amd.data import prepare_batch
    case = C.GEOM7[0]
    samples, rows = list(C.prep_samples(case)), case["rows"]
    jit = _jitter_rows(len(rows))
    img, seg, depth, mask = prepare_batch(samples, (case["h"], case["w"]), rows, DEV, out_dtype=F16, jitter=jit)
    ri, rs, rd, rm = D.prepare_augmented_jitter(samples, (case["h"], case["w"]), rows, jit, *C.CLIP)
    assert img.dtype == F16 and mask.dtype == torch.bool and depth.shape == (len(rows), 1, case["h"], case["w"])
    same_rows("prepare_batch fp16 image", img, image_as(np.ascontiguousarray(ri, np.float32), F16), case["row_ids"])
    same_rows("prepare_batch seg", seg, rs, case["row_ids"])
    same_rows("prepare_batch depth", depth, np.ascontiguousarray(rd, np.float32), case["row_ids"])
    same_rows("prepare_batch mask", mask.view(U8), np.ascontiguousarray(rm).astype(np.uint8), case["row_ids"])
    # the all-identity last row equals the jitter-free path
    plain, *_ = prepare_batch(samples, (case["h"], case["w"]), rows, DEV, out_dtype=F16)
    assert bitwise_equal(img[-1], plain[-1]) and not bitwise_equal(img[0], plain[0])


def test_op_refuses_malformed_arguments():
    """every malformed tensor holds at least as many bytes as the well-formed one: a wider dtype, an extra row, or a
    view of a buffer of the same size"""
    case = C.GEOM3[0]
    good = _op_args(case, dtype=F32)
    img, ids, disp = good[:3]
    B, H, W = ids.shape
    more = lambda t: torch.cat([t, t[:, :1]], 1).contiguous()  # noqa: E731  (B, H + 1, W)
    bad = [("img int16", 0, img.to(torch.int16)), ("img float", 0, img.float()),
           ("ids int64", 1, ids.long()), ("ids int16", 1, ids.to(torch.int16)),
           ("disp int32", 2, disp.int()), ("disp float", 2, disp.float()), ("disp uint8 pairs", 2, disp.view(U8)),
           ("ids (B, H + 1, W)", 1, more(ids)), ("disp (B, H + 1, W)", 2, more(disp)),
           ("ids (B, W, H)", 1, ids.reshape(B, W, H)), ("disp (B, 1, H, W)", 2, disp.reshape(B, 1, H, W)),
           ("ids (B H, W)", 1, ids.reshape(B * H, W)),
           ("ids on the CPU", 1, ids.cpu()), ("disp on the CPU", 2, disp.cpu()), ("img on the CPU", 0, img.cpu()),
           ("crop on the CPU", 3, good[3].cpu()),
           ("img not contiguous", 0, torch.empty(B, W, H, 3, dtype=U8, device=DEV).permute(0, 2, 1, 3)),
           ("ids not contiguous", 1, torch.empty(B, W, H, dtype=U8, device=DEV).permute(0, 2, 1))]
    for what, i, t in bad:
        assert t.numel() * t.element_size() >= good[i].numel() * good[i].element_size(), what
        args = list(good)
        args[i] = t
        with pytest.raises(RuntimeError):
            _op()(*args)
            torch.cuda.synchronize()
            print(f"NOT refused: {what}")
    for h, w in ((0, 4), (4, 0), (-1, 4)):
        args = list(good)
        args[4], args[5] = h, w
        with pytest.raises(RuntimeError):
            _op()(*args)
    # the well-formed call still runs, and is right
    out, seg, depth, mask = _op()(*good)
    e = expected(case["id"])
    same_rows("after the refusals: image", out, e["img"], case["row_ids"])
    same_rows("after the refusals: seg", seg, e["seg"], case["row_ids"])
    same_rows("after the refusals: depth", depth[:, 0], e["depth"], case["row_ids"])
    same_rows("after the refusals: mask", mask[:, 0], e["mask"], case["row_ids"])
