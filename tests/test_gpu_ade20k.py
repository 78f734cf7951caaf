"""dclip_ade20k_prepare / torch.ops.dclip_data.ade20k_prepare / data.prepare_ade20k_batch on the GPU against the
NumPy restatement of the reference pipeline (ade_ref.py, held to PIL and to the reference's recorded outputs by
test_ade20k_cpu.py).  Neither PIL nor the reference is needed here.

Bounds: labels and the uint8 crop (out_dtype uint8: the stage before the normalisation) bit-exact; the f32
image within 1e-6 absolute of the f64 restatement (one f32 rounding of a value below 2.7 is 1.2e-7; the bound is
the CPU test's); a bf16 / f16 image within ulp16(ref) / 2 + 1e-6 (the f64 result is rounded to f32, then to 16
bits).  C-ABI calls run on guard-banded, poisoned buffers (abi_guard.run_poisoned)."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ade_ref as R
from abi_guard import bitwise_equal, guarded, guarded_copy, run_poisoned
from helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(37, 53), (64, 48), (96, 128), (64, 48)]
CROPS = [(32, 32), (40, 36), (33, 30)]  # square; the issue's non-square; a width that is no multiple of 4
IMG_TOL = 1e-6
_name = lambda d: str(d).replace("torch.", "")  # noqa: E731


@pytest.fixture(autouse=True)
def _need(hip):
    pass


def D():
    from denseclip_vit_multimodal_amd import data
    return data


@functools.lru_cache(maxsize=None)
def random_planes():
    g = np.random.RandomState(42)
    out = []
    for H, W in SIZES:
        img = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
        lab = g.randint(0, 151, (H, W)).astype(np.uint8)
        lab[g.rand(H, W) < 0.1] = 0
        lab[0, 0], lab[0, 1], lab[-1, -1], lab[H // 2, W // 2] = 0, 1, 150, 255
        out.append((img, lab))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_case(crop_hw, ignore_label=255):
    """(samples, params, f64 images (B, 3, h, w), labels, uint8 crops (B, 3, h, w)) of the random batch"""
    samples = random_planes()
    prm = D().ade20k_params(SIZES, crop_hw, rng=np.random.RandomState(7 + crop_hw[1]), flip_p=0.5)
    ref = [R.sample(im, lb, p, crop_hw, ignore_label) for (im, lb), p in zip(samples, prm.tolist())]
    return (samples, prm, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]),
            np.stack([r[2].transpose(2, 0, 1) for r in ref]))


def check_image(got, ref64, dtype):
    got = got.double().cpu().numpy()
    err = np.abs(got - ref64)
    bound = IMG_TOL if dtype == torch.float32 else R.ulp16(ref64, dtype) / 2 + IMG_TOL
    print(f"{_name(dtype)}: max abs err {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert bool((err <= bound).all())


# ----------------------------------------------------------------------------- kernel vs restatement
@pytest.mark.parametrize("crop_hw", CROPS, ids=lambda c: f"{c[0]}x{c[1]}")
def test_random_planes_mixed_sizes_in_one_batch(crop_hw):
    samples, prm, ref_img, ref_lab, ref_u8 = random_case(crop_hw)
    assert len({tuple(p[:2]) for p in prm.tolist()}) > 1 and bool((prm[:, 6] == 1).any())
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        img, seg, depth, mask = D().prepare_ade20k_batch(list(samples), crop_hw, prm, DEV, out_dtype=dt)
        assert depth is None and mask is None and img.dtype == dt and img.shape == (4, 3) + crop_hw
        assert seg.dtype == torch.int64 and seg.shape == (4,) + crop_hw
        assert np.array_equal(seg.cpu().numpy(), ref_lab)
        check_image(img, ref_img, dt)
    u8, seg, _, _ = D().prepare_ade20k_batch(list(samples), crop_hw, prm, DEV, out_dtype=torch.uint8)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), ref_u8)
    assert np.array_equal(seg.cpu().numpy(), ref_lab)


def test_fixture_planes_against_restatement_and_reference():
    """the planes the reference's loader saw, batched per crop size: the restatement's bounds, and the recorded
    reference outputs themselves (the restatement is within 1e-6 of them, so 2e-6 here; labels exact on the
    columns the reference's crop_h-wide label holds)"""
    groups = {}
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ade20k", "*.npz"))):
        z = np.load(p)
        groups.setdefault(tuple(int(v) for v in z["crop_hw"]), []).append({k: z[k] for k in z.files})
    assert len(groups) >= 3
    for crop_hw, cases in groups.items():
        samples = [(c["img"], c["lab"]) for c in cases]
        prm = torch.tensor(np.stack([c["params"] for c in cases]))
        ref = [R.sample(c["img"], c["lab"], c["params"], crop_hw) for c in cases]
        img, seg, _, _ = D().prepare_ade20k_batch(samples, crop_hw, prm, DEV, out_dtype=torch.float32)
        u8, _, _, _ = D().prepare_ade20k_batch(samples, crop_hw, prm, DEV, out_dtype=torch.uint8)
        assert np.array_equal(seg.cpu().numpy(), np.stack([r[1] for r in ref]))
        assert np.array_equal(u8.cpu().numpy(), np.stack([r[2].transpose(2, 0, 1) for r in ref]))
        check_image(img, np.stack([r[0] for r in ref]), torch.float32)
        for i, c in enumerate(cases):
            wl = min(crop_hw[1], c["ref_lab"].shape[1])
            assert np.array_equal(seg[i, :, :wl].cpu().numpy(), c["ref_lab"][:, :wl])
            assert float(np.abs(img[i].double().cpu().numpy() - c["ref_img"]).max()) <= 2 * IMG_TOL


# ----------------------------------------------------------------------------- special cases
def test_scale_one_skips_every_pass():
    (img, lab), crop_hw = random_planes()[0], (32, 32)
    H, W = lab.shape
    prm = [(H, W, H, W, 4, 9, 0)]
    u8, seg, _, _ = D().prepare_ade20k_batch([(img, lab)], crop_hw, prm, DEV, out_dtype=torch.uint8)
    assert np.array_equal(u8[0].cpu().numpy(), img[4:36, 9:41].transpose(2, 0, 1))
    assert np.array_equal(seg[0].cpu().numpy(), R.map_labels(lab[4:36, 9:41]))
    # one axis only: the other axis' pass is skipped
    for prm in ([(H, 70, H, 70, 2, 30, 0)], [(50, W, 50, W, 11, 3, 1)]):
        got = D().prepare_ade20k_batch([(img, lab)], crop_hw, prm, DEV, out_dtype=torch.uint8)
        ref = R.sample(img, lab, prm[0], crop_hw)
        assert np.array_equal(got[0][0].cpu().numpy(), ref[2].transpose(2, 0, 1))
        assert np.array_equal(got[1][0].cpu().numpy(), ref[1])


def test_whole_image_without_a_crop():
    img, lab = random_planes()[2]
    out, seg, depth, mask = D().prepare_ade20k_batch([(img, lab)], None, None, DEV, out_dtype=torch.float32)
    assert out.shape == (1, 3, 96, 128) and seg.shape == (1, 96, 128) and depth is None and mask is None
    assert np.array_equal(seg[0].cpu().numpy(), R.map_labels(lab))
    check_image(out[0], R.normalize(img), torch.float32)


def test_flip_is_the_mirror_bitwise():
    samples, prm, _, _, _ = random_case((40, 36))
    a, b = prm.clone(), prm.clone()
    a[:, 6], b[:, 6] = 0, 1
    for dt in (torch.float32, torch.bfloat16, torch.uint8):
        pa = D().prepare_ade20k_batch(list(samples), (40, 36), a, DEV, out_dtype=dt)
        pb = D().prepare_ade20k_batch(list(samples), (40, 36), b, DEV, out_dtype=dt)
        assert bitwise_equal(pb[0], pa[0].flip(-1)) and torch.equal(pb[1], pa[1].flip(-1))
        assert not torch.equal(pb[1], pa[1])


def test_ignore_label_none_keeps_the_labels():
    samples, prm, _, _, _ = random_case((32, 32))
    _, _, _, want, _ = random_case((32, 32), None)
    _, seg, _, _ = D().prepare_ade20k_batch(list(samples), (32, 32), prm, DEV, ignore_label=None)
    assert np.array_equal(seg.cpu().numpy(), want) and int(seg.max()) == 255 and int((seg == 0).sum()) > 0
    _, seg, _, _ = D().prepare_ade20k_batch(list(samples), (32, 32), prm, DEV, ignore_label=200)
    assert np.array_equal(seg.cpu().numpy(), np.where(want > 0, want - 1, 200))


# ----------------------------------------------------------------------------- C ABI: memory safety
def _native():
    from denseclip_vit_multimodal_amd import _native as N
    return N


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class AbiCase:
    """the random batch at `crop_hw` as guarded device buffers for direct C-ABI calls"""

    def __init__(self, crop_hw, out_dtype=torch.float32):
        N = _native()
        self.samples, self.prm, self.ref_img, self.ref_lab, _ = random_case(crop_hw)
        self.h, self.w = crop_hw
        self.geom_host, self.nimg, self.nlab = D().ade20k_geometry(SIZES, self.prm, crop_hw)
        self.img = guarded_copy(torch.from_numpy(np.concatenate([s[0].reshape(-1) for s in self.samples])).to(DEV))
        self.lab = guarded_copy(torch.from_numpy(np.concatenate([s[1].reshape(-1) for s in self.samples])).to(DEV))
        self.geom = guarded_copy(self.geom_host.to(DEV))
        self.need = int(N.lib().dclip_ade20k_prepare_ws_bytes(ctypes.c_void_p(self.geom_host.data_ptr()), 4, self.h, self.w))
        assert self.need > 0
        self.ws = guarded(self.need)
        self.out = guarded((4, 3, self.h, self.w), out_dtype)
        self.seg = guarded((4, self.h, self.w), torch.int64)
        self.dt = {torch.float32: N.F32, torch.float16: N.F16, torch.bfloat16: N.BF16, torch.uint8: N.U8}[out_dtype]
        self.mean = (ctypes.c_double * 3)(*D().IMAGENET_MEAN)
        self.std = (ctypes.c_double * 3)(*D().IMAGENET_STD)

    def args(self, geom_host=None, B=4, ws_bytes=None, img_bytes=None):
        gh = self.geom_host if geom_host is None else geom_host
        self._keep = gh
        return (self.img.ptr(), self.nimg if img_bytes is None else img_bytes, self.lab.ptr(), self.nlab, self.geom.ptr(),
                ctypes.c_void_p(gh.data_ptr()), B, self.h, self.w, self.mean, self.std, 255, self.out.ptr(), self.dt,
                self.seg.ptr(), self.ws.ptr(), self.need if ws_bytes is None else ws_bytes, _stream())


@pytest.mark.parametrize("crop_hw", [(32, 32), (33, 30)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_poisoned_guarded_buffers_and_two_runs_bitwise(crop_hw):
    c = AbiCase(crop_hw)
    out, seg = run_poisoned(lambda: _native().call("dclip_ade20k_prepare", *c.args()), inputs=[c.img, c.lab, c.geom],
                            outputs=[c.out, c.seg], scratch=[c.ws])
    assert np.array_equal(seg.cpu().numpy(), c.ref_lab)
    check_image(out, c.ref_img, torch.float32)
    again = run_poisoned(lambda: _native().call("dclip_ade20k_prepare", *c.args()), inputs=[c.img, c.lab, c.geom],
                         outputs=[c.out, c.seg], scratch=[c.ws])
    assert bitwise_equal(again[0], out) and torch.equal(again[1], seg)


def test_bad_geometry_is_refused_on_the_host_and_nothing_is_launched():
    N = _native()
    c = AbiCase((32, 32))

    def edited(row, col, value):
        g = c.geom_host.clone()
        g[row, col] = value
        return g

    cases = [(dict(geom_host=edited(2, 9, int(c.geom_host[2, 7]) - 31)), "crop window"),     # the window leaves the image
             (dict(geom_host=edited(3, 0, c.nimg - 64 * 48 * 3 + 1)), "image plane"),          # offset past the buffer
             (dict(geom_host=edited(3, 1, c.nlab)), "label plane"),
             (dict(B=0), "bad sizes"),
             (dict(ws_bytes=c.need - 1), "workspace"),                                          # one byte short
             (dict(img_bytes=c.nimg - 1), "image plane")]
    for g in (c.out, c.seg, c.ws):
        g.fill(0x3C)
    for kw, needle in cases:
        with pytest.raises(N.NativeError, match=needle):
            N.call("dclip_ade20k_prepare", *c.args(**kw))
    torch.cuda.synchronize()
    for g in (c.out, c.seg, c.ws):
        assert bool((g.raw[g.off:g.off + g.nbytes] == 0x3C).all()), "a refused call wrote"
        g.check()
    # the op refuses the same table as a RuntimeError
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    bad = edited(2, 9, int(c.geom_host[2, 7]) - 31)
    with pytest.raises(RuntimeError, match="crop window"):
        torch.ops.dclip_data.ade20k_prepare(c.img.t, c.lab.t, bad.to(DEV), bad, 32, 32, list(D().IMAGENET_MEAN),
                                            list(D().IMAGENET_STD), 255, torch.float32)


def test_device_table_that_fails_the_checks_writes_nothing():
    """the host copy passes, the device copy of one image does not (a caller's slip): that image is skipped by every
    kernel, the others are computed, nothing outside the declared extents changes"""
    c = AbiCase((32, 32))
    dev = c.geom_host.clone()
    dev[1, 9] = int(dev[1, 7])  # x0 = W2 on the device only
    c.geom.t.copy_(dev.to(DEV))
    for g in (c.out, c.seg, c.ws):
        g.fill(0x3C)
    _native().call("dclip_ade20k_prepare", *c.args())
    torch.cuda.synchronize()
    for g in (c.img, c.lab, c.geom, c.out, c.seg, c.ws):
        g.check()
    seg = c.seg.t.cpu().numpy()
    assert bool((c.seg.raw[c.seg.off:c.seg.off + c.seg.nbytes].view(4, -1)[1] == 0x3C).all())
    keep = [0, 2, 3]
    assert np.array_equal(seg[keep], c.ref_lab[keep])


# ----------------------------------------------------------------------------- graph capture
def test_graph_capture_replays_on_new_pixels():
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    op = torch.ops.dclip_data.ade20k_prepare
    crop_hw = (40, 36)
    samples, prm, _, _, _ = random_case(crop_hw)
    geom_host, _, _ = D().ade20k_geometry(SIZES, prm, crop_hw)
    pack = lambda k: torch.from_numpy(np.concatenate([s[k].reshape(-1) for s in samples])).to(DEV)  # noqa: E731
    img, lab, geom = pack(0), pack(1), geom_host.to(DEV)
    mean, std = list(D().IMAGENET_MEAN), list(D().IMAGENET_STD)
    call = lambda: op(img, lab, geom, geom_host, 40, 36, mean, std, 255, torch.bfloat16)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, seg = call()
    # new pixels and labels in the captured buffers, same geometry
    img.copy_(img.flip(0))
    lab.copy_(lab.roll(5))
    graph.replay()
    want = call()
    torch.cuda.synchronize()
    assert bitwise_equal(out, want[0]) and torch.equal(seg, want[1])


# ----------------------------------------------------------------------------- end to end
def test_two_train_steps_of_a_seg_only_150_class_model():
    from test_gpu_classes import build_150
    from helpers import TINY_CFG
    from denseclip_vit_multimodal_amd.train import freeze_for_mode, make_optimizer, train_step
    m = build_150(TINY_CFG, "tiny", depth=False)
    assert m.depth_head is None
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    m.fused_head_loss = True
    opt = make_optimizer(freeze_for_mode(m, "F"))
    crop_hw = (64, 64)
    samples = list(random_planes())
    prm = D().ade20k_params(SIZES, crop_hw, rng=np.random.RandomState(3))
    batch = D().prepare_ade20k_batch(samples, crop_hw, prm, DEV, out_dtype=torch.float32)
    assert batch[0].shape == (4, 3, 64, 64) and batch[2] is None and batch[3] is None
    losses = [float(train_step(m, opt, batch)) for _ in range(2)]
    print(f"losses {losses}")
    assert all(np.isfinite(losses)) and losses[1] != losses[0], losses
