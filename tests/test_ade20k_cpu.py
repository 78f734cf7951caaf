"""The ADE20K data path without a GPU: the NumPy restatement of Pillow's 8-bit resize (ade_ref.py) against PIL
itself and against outputs recorded from the reference's own loader (tests/golden/ade20k, written by
tests/golden/gen_ade20k.py), the dataset scan, the parameter draws, the refusals, the op registration and the
host-side geometry checks of dclip_ade20k_prepare (they run before any HIP call).

Image bound against the reference's float64 output: 1e-6 absolute.  The restatement repeats the reference's
own operations (float32 division, float64 subtract / divide), so it is equal up to three f32 roundings of
values below 2.7 after a cancellation at about 0.45 divided by std >= 0.224: about 5e-7."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import ade_ref as R
from helpers import ROOT
from denseclip_vit_multimodal_amd import data as D

GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ade20k", "*.npz")))
# what the recorded cases must exercise between them (gen_ade20k.properties)
COVERAGE = {"downscale", "upscale", "second_both_w", "second_both_h", "second_w", "second_h", "clamp", "x_max_0",
            "right_bottom", "width_not_x4"}
IMG_TOL = 1e-6


def load_case(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def case_properties(c):
    """gen_ade20k.properties, from the recorded parameters alone"""
    H, W = c["lab"].shape
    ch, cw = (int(v) for v in c["crop_hw"])
    H1, W1, H2, W2, y0, x0, _ = (int(v) for v in c["params"])
    got = set()
    if H1 < H and W1 < W:
        # in / out > 1 widens the support: Pillow's ksize = 2 ceil(in / out) + 1 is 5 taps (7 when int() pushed
        # the ratio just past 2)
        assert int(np.ceil(W / W1)) * 2 + 1 in (5, 7) and max(len(k) for _, k in R.bilinear_table(W, W1)) >= 3
        got.add("downscale")
    if H1 > H and W1 > W:
        got.add("upscale")
    second = R.second_resize(W1, H1, cw, ch)
    if second is None:
        assert (H2, W2) == (H1, W1)
    else:
        assert second[:2] == (W2, H2)
        got.add("second_" + second[2])
        if second[3]:
            got.add("clamp")
    if W2 == cw:
        assert x0 == 0
        got.add("x_max_0")
    if W2 > cw and H2 > ch and x0 == W2 - cw and y0 == H2 - ch:
        got.add("right_bottom")
    if cw % 4:
        got.add("width_not_x4")
    return got


# ----------------------------------------------------------------------------- restatement vs PIL
@pytest.mark.parametrize("size", [(1, 7), (37, 53), (64, 64), (96, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_pil(size):
    Image = pytest.importorskip("PIL.Image")
    H, W = size
    g = np.random.RandomState(H * 1000 + W)
    img = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    lab = g.randint(0, 151, (H, W)).astype(np.uint8)
    ran = 0
    for s in (0.31, 0.5, 0.73, 1.0, 1.37, 1.999, 2.0):
        nw, nh = int(W * s), int(H * s)
        if nw < 1 or nh < 1:
            continue  # the reference cannot resize to an empty image either (ade20k_params raises)
        a = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
        b = np.asarray(Image.fromarray(lab).resize((nw, nh), Image.NEAREST))
        ra, rb = R.resize_bilinear(img, nw, nh), R.resize_nearest(lab, nw, nh)
        assert np.array_equal(a, ra) and np.array_equal(b, rb), (size, s)
        # the two-resize chain: the first result resized again, to the size ade20k.py:97-118 gives for a 48 x 40 crop
        second = R.second_resize(nw, nh, 40, 48)
        if second is not None:
            tw, th = second[:2]
            a2 = np.asarray(Image.fromarray(a).resize((tw, th), Image.BILINEAR))
            b2 = np.asarray(Image.fromarray(b).resize((tw, th), Image.NEAREST))
            assert np.array_equal(a2, R.resize_bilinear(ra, tw, th)) and np.array_equal(b2, R.resize_nearest(rb, tw, th))
        ran += 1
    assert ran >= 4  # 1 x 7: the three scales below 1 leave no row


# ----------------------------------------------------------------------------- the reference's recorded outputs
def test_fixture_covers_every_case():
    assert len(GOLDEN) >= 4
    seen, values = set(), set()
    for p in GOLDEN:
        c = load_case(p)
        assert c["img"].shape[0] <= 96 and c["img"].shape[1] <= 128
        seen |= case_properties(c)
        values |= set(np.unique(c["lab"]).tolist())
    assert seen >= COVERAGE, COVERAGE - seen
    assert values >= {0, 1, 150, 255}
    assert sum(os.path.getsize(p) for p in GOLDEN) < 300 * 1024


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_restatement_equals_the_reference_loader(path):
    c = load_case(path)
    crop_hw = tuple(int(v) for v in c["crop_hw"])
    prm = D.ade20k_params([c["lab"].shape], crop_hw, rng=np.random.RandomState(int(c["seed"])))
    assert prm.dtype == torch.int64 and prm.shape == (1, 7)
    assert prm[0].tolist() == c["params"].tolist()
    img, lab, _ = R.sample(c["img"], c["lab"], prm[0].tolist(), crop_hw)
    assert c["ref_img"].dtype == np.float64 and c["ref_img"].shape == (3,) + crop_hw and img.dtype == np.float64
    err = float(np.abs(img - c["ref_img"]).max())
    print(f"image max abs err {err:.3e}")
    assert err <= IMG_TOL
    # the reference's label crop is crop_h wide (ade20k.py:136): the columns both hold
    wl = min(crop_hw[1], c["ref_lab"].shape[1])
    assert c["ref_lab"].dtype == np.int64 and c["ref_lab"].shape == (crop_hw[0], crop_hw[0]) and lab.dtype == np.int64
    assert np.array_equal(lab[:, :wl], c["ref_lab"][:, :wl])
    assert lab.min() >= 0 and lab.max() <= 255


def test_label_map():
    lab = np.array([[0, 1, 150, 255]], dtype=np.uint8)
    assert R.map_labels(lab).tolist() == [[255, 0, 149, 254]]
    assert R.map_labels(lab, None).tolist() == [[0, 1, 150, 255]]


# ----------------------------------------------------------------------------- dataset and refusals
def make_tree(root, names, with_info=True, split="training"):
    Image = pytest.importorskip("PIL.Image")
    base = root / "ADEChallengeData2016"
    g = np.random.RandomState(3)
    for n in names:
        for sub, ext, arr in (("images", ".jpg", g.randint(0, 256, (12, 17, 3)).astype(np.uint8)),
                              ("annotations", ".png", g.randint(0, 151, (12, 17)).astype(np.uint8))):
            d = base / sub / split
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(arr).save(str(d / (n + ext)))
    if with_info:
        (base / "objectInfo150.txt").write_text(
            "Idx\tRatio\tTrain\tVal\tName\n1\t0.1576\t11664\t1172\twall\n2\t0.1072\t6046\t612\tbuilding, edifice\n"
            "3\t0.0878\t8265\t796\tsky\n4\t0.0621\t9336\t917\tfloor, flooring\n")
    return str(root)


def test_dataset_scan(tmp_path):
    root = make_tree(tmp_path, ["ADE_train_00000010", "ADE_train_00000002", "ADE_train_00000007"])
    (tmp_path / "ADEChallengeData2016" / "images" / "training" / "notes.txt").write_text("x")
    ds = D.ADE20KSegmentation(root, split="training", crop_size=(40, 36))
    assert len(ds) == 3 and ds.crop_hw == (40, 36) and ds.scale == (0.5, 2.0) and ds.ignore_label == 255
    assert ds.filenames == ["ADE_train_00000002", "ADE_train_00000007", "ADE_train_00000010"]
    img, lab = ds[1]
    assert img.dtype == np.uint8 and img.shape == (12, 17, 3) and lab.dtype == np.uint8 and lab.shape == (12, 17)
    assert D.ADE20KSegmentation(root, crop_size=512).crop_hw == (512, 512)
    assert ds.class_names == ("wall", "building", "sky", "floor")
    os.remove(os.path.join(ds.label_dir, "ADE_train_00000007.png"))
    with pytest.raises(FileNotFoundError, match="ADE_train_00000007"):
        ds[1]
    with pytest.raises(RuntimeError, match="dir not found"):
        D.ADE20KSegmentation(root, split="validation")
    with pytest.raises(RuntimeError, match="dir not found"):
        D.ADE20KSegmentation(str(tmp_path / "nowhere"))


def test_dataset_validation_split_and_missing_class_file(tmp_path):
    root = make_tree(tmp_path, ["ADE_val_00000001"], with_info=False, split="validation")
    ds = D.ADE20KSegmentation(root, split="validation")
    assert ds.image_dir.endswith(os.path.join("images", "validation")) and len(ds) == 1
    with pytest.raises(FileNotFoundError, match="objectInfo150"):
        ds.class_names


def test_params_follow_the_reference_draws():
    """one uniform, then randint for x, then randint for y, per sample, from one stream"""
    sizes, crop = [(37, 53), (96, 128), (64, 48)], (40, 36)
    got = D.ade20k_params(sizes, crop, rng=np.random.RandomState(11))
    r = np.random.RandomState(11)
    for (H, W), row in zip(sizes, got.tolist()):
        s = r.uniform(0.5, 2.0)
        w, h = int(W * s), int(H * s)
        second = R.second_resize(w, h, crop[1], crop[0])
        W2, H2 = second[:2] if second else (w, h)
        x = r.randint(0, max(0, W2 - crop[1]) + 1)
        y = r.randint(0, max(0, H2 - crop[0]) + 1)
        assert row == [h, w, H2, W2, y, x, 0]
    flips = D.ade20k_params([(64, 64)] * 64, (32, 32), rng=np.random.RandomState(1), flip_p=0.5)[:, 6]
    assert 10 < int(flips.sum()) < 54
    # the flip is drawn last: the other six columns of the first sample are those of the unflipped stream
    a = D.ade20k_params([(64, 64)], (32, 32), rng=np.random.RandomState(1), flip_p=0.5)
    b = D.ade20k_params([(64, 64)], (32, 32), rng=np.random.RandomState(1))
    assert a[0, :6].tolist() == b[0, :6].tolist()


def test_params_and_batch_refusals():
    with pytest.raises(ValueError, match="below 1"):
        D.ade20k_params([(1, 7)], (4, 4), scale=(0.5, 0.9), rng=np.random.RandomState(0))
    with pytest.raises(ValueError, match="at least 1x1"):
        D.ade20k_params([(0, 7)], (4, 4))
    with pytest.raises(ValueError, match="at least 1x1"):
        D.ade20k_params([(8, 8)], (0, 4))
    img, lab = np.zeros((8, 9, 3), np.uint8), np.zeros((8, 9), np.uint8)
    prm = D.ade20k_params([(8, 9)], (4, 4), rng=np.random.RandomState(0))
    with pytest.raises(RuntimeError, match="GPU"):
        D.prepare_ade20k_batch([(img, lab)], (4, 4), prm, "cpu")
    with pytest.raises(ValueError, match="empty"):
        D.prepare_ade20k_batch([], (4, 4), prm, "cuda")
    with pytest.raises(ValueError, match="one sample"):
        D.prepare_ade20k_batch([(img, lab), (img, lab)], None, None, "cuda")
    with pytest.raises(ValueError, match="uint8"):
        D.prepare_ade20k_batch([(img.astype(np.float32), lab)], (4, 4), prm, "cuda")
    bad = prm.clone()
    bad[0, 5] = bad[0, 3]  # x0 = W2: the window leaves the image
    with pytest.raises(ValueError, match="bad resize / crop"):
        D.prepare_ade20k_batch([(img, lab)], (4, 4), bad, "cuda")


# ----------------------------------------------------------------------------- ops and ABI
@pytest.fixture(scope="module")
def ops():
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    return torch.ops.dclip_data


def test_ops_are_registered_beside_the_pinned_set(ops):
    from test_torch_ops_cpu import OPS
    names = set(torch._C._dispatch_get_all_op_names())
    assert {n for n in names if n.startswith("dclip_data::")} == {"dclip_data::ade20k_prepare", "dclip_data::ade20k_ws_bytes"}
    assert {n for n in names if n.startswith("dclip::")} == {"dclip::" + o for o in OPS}
    schema = str(ops.ade20k_prepare.default._schema)
    assert "Tensor geom_host" in schema and "ScalarType out_dtype" in schema and "int ignore_label" in schema


def test_fake_shapes_and_cpu_refusal(ops):
    from torch._subclasses.fake_tensor import FakeTensorMode
    geom, nimg, nlab = D.ade20k_geometry([(37, 53), (64, 48)], [(48, 70, 48, 70, 3, 0, 0), (39, 29, 43, 32, 9, 0, 1)], (32, 32))
    assert geom.shape == (2, D.ADE_GEOM_WORDS) and nimg == 3 * nlab == 3 * (37 * 53 + 64 * 48)
    assert geom[1, :2].tolist() == [37 * 53 * 3, 37 * 53]
    with FakeTensorMode(allow_non_fake_inputs=True):  # geom_host stays a real CPU tensor: the host reads it
        img = torch.empty(nimg, dtype=torch.uint8, device="cuda")
        lab = torch.empty(nlab, dtype=torch.uint8, device="cuda")
        g = torch.empty(2, D.ADE_GEOM_WORDS, dtype=torch.int64, device="cuda")
        for dt in (torch.float32, torch.bfloat16, torch.float16, torch.uint8):
            o, s = ops.ade20k_prepare(img, lab, g, geom, 32, 32, list(D.IMAGENET_MEAN), list(D.IMAGENET_STD), 255, dt)
            assert o.shape == (2, 3, 32, 32) and o.dtype == dt and s.shape == (2, 32, 32) and s.dtype == torch.int64
    with pytest.raises(NotImplementedError, match="CPU"):
        ops.ade20k_prepare(torch.zeros(nimg, dtype=torch.uint8), torch.zeros(nlab, dtype=torch.uint8), geom, geom, 32, 32,
                           list(D.IMAGENET_MEAN), list(D.IMAGENET_STD), 255, torch.float32)
    assert ops.ade20k_ws_bytes(geom, 32, 32) > 0


def test_header_binding_and_library_agree():
    import re
    from denseclip_vit_multimodal_amd import _native as N
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", src, re.M))
    lib = N.load()
    for name in ("dclip_ade20k_prepare", "dclip_ade20k_prepare_ws_bytes"):
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert int(re.search(r"#define DCLIP_ADE_GEOM_WORDS (\d+)", src).group(1)) == N.ADE_GEOM_WORDS == D.ADE_GEOM_WORDS
    assert int(re.search(r"#define DCLIP_U8 (\d+)", src).group(1)) == N.U8


def geom_ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def test_workspace_query_and_host_checks_without_a_gpu():
    """the geometry checks run on the host copy before any HIP call: bad rows are refused here, with null
    device pointers never reached"""
    from denseclip_vit_multimodal_amd import _native as N
    lib = N.load()
    sizes, prm = [(37, 53), (64, 48)], [(48, 70, 48, 70, 3, 0, 0), (39, 29, 43, 32, 9, 0, 1)]
    geom, nimg, nlab = D.ade20k_geometry(sizes, prm, (32, 32))
    need = lib.dclip_ade20k_prepare_ws_bytes(geom_ptr(geom), 2, 32, 32)
    one = [lib.dclip_ade20k_prepare_ws_bytes(geom_ptr(geom[i:i + 1].contiguous()), 1, 32, 32) for i in (0, 1)]
    assert need == 2 * max(one) and min(one) > 0 and need % 16 == 0
    # every pass skipped: the two nearest tables alone
    ident, _, _ = D.ade20k_geometry([(20, 24)], [(20, 24, 20, 24, 2, 3, 0)], (16, 16))
    assert lib.dclip_ade20k_prepare_ws_bytes(geom_ptr(ident), 1, 16, 16) == 2 * 16 * 4
    mean = (ctypes.c_double * 3)(*D.IMAGENET_MEAN)
    std = (ctypes.c_double * 3)(*D.IMAGENET_STD)
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below fails in the host checks

    def call(g, B=2, img_bytes=nimg, lab_bytes=nlab, ws_bytes=need, h=32, w=32):
        rc = lib.dclip_ade20k_prepare(fake, img_bytes, fake, lab_bytes, fake, geom_ptr(g), B, h, w, mean, std, 255, fake,
                                      N.F32, fake, fake, ws_bytes, None)
        return rc, lib.dclip_last_error().decode()

    def edited(row, col, value):
        g = geom.clone()
        g[row, col] = value
        return g

    for g, needle in ((edited(1, 9, 1), "crop window"), (edited(0, 8, 48 - 31), "crop window"), (edited(0, 8, -1), "crop window"),
                      (edited(1, 0, nimg - 64 * 48 * 3 + 1), "image plane"), (edited(1, 1, nlab), "label plane"),
                      (edited(0, 0, -1), "image plane"), (edited(0, 4, 0), "below 1"), (edited(1, 3, 1 << 20), "below 1"),
                      (edited(0, 7, 31), "crop window"), (edited(1, 2, 1 << 15), "above 16384")):
        rc, msg = call(g)
        assert rc == -1 and needle in msg, (needle, msg)
        assert lib.dclip_ade20k_prepare_ws_bytes(geom_ptr(g), 2, 32, 32) == -1 or "plane" in needle
    assert call(geom, ws_bytes=need - 1) == (-1, call(geom, ws_bytes=need - 1)[1]) and "workspace" in call(geom, ws_bytes=need - 1)[1]
    assert call(geom, B=0)[0] == -1 and "bad sizes" in call(geom, B=0)[1]
    assert call(geom, img_bytes=nimg - 1)[0] == -1 and "image plane" in call(geom, img_bytes=nimg - 1)[1]
    assert call(geom, lab_bytes=nlab - 1)[0] == -1 and "label plane" in call(geom, lab_bytes=nlab - 1)[1]
    assert call(geom, h=33)[0] == -1
    assert lib.dclip_ade20k_prepare_ws_bytes(geom_ptr(geom), 0, 32, 32) == -1
