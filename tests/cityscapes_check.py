"""The cases and expected outputs of test_gpu_cityscapes_contract.py (the four entry points of
csrc/data.hip: dclip_cityscapes_prepare, dclip_cityscapes_augment, dclip_color_jitter and
dclip_normalize_u8), on the CPU and with no GPU import, so that the case set goes through
test_cityscapes_contract_emulation_cpu.py before any kernel meets it.

The reference of everything here is oracle/data_oracle.py, compared bit for bit: the pipeline is
integer work plus correctly rounded f32 steps in the reference's order.  A 16-bit image is the
oracle's f32 result cast with torch.Tensor.to(dtype); a uint8 image (the augment kernel's HWC crop
before ColorJitter / Normalize) is the oracle's crop under the identity normalisation.

Every function that builds an expectation takes the oracle module as `oracle`, so that the CPU test
can pass a copy with a planted defect (PLANTED, planted_oracle) and see which cases notice.

Tables (every entry has an "id"):
  GEOM7      rows (Hs, Ws, pad_top, pad_left, y0, x0, flip) of dclip_cityscapes_augment, one batch
  GEOM3      batches of 3 windows (y0, x0, flip) of dclip_cityscapes_prepare
  DOMAINS    the 256 x 256 plane of every label id and every uint16 disparity, per (bf, depth_max)
  JITTER     batches of uint8 images with their (B, 8) ColorJitter tables
  NORMALISE  mean / std pairs for dclip_normalize_u8
"""
import functools
import inspect
import itertools
import types

import numpy as np

from oracle import data_oracle as D

CLIP = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
IDENTITY_NORM = ((0.0, 0.0, 0.0), (1 / 255.0,) * 3)  # (x - 0) * (1 / (255 / 255)) = x
SRC_HW = (37, 53)   # odd sizes, no multiple of anything
CROP_HW = (24, 28)  # h * w = 672: no multiple of 256


# ----------------------------------------------------------------------------- sources
@functools.lru_cache(maxsize=None)
def random_samples(B, H, W, seed):
    """B decoded samples (img uint8 HxWx3, ids uint8 HxW, disp uint16 HxW): label ids over the whole
    byte range with the table's own range favoured, disparities around the depth_max boundary and
    over the whole uint16 range, zeros (invalid) among them"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ids = np.where(rng.random((H, W)) < 0.7, rng.integers(0, 36, (H, W)), rng.integers(0, 256, (H, W)))
        disp = np.where(rng.random((H, W)) < 0.6, rng.integers(0, 3000, (H, W)), rng.integers(0, 65536, (H, W)))
        disp[rng.random((H, W)) < 0.05] = 0
        out.append((img, ids.astype(np.uint8), disp.astype(np.uint16)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def domain_sample():
    """256 x 256: ids[y, x] = x (every byte in every row), disp[y, x] = 256 y + x (every uint16 once)"""
    yy, xx = np.mgrid[0:256, 0:256]
    img = np.random.default_rng(11).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    return ((img, xx.astype(np.uint8), (256 * yy + xx).astype(np.uint16)),)


# ----------------------------------------------------------------------------- geometry tables
def _geom7():
    (H, W), (h, w) = SRC_HW, CROP_HW
    rows = [
        ("scale0.5_padded_both", D.scale_pad_params(H, W, h, w, 0.5, 0.3, 0.6, 0)),
        ("scale2.0_origin", (2 * H, 2 * W, 0, 0, 0, 0, 0)),
        ("scale2.0_far_corner_flipped", (2 * H, 2 * W, 0, 0, 2 * H - h, 2 * W - w, 1)),
        ("identity_far_corner_flipped", (H, W, 0, 0, H - h, W - w, 1)),
        ("rows_padded_columns_not", (18, 60, 3, 0, 0, 32, 0)),
        ("columns_padded_rows_not_flipped", (60, 20, 0, 4, 36, 0, 1)),
        ("one_row_scaled_image", (1, 53, 11, 0, 0, 5, 0)),
        ("one_pixel_scaled_image", (1, 1, 11, 13, 0, 0, 0)),
        ("scale2.0_top_right_flipped", (2 * H, 2 * W, 0, 0, 0, 2 * W - w, 1)),
        ("scale2.0_bottom_left", (2 * H, 2 * W, 0, 0, 2 * H - h, 0, 0)),
        # 37 -> 63 rows and 53 -> 82 columns: at scaled row 2 and scaled column 12 a cubic coefficient
        # times 2048 is a half in f32 (even integer part), where half-even and half-up rounding part.
        # Dyadic fractions never tie: the coefficients at k / 128 times 2048 are all off a half
        ("coefficient_ties", (63, 82, 0, 0, 0, 0, 0)),
    ]
    return dict(id="geom7", kind="augment", H=H, W=W, h=h, w=w, seed=21, bf=500.0, depth_max=80.0,
                rows=[r for _, r in rows], row_ids=[n for n, _ in rows])


def _geom3():
    (H, W), (h, w) = SRC_HW, CROP_HW
    corners = [("top_left", 0, 0), ("top_right", 0, W - w), ("bottom_left", H - h, 0), ("bottom_right", H - h, W - w)]
    win = [(f"{n}{'_flipped' if f else ''}", (y, x, f)) for n, y, x in corners for f in (0, 1)]
    win.append(win[0])  # 8 windows in batches of 3
    out = []
    for i in range(3):
        part = win[3 * i:3 * i + 3]
        out.append(dict(id=f"geom3_corners{i}", kind="prepare", H=H, W=W, h=h, w=w, seed=31 + i, bf=500.0,
                        depth_max=80.0, rows=[r for _, r in part], row_ids=[n for n, _ in part]))
    out.append(dict(id="geom3_full_window", kind="prepare", H=H, W=W, h=H, w=W, seed=34, bf=500.0, depth_max=80.0,
                    rows=[(0, 0, 0), (0, 0, 1), (0, 0, 1)], row_ids=["full", "full_flipped", "full_flipped_again"]))
    return out


def depth_of(d, bf):
    """the f32 depth the reference gives disparity d (for a depth_max that equals a depth exactly)"""
    return float(np.float32(bf) / ((np.float32(d) - np.float32(1)) / np.float32(256) + np.float32(1e-6)))


def _domains():
    out = []
    # depth_max = the depth of disparity 1281 itself: `depth <= depth_max` holds with equality there.  At
    # (500, 80) and (250, 40) no disparity gives a depth equal to depth_max (d = 1601 gives 79.99999)
    settings = [("default", 500.0, 80.0), ("bf250_max40", 250.0, 40.0), ("max_is_a_depth", 500.0, depth_of(1281, 500.0))]
    for name, bf, dmax in settings:
        out.append(dict(id=f"domain_prepare_{name}", kind="prepare", H=256, W=256, h=256, w=256, source="domain",
                        bf=bf, depth_max=dmax, rows=[(0, 0, 0)], row_ids=["full"]))
        out.append(dict(id=f"domain_augment_{name}", kind="augment", H=256, W=256, h=256, w=256, source="domain",
                        bf=bf, depth_max=dmax, rows=[(256, 256, 0, 0, 0, 0, 0)], row_ids=["identity"]))
    return out


GEOM7 = [_geom7()]
GEOM3 = _geom3()
DOMAINS = _domains()
PREP_CASES = GEOM7 + GEOM3 + DOMAINS


def prep_samples(case):
    if case.get("source") == "domain":
        return domain_sample()
    return random_samples(len(case["rows"]), case["H"], case["W"], case["seed"])


def prep_expected(case, oracle=D, norm=CLIP):
    """(img f32 (B, 3, h, w), seg int64 (B, h, w), depth f32 (B, h, w), mask uint8 (B, h, w)) of the case"""
    fn = oracle.prepare_augmented if case["kind"] == "augment" else oracle.prepare
    img, seg, depth, mask = fn(list(prep_samples(case)), (case["h"], case["w"]), case["rows"], norm[0], norm[1],
                               case["bf"], case["depth_max"])
    B, h, w = len(case["rows"]), case["h"], case["w"]
    return (np.ascontiguousarray(img, np.float32), np.ascontiguousarray(seg, np.int64),
            np.ascontiguousarray(depth, np.float32).reshape(B, h, w),
            np.ascontiguousarray(mask).astype(np.uint8).reshape(B, h, w))


def prep_expected_u8(case, oracle=D):
    """the uint8 HWC crop (B, h, w, 3) of an augment case: DCLIP_U8, before ColorJitter / Normalize"""
    img, seg, depth, mask = prep_expected(case, oracle, IDENTITY_NORM)
    u8 = np.rint(img).astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), img)
    return np.ascontiguousarray(u8.transpose(0, 2, 3, 1)), seg, depth, mask


def padded(case):
    """bool (B, h, w): the output pixels of an augment case that PadIfNeeded fills"""
    h, w = case["h"], case["w"]
    out = np.zeros((len(case["rows"]), h, w), bool)
    for b, (Hs, Ws, pt, pl, y0, x0, flip) in enumerate(case["rows"]):
        ys = y0 + np.arange(h)[:, None] - pt
        xs = (x0 + w - 1 - np.arange(w) if flip else x0 + np.arange(w))[None, :] - pl
        out[b] = (ys < 0) | (ys >= Hs) | (xs < 0) | (xs >= Ws)
    return out


# ----------------------------------------------------------------------------- the colour lattice
@functools.lru_cache(maxsize=None)
def lattice():
    """uint8 (h, 1024, 3): every pair (max, min) of channel values, min <= max, in each of the six
    channel orders, the middle channel at min, min + 1, max - 1, max and the values nearest
    min + k (max - min) / 7, k = 1..6 (duplicates dropped): every index pair of the 8-bit HSV
    path's division tables (by max and by max - min) with the hue swept across each sector.  The
    last row is filled up with the last pixel.  Returns (image, number of lattice pixels)."""
    mx, mn = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    keep = mn <= mx
    mx, mn = mx[keep], mn[keep]                                  # 32896 pairs
    d = mx - mn
    mids = [mn, np.minimum(mn + 1, mx), np.maximum(mx - 1, mn), mx]
    mids += [mn + (2 * k * d + 7) // 14 for k in range(1, 7)]   # nearest to min + k d / 7
    mid = np.stack(mids, 1)                                      # (pairs, 10)
    trip = np.stack([np.broadcast_to(mx[:, None], mid.shape), mid, np.broadcast_to(mn[:, None], mid.shape)], -1)
    trip = trip.reshape(-1, 3)                                   # (max, mid, min)
    px = np.concatenate([trip[:, list(p)] for p in itertools.permutations(range(3))])
    code = np.unique(px[:, 0] << 16 | px[:, 1] << 8 | px[:, 2])  # duplicates dropped
    px = np.stack([code >> 16, code >> 8 & 255, code & 255], 1).astype(np.uint8)
    n = len(px)
    rows = -(-n // 1024)
    px = np.concatenate([px, np.repeat(px[-1:], rows * 1024 - n, 0)])
    return px.reshape(rows, 1024, 3), n


# ----------------------------------------------------------------------------- ColorJitter tables
ORDERS = list(itertools.permutations(range(4)))  # all 24
ACTIVE = (1.3, 0.7, 1.35, -0.07)
IDENT = (1.0, 1.0, 1.0, 0.0)
HAND_PICKED = [[255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 128, 128], [0, 0, 0], [255, 255, 255], [255, 255, 0],
               [1, 2, 3]]


def _row(fac, order=(0, 1, 2, 3)):
    return [float(f) for f in fac] + [float(o) for o in order]


def _alone(op, f):
    fac = list(IDENT)
    fac[op] = f
    return _row(fac)


def _random_images(B, h, w, seed):
    img = np.random.default_rng(seed).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    if h * w >= 8:
        img.reshape(B, -1, 3)[:, :8] = HAND_PICKED
    return img


def _grey_mean_images(h, w, seed):
    """two grey images (gray_u8(v, v, v) = v) of pairs 100 -+ k: gray mean exactly 100, and of pairs
    (100 - k, 101 + k): gray mean exactly 100.5"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 100, h * w // 2)
    a = rng.permutation(np.concatenate([100 - k, 100 + k]))
    b = rng.permutation(np.concatenate([100 - k, 101 + k]))
    img = np.stack([a, b]).astype(np.uint8).reshape(2, h, w, 1)
    return np.ascontiguousarray(np.broadcast_to(img, (2, h, w, 3)))


def _jitter_cases():
    cases = []
    # each operation alone, one image per factor; the last row is the all-identity table
    alone = [("brightness", 0, f) for f in (0.6, 0.75, 1.25, 1.4)] + [("contrast", 1, f) for f in (0.6, 0.75, 1.25, 1.4)]
    alone += [("saturation", 2, f) for f in (0.0, 0.6, 1.4)]
    alone += [("hue", 3, f) for f in (0.1, -0.1, 0.5, -0.5, 1 / 180, 1 / 360, -1 / 360)]
    cases.append(dict(id="jitter_each_alone", images=lambda: _random_images(len(alone) + 1, 20, 28, 41),
                      params=[_alone(op, f) for _, op, f in alone] + [_row(IDENT)],
                      row_ids=[f"{n}_{f:+.4f}" for n, _, f in alone] + ["all_identity"]))
    # contrast on gray means of exactly 100 and exactly 100.5: i f + m (1 - f) lands on integers
    cf = (0.0, 0.6, 0.75, 1.25, 1.4, 2.0)
    cases.append(dict(id="jitter_contrast_exact_means",
                      images=lambda: np.concatenate([_grey_mean_images(20, 28, 42)] * len(cf)),
                      params=[_alone(1, f) for f in cf for _ in range(2)],
                      row_ids=[f"contrast_{f}_mean{m}" for f in cf for m in ("100", "100.5")]))
    # all 24 orders: active factors, then an identity brightness / hue inside the active order
    for name, fac in (("active", ACTIVE), ("brightness_identity", (1.0,) + ACTIVE[1:]), ("hue_identity", ACTIVE[:3] + (0.0,))):
        cases.append(dict(id=f"jitter_orders_{name}", images=lambda: _random_images(24, 20, 28, 43),
                          params=[_row(fac, o) for o in ORDERS], row_ids=["order" + "".join(map(str, o)) for o in ORDERS]))
    # sizes: h * w = 1, 255, 257 (one block, its last thread idle / a second block of one pixel)
    for h, w in ((1, 1), (15, 17), (1, 257)):
        cases.append(dict(id=f"jitter_size_{h}x{w}", images=functools.partial(_random_images, 2, h, w, 44 + h),
                          params=[_row(ACTIVE, (1, 3, 0, 2)), _row(ACTIVE, (2, 1, 3, 0))], row_ids=["a", "b"]))

    # 520 x 520 = 270400 > 1024 blocks x 256: the gray-mean reduction's grid-stride loop runs
    def big():
        rng = np.random.default_rng(47)
        return np.stack([rng.integers(0, 120, (520, 520, 3)), rng.integers(100, 256, (520, 520, 3))]).astype(np.uint8)

    cases.append(dict(id="jitter_520x520_grid_stride", images=big,
                      params=[_alone(1, 0.6), _row((1.0, 1.4, 1.0, 0.0), (3, 1, 0, 2))], row_ids=["dark_0.6", "bright_1.4"]))
    # the max / min lattice: hue first in the four-operation row, so the tables see the lattice itself
    cases.append(dict(id="jitter_lattice", images=lambda: np.stack([lattice()[0]] * 3),
                      params=[_row(ACTIVE, (3, 2, 1, 0)), _alone(3, 1 / 180), _alone(2, 0.6)],
                      row_ids=["four_ops_hue_first", "hue_1/180", "saturation_0.6"]))
    return cases


JITTER = _jitter_cases()


def jitter_images(case):
    """uint8 (B, h, w, 3)"""
    img = np.ascontiguousarray(case["images"]())
    assert img.dtype == np.uint8 and img.shape[0] == len(case["params"]) and img.shape[3] == 3
    return img


def jitter_expected(case, oracle=D, images=None):
    img = jitter_images(case) if images is None else images
    return np.stack([oracle.color_jitter(img[b], case["params"][b]) for b in range(len(img))])


# ----------------------------------------------------------------------------- Normalize
NORMALISE = [dict(id="normalise_clip", norm=CLIP), dict(id="normalise_imagenet", norm=IMAGENET)]


@functools.lru_cache(maxsize=None)
def normalise_image():
    """uint8 (2, 9, 57, 3) (513 pixels per image): every byte value in every channel, then random"""
    img = np.random.default_rng(51).integers(0, 256, (2, 9 * 57, 3), dtype=np.uint8)
    i = np.arange(256)
    img[0, :256] = np.stack([i, 255 - i, (7 * i + 3) % 256], 1)
    return img.reshape(2, 9, 57, 3)


def normalise_expected(case, oracle=D):
    """f32 (B, 3, h, w)"""
    img = normalise_image()
    return np.ascontiguousarray(oracle.normalize(img, *case["norm"]).transpose(0, 3, 1, 2), np.float32)


ALL_CASES = PREP_CASES + JITTER + NORMALISE


# ----------------------------------------------------------------------------- planted defects
# name -> (families that could notice, [(text of oracle/data_oracle.py, its replacement), ...]).  Each
# old text must occur exactly once in the oracle's source (planted_oracle asserts it).
_FLIP_AUG = """        if flip:
            im, lab, dep = im[:, ::-1], lab[:, ::-1], dep[:, ::-1]
"""
_FLIP_AUG_OFF = """        if flip:
            win = (slice(y0, y0 + h), slice(x0 + 1, x0 + w + 1))
            im, lab, dep = pim[win][:, ::-1], plab[win][:, ::-1], pdep[win][:, ::-1]
"""
_FLIP_PREP = "            im, lab, dp = im[:, ::-1], lab[:, ::-1], dp[:, ::-1]\n"
_FLIP_PREP_OFF = """            cols = np.minimum(np.arange(x0 + w, x0, -1), img.shape[1] - 1)
            im, lab, dp = img[y0:y0 + h][:, cols], ids[y0:y0 + h][:, cols], disp[y0:y0 + h][:, cols]
"""
_CANVAS = "Hp, Wp = max(Hs + pt, y0 + h), max(Ws + pl, x0 + w)"
_PLACE = "        pim[pt:pt + Hs, pl:pl + Ws], plab[pt:pt + Hs, pl:pl + Ws], pdep[pt:pt + Hs, pl:pl + Ws] = im, lab, dep\n"
_PLACE_FAR = """        im, lab, dep = (np.pad(a, ((0, 1), (0, 1)) + ((0, 0),) * (a.ndim - 2), mode="edge") for a in (im, lab, dep))
        pim[pt:pt + Hs + 1, pl:pl + Ws + 1], plab[pt:pt + Hs + 1, pl:pl + Ws + 1] = im, lab
        pdep[pt:pt + Hs + 1, pl:pl + Ws + 1] = dep
"""
_NN_W = "np.minimum(np.floor(np.arange(Ws) * (1.0 / (float(Ws) / W))).astype(np.int64), W - 1)"
_NN_H = "np.minimum(np.floor(np.arange(Hs) * (1.0 / (float(Hs) / H))).astype(np.int64), H - 1)"
_MEAN = "lut = lut + _gray_u8(img).mean() * (1 - f)"

PLANTED = {
    "mirror_off_by_one": (("geom7", "geom3"), [
        (_CANVAS, "Hp, Wp = max(Hs + pt, y0 + h), max(Ws + pl, x0 + w) + 1"), (_FLIP_AUG, _FLIP_AUG_OFF),
        (_FLIP_PREP, _FLIP_PREP_OFF)]),
    "cubic_window_clamped_at_W-2": (("geom7",), [
        ("cols = np.clip(sx[:, None] - 1 + np.arange(4), 0, W - 1)", "cols = np.clip(sx[:, None] - 1 + np.arange(4), 0, W - 2)")]),
    "coefficients_rounded_half_up": (("geom7",), [
        ("np.clip(np.rint(c), -32768, 32767)", "np.clip(np.floor(c + np.float32(0.5)), -32768, 32767)")]),
    "vertical_pass_without_2^21": (("geom7",), [("(v + (1 << 21)) >> 22", "v >> 22")]),
    "pad_test_gt_at_the_far_edge": (("geom7",), [
        (_CANVAS, "Hp, Wp = max(Hs + pt, y0 + h) + 1, max(Ws + pl, x0 + w) + 1"), (_PLACE, _PLACE_FAR)]),
    "padded_mask_0": (("geom7",), [("masks.append((dep > 0)[None])", "masks.append(((dep > 0) & (dep != 255.0))[None])")]),
    "depth_lt_depth_max": (("domain",), [("valid = valid0 & (depth <= np.float32(depth_max))",
                                         "valid = valid0 & (depth < np.float32(depth_max))")]),
    "ids_le_34": (("domain", "geom7", "geom3"), [
        ("ok = ids < len(ID_TO_TRAIN_ID)", "ok = ids <= len(ID_TO_TRAIN_ID)"),
        ("out[ok] = ID_TO_TRAIN_ID[ids[ok]]", "out[ok] = np.append(ID_TO_TRAIN_ID, np.uint8(0))[ids[ok]]")]),
    "gray_R_and_B_weights_swapped": (("jitter",), [
        ("x[..., 0] * 4899 + x[..., 1] * 9617 + x[..., 2] * 1868", "x[..., 0] * 1868 + x[..., 1] * 9617 + x[..., 2] * 4899")]),
    "saturation_truncated": (("jitter",), [
        ("img = np.clip(np.rint(t), 0, 255).astype(np.uint8)", "img = np.clip(np.trunc(t), 0, 255).astype(np.uint8)")]),
    "hue_lut_without_negative_wrap": (("jitter",), [
        ("lut = np.mod(np.arange(0, 256, dtype=np.int16) + 180 * f, 180).astype(np.uint8)",
         "lut = (np.fmod(np.arange(0, 256, dtype=np.int16) + 180 * f, 180).astype(np.int64) & 255).astype(np.uint8)")]),
    "hdiv_truncated": (("jitter",), [
        ("hdiv = np.where(i > 0, np.rint((180 << 12) / (6.0 * i)), 0)", "hdiv = np.where(i > 0, np.floor((180 << 12) / (6.0 * i)), 0)")]),
    "contrast_mean_before_the_first_position_only": (("jitter",), [
        ("    img = img.copy()\n    fac, order", "    img = img.copy()\n    mean0 = _gray_u8(img).mean()\n    fac, order"),
        (_MEAN, "lut = lut + mean0 * (1 - f)")]),
}
# Two slips of the issue's list that NO input can show (test_cityscapes_contract_emulation_cpu.py proves
# each): they are planted like the others and must leave every case unchanged.
#   * nearest index without min(., W - 1): floor(x * (1 / (Ws / W))) < W for every x < Ws unless the two
#     roundings of the scale amount to a relative error of 1 / Ws, and they amount to 2^-52;
#   * s >= 1e-3 for s > 1e-3: s = (d - 1) / 256 is a multiple of 1 / 256, never float32(1e-3).
UNOBSERVABLE = {
    "nearest_without_min": (("geom7", "domain"), [
        (_NN_W, "np.floor(np.arange(Ws) * (1.0 / (float(Ws) / W))).astype(np.int64)"),
        (_NN_H, "np.floor(np.arange(Hs) * (1.0 / (float(Hs) / H))).astype(np.int64)")]),
    "s_ge_1e-3": (("domain", "geom7", "geom3"), [("use = s > np.float32(1e-3)", "use = s >= np.float32(1e-3)")]),
}
FAMILIES = {"geom7": GEOM7, "geom3": GEOM3, "domain": DOMAINS, "jitter": JITTER}


def planted_oracle(edits):
    """a copy of oracle.data_oracle with `edits` (old text, new text) applied to its source"""
    src = inspect.getsource(D)
    for old, new in edits:
        assert src.count(old) == 1, f"{old!r} occurs {src.count(old)} times in oracle/data_oracle.py"
        src = src.replace(old, new)
    mod = types.ModuleType("data_oracle_planted")
    exec(compile(src, "data_oracle_planted", "exec"), mod.__dict__)
    return mod


def expected(case, oracle=D):
    """every expected output of a PREP / JITTER case as a dict name -> array"""
    if "kind" in case:
        out = dict(zip(("img", "seg", "depth", "mask"), prep_expected(case, oracle)))
        if case["kind"] == "augment":
            out["u8"] = prep_expected_u8(case, oracle)[0]
        return out
    return {"img": jitter_expected(case, oracle)}
