"""NumPy restatement of the reference's ADE20K sample pipeline (datasets/ade20k.py:57-185): the checker
of `prepare_ade20k_batch` / dclip_ade20k_prepare.  Never imported by the product.

Pillow's 8-bit resize, restated from its algorithm (Resample.c, Geometry.c):

BILINEAR is separable, the horizontal pass first, each pass writing uint8; a pass whose input and
output sizes are equal is skipped.  Per output coordinate xx of a pass inS -> outS, in f64:
    scale = inS / outS, fs = max(scale, 1), support = fs, center = (xx + 0.5) scale
    xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), inS)
    w_x = max(0, 1 - |(x + xmin - center + 0.5) (1 / fs)|), divided by their sum ww (in index order)
    k_x = int(0.5 + w_x 2^22)           (-0.5 for a negative w_x)
    out = clip(((1 << 21) + sum px k_x) >> 22, 0, 255)
NEAREST reads source index int(xo), xo = a0 / 2 for output 0 and one accumulated `xo += a0` per
further output (a0 = inS / outS): the table is built serially, not as (x + 0.5) a0.

`test_ade20k_cpu.py` holds this file bit for bit to PIL itself (where PIL is importable) and to
outputs recorded from the reference's own loader (tests/golden/ade20k).
"""
import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22


def bilinear_table(inS, outS):
    """[(xmin, int coefficients k_0 .. k_{n-1})] per output coordinate of a pass inS -> outS"""
    scale = inS / outS
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    out = []
    for xx in range(outS):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), inS)
        w = []
        for x in range(xmax - xmin):
            v = (x + xmin - center + 0.5) * ss
            v = -v if v < 0 else v
            w.append(1.0 - v if v < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
                           for v in w]))
    return out


def _pass(a, outS, axis):
    """one separable pass along `axis` of a uint8 (H, W, C) array"""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    res = np.empty((outS,) + a.shape[1:], dtype=np.uint8)
    for xx, (xmin, k) in enumerate(bilinear_table(a.shape[0], outS)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(np.asarray(k, dtype=np.int64), a[xmin:xmin + len(k)], axes=(0, 0))
        res[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(res, 0, axis)


def resize_bilinear(img, out_w, out_h):
    """PIL Image.resize((out_w, out_h), BILINEAR) of a uint8 (H, W, 3) array"""
    if img.shape[1] != out_w:
        img = _pass(img, out_w, 1)
    if img.shape[0] != out_h:
        img = _pass(img, out_h, 0)
    return np.ascontiguousarray(img)


def nearest_table(inS, outS):
    a0 = inS / outS
    xo = a0 * 0.5
    tab = []
    for _ in range(outS):
        tab.append(int(xo))
        xo += a0
    return np.asarray(tab, dtype=np.int64)


def resize_nearest(lab, out_w, out_h):
    """PIL Image.resize((out_w, out_h), NEAREST) of a uint8 (H, W) array"""
    if lab.shape == (out_h, out_w):
        return lab.copy()
    return lab[nearest_table(lab.shape[0], out_h)][:, nearest_table(lab.shape[1], out_w)]


def second_resize(w, h, crop_w, crop_h):
    """(target_w, target_h, branch, clamped) of ade20k.py:97-118 for a w x h image, or None when the image
    covers the crop.  branch: 'both_w' / 'both_h' (both sides smaller; the width / the height proportionally
    smaller), 'w', 'h'; clamped: max(target, crop) raised a side."""
    if not (w < crop_w or h < crop_h):
        return None
    aspect_ratio = w / h
    tw, th = w, h
    if w < crop_w and h < crop_h:
        if w / crop_w < h / crop_h:
            branch, tw = "both_w", crop_w
            th = int(tw / aspect_ratio)
        else:
            branch, th = "both_h", crop_h
            tw = int(th * aspect_ratio)
    elif w < crop_w:
        branch, tw = "w", crop_w
        th = int(tw / aspect_ratio)
    else:
        branch, th = "h", crop_h
        tw = int(th * aspect_ratio)
    return max(tw, crop_w), max(th, crop_h), branch, (tw < crop_w or th < crop_h)


def map_labels(lab, ignore_label=255):
    out = lab.astype(np.int64)
    if ignore_label is not None:
        out = np.where(out > 0, out - 1, ignore_label)
    return out


def normalize(u8_hwc, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """float32(u8) / 255 in f32, (. - mean) / std in f64, HWC -> CHW (ade20k.py:178-182)"""
    x = u8_hwc.astype(np.float32) / 255.0
    return ((x - np.array(mean)) / np.array(std)).transpose(2, 0, 1)


def sample(img, lab, prm, crop_hw, ignore_label=255, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """One sample through the pipeline.  prm = (H1, W1, H2, W2, y0, x0, flip) as `ade20k_params` draws
    them; crop_hw = (h, w).  Returns (image f64 (3, h, w), label int64 (h, w), uint8 crop (h, w, 3))."""
    H1, W1, H2, W2, y0, x0, flip = (int(v) for v in prm)
    h, w = crop_hw
    a, b = resize_bilinear(img, W1, H1), resize_nearest(lab, W1, H1)
    if (H2, W2) != (H1, W1):
        a, b = resize_bilinear(a, W2, H2), resize_nearest(b, W2, H2)
    a, b = a[y0:y0 + h, x0:x0 + w], b[y0:y0 + h, x0:x0 + w]
    assert a.shape == (h, w, 3) and b.shape == (h, w), "crop window outside the image"
    if flip:
        a, b = a[:, ::-1], b[:, ::-1]
    a = np.ascontiguousarray(a)
    return normalize(a, mean, std), map_labels(b, ignore_label), a


def ulp16(x, dtype):
    """the spacing of `dtype` (torch.bfloat16 / float16) at |x| (numpy f64 in, f64 out)"""
    import torch
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** emin)))
    return 2.0 ** (e - mant)
