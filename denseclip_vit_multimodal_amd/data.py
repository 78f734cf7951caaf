"""Cityscapes depth + segmentation data path, GPU-side.

The reference loader (seg/datasets/cityscapes_depth_seg.py) decodes three PNGs per sample,
remaps label ids, turns the uint16 disparity into metric depth and runs the trainer's
albumentations pipeline on the CPU, then ships f32 / int64 tensors (25 bytes per pixel).
Here the CPU only scans and decodes (`CityscapesDepthSegDataset`, same file layout, names and
errors as the reference); `prepare_batch` uploads the decoded uint8 / uint16 planes (6 bytes
per pixel) and one HIP kernel does the label remap, the disparity -> depth conversion, the
trainer's spatial augmentation and the normalisation, writing the batch in the layout
`train.train_step` takes:
  * `dclip_cityscapes_augment` (params from `random_scale_crops`): the whole train pipeline of
    train_denseclip.py:138-149, RandomScale(0.5..2.0) -> PadIfNeeded -> RandomCrop ->
    HorizontalFlip -> Normalize, with cv2's 8-bit INTER_CUBIC for the image (the reference's
    interpolation=Image.BILINEAR is the integer 2, which cv2 reads as INTER_CUBIC) and
    INTER_NEAREST for the label ids / disparity, restated from OpenCV's resize (cv2 is not
    installed here: that restatement is parity-unpinned against cv2 itself);
  * `dclip_cityscapes_prepare` (crops from `random_crops`): crop + flip only (no rescale).

  * ColorJitter (the reference's `color_jitter: true`, off in the Cityscapes configs): params from
    `color_jitter_params`, `dclip_color_jitter` between the spatial transforms and Normalize.

The ADE20K data path (`ADE20KSegmentation`, `ade20k_params`, `prepare_ade20k_batch`) is the second half of
this file.
"""
import os
import os.path as osp

import numpy as np
import torch



# reference constants (datasets/cityscapes_depth_seg.py:19-23) and CLIP normalisation
# (train_denseclip.py:113-114)
BASELINE_FOCAL_LENGTH = 500.0
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
SEG_IGNORE_INDEX = 255


class CityscapesDepthSegDataset:
    """File scan and PNG decode of the reference dataset (cityscapes_depth_seg.py:57-126):
    `root/leftImg8bit/<split>/<city>/*_leftImg8bit.png` with `gtFine/..._gtFine_labelIds.png` and
    `disparity/..._disparity.png`.  `__getitem__` returns the DECODED planes (uint8 HxWx3 RGB,
    uint8 HxW label ids, uint16 HxW disparity); `prepare_batch` turns a list of them into the
    training batch on the GPU.  Unlike the reference, a broken file raises instead of
    returning Nones."""

    CLASSES = ('road', 'sidewalk', 'building', 'wall', 'fence', 'pole', 'traffic light', 'traffic sign',
               'vegetation', 'terrain', 'sky', 'person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle',
               'bicycle')
    SEG_IGNORE_INDEX = SEG_IGNORE_INDEX

    def __init__(self, root, split="train", depth_max=80.0):
        self.root, self.split, self.depth_max = root, split, depth_max
        self.bf = BASELINE_FOCAL_LENGTH
        self.images_base = osp.join(root, "leftImg8bit", split)
        self.labels_base = osp.join(root, "gtFine", split)
        self.disparity_base = osp.join(root, "disparity", split)
        for d, what in ((self.images_base, "Image"), (self.labels_base, "Label"), (self.disparity_base, "Disparity")):
            if not osp.isdir(d):
                raise RuntimeError(f"{what} dir not found: {d}")
        self.img_files, self.label_files, self.disp_files = [], [], []
        for city in sorted(os.listdir(self.images_base)):
            img_dir = osp.join(self.images_base, city)
            label_dir = osp.join(self.labels_base, city)
            disp_dir = osp.join(self.disparity_base, city)
            if not (osp.isdir(img_dir) and osp.isdir(label_dir) and osp.isdir(disp_dir)):
                continue
            for fn in sorted(os.listdir(img_dir)):
                if not fn.endswith("_leftImg8bit.png"):
                    continue
                base = fn[: -len("_leftImg8bit.png")]
                lp = osp.join(label_dir, f"{base}_gtFine_labelIds.png")
                dp = osp.join(disp_dir, f"{base}_disparity.png")
                if osp.exists(lp) and osp.exists(dp):
                    self.img_files.append(osp.join(img_dir, fn))
                    self.label_files.append(lp)
                    self.disp_files.append(dp)
        if not self.img_files:
            raise RuntimeError(f"No valid data triplets found for split '{split}' in {root}")

    def __len__(self):
        return len(self.img_files)

    def __getitem__(self, idx):
        from PIL import Image
        img = np.asarray(Image.open(self.img_files[idx]).convert("RGB"), dtype=np.uint8)
        ids = np.asarray(Image.open(self.label_files[idx]), dtype=np.uint8)
        disp = np.asarray(Image.open(self.disp_files[idx])).astype(np.uint16)
        if ids.shape != img.shape[:2] or disp.shape != img.shape[:2]:
            raise RuntimeError(f"sample {idx}: image {img.shape[:2]}, labels {ids.shape}, disparity {disp.shape}")
        return img, ids, disp


def random_crops(B, H, W, h, w, generator=None, flip_p=0.5):
    """RandomCrop + HorizontalFlip parameters (y0, x0, flip) per image, int32 (B, 3)."""
    if h > H or w > W:
        raise ValueError(f"crop {h}x{w} larger than the image {H}x{W} (padding is not supported)")
    g = generator
    y0 = torch.randint(0, H - h + 1, (B,), generator=g)
    x0 = torch.randint(0, W - w + 1, (B,), generator=g)
    flip = (torch.rand(B, generator=g) < flip_p).to(torch.int64)
    return torch.stack([y0, x0, flip], 1).to(torch.int32)


def random_scale_crops(B, H, W, h, w, scale_range=(0.5, 2.0), rng=None, flip_p=0.5):
    """RandomScale + PadIfNeeded + RandomCrop + HorizontalFlip parameters per image, int32 (B, 7) =
    (Hs, Ws, pad_top, pad_left, y0, x0, flip), drawn like albumentations (train_denseclip.py:
    138-149): scale ~ U(scale_range), (Hs, Ws) = (int(H s), int(W s)); centred padding up to
    the crop, top = int(pad / 2); y0 = int((Hp - h + 1) u), x0 likewise; flip with flip_p.
    rng: a `random.Random` (albumentations draws from Python's `random`)."""
    import random
    r = rng if rng is not None else random
    out = []
    for _ in range(B):
        s = r.uniform(scale_range[0], scale_range[1])
        Hs, Ws = int(H * s), int(W * s)
        ph, pw = max(0, h - Hs), max(0, w - Ws)
        pt, pl = int(ph / 2.0), int(pw / 2.0)
        Hp, Wp = Hs + ph, Ws + pw
        y0 = int((Hp - h + 1) * r.random())
        x0 = int((Wp - w + 1) * r.random())
        out.append((Hs, Ws, pt, pl, y0, x0, int(r.random() < flip_p)))
    return torch.tensor(out, dtype=torch.int32)


def color_jitter_params(B, rng=None, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8):
    """ColorJitter(brightness, contrast, saturation, hue, p) parameters per image as albumentations
    draws them (train_denseclip.py:152-155): with probability p, factors U(1 - b, 1 + b) (clipped at
    0) for brightness / contrast / saturation, U(-hue, hue) for hue, and a random order of the four;
    otherwise the identity (1, 1, 1, 0).  float64 (B, 8): factors, then the order (0 brightness,
    1 contrast, 2 saturation, 3 hue).  rng: a `random.Random`."""
    import random
    r = rng if rng is not None else random
    out = []
    for _ in range(B):
        if r.random() < p:
            f = [r.uniform(max(0.0, 1 - brightness), 1 + brightness), r.uniform(max(0.0, 1 - contrast), 1 + contrast),
                 r.uniform(max(0.0, 1 - saturation), 1 + saturation), r.uniform(-hue, hue)]
            order = [0, 1, 2, 3]
            r.shuffle(order)
        else:
            f, order = [1.0, 1.0, 1.0, 0.0], [0, 1, 2, 3]
        out.append(f + [float(o) for o in order])
    return torch.tensor(out, dtype=torch.float64)


def prepare_batch(samples, crop_hw, crops, device, out_dtype=torch.bfloat16, mean=CLIP_MEAN, std=CLIP_STD,
                  depth_max=80.0, bf=BASELINE_FOCAL_LENGTH, jitter=None):
    """samples: list of (img uint8 HxWx3, ids uint8 HxW, disp uint16 HxW) of one size;
    crops: int32 (B, 3) (y0, x0, flip) — a window of the image (`random_crops`) — or (B, 7)
    (Hs, Ws, pad_top, pad_left, y0, x0, flip) — the rescaled / padded pipeline
    (`random_scale_crops`).  Returns (img (B,3,h,w) out_dtype, seg int64 (B,h,w), depth f32
    (B,1,h,w), mask bool (B,1,h,w)) on `device`, ready for train.train_step.  jitter: (B, 8) from
    `color_jitter_params` (needs the (B, 7) parameters) applies ColorJitter before Normalize."""
    if not samples:
        raise ValueError("empty batch")
    H, W = samples[0][1].shape
    h, w = crop_hw
    B = len(samples)
    crops = torch.as_tensor(crops, dtype=torch.int32)
    if crops.dim() == 2 and crops.shape == (B, 7):
        Hs, Ws, pt, pl, y0, x0 = (crops[:, i] for i in range(6))
        bad = (Hs < 1) | (Ws < 1) | (pt < 0) | (pl < 0) | (y0 < 0) | (x0 < 0) | \
              (y0 + h > torch.maximum(Hs + pt, torch.full_like(Hs, h))) | \
              (x0 + w > torch.maximum(Ws + pl, torch.full_like(Ws, w)))
        if bad.any():
            raise ValueError(f"bad scale / pad / crop parameters {crops.tolist()} for a {h}x{w} crop")
    else:
        crops = crops.reshape(B, 3)
        if ((crops[:, 0] < 0) | (crops[:, 0] + h > H) | (crops[:, 1] < 0) | (crops[:, 1] + w > W)).any():
            raise ValueError(f"crop windows must lie inside the {H}x{W} images (got {crops.tolist()})")
    for s in samples:
        if s[0].shape != (H, W, 3) or s[1].shape != (H, W) or s[2].shape != (H, W):
            raise ValueError("all samples of a batch must share one image size")
    jt = None
    if jitter is not None:
        # the kernel indexes a row's factors by its order entries: refuse a bad table here
        jt = torch.as_tensor(jitter, dtype=torch.float64).reshape(B, 8)
        if not bool(torch.isfinite(jt).all()):
            raise ValueError(f"ColorJitter parameters must be finite (got {jt.tolist()})")
        if not bool((jt[:, 4:].sort(1).values == torch.arange(4, dtype=torch.float64)).all()):
            raise ValueError(f"ColorJitter order must be a permutation of 0..3 per image (got {jt[:, 4:].tolist()})")
        if bool((jt[:, :3] < 0).any()):
            raise ValueError("ColorJitter brightness, contrast and saturation factors must not be negative "
                             f"(got {jt[:, :3].tolist()})")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("prepare_batch runs on the GPU (no CPU fallback)")
    pin = torch.cuda.is_available()

    def up(arrs):
        t = torch.from_numpy(np.ascontiguousarray(np.stack(arrs)))
        return (t.pin_memory() if pin else t).to(dev, non_blocking=True)

    img = up([s[0] for s in samples])
    ids = up([s[1] for s in samples])
    disp = up([s[2].view(np.int16) for s in samples])  # the uint16 bits through an int16 tensor
    cr = crops.to(dev)
    from .ops import D
    if jt is not None:
        jt = jt.to(dev)
    out_img, seg, depth, mask = D().cityscapes_prepare(img, ids, disp, cr, h, w, [float(v) for v in mean],
                                                       [float(v) for v in std], float(bf), float(depth_max), out_dtype,
                                                       jt)
    return out_img, seg, depth, mask.view(torch.bool)


# ============================================================================== ADE20K
# The reference's ADE20K sample pipeline (datasets/ade20k.py:57-185; `dataset_type: ADE20KSegmentation`,
# train_denseclip.py:176-214): PIL resize by a random scale (image BILINEAR, label NEAREST), a second
# resize up to the crop when a side fell below it, a random crop, the label shift (0 -> ignore,
# v -> v - 1) and the ImageNet normalisation.  Here the CPU scans and decodes (`ADE20KSegmentation`)
# and draws the parameters (`ade20k_params`); `prepare_ade20k_batch` uploads the decoded planes of
# the batch, of whatever sizes, as one packed uint8 buffer each, and dclip_ade20k_prepare
# (csrc/dataade.hip) runs Pillow's 8-bit resize arithmetic, the crop, the optional flip, the label
# map and the normalisation on the GPU, bit for bit what the reference's loader computes.
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
ADE_GEOM_WORDS = 12  # DCLIP_ADE_GEOM_WORDS


class ADE20KSegmentation:
    """File scan and decode of the reference dataset (datasets/ade20k.py:36-72), same arguments and
    layout: `root/ADEChallengeData2016/images/<training|validation>/*.jpg` with
    `annotations/<...>/*.png`.  `__getitem__` returns the DECODED planes (uint8 HxWx3 RGB, uint8
    HxW raw labels 0..150); `prepare_ade20k_batch` turns a list of them into the training batch on
    the GPU.  The file list is sorted (the reference keeps os.listdir's order); a missing or
    mismatched file raises.  `class_names` comes from the dataset's own objectInfo150.txt."""

    def __init__(self, root, split="training", crop_size=512, scale=(0.5, 2.0), ignore_label=255):
        self.root, self.split, self.crop_size, self.scale, self.ignore_label = root, split, crop_size, scale, ignore_label
        sub = "training" if split == "training" else "validation"
        self.base = osp.join(root, "ADEChallengeData2016")
        self.image_dir = osp.join(self.base, "images", sub)
        self.label_dir = osp.join(self.base, "annotations", sub)
        for d, what in ((self.image_dir, "Image"), (self.label_dir, "Label")):
            if not osp.isdir(d):
                raise RuntimeError(f"{what} dir not found: {d}")
        self.filenames = sorted(f[:-len(".jpg")] for f in os.listdir(self.image_dir) if f.endswith(".jpg"))
        if not self.filenames:
            raise RuntimeError(f"No .jpg images found for split '{split}' in {self.image_dir}")
        self._class_names = None

    @property
    def crop_hw(self):
        c = self.crop_size
        return (c, c) if isinstance(c, int) else (int(c[0]), int(c[1]))

    def __len__(self):
        return len(self.filenames)

    def __getitem__(self, idx):
        from PIL import Image
        ip = osp.join(self.image_dir, self.filenames[idx] + ".jpg")
        lp = osp.join(self.label_dir, self.filenames[idx] + ".png")
        if not osp.exists(lp):
            raise FileNotFoundError(f"sample {idx}: no label file {lp} for {ip}")
        img = np.asarray(Image.open(ip).convert("RGB"), dtype=np.uint8)
        lab = np.asarray(Image.open(lp), dtype=np.uint8)
        if lab.shape != img.shape[:2]:
            raise RuntimeError(f"sample {idx}: image {img.shape[:2]}, labels {lab.shape}")
        return img, lab

    @property
    def class_names(self):
        """The 150 class names from `ADEChallengeData2016/objectInfo150.txt` (tab-separated Idx, Ratio, Train,
        Val, Name under one header row): the first comma-separated synonym of each Name."""
        if self._class_names is None:
            path = osp.join(self.base, "objectInfo150.txt")
            if not osp.exists(path):
                raise FileNotFoundError(f"class names: {path} not found")
            with open(path) as f:
                rows = [ln.rstrip("\n") for ln in f if ln.strip()]
            head = [c.strip().lower() for c in rows[0].split("\t")]
            if "name" not in head:
                raise RuntimeError(f"{path}: no Name column in {rows[0]!r}")
            col = head.index("name")
            self._class_names = tuple(r.split("\t")[col].split(",")[0].strip() for r in rows[1:])
        return self._class_names


def ade20k_params(sizes, crop_hw, scale=(0.5, 2.0), rng=None, flip_p=0.0):
    """Per-sample parameters of the reference pipeline, int64 (B, 7) = (H1, W1, H2, W2, y0, x0, flip).
    sizes: (H, W) of each decoded sample; crop_hw = (crop_h, crop_w).  Per sample, in the reference's
    order and integer arithmetic (ade20k.py:75-134): s = uniform(*scale), (W1, H1) = (int(W s), int(H s));
    when W1 < crop_w or H1 < crop_h the second resize's target (W2, H2) (ade20k.py:97-118: the smaller
    side to the crop, the other by int(target / aspect) or int(target * aspect), then max(target, crop)),
    else (W2, H2) = (W1, H1); x0 = randint(0, max(0, W2 - crop_w) + 1), then y0 likewise.
    rng: a numpy.random.RandomState (default: numpy's global one, which the reference draws from);
    RandomState(seed) reproduces the reference under np.random.seed(seed), one sample per seed state.
    flip_p > 0 (an extension, off by default) draws a horizontal flip last.  A rescaled side below 1
    raises ValueError."""
    r = rng if rng is not None else np.random
    crop_h, crop_w = (int(v) for v in crop_hw)
    if crop_h < 1 or crop_w < 1:
        raise ValueError(f"crop {crop_h}x{crop_w} must be at least 1x1")
    out = []
    for H, W in sizes:
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"image size {H}x{W} must be at least 1x1")
        s = r.uniform(*scale)
        w, h = int(W * s), int(H * s)
        if w < 1 or h < 1:
            raise ValueError(f"scale {s} leaves a {H}x{W} image with a side below 1 ({h}x{w})")
        H1, W1 = h, w
        if w < crop_w or h < crop_h:
            aspect_ratio = w / h
            target_w, target_h = w, h
            if w < crop_w and h < crop_h:
                if w / crop_w < h / crop_h:
                    target_w = crop_w
                    target_h = int(target_w / aspect_ratio)
                else:
                    target_h = crop_h
                    target_w = int(target_h * aspect_ratio)
            elif w < crop_w:
                target_w = crop_w
                target_h = int(target_w / aspect_ratio)
            else:
                target_h = crop_h
                target_w = int(target_h * aspect_ratio)
            w, h = max(target_w, crop_w), max(target_h, crop_h)
        x0 = r.randint(0, max(0, w - crop_w) + 1)
        y0 = r.randint(0, max(0, h - crop_h) + 1)
        flip = int(r.random_sample() < flip_p) if flip_p > 0 else 0
        out.append((H1, W1, h, w, int(y0), int(x0), flip))
    return torch.tensor(out, dtype=torch.int64).reshape(len(out), 7)


def ade20k_geometry(sizes, params, crop_hw):
    """The (B, ADE_GEOM_WORDS) int64 geometry table of dclip_ade20k_prepare (include/dclip.h) for samples of
    `sizes` packed back to back: byte offsets of each image / label plane, the sizes of the source and of both
    resizes, the crop origin and the flip.  Returns (table, image bytes, label bytes)."""
    prm = torch.as_tensor(params, dtype=torch.int64).reshape(len(sizes), 7).tolist()
    rows, io, lo = [], 0, 0
    for (H, W), (H1, W1, H2, W2, y0, x0, flip) in zip(sizes, prm):
        rows.append((io, lo, int(H), int(W), H1, W1, H2, W2, y0, x0, flip, 0))
        io += int(H) * int(W) * 3
        lo += int(H) * int(W)
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), ADE_GEOM_WORDS), io, lo


def prepare_ade20k_batch(samples, crop_hw, params, device, out_dtype=torch.bfloat16, mean=IMAGENET_MEAN,
                         std=IMAGENET_STD, ignore_label=255):
    """samples: list of (img uint8 HxWx3, lab uint8 HxW) of ANY sizes (`ADE20KSegmentation.__getitem__`);
    params: (B, 7) from `ade20k_params`.  Returns (img (B,3,h,w) out_dtype, seg int64 (B,h,w), None, None) on
    `device`: the batch train.train_step / train_step_accum / evaluate.validate take for a seg-only model.
    The image is float32(u8) / 255, then (. - mean) / std; the label v > 0 -> v - 1, 0 -> ignore_label
    (unchanged with ignore_label=None).  crop_hw=None with one sample (and params=None) returns the
    whole image with no resize, for validation.

    The crop is (x0, y0, x0 + crop_w, y0 + crop_h) for both image and label.  The reference crops the label
    with x0 + crop_h as its right edge (ade20k.py:136), a slip that shows for non-square crops only; square
    crops are identical."""
    if not samples:
        raise ValueError("empty batch")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("prepare_ade20k_batch runs on the GPU (no CPU fallback)")
    B = len(samples)
    sizes = []
    for i, (im, lb) in enumerate(samples):
        if im.dtype != np.uint8 or lb.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or lb.shape != im.shape[:2]:
            raise ValueError(f"sample {i}: uint8 (H, W, 3) image and uint8 (H, W) labels expected, got "
                             f"{im.dtype} {im.shape} and {lb.dtype} {lb.shape}")
        sizes.append(lb.shape)
    if crop_hw is None:
        if B != 1:
            raise ValueError("crop_hw=None (the whole image) takes one sample: images of a batch differ in size")
        H, W = sizes[0]
        h, w = H, W
        if params is None:
            params = [(H, W, H, W, 0, 0, 0)]
    else:
        h, w = (int(v) for v in crop_hw)
    prm = torch.as_tensor(params, dtype=torch.int64).reshape(B, 7)
    H2, W2, y0, x0 = prm[:, 2], prm[:, 3], prm[:, 4], prm[:, 5]
    if bool(((prm[:, :4] < 1).any(1) | (y0 < 0) | (x0 < 0) | (y0 + h > H2) | (x0 + w > W2)).any()):
        raise ValueError(f"bad resize / crop parameters {prm.tolist()} for a {h}x{w} crop")
    geom, _, _ = ade20k_geometry(sizes, prm, (h, w))
    pin = torch.cuda.is_available()

    def up(t):
        return (t.pin_memory() if pin else t).to(dev, non_blocking=True)

    img = up(torch.from_numpy(np.concatenate([np.ascontiguousarray(s[0]).reshape(-1) for s in samples])))
    lab = up(torch.from_numpy(np.concatenate([np.ascontiguousarray(s[1]).reshape(-1) for s in samples])))
    from . import _torch_ops
    _torch_ops.load()
    out_img, seg = torch.ops.dclip_data.ade20k_prepare(img, lab, up(geom), geom, h, w, [float(v) for v in mean],
                                                       [float(v) for v in std],
                                                       -1 if ignore_label is None else int(ignore_label), out_dtype)
    return out_img, seg, None, None
