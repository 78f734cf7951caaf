"""Golden vectors for the ADE20K sample pipeline, produced by the REFERENCE's own loader
(datasets/ade20k.py: ADE20KSegmentation.__getitem__) on a tiny synthetic dataset tree.  Run ONLY in
the development container, with PIL and the reference checkout at hand:

    DENSECLIP_REFERENCE=<reference checkout> python tests/golden/gen_ade20k.py   # writes tests/golden/ade20k/*.npz

Each file holds one sample: the decoded uint8 image and the raw label plane exactly as the reference
saw them (np.asarray of what it opened), the seed given to np.random.seed before __getitem__, the crop
size, the parameters `ade20k_params(RandomState(seed))` draws for it, and the reference's outputs
(float64 (3, h, w) image, int64 label).  For a non-square crop the reference's label is crop_h wide
(its crop uses x + crop_h as the right edge, ade20k.py:136).

The (size, crop, seed) cases are searched, not hand-picked: for every configuration below the seeds
0 .. SEEDS-1 are classified by what their parameters exercise (test_ade20k_cpu.COVERAGE), and a greedy
cover takes the first seeds that add a property not yet seen.
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEEDS = 600
# (H, W) of the source, crop_size as the reference takes it (int, or (crop_h, crop_w))
CONFIGS = [((37, 53), 32), ((64, 48), 32), ((96, 128), 32), ((64, 48), (40, 36)), ((37, 53), (40, 36)),
           ((26, 30), (26, 30)), ((48, 64), (34, 38))]


def properties(size, crop_hw, prm):
    """what one sample's parameters exercise (the names test_ade20k_cpu.COVERAGE lists)"""
    import ade_ref as R
    H, W = size
    ch, cw = crop_hw
    H1, W1, H2, W2, y0, x0, _ = (int(v) for v in prm)
    got = set()
    if H1 < H and W1 < W:
        got.add("downscale")
    if H1 > H and W1 > W:
        got.add("upscale")
    second = R.second_resize(W1, H1, cw, ch)
    if second is not None:
        assert second[:2] == (W2, H2)
        got.add("second_" + second[2])
        if second[3]:
            got.add("clamp")
    if W2 == cw:
        got.add("x_max_0")
    if W2 > cw and H2 > ch and x0 == W2 - cw and y0 == H2 - ch:
        got.add("right_bottom")
    if cw % 4:
        got.add("width_not_x4")
    return got


def synth(size, seed):
    """a smooth image with some texture (so the JPEG stays small) and a blocky label plane holding 0, 1, 150, 255"""
    H, W = size
    g = np.random.RandomState(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([127 + 120 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (4.0 + c)) for c in range(3)], -1)
    img = np.clip(img + g.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)
    blocks = g.randint(0, 151, ((H + 4) // 5, (W + 6) // 7)).astype(np.uint8)
    lab = np.kron(blocks, np.ones((5, 7), dtype=np.uint8))[:H, :W].copy()
    lab[0, :3] = (0, 1, 150)
    lab[H // 2, W // 2:W // 2 + 2] = 255
    lab[-1, -3:] = (150, 0, 1)
    return img, lab


def main():
    from PIL import Image
    from denseclip_vit_multimodal_amd.data import ade20k_params
    ref_root = os.environ.get("DENSECLIP_REFERENCE")
    if not ref_root:
        raise SystemExit("set DENSECLIP_REFERENCE to the reference checkout")
    # by file path: `datasets` would resolve to the installed HuggingFace package
    spec = importlib.util.spec_from_file_location("ref_ade20k", os.path.join(ref_root, "segmentation", "datasets", "ade20k.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out_dir = os.path.join(HERE, "ade20k")
    os.makedirs(out_dir, exist_ok=True)
    seen, cases = set(), []
    for size, crop in CONFIGS:
        crop_hw = (crop, crop) if isinstance(crop, int) else crop
        for seed in range(SEEDS):
            prm = ade20k_params([size], crop_hw, rng=np.random.RandomState(seed))[0].tolist()
            new = properties(size, crop_hw, prm) - seen
            if new:
                seen |= new
                cases.append((size, crop, seed, prm))
    print("covered:", sorted(seen))
    total = 0
    for i, (size, crop, seed, prm) in enumerate(cases):
        crop_hw = (crop, crop) if isinstance(crop, int) else crop
        img, lab = synth(size, seed)
        with tempfile.TemporaryDirectory() as tmp:
            for sub, arr, name in (("images", img, "s_0001.jpg"), ("annotations", lab, "s_0001.png")):
                d = os.path.join(tmp, "ADEChallengeData2016", sub, "training")
                os.makedirs(d)
                Image.fromarray(arr).save(os.path.join(d, name), **({"quality": 90} if sub == "images" else {}))
            ds = mod.ADE20KSegmentation(tmp, split="training", crop_size=crop)
            seen_img = np.asarray(Image.open(os.path.join(ds.image_dir, "s_0001.jpg")).convert("RGB"), dtype=np.uint8)
            seen_lab = np.asarray(Image.open(os.path.join(ds.label_dir, "s_0001.png")), dtype=np.uint8)
            np.random.seed(seed)
            ref_img, ref_lab = ds[0]
        assert set(np.unique(seen_lab)) >= {0, 1, 150, 255}
        path = os.path.join(out_dir, f"case{i:02d}.npz")
        np.savez_compressed(path, img=seen_img, lab=seen_lab, seed=np.int64(seed), crop_hw=np.asarray(crop_hw, dtype=np.int64),
                            params=np.asarray(prm, dtype=np.int64), ref_img=ref_img.numpy(), ref_lab=ref_lab.numpy())
        total += os.path.getsize(path)
        print(f"case{i:02d}: {size} crop {crop_hw} seed {seed} params {prm} -> {sorted(properties(size, crop_hw, prm))}")
    print(f"{len(cases)} cases, {total} bytes")


if __name__ == "__main__":
    main()
