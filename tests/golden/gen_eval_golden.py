"""Generate tests/golden/eval_metrics.npz by running the REFERENCE metric modules on CPU.

Run ONLY in the development container (the reference tree does not travel with the repository):

    python tests/golden/gen_eval_golden.py

The reference's compute_segmentation_metrics (segmentation/denseclip/utils.py:109-139) and
compute_depth_errors (segmentation/utils/depth_metrics.py:12-88) are loaded from their files (the
packages around them import the whole model); `ftfy` / `regex`, which utils.py imports for its
tokenizer, get stand-in modules when they are not installed.  They are fed
F.interpolate(..., 'bilinear', align_corners=False) of seeded low-res maps, exactly as the trainer's
validate() feeds them (train_denseclip.py:461-467, 497, 582, 589-593).

The reference indexes its confusion matrix with every label that is not 255 and F.cross_entropy
rejects a target outside [0, 19), so a label in 19..254 would make both raise: the reference sees
those labels as 255 (the kernel skips them the same way), and the fixture stores the labels as
generated.

Besides the reference's outputs the file holds the fp64 sums of the same formulas on the reference's
own fp32 resize (thresholds counted on the fp32 ratio, as the reference counts them): the state an
Evaluator would hold, for the CPU test of Evaluator.compute().
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_ref as R  # noqa: E402

REF_SEG = os.environ.get("DCLIP_REFERENCE", "/root/reference/segmentation")
OUT = os.path.join(HERE, "eval_metrics.npz")
B, h, w, H, W = R.SHAPES[0]


def load_reference(name, rel_path):
    for mod, attrs in (("ftfy", {"fix_text": lambda t: t}), ("regex", None)):
        try:
            __import__(mod)
        except ImportError:
            if attrs is None:
                import re
                sys.modules[mod] = re
            else:
                m = types.ModuleType(mod)
                m.__dict__.update(attrs)
                sys.modules[mod] = m
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF_SEG, rel_path))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    except Exception as e:  # the tokenizer at the end of utils.py; the metric functions are defined before it
        if not hasattr(mod, "compute_segmentation_metrics"):
            raise
        print(f"note: {rel_path} stopped after the metric functions ({type(e).__name__}: {e})")
    return mod


def main():
    seg_metrics = load_reference("ref_denseclip_utils", "denseclip/utils.py").compute_segmentation_metrics
    depth_errors = load_reference("ref_depth_metrics", "utils/depth_metrics.py").compute_depth_errors

    logits, depth = R.logits(B, h, w), R.depth_low(B, h, w)
    lab = R.labels(B, H, W, torch.uint8)
    gt, mask = R.depth_target(B, H, W), R.depth_mask(B, H, W)
    assert 0.08 < float((lab == 255).float().mean()) < 0.12 and int(((lab >= 19) & (lab < 255)).sum()) > 0
    assert float(depth.min()) >= 0.5 and float(depth.max()) <= 60 and int((gt == 0).sum()) > 0

    up_seg = F.interpolate(logits, size=(H, W), mode="bilinear", align_corners=False)
    up_depth = F.interpolate(depth, size=(H, W), mode="bilinear", align_corners=False)
    lab_ref = torch.where(R.valid_labels(lab), lab.long(), torch.full((), 255, dtype=torch.int64))

    seg = seg_metrics(up_seg, lab_ref, 19, ignore_index=255)
    preds = up_seg.argmax(1)
    cm = torch.bincount((lab_ref * 19 + preds)[lab_ref != 255], minlength=361).view(19, 19)
    acc = float((preds == lab_ref)[lab_ref != 255].sum()) / (float((lab_ref != 255).sum()) + 1e-5)
    assert abs(acc - seg["accuracy"]) < 1e-12  # the recorded matrix is the one the reference built
    iou = torch.diag(cm) / (cm.sum(0) + cm.sum(1) - torch.diag(cm) + 1e-8)
    assert np.array_equal(iou.numpy(), seg["class_iou"])
    ce = F.cross_entropy(up_seg, lab_ref, ignore_index=255)

    dm = depth_errors(gt, up_depth[:, 0], mask.bool(), min_depth=1e-3, max_depth=80.0, clamp_pred=True)
    mb = mask.bool()
    rmse_masked = torch.sqrt(torch.mean((up_depth[:, 0][mb] - gt[mb]) ** 2))  # torchmetrics MeanSquaredError(squared=False)

    # the Evaluator state of this batch: fp64 sums of the fp32 resize; thresholds counted in fp32
    sums = R.depth_sums(up_depth.double(), gt, mask)
    sums[5:8] = R.depth_sums(up_depth, gt, mask)[5:8]
    ce_sums = [R.ce_sum(up_seg.double(), lab), float(R.valid_labels(lab).sum())]

    np.savez_compressed(
        OUT, logits=logits.numpy(), depth=depth.numpy(), labels=lab.numpy(), depth_target=gt.numpy(),
        depth_mask=mask.numpy(), confusion_matrix=cm.numpy(), accuracy=np.float64(seg["accuracy"]),
        mean_iou=np.float64(seg["mean_iou"]), class_iou=np.asarray(seg["class_iou"], dtype=np.float64),
        loss_seg=np.float64(float(ce)), rmse_masked=np.float64(float(rmse_masked)),
        depth_sums=np.asarray(sums, dtype=np.float64), ce_sums=np.asarray(ce_sums, dtype=np.float64),
        **{k: np.float64(v) for k, v in dm.items()})
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; accuracy {seg['accuracy']:.6f} mIoU {seg['mean_iou']:.6f} "
          f"CE {float(ce):.6f} depth {dm} rmse_masked {float(rmse_masked):.6f}")
    assert os.path.getsize(OUT) < 512 * 1024


if __name__ == "__main__":
    main()
