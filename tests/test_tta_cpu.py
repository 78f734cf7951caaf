"""CPU checks of the test-time-ensembling path (csrc/headensemble.hip, torch.ops.dclip_eval.ensemble_*,
evaluate.py): the three new entry points are declared, bound and exported beside an unchanged ABI
version; their host checks reject bad arguments before any launch with a message that names the
value; the workspace size is a function of its arguments alone; the four ops are registered with
fake implementations and refuse CPU tensors; tta_views yields the right sizes and flags; an unknown
averaging rule raises; the alias package re-exports the new names."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT
from denseclip_vit_multimodal_amd import _native as N

NEW = ["dclip_ensemble_eval_depth", "dclip_ensemble_eval_seg", "dclip_ensemble_eval_ws_bytes"]
P = 0x1000  # a non-null pointer the host checks never dereference


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", src, re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert lib.dclip_ensemble_eval_ws_bytes.restype is ctypes.c_int64
    assert "dclip_view" in src and int(re.search(r"#define DCLIP_ENSEMBLE_MAX_VIEWS (\d+)", src).group(1)) == 16
    assert N.ENSEMBLE_MAX_VIEWS == 16
    # dclip_view as C lays it out: pointer, three ints, padded to the pointer's alignment
    assert ctypes.sizeof(N.View) == 24 and N.View.h.offset == 8 and N.View.flip.offset == 16


def _views(views):
    return N.view_table([(p, h, w, f) for p, h, w, f in views])


ONE = [(P, 4, 8, 0)]


def _seg(L, views=ONE, nviews=None, K=19, B=1, H=64, W=128, average=0, labels=P, pred=P, cm=P, loss=P, count=P, ws=P,
         low_dt=0, lab_dt=0):
    tab = _views(views) if views else None
    return L.dclip_ensemble_eval_seg(low_dt, tab, len(views) if nviews is None else nviews, B, K, average, labels,
                                     lab_dt, H, W, 255, pred, cm, loss, count, ws, None)


def _depth(L, views=ONE, nviews=None, B=1, H=64, W=128, target=P, up=None, sums=P, ws=P, low_dt=0):
    tab = _views(views) if views else None
    return L.dclip_ensemble_eval_depth(low_dt, tab, len(views) if nviews is None else nviews, B, target, None, H, W,
                                       1e-3, 80.0, 1, 1e-6, up, sums, ws, None)


@pytest.mark.parametrize("call,needle", [
    (lambda L: _seg(L, nviews=0), "nviews=0"),
    (lambda L: _seg(L, views=ONE * 17), "nviews=17"),
    (lambda L: _seg(L, K=20), "K=20"),
    (lambda L: _seg(L, views=[(P, 4, 8, 0), (None, 4, 8, 1)]), "view 1: low is null"),
    (lambda L: _seg(L, views=[(P, 4, 8, 2)]), "flip=2"),
    (lambda L: _seg(L, views=[(P, 4, 8, 0), (P, 4, 8, -1)]), "flip=-1"),
    (lambda L: _seg(L, average=2), "average=2"),
    (lambda L: _seg(L, views=[(P, 4, 8, 0), (P, 65, 8, 0)]), "smaller than the input (65 x 8)"),
    (lambda L: _seg(L, views=[(P, 4, 129, 1)]), "smaller than the input (4 x 129)"),
    (lambda L: _seg(L, B=8, H=16384, W=16384), "B*H*W = 2147483648"),
    (lambda L: _seg(L, cm=None), "cm, loss_sum and count required"),
    (lambda L: _seg(L, labels=None), "must be null without labels"),
    (lambda L: _seg(L, labels=None, pred=None, cm=None, loss=None, count=None), "nothing to do"),
    (lambda L: _seg(L, ws=None), "ws="),
    (lambda L: _seg(L, ws=0x1004), "ws=0x1004"),
    (lambda L: _seg(L, low_dt=5), "low_dt=5"),
    (lambda L: _seg(L, lab_dt=3), "lab_dt=3"),
    (lambda L: _depth(L, nviews=0), "nviews=0"),
    (lambda L: _depth(L, views=ONE * 17), "nviews=17"),
    (lambda L: _depth(L, views=[(None, 4, 8, 0)]), "view 0: low is null"),
    (lambda L: _depth(L, views=[(P, 4, 8, 3)]), "flip=3"),
    (lambda L: _depth(L, views=[(P, 65, 8, 0)]), "smaller than the input (65 x 8)"),
    (lambda L: _depth(L, B=2, H=32768, W=32768), "B*H*W = 2147483648"),
    (lambda L: _depth(L, sums=None), "sums required"),
    (lambda L: _depth(L, ws=None), "ws="),
    (lambda L: _depth(L, ws=0x1004), "ws=0x1004"),
    (lambda L: _depth(L, target=None, up=None, sums=None, ws=None), "nothing to do"),
    (lambda L: _depth(L, low_dt=-1), "low_dt=-1"),
], ids=["seg_no_views", "seg_17_views", "K20", "seg_null_low", "seg_flip2", "seg_flip_neg", "average2", "seg_h_gt_H",
        "seg_w_gt_W", "seg_2^31", "null_cm", "cm_without_labels", "seg_nothing", "seg_null_ws", "seg_odd_ws",
        "seg_dtype", "label_dtype", "depth_no_views", "depth_17_views", "depth_null_low", "depth_flip3",
        "depth_h_gt_H", "depth_2^31", "null_sums", "depth_null_ws", "depth_odd_ws", "depth_nothing", "depth_dtype"])
def test_host_checks_reject_before_any_launch(call, needle):
    """every pointer is null or 0x1000: a launch would fault, a host check returns -1 first"""
    L = N.load()
    assert call(L) == -1
    assert needle in L.dclip_last_error().decode(), L.dclip_last_error().decode()


def test_ws_bytes_is_a_function_of_its_arguments_alone():
    L = N.load()
    args = [(8, 19, 12), (1, 19, 1), (2, 1, 16), (8, 1, 3)]
    base = [L.dclip_ensemble_eval_ws_bytes(*a) for a in args]
    assert all(b > 0 and b % 8 == 0 for b in base)
    # no smaller than the single-view workspace: the folds are shared
    assert base[0] >= L.dclip_upsample_eval_ws_bytes(8, 19, 64, 128)
    for bad in ((0, 19, 4), (1, 19, 0), (1, 19, 17), (1, 0, 4)):
        assert L.dclip_ensemble_eval_ws_bytes(*bad) == 0, bad
    touched = []
    try:
        for opt in range(20):
            for value in (1, 2, 7):
                if L.dclip_set_option(opt, value) == 0:
                    touched.append(opt)
                    assert [L.dclip_ensemble_eval_ws_bytes(*a) for a in args] == base, (opt, value)
    finally:
        for opt in set(touched):
            L.dclip_set_option(opt, 0)


def test_ensemble_ops_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    E = torch.ops.dclip_eval
    for name in ("ensemble_argmax", "ensemble_seg_update", "ensemble_depth", "ensemble_depth_update"):
        assert hasattr(E, name), name
    assert str(E.ensemble_seg_update.default._schema.returns[0].type) == "Optional[Tensor]"
    assert str(E.ensemble_depth_update.default._schema.returns[0].type) == "Optional[Tensor]"
    with FakeTensorMode():
        dev = "cuda"
        lgs = [torch.empty(2, 19, h, 2 * h, device=dev, dtype=torch.bfloat16) for h in (4, 8, 12)]
        flips = [0, 1, 0]
        lab = torch.empty(2, 128, 256, device=dev, dtype=torch.uint8)
        cm = torch.empty(19, 19, device=dev, dtype=torch.int64)
        ce = torch.empty(2, device=dev, dtype=torch.float64)
        for probs in (False, True):
            pm = E.ensemble_argmax(lgs, flips, 128, 256, probs)
            assert pm.shape == (2, 128, 256) and pm.dtype == torch.uint8 and pm.device.type == "cuda"
            pm = E.ensemble_seg_update(lgs, flips, lab, 255, probs, cm, ce, True)
            assert pm.shape == (2, 128, 256) and pm.dtype == torch.uint8
            assert E.ensemble_seg_update(lgs, flips, lab, 255, probs, cm, ce, False) is None
        dps = [torch.empty(2, 1, h, 2 * h, device=dev, dtype=torch.float16) for h in (4, 8, 12)]
        up = E.ensemble_depth(dps, flips, 128, 256)
        assert up.shape == (2, 1, 128, 256) and up.dtype == torch.float32 and up.device.type == "cuda"
        tg = torch.empty(2, 128, 256, device=dev)
        sums = torch.empty(12, device=dev, dtype=torch.float64)
        up = E.ensemble_depth_update(dps, flips, tg, None, 1e-3, 80.0, True, 1e-6, sums, True)
        assert up.shape == (2, 1, 128, 256) and up.dtype == torch.float32
        assert E.ensemble_depth_update(dps, flips, tg, lab, 1e-3, 80.0, True, 1e-6, sums, False) is None


def test_cpu_tensors_are_refused():
    """no CPU kernel behind the ops, and the Python layer says so before it reaches them"""
    from denseclip_vit_multimodal_amd import _torch_ops
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    _torch_ops.load()
    E = torch.ops.dclip_eval
    lgs, dps = [torch.zeros(1, 19, 4, 8)], [torch.zeros(1, 1, 4, 8)]
    with pytest.raises(NotImplementedError):
        E.ensemble_argmax(lgs, [0], 64, 128, False)
    with pytest.raises(NotImplementedError):
        E.ensemble_depth(dps, [0], 64, 128)
    with pytest.raises(NotImplementedError):
        E.ensemble_seg_update(lgs, [0], torch.zeros(1, 64, 128, dtype=torch.int64), 255, False,
                              torch.zeros(19, 19, dtype=torch.int64), torch.zeros(2, dtype=torch.float64), False)
    with pytest.raises(NotImplementedError):
        E.ensemble_depth_update(dps, [0], torch.zeros(1, 64, 128), None, 1e-3, 80.0, True, 1e-6,
                                torch.zeros(12, dtype=torch.float64), False)
    ev = Evaluator(device="cpu")
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ev.update_views(lgs, None, [0], seg_target=torch.zeros(1, 64, 128, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ev.update_views(None, dps, [0], depth_target=torch.zeros(1, 64, 128))


def test_tta_views_sizes_flags_and_passthrough():
    from denseclip_vit_multimodal_amd.evaluate import TTA_SCALES, tta_views
    assert TTA_SCALES == (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
    img = torch.randn(2, 3, 10, 22, generator=torch.Generator().manual_seed(5))
    views = list(tta_views(img))
    assert [f for _, f in views] == [False, True] * 6
    sizes = [(int(10 * s + 0.5), int(22 * s + 0.5)) for s in TTA_SCALES]
    assert sizes[0] == (5, 11) and sizes[1] == (8, 17) and sizes[5] == (18, 39)  # int(7.5 + 0.5), int(16.5 + 0.5)
    for i, s in enumerate(sizes):
        plain, flipped = views[2 * i][0], views[2 * i + 1][0]
        assert tuple(plain.shape) == (2, 3) + s and torch.equal(flipped, plain.flip(-1))
    assert views[4][0] is img  # scale 1: the image itself, not a resized copy
    want = torch.nn.functional.interpolate(img, size=sizes[3], mode="bilinear", align_corners=False)
    assert torch.equal(views[6][0], want)
    plain_only = list(tta_views(img, scales=(0.5, 1.0), flip=False))
    assert [f for _, f in plain_only] == [False, False] and plain_only[1][0] is img


def test_unknown_average_raises():
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, predict_tta, validate
    for call in (lambda: predict_tta(None, torch.zeros(1, 3, 8, 8), average="foo"),
                 lambda: Evaluator(device="cpu").update_views([], [], [], average="foo"),
                 lambda: validate(torch.nn.Identity(), [], tta=dict(average="foo"))):
        with pytest.raises(ValueError) as e:
            call()
        assert "logits" in str(e.value) and "probs" in str(e.value) and "foo" in str(e.value)
    with pytest.raises(ValueError, match="scale"):
        validate(torch.nn.Identity(), [], tta=dict(scale=(1.0,)))


def test_alias_package_reexports_the_new_names():
    import denseclip.evaluate as ev
    from denseclip_vit_multimodal_amd import evaluate
    assert ev is evaluate
    for name in ("TTA_SCALES", "tta_views", "forward_views", "predict_tta"):
        assert hasattr(ev, name), name
    assert hasattr(ev.Evaluator, "update_views")
    import inspect
    sig = inspect.signature(ev.validate)
    assert sig.parameters["tta"].default is None
    from denseclip_vit_multimodal_amd import DenseCLIP
    assert "predict_tta" in DenseCLIP.aug_test.__doc__ and "un-mirrored" in DenseCLIP.aug_test.__doc__
