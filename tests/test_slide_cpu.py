"""CPU checks of the sliding-window path (csrc/headslide.hip, torch.ops.dclip_eval.slide_*,
evaluate.py): the three new entry points are declared, bound and exported beside an unchanged ABI
version; their host checks reject bad arguments before any launch with a message that names the
value, an uncovered pixel included; the workspace size is a function of its arguments alone;
slide_windows places the windows by mmseg's rule; the four ops are registered with fake
implementations and refuse CPU tensors; validate refuses slide with tta and slide=True without a
slide test_cfg; the alias package re-exports the new names."""
import ctypes
import os
import re

import pytest
import torch

import slide_ref as S
from helpers import ROOT
from denseclip_vit_multimodal_amd import _native as N

NEW = ["dclip_slide_eval_depth", "dclip_slide_eval_seg", "dclip_slide_eval_ws_bytes"]
P = 0x1000  # a non-null pointer the host checks never dereference


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", src, re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert lib.dclip_slide_eval_ws_bytes.restype is ctypes.c_int64
    assert "dclip_window" in src and int(re.search(r"#define DCLIP_SLIDE_MAX_WINDOWS (\d+)", src).group(1)) == 64
    assert N.SLIDE_MAX_WINDOWS == 64
    # dclip_window as C lays it out: pointer, two ints
    assert ctypes.sizeof(N.Window) == 16 and N.Window.y0.offset == 8 and N.Window.x0.offset == 12
    assert "mode='slide'" in src and "denseclip_fpn_vit-b_640x640_80k.py:51" in src


# the `thirds` geometry: 64 x 128, windows 32 x 64 from 2 x 4 maps
THIRDS = [(P, y, x) for y in (0, 21, 32) for x in (0, 42, 64)]


def _seg(L, wins=THIRDS, nwin=None, K=19, B=1, h=2, w=4, wh=32, ww=64, H=64, W=128, labels=P, pred=P, cm=P, loss=P,
         count=P, ws=P, low_dt=0, lab_dt=0):
    tab = N.window_table(wins) if wins else None
    return L.dclip_slide_eval_seg(low_dt, tab, len(wins) if nwin is None else nwin, B, K, h, w, wh, ww, labels, lab_dt,
                                  H, W, 255, pred, cm, loss, count, ws, None)


def _depth(L, wins=THIRDS, nwin=None, B=1, h=2, w=4, wh=32, ww=64, H=64, W=128, target=P, up=None, sums=P, ws=P,
           low_dt=0):
    tab = N.window_table(wins) if wins else None
    return L.dclip_slide_eval_depth(low_dt, tab, len(wins) if nwin is None else nwin, B, h, w, wh, ww, target, None, H,
                                    W, 1e-3, 80.0, 1, 1e-6, up, sums, ws, None)


FULL = [(P, 0, 0)]  # one window over the whole image, with wh = H and ww = W
GAP = [(P, 0, 0), (P, 0, 70)]  # 64 x 64 windows on a 64 x 134 image: columns 64 .. 69 uncovered


@pytest.mark.parametrize("call,needle", [
    (lambda L: _seg(L, nwin=0), "nwin=0"),
    (lambda L: _seg(L, wins=FULL * 65, wh=64, ww=128), "nwin=65"),
    (lambda L: _seg(L, K=20), "K=20"),
    (lambda L: _seg(L, low_dt=5), "low_dt=5"),
    (lambda L: _seg(L, lab_dt=3), "lab_dt=3"),
    (lambda L: _seg(L, wins=[(P, 0, 0), (None, 0, 64)]), "window 1: low is null"),
    (lambda L: _seg(L, h=33), "h=33 <= wh=32"),
    (lambda L: _seg(L, wh=65), "wh=65 <= H=64"),
    (lambda L: _seg(L, w=65), "w=65 <= ww=64"),
    (lambda L: _seg(L, ww=129), "ww=129 <= W=128"),
    (lambda L: _seg(L, wins=THIRDS + [(P, -1, 0)]), "window 9: y0=-1"),
    (lambda L: _seg(L, wins=THIRDS + [(P, 33, 0)]), "window 9: y0=33"),
    (lambda L: _seg(L, wins=THIRDS + [(P, 0, -4)]), "window 9: x0=-4"),
    (lambda L: _seg(L, wins=THIRDS + [(P, 0, 65)]), "window 9: x0=65"),
    (lambda L: _seg(L, wins=FULL, B=8, h=4, w=4, wh=16384, ww=16384, H=16384, W=16384), "B*H*W = 2147483648"),
    (lambda L: _seg(L, wins=GAP, wh=64, ww=64, W=134), "pixel (y=0, x=64) is covered by no window"),
    (lambda L: _seg(L, wins=THIRDS[:8]), "pixel (y=53, x=106) is covered by no window"),
    (lambda L: _seg(L, wins=[(P, 0, 0), (P, 0, 64), (P, 32, 64)]), "pixel (y=32, x=0) is covered by no window"),
    (lambda L: _seg(L, cm=None), "cm, loss_sum and count required"),
    (lambda L: _seg(L, labels=None), "must be null without labels"),
    (lambda L: _seg(L, labels=None, pred=None, cm=None, loss=None, count=None), "nothing to do"),
    (lambda L: _seg(L, ws=None), "ws="),
    (lambda L: _seg(L, ws=0x1004), "ws=0x1004"),
    (lambda L: _depth(L, nwin=0), "nwin=0"),
    (lambda L: _depth(L, wins=FULL * 65, wh=64, ww=128), "nwin=65"),
    (lambda L: _depth(L, low_dt=-1), "low_dt=-1"),
    (lambda L: _depth(L, wins=[(None, 0, 0)]), "window 0: low is null"),
    (lambda L: _depth(L, h=40), "h=40 <= wh=32"),
    (lambda L: _depth(L, ww=200), "ww=200 <= W=128"),
    (lambda L: _depth(L, wins=[(P, 40, 0)]), "window 0: y0=40"),
    (lambda L: _depth(L, wins=[(P, 0, 70)]), "window 0: x0=70"),
    (lambda L: _depth(L, wins=FULL, B=2, h=4, w=4, wh=32768, ww=32768, H=32768, W=32768), "B*H*W = 2147483648"),
    (lambda L: _depth(L, wins=GAP, wh=64, ww=64, W=134), "pixel (y=0, x=64) is covered by no window"),
    (lambda L: _depth(L, sums=None), "sums required"),
    (lambda L: _depth(L, ws=None), "ws="),
    (lambda L: _depth(L, ws=0x1004), "ws=0x1004"),
    (lambda L: _depth(L, target=None, up=None, sums=None, ws=None), "nothing to do"),
], ids=["seg_no_windows", "seg_65_windows", "K20", "seg_dtype", "label_dtype", "seg_null_low", "seg_h_gt_wh",
        "seg_wh_gt_H", "seg_w_gt_ww", "seg_ww_gt_W", "seg_y0_neg", "seg_y0_past", "seg_x0_neg", "seg_x0_past",
        "seg_2^31", "seg_gap", "seg_corner_missing", "seg_quadrant_missing", "null_cm", "cm_without_labels",
        "seg_nothing", "seg_null_ws", "seg_odd_ws", "depth_no_windows", "depth_65_windows", "depth_dtype",
        "depth_null_low", "depth_h_gt_wh", "depth_ww_gt_W", "depth_y0_past", "depth_x0_past", "depth_2^31",
        "depth_gap", "null_sums", "depth_null_ws", "depth_odd_ws", "depth_nothing"])
def test_host_checks_reject_before_any_launch(call, needle):
    """every pointer is null or 0x1000: a launch would fault, a host check returns -1 first"""
    L = N.load()
    assert call(L) == -1
    assert needle in L.dclip_last_error().decode(), L.dclip_last_error().decode()


def test_ws_bytes_is_a_function_of_its_arguments_alone():
    L = N.load()
    args = [(8, 19, 9), (1, 19, 1), (2, 1, 64), (8, 1, 3)]
    base = [L.dclip_slide_eval_ws_bytes(*a) for a in args]
    assert all(b > 0 and b % 8 == 0 for b in base)
    # no smaller than the single-view workspace: the folds are shared
    assert base[0] >= L.dclip_upsample_eval_ws_bytes(8, 19, 64, 128)
    for bad in ((0, 19, 4), (1, 19, 0), (1, 19, 65), (1, 0, 4)):
        assert L.dclip_slide_eval_ws_bytes(*bad) == 0, bad
    touched = []
    try:
        for opt in range(20):
            for value in (1, 2, 7):
                if L.dclip_set_option(opt, value) == 0:
                    touched.append(opt)
                    assert [L.dclip_slide_eval_ws_bytes(*a) for a in args] == base, (opt, value)
    finally:
        for opt in set(touched):
            L.dclip_set_option(opt, 0)


def _grid(ys, xs):
    return [(y, x) for y in ys for x in xs]


def test_slide_windows_places_the_windows_by_the_rule():
    from denseclip_vit_multimodal_amd.evaluate import slide_windows
    want = {
        "thirds": ((32, 64), _grid((0, 21, 32), (0, 42, 64))),
        "odd": ((20, 131), _grid((0, 13, 23), (0, 87, 170))),
        "straddle": ((24, 300), _grid((0,), (0, 228))),
        "narrow_tile": ((12, 68), _grid((0,), (0, 34, 68))),
        "small_image": ((20, 50), [(0, 0)]),
    }
    for case, (size, origins) in want.items():
        B, H, W, crop, stride, _ = S.CASES[case]
        assert slide_windows(H, W, crop, stride) == (size, origins), case
        assert S.windows(H, W, crop, stride) == (size, origins), case  # the tests' own restatement agrees
    for case, (B, H, W, crop, stride, _) in S.CASES.items():
        assert slide_windows(H, W, crop, stride) == S.windows(H, W, crop, stride), case
    # Cityscapes: 9 windows, up to 4 on a pixel
    assert slide_windows(1024, 2048, (512, 1024), (341, 683)) == ((512, 1024), _grid((0, 341, 512), (0, 683, 1024)))
    # the reference config's 640 / 426 on a 512 x 683 image: one row of windows 512 x 640
    assert slide_windows(512, 683, 640, 426) == ((512, 640), [(0, 0), (0, 43)])
    assert slide_windows(512, 683, (640, 640), [426, 426]) == ((512, 640), [(0, 0), (0, 43)])
    for bad in (dict(crop_size=0, stride=4), dict(crop_size=(8, -8), stride=4), dict(crop_size=8, stride=(4, 0)),
                dict(crop_size=8, stride=-1)):
        with pytest.raises(ValueError, match="positive"):
            slide_windows(64, 64, **bad)
    with pytest.raises(ValueError, match="positive"):
        slide_windows(0, 64, 8, 4)
    assert len(slide_windows(64, 64, 8, 8)[1]) == 64
    with pytest.raises(ValueError, match="72 windows"):
        slide_windows(64, 72, 8, 8)


def test_slide_ops_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    E = torch.ops.dclip_eval
    for name in ("slide_argmax", "slide_seg_update", "slide_depth", "slide_depth_update"):
        assert hasattr(E, name), name
    assert str(E.slide_seg_update.default._schema.returns[0].type) == "Optional[Tensor]"
    assert str(E.slide_depth_update.default._schema.returns[0].type) == "Optional[Tensor]"
    with FakeTensorMode():
        dev = "cuda"
        origins = [c for o in _grid((0, 21, 32), (0, 42, 64)) for c in o]
        lgs = [torch.empty(2, 19, 2, 4, device=dev, dtype=torch.bfloat16) for _ in range(9)]
        lab = torch.empty(2, 64, 128, device=dev, dtype=torch.uint8)
        cm = torch.empty(19, 19, device=dev, dtype=torch.int64)
        ce = torch.empty(2, device=dev, dtype=torch.float64)
        pm = E.slide_argmax(lgs, origins, 32, 64, 64, 128)
        assert pm.shape == (2, 64, 128) and pm.dtype == torch.uint8 and pm.device.type == "cuda"
        pm = E.slide_seg_update(lgs, origins, 32, 64, lab, 255, cm, ce, True)
        assert pm.shape == (2, 64, 128) and pm.dtype == torch.uint8
        assert E.slide_seg_update(lgs, origins, 32, 64, lab, 255, cm, ce, False) is None
        dps = [torch.empty(2, 1, 2, 4, device=dev, dtype=torch.float16) for _ in range(9)]
        up = E.slide_depth(dps, origins, 32, 64, 64, 128)
        assert up.shape == (2, 1, 64, 128) and up.dtype == torch.float32 and up.device.type == "cuda"
        tg = torch.empty(2, 64, 128, device=dev)
        sums = torch.empty(12, device=dev, dtype=torch.float64)
        up = E.slide_depth_update(dps, origins, 32, 64, tg, None, 1e-3, 80.0, True, 1e-6, sums, True)
        assert up.shape == (2, 1, 64, 128) and up.dtype == torch.float32
        assert E.slide_depth_update(dps, origins, 32, 64, tg, lab, 1e-3, 80.0, True, 1e-6, sums, False) is None


def test_cpu_tensors_are_refused():
    """no CPU kernel behind the ops, and the Python layer says so before it reaches them"""
    from denseclip_vit_multimodal_amd import _torch_ops
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    _torch_ops.load()
    E = torch.ops.dclip_eval
    lgs, dps = [torch.zeros(1, 19, 4, 8)], [torch.zeros(1, 1, 4, 8)]
    with pytest.raises(NotImplementedError):
        E.slide_argmax(lgs, [0, 0], 64, 128, 64, 128)
    with pytest.raises(NotImplementedError):
        E.slide_depth(dps, [0, 0], 64, 128, 64, 128)
    with pytest.raises(NotImplementedError):
        E.slide_seg_update(lgs, [0, 0], 64, 128, torch.zeros(1, 64, 128, dtype=torch.int64), 255,
                           torch.zeros(19, 19, dtype=torch.int64), torch.zeros(2, dtype=torch.float64), False)
    with pytest.raises(NotImplementedError):
        E.slide_depth_update(dps, [0, 0], 64, 128, torch.zeros(1, 64, 128), None, 1e-3, 80.0, True, 1e-6,
                             torch.zeros(12, dtype=torch.float64), False)
    ev = Evaluator(device="cpu")
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ev.update_windows(lgs, None, (64, 128), [(0, 0)], seg_target=torch.zeros(1, 64, 128, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ev.update_windows(None, dps, (64, 128), [(0, 0)], depth_target=torch.zeros(1, 64, 128))


class _Cfg(torch.nn.Identity):
    def __init__(self, test_cfg):
        super().__init__()
        self.test_cfg = test_cfg


REFERENCE_TEST_CFG = dict(mode="slide", crop_size=(640, 640), stride=(426, 426))  # the reference's ViT configs


def test_validate_refuses_slide_with_tta_and_a_missing_test_cfg():
    from denseclip_vit_multimodal_amd.evaluate import validate
    with pytest.raises(ValueError, match="slide and tta"):
        validate(torch.nn.Identity(), [], slide=dict(crop_size=8, stride=4), tta=dict(flip=True))
    with pytest.raises(ValueError, match="slide and tta"):
        validate(_Cfg(REFERENCE_TEST_CFG), [], slide=True, tta={})
    with pytest.raises(ValueError, match="crop"):
        validate(torch.nn.Identity(), [], slide=dict(crop=8, stride=4))
    with pytest.raises(ValueError, match="crop_size and stride"):
        validate(torch.nn.Identity(), [], slide=dict(crop_size=8))
    with pytest.raises(ValueError, match="positive"):
        validate(torch.nn.Identity(), [], slide=dict(crop_size=8, stride=0))
    for cfg in (None, dict(mode="whole"), "slide", dict(crop_size=8, stride=4)):
        with pytest.raises(ValueError, match="test_cfg"):
            validate(_Cfg(cfg), [], slide=True)
    with pytest.raises(ValueError, match="test_cfg"):
        validate(torch.nn.Identity(), [], slide=True)  # no test_cfg attribute at all
    with pytest.raises(ValueError, match="crop_size and stride"):
        validate(_Cfg(dict(mode="slide", crop_size=8)), [], slide=True)
    # accepted: nothing to evaluate, the empty evaluator's metrics
    for slide in (True, dict(crop_size=(640, 640), stride=(426, 426))):
        out = validate(_Cfg(REFERENCE_TEST_CFG), [], slide=slide, device="cpu")
        assert int(out["confusion_matrix"].sum()) == 0


def test_slide_from_test_cfg_round_trips_the_reference_config():
    from denseclip_vit_multimodal_amd.evaluate import slide_from_test_cfg, slide_windows
    kw = slide_from_test_cfg(REFERENCE_TEST_CFG)
    assert kw == dict(crop_size=(640, 640), stride=(426, 426))
    assert slide_windows(512, 683, **kw) == ((512, 640), [(0, 0), (0, 43)])
    for cfg in (None, dict(mode="whole"), dict(), "slide"):
        assert slide_from_test_cfg(cfg) is None
    # the model keeps what it was given; config.model_kwargs goes on dropping it
    from denseclip_vit_multimodal_amd import config
    assert "test_cfg" not in config.model_kwargs(dict(model=dict(type="DenseCLIP", test_cfg=REFERENCE_TEST_CFG)))


def test_alias_package_reexports_the_new_names():
    import inspect
    import denseclip.evaluate as ev
    from denseclip_vit_multimodal_amd import evaluate
    assert ev is evaluate
    for name in ("slide_windows", "forward_windows", "predict_slide", "slide_from_test_cfg"):
        assert hasattr(ev, name), name
    assert hasattr(ev.Evaluator, "update_windows")
    sig = inspect.signature(ev.validate)
    assert sig.parameters["slide"].default is None and sig.parameters["tta"].default is None
    assert list(inspect.signature(ev.forward_windows).parameters) == ["model", "img", "crop_size", "stride",
                                                                     "windows_per_forward"]
