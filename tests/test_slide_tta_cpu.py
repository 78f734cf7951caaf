"""CPU checks of sliding windows under multi-scale + flip ensembling (csrc/headslidetta.hip,
torch.ops.dclip_eval.slide_tta_*, evaluate.py): the three new entry points are declared, bound and
exported beside an unchanged ABI version; their host checks reject bad arguments before any launch
with a message that names the value, a view's uncovered pixel included; the workspace size is a
function of its arguments alone; view_windows places the windows of every view by the rule; the four
ops are registered with fake implementations and refuse CPU tensors; validate refuses slide_tta with
slide or tta, unknown keys and True without a slide test_cfg; the alias package re-exports the names."""
import ctypes
import os
import re

import pytest
import torch

import slide_ref as S
import slide_tta_ref as T
from helpers import ROOT
from denseclip_vit_multimodal_amd import _native as N

NEW = ["dclip_slide_tta_eval_depth", "dclip_slide_tta_eval_seg", "dclip_slide_tta_eval_ws_bytes"]
P = 0x1000  # a non-null pointer the host checks never dereference


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", src, re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert lib.dclip_slide_tta_eval_ws_bytes.restype is ctypes.c_int64
    assert int(re.search(r"#define DCLIP_SLIDE_TTA_MAX_WINDOWS (\d+)", src).group(1)) == 1024
    assert N.SLIDE_TTA_MAX_WINDOWS == 1024
    assert "dclip_slide_view" in src
    # dclip_slide_view as C lays it out: nine ints
    assert ctypes.sizeof(N.SlideView) == 36 and N.SlideView.first.offset == 28 and N.SlideView.nwin.offset == 32
    v = N.slide_view_table([(64, 128, 1, 32, 64, 2, 4, 0, 9)])[0]
    assert (v.Hv, v.Wv, v.flip, v.wh, v.ww, v.h, v.w, v.first, v.nwin) == (64, 128, 1, 32, 64, 2, 4, 0, 9)


# slide_ref's `thirds` geometry as a view: 64 x 128, windows 32 x 64 from 2 x 4 maps
THIRDS = [(P, y, x) for y in (0, 21, 32) for x in (0, 42, 64)]
V0 = dict(Hv=64, Wv=128, flip=0, wh=32, ww=64, h=2, w=4, first=0, nwin=9)
FIELDS = ("Hv", "Wv", "flip", "wh", "ww", "h", "w", "first", "nwin")


def _views(*vs):
    return [tuple(dict(V0, **v)[k] for k in FIELDS) for v in vs]


def _seg(L, views=None, wins=THIRDS, nviews=None, nwin_total=None, K=19, B=1, average=1, H=64, W=128, labels=P, pred=P,
         cm=P, loss=P, count=P, ws=P, low_dt=0, lab_dt=0):
    views = _views({}) if views is None else views
    vt = N.slide_view_table(views) if views else None
    tab = N.window_table(wins) if wins else None
    return L.dclip_slide_tta_eval_seg(low_dt, vt, len(views) if nviews is None else nviews, tab,
                                      len(wins) if nwin_total is None else nwin_total, B, K, average, labels, lab_dt, H,
                                      W, 255, pred, cm, loss, count, ws, None)


def _depth(L, views=None, wins=THIRDS, nviews=None, nwin_total=None, B=1, H=64, W=128, target=P, up=None, sums=P, ws=P,
           low_dt=0):
    views = _views({}) if views is None else views
    vt = N.slide_view_table(views) if views else None
    tab = N.window_table(wins) if wins else None
    return L.dclip_slide_tta_eval_depth(low_dt, vt, len(views) if nviews is None else nviews, tab,
                                        len(wins) if nwin_total is None else nwin_total, B, target, None, H, W, 1e-3,
                                        80.0, 1, 1e-6, up, sums, ws, None)


FULL = dict(wh=64, ww=128, nwin=1)  # one window over the whole 64 x 128 view
GAP = [(P, 0, 0), (P, 0, 70)]  # 64 x 64 windows on a 64 x 134 view: columns 64 .. 69 uncovered
TWO = _views({}, dict(flip=1, first=9))  # two views of nine windows each


@pytest.mark.parametrize("call,needle", [
    (lambda L: _seg(L, K=20), "K=20"),
    (lambda L: _seg(L, average=2), "average=2"),
    (lambda L: _seg(L, nviews=0), "nviews=0"),
    (lambda L: _seg(L, views=_views(FULL) * 17, wins=[(P, 0, 0)]), "nviews=17"),
    (lambda L: _seg(L, nwin_total=0), "nwin_total=0"),
    (lambda L: _seg(L, views=_views(FULL), wins=[(P, 0, 0)] * 1025), "nwin_total=1025"),
    (lambda L: _seg(L, low_dt=5), "low_dt=5"),
    (lambda L: _seg(L, lab_dt=3), "lab_dt=3"),
    (lambda L: _seg(L, views=_views(dict(flip=2))), "view 0: flip=2"),
    (lambda L: _seg(L, views=_views(dict(h=33))), "view 0: h=33 <= wh=32"),
    (lambda L: _seg(L, views=_views(dict(wh=65))), "wh=65 <= Hv=64"),
    (lambda L: _seg(L, views=_views(dict(w=65))), "w=65 <= ww=64"),
    (lambda L: _seg(L, views=_views(dict(ww=129))), "ww=129 <= Wv=128"),
    (lambda L: _seg(L, views=_views(dict(nwin=10))), "view 0: windows [0, 0 + 10) outside the table of 9"),
    (lambda L: _seg(L, views=_views({}, dict(first=5, nwin=5)), wins=THIRDS), "view 1: windows [5, 5 + 5)"),
    (lambda L: _seg(L, views=_views(dict(nwin=0))), "view 0: windows [0, 0 + 0)"),
    (lambda L: _seg(L, views=TWO, wins=THIRDS + THIRDS[:4] + [(None, 21, 42)] + THIRDS[5:]),
     "view 1: window 13: low is null"),
    (lambda L: _seg(L, views=_views(dict(nwin=10)), wins=THIRDS + [(P, -1, 0)]), "window 9: y0=-1"),
    (lambda L: _seg(L, views=_views(dict(nwin=10)), wins=THIRDS + [(P, 33, 0)]), "window 9: y0=33"),
    (lambda L: _seg(L, views=_views(dict(nwin=10)), wins=THIRDS + [(P, 0, -4)]), "window 9: x0=-4"),
    (lambda L: _seg(L, views=_views(dict(nwin=10)), wins=THIRDS + [(P, 0, 65)]), "window 9: x0=65"),
    (lambda L: _seg(L, views=_views(dict(Hv=16384, Wv=16384, wh=16384, ww=16384, h=4, w=4, nwin=1)), wins=[(P, 0, 0)],
                    B=8, H=16384, W=16384), "B*H*W = 2147483648"),
    (lambda L: _seg(L, views=_views(dict(Hv=32768, Wv=32768, wh=64, ww=64, nwin=1)), wins=[(P, 0, 0)], B=2),
     "view 0: B*Hv*Wv = 2147483648"),
    (lambda L: _seg(L, views=_views(dict(Wv=134, wh=64, ww=64, nwin=2)), wins=GAP),
     "view 0: pixel (y=0, x=64) is covered by no window"),
    (lambda L: _seg(L, views=_views({}, dict(first=9, nwin=8)), wins=THIRDS + THIRDS[:8]),
     "view 1: pixel (y=53, x=106) is covered by no window"),
    (lambda L: _seg(L, views=_views(dict(nwin=3)), wins=[(P, 0, 0), (P, 0, 64), (P, 32, 64)]),
     "pixel (y=32, x=0) is covered by no window"),
    (lambda L: _seg(L, cm=None), "cm, loss_sum and count required"),
    (lambda L: _seg(L, labels=None), "must be null without labels"),
    (lambda L: _seg(L, labels=None, pred=None, cm=None, loss=None, count=None), "nothing to do"),
    (lambda L: _seg(L, ws=None), "ws="),
    (lambda L: _seg(L, ws=0x1004), "ws=0x1004"),
    (lambda L: _seg(L, labels=None, cm=None, loss=None, count=None, ws=None), "it holds the window table"),
    (lambda L: _depth(L, nviews=0), "nviews=0"),
    (lambda L: _depth(L, views=_views(FULL), wins=[(P, 0, 0)] * 1025), "nwin_total=1025"),
    (lambda L: _depth(L, low_dt=-1), "low_dt=-1"),
    (lambda L: _depth(L, views=_views(FULL), wins=[(None, 0, 0)]), "window 0: low is null"),
    (lambda L: _depth(L, views=_views(dict(h=40))), "h=40 <= wh=32"),
    (lambda L: _depth(L, views=_views(dict(ww=200))), "ww=200 <= Wv=128"),
    (lambda L: _depth(L, views=_views(dict(nwin=1)), wins=[(P, 40, 0)]), "window 0: y0=40"),
    (lambda L: _depth(L, views=_views(dict(nwin=1)), wins=[(P, 0, 70)]), "window 0: x0=70"),
    (lambda L: _depth(L, views=_views(dict(Hv=32768, Wv=32768, wh=32768, ww=32768, h=4, w=4, nwin=1)),
                      wins=[(P, 0, 0)], B=2, H=32768, W=32768), "B*H*W = 2147483648"),
    (lambda L: _depth(L, views=_views(dict(Hv=32768, Wv=32768, wh=64, ww=64, nwin=1)), wins=[(P, 0, 0)], B=2),
     "B*Hv*Wv = 2147483648"),
    (lambda L: _depth(L, views=_views(dict(Wv=134, wh=64, ww=64, nwin=2)), wins=GAP),
     "view 0: pixel (y=0, x=64) is covered by no window"),
    (lambda L: _depth(L, sums=None), "sums required"),
    (lambda L: _depth(L, ws=None), "ws="),
    (lambda L: _depth(L, ws=0x1004), "ws=0x1004"),
    (lambda L: _depth(L, target=None, up=None, sums=None), "nothing to do"),
], ids=["K20", "average", "seg_no_views", "seg_17_views", "seg_no_windows", "seg_1025_windows", "seg_dtype",
        "label_dtype", "seg_flip", "seg_h_gt_wh", "seg_wh_gt_Hv", "seg_w_gt_ww", "seg_ww_gt_Wv", "seg_slice_past",
        "seg_slice_past_view1", "seg_empty_view", "seg_null_low", "seg_y0_neg", "seg_y0_past", "seg_x0_neg",
        "seg_x0_past", "seg_2^31", "seg_view_2^31", "seg_gap", "seg_corner_missing_view1", "seg_quadrant_missing",
        "null_cm", "cm_without_labels", "seg_nothing", "seg_null_ws", "seg_odd_ws", "seg_pred_only_null_ws",
        "depth_no_views", "depth_1025_windows", "depth_dtype", "depth_null_low", "depth_h_gt_wh", "depth_ww_gt_Wv",
        "depth_y0_past", "depth_x0_past", "depth_2^31", "depth_view_2^31", "depth_gap", "null_sums", "depth_null_ws",
        "depth_odd_ws", "depth_nothing"])
def test_host_checks_reject_before_any_launch(call, needle):
    """every pointer is null or 0x1000: a launch would fault, a host check returns -1 first"""
    L = N.load()
    assert call(L) == -1
    assert needle in L.dclip_last_error().decode(), L.dclip_last_error().decode()


def test_ws_bytes_is_a_function_of_its_arguments_alone():
    L = N.load()
    args = [(1, 19, 12, 196), (2, 19, 4, 47), (1, 1, 8, 440), (8, 1, 1, 1), (1, 19, 16, 1024)]
    base = [L.dclip_slide_tta_eval_ws_bytes(*a) for a in args]
    assert all(b > 0 and b % 8 == 0 for b in base)
    # the sibling's records plus the table: 16 bytes a window
    assert base[0] == L.dclip_slide_eval_ws_bytes(1, 19, 9) + 196 * ctypes.sizeof(N.Window)
    assert base[2] == L.dclip_slide_eval_ws_bytes(1, 1, 9) + 440 * ctypes.sizeof(N.Window)
    for bad in ((0, 19, 4, 4), (1, 0, 4, 4), (1, 19, 0, 4), (1, 19, 17, 4), (1, 19, 4, 0), (1, 19, 4, 1025)):
        assert L.dclip_slide_tta_eval_ws_bytes(*bad) == 0, bad
    touched = []
    try:
        for opt in range(20):
            for value in (1, 2, 7):
                if L.dclip_set_option(opt, value) == 0:
                    touched.append(opt)
                    assert [L.dclip_slide_tta_eval_ws_bytes(*a) for a in args] == base, (opt, value)
    finally:
        for opt in set(touched):
            L.dclip_set_option(opt, 0)


def _rule(H, W, crop, stride, scales, flip):
    """mmseg's aug_test over slide_inference, restated: per ratio the view's size, slide_ref's windows"""
    out = []
    for s in scales:
        Hv, Wv = int(H * s + 0.5), int(W * s + 0.5)
        size, origins = S.windows(Hv, Wv, crop, stride)
        for f in ((False, True) if flip else (False,)):
            out.append((Hv, Wv, f, size, origins))
    return out


def test_view_windows_places_the_windows_by_the_rule():
    from denseclip_vit_multimodal_amd.evaluate import TTA_SCALES, view_windows
    # the reference geometry: 2 + 8 + 10 + 18 + 28 + 32 = 98 windows per flip state
    ref = view_windows(1024, 2048, (640, 640), (426, 426))
    assert ref == _rule(1024, 2048, (640, 640), (426, 426), TTA_SCALES, True)
    assert [(v[0], v[1], v[2]) for v in ref] == [(int(1024 * s + 0.5), int(2048 * s + 0.5), f)
                                                 for s in TTA_SCALES for f in (False, True)]
    assert [len(v[4]) for v in ref[0::2]] == [2, 8, 10, 18, 28, 32] and sum(len(v[4]) for v in ref) == 196
    assert ref[0][3] == (512, 640) and ref[0][4] == [(0, 0), (0, 384)]  # the x0.5 view is lower than the crop
    assert all(v[3] == (640, 640) for v in ref[2:])
    assert view_windows(1024, 2048, 640, 426) == ref  # ints as pairs
    assert view_windows(1024, 2048, 640, 426, flip=False) == ref[0::2]
    # the tests' cases: the views of a case at ratio Hv / H
    for case, (B, H, W, crop, stride, vs, p) in T.CASES.items():
        views = T.geometry(case)[3]
        assert sum(len(v[4]) for v in views) == T.N_WINDOWS[case], case
        for (Hv, Wv, flip, size, origins, hw) in views:
            got = view_windows(Hv, Wv, crop, stride, scales=(1.0,), flip=False)
            assert got == [(Hv, Wv, False, size, origins)], case
    assert view_windows(64, 128, (40, 40), (27, 27), scales=(0.5, 1.0, 1.75)) == \
        [(Hv, Wv, bool(f), size, origins) for Hv, Wv, f, size, origins, hw in T.geometry("city16")[3]]
    with pytest.raises(ValueError, match="positive"):
        view_windows(64, 128, 0, 4)
    with pytest.raises(ValueError, match="views"):
        view_windows(64, 128, 40, 27, scales=(1.0,) * 9)
    with pytest.raises(ValueError, match="1152 windows"):
        view_windows(64, 72, 8, 8, scales=(1.0,) * 8)  # 8 x 2 views of 72 windows


def test_slide_tta_ops_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    E = torch.ops.dclip_eval
    for name in ("slide_tta_argmax", "slide_tta_seg_update", "slide_tta_depth", "slide_tta_depth_update"):
        assert hasattr(E, name), name
    assert str(E.slide_tta_seg_update.default._schema.returns[0].type) == "Optional[Tensor]"
    assert str(E.slide_tta_depth_update.default._schema.returns[0].type) == "Optional[Tensor]"
    with FakeTensorMode():
        dev = "cuda"
        origins = [c for y in (0, 21, 32) for x in (0, 42, 64) for c in (y, x)] + [0, 0]
        views = [64, 128, 0, 32, 64, 9, 32, 64, 1, 32, 64, 1]
        lgs = [torch.empty(2, 19, 2, 4, device=dev, dtype=torch.bfloat16) for _ in range(9)] + \
              [torch.empty(2, 19, 4, 8, device=dev, dtype=torch.bfloat16)]
        lab = torch.empty(2, 64, 128, device=dev, dtype=torch.uint8)
        cm = torch.empty(19, 19, device=dev, dtype=torch.int64)
        ce = torch.empty(2, device=dev, dtype=torch.float64)
        pm = E.slide_tta_argmax(lgs, views, origins, 64, 128, True)
        assert pm.shape == (2, 64, 128) and pm.dtype == torch.uint8 and pm.device.type == "cuda"
        pm = E.slide_tta_seg_update(lgs, views, origins, lab, 255, True, cm, ce, True)
        assert pm.shape == (2, 64, 128) and pm.dtype == torch.uint8
        assert E.slide_tta_seg_update(lgs, views, origins, lab, 255, False, cm, ce, False) is None
        dps = [torch.empty(2, 1, 2, 4, device=dev, dtype=torch.float16) for _ in range(9)] + \
              [torch.empty(2, 1, 4, 8, device=dev, dtype=torch.float16)]
        up = E.slide_tta_depth(dps, views, origins, 64, 128)
        assert up.shape == (2, 1, 64, 128) and up.dtype == torch.float32 and up.device.type == "cuda"
        tg = torch.empty(2, 64, 128, device=dev)
        sums = torch.empty(12, device=dev, dtype=torch.float64)
        up = E.slide_tta_depth_update(dps, views, origins, tg, None, 1e-3, 80.0, True, 1e-6, sums, True)
        assert up.shape == (2, 1, 64, 128) and up.dtype == torch.float32
        assert E.slide_tta_depth_update(dps, views, origins, tg, lab, 1e-3, 80.0, True, 1e-6, sums, False) is None


def test_cpu_tensors_are_refused():
    """no CPU kernel behind the ops, and the Python layer says so before it reaches them"""
    from denseclip_vit_multimodal_amd import _torch_ops
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    _torch_ops.load()
    E = torch.ops.dclip_eval
    lgs, dps = [torch.zeros(1, 19, 4, 8)], [torch.zeros(1, 1, 4, 8)]
    views, origins = [64, 128, 0, 64, 128, 1], [0, 0]
    with pytest.raises(NotImplementedError):
        E.slide_tta_argmax(lgs, views, origins, 64, 128, True)
    with pytest.raises(NotImplementedError):
        E.slide_tta_depth(dps, views, origins, 64, 128)
    with pytest.raises(NotImplementedError):
        E.slide_tta_seg_update(lgs, views, origins, torch.zeros(1, 64, 128, dtype=torch.int64), 255, True,
                               torch.zeros(19, 19, dtype=torch.int64), torch.zeros(2, dtype=torch.float64), False)
    with pytest.raises(NotImplementedError):
        E.slide_tta_depth_update(dps, views, origins, torch.zeros(1, 64, 128), None, 1e-3, 80.0, True, 1e-6,
                                 torch.zeros(12, dtype=torch.float64), False)
    ev = Evaluator(device="cpu")
    v = [(64, 128, 0, 64, 128, 1)]
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ev.update_view_windows(lgs, None, v, [(0, 0)], seg_target=torch.zeros(1, 64, 128, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ev.update_view_windows(None, dps, v, [(0, 0)], depth_target=torch.zeros(1, 64, 128))
    with pytest.raises(ValueError, match="average"):
        ev.update_view_windows(lgs, None, v, [(0, 0)], average="mean")


class _Cfg(torch.nn.Identity):
    def __init__(self, test_cfg):
        super().__init__()
        self.test_cfg = test_cfg


REFERENCE_TEST_CFG = dict(mode="slide", crop_size=(640, 640), stride=(426, 426))  # the reference's ViT configs


def test_validate_refuses_slide_tta_with_slide_or_tta_unknown_keys_and_a_missing_test_cfg():
    from denseclip_vit_multimodal_amd.evaluate import validate
    st = dict(crop_size=8, stride=4)
    with pytest.raises(ValueError, match="slide_tta .* does not combine with slide or tta"):
        validate(torch.nn.Identity(), [], slide_tta=st, slide=st)
    with pytest.raises(ValueError, match="does not combine with slide or tta"):
        validate(torch.nn.Identity(), [], slide_tta=st, tta=dict(flip=True))
    with pytest.raises(ValueError, match="does not combine with slide or tta"):
        validate(_Cfg(REFERENCE_TEST_CFG), [], slide_tta=True, slide=True)
    # slide with tta goes on raising what it raised, now naming the way out
    with pytest.raises(ValueError, match="slide and tta do not combine .*slide_tta"):
        validate(torch.nn.Identity(), [], slide=st, tta=dict(flip=True))
    with pytest.raises(ValueError, match=r"unknown slide_tta keys \['crop', 'scale'\]"):
        validate(torch.nn.Identity(), [], slide_tta=dict(crop=8, stride=4, scale=(1.0,)))
    with pytest.raises(ValueError, match="crop_size and stride"):
        validate(torch.nn.Identity(), [], slide_tta=dict(crop_size=8))
    with pytest.raises(ValueError, match="positive"):
        validate(torch.nn.Identity(), [], slide_tta=dict(crop_size=8, stride=0))
    with pytest.raises(ValueError, match="average"):
        validate(torch.nn.Identity(), [], slide_tta=dict(st, average="mean"))
    for cfg in (None, dict(mode="whole"), "slide", dict(crop_size=8, stride=4)):
        with pytest.raises(ValueError, match="test_cfg"):
            validate(_Cfg(cfg), [], slide_tta=True)
    with pytest.raises(ValueError, match="test_cfg"):
        validate(torch.nn.Identity(), [], slide_tta=True)  # no test_cfg attribute at all
    # accepted: nothing to evaluate, the empty evaluator's metrics
    for slide_tta in (True, dict(crop_size=(640, 640), stride=(426, 426), scales=(0.5, 1.0), flip=False,
                                 average="logits", windows_per_forward=4)):
        out = validate(_Cfg(REFERENCE_TEST_CFG), [], slide_tta=slide_tta, device="cpu")
        assert int(out["confusion_matrix"].sum()) == 0
    assert int(validate(torch.nn.Identity(), [], slide_tta=False, slide=False, device="cpu")["confusion_matrix"].sum()) == 0


def test_alias_package_reexports_the_new_names():
    import inspect
    import denseclip.evaluate as ev
    from denseclip_vit_multimodal_amd import evaluate
    assert ev is evaluate
    for name in ("view_windows", "forward_view_windows", "predict_slide_tta"):
        assert hasattr(ev, name), name
    assert hasattr(ev.Evaluator, "update_view_windows")
    sig = inspect.signature(ev.validate)
    assert sig.parameters["slide_tta"].default is None
    assert list(sig.parameters)[:5] == ["model", "batches", "evaluator", "tta", "slide"]
    assert list(inspect.signature(ev.forward_view_windows).parameters) == [
        "model", "img", "crop_size", "stride", "scales", "flip", "windows_per_forward"]
    assert inspect.signature(ev.predict_slide_tta).parameters["average"].default == "probs"
    assert list(inspect.signature(ev.view_windows).parameters) == ["H", "W", "crop_size", "stride", "scales", "flip"]
    assert "slide_tta" in evaluate.__doc__ and "headslidetta.hip" in evaluate.__doc__
