"""CPU checks of the any-class-count paths (csrc/classes.hip, torch.ops.dclip_classes / dclip_eval,
ops.py and evaluate.py's dispatch): the new entry points are declared, bound and exported; their host
checks reject bad arguments before any launch; the workspace sizes depend on the arguments alone and
respect their caps; the ops have fake implementations and refuse CPU tensors; K = 19 keeps today's
ops and any other K <= 256 takes the new ones.

REF_FP32_DEPARTURE_CE: the departure of torch's own fp32 evaluation (F.interpolate fp32 ->
F.cross_entropy fp32, sum) from the fp64 evaluation of the same values, relative, maximised over the
cases of test_gpu_classes.py (K in 2, 33, 150, 256; classes_ref.SHAPES; bf16 / f16 / f32 logits; int64
/ uint8 labels).  Recorded from `python tests/classes_ref.py` (8 threads), which printed 2.4034e-07 (the worst case: K = 33).  The GPU test
allows the kernel 4x this figure."""
import ctypes
import os
import re

import pytest
import torch

import classes_ref as R
from helpers import ROOT
from denseclip_vit_multimodal_amd import _native as N

REF_FP32_DEPARTURE_CE = 2.4034e-7
NEW = ["dclip_score_map_classes", "dclip_upsample_ce_classes", "dclip_upsample_ce_classes_ws_floats",
       "dclip_upsample_eval_seg_classes", "dclip_upsample_eval_seg_classes_ws_bytes"]
P = ctypes.c_void_p(0x1000)  # a non-null pointer the host checks never dereference
MIB = 1 << 20


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", f.read(), re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert lib.dclip_upsample_ce_classes_ws_floats.restype is ctypes.c_int64
    assert lib.dclip_upsample_eval_seg_classes_ws_bytes.restype is ctypes.c_int64


def _seg(L, K=150, B=1, h=4, w=8, H=64, W=128, logits=P, labels=P, pred=P, cm=P, loss=P, count=P, ws=P, low_dt=0,
         lab_dt=0):
    return L.dclip_upsample_eval_seg_classes(low_dt, logits, B, K, h, w, labels, lab_dt, H, W, 255, pred, cm, loss,
                                             count, ws, None)


def _ce(L, K=150, B=1, h=4, w=8, H=64, W=128, logits=P, labels=P, loss=P, count=P, grad=P, ws=P, low_dt=0, lab_dt=0):
    return L.dclip_upsample_ce_classes(low_dt, logits, B, K, h, w, labels, lab_dt, H, W, 255, loss, count, grad, ws,
                                       None)


def _score(L, K=150, v=P, t=P, score=P, v_dt=2, C=512, B=1, HW=64):
    return L.dclip_score_map_classes(v, v_dt, HW * C, 0, C, t, score, B, HW, C, K, 1e-12, None)


@pytest.mark.parametrize("call,needle", [
    (lambda L: _seg(L, K=0), "K=0"),
    (lambda L: _seg(L, K=257), "K=257"),
    (lambda L: _seg(L, low_dt=5), "low_dt=5"),
    (lambda L: _seg(L, lab_dt=3), "lab_dt=3"),
    (lambda L: _seg(L, H=3), "smaller than the input"),
    (lambda L: _seg(L, B=8, H=16384, W=16384), "below 2^31"),
    (lambda L: _seg(L, logits=None), "logits required"),
    (lambda L: _seg(L, cm=None), "cm, loss_sum and count required"),
    (lambda L: _seg(L, labels=None), "must be null without labels"),
    (lambda L: _seg(L, labels=None, pred=None, cm=None, loss=None, count=None), "nothing to do"),
    (lambda L: _seg(L, ws=None), "ws"),
    (lambda L: _seg(L, ws=ctypes.c_void_p(0x1004)), "ws"),
    (lambda L: _ce(L, K=0), "K=0"),
    (lambda L: _ce(L, K=257), "K=257"),
    (lambda L: _ce(L, low_dt=7), "low_dt=7"),
    (lambda L: _ce(L, lab_dt=-1), "lab_dt=-1"),
    (lambda L: _ce(L, h=0), "bad sizes"),
    (lambda L: _ce(L, grad=None), "outputs required"),
    (lambda L: _ce(L, loss=None), "outputs required"),
    (lambda L: _ce(L, count=None), "outputs required"),
    (lambda L: _ce(L, labels=None), "logits and labels required"),
    (lambda L: _ce(L, ws=None), "ws"),
    (lambda L: _ce(L, ws=ctypes.c_void_p(0x1004)), "ws"),
    (lambda L: _score(L, K=0), "K=0"),
    (lambda L: _score(L, K=257), "K=257"),
    (lambda L: _score(L, v_dt=0), "f16/bf16"),
    (lambda L: _score(L, C=520), "C % 16"),
    (lambda L: _score(L, score=None), "score required"),
], ids=["seg_K0", "seg_K257", "seg_dtype", "seg_label_dtype", "seg_H_lt_h", "seg_2^31", "seg_null_logits", "seg_null_cm",
        "seg_cm_without_labels", "seg_nothing", "seg_null_ws", "seg_misaligned_ws", "ce_K0", "ce_K257", "ce_dtype",
        "ce_label_dtype", "ce_sizes", "ce_null_grad", "ce_null_loss", "ce_null_count", "ce_null_labels", "ce_null_ws",
        "ce_misaligned_ws", "score_K0", "score_K257", "score_dtype", "score_C", "score_null_out"])
def test_host_checks_reject_before_any_launch(call, needle):
    L = N.load()
    assert call(L) == -1
    assert needle in L.dclip_last_error().decode()


def test_existing_entry_points_still_refuse_other_class_counts():
    L = N.load()
    assert L.dclip_upsample_eval_seg(0, P, 1, 150, 4, 8, P, 0, 64, 128, 255, P, P, P, P, P, None) == -1
    assert L.dclip_upsample_ce(0, P, 1, 150, 4, 8, P, 0, 64, 128, 255, P, P, P, P, None) == -1
    assert L.dclip_score_map(P, 2, 0, 0, 512, P, P, 1, 4, 512, 40, 1e-12, None) == -1


def test_workspaces_depend_on_the_arguments_alone_and_respect_their_caps():
    L = N.load()
    ce, ev = L.dclip_upsample_ce_classes_ws_floats, L.dclip_upsample_eval_seg_classes_ws_bytes
    args = [(8, 150, 64, 128), (8, 256, 64, 128), (1, 2, 1, 1), (2, 33, 5, 37), (8, 256, 64, 40), (1, 150, 11, 66)]
    base = [(ce(*a), ev(*a)) for a in args]
    for (B, K, h, w), (f, b) in zip(args, base):
        assert f > 0 and b > 0 and b % 8 == 0 and (f * 4) % 8 == 0
        assert f * 4 <= 3 * B * K * h * w * 4 + MIB, (B, K, h, w, f)
        assert b <= 80 * MIB, (B, K, h, w, b)
    for bad in [(0, 150, 4, 4), (1, 0, 4, 4), (1, 257, 4, 4), (1, 150, 0, 4), (1, 150, 4, 0)]:
        assert ce(*bad) == 0 and ev(*bad) == 0
    touched = []
    try:
        for opt in range(20):
            for value in (1, 2, 7):
                if L.dclip_set_option(opt, value) == 0:
                    touched.append(opt)
                    assert [(ce(*a), ev(*a)) for a in args] == base, (opt, value)
    finally:
        for opt in set(touched):
            L.dclip_set_option(opt, 0)


@pytest.fixture(scope="module")
def loaded():
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    return torch.ops


def test_ops_registered_with_fakes(loaded):
    from torch._subclasses.fake_tensor import FakeTensorMode
    E, C = loaded.dclip_eval, loaded.dclip_classes
    assert str(E.seg_update_classes.default._schema.returns[0].type) == "Optional[Tensor]"
    K = 150
    with FakeTensorMode():
        dev = "cuda"
        lg = torch.empty(2, K, 8, 16, device=dev, dtype=torch.bfloat16)
        lab = torch.empty(2, 128, 256, device=dev, dtype=torch.uint8)
        cm = torch.empty(K, K, device=dev, dtype=torch.int64)
        ce = torch.empty(2, device=dev, dtype=torch.float64)
        ws = torch.empty(1 << 22, device=dev, dtype=torch.uint8)
        pm = E.upsample_argmax_classes(lg, 128, 256)
        assert pm.shape == (2, 128, 256) and pm.dtype == torch.uint8 and pm.device.type == "cuda"
        pm = E.seg_update_classes(lg, lab, 255, cm, ce, True, ws)
        assert pm.shape == (2, 128, 256) and pm.dtype == torch.uint8
        assert E.seg_update_classes(lg, lab, 255, cm, ce, False) is None
        s, n, g = C.upsample_ce(lg, lab, 255)
        assert s.shape == (1,) and s.dtype == torch.float64 and n.dtype == torch.int32
        assert g.shape == lg.shape and g.dtype == torch.float32
        v = torch.empty(2 * 40, 512, device=dev, dtype=torch.float16)
        sc = C.score_map(v, 40 * 512, 0, 512, torch.empty(2, K, 512, device=dev), 2, 40, 1e-12)
        assert sc.shape == (2, K, 40) and sc.dtype == torch.float32
    L = N.load()
    assert E.seg_classes_ws_bytes(2, K, 8, 16) == L.dclip_upsample_eval_seg_classes_ws_bytes(2, K, 8, 16)


def test_cpu_tensors_are_refused(loaded):
    E, C = loaded.dclip_eval, loaded.dclip_classes
    lg, lab = torch.randn(1, 150, 4, 4), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="CPU"):
        E.upsample_argmax_classes(lg, 8, 8)
    with pytest.raises(NotImplementedError, match="CPU"):
        E.seg_update_classes(lg, lab, 255, torch.zeros(150, 150, dtype=torch.int64), torch.zeros(2, dtype=torch.float64),
                             False)
    with pytest.raises(NotImplementedError, match="CPU"):
        C.upsample_ce(lg, lab, 255)
    with pytest.raises(NotImplementedError, match="CPU"):
        C.score_map(torch.randn(16, 64).half(), 16 * 64, 0, 64, torch.randn(1, 150, 64), 1, 16, 1e-12)


class _Table:
    """stands in for an op namespace: records which op was asked for, then stops the call"""

    def __init__(self):
        self.asked = []

    def __getattr__(self, name):
        def op(*a, **k):
            self.asked.append(name)
            raise _Asked(name)
        return op


class _Asked(Exception):
    pass


def test_python_dispatch_by_class_count(monkeypatch):
    from denseclip_vit_multimodal_amd import evaluate, ops
    old, new, ev = _Table(), _Table(), _Table()
    monkeypatch.setattr(ops, "D", lambda: old)
    monkeypatch.setattr(ops, "DC", lambda: new)
    monkeypatch.setattr(ops, "_check", lambda *a, **k: None)
    monkeypatch.setattr(evaluate, "_E", lambda: ev)
    monkeypatch.setattr(evaluate, "_need_gpu", lambda *a: None)
    lab = torch.zeros(1, 8, 8, dtype=torch.int64)
    for K, table, name in ((19, old, "upsample_ce"), (150, new, "upsample_ce"), (2, new, "upsample_ce"),
                           (256, new, "upsample_ce")):
        before = ops.STATS.get("upsample_ce_classes", 0)
        with pytest.raises(_Asked):
            ops.UpsampleCEFn.apply(torch.zeros(1, K, 2, 2), lab, 255)
        assert table.asked[-1] == name
        assert ops.STATS.get("upsample_ce_classes", 0) == before + (table is new)
    with pytest.raises(ValueError, match="256"):
        ops.UpsampleCEFn.apply(torch.zeros(1, 300, 2, 2), lab, 255)
    n_old, n_new = len(old.asked), len(new.asked)
    for K, table in ((19, old), (32, old), (33, new), (150, new), (256, new)):
        with pytest.raises(_Asked):
            ops.score_map(torch.zeros(16, 64, dtype=torch.float16), torch.zeros(1, K, 64), 1, 16)
        assert table.asked[-1] == "score_map"
    assert len(old.asked) == n_old + 2 and len(new.asked) == n_new + 3
    with pytest.raises(ValueError, match="256"):
        ops.score_map(torch.zeros(16, 64, dtype=torch.float16), torch.zeros(1, 257, 64), 1, 16)
    for K, name in ((19, "upsample_argmax"), (150, "upsample_argmax_classes"), (2, "upsample_argmax_classes")):
        with pytest.raises(_Asked):
            evaluate.upsample_argmax(torch.zeros(1, K, 2, 2), (8, 8))
        assert ev.asked[-1] == name
    with pytest.raises(ValueError, match="256"):
        evaluate.upsample_argmax(torch.zeros(1, 300, 2, 2), (8, 8))
    for K, name in ((19, "seg_update"), (150, "seg_update_classes")):
        e = evaluate.Evaluator(num_classes=K, device="cpu")
        assert e.chunked == (K != 19)
        monkeypatch.setattr(e, "_classes_ws", lambda low: None)
        with pytest.raises(_Asked):
            e.update(torch.zeros(1, K, 2, 2), None, lab)
        assert ev.asked[-1] == name


def test_evaluator_limits_and_the_19_class_only_paths():
    from denseclip_vit_multimodal_amd import evaluate
    with pytest.raises(ValueError, match="256"):
        evaluate.Evaluator(num_classes=300, device="cpu")
    with pytest.raises(ValueError):
        evaluate.Evaluator(num_classes=0, device="cpu")
    e = evaluate.Evaluator(num_classes=150, device="cpu")
    assert e.cm.shape == (150, 150)
    lab = torch.zeros(1, 8, 8, dtype=torch.int64)
    lows = [torch.zeros(1, 150, 2, 2)]
    with pytest.raises(NotImplementedError, match="19 classes"):
        e.update_views(lows, None, [0], lab)
    with pytest.raises(NotImplementedError, match="19 classes"):
        e.update_windows(lows, None, (8, 8), [(0, 0)], lab)
    with pytest.raises(NotImplementedError, match="19 classes"):
        e.update_view_windows(lows, None, [(8, 8, 0, 8, 8, 1)], [(0, 0)], lab)

    class Model:
        num_classes = 150

        def forward_lowres(self, img):
            raise AssertionError("the model must not run: the class count is refused first")

    img = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="19 classes"):
        evaluate.predict_tta(Model(), img)
    with pytest.raises(NotImplementedError, match="19 classes"):
        evaluate.predict_slide(Model(), img, 8, 8)
    with pytest.raises(NotImplementedError, match="19 classes"):
        evaluate.predict_slide_tta(Model(), img, 8, 8)


def test_evaluator_workspace_is_sized_by_the_new_query(monkeypatch):
    from denseclip_vit_multimodal_amd import evaluate
    asked = []

    class E:
        @staticmethod
        def seg_classes_ws_bytes(B, K, h, w):
            asked.append((B, K, h, w))
            return 4096

    monkeypatch.setattr(evaluate, "_E", lambda: E)
    e = evaluate.Evaluator(num_classes=150, device="cpu")
    low = torch.zeros(2, 150, 4, 6)
    ws = e._classes_ws(low)
    assert asked == [(2, 150, 4, 6)] and ws.numel() == 4096 and ws.dtype == torch.uint8
    # one buffer per (device, byte count): another shape with the same need reuses it
    assert e._classes_ws(low) is ws and e._classes_ws(torch.zeros(1, 150, 9, 5)) is ws and len(e._seg_ws) == 1
    assert asked[-1] == (1, 150, 9, 5)


def test_a_config_with_150_classes_builds_the_model():
    from helpers import MID_CFG, CITYSCAPES_CLASSES
    from denseclip_vit_multimodal_amd import DenseCLIP
    names = [CITYSCAPES_CLASSES[i % 19] for i in range(150)]
    cfg = dict(MID_CFG)
    cfg["decode_head"] = dict(cfg["decode_head"], num_classes=150)
    cfg.pop("depth_head", None)
    model = DenseCLIP(class_names=names, **cfg)
    assert model.num_classes == 150 and model.depth_head is None and model.texts.shape[0] == 150


def test_yaml_classes_and_class_names_build_the_model():
    """`data.classes: N` with N `data.class_names` (and the head's num_classes) builds an N-class model;
    a count that disagrees with the names is refused"""
    import copy
    from helpers import MID_CFG, CITYSCAPES_CLASSES
    from denseclip_vit_multimodal_amd.config import build_model, config_class_names
    names = [CITYSCAPES_CLASSES[i % 19] for i in range(150)]
    model = {k: v for k, v in MID_CFG.items() if k not in ("clip_pretrained_path", "depth_head")}
    model["decode_head"] = dict(model["decode_head"], num_classes=150)
    cfg = {"data": {"classes": 150, "class_names": names}, "model": dict(model, type="DenseCLIP")}
    m = build_model(copy.deepcopy(cfg), clip_path_override="")
    assert m.num_classes == 150 and m.decode_head.classifier.out_channels == 150 and m.depth_head is None
    assert config_class_names({"data": {"classes": 19}, "model": {}}) == CITYSCAPES_CLASSES
    bad = copy.deepcopy(cfg)
    bad["data"]["classes"] = 151
    with pytest.raises(ValueError, match="151"):
        build_model(bad, clip_path_override="")
    with pytest.raises(ValueError, match="class_names"):
        config_class_names({"data": {"classes": 150}, "model": {}})
    bad = copy.deepcopy(cfg)
    bad["model"]["decode_head"]["num_classes"] = 19
    with pytest.raises(ValueError, match="num_classes"):
        build_model(bad, clip_path_override="")
