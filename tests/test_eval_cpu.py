"""CPU checks of the validation path (csrc/headeval.hip, torch.ops.dclip_eval, evaluate.py): the three
new entry points are declared, bound and exported; their host checks reject bad arguments before any
launch; the dclip_eval ops are registered with fake implementations; Evaluator.compute() reproduces
the reference's recorded metrics (tests/golden/eval_metrics.npz, written by
golden/gen_eval_golden.py from the reference's compute_segmentation_metrics / compute_depth_errors)
from a state set by hand; Evaluator.all_reduce sums the state over gloo ranks."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import ROOT
from denseclip_vit_multimodal_amd import _native as N

NEW = ["dclip_upsample_eval_depth", "dclip_upsample_eval_seg", "dclip_upsample_eval_ws_bytes"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
P = ctypes.c_void_p(0x1000)  # a non-null pointer the host checks never dereference


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", f.read(), re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert lib.dclip_upsample_eval_ws_bytes.restype is ctypes.c_int64


def _seg(L, K=19, B=1, h=4, w=8, H=64, W=128, labels=P, pred=P, cm=P, loss=P, count=P, ws=P, low_dt=0, lab_dt=0):
    return L.dclip_upsample_eval_seg(low_dt, P, B, K, h, w, labels, lab_dt, H, W, 255, pred, cm, loss, count, ws, None)


def _depth(L, B=1, h=4, w=8, H=64, W=128, pred=P, target=P, sums=P, ws=P, low_dt=0):
    return L.dclip_upsample_eval_depth(low_dt, pred, B, h, w, target, None, H, W, 1e-3, 80.0, 1, 1e-6, None, sums, ws,
                                       None)


@pytest.mark.parametrize("call,needle", [
    (lambda L: _seg(L, K=20), "K=20"),
    (lambda L: _seg(L, H=3), "smaller than the input"),
    (lambda L: _seg(L, W=7), "smaller than the input"),
    (lambda L: _seg(L, B=8, H=16384, W=16384), "below 2^31"),
    (lambda L: _seg(L, cm=None), "cm, loss_sum and count required"),
    (lambda L: _seg(L, labels=None), "must be null without labels"),
    (lambda L: _seg(L, labels=None, pred=None, cm=None, loss=None, count=None), "nothing to do"),
    (lambda L: _seg(L, ws=None), "ws"),
    (lambda L: _seg(L, low_dt=5), "low_dt=5"),
    (lambda L: _seg(L, lab_dt=3), "lab_dt=3"),
    (lambda L: _depth(L, H=3), "smaller than the input"),
    (lambda L: _depth(L, B=2, H=32768, W=32768), "below 2^31"),
    (lambda L: _depth(L, sums=None), "sums required"),
    (lambda L: _depth(L, ws=None), "ws"),
    (lambda L: _depth(L, low_dt=-1), "low_dt=-1"),
], ids=["K20", "H_lt_h", "W_lt_w", "seg_2^31", "null_cm", "cm_without_labels", "nothing", "seg_null_ws", "seg_dtype",
        "label_dtype", "depth_H_lt_h", "depth_2^31", "null_sums", "depth_null_ws", "depth_dtype"])
def test_host_checks_reject_before_any_launch(call, needle):
    L = N.load()
    assert call(L) == -1
    assert needle in L.dclip_last_error().decode()


def test_k20_message_names_k():
    L = N.load()
    assert _seg(L, K=20) == -1 and "K" in L.dclip_last_error().decode()


def test_ws_bytes_is_a_function_of_its_arguments_alone():
    L = N.load()
    args = [(8, 19, 64, 128), (1, 19, 1, 1), (2, 1, 8, 16), (8, 1, 64, 128)]
    base = [L.dclip_upsample_eval_ws_bytes(*a) for a in args]
    assert all(b > 0 and b % 8 == 0 for b in base)
    assert L.dclip_upsample_eval_ws_bytes(0, 19, 4, 4) == 0
    touched = []
    try:
        for opt in range(20):
            for value in (1, 2, 7):
                if L.dclip_set_option(opt, value) == 0:
                    touched.append(opt)
                    assert [L.dclip_upsample_eval_ws_bytes(*a) for a in args] == base, (opt, value)
    finally:
        for opt in set(touched):
            L.dclip_set_option(opt, 0)


def test_eval_ops_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    E = torch.ops.dclip_eval
    for name in ("upsample_argmax", "seg_update", "depth_update"):
        assert hasattr(E, name), name
    assert str(E.seg_update.default._schema.returns[0].type) == "Optional[Tensor]"
    with FakeTensorMode():
        dev = "cuda"
        lg = torch.empty(2, 19, 8, 16, device=dev, dtype=torch.bfloat16)
        lab = torch.empty(2, 128, 256, device=dev, dtype=torch.uint8)
        cm = torch.empty(19, 19, device=dev, dtype=torch.int64)
        ce = torch.empty(2, device=dev, dtype=torch.float64)
        pm = E.upsample_argmax(lg, 128, 256)
        assert pm.shape == (2, 128, 256) and pm.dtype == torch.uint8 and pm.device.type == "cuda"
        pm = E.seg_update(lg, lab, 255, cm, ce, True)
        assert pm.shape == (2, 128, 256) and pm.dtype == torch.uint8
        assert E.seg_update(lg, lab, 255, cm, ce, False) is None
        dp = torch.empty(2, 1, 8, 16, device=dev, dtype=torch.float16)
        tg = torch.empty(2, 128, 256, device=dev)
        sums = torch.empty(12, device=dev, dtype=torch.float64)
        up = E.depth_update(dp, tg, None, 1e-3, 80.0, True, 1e-6, sums, True)
        assert up.shape == (2, 1, 128, 256) and up.dtype == torch.float32
        assert E.depth_update(dp, tg, lab, 1e-3, 80.0, True, 1e-6, sums, False) is None


def test_alias_package_reexports_evaluate():
    import denseclip.evaluate as ev
    from denseclip_vit_multimodal_amd import evaluate
    assert ev is evaluate and hasattr(ev, "Evaluator") and hasattr(ev, "predict") and hasattr(ev, "validate")
    from denseclip_vit_multimodal_amd import DenseCLIP, serve
    assert hasattr(DenseCLIP, "forward_lowres") and hasattr(serve, "CapturedEval")


def test_compute_reproduces_the_reference_metrics():
    """The Evaluator state of the fixture's batch (its confusion matrix and fp64 sums) gives every
    metric the reference recorded, to 1e-6 relative (the reference reduces in fp32)."""
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, DEPTH_KEYS
    g = np.load(GOLDEN)
    ev = Evaluator(device="cpu")
    ev.cm.copy_(torch.from_numpy(g["confusion_matrix"]))
    ev.ce_sums.copy_(torch.from_numpy(g["ce_sums"]))
    ev.depth_sums.copy_(torch.from_numpy(g["depth_sums"]))
    m = ev.compute()
    for k in ("accuracy", "mean_iou", "loss_seg", "rmse_masked") + DEPTH_KEYS:
        assert abs(m[k] - float(g[k])) <= 1e-6 * abs(float(g[k])), (k, m[k], float(g[k]))
    np.testing.assert_allclose(m["class_iou"], g["class_iou"], rtol=1e-6, atol=0)
    assert np.array_equal(m["confusion_matrix"], g["confusion_matrix"])
    # SILogLoss of the same sums
    s = g["depth_sums"]
    assert abs(m["loss_silog"] - (s[11] / s[8] - 0.5 * s[10] ** 2 / s[8] ** 2)) < 1e-12
    ev.reset()
    assert int(ev.cm.sum()) == 0 and float(ev.ce_sums.sum()) == 0 and float(ev.depth_sums.sum()) == 0


def test_compute_without_evaluated_pixels():
    from denseclip_vit_multimodal_amd.evaluate import Evaluator, DEPTH_KEYS
    ev = Evaluator(device="cpu")
    m = ev.compute()
    assert all(m[k] is None for k in DEPTH_KEYS) and m["rmse_masked"] is None and m["loss_seg"] is None
    assert m["loss_silog"] == 0.0 and m["accuracy"] == 0.0 and m["mean_iou"] == 0.0
    # masked pixels, none of them in [min_depth, max_depth]: the trainer's RMSE exists, the depth errors do not
    ev.depth_sums[8], ev.depth_sums[9] = 4.0, 16.0
    m = ev.compute()
    assert all(m[k] is None for k in DEPTH_KEYS) and m["rmse_masked"] == 2.0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _state(rank):
    g = torch.Generator().manual_seed(77 + rank)
    return (torch.randint(0, 1 << 40, (19, 19), generator=g), torch.rand(2, generator=g, dtype=torch.float64) * 1e6,
            torch.rand(12, generator=g, dtype=torch.float64) * 1e6)


def _reduce_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    from denseclip_vit_multimodal_amd.utils import init_distributed, cleanup
    from denseclip_vit_multimodal_amd.evaluate import Evaluator
    init_distributed(rank, world, backend="gloo")
    try:
        ev = Evaluator(device="cpu")
        for t, v in zip((ev.cm, ev.ce_sums, ev.depth_sums), _state(rank)):
            t.copy_(v)
        ev.all_reduce()
        torch.save({"cm": ev.cm, "ce": ev.ce_sums, "depth": ev.depth_sums}, os.path.join(out_dir, f"ev{rank}.pt"))
    finally:
        cleanup()


@pytest.mark.timeout(300)
def test_all_reduce_sums_the_state_over_ranks(tmp_path):
    world = 2
    mp.spawn(_reduce_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    a, b = _state(0), _state(1)
    for rank in range(world):
        r = torch.load(tmp_path / f"ev{rank}.pt", weights_only=True)
        assert torch.equal(r["cm"], a[0] + b[0])
        assert torch.equal(r["ce"], a[1] + b[1]) and torch.equal(r["depth"], a[2] + b[2])
