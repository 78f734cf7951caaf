"""bench.py's `--full` switch and its `--dump-outputs` writer, on the CPU: a plain run asks for none
of the extra measurements, and the writer samples the same elements on every call, as float32,
within the size budget."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

K = bench.DUMP_PER_TENSOR


def test_full_and_dump_outputs_default_off():
    a = bench.parse(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def _toy():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(96, 128), torch.nn.Linear(128, 3))  # 12288 > DUMP_PER_TENSOR
    m[0].weight.data = torch.arange(96 * 128.).view(128, 96) / 4096  # distinct values: a sample names its indices
    m[1].bias.requires_grad_(False)  # a frozen parameter: left out
    m(torch.randn(5, 96)).sum().backward()
    m[1].weight.grad = None  # trainable but without a gradient: zeros
    return m


def test_dump_train_step_outputs(tmp_path):
    m = _toy()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, {"loss": torch.tensor(2.5)})
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("loss", "grads", "params")}
    assert sorted(os.listdir(tmp_path / "a")) == ["grads.npy", "loss.npy", "params.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"].tolist() == [2.5]
    n = K + 128 + 128 * 3  # the sampled weight, the whole bias, the whole second weight
    assert got["grads"].shape == got["params"].shape == (n,)
    # small tensors whole and in order; the gradient-less one as zeros
    assert np.array_equal(got["params"][K:K + 128], m[0].bias.detach().numpy())
    assert np.array_equal(got["grads"][K:K + 128], m[0].bias.grad.numpy())
    assert np.array_equal(got["params"][-384:], m[1].weight.detach().numpy().ravel())
    assert not got["grads"][-384:].any()
    # the sample: elements of the tensor, the gradient at the same indices as the value
    w, g = m[0].weight.detach().numpy().ravel(), m[0].weight.grad.numpy().ravel()
    idx = {float(v): i for i, v in enumerate(w)}
    pick = [idx[float(v)] for v in got["params"][:K]]
    assert np.array_equal(got["grads"][:K], g[pick])
    # the same elements on every call
    for name, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (name + ".npy"))), name


def test_dump_inference_outputs_within_budget(tmp_path):
    big = 3 * bench.DUMP_PER_OUTPUT
    out = {"seg": torch.arange(big, dtype=torch.float64).view(3, -1), "depth": torch.ones(2, 7)}
    bench.dump_outputs(str(tmp_path), None, {"out": out})
    seg, depth = np.load(tmp_path / "seg.npy"), np.load(tmp_path / "depth.npy")
    assert seg.dtype == depth.dtype == np.float32
    assert seg.shape == (bench.DUMP_PER_OUTPUT,) and depth.shape == (14,)
    assert np.array_equal(seg, np.round(seg)) and seg.max() < big and len(np.unique(seg)) > 1
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) < 64 * 2 ** 20


def test_dump_budget_for_the_largest_model():
    """ViT-L/14 DenseCLIP has under 1000 parameter tensors: two files of DUMP_PER_TENSOR floats each
    stay far below 64 MB."""
    assert 2 * 1000 * bench.DUMP_PER_TENSOR * 4 < 64 * 2 ** 20
