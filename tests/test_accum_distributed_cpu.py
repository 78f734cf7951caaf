"""Gradient accumulation under GradAllReduce on CPU (gloo, world size 2): 2 ranks x 2 micro-batches
through train.train_step_accum with torch AdamW.  The post-step parameters equal one process
stepping on the mean gradient of the four batches; no collective is issued inside no_sync()
(the first micro-batch's backward): every all_reduce of the step belongs to the last backward,
one per reduced gradient.

The module under the wrapper is test_distributed_cpu.py's: the trainable set of the reference
regime (neck + heads) on per-rank feature maps, in eval mode so BatchNorm keeps the check exact."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_distributed_cpu import _model, _batch, _free_port


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    import torch.distributed as dist
    from denseclip_vit_multimodal_amd.utils import init_distributed, cleanup
    from denseclip_vit_multimodal_amd import train
    init_distributed(rank, world, backend="gloo")
    try:
        model = train.GradAllReduce(_model())
        opt = train.make_optimizer([p for p in model.parameters() if p.requires_grad])
        calls, log = [0], []
        real = dist.all_reduce

        def counted(*a, **k):
            calls[0] += 1
            return real(*a, **k)

        real_backward = torch.Tensor.backward

        def backward(self, *a, **k):  # the collectives issued by each backward
            before = calls[0]
            real_backward(self, *a, **k)
            log.append(calls[0] - before)

        dist.all_reduce = counted
        torch.Tensor.backward = backward
        try:
            with model.no_sync():
                assert model._sync is False
            assert model._sync is True
            mbs = [_batch(2 * rank + i) for i in range(2)]  # batches 0, 1 on rank 0; 2, 3 on rank 1
            loss = train.train_step_accum(model, opt, mbs)
        finally:
            dist.all_reduce = real
            torch.Tensor.backward = real_backward
        reduced = sum(len(b) for b in model._buckets)
        params = {n: p.detach().clone() for n, p in model.module.named_parameters()}
        torch.save({"params": params, "loss": loss, "log": torch.tensor(log), "reduced": reduced},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        cleanup()


@pytest.mark.timeout(300)
def test_accumulation_world2_matches_single_process(tmp_path):
    from denseclip_vit_multimodal_amd.train import loss_fn, make_optimizer
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"rank{i}.pt", weights_only=True) for i in range(world)]

    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    ref = _model()
    opt = make_optimizer([p for p in ref.parameters() if p.requires_grad])
    total = 0
    for b in range(4):
        maps, seg, depth, mask = _batch(b)
        total = total + loss_fn(ref(maps, gt_semantic_seg=seg, gt_depth=depth), seg, depth, mask)
    (total / 4).backward()
    opt.step()
    torch.set_num_threads(nt)

    for i in range(world):
        # no collective inside no_sync(): the first backward issued none, the last one per gradient
        assert r[i]["log"].tolist() == [0, r[i]["reduced"]], (r[i]["log"], r[i]["reduced"])
        assert r[i]["reduced"] > 10
    for n, p in ref.named_parameters():
        assert torch.equal(r[0]["params"][n], r[1]["params"][n]), n  # the replicas stay identical
        # fp32 summation order is the only difference (two sums of two vs one sum of four)
        torch.testing.assert_close(r[0]["params"][n], p.detach(), rtol=1e-6, atol=0, msg=n)
    assert not torch.equal(r[0]["loss"], r[1]["loss"])  # the shards really differ
