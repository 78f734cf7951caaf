"""Serving path: the DenseCLIP eval forward captured once into a HIP graph and replayed.

An inference step of ViT-B/16 issues ~620 launches from Python.  A captured forward replays every
launch of the step from one hipGraphLaunch: the host only copies the input in and launches, so a
small batch (latency-bound serving) runs at the GPU's pace and the host is free for the data path;
at the benchmark's batch of 8 the eager forward is already GPU-bound (the host runs ahead).  Every op of the eval forward is capture-safe (no host synchronisation, outputs from the
caching allocator, kernels on the current stream — csrc/torch_ops.cpp); the frozen text path is
captured as a parallel branch (launched eagerly on the model's side stream at the start of the
forward and joined before the score map, DenseCLIP._text_side_eager), so the replay recomputes it
like the reference does (denseclip.py:627-640) beside the backbone, as the eager forward's
side-stream graph replay does.

reference: segmentation/denseclip/denseclip.py:702-916 (DenseCLIP.forward, eval branch)
"""
import torch


class CapturedForward:
    """`model(img, return_loss=False)` for a fixed input shape / dtype / device, captured into a HIP
    graph.  Calling it copies `img` into the captured input buffer, replays the graph and returns the
    captured output dict ({'seg', 'depth'}: the SAME tensors every call — clone them to keep a result
    past the next call).  Weights must stay where they are (in-place updates are seen by the replay;
    a re-allocated parameter is not): build a new CapturedForward after loading other weights."""

    def __init__(self, model, example, warmup=2):
        if not example.is_cuda:
            raise RuntimeError("CapturedForward needs a GPU input (the MI355X path has no CPU fallback)")
        self.model = model
        self.static_in = example.detach().clone()
        saved = getattr(model, "graph_text", None)
        if saved is not None:
            model.graph_text = "side"  # the text path as a forked branch of this capture (no nested graph)
        try:
            side = torch.cuda.Stream(device=example.device)
            side.wait_stream(torch.cuda.current_stream(example.device))
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(max(1, warmup)):  # allocator pools, weight casts, library handles
                    model(self.static_in, return_loss=False)
            torch.cuda.current_stream(example.device).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(self.graph):
                self.static_out = model(self.static_in, return_loss=False)
        finally:
            if saved is not None:
                model.graph_text = saved

    def __call__(self, img):
        if img.shape != self.static_in.shape or img.dtype != self.static_in.dtype:
            raise ValueError(f"CapturedForward was captured for {tuple(self.static_in.shape)} {self.static_in.dtype}, "
                             f"got {tuple(img.shape)} {img.dtype}")
        if img.data_ptr() != self.static_in.data_ptr():
            self.static_in.copy_(img)
        self.graph.replay()
        return self.static_out


class CapturedEval:
    """`evaluate.predict(model, img)` for a fixed input shape / dtype / device, captured into a HIP
    graph: `forward_lowres`, the fused upsample + argmax of the logits and the resize of the depth.
    Calling it copies `img` in, replays and returns the captured {'seg': uint8 (B, H, W) class map,
    'depth': fp32 (B, 1, H, W)} (the SAME tensors every call, as CapturedForward's).  The resized
    (B, K, H, W) logits are never materialised, so the graph's pool does not hold them either."""

    def __init__(self, model, example, size=None, warmup=2):
        from . import evaluate
        if not example.is_cuda:
            raise RuntimeError("CapturedEval needs a GPU input (the MI355X path has no CPU fallback)")
        self.model = model
        self.size = size
        self.static_in = example.detach().clone()
        saved = getattr(model, "graph_text", None)
        if saved is not None:
            model.graph_text = "side"  # the text path as a forked branch of this capture (no nested graph)
        try:
            side = torch.cuda.Stream(device=example.device)
            side.wait_stream(torch.cuda.current_stream(example.device))
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):  # allocator pools, weight casts, library handles
                    evaluate.predict(model, self.static_in, size)
            torch.cuda.current_stream(example.device).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_out = evaluate.predict(model, self.static_in, size)
        finally:
            if saved is not None:
                model.graph_text = saved

    def __call__(self, img):
        if img.shape != self.static_in.shape or img.dtype != self.static_in.dtype:
            raise ValueError(f"CapturedEval was captured for {tuple(self.static_in.shape)} {self.static_in.dtype}, "
                             f"got {tuple(img.shape)} {img.dtype}")
        if img.data_ptr() != self.static_in.data_ptr():
            self.static_in.copy_(img)
        self.graph.replay()
        return self.static_out
