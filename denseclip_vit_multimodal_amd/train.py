"""Data-parallel train step of the reference trainer, restated for one process per GPU.

What `seg/train_denseclip.py` does around the hot path, kept to the parts that shape the
step (its CLI, logging, metrics and checkpointing are out of scope — DESIGN.md §7):
  * freeze rule            train_denseclip.py:1040-1044 (backbone.* and text_encoder.*)
  * DDP wrap               train_denseclip.py:1050-1054 (gradient all-reduce over RCCL)
  * loss                   train_denseclip.py:1086-1095, 1265-1314: CE(ignore 255) + 0.1 SILog
  * optimiser              train_denseclip.py:1061: AdamW(lr 2e-5, weight decay 0.01)
  * per-rank data          DistributedSampler (train_denseclip.py:242): rank r sees its own
                           shard; here synthetic Cityscapes-shaped tensors seeded per rank
                           (real data: data.CityscapesDepthSegDataset + data.prepare_batch).
  * checkpoints            train_denseclip.py:1012-1034 (--load), 1107-1133 (--resume),
                           1491-1521 (save): {'epoch', 'state_dict', 'optimizer'[, 'scheduler']}.
Mode "R" is the reference regime (backbone + text frozen); mode "F" also trains the ViT,
which exercises the HIP backward kernels (the north star's roofline applies there).
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from .losses import SILogLoss

# parameters that never receive a gradient: the unused CLIP projection and everything the
# score-map branch touches — the learnable text contexts, gamma, vis_proj / global_proj and the
# ContextDecoder.  That branch runs under no_grad and its output is discarded for every
# score_concat_index (the reference concatenates the score map onto a clone of the maps that the
# forward never passes on, denseclip.py:586, 684-694, 747).  They stay trainable — the
# reference's AdamW param list holds them (train_denseclip.py:1040-1044, 1061), so optimizer
# states interoperate — and are kept out of the DDP gradient reduction instead.
#
# With an identity head (DenseCLIP(identity_head=...)) the branch trains: score / tau is supervised as
# segmentation logits, so the contexts and vis_proj get gradients, gamma and the ContextDecoder too when
# one is configured, and global_proj when the decoder's context holds the pooled feature
# (context_feature "attention").  Without a decoder the pooled feature feeds nothing: gamma and
# global_proj stay dead.  backbone.proj is dead either way.
_DEAD = ("backbone.proj", "contexts", "gamma")
_DEAD_PREFIX = ("vis_proj.", "global_proj.", "context_decoder.")


def _dead_names(m):
    """(exact names, prefixes) of the parameters the model's configuration leaves without a gradient"""
    if not getattr(m, "with_identity_head", False):
        return _DEAD, _DEAD_PREFIX
    if getattr(m, "context_decoder", None) is None:
        return ("backbone.proj", "gamma"), ("global_proj.",)
    if getattr(m, "context_feature", "attention") == "attention":
        return ("backbone.proj",), ()
    return ("backbone.proj",), ("global_proj.",)


def gradless_parameter_names(model):
    """Trainable parameter names that get no gradient (DDP must not wait for them)."""
    m = _unwrap(model)
    dead, prefix = _dead_names(m)
    return [n for n, p in m.named_parameters()
            if p.requires_grad and (n in dead or (bool(prefix) and n.startswith(prefix)))]


def freeze_for_mode(model, mode):
    """requires_grad per the reference freeze rule (train_denseclip.py:1040-1044: backbone.* and
    text_encoder.* frozen; mode F also trains the backbone); returns the trainable parameters
    in named_parameters order — the reference optimizer's param list."""
    if mode not in ("F", "R"):
        raise ValueError(f"mode must be 'F' or 'R' (got {mode!r})")
    params = []
    for name, p in model.named_parameters():
        frozen = name.startswith("text_encoder.")
        if mode == "R":
            frozen = frozen or name.startswith("backbone.")
        p.requires_grad_(not frozen)
        if not frozen:
            params.append(p)
    return params


def synth_batch(B, H, W, device, rank=0, image_dtype=torch.bfloat16, num_classes=19):
    """Rank-seeded synthetic Cityscapes-shaped batch (images randn seed 1234,
    seg labels with 10 % ignore (255) seed 1235, depth U(1, 80) with 20 % invalid seed 1236)."""
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    img = torch.randn(B, 3, H, W, generator=g).to(device).to(image_dtype)
    g = torch.Generator(device="cpu").manual_seed(1235 + rank)
    seg = torch.randint(0, num_classes, (B, H, W), generator=g)
    seg[torch.rand(B, H, W, generator=g) < 0.1] = 255
    g = torch.Generator(device="cpu").manual_seed(1236 + rank)
    depth = 1 + 79 * torch.rand(B, 1, H, W, generator=g)
    mask = torch.rand(B, 1, H, W, generator=g) >= 0.2
    return img, seg.to(device), depth.to(device), mask.to(device)


def loss_config(cfg):
    """(seg weight, silog weight, SILogLoss) from a trainer YAML (train_denseclip.py:1088-1095,
    1311-1312: training.loss_weights.{seg, silog}, training.silog_loss.{lambda, eps})."""
    tr = (cfg or {}).get("training", {}) or {}
    # the reference's defaults: the whole dict {'seg': 1.0, 'silog': 0.1} when absent, 1.0 for a
    # key missing from a given dict (train_denseclip.py:1094-1095, 1311-1312)
    w = tr.get("loss_weights", {"seg": 1.0, "silog": 0.1}) or {}
    sl = tr.get("silog_loss", {}) or {}
    return (float(w.get("seg", 1.0)), float(w.get("silog", 1.0)),
            SILogLoss(lambd=float(sl.get("lambda", 0.5)), eps=float(sl.get("eps", 1e-6))))


def identity_loss_weight(cfg_or_model):
    """The identity head's loss weight, or None without one.  A model: its head's (DenseCLIP(identity_head=
    dict(loss_weight=...)), 0.4 in the published configs).  A trainer YAML: model.identity_head's
    (loss_decode.loss_weight first, then loss_weight, then 0.4), overridden by training.loss_weights.identity."""
    if isinstance(cfg_or_model, torch.nn.Module):
        m = _unwrap(cfg_or_model)
        return m.identity_loss_weight if getattr(m, "with_identity_head", False) else None
    cfg = cfg_or_model or {}
    head = (cfg.get("model", {}) or {}).get("identity_head")
    if not head:
        return None
    w = ((cfg.get("training", {}) or {}).get("loss_weights", {}) or {}).get("identity")
    if w is None:
        ld = head.get("loss_decode")
        w = ld.get("loss_weight") if isinstance(ld, dict) else None
    if w is None:
        w = head.get("loss_weight", 0.4)
    return float(w)


def seg_loss_config(cfg, num_classes):
    """The segmentation loss of a trainer YAML, or None when it has none (the plain CE):
    training.seg_loss: {class_weight: [num_classes floats], label_smoothing: x, ohem: {thresh:, min_kept:}},
    every key optional.  Returns a losses.SegCrossEntropy for loss_fn's seg_loss."""
    sl = ((cfg or {}).get("training", {}) or {}).get("seg_loss")
    if sl is None:
        return None
    cw = sl.get("class_weight")
    if cw is not None:
        cw = [float(x) for x in cw]
        if len(cw) != int(num_classes):
            raise ValueError(f"training.seg_loss.class_weight: {len(cw)} weights for {num_classes} classes")
        if any(not x >= 0.0 for x in cw):
            raise ValueError("training.seg_loss.class_weight: a negative weight")
    eps = float(sl.get("label_smoothing", 0.0))
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"training.seg_loss.label_smoothing={eps} (0 <= label_smoothing < 1)")
    ohem = sl.get("ohem")
    if ohem is not None:
        ohem = {"thresh": float(ohem.get("thresh", 0.7)), "min_kept": int(ohem.get("min_kept", 100000))}
        if not 0.0 < ohem["thresh"] <= 1.0:
            raise ValueError(f"training.seg_loss.ohem.thresh={ohem['thresh']} (0 < thresh <= 1)")
        if ohem["min_kept"] < 0:
            raise ValueError(f"training.seg_loss.ohem.min_kept={ohem['min_kept']} (>= 0)")
    from .losses import SegCrossEntropy
    return SegCrossEntropy(weight=cw, label_smoothing=eps, ignore_index=255, ohem=ohem)


def depth_loss_config(cfg):
    """The depth loss of a trainer YAML, or None when it has none (the plain SILog): training.depth_loss is
    either {type: silog | l1 | berhu} (the reference's LOSS_TYPE, configs/denseclip_multitask_cityscapes.yaml:
    67-70) or {terms: {silog: 1.0, l1: 0.5, berhu: 0.5}} (a weighted sum; an absent term weighs 0), with an
    optional berhu_threshold (0.2).  SILog's lambda / eps come from training.silog_loss, as loss_config reads
    them.  Returns a losses.DepthLoss for loss_fn's depth_loss."""
    tr = (cfg or {}).get("training", {}) or {}
    dl = tr.get("depth_loss")
    if dl is None:
        return None
    if not isinstance(dl, dict) or ("type" in dl) == ("terms" in dl):
        raise ValueError("training.depth_loss: give either type (silog, l1 or berhu) or terms ({silog:, l1:, berhu:})")
    unknown = set(dl) - {"type", "terms", "berhu_threshold"}
    if unknown:
        raise ValueError(f"training.depth_loss: unknown keys {sorted(unknown)} (type, terms, berhu_threshold)")
    names = ("silog", "l1", "berhu")
    if "type" in dl:
        kind = str(dl["type"]).lower()
        if kind not in names:
            raise ValueError(f"training.depth_loss.type={dl['type']!r} (silog, l1 or berhu)")
        w = {n: float(n == kind) for n in names}
    else:
        terms = dl["terms"]
        if not isinstance(terms, dict) or not terms or set(terms) - set(names):
            raise ValueError(f"training.depth_loss.terms={terms!r} (weights for silog, l1 and / or berhu)")
        w = {n: float(terms.get(n, 0.0)) for n in names}
        if any(not (math.isfinite(v) and v >= 0.0) for v in w.values()):
            raise ValueError(f"training.depth_loss.terms={terms!r}: a weight is negative or not finite")
        if not any(v > 0.0 for v in w.values()):
            raise ValueError(f"training.depth_loss.terms={terms!r}: every weight is zero")
    theta = float(dl.get("berhu_threshold", 0.2))
    if not 0.0 < theta <= 1.0:
        raise ValueError(f"training.depth_loss.berhu_threshold={theta} (0 < berhu_threshold <= 1)")
    sl = tr.get("silog_loss", {}) or {}
    from .losses import DepthLoss
    return DepthLoss(silog=w["silog"], l1=w["l1"], berhu=w["berhu"], lambd=float(sl.get("lambda", 0.5)),
                     eps=float(sl.get("eps", 1e-6)), berhu_threshold=theta)


def loss_fn(out, seg, depth, mask, silog=None, seg_weight=1.0, silog_weight=0.1, seg_loss=None, identity_weight=None,
            depth_loss=None):
    """seg_weight * CE(ignore 255) + silog_weight * SILog (train_denseclip.py:1265-1314; the
    weights and the SILog parameters come from the config, `loss_config`).  With a model in
    fused_head_loss mode the outputs are the heads' low-res maps and the resize + loss run
    as one fused kernel each (identical loss and gradients).  A batch whose labels are all
    ignored gives a NaN CE, as torch's CrossEntropyLoss does (the reference trainer then
    skips the step, train_denseclip.py:1323).  seg_loss: a losses.SegCrossEntropy (`seg_loss_config`) in
    the CE's place: class weights, label smoothing, OHEM; None is the plain CE.
    identity_weight (`identity_loss_weight`): adds identity_weight * CE(identity logits, ignore 255), the plain
    CE on the model's score map / tau (DenseCLIP(identity_head=...)): the fused resize + CE on
    out["identity_output_lowres"], F.cross_entropy on out["aux_losses"]["identity_head"] otherwise.  Logits
    without a weight raise: the head's parameters are counted as alive.
    depth_loss: a losses.DepthLoss (`depth_loss_config`) in SILog's place: any weighted sum of SILog, L1 and
    BerHu, the whole of it times silog_weight (the reference weights "the sum of depth components" by
    loss_weights.silog, train_denseclip.py:1276-1312); `silog` is then unused.  None is the plain SILog."""
    silog = silog or SILogLoss()
    low = out.get("identity_output_lowres")
    full = (out.get("aux_losses") or {}).get("identity_head")
    if identity_weight is None and (low is not None or full is not None):
        # the head's parameters count as alive (gradless_parameter_names): without the term they would get no
        # gradient and GradAllReduce's buckets would never complete
        raise ValueError("loss_fn: the model returned identity-head logits but no identity_weight was given "
                         "(pass identity_weight=train.identity_loss_weight(model))")
    if identity_weight is not None:
        if low is None and full is None:
            raise ValueError("loss_fn: identity_weight given but the model returned no identity logits "
                             "(build it with identity_head=dict(type='IdentityHead', ...) and call it in training)")
    if out.get("main_output_lowres") is not None:
        from . import ops
        if seg_loss is None:
            ce = ops.UpsampleCEFn.apply(out["main_output_lowres"], seg, 255)
        else:
            ce = seg_loss.fused(out["main_output_lowres"], seg)
        loss = seg_weight * ce
        if out.get("depth_output_lowres") is not None:
            if depth_loss is None:
                loss = loss + silog_weight * ops.UpsampleSILogFn.apply(out["depth_output_lowres"], depth, mask,
                                                                       silog.lambd, silog.eps)
            else:
                loss = loss + silog_weight * depth_loss.fused(out["depth_output_lowres"], depth, mask)
        if identity_weight is not None:
            loss = loss + identity_weight * _identity_ce(low, full, seg)
        return loss
    if seg_loss is None:
        ce = F.cross_entropy(out["main_output"], seg, ignore_index=255)
    else:
        ce = seg_loss(out["main_output"], seg)
    loss = seg_weight * ce
    if out.get("depth_output") is not None:
        dl = silog if depth_loss is None else depth_loss
        loss = loss + silog_weight * dl(out["depth_output"], depth, mask)
    if identity_weight is not None:
        loss = loss + identity_weight * _identity_ce(low, full, seg)
    return loss


def _identity_ce(low, full, seg):
    if low is not None:
        from . import ops
        return ops.upsample_cross_entropy(low, seg, ignore_index=255)
    return F.cross_entropy(full, seg, ignore_index=255)


# wrap_ddp's data-parallel implementation: "allreduce" (GradAllReduce: bucketed in-place
# all-reduces of the gradients autograd produced) or "ddp" (torch's DistributedDataParallel)
DP_IMPL = "allreduce"


def wrap_ddp(model, device=None, grad_dtype=None, impl=None):
    """Data parallelism over the default process group (RCCL on GPUs, gloo on CPU): GradAllReduce
    (DP_IMPL "allreduce", the default) or torch DDP ("ddp", and always for grad_dtype bf16).
    DDP: 100 MB buckets:
    fewer, larger all-reduces suit xGMI's per-link ring bandwidth; the buckets are views of
    the gradients (no copy).  Trainable parameters that get no gradient in this config
    (`gradless_parameter_names`) are left out of the reduction rather than searched for every
    step (find_unused_parameters).  grad_dtype=torch.bfloat16 all-reduces the buckets in bf16
    (half the xGMI bytes; the sum is rounded to 8 mantissa bits) via DDP's compression hook."""
    impl = impl or DP_IMPL
    if impl not in ("allreduce", "ddp"):
        raise ValueError(f"unknown data-parallel implementation {impl!r}")
    if impl == "allreduce" and grad_dtype in (None, torch.float32):
        return GradAllReduce(model)
    from torch.nn.parallel import DistributedDataParallel as DDP
    ignore = set(gradless_parameter_names(model))
    if ignore:
        # DDP matches both the named_parameters() name ("gamma") and f"{module_name}.{param_name}"
        # (".gamma" for a top-level parameter) in different places: give both forms
        fq = [f"{mn}.{pn}" for mn, mod in model.named_modules() for pn, _ in mod.named_parameters(recurse=False)
              if (f"{mn}.{pn}" if mn else pn) in ignore]
        DDP._set_params_and_buffers_to_ignore_for_model(model, sorted(ignore | set(fq)))
    ids = [device.index] if device is not None and device.type == "cuda" else None
    ddp = DDP(model, device_ids=ids, bucket_cap_mb=100, gradient_as_bucket_view=True,
              find_unused_parameters=False)
    if grad_dtype == torch.bfloat16:
        from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
        ddp.register_comm_hook(None, default_hooks.bf16_compress_hook)
    elif grad_dtype not in (None, torch.float32):
        raise ValueError(f"unsupported gradient all-reduce dtype {grad_dtype}")
    return ddp


class GradAllReduce(torch.nn.Module):
    """Data parallelism over the default process group without DDP's gradient copies: the same
    contract as wrap_ddp (parameters broadcast from rank 0 at wrap time, buffers before every
    forward, gradients averaged over the ranks before the optimizer step, overlapped with the
    backward, ~100 MB buckets in reverse registration order — the last to complete ~25 MB, so
    little is left exposed after the backward — the gradless parameters left out)
    — but each bucket's collective runs on the gradient tensors autograd produced, in place.

    Why: DDP keeps a flat bucket per ~100 MB and copies every gradient into it (or accumulates
    into bucket views): at ViT-B/16 ~250 device copies and ~100 fills per step, +3 % of the step at
    world size 1 (profiles/r05/r5ac) — a fixed cost of every N > 1 step.  Here a post-accumulate-
    grad hook counts each bucket's arrivals; the bucket whose last gradient lands is reduced at
    once (RCCL: one coalesced group of in-place AVG all-reduces on the process group's stream; gloo:
    SUM then / world), and a callback queued on the autograd engine waits for every bucket at the
    end of the backward (the current stream waits on the collectives' stream; no host sync for
    RCCL).  Gradients of `set_to_none` steps are stolen by autograd, so nothing is copied."""

    def __init__(self, module, bucket_cap_mb=100, broadcast_buffers=True, last_bucket_cap_mb=25):
        super().__init__()
        import torch.distributed as dist
        self.module = module
        self._dist = dist
        ignore = set(gradless_parameter_names(module))
        params = [(n, p) for n, p in module.named_parameters() if p.requires_grad and n not in ignore]
        # the parameters not ignored (DDP's attribute: frozen ones included; only those with
        # requires_grad are reduced)
        self._module_parameters = [p for n, p in module.named_parameters() if n not in ignore]
        from torch.distributed.distributed_c10d import _get_default_group
        if self._module_parameters and dist.get_world_size() > 1:
            # rank 0's initial parameters, flattened into ~250 MB broadcasts: EVERY parameter not
            # ignored, frozen ones included, as DDP's _sync_module_states does (the reference seeds
            # each rank with seed + rank, train_denseclip.py:941, so a randomly initialised frozen
            # weight would otherwise differ between ranks)
            with torch.no_grad():
                dist._broadcast_coalesced(_get_default_group(), [p.data for p in self._module_parameters],
                                          250 * 2 ** 20, 0)
        self._buffers_to_sync = [b for b in module.buffers()] if broadcast_buffers else []
        # gradients arrive roughly in reverse registration order, so the bucket of the FIRST
        # registered parameters (patch embedding, block 0) completes last and its all-reduce is the
        # one left exposed after the backward: it is cut at last_bucket_cap_mb (~block 0 at
        # ViT-B/16), the others at bucket_cap_mb (few, large collectives for xGMI's ring links)
        caps = (min(last_bucket_cap_mb, bucket_cap_mb) * 2 ** 20, bucket_cap_mb * 2 ** 20)
        fwd, cur, size = [], [], 0
        for _, p in params:
            cur.append(p)
            size += p.numel() * p.element_size()
            if size >= caps[1 if fwd else 0]:
                fwd.append(cur)
                cur, size = [], 0
        if cur:
            fwd.append(cur)
        self._buckets = [list(reversed(b)) for b in reversed(fwd)]  # in the order they complete
        self._bucket_of = {}
        for i, b in enumerate(self._buckets):
            for p in b:
                self._bucket_of[p] = i
        self._nccl = dist.get_backend() == "nccl"
        self._world = dist.get_world_size()
        # one rank: the average is the identity and no collective is issued (set False to exercise
        # the collective path anyway — bench.py's ddp1 line prices RCCL's one-rank all-reduce so)
        self.skip_collectives = self._world == 1
        self.coalesce = True  # RCCL: a bucket's all-reduces as one group call
        # the persistent GEMMs' tile walk while a bucket's collective is in flight (DCLIP_OPT_GEMM_SCHED
        # value: 1 = every tile claimed, so the workgroups that find a CU held by RCCL's channel
        # kernels leave their tiles to the others; None keeps whatever walk is set).  The static walk
        # is faster uncontended (+4 % for claims) but loses 49 % vs 22 % with 16 CUs held
        # (profiles/r05/r5e_ab_gemm_walks.log), and the buckets complete through the whole backward,
        # so the GEMMs launched between the first bucket's launch and _finish take the claims walk
        self.gemm_walk_under_collectives = 1
        self._pending = None
        self._sync = True  # False inside no_sync()
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for _, p in params]

    @contextlib.contextmanager
    def no_sync(self):
        """Gradient accumulation, as DistributedDataParallel.no_sync(): backwards run inside it add
        to the local gradients only — the hooks neither count arrivals nor launch a collective.
        The first backward outside it reduces the accumulated sums (train_step_accum)."""
        prev, self._sync = self._sync, False
        try:
            yield
        finally:
            self._sync = prev

    def forward(self, *args, **kwargs):
        if self._buffers_to_sync and self._world > 1:
            # rank 0's buffers (BN running statistics: 45 small tensors at ViT-B/16) in one
            # flattened broadcast per dtype, as DDP's buffer sync does — not one collective each
            from torch.distributed.distributed_c10d import _get_default_group
            with torch.no_grad():
                self._dist._broadcast_coalesced(_get_default_group(), self._buffers_to_sync, 250 * 2 ** 20, 0)
        self._pending = None
        return self.module(*args, **kwargs)

    def _launch(self, i):
        grads = [p.grad for p in self._buckets[i] if p.grad is not None]
        st = self._pending
        st["launched"][i] = True
        if not grads or self.skip_collectives:
            return
        if st["walk"] is None and self.gemm_walk_under_collectives is not None:
            from . import ops
            st["walk"] = ops.set_gemm_walk(self.gemm_walk_under_collectives)
        d = self._dist
        if self._nccl and self.coalesce:
            with d._coalescing_manager(async_ops=True) as cm:
                for g in grads:
                    d.all_reduce(g, op=d.ReduceOp.AVG)
            st["works"].append((cm, None))
        elif self._nccl:  # one async call per tensor
            for g in grads:
                st["works"].append((d.all_reduce(g, op=d.ReduceOp.AVG, async_op=True), None))
        else:
            for g in grads:
                st["works"].append((d.all_reduce(g, async_op=True), g))

    def _on_grad(self, p):
        if not self._sync:
            return
        if self._pending is None:
            self._pending = {"ready": [0] * len(self._buckets), "launched": [False] * len(self._buckets), "works": [],
                             "next": 0, "walk": None}
            torch.autograd.Variable._execution_engine.queue_callback(self._finish)
        i = self._bucket_of[p]
        st = self._pending
        st["ready"][i] += 1
        # collectives are issued in BUCKET order, as DDP's reducer does: a bucket that completes
        # early waits for its predecessors, so every rank issues the same sequence of collectives
        # even if autograd visits the parameters in a different order on some rank
        while st["next"] < len(self._buckets) and st["ready"][st["next"]] == len(self._buckets[st["next"]]):
            self._launch(st["next"])
            st["next"] += 1

    def _finish(self):
        st = self._pending
        if st is None:
            return
        for i, done in enumerate(st["launched"]):
            if not done:  # a bucket some of whose parameters got no gradient this step (bucket order)
                self._launch(i)
        for w, g in st["works"]:
            w.wait()
            if g is not None:  # gloo has no AVG
                g.div_(self._world)
        if st["walk"] is not None:  # the current stream now waits on the collectives: back to the walk before
            from . import ops
            ops.set_gemm_walk(st["walk"])
        self._pending = None


def make_optimizer(params, fused=None, capturable=False, native=False, clip_grad_norm=None):
    """AdamW(lr 2e-5, weight decay 0.01) as the reference trainer builds it (train_denseclip.py:1061),
    fused on GPU parameters; capturable=True keeps its step counts on the device (required by
    CapturedTrainStep).  native=True: FusedAdamW, this package's own multi-tensor step (always
    capturable), which clips to a global norm of clip_grad_norm when that is given."""
    params = list(params)
    if native:
        return FusedAdamW(params, lr=2e-5, weight_decay=0.01, max_norm=clip_grad_norm)
    if clip_grad_norm is not None:
        raise ValueError("make_optimizer: clip_grad_norm belongs to the native optimizer (native=True); with a torch "
                         "optimizer pass it to train_step_accum")
    if fused is None:
        fused = all(p.is_cuda for p in params)
    if capturable:
        return torch.optim.AdamW(params, lr=2e-5, weight_decay=0.01, fused=fused, capturable=True)
    return torch.optim.AdamW(params, lr=2e-5, weight_decay=0.01, fused=fused)


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's step as this package's own two HIP passes (csrc/optim.hip, the arithmetic
    in include/dclip.h), with what the trainer's YAML asks for around it:
      * max_norm         torch.nn.utils.clip_grad_norm_ over ALL groups' gradients, applied as a
                         factor on load (the gradients are never rewritten); the threshold is
                         the first group's
      * set_inv_accum    the 1/k of a k-micro-batch accumulation, applied the same way
      * group["lr"]      a float, or a 1-element device tensor that a scheduler may rewrite between
                         replays of a captured step (the kernels read lr from device memory)
      * found_inf        honoured as torch's fused optimizers honour it (step_unless_nonfinite);
                         with check_grads the norm pass also flags non-finite gradients
      * the 16-bit plain and transposed weight copies of ops.WEIGHTS are written by the update
        itself (no weight_refresh launch follows), under ops.collect_weight_copies' rules.
    GPU fp32 parameters only (no CPU fallback).  One step count for the whole optimizer, on the
    device; it does not advance on a skipped step.  state_dict() / load_state_dict() interchange
    with torch.optim.AdamW: 'step' (f32), 'exp_avg', 'exp_avg_sq' per parameter — loading per-
    parameter steps that differ raises.  No host synchronisation in step().  amsgrad / maximize
    are not supported.

    last_total_norm / last_found_inf: 0-dim device tensors of the last prepared step (views of the
    optimizer's state: clone them to keep a value).

    The gradient addresses go to the kernels as launch arguments, 256 per launch: nothing
    the host could overwrite while an earlier step's launch still reads it."""

    writes_weight_copies = True  # ops' step hook: no weight_refresh after this optimizer

    def __init__(self, params, lr=2e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=None):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0 or weight_decay < 0:
            raise ValueError(f"FusedAdamW: invalid betas {betas}, eps {eps} or weight_decay {weight_decay}")
        # every key a torch.optim.AdamW group carries, so that state dicts load in both directions
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, fused=True, capturable=True,
                        max_norm=max_norm)
        super().__init__(params, defaults)
        self._device = None
        for g in self.param_groups:
            for p in g["params"]:
                if not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError(f"FusedAdamW: GPU fp32 parameters only (got {tuple(p.shape)} {p.dtype} on "
                                       f"{p.device}); the MI355X path has no CPU fallback")
                if self._device is None:
                    self._device = p.device
                elif p.device != self._device:
                    raise RuntimeError("FusedAdamW: all parameters on one device")
        self._inv_accum = 1.0
        self._hp = self._st = None   # device hyper-parameter table / state (include/dclip.h)
        self._hp_host = []           # the floats last written to the table, per row
        self._desc = None            # (key, device descriptor, host descriptor, tiles)
        self._prepared = None        # (desc, grads, copies, [(p, p.grad)]) between prepare() and step()
        self._stepped = None         # copies of the last step, for the hook's re-stamp

    # ------------------------------------------------------------------ device scalars
    def _buffers(self):
        rows = len(self.param_groups)
        if self._st is None or self._hp.shape[0] != rows:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: run one eager step before capturing the train step")
            step = None if self._st is None else self._st[3].clone()
            self._hp = torch.zeros(rows, 8, dtype=torch.float32, device=self._device)
            self._st = torch.zeros(8 + 12 * rows, dtype=torch.float32, device=self._device)
            if step is not None:
                self._st[3] = step
            self._hp_host = [None] * rows
        return self._hp, self._st

    @property
    def last_total_norm(self):
        return self._buffers()[1][0]

    @property
    def last_found_inf(self):
        return self._buffers()[1][2]

    @property
    def step_count(self):
        """0-dim device f32: the number of steps applied"""
        return self._buffers()[1][3]

    def set_inv_accum(self, inv_accum):
        """1 / k for gradients summed over k micro-batches (train_step_accum)"""
        self._inv_accum = float(inv_accum)

    def _sync_hp(self):
        """Bring the device table up to the groups' values: a changed float is written by a fill
        (a kernel argument: no host buffer, no synchronisation); a tensor lr is copied on the device."""
        hp, _ = self._buffers()
        capturing = torch.cuda.is_current_stream_capturing()
        for r, g in enumerate(self.param_groups):
            if g.get("amsgrad") or g.get("maximize"):
                raise RuntimeError("FusedAdamW: amsgrad / maximize are not supported")
            lr = g["lr"]
            vals = [None if torch.is_tensor(lr) else float(lr), 1.0 - float(g["betas"][0]), 1.0 - float(g["betas"][1]),
                    float(g["eps"]), float(g["weight_decay"]), float(g.get("max_norm") or 0.0), self._inv_accum, 0.0]
            old = self._hp_host[r]
            for k, v in enumerate(vals):
                if v is None:
                    if not lr.is_cuda or lr.numel() != 1:
                        raise RuntimeError("FusedAdamW: a tensor lr must be a 1-element GPU tensor")
                    hp[r, 0:1].copy_(lr.detach().reshape(1))
                elif old is None or old[k] != v:
                    if capturing:
                        raise RuntimeError(f"FusedAdamW: hyper-parameter {k} of group {r} changed under stream capture "
                                           "(use a 1-element device tensor for a scheduled lr; run one eager step "
                                           "before capturing the train step)")
                    hp[r, k].fill_(v)
            self._hp_host[r] = vals

    # ------------------------------------------------------------------ descriptor
    def _collect(self):
        """Entries for the parameters that have a gradient: (descriptor, gradients, copy items)."""
        from . import ops
        entries = []
        for r, g in enumerate(self.param_groups):
            for p in g["params"]:
                gr = p.grad
                if gr is None or p.numel() == 0:
                    continue
                if gr.is_sparse or gr.dtype != torch.float32 or gr.device != p.device:
                    raise RuntimeError(f"FusedAdamW: dense fp32 gradients on the parameter's device only "
                                       f"(parameter {tuple(p.shape)})")
                w = p.detach()
                if not (w.is_contiguous() or (w.dim() == 4 and w.is_contiguous(memory_format=torch.channels_last))):
                    raise RuntimeError(f"FusedAdamW: parameter {tuple(p.shape)} is not dense in memory")
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(w, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(w, memory_format=torch.preserve_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if m.stride() != w.stride() or v.stride() != w.stride():
                    raise RuntimeError(f"FusedAdamW: the moments of parameter {tuple(p.shape)} have another layout")
                if gr.stride() != w.stride():  # elementwise over the storage: the same layout as p
                    gr = torch.empty_like(w, memory_format=torch.preserve_format).copy_(gr)
                entries.append((r, p, w, gr, m, v))
        if not entries:
            return None
        copies = {}
        for items in ops.collect_weight_copies([e[1] for e in entries]).values():
            for it in items:  # a parameter with copies in both dtypes: the first (bf16) is written here,
                copies.setdefault(id(it[-1]), it)  # the other keeps a stale stamp and is rebuilt on use
        key, mine = [], []
        for r, p, w, gr, m, v in entries:
            it = copies.get(id(p))
            rows = w.shape[0] if w.dim() else 1
            cols = w.numel() // rows
            vp = vt = None
            dt = 0
            if it is not None:
                _, tdt, _, vp, vt, stamp, _, _, _ = it
                dt = 2 if tdt == torch.bfloat16 else 1  # DCLIP_BF16 / DCLIP_F16
                cache = it[0]
                # a copy that was stale BEFORE the step stays stale if the step is skipped on the
                # device: only copies valid now are re-stamped (steady state: all of them)
                mine.append((it, vp is not None and cache[(tdt, False)][0] == stamp,
                             vt is not None and cache[(tdt, True)][0] == stamp))
            key.append((w.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if vp is None else vp.data_ptr(),
                        0 if vt is None else vt.data_ptr(), rows, cols, r, dt))
        key = tuple(key)
        if self._desc is None or self._desc[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: the parameters, moments or cached weight copies changed since the last "
                                   "eager optimizer step; run one eager step before capturing the train step")
            table, tiles = [], 0
            for pp, mp, vp_, dp, dtp, rows, cols, r, dt in key:
                tcn = (cols + 63) // 64 if dtp else 0
                table.append([pp, mp, vp_, dp, dtp, rows, cols, tiles, tcn, r, dt, 0])
                tiles += ((rows + 63) // 64) * tcn if tcn else (rows * cols + 4095) // 4096
            host = torch.tensor(table, dtype=torch.int64)
            self._desc = (key, host.to(self._device), host, tiles)
        return self._desc, [e[3] for e in entries], mine, [(e[1], e[1].grad) for e in entries]

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def prepare(self, found_inf=None, check_grads=False):
        """First half of a step: the gradient norm pass (when a group clips, or check_grads) and the
        fold that writes the step's scalars — total norm, clip coefficient, found_inf (the sum of
        squares is not finite, or `found_inf` is non-zero), the bias corrections of the step count
        this step will have.  The next step() applies exactly this prepared step — unless
        zero_grad() ran or a parameter's .grad is another tensor by then: a prepared step that went
        stale is dropped and step() prepares afresh.  Nothing is counted here: the update commits
        the step count, so preparing twice, or without a step(), counts no step.  False when no
        parameter has a gradient."""
        got = self._collect()
        if got is None:
            self._prepared = None
            return False
        desc, grads, copies, live = got
        self._sync_hp()
        from . import ops
        ops.D()
        if found_inf is not None:
            found_inf = found_inf.detach().to(device=self._device, dtype=torch.float32).reshape(1)
        with_norm = bool(check_grads) or any(g.get("max_norm") for g in self.param_groups)
        torch.ops.dclip_optim.adamw_prepare(desc[1], desc[2], grads, desc[3], self._hp, found_inf, self._st, with_norm)
        self._prepared = (desc, grads, copies, live)
        return True

    def zero_grad(self, set_to_none=True):
        self._prepared = None  # a prepared step does not outlive its gradients
        super().zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._prepared is not None and any(p.grad is not g for p, g in self._prepared[3]):
            self._prepared = None  # prepared on gradients that have been replaced since
        if self._prepared is None and not self.prepare(getattr(self, "found_inf", None)):
            self._stepped = None
            return loss
        desc, grads, copies, _ = self._prepared
        self._prepared = None
        torch.ops.dclip_optim.adamw_update(desc[1], desc[2], grads, desc[3], self._st)
        self._stepped = copies
        return loss

    def restamp_weight_copies(self):
        """Called by ops' optimizer-step hook once the parameters carry the new step stamp: the
        copies this step wrote (or, on a skipped step, left equal to their unchanged parameter)
        are valid for the next forward."""
        from . import ops
        for it, plain, transposed in self._stepped or ():
            ops.restamp_weight_copies([it], plain, transposed)
        self._stepped = None

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        sd = super().state_dict()
        if sd["state"]:
            step = self.step_count
            sd["state"] = {i: {"step": step.clone(), **s} for i, s in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        # checked on the incoming dict, before anything of this optimizer changes
        steps = [float(s["step"]) for s in state_dict["state"].values() if "step" in s]
        if steps and min(steps) != max(steps):
            raise ValueError("FusedAdamW.load_state_dict: the per-parameter step counts differ "
                             f"({min(steps):g} .. {max(steps):g}); this optimizer keeps one")
        keep = [g.get("max_norm") for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, mn in zip(self.param_groups, keep):
            g.setdefault("max_norm", mn)
            g["fused"], g["capturable"] = True, True
        for s in self.state.values():
            s.pop("step", None)
        self._buffers()[1][3] = steps[0] if steps else 0.0
        self._hp_host = [None] * len(self.param_groups)
        self._desc = self._prepared = None


def nonfinite_flag(opt, loss, check_grads=True):
    """0-dim f32 on the loss's device: 1 when the loss — or, with check_grads, any gradient the
    optimizer would apply — is NaN / Inf; MAX-reduced over the process group so every rank takes
    the same decision.  The gradient check is one multi-tensor inf-norm pass (no host sync); it
    catches an fp16 overflow in a backward whose loss stayed finite (the neck / heads run on one
    power-of-two gradient scale, ops.HeadScale)."""
    flag = (~torch.isfinite(loss.detach().reshape(-1)[0])).to(torch.float32)
    if isinstance(opt, FusedAdamW):
        # the gradients' finiteness comes from the optimizer's own norm pass (one read of the
        # gradients, shared with the clipping): the loss flag goes in as its external flag, after
        # the MAX-reduction — the gradients are identical on every rank after the all-reduce, so
        # their flag needs no collective.  opt.step() then applies the step prepared here.
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if opt.prepare(found_inf=flag, check_grads=check_grads):
            flag = opt.last_found_inf
        if check_grads:
            from . import ops
            ops.watch_fp16_overflow(flag)
        return flag
    if check_grads:
        grads = [p.grad for g in opt.param_groups for p in g["params"] if p.grad is not None]
        if grads:
            norms = torch._foreach_norm(grads, float("inf"))
            bad = (~torch.isfinite(torch.stack([n.to(flag.device) for n in norms]))).any()
            flag = torch.maximum(flag, bad.to(torch.float32))
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    if check_grads:  # an overflowed fp16 step re-primes the delayed gradient scales (ops.FP16_DELAYED_SCALE)
        from . import ops
        ops.watch_fp16_overflow(flag)
    return flag


def step_unless_nonfinite(opt, loss, check_grads=True):
    """opt.step(), skipped when the loss (or a gradient, check_grads) is NaN / Inf — the reference
    trainer skips such a step (train_denseclip.py:1323; e.g. a batch whose labels are all ignored
    gives a NaN CE).

    Fused torch optimizers take the decision ON THE DEVICE through their `found_inf` input (the
    AdamW kernel leaves parameters, moments and the step count untouched when it is non-zero): no
    host sync.  Non-fused optimizers read the flag on the host.  Either way the flag is
    MAX-reduced over the process group first, so every rank skips together and the replicas stay
    identical (a per-rank host check would let one rank skip while the others step)."""
    flag = nonfinite_flag(opt, loss, check_grads)
    if not all(g.get("fused") for g in opt.param_groups):
        if not bool(flag):
            opt.step()
        return
    opt.found_inf = flag
    try:
        opt.step()
    finally:
        del opt.found_inf


def train_step(model, opt, batch, silog=None, seg_weight=1.0, silog_weight=0.1, seg_loss=None, identity_weight=None,
               depth_loss=None):
    """One step: forward (DenseCLIP.forward train branch), loss, backward (DDP all-reduce
    overlapped with it), AdamW (skipped for a non-finite loss, step_unless_nonfinite).  Returns
    the loss tensor (no host sync)."""
    img, seg, depth, mask = batch
    out = model(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
    loss = loss_fn(out, seg, depth, mask, silog, seg_weight, silog_weight, seg_loss=seg_loss,
                   identity_weight=identity_weight, depth_loss=depth_loss)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    # the gradients are checked too when the backward ran in fp16 (power-of-two scaled casts can
    # overflow there); bf16 / fp32 keep the reference's loss-only rule
    step_unless_nonfinite(opt, loss, check_grads=fp16_backward(model, img))
    return loss.detach()


def train_step_accum(model, opt, micro_batches, silog=None, seg_weight=1.0, silog_weight=0.1, clip_grad_norm=None,
                     seg_loss=None, identity_weight=None, depth_loss=None):
    """One optimizer step on the mean gradient of k = len(micro_batches) micro-batches
    (training.grad_accum_steps, train_denseclip.py:1154, 1314, 1356-1358): zero_grad, then forward /
    loss / backward per micro-batch — every one but the last inside the wrapper's no_sync(), so the
    data-parallel all-reduce runs once, on the accumulated gradients — then one step.
    A torch optimizer gets each loss scaled by 1/k, as the reference does, and, with clip_grad_norm,
    torch.nn.utils.clip_grad_norm_ before the step.  FusedAdamW gets the unscaled sums and applies
    1/k (set_inv_accum) and the clipping (its groups' max_norm, or clip_grad_norm when given)
    inside its kernels; both factors are set for this step and restored after it.  Returns the mean loss (no host sync).

    Departure from the reference: a non-finite micro-batch loss poisons the mean loss and the
    accumulated gradients, and the WHOLE step is then skipped on the device
    (step_unless_nonfinite); the reference skips only that micro-batch's backward, on a host check
    of its loss (train_denseclip.py:1323), and steps on the rest."""
    k = len(micro_batches)
    if k < 1:
        raise ValueError("train_step_accum: at least one micro-batch")
    native = isinstance(opt, FusedAdamW)
    opt.zero_grad(set_to_none=True)
    total = None
    for i, (img, seg, depth, mask) in enumerate(micro_batches):
        hold = i < k - 1 and hasattr(model, "no_sync")
        with (model.no_sync() if hold else contextlib.nullcontext()):
            out = model(img, gt_semantic_seg=seg, gt_depth=depth, return_loss=True)
            loss = loss_fn(out, seg, depth, mask, silog, seg_weight, silog_weight, seg_loss=seg_loss,
                           identity_weight=identity_weight, depth_loss=depth_loss)
            (loss if native else loss / k).backward()
        total = loss.detach() if total is None else total + loss.detach()
    mean = total / k
    if not native:
        if clip_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], clip_grad_norm)
        step_unless_nonfinite(opt, mean, check_grads=fp16_backward(model, img))
        return mean
    # the two factors hold for this step only: a later train_step with the same optimizer sees 1
    # and its own max_norm again (the device table is written when a prepare finds a changed value)
    saved = (opt._inv_accum, [g.get("max_norm") for g in opt.param_groups])
    opt.set_inv_accum(1.0 / k)
    if clip_grad_norm is not None:
        for g in opt.param_groups:
            g["max_norm"] = clip_grad_norm
    try:
        step_unless_nonfinite(opt, mean, check_grads=fp16_backward(model, img))
    finally:
        opt.set_inv_accum(saved[0])
        for g, mn in zip(opt.param_groups, saved[1]):
            g["max_norm"] = mn
    return mean


def trainer_config(cfg):
    """What the reference trainer reads from training.* around the step (train_denseclip.py:1057-1069,
    1154-1155), with its defaults: {'grad_accum_steps', 'clip_grad_norm', 'optimizer' (its kwargs,
    'type' kept), 'scheduler' (the config make_scheduler takes), 'epochs'}."""
    tr = (cfg or {}).get("training", {}) or {}
    epochs = tr.get("epochs")
    sched = dict(tr.get("scheduler") or {"type": "CosineAnnealingLR", "T_max": epochs, "eta_min": 1e-6})
    clip = tr.get("clip_grad_norm", None)
    return {"grad_accum_steps": int(tr.get("grad_accum_steps", 1)),
            "clip_grad_norm": None if clip is None else float(clip),
            "optimizer": dict(tr.get("optimizer") or {"type": "AdamW", "lr": 0.0001, "weight_decay": 0.0001}),
            "scheduler": sched, "epochs": epochs}


def make_scheduler(opt, cfg):
    """The reference's LR scheduler (train_denseclip.py:1066-1083) from a trainer YAML:
    CosineAnnealingLR (T_max defaults to training.epochs), StepLR, or 'poly' = PolynomialLR
    (total_iters defaults to the epochs, power to 0.9); stepped once per epoch.  An unknown type
    raises (the reference warns and trains at a constant rate)."""
    tc = trainer_config(cfg)
    sc = dict(tc["scheduler"])
    kind = str(sc.pop("type", "CosineAnnealingLR")).lower()
    if kind == "cosineannealinglr":
        sc.setdefault("T_max", tc["epochs"])
        return torch.optim.lr_scheduler.CosineAnnealingLR(opt, **sc)
    if kind == "steplr":
        return torch.optim.lr_scheduler.StepLR(opt, **sc)
    if kind == "poly":
        sc.setdefault("total_iters", tc["epochs"])
        sc.setdefault("power", 0.9)
        return torch.optim.lr_scheduler.PolynomialLR(opt, **sc)
    raise ValueError(f"make_scheduler: unknown scheduler type {kind!r} (CosineAnnealingLR, StepLR or poly)")


class CapturedTrainStep:
    """train_step captured once into one HIP graph and replayed: forward, loss, backward, the
    non-finite check and the fused AdamW update (skipped on the device when the flag is set), and
    the refresh of the 16-bit weight copies the next forward reads — every launch of the step
    replayed from one hipGraphLaunch, so the host issues nothing per kernel and the step runs at
    the GPU's pace with the inter-kernel gaps of a graph (ops are stream-ordered and capture-safe:
    outputs from the caching allocator, no host synchronisation; the frozen text path becomes a
    parallel branch of the graph as in serve.CapturedForward).

    Call it with a batch of the captured shapes / dtypes (copied into the static input buffers)
    or with no argument (the same batch again); it returns the step's loss tensor (the SAME
    tensor every call).  Requirements: one process (no DDP: its bucketed all-reduce hooks are not
    captured here), a fused AdamW built with capturable=True (its step counts live on the device),
    and parameters that stay where they are.  An fp16 backward is captured with EXACT gradient
    scales (the delayed scales' use counter is host state, so ops takes exact scales under stream
    capture): its replays equal eager steps run with ops.FP16_DELAYED_SCALE = False bit for bit
    (tests/test_gpu_determinism.py; the step is bitwise reproducible since the fixed-order loss
    folds of ABI 7), and measured slower than the eager delayed-scale step (137.5 vs 135.1 ms,
    DESIGN.md §5), so the bench's fp16 line stays eager.

    FusedAdamW is accepted like a capturable torch AdamW; a learning rate held in a 1-element device
    tensor is read by every replay.  identity_weight: the identity head's term (loss_fn).  accum_steps=k: `batch` is a sequence of k micro-batches and the
    one graph holds k forward / backward passes and one update (train_step_accum)."""

    def __init__(self, model, opt, batch, silog=None, seg_weight=1.0, silog_weight=0.1, warmup=3, accum_steps=1,
                 seg_loss=None, identity_weight=None, depth_loss=None):
        if isinstance(model, (torch.nn.parallel.DistributedDataParallel, GradAllReduce)):
            raise RuntimeError("CapturedTrainStep: one process only (the data-parallel all-reduce hooks are not captured)")
        if not all(g.get("fused") and g.get("capturable") for g in opt.param_groups):
            raise RuntimeError("CapturedTrainStep: needs a fused AdamW with capturable=True "
                               "(make_optimizer(..., capturable=True))")
        self.accum_steps = int(accum_steps)
        if self.accum_steps > 1:
            if len(batch) != self.accum_steps:
                raise ValueError(f"CapturedTrainStep: accum_steps={accum_steps} needs that many micro-batches "
                                 f"(got {len(batch)})")
            if not all(t.is_cuda for mb in batch for t in mb if t is not None):
                raise RuntimeError("CapturedTrainStep: GPU batch tensors only (no CPU fallback)")
            self.micro = [[None if t is None else t.detach().clone() for t in mb] for mb in batch]
            self.static = [t for mb in self.micro for t in mb]
            step_fn, first = train_step_accum, self.micro
        else:
            # a seg-only model's batch has no depth target / mask: (img, seg, None, None)
            if not all(t.is_cuda for t in batch if t is not None):
                raise RuntimeError("CapturedTrainStep: GPU batch tensors only (no CPU fallback)")
            self.static = [None if t is None else t.detach().clone() for t in batch]
            step_fn, first = train_step, self.static
        args = (silog, seg_weight, silog_weight)
        kw = {} if seg_loss is None else {"seg_loss": seg_loss}
        if identity_weight is not None:  # the text path then runs eagerly inside the capture, with autograd
            kw["identity_weight"] = identity_weight
        if depth_loss is not None:  # a losses.DepthLoss in SILog's place (loss_fn); BerHu's c is per micro-batch
            kw["depth_loss"] = depth_loss
        m = _unwrap(model)
        saved = getattr(m, "graph_text", None)
        if saved is not None:
            m.graph_text = "side"  # the text path as a forked branch of this capture (no nested graph)
        try:
            dev = next(t for t in self.static if t is not None).device
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):  # caches, allocator pools, the weight-refresh descriptor
                    step_fn(model, opt, first, *args, **kw)
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.loss = step_fn(model, opt, first, *args, **kw)
        finally:
            if saved is not None:
                m.graph_text = saved

    def __call__(self, batch=None):
        if batch is not None:
            if self.accum_steps > 1:
                batch = [t for mb in batch for t in mb]
            for s, t in zip(self.static, batch):
                if s is None and t is None:
                    continue
                if s is None or t is None:
                    raise ValueError("CapturedTrainStep was captured with other batch entries absent (None)")
                if s.shape != t.shape or s.dtype != t.dtype:
                    raise ValueError(f"CapturedTrainStep was captured for {tuple(s.shape)} {s.dtype}, "
                                     f"got {tuple(t.shape)} {t.dtype}")
                if s.data_ptr() != t.data_ptr():
                    s.copy_(t)
        self.graph.replay()
        return self.loss


def fp16_backward(model, img=None):
    """Whether the model's backward runs in fp16: 16-bit images set the compute dtype themselves
    (CLIPVisionTransformer._cdt), fp32 images use the backbone's compute_dtype."""
    if img is not None and img.dtype in (torch.bfloat16, torch.float16):
        return img.dtype == torch.float16
    bb = getattr(_unwrap(model), "backbone", None)
    return getattr(bb, "compute_dtype", None) == torch.float16


# ---------------------------------------------------------------------------- checkpoints
def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def save_checkpoint(path, model, optimizer, epoch, scheduler=None):
    """The reference trainer's checkpoint (train_denseclip.py:1499-1512): the UNWRAPPED model's
    state dict (no 'module.' prefix), the optimizer's and optionally the scheduler's."""
    state = {"epoch": epoch, "state_dict": _unwrap(model).state_dict(), "optimizer": optimizer.state_dict()}
    if scheduler is not None:
        state["scheduler"] = scheduler.state_dict()
    torch.save(state, path)


def _model_weights(ckpt):
    """Weight dict of a checkpoint as --load reads it (train_denseclip.py:1019-1021): under
    'state_dict', 'model_state_dict' or 'model', or the dict itself; a 'module.' prefix on every
    key (a DDP-saved model) is stripped."""
    for key in ("state_dict", "model_state_dict", "model"):
        if key in ckpt:
            ckpt = ckpt[key]
            break
    if ckpt and all(k.startswith("module.") for k in ckpt):
        ckpt = {k[len("module."):]: v for k, v in ckpt.items()}
    return ckpt


def load_weights(path, model, map_location="cpu"):
    """--load (train_denseclip.py:1012-1024): non-strict load of a checkpoint's model weights;
    returns the load message.  Files are read with weights_only=True; an unreadable file raises
    (the reference logs and continues)."""
    ckpt = torch.load(path, map_location=map_location, weights_only=True)
    return _unwrap(model).load_state_dict(_model_weights(ckpt), strict=False)


def resume(path, model, optimizer=None, scheduler=None, map_location="cpu"):
    """--resume (train_denseclip.py:1107-1133): model, optimizer and scheduler state; returns the
    epoch to start from (saved epoch + 1)."""
    ckpt = torch.load(path, map_location=map_location, weights_only=True)
    if "state_dict" in ckpt:
        _unwrap(model).load_state_dict(_model_weights(ckpt), strict=False)
    if optimizer is not None and "optimizer" in ckpt:
        optimizer.load_state_dict(ckpt["optimizer"])
    if scheduler is not None and "scheduler" in ckpt:
        scheduler.load_state_dict(ckpt["scheduler"])
    return ckpt.get("epoch", -1) + 1
