"""The depth loss as a weighted sum of SILog, L1 and BerHu, everything that needs no GPU: the C ABI's new
symbols and their host checks (which reject before any launch), the two torch ops' schemas, fake kernels and
refusal of CPU tensors, losses.DepthLoss against the written formulas, train.depth_loss_config and
train.loss_fn's materialised path, and that depth_loss=None calls exactly what was called before."""
import ctypes
import os
import re

import pytest
import torch

from helpers import ROOT
from denseclip_vit_multimodal_amd import _native as N

NEW = ["dclip_upsample_depth_loss_ws_floats", "dclip_upsample_depth_stats", "dclip_upsample_depth_finish"]
P = ctypes.c_void_p(0x1000)  # a non-null pointer the host checks never dereference


def test_new_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dclip.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(dclip_\w+)\s*\(", text, re.M))
    lib = N.load()
    for name in NEW:
        assert name in declared and name in N.EXPORTED and hasattr(lib, name), name
    assert lib.dclip_abi_version() == 7
    assert re.search(r"#define DCLIP_DEPTH_SILOG 1\n#define DCLIP_DEPTH_L1 2\n#define DCLIP_DEPTH_BERHU 4", text)
    from denseclip_vit_multimodal_amd import ops
    assert (ops.DEPTH_SILOG, ops.DEPTH_L1, ops.DEPTH_BERHU) == (1, 2, 4)
    assert lib.dclip_upsample_depth_loss_ws_floats.restype is ctypes.c_int64
    # per workgroup 6 f64 records; per band 2 rows of w + chunks - 1 tile columns
    assert lib.dclip_upsample_depth_loss_ws_floats(2, 3, 33) == 2 * 3 * 2 * 12 + 2 * 3 * 2 * 34
    assert lib.dclip_upsample_depth_loss_ws_floats(1, 1, 1) == 12 + 2
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)]:
        assert lib.dclip_upsample_depth_loss_ws_floats(*bad) == 0


def _stats(L, low_dt=0, pred=P, B=1, h=4, w=8, target=P, mask=P, H=64, W=128, eps=1e-6, terms=7, stats=P, ws=P):
    return L.dclip_upsample_depth_stats(low_dt, pred, B, h, w, target, mask, H, W, eps, terms, stats, ws, None)


def _finish(L, low_dt=0, pred=P, B=1, h=4, w=8, target=P, mask=P, H=64, W=128, eps=1e-6, lambd=0.5, terms=7, w_s=1.0,
            w_1=0.5, w_b=0.25, theta=0.2, stats=P, bsum=P, grad=P, ws=P):
    return L.dclip_upsample_depth_finish(low_dt, pred, B, h, w, target, mask, H, W, eps, lambd, terms, w_s, w_1, w_b,
                                         theta, stats, bsum, grad, ws, None)


INF, NAN = float("inf"), float("nan")
HOST_CHECKS = {
    "stats_h0": (lambda L: _stats(L, h=0), "bad sizes"),
    "stats_W_negative": (lambda L: _stats(L, W=-1), "bad sizes"),
    "stats_dtype": (lambda L: _stats(L, low_dt=7), "low_dt=7"),
    "stats_2^31": (lambda L: _stats(L, B=8, H=16384, W=16384), "below 2^31"),
    "stats_terms0": (lambda L: _stats(L, terms=0), "terms=0"),
    "stats_terms8": (lambda L: _stats(L, terms=8), "terms=8"),
    "stats_null_pred": (lambda L: _stats(L, pred=None), "missing buffers"),
    "stats_null_target": (lambda L: _stats(L, target=None), "missing buffers"),
    "stats_null_stats": (lambda L: _stats(L, stats=None), "missing buffers"),
    "stats_null_ws": (lambda L: _stats(L, ws=None), "ws"),
    "stats_misaligned_ws": (lambda L: _stats(L, ws=ctypes.c_void_p(0x1004)), "ws"),
    "finish_B0": (lambda L: _finish(L, B=0), "bad sizes"),
    "finish_dtype": (lambda L: _finish(L, low_dt=3), "low_dt=3"),
    "finish_terms0": (lambda L: _finish(L, terms=0), "terms=0"),
    "finish_silog_not_built": (lambda L: _finish(L, terms=6), "not built for"),
    "finish_l1_not_built": (lambda L: _finish(L, terms=5), "not built for"),
    "finish_berhu_not_built": (lambda L: _finish(L, terms=3), "not built for"),
    "finish_weight_negative": (lambda L: _finish(L, w_1=-0.5), "finite and >= 0"),
    "finish_weight_inf": (lambda L: _finish(L, w_s=INF), "finite and >= 0"),
    "finish_weight_nan": (lambda L: _finish(L, w_b=NAN), "finite and >= 0"),
    "finish_all_zero": (lambda L: _finish(L, w_s=0.0, w_1=0.0, w_b=0.0, bsum=None), "every weight is zero"),
    "finish_theta0": (lambda L: _finish(L, theta=0.0), "0 < threshold <= 1"),
    "finish_theta_above_1": (lambda L: _finish(L, theta=1.5), "0 < threshold <= 1"),
    "finish_theta_nan": (lambda L: _finish(L, theta=NAN), "0 < threshold <= 1"),
    "finish_null_target": (lambda L: _finish(L, target=None), "missing buffers"),
    "finish_null_stats": (lambda L: _finish(L, stats=None), "missing buffers"),
    "finish_berhu_without_sum": (lambda L: _finish(L, bsum=None), "berhu_sum"),
    "finish_sum_without_berhu": (lambda L: _finish(L, w_b=0.0), "berhu_sum"),
    "finish_nothing_to_write": (lambda L: _finish(L, w_b=0.0, bsum=None, grad=None), "nothing to write"),
    "finish_null_ws": (lambda L: _finish(L, ws=None), "ws"),
    "finish_misaligned_ws": (lambda L: _finish(L, ws=ctypes.c_void_p(0x1004)), "ws"),
}


@pytest.mark.parametrize("name", list(HOST_CHECKS))
def test_host_checks_reject_before_any_launch(name):
    call, needle = HOST_CHECKS[name]
    L = N.load()
    assert call(L) == -1
    assert needle in L.dclip_last_error().decode(), L.dclip_last_error().decode()


@pytest.fixture(scope="module")
def loaded():
    from denseclip_vit_multimodal_amd import _torch_ops
    _torch_ops.load()
    return torch.ops


def test_ops_registered_with_fakes(loaded):
    from torch._subclasses.fake_tensor import FakeTensorMode
    st, fin = loaded.dclip_loss.upsample_depth_stats, loaded.dclip_loss.upsample_depth_finish
    assert [str(r.type) for r in st.default._schema.returns] == ["Tensor"]
    assert [str(r.type) for r in fin.default._schema.returns] == ["Tensor", "Optional[Tensor]"]
    assert [a.name for a in fin.default._schema.arguments] == [
        "pred", "target", "mask", "stats", "eps", "lambd", "terms", "w_silog", "w_l1", "w_berhu", "threshold",
        "want_grad"]
    with FakeTensorMode():
        pred = torch.empty(2, 1, 8, 16, device="cuda", dtype=torch.bfloat16)
        tg = torch.empty(2, 128, 256, device="cuda")
        mk = torch.empty(2, 128, 256, device="cuda", dtype=torch.uint8)
        s = st(pred, tg, mk, 1e-6, 7)
        assert s.shape == (6,) and s.dtype == torch.float64 and s.device.type == "cuda"
        b, g = fin(pred, tg, None, s, 1e-6, 0.5, 7, 1.0, 0.5, 0.25, 0.2, True)
        assert b.shape == (1,) and b.dtype == torch.float64
        assert g.shape == pred.shape and g.dtype == torch.float32 and g.device.type == "cuda"
        b, g = fin(pred, tg, mk, s, 1e-6, 0.5, 7, 1.0, 0.5, 0.25, 0.2, False)
        assert g is None and b.shape == (1,)


def test_cpu_tensors_are_refused(loaded):
    pred, tg = torch.rand(1, 1, 4, 4), torch.rand(1, 8, 8)
    with pytest.raises(NotImplementedError, match="CPU"):
        loaded.dclip_loss.upsample_depth_stats(pred, tg, None, 1e-6, 7)
    with pytest.raises(NotImplementedError, match="CPU"):
        loaded.dclip_loss.upsample_depth_finish(pred, tg, None, torch.zeros(6, dtype=torch.float64), 1e-6, 0.5, 7, 1.0,
                                                0.5, 0.25, 0.2, True)
    from denseclip_vit_multimodal_amd import ops
    from denseclip_vit_multimodal_amd.losses import BerHuLoss
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.upsample_depth_loss(pred, tg, l1=1.0)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        BerHuLoss().fused(pred, tg)


def test_argument_checks_and_silog_alone_is_todays_function(monkeypatch):
    from denseclip_vit_multimodal_amd import ops
    pred, tg = torch.rand(1, 1, 4, 4), torch.rand(1, 8, 8)
    for kw, needle in ((dict(silog=-1.0), "weights"), (dict(silog=0.0), "weights"), (dict(l1=float("inf")), "weights"),
                       (dict(berhu=float("nan")), "weights"), (dict(berhu=1.0, berhu_threshold=0.0), "berhu_threshold"),
                       (dict(berhu_threshold=1.01), "berhu_threshold")):
        with pytest.raises(ValueError, match=needle):
            ops.upsample_depth_loss(pred, tg, **kw)
    calls = []

    class Spy:
        @staticmethod
        def apply(*a):
            calls.append(a)
            return torch.tensor(2.0)

    monkeypatch.setattr(ops, "UpsampleSILogFn", Spy)
    monkeypatch.setattr(ops, "UpsampleDepthLossFn", None)  # any use of it would raise
    assert float(ops.upsample_depth_loss(pred, tg, None, silog=0.5, lambd=0.85, eps=1e-3)) == 1.0
    assert float(ops.upsample_depth_loss(pred, tg)) == 2.0
    assert [c[1:] for c in calls] == [(tg, None, 0.85, 1e-3), (tg, None, 0.5, 1e-6)] and calls[0][0] is pred


# ----------------------------------------------------------------------------- losses.DepthLoss
def _data(seed=0, n=(2, 1, 9, 11)):
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(n, generator=g, dtype=torch.float64) * 60 - 5)
    t = 1 + 79 * torch.rand(n, generator=g, dtype=torch.float64)
    m = torch.rand(n, generator=g) < 0.7
    return p, t, m


def _formulas(p, t, m, w, lambd, eps, theta):
    """the issue's definitions, literally, with the hand-written gradient"""
    M = torch.ones_like(p, dtype=torch.bool) if m is None else m
    T = float(M.sum())
    r = torch.where(M, p - torch.where(M, t, torch.zeros_like(t)), torch.zeros_like(p))
    e = r.abs()
    d = torch.where(M, torch.log(p.clamp(min=eps)) - torch.log(torch.where(M, t, torch.ones_like(t)).clamp(min=eps)),
                    torch.zeros_like(p))
    S0, S1 = d.sum(), (d * d).sum()
    c = theta * float(e[M].max())
    b = torch.where(e <= c, e, (e * e + c * c) / (2 * c))
    loss = w[0] * (S1 / T - lambd * S0 ** 2 / T ** 2) + w[1] * e.sum() / T + w[2] * b.sum() / T
    gs = torch.where(M & (p >= eps), (2 * d / T - 2 * lambd * S0 / T ** 2) / p, torch.zeros_like(p))
    g1 = torch.sign(r) / T
    gb = torch.where(e <= c, torch.sign(r) / T, r / (c * T))
    return float(loss), torch.where(M, w[0] * gs + w[1] * g1 + w[2] * gb, torch.zeros_like(p))


@pytest.mark.parametrize("w,theta", [((0.0, 1.0, 0.0), 0.2), ((0.0, 0.0, 1.0), 0.2), ((0.0, 0.0, 1.0), 0.9),
                                     ((1.0, 0.5, 0.25), 0.2)])
@pytest.mark.parametrize("masked", [True, False])
def test_depth_loss_forward_is_the_written_formulas(w, theta, masked):
    from denseclip_vit_multimodal_amd.losses import DepthLoss
    p, t, m = _data()
    m = m if masked else None
    if masked:
        t[~m] = float("nan")  # masked-out targets may hold anything
    p[0, 0, 0, 0] = t[0, 0, 0, 0] if not masked or bool(m[0, 0, 0, 0]) else p[0, 0, 0, 0]  # r = 0: sign(0) = 0
    lref, gref = _formulas(p, t, m, w, 0.5, 1e-6, theta)
    x = p.clone().requires_grad_(True)
    loss = DepthLoss(*w, lambd=0.5, eps=1e-6, berhu_threshold=theta)(x, t, m)
    loss.backward()
    assert abs(float(loss.detach()) - lref) <= 1e-12 * abs(lref)
    assert float((x.grad - gref).abs().max()) <= 1e-12 * float(gref.abs().max())
    # a (B, H, W) mask against a (B, 1, H, W) prediction, as SILogLoss takes it; a u8 mask with bytes other than 1
    if masked:
        again = DepthLoss(*w, berhu_threshold=theta)(p, t, (m[:, 0].to(torch.uint8) * 255))
        assert float(again) == float(loss.detach())


def test_depth_loss_classes_empty_mask_and_errors():
    from denseclip_vit_multimodal_amd.losses import BerHuLoss, DepthLoss, L1DepthLoss, SILogLoss
    p, t, m = _data(1)
    none = torch.zeros_like(m)
    for mod in (L1DepthLoss(), BerHuLoss(), BerHuLoss(0.9), DepthLoss(1.0, 0.5, 0.25), DepthLoss()):
        x = p.clone().requires_grad_(True)
        loss = mod(x, torch.full_like(t, float("nan")), none)
        assert float(loss.detach()) == 0.0
        loss.backward()
        assert bool((x.grad == 0).all())
    assert float(L1DepthLoss()(p, t, m)) == float(DepthLoss(0.0, 1.0, 0.0)(p, t, m))
    assert float(BerHuLoss(0.9)(p, t, m)) == float(DepthLoss(0.0, 0.0, 1.0, berhu_threshold=0.9)(p, t, m))
    assert float(DepthLoss(lambd=0.85, eps=1e-3)(p, t, m)) == float(SILogLoss(0.85, 1e-3)(p, t, m))
    # a NaN under the mask reaches every term, as the kernels' sums keep it
    t2 = t.clone()
    t2[m.nonzero()[3].unbind()] = float("nan")
    for mod in (L1DepthLoss(), BerHuLoss(), DepthLoss()):
        assert bool(torch.isnan(mod(p, t2, m)))
    for kw in (dict(silog=0.0), dict(l1=-1.0), dict(berhu=float("inf")), dict(berhu_threshold=0.0),
               dict(berhu_threshold=1.5)):
        with pytest.raises(ValueError):
            DepthLoss(**kw)
    with pytest.raises(ValueError, match="Mask shape"):
        L1DepthLoss()(p, t, m[0, 0])


# ----------------------------------------------------------------------------- train
def test_depth_loss_config():
    from denseclip_vit_multimodal_amd.losses import DepthLoss
    from denseclip_vit_multimodal_amd.train import depth_loss_config
    assert depth_loss_config(None) is None and depth_loss_config({"training": {"silog_loss": {"eps": 1e-3}}}) is None
    for kind, want in (("silog", (1.0, 0.0, 0.0)), ("l1", (0.0, 1.0, 0.0)), ("BerHu", (0.0, 0.0, 1.0))):
        dl = depth_loss_config({"training": {"depth_loss": {"type": kind}}})
        assert isinstance(dl, DepthLoss) and (dl.silog, dl.l1, dl.berhu) == want
        assert (dl.lambd, dl.eps, dl.berhu_threshold) == (0.5, 1e-6, 0.2)
    dl = depth_loss_config({"training": {"silog_loss": {"lambda": 0.85, "eps": 1e-3},
                                         "depth_loss": {"terms": {"silog": 1.0, "berhu": 0.5}, "berhu_threshold": 0.3}}})
    assert (dl.silog, dl.l1, dl.berhu, dl.lambd, dl.eps, dl.berhu_threshold) == (1.0, 0.0, 0.5, 0.85, 1e-3, 0.3)
    for bad, needle in (({"type": "huber"}, "type"), ({"type": "l1", "terms": {"l1": 1.0}}, "either"), ({}, "either"),
                        ({"terms": {}}, "terms"), ({"terms": {"l2": 1.0}}, "terms"),
                        ({"terms": {"l1": -1.0}}, "negative"), ({"terms": {"l1": float("nan")}}, "not finite"),
                        ({"terms": {"l1": 0.0, "berhu": 0.0}}, "zero"),
                        ({"type": "berhu", "berhu_threshold": 0.0}, "berhu_threshold"),
                        ({"type": "berhu", "berhu_threshold": 1.2}, "berhu_threshold"),
                        ({"type": "l1", "threshold": 0.2}, "unknown keys"), ("l1", "either")):
        with pytest.raises(ValueError, match=needle):
            depth_loss_config({"training": {"depth_loss": bad}})


def test_loss_fn_materialised_path_and_none_is_todays_call(monkeypatch):
    import torch.nn.functional as F
    from denseclip_vit_multimodal_amd import ops, train
    from denseclip_vit_multimodal_amd.losses import DepthLoss, SILogLoss
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 19, 9, 11, generator=g)
    seg = torch.randint(0, 19, (2, 9, 11), generator=g)
    p, t, m = (v.float() if v.dtype == torch.float64 else v for v in _data(2))
    dl = DepthLoss(1.0, 0.5, 0.25, lambd=0.85, eps=1e-3, berhu_threshold=0.3)
    out = {"main_output": logits, "depth_output": p}
    ce = F.cross_entropy(logits, seg, ignore_index=255)
    got = train.loss_fn(out, seg, t, m, seg_weight=0.7, silog_weight=0.3, depth_loss=dl)
    assert float(got) == float(0.7 * ce + 0.3 * dl(p, t, m))
    # None: SILog, as before
    assert float(train.loss_fn(out, seg, t, m, silog_weight=0.3)) == float(1.0 * ce + 0.3 * SILogLoss()(p, t, m))
    # the fused branch: None applies ops.UpsampleSILogFn with today's arguments and nothing else; a DepthLoss goes
    # through its fused(), the whole of it times silog_weight
    calls = []

    class Spy:
        @staticmethod
        def apply(*a):
            calls.append(a)
            return torch.tensor(2.0)

    monkeypatch.setattr(ops, "UpsampleSILogFn", Spy)
    monkeypatch.setattr(ops, "UpsampleCEFn", type("CE", (), {"apply": staticmethod(lambda *a: torch.tensor(10.0))}))
    monkeypatch.setattr(ops, "UpsampleDepthLossFn", None)
    monkeypatch.setattr(ops, "upsample_depth_loss", None)
    low = {"main_output_lowres": logits, "depth_output_lowres": p}
    sil = SILogLoss(0.85, 1e-3)
    assert float(train.loss_fn(low, seg, t, m, silog=sil, silog_weight=0.5)) == 10.0 + 0.5 * 2.0
    assert float(train.loss_fn(low, seg, t, m, silog=sil, silog_weight=0.5, depth_loss=None)) == 11.0
    assert len(calls) == 2 and all(c[0] is p and c[1] is t and c[2] is m and c[3:] == (0.85, 1e-3) for c in calls)
    seen = []
    monkeypatch.setattr(dl, "fused", lambda *a: (seen.append(a), torch.tensor(4.0))[1])
    assert float(train.loss_fn(low, seg, t, m, silog_weight=0.5, depth_loss=dl)) == 10.0 + 0.5 * 4.0
    assert len(calls) == 2 and len(seen) == 1 and seen[0][0] is p and seen[0][1] is t and seen[0][2] is m
    for fn in (train.train_step, train.train_step_accum, train.CapturedTrainStep.__init__):
        import inspect
        assert inspect.signature(fn).parameters["depth_loss"].default is None
