"""train.FusedAdamW (csrc/optim.hip) on the GPU: arithmetic against an fp64 restatement of the
formulas documented in include/dclip.h, the global norm, clipping and accumulation factors, the
16-bit weight copies it writes, the skipped step, determinism, the gradient-pointer hazard, state
dict interchange with torch.optim.AdamW, and the model-level captured / accumulated steps.

Every buffer of the kernel-level tests (parameters, gradients, moments, copies) is a slice of a
guard-banded allocation (abi_guard.py); outputs start poisoned.

Error bounds (eps = 2^-24, the fp32 unit roundoff) come from counting fp32 roundings, not from
observed error.  The fp32 inputs of the restatement are p, g, m, v AND the hyper-parameter table:
lr, 1 - beta1, 1 - beta2, eps, weight decay, max_norm and inv_accum are rounded to fp32 first, as
the device table holds them (the betas as their complements, which keeps 1 - beta2 to fp32 precision).
  g' = g c            c is one fp32 rounding of coef * inv_accum, the product another:   2 eps |g'|
  m                   0.1 x (the above + the subtraction + factor and product) + the final
                      addition:                               < 2 eps (|m| + |g'|)  <=  4 eps (...)
  v                   g'^2: 2 x 2 eps + eps; (1 - beta2): 2 eps; beta2 v: 2 eps; the sum: eps
                                                               <= 8 eps v
  p                   the decay as one fma (p - (lr wd) p) and the final subtraction: 2 eps |p|;
                      sqrt(v): 4 eps + eps, / sqrt(bc2): 2 eps, + eps: eps -> denom to 8 eps;
                      m to 2 eps (|m| + |g'|); the quotient eps; lr / bc1 and the product 3 eps;
                      the subtraction eps:                    15 eps  <=  16 eps (lr/bc1)(|m|+|g'|)/denom
"""
import copy
import math

import numpy as np
import pytest
import torch

import helpers  # noqa: F401  (puts the repository root on sys.path: bench.make_model)
import abi_guard as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = 2.0 ** -24
BF, HF = torch.bfloat16, torch.float16


def f32(x):
    return float(np.float32(x))


# (shape, copies' dtype, plain, transposed, group)
SPECS = [
    ((64, 64), BF, True, True, 0),       # one exact tile
    ((65, 67), HF, True, True, 0),       # ragged both ways, cols % 4 != 0
    ((130, 72), BF, True, True, 0),      # rows % 8 != 0
    ((8, 4, 3, 3), BF, True, False, 0),  # 4-D, plain copy only
    ((19,), None, False, False, 1),
    ((1,), None, False, False, 1),
    ((4097,), None, False, False, 1),    # flat chunks across a boundary
    ((300, 4096), None, False, False, 1),  # 300 norm partials: more than one wave of the fold
]
NOGRAD = ((64, 72), BF, True, True, 0)   # in the optimizer, grad is None
OUTSIDE = ((33, 5), None, False, False, None)  # has a gradient, not in the optimizer
GROUPS = [dict(lr=1e-3, weight_decay=0.01), dict(lr=3e-4, weight_decay=0.1)]
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
B1, B2 = 1 - f32(1 - BETAS[0]), 1 - f32(1 - BETAS[1])  # the betas the device table's complements stand for


def _grad_values(shape, gen):
    """magnitudes log-uniform in [1e-6, 1e2], random signs, ~10 % exact zeros"""
    mag = 10.0 ** (torch.rand(shape, generator=gen, dtype=torch.float64) * 8 - 6)
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    g = (mag * sign).float()
    g[torch.rand(shape, generator=gen) < 0.1] = 0.0
    return g


class ParamSet:
    """The issue's parameter set in guarded buffers, with a FusedAdamW over two groups."""

    def __init__(self, seed=0, max_norm=None, warm=False):
        from denseclip_vit_multimodal_amd import ops
        from denseclip_vit_multimodal_amd.train import FusedAdamW
        gen = torch.Generator().manual_seed(seed)
        self.guards, self.items = [], []
        for spec in SPECS + [NOGRAD, OUTSIDE]:
            shape, dt, plain, transposed, group = spec
            gp = G.guarded_copy(torch.randn(shape, generator=gen).to(DEV))
            p = torch.nn.Parameter(gp.t)
            it = {"spec": spec, "p": p, "group": group, "gp": gp}
            self.guards.append(gp)
            if spec is not NOGRAD:
                it["gg"] = G.guarded_copy(_grad_values(shape, gen).to(DEV))
                p.grad = it["gg"].t
                self.guards.append(it["gg"])
            rows = shape[0]
            cols = p.numel() // rows
            cache = {}
            if plain:
                it["cp"] = G.guarded((rows, cols), dt, fill=G.POISON)
                cache[(dt, False)] = (ops._Cast.stamp(p), it["cp"].t)
                self.guards.append(it["cp"])
            if transposed:
                it["ct"] = G.guarded((cols, rows), dt, fill=G.POISON)
                cache[(dt, True)] = (ops._Cast.stamp(p), it["ct"].t)
                self.guards.append(it["ct"])
            if cache:
                p.__dict__["_dclip_cache"] = cache
            self.items.append(it)
        groups = [dict(params=[it["p"] for it in self.items if it["group"] == k], **GROUPS[k]) for k in (0, 1)]
        self.opt = FusedAdamW(groups, betas=BETAS, eps=ADAM_EPS, max_norm=max_norm)
        for it in self.items:  # the moments in guarded buffers too
            if it["group"] is None or it["spec"] is NOGRAD:
                continue
            shape = it["spec"][0]
            if warm:
                m0 = 0.1 * torch.randn(shape, generator=gen)
                v0 = 0.01 * torch.rand(shape, generator=gen) ** 2
            else:
                m0, v0 = torch.zeros(shape), torch.zeros(shape)
            it["gm"], it["gv"] = G.guarded_copy(m0.to(DEV)), G.guarded_copy(v0.to(DEV))
            self.opt.state[it["p"]]["exp_avg"] = it["gm"].t
            self.opt.state[it["p"]]["exp_avg_sq"] = it["gv"].t
            self.guards += [it["gm"], it["gv"]]
        self.stepped = [it for it in self.items if "gm" in it]

    def snapshot(self):
        return [(it["p"].detach().clone(), it["gg"].t.clone(), it["gm"].t.clone(), it["gv"].t.clone())
                for it in self.stepped]

    def check_guards(self):
        ok = [g.intact() for g in self.guards]
        torch.cuda.synchronize()
        assert all(bool(v) for v in ok), "a guard band was written"

    def check_untouched(self, before):
        for it in self.items:
            if it["spec"] is NOGRAD or it["spec"] is OUTSIDE:
                assert G.bitwise_equal(it["p"].detach(), before[id(it)]), it["spec"][0]
                assert it["p"] not in self.opt.state or "exp_avg" not in self.opt.state[it["p"]]
                for k in ("cp", "ct"):  # its copies were never written
                    if k in it:
                        assert bool((G.bits(it[k].t) == -1).all()), (it["spec"][0], k)


def ref_step(p, g, m, v, lr, wd, c, t, device="cpu"):
    """the documented formulas in fp64 on fp32 inputs (the hyper-parameters rounded to fp32 first)"""
    b1, b2, eps = B1, B2, f32(ADAM_EPS)
    lr, wd = f32(lr), f32(wd)
    p, g, m, v = (x.double().to(device) for x in (p, g, m, v))
    gp = g * c
    p1 = p * (1 - lr * wd)
    m1 = m + (1 - b1) * (gp - m)
    v1 = b2 * v + (1 - b2) * gp * gp
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    p2 = p1 - (lr / bc1) * m1 / denom
    bound_m = 4 * EPS * (m.abs() + gp.abs())
    bound_v = 8 * EPS * v1
    bound_p = 2 * EPS * p.abs() + 16 * EPS * (lr / bc1) * (m.abs() + gp.abs()) / denom
    return p2, m1, v1, bound_p, bound_m, bound_v


def norm64(grads):
    return float(torch.linalg.vector_norm(torch.cat([g.double().reshape(-1).cpu() for g in grads])))


def clip_factor(norm, max_norm, inv_accum):
    """(total_norm, c) in fp64 from the fp32 table values"""
    ia = f32(inv_accum)
    total = norm * ia
    coef = min(1.0, f32(max_norm) / (total + 1e-6)) if max_norm else 1.0
    return total, coef * ia


def check_against_fp64(ps, before, c, t, what=""):
    for it, (p0, g0, m0, v0) in zip(ps.stepped, before):
        k = it["group"]
        p64, m64, v64, bp, bm, bv = ref_step(p0, g0, m0, v0, GROUPS[k]["lr"], GROUPS[k]["weight_decay"], c, t)
        for name, got, ref, bound in (("m", it["gm"].t, m64, bm), ("v", it["gv"].t, v64, bv),
                                      ("p", it["p"].detach(), p64, bp)):
            err = (got.double().cpu() - ref).abs()
            assert bool(torch.isfinite(got).all()), (what, it["spec"][0], name)
            worst = float((err - bound).max())
            assert worst <= 0, (what, it["spec"][0], name, "max error / bound",
                                float((err / bound.clamp_min(1e-300)).max()))
        assert G.bitwise_equal(it["gg"].t, g0), "the gradient was rewritten"


def check_copies(ps):
    for it in ps.stepped:
        shape, dt, plain, transposed, _ = it["spec"]
        w = it["p"].detach()
        if plain:
            assert G.bitwise_equal(it["cp"].t, w.reshape(shape[0], -1).to(dt)), (shape, "plain")
        if transposed:
            assert G.bitwise_equal(it["ct"].t, w.reshape(shape[0], -1).t().contiguous().to(dt)), (shape, "transposed")


CASES = [  # max_norm as a fraction of the gradient norm (None: no clipping), inv_accum, step count
    (None, 1.0, 1), (0.5, 1.0, 1), (2.0, 1.0, 1), (None, 0.25, 1), (0.5, 1.0 / 3, 1), (0.5, 0.25, 1000),
    (None, 1.0, 1000), (2.0, 1.0 / 3, 1000)]


@pytest.mark.parametrize("frac,inv_accum,t", CASES,
                         ids=[f"clip{c[0]}-accum{c[1]:.2f}-t{c[2]}" for c in CASES])
def test_one_step_against_fp64(frac, inv_accum, t):
    probe = ParamSet(seed=1)
    gnorm = norm64([it["gg"].t for it in probe.stepped])  # the same seed gives the same gradients
    max_norm = None if frac is None else frac * gnorm * inv_accum
    ps = ParamSet(seed=1, max_norm=max_norm, warm=t > 1)
    ps.opt.set_inv_accum(inv_accum)
    if t > 1:
        ps.opt.step_count.fill_(t - 1)
    before = ps.snapshot()
    untouched = {id(it): it["p"].detach().clone() for it in ps.items}
    if max_norm is None:
        ps.opt.prepare(check_grads=True)  # the norm pass without clipping
    ps.opt.step()
    total, c = clip_factor(gnorm, max_norm, inv_accum)
    if frac is not None:
        assert (c < f32(inv_accum)) == (frac < 1)  # clipping acts below the norm only
    got = float(ps.opt.last_total_norm)
    assert abs(got - total) <= 2.0 ** -23 * total, (got, total)
    assert float(ps.opt.last_found_inf) == 0 and float(ps.opt.step_count) == t
    check_against_fp64(ps, before, c, t, what=(frac, inv_accum, t))
    check_copies(ps)
    ps.check_untouched(untouched)
    ps.check_guards()


def test_five_step_trajectory_against_fp64_torch_adamw():
    """Five clipped steps with fresh gradients against torch.optim.AdamW + clip_grad_norm_ in fp64
    on the CPU (built with the fp32-rounded hyper-parameters the device table holds): every
    parameter stays within twice the sum of the per-step bounds along the fp64 trajectory."""
    ps = ParamSet(seed=2, max_norm=None)
    gen = torch.Generator().manual_seed(22)
    ref = [torch.nn.Parameter(it["p"].detach().double().cpu()) for it in ps.stepped]
    ropt = torch.optim.AdamW(
        [dict(params=[r for r, it in zip(ref, ps.stepped) if it["group"] == k], lr=f32(GROUPS[k]["lr"]),
              weight_decay=f32(GROUPS[k]["weight_decay"])) for k in (0, 1)],
        betas=(B1, B2), eps=f32(ADAM_EPS))
    budget = [torch.zeros_like(r) for r in ref]
    for t in range(1, 6):
        grads = [_grad_values(it["spec"][0], gen) for it in ps.stepped]
        max_norm = 0.7 * norm64(grads)
        for g in ps.opt.param_groups:
            g["max_norm"] = max_norm
        for it, g, r in zip(ps.stepped, grads, ref):
            it["p"].grad = g.to(DEV)
            r.grad = g.double()
        m_old = [ropt.state[r]["exp_avg"].clone() if t > 1 else torch.zeros_like(r) for r in ref]
        p_old = [r.detach().clone() for r in ref]
        torch.nn.utils.clip_grad_norm_(ref, f32(max_norm))
        ropt.step()
        ps.opt.step()
        for i, (it, r) in enumerate(zip(ps.stepped, ref)):
            k = it["group"]
            lr = f32(GROUPS[k]["lr"])
            denom = ropt.state[r]["exp_avg_sq"].sqrt() / math.sqrt(1 - B2 ** t) + f32(ADAM_EPS)
            budget[i] += 2 * EPS * p_old[i].abs() + 16 * EPS * (lr / (1 - B1 ** t)) * (
                m_old[i].abs() + r.grad.abs()) / denom
    for it, r, b in zip(ps.stepped, ref, budget):
        err = (it["p"].detach().double().cpu() - r.detach()).abs()
        assert float((err - 2 * b).max()) <= 0, (it["spec"][0], float((err / b).max()))
    assert float(ps.opt.step_count) == 5
    ps.check_guards()


def test_copies_are_valid_for_the_next_forward_and_no_refresh_is_launched(monkeypatch):
    from denseclip_vit_multimodal_amd import ops
    D = ops.D()
    real, calls = D.weight_refresh, [0]

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(D, "weight_refresh", counted)
    ps = ParamSet(seed=3)
    ps.opt.step()
    assert calls[0] == 0
    check_copies(ps)
    for it in ps.stepped:
        shape, dt, plain, transposed, _ = it["spec"]
        if plain:  # the stamps are valid: the cache hands back the very tensors the step wrote
            assert ops.WEIGHTS.get(it["p"], dt) is it["cp"].t
        if transposed:
            assert ops.WEIGHTS.get(it["p"], dt, transposed=True) is it["ct"].t
    # the wrapper does count: any other optimizer's step launches the refresh
    sgd = torch.optim.SGD([ps.stepped[0]["p"]], lr=0.1)
    sgd.step()
    assert calls[0] == 1
    check_copies(ps)
    ps.check_guards()


@pytest.mark.parametrize("how", ["inf_gradient", "external_flag"])
def test_skipped_step_writes_nothing(how):
    ps = ParamSet(seed=4, max_norm=1.0, warm=True)
    ps.opt.step_count.fill_(7)
    if how == "inf_gradient":
        ps.stepped[2]["gg"].t[100, 3] = float("inf")
    else:
        ps.opt.found_inf = torch.full((), 2.0, device=DEV)
    before = ps.snapshot()
    copies = [(it[k].t.clone()) for it in ps.stepped for k in ("cp", "ct") if k in it]
    ps.opt.step()
    for it, (p0, g0, m0, v0) in zip(ps.stepped, before):
        assert G.bitwise_equal(it["p"].detach(), p0) and G.bitwise_equal(it["gm"].t, m0)
        assert G.bitwise_equal(it["gv"].t, v0)
    after = [it[k].t for it in ps.stepped for k in ("cp", "ct") if k in it]
    assert all(G.bitwise_equal(a, b) for a, b in zip(after, copies))
    assert float(ps.opt.step_count) == 7 and float(ps.opt.last_found_inf) == 1
    if how == "inf_gradient":
        assert not math.isfinite(float(ps.opt.last_total_norm))
    ps.check_guards()


def _two_steps(sync):
    ps = ParamSet(seed=5, max_norm=3.0)
    gen = torch.Generator().manual_seed(55)
    second = [_grad_values(it["spec"][0], gen).to(DEV) for it in ps.stepped]  # other tensors, other addresses
    torch.cuda.synchronize()
    ps.opt.step()
    if sync:
        torch.cuda.synchronize()
    for it, g in zip(ps.stepped, second):
        assert g.data_ptr() != it["gg"].t.data_ptr()
        it["p"].grad = g
    ps.opt.step()
    if sync:
        torch.cuda.synchronize()
    norm = ps.opt.last_total_norm.clone()
    torch.cuda.synchronize()
    ps.check_guards()
    return [(it["p"].detach().clone(), it["gm"].t.clone(), it["gv"].t.clone()) for it in ps.stepped], norm


def test_deterministic_and_ordered_without_synchronisation():
    """Two runs agree bitwise; two steps issued back to back with fresh gradient tensors and no
    synchronisation equal the same steps with a synchronise after each (the gradient addresses
    travel as launch arguments: the second step cannot disturb the first one's)."""
    a, na = _two_steps(sync=True)
    b, nb = _two_steps(sync=True)
    c, nc = _two_steps(sync=False)
    for x, y, z in zip(a, b, c):
        for i in range(3):
            assert G.bitwise_equal(x[i], y[i]) and G.bitwise_equal(x[i], z[i])
    assert G.bitwise_equal(na, nb) and G.bitwise_equal(na, nc)


def _one_step_bound(p0, g0, m0, v0, k, t):
    return ref_step(p0, g0, m0, v0, GROUPS[k]["lr"], GROUPS[k]["weight_decay"], 1.0, t)[3]


@pytest.mark.parametrize("direction", ["native_to_torch", "torch_to_native"])
def test_state_dict_interchanges_with_torch_adamw(direction):
    from denseclip_vit_multimodal_amd.train import FusedAdamW
    gen = torch.Generator().manual_seed(6)
    shapes = [s[0] for s in SPECS]
    pa = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]

    def groups(ps):
        return [dict(params=ps[:4], **GROUPS[0]), dict(params=ps[4:], **GROUPS[1])]

    native = FusedAdamW(groups(pa if direction == "native_to_torch" else pb), betas=BETAS, eps=ADAM_EPS)
    torch_opt = torch.optim.AdamW(groups(pb if direction == "native_to_torch" else pa), betas=BETAS, eps=ADAM_EPS,
                                  fused=True)
    src, dst = (native, torch_opt) if direction == "native_to_torch" else (torch_opt, native)
    for _ in range(3):
        for p in pa:
            p.grad = _grad_values(p.shape, gen).to(DEV)
        src.step()
    sd = copy.deepcopy(src.state_dict())  # a checkpoint's copy: load_state_dict itself shares the tensors it is given
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 3 and s["step"].dtype == torch.float32
               for s in sd["state"].values())
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    dst.load_state_dict(sd)
    before = [(p.detach().clone(), src.state[p]["exp_avg"].clone(), src.state[p]["exp_avg_sq"].clone()) for p in pa]
    for a, b in zip(pa, pb):
        a.grad = _grad_values(a.shape, gen).to(DEV)
        b.grad = a.grad.clone()
    src.step()
    dst.step()
    assert float(native.step_count) == 4
    for i, (a, b) in enumerate(zip(pa, pb)):
        p0, m0, v0 = before[i]
        bound = _one_step_bound(p0, a.grad, m0, v0, 0 if i < 4 else 1, 4)
        err = (a.detach().double().cpu() - b.detach().double().cpu()).abs()
        assert float((err - bound).max()) <= 0, (shapes[i], float((err / bound.clamp_min(1e-300)).max()))
        assert not torch.equal(a.detach(), p0)
    if direction == "torch_to_native":
        sd["state"][1]["step"] = sd["state"][1]["step"] + 1  # differing per-parameter steps
        m_before = native.state[pb[0]]["exp_avg"]
        with pytest.raises(ValueError, match="step counts differ"):
            native.load_state_dict(sd)
        # refused before anything changed
        assert float(native.step_count) == 4 and native.state[pb[0]]["exp_avg"] is m_before


def test_a_prepared_step_never_goes_stale_or_counts_twice():
    """prepare() alone (train.nonfinite_flag is public) counts no step; preparing twice counts one;
    after zero_grad, or once a parameter's .grad is another tensor, step() prepares afresh and
    applies the NEW gradients."""
    ps = ParamSet(seed=7, max_norm=2.0)
    ps.opt.prepare(check_grads=True)
    ps.opt.prepare(check_grads=True)
    assert float(ps.opt.step_count) == 0
    gen = torch.Generator().manual_seed(77)
    fresh = [_grad_values(it["spec"][0], gen).to(DEV) for it in ps.stepped]
    for it, g in zip(ps.stepped, fresh):  # other tensors with other values, as autograd hands them over
        it["gg"] = G.guarded_copy(g)
        it["p"].grad = it["gg"].t
        ps.guards.append(it["gg"])
    before = ps.snapshot()
    ps.opt.step()
    assert float(ps.opt.step_count) == 1
    total, c = clip_factor(norm64(fresh), 2.0, 1.0)
    assert abs(float(ps.opt.last_total_norm) - total) <= 2.0 ** -23 * total
    check_against_fp64(ps, before, c, 1, what="fresh gradients after a stale prepare")
    ps.opt.prepare()
    ps.opt.zero_grad()
    assert ps.opt._prepared is None
    ps.opt.step()  # no gradients: nothing to do, nothing counted
    assert float(ps.opt.step_count) == 1
    ps.check_guards()


# ---------------------------------------------------------------------------- model level
def _vit(opt_fn):
    import bench
    torch.manual_seed(0)
    m = bench.make_model(DEV, "F").train()
    m.backbone.compute_dtype = torch.bfloat16
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m, opt_fn([p for p in m.parameters() if p.requires_grad])


def _batches(n):
    from denseclip_vit_multimodal_amd.train import synth_batch
    return [synth_batch(2, 256, 512, DEV, r, image_dtype=torch.bfloat16) for r in range(n)]


def _same_params(ma, mb):
    pa = dict(ma.named_parameters())
    diff = [n for n, p in mb.named_parameters() if not torch.equal(p, pa[n])]
    assert not diff, (len(diff), diff[:8])


def test_captured_native_step_equals_eager_and_reads_a_scheduled_lr():
    """ViT-B/16 mode F, bf16, 2 x 256 x 512 (test_gpu_determinism.py's whole-step graph shapes):
    CapturedTrainStep with FusedAdamW replays bit-equal to eager native steps; the learning rate
    lives in a device tensor, and after it is set to 0 the next replay leaves every parameter
    bitwise fixed while the moments move."""
    from denseclip_vit_multimodal_amd.train import CapturedTrainStep, FusedAdamW, train_step
    b1, b2 = _batches(2)
    ma, oa = _vit(lambda ps: FusedAdamW(ps, lr=2e-5, weight_decay=0.01))
    la = [float(train_step(ma, oa, b)) for b in (b1, b1, b1, b2, b1)]
    lr = torch.full((1,), 2e-5, device=DEV)
    mb, ob = _vit(lambda ps: FusedAdamW(ps, lr=lr, weight_decay=0.01))
    cap = CapturedTrainStep(mb, ob, b1)  # three eager warm-up steps on b1
    lb = [float(cap(b2)), float(cap(b1))]
    torch.cuda.synchronize()
    assert lb == la[3:], (lb, la)
    _same_params(ma, mb)
    assert float(ob.step_count) == 5
    # a scheduler writes the tensor: the next replay reads it
    lr.fill_(0.0)
    named = [(n, p) for n, p in mb.named_parameters() if p in ob.state and "exp_avg" in ob.state[p]]
    assert len(named) > 100
    snap = [(p.detach().clone(), ob.state[p]["exp_avg"].clone(), ob.state[p]["exp_avg_sq"].clone()) for _, p in named]
    cap(b2)
    torch.cuda.synchronize()
    moved = 0
    for (n, p), (p0, m0, v0) in zip(named, snap):
        assert torch.equal(p.detach(), p0), n
        moved += int(not torch.equal(ob.state[p]["exp_avg"], m0)) + int(not torch.equal(ob.state[p]["exp_avg_sq"], v0))
    assert moved >= len(named), (moved, len(named))
    assert float(ob.step_count) == 6


def test_captured_accumulation_equals_train_step_accum():
    from denseclip_vit_multimodal_amd.train import CapturedTrainStep, FusedAdamW, train_step_accum
    mbs = _batches(2)
    ma, oa = _vit(lambda ps: FusedAdamW(ps, max_norm=1.0))
    la = [float(train_step_accum(ma, oa, mbs)) for _ in range(5)]
    # the 1/k factor held for those steps only: a plain train_step with this optimizer would see 1
    assert oa._inv_accum == 1.0 and all(g["max_norm"] == 1.0 for g in oa.param_groups)
    mb, ob = _vit(lambda ps: FusedAdamW(ps, max_norm=1.0))
    cap = CapturedTrainStep(mb, ob, mbs, accum_steps=2)  # three eager warm-up steps
    lb = [float(cap()), float(cap(mbs))]
    torch.cuda.synchronize()
    assert lb == la[3:], (lb, la)
    _same_params(ma, mb)
    assert float(ob.step_count) == 5 and float(ob.last_total_norm) > 0


def test_three_native_steps_track_torch_fused_adamw():
    """Three train_steps with FusedAdamW(max_norm=None) against three with make_optimizer().
    Step 1 is the same computation on the same parameters: the losses are equal and so are the
    gradients, so after it every stepped parameter of the native model is held to the counted one-step
    bound against the fp64 restatement (m = v = 0, t = 1, lr 2e-5, weight decay 0.01) and against
    the torch model's — a wrong lr, decay or bias correction is far outside.
    From there the two optimizers' rounding orders differ in the last fp32 bits, and a few bf16
    weight copies by one ulp.  test_gpu_determinism.py compares eager and captured steps for
    equality only, which two rounding orders cannot meet, so the later losses are held to one ulp
    of the compute dtype, 2^-8 relative — and each must have moved from the first loss by more than
    that, so the tolerance cannot hide a step that did nothing."""
    from denseclip_vit_multimodal_amd.train import FusedAdamW, make_optimizer, train_step
    b1, b2 = _batches(2)
    ma, oa = _vit(lambda ps: FusedAdamW(ps, lr=2e-5, weight_decay=0.01, max_norm=None))
    mb, ob = _vit(make_optimizer)
    start = {n: p.detach().clone() for n, p in ma.named_parameters()}
    la, lb = [float(train_step(ma, oa, b1))], [float(train_step(mb, ob, b1))]
    assert la[0] == lb[0]
    pb = dict(mb.named_parameters())
    checked = 0
    for n, p in ma.named_parameters():
        if p.grad is None:
            assert torch.equal(p.detach(), start[n]), n
            continue
        assert torch.equal(p.grad, pb[n].grad), n
        zero = torch.zeros_like(p)
        p64, _, _, bound, _, _ = ref_step(start[n], p.grad, zero, zero, 2e-5, 0.01, 1.0, 1, device=DEV)
        err = (p.detach().double() - p64).abs()
        assert float((err - bound).max()) <= 0, (n, "vs fp64", float((err / bound.clamp_min(1e-300)).max()))
        err = (p.detach().double() - pb[n].detach().double()).abs()
        assert float((err - bound).max()) <= 0, (n, "vs torch", float((err / bound.clamp_min(1e-300)).max()))
        checked += int(not torch.equal(p.detach(), start[n]))
    assert checked > 100  # the step did move the parameters
    la += [float(train_step(ma, oa, b)) for b in (b2, b1)]
    lb += [float(train_step(mb, ob, b)) for b in (b2, b1)]
    print("native", la, "torch", lb)
    for x, y in zip(la[1:], lb[1:]):
        tol = 2.0 ** -8 * abs(y)
        assert abs(x - y) <= tol, (la, lb)
        assert abs(x - la[0]) > tol and abs(y - lb[0]) > tol, (la, lb)
