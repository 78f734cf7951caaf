"""The checker of test_gpu_norm_contract.py before any kernel meets it (norm_check.py):
  * a plain f32 torch emulation of every entry point stays under every bound at every case of the
    GPU test, the delayed-scale families through uses 1 .. 5 of one state (a bound this emulation
    misses would be a wrong bound, not a strict one);
  * the fp64 LayerNorm reference agrees with torch.nn.functional.layer_norm and with autograd, both
    in fp64, to 1e-12, which ties it to PyTorch;
  * the rsqrt allowance is the measured one: torch.rsqrt against fp64, and twice that for the GPU;
  * each planted defect fails the checker, next to what the norm-wise criterion of
    test_gpu_kernels.py (helpers.rel_err under that file's 1e-5) makes of the same output."""
import pytest
import torch
import torch.nn.functional as Fn

import norm_check as NC
from norm_check import BF16, F16, F32, U  # noqa: F401

WORST = {}
OLD_TOL = 1e-5  # test_layernorm_fwd / _bwd / _bwd_res of test_gpu_kernels.py


def find(family, **want):
    hits = [c for c in NC.FAMILIES[family][0]() if all(c[k] == v for k, v in want.items())]
    assert hits, (family, want)
    return hits[0]


def verdict(family, c, inp, outs):
    _, _, _, refs, split = NC.FAMILIES[family]
    return NC.passes(f"planted {family}", refs(c, inp, outs), split(c, outs))


def ref_of(family, c, inp, outs, name):
    return dict((n, r) for n, r, _ in NC.FAMILIES[family][3](c, inp, outs))[name]


def old(what, bad, ref):
    e = NC.old_rel_err(bad, ref)
    print(f"{what}: norm-wise error {e:.2e}, {'passes' if e < OLD_TOL else 'fails'} the old {OLD_TOL:g}")
    return e


def at_use(family, base, use):
    """(case, inputs) of use `use` after the emulation ran the uses before it on one state"""
    _, inputs, emulate, _, _ = NC.FAMILIES[family]
    st = NC.run_sequence(family, base, emulate, uses=range(1, use))
    c = dict(base, use=use)
    inp = inputs(c)
    inp["st"] = st
    return c, inp


@pytest.mark.parametrize("family", list(NC.FAMILIES))
def test_emulation_stays_under_the_bounds(family):
    cases, inputs, emulate, _, _ = NC.FAMILIES[family]
    ids = [NC.norm_case_id(c) for c in cases()]
    assert len(set(ids)) == len(ids), "two cases share an id"
    for c in cases():
        w = WORST.setdefault((family, NC.dtype_key(c)), {})
        if family in NC.SEQUENCES:
            NC.run_sequence(family, c, emulate, w)
        else:
            inp = inputs(c)
            NC.check_case(family, c, inp, emulate(c, inp), w)
    for (fam, key), w in sorted(WORST.items()):
        if fam == family:
            print(f"emulation {fam} {key}: worst figure / bound over its cases: "
                  + ", ".join(f"{n} {v:.3f}" for n, v in sorted(w.items())))
            assert all(v <= 1.0 for v in w.values())


def test_reference_is_layer_norm_and_its_autograd_in_fp64():
    for rows, cols, eps in ((5, 260, 1e-5), (7, 768, 1e-2), (3, 2048, 1e-12)):
        g = NC.gen(rows + cols)
        x = (NC.randn(g, rows, cols).double() + 0.3).requires_grad_(True)
        w = NC.signed_weight(g, cols).double().requires_grad_(True)
        b = NC.randn(g, cols).double().requires_grad_(True)
        dy = NC.randn(g, rows, cols).double()
        eps32 = NC.f32(eps)
        y = Fn.layer_norm(x, (cols,), w, b, eps32)
        y.backward(dy)
        mu, var, r = NC.ln_fwd_stats64(x.detach(), eps)
        yref = (x.detach() - mu) * r * w.detach() + b.detach()
        zero = torch.zeros(cols, dtype=torch.float64)
        dx, _, dw, _, db, _ = NC.bwd_ref(dy, x.detach(), w.detach(), mu[:, 0], r[:, 0], None, None, zero, zero)
        for name, a, ref in (("y", yref, y.detach()), ("dx", dx, x.grad), ("dw", dw, w.grad), ("db", db, b.grad)):
            e = float((a - ref).abs().max() / ref.abs().max())
            print(f"fp64 reference against torch {rows} x {cols} eps {eps:g} {name}: {e:.2e}")
            assert e < 1e-12, (name, e)


def test_rsqrt_allowance_was_measured():
    """torch.rsqrt (f32, CPU) against fp64: the figure norm_check.py records (1.50 u, torch 2.10 for ROCm
    7.0 on x86-64), and the GPU's allowance twice it.  Another build's vector library may round the
    worst argument differently, so the recorded figure is held with RSQRT_CPU_MARGIN = 0.25 u of slack
    and not to the digit; the allowance itself is a constant and moves with no build."""
    g = NC.gen(0)
    v = torch.cat([torch.rand(4_000_000, generator=g) * 3 + 1, torch.logspace(-13, 6, 1_000_000),
                   torch.rand(1_000_000, generator=g) * 1e-4]).float()
    ref = v.double().rsqrt()
    worst = float(((torch.rsqrt(v).double() - ref).abs() / ref).max()) / U
    print(f"torch.rsqrt against fp64: {worst:.3f} u at worst; allowance {NC.RSQRT_U} u")
    assert worst <= NC.RSQRT_CPU_MEASURED + NC.RSQRT_CPU_MARGIN and NC.RSQRT_U == 2 * NC.RSQRT_CPU_MEASURED


# ----------------------------------------------------------------------------- planted defects
def fwd_defect(**defect):
    c = find("ln_fwd", rows=517, cols=4, ydt=F32)
    assert c["eps"] == 1e-5
    inp = NC.ln_fwd_inputs(c)
    good, bad = NC.ln_fwd_emulate(c, inp), NC.ln_fwd_emulate(c, inp, **defect)
    for k in bad:  # the constant and the zero row stay right: the defect is to show on ordinary rows
        bad[k][1:3] = good[k][1:3]
    assert verdict("ln_fwd", c, inp, good)
    assert not verdict("ln_fwd", c, inp, bad)
    return old(f"ln_fwd {defect} y", bad["y"], ref_of("ln_fwd", c, inp, good, "y"))


def test_planted_unbiased_variance():
    assert fwd_defect(unbiased=True) > OLD_TOL  # n = 4: a seventh of every value; no new bound needed


def test_planted_eps_ignored():
    fwd_defect(no_eps=True)


def big_bwd():
    c = find("ln_bwd", rows=4107, cols=768, dsc=True, ntok=5)
    inp = NC.ln_bwd_inputs(c)
    good = NC.ln_bwd_emulate(c, inp)
    assert verdict("ln_bwd", c, inp, good)
    return c, inp, good


def test_planted_row_without_its_mgx_term():
    c, inp, good = big_bwd()
    bad = NC.ln_bwd_emulate(c, inp, drop_mgx_row=4101)
    assert not verdict("ln_bwd", c, inp, bad)
    assert old("one row of dx without mgx", bad["dx"], ref_of("ln_bwd", c, inp, good, "dx")) > OLD_TOL
    # one row of 4107 is 1.6 % of the norm times the row's own error: the old criterion sees a row that
    # is wrong by more than 0.07 %.  A row whose x^ mgx term is 1e-4 of it does not show:
    small = dict(good, dx=good["dx"].clone())
    small["dx"][4101] *= 1 + 1e-4
    assert not verdict("ln_bwd", c, inp, small)
    assert old("one row of dx off by 1e-4", small["dx"], ref_of("ln_bwd", c, inp, good, "dx")) < OLD_TOL


def test_planted_stale_row_at_the_wrap_seam():
    """row 4096, the first of the second walk, holds what the look-ahead registers held: row 4095"""
    c, inp, good = big_bwd()
    bad = dict(good, dx=good["dx"].clone())
    bad["dx"][4096] = good["dx"][4095]
    bad["lp"] = bad["dx"].to(c["lp"])
    assert not verdict("ln_bwd", c, inp, bad)
    old("row 4096 = row 4095", bad["dx"], ref_of("ln_bwd", c, inp, good, "dx"))


def test_planted_dy_ntok_ignored():
    c, inp, good = big_bwd()
    raw = dict(inp, dy=torch.where(torch.isnan(inp["dy"]), torch.ones_like(inp["dy"]), inp["dy"]))
    bad = NC.ln_bwd_emulate(dict(c, ntok=0), raw)
    assert not verdict("ln_bwd", c, inp, bad)
    old("dy_ntok ignored", bad["dx"], ref_of("ln_bwd", c, inp, good, "dx"))


def test_planted_lp_cast_before_res():
    c, inp, good = big_bwd()
    bad = dict(good, lp=(good["dx"] - inp["res"]).to(c["lp"]))
    assert not verdict("ln_bwd", c, inp, bad)
    old("lp before res", bad["lp"].float(), good["lp"].float())


def test_planted_dw_without_the_last_blocks_rows():
    """rows 4104 .. 4106, the ragged 514th group of 8, never reach dw"""
    c, inp, good = big_bwd()
    bad = NC.ln_bwd_emulate(c, inp, dw_rows=slice(0, 4104))
    assert not verdict("ln_bwd", c, inp, bad)
    old("dw without rows 4104 ..", bad["dw"], ref_of("ln_bwd", c, inp, good, "dw"))


def test_planted_dw_overwritten():
    c, inp, good = big_bwd()
    bad = dict(good, dw=good["dw"] - inp["dw0"])
    assert not verdict("ln_bwd", c, inp, bad)
    old("dw overwritten", bad["dw"], ref_of("ln_bwd", c, inp, good, "dw"))


def test_planted_cls_row_of_add_not_zeroed():
    c = find("ln_bwd_add", rows=4107, cols=768)
    inp = NC.fused_inputs(c)
    good = NC.fused_emulate(c, inp)
    assert verdict("ln_bwd_add", c, inp, good)
    # finite values of the size of 2^-12 in the CLS rows: NaN there would fail any criterion
    raw = dict(inp, add=torch.where(torch.isnan(inp["add"].float()), torch.full_like(inp["add"], 2.0 ** -12), inp["add"]))
    bad = NC.fused_emulate(c, raw, keep_cls=True)
    assert not verdict("ln_bwd_add", c, inp, bad)
    assert old("CLS rows of add kept", bad["dx"], ref_of("ln_bwd_add", c, inp, good, "dx")) > OLD_TOL
    one = dict(good, dx=good["dx"].clone())  # a single CLS row, as a last ragged image would leave it
    one["dx"][4100] += 2.0 ** -12
    one["lp"] = one["dx"].to(c["lp"])
    assert not verdict("ln_bwd_add", c, inp, one)
    assert old("one CLS row of add kept", one["dx"], ref_of("ln_bwd_add", c, inp, good, "dx")) < OLD_TOL


def test_planted_scale_of_this_uses_maximum():
    base = find("ln_bwd_scaled", entry="scaled_add", rows=10, cols=768)
    c, inp = at_use("ln_bwd_scaled", base, 2)
    good = NC.fused_emulate(c, inp)
    assert verdict("ln_bwd_scaled", c, inp, good)
    own = 2.0 ** NC.scale_exponent(NC.TARGET, NC.maxbits(good["dx"]))
    assert own != NC.ds_scale(inp["st"], 2)  # use 2's data are 2^6 times use 1's
    assert not verdict("ln_bwd_scaled", c, inp, NC.fused_emulate(c, inp, s=own))
    base = find("readout_scaled", rows=1029)
    c, inp = at_use("readout_scaled", base, 2)
    assert verdict("readout_scaled", c, inp, NC.readout_scaled_emulate(c, inp))
    assert not verdict("readout_scaled", c, inp, NC.readout_scaled_emulate(c, inp, s=own))


def test_planted_next_shards_not_cleared():
    """use 2 clears shards 0, which hold the seed: left alone, use 3 would join its maximum into them"""
    base = find("ln_bwd_scaled", entry="scaled", rows=10, cols=512)
    c, inp = at_use("ln_bwd_scaled", base, 2)
    assert verdict("ln_bwd_scaled", c, inp, NC.fused_emulate(c, inp))
    assert not verdict("ln_bwd_scaled", c, inp, NC.fused_emulate(c, inp, clear=False))


def test_planted_grad_scale_defects():
    c = find("grad_scale", n=1027, place="tail", kind="normal")
    inp = NC.grad_scale_inputs(c)
    assert verdict("grad_scale", c, inp, NC.grad_scale_emulate(c, inp))
    assert not verdict("grad_scale", c, inp, NC.grad_scale_emulate(c, inp, skip_tail=True))
    # 256 / 37.5 = 2^2.77: floor gives 4, round-to-nearest 8, and 37.5 x 8 is past the target
    assert not verdict("grad_scale", c, inp, NC.grad_scale_emulate(c, inp, nearest=True))
