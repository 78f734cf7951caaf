"""The checker of test_gpu_misc_contract.py before any kernel meets it (misc_check.py):
  * a plain f32 torch emulation of every entry point stays under every bound at every case of the
    GPU test (a bound this emulation misses would be a wrong bound, not a strict one);
  * the resize reference (interpolation matrices from f32 weights, product in fp64) reproduces
    F.interpolate(bilinear, align_corners=False) on the CPU within the forward bound at every
    geometry in use, which ties it to PyTorch;
  * one planted defect per op family fails the checker, next to what the norm-wise criterion of
    test_gpu_kernels.py (helpers.rel_err under that file's tolerance) makes of the same output."""
import pytest
import torch
import torch.nn.functional as Fn

import misc_check as MC
from misc_check import BF16, F16, F32, U  # noqa: F401

WORST = {}


def find(family, **want):
    hits = [c for c in MC.FAMILIES[family][0]() if all(c[k] == v for k, v in want.items())]
    assert hits, (family, want)
    return hits[0]


def emulated(family, c):
    _, inputs, emulate, refs, split = MC.FAMILIES[family]
    inp = inputs(c)
    outs = emulate(c, inp)
    return inp, outs


def verdict(family, c, inp, outs):
    _, _, _, refs, split = MC.FAMILIES[family]
    return MC.passes(f"planted {family}", refs(c, inp, outs), split(c, outs))


@pytest.mark.parametrize("family", list(MC.FAMILIES))
def test_emulation_stays_under_the_bounds(family):
    cases = MC.FAMILIES[family][0]()
    ids = [MC.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids), "two cases share an id"
    for c in cases:
        inp, outs = emulated(family, c)
        MC.check_case(family, c, inp, outs, WORST.setdefault((family, MC.dtype_key(c)), {}))
    for (fam, key), w in sorted(WORST.items()):
        if fam == family:
            print(f"emulation {fam} {key}: worst figure / bound over its cases: "
                  + ", ".join(f"{n} {v:.3f}" for n, v in sorted(w.items())))
            assert all(v <= 1.0 for v in w.values())


def resize_geometries():
    geo = {(i, o) for i, o in MC.GEOMETRIES} | {((64, 64), (1, 1))}
    geo |= {((c["g"], c["g"]), (c["H"], c["W"])) for c in MC.pos_interp_cases()}
    geo |= {((c["hs"], c["ws"]), (c["h"], c["w"])) for c in MC.score_concat_cases()}
    return sorted(geo)


def test_matrix_form_reproduces_interpolate():
    """ref = Wy X Wx^T from the f32 weights against torch's own CPU kernel, under the forward bound"""
    worst = 0.0
    for (i, o) in resize_geometries():
        x = MC.randn(MC.gen(3 + i[0] + 5 * o[1]), 3, *i)
        y = Fn.interpolate(x[None], size=o, mode="bilinear", align_corners=False)[0]
        ref, absacc = MC.resize_ref(x, *o)
        r, where = MC.ratio(y, ref, MC.eps_of(F32) * ref.abs() + (4 + 4) * U * absacc)
        print(f"interpolate {i} -> {o}: worst |y - ref| / bound {r:.3f} at {where}")
        worst = max(worst, r)
    assert worst <= 1.0, worst


def test_source_index_is_one_fused_multiply_add():
    """with the product scale (dst + .5) rounded on its own, the f32 source index differs at a fifth
    of the columns of 5 -> 1028 and torch's kernel is outside the bound: the reference fuses it"""
    i, o = (3, 5), (7, 1028)
    assert int((MC.lerp(5, 1028)[3] != MC.lerp(5, 1028, fused=False)[3]).sum()) == 221
    x = MC.randn(MC.gen(3 + i[0] + 5 * o[1]), 3, *i).double()
    y = Fn.interpolate(x.float()[None], size=o, mode="bilinear", align_corners=False)[0]
    Wy, Wx = MC.lerp_matrix(3, 7, fused=False), MC.lerp_matrix(5, 1028, fused=False)
    ref, absacc = Wy @ x @ Wx.t(), Wy.abs() @ x.abs() @ Wx.abs().t()
    r, _ = MC.ratio(y, ref, MC.eps_of(F32) * ref.abs() + (4 + 4) * U * absacc)
    print(f"interpolate {i} -> {o} against unfused weights: worst |y - ref| / bound {r:.3f}")
    assert r > 1.0


def test_fp64_weights_are_not_the_reference():
    """the f32 source index of a 583 -> 2047 resize is up to half an ulp of ~583 from the exact one,
    50 times the 8 u of the forward bound and more: the reference has to use the f32 weights"""
    n_in, n_out = 583, 2047
    dst = torch.arange(n_out, dtype=torch.float64)
    src = ((n_in / n_out) * (dst + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    l1 = src - i0
    exact = torch.zeros(n_out, n_in, dtype=torch.float64)
    exact.index_put_((torch.arange(n_out), i0), 1 - l1, accumulate=True)
    exact.index_put_((torch.arange(n_out), (i0 + 1).clamp(max=n_in - 1)), l1, accumulate=True)
    diff = float((MC.lerp_matrix(n_in, n_out) - exact).abs().max())
    print(f"f32 against fp64 weights at {n_in} -> {n_out}: {diff:.3e}")
    assert diff > 50 * 8 * U


# ----------------------------------------------------------------------------- planted defects
def test_planted_row_left_at_its_entry_value():
    """one pixel of dclip_score_map never written: it keeps the 0x3C fill (0.0115 as f32)"""
    c = find("score_map", HW=33, dt=BF16, token=False)
    inp, outs = emulated("score_map", c)
    assert verdict("score_map", c, inp, outs)
    bad = outs["score"].clone()
    bad[1, :, 32] = torch.tensor([0x3C3C3C3C], dtype=torch.int32).view(F32)
    assert not verdict("score_map", c, inp, {"score": bad})
    # The old criterion (rel_err < 4e-3 at bf16) sees this by value too, one pixel being 1 / 66 of the
    # map: it missed such a row only because the allocator handed back the previous, correct result,
    # which the poisoned buffers address, not a bound.
    ref = MC.score_map_refs(c, inp, outs)[0][1]
    assert MC.old_rel_err(bad, ref) > 4e-3


def test_planted_swapped_lerp_weights_at_one_column():
    c = find("bilinear_fwd", i=(3, 5), o=(7, 1028), NC=3, idt=F32)
    inp, outs = emulated("bilinear_fwd", c)
    assert verdict("bilinear_fwd", c, inp, outs)
    x, j = inp["x"], 517
    y0, y1, ly0, ly1 = MC.lerp(3, 7)
    x0, x1, lx0, lx1 = MC.lerp(5, 1028)
    assert x0[j] != x1[j] and lx0[j] != lx1[j]
    top = lx1[j] * x[:, y0, x0[j]] + lx0[j] * x[:, y0, x1[j]]
    bot = lx1[j] * x[:, y1, x0[j]] + lx0[j] * x[:, y1, x1[j]]
    bad = outs["out"].clone()
    bad[:, :, j] = ly0 * top + ly1 * bot
    assert not verdict("bilinear_fwd", c, inp, {"out": bad})
    # one of 1028 columns is 3 % of the norm: the old 1e-6 sees it as well; this case needs no new bound
    assert MC.old_rel_err(bad, MC.bilinear_fwd_refs(c, inp, outs)[0][1]) > 1e-6


def test_planted_biased_running_var():
    c = find("bn", rows=37, dt=BF16, relu=0, null=False)
    inp = MC.bn_inputs(c)
    good, bad = MC.bn_emulate(c, inp), MC.bn_emulate(c, inp, biased_running_var=True)
    assert verdict("bn", c, inp, good)
    assert not torch.equal(good["rv"], bad["rv"])
    assert not verdict("bn", c, inp, bad)
    ref = dict((n, r) for n, r, _ in MC.bn_refs(c, inp, good))["rv"]
    old = MC.old_rel_err(bad["rv"], ref)
    print(f"biased running_var: norm-wise error {old:.2e}")
    assert old < 1e-2  # the tolerance of test_bn_rows_*: momentum / rows of the variance passes it


def test_planted_class_embedding_not_normalised():
    c = find("score_map", HW=31, dt=F16, token=False)
    inp, outs = emulated("score_map", c)
    assert verdict("score_map", c, inp, outs)
    bad = MC.score_map_emulate(c, inp, raw_class=5)
    assert not verdict("score_map", c, inp, bad)
    # |t| = sqrt(512): that class is 22 times too large and the old 1e-3 fails as well; no new bound needed
    assert MC.old_rel_err(bad["score"], MC.score_map_refs(c, inp, outs)[0][1]) > 1e-3


def test_planted_cls_row_not_skipped():
    """row_off off by one: the mean over the CLS row and all pixel rows but the last"""
    c = find("row_mean", rows=127, dt=BF16, token=True)
    inp, outs = emulated("row_mean", c)
    assert verdict("row_mean", c, inp, outs)
    cls = MC.randn(MC.gen(5), c["B"], 1, c["C"]).to(BF16)
    shifted = torch.cat([cls, inp["x"][:, :-1]], 1)
    bad = {"out": shifted.float().sum(1) / c["rows"]}
    assert not verdict("row_mean", c, inp, bad)
    # two rows of 127 differ: 1 % of the mean, above the old 1e-5 too; no new bound needed
    assert MC.old_rel_err(bad["out"], MC.row_mean_refs(c, inp, outs)[0][1]) > 1e-5


def test_planted_dw_channel_off_by_1e_3():
    c = find("bn", rows=37, dt=F16, relu=0, null=False)
    inp = MC.bn_inputs(c)
    outs = MC.bn_emulate(c, inp)
    assert verdict("bn", c, inp, outs)
    items = dict((n, (r, b)) for n, r, b in MC.bn_refs(c, inp, outs))
    ref, bound = items["dw"]
    ch = int((ref.abs() / bound).argmax())
    bad = dict(outs, dw=outs["dw"].clone())
    bad["dw"][ch] *= 1 + 1e-3
    assert not verdict("bn", c, inp, bad)
    old = MC.old_rel_err(bad["dw"], ref)
    print(f"dw channel {ch} off by 1e-3: norm-wise error {old:.2e}")
    assert old < 1e-2  # test_bn_rows_fused_relu's tolerance: one channel of 768 passes
