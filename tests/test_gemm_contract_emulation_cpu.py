"""The bounds of test_gpu_gemm_contract.py hold for a plain emulation of the kernels (gemm_check.emulate:
torch's f32 product of the rounded operands, the epilogue in f32, the outputs rounded to their
dtype) at the small shapes, over five seeds, through the same checker the kernels go through.  A
bound this emulation misses would be a wrong bound, not a strict one."""
import pytest
import torch

import gemm_check as GC

SHAPES = [(65, 72, 64), (257, 264, 128), (300, 200, 192), (264, 256, 768)]
DTS = [torch.float16, torch.bfloat16]
WORST = {}


@pytest.mark.parametrize("form", list(GC.FORMS))
@pytest.mark.parametrize("dt", DTS, ids=["fp16", "bf16"])
def test_emulation_stays_under_the_bounds(dt, form):
    worst = {}
    for si, (M, N, K) in enumerate(SHAPES):
        for seed in range(5):
            case = si + seed + list(GC.FORMS).index(form)
            alpha = 0.5 * 0.25 if case & 1 else 1.0
            o = GC.operands(M, N, K, dt, 100 * si + seed, "cpu")
            bias = o["bias"] if case & 2 else None
            splits = (1, 2, 4)[seed % 3] if form == "splitk" and K % 256 == 0 else 1
            outs = GC.emulate(form, dt, o["A"], o["B"], alpha, bias, o["scale"], o["res"], o["z0"], splits)
            A64, B64 = o["A"].double(), o["B"].double()
            refs = GC.references(form, dt, K, A64 @ B64.t(), A64.abs() @ B64.abs().t(), alpha, bias, o["scale"],
                                 o["res"], o["z0"], outs)
            GC.check(f"emulation {form} {dt} {M}x{N}x{K} seed {seed}", refs, outs, worst)
    WORST[form, dt] = worst
    print(f"emulation {form} {dt}: worst figure / bound over {len(SHAPES)} shapes x 5 seeds: "
          + ", ".join(f"{n} {c} {v:.3f}" for (n, c), v in sorted(worst.items())))
