"""The persistent one-pass attention-backward sweep (DCLIP_OPT_ATTN_BWD_BLOCK 0: at most one
workgroup per CU walks the tiles and, at each seam, reduces its share of the dQ partials of the
(image, head) it walked a round earlier; a completion pass reduces the rest) against the launch it
replaces (option 10: a workgroup per tile, the whole reduction in its own pass).  The arithmetic is
the same, so the whole dQKV is BIT FOR BIT equal, whatever a seam found complete.

DCLIP_OPT_ATTN_BWD_WGS caps the workgroup count so that these small shapes walk several rounds.  The
workspace is pre-filled with NaN bytes: the seam state (done[B*H] counters, then reduced[B*H][nrb]
flags, nrb = ceil((N-1)/32), at the workspace's start) is zeroed by every call itself."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LEGACY = 10
CASES = [  # B, H, N, cap
    (3, 2, 513, 4),    # 12 tiles, 3 rounds
    (2, 3, 803, 8),    # ragged last key block and slice
    (2, 2, 1345, 4),   # nkb = 6, multi-round
    (3, 2, 257, 2),    # nkb = 1
    (1, 2, 2049, 0),   # tiles <= workgroups: the completion pass does everything
]
DTS = [torch.float16, torch.bfloat16]


def lib():
    from denseclip_vit_multimodal_amd import _native
    return _native, _native.load()


_INPUTS = {}


def inputs(B, H, N, dt):
    """log2-domain q (as the kernels take it), k, v, dO and the forward's (o, lse); computed once"""
    key = (B, H, N, dt)
    if key not in _INPUTS:
        _, L = lib()
        C = 64 * H
        torch.manual_seed(100 + N)
        qkv = torch.randn(B * N, 3 * C, device=DEV) * 1.5
        qkv[:, :C] *= 0.125 * 1.4426950408889634
        qkv = qkv.to(dt)
        dout = torch.randn(B * N, C, device=DEV).to(dt)
        o = torch.empty(B * N, C, device=DEV, dtype=dt)
        lse = torch.empty(B * H * N, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        assert L.dclip_attn_fwd(code(dt), qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, 64, 0.125, st) == 0
        torch.cuda.synchronize()
        _INPUTS[key] = (qkv, dout, o, lse)
    return _INPUTS[key]


def code(dt):
    return 2 if dt == torch.bfloat16 else 1


def poisoned_ws(B, H, N):
    _, L = lib()
    ws = torch.empty(L.dclip_attn_bwd_workspace(B, N, H), device=DEV, dtype=torch.float32)
    ws.view(torch.uint8).fill_(0xFF)  # NaN bytes
    return ws


def launch(B, H, N, dt, ws, dqkv):
    _, L = lib()
    qkv, dout, o, lse = inputs(B, H, N, dt)
    st = torch.cuda.current_stream().cuda_stream
    assert L.dclip_attn_bwd(code(dt), qkv.data_ptr(), o.data_ptr(), dout.data_ptr(), lse.data_ptr(), ws.data_ptr(),
                            dqkv.data_ptr(), B, N, H, 64, 0.125, st) == 0, L.dclip_last_error()


class options:
    def __init__(self, block, cap=0, reduce=0):
        self.v = (block, cap, reduce)

    def __enter__(self):
        n, L = lib()
        for o, v in zip((n.OPT_ATTN_BWD_BLOCK, n.OPT_ATTN_BWD_WGS, n.OPT_ATTN_DQ_REDUCE), self.v):
            assert L.dclip_set_option(o, v) == 0

    def __exit__(self, *exc):
        n, L = lib()
        for o in (n.OPT_ATTN_BWD_BLOCK, n.OPT_ATTN_BWD_WGS, n.OPT_ATTN_DQ_REDUCE):
            L.dclip_set_option(o, 0)


def bwd(B, H, N, dt, block, cap=0, reduce=0, ws=None):
    ws = poisoned_ws(B, H, N) if ws is None else ws
    qkv = inputs(B, H, N, dt)[0]
    dqkv = torch.full_like(qkv, float("nan"))
    with options(block, cap, reduce):
        launch(B, H, N, dt, ws, dqkv)
    torch.cuda.synchronize()
    return dqkv, ws


def seam_state(ws, B, H, N):
    """(done[B*H], reduced[B*H][nrb]) as the last persistent call left them"""
    nrb = (N - 1 + 31) // 32
    w = ws.view(torch.int32)[:B * H * (1 + nrb)]
    return w[:B * H], w[B * H:].view(B * H, nrb)


_LEGACY = {}


def legacy(B, H, N, dt):
    key = (B, H, N, dt)
    if key not in _LEGACY:
        _LEGACY[key] = bwd(B, H, N, dt, LEGACY)[0]
        assert torch.isfinite(_LEGACY[key].float()).all()
    return _LEGACY[key]


def check_seams(ws, B, H, N, cap, what):
    """several rounds: every tile was published, and some seam found its (image, head) complete and
    reduced its share (it finished a whole tile earlier)"""
    nkb = (N - 1 + 255) // 256
    done, reduced = seam_state(ws, B, H, N)
    share = float(reduced.float().mean())
    print(f"{what}: {B * H * nkb} tiles on {cap} workgroups, seam duties reduced {100 * share:.0f} % of the 32-row blocks")
    assert bool((done == nkb).all()), done.tolist()
    assert bool(((reduced == 0) | (reduced == 1)).all())
    assert share > 0


@pytest.mark.parametrize("B,H,N,cap", CASES)
@pytest.mark.parametrize("dt", DTS, ids=["f16", "bf16"])
def test_persistent_bitwise_legacy(dt, B, H, N, cap):
    ref = legacy(B, H, N, dt)
    out, ws = bwd(B, H, N, dt, 0, cap)
    assert torch.equal(out, ref)
    if cap:
        check_seams(ws, B, H, N, cap, f"B={B} H={H} N={N} {dt}")


@pytest.mark.parametrize("dt", DTS, ids=["f16", "bf16"])
def test_persistent_twice_and_graph_replay(dt):
    """the counters are reset by every call: a second call on the same workspace, and replays of a
    captured call, give the same bits"""
    B, H, N, cap = CASES[0]
    ref = legacy(B, H, N, dt)
    out, ws = bwd(B, H, N, dt, 0, cap)
    assert torch.equal(out, ref)
    out2, _ = bwd(B, H, N, dt, 0, cap, ws=ws)
    assert torch.equal(out2, ref)
    check_seams(ws, B, H, N, cap, "second call")
    dqkv = torch.full_like(ref, float("nan"))
    g = torch.cuda.CUDAGraph()
    with options(0, cap):
        with torch.cuda.graph(g):
            launch(B, H, N, dt, ws, dqkv)
    for _ in range(2):
        dqkv.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dqkv, ref)
        check_seams(ws, B, H, N, cap, "replay")


@pytest.mark.parametrize("dt", DTS, ids=["f16", "bf16"])
def test_persistent_with_lds_completion_pass(dt):
    """DCLIP_OPT_ATTN_DQ_REDUCE 1 as the completion pass (8 queries per workgroup: it skips by the
    32-row block they are in); a ragged N - 1"""
    B, H, N, cap = CASES[1]
    out, ws = bwd(B, H, N, dt, 0, cap, reduce=1)
    assert torch.equal(out, legacy(B, H, N, dt))
    check_seams(ws, B, H, N, cap, "lds completion pass")


@pytest.mark.parametrize("dt", DTS, ids=["f16", "bf16"])
def test_persistent_after_legacy_on_same_workspace(dt):
    """L1-warm: the legacy path ran first on the same workspace, so the CUs that do the seam duties
    have read these partial lines before (other inputs' values: a stale line would show)"""
    B, H, N, cap = CASES[2]
    ref = legacy(B, H, N, dt)
    ws = poisoned_ws(B, H, N)
    qkv, dout, o, lse = inputs(B, H, N, dt)
    other = torch.full_like(qkv, float("nan"))
    _INPUTS[B, H, N, dt] = (qkv, dout.flip(0).contiguous(), o, lse)  # other partials on the same lines
    try:
        with options(LEGACY):
            launch(B, H, N, dt, ws, other)
    finally:
        _INPUTS[B, H, N, dt] = (qkv, dout, o, lse)
    out, _ = bwd(B, H, N, dt, 0, cap, ws=ws)
    assert not torch.equal(other, ref)
    assert torch.equal(out, ref)
    check_seams(ws, B, H, N, cap, "after the legacy path")
