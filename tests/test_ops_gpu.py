"""Per-kernel parity: every HIP kernel of the C ABI against a plain PyTorch fp32 statement of the same op
(inputs rounded to bf16 first, so the comparison isolates the kernel's own arithmetic: fp32 accumulate and one
bf16 rounding of the output).  Tolerances: rel-L2 <= 4e-3 for bf16 outputs of O(1) data (bf16 has 8 significant
bits: rounding alone gives ~1.7e-3), 1e-5 for fp32 outputs of elementwise kernels."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rel_l2(a, b):
    a = a.float().cpu(); b = b.float().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


def bf(x):
    return x.to(torch.bfloat16)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def ops():
    from dynamicrafter_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("M,N,K", [(256, 320, 320), (130, 640, 64), (1000, 448, 192), (77, 64, 1024), (513, 4, 128)])
def test_gemm_plain(ops, M, N, K):
    x = bf(rnd(M, K, seed=1)); w = rnd(N, K, seed=2, scale=K ** -0.5); b = rnd(N, seed=3)
    pw = ops.PackedWeight.linear(w, b, DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x.to(DEV), pw, out)
    ref = x.float() @ bf(w).float().t() + b
    assert rel_l2(out, ref) < 4e-3
    # fp32 output + alpha
    out32 = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ops.gemm(x.to(DEV), pw, out32, alpha=0.5)
    assert rel_l2(out32, 0.5 * ref) < 1e-5 + 1e-6


def test_gemm_epilogues(ops):
    M, N, K = 384, 320, 640
    x = bf(rnd(M, K, seed=1)); w = rnd(N, K, seed=2, scale=K ** -0.5); b = rnd(N, seed=3)
    res = bf(rnd(M, N, seed=4)); rv = rnd(3, N, seed=5)
    pw = ops.PackedWeight.linear(w, b, DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x.to(DEV), pw, out, residual=res.to(DEV), rowvec=rv.to(DEV), rows_per_vec=128)
    ref = x.float() @ bf(w).float().t() + b + rv.repeat_interleave(128, 0)
    ref = bf(ref).float() + res.float()   # kernel rounds to bf16 before the residual add
    assert rel_l2(out, ref) < 4e-3
    # strided input / output views (lda, ldc > width)
    big_in = torch.zeros(M, K + 64, dtype=torch.bfloat16, device=DEV); big_in[:, 32 - 32:K] = x.to(DEV)
    big_out = torch.zeros(M, N + 320, dtype=torch.bfloat16, device=DEV)
    ops.gemm(big_in[:, :K], pw, big_out[:, 320:])
    assert rel_l2(big_out[:, 320:], x.float() @ bf(w).float().t() + b) < 4e-3
    assert big_out[:, :320].abs().max().item() == 0


def test_gemm_geglu(ops):
    M, dim, inner = 200, 128, 512
    x = bf(rnd(M, dim, seed=1)); w = rnd(2 * inner, dim, seed=2, scale=dim ** -0.5); b = rnd(2 * inner, seed=3, scale=0.1)
    pw = ops.PackedWeight.linear(w, b, DEV)
    out = torch.empty(M, inner, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x.to(DEV), pw, out, geglu=True)
    h = x.float() @ bf(w).float().t() + b
    val, gate = h.chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    assert rel_l2(out, ref) < 4e-3


@pytest.mark.parametrize("cfg", [
    dict(n=3, C=64, Co=128, H=9, W=11, stride=1, pad=1, ups=0),
    dict(n=2, C=128, Co=320, H=12, W=16, stride=2, pad=1, ups=0),      # UNet Downsample
    dict(n=2, C=64, Co=64, H=12, W=10, stride=2, pad=0, ups=0),        # AE Downsample: pad (0,1,0,1)
    dict(n=2, C=128, Co=192, H=6, W=7, stride=1, pad=1, ups=1),        # nearest x2 + conv
    dict(n=2, C=8, Co=64, H=8, W=8, stride=1, pad=1, ups=0),           # Cin padded to 64
])
def test_conv3x3(ops, cfg):
    _conv3x3(ops, cfg)


def _under_plan(ops, plan, fn):
    """fn() with the GEMM plan set to `plan` (None: whatever is set), restored afterwards"""
    if plan is None:
        return fn()
    lib = ops._hip.lib()
    prev = lib.dc_gemm_set_plan(plan)
    assert prev >= 0
    try:
        return fn()
    finally:
        lib.dc_gemm_set_plan(prev)


def _conv3x3(ops, cfg, routes=None):
    """routes = {plan: kernel name}: the launch is repeated under each plan and must be dispatched to exactly that kernel
    (dc_gemm_last_variant); None: one launch under the current plan, whichever kernel takes it."""
    n, Cc, Co, H, W = cfg["n"], cfg["C"], cfg["Co"], cfg["H"], cfg["W"]
    x = bf(rnd(n, Cc, H, W, seed=1)); w = rnd(Co, Cc, 3, 3, seed=2, scale=(9 * Cc) ** -0.5); b = rnd(Co, seed=3)
    xr = x.float()
    if cfg["ups"]:
        xr = F.interpolate(xr, scale_factor=2, mode="nearest")
    if cfg["stride"] == 2 and cfg["pad"] == 0:
        xr = F.pad(xr, (0, 1, 0, 1))
        ref = F.conv2d(xr, bf(w).float(), b, stride=2, padding=0)
    else:
        ref = F.conv2d(xr, bf(w).float(), b, stride=cfg["stride"], padding=cfg["pad"])
    OH, OW = ref.shape[2], ref.shape[3]
    pw = ops.PackedWeight.conv3x3(w, b, DEV)
    cp = pw.Cin
    rows = torch.zeros(n * H * W, cp, dtype=torch.bfloat16, device=DEV)
    rows[:, :Cc] = x.permute(0, 2, 3, 1).reshape(-1, Cc).to(DEV)
    for plan, want in (routes or {None: None}).items():
        out = torch.empty(n * OH * OW, Co, dtype=torch.bfloat16, device=DEV)
        _under_plan(ops, plan, lambda: ops.gemm(rows, pw, out, conv=dict(IH=H, IW=W, OH=OH, OW=OW, stride=cfg["stride"],
                                                                         pad=cfg["pad"], ups=cfg["ups"])))
        assert want is None or _variant(ops) == want, (plan, want, _variant(ops))
        got = out.float().cpu().reshape(n, OH, OW, Co).permute(0, 3, 1, 2)
        assert rel_l2(got, ref) < 4e-3


# ---- conv_out of the UNet (320 -> 4, fp32 rows) and of the AE decoder (128 -> 3, bf16 rows, N padded to 4): the narrow-N kernel
# (conv3x3_narrow_kernel: halo window of a 4 x 64 pixel tile in LDS, 16x16x32 MFMA) against torch and against the tile kernel
@pytest.mark.parametrize("n,C,Co,H,W,f32", [
    (4, 320, 4, 18, 32, True),        # whole tiles in y, half a tile in x
    (3, 128, 3, 17, 70, False),       # ragged in both directions, 3 real channels of 4
    (2, 64, 4, 8, 200, True),         # one slice, four tiles across
    (5, 640, 8, 5, 9, False),         # tiny frames, two channel quads, ten slices
])
def test_conv3x3_narrow_out(ops, n, C, Co, H, W, f32):
    x = bf(rnd(n, C, H, W, seed=1)); w = rnd(Co, C, 3, 3, seed=2, scale=(9 * C) ** -0.5); b = rnd(Co, seed=3)
    ref = F.conv2d(x.float(), bf(w).float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    pw = ops.PackedWeight.conv3x3(w, b, DEV, n_align=4)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    conv = dict(IH=H, IW=W, OH=H, OW=W, stride=1, pad=1, ups=0)
    out = torch.full((n * H * W, pw.N), 7.0, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
    ops.gemm(rows, pw, out, conv=conv)
    assert _variant(ops) == "conv3x3_narrow_kernel", _variant(ops)
    assert rel_l2(out[:, :Co], ref) < (1e-5 if f32 else 4e-3)
    if pw.N > Co:
        assert out[:, Co:].abs().max().item() == 0          # the padding channel: zero weights and bias
    lib = ops._hip.lib()
    prev = lib.dc_gemm_set_plan(19 | 128)                   # plan bit 7: the tile kernels take the launch
    assert prev >= 0
    try:
        out2 = torch.empty_like(out)
        ops.gemm(rows, pw, out2, conv=conv)
        assert _variant(ops) != "conv3x3_narrow_kernel", _variant(ops)
    finally:
        lib.dc_gemm_set_plan(prev)
    assert rel_l2(out, out2) < (2e-6 if f32 else 4e-3)       # fp32 rows: the same bf16 products, another summation order


# ---- the AE's full-resolution ResnetBlock convs (N = 128): conv3x3_window128_kernel (halo window + weight taps through LDS)
@pytest.mark.parametrize("n,C,H,W,res,Co", [
    (16, 128, 64, 256, False, 128),   # 1024 whole tiles
    (18, 128, 61, 250, True, 128),    # ragged in both directions, + residual (conv2 of a ResnetBlock)
    (18, 256, 61, 250, False, 128),   # four channel slices (the 256 -> 128 conv of decoder block 0)
    (18, 128, 61, 250, True, 256),    # N = 256: two launches over the channel halves
])
def test_conv3x3_window128(ops, n, C, H, W, res, Co):
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn(n, C, H, W, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(Co, C, 3, 3, device=DEV, generator=g) * (9 * C) ** -0.5
    b = torch.randn(Co, device=DEV, generator=g)
    r = torch.randn(n * H * W, Co, device=DEV, generator=g).to(torch.bfloat16) if res else None
    ref = F.conv2d(x.float(), w.to(torch.bfloat16).float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    if res:
        ref = ref.to(torch.bfloat16).float() + r.float()
    pw = ops.PackedWeight.conv3x3(w.cpu(), b.cpu(), DEV)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    conv = dict(IH=H, IW=W, OH=H, OW=W, stride=1, pad=1, ups=0)
    out = torch.empty(n * H * W, Co, dtype=torch.bfloat16, device=DEV)
    ops.gemm(rows, pw, out, conv=conv, residual=r)
    assert _variant(ops).startswith("conv3x3_window128_kernel"), _variant(ops)
    assert rel_l2(out, ref) < 4e-3
    out_b = torch.empty_like(out)
    ops.gemm(rows, pw, out_b, conv=conv, residual=r)
    assert torch.equal(out, out_b)                          # deterministic
    lib = ops._hip.lib()
    prev = lib.dc_gemm_set_plan(19 | 256)                   # plan bit 8: the tile kernel takes the launch
    assert prev >= 0
    try:
        out2 = torch.empty_like(out)
        ops.gemm(rows, pw, out2, conv=conv, residual=r)
        assert not _variant(ops).startswith("conv3x3_window128_kernel"), _variant(ops)
    finally:
        lib.dc_gemm_set_plan(prev)
    assert rel_l2(out, out2) < 4e-3


def test_tconv3(ops):
    B, T, HW, Cc = 2, 5, 37, 128
    x = bf(rnd(B, Cc, T, HW, 1, seed=1)); w = rnd(Cc, Cc, 3, 1, 1, seed=2, scale=(3 * Cc) ** -0.5); b = rnd(Cc, seed=3)
    ref = F.conv3d(x.float(), bf(w).float(), b, padding=(1, 0, 0))
    pw = ops.PackedWeight.tconv3(w, b, DEV)
    rows = x.permute(0, 2, 3, 4, 1).reshape(-1, Cc).contiguous().to(DEV)
    out = torch.empty_like(rows)
    ops.gemm(rows, pw, out, tconv=dict(T=T, HW=HW))
    got = out.float().cpu().reshape(B, T, HW, 1, Cc).permute(0, 4, 1, 2, 3)
    assert rel_l2(got, ref) < 4e-3


@pytest.mark.parametrize("Cc,n_inst,rpi,silu,eps", [(320, 4, 200, True, 1e-5), (64, 2, 33, False, 1e-6),
                                                    (2560, 2, 144, True, 1e-5), (128, 1, 5000, True, 1e-6),
                                                    (960, 3, 64, True, 1e-5),
                                                    (320, 32, 4608, True, 1e-5),       # the 4-D norms of the step: 32 frames x 64 chunks
                                                    (1280, 32, 150, True, 1e-5)])
def test_groupnorm(ops, Cc, n_inst, rpi, silu, eps):
    x = bf(rnd(n_inst * rpi, Cc, seed=1) * 2 + 0.5)
    g = 1 + 0.2 * rnd(Cc, seed=2); b = 0.3 * rnd(Cc, seed=3)
    y = torch.empty_like(x, device=DEV)
    ops.groupnorm(x.to(DEV), y, g.to(DEV), b.to(DEV), groups=32, n_inst=n_inst, rows_per_inst=rpi, eps=eps, silu=silu)
    xr = x.float().reshape(n_inst, rpi, Cc).permute(0, 2, 1)     # [n, C, rows]
    ref = F.group_norm(xr, 32, g, b, eps)
    if silu:
        ref = F.silu(ref)
    ref = ref.permute(0, 2, 1).reshape(-1, Cc)
    assert rel_l2(y, ref) < 4e-3


@pytest.mark.parametrize("n_inst,rpi", [(2, 40000), (32, 2500)])      # 625 / 40 chunks per instance
@pytest.mark.parametrize("offset,std", [(50.0, 1.0), (300.0, 0.5), (-20.0, 3.0)])
def test_groupnorm_large_dc_offset(ops, offset, std, n_inst, rpi):
    """Channels with a large mean (real-checkpoint activations, AE high-resolution levels): the statistics are shifted
    moments merged with Chan's update, not E[x^2] - mean^2. Reference: fp64 group_norm of the same bf16 samples."""
    Cc = 320
    x = bf(rnd(n_inst * rpi, Cc, seed=4) * std + offset)
    g = 1 + 0.2 * rnd(Cc, seed=2); b = 0.3 * rnd(Cc, seed=3)
    y = torch.empty_like(x, device=DEV)
    ops.groupnorm(x.to(DEV), y, g.to(DEV), b.to(DEV), groups=32, n_inst=n_inst, rows_per_inst=rpi, eps=1e-5, silu=False)
    xr = x.double().reshape(n_inst, rpi, Cc).permute(0, 2, 1)
    ref = F.group_norm(xr, 32, g.double(), b.double(), 1e-5).permute(0, 2, 1).reshape(-1, Cc)
    assert rel_l2(y, ref) < 4e-3


@pytest.mark.parametrize("Cc", [320, 512, 640, 1280, 64])
def test_layernorm(ops, Cc):
    R = 301
    x = bf(rnd(R, Cc, seed=1) * 3 - 1)
    g = 1 + 0.2 * rnd(Cc, seed=2); b = 0.3 * rnd(Cc, seed=3)
    y = torch.empty_like(x, device=DEV)
    ops.layernorm(x.to(DEV), y, g.to(DEV), b.to(DEV), 1e-5)
    assert rel_l2(y, F.layer_norm(x.float(), (Cc,), g, b, 1e-5)) < 4e-3


def _attn_ref(q, k, v, heads, scale):
    # q [B, Lq, h*64], k/v [B, Lk, h*64] -> [B, Lq, h*64]
    B, Lq, _ = q.shape
    qh = q.reshape(B, Lq, heads, 64).transpose(1, 2)
    kh = k.reshape(B, -1, heads, 64).transpose(1, 2)
    vh = v.reshape(B, -1, heads, 64).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, Lq, heads * 64)


@pytest.mark.parametrize("B,heads,Lq,Lk", [(2, 5, 144, 144), (1, 2, 300, 77), (3, 1, 64, 16), (1, 3, 1000, 1000),
                                           (2, 2, 40, 40)])
def test_flash_attn(ops, B, heads, Lq, Lk):
    Cc = heads * 64
    q = bf(rnd(B, Lq, Cc, seed=1)); k = bf(rnd(B, Lk, Cc, seed=2)); v = bf(rnd(B, Lk, Cc, seed=3))
    o = torch.zeros(B * Lq, Cc, dtype=torch.bfloat16, device=DEV)
    ops.flash_attn(q.reshape(-1, Cc).to(DEV), k.reshape(-1, Cc).to(DEV), v.reshape(-1, Cc).to(DEV), o,
                   batch=B, heads=heads, Lq=Lq, Lk=Lk, scale=0.125)
    ref = _attn_ref(q.float(), k.float(), v.float(), heads, 0.125).reshape(-1, Cc)
    assert rel_l2(o, ref) < 6e-3
    # accumulate epilogue: o += 0.5 * attn
    ops.flash_attn(q.reshape(-1, Cc).to(DEV), k.reshape(-1, Cc).to(DEV), v.reshape(-1, Cc).to(DEV), o,
                   batch=B, heads=heads, Lq=Lq, Lk=Lk, scale=0.125, accumulate=True, acc_scale=0.5)
    assert rel_l2(o, 1.5 * ref) < 8e-3


def test_flash_attn_fused_qkv_and_spike(ops):
    """q/k/v as column slices of one [rows, 3C] buffer; a spiked key forces a large running-max jump."""
    B, heads, L = 2, 2, 200
    Cc = heads * 64
    qkv = rnd(B * L, 3 * Cc, seed=5)
    qkv[130, Cc:2 * Cc] *= 12.0
    qkv = bf(qkv)
    d = qkv.to(DEV)
    o = torch.empty(B * L, Cc, dtype=torch.bfloat16, device=DEV)
    ops.flash_attn(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], o, batch=B, heads=heads, Lq=L, Lk=L, scale=0.125)
    f = qkv.float().reshape(B, L, 3 * Cc)
    ref = _attn_ref(f[..., :Cc], f[..., Cc:2 * Cc], f[..., 2 * Cc:], heads, 0.125).reshape(-1, Cc)
    assert rel_l2(o, ref) < 6e-3


# modes of the long self-attention kernel (dc_flash_attn_set_mode): (mode, thr) - default = no running max in the main pass (shift
# 0, out-of-range row sums fall back to the tracking pass), three query blocks per wave when Lq % 384 == 0; bit 0 = the
# running-max (tracking) pass run directly, with thr = 0 (rescale on every growth) and 8; bit 1 = two query blocks per wave
FLASH_MODES = [(0, 8.0), (1, 0.0), (1, 8.0), (2, 8.0), (3, 0.0)]


@pytest.fixture
def flash_mode(request):
    from dynamicrafter_amd import _hip
    mode, thr = request.param
    assert _hip.lib().dc_flash_attn_set_mode(mode, thr) == 0
    yield request.param
    assert _hip.lib().dc_flash_attn_set_mode(0, 8.0) == 0


@pytest.mark.parametrize("flash_mode", FLASH_MODES, indirect=True)
@pytest.mark.parametrize("B,heads,Lq,Lk", [(2, 2, 1024, 1024), (1, 3, 768, 256), (1, 1, 1000, 512), (1, 2, 512, 2304),
                                           (2, 1, 1152, 1152), (1, 2, 768, 320), (1, 1, 640, 448), (1, 1, 530, 128 + 64)])
def test_flash_attn_long_self(ops, flash_mode, B, heads, Lq, Lk):
    """Shapes that take the one-wave-per-SIMD software-pipelined kernel (flash_pipe.hip: Lq >= 512, Lk >= 256, Lk % 64 == 0)
    and, last case, its boundary (Lk = 192 stays on the two-waves kernel). Ragged Lq exercises the clamped tail rows, Lk = 256 /
    320 / 448 the shortest rings (4, 5 and 7 tiles: the loop runs Lk / 64 - 1 iterations around a 4-stage ring)."""
    Cc = heads * 64
    q = bf(rnd(B, Lq, Cc, seed=11)); k = bf(rnd(B, Lk, Cc, seed=12)); v = bf(rnd(B, Lk, Cc, seed=13))
    o = torch.zeros(B * Lq, Cc, dtype=torch.bfloat16, device=DEV)
    ops.flash_attn(q.reshape(-1, Cc).to(DEV), k.reshape(-1, Cc).to(DEV), v.reshape(-1, Cc).to(DEV), o,
                   batch=B, heads=heads, Lq=Lq, Lk=Lk, scale=0.125)
    ref = _attn_ref(q.float(), k.float(), v.float(), heads, 0.125).reshape(-1, Cc)
    assert rel_l2(o, ref) < 6e-3


@pytest.mark.parametrize("flash_mode", FLASH_MODES, indirect=True)
@pytest.mark.parametrize("spikes", [(5,), (40,), (70,), (100,), (130, 131), (511,), (480,), (449, 20), (200, 300, 400, 500),
                                    tuple(range(0, 512, 37))])
@pytest.mark.parametrize("L", [512, 768])
def test_flash_attn_long_self_running_max_jumps(ops, flash_mode, spikes, L):
    """Keys with 6-14x the norm at chosen positions (first / second half tile, tile seams, the last half tiles, many at
    once; growing sizes so that each raises the maximum again). The default pass keeps the shift of the first 32 keys (its P
    then reach 2^40 and more: same relative precision); the tracking pass decides one half tile late whether a row's running
    max grew and rescales O, the row sums and the already packed P of the pending half tile - the spikes force that path at
    every stage of its pipeline. L = 768 takes the three-blocks-per-wave kernel."""
    B, heads = 1, 2
    Cc = heads * 64
    qkv = rnd(B * L, 3 * Cc, seed=21)
    for n, pos in enumerate(spikes):
        qkv[pos, Cc:2 * Cc] *= 6.0 + 0.6 * n
    qkv = bf(qkv)
    d = qkv.to(DEV)
    o = torch.empty(B * L, Cc, dtype=torch.bfloat16, device=DEV)
    ops.flash_attn(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], o, batch=B, heads=heads, Lq=L, Lk=L, scale=0.125)
    f = qkv.float().reshape(B, L, 3 * Cc)
    ref = _attn_ref(f[..., :Cc], f[..., Cc:2 * Cc], f[..., 2 * Cc:], heads, 0.125).reshape(-1, Cc)
    assert torch.isfinite(o.float()).all()
    assert rel_l2(o, ref) < 6e-3


@pytest.mark.parametrize("flash_mode", [(0, 8.0), (2, 8.0)], indirect=True)
@pytest.mark.parametrize("L", [512, 768])
@pytest.mark.parametrize("pos", [3, 33, 100, 300, 511])
def test_flash_attn_long_self_fallback_to_tracking_pass(ops, flash_mode, pos, L):
    """A key whose scores reach +-600 in exp2 units: the default pass (no running max) overflows its row sums for most rows
    and the workgroup must repeat its block with the running-max pass (softmax is a one-hot on the spiked key for rows
    with a positive score, and the plain softmax elsewhere). A second launch with ordinary data follows: the fallback
    leaves no state behind."""
    B, heads = 1, 2
    Cc = heads * 64
    qkv = rnd(B * L, 3 * Cc, seed=41)
    qkv[pos, Cc:2 * Cc] *= 150.0
    qkv = bf(qkv)
    d = qkv.to(DEV)
    o = torch.empty(B * L, Cc, dtype=torch.bfloat16, device=DEV)
    ops.flash_attn(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], o, batch=B, heads=heads, Lq=L, Lk=L, scale=0.125)
    f = qkv.float().reshape(B, L, 3 * Cc)
    ref = _attn_ref(f[..., :Cc], f[..., Cc:2 * Cc], f[..., 2 * Cc:], heads, 0.125).reshape(-1, Cc)
    assert torch.isfinite(o.float()).all()
    # scores of +-600 in exp2 units: the bf16 rounding of the pre-scaled Q (2^-9 relative) moves them by ~1 unit, which
    # shows in the rows where the spiked key competes with another one (measured 8e-3; the two-waves kernel likewise)
    assert rel_l2(o, ref) < 1.6e-2
    qkv2 = bf(rnd(B * L, 3 * Cc, seed=42)).to(DEV)
    ops.flash_attn(qkv2[:, :Cc], qkv2[:, Cc:2 * Cc], qkv2[:, 2 * Cc:], o, batch=B, heads=heads, Lq=L, Lk=L, scale=0.125)
    f = qkv2.float().cpu().reshape(B, L, 3 * Cc)
    ref = _attn_ref(f[..., :Cc], f[..., Cc:2 * Cc], f[..., 2 * Cc:], heads, 0.125).reshape(-1, Cc)
    assert rel_l2(o, ref) < 6e-3


@pytest.mark.parametrize("flash_mode", [(0, 8.0), (2, 8.0)], indirect=True)
def test_flash_attn_long_self_all_scores_far_below_zero(ops, flash_mode):
    """Every score of some rows below -100 in exp2 units (q and all keys anti-aligned and large): the default pass's row sums
    underflow there and the fallback must produce the ordinary softmax."""
    B, heads, L = 1, 1, 768
    g = torch.Generator().manual_seed(51)
    u = torch.randn(64, generator=g); u = u / u.norm()
    q = rnd(L, 64, seed=52); k = rnd(L, 64, seed=53); v = rnd(L, 64, seed=54)
    k = k + 40.0 * u                       # every key has a large component along u
    q[100:140] = q[100:140] - 30.0 * u     # these queries point the other way: scores ~ -1200 / 8 = -150 nats
    q, k, v = bf(q), bf(k), bf(v)
    o = torch.zeros(L, 64, dtype=torch.bfloat16, device=DEV)
    ops.flash_attn(q.to(DEV), k.to(DEV), v.to(DEV), o, batch=B, heads=heads, Lq=L, Lk=L, scale=0.125)
    ref = _attn_ref(q.float()[None], k.float()[None], v.float()[None], heads, 0.125).reshape(-1, 64)
    assert torch.isfinite(o.float()).all()
    assert rel_l2(o, ref) < 1.6e-2


def test_flash_attn_long_self_strided_batches(ops):
    """q/k/v as column slices of one fused buffer with batch strides larger than L (the UNet's call shape)."""
    B, heads, L, Lpad = 3, 5, 576, 600
    Cc = heads * 64
    qkv = bf(rnd(B * Lpad, 3 * Cc, seed=31))
    d = qkv.to(DEV)
    o = torch.zeros(B * Lpad, Cc, dtype=torch.bfloat16, device=DEV)
    ops.flash_attn(d[:, :Cc], d[:, Cc:2 * Cc], d[:, 2 * Cc:], o, batch=B, heads=heads, Lq=L, Lk=L, scale=0.125,
                   q_bstride=Lpad, kv_bstride=Lpad)
    f = qkv.float().reshape(B, Lpad, 3 * Cc)[:, :L]
    ref = _attn_ref(f[..., :Cc], f[..., Cc:2 * Cc], f[..., 2 * Cc:], heads, 0.125)
    got = o.float().cpu().reshape(B, Lpad, Cc)
    assert rel_l2(got[:, :L].reshape(-1, Cc), ref.reshape(-1, Cc)) < 6e-3
    assert (got[:, L:] == 0).all()          # rows between the batch items are not touched


@pytest.mark.parametrize("B,T,HW,heads", [(2, 16, 50, 5), (1, 16, 7, 8), (1, 4, 33, 2)])
def test_temporal_attn(ops, B, T, HW, heads):
    Cc = heads * 64
    qkv = bf(rnd(B * T * HW, 3 * Cc, seed=7))
    o = torch.zeros(B * T * HW, Cc, dtype=torch.bfloat16, device=DEV)
    ops.temporal_attn(qkv.to(DEV), o, B=B, T=T, HW=HW, heads=heads, scale=0.125)
    f = qkv.float().reshape(B, T, HW, 3 * Cc).permute(0, 2, 1, 3).reshape(B * HW, T, 3 * Cc)
    ref = _attn_ref(f[..., :Cc], f[..., Cc:2 * Cc], f[..., 2 * Cc:], heads, 0.125)
    ref = ref.reshape(B, HW, T, Cc).permute(0, 2, 1, 3).reshape(-1, Cc)
    assert rel_l2(o, ref) < 6e-3


def test_gemv_and_embedding(ops):
    M, K, N = 2, 320, 1280
    t = torch.tensor([999, 17], dtype=torch.int64)
    emb = torch.empty(M, K, dtype=torch.float32, device=DEV)
    ops.timestep_embedding(t.to(DEV), emb, K)
    half = K // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    ref_e = torch.cat([torch.cos(args), torch.sin(args)], -1)
    assert (emb.cpu() - ref_e).abs().max().item() < 2e-4     # fp32 cos/sin of arguments up to 999
    w = rnd(N, K, seed=1, scale=K ** -0.5); b = rnd(N, seed=2)
    pw = ops.PackedWeight.linear(w, b, DEV)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ops.gemv_small(emb, pw, out, act_in=0, act_out=1)
    ref = F.silu(emb.cpu() @ bf(w).float().t() + b)
    assert rel_l2(out, ref) < 1e-5
    out2 = out.clone()
    ops.gemv_small(emb, pw, out2, act_in=1, act_out=0, accumulate=True)
    ref2 = ref + F.silu(emb.cpu()) @ bf(w).float().t() + b
    assert rel_l2(out2, ref2) < 1e-5


def test_layout_kernels(ops):
    B, Cx, Cc, T, HW = 2, 4, 4, 3, 20
    x = rnd(B, Cx, T, HW, seed=1); cc = rnd(B, Cc, T, HW, seed=2)
    out = torch.full((2 * B * T * HW, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.pack_latent(x.to(DEV), cc.to(DEV), out, B=B, Cx=Cx, Cc=Cc, T=T, HW=HW, nrep=2)
    ref = torch.cat([x, cc], 1).permute(0, 2, 3, 1).reshape(-1, Cx + Cc)
    got = out.float().cpu()
    assert torch.equal(got[:B * T * HW, :8], bf(ref).float()) and torch.equal(got[B * T * HW:, :8], bf(ref).float())
    assert got[:, 8:].abs().max().item() == 0
    # nchw <-> rows
    img = rnd(3, 3, 30, seed=3)
    rows = torch.empty(3 * 30, 64, dtype=torch.bfloat16, device=DEV)
    ops.nchw_to_rows(img.to(DEV), rows, N=3, Cc=3, HW=30, scale=2.0)
    assert torch.equal(rows[:, :3].float().cpu(), bf(2 * img.permute(0, 2, 1).reshape(-1, 3)).float())
    back = torch.empty(3, 3, 30, dtype=torch.float32, device=DEV)
    ops.rows_to_nchw(rows, back, N=3, Cc=3, HW=30, scale=0.5)
    assert torch.equal(back.cpu(), bf(2 * img).float() * 0.5)
    # copy2d into a concat buffer, add_rows
    a = bf(rnd(50, 64, seed=4)); b2 = bf(rnd(50, 128, seed=5))
    cat = torch.empty(50, 192, dtype=torch.bfloat16, device=DEV)
    ops.copy2d(a.to(DEV), cat[:, :64]); ops.copy2d(b2.to(DEV), cat[:, 64:])
    assert torch.equal(cat.cpu(), torch.cat([a, b2], 1))
    s = torch.empty(50, 64, dtype=torch.bfloat16, device=DEV)
    ops.add_rows(a.to(DEV), a.to(DEV), s)
    assert torch.equal(s.cpu(), bf(a.float() * 2))
    # context assembly
    Bc, Tc, L, D = 2, 3, 4, 64
    ctx = rnd(Bc, 77 + Tc * L, D, seed=6)
    outc = torch.empty(Bc * Tc, 77 + L, D, dtype=torch.bfloat16, device=DEV)
    ops.build_context(ctx.to(DEV), outc, B=Bc, T=Tc, n_text=77, L=L, D=D)
    text = ctx[:, :77].repeat_interleave(Tc, 0)
    imgc = ctx[:, 77:].reshape(Bc, Tc, L, D).reshape(Bc * Tc, L, D)
    assert torch.equal(outc.cpu(), bf(torch.cat([text, imgc], 1)))


def test_softmax_and_vae_sample(ops):
    x = rnd(37, 1000, seed=1) * 4
    y = torch.empty(37, 1000, dtype=torch.bfloat16, device=DEV)
    ops.softmax_rows(x.to(DEV), y)
    assert rel_l2(y, torch.softmax(x, -1)) < 4e-3
    N, zc, HW = 2, 4, 50
    mom = bf(rnd(N * HW, 8, seed=2) * 3); noise = rnd(N, zc, HW, seed=3)
    z = torch.empty(N, zc, HW, dtype=torch.float32, device=DEV)
    ops.vae_sample(mom.to(DEV), noise.to(DEV), z, N=N, zc=zc, HW=HW, scale=0.18215)
    m = mom.float().reshape(N, HW, 8).permute(0, 2, 1)
    mean, logvar = m[:, :4], torch.clamp(m[:, 4:], -30, 20)
    ref = 0.18215 * (mean + torch.exp(0.5 * logvar) * noise)
    assert rel_l2(z, ref) < 1e-5


# ---- large launches: these shapes take the 256-row LDS-DMA pipeline (gemm_conv_glds.hip) --------------------
# Which kernel each shape of the tests below is dispatched to (dc_gemm_last_variant, asserted by exact name), per plan: 19 is the
# default, 0 the documented A/B fallback without the one-wave and ping-pong kernels (3 = 19 without the ping-pong kernel). A test
# named after a kernel that today's default plan no longer gives its shape runs under both plans; a threshold edit that moves a
# shape to another kernel fails here instead of silently changing what the test covers. (tests/exact_cases.py has the smallest
# shape of every variant and the dispatch rules.)
_T, _G, _P, _PIPE = "gemm_conv_kernel", "gemm_conv_glds_kernel", "gemm_persist_kernel", "gemm_pipe320x16_kernel"
_P320 = (_P + "<320,residual>", _P + "<320>")               # (bf16 launch with residual + row vector, fp32 launch)
GEMM_ROUTES = {                                             # (M, N, K) -> {plan: (bf16 launch, fp32 launch)}
    (25600, 512, 320): {19: (_G + "<256>",) * 2},
    (20480 + 77, 320, 640): {19: (_T + "<64>",) * 2},       # 81 row tiles: below every large-tile threshold
    (30000, 448, 192): {19: (_G + "<128>",) * 2},
    (131072, 64, 64): {19: (_P + "<64>",) * 2},
    (51200 + 100, 320, 128): {19: (_P + "<64>",) * 2},      # 201 x 5 tiles of 64 columns: the persistent kernel, not the 320-wide tile
    (25600 + 7, 640, 320): {19: (_G + "<320>",) * 2},
    (52000, 1280, 64): {19: _P320},
    (65536 + 50, 512, 320): {19: (_P + "<128>",) * 2},
    (65536 + 50, 320, 320): {19: (_P + "<64>",) * 2},
    (140000, 640, 640): {19: _P320},
    (70000, 448, 64): {19: (_P + "<128>",) * 2},
    (140000, 320, 320): {19: _P320},
    (135000, 960, 128): {19: _P320},
    (18432, 1280, 1280): {19: (_P + "<128>",) * 2},         # 72 x 4 = 288 tiles of 320: the 128-wide persistent kernel (720 tiles)
    (4608 + 33, 1280, 640): {19: (_T + "<128>",) * 2},
    (73728, 640, 320): {19: _P320},
    (10000, 320, 2560): {19: (_PIPE + "+splitk", _G + "<320>+splitk"), 0: (_G + "<320>+splitk",) * 2},
    (256 * 70, 960, 128): {19: (_P + "<128>",) * 2},
}
CONV_ROUTES = {                                             # (n, C, Co, H, W, stride, pad, ups) -> {plan: kernel}
    (32, 64, 256, 40, 40, 1, 1, 0): {19: _G + "<256,conv>"},
    (30, 128, 320, 33, 47, 1, 1, 0): {19: _PIPE + "<conv>", 0: _T + "<64>"},
    (32, 64, 256, 20, 20, 1, 1, 1): {19: _G + "<256,conv>"},
    (32, 64, 256, 80, 80, 2, 1, 0): {19: _G + "<256,conv>"},
    (36, 128, 320, 33, 47, 1, 1, 0): {19: _PIPE + "<conv>", 0: _G + "<320,conv>"},
    (32, 64, 640, 20, 20, 1, 1, 1): {19: _PIPE + "<conv,ups>", 0: _G + "<320,conv>"},
    (32, 64, 320, 81, 80, 2, 1, 0): {19: _PIPE + "<conv>", 0: _G + "<320,conv>"},
    (32, 128, 1280, 18, 32, 1, 1, 0): {19: _PIPE + "<conv>+splitk", 0: _G + "<320,conv>+splitk"},
    (32, 64, 640, 9, 16, 1, 1, 0): {19: _T + "<128>"},
    (30, 192, 320, 17, 23, 1, 1, 0): {19: _PIPE + "<conv>+splitk", 0: _G + "<320,conv>+splitk"},
    (32, 64, 640, 18, 16, 1, 1, 1): {19: _G + "<128,conv>"},
    # named after gemm_persist_kernel<320,conv>, which takes >= 1024 tiles (and only where the one-wave kernel is off): these
    # 576..588-tile shapes go to the one-wave kernel, or to the 320-wide tile under plan 0; the persistent conv kernel itself is
    # pinned by test_conv3x3_persistent_residual_rowvec under plan 0 and by the exact cases
    (16, 128, 320, 96, 96, 1, 1, 0): {19: _PIPE + "<conv>+splitk", 0: _G + "<320,conv>+splitk"},
    (15, 64, 320, 97, 101, 1, 1, 0): {19: _PIPE + "<conv>", 0: _G + "<320,conv>"},
    (16, 64, 320, 192, 192, 2, 1, 0): {19: _PIPE + "<conv>", 0: _G + "<320,conv>"},
    (16, 64, 320, 192, 192, 2, 0, 0): {19: _PIPE + "<conv>", 0: _G + "<320,conv>"},
    # test_conv3x3_splitk
    (8, 1280, 1280, 18, 32, 1, 1, 0): {19: _PIPE + "<conv>+splitk", 0: _G + "<320,conv>+splitk"},
    (32, 1280, 1280, 18, 32, 1, 1, 0): {19: _PIPE + "<conv>+splitk", 0: _G + "<320,conv>+splitk"},
}


def _conv_routes(cfg):
    return CONV_ROUTES[tuple(cfg[k] for k in ("n", "C", "Co", "H", "W", "stride", "pad", "ups"))]


def _geglu_routed(ops, M, dim, inner, routes):
    """The GEGLU projection [M, dim] -> [M, inner] under each plan of routes = {plan: kernel name}"""
    x = bf(rnd(M, dim, seed=1)); w = rnd(2 * inner, dim, seed=2, scale=dim ** -0.5); b = rnd(2 * inner, seed=3, scale=0.1)
    pw = ops.PackedWeight.linear(w, b, DEV)
    h = x.float() @ bf(w).float().t() + b
    val, gate = h.chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    xd = x.to(DEV)
    for plan, want in routes.items():
        out = torch.empty(M, inner, dtype=torch.bfloat16, device=DEV)
        _under_plan(ops, plan, lambda: ops.gemm(xd, pw, out, geglu=True))
        assert _variant(ops) == want, (plan, want, _variant(ops))
        assert rel_l2(out, ref) < 4e-3


def _tconv3_routed(ops, B, T, HW, Cc, res, routes, twice=False):
    """The 3-tap temporal conv (+ residual) under each plan of routes = {plan: kernel name}; None: the current plan, any kernel"""
    x = bf(rnd(B, Cc, T, HW, 1, seed=1)); w = rnd(Cc, Cc, 3, 1, 1, seed=2, scale=(3 * Cc) ** -0.5); b = rnd(Cc, seed=3)
    ref = F.conv3d(x.float(), bf(w).float(), b, padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(-1, Cc)
    pw = ops.PackedWeight.tconv3(w, b, DEV)
    rows = x.permute(0, 2, 3, 4, 1).reshape(-1, Cc).contiguous().to(DEV)
    r = bf(rnd(rows.shape[0], Cc, seed=res)) if res else None
    if res:
        ref = bf(ref).float() + r.float()
        r = r.to(DEV)
    for plan, want in (routes or {None: None}).items():
        out = torch.empty_like(rows)
        _under_plan(ops, plan, lambda: ops.gemm(rows, pw, out, tconv=dict(T=T, HW=HW), residual=r))
        assert want is None or _variant(ops) == want, (plan, want, _variant(ops))
        assert rel_l2(out, ref) < 4e-3
        if twice:
            out2 = torch.empty_like(rows)
            _under_plan(ops, plan, lambda: ops.gemm(rows, pw, out2, tconv=dict(T=T, HW=HW), residual=r))
            assert torch.equal(out, out2)            # fixed summation order: bitwise reproducible
@pytest.mark.parametrize("M,N,K", [(25600, 512, 320), (20480 + 77, 320, 640), (30000, 448, 192), (131072, 64, 64)])
def test_gemm_plain_large(ops, M, N, K):
    _gemm_plain_large(ops, M, N, K, GEMM_ROUTES[(M, N, K)])


def _gemm_plain_large(ops, M, N, K, routes=None):
    """routes = {plan: (kernel of the bf16 launch, kernel of the fp32 launch)}, as for _conv3x3"""
    x = bf(rnd(M, K, seed=1)); w = rnd(N, K, seed=2, scale=K ** -0.5); b = rnd(N, seed=3)
    res = bf(rnd(M, N, seed=4)); rv = rnd(4, N, seed=5)
    pw = ops.PackedWeight.linear(w, b, DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    rpv = (M + 3) // 4
    ref32 = x.float() @ bf(w).float().t() + b
    ref = ref32 + rv.repeat_interleave(rpv, 0)[:M]
    ref = bf(ref).float() + res.float()
    xd, resd, rvd = x.to(DEV), res.to(DEV), rv.to(DEV)
    for plan, want in (routes or {None: (None, None)}).items():
        out.fill_(7.0)
        _under_plan(ops, plan, lambda: ops.gemm(xd, pw, out, residual=resd, rowvec=rvd, rows_per_vec=rpv))
        assert want[0] is None or _variant(ops) == want[0], (plan, want[0], _variant(ops))
        assert rel_l2(out, ref) < 4e-3
        out32 = torch.empty(M, N, dtype=torch.float32, device=DEV)
        _under_plan(ops, plan, lambda: ops.gemm(xd, pw, out32, alpha=0.25))
        assert want[1] is None or _variant(ops) == want[1], (plan, want[1], _variant(ops))
        assert rel_l2(out32, 0.25 * ref32) < 2e-5


def test_gemm_geglu_large(ops):
    _geglu_routed(ops, 25600 + 33, 128, 512, {19: _P + "<128,geglu>"})        # 101 x 8 = 808 tiles of 64 columns


@pytest.mark.parametrize("cfg", [
    dict(n=32, C=64, Co=256, H=40, W=40, stride=1, pad=1, ups=0),
    dict(n=30, C=128, Co=320, H=33, W=47, stride=1, pad=1, ups=0),      # ragged rows, N=320 (64-wide tiles)
    dict(n=32, C=64, Co=256, H=20, W=20, stride=1, pad=1, ups=1),       # fused nearest x2
    dict(n=32, C=64, Co=256, H=80, W=80, stride=2, pad=1, ups=0),       # stride 2
])
def test_conv3x3_large(ops, cfg):
    _conv3x3(ops, cfg, _conv_routes(cfg))


def test_tconv3_large(ops):
    _tconv3_routed(ops, 2, 16, 1601, 256, 9, {19: _G + "<256,tconv>"})


# ---- 256x320 / 256x256 LDS-DMA tiles (2-stage ring) --------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(51200 + 100, 320, 128), (25600 + 7, 640, 320), (52000, 1280, 64)])
def test_gemm_plain_320_tiles(ops, M, N, K):
    _gemm_plain_large(ops, M, N, K, GEMM_ROUTES[(M, N, K)])


def test_gemm_geglu_256_tile(ops):
    _geglu_routed(ops, 32768 - 19, 128, 512, {19: "gemm_pp_kernel<geglu>", 3: _P + "<256,geglu>"})


@pytest.mark.parametrize("cfg", [
    dict(n=36, C=128, Co=320, H=33, W=47, stride=1, pad=1, ups=0),
    dict(n=32, C=64, Co=640, H=20, W=20, stride=1, pad=1, ups=1),
    dict(n=32, C=64, Co=320, H=81, W=80, stride=2, pad=1, ups=0),
])
def test_conv3x3_320_tiles(ops, cfg):
    _conv3x3(ops, cfg, _conv_routes(cfg))


def test_tconv3_320_tile(ops):
    _tconv3_routed(ops, 2, 16, 1601, 320, 0, {19: _G + "<320,tconv>"})


# ---- persistent cross-tile pipelined GEMM (mode 0, >= 512 output tiles, K <= 1280) --------------------------
@pytest.mark.parametrize("M,N,K", [(65536 + 50, 512, 320), (65536 + 50, 320, 320), (140000, 640, 640), (70000, 448, 64)])
def test_gemm_persistent(ops, M, N, K):
    _gemm_plain_large(ops, M, N, K, GEMM_ROUTES[(M, N, K)])


def test_gemm_geglu_persistent(ops):
    _geglu_routed(ops, 65536 + 21, 320, 640, {19: "gemm_pp_kernel<geglu>", 3: _P + "<256,geglu>"})


@pytest.mark.parametrize("M,N,K", [(140000, 320, 320), (140000, 640, 640), (135000, 960, 128)])
def test_gemm_persistent_320(ops, M, N, K):
    _gemm_plain_large(ops, M, N, K, GEMM_ROUTES[(M, N, K)])


def test_gemm_geglu_persistent_256(ops):
    _geglu_routed(ops, 131072 + 21, 128, 512, {19: "gemm_pp_kernel<geglu>", 3: _P + "<256,geglu>"})


# ---- ragged tile counts for the wide (256 x 320, GEGLU 256 x 256) tiles -------------
@pytest.mark.parametrize("M,N,K", [(18432, 1280, 1280), (4608 + 33, 1280, 640), (73728, 640, 320), (10000, 320, 2560),
                                    (256 * 70, 960, 128)])
def test_gemm_ragged_wide(ops, M, N, K):
    _gemm_plain_large(ops, M, N, K, GEMM_ROUTES[(M, N, K)])


@pytest.mark.parametrize("cfg", [
    dict(n=32, C=128, Co=1280, H=18, W=32, stride=1, pad=1, ups=0),       # 72 row tiles x 4 = 288 tiles
    dict(n=32, C=64, Co=640, H=9, W=16, stride=1, pad=1, ups=0),          # 18 x 2 = 36 tiles
    dict(n=30, C=192, Co=320, H=17, W=23, stride=1, pad=1, ups=0),
    dict(n=32, C=64, Co=640, H=18, W=16, stride=1, pad=1, ups=1),
])
def test_conv3x3_ragged_wide(ops, cfg):
    _conv3x3(ops, cfg, _conv_routes(cfg))


def test_tconv3_ragged_wide(ops):
    _tconv3_routed(ops, 2, 16, 577, 640, 0, {19: _T + "<128>"}, twice=True)        # 73 row tiles x 2: below every large-tile threshold


def test_gemm_geglu_ragged_wide(ops):
    _geglu_routed(ops, 18432 + 5, 256, 1280, {19: "gemm_pp_kernel<geglu>", 3: _P + "<256,geglu>"})


# ---- split-K plans of the 320-wide tile: few tiles (level 3: every tile cut along K) and a little over one wave
# (level 2: 256 whole tiles + the 32-tile remainder cut 8 ways), then the reduce kernel's epilogue
@pytest.mark.parametrize("cfg,res", [
    (dict(n=8, C=1280, Co=1280, H=18, W=32, stride=1, pad=1, ups=0), False),     # 18 x 4 = 72 tiles, 3 splits of 60 K tiles
    (dict(n=8, C=1280, Co=1280, H=18, W=32, stride=1, pad=1, ups=0), True),
    (dict(n=32, C=1280, Co=1280, H=18, W=32, stride=1, pad=1, ups=0), True),     # 288 tiles: 256 whole + 32 x 8 splits
])
def test_conv3x3_splitk(ops, cfg, res):
    n, C, Co, H, W = (cfg[k] for k in ("n", "C", "Co", "H", "W"))
    x = bf(rnd(n, C, H, W, seed=1)); w = rnd(Co, C, 3, 3, seed=2, scale=(9 * C) ** -0.5); b = rnd(Co, seed=3)
    ref = F.conv2d(x.float(), bf(w).float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    r = bf(rnd(n * H * W, Co, seed=4)) if res else None
    if res:
        ref = bf(ref).float() + r.float()
    pw = ops.PackedWeight.conv3x3(w, b, DEV)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    rd = None if r is None else r.to(DEV)
    for plan, want in _conv_routes(cfg).items():            # the one-wave kernel's split-K plan, and the 8-wave tile's under plan 0
        outs = []
        for _ in range(2):
            out = torch.empty(n * H * W, Co, dtype=torch.bfloat16, device=DEV)
            _under_plan(ops, plan, lambda: ops.gemm(rows, pw, out, conv=dict(IH=H, IW=W, OH=H, OW=W, stride=1, pad=1, ups=0), residual=rd))
            assert _variant(ops) == want, (plan, want, _variant(ops))
            outs.append(out)
        assert rel_l2(outs[0], ref) < 4e-3
        assert torch.equal(outs[0], outs[1])                # fixed summation order: bitwise reproducible


def test_tconv3_splitk(ops):
    # M = 4608: 72 tiles, K = 3840 (60 K tiles) -> 3 splits; on the one-wave kernel by default (K >= 1920)
    _tconv3_routed(ops, 2, 4, 576, 1280, 0, {19: _PIPE + "<tconv>+splitk", 0: _G + "<320,tconv>+splitk"})


# ---- persistent 256 x 320 kernel in conv / temporal-conv mode (>= 512 tiles, K <= 2880)
@pytest.mark.parametrize("cfg", [
    dict(n=16, C=128, Co=320, H=96, W=96, stride=1, pad=1, ups=0),        # 576 tiles, 18 K tiles
    dict(n=15, C=64, Co=320, H=97, W=101, stride=1, pad=1, ups=0),        # ragged rows
    dict(n=16, C=64, Co=320, H=192, W=192, stride=2, pad=1, ups=0),       # stride 2
    dict(n=16, C=64, Co=320, H=192, W=192, stride=2, pad=0, ups=0),       # AE-style asymmetric pad
])
def test_conv3x3_persistent(ops, cfg):
    _conv3x3(ops, cfg, _conv_routes(cfg))


def test_conv3x3_persistent_residual_rowvec(ops):
    n, C, Co, H, W = 16, 64, 640, 96, 96                   # 2 N tiles per row tile
    x = bf(rnd(n, C, H, W, seed=1)); w = rnd(Co, C, 3, 3, seed=2, scale=(9 * C) ** -0.5); b = rnd(Co, seed=3)
    emb = rnd(n // 4, Co, seed=5)                            # one vector per 4 frames
    r = bf(rnd(n * H * W, Co, seed=4))
    ref = F.conv2d(x.float(), bf(w).float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    ref = ref + emb.repeat_interleave(4 * H * W, 0)
    ref = bf(ref).float() + r.float()
    pw = ops.PackedWeight.conv3x3(w, b, DEV)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    rd, embd = r.to(DEV), emb.to(DEV)
    # 576 x 2 = 1152 tiles: the persistent conv kernel where the one-wave kernel is off (plan 0); the one-wave kernel by default
    for plan, want in {19: _PIPE + "<conv>", 0: _P + "<320,conv>"}.items():
        out = torch.empty(n * H * W, Co, dtype=torch.bfloat16, device=DEV)
        _under_plan(ops, plan, lambda: ops.gemm(rows, pw, out, conv=dict(IH=H, IW=W, OH=H, OW=W, stride=1, pad=1, ups=0), residual=rd,
                                                rowvec=embd, rows_per_vec=4 * H * W))
        assert _variant(ops) == want, (plan, want, _variant(ops))
        assert rel_l2(out, ref) < 4e-3


@pytest.mark.parametrize("B,T,HW", [(2, 16, 4608), (3, 5, 9830)])
def test_tconv3_persistent(ops, B, T, HW):
    _tconv3_routed(ops, B, T, HW, 320, 4, {19: _P + "<320,tconv>"})


# ---- the one-wave-per-SIMD 320-wide kernel (gemm_pipe16.h) behind dc_gemm_set_plan: same shapes, same checkers (plan 1: convs
# only, 3 = default: + long-K plain / temporal launches, 0: the 8-wave kernels; 9 / 11 are the older spellings of 1 / 3)
@pytest.fixture
def gemm_plan(ops, request):
    lib = ops._hip.lib()
    prev = lib.dc_gemm_set_plan(request.param)
    assert prev >= 0
    yield request.param
    lib.dc_gemm_set_plan(prev)


def _variant(ops):
    return ops._hip.lib().dc_gemm_last_variant().decode()


PIPE_CONVS = [
    (dict(n=8, C=1280, Co=1280, H=18, W=32, stride=1, pad=1, ups=0), True),       # 72 tiles: every tile cut 3 ways along K
    (dict(n=32, C=640, Co=1280, H=18, W=32, stride=1, pad=1, ups=0), False),      # 288 tiles: 256 whole + 32 x 8 splits
    (dict(n=32, C=320, Co=640, H=36, W=64, stride=1, pad=1, ups=0), True),        # 576 tiles: 512 whole + 64 x 4
    (dict(n=30, C=192, Co=320, H=17, W=23, stride=1, pad=1, ups=0), False),       # ragged rows, odd image width, 3 slices
    (dict(n=3, C=64, Co=320, H=130, W=135, stride=1, pad=1, ups=0), True),        # wide image, one channel slice
    (dict(n=36, C=128, Co=320, H=33, W=47, stride=1, pad=1, ups=0), False),
]


@pytest.mark.parametrize("gemm_plan", [1, 9], indirect=True)
@pytest.mark.parametrize("cfg,res", PIPE_CONVS)
def test_conv3x3_pipe_plans(ops, gemm_plan, cfg, res):
    n, C, Co, H, W = (cfg[k] for k in ("n", "C", "Co", "H", "W"))
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(n, C, H, W, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(Co, C, 3, 3, device=DEV, generator=g) * (9 * C) ** -0.5
    b = torch.randn(Co, device=DEV, generator=g)
    emb = torch.randn(n, Co, device=DEV, generator=g)                 # one vector per image (ResBlock emb_layers)
    r = torch.randn(n * H * W, Co, device=DEV, generator=g).to(torch.bfloat16) if res else None
    ref = F.conv2d(x.float(), w.to(torch.bfloat16).float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    ref = ref + emb.repeat_interleave(H * W, 0)
    if res:
        ref = ref.to(torch.bfloat16).float() + r.float()
    pw = ops.PackedWeight.conv3x3(w.cpu(), b.cpu(), DEV)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    outs = []
    for _ in range(2):
        out = torch.empty(n * H * W, Co, dtype=torch.bfloat16, device=DEV)
        ops.gemm(rows, pw, out, conv=dict(IH=H, IW=W, OH=H, OW=W, stride=1, pad=1, ups=0), residual=r, rowvec=emb, rows_per_vec=H * W)
        outs.append(out)
    want = "gemm_pipe320x16"
    assert want in _variant(ops), _variant(ops)
    assert rel_l2(outs[0], ref) < 4e-3
    assert torch.equal(outs[0], outs[1])                             # fixed summation order: bitwise reproducible


# ---- "whole waves + split remainder" as ONE launch (GemmSplit::whole, the default) against the two-launch form (plan bit 6):
# the same tiles, K ranges and summation order, so the outputs are bit-identical
@pytest.mark.parametrize("cfg,res", [PIPE_CONVS[1], PIPE_CONVS[2],
                                     (dict(n=32, C=640, Co=640, H=18, W=32, stride=1, pad=1, ups=1), False)])
def test_pipe_merged_split_launch_bitwise(ops, cfg, res):
    lib = ops._hip.lib()
    n, C, Co, H, W, ups = (cfg[k] for k in ("n", "C", "Co", "H", "W", "ups"))
    OH, OW = (2 * H, 2 * W) if ups else (H, W)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(n, C, H, W, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(Co, C, 3, 3, device=DEV, generator=g) * (9 * C) ** -0.5
    b = torch.randn(Co, device=DEV, generator=g)
    r = torch.randn(n * OH * OW, Co, device=DEV, generator=g).to(torch.bfloat16) if res else None
    xin = F.interpolate(x.float(), scale_factor=2, mode="nearest") if ups else x.float()
    ref = F.conv2d(xin, w.to(torch.bfloat16).float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    if res:
        ref = ref.to(torch.bfloat16).float() + r.float()
    pw = ops.PackedWeight.conv3x3(w.cpu(), b.cpu(), DEV)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    outs = {}
    for plan in (19, 19 | 64):
        prev = lib.dc_gemm_set_plan(plan)
        assert prev >= 0
        try:
            out = torch.empty(n * OH * OW, Co, dtype=torch.bfloat16, device=DEV)
            ops.gemm(rows, pw, out, conv=dict(IH=H, IW=W, OH=OH, OW=OW, stride=1, pad=1, ups=ups), residual=r)
            assert "gemm_pipe320x16" in _variant(ops) and "+splitk" in _variant(ops), _variant(ops)
            outs[plan] = out
        finally:
            lib.dc_gemm_set_plan(prev)
    assert rel_l2(outs[19], ref) < 4e-3
    assert torch.equal(outs[19], outs[19 | 64])
    torch.cuda.synchronize()
    ops._hip.check_error_word("merged split launch")


@pytest.mark.parametrize("gemm_plan", [3, 0], indirect=True)
@pytest.mark.parametrize("cfg", [
    dict(n=32, C=1280, Co=1280, H=9, W=16, stride=1, pad=1, ups=1),          # level 3 -> 2 Upsample: 72 tiles, split-K
    dict(n=32, C=640, Co=640, H=18, W=32, stride=1, pad=1, ups=1),           # 288 x 2 tiles
    dict(n=15, C=64, Co=320, H=33, W=27, stride=1, pad=1, ups=1),            # odd sizes: every parity / border combination, ragged rows
])
def test_conv3x3_upsample_fused_pipe16(ops, gemm_plan, cfg):
    test_conv3x3(ops, cfg)
    if gemm_plan == 3:                         # (n = 15: 209 row tiles -> whole 320-wide tiles)
        assert "gemm_pipe320x16_kernel<conv,ups>" in _variant(ops), _variant(ops)


@pytest.mark.parametrize("gemm_plan", [3], indirect=True)
def test_gemm_and_tconv_pipe_plan(ops, gemm_plan):
    # plain rows (K = 2560, split-K plan of 72 tiles) and the temporal 3-tap mode of the same kernel
    _gemm_plain_large(ops, 4608 + 33, 1280, 2560)
    assert "gemm_pipe320" in _variant(ops) or "gemm_persist" in _variant(ops) or "glds" in _variant(ops)
    M, N, K = 18432, 1280, 5120
    x = bf(rnd(M, K, seed=1)); w = rnd(N, K, seed=2, scale=K ** -0.5); b = rnd(N, seed=3)
    pw = ops.PackedWeight.linear(w, b, DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x.to(DEV), pw, out)
    assert "gemm_pipe320" in _variant(ops), _variant(ops)
    assert rel_l2(out, x.float() @ bf(w).float().t() + b) < 4e-3
    _tconv3_routed(ops, 2, 4, 576, 1280, 0, None)
    assert "gemm_pipe320" in _variant(ops), _variant(ops)
    _tconv3_routed(ops, 2, 16, 577, 640, 0, None, twice=True)


# ---- conv_in as im2col (9 taps x 8 channels -> one 128-wide K) + plain GEMM, against torch and against the implicit-GEMM conv
@pytest.mark.parametrize("n,ci,H,W", [(3, 8, 17, 23), (32, 8, 32, 32), (2, 5, 9, 40)])
def test_conv_in_im2col_c8(ops, n, ci, H, W):
    g = torch.Generator().manual_seed(23)
    Co = 320
    x = torch.randn(n, ci, H, W, generator=g).to(torch.bfloat16)
    w = torch.randn(Co, ci, 3, 3, generator=g) * (9 * ci) ** -0.5
    b = torch.randn(Co, generator=g)
    ref = F.conv2d(x.float(), bf(w).float(), b, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    rows = torch.zeros(n * H * W, 64, dtype=torch.bfloat16)                    # the x_rows layout: 8 channels in a 64-wide row
    rows[:, :ci] = x.permute(0, 2, 3, 1).reshape(-1, ci)
    rows = rows.to(DEV)
    cols = torch.full((n * H * W, 128), 7.0, dtype=torch.bfloat16, device=DEV)  # every element must be overwritten
    ops.im2col3x3_c8(rows, cols, n_img=n, H=H, W=W)
    assert cols[:, 72:].abs().max().item() == 0
    pw = ops.PackedWeight.conv3x3_c8_as_linear(w, b, DEV)
    out = torch.empty(n * H * W, Co, dtype=torch.bfloat16, device=DEV)
    ops.gemm(cols, pw, out)
    assert rel_l2(out, ref) < 4e-3
    out2 = torch.empty_like(out)
    ops.gemm(rows, ops.PackedWeight.conv3x3(w, b, DEV), out2, conv=dict(IH=H, IW=W, OH=H, OW=W, stride=1, pad=1, ups=0))
    assert rel_l2(out, out2) < 3e-3                                            # same products, another summation order


# ---- the ping-pong kernel (gemm_pp.h: 4-wave workgroups, two per CU, GEGLU formed in registers) behind plan bit 4 (16: default,
# K <= 640) and bit 5 (32: any K)
@pytest.mark.parametrize("gemm_plan", [51, 19, 3], indirect=True)
@pytest.mark.parametrize("M,dim,inner", [
    (73728, 640, 2560),        # level 1 of the 1024 config: 288 x 40 tiles, 10 K tiles
    (18432, 1280, 5120),       # level 2: 72 x 80 tiles, 20 K tiles
    (4608, 1280, 5120),        # level 3: 18 x 80 tiles
    (16384 + 77, 192, 1024),   # ragged rows, 3 K tiles (K range shorter than the weight ring)
    (32768, 128, 512),         # 2 K tiles
])
def test_gemm_geglu_pingpong(ops, gemm_plan, M, dim, inner):
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, dim, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(2 * inner, dim, device=DEV, generator=g) * dim ** -0.5)
    b = torch.randn(2 * inner, device=DEV, generator=g) * 0.1
    pw = ops.PackedWeight.linear(w.cpu(), b.cpu(), DEV)
    big = torch.zeros(M, inner + 64, dtype=torch.bfloat16, device=DEV)            # strided output view (ldc > width)
    outs = []
    for _ in range(2):
        out = big[:, 64:] if not outs else torch.empty(M, inner, dtype=torch.bfloat16, device=DEV)
        ops.gemm(x, pw, out, geglu=True)
        outs.append(out)
    v = _variant(ops)
    assert ("gemm_pp_kernel<geglu>" in v) == (gemm_plan == 51 or (gemm_plan == 19 and dim <= 640)), v
    h = x.float() @ w.to(torch.bfloat16).float().t() + b
    val, gate = h.chunk(2, dim=-1)
    ref = val * F.gelu(gate)
    assert rel_l2(outs[0], ref) < 4e-3
    assert torch.equal(outs[0], outs[1])                                           # bitwise reproducible, any output stride
    assert big[:, :64].abs().max().item() == 0
    from dynamicrafter_amd import _hip
    _hip.check_error_word("gemm_pp")


def test_gelu_phi_error(ops):
    """The GEMM epilogues' GELU is x * Phi(x) with a clamped degree-6 polynomial for Phi (csrc/dc_common.h: gelu_phi_f) instead
    of erf: max |error| against torch's erf GELU <= 2.5e-4 over the whole range the kernel can see (stated 1.9e-4 + the bf16
    rounding of the test's own output), exactly x / exactly 0 beyond |x| = 4. Measured through the GELU epilogue of dc_gemm_conv
    with an identity weight: out = gelu(x)."""
    K = 64
    xs = torch.linspace(-12, 12, 256 * 1024, dtype=torch.float32)
    x = torch.zeros(xs.numel() // K, K)
    x[:] = xs.view(-1, K)
    xb = bf(x)
    pw = ops.PackedWeight.linear(torch.eye(K), torch.zeros(K), DEV)
    out = torch.empty(x.shape[0], K, dtype=torch.float32, device=DEV)
    ops.gemm(xb.to(DEV), pw, out, gelu=True)
    ref = F.gelu(xb.double())
    err = (out.double().cpu() - ref).abs()
    print(f"\n[gelu_phi] max |gelu_phi - gelu_erf| = {err.max().item():.3e} at x = {xb.flatten()[err.argmax()].item():.3f}")
    assert err.max().item() < 2.5e-4
    far = xb.flatten().abs() > 4.0
    o = out.cpu().flatten()
    assert torch.equal(o[far & (xb.flatten() > 0)], xb.flatten()[far & (xb.flatten() > 0)].float())
    assert o[far & (xb.flatten() < 0)].abs().max().item() == 0.0


# ---- dispatch fuzz: random shapes across the tile / persistent / split-K decision boundaries. The checker is a
# device-side fp32 matmul / conv (rocBLAS / MIOpen via torch) - CPU references of these sizes would take minutes.
def _fuzz_cases():
    import random
    rng = random.Random(1234)
    Ns = [64, 128, 256, 320, 512, 640, 960, 1280, 1920, 2560]
    cases = []
    for i in range(28):
        N = rng.choice(Ns)
        K = 64 * rng.choice([1, 2, 5, 8, 10, 20, 30, 40, 60])
        M = rng.choice([rng.randint(1, 4000), rng.randint(4000, 40000), rng.randint(40000, 160000)])
        cases.append((M, N, K, rng.random() < 0.4, rng.random() < 0.8, i))
    return cases


@pytest.mark.parametrize("M,N,K,res,bias,seed", _fuzz_cases())
def test_gemm_dispatch_fuzz(ops, M, N, K, res, bias, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5)
    b = torch.randn(N, device=DEV, generator=g) if bias else None
    r = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16) if res else None
    pw = ops.PackedWeight.linear(w.cpu(), None if b is None else b.cpu(), DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x, pw, out, residual=r)
    ref = x.float() @ w.to(torch.bfloat16).float().t()
    if b is not None:
        ref = ref + b
    if r is not None:
        ref = ref.to(torch.bfloat16).float() + r.float()
    assert rel_l2(out, ref) < 4e-3, ops._hip.lib().dc_gemm_last_variant().decode()


@pytest.mark.parametrize("n,C,Co,H,W,stride,seed", [
    (5, 64, 320, 40, 64, 1, 0), (32, 320, 320, 40, 64, 1, 1), (32, 640, 640, 20, 32, 1, 2), (32, 1280, 1280, 10, 16, 1, 3),
    (32, 1280, 1280, 5, 8, 1, 4), (32, 320, 320, 40, 64, 2, 5), (32, 640, 1280, 20, 32, 1, 6), (7, 1920, 640, 23, 31, 1, 7),
    (2, 2560, 1280, 18, 32, 1, 8), (33, 960, 320, 17, 29, 1, 9)])
def test_conv_dispatch_fuzz(ops, n, C, Co, H, W, stride, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, C, H, W, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(Co, C, 3, 3, device=DEV, generator=g) * (9 * C) ** -0.5
    b = torch.randn(Co, device=DEV, generator=g)
    ref = F.conv2d(x.float(), w.to(torch.bfloat16).float(), b, stride=stride, padding=1)
    OH, OW = ref.shape[2], ref.shape[3]
    pw = ops.PackedWeight.conv3x3(w.cpu(), b.cpu(), DEV)
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    out = torch.empty(n * OH * OW, Co, dtype=torch.bfloat16, device=DEV)
    ops.gemm(rows, pw, out, conv=dict(IH=H, IW=W, OH=OH, OW=OW, stride=stride, pad=1, ups=0))
    want = ref.permute(0, 2, 3, 1).reshape(-1, Co)
    assert rel_l2(out, want) < 4e-3, ops._hip.lib().dc_gemm_last_variant().decode()


@pytest.mark.parametrize("B,heads,L,d,causal", [(2, 16, 257, 80, False), (3, 16, 77, 64, True), (1, 3, 40, 6, True),
                                                (1, 2, 500, 64, False)])
def test_attn_small_vs_torch(ops, B, heads, L, d, causal):
    """dc_attn_small (CLIP towers: any head width, optional causal mask) against fp32 softmax attention."""
    g = torch.Generator().manual_seed(5)
    D = heads * d
    Dp = (D + 7) // 8 * 8
    qkv = (torch.randn(B * L, 3 * Dp, generator=g)).to(torch.bfloat16).to(DEV)
    q, k, v = qkv[:, :D], qkv[:, Dp:Dp + D], qkv[:, 2 * Dp:2 * Dp + D]
    o = torch.zeros(B * L, Dp, dtype=torch.bfloat16, device=DEV)
    ops.attn_small(q, k, v, o, batch=B, heads=heads, Lq=L, Lk=L, d=d, scale=d ** -0.5, causal=causal)
    sp = lambda t: t.float().cpu().reshape(B, L, heads, d).transpose(1, 2)
    s = (sp(q) * d ** -0.5) @ sp(k).transpose(-1, -2)
    if causal:
        s = s + torch.full((L, L), float("-inf")).triu_(1)
    ref = (s.softmax(-1) @ sp(v)).transpose(1, 2).reshape(B * L, D)
    assert rel_l2(o[:, :D], ref) < 6e-3


def test_clip_preprocess_patchify_embed_vs_oracle(ops):
    from oracle import clip as oclip
    g = torch.Generator().manual_seed(6)
    for shape in ((2, 3, 320, 512), (1, 3, 576, 1024), (1, 3, 224, 224), (1, 3, 200, 180)):
        img = (torch.rand(*shape, generator=g) * 2 - 1)
        out = ops.clip_preprocess(img.to(DEV))
        ref = oclip.preprocess(img)
        assert tuple(out.shape) == tuple(ref.shape)
        assert ((out.cpu() - ref).abs().max() / ref.abs().max()).item() < 1e-4, shape      # fp32 both; __expf taps, summation order
    img = torch.randn(2, 3, 28, 42, generator=g)
    rows = torch.empty(2 * 2 * 3, 640, dtype=torch.bfloat16, device=DEV)
    ops.patchify(img.to(DEV), rows, patch=14)
    ref = torch.nn.functional.unfold(img, 14, stride=14).transpose(1, 2).reshape(12, 588)
    assert torch.equal(rows[:, :588].float().cpu(), ref.to(torch.bfloat16).float())
    assert float(rows[:, 588:].float().abs().max()) == 0.0
    table = torch.randn(50, 64, generator=g).to(torch.bfloat16)
    pos = torch.randn(7, 64, generator=g).to(torch.bfloat16)
    tok = torch.randint(0, 50, (3, 7), generator=g)
    out = torch.empty(21, 64, dtype=torch.bfloat16, device=DEV)
    ops.embed_tokens(tok.to(DEV), table.to(DEV), pos.to(DEV), out)
    ref = (table.float()[tok] + pos.float()).reshape(21, 64).to(torch.bfloat16)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("B,heads,Lq,nt,ni,s2", [(3, 5, 300, 77, 16, 1.0), (2, 2, 70, 77, 16, 1.7), (1, 20, 144, 5, 3, 0.4),
                                                 # Lq >= 512, 64 < Lk <= 96, Lk2 <= 32: the keys-resident kernel (several query tiles per
                                                 # workgroup under one staging of both sets): level 0 / 1 / 2 of the 1024 config, ragged rows
                                                 (4, 5, 9216, 77, 16, 1.0), (3, 10, 2304, 77, 16, 0.7), (2, 20, 576, 77, 16, 1.3),
                                                 (2, 3, 1000, 90, 32, 0.5), (1, 2, 640, 65, 1, 1.0)])
def test_cross_attn_dual_vs_torch(ops, B, heads, Lq, nt, ni, s2):
    """Text + image cross-attention with separate softmaxes in one launch (attention.py:128-142) vs fp32 torch, and vs the
    two-launch form (text pass, then accumulate the image pass)."""
    g = torch.Generator().manual_seed(9)
    Cc, Lc = heads * 64, nt + ni
    q = torch.randn(B * Lq, Cc, generator=g).to(torch.bfloat16).to(DEV)
    kv = torch.randn(B * Lc, 4 * Cc, generator=g).to(torch.bfloat16).to(DEV)
    o = torch.empty(B * Lq, Cc, dtype=torch.bfloat16, device=DEV)
    ops.cross_attn_dual(q, kv[:, :Cc], kv[:, Cc:2 * Cc], kv[nt:, 2 * Cc:3 * Cc], kv[nt:, 3 * Cc:], o, batch=B, heads=heads,
                        Lq=Lq, Lk=nt, Lk2=ni, scale=0.125, scale2=s2, kv_bstride=Lc)
    qf = q.float().cpu().reshape(B, Lq, Cc)
    kvf = kv.float().cpu().reshape(B, Lc, 4 * Cc)
    ref = (_attn_ref(qf, kvf[:, :nt, :Cc], kvf[:, :nt, Cc:2 * Cc], heads, 0.125)
           + s2 * _attn_ref(qf, kvf[:, nt:, 2 * Cc:3 * Cc], kvf[:, nt:, 3 * Cc:], heads, 0.125))
    assert rel_l2(o, ref.reshape(B * Lq, Cc)) < 6e-3
    o2 = torch.empty_like(o)
    ops.flash_attn(q, kv[:, :Cc], kv[:, Cc:2 * Cc], o2, batch=B, heads=heads, Lq=Lq, Lk=nt, scale=0.125, kv_bstride=Lc)
    ops.flash_attn(q, kv[nt:, 2 * Cc:3 * Cc], kv[nt:, 3 * Cc:], o2, batch=B, heads=heads, Lq=Lq, Lk=ni, scale=0.125,
                   kv_bstride=Lc, accumulate=True, acc_scale=s2)
    assert rel_l2(o, o2) < 6e-3


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(128, 320, 320), (40000, 960, 320), (333, 64, 320), (73728, 1920, 640), (300, 96, 640),
                                   (4096, 640, 640)])
def test_ln_linear_vs_layernorm_plus_gemm(ops, M, N, K):
    """dc_ln_linear = dc_layernorm + dc_gemm_conv (same rounding points) and = torch fp32 LayerNorm + Linear"""
    g = torch.Generator().manual_seed(M + N)
    x = (torch.randn(M, K, generator=g) * 1.3 + 0.4).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    gam = 1 + 0.2 * torch.randn(K, generator=g); bet = 0.3 * torch.randn(K, generator=g)
    for bias in (None, b):
        pw = ops.PackedWeight.linear(w, bias, DEV)
        xd = x.to(DEV)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        ops.ln_linear(xd, pw, out, ln=(gam.to(DEV), bet.to(DEV)))
        n = torch.empty_like(xd)
        ops.layernorm(xd, n, gam.to(DEV), bet.to(DEV), 1e-5)
        want = torch.empty_like(out)
        ops.gemm(n, pw, want)
        assert rel_l2(out, want) < 2e-3
        ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(x.float(), (K,), gam, bet, 1e-5), w, bias)
        assert rel_l2(out.float().cpu(), ref) < 6e-3
        # without the LayerNorm it is the plain Linear
        ops.ln_linear(xd, pw, out)
        ops.gemm(xd, pw, want)
        assert rel_l2(out, want) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(4096, 320, 320), (1000, 320, 320), (3333, 64, 320), (36864, 640, 640), (777, 640, 640),
                                   (131, 1280, 640)])
def test_linear_residual_vs_gemm_with_residual(ops, M, N, K):
    """dc_linear_residual (X-stationary kernel, residual fetched in the stores' pattern and added in fp32) = dc_gemm_conv with
    a residual operand (bit for bit: same fp32 sum, one rounding) = torch fp32; in place (residual is the output buffer), into
    a column slice of a wider buffer, and with a ragged last tile."""
    g = torch.Generator().manual_seed(M * 3 + N)
    x = (torch.randn(M, K, generator=g)).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    r = (torch.randn(M, N, generator=g) * 2).to(torch.bfloat16)
    ref = r.float() + torch.nn.functional.linear(x.float(), w, b)
    pw = ops.PackedWeight.linear(w, b, DEV)
    xd, rd = x.to(DEV), r.to(DEV)
    want = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm(xd, pw, want, residual=rd)
    out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.linear_residual(xd, pw, rd, out)
    e_new, e_old, d = rel_l2(out.float().cpu(), ref), rel_l2(want.float().cpu(), ref), rel_l2(out, want)
    print(f"\n[linear_residual {M}x{N}x{K}] vs fp32: X-stationary {e_new:.2e}, tile GEMM {e_old:.2e}; between them {d:.2e}")
    assert e_new < 2.6e-3                                # one bf16 rounding of the fp32 sum (measured 1.7e-3)
    assert d < 3e-3                                      # two roundings of sums that differ in the order of the fp32 adds
    inplace = rd.clone()
    ops.linear_residual(xd, pw, inplace, inplace)
    assert torch.equal(inplace, out)
    wide = torch.full((M, N + 64), 3.0, dtype=torch.bfloat16, device=DEV)
    ops.linear_residual(xd, pw, rd, wide[:, 32:32 + N])
    assert torch.equal(wide[:, 32:32 + N], out) and (wide[:, :32] == 3).all() and (wide[:, 32 + N:] == 3).all()
    pw0 = ops.PackedWeight.linear(w, None, DEV)
    ops.linear_residual(xd, pw0, rd, out)
    assert rel_l2(out.float().cpu(), r.float() + torch.nn.functional.linear(x.float(), w)) < 4e-3


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst,rpi,N,K", [(3, 256, 320, 320), (2, 9216, 320, 320), (5, 128, 64, 320), (32, 2304, 640, 640),
                                             (3, 384, 96, 640)])
def test_gn_linear_vs_groupnorm_plus_gemm(ops, n_inst, rpi, N, K):
    """dc_groupnorm_stats + dc_gn_linear = dc_groupnorm + dc_gemm_conv (same rounding points) = torch fp32 reference"""
    g = torch.Generator().manual_seed(n_inst * rpi + N)
    M = n_inst * rpi
    x = (torch.randn(M, K, generator=g) * (1 + torch.arange(K) % 7 * 0.3) + 0.5).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    gam = (1 + 0.2 * torch.randn(K, generator=g)).to(DEV); bet = (0.3 * torch.randn(K, generator=g)).to(DEV)
    pw = ops.PackedWeight.linear(w, b, DEV)
    xd = x.to(DEV)
    st = torch.empty(n_inst * 32 * 2, dtype=torch.float32, device=DEV)
    ops.groupnorm_stats(xd, st, groups=32, n_inst=n_inst, rows_per_inst=rpi, eps=1e-6)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gn_linear(xd, gam, bet, st, pw, out, groups=32, rows_per_inst=rpi)
    n = torch.empty_like(xd)
    ops.groupnorm(xd, n, gam, bet, groups=32, n_inst=n_inst, rows_per_inst=rpi, eps=1e-6, silu=False)
    want = torch.empty_like(out)
    ops.gemm(n, pw, want)
    assert rel_l2(out, want) < 2e-3
    xf = x.float().reshape(n_inst, rpi, K).permute(0, 2, 1)
    ref = torch.nn.functional.group_norm(xf, 32, gam.cpu(), bet.cpu(), 1e-6).permute(0, 2, 1).reshape(M, K)
    ref = torch.nn.functional.linear(ref, w, b)
    assert rel_l2(out.float().cpu(), ref) < 6e-3
    with pytest.raises(ValueError):
        ops.gn_linear(xd, gam, bet, st, pw, out, groups=32, rows_per_inst=rpi + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("B,HW,C", [(1, 8, 320), (2, 72, 320), (2, 2304, 320), (1, 8, 640), (2, 72, 640), (2, 2304, 640)])
def test_ln_qkv_temporal_attn320_vs_three_kernels(ops, B, HW, C):
    """dc_ln_qkv_temporal_attn320 / 640 = dc_layernorm -> dc_gemm_conv (qkv) -> dc_temporal_attn_d64, and = torch fp32"""
    g = torch.Generator().manual_seed(B * HW + C)
    T, heads = 16, C // 64
    M = B * T * HW
    x = (torch.randn(M, C, generator=g) * 1.2 + 0.3).to(torch.bfloat16)
    w = torch.randn(3 * C, C, generator=g) * C ** -0.5 * 1.5
    gam = 1 + 0.2 * torch.randn(C, generator=g); bet = 0.3 * torch.randn(C, generator=g)
    pw = ops.PackedWeight.linear(w, None, DEV)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    out = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
    ops.ln_qkv_temporal_attn(xd, (gd, bd), pw, out, B=B, T=T, HW=HW, scale=0.125)
    n = torch.empty_like(xd)
    ops.layernorm(xd, n, gd, bd, 1e-5)
    qkv = torch.empty(M, 3 * C, dtype=torch.bfloat16, device=DEV)
    ops.gemm(n, pw, qkv)
    want = torch.empty_like(out)
    ops.temporal_attn(qkv, want, B=B, T=T, HW=HW, heads=heads, scale=0.125)
    assert rel_l2(out, want) < 4e-3
    # torch fp32: rows (b, t, p) -> per (b, p, head) attention over t
    nf = torch.nn.functional.layer_norm(x.float(), (C,), gam, bet, 1e-5)
    q, k, v = (nf @ w.t()).reshape(B, T, HW, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)  # [3][B, HW, heads, T, 64]
    a = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v                   # [B, HW, heads, T, 64]
    ref = a.permute(0, 3, 1, 2, 4).reshape(M, C)
    assert rel_l2(out.float().cpu(), ref) < 1e-2
    with pytest.raises(ValueError):
        ops.ln_qkv_temporal_attn(xd, (gd, bd), pw, xd, B=B, T=T, HW=HW, scale=0.125)


@pytest.mark.gpu
@pytest.mark.parametrize("B,HW,C", [(1, 8, 320), (2, 72, 320), (2, 2304, 320), (2, 2304, 640), (1, 40, 640)])
def test_gn_silu_tconv3_vs_groupnorm_plus_tconv(ops, B, HW, C):
    """dc_groupnorm_stats + dc_gn_silu_tconv3 = dc_groupnorm(silu) + dc_gemm_conv(tconv) (+ residual), and = torch fp32
    GroupNorm -> SiLU -> Conv3d (3,1,1)"""
    g = torch.Generator().manual_seed(7 * B + HW)
    T = 16
    M = B * T * HW
    x = (torch.randn(M, C, generator=g) * (1 + torch.arange(C) % 5 * 0.4) + 0.3).to(torch.bfloat16)
    w = torch.randn(C, C, 3, 1, 1, generator=g) * (3 * C) ** -0.5
    bias = torch.randn(C, generator=g) * 0.1
    res = torch.randn(M, C, generator=g).to(torch.bfloat16)
    gam = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV); bet = (0.3 * torch.randn(C, generator=g)).to(DEV)
    pw = ops.PackedWeight.tconv3(w, bias, DEV)
    xd, rd = x.to(DEV), res.to(DEV)
    st = torch.empty(B * 32 * 2, dtype=torch.float32, device=DEV)
    ops.groupnorm_stats(xd, st, groups=32, n_inst=B, rows_per_inst=T * HW, eps=1e-5)
    n = torch.empty_like(xd)
    ops.groupnorm(xd, n, gam, bet, groups=32, n_inst=B, rows_per_inst=T * HW, eps=1e-5, silu=True)
    for residual in (None, rd):
        out = torch.empty(M, C, dtype=torch.bfloat16, device=DEV)
        ops.gn_silu_tconv3(xd, gam, bet, st, pw, out, B=B, T=T, HW=HW, residual=residual)
        want = torch.empty_like(out)
        ops.gemm(n, pw, want, tconv=dict(T=T, HW=HW), residual=residual)
        assert rel_l2(out, want) < 3e-3
    x5 = x.float().reshape(B, T, HW, C).permute(0, 3, 1, 2)                            # [B, C, T, HW]
    a = torch.nn.functional.silu(torch.nn.functional.group_norm(x5, 32, gam.cpu(), bet.cpu(), 1e-5))
    ref = torch.nn.functional.conv3d(a.unsqueeze(-1), w, bias, padding=(1, 0, 0)).squeeze(-1)      # [B, C, T, HW]
    ref = ref.permute(0, 2, 3, 1).reshape(M, C) + res.float()
    assert rel_l2(out.float().cpu(), ref) < 8e-3


@pytest.mark.parametrize("M", [128 * 5, 1000, 40000])
def test_ff_geglu_fused320_vs_torch(ops, M):
    """ff1 -> GEGLU -> ff2 (+ residual) in one kernel (dim 320) vs fp32 torch and vs the two-GEMM path."""
    g = torch.Generator().manual_seed(21)
    w1 = torch.randn(2560, 320, generator=g) * 320 ** -0.5
    b1 = torch.randn(2560, generator=g) * 0.1
    w2 = torch.randn(320, 1280, generator=g) * 1280 ** -0.5
    b2 = torch.randn(320, generator=g) * 0.1
    x = bf(torch.randn(M, 320, generator=g))
    res = bf(torch.randn(M, 320, generator=g))
    pw1 = ops.PackedWeight.linear(w1, b1, DEV)
    pw2 = ops.PackedWeight.linear(w2, b2, DEV)
    w2p = ops.ff2_permuted(w2, DEV)
    out = torch.empty(M, 320, dtype=torch.bfloat16, device=DEV)
    ops.ff_geglu_fused320(x.to(DEV), pw1, w2p, pw2.bias, out, residual=res.to(DEV))
    xf = x.float()
    hmid = xf @ bf(w1).float().T + b1
    val, gate = hmid[:, :1280], hmid[:, 1280:]
    ref = (bf(val * F.gelu(gate)).float() @ bf(w2).float().T + b2) + res.float()
    assert rel_l2(out, ref) < 4e-3
    mid = torch.empty(M, 1280, dtype=torch.bfloat16, device=DEV)
    ops.gemm(x.to(DEV), pw1, mid, geglu=True)
    out2 = torch.empty_like(out)
    ops.gemm(mid, pw2, out2, residual=res.to(DEV))
    assert rel_l2(out, out2) < 4e-3
    # in place (out aliases the residual), as the transformer blocks call it
    h = res.to(DEV).clone()
    ops.ff_geglu_fused320(x.to(DEV), pw1, w2p, pw2.bias, h, residual=h)
    assert torch.equal(h, out)
    # with the LayerNorm in front folded in: x = ff(LN(x)) + x, input = residual = output buffer
    gam = 1 + 0.2 * torch.randn(320, generator=g); bet = 0.3 * torch.randn(320, generator=g)
    h = (x * 1.7 + 0.3).to(torch.bfloat16).to(DEV)
    n_ref = torch.empty_like(h)
    ops.layernorm(h, n_ref, gam.to(DEV), bet.to(DEV), 1e-5)
    want = torch.empty_like(h)
    ops.ff_geglu_fused320(n_ref, pw1, w2p, pw2.bias, want, residual=h)
    ops.ff_geglu_fused320(h, pw1, w2p, pw2.bias, h, residual=h, ln=(gam.to(DEV), bet.to(DEV)))
    assert rel_l2(h, want) < 2e-3                      # same rounding points; the row statistics sum in a different order
    # with the transformer's proj_out (+ its residual) behind: y = r2 + proj(x + ff(LN(x)))
    wp = torch.randn(320, 320, generator=g) * 320 ** -0.5; bp = torch.randn(320, generator=g) * 0.1
    pwp = ops.PackedWeight.linear(wp, bp, DEV)
    r2 = torch.randn(M, 320, generator=g).to(torch.bfloat16).to(DEV)
    y_want = torch.empty_like(want)
    ops.gemm(want, pwp, y_want, residual=r2)
    h0 = (x * 1.7 + 0.3).to(torch.bfloat16).to(DEV)
    y = torch.empty_like(h0)
    ops.ff_geglu_proj_fused320(h0, pw1, w2p, pw2.bias, ops.ff2_permuted(wp, DEV), pwp.bias, r2, y, ln=(gam.to(DEV), bet.to(DEV)))
    assert rel_l2(y, y_want) < 3e-3
    y2 = r2.clone()                                     # in place on the transformer's input buffer
    ops.ff_geglu_proj_fused320(h0, pw1, w2p, pw2.bias, ops.ff2_permuted(wp, DEV), pwp.bias, y2, y2, ln=(gam.to(DEV), bet.to(DEV)))
    assert torch.equal(y2, y)
