"""K/V token downsampling on the GPU: ops.ln_pool_tokens (csrc/token_pool.hip) against ops.layernorm and the float64
restatement (tests/todo_restatement.py), the spatial self-attention sub-path on every attention kernel, the tiny UNet against the
CPU oracle's loop with the downsampled attn1, that off is free, and the samplers with `token_downsampling=`.

Stated tolerances (every test prints what it measures):
  nearest             torch.equal with ops.layernorm on the same input at the kept rows (the kernel repeats its row arithmetic)
  mean                |got - ref64| <= 2^-8 |ref64| + 4 e32: one bf16 rounding, and four times the largest absolute error e32 of
                      the same restatement run in fp32 torch on the CPU against float64 on those inputs (measured in the test;
                      the factor 4 is the kernel / fp32 allowance of tests/test_apg_gpu.py)
  constant rows       bf16(beta), bit for bit, in both modes
  around the output   sentinel rows and columns: bit for bit
  attention sub-path  rel-L2 <= 6e-3, the bound of tests/test_ops_gpu.py::test_flash_attn (5 heads: its case (2, 5, 144, 144))
                      and ::test_flash_attn_long_self (the pipelined kernel) for flash_attn against the fp32 reference
  tiny UNet           rel-L2 <= 3e-2, the bound of tests/test_model_gpu.py's tiny-UNet parity tests; on vs off above it
  graph vs eager, rewind, off   torch.equal
  on vs off, samplers rel-L2 > 1e-3
"""
import ctypes as C

import pytest
import torch

from tests import todo_restatement as R
from tests.test_windows_gpu import _tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNET_TOL = 3e-2                     # tests/test_model_gpu.py: test_unet_tiny_vs_reference / test_unet_vs_oracle_odd_sizes
ATTN_TOL = 6e-3                     # tests/test_ops_gpu.py: test_flash_attn / test_flash_attn_long_self
SHAPES = [(2, 4, 6, 64, 2), (3, 9, 16, 128, 2), (1, 5, 7, 256, 3), (2, 32, 32, 320, 2), (1, 18, 32, 1280, 4), (2, 3, 3, 640, 8)]
GUARD, OFF, PAD = 4, 8, 16          # sentinel rows above / below, sentinel columns left / right of the output
SENTINEL = 12345.0


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _affine(Cc, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return 1 + 0.2 * torch.randn(Cc, generator=g), 0.3 * torch.randn(Cc, generator=g)


def _inputs(F, H, W, Cc, seed=0):
    """bf16 rows [F*H*W, C] on the CPU: N(0, 1.5^2) with an offset and a scale per token, so that rows differ in mean and variance."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * F + 11 * H + 13 * W + Cc)
    x = torch.randn(F * H * W, Cc, generator=g) * (0.5 + 2 * torch.rand(F * H * W, 1, generator=g)) + torch.randn(F * H * W, 1, generator=g)
    return x.to(torch.bfloat16).contiguous()


def _run(x, gamma, beta, F, H, W, f, mode, padded_in):
    """ops.ln_pool_tokens into a column slice of a wider buffer with sentinels all around; the input with a row stride of C or
    of C + 16 -> (result rows on the CPU, the input as the kernel saw it (on the GPU), the wide buffer's bits before and after)."""
    from dynamicrafter_amd import ops
    Cc = x.shape[1]
    Hp, Wp = R.pooled_grid(H, W, f)
    rows = F * Hp * Wp
    xin = x.to(DEV)
    if padded_in:
        xw = torch.full((x.shape[0], Cc + 16), SENTINEL, dtype=torch.bfloat16, device=DEV)
        xw[:, :Cc] = xin
        xin = xw[:, :Cc]
    assert xin.stride(0) == (Cc + 16 if padded_in else Cc)
    wide = torch.full((rows + 2 * GUARD, OFF + Cc + PAD), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = wide[GUARD:GUARD + rows, OFF:OFF + Cc]
    before = wide.view(torch.int16).clone()
    out = ops.ln_pool_tokens(xin, y, gamma.to(DEV), beta.to(DEV), F=F, H=H, W=W, factor=f, mode=mode)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    return y.cpu(), xin, before.cpu(), wide.view(torch.int16).cpu()


def _check_untouched(before, after, rows, Cc):
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[GUARD:GUARD + rows, OFF:OFF + Cc] = False
    assert torch.equal(before[keep], after[keep])


def _kept_rows(F, H, W, f):
    idx = torch.arange(F * H * W).reshape(F, H, W)[:, ::f, ::f]
    return idx.reshape(-1)


# ------------------------------------------------------------------ the op
@pytest.mark.parametrize("padded_in", [False, True])
@pytest.mark.parametrize("F,H,W,Cc,f", SHAPES)
def test_op_nearest_is_layernorm_at_the_kept_rows(F, H, W, Cc, f, padded_in):
    from dynamicrafter_amd import ops
    x = _inputs(F, H, W, Cc)
    gamma, beta = _affine(Cc)
    got, xin, before, after = _run(x, gamma, beta, F, H, W, f, "nearest", padded_in)
    Hp, Wp = R.pooled_grid(H, W, f)
    _check_untouched(before, after, F * Hp * Wp, Cc)
    full = torch.empty(F * H * W, Cc, dtype=torch.bfloat16, device=DEV)
    ops.layernorm(xin, full, gamma.to(DEV), beta.to(DEV), 1e-5)
    want = full.cpu()[_kept_rows(F, H, W, f)]
    assert want.shape == got.shape
    assert torch.equal(_bits(got), _bits(want))                       # bit for bit the rows of dc_layernorm
    ref = R.ln_pool_tokens(x.reshape(F, H * W, Cc), gamma, beta, H, W, f, "nearest").reshape(-1, Cc)
    assert rel_l2(got, ref) < 4e-3                                    # and a LayerNorm at all (tests/test_ops_gpu.py::test_layernorm)
    again, _, _, _ = _run(x, gamma, beta, F, H, W, f, "nearest", padded_in)
    assert torch.equal(_bits(again), _bits(got))


@pytest.mark.parametrize("padded_in", [False, True])
@pytest.mark.parametrize("F,H,W,Cc,f", SHAPES)
def test_op_mean_vs_restatement(F, H, W, Cc, f, padded_in):
    x = _inputs(F, H, W, Cc, seed=1)
    gamma, beta = _affine(Cc, seed=1)
    got, _, before, after = _run(x, gamma, beta, F, H, W, f, "mean", padded_in)
    Hp, Wp = R.pooled_grid(H, W, f)
    _check_untouched(before, after, F * Hp * Wp, Cc)
    x3 = x.reshape(F, H * W, Cc)
    ref = R.ln_pool_tokens(x3, gamma, beta, H, W, f, "mean").reshape(-1, Cc)
    ref32 = R.ln_pool_tokens(x3, gamma, beta, H, W, f, "mean", dtype=torch.float32).reshape(-1, Cc)
    e32 = (ref32.double() - ref).abs().max().item()
    err = (got.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 4 * e32
    worst = (err / bound).max().item()
    # what is left of the error once the final bf16 rounding (at most 2^-8 |ref|) is taken out, against e32: at most 4
    excess = (err - 2.0 ** -8 * ref.abs()).clamp_min(0).max().item()
    print(f"\n[ln_pool mean F{F} {H}x{W} C{Cc} f{f} padded_in={padded_in}] e32 {e32:.3e}, worst err / bound {worst:.3f}, "
          f"error beyond one bf16 rounding / e32 {excess / e32:.3f}")
    assert e32 > 0
    assert bool((err <= bound).all())
    # not the nearest tokens, and not a mean with the full-cell divisor at clipped borders
    near = R.ln_pool_tokens(x3, gamma, beta, H, W, f, "nearest").reshape(-1, Cc)
    assert rel_l2(got, near) > 0.1 or H * W == 1
    again, _, _, _ = _run(x, gamma, beta, F, H, W, f, "mean", padded_in)
    assert torch.equal(_bits(again), _bits(got))


@pytest.mark.parametrize("mode", ["nearest", "mean"])
@pytest.mark.parametrize("F,H,W,Cc,f", SHAPES)
def test_op_constant_rows_return_beta(F, H, W, Cc, f, mode):
    """A row whose C entries are all +-2^k has mean exactly that value in fp32: the sum C 2^k is exact, and fl(1 / C) is exact for
    the widths that are powers of two and 2^-26 (relative) above 1 / C for 320, 640 and 1280 (5 x 2^n), so the product rounds
    back to 2^k. Every deviation is then 0 and LayerNorm returns beta for any gamma.
    beta is drawn within a quarter of a bf16 ulp of a bf16 value, away from rounding ties: the mean of up to f^2 equal fp32
    numbers may be off by a few fp32 ulps, which then cannot change bf16(beta)."""
    g = torch.Generator().manual_seed(F + H + W + Cc + f)
    k = torch.randint(-3, 4, (F * H * W, 1), generator=g).float()
    sign = torch.randint(0, 2, (F * H * W, 1), generator=g).float() * 2 - 1
    x = (sign * 2.0 ** k).expand(F * H * W, Cc).to(torch.bfloat16).contiguous()
    gamma, _ = _affine(Cc, seed=2)
    b16 = (0.3 * torch.randn(Cc, generator=g)).to(torch.bfloat16)
    beta = b16.float() * (1 + (torch.rand(Cc, generator=g) * 2 - 1) * 2.0 ** -10)
    assert torch.equal(beta.to(torch.bfloat16), b16) and not torch.equal(beta, b16.float())
    got, _, before, after = _run(x, gamma, beta, F, H, W, f, mode, False)
    Hp, Wp = R.pooled_grid(H, W, f)
    _check_untouched(before, after, F * Hp * Wp, Cc)
    assert torch.equal(_bits(got), _bits(b16[None].expand(F * Hp * Wp, Cc)))


def test_op_refuses_bad_arguments():
    from dynamicrafter_amd import _hip, ops
    F, H, W, Cc, f = 2, 4, 6, 64, 2
    x = torch.zeros(F * H * W, Cc, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(F * 2 * 3, Cc, dtype=torch.bfloat16, device=DEV)
    gamma, beta = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    kw = dict(F=F, H=H, W=W, factor=f, mode="nearest")
    ops.ln_pool_tokens(x, y, gamma, beta, **kw)
    # the C entry: the error codes of include/dcrafter_hip.h, nothing launched
    fn = _hip.lib().dc_ln_pool_tokens
    p = lambda t: C.c_void_p(t.data_ptr())
    ok = dict(x=p(x), ldx=Cc, y=p(y), ldy=Cc, gamma=p(gamma), beta=p(beta), F=F, H=H, W=W, C=Cc, factor=f, mode=0)
    call = lambda **k: fn(*dict(ok, **k).values(), 1e-5, ops.stream_ptr())
    assert call() == 0
    for k in ("x", "y", "gamma", "beta"):
        assert call(**{k: None}) == -2, k
    for bad in (dict(C=60), dict(C=2056), dict(ldx=68), dict(ldy=60), dict(ldx=56), dict(F=0), dict(H=0), dict(W=-3),
                dict(factor=1), dict(factor=9), dict(mode=2), dict(mode=-1), dict(x=C.c_void_p(x.data_ptr() + 8)),
                dict(y=C.c_void_p(y.data_ptr() + 2))):
        assert call(**bad) == -1, bad
    # ops raises before a launch
    for bad, match in ((dict(mode="max"), "mode"), (dict(mode=0), "mode"), (dict(factor=1), "factor"), (dict(factor=9), "factor"),
                       (dict(factor=2.0), "factor"), (dict(factor=True), "factor"), (dict(F=3), "expected"), (dict(H=5), "expected"),
                       (dict(W=0), "expected")):
        with pytest.raises(ValueError, match=match):
            ops.ln_pool_tokens(x, y, gamma, beta, **dict(kw, **bad))
    with pytest.raises(ValueError, match="addresses"):
        ops.ln_pool_tokens(x, y[:-1], gamma, beta, **kw)              # an output one row short
    with pytest.raises(ValueError, match="bf16|bfloat16"):
        ops.ln_pool_tokens(x.float(), y, gamma, beta, **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.ln_pool_tokens(x, y, gamma[:60], beta, **kw)
    wide = torch.zeros(F * H * W, Cc + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="aligned"):
        ops.ln_pool_tokens(wide[:, 4:4 + Cc], y, gamma, beta, **kw)   # an 8-byte offset
    odd = torch.zeros(F * H * W, Cc + 4, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="stride"):
        ops.ln_pool_tokens(odd[:, :Cc], y, gamma, beta, **kw)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


# ------------------------------------------------------------------ the attention sub-path
ATTN_CASES = [  # F, H, W, C (heads = C / 64), factor, mode: Lq = H W, Lk = ceil(H / f) ceil(W / f)
    (4, 32, 32, 320, 2, "nearest"),     # Lq 1024, Lk 256: flash_pipe; 4096 rows at width 320: q through the fused ln_linear
    (4, 32, 32, 320, 2, "mean"),
    (2, 24, 24, 128, 2, "nearest"),     # Lq 576, Lk 144: the non-pipe kernel (Lk < 256)
    (2, 9, 16, 640, 2, "mean"),         # Lq 144, Lk 5 x 8 = 40: an odd pooled grid
    (2, 9, 16, 640, 2, "nearest"),
]


@pytest.mark.parametrize("F,H,W,Cc,f,mode", ATTN_CASES)
def test_attention_subpath_vs_restatement(tiny, F, H, W, Cc, f, mode):
    """UNetModel._attn_self_spatial with packed weights of its own against self_attention_todo + the residual in float64, on
    the same bf16-rounded weights and inputs. Bound: rel-L2 <= 6e-3, what tests/test_ops_gpu.py::test_flash_attn (5 heads:
    (2, 5, 144, 144)) and ::test_flash_attn_long_self state for flash_attn alone; here the LayerNorm, the q and kv projections,
    the pooling and to_out with its residual sit inside the same bound."""
    from dynamicrafter_amd import ops
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    from dynamicrafter_amd.ops import PackedWeight
    net = tiny[0].model.diffusion_model
    heads = Cc // 64
    g = torch.Generator().manual_seed(F + H + W + Cc)
    bf = lambda t: t.to(torch.bfloat16).float()
    w = {k: bf(torch.randn(Cc, Cc, generator=g) * a / Cc ** 0.5) for k, a in (("q", 1.5), ("k", 1.5), ("v", 1.0), ("out", 2.0))}
    b_out = 0.1 * torch.randn(Cc, generator=g)
    gamma, beta = _affine(Cc, seed=3)
    h = _inputs(F, H, W, Cc, seed=4)
    Wa = {"qkv": PackedWeight.linear(torch.cat([w["q"], w["k"], w["v"]], 0), None, DEV), "out": PackedWeight.linear(w["out"], b_out, DEV)}
    UNetModel._split_attn1({"in": [[{"blk": {"attn1": Wa, "q2": None}}]], "mid": [], "out": []})
    assert Wa["q"].N == Cc and Wa["kv"].N == 2 * Cc and Wa["q"].K == Wa["kv"].K == Cc
    ln = (gamma.to(DEV), beta.to(DEV))
    geo = dict(F=F, H=H, W=W, HW=H * W, lvl=0)
    names = []
    real = ops._launch
    prev = net.set_token_downsampling(dict(factor=f, levels=(0,), mode=mode))
    try:
        ops._launch = lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1]
        hd = h.to(DEV)
        out = net._attn_self_spatial(Wa, ln, hd, dict(geo), heads)
        torch.cuda.synchronize()
        got = out.cpu()
        first = list(names)                                           # the launches of one call
        hd2 = h.to(DEV)
        assert torch.equal(net._attn_self_spatial(Wa, ln, hd2, dict(geo), heads).cpu(), got)
        net.disable_token_downsampling()
        full = net._attn_self_spatial(Wa, ln, h.to(DEV), dict(geo), heads).cpu()
    finally:
        ops._launch = real
        net.set_token_downsampling(prev)
    print(f"\n[attn1 F{F} {H}x{W} C{Cc} f{f} {mode}] launches {first}")
    assert first.count(f"ln_pool_tokens({mode})") == 1 and len([n for n in first if n.startswith("flash_attn_d64")]) == 1
    if F * H * W >= 4096 and Cc in (320, 640):
        assert first[0] == "ln_linear"                                # q: the fused LayerNorm + Linear route
    sd = {f"a.to_{k}.weight": w[k].double() for k in "qkv"}
    sd["a.to_out.0.weight"], sd["a.to_out.0.bias"] = w["out"].double(), b_out.double()
    h64 = h.double().reshape(F, H * W, Cc)
    n = torch.nn.functional.layer_norm(h64, (Cc,), gamma.double(), beta.double(), 1e-5)
    branch = R.self_attention_todo(sd, "a", n, heads, 64, H, W, f, mode)
    ref = (branch + h64).reshape(-1, Cc)
    from oracle import unet as ounet
    ref_full = (ounet.cross_attention(sd, "a", n, None, heads, 64, None, False) + h64).reshape(-1, Cc)
    other = "mean" if mode == "nearest" else "nearest"
    ref_other = (R.self_attention_todo(sd, "a", n, heads, 64, H, W, f, other) + h64).reshape(-1, Cc)
    r = rel_l2(got, ref)
    print(f"[attn1 F{F} {H}x{W} C{Cc} f{f} {mode}] rel-L2 {r:.3e} (bound {ATTN_TOL:.0e}); branch / input norm "
          f"{(branch.norm() / h64.norm()).item():.3f}; full attention: kernels {rel_l2(full, ref_full):.3e}, reference vs this "
          f"{rel_l2(ref_full, ref):.3e}; other mode's reference vs this {rel_l2(ref_other, ref):.3e}")
    assert r < ATTN_TOL
    assert rel_l2(full, ref_full) < ATTN_TOL                          # the path it replaces, on the same data
    assert rel_l2(ref_full, ref) > 5 * ATTN_TOL and rel_l2(ref_other, ref) > 5 * ATTN_TOL     # the bound tells them apart


# ------------------------------------------------------------------ the tiny UNet
SETTINGS = {"nearest-012": dict(factor=2, levels=(0, 1, 2), mode="nearest"), "nearest-0": dict(factor=2, levels=(0,), mode="nearest"),
            "mean-012": dict(factor=2, levels=(0, 1, 2), mode="mean")}


@pytest.fixture(scope="module")
def unet_case(tiny):
    """Inputs (those of tests/test_freeu_gpu.py's unet_case) and the CPU references, computed once: off and the three settings."""
    model, sd, ocfg = tiny
    g = torch.Generator().manual_seed(21)
    b, t, h, w = 1, 4, 16, 16
    x = torch.randn(b, 8, t, h, w, generator=g)
    ctx = torch.randn(b, 77 + 16 * t, 128, generator=g)
    ts = torch.tensor([444])
    fs = torch.tensor([24])
    refs = {k: R.unet_forward_todo(sd, ocfg, x, ts, ctx, fs, todo=v) for k, v in dict(SETTINGS, off=None).items()}
    return dict(x=x, ctx=ctx, ts=ts, fs=fs, refs=refs)


def _forward(net, c):
    return net(c["x"].to(DEV), c["ts"].to(DEV), context=c["ctx"].to(DEV), fs=c["fs"].to(DEV)).clone()


def test_restated_loop_is_the_oracles_loop(tiny, unet_case):
    from oracle import unet as ounet
    _, sd, ocfg = tiny
    c = unet_case
    assert torch.equal(c["refs"]["off"], ounet.unet_forward(sd, ocfg, c["x"], c["ts"], c["ctx"], c["fs"]))


@pytest.mark.parametrize("name", list(SETTINGS))
def test_unet_with_token_downsampling_vs_oracle(tiny, unet_case, name):
    """Measured with the fp32 oracle on the CPU, on vs off: nearest / 2 / levels 0-2 1.18e-1, nearest / 2 / level 0 6.8e-2,
    mean / 2 / levels 0-2 8.4e-2: the reference alone separates on from off by 2-4 x the bound."""
    model, _, _ = tiny
    net = model.model.diffusion_model
    c = unet_case
    net.disable_token_downsampling()
    plain = _forward(net, c)
    try:
        net.enable_token_downsampling(**SETTINGS[name])
        y = _forward(net, c)
        y2 = _forward(net, c)
    finally:
        net.disable_token_downsampling()
    r, off = rel_l2(y, c["refs"][name]), rel_l2(plain, c["refs"]["off"])
    moved = rel_l2(y, plain)
    print(f"\n[tiny UNet, token downsampling {name}] vs oracle rel-L2 {r:.3e} (off: {off:.3e}); on vs off {moved:.3e}; "
          f"oracle on vs off {rel_l2(c['refs'][name], c['refs']['off']):.3e}")
    assert off < UNET_TOL
    assert r < UNET_TOL
    assert moved > UNET_TOL                                           # it changes the output by more than the parity bound
    assert rel_l2(c["refs"][name], c["refs"]["off"]) > UNET_TOL
    assert torch.equal(y, y2)
    assert torch.equal(_forward(net, c), plain)                       # off again: the bits of the plain forward


def test_shared_prefix_path_gets_the_same_treatment(tiny, unet_case):
    """forward_rows(shared_prefix=2) reaches the first transformer's self-attention through _spatial_pre: with the setting on
    it returns, per branch, the bits of the unshared forward (as tests/test_model_gpu.py::test_shared_prefix_is_bit_identical
    shows with it off)."""
    from dynamicrafter_amd import ops
    model, _, _ = tiny
    net = model.model.diffusion_model
    c = unet_case
    B, T, H, W = 2, 4, 16, 16
    x2 = c["x"].repeat(2, 1, 1, 1, 1).to(DEV)
    ctx2 = torch.cat([c["ctx"], c["ctx"].flip(1)], 0).to(DEV)        # two branches: same latent, different context
    xr = torch.empty(B * T * H * W, 64, dtype=torch.bfloat16, device=DEV)
    ops.pack_latent(x2.float().contiguous(), None, xr, B=B, Cx=8, Cc=0, T=T, HW=H * W)
    ctx_rows, Lc = net.build_context_rows(ctx2, B, T, tag="ctx_sp")
    tt = torch.tensor([[444, 444]], dtype=torch.int64, device=DEV)
    fs = torch.tensor([24, 24], dtype=torch.int64, device=DEV)
    run = lambda sp: net.forward_rows(xr, tt, ctx_rows, B=B, T=T, H=H, W=W, Lc=Lc, fs_table=fs, shared_prefix=sp).clone()
    off = run(2)
    try:
        net.enable_token_downsampling(**SETTINGS["nearest-012"])
        shared, unshared = run(2), run(1)
    finally:
        net.disable_token_downsampling()
    assert torch.equal(shared, unshared)
    assert rel_l2(shared, off) > UNET_TOL
    assert torch.equal(run(2), off)


# ------------------------------------------------------------------ off is free
def _traced_forward(net, c):
    """(output, [(launch name, tag)], [(arena tag, rows, cols)]) of one forward."""
    from dynamicrafter_amd import ops
    asked = []
    real = net._arena.get
    net._arena.get = lambda tag, rows, cols, *a, **k: (asked.append((tag, rows, cols)), real(tag, rows, cols, *a, **k))[1]
    try:
        with ops.Tracer() as tr:
            y = _forward(net, c)
            launches = [(r[0], r[5]) for r in tr.records]
            torch.cuda.synchronize()
            tr.summary()                                              # releases the events
    finally:
        del net._arena.get
    return y, launches, asked


def test_off_is_free(tiny, unet_case):
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    from tests.golden_cfg import TINY_UNET
    model, sd, _ = tiny
    fresh = UNetModel(**dict(TINY_UNET, default_fs=24))
    fresh.load_state_dict(sd, strict=True)
    fresh.to(DEV)
    never, l_never, a_never = _traced_forward(fresh, unet_case)
    assert "attn1_split" not in fresh._packed                         # no split weights either
    assert not [k for k in fresh._arena._bufs if str(k[0]).startswith("todo")]
    net = model.model.diffusion_model
    net.enable_token_downsampling(**SETTINGS["mean-012"])
    on, l_on, a_on = _traced_forward(net, unet_case)
    net.disable_token_downsampling()
    off, l_off, a_off = _traced_forward(net, unet_case)
    assert torch.equal(off, never)
    assert l_off == l_never and a_off == a_never                      # launch for launch, buffer for buffer
    names = [n for n, _ in l_off]
    assert not [n for n in names if n.startswith("ln_pool")] and not [t for t, _, _ in a_off if str(t).startswith("todo")]
    # on: one pooling launch per selected attn1 (levels 0-2: 2 down + 3 up blocks each), and its three buffers
    pools = [n for n, _ in l_on if n.startswith("ln_pool")]
    assert pools == ["ln_pool_tokens(mean)"] * 15
    assert {t for t, _, _ in a_on if str(t).startswith("todo")} == {"todo_q", "todo_pool", "todo_kv"}
    assert len(l_on) == len(l_off) + 15 * 2                           # q and kv in place of qkv, plus the pooling
    assert not torch.equal(on, off)


# ------------------------------------------------------------------ the samplers
def _sampler_inputs(S, seed=9, b=1, t=4, h=16, w=16, T=4):
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(b, 4, t, h, w, generator=g), ctx=[torch.randn(b, 77 + 16 * T, 128, generator=g) for _ in range(3)],
                cc=torch.randn(b, 4, t, h, w, generator=g) * 0.2, noises=torch.randn(S, b, 4, t, h, w, generator=g),
                fs=torch.tensor([24] * b))


def _mk(inp, k):
    return {"c_crossattn": [inp["ctx"][k].to(DEV)], "c_concat": [inp["cc"].to(DEV)]}


def _sample(sampler, inp, S, guidance_rescale=0.7, **kw):
    out, _ = sampler.sample(S=S, batch_size=1, shape=tuple(inp["x"].shape[1:]), conditioning=_mk(inp, 0), verbose=False,
                            unconditional_guidance_scale=7.5, unconditional_conditioning=_mk(inp, 1), eta=1.0,
                            x_T=inp["x"].to(DEV), fs=inp["fs"].to(DEV), timestep_spacing="uniform_trailing",
                            guidance_rescale=guidance_rescale, noises=inp["noises"].to(DEV), **kw)
    return out.clone()


@pytest.mark.parametrize("name", ["nearest-0", "mean-012"])
def test_ddim_graph_equals_eager_and_rewinds(tiny, name):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    model, _, _ = tiny
    net = model.model.diffusion_model
    inp = _sampler_inputs(3)
    td = SETTINGS[name]
    net.enable_token_downsampling(factor=4, levels=(1,))             # a setting of the user's, to be found again afterwards
    try:
        before = net.token_downsampling
        eager = _sample(DDIMSampler(model), inp, 3, token_downsampling=td, use_graph=False)
        assert net.token_downsampling == before                       # the call restores the model's setting
        s = DDIMSampler(model)
        graph = _sample(s, inp, 3, token_downsampling=td, use_graph=True)
        assert net.token_downsampling == before
    finally:
        net.disable_token_downsampling()
    plain = _sample(DDIMSampler(model), inp, 3, use_graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph)                                  # graph replay == eager launches, bit for bit
    print(f"\n[3-step DDIM, token downsampling {name}] on vs off rel-L2 {rel_l2(eager, plain):.3e}")
    assert not torch.equal(eager, plain) and rel_l2(eager, plain) > 1e-3
    # the captured run keeps the setting it was captured with: replayed with the model's setting off, it repeats itself
    run = s._last_run
    assert run.graph is not None and net.token_downsampling is None
    run.rewind(inp["x"].to(DEV))
    for _ in range(run.S):
        run.step()
    run.sync()
    assert torch.equal(run.img, graph)


def test_dpm_solver_decode_encode_and_windows(tiny):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    model, _, _ = tiny
    net = model.model.diffusion_model
    inp = _sampler_inputs(3, seed=10)
    td = SETTINGS["nearest-012"]
    on = _sample(DPMSolverSampler(model, solver="dpmpp_2m"), inp, 3, token_downsampling=td, use_graph=True)
    off = _sample(DPMSolverSampler(model, solver="dpmpp_2m"), inp, 3, use_graph=True)
    assert torch.isfinite(on).all() and rel_l2(on, off) > 1e-3
    assert torch.equal(on, _sample(DPMSolverSampler(model, solver="dpmpp_2m"), inp, 3, token_downsampling=td, use_graph=False))
    s = DDIMSampler(model)
    s.make_schedule(4, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    enc = lambda **kw: s.encode(inp["x"].to(DEV), _mk(inp, 0), 2, fs=inp["fs"].to(DEV), unconditional_guidance_scale=2.0,
                                unconditional_conditioning=_mk(inp, 1), **kw)[0].clone()
    e_on, e_off = enc(token_downsampling=td), enc()
    assert torch.isfinite(e_on).all() and rel_l2(e_on, e_off) > 1e-3
    assert torch.equal(enc(token_downsampling=td, use_graph=True), e_on)
    dec = lambda **kw: s.decode(e_on, _mk(inp, 0), 2, unconditional_guidance_scale=7.5, unconditional_conditioning=_mk(inp, 1),
                                fs=inp["fs"].to(DEV), **kw).clone()
    d_on, d_off = dec(token_downsampling=td), dec()
    assert torch.isfinite(d_on).all() and rel_l2(d_on, d_off) > 1e-3
    assert torch.equal(dec(token_downsampling=td, use_graph=True), d_on)
    long = _sampler_inputs(3, seed=11, t=8)                           # T = 8 over windows of 4
    w_on = _sample(DDIMSampler(model), long, 3, token_downsampling=td, window_stride=2, use_graph=True)
    w_off = _sample(DDIMSampler(model), long, 3, window_stride=2, use_graph=True)
    assert torch.isfinite(w_on).all() and rel_l2(w_on, w_off) > 1e-3
    assert torch.equal(w_on, _sample(DDIMSampler(model), long, 3, token_downsampling=td, window_stride=2, use_graph=False))
    assert net.token_downsampling is None


def test_together_with_freeu_apg_and_three_branches(tiny):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.ddim_multiplecond import DDIMSampler as DDIMSampler3
    model, _, _ = tiny
    net = model.model.diffusion_model
    inp = _sampler_inputs(3, seed=12)
    td = SETTINGS["mean-012"]
    kw = dict(token_downsampling=td, freeu=dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6, version=2),
              apg=dict(eta=0.0, norm_threshold=20.0, momentum=-0.5), guidance_rescale=0.0)
    eager = _sample(DDIMSampler(model), inp, 3, use_graph=False, **kw)
    graph = _sample(DDIMSampler(model), inp, 3, use_graph=True, **kw)
    assert torch.isfinite(eager).all() and torch.equal(eager, graph)
    without = _sample(DDIMSampler(model), inp, 3, use_graph=True, **dict(kw, token_downsampling=None))
    assert rel_l2(eager, without) > 1e-3
    assert net.token_downsampling is None and net.freeu is None
    three = dict(cfg_img=2.0, unconditional_conditioning_img_nonetext=_mk(inp, 2))
    e3 = _sample(DDIMSampler3(model), inp, 3, use_graph=False, token_downsampling=td, **three)
    g3 = _sample(DDIMSampler3(model), inp, 3, use_graph=True, token_downsampling=td, **three)
    p3 = _sample(DDIMSampler3(model), inp, 3, use_graph=True, **three)
    assert torch.isfinite(e3).all() and torch.equal(e3, g3) and rel_l2(e3, p3) > 1e-3
