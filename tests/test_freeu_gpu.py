"""FreeU on the GPU: ops.freeu (csrc/freeu.hip) against the float64 restatement (tests/freeu_restatement.py), the tiny UNet with
FreeU against the CPU oracle's loop with FreeU ahead of every concat, and the samplers with `freeu=`.

Stated tolerances (every test prints what it measures):
  skip columns      |got - ref64| <= 2^-8 |ref64| + 4 HW 2^-24 |s-1| max|x|   one bf16 rounding + fp32 accumulation over HW terms
                    of the four modes' sums (max|x| over the plane)
  backbone, v1      bf16(float32(x) * b), bit for bit
  backbone, v2      |got - ref64| <= 2^-8 |ref64| + ch 2^-24 max|h|            one bf16 rounding + the fp32 mean over ch columns
  untouched         columns ch/2..ch-1 and everything around the buffer: bit for bit
  tiny UNet         rel-L2 <= 3e-2, the bound of tests/test_model_gpu.py's tiny-UNet parity tests
  graph vs eager    torch.equal, the criterion of the existing graph tests
"""
import pytest
import torch

from tests import freeu_restatement as R
from tests.test_windows_gpu import _tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNET_TOL = 3e-2                     # tests/test_model_gpu.py: test_unet_tiny_vs_reference / test_unet_vs_oracle_odd_sizes
FREEU = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
CASES = [(2, 3, 5, 128, 64), (3, 2, 2, 128, 64), (2, 9, 16, 128, 128), (1, 18, 32, 256, 192), (2, 5, 8, 128, 320)]
GUARD, OFF, PAD = 3, 8, 16          # sentinel rows above / below, sentinel columns left / right of the cat buffer
SENTINEL = 12345.0


def rel_l2(a, b):
    a = torch.as_tensor(a).float().cpu(); b = torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _planes(rows, F, H, W):
    """rows [F*H*W, C] -> [F, C, H, W] float64 on the CPU"""
    return rows.detach().to("cpu", torch.float64).reshape(F, H, W, -1).permute(0, 3, 1, 2)


def _rows(planes):
    F, Cc, H, W = planes.shape
    return planes.permute(0, 2, 3, 1).reshape(F * H * W, Cc)


def _inputs(F, H, W, ch, cs, kind="random", seed=0):
    """bf16 rows [F*H*W, ch + cs] on the CPU. random: N(0,1) plus a per-pixel ramp on h, so that the channel mean of h is far
    from constant over a frame; constant: every skip plane one bf16 value, every row of h of frame 0 the same."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * F + 11 * H + 13 * W + ch + cs)
    h = torch.randn(F, ch, H, W, generator=g) + torch.linspace(-1.5, 1.5, H * W).reshape(1, 1, H, W).roll(seed + 1, -1)
    skip = torch.randn(F, cs, H, W, generator=g) * 1.3 + 0.2
    if kind == "constant":
        skip = (torch.randn(F, cs, 1, 1, generator=g) * 2).expand(F, cs, H, W)
        h[0] = torch.randn(ch, 1, 1, generator=g)
    return _rows(torch.cat([h, skip], 1)).to(torch.bfloat16).contiguous()


def _run(x, F, H, W, ch, cs, b, s, version):
    """ops.freeu on a column slice of a wider buffer with sentinels all around -> (result rows on the CPU, the whole wide buffer
    before and after as int16 bits)."""
    from dynamicrafter_amd import ops
    rows = F * H * W
    wide = torch.full((rows + 2 * GUARD, OFF + ch + cs + PAD), SENTINEL, dtype=torch.bfloat16, device=DEV)
    cat = wide[GUARD:GUARD + rows, OFF:OFF + ch + cs]
    cat.copy_(x.to(DEV))
    before = wide.view(torch.int16).clone()
    scratch = torch.full((ops.freeu_scratch_floats(cs=cs, F=F, H=H, W=W, version=version) + 32,), SENTINEL,
                         dtype=torch.float32, device=DEV)
    n = ops.freeu_scratch_floats(cs=cs, F=F, H=H, W=W, version=version)
    out = ops.freeu(cat, ch=ch, cs=cs, F=F, H=H, W=W, b=b, s=s, version=version, scratch=scratch[:n])
    torch.cuda.synchronize()
    assert out.data_ptr() == cat.data_ptr()
    assert bool((scratch[n:] == SENTINEL).all())                       # the scratch is not overrun either
    return cat.cpu(), before.cpu(), wide.view(torch.int16).cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_untouched(before, after, rows, ch, cs):
    keep = torch.ones_like(before, dtype=torch.bool)
    keep[GUARD:GUARD + rows, OFF:OFF + ch // 2] = False
    keep[GUARD:GUARD + rows, OFF + ch:OFF + ch + cs] = False
    assert torch.equal(before[keep], after[keep])


def _check_skip(got, x, F, H, W, ch, cs, s, what):
    xs = _planes(x[:, ch:], F, H, W)
    ref = R.skip_filter_real(xs, s)
    bound = 2.0 ** -8 * ref.abs() + 4 * H * W * 2.0 ** -24 * abs(s - 1) * xs.abs().amax(dim=(2, 3), keepdim=True)
    err = (_planes(got[:, ch:], F, H, W) - ref).abs()
    print(f"\n[freeu skip {what} F{F} {H}x{W} ch{ch} cs{cs} s={s}] worst err / bound {(err / bound.clamp_min(1e-30)).max().item():.3f}")
    assert bool((err <= bound).all())
    return ref


@pytest.mark.parametrize("F,H,W,ch,cs", CASES)
def test_op_version1_vs_restatement(F, H, W, ch, cs):
    b, s = 1.5, 0.2
    x = _inputs(F, H, W, ch, cs)
    got, before, after = _run(x, F, H, W, ch, cs, b, s, 1)
    _check_untouched(before, after, F * H * W, ch, cs)
    _check_skip(got, x, F, H, W, ch, cs, s, "v1")
    want = (x[:, :ch // 2].float() * b).to(torch.bfloat16)
    assert torch.equal(_bits(got[:, :ch // 2]), _bits(want))          # bf16(float32(x) * b), bit for bit
    assert torch.equal(_bits(got[:, ch // 2:ch]), _bits(x[:, ch // 2:ch]))
    again, _, _ = _run(x, F, H, W, ch, cs, b, s, 1)
    assert torch.equal(_bits(again), _bits(got))                      # two runs, the same bits
    # a scale above 1 as well (s - 1 changes sign)
    got2, _, _ = _run(x, F, H, W, ch, cs, 0.8, 1.7, 1)
    _check_skip(got2, x, F, H, W, ch, cs, 1.7, "v1")


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("F,H,W,ch,cs", CASES)
def test_op_identity_settings_return_the_input(F, H, W, ch, cs, version):
    x = _inputs(F, H, W, ch, cs, seed=1)
    got, before, after = _run(x, F, H, W, ch, cs, 1.0, 1.0, version)
    assert torch.equal(before, after)
    assert torch.equal(_bits(got), _bits(x))


@pytest.mark.parametrize("F,H,W,ch,cs", CASES)
def test_op_constant_planes(F, H, W, ch, cs):
    """A constant plane c is its own mean: the filter returns s * c. Frame 0 of h has a flat channel mean: version 2 leaves it
    alone (mhat = 0 there, where the published code divides by zero)."""
    s = 0.2
    x = _inputs(F, H, W, ch, cs, kind="constant", seed=2)
    got, before, after = _run(x, F, H, W, ch, cs, 1.5, s, 2)
    _check_untouched(before, after, F * H * W, ch, cs)
    ref = _check_skip(got, x, F, H, W, ch, cs, s, "constant")
    assert (ref - s * _planes(x[:, ch:], F, H, W)).abs().max().item() <= 1e-12
    assert torch.equal(_bits(got[:H * W, :ch // 2]), _bits(x[:H * W, :ch // 2]))
    assert torch.isfinite(got.float()).all()


@pytest.mark.parametrize("F,H,W,ch,cs", CASES)
def test_op_version2_vs_restatement(F, H, W, ch, cs):
    b, s = 1.6, 0.9
    x = _inputs(F, H, W, ch, cs, seed=3)
    got, before, after = _run(x, F, H, W, ch, cs, b, s, 2)
    _check_untouched(before, after, F * H * W, ch, cs)
    _check_skip(got, x, F, H, W, ch, cs, s, "v2")                     # the skip filter is the same in both versions
    h = _planes(x[:, :ch], F, H, W)
    fac = R.backbone_factor(h, b, 2)
    assert (fac.amax(dim=(2, 3)) - fac.amin(dim=(2, 3))).min().item() > 0.5 * (b - 1)      # the mean is not constant
    ref = R.backbone_scale(h, b, 2)[:, :ch // 2]
    err = (_planes(got[:, :ch // 2], F, H, W) - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + ch * 2.0 ** -24 * h.abs().max()
    print(f"\n[freeu backbone v2 F{F} {H}x{W} ch{ch}] worst err / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(_bits(got[:, ch // 2:ch]), _bits(x[:, ch // 2:ch]))
    again, _, _ = _run(x, F, H, W, ch, cs, b, s, 2)
    assert torch.equal(_bits(again), _bits(got))


def test_op_refuses_bad_arguments():
    from dynamicrafter_amd import ops
    F, H, W, ch, cs = 2, 3, 5, 128, 64
    rows = F * H * W
    cat = torch.zeros(rows, ch + cs, dtype=torch.bfloat16, device=DEV)
    scr = torch.zeros(ops.freeu_scratch_floats(cs=cs, F=F, H=H, W=W, version=2), device=DEV)
    kw = dict(ch=ch, cs=cs, F=F, H=H, W=W, b=1.5, s=0.2, scratch=scr)
    ops.freeu(cat, **kw)
    for bad, match in ((dict(cs=32), "cs % 64"), (dict(ch=64), "ch % 128"), (dict(F=3), "expected"), (dict(H=4), "expected"),
                       (dict(version=3), "version"), (dict(b=float("nan")), "finite"), (dict(s=float("inf")), "finite"),
                       (dict(scratch=scr[:F * cs * 7 - 1]), "scratch"), (dict(scratch=scr.double()), "scratch"),
                       (dict(version=2, scratch=scr[:F * cs * 7]), "scratch")):
        with pytest.raises(ValueError, match=match):
            ops.freeu(cat, **dict(kw, **bad))
    with pytest.raises(ValueError, match="bf16|bfloat16"):
        ops.freeu(cat.float(), **kw)
    wide = torch.zeros(rows, ch + cs + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="aligned"):
        ops.freeu(wide[:, 4:4 + ch + cs], **kw)                       # an 8-byte offset
    odd = torch.zeros(rows, ch + cs + 4, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="stride"):
        ops.freeu(odd[:, :ch + cs], **kw)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the tiny UNet
@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


@pytest.fixture(scope="module")
def unet_case(tiny):
    """Inputs and the three CPU references (computed once): FreeU off, version 1, version 2."""
    model, sd, ocfg = tiny
    g = torch.Generator().manual_seed(21)
    b, t, h, w = 1, 4, 16, 16
    x = torch.randn(b, 8, t, h, w, generator=g)
    ctx = torch.randn(b, 77 + 16 * t, 128, generator=g)
    ts = torch.tensor([444])
    fs = torch.tensor([24])
    refs = {v: R.unet_forward_freeu(sd, ocfg, x, ts, ctx, fs, freeu=None if v == 0 else dict(FREEU, version=v)) for v in (0, 1, 2)}
    return dict(x=x, ctx=ctx, ts=ts, fs=fs, refs=refs)


def _forward(net, c):
    return net(c["x"].to(DEV), c["ts"].to(DEV), context=c["ctx"].to(DEV), fs=c["fs"].to(DEV)).clone()


def test_restated_loop_is_the_oracles_loop(tiny, unet_case):
    from oracle import unet as ounet
    _, sd, ocfg = tiny
    c = unet_case
    assert torch.equal(c["refs"][0], ounet.unet_forward(sd, ocfg, c["x"], c["ts"], c["ctx"], c["fs"]))


@pytest.mark.parametrize("version", [1, 2])
def test_unet_with_freeu_vs_oracle(tiny, unet_case, version):
    model, _, _ = tiny
    net = model.model.diffusion_model
    c = unet_case
    net.disable_freeu()
    plain = _forward(net, c)
    try:
        net.enable_freeu(**FREEU, version=version)
        y = _forward(net, c)
        y2 = _forward(net, c)
    finally:
        net.disable_freeu()
    r, off = rel_l2(y, c["refs"][version]), rel_l2(plain, c["refs"][0])
    moved = rel_l2(y, plain)
    print(f"\n[tiny UNet, FreeU v{version}] vs oracle rel-L2 {r:.3e} (FreeU off: {off:.3e}); on vs off {moved:.3e}; "
          f"oracle on vs off {rel_l2(c['refs'][version], c['refs'][0]):.3e}")
    assert off < UNET_TOL
    assert r < UNET_TOL
    assert moved > UNET_TOL                                           # FreeU changes the output by more than the parity bound
    assert torch.equal(y, y2)
    assert torch.equal(_forward(net, c), plain)                       # off again: the bits of the plain forward


def test_disable_is_bit_identical_to_never_enabled(tiny, unet_case):
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    from tests.golden_cfg import TINY_UNET
    model, sd, _ = tiny
    fresh = UNetModel(**dict(TINY_UNET, default_fs=24))
    fresh.load_state_dict(sd, strict=True)
    fresh.to(DEV)
    never = _forward(fresh, unet_case)
    net = model.model.diffusion_model
    net.enable_freeu(**FREEU, version=2)
    _forward(net, unet_case)
    net.disable_freeu()
    assert torch.equal(_forward(net, unet_case), never)
    launches = []
    from dynamicrafter_amd import ops
    real = ops.freeu
    try:
        ops.freeu = lambda *a, **k: (launches.append(1), real(*a, **k))[1]
        _forward(net, unet_case)
        assert launches == []                                         # off: not one launch is added
        net.enable_freeu(**FREEU)
        _forward(net, unet_case)
        assert len(launches) == 10                                    # up blocks 0-9
    finally:
        ops.freeu = real
        net.disable_freeu()


# ------------------------------------------------------------------ the samplers
def _sampler_inputs(S, seed=9, b=1, t=4, h=16, w=16):
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(b, 4, t, h, w, generator=g), ctx=[torch.randn(b, 77 + 16 * t, 128, generator=g) for _ in range(2)],
                cc=torch.randn(b, 4, t, h, w, generator=g) * 0.2, noises=torch.randn(S, b, 4, t, h, w, generator=g),
                fs=torch.tensor([24] * b))


def _mk(inp, k):
    return {"c_crossattn": [inp["ctx"][k].to(DEV)], "c_concat": [inp["cc"].to(DEV)]}


def _sample(sampler, inp, S, **kw):
    out, _ = sampler.sample(S=S, batch_size=1, shape=tuple(inp["x"].shape[1:]), conditioning=_mk(inp, 0), verbose=False,
                            unconditional_guidance_scale=7.5, unconditional_conditioning=_mk(inp, 1), eta=1.0,
                            x_T=inp["x"].to(DEV), fs=inp["fs"].to(DEV), timestep_spacing="uniform_trailing",
                            guidance_rescale=0.7, noises=inp["noises"].to(DEV), **kw)
    return out.clone()


@pytest.mark.parametrize("version", [1, 2])
def test_ddim_with_freeu_graph_equals_eager(tiny, version):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    model, _, _ = tiny
    net = model.model.diffusion_model
    inp = _sampler_inputs(3)
    fu = dict(FREEU, version=version)
    eager = _sample(DDIMSampler(model), inp, 3, freeu=fu, use_graph=False)
    assert net.freeu is None                                          # the call restores the model's setting
    graph = _sample(DDIMSampler(model), inp, 3, freeu=fu, use_graph=True)
    plain = _sample(DDIMSampler(model), inp, 3, use_graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graph)                                  # graph replay == eager launches, bit for bit
    print(f"\n[3-step DDIM, FreeU v{version}] on vs off rel-L2 {rel_l2(eager, plain):.3e}")
    assert not torch.equal(eager, plain) and rel_l2(eager, plain) > 1e-3


def test_dpm_solver_and_encode_with_freeu(tiny):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    from dynamicrafter_amd.lvdm.models.samplers.dpm_solver import DPMSolverSampler
    model, _, _ = tiny
    net = model.model.diffusion_model
    inp = _sampler_inputs(2, seed=10)
    fu = dict(FREEU, version=1)
    on = _sample(DPMSolverSampler(model), inp, 2, freeu=fu, use_graph=True)
    off = _sample(DPMSolverSampler(model), inp, 2, use_graph=True)
    assert torch.isfinite(on).all() and rel_l2(on, off) > 1e-3
    s = DDIMSampler(model)
    s.make_schedule(4, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
    enc = lambda **kw: s.encode(inp["x"].to(DEV), _mk(inp, 0), 2, fs=inp["fs"].to(DEV), unconditional_guidance_scale=2.0,
                                unconditional_conditioning=_mk(inp, 1), **kw)[0].clone()
    e_on, e_off = enc(freeu=fu), enc()
    assert torch.isfinite(e_on).all() and rel_l2(e_on, e_off) > 1e-3
    assert torch.equal(enc(freeu=fu, use_graph=True), e_on)
    assert net.freeu is None
