"""The launches of a sampler step are what they were before the sampling options moved into samplers/options.py: one eager
FusedRun step and one eager InvertRun step, options off and on, against the lists recorded on the commit before
(tests/launch_sequence.py, tests/golden/launch_sequence.json), kernel name by kernel name and tag by tag, in order. And the
scope is the setting made by hand: `sample` / `encode` with `freeu=` and `token_downsampling=` give the bits of the same call
with the two enabled on the UNet beforehand."""
import json
import os

import pytest
import torch

from tests import launch_sequence as L
from tests.test_windows_gpu import _tiny_model

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "launch_sequence.json")


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()[0]


def test_launch_lists_are_the_recorded_ones(tiny):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = L.record(tiny, L.inputs())
    assert sorted(got) == sorted(want) == ["fused_off", "fused_on", "invert_off", "invert_on"]
    for k in want:
        assert len(want[k]) > 100                        # a UNet forward and an update, not an empty trace
        assert got[k] == want[k], k
    names = lambda k: {n for n, _ in got[k]}
    assert not [n for n in names("fused_off") | names("invert_off") if n.startswith(("freeu", "ln_pool", "apg"))]
    assert {n.split("(")[0] for n in names("fused_on") if n.startswith(("freeu", "ln_pool", "apg"))} >= \
        {"freeu_apply", "ln_pool_tokens", "apg_reduce", "apg_apply"}
    assert not [n for n in names("invert_on") if n.startswith("apg")]


def test_scoped_call_is_the_setting_made_by_hand(tiny):
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    net = tiny.model.diffusion_model
    inp = L.inputs()
    cond, uc = inp["branches"]

    def sample(**kw):
        out, _ = DDIMSampler(tiny).sample(S=L.S, batch_size=1, shape=tuple(inp["x"].shape[1:]), conditioning=cond, verbose=False,
                                          unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=1.0,
                                          x_T=inp["x"], fs=inp["fs"], timestep_spacing="uniform_trailing", guidance_rescale=0.0,
                                          noises=inp["noises"], apg=dict(L.APG), **kw)
        return out.clone()

    def encode(**kw):
        s = DDIMSampler(tiny)
        s.make_schedule(L.S, ddim_discretize="uniform_trailing", ddim_eta=0.0, verbose=False)
        return s.encode(inp["x"], cond, L.S, fs=inp["fs"], unconditional_guidance_scale=2.0, unconditional_conditioning=uc,
                        **kw)[0].clone()

    scoped = sample(freeu=L.FREEU, token_downsampling=L.TODO), encode(freeu=L.FREEU, token_downsampling=L.TODO)
    assert net.freeu is None and net.token_downsampling is None
    off = sample(), encode()
    net.enable_freeu(**L.FREEU)
    net.enable_token_downsampling(**L.TODO)
    try:
        by_hand = sample(), encode()
    finally:
        net.disable_freeu()
        net.disable_token_downsampling()
    for a, b, c in zip(scoped, by_hand, off):
        assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, c)
