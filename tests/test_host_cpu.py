"""CPU-side tests (no GPU): the C-ABI library loads and exports every declared symbol, host-side schedule logic is
bit-exact against the reference's golden tables, state_dict keys match the reference's, the registry resolves the
released YAMLs, and the clip-sharding path works across 2 gloo ranks."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_cabi_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "dcrafter_hip.h")).read()
    declared = set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", hdr))
    from dynamicrafter_amd import _hip
    assert declared == set(_hip.SIGNATURES), (declared ^ set(_hip.SIGNATURES))
    lib = _hip.lib()                       # raises if the .so or any symbol is missing
    for name in declared:
        assert hasattr(lib, name)
    assert lib.dc_version().startswith(b"dcrafter_hip")
    # exported as plain C symbols (no torch types in the ABI)
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (dc_[a-z0-9_]+)", nm))
    assert declared <= exported


def test_cabi_argument_errors_without_gpu():
    """Bad arguments are rejected before any launch (return codes, no exceptions from C)."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    p = _hip.DcGemmParams()
    p.M, p.N, p.K = 128, 64, 63            # K not a multiple of 64
    import ctypes as C
    assert lib.dc_gemm_conv(C.byref(p), None) == -1
    assert lib.dc_layernorm(None, 0, None, 0, None, None, 1, 64, 1e-5, None) == -2
    assert lib.dc_temporal_attn_d64(C.c_void_p(8), 64, C.c_void_p(8), 64, 1, 17, 4, 1, 0.125, None) == -1


def test_gemm_plan_validation_without_gpu():
    """dc_gemm_set_plan: bits 0, 1, 4-7 are kernel-selection bits, bit 3 is accepted and dropped, bit 2 and values past 511 are
    rejected; the call returns the previous plan (no GPU work)."""
    from dynamicrafter_amd import _hip
    lib = _hip.lib()
    prev = lib.dc_gemm_set_plan(19)
    assert prev >= 0
    try:
        assert lib.dc_gemm_set_plan(19 | 64 | 128) == 19
        assert lib.dc_gemm_set_plan(11) == (19 | 64 | 128)          # bit 3 dropped on the way in
        assert lib.dc_gemm_set_plan(4) == -2 and lib.dc_gemm_set_plan(512) == -2 and lib.dc_gemm_set_plan(-1) == -2
        assert lib.dc_gemm_set_plan(0) == 3
    finally:
        lib.dc_gemm_set_plan(prev)


CSRC = os.path.join(ROOT, "dynamicrafter_amd", "csrc")


# (file, fewest functions its assembly must yield - the bound the ff_fused test always had; elsewhere `pieces > 0` below is what
#  shows that the LDS-DMA kernels were found -, may it save and restore m0)
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("name,min_kernels,keeps_m0", [
    pytest.param("ff_fused", 10, False, id="ff_fused"),
    pytest.param("gemm_conv", 1, False, id="gemm_conv"),
    pytest.param("gemm_conv_glds", 1, True, id="gemm_conv_glds"),      # its 8-wave kernels issue through lds_dma16_keep_m0
])
def test_isa_keeps_m0_for_the_lds_dma_only(tmp_path, name, min_kernels, keeps_m0):
    """The LDS-DMA pieces issued through lds_dma16 / lds_dma16_sbase (csrc/lds_stage.h) write m0 without saving it (two scalar
    moves per piece are issue slots of a one-wave-per-SIMD stream). That is only sound while nothing else in those kernels
    reads or writes m0: checked here in the ISA hipcc emits for the flags build.sh gives each file - every m0 reference must
    be an `s_mov_b32 m0, s..` of a piece (or, only in the file that uses lds_dma16_keep_m0, the `s_mov_b32 s.., m0` that saves
    it), and every kernel that issues global_load_lds must set m0 at least as often."""
    # the per-file flags come from build.sh's own file_flags function
    fn = [ln for ln in open(os.path.join(CSRC, "build.sh")) if ln.startswith("file_flags()")]
    assert len(fn) == 1
    file_flags = subprocess.run(["bash", "-c", fn[0] + f"file_flags {name}"], capture_output=True, text=True, check=True).stdout.split()
    assert name != "ff_fused" or "-fno-slp-vectorize" in file_flags      # the flag this file's ISA was always checked under
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *file_flags,
                          f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "--cuda-device-only", "-S", "-o",
                          str(tmp_path / "k.s"), os.path.join(CSRC, name + ".hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = re.findall(r"^(_Z\S+):[^\n]*\n(.*?)\.Lfunc_end", open(tmp_path / "k.s").read(), re.S | re.M)
    assert len(kernels) >= min_kernels
    allowed = r"s_mov_b32 (m0, s\d+|s\d+, m0)$" if keeps_m0 else r"s_mov_b32 m0, s\d+"
    pieces = 0
    for kname, body in kernels:
        lines = [ln.strip() for ln in body.splitlines() if "m0" in ln and not ln.strip().startswith(";")]
        other = [ln for ln in lines if not re.match(allowed, ln)]
        assert not other, (kname, other[:3])
        sets = [ln for ln in lines if re.match(r"s_mov_b32 m0, s\d+", ln)]
        assert len(sets) >= body.count("global_load_lds_dwordx4"), kname
        pieces += body.count("global_load_lds_dwordx4")
    assert pieces > 0


def test_lds_dma_asm_lives_in_lds_stage_h_only():
    """One spelling of the LDS-DMA inline asm (and of its m0 rule): outside csrc/lds_stage.h the instruction may be named in
    comments only."""
    def code(path):
        text = open(path).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert "lds_stage.h" in files and len(files) > 10
    users = [f for f in files if "global_load_lds_dwordx4" in code(os.path.join(CSRC, f))]
    assert users == ["lds_stage.h"], users


def test_gemm_parts_are_spelled_once():
    """One spelling of the packed bf16 residual add (csrc/dc_common.h: add_bf2 / add_bf8) and of the conv modes' tap-validity
    masks (csrc/gemm_parts.h): no kernel file writes either out by hand. Two named exemptions, each one loop, because every
    other spelling changed instructions inside the kernel's K loop (profiles/gemm_parts_isa.txt): set_issue_tile of
    gemm_persist_kernel (gemm_conv_glds.hip) and the 3-bit temporal mask of gemm_pipe320x16_kernel (gemm_pipe16.h)."""
    def code(path):
        text = open(path).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert "gemm_parts.h" in files and "dc_common.h" in files and len(files) > 10
    adders = [f for f in files if "& 0xffff0000u) + __uint_as_float(" in code(os.path.join(CSRC, f))]
    assert adders == ["dc_common.h"], adders
    maskers = {f: code(os.path.join(CSRC, f)).count("|= 1 << t") for f in files}
    assert {f: n for f, n in maskers.items() if n} == {"gemm_parts.h": 1, "gemm_conv_glds.hip": 1, "gemm_pipe16.h": 1}, maskers
    glds = code(os.path.join(CSRC, "gemm_conv_glds.hip"))
    assert glds.index("auto set_issue_tile") < glds.index("|= 1 << t") < glds.index("auto issue_next_part")
    pipe = code(os.path.join(CSRC, "gemm_pipe16.h"))
    assert "tt < p.T) mk |= 1 << t" in pipe


def test_attn_parts_are_spelled_once():
    """One spelling of the fragment scheme of the 32x32x16 attention kernels (csrc/attn_parts.h): the pre-scaled Q fragment,
    the lane offset of the transposed V read, the two transposed reads 8 V rows apart, the permlane-swap store, and one V row
    pitch. Named exemptions, each because every shared spelling moved instructions between the kernel's MFMAs or grew its
    registers (profiles/attn_parts_isa.txt): flash_attn_d64_kernel (attention.hip) reads its V^T fragment and stages its K / V
    rows by hand; flash_attn_d64_pipe_kernel (flash_pipe.hip) issues the two reads of a V^T fragment in different gaps of its
    schedule (rd_v_half) and keeps its store epilogue."""
    def code(path):
        text = open(path).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert "attn_parts.h" in files and len(files) > 10
    src = {f: code(os.path.join(CSRC, f)) for f in files}
    count = lambda pattern: {f: n for f in files if (n := len(re.findall(pattern, src[f])))}
    # 8 bf16 times one scalar, rounded to bf16 again: the Q pre-scale (and the pipe kernel's rescale of the packed P, through it)
    assert count(r"<< 16\) \* (\w+), __uint_as_float\([^()]* & 0xffff0000u\) \* \1\)") == {"attn_parts.h": 1}
    # lane -> offset of its transposed V read
    assert count(r"\(\(\(lane >> 4\) & 1\) \* 16 \+ \(\w+ & 3\) \* 4\) \* 2") == {"attn_parts.h": 1}
    # the read 8 V rows further on
    assert count(r"\+ 8 \* \w*VLD\b") == {"attn_parts.h": 1, "attention.hip": 1, "flash_pipe.hip": 1}
    att, fp = src["attention.hip"], src["flash_pipe.hip"]
    k0, k1 = att.index("void flash_attn_d64_kernel("), att.index("void cross_attn_resident_kernel(")
    assert k0 < att.index("+ 8 * ATTN_VLD") < k1
    assert fp.index("auto rd_v_half") < fp.index("+ 8 * ATTN_VLD") < fp.index("auto rescale")
    # K / V row staging: lds_off128 for K, the pitch for V
    assert count(r"\w+ \* ATTN_VLD \+ chunk \* 16") == {"attn_parts.h": 1, "attention.hip": 1, "flash_pipe.hip": 1}
    assert att.index("auto store_tile") < att.index("* ATTN_VLD + chunk * 16") < att.index("f32x16_t oacc[QB][2]")
    assert "vso = (unsigned)(FP_KBYTES + srow * ATTN_VLD + chunk * 16)" in fp       # an offset for its own stores, kept in a register
    # the permlane-swap store
    assert count(r"permlane32_swap") == {"attn_parts.h": 2, "flash_pipe.hip": 2}
    assert fp.index("row_sums();") < fp.index("permlane32_swap") and fp.count("void flash_attn_d64_pipe_kernel(") == 1
    # one pitch, one name
    for f in ("attention.hip", "flash_pipe.hip", "ff_fused.hip"):
        assert not re.search(r"\b(V_LD|FP_VLD|TA_VLD)\b", src[f]), f
        assert not re.search(r"\b192\b", src[f]), f
    assert len(re.findall(r"\b192\b", src["attn_parts.h"])) == 1


def test_pack_parts_are_spelled_once():
    """One spelling of the pack stage of the JPEG, GIF and PNG encoders (csrc/stream_pack.h): the wave prefix sum and the
    per-frame scan with its running base live there and the three kernel files include it; the integer wave reductions live
    in csrc/dc_common.h beside the float ones."""
    def code(path):
        text = open(path).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert "stream_pack.h" in files and "dc_common.h" in files and len(files) > 10
    src = {f: code(os.path.join(CSRC, f)) for f in files}
    users = lambda text: [f for f in files if text in src[f]]
    assert users("if (lane >= o) inc += up") == ["stream_pack.h"]                           # the wave prefix-sum step
    assert users("part[0] + part[1] + part[2] + part[3]") == ["stream_pack.h"]              # the frame scan's running base
    for name in ("wave_sum_i", "wave_max_i", "wave_sum_u64"):
        definers = [f for f in files if re.search(r"__device__[^;{()]*\b" + name + r"\s*\(", src[f])]
        assert definers == ["dc_common.h"], (name, definers)
    for f in ("jpeg.hip", "gif.hip", "png.hip"):
        assert '#include "stream_pack.h"' in src[f], f


def _tiny_model(config_name, extra=None):
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from tests.golden_cfg import TINY_AE, TINY_UNET
    cfg = yaml.safe_load(open(os.path.join(ROOT, "dynamicrafter_amd", "configs", config_name)))
    p = cfg["model"]["params"]
    p["unet_config"]["params"] = dict(TINY_UNET, default_fs=p["unet_config"]["params"]["default_fs"], **(extra or {}))
    p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
    for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
        p[k] = {"target": "torch.nn.Identity"}
    return instantiate_from_config(cfg["model"])


def test_host_schedules_bit_exact_vs_reference():
    from dynamicrafter_amd.lvdm.models.samplers.ddim import DDIMSampler
    g = np.load(os.path.join(G, "schedules.npz"))
    for tag in ("256", "512", "1024"):
        m = _tiny_model(f"inference_{tag}_v1.0.yaml")
        for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                  "sqrt_one_minus_alphas_cumprod"):
            assert np.array_equal(getattr(m, k).numpy(), g[f"{tag}/{k}"]), (tag, k)
        if m.use_dynamic_rescale:
            assert np.array_equal(m.scale_arr.numpy(), g[f"{tag}/scale_arr"])
        for S in (10, 50):
            for disc in ("uniform", "uniform_trailing"):
                for eta in (0, 1):
                    s = DDIMSampler(m)
                    s.make_schedule(S, ddim_discretize=disc, ddim_eta=float(eta), verbose=False)
                    key = f"{tag}/S{S}/{disc}/eta{eta}"
                    assert np.array_equal(s.ddim_timesteps, g[key + "/ddim_timesteps"])
                    for nm in ("a_t", "a_prev", "sigma_t", "sqrt_one_minus_at"):
                        assert np.array_equal(s._tables[nm].numpy()[::-1], g[f"{key}/{nm}"], equal_nan=True), (key, nm)
                    if m.use_dynamic_rescale:
                        assert np.array_equal(s._tables["scale_ratio"].numpy()[::-1],
                                              g[key + "/scale_prev"] / g[key + "/scale_t"])


def test_released_yaml_instantiates_with_reference_keys():
    """The full 1024 config through the registry; UNet state_dict keys/shapes == the reference's 1516 tensors."""
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "dynamicrafter_amd", "configs", "inference_1024_v1.0.yaml")))
    unet = instantiate_from_config(cfg["model"]["params"]["unet_config"].copy() | {"params": dict(
        cfg["model"]["params"]["unet_config"]["params"])})
    g = np.load(os.path.join(G, "unet_fullwidth_8x8.npz"))
    digest = sorted(f"{k}:{'x'.join(map(str, v.shape))}" for k, v in unet.state_dict().items())
    assert digest == [str(s) for s in g["key_digest"]]
    assert sum(p.numel() for p in unet.parameters()) == 1438854980
    # the OpenCLIP towers are built from the released YAML entries; their state_dict keys are the open_clip CLIP object's
    # (text wrapper: no `visual.*`; vision wrapper: no `transformer.*`) - what `cond_stage_model.*` / `embedder.*` of a
    # released checkpoint hold. Built on the meta device here (2 x ~0.7 B parameters).
    from oracle import clip as oclip
    with torch.device("meta"):
        enc = instantiate_from_config(cfg["model"]["params"]["cond_stage_config"])
        emb = instantiate_from_config(cfg["model"]["params"]["img_cond_stage_config"])
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == oclip.clip_text_shapes()
    assert {k: tuple(v.shape) for k, v in emb.state_dict().items()} == oclip.clip_vision_shapes()
    assert enc.layer == "penultimate" and enc.layer_idx == 1
    assert sum(v.numel() for k, v in emb.state_dict().items() if "visual" in k) == 632076800       # ViT-H/14 vision tower
    with pytest.raises(FileNotFoundError):                       # no BPE vocabulary in this image: loud, not silent
        enc.tokenize(["a prompt"])
    with pytest.raises(RuntimeError):                            # and no CPU fallback
        enc(torch.zeros(1, 77, dtype=torch.long))
    # reference YAML content is unchanged (tests/golden/reference_yaml.npz: digest of the reference's file, parsed)
    ref = str(np.load(os.path.join(G, "reference_yaml.npz"))["inference_1024_sha256"])
    assert hashlib.sha256(json.dumps(cfg, sort_keys=True).encode()).hexdigest() == ref


def test_load_model_checkpoint_key_conventions(tmp_path):
    """inference.py:34-59: Lightning {"state_dict": ...} strict load, the 256-release `framestride_embed` rename, and
    the DeepSpeed {"module": {"_forward_module.<key>": ...}} form. Host-side only (weights stay on the CPU)."""
    from collections import OrderedDict
    from dynamicrafter_amd.scripts.evaluation.inference import load_model_checkpoint
    from dynamicrafter_amd.utils.utils import instantiate_from_config
    from tests.golden_cfg import TINY_AE, TINY_UNET

    def build():
        cfg = yaml.safe_load(open(os.path.join(ROOT, "dynamicrafter_amd", "configs", "inference_256_v1.0.yaml")))
        p = cfg["model"]["params"]
        p["unet_config"]["params"] = dict(TINY_UNET, image_cross_attention_scale_learnable=True)
        p["first_stage_config"]["params"]["ddconfig"] = dict(TINY_AE)
        for k in ("cond_stage_config", "img_cond_stage_config", "image_proj_stage_config"):
            p[k] = {"target": "torch.nn.Identity"}
        return instantiate_from_config(cfg["model"])

    src = build()
    g = torch.Generator().manual_seed(5)
    sd = OrderedDict((k, torch.empty_like(v).normal_(generator=g) if v.is_floating_point() else v.clone())
                     for k, v in src.state_dict().items())
    assert any("fps_embedding" in k for k in sd) and any("temopral_conv" in k for k in sd)     # reference spellings

    def check(m):
        got = m.state_dict()
        assert list(got) == list(sd)
        assert all(torch.equal(got[k], sd[k]) for k in sd)

    # (1) Lightning checkpoint from a file
    f = tmp_path / "model.ckpt"
    torch.save({"state_dict": sd, "epoch": 3}, f)
    check(load_model_checkpoint(build(), str(f)))
    # (2) 256-release key name
    old = OrderedDict((k.replace("fps_embedding", "framestride_embed"), v) for k, v in sd.items())
    check(load_model_checkpoint(build(), {"state_dict": old}))
    # (3) DeepSpeed
    check(load_model_checkpoint(build(), {"module": OrderedDict(("_forward_module." + k, v) for k, v in sd.items())}))
    # a wrong key still fails loudly (strict)
    bad = OrderedDict(sd); bad["model.diffusion_model.nonexistent.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        load_model_checkpoint(build(), {"state_dict": bad})


def test_unsupported_configuration_is_loud():
    from dynamicrafter_amd.lvdm.modules.networks.openaimodel3d import UNetModel
    from tests.golden_cfg import TINY_UNET
    with pytest.raises(NotImplementedError):
        UNetModel(**dict(TINY_UNET, num_head_channels=32))
    with pytest.raises(NotImplementedError):
        UNetModel(**dict(TINY_UNET, use_relative_position=True))


def test_shard_indices_match_reference_semantics():
    from dynamicrafter_amd.parallel import shard_indices
    assert shard_indices(8, 8, 3) == [3]
    assert shard_indices(10, 4, 0) == [0, 1] and shard_indices(10, 4, 3) == [6, 7]     # tail (8, 9) dropped
    assert shard_indices(3, 8, 2) == []


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from dynamicrafter_amd.parallel import scatter_conditioning, gather_clips, shard_indices
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
full = None
if rank == 0:
    g = torch.Generator().manual_seed(0)
    full = {"ctx": torch.randn(4, 333, 16, generator=g), "c_concat": torch.randn(4, 4, 2, 3, 3, generator=g),
            "fs": torch.arange(4, dtype=torch.int64)}
mine = scatter_conditioning(full, src=0)
g = torch.Generator().manual_seed(0)
ref = {"ctx": torch.randn(4, 333, 16, generator=g), "c_concat": torch.randn(4, 4, 2, 3, 3, generator=g),
       "fs": torch.arange(4, dtype=torch.int64)}
idx = shard_indices(4, world, rank)
for k in ref:
    assert torch.equal(mine[k], ref[k][idx]), (rank, k)
out = gather_clips(mine["c_concat"] * 2, dst=0)
if rank == 0:
    assert torch.equal(out, ref["c_concat"] * 2)
dist.barrier()
print("rank", rank, "ok")
'''


def test_two_rank_scatter_gather_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29631", str(script), ROOT],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == 2


def _png_decode(path):
    """Minimal PNG/APNG reader for the writer tests: checks every chunk CRC, returns (frames [t,h,w,c], fps or None)."""
    import struct
    import zlib
    b = open(path, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    pos, w = 8, None
    frames, cur, delay = [], b"", None
    while pos < len(b):
        n, tag = struct.unpack(">I4s", b[pos:pos + 8])
        data = b[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", b[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        pos += 12 + n
        if tag == b"IHDR":
            w, h, depth, color = struct.unpack(">IIBB", data[:10])
            assert depth == 8
            c = {0: 1, 2: 3, 6: 4}[color]
        elif tag == b"fcTL":
            if cur:
                frames.append(cur); cur = b""
            delay = struct.unpack(">HH", data[20:24])
        elif tag == b"IDAT":
            cur += data
        elif tag == b"fdAT":
            cur += data[4:]
        elif tag == b"IEND":
            frames.append(cur)
    out = []
    for f in frames:
        raw = np.frombuffer(zlib.decompress(f), dtype=np.uint8).reshape(h, 1 + w * c)
        assert (raw[:, 0] == 0).all()
        out.append(raw[:, 1:].reshape(h, w, c))
    return np.stack(out), (None if delay is None else delay[1] / delay[0])


def test_png_and_apng_writers_round_trip(tmp_path):
    from dynamicrafter_amd.utils.save_video import write_apng, write_png
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    dec, fps = _png_decode(write_png(str(tmp_path / "a" / "still.png"), img))
    assert fps is None and np.array_equal(dec[0], img)
    clip = rng.integers(0, 256, size=(5, 16, 24, 3), dtype=np.uint8)
    dec, fps = _png_decode(write_apng(str(tmp_path / "clip.png"), torch.from_numpy(clip), fps=8))
    assert fps == 8 and np.array_equal(dec, clip)
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "bad.png"), img.astype(np.float32))


def test_conv_weight_packing_matches_integration_doc():
    """INTEGRATION.md / include/dcrafter_hip.h state the conv weight layout a C-ABI caller must produce: bf16 [n_pad][K],
    K index = (ci // 64) * taps * 64 + tap * 64 + (ci % 64), tap = kh * 3 + kw (temporal: tap = kt), Cin zero-padded to
    a multiple of 64. Build it from that sentence and compare with what the host classes feed the kernels."""
    from dynamicrafter_amd.ops import PackedWeight
    g = torch.Generator().manual_seed(1)
    for co, ci in ((8, 3), (130, 64), (64, 192)):
        w = torch.randn(co, ci, 3, 3, generator=g)
        pw = PackedWeight.conv3x3(w, None, torch.device("cpu"))
        cip = (ci + 63) // 64 * 64
        assert pw.K == 9 * cip and pw.n_pad % 128 == 0 and pw.n_pad >= co
        doc = torch.zeros(pw.n_pad, pw.K)
        for c in range(ci):
            for kh in range(3):
                for kw in range(3):
                    doc[:co, (c // 64) * 9 * 64 + (kh * 3 + kw) * 64 + c % 64] = w[:, c, kh, kw]
        assert torch.equal(pw.w.float(), doc.to(torch.bfloat16).float())
    w = torch.randn(64, 128, 3, 1, 1, generator=g)
    pw = PackedWeight.tconv3(w, None, torch.device("cpu"))
    doc = torch.zeros(pw.n_pad, pw.K)
    for c in range(128):
        for kt in range(3):
            doc[:64, (c // 64) * 3 * 64 + kt * 64 + c % 64] = w[:, c, kt, 0, 0]
    assert torch.equal(pw.w.float(), doc.to(torch.bfloat16).float())


def test_load_model_checkpoint_safetensors(tmp_path):
    """Community releases ship the same keys as a flat .safetensors file (README.md:384-385): accepted as a state dict."""
    from safetensors.torch import save_file
    from dynamicrafter_amd.scripts.evaluation.inference import load_model_checkpoint
    src = _tiny_model("inference_512_v1.0.yaml")
    g = torch.Generator().manual_seed(6)
    sd = {k: (torch.empty_like(v).normal_(generator=g).half() if v.is_floating_point() else v.clone())
          for k, v in src.state_dict().items()}
    f = tmp_path / "model.safetensors"
    save_file(sd, str(f))
    m = load_model_checkpoint(_tiny_model("inference_512_v1.0.yaml"), str(f))
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k].to(got[k].dtype)) for k in sd)


_BENCH_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
import bench
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
mine = bench.distribute_inputs("256", world, rank, torch.device("cpu"))
ref = bench.make_clip_inputs("256", world)
for k, v in ref.items():
    assert mine[k].shape[0] == 1 and torch.equal(mine[k], v[rank:rank + 1]), (rank, k)
assert not torch.equal(ref["cond_ctx"][0], ref["cond_ctx"][1])          # the clips are distinct
dist.barrier()
print("rank", rank, "ok")
'''


def test_bench_conditioning_scatter_two_ranks_gloo(tmp_path):
    """bench.py's N > 1 leg distributes N DISTINCT clips' conditioning with parallel.scatter_conditioning; the same
    function runs over RCCL on the GPUs. Rehearsed here on 2 gloo ranks (no GPU needed for this part of bench.py)."""
    script = tmp_path / "bench_worker.py"
    script.write_text(_BENCH_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29633", str(script), ROOT],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok") == 2
