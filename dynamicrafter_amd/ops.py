"""Tensor-level wrappers over the C ABI (include/dcrafter_hip.h).

Every function takes torch CUDA tensors purely as (pointer, stride) carriers and enqueues HIP kernels on the
current torch stream. Activations are channels-last bf16 rows: 2-D tensors [rows, C] with stride (ld, 1).
Nothing here computes with torch.
"""
import ctypes as C
import os
import math

import torch

from . import _hip
from ._hip import DcDdimParams, DcGemmParams, check

_BF16 = torch.bfloat16


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Tracer:
    """Per-launch HIP-event timing + algorithmic work accounting (bench.py's roofline leg). While a Tracer is
    installed (`with Tracer() as tr:`) every heavy op brackets its launch with two hipEvents on the launch stream;
    `summary()` reduces them per kernel family: launches, total ms, FLOPs, algorithmic HBM bytes."""

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _TRACE
        _TRACE = self
        return self

    def __exit__(self, *a):
        global _TRACE
        _TRACE = None

    def _event(self):
        e = C.c_void_p()
        check(_hip.lib().dc_event_create(C.byref(e)), "dc_event_create")
        return e

    def summary(self):
        l = _hip.lib()
        out = {}
        self.detail = {}
        for name, flops, nbytes, e0, e1, tag in self.records:
            ms = C.c_float()
            check(l.dc_event_elapsed_ms(e0, e1, C.byref(ms)), "dc_event_elapsed_ms")
            d = out.setdefault(name, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1; d["ms"] += ms.value; d["flops"] += flops; d["bytes"] += nbytes
            if tag is not None:
                dd = self.detail.setdefault((name, tag), dict(launches=0, ms=0.0, flops=0.0))
                dd["launches"] += 1; dd["ms"] += ms.value; dd["flops"] += flops
            l.dc_event_destroy(e0); l.dc_event_destroy(e1)
        self.records = []
        return out


_TRACE = None


def _launch(name, flops, nbytes, fn, *args, tag=None):
    tr = _TRACE
    if tr is None:
        check(fn(*args), name)
        return
    l = _hip.lib()
    e0, e1 = tr._event(), tr._event()
    sp = stream_ptr()
    l.dc_event_record(e0, sp)
    check(fn(*args), name)
    l.dc_event_record(e1, sp)
    if name == "dc_gemm_conv":                      # label by the kernel family the dispatcher actually launched
        name = l.dc_gemm_last_variant().decode()
    tr.records.append((name, flops, nbytes, e0, e1, tag))


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _rows(t, name="tensor", dtype=_BF16):
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1 or not t.is_cuda:
        raise ValueError(f"{name}: expected CUDA {dtype} rows [R, C] with unit column stride, got "
                         f"{t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    return t


class PackedWeight:
    """Device copy of a Linear / conv weight in the layout dc_gemm_conv consumes: bf16 [n_pad][K]; conv K is
    ordered (64-channel slice, tap, channel); rows zero-padded to a multiple of 128. Derived from the
    nn.Parameter, never serialised."""

    __slots__ = ("w", "bias", "N", "K", "n_pad", "Cin", "taps", "k_real")

    def __init__(self, w, bias, N, K, Cin, taps, k_real=None):
        self.w, self.bias, self.N, self.K, self.Cin, self.taps = w, bias, N, K, Cin, taps
        self.n_pad = w.shape[0]
        self.k_real = k_real        # un-padded reduction length (algorithmic FLOP accounting)

    @staticmethod
    def _finish(w2d, bias, device, Cin, taps, pad_n_to=None):
        N, K = w2d.shape
        n_pad = (N + 127) // 128 * 128
        if pad_n_to is not None:
            n_pad = max(n_pad, pad_n_to)
        wp = torch.zeros((n_pad, K), dtype=_BF16, device=device)
        wp[:N] = w2d.to(device=device, dtype=_BF16)
        b = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
        return PackedWeight(wp, b, N, K, Cin, taps)

    @staticmethod
    def linear(weight, bias, device, n_align=1):
        """nn.Linear / Conv1d(k=1) / Conv2d(k=1) weight [N, K, ...]. n_align pads N (zero rows + zero bias)."""
        w = weight.detach().reshape(weight.shape[0], -1)
        N, K = w.shape
        if K % 64 != 0:
            kp = (K + 63) // 64 * 64
            w = torch.nn.functional.pad(w, (0, kp - K))
        if N % n_align != 0:
            npad = (N + n_align - 1) // n_align * n_align
            w = torch.nn.functional.pad(w, (0, 0, 0, npad - N))
            if bias is not None:
                bias = torch.nn.functional.pad(bias.detach(), (0, npad - N))
        return PackedWeight._finish(w, bias, device, w.shape[1], 1)

    @staticmethod
    def conv3x3(weight, bias, device, n_align=1):
        """nn.Conv2d 3x3 weight [Cout, Cin, 3, 3] -> [Cout][kh][kw][Cin_pad64]."""
        co, ci = weight.shape[0], weight.shape[1]
        w = weight.detach().permute(0, 2, 3, 1)
        cip = (ci + 63) // 64 * 64
        if cip != ci:
            w = torch.nn.functional.pad(w, (0, cip - ci))
        # K order = (64-channel slice, tap, channel-in-slice): the kernel walks all 9 taps of a slice back to back
        w = w.reshape(co, 9, cip // 64, 64).permute(0, 2, 1, 3).reshape(co, 9 * cip)
        if co % n_align != 0:
            npad = (co + n_align - 1) // n_align * n_align
            w = torch.nn.functional.pad(w, (0, 0, 0, npad - co))
            if bias is not None:
                bias = torch.nn.functional.pad(bias.detach(), (0, npad - co))
        pw = PackedWeight._finish(w, bias, device, cip, 9)
        pw.k_real = 9 * ci
        return pw

    @staticmethod
    def conv3x3_c8_as_linear(weight, bias, device):
        """nn.Conv2d 3x3 weight [Cout, Cin <= 8, 3, 3] -> the Linear weight [Cout][128] that goes with ops.im2col3x3_c8:
        k = 8 (kh*3 + kw) + c, zeros elsewhere."""
        co, ci = weight.shape[0], weight.shape[1]
        assert ci <= 8
        w = torch.zeros(co, 16, 8, dtype=weight.dtype)
        w[:, :9, :ci] = weight.detach().permute(0, 2, 3, 1).reshape(co, 9, ci)
        pw = PackedWeight._finish(w.reshape(co, 128), bias, device, 128, 1)
        pw.k_real = 9 * ci
        return pw

    @staticmethod
    def tconv3(weight, bias, device):
        """nn.Conv3d (3,1,1) weight [Cout, Cin, 3, 1, 1] -> [Cout][kt][Cin]."""
        co, ci = weight.shape[0], weight.shape[1]
        assert ci % 64 == 0, "temporal conv width must be a multiple of 64"
        w = weight.detach().reshape(co, ci // 64, 64, 3).permute(0, 1, 3, 2).reshape(co, 3 * ci)   # (slice, tap, channel)
        return PackedWeight._finish(w, bias, device, ci, 3)


def gemm(a, pw, out, *, M=None, residual=None, rowvec=None, rows_per_vec=1, geglu=False, gelu=False, alpha=1.0,
         conv=None, tconv=None):
    """out[M, N] = epilogue(gather(a) @ pw.w[:N].T). `out` dtype bf16 or float32 selects the output type.

    conv  = dict(IH, IW, OH, OW, stride, pad, ups)   -> 3x3 implicit GEMM over frames of a
    tconv = dict(T, HW)                               -> 3-tap temporal conv
    """
    _rows(a, "a")
    out_f32 = out.dtype == torch.float32
    if not out_f32:
        _rows(out, "out")
    p = DcGemmParams()
    p.A, p.W, p.C = a.data_ptr(), pw.w.data_ptr(), out.data_ptr()
    p.bias = 0 if pw.bias is None else pw.bias.data_ptr()
    p.rowvec = 0 if rowvec is None else rowvec.data_ptr()
    p.rowvec_ld = 0 if rowvec is None else rowvec.stride(0)
    p.rows_per_vec = rows_per_vec
    p.residual = 0 if residual is None else _rows(residual, "residual").data_ptr()
    p.ldr = 0 if residual is None else residual.stride(0)
    p.lda, p.ldc = a.stride(0), out.stride(0)
    p.M = out.shape[0] if M is None else M
    p.N, p.K, p.n_pad = pw.N, pw.K, pw.n_pad
    p.Cin = pw.Cin
    p.flags = (_hip.DC_GEMM_OUT_F32 if out_f32 else 0) | (_hip.DC_GEMM_GEGLU if geglu else 0) | \
        (_hip.DC_GEMM_GELU if gelu else 0)
    p.alpha = alpha
    ws = _gemm_workspace(a.device, torch.cuda.current_stream().cuda_stream)
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    if conv is not None:
        p.mode = 1
        p.IH, p.IW, p.OH, p.OW = conv["IH"], conv["IW"], conv["OH"], conv["OW"]
        p.stride, p.pad, p.ups = conv.get("stride", 1), conv.get("pad", 1), conv.get("ups", 0)
        if pw.taps != 9 or a.shape[1] < pw.Cin:
            raise ValueError("conv3x3 weight / activation mismatch")
    elif tconv is not None:
        p.mode = 2
        p.T, p.HW = tconv["T"], tconv["HW"]
        if pw.taps != 3:
            raise ValueError("tconv weight mismatch")
    else:
        p.mode = 0
        if a.shape[1] < pw.K:
            raise ValueError(f"gemm: activation has {a.shape[1]} columns, weight K={pw.K}")
    n_out = pw.N // 2 if geglu else pw.N
    if out.shape[1] < n_out:
        raise ValueError(f"gemm: out has {out.shape[1]} columns, need {n_out}")
    # row extents the launch addresses (the C ABI takes raw pointers)
    if out.shape[0] < p.M or (residual is not None and (residual.shape[0] < p.M or residual.shape[1] < n_out)):
        raise ValueError(f"gemm: out/residual have fewer than M={p.M} rows (or residual fewer than {n_out} columns)")
    if p.mode == 1:
        if p.M % (p.OH * p.OW) != 0 or a.shape[0] < (p.M // (p.OH * p.OW)) * p.IH * p.IW:
            raise ValueError(f"conv3x3: M={p.M} output rows need {p.M // (p.OH * p.OW)} frames of {p.IH}x{p.IW} input rows, "
                             f"activation has {a.shape[0]}")
    elif a.shape[0] < p.M:
        raise ValueError(f"gemm: activation has {a.shape[0]} rows, M={p.M}")
    if p.mode == 2 and (p.M % (p.T * p.HW) != 0 or a.shape[1] < pw.Cin):
        raise ValueError("tconv: M must be a multiple of T*HW and the activation at least Cin wide")
    if rowvec is not None and (rowvec.shape[0] * rows_per_vec < p.M or rowvec.shape[1] < n_out):
        raise ValueError("gemm: rowvec does not cover every row group / output column")
    if _TRACE is not None:
        variant = "dc_gemm_conv"
        k_real = pw.k_real if pw.k_real else pw.K
        flops = 2.0 * p.M * pw.N * k_real
        esz = 4 if out_f32 else 2
        nbytes = 2.0 * p.M * (k_real if p.mode == 0 else pw.Cin) + 2.0 * pw.N * pw.K + esz * p.M * n_out \
            + (2.0 * p.M * n_out if residual is not None else 0)
        _launch(variant, flops, nbytes, _hip.lib().dc_gemm_conv, C.byref(p), stream_ptr(),
                tag=(p.mode, p.M, pw.N, k_real))
    else:
        check(_hip.lib().dc_gemm_conv(C.byref(p), stream_ptr()), "dc_gemm_conv")
    return out


def gemm_fits(M, pw):
    """Does out[M, pw.N] = a @ pw.w.T tile exactly into rounds of 288 x 320 tiles over this device's CUs (dc_gemm_fit_shape)?
    Shape only: gemm_fit itself still checks strides and alignment."""
    return bool(_hip.lib().dc_gemm_fit_shape(int(M), int(pw.N), int(pw.K)))


def gemm_fit(a, pw, out, residual=None):
    """out[M, N] = a @ pw.w[:N].T (+ pw.bias) (+ residual) on the exact-fit kernel (gemm_fit.hip); M = out.shape[0]. bf16 rows;
    bias and residual are added in fp32 and rounded once; `out` may be `residual`. Raises where the shape does not fit
    (gemm_fits): there is no second path behind it."""
    _rows(a, "a")
    _rows(out, "out")
    M = out.shape[0]
    if a.shape[0] < M or a.shape[1] < pw.K or out.shape[1] < pw.N or pw.taps != 1:
        raise ValueError(f"gemm_fit: a {tuple(a.shape)} / out {tuple(out.shape)} do not match the weight [N={pw.N}, K={pw.K}]")
    if residual is not None and (_rows(residual, "residual").shape[0] < M or residual.shape[1] < pw.N):
        raise ValueError(f"gemm_fit: residual {tuple(residual.shape)} does not cover [{M}, {pw.N}]")
    p = DcGemmParams()
    p.A, p.W, p.C = a.data_ptr(), pw.w.data_ptr(), out.data_ptr()
    p.bias = 0 if pw.bias is None else pw.bias.data_ptr()
    p.residual = 0 if residual is None else residual.data_ptr()
    p.ldr = 0 if residual is None else residual.stride(0)
    p.lda, p.ldc = a.stride(0), out.stride(0)
    p.M, p.N, p.K, p.n_pad = M, pw.N, pw.K, pw.n_pad
    p.Cin, p.mode, p.flags, p.alpha = pw.Cin, 0, 0, 1.0
    k_real = pw.k_real if pw.k_real else pw.K
    nbytes = 2.0 * M * k_real + 2.0 * pw.N * pw.K + 2.0 * M * pw.N * (2 if residual is not None else 1)
    _launch("gemm_fit_kernel", 2.0 * M * pw.N * k_real, nbytes, _hip.lib().dc_gemm_fit, C.byref(p), stream_ptr(),
            tag=(0, M, pw.N, k_real))
    return out


_gemm_ws = {}


def _gemm_workspace(device, stream):
    """One scratch buffer per (device, stream) for split-K partial sums: launches on one stream use it one after
    another; a graph replay on its private stream and eager work on another stream never share partials."""
    key = (device.index, stream)
    buf = _gemm_ws.get(key)
    if buf is None:
        buf = torch.empty(int(_hip.lib().dc_gemm_workspace_bytes()), dtype=torch.uint8, device=device)
        _gemm_ws[key] = buf
    return buf


class Arena:
    """Named, shape-keyed device scratch: allocated on first use, stable afterwards (graph-safe).

    DC_ARENA_GUARD=1 (debugging / tests): every buffer is carved out of a larger allocation with `GUARD` sentinel
    rows before and after it; `check()` raises if a launch wrote outside its buffer. The kernels take raw pointers,
    so this is the only place an overrun of a scratch buffer can be made visible."""
    GUARD = 8

    def __init__(self):
        self._bufs = {}
        self._guarded = {}
        self.guard = os.environ.get("DC_ARENA_GUARD", "0") == "1"

    def get(self, tag, rows, cols, dtype=_BF16, device=None, zero=False):
        key = (tag, rows, cols, dtype)
        b = self._bufs.get(key)
        if b is None:
            if rows * cols >= 2 ** 31:                  # the kernels index a buffer with 32-bit element offsets
                raise ValueError(f"scratch buffer {tag} [{rows} x {cols}] has 2^31 elements or more")
            if self.guard:
                G = self.GUARD
                whole = torch.empty((rows + 2 * G, cols), dtype=dtype, device=device)
                whole.fill_(self._sentinel(dtype))
                b = whole[G:G + rows]
                if zero:
                    b.zero_()
                self._guarded[key] = whole
            else:
                b = (torch.zeros if zero else torch.empty)((rows, cols), dtype=dtype, device=device)
            self._bufs[key] = b
        return b

    @staticmethod
    def _sentinel(dtype):
        return 12345.0 if dtype.is_floating_point else 0x5a

    def check(self):
        """Verify the guard rows of every buffer (guard mode only). Synchronises."""
        bad = []
        for (tag, rows, cols, dtype), whole in self._guarded.items():
            G = self.GUARD
            ref = torch.full((1,), self._sentinel(dtype), dtype=dtype, device=whole.device)
            if not (bool((whole[:G] == ref).all()) and bool((whole[G + rows:] == ref).all())):
                bad.append(f"{tag}[{rows}x{cols} {dtype}]")
        if bad:
            raise RuntimeError("scratch buffers overrun: " + ", ".join(bad))
        return len(self._guarded)

    def nbytes(self):
        return sum(b.numel() * b.element_size() for b in self._bufs.values())


_gn_ws = {}


_gn_ws_retired = []


def _gn_workspace(device, nbytes):
    """GroupNorm statistics scratch per (device, stream). A buffer that was ever handed out is never released: a captured
    hipGraph keeps its address, so a larger request allocates a new buffer and the old one is parked, not freed."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    buf = _gn_ws.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        if buf is not None:
            _gn_ws_retired.append(buf)
        buf = torch.empty((max(nbytes, 4 << 20) + 3) // 4, dtype=torch.float32, device=device)
        _gn_ws[key] = buf
    return buf


def _need(t, n, name):
    """The C ABI takes raw pointers: refuse operands smaller than the extent the kernel will touch."""
    if t is not None and t.numel() < n:
        raise ValueError(f"{name}: {t.numel()} elements, the launch reads/writes {n}")


def _need_rows(t, rows, cols, name):
    if t.shape[0] < rows or t.shape[1] < cols:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, the launch addresses [{rows}, {cols}]")


def groupnorm(x, y, gamma, beta, *, groups, n_inst, rows_per_inst, eps, silu):
    _rows(x, "x"); _rows(y, "y")
    _need_rows(x, n_inst * rows_per_inst, gamma.numel(), "x"); _need_rows(y, n_inst * rows_per_inst, gamma.numel(), "y")
    _need(beta, gamma.numel(), "beta")
    Cc = gamma.numel()
    l = _hip.lib()
    ws = _gn_workspace(x.device, int(l.dc_groupnorm_workspace_bytes(n_inst, groups, rows_per_inst)))
    _launch("groupnorm(2-3 kernels)", 0.0, 6.0 * n_inst * rows_per_inst * Cc, l.dc_groupnorm, _ptr(x), x.stride(0), _ptr(y),
            y.stride(0), _ptr(gamma), _ptr(beta), Cc, groups, n_inst, rows_per_inst, eps, 1 if silu else 0, _ptr(ws),
            stream_ptr())
    return y


def layernorm(x, y, gamma, beta, eps=1e-5):
    _rows(x, "x"); _rows(y, "y")
    _need_rows(x, x.shape[0], gamma.numel(), "x"); _need_rows(y, x.shape[0], gamma.numel(), "y"); _need(beta, gamma.numel(), "beta")
    _launch("layernorm", 0.0, 4.0 * x.shape[0] * gamma.numel(), _hip.lib().dc_layernorm, _ptr(x), x.stride(0), _ptr(y),
            y.stride(0), _ptr(gamma), _ptr(beta), x.shape[0], gamma.numel(), eps, stream_ptr())
    return y


POOL_MODES = {"nearest": 0, "mean": 1}


def pooled_grid(H, W, factor):
    """(Hp, Wp) = (ceil(H / factor), ceil(W / factor)): the token grid ln_pool_tokens writes."""
    return (H + factor - 1) // factor, (W + factor - 1) // factor


def ln_pool_tokens(x, y, gamma, beta, *, F, H, W, factor, mode, eps=1e-5):
    """y = the LayerNorm'd tokens of x on the grid pooled by `factor`: x bf16 rows [F*H*W, C] ordered (frame, y, x), y bf16 rows
    [F*Hp*Wp, C] with (Hp, Wp) = pooled_grid(H, W, factor). mode "nearest": LayerNorm(x)[::factor, ::factor] per frame, the bits
    of ops.layernorm at the kept rows; "mean": the mean of the LayerNorm'd tokens of each factor x factor cell, clipped at the
    border (avg_pool2d, ceil_mode=True, count_include_pad=False). The K/V tokens of a spatial self-attention with token
    downsampling (UNetModel.enable_token_downsampling); one launch, no atomics: bit-reproducible and graph-capturable."""
    _rows(x, "x"); _rows(y, "y")
    if mode not in POOL_MODES:
        raise ValueError(f"ln_pool_tokens: mode must be 'nearest' or 'mean', got {mode!r}")
    if isinstance(factor, bool) or not isinstance(factor, int) or not 2 <= factor <= 8:
        raise ValueError(f"ln_pool_tokens: factor must be an int in 2..8, got {factor!r}")
    Cc = gamma.numel()
    if Cc % 8 or not 0 < Cc <= 2048:
        raise ValueError(f"ln_pool_tokens: C must be a multiple of 8 and at most 2048, got {Cc}")
    if min(F, H, W) < 1 or x.shape[0] != F * H * W:
        raise ValueError(f"ln_pool_tokens: x is {tuple(x.shape)}, expected [F*H*W, C] = [{F * H * W}, {Cc}]")
    Hp, Wp = pooled_grid(H, W, factor)
    _need_rows(x, F * H * W, Cc, "x"); _need_rows(y, F * Hp * Wp, Cc, "y"); _need(beta, Cc, "beta")
    for t, n in ((x, "x"), (y, "y")):
        if t.stride(0) % 8 or t.data_ptr() % 16:
            raise ValueError(f"ln_pool_tokens: {n} needs a row stride that is a multiple of 8 and a 16-byte aligned start, got "
                             f"stride {t.stride(0)}, address % 16 = {t.data_ptr() % 16}")
    cell = 1 if mode == "nearest" else factor * factor
    _launch(f"ln_pool_tokens({mode})", 0.0, 2.0 * F * Hp * Wp * Cc * (min(cell, H * W) + 1), _hip.lib().dc_ln_pool_tokens, _ptr(x),
            x.stride(0), _ptr(y), y.stride(0), _ptr(gamma), _ptr(beta), F, H, W, Cc, factor, POOL_MODES[mode], eps, stream_ptr(),
            tag=f"F{F} {H}x{W} C{Cc} f{factor}")
    return y


def flash_attn(q, k, v, o, *, batch, heads, Lq, Lk, scale, accumulate=False, acc_scale=1.0, q_bstride=None,
               kv_bstride=None):
    """q/o rows [batch*Lq, >=heads*64]; k/v rows [batch*Lk, ...] (views into a fused qkv buffer are fine).
    q_bstride / kv_bstride: rows between consecutive batch items (default Lq / Lk)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
        _rows(t, n)
    qb = Lq if q_bstride is None else q_bstride
    kb = Lk if kv_bstride is None else kv_bstride
    _need_rows(q, (batch - 1) * qb + Lq, heads * 64, "q"); _need_rows(o, (batch - 1) * qb + Lq, heads * 64, "o")
    _need_rows(k, (batch - 1) * kb + Lk, heads * 64, "k"); _need_rows(v, (batch - 1) * kb + Lk, heads * 64, "v")
    _launch("flash_attn_d64(self)" if Lk > 128 else "flash_attn_d64(cross)", 4.0 * batch * heads * Lq * Lk * 64,
            2.0 * batch * heads * 64 * (2 * Lq + 2 * Lk), _hip.lib().dc_flash_attn_d64, _ptr(q), _ptr(k), _ptr(v), _ptr(o),
            q.stride(0), k.stride(0), v.stride(0), o.stride(0), batch, heads, Lq, Lk,
            Lq if q_bstride is None else q_bstride, Lk if kv_bstride is None else kv_bstride, scale,
            1 if accumulate else 0, acc_scale, stream_ptr())
    return o


def cross_attn_dual(q, k, v, k2, v2, o, *, batch, heads, Lq, Lk, Lk2, scale, scale2, kv_bstride):
    """o = attn(q; k, v) + scale2 * attn(q; k2, v2): text + image cross-attention of one query tensor in one launch.
    k/v/k2/v2 are column views of one projection buffer (same row stride), kv_bstride rows per batch item."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (k2, "k2"), (v2, "v2"), (o, "o")):
        _rows(t, n)
    if len({k.stride(0), v.stride(0), k2.stride(0), v2.stride(0)}) != 1:
        raise ValueError("cross_attn_dual: k, v, k2, v2 must share one row stride")
    _need_rows(q, batch * Lq, heads * 64, "q"); _need_rows(o, batch * Lq, heads * 64, "o")
    _need_rows(k, (batch - 1) * kv_bstride + Lk, heads * 64, "k"); _need_rows(v, (batch - 1) * kv_bstride + Lk, heads * 64, "v")
    _need_rows(k2, (batch - 1) * kv_bstride + Lk2, heads * 64, "k2"); _need_rows(v2, (batch - 1) * kv_bstride + Lk2, heads * 64, "v2")
    _launch("flash_attn_d64(cross)", 4.0 * batch * heads * Lq * (Lk + Lk2) * 64, 2.0 * batch * heads * 64 * (2 * Lq + 2 * (Lk + Lk2)),
            _hip.lib().dc_cross_attn_dual_d64, _ptr(q), _ptr(k), _ptr(v), _ptr(k2), _ptr(v2), _ptr(o), q.stride(0), k.stride(0),
            o.stride(0), batch, heads, Lq, Lk, Lk2, Lq, kv_bstride, scale, scale2, stream_ptr())
    return o


def temporal_attn(qkv, o, *, B, T, HW, heads, scale):
    _rows(qkv, "qkv"); _rows(o, "o")
    _need_rows(qkv, B * T * HW, 3 * heads * 64, "qkv"); _need_rows(o, B * T * HW, heads * 64, "o")
    _launch("temporal_attn_d64", 4.0 * B * HW * heads * T * T * 64, 2.0 * B * T * HW * heads * 64 * 4,
            _hip.lib().dc_temporal_attn_d64, _ptr(qkv), qkv.stride(0), _ptr(o), o.stride(0), B, T, HW, heads, scale,
            stream_ptr())
    return o


def ff2_permuted(weight, device):
    """ff.net.2.weight [320, 1280] -> bf16 [384, 1280] in the k order dc_ff_geglu_fused320 reads: inside every
    32-channel chunk, position 16 s + 8 h + e holds channel 8 (2 s + e // 4) + 4 h + e % 4."""
    w = weight.detach()
    N, K = w.shape
    pos = torch.arange(32)
    s_, h_, e_ = pos // 16, (pos // 8) % 2, pos % 8
    chan = 8 * (2 * s_ + e_ // 4) + 4 * h_ + e_ % 4
    idx = (torch.arange(K // 32)[:, None] * 32 + chan[None, :]).reshape(-1)
    n_pad = (N + 127) // 128 * 128
    out = torch.zeros((n_pad, K), dtype=_BF16, device=device)
    out[:N] = w[:, idx].to(device=device, dtype=_BF16)
    return out


def ff_geglu_fused320(x, pw1, w2p, b2, out, residual=None, ln=None, ln_eps=1e-5):
    """out = FeedForward_GEGLU(LayerNorm(x) if ln else x) (+ residual) for dim 320 in one launch; pw1 =
    PackedWeight.linear(ff.net.0.proj); ln = (gamma, beta) fp32 or None."""
    _rows(x, "x"); _rows(out, "out")
    M = x.shape[0]
    if pw1.K != 320 or pw1.N != 2560 or pw1.bias is None or tuple(w2p.shape[1:]) != (1280,) or w2p.shape[0] < 320:
        raise ValueError("ff_geglu_fused320: dim must be 320 (ff1 [2560, 320] with bias, ff2 [320, 1280])")
    _need_rows(x, M, 320, "x"); _need_rows(out, M, 320, "out")
    if residual is not None:
        _rows(residual, "residual"); _need_rows(residual, M, 320, "residual")
    if ln is not None:
        _need(ln[0], 320, "ln gamma"); _need(ln[1], 320, "ln beta")
    flops = 2.0 * M * (2560 + 1280) * 320
    nbytes = 2.0 * M * 320 * (3 if residual is not None else 2) + 2.0 * (2560 * 320 + 320 * 1280)
    _launch("ff_geglu_fused320", flops, nbytes, _hip.lib().dc_ff_geglu_fused320, _ptr(x), x.stride(0),
            _ptr(None if ln is None else ln[0]), _ptr(None if ln is None else ln[1]), ln_eps, _ptr(pw1.w), _ptr(pw1.bias),
            _ptr(w2p), _ptr(b2), _ptr(residual), 0 if residual is None else residual.stride(0), _ptr(out), out.stride(0), M,
            stream_ptr())
    return out


def ff_geglu_proj_fused320(x, pw1, w2p, b2, wp, bp, residual2, out, ln=None, ln_eps=1e-5):
    """out = residual2 + Linear_p(x + FeedForward_GEGLU(LayerNorm(x) if ln else x)) for dim 320 in one launch (the last two
    steps of a transformer: FeedForward with its residual, proj_out with the transformer's residual); wp =
    ff2_permuted(proj_out.weight)."""
    _rows(x, "x"); _rows(out, "out"); _rows(residual2, "residual2")
    M = x.shape[0]
    if pw1.K != 320 or pw1.N != 2560 or pw1.bias is None or tuple(w2p.shape[1:]) != (1280,) or w2p.shape[0] < 320 \
            or tuple(wp.shape[1:]) != (320,) or wp.shape[0] < 320:
        raise ValueError("ff_geglu_proj_fused320: dim must be 320 (ff1 [2560, 320] with bias, ff2 [320, 1280], proj [320, 320])")
    if x.data_ptr() == out.data_ptr():
        raise ValueError("ff_geglu_proj_fused320: out must not alias x")
    _need_rows(x, M, 320, "x"); _need_rows(out, M, 320, "out"); _need_rows(residual2, M, 320, "residual2")
    _need(b2, 320, "b2"); _need(bp, 320, "bp")
    if ln is not None:
        _need(ln[0], 320, "ln gamma"); _need(ln[1], 320, "ln beta")
    _launch("ff_geglu_proj_fused320", 2.0 * M * (2560 + 1280 + 320) * 320, 2.0 * M * 320 * 3 + 2.0 * (2560 * 320 + 320 * 1280 + 320 * 320),
            _hip.lib().dc_ff_geglu_proj_fused320, _ptr(x), x.stride(0), _ptr(None if ln is None else ln[0]),
            _ptr(None if ln is None else ln[1]), ln_eps, _ptr(pw1.w), _ptr(pw1.bias), _ptr(w2p), _ptr(b2), _ptr(wp), _ptr(bp),
            _ptr(residual2), residual2.stride(0), _ptr(out), out.stride(0), M, stream_ptr())
    return out


def ln_linear(x, pw, out, ln=None, ln_eps=1e-5):
    """out = Linear(LayerNorm(x) if ln else x) for dim 320 / 640 in one launch; pw = PackedWeight.linear (N % 32 == 0);
    ln = (gamma, beta) fp32 or None."""
    _rows(x, "x"); _rows(out, "out")
    M, K = x.shape[0], pw.K
    if K not in (320, 640) or pw.N % 32:
        raise ValueError("ln_linear: K must be 320 or 640 and N a multiple of 32")
    _need_rows(x, M, K, "x"); _need_rows(out, M, pw.N, "out")
    if ln is not None:
        _need(ln[0], K, "ln gamma"); _need(ln[1], K, "ln beta")
    _launch("ln_linear", 2.0 * M * pw.N * K, 2.0 * M * (K + pw.N) + 2.0 * pw.N * K, _hip.lib().dc_ln_linear,
            _ptr(x), x.stride(0), K, _ptr(None if ln is None else ln[0]), _ptr(None if ln is None else ln[1]), ln_eps,
            _ptr(pw.w), _ptr(pw.bias), _ptr(out), out.stride(0), M, pw.N, stream_ptr())
    return out


def linear_residual(x, pw, residual, out):
    """out = residual + Linear(x) for dim K = 320 / 640 in the X-stationary kernel (pw = PackedWeight.linear, N % 32 == 0);
    residual may be `out` itself."""
    _rows(x, "x"); _rows(out, "out"); _rows(residual, "residual")
    M, K = x.shape[0], pw.K
    if K not in (320, 640) or pw.N % 32:
        raise ValueError("linear_residual: K must be 320 or 640 and N a multiple of 32")
    _need_rows(x, M, K, "x"); _need_rows(out, M, pw.N, "out"); _need_rows(residual, M, pw.N, "residual")
    _launch("linear_residual", 2.0 * M * pw.N * K, 2.0 * M * (K + 2 * pw.N) + 2.0 * pw.N * K, _hip.lib().dc_linear_residual,
            _ptr(x), x.stride(0), K, _ptr(pw.w), _ptr(pw.bias), _ptr(residual), residual.stride(0), _ptr(out), out.stride(0),
            M, pw.N, stream_ptr())
    return out


def ln_qkv_temporal_attn(x, ln, pw_qkv, out, *, B, T, HW, scale, ln_eps=1e-5):
    """out = temporal self-attention (over the T = 16 frames of a position) of LayerNorm(x), q/k/v projected in the same
    launch; dim 320 = 5 heads x 64 or 640 = 10 heads x 64; rows ordered (clip, frame, position)."""
    _rows(x, "x"); _rows(out, "out")
    M = B * T * HW
    Cc = pw_qkv.K
    if Cc not in (320, 640) or pw_qkv.N != 3 * Cc or pw_qkv.bias is not None or T != 16 or HW % 8:
        raise ValueError("ln_qkv_temporal_attn: dim 320 / 640 (qkv weight [3 C, C], no bias), T = 16, HW % 8 == 0")
    if x.data_ptr() == out.data_ptr():
        raise ValueError("ln_qkv_temporal_attn: out must not alias x")
    _need_rows(x, M, Cc, "x"); _need_rows(out, M, Cc, "out"); _need(ln[0], Cc, "ln gamma"); _need(ln[1], Cc, "ln beta")
    fn = _hip.lib().dc_ln_qkv_temporal_attn320 if Cc == 320 else _hip.lib().dc_ln_qkv_temporal_attn640
    _launch(f"ln_qkv_temporal_attn{Cc}", 2.0 * M * 3 * Cc * Cc + 4.0 * M * T * Cc, 4.0 * M * Cc + 2.0 * 3 * Cc * Cc,
            fn, _ptr(x), x.stride(0), _ptr(ln[0]), _ptr(ln[1]), ln_eps, _ptr(pw_qkv.w),
            _ptr(out), out.stride(0), B, T, HW, scale, stream_ptr())
    return out


def gn_silu_tconv3(x, gamma, beta, stats, pw, out, *, B, T, HW, groups=32, residual=None):
    """out = tconv3(silu(GroupNorm(x))) (+ residual) for 320 / 640 input channels, statistics from groupnorm_stats over the
    clips (n_inst = B, rows_per_inst = T * HW); pw = PackedWeight.tconv3; rows ordered (clip, frame, position)."""
    _rows(x, "x"); _rows(out, "out")
    M = B * T * HW
    C = pw.w.shape[1] // 3
    if C not in (320, 640) or pw.w.shape[1] != 3 * C or pw.N % 32 or pw.bias is None or T != 16 or HW % 8:
        raise ValueError("gn_silu_tconv3: 320 / 640 input channels (weight [N, 3 C] with bias), N % 32 == 0, T = 16, HW % 8 == 0")
    if x.data_ptr() == out.data_ptr():
        raise ValueError("gn_silu_tconv3: out must not alias x")
    _need_rows(x, M, C, "x"); _need_rows(out, M, pw.N, "out")
    _need(gamma, C, "gamma"); _need(beta, C, "beta"); _need(stats, B * groups * 2, "stats")
    if residual is not None:
        _rows(residual, "residual"); _need_rows(residual, M, pw.N, "residual")
    _launch("gn_silu_tconv3", 2.0 * M * pw.N * 3 * C, 2.0 * M * (C + pw.N * (2 if residual is not None else 1)) + 2.0 * pw.N * 3 * C,
            _hip.lib().dc_gn_silu_tconv3, _ptr(x), x.stride(0), C, _ptr(gamma), _ptr(beta), _ptr(stats), groups, _ptr(pw.w),
            _ptr(pw.bias), _ptr(residual), 0 if residual is None else residual.stride(0), _ptr(out), out.stride(0), B, T, HW,
            pw.N, stream_ptr())
    return out


def groupnorm_stats(x, stats, *, groups, n_inst, rows_per_inst, eps):
    """(mean, rstd) per (instance, group) of channels-last rows -> stats fp32 [n_inst, groups, 2] (for gn_linear320)."""
    _rows(x, "x")
    Cc = x.shape[1]
    _need_rows(x, n_inst * rows_per_inst, Cc, "x"); _need(stats, n_inst * groups * 2, "stats")
    l = _hip.lib()
    ws = _gn_workspace(x.device, int(l.dc_groupnorm_workspace_bytes(n_inst, groups, rows_per_inst)))
    _launch("groupnorm_stats(2 kernels)", 0.0, 2.0 * n_inst * rows_per_inst * Cc, l.dc_groupnorm_stats, _ptr(x), x.stride(0),
            Cc, groups, n_inst, rows_per_inst, eps, _ptr(ws), _ptr(stats), stream_ptr())
    return stats


def gn_linear(x, gamma, beta, stats, pw, out, *, groups, rows_per_inst):
    """out = Linear(GroupNorm(x)) for dim 320 / 640 with the statistics of groupnorm_stats, normalisation applied in
    registers."""
    _rows(x, "x"); _rows(out, "out")
    M, K = x.shape[0], pw.K
    if K not in (320, 640) or pw.N % 32 or rows_per_inst % 128 or M % rows_per_inst:
        raise ValueError("gn_linear: K in (320, 640), N % 32 == 0, rows_per_inst % 128 == 0, M % rows_per_inst == 0")
    _need_rows(x, M, K, "x"); _need_rows(out, M, pw.N, "out")
    _need(gamma, K, "gamma"); _need(beta, K, "beta"); _need(stats, (M // rows_per_inst) * groups * 2, "stats")
    _launch("gn_linear", 2.0 * M * pw.N * K, 2.0 * M * (K + pw.N) + 2.0 * pw.N * K, _hip.lib().dc_gn_linear,
            _ptr(x), x.stride(0), K, _ptr(gamma), _ptr(beta), _ptr(stats), groups, rows_per_inst, _ptr(pw.w), _ptr(pw.bias),
            _ptr(out), out.stride(0), M, pw.N, stream_ptr())
    return out


def attn_small(q, k, v, o, *, batch, heads, Lq, Lk, d, scale, causal=False):
    """Any-head-width attention (CLIP towers): q/o rows [batch*Lq, >= heads*d], k/v rows [batch*Lk, >= heads*d]."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
        _rows(t, n)
    _need_rows(q, batch * Lq, heads * d, "q"); _need_rows(o, batch * Lq, heads * d, "o")
    _need_rows(k, batch * Lk, heads * d, "k"); _need_rows(v, batch * Lk, heads * d, "v")
    _launch("attn_small", 4.0 * batch * heads * Lq * Lk * d, 2.0 * batch * heads * d * (2 * Lq + 2 * Lk),
            _hip.lib().dc_attn_small, _ptr(q), _ptr(k), _ptr(v), _ptr(o), q.stride(0), k.stride(0), v.stride(0), o.stride(0),
            batch, heads, Lq, Lk, d, scale, 1 if causal else 0, stream_ptr())
    return o


def clip_preprocess(img, out_hw=(224, 224), antialias=True, mean=(0.48145466, 0.4578275, 0.40821073),
                    std=(0.26862954, 0.26130258, 0.27577711)):
    """img fp32 [N,3,H,W] in [-1,1] -> fp32 [N,3,OH,OW] (bicubic align_corners resize w/ antialias blur, CLIP mean/std)."""
    img = img.to(torch.float32).contiguous()
    N, Cc, H, W = img.shape
    out = torch.empty((N, Cc, out_hw[0], out_hw[1]), dtype=torch.float32, device=img.device)
    blur = antialias and max(H / out_hw[0], W / out_hw[1]) > 1.0
    t0 = torch.empty_like(img) if blur else None
    t1 = torch.empty_like(img) if blur else None
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(_hip.lib().dc_clip_preprocess(_ptr(img), _ptr(t0), _ptr(t1), _ptr(out), N, Cc, H, W, out_hw[0], out_hw[1],
                                        1 if antialias else 0, m3, s3, stream_ptr()), "dc_clip_preprocess")
    return out


def patchify(img, rows, *, patch):
    N, Cc, H, W = img.shape
    _need_rows(rows, N * (H // patch) * (W // patch), Cc * patch * patch, "rows")
    check(_hip.lib().dc_patchify(_ptr(img), _ptr(rows), N, Cc, H, W, patch, rows.stride(0), stream_ptr()), "dc_patchify")
    return rows


def embed_tokens(tokens, table, pos, out):
    B, L = tokens.shape
    D = table.shape[1]
    _need_rows(out, B * L, D, "out"); _need_rows(pos, L, D, "pos")
    if out.stride(0) != D or table.stride(0) != D or pos.stride(0) != D:
        raise ValueError("embed_tokens: dense rows expected")
    check(_hip.lib().dc_embed_tokens(_ptr(tokens), _ptr(table), _ptr(pos), _ptr(out), B, L, D, table.shape[0], stream_ptr()),
          "dc_embed_tokens")
    return out


def gemv_small(x, pw, out, *, act_in=0, act_out=0, accumulate=False):
    """x [M, K] fp32, out [M, N] fp32; the kernel takes M <= 8 rows, more rows (the clips of a windowed UNet call) go in
    launches of 8."""
    if x.shape[1] < pw.K or out.shape[0] < x.shape[0] or out.shape[1] < pw.N:
        raise ValueError(f"gemv_small: x {tuple(x.shape)}, weight [{pw.N}, {pw.K}], out {tuple(out.shape)}")
    for r in range(0, x.shape[0], 8):
        xs, os_ = x[r:r + 8], out[r:r + 8]
        check(_hip.lib().dc_gemv_small(_ptr(xs), x.stride(0), _ptr(pw.w), _ptr(pw.bias), _ptr(os_), out.stride(0),
                                       xs.shape[0], pw.N, pw.K, act_in, act_out, 1 if accumulate else 0, stream_ptr()),
              "dc_gemv_small")
    return out


def timestep_embedding(t_table, out, dim, *, t_index=None, t_stride=0, max_period=10000.0):
    if out.shape[1] < dim or t_table.numel() < out.shape[0]:
        raise ValueError(f"timestep_embedding: out {tuple(out.shape)}, dim {dim}, table of {t_table.numel()} entries")
    check(_hip.lib().dc_timestep_embedding(_ptr(t_table), _ptr(t_index), t_stride, _ptr(out), out.shape[0], dim,
                                           max_period, stream_ptr()), "dc_timestep_embedding")
    return out


def pack_latent(x, cc, out, *, B, Cx, Cc, T, HW, nrep=1):
    _need(x, B * Cx * T * HW, "x"); _need(cc, B * Cc * T * HW, "c_concat"); _need_rows(out, nrep * B * T * HW, Cx + Cc, "out")
    check(_hip.lib().dc_pack_latent(_ptr(x), _ptr(cc), _ptr(out), B, Cx, Cc, T, HW, out.stride(0), nrep,
                                    stream_ptr()), "dc_pack_latent")
    return out


def window_tables(starts, wn, *, T_long, T, device):
    """The device tables of a window plan (samplers/windows.py): starts int32 [S, W], wn fp32 [S, W, T]. The C entries
    cannot look into device memory, so the values are checked here, on the host copy, before upload: every start in
    [0, T_long - T], weights finite, >= 0 and summing to 1 on every frame of every step."""
    import numpy as np
    from .lvdm.models.samplers.windows import check_plan
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    wn = np.ascontiguousarray(wn, dtype=np.float32)
    S, W = check_plan(starts, wn, T_long, T)
    return dict(starts=torch.from_numpy(starts).to(device), wn=torch.from_numpy(wn).to(device), S=S, W=W, T=int(T),
                T_long=int(T_long), host_starts=starts, host_wn=wn)


def _need_windows(plan, w0, n_w, index, step_index):
    S, W, T = plan["S"], plan["W"], plan["T"]
    if w0 < 0 or n_w < 1 or w0 + n_w > W:
        raise ValueError(f"windows {w0} .. {w0 + n_w - 1} are not all in the plan's {W}")
    if step_index is None and not 0 <= index < S:
        raise ValueError(f"step {index} is outside the plan's {S} steps")
    for t, dt, n, nm in ((plan["starts"], torch.int32, S * W, "starts"), (plan["wn"], torch.float32, S * W * T, "wn")):
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"window plan: {nm} must be a contiguous CUDA {dt} tensor")
        _need(t, n, nm)
    return S, W, T


def pack_latent_windows(x, cc, out, plan, *, B, Cx, Cc, HW, w0=0, n_w=None, index=0, step_index=None, nrep=1):
    """pack_latent for the windows w0 .. w0 + n_w - 1 of the current step of `plan` (window_tables): rows
    [(rep, b, w, f, p)][c_pad] (dc_pack_latent_windows). x, cc: fp32 [B, C, T_long, HW]."""
    n_w = plan["W"] - w0 if n_w is None else n_w
    S, W, T = _need_windows(plan, w0, n_w, index, step_index)
    TL = plan["T_long"]
    _need(x, B * Cx * TL * HW, "x"); _need(cc, B * Cc * TL * HW, "c_concat")
    _rows(out, "out"); _need_rows(out, nrep * B * n_w * T * HW, Cx + Cc, "out")
    check(_hip.lib().dc_pack_latent_windows(_ptr(x), _ptr(cc), _ptr(out), _ptr(plan["starts"]), _ptr(step_index), index,
                                            S, W, w0, n_w, B, Cx, Cc, TL, T, HW, out.stride(0), nrep, stream_ptr()),
          "dc_pack_latent_windows")
    return out


def window_merge(e, out, plan, *, nb, B, C, HW, w0=0, n_w=None, index=0, step_index=None, accumulate=False):
    """out rows [(k, b, F, p)][ld_out] = the weighted blend of the window rows e [(k, b, w, f, p)][ld_e] of the windows
    w0 .. w0 + n_w - 1 (dc_window_merge); accumulate adds to `out` (chunked evaluation, ascending chunks)."""
    n_w = plan["W"] - w0 if n_w is None else n_w
    S, W, T = _need_windows(plan, w0, n_w, index, step_index)
    _rows(e, "e", torch.float32); _rows(out, "out", torch.float32)
    _need_rows(e, nb * B * n_w * T * HW, C, "e"); _need_rows(out, nb * B * plan["T_long"] * HW, C, "out")
    check(_hip.lib().dc_window_merge(_ptr(e), e.stride(0), _ptr(out), out.stride(0), _ptr(plan["starts"]),
                                     _ptr(plan["wn"]), _ptr(step_index), index, S, W, w0, n_w, nb, B, C, plan["T_long"],
                                     T, HW, 1 if accumulate else 0, stream_ptr()), "dc_window_merge")
    return out


def tile_tables(box, g, *, long_shape, box_shape, device):
    """The device tables of a tile plan (samplers/tiles.py): box int32 [S, W, 3], g fp32 [S, W, T + h + w]. The C entries
    cannot look into device memory, so the values are checked here, on the host copy, before upload (check_tiles): every
    start in range, weights finite, >= 0 and summing to 1 on every position of every step."""
    import numpy as np
    from .lvdm.models.samplers.tiles import check_tiles
    box = np.ascontiguousarray(box, dtype=np.int32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    long_shape, box_shape = tuple(int(v) for v in long_shape), tuple(int(v) for v in box_shape)
    S, W = check_tiles(box, g, long_shape, box_shape)
    return dict(box=torch.from_numpy(box).to(device), g=torch.from_numpy(g).to(device), S=S, W=W, long_shape=long_shape,
                box_shape=box_shape, host_box=box, host_g=g)


def _need_tiles(plan, w0, n_w, index, step_index):
    S, W = plan["S"], plan["W"]
    if w0 < 0 or n_w < 1 or w0 + n_w > W:
        raise ValueError(f"boxes {w0} .. {w0 + n_w - 1} are not all in the plan's {W}")
    if step_index is None and not 0 <= index < S:
        raise ValueError(f"step {index} is outside the plan's {S} steps")
    for t, dt, n, nm in ((plan["box"], torch.int32, S * W * 3, "box"),
                         (plan["g"], torch.float32, S * W * sum(plan["box_shape"]), "g")):
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"tile plan: {nm} must be a contiguous CUDA {dt} tensor")
        _need(t, n, nm)
    return S, W


def pack_latent_tiles(x, cc, out, plan, *, B, Cx, Cc, w0=0, n_w=None, index=0, step_index=None, nrep=1):
    """pack_latent for the boxes w0 .. w0 + n_w - 1 of the current step of `plan` (tile_tables): rows
    [(rep, b, w, f, y, x)][c_pad] (dc_pack_latent_tiles). x, cc: fp32 [B, C, T_long, H_long, W_long]."""
    n_w = plan["W"] - w0 if n_w is None else n_w
    S, W = _need_tiles(plan, w0, n_w, index, step_index)
    (TL, HL, WL), (T, H, Wd) = plan["long_shape"], plan["box_shape"]
    _need(x, B * Cx * TL * HL * WL, "x"); _need(cc, B * Cc * TL * HL * WL, "c_concat")
    _rows(out, "out"); _need_rows(out, nrep * B * n_w * T * H * Wd, Cx + Cc, "out")
    check(_hip.lib().dc_pack_latent_tiles(_ptr(x), _ptr(cc), _ptr(out), _ptr(plan["box"]), _ptr(step_index), index, S, W,
                                          w0, n_w, B, Cx, Cc, TL, HL, WL, T, H, Wd, out.stride(0), nrep, stream_ptr()),
          "dc_pack_latent_tiles")
    return out


def tile_merge(e, out, plan, *, nb, B, C, w0=0, n_w=None, index=0, step_index=None, accumulate=False):
    """out rows [(k, b, F, Y, X)][ld_out] = the weighted blend of the box rows e [(k, b, w, f, y, x)][ld_e] of the boxes
    w0 .. w0 + n_w - 1 (dc_tile_merge); accumulate adds to `out` (chunked evaluation, ascending chunks)."""
    n_w = plan["W"] - w0 if n_w is None else n_w
    S, W = _need_tiles(plan, w0, n_w, index, step_index)
    (TL, HL, WL), (T, H, Wd) = plan["long_shape"], plan["box_shape"]
    _rows(e, "e", torch.float32); _rows(out, "out", torch.float32)
    _need_rows(e, nb * B * n_w * T * H * Wd, C, "e"); _need_rows(out, nb * B * TL * HL * WL, C, "out")
    check(_hip.lib().dc_tile_merge(_ptr(e), e.stride(0), _ptr(out), out.stride(0), _ptr(plan["box"]), _ptr(plan["g"]),
                                   _ptr(step_index), index, S, W, w0, n_w, nb, B, C, TL, HL, WL, T, H, Wd,
                                   1 if accumulate else 0, stream_ptr()), "dc_tile_merge")
    return out


def nchw_to_rows(x, out, *, N, Cc, HW, scale=1.0):
    _need(x, N * Cc * HW, "x"); _need_rows(out, N * HW, Cc, "out")
    check(_hip.lib().dc_nchw_to_rows(_ptr(x), _ptr(out), N, Cc, HW, out.stride(0), scale, stream_ptr()),
          "dc_nchw_to_rows")
    return out


def rows_to_nchw(rows, y, *, N, Cc, HW, scale=1.0):
    _need_rows(rows, N * HW, Cc, "rows"); _need(y, N * Cc * HW, "y")
    check(_hip.lib().dc_rows_to_nchw(_ptr(rows), rows.stride(0), 1 if rows.dtype == torch.float32 else 0, _ptr(y),
                                     N, Cc, HW, scale, stream_ptr()), "dc_rows_to_nchw")
    return y


def im2col3x3_c8(x, out, *, n_img, H, W):
    """rows [n_img*H*W, >= 8] (first 8 channels) -> rows [n_img*H*W, 128]: 9 taps x 8 channels + zeros (dc_im2col3x3_c8)."""
    _rows(x, "x"); _rows(out, "out")
    M = n_img * H * W
    _need_rows(x, M, 8, "x"); _need_rows(out, M, 128, "out")
    _launch("im2col3x3_c8", 0.0, 2.0 * M * (16 + 256), _hip.lib().dc_im2col3x3_c8, _ptr(x), x.stride(0), _ptr(out), out.stride(0),
            n_img, H, W, stream_ptr())
    return out


def copy2d(src, dst, cols=None):
    _rows(src, "src"); _rows(dst, "dst")
    cols = src.shape[1] if cols is None else cols
    _launch("copy2d", 0.0, 4.0 * src.shape[0] * cols, _hip.lib().dc_copy2d, _ptr(src), src.stride(0), _ptr(dst),
            dst.stride(0), src.shape[0], cols, stream_ptr())
    return dst


def transpose(src, dst, rows=None, cols=None):
    """dst[c, r] = src[r, c] (bf16)."""
    rows = src.shape[0] if rows is None else rows
    cols = src.shape[1] if cols is None else cols
    check(_hip.lib().dc_transpose(_ptr(src), src.stride(0), _ptr(dst), dst.stride(0), rows, cols, stream_ptr()),
          "dc_transpose")
    return dst


def add_rows(a, b, y):
    check(_hip.lib().dc_add_rows(_ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(y), y.stride(0), a.shape[0],
                                 a.shape[1], stream_ptr()), "dc_add_rows")
    return y


def freeu_scratch_floats(*, cs, F, H, W, version=1):
    """fp32 elements of freeu's `scratch`: the seven sums per (frame, skip channel), as partial sums over up to 8 slices of
    a large plane; version 2 adds the row means of h and a (min, max) pair per frame. Its contents need no initialisation."""
    n = int(_hip.lib().dc_freeu_scratch_floats(cs, F, H, W, version))
    if n < 0:
        raise ValueError(f"freeu_scratch_floats: bad arguments cs={cs} F={F} H={H} W={W} version={version}")
    return n


def freeu(cat, *, ch, cs, F, H, W, b, s, version=1, scratch):
    """FreeU in place on cat = [h | skip] (bf16 rows [F*H*W, ch + cs], rows ordered frame, y, x; a column slice of a wider
    buffer is fine): the skip columns get fourier_filter(x, threshold=1, scale=s) per (frame, channel) plane, the first ch/2
    columns of h are scaled by b (version 1) or by (b-1)*mhat + 1 (version 2: mhat = the row mean of h over all ch columns,
    min-max normalised per frame; 0 for a frame whose mean is flat, where the published code divides by zero). Columns
    ch/2..ch-1 are not touched. 2 launches (version 2: 3), no atomics: bit-reproducible and graph-capturable.
    scratch: fp32, freeu_scratch_floats(...) elements, from the caller's arena."""
    _rows(cat, "cat")
    if version not in (1, 2):
        raise ValueError(f"freeu: version must be 1 or 2, got {version!r}")
    if cs < 64 or cs % 64 or ch < 128 or ch % 128:
        raise ValueError(f"freeu: needs cs % 64 == 0 and ch % 128 == 0, got ch={ch} cs={cs}")
    if min(F, H, W) < 1 or cat.shape[0] != F * H * W or cat.shape[1] != ch + cs:
        raise ValueError(f"freeu: cat is {tuple(cat.shape)}, expected [F*H*W, ch+cs] = [{F * H * W}, {ch + cs}]")
    if cat.stride(0) % 8 or cat.data_ptr() % 16:
        raise ValueError(f"freeu: cat needs a row stride that is a multiple of 8 and a 16-byte aligned start, got stride "
                         f"{cat.stride(0)}, address % 16 = {cat.data_ptr() % 16}")
    if not (math.isfinite(b) and math.isfinite(s)):
        raise ValueError(f"freeu: b and s must be finite, got b={b} s={s}")
    if scratch.dtype != torch.float32 or not scratch.is_cuda or not scratch.is_contiguous():
        raise ValueError("freeu: scratch must be a contiguous CUDA float32 tensor")
    _need(scratch, freeu_scratch_floats(cs=cs, F=F, H=H, W=W, version=version), "scratch")
    l = _hip.lib()
    rows, ld = F * H * W, cat.stride(0)
    geo = (_ptr(cat), ld, ch, cs, F, H, W)
    n_stats = freeu_scratch_floats(cs=cs, F=F, H=H, W=W, version=1)
    stats = C.c_void_p(scratch.data_ptr())
    hmean = mm = C.c_void_p(0)
    tag = f"F{F} {H}x{W} ch{ch} cs{cs}"             # per-shape rows of a Tracer's detail table (tools/freeu_ab.py)
    if version == 2:
        hmean = C.c_void_p(scratch.data_ptr() + 4 * n_stats)
        mm = C.c_void_p(scratch.data_ptr() + 4 * (n_stats + rows))
        _launch("freeu_hmean", 0.0, 2.0 * rows * ch + 4.0 * rows, l.dc_freeu_hmean, *geo, hmean, stream_ptr(), tag=tag)
    _launch("freeu_skip_stats", 0.0, 2.0 * rows * cs + 4.0 * n_stats, l.dc_freeu_skip_stats, *geo, stats, hmean, mm, stream_ptr(),
            tag=tag)
    _launch("freeu_apply", 0.0, 4.0 * rows * (cs + ch // 2), l.dc_freeu_apply, *geo, stats, float(b), float(s), hmean, mm,
            stream_ptr(), tag=tag)
    return cat


def build_context(ctx, out, *, B, T, n_text, L, D):
    _need(ctx, B * (n_text + T * L) * D, "context"); _need(out, B * T * (n_text + L) * D, "out")
    check(_hip.lib().dc_build_context(_ptr(ctx), _ptr(out), B, T, n_text, L, D, stream_ptr()), "dc_build_context")
    return out


def softmax_rows(x, y):
    check(_hip.lib().dc_softmax_rows(_ptr(x), x.stride(0), _ptr(y), y.stride(0), x.shape[0], x.shape[1],
                                     stream_ptr()), "dc_softmax_rows")
    return y


def vae_sample(moments, noise, z, *, N, zc, HW, scale):
    _need_rows(moments, N * HW, 2 * zc, "moments"); _need(noise, N * zc * HW, "noise"); _need(z, N * zc * HW, "z")
    check(_hip.lib().dc_vae_sample(_ptr(moments), moments.stride(0), _ptr(noise), _ptr(z), N, zc, HW, scale,
                                   stream_ptr()), "dc_vae_sample")
    return z


STEP_WS_FLOATS = 16 * 256     # per clip: what dc_ddim_step / dc_dpmpp_step / dc_sds_step carve their partial sums out of
                              # (include/dcrafter_hip.h documents it, csrc/elementwise.hip static_asserts its largest layout)


def step_workspace(B, device):
    """The `workspace` operand of ddim_step / dpmpp_step / sds_step for B clips (scratch, no initialisation)."""
    return torch.empty(STEP_WS_FLOATS * B, dtype=torch.float32, device=device)


def _step_params(p, tables, fields, e_cond, index, step_index, v_param, cfg_scale, cfg_img, guidance_rescale,
                 temperature, e_nchw, ld_e, noise_step_stride):
    """Fill what DcDdimParams and DcDpmParams have in common (fields: struct field -> key of `tables`); returns ld_e."""
    for f, k in fields.items():
        t = tables.get(k)
        setattr(p, f, 0 if t is None else t.data_ptr())
    p.step_index = 0 if step_index is None else step_index.data_ptr()
    p.index, p.v_param = index, 1 if v_param else 0
    p.cfg_scale, p.cfg_img, p.guidance_rescale, p.temperature = cfg_scale, cfg_img, guidance_rescale, temperature
    p.e_nchw, p.noise_step_stride = 1 if e_nchw else 0, noise_step_stride
    if ld_e is None:
        ld_e = 0 if e_nchw else e_cond.stride(0)
    return ld_e


def _need_step(latents, workspace, e_rows, *, B, Cc, THW, e_nchw, ld_e, noise=None, steps=1, noise_step_stride=0):
    """Extent checks of a step launch: `latents` ((tensor, name) pairs of B*Cc*THW elements), the workspace, the e_*
    operands in their layout and the noise of the `steps` addressable steps."""
    n = B * Cc * THW
    for t, nm in latents:
        _need(t, n, nm)
    _need(workspace, STEP_WS_FLOATS * B, "workspace")
    for t, nm in e_rows:
        _need(t, n if e_nchw else (B * THW - 1) * ld_e + Cc, nm)
    _need(noise, (steps - 1) * noise_step_stride + n, "noise")


_DDIM_FIELDS = {k: k for k in ("a_t", "a_prev", "sigma_t", "sqrt_one_minus_at", "sqrt_acp_t", "sqrt_1macp_t", "scale_ratio")}
_DPM_FIELDS = {**{k: "dpm_" + k for k in ("A", "alpha_t", "alpha_p_r", "k", "N")},
               **{k: k for k in ("sqrt_one_minus_at", "sqrt_acp_t", "sqrt_1macp_t", "scale_ratio")}}


def ddim_step(tables, e_cond, e_uncond, e_img, x, noise, x_prev, pred_x0, workspace, *, B, Cc, THW, index=0,
              step_index=None, v_param=False, cfg_scale=1.0, cfg_img=1.0, guidance_rescale=0.0, temperature=1.0,
              e_nchw=False, ld_e=None, noise_step_stride=0):
    """tables: dict of fp32 device vectors (a_t, a_prev, sigma_t, sqrt_one_minus_at[, sqrt_acp_t, sqrt_1macp_t,
    scale_ratio]) indexed by the DDIM index."""
    p = DcDdimParams()
    ld_e = _step_params(p, tables, _DDIM_FIELDS, e_cond, index, step_index, v_param, cfg_scale, cfg_img,
                        guidance_rescale, temperature, e_nchw, ld_e, noise_step_stride)
    # with a device step counter the kernel reads noise[step * noise_step_stride + i], step < the number of table rows
    _need_step(((x, "x"), (x_prev, "x_prev"), (pred_x0, "pred_x0")), workspace,
               ((e_cond, "e_cond"), (e_uncond, "e_uncond"), (e_img, "e_img")), B=B, Cc=Cc, THW=THW, e_nchw=e_nchw,
               ld_e=ld_e, noise=noise, steps=1 if step_index is None else int(tables["a_t"].numel()),
               noise_step_stride=noise_step_stride)
    check(_hip.lib().dc_ddim_step(C.byref(p), _ptr(e_cond), _ptr(e_uncond), _ptr(e_img), ld_e, _ptr(x),
                                  _ptr(noise), _ptr(x_prev), _ptr(pred_x0), B, Cc, THW, _ptr(workspace),
                                  stream_ptr()), "dc_ddim_step")
    return x_prev, pred_x0


_INVERT_FIELDS = {"sqrt_a_src": "inv_sqrt_a_src", "sqrt_1ma_src": "inv_sqrt_1ma_src", "sqrt_a_dst": "inv_sqrt_a_dst",
                  "sqrt_1ma_dst": "inv_sqrt_1ma_dst", "scale_ratio": "inv_scale_ratio"}


def ddim_invert_step(tables, e_cond, e_uncond, e_img, x, x_next, pred_x0, workspace, *, B, Cc, THW, index=0,
                     step_index=None, v_param=False, cfg_scale=1.0, cfg_img=1.0, guidance_rescale=0.0, e_nchw=False,
                     ld_e=None):
    """One DDIM inversion step (dc_ddim_invert_step): x at level ddim_alphas_prev[k] -> x_next at ddim_alphas[k], k the
    step. tables: dict of fp32 device vectors in ascending k - inv_sqrt_a_src, inv_sqrt_1ma_src, inv_sqrt_a_dst,
    inv_sqrt_1ma_dst [, inv_scale_ratio] (DDIMSampler.make_schedule). x and x_next may be the same tensor."""
    p = _hip.DcInvertParams()
    steps = None
    for f, k in _INVERT_FIELDS.items():
        t = tables.get(k)
        if t is None:
            if f != "scale_ratio":
                raise ValueError(f"ddim_invert_step: table {k} is missing")
        else:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"ddim_invert_step: table {k} must be contiguous fp32")
            if steps is not None and t.numel() != steps:
                raise ValueError(f"ddim_invert_step: table {k} has {t.numel()} entries, the others {steps}")
            steps = t.numel()
        setattr(p, f, 0 if t is None else t.data_ptr())
    if step_index is None and not 0 <= index < steps:
        raise ValueError(f"ddim_invert_step: step {index} is outside the tables' {steps} steps")
    if e_img is not None and e_uncond is None:
        raise ValueError("ddim_invert_step: e_img needs e_uncond")
    if ld_e is None:
        ld_e = 0 if e_nchw else e_cond.stride(0)
    if not e_nchw and ld_e < Cc:
        raise ValueError(f"ddim_invert_step: ld_e = {ld_e} is below the {Cc} channels")
    p.step_index = 0 if step_index is None else step_index.data_ptr()
    p.index, p.v_param, p.e_nchw = index, 1 if v_param else 0, 1 if e_nchw else 0
    p.cfg_scale, p.cfg_img, p.guidance_rescale = cfg_scale, cfg_img, guidance_rescale
    _need_step(((x, "x"), (x_next, "x_next"), (pred_x0, "pred_x0")), workspace,
               ((e_cond, "e_cond"), (e_uncond, "e_uncond"), (e_img, "e_img")), B=B, Cc=Cc, THW=THW, e_nchw=e_nchw, ld_e=ld_e)
    check(_hip.lib().dc_ddim_invert_step(C.byref(p), _ptr(e_cond), _ptr(e_uncond), _ptr(e_img), ld_e, _ptr(x),
                                         _ptr(x_next), _ptr(pred_x0), B, Cc, THW, _ptr(workspace), stream_ptr()),
          "dc_ddim_invert_step")
    return x_next, pred_x0


def dpmpp_step(tables, e_cond, e_uncond, e_img, x, noise, x_prev, pred_x0, workspace, x0_hist, *, B, Cc, THW, index=0,
               step_index=None, v_param=False, cfg_scale=1.0, cfg_img=1.0, guidance_rescale=0.0, temperature=1.0,
               e_nchw=False, ld_e=None, noise_step_stride=0):
    """One DPM-Solver++ (2M / 2M SDE) update (dc_dpmpp_step). tables: dict of fp32 device vectors in execution order -
    the solver's dpm_A, dpm_alpha_t, dpm_alpha_p_r, dpm_k [, dpm_N] and the DDIM sampler's sqrt_one_minus_at /
    sqrt_acp_t / sqrt_1macp_t [/ scale_ratio]. x0_hist: [2, B*C*THW] fp32 ring of raw data predictions."""
    p = _hip.DcDpmParams()
    ld_e = _step_params(p, tables, _DPM_FIELDS, e_cond, index, step_index, v_param, cfg_scale, cfg_img,
                        guidance_rescale, temperature, e_nchw, ld_e, noise_step_stride)
    p.x0_hist = x0_hist.data_ptr()
    _need(x0_hist, 2 * B * Cc * THW, "x0_hist")
    _need_step(((x, "x"), (x_prev, "x_prev"), (pred_x0, "pred_x0")), workspace,
               ((e_cond, "e_cond"), (e_uncond, "e_uncond"), (e_img, "e_img")), B=B, Cc=Cc, THW=THW, e_nchw=e_nchw,
               ld_e=ld_e, noise=noise, steps=1 if step_index is None else int(tables["dpm_A"].numel()),
               noise_step_stride=noise_step_stride)
    check(_hip.lib().dc_dpmpp_step(C.byref(p), _ptr(e_cond), _ptr(e_uncond), _ptr(e_img), ld_e, _ptr(x), _ptr(noise),
                                   _ptr(x_prev), _ptr(pred_x0), B, Cc, THW, _ptr(workspace), stream_ptr()),
          "dc_dpmpp_step")
    return x_prev, pred_x0


APG_SPACES = ("x0", "model")


def apg_workspace_floats(*, B, Cc, THW):
    """fp32 elements of apg_guide's `workspace` for B clips of Cc x THW elements: three partial sums per workgroup of the
    reduction (min(256, ceil(THW / 256)) workgroups per clip). Its contents need no initialisation."""
    n = int(_hip.lib().dc_apg_workspace_floats(B, Cc, THW))
    if n < 0:
        raise ValueError(f"apg_workspace_floats: bad arguments B={B} Cc={Cc} THW={THW}")
    return n


def apg_guide(tables, e_cond, e_uncond, x, momentum_buf, out, workspace, *, B, Cc, THW, cfg_scale, eta, norm_threshold,
              momentum, space, v_param, index=0, step_index=None, e_nchw=False, ld_e=None):
    """Adaptive projected guidance (dc_apg_reduce + dc_apg_apply) in place of the CFG combine: `out` = the guided model
    output, which ddim_step / dpmpp_step then take as e_cond with e_uncond=None and cfg_scale=1. e_cond, e_uncond and out:
    fp32 rows [B*THW, ld] (out may have a row stride of its own) or [B, Cc, THW] under e_nchw; x and momentum_buf: fp32
    [B, Cc, THW]. momentum_buf is the running update m, changed in place: zero it ahead of the first step of a run (with
    momentum == 0 it is only written). space "x0" projects in the space of the denoised prediction (tables: sqrt_acp_t and
    sqrt_1macp_t for v models, a_t and sqrt_one_minus_at for eps models, indexed by the step), "model" on the raw outputs.
    norm_threshold None or <= 0: no clipping. workspace: apg_workspace_floats(...) fp32 elements."""
    if space not in APG_SPACES:
        raise ValueError(f"apg_guide: space must be one of {APG_SPACES}, got {space!r}")
    for nm, v in (("cfg_scale", cfg_scale), ("eta", eta), ("momentum", momentum),
                  ("norm_threshold", 0.0 if norm_threshold is None else norm_threshold)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"apg_guide: {nm} must be a finite number, got {v!r}")
    if e_uncond is None:
        raise ValueError("apg_guide: needs e_uncond (guidance with two branches)")
    n = B * Cc * THW
    if min(B, Cc, THW) < 1 or B > 65535:
        raise ValueError(f"apg_guide: bad shape B={B} Cc={Cc} THW={THW} (1 <= B <= 65535)")
    if ld_e is None:
        ld_e = 0 if e_nchw else e_cond.stride(0)
    ld_out = 0 if e_nchw else (out.stride(0) if out.dim() == 2 else Cc)
    if not e_nchw and (ld_e < Cc or ld_out < Cc):
        raise ValueError(f"apg_guide: row strides {ld_e} / {ld_out} are below the {Cc} channels")
    for t, nm in ((e_cond, "e_cond"), (e_uncond, "e_uncond"), (x, "x"), (momentum_buf, "momentum_buf"), (out, "out"),
                  (workspace, "workspace")):
        if t is None:
            if nm == "x" and space == "model":
                continue
            raise ValueError(f"apg_guide: {nm} is missing")
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"apg_guide: {nm} must be a CUDA float32 tensor, got {t.dtype} on {t.device}")
    for t, nm in ((x, "x"), (momentum_buf, "momentum_buf"), (workspace, "workspace")):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"apg_guide: {nm} must be contiguous")
    _need(x, n, "x"); _need(momentum_buf, n, "momentum_buf")
    _need(workspace, apg_workspace_floats(B=B, Cc=Cc, THW=THW), "workspace")
    for t, nm in ((e_cond, "e_cond"), (e_uncond, "e_uncond")):
        _need(t, n if e_nchw else (B * THW - 1) * ld_e + Cc, nm)
    # out may be a column slice of a wider buffer: what counts is the storage behind its first element
    room = out.untyped_storage().nbytes() // 4 - out.storage_offset()
    if room < (n if e_nchw else (B * THW - 1) * ld_out + Cc):
        raise ValueError(f"out: {room} elements from its start, the launch writes {n if e_nchw else (B * THW - 1) * ld_out + Cc}")
    p = _hip.DcApgParams()
    x0 = space == "x0"
    need = (("sqrt_acp_t", "sqrt_1macp_t") if v_param else ("a_t", "sqrt_one_minus_at")) if x0 else ()
    for k in ("a_t", "sqrt_one_minus_at", "sqrt_acp_t", "sqrt_1macp_t"):
        t = tables.get(k) if k in need else None
        if k in need:
            if t is None or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"apg_guide: table {k} must be a contiguous fp32 vector (space='x0')")
            if step_index is None and not 0 <= index < t.numel():
                raise ValueError(f"apg_guide: step {index} is outside table {k}'s {t.numel()} steps")
        setattr(p, k, 0 if t is None else t.data_ptr())
    p.step_index = 0 if step_index is None else step_index.data_ptr()
    p.index, p.v_param, p.x0_space, p.e_nchw = index, 1 if v_param else 0, 1 if x0 else 0, 1 if e_nchw else 0
    p.cfg_scale, p.eta, p.momentum = cfg_scale, eta, momentum
    p.norm_threshold = 0.0 if norm_threshold is None else norm_threshold
    l = _hip.lib()
    xp = _ptr(x if x0 else None)
    _launch("apg_reduce", 3.0 * n, 4.0 * n * (5 if x0 else 4), l.dc_apg_reduce, C.byref(p), _ptr(e_cond), _ptr(e_uncond), ld_e,
            xp, _ptr(momentum_buf), B, Cc, THW, _ptr(workspace), stream_ptr())
    _launch("apg_apply", 3.0 * n, 4.0 * n * (4 if x0 else 3), l.dc_apg_apply, C.byref(p), _ptr(e_cond), ld_e, xp,
            _ptr(momentum_buf), _ptr(out), ld_out, B, Cc, THW, _ptr(workspace), stream_ptr())
    return out


SDS_WEIGHT_TYPES = ("t", "ada", "uniform")
SDS_X0_FORMULAS = ("reference", "parameterization")


def _sds_params(tables, B, step_index, index, noise_step_stride=0, weight_type="t", x0_formula="reference", e_nchw=False,
                cfg_scale=1.0, guidance_rescale=0.0, betas=(0.9, 0.999), eps=1e-8, decay=1.0, grad_scale=1.0, loss=None):
    if weight_type not in SDS_WEIGHT_TYPES:
        raise ValueError(f"weight_type must be one of {SDS_WEIGHT_TYPES}, got {weight_type!r}")
    if x0_formula not in SDS_X0_FORMULAS:
        raise ValueError(f"x0_formula must be one of {SDS_X0_FORMULAS}, got {x0_formula!r}")
    # the kernels read entry [k * B + b] of the per-clip tables and [k] of the per-step ones, k < steps
    steps = int(tables["step_size"].numel()) if step_index is not None else index + 1
    for k in ("c1", "c2", "w"):
        _need(tables.get(k), steps * B, k)
    for k in ("step_size", "bc2_sqrt"):
        _need(tables.get(k), steps, k)
    _need(loss, steps, "loss")
    p = _hip.DcSdsParams()
    for k in ("c1", "c2", "w", "step_size", "bc2_sqrt"):
        t = tables.get(k)
        setattr(p, k, 0 if t is None else t.data_ptr())
    p.step_index = 0 if step_index is None else step_index.data_ptr()
    p.index, p.weight_type = index, SDS_WEIGHT_TYPES.index(weight_type)
    p.x0_param, p.e_nchw = SDS_X0_FORMULAS.index(x0_formula), 1 if e_nchw else 0
    p.cfg_scale, p.guidance_rescale = cfg_scale, guidance_rescale
    p.beta2, p.eps = betas[1], eps
    p.one_minus_beta1, p.one_minus_beta2 = 1.0 - betas[0], 1.0 - betas[1]     # float64, then fp32: as torch.optim
    p.decay, p.grad_scale = decay, grad_scale
    p.noise_step_stride = noise_step_stride
    p.loss = 0 if loss is None else loss.data_ptr()
    return p


def sds_noise(tables, latent, noise, x_t, *, B, index=0, step_index=None, noise_step_stride=0):
    """x_t = c1 latent + c2 noise (dc_sds_noise) per clip; tables: fp32 device c1, c2 [S*B] (+ step_size [S] with a
    step counter). With step_index, step k's noise starts at noise + k * noise_step_stride."""
    n = latent.numel()
    _need(x_t, n, "x_t")
    if step_index is not None:
        _need(noise, (int(tables["step_size"].numel()) - 1) * noise_step_stride + n, "noise")
    else:
        _need(noise, n, "noise")
    p = _sds_params(tables, B, step_index, index, noise_step_stride)
    check(_hip.lib().dc_sds_noise(C.byref(p), _ptr(latent), _ptr(noise), _ptr(x_t), B, n // B, stream_ptr()),
          "dc_sds_noise")
    return x_t


def sds_step(tables, e_cond, e_uncond, x_t, latent, m, v, workspace, loss=None, *, B, Cc, THW, index=0, step_index=None,
             weight_type="t", x0_formula="reference", cfg_scale=1.0, guidance_rescale=0.0, betas=(0.9, 0.999), eps=1e-8,
             decay=1.0, grad_scale=None, e_nchw=False, ld_e=None):
    """One SDS gradient + Adam(W) step on `latent` in place (dc_sds_step). tables: fp32 device vectors c1, c2, w [S*B]
    and step_size, bc2_sqrt [S] (samplers/sds.py); m, v: the moments; loss: [S] fp32 or None. grad_scale defaults to
    1 / (B * numel(latent)), the gradient of 0.5 mse / B."""
    n = B * Cc * THW
    if ld_e is None:
        ld_e = 0 if e_nchw else e_cond.stride(0)
    _need_step(((x_t, "x_t"), (latent, "latent"), (m, "m"), (v, "v")), workspace,
               ((e_cond, "e_cond"), (e_uncond, "e_uncond")), B=B, Cc=Cc, THW=THW, e_nchw=e_nchw, ld_e=ld_e)
    if grad_scale is None:
        grad_scale = 1.0 / (B * n)
    p = _sds_params(tables, B, step_index, index, 0, weight_type, x0_formula, e_nchw, cfg_scale, guidance_rescale,
                    betas, eps, decay, grad_scale, loss)
    check(_hip.lib().dc_sds_step(C.byref(p), _ptr(e_cond), _ptr(e_uncond), ld_e, _ptr(x_t), _ptr(latent), _ptr(m),
                                 _ptr(v), B, Cc, THW, _ptr(workspace), stream_ptr()), "dc_sds_step")
    return latent


def mask_blend(img, x0, mask, qnoise, tables, *, index=0, step_index=None, clean=False, noise_step_stride=0):
    """img = orig*mask + (1-mask)*img in place, orig = x0 or its q_sample at the step's timestep (fp32, same shapes)."""
    n = img.numel()
    for t, nm in ((x0, "x0"), (mask, "mask")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"mask_blend: {nm} must be contiguous fp32 of the latent's shape")
    if img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError("mask_blend: latent must be contiguous fp32")
    if not clean:
        # with a device step counter the kernel reads qnoise[step * noise_step_stride + i], step < the number of table rows
        steps = int(tables["sqrt_acp_t"].numel()) if step_index is not None else 1
        _need(qnoise, (steps - 1) * noise_step_stride + n if step_index is not None else n, "qnoise")
    check(_hip.lib().dc_mask_blend(_ptr(img), _ptr(x0), _ptr(mask), _ptr(None if clean else qnoise),
                                   _ptr(tables.get("sqrt_acp_t")), _ptr(tables.get("sqrt_1macp_t")), _ptr(step_index), index,
                                   n, noise_step_stride, 1 if clean else 0, stream_ptr()), "dc_mask_blend")
    return img


def advance_counter(counter):
    check(_hip.lib().dc_advance_counter(_ptr(counter), stream_ptr()), "dc_advance_counter")


# ---------------------------------------------------------------------------------------------- baseline JPEG (csrc/jpeg.hip)
JPEG_MCU_MAX_BYTES = 2496                       # DC_JPEG_MCU_MAX_BYTES of include/dcrafter_hip.h


def _flat(t, dtype, name):
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous CUDA {dtype} tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def jpeg_mcu_grid(H, W):
    return (H + 15) // 16, (W + 15) // 16


def jpeg_dct_quant(frames, qtab, coef):
    """frames uint8 [T, H, W, 3], qtab uint8 [2, 64] (zigzag order) -> coef int16 [T, my, mx, 6, 64] (zigzag order)."""
    _flat(frames, torch.uint8, "frames"); _flat(qtab, torch.uint8, "qtab"); _flat(coef, torch.int16, "coef")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"jpeg_dct_quant: frames [T, H, W, 3] expected, got {tuple(frames.shape)}")
    T, H, W, _ = frames.shape
    my, mx = jpeg_mcu_grid(H, W)
    _need(qtab, 128, "qtab"); _need(coef, T * my * mx * 384, "coef")
    _launch("jpeg_dct_quant", 0.0, frames.numel() + 2.0 * T * my * mx * 384, _hip.lib().dc_jpeg_dct_quant, _ptr(frames),
            _ptr(qtab), _ptr(coef), T, H, W, stream_ptr())
    return coef


def jpeg_entropy(coef, scratch, seg_len, *, T, my, mx, ri, stride):
    """coef int16 [T, my, mx, 6, 64] -> scratch uint8 [n_seg, stride], seg_len int32 [n_seg]; n_seg = T ceil(my mx / ri)."""
    _flat(coef, torch.int16, "coef"); _flat(scratch, torch.uint8, "scratch"); _flat(seg_len, torch.int32, "seg_len")
    if min(T, my, mx, ri) < 1:
        raise ValueError(f"jpeg_entropy: T {T}, my {my}, mx {mx}, ri {ri}")
    n_seg = T * ((my * mx + ri - 1) // ri)
    if stride < min(ri, my * mx) * JPEG_MCU_MAX_BYTES + 1:
        raise ValueError(f"jpeg_entropy: stride {stride} below the worst case of {min(ri, my * mx)} MCUs")
    _need(coef, T * my * mx * 384, "coef"); _need(scratch, n_seg * stride, "scratch"); _need(seg_len, n_seg, "seg_len")
    _launch("jpeg_entropy", 0.0, 2.0 * T * my * mx * 384, _hip.lib().dc_jpeg_entropy, _ptr(coef), _ptr(scratch), _ptr(seg_len),
            T, my, mx, ri, stride, stream_ptr())
    return n_seg


def _check_pack(name, scratch, words, out, frame_len, *, T, rows, stride, frame_stride):
    """What the three pack wrappers share: uint8 scratch [T rows, stride] and out [T, frame_stride], int32 frame_len [T] and
    `words` (name -> int32 tensor with one element per scratch row: the lengths, the offsets), positive geometry, T within
    gridDim.y, and the extents the launch touches."""
    _flat(scratch, torch.uint8, "scratch"); _flat(out, torch.uint8, "out"); _flat(frame_len, torch.int32, "frame_len")
    if min(T, rows, stride, frame_stride) < 1 or T > 65535:
        raise ValueError(f"{name}: T {T}, {rows} scratch rows per frame, stride {stride}, frame_stride {frame_stride}")
    for k, t in words.items():
        _need(_flat(t, torch.int32, k), T * rows, k)
    _need(scratch, T * rows * stride, "scratch"); _need(out, T * frame_stride, "out"); _need(frame_len, T, "frame_len")


def jpeg_pack(scratch, seg_len, seg_off, out, frame_len, *, T, segs_per_frame, stride, frame_stride):
    """scratch [T segs_per_frame, stride] + seg_len -> out uint8 [T, frame_stride] (RSTm between a frame's segments),
    frame_len int32 [T]; seg_off int32 [T segs_per_frame] is workspace."""
    _check_pack("jpeg_pack", scratch, {"seg_len": seg_len, "seg_off": seg_off}, out, frame_len, T=T, rows=segs_per_frame,
                stride=stride, frame_stride=frame_stride)
    _launch("jpeg_pack(2 kernels)", 0.0, 0.0, _hip.lib().dc_jpeg_pack, _ptr(scratch), _ptr(seg_len), _ptr(seg_off), _ptr(out),
            _ptr(frame_len), T, segs_per_frame, stride, frame_stride, stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- JPEG decoding (csrc/jpeg_decode.hip)
JPEG_FRAME_TAB_BYTES = 1352                     # DC_JPEG_FRAME_TAB_BYTES of include/dcrafter_hip.h
JPEG_SEG_STATUS = {1: "a code that is in no table", 2: "a zero run past coefficient 63", 3: "a DC category above 11 or an AC "
                   "category above 10", 4: "bytes left over", 5: "bytes missing", 6: "a descriptor outside the batch"}


def jpeg_decode_geometry(H, W, ncomp, hs, vs):
    """(my, mx, blocks per MCU, bytes of one frame's padded sample planes) of a frame; ValueError for a sampling the decoder
    does not take."""
    if (ncomp, hs, vs) not in ((1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)):
        raise ValueError(f"jpeg_decode: {ncomp} components with luma sampling {hs}x{vs} (1 or 3 components; 1x1, 2x1 or 2x2)")
    my, mx = (H + 8 * vs - 1) // (8 * vs), (W + 8 * hs - 1) // (8 * hs)
    bpm = hs * vs + (2 if ncomp == 3 else 0)
    return my, mx, bpm, my * mx * 64 * bpm


def jpeg_decode_entropy(scan, seg, frame_seg, ftab, coef, status, *, T, my, mx, ncomp, hs, vs, max_segs_per_frame):
    """scan uint8 (the segments' bytes), seg int32 [n_seg, 5] (offset, length, first MCU, MCUs, frame), frame_seg int32 [T + 1],
    ftab uint8 [T, JPEG_FRAME_TAB_BYTES] -> coef int16 [T, my, mx, bpm, 64] (zigzag order), status int32 [n_seg]."""
    _flat(scan, torch.uint8, "scan"); _flat(ftab, torch.uint8, "ftab"); _flat(coef, torch.int16, "coef")
    for t, name in ((seg, "seg"), (frame_seg, "frame_seg"), (status, "status")):
        _flat(t, torch.int32, name)
    bpm = jpeg_decode_geometry(8 * vs * my, 8 * hs * mx, ncomp, hs, vs)[2]
    n_seg = seg.numel() // 5
    if min(T, my, mx, n_seg, max_segs_per_frame, scan.numel()) < 1 or seg.numel() != 5 * n_seg:
        raise ValueError(f"jpeg_decode_entropy: T {T}, my {my}, mx {mx}, {seg.numel()} descriptor words, {scan.numel()} bytes")
    _need(frame_seg, T + 1, "frame_seg"); _need(ftab, T * JPEG_FRAME_TAB_BYTES, "ftab"); _need(status, n_seg, "status")
    _need(coef, T * my * mx * bpm * 64, "coef")
    _launch("jpeg_decode_entropy", 0.0, scan.numel() + 2.0 * T * my * mx * bpm * 64, _hip.lib().dc_jpeg_decode_entropy, _ptr(scan),
            scan.numel(), _ptr(seg), _ptr(frame_seg), _ptr(ftab), _ptr(coef), _ptr(status), n_seg, T, my, mx, ncomp, hs, vs,
            max_segs_per_frame, stream_ptr())
    return coef


def jpeg_decode_idct(coef, ftab, planes, *, T, my, mx, ncomp, hs, vs):
    """coef int16 [T, my, mx, bpm, 64] -> planes uint8, per frame Y [my 8 vs, mx 8 hs] then Cb, Cr [my 8, mx 8]."""
    _flat(coef, torch.int16, "coef"); _flat(ftab, torch.uint8, "ftab"); _flat(planes, torch.uint8, "planes")
    n = jpeg_decode_geometry(8 * vs * my, 8 * hs * mx, ncomp, hs, vs)[3]
    if min(T, my, mx) < 1:
        raise ValueError(f"jpeg_decode_idct: T {T}, my {my}, mx {mx}")
    _need(coef, T * n, "coef"); _need(ftab, T * JPEG_FRAME_TAB_BYTES, "ftab"); _need(planes, T * n, "planes")
    _launch("jpeg_decode_idct", 32.0 * T * n, 3.0 * T * n, _hip.lib().dc_jpeg_decode_idct, _ptr(coef), _ptr(ftab), _ptr(planes), T,
            my, mx, ncomp, hs, vs, stream_ptr())
    return planes


def jpeg_decode_output(planes, out, *, T, H, W, ncomp, hs, vs):
    """planes -> out: uint8 [T, H, W, 3], or fp32 [T, 3, H, W] holding the same integers (chosen by out's dtype)."""
    _flat(planes, torch.uint8, "planes")
    if out.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"jpeg_decode_output: out must be uint8 [T, H, W, 3] or fp32 [T, 3, H, W], got {out.dtype}")
    _flat(out, out.dtype, "out")
    if min(T, H, W) < 1 or max(H, W) > 65535:
        raise ValueError(f"jpeg_decode_output: T {T}, H {H}, W {W}")
    n = jpeg_decode_geometry(H, W, ncomp, hs, vs)[3]
    _need(planes, T * n, "planes"); _need(out, T * H * W * 3, "out")
    _launch("jpeg_decode_output", 0.0, T * n + T * H * W * 3.0 * out.element_size(), _hip.lib().dc_jpeg_decode_output, _ptr(planes),
            _ptr(out), T, H, W, ncomp, hs, vs, 1 if out.dtype == torch.float32 else 0, stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- animated GIF (csrc/gif.hip)
GIF_HIST_BINS = 32768                           # DC_GIF_HIST_BINS of include/dcrafter_hip.h
GIF_CLEAR_INTERVAL = 3838                       # DC_GIF_CLEAR_INTERVAL: data codes in front of a Clear inside a chunk
GIF_CHUNK = 8192                                # pixels per independently coded chunk (utils/save_video.py's default)


def gif_chunk_max_bytes(n):
    """DC_GIF_CHUNK_MAX_BYTES(n): the worst-case code string of a chunk of n pixels, in whole 32-bit words. n data codes, n // 3838
    Clears inside the chunk and one terminator, 12 bits each."""
    return (12 * (n + n // GIF_CLEAR_INTERVAL + 1) + 31) // 32 * 4


def gif_frame_max_bytes(hw, chunk):
    """The worst-case image data of one frame as dc_gif_pack writes it: the leading Clear and every chunk's worst case, in
    sub-blocks of 255 bytes with their length bytes, and the closing 00."""
    full, rest = divmod(hw, chunk)
    bits = 9 + full * 12 * (chunk + chunk // GIF_CLEAR_INTERVAL + 1) + (12 * (rest + rest // GIF_CLEAR_INTERVAL + 1) if rest else 0)
    nbytes = (bits + 7) // 8
    return nbytes + (nbytes + 254) // 255 + 1


def gif_histogram(frames, hist):
    """frames uint8 [T, H, W, 3] -> hist uint32-as-int32 [32768]: pixels per bin (r>>3)<<10 | (g>>3)<<5 | (b>>3). The launch
    clears hist itself."""
    _flat(frames, torch.uint8, "frames"); _flat(hist, torch.int32, "hist")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"gif_histogram: frames [T, H, W, 3] expected, got {tuple(frames.shape)}")
    T, H, W, _ = frames.shape
    if min(T, H, W) < 1 or T * H * W > 0xFFFFFFFF:
        raise ValueError(f"gif_histogram: frames of {H} x {W} x {T}")
    _need(hist, GIF_HIST_BINS, "hist")
    _launch("gif_histogram(2 kernels)", 0.0, float(frames.numel()), _hip.lib().dc_gif_histogram, _ptr(frames), _ptr(hist), T, H, W,
            stream_ptr())
    return hist


def gif_map(frames, palette, idx, *, n, dither=0):
    """frames uint8 [T, H, W, 3] + palette uint8 [>= n, 3] -> idx uint8 [T, H, W]: ordered dither of amplitude `dither` (0..64),
    then the nearest of the first n palette entries (ties to the lowest index)."""
    _flat(frames, torch.uint8, "frames"); _flat(palette, torch.uint8, "palette"); _flat(idx, torch.uint8, "idx")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"gif_map: frames [T, H, W, 3] expected, got {tuple(frames.shape)}")
    T, H, W, _ = frames.shape
    if min(T, H, W) < 1 or not 1 <= n <= 256 or not 0 <= dither <= 64:
        raise ValueError(f"gif_map: frames of {H} x {W} x {T}, n {n}, dither {dither}")
    _need(palette, 3 * n, "palette"); _need(idx, T * H * W, "idx")
    _launch("gif_map", 8.0 * n * T * H * W, 4.0 * T * H * W, _hip.lib().dc_gif_map, _ptr(frames), _ptr(palette), _ptr(idx), T, H, W,
            int(n), int(dither), stream_ptr())
    return idx


def gif_lzw(idx, scratch, chunk_bits, *, T, hw, chunk, stride):
    """idx uint8 [T, hw] -> scratch uint8 [n_chunks, stride], chunk_bits int32 [n_chunks] (lengths in bits);
    n_chunks = T ceil(hw / chunk)."""
    _flat(idx, torch.uint8, "idx"); _flat(scratch, torch.uint8, "scratch"); _flat(chunk_bits, torch.int32, "chunk_bits")
    if min(T, hw, chunk) < 1:
        raise ValueError(f"gif_lzw: T {T}, hw {hw}, chunk {chunk}")
    n_chunks = T * ((hw + chunk - 1) // chunk)
    if stride % 4 or stride < gif_chunk_max_bytes(min(chunk, hw)):
        raise ValueError(f"gif_lzw: stride {stride} is no multiple of 4 or below the worst case of {min(chunk, hw)} pixels")
    if scratch.data_ptr() % 4:
        raise ValueError("gif_lzw: scratch must be 4-byte aligned")
    _need(idx, T * hw, "idx"); _need(scratch, n_chunks * stride, "scratch"); _need(chunk_bits, n_chunks, "chunk_bits")
    _launch("gif_lzw", 0.0, float(T * hw), _hip.lib().dc_gif_lzw, _ptr(idx), _ptr(scratch), _ptr(chunk_bits), T, hw, chunk, stride,
            stream_ptr())
    return n_chunks


def gif_pack(scratch, chunk_bits, chunk_off, out, frame_len, *, T, chunks_per_frame, stride, frame_stride):
    """scratch [T chunks_per_frame, stride] + chunk_bits -> out uint8 [T, frame_stride] (a frame's sub-blocked image data behind a
    leading Clear), frame_len int32 [T]; chunk_off int32 [T chunks_per_frame] is workspace."""
    _check_pack("gif_pack", scratch, {"chunk_bits": chunk_bits, "chunk_off": chunk_off}, out, frame_len, T=T,
                rows=chunks_per_frame, stride=stride, frame_stride=frame_stride)
    if 9 + chunks_per_frame * stride * 8 > 0x7FFFFFFF:
        raise ValueError(f"gif_pack: {chunks_per_frame} chunks of {stride} bytes pass 2^31 bits in a frame")
    _launch("gif_pack(2 kernels)", 0.0, 0.0, _hip.lib().dc_gif_pack, _ptr(scratch), _ptr(chunk_bits), _ptr(chunk_off), _ptr(out),
            _ptr(frame_len), T, chunks_per_frame, stride, frame_stride, stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- PNG / APNG (csrc/png.hip)
PNG_CHUNK = 16384                               # DC_PNG_CHUNK: bytes of a frame's scanlines per independently coded chunk
PNG_CHUNK_LIMIT = 65535                         # DC_PNG_CHUNK_LIMIT: LEN of a stored block is 16 bits


def png_chunk_max_bytes(n):
    """DC_PNG_CHUNK_MAX_BYTES(n): the worst-case string of a chunk of n bytes (the stored form, n + 5), in whole 32-bit words."""
    return (n + 5 + 3) // 4 * 4


def png_frame_max_bytes(N, chunk):
    """DC_PNG_FRAME_MAX_BYTES(N, chunk): 78 01, every chunk of a plane of N bytes in the stored form, Adler-32."""
    return 6 + N + 5 * ((N + chunk - 1) // chunk)


def png_filter(frames, planes):
    """frames uint8 [T, H, W, C] (C in 1, 3, 4) -> planes uint8 [T, H, 1 + W C]: per row the filter type 0..4 with the least sum of
    min(r, 256 - r) over its residuals (the lowest type on a tie) and the residuals."""
    _flat(frames, torch.uint8, "frames"); _flat(planes, torch.uint8, "planes")
    if frames.dim() != 4 or frames.shape[3] not in (1, 3, 4):
        raise ValueError(f"png_filter: frames [T, H, W, 1|3|4] expected, got {tuple(frames.shape)}")
    T, H, W, Cc = frames.shape
    if min(T, H, W) < 1 or H * (1 + W * Cc) > 0x7FFFFFFF:
        raise ValueError(f"png_filter: frames of {H} x {W} x {Cc} x {T}")
    _need(planes, T * H * (1 + W * Cc), "planes")
    _launch("png_filter", 0.0, 2.0 * frames.numel(), _hip.lib().dc_png_filter, _ptr(frames), _ptr(planes), T, H, W, Cc, stream_ptr())
    return planes


def png_deflate(planes, scratch, chunk_len, chunk_adler, *, T, N, chunk, stride):
    """planes uint8 [T, N] -> scratch uint8 [n_chunks, stride], chunk_len int32 [n_chunks] (bytes), chunk_adler int32 [n_chunks]
    (the Adler-32 of the chunk alone, as a bit pattern); n_chunks = T ceil(N / chunk)."""
    _flat(planes, torch.uint8, "planes"); _flat(scratch, torch.uint8, "scratch")
    _flat(chunk_len, torch.int32, "chunk_len"); _flat(chunk_adler, torch.int32, "chunk_adler")
    if min(T, N, chunk) < 1 or chunk > PNG_CHUNK_LIMIT or N > 0x7FFFFFFF:
        raise ValueError(f"png_deflate: T {T}, N {N}, chunk {chunk}")
    n_chunks = T * ((N + chunk - 1) // chunk)
    if stride % 4 or stride < png_chunk_max_bytes(min(chunk, N)):
        raise ValueError(f"png_deflate: stride {stride} is no multiple of 4 or below the worst case of {min(chunk, N)} bytes")
    if scratch.data_ptr() % 4:
        raise ValueError("png_deflate: scratch must be 4-byte aligned")
    _need(planes, T * N, "planes"); _need(scratch, n_chunks * stride, "scratch")
    _need(chunk_len, n_chunks, "chunk_len"); _need(chunk_adler, n_chunks, "chunk_adler")
    _launch("png_deflate", 0.0, float(T * N), _hip.lib().dc_png_deflate, _ptr(planes), _ptr(scratch), _ptr(chunk_len),
            _ptr(chunk_adler), T, N, chunk, stride, stream_ptr())
    return n_chunks


def png_pack(scratch, chunk_len, chunk_adler, chunk_off, out, frame_len, *, T, N, chunk, stride, frame_stride):
    """scratch [T ceil(N / chunk), stride] + chunk_len + chunk_adler -> out uint8 [T, frame_stride] (one zlib stream per frame),
    frame_len int32 [T]; chunk_off int32 [T ceil(N / chunk)] is workspace."""
    if min(N, chunk) < 1 or chunk > PNG_CHUNK_LIMIT:
        raise ValueError(f"png_pack: N {N}, chunk {chunk}")
    cpf = (N + chunk - 1) // chunk
    _check_pack("png_pack", scratch, {"chunk_len": chunk_len, "chunk_adler": chunk_adler, "chunk_off": chunk_off}, out, frame_len,
                T=T, rows=cpf, stride=stride, frame_stride=frame_stride)
    if 6 + cpf * stride > 0x7FFFFFFF:
        raise ValueError(f"png_pack: {cpf} chunks of {stride} bytes pass 2^31 in a frame")
    _launch("png_pack(2 kernels)", 0.0, 0.0, _hip.lib().dc_png_pack, _ptr(scratch), _ptr(chunk_len), _ptr(chunk_adler), _ptr(chunk_off),
            _ptr(out), _ptr(frame_len), T, N, chunk, stride, frame_stride, stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- image -> clip (csrc/preprocess.hip)
RESIZE_PRECISION_BITS = 22                      # Pillow's PRECISION_BITS for 8-bit channels (32 - 8 - 2)


def resize_coeffs(n_in, n_out):
    """Pillow's BILINEAR resampling tables of one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc), on the host in
    float64 with Pillow's operation order: k int32 [n_out, ksize], xmin int32 [n_out], n int32 [n_out] (numpy). The weights of
    an output are summed tap by tap as Pillow sums them (numpy's pairwise sum would round differently)."""
    import numpy as np
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_coeffs: {n_in} -> {n_out}")
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                                   # the triangle filter's support is 1
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # the cast truncates, as C's (int) does
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = xmax - xmin
    w = np.zeros((n_out, ksize), dtype=np.float64)
    ww = np.zeros(n_out, dtype=np.float64)
    for x in range(ksize):
        a = np.abs((x + xmin - center + 0.5) * ss)
        w[:, x] = np.where((a < 1.0) & (x < n), 1.0 - a, 0.0)
        ww += w[:, x]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = (0.5 + w * float(1 << RESIZE_PRECISION_BITS)).astype(np.int32)          # weights are >= 0: truncation = C's (int)
    k[np.arange(ksize)[None, :] >= n[:, None]] = 0
    return k, xmin.astype(np.int32), n.astype(np.int32)


class ResizeTables:
    """Device copy of resize_coeffs(n_in, n_out) plus the host bounds the launch wrappers plan and check with. The kernels
    trust the tables (include/dcrafter_hip.h), so this is where xmin + n <= n_in and n <= ksize are guaranteed."""

    __slots__ = ("n_in", "n_out", "ksize", "k", "xmin", "n", "host_xmin", "host_n")

    def __init__(self, n_in, n_out, device):
        k, xmin, n = resize_coeffs(n_in, n_out)
        if (xmin < 0).any() or (n < 0).any() or (n > k.shape[1]).any() or (xmin.astype("int64") + n > n_in).any():
            raise AssertionError(f"resize tables {n_in} -> {n_out}: a window leaves the input")
        self.n_in, self.n_out, self.ksize = int(n_in), int(n_out), int(k.shape[1])
        self.host_xmin, self.host_n = xmin, n
        self.k, self.xmin, self.n = (torch.from_numpy(a).to(device) for a in (k, xmin, n))

    def span(self, lo, hi):
        """(first, count) of the inputs that the outputs lo .. hi - 1 read."""
        first = int(self.host_xmin[lo:hi].min())
        return first, int((self.host_xmin[lo:hi] + self.host_n[lo:hi]).max()) - first


def _image_u8(t, name):
    _flat(t, torch.uint8, name)
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name}: uint8 [H, W, 3] expected, got {tuple(t.shape)}")
    return t.shape[0], t.shape[1]


def prep_resize_h(src, tmp, tab, *, y0, rows, x0, cols):
    """Horizontal pass of src uint8 [H, W, 3] into tmp uint8 [rows, cols, 3] (workspace of the caller): source rows
    y0 .. y0 + rows - 1, resized columns x0 .. x0 + cols - 1 (dc_prep_resize_h)."""
    H, W = _image_u8(src, "src")
    _flat(tmp, torch.uint8, "tmp")
    if tab.n_in != W or tab.k.device != src.device or tmp.device != src.device:
        raise ValueError(f"prep_resize_h: tables for width {tab.n_in} on {tab.k.device}, source width {W} on {src.device}")
    if rows < 1 or cols < 1 or y0 < 0 or y0 + rows > H or x0 < 0 or x0 + cols > tab.n_out:
        raise ValueError(f"prep_resize_h: rows {y0}+{rows} of {H}, columns {x0}+{cols} of {tab.n_out}")
    _need(tmp, rows * cols * 3, "tmp")
    _launch("prep_resize_h", 0.0, 3.0 * (rows * W + rows * cols), _hip.lib().dc_prep_resize_h, _ptr(src), _ptr(tmp), _ptr(tab.k),
            _ptr(tab.xmin), _ptr(tab.n), tab.ksize, H, W, tab.n_out, y0, rows, x0, cols, stream_ptr())
    return tmp


def prep_finish(src, clip, tab, *, axis, src_hw, origin, resized, offset, t0, nt):
    """The last pass (axis 0: none, 1: horizontal, 2: vertical; `tab` = its ResizeTables or None) + crop / padding / ToTensor /
    Normalize into frames t0 .. t0 + nt - 1 of clip fp32 [3, T, ch, cw] (dc_prep_finish). src: uint8, `src_hw` pixels of 3
    bytes whose first is pixel `origin` = (y, x) of its image; `resized` = (rh, rw); crop pixel (oy, ox) is the resized pixel
    (oy + offset[0], ox + offset[1])."""
    _flat(src, torch.uint8, "src"); _flat(clip, torch.float32, "clip")
    if clip.dim() != 4 or clip.shape[0] != 3 or clip.device != src.device:
        raise ValueError(f"prep_finish: clip fp32 [3, T, ch, cw] on {src.device} expected, got {tuple(clip.shape)} on {clip.device}")
    _, T, ch, cw = clip.shape
    (sh, sw), (sy0, sx0), (rh, rw), (yoff, xoff) = src_hw, origin, resized, offset
    _need(src, sh * sw * 3, "src")
    if nt < 1 or t0 < 0 or t0 + nt > T:
        raise ValueError(f"prep_finish: frames {t0} .. {t0 + nt - 1} of {T}")
    if axis not in (0, 1, 2) or (tab is None) != (axis == 0):
        raise ValueError(f"prep_finish: axis {axis} with{'out' if tab is None else ''} tables")
    ry0, ry1, rx0, rx1 = max(yoff, 0), min(ch + yoff, rh), max(xoff, 0), min(cw + xoff, rw)
    if tab is not None:
        if tab.k.device != src.device or tab.n_out != (rw if axis == 1 else rh):
            raise ValueError(f"prep_finish: tables {tab.n_in} -> {tab.n_out} on {tab.k.device} for a resized image of {rh} x {rw}")
        # the windows of every output the crop keeps lie inside src (the kernel trusts this)
        lo, hi, s0, sn = (rx0, rx1, sx0, sw) if axis == 1 else (ry0, ry1, sy0, sh)
        if lo < hi:
            first, count = tab.span(lo, hi)
            if first < s0 or first + count > s0 + sn:
                raise ValueError(f"prep_finish: the pass reads inputs {first} .. {first + count - 1}, src holds {s0} .. {s0 + sn - 1}")
    z = C.c_void_p(0)
    _launch("prep_finish", 0.0, 3.0 * sh * sw + 12.0 * nt * ch * cw, _hip.lib().dc_prep_finish, _ptr(src), _ptr(clip),
            z if tab is None else _ptr(tab.k), z if tab is None else _ptr(tab.xmin), z if tab is None else _ptr(tab.n),
            0 if tab is None else tab.ksize, axis, sh, sw, sy0, sx0, rh, rw, yoff, xoff, ch, cw, T, t0, nt, stream_ptr())
    return clip


# ---------------------------------------------------------------------------------------------- float image resize (csrc/preprocess.hip)
def resize_coeffs_f32(n_in, n_out, antialias):
    """Bilinear resampling tables of one axis for fp32 images, on the host in float32 with ATen's operation order
    (UpSampleKernel.cpp): k fp32 [n_out, ksize], xmin int32 [n_out], n int32 [n_out] (numpy). scale = n_in / n_out.
    antialias=True: the window rule of _compute_indices_min_size_weights_aa with the triangle filter; the support is `scale` on a
    downscale and 1 otherwise, the weights are summed tap by tap and normalised to sum 1.
    antialias=False: interpolate's two taps (area_pixel_compute_source_index, guard_index_and_lambda): src = fma(scale, i + 0.5,
    -0.5) clamped at 0, i0 = min(floor(src), n_in - 1), lambda = src - i0, weights (1 - lambda, lambda); at the right border,
    where both taps are the last pixel, one tap of weight 1. The window rule with support 1 describes the same two taps, but
    rounds the position at another place than ATen does, which shows from a few hundred pixels on (2^-24 * n_in in a weight)."""
    import numpy as np
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_coeffs_f32: {n_in} -> {n_out}")
    f = np.float32
    scale = f(n_in) / f(n_out)
    if not antialias:
        # one rounding, as ATen's builds contract the expression into a fused multiply-add (the float64 product is exact)
        src = np.maximum((np.float64(scale) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(f), f(0.0))
        i0 = np.minimum(src.astype(np.int64), n_in - 1)                        # src >= 0: truncation = floor
        lam = np.minimum(np.maximum(src - i0.astype(f), f(0.0)), f(1.0))
        two = i0 + 1 <= n_in - 1
        w = np.zeros((n_out, 2), dtype=f)
        w[:, 0] = np.where(two, f(1.0) - lam, f(1.0))
        w[:, 1] = np.where(two, lam, f(0.0))
        return w, i0.astype(np.int32), np.where(two, 2, 1).astype(np.int32)
    aa = scale >= 1.0
    support = scale if aa else f(1.0)
    invscale = f(1.0) / scale if aa else f(1.0)
    ksize = int(math.ceil(float(support))) * 2 + 1
    center = scale * (np.arange(n_out, dtype=f) + f(0.5))
    xmin = np.maximum((center - support + f(0.5)).astype(np.int64), 0)         # the cast truncates, as C's (int) does
    xmax = np.minimum((center + support + f(0.5)).astype(np.int64), n_in)
    n = xmax - xmin
    w = np.zeros((n_out, ksize), dtype=f)
    total = np.zeros(n_out, dtype=f)
    for j in range(ksize):
        a = np.abs((f(j) + xmin.astype(f) - center + f(0.5)) * invscale)
        w[:, j] = np.where(j < n, np.maximum(f(0.0), f(1.0) - a), f(0.0))
        total += w[:, j]
    w = np.where((total != 0)[:, None], w / np.where(total != 0, total, f(1.0))[:, None], w).astype(f)
    return w, xmin.astype(np.int32), n.astype(np.int32)


class ResizeTablesF32:
    """Device copy of resize_coeffs_f32(n_in, n_out, antialias) plus the host bounds the launch wrappers plan and check with
    (the kernels trust the tables, as with ResizeTables)."""

    __slots__ = ("n_in", "n_out", "antialias", "ksize", "k", "xmin", "n", "host_xmin", "host_n")

    def __init__(self, n_in, n_out, antialias, device):
        k, xmin, n = resize_coeffs_f32(n_in, n_out, antialias)
        if (xmin < 0).any() or (n < 1).any() or (n > k.shape[1]).any() or (xmin.astype("int64") + n > n_in).any():
            raise AssertionError(f"resize tables {n_in} -> {n_out}: a window leaves the input")
        if (xmin[1:] < xmin[:-1]).any() or ((xmin + n)[1:] < (xmin + n)[:-1]).any():
            raise AssertionError(f"resize tables {n_in} -> {n_out}: the windows do not advance with the output")
        self.n_in, self.n_out, self.antialias, self.ksize = int(n_in), int(n_out), bool(antialias), int(k.shape[1])
        self.host_xmin, self.host_n = xmin, n
        self.k, self.xmin, self.n = (torch.from_numpy(a).to(device) for a in (k, xmin, n))

    span = ResizeTables.span


def _planes_f32(t, name):
    _flat(t, torch.float32, name)
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{name}: fp32 [C, H, W] expected, got {tuple(t.shape)}")
    return tuple(t.shape)


RESIZE_F32_TILE, RESIZE_F32_LDS_MAX = 256, 65536       # DC_RESIZE_F32_TILE, DC_RESIZE_F32_LDS_MAX (include/dcrafter_hip.h)


def resize_f32_h_seg(tab, x0, cols):
    """The `seg` argument of dc_resize_f32_h for the resized columns x0 .. x0 + cols - 1: the most source columns a tile of
    RESIZE_F32_TILE outputs spans, or 0 (the direct form) when that and the tile's weights exceed RESIZE_F32_LDS_MAX bytes."""
    import numpy as np
    first = np.arange(x0, x0 + cols, RESIZE_F32_TILE)
    last = np.minimum(first + RESIZE_F32_TILE - 1, x0 + cols - 1)
    seg = int((tab.host_xmin[last].astype(np.int64) + tab.host_n[last] - tab.host_xmin[first]).max())
    return seg if 4 * (seg + RESIZE_F32_TILE * tab.ksize) <= RESIZE_F32_LDS_MAX else 0


def resize_f32_h(src, tmp, tab, *, y0, rows, x0, cols, staged=None):
    """Horizontal pass of src fp32 [C, H, W] into tmp fp32 [C, rows, cols] (workspace of the caller): source rows
    y0 .. y0 + rows - 1, resized columns x0 .. x0 + cols - 1 (dc_resize_f32_h). `staged`: through the LDS (True), straight from
    global memory (False), or (None) through the LDS whenever a tile's source segment and weights fit it; the same bits."""
    Cn, H, W = _planes_f32(src, "src")
    _flat(tmp, torch.float32, "tmp")
    if tab.n_in != W or tab.k.device != src.device or tmp.device != src.device:
        raise ValueError(f"resize_f32_h: tables for width {tab.n_in} on {tab.k.device}, source width {W} on {src.device}")
    if rows < 1 or cols < 1 or y0 < 0 or y0 + rows > H or x0 < 0 or x0 + cols > tab.n_out:
        raise ValueError(f"resize_f32_h: rows {y0}+{rows} of {H}, columns {x0}+{cols} of {tab.n_out}")
    _need(tmp, Cn * rows * cols, "tmp")
    seg = resize_f32_h_seg(tab, x0, cols)
    fits = seg > 0
    if staged and not fits:
        raise ValueError(f"resize_f32_h: a tile's source segment and its {tab.ksize}-tap weights are more than the LDS form takes")
    if staged is False or not fits:
        seg = 0
    _launch("resize_f32_h", 0.0, 4.0 * Cn * (rows * W + rows * cols), _hip.lib().dc_resize_f32_h, _ptr(src), _ptr(tmp),
            _ptr(tab.k), _ptr(tab.xmin), _ptr(tab.n), tab.ksize, Cn, H, W, tab.n_out, y0, rows, x0, cols, seg, stream_ptr())
    return tmp


def resize_f32_finish(src, out, tab, *, axis, src_hw, origin, resized, offset):
    """The last pass (axis 0: none, 1: horizontal, 2: vertical; `tab` = its ResizeTablesF32 or None) + crop / 0.0 padding into
    out fp32 [C, ch, cw] (dc_resize_f32_finish). src: fp32, C planes of `src_hw` pixels whose first is pixel `origin` = (y, x) of
    its image; `resized` = (rh, rw); pixel (oy, ox) of out is the resized pixel (oy + offset[0], ox + offset[1])."""
    _flat(src, torch.float32, "src")
    Cn, ch, cw = _planes_f32(out, "out")
    if out.device != src.device:
        raise ValueError(f"resize_f32_finish: out on {out.device}, src on {src.device}")
    (sh, sw), (sy0, sx0), (rh, rw), (yoff, xoff) = src_hw, origin, resized, offset
    if min(sh, sw, rh, rw) < 1 or sy0 < 0 or sx0 < 0:
        raise ValueError(f"resize_f32_finish: src {sh} x {sw} at {sy0}, {sx0}, resized {rh} x {rw}")
    _need(src, Cn * sh * sw, "src")
    if axis not in (0, 1, 2) or (tab is None) != (axis == 0):
        raise ValueError(f"resize_f32_finish: axis {axis} with{'out' if tab is None else ''} tables")
    ry0, ry1, rx0, rx1 = max(yoff, 0), min(ch + yoff, rh), max(xoff, 0), min(cw + xoff, rw)
    if ry0 < ry1 and rx0 < rx1:
        # along the axis it is addressed directly, src holds every resized pixel the crop keeps (the entry checks this too)
        if (axis != 2 and (ry0 < sy0 or ry1 > sy0 + sh)) or (axis != 1 and (rx0 < sx0 or rx1 > sx0 + sw)):
            raise ValueError(f"resize_f32_finish: the crop keeps rows {ry0} .. {ry1 - 1}, columns {rx0} .. {rx1 - 1}; src holds "
                             f"{sh} x {sw} from ({sy0}, {sx0})")
    if tab is not None:
        if tab.k.device != src.device or tab.n_out != (rw if axis == 1 else rh):
            raise ValueError(f"resize_f32_finish: tables {tab.n_in} -> {tab.n_out} on {tab.k.device} for a resized image of "
                             f"{rh} x {rw}")
        lo, hi, s0, sn = (rx0, rx1, sx0, sw) if axis == 1 else (ry0, ry1, sy0, sh)
        if lo < hi:                             # the windows of every output the crop keeps lie inside src (the kernel trusts this)
            first, count = tab.span(lo, hi)
            if first < s0 or first + count > s0 + sn:
                raise ValueError(f"resize_f32_finish: the pass reads inputs {first} .. {first + count - 1}, src holds {s0} .. "
                                 f"{s0 + sn - 1}")
    z = C.c_void_p(0)
    _launch("resize_f32_finish", 0.0, 4.0 * Cn * (sh * sw + ch * cw), _hip.lib().dc_resize_f32_finish, _ptr(src), _ptr(out),
            z if tab is None else _ptr(tab.k), z if tab is None else _ptr(tab.xmin), z if tab is None else _ptr(tab.n),
            0 if tab is None else tab.ksize, axis, Cn, sh, sw, sy0, sx0, rh, rw, yoff, xoff, ch, cw, stream_ptr())
    return out


_RESIZE_TABLES_F32 = {}


def _resize_tables_f32(n_in, n_out, antialias, device):
    """Cached ResizeTablesF32 (an application resizes to one resolution; the last 16 are kept)."""
    key = (int(n_in), int(n_out), bool(antialias), str(device))
    tab = _RESIZE_TABLES_F32.pop(key, None)
    if tab is None:
        tab = ResizeTablesF32(n_in, n_out, antialias, device)
    _RESIZE_TABLES_F32[key] = tab
    while len(_RESIZE_TABLES_F32) > 16:
        _RESIZE_TABLES_F32.pop(next(iter(_RESIZE_TABLES_F32)))
    return tab


def resize_f32(img, resized_hw, crop_hw=None, offset=(0, 0), antialias=True, out=None):
    """img fp32 [C, H, W] on the device -> fp32 [C, ch, cw]: bilinear resize to `resized_hw` = (rh, rw) as
    torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=antialias) does it, then the window of
    `crop_hw` = (ch, cw) (default: the resized image) whose pixel (oy, ox) is the resized pixel (oy + offset[0], ox + offset[1]);
    0.0 outside the resized image. One or two launches on the current stream (horizontal pass first, only the rows and columns
    the crop keeps; a pass is left out when its axis keeps its size). Allocates the result unless `out` is given, and the
    intermediate of a two-pass resize. HIP path only: a CPU tensor raises RuntimeError."""
    if not isinstance(img, torch.Tensor) or not img.is_cuda or (out is not None and not out.is_cuda):
        raise RuntimeError("resize_f32 runs on the HIP path only (there is no CPU fallback)")
    Cn, H, W = _planes_f32(img, "img")
    rh, rw = int(resized_hw[0]), int(resized_hw[1])
    ch, cw = (rh, rw) if crop_hw is None else (int(crop_hw[0]), int(crop_hw[1]))
    yoff, xoff = int(offset[0]), int(offset[1])
    if min(rh, rw, ch, cw) < 1:
        raise ValueError(f"resize_f32: resized {rh} x {rw}, crop {ch} x {cw}")
    if out is None:
        out = torch.empty((Cn, ch, cw), dtype=torch.float32, device=img.device)
    elif tuple(out.shape) != (Cn, ch, cw) or out.dtype != torch.float32 or out.device != img.device or not out.is_contiguous():
        raise ValueError(f"resize_f32: out must be contiguous fp32 [{Cn}, {ch}, {cw}] on {img.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    with torch.cuda.device(img.device):
        tab_x = _resize_tables_f32(W, rw, antialias, img.device) if rw != W else None
        tab_y = _resize_tables_f32(H, rh, antialias, img.device) if rh != H else None
        common = dict(resized=(rh, rw), offset=(yoff, xoff))
        ry0, ry1, rx0, rx1 = max(yoff, 0), min(ch + yoff, rh), max(xoff, 0), min(cw + xoff, rw)
        if ry0 >= ry1 or rx0 >= rx1:                                  # the window misses the image: all padding
            resize_f32_finish(img, out, None, axis=0, src_hw=(H, W), origin=(0, 0), **common)
        elif tab_x is not None and tab_y is not None:
            y0, rows = tab_y.span(ry0, ry1)
            cols = rx1 - rx0
            tmp = torch.empty((Cn, rows, cols), dtype=torch.float32, device=img.device)
            resize_f32_h(img, tmp, tab_x, y0=y0, rows=rows, x0=rx0, cols=cols)
            resize_f32_finish(tmp, out, tab_y, axis=2, src_hw=(rows, cols), origin=(y0, rx0), **common)
        elif tab_x is not None:
            resize_f32_finish(img, out, tab_x, axis=1, src_hw=(H, W), origin=(0, 0), **common)
        elif tab_y is not None:
            resize_f32_finish(img, out, tab_y, axis=2, src_hw=(H, W), origin=(0, 0), **common)
        else:
            resize_f32_finish(img, out, None, axis=0, src_hw=(H, W), origin=(0, 0), **common)
    return out


class DeviceGraph:
    """hipGraph capture/replay of a block of dc_* calls issued on a private stream (runtime.hip)."""

    def __init__(self):
        l = _hip.lib()
        s = C.c_void_p()
        check(l.dc_stream_create(C.byref(s)), "dc_stream_create")
        self._stream = s
        self.torch_stream = torch.cuda.ExternalStream(s.value)
        self._exec = None

    def capture(self, fn):
        l = _hip.lib()
        torch.cuda.synchronize()
        # the per-stream workspaces of the capture stream must exist before capture begins (no allocation inside a
        # capture): size them like the ones the eager warm-up used on the current stream
        cur = torch.cuda.current_stream()
        dev = cur.device
        cap = self.torch_stream.cuda_stream
        if (dev.index, cur.cuda_stream) in _gemm_ws:
            _gemm_workspace(dev, cap)
        like = _gn_ws.get((dev.index, cur.cuda_stream))
        if like is not None:
            with torch.cuda.stream(self.torch_stream):
                _gn_workspace(dev, like.numel() * 4)
        with torch.cuda.stream(self.torch_stream):
            check(l.dc_graph_begin_capture(self._stream), "dc_graph_begin_capture")
            try:
                fn()
            finally:
                ex = C.c_void_p()
                code = l.dc_graph_end_capture(self._stream, C.byref(ex))
            check(code, "dc_graph_end_capture")
        self._exec = ex
        return self

    def launch(self):
        check(_hip.lib().dc_graph_launch(self._exec, self._stream), "dc_graph_launch")

    def sync(self):
        check(_hip.lib().dc_stream_sync(self._stream), "dc_stream_sync")

    def __del__(self):
        try:
            l = _hip.lib()
            if self._exec is not None:
                l.dc_graph_destroy(self._exec)
            l.dc_stream_destroy(self._stream)
        except Exception:
            pass
