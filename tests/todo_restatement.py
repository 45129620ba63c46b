"""K/V token downsampling ("ToDo", Smith et al., IJCAI 2024) of the spatial self-attention restated in torch, no GPU: what
csrc/token_pool.hip, ops.ln_pool_tokens and UNetModel.enable_token_downsampling are tested against (tests/test_todo_cpu.py,
tests/test_todo_gpu.py).

    pooled_grid          (ceil(H / f), ceil(W / f))
    pool_tokens          the pooled tokens of a normalised token tensor, float64: "nearest" n[::f, ::f], "mean" the cell means
    ln_pool_tokens       LayerNorm, then pool_tokens, in a chosen dtype (float64: the reference; float32: its fp32 error)
    self_attention_todo  attn1 with q from all tokens and k / v from the pooled ones, from oracle.unet's parts
    unet_forward_todo    oracle.unet.unet_forward's loop with that attn1 at the selected resolution levels
"""
import torch
import torch.nn.functional as F

from oracle import unet as ounet

MODES = ("nearest", "mean")


def pooled_grid(H, W, f):
    return -(-H // f), -(-W // f)


def _pool(n, H, W, f, mode):
    """n [..., H*W, C] (tokens in row-major (y, x) order) -> [..., Hp*Wp, C] in n's dtype, written out cell by cell."""
    if mode not in MODES:
        raise ValueError(mode)
    lead, Cc = n.shape[:-2], n.shape[-1]
    g = n.reshape(lead + (H, W, Cc))
    Hp, Wp = pooled_grid(H, W, f)
    if mode == "nearest":
        return g[..., ::f, ::f, :].reshape(lead + (Hp * Wp, Cc))
    out = torch.empty(lead + (Hp, Wp, Cc), dtype=n.dtype)
    for yp in range(Hp):
        for xp in range(Wp):
            cell = g[..., yp * f:min(H, yp * f + f), xp * f:min(W, xp * f + f), :]
            count = cell.shape[-3] * cell.shape[-2]                  # the tokens actually in the cell (clipped at the border)
            out[..., yp, xp, :] = cell.sum(dim=(-3, -2)) / count
    return out.reshape(lead + (Hp * Wp, Cc))


def pool_tokens(n, H, W, f, mode):
    """The definition, in float64."""
    return _pool(n.to(torch.float64), H, W, f, mode)


def ln_pool_tokens(x, gamma, beta, H, W, f, mode, eps=1e-5, dtype=torch.float64):
    """pool(LayerNorm(x)) with everything in `dtype`; x [..., H*W, C]."""
    x = x.to(dtype)
    n = F.layer_norm(x, (x.shape[-1],), gamma.to(dtype), beta.to(dtype), eps)
    return _pool(n, H, W, f, mode)


def self_attention_todo(sd, p, n, heads, dim_head, H, W, f, mode):
    """attn1 of a spatial transformer block on the normalised tokens n [b, H*W, C]: q = to_q(n) on all tokens, k = to_k(p),
    v = to_v(p) on the pooled tokens p, softmax(q k^T dim_head^-0.5) v, to_out. In n's dtype (the pooling is then in that dtype
    too: a strided slice, or sums of at most f^2 terms)."""
    pooled = _pool(n, H, W, f, mode)
    q = ounet._lin(sd, p + ".to_q", n)
    k = ounet._lin(sd, p + ".to_k", pooled)
    v = ounet._lin(sd, p + ".to_v", pooled)
    out = ounet.attention_core(q, k, v, heads, dim_head ** -0.5)
    return ounet._lin(sd, p + ".to_out.0", out)


def _transformer_block(sd, p, x, context, heads, dim_head, cfg, image_cross, H, W, todo):
    """oracle.unet.transformer_block with attn1 replaced when `todo` = (f, mode) is given."""
    def ln(name, t):
        return F.layer_norm(t, (t.shape[-1],), sd[f"{p}.{name}.weight"], sd[f"{p}.{name}.bias"], 1e-5)
    if todo is None:
        x = ounet.cross_attention(sd, p + ".attn1", ln("norm1", x), None, heads, dim_head, cfg, False) + x
    else:
        x = self_attention_todo(sd, p + ".attn1", ln("norm1", x), heads, dim_head, H, W, *todo) + x
    x = ounet.cross_attention(sd, p + ".attn2", ln("norm2", x), context, heads, dim_head, cfg, image_cross) + x
    x = ounet.feed_forward(sd, p + ".ff", ln("norm3", x)) + x
    return x


def _spatial_transformer(sd, p, x, context, heads, dim_head, cfg, todo):
    """oracle.unet.spatial_transformer around _transformer_block."""
    b, c, h, w = x.shape
    x_in = x
    x = ounet._gn(sd, p + ".norm", x, 1e-6)
    x = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
    x = ounet._lin(sd, p + ".proj_in", x)
    x = _transformer_block(sd, p + ".transformer_blocks.0", x, context, heads, dim_head, cfg, cfg.image_cross_attention, h, w, todo)
    x = ounet._lin(sd, p + ".proj_out", x)
    x = x.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return x + x_in


def _run_block(sd, prefix, layers, h, emb, context, b, cfg, lvl, todo):
    """oracle.unet._run_block's dispatch, each layer through that module's own function, with the resolution level tracked
    through down / up and the spatial transformers of the selected levels replaced; returns (h, the level after the block)."""
    for j, (kind, info) in enumerate(layers):
        p = f"{prefix}.{j}"
        if kind == "conv_in":
            h = F.conv2d(h, sd[p + ".weight"], sd[p + ".bias"], padding=1)
        elif kind == "res":
            h = ounet.res_block(sd, p, h, emb, b, cfg)
        elif kind == "spatial":
            on = todo is not None and lvl in todo["levels"]
            h = _spatial_transformer(sd, p, h, context, info["heads"], cfg.num_head_channels, cfg,
                                     (todo["factor"], todo["mode"]) if on else None)
        elif kind == "temporal":
            bt, c, hh, ww = h.shape
            h5 = h.reshape(b, bt // b, c, hh, ww).permute(0, 2, 1, 3, 4)
            h5 = ounet.temporal_transformer(sd, p, h5, info["heads"], cfg.num_head_channels, cfg)
            h = h5.permute(0, 2, 1, 3, 4).reshape(bt, c, hh, ww)
        elif kind == "down":
            h = F.conv2d(h, sd[p + ".op.weight"], sd[p + ".op.bias"], stride=2, padding=1)
            lvl += 1
        elif kind == "up":
            h = F.interpolate(h, scale_factor=2, mode="nearest")
            h = F.conv2d(h, sd[p + ".conv.weight"], sd[p + ".conv.bias"], padding=1)
            lvl -= 1
        else:
            raise ValueError(kind)
    return h, lvl


def check_todo(todo, cfg):
    """The completed copy of a `todo` dict (factor, levels, mode), or None."""
    if todo is None:
        return None
    t = dict(factor=2, levels=(0,), mode="nearest")
    t.update(todo)
    assert isinstance(t["factor"], int) and 2 <= t["factor"] <= 8 and t["mode"] in MODES
    assert t["levels"] and all(0 <= l < len(cfg.channel_mult) for l in t["levels"])
    return t


@torch.no_grad()
def unet_forward_todo(sd, cfg, x, timesteps, context, fs=None, todo=None):
    """oracle.unet.unet_forward with token downsampling in the spatial attn1 of the levels todo["levels"]; todo = dict(factor,
    levels, mode) or None (then, bit for bit, unet_forward). The loop is unet_forward's, rebuilt from that module's own parts."""
    todo = check_todo(todo, cfg)
    b, _, t, _, _ = x.shape
    mc = cfg.model_channels
    emb = ounet._mlp(sd, "time_embed", ounet.timestep_embedding(timesteps, mc))
    if context.shape[1] == 77 + t * 16:
        ctx_text, ctx_img = context[:, :77], context[:, 77:]
        ctx_text = ctx_text.repeat_interleave(t, dim=0)
        ctx_img = ctx_img.reshape(b, t, -1, ctx_img.shape[-1]).reshape(b * t, -1, ctx_img.shape[-1])
        context = torch.cat([ctx_text, ctx_img], dim=1)
    else:
        context = context.repeat_interleave(t, dim=0)
    emb = emb.repeat_interleave(t, dim=0)
    h = x.permute(0, 2, 1, 3, 4).reshape(b * t, x.shape[1], x.shape[3], x.shape[4])
    if cfg.fs_condition:
        if fs is None:
            fs = torch.tensor([cfg.default_fs] * b, dtype=torch.long)
        emb = emb + ounet._mlp(sd, "fps_embedding", ounet.timestep_embedding(fs, mc)).repeat_interleave(t, dim=0)
    inp, mid, out = ounet.build_plan(cfg)
    hs = []
    lvl = 0
    for i, layers in enumerate(inp):
        h, lvl = _run_block(sd, f"input_blocks.{i}", layers, h, emb, context, b, cfg, lvl, todo)
        if i == 0 and cfg.addition_attention:
            bt, c, hh, ww = h.shape
            h5 = h.reshape(b, t, c, hh, ww).permute(0, 2, 1, 3, 4)
            h5 = ounet.temporal_transformer(sd, "init_attn.0", h5, 8, cfg.num_head_channels, cfg)
            h = h5.permute(0, 2, 1, 3, 4).reshape(bt, c, hh, ww)
        hs.append(h)
    h, lvl = _run_block(sd, "middle_block", mid, h, emb, context, b, cfg, lvl, todo)
    for i, layers in enumerate(out):
        h = torch.cat([h, hs.pop()], dim=1)
        h, lvl = _run_block(sd, f"output_blocks.{i}", layers, h, emb, context, b, cfg, lvl, todo)
    assert lvl == 0
    h = F.silu(ounet._gn(sd, "out.0", h, 1e-5))
    y = F.conv2d(h, sd["out.2.weight"], sd["out.2.bias"], padding=1)
    return y.reshape(b, t, y.shape[1], y.shape[2], y.shape[3]).permute(0, 2, 1, 3, 4)
