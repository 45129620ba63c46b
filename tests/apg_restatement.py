"""Adaptive projected guidance restated from Algorithm 1 of Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of
High Guidance Scales in Diffusion Models" (ICLR 2025), in plain torch on the CPU. float64 is the reference of the tests; the same
code in float32 is their yardstick for what one precision class costs.

Per clip (all norms and dot products over every non-batch element), w the guidance scale:
    d      = p_c - p_u
    m      = d + momentum * m_prev            (m_prev = 0 at the first step; m is kept unscaled)
    s      = min(1, norm_threshold / ||m||)   (no threshold, a threshold <= 0 or ||m|| = 0: s = 1)
    D      = s * m
    par    = (D . p_c / ||p_c||^2) * p_c      (p_c = 0: par = 0)
    guided = p_c + (w - 1) * ((D - par) + eta * par)
space "model": p_c, p_u are the model outputs. space "x0": the denoised predictions, x0 = sqrt(a) x - sqrt(1-a) v for a v model,
(x - sqrt(1-a) eps) / sqrt(a) for an eps model, and the guided x0 is mapped back to the model's output space."""
import torch


def _per_clip(v, like):
    return v.reshape((-1,) + (1,) * (like.dim() - 1))


def guide(p_c, p_u, m_prev, *, w, eta=0.0, norm_threshold=None, momentum=0.0):
    """(guided, m) for predictions [B, ...] in the dtype of p_c."""
    d = p_c - p_u
    m = d if m_prev is None else d + momentum * m_prev
    s = torch.ones(p_c.shape[0], dtype=p_c.dtype)
    if norm_threshold is not None and norm_threshold > 0:
        norm = m.flatten(1).norm(dim=1)
        s = torch.where(norm > 0, torch.minimum(torch.ones_like(norm), norm_threshold / norm.clamp_min(1e-30)), s)
    D = _per_clip(s, m) * m
    pp = (p_c * p_c).flatten(1).sum(1)
    dot = (D * p_c).flatten(1).sum(1)
    coef = torch.where(pp > 0, dot / torch.where(pp > 0, pp, torch.ones_like(pp)), torch.zeros_like(pp))
    par = _per_clip(coef, p_c) * p_c
    return p_c + (w - 1.0) * ((D - par) + eta * par), m


def to_x0(e, x, sqrt_a, sqrt_1ma, v_param):
    return sqrt_a * x - sqrt_1ma * e if v_param else (x - sqrt_1ma * e) / sqrt_a


def from_x0(p, x, sqrt_a, sqrt_1ma, v_param):
    return (sqrt_a * x - p) / sqrt_1ma if v_param else (x - sqrt_a * p) / sqrt_1ma


def apg(e_c, e_u, x, m_prev, *, w, eta=0.0, norm_threshold=None, momentum=0.0, space="x0", v_param=True, sqrt_a=None,
        sqrt_1ma=None, dtype=torch.float64):
    """One step on model outputs e_c, e_u and the latent x ([B, C, ...]): (the guided model output, m), computed in `dtype`.
    sqrt_a, sqrt_1ma: sqrt(a_t) and sqrt(1 - a_t) of the step, Python floats (space "x0")."""
    e_c, e_u, x = (t.to(dtype) for t in (e_c, e_u, x))
    m_prev = None if m_prev is None else m_prev.to(dtype)
    kw = dict(w=w, eta=eta, norm_threshold=norm_threshold, momentum=momentum)
    if space == "model":
        return guide(e_c, e_u, m_prev, **kw)
    assert space == "x0"
    g, m = guide(to_x0(e_c, x, sqrt_a, sqrt_1ma, v_param), to_x0(e_u, x, sqrt_a, sqrt_1ma, v_param), m_prev, **kw)
    return from_x0(g, x, sqrt_a, sqrt_1ma, v_param), m


def cfg(e_c, e_u, w):
    return e_u + w * (e_c - e_u)
