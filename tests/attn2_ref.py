"""Independent reference for the fused attention kernel (csrc/attn2.hip).

A plain torch implementation of the kernel's contract, written from the
header comment of attn2.hip and not from models/attention.py:

    q      (R, DM)         row r = (b*heads + head)*n + i
    k, v   (Rkv, J, DM)    Rkv = R, or b*n when kv_one
    mask   (b, n, J)       nonzero = attend; None = attend everywhere
    qf     (b*n, rot)      rotary arguments for the queries, or None
    kf     (b*n, jr, rot)  rotary arguments for the LAST jr keys, or None

    out = softmax_j(scale * <rope(q), rope(k_j)>, masked -> -finfo(f32).max)
          @ rope(v)

The rotation acts on the first `rot` entries of the DM axis:

    out[d] = t[d] cos f[d] + sgn(d) t[P(d)] sin f[d]
    P(d) = 2d+1 for d < rot/2, else 2d-rot;   sgn = -1 in the first half

Masking is a masked_fill, so a row whose keys are all masked gets uniform
weights 1/J and no gradient passes the fill. Everything runs in `dtype`
(f64 for the reference proper; the GPU tests also run it in f32 as the
yardstick for what plain fp32 arithmetic loses). Gradients come from
autograd. The steps are separate functions so that the CPU tests can
rebuild the pipeline with one step deliberately broken.
"""
import torch

MASK_FILL = -torch.finfo(torch.float32).max


def rope_pairing(rot, device=None):
    """P(d) and sgn(d) of the rotation, d = 0..rot-1."""
    d = torch.arange(rot, device=device)
    P = torch.where(d < rot // 2, 2 * d + 1, 2 * d - rot)
    sgn = torch.where(d < rot // 2, -1.0, 1.0)
    return P, sgn


def rope(t, f, P=None):
    """Rotate the first rot = f.shape[-1] entries of t's last axis; `f`
    broadcasts against t[..., :rot]. `P` overrides the pairing."""
    rot = f.shape[-1]
    P0, sgn = rope_pairing(rot, t.device)
    if P is None:
        P = P0
    head, tail = t[..., :rot], t[..., rot:]
    head = head * f.cos() + sgn.to(t.dtype) * head[..., P] * f.sin()
    return torch.cat((head, tail), dim=-1)


def unflatten(q, k, v, mask, qf, kf, n, heads, kv_one):
    """The kernel's flat rows as (b, heads, n, ...) tensors; the head axis
    has size 1 where the kernel shares a row between heads."""
    R, DM = q.shape
    J = k.shape[1]
    b = R // (heads * n)
    assert R == b * heads * n
    q = q.view(b, heads, n, DM)
    kvh = 1 if kv_one else heads
    assert k.shape[0] == b * kvh * n and v.shape == k.shape
    k = k.view(b, kvh, n, J, DM)
    v = v.view(b, kvh, n, J, DM)
    if mask is not None:
        mask = (mask.view(b, 1, n, J) != 0)
    if qf is not None:
        qf = qf.view(b, 1, n, qf.shape[-1])
    if kf is not None:
        kf = kf.view(b, 1, n, kf.shape[1], kf.shape[2])
    return q, k, v, mask, qf, kf


def rope_last(t, kf, P=None):
    """Rotate the last jr = kf.shape[-2] keys of t (b, h, n, J, DM)."""
    jr = kf.shape[-2]
    J = t.shape[-2]
    return torch.cat((t[..., :J - jr, :], rope(t[..., J - jr:, :], kf, P)),
                     dim=-2)


def attend(q, k, v, mask, scale):
    """q (b,h,n,DM), k/v (b,h|1,n,J,DM), mask (b,1,n,J) bool or None."""
    sim = (q.unsqueeze(-2) * k).sum(-1) * scale          # b h n J
    if mask is not None:
        sim = sim.masked_fill(~mask, MASK_FILL)
    attn = sim.softmax(dim=-1)
    return (attn.unsqueeze(-1) * v).sum(-2)              # b h n DM


def attn2_reference(q, k, v, mask, n, heads, scale, kv_one=False,
                    qf=None, kf=None):
    """out (R, DM) in q's dtype; differentiable in q, k, v."""
    q5, k5, v5, m5, qf5, kf5 = unflatten(q, k, v, mask, qf, kf, n, heads,
                                         kv_one)
    if qf5 is not None:
        q5 = rope(q5, qf5.to(q.dtype))
    if kf5 is not None:
        k5 = rope_last(k5, kf5.to(q.dtype))
        v5 = rope_last(v5, kf5.to(q.dtype))
    return attend(q5, k5, v5, m5, scale).reshape(q.shape)


def with_grads(fn, q, k, v, g, dtype=torch.float64):
    """Run fn(q, k, v) -> out on detached `dtype` copies and pull the fixed
    upstream gradient g back through it. Returns (out, dq, dk, dv)."""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    out = fn(q, k, v)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), g.to(dtype))
    return out.detach(), dq, dk, dv


def reference_with_grads(q, k, v, mask, n, heads, scale, kv_one, qf, kf, g,
                         dtype=torch.float64):
    return with_grads(
        lambda q_, k_, v_: attn2_reference(q_, k_, v_, mask, n, heads, scale,
                                           kv_one, qf, kf),
        q, k, v, g, dtype)
