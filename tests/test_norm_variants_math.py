"""The analytic backward of the gated-scale NormSE3 that csrc/norm_se3.hip
implements, transcribed to torch and checked against autograd in f64.

    nu    = max(|t|, eps)            p = t / nu          live = |t| > eps
    gate  = nu @ W                   a = p . dout
    out   = g(gate) * p
    dgate = g'(gate) * a
    dnu   = dgate @ W^T
    dt    = g(gate)/nu * (dout - a p) + dnu * p      (live)
    dt    = g(gate)/eps * dout                       (clamped: no dnu term)
    dW    = nu^T @ dgate
"""
import math

import pytest
import torch
from torch import nn

from se3_transformer_amd.models.core import NormSE3
from se3_transformer_amd.models.fiber import Fiber


def _g(name, x):
    if name == 'identity':
        return x, torch.ones_like(x)
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return x * cdf, cdf + x * pdf


def gated_backward(t, W, dout, eps, nonlin):
    """t, dout (N, C, M); W (C, C). Returns out, dt, dW."""
    nraw = t.norm(dim=-1)
    live = (nraw > eps).unsqueeze(-1)
    nu = nraw.clamp(min=eps)
    p = t / nu.unsqueeze(-1)
    gate = nu @ W
    g, gp = _g(nonlin, gate)
    out = g.unsqueeze(-1) * p
    a = (p * dout).sum(-1)
    dgate = gp * a
    dnu = dgate @ W.t()
    dt_live = (g / nu).unsqueeze(-1) * (dout - a.unsqueeze(-1) * p) \
        + dnu.unsqueeze(-1) * p
    dt_clamped = (g / eps).unsqueeze(-1) * dout
    dt = torch.where(live, dt_live, dt_clamped)
    dW = nu.t() @ dgate
    return out, dt, dW


@pytest.mark.parametrize('nonlin', ['gelu', 'identity'])
@pytest.mark.parametrize('m', [1, 3, 5, 7])
def test_gated_backward_formulas_match_autograd(m, nonlin):
    torch.manual_seed(0)
    N, C, eps = 11, 9, 1e-3
    degree = (m - 1) // 2
    mod = NormSE3(Fiber([(degree, C)]), gated_scale=True, eps=eps,
                  nonlin=nn.GELU() if nonlin == 'gelu' else nn.Identity()
                  ).double()
    W = mod.transform[str(degree)]['w_gate']
    with torch.no_grad():
        W.copy_(torch.randn(C, C, dtype=torch.float64) / math.sqrt(C))
    t = torch.randn(1, N, C, m, dtype=torch.float64)
    with torch.no_grad():
        t[0, 2, 4] = 0                 # one zero vector
        t[0, 7] = 0                    # one zero node
        t[0, 5, 1] *= 1e-4 / t[0, 5, 1].norm()    # below eps, not zero
    t.requires_grad_(True)
    dout = torch.randn(1, N, C, m, dtype=torch.float64)

    ref = mod({str(degree): t})[str(degree)]
    ref.backward(dout)

    out, dt, dW = gated_backward(t.detach()[0], W.detach(), dout[0], eps,
                                 nonlin)
    assert torch.isfinite(dt).all() and torch.isfinite(dW).all()
    assert (out - ref.detach()[0]).abs().max() < 1e-13
    assert (dt - t.grad[0]).abs().max() < 1e-12 * (1 + t.grad.abs().max())
    assert (dW - W.grad).abs().max() < 1e-12 * (1 + W.grad.abs().max())
    # clamped vectors carry no dnu term
    g, _ = _g(nonlin, (t.detach()[0].norm(dim=-1).clamp(min=eps)
                       @ W.detach()))
    for (n, c) in [(2, 4), (7, 0), (7, C - 1), (5, 1)]:
        assert torch.equal(dt[n, c], g[n, c] / eps * dout[0, n, c])
