"""The RadialFunc trunk (net.0 .. net.5: Linear(D->128), LayerNorm, exact-erf
GELU, Linear(128->128), LayerNorm, GELU) in explicit formulas, forward and
backward, as the model of a correct csrc/radial.hip.

With declared_rounding off it is exact math on the given inputs in `dtype`.
With it on, a value is rounded to bf16 wherever radial.hip declares, in its
header and its buffers, that it is held in bf16:
  forward   a1 before the second GEMM; H, yh0, yh3 as stored
  backward  dH on entry; z and a1 recomputed from the stored (rounded) yh;
            dy3 before its two GEMMs (dW3 and da1)
Everything else stays in `dtype`; the variance is two-pass, sums are torch's.
Nothing here follows the kernel's summation order or its variance formula.

Every step a kernel could get wrong is a method of Trunk, so that
test_radial_reference.py can break exactly one of them in a subclass.
"""
import math
from collections import namedtuple

import torch

Forward = namedtuple('Forward', 'H yh0 yh3 rs0 rs3')
Grads = namedtuple('Grads', 'dX dW0 db0 dg0 dbe0 dW3 db3 dg3 dbe3')
FWD_NAMES = Forward._fields
GRAD_NAMES = Grads._fields

_SQRT_HALF = math.sqrt(0.5)
_INV_SQRT_2PI = 1. / math.sqrt(2. * math.pi)


def gelu(z):
    return 0.5 * z * (1. + torch.erf(z * _SQRT_HALF))


def dgelu(z):
    cdf = 0.5 * (1. + torch.erf(z * _SQRT_HALF))
    return cdf + z * _INV_SQRT_2PI * torch.exp(-0.5 * z * z)


class Trunk:
    def __init__(self, dtype=torch.float64, declared_rounding=False):
        self.dtype = dtype
        self.declared_rounding = declared_rounding

    def r(self, t):
        """A declared bf16 storage point."""
        if not self.declared_rounding:
            return t
        return t.to(torch.bfloat16).to(self.dtype)

    # ---- the steps ---------------------------------------------------------
    def stats(self, y, layer):
        """Mean and (biased) variance of each row of LayerNorm `layer`
        (0 or 3), two-pass."""
        mean = y.mean(-1, keepdim=True)
        var = ((y - mean) ** 2).mean(-1, keepdim=True)
        return mean, var

    def rstd(self, var, eps):
        return (var + eps) ** -0.5

    def yhat_in_backward(self, yh_stored, g, be):
        """The normalised activation the backward works from: the stored
        one. z follows from it without a division."""
        return yh_stored

    def ln_param_grads(self, dz, yh):
        """(dgamma, dbeta) of z = yh * gamma + beta."""
        return (dz * yh).sum(0), dz.sum(0)

    def ln_backward(self, dz, yh, g, rs):
        dyh = dz * g
        m1 = dyh.mean(-1, keepdim=True)
        m2 = (dyh * yh).mean(-1, keepdim=True)
        return rs * (dyh - m1 - yh * m2)

    def db3(self, dz3, dy3):
        return dy3.sum(0)

    def da1(self, dy3, W3):
        return dy3 @ W3

    def rs_in_ln0_backward(self, rs0, rs3):
        return rs0

    def dx(self, dy0, W0):
        return dy0 @ W0

    # ---- the trunk ---------------------------------------------------------
    def layer_norm(self, y, layer, eps):
        mean, var = self.stats(y, layer)
        rs = self.rstd(var, eps)
        return (y - mean) * rs, rs

    def __call__(self, x, W0, b0, g0, be0, W3, b3, g3, be3, dH=None,
                 eps=1e-5):
        T = self.dtype
        x, W0, b0, g0, be0, W3, b3, g3, be3 = (
            t.detach().to(T) for t in (x, W0, b0, g0, be0, W3, b3, g3, be3))
        r = self.r
        y0 = x @ W0.t() + b0
        yh0, rs0 = self.layer_norm(y0, 0, eps)
        a1 = r(gelu(yh0 * g0 + be0))
        y3 = a1 @ W3.t() + b3
        yh3, rs3 = self.layer_norm(y3, 3, eps)
        H = r(gelu(yh3 * g3 + be3))
        yh0_s, yh3_s = r(yh0), r(yh3)
        fwd = Forward(H, yh0_s, yh3_s, rs0[:, 0], rs3[:, 0])
        if dH is None:
            return fwd

        dH = r(dH.detach().to(T))
        yb3 = self.yhat_in_backward(yh3_s, g3, be3)
        yb0 = self.yhat_in_backward(yh0_s, g0, be0)
        z0 = yb0 * g0 + be0
        a1b = r(gelu(z0))
        dz3 = dH * dgelu(yb3 * g3 + be3)
        dg3, dbe3 = self.ln_param_grads(dz3, yb3)
        dy3 = self.ln_backward(dz3, yb3, g3, rs3)
        db3 = self.db3(dz3, dy3)
        dy3 = r(dy3)
        dW3 = dy3.t() @ a1b
        dz0 = self.da1(dy3, W3) * dgelu(z0)
        dg0, dbe0 = self.ln_param_grads(dz0, yb0)
        dy0 = self.ln_backward(dz0, yb0, g0,
                               self.rs_in_ln0_backward(rs0, rs3))
        db0 = dy0.sum(0)
        dW0 = dy0.t() @ x
        dX = self.dx(dy0, W0)
        return fwd, Grads(dX, dW0, db0, dg0, dbe0, dW3, db3, dg3, dbe3)


def radial_reference(x, W0, b0, g0, be0, W3, b3, g3, be3, dH=None, eps=1e-5,
                     dtype=torch.float64, declared_rounding=False,
                     trunk=Trunk):
    """Forward(H, yh0, yh3, rs0, rs3), and with dH also
    Grads(dX, dW0, db0, dg0, dbe0, dW3, db3, dg3, dbe3), all in `dtype`."""
    return trunk(dtype, declared_rounding)(x, W0, b0, g0, be0, W3, b3, g3,
                                           be3, dH=dH, eps=eps)
