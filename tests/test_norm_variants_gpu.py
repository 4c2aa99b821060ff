"""GPU parity of the fused NormSE3 variants (csrc/norm_se3.hip):
{scale, gated scale} x {exact-erf GELU, identity}. The oracle is always the
same module under SE3_EAGER_NORM=1, the metric the max-normalised _rel_err.

w_gate is set to randn(C, C)/sqrt(C): the default +-1e-3 init leaves
gate ~ 0, which tests nothing.
"""
import math

import pytest
import torch
from torch import nn

from fused_helpers import switches

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

NONLINS = {'gelu': nn.GELU, 'identity': nn.Identity}


def _rel_err(a, b):
    denom = b.abs().max().clamp(min=1e-6)
    return ((a - b).abs().max() / denom).item()


def _make(C, m, nonlin, gated, eps=1e-12, seed=0, device='cuda'):
    from se3_transformer_amd.models.core import NormSE3
    from se3_transformer_amd.models.fiber import Fiber
    degree = (m - 1) // 2
    mod = NormSE3(Fiber([(degree, C)]), nonlin=NONLINS[nonlin](),
                  gated_scale=gated, eps=eps)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        if gated:
            mod.transform[str(degree)]['w_gate'].copy_(
                torch.randn(C, C, generator=g) / math.sqrt(C))
        else:
            mod.transform[str(degree)]['scale'].copy_(
                1 + 0.5 * torch.randn(1, 1, C, generator=g))
    return mod.to(device), str(degree)


def _feats(shape, floor=0.05):
    """randn features with every vector norm at least `floor`.

    The eager oracle's own fp32 backward goes through t/|t|, whose two
    gradient terms d/|t| and (d.t) t/|t|^3 cancel (at M = 1 completely), so
    its t.grad carries noise of about 1e-7/|t| relative. Measured on the CPU,
    eager fp32 against eager f64 at these shapes with plain randn and M = 1:
    median 1e-5, up to 2.5e-4 over 20 seeds, i.e. the oracle alone can
    exceed the 1e-4 bound. With |t| >= 0.05 the same measurement gives
    median 1.5e-6, at most 5e-6, and the bound judges the kernel. Tiny and zero vectors are the clamp test's.
    """
    t = torch.randn(shape, device='cuda')
    n = t.norm(dim=-1, keepdim=True)
    return torch.where(n < floor, t * (floor / n.clamp(min=1e-30)), t)


def _param(mod, key):
    p = mod.transform[key]
    return p['w_gate'] if 'w_gate' in p else p['scale']


def _run(mod, key, t, dout=None, eager=False):
    """forward + backward; returns out, t.grad, param.grad (all detached)."""
    t = t.detach().clone().requires_grad_(True)
    mod.zero_grad()
    if eager:
        with switches(SE3_EAGER_NORM='1'):
            out = mod({key: t})[key]
    else:
        out = mod({key: t})[key]
    if dout is None:
        out.pow(2).mean().backward()
    else:
        out.backward(dout)
    return out.detach(), t.grad.clone(), _param(mod, key).grad.clone()


class _Counter:
    """Counts calls to the fused entry points of ops.fused."""

    def __init__(self, monkeypatch):
        from se3_transformer_amd.ops import fused
        self.n = {'norm_se3': 0, 'norm_se3_gated': 0}
        for name in self.n:
            monkeypatch.setattr(fused, name, self._wrap(name,
                                                        getattr(fused, name)))

    def _wrap(self, name, fn):
        def counted(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return counted

    @property
    def total(self):
        return sum(self.n.values())


# ---- 1. dispatch ----------------------------------------------------------

@needs_gpu
def test_variants_reach_the_fused_path(monkeypatch):
    from se3_transformer_amd.ops import fused
    ext = fused._load_ext()
    for name in ('norm_se3_nl_fwd', 'norm_se3_nl_bwd',
                 'norm_se3_gated_fwd', 'norm_se3_gated_bwd'):
        assert hasattr(ext, name), f'extension lacks {name}'
    assert fused.ext_available()

    cnt = _Counter(monkeypatch)
    t = torch.randn(2, 5, 24, 3, device='cuda')
    for nonlin in ('gelu', 'identity'):
        mod, key = _make(24, 3, nonlin, gated=True)
        before = cnt.n['norm_se3_gated']
        mod({key: t})
        assert cnt.n['norm_se3_gated'] == before + 1, nonlin
    mod, key = _make(24, 3, 'identity', gated=False)
    before = cnt.n['norm_se3']
    mod({key: t})
    assert cnt.n['norm_se3'] == before + 1

    total = cnt.total
    with switches(SE3_EAGER_NORM='1'):
        for nonlin in ('gelu', 'identity'):
            for gated in (True, False):
                mod, key = _make(24, 3, nonlin, gated=gated)
                mod({key: t})
    assert cnt.total == total, 'SE3_EAGER_NORM=1 reached the fused path'


# ---- 2. kernel parity, fp32 ----------------------------------------------

# rows no multiple of the node tile and C below one wave; C just over two
# waves; C above the 256-thread block (strided channel loop)
SHAPES = [(2, 37, 24), (1, 5, 130), (1, 3, 300)]


# scale+GELU is the original kernel pair: test_fused_gpu covers it
NEW_VARIANTS = [('gated', 'gelu'), ('gated', 'identity'),
                ('scale', 'identity')]


@needs_gpu
@pytest.mark.parametrize('variant,nonlin', NEW_VARIANTS)
@pytest.mark.parametrize('m', [1, 3, 5, 7])
def test_kernel_vs_eager_fp32(m, variant, nonlin):
    for si, (b, n, C) in enumerate(SHAPES):
        torch.manual_seed(10 + si)
        mod, key = _make(C, m, nonlin, gated=(variant == 'gated'), seed=si)
        t = _feats((b, n, C, m))
        ref, dt_ref, dp_ref = _run(mod, key, t, eager=True)
        out, dt, dp = _run(mod, key, t)
        errs = (_rel_err(out, ref), _rel_err(dt, dt_ref),
                _rel_err(dp, dp_ref))
        print(f'{variant} {nonlin} m={m} {(b, n, C)}: out/dt/dparam {errs}')
        assert dp.shape == _param(mod, key).shape
        assert dp.dtype == torch.float32
        assert errs[0] < 1e-5, errs
        assert errs[1] < 1e-4, errs
        assert errs[2] < 1e-4, errs


# ---- 3. clamp branch -------------------------------------------------------

@needs_gpu
@pytest.mark.parametrize('variant', ['gated', 'scale'])
@pytest.mark.parametrize('nonlin', ['gelu', 'identity'])
def test_clamp_branch(nonlin, variant):
    import torch.nn.functional as F
    eps, C, m = 1e-3, 24, 3
    torch.manual_seed(3)
    mod, key = _make(C, m, nonlin, gated=(variant == 'gated'), eps=eps)
    t = torch.randn(2, 9, C, m, device='cuda')
    t[0, 2, 4] = 0                       # one zero vector
    t[1, 6] = 0                          # one whole node
    t[0, 5, 1] *= 1e-4 / t[0, 5, 1].norm()      # norm 1e-4 < eps
    dout = torch.randn_like(t)
    ref, dt_ref, dp_ref = _run(mod, key, t, dout, eager=True)
    out, dt, dp = _run(mod, key, t, dout)
    for x in (out, dt, dp):
        assert torch.isfinite(x).all()
    errs = (_rel_err(out, ref), _rel_err(dt, dt_ref), _rel_err(dp, dp_ref))
    print(f'clamp {variant} {nonlin}: out/dt/dparam {errs}')
    assert errs[0] < 1e-5, errs
    assert errs[1] < 1e-4, errs
    assert errs[2] < 1e-4, errs

    # clamped vectors: dt = g(gate)/eps * dout and nothing else. The gate is
    # rebuilt here in fp32 from the same inputs, so agreement is to the
    # last bits of the erf and of the C-term sum (1e-5, the forward bound);
    # a stray dnu*p or a*p term would be of order one.
    nu = t.norm(dim=-1).clamp(min=eps)
    p = _param(mod, key).detach()
    gate = nu @ p if variant == 'gated' else nu * p
    g = F.gelu(gate) if nonlin == 'gelu' else gate
    want = (g / eps).unsqueeze(-1) * dout
    clamped = torch.zeros(2, 9, C, dtype=torch.bool, device='cuda')
    clamped[0, 2, 4] = clamped[1, 6] = clamped[0, 5, 1] = True
    assert torch.equal(clamped, t.norm(dim=-1) <= eps)
    assert _rel_err(dt[clamped], want[clamped]) < 1e-5


# ---- 4. bf16 storage -------------------------------------------------------

@needs_gpu
@pytest.mark.parametrize('variant', ['gated', 'scale'])
@pytest.mark.parametrize('nonlin', ['gelu', 'identity'])
@pytest.mark.parametrize('shape', [(2, 37, 24, 3), (1, 5, 130, 7)])
def test_kernel_vs_eager_bf16(shape, nonlin, variant):
    """bf16 t and dout, math in fp32: against the eager module on .float()
    copies of the same bf16 tensors the only divergence is the kernel's
    final rounding. Half an ulp is 2^-9 relative per element, doubled for
    the rounding of the oracle's own comparison copy: 2^-8."""
    b, n, C, m = shape
    torch.manual_seed(4)
    mod, key = _make(C, m, nonlin, gated=(variant == 'gated'))
    t = _feats(shape).to(torch.bfloat16)
    dout = (torch.randn(shape, device='cuda') / t.numel()).to(torch.bfloat16)
    ref, dt_ref, dp_ref = _run(mod, key, t.float(), dout.float(), eager=True)
    out, dt, dp = _run(mod, key, t, dout)
    assert out.dtype == torch.bfloat16 and dt.dtype == torch.bfloat16
    assert dp.dtype == torch.float32
    errs = (_rel_err(out.float(), ref.to(torch.bfloat16).float()),
            _rel_err(dt.float(), dt_ref.to(torch.bfloat16).float()),
            _rel_err(dp, dp_ref))
    print(f'bf16 {variant} {nonlin} {shape}: out/dt/dparam {errs}')
    assert errs[0] < 2 ** -8, errs
    assert errs[1] < 2 ** -8, errs
    assert errs[2] < 1e-4, errs


# ---- 5. fallbacks ----------------------------------------------------------

@needs_gpu
def test_fallbacks_stay_eager(monkeypatch):
    from se3_transformer_amd.models.core import NormSE3
    from se3_transformer_amd.models.fiber import Fiber
    from se3_transformer_amd.ops import fused
    cnt = _Counter(monkeypatch)
    torch.manual_seed(5)

    def same_as_oracle(mod, key, t):
        out = mod({key: t})[key]
        with switches(SE3_EAGER_NORM='1'):
            ref = mod({key: t})[key]
        assert torch.equal(out, ref)

    # one channel above the gated kernels' ceiling
    C = fused.NORM_GATED_MAX_C + 1
    mod, key = _make(C, 3, 'gelu', gated=True)
    same_as_oracle(mod, key, torch.randn(1, 4, C, 3, device='cuda'))
    # tanh-GELU is not the kernels' exact-erf GELU
    for gated in (True, False):
        mod = NormSE3(Fiber([(1, 24)]), nonlin=nn.GELU(approximate='tanh'),
                      gated_scale=gated).to('cuda')
        same_as_oracle(mod, '1', torch.randn(2, 5, 24, 3, device='cuda'))
    # f64
    for gated in (True, False):
        mod, key = _make(24, 3, 'identity', gated=gated)
        mod = mod.double()
        same_as_oracle(mod, key, torch.randn(2, 5, 24, 3, device='cuda',
                                             dtype=torch.float64))
    assert cnt.total == 0

    # and the ceiling itself is still fused
    mod, key = _make(fused.NORM_GATED_MAX_C, 1, 'identity', gated=True)
    mod({key: torch.randn(1, 4, fused.NORM_GATED_MAX_C, 1, device='cuda')})
    assert cnt.n['norm_se3_gated'] == 1


# ---- 6. model level --------------------------------------------------------

# Eager fp32 against eager f64 of these two models on identical weights and
# inputs (CPU, same seeds as below), max-normalised:
#   sequential: output 2.5e-7, worst parameter gradient 3.0e-6
#   reversible: output 2.6e-7, worst parameter gradient 3.4e-6
# The bound is 10x the larger figure of each kind, a margin for the
# reordered sums carried through the downstream layers.
MODEL_OUT_BOUND = 10 * 2.6e-7
MODEL_GRAD_BOUND = 10 * 3.4e-6


@needs_gpu
@pytest.mark.parametrize('reversible', [False, True])
def test_model_gated_norm_vs_eager(reversible, monkeypatch):
    from se3_transformer_amd import SE3Transformer
    cnt = _Counter(monkeypatch)
    torch.manual_seed(0)
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, num_neighbors=4,
                           norm_gated_scale=True, norm_out=True,
                           reversible=reversible)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('w_gate'):
                p.copy_(torch.randn(p.shape, generator=g)
                        / math.sqrt(p.shape[0]))
    model = model.to('cuda')
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(1, 16, 32, generator=g).cuda()
    coors = torch.randn(1, 16, 3, generator=g).cuda()
    mask = torch.ones(1, 16, dtype=torch.bool, device='cuda')

    def run():
        model.zero_grad()
        out = model(feats, coors, mask, return_type=0)
        out.pow(2).mean().backward()
        return out.detach(), {n: p.grad.clone()
                              for n, p in model.named_parameters()
                              if p.grad is not None}

    with switches(SE3_EAGER_NORM='1'):
        ref, gref = run()
    assert cnt.total == 0
    out, grads = run()
    assert cnt.n['norm_se3_gated'] > 0, 'the model never reached the kernels'

    picked = [n for n in grads
              if n.endswith('prenorm.transform.1.w_gate')
              or n.endswith('prenorm.transform.0.w_gate')
              or n.startswith('norm.transform.0.')
              or n.endswith('to_q.weights.1')
              or n == 'conv_in.self_interact.weights.0']
    assert any('prenorm' in n for n in picked)
    assert 'norm.transform.0.w_gate' in picked
    e_out = _rel_err(out, ref)
    print(f'model reversible={reversible}: out {e_out}')
    for n in picked:
        print(f'  {n}: {_rel_err(grads[n], gref[n])}')
    assert e_out < MODEL_OUT_BOUND, e_out
    for n in picked:
        e = _rel_err(grads[n], gref[n])
        assert e < MODEL_GRAD_BOUND, (n, e)


# ---- 7. hipGraph -----------------------------------------------------------

@needs_gpu
def test_gated_norm_graph_capture():
    torch.manual_seed(7)
    shape = (1, 16, 64, 3)
    mod, key = _make(64, 3, 'gelu', gated=True)
    w = _param(mod, key)
    st = torch.randn(shape, device='cuda', requires_grad=True)

    def step():
        st.grad = None       # captured grads live in the graph's own pool
        w.grad = None
        out = mod({key: st})[key]
        out.pow(2).mean().backward()
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sout = step()

    fresh = _feats(shape)
    with torch.no_grad():
        st.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    out_g, dt_g, dw_g = sout.detach().clone(), st.grad.clone(), w.grad.clone()

    out, dt, dw = _run(mod, key, fresh)
    assert _rel_err(out_g, out) < 1e-5
    assert _rel_err(dt_g, dt) < 1e-4
    assert _rel_err(dw_g, dw) < 1e-4
