"""Kernel-level GPU tests of csrc/attn2.hip against the f64 reference of
tests/attn2_ref.py, on the cases of tests/attn2_cases.py, plus the gates
that route a module to the kernel or away from it.

Bands (attn2_cases.py): margin x max(e32, 1e-7), never above the case's
cap, where e32 is what the same formula loses when torch evaluates it in
fp32 on the device. The margins are twice the largest kernel_err / e32
measured over all cases; the table is in profiles/attn2_parity.md.
test_attn2_reference.py proves without a GPU that each case separates a
broken kernel from a right one by at least 10x these bands.
"""
import copy

import pytest
import torch

import attn2_cases as C
import attn2_ref as A

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')

TENSORS = ('out', 'dq', 'dk', 'dv')


def _rel_err(a, b):
    denom = b.abs().max().clamp(min=1e-6)
    return ((a - b).abs().max() / denom).item()


def _to_dev(inp):
    return {k_: (t.cuda() if torch.is_tensor(t) else t)
            for k_, t in inp.items()}


def run_kernel(inp):
    """One forward + backward of the kernel on device inputs. Returns
    (out, dq, dk, dv) as the wrapper hands them out. Checks on the way that
    the rotary tables get no gradient and are left as they were."""
    from se3_transformer_amd.ops import fused
    q, k, v = (inp[x].detach().clone().requires_grad_(True)
               for x in ('q', 'k', 'v'))
    qf, kf = inp['qf'], inp['kf']
    tables = [t.detach().clone().requires_grad_(True) if t is not None
              else None for t in (qf, kf)]
    out = fused.fused_attention(q, k, v, inp['mask'], inp['n'], inp['heads'],
                                inp['scale'], inp['kv_one'],
                                qf=tables[0], kf=tables[1])
    out.backward(inp['g'])
    for t, orig in zip(tables, (qf, kf)):
        if t is not None:
            assert t.grad is None, 'rotary table received a gradient'
            assert torch.equal(t.detach(), orig), 'rotary table was modified'
    return out.detach(), q.grad, k.grad, v.grad


def measure(case, kv_one, dtype):
    """Kernel and fp32-torch errors against the f64 reference, per tensor:
    {'out': (kernel_err, e32, rerun_diff), ...}, plus the raw results."""
    inp = _to_dev(C.make_inputs(case, kv_one, dtype))
    args = (inp['q'], inp['k'], inp['v'], inp['mask'], inp['n'],
            inp['heads'], inp['scale'], kv_one, inp['qf'], inp['kf'],
            inp['g'])
    ref = A.reference_with_grads(*args, dtype=torch.float64)
    y32 = A.reference_with_grads(*args, dtype=torch.float32)
    got = run_kernel(inp)
    assert got[0].dtype == torch.float32
    assert all(t.dtype == dtype for t in got[1:])
    # shared-KV gradients are accumulated with atomics: run those twice
    again = run_kernel(inp) if kv_one else got
    errs = {}
    for name, r, y, a, b in zip(TENSORS, ref, y32, got, again):
        errs[name] = (max(_rel_err(a.double(), r), _rel_err(b.double(), r)),
                      _rel_err(y.double(), r),
                      _rel_err(a.double(), b.double()))
    return errs, inp, ref, got


def band(case, dtype, name, e32):
    cap_fwd, cap_grad = C.caps(case)
    m_fwd, m_grad = C.margins(case)
    if name == 'out':
        return min(m_fwd * max(e32, C.E32_FLOOR), cap_fwd)
    fp32_band = min(m_grad * max(e32, C.E32_FLOOR), cap_grad)
    return fp32_band + (C.BF16_ULP if dtype == torch.bfloat16 else 0.)


@needs_gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16],
                         ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kv_one', [False, True], ids=['perhead', 'kvone'])
@pytest.mark.parametrize('case', C.CASES, ids=lambda c: c.id)
def test_attn2_kernel_vs_f64_reference(case, kv_one, dtype):
    errs, inp, ref, got = measure(case, kv_one, dtype)
    bad = []
    for name in TENSORS:
        kerr, e32, rerun = errs[name]
        lim = band(case, dtype, name, e32)
        print(f'attn2-parity {case.id} kv_one={int(kv_one)} '
              f'{"bf16" if dtype == torch.bfloat16 else "fp32"} {name} '
              f'kernel={kerr:.3e} e32={e32:.3e} ratio={kerr / max(e32, C.E32_FLOOR):.2f} '
              f'rerun={rerun:.3e} band={lim:.3e}')
        if not kerr <= lim:
            bad.append(f'{name}: {kerr:.3e} > band {lim:.3e} (e32 {e32:.3e})')
        if not rerun <= lim:
            bad.append(f'{name}: run-to-run {rerun:.3e} > band {lim:.3e}')
    assert not bad, '; '.join(bad)

    mask = inp['mask']
    if mask is not None and not kv_one:
        # per-row key tensors: a masked key's dk is written by one row only
        # and must be exactly zero; so must dq and dk of an all-masked row
        mrow = (mask != 0)[:, None].expand(case.b, case.heads, case.n, case.J)
        mrow = mrow.reshape(case.R, case.J)
        _, dq, dk, _ = got
        if not mrow.all():
            assert dk[~mrow].abs().max().item() == 0
        dead = ~mrow.any(-1)
        if dead.any():
            assert dq[dead].abs().max().item() == 0
    if case.mask in ('full_mid', 'full_last'):
        # the semantics spelled out: mean of v, dv_j = g / J
        mrow = (mask != 0)[:, None].expand(case.b, case.heads, case.n, case.J)
        dead = ~mrow.reshape(case.R, case.J).any(-1)
        assert dead.any()
        if not kv_one:
            v32 = inp['v'].float()
            assert _rel_err(got[0][dead], v32[dead].mean(1)) < 1e-5
            want = (inp['g'][dead] / case.J)[:, None].expand(-1, case.J, -1)
            tol = 1e-6 + (C.BF16_ULP if dtype == torch.bfloat16 else 0.)
            assert _rel_err(got[3][dead].float(), want) < tol


# ---- gates -------------------------------------------------------------------

@needs_gpu
def test_attn_kernel_gate_edges(monkeypatch):
    from se3_transformer_amd.models.attention import _attn_kernel_ok
    monkeypatch.delenv('SE3_ATTN_MAX_J', raising=False)
    monkeypatch.delenv('SE3_EAGER_ATTN', raising=False)
    q32 = torch.empty(1, device='cuda')
    assert _attn_kernel_ok(q32, 9, 448)
    assert not _attn_kernel_ok(q32, 9, 449)
    assert _attn_kernel_ok(q32.bfloat16(), 9, 448)
    assert not _attn_kernel_ok(q32.double(), 9, 64)
    assert not _attn_kernel_ok(q32.half(), 9, 64)
    assert not _attn_kernel_ok(q32.cpu(), 9, 64)
    monkeypatch.setenv('SE3_ATTN_MAX_J', '9')
    assert _attn_kernel_ok(q32, 9, 64)
    assert not _attn_kernel_ok(q32, 10, 64)
    monkeypatch.delenv('SE3_ATTN_MAX_J')
    monkeypatch.setenv('SE3_EAGER_ATTN', '1')
    assert not _attn_kernel_ok(q32, 9, 64)


@needs_gpu
def test_rope_in_kernel_gate_edges(monkeypatch):
    from se3_transformer_amd.models.attention import _rope_in_kernel_ok
    monkeypatch.delenv('SE3_ATTN_MAX_J', raising=False)
    monkeypatch.delenv('SE3_EAGER_ATTN', raising=False)
    b, h, n, j = 1, 2, 3, 4

    def ok(rot, d, kpe_grad=False, j_tab=j, null=False, gfeats=None):
        q = torch.empty(b, h, n, d, 1, device='cuda')
        qpe = torch.zeros(b, n, rot, device='cuda')
        kpe = torch.zeros(b, n, j_tab, rot, device='cuda',
                          requires_grad=kpe_grad)
        return _rope_in_kernel_ok(q, j, qpe, kpe, null, gfeats)

    assert ok(64, 64)                   # every lane paired
    assert ok(64, 128)
    assert ok(2, 2)
    assert not ok(66, 66)               # more pairs than lanes
    assert not ok(66, 128)
    assert not ok(15, 16)               # odd
    assert not ok(16, 8)                # rot > dm
    assert not ok(16, 16, kpe_grad=True)
    assert not ok(16, 16, j_tab=j - 1)  # table does not cover the keys
    assert ok(16, 448, null=True,
              gfeats={'0': torch.zeros(b, 2, 5, 1, device='cuda')})
    assert not ok(16, 449)
    monkeypatch.setenv('SE3_ATTN_MAX_J', str(j + 2))
    assert ok(16, 16, null=True,
              gfeats={'0': torch.zeros(b, 1, 5, 1, device='cuda')})
    assert not ok(16, 16, null=True,    # prefix keys count towards J
                  gfeats={'0': torch.zeros(b, 2, 5, 1, device='cuda')})


class _Calls:
    """Records every call of ops.fused.fused_attention."""

    def __init__(self, monkeypatch):
        from se3_transformer_amd.ops import fused
        self.rope = []          # per call: were rotary tables passed?
        real = fused.fused_attention

        def counted(*a, **k):
            self.rope.append(k.get('qf') is not None)
            return real(*a, **k)
        monkeypatch.setattr(fused, 'fused_attention', counted)


def _small_module(klass, gen, global_dim=None):
    from se3_transformer_amd.models.fiber import Fiber
    # 8 channels: the convolutions stay on their fp32 path, so attention
    # is the only kernel between the fp32 and the f64 run
    attn = klass(Fiber([(0, 8), (1, 8)]), dim_head=4, heads=2,
                 attend_self=True, use_null_kv=True,
                 global_feats_dim=global_dim).double()
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=p.dtype) * 0.5)
    return attn


def _small_inputs(gen, b=2, n=8, kn=3, dim=8, rot=4, global_dim=None):
    f64 = dict(generator=gen, dtype=torch.float64)
    nbr_idx = torch.randint(0, n, (b, n, kn), generator=gen)
    nbr_mask = torch.rand(b, n, kn, generator=gen) > 0.3
    rel_dist = torch.rand(b, n, kn, **f64) * 3
    basis = {(di, do): torch.randn(b, n, kn, 2 * do + 1, 2 * di + 1,
                                   2 * min(di, do) + 1, **f64)
             for di in (0, 1) for do in (0, 1)}
    feats = {'0': torch.randn(b, n, dim, 1, **f64),
             '1': torch.randn(b, n, dim, 3, **f64)}
    pos_emb = (torch.randn(b, n, rot, **f64) * 2,
               torch.randn(b, n, kn + 1, rot, **f64) * 2)
    gfeats = None
    if global_dim is not None:
        gfeats = {'0': torch.randn(b, 2, global_dim, 1, **f64)}
    gout = {k_: torch.randn(t.shape, **f64) for k_, t in feats.items()}
    return dict(edge=(nbr_idx, nbr_mask, None), rel_dist=rel_dist,
                basis=basis, feats=feats, pos_emb=pos_emb, gfeats=gfeats,
                gout=gout)


def _cast(x, device, dtype):
    if isinstance(x, dict):
        return {k_: _cast(t, device, dtype) for k_, t in x.items()}
    if isinstance(x, tuple):
        return tuple(_cast(t, device, dtype) for t in x)
    if torch.is_tensor(x):
        x = x.detach().clone().to(device)
        return x.to(dtype) if x.is_floating_point() else x
    return x


def _run_module(attn, data, device, dtype, rope=True, kpe_grad=False):
    """out['0'], out['1'] and the feature gradients under the fixed
    upstream gradient, in f64 on the CPU for comparison."""
    mod = copy.deepcopy(attn).to(device, dtype)
    d = _cast(data, device, dtype)
    feats = {k_: t.requires_grad_(True) for k_, t in d['feats'].items()}
    pos_emb = None
    if rope:
        qpe, kpe = d['pos_emb']
        pos_emb = (qpe, kpe.requires_grad_(True) if kpe_grad else kpe)
    out = mod(feats, d['edge'], d['rel_dist'], d['basis'],
              global_feats=d['gfeats'], pos_emb=pos_emb)
    loss = sum((out[k_] * d['gout'][k_]).sum() for k_ in out)
    grads = torch.autograd.grad(loss, [feats['0'], feats['1']])
    return [t.detach().double().cpu()
            for t in (out['0'], out['1'], *grads)]


# the kernel-level caps at J <= 64: 1e-4 forward, 1e-3 gradients
MODULE_BANDS = (1e-4, 1e-4, 1e-3, 1e-3)


def _assert_close(res, ref, what):
    for name, lim, a, r in zip(('out0', 'out1', 'g0', 'g1'), MODULE_BANDS,
                               res, ref):
        err = _rel_err(a, r)
        assert err < lim, f'{what} {name}: {err:.3e}'


@needs_gpu
def test_attention_module_branches(monkeypatch):
    """One small AttentionSE3 (n = 8, three neighbours): which branch each
    gate setting takes, and that every branch agrees with the module run
    in f64."""
    from se3_transformer_amd.models.attention import AttentionSE3
    monkeypatch.delenv('SE3_ATTN_MAX_J', raising=False)
    monkeypatch.delenv('SE3_EAGER_ATTN', raising=False)
    gen = torch.Generator().manual_seed(21)
    attn = _small_module(AttentionSE3, gen)
    data = _small_inputs(gen)
    calls = _Calls(monkeypatch)

    ref = {r: _run_module(attn, data, 'cpu', torch.float64, rope=r)
           for r in (False, True)}
    assert calls.rope == []

    # f64 on the device: eager (1e-8 is the suite's f64-on-device bound)
    res = _run_module(attn, data, 'cuda', torch.float64)
    assert calls.rope == []
    for a, r in zip(res, ref[True]):
        assert _rel_err(a, r) < 1e-8

    # fp32: one kernel call per degree; rotary tables go in on degree 0
    res = _run_module(attn, data, 'cuda', torch.float32)
    assert calls.rope == [True, False]
    _assert_close(res, ref[True], 'rope in kernel')

    calls.rope.clear()
    res = _run_module(attn, data, 'cuda', torch.float32, rope=False)
    assert calls.rope == [False, False]
    _assert_close(res, ref[False], 'no rope')

    # tables that need grad: rotation stays eager, attention on the kernel
    calls.rope.clear()
    res = _run_module(attn, data, 'cuda', torch.float32, kpe_grad=True)
    assert calls.rope == [False, False]
    _assert_close(res, ref[True], 'eager rotation')

    # J = 3 neighbours + self + null = 5 keys
    calls.rope.clear()
    monkeypatch.setenv('SE3_ATTN_MAX_J', '5')
    res = _run_module(attn, data, 'cuda', torch.float32)
    assert calls.rope == [True, False]
    _assert_close(res, ref[True], 'J at the cap')
    calls.rope.clear()
    monkeypatch.setenv('SE3_ATTN_MAX_J', '4')
    res = _run_module(attn, data, 'cuda', torch.float32)
    assert calls.rope == []
    _assert_close(res, ref[True], 'J over the cap')


@needs_gpu
def test_one_headed_rotary_null_global(monkeypatch):
    """Shared-KV attention with rotary, a null key and global keys at once:
    three prefix keys, rope on the rest, atomic dk/dv. Against the module
    itself on the CPU in f64."""
    from se3_transformer_amd.models.attention import OneHeadedKVAttentionSE3
    monkeypatch.delenv('SE3_ATTN_MAX_J', raising=False)
    monkeypatch.delenv('SE3_EAGER_ATTN', raising=False)
    gen = torch.Generator().manual_seed(22)
    attn = _small_module(OneHeadedKVAttentionSE3, gen, global_dim=6)
    data = _small_inputs(gen, global_dim=6)
    calls = _Calls(monkeypatch)
    ref = _run_module(attn, data, 'cpu', torch.float64)
    res = _run_module(attn, data, 'cuda', torch.float32)
    assert calls.rope == [True, False]
    _assert_close(res, ref, 'one-headed rope+null+global')
