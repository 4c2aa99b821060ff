"""kNN kernel past k = 64 (`pytest -m gpu`): direct kernel calls against a
dense torch oracle, the default (`num_neighbors=inf`) and radius graphs at
model level against the eager graph build, differentiable coordinates
against a float64 oracle, and the SE3_COMPACT_NEIGHBORS knob.

Slots of a kernel row come in two kinds. The first c = min(k, candidates of
the row) are *selected*: a real neighbour with its real geometry, masked or
not. The rest are *fabricated*: no candidate was left (causal rows, rows
thinned by `allow`), they carry a placeholder index, zero geometry and
mask 0. The candidate count comes from the oracle, not from the kernel.
"""
import copy

import pytest
import torch

from se3_transformer_amd import SE3Transformer
from se3_transformer_amd.ops import fused

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')]

INF = float('inf')
NO_RADIUS = 1e5


# ------------------------------------------------------------ direct kernel

def oracle(coors, k, radius, nmask, allow, sparse, causal):
    """The documented selection rules on a dense (b,n,n) squared-distance
    matrix: returns the effective squared distances (inf = no candidate),
    their k smallest per row, and the dense output mask."""
    b, n, _ = coors.shape
    dev = coors.device
    diff = coors[:, :, None] - coors[:, None]
    d2 = (diff * diff).sum(-1)
    ar = torch.arange(n, device=dev)
    cand = (ar[:, None] != ar[None, :]).expand(b, n, n).clone()   # self excluded
    sp = sparse.bool() if sparse is not None else torch.zeros_like(cand)
    if allow is not None:
        cand &= allow.bool() | sp            # sparse is exempt from `allow`
    if causal:
        cand &= (ar[None, :] < ar[:, None])  # overrides everything
    eff = torch.where(sp, torch.zeros_like(d2), d2)
    eff = torch.where(cand, eff, torch.full_like(d2, INF))
    top = eff.topk(k, dim=-1, largest=False).values
    ok = cand & (sp | (d2.sqrt() <= radius))  # sparse is exempt from the radius
    if nmask is not None:                     # node mask: output mask only
        ok &= nmask.bool()[:, :, None] & nmask.bool()[:, None, :]
    return eff, top, ok


def run_kernel(coors, k, radius, nmask, allow, sparse, causal):
    ext = fused._load_ext()
    b, n, _ = coors.shape
    dev = coors.device
    idx = torch.full((b, n, k), -7, dtype=torch.int64, device=dev)
    dist = torch.full((b, n, k), -7., device=dev)
    rel = torch.full((b, n, k, 3), -7., device=dev)
    m = torch.full((b, n, k), 7, dtype=torch.uint8, device=dev)
    e = torch.empty(0, dtype=torch.uint8, device=dev)
    ext.knn_graph(coors.contiguous(),
                  nmask.to(torch.uint8).contiguous() if nmask is not None else e,
                  allow.to(torch.uint8).contiguous() if allow is not None else e,
                  sparse.to(torch.uint8).contiguous() if sparse is not None else e,
                  idx, dist, rel, m, k, float(radius), causal)
    torch.cuda.synchronize()
    return idx, dist, rel, m


def make_case(name):
    """(coors, k, radius, nmask, allow, sparse, causal) built on the CPU from
    a fixed seed; b = 2 and randn * 1.5 coordinates unless stated."""
    g = torch.Generator().manual_seed(21)

    def pts(b, n):
        return torch.randn(b, n, 3, generator=g) * 1.5

    nmask = allow = sparse = None
    radius, causal = NO_RADIUS, False
    if name == 'first_past_64':        # L = 2; pass 2 of the output loop: 1 lane
        coors, k = pts(2, 66), 65
    elif name == 'cutoff_past_64':     # k < candidates, > 64 merge rounds
        coors, k = pts(2, 200), 65
    elif name == 'radius_all':         # k = n-1 with a radius and a node mask
        coors, k, radius = pts(2, 150), 149, 3.0
        nmask = torch.rand(2, 150, generator=g) > 0.1
    elif name == 'causal':             # rows short of k, row 0 empty: the fill
        coors, k, causal = pts(2, 130), 129, True
    elif name == 'allow_sparse':       # exclusion and priority beyond 64
        coors, k = pts(2, 150), 100
        allow = torch.rand(2, 150, 150, generator=g) < 0.7
        ar = torch.arange(150)
        sparse = ((ar[:, None] - ar[None, :]).abs() == 1).expand(2, 150, 150)
    elif name == 'sel_past_1024':      # 18 passes of the output loop
        coors, k = pts(1, 1100), 1099
    else:
        raise KeyError(name)
    cu = lambda t: t.cuda() if t is not None else None
    return cu(coors), k, radius, cu(nmask), cu(allow), cu(sparse), causal


CASES = ('first_past_64', 'cutoff_past_64', 'radius_all', 'causal',
         'allow_sparse', 'sel_past_1024')


@pytest.mark.parametrize('name', CASES)
def test_kernel_vs_dense_oracle(name):
    coors, k, radius, nmask, allow, sparse, causal = make_case(name)
    b, n, _ = coors.shape
    eff, top, ok = oracle(coors, k, radius, nmask, allow, sparse, causal)
    idx, dist, rel, m = run_kernel(coors, k, radius, nmask, allow, sparse, causal)

    assert ((idx >= 0) & (idx < n)).all(), 'index out of range'
    assert ((m == 0) | (m == 1)).all()
    valid = m.bool()
    ncand = torch.isfinite(eff).sum(-1).clamp(max=k)             # (b,n)
    slot = torch.arange(k, device=coors.device)
    selected = slot.view(1, 1, k) < ncand.unsqueeze(-1)
    assert not (valid & ~selected).any(), 'a fabricated slot is marked valid'

    # 1. self-consistency of the selected (and with them all valid) slots
    rows = torch.arange(n, device=coors.device).view(1, n, 1).expand(b, n, k)
    assert (idx != rows)[selected].all()
    nbr = torch.gather(coors.unsqueeze(1).expand(b, n, n, 3), 2,
                       idx.unsqueeze(-1).expand(b, n, k, 3))
    want_rel = coors.unsqueeze(2) - nbr
    assert torch.equal(rel[selected], want_rel[selected])
    torch.testing.assert_close(dist[selected], rel.norm(dim=-1)[selected],
                               rtol=1e-6, atol=0)

    # 2. no duplicates among a row's selected slots; fabricated slots are zero
    probe = torch.where(selected, idx, n + slot.view(1, 1, k).expand(b, n, k))
    srt = probe.sort(dim=-1).values
    assert (srt[..., 1:] != srt[..., :-1]).all(), 'duplicate neighbour'
    assert (dist[~selected] == 0).all() and (rel[~selected] == 0).all()

    # 3. selection: sorted effective distances against the oracle's top-k
    got = torch.gather(eff, 2, idx)
    got = torch.where(selected, got, torch.full_like(got, INF))
    torch.testing.assert_close(got.sort(dim=-1).values, top, rtol=1e-6, atol=0)

    # 4. mask, at the kernel's own indices
    assert torch.equal(valid, torch.gather(ok, 2, idx) & selected)

    per_row = valid.sum(-1)
    print(f'{name}: n={n} k={k} candidates/row {int(ncand.min())}..'
          f'{int(ncand.max())} valid/row {int(per_row.min())}..'
          f'{int(per_row.max())}')
    if name == 'radius_all':
        # 5. not vacuous: some row has between 1 and 148 valid slots
        assert ((per_row >= 1) & (per_row <= 148)).any()
    if name == 'causal':
        assert not valid[:, 0].any() and int(ncand.min()) == 0


def test_lds_budget_is_enforced():
    """A launch past knn_max_lds_bytes() is refused by name, not attempted."""
    ext = fused._load_ext()
    assert ext.knn_max_lds_bytes() == fused.KNN_MAX_LDS
    n, k = 6000, 5999
    assert not fused.knn_ok(n, k)
    coors = torch.zeros(1, n, 3, device='cuda')
    e = torch.empty(0, dtype=torch.uint8, device='cuda')
    idx = torch.empty(1, n, k, dtype=torch.int64, device='cuda')
    dist = torch.empty(1, n, k, device='cuda')
    rel = torch.empty(1, n, k, 3, device='cuda')
    m = torch.empty(1, n, k, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match=r'n=6000 k=5999.*65536'):
        ext.knn_graph(coors, e, e, e, idx, dist, rel, m, k, 1.0, False)


# -------------------------------------------------------------------- model

N = 80


def make_model(**kw):
    torch.manual_seed(5)
    return SE3Transformer(dim=32, heads=2, dim_head=16, depth=1, num_degrees=2,
                          valid_radius=3.0, **kw).cuda()


def make_inputs(seed=22, b=2, n=N, dim=32):
    """On the CPU, seed 22, n=80, randn * 1.5 and radius 3.0 give in-radius
    counts (self excluded, node mask ignored) of 1 to 62 of 79 per row."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(b, n, dim, generator=g)
    coors = torch.randn(b, n, 3, generator=g) * 1.5
    mask = torch.rand(b, n, generator=g) > 0.1
    cot = torch.randn(b, n, dim, 3, generator=g)
    return feats.cuda(), coors.cuda(), mask.cuda(), cot.cuda()


def set_env(monkeypatch, **names):
    for v in ('SE3_EAGER_KNN', 'SE3_COMPACT_NEIGHBORS'):
        if names.get(v):
            monkeypatch.setenv(v, '1')
        else:
            monkeypatch.delenv(v, raising=False)


def spy(monkeypatch, calls, obj, name):
    real = getattr(obj, name)

    def wrapped(*a, **kw):
        calls[name] = calls.get(name, 0) + 1
        return real(*a, **kw)
    monkeypatch.setattr(obj, name, wrapped, raising=True)


def test_default_neighbors_take_the_kernel(monkeypatch):
    """num_neighbors left at inf, k_total = n-1 = 79: the kernel builds the
    graph, the dense build is never entered, and the output matches the
    eager build within the 1e-4 of the existing kNN parity tests."""
    from se3_transformer_amd.models import transformer as tr
    model = make_model()
    feats, coors, mask, _ = make_inputs()
    with torch.no_grad():
        set_env(monkeypatch, SE3_EAGER_KNN=True)
        ref = model(feats, coors, mask, return_type=0)

        calls = {}
        spy(monkeypatch, calls, fused._load_ext(), 'knn_graph')
        spy(monkeypatch, calls, tr, '_remove_self')
        spy(monkeypatch, calls, tr, '_off_diag_indices')
        set_env(monkeypatch)
        out = model(feats, coors, mask, return_type=0)
    assert calls.get('knn_graph', 0) == 1, 'the kNN kernel was not called'
    assert calls.get('_remove_self', 0) == 0
    assert calls.get('_off_diag_indices', 0) == 0
    err = (out - ref).abs().max().item()
    print(f'default neighbours, n={N}: max-abs vs eager build {err:.3e}')
    assert torch.isfinite(out).all()
    assert err < 1e-4


def rel_err(a, ref):
    return ((a.double() - ref.double()).abs().max()
            / ref.double().abs().max()).item()


def run_grad(model, inputs, dtype=torch.float32):
    feats, coors, mask, cot = inputs
    model.zero_grad(set_to_none=True)
    c = coors.to(dtype).clone().requires_grad_()
    out = model(feats.to(dtype), c, mask, return_type=1)
    (out * cot.to(dtype)).sum().backward()
    pgrad = torch.cat([p.grad.reshape(-1).double() for p in model.parameters()
                       if p.grad is not None])
    return out.detach(), c.grad, pgrad


def test_differentiable_coors_default_neighbors(monkeypatch):
    """differentiable_coors at k = n-1: output, coors.grad and parameter
    gradients of the kernel path against the same weights in float64 eager,
    bound err_new <= max(8 * err_eager, 2e-5) with err_eager the error of
    the SE3_EAGER_KNN=1 fp32 path against the same oracle."""
    model = make_model(output_degrees=2, differentiable_coors=True)
    inputs = make_inputs()
    calls = {}
    spy(monkeypatch, calls, fused._load_ext(), 'knn_graph')

    set_env(monkeypatch)
    new = run_grad(model, inputs)
    assert calls.get('knn_graph', 0) == 1, 'the kNN kernel was not called'
    set_env(monkeypatch, SE3_EAGER_KNN=True)
    eager = run_grad(model, inputs)
    ref = run_grad(copy.deepcopy(model).double(), inputs, dtype=torch.float64)
    assert calls['knn_graph'] == 1

    assert torch.isfinite(new[1]).all()
    for name, a, p, r in zip(('out', 'coors.grad', 'param grads'),
                             new, eager, ref):
        assert a.shape == r.shape
        err_new, err_eager = rel_err(a, r), rel_err(p, r)
        print(f'diff coors k=n-1 {name}: err_new={err_new:.3e} '
              f'err_eager={err_eager:.3e}')
        assert err_new <= max(8 * err_eager, 2e-5), name


def watch_k(model, seen):
    return model.conv_in.register_forward_pre_hook(
        lambda mod, args: seen.append(args[1][0].shape[2]))


def test_compaction_cuts_trailing_columns(monkeypatch):
    """SE3_COMPACT_NEIGHBORS=1 hands the trunk fewer than n-1 columns (the
    inputs' largest in-radius count is 62 of 79, see make_inputs), unset it
    hands all n-1; the outputs agree within 1e-4 (summation order only)."""
    model = make_model()
    feats, coors, mask, _ = make_inputs()
    seen = []
    watch_k(model, seen)
    with torch.no_grad():
        set_env(monkeypatch)
        full = model(feats, coors, mask, return_type=0)
        set_env(monkeypatch, SE3_COMPACT_NEIGHBORS=True)
        cut = model(feats, coors, mask, return_type=0)
        set_env(monkeypatch, SE3_COMPACT_NEIGHBORS=True, SE3_EAGER_KNN=True)
        model(feats, coors, mask, return_type=0)
    print(f'compaction: neighbour axis {seen}')
    assert seen[0] == N - 1
    assert 1 <= seen[1] < N - 1
    assert seen[1] <= 62
    assert seen[2] == N - 1, 'the eager build must not be compacted'
    err = (cut - full).abs().max().item()
    print(f'compaction: max-abs vs uncompacted {err:.3e}')
    assert err < 1e-4


def test_compaction_is_skipped_under_graph_capture(monkeypatch):
    """With the knob set a forward still captures into a hipGraph and
    replays: the host read is skipped while capturing, so the captured
    forward sees the full n-1 columns."""
    model = make_model()
    feats, coors, mask, _ = make_inputs()
    seen = []
    watch_k(model, seen)
    set_env(monkeypatch, SE3_COMPACT_NEIGHBORS=True)
    with torch.no_grad():
        for _ in range(2):                      # allocator warm-up
            warm = model(feats, coors, mask, return_type=0)
        torch.cuda.synchronize()
        assert seen[-1] < N - 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = model(feats, coors, mask, return_type=0)
        assert seen[-1] == N - 1
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert (out - warm).abs().max().item() < 1e-4
