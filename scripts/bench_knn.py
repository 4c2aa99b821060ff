"""Time the graph-build section of SE3Transformer.forward: the kNN kernel
against SE3_EAGER_KNN=1 (the dense build it replaces), and one train step
of a radius-graph model with and without SE3_COMPACT_NEIGHBORS=1.

Usage (GPU box):  python scripts/bench_knn.py [--out profiles/knn_any_k.md]

Graph build: b=1, fp32 coordinates, (n, k) = (1024, 64), (1024, 128),
(1024, 1023), (4096, 4095); k = n-1 is the default num_neighbors=inf. The
section is timed inside the real forward: the model runs up to the call of
the basis, the first thing after the graph build, and stops there. The two
paths alternate in one process; each window is timed with device events
after warm-up and sized to about --window seconds. Peak memory is
max_memory_allocated over one call, above what was allocated before it.

The eager build is what ran before the kernel took k > 64, so
`kernel_ms <= eager_ms` is the expectation, not a promise: a slower point
is reported as such.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from se3_transformer_amd import SE3Transformer
from se3_transformer_amd.models import transformer as tr
from se3_transformer_amd.ops import fused

GRAPH_CASES = ((1024, 64), (1024, 128), (1024, 1023), (4096, 4095))


class _GraphBuilt(Exception):
    pass


def _stop(*a, **kw):
    raise _GraphBuilt


def window_ms(step, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def with_env(step, **env):
    def wrapped():
        for k, v in env.items():
            os.environ[k] = v
        try:
            step()
        finally:
            for k in env:
                os.environ.pop(k, None)
    return wrapped


def alternate(steps, window, rounds, warmup=5):
    """steps: name -> callable. Median ms of `rounds` alternating windows."""
    iters = {}
    for name, step in steps.items():
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        ms = window_ms(step, 5)
        iters[name] = max(5, int(window * 1e3 / ms) + 1)
    times = {name: [] for name in steps}
    for _ in range(rounds):
        for name, step in steps.items():
            times[name].append(window_ms(step, iters[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max((max(v) - min(v)) / med[k] for k, v in times.items())
    return med, spread, iters


def peak_mib(step):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_graph_build(n, k, args):
    torch.manual_seed(0)
    kw = {} if k == n - 1 else {'num_neighbors': k}
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, **kw).cuda()
    feats = torch.randn(1, n, 32, device='cuda')
    coors = torch.randn(1, n, 3, device='cuda') * 1.5
    mask = torch.ones(1, n, dtype=torch.bool, device='cuda')
    assert fused.knn_ok(n, k)

    def build():
        try:
            with torch.no_grad():
                model(feats, coors, mask, return_type=0)
        except _GraphBuilt:
            return
        raise AssertionError('forward did not reach the basis')

    calls = []
    real = fused._load_ext().knn_graph
    steps = {'kernel': build, 'eager': with_env(build, SE3_EAGER_KNN='1')}
    real_basis = tr.get_basis_packed
    tr.get_basis_packed = _stop
    try:
        fused._load_ext().knn_graph = lambda *a: (calls.append(1), real(*a))[1]
        steps['kernel']()
        assert calls, 'the kNN kernel was not called'
        steps['eager']()
        assert len(calls) == 1, 'SE3_EAGER_KNN=1 still called the kernel'
        fused._load_ext().knn_graph = real
        med, spread, iters = alternate(steps, args.window, args.rounds)
        peak = {name: peak_mib(step) for name, step in steps.items()}
    finally:
        fused._load_ext().knn_graph = real
        tr.get_basis_packed = real_basis
    L = min(k, -(-n // 64))
    return {'n': n, 'k': k, 'L': L, 'lds': fused.knn_lds_bytes(n, k),
            'winners': min(k, n - 1), 'med': med, 'spread': spread,
            'iters': iters, 'peak': peak}


def bench_compaction(n, args):
    torch.manual_seed(5)
    model = SE3Transformer(dim=32, heads=2, dim_head=16, depth=1,
                           num_degrees=2, valid_radius=3.0).cuda()
    g = torch.Generator().manual_seed(22)
    feats = torch.randn(2, n, 32, generator=g).cuda()
    coors = (torch.randn(2, n, 3, generator=g) * 1.5).cuda()
    mask = (torch.rand(2, n, generator=g) > 0.1).cuda()
    seen = []
    model.conv_in.register_forward_pre_hook(
        lambda mod, a: seen.append(a[1][0].shape[2]))

    def step():
        model.zero_grad(set_to_none=True)
        out = model(feats, coors, mask, return_type=0)
        out.pow(2).mean().backward()

    steps = {'full': step,
             'compact': with_env(step, SE3_COMPACT_NEIGHBORS='1')}
    k_seen = {}
    for name, s in steps.items():
        s()
        k_seen[name] = seen[-1]
    med, spread, iters = alternate(steps, args.window, args.rounds, warmup=3)
    peak = {name: peak_mib(s) for name, s in steps.items()}
    return {'n': n, 'k_seen': k_seen, 'med': med, 'spread': spread,
            'iters': iters, 'peak': peak}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--window', type=float, default=1.0,
                   help='seconds of work per timed window')
    p.add_argument('--rounds', type=int, default=3,
                   help='alternating windows per case')
    p.add_argument('--compact-n', type=int, default=256)
    p.add_argument('--out', default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        'profiles', 'knn_any_k.md'))
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit('bench_knn.py needs a GPU')
    fused.require_ext()

    lines = [
        '# kNN kernel at any k: graph build against the eager build',
        '',
        f'`python scripts/bench_knn.py` on {torch.cuda.get_device_name(0)}, '
        f'torch {torch.__version__}. Device events around alternating '
        f'windows of about {args.window:g} s, median of {args.rounds}; '
        'spread = (max - min) / median over the windows of a path, the '
        'larger of the two paths. Peak = max_memory_allocated over one '
        'call above the level before it.',
        '',
        '## Graph-build section of `forward` (b=1, fp32, no grad)',
        '',
        'kernel = `csrc/knn.hip`; eager = `SE3_EAGER_KNN=1`, the dense '
        '(b,n,n,3) build with masked `topk` and gathers. Winners = slots '
        'the merge fills per wave (one wave per query row); a merge round '
        'takes every list head below the smallest second entry, about ten '
        'winners on random points.',
        '',
        '| n | k | L | LDS B/block | winners/wave | kernel ms | eager ms '
        '| eager/kernel | spread | kernel peak MiB | eager peak MiB |',
        '|---|---|---|---|---|---|---|---|---|---|---|',
    ]
    for n, k in GRAPH_CASES:
        r = bench_graph_build(n, k, args)
        m, pk = r['med'], r['peak']
        row = (f"| {n} | {k} | {r['L']} | {r['lds']} | {r['winners']} "
               f"| {m['kernel']:.3f} | {m['eager']:.3f} "
               f"| {m['eager'] / m['kernel']:.2f} | {r['spread']:.1%} "
               f"| {pk['kernel']:.1f} | {pk['eager']:.1f} |")
        print(row, flush=True)
        lines.append(row)

    c = bench_compaction(args.compact_n, args)
    m, pk, ks = c['med'], c['peak'], c['k_seen']
    lines += [
        '',
        f"## One train step, radius graph, n={c['n']} (b=2, fp32)",
        '',
        'dim=32, heads=2, dim_head=16, depth=1, num_degrees=2, '
        'valid_radius=3.0, num_neighbors at its default, coordinates '
        'randn * 1.5, ~10% of the nodes masked; forward + backward.',
        '',
        '| SE3_COMPACT_NEIGHBORS | neighbour axis seen by the trunk | '
        'ms/step | peak MiB |',
        '|---|---|---|---|',
        f"| unset | {ks['full']} | {m['full']:.2f} | {pk['full']:.1f} |",
        f"| 1 | {ks['compact']} (k_eff) | {m['compact']:.2f} "
        f"| {pk['compact']:.1f} |",
        '',
        f"Spread {c['spread']:.1%}.",
        '',
    ]
    print('\n'.join(lines[-9:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines))
    print('wrote', args.out)


if __name__ == '__main__':
    main()
