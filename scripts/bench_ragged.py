"""Time models and single degree pairs whose channel counts are no multiple
of the pairconv tile (8 mo x 32 urows).

Usage (GPU box):  python scripts/bench_ragged.py --label NAME --out FILE.json

Under autocast (bf16), forward + backward:
  * the step of three models at n = 128, k = 8: dim=16 (2 degrees), the
    reference README's fiber-dict example, and dim=48 (3 degrees);
  * one PairwiseConv (d_in, d_out) = (0, 1), so F = 1, O = 3 and
    miF = channels in, at (mo, miF) in {(1, 4), (8, 16), (24, 48), (48, 144)}
    and E = 9216 edges, through apply_fused (radial trunk, ubuild, pairconv).

The script asks nothing of the package but its public classes, so the same
file times a checkout from before the kernels took these shapes (where they
run the eager chunked path) and one after. Each figure is the median of
--repeats windows of --iters steps after --warmup steps, a device
synchronise closing every window; min and max are kept as the spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from se3_transformer_amd import SE3Transformer
from se3_transformer_amd.models.core import PairwiseConv

PAIRS = [(1, 4), (8, 16), (24, 48), (48, 144)]


def windows(step, warmup, iters, repeats):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / iters * 1000)
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms),
            'max_ms': max(ms), 'windows': ms}


def models(n):
    dev = 'cuda'

    def feats(dim):
        return (torch.randn(1, n, dim, device=dev),
                torch.randn(1, n, 3, device=dev),
                torch.ones(1, n, dtype=torch.bool, device=dev))

    yield ('dim16_deg2',
           SE3Transformer(dim=16, heads=2, dim_head=8, depth=1, num_degrees=2,
                          num_neighbors=8),
           feats(16), dict(return_type=0))
    yield ('readme_fiber',
           SE3Transformer(num_tokens=28, dim=64, num_edge_tokens=4, edge_dim=16,
                          depth=2, input_degrees=1, num_degrees=3,
                          output_degrees=1,
                          hidden_fiber_dict={0: 16, 1: 8, 2: 4},
                          out_fiber_dict={0: 16, 1: 1}, reduce_dim_out=False,
                          num_neighbors=8),
           (torch.randint(0, 28, (1, n), device=dev),
            torch.randn(1, n, 3, device=dev),
            torch.ones(1, n, dtype=torch.bool, device=dev)),
           dict(edges=torch.randint(0, 4, (1, n, n), device=dev)))
    yield ('dim48_deg3',
           SE3Transformer(dim=48, heads=2, dim_head=24, depth=1, num_degrees=3,
                          num_neighbors=8),
           feats(48), dict(return_type=0))


def flat(out):
    if isinstance(out, dict):
        return torch.cat([out[k].float().reshape(-1) for k in sorted(out)])
    return out.float().reshape(-1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--label', required=True)
    p.add_argument('--out', required=True)
    p.add_argument('--n', type=int, default=128)
    p.add_argument('--E', type=int, default=9216)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--repeats', type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_ragged.py measures on the GPU: none found')
    torch.manual_seed(0)
    res = {'label': args.label, 'n': args.n, 'E': args.E, 'models': {},
           'pairs': {}}

    for name, model, inputs, kw in models(args.n):
        model = model.cuda()

        def step():
            model.zero_grad(set_to_none=True)
            with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
                out = model(*inputs, **kw)
            flat(out).pow(2).mean().backward()

        res['models'][name] = windows(step, args.warmup, args.iters,
                                      args.repeats)
        print(args.label, name, res['models'][name], flush=True)
        del model

    E = args.E
    for mo, mi in PAIRS:
        pc = PairwiseConv(0, mi, 1, mo, edge_dim=0).cuda()
        ef = torch.randn(E, 1, device='cuda')
        basis = {(0, 1): torch.randn(E, 3, 1, 1, device='cuda')}
        x = torch.randn(E, mi, 1, device='cuda', requires_grad=True)

        def step():
            pc.zero_grad(set_to_none=True)
            x.grad = None
            with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
                out = pc.apply_fused(ef, basis, x)
            out.float().pow(2).mean().backward()

        key = f'mo{mo}_miF{mi}'
        res['pairs'][key] = windows(step, args.warmup, args.iters,
                                    args.repeats)
        print(args.label, key, res['pairs'][key], flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
