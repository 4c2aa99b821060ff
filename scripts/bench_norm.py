"""Time NormSE3 forward+backward, fused HIP path against SE3_EAGER_NORM=1.

Usage (GPU box):  python scripts/bench_norm.py [--out profiles/norm_variants.json]

The four variants {scale, gated} x {GELU, identity} at the model's own
shapes: b*n = 1024 nodes, C = 512 channels, degrees 0..3 in one module (one
step = forward + backward of all four degrees), fp32 and bf16 features.
The two paths alternate in one process; each window is timed with device
events after warm-up and sized to about --window seconds. The eager path is
what ran before the variants had kernels, so `fused_ms <= eager_ms` beyond
the run-to-run spread measured here is the acceptance line; the speed-up
itself is only recorded.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from torch import nn

from se3_transformer_amd.models.core import NormSE3
from se3_transformer_amd.models.fiber import Fiber
from se3_transformer_amd.ops import fused


def window_ms(step, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def make_step(mod, feats, douts, eager):
    def step():
        if eager:
            os.environ['SE3_EAGER_NORM'] = '1'
        try:
            out = mod(feats)
        finally:
            os.environ.pop('SE3_EAGER_NORM', None)
        torch.autograd.backward([out[k] for k in feats],
                                [douts[k] for k in feats])
        for t in feats.values():
            t.grad = None
        mod.zero_grad(set_to_none=True)
    return step


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--nodes', type=int, default=1024)
    p.add_argument('--ch', type=int, default=512)
    p.add_argument('--degrees', type=int, default=4)
    p.add_argument('--window', type=float, default=1.0,
                   help='seconds of work per timed window')
    p.add_argument('--rounds', type=int, default=3,
                   help='alternating fused/eager windows per case')
    p.add_argument('--out', default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        'profiles', 'norm_variants.json'))
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit('bench_norm.py needs a GPU')
    fused.require_ext()
    dev = 'cuda'
    N, C = args.nodes, args.ch
    fiber = Fiber([(d, C) for d in range(args.degrees)])

    results = []
    for gated in (False, True):
        for nl_name, nl in (('gelu', nn.GELU), ('identity', nn.Identity)):
            for dtype in (torch.float32, torch.bfloat16):
                torch.manual_seed(0)
                mod = NormSE3(fiber, nonlin=nl(), gated_scale=gated).to(dev)
                if gated:
                    with torch.no_grad():
                        for prm in mod.parameters():
                            prm.copy_(torch.randn_like(prm) / math.sqrt(C))
                feats = {str(d): torch.randn(1, N, C, 2 * d + 1, device=dev)
                         .to(dtype).requires_grad_(True)
                         for d in range(args.degrees)}
                douts = {k: torch.randn_like(v) for k, v in feats.items()}
                steps = {'fused': make_step(mod, feats, douts, False),
                         'eager': make_step(mod, feats, douts, True)}
                iters = {}
                for name, step in steps.items():      # warm-up + sizing
                    for _ in range(10):
                        step()
                    torch.cuda.synchronize()
                    ms = window_ms(step, 20)
                    iters[name] = max(20, int(args.window * 1e3 / ms) + 1)
                times = {'fused': [], 'eager': []}
                for _ in range(args.rounds):
                    for name in ('fused', 'eager'):
                        times[name].append(window_ms(steps[name], iters[name]))
                med = {k: statistics.median(v) for k, v in times.items()}
                spread = max((max(v) - min(v)) / med[k]
                             for k, v in times.items())
                row = {
                    'variant': 'gated' if gated else 'scale',
                    'nonlin': nl_name,
                    'dtype': str(dtype).replace('torch.', ''),
                    'fused_ms': med['fused'], 'eager_ms': med['eager'],
                    'fused_windows_ms': times['fused'],
                    'eager_windows_ms': times['eager'],
                    'iters_per_window': iters,
                    'spread_rel': spread,
                    'speedup': med['eager'] / med['fused'],
                    'no_slower': med['fused'] <= med['eager'] * (1 + spread),
                }
                results.append(row)
                print(f"{row['variant']:5s} {nl_name:8s} {row['dtype']:8s} "
                      f"fused {med['fused']:7.3f} ms  eager "
                      f"{med['eager']:7.3f} ms  x{row['speedup']:.2f}  "
                      f"spread {spread:.1%}", flush=True)

    doc = {
        'what': 'NormSE3 forward+backward, all degrees in one step; '
                'eager = SE3_EAGER_NORM=1 (the path before the kernels)',
        'device': torch.cuda.get_device_name(0),
        'nodes': N, 'channels': C, 'degrees': args.degrees,
        'window_s': args.window, 'rounds': args.rounds,
        'timing': 'device events around iters_per_window steps, median of '
                  'alternating windows; spread_rel = (max-min)/median',
        'results': results,
        'all_no_slower': all(r['no_slower'] for r in results),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
