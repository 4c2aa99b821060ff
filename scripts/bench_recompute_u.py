"""Time and size one training step with SE3_RECOMPUTE_U off against on.

Usage (GPU box):  python scripts/bench_recompute_u.py [--only on]
                      [--num-neighbors 32] [--out profiles/recompute_u.json]

The model is bench.py's: by default the headline config (1024 points,
dim 512, 8 heads, depth 6, 4 degrees, k = 8), bf16 autocast, one SGD step,
no graph capture. The two settings alternate in one process (the switch is
read at call time). Each window is one warm-up step, then
torch.cuda.reset_peak_memory_stats(), then --steps steps between two device
events, closed by a synchronise. Recorded per setting: ms_per_step and
max_memory_allocated of every window; beside them the bytes of the U set
(U (mi*F, E, OP) bf16 of every degree pair of every ConvSE3, E = batch *
points * k), computed from the shapes, which is what the switch should take
off the peak. An out-of-memory error is recorded as a result.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from se3_transformer_amd import SE3Transformer
from se3_transformer_amd.models.core import ConvSE3
from se3_transformer_amd.ops import fused

SWITCH = 'SE3_RECOMPUTE_U'


def u_set_bytes(model, E):
    """Bytes of U over the pairs the ubuild kernels serve, and the bytes of
    the node features and rows saved in their place (fp32 features)."""
    u = nodes = convs = 0
    for m in model.modules():
        if not isinstance(m, ConvSE3):
            continue
        convs += 1
        for pc in m.kernel_unary.values():
            I = 2 * pc.degree_in + 1
            if pc.nc_in % 32 or pc.d_out * I * pc.num_freq > 343:
                continue
            u += pc.nc_in * pc.num_freq * E * fused.opad(pc.d_out) * 2
        nodes += sum(mi * (2 * di + 1) for di, mi in m.fiber_in) * 4
    return u, nodes, convs


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=1)
    p.add_argument('--points', type=int, default=1024)
    p.add_argument('--dim', type=int, default=512)
    p.add_argument('--heads', type=int, default=8)
    p.add_argument('--dim-head', type=int, default=64)
    p.add_argument('--depth', type=int, default=6)
    p.add_argument('--num-degrees', type=int, default=4)
    p.add_argument('--num-neighbors', type=int, default=8)
    p.add_argument('--valid-radius', type=float, default=10.)
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--init-scale', type=float, default=0.5)
    p.add_argument('--steps', type=int, default=3)
    p.add_argument('--rounds', type=int, default=2,
                   help='alternating off/on windows per setting')
    p.add_argument('--only', choices=['off', 'on'], default=None,
                   help='run one setting alone')
    p.add_argument('--out', default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        'profiles', 'recompute_u.json'))
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit('bench_recompute_u.py needs a GPU')
    fused.require_ext()
    dev = torch.device('cuda')
    torch.manual_seed(0)
    with torch.device(dev):
        model = SE3Transformer(dim=args.dim, heads=args.heads,
                               dim_head=args.dim_head, depth=args.depth,
                               num_degrees=args.num_degrees,
                               valid_radius=args.valid_radius,
                               num_neighbors=args.num_neighbors,
                               attend_self=True)
    with torch.no_grad():
        for prm in model.parameters():
            if prm.dim() >= 2:
                prm.mul_(args.init_scale)
    opt = torch.optim.SGD(model.parameters(), lr=args.lr)

    g = torch.Generator(device='cpu').manual_seed(1000)
    feats = torch.randn(args.batch, args.points, args.dim, generator=g).to(dev)
    coors = (torch.randn(args.batch, args.points, 3, generator=g) * 2.0).to(dev)
    mask = torch.ones(args.batch, args.points, dtype=torch.bool, device=dev)
    target = torch.randn(args.batch, args.points, args.dim, generator=g).to(dev)

    def step():
        opt.zero_grad(set_to_none=False)
        with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
            out = model(feats, coors, mask, return_type=0)
            loss = (out.float() - target).pow(2).mean()
        loss.backward()
        opt.step()
        return loss.detach()

    def window(setting):
        os.environ.pop(SWITCH, None)
        if setting == 'on':
            os.environ[SWITCH] = '1'
        try:
            step()                                  # warm-up
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.steps):
                loss = step()
            end.record()
            torch.cuda.synchronize()
            return {'ms_per_step': start.elapsed_time(end) / args.steps,
                    'max_memory_allocated': torch.cuda.max_memory_allocated(),
                    'loss': loss.item()}
        except torch.OutOfMemoryError as e:
            opt.zero_grad(set_to_none=True)
            return {'oom': True, 'message': str(e).split('\n')[0],
                    'max_memory_allocated': torch.cuda.max_memory_allocated()}
        finally:
            os.environ.pop(SWITCH, None)

    E = args.batch * args.points * args.num_neighbors
    u_bytes, node_units, convs = u_set_bytes(model, E)
    settings = [args.only] if args.only else ['off', 'on']
    windows = {s: [] for s in settings}
    for r in range(args.rounds):
        for s in settings:
            w = window(s)
            windows[s].append(w)
            print(f'round {r} {s:3s}: ' + json.dumps(w), flush=True)
            if w.get('oom'):
                break
            torch.cuda.empty_cache()
        if any(w.get('oom') for ws in windows.values() for w in ws):
            break

    def summary(ws):
        ok = [w for w in ws if not w.get('oom')]
        if not ok:
            return {'oom': True, 'windows': ws}
        return {'ms_per_step': statistics.median(w['ms_per_step'] for w in ok),
                'max_memory_allocated': max(w['max_memory_allocated']
                                            for w in ok),
                'oom': len(ok) < len(ws), 'windows': ws}

    doc = {
        'what': 'one training step (forward, backward, SGD), bf16 autocast, '
                'no graph capture, SE3_RECOMPUTE_U off against on',
        'device': torch.cuda.get_device_name(0),
        'total_memory': torch.cuda.get_device_properties(0).total_memory,
        'config': {k: getattr(args, k) for k in (
            'batch', 'points', 'dim', 'heads', 'dim_head', 'depth',
            'num_degrees', 'num_neighbors', 'steps', 'rounds')},
        'parameters': sum(p_.numel() for p_ in model.parameters()),
        'convse3_modules': convs,
        'u_set_bytes_from_shapes': u_bytes,
        'node_feature_bytes_from_shapes': node_units * args.batch * args.points,
        'timing': 'device events around --steps steps after one warm-up step, '
                  'median over the alternating windows; peak = '
                  'max_memory_allocated after reset_peak_memory_stats, '
                  'largest window',
        'settings': {s: summary(ws) for s, ws in windows.items()},
    }
    if all(not v.get('oom') for v in doc['settings'].values()) \
            and len(settings) == 2:
        off, on = doc['settings']['off'], doc['settings']['on']
        doc['peak_drop_bytes'] = (off['max_memory_allocated']
                                  - on['max_memory_allocated'])
        doc['time_cost_rel'] = on['ms_per_step'] / off['ms_per_step'] - 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
