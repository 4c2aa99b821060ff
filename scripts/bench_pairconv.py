"""Microbenchmark the fused pairconv kernels at headline shapes.

Usage (GPU box):  python scripts/bench_pairconv.py [--pair 3,3]
Prints per-kernel ms and GEMM-equivalent TFLOP/s for fwd, bwd_dh, bwd_dw,
bwd_du on the o-padded edge-major tensors U (miF, E, OP) / G (mo, E, OP), and
the times of their two producers, ubuild_fwd and pack_g, separately.
bwd_dw is timed with and without db; --du-dtype picks the dU that bwd_du
writes (bf16 is what training uses, f32 what it wrote before).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from se3_transformer_amd import _C


def timeit(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1000


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--pair', default='3,3')
    p.add_argument('--E', type=int, default=9216)
    p.add_argument('--ch', type=int, default=512)
    p.add_argument('--only', default=None, choices=['fwd','dh','dw','du'])
    p.add_argument('--du-dtype', default='bf16', choices=['bf16', 'f32'])
    args = p.parse_args()
    di, do = map(int, args.pair.split(','))
    F = 2 * min(di, do) + 1
    O = 2 * do + 1
    mi = mo = args.ch
    miF = mi * F
    E, K = args.E, 128
    N = mo * miF
    dev = 'cuda'
    du_dtype = {'bf16': torch.bfloat16, 'f32': torch.float32}[args.du_dtype]
    g = torch.Generator(device=dev).manual_seed(0)

    H = torch.randn(E, K, generator=g, device=dev).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device=dev) / K**0.5).to(torch.bfloat16)
    Ut = torch.randn(miF, O, E, generator=g, device=dev).to(torch.bfloat16)
    out = torch.zeros(E, mo, O, device=dev)
    gt = torch.randn(mo, O, E, generator=g, device=dev).to(torch.bfloat16)
    bias = torch.zeros(N, device=dev)
    # the same seeded values in the layout the kernels read
    OP = _C.pairconv_opad(O)
    pad = torch.nn.functional.pad
    U = pad(Ut.permute(0, 2, 1), (0, OP - O)).contiguous()
    G = pad(gt.permute(0, 2, 1), (0, OP - O)).contiguous()
    del Ut

    gemm_fl = 2.0 * E * N * K
    epi_fl = 2.0 * E * N * O

    from se3_transformer_amd.ops.fused import _pack_w_dh, _pack_w_fwd
    P = _pack_w_fwd(W, mo, miF)

    Pf2 = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
    Pdh2 = torch.empty(N * K, dtype=torch.bfloat16, device=dev)
    _C.pack_w_both(W, Pf2, Pdh2, mo)
    okf = torch.equal(Pf2.view_as(P), P)
    okd = torch.equal(Pdh2.view(_pack_w_dh(W, mo, miF).shape),
                      _pack_w_dh(W, mo, miF))
    ms = timeit(lambda: _C.pack_w_both(W, Pf2, Pdh2, mo))
    gb = (N * K * 2 * 3) / 1e9   # read W bf16 + write both
    print(f'pack_w_both: {ms:8.3f} ms  {gb/ms:7.2f} TB/s  '
          f'parity fwd={okf} dh={okd}')

    if args.only:
        fn = {'fwd': lambda: _C.pairconv_fwd_opad(H, P, U, out, mo),
              'dh': lambda: _C.pairconv_bwd_dh(G, U, _pack_w_dh(W, mo, miF),
                                               torch.zeros(E, K, device=dev), mo, O),
              'dw': lambda: _C.pairconv_bwd_dw(G, U, H.t().contiguous(),
                                               torch.empty(N, K, device=dev),
                                               torch.empty(N, device=dev), mo, O),
              'du': lambda: _C.pairconv_bwd_du(H, P, bias, G,
                                               torch.empty(miF, E, OP, device=dev,
                                                           dtype=du_dtype),
                                               mo, O)}[args.only]
        print(args.only, timeit(fn, iters=3, warmup=1), 'ms')
        return

    # producers of the padded layout
    gout = gt.permute(2, 0, 1).float().contiguous()          # (E, mo, O) f32
    G2 = torch.empty_like(G)
    ms = timeit(lambda: _C.pack_g(gout, G2))
    gb = (gout.numel() * 4 + G2.numel() * 2) / 1e9
    print(f'pack_g      ({di},{do}): {ms:8.3f} ms  {gb/ms:7.2f} TB/s  '
          f'parity={torch.equal(G2, G)}')
    del gout, G2
    I = 2 * di + 1
    Bb = torch.randn(E, O, I, F, generator=g, device=dev)
    X = torch.randn(E, mi, I, generator=g, device=dev).to(torch.bfloat16)
    U2 = torch.empty_like(U)
    ms = timeit(lambda: _C.ubuild_fwd(Bb, X, U2, O, I, F))
    gb = (Bb.numel() * 4 + X.numel() * 2 + U2.numel() * 2) / 1e9
    print(f'ubuild_fwd  ({di},{do}): {ms:8.3f} ms  {gb/ms:7.2f} TB/s')
    del Bb, X, U2

    ms = timeit(lambda: _C.pairconv_fwd_opad(H, P, U, out, mo))
    print(f'fwd    ({di},{do}): {ms:8.3f} ms  {gemm_fl/ms/1e9:7.1f} TF/s (gemm) '
          f'{(gemm_fl+epi_fl)/ms/1e9:7.1f} TF/s (total)')

    P1 = _pack_w_dh(W, mo, miF)
    dH = torch.zeros(E, K, device=dev)
    ms = timeit(lambda: _C.pairconv_bwd_dh(G, U, P1, dH, mo, O))
    print(f'bwd_dh ({di},{do}): {ms:8.3f} ms  {gemm_fl/ms/1e9:7.1f} TF/s')

    Ht = H.t().contiguous()
    dW = torch.empty(N, K, device=dev)
    no_db = torch.empty(0, device=dev)
    ms = timeit(lambda: _C.pairconv_bwd_dw(G, U, Ht, dW, no_db, mo, O))
    print(f'bwd_dw ({di},{do}): {ms:8.3f} ms  {gemm_fl/ms/1e9:7.1f} TF/s')
    db = torch.empty(N, device=dev)
    ms = timeit(lambda: _C.pairconv_bwd_dw(G, U, Ht, dW, db, mo, O))
    print(f'bwd_dw+db ({di},{do}): {ms:8.3f} ms  {gemm_fl/ms/1e9:7.1f} TF/s')
    ms = timeit(lambda: G.view(mo, E * OP) @ U.view(miF, E * OP).t())
    print(f'db as a library GEMM ({di},{do}): {ms:8.3f} ms')

    dU = torch.empty(miF, E, OP, device=dev, dtype=du_dtype)
    ms = timeit(lambda: _C.pairconv_bwd_du(H, P, bias, G, dU, mo, O))
    print(f'bwd_du ({di},{do}) {args.du_dtype}: {ms:8.3f} ms  '
          f'{gemm_fl/ms/1e9:7.1f} TF/s')

    # library GEMM reference: the raw R = H @ W^T (what eager must do, without
    # even the contraction), on a slab 1/8 of N to fit memory
    Nr = N // 8
    Wr = W[:Nr]
    ms = timeit(lambda: H @ Wr.t(), iters=5)
    print(f'hipblaslt H@W[{Nr}] : {ms:8.3f} ms  {2.0*E*Nr*K/ms/1e9:7.1f} TF/s'
          f'  (writes R slab: {E*Nr*2/1e9:.2f} GB)')


if __name__ == '__main__':
    main()
