"""GPU tests of the o-padded edge-major layout: U (miF, E, OP) and
G (mo, E, OP) bf16, dU (miF, E, OP) fp32, OP = 8 for O in (5, 7), 4 for
O = 3, pad lanes exactly zero (csrc/pairconv_common.h).

The producers (ubuild_opad, pack_g) and the consumer (fused_pairconv_opad)
are checked on the padded tensors themselves; the (miF, O, E) entry points
are thin torch compositions over them and are held to agree with them.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason='no GPU')


def _rel_err(a, b):
    denom = b.abs().max().clamp(min=1e-6)
    return ((a - b).abs().max() / denom).item()


def _rnd16(gen, *shape):
    """bf16-representable fp32 values."""
    x = torch.randn(*shape, generator=gen, device='cuda')
    return x.to(torch.bfloat16).float()


def _pad_o(x, OP):
    return torch.nn.functional.pad(x, (0, OP - x.shape[-1]))


@needs_gpu
def test_opad_widths():
    from se3_transformer_amd.ops import fused
    assert [fused.opad(O) for O in (1, 3, 5, 7)] == [1, 4, 8, 8]


@needs_gpu
@pytest.mark.parametrize('O,mo,miF,E',
                         [(O, mo, 64, 77) for O in (3, 5, 7)
                          for mo in (8, 16)] + [(3, 128, 256, 77)])
def test_fused_pairconv_opad_vs_oracle(O, mo, miF, E):
    """fused_pairconv_opad on padded tensors against fp32 autograd of
    _FusedPairConvOpad's docstring formula on the bf16-rounded inputs.

    E=77 is a full 64-edge block plus a ragged 13-edge one, and is odd, so
    at OP=4 the rows of U are only 8-byte aligned. miF=64 makes the chunk
    loops and the register staging iterate; mo=8 is one mo-block per
    workgroup (MB2=1, dh unsplit), mo=16 two (MB2=2). (3, 128, 256) takes
    the XCD-cohort block mapping (fwd and du) and dh's 16-way split-K.

    Bands: those of test_pairconv_kernels_small_shapes_vs_oracle (dR is
    still rounded to bf16 once). The pad lanes of dU must be exactly zero.
    """
    from se3_transformer_amd.ops import fused

    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(1000 * O + mo)
    vals = [_rnd16(gen, E, 128), _rnd16(gen, mo * miF, 128),
            _rnd16(gen, mo * miF), _pad_o(_rnd16(gen, miF, E, O), OP)]
    gout = _rnd16(gen, E, mo, O)

    def leaves():
        return [v.clone().requires_grad_(True) for v in vals]

    H, W, bias, U = leaves()
    R = (H @ W.t() + bias).view(E, mo, miF)
    ref = torch.einsum('emc,ceo->emo', R, U[:, :, :O])
    ref_grads = torch.autograd.grad(ref, (H, W, bias, U), gout)

    H, W, bias, U = leaves()
    out = fused.fused_pairconv_opad(H, W, bias, U, mo, O)
    assert out.shape == (E, mo, O) and out.dtype == torch.float32
    grads = torch.autograd.grad(out, (H, W, bias, U), gout)

    errs = {'out': _rel_err(out.detach(), ref.detach())}
    for name, a, b in zip(('dH', 'dW', 'db', 'dU'), grads, ref_grads):
        errs[name] = _rel_err(a.float(), b)
    print(f'opad oracle O={O} mo={mo} miF={miF} E={E}: '
          + ' '.join(f'{k}={v:.3e}' for k, v in errs.items()))
    bands = {'out': 8e-4, 'dH': 8e-3, 'dW': 9e-3, 'db': 2e-2, 'dU': 1e-2}
    for name, band in bands.items():
        assert errs[name] < band, (name, errs)
    dU = grads[3]
    assert dU.shape == (miF, E, OP)
    assert torch.equal(dU[..., O:], torch.zeros_like(dU[..., O:])), \
        'dU pad lanes must be exactly zero'


@needs_gpu
@pytest.mark.parametrize('O,I,F_', [(3, 5, 3), (5, 5, 5), (7, 7, 7)])
def test_ubuild_opad_vs_einsum(O, I, F_):
    """ubuild_opad forward and dX against the eager einsum, bands of
    test_ubuild_kernel_vs_einsum; the pad lanes are exactly zero. E=77 is
    two full 32-edge forward blocks plus a ragged one."""
    from se3_transformer_amd.ops import fused

    torch.manual_seed(14)
    E, C = 77, 32
    OP = fused.opad(O)
    B = torch.randn(E, O, I, F_, device='cuda')
    x0 = torch.randn(E, C, I, device='cuda', requires_grad=True)
    x1 = x0.detach().clone().requires_grad_(True)

    ref = torch.einsum('eoif,eci->cfeo', B, x0).reshape(C * F_, E, O)
    ref.float().pow(2).mean().backward()

    out = fused.ubuild_opad(x1, B.contiguous(), O, I, F_)
    assert out.shape == (C * F_, E, OP) and out.dtype == torch.bfloat16
    assert out.is_contiguous()
    assert torch.equal(out[..., O:], torch.zeros_like(out[..., O:])), \
        'U pad lanes must be exactly zero'
    # same loss as the reference: the pads contribute nothing to the sum
    (out.float().pow(2).sum() / ref.numel()).backward()

    assert _rel_err(out[..., :O].float(), ref) < 1e-2, 'ubuild_opad forward'
    assert _rel_err(x1.grad, x0.grad) < 3e-2, 'ubuild_opad dX'


@needs_gpu
def test_ubuild_opad_db():
    """dB through the padded dU, band of tests/test_diffcoors_gpu.py's
    test_ubuild_db: x and the cotangent are bf16-representable, so only the
    summation order over the C = 32 terms differs from the fp32 einsum."""
    from se3_transformer_amd.ops import fused

    E, C, O, I, F_ = 77, 32, 5, 5, 5
    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(3)
    x = _rnd16(gen, E, C, I).requires_grad_()
    B = torch.randn(E, O, I, F_, generator=gen, device='cuda').requires_grad_()
    G = _rnd16(gen, C * F_, E, OP)      # pad lanes carry a cotangent too
    out = fused.ubuild_opad(x, B, O, I, F_)
    (out.float() * G).sum().backward()

    db_ref = torch.einsum('eci,cfeo->eoif', x.detach(),
                          G[..., :O].reshape(C, F_, E, O))
    err = _rel_err(B.grad, db_ref)
    print(f'ubuild_opad dB ({O},{I},{F_}): rel_err={err:.3e}')
    assert B.grad.dtype == torch.float32 and B.grad.shape == (E, O, I, F_)
    assert err < 1e-5


@needs_gpu
@pytest.mark.parametrize('O', [3, 5, 7])
def test_pack_g_bit_exact(O):
    """pack_g == grad.to(bf16), permuted to (mo, E, O) and zero-padded."""
    from se3_transformer_amd.ops import fused

    ext = fused._load_ext()
    E, mo = 77, 16
    OP = fused.opad(O)
    gen = torch.Generator('cuda').manual_seed(O)
    # scaled so that round-to-nearest-even ties and several exponents occur
    grad = torch.randn(E, mo, O, generator=gen, device='cuda') * 37.0
    grad[0, 0, 0] = 1.00390625          # exact tie between two bf16 values
    grad[1, 0, 0] = 1.01171875          # tie, odd neighbour below
    G = torch.full((mo, E, OP), 7.0, dtype=torch.bfloat16, device='cuda')
    ext.pack_g(grad, G)
    ref = _pad_o(grad.to(torch.bfloat16).permute(1, 0, 2), OP)
    assert torch.equal(G, ref)


@needs_gpu
def test_old_and_new_entry_points_agree():
    """ubuild() is a view of ubuild_opad() and fused_pairconv() a repack
    around fused_pairconv_opad(): forward bit-equal; dH, summed by split-K
    atomics in no fixed order, inside the 1e-5 max-normalised band
    profiles/pairconv_prune.md uses for it."""
    from se3_transformer_amd.ops import fused

    E, C, O, I, F_, mo = 77, 32, 5, 5, 5, 16
    miF = C * F_
    gen = torch.Generator('cuda').manual_seed(11)
    x = torch.randn(E, C, I, generator=gen, device='cuda')
    B = torch.randn(E, O, I, F_, generator=gen, device='cuda')
    U = fused.ubuild_opad(x, B, O, I, F_)
    Ut = fused.ubuild(x, B, O, I, F_)
    assert Ut.shape == (miF, O, E)
    assert torch.equal(Ut, U[:, :, :O].permute(0, 2, 1))

    W = torch.randn(mo * miF, 128, generator=gen, device='cuda') / 128 ** 0.5
    bias = torch.randn(mo * miF, generator=gen, device='cuda')
    gout = torch.randn(E, mo, O, generator=gen, device='cuda')
    H0 = _rnd16(gen, E, 128)            # fp32 leaf, so dH comes back fp32

    Ha = H0.clone().requires_grad_()
    out_a = fused.fused_pairconv_opad(Ha, W, bias, U, mo, O)
    dHa, = torch.autograd.grad(out_a, Ha, gout)
    Hb = H0.clone().requires_grad_()
    out_b = fused.fused_pairconv(Hb, W, bias, Ut, mo)
    dHb, = torch.autograd.grad(out_b, Hb, gout)

    assert torch.equal(out_a, out_b)
    err = _rel_err(dHa.float(), dHb.float())
    print(f'old vs new entry points: dH rel_err={err:.3e}')
    assert err < 1e-5
