"""CPU checks of the pairconv and ubuild kernels' gates and padding helpers
for channel counts that are no multiple of the MFMA tile (8 mo x 32 urows):
the gates open for any mo, miF >= 1, SE3_RECOMPUTE_U keeps C % 32 == 0, the
torch packs of a ragged W are the packs of the zero-padded W, and a CPU
forward of a ragged model stays away from the extension."""
import types

import pytest
import torch

from fused_helpers import (install_ext, no_switches, stub_ext,  # noqa: F401
                           switches)
from se3_transformer_amd.ops import fused


def _t(*shape, dtype=torch.float32, cuda=True):
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, shape=shape,
                                 dim=lambda: len(shape), requires_grad=False)


def test_pad_dims():
    assert fused.pad_dims(1, 1) == (8, 32)
    assert fused.pad_dims(8, 32) == (8, 32)
    assert fused.pad_dims(9, 33) == (16, 64)
    assert fused.pad_dims(24, 48) == (24, 64)


def test_fused_shapes_ok_for_any_channel_count():
    assert fused.fused_shapes_ok(1, 1, 1, 128)
    assert fused.fused_shapes_ok(7, 33, 7, 128)
    assert fused.fused_shapes_ok(24, 48, 3, 128)
    assert fused.fused_shapes_ok(32, 192, 3, 128)
    # what still closes the gate
    assert not fused.fused_shapes_ok(7, 33, 7, 64)
    assert not fused.fused_shapes_ok(7, 33, 9, 128)
    assert not fused.fused_shapes_ok(0, 33, 3, 128)
    assert not fused.fused_shapes_ok(7, 0, 3, 128)


def test_ubuild_gate_takes_any_c_and_recompute_u_keeps_c32(monkeypatch):
    install_ext(monkeypatch, stub_ext())
    B = _t(30, 3, 3, 3)
    for C in (5, 48, 1, 32):
        assert fused.ubuild_ok(B, C, 3, 3, 3), C
    assert not fused.ubuild_ok(B, 0, 3, 3, 3)
    assert not fused.ubuild_ok(B, 5, 7, 7, 8)            # O*I*F = 392 > 343
    with switches(SE3_EAGER_UBUILD='1'):
        assert not fused.ubuild_ok(B, 5, 3, 3, 3)
    with switches(SE3_RECOMPUTE_U='1'):
        assert fused.recompute_u_ok(_t(10, 32, 3), B, 32, 3, 3, 3)
        assert not fused.recompute_u_ok(_t(10, 48, 3), B, 48, 3, 3, 3)
        assert not fused.recompute_u_ok(_t(10, 5, 3), B, 5, 3, 3, 3)


def test_pairconv_gate_opens_on_ragged_shapes(monkeypatch):
    install_ext(monkeypatch, stub_ext())
    x16 = _t(130, 24, 3, dtype=torch.bfloat16)
    assert fused.pairconv_ok(x16, 5, 72, 5, 128)
    assert fused.pairconv_ok(x16, 1, 1, 1, 128)
    assert not fused.pairconv_ok(_t(130, 24, 3, cuda=False), 5, 72, 5, 128)


@pytest.mark.parametrize('mo,miF', [(1, 1), (7, 33), (9, 31), (24, 48),
                                    (17, 65), (8, 32)])
def test_torch_packs_of_a_ragged_w_are_the_packs_of_the_padded_w(mo, miF):
    gen = torch.Generator().manual_seed(100 * mo + miF)
    W = torch.randn(mo * miF, 128, generator=gen).to(torch.bfloat16)
    mo_p, miF_p = fused.pad_dims(mo, miF)
    Wp = torch.zeros(mo_p, miF_p, 128, dtype=torch.bfloat16)
    Wp[:mo, :miF] = W.view(mo, miF, 128)
    Wp = Wp.view(mo_p * miF_p, 128)
    assert torch.equal(fused._pad_rows(W, mo, miF), Wp)
    Pf, Pdh = fused._pack_w_fwd(W, mo, miF), fused._pack_w_dh(W, mo, miF)
    assert Pf.numel() == Pdh.numel() == mo_p * miF_p * 128
    assert torch.equal(Pf, fused._pack_w_fwd(Wp, mo_p, miF_p))
    assert torch.equal(Pdh, fused._pack_w_dh(Wp, mo_p, miF_p))
    # a pack permutes: nothing but W's values and the zero pads
    assert torch.equal(Pf.reshape(-1).float().sort().values,
                       Wp.reshape(-1).float().sort().values)


def test_bias_and_u_padding_helpers():
    b = torch.arange(1., 7.)                              # (mo=2, miF=3)
    bp = fused._pad_rows(b, 2, 3).view(8, 32)
    assert torch.equal(bp[:2, :3], b.view(2, 3))
    assert bp.abs().sum() == b.abs().sum()
    U = torch.randn(3, 5, 4).to(torch.bfloat16)
    Up = fused._pad_u_rows(U, 3)
    assert Up.shape == (32, 5, 4) and torch.equal(Up[:3], U)
    assert not Up[3:].any()
    assert fused._pad_u_rows(Up, 3) is Up                 # padded already
    with pytest.raises(ValueError):
        fused._pad_u_rows(torch.zeros(4, 5, 4), 3)


def test_cpu_forward_of_a_ragged_model_leaves_the_loader_alone(monkeypatch):
    from se3_transformer_amd import SE3Transformer
    monkeypatch.setattr(fused, '_load_ext',
                        lambda: pytest.fail('the extension loader was touched'))
    torch.manual_seed(0)
    model = SE3Transformer(dim=16, heads=2, dim_head=8, depth=1,
                           num_degrees=2, num_neighbors=4)
    feats, coors = torch.randn(1, 8, 16), torch.randn(1, 8, 3)
    mask = torch.ones(1, 8, dtype=torch.bool)
    out = model(feats, coors, mask, return_type=0)
    assert out.shape == (1, 8, 16) and torch.isfinite(out).all()
