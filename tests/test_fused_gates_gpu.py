"""GPU checks of the gates of ops/fused.py with the built extension, at the
shapes of the smoke run. Tensors are only allocated: no kernel is launched."""
import pytest
import torch

from fused_helpers import check_switches, no_switches  # noqa: F401
from se3_transformer_amd.ops import fused

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason='no GPU')]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_every_gate_opens_and_only_its_own_switch_closes_it(dtype):
    check_switches(lambda *shape, dtype=dtype:
                   torch.empty(*shape, dtype=dtype, device='cuda'))
    with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
        assert fused.pairconv_ok(torch.empty(512, 64, 3, device='cuda'),
                                 64, 192, 3, 128)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_gates_flip_at_the_kernel_limits(dtype):
    def t(*shape, dtype=dtype):
        return torch.empty(*shape, dtype=dtype, device='cuda')
    C = fused.NORM_GATED_MAX_C
    assert fused.norm_ok(t(1, 2, C, 3), True, 'gelu')
    assert not fused.norm_ok(t(1, 2, C + 1, 3), True, 'gelu')
    assert fused.norm_ok(t(1, 2, C + 1, 3), False, 'gelu')   # scale: no ceiling

    coors = t(1, 5441, 3, dtype=torch.float32)
    assert fused.knn_kernel_ok(coors[:, :5440], 5440, 5439)
    assert not fused.knn_kernel_ok(coors, 5441, 5440)

    assert fused.attn_ok(t(1, 4, 64, 448, 1), 9, 448)
    assert not fused.attn_ok(t(1, 4, 64, 449, 1), 9, 449)
    for rot, ok in ((64, True), (66, False)):
        q, qpe, kpe = t(1, 4, 64, 128, 1), t(1, 64, rot), t(1, 64, 8, rot)
        assert fused.rope_ok(q, 8, qpe, kpe, True, None) is ok, rot
