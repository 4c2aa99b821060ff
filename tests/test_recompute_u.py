"""CPU checks of SE3_RECOMPUTE_U: the edge rows, the gate and its order, the
entry-point check at load, and that the eager path does not see the switch."""
import types

import pytest
import torch

from fused_helpers import (install_ext, no_switches, stub_ext,  # noqa: F401
                           switches)
from se3_transformer_amd.models.core import ConvSE3
from se3_transformer_amd.models.fiber import Fiber
from se3_transformer_amd.ops import fused
from se3_transformer_amd.ops.basis import get_basis_packed
from se3_transformer_amd.utils import batched_index_select


def _t(*shape, dtype=torch.float32, cuda=True):
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, shape=shape,
                                 dim=lambda: len(shape), requires_grad=False)


def test_switch_is_listed():
    assert 'SE3_RECOMPUTE_U' in fused.SWITCHES
    assert fused.switch('SE3_RECOMPUTE_U') is None


def test_edge_rows_index_the_flattened_nodes():
    b, n, k, C, I = 2, 5, 3, 4, 3
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(b, n, C, I, generator=gen)
    idx = torch.randint(0, n, (b, n, k), generator=gen)
    rows = fused.edge_rows(idx, n)
    assert rows.shape == (b * n * k,) and rows.dtype == torch.int32
    assert rows.is_contiguous()
    got = x.reshape(b * n, C, I)[rows.long()].view(b, n, k, C, I)
    assert torch.equal(got, batched_index_select(x, idx, dim=1))


def test_gate_is_false_on_the_cpu_and_leaves_the_loader_alone(monkeypatch):
    monkeypatch.setattr(fused, '_load_ext',
                        lambda: pytest.fail('the extension loader was touched'))
    with switches(SE3_RECOMPUTE_U='1'):
        assert fused.recompute_u_ok(torch.zeros(10, 32, 3),
                                    torch.zeros(30, 3, 3, 3), 32, 3, 3, 3) is False
        assert fused.recompute_u_ok(_t(10, 32, 3, cuda=False),
                                    _t(30, 3, 3, 3), 32, 3, 3, 3) is False
        # nor by GPU tensors that dtype or shape keep on today's path
        assert not fused.recompute_u_ok(_t(10, 32, 3, dtype=torch.float64),
                                        _t(30, 3, 3, 3), 32, 3, 3, 3)
        assert not fused.recompute_u_ok(_t(10, 48, 3), _t(30, 3, 3, 3),
                                        48, 3, 3, 3)
    # nor, switched off, by anything
    assert not fused.recompute_u_ok(_t(10, 32, 3), _t(30, 3, 3, 3), 32, 3, 3, 3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_gate_with_the_extension_stubbed(monkeypatch, dtype):
    install_ext(monkeypatch, stub_ext())
    x, B = _t(10, 32, 3, dtype=dtype), _t(30, 3, 3, 3)

    def ok(C=32, O=3, I=3, F=3):
        return fused.recompute_u_ok(_t(10, C, I, dtype=dtype), B, C, O, I, F)

    assert not ok()
    with switches(SE3_RECOMPUTE_U='0'):
        assert not ok()
    with switches(SE3_RECOMPUTE_U='1'):
        assert ok() and ok(O=7, I=7, F=7)
        assert fused.recompute_u_ok(x, B, 32, 3, 3, 3)
        assert not ok(C=48)
        assert not ok(O=7, I=7, F=8)                 # O*I*F = 392 > 343
        assert not fused.recompute_u_ok(x, _t(30, 3, 3, 3, dtype=torch.float64),
                                        32, 3, 3, 3)
        with switches(SE3_EAGER_UBUILD='1'):
            assert not ok()
    assert not ok()


def test_a_module_without_the_gather_kernels_is_a_load_error(monkeypatch):
    stale = tuple(n for n in fused._ENTRY_POINTS if n != 'ubuild_gather_fwd')
    assert len(stale) == len(fused._ENTRY_POINTS) - 1
    install_ext(monkeypatch, stub_ext(names=stale))
    with pytest.raises(RuntimeError, match='ubuild_gather_fwd'):
        fused._load_ext()


def test_eager_path_does_not_see_the_switch():
    """A CPU ConvSE3 forward and backward with the switch set is the run with
    it unset, bit for bit."""
    torch.manual_seed(0)
    b, n, k = 1, 6, 3
    fiber = Fiber([(0, 4), (1, 4)])
    conv = ConvSE3(fiber, fiber, pool=True, self_interaction=True)
    feats = {'0': torch.randn(b, n, 4, 1), '1': torch.randn(b, n, 4, 3)}
    coors = torch.randn(b, n, 3)
    idx = torch.stack([torch.randperm(n)[:k] for _ in range(b * n)]) \
        .view(b, n, k)
    rel_pos = coors.unsqueeze(2) - batched_index_select(coors, idx, dim=1)
    basis = get_basis_packed(rel_pos, 1)
    mask = torch.ones(b, n, k, dtype=torch.bool)

    def run():
        leaves = {d: t.clone().requires_grad_() for d, t in feats.items()}
        out = conv(leaves, (idx, mask, None), rel_dist=rel_pos.norm(dim=-1),
                   basis=basis)
        params = list(conv.parameters())
        grads = torch.autograd.grad(
            sum(o.pow(2).sum() for o in out.values()),
            list(leaves.values()) + params)
        return list(out.values()) + list(grads)

    off = run()
    with switches(SE3_RECOMPUTE_U='1'):
        on = run()
    assert len(on) == len(off)
    for a, b_ in zip(on, off):
        assert torch.equal(a, b_)
