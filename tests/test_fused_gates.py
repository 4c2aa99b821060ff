"""CPU checks of the gate layer of ops/fused.py: the switch table, its one
reader, and the order in which a gate looks at things. Tensors "on a GPU" are
stand-ins (a gate asks only is_cuda, dtype, shape, dim and requires_grad)."""
import os
import re
import types

import pytest
import torch

from fused_helpers import (check_switches, gate_calls, install_ext,  # noqa: F401
                           no_switches, stub_ext, switches)
from se3_transformer_amd.ops import fused

README = os.path.join(os.path.dirname(os.path.dirname(__file__)), 'README.md')


def _t(*shape, dtype=torch.float32, cuda=True):
    return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, shape=shape,
                                 dim=lambda: len(shape), requires_grad=False)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_every_switch_is_honoured_and_read_at_call_time(monkeypatch, dtype):
    install_ext(monkeypatch, stub_ext())
    check_switches(lambda *shape, dtype=dtype: _t(*shape, dtype=dtype))
    with switches(SE3_ATTN_MAX_J='9'):
        assert fused.attn_shapes_ok(9, 64) and not fused.attn_shapes_ok(10, 64)
    with pytest.raises(KeyError):
        fused.switch('SE3_NO_SUCH_SWITCH')


def test_pairconv_raises_without_the_extension_the_rest_fall_back(monkeypatch):
    install_ext(monkeypatch, None)
    gates = gate_calls(_t)
    with pytest.raises(RuntimeError, match='python scripts/build_ext.py'):
        gates.pop(None)()
    assert not any(g() for g in gates.values())


def test_the_loader_is_touched_last(monkeypatch):
    monkeypatch.setattr(fused, '_load_ext',
                        lambda: pytest.fail('the extension loader was touched'))
    cpu = gate_calls(lambda *shape, **kw: _t(*shape, cuda=False, **kw))
    assert [key for key, g in cpu.items() if g() is not False] == []
    assert not fused.norm_ok(torch.zeros(1, 4, 8, 3), False, 'gelu')
    assert not fused.sh_basis_ok(torch.zeros(4, 3))
    assert not fused.knn_kernel_ok(torch.zeros(1, 16, 3), 16, 4)
    # nor by a GPU tensor that its switch, dtype or shape sends to eager
    with switches(SE3_EAGER_KNN='1'):
        assert not fused.knn_kernel_ok(_t(64, 3), 64, 8)
    assert not fused.knn_kernel_ok(_t(64, 3, dtype=torch.float64), 64, 8)
    assert not fused.norm_ok(_t(1, 64, fused.NORM_GATED_MAX_C + 1, 3), True, 'gelu')
    assert not fused.norm_ok(_t(1, 64, 64, 3), True, None)
    assert not fused.attn_ok(_t(1, 4, 64, 449, 1), 9, 449)
    # and never by the shape arithmetic
    assert fused.attn_shapes_ok(9, 448, 64) and not fused.attn_shapes_ok(9, 449, 66)
    assert not fused.norm_shapes_ok(fused.NORM_GATED_MAX_C + 1, 3, True)


def test_radial_gate_wants_one_eps_for_both_layernorms(monkeypatch):
    """The kernel takes one eps: a trunk whose two LayerNorms differ in it
    stays eager, decided before the extension is looked at."""
    install_ext(monkeypatch, stub_ext())
    x = _t(512, 3)
    assert fused.radial_ok(x, 128) and fused.radial_ok(x, 128, 1e-6, 1e-6)
    monkeypatch.setattr(fused, '_load_ext',
                        lambda: pytest.fail('the extension loader was touched'))
    assert not fused.radial_ok(x, 128, 1e-5, 1e-6)

    from se3_transformer_amd.models.core import RadialFunc
    seen = []
    monkeypatch.setattr(fused, 'radial_ok',
                        lambda x, mid, *eps: seen.append(eps) or False)
    rp = RadialFunc(1, 1, 1, edge_dim=2)
    rp.net[4].eps = 1e-3
    rp.hidden(torch.zeros(4, 3))
    assert seen == [(1e-5, 1e-3)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('need_x', [False, True])
def test_radial_trunk_of_no_edges_never_reaches_the_extension(monkeypatch,
                                                              dtype, need_x):
    monkeypatch.setattr(fused, '_load_ext',
                        lambda: pytest.fail('the extension loader was touched'))
    from se3_transformer_amd.models.core import RadialFunc
    rp = RadialFunc(1, 1, 1, edge_dim=2)
    params = [p for n, p in rp.named_parameters() if not n.startswith('net.6')]
    x = torch.zeros(0, 3, dtype=dtype, requires_grad=need_x)
    H = fused.radial_trunk(x, *params)
    assert H.shape == (0, 128) and H.dtype == torch.bfloat16
    H.backward(torch.zeros(0, 128, dtype=torch.bfloat16))
    for p in params:
        assert p.grad is not None and p.grad.shape == p.shape
        assert p.grad.dtype == torch.float32 and not p.grad.any()
    if need_x:
        assert x.grad.shape == (0, 3) and x.grad.dtype == dtype
    else:
        assert x.grad is None


def test_readme_lists_exactly_the_switch_table():
    with open(README) as f:
        cells = [line.split('|')[1] for line in f if line.startswith('| `')]
    listed = {n for cell in cells for n in re.findall(r'SE3_[A-Z_]+', cell)}
    assert listed - {'SE3_RES_USAGE'} == set(fused.SWITCHES)   # build-time one
