"""Test helpers for ops/fused.py: flip its runtime switches for a block, and
stand a stub in for the extension module."""
import contextlib
import os
import sys
import types
from unittest import mock

import pytest
import torch

from se3_transformer_amd.ops import fused


@contextlib.contextmanager
def switches(**values):
    """`with switches(SE3_EAGER_NORM='1'):` sets each named switch for the
    block (None unsets it) and puts the previous state back afterwards."""
    assert set(values) <= set(fused.SWITCHES), values
    on = {name: v for name, v in values.items() if v is not None}
    with mock.patch.dict(os.environ, on):        # restores what it found
        for name in set(values) - set(on):
            os.environ.pop(name, None)
        yield


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    """Imported by a test module, starts each of its tests with none set."""
    for name in fused.SWITCHES:
        monkeypatch.delenv(name, raising=False)


def stub_ext(names=fused._ENTRY_POINTS, max_c=fused.NORM_GATED_MAX_C,
             knn_lds=fused.KNN_MAX_LDS, opad=fused.opad):
    """A module with the named entry points as no-ops and the three constant
    getters reporting what is passed (by default what fused.py mirrors)."""
    mod = types.ModuleType('se3_transformer_amd._C')
    for n in names:
        setattr(mod, n, lambda *a, **k: None)
    for n, fn in (('norm_se3_gated_max_c', lambda: max_c),
                  ('knn_max_lds_bytes', lambda: knn_lds),
                  ('pairconv_opad', opad)):
        if n in names:
            setattr(mod, n, fn)
    return mod


def install_ext(monkeypatch, mod):
    """Make `mod` (None: no extension) what fused._load_ext() imports next."""
    import se3_transformer_amd
    monkeypatch.setattr(fused, '_EXT', None)
    monkeypatch.setattr(fused, '_EXT_ERR', None)
    monkeypatch.setitem(sys.modules, 'se3_transformer_amd._C', mod)
    if mod is None:
        monkeypatch.delattr(se3_transformer_amd, '_C', raising=False)
    else:
        monkeypatch.setattr(se3_transformer_amd, '_C', mod, raising=False)


def gate_calls(t):
    """One call per kernel family at the smoke run's shapes (dim 64, heads 4,
    dim_head 16, n 64, k 8; degree 1), keyed by the switch that turns it off.
    t(*shape) makes a tensor of the dtype under test; coordinates and the
    basis stay fp32, and outside autocast pairconv takes bf16 features."""
    f32 = t(512, 3, dtype=torch.float32)
    x16 = t(512, 64, 3, dtype=torch.bfloat16)
    q, qpe, kpe = t(1, 4, 64, 16, 3), t(1, 64, 16), t(1, 64, 8, 16)
    return {
        'SE3_EAGER_NORM': lambda: fused.norm_ok(t(1, 64, 64, 3), True, 'gelu'),
        'SE3_EAGER_RADIAL': lambda: fused.radial_ok(t(512, 1), 128),
        'SE3_EAGER_UBUILD': lambda: fused.ubuild_ok(f32, 64, 3, 3, 3),
        'SE3_EAGER_ATTN': lambda: fused.attn_ok(q, 9, 48),
        'rope': lambda: fused.rope_ok(q, 8, qpe, kpe, True, None),
        'SE3_EAGER_KNN': lambda: fused.knn_kernel_ok(f32, 64, 8),
        'SE3_EAGER_BASIS': lambda: fused.sh_basis_ok(f32),
        'SE3_EAGER_EGNN': lambda: fused.egnn_ok(t(1, 64, 64), 2, 5),
        None: lambda: fused.pairconv_ok(x16, 64, 192, 3, 128),
    }


OFF_SWITCH = {'rope': 'SE3_EAGER_ATTN'}    # the rotary gate has no own switch


def check_switches(t):
    """Every gate is open; what a switch names changes only while that switch
    is '1' (not unset, not '0', not under another switch): read at call time."""
    gates = gate_calls(t)
    x32 = t(512, 64, 3, dtype=torch.float32)         # fp32 outside autocast
    effect = {name: (lambda g=g: not g()) for name, g in gates.items() if name}
    effect['SE3_FORCE_FUSED'] = lambda: fused.pairconv_ok(x32, 64, 192, 3, 128)
    effect['SE3_ATTN_MAX_J'] = lambda: not fused.attn_shapes_ok(2, 64)  # J <= 1
    for name in fused.SWITCHES:
        effect.setdefault(name, lambda name=name: fused.switch_on(name))
    assert gates[None]() and not any(e() for e in effect.values())
    for name in fused.SWITCHES:
        hit = {name}
        if name == 'SE3_ATTN_MAX_J':     # a number: '0' and '1' both cap J,
            hit.add('SE3_EAGER_ATTN')    # which closes the attention gates
        else:
            with switches(**{name: '0'}):
                assert not any(e() for e in effect.values()), name
        with switches(**{name: '1'}):
            for key, e in effect.items():
                assert e() is (OFF_SWITCH.get(key, key) in hit), (name, key)
        assert not any(e() for e in effect.values()), name
