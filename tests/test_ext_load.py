"""CPU checks of the extension load check in ops/fused.py: a module that
lacks an entry point the package calls is an error at load, with one
message that names what is missing; no extension at all stays `None`."""
import sys
import types

import pytest

from se3_transformer_amd.ops import fused


@pytest.fixture
def fresh_loader(monkeypatch):
    monkeypatch.setattr(fused, '_EXT', None)
    monkeypatch.setattr(fused, '_EXT_ERR', None)
    return monkeypatch


def _stub(names, max_c=fused.NORM_GATED_MAX_C):
    mod = types.ModuleType('se3_transformer_amd._C')
    for n in names:
        setattr(mod, n, lambda *a, **k: None)
    if 'norm_se3_gated_max_c' in names:
        mod.norm_se3_gated_max_c = lambda: max_c
    return mod


def _install(monkeypatch, mod):
    import se3_transformer_amd
    monkeypatch.setitem(sys.modules, 'se3_transformer_amd._C', mod)
    monkeypatch.setattr(se3_transformer_amd, '_C', mod, raising=False)


def test_complete_module_loads(fresh_loader):
    mod = _stub(fused._ENTRY_POINTS)
    _install(fresh_loader, mod)
    assert fused._load_ext() is mod
    assert fused.ext_available() and fused.norm_variants_ok()


def test_stale_module_is_an_error_naming_what_is_missing(fresh_loader):
    stale = [n for n in fused._ENTRY_POINTS
             if n not in ('pack_w_both', 'ubuild_bwd_db')]
    _install(fresh_loader, _stub(stale))
    with pytest.raises(RuntimeError) as ei:
        fused._load_ext()
    msg = str(ei.value)
    assert 'pack_w_both' in msg and 'ubuild_bwd_db' in msg
    assert 'python scripts/build_ext.py' in msg
    assert 'pairconv_fwd' not in msg


def test_gated_channel_ceiling_must_match(fresh_loader):
    _install(fresh_loader, _stub(fused._ENTRY_POINTS, max_c=1024))
    with pytest.raises(RuntimeError, match='norm_se3_gated_max_c'):
        fused._load_ext()


def test_no_extension_is_none(fresh_loader):
    import se3_transformer_amd
    fresh_loader.setitem(sys.modules, 'se3_transformer_amd._C', None)
    fresh_loader.delattr(se3_transformer_amd, '_C', raising=False)
    assert fused._load_ext() is None
    assert not fused.ext_available() and not fused.norm_variants_ok()
    assert not fused.radial_trunk_ok(1, 128) and not fused.egnn_kernels_ok(3)
