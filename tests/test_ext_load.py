"""CPU checks of the extension load check in ops/fused.py: a module that
lacks an entry point the package calls, or reports a constant other than
the one mirrored in fused.py, is an error at load, with one message that
names what is missing; no extension at all stays `None`."""
import types

import pytest

from fused_helpers import install_ext, stub_ext
from se3_transformer_amd.ops import fused


def test_complete_module_loads(monkeypatch):
    mod = stub_ext()
    install_ext(monkeypatch, mod)
    assert fused._load_ext() is mod
    assert fused.ext_available()


def test_stale_module_is_an_error_naming_what_is_missing(monkeypatch):
    stale = [n for n in fused._ENTRY_POINTS
             if n not in ('pack_w_both', 'ubuild_bwd_db')]
    install_ext(monkeypatch, stub_ext(stale))
    with pytest.raises(RuntimeError) as ei:
        fused._load_ext()
    msg = str(ei.value)
    assert 'pack_w_both' in msg and 'ubuild_bwd_db' in msg
    assert 'python scripts/build_ext.py' in msg
    assert 'pairconv_fwd_opad' not in msg


def test_gated_channel_ceiling_must_match(monkeypatch):
    install_ext(monkeypatch, stub_ext(max_c=1024))
    with pytest.raises(RuntimeError, match='norm_se3_gated_max_c'):
        fused._load_ext()


@pytest.mark.parametrize('stale,named', [
    (dict(knn_lds=32768), 'lacks knn_max_lds_bytes() == 65536;'),
    (dict(opad=lambda O: 8), 'lacks pairconv_opad(1) == 1, pairconv_opad(3) == 4;'),
])
def test_knn_budget_and_opad_must_match(monkeypatch, stale, named):
    install_ext(monkeypatch, stub_ext(**stale))
    with pytest.raises(RuntimeError) as ei:
        fused._load_ext()
    assert named in str(ei.value)
    assert 'python scripts/build_ext.py' in str(ei.value)


def test_no_extension_is_none(monkeypatch):
    install_ext(monkeypatch, None)
    assert fused._load_ext() is None
    assert not fused.ext_available()
    on_gpu = types.SimpleNamespace(is_cuda=True, shape=(4, 1))
    assert not fused.radial_ok(on_gpu, 128)
    assert not fused.egnn_ok(on_gpu, 2, 3)
