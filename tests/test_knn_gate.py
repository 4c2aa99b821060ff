"""CPU checks of `fused.knn_ok`, the pure-Python gate of the kNN kernel:
any 1 <= k <= n-1 whose LDS footprint, min(k, ceil(n/64)) * 512 + 4k bytes
(64 sorted lists of (distance, index) pairs plus the k winners), fits
KNN_MAX_LDS."""
import pytest

from fused_helpers import install_ext, stub_ext
from se3_transformer_amd.ops import fused


@pytest.mark.parametrize('n,k,expected', [
    (66, 65, True),
    (1024, 1023, True),
    (4096, 4095, True),
    (50, 6, True),
    (50, 50, False),            # k > n - 1
    (50, 0, False),
    (100000, 99999, False),     # LDS
])
def test_knn_ok_table(n, k, expected):
    assert fused.knn_ok(n, k) is expected


def test_knn_ok_matches_lds_formula():
    assert fused.KNN_MAX_LDS == 64 * 1024
    for n in (2, 3, 64, 65, 66, 129, 1000, 4096, 5300, 5400, 5500, 6000,
              20000):
        for k in (0, 1, 2, 63, 64, 65, 128, 1000, n - 2, n - 1, n, n + 1):
            lds = min(k, -(-n // 64)) * 512 + 4 * k
            want = 1 <= k <= n - 1 and lds <= fused.KNN_MAX_LDS
            assert fused.knn_ok(n, k) is want, (n, k)


def test_stale_budget_is_an_error_on_first_use(monkeypatch):
    """KNN_MAX_LDS must be the budget the built kernel enforces: a module
    that reports another one is refused at load, before its kernel is
    called."""
    called = []
    mod = stub_ext(knn_lds=32768)
    mod.knn_graph = lambda *a: called.append(a)
    install_ext(monkeypatch, mod)
    with pytest.raises(RuntimeError, match='knn_max_lds_bytes'):
        fused.knn_graph(*[None] * 11)
    assert not called
    mod.knn_max_lds_bytes = lambda: fused.KNN_MAX_LDS
    fused.knn_graph(*[None] * 11)
    assert len(called) == 1 and fused._load_ext() is mod


def test_budget_boundary():
    """k = n-1: 8 * ceil(n/64) * 64 + 4(n-1) bytes; the largest n inside
    64 KiB is 5440 (85 * 512 + 4 * 5439 = 65276; n = 5441 has L = 86)."""
    assert fused.knn_ok(5440, 5439)
    assert not fused.knn_ok(5441, 5440)
