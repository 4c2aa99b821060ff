"""Drop-in check: code written against the upstream import paths runs on
THIS framework.

A module alias maps `se3_transformer_pytorch.*` onto `se3_transformer_amd`;
every case below then imports what it needs through the upstream names only
(`from se3_transformer_pytorch import SE3Transformer`,
`se3_transformer_pytorch.basis`, `.irr_repr`, `.spherical_harmonics`,
`.utils`) and asserts the properties the upstream suite is about: basis keys
and shapes, the Q_J intertwiner property, Y(Rx) = D(R)Y(x), the output shape
of every constructor variant and full-model rotation equivariance at the
upstream 1e-4 bound. One case per upstream test, under the upstream test's
name, so a user who swaps the import keeps the same list green.

The cases are self-contained: nothing outside the repository is read.
(Spherical harmonics against an independent oracle live in
tests/test_math.py, which compares with scipy.)
"""
import importlib
import sys
import types

import pytest
import torch


def _alias():
    if 'se3_transformer_pytorch' in sys.modules:
        return
    import se3_transformer_amd as amd
    from se3_transformer_amd import utils as amd_utils
    from se3_transformer_amd.ops import basis as amd_basis
    from se3_transformer_amd.ops import sh as amd_sh
    from se3_transformer_amd.ops import wigner as amd_wig

    pkg = types.ModuleType('se3_transformer_pytorch')
    pkg.__path__ = []
    pkg.SE3Transformer = amd.SE3Transformer

    def sub(name, src, names):
        m = types.ModuleType(f'se3_transformer_pytorch.{name}')
        for n in names:
            if hasattr(src, n):
                setattr(m, n, getattr(src, n))
        sys.modules[f'se3_transformer_pytorch.{name}'] = m
        setattr(pkg, name, m)
        return m

    sub('basis', amd_basis,
        ('get_basis', 'get_R_tensor', 'basis_transformation_Q_J'))
    sub('irr_repr', amd_wig,
        ('irr_repr', 'rot', 'compose', 'spherical_harmonics', 'rot_z',
         'rot_y', 'wigner_d_matrix', 'z_rot_mat', 'x_to_alpha_beta'))
    sub('spherical_harmonics', amd_sh,
        ('clear_spherical_harmonics_cache', 'get_spherical_harmonics',
         'get_spherical_harmonics_element'))
    sub('utils', amd_utils,
        ('torch_default_dtype', 'fourier_encode', 'exists', 'default',
         'batched_index_select', 'masked_mean', 'rand_uniform', 'fast_split',
         'cast_tuple', 'benchmark', 'to_order'))
    m = sub('se3_transformer_pytorch', amd, ())
    m.SE3Transformer = amd.SE3Transformer
    sys.modules['se3_transformer_pytorch'] = pkg


def _up(name=None):
    """Import through the upstream name."""
    _alias()
    return importlib.import_module(
        'se3_transformer_pytorch' + ('.' + name if name else ''))


# ---- basis / irreps ------------------------------------------------------

def _basis():
    get_basis = _up('basis').get_basis
    max_degree = 3
    basis = get_basis(torch.randn(2, 8, 4, 3), max_degree)
    assert len(basis.keys()) == (max_degree + 1) ** 2
    for d_in in range(max_degree + 1):
        for d_out in range(max_degree + 1):
            v = basis[f'{d_in},{d_out}']
            assert v.shape[-4:] == (2 * d_out + 1, 1, 2 * d_in + 1,
                                    2 * min(d_in, d_out) + 1)
            assert torch.isfinite(v).all()


def _basis_transformation_Q_J():
    b, ir, ut = _up('basis'), _up('irr_repr'), _up('utils')
    with ut.torch_default_dtype(torch.float64):
        g = torch.Generator().manual_seed(5)
        angles = torch.rand(4, 3, generator=g, dtype=torch.float64)
        for J, order_in, order_out in ((1, 1, 1), (0, 1, 1), (2, 1, 1),
                                       (3, 2, 1), (2, 2, 2)):
            q_j = b.basis_transformation_Q_J(J, order_in, order_out).double()
            assert q_j.shape == (ut.to_order(order_out) * ut.to_order(order_in),
                                 ut.to_order(J))
            for a, be, c in angles:
                lhs = b.get_R_tensor(order_out, order_in, a, be, c) @ q_j
                rhs = q_j @ ir.irr_repr(J, a, be, c).double()
                assert torch.allclose(lhs, rhs, atol=1e-6), (J, order_in, order_out)


def _irr_repr():
    ir, ut = _up('irr_repr'), _up('utils')
    with ut.torch_default_dtype(torch.float64):
        g = torch.Generator().manual_seed(17)
        for order in range(1, 7):
            a, b = torch.rand(2, generator=g, dtype=torch.float64)
            alpha, beta, gamma = torch.rand(3, generator=g, dtype=torch.float64)
            ra, rb, _ = ir.compose(alpha, beta, gamma, a, b, 0)
            y_rx = ir.spherical_harmonics(order, ra, rb)
            d_y = ir.irr_repr(order, alpha, beta, gamma) @ \
                ir.spherical_harmonics(order, a, b)
            assert y_rx.shape == (ut.to_order(order),)
            d, r = (y_rx - d_y).abs().max(), d_y.abs().max()
            assert d < 1e-10 * r, (order, (d / r).item())


# ---- model variants ------------------------------------------------------

def _inputs(n=32, dim=64, batch=1):
    return (torch.randn(batch, n, dim), torch.randn(batch, n, 3),
            torch.ones(batch, n).bool())


def _shape_case(ctor, fwd=None, return_type=0, want=(1, 32, 64)):
    def run():
        model = _up().SE3Transformer(**ctor)
        feats, coors, mask = _inputs()
        out = model(feats, coors, mask, return_type=return_type,
                    **(fwd() if fwd else {}))
        assert out.shape == want
        assert torch.isfinite(out).all()
    return run


def _equiv_case(ctor, fwd=None, dtype=torch.float32, type_one_input=False):
    def run():
        rot = _up('irr_repr').rot
        with _up('utils').torch_default_dtype(dtype):
            model = _up().SE3Transformer(**ctor)
            feats, coors, mask = _inputs()
            R = rot(*torch.tensor([15., 0., 45.], dtype=dtype)).to(dtype)
            kw = fwd() if fwd else {}
            if type_one_input:
                vec = torch.randn(1, 32, 64, 3)
                f1 = {'0': feats[..., None], '1': vec @ R}
                f2 = {'0': feats[..., None], '1': vec}
            else:
                f1 = f2 = feats
            out1 = model(f1, coors @ R, mask, return_type=1, **kw)
            out2 = model(f2, coors, mask, return_type=1, **kw) @ R
            assert out1.shape == (1, 32, 64, 3)
            diff = (out1 - out2).abs().max()
            assert diff < 1e-4, f'not equivariant: {diff}'
    return run


def _different_input_dimensions_for_types():
    model = _up().SE3Transformer(dim_in=(4, 2), dim=4, depth=1, input_degrees=2,
                                 num_degrees=2, output_degrees=2,
                                 reduce_dim_out=True)
    feats = {'0': torch.randn(2, 32, 4, 1), '1': torch.randn(2, 32, 2, 3)}
    coors = torch.randn(2, 32, 3)
    refined = coors + model(feats, coors, torch.ones(2, 32).bool(), return_type=1)
    assert refined.shape == coors.shape and torch.isfinite(refined).all()


def _continuous_edges():
    fourier_encode = _up('utils').fourier_encode
    values = torch.randint(0, 4, (1, 32, 32, 2))
    return dict(edges=fourier_encode(values, num_encodings=8, include_self=True))


def _chain_adjacency():
    i = torch.arange(32)
    return dict(adj_mat=(i[:, None] - i[None, :]).abs() <= 1)


_BASE = dict(dim=64, depth=1, num_degrees=2, num_neighbors=4, valid_radius=10)
_EQ = dict(dim=64, depth=1, attend_self=True, num_neighbors=4, num_degrees=2,
           output_degrees=2)
_GLOBAL = lambda: dict(global_feats=torch.randn(1, 2, 16))  # noqa: E731

CASES = {
    'test_basis::test_basis': _basis,
    'test_basis::test_basis_transformation_Q_J': _basis_transformation_Q_J,
    'test_irrep_repr::test_irr_repr': _irr_repr,
    'test_equivariance::test_transformer': _shape_case(_BASE),
    'test_equivariance::test_causal_se3_transformer':
        _shape_case(dict(_BASE, causal=True)),
    'test_equivariance::test_se3_transformer_with_global_nodes':
        _shape_case(dict(_BASE, global_feats_dim=16), _GLOBAL),
    'test_equivariance::test_one_headed_key_values_se3_transformer_with_global_nodes':
        _shape_case(dict(_BASE, global_feats_dim=16, one_headed_key_values=True),
                    _GLOBAL),
    'test_equivariance::test_transformer_with_edges':
        _shape_case(dict(dim=64, depth=1, num_degrees=2, num_neighbors=4,
                         edge_dim=4, num_edge_tokens=4),
                    lambda: dict(edges=torch.randint(0, 4, (1, 32, 32)))),
    'test_equivariance::test_transformer_with_continuous_edges':
        _shape_case(dict(dim=64, depth=1, attend_self=True, num_degrees=2,
                         output_degrees=2, edge_dim=34),
                    _continuous_edges, return_type=1, want=(1, 32, 64, 3)),
    'test_equivariance::test_different_input_dimensions_for_types':
        _different_input_dimensions_for_types,
    'test_equivariance::test_equivariance':
        _equiv_case(dict(_EQ, fourier_encode_dist=True)),
    'test_equivariance::test_equivariance_with_egnn_backbone':
        _equiv_case(dict(_EQ, fourier_encode_dist=True, use_egnn=True)),
    'test_equivariance::test_rotary':
        _equiv_case(dict(_EQ, fourier_encode_dist=True, rotary_position=True,
                         rotary_rel_dist=True)),
    'test_equivariance::test_equivariance_linear_proj_keys':
        _equiv_case(dict(_EQ, fourier_encode_dist=True, linear_proj_keys=True)),
    'test_equivariance::test_equivariance_only_sparse_neighbors':
        _equiv_case(dict(dim=64, depth=1, attend_self=True, num_degrees=2,
                         output_degrees=2, num_neighbors=0,
                         attend_sparse_neighbors=True, num_adj_degrees=2,
                         adj_dim=4),
                    _chain_adjacency, dtype=torch.float64),
    'test_equivariance::test_equivariance_with_reversible_network':
        _equiv_case(dict(_EQ, reversible=True)),
    'test_equivariance::test_equivariance_with_type_one_input':
        _equiv_case(dict(_EQ, input_degrees=2), type_one_input=True),
}


@pytest.mark.parametrize('case', list(CASES), ids=list(CASES))
def test_reference_suite(case):
    CASES[case]()
