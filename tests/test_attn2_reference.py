"""CPU tests that keep the attn2 reference (tests/attn2_ref.py) honest.

1. The reference agrees with AttentionSE3 / OneHeadedKVAttentionSE3 run on
   the CPU in f64 (their einsum branch), with q/k/v/mask assembled here the
   way models/attention.py assembles them for the kernel.
2. Every edge the GPU cases of test_attn2_gpu.py aim at can actually be
   seen by them: a mutant of the REFERENCE (one step broken the way a
   kernel could be) differs from the true reference, on the case's exact
   inputs, by at least 10x the widest band the GPU test may use there.
   The kernel is neither mutated nor run.
"""
import pytest
import torch
import torch.nn.functional as F

import attn2_cases as C
import attn2_ref as A


def _rel_err(a, b):
    denom = b.abs().max().clamp(min=1e-6)
    return ((a - b).abs().max() / denom).item()


# ---- 1. reference vs module -------------------------------------------------

def _module_inputs(b, n, kn, dim, gen):
    nbr_idx = torch.randint(0, n, (b, n, kn), generator=gen)
    nbr_mask = torch.rand(b, n, kn, generator=gen) > 0.3
    rel_dist = torch.rand(b, n, kn, generator=gen, dtype=torch.float64) * 3
    basis = {}
    for di in (0, 1):
        for do in (0, 1):
            basis[(di, do)] = torch.randn(
                b, n, kn, 2 * do + 1, 2 * di + 1, 2 * min(di, do) + 1,
                generator=gen, dtype=torch.float64)
    feats = {'0': torch.randn(b, n, dim, 1, generator=gen,
                              dtype=torch.float64),
             '1': torch.randn(b, n, dim, 3, generator=gen,
                              dtype=torch.float64)}
    return nbr_idx, nbr_mask, rel_dist, basis, feats


def _via_reference(attn, one_headed, feats, edge_info, rel_dist, basis,
                   pos_emb):
    """The module's forward with the attention core replaced by the
    reference: q/k/v/mask laid out as for fused.fused_attention, rotary
    tables passed raw."""
    h = attn.heads
    nbr_idx, nbr_mask, _ = edge_info
    queries = attn.to_q(feats)
    values = attn.to_v(feats, edge_info, rel_dist, basis)
    keys = attn.to_k(feats, edge_info, rel_dist, basis)
    if attn.attend_self:
        self_k, self_v = attn.to_self_k(feats), attn.to_self_v(feats)
    outputs = {}
    for deg in feats:
        q, k, v = queries[deg], keys[deg], values[deg]
        b, n, m = q.shape[0], q.shape[1], q.shape[-1]
        q = q.view(b, n, h, -1, m).permute(0, 2, 1, 3, 4)       # b h i d m
        d = q.shape[3]
        if one_headed:                                           # b i j d m
            if attn.attend_self:
                k = torch.cat((self_k[deg].unsqueeze(2), k), dim=2)
                v = torch.cat((self_v[deg].unsqueeze(2), v), dim=2)
        else:                                                  # b h i j d m
            k = k.view(b, n, k.shape[2], h, -1, m).permute(0, 3, 1, 2, 4, 5)
            v = v.view(b, n, v.shape[2], h, -1, m).permute(0, 3, 1, 2, 4, 5)
            if attn.attend_self:
                sk = self_k[deg].view(b, n, h, -1, m).permute(0, 2, 1, 3, 4)
                sv = self_v[deg].view(b, n, h, -1, m).permute(0, 2, 1, 3, 4)
                k = torch.cat((sk.unsqueeze(3), k), dim=3)
                v = torch.cat((sv.unsqueeze(3), v), dim=3)
        jdim = 2 if one_headed else 3
        qf = kf = None
        if pos_emb is not None and deg == '0':
            qpe, kpe = pos_emb
            assert kpe.shape[2] == k.shape[jdim]
            qf = qpe.reshape(-1, qpe.shape[-1])
            kf = kpe.reshape(-1, kpe.shape[2], kpe.shape[-1])
        if attn.use_null_kv:
            nk, nv = attn.null_keys[deg], attn.null_values[deg]
            if one_headed:
                nk = nk.view(1, 1, 1, -1, m).expand(b, n, 1, -1, m)
                nv = nv.view(1, 1, 1, -1, m).expand(b, n, 1, -1, m)
            else:
                nk = nk.view(1, h, 1, 1, -1, m).expand(b, h, n, 1, -1, m)
                nv = nv.view(1, h, 1, 1, -1, m).expand(b, h, n, 1, -1, m)
            k = torch.cat((nk, k), dim=jdim)
            v = torch.cat((nv, v), dim=jdim)
        J = k.shape[jdim]
        mask_u8 = F.pad(nbr_mask, (J - nbr_mask.shape[-1], 0), value=True) \
            .to(torch.uint8)
        out = A.attn2_reference(
            q.reshape(b * h * n, d * m), k.reshape(-1, J, d * m),
            v.reshape(-1, J, d * m), mask_u8, n, h, attn.scale,
            kv_one=one_headed, qf=qf, kf=kf)
        outputs[deg] = out.view(b, h, n, d, m).permute(0, 2, 1, 3, 4) \
            .reshape(b, n, -1, m)
    return attn.to_out(outputs)


@pytest.mark.parametrize('one_headed', [False, True])
@pytest.mark.parametrize('variant', ['bare-masked-row', 'self-null-rotary'])
def test_reference_matches_module_f64(one_headed, variant):
    from se3_transformer_amd.models.attention import (
        AttentionSE3, OneHeadedKVAttentionSE3)
    from se3_transformer_amd.models.fiber import Fiber

    gen = torch.Generator().manual_seed(3)
    b, n, kn, dim, dim_head, heads = 2, 6, 5, 8, 4, 2
    rich = variant == 'self-null-rotary'
    klass = OneHeadedKVAttentionSE3 if one_headed else AttentionSE3
    attn = klass(Fiber([(0, dim), (1, dim)]), dim_head=dim_head, heads=heads,
                 attend_self=rich, use_null_kv=rich).double()
    with torch.no_grad():
        for p in attn.parameters():     # null keys start at zero: fill them
            p.copy_(torch.randn(p.shape, generator=gen, dtype=p.dtype) * 0.5)
    nbr_idx, nbr_mask, rel_dist, basis, feats = _module_inputs(
        b, n, kn, dim, gen)
    pos_emb = None
    if rich:
        j_pre = kn + 1
        pos_emb = (torch.randn(b, n, dim_head, generator=gen,
                               dtype=torch.float64) * 2,
                   torch.randn(b, n, j_pre, dim_head, generator=gen,
                               dtype=torch.float64) * 2)
    else:
        nbr_mask[0, 2] = False          # class defaults: an all-masked row
        nbr_mask[1, n - 1] = False
    edge_info = (nbr_idx, nbr_mask, None)
    gout = {k_: torch.randn(t.shape, generator=gen, dtype=torch.float64)
            for k_, t in feats.items()}

    res = []
    for via_ref in (False, True):
        fs = {k_: t.clone().requires_grad_(True) for k_, t in feats.items()}
        if via_ref:
            out = _via_reference(attn, one_headed, fs, edge_info, rel_dist,
                                 basis, pos_emb)
        else:
            out = attn(fs, edge_info, rel_dist, basis, pos_emb=pos_emb)
        loss = sum((out[k_] * gout[k_]).sum() for k_ in out)
        grads = torch.autograd.grad(loss, [fs['0'], fs['1']])
        res.append((out['0'].detach(), out['1'].detach(), *grads))
    for name, mod, ref in zip(('out0', 'out1', 'g0', 'g1'), *res):
        assert mod.abs().max() > 1e-3, name
        err = _rel_err(ref, mod)
        assert err < 1e-10, f'{name}: {err}'


def test_rope_formula_against_explicit_loop():
    """rope() against the pairing formula written out element by element."""
    gen = torch.Generator().manual_seed(4)
    for rot, DM in ((2, 2), (6, 9), (64, 64)):
        t = torch.randn(3, DM, generator=gen, dtype=torch.float64)
        f = torch.randn(3, rot, generator=gen, dtype=torch.float64) * 3
        want = t.clone()
        for d in range(rot):
            first = d < rot // 2
            p = 2 * d + 1 if first else 2 * d - rot
            want[:, d] = t[:, d] * f[:, d].cos() \
                + (-1 if first else 1) * t[:, p] * f[:, d].sin()
        assert torch.allclose(A.rope(t, f), want, rtol=0, atol=1e-14)


# ---- 2. every edge case discriminates ---------------------------------------

def _mutant_forward(name, inp):
    """fn(q, k, v) -> out: the reference with one step broken."""
    n, h, scale, kv_one = inp['n'], inp['heads'], inp['scale'], inp['kv_one']

    def fn(q, k, v):
        q5, k5, v5, m5, qf5, kf5 = A.unflatten(
            q, k, v, inp['mask'], inp['qf'], inp['kf'], n, h, kv_one)
        b, J = q5.shape[0], k5.shape[-2]
        P = None
        if name == 'drop_last_key':
            keep = torch.arange(J) != J - 1
            m5 = keep.expand(b, 1, n, J) if m5 is None else m5 & keep
        elif name == 'mask_shift':
            m5 = torch.roll(m5, 1, dims=-1)
        elif name == 'zero_chunk':
            q5 = torch.cat((q5[..., :64], 0 * q5[..., 64:]), dim=-1)
            v5 = torch.cat((v5[..., :64], 0 * v5[..., 64:]), dim=-1)
        elif name == 'pair_xor':
            P = torch.arange(inp['rot']) ^ 1
        elif name == 'head_in_bi':
            # the (b, i) row looked up with r % (b n) instead of b n + i
            r = torch.arange(b * h * n) % (b * n)
            m5 = m5.reshape(b * n, J)[r].view(b, h, n, J)
            if kv_one:
                k5 = k5.reshape(b * n, J, -1)[r].view(b, h, n, J, -1)
                v5 = v5.reshape(b * n, J, -1)[r].view(b, h, n, J, -1)
        if qf5 is not None:
            q5 = A.rope(q5, qf5.to(q.dtype), P)
        if kf5 is not None:
            kf5 = kf5.to(q.dtype)
            if name == 'rope_first_keys':
                jr = kf5.shape[-2]
                first = lambda t: torch.cat(
                    (A.rope(t[..., :jr, :], kf5), t[..., jr:, :]), dim=-2)
                k5, v5 = first(k5), first(v5)
            else:
                k5 = A.rope_last(k5, kf5, P)
                if name != 'no_rope_v':
                    v5 = A.rope_last(v5, kf5, P)
        return A.attend(q5, k5, v5, m5, scale).reshape(q.shape)
    return fn


def _manual_backward(inp, ones_on_dead_rows=False, keep_masked_ds=False):
    """The kernel's backward recipe (a_j from the saved lse, delta, ds) in
    f64, no rotary. With both flags off it must equal autograd; the flags
    are the two halves of the fully-masked-row defect."""
    n, h, scale, kv_one = inp['n'], inp['heads'], inp['scale'], inp['kv_one']
    q, k, v, g = (inp[x].double() for x in ('q', 'k', 'v', 'g'))
    q5, k5, v5, m5, _, _ = A.unflatten(q, k, v, inp['mask'], None, None,
                                       n, h, kv_one)
    g5 = g.view(q5.shape)
    sim = (q5.unsqueeze(-2) * k5).sum(-1) * scale
    sim = sim.masked_fill(~m5, A.MASK_FILL)
    a = sim.softmax(-1)                         # 1/J on an all-masked row
    dead = ~m5.any(-1, keepdim=True)
    if ones_on_dead_rows:
        a = torch.where(dead, torch.ones_like(a), a)
    out = A.attend(q5, k5, v5, m5, scale)
    delta = (g5 * out).sum(-1, keepdim=True)
    ds = a * ((g5.unsqueeze(-2) * v5).sum(-1) - delta) * scale
    if not keep_masked_ds:
        ds = ds.masked_fill(~m5, 0.)
    dq = (ds.unsqueeze(-1) * k5).sum(-2)
    dk = ds.unsqueeze(-1) * q5.unsqueeze(-2)
    dv = a.unsqueeze(-1) * g5.unsqueeze(-2)
    if kv_one:
        dk, dv = dk.sum(1), dv.sum(1)
    return out.reshape(q.shape), dq.reshape(q.shape), dk.reshape(k.shape), \
        dv.reshape(v.shape)


# mutant -> (tensor it must move, the cases it applies to)
def _applies(mut, c):
    if mut == 'drop_last_key':
        return c.id.startswith('j') and c.J > 1
    if mut == 'mask_shift':
        return c.id.startswith(('mask-', 'rows-')) or c.id == 'logit60'
    if mut == 'zero_chunk':
        return c.DM > 64
    if mut == 'pair_xor':
        return c.rot > 2            # at rot = 2 both pairings coincide
    if mut == 'rope_first_keys':
        return c.rope in ('k', 'both') and c.jr < c.J
    if mut == 'no_rope_v':
        return c.rope in ('k', 'both')
    if mut == 'head_in_bi':
        return c.id.startswith('rows-') and c.heads > 1
    if mut in ('dead_row_weight_one', 'masked_ds_kept'):
        return c.mask in ('full_mid', 'full_last')
    raise KeyError(mut)


MUTANTS = {'drop_last_key': 'dv', 'mask_shift': 'out', 'zero_chunk': 'out',
           'pair_xor': 'out', 'rope_first_keys': 'out', 'no_rope_v': 'out',
           'head_in_bi': 'out', 'dead_row_weight_one': 'dv',
           'masked_ds_kept': 'dk'}
PAIRS = [(m, c.id) for m in MUTANTS for c in C.CASES if _applies(m, c)]


def _widest_band(case, tensor):
    """No GPU band for this case can be wider: the cap, plus one bf16
    rounding for a gradient of bf16 inputs."""
    cap_fwd, cap_grad = C.caps(case)
    return cap_fwd if tensor == 'out' else cap_grad + C.BF16_ULP


@pytest.mark.parametrize('mutant,case_id', PAIRS)
def test_case_tells_mutant_from_reference(mutant, case_id):
    case = C.BY_ID[case_id]
    tensor = MUTANTS[mutant]
    idx = ('out', 'dq', 'dk', 'dv').index(tensor)
    for kv_one in (False, True):
        for dtype in (torch.float32, torch.bfloat16):
            inp = C.make_inputs(case, kv_one, dtype)
            inp['rot'] = case.rot
            ref = A.reference_with_grads(
                inp['q'], inp['k'], inp['v'], inp['mask'], inp['n'],
                inp['heads'], inp['scale'], kv_one, inp['qf'], inp['kf'],
                inp['g'])
            if mutant == 'dead_row_weight_one':
                mut = _manual_backward(inp, ones_on_dead_rows=True)
            elif mutant == 'masked_ds_kept':
                mut = _manual_backward(inp, keep_masked_ds=True)
            else:
                mut = A.with_grads(_mutant_forward(mutant, inp), inp['q'],
                                   inp['k'], inp['v'], inp['g'])
            gap = _rel_err(mut[idx], ref[idx])
            need = 10 * _widest_band(case, tensor)
            assert gap >= need, (f'{mutant} on {case_id} kv_one={kv_one} '
                                 f'{dtype}: {tensor} moves {gap:.3g}, '
                                 f'needs {need:.3g}')


@pytest.mark.parametrize('case_id', ['mask-full_mid', 'mask-full_last',
                                     'mask-one_first', 'j65-dm48'])
@pytest.mark.parametrize('kv_one', [False, True])
def test_manual_backward_is_autograd(case_id, kv_one):
    """The hand-written backward the two gradient mutants are cut from is,
    unmutated, the autograd gradient of the reference."""
    inp = C.make_inputs(C.BY_ID[case_id], kv_one, torch.float32)
    ref = A.reference_with_grads(
        inp['q'], inp['k'], inp['v'], inp['mask'], inp['n'], inp['heads'],
        inp['scale'], kv_one, None, None, inp['g'])
    for name, a, b in zip(('out', 'dq', 'dk', 'dv'), _manual_backward(inp),
                          ref):
        assert _rel_err(a, b) < 1e-12, name


def test_fully_masked_row_semantics():
    """What the issue fixes in the kernel, stated on the reference: mean of
    v forward, dv_j = g/J, dq = 0, dk_j = 0 on the dead rows."""
    case = C.BY_ID['mask-full_mid']
    inp = C.make_inputs(case, False, torch.float32)
    out, dq, dk, dv = A.reference_with_grads(
        inp['q'], inp['k'], inp['v'], inp['mask'], inp['n'], inp['heads'],
        inp['scale'], False, None, None, inp['g'])
    rows = [(bh * case.n + 1) for bh in range(case.heads)]   # b = 0, i = 1
    assert not inp['mask'][0, 1].any()
    for r in rows:
        assert torch.allclose(out[r], inp['v'][r].double().mean(0),
                              rtol=0, atol=1e-14)
        assert torch.allclose(dv[r], (inp['g'][r].double() / case.J)
                              .expand(case.J, -1), rtol=0, atol=1e-15)
        assert dq[r].abs().max() == 0 and dk[r].abs().max() == 0


def test_case_properties():
    """The cases are what their names say."""
    ids = [c.id for c in C.CASES]
    assert len(set(ids)) == len(ids)
    assert sum(c.R % 4 != 0 for c in C.CASES if c.id.startswith('rows-')) >= 2
    for c in C.CASES:
        assert c.R <= 200
    # logit60: |logit| reaches 60 in every row, mostly in the second tile
    for kv_one in (False, True):
        inp = C.make_inputs(C.BY_ID['logit60'], kv_one, torch.float32)
        q5, k5, _, _, _, _ = A.unflatten(
            inp['q'].double(), inp['k'].double(), inp['v'].double(), None,
            None, None, inp['n'], inp['heads'], kv_one)
        sim = (q5.unsqueeze(-2) * k5).sum(-1) * inp['scale']
        top = sim.abs().amax(-1)
        assert (top - 60).abs().max() < 1e-3
        arg = sim.argmax(-1).flatten()
        in_tile1 = ((arg >= 64) & (arg < 128)).float().mean()
        assert in_tile1 >= 0.5, in_tile1
        assert sim.amax(-1).max() > 50
    # seq4096: arguments reach 4096 and keep the 1/10000^(2i/d) spread
    inp = C.make_inputs(C.BY_ID['ropebig64-dm64-j66'], False, torch.float32)
    assert inp['qf'].abs().max() == 4096 and inp['kf'].abs().max() == 4096
    assert inp['kf'][..., -1].abs().max() < 1.
    # the hand-built masks
    m = C.make_inputs(C.BY_ID['mask-full_last'], False, torch.float32)['mask']
    assert not m[-1, -1].any() and m[:-1].any(-1).all()
    m = C.make_inputs(C.BY_ID['mask-one_last'], False, torch.float32)['mask']
    assert (m[:, 1::2].sum(-1) == 1).all() and m[:, 1::2, -1].all()
    m = C.make_inputs(C.BY_ID['mask-tile0_masked'], False,
                      torch.float32)['mask']
    assert not m[:, 1::2, :64].any() and m[:, 1::2, 64:].any(-1).all()
    m = C.make_inputs(C.BY_ID['mask-tile1_masked'], False,
                      torch.float32)['mask']
    assert not m[:, 1::2, 64:].any() and m[:, 1::2, :64].any(-1).all()
