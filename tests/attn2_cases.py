"""The kernel-level attn2 cases, shared by test_attn2_gpu.py (which runs
the kernel on them) and test_attn2_reference.py (which proves, on the very
same inputs and without a GPU, that each case can tell a broken kernel from
a right one). Inputs are drawn on the CPU from a generator seeded by the
case id, so both files see the same numbers."""
import math
import zlib
from dataclasses import dataclass

import torch

# ---- bands -----------------------------------------------------------------
# band = min(margin * max(e32, 1e-7), cap); e32 is the error of the same
# formula evaluated in fp32 torch on the device against the f64 reference.
# Margins: twice the largest kernel_err / max(e32, 1e-7) measured over all
# cases with fp32 arithmetic on both sides (profiles/attn2_parity.md):
# 3.92 forward, 7.73 gradients; 1274 and 1051 where the rotary arguments
# reach 4096 (__sinf/__cosf lose absolute accuracy there, torch's cos/sin
# do not). Caps: what the suite already asserted for this kernel before
# these tests existed; they are conditions, not measurements.
MARGIN_FWD = 7.84
MARGIN_GRAD = 15.5
MARGIN_BIGF_FWD = 2547.
MARGIN_BIGF_GRAD = 2103.
E32_FLOOR = 1e-7
BF16_ULP = 2.0 ** -8      # one bf16 rounding of a gradient, rel. to its max


def caps(case):
    """(forward cap, gradient cap) for fp32 inputs."""
    if case.fmode == 'seq4096':
        return 2e-3, 5e-3
    if case.J <= 64:
        return 1e-4, 1e-3
    return 2e-3, 2e-3


def margins(case):
    if case.fmode == 'seq4096':
        return MARGIN_BIGF_FWD, MARGIN_BIGF_GRAD
    return MARGIN_FWD, MARGIN_GRAD


@dataclass(frozen=True)
class Case:
    id: str
    J: int
    DM: int
    b: int = 2
    heads: int = 3
    n: int = 7
    mask: str = 'rand'      # rand | none | full_mid | full_last | one_first
    #                         | one_last | tile0_masked | tile1_masked
    rot: int = 0
    jr: int = 0
    rope: str = ''          # '' | q | k | both
    fmode: str = 'pi'       # pi: U[-pi, pi];  seq4096: position * inv_freq
    big_logits: bool = False

    @property
    def R(self):
        return self.b * self.heads * self.n


def _cases():
    out = []
    for DM in (1, 24, 63, 64, 65, 128, 192, 320, 385, 448):
        out.append(Case(f'dm{DM}', J=9, DM=DM))
    for DM in (48, 192):
        for J in (1, 63, 64, 65, 128, 129):
            out.append(Case(f'j{J}-dm{DM}', J=J, DM=DM))
    for b, h, n in ((1, 1, 5), (2, 3, 7), (3, 2, 1)):
        out.append(Case(f'rows-b{b}h{h}n{n}', J=9, DM=24, b=b, heads=h, n=n))
    out.append(Case('nomask', J=9, DM=24, mask='none'))
    for kind in ('full_mid', 'full_last', 'one_first', 'one_last',
                 'tile0_masked', 'tile1_masked'):
        out.append(Case(f'mask-{kind}', J=70, DM=24, mask=kind))
    for rot, DM in ((2, 2), (16, 16), (16, 24), (64, 64), (64, 128)):
        for J in (5, 66):
            for pre in (0, 1, 3):
                for which in ('q', 'k', 'both'):
                    out.append(Case(f'rope{rot}-dm{DM}-j{J}-pre{pre}-{which}',
                                    J=J, DM=DM, rot=rot, jr=J - pre,
                                    rope=which))
    out.append(Case('ropebig64-dm64-j66', J=66, DM=64, rot=64, jr=65,
                    rope='both', fmode='seq4096'))
    out.append(Case('ropebig16-dm24-j5', J=5, DM=24, rot=16, jr=4,
                    rope='both', fmode='seq4096'))
    out.append(Case('logit60', J=130, DM=48, big_logits=True))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def _mask(case, gen):
    b, n, J = case.b, case.n, case.J
    if case.mask == 'none':
        return None
    # a different draw per (b, i): a wrong mask row shows at once
    m = torch.rand(b, n, J, generator=gen) > 0.3
    if case.mask == 'full_mid':
        m[0, 1] = False              # rows r = 1 (+ n per head): mid-block
    elif case.mask == 'full_last':
        m[b - 1, n - 1] = False      # includes the very last row R-1
    elif case.mask in ('one_first', 'one_last'):
        m[:, 1::2] = False           # odd nodes keep exactly one key
        m[:, 1::2, 0 if case.mask == 'one_first' else J - 1] = True
    elif case.mask == 'tile0_masked':
        m[:, 1::2, :64] = False      # odd nodes: first 64-key tile dark
        m[:, 1::2, 64] = True
    elif case.mask == 'tile1_masked':
        m[:, 1::2, 64:] = False
        m[:, 1::2, 0] = True
    return m.to(torch.uint8)


def _freqs(case, shape, gen):
    rot = case.rot
    if case.fmode == 'pi':
        return (torch.rand(*shape, rot, generator=gen) * 2 - 1) * math.pi
    # SinusoidalEmbeddings at positions of a 4096-long sequence
    pos = (torch.rand(*shape, generator=gen) * 2 - 1) * 4096
    pos[..., 0] = 4096.                     # the extreme is always present
    inv_freq = 1. / (10000 ** (torch.arange(0, rot, 2).float() / rot))
    return (pos[..., None] * inv_freq).repeat_interleave(2, dim=-1)


def make_inputs(case, kv_one, dtype):
    """CPU tensors: q, k, v in `dtype` (fp32 or bf16; bf16 = fp32 draw
    rounded once), mask u8 or None, qf/kf fp32 or None, g fp32."""
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    b, h, n, J, DM = case.b, case.heads, case.n, case.J, case.DM
    R, Rkv = case.R, (b * n if kv_one else case.R)
    q = torch.randn(R, DM, generator=gen)
    k = torch.randn(R, J, DM, generator=gen)
    v = torch.randn(R, J, DM, generator=gen)
    g = torch.randn(R, DM, generator=gen)
    mask = _mask(case, gen)
    qf = kf = None
    if case.rope in ('q', 'both'):
        qf = _freqs(case, (b * n,), gen)
    if case.rope in ('k', 'both'):
        kf = _freqs(case, (b * n, case.jr), gen)
    if kv_one:      # head 0 of every batch element provides the shared rows
        k = k.view(b, h, n, J, DM)[:, 0].reshape(Rkv, J, DM).contiguous()
        v = v.view(b, h, n, J, DM)[:, 0].reshape(Rkv, J, DM).contiguous()
    scale = DM ** -0.5
    if case.big_logits:
        # keys of the second tile twice as long, so the row maximum falls
        # there; then each q row stretched until its largest |logit| is 60
        k[:, 64:128] *= 2
        kk = k.view(b, 1 if kv_one else h, n, J, DM).double()
        sim = (q.view(b, h, n, 1, DM).double() * kk).sum(-1) * scale
        q = q * (60. / sim.abs().amax(-1)).reshape(R, 1).float()
    q, k, v = (t.to(dtype) for t in (q, k, v))
    return dict(q=q, k=k, v=v, mask=mask, qf=qf, kf=kf, g=g, n=n, heads=h,
                scale=scale, kv_one=kv_one)
