"""Canonical semantics of the log-int-softmax at the width of its module's bit type (QIntSoftmax.forward, models/ptq/layers.py:372-375:
``mask = rounds >= 2**bits``, clamp to ``2**bits - 1``, masked entries 0), for the tests: a restatement on ``p2vit_oracle``'s pieces;
the oracle itself is not touched.

    p = 2^-k for k < 2^bits, else 0,      bits 3 or 4

``lis_int_bits`` is ``O.lis_int`` with every k >= 2^bits mapped to 16 (the oracle's and the engine's "zero" exponent), ``lis_float_bits`` the
matching calibration-pass function.  Whole-model forwards of ``OracleViT`` / ``OracleSwin`` and the restatements built on ``O.lis_int`` run
with the two put in place for the duration of the call by the context manager ``patched`` (the pattern of ``_swin_float_ops_ref``, without
pytest); per-block widths are served by a sequence that hands one width to every call of ``O.lis_int``, in module order.
"""
import os

import numpy as np
import torch

import p2vit_oracle as O
import swin_oracle as SO

_LIS_INT, _LIS_FLOAT = O.lis_int, O.lis_float          # the oracle's own functions, whatever a test puts in their place later
_FIXTURE = []


def fixture():
    """tests/golden/softmax_bits.npz (tools/gen_golden_softmax_bits.py: the REAL reference under BIT_TYPE_S = uint3), loaded once"""
    if not _FIXTURE:
        _FIXTURE.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'softmax_bits.npz')))
    return _FIXTURE[0]


def lis_int_bits(codes, sf, bits):
    """integer score codes -> exponents k, 16 = zero: every k >= 2^bits is zero"""
    assert bits in (3, 4)
    k = _LIS_INT(codes, sf)
    return torch.where(k >= 2 ** bits, torch.full_like(k, 16), k)


def lis_float_bits(x, sf, bits):
    """QIntSoftmax.forward on un-quantized scores (the calibration pass) at ``bits``: the oracle's 4-bit result holds the exact 2^-k for
    k <= 15, so the narrower clamp is a threshold on it"""
    assert bits in (3, 4)
    p = _LIS_FLOAT(x, sf)
    return torch.where(p < 2.0 ** -(2 ** bits - 1), torch.zeros_like(p), p)


def probs(k):
    return O.lis_probs(k)


class _Widths:
    """one width per call, cycling through ``widths`` (a forward calls the softmax once per attention module, in module order)"""

    def __init__(self, widths):
        self.widths, self.calls = [int(b) for b in widths], 0

    def next(self):
        b = self.widths[self.calls % len(self.widths)]
        self.calls += 1
        return b


def widths_of(bits, n):
    return [int(bits)] * n if isinstance(bits, (int, np.integer)) else [int(b) for b in bits]


class patched:
    """``with patched(widths): ...``: ``O.lis_int`` / ``O.lis_float`` run at the widths, one per call in turn; the oracle's own functions
    are back in place afterwards, whatever happens inside"""

    def __init__(self, widths):
        self.w = _Widths(widths)

    def __enter__(self):
        self.saved = (O.lis_int, O.lis_float)
        O.lis_int = lambda codes, sf: lis_int_bits(codes, sf, self.w.next())
        O.lis_float = lambda x, sf: lis_float_bits(x, sf, self.w.next())
        return self.w

    def __exit__(self, *exc):
        O.lis_int, O.lis_float = self.saved
        return False


def vit_calibrate(arch, state_dict, x, bits):
    """``OracleViT.calibrate`` at the widths -> (oracle with its calibration state, logits of the pass)"""
    orc = O.OracleViT(arch, state_dict)
    with patched(widths_of(bits, arch['depth'])), torch.no_grad():
        y = orc.calibrate(x)
    return orc, y


def vit_forward(arch, state_dict, calib, x, bit_config, bits, taps=None):
    """``OracleViT.quant_forward`` at the widths (an int or one per block)"""
    orc = O.OracleViT(arch, {k: v.detach().cpu() for k, v in state_dict.items()})
    orc.calib = calib
    with patched(widths_of(bits, arch['depth'])) as w, torch.no_grad():
        y = orc.quant_forward(x, list(bit_config), taps)
    assert w.calls == arch['depth']
    return y


def swin_forward(arch, state_dict, calib, x, wbits, bits, taps=None):
    """``OracleSwin.quant_forward`` (weight width ``wbits``) at the softmax widths ``bits`` (an int or one per attention module)"""
    n = sum(arch['depths'])
    calib = {k: v for k, v in calib.items() if not k.endswith('.bits')}
    with patched(widths_of(bits, n)) as w, torch.no_grad():
        y = SO.OracleSwin(arch, {k: v.detach().cpu() for k, v in state_dict.items()}).quant_forward(x, calib, wbits, taps)
    assert w.calls == n
    return y


def window_attention(x_codes, s_in, W, c, heads, ws, bits, mask=None, taps=None, wbits=8):
    """``swin_oracle.window_attention_quant`` at ``bits``"""
    with patched([bits]), torch.no_grad():
        return SO.window_attention_quant(x_codes, s_in, W, c, heads, ws, mask=mask, taps=taps, bits=wbits)


def attention(qkv, heads, at, bits):
    """the ViT attention core on int8 qkv codes [B, N, 3 D] -> (qact2 codes [B, N, D], score codes [B, H, N, N], exponents [B, H, N, N]):
    the lines of ``OracleViT.quant_forward`` between qact1 and qact2 (vit_fquant.py:309-326).  ``at``: dict with s_q1, s_attn, s_q2 (PoT)"""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // heads
    s_q1, s_at, s_a2 = (torch.tensor(float(at[k])) for k in ('s_q1', 's_attn', 's_q2'))
    q = qkv.float().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    acc = q[0] @ q[1].transpose(-2, -1)
    attn = (acc * (s_q1 * s_q1)) * (hd ** -0.5)
    sc = torch.clamp(torch.round(attn / s_at), -128, 127)
    k = lis_int_bits(sc, s_at, bits)
    o = (O.lis_probs(k) @ (q[2] * s_q1)).transpose(1, 2).reshape(B, N, D)
    return torch.clamp(torch.round(o / s_a2), -128, 127).to(torch.int8), sc.to(torch.int8), k.to(torch.int8)


def linear_outputs(arch, W, c, taps, bits):
    """the fp32 output of every QConv2d / QLinear in bit_config order, rebuilt with ``O.qgemm`` from the integer codes ``taps`` of the
    QActs in front of them (the oracle's tap names: a forward's own taps, or the reference's stored ones)"""
    import torch.nn.functional as F
    P = arch['patch_size']
    t = {k: torch.as_tensor(np.asarray(v)).float() for k, v in taps.items()}
    cols = F.unfold(t['qact_input'], kernel_size=P, stride=P).transpose(1, 2)
    s_w = c['patch_embed.proj']['int%d' % bits[0]]
    wq = O.weight_codes(W['patch_embed.proj.weight'], None, s_w, bits[0])
    out = [O.qgemm(cols.reshape(-1, cols.shape[-1]), c['qact_input'], wq, s_w.reshape(-1), W['patch_embed.proj.bias'])]
    for i in range(arch['depth']):
        p = 'blocks.%d.' % i
        b = bits[1 + 4 * i: 5 + 4 * i]
        for nm, tin, kind, bit in (('attn.qkv', 'attn.qact0', 'attn', b[0]), ('attn.proj', 'attn.qact2', 'attn.proj', b[1]),
                                   ('mlp.fc1', 'mlp.qact0', 'mlp', b[2]), ('mlp.fc2', 'mlp.qact1', 'mlp.fc2', b[3])):
            if kind in ('attn', 'mlp'):
                bi = O.BIT_POOL.index(bit)
                s_x, cs = c[p + kind + '.best_act_scale'][bi], c[p + kind + '.best_scale'][bi]
                s_w = c[p + kind + '.best_weight_scale'][bi]['int%d' % bit]
            else:
                s_x, cs = c[p + tin], None
                s_w = c[p + kind]['int%d' % bit]
            wq = O.weight_codes(W[p + nm + '.weight'], cs, s_w, bit)
            xin = t[p + tin]
            out.append(O.qgemm(xin.reshape(-1, xin.shape[-1]), s_x, wq, s_w.reshape(-1), W[p + nm + '.bias']))
    s_w = c['head']['int%d' % bits[-1]]
    wq = O.weight_codes(W['head.weight'], None, s_w, bits[-1])
    out.append(O.qgemm(t['qact2'], c['qact2'], wq, s_w.reshape(-1), W['head.bias']))
    return out


def exponent_classes(k):
    """the set of exponents present in ``k`` (0 .. 15 and the zero class 16)"""
    return set(int(v) for v in torch.unique(torch.as_tensor(k)))


MICRO_SEED, QKV_GAIN = 1, 4.0


def micro_weights(synth, arch, seed=MICRO_SEED, gain=QKV_GAIN):
    """the weight recipe of the fixture: synthetic weights of ``seed`` with every attn.qkv.weight times ``gain`` - scores wide enough for
    the exponents 8 ... 15 that tell a 3-bit softmax from a 4-bit one (at gain 1 no exponent reaches 8)"""
    sd = synth.vit_state_dict(arch, seed)
    return {k: (v * gain if k.endswith('attn.qkv.weight') else v) for k, v in sd.items()}


def micro_bit_lists(L):
    mixed = [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)]
    return {'q8': [8] * L, 'q4': [4] * L, 'qmix': mixed}
