"""Canonical semantics of a Swin model under Config(ptf=False) - every QAct layer-wise, every LayerNorm ``F.layer_norm`` followed by the next
QAct - for the tests: ``OracleSwin.quant_forward`` with ``p2vit_oracle.int_layernorm`` replaced, for the duration of the call, by a wrapper
around ``_float_ops_ref.float_layernorm`` (S1 / S2 exact integers, then the fp64 chain, every operation rounded on its own).  Under
lis=False it composes with ``_swin_float_ops_ref.window_softmax_attention``, put in place the way that file does.  The oracle files are not
edited.

``export_calib()`` gives ONE scale per QAct under ptf=False, and ``OracleSwin`` indexes ``qact2`` / ``qact4`` / ``downsample.qact2`` per
channel (they are PTF vectors under ptf=True): ``expand_calib`` repeats those scalars over the channels first.
"""
import re
import types

import pytest
import torch

import p2vit_oracle as O
import swin_oracle as SO
import _swin_float_ops_ref as RS
from _float_ops_ref import float_layernorm

SWIN_EPS = 1e-5            # nn.LayerNorm's default: what swin.py's QIntLayerNorm modules carry
CONFIGS = {'ft': (False, True), 'ff': (False, False)}


def float_ln_wrapper(eps):
    """a stand-in with ``p2vit_oracle.int_layernorm``'s signature (dequantised input, per-channel input scales, gamma, beta, per-channel
    output scales) -> the codes of the float LayerNorm and the QAct behind it, as floats"""
    def fln(x, s_in_vec, gamma, beta, s_out_vec, *a, **k):
        assert not a and not k, (a, k)
        s_in, s_out = float(s_in_vec.reshape(-1)[0]), float(s_out_vec.reshape(-1)[0])
        assert bool((s_in_vec == s_in).all()) and bool((s_out_vec == s_out).all()), 'ptf=False: one scale per QAct'
        q = torch.round(x / s_in)
        assert torch.equal(q * s_in, x)                    # the input is codes on a power-of-two grid
        codes, _ = float_layernorm(q, s_in, gamma, beta, eps, torch.full((q.shape[-1],), 1.0 / s_out))
        return codes.float()
    return fln


def expand_calib(calib, state_dict):
    """the calibration dict with the scalar scales of qact2 / qact4 / downsample.qact2 repeated over the channels"""
    out = {k: (dict(v) if isinstance(v, dict) else v) for k, v in calib.items()}
    for k in list(out):
        mt = re.match(r'(layers\.\d+\.blocks\.\d+)\.(qact2|qact4)$', k)
        if mt:
            assert out[k].numel() == 1, k
            out[k] = out[k].reshape(-1).expand(state_dict[mt.group(1) + '.norm1.weight'].numel()).clone()
        mt = re.match(r'(layers\.\d+\.downsample)\.qact2$', k)
        if mt:
            assert out[k].numel() == 1, k
            out[k] = out[k].reshape(-1).expand(state_dict[mt.group(1) + '.reduction.weight'].shape[0]).clone()
    return out


def patched(lis, eps=SWIN_EPS):
    """context: the oracle's LayerNorm (and, under lis=False, its window attention) replaced by the float operators' helpers"""
    mp = pytest.MonkeyPatch()
    mp.setattr(O, 'int_layernorm', float_ln_wrapper(eps))
    if not lis:
        mp.setattr(SO, 'window_attention_quant', RS.window_softmax_attention)
    return mp


def quant_forward(arch, state_dict, calib, x, bits=8, taps=None, lis=True, eps=SWIN_EPS):
    """logits of the whole model under Config(False, lis); ``calib`` as ``export_calib()`` gives it (expanded here)"""
    sd = {k: v.detach().cpu() for k, v in state_dict.items()}
    mp = patched(lis, eps)
    try:
        with torch.no_grad():
            return SO.OracleSwin(arch, sd).quant_forward(x, expand_calib(calib, sd), bits, taps)
    finally:
        mp.undo()


def mixed_forward(m, x, bit_list, taps=None, lis=True):
    """per-layer widths: composed with ``_swin_bits_ref.substituted``"""
    from _swin_bits_ref import substituted
    sd, calib = substituted(m, bit_list)
    return quant_forward(m.arch, sd, calib, x, 8, taps, lis)


def model_view(m):
    """what ``test_swin_modeldiff_gpu.oracle_stages`` reads of a model (arch, state_dict(), export_calib()), with the calibration expanded"""
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    calib = expand_calib(m.export_calib(), sd)
    return types.SimpleNamespace(arch=m.arch, state_dict=lambda: sd, export_calib=lambda: calib)


def micro_swin(dva, cfg, factory='swin_micro_patch4_window7_56', img=56, n_images=3, **kw):
    return RS.micro_swin(dva, factory, img, n_images, cfg=cfg, **kw)
