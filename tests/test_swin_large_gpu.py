"""GPU: Swin-L on the engine.  The micro architecture of tests/test_swin_large.py (768 -> 3072-channel merge LayerNorm -> 1536) against
OracleSwin on every residual-stream tap and on the logits, its uint8 / sliced forwards and its model diff; the real Swin-L widths
(192 ... 1536 channels, 6 ... 48 heads, merge LayerNorms of 768 / 1536 / 3072 channels) at 96^2; and single launches of the GEMM and
window-attention shapes that only Swin-L has, against the oracle.  Every comparison is bit equality except the fp32 DDV stages, which
are not looked at here."""
import functools

import numpy as np
import pytest
import torch

from _arena import twice
from conftest import gpu_ok
from test_kernel_edges_gpu import Layer, _check, _gen, _randint, dva  # noqa: F401  (dva: fixture)
from test_swin_large import large_micro

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


# ------------------------------------------------------------------------------------------------
# 1. the micro architecture: 768 -> merge LayerNorm over 3072 channels -> 1536
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _micro_oracle(bits):
    import swin_oracle as SO
    m, x = large_micro()
    taps = {}
    with torch.no_grad():
        ref = SO.OracleSwin(m.arch, {k: v.cpu() for k, v in m.state_dict().items()}).quant_forward(x, m.export_calib(), bits, taps)
    return ref, taps


@pytest.mark.parametrize('bits', [8, 4])
def test_large_micro_engine_vs_oracle(dva, bits):
    """the frozen plan (whose construction needs p2v_ln_prefold at C = 3072) == OracleSwin on every residual-stream tap and all logits"""
    m, x = large_micro()
    ref, taps_o = _micro_oracle(bits)
    m.cuda()
    try:
        with torch.no_grad():
            out = m(x.cuda(), bits=bits)
            taps_g = {}
            m._plan.forward(x.cuda(), taps=taps_g)
            torch.cuda.synchronize()
    finally:
        m.cpu()
    # (the 3072-wide LayerNorm's codes feed the reduction whose requantized output is the tap layers.0.downsample.qact2)
    assert 'layers.0.downsample.qact2' in taps_g and len(taps_g) >= 10
    assert taps_g['layers.0.downsample.qact2'].numel() == 4 * 16 * 1536
    for name, t in taps_g.items():
        want = taps_o[name].reshape(t.shape)
        assert torch.equal(t.cpu().int(), want.int()), (name, int((t.cpu().int() != want.int()).sum()), t.numel())
    assert torch.equal(out.cpu(), ref), float((out.cpu() - ref).abs().max())
    assert float((ref[0] - ref[1]).abs().max()) > 0


def test_large_micro_uint8_and_slices(dva):
    """forward_uint8 == forward on the normalised images; an explicitly sliced forward == one stream"""
    from diff_vit_amd import data as D
    m, _ = large_micro()
    mean, std = D.MODEL_STATS['swin'][:2]
    u8 = dva.synth.images_uint8(7, 3, 32)
    x = dva.synth.images(12, 7, 32).cuda()
    m.cuda()
    try:
        with torch.no_grad():
            want = m(D.normalize_uint8(u8, mean, std, 'NHWC').cuda(), 8).cpu()
            got = m.forward_uint8(u8.cuda(), 8, mean, std, 'NHWC').cpu()
            m(x[:1])
            single = m._plan.forward(x, n_streams=1).cpu()
            sliced = m._plan.forward(x, n_streams=2, slices=[3, 2, 2]).cpu()
    finally:
        m.cpu()
    assert torch.equal(got, want)
    assert single.shape == (7, 10) and torch.equal(sliced, single)
    assert float((single[0] - single[1]).abs().max()) > 0


def test_large_micro_model_diff(dva):
    """forward_ddv: logits byte-equal to forward, the sums of the 3072-wide stage layers.0.downsample.qact1 equal pair_cosine_cpu on the
    oracle's codes bit for bit (an int8 stage with one scale: exact integer sums, the bound tests/test_swin_modeldiff_gpu.py uses for
    such stages); forward_linear_taps returns layers.0.downsample.reduction (K = 3072) == the oracle's qgemm"""
    import p2vit_oracle as O
    m, x = large_micro()
    ref, taps_o = _micro_oracle(8)
    n = 2
    m.cuda()
    try:
        with torch.no_grad():
            fwd = m(x.cuda(), bits=8).cpu()
            plan = m._plan
            logits, names, sums = plan.forward_ddv(x.cuda(), True)
            lin_logits, lin = plan.forward_linear_taps(x.cuda())
            torch.cuda.synchronize()
            lin_names = plan.linear_tap_names()
    finally:
        m.cpu()
    assert names == dva.ddv.swin_stage_names(m.arch['depths'], True)
    assert torch.equal(logits.cpu(), fwd) and torch.equal(fwd, ref) and torch.equal(lin_logits.cpu(), fwd)
    sums = sums.cpu()
    assert bool(torch.isfinite(sums).all())
    v = taps_o['layers.0.downsample.qact1'].reshape(2 * n, -1)
    assert v.shape[1] == 16 * 3072
    want = dva.ddv.pair_cosine_cpu([v[:n].to(torch.int32)], [v[n:].to(torch.int32)])[0]
    assert torch.equal(sums[names.index('layers.0.downsample.qact1')], want)
    assert float(want[:, 1].min()) > 0
    # the reduction's fp32 output, K = 3072
    c, W = m.export_calib(), {k: v_.detach().float().cpu() for k, v_ in m.state_dict().items()}
    nm = 'layers.0.downsample.reduction'
    s_w = c[nm]['int8'].reshape(-1)
    y = O.qgemm(v.reshape(-1, 3072).float(), c['layers.0.downsample.qact1'].reshape(()), O.weight_codes(W[nm + '.weight'], None, s_w, 8), s_w, None)
    got = lin[lin_names.index(nm)].cpu()
    assert tuple(got.shape) == (2 * n, 16, 1536)
    assert torch.equal(got.reshape(-1, 1536), y)


# ------------------------------------------------------------------------------------------------
# 2. the real Swin-L widths at 96^2
# ------------------------------------------------------------------------------------------------
def test_swin_large_widths_engine_vs_oracle(dva):
    """swin_large_patch4_window12_384(depths=(1, 1, 1, 1), img_size=96): maps of 24 / 12 / 6 / 3 tokens, 192 ... 1536 channels, 6 ... 48
    heads, merge LayerNorms of 768 / 1536 / 3072 channels; two images, all logits == OracleSwin"""
    import swin_oracle as SO
    m = dva.swin.swin_large_patch4_window12_384(depths=(1, 1, 1, 1), img_size=96, num_classes=10, cfg=dva.Config(True, True, 'minmax')).eval()
    assert m.arch['embed_dim'] == 192 and m.arch['num_heads'] == (6, 12, 24, 48) and m.layers[2].downsample.norm.weight.shape == (3072,)
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    x = dva.synth.images(5, 2, 96)
    m.cuda()
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:1].cuda()); m.model_close_calibrate()
        m.model_quant()
        out = m(x.cuda()).cpu()
        torch.cuda.synchronize()
        ref = SO.OracleSwin(m.arch, {k: v.cpu() for k, v in m.state_dict().items()}).quant_forward(x, m.export_calib(), 8)
    assert torch.equal(out, ref), int((out != ref).sum())
    assert float((ref[0] - ref[1]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------
# 3. single launches at the widths only Swin-L has
# ------------------------------------------------------------------------------------------------
M_ROWS = 70
# kind, K, N, log2 of s_x * s_w: uniform codes give |acc| ~ 74^2 sqrt(K) (2.1e5 at K = 1536, 4.3e5 at K = 6144), y = acc * 2^e ~ 1.6
GEMMS = [('gelu_tab', 1536, 6144, -17), ('resid_pre', 6144, 1536, -18), ('requant', 1536, 4608, -17), ('requant', 3072, 1536, -18)]


@functools.lru_cache(maxsize=None)
def _uniform_operands(K, N):
    gen = _gen(7000 + K + N)
    return _randint(gen, -128, 127, (M_ROWS, K)), _randint(gen, -128, 127, (N, K)), gen


@pytest.mark.parametrize('kind,K,N,e', GEMMS)
def test_gemm_at_swin_large_widths(dva, oracle, kind, K, N, e):
    """fc1 (GELU), fc2 (RESID with its pre-folded table) and qkv (REQUANT) of the 1536-channel stage, and the bias-less reduction
    3072 -> 1536; codes drawn uniformly so that the oracle's 24-bit bound on the accumulator holds at K = 6144 (asserted by qgemm)"""
    E = dva.engine
    x, w, gen = _uniform_operands(K, N)
    acc_max = float((x.double() @ w.double().t()).abs().max())
    assert acc_max < 2.0 ** 22, acc_max                                # far inside qgemm's 2^24
    ptf = lambda base: base * 2.0 ** torch.randint(0, 4, (N,), generator=_gen(K + N + int(base * 1e4))).float()
    p = dict(e_req=3, e_gelu=5, s_mid=ptf(0.0131), s_res=ptf(0.0173), s_next=ptf(0.0209),
             res=torch.clamp(torch.round(torch.randn(M_ROWS, N, generator=_gen(K + N)) * 50.0), -128, 127))
    bias = torch.zeros(N) if K == 3072 else torch.randn(N, generator=_gen(K * 3 + N)) * 0.4
    lay = Layer(E, oracle, x, w, 2.0 ** -6, torch.full((N,), 2.0 ** (e + 6)), bias, False, p)
    ref = lay.reference(oracle, kind, M_ROWS)
    share = float((ref['out'].abs() >= 127).float().mean())
    assert float(ref['out'].float().std()) > 4.0 and share < 0.6, (share, 'the codes use their range')
    got = twice(lambda s: lay.run(kind, M_ROWS, K, N, s))
    _check(got, ref, (kind, K, N))


@pytest.mark.parametrize('heads,Hf,ws,shift,B', [(48, 3, 3, 0, 2), (6, 24, 12, 6, 1)])
def test_window_attention_at_swin_large_head_counts(dva, heads, Hf, ws, shift, B):
    """the last stage (48 heads, a 3 x 3 map as one window) and the first (6 heads on 24 x 24 in shifted 12 x 12 windows) of Swin-L at 96^2"""
    from test_swin_window12_gpu import SCALES, case_inputs, run_kernel
    qkv, tab, ref = case_inputs(heads, Hf, ws, shift, B)
    assert float((ref['want'] != 0).float().mean()) >= 0.5 and bool((ref['k'] < 16).any())
    out, pk = run_kernel(dva.engine, qkv, tab, ref, heads, ws, SCALES, tap=True)
    assert torch.equal(pk, ref['k']), int((pk != ref['k']).sum())
    assert torch.equal(out, ref['want']), int((out != ref['want']).sum())
