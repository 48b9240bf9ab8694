"""CPU: the DDV stages inside attention (compute_ddv(..., attention=True)) - the stage lists and counts, the module-graph path on float and
quant-state micro models against a direct torch computation and against the oracle's taps (tests/_ddv_attention_ref.py), attention=False
as the unchanged default, and the argument refusals of the new entry points (made before the first HIP call).

Bounds (those of test_ddv.py / test_ddv_gpu.py): a DDV entry from hooked fp32 values against the same values summed in another fp64 order,
or against the exact integer sums of the oracle's codes, 1e-9."""
import ctypes

import numpy as np
import pytest
import torch

from _ddv_attention_ref import ddv_of, expected, swin_attention_stages, vit_attention_stages
from _ddv_full_ref import load_reference_calibration
from conftest import golden_calib, golden_weights, load_golden
from test_ddv import micro_model


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def _pair_ddv(a, b):
    """reference formula on two [n, ...] float tensors (fp64)"""
    n = a.shape[0]
    a, b = a.reshape(n, -1).double().numpy(), b.reshape(n, -1).double().numpy()
    return ddv_of(np.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], 1))


def test_stage_lists_and_counts(dva):
    D = dva.ddv
    for depth in (1, 2, 12):
        for lin in (False, True):
            for full in (False, True):
                base, att = D.stage_names(depth, lin, full), D.stage_names(depth, lin, full, attention=True)
                assert D.stage_names(depth, lin, full, False) == base                       # the default list is today's
                assert len(att) == len(base) + 2 * depth and len(set(att)) == len(att)
                assert [n for n in att if n in set(base)] == base
                for i in range(depth):
                    p = 'blocks.%d.attn.' % i
                    k = att.index(p + 'qact1')
                    assert att[k:k + 4] == [p + 'qact1', p + 'qact_attn1', p + 'log_int_softmax', p + 'qact2']
    assert (len(D.stage_names(12, False)), len(D.stage_names(12, True))) == (63, 112)
    for depths in ((2, 2), (2, 2, 6, 2), (1, 1)):
        blocks = sum(depths)
        for lin in (False, True):
            base, att = D.swin_stage_names(depths, lin), D.swin_stage_names(depths, lin, attention=True)
            assert D.swin_stage_names(depths, lin, False) == base
            assert len(att) == len(base) + 3 * blocks and [n for n in att if n in set(base)] == base
            p = 'layers.0.blocks.0.attn.'
            k = att.index(p + 'qact1')
            assert att[k:k + 5] == [p + 'qact1', p + 'qact_attn1', p + 'qact2', p + 'log_int_softmax', p + 'qact3']
            assert not any('qact_table' in n for n in att)
    m = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10)
    mods = dict(m.named_modules())
    assert all(n in mods for n in D.swin_stage_names(m.arch['depths'], True, True))
    v = micro_model(dva, dva.synth, load_golden('micro_vit'))
    assert all(n in dict(v.named_modules()) for n in D.stage_names(2, True, True, True))


def test_vit_float_module_graph_against_direct_torch(dva, synth):
    """float micro-ViT: qact_attn1 is the identity on (q @ k^T) * scale of the kept qkv output and log_int_softmax a plain softmax of it"""
    k = load_golden('ddv_micro')
    m = micro_model(dva, synth, load_golden('micro_vit'))
    x, xa = torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])
    d = dva.compute_ddv(m, x, xa, attention=True)
    assert list(d) == dva.ddv.stage_names(2, True, False, True)
    d0 = dva.compute_ddv(m, x, xa)
    assert list(d0) == dva.ddv.stage_names(2, True) and all(torch.equal(v, d[nm]) for nm, v in d0.items())     # attention=False: today's dict

    def direct(inp):
        with torch.no_grad():
            m(inp)
        out = []
        for blk in m.blocks:
            y = blk.attn.qkv_output
            B, N, _ = y.shape
            H = blk.attn.num_heads
            qkv = y.reshape(B, N, 3, H, -1).permute(2, 0, 3, 1, 4)
            s = (qkv[0] @ qkv[1].transpose(-2, -1)) * blk.attn.scale
            out.append((s, s.softmax(dim=-1)))
        return out
    a, b = direct(x), direct(xa)
    for i in range(2):
        for j, nm in enumerate(('qact_attn1', 'log_int_softmax')):
            err = float(np.abs(d['blocks.%d.attn.%s' % (i, nm)].numpy() - _pair_ddv(a[i][j], b[i][j])).max())
            print('float', i, nm, err)
            assert err <= 1e-9, (i, nm, err)


@pytest.mark.parametrize('tag', ['q8', 'q4'])
def test_vit_quant_state_module_graph_against_oracle_taps(dva, oracle, synth, tag):
    """quant-state micro-ViT on the CPU (no engine: hooks on the module graph): the hooked fp32 values code * scale and 2^-k give the DDVs
    of the oracle's integer codes and exponents; with stages='full' the same entries"""
    k, g = load_golden('ddv_micro'), load_golden('micro_vit')
    m = micro_model(dva, synth, g)
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']))
    load_reference_calibration(m, golden_calib(g, oracle))
    bits = [8] * 10 if tag == 'q8' else [4] * 10
    x, xa = torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])
    d = dva.compute_ddv(m, x, xa, bits, attention=True)
    assert list(d) == dva.ddv.stage_names(2, True, False, True)
    st, _, _ = vit_attention_stages(oracle, synth.ARCHS['micro'], golden_weights(g), golden_calib(g, oracle), torch.cat((x, xa), 0), bits)
    assert len(st) == 4
    for nm, (v, kind) in st.items():
        err = float(np.abs(d[nm].numpy() - ddv_of(expected(v, kind))).max())
        print(tag, nm, err)
        assert err <= 1e-9, (tag, nm, err)
    assert all(len(torch.unique(v)) >= 4 for v, kind in st.values())                  # (liveness: no constant stage)
    df = dva.compute_ddv(m, x, xa, bits, stages='full', attention=True)
    assert list(df) == dva.ddv._with_qact_pos(dva.ddv.stage_names(2, True, True, True))
    assert all(torch.equal(df[nm], d[nm]) for nm in st)
    # a -1 entry (mixed float / quantized layers) keeps to the hooks and the same key list
    dm = dva.compute_ddv(m, x, xa, [8] * 9 + [-1], attention=True)
    assert list(dm) == list(d)


def test_swin_module_graph_float_and_quant(dva):
    """micro Swin (window 7, 56 x 56: shifted and unshifted blocks, one merge) on the CPU.  float: qact_attn1 = (q * scale) @ k^T of the hooked
    attn.qact1 output, qact2 = that plus the bias table, log_int_softmax = softmax (plus the block's mask), window outputs regrouped per
    image.  quant state: the DDVs of the oracle's window taps."""
    S = dva.synth
    m = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    m.load_state_dict(S.swin_state_dict(m.state_dict(), 5))
    x = S.images(11, 3, 56)
    xa = x + 0.25 * S.images(12, 3, 56)
    names = dva.ddv.swin_stage_names(m.arch['depths'], True, attention=True)
    with pytest.raises(NotImplementedError):
        dva.compute_ddv(m, x, xa, [8] * 10, attention=True)
    d = dva.compute_ddv(m, x, xa, None, attention=True)
    assert list(d) == names and all(v.dtype == torch.float64 and v.shape == (3,) and bool(torch.isfinite(v).all()) for v in d.values())
    d0 = dva.compute_ddv(m, x, xa, None)
    assert list(d0) == dva.ddv.swin_stage_names(m.arch['depths'], True) and all(torch.equal(v, d[nm]) for nm, v in d0.items())
    blocks = [(('layers.%d.blocks.%d.' % (li, bi)), blk) for li, lay in enumerate(m.layers) for bi, blk in enumerate(lay.blocks)]

    def direct(inp):
        q1 = dva.ddv._swin_hooked_outputs(m, inp, [p + 'attn.qact1' for p, _ in blocks])
        out = {}
        for (p, blk), y in zip(blocks, q1):
            at = blk.attn
            N = blk.window_size ** 2
            H = at.num_heads
            qkv = y.reshape(-1, N, 3, H, 32).permute(2, 0, 3, 1, 4)
            a1 = (qkv[0] * at.scale) @ qkv[1].transpose(-2, -1)
            bias = at.relative_position_bias_table[at.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()
            a2 = a1 + bias.unsqueeze(0)
            xi = a2
            if blk.attn_mask is not None:
                nW = blk.attn_mask.shape[0]
                xi = (a2.view(-1, nW, H, N, N) + blk.attn_mask.unsqueeze(1).unsqueeze(0)).view(-1, H, N, N)
            B = inp.shape[0]
            out[p + 'attn.qact_attn1'], out[p + 'attn.qact2'] = a1.detach().reshape(B, -1), a2.detach().reshape(B, -1)
            out[p + 'attn.log_int_softmax'] = xi.softmax(dim=-1).detach().reshape(B, -1)
        return out
    with torch.no_grad():
        a, b = direct(x), direct(xa)
    assert len(a) == 3 * len(blocks) == 12
    for nm in a:
        err = float(np.abs(d[nm].numpy() - _pair_ddv(a[nm], b[nm])).max())
        assert err <= 1e-9, ('float', nm, err)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:2]); m.model_close_calibrate()
        m.model_quant()
    dq = dva.compute_ddv(m, x, xa, 8, attention=True)
    assert list(dq) == names
    with torch.no_grad():
        st, _ = swin_attention_stages(m, torch.cat((x, xa), 0), 8)
    assert set(st) == set(a)
    for nm, (v, kind) in st.items():
        err = float(np.abs(dq[nm].numpy() - ddv_of(expected(v, kind))).max())
        print('quant', nm, err)
        assert err <= 1e-9, ('quant', nm, err)


def test_refusals_without_gpu(dva):
    """stage counts and scratch size of the flagged stage sets; every refusal of the new entry points comes before a HIP call"""
    E = dva.engine
    L = E.lib()
    h = ctypes.c_void_p()
    desc = E.ModelDesc(E.P2V_ABI_VERSION, 224, 16, 3, 384, 12, 6, 1536, 1000)
    E.check(L.p2v_plan_create(ctypes.byref(desc), ctypes.byref(h)))
    A = E.DDV_STAGES_ATTN
    assert A == 2 and E.COS_LOG2K == 3
    for lin in (0, 1):
        for base in (E.DDV_STAGES_ENGINE, E.DDV_STAGES_FULL):
            assert L.p2v_ddv_stage_count_ex2(h, lin, base) == L.p2v_ddv_stage_count_ex(h, lin, base)
            assert L.p2v_ddv_stage_count_ex2(h, lin, base | A) == L.p2v_ddv_stage_count_ex(h, lin, base) + 24
    assert L.p2v_ddv_stage_count_ex2(h, 1, 4) == E.E_ARG and b'stage_set' in L.p2v_last_error()
    assert L.p2v_ddv_stage_count_ex2(h, 1, -1) == E.E_ARG
    assert L.p2v_ddv_stage_count_ex(h, 1, 2) == E.E_ARG                        # the earlier entry keeps refusing the flag
    n = 4
    assert L.p2v_ddv_attn_scratch_bytes(h, n) == 2 * 2 * n * 6 * 197 * 208
    assert L.p2v_ddv_attn_scratch_bytes(h, 0) == 0 and L.p2v_ddv_attn_scratch_bytes(None, 4) == 0
    cfg = (ctypes.c_int8 * 50)(*([8] * 50))
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(264)
    big = 1 << 40

    def call(stage_set, att, att_bytes):
        return L.p2v_forward_ddv_ex2(h, one, n, cfg, 50, one, one, big, 0, stage_set, one, big, att, att_bytes, one, None)
    assert call(A, None, big) == E.E_ARG and b'attn_scratch' in L.p2v_last_error()
    assert call(A | 1, None, 0) == E.E_ARG
    assert call(A, odd, big) == E.E_ARG and b'aligned' in L.p2v_last_error()
    assert call(A, one, L.p2v_ddv_attn_scratch_bytes(h, n) - 1) == E.E_WORKSPACE and b'attn_scratch' in L.p2v_last_error()
    assert call(4, one, big) == E.E_ARG and b'unknown stage_set 4' in L.p2v_last_error()
    assert call(-1, one, big) == E.E_ARG
    # the reduction: the exponent form takes no scales, and only the three element types exist
    lay = (E.CosLayer * 1)(E.CosLayer(one, one, one, 64, 16, 4, 5, E.COS_LOG2K))
    assert L.p2v_pair_cosine_workspace_bytes(lay, 1, 1) == 0
    assert L.p2v_pair_cosine(lay, 1, 1, one, one, big, None) == E.E_ARG and b'no scales' in L.p2v_last_error()
    lay[0].scale = None
    assert L.p2v_pair_cosine_workspace_bytes(lay, 1, 1) > 0
    for unknown in (2, 4, -1):
        lay[0].dtype = unknown
        assert L.p2v_pair_cosine(lay, 1, 1, one, one, big, None) == E.E_ARG and b'dtype' in L.p2v_last_error()
    # the operator taps: pitch and alignment
    at = E.Attn(2.0 ** -8, 0.125, 16.0, 0.5, -12, 43, 714)
    assert L.p2v_lis_attention_taps(one, 1, 17, 1, 64, ctypes.byref(at), one, one, one, 17, None) == E.E_ARG and b'pitch' in L.p2v_last_error()
    assert L.p2v_lis_attention_taps(one, 1, 17, 1, 64, ctypes.byref(at), one, one, one, 16, None) == E.E_ARG
    assert L.p2v_lis_attention_taps(one, 1, 17, 1, 64, ctypes.byref(at), one, odd, None, 32, None) == E.E_ARG and b'aligned' in L.p2v_last_error()
    wa = E.WinAttn(2.0 ** -4, float(np.float32(32 ** -0.5)), 2.0 ** -3, 2.0 ** -5, 2.0 ** -4, 2.0 ** -3, -12, 43, 714, one, one, None, 7, 4)
    assert L.p2v_window_attention_taps(one, 1, 196, 3, 32, ctypes.byref(wa), one, one, None, None, 48, None) == E.E_ARG and b'pitch' in L.p2v_last_error()
    assert L.p2v_window_attention_taps(one, 1, 196, 3, 32, ctypes.byref(wa), one, None, odd, None, 64, None) == E.E_ARG
    L.p2v_plan_destroy(h)
