"""CPU: Config(ptf=True, lis=False) of a Swin model - the canonical table softmax of tests/_swin_float_ops_ref.py against the REAL reference's
WindowAttention (tests/golden/swin_winattn_softmax.npz), the module graph of swin.py against the helper's whole-model forward, and what
``SwinTransformer.freeze`` refuses."""
import numpy as np
import pytest
import torch

import _swin_float_ops_ref as R


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def test_helper_against_the_reference_fixture():
    """the canonical operator, fed the reference's own qact2 and qact1 codes, gives the reference's qact3 codes up to the link rule of the
    float operators: at most +-1 anywhere, at most 1 code per 1 000 per stage; every qact2 scale is at most 2^-2"""
    g = R.fixture()
    cap = int(g['cap_per_1000'])
    heads, dim = int(g['heads']), int(g['dim'])
    for ws, seed in g['cases']:
        pre = 'ws%d/' % ws
        N = int(ws) * int(ws)
        s1, s2, s3 = (float(g[pre + 'scale/' + k][0]) for k in ('qact1', 'qact2', 'qact3'))
        assert s2 <= R.S_Q2_MAX
        tab = R.softmax_table(s2)
        assert np.array_equal(tab, g[pre + 'softmax_table'].astype(np.int64)) and tab[0] == (1 << 21) - 1
        q1 = torch.from_numpy(g[pre + 'taps/nomask/qact1'].astype(np.int64))
        B_ = q1.shape[0]
        v = q1.reshape(B_, N, 3, heads, dim // heads).permute(2, 0, 3, 1, 4)[2]
        a2 = torch.from_numpy(g[pre + 'taps/nomask/qact2'].astype(np.int64)).reshape(B_, heads, N, N)
        region = torch.from_numpy(g[pre + 'region'].astype(np.int64))
        mask = (region.unsqueeze(1) != region.unsqueeze(2)).float() * -100.0
        for tag, msk in (('nomask', None), ('mask', mask)):
            q3 = R.table_softmax_pv(a2, v, R.allowed_of_mask(msk, B_), tab, s1 / s3).transpose(1, 2).reshape(B_, N, dim).numpy()
            d = q3 - g[pre + 'taps/%s/qact3' % tag].reshape(B_, N, dim).astype(np.int64)
            nd, n, mx = int((d != 0).sum()), int(d.size), int(np.abs(d).max())
            print('ws %2d seed %d %-6s: %d of %d qact3 codes differ from the reference (max %d)' % (ws, seed, tag, nd, n, mx))
            assert [nd, n, mx] == [int(t) for t in g[pre + 'stage_diff/' + tag]]
            assert mx <= 1 and nd * 1000 <= cap * n, (ws, tag, nd, n, mx)
        # the mask moves the result: the two runs of the fixture are told apart
        assert not np.array_equal(g[pre + 'taps/nomask/qact3'].astype(np.int64), g[pre + 'taps/mask/qact3'].astype(np.int64))


def test_module_graph_against_the_helper(dva, monkeypatch):
    """the module graph of swin.py under Config(True, False) (torch's fp32 softmax) against the helper's whole-model forward on the calibrated
    micro model: how many logit codes differ is recorded, without a cap"""
    m, x = R.micro_swin(dva)
    calib = m.export_calib()
    s2 = [float(v) for k, v in calib.items() if k.endswith('attn.qact2')]
    assert len(s2) == sum(m.arch['depths']) and max(s2) <= R.S_Q2_MAX
    want = R.quant_forward(monkeypatch, m.arch, m.state_dict(), calib, x, 8)
    for mod in m._q_modules():                  # every module fake-quantises; the frozen engine is not asked (no GPU here)
        assert mod.quant and not mod.calibrate
    with torch.no_grad():
        got = m.act_out(m.head(m.forward_features(x), m.global_distance))
    s_o = float(calib['act_out'].reshape(-1)[0])
    d = torch.round((got - want) / s_o).abs()
    print('module graph vs helper: %d of %d logit codes differ (max %d)' % (int((d > 0).sum()), d.numel(), int(d.max())))
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    # the helper is not the log-int-softmax oracle in disguise
    import _swin_bits_ref as RB
    assert not torch.equal(want, RB.uniform_oracle(m, x, 8))


def test_ddv_tool_refuses_attention_without_lis(dva):
    """refused before a model is built or anything runs"""
    with pytest.raises(NotImplementedError, match='--attention --no-lis'):
        dva.ddv.main(['--model', 'swin_tiny', '--attention', '--no-lis', '--n', '2', '--steps', '1', '--device', 'cpu'])


def test_freeze_refusals(dva):
    """ptf=False stays refused for a Swin model, whatever lis; (True, False) passes the configuration check and fails only for want of a GPU"""
    from diff_vit_amd import swin
    for ptf, lis in ((False, True), (False, False)):
        s = swin.swin_micro_patch4_window7_56(cfg=dva.Config(ptf, lis, 'minmax'), num_classes=10).eval()
        with pytest.raises(NotImplementedError, match='ptf'):
            s.freeze('cpu')
    s = swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, False, 'minmax'), num_classes=10).eval()
    with pytest.raises(RuntimeError, match='needs a GPU device'):
        s.freeze('cpu')
