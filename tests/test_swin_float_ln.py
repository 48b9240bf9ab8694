"""CPU: Config(ptf=False) of a Swin model - the restatement of tests/_swin_float_ln_ref.py against the product's own module graph
(torch's fp32 F.layer_norm), the float LayerNorm helper against F.layer_norm at every Swin width up to 4096 channels, and the argument
checks of p2v_float_layernorm / P2V_OP_FLOAT_LAYERNORM around the 4096-channel limit (host side: nothing is launched, no GPU is needed)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _swin_float_ln_ref as R
from _float_ops_ref import float_layernorm


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def E(dva):
    from diff_vit_amd import engine
    engine.lib()
    return engine


# ---- the restatement against the module graph ------------------------------------------------------------------------------------------
def _graph_vs_restatement(dva, cfg):
    m, x = R.micro_swin(dva, cfg)
    calib = m.export_calib()
    assert all(v.numel() == 1 for k, v in calib.items() if not isinstance(v, dict)), 'ptf=False: every QAct has one scale'
    assert all(type(n) is not dva.QIntLayerNorm or (n.mode == 'ln' and n.eps == R.SWIN_EPS) for n in m.modules())
    for mod in m._q_modules():                  # every module fake-quantises; the frozen engine is not asked (no GPU here)
        assert mod.quant and not mod.calibrate
    with torch.no_grad():
        graph = m.act_out(m.head(m.forward_features(x), m.global_distance))
    want = R.quant_forward(m.arch, m.state_dict(), calib, x, 8, lis=cfg[1])
    s_o = float(calib['act_out'].reshape(-1)[0])
    d = (torch.round(graph / s_o) - torch.round(want / s_o)).abs()
    print('Config%r: %d of %d logit codes of the module graph differ from the restatement (max %d)'
          % (cfg, int((d > 0).sum()), d.numel(), int(d.max())))
    assert graph.shape == want.shape == (3, 10) and bool(torch.isfinite(graph).all())
    return m, x, want, d


def test_module_graph_equals_the_restatement_under_lis(dva):
    """Config(False, True) on the calibrated micro Swin, 3 images, bits = 8: the module graph (F.layer_norm in fp32) and the restatement
    (the fp64 chain on integer sums) give the same 30 logit codes.  And the restatement is not the integer-LayerNorm oracle in disguise:
    handed the same scales, that one computes other logits."""
    m, x, want, d = _graph_vs_restatement(dva, (False, True))
    assert int((d > 0).sum()) == 0
    import swin_oracle as SO
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        int_ln = SO.OracleSwin(m.arch, sd).quant_forward(x, R.expand_calib(m.export_calib(), sd), 8)
    assert not torch.equal(int_ln, want)


def test_module_graph_against_the_restatement_without_lis(dva):
    """Config(False, False): the distance is recorded, not capped - it is the known distance between torch's softmax and the table softmax
    (measured: 2 of 30 codes, by at most 2), not the LayerNorm's, whose link test_module_graph_equals_the_restatement_under_lis pins"""
    m, x, want, d = _graph_vs_restatement(dva, (False, False))
    assert not torch.equal(want, R.quant_forward(m.arch, m.state_dict(), m.export_calib(), x, 8, lis=True))


# ---- the helper against F.layer_norm ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_', [96, 384, 768, 1536, 2048, 2052, 3072, 4096])
def test_helper_against_torch_layer_norm(C_):
    """random codes plus the edge rows under three (s_in, s_out) pairs: no code differs from clamp(round(F.layer_norm(q s_in) / s_out)) by
    more than 1, and at most 1 code in 1 000 per width (the cap of the float operators' link rule; measured: at most 0.014 per 1 000)"""
    gen = torch.Generator().manual_seed(3 + C_)
    tot = bad = big = 0
    for s_in_e, s_out_e in ((-4, -5), (-3, -6), (-6, -4)):
        q = torch.randint(-128, 128, (64, C_), generator=gen)
        q[0], q[1], q[2] = 127, -128, 5                      # constant rows: variance exactly 0
        q[3, ::2], q[3, 1::2] = 127, -128
        q[4] = 0
        q[4, C_ // 3] = 127                                  # one-hot
        gamma = (torch.randn(C_, generator=gen) * 0.5 + 1).float()
        beta = (torch.randn(C_, generator=gen) * 0.3).float()
        s_in, s_out = 2.0 ** s_in_e, 2.0 ** s_out_e
        codes, _ = float_layernorm(q, s_in, gamma, beta, R.SWIN_EPS, torch.full((C_,), 1.0 / s_out))
        y = F.layer_norm(q.float() * s_in, (C_,), gamma, beta, R.SWIN_EPS)
        ref = torch.clamp(torch.round(y / s_out), -128, 127).long()
        d = (codes - ref).abs()
        tot += d.numel()
        bad += int((d > 0).sum())
        big += int((d > 1).sum())
    print('C %d: %d of %d codes differ from F.layer_norm (%.3f per 1000), %d by more than 1' % (C_, bad, tot, 1000.0 * bad / tot, big))
    assert big == 0 and bad * 1000 <= tot


# ---- argument checks, host side ---------------------------------------------------------------------------------------------------------
_DUMMY = C.c_void_p(4096)             # non-null, 16-byte aligned, never dereferenced


def test_entry_point_accepts_up_to_4096_channels(E):
    """2052 ... 4096 channels pass the shape check (they are refused only for the missing constants); 2050 and 4100 are refused by their
    own codes, as are rows that overlap beyond 2048 channels - all before any launch"""
    L = E.lib()
    assert hasattr(L, 'p2v_float_layernorm_max_channels') and L.p2v_float_layernorm_max_channels() == 4096
    none = E.FloatLn(0.125, 1e-5, None, None, None)
    ok = E.FloatLn(0.125, 1e-5, _DUMMY, _DUMMY, _DUMMY)
    for C_ in (2052, 3072, 4096):
        assert L.p2v_float_layernorm(_DUMMY, C_, 2, C_, C.byref(none), _DUMMY, C_, None, None) == E.E_ARG
        assert b'constants missing' in L.p2v_last_error()
    assert L.p2v_float_layernorm(_DUMMY, 2052, 2, 2050, C.byref(ok), _DUMMY, 2052, None, None) == E.E_UNSUPPORTED
    assert L.p2v_float_layernorm(_DUMMY, 4100, 2, 4100, C.byref(ok), _DUMMY, 4100, None, None) == E.E_SHAPE
    assert b'C=4100' in L.p2v_last_error() and b'4096' in L.p2v_last_error()
    assert L.p2v_float_layernorm(_DUMMY, 64, 2, 3072, C.byref(ok), _DUMMY, 3072, None, None) == E.E_SHAPE         # overlapping rows
    assert b'row_stride >= C' in L.p2v_last_error()
    assert L.p2v_float_layernorm(_DUMMY, 3072, 2, 3072, C.byref(ok), _DUMMY, 3068, None, None) == E.E_SHAPE
    assert L.p2v_float_layernorm(_DUMMY, 3072, 2, 3072, C.byref(E.FloatLn(0.3, 1e-5, _DUMMY, _DUMMY, _DUMMY)), _DUMMY, 3072, None, None) == E.E_UNSUPPORTED
    assert L.p2v_float_layernorm(_DUMMY, 3072, 2, 3072, C.byref(E.FloatLn(0.125, 0.0, _DUMMY, _DUMMY, _DUMMY)), _DUMMY, 3072, None, None) == E.E_ARG


def test_record_kind_refuses_like_the_entry_point(E):
    """P2V_OP_FLOAT_LAYERNORM = 12 is a known kind and carries its constants in lin / f0 / f1 / ep.tap_out"""
    L = E.lib()
    assert E.OP_FLOAT_LAYERNORM == 12
    o = E.Op()
    o.kind, o.inp, o.out = E.OP_FLOAT_LAYERNORM, _DUMMY, _DUMMY
    o.M, o.N, o.lda, o.ldo, o.f0, o.f1 = 2, 3072, 3072, 3072, 0.125, 1e-5
    assert L.p2v_run_ops(C.byref(o), 1, None) == E.E_ARG and b'p2v_float_layernorm: float LayerNorm constants missing' in L.p2v_last_error()
    o.lin.w_codes, o.lin.colscale, o.lin.bias = _DUMMY, _DUMMY, _DUMMY
    o.N = o.lda = o.ldo = 4100
    assert L.p2v_run_ops(C.byref(o), 1, None) == E.E_SHAPE and b'C=4100' in L.p2v_last_error()
    o.N = o.lda = o.ldo = 3072
    o.f0 = 0.3
    assert L.p2v_run_ops(C.byref(o), 1, None) == E.E_UNSUPPORTED
    o.f0 = 0.125
    o.ep.tap_out = C.c_void_p(4096 + 8)
    assert L.p2v_run_ops(C.byref(o), 1, None) == E.E_ARG and b'tap_out 16-byte aligned' in L.p2v_last_error()


def test_freeze_takes_ptf_false(dva):
    """SwinTransformer.freeze no longer refuses the configuration: a calibrated model fails without a GPU only for want of one, whatever
    lis.  A model that was never calibrated has no layer-wise scales for the float LayerNorm: refused by the first QAct's name."""
    from diff_vit_amd import swin
    for lis in (True, False):
        m, _ = R.micro_swin(dva, (False, lis))
        with pytest.raises(RuntimeError, match='needs a GPU device'):
            m.freeze('cpu')
        s = swin.swin_micro_patch4_window7_56(cfg=dva.Config(False, lis, 'minmax'), num_classes=10).eval()
        with pytest.raises(NotImplementedError, match=r'qact_input: Config\(ptf=False\) needs the one calibrated layer-wise scale'):
            s.freeze('cpu')
