"""CPU: the stage statistics (diff_vit_amd.stats) - the numpy restatement of the record (tests/_stats_ref.py) and ``code_stats_cpu`` on the
REAL reference's codes of tests/golden/micro_vit.npz, ``compute_stats`` on the CPU micro model against those codes, ``merge``, refusals."""
import numpy as np
import pytest
import torch

import _stats_ref as SR
from conftest import golden_calib, load_golden
from test_ddv import micro_model


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def stage_of(tap):
    """tap name of the fixture -> (stage name, codes as the record's element kind) or None: attn.qact0 / mlp.qact0 are no stages"""
    if tap.endswith('.qact0'):
        return None
    return tap.replace('attn.softmax_k', 'attn.log_int_softmax')


def fixture_codes(g, tag):
    """stage name -> the reference's codes (int8; the softmax exponents as uint8), every stage the fixture has under bit list ``tag``"""
    out = {}
    pre = 'taps/%s/' % tag
    for k in g.files:
        if k.startswith(pre) and stage_of(k[len(pre):]) is not None:
            v = g[k]
            assert v.min() >= -128 and v.max() <= 127
            nm = stage_of(k[len(pre):])
            out[nm] = v.astype(np.int8).view(np.uint8) if nm.endswith('log_int_softmax') else v.astype(np.int8)
    return out


def test_helper_and_cpu_twin_on_the_reference_codes(dva):
    g = load_golden('micro_vit')
    seen = 0
    for tag in ('q8', 'q4', 'qmix'):
        codes = fixture_codes(g, tag)
        if tag == 'q4':
            assert not codes            # the fixture stores the taps of the 8-bit and of the mixed list
            continue
        assert len(codes) == 2 * 9 + 5
        st = dva.stats.code_stats_cpu([torch.from_numpy(v) for v in codes.values()], list(codes))
        for nm, v in codes.items():
            r = SR.record(v)
            wide = v.astype(np.int64).reshape(-1, v.shape[-1])
            assert int(r['count']) == v.size and int(r['hist'].sum()) == v.size
            assert int(r['lo'].min()) == int(wide.min()) and int(r['hi'].max()) == int(wide.max())
            assert np.array_equal(r['sum'], wide.sum(0)) and np.array_equal(r['sumsq'], (wide * wide).sum(0))
            assert not r['nonfinite'].any()
            SR.same(SR.fields_of(st.record(nm)), r, (tag, nm))
            assert st.kind(nm) == ('u8' if nm.endswith('log_int_softmax') else 'i8')
            seen += 1
    assert seen == 2 * 23
    # fp32: specials, both zeros, denormals, a column without a finite element
    x = np.array([[1.5, -0.0, np.nan, 1e-40], [-2.0, 0.0, np.nan, -1e-41], [np.inf, -np.inf, np.nan, 0.0]], np.float32)
    r = SR.record(x)
    assert r['nonfinite'].tolist() == [3, 1, 1] and int(r['hist'][255]) == 5 and int(r['hist'][0]) == 5 and not r['sum'].any()
    assert r['lo'].view(np.uint32).tolist() == [0xc0000000, 0x80000000, 0x7f800000, np.float32(-1e-41).view(np.uint32)]
    assert r['hi'].view(np.uint32).tolist() == [0x3fc00000, 0x00000000, 0xff800000, np.float32(1e-40).view(np.uint32)]
    SR.same(SR.fields_of(dva.stats.code_stats_cpu([torch.from_numpy(x)]).record('0')), r, 'fp32 specials')


def test_compute_stats_cpu_model_against_the_reference_codes(dva, synth, oracle):
    """a calibrated CPU model has no engine: compute_stats hooks the same-named modules, whose outputs are the fake-quantised values
    code * scale (fp32 products), so per channel the range is fl(lo * s_c) ... fl(hi * s_c) of the reference's codes - exactly."""
    from _ddv_full_ref import load_reference_calibration
    g = load_golden('micro_vit')
    m = micro_model(dva, synth, g)
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']))
    c = golden_calib(g, oracle)
    load_reference_calibration(m, c)
    x = torch.from_numpy(g['x_ev'])
    for tag, bits in (('q8', [8] * 10), ('qmix', [int(b) for b in g['bit_qmix']])):
        st = dva.compute_stats(m, x, bits, with_linear=False, stages='full', attention=True)
        assert st.names == dva.ddv.stage_names(2, False, True, True)
        codes = fixture_codes(g, tag)
        assert set(codes) <= set(st.names)
        for nm, v in codes.items():
            r = SR.record(v)
            lo, hi = st.channel_ranges(nm)
            if nm.endswith('log_int_softmax'):              # the module's output is the probability 2^-k, 0 from k = 16 on
                p = np.where(v >= 16, np.float32(0), np.ldexp(np.float32(1), -np.minimum(v, 16).astype(np.int32))).astype(np.float32)
                rp = SR.record(p)
                want_lo, want_hi = rp['lo'], rp['hi']
            else:
                s = c[nm].reshape(-1).numpy().astype(np.float32)
                want_lo, want_hi = r['lo'].astype(np.float32) * s, r['hi'].astype(np.float32) * s
            assert np.array_equal(lo.numpy(), want_lo) and np.array_equal(hi.numpy(), want_hi), (tag, nm)
            assert int(st.record(nm)['count']) == v.size and st.kind(nm) == 'f32'
    # the three bit lists run; with_linear adds the layer outputs in front of their QActs
    st = dva.compute_stats(m, x, [4] * 10)
    assert st.names == dva.ddv.stage_names(2, True) and all(int(st.record(nm)['count']) > 0 for nm in st.names)
    # a float model: the same names, finite ranges
    fp = micro_model(dva, synth, g)
    sf = dva.compute_stats(fp, x)
    assert sf.names == st.names and all(torch.isfinite(torch.stack(sf.channel_ranges(nm))).all() for nm in sf.names)


def test_merge_is_exact_and_commutative(dva):
    gen = np.random.RandomState(7)
    a = [gen.randint(-128, 128, (5, 9, 20)).astype(np.int8), gen.randint(0, 256, (5, 3, 10)).astype(np.uint8),
         (gen.standard_normal((5, 4, 7)) * np.exp2(gen.randint(-30, 30, (5, 4, 7)))).astype(np.float32)]
    a[2][0, 0, 0], a[2][1, 1, 1], a[2][2, 2, 2], a[2][:, :, 3] = np.nan, -0.0, -np.inf, np.inf
    t = [torch.from_numpy(v) for v in a]
    A = dva.stats.code_stats_cpu([v[:2] for v in t])
    B = dva.stats.code_stats_cpu([v[2:] for v in t])
    whole = dva.stats.code_stats_cpu(t)
    ab, ba = A.merge(B), B.merge(A)
    assert torch.equal(ab.arena, whole.arena) and torch.equal(ba.arena, whole.arena)
    for k, v in enumerate(a):
        SR.same(SR.fields_of(ab.record(str(k))), SR.record(v), k)
        SR.same(SR.merge(SR.record(v[:2]), SR.record(v[2:])), SR.record(v), k)
    into = dva.stats.code_stats_cpu([v[:2] for v in t])
    assert dva.stats.code_stats_cpu([v[2:] for v in t], into=into) is into and torch.equal(into.arena, whole.arena)
    empty = dva.stats.code_stats_cpu([v[:0] for v in t])
    assert torch.equal(empty.merge(whole).arena, whole.arena)
    # derived views
    lo, hi = whole.channel_ranges('0')
    assert lo.dtype == torch.float32 and torch.equal(lo, torch.from_numpy(a[0].reshape(-1, 20).min(0).astype(np.float32)))
    n = a[0].size
    assert whole.rail_share('0') == (int((a[0] == -128).sum()) / n, int((a[0] == 127).sum()) / n)
    p = np.bincount(a[1].reshape(-1), minlength=256) / a[1].size
    assert abs(whole.used_bits('1') - float(-(p[p > 0] * np.log2(p[p > 0])).sum())) < 1e-12
    mean, var = whole.channel_mean_var('0')
    w = a[0].reshape(-1, 20).astype(np.float64)
    assert np.allclose(mean.numpy(), w.mean(0), rtol=1e-14, atol=0) and np.allclose(var.numpy(), w.var(0), rtol=1e-12, atol=0)
    with pytest.raises(NotImplementedError):
        whole.channel_mean_var('2')


def test_refusals(dva, monkeypatch):
    # the command line refuses before anything is built or run
    from diff_vit_amd import harness
    monkeypatch.setattr(harness, 'str2model', lambda name: pytest.fail('a model was built'))
    with pytest.raises(NotImplementedError):
        dva.stats.main(['--model', 'deit_tiny', '--attention', '--no-lis'])
    with pytest.raises(NotImplementedError):
        dva.stats.main(['--model', 'swin_tiny', '--bits', 'mixed'])
    assert 'code_stats' in dva.ops.OPS
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.code_stats([torch.zeros(2, 3, 4, dtype=torch.int8)])
    E = dva.engine
    L = E.lib()
    assert L.p2v_stats_bytes(0) == 0 and L.p2v_stats_bytes(10) == SR.record_bytes(10) == 2320 and L.p2v_stats_bytes(64) == 2080 + 24 * 64
    assert L.p2v_stats_init(None, 4096, 0, 10, None) == E.E_ARG
    op = E.Op()
    op.kind = E.OP_STATS
    assert L.p2v_run_ops((E.Op * 1)(op), 1, None) == E.E_ARG and b'P2V_OP_STATS' in L.p2v_last_error()
    fp = dva.swin.swin_micro_patch4_window7_56(num_classes=10).eval()
    with pytest.raises(NotImplementedError):
        dva.compute_stats(fp, torch.zeros(1, 3, 56, 56), [8] * 4)
