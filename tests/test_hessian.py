"""CPU: per-layer Hessian traces (diff_vit_amd.hessian) against the REAL reference's Hutchinson loop (tests/golden/hessian_micro.npz,
recorded by tools/gen_golden_hessian.py), against a dense Hessian, and the wiring into the harness."""
import ctypes
import math
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import load_golden


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def gold():
    return load_golden('hessian_micro')


def _micro(dva, cfg=None, seed=None):
    a = dva.synth.ARCHS['micro']
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=cfg or dva.Config())
    m.arch = dict(a)
    if seed is not None:
        m.load_state_dict(dva.synth.vit_state_dict(a, seed), strict=False)
    return m.eval()


def _batches(dva, g):
    n, size = int(g['batch']), dva.synth.ARCHS['micro']['img_size']
    return [(dva.synth.images(int(g['image_seed']), n, size, offset=b * n), torch.from_numpy(g['b%d/labels' % b])) for b in range(int(g['n_batches']))]


def _sequences(g, b):
    counts, flat = g['b%d/counts' % b], g['b%d/values' % b]
    ends = np.cumsum(counts)
    return [flat[e - c:e] for c, e in zip(counts, ends)]


@pytest.fixture(scope='module')
def pinned(dva, gold):
    """the project's loop on the project's micro-ViT under the fixture's torch seed: computed once, never modified"""
    if str(gold['torch_version']) != torch.__version__:
        state = torch.get_rng_state()
        torch.manual_seed(int(gold['seed']))
        p = dva.select_params(_micro(dva, seed=int(gold['weight_seed'])))[1][0]
        first = torch.randint_like(p, high=2).reshape(-1)[:64] * 2 - 1
        torch.set_rng_state(state)
        if not np.array_equal(first.numpy(), gold['b0/first_signs']):
            pytest.fail('torch %s draws other signs than the torch %s that recorded the fixture: regenerate it (tools/gen_golden_hessian.py)'
                        % (torch.__version__, gold['torch_version']))
    model = _micro(dva, seed=int(gold['weight_seed']))
    torch.manual_seed(int(gold['seed']))
    out = [dva.hutchinson_traces(model, nn.CrossEntropyLoss(), x, y, max_iter=int(gold['max_iter']), tol=float(gold['tol']), probes='layer',
                                 rng='torch') for x, y in _batches(dva, gold)]
    return out


def test_select_params(dva, gold):
    names = [str(n) for n in gold['names']]
    m = _micro(dva)
    ref, lay = dva.select_params(m, 'reference'), dva.select_params(m, 'layers')
    assert ref[0] == names == lay[0] and all(a is b for a, b in zip(ref[1], lay[1]))
    assert len(names) == 4 * m.depth + 1
    t = dva.deit_tiny_patch16_224(cfg=dva.Config())
    r, l = dva.select_params(t, 'reference'), dva.select_params(t, 'layers')
    assert r[0] == l[0] and len(r[0]) == 49 == len(t.flops()) - 1            # search asserts len(FLOPs) - 1 == len(global_distance) == len(mean_hessian)
    assert r[0][:5] == ['blocks.0.attn.qkv.weight', 'blocks.0.attn.proj.weight', 'blocks.0.mlp.fc1.weight', 'blocks.0.mlp.fc2.weight',
                        'blocks.1.attn.qkv.weight'] and r[0][-1] == 'head.weight'
    assert r[0][:4] == names[:4] and names[-1] == 'head.weight'
    with pytest.raises(ValueError):
        dva.select_params(m, 'all')


def test_select_layers_matches_global_distance_of_a_calibrated_model(dva):
    m = _micro(dva, seed=3)
    _, flops, gd = dva.harness.calibrate_model(m, dva.synth.images(2, 2, 32))
    assert len(dva.select_params(m)[0]) == len(gd) == len(flops) - 1


def test_stop_scan_reproduces_the_reference(dva, gold):
    tol = float(gold['tol'])
    for b in range(int(gold['n_batches'])):
        for seq, count, trace in zip(_sequences(gold, b), gold['b%d/counts' % b], gold['b%d/traces' % b]):
            got, probes, conv = dva.hessian.stop_scan(seq, tol)
            assert probes == int(count) and (conv or probes == int(gold['max_iter']))
            assert abs(got - float(trace)) <= 1e-12 * abs(float(trace))
            if conv:                                                    # values behind the stop are ignored
                assert dva.hessian.stop_scan(list(seq) + [1e30, -1e30], tol) == (got, probes, True)
    assert float(gold['margin']) >= 0.01


def test_stop_scan_by_hand(dva):
    S = dva.hessian.stop_scan
    assert S([2.0, 2.0], 5e-3) == (2.0, 2, True)                       # probe 0: |2 - 0| / 1e-6 is no stop; probe 1: the mean stays
    assert S([4.0, 4.0 + 1e-3, 9.0], 5e-3) == (4.0, 2, True)           # returns the PREVIOUS prefix mean, not (4 + 4.001) / 2
    vals = [float((-2) ** k) for k in range(10)]
    trace, probes, conv = S(vals, 5e-3)
    assert (probes, conv) == (10, False) and trace == sum(vals) / 10   # never stops: the last mean
    assert S([0.0, 0.0, 5.0], 5e-3) == (0.0, 1, True)                  # an exact zero converges at once on trace 0.0 - ONE entry
    assert S([0.0] * 4, 0.0) == (0.0, 4, False)                        # tol 0 never stops
    assert S([3.0], 5e-3) == (3.0, 1, False) and S([], 5e-3) == (0.0, 0, False)


def test_pinned_to_the_reference(dva, gold, pinned):
    """probes='layer', rng='torch' under the reference's seed: same names and probe counts, every per-probe value within 1e-5 relative
    (the project's float-parity bound) of what the reference's own loop recorded on the reference's own model"""
    worst = 0.0
    for b, (names, traces, info) in enumerate(pinned):
        assert names == [str(n) for n in gold['names']]
        assert info['probes'] == [int(c) for c in gold['b%d/counts' % b]]
        for got, want in zip(info['values'], _sequences(gold, b)):
            assert len(got) == len(want)
            rel = np.abs(np.asarray(got) - want) / np.abs(want)
            worst = max(worst, float(rel.max()))
    print('largest relative difference of a per-probe value: %.3g' % worst)
    assert worst <= 1e-5


def test_mean_hessian_matches_the_reference(dva, gold, pinned):
    got = dva.hessian.normalise_traces([t for _, t, _ in pinned])
    want = gold['mean_hessian']
    assert len(got) == len(want) and min(got) >= 0.0 and max(got) <= 1.0
    assert np.abs(np.asarray(got) - want).max() <= 1e-12
    # the public entry point is the same composition
    model = _micro(dva, seed=int(gold['weight_seed']))
    torch.manual_seed(int(gold['seed']))
    mh = dva.mean_hessian(model, nn.CrossEntropyLoss(), _batches(dva, gold), max_iter=int(gold['max_iter']), tol=float(gold['tol']),
                          probes='layer', rng='torch')
    assert mh == got
    with pytest.raises(ValueError, match='same'):
        dva.hessian.normalise_traces([[2.0, -2.0, 2.0]])


class _Tiny(nn.Module):
    """the layer kinds of a ViT block at a size whose dense Hessian is cheap: Linear, LayerNorm, GELU, one softmax attention head"""

    def __init__(self, d=8, hidden=16, classes=4):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.qkv, self.proj = nn.Linear(d, 3 * d), nn.Linear(d, d)
        self.fc1, self.fc2, self.head = nn.Linear(d, hidden), nn.Linear(hidden, d), nn.Linear(d, classes)
        self.d = d

    def forward(self, x):
        q, k, v = self.qkv(self.norm1(x)).split(self.d, dim=-1)
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(self.d), dim=-1)
        x = x + self.proj(att @ v)
        x = x + self.fc2(nn.functional.gelu(self.fc1(self.norm2(x))))
        return self.head(x[:, 0])


def test_exact_against_a_dense_hessian(dva):
    """no statistics: for three counter-generator probes the 'layer' value is v_l^T H_ll v_l and the 'joint' value v_l^T (H v)_l of the
    dense Hessian, within 1e-9 * sum |H_ij| (orders above fp64 rounding, orders below an indexing or sign mistake)"""
    torch.manual_seed(5)
    m = _Tiny().double().eval()
    for p in m.parameters():
        p.data.mul_(3.0)
    x, y = torch.randn(3, 4, 8, dtype=torch.float64), torch.tensor([0, 3, 1])
    crit = nn.CrossEntropyLoss()
    names, params = dva.select_params(m)
    sizes = [p.numel() for p in params]
    assert names == ['qkv.weight', 'proj.weight', 'fc1.weight', 'fc2.weight', 'head.weight'] and sum(sizes) <= 800 and max(sizes) <= 256

    def loss_of(flat):
        parts = flat.split(sizes)
        return crit(torch.func.functional_call(m, {n: t.view_as(p) for n, t, p in zip(names, parts, params)}, (x,)), y)
    H = torch.autograd.functional.hessian(loss_of, torch.cat([p.detach().reshape(-1) for p in params]))
    bound = 1e-9 * float(H.abs().sum())
    offs = np.concatenate([[0], np.cumsum(sizes)])
    seed, n_probes = 11, 3
    vs = [[torch.from_numpy(dva.hessian.rademacher_host(seed, l, i, n)).double() for l, n in enumerate(sizes)] for i in range(n_probes)]
    got = {mode: dva.hutchinson_traces(m, crit, x, y, max_iter=n_probes, tol=0.0, probes=mode, rng='counter', seed=seed)[2] for mode in ('layer', 'joint')}
    cross = 0.0
    for mode in ('layer', 'joint'):
        assert got[mode]['probes'] == [n_probes] * len(sizes) and got[mode]['converged'] == [False] * len(sizes)
        assert got[mode]['hvps'] == (n_probes * len(sizes) if mode == 'layer' else n_probes)
    for i in range(n_probes):
        Hv = H @ torch.cat(vs[i])
        for l in range(len(sizes)):
            a, b = offs[l], offs[l + 1]
            diag = float(vs[i][l] @ H[a:b, a:b] @ vs[i][l])
            joint = float(vs[i][l] @ Hv[a:b])
            assert abs(got['layer']['values'][l][i] - diag) <= bound
            assert abs(got['joint']['values'][l][i] - joint) <= bound
            cross = max(cross, abs(joint - diag))
    assert cross > 1e3 * bound                                          # the two modes differ by the off-diagonal blocks, visibly


def test_rademacher_host(dva):
    R = dva.hessian.rademacher_host
    v = R(0, 0, 0, 4096)
    assert v.dtype == np.float32 and set(np.unique(v)) == {-1.0, 1.0}
    assert abs(float(v.sum())) <= 5 * math.sqrt(4096)                  # 4096 fair signs: sigma of the sum is 64
    for n in (1, 63, 64, 65, 1000):
        assert np.array_equal(R(3, 2, 1, n), R(3, 2, 1, 4096)[:n])     # counter based: a prefix of a longer draw
    base = R(3, 2, 1, 4096)
    for other in (R(4, 2, 1, 4096), R(3, 3, 1, 4096), R(3, 2, 2, 4096), R(3, 1, 2, 4096)):
        agree = float((other == base).mean())
        assert abs(agree - 0.5) <= 5 * 0.5 / math.sqrt(4096)           # an independent stream agrees on half the signs
    assert np.array_equal(R(2 ** 64 + 3, 2, 1, 100), R(3, 2, 1, 100))   # the seed is taken mod 2^64


def test_result_does_not_depend_on_check_every(dva):
    m = _micro(dva, seed=4)
    x, y = dva.synth.images(9, 4, 32), torch.tensor([1, 7, 3, 0])
    crit = nn.CrossEntropyLoss()
    for mode in ('layer', 'joint'):
        runs = [dva.hutchinson_traces(m, crit, x, y, max_iter=24, tol=3e-2, probes=mode, seed=2, check_every=c) for c in (1, 8, 150)]
        stopped = sum(runs[0][2]['converged'])
        assert 0 < stopped, 'the case should stop some layers early'
        for names, traces, info in runs[1:]:
            assert traces == runs[0][1] and info['probes'] == runs[0][2]['probes'] and info['values'] == runs[0][2]['values']
            assert info['converged'] == runs[0][2]['converged']
        if mode == 'layer':
            assert runs[0][2]['hvps'] < runs[2][2]['hvps']              # a later look costs double backwards, never a result


def test_refusals(dva):
    m = _micro(dva, seed=4)
    x, y = dva.synth.images(9, 2, 32), torch.tensor([1, 7])
    crit = nn.CrossEntropyLoss()
    for bad in (dict(probes='both'), dict(rng='numpy'), dict(max_iter=0), dict(check_every=0), dict(select='all')):
        with pytest.raises(ValueError):
            dva.hutchinson_traces(m, crit, x, y, **bad)
    with pytest.raises(ValueError):
        dva.hessian.hessian(m, crit)
    names, traces = dva.hessian.hessian(m, crit, data=(x, y), cuda=False, probes='joint').trace(maxIter=2)
    assert names == dva.select_params(m)[0] and len(traces) == len(names)
    dva.harness.calibrate_model(m, x)
    with pytest.raises(ValueError, match='float model'):
        dva.hutchinson_traces(m, crit, x, y)


_ONE = ctypes.c_void_p(4096)


def _refused(L, rc, code, text):
    assert rc == code, (rc, L.p2v_last_error())
    assert text in L.p2v_last_error(), L.p2v_last_error()


def test_entry_points_refuse_bad_arguments_without_a_gpu(dva):
    """argument validation happens before any HIP call"""
    E = dva.engine
    L = E.lib()
    ok = (E.Seg * 2)(E.Seg(4096, 5, 0), E.Seg(8192 + 4, 1, 7))
    fill = lambda segs=ok, n=2: L.p2v_rademacher_fill(segs, n, 1, 0, None)
    for n in (0, -1, 65537):
        _refused(L, fill(n=n), E.E_ARG, b'p2v_rademacher_fill: n_segs = %d' % n)
    _refused(L, fill(segs=None), E.E_ARG, b'p2v_rademacher_fill: null argument')
    for seg, text in ((E.Seg(None, 5, 0), b'segment 1: null or misaligned pointer'), (E.Seg(4098, 5, 0), b'segment 1: null or misaligned pointer'),
                      (E.Seg(4096, 0, 0), b'segment 1: n = 0'), (E.Seg(4096, -4, 0), b'segment 1: n = -4'), (E.Seg(4096, 2 ** 31, 0), b'segment 1: n = 2147483648')):
        _refused(L, fill(segs=(E.Seg * 2)(ok[0], seg)), E.E_ARG, text)

    ok2 = (E.Seg2 * 2)(E.Seg2(4096, 8192, 5), E.Seg2(8192 + 4, 4096 + 8, 4100))
    assert L.p2v_group_dot_workspace_bytes(ok2, 2) == 8 * (1 + 2)          # chunks of 1024 quads behind the head: 1, and 3 + 4097 -> 1025 quads -> 2
    assert L.p2v_group_dot_workspace_bytes(ok2, 0) == 0 and L.p2v_group_dot_workspace_bytes(None, 2) == 0
    dot = lambda segs=ok2, n=2, out=_ONE, ws=_ONE, ws_bytes=24: L.p2v_group_dot(segs, n, out, ws, ws_bytes, None)
    _refused(L, dot(n=0), E.E_ARG, b'p2v_group_dot: n_segs = 0')
    _refused(L, dot(segs=None), E.E_ARG, b'p2v_group_dot: null argument')
    for seg, text in ((E.Seg2(None, 8192, 5), b'segment 0: null or misaligned pointer'), (E.Seg2(4096, None, 5), b'segment 0: null or misaligned pointer'),
                      (E.Seg2(4096, 8193, 5), b'segment 0: null or misaligned pointer'), (E.Seg2(4096, 8192, 0), b'segment 0: n = 0'),
                      (E.Seg2(4096, 8192, 2 ** 31), b'segment 0: n = 2147483648')):
        bad = (E.Seg2 * 2)(seg, ok2[1])
        _refused(L, dot(segs=bad), E.E_ARG, text)
        assert L.p2v_group_dot_workspace_bytes(bad, 2) == 0
    _refused(L, dot(out=None), E.E_ARG, b'p2v_group_dot: null argument')
    _refused(L, dot(ws=None), E.E_ARG, b'p2v_group_dot: null argument')
    _refused(L, dot(ws=ctypes.c_void_p(4100)), E.E_ARG, b'8-byte aligned')
    _refused(L, dot(ws_bytes=23), E.E_WORKSPACE, b'p2v_group_dot: workspace 23 < 24 bytes')

    need = L.p2v_hutchinson_state_bytes(2)
    assert need == E.HS_HEADER_BYTES + 2 * E.HS_LAYER_BYTES and L.p2v_hutchinson_state_bytes(0) == 0
    _refused(L, L.p2v_hutchinson_init(None, need, 2, None), E.E_ARG, b'p2v_hutchinson_init: null or misaligned state')
    _refused(L, L.p2v_hutchinson_init(_ONE, need - 1, 2, None), E.E_WORKSPACE, b'p2v_hutchinson_init: state')
    _refused(L, L.p2v_hutchinson_init(_ONE, need, 0, None), E.E_ARG, b'p2v_hutchinson_init: n_segs = 0')
    step = lambda segs=ok2, n=2, probe=0, max_iter=4, tol=5e-3, record=_ONE, state=_ONE, sb=need, ws=_ONE, wb=24: \
        L.p2v_hutchinson_step(segs, n, probe, max_iter, tol, record, state, sb, ws, wb, None)
    _refused(L, step(n=0), E.E_ARG, b'p2v_hutchinson_step: n_segs = 0')
    _refused(L, step(record=None), E.E_ARG, b'p2v_hutchinson_step: null argument')
    _refused(L, step(state=None), E.E_ARG, b'p2v_hutchinson_step: null or misaligned state')
    for probe, max_iter in ((-1, 4), (4, 4), (0, 0)):
        _refused(L, step(probe=probe, max_iter=max_iter), E.E_ARG, b'p2v_hutchinson_step: probe %d outside' % probe)
    _refused(L, step(tol=float('nan')), E.E_ARG, b'p2v_hutchinson_step: tol is not a number')
    _refused(L, step(sb=need - 1), E.E_WORKSPACE, b'p2v_hutchinson_step: state')
    _refused(L, step(wb=8), E.E_WORKSPACE, b'p2v_hutchinson_step: workspace 8 < 24 bytes')
    with pytest.raises(E.P2VError):
        E.check(E.E_ARG)


def test_ops_registered_gpu_only_and_exported(dva):
    for name in ('rademacher_fill', 'group_dot', 'hutchinson_init', 'hutchinson_step'):
        assert name in dva.ops.OPS and hasattr(torch.ops.p2vit, name)
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.group_dot([torch.ones(3)], [torch.ones(3)])
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.rademacher_fill([torch.ones(3)], [0], 0, 0)
    for name in ('hutchinson_traces', 'mean_hessian', 'select_params'):
        assert name in dva.__all__ and getattr(dva, name) is getattr(dva.hessian, name)
    assert dva.engine.P2V_ABI_VERSION == 6 == dva.engine.lib().p2v_abi_version()


class _Stop(Exception):
    pass


def test_harness_hands_the_search_its_weights(dva, monkeypatch, capsys):
    """--mixed --hessian-batches 1 computes the vector on the float model BEFORE the calibration and passes it on; 0 passes None"""
    seen, order = [], []

    def spy(score, FLOPs, global_distance, mean_hessian=None, **kw):
        seen.append((mean_hessian, len(global_distance)))
        raise _Stop()
    real_cal = dva.harness.calibrate_model
    monkeypatch.setattr(dva.harness, 'calibrate_model', lambda *a, **k: order.append('calibrate') or real_cal(*a, **k))
    real_mh = dva.hessian.mean_hessian
    monkeypatch.setattr(dva.hessian, 'mean_hessian', lambda model, *a, **k: order.append('hessian quant=%s' % model.quant) or real_mh(model, *a, **k))
    monkeypatch.setattr(dva.search, 'mixed_precision_search', spy)
    monkeypatch.setattr(dva.harness, 'str2model', lambda name: (lambda pretrained=False, cfg=None: _micro(dva, cfg)))
    argv = ['--model', 'micro', '--quant', '--mixed', '--device', 'cpu', '--calib-batchsize', '2', '--n-val', '8', '--val-batchsize', '4']
    with pytest.raises(_Stop):
        dva.harness.main(argv + ['--hessian-batches', '1', '--hessian-batch-size', '4', '--hessian-probes', 'joint'])
    out = capsys.readouterr().out
    mh, n = seen[-1]
    assert order == ['hessian quant=False', 'calibrate'] and '***Trace: ' in out
    assert n == 9 and len(mh) == n and min(mh) == 0.0 and max(mh) == 1.0 and len(set(mh)) > 2
    order.clear()
    with pytest.raises(_Stop):
        dva.harness.main(argv)
    assert seen[-1] == (None, 9) and order == ['calibrate'] and '***Trace' not in capsys.readouterr().out
    d = dva.harness.build_parser().parse_args([])
    assert (d.hessian_batches, d.hessian_batch_size, d.hessian_probes) == (0, 32, 'joint')
