"""ModelDiff's black-box profiling inputs (diff_vit_amd.profiling) without a GPU: the host loop against the REAL reference's trajectory
(tests/golden/profiling_micro.npz, run a: tools/gen_golden_profiling.py), the order of the random draws, the diversity metric, every
refusal of the p2v_profile_* entry points, the exports and the unchanged CLI default."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_ddv import micro_model


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def float_pair(dva, synth):
    """the two float micro models of fixture run a"""
    k = load_golden('profiling_micro')
    g = load_golden('micro_vit')
    m1 = micro_model(dva, synth, g)
    m2 = micro_model(dva, synth, g)
    m2.load_state_dict(synth.vit_state_dict(synth.ARCHS['micro'], int(k['seed_w2'])), strict=False)
    return m1, m2.eval(), k


def test_host_loop_matches_reference_trajectory(dva, synth):
    """All 1000 iterations the reference hard-codes, on the CPU: 11 s on 16 threads (4 full-batch micro forwards per iteration).  The float
    forward is bit-equal to the reference's on one host and the generator asserted that no decision hangs on less than 1e-9 relative, so
    a restatement within 1e-12 (fp64 sums of 10 and 16 terms in another order: a few 1e-16) must take every decision alike."""
    m1, m2, k = float_pair(dva, synth)
    rng = np.random.RandomState(int(k['a/numpy_seed']))
    trace = []
    t0 = time.time()
    x = dva.gen_profiling_inputs_in_blackbox(m1, None, m2, None, torch.from_numpy(k['a/x0']), epsilon=float(k['a/epsilon']),
                                             max_iterations=len(k['a/decision']), rng=rng, trace=trace)
    print('host loop: %d iterations in %.1f s' % (len(trace), time.time() - t0))
    t = np.array(trace, dtype=np.float64)
    assert np.array_equal(t[:, 2].astype(np.int8), k['a/decision'])
    for col, name in ((0, 'a/score_right'), (1, 'a/score_left'), (3, 'a/score')):
        rel = np.abs(t[:, col] - k[name]) / np.maximum(np.abs(k[name]), 1e-300)
        assert rel.max() <= 1e-12, (name, rel.max())
    assert np.array_equal(x.numpy(), k['a/x_final'])


def test_draws_follow_the_reference_order(dva):
    """a literal transcription of dataset_utility.py:272 and :280 inside the loop of :264"""
    want_pos, want_idx = [], []
    r = np.random.RandomState(7)
    for _ in range(25):
        want_pos.append(r.randint(0, 3 * 32 * 32))
        want_idx.append(r.randint(0, 5))
    pos, idx = dva.profiling.draw_mutations(3 * 32 * 32, 5, 25, np.random.RandomState(7))
    assert pos == want_pos and idx == want_idx
    np.random.seed(7)                                    # rng=None: the global generator, as the reference
    assert dva.profiling.draw_mutations(3 * 32 * 32, 5, 25) == (want_pos, want_idx)
    k = load_golden('profiling_micro')
    for tag in ('a', 'b'):
        pos, idx = dva.profiling.draw_mutations(3 * 32 * 32, 4, 1000, np.random.RandomState(int(k[tag + '/numpy_seed'])))
        assert np.array_equal(pos, k[tag + '/pos']) and np.array_equal(idx, k[tag + '/idx'])


class _Fixed(torch.nn.Module):
    """a 'model' with the reference's call signature whose logits are a fixed function of the inputs"""

    def __init__(self, classes):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(12, classes, generator=torch.Generator().manual_seed(3)))

    def forward(self, x, bit_config=None, plot=False):
        return x.reshape(x.shape[0], -1) @ self.w, [], []


@pytest.mark.parametrize('n', [1, 2, 7])
def test_metrics_output_diversity_cpu(dva, n):
    m = _Fixed(10)
    x = torch.randn(n, 3, 2, 2, generator=torch.Generator().manual_seed(n))
    o = m(x)[0].detach().numpy().astype(np.float64)
    d = o[:, None, :] - o[None, :, :]
    want = np.mean(np.sqrt((d * d).sum(-1)))
    got = dva.metrics_output_diversity(m, None, x)
    assert isinstance(got, float) and abs(got - want) <= 1e-12 * max(want, 1e-300)
    if n == 1:
        assert got == 0.0


def test_profile_abi_refusals(dva):
    """every refusal is made before the first HIP call, so it can be provoked on a machine without a GPU"""
    E = dva.engine
    L = E.lib()
    a16, a8, a4 = C.c_void_p(4096), C.c_void_p(4104), C.c_void_p(4100)
    big = 1 << 40
    assert L.p2v_profile_state_bytes(0, 10) == 0 and L.p2v_profile_state_bytes(1025, 10) == 0
    assert L.p2v_profile_state_bytes(4, 0) == 0 and L.p2v_profile_state_bytes(4, 65537) == 0
    nb = L.p2v_profile_state_bytes(4, 10)
    # score + pad, per model D + g + rowd + rowg, then per model O + O0
    assert nb == 8 * (2 + 2 * (16 + 4 + 8 + 2)) + 4 * (4 * 4 * 10) and L.p2v_profile_state_bytes(256, 1000) > 0
    assert L.p2v_profile_state_bytes(1024, 65536) > 0

    def init(state=a16, nbytes=big, n=4, classes=10, l1=a4, l2=a4):
        return L.p2v_profile_init(state, nbytes, n, classes, l1, l2, None)

    for bad, rc in ((dict(state=None), E.E_ARG), (dict(l1=None), E.E_ARG), (dict(l2=None), E.E_ARG), (dict(state=a8), E.E_ARG),
                    (dict(l1=C.c_void_p(4098)), E.E_ARG), (dict(n=0), E.E_SHAPE), (dict(n=1025), E.E_SHAPE), (dict(classes=0), E.E_SHAPE),
                    (dict(classes=65537), E.E_SHAPE), (dict(nbytes=nb - 1), E.E_WORKSPACE)):
        assert init(**bad) == rc, bad
        assert b'p2v_profile_init' in L.p2v_last_error()

    def cand(inputs=a16, n=4, elems=48, idx=0, pos=0, staging=a16):
        return L.p2v_profile_candidates(inputs, n, elems, idx, pos, 0.2, staging, None)

    for bad, rc in ((dict(inputs=None), E.E_ARG), (dict(staging=None), E.E_ARG), (dict(inputs=a8), E.E_ARG), (dict(staging=a4), E.E_ARG),
                    (dict(idx=-1), E.E_ARG), (dict(idx=4), E.E_ARG), (dict(pos=-1), E.E_ARG), (dict(pos=48), E.E_ARG),
                    (dict(n=0), E.E_SHAPE), (dict(n=1025), E.E_SHAPE), (dict(elems=0), E.E_SHAPE), (dict(elems=(1 << 30) + 1), E.E_SHAPE)):
        assert cand(**bad) == rc, bad
        assert b'p2v_profile_candidates' in L.p2v_last_error()

    def step(state=a16, nbytes=big, n=4, classes=10, c1=a4, c2=a4, staging=a16, inputs=a16, elems=48, idx=0, pos=0, trace=a8):
        return L.p2v_profile_step(state, nbytes, n, classes, c1, c2, staging, inputs, elems, idx, pos, trace, None)

    for bad, rc in ((dict(state=None), E.E_ARG), (dict(c1=None), E.E_ARG), (dict(c2=None), E.E_ARG), (dict(staging=None), E.E_ARG),
                    (dict(inputs=None), E.E_ARG), (dict(trace=None), E.E_ARG), (dict(state=a8), E.E_ARG), (dict(c2=C.c_void_p(4097)), E.E_ARG),
                    (dict(staging=a8), E.E_ARG), (dict(inputs=a4), E.E_ARG), (dict(trace=a4), E.E_ARG), (dict(idx=-1), E.E_ARG),
                    (dict(idx=4), E.E_ARG), (dict(pos=-1), E.E_ARG), (dict(pos=48), E.E_ARG), (dict(n=0), E.E_SHAPE),
                    (dict(n=1025), E.E_SHAPE), (dict(classes=0), E.E_SHAPE), (dict(classes=65537), E.E_SHAPE), (dict(elems=0), E.E_SHAPE),
                    (dict(nbytes=nb - 1), E.E_WORKSPACE)):
        assert step(**bad) == rc, bad
        assert b'p2v_profile_step' in L.p2v_last_error()

    def div(logits=a4, ld=10, n=4, classes=10, out=a8, ws=a8, ws_bytes=4 * 4 * 8):
        return L.p2v_profile_diversity(logits, ld, n, classes, out, ws, ws_bytes, None)

    for bad, rc in ((dict(logits=None), E.E_ARG), (dict(out=None), E.E_ARG), (dict(ws=None), E.E_ARG), (dict(logits=C.c_void_p(4098)), E.E_ARG),
                    (dict(out=a4), E.E_ARG), (dict(ws=a4), E.E_ARG), (dict(n=0), E.E_SHAPE), (dict(n=1025), E.E_SHAPE),
                    (dict(classes=0), E.E_SHAPE), (dict(ld=9), E.E_SHAPE), (dict(ws_bytes=4 * 4 * 8 - 1), E.E_WORKSPACE)):
        assert div(**bad) == rc, bad
        assert b'p2v_profile_diversity' in L.p2v_last_error()


def test_exports_and_swin_list(dva):
    assert 'gen_profiling_inputs_in_blackbox' in dva.__all__ and 'metrics_output_diversity' in dva.__all__
    assert dva.gen_profiling_inputs_in_blackbox is dva.profiling.gen_profiling_inputs_in_blackbox
    sm = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    x = torch.zeros(2, 3, 56, 56)
    with pytest.raises(NotImplementedError):
        dva.gen_profiling_inputs_in_blackbox(sm, [8] * 10, sm, 4, x, max_iterations=1)
    with pytest.raises(NotImplementedError):
        dva.metrics_output_diversity(sm, [8] * 10, x)
    # a float Swin (bare logits) runs the host loop
    tr = []
    out = dva.gen_profiling_inputs_in_blackbox(sm, None, sm, None, x, max_iterations=2, rng=np.random.RandomState(0), trace=tr)
    assert out.shape == x.shape and len(tr) == 2 and all(r[2] in (0, 1, 2) for r in tr)


def test_cli_default_is_pgd(dva, monkeypatch):
    """``ddv.main`` without --inputs takes gen_adv_inputs exactly as before and never touches the black-box generator"""
    calls = []
    real = dva.ddv.gen_adv_inputs
    monkeypatch.setattr(dva.ddv, 'gen_adv_inputs', lambda *a, **k: calls.append(('pgd', k)) or real(*a, **k))
    monkeypatch.setattr(dva.profiling, 'gen_profiling_inputs_in_blackbox', lambda *a, **k: calls.append(('blackbox', k)))

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(dva.ddv, 'compute_ddv', stop)
    monkeypatch.setattr(dva.harness, 'str2model', lambda name: (lambda cfg=None: _micro(dva, cfg)))
    with pytest.raises(Stop):
        dva.ddv.main(['--model', 'micro', '--n', '2', '--steps', '1', '--device', 'cpu'])
    assert [c[0] for c in calls] == ['pgd'] and calls[0][1] == {'num_steps': 1}
    calls.clear()
    with pytest.raises(Stop):
        dva.ddv.main(['--model', 'micro', '--n', '2', '--inputs', 'blackbox', '--mut-iters', '3', '--device', 'cpu'])
    assert [c[0] for c in calls] == ['blackbox'] and calls[0][1]['max_iterations'] == 3
    with pytest.raises(SystemExit):
        dva.ddv.main(['--inputs', 'nonsense'])


def _micro(dva, cfg):
    from functools import partial
    a = dva.synth.ARCHS['micro']
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=cfg)
    m.arch = dict(a)
    return m
