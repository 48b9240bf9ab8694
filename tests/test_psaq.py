"""CPU: the data-free calibration images (diff_vit_amd.psaq; the reference's --mode 2) against tests/golden/psaq_kat.npz, the outputs of
the REAL reference's functions (tools/gen_golden_psaq.py).  The fp64 restatement of the entropy (tests/_psaq_ref.py) against the
reference's fp64 run; the CPU twin of the operator against the restatement, bounded by the error of the reference's own fp32 run; the host-side
helpers; the structure of the gradient; the C symbols, the binding and the op; ``av_hook``; ``generate_data`` and ``harness --mode 2`` on the
micro models."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _psaq_ref as R
from conftest import ROOT, load_golden

STORED = ('ragged', 'tile', 'windows', 'minimum', 'correlated')


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def kat():
    g = load_golden('psaq_kat')
    out = {}
    for name in STORED:
        av, groups = torch.from_numpy(g[name + '/av']), int(g[name + '/groups'])
        v64, g64 = R.value_and_grad(av, groups)
        out[name] = dict(av=av, groups=groups, v64=v64, g64=g64, ref_v64=float(g[name + '/value64']), ref_g64=torch.from_numpy(g[name + '/grad64']),
                         ref_v32=float(g[name + '/value32']), ref_g32=torch.from_numpy(g[name + '/grad32']))
    return out


def _model_stats():
    from diff_vit_amd.data import MODEL_STATS
    return MODEL_STATS


def _micro_vit(dva):
    from test_profiling import _micro
    m = _micro(dva, dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(dva.synth.ARCHS['micro'], 0), strict=False)
    return m.eval()


def _micro_swin(dva):
    m = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10)
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 0))
    return m.eval()


def _yardstick(kat):
    """the error of the reference's own fp32 run against the fp64 truth, pooled as the maximum over the stored cases: (value, gradient)"""
    ref_v = max(R.value_error(k['ref_v32'], k['v64']) for k in kat.values())
    ref_g = max(e for e in (R.grad_error(k['ref_g32'], k['g64'], k['groups']) for k in kat.values()) if e is not None)
    return ref_v, ref_g


def test_restatement_matches_the_reference_in_fp64(kat):
    """value by the formula and autograd gradient == the reference's lines run in fp64.  Both are fp64 evaluations of one function in
    different operation orders: 1e-11 leaves three digits over the measured 1e-14."""
    skipped = 0
    for name, k in kat.items():
        assert R.value_error(k['v64'], k['ref_v64']) < 1e-11, name
        assert float(R.value_of(k['av'], k['groups'])) == pytest.approx(float(k['v64']), rel=1e-12)
        err = R.grad_error(k['g64'], k['ref_g64'], k['groups'])
        if err is None:
            skipped += 1                                     # two patches: the gradient is 1e-33, nothing to compare
            assert float((k['g64'] - k['ref_g64']).abs().max()) < 1e-20, name
        else:
            assert err < 1e-11, (name, err)
    assert skipped <= 1


def test_cpu_twin_against_the_restatement(dva, kat):
    """the twin of the op runs the reference's composition image by image: its error against the fp64 truth is held to 4 x the error of
    the reference's own fp32 run (pooled as the maximum over the cases), and an fp64 input brings it to the truth."""
    ref_v, ref_g = _yardstick(kat)
    print('reference fp32 composition: value error %.3g, gradient error %.3g' % (ref_v, ref_g))
    assert 1e-8 < ref_v < 1e-3 and 1e-8 < ref_g < 1e-3
    for name, k in kat.items():
        v, g = dva.psaq.patch_similarity_entropy_cpu(k['av'], k['groups'])
        assert v.dtype == torch.float64 and g.dtype == torch.float32 and g.shape == k['av'].shape
        ev, eg = R.value_error(v, k['v64']), R.grad_error(g, k['g64'], k['groups'])
        print('%-10s twin value error %.3g gradient error %s' % (name, ev, eg))
        assert ev <= 4 * ref_v, (name, ev)
        assert eg is None or eg <= 4 * ref_g, (name, eg)
        v, g = dva.psaq.patch_similarity_entropy_cpu(k['av'].double(), k['groups'])
        assert R.value_error(v, k['v64']) < 1e-5                  # the composition keeps the reference's fp32 constant c
        eg = R.grad_error(g, k['g64'], k['groups'])
        assert eg is None or eg < 1e-6, (name, eg)


def test_autograd_function_and_composition_agree(dva, kat):
    """patch_similarity_entropy (one call, stored gradient) and the whole-batch composition under autograd: the same value and
    gradient up to the fp32 yardstick, and backward scales the stored gradient"""
    k = kat['windows']
    a = k['av'].clone().requires_grad_(True)
    v = dva.patch_similarity_entropy(a, k['groups'])
    (-3.0 * v).backward()
    b = k['av'].clone().requires_grad_(True)
    w = dva.psaq.patch_similarity_entropy_torch(b, k['groups'])
    (-3.0 * w).backward()
    ref_v, ref_g = _yardstick(kat)
    assert R.value_error(v, k['v64']) <= 4 * ref_v and R.value_error(w, k['v64']) <= 4 * ref_v
    assert R.grad_error(a.grad / -3.0, k['g64'], k['groups']) <= 4 * ref_g
    assert R.grad_error(b.grad / -3.0, k['g64'], k['groups']) <= 4 * ref_g


def test_gradient_structure(dva, kat):
    """row 0 of every group carries no gradient and every head carries the same slice (the mean over heads)"""
    for name, k in kat.items():
        for g in (k['g64'], dva.psaq.patch_similarity_entropy_cpu(k['av'], k['groups'])[1]):
            assert bool((g[:, :, 0, :] == 0).all()), name
            assert all(torch.equal(g[:, 0], g[:, h]) for h in range(g.shape[1])), name


def test_degenerate_inputs_on_the_cpu(dva):
    """all similarities equal: value 0, zero gradient; a zero row: similarity 0 by the eps rule, finite results"""
    av = torch.zeros(2, 2, 5, 4)
    av[:, :, :, 0] = 2.0
    v, g = dva.psaq.patch_similarity_entropy_cpu(av, 1)
    assert float(v) == 0.0 and bool((g == 0).all())
    v64, g64 = R.value_and_grad(av, 1)
    assert float(v64) == 0.0 and bool((g64 == 0).all())
    av = torch.randn(1, 2, 6, 8, generator=torch.Generator().manual_seed(5))
    av[:, :, 3] = 0.0
    assert float(R.similarities(av, 1)[0, 0, 2].abs().max()) == 0.0
    for v, g in (dva.psaq.patch_similarity_entropy_cpu(av, 1), R.value_and_grad(av, 1)):
        assert bool(torch.isfinite(v)) and bool(torch.isfinite(g).all())


def test_host_side_helpers_against_the_reference(dva):
    g = load_golden('psaq_kat')
    P = dva.psaq
    assert np.array_equal(P.image_prior_loss(torch.from_numpy(g['tv/x'])).numpy(), g['tv/value'])
    mean, std, _ = _model_stats()['deit']                    # the statistics the reference's clip hard-codes
    x = torch.from_numpy(g['clip/x'].copy())
    out = P.clip_images(x, mean, std)
    assert out is x and np.array_equal(out.numpy(), g['clip/out'])
    for c in range(3):
        assert float(out[:, c].min()) >= -mean[c] / std[c] - 1e-6 and float(out[:, c].max()) <= (1 - mean[c]) / std[c] + 1e-6
    base, warm, epochs = g['lr/args']
    policy = P.lr_cosine_policy(float(base), int(warm), int(epochs))

    class Opt:
        param_groups = [{'lr': None}, {'lr': None}]
    got = []
    for it in range(int(epochs)):
        policy(Opt, it, it)
        assert Opt.param_groups[0]['lr'] == Opt.param_groups[1]['lr']
        got.append(Opt.param_groups[0]['lr'])
    assert np.allclose(np.array(got), g['lr/values'], rtol=1e-13, atol=0)


def test_symbols_declared_exported_and_bound(dva):
    src = open(os.path.join(ROOT, 'include', 'p2vit.h')).read()
    E = dva.engine
    L = E.lib()
    for name in ('p2v_psaq_workspace_bytes', 'p2v_patch_similarity_entropy'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert getattr(L, name).argtypes, name
    assert L.p2v_psaq_workspace_bytes.restype is C.c_size_t
    assert E.P2V_ABI_VERSION == L.p2v_abi_version()               # additive: no version change
    T = 196
    assert L.p2v_psaq_workspace_bytes(32, 1, 6, 197, 64) >= 32 * T * T * 4
    assert L.p2v_psaq_workspace_bytes(32, 1, 6, 197, 64) < 32 * T * T * 4 * 2     # S plus small change, not the O(10 n) tensors
    # the refusals need no GPU: shape code first, before any pointer is looked at
    for bad in ((0, 1, 1, 5, 4), (1, 0, 1, 5, 4), (1, 1, 0, 5, 4), (1, 1, 1, 2, 4), (1, 1, 1, 1026, 4), (1, 1, 1, 5, 6), (1, 1, 1, 5, 0),
                (1, 1, 1, 5, 132)):
        assert L.p2v_psaq_workspace_bytes(*bad) == 0, bad
        assert L.p2v_patch_similarity_entropy(None, *bad, None, None, None, None) == E.E_SHAPE, bad
        with pytest.raises(AssertionError):
            E.check(E.E_SHAPE)
    assert L.p2v_psaq_workspace_bytes(1, 1, 1, 3, 4) > 0 and L.p2v_psaq_workspace_bytes(1, 1, 1, 1025, 128) > 0
    assert L.p2v_patch_similarity_entropy(None, 1, 1, 1, 5, 4, None, None, None, None) == E.E_ARG


def test_op_registered_and_gpu_only(dva):
    assert 'patch_similarity_entropy' in dva.ops.OPS and hasattr(torch.ops.p2vit, 'patch_similarity_entropy')
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.patch_similarity_entropy(torch.zeros(1, 1, 5, 4), 1)
    assert 'generate_data' in dva.__all__ and dva.generate_data is dva.psaq.generate_data


def test_av_hook_default_changes_nothing(dva):
    """a plain attribute: no submodule, no state-dict key, and the float forward is the same with a hook that only looks"""
    for make, attn_of in ((_micro_vit, lambda m: [b.attn for b in m.blocks]), (_micro_swin, lambda m: [b.attn for l in m.layers for b in l.blocks])):
        m = make(dva)
        attns = attn_of(m)
        assert all(a.av_hook is None for a in attns)
        assert not any('av_hook' in n for n, _ in m.named_modules()) and not any('av_hook' in k for k in m.state_dict())
        names, keys = [n for n, _ in m.named_modules()], list(m.state_dict().keys())
        x = dva.synth.images(3, 2, m.arch['img_size'])
        with torch.no_grad():
            base = dva.psaq._logits(m, x)
            seen = []
            for a in attns:
                a.av_hook = seen.append
            hooked = dva.psaq._logits(m, x)
            for a in attns:
                a.av_hook = None
        assert torch.equal(base, hooked) and len(seen) == len(attns)
        assert all(t.dim() == 4 and t.shape[1] == a.num_heads for t, a in zip(seen, attns))
        assert names == [n for n, _ in m.named_modules()] and keys == list(m.state_dict().keys())


def _check_generated(dva, m, x, batch, family):
    mean, std, _ = _model_stats()[family]
    size = m.arch['img_size']
    assert x.shape == (batch, 3, size, size) and x.dtype == torch.float32 and not x.requires_grad
    assert x.device == next(m.parameters()).device and bool(torch.isfinite(x).all())
    for c in range(3):
        assert float(x[:, c].min()) >= -mean[c] / std[c] - 1e-6 and float(x[:, c].max()) <= (1 - mean[c]) / std[c] + 1e-6


def test_generate_data_on_the_micro_vit(dva):
    m = _micro_vit(dva)
    flags = [p.requires_grad for p in m.parameters()]
    x = dva.generate_data(m, 3, iterations=2, seed=11)
    _check_generated(dva, m, x, 3, 'deit')
    torch.manual_seed(11)
    noise = torch.randn(3, 3, 32, 32)                              # what the loop started from
    assert float((x - noise).abs().max()) > 0.1
    assert torch.equal(x, dva.generate_data(m, 3, iterations=2, seed=11))          # seeded: repeatable
    assert not torch.equal(x, dva.generate_data(m, 3, iterations=2, seed=12))
    assert flags == [p.requires_grad for p in m.parameters()] and all(b.attn.av_hook is None for b in m.blocks) and not m.training
    with pytest.raises(ValueError):
        dva.generate_data(m, 3, iterations=1, loss='nonsense')
    dva.harness.calibrate_model(m, x)
    with pytest.raises(ValueError, match='float model'):
        dva.generate_data(m, 3, iterations=1)
    m2 = _micro_vit(dva)
    m2.model_open_calibrate()
    with pytest.raises(ValueError, match='float model'):
        dva.generate_data(m2, 3, iterations=1)


def test_generate_data_consumes_random_in_the_reference_order(dva, monkeypatch):
    """batch pseudo labels, var_pred, then per step the jitter offset and the flip draw (generate_data.py:58-59, 83-86)"""
    import random
    calls = []
    for name in ('randint', 'uniform', 'random'):
        real = getattr(random, name)
        monkeypatch.setattr(dva.psaq.random, name, lambda *a, _n=name, _r=real: calls.append((_n,) + a) or _r(*a))
    dva.generate_data(_micro_vit(dva), 2, iterations=1, seed=1)
    assert calls == [('randint', 0, 9), ('randint', 0, 9), ('uniform', 2500, 3000), ('randint', -15, 15), ('random',), ('randint', -30, 30),
                     ('random',)]


def test_generate_data_on_the_micro_swin(dva):
    m = _micro_swin(dva)
    x = dva.generate_data(m, 2, iterations=1, seed=4)
    _check_generated(dva, m, x, 2, 'swin')
    _check_generated(dva, m, dva.generate_data(m, 2, iterations=1, seed=4, loss='torch'), 2, 'swin')
    assert all(b.attn.av_hook is None for l in m.layers for b in l.blocks)


def test_harness_mode_2_on_the_cpu(dva, monkeypatch, capsys):
    """--mode 2 generates and calibrates; the quantized validation behind it has no CPU path (FrozenPlan), so on the CPU the run ends
    there, with the calibrated model - the GPU test of the same name runs to the end"""
    made = []

    def factory(pretrained=False, cfg=None):
        from test_profiling import _micro
        made.append(_micro(dva, cfg))
        return made[-1]
    monkeypatch.setattr(dva.harness, 'str2model', lambda name: factory)
    argv = ['--model', 'micro', '--quant', '--psaq-iters', '1', '--device', 'cpu', '--calib-batchsize', '2', '--n-val', '4',
            '--val-batchsize', '4']
    with pytest.raises(RuntimeError, match='FrozenPlan needs a GPU'):
        dva.harness.main(argv + ['--mode', '2'])
    out = capsys.readouterr().out
    assert 'Generating data...' in out and 'Calibrating with generated data...' in out and 'Gaussian' not in out
    assert made[-1].quant and all(m.quant and not m.calibrate for m in made[-1]._q_modules())
    with pytest.raises(RuntimeError, match='FrozenPlan needs a GPU'):
        dva.harness.main(argv + ['--mode', '1'])
    out = capsys.readouterr().out
    assert 'Generating data...' not in out and 'Calibrating with Gaussian noise...' in out
    assert dva.harness.build_parser().parse_args([]).psaq_iters == 500
