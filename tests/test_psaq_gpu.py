"""GPU: the patch-similarity entropy operator (csrc/p2vit_psaq.hip) and the data generation on the engine.

Truth is the fp64 restatement (tests/_psaq_ref.py).  The yardstick is the error of the reference's own fp32 torch composition against it on
the same inputs, computed here on the CPU (never from the kernel), pooled as the maximum over the case list; the kernel gets 4 x that: its
rounding pattern (MFMA product order, the exponential, the fp32 similarity in its argument) is another draw from the same distribution,
while an indexing, transpose or trapezoid-weight mistake shows at 1e-2 or more.  Metrics: per image |g - g64|_2 / |g64|_2 and
|v - v64| / |v64|; a case whose |g64|_2 is below 1e-6 has no gradient metric (at most one: the two-patch case).

Measured on an MI355X (maximum over the cases): see DESIGN.md, "Data-free calibration images"."""
import ctypes as C

import numpy as np
import pytest
import torch

import _psaq_ref as R
from _arena import Arena, twice
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def truth(dva):
    """per case: input, fp64 value / gradient, and the errors of the reference's fp32 composition (the CPU twin runs its lines)"""
    out = []
    n_threads = torch.get_num_threads()
    torch.set_num_threads(min(n_threads, 16))
    try:
        for k, shape in enumerate(R.CASES):
            av = R.case_input(k)
            v64, g64 = R.value_and_grad(av, shape[1])
            v32, g32 = dva.psaq.patch_similarity_entropy_cpu(av, shape[1])
            out.append(dict(shape=shape, av=av, v64=v64, g64=g64, ref_v=R.value_error(v32, v64), ref_g=R.grad_error(g32, g64, shape[1])))
    finally:
        torch.set_num_threads(n_threads)
    return out


@pytest.fixture(scope='module')
def yardstick(truth):
    ref_v = max(t['ref_v'] for t in truth)
    graded = [t['ref_g'] for t in truth if t['ref_g'] is not None]
    assert len(graded) >= len(truth) - 1                           # at most one case without a gradient metric
    ref_g = max(graded)
    print('fp32 composition against fp64: value error %.3g, gradient error %.3g (maximum over %d cases)' % (ref_v, ref_g, len(truth)))
    assert 1e-8 < ref_v < 1e-3 and 1e-8 < ref_g < 1e-3             # a yardstick of fp32 size, not a free pass
    return ref_v, ref_g


def _run(dva, av, groups, sentinel):
    """one call of the C entry with every operand in a sentinel arena -> dict(value [1][1] fp64, grad like av)"""
    E = dva.engine
    L = E.lib()
    BG, H, N, hd = av.shape
    nbytes = L.p2v_psaq_workspace_bytes(BG // groups, groups, H, N, hd)
    assert nbytes > 0
    a = Arena(1, av.numel(), dtype=torch.float32, sentinel=sentinel, init=av.reshape(1, -1))
    ws = Arena(1, nbytes, dtype=torch.uint8, sentinel=sentinel, offset=0)
    val = Arena(1, 1, dtype=torch.float64, sentinel=sentinel)
    grad = Arena(1, av.numel(), dtype=torch.float32, sentinel=sentinel)
    E.check(L.p2v_patch_similarity_entropy(a.ptr, BG // groups, groups, H, N, hd, ws.ptr, val.ptr, grad.ptr, E.stream_ptr()))
    torch.cuda.synchronize()
    what = tuple(av.shape) + (groups,)
    assert np.array_equal(a.read(('av', what)).numpy().view(np.uint32).reshape(-1), av.numpy().view(np.uint32).reshape(-1))
    ws.read(('workspace', what))                                   # the guards around the workspace_bytes the query named
    return dict(value=val.read(('value_out', what)), grad=grad.read(('grad_out', what)).reshape(av.shape))


@pytest.mark.parametrize('k', range(len(R.CASES)), ids=['x'.join(map(str, s)) for s in R.CASES])
def test_operator_against_the_restatement(dva, truth, yardstick, k):
    """value and gradient in a sentinel arena: within 4 x the fp32 composition's pooled error of the fp64 truth, nothing written outside
    grad_out, value_out and the workspace, a second run byte-equal, row 0 exactly zero, the head slices byte-equal"""
    t = truth[k]
    groups = t['shape'][1]
    ref_v, ref_g = yardstick
    got = twice(lambda s: _run(dva, t['av'], groups, s))
    v, g = float(got['value'][0, 0]), got['grad']
    ev, eg = R.value_error(v, t['v64']), R.grad_error(g, t['g64'], groups)
    print('case %s: kernel value error %.3g (composition %.3g, bound %.3g), gradient error %s (composition %s, bound %.3g)'
          % (t['shape'], ev, t['ref_v'], 4 * ref_v, eg, t['ref_g'], 4 * ref_g))
    assert ev <= 4 * ref_v, (t['shape'], ev, ref_v)
    assert (eg is None) == (t['ref_g'] is None)
    if eg is not None:
        assert eg <= 4 * ref_g, (t['shape'], eg, ref_g)
    else:
        assert float((g.double() - t['g64']).abs().max()) < 1e-6 and bool(torch.isfinite(g).all())
    assert bool((g[:, :, 0, :].numpy().view(np.uint32) == 0).all()), 'row 0 must be +0.0'
    assert all(np.array_equal(g[:, 0].numpy().view(np.uint32), g[:, h].numpy().view(np.uint32)) for h in range(g.shape[1]))


def test_op_matches_the_c_entry(dva, truth):
    """torch.ops.p2vit.patch_similarity_entropy allocates its own workspace: the same bytes as the C call, input untouched"""
    t = truth[0]
    av = t['av'].cuda()
    keep = av.clone()
    value, grad = torch.ops.p2vit.patch_similarity_entropy(av, t['shape'][1])
    assert value.dtype == torch.float64 and value.dim() == 0 and grad.dtype == torch.float32 and grad.shape == av.shape and grad.is_cuda
    ref = _run(dva, t['av'], t['shape'][1], 0x5B)
    assert float(value) == float(ref['value'][0, 0]) and torch.equal(grad.cpu(), ref['grad']) and torch.equal(av, keep)
    with pytest.raises(AssertionError):
        torch.ops.p2vit.patch_similarity_entropy(av, 3)            # 2 groups are no multiple of 3
    with pytest.raises(AssertionError):
        torch.ops.p2vit.patch_similarity_entropy(av[:, :, :2], 1)  # one patch row


def test_degenerate_inputs(dva):
    """lo == hi: value 0 and a zero gradient; a zero row: similarity 0 by the eps rule, finite value and gradient near the truth"""
    av = torch.zeros(2, 2, 5, 4)
    av[:, :, :, 0] = 2.0                                           # every normalised row is (1, 0, 0, 0) exactly: S == 1
    got = twice(lambda s: _run(dva, av, 1, s))
    assert float(got['value'][0, 0]) == 0.0 and bool((got['grad'] == 0).all())
    av = torch.randn(1, 2, 6, 8, generator=torch.Generator().manual_seed(5))
    av[:, :, 3] = 0.0
    got = twice(lambda s: _run(dva, av, 1, s))
    v64, g64 = R.value_and_grad(av, 1)
    v32, g32 = dva.psaq.patch_similarity_entropy_cpu(av, 1)
    assert bool(torch.isfinite(got['value']).all()) and bool(torch.isfinite(got['grad']).all())
    assert R.value_error(got['value'][0, 0], v64) <= 4 * max(R.value_error(v32, v64), 2.0 ** -23)
    # the zero row's own gradient is g / eps - 1e8 times the others -, so the norm of the whole image measures that row
    assert R.grad_error(got['grad'], g64, 1) <= 4 * max(R.grad_error(g32, g64, 1), 2.0 ** -23)


def test_refusals_before_any_launch(dva):
    """every refusal by its code; the output arenas keep their sentinel (nothing was launched)"""
    E = dva.engine
    L = E.lib()
    av = Arena(1, 2 * 5 * 8, dtype=torch.float32, init=torch.ones(1, 80))
    ws = Arena(1, 1 << 16, dtype=torch.uint8, offset=0)
    val = Arena(1, 1, dtype=torch.float64)
    grad = Arena(1, 80, dtype=torch.float32)
    st = E.stream_ptr()

    def call(av_p=av.ptr, B=1, G=1, H=2, N=5, hd=8, ws_p=ws.ptr, val_p=val.ptr, grad_p=grad.ptr):
        return L.p2v_patch_similarity_entropy(av_p, B, G, H, N, hd, ws_p, val_p, grad_p, st)
    for kw in (dict(B=0), dict(G=0), dict(H=0), dict(N=2), dict(N=1026), dict(hd=6), dict(hd=0), dict(hd=132), dict(B=-1)):
        assert call(**kw) == E.E_SHAPE, kw
        with pytest.raises(AssertionError):
            E.check(call(**kw))
    off = lambda p, n: C.c_void_p(p.value + n)
    for kw in (dict(av_p=None), dict(ws_p=None), dict(val_p=None), dict(grad_p=None), dict(av_p=off(av.ptr, 4)), dict(grad_p=off(grad.ptr, 8)),
               dict(val_p=off(val.ptr, 4)), dict(ws_p=off(ws.ptr, 16))):
        assert call(**kw) == E.E_ARG, kw
        with pytest.raises(E.P2VError):
            E.check(call(**kw))
    torch.cuda.synchronize()
    for a in (ws, val, grad):
        assert bool((a.dev.cpu() == a.sentinel).all())
    assert call() == 0                                             # and the accepted call runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(val.read('value')).all())


def _micro_vit(dva, dtype=torch.float32):
    from test_profiling import _micro
    m = _micro(dva, dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(dva.synth.ARCHS['micro'], 0), strict=False)
    return m.eval().to(dtype)


def _entropy_image_gradient(dva, m, x, entropy):
    """d(sum over blocks of entropy(attn @ v)) / d(images) through the float module graph"""
    x = x.clone().requires_grad_(True)
    seen = []
    for b in m.blocks:
        b.attn.av_hook = seen.append
    try:
        dva.psaq._logits(m, x)
        total = sum(entropy(av) for av in seen)
        g, = torch.autograd.grad(total, x)
    finally:
        for b in m.blocks:
            b.attn.av_hook = None
    return total.detach(), g


def test_autograd_function_inside_a_graph(dva):
    """d(entropy) / d(images) through the float micro ViT: the operator on the GPU against the micro model in fp64 on the CPU; the
    yardstick is the fp32 composition through the same model on the CPU, pooled as the maximum over four input batches like the case
    list of the operator test, the bound 4 x that"""
    m64, m32, mgpu = _micro_vit(dva, torch.float64), _micro_vit(dva), _micro_vit(dva).cuda()
    rows = []
    for seed in (5, 6, 7, 8):
        x = dva.synth.images(seed, 3, 32)
        v64, g64 = _entropy_image_gradient(dva, m64, x.double(), lambda av: R.value_of(av, 1))
        v32, g32 = _entropy_image_gradient(dva, m32, x, lambda av: dva.psaq.patch_similarity_entropy_torch(av, 1))
        v, g = _entropy_image_gradient(dva, mgpu, x.cuda(), lambda av: dva.patch_similarity_entropy(av, 1))
        rows.append((R.value_error(v32, v64), R.grad_error(g32, g64, 1), R.value_error(v.cpu(), v64), R.grad_error(g.cpu(), g64, 1)))
        print('graph, batch %d: kernel value error %.3g (composition %.3g), gradient error %.3g (composition %.3g)'
              % (seed, rows[-1][2], rows[-1][0], rows[-1][3], rows[-1][1]))
    ref_v, ref_g = max(r[0] for r in rows), max(r[1] for r in rows)
    assert 1e-9 < ref_v < 1e-3 and 1e-9 < ref_g < 1e-3
    for r in rows:
        assert r[2] <= 4 * ref_v and r[3] <= 4 * ref_g, (r, ref_v, ref_g)


def _check_generated(dva, m, x, batch, family):
    from diff_vit_amd.data import MODEL_STATS
    mean, std, _ = MODEL_STATS[family]
    size = m.arch['img_size']
    assert x.shape == (batch, 3, size, size) and x.dtype == torch.float32 and not x.requires_grad
    assert x.is_cuda and bool(torch.isfinite(x).all())
    for c in range(3):
        assert float(x[:, c].min()) >= -mean[c] / std[c] - 1e-6 and float(x[:, c].max()) <= (1 - mean[c]) / std[c] + 1e-6


def test_generate_data_on_the_engine(dva, monkeypatch):
    """generate_data(loss='engine') on the micro ViT and the micro Swin (49-token windows, 4 and 1 per image): the mechanical
    properties of the CPU test, and every block's term went through the op"""
    calls = []
    real = torch.ops.p2vit.patch_similarity_entropy
    for make, family, blocks in ((_micro_vit, 'deit', 2), (None, 'swin', 4)):
        if make is None:
            m = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10)
            m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 0))
            m = m.eval()
        else:
            m = make(dva)
        m = m.cuda()
        del calls[:]
        monkeypatch.setattr(dva.psaq, '_PatchSimilarityEntropy', _counting(dva.psaq._PatchSimilarityEntropy, calls))
        x = dva.generate_data(m, 3, iterations=2, seed=11)
        monkeypatch.undo()
        _check_generated(dva, m, x, 3, family)
        assert len(calls) == 2 * 2 * blocks and all(c == 'cuda' for c in calls)
        torch.manual_seed(11)
        noise = torch.randn(3, 3, m.arch['img_size'], m.arch['img_size'])
        assert float((x.cpu() - noise).abs().max()) > 0.1
        assert torch.equal(x, dva.generate_data(m, 3, iterations=2, seed=11))          # deterministic kernels: repeatable
        dva.harness.calibrate_model(m, x)
        with pytest.raises(ValueError, match='float model'):
            dva.generate_data(m, 3, iterations=1)
    assert real is torch.ops.p2vit.patch_similarity_entropy


def _counting(fn, calls):
    class Counting:
        @staticmethod
        def apply(av, groups):
            calls.append(av.device.type)
            return fn.apply(av, groups)
    return Counting


def test_harness_mode_2(dva, monkeypatch, capsys):
    """harness --quant --mode 2 --psaq-iters 1 on the micro ViT: generates, calibrates on the generated images, validates on the engine"""
    from test_profiling import _micro
    monkeypatch.setattr(dva.harness, 'str2model', lambda name: (lambda pretrained=False, cfg=None: _micro(dva, cfg)))
    loss, top1, top5 = dva.harness.main(['--model', 'micro', '--quant', '--mode', '2', '--psaq-iters', '1', '--calib-batchsize', '4', '--n-val', '8',
                                         '--val-batchsize', '8'])
    out = capsys.readouterr().out
    assert 'Generating data...' in out and 'Calibrating with generated data...' in out and 'Gaussian' not in out
    assert np.isfinite(loss) and 0.0 <= top1 <= 100.0 and 0.0 <= top5 <= 100.0
