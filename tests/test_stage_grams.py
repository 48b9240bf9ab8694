"""CPU: CKA over the DDV stage list (diff_vit_amd.cka.get_stage_grams / compute_cka(stages=)) - the int64 restatement of the stage Grams
(tests/_stage_grams_ref.py) against cka.gram_matrix, the hook path on the micro-ViT, the unchanged default path, the refusals, and the
argument checks of the new C entry points (made before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _stage_grams_ref as G
from conftest import ROOT, load_golden
from test_cka import _micro_float, _run_kat


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.mark.parametrize('n,rows,cols', [(4, 1, 1), (5, 3, 17), (33, 5, 48), (50, 17, 64)])
def test_restatement_against_gram_matrix(dva, n, rows, cols):
    """centre(integer Gram) * unit^2 against cka.gram_matrix on the dequantised fp32 values: 1e-5 of the largest entry (fp32 products and
    sums on one side, exact integers on the other)"""
    g = torch.Generator().manual_seed(n * 1000 + cols)
    codes = torch.randint(-128, 128, (n, rows, cols), generator=g, dtype=torch.int64).to(torch.int8)
    m = torch.randint(0, 4, (cols,), generator=g).to(torch.uint8)
    for shift, unit in ((None, 0.0625), (m, 0.0123)):
        scale = None if shift is None else torch.exp2(shift.double()) * unit
        if scale is not None and int(m.min()) == 0:
            assert torch.equal(G.shifts_of(scale)[0], m) and G.shifts_of(scale)[1] == unit
        raw = G.int_gram(codes, shift).double() * unit * unit
        want = G.centre(raw)
        got = dva.cka.gram_matrix(G.dequantised(codes, shift, unit)).reshape(n, n).double()
        tol = 1e-5 * max(float(want.abs().max()), float(raw.abs().max()))
        assert float((got - want).abs().max()) <= tol, (n, rows, cols, shift is None)
    # the strided walk: a stage inside a larger buffer, samples 5 rows apart, rows padded
    rs, ss = cols + 7, 5 * (cols + 7)
    buf = torch.full((n * ss + 64,), 91, dtype=torch.int8)
    v = torch.randint(-128, 128, (n, min(rows, 5), cols), generator=g, dtype=torch.int64).to(torch.int8)
    idx = G.strided(torch.arange(buf.numel()), n, v.shape[1], cols, ss, rs, 3)
    buf[idx.reshape(-1)] = v.reshape(-1)
    assert torch.equal(G.strided(buf, n, v.shape[1], cols, ss, rs, 3), v)
    assert torch.equal(G.int_gram(G.strided(buf, n, v.shape[1], cols, ss, rs, 3), m), G.int_gram(v, m))
    x = torch.randn(n, rows * cols, generator=g)
    gram, bound = G.f64_gram(x)
    assert torch.equal(gram, gram.t()) and bound >= float(gram.abs().max())


def test_shifts_of_refuses_other_ratios():
    assert G.shifts_of(torch.tensor([0.5, 1.0, 4.0, 2.0]))[0].tolist() == [0, 1, 3, 2]
    assert G.shifts_of(torch.tensor([0.3, 0.3]))[0].tolist() == [0, 0] and G.shifts_of(torch.tensor([0.3, 0.3]))[1] == float(torch.tensor(0.3).double())
    for bad in ([1.0, 3.0], [1.0, 16.0]):
        with pytest.raises(AssertionError):
            G.shifts_of(torch.tensor(bad))


@pytest.fixture(scope='module')
def micro_pair(dva, synth):
    fp, g = _micro_float(dva, synth)
    q, _ = _micro_float(dva, synth)
    dva.harness.calibrate_model(q, torch.from_numpy(g['x_cal']))
    return fp, q, torch.from_numpy(g['x_ev'])


@pytest.mark.parametrize('stages', ['engine', 'full'])
@pytest.mark.parametrize('with_linear', [False, True])
def test_get_stage_grams_hook_path(dva, micro_pair, stages, with_linear):
    """a CPU model has no engine: forward hooks on the stage names, the Grams of cka._grams; names are ddv.stage_names"""
    fp, q, x = micro_pair
    names = dva.ddv.stage_names(2, with_linear, stages == 'full')
    for model, bits in ((fp, None), (q, [8] * 10)):
        got_names, g = dva.cka.get_stage_grams(x, model, bits, 'cpu', stages=stages, with_linear=with_linear)
        assert got_names == names and g.shape == (len(names), x.shape[0], x.shape[0]) and g.dtype == torch.float32
        # (the reference's formula subtracts the column mean, then the row mean: symmetric up to the fp32 rounding of the two orders)
        assert bool(torch.isfinite(g).all()) and float((g - g.transpose(1, 2)).abs().max()) <= 1e-5 * float(g.abs().max())
        assert float(g.diagonal(dim1=1, dim2=2).abs().max()) == 0
    # the hooked outputs themselves: one stage against gram_matrix on the output of a hook of our own
    seen = {}
    h = dict(q.named_modules())['blocks.1.qact2'].register_forward_hook(lambda m, i, o: seen.setdefault('v', o.detach()))
    try:
        _, g = dva.cka.get_stage_grams(x, q, [8] * 10, 'cpu', stages=stages, with_linear=with_linear)
    finally:
        h.remove()
    assert torch.equal(g[names.index('blocks.1.qact2')].reshape(-1), dva.cka.gram_matrix(seen['v']))


def test_compute_cka_stages_on_cpu_and_default_path_unchanged(dva, micro_pair, synth):
    fp, q, x = micro_pair
    hm = dva.compute_cka(fp, q, [x], None, [8] * 10, stages='engine')
    S = len(dva.ddv.stage_names(2, False, False))
    assert hm.shape == (S, S) and bool(torch.isfinite(hm).all())
    # by hand from get_stage_grams + update_state_across_models_grams
    _, g1 = dva.cka.get_stage_grams(x, fp, None, 'cpu')
    _, g2 = dva.cka.get_stage_grams(x, q, [8] * 10, 'cpu')
    c = dva.MinibatchCKA(S, S, across_models=True)
    c.update_state_across_models_grams(g1, g2)
    assert torch.equal(c.result(), hm)
    # a model against itself: update_state_grams gives ones on the diagonal, as update_state does
    c = dva.MinibatchCKA(S)
    c.update_state_grams(g2)
    assert float((c.result().diagonal() - 1).abs().max()) <= 1e-5
    a = dva.MinibatchAdvCKA(S, S)
    a.update_state_grams(g1, g2)
    assert torch.allclose(a.result(), hm, atol=1e-6)
    # stages=None is the code path of before: the known-answer flow of tests/golden/cka_kat.npz, and the same tensor with and without the argument
    g = load_golden('cka_kat')
    for n in [int(v) for v in g['ns']]:
        for kind, t in zip(('internal', 'across', 'adv'), _run_kat(dva.cka, g, n, synth)):
            assert np.abs(t.numpy() - g['%s/n%d' % (kind, n)]).max() <= 1e-6
    assert torch.equal(dva.compute_cka(fp, fp, [x], None, None), dva.compute_cka(fp, fp, [x], None, None, stages=None, with_linear=False))


def test_refusals(dva, micro_pair):
    fp, q, x = micro_pair
    from diff_vit_amd import swin
    s = swin.swin_micro_patch4_window7_56(num_classes=10).eval()
    with pytest.raises(NotImplementedError, match='Swin'):
        dva.compute_cka(s, s, [torch.zeros(4, 3, 56, 56)], None, None, stages='engine')
    with pytest.raises(NotImplementedError, match='Swin'):
        dva.cka.get_stage_grams(torch.zeros(4, 3, 56, 56), s, None, 'cpu')
    with pytest.raises(NotImplementedError, match='attention'):
        dva.cka.get_stage_grams(x, q, [8] * 10, 'cpu', attention=True)
    with pytest.raises(NotImplementedError, match='attention'):
        dva.compute_cka(fp, q, [x], None, [8] * 10, stages='attention')
    with pytest.raises(ValueError):
        dva.compute_cka(fp, q, [x], None, [8] * 10, stages='linear')
    with pytest.raises(NotImplementedError):
        dva.compute_cka(fp, q, [x], None, [8] * 10, normalize_act=True, stages='engine')
    with pytest.raises(NotImplementedError):
        dva.cka.main(['--model', 'swin_tiny', '--stages', 'engine', '--device', 'cpu'])


def test_ops_have_no_cpu_kernel(dva):
    assert 'code_grams' in dva.ops.OPS and 'cka_centre' in dva.ops.OPS
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.code_grams([torch.zeros(4, 2, 16, dtype=torch.int8)], [None])
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.cka_centre(torch.zeros(1, 4, 4, dtype=torch.float64))


def test_entry_points_declared_exported_and_refusing_without_gpu(dva):
    E = dva.engine
    L = E.lib()
    src = open(os.path.join(ROOT, 'include', 'p2vit.h')).read()
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in ('p2v_code_grams', 'p2v_code_grams_workspace_bytes', 'p2v_cka_centre', 'p2v_plan_prepare_grams', 'p2v_forward_grams',
                 'p2v_forward_grams_stage_count', 'p2v_forward_grams_bytes', 'p2v_forward_grams_layout'):
        assert (name + '(') in src and hasattr(lib, name), name
    assert E.P2V_ABI_VERSION == 6 == L.p2v_abi_version()
    assert ('#define P2V_GRAM_CHUNK %d' % E.GRAM_CHUNK) in src and ('#define P2V_GRAM_MAX_N %d' % E.GRAM_MAX_N) in src
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 255) // 256 * 256            # 256-byte aligned, never dereferenced

    def layer(**kw):
        d = E.GramLayer()
        d.base, d.shift, d.sample_stride, d.row_stride, d.rows, d.cols, d.dtype = p, None, 64, 16, 4, 16, E.GRAM_I8
        for k, v in kw.items():
            setattr(d, k, v)
        return (E.GramLayer * 1)(d)

    def rc(lay, n=8, grams=p, ws=p, ws_bytes=1 << 40, n_layers=1):
        return L.p2v_code_grams(lay, n_layers, n, grams, ws, ws_bytes, None)
    T = 1                                                                    # tiles of n = 8
    assert L.p2v_code_grams_workspace_bytes(layer(), 1, 8) == T * 1 * 1024 * 8
    assert L.p2v_code_grams_workspace_bytes(layer(rows=1, cols=E.GRAM_CHUNK + 16, row_stride=E.GRAM_CHUNK + 16), 1, 33) == 3 * 2 * 8192
    assert L.p2v_code_grams_workspace_bytes(layer(), 1, 0) == 0 and L.p2v_code_grams_workspace_bytes(layer(), 1, 513) == 0
    assert L.p2v_code_grams_workspace_bytes(layer(), 1, 512) > 0 and L.p2v_code_grams_workspace_bytes(layer(), 1, 1) > 0
    for want, got in ((E.E_ARG, rc(None)), (E.E_ARG, rc(layer(), n_layers=0)), (E.E_ARG, rc(layer(), grams=None)), (E.E_ARG, rc(layer(), ws=None)),
                      (E.E_ARG, rc(layer(), ws=p + 16)), (E.E_ARG, rc(layer(), grams=p + 4)),
                      (E.E_SHAPE, rc(layer(), n=0)), (E.E_SHAPE, rc(layer(), n=513)), (E.E_ARG, rc(layer(base=None))),
                      (E.E_ARG, rc(layer(dtype=2))), (E.E_SHAPE, rc(layer(rows=0))), (E.E_SHAPE, rc(layer(cols=0))),
                      (E.E_ARG, rc(layer(row_stride=15))), (E.E_ARG, rc(layer(sample_stride=-1))), (E.E_ARG, rc(layer(base=p + 8))),
                      (E.E_ARG, rc(layer(shift=p + 8))), (E.E_ARG, rc(layer(shift=p, dtype=E.GRAM_F32))),
                      (E.E_UNSUPPORTED, rc(layer(rows=1 << 16, cols=1 << 15, row_stride=1 << 15))),
                      (E.E_UNSUPPORTED, rc(layer(dtype=E.GRAM_F32, row_stride=20))),
                      (E.E_WORKSPACE, rc(layer(), ws_bytes=8191))):
        assert got == want, (got, want, L.p2v_last_error())
    # p2v_cka_centre
    cen = lambda raw=p, pitch=8, stride=64, layers=1, n=8, out=p: L.p2v_cka_centre(raw, pitch, stride, layers, n, out, None)
    for want, got in ((E.E_ARG, cen(raw=None)), (E.E_ARG, cen(out=None)), (E.E_ARG, cen(layers=0)), (E.E_SHAPE, cen(n=3)), (E.E_SHAPE, cen(n=513)),
                      (E.E_ARG, cen(pitch=7)), (E.E_ARG, cen(stride=-1)), (E.E_ARG, cen(raw=p + 4))):
        assert got == want, (got, want, L.p2v_last_error())
    # the whole-model entry points: null plan
    assert L.p2v_plan_prepare_grams(None) == E.E_ARG
    assert L.p2v_forward_grams_stage_count(None, 0, 0) == E.E_ARG and L.p2v_forward_grams_bytes(None, 4, 0, 0) == 0
    assert L.p2v_forward_grams_layout(None, 0, 0, 0, None, None, None, None) == E.E_ARG
    assert L.p2v_forward_grams(None, None, 4, None, 0, None, p, 0, 0, 0, None, 0, p, 0, p, 0, None) == E.E_ARG
