"""GPU: the DDV model diff on the MI355X - the pair-cosine kernels against numpy, p2v_forward_ddv against the oracle's integer taps and
the linear-layer taps, the fused model's DDV against the REAL reference's (tests/golden/ddv_micro.npz), the float model's module-graph
path, refusals and the command line.  Adds 25 s to the GPU suite (16.5 s of it the command-line test with its 50 PGD steps)."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import golden_calib, load_golden
from test_ddv import micro_model, shared_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def _up(v, m):
    return (v + m - 1) // m * m


def _strided(n, rows, cols, dtype, gen, wide):
    """[n, rows, cols] view: rows padded by `wide` 16-byte groups, samples by one more row (strides larger than the shape)"""
    vec = 16 if dtype == torch.int8 else 4
    rs = _up(cols, vec) + (vec if wide else 0)
    if dtype == torch.int8:
        buf = torch.randint(-128, 128, (n, rows + (1 if wide else 0), rs), dtype=torch.int8, device='cuda', generator=gen)
    else:
        buf = torch.randn(n, rows + (1 if wide else 0), rs, device='cuda', generator=gen)
    return buf[:, :rows, :cols]


def _call(dva, a, b, scales):
    """p2v_pair_cosine through ctypes on [n, rows, cols] views, strides as they are"""
    E = dva.engine
    L = E.lib()
    n = a[0].shape[0]
    descs = (E.CosLayer * len(a))()
    for d, x, y, sc in zip(descs, a, b, scales):
        assert x.stride() == y.stride() and x.stride(2) == 1
        d.a, d.b, d.scale = x.data_ptr(), y.data_ptr(), None if sc is None else sc.data_ptr()
        d.sample_stride, d.row_stride, d.rows, d.cols = x.stride(0), x.stride(1), x.shape[1], x.shape[2]
        d.dtype = E.COS_I8 if x.dtype == torch.int8 else E.COS_F32
    nbytes = L.p2v_pair_cosine_workspace_bytes(descs, len(a), n)
    assert nbytes > 0, L.p2v_last_error()
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    out = torch.empty(len(a), n, 3, dtype=torch.float64, device='cuda')
    rc = L.p2v_pair_cosine(descs, len(a), n, E.ptr(out), E.ptr(ws), nbytes, E.stream_ptr())
    assert rc == 0, L.p2v_last_error()
    return out


def _int_sums(x, y, per_channel=False):
    """int64 sums of integer codes [n, rows, cols] on the host: [n, 3], or [n, cols, 3] per channel"""
    x, y = x.cpu().to(torch.int32), y.cpu().to(torch.int32)                     # products <= 2^14: exact in int32, summed in int64
    pc = torch.stack([(x * y).sum(1, dtype=torch.int64), (x * x).sum(1, dtype=torch.int64), (y * y).sum(1, dtype=torch.int64)], -1)
    return (pc if per_channel else pc.sum(1)).numpy()


SHAPES = [(r, c) for r in (1, 17, 197, 577) for c in (16, 48, 384, 1536, 1000)]


@pytest.mark.parametrize('n', [1, 3, 50])
def test_pair_cosine_against_numpy(dva, n):
    gen = torch.Generator(device='cuda').manual_seed(100 + n)
    # ---- int8 codes, one scale per tensor: the exact integer sums
    a = [_strided(n, r, c, torch.int8, gen, (k % 2) == 0) for k, (r, c) in enumerate(SHAPES)]
    b = [_strided(n, r, c, torch.int8, gen, (k % 2) == 0) for k, (r, c) in enumerate(SHAPES)]
    got = _call(dva, a, b, [None] * len(a))
    assert torch.equal(got, _call(dva, a, b, [None] * len(a)))                   # bitwise repeatable
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(got[k].cpu().numpy(), _int_sums(x, y).astype(np.float64)), (n, SHAPES[k])
    # ---- int8 codes with per-channel scales: C <= 4096 terms -> 2 C 2^-53 < 1e-12
    scales = [(torch.rand(c, device='cuda', generator=gen) + 0.05) * 2.0 ** ((k % 7) - 5) for k, (r, c) in enumerate(SHAPES)]
    got = _call(dva, a, b, scales)
    assert torch.equal(got, _call(dva, a, b, scales))
    for k, (x, y) in enumerate(zip(a, b)):
        s2 = scales[k].cpu().double().numpy() ** 2
        want = (_int_sums(x, y, True).astype(np.float64) * s2[None, :, None]).sum(1)                     # [n, 3]
        g = got[k].cpu().numpy()
        root = np.sqrt(want[:, 1] * want[:, 2])
        assert np.all(np.abs(g[:, 1] - want[:, 1]) <= 1e-12 * want[:, 1]), (n, SHAPES[k])
        assert np.all(np.abs(g[:, 2] - want[:, 2]) <= 1e-12 * want[:, 2]), (n, SHAPES[k])
        assert np.all(np.abs(g[:, 0] - want[:, 0]) <= 1e-12 * root), (n, SHAPES[k])
    same = dva.ddv.cosines(_call(dva, a, a, scales))
    assert float((same - 1).abs().max()) <= 1e-15
    same = dva.ddv.cosines(_call(dva, b, b, [None] * len(b)))
    assert float((same - 1).abs().max()) <= 1e-15
    del a, b
    # ---- fp32 values
    a = [_strided(n, r, c, torch.float32, gen, (k % 2) == 1) for k, (r, c) in enumerate(SHAPES)]
    b = [x * 0.5 + _strided(n, r, c, torch.float32, gen, (k % 2) == 1) for k, ((r, c), x) in enumerate(zip(SHAPES, a))]
    b = [y if y.stride() == x.stride() else torch.empty_strided(x.shape, x.stride(), device='cuda').copy_(y) for x, y in zip(a, b)]
    got = _call(dva, a, b, [None] * len(a))
    assert torch.equal(got, _call(dva, a, b, [None] * len(a)))
    for k, (x, y) in enumerate(zip(a, b)):
        xd, yd = x.double().reshape(n, -1), y.double().reshape(n, -1)
        want = torch.stack([(xd * yd).sum(1), (xd * xd).sum(1), (yd * yd).sum(1)], 1)
        root = torch.sqrt(want[:, 1] * want[:, 2]).unsqueeze(1)
        assert bool(((got[k] - want).abs() <= 1e-9 * root).all()), (n, SHAPES[k])
    same = dva.ddv.cosines(_call(dva, a, a, [None] * len(a)))
    assert float((same - 1).abs().max()) <= 1e-15


def test_pair_cosine_op_and_refusals(dva):
    E = dva.engine
    L = E.lib()
    gen = torch.Generator(device='cuda').manual_seed(7)
    # the custom op: any layout, ragged feature counts (zero padding), int8 with scales of the last dimension, floats
    a = [torch.randn(6, 3, 14, 14, device='cuda', generator=gen), torch.randn(6, 10, device='cuda', generator=gen),
         torch.randint(-128, 128, (6, 5, 20), dtype=torch.int8, device='cuda', generator=gen),
         torch.randint(-128, 128, (6, 5, 20), dtype=torch.int8, device='cuda', generator=gen),
         torch.randn(6, 197, 384, device='cuda', generator=gen).transpose(1, 2)]
    b = [torch.randn_like(a[0]), torch.randn_like(a[1]), a[3], a[2], torch.randn(6, 384, 197, device='cuda', generator=gen)]
    sc = [None, None, None, torch.rand(20, device='cuda', generator=gen) + 0.1, None]
    got = torch.ops.p2vit.pair_cosine(a, b, sc).cpu()
    want = dva.ddv.pair_cosine_cpu([t.cpu() for t in a], [t.cpu() for t in b], [None if s is None else s.cpu() for s in sc])
    assert torch.equal(got[2], want[2])
    root = torch.sqrt(want[..., 1] * want[..., 2]).unsqueeze(-1)
    assert bool(((got - want).abs() <= 1e-9 * root).all())
    # an all-zero sample: 0/0 = NaN, as numpy gives in the reference
    z = torch.zeros(2, 4, 16, dtype=torch.int8, device='cuda')
    assert torch.isnan(dva.ddv.cosines(torch.ops.p2vit.pair_cosine([z], [z], [None]))).all()
    # misaligned pointers and strides
    buf = torch.zeros(4096, dtype=torch.int8, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    out = torch.empty(3, 3, dtype=torch.float64, device='cuda')
    base = buf.data_ptr()
    assert base % 16 == 0
    ok = dict(a=base, b=base + 1024, sample_stride=64, row_stride=16)
    for field, bad in ((None, None), ('a', base + 4), ('b', base + 1032), ('row_stride', 20), ('sample_stride', 72)):
        kw = dict(ok)
        if field:
            kw[field] = bad
        d = E.CosLayer(kw['a'], kw['b'], None, kw['sample_stride'], kw['row_stride'], 4, 16, E.COS_I8)
        rc = L.p2v_pair_cosine((E.CosLayer * 1)(d), 1, 3, E.ptr(out), E.ptr(ws), ws.numel(), E.stream_ptr())
        assert rc == (E.E_ARG if field else 0), (field, rc)
    torch.cuda.synchronize()


def _stage_sums(a, b, scale=None):
    """numpy sums of one stage from integer codes [2n, ...] split into halves; per-channel scales as fp64 s^2 on per-channel sums"""
    n = a.shape[0]
    if scale is None or scale.numel() == 1:
        return _int_sums(a.reshape(n, 1, -1), b.reshape(n, 1, -1)).astype(np.float64)
    C = a.shape[-1]
    s2 = scale.double().numpy().reshape(-1) ** 2
    return (_int_sums(a.reshape(n, -1, C), b.reshape(n, -1, C), True).astype(np.float64) * s2[None, :, None]).sum(1)


def _check_forward_ddv(dva, O, plan, arch, W, c, x, bits):
    n = x.shape[0] // 2
    xc = x.cuda()
    logits, names, sums = plan.forward_ddv(xc, bits, with_linear=False)
    assert torch.equal(logits, plan.forward(xc, bits))
    assert names == dva.ddv.stage_names(arch['depth'], False) and sums.shape == (5 * arch['depth'] + 3, n, 3)
    logits2, names2, sums2 = plan.forward_ddv(xc, bits, with_linear=True)
    assert torch.equal(logits2, logits) and names2 == dva.ddv.stage_names(arch['depth'], True)
    assert sums2.shape == (9 * arch['depth'] + 4, n, 3)
    # the ONE fp32 buffer: the largest single tap of 2n images, not all of them
    T, D, Hd = plan.tokens, plan.D, plan.hidden
    one = 2 * n * T * max(3 * D, Hd) * 4
    assert plan.ddv_tap_bytes(n) == one == dva.engine.lib().p2v_ddv_tap_scratch_bytes(plan._handle, n)
    assert one < sum(int(np.prod(s)) for s in plan.tap_shapes(2 * n)) * 4 / arch['depth']
    by2 = dict(zip(names2, sums2.cpu().numpy()))
    for k, nm in enumerate(names):                                               # with_linear does not touch the int8 stages' bits
        assert np.array_equal(sums[k].cpu().numpy(), by2[nm]), nm
    assert torch.equal(sums2, plan.forward_ddv(xc, bits, with_linear=True)[2])   # bitwise repeatable
    # int8 stages against the ORACLE's integer taps of the same names
    orc = O.OracleViT(arch, W)
    orc.calib = c
    taps = {}
    ref_logits = orc.quant_forward(x, bits, taps)
    assert torch.equal(logits.cpu(), ref_logits)
    per_channel = {'qact1': c['qact1']}
    for i in range(arch['depth']):
        per_channel['blocks.%d.qact2' % i] = c['blocks.%d.qact2' % i]
        per_channel['blocks.%d.qact4' % i] = c['blocks.%d.qact4' % i]
    for nm in names[:-1]:
        t = taps[nm]
        sc = per_channel.get(nm)
        sc = None if sc is None else sc.detach().float().reshape(-1)
        want = _stage_sums(t[:n], t[n:], sc)
        got = by2[nm]
        if sc is None or sc.numel() == 1:
            if sc is not None:
                want = want * float(sc.double() ** 2)
                assert np.all(np.abs(got - want) <= 1e-12 * np.sqrt(want[:, 1:2] * want[:, 2:3])), (bits[:3], nm)
            else:
                assert np.array_equal(got, want), (bits[:3], nm)
        else:
            root = np.sqrt(want[:, 1] * want[:, 2])
            assert np.all(np.abs(got[:, 1] - want[:, 1]) <= 1e-12 * want[:, 1]), (bits[:3], nm)
            assert np.all(np.abs(got[:, 2] - want[:, 2]) <= 1e-12 * want[:, 2]), (bits[:3], nm)
            assert np.all(np.abs(got[:, 0] - want[:, 0]) <= 1e-12 * root), (bits[:3], nm)
    # linear stages and the logits against fp64 sums of the fp32 tensors
    _, lin = plan.forward_linear_taps(xc, bits, want=set(range(1, len(bits))))
    fp32 = {'head': lin[-1], 'act_out': logits}
    for i in range(arch['depth']):
        for j, nm in enumerate(('attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2')):
            fp32['blocks.%d.%s' % (i, nm)] = lin[1 + 4 * i + j]
    for nm, t in fp32.items():
        xd, yd = t[:n].double().reshape(n, -1), t[n:].double().reshape(n, -1)
        want = torch.stack([(xd * yd).sum(1), (xd * xd).sum(1), (yd * yd).sum(1)], 1).cpu().numpy()
        root = np.sqrt(want[:, 1:2] * want[:, 2:3])
        assert np.all(np.abs(by2[nm] - want) <= 1e-9 * root), (bits[:3], nm)


def _fused_micro(dva, synth):
    g = load_golden('micro_vit')
    m = micro_model(dva, synth, g).cuda()
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']).cuda())
    return m, g


def test_forward_ddv_micro_vit(dva, oracle, synth):
    m, g = _fused_micro(dva, synth)
    k = load_golden('ddv_micro')
    x = torch.cat((torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])), 0)
    m(x.cuda(), [8] * 10, False)                               # freezes the plan
    sd = {kk[2:]: torch.from_numpy(g[kk]) for kk in g.files if kk.startswith('w/')}
    c = m.export_calib()
    for bits in ([8] * 10, [4] * 10, [int(b) for b in g['bit_qmix']]):
        _check_forward_ddv(dva, oracle, m._plan, synth.ARCHS['micro'], sd, c, x, bits)
    with pytest.raises(AssertionError):
        m._plan.forward_ddv(x[:3].cuda(), [8] * 10)            # an odd batch is no set of pairs


def test_forward_ddv_deit_small(dva, oracle, synth):
    g = load_golden('deit_small')
    arch = synth.ARCHS['deit_small']
    sd = synth.vit_state_dict(arch, int(g['seed']))
    c = golden_calib(g, oracle)
    plan = dva.FrozenPlan(arch, sd, c, device=torch.device('cuda:0'))
    x = synth.images(int(g['seed']), 8, 224, offset=1000)
    L = 4 * arch['depth'] + 2
    for bits in ([8] * L, [4] * L, [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)]):
        _check_forward_ddv(dva, oracle, plan, arch, sd, c, x, bits)


def test_quantized_ddv_matches_reference(dva, synth, monkeypatch):
    """the engine's codes are bit-equal to the reference's at micro size (test_micro_model_vs_reference_golden), so only the fp64
    summation order differs: 1e-9 (test_ddv.test_float_ddv_matches_reference has the derivation).  A fused model takes ONE forward_ddv
    call and never the hooked module graph."""
    m, _ = _fused_micro(dva, synth)
    k = load_golden('ddv_micro')
    x, xa = torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])
    calls = {'engine': 0, 'hooks': 0}
    real_ddv, real_hooks = dva.FrozenPlan.forward_ddv, dva.ddv._hooked_outputs

    def spy_ddv(self, *a, **kw):
        calls['engine'] += 1
        return real_ddv(self, *a, **kw)

    def spy_hooks(*a, **kw):
        calls['hooks'] += 1
        return real_hooks(*a, **kw)
    monkeypatch.setattr(dva.FrozenPlan, 'forward_ddv', spy_ddv)
    monkeypatch.setattr(dva.ddv, '_hooked_outputs', spy_hooks)
    for tag, bits in (('q8', [8] * 10), ('q4', [4] * 10)):
        calls.update(engine=0, hooks=0)
        d = dva.compute_ddv(m, x, xa, bits)
        assert calls == {'engine': 1, 'hooks': 0}, calls
        assert all(v.is_cuda and v.dtype == torch.float64 for v in d.values())
        keys = shared_keys(dva, k, tag, d)
        assert len(keys) == 2 * 6 + 4
        for r in keys:
            err = float(np.abs(d[dva.ddv.REFERENCE_KEYS[r]].cpu().numpy() - k['ddv64/%s/%s' % (tag, r)]).max())
            print(tag, r, err)
            assert err <= 1e-9, (tag, r, err)
    # a -1 entry or model_dequant() leaves the fused state: the module graph with hooks, the same stage names
    d8 = dva.compute_ddv(m, x, xa, [8] * 10)
    calls.update(engine=0, hooks=0)
    dm = dva.compute_ddv(m, x, xa, [8] * 9 + [-1])
    assert list(dm) == list(d8) and calls == {'engine': 0, 'hooks': 2}


def test_float_model_ddv_on_gpu(dva, synth, monkeypatch):
    """module graph + torch.ops.p2vit.pair_cosine against a torch fp64 computation on the SAME GPU activations (rocBLAS float passes
    differ from the host's, so the CPU fixture is no reference here)"""
    m = micro_model(dva, synth, load_golden('micro_vit')).cuda()
    k = load_golden('ddv_micro')
    seen = []
    real = dva.ddv._hooked_outputs

    def spy(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(dva.ddv, '_hooked_outputs', spy)
    d = dva.compute_ddv(m, torch.from_numpy(k['x']), torch.from_numpy(k['x_adv']))
    assert len(seen) == 2 and all(t.is_cuda for t in seen[0])
    for nm, a, b in zip(d, seen[0], seen[1]):
        a, b = a.double().reshape(8, -1), b.double().reshape(8, -1)
        cos = (a * b).sum(1) / (torch.sqrt((a * a).sum(1)) * torch.sqrt((b * b).sum(1)))
        want = cos / torch.sqrt((cos * cos).sum())
        assert float((d[nm] - want).abs().max()) <= 1e-9, nm


def test_refusals_and_cli(dva, tmp_path):
    E = dva.engine
    L = E.lib()
    with pytest.raises(NotImplementedError):
        dva.compute_ddv(dva.swin_tiny_patch4_window7_224(), torch.zeros(2, 3, 224, 224), torch.zeros(2, 3, 224, 224), [8] * 50)
    h = ctypes.c_void_p()
    desc = E.ModelDesc(E.P2V_ABI_VERSION, 224, 16, 3, 384, 12, 6, 1536, 1000)
    E.check(L.p2v_plan_create(ctypes.byref(desc), ctypes.byref(h)))
    assert L.p2v_ddv_stage_count(h, 0) == 63 and L.p2v_ddv_stage_count(h, 1) == 112
    cfg = (ctypes.c_int8 * 50)(*([8] * 50))
    one = ctypes.c_void_p(256)
    with pytest.raises(AssertionError):                        # 2n beyond what a plan takes
        E.check(L.p2v_forward_ddv(h, one, 1 << 30, cfg, 50, one, one, 1 << 40, 0, None, 0, one, None))
    with pytest.raises(E.P2VError):                            # a workspace sized for the plain forward of n images
        E.check(L.p2v_forward_ddv(h, one, 4, cfg, 50, one, one, L.p2v_workspace_bytes(h, 4), 0, None, 0, one, None))
    assert L.p2v_ddv_workspace_bytes(h, 4) > L.p2v_workspace_bytes(h, 8)
    L.p2v_plan_destroy(h)
    out = str(tmp_path / 'ddv_result')
    sim = dva.ddv.main(['--model', 'deit_tiny', '--n', '8', '--result-name', out])
    with open(os.path.join(out, 'ddv.pkl'), 'rb') as f:
        res = pickle.load(f)
    assert list(res['float']) == dva.ddv.stage_names(12, True) == list(res['quantized']) == list(sim)
    assert all(v.shape == (8,) for v in res['quantized'].values())
    assert all(np.isfinite(v) and -1 - 1e-9 <= v <= 1 + 1e-9 for v in sim.values())
