"""GPU: p2v_forward_many / p2v_forward_many_u8 against the per-list forward, bit for bit: a depth-4 micro ViT (17 tokens) under the three
Config variants, the class-row shortcut on and off, one call and sliced over streams, fp32 and uint8 images, inside sentinel arenas;
the DeiT-S fixture model; harness.validate_many and restore.restore_sweep through the new path.  No tolerance anywhere."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

from _arena import Arena, twice
from _tuning import tuning
from conftest import golden_calib, gpu_ok, load_golden
from test_forward_many import flat, nested_lists, restore_lists, tree_counts

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

ARCH = dict(img_size=32, patch_size=8, embed_dim=64, depth=4, num_heads=2, num_classes=10, mlp_ratio=4.0)
N = 4 * ARCH['depth'] + 2
BATCHES = (1, 3, 5)
CONFIGS = {'int': (True, True), 'float': (False, False), 'float_softmax': (True, False)}


def list_sets():
    """the sets of the issue: the full single-restore sweep, seeded random lists that branch at several depths of one path, duplicates,
    lists that differ only in the stem entry, lists that differ only in the head entry"""
    a = nested_lists(ARCH['depth'], 11)[0]
    sets = {'sweep': restore_lists(N, [(i,) for i in range(N)]), 'nested': nested_lists(ARCH['depth'], 11), 'duplicates': [a, a, a],
            'stem': [a, [12 - a[0]] + a[1:]], 'head': [a, a[:-1] + [12 - a[-1]]]}
    assert tree_counts(sets['nested'], ARCH['depth'])['snapshots'] >= 3
    return sets


SETS = list_sets()


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def _micro4(dva, ptf, lis):
    m = dva.VisionTransformer(qkv_bias=True, norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True,
                              cfg=dva.Config(ptf, lis, 'minmax'), **ARCH)
    m.load_state_dict(dva.synth.vit_state_dict(ARCH, 7), strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(8, 4, ARCH['img_size']).cuda())
    with torch.no_grad():
        m(dva.synth.images(9, 1, ARCH['img_size']).cuda(), [8] * N, False)          # freezes the plan
    assert m._plan is not None and m._plan.tokens == 17 and m._plan.depth == 4
    return m


@pytest.fixture(scope='module')
def models(dva):
    return {}


def model_of(dva, models, name):
    if name not in models:
        models[name] = _micro4(dva, *CONFIGS[name])
    return models[name]


_REF = {}


def reference(plan, key, x, lists, fwd=None):
    """plan.forward per distinct list, computed once per (model, batch, entry) and shared: {list as tuple: logits}"""
    ref = _REF.setdefault(key, {})
    for bc in lists:
        if tuple(bc) not in ref:
            ref[tuple(bc)] = (fwd or (lambda b: plan.forward(x, b)))(list(bc)).clone()
    return ref


def images(dva, B):
    return dva.synth.images(21, B, ARCH['img_size'], offset=50).cuda()


def check(out, ref, lists, what):
    assert tuple(out.shape) == (len(lists), ref[tuple(lists[0])].shape[0], ARCH['num_classes'])
    for l, bc in enumerate(lists):
        assert torch.equal(out[l], ref[tuple(bc)]), (what, l, bc, int((out[l] != ref[tuple(bc)]).sum()))


@pytest.mark.parametrize('cls_rows', (1, 0))
@pytest.mark.parametrize('name', list(CONFIGS))
def test_every_set_equals_the_per_list_forward(dva, models, name, cls_rows):
    """one call per set and batch, the class-row shortcut of the last block on and off (the float plans never take it: both runs are the
    full last block there); the counted schedule is the restatement's"""
    plan = model_of(dva, models, name)._plan
    with tuning(dva.engine.lib(), cls_rows=cls_rows):
        for B in BATCHES:
            x = images(dva, B)
            for tag, lists in SETS.items():
                ref = reference(plan, (name, B, 'fp32', cls_rows), x, lists)
                out = plan.forward_many(x, lists)
                torch.cuda.synchronize()
                check(out, ref, lists, (name, cls_rows, B, tag))
                assert torch.isfinite(out).all() and out.abs().max() > 0
    for tag, lists in SETS.items():
        assert plan.forward_many_plan(lists) == tree_counts(lists, ARCH['depth']), tag
    # the shortcut does not change a list's logits either
    for B in BATCHES:
        on, off = _REF.get((name, B, 'fp32', 1)), _REF.get((name, B, 'fp32', 0))
        if on and off:
            assert all(torch.equal(on[k], off[k]) for k in on)


@pytest.mark.parametrize('name', ('int', 'float'))
def test_uint8_form(dva, models, name):
    from diff_vit_amd import data as D
    plan = model_of(dva, models, name)._plan
    mean, std, _ = D.MODEL_STATS['deit']
    lut = plan.input_lut(D.uint8_lut(mean, std))
    for B in BATCHES:
        u8 = dva.synth.images_uint8(31, B, ARCH['img_size']).cuda()
        for tag in ('sweep', 'nested'):
            lists = SETS[tag]
            ref = reference(plan, (name, B, 'u8'), None, lists, lambda b: plan.forward_uint8(u8, lut, b))
            out = plan.forward_many_uint8(u8, lut, lists)
            torch.cuda.synchronize()
            check(out, ref, lists, (name, B, tag, 'u8'))


@pytest.mark.parametrize('n_streams,slices', [(1, [3, 2]), (3, [2, 2, 1]), (3, [1, 1, 1, 2])])
def test_sliced_over_streams(dva, models, n_streams, slices):
    """every slice runs the whole tree on its own stream and workspace; the result is the unsliced one"""
    from diff_vit_amd import data as D
    plan = model_of(dva, models, 'int')._plan
    x = images(dva, 5)
    for tag in ('nested', 'sweep'):
        lists = SETS[tag]
        ref = reference(plan, ('int', 5, 'fp32', 1), x, lists)
        out = plan.forward_many(x, lists, n_streams=n_streams, slices=slices)
        torch.cuda.synchronize()
        check(out, ref, lists, (tag, n_streams, slices))
    mean, std, _ = D.MODEL_STATS['deit']
    lut = plan.input_lut(D.uint8_lut(mean, std))
    u8 = dva.synth.images_uint8(31, 5, ARCH['img_size']).cuda()
    ref = reference(plan, ('int', 5, 'u8'), None, SETS['nested'], lambda b: plan.forward_uint8(u8, lut, b))
    out = plan.forward_many_uint8(u8, lut, SETS['nested'], n_streams=n_streams, slices=slices)
    torch.cuda.synchronize()
    check(out, ref, SETS['nested'], ('u8', n_streams, slices))


@pytest.mark.parametrize('tag', ('nested', 'sweep', 'duplicates'))
def test_in_sentinel_arenas(dva, models, tag):
    """workspace of exactly p2v_forward_many_bytes on a 256-byte boundary and the logits, each between guards, under two fills: nothing
    outside [ws, ws + bytes) and [n_lists][batch][classes] is written, the result does not depend on the fill, a second run repeats the
    first bit for bit, and a workspace one byte short is refused"""
    E = dva.engine
    L = E.lib()
    plan = model_of(dva, models, 'int')._plan
    lists = SETS[tag]
    B = 3
    x = images(dva, B)
    ref = reference(plan, ('int', B, 'fp32', 1), x, lists)
    cfgs = flat(lists)
    need = L.p2v_forward_many_bytes(plan._handle, B, cfgs, len(lists), N)
    snaps = tree_counts(lists, ARCH['depth'])['snapshots']
    assert need == L.p2v_workspace_bytes(plan._handle, B) + snaps * ((B * 17 * 64 + 255) // 256 * 256)

    def run(fill):
        ws = Arena(1, need, None, torch.uint8, fill, offset=0)
        out = Arena(len(lists) * B, ARCH['num_classes'], None, torch.float32, fill)
        E.check(L.p2v_forward_many(plan._handle, E.ptr(x), B, cfgs, len(lists), N, out.ptr, ws.ptr, need, E.stream_ptr()))
        torch.cuda.synchronize()
        ws.read(('workspace', tag, hex(fill)))
        return dict(logits=out.read(('logits', tag, hex(fill))))
    got = twice(run)['logits'].reshape(len(lists), B, ARCH['num_classes'])
    check(got, {k: v.cpu() for k, v in ref.items()}, lists, ('arena', tag))
    if snaps:
        ws = Arena(1, need, None, torch.uint8, 0x5B, offset=0)
        out = Arena(len(lists) * B, ARCH['num_classes'], None, torch.float32, 0x5B)
        rc = L.p2v_forward_many(plan._handle, E.ptr(x), B, cfgs, len(lists), N, out.ptr, ws.ptr, need - 1, E.stream_ptr())
        assert rc == E.E_WORKSPACE and b'p2v_forward_many: workspace %d < %d bytes' % (need - 1, need) in L.p2v_last_error()
        torch.cuda.synchronize()
        assert int((out.dev != 0x5B).sum()) == 0 and int((ws.dev != 0x5B).sum()) == 0           # refused: nothing written


def test_deit_small_fixture(dva, oracle):
    """the DeiT-S fixture model at batch 4: [8] * 50, [4] * 50, the fixture's mixed list and three single restores"""
    g = load_golden('deit_small')
    arch = dva.synth.ARCHS['deit_small']
    plan = dva.FrozenPlan(arch, dva.synth.vit_state_dict(arch, int(g['seed'])), golden_calib(g, oracle))
    lists = [[8] * 50, [4] * 50, [int(b) for b in g['bit_qmix']]] + restore_lists(50, [(0,), (22,), (49,)])[1:]
    x = dva.synth.images(41, 4, arch['img_size'], offset=300).cuda()
    out = plan.forward_many(x, lists)
    torch.cuda.synchronize()
    assert plan.forward_many_plan(lists) == tree_counts(lists, 12)
    for l, bc in enumerate(lists):
        want = plan.forward(x, bc)
        assert torch.equal(out[l], want), (l, int((out[l] != want).sum()))
    assert len({out[l].cpu().numpy().tobytes() for l in range(6)}) == 6            # six lists, six different results


def test_validate_many_and_restore_sweep_through_the_engine_call(dva, models, monkeypatch):
    """validate_many on the fused micro model forwards every batch through FrozenPlan.forward_many (fp32 and uint8 loaders) and returns
    exactly what per-list validate returns; the baseline row of restore_sweep is validate(model, [4] * L)"""
    H = dva.harness
    from diff_vit_amd.restore import restore_sweep
    model = model_of(dva, models, 'int')
    dev = torch.device('cuda:0')
    calls = []
    for name in ('forward_many', 'forward_many_uint8'):
        real = getattr(dva.FrozenPlan, name)
        monkeypatch.setattr(dva.FrozenPlan, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name), _real(self, *a, **k))[1])
    configs = SETS['nested'][:6] + [SETS['nested'][0]]
    for extra, entry in (([], 'forward_many'), (['--uint8-input', '--model', 'deit_tiny'], 'forward_many_uint8')):
        args = H.build_parser().parse_args(['--print-freq', str(10 ** 9)] + extra)
        plain = H.SyntheticLoader(24, 8, ARCH['img_size'], ARCH['num_classes'], seed=3, uint8=bool(extra))
        with torch.no_grad():
            tgt = torch.cat([H._forward(model, d.cuda(), [8] * N, H.uint8_stats(args))[0].argmax(1).cpu() for d, _ in plain])
        loader = H.SyntheticLoader(24, 8, ARCH['img_size'], ARCH['num_classes'], seed=3, targets=tgt, uint8=bool(extra))
        single = [H.validate(args, loader, model, None, dev, c, device_metrics=True) for c in configs]
        del calls[:]
        assert H.validate_many(args, loader, model, dev, configs) == single
        assert calls == [entry] * 3                                                  # three batches, one engine call each
    rows = restore_sweep(args, loader, model, dev, [[0], [5, 9], [N - 1]])
    assert [r[0] for r in rows] == [[], [0], [5, 9], [N - 1]]
    assert rows[0][1:] == H.validate(args, loader, model, None, dev, [4] * N, device_metrics=True)
    assert rows[2][1:] == H.validate(args, loader, model, None, dev, restore_lists(N, [(5, 9)])[1], device_metrics=True)
