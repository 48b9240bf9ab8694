"""CPU: many bit lists in one call (p2v_forward_many): the four symbols and their binding, the counted schedule of
p2v_forward_many_plan against the expected numbers and against a pure-Python restatement of the prefix tree, every refusal before the
first HIP call, VisionTransformer.forward_many in the states that run the per-list forward, and the restore sweep's command line."""
import ctypes as C
import json
import os
import random
import re
from functools import partial

import pytest
import torch

from conftest import ROOT

MANY = ('p2v_forward_many', 'p2v_forward_many_u8', 'p2v_forward_many_bytes', 'p2v_forward_many_plan')
COUNTS = ('stems', 'blocks', 'norms', 'heads', 'copies', 'snapshots')
_ONE = C.c_void_p(4096)           # a non-null, 256-byte aligned "device pointer" that is never followed


def tree_counts(lists, depth):
    """pure-Python restatement of the schedule in include/p2vit.h: a prefix tree keyed by cfg[0], then the four entries of every block;
    children in order of first appearance; a node behind the stem with c > 1 children costs c copies of x and holds one slot while its
    children run; under a distinct block prefix one final norm and one head GEMM per distinct last entry"""
    n = 4 * depth + 2
    assert all(len(l) == n for l in lists)
    c = dict.fromkeys(COUNTS, 0)

    def key(l, level):
        return (l[0],) if level == 0 else tuple(l[1 + 4 * (level - 1):5 + 4 * (level - 1)])

    def visit(group, level, held):
        if level == depth + 1:
            c['norms'] += 1
            c['heads'] += len(dict.fromkeys(l[-1] for l in group))
            return
        kids = {}
        for l in group:
            kids.setdefault(key(l, level), []).append(l)
        keep = level > 0 and len(kids) > 1
        if keep:
            c['copies'] += len(kids)
            c['snapshots'] = max(c['snapshots'], held + 1)
        for g in kids.values():
            c['stems' if level == 0 else 'blocks'] += 1
            visit(g, level + 1, held + keep)
    visit([tuple(l) for l in lists], 0, 0)
    return c


def restore_lists(n, combos):
    return [[8 if i in c else 4 for i in range(n)] for c in [()] + [tuple(c) for c in combos]]


def nested_lists(depth, seed, n_lists=24):
    """seeded random lists that branch late and often: each new list copies an earlier one up to a random block and is random behind it,
    plus the first list with only its head flipped, an exact duplicate, and one list with another stem entry"""
    rng, n = random.Random(seed), 4 * depth + 2
    lists = [[rng.choice((4, 8)) for _ in range(n)]]
    while len(lists) < n_lists:
        cut = 1 + 4 * rng.randrange(depth + 1)
        lists.append(lists[rng.randrange(len(lists))][:cut] + [rng.choice((4, 8)) for _ in range(n - cut)])
    lists.append(lists[0][:-1] + [12 - lists[0][-1]])
    lists.append(list(lists[3]))
    lists.append([12 - lists[1][0]] + lists[1][1:])
    return lists


def flat(lists):
    return (C.c_int8 * sum(len(l) for l in lists))(*[b for l in lists for b in l])


def plan_counts(E, h, lists, n_cfg=None):
    v = [C.c_int(-1) for _ in COUNTS]
    E.check(E.lib().p2v_forward_many_plan(h, flat(lists), len(lists), len(lists[0]) if n_cfg is None else n_cfg, *[C.byref(x) for x in v]))
    return {k: x.value for k, x in zip(COUNTS, v)}


@pytest.fixture(scope='module')
def E():
    import diff_vit_amd
    return diff_vit_amd.engine


@pytest.fixture()
def deit_s(E):
    """a DeiT-S description: the dry pass needs the geometry only (no setter, no GPU)"""
    h = C.c_void_p()
    E.check(E.lib().p2v_plan_create(C.byref(E.ModelDesc(E.P2V_ABI_VERSION, 224, 16, 3, 384, 12, 6, 1536, 1000)), C.byref(h)))
    yield h
    E.lib().p2v_plan_destroy(h)


def test_symbols_declared_exported_and_bound(E):
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'p2vit.h')).read(), flags=re.S)
    L = E.lib()
    raw = C.CDLL(E.LIB_PATH)
    for name in MANY:
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    assert L.p2v_forward_many_bytes.restype is C.c_size_t
    assert L.p2v_abi_version() == 6 == E.P2V_ABI_VERSION


def test_counts_of_the_single_restore_sweep(E, deit_s):
    """51 lists on a depth-12 model: 336 blocks instead of 612"""
    lists = restore_lists(50, [(i,) for i in range(50)])
    got = plan_counts(E, deit_s, lists)
    assert (got['stems'], got['blocks'], got['norms'], got['heads']) == (2, 336, 50, 51), got
    assert got['snapshots'] >= 1
    assert got == tree_counts(lists, 12)
    # the workspace: the forward's plus `snapshots` slots of x, each a multiple of 256 bytes
    L = E.lib()
    slot = (256 * 197 * 384 + 255) // 256 * 256
    assert L.p2v_forward_many_bytes(deit_s, 256, flat(lists), 51, 50) == L.p2v_workspace_bytes(deit_s, 256) + got['snapshots'] * slot
    assert L.p2v_forward_many_bytes(deit_s, 256, flat(lists[:1]), 1, 50) == L.p2v_workspace_bytes(deit_s, 256)


def test_counts_of_small_sets(E, deit_s):
    a = [random.Random(5).choice((4, 8)) for _ in range(50)]
    got = plan_counts(E, deit_s, [a, a, a])
    assert (got['stems'], got['blocks'], got['norms'], got['heads'], got['copies']) == (1, 12, 1, 1, 0), got
    got = plan_counts(E, deit_s, [a, [12 - a[0]] + a[1:]])
    assert got['blocks'] == 24 and got['stems'] == 2, got
    got = plan_counts(E, deit_s, [a, a[:-1] + [12 - a[-1]]])
    assert (got['blocks'], got['norms'], got['heads'], got['copies']) == (12, 1, 2, 0), got


@pytest.mark.parametrize('seed', range(6))
def test_counts_of_random_lists_against_the_restatement(E, deit_s, seed):
    lists = nested_lists(12, seed)
    want = tree_counts(lists, 12)
    assert plan_counts(E, deit_s, lists) == want
    assert want['blocks'] < len(lists) * 12 and want['snapshots'] >= 2
    rng = random.Random(100 + seed)
    lists = [[rng.choice((4, 8)) for _ in range(50)] for _ in range(40)]
    assert plan_counts(E, deit_s, lists) == tree_counts(lists, 12)


def test_null_counts_are_skipped(E, deit_s):
    blocks = C.c_int(-1)
    lists = restore_lists(50, [(3,), (7,)])
    assert E.lib().p2v_forward_many_plan(deit_s, flat(lists), 3, 50, None, C.byref(blocks), None, None, None, None) == 0
    assert blocks.value == tree_counts(lists, 12)['blocks']


class _DummyPlan:
    """a depth-1 plan (5 tokens, 6 layers) over dummy pointers, which reaches every check that runs before the first HIP call;
    `without`: (layer, bits) pairs to leave unset"""

    def __init__(self, E, without=()):
        self.L = E.lib()
        self.h = C.c_void_p()
        E.check(self.L.p2v_plan_create(C.byref(E.ModelDesc(E.P2V_ABI_VERSION, 32, 16, 3, 64, 1, 2, 128, 10)), C.byref(self.h)))
        lin = E.Linear(_ONE, _ONE, _ONE, None, 0)
        for layer in range(6):
            for bits in (4, 8):
                if (layer, bits) not in without:
                    E.check(self.L.p2v_plan_set_linear(self.h, layer, bits, C.byref(lin)))
        E.check(self.L.p2v_plan_set_embed(self.h, 16.0, C.byref(E.Epilogue()), _ONE))
        b = E.Block()
        ln = E.Ln(1.0, _ONE, _ONE, _ONE, _ONE, _ONE, None)
        for i in range(2):
            b.ln1[i] = ln
            b.inv_s_qkv[i] = 16.0
            for j in range(2):
                b.ln2[i][j] = ln
        b.attn = E.Attn(2.0 ** -8, 0.125, 16.0, 0.5, -12, 43, 714)
        for e in (b.proj_epi, b.fc2_epi):
            e.s_mid, e.s_res, e.s_next = _ONE, _ONE, _ONE
        b.inv_s_fc1 = 8.0
        b.gelu_fc1 = E.GeluTab(None, 0.0, 0.0, 0)
        E.check(self.L.p2v_plan_set_block(self.h, 0, C.byref(b)))
        E.check(self.L.p2v_plan_set_head(self.h, C.byref(ln), 1.0, 1.0))

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        self.L.p2v_plan_destroy(self.h)


def _refused(L, rc, code, *texts):
    msg = L.p2v_last_error()
    assert rc == code and all(t in msg for t in texts), (rc, code, msg)


def test_refusals_before_any_hip_call(E):
    """null argument, n_cfg, an entry outside {4, 8}, n_lists outside 1 ... 4096, a short workspace, and per list what p2v_forward
    refuses - each with its status and a message that names the entry point"""
    L = E.lib()
    two = [[8] * 6, [8, 4, 4, 8, 8, 4]]
    big = 1 << 40

    def many(h, images=_ONE, batch=2, lists=two, n_lists=None, n_cfg=6, logits=_ONE, ws=_ONE, ws_bytes=big, cfgs=True):
        return L.p2v_forward_many(h, images, batch, flat(lists) if cfgs else None, len(lists) if n_lists is None else n_lists, n_cfg, logits,
                                  ws, ws_bytes, None)

    def many_u8(h, images=_ONE, layout=0, lut=_ONE, lists=two, n_lists=None, n_cfg=6, ws_bytes=big):
        return L.p2v_forward_many_u8(h, images, layout, lut, 2, flat(lists), len(lists) if n_lists is None else n_lists, n_cfg, _ONE, _ONE,
                                     ws_bytes, None)

    with _DummyPlan(E) as h:
        need = L.p2v_forward_many_bytes(h, 2, flat(two), 2, 6)
        assert need == L.p2v_workspace_bytes(h, 2) + (2 * 5 * 64 + 255) // 256 * 256            # one branching node: one slot of x
        for null in (dict(images=None), dict(logits=None), dict(ws=None), dict(cfgs=False)):
            _refused(L, many(h, **null), E.E_ARG, b'p2v_forward_many: null argument')
        _refused(L, many(None), E.E_ARG, b'p2v_forward_many: null argument')
        _refused(L, many(h, batch=0), E.E_SHAPE, b'p2v_forward_many: batch must be positive')
        for n in (0, -1, 4097):
            _refused(L, many(h, n_lists=n), E.E_SHAPE, b'p2v_forward_many: %d lists' % n)
        _refused(L, many(h, n_cfg=5), E.E_BITS, b'p2v_forward_many: the bit lists have 5 entries, model needs 6')
        for bad in (6, 0, -1, 16):
            _refused(L, many(h, lists=[[8] * 6, [8, 8, bad, 8, 8, 8]]), E.E_BITS, b'p2v_forward_many: list 1: %d is not in list' % bad)
        _refused(L, many(h, ws_bytes=need - 1), E.E_WORKSPACE, b'p2v_forward_many: workspace %d < %d bytes' % (need - 1, need))
        _refused(L, many(h, ws_bytes=L.p2v_workspace_bytes(h, 2)), E.E_WORKSPACE, b'p2v_forward_many: workspace')   # the forward's part alone
        # the uint8 form: its image checks first, then the same list
        _refused(L, many_u8(h, lut=None), E.E_ARG, b'p2v_forward_many_u8: null images or lut')
        _refused(L, many_u8(h, layout=2), E.E_ARG, b'p2v_forward_many_u8: unknown layout 2')
        _refused(L, many_u8(h, images=C.c_void_p(4098)), E.E_ARG, b'p2v_forward_many_u8: images must start on a 4-byte boundary')
        _refused(L, many_u8(h, n_lists=0), E.E_SHAPE, b'p2v_forward_many_u8: 0 lists')
        _refused(L, many_u8(h, n_cfg=7), E.E_BITS, b'p2v_forward_many_u8: the bit lists have 7 entries')
        _refused(L, many_u8(h, ws_bytes=need - 1), E.E_WORKSPACE, b'p2v_forward_many_u8: workspace %d < %d bytes' % (need - 1, need))
        # the queries refuse the same lists: 0 bytes, and the dry pass its status
        assert L.p2v_forward_many_bytes(h, 2, flat(two), 2, 5) == 0 and L.p2v_forward_many_bytes(h, 0, flat(two), 2, 6) == 0
        assert L.p2v_forward_many_bytes(h, 2, flat(two), 0, 6) == 0 and L.p2v_forward_many_bytes(None, 2, flat(two), 2, 6) == 0
        assert L.p2v_forward_many_bytes(h, 2, flat([[8] * 6, [8, 8, 5, 8, 8, 8]]), 2, 6) == 0
        v = [C.c_int() for _ in COUNTS]
        out = [C.byref(x) for x in v]
        _refused(L, L.p2v_forward_many_plan(h, None, 2, 6, *out), E.E_ARG, b'p2v_forward_many_plan: null argument')
        _refused(L, L.p2v_forward_many_plan(h, flat(two), 4097, 6, *out), E.E_SHAPE, b'p2v_forward_many_plan: 4097 lists')
        _refused(L, L.p2v_forward_many_plan(h, flat(two), 2, 5, *out), E.E_BITS, b'p2v_forward_many_plan: the bit lists have 5 entries')
    with _DummyPlan(E, without=((3, 4),)) as h:
        # a layer that was not set at the width a list names: the status p2v_forward gives the same list, the message names call and list
        one = (C.c_int8 * 6)(8, 4, 4, 4, 8, 4)
        rc_one = L.p2v_forward(h, _ONE, 2, one, 6, _ONE, _ONE, big, -1, None)
        _refused(L, rc_one, E.E_STATE, b'layer 3 has no 4-bit weights')
        _refused(L, many(h, lists=[[8] * 6, list(one)]), E.E_STATE, b'p2v_forward_many: list 1: layer 3 has no 4-bit weights')
        _refused(L, many(h, lists=[[8] * 6], ws_bytes=0), E.E_WORKSPACE, b'p2v_forward_many: workspace 0 <')


# ---- VisionTransformer.forward_many where it is the per-list forward ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def micro_model(micro):
    import diff_vit_amd as dva
    a = micro['arch']
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(micro['sd'], strict=False)
    m = m.eval()
    dva.harness.calibrate_model(m, micro['x_cal'])
    return m


def test_model_forward_many_on_the_cpu(micro_model, micro):
    """float state, fake-quant (dequant) state and a list with -1: list by list what model(x, cfg)[0] gives"""
    import diff_vit_amd as dva
    m, x = micro_model, micro['x_ev']
    n = 4 * micro['arch']['depth'] + 2
    lists = [[8] * n, [4] * n, [8 if i % 3 else 4 for i in range(n)], [8] * n]
    try:
        m.model_dequant()
        with torch.no_grad():
            outs = m.forward_many(x, lists)
            assert len(outs) == 4
            for o, bc in zip(outs, lists):
                assert torch.equal(o, m(x, bc)[0])
            assert torch.equal(dva.forward_many(m, x, lists)[2], outs[2])
            assert m.forward_many(x, []) == []
    finally:
        m.model_quant()
    a = micro['arch']
    f = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    f.load_state_dict(micro['sd'], strict=False)
    f = f.eval()                                                        # the float model: never calibrated, takes any list or none
    with torch.no_grad():
        want = f(x, None)[0]
        for o in f.forward_many(x, [None, [8] * n, [4] * n]):
            assert torch.equal(o, want)


def test_model_forward_many_with_a_float_layer(micro):
    """a -1 entry sends the whole call down the per-list module graph, as forward does with that list (a model of its own: the -1 flips
    the block's norm to float for good)"""
    import diff_vit_amd as dva
    a = micro['arch']
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(micro['sd'], strict=False)
    m = m.eval()
    dva.harness.calibrate_model(m, micro['x_cal'])
    n = 4 * a['depth'] + 2
    lists = [[8] * 3 + [-1] + [8] * (n - 4), [8] * n]
    with torch.no_grad():
        want = [m(micro['x_ev'], bc)[0] for bc in lists]
        outs = m.forward_many(micro['x_ev'], lists)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)


# ---- the restore sweep -------------------------------------------------------------------------------------------------------------------
def test_combination_enumeration_and_sampling():
    from diff_vit_amd.restore import enumerate_combinations, restored_list
    assert enumerate_combinations(50, 1) == [[i] for i in range(50)]
    assert enumerate_combinations(5, 2, 10) == [[0, 1], [0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [1, 4], [2, 3], [2, 4], [3, 4]]
    assert enumerate_combinations(6, 0) == [[]]
    s = enumerate_combinations(50, 4, 30, seed=3)
    assert len(s) == 30 and len({tuple(c) for c in s}) == 30
    assert all(c == sorted(c) and len(set(c)) == 4 and 0 <= c[0] and c[-1] < 50 for c in s)
    assert s == enumerate_combinations(50, 4, 30, seed=3) and s != enumerate_combinations(50, 4, 30, seed=4)
    assert len(enumerate_combinations(5, 2, 9, seed=0)) == 9                                   # one short of all ten: sampled
    with pytest.raises(ValueError):
        enumerate_combinations(10, 11)
    assert restored_list(6, [1, 4]) == [4, 8, 4, 4, 8, 4]
    with pytest.raises(ValueError):
        restored_list(6, [6])


def test_restore_line_formats():
    from diff_vit_amd.restore import format_line
    assert format_line([], 12.3456, 50.0, 1.5) == ' * Restore Index: nothing, Prec@1 12.346 Prec@5 50.000 Time 1.500'
    assert format_line([2, 17], 1.0, 2.25, 0.125) == ' *Restore Indices: [2, 17], Prec@1 1.000 Prec@5 2.250 Time 0.125'


def test_restore_main_on_the_cpu_micro_model(tmp_path, monkeypatch, capsys):
    """restore.main end to end on the CPU (a model in quant state has no CPU forward, so the sweep's lists are scored on the calibrated
    model's fake-quant path): rows, printed lines and the appended file"""
    import diff_vit_amd as dva
    from diff_vit_amd import harness, restore, vit
    a = dva.synth.ARCHS['micro']

    def micro_factory(pretrained=False, cfg=None, **kw):
        return vit.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                                     num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                                     norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=cfg)
    monkeypatch.setattr(harness, 'str2model', lambda name: micro_factory)
    seen = {}
    real = harness.validate_many

    def fake_validate_many(args, loader, model, device, bit_configs):
        # (a calibrated model in quant state has no CPU forward: score the lists on the fake-quant graph)
        seen['lists'] = [list(bc) for bc in bit_configs]
        model.model_dequant()
        try:
            return real(args, loader, model, device, bit_configs)
        finally:
            model.model_quant()
    monkeypatch.setattr(harness, 'validate_many', fake_validate_many)
    n = 4 * a['depth'] + 2
    combos = tmp_path / 'combos.json'
    combos.write_text(json.dumps([[1, 0], [n - 1, 2]]))
    common = ['--model', 'micro', '--device', 'cpu', '--n-val', '6', '--val-batchsize', '3', '--calib-batchsize', '2', '--out-dir', str(tmp_path)]
    rows = restore.main(common + ['--combos', str(combos)])
    assert [r[0] for r in rows] == [[], [0, 1], [2, n - 1]]
    assert seen['lists'] == restore_lists(n, [(0, 1), (2, n - 1)])
    out = capsys.readouterr().out
    lines = (tmp_path / 'restore_2_layers.txt').read_text().splitlines()
    assert len(lines) == 3 and all(l in out for l in lines)
    assert re.fullmatch(r' \* Restore Index: nothing, Prec@1 \d+\.\d{3} Prec@5 \d+\.\d{3} Time \d+\.\d{3}', lines[0]), lines[0]
    assert re.fullmatch(r' \*Restore Indices: \[0, 1\], Prec@1 \d+\.\d{3} Prec@5 \d+\.\d{3} Time \d+\.\d{3}', lines[1]), lines[1]
    assert lines[2].startswith(' *Restore Indices: [2, %d], Prec@1 ' % (n - 1))
    for (idx, loss, top1, top5), line in zip(rows, lines):
        assert 'Prec@1 %.3f Prec@5 %.3f' % (top1, top5) in line
    # K-subsets: all of them under --max-combos, appended to the file of that K; a second run appends
    rows = restore.main(common + ['--restore', '1'])
    assert [r[0] for r in rows] == [[]] + [[i] for i in range(n)]
    rows = restore.main(common + ['--restore', '1', '--max-combos', '4', '--seed', '2'])
    assert [r[0] for r in rows] == [[]] + restore.enumerate_combinations(n, 1, 4, 2)
    assert len((tmp_path / 'restore_1_layers.txt').read_text().splitlines()) == (n + 1) + 5
