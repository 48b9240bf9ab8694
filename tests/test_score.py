"""CPU: scoring with a defined tie rule (score.py) - the numpy restatement against torch, the tie rule on literal rows, DeviceMeter,
the argument checks of the three C entry points, the batched search and validate / validate_many on the micro model."""
import ctypes as C
import os
import random
import sys
from functools import partial

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from conftest import ROOT, load_golden

def loss_bound(classes, ref):
    """(classes + 64) * 2^-52 * max(1, |ref|): a classes-term fp64 sum in any order, 1 ulp each for exp and log, two roundings, 2x margin"""
    return (classes + 64) * 2.0 ** -52 * np.maximum(1.0, np.abs(ref))


def codes(rows, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-128, 128, (rows, classes), generator=g).float() * 2.0 ** -3, torch.randint(0, classes, (rows,), generator=g)


@pytest.mark.parametrize('classes', [10, 1000])
def test_restatement_against_torch(classes):
    from diff_vit_amd.score import score_rows_reference
    x, y = codes(64, classes, classes)
    ranks, loss = score_rows_reference(x, y)
    gt, lo, hi = (ranks[:, c].astype(np.int64) for c in range(3))
    assert (gt >= 0).all() and np.array_equal(ranks[:, 3], [int(np.flatnonzero(r == r.max())[0]) for r in x.numpy()])
    for k in (1, 5):
        top = (x.topk(k, 1, True, True).indices == y[:, None]).any(1).numpy()
        sure, possible = gt + lo + hi < k, gt < k
        assert (sure <= top).all() and (top <= possible).all(), k
    ref = F.cross_entropy(x.double(), y, reduction='none').numpy()
    assert (np.abs(loss - ref) <= loss_bound(classes, ref)).all(), np.abs(loss - ref).max()


def _counts(ranks, ks):
    gt, lo, hi = (ranks[:, c].astype(np.int64) for c in range(3))
    ok = gt >= 0
    return {k: (int((ok & (gt + lo < k)).sum()), int((ok & (gt + lo + hi < k)).sum()), int((ok & (gt < k)).sum())) for k in ks}


def test_tie_rule_on_literal_rows():
    from diff_vit_amd.score import DeviceMeter, score_rows_reference
    row = torch.tensor([[1., 3., 3., 0.]])
    r, _ = score_rows_reference(row, torch.tensor([1]))
    assert r.tolist() == [[0, 0, 1, 1]]
    assert [_counts(r, (1, 2, 3))[k][0] for k in (1, 2, 3)] == [1, 1, 1]
    r, _ = score_rows_reference(row, torch.tensor([2]))
    assert r.tolist() == [[0, 1, 0, 1]]
    c = _counts(r, (1, 2, 3))
    assert [c[k] for k in (1, 2, 3)] == [(0, 0, 1), (1, 1, 1), (1, 1, 1)]          # (hit, sure, possible)
    m = DeviceMeter(ks=(1, 2, 3))
    m.update(row, torch.tensor([2]))
    res = m.result()
    assert [res['prec'][k] for k in (1, 2, 3)] == [0.0, 100.0, 100.0] and [res['sure'][k] for k in (1, 2, 3)] == [0.0, 100.0, 100.0]
    assert [res['possible'][k] for k in (1, 2, 3)] == [100.0, 100.0, 100.0]
    flat = torch.full((7, 7), 0.375)
    r, loss = score_rows_reference(flat, torch.arange(7))
    assert r.tolist() == [[0, y, 6 - y, 0] for y in range(7)]
    assert np.abs(loss - np.log(7.0)).max() <= loss_bound(7, np.log(7.0))
    x, y = codes(5, 10, 1)
    y[1], y[3] = -100, 10
    r, loss = score_rows_reference(x, y)
    assert r[[1, 3], :3].tolist() == [[-1, 0, 0]] * 2 and loss[[1, 3]].tolist() == [0.0, 0.0]
    assert np.array_equal(r[:, 3], [int(np.flatnonzero(v == v.max())[0]) for v in x.numpy()])
    m = DeviceMeter()
    m.update(x, y)
    res = m.result()
    assert res['n'] == 3 and res['invalid'] == 2
    ref = F.cross_entropy(x[[0, 2, 4]].double(), y[[0, 2, 4]], reduction='none').numpy()     # (torch itself refuses label 10)
    assert abs(res['loss'] - ref.mean()) <= 2 * loss_bound(10, ref).max()


def test_device_meter_on_cpu_tensors():
    from diff_vit_amd.score import DeviceMeter, score_rows_reference
    x, y = codes(369, 40, 7)
    y[11], y[200] = -100, 40
    ranks, loss = score_rows_reference(x, y)
    m = DeviceMeter(ks=(1, 5, 9), slots=3)
    for a, b in ((0, 5), (5, 69), (69, 369)):
        m.update(x[a:b], y[a:b], slot=1)
    m.update(x[:5], y[:5], slot=2)
    assert m.result(0)['n'] == 0 and m.result(0)['invalid'] == 0 and m.result(0)['loss'] == 0.0
    res, want = m.result(1), _counts(ranks, (1, 5, 9))
    assert res['n'] == 367 and res['invalid'] == 2
    for k in (1, 5, 9):
        assert (res['prec'][k], res['sure'][k], res['possible'][k]) == tuple(100.0 * v / 367 for v in want[k]), k
    ref_sum = loss[ranks[:, 0] >= 0].sum()
    assert abs(res['loss'] * 367 - ref_sum) <= 369 * 2.0 ** -52 * abs(ref_sum)
    assert m.result(2)['n'] == 5
    m.reset()
    assert m.result(1)['n'] == 0 and m.result(2)['n'] == 0
    with pytest.raises(IndexError):
        m.update(x[:5], y[:5], slot=3)
    with pytest.raises(ValueError):
        DeviceMeter(ks=())
    with pytest.raises(ValueError):
        DeviceMeter(ks=(0, 1))


def test_argument_errors_without_gpu():
    """p2v_score_logits / p2v_score_totals_bytes / p2v_score_accumulate validate before any HIP call"""
    import diff_vit_amd
    E = diff_vit_amd.engine
    L = E.lib()
    one = C.c_void_p(16)
    ok = dict(logits=one, ld=10, rows=4, classes=10, labels=one, ranks=one, loss=one)

    def sl(**kw):
        a = dict(ok, **kw)
        return L.p2v_score_logits(a['logits'], a['ld'], a['rows'], a['classes'], a['labels'], a['ranks'], a['loss'], None)

    for bad in (dict(logits=None), dict(labels=None), dict(ranks=None), dict(loss=None), dict(rows=-1), dict(classes=0), dict(ld=9)):
        assert sl(**bad) == E.E_ARG, bad
        assert b'p2v_score_logits' in L.p2v_last_error()
    assert sl(rows=0) == 0                                                          # succeeds, launches nothing
    assert [L.p2v_score_totals_bytes(n) for n in (0, 1, 2, 8, 9)] == [0, 48, 72, 216, 0]

    def sa(ranks=one, loss=one, rows=4, ks=(1, 5), n_k=None, totals=one):
        arr = (C.c_int * 9)(*ks) if ks is not None else None
        return L.p2v_score_accumulate(ranks, loss, rows, arr, len(ks) if n_k is None else n_k, totals, None)

    for bad in (dict(ranks=None), dict(loss=None), dict(ks=None, n_k=2), dict(totals=None), dict(rows=-1), dict(n_k=0), dict(n_k=9),
                dict(ks=(1, 0)), dict(ks=(-3,))):
        assert sa(**bad) == E.E_ARG, bad
        assert b'p2v_score_accumulate' in L.p2v_last_error()
    assert sa(rows=0) == 0
    with pytest.raises(NotImplementedError):                                        # no CPU kernel behind the ops
        torch.ops.p2vit.score_logits(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.score_accumulate(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.float64), [1, 5],
                                         torch.zeros(9, dtype=torch.long))


def _search_setup():
    import diff_vit_amd as dva
    m = dva.deit_tiny_patch16_224(cfg=dva.Config())
    flops = m.flops()
    rng = random.Random(1)
    gd = [[rng.random() * 0.1 + 0.2, rng.random() * 0.05 + 0.05, rng.random() * 0.04 + 0.04, rng.random() * 0.001] for _ in range(len(flops) - 1)]
    return dva, flops, gd


def test_search_batched_equals_sequential():
    dva, flops, gd = _search_setup()
    calls = []

    def score(cfg):                       # the synthetic score of tests/test_search.py
        calls.append(tuple(cfg))
        return sum((i + 1) * (b == 8) for i, b in enumerate(cfg)) / 10.0

    # slack 1.6: the settings of tests/test_search.py; 1.2: most children break the size constraint and carry the score before them
    for seed, slack in [(s, 1.6) for s in range(5)] + [(s, 1.2) for s in range(5)]:
        kw = dict(log=lambda *a: None, evo_iter=3, slack=slack, max_configs=40)
        del calls[:]
        r1, p1 = dva.search.mixed_precision_search(score, flops, gd, seed=seed, **kw)
        seq = list(calls)
        del calls[:]
        batches = []

        def many(cfgs):
            batches.append([tuple(c) for c in cfgs])
            return [score(c) for c in cfgs]

        def never(cfg):
            raise AssertionError('score_fn called although score_many was given')

        r2, p2 = dva.search.mixed_precision_search(never, flops, gd, seed=seed, score_many=many, **kw)
        assert r1 == r2 and p1 == p2, (seed, slack)
        assert len(batches) == 2 + 3 and len(batches[0]) == 5, [len(b) for b in batches]
        assert slack != 1.6 or len(batches[1]) == 25
        assert [c for b in batches for c in b] == seq, (seed, slack)


def _micro_float(dva):
    a = dva.synth.ARCHS['micro']
    g = load_golden('micro_vit')
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(sd, strict=False)
    return m.eval(), a


def test_validate_and_validate_many_on_the_cpu_micro_model(capsys):
    import diff_vit_amd as dva
    H = dva.harness
    model, a = _micro_float(dva)
    args = H.build_parser().parse_args(['--print-freq', '2'])
    loader = H.SyntheticLoader(24, 8, a['img_size'], a['num_classes'], seed=3)
    with torch.no_grad():
        logits = torch.cat([model(d, None, False)[0] for d, _ in loader])
    tgt = logits.argsort(1, descending=True)[torch.arange(24), torch.arange(24) % 6]          # labels of rank 1 .. 6: both boundaries are hit
    loader = H.SyntheticLoader(24, 8, a['img_size'], a['num_classes'], seed=3, targets=tgt)
    meter = dva.DeviceMeter()
    meter.update(logits, tgt)
    r = meter.result()
    assert r['sure'] == r['possible'] and 0.0 < r['prec'][1] < r['prec'][5] < 100.0          # no boundary ties for this seed
    ref = H.validate(args, loader, model, torch.nn.CrossEntropyLoss(), 'cpu')
    capsys.readouterr()
    got = H.validate(args, loader, model, None, 'cpu', device_metrics=True)
    out = capsys.readouterr().out
    assert got[1] == ref[1] and got[2] == ref[2] and (got[1], got[2]) == (r['prec'][1], r['prec'][5])
    assert abs(got[0] - ref[0]) <= 1e-5 * max(1.0, abs(ref[0]))                               # the default path's loss is fp32
    assert out.count('Test: [') == 2 and ' * Prec@1 %.3f Prec@5 %.3f' % (got[1], got[2]) in out and ' * ties: Prec@1 in [' in out
    c1, c2 = [8] * 10, [4] * 10
    single = [H.validate(args, loader, model, None, 'cpu', c, device_metrics=True) for c in (c1, c2, c1)]
    calls = []
    fwd = H._forward
    H._forward = lambda *a, **k: (calls.append(1), fwd(*a, **k))[1]
    try:
        many = H.validate_many(args, loader, model, 'cpu', [c1, c2, c1])
    finally:
        H._forward = fwd
    assert many == single and len(calls) == 3 * 2                                             # loss bits included; duplicates scored once
    assert H.validate_many(args, loader, model, 'cpu', []) == []


def _reduce_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import diff_vit_amd as dva
    x, y = codes(50, 12, 21)
    m = dva.DeviceMeter(slots=2)
    lo, hi = (0, 20) if rank == 0 else (20, 50)
    m.update(x[lo:hi], y[lo:hi], slot=1)
    m.all_reduce()
    if rank == 0:
        q.put((m.result(0), m.result(1)))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_gloo_world_2():
    import diff_vit_amd as dva
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 977) % 2000
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    r0, r1 = q.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    x, y = codes(50, 12, 21)
    one = dva.DeviceMeter()
    one.update(x, y)
    want = one.result()
    assert r0['n'] == 0 and r1['n'] == 50
    assert {k: v for k, v in r1.items() if k != 'loss'} == {k: v for k, v in want.items() if k != 'loss'}
    assert abs(r1['loss'] - want['loss']) <= 50 * 2.0 ** -52 * abs(want['loss'])
