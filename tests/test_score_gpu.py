"""GPU: the score kernels (p2vit_score.hip) against score.score_rows_reference - ranks and counters bit for bit, the fp64 loss within
(classes + 64) * 2^-52 * max(1, |ref|) - their output footprint, the running totals, and DeviceMeter / validate / validate_many on the
micro-ViT through the engine."""
import re
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _arena import Arena, twice
from conftest import gpu_ok, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

KS8 = (1, 2, 3, 5, 7, 10, 100, 1000)


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def loss_bound(classes, ref):
    """a classes-term fp64 sum in any order ((classes - 1) * 2^-53), 1 ulp each for exp and log, two roundings, 2x margin"""
    return (classes + 64) * 2.0 ** -52 * np.maximum(1.0, np.abs(ref))


def make_case(rows, classes, seed):
    """int8 codes x 2^-3 (many ties at 1000 classes) and labels that cycle through: 0, classes - 1, the argmax, a class tied with the
    maximum, -100, classes, then random classes"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-128, 128, (rows, classes), generator=g).float() * 2.0 ** -3
    y = torch.randint(0, classes, (rows,), generator=g)
    for r in range(rows):
        am = int(x[r].argmax())
        kind = r % 8
        if kind == 0:
            y[r] = 0
        elif kind == 1:
            y[r] = classes - 1
        elif kind == 2:
            y[r] = am
        elif kind == 3:
            other = (am + 1 + r) % classes
            x[r, other] = x[r, am]
            y[r] = other
        elif kind == 4:
            y[r] = -100
        elif kind == 5:
            y[r] = classes
    return x, y


def check_records(dva, x, y, ranks, loss, what):
    classes = x.shape[1]
    ref_ranks, ref_loss = dva.score_rows_reference(x, y)
    assert np.array_equal(ranks, ref_ranks), (what, np.argwhere(ranks != ref_ranks)[:4].tolist())
    ok = ref_ranks[:, 0] >= 0
    assert (loss[~ok] == 0.0).all(), what
    err = np.abs(loss[ok] - ref_loss[ok])
    assert (err <= loss_bound(classes, ref_loss[ok])).all(), (what, float(err.max()))
    return ref_ranks, ref_loss


@pytest.mark.parametrize('classes', [1, 2, 63, 64, 65, 1000, 1003])
def test_score_logits_against_reference(dva, classes):
    for rows in (1, 3, 64, 257):
        x, y = make_case(rows, classes, 1000 * classes + rows)
        yd = y.cuda()
        for ld, pad in ((classes, None), (classes + 5, float('inf')), ((classes + 3) // 4 * 4 + 4, float('nan'))):
            if pad is None:
                view = x.cuda()
            else:
                buf = torch.full((rows, ld), pad, device='cuda')
                buf[:, :classes] = x.cuda()
                view = buf[:, :classes]                       # rows ld floats apart: 16-byte aligned for ld % 4 == 0 only
            ranks, loss = torch.ops.p2vit.score_logits(view, yd)
            check_records(dva, x, y, ranks.cpu().numpy(), loss.cpu().numpy(), (rows, classes, ld))
    if classes == 1000:                                       # the same bound against torch's double-precision cross-entropy
        ok = ((y >= 0) & (y < classes)).numpy()
        ref = F.cross_entropy(x[ok].double(), y[ok], reduction='none').numpy()
        assert (np.abs(loss.cpu().numpy()[ok] - ref) <= loss_bound(classes, ref)).all()


def test_score_logits_21843_classes(dva):
    x, y = make_case(3, 21843, 5)
    y[0], y[1], y[2] = 21842, int(x[1].argmax()), 17
    ranks, loss = torch.ops.p2vit.score_logits(x.cuda(), y.cuda())
    check_records(dva, x, y, ranks.cpu().numpy(), loss.cpu().numpy(), 'imagenet-21k')


def test_output_footprint(dva):
    """ranks and loss inside sentinel arenas: only the records of rows [0, rows) change, the logits (strided, poisoned padding) do not"""
    E = dva.engine
    L = E.lib()
    rows, classes, ld = 7, 65, 70
    x, y = make_case(rows, classes, 11)
    yd = y.cuda()

    def run(sentinel):
        a_x = Arena(rows, classes, stride=ld, dtype=torch.float32, sentinel=sentinel, init=x)
        a_r = Arena(rows, 4, dtype=torch.int32, sentinel=sentinel)
        a_l = Arena(1, rows * 8, dtype=torch.uint8, sentinel=sentinel)
        before = a_x.dev.clone()
        E.check(L.p2v_score_logits(a_x.ptr, ld, rows, classes, E.ptr(yd), a_r.ptr, a_l.ptr, E.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(a_x.dev, before), 'the logits buffer changed'
        ranks = a_r.read('ranks')
        loss = torch.from_numpy(a_l.read('loss').numpy().reshape(-1).view(np.float64).copy())
        return {'ranks': ranks, 'loss_bits': loss.view(torch.int64)}

    got = twice(run)
    check_records(dva, x, y, got['ranks'].numpy(), got['loss_bits'].view(torch.float64).numpy(), 'arena')


def test_score_accumulate(dva):
    E = dva.engine
    L = E.lib()
    classes = 1003
    x, y = make_case(369, classes, 23)
    ranks, loss = torch.ops.p2vit.score_logits(x.cuda(), y.cuda())
    ref_ranks, _ = check_records(dva, x, y, ranks.cpu().numpy(), loss.cpu().numpy(), 'accumulate')
    W = 3 + 3 * len(KS8)
    assert L.p2v_score_totals_bytes(len(KS8)) == 8 * W

    def run():
        totals = torch.full((3, W), 0x5B5B5B5B5B5B5B5B, dtype=torch.int64, device='cuda')
        totals[1].zero_()
        for a, b in ((0, 5), (5, 69), (69, 369)):
            torch.ops.p2vit.score_accumulate(ranks[a:b], loss[a:b], list(KS8), totals[1])
        return totals.cpu().numpy()

    t = run()
    assert (t[0] == 0x5B5B5B5B5B5B5B5B).all() and (t[2] == 0x5B5B5B5B5B5B5B5B).all()
    gt, lo, hi = (ref_ranks[:, c].astype(np.int64) for c in range(3))
    ok = gt >= 0
    want = [int(ok.sum()), int((~ok).sum())]
    want += [int((ok & (gt + lo < k)).sum()) for k in KS8] + [int((ok & (gt + lo + hi < k)).sum()) for k in KS8] + [int((ok & (gt < k)).sum()) for k in KS8]
    assert t[1, :-1].tolist() == want
    assert want[1] > 0 and want[2] < want[2 + 2 * len(KS8)], 'the case has invalid labels and top-1 ties'
    loss_sum = float(t[1, -1:].view(np.float64)[0])
    dev_rows = loss.cpu().numpy()[ok]                         # the per-row losses have their own bound: the sum is checked on its own
    assert abs(loss_sum - dev_rows.sum()) <= 369 * 2.0 ** -52 * np.abs(dev_rows).sum()
    assert np.array_equal(run(), t), 'a second identical run differs'
    m = dva.DeviceMeter(ks=KS8, slots=3)                      # the same through the meter
    for a, b in ((0, 5), (5, 69), (69, 369)):
        m.update(x[a:b].cuda(), y[a:b].cuda(), slot=1)
    assert np.array_equal(m.totals.cpu().numpy()[1], t[1]) and m.result(0)['n'] == 0 and m.result(2)['n'] == 0
    r = m.result(1)
    assert r['n'] == want[0] and r['prec'][1000] == 100.0 * want[2 + 7] / want[0]


def _micro_quant(dva):
    g = load_golden('micro_vit')
    a = dva.synth.ARCHS['micro']
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    model = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                                  num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                                  norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    model.load_state_dict(sd, strict=False)
    model = model.to('cuda:0').eval()
    dva.harness.calibrate_model(model, torch.from_numpy(g['x_cal']).to('cuda:0'))
    return model, a, g


@pytest.fixture(scope='module')
def micro_quant(dva):
    return _micro_quant(dva)


def _bit_lists(g):
    return {'q8': [8] * 10, 'q4': [4] * 10, 'qmix': [int(b) for b in g['bit_qmix']]}


def test_engine_logits_through_the_meter(dva, micro_quant):
    model, a, g = micro_quant
    x = torch.from_numpy(g['x_ev']).cuda()
    for tag, bits in _bit_lists(g).items():
        with torch.no_grad():
            out = model(x, bits, False)[0]
        host = out.cpu()
        if tag == 'q8':
            assert np.array_equal(host.numpy(), g['logits/q8'])
        order = host.argsort(dim=1, descending=True, stable=True)
        for rank in (0, 4, 5):                                # every image labelled with its 1st, 5th, 6th ranked class
            tgt = order[:, rank].contiguous()
            rr, _ = dva.score_rows_reference(host, tgt)
            gt, lo, hi = (rr[:, c].astype(np.int64) for c in range(3))
            for k in (1, 5):                                  # the fixture's logits have no tie at either boundary
                assert np.array_equal(gt + lo + hi < k, gt < k), (tag, rank, k)
            m = dva.DeviceMeter()
            m.update(out, tgt.cuda())
            res = m.result()
            acc = dva.harness.accuracy(host, tgt, topk=(1, 5))
            hits = [int(round(v.item() * 6 / 100.0)) for v in acc]
            assert hits == [6 * (rank < 1), 6 * (rank < 5)], (tag, rank, hits)
            assert (res['prec'][1], res['prec'][5]) == (100.0 * hits[0] / 6, 100.0 * hits[1] / 6), (tag, rank)
            assert res['sure'] == res['possible'] == res['prec'] and res['n'] == 6 and res['invalid'] == 0
            ref = F.cross_entropy(host.double(), tgt, reduction='none').numpy()
            _, loss = torch.ops.p2vit.score_logits(out, tgt.cuda())
            assert (np.abs(loss.cpu().numpy() - ref) <= loss_bound(10, ref)).all(), (tag, rank)
            assert abs(res['loss'] - ref.mean()) <= loss_bound(10, ref).max() + 6 * 2.0 ** -52 * np.abs(ref).mean()


def test_validate_and_validate_many_on_the_gpu(dva, micro_quant, capsys):
    model, a, g = micro_quant
    H = dva.harness
    dev = torch.device('cuda:0')
    lists = _bit_lists(g)
    args = H.build_parser().parse_args(['--print-freq', '100'])
    plain = H.SyntheticLoader(24, 8, a['img_size'], a['num_classes'], seed=3)
    with torch.no_grad():
        logits = torch.cat([model(d.cuda(), lists['q8'], False)[0].cpu() for d, _ in plain])
    tgt = logits.argsort(dim=1, descending=True, stable=True)[torch.arange(24), torch.arange(24) % 6]
    loader = H.SyntheticLoader(24, 8, a['img_size'], a['num_classes'], seed=3, targets=tgt)
    meter = dva.DeviceMeter()
    meter.update(logits, tgt)                                 # the bracket, from the host copy through the reference
    r = meter.result()
    ref = H.validate(args, loader, model, torch.nn.CrossEntropyLoss().to(dev), dev, lists['q8'])
    got = H.validate(args, loader, model, None, dev, lists['q8'], device_metrics=True)
    out = capsys.readouterr().out
    assert ' * ties: Prec@1 in [' in out
    assert (got[1], got[2]) == (r['prec'][1], r['prec'][5])
    for k, top in ((1, ref[1]), (5, ref[2])):                 # 8-image batches: the default path's fp32 percentages are exact
        assert r['sure'][k] <= top <= r['possible'][k], (k, top, r)
        if r['sure'][k] == r['possible'][k]:
            assert top == r['prec'][k], k
    assert abs(got[0] - ref[0]) <= 1e-5 * max(1.0, abs(ref[0]))      # fp64 loss against the default path's fp32 loss
    configs = [lists['q8'], lists['q4'], lists['qmix']]
    single = [H.validate(args, loader, model, None, dev, c, device_metrics=True) for c in configs]
    assert H.validate_many(args, loader, model, dev, configs) == single
    assert H.validate_many(args, loader, model, dev, [configs[1], configs[0], configs[1]]) == [single[1], single[0], single[1]]
    capsys.readouterr()


def test_sliced_forward_feeds_the_meter(dva, micro_quant):
    """one 64-image batch: the forward runs in slices on several streams; the meter, enqueued right behind it, sees the joined logits"""
    model, a, g = micro_quant
    H = dva.harness
    data, tgt = next(iter(H.SyntheticLoader(64, 64, a['img_size'], a['num_classes'], seed=9)))
    tgt[5], tgt[40] = -100, a['num_classes']
    m = dva.DeviceMeter()
    with torch.no_grad():
        out = model(data.cuda(), [8] * 10, False)[0]
    m.update(out, tgt.cuda())
    got = m.result()
    host = dva.DeviceMeter()
    host.update(out.cpu(), tgt)
    want = host.result()
    assert {k: v for k, v in got.items() if k != 'loss'} == {k: v for k, v in want.items() if k != 'loss'}
    assert got['n'] == 62 and got['invalid'] == 2
    assert abs(got['loss'] - want['loss']) <= loss_bound(10, want['loss']) + 64 * 2.0 ** -52 * abs(want['loss'])


def test_harness_flag_device_metrics(dva, capsys, monkeypatch):
    """--device-metrics through harness.main on DeiT-T: with --mixed the search scores its phases through validate_many (2 + iterations
    calls); with --uint8-input the default path's Prec@k lies in the printed [sure, possible] bracket and the run repeats bit for bit."""
    H = dva.harness
    calls = []
    many = H.validate_many
    monkeypatch.setattr(H, 'validate_many', lambda *a, **k: (calls.append(len(a[4])), many(*a, **k))[1])
    res = H.main(['--model', 'deit_tiny', '--quant', '--mixed', '--device-metrics', '--n-val', '16', '--val-batchsize', '16',
                  '--calib-batchsize', '2', '--search-pop', '4', '--search-iter', '1', '--search-max-configs', '8', '--search-slack', '1.6'])
    out = capsys.readouterr().out
    loss, top1, top5, best = res
    assert 'best mixed-precision configuration' in out and ' * ties: Prec@1 in [' in out
    assert len(calls) == 3 and calls[:2] == [5, 4], calls
    assert len(best) == 50 and set(best) <= {4, 8} and best[0] == 8 and 0.0 <= top1 <= top5 <= 100.0
    common = ['--model', 'deit_tiny', '--quant', '--uint8-input', '--n-val', '16', '--val-batchsize', '8', '--calib-batchsize', '2']
    ref = H.main(common)                                      # the default path on uint8 crops: torch's topk, fp32 loss
    capsys.readouterr()
    got = H.main(common + ['--device-metrics'])
    out = capsys.readouterr().out
    lo1, hi1, lo5, hi5 = (float(v) for v in re.search(r'ties: Prec@1 in \[([\d.]+), ([\d.]+)\] Prec@5 in \[([\d.]+), ([\d.]+)\]', out).groups())
    assert lo1 <= got[1] <= hi1 and lo5 <= got[2] <= hi5 and got[1] > 0.0
    assert lo1 <= ref[1] <= hi1 and lo5 <= ref[2] <= hi5, (ref, out)          # 8-image batches: multiples of 6.25, exact at 3 decimals
    assert abs(got[0] - ref[0]) <= 1e-5 * max(1.0, abs(ref[0]))
    assert H.main(common + ['--device-metrics']) == got                         # repeatable, loss bits included
    capsys.readouterr()
