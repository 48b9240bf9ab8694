"""GPU: the mixed-precision search on the product path.  The quantized micro-ViT on the engine scores a small walk (population 8, two
iterations) over 24 synthetic images in batches of 8, once per candidate through ``harness.validate`` and once per phase through
``harness.validate_many``; both walks must be the same, and every score must be the top-1 of the CPU oracle's logits
(``OracleViT.quant_forward``, which the engine equals bit for bit) for the same images, targets and ``bit_config``.

Tie rule.  The micro-ViT's ten logits lie on an int8 grid and tie often: of the few dozen configurations of this walk about every
third has an image whose target shares the maximum.  ``torch.topk``'s order among equal logits is no contract, so both runs score with
the harness's defined rule (``device_metrics=True``: among equal logits the lower class index ranks first), and the host side applies
the same rule to the oracle's logits with ``score_rows_reference``.  The default path (``harness.accuracy``, torch.topk) is checked for
every distinct configuration too: it must land in the [sure, possible] bracket of the oracle's logits, and on the value itself where
the bracket is one point."""
import contextlib
import io
from functools import partial

import numpy as np
import pytest
import torch

from conftest import gpu_ok, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

N_VAL, BATCH, LOADER_SEED = 24, 8, 3
# slack 1.5 on the micro-ViT's FLOPs: 12 of the 32 pair-tied candidates fit, and of the 44 children several break the size constraint
# or repeat a sibling (the test asserts at least three from the walk itself)
SEARCH = dict(seed=0, slack=1.5, pop_size=8, evo_iter=2)
N_CHILDREN = SEARCH['evo_iter'] * 22


def micro_setup(dva, device):
    """the calibrated micro-ViT of tests/golden/micro_vit.npz on ``device``, its FLOPs and weight distances, the oracle with the same
    calibration, the 24 images and their targets: the oracle's 8-bit top-1, for every third image the runner-up instead"""
    import p2vit_oracle as O
    H = dva.harness
    g = load_golden('micro_vit')
    a = dva.synth.ARCHS['micro']
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    model = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                                  num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                                  norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    model.load_state_dict(sd, strict=False)
    model = model.to(device).eval()
    _, flops, gd = H.calibrate_model(model, torch.from_numpy(g['x_cal']).to(device))
    orc = O.OracleViT(a, sd)
    orc.calib = model.export_calib()
    x = torch.cat([d for d, _ in H.SyntheticLoader(N_VAL, BATCH, a['img_size'], a['num_classes'], seed=LOADER_SEED)])
    order = orc.quant_forward(x, [8] * len(flops)).argsort(dim=1, descending=True, stable=True)
    tgt = order[torch.arange(N_VAL), (torch.arange(N_VAL) % 3 == 0).long()]
    loader = H.SyntheticLoader(N_VAL, BATCH, a['img_size'], a['num_classes'], seed=LOADER_SEED, targets=tgt)
    return dict(model=model, flops=flops, gd=gd, orc=orc, x=x, tgt=tgt, loader=loader)


def oracle_top1(dva, s, cfg):
    """(top-1 under the defined tie rule, sure, possible) in percent, from the oracle's logits"""
    rr, _ = dva.score_rows_reference(s['orc'].quant_forward(s['x'], [int(b) for b in cfg]), s['tgt'])
    gt, lo, hi = (rr[:, c].astype(np.int64) for c in range(3))
    assert (gt >= 0).all()
    return tuple(100.0 * int(hit.sum()) / N_VAL for hit in (gt + lo < 1, gt + lo + hi < 1, gt < 1))


def run_walks(dva, s, one, many):
    """the search with ``one(cfg) -> score`` per candidate, then with ``many(cfgs) -> scores`` per phase"""
    S = dva.search
    seq, batches = [], []

    def score(cfg):
        seq.append(tuple(cfg))
        return one(cfg)

    def score_many(cfgs):
        batches.append([tuple(c) for c in cfgs])
        return many(cfgs)

    def never(cfg):
        raise AssertionError('score_fn called although score_many was given')

    kw = dict(log=lambda *a: None, **SEARCH)
    r1, p1 = S.mixed_precision_search(score, s['flops'], s['gd'], **kw)
    r2, p2 = S.mixed_precision_search(never, s['flops'], s['gd'], score_many=score_many, **kw)
    return dict(r1=r1, p1=p1, r2=r2, p2=p2, seq=seq, batches=batches)


@pytest.fixture(scope='module')
def walk():
    import diff_vit_amd as dva
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    dva.engine.lib()
    H = dva.harness
    dev = torch.device('cuda:0')
    s = micro_setup(dva, dev)
    args = H.build_parser().parse_args(['--print-freq', str(10 ** 9)])
    scores = {}

    def one(cfg):
        with contextlib.redirect_stdout(io.StringIO()):
            v = H.validate(args, s['loader'], s['model'], None, dev, cfg, device_metrics=True)[1]
        assert scores.setdefault(tuple(cfg), v) == v, 'one configuration, two scores'
        return v

    def many(cfgs):
        out = [r[1] for r in H.validate_many(args, s['loader'], s['model'], dev, cfgs)]
        for c, v in zip(cfgs, out):
            assert scores.setdefault(tuple(c), v) == v, 'validate and validate_many disagree on %s' % (c,)
        return out

    w = run_walks(dva, s, one, many)
    w.update(dva=dva, s=s, scores=scores, args=args, dev=dev)
    return w


def test_both_walks_are_one_walk(walk):
    w = walk
    assert w['r1'] == w['r2'] and w['p1'] == w['p2']
    assert [c for b in w['batches'] for c in b] == w['seq']
    n_pop = min(SEARCH['pop_size'], len(w['r1']))
    assert len(w['batches']) == 2 + SEARCH['evo_iter'] and len(w['batches'][0]) == 5 and len(w['batches'][1]) == n_pop == 8
    rejected = N_CHILDREN - (len(w['seq']) - 5 - n_pop)
    print('rejected children: %d of %d; validate calls %d, distinct configurations %d' % (rejected, N_CHILDREN, len(w['seq']), len(set(w['seq']))))
    assert rejected >= 3
    S, s = w['dva'].search, w['s']
    constraint = SEARCH['slack'] * sum(4 * f for f in s['flops'])
    assert all(len(c) == len(s['flops']) and set(c) <= {4, 8} and not S.model_size(s['flops'], c) > constraint for c in w['seq'])
    assert len(w['p1']) == 8 and [p[1] for p in w['p1']] == sorted((p[1] for p in w['p1']), reverse=True)


def test_every_score_is_the_oracles_top1(walk):
    w = walk
    distinct = list(dict.fromkeys(w['seq']))
    assert set(distinct) == set(w['scores']) and 8 < len(distinct) <= 5 + 8 + N_CHILDREN
    want = {c: oracle_top1(w['dva'], w['s'], c) for c in distinct}
    bad = [(c, w['scores'][c], want[c][0]) for c in distinct if w['scores'][c] != want[c][0]]
    assert not bad, bad[:4]
    assert len({v[0] for v in want.values()}) >= 3, 'the scores do not tell the configurations apart'
    # the default path (harness.accuracy: torch.topk, fp32 percentages of 8-image batches, exact) inside the oracle's bracket
    H, s = w['dva'].harness, w['s']
    crit = torch.nn.CrossEntropyLoss().to(w['dev'])
    for c in distinct:
        with contextlib.redirect_stdout(io.StringIO()):
            top1 = H.validate(w['args'], s['loader'], s['model'], crit, w['dev'], list(c))[1]
        _, sure, possible = want[c]
        assert sure <= top1 <= possible, (c, top1, want[c])
