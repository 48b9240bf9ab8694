"""CPU: the mixed-precision search loop (counterpart of test_quant.py:253-408) with a synthetic score function: properties, and the
walk itself against tests/golden/search_walk.npz.  The reference's loop is inline in main() and cannot be imported, so
oracle/gen_golden_search.py executed its statements with stubs and recorded, per (seed, slack, score, sensitivities) case, the
constraint, the ranked candidates with their omegas, every validated configuration in call order and the final population."""
import functools
import random

import numpy as np
import pytest

from conftest import load_golden

N_CASES = 14                              # what oracle/gen_golden_search.py writes: 5 seeds x 2 slacks, 2 coarse-score, 2 non-uniform-Hessian


def _setup():
    import diff_vit_amd as dva
    m = dva.deit_tiny_patch16_224(cfg=dva.Config())
    flops = m.flops()
    rng = random.Random(1)
    gd = [[rng.random() * 0.1 + 0.2, rng.random() * 0.05 + 0.05, rng.random() * 0.04 + 0.04, rng.random() * 0.001] for _ in range(len(flops) - 1)]
    return dva, flops, gd


def test_pareto_and_omega():
    dva, flops, gd = _setup()
    S = dva.search
    bit_list, constraint = S.pareto_candidates(flops, len(gd), random.Random(0), slack=1.6, max_configs=40)
    assert len(bit_list) == 41 and all(len(c) == 50 and c[0] == 8 for c in bit_list)
    assert all(S.model_size(flops, c) <= constraint for c in bit_list)
    assert all(c[1 + 2 * j] == c[2 + 2 * j] for c in bit_list for j in range(24))       # layer pairs tied
    ranked = S.omega_rank(bit_list, gd, [1.0] * len(gd))
    assert [r[1] for r in ranked] == sorted(r[1] for r in ranked)
    # index quirk: bit 4 reads distance column 0, bit 8 column 1
    c = ranked[0][0]
    assert abs(ranked[0][1] - sum(gd[i - 1][0 if c[i] == 4 else 1] for i in range(1, 50))) < 1e-9


def test_evolution_is_deterministic_and_monotone():
    dva, flops, gd = _setup()
    calls = []

    def score(cfg):                       # more 8-bit layers late in the network -> higher "accuracy"
        calls.append(tuple(cfg))
        return sum((i + 1) * (b == 8) for i, b in enumerate(cfg)) / 10.0

    r1, p1 = dva.search.mixed_precision_search(score, flops, gd, seed=3, log=lambda *a: None, evo_iter=3, slack=1.6, max_configs=40)
    n1 = len(calls)
    r2, p2 = dva.search.mixed_precision_search(score, flops, gd, seed=3, log=lambda *a: None, evo_iter=3, slack=1.6, max_configs=40)
    assert p1 == p2 and r1 == r2 and len(calls) == 2 * n1
    assert len(p1) == 25 and [x[1] for x in p1] == sorted((x[1] for x in p1), reverse=True)
    assert p1[0][1] >= max(score(c[0]) for c in r1[:25]) - 1e-9
    assert n1 >= 5 + 25 + 3                # top-5 validation, initial population, children


@functools.lru_cache(maxsize=None)
def _cases():
    g = load_golden('search_walk')
    n = int(g['n_cases'])
    flops, gd = [int(f) for f in g['flops']], [[float(v) for v in row] for row in g['global_distance']]
    return flops, gd, [{k.split('/', 1)[1]: g[k] for k in g.files if k.startswith('case%02d/' % i)} for i in range(n)]


def test_recorded_cases_are_all_there():
    """the inputs of the record are those of ``_setup``; no case is missing, and the record holds what makes it a test of the walk: a
    rejected first child (which carries the score of the last initial member into the population) and coarse scores"""
    dva, flops, gd = _setup()
    rflops, rgd, cases = _cases()
    assert len(cases) == N_CASES and all(len(c) == 13 for c in cases)
    assert sum(k.startswith('case') for k in load_golden('search_walk').files) == 13 * N_CASES
    for c in cases:                       # per call: (phase, index in it); phase -2 the validated five, -1 the initial population, else the iteration
        where = [tuple(w) for w in c['where'].tolist()]
        assert len(where) == len(c['calls']) and where[:30] == [(-2, i) for i in range(5)] + [(-1, i) for i in range(25)]
        assert where[30:] == sorted(where[30:]) and all(0 <= e < 8 and 0 <= i < 22 for e, i in where[30:])
        assert bool(c['first_rejected']) == ((0, 0) not in where) and int(c['n_rejected']) == 8 * 22 - len(where[30:])
    assert rflops == [int(f) for f in flops] and rgd == gd
    assert {(int(c['seed']), float(c['slack'])) for c in cases} >= {(s, sl) for s in range(5) for sl in (1.6, 1.2)}
    for sl in (1.6, 1.2):
        assert any(float(c['slack']) == sl and float(c['step']) == 6.25 for c in cases)
        assert any(float(c['slack']) == sl and len(set(c['mean_hessian'].tolist())) > 1 for c in cases)
    assert sum(bool(c['first_rejected']) for c in cases) >= 4 and all(len(c['ranked']) >= 25 for c in cases)


@pytest.mark.parametrize('batched', [False, True], ids=['sequential', 'score_many'])
@pytest.mark.parametrize('case', range(N_CASES))
def test_walk_equals_the_reference_record(case, batched):
    """exact: integer lists, and omegas that are Python float sums formed in the same list order on both sides"""
    import diff_vit_amd as dva
    S = dva.search
    flops, gd, cases = _cases()
    c = cases[case]
    step, what = float(c['step']), (case, int(c['seed']), float(c['slack']))
    calls, batches = [], []

    def score(cfg):
        calls.append([int(b) for b in cfg])
        return S.synthetic_score(cfg, step)

    def many(cfgs):
        batches.append(len(cfgs))
        return [score(cfg) for cfg in cfgs]

    def never(cfg):
        raise AssertionError('score_fn called although score_many was given')

    kw = dict(mean_hessian=c['mean_hessian'].tolist(), seed=int(c['seed']), slack=float(c['slack']), log=lambda *a: None)
    if batched:
        ranked, pop = S.mixed_precision_search(never, flops, gd, score_many=many, **kw)
        assert len(batches) == 2 + 8 and batches[:2] == [5, 25] and sum(batches) == len(calls), (what, batches)
    else:
        ranked, pop = S.mixed_precision_search(score, flops, gd, **kw)
    assert S.pareto_candidates(flops, len(gd), random.Random(int(c['seed'])), slack=float(c['slack']))[1] == float(c['constraint']), what
    assert [r[0] for r in ranked] == c['ranked'].tolist(), what
    omega = c['omega'].tolist()
    assert [r[1] for r in ranked] == omega, (what, [i for i, r in enumerate(ranked) if r[1] != omega[i]])
    rec = c['calls'].tolist()
    first = next((i for i, (a, b) in enumerate(zip(calls, rec)) if a != b), min(len(calls), len(rec)))
    assert calls == rec, (what, 'validate calls: %d, reference %d, first difference at call %d' % (len(calls), len(rec), first))
    assert [p[0] for p in pop] == c['pop'].tolist() and [p[1] for p in pop] == c['pop_score'].tolist(), what
    assert 8 * 22 - (len(calls) - 30) == int(c['n_rejected']), what
