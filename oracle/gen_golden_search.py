"""Generate tests/golden/search_walk.npz by RUNNING THE REAL REFERENCE's mixed-precision search: the body of the ``if args.mixed:``
statement of /root/reference/test_quant.py that prints "Pareto Frontier" (Pareto sampling, Omega ranking, the validation of the best
five and the evolutionary loop).  The loop is inline in main() and cannot be imported, so the statement is located in the parsed file
by its AST position, its body is compiled from the tree and executed with stubs for everything around it.

Run once in the build container:   python oracle/gen_golden_search.py

Nothing of the reference's text is stored: it is read when this recipe runs.  Stored are the inputs (FLOPs, global_distance,
mean_hessian, seed, slack, score step) and what the loop did with them: the constraint, the ranked configurations and their omegas,
every validated configuration in call order, the final population, the number of rejected children and whether the first child of
iteration 0 was rejected.

One constant of the block is replaced before compiling: the size constraint factor 1.1 becomes the name SLACK.  With DeiT-T's FLOPs
a random candidate almost never satisfies 1.1, and the 2**len(global_distance) sampling loop does not end.

Stubs: ``random`` is the module, seeded with random.seed(seed) (search.py's random.Random(seed) is the same generator); ``validate``
records the configuration and returns (0.0, score(cfg), 0.0) with search.synthetic_score; ``print`` does nothing.
"""
import ast
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference/test_quant.py'
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COARSE = 6.25                      # top-1 over 16 validation images
# (seed, slack, score step, seed of the non-uniform mean_hessian or None)
CASES = [(s, sl, 0.0, None) for s in range(5) for sl in (1.6, 1.2)]
CASES += [(5, sl, COARSE, None) for sl in (1.6, 1.2)]
CASES += [(6, sl, 0.0, 60 + i) for i, sl in enumerate((1.6, 1.2))]


def reference_block():
    """code object of the search block, the constraint factor replaced by the name SLACK"""
    with open(REF) as f:
        src = f.read()
    found = []
    for node in ast.walk(ast.parse(src)):
        if not isinstance(node, ast.If):
            continue
        t = node.test
        if not (isinstance(t, ast.Attribute) and t.attr == 'mixed' and isinstance(t.value, ast.Name) and t.value.id == 'args'):
            continue
        if 'Pareto Frontier' in ast.get_source_segment(src, node):
            found.append(node)
    assert len(found) == 1, 'expected one `if args.mixed:` with the Pareto print, found %d' % len(found)
    replaced = []

    class Slack(ast.NodeTransformer):
        def visit_Constant(self, c):
            if isinstance(c.value, float) and c.value == 1.1:
                replaced.append(c)
                return ast.copy_location(ast.Name(id='SLACK', ctx=ast.Load()), c)
            return c

    mod = ast.Module(body=[Slack().visit(s) for s in found[0].body], type_ignores=[])
    assert len(replaced) == 1, 'expected the constraint factor 1.1 once, found %d' % len(replaced)
    return compile(ast.fix_missing_locations(mod), REF, 'exec')


def inputs():
    """DeiT-T FLOPs and the global_distance of tests/test_search.py::_setup"""
    import diff_vit_amd as dva
    flops = dva.deit_tiny_patch16_224(cfg=dva.Config()).flops()
    rng = random.Random(1)
    gd = [[rng.random() * 0.1 + 0.2, rng.random() * 0.05 + 0.05, rng.random() * 0.04 + 0.04, rng.random() * 0.001] for _ in range(len(flops) - 1)]
    return dva, [int(f) for f in flops], gd


def run_case(code, score, flops, gd, seed, slack, step, hseed):
    n = len(gd)
    hrng = random.Random(hseed)
    mh = [1.0] * n if hseed is None else [hrng.random() for _ in range(n)]
    calls, where = [], []
    env = {}

    def validate(args, val_loader, model, criterion, device, bit_config=None):
        calls.append([int(b) for b in bit_config])
        # phase: -2 the five of the Hessian-based validation, -1 the initial population, else the iteration; and the child's index in it
        if 'children_list' in env:
            where.append((env['evo'], len(env['children_list'])))
        else:
            where.append((-1 if 'parent_popu' in env else -2, len(calls) - 1 - (5 if 'parent_popu' in env else 0)))
        return 0.0, score(bit_config, step), 0.0

    env.update(SLACK=slack, FLOPs=list(flops), global_distance=[list(r) for r in gd], mean_hessian=list(mh), random=random, validate=validate,
               print=lambda *a, **k: None, args=None, val_loader=None, model=None, criterion=None, device=None, torch=None)
    random.seed(seed)
    exec(code, env)
    ranked, pop = env['omega_list'], env['parent_popu']
    n_children = env['evo_iter'] * (env['mutate_size'] + 1 + env['crossover_size'] + 1)
    n_rejected = n_children - sum(1 for p, _ in where if p >= 0)
    return dict(seed=seed, slack=slack, step=step, mean_hessian=np.asarray(mh, np.float64), constraint=np.float64(env['model_constraint']),
                ranked=np.asarray([r[0] for r in ranked], np.int8), omega=np.asarray([r[1] for r in ranked], np.float64),
                calls=np.asarray(calls, np.int8), where=np.asarray(where, np.int16),
                pop=np.asarray([p[0] for p in pop], np.int8), pop_score=np.asarray([p[1] for p in pop], np.float64),
                n_rejected=n_rejected, first_rejected=(0, 0) not in where)


def tie_at_cut(case, score):
    """a validated configuration outside the final population scores exactly what the population's last member does: the strict
    ``child[1] > parent_popu[-1][1]`` or the stable sort before the cut decided between equals"""
    pop = {tuple(c) for c in case['pop'].tolist()}
    low = float(case['pop_score'][-1])
    return any(tuple(c) not in pop and score(c, float(case['step'])) == low for c in case['calls'].tolist())


def main():
    dva, flops, gd = inputs()
    score = dva.search.synthetic_score
    code = reference_block()
    out = {'flops': np.asarray(flops, np.int64), 'global_distance': np.asarray(gd, np.float64), 'n_cases': np.int64(len(CASES))}
    cases = []
    for i, (seed, slack, step, hseed) in enumerate(CASES):
        c = run_case(code, score, flops, gd, seed, slack, step, hseed)
        cases.append(c)
        for k, v in c.items():
            out['case%02d/%s' % (i, k)] = np.asarray(v)
        print('case %2d seed %d slack %.1f step %.2f hessian %s: %d ranked, %d validate calls, %d rejected children, first child rejected: %s'
              % (i, seed, slack, step, hseed, len(c['ranked']), len(c['calls']), c['n_rejected'], c['first_rejected']))
    assert all(len(c['ranked']) >= 25 for c in cases), 'the reference indexes omega_list[i] for 25'
    assert all(c['pop'].shape == (25, len(flops)) and c['calls'].shape[1] == len(flops) for c in cases)
    assert sum(bool(c['first_rejected']) for c in cases) >= 4, 'too few cases with a rejected first child'
    ties = [i for i, c in enumerate(cases) if c['step'] and tie_at_cut(c, score)]
    assert ties, 'no coarse case has a tie at the cut of the population'
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, 'search_walk.npz')
    np.savez_compressed(path, **out)
    print('search_walk: wrote %d cases, %d arrays, %d bytes; coarse cases with a tie at the cut: %s' % (len(cases), len(out), os.path.getsize(path), ties))


if __name__ == '__main__':
    main()
