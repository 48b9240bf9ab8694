"""Mixed-precision bit-width search on top of the fast quantized forward.

Counterpart of the inline search in the reference driver (test_quant.py:253-408): Pareto-style sampling of 4/8-bit
configurations under a model-size constraint, ranking by Omega = sum_i hessian_i * distance_i, validation of the best
five, then an evolutionary search (population 25, 8 iterations, 10 mutations + 10 crossovers per iteration) scored by
top-1 from ``validate``.  Every candidate is one ``model(data, bit_config)`` sweep -- thousands of forwards with a
different ``bit_config`` per call, which the engine serves from the per-bit weight copies of the frozen plan.

Kept from the reference, on purpose (same walk for the same ``random`` seed and the same scores):
  * candidates tie the two layers of each pair: ``[8] + [b for b in cfg for _ in range(2)] + [choice]`` (:269-273);
  * Omega indexes ``global_distance[i-1][k]`` with k = index of the bit in ``bit_choice`` = {0, 1}, i.e. it reads the
    uint3/uint4 weight MSEs of the calibration bookkeeping (models/ptq/layers.py:151-170), not int4/int8 (:293-296);
  * a rejected mutation/crossover child is still appended with the score of the configuration validated last before it
    (:369-373, :390-394).  ``val_prec1`` is one variable of main(): into iteration 0 it carries the score of the last member of the
    initial population in Omega order, ``omega_list[pop_size-1]``, taken BEFORE the population is sorted (:348-353) -- not the best
    score -- and into every later iteration the score in force at the end of the one before.
One deliberate deviation: the crossover loop leaves when the population has fewer than two members (``len(parent) < 2``).  The
reference draws two parents until they differ and never returns from a population of one; the exit consumes no ``random`` draw the
reference would have survived to make.
The walk is pinned to the reference's own statements: oracle/gen_golden_search.py executes them with stubs and records them in
tests/golden/search_walk.npz, tests/test_search.py replays every record exactly, sequentially and through ``score_many``.
The per-layer Hessian sensitivities (``mean_hessian``; pyhessian in the reference, out of scope here, and undefined as
shipped: test_quant.py:186) are an input; uniform sensitivities reduce Omega to the summed weight distance.
"""
import random


def synthetic_score(bit_config, step=0.0):
    """the stand-in for top-1 that the recorded walks of tests/golden/search_walk.npz were scored with (oracle/gen_golden_search.py and
    tests/test_search.py share it): more 8-bit layers late in the network -> higher.  ``step`` > 0 rounds down to multiples of it, as
    top-1 over ``n`` images is a multiple of 100 / n (6.25 at 16 images): ties then decide the population's cut and the stable sorts."""
    s = sum((i + 1) * (b == 8) for i, b in enumerate(bit_config)) / 10.0
    return s // step * step if step else s


def model_size(FLOPs, bit_config):
    return sum(FLOPs[i] * bit_config[i] for i in range(len(FLOPs)))


def pareto_candidates(FLOPs, n_layers_gd, rng, bit_choice=(4, 8), max_configs=50, slack=1.1, ties=None):
    """test_quant.py:262-284.  ``ties`` None: the reference's walk (the conv at the widest choice, the layers behind it tied in pairs, the
    head alone).  Otherwise a list of index groups: each group draws ONE bit, the groups in ascending order of their first index, and an
    index in no group stays at 8 (Swin: ``SwinTransformer.search_ties``)."""
    bit_choice = list(bit_choice)
    constraint = slack * sum(FLOPs[i] * 4 for i in range(len(FLOPs)))
    bit_list = []
    if ties is not None:
        ties = sorted((sorted(g) for g in ties), key=lambda g: g[:1])
        seen = [i for g in ties for i in g]
        if not all(ties) or len(set(seen)) != len(seen) or min(seen, default=0) < 0 or max(seen, default=0) >= len(FLOPs):
            raise ValueError('ties must be disjoint, non-empty groups of layer indices below %d' % len(FLOPs))
    for _ in range(2 ** min(n_layers_gd, 24)):
        if ties is None:
            cfg = [rng.choice(bit_choice) for _ in range(len(FLOPs) // 2 - 1)]
            new = [max(bit_choice)] + [b for b in cfg for _ in range(2)] + [rng.choice(bit_choice)]
        else:
            new = [8] * len(FLOPs)
            for g in ties:
                b = rng.choice(bit_choice)
                for i in g:
                    new[i] = b
        if not model_size(FLOPs, new) > constraint and new not in bit_list:
            bit_list.append(new)
        if len(bit_list) > max_configs:
            break
    return bit_list, constraint


def omega_rank(bit_list, global_distance, mean_hessian, bit_choice=(4, 8)):
    """test_quant.py:286-318: [[bit_config, omega], ...] sorted by omega."""
    bit_choice = list(bit_choice)
    out = []
    for cfg in bit_list:
        sel = []
        for i, bit in enumerate(cfg):
            if i == 0:
                continue
            for k, choice in enumerate(bit_choice):
                if choice == bit:
                    sel.append(global_distance[i - 1][k])
                    break
        omega = [mean_hessian[i] * sel[i] for i in range(len(cfg) - 1)]
        out.append([cfg, float(sum(omega))])
    out.sort(key=lambda x: x[-1])
    return out


class _Pending:
    """scores of one phase: ``score_fn`` at once, or (``score_many``) collected and resolved by one call in ``resolve``"""

    def __init__(self, score_fn, score_many):
        self.score_fn, self.score_many, self.cfgs = score_fn, score_many, []

    def __call__(self, cfg):
        if self.score_many is None:
            return self.score_fn(cfg)
        self.cfgs.append(cfg)
        return self                                    # placeholder: replaced in resolve()

    def resolve(self, entries, val):
        """``entries``: [config, score or placeholder or None] in generation order; None = rejected child, which carries the score
        in force before it (test_quant.py:369-373, :390-394).  Returns the score in force after the last entry."""
        scores = iter(self.score_many(self.cfgs) if self.score_many is not None else ())
        for e in entries:
            if e[1] is self:
                e[1] = next(scores)
            elif e[1] is None:
                e[1] = val
            val = e[1]
        self.cfgs = []
        return val


def evolutionary_search(score_fn, omega_list, FLOPs, constraint, rng, bit_choice=(4, 8), pop_size=25, evo_iter=8,
                        mutate_size=10, mutate_prob=0.5, crossover_size=10, crossover_prob=0.5, log=print, score_many=None):
    """test_quant.py:340-408.  ``score_fn(bit_config) -> top-1``.  ``score_many(list of bit_configs) -> list of scores`` (optional):
    the initial population, and then each iteration's mutation and crossover children together, are scored by ONE call.  Within such a
    phase nothing the ``random`` walk consumes depends on a score (the parents stay as they are until all children of the iteration
    exist), so the configurations are generated first, scored together, and the scores assigned afterwards: same seed and same score
    function give the same population as the sequential path."""
    bit_choice = list(bit_choice)
    score = _Pending(score_fn, score_many)
    parent = [[omega_list[i][0], score(omega_list[i][0])] for i in range(min(pop_size, len(omega_list)))]
    val = score.resolve(parent, 0.0)                   # val_prec1 of the LAST validated member, before the sort (:348-353)
    parent.sort(key=lambda x: x[-1], reverse=True)
    for evo in range(evo_iter):
        children, seen = [], []
        while True:
            old = rng.choice(parent)[0]
            new = [b if rng.random() < mutate_prob else rng.choice(bit_choice) for b in old]
            children.append([new, score(new) if not model_size(FLOPs, new) > constraint and new not in seen else None])
            seen.append(new)
            if len(seen) > mutate_size:
                break
        seen = []
        while True:
            a, b = rng.choice(parent)[0], rng.choice(parent)[0]
            if a == b:
                if len(parent) < 2:
                    break
                continue
            new = [x if rng.random() < crossover_prob else y for x, y in zip(a, b)]
            children.append([new, score(new) if not model_size(FLOPs, new) > constraint and new not in seen else None])
            seen.append(new)
            if len(seen) > crossover_size:
                break
        val = score.resolve(children, val)
        for child in children:
            if child[1] > parent[-1][1]:
                parent.append(child)
        parent.sort(key=lambda x: x[-1], reverse=True)
        parent = parent[:pop_size]
        log('Evolotionary iteration: ', evo)
    return parent


def mixed_precision_search(score_fn, FLOPs, global_distance, mean_hessian=None, seed=0, log=print, score_many=None, ties=None, **kw):
    """the whole block test_quant.py:253-408; returns (pareto-ranked list, final population).  ``score_many``: see
    ``evolutionary_search``; the top-5 validation is one call of it as well.  ``ties``: see ``pareto_candidates``."""
    assert len(FLOPs) - 1 == len(global_distance)
    if mean_hessian is None:
        mean_hessian = [1.0] * len(global_distance)
    assert len(mean_hessian) == len(global_distance)
    rng = random.Random(seed)
    log('Pareto Frontier.......')
    pk = {k: v for k, v in kw.items() if k in ('max_configs', 'slack')}
    bit_list, constraint = pareto_candidates(FLOPs, len(global_distance), rng, ties=ties, **pk)
    ranked = omega_rank(bit_list, global_distance, mean_hessian)
    log('Hessien-Based Validating...')
    for i in range(min(5, len(ranked))):
        log(ranked[i][0])
        if score_many is None:
            score_fn(ranked[i][0])
    if score_many is not None:
        score_many([ranked[i][0] for i in range(min(5, len(ranked)))])
    log('Start Evolutionary.......')
    evo = {k: v for k, v in kw.items() if k in ('pop_size', 'evo_iter', 'mutate_size', 'mutate_prob', 'crossover_size', 'crossover_prob')}
    return ranked, evolutionary_search(score_fn, ranked, FLOPs, constraint, rng, log=log, score_many=score_many, **evo)
