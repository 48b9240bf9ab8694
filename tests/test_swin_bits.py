"""CPU: the per-layer bit-list surface of the Swin models - names, length, errors, layer_macs, global_distance - the tied candidate walk
of the search, and the MIXED oracle (tests/_swin_bits_ref.py) the GPU tests compare the engine against."""
import random

import pytest
import torch

import _swin_bits_ref as R


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def micro(dva):
    return R.micro_swin(dva)


def test_names_length_and_macs(dva):
    from diff_vit_amd import swin
    m = swin.swin_micro_patch4_window7_56(num_classes=10)
    names = m.bit_config_names()
    blocks = ['attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2']
    want = (['patch_embed.proj'] + ['layers.0.blocks.%d.%s' % (b, k) for b in range(2) for k in blocks] + ['layers.0.downsample.reduction'] +
            ['layers.1.blocks.%d.%s' % (b, k) for b in range(2) for k in blocks] + ['head'])
    assert names == want == [n for n, _ in m.linear_modules()]
    assert m.bit_config_length() == len(names) == 19
    # hand count: 14 x 14 tokens of 64 channels, then 7 x 7 tokens of 128; 4 x 4 x 3 = 48 inputs per patch; 10 classes
    T0, T1 = 196, 49
    blk = lambda T, C: [T * C * 3 * C, T * C * C, T * C * 4 * C, T * 4 * C * C]
    assert m.layer_macs() == [T0 * 48 * 64] + blk(T0, 64) * 2 + [T1 * 256 * 128] + blk(T1, 128) * 2 + [128 * 10]
    assert swin.swin_tiny_patch4_window7_224().bit_config_length() == 53
    b = swin.swin_base_patch4_window7_224()
    macs = b.layer_macs()
    assert b.bit_config_length() == len(macs) == len(b.bit_config_names()) == 101
    assert sum(macs) == 15126077440 and sum(macs[1:-1]) == 15105785856          # "linear 15 105.79 M"
    assert swin.swin_large_patch4_window12_384().bit_config_length() == 101


def test_bit_list_errors(micro):
    m, x = micro
    L = m.bit_config_length()
    with torch.no_grad():
        for bad in ([8] * (L - 1), [8] * (L + 1), [], [8] * (L - 1) + [6], [0] + [8] * (L - 1), [8] * (L - 1) + [16]):
            with pytest.raises(ValueError):
                m(x, bits=bad)
            with pytest.raises(ValueError):
                m.forward_uint8(torch.zeros(1, 56, 56, 3, dtype=torch.uint8), bits=bad)
        with pytest.raises(NotImplementedError):
            m(x, bits=[8] * (L - 1) + [-1])
        with pytest.raises(ValueError):                  # (the length is checked first)
            m(x, bits=[-1])
        with pytest.raises(RuntimeError):                # a good list reaches the engine, which has no CPU path
            m(x, bits=[8] * L)


def test_global_distance(dva, micro):
    m, x = micro
    gd = m.global_distance
    assert len(gd) == m.bit_config_length() - 1 == 18
    assert all(len(e) == len(gd[0]) >= 2 for e in gd)
    m2, _ = R.micro_swin(dva)
    m2.model_dequant()
    with torch.no_grad():
        out, flops, dist = dva.harness._forward(m2, x[:1], None)            # float state: nothing is collected
        assert flops == m2.layer_macs() and dist is m2.global_distance and len(dist) == 18
        # a second calibration starts the list again, and the harness hands it out with the MACs
        out, flops, dist = dva.harness.calibrate_model(m2, x[:2])
    assert flops == m2.layer_macs() and dist is m2.global_distance and len(dist) == 18
    assert all(len(e) == len(gd[0]) and all(float(v) >= 0.0 for v in e) for e in dist)
    # a QLinear called without a list (the op-by-op graph of other tests) does not reach the model's list
    with torch.no_grad():
        m2.model_dequant(); m2.model_open_calibrate(); m2.head(torch.zeros(1, m2.num_features)); m2.model_close_calibrate()
    assert len(m2.global_distance) == 0


def _reference_walk(FLOPs, n_layers_gd, rng, bit_choice=(4, 8), max_configs=50, slack=1.1):
    """the candidate walk as it was before ``ties`` existed"""
    bit_choice = list(bit_choice)
    constraint = slack * sum(f * 4 for f in FLOPs)
    bit_list = []
    for _ in range(2 ** min(n_layers_gd, 24)):
        cfg = [rng.choice(bit_choice) for _ in range(len(FLOPs) // 2 - 1)]
        new = [max(bit_choice)] + [b for b in cfg for _ in range(2)] + [rng.choice(bit_choice)]
        if not sum(f * b for f, b in zip(FLOPs, new)) > constraint and new not in bit_list:
            bit_list.append(new)
        if len(bit_list) > max_configs:
            break
    return bit_list, constraint


def test_ties_none_is_the_reference_walk(dva):
    from diff_vit_amd import search
    FLOPs = [3, 5, 5, 7, 7, 5, 5, 7, 7, 2]
    for seed in (0, 7):
        a, b = random.Random(seed), random.Random(seed)
        got = search.pareto_candidates(FLOPs, 9, a, max_configs=20, slack=1.6)
        assert got == _reference_walk(FLOPs, 9, b, max_configs=20, slack=1.6)
        assert a.random() == b.random()                   # the same consumption of the generator
        assert len(got[0]) > 5


def test_swin_ties(dva):
    from diff_vit_amd import search, swin
    m = swin.swin_tiny_patch4_window7_224()
    names, ties, macs = m.bit_config_names(), m.search_ties(), m.layer_macs()
    L = len(names)
    assert sorted(i for g in ties for i in g) == list(range(1, L))            # index 0 is in no group
    for g in ties:
        kinds = [names[i].rsplit('.', 1)[-1] for i in g]
        assert kinds in (['qkv', 'proj'], ['fc1', 'fc2'], ['reduction'], ['head']), kinds
        assert len(g) == 1 or names[g[0]].rsplit('.', 2)[0] == names[g[1]].rsplit('.', 2)[0]      # of ONE block
    cands, constraint = search.pareto_candidates(macs, L - 1, random.Random(3), max_configs=30, slack=1.5, ties=ties)
    assert len(cands) == 31
    for c in cands:
        assert len(c) == L and c[0] == 8 and set(c) <= {4, 8}
        assert all(len({c[i] for i in g}) == 1 for g in ties)
        assert search.model_size(macs, c) <= constraint
    assert len({tuple(c) for c in cands}) == len(cands)
    # groups draw in ascending order of their first index, one bit each
    r = random.Random(11)
    one, _ = search.pareto_candidates(macs, L - 1, random.Random(11), max_configs=0, slack=2.0, ties=list(reversed(ties)))
    want = [8] * L
    for g in sorted(ties, key=lambda g: g[0]):
        b = r.choice([4, 8])
        for i in g:
            want[i] = b
    assert one == [want]
    with pytest.raises(ValueError):
        search.pareto_candidates(macs, L - 1, random.Random(0), ties=[[1, 2], [2, 3]])


def test_mixed_precision_search_on_swin_tiny(dva):
    from diff_vit_amd import search, swin
    m = swin.swin_tiny_patch4_window7_224()
    macs, ties, L = m.layer_macs(), m.search_ties(), m.bit_config_length()
    gd = [[0.4, 0.1] for _ in range(L - 1)]
    seen = []

    def score(cfg):                                        # more bits, more "accuracy"
        seen.append(list(cfg))
        return sum(cfg) / (8.0 * L)
    ranked, pop = search.mixed_precision_search(score, macs, gd, seed=2, log=lambda *a: None, ties=ties, max_configs=12, slack=1.5,
                                                pop_size=6, evo_iter=2, mutate_size=3, crossover_size=3)
    assert len(ranked) == 13 and all(len(c) == L and c[0] == 8 for c, _ in ranked)
    assert all(all(len({c[i] for i in g}) == 1 for g in ties) for c, _ in ranked)
    assert [o for _, o in ranked] == sorted(o for _, o in ranked)
    assert 1 <= len(pop) <= 6 and pop[0][1] == max(p[1] for p in pop)
    assert all(len(c) == L for c in seen)


def test_mixed_oracle(dva, micro):
    """the substituted oracle IS the uniform oracle at [4] * L and [8] * L, and every single-4 list moves the logits: the GPU test that
    compares the engine with it can tell every layer's width apart"""
    m, x = micro
    L = m.bit_config_length()
    o8, o4 = R.uniform_oracle(m, x, 8), R.uniform_oracle(m, x, 4)
    assert torch.equal(R.mixed_oracle(m, x, [8] * L), o8)
    assert torch.equal(R.mixed_oracle(m, x, [4] * L), o4)
    for i in range(L):
        assert not torch.equal(R.mixed_oracle(m, x, [4 if j == i else 8 for j in range(L)]), o8), m.bit_config_names()[i]
