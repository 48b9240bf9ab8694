"""tests/golden/profiling_micro.npz from the REAL reference's black-box profiling-input generator
(dataset_utility.gen_profiling_inputs_in_blackbox, dataset_utility.py:209-302) on the micro-ViT of tests/golden/micro_vit.npz.  Runs
where the reference tree is importable (oracle/gen_golden.py::import_reference, which also makes ``Tensor.cuda`` the identity: the
reference moves everything to a GPU); stores inputs and results only.

    python tools/gen_golden_profiling.py

dataset_utility imports torchvision for its loaders, which nothing here calls: empty stand-in modules are enough; scipy is the real one.
The reference prints, per evaluation, the two divergences and the two diversities (their repr round-trips), so the whole trajectory is
parsed from its output: per iteration the scores of the right and the left candidate, and from them the decision and the score kept.

    a/...   two FLOAT micro models (the second with the seeded weights synth.vit_state_dict(micro, SEED_W2)), bit_config None
    b/...   the quantized micro model at [8] * 10 against itself at [4] * 10
    <run>/x0, numpy_seed, epsilon     the N seeded images, the seed given to np.random.seed in front of the call, the step
    <run>/pos, idx                    the draws, recorded from np.random.randint as the reference made them
    <run>/score_right, score_left, decision (0 keep / 1 right / 2 left), score     per iteration; <run>/score0 the initial score
    <run>/parts                       [1 + 2 * iterations, 4] divergence1, divergence2, diversity1, diversity2 of every evaluation
    <run>/x_final                     what the reference returned

Asserted here: (i) at every decision the compared scores are exactly equal or differ by at least 1e-9 relative (so a restatement within
1e-12 takes the same decisions); (ii) for run b the canonical oracle (OracleViT on the CPU) gives the reference's logits bit for bit on
every candidate batch the run evaluated.  Seeds tried: SEED = 41, N = 4 (the first choice; both conditions hold)."""
import contextlib
import io
import os
import re
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as GG  # noqa: E402

synth = GG.synth
OUT = os.path.join(ROOT, 'tests', 'golden', 'profiling_micro.npz')
SEED, SEED_W2, N, EPS = 41, 42, 4, 0.2


class Recorded:
    """the model, with every (inputs, bit_config, logits) of its calls kept"""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, inputs, bit_config=None, plot=False):
        out = self.model(inputs, bit_config, plot)
        self.calls.append((inputs.detach().clone(), bit_config, out[0].detach().clone()))
        return out


def gap_ok(a, b):
    return a == b or abs(a - b) >= 1e-9 * max(abs(a), abs(b))


def run(DU, m1, c1, m2, c2, x0, numpy_seed):
    draws, real = [], np.random.randint
    np.random.randint = lambda *a, **k: draws.append(int(real(*a, **k))) or draws[-1]
    buf = io.StringIO()
    try:
        np.random.seed(numpy_seed)
        with contextlib.redirect_stdout(buf), torch.no_grad():
            x_final = DU.gen_profiling_inputs_in_blackbox(m1, c1, m2, c2, x0.clone(), epsilon=EPS)
    finally:
        np.random.randint = real
    text = buf.getvalue()
    num = r'([-+0-9.einfa]+)'
    parts = np.array([[float(v) for v in m] for m in re.findall(r'output distance: %s,%s\n\s*metrics: %s,%s' % (num, num, num, num), text)])
    iters = len(re.findall(r'mutation \d+-th iteration', text))
    assert parts.shape == (1 + 2 * iters, 4) and len(draws) == 2 * iters, (parts.shape, iters, len(draws))
    ev = parts[:, 0] * parts[:, 1] * parts[:, 2] * parts[:, 3]                   # dataset_utility.py:258, the same fp64 products
    score0 = float(re.search(r'^score=(\S+)$', text, flags=re.M).group(1))
    assert score0 == ev[0]
    moves = re.findall(r'^mutate (right|left): (\S+)->(\S+)$', text, flags=re.M)
    score, rows, k = score0, [], 0
    for it in range(iters):
        r, l = float(ev[1 + 2 * it]), float(ev[2 + 2 * it])
        assert gap_ok(r, score) and gap_ok(l, score) and gap_ok(r, l), ('condition (i) fails at iteration', it, r, l, score)
        dec = 0 if (r <= score and l <= score) else (1 if r > l else 2)
        if dec:
            side, was, now = moves[k]
            k += 1
            assert side == ('right', 'left')[dec - 1] and float(was) == score and float(now) == (r, l)[dec - 1]
            score = (r, l)[dec - 1]
        rows.append((r, l, dec, score))
    assert k == len(moves)
    rows = np.array(rows)
    return {'x0': x0.numpy(), 'numpy_seed': np.int64(numpy_seed), 'epsilon': np.float64(EPS), 'pos': np.array(draws[0::2], dtype=np.int64),
            'idx': np.array(draws[1::2], dtype=np.int64), 'score0': np.float64(score0), 'score_right': rows[:, 0], 'score_left': rows[:, 1],
            'decision': rows[:, 2].astype(np.int8), 'score': rows[:, 3], 'parts': parts, 'x_final': x_final.numpy()}


def main():
    ref = GG.import_reference()
    for name in ('torchvision', 'torchvision.datasets', 'torchvision.transforms'):
        sys.modules.setdefault(name, types.ModuleType(name))
    import dataset_utility as DU
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'micro_vit.npz'))
    arch = synth.ARCHS['micro']
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    fp1 = GG.build_ref(arch, sd, ref)
    fp2 = GG.build_ref(arch, synth.vit_state_dict(arch, SEED_W2), ref)
    q = GG.build_ref(arch, sd, ref)
    with torch.no_grad():
        q.model_open_calibrate()
        q.model_open_last_calibrate()
        q(torch.from_numpy(g['x_cal']), plot=False)
        q.model_close_calibrate()
        q.model_quant()
    x0 = synth.uniform(SEED, 'profiling/x', (N, 3, arch['img_size'], arch['img_size']))
    out = {'seed': np.int64(SEED), 'seed_w2': np.int64(SEED_W2)}
    a = run(DU, fp1, None, fp2, None, x0, SEED)
    rq = Recorded(q)
    b = run(DU, rq, [8] * 10, rq, [4] * 10, x0, SEED + 1)
    # (ii) the canonical oracle on every distinct (batch, bit_config) the reference evaluated
    orc = GG.oracle.OracleViT(arch, sd)
    orc.calib = GG.oracle.extract_calib(q)
    seen, bad = {}, 0
    for x, cfg, logits in rq.calls:
        key = (x.numpy().tobytes(), tuple(cfg))
        if key not in seen:
            with torch.no_grad():
                seen[key] = orc.quant_forward(x, list(cfg))
        bad += not torch.equal(seen[key], logits)
    assert bad == 0, 'condition (ii) fails: the oracle differs from the reference on %d of %d evaluations' % (bad, len(rq.calls))
    for tag, r in (('a', a), ('b', b)):
        for k, v in r.items():
            out['%s/%s' % (tag, k)] = v
        d = r['decision']
        print('run %s: %d iterations, keep / right / left = %d / %d / %d, final score %.6g' % (
            tag, len(d), int((d == 0).sum()), int((d == 1).sum()), int((d == 2).sum()), r['score'][-1]))
    print('oracle == reference on %d evaluations (%d distinct)' % (len(rq.calls), len(seen)))
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
