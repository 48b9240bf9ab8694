"""GPU: the profiling-input search on the MI355X - the p2v_profile_* kernels against the fp64 numpy restatement (tests/_profiling_ref.py),
bit-equal ties, output footprints in sentinel arenas, the candidate builder, the whole device loop against the REAL reference's
trajectory (tests/golden/profiling_micro.npz, run b), the device loop teacher-forced against full-batch forwards, epsilon below the input
step, and the loop under torch's synchronisation debug mode."""
import copy

import numpy as np
import pytest
import torch

import _profiling_ref as R
from _arena import Arena
from conftest import load_golden
from test_ddv import micro_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def layout(n, classes):
    """the state block of include/p2vit.h: offsets in doubles (D, g, rowd, rowg per model) and in floats (O, O0 per model), bytes"""
    at, lay = 2, {}
    for m in range(2):
        for name, size in (('D', n * n), ('g', n), ('rowd', 2 * n), ('rowg', 2)):
            lay[name, m] = at
            at += size
    at = (at + 1) // 2 * 2
    f = at * 2
    for m in range(2):
        for name in ('O', 'O0'):
            lay[name, m] = f
            f += n * classes
    return lay, (f * 4 + 15) // 16 * 16


class Search:
    """one search state on the device, every buffer in a sentinel arena, driven through ctypes"""

    def __init__(self, dva, n, classes, elems, logits1, logits2, x, sentinel=0x5B):
        self.E, self.L = dva.engine, dva.engine.lib()
        self.n, self.classes, self.elems = n, classes, elems
        self.lay, self.nbytes = layout(n, classes)
        assert self.L.p2v_profile_state_bytes(n, classes) == self.nbytes
        self.state = Arena(1, self.nbytes, dtype=torch.uint8, sentinel=sentinel)
        self.x = Arena(1, n * elems, dtype=torch.float32, sentinel=sentinel, init=x.reshape(1, -1))
        self.staging = Arena(1, 2 * elems, dtype=torch.float32, sentinel=sentinel)
        self.trace = Arena(1, 4, dtype=torch.float64, sentinel=sentinel)
        self.cand = [Arena(1, 2 * classes, dtype=torch.float32, sentinel=sentinel, offset=84, init=torch.zeros(1, 2 * classes)) for _ in range(2)]
        lg = [Arena(1, n * classes, dtype=torch.float32, sentinel=sentinel, offset=84, init=t.reshape(1, -1)) for t in (logits1, logits2)]
        self.E.check(self.L.p2v_profile_init(self.state.ptr, self.nbytes, n, classes, lg[0].ptr, lg[1].ptr, None))
        torch.cuda.synchronize()
        for a in lg:
            a.read('init logits')

    def read(self, what):
        """-> dict: score, D, g, O, O0 (numpy); checks the guards of the state block"""
        raw = self.state.read(what).numpy().reshape(-1)
        d, f = raw.view(np.float64), raw.view(np.float32)
        n, c = self.n, self.classes
        out = {'score': d[0].copy(), 'raw': raw.copy()}
        for m in range(2):
            out['D', m] = d[self.lay['D', m]: self.lay['D', m] + n * n].reshape(n, n).copy()
            out['g', m] = d[self.lay['g', m]: self.lay['g', m] + n].copy()
            for nm in ('O', 'O0'):
                out[nm, m] = f[self.lay[nm, m]: self.lay[nm, m] + n * c].reshape(n, c).copy()
        return out

    def candidates(self, idx, pos, eps):
        self.E.check(self.L.p2v_profile_candidates(self.x.ptr, self.n, self.elems, idx, pos, eps, self.staging.ptr, None))

    def step(self, idx, pos, cand1, cand2):
        """cand1 / cand2: numpy fp32 [2][classes] -> the trace row (numpy fp64 [4])"""
        for a, cnd in zip(self.cand, (cand1, cand2)):
            flat = torch.from_numpy(np.ascontiguousarray(cnd, dtype=np.float32).reshape(-1)).cuda()
            a.dev[a.start: a.start + flat.numel() * 4].copy_(flat.view(torch.uint8))
        self.E.check(self.L.p2v_profile_step(self.state.ptr, self.nbytes, self.n, self.classes, self.cand[0].ptr, self.cand[1].ptr,
                                             self.staging.ptr, self.x.ptr, self.elems, idx, pos, self.trace.ptr, None))
        torch.cuda.synchronize()
        return self.trace.read('trace').numpy().reshape(-1)


def close(got, want, what):
    """1e-9 relative, element by element; exact zeros stay exact"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(got == 0, want == 0), what
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (what, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))))


def script(n, classes, seed):
    """seed logits and a sequence of (idx, candidate rows of model 1 [2][classes], of model 2, expected decision): far moves of one side
    against the unchanged row force right / left, unchanged rows on both sides and a return to the seed rows force keep.  The expected
    decisions are those of the numpy restatement, with margins far above 1e-9 (checked by the caller)."""
    g = np.random.RandomState(seed)
    o = [g.randn(n, classes).astype(np.float32) for _ in range(2)]
    ref = R.State(o[0], o[1])
    steps = []
    order = [(0, 'right'), (n - 1, 'left'), (0, 'tie'), (n // 2, 'right'), (n - 1, 'back'), (min(1, n - 1), 'left'), (n // 2, 'tie')]
    for k, (idx, kind) in enumerate(order):
        cur = [ref.O[m][idx].copy() for m in range(2)]
        far = [(cur[m] + (8.0 + 4 * k) * g.randn(classes)).astype(np.float32) for m in range(2)]
        if kind == 'right':
            c = [np.stack([far[m], cur[m]]) for m in range(2)]
        elif kind == 'left':
            c = [np.stack([cur[m], far[m]]) for m in range(2)]
        elif kind == 'tie':
            c = [np.stack([cur[m], cur[m]]) for m in range(2)]
        else:                                               # both candidates: the seed row again (divergence term 0)
            c = [np.stack([ref.O0[m][idx], ref.O0[m][idx]]) for m in range(2)]
        before = ref.score
        r, l, dec, after = ref.step(idx, c[0], c[1])
        steps.append((idx, c[0], c[1], (r, l, dec, after), before))
    return o, steps


@pytest.mark.parametrize('classes', [1, 10, 1000, 1003])
@pytest.mark.parametrize('n', [1, 2, 5, 33])
def test_kernels_against_numpy(dva, n, classes):
    """init, then scripted steps; D, g, O, score and trace after every step.  fp64 sums of n^2 * classes <= 1.1e6 terms in any order differ
    by at most 1.1e6 * 2^-53 = 1.2e-10 relative (all terms positive): inside the 1e-9 the DDV tests use.  Decisions are exact: the
    scripted margins are above 1e-6 (asserted on the restatement), or the scores are equal bit for bit (ties)."""
    o, steps = script(n, classes, 100 * n + classes)
    x = torch.arange(n * 8, dtype=torch.float32).reshape(n, 8)
    s = Search(dva, n, classes, 8, torch.from_numpy(o[0]), torch.from_numpy(o[1]), x)
    ref = R.State(o[0], o[1])
    got = s.read('init')
    for m in range(2):
        close(got['D', m], ref.D[m], 'D')
        assert np.array_equal(got['g', m], np.zeros(n)) and np.array_equal(got['O', m], o[m]) and np.array_equal(got['O0', m], o[m])
        assert np.array_equal(got['D', m], got['D', m].T) and np.all(np.diag(got['D', m]) == 0)
    assert got['score'] == 0.0
    seen = set()
    for idx, c1, c2, (r, l, dec, after), before in steps:
        for a, b in ((r, before), (l, before), (r, l)):
            assert a == b or abs(a - b) > 1e-6 * max(abs(a), abs(b)), 'the script leaves a decision to less than 1e-6'
        s.candidates(idx, 3, 0.5)
        t = s.step(idx, 3, c1, c2)
        ref.step(idx, c1, c2)
        close(t[[0, 1, 3]], [r, l, after], 'trace')
        assert int(t[2]) == dec and t[2] in (0.0, 1.0, 2.0)
        seen.add(dec)
        got = s.read('step')
        close(got['score'], ref.score, 'score')
        assert got['score'] == t[3]
        for m in range(2):
            close(got['D', m], ref.D[m], 'D')
            close(got['g', m], ref.g[m], 'g')
            assert np.array_equal(got['O', m], ref.O[m]) and np.array_equal(got['O0', m], o[m])
            assert np.array_equal(got['D', m], got['D', m].T)
    assert seen == ({0} if n == 1 else {0, 1, 2})          # one input: the diversity and so every score is 0


def test_diversity_entry_point(dva):
    for n, classes in ((1, 7), (2, 10), (7, 1003), (33, 1000)):
        o = torch.randn(n, classes, generator=torch.Generator().manual_seed(n)).cuda()
        got = float(dva.profiling._diversity_gpu(o))
        want = R.diversity(o.cpu().numpy())
        assert abs(got - want) <= 1e-9 * want and (n > 1 or got == 0.0)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.randn(12, 10))

        def forward(self, x, bit_config=None, plot=False):
            return x.reshape(x.shape[0], -1) @ self.w, [], []

    m, x = M().cuda(), torch.randn(5, 3, 2, 2)
    want = R.diversity(m(x.cuda())[0].detach().cpu().numpy())
    assert abs(dva.metrics_output_diversity(m, None, x) - want) <= 1e-9 * want


@pytest.mark.parametrize('classes', [10, 1003])
def test_ties_score_bit_equal(dva, classes):
    """a candidate equal to the current rows scores bit-equal to the stored score and is kept: at every idx, after commits at other rows,
    with candidates built with epsilon = 0"""
    n = 5
    o, steps = script(n, classes, 7)
    x = torch.rand(n, 12, generator=torch.Generator().manual_seed(1))
    s = Search(dva, n, classes, 12, torch.from_numpy(o[0]), torch.from_numpy(o[1]), x)
    moves = [st_ for st_ in steps if st_[3][2] != 0]          # the script's accepted steps (its kept ones leave the state as it is)
    assert len(moves) == 4
    for round_ in range(3):
        st = s.read('state')
        assert round_ == 0 or st['score'] > 0
        for idx in range(n):
            s.candidates(idx, idx, 0.0)
            stg = s.staging.read('staging').reshape(2, 12)
            assert torch.equal(stg[0], x[idx]) and torch.equal(stg[1], x[idx])
            rows = [np.stack([st['O', m][idx], st['O', m][idx]]) for m in range(2)]
            t = s.step(idx, idx, rows[0], rows[1])
            assert t.view(np.uint64)[0] == t.view(np.uint64)[1] == t.view(np.uint64)[3] == st['score'].view(np.uint64) and t[2] == 0.0
            assert np.array_equal(s.read('tie')['raw'][:8], st['raw'][:8])
        for idx, c1, c2, want, _ in moves[2 * round_: 2 * round_ + 2]:       # commits at other rows, then again
            t = s.step(idx, 0, c1, c2)
            assert int(t[2]) == want[2]
        x = s.x.read('inputs').reshape(n, 12)               # (the accepted steps copied staging[.][0] of the last builder call)


def test_footprint_in_arenas(dva):
    """state block, trace, staging batch and inputs in sentinel arenas, twice with two sentinels; an accepted step changes exactly one
    input element, a kept one none"""
    n, classes, elems = 5, 1003, 50
    o, steps = script(n, classes, 11)
    x = torch.rand(n, elems, generator=torch.Generator().manual_seed(2))

    def run(sentinel):
        s = Search(dva, n, classes, elems, torch.from_numpy(o[0]), torch.from_numpy(o[1]), x, sentinel=sentinel)
        out, cur = {}, x.clone()
        for k, (idx, c1, c2, want, _) in enumerate(steps):
            pos = (7 * k + 3) % elems
            s.candidates(idx, pos, 0.25)
            t = s.step(idx, pos, c1, c2)
            stg = s.staging.read('staging').reshape(2, elems)
            now = s.x.read('inputs').reshape(n, elems)
            changed = (now != cur).nonzero()
            dec = int(t[2])
            assert dec == want[2]
            if dec == 0:
                assert changed.numel() == 0
            else:
                assert changed.tolist() == [[idx, pos]] and now[idx, pos] == stg[dec - 1, pos]
            cur = now
            for c in s.cand:
                c.read('candidate logits')
            out['trace%d' % k] = torch.from_numpy(t.copy())
        st = s.read('end')
        out['state'] = torch.from_numpy(st['raw'][16:].copy().view(np.float32))       # (behind the score and its padding)
        out['score'] = torch.from_numpy(st['raw'][:8].copy().view(np.float64))
        out['pad'] = torch.from_numpy(st['raw'][8:16].copy())
        out['x'] = cur
        return out

    a = run(0x5B)
    b = run(0xA6)
    assert bool((a['pad'] == 0x5B).all()) and bool((b['pad'] == 0xA6).all())              # the padding double is never written
    for k in a:
        if k != 'pad':
            assert np.array_equal(a[k].numpy().view(np.uint8), b[k].numpy().view(np.uint8)), k


@pytest.mark.parametrize('elems', [48, 50, 7, 1])
def test_candidate_builder(dva, elems):
    """image sizes with and without a 16-byte tail (and images that start off a 16-byte boundary); pos first, last and around a chunk
    boundary; candidates bit-equal to x +- np.float32(eps), everything else copied"""
    n, eps = 3, 0.2
    x = torch.rand(n, elems, generator=torch.Generator().manual_seed(elems)) - 0.5
    o = torch.zeros(n, 4)
    s = Search(dva, n, 4, elems, o, o, x)
    e32 = np.float32(eps)
    for idx in range(n):
        for pos in sorted({0, elems - 1, min(3, elems - 1), min(4, elems - 1), elems // 2}):
            s.candidates(idx, pos, eps)
            torch.cuda.synchronize()
            got = s.staging.read('staging').numpy().reshape(2, elems)
            want = np.stack([x[idx].numpy(), x[idx].numpy()])
            want[0, pos] = want[0, pos] + e32
            want[1, pos] = want[1, pos] - e32
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (idx, pos)
    assert torch.equal(s.x.read('inputs').reshape(n, elems), x)


def _quant_micro(dva, synth):
    g = load_golden('micro_vit')
    m = micro_model(dva, synth, g).cuda()
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']).cuda())
    return m


def test_device_loop_matches_reference_trajectory(dva, synth):
    """fixture run b: the quantized micro-ViT at [8] * 10 against itself at [4] * 10, all 1000 iterations of the REAL reference.  The
    generator asserted oracle == reference on every batch the run evaluated and the engine equals the oracle bit for bit at micro size, so
    the logits are the reference's and only the fp64 distance sums differ in order (1e-9, as above); no decision hangs on less than that."""
    k = load_golden('profiling_micro')
    m = _quant_micro(dva, synth)
    trace = []
    x = dva.gen_profiling_inputs_in_blackbox(m, [8] * 10, m, [4] * 10, torch.from_numpy(k['b/x0']), epsilon=float(k['b/epsilon']),
                                             max_iterations=len(k['b/decision']), rng=np.random.RandomState(int(k['b/numpy_seed'])), trace=trace)
    t = np.array(trace, dtype=np.float64)
    assert x.is_cuda and np.array_equal(t[:, 2].astype(np.int8), k['b/decision'])
    for col, name in ((0, 'b/score_right'), (1, 'b/score_left'), (3, 'b/score')):
        want = k[name]
        assert np.all(np.abs(t[:, col] - want) <= 1e-9 * np.abs(want)), name
    assert np.array_equal(x.cpu().numpy(), k['b/x_final'])


def _teacher_forced(dva, f1, f2, x0, eps, pos, idx, trace):
    """follow the device's decisions; restate both scores of every iteration from FULL-batch forwards (fp64 torch, the host loop's
    formulas); -> the largest relative difference.  Each recorded decision must follow from the recorded scores under the reference's rule."""
    P = dva.profiling
    x, n = x0.clone(), x0.shape[0]
    o01, o02 = f1(x), f2(x)
    e = torch.tensor(eps, dtype=torch.float32, device=x.device)
    score, worst = 0.0, 0.0
    for (r, l, dec, after), p, i in zip(trace, pos, idx):
        cands = []
        for sign in (1, -1):
            c = x.clone()
            c.view(n, -1)[i, p] = x.view(n, -1)[i, p] + sign * e
            cands.append(c)
        for got, c in ((r, cands[0]), (l, cands[1])):
            o1, o2 = f1(c), f2(c)
            want = float(P.divergence(o1, o01)) * float(P.divergence(o2, o02)) * float(P.diversity(o1)) * float(P.diversity(o2))
            worst = max(worst, abs(got - want) / max(abs(want), 1e-300) if want != got else 0.0)
        assert dec == (0 if (r <= score and l <= score) else (1 if r > l else 2))
        assert after == (score, r, l)[dec]
        if dec:
            x, score = cands[dec - 1], after
    return worst, x


def test_device_loop_teacher_forced_swin(dva, synth):
    """swin_micro, 8 against 4 bits, n = 3, 40 iterations: engine logits do not depend on the batch, so the 2-image device loop and
    full-batch forwards differ by the order of the fp64 sums only"""
    m8 = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    m8.load_state_dict(synth.swin_state_dict(m8.state_dict(), 5))
    m8 = m8.cuda()
    dva.harness.calibrate_model(m8, synth.images(12, 4, 56).cuda())
    m4 = copy.deepcopy(m8)
    x0 = synth.images(11, 3, 56).cuda()
    pos, idx = dva.profiling.draw_mutations(3 * 56 * 56, 3, 40, np.random.RandomState(3))
    trace = []
    x = dva.gen_profiling_inputs_in_blackbox(m8, 8, m4, 4, x0, epsilon=0.2, max_iterations=40, rng=np.random.RandomState(3), trace=trace)
    f8, f4 = (lambda t: dva.profiling._module_logits(m8, 8, t)), (lambda t: dva.profiling._module_logits(m4, 4, t))
    worst, x_want = _teacher_forced(dva, f8, f4, x0, float(np.float32(0.2)), pos, idx, trace)
    print('swin teacher-forced: worst relative score difference %.3g, decisions %s' % (worst, [r[2] for r in trace]))
    assert worst <= 1e-9 and torch.equal(x, x_want)
    with pytest.raises(NotImplementedError):
        dva.gen_profiling_inputs_in_blackbox(m8, [8] * 10, m4, 4, x0, max_iterations=1)


FLOAT_BATCH_TOL = 1e-4


def test_device_loop_teacher_forced_float_model(dva, synth):
    """micro-ViT, n = 5, model 1 the FLOAT module graph, model 2 the engine at [8] * 10.  A float row from a 2-image batch can differ from
    the same row of the full batch in the last ulps (a float-batching effect of the BLAS, not a kernel property): fp32 logits are good to
    a few 2^-24 = 6e-8 relative to the row's largest entry, a distance between two rows that are 1e-2 of that apart then to some 1e-5,
    and the score is a product of four such means - FLOAT_BATCH_TOL = 1e-4, set before it was measured; measured on the MI355X against
    full-batch forwards on the same GPU: 3.62e-05, a margin of 2.8 (printed)."""
    g = load_golden('micro_vit')
    fp = micro_model(dva, synth, g).cuda()
    q = _quant_micro(dva, synth)
    x0 = synth.uniform(5, 'profiling/float', (5, 3, 32, 32)).cuda()
    pos, idx = dva.profiling.draw_mutations(3 * 32 * 32, 5, 40, np.random.RandomState(4))
    trace = []
    x = dva.gen_profiling_inputs_in_blackbox(fp, None, q, [8] * 10, x0, epsilon=0.2, max_iterations=40, rng=np.random.RandomState(4), trace=trace)
    f1, f2 = (lambda t: dva.profiling._module_logits(fp, None, t)), (lambda t: dva.profiling._module_logits(q, [8] * 10, t))
    worst, x_want = _teacher_forced(dva, f1, f2, x0, float(np.float32(0.2)), pos, idx, trace)
    print('float-model teacher-forced: worst relative score difference %.3g (tolerance %.0e)' % (worst, FLOAT_BATCH_TOL))
    assert worst <= FLOAT_BATCH_TOL and torch.equal(x, x_want)
    assert {r[2] for r in trace} - {0, 1, 2} == set()


def test_epsilon_below_input_step_keeps_everything(dva, synth):
    """inputs on the qact_input grid and epsilon an eighth of its step: both candidates quantise to the current codes, every logits row is
    unchanged, every score ties bit for bit, every iteration keeps and the inputs come back unchanged.  (Any changed logits row would raise
    the score above the seed's 0 and be accepted; ties at a positive score are test_ties_score_bit_equal's.)"""
    m = _quant_micro(dva, synth)
    s = float(m.qact_input.quantizer.scale.reshape(-1)[0])
    x0 = (torch.round(synth.uniform(6, 'profiling/grid', (4, 3, 32, 32)) / s) * s).cuda()
    trace = []
    x = dva.gen_profiling_inputs_in_blackbox(m, [8] * 10, m, [4] * 10, x0, epsilon=s / 8, max_iterations=60, rng=np.random.RandomState(2),
                                             trace=trace)
    assert all(r[2] == 0 and r[0] == r[1] == r[3] for r in trace) and torch.equal(x, x0)


def test_device_loop_never_synchronises(dva, synth):
    """engine models under torch.cuda.set_sync_debug_mode('error') for the loop's duration (the plans are frozen by a first call)"""
    m = _quant_micro(dva, synth)
    x0 = synth.uniform(7, 'profiling/sync', (4, 3, 32, 32)).cuda()
    sw = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    sw.load_state_dict(synth.swin_state_dict(sw.state_dict(), 5))
    sw = sw.cuda()
    dva.harness.calibrate_model(sw, synth.images(12, 4, 56).cuda())
    sw4 = copy.deepcopy(sw)
    xs = synth.images(11, 3, 56).cuda()
    runs = ((m, [8] * 10, m, [4] * 10, x0), (sw, 8, sw4, 4, xs))
    for a in runs:
        dva.gen_profiling_inputs_in_blackbox(*a, max_iterations=2, rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        outs = [dva.gen_profiling_inputs_in_blackbox(*a, max_iterations=20, rng=np.random.RandomState(0)) for a in runs]
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert all(o.is_cuda and bool(torch.isfinite(o).all()) for o in outs)
