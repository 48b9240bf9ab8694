"""Generate tests/golden/micro_vit_float_ops.npz by RUNNING THE REAL REFERENCE on the CPU under Config(ptf, lis) = (False, False),
(True, False) and (False, True): the configurations whose LayerNorm and / or softmax are the reference's float operators.

    python tools/gen_golden_float_ops.py [seed]

Nothing of the reference is copied: the fixture holds data only - the calibrated scales, the int8 codes at every QAct for the all-8-bit list,
the logits of three bit lists, the softmax tables, and the measured distance between the reference's float operators and the canonical
restatement of tests/_float_ops_ref.py.  Weights and images come from the package's deterministic generator (synth.py): the fixture keeps
the seed.

The generator asserts what tests/test_float_ops.py repeats: the canonical operators, fed the reference's INPUT codes of each stage, give
output codes that differ from the reference's by at most 1 anywhere and in at most 1 code per 1 000 per stage.  The whole-model figure (logit
codes that differ) is recorded without a cap.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gen_golden as G                      # noqa: E402  (import_reference / build_ref / run_with_taps, synth, oracle)
import _float_ops_ref as R                  # noqa: E402

CONFIGS = {'ff': (False, False), 'tf': (True, False), 'ft': (False, True)}      # tag -> (ptf, lis)
CAP_PER_1000 = 1


def bit_lists(L):
    mixed = [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)]
    return {'q8': [8] * L, 'q4': [4] * L, 'qmix': mixed}


def stage_checks(arch, W, c, taps, bits, ptf, lis):
    """-> {stage name: (differing codes, codes, max |difference|)} of the canonical float operators on the reference's input codes"""
    D, H, depth = arch['embed_dim'], arch['num_heads'], arch['depth']
    hd = D // H
    out = {}

    def cmp(name, got, want):
        d = (got.reshape(want.shape).numpy().astype(np.int64) - want.astype(np.int64))
        out[name] = (int((d != 0).sum()), int(d.size), int(np.abs(d).max()))

    prev, s_prev = 'qact1', c['qact1']
    for i in range(depth):
        p = 'blocks.%d.' % i
        bi, bm = R.BIT_POOL.index(bits[4 * i + 1]), R.BIT_POOL.index(bits[4 * i + 3])
        if not ptf:
            cs, s0 = c[p + 'attn.best_scale'][bi], c[p + 'attn.best_act_scale'][bi]
            q0, _ = R.float_layernorm(torch.from_numpy(taps[prev].astype(np.int64)), float(s_prev.reshape(-1)[0]), W[p + 'norm1.weight'],
                                      W[p + 'norm1.bias'], 1e-6, 1.0 / (cs * s0).reshape(-1).expand(D))
            cmp(p + 'attn.qact0', q0, taps[p + 'attn.qact0'])
            csm, sm0 = c[p + 'mlp.best_scale'][bm], c[p + 'mlp.best_act_scale'][bm]
            q0, _ = R.float_layernorm(torch.from_numpy(taps[p + 'qact2'].astype(np.int64)), float(c[p + 'qact2'].reshape(-1)[0]),
                                      W[p + 'norm2.weight'], W[p + 'norm2.bias'], 1e-6, 1.0 / (csm * sm0).reshape(-1).expand(D))
            cmp(p + 'mlp.qact0', q0, taps[p + 'mlp.qact0'])
        if not lis:
            q1 = torch.from_numpy(taps[p + 'attn.qact1'].astype(np.int64))
            Bn, N = q1.shape[0], q1.shape[1]
            v = q1.reshape(Bn, N, 3, H, hd).permute(2, 0, 3, 1, 4)[2]
            sc = torch.from_numpy(taps[p + 'attn.qact_attn1'].astype(np.int64))
            q2 = R.softmax_attention(sc, v, R.softmax_table(c[p + 'attn.qact_attn1']), float(c[p + 'attn.qact1'] / c[p + 'attn.qact2']))
            cmp(p + 'attn.qact2', q2.transpose(1, 2).reshape(Bn, N, D), taps[p + 'attn.qact2'])
        prev, s_prev = p + 'qact4', c[p + 'qact4']
    if not ptf:
        s_f = c['qact2']
        qf, _ = R.float_layernorm(torch.from_numpy(taps[prev].astype(np.int64))[:, 0], float(s_prev.reshape(-1)[0]), W['norm.weight'], W['norm.bias'],
                                  1e-6, (1.0 / s_f).reshape(-1).expand(D))
        cmp('qact2', qf, taps['qact2'])
    return out


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    torch.manual_seed(0)
    ref_config, ref_models, vit_fquant = G.import_reference()
    arch = G.synth.ARCHS['micro']
    sd = G.synth.vit_state_dict(arch, seed)
    x_cal = G.synth.images(seed, 4, arch['img_size'])
    x_ev = G.synth.images(seed, 6, arch['img_size'], offset=1000)
    L = 4 * arch['depth'] + 2
    lists = bit_lists(L)
    out = {'seed': np.int64(seed), 'n_calib': np.int64(4), 'n_eval': np.int64(6), 'bit_qmix': np.array(lists['qmix'], dtype=np.int8),
           'cap_per_1000': np.int64(CAP_PER_1000)}
    ok = True
    for tag, (ptf, lis) in CONFIGS.items():
        shim = types.SimpleNamespace(Config=lambda *a, _p=ptf, _l=lis: ref_config.Config(_p, _l, 'minmax'))
        model = G.build_ref(arch, sd, (shim, ref_models, vit_fquant))
        with torch.no_grad():
            model.model_open_calibrate()
            model.model_open_last_calibrate()
            model(x_cal, plot=False)
            model.model_close_calibrate()
            model.model_quant()
        calib = G.oracle.extract_calib(model)
        for k, v in G.oracle.flatten_calib(calib).items():
            out['%s/calib/%s' % (tag, k)] = v.numpy()
        if not lis:
            for i in range(arch['depth']):
                out['%s/softmax_table/%d' % (tag, i)] = R.softmax_table(calib['blocks.%d.attn.qact_attn1' % i]).astype(np.uint32)
        for name, bits in lists.items():
            o, _, _, taps = G.run_with_taps(model, x_ev, bits, lambda n: not n.endswith('log_int_softmax'))
            out['%s/logits/%s' % (tag, name)] = o.numpy()
            canon = R.quant_forward(G.oracle, arch, sd, calib, x_ev, bits, ptf, lis)
            s_o = float(calib['act_out'].reshape(-1)[0])
            dl = torch.round((canon - o) / s_o).abs()
            out['%s/logit_codes_differ/%s' % (tag, name)] = np.array([int((dl > 0).sum()), dl.numel(), int(dl.max())], dtype=np.int64)
            print('%s %s: whole model, %d of %d logit codes differ from the reference (max %d)' % (tag, name, int((dl > 0).sum()), dl.numel(), int(dl.max())))
            checks = stage_checks(arch, sd, calib, taps, bits, ptf, lis)
            for st, (nd, n, mx) in checks.items():
                out['%s/stage_diff/%s/%s' % (tag, name, st)] = np.array([nd, n, mx], dtype=np.int64)
                good = mx <= 1 and nd * 1000 <= CAP_PER_1000 * n
                ok = ok and good
                print('   %-28s %d of %d codes differ (max %d)%s' % (st, nd, n, mx, '' if good else '   <-- over the cap'))
            if name == 'q8':
                for k, v in taps.items():
                    out['%s/taps/%s' % (tag, k)] = v.astype(np.int8) if np.abs(v).max() < 128 else v
    assert ok, 'seed %d: a stage is over the cap (at most 1 code per 1 000, never by more than 1): choose another seed' % seed
    path = os.path.join(G.GOLD, 'micro_vit_float_ops.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
