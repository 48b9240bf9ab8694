"""Generate tests/golden/softmax_bits.npz by RUNNING THE REAL REFERENCE on the CPU with a 3-bit log-int-softmax
(``cfg.BIT_TYPE_S = BIT_TYPE_DICT['uint3']``, the edit point of the reference's config.py:34-36).

    python tools/gen_golden_softmax_bits.py [seed]

Nothing of the reference is copied: the fixture holds data only.
  1. ``QIntSoftmax(uint3)`` on the score vectors tests/golden/kat_ops.npz uses for uint4: the exponents (16 = zero).
  2. the reference's ``WindowAttention`` under uint3 at 7 x 7, with and without a three-region mask (the module, weights and inputs of
     oracle/gen_golden_swin.py): scales and the codes at every QAct.
  3. the micro ViT calibrated and run by the reference under uint3, weights of ``_softmax_bits_ref.micro_weights`` (seed 1, every
     attn.qkv.weight times 4): calibration state, logits of [8]*10, [4]*10 and a mixed list, the taps of the all-8-bit list.
The generator asserts what tests/test_softmax_bits.py repeats - the helper of tests/_softmax_bits_ref.py equals the reference on every
element of 1 and 2 and on the logits and taps of 3 - and that the fixture tells the widths apart: every block of 3 has exponents in 8 ... 15
under uint4 and at least one logit code differs from the uint4 run of the same weights.  If a platform-dependent rounding
hits at this seed, move the seed: no tolerance.
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
import swin_oracle as SO                    # noqa: E402
import _softmax_bits_ref as R               # noqa: E402


def small(v):
    return v.astype(np.int8) if v.min() >= -128 and v.max() <= 127 else v.astype(np.int16)


def k_of(p):
    return torch.where(p > 0, -torch.log2(p.clamp(min=1e-30)), torch.full_like(p, 16.0)).round().to(torch.int8)


def gen_kat(out, ref_models, bit3):
    g = np.load(os.path.join(G.GOLD, 'kat_ops.npz'))
    for e in range(3, 9):
        sf = torch.tensor([2.0 ** -e])
        codes = torch.from_numpy(g['lis/%d/codes' % e].astype(np.float32))
        sm = ref_models.QIntSoftmax(log_i_softmax=True, bit_type=bit3, quantizer_str='log2')
        k = k_of(sm(codes * sf, sf))
        assert torch.equal(R.lis_int_bits(codes, sf, 3).to(torch.int8), k), e
        assert torch.equal(R.lis_int_bits(codes, sf, 4).to(torch.int8), k_of(torch.from_numpy(g['lis/%d/probs' % e]))), e
        out['lis3/%d/k' % e] = k.numpy()
        print('kat sf 2^-%d: exponents %s' % (e, sorted(R.exponent_classes(k))))


def gen_window(out, ref_config, ref_models, bit3):
    from models import swin_quant
    synth = G.synth
    dim, heads, ws, nW, Bimg = 64, 2, 7, 3, 2
    N = ws * ws
    cfg = ref_config.Config(True, True, 'minmax')
    cfg.BIT_TYPE_S = bit3
    m = swin_quant.WindowAttention(dim, window_size=(ws, ws), num_heads=heads, qkv_bias=True, quant=False, calibrate=False, cfg=cfg)
    W = {
        'qkv.weight': synth.normal(21, 'wa/qkv.w', (3 * dim, dim), 0.09), 'qkv.bias': synth.normal(21, 'wa/qkv.b', (3 * dim,), 0.1),
        'proj.weight': synth.normal(21, 'wa/proj.w', (dim, dim), 0.08), 'proj.bias': synth.normal(21, 'wa/proj.b', (dim,), 0.05),
        'relative_position_bias_table': synth.normal(21, 'wa/table', ((2 * ws - 1) ** 2, heads), 0.6),
    }
    missing, unexpected = m.load_state_dict(W, strict=False)
    assert not unexpected and set(missing) <= {'relative_position_index'}, (missing, unexpected)
    m.eval()
    assert m.log_int_softmax.bit_type.bits == 3
    s_in = 2.0 ** -4
    codes_cal = torch.clamp(torch.round(synth.normal(21, 'wa/xcal', (Bimg * nW, N, dim), 18.0)), -128, 127)
    codes_ev = torch.clamp(torch.round(synth.normal(21, 'wa/xev', (Bimg * nW, N, dim), 18.0)), -128, 127)
    region = torch.zeros(nW, N, dtype=torch.long)
    region[1, 28:] = 1
    region[2, :] = (torch.arange(N) % 7 >= 4).long() + 2 * (torch.arange(N) >= 21).long()
    mask = (region.unsqueeze(1) != region.unsqueeze(2)).float() * -100.0
    q_mods = {n: mod for n, mod in m.named_modules() if isinstance(mod, (ref_models.QAct, ref_models.QLinear))}
    with torch.no_grad():
        for mod in q_mods.values():
            mod.calibrate, mod.last_calibrate = True, True
        m(codes_cal * s_in, mask=mask)
        for mod in q_mods.values():
            mod.calibrate, mod.last_calibrate, mod.quant = False, False, True
        m.log_int_softmax.quant = True
        c = {n: mod.quantizer.scale.detach().float().reshape(-1) for n, mod in q_mods.items() if isinstance(mod, ref_models.QAct)}
        for n in ('qkv', 'proj'):
            c[n] = q_mods[n].quantizer.dic_scale['int8'].detach().float().reshape(-1)
        for tag, msk in (('nomask', None), ('mask', mask)):
            taps, hooks = {}, []

            def mk(name, mod):
                def hook(_m, _inp, o):
                    if name == 'log_int_softmax':
                        taps['softmax_k'] = k_of(o).numpy()
                    else:
                        taps[name] = torch.round(o / mod.quantizer.scale.reshape(G.oracle.act_shape(o) if o.dim() > 1 else (-1,))).to(torch.int16).numpy()
                return hook
            for name, mod in m.named_modules():
                if isinstance(mod, ref_models.QAct) or name == 'log_int_softmax':
                    hooks.append(mod.register_forward_hook(mk(name, mod)))
            m(codes_ev * s_in, mask=msk)
            for h in hooks:
                h.remove()
            mine, mine4 = {}, {}
            R.window_attention(codes_ev, s_in, W, c, heads, ws, 3, mask=msk, taps=mine)
            R.window_attention(codes_ev, s_in, W, c, heads, ws, 4, mask=msk, taps=mine4)
            for name in ('qact1', 'qact_attn1', 'qact_table', 'qact2', 'softmax_k', 'qact3', 'qact4'):
                got = mine[name].numpy().astype(np.int64)
                assert np.array_equal(got, taps[name].astype(np.int64).reshape(got.shape)), (tag, name)
                out['win/taps/%s/%s' % (tag, name)] = small(taps[name])
            k4 = mine4['softmax_k']
            n_hi = int(((k4 >= 8) & (k4 <= 15)).sum())
            n_q3 = int((mine4['qact3'] != mine['qact3']).sum())
            print('window %-6s: %d of %d probabilities have exponents 8 ... 15 under uint4; %d of %d qact3 codes differ between the widths'
                  % (tag, n_hi, k4.numel(), n_q3, mine['qact3'].numel()))
            assert n_hi > 0 and n_q3 > 0, 'the window case does not tell the widths apart: move the seed'
    for n, s in c.items():
        out['win/scale/' + n] = s.numpy()
    out['win/x_ev'] = codes_ev.to(torch.int8).numpy()
    out['win/s_in'] = np.float32(s_in)
    out['win/region'] = region.to(torch.int8).numpy()
    out['win/seed'] = np.int64(21)


def gen_micro(out, ref, bit3, bit4, seed):
    ref_config, ref_models, vit_fquant = ref
    arch = G.synth.ARCHS['micro']
    sd = R.micro_weights(G.synth, arch, seed)
    x_cal = G.synth.images(seed, 4, arch['img_size'])
    x_ev = G.synth.images(seed, 2, arch['img_size'], offset=1000)
    L = 4 * arch['depth'] + 2
    lists = R.micro_bit_lists(L)
    logits = {}
    for bt in (bit4, bit3):
        def config(*a, _bt=bt):
            cfg = ref_config.Config(True, True, 'minmax')
            cfg.BIT_TYPE_S = _bt
            return cfg
        model = G.build_ref(arch, sd, (types.SimpleNamespace(Config=config), ref_models, vit_fquant))
        assert all(b.attn.log_int_softmax.bit_type.bits == bt.bits for b in model.blocks)
        with torch.no_grad():
            model.model_open_calibrate()
            model.model_open_last_calibrate()
            cal = model(x_cal, plot=False)[0]
            model.model_close_calibrate()
            model.model_quant()
        calib = G.oracle.extract_calib(model)
        logits[bt.bits] = {}
        for name, bits in lists.items():
            o, _, _, taps = G.run_with_taps(model, x_ev, bits)
            logits[bt.bits][name] = o
            mine = {}
            canon = R.vit_forward(arch, sd, calib, x_ev, bits, bt.bits, mine)
            assert torch.equal(canon, o), (bt.bits, name, 'the helper differs from the reference: move the seed')
            for k, v in taps.items():
                assert np.array_equal(mine[k].numpy().astype(np.int64).reshape(v.shape), v.astype(np.int64)), (bt.bits, name, k)
            if bt.bits == 4 and name == 'q8':
                for i in range(arch['depth']):
                    k4 = taps['blocks.%d.attn.softmax_k' % i]
                    n_hi = int(((k4 >= 8) & (k4 <= 15)).sum())
                    print('micro block %d: %d of %d probabilities have exponents 8 ... 15 under uint4' % (i, n_hi, k4.size))
                    assert n_hi > 0, 'block %d has no exponent in 8 ... 15: the fixture would not tell the widths apart' % i
            if bt.bits == 3:
                out['micro/logits/' + name] = o.numpy()
                if name == 'q8':
                    for k, v in taps.items():
                        out['micro/taps/' + k] = small(v)
        if bt.bits == 3:
            orc, cal_mine = R.vit_calibrate(arch, sd, x_cal, 3)
            flat, mine = G.oracle.flatten_calib(calib), G.oracle.flatten_calib(orc.calib)
            assert set(flat) == set(mine) and all(torch.equal(flat[k], mine[k]) for k in flat), 'calibration: the helper differs from the reference'
            for k, v in flat.items():
                out['micro/calib/' + k] = v.numpy()
            out['micro/calib_logits'] = cal.numpy()
    s_o = float(out['micro/calib/act_out'].reshape(-1)[0])
    d = torch.round((logits[3]['q8'] - logits[4]['q8']) / s_o)
    print('micro: %d of %d logit codes of [8]*%d differ between uint3 and uint4' % (int((d != 0).sum()), d.numel(), L))
    assert int((d != 0).sum()) > 0
    out['micro/codes_differ_from_uint4'] = np.int64(int((d != 0).sum()))
    out['micro/seed'] = np.int64(seed)
    out['micro/qkv_gain'] = np.float32(R.QKV_GAIN)
    out['micro/n_calib'], out['micro/n_eval'] = np.int64(4), np.int64(2)
    out['micro/bit_qmix'] = np.array(lists['qmix'], dtype=np.int8)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else R.MICRO_SEED
    torch.manual_seed(0)
    ref = G.import_reference()
    from models.ptq.bit_type import BIT_TYPE_DICT
    bit3, bit4 = BIT_TYPE_DICT['uint3'], BIT_TYPE_DICT['uint4']
    out = {}
    gen_kat(out, ref[1], bit3)
    gen_window(out, ref[0], ref[1], bit3)
    gen_micro(out, ref, bit3, bit4, seed)
    path = os.path.join(G.GOLD, 'softmax_bits.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= (1 << 20), 'fixture over the size limit for a committed file'


if __name__ == '__main__':
    main()
