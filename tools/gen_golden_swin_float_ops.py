"""Generate tests/golden/swin_winattn_softmax.npz by RUNNING THE REAL REFERENCE ``WindowAttention`` (models/swin_quant.py:53-221) standalone
on the CPU under Config(ptf=True, lis=False, 'minmax'): the configuration whose softmax is the reference's float one.

    python tools/gen_golden_swin_float_ops.py

Windows of 7 x 7, 12 x 12 and 2 x 2 tokens (dim 64, 2 heads, 2 images of 3 windows), each with and without a three-region mask; weights
and inputs come from the package's deterministic generator, as in oracle/gen_golden_swin.py (seeds 21 / 22 / 23).  Nothing of the reference
is copied: the fixture holds data only - the evaluation input codes (the calibration inputs follow from the seed), calibrated scales, region ids, the codes at every QAct, the softmax tables and the
measured distance between the reference's float softmax and the canonical restatement of tests/_swin_float_ops_ref.py.

The generator asserts what tests/test_swin_float_ops.py repeats: the canonical operator, fed the reference's own qact2 and qact1 codes,
gives qact3 codes that differ from the reference's by at most 1 anywhere and in at most 1 code per 1 000 per stage; and every qact2 scale
is at most 2^-2 (a masked key rounds to zero).  If a generator change breaks either, choose another seed.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import gen_golden as G                      # noqa: E402  (import_reference, synth, oracle)
import _swin_float_ops_ref as R             # noqa: E402

CASES = ((7, 21), (12, 22), (2, 23))        # (window side, seed)
CAP_PER_1000 = 1
DIM, HEADS, NW, BIMG = 64, 2, 3, 2


def regions(ws):
    """region ids [nW, N]: window 0 one region, window 1 two, window 2 three (the ids of oracle/gen_golden_swin.py at ws = 7)"""
    N = ws * ws
    t = torch.arange(N)
    region = torch.zeros(NW, N, dtype=torch.long)
    region[1, (4 * N) // 7:] = 1
    region[2, :] = (t % ws >= (4 * ws) // 7).long() + 2 * (t >= (3 * N) // 7).long()
    return region


def small(v):
    return v.astype(np.int8) if v.min() >= -128 and v.max() <= 127 else v.astype(np.int16)


def main():
    torch.manual_seed(0)
    ref_config, ref_models, _ = G.import_reference()
    from models import swin_quant
    synth = G.synth
    out = {'cap_per_1000': np.int64(CAP_PER_1000), 'cases': np.array(CASES, dtype=np.int64), 'dim': np.int64(DIM), 'heads': np.int64(HEADS),
           'n_windows': np.int64(NW), 'images': np.int64(BIMG)}
    ok = True
    for ws, seed in CASES:
        N = ws * ws
        pre = 'ws%d/' % ws
        cfg = ref_config.Config(True, False, 'minmax')
        m = swin_quant.WindowAttention(DIM, window_size=(ws, ws), num_heads=HEADS, qkv_bias=True, quant=False, calibrate=False, cfg=cfg)
        sd = {
            'qkv.weight': synth.normal(seed, 'wa/qkv.w', (3 * DIM, DIM), 0.09), 'qkv.bias': synth.normal(seed, 'wa/qkv.b', (3 * DIM,), 0.1),
            'proj.weight': synth.normal(seed, 'wa/proj.w', (DIM, DIM), 0.08), 'proj.bias': synth.normal(seed, 'wa/proj.b', (DIM,), 0.05),
            'relative_position_bias_table': synth.normal(seed, 'wa/table', ((2 * ws - 1) ** 2, HEADS), 0.6),
        }
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and set(missing) <= {'relative_position_index'}, (missing, unexpected)
        m.eval()
        s_in = 2.0 ** -4
        codes_cal = torch.clamp(torch.round(synth.normal(seed, 'wa/xcal', (BIMG * NW, N, DIM), 18.0)), -128, 127)
        codes_ev = torch.clamp(torch.round(synth.normal(seed, 'wa/xev', (BIMG * NW, N, DIM), 18.0)), -128, 127)
        region = regions(ws)
        mask = (region.unsqueeze(1) != region.unsqueeze(2)).float() * -100.0
        q_mods = {n: mod for n, mod in m.named_modules() if isinstance(mod, (ref_models.QAct, ref_models.QLinear))}
        with torch.no_grad():
            for mod in q_mods.values():
                mod.calibrate, mod.last_calibrate = True, True
            m(codes_cal * s_in, mask=mask)
            for mod in q_mods.values():
                mod.calibrate, mod.last_calibrate, mod.quant = False, False, True
            m.log_int_softmax.quant = True
            scales = {n: mod.quantizer.scale.detach().float().reshape(-1) for n, mod in q_mods.items() if isinstance(mod, ref_models.QAct)}
            s1, s2, s3 = (float(scales[k][0]) for k in ('qact1', 'qact2', 'qact3'))
            assert s2 <= R.S_Q2_MAX, 'ws %d seed %d: qact2 scale %g above 2^-2: choose another seed' % (ws, seed, s2)
            tab = R.softmax_table(s2)
            for tag, msk in (('nomask', None), ('mask', mask)):
                taps, hooks = {}, []

                def mk(name, mod):
                    def hook(_m, _inp, o):
                        taps[name] = torch.round(o / mod.quantizer.scale.reshape(G.oracle.act_shape(o) if o.dim() > 1 else (-1,))).to(torch.int16).numpy()
                    return hook
                for name, mod in m.named_modules():
                    if isinstance(mod, ref_models.QAct):
                        hooks.append(mod.register_forward_hook(mk(name, mod)))
                m(codes_ev * s_in, mask=msk)
                for h in hooks:
                    h.remove()
                # the canonical operator on the reference's own qact2 and qact1 codes
                B_ = BIMG * NW
                v = torch.from_numpy(taps['qact1'].astype(np.int64)).reshape(B_, N, 3, HEADS, DIM // HEADS).permute(2, 0, 3, 1, 4)[2]
                a2 = torch.from_numpy(taps['qact2'].astype(np.int64)).reshape(B_, HEADS, N, N)
                q3 = R.table_softmax_pv(a2, v, R.allowed_of_mask(msk, B_), tab, s1 / s3).transpose(1, 2).reshape(B_, N, DIM).numpy()
                d = q3 - taps['qact3'].reshape(B_, N, DIM).astype(np.int64)
                nd, n, mx = int((d != 0).sum()), int(d.size), int(np.abs(d).max())
                good = mx <= 1 and nd * 1000 <= CAP_PER_1000 * n
                ok = ok and good
                print('ws %2d seed %d %-6s: %d of %d qact3 codes differ (max %d)%s' % (ws, seed, tag, nd, n, mx, '' if good else '   <-- over the cap'))
                out[pre + 'stage_diff/' + tag] = np.array([nd, n, mx], dtype=np.int64)
                for k, val in taps.items():
                    if tag == 'mask' and k in ('qact1', 'qact_attn1', 'qact_table', 'qact2'):
                        assert np.array_equal(val, out[pre + 'taps/nomask/' + k].astype(val.dtype)), k     # in front of the mask: stored once
                        continue
                    out[pre + 'taps/%s/%s' % (tag, k)] = small(val)
        for name, s in scales.items():
            out[pre + 'scale/' + name] = s.numpy()
        for name, mod in q_mods.items():
            if isinstance(mod, ref_models.QLinear):
                for bt, s in mod.quantizer.dic_scale.items():
                    out[pre + 'wscale/%s/%s' % (name, bt)] = s.detach().float().reshape(-1).numpy()
        out[pre + 'x_ev'] = codes_ev.to(torch.int8).numpy()
        out[pre + 's_in'] = np.float32(s_in)
        out[pre + 'region'] = region.to(torch.int8).numpy()
        out[pre + 'softmax_table'] = tab.astype(np.uint32)
        out[pre + 'seed'] = np.int64(seed)
    assert ok, 'a case is over the cap (at most 1 code per 1 000, never by more than 1): choose another seed'
    path = os.path.join(G.GOLD, 'swin_winattn_softmax.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) <= (1 << 20), 'fixture over the size limit for a committed file'


if __name__ == '__main__':
    main()
