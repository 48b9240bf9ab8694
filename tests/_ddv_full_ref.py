"""Expected values of the FULL DDV stages (P2V_DDV_STAGES_FULL) from the oracle's existing taps plus ``p2vit_oracle.int_layernorm``: a
restatement for the tests, the oracle itself is not touched.

``full_stage_values`` returns, per new stage name, (values [2n, ...], per-channel scale or None):
    qact_input / patch_embed.qact / qact_embed     integer codes, one scale (a cosine does not see it)
    blocks.i.attn.qact3 / mlp.qact2                integer codes with their per-channel PTF scale; the stage's VALUES are the fp32 products
                                                   q8(y, s_mid[c]) * s_mid[c] the fake-quantising QAct returns (the scales are no powers
                                                   of two, so the product rounds: summing exact code * scale instead moves a DDV entry of
                                                   the micro fixture by up to 1.9e-9, past the 1e-9 that pins the reference)
    blocks.i.norm1 / norm2 / norm                  fp32: the UNCLAMPED integer of QIntLayerNorm times its per-channel out_scale
                                                   (layers.py:288-289), every row
and the unclamped integers of the block norms, for the precondition that a clamped tap would be told apart."""
import numpy as np
import torch

BIT_POOL = [4, 8]


def _q8(v, s):
    return torch.clamp(torch.round(v / s), -128, 127)


def full_stage_values(O, arch, W, c, x, bits):
    orc = O.OracleViT(arch, W)
    orc.calib = c
    taps = {}
    logits = orc.quant_forward(x, bits, taps)
    D, depth = arch['embed_dim'], arch['depth']
    B = x.shape[0]
    out, block_norm_ints = {}, []
    out['qact_input'] = (taps['qact_input'], None)
    pe = taps['patch_embed.qact']
    out['patch_embed.qact'] = (pe, None)
    xv = torch.cat((W['cls_token'].expand(B, -1, -1), pe.float() * c['patch_embed.qact']), dim=1)     # vit_fquant.py:718-720
    out['qact_embed'] = (_q8(xv, c['qact_embed']).to(torch.int32), None)
    codes, s_res = taps['qact1'], c['qact1']
    for i in range(depth):
        p = 'blocks.%d.' % i
        bi, bm = BIT_POOL.index(bits[4 * i + 1]), BIT_POOL.index(bits[4 * i + 3])
        cs = c[p + 'attn.best_scale'][bi]
        o1 = (c[p + 'attn.best_act_scale'][bi] * cs).reshape(-1).expand(D)
        v = codes.float() * s_res.reshape(1, 1, -1)
        n1 = O.int_layernorm(v, s_res, W[p + 'norm1.weight'], W[p + 'norm1.bias'], o1)
        out[p + 'norm1'] = (n1 * o1.reshape(1, 1, -1), None)
        out[p + 'attn.qact3'] = (taps[p + 'attn.qact3'], c[p + 'attn.qact3'].reshape(-1))
        codes, s_res = taps[p + 'qact2'], c[p + 'qact2']
        o2 = (c[p + 'mlp.best_act_scale'][bm] * cs).reshape(-1).expand(D)            # the ATTENTION's channel scale, vit_fquant.py:464
        v = codes.float() * s_res.reshape(1, 1, -1)
        n2 = O.int_layernorm(v, s_res, W[p + 'norm2.weight'], W[p + 'norm2.bias'], o2)
        out[p + 'norm2'] = (n2 * o2.reshape(1, 1, -1), None)
        out[p + 'mlp.qact2'] = (taps[p + 'mlp.qact2'], c[p + 'mlp.qact2'].reshape(-1))
        codes, s_res = taps[p + 'qact4'], c[p + 'qact4']
        block_norm_ints += [n1, n2]
    s_f = c['qact2'].reshape(-1).expand(D)
    v = codes.float() * s_res.reshape(1, 1, -1)
    nf = O.int_layernorm(v, s_res, W['norm.weight'], W['norm.bias'], s_f)
    out['norm'] = (nf * s_f.reshape(1, 1, -1), None)                                 # every row: the hook sits in front of [:, 0]
    return out, block_norm_ints, taps, logits


def load_reference_calibration(model, c):
    """the QAct scales of the fixture's calibration (the REAL reference's, tests/golden/micro_vit.npz) into a calibrated model.  The PTF
    base scales of attn.qact3 / mlp.qact2 come from a min / max over float GEMM outputs, and a host's or the GPU's BLAS moves them by an
    fp32 ulp (1e-7 relative on all 64 channels of three layers of the micro model): the codes stay the reference's, but every VALUE
    code * scale moves with the scale, and a DDV entry by ~1e-9.  A comparison with the reference's DDVs at 1e-9 needs its scales."""
    mods = dict(model.named_modules())
    changed = 0
    for name, v in c.items():
        if torch.is_tensor(v) and name in mods and getattr(mods[name], 'quantizer', None) is not None:
            q = mods[name].quantizer
            new = v.to(q.scale.device, q.scale.dtype).reshape(q.scale.shape)
            changed += int(not torch.equal(new, q.scale))
            q.scale = new
    model._plan = None
    return changed


def int_sums(x, y, per_channel=False):
    """int64 sums of integer codes [n, rows, cols]: [n, 3], or [n, cols, 3] per channel"""
    x, y = x.cpu().to(torch.int32), y.cpu().to(torch.int32)
    pc = torch.stack([(x * y).sum(1, dtype=torch.int64), (x * x).sum(1, dtype=torch.int64), (y * y).sum(1, dtype=torch.int64)], -1)
    return (pc if per_channel else pc.sum(1)).numpy()


def expected_sums(values, scale):
    """fp64 [n, 3] = (sum a.b, sum a.a, sum b.b) of one stage from its [2n, ...] values: exact integer sums for one-scale codes, fp64 sums
    of the fp32 values otherwise (codes with per-channel scales: of the fp32 products code * scale[c])"""
    n = values.shape[0] // 2
    if scale is not None:
        values = values.float() * scale.float().reshape(1, 1, -1)
    a, b = values[:n], values[n:]
    if values.dtype.is_floating_point:
        a, b = a.double().reshape(n, -1), b.double().reshape(n, -1)
        return torch.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], 1).numpy()
    return int_sums(a.reshape(n, 1, -1), b.reshape(n, 1, -1)).astype(np.float64)


def check_stage(name, got, values, scale, tag=''):
    """the tolerances of test_ddv_gpu.py: bit-equal integer sums for one-scale codes, 1e-12 relative for per-channel codes, 1e-9 of
    sqrt(aa bb) for fp32 values (F <= 2^20 features in two orders)"""
    want = expected_sums(values, scale)
    if values.dtype.is_floating_point and scale is None:
        root = np.sqrt(want[:, 1:2] * want[:, 2:3])
        err = float((np.abs(got - want) / root).max())
        print(tag, name, 'fp32 stage, max error / sqrt(aa bb) =', err)
        assert err <= 1e-9, (tag, name, err)
    elif scale is None:
        print(tag, name, 'one-scale codes, equal =', np.array_equal(got, want))
        assert np.array_equal(got, want), (tag, name)
    else:
        root = np.sqrt(want[:, 1] * want[:, 2])
        e = max(float((np.abs(got[:, 1] - want[:, 1]) / want[:, 1]).max()), float((np.abs(got[:, 2] - want[:, 2]) / want[:, 2]).max()),
                float((np.abs(got[:, 0] - want[:, 0]) / root).max()))
        print(tag, name, 'per-channel codes, max relative error =', e)
        assert e <= 1e-12, (tag, name, e)


def ddv_of(values, scale):
    """the reference's DDV of a stage from its expected sums (fp64)"""
    s = expected_sums(values, scale)
    cos = s[:, 0] / (np.sqrt(s[:, 1]) * np.sqrt(s[:, 2]))
    norm = np.sqrt((cos * cos).sum())
    return cos / norm if norm != 0 else cos
