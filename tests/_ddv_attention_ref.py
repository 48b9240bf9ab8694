"""Expected values of the DDV stages INSIDE attention (P2V_DDV_STAGES_ATTN; Swin: the tapped window launches) from the oracle's existing
taps: a restatement for the tests in the style of tests/_ddv_full_ref.py, the oracle itself is not touched.

    ViT     blocks.i.attn.qact_attn1       = OracleViT tap 'attn.qact_attn1'   int8 score codes [B, H, N, N]
            blocks.i.attn.log_int_softmax  = tap 'attn.softmax_k'              exponents k; the VALUE is 2^-k, 0 from k = 16 on
    Swin    ...attn.qact_attn1 / attn.qact2 / attn.log_int_softmax = taps 'qact_attn1' / 'qact2' / 'softmax_k' of window_attention_quant on
            the tapped qact1 codes in window order, [B * nW, heads, N, N] regrouped per image

Both kinds of sums are exact integers: codes as int64 sums; exponents as int64 sums of 2^(15 - ka) * 2^(15 - kb), times 2^-30 (a power of
two: exact in fp64 while the integer is below 2^53, which a softmax row guarantees - its probabilities sum to about 1)."""
import numpy as np
import torch


def int_sums(a, b):
    """fp64 [n, 3] from integer codes [n, ...]: exact int64 sums, converted once"""
    n = a.shape[0]
    a, b = a.reshape(n, -1).to(torch.int64), b.reshape(n, -1).to(torch.int64)
    return torch.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], 1).numpy().astype(np.float64)


def log2k_units(k):
    """exponent bytes -> the probability in units of 2^-15 as int64: 2^(15 - k) for 0 <= k <= 15, 0 from 16 on (bytes read unsigned)"""
    k = k.to(torch.int64) & 255
    return torch.where(k < 16, torch.ones_like(k) << (15 - torch.clamp(k, max=15)), torch.zeros_like(k))


def log2k_sums(ka, kb):
    """fp64 [n, 3] from exponents [n, ...]: int64 sums of the unit products, scaled by 2^-30"""
    s = int_sums(log2k_units(ka), log2k_units(kb))
    assert float(s.max()) < 2.0 ** 53
    return s * 2.0 ** -30


def ddv_of(sums):
    """numpy's DDV of [n, 3] sums: cosines (0 / 0 = NaN) divided by their L2 norm where that is not zero"""
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = sums[:, 0] / (np.sqrt(sums[:, 1]) * np.sqrt(sums[:, 2]))
        norm = np.sqrt((cos * cos).sum())
        return cos / norm if norm != 0 else cos


def vit_attention_stages(O, arch, W, c, x, bits):
    """(name -> (values [2n, H, N, N], kind), all oracle taps, logits) with kind 'codes' or 'log2k'"""
    orc = O.OracleViT(arch, W)
    orc.calib = c
    taps = {}
    logits = orc.quant_forward(x, bits, taps)
    out = {}
    for i in range(arch['depth']):
        p = 'blocks.%d.attn.' % i
        out[p + 'qact_attn1'] = (taps[p + 'qact_attn1'], 'codes')
        out[p + 'log_int_softmax'] = (taps[p + 'softmax_k'], 'log2k')
    return out, taps, logits


def expected(values, kind):
    n = values.shape[0] // 2
    return (int_sums if kind == 'codes' else log2k_sums)(values[:n], values[n:])


def swin_attention_stages(m, x, bits):
    """name -> (values [2n, ...], kind) for the three stages of every block of the calibrated Swin model ``m`` (on the CPU), and the logits"""
    import swin_oracle as SO
    a, c = m.arch, m.export_calib()
    W = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    bt = 'int%d' % bits
    taps = {}
    logits = SO.OracleSwin(a, W).quant_forward(x, c, bits, taps)
    B = x.shape[0]
    H = a['img_size'] // a['patch_size']
    out = {}
    for li, depth in enumerate(a['depths']):
        Cc, heads, wsz = a['embed_dim'] * 2 ** li, a['num_heads'][li], min(a['window_size'], H)
        for bi in range(depth):
            p = 'layers.%d.blocks.%d.' % (li, bi)
            shift = 0 if (bi % 2 == 0 or H <= a['window_size']) else a['window_size'] // 2
            q1 = taps[p + 'qact1'].float()
            idx = SO.window_index(H, H, wsz, shift)
            xw = q1[:, idx.reshape(-1)].reshape(B * idx.shape[0], wsz * wsz, Cc)
            cw = {k: c[p + 'attn.' + k] for k in ('qact1', 'qact_attn1', 'qact_table', 'qact2', 'qact3', 'qact4')}
            cw['qkv'], cw['proj'] = c[p + 'attn.qkv'][bt], c[p + 'attn.proj'][bt]
            Wa = {k: W[p + 'attn.' + k] for k in ('qkv.weight', 'qkv.bias', 'proj.weight', 'proj.bias', 'relative_position_bias_table')}
            wt = {}
            SO.window_attention_quant(xw, float(c[p + 'qact1'].reshape(())), Wa, cw, heads, wsz,
                                      mask=SO.shifted_window_mask(H, H, wsz, shift) if shift else None, taps=wt, bits=bits)
            out[p + 'attn.qact_attn1'] = (wt['qact_attn1'].reshape(B, -1), 'codes')
            out[p + 'attn.qact2'] = (wt['qact2'].reshape(B, -1), 'codes')
            out[p + 'attn.log_int_softmax'] = (wt['softmax_k'].reshape(B, -1), 'log2k')
        if li < len(a['depths']) - 1:
            H //= 2
    return out, logits


def window_taps_reference(qkv, tab, heads, Hf, ws, shift, c):
    """the scores / softmax / AV part of swin_oracle.window_attention_quant on the partitioned windows of qact1 codes [B, T, 3C]:
    dict(idx, region, a1 / a2 / k [B, nW, heads, N, N] (qact_attn1 codes, qact2 codes in front of the mask, exponents), want [B, T, C])"""
    import p2vit_oracle as O
    import swin_oracle as SO
    B, T = qkv.shape[:2]
    C_, N = heads * 32, ws * ws
    idx = SO.window_index(Hf, Hf, ws, shift)
    nW = idx.shape[0]
    region = mask = None
    if shift:
        mask = SO.shifted_window_mask(Hf, Hf, ws, shift)
        img = torch.zeros(Hf, Hf)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[hs, wsl] = cnt
                cnt += 1
        region = img.reshape(Hf // ws, ws, Hf // ws, ws).permute(0, 2, 1, 3).reshape(nW, N).long()
    xw = qkv[:, idx.reshape(-1)].reshape(B * nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s1 = torch.tensor(c['qact1'])
    qs = (xw[0] * s1) * torch.tensor(32 ** -0.5, dtype=torch.float32)
    attn = (qs.double() @ (xw[1] * s1).double().transpose(-2, -1)).float()
    a1 = SO.q8(attn, c['qact_attn1'])
    bias = (tab * c['qact_table'])[SO.relative_position_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    a2 = SO.q8(a1 * c['qact_attn1'] + bias.unsqueeze(0), c['qact2'])
    xi = a2
    if mask is not None:
        xi = (a2.reshape(B, nW, heads, N, N) + torch.round(mask / c['qact2']).unsqueeze(1).unsqueeze(0)).reshape(B * nW, heads, N, N)
    k = O.lis_int(xi, torch.tensor([c['qact2']]))
    o = (O.lis_probs(k) @ (xw[2] * s1)).transpose(1, 2).reshape(B, nW * N, C_)
    want = torch.zeros(B, T, C_)
    want[:, idx.reshape(-1)] = SO.q8(o, c['qact3'])
    shape = (B, nW, heads, N, N)
    return dict(idx=idx, region=region, a1=a1.reshape(shape), a2=a2.reshape(shape), k=k.long().reshape(shape), want=want)
