"""Canonical semantics of the two float operators of Config(ptf=False) / Config(lis=False) and the whole model under them, for the tests:
a restatement built on ``p2vit_oracle``'s pieces (``qgemm``, ``weight_codes``, ``gelu_rn``, ``lis_int``, ``int_layernorm``); the oracle itself
is not touched.

Float LayerNorm -> QAct (QIntLayerNorm in mode 'ln', then / channel_scale, then the QAct).  A row of C int8 codes q_c under ONE
power-of-two input scale s_in; gamma, beta, eps fp32 widened to fp64; S1 = sum q, S2 = sum q^2 exact integers; in fp64, every operation
rounded on its own:
    var = ((C S2 - S1^2) / (C C)) s_in s_in;   r = 1 / sqrt(var + eps);   y_c = ((((C q_c - S1) / C) s_in) r) gamma_c + beta_c
    code_c = clamp(rne(y_c g_c), -128, 127),   g_c = 1 / (channel_scale_c s_out) a power of two
(numpy float64 throughout: its sqrt and division are the IEEE ones).

Softmax attention -> QAct (QIntSoftmax with log_i_softmax = False).  Score codes c_ij from the unchanged qact_attn1 requantisation;
    d_ij = max_j c_ij - c_ij;  E_ij = tab[d_ij];  num_ic = sum_j E_ij v_jc;  den_i = sum_j E_ij      (exact integers)
    code_ic = clamp(rne((double(num_ic) / double(den_i)) av_mul), -128, 127)
with tab[d] = min(rne(exp(-s_attn1 d) 2^21), 2^21 - 1) built in fp64 (``softmax_table``); the table is operator input.
"""
import numpy as np
import torch

BIT_POOL = [4, 8]
FRAC_BITS = 21
CONFIGS = {'ff': (False, False), 'tf': (True, False), 'ft': (False, True)}      # fixture tag -> Config(ptf, lis)
_FIXTURE = []


def fixture():
    """tests/golden/micro_vit_float_ops.npz (tools/gen_golden_float_ops.py: the REAL reference under the three configurations), loaded once"""
    import os
    if not _FIXTURE:
        _FIXTURE.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'micro_vit_float_ops.npz')))
    return _FIXTURE[0]


def fixture_calib(g, tag, O):
    pre = tag + '/calib/'
    return O.unflatten_calib({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})


def bit_lists(g, L):
    return {'q8': [8] * L, 'q4': [4] * L, 'qmix': [int(b) for b in g['bit_qmix']]}


def make_model(dva, arch, sd, tag, device='cpu'):
    """the product's VisionTransformer under the configuration of ``tag``, weights loaded, in eval mode on ``device``"""
    from functools import partial
    ptf, lis = CONFIGS[tag]
    m = dva.VisionTransformer(img_size=arch['img_size'], patch_size=arch['patch_size'], embed_dim=arch['embed_dim'], depth=arch['depth'],
                              num_heads=arch['num_heads'], num_classes=arch['num_classes'], mlp_ratio=arch['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config(ptf, lis))
    m.load_state_dict(sd, strict=False)
    return m.to(device).eval()


def softmax_table(s_attn):
    s = float(torch.as_tensor(s_attn).reshape(-1)[0])
    e = np.rint(np.exp(-s * np.arange(256, dtype=np.float64)) * float(1 << FRAC_BITS))
    return np.minimum(e, float((1 << FRAC_BITS) - 1)).astype(np.int64)


def float_layernorm(q, s_in, gamma, beta, eps, g):
    """q: integer codes [..., C] (any integer or float dtype holding integers); s_in, eps: python floats (fp32 values); gamma, beta, g:
    fp32 [C].  Returns (int64 codes [..., C], fp32 values RN32(y) [..., C]) as torch tensors."""
    qi = np.asarray(torch.as_tensor(q).to(torch.int64).numpy())
    C = qi.shape[-1]
    S1 = qi.sum(-1, keepdims=True)
    S2 = (qi * qi).sum(-1, keepdims=True)
    s_in = np.float64(np.float32(s_in))
    eps = np.float64(np.float32(eps))
    gm = np.asarray(gamma.detach().float().numpy(), dtype=np.float64).reshape(-1)
    bt = np.asarray(beta.detach().float().numpy(), dtype=np.float64).reshape(-1)
    gg = np.asarray(g.detach().float().numpy(), dtype=np.float64).reshape(-1)
    Cd = np.float64(C)
    var = (((C * S2 - S1 * S1).astype(np.float64) / (Cd * Cd)) * s_in) * s_in
    r = np.float64(1.0) / np.sqrt(var + eps)
    y = ((((C * qi - S1).astype(np.float64) / Cd) * s_in) * r) * gm + bt
    codes = np.clip(np.rint(y * gg), -128, 127).astype(np.int64)
    return torch.from_numpy(codes), torch.from_numpy(y.astype(np.float32))


def softmax_attention(score_codes, v_codes, tab, av_mul):
    """score_codes int [..., N, N], v_codes int [..., N, hd], tab int64 [256], av_mul a python float (a power of two) ->
    int64 codes [..., N, hd]"""
    sc = score_codes.to(torch.int64)
    d = sc.max(dim=-1, keepdim=True)[0] - sc
    E = torch.as_tensor(np.asarray(tab, dtype=np.int64))[d]
    # integer sums of products below 2^21 * 2^7 * tokens < 2^53: exact in fp64 whatever the order (the fp64 GEMM is only the fast way to them)
    assert sc.shape[-1] < (1 << 20)
    num = E.double() @ v_codes.double()
    den = E.sum(-1, keepdim=True)
    val = (num.numpy() / den.numpy().astype(np.float64)) * np.float64(av_mul)
    return torch.from_numpy(np.clip(np.rint(val), -128, 127).astype(np.int64))


def score_codes(O, q_codes, k_codes, s_q1, s_at, hd):
    """the existing score requantisation (p2vit_oracle.quant_forward): exact integer q.k, * s_q1^2, * head_dim^-0.5, qact_attn1"""
    acc = q_codes.float() @ k_codes.float().transpose(-2, -1)
    attn = (acc * (s_q1 * s_q1)) * (hd ** -0.5)
    return torch.clamp(torch.round(attn / s_at), -128, 127)


def _q8(v, s):
    return torch.clamp(torch.round(v / s), -128, 127)


def quant_forward(O, arch, W, c, x, bit_config, int_norm, int_softmax, ln_eps=1e-6, taps=None, stages=None):
    """``OracleViT.quant_forward`` (same statements, same order) with the LayerNorm and the softmax chosen by (int_norm, int_softmax).
    taps: name -> integer codes (the oracle's names).  stages: name -> (values, per-channel scale or None, kind), the DDV stages of
    ``ddv.stage_names(depth, False, full=True)``; kind says how the engine reduces the stage (``check_stage``)."""
    D, H, depth = arch['embed_dim'], arch['num_heads'], arch['depth']
    hd = D // H
    assert len(bit_config) == 4 * depth + 2

    def tap(name, t):
        if taps is not None:
            taps[name] = t.to(torch.int32)

    def stage(name, v, scale=None, kind=None):
        if stages is not None:
            stages[name] = (v, scale, kind or ('f32' if v.dtype.is_floating_point else ('codes' if scale is None else 'per_channel')))

    def per_ch(s):
        return s.reshape(-1).expand(D) if s.numel() == 1 else s.reshape(-1)

    def norm(codes, s_res, gamma, beta, out_scale, g, name):
        """-> the fp32 value h the oracle forms behind the LayerNorm (in front of / channel_scale and the QAct), or for the float
        LayerNorm the codes themselves; returns q0 codes [B, N, D]"""
        if int_norm:
            xv = codes * s_res.reshape(1, 1, -1)
            n = O.int_layernorm(xv, s_res, gamma, beta, out_scale)
            stage(name, n * out_scale.reshape(1, 1, -1))
            return n, True
        s = s_res.reshape(-1)
        assert float(s.min()) == float(s.max())
        q0, y32 = float_layernorm(codes, float(s[0]), gamma, beta, ln_eps, g)
        stage(name, y32)
        return q0.float(), False

    s_in = c['qact_input']
    q = _q8(x, s_in)
    tap('qact_input', q)
    stage('qact_input', q.to(torch.int32))
    bit = bit_config[0]
    s_w = c['patch_embed.proj']['int%d' % bit]
    wq = O.weight_codes(W['patch_embed.proj.weight'], None, s_w, bit)
    P = arch['patch_size']
    Bn = x.shape[0]
    cols = torch.nn.functional.unfold(q, kernel_size=P, stride=P).transpose(1, 2)
    y = O.qgemm(cols.reshape(-1, cols.shape[-1]), s_in, wq, s_w.reshape(-1), W['patch_embed.proj.bias']).reshape(Bn, -1, D)
    s_pe = c['patch_embed.qact']
    xv = _q8(y, s_pe) * s_pe
    tap('patch_embed.qact', _q8(y, s_pe))
    stage('patch_embed.qact', _q8(y, s_pe).to(torch.int32))
    xv = torch.cat((W['cls_token'].expand(Bn, -1, -1), xv), dim=1)
    s_e = c['qact_embed']
    stage('qact_embed', _q8(xv, s_e).to(torch.int32))
    xv = _q8(xv, s_e) * s_e
    s_p = c['qact_pos']
    xv = xv + _q8(W['pos_embed'], s_p) * s_p
    s_res = per_ch(c['qact1'])
    qr = _q8(xv, s_res.reshape(1, 1, -1))
    tap('qact1', qr)
    stage('qact1', qr.to(torch.int32), s_res)
    xv = qr * s_res.reshape(1, 1, -1)

    for i in range(depth):
        p = 'blocks.%d.' % i
        bits = bit_config[4 * i + 1: 4 * i + 5]
        bi = BIT_POOL.index(bits[0])
        cs = c[p + 'attn.best_scale'][bi]
        s_a0 = c[p + 'attn.best_act_scale'][bi]
        s_wq = c[p + 'attn.best_weight_scale'][bi]['int%d' % bits[0]]
        o1 = per_ch(s_a0 * cs)
        n, is_int = norm(qr, s_res, W[p + 'norm1.weight'], W[p + 'norm1.bias'], o1, 1.0 / per_ch(cs * s_a0), p + 'norm1')
        q0 = _q8((n * o1.reshape(1, 1, -1)) / cs.reshape((1, 1, -1)), s_a0) if is_int else n
        tap(p + 'attn.qact0', q0)
        wq = O.weight_codes(W[p + 'attn.qkv.weight'], cs, s_wq, bits[0])
        N = q0.shape[1]
        y = O.qgemm(q0.reshape(-1, D), s_a0, wq, s_wq.reshape(-1), W[p + 'attn.qkv.bias']).reshape(Bn, N, 3 * D)
        s_q1 = c[p + 'attn.qact1']
        q1 = _q8(y, s_q1)
        tap(p + 'attn.qact1', q1)
        stage(p + 'attn.qact1', q1.to(torch.int32))
        qkv = q1.reshape(Bn, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        s_at = c[p + 'attn.qact_attn1']
        sc = score_codes(O, qkv[0], qkv[1], s_q1, s_at, hd)
        tap(p + 'attn.qact_attn1', sc)
        s_a2 = c[p + 'attn.qact2']
        if int_softmax:
            k = O.lis_int(sc, s_at)
            o = (O.lis_probs(k) @ (qkv[2] * s_q1)).transpose(1, 2).reshape(Bn, N, D)
            q2 = _q8(o, s_a2)
        else:
            q2 = softmax_attention(sc, qkv[2], softmax_table(s_at), float(s_q1 / s_a2)).transpose(1, 2).reshape(Bn, N, D).float()
        tap(p + 'attn.qact2', q2)
        stage(p + 'attn.qact2', q2.to(torch.int32))
        s_wp = c[p + 'attn.proj']['int%d' % bits[1]]
        wq = O.weight_codes(W[p + 'attn.proj.weight'], None, s_wp, bits[1])
        y = O.qgemm(q2.reshape(-1, D), s_a2, wq, s_wp.reshape(-1), W[p + 'attn.proj.bias']).reshape(Bn, N, D)
        s_a3 = per_ch(c[p + 'attn.qact3']).reshape(1, 1, -1)
        q3 = _q8(y, s_a3)
        tap(p + 'attn.qact3', q3)
        stage(p + 'attn.qact3', q3.to(torch.int32), s_a3.reshape(-1), 'deq')
        s_b2 = per_ch(c[p + 'qact2'])
        qr = _q8(xv + q3 * s_a3, s_b2.reshape(1, 1, -1))
        tap(p + 'qact2', qr)
        stage(p + 'qact2', qr.to(torch.int32), s_b2)
        xv = qr * s_b2.reshape(1, 1, -1)
        s_res = s_b2
        bm = BIT_POOL.index(bits[2])
        cs_m = c[p + 'mlp.best_scale'][bm]
        s_m0 = c[p + 'mlp.best_act_scale'][bm]
        s_w1 = c[p + 'mlp.best_weight_scale'][bm]['int%d' % bits[2]]
        o2 = per_ch(s_m0 * cs)                       # the ATTENTION's channel scale, vit_fquant.py:464
        n, is_int = norm(qr, s_res, W[p + 'norm2.weight'], W[p + 'norm2.bias'], o2, 1.0 / per_ch(cs_m * s_m0), p + 'norm2')
        q0 = _q8((n * o2.reshape(1, 1, -1)) / cs_m.reshape((1, 1, -1)), s_m0) if is_int else n
        tap(p + 'mlp.qact0', q0)
        wq = O.weight_codes(W[p + 'mlp.fc1.weight'], cs_m, s_w1, bits[2])
        y = O.qgemm(q0.reshape(-1, D), s_m0, wq, s_w1.reshape(-1), W[p + 'mlp.fc1.bias'])
        s_m1 = c[p + 'mlp.qact1']
        q1 = _q8(O.gelu_rn(y), s_m1)
        tap(p + 'mlp.qact1', q1.reshape(Bn, N, -1))
        stage(p + 'mlp.qact1', q1.reshape(Bn, N, -1).to(torch.int32))
        s_w2 = c[p + 'mlp.fc2']['int%d' % bits[3]]
        wq = O.weight_codes(W[p + 'mlp.fc2.weight'], None, s_w2, bits[3])
        y = O.qgemm(q1, s_m1, wq, s_w2.reshape(-1), W[p + 'mlp.fc2.bias']).reshape(Bn, N, D)
        s_m2 = per_ch(c[p + 'mlp.qact2']).reshape(1, 1, -1)
        q2 = _q8(y, s_m2)
        tap(p + 'mlp.qact2', q2)
        stage(p + 'mlp.qact2', q2.to(torch.int32), s_m2.reshape(-1), 'deq')
        s_b4 = per_ch(c[p + 'qact4'])
        qr = _q8(xv + q2 * s_m2, s_b4.reshape(1, 1, -1))
        tap(p + 'qact4', qr)
        stage(p + 'qact4', qr.to(torch.int32), s_b4)
        xv = qr * s_b4.reshape(1, 1, -1)
        s_res = s_b4

    s_f = c['qact2']
    sfD = per_ch(s_f)
    n, is_int = norm(qr, s_res, W['norm.weight'], W['norm.bias'], sfD, 1.0 / sfD, 'norm')     # every row: the hook sits in front of [:, 0]
    qf = _q8(n[:, 0] * s_f, s_f) if is_int else n[:, 0]
    tap('qact2', qf)
    stage('qact2', qf.reshape(Bn, 1, D).to(torch.int32))
    bit = bit_config[-1]
    s_wh = c['head']['int%d' % bit]
    wq = O.weight_codes(W['head.weight'], None, s_wh, bit)
    y = O.qgemm(qf, s_f, wq, s_wh.reshape(-1), W['head.bias'])
    s_o = c['act_out']
    ql = _q8(y, s_o)
    tap('act_out', ql)
    stage('act_out', (ql * s_o).reshape(Bn, 1, -1))
    return ql * s_o


def check_stage(name, got, values, scale, kind, tag=''):
    """sums [n, 3] of one DDV stage of the engine against the stage's values [2n, ...], with the tolerances of tests/test_ddv_gpu.py and
    tests/test_ddv_full_gpu.py:
      codes        int8 codes under one scale: exact integer sums, bit for bit
      per_channel  int8 codes under per-channel scales: exact per-channel integer sums times s_c^2 in fp64, 1e-12 relative
      deq          int8 codes as the fp32 products code * s_c a fake-quantising QAct returns, summed in fp64, 1e-12 relative
      f32          fp32 values summed in fp64 in another order, 1e-9 of sqrt(aa bb)"""
    n = values.shape[0] // 2

    def isums(a, b):
        a, b = a.to(torch.int64), b.to(torch.int64)
        return torch.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], -1).numpy()

    if kind == 'codes':
        want = isums(values[:n].reshape(n, -1), values[n:].reshape(n, -1)).astype(np.float64)
        print(tag, name, 'codes, equal =', np.array_equal(got, want))
        assert np.array_equal(got, want), (tag, name)
        return
    if kind == 'per_channel':
        C = values.shape[-1]
        pc = isums(values[:n].reshape(n, -1, C), values[n:].reshape(n, -1, C)).astype(np.float64)            # [n, C, 3]
        want = (pc * (scale.double().numpy().reshape(-1) ** 2)[None, :, None]).sum(1)
        tol = 1e-12
    else:
        v = values.float() * scale.float().reshape(1, 1, -1) if kind == 'deq' else values
        a, b = v[:n].double().reshape(n, -1), v[n:].double().reshape(n, -1)
        want = torch.stack([(a * b).sum(1), (a * a).sum(1), (b * b).sum(1)], 1).numpy()
        tol = 1e-12 if kind == 'deq' else 1e-9
    root = np.sqrt(want[:, 1] * want[:, 2])
    err = max(float((np.abs(got[:, 1] - want[:, 1]) / want[:, 1]).max()), float((np.abs(got[:, 2] - want[:, 2]) / want[:, 2]).max()),
              float((np.abs(got[:, 0] - want[:, 0]) / root).max()))
    print(tag, name, kind, 'max relative error =', err)
    assert err <= tol, (tag, name, kind, err)
