"""``torch.ops.p2vit.*``: the C-ABI entry points registered as PyTorch custom ops ("bound via
torch.library custom ops").  Each op is a thin argument adapter over ``engine.lib()``; tensors are int8 code tensors or
fp32 parameter vectors on the GPU, results are freshly allocated tensors on the same device and stream.  There is no CPU
kernel behind any of them: calling one with CPU tensors raises ``NotImplementedError`` from the dispatcher, and calling
one without the built library raises ``RuntimeError`` from ``engine.lib()``.

    torch.ops.p2vit.fake_quant(x, scale, inner, lo, hi)                         UniformQuantizer.forward   quantizer/uniform.py:82-88
    torch.ops.p2vit.quantize_patchify(images, inv_s, patch)                     qact_input + im2col        vit_fquant.py:705, layers.py:55-88
    torch.ops.p2vit.linear_requant(x, w, colscale, bias, inv_s_out)             QLinear + QAct             layers.py:133-178, 207-220
    torch.ops.p2vit.linear_gelu_requant(x, w, colscale, bias, inv_s_out)        fc1 + GELU + qact1         layers_quant.py:304-351
    torch.ops.p2vit.int_layernorm(x, s1, mask, gamma, beta, inv_out, post_mul)  QIntLayerNorm 'int'        layers.py:255-289
    torch.ops.p2vit.lis_attention(qkv, heads, s_qkv_sq, qk_scale, inv_s_attn, av_mul, x0, b, c)   vit_fquant.py:309-326, layers.py:323-376
    torch.ops.p2vit.forward(plan_handle, images, bit_config)                    VisionTransformer.forward  vit_fquant.py:780-799
    torch.ops.p2vit.cka_grams(xs, ys)                                           _generate_gram_matrix      efficient_CKA.py:23-39
    torch.ops.p2vit.hsic_accumulate(g1, g2, acc, self1, self2)                  update_state*              efficient_CKA.py:41-58
    torch.ops.p2vit.pair_cosine(a, b, scales)                                   per-sample cosine sums     modeldiff_p2.py:101-108
    torch.ops.p2vit.score_logits(logits, labels)                                tie-aware ranks + fp64 loss  test_quant.py:430-436, 488-501
    torch.ops.p2vit.score_accumulate(ranks, loss, ks, totals)                   running totals of a pass   test_quant.py:437-439
    torch.ops.p2vit.code_stats(tensors)                                         per-channel ranges, histogram, sums   plot_distrib.py:30-61
    torch.ops.p2vit.code_grams(tensors, shifts)                                 raw fp64 Grams X X^T of codes / values   DDV_CKA.py (MinibatchAdvCKA)
    torch.ops.p2vit.cka_centre(raw)                                             the centring of _generate_gram_matrix   efficient_CKA.py:28-39
    torch.ops.p2vit.patch_similarity_entropy(av, groups)                        entropy term and its gradient   generate_data.py:102-113, 128-134
    torch.ops.p2vit.rademacher_fill(tensors, layers, seed, probe)               the +-1 probe vectors of all tensors   pyhessian/hessian.py:184-190
    torch.ops.p2vit.group_dot(a, b)                                             fp64 sum(a * b) per tensor pair   pyhessian/utils.py:27-34
    torch.ops.p2vit.hutchinson_init(state, n_layers)                            clears the stopping state
    torch.ops.p2vit.hutchinson_step(a, b, probe, tol, record, state)            group_dot + the stopping rule per layer   pyhessian/hessian.py:196-204
"""
import ctypes as C

import torch

from . import engine as E

_LIB = torch.library.Library('p2vit', 'DEF')
_LIB.define('fake_quant(Tensor x, Tensor scale, int inner, int lo, int hi) -> Tensor')
_LIB.define('quantize_patchify(Tensor images, float inv_s, int patch) -> Tensor')
_LIB.define('linear_requant(Tensor x, Tensor w, Tensor colscale, Tensor bias, float inv_s_out) -> Tensor')
_LIB.define('linear_gelu_requant(Tensor x, Tensor w, Tensor colscale, Tensor bias, float inv_s_out) -> Tensor')
_LIB.define('int_layernorm(Tensor x, float s1, Tensor mask, Tensor gamma, Tensor beta, Tensor inv_out, Tensor post_mul) -> Tensor')
_LIB.define('lis_attention(Tensor qkv, int heads, float s_qkv_sq, float qk_scale, float inv_s_attn, float av_mul, int x0, int b, int c) -> Tensor')
_LIB.define('lis_attention_rows(Tensor qkv, int heads, float s_qkv_sq, float qk_scale, float inv_s_attn, float av_mul, int x0, int b, int c, '
            'int query_rows) -> Tensor')
_LIB.define('forward(int plan, Tensor images, int[] bit_config) -> Tensor')
_LIB.define('cka_grams(Tensor[] xs, Tensor[] ys) -> Tensor')
_LIB.define('hsic_accumulate(Tensor g1, Tensor g2, Tensor(a!) acc, Tensor(b!)? self1, Tensor(c!)? self2) -> ()')
_LIB.define('pair_cosine(Tensor[] a, Tensor[] b, Tensor?[] scales) -> Tensor')
_LIB.define('score_logits(Tensor logits, Tensor labels) -> (Tensor ranks, Tensor loss)')
_LIB.define('score_accumulate(Tensor ranks, Tensor loss, int[] ks, Tensor(a!) totals) -> ()')
_LIB.define('code_stats(Tensor[] tensors) -> Tensor[]')
_LIB.define('code_grams(Tensor[] tensors, Tensor?[] shifts) -> Tensor')
_LIB.define('cka_centre(Tensor raw) -> Tensor')
_LIB.define('patch_similarity_entropy(Tensor av, int groups) -> (Tensor value, Tensor grad)')
_LIB.define('rademacher_fill(Tensor(a!)[] tensors, int[] layers, int seed, int probe) -> ()')
_LIB.define('group_dot(Tensor[] a, Tensor[] b) -> Tensor')
_LIB.define('hutchinson_init(Tensor(a!) state, int n_layers) -> ()')
_LIB.define('hutchinson_step(Tensor[] a, Tensor[] b, int probe, float tol, Tensor(a!) record, Tensor(b!) state) -> ()')


def _f32(t):
    return t.contiguous().float()


def _fake_quant(x, scale, inner, lo, hi):
    x, scale = _f32(x), _f32(scale)
    out = torch.empty_like(x)
    E.check(E.lib().p2v_fake_quant_f32(E.ptr(x), x.numel(), E.ptr(scale), scale.numel(), inner, lo, hi, E.ptr(out), None,
                                       E.stream_ptr()))
    return out


def _quantize_patchify(images, inv_s, patch):
    images = _f32(images)
    B, Cin, H, W = images.shape
    k = Cin * patch * patch
    k_pad = (k + 63) // 64 * 64
    out = torch.zeros(B * (H // patch) * (W // patch), k_pad, dtype=torch.int8, device=images.device)
    E.check(E.lib().p2v_quantize_patchify(E.ptr(images), B, Cin, H, W, patch, inv_s, E.ptr(out), k_pad, E.stream_ptr()))
    return out


def _linear(kind, x, w, colscale, bias, inv_s_out):
    x = x.contiguous()
    M, K = x.shape
    N = w.shape[0]
    n_pad = (N + 127) // 128 * 128            # the GEMM stages whole 128-row weight tiles
    wp = torch.zeros(n_pad, K, dtype=torch.int8, device=x.device)
    wp[:N] = w
    w = wp
    cs = torch.zeros(n_pad, device=x.device)
    cs[:N] = colscale
    bs = torch.zeros(n_pad, device=x.device)
    bs[:N] = bias
    colscale, bias = cs, bs
    lin = E.Linear(E.ptr(w), E.ptr(colscale), E.ptr(bias))
    epi = E.Epilogue()
    epi.inv_s_out = inv_s_out
    out = torch.empty(M, N, dtype=torch.int8, device=x.device)
    E.check(E.lib().p2v_gemm_i8(kind, E.ptr(x), K, M, K, N, C.byref(lin), C.byref(epi), E.ptr(out), N, None, E.stream_ptr()))
    return out


def _int_layernorm(x, s1, mask, gamma, beta, inv_out, post_mul):
    x = x.contiguous()
    rows, Cc = x.shape
    keep = [_f32(t) for t in (mask, gamma, beta, inv_out, post_mul)]
    ln = E.Ln(s1, *[E.ptr(t) for t in keep])
    out = torch.empty_like(x)
    E.check(E.lib().p2v_int_layernorm(E.ptr(x), Cc, rows, Cc, C.byref(ln), E.ptr(out), Cc, E.stream_ptr()))
    return out


def _lis_attention(qkv, heads, s_qkv_sq, qk_scale, inv_s_attn, av_mul, x0, b, c):
    qkv = qkv.contiguous()
    B, N, D3 = qkv.shape
    D = D3 // 3
    at = E.Attn(s_qkv_sq, qk_scale, inv_s_attn, av_mul, x0, b, c)
    out = torch.empty(B, N, D, dtype=torch.int8, device=qkv.device)
    E.check(E.lib().p2v_lis_attention(E.ptr(qkv), B, N, heads, D // heads, C.byref(at), E.ptr(out), None, E.stream_ptr()))
    return out


def _lis_attention_rows(qkv, heads, s_qkv_sq, qk_scale, inv_s_attn, av_mul, x0, b, c, query_rows):
    """``lis_attention`` for the first ``query_rows`` query tokens of every image (all keys): [B, query_rows, D]."""
    qkv = qkv.contiguous()
    B, N, D3 = qkv.shape
    D = D3 // 3
    at = E.Attn(s_qkv_sq, qk_scale, inv_s_attn, av_mul, x0, b, c)
    out = torch.zeros(B, N, D, dtype=torch.int8, device=qkv.device)     # the kernel works in 16-row blocks: rows past them stay untouched
    E.check(E.lib().p2v_lis_attention_rows(E.ptr(qkv), B, N, heads, D // heads, C.byref(at), query_rows, E.ptr(out), E.stream_ptr()))
    return out[:, :query_rows].contiguous()


_PLANS = {}          # handle -> FrozenPlan, filled by plan.FrozenPlan (weak registry of live plans)


def _forward(plan, images, bit_config):
    p = _PLANS.get(plan)
    if p is None:
        raise RuntimeError('p2vit::forward: %d is not a live plan handle' % plan)
    return p.forward(images, list(bit_config))


def _cka_rows(x, n):
    """(tensor kept alive, row stride) of ``x`` viewed as n rows of F = x[0].numel() fp32 features, without a copy where the rows
    already lie in memory one after another (any feature order: a Gram matrix does not depend on it), e.g. the permuted
    [B, D, H/P, W/P] patch-embed tap."""
    if x.dim() == 0 or x.shape[0] != n:
        raise AssertionError('cka_grams: every activation needs %d rows (got shape %s)' % (n, tuple(x.shape)))
    x = x.float()
    F = x[0].numel()
    if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= F:
        return x, x.stride(0)
    order = [0] + sorted(range(1, x.dim()), key=lambda d: -x.stride(d))
    if x.stride(0) == F and x.permute(order).is_contiguous():
        return x, F
    return x.reshape(n, -1).contiguous(), F


def _cka_grams(xs, ys):
    if not xs:
        raise AssertionError('cka_grams: no layers')
    if ys and len(ys) != len(xs):
        raise AssertionError('cka_grams: %d x layers but %d y layers' % (len(xs), len(ys)))
    n, dev = xs[0].shape[0] if xs[0].dim() else 0, xs[0].device
    keep, descs = [], (E.CkaLayer * len(xs))()
    for k, x in enumerate(xs):
        xt, ldx = _cka_rows(x, n)
        keep.append(xt)
        d = descs[k]
        d.x, d.features, d.ldx = xt.data_ptr(), xt[0].numel(), ldx
        if ys:
            if tuple(ys[k].shape[1:]) != tuple(x.shape[1:]) and ys[k][0].numel() != xt[0].numel():
                raise AssertionError('cka_grams: layer %d: x and y differ in features' % k)
            yt, ldy = _cka_rows(ys[k], n)
            keep.append(yt)
            d.y, d.ldy = yt.data_ptr(), ldy
        for t in keep[-2:]:
            if t.device != dev:
                raise AssertionError('cka_grams: every activation must be on %s' % dev)
    L = E.lib()
    with torch.cuda.device(dev):
        nbytes = L.p2v_cka_workspace_bytes(descs, len(xs), n)
        if nbytes == 0:
            E.check(L.p2v_cka_grams(descs, len(xs), n, None, None, 0, None))       # raises with the validation message
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(len(xs), n, n, dtype=torch.float32, device=dev)
        E.check(L.p2v_cka_grams(descs, len(xs), n, E.ptr(out), E.ptr(ws), nbytes, E.stream_ptr(dev)))
    return out


def _hsic_accumulate(g1, g2, acc, self1, self2):
    dt = {torch.float32: 0, torch.float64: 1}.get(acc.dtype)
    if dt is None:
        raise AssertionError('hsic_accumulate: the accumulators are fp32 or fp64')
    n = g1.shape[-1]                          # grams [layers][n][n]
    l1, l2 = g1.shape[0], g2.shape[0]
    for t, shp in ((acc, (l1, l2)), (self1, (l1,)), (self2, (l2,))):
        if t is not None and (tuple(t.shape) != shp or t.dtype != acc.dtype or not t.is_contiguous() or t.device != g1.device):
            raise AssertionError('hsic_accumulate: accumulator of shape %s, dtype %s, contiguous, on %s expected' % (shp, acc.dtype, g1.device))
    g1, g2 = g1.float().contiguous(), g2.float().contiguous()
    if g1.numel() != l1 * n * n or g2.numel() != l2 * n * n:
        raise AssertionError('hsic_accumulate: grams must be [layers][n][n]')
    with torch.cuda.device(g1.device):
        E.check(E.lib().p2v_hsic_accumulate(E.ptr(g1), l1, E.ptr(g2), l2, n, E.ptr(acc), E.ptr(self1), E.ptr(self2), dt,
                                            E.stream_ptr(g1.device)))


def _cos_view(t, n):
    """(tensor kept alive, rows, cols, sample stride, row stride) of ``t`` as n samples of rows x cols int8 codes / fp32 values with
    16-byte aligned strides.  A [n, rows, cols] view whose strides already fit is taken as it is; anything else is made contiguous,
    padded with zeros to whole 16-byte groups (they add nothing to a sum) and cut into rows of its last dimension, which gives the
    kernel workgroups to split a sample over (a sample's sums do not depend on how its elements are arranged in rows)."""
    if t.dim() == 0 or t.shape[0] != n:
        raise AssertionError('pair_cosine: every operand needs %d samples (got shape %s)' % (n, tuple(t.shape)))
    if t.dtype != torch.int8:
        t = t.float()
    vec = 16 // t.element_size()
    if t.dim() == 3 and t.stride(2) == 1 and t.stride(1) % vec == 0 and t.stride(0) % vec == 0 and t.stride(1) >= t.shape[2] \
            and t.data_ptr() % 16 == 0:
        return t, t.shape[1], t.shape[2], t.stride(0), t.stride(1)
    cols = t.shape[-1] if t.dim() >= 3 and t.shape[-1] % vec == 0 else 0
    flat = t.reshape(n, -1)
    Fn = flat.shape[1]
    if not flat.is_contiguous() or Fn % vec or flat.data_ptr() % 16:
        buf = torch.zeros(n, (Fn + vec - 1) // vec * vec, dtype=flat.dtype, device=flat.device)
        buf[:, :Fn] = flat
        flat = buf
    Fp = flat.shape[1]
    if not cols or Fp != Fn:
        cols = next((c for c in (4096, 1024, 256, 64, 16, 4) if c % vec == 0 and Fp % c == 0 and Fp > c), Fp)
    return flat, Fp // cols, cols, Fp, cols


def _pair_cosine(a, b, scales):
    """sums [stages, n, 3] fp64 = (sum a.b, sum a.a, sum b.b) per stage and sample (p2v_pair_cosine): a[k], b[k] hold n samples each,
    int8 codes (scales[k]: None or the per-channel fp32 scales of the LAST dimension) or floats."""
    if not a or len(a) != len(b) or len(scales) != len(a):
        raise AssertionError('pair_cosine: %d a, %d b, %d scales' % (len(a), len(b), len(scales)))
    n, dev = a[0].shape[0] if a[0].dim() else 0, a[0].device
    keep, descs = [], (E.CosLayer * len(a))()
    for k, (x, y, sc) in enumerate(zip(a, b, scales)):
        if x.shape != y.shape or (x.dtype == torch.int8) != (y.dtype == torch.int8) or x.device != dev or y.device != dev:
            raise AssertionError('pair_cosine: stage %d: a %s %s on %s, b %s %s on %s' % (k, tuple(x.shape), x.dtype, x.device,
                                                                                        tuple(y.shape), y.dtype, y.device))
        if sc is not None:
            if x.dtype != torch.int8 or x.dim() < 2 or sc.numel() != x.shape[-1]:
                raise AssertionError('pair_cosine: stage %d: scales go with int8 codes, one per element of the last dimension' % k)
            if x.dim() != 3:
                x, y = x.reshape(n, -1, x.shape[-1]), y.reshape(n, -1, y.shape[-1])
            if x.shape[-1] % 16:                                                 # rows padded to whole 16-byte groups, cols stay
                Cp = (x.shape[-1] + 15) // 16 * 16
                xp, yp = (torch.zeros(n, x.shape[1], Cp, dtype=torch.int8, device=dev) for _ in range(2))
                xp[..., :x.shape[-1]], yp[..., :x.shape[-1]] = x, y
                x, y = xp[..., :x.shape[-1]], yp[..., :x.shape[-1]]
            sc = _f32(sc.reshape(-1)).to(dev)
            keep.append(sc)
        xv, yv = _cos_view(x, n), _cos_view(y, n)
        if xv[1:] != yv[1:]:                                                     # two different views of equal shapes: plain copies
            if sc is not None:
                raise AssertionError('pair_cosine: stage %d: scaled operands must share their strides' % k)
            xv, yv = _cos_view(x.contiguous(), n), _cos_view(y.contiguous(), n)
        keep += [xv[0], yv[0]]
        d = descs[k]
        d.a, d.b, d.scale = xv[0].data_ptr(), yv[0].data_ptr(), None if sc is None else sc.data_ptr()
        d.rows, d.cols, d.sample_stride, d.row_stride = xv[1], xv[2], xv[3], xv[4]
        d.dtype = E.COS_I8 if xv[0].dtype == torch.int8 else E.COS_F32
    L = E.lib()
    with torch.cuda.device(dev):
        nbytes = L.p2v_pair_cosine_workspace_bytes(descs, len(a), n)
        if nbytes == 0:
            E.check(L.p2v_pair_cosine(descs, len(a), n, None, None, 0, None))       # raises with the validation message
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(len(a), n, 3, dtype=torch.float64, device=dev)
        E.check(L.p2v_pair_cosine(descs, len(a), n, E.ptr(out), E.ptr(ws), nbytes, E.stream_ptr(dev)))
    return out


def _score_logits(logits, labels):
    """(ranks int32 [rows, 4] = gt, eq_lo, eq_hi, argmax; loss fp64 [rows]) of fp32 logits [rows, classes] against int64 labels [rows]
    (p2v_score_logits).  A row-strided view (``stride(1) == 1``) is read in place: the columns between the rows are never touched."""
    if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0] or logits.shape[1] < 1:
        raise AssertionError('score_logits: logits [rows, classes] and labels [rows] (got %s, %s)' % (tuple(logits.shape), tuple(labels.shape)))
    if labels.device != logits.device:
        raise AssertionError('score_logits: labels on %s, logits on %s' % (labels.device, logits.device))
    rows, classes = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1 or (rows > 1 and logits.stride(0) < classes):
        logits = _f32(logits)
    ld = logits.stride(0) if rows > 1 else classes
    labels = labels.contiguous().long()
    ranks = torch.empty(rows, 4, dtype=torch.int32, device=logits.device)
    loss = torch.empty(rows, dtype=torch.float64, device=logits.device)
    with torch.cuda.device(logits.device):
        E.check(E.lib().p2v_score_logits(E.ptr(logits), ld, rows, classes, E.ptr(labels), E.ptr(ranks), E.ptr(loss),
                                         E.stream_ptr(logits.device)))
    return ranks, loss


def _score_accumulate(ranks, loss, ks, totals):
    """fold the records of ``score_logits`` into one totals slot: int64 [3 + 3 * len(ks)] = n, invalid, hit[], sure[], possible[], and
    the bits of the fp64 loss sum (p2v_score_accumulate)"""
    ks = [int(k) for k in ks]
    rows = ranks.shape[0]
    if ranks.dtype != torch.int32 or tuple(ranks.shape) != (rows, 4) or loss.dtype != torch.float64 or tuple(loss.shape) != (rows,) \
            or not ranks.is_contiguous() or not loss.is_contiguous():
        raise AssertionError('score_accumulate: ranks int32 [rows, 4] and loss fp64 [rows], contiguous')
    if totals.dtype != torch.int64 or totals.numel() != 3 + 3 * len(ks) or not totals.is_contiguous() or totals.device != ranks.device \
            or loss.device != ranks.device:
        raise AssertionError('score_accumulate: totals int64 [%d], contiguous, on %s' % (3 + 3 * len(ks), ranks.device))
    with torch.cuda.device(ranks.device):
        E.check(E.lib().p2v_score_accumulate(E.ptr(ranks), E.ptr(loss), rows, (C.c_int * max(1, len(ks)))(*ks), len(ks), E.ptr(totals),
                                             E.stream_ptr(ranks.device)))


def _stat_view(t):
    """(tensor kept alive, kind, samples, rows, cols, sample stride, row stride) of ``t`` = [samples, ..., cols] int8 codes, uint8 bytes or
    floats for ``p2v_code_stats``.  A [samples, rows, cols] view whose base and strides are 16-byte aligned is read in place; anything
    else is made contiguous, its rows padded to whole 16-byte groups when cols is no multiple (the padding is never read)."""
    if t.dim() < 2:
        raise AssertionError('code_stats: every tensor is [samples, ..., cols] (got shape %s)' % (tuple(t.shape),))
    kind = {torch.int8: E.STAT_I8, torch.uint8: E.STAT_U8}.get(t.dtype, E.STAT_F32)
    if kind == E.STAT_F32 and t.dtype != torch.float32:
        t = t.float()
    vec = 16 // t.element_size()
    S, cols = t.shape[0], t.shape[-1]
    if cols < 1:
        raise AssertionError('code_stats: a tensor without columns (shape %s)' % (tuple(t.shape),))
    if t.dim() == 3 and t.stride(2) == 1 and t.stride(1) % vec == 0 and t.stride(0) % vec == 0 and t.stride(1) >= cols and t.data_ptr() % 16 == 0:
        return t, kind, S, t.shape[1], cols, t.stride(0), t.stride(1)
    if t.numel() == 0:                      # nothing to read: the record keeps what it holds
        return t, kind, 0, 0, cols, 0, cols
    x = t.reshape(S, -1, cols)
    R = x.shape[1]
    if cols % vec or not x.is_contiguous() or x.data_ptr() % 16:
        Cp = (cols + vec - 1) // vec * vec
        buf = torch.empty(S, R, Cp, dtype=x.dtype, device=x.device)
        buf[..., :cols] = x
        x = buf
    return x, kind, S, R, cols, R * x.shape[2], x.shape[2]


def stats_record_bytes(cols):
    """``p2v_stats_bytes``: 260 int64 (hist[256], count, nonfinite[3]), lo / hi [cols] 4 bytes each, sum / sumsq [cols] int64, to 16 bytes"""
    return (2080 + 24 * cols + 15) // 16 * 16


def _code_stats(tensors, records=None):
    """one record (uint8 [stats_record_bytes(cols)], the layout of ``p2v_code_stats`` in include/p2vit.h) per tensor, reduced over every
    sample and row per column of the LAST dimension.  ``records``: existing records to accumulate into (``stats.code_stats``); the op
    itself returns fresh ones."""
    if not tensors:
        raise AssertionError('code_stats: no tensors')
    dev = tensors[0].device
    views = []
    for k, t in enumerate(tensors):
        if t.device != dev:
            raise AssertionError('code_stats: every tensor must be on %s' % dev)
        views.append(_stat_view(t))
    L = E.lib()
    out = []
    with torch.cuda.device(dev):
        st = E.stream_ptr(dev)
        for k, v in enumerate(views):
            if records is None:
                rec = torch.empty(stats_record_bytes(v[4]), dtype=torch.uint8, device=dev)
                E.check(L.p2v_stats_init(E.ptr(rec), rec.numel(), v[1], v[4], st))
            else:
                rec = records[k]
                if rec.dtype != torch.uint8 or rec.numel() < stats_record_bytes(v[4]) or not rec.is_contiguous() or rec.device != dev:
                    raise AssertionError('code_stats: record %d must be a contiguous uint8 tensor of %d bytes on %s' % (k, stats_record_bytes(v[4]), dev))
            out.append(rec)
        live = [k for k, v in enumerate(views) if v[0].numel() > 0]         # an empty plane launches nothing (and has no pointer)
        if live:
            lays = (E.StatLayer * len(live))()
            recs = (C.c_void_p * len(live))()
            for j, k in enumerate(live):
                x, kind, S, R, cols, ss, rs = views[k]
                d = lays[j]
                d.base, d.sample_stride, d.row_stride, d.samples, d.rows, d.cols, d.dtype = x.data_ptr(), ss, rs, S, R, cols, kind
                recs[j] = out[k].data_ptr()
            E.check(L.p2v_code_stats(lays, len(live), recs, None, 0, st))
    return out


def _gram_view(t, n):
    """(tensor kept alive, kind, rows, cols, sample stride, row stride) of ``t`` = [n, ..., cols] int8 codes or floats for
    ``p2v_code_grams``.  A [n, rows, cols] int8 view (last stride 1, any row and sample stride) on a 16-byte aligned base is read in place;
    anything else is made contiguous (fp32 stages need dense rows)."""
    if t.dim() < 2 or t.shape[0] != n or t[0].numel() < 1:
        raise AssertionError('code_grams: every tensor is [%d, ..., cols] (got shape %s)' % (n, tuple(t.shape)))
    if t.dtype != torch.int8:
        x = _f32(t).reshape(n, -1)
        if x.data_ptr() % 16:
            x = x.clone()
        return x, E.GRAM_F32, 1, x.shape[1], x.shape[1], x.shape[1]
    if t.dim() == 3 and t.stride(2) == 1 and t.stride(1) >= t.shape[2] and t.stride(0) >= 0 and t.data_ptr() % 16 == 0:
        return t, E.GRAM_I8, t.shape[1], t.shape[2], t.stride(0), t.stride(1)
    x = t.reshape(n, -1, t.shape[-1]).contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    return x, E.GRAM_I8, x.shape[1], x.shape[2], x.shape[1] * x.shape[2], x.shape[2]


def _code_grams(tensors, shifts):
    """raw Grams fp64 [stages, n, n] (p2v_code_grams): tensors[k] holds n samples, int8 codes (shifts[k]: None or the uint8 exponents m_c of
    the LAST dimension, the values are code * 2^m_c) or floats (fp32 Gram with a zero diagonal)."""
    if not tensors or len(shifts) != len(tensors):
        raise AssertionError('code_grams: %d tensors, %d shifts' % (len(tensors), len(shifts)))
    n, dev = tensors[0].shape[0] if tensors[0].dim() else 0, tensors[0].device
    keep, lays = [], (E.GramLayer * len(tensors))()
    for k, (t, sh) in enumerate(zip(tensors, shifts)):
        if t.device != dev:
            raise AssertionError('code_grams: every tensor must be on %s' % dev)
        x, kind, rows, cols, ss, rs = _gram_view(t, n)
        keep.append(x)
        d = lays[k]
        d.base, d.sample_stride, d.row_stride, d.rows, d.cols, d.dtype = x.data_ptr(), ss, rs, rows, cols, kind
        if sh is not None:
            if kind != E.GRAM_I8 or sh.numel() != cols or sh.device != dev:
                raise AssertionError('code_grams: stage %d: shifts go with int8 codes, one byte per element of the last dimension, on %s' % (k, dev))
            sh = sh.reshape(-1).to(torch.uint8).contiguous()
            if sh.data_ptr() % 16:
                sh = sh.clone()
            keep.append(sh)
            d.shift = sh.data_ptr()
    L = E.lib()
    with torch.cuda.device(dev):
        nbytes = L.p2v_code_grams_workspace_bytes(lays, len(tensors), n)
        if nbytes == 0:
            E.check(L.p2v_code_grams(lays, len(tensors), n, None, None, 0, None))       # raises with the validation message
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(len(tensors), n, n, dtype=torch.float64, device=dev)
        E.check(L.p2v_code_grams(lays, len(tensors), n, E.ptr(out), E.ptr(ws), nbytes, E.stream_ptr(dev)))
    return out


def _cka_centre(raw):
    """centred fp32 Grams [layers, n, n] of raw fp64 Grams [layers, n, n] (p2v_cka_centre); a view with a row pitch and a layer stride -
    the off-diagonal block ``big[:, :n, n:]`` of [layers, 2n, 2n] Grams, which centres as the X Y^T form - is read in place."""
    if raw.dim() == 2:
        raw = raw.unsqueeze(0)
    if raw.dim() != 3 or raw.shape[1] != raw.shape[2]:
        raise AssertionError('cka_centre: raw Grams are [layers, n, n] (got shape %s)' % (tuple(raw.shape),))
    if raw.dtype != torch.float64 or raw.stride(2) != 1 or raw.stride(1) < raw.shape[2] or raw.stride(0) < 0:
        raw = raw.double().contiguous()
    Ln, n = raw.shape[0], raw.shape[1]
    out = torch.empty(Ln, n, n, dtype=torch.float32, device=raw.device)
    with torch.cuda.device(raw.device):
        E.check(E.lib().p2v_cka_centre(raw.data_ptr(), raw.stride(1), raw.stride(0), Ln, n, E.ptr(out), E.stream_ptr(raw.device)))
    return out


def _patch_similarity_entropy(av, groups):
    """(value fp64 [], grad fp32 like av) of the patch-similarity entropy (p2v_patch_similarity_entropy): av [images * groups, heads,
    tokens, head_dim], one block's attn @ v; the workspace is allocated here, nothing synchronises."""
    if av.dim() != 4 or groups < 1 or av.shape[0] % max(groups, 1):
        raise AssertionError('patch_similarity_entropy: av is [images * groups, heads, tokens, head_dim] (got shape %s, groups %d)'
                             % (tuple(av.shape), groups))
    av = _f32(av)
    if av.data_ptr() % 16:
        av = av.clone()
    BG, H, N, hd = av.shape
    L = E.lib()
    with torch.cuda.device(av.device):
        nbytes = L.p2v_psaq_workspace_bytes(BG // groups, groups, H, N, hd)
        if nbytes == 0:
            E.check(L.p2v_patch_similarity_entropy(None, BG // groups, groups, H, N, hd, None, None, None, None))   # raises with the validation message
        ws = torch.empty(nbytes, dtype=torch.uint8, device=av.device)
        value = torch.empty((), dtype=torch.float64, device=av.device)
        grad = torch.empty_like(av)
        E.check(L.p2v_patch_similarity_entropy(E.ptr(av), BG // groups, groups, H, N, hd, E.ptr(ws), E.ptr(value), E.ptr(grad),
                                               E.stream_ptr(av.device)))
    return value, grad


def _flat_f32(who, t, dev):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() < 1:
        raise AssertionError('%s: tensors are non-empty contiguous fp32 on %s (got %s %s on %s)' % (who, dev, t.dtype, tuple(t.shape), t.device))
    return t


def _rademacher_fill(tensors, layers, seed, probe):
    """fills every tensor with +-1 in place: element e of tensors[k] from (seed, layers[k], probe, e) - ``hessian.rademacher_host`` gives
    the same values; one launch per 64 tensors, nothing synchronises"""
    if not tensors or len(layers) != len(tensors):
        raise AssertionError('rademacher_fill: one layer id per tensor, at least one tensor')
    dev = tensors[0].device
    segs = (E.Seg * len(tensors))()
    for k, (t, l) in enumerate(zip(tensors, layers)):
        _flat_f32('rademacher_fill', t, dev)
        segs[k].ptr, segs[k].n, segs[k].layer = t.data_ptr(), t.numel(), int(l)
    with torch.cuda.device(dev):
        E.check(E.lib().p2v_rademacher_fill(segs, len(tensors), int(seed) & (2 ** 64 - 1), int(probe) & (2 ** 64 - 1), E.stream_ptr(dev)))


def seg2_table(who, a, b):
    """the ``p2v_seg2`` array of the tensor pairs (a[k], b[k])"""
    if not a or len(a) != len(b):
        raise AssertionError('%s: as many tensors in a as in b, at least one' % who)
    dev = a[0].device
    segs = (E.Seg2 * len(a))()
    for k, (x, y) in enumerate(zip(a, b)):
        _flat_f32(who, x, dev)
        _flat_f32(who, y, dev)
        if x.numel() != y.numel():
            raise AssertionError('%s: pair %d has %d and %d elements' % (who, k, x.numel(), y.numel()))
        segs[k].a, segs[k].b, segs[k].n = x.data_ptr(), y.data_ptr(), x.numel()
    return segs, dev


def _dot_workspace(who, segs, n, dev):
    nbytes = E.lib().p2v_group_dot_workspace_bytes(segs, n)
    if nbytes == 0:
        E.check(E.lib().p2v_group_dot(segs, n, None, None, 0, None))       # raises with the validation message
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev)


def _group_dot(a, b):
    """fp64 [len(a)]: sum over the elements of a[k] * b[k], every product exact, fixed summation order (p2v_group_dot)"""
    segs, dev = seg2_table('group_dot', a, b)
    with torch.cuda.device(dev):
        ws = _dot_workspace('group_dot', segs, len(a), dev)
        out = torch.empty(len(a), dtype=torch.float64, device=dev)
        E.check(E.lib().p2v_group_dot(segs, len(a), E.ptr(out), E.ptr(ws), ws.numel() * 8, E.stream_ptr(dev)))
    return out


def hutchinson_state(n_layers, device):
    """a cleared stopping state of ``n_layers`` layers (int32 words; ``hessian.read_state`` decodes it)"""
    state = torch.empty(E.lib().p2v_hutchinson_state_bytes(n_layers) // 4, dtype=torch.int32, device=device)
    _hutchinson_init(state, n_layers)
    return state


def _hutchinson_init(state, n_layers):
    if state.dtype != torch.int32 or not state.is_contiguous():
        raise AssertionError('hutchinson_init: the state is a contiguous int32 tensor')
    with torch.cuda.device(state.device):
        E.check(E.lib().p2v_hutchinson_init(E.ptr(state), state.numel() * 4, n_layers, E.stream_ptr(state.device)))


def _hutchinson_step(a, b, probe, tol, record, state):
    """one probe of all layers: record[probe][k] = sum(a[k] * b[k]), then every layer's stopping rule on the device
    (p2v_hutchinson_step); record fp64 [max_iter, len(a)], state from ``hutchinson_state``"""
    segs, dev = seg2_table('hutchinson_step', a, b)
    if record.dtype != torch.float64 or record.dim() != 2 or record.shape[1] != len(a) or not record.is_contiguous() or record.device != dev:
        raise AssertionError('hutchinson_step: record is contiguous fp64 [max_iter, %d] on %s' % (len(a), dev))
    if state.dtype != torch.int32 or not state.is_contiguous() or state.device != dev:
        raise AssertionError('hutchinson_step: the state is a contiguous int32 tensor on %s' % dev)
    with torch.cuda.device(dev):
        ws = _dot_workspace('hutchinson_step', segs, len(a), dev)
        E.check(E.lib().p2v_hutchinson_step(segs, len(a), int(probe), record.shape[0], float(tol), E.ptr(record), E.ptr(state), state.numel() * 4,
                                            E.ptr(ws), ws.numel() * 8, E.stream_ptr(dev)))


_LIB.impl('fake_quant', _fake_quant, 'CUDA')
_LIB.impl('quantize_patchify', _quantize_patchify, 'CUDA')
_LIB.impl('linear_requant', lambda x, w, cs, b, inv: _linear(E.EPI_REQUANT, x, w, cs, b, inv), 'CUDA')
_LIB.impl('linear_gelu_requant', lambda x, w, cs, b, inv: _linear(E.EPI_GELU, x, w, cs, b, inv), 'CUDA')
_LIB.impl('int_layernorm', _int_layernorm, 'CUDA')
_LIB.impl('lis_attention', _lis_attention, 'CUDA')
_LIB.impl('lis_attention_rows', _lis_attention_rows, 'CUDA')
_LIB.impl('forward', _forward, 'CUDA')
_LIB.impl('cka_grams', _cka_grams, 'CUDA')
_LIB.impl('hsic_accumulate', _hsic_accumulate, 'CUDA')
_LIB.impl('pair_cosine', _pair_cosine, 'CUDA')
_LIB.impl('score_logits', _score_logits, 'CUDA')
_LIB.impl('score_accumulate', _score_accumulate, 'CUDA')
_LIB.impl('code_stats', lambda tensors: _code_stats(tensors), 'CUDA')
_LIB.impl('code_grams', _code_grams, 'CUDA')
_LIB.impl('cka_centre', _cka_centre, 'CUDA')
_LIB.impl('patch_similarity_entropy', _patch_similarity_entropy, 'CUDA')
_LIB.impl('rademacher_fill', _rademacher_fill, 'CUDA')
_LIB.impl('group_dot', _group_dot, 'CUDA')
_LIB.impl('hutchinson_init', _hutchinson_init, 'CUDA')
_LIB.impl('hutchinson_step', _hutchinson_step, 'CUDA')

OPS = ('fake_quant', 'quantize_patchify', 'linear_requant', 'linear_gelu_requant', 'int_layernorm', 'lis_attention', 'lis_attention_rows', 'forward', 'cka_grams',
       'hsic_accumulate', 'pair_cosine', 'score_logits', 'score_accumulate', 'code_stats', 'code_grams', 'cka_centre',
       'patch_similarity_entropy', 'rademacher_fill', 'group_dot', 'hutchinson_init', 'hutchinson_step')
