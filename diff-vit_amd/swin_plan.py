"""Frozen integer plan of a calibrated Swin model: int8 weight codes and per-channel requant constants on the GPU, and a forward
that is a fixed sequence of HIP kernels called through the C ABI (``p2v_quantize_patchify``, ``p2v_gemm_i8``,
``p2v_int_layernorm`` - under Config(ptf=False) ``p2v_float_layernorm`` -, ``p2v_window_attention`` - under Config(lis=False)
``p2v_window_softmax_attention`` -, ``p2v_patch_merge_gather``, ``p2v_avgpool_quant``).  Window partition, cyclic
shift and their inverses are index tables consumed by the attention kernel; nothing runs on the CPU and nothing falls back.

Call order = swin_quant.py (forward_features :790-811, SwinTransformerBlock.forward :351-399, PatchMerging.forward :438-461).
"""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from .swin import check_bit_list, relative_position_index, shifted_window_regions  # noqa: F401


def _pad128(n):
    return (n + 127) // 128 * 128


def _lis_consts(sf):
    """x0_int, b_int, c_int of the I-BERT polynomial in fp32 (layers.py:334-351); range-checked like the ViT plan's."""
    from .plan import lis_consts
    return lis_consts(torch.tensor(float(sf), dtype=torch.float32))


def _window_index(H, W, ws, shift):
    hh = (torch.arange(H) + shift) % H
    ww = (torch.arange(W) + shift) % W
    grid = hh[:, None] * W + ww[None, :]
    return grid.reshape(H // ws, ws, W // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)


class SwinPlan:
    """``bits``: the plan's default weight width (what every entry point runs without a list; the model-diff paths know only this one).
    The plan holds the fp32 weights on the GPU and freezes the codes of a (layer, width, layout) with ``p2v_freeze_weights`` when a
    forward first asks for them, so ``forward(..., bit_config=[...])`` takes one width per layer - in the order of ``linear_tap_names()`` -
    without rebuilding anything.  ``pack4``: 4-bit layers of the fused forward stream packed codes (two per byte); False keeps them
    one per byte (A/B comparison).  The tapped / model-diff sequences always read int8-stored codes.
    ``int_softmax=False`` (Config(lis=False)): every window-attention record of every sequence is ``P2V_OP_WINATTN_SOFTMAX`` - the float
    softmax behind the qact2 codes as a 256-entry fixed-point table per block (``plan.softmax_table`` of the block's qact2 scale), which
    needs that scale to be at most 2^-2 (``NotImplementedError`` here otherwise, naming the layer).
    ``softmax_bits``: the width of every window attention's log-int-softmax (p = 2^-k for k < 2^bits, else 0): None = the widths the
    calibration state names (``<path>.log_int_softmax.bits``, else 4), an int, or one entry per attention module in model order (a named
    width that disagrees is refused); kept as ``plan.softmax_bits`` and written into every ``P2V_OP_WINATTN``
    record.  Unused (as in the reference) under ``int_softmax=False``.
    ``int_norm=False`` (Config(ptf=False)): every QAct is layer-wise, and every LayerNorm stays ``F.layer_norm`` followed by the next QAct.
    Every LayerNorm record of every sequence - ``patch_embed.norm``, each block's ``norm1`` / ``norm2``, each ``downsample.norm`` behind the
    merge gather, the final ``norm`` - is ``P2V_OP_FLOAT_LAYERNORM`` (``p2v_float_layernorm``: s_in the producing QAct's one scale,
    g = 1 / s_out repeated over the channels, ``ln_eps`` the modules' eps); no fused ``P2V_OP_LN_GEMM`` record runs behind it and no
    ``p2v_ln_prefold`` buffer is built.  The one scale of ``qact2`` / ``qact4`` / ``downsample.qact2`` is repeated over the channels
    wherever the plan keeps per-channel vectors, so every other record is the integer arithmetic of the ptf=True plan.  A scale that is
    no power of two stays refused (``NotImplementedError`` naming the module), as is a library without the record kind."""

    def __init__(self, arch, state_dict, calib, device='cuda', in_chans=3, bits=8, pack4=True, int_softmax=True, softmax_bits=None,
                 int_norm=True, ln_eps=1e-5):
        if bits not in (4, 8):
            raise KeyError('int%s' % (bits,))          # (the weight scale a width has none of: what the lookup below raised)
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('SwinPlan: building a plan uploads and synchronises, which a stream that is capturing a graph cannot do: '
                               'freeze the model and run one eager forward before the capture')
        self.arch, self.device, self.in_chans, self.bits, self.pack4 = dict(arch), torch.device(device), in_chans, bits, bool(pack4)
        self.int_softmax = bool(int_softmax)
        self.int_norm, self.ln_eps = bool(int_norm), float(ln_eps)
        from .plan import calib_softmax_bits
        self.softmax_bits = calib_softmax_bits(calib, ['layers.%d.blocks.%d.attn' % (li, bi) for li, d in enumerate(self.arch['depths'])
                                                       for bi in range(d)], softmax_bits)
        if self.device.type != 'cuda':
            raise RuntimeError('SwinPlan needs a GPU device: the quantized forward has no CPU path')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if not self.int_norm and not hasattr(E.lib(), 'p2v_float_layernorm_max_channels'):
            raise RuntimeError('libp2vit_hip.so lacks P2V_OP_FLOAT_LAYERNORM (Config(ptf=False) of a Swin model): rebuild')
        self._keep = []
        self.W = {k: v.detach().float().cpu() for k, v in state_dict.items() if v.dtype == torch.float32}
        self.c = calib
        self._recorded = {}
        self._layers, self._all_frozen = [], False
        self.resid_prefolded = []
        with torch.cuda.device(self.device):      # uploads and GELU-table builds on the plan's device, whatever the caller's current one
            self._build()
            self._names = self.linear_tap_names()
            assert [d['name'] for d in sorted(self._layers, key=lambda d: self._names.index(d['name']))] == self._names
            for d in self._layers:
                d['idx'] = self._names.index(d['name'])
            self._layers.sort(key=lambda d: d['idx'])

    # ---- helpers -------------------------------------------------------------------------------------------------------
    def _no_capture(self, what):
        """lazy plan state - freezing codes, building a RESID table, recording a sequence - uploads, allocates and synchronises, and a
        graph capture would record that work instead of running it while the plan cached it as done: refused before anything is
        allocated, enqueued or cached, so the plan is as usable afterwards as before (DESIGN, graph capture of the forwards)"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('SwinPlan: the stream is capturing a graph and %s is not there yet: make the same forward(...) call - this batch size, '
                               'slicing and bit_config - once eagerly before the capture (freeze_all() ahead of it freezes every width)' % what)

    def _dev(self, t, dtype=torch.float32):
        t = t.to(dtype).contiguous().to(self.device)
        self._keep.append(t)
        return t

    def _vec(self, v, n):
        """per-channel fp32 vector of length n, padded to a multiple of 128 (whole tiles are staged)."""
        v = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        if v.numel() == 1:
            v = v.expand(n)
        out = torch.ones(_pad128(n))
        out[:n] = v
        return self._dev(out)

    def _pot(self, name):
        s = float(self.c[name].reshape(-1)[0])
        m, _ = np.frexp(s)
        if self.c[name].numel() != 1 or m != 0.5:
            raise NotImplementedError('%s: the engine needs a power-of-two layer-wise scale, got %r' % (name, self.c[name][:4]))
        return s

    def _linear(self, name, s_x, bias=True, k_pad=None, frag=False):
        """one QConv2d / QLinear: the fp32 weights [N][K] and the bias on the GPU.  Codes, column scales and RESID tables are made per
        width on first use (``_lin``).  ``frag``: the fused LayerNorm+GEMM kernel may stream this layer (qkv / fc1 of stages up to 384
        channels), which reads the MFMA-fragment-order copy."""
        w = self.W[name + '.weight']
        w2 = w.reshape(w.shape[0], -1)
        N, K = w2.shape
        kp = (K + 63) // 64 * 64                   # the GEMM walks 64-deep k-tiles: extra weight columns are zero
        assert k_pad in (None, kp)
        b = torch.zeros(_pad128(N))
        if bias:
            b[:N] = self.W[name + '.bias']
        d = dict(name=name, N=N, K=kp, frag=bool(frag), s_x=float(s_x), w32=self._dev(w2), b=self._dev(b), width={}, forms={}, epi=None)
        self._layers.append(d)
        return d

    def _width(self, d, bits):
        """(weight scales, colscale = s_x * s_w) of layer ``d`` at ``bits``, on the GPU"""
        if bits not in d['width']:
            s_w = self.c[d['name']]['int%d' % bits].reshape(-1).float()
            cs = torch.zeros(_pad128(d['N']))
            cs[:d['N']] = (torch.tensor(d['s_x']) * s_w.expand(d['N'])).float()
            d['width'][bits] = (self._dev(s_w), self._dev(cs))
        return d['width'][bits]

    def _packed(self, bits):
        return self.pack4 and bits == 4

    def _lin(self, d, bits, packed=False, frag=False):
        """the ``p2v_linear`` of layer ``d`` at ``bits``: int8-stored codes, or (``packed``) the packed int4 tiles; ``frag``: with the
        fragment-order copy.  Frozen on the current stream on first use, kept afterwards."""
        f = d['forms'].get((bits, packed))
        if f is not None and (f['wf'] is not None or not frag):
            return f['lin']
        self._no_capture('the %d-bit codes of %s' % (bits, d['name']))
        with torch.cuda.device(self.device):
            s_w, cs = self._width(d, bits)
            if f is None:
                w = E.freeze_weights(d['w32'], s_w, bits, E.W_TILES_P4 if packed else E.W_ROWS_I8)
                f = d['forms'][(bits, packed)] = dict(w=w, wf=None, tab=None, lin=E.Linear(E.ptr(w), E.ptr(cs), E.ptr(d['b']), None, 1 if packed else 0))
            if frag and f['wf'] is None:
                f['wf'] = E.freeze_weights(d['w32'], s_w, bits, E.W_FRAG_P4 if packed else E.W_FRAG_I8)
                f['lin'].w_frag = E.ptr(f['wf'])
        return f['lin']

    def _resid_tab(self, d, bits, packed=False):
        """``p2v_epilogue.resid_tab`` of the RESID layer ``d`` at ``bits`` (None where the library does not prove the table exact): it
        folds the layer's column scales and bias, so there is one per weights / epilogue pair"""
        lin = self._lin(d, bits, packed)
        f = d['forms'][(bits, packed)]
        if f['tab'] is None:
            self._no_capture('the %d-bit RESID table of %s' % (bits, d['name']))
            with torch.cuda.device(self.device):
                e, n, L = d['epi'], d['N'], E.lib()
                nbytes = L.p2v_resid_prefold_bytes(n)
                tab = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
                usable = C.c_int(0)
                torch.cuda.synchronize(self.device)                       # the vectors were uploaded on torch's stream
                E.check(L.p2v_resid_prefold(C.byref(lin), C.byref(e), n, E.ptr(tab), nbytes, C.byref(usable), None))
                f['tab'] = (tab if usable.value else False,)
                self.resid_prefolded.append(bool(usable.value))
        t = f['tab'][0]
        return C.cast(E.ptr(t), C.c_void_p) if t is not False else None

    def _ensure(self, d, bits, packed):
        self._lin(d, bits, packed, frag=d['frag'])
        if d['epi'] is not None:
            self._resid_tab(d, bits, packed)

    def freeze_all(self):
        """freeze every (layer, width) a fused forward can ask for - 8-bit codes, 4-bit codes (packed with ``pack4``), the fragment-order
        copies and the RESID tables - so that no later ``bit_config`` allocates or synchronises"""
        for d in self._layers:
            for bits in (8, 4):
                self._ensure(d, bits, self._packed(bits))
        torch.cuda.synchronize(self.device)
        self._all_frozen = True
        return self

    def bit_config(self, bit_config=None):
        """the validated per-layer widths as a tuple of ``len(linear_tap_names())`` ints (None: the plan's default width everywhere).
        ValueError for a wrong length or an entry outside {4, 8, -1}; NotImplementedError for -1 (Swin has no per-layer fp fallback)."""
        n = len(self._names)
        if bit_config is None:
            return (self.bits,) * n
        try:
            cfg = tuple(int(b) for b in bit_config)
        except TypeError:
            raise ValueError('bit_config must be a list of %d entries of 4 or 8, got %r' % (n, bit_config))
        check_bit_list(cfg, n)
        return cfg

    def _ln(self, prefix, s_in_vec, s_out, C_):
        """QIntLayerNorm 'int' constants: mask = round(in_scale / min), inv_out = 1 / out_scale; the following QAct has the LN's
        own output scale, so post_mul = 1.  ``int_norm=False``: the ``p2v_float_ln`` of the float LayerNorm instead."""
        if not self.int_norm:
            return self._float_ln(prefix, s_in_vec, s_out, C_)
        s_in_vec = torch.as_tensor(s_in_vec, dtype=torch.float32).reshape(-1)
        if s_in_vec.numel() == 1:
            s_in_vec = s_in_vec.expand(C_)
        s1 = s_in_vec.min()
        mask_max = float(torch.round(s_in_vec / s1).max())
        if C_ * (128.0 * mask_max) ** 2 >= 2.0 ** 32:      # the kernel keeps sum(x_q^2) exactly in 32 unsigned bits
            raise NotImplementedError('LayerNorm input scale ratios up to %g over %d channels exceed the exact 32-bit statistics' % (mask_max, C_))
        t = [self._dev(torch.round(s_in_vec / s1)), self._dev(self.W[prefix + '.weight']), self._dev(self.W[prefix + '.bias']),
             self._dev(torch.full((C_,), 1.0 / float(s_out))), self._dev(torch.ones(C_))]
        ln = E.Ln(float(s1), *[E.ptr(x) for x in t])
        # the constants folded once here instead of by every workgroup of every launch (p2v_ln_prefold: gamma / out_scale, beta / out_scale and
        # the fast-chain tests; the wide stages' stand-alone LayerNorm folds for only 16 - 32 rows per workgroup otherwise)
        L = E.lib()
        nbytes = L.p2v_ln_prefold_bytes(C_)
        buf = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        self._keep.append(buf)
        E.check(L.p2v_ln_prefold(C.byref(ln), C_, E.ptr(buf), nbytes))
        return ln

    def _float_ln(self, prefix, s_in_vec, s_out, C_):
        """QIntLayerNorm in mode 'ln' and the QAct behind it (Config(ptf=False)): one input scale, g = 1 / s_out over the channels"""
        s_in_vec = torch.as_tensor(s_in_vec, dtype=torch.float32).reshape(-1)
        s_in = float(s_in_vec[0])
        if not bool((s_in_vec == s_in).all()):
            raise NotImplementedError('%s: the float LayerNorm of Config(ptf=False) needs ONE input scale, got %r' % (prefix, s_in_vec[:4]))
        if C_ % 4 or not 16 <= C_ <= E.lib().p2v_float_layernorm_max_channels():
            raise NotImplementedError('%s: %d channels, the float LayerNorm covers multiples of 4 in 16 .. %d'
                                      % (prefix, C_, E.lib().p2v_float_layernorm_max_channels()))
        t = [self._dev(self.W[prefix + '.weight']), self._dev(self.W[prefix + '.bias']), self._dev(torch.full((C_,), 1.0 / float(s_out)))]
        return E.FloatLn(s_in, self.ln_eps, *[E.ptr(x) for x in t])

    def _chan(self, name, n):
        """the scale of a QAct that is a PTF vector under ptf=True, as n per-channel values: the calibrated vector, or (``int_norm=False``:
        every QAct is layer-wise) its one power-of-two scale repeated"""
        if self.int_norm:
            return self.c[name].reshape(-1)
        return torch.full((n,), self._pot(name))

    # ---- plan ----------------------------------------------------------------------------------------------------------
    def _build(self):
        a, c = self.arch, self.c
        P, D0, ws = a['patch_size'], a['embed_dim'], a['window_size']
        g = a['img_size'] // P
        self.g = g
        self.s_in = self._pot('qact_input')
        kpatch = self.in_chans * P * P
        self.k_patch = (kpatch + 63) // 64 * 64
        self.pe = self._linear('patch_embed.proj', self.s_in, k_pad=self.k_patch)
        self.s_pe_b = self._pot('patch_embed.qact_before_norm')
        s_pe = self._pot('patch_embed.qact')
        self.pe_ln = self._ln('patch_embed.norm', torch.tensor([self.s_pe_b]), s_pe, D0)
        s_res = torch.full((D0,), s_pe)
        self.stages = []
        H = g
        for li, depth in enumerate(a['depths']):
            Cc = D0 * 2 ** li
            heads = a['num_heads'][li]
            if Cc // heads != 32:
                raise NotImplementedError('window attention kernel: head_dim must be 32 (got %d)' % (Cc // heads))
            wsz = min(ws, H)
            blocks = []
            for bi in range(depth):
                p = 'layers.%d.blocks.%d.' % (li, bi)
                shift = 0 if (bi % 2 == 0 or H <= ws) else ws // 2
                s1 = self._pot(p + 'qact1')
                b = dict(C=Cc, heads=heads, H=H, ws=wsz, shift=shift, softmax_bits=self.softmax_bits[sum(a['depths'][:li]) + bi])
                b['ln1'] = self._ln(p + 'norm1', s_res, s1, Cc)
                s_q1 = self._pot(p + 'attn.qact1')
                b['qkv'] = self._linear(p + 'attn.qkv', s1, frag=self.int_norm and Cc <= 384)
                b['inv_s_qkv'] = 1.0 / s_q1
                s_q2 = self._pot(p + 'attn.qact2')
                s_q3 = self._pot(p + 'attn.qact3')
                tab = torch.clamp(torch.round(self.W[p + 'attn.relative_position_bias_table'] / self._pot(p + 'attn.qact_table')), -128, 127)
                idx = _window_index(H, H, wsz, shift)
                reg = shifted_window_regions(H, H, wsz, shift) if shift else None
                x0, bb, cc = _lis_consts(s_q2)
                b['tab'], b['idx'] = self._dev(tab, torch.int8), self._dev(idx, torch.int32)
                b['reg'] = self._dev(reg, torch.int8) if reg is not None else None
                b['wa'] = E.WinAttn(s_q1, float(np.float32(32 ** -0.5)), self._pot(p + 'attn.qact_attn1'), self._pot(p + 'attn.qact_table'),
                                    s_q2, s_q3, x0, bb, cc, E.ptr(b['tab']), E.ptr(b['idx']),
                                    E.ptr(b['reg']) if b['reg'] is not None else None, wsz, idx.shape[0])
                b['sm_tab'] = None
                if not self.int_softmax:
                    # a masked key is exactly zero only while 100 / s_q2 > 255 codes and exp(-(100 - 255 s_q2)) 2^21 rounds to 0
                    if s_q2 > 2.0 ** -2:
                        raise NotImplementedError('%sattn.qact2: scale %g above 2^-2, the table softmax of Config(lis=False) needs a masked '
                                                  'key to round to zero' % (p, s_q2))
                    from .plan import softmax_table
                    b['sm_tab'] = self._dev(torch.from_numpy(softmax_table(s_q2).astype(np.int32)), torch.int32)
                b['proj'] = self._linear(p + 'attn.proj', s_q3)
                s_b2 = self._chan(p + 'qact2', Cc)
                b['proj_epi'] = self._resid_epi(self._pot(p + 'attn.qact4'), s_res, s_b2, Cc, b['proj'])
                s3 = self._pot(p + 'qact3')
                b['ln2'] = self._ln(p + 'norm2', s_b2, s3, Cc)
                b['fc1'] = self._linear(p + 'mlp.fc1', s3, frag=self.int_norm and Cc <= 384)
                s_m1 = self._pot(p + 'mlp.qact1')
                b['inv_s_fc1'] = 1.0 / s_m1
                b['fc2'] = self._linear(p + 'mlp.fc2', s_m1)
                s_b4 = self._chan(p + 'qact4', Cc)
                b['fc2_epi'] = self._resid_epi(self._pot(p + 'mlp.qact2'), s_b2, s_b4, Cc, b['fc2'])
                s_res = s_b4.clone()
                blocks.append(b)
            st = dict(blocks=blocks, C=Cc, H=H, merge=None)
            if li < len(a['depths']) - 1:
                p = 'layers.%d.downsample.' % li
                sd1 = self._pot(p + 'qact1')
                sd2 = self._chan(p + 'qact2', 2 * Cc)
                red = self._linear(p + 'reduction', sd1, bias=False)
                # single PTF requant through the RESID epilogue: s_mid = s_next and an all-zero residual make it
                # Q(Q(y; s) * s; s) = Q(y; s)   (|code * eps| << 0.5)
                st['merge'] = dict(ln=self._ln(p + 'norm', s_res.repeat(4), sd1, 4 * Cc), red=red,
                                   epi=self._resid_epi(sd2, torch.ones(2 * Cc), sd2, 2 * Cc, red))
                s_res = sd2.clone()
                H //= 2
            self.stages.append(st)
        Cl = D0 * 2 ** (len(a['depths']) - 1)
        self.C_last, self.H_last = Cl, H
        self.s_f = self._pot('qact2')
        self.fin_ln = self._ln('norm', s_res, self.s_f, Cl)
        self.s_pool = self._pot('qact3')
        self.head = self._linear('head', self.s_pool)
        self.s_out = self._pot('act_out')

    def _resid_epi(self, s_mid, s_res, s_next, n, lin):
        """constants of the RESID epilogue behind layer ``lin``; the pre-folded table of ``p2v_resid_prefold`` is made per width
        (``_resid_tab``)"""
        e = E.Epilogue()
        t = [self._vec(s_mid, n), self._vec(s_res, n), self._vec(s_next, n)]
        e.s_mid, e.s_res, e.s_next = [C.cast(E.ptr(x), C.c_void_p) for x in t]
        lin['epi'] = e
        return e

    # ---- forward -------------------------------------------------------------------------------------------------------
    def _record(self, B, fused=True, ddv_n=0, with_linear=False, lin_taps=False, attention=False, cfg=None, stats=False):
        """the launch sequence of one forward at batch B as a ``p2v_op`` array with its own activation buffers (built once
        per batch size and stream slot, replayed by ``p2v_run_ops``).  ``fused``: norm1 + qkv and norm2 + fc1 of stages up to 384
        channels run as ONE launch each (``P2V_OP_LN_GEMM``: the LayerNorm output stays in LDS); the tap replay records the
        unfused sequence, whose LayerNorm outputs exist in HBM.  Under ``int_norm=False`` nothing is fused behind the float LayerNorm: both
        sequences hold the same LayerNorm and GEMM records.
        ``ddv_n`` > 0 (B = 2 * ddv_n, unfused): behind the launch that completes a DDV stage a ``P2V_OP_COS`` record reduces samples
        [0, n) of the live buffer against samples [n, 2n); proj / fc2 also store their mid codes (attn.qact4 / mlp.qact2); ``with_linear``
        adds the fp32 layer outputs through ONE scratch buffer; a ``P2V_OP_COS_COMBINE`` closes the sequence.
        ``lin_taps`` (unfused): the fp32 output of every QConv2d / QLinear into a buffer of its own (``forward_linear_taps``).
        ``attention`` (with ``ddv_n``): the window launches run tapped (the planes of ``p2v_window_attention_taps``, named in the WINATTN
        record) into three planes per stage that its blocks share - qact_attn1, qact2 (int8 codes) and the softmax exponents
        (``P2V_COS_LOG2K``) - each reduced right behind the launch.
        ``stats`` (unfused, instead of ``ddv_n``): the same stage sites, mid codes, scratch and tapped window launches, but every site writes
        a ``P2V_OP_STATS`` record that reduces all B samples of the live buffer into the stage's record (``forward_stats`` names the
        records before each replay); no combine.
        ``cfg`` (fused only): the width of every layer (``bit_config()``); 4-bit layers read packed codes with ``pack4``.  ``_switch``
        moves the recording to another list.  Every other sequence runs the plan's default width on int8-stored codes (the RESID mid-code
        tap and the records of ``p2v_gemm_i8`` behind it take those)."""
        a = self.arch
        self._no_capture('the recorded launch sequence of batch %d' % B)
        if attention and not self.int_softmax:
            raise NotImplementedError('the attention stages of the DDV and of the stage statistics need the log-int-softmax: the probabilities of the float softmax '
                                      '(Config(lis=False)) are not codes')
        if not fused or cfg is None:
            cfg = (self.bits,) * len(self._names)
        lin_ops = []

        def L_(d, frag=False):
            """(p2v_linear, RESID table or None) of layer ``d`` in this sequence"""
            bits = cfg[d['idx']]
            packed = fused and self._packed(bits)
            return self._lin(d, bits, packed, frag), (self._resid_tab(d, bits, packed) if d['epi'] is not None else None)
        P, g = a['patch_size'], self.g
        dev = self.device
        ops, taps, keep = [], [], []
        n = B if stats else ddv_n           # (what the stage sites, the mid codes and the scratch are gated on)
        stages, lin_out = [], []
        scratch = None
        if n and with_linear:           # the largest single tap of the 2n images
            big = max([B * g * g * a['embed_dim'], B * (self.head['N'] + 3)] +
                      [B * st_['H'] * st_['H'] * max(b_['qkv']['N'], b_['fc1']['N']) for st_ in self.stages for b_ in st_['blocks']])
            scratch = torch.empty(big, dtype=torch.float32, device=dev)
            keep.append(scratch)

        def stage(name, t_, rows, cols, stride, dtype=E.COS_I8, scale=None):
            """DDV stage ``name``: per image rows x cols elements of ``t_`` (row stride ``stride`` elements: padding behind ``cols`` is never read)"""
            if not n:
                return
            if stats:       # one record per stage: every sample of the live buffer, the addressing in the members P2V_OP_COS uses
                o = E.Op()
                o.kind, o.inp = E.OP_STATS, E.ptr(t_)
                o.i0, o.i1, o.M, o.N, o.lda = B, {E.COS_I8: E.STAT_I8, E.COS_F32: E.STAT_F32, E.COS_LOG2K: E.STAT_U8}[dtype], rows, cols, stride
                ss = rows * stride
                o.i2, o.i3 = ((ss & 0xffffffff) ^ 0x80000000) - 0x80000000, ss >> 32
                stages.append((name, len(ops), (cols, o.i1, scale)))
                ops.append(o)
                return
            esz = 4 if dtype == E.COS_F32 else 1
            lay = E.CosLayer(E.ptr(t_), C.c_void_p(t_.data_ptr() + n * rows * stride * esz), scale, rows * stride, stride, rows, cols, dtype)
            o = E.Op()
            o.kind, o.inp = E.OP_COS, E.ptr(t_)
            o.i0, o.i1, o.M, o.N, o.lda = n, dtype, rows, cols, stride
            ss = rows * stride
            o.i2, o.i3 = ((ss & 0xffffffff) ^ 0x80000000) - 0x80000000, ss >> 32
            o.lin.colscale = scale
            ops.append(o)
            stages.append((name, o, lay))

        def ftap(name, rows_total, N):
            """fp32 destination of layer ``name``'s output, or None: the one DDV scratch buffer / a buffer of its own for the linear taps"""
            if lin_taps:
                t_ = torch.empty(rows_total, N, dtype=torch.float32, device=dev)
                keep.append(t_)
                lin_out.append((name, t_))
                return t_
            if scratch is not None:
                return scratch[:rows_total * N].view(rows_total, N)
            return None

        def ftap_stage(name, t_, rows):
            if t_ is not None and n:
                stage(name, t_, rows, t_.shape[1], t_.shape[1], E.COS_F32)

        def gemm_f32(name, x, lin, rows):
            """layers whose epilogue has no fp32 tap (RESID, HEAD): one fp32-output GEMM over the layer's int8 input; rows of the output
            are a multiple of 16 bytes apart (a class count that is no multiple of 4)"""
            N, ld = lin['N'], (lin['N'] + 3) // 4 * 4
            t_ = ftap(name, x.shape[0], ld)
            if t_ is None:
                return
            o = E.Op()
            o.kind, o.inp, o.out = E.OP_GEMM_F32, E.ptr(x), E.ptr(t_)
            o.M, o.K, o.N, o.lda, o.ldo = x.shape[0], x.shape[1], N, x.shape[1], ld
            o.lin = L_(lin)[0]
            ops.append(o)
            if n:
                stage(name, t_, rows, N, ld, E.COS_F32)

        def buf(rows, cols, zero=False):
            t_ = (torch.zeros if zero else torch.empty)(rows, cols, dtype=torch.int8, device=dev)
            keep.append(t_)
            return t_

        def pad64(n):
            return (n + 63) // 64 * 64

        def gemm(kind, x, lin, epi, out):
            o = E.Op()
            o.kind, o.epi, o.inp, o.out = E.OP_GEMM, kind, E.ptr(x), E.ptr(out)
            o.M, o.K, o.N, o.lda, o.ldo = x.shape[0], x.shape[1], lin['N'], x.shape[1], out.shape[1]
            o.lin, o.ep = L_(lin)[0], epi
            if kind == E.EPI_RESID:
                o.ep.resid_tab = L_(lin)[1]
            lin_ops.append((len(ops), lin))
            ops.append(o)
            return out

        def ln_gemm(kind, x, ln, Cc, lin, epi, out):
            o = E.Op()
            o.kind, o.epi, o.inp, o.out = E.OP_LN_GEMM, kind, E.ptr(x), E.ptr(out)
            o.M, o.K, o.N, o.lda, o.ldo = x.shape[0], Cc, lin['N'], x.shape[1], lin['N']
            o.lin, o.ep, o.ln = L_(lin, frag=True)[0], epi, ln
            lin_ops.append((len(ops), lin))
            ops.append(o)
            return out

        def lnorm(x, ln, Cc, out):
            o = E.Op()
            o.kind, o.inp, o.out = E.OP_LAYERNORM, E.ptr(x), E.ptr(out)
            o.M, o.N, o.lda, o.ldo = x.shape[0], Cc, x.shape[1], out.shape[1]
            if isinstance(ln, E.FloatLn):       # Config(ptf=False): the constants in the members of the op table (include/p2vit.h)
                o.kind, o.f0, o.f1 = E.OP_FLOAT_LAYERNORM, ln.s_in, ln.eps
                o.lin.w_codes, o.lin.colscale, o.lin.bias = ln.gamma, ln.beta, ln.g
            else:
                o.ln = ln
            ops.append(o)
            return out

        def epi_req(inv_s, tap=None):
            e = E.Epilogue()
            e.inv_s_out = inv_s
            e.tap_out = E.ptr(tap)
            return e

        def epi_res(src, residual, mid=None):
            e = E.Epilogue()
            e.s_mid, e.s_res, e.s_next, e.residual = src.s_mid, src.s_res, src.s_next, E.ptr(residual)      # (resid_tab: per width, set by gemm)
            e.tap_out = E.ptr(mid)              # RESID records: the int8 mid-code destination (include/p2vit.h, op table)
            return e

        o = E.Op()
        patches = buf(B * g * g, self.k_patch, zero=True)
        o.kind, o.out = E.OP_PATCHIFY, E.ptr(patches)
        o.i0, o.i1, o.i2, o.i3, o.i4, o.i5, o.f0 = B, self.in_chans, a['img_size'], a['img_size'], P, self.k_patch, 1.0 / self.s_in
        ops.append(o)
        D0 = a['embed_dim']
        t_pe = ftap('patch_embed.proj', B * g * g, D0)
        pe = gemm(E.EPI_REQUANT, patches, self.pe, epi_req(1.0 / self.s_pe_b, t_pe), buf(B * g * g, D0))
        ftap_stage('patch_embed.proj', t_pe, g * g)
        stage('patch_embed.qact_before_norm', pe, g * g, D0, D0)
        x = lnorm(pe, self.pe_ln, D0, buf(B * g * g, D0))
        taps.append((len(ops), 'patch_embed.qact', x))
        stage('patch_embed.qact', x, g * g, D0, D0)
        for li, stg in enumerate(self.stages):
            T, Cc = stg['H'] * stg['H'], stg['C']
            rows = B * T
            x2 = buf(rows, Cc)
            ln = buf(rows, pad64(Cc))
            qkv = buf(rows, 3 * Cc)
            att = buf(rows, pad64(Cc))
            # the MLP's hidden codes: as wide as fc2 contracts over (int(Cc * mlp_ratio), walked in whole 64-deep k-tiles: columns behind
            # fc1's outputs stay zero and meet zero weight columns) - NOT 4 * Cc, which made fc2 read rows and weights of another width
            # whenever mlp_ratio was not 4
            fc1_n, hid_k = stg['blocks'][0]['fc1']['N'], stg['blocks'][0]['fc2']['K']
            hid = buf(rows, hid_k, zero=hid_k != fc1_n)
            mid = buf(rows, Cc) if n else None
            wb = stg['blocks'][0]
            Nw, nW = wb['ws'] * wb['ws'], wb['wa'].n_windows
            pitch = (Nw + 15) // 16 * 16
            planes = [buf(B * nW * wb['heads'] * Nw, pitch) for _ in range(3)] if (n and attention) else None
            for bi, b in enumerate(stg['blocks']):
                p = 'layers.%d.blocks.%d.' % (li, bi)
                t_qkv, t_fc1 = ftap(p + 'attn.qkv', rows, b['qkv']['N']), None
                e_fc1 = epi_req(b['inv_s_fc1'])
                e_fc1.gelu = E.gelu_table(b['inv_s_fc1'], self.device)       # exact GELU -> qact1 threshold table (cached per scale)
                fuse = (fused and self.int_norm and b['qkv']['frag'] and hid_k == fc1_n and E.lib().p2v_ln_gemm_fusable(E.EPI_REQUANT, Cc, b['qkv']['N'], 0) == 1
                        and E.lib().p2v_ln_gemm_fusable(E.EPI_GELU, Cc, b['fc1']['N'], e_fc1.gelu.cells if e_fc1.gelu.table else 0) == 1)
                if fuse:
                    ln_gemm(E.EPI_REQUANT, x, b['ln1'], Cc, b['qkv'], epi_req(b['inv_s_qkv']), qkv)
                else:
                    lnorm(x, b['ln1'], Cc, ln)
                    taps.append((len(ops), p + 'qact1', ln))
                    stage(p + 'qact1', ln, T, Cc, ln.shape[1])
                    gemm(E.EPI_REQUANT, ln, b['qkv'], epi_req(b['inv_s_qkv'], t_qkv), qkv)
                    ftap_stage(p + 'attn.qkv', t_qkv, T)
                    stage(p + 'attn.qact1', qkv, T, 3 * Cc, 3 * Cc)
                o = E.Op()
                o.kind, o.inp, o.out = E.OP_WINATTN, E.ptr(qkv), E.ptr(att)
                o.i0, o.i1, o.i2, o.i3 = B, T, b['heads'], 32
                o.wa = b['wa']
                o.wa.out_stride = att.shape[1]
                o.i4 = b['softmax_bits']     # the width of the log-int-softmax (0, an earlier record, = 4); the table softmax reads none
                if b['sm_tab'] is not None:  # Config(lis=False): the table softmax behind the same qact2 codes; the table in lin.w_codes
                    o.kind, o.lin.w_codes = E.OP_WINATTN_SOFTMAX, E.ptr(b['sm_tab'])
                if planes is not None:       # the tapped launch (op table of include/p2vit.h: members the record did not use before)
                    o.lin.w_codes, o.lin.w_frag, o.ep.tap_out, o.ldo = E.ptr(planes[0]), E.ptr(planes[1]), E.ptr(planes[2]), pitch
                ops.append(o)
                if planes is not None:
                    stage(p + 'attn.qact_attn1', planes[0], nW * b['heads'] * Nw, Nw, pitch)
                    stage(p + 'attn.qact2', planes[1], nW * b['heads'] * Nw, Nw, pitch)
                    stage(p + 'attn.log_int_softmax', planes[2], nW * b['heads'] * Nw, Nw, pitch, E.COS_LOG2K)
                stage(p + 'attn.qact3', att, T, Cc, att.shape[1])       # (the out_stride padding of att is never written: cols = Cc)
                gemm_f32(p + 'attn.proj', att, b['proj'], T)
                gemm(E.EPI_RESID, att, b['proj'], epi_res(b['proj_epi'], x, mid), x2)
                stage(p + 'attn.qact4', mid, T, Cc, Cc)
                taps.append((len(ops), p + 'qact2', x2))
                stage(p + 'qact2', x2, T, Cc, Cc, scale=b['proj_epi'].s_next)
                if fuse:
                    ln_gemm(E.EPI_GELU, x2, b['ln2'], Cc, b['fc1'], e_fc1, hid)
                else:
                    lnorm(x2, b['ln2'], Cc, ln)
                    stage(p + 'qact3', ln, T, Cc, ln.shape[1])
                    t_fc1 = ftap(p + 'mlp.fc1', rows, b['fc1']['N'])
                    e_fc1.tap_out = E.ptr(t_fc1)
                    gemm(E.EPI_GELU, ln, b['fc1'], e_fc1, hid)
                    ftap_stage(p + 'mlp.fc1', t_fc1, T)
                    stage(p + 'mlp.qact1', hid, T, fc1_n, hid.shape[1])
                gemm_f32(p + 'mlp.fc2', hid, b['fc2'], T)
                gemm(E.EPI_RESID, hid, b['fc2'], epi_res(b['fc2_epi'], x2, mid), x)
                stage(p + 'mlp.qact2', mid, T, Cc, Cc)
                taps.append((len(ops), p + 'qact4', x))
                stage(p + 'qact4', x, T, Cc, Cc, scale=b['fc2_epi'].s_next)
            if stg['merge'] is not None:
                m, H = stg['merge'], stg['H']
                r2 = B * (H // 2) * (H // 2)
                gathered = buf(r2, 4 * Cc)
                o = E.Op()
                o.kind, o.inp, o.out = E.OP_MERGE, E.ptr(x), E.ptr(gathered)
                o.i0, o.i1, o.i2, o.i3 = B, H, H, Cc
                ops.append(o)
                lnm = lnorm(gathered, m['ln'], 4 * Cc, buf(r2, 4 * Cc))
                stage('layers.%d.downsample.qact1' % li, lnm, r2 // B, 4 * Cc, 4 * Cc)
                gemm_f32('layers.%d.downsample.reduction' % li, lnm, m['red'], r2 // B)
                x = gemm(E.EPI_RESID, lnm, m['red'], epi_res(m['epi'], buf(r2, 2 * Cc, zero=True)), buf(r2, 2 * Cc))
                taps.append((len(ops), 'layers.%d.downsample.qact2' % li, x))
                stage('layers.%d.downsample.qact2' % li, x, r2 // B, 2 * Cc, 2 * Cc, scale=m['epi'].s_next)
        fin = lnorm(x, self.fin_ln, self.C_last, buf(x.shape[0], self.C_last))
        taps.append((len(ops), 'qact2', fin))
        stage('qact2', fin, self.H_last * self.H_last, self.C_last, self.C_last)
        pooled = buf(B, self.C_last)
        o = E.Op()
        o.kind, o.inp, o.out = E.OP_AVGPOOL, E.ptr(fin), E.ptr(pooled)
        o.i0, o.i1, o.i2, o.f0, o.f1 = B, self.H_last * self.H_last, self.C_last, self.s_f, 1.0 / self.s_pool
        ops.append(o)
        taps.append((len(ops), 'qact3', pooled))
        stage('qact3', pooled, 1, self.C_last, self.C_last)
        gemm_f32('head', pooled, self.head, 1)
        e = E.Epilogue()
        e.inv_s_out, e.s_out = 1.0 / self.s_out, self.s_out
        o = E.Op()
        o.kind, o.epi, o.inp = E.OP_GEMM, E.EPI_HEAD, E.ptr(pooled)
        o.M, o.K, o.N, o.lda, o.ldo = B, self.C_last, self.head['N'], self.C_last, self.head['N']
        o.lin, o.ep = L_(self.head)[0], e
        lin_ops.append((len(ops), self.head))
        ops.append(o)
        rec = dict(taps=taps, keep=keep, head=len(ops) - 1, lin_out=lin_out, cfg=tuple(cfg), lin_ops=lin_ops)
        if n:
            # the stages reference a STATIC logits buffer (their records hold its address); forward_ddv returns a copy
            ldl = (self.head['N'] + 3) // 4 * 4
            logits = torch.zeros(B, ldl, dtype=torch.float32, device=dev)
            o.out, o.ldo = E.ptr(logits), ldl
            stage('act_out', logits, 1, self.head['N'], ldl, E.COS_F32)
            keep.append(logits)
            rec.update(names=[st_[0] for st_ in stages], logits=logits)
        if stats:
            rec.update(stat_ops=[st_[1] for st_ in stages], stat_layout=[st_[2] for st_ in stages])
        elif n:
            L = E.lib()
            lays = (E.CosLayer * len(stages))(*[st_[2] for st_ in stages])
            dbytes = L.p2v_cos_stage_desc_bytes()
            host = (C.c_char * (dbytes * len(stages)))()
            items = L.p2v_cos_stage_descs(lays, len(stages), n, host)
            if items < 0:
                E.check(int(items))
            descs = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev)
            partials = torch.empty(int(items) * 3, dtype=torch.int64, device=dev)
            sums = torch.empty(len(stages), n, 3, dtype=torch.float64, device=dev)
            for k, (_, so, _) in enumerate(stages):
                so.out = E.ptr(partials)
                so.lin.w_codes = C.c_void_p(descs.data_ptr() + k * dbytes)
            o = E.Op()
            o.kind, o.inp, o.out = E.OP_COS_COMBINE, E.ptr(descs), E.ptr(sums)
            o.i0, o.i1 = n, len(stages)
            o.lin.w_codes = E.ptr(partials)
            ops.append(o)
            keep += [descs, partials]
            rec.update(sums=sums)
        rec['ops'] = (E.Op * len(ops))(*ops)
        rec['n'] = len(ops)
        return rec

    def _prepare(self, cfg):
        """freeze, on the caller's stream and thread, whatever a fused forward under ``cfg`` reads and the plan does not hold yet"""
        if not self._all_frozen:
            for d in self._layers:
                self._ensure(d, cfg[d['idx']], self._packed(cfg[d['idx']]))

    def _switch(self, r, cfg):
        """move the fused recording ``r`` to the widths ``cfg``: the ``lin`` and ``ep.resid_tab`` members of its GEMM / LN_GEMM records in
        the host op table, which ``p2v_run_ops`` reads when it is called.  Buffers, shapes and record kinds do not depend on a width."""
        old = r['cfg']
        for i, d in r['lin_ops']:
            bits = cfg[d['idx']]
            if bits != old[d['idx']]:
                o = r['ops'][i]
                packed = self._packed(bits)
                o.lin = self._lin(d, bits, packed, frag=o.kind == E.OP_LN_GEMM)
                if d['epi'] is not None:
                    o.ep.resid_tab = self._resid_tab(d, bits, packed)
        r['cfg'] = cfg

    def _fused_record(self, B, slot, cfg):
        """the one fused recording of (batch, slot), at the widths ``cfg``"""
        key = (B, slot, True)
        if key not in self._recorded:
            self._recorded[key] = self._record(B, fused=True, cfg=cfg)
        r = self._recorded[key]
        if r['cfg'] != cfg:
            self._switch(r, cfg)
        return r

    def _replay(self, images, slot, taps=None, profile=False, cfg=None):
        with torch.cuda.device(self.device):       # the recorded pointers and the launch stream belong to the plan's GPU
            return self._replay_on_device(images, slot, taps, profile, cfg or self.bit_config())

    def _replay_on_device(self, images, slot, taps, profile, cfg):
        B = images.shape[0]
        if taps is None:
            r = self._fused_record(B, slot, cfg)
        else:
            key = (B, slot, False, self.bits)
            if key not in self._recorded:
                self._recorded[key] = self._record(B, fused=False)
            r = self._recorded[key]
        out = torch.empty(B, self.head['N'], dtype=torch.float32, device=self.device)
        r['ops'][0].inp = E.ptr(images)
        r['ops'][r['n'] - 1].out = E.ptr(out)
        L = E.lib()
        if profile:
            ms = (C.c_float * r['n'])()
            E.check(L.p2v_run_ops_profile(r['ops'], r['n'], E.stream_ptr(self.device), ms))
            return out, list(ms)
        if taps is None:
            E.check(L.p2v_run_ops(r['ops'], r['n'], E.stream_ptr(self.device)))
            return out
        done = 0
        for upto, name, t_ in r['taps']:          # replay in segments and copy the tapped buffers (they are reused later)
            E.check(L.p2v_run_ops(C.cast(C.byref(r['ops'], done * C.sizeof(E.Op)), C.POINTER(E.Op)), upto - done, E.stream_ptr(self.device)))
            taps[name] = t_[:, :t_.shape[1]].clone()
            done = upto
        E.check(L.p2v_run_ops(C.cast(C.byref(r['ops'], done * C.sizeof(E.Op)), C.POINTER(E.Op)), r['n'] - done, E.stream_ptr(self.device)))
        return out

    def _replay_extra(self, images, key, **kw):
        """replay the recorded sequence ``key`` (made with ``_record(B, fused=False, **kw)`` on first use) in one ``p2v_run_ops`` call"""
        with torch.cuda.device(self.device):
            key = key + (self.bits,)
            if key not in self._recorded:
                self._recorded[key] = self._record(images.shape[0], fused=False, **kw)
            r = self._recorded[key]
            r['ops'][0].inp = E.ptr(images)
            out = None
            if 'logits' not in r:
                out = torch.empty(images.shape[0], self.head['N'], dtype=torch.float32, device=self.device)
                r['ops'][r['head']].out = E.ptr(out)
            E.check(E.lib().p2v_run_ops(r['ops'], r['n'], E.stream_ptr(self.device)))
            return r, out

    def forward_ddv(self, images_2n, with_linear=True, attention=False):
        """The DDV of the quantized model inside the forward: ``images_2n`` = n clean images followed by their n perturbed twins.
        Returns (logits [2n, classes], byte-equal to ``forward``; stage names = ``ddv.swin_stage_names(depths, with_linear)``; sums fp64
        [stages, n, 3] = sum a.b, sum a.a, sum b.b per stage and pair).  One recorded sequence, one ``p2v_run_ops`` call on the current
        stream: every stage is reduced from the live buffer right behind the launch that completes it (the LayerNorm outputs exist in HBM
        because the unfused sequence is recorded; attn.qact4 / mlp.qact2 come from the mid-code output of the RESID epilogue), one combine
        launch closes it.  ``attention``: also the QActs inside the window kernel - attn.qact_attn1, attn.qact2 (codes) and
        attn.log_int_softmax (the log2 probabilities at the block's softmax width), exact sums from the tapped window launch; stage names =
        ``ddv.swin_stage_names(depths, with_linear, attention=True)``.  qact_table does not depend on the input and is not a stage."""
        images_2n = self._check_images(images_2n)
        if images_2n.shape[0] < 2 or images_2n.shape[0] % 2:
            raise AssertionError('forward_ddv takes n clean images followed by their n perturbed twins, got %d images' % images_2n.shape[0])
        n = images_2n.shape[0] // 2
        key = ('ddv', n, bool(with_linear)) + (('attn',) if attention else ())
        r, _ = self._replay_extra(images_2n, key, ddv_n=n, with_linear=bool(with_linear), attention=bool(attention))
        return r['logits'][:, :self.head['N']].clone(), list(r['names']), r['sums'].clone()

    def forward_stats(self, x, with_linear=False, attention=False, into=None):
        """(logits, ``stats.StageStats``) of the quantized model inside the forward, for any batch >= 1: the stages of ``forward_ddv``
        (``ddv.swin_stage_names(depths, with_linear, attention)``), each reduced over all images and tokens by one ``P2V_OP_STATS`` record
        right behind the launch that completes it - per channel the lowest and highest code and the integer sums, and the histogram of
        the codes (fp32 stages: of the exponent field).  One recorded sequence, one ``p2v_run_ops`` call.  ``attention``: the window
        launches run tapped, with the three planes.  ``into``: a result of an earlier call with the same arguments; the batch is
        accumulated into its records on the device, without a host synchronisation."""
        from .stats import StageStats
        x = self._check_images(x)
        B = x.shape[0]
        key = ('stats', B, bool(with_linear)) + (('attn',) if attention else ())
        with torch.cuda.device(self.device):
            full_key = key + (self.bits,)
            if full_key not in self._recorded:
                self._recorded[full_key] = self._record(B, fused=False, with_linear=bool(with_linear), attention=bool(attention), stats=True)
            r = self._recorded[full_key]
            names = list(r['names'])
            skey = ('swin', id(self), self.bits, bool(with_linear), bool(attention))
            if into is None:
                by_ptr = {t.data_ptr(): t for t in self._keep}
                scales = []
                for nm, (cols, kind, sc) in zip(names, r['stat_layout']):
                    sc = getattr(sc, 'value', sc)
                    if sc:
                        scales.append(by_ptr[sc][:cols])
                    else:
                        c = self.c.get(nm) if kind == E.STAT_I8 else None
                        scales.append(float(c.reshape(-1)[0]) if c is not None and c.numel() == 1 else None)
                into = StageStats.empty(names, [l[0] for l in r['stat_layout']], [l[1] for l in r['stat_layout']], scales, self.device, key=skey)
            elif into.key != skey or into.names != names:
                raise AssertionError('forward_stats(into=...): the result was made by another plan or with other stages')
            for k, i in enumerate(r['stat_ops']):
                r['ops'][i].out = C.c_void_p(into.arena.data_ptr() + into.offsets[k])
            r['ops'][0].inp = E.ptr(x)
            E.check(E.lib().p2v_run_ops(r['ops'], r['n'], E.stream_ptr(self.device)))
            return r['logits'][:, :self.head['N']].clone(), into

    def forward_linear_taps(self, images):
        """(logits, [fp32 tensors]): the output of every QConv2d / QLinear in ``named_modules`` order (patch_embed.proj; qkv, proj, fc1,
        fc2 of every block; downsample.reduction behind a stage's blocks; head) as [B, tokens, N] in NATURAL token order ([B, N] for the
        head).  The module graph would hand qkv and proj over in window order ([B * nW, ws * ws, N]): the same values with the tokens of an
        image permuted.  A Gram matrix over the flattened features of an image (CKA) does not see a permutation of features."""
        images = self._check_images(images)
        B = images.shape[0]
        r, out = self._replay_extra(images, ('lin', B), lin_taps=True)
        return out, [t_[:, :self.head['N']].clone() if nm == 'head' else t_.view(B, -1, t_.shape[1]).clone() for nm, t_ in r['lin_out']]

    def linear_tap_names(self):
        names = ['patch_embed.proj']
        for li, st_ in enumerate(self.stages):
            for bi in range(len(st_['blocks'])):
                names += ['layers.%d.blocks.%d.%s' % (li, bi, k) for k in ('attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2')]
            if st_['merge'] is not None:
                names.append('layers.%d.downsample.reduction' % li)
        return names + ['head']

    def _check_images(self, images):
        a = self.arch
        images = images.contiguous().float()
        if images.device != self.device:
            raise RuntimeError('images must live on %s' % self.device)
        if tuple(images.shape[1:]) != (self.in_chans, a['img_size'], a['img_size']):
            raise AssertionError("Input image size (%d*%d) doesn't match model (%d*%d)." % (images.shape[2], images.shape[3], a['img_size'], a['img_size']))
        return images

    def input_lut(self, lut_f32):
        """the int8 table [C, 256] ``forward_uint8`` reads: the codes of data.uint8_lut's values under qact_input (data.uint8_lut_i8)"""
        from .data import uint8_lut_i8
        return uint8_lut_i8(lut_f32.detach().float().cpu(), 1.0 / self.s_in).contiguous().to(self.device)

    def _replay_u8(self, images, lut, layout, slot, cfg=None):
        """the recorded sequence with its first launch replaced: p2v_u8_patchify writes the same patch matrix into the recorded buffer"""
        with torch.cuda.device(self.device):
            B = images.shape[0]
            r = self._fused_record(B, slot, cfg or self.bit_config())
            out = torch.empty(B, self.head['N'], dtype=torch.float32, device=self.device)
            p = r['ops'][0]
            L, st = E.lib(), E.stream_ptr(self.device)
            E.check(L.p2v_u8_patchify(E.ptr(images), E.LAYOUTS[layout], E.ptr(lut), B, p.i1, p.i2, p.i3, p.i4, p.out, p.i5, st))
            r['ops'][r['n'] - 1].out = E.ptr(out)
            E.check(L.p2v_run_ops(C.cast(C.byref(r['ops'], C.sizeof(E.Op)), C.POINTER(E.Op)), r['n'] - 1, st))
            return out

    def forward_uint8(self, images, lut, layout='NHWC', n_streams=3, slices=None, bit_config=None):
        """``forward`` on uint8 images ([B, S, S, C] for 'NHWC', [B, C, S, S] for 'NCHW') read through ``lut`` (``input_lut``), single or
        sliced like ``forward``: the logits equal ``forward`` on the images data.normalize_uint8 makes of them.  ``bit_config``: as in
        ``forward``."""
        cfg = self.bit_config(bit_config)
        a, S, Cin = self.arch, self.arch['img_size'], self.in_chans
        if layout not in E.LAYOUTS:
            raise AssertionError("layout must be 'NHWC' or 'NCHW', got %r" % (layout,))
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
            raise AssertionError('forward_uint8 takes uint8 images, got %s (fp32 images go to forward)' % getattr(images, 'dtype', type(images)))
        want = (S, S, Cin) if layout == 'NHWC' else (Cin, S, S)
        if images.dim() != 4 or tuple(images.shape[1:]) != want or images.shape[0] < 1:
            raise AssertionError('uint8 images in layout %s must be [B, %d, %d, %d], got %s' % ((layout,) + want + (tuple(images.shape),)))
        if images.device != self.device:
            raise RuntimeError('images must live on %s' % self.device)
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.int8 or tuple(lut.shape) != (Cin, 256) or lut.device != self.device or not lut.is_contiguous():
            raise AssertionError('lut must be a contiguous int8 [%d, 256] tensor on %s (SwinPlan.input_lut)' % (Cin, self.device))
        images = images.contiguous()
        with torch.cuda.device(self.device):
            self._prepare(cfg)
        return self._sliced(images, n_streams, slices, lambda x, slot: self._replay_u8(x, lut, layout, slot, cfg))

    def forward(self, images, taps=None, n_streams=3, slices=None, bit_config=None):
        """images fp32 [B, in_chans, S, S] on the plan's device -> logits fp32 [B, classes] (act_out grid).  One C call replays
        the recorded launch sequence; a large batch runs as ``n_streams`` contiguous slices on their own HIP streams (images are
        independent), like the ViT plan (three: Swin-B at 256 images 25.1 k img/s against 24.6 k on two, same call, profiles/r04_slices.txt).
        ``slices``: explicit slice sizes; slices beyond ``n_streams`` run on the caller's stream.
        ``bit_config``: one width (4 or 8) per QConv2d / QLinear in the order of ``linear_tap_names()``; None = the plan's default width
        everywhere.  Another list costs no rebuild and no device memory: the one recording of a (batch, slot) is moved to it (``_switch``),
        and codes the plan does not hold yet are frozen on the caller's stream first (``freeze_all`` does that ahead of time)."""
        cfg = self.bit_config(bit_config)
        images = self._check_images(images)
        if taps is not None:
            if bit_config is not None:
                raise NotImplementedError('the tapped forward runs the plan\'s one default width: no bit_config list')
            return self._replay(images, 0, taps)
        with torch.cuda.device(self.device):
            self._prepare(cfg)
        return self._sliced(images, n_streams, slices, lambda x, slot: self._replay(x, slot, cfg=cfg))

    def _sliced(self, images, n_streams, slices, replay):
        """the batch slicing of ``forward``; ``replay(images, slot)`` runs one slice on the current stream"""
        B = images.shape[0]
        n_streams = min(n_streams, E.compute_side_streams(self.device))       # (one less while an input pipeline copies on engine.copy_stream)
        if n_streams <= 1 or (slices is None and B < 16 * n_streams):
            return replay(images, 0)
        if slices is None:
            step = (B + n_streams - 1) // n_streams
            slices = [min(step, B - i * step) for i in range(n_streams) if i * step < B]
        if sum(slices) != B or min(slices) < 1:
            raise AssertionError('slices %r do not cover a batch of %d' % (list(slices), B))
        if torch.cuda.is_current_stream_capturing():      # before the fork: an exception between fork and join would leave the capture unjoined
            for i, part in enumerate(images.split(list(slices))):
                slot = i + 1 if i < min(n_streams, len(slices)) else 0
                if (part.shape[0], slot, True) not in self._recorded:
                    self._no_capture('the recorded launch sequence of slice %d (batch %d)' % (i, part.shape[0]))
        self._streams = E.side_streams(self.device, n_streams)          # the process's shared side streams of this device (engine.side_streams)
        n_side = min(n_streams, len(slices))
        parts = images.split(list(slices))
        outs = [None] * len(parts)

        # side slice i on side stream i with its own recording (slot i + 1); slices beyond the side streams run on the caller's own stream
        # (slot 0: its single-stream record).  Worker threads (engine.run_on_streams) once the launch sequences are recorded: the replay is
        # one C call of ~1 ms of host time per slice
        def job(i):
            def on_side_stream(st):
                with torch.cuda.stream(st):            # (the current stream is a per-thread setting)
                    outs[i] = replay(parts[i], i + 1)

            def on_callers_stream(st):
                outs[i] = replay(parts[i], 0)
            return on_side_stream if i < n_side else on_callers_stream

        jobs = [[job(i)] for i in range(n_side)] + [[job(i) for i in range(n_side, len(parts))]]
        recorded = all((parts[i].shape[0], i + 1, True) in self._recorded for i in range(n_side))
        E.run_on_streams(self.device, self._streams[:n_side], jobs, threads=recorded)
        cur = torch.cuda.current_stream(self.device)
        for o in outs:
            o.record_stream(cur)
        return torch.cat(outs, 0)

    def profile(self, images):
        """per-op durations (ms, HIP events on the launch stream) of one single-stream forward: [(kind, epilogue, ms), ...]."""
        images = self._check_images(images)
        _, ms = self._replay(images, 0, profile=True)
        r = self._recorded[(images.shape[0], 0, True)]
        names = {E.OP_PATCHIFY: 'patchify', E.OP_GEMM: 'gemm', E.OP_LAYERNORM: 'layernorm', E.OP_WINATTN: 'window_attention',
                 E.OP_MERGE: 'merge_gather', E.OP_AVGPOOL: 'avgpool', E.OP_LN_GEMM: 'ln_gemm', E.OP_WINATTN_SOFTMAX: 'window_softmax_attention',
                 E.OP_FLOAT_LAYERNORM: 'float_layernorm'}
        return [(names[r['ops'][i].kind], int(r['ops'][i].epi), ms[i]) for i in range(r['n'])]
