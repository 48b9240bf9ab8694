"""Freeze a calibrated PoT-PTQ ViT into the integer plan the HIP engine executes.

The reference keeps its calibrated state in Python attributes (``quantizer.scale``, ``dic_scale``,
``best_scale/best_act_scale/best_weight_scale`` -- models/vit_fquant.py:234-239,273-278) and re-derives
everything on every forward: weights are fake-quantised per call (models/ptq/layers.py:177,
quantizer/uniform.py:82-88), LN multipliers and softmax constants are recomputed per call
(layers.py:255-289,334-351).  Freezing does that work once, with the same fp32 operations, and uploads
the result; ``forward`` then is one C call (``p2v_forward``).

Input is a *calibration dict* (nested: name -> tensor | {bit_name: tensor} | [per-bit-pool-index ...]),
the format ``export_calib`` produces from the module surface; plus the fp32 ``state_dict``.
"""
import ctypes as C
import warnings
import weakref

import numpy as np
import torch

from . import engine as E

BIT_POOL = (4, 8)                                # models/vit_fquant.py:33
BOUNDS = {4: (-8, 7), 8: (-128, 127)}            # models/ptq/bit_type.py:17-27 for int4 / int8
GEMM_N_PAD, GEMM_K_PAD = 128, 64


def _is_pot(t):
    m, _ = torch.frexp(t.detach().float().reshape(-1))
    return bool(torch.all(m == 0.5))


def _need_pot(name, t):
    if not _is_pot(t):
        # the kernels replace x / s by exact multiplications with 1/s; only valid for PoT scales
        raise NotImplementedError('%s is not a power of two (observer other than the PoT minmax?)' % name)
    return t.detach().float()


def _q8(v, s):
    return torch.clamp(torch.round(v / s), -128, 127)


def lis_consts(sf):
    """x0_int, b_int, c_int with the reference's fp32 expressions (models/ptq/layers.py:334-351)."""
    sf = sf.detach().float().reshape(())
    x0 = torch.floor(-0.6931 / sf)
    b = torch.floor((0.96963238 / 0.35815147) / sf)
    c = torch.floor((1. / 0.35815147) / sf**2)
    x0, b, c = int(x0), int(b), int(c)
    # the kernels keep z = r (r + b) + c exactly in fp32 and the exp table in int64 (include/p2vit.h, Limits): refuse at plan time
    if not (-(1 << 12) <= x0 < 0 and 0 <= b < (1 << 23) and 0 < c < (1 << 24)):
        raise NotImplementedError('log-int-softmax input scale %g is outside the exact range of the attention kernel '
                                  '(x0_int %d, b_int %d, c_int %d; scales from 2^-11 up are covered)' % (float(sf), x0, b, c))
    return x0, b, c


SOFTMAX_FRAC_BITS = 21


def softmax_table(s_attn):
    """the 256-entry fixed-point exp table of the float softmax (Config(lis=False)): tab[d] = min(rne(exp(-s d) 2^21), 2^21 - 1) for
    d = max - code, in fp64 on the host; operator input of p2v_softmax_attention (the kernel never evaluates exp)."""
    s = float(torch.as_tensor(s_attn).reshape(-1)[0])
    e = np.rint(np.exp(-s * np.arange(256, dtype=np.float64)) * float(1 << SOFTMAX_FRAC_BITS))
    return np.minimum(e, float((1 << SOFTMAX_FRAC_BITS) - 1)).astype(np.uint32)


SOFTMAX_BITS = (3, 4)                            # the widths of the log-int-softmax on the engine (uint3 / uint4 of Config.BIT_TYPE_S)


def softmax_bits_list(softmax_bits, n, who='softmax_bits'):
    """``softmax_bits`` of a plan as one width per attention module: None (4 everywhere), an int, or ``n`` entries"""
    if softmax_bits is None:
        return [4] * n
    if isinstance(softmax_bits, (int, np.integer)) and not isinstance(softmax_bits, bool):
        vals = [int(softmax_bits)] * n
    else:
        vals = [int(b) for b in softmax_bits]
        if len(vals) != n:
            raise ValueError('%s has %d entries, the model has %d attention modules' % (who, len(vals), n))
    for i, b in enumerate(vals):
        if b not in SOFTMAX_BITS:
            raise NotImplementedError('%s[%d] = %d: the log-int-softmax runs at 3 or 4 bits on the engine' % (who, i, b))
    return vals


def module_softmax_bits(model, int_softmax=True):
    """What ``freeze`` reads off the module graph: the width of every QIntSoftmax in module order (its own ``bit_type``, as
    QIntSoftmax.forward reads it), and a refusal - ``NotImplementedError`` naming the module path - of what the engine would otherwise
    ignore: a log-int-softmax that is neither uint3 nor uint4, a QAct that is not int8 (Config.BIT_TYPE_A = uint8).  Under
    ``int_softmax=False`` the softmax bit type (uint8) is unused, as in the reference."""
    from .ptq.layers import QAct, QIntSoftmax
    widths = []
    for name, m in model.named_modules():
        if type(m) is QAct and m.bit_type.name != 'int8':
            raise NotImplementedError('%s: QAct bit type %s: the HIP engine runs int8 activations only' % (name, m.bit_type.name))
        if type(m) is QIntSoftmax:
            if int_softmax and m.bit_type.name not in ('uint3', 'uint4'):
                raise NotImplementedError('%s: log-int-softmax bit type %s: the HIP engine runs uint3 and uint4' % (name, m.bit_type.name))
            widths.append(m.bit_type.bits if int_softmax else 4)
    return widths


def calib_softmax_bits(calib, paths, softmax_bits=None):
    """the width of the attention modules ``paths``, in order, from a plan's ``softmax_bits`` argument and the calibration state.
    ``export_calib`` writes the key ``<path>.log_int_softmax.bits`` only where the width is not 4, so a missing key says nothing:
    with ``softmax_bits`` None a named width is taken and the rest are 4 (files and dicts without the key read as 4); with an argument
    (an int or one entry per module) a named width that disagrees with it is refused - ``ValueError`` naming the module - instead of
    one of the two being ignored."""
    named = [int(round(float(torch.as_tensor(calib[p + '.log_int_softmax.bits']).reshape(-1)[0]))) if (p + '.log_int_softmax.bits') in calib else None
             for p in paths]
    if softmax_bits is None:
        return softmax_bits_list([4 if b is None else b for b in named], len(paths), 'log_int_softmax.bits')
    vals = softmax_bits_list(softmax_bits, len(paths))
    for p, b, v in zip(paths, named, vals):
        if b is not None and b != v:
            raise ValueError('%s.log_int_softmax.bits = %d in the calibration state, softmax_bits says %d' % (p, b, v))
    return vals


def _per_channel(t, D):
    """a QAct scale as D per-channel values: the PTF vector, or the one layer-wise scale of Config(ptf=False) repeated"""
    t = t.detach().float().reshape(-1)
    return t.expand(D).contiguous() if t.numel() == 1 else t


class FrozenPlan:
    """Device-resident integer plan + handle of the C plan object."""

    def __init__(self, arch, state_dict, calib, device='cuda', in_chans=3, input_quant=True, int_norm=True, int_softmax=True, ln_eps=1e-6,
                 softmax_bits=None):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FrozenPlan: building a plan uploads and synchronises, which a stream that is capturing a graph cannot do: '
                               'freeze the model and run one eager forward before the capture')
        self.arch = dict(arch)
        # width of every block's log-int-softmax (the bit type of its QIntSoftmax: p = 2^-k for k < 2^bits, else 0): None = what the
        # calibration state names (export_calib of a uint3 model), else 4; an int, or one entry per block, which a named width must
        # agree with.  Unused (as in the reference) under int_softmax=False
        self.softmax_bits = calib_softmax_bits(calib, ['blocks.%d.attn' % i for i in range(self.arch['depth'])], softmax_bits)
        # Config(ptf, lis): False selects the float LayerNorm (F.layer_norm -> QAct) / the float softmax as the engine's fp64 / table operators
        self.int_norm, self.int_softmax, self.ln_eps = bool(int_norm), bool(int_softmax), float(ln_eps)
        self.input_quant = bool(input_quant)      # False: the fp32 image feeds the patch-embed convolution (vit_fquant.py:705, :925)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('FrozenPlan needs a GPU device: the quantized forward runs on the HIP engine only (no CPU path)')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.in_chans = in_chans
        self._keep = []          # tensors whose device pointers the C plan borrows
        self._handle = C.c_void_p()
        self._ws = None
        self._ws_batch = 0
        self._ws_multi = []      # grow-only workspace of slice i of the sliced forward
        self._streams = []       # the side streams the last sliced forward borrowed (engine.side_streams)
        a = self.arch
        self.D, self.depth, self.H = a['embed_dim'], a['depth'], a['num_heads']
        self.hidden = int(self.D * a['mlp_ratio'])
        self.patches = (a['img_size'] // a['patch_size']) ** 2
        self.tokens = self.patches + 1
        self.n_layers = 4 * self.depth + 2
        L = E.lib()
        desc = E.ModelDesc(E.P2V_ABI_VERSION, a['img_size'], a['patch_size'], in_chans, self.D, self.depth, self.H,
                           self.hidden, a['num_classes'])
        E.check(L.p2v_plan_create(C.byref(desc), C.byref(self._handle)))
        if not (self.int_norm and self.int_softmax):
            if not hasattr(L, 'p2v_plan_set_float_ops'):
                raise RuntimeError('libp2vit_hip.so lacks p2v_plan_set_float_ops (Config(ptf=False) / Config(lis=False)): rebuild')
            try:      # refused where the plan is created: head_dim other than 32 / 64 or more than 608 tokens under lis=False
                E.check(L.p2v_plan_set_float_ops(self._handle, int(not self.int_norm), int(not self.int_softmax)))
            except Exception:
                L.p2v_plan_destroy(self._handle)
                self._handle = C.c_void_p()
                raise
        W = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        # every upload and the plan-time fold of p2v_plan_set_block (a hipMalloc + copies) happen with the plan's device current,
        # whichever device the caller has selected (a plan for cuda:1 built while cuda:0 is current)
        with torch.cuda.device(self.device):
            self._build(W, calib)
        from . import ops                      # torch.ops.p2vit.forward(handle, images, bit_config)
        ops._PLANS[self.handle] = weakref.proxy(self)

    @property
    def handle(self):
        """integer value of the C plan pointer (the ``plan`` argument of ``torch.ops.p2vit.forward``)."""
        return int(self._handle.value or 0)

    @property
    def attention_kernel(self):
        """'resident' | 'packed' | 'stream': the attention kernel the forward of this geometry launches under the current switches - the
        library's own selection (p2v_attention_kernel), asked at every read; 'softmax' for a lis=False plan (k_softmax_attention)."""
        if not self.int_softmax:
            return 'softmax'
        which = E.lib().p2v_attention_kernel(self.D // self.H, self.tokens, 0)
        if which < 0:
            raise NotImplementedError('no attention kernel for head_dim %d at %d tokens' % (self.D // self.H, self.tokens))
        return ('resident', 'packed', 'stream')[which]

    # ---------------------------------------------------------------------------------------------
    def _dev(self, t, dtype=torch.float32):
        t = t.detach().to(dtype).contiguous().to(self.device)
        self._keep.append(t)
        return t

    def _linear(self, layer, w, cs, s_x, dic, bias, pack4=True, per_bit=False):
        """QLinear/QConv2d weight for both bit widths (layers.py:173-178; uniform.py:82-88).  ``pack4`` False keeps 4-bit codes one
        per byte (the fp32-input patch embedding reads unpacked codes).  ``per_bit`` (qkv / fc1): ``cs``, ``s_x`` and ``dic`` are lists,
        the SmoothQuant state is looked up per bit-pool index (vit_fquant.py:282-292); these layers follow a LayerNorm, so a second copy
        in MFMA-fragment order feeds the fused LayerNorm+GEMM kernel."""
        L = E.lib()
        w = w.reshape(w.shape[0], -1)
        N, K = w.shape
        n_pad = (N + GEMM_N_PAD - 1) // GEMM_N_PAD * GEMM_N_PAD
        k_pad = (K + GEMM_K_PAD - 1) // GEMM_K_PAD * GEMM_K_PAD
        for bi, bits in enumerate(BIT_POOL):
            name = 'int%d' % bits
            cs_b, s_x_b, dic_b = (cs[bi], s_x[bi], dic[bi]) if per_bit else (cs, s_x, dic)
            w2 = w if cs_b is None else w * cs_b.reshape((1, -1))          # weight_smoothed, vit_fquant.py:285
            s_w = _need_pot('%d.%s weight scale' % (layer, name), dic_b[name]).reshape(-1)
            s_x_b = _need_pot('%d act scale' % layer, s_x_b).reshape(-1)
            lo, hi = BOUNDS[bits]
            wp = torch.zeros(n_pad, k_pad, dtype=torch.int8)
            wp[:N, :K] = torch.clamp(torch.round(w2 / s_w.reshape(-1, 1)), lo, hi).to(torch.int8)
            cs_col = torch.zeros(n_pad)
            cs_col[:N] = (s_x_b * s_w).expand(N)
            bp = torch.zeros(n_pad)
            if bias is not None:
                bp[:N] = bias
            # 4-bit weights travel packed, two codes per byte (half the HBM bytes of BASELINE config 5), as LDS tile images
            packed = bits == 4 and pack4
            wdev = self._dev(E.pack_int4_tiles(wp), torch.uint8) if packed else self._dev(wp, torch.int8)
            frag = None
            if per_bit and self.D <= 384:        # 4-bit layers: the fragment copy travels packed too (two codes per byte, ABI 4)
                frag = E.ptr(self._dev(E.fragment_order_packed4(wp), torch.uint8) if bits == 4 else self._dev(E.fragment_order(wp), torch.int8))
            lin = E.Linear(E.ptr(wdev), E.ptr(self._dev(cs_col)), E.ptr(self._dev(bp)), frag, 1 if packed else 0)
            E.check(L.p2v_plan_set_linear(self._handle, layer, bits, C.byref(lin)))

    def _ln(self, in_scale, gamma, beta, out_scale, post_mul):
        """Constants of QIntLayerNorm mode 'int' (layers.py:255-289)."""
        in_scale = in_scale.reshape(-1).float()
        D = gamma.numel()
        s1 = in_scale.min()
        mask = torch.round(in_scale / s1).expand(D) if in_scale.numel() == 1 else torch.round(in_scale / s1)
        # the kernel keeps sum(x_q^2) exactly in 32 unsigned bits: C * (128 * mask)^2 < 2^32 (PTF masks are 1, 2, 4 or 8: ptf.py:96-134)
        if float(mask.min()) < 1 or D * (128.0 * float(mask.max())) ** 2 >= 2.0 ** 32:
            raise NotImplementedError('LayerNorm input scale ratios up to %g over %d channels exceed the exact 32-bit statistics' % (float(mask.max()), D))
        out_scale = _need_pot('LN out scale', out_scale.reshape(-1).expand(D).contiguous())
        post_mul = _need_pot('LN post multiplier', post_mul.reshape(-1).expand(D).contiguous())
        return E.Ln(float(s1), E.ptr(self._dev(mask)), E.ptr(self._dev(gamma)), E.ptr(self._dev(beta)),
                    E.ptr(self._dev(1.0 / out_scale)), E.ptr(self._dev(post_mul)))

    def _fln(self, s_in, gamma, beta, g):
        """constants of the float LayerNorm -> QAct (p2v_float_ln): ONE power-of-two input scale, g = 1 / (channel scale * s_out)"""
        s_in = _need_pot('float LayerNorm input scale', s_in.reshape(-1))
        if float(s_in.min()) != float(s_in.max()):
            raise NotImplementedError('float LayerNorm behind a per-channel input scale')
        D = gamma.numel()
        g = _need_pot('float LayerNorm output multiplier', g.reshape(-1).expand(D).contiguous())
        return E.FloatLn(float(s_in[0]), self.ln_eps, E.ptr(self._dev(gamma)), E.ptr(self._dev(beta)), E.ptr(self._dev(g)))

    def _build(self, W, c):
        L = E.lib()
        a, D = self.arch, self.D
        hd = D // self.H
        # ---- stem ------------------------------------------------------------------------------
        if self.input_quant:
            s_in = _need_pot('qact_input', c['qact_input'])
            self._linear(0, W['patch_embed.proj.weight'], None, s_in, c['patch_embed.proj'], W['patch_embed.proj.bias'])
        else:      # no input QAct: colscale = s_w, unpacked codes; p2v_plan_set_embed(inv_s_input = 0) selects the fp32-image kernel
            s_in = torch.ones(1)
            self._linear(0, W['patch_embed.proj.weight'], None, s_in, c['patch_embed.proj'], W['patch_embed.proj.bias'], pack4=False)
        s_pe = _need_pot('patch_embed.qact', c['patch_embed.qact'])
        s_e = _need_pot('qact_embed', c['qact_embed'])
        s_p = _need_pot('qact_pos', c['qact_pos'])
        s_res = _per_channel(c['qact1'], D)                                   # PTF: arbitrary fp32
        pos_deq = (_q8(W['pos_embed'], s_p) * s_p).reshape(self.tokens, D)
        cls_v = _q8(W['cls_token'].reshape(1, D), s_e) * s_e + pos_deq[0:1]   # vit_fquant.py:718-725
        cls_codes = _q8(cls_v, s_res.reshape(1, -1)).reshape(D)
        epi = E.Epilogue()
        epi.inv_s_pe = float(1.0 / s_pe)
        epi.pe_to_embed = float(s_pe / s_e)
        epi.s_embed = float(s_e)
        epi.s_next = E.ptr(self._dev(s_res))
        epi.pos_deq = E.ptr(self._dev(pos_deq))
        epi.patches = self.patches
        self.inv_s_input = float(1.0 / s_in) if self.input_quant else 0.0
        E.check(L.p2v_plan_set_embed(self._handle, self.inv_s_input, C.byref(epi),
                                     E.ptr(self._dev(cls_codes, torch.int8))))
        # the FULL DDV stages: the class row of the qact_embed plane, and whether qact_pos holds anything but zeros (ddv.compute_ddv)
        if hasattr(L, 'p2v_plan_set_embed_tap_cls'):      # (additive: side builds of older revisions lack it)
            E.check(L.p2v_plan_set_embed_tap_cls(self._handle, E.ptr(self._dev(_q8(W['cls_token'].reshape(D), s_e), torch.int8))))
        self.qact_pos_all_zero = not bool((_q8(W['pos_embed'], s_p) != 0).any())
        # the one scale of every stage whose codes share it (forward_stats; the per-channel ones come with the library's layout)
        self.stage_scales = {'qact_input': float(s_in), 'patch_embed.qact': float(s_pe), 'qact_embed': float(s_e)}
        # ---- blocks ----------------------------------------------------------------------------
        for i in range(self.depth):
            p = 'blocks.%d.' % i
            blk = E.Block()
            cs_a, s_a0 = c[p + 'attn.best_scale'], c[p + 'attn.best_act_scale']
            cs_m, s_m0 = c[p + 'mlp.best_scale'], c[p + 'mlp.best_act_scale']
            g1, b1 = W[p + 'norm1.weight'], W[p + 'norm1.bias']
            g2, b2 = W[p + 'norm2.weight'], W[p + 'norm2.bias']
            s_b2 = _per_channel(c[p + 'qact2'], D)
            s_b4 = _per_channel(c[p + 'qact4'], D)
            fblk = E.FloatBlock()
            s_q1 = _need_pot(p + 'attn.qact1', c[p + 'attn.qact1'])
            s_at = _need_pot(p + 'attn.qact_attn1', c[p + 'attn.qact_attn1'])
            s_a2 = _need_pot(p + 'attn.qact2', c[p + 'attn.qact2'])
            s_m1 = _need_pot(p + 'mlp.qact1', c[p + 'mlp.qact1'])
            self.stage_scales.update({p + 'attn.qact1': float(s_q1), p + 'attn.qact_attn1': float(s_at), p + 'attn.qact2': float(s_a2),
                                      p + 'mlp.qact1': float(s_m1)})
            for bi in range(2):
                csb = _need_pot(p + 'attn.channel_scale', cs_a[bi])
                sab = _need_pot(p + 'attn.qact0', s_a0[bi])
                out_scale = sab * csb                                          # layers.py:264-265
                blk.ln1[bi] = self._ln(s_res, g1, b1, out_scale, out_scale / csb / sab)
                if not self.int_norm:
                    fblk.ln1[bi] = self._fln(s_res, g1, b1, 1.0 / (csb * sab))
                blk.inv_s_qkv[bi] = float(1.0 / s_q1)
                for bm in range(2):
                    csm = _need_pot(p + 'mlp.channel_scale', cs_m[bm])
                    smb = _need_pot(p + 'mlp.qact0', s_m0[bm])
                    o2 = smb * csb                                             # attention's scale: vit_fquant.py:464
                    blk.ln2[bi][bm] = self._ln(s_b2, g2, b2, o2, o2 / csm / smb)
                    if not self.int_norm:
                        fblk.ln2[bi][bm] = self._fln(s_b2, g2, b2, 1.0 / (csm * smb))
            # qkv / fc1 depend on the bit-pool index through best_* (identical when |alpha_pool| == 1)
            self._linear(1 + 4 * i, W[p + 'attn.qkv.weight'], cs_a, s_a0, c[p + 'attn.best_weight_scale'], W[p + 'attn.qkv.bias'], per_bit=True)
            if self.int_softmax:
                x0, bb, cc = lis_consts(s_at)
            else:      # the table softmax reads none of them (any valid triple passes the block's checks)
                x0, bb, cc = -1, 0, 1
                fblk.softmax_table = E.ptr(self._dev(torch.from_numpy(softmax_table(s_at).astype(np.int32)), torch.int32))
            blk.attn = E.Attn(float(s_q1 * s_q1), float(np.float32(hd ** -0.5)), float(1.0 / s_at), float(s_q1 / s_a2), x0, bb, cc)
            self._linear(2 + 4 * i, W[p + 'attn.proj.weight'], None, s_a2, c[p + 'attn.proj'], W[p + 'attn.proj.bias'])
            pe = E.Epilogue()
            pe.s_mid = E.ptr(self._dev(_per_channel(c[p + 'attn.qact3'], D)))
            pe.s_res = E.ptr(self._dev(s_res))
            pe.s_next = E.ptr(self._dev(s_b2))
            blk.proj_epi = pe
            self._linear(3 + 4 * i, W[p + 'mlp.fc1.weight'], cs_m, s_m0, c[p + 'mlp.best_weight_scale'], W[p + 'mlp.fc1.bias'], per_bit=True)
            blk.inv_s_fc1 = float(1.0 / s_m1)
            blk.gelu_fc1 = E.gelu_table(float(1.0 / s_m1), self.device)      # exact GELU -> qact1 threshold table (cached per scale)
            self._linear(4 + 4 * i, W[p + 'mlp.fc2.weight'], None, s_m1, c[p + 'mlp.fc2'], W[p + 'mlp.fc2.bias'])
            fe = E.Epilogue()
            fe.s_mid = E.ptr(self._dev(_per_channel(c[p + 'mlp.qact2'], D)))
            fe.s_res = E.ptr(self._dev(s_b2))
            fe.s_next = E.ptr(self._dev(s_b4))
            blk.fc2_epi = fe
            if self.int_softmax and self.softmax_bits[i] != 4:
                if not hasattr(L, 'p2v_plan_set_softmax_bits'):
                    raise RuntimeError('libp2vit_hip.so lacks p2v_plan_set_softmax_bits (a %d-bit log-int-softmax): rebuild' % self.softmax_bits[i])
                E.check(L.p2v_plan_set_softmax_bits(self._handle, i, self.softmax_bits[i]))
            E.check(L.p2v_plan_set_block(self._handle, i, C.byref(blk)))
            if not (self.int_norm and self.int_softmax):
                E.check(L.p2v_plan_set_float_block(self._handle, i, C.byref(fblk)))
            if L.p2v_plan_block_prefolded(self._handle, i) != 1:        # same results either way: the kernels then fold per workgroup
                warnings.warn('block %d: LayerNorm constants not folded at plan time: %s' % (i, (L.p2v_last_error() or b'').decode()))
            s_res = s_b4
        # ---- head ------------------------------------------------------------------------------
        s_f = _need_pot('qact2', c['qact2'])
        s_o = _need_pot('act_out', c['act_out'])
        self.stage_scales['qact2'] = float(s_f)
        fl = self._ln(s_res, W['norm.weight'], W['norm.bias'], s_f, s_f / s_f)
        E.check(L.p2v_plan_set_head(self._handle, C.byref(fl), float(1.0 / s_o), float(s_o)))
        if not self.int_norm:
            ff = self._fln(s_res, W['norm.weight'], W['norm.bias'], 1.0 / s_f)
            E.check(L.p2v_plan_set_float_head(self._handle, C.byref(ff)))
        self._linear(self.n_layers - 1, W['head.weight'], None, s_f, c['head'], W['head.bias'])
        self.s_out = float(s_o)

    # ---------------------------------------------------------------------------------------------
    def workspace(self, batch, min_bytes=0):
        """the plan's grow-only workspace: enough for a forward of ``batch`` images, and at least ``min_bytes``"""
        if self._ws is None or self._ws_batch < batch or self._ws.numel() < min_bytes:
            self._ws_batch = max(self._ws_batch, batch)
            n = max(E.lib().p2v_workspace_bytes(self._handle, self._ws_batch), min_bytes)
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._ws

    def _check_here(self, images):
        """a device pointer on THIS plan's GPU, and something to run"""
        if not images.is_cuda:
            raise RuntimeError('the quantized forward runs on the HIP engine only: move the input to the GPU')
        if images.device != self.device:
            raise RuntimeError('images live on %s, the frozen plan on %s' % (images.device, self.device))
        if images.shape[0] < 1:
            raise AssertionError('empty batch')

    @staticmethod
    def _cfg(bit_config):
        """``bit_config`` as the int8 array of the C ABI (an entry that does not fit a byte becomes 127, which the library refuses)"""
        if bit_config is None:
            raise ValueError('None is not in list')        # bit_pool.index(None), vit_fquant.py:282
        return (C.c_int8 * len(bit_config))(*[int(b) if -128 <= int(b) <= 127 else 127 for b in bit_config])

    def _check(self, images, bit_config):
        """the reference's input checks (layers_quant.py:437-439, vit_fquant.py:282) plus what the C ABI trusts: the geometry in
        the plan descriptor, a device pointer on THIS plan's GPU.  Shared by every entry point that takes fp32 images
        (a wrong-sized or foreign tensor would otherwise be an out-of-bounds read in ``k_quantize_patchify``)."""
        a = self.arch
        if images.dim() != 4 or images.shape[2] != a['img_size'] or images.shape[3] != a['img_size']:
            raise AssertionError("Input image size (%d*%d) doesn't match model (%d*%d)." % (
                images.shape[2] if images.dim() > 2 else -1, images.shape[3] if images.dim() > 3 else -1, a['img_size'], a['img_size']))
        if images.shape[1] != self.in_chans:
            raise AssertionError('expected %d input channels' % self.in_chans)
        self._check_here(images)
        return images.contiguous().float(), self._cfg(bit_config)

    def _check_out(self, out, B):
        # the C ABI writes B x classes floats through the raw pointer
        if tuple(out.shape) != (B, self.arch['num_classes']) or out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous():
            raise AssertionError('out must be a contiguous fp32 [%d, %d] tensor on %s' % (B, self.arch['num_classes'], self.device))

    def _out(self, out, B):
        """the logits of B images: the caller's ``out``, checked, or a new tensor"""
        if out is None:
            return torch.empty(B, self.arch['num_classes'], dtype=torch.float32, device=self.device)
        self._check_out(out, B)
        return out

    def input_lut(self, lut_f32):
        """the device table ``forward_uint8`` reads for the fp32 table ``lut_f32`` [C, 256] (data.uint8_lut): its codes under this plan's
        input scale (int8, data.uint8_lut_i8), or the fp32 values themselves for a plan without an input QAct (input_quant=False)."""
        from .data import uint8_lut_i8
        lut_f32 = lut_f32.detach().float().cpu()
        t = uint8_lut_i8(lut_f32, self.inv_s_input) if self.input_quant else lut_f32
        return t.contiguous().to(self.device)

    def _check_u8(self, images, lut, bit_config, layout):
        """``_check`` for uint8 images in ``layout`` ('NHWC' [B, H, W, C] or 'NCHW' [B, C, H, W]) and the device table of ``input_lut``:
        the C ABI trusts the geometry, the table's size and type, and the device, so every one is checked here (same exception classes)."""
        a, S, Cin = self.arch, self.arch['img_size'], self.in_chans
        if layout not in E.LAYOUTS:
            raise AssertionError("layout must be 'NHWC' or 'NCHW', got %r" % (layout,))
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
            raise AssertionError('forward_uint8 takes uint8 images, got %s (fp32 images go to forward)' % getattr(images, 'dtype', type(images)))
        want = (S, S, Cin) if layout == 'NHWC' else (Cin, S, S)
        if images.dim() != 4 or tuple(images.shape[1:]) != want:
            raise AssertionError('uint8 images in layout %s must be [B, %d, %d, %d], got %s' % ((layout,) + want + (tuple(images.shape),)))
        self._check_here(images)
        lut_dtype = torch.int8 if self.input_quant else torch.float32
        if (not isinstance(lut, torch.Tensor) or lut.dtype != lut_dtype or tuple(lut.shape) != (Cin, 256) or lut.device != self.device
                or not lut.is_contiguous()):
            raise AssertionError('lut must be a contiguous %s [%d, 256] tensor on %s (FrozenPlan.input_lut)' % (lut_dtype, Cin, self.device))
        return images.contiguous(), self._cfg(bit_config)

    def forward_uint8(self, images, lut, bit_config, layout='NHWC', out=None, stop_after=-1):
        """``forward`` on uint8 images: p2v_forward_u8 reads them through ``lut`` (``input_lut``) in its first launch; the logits equal
        ``forward`` on the fp32 images ``data.normalize_uint8`` makes of them, bit for bit (so does the patch matrix after stop_after=1)."""
        images, cfg = self._check_u8(images, lut, bit_config, layout)
        B = images.shape[0]
        with torch.cuda.device(self.device):
            ws, out = self.workspace(B), self._out(out, B)
            E.check(E.lib().p2v_forward_u8(self._handle, E.ptr(images), E.LAYOUTS[layout], E.ptr(lut), B, cfg, len(bit_config), E.ptr(out),
                                           E.ptr(ws), ws.numel(), stop_after, E.stream_ptr(self.device)))
        return out

    def forward_uint8_streams(self, images, lut, bit_config, out, layout='NHWC', n_streams=3, slices=None):
        """``forward_streams`` on uint8 images: the same slices (contiguous in the batch dimension in both layouts), each one
        p2v_forward_u8 call."""
        images, cfg = self._check_u8(images, lut, bit_config, layout)
        L, handle, n_cfg, lay, lp = E.lib(), self._handle, len(bit_config), E.LAYOUTS[layout], E.ptr(lut)
        return self._run_slices(images, out, n_streams, slices, lambda: self.forward_uint8(images, lut, bit_config, layout, out=out),
                                lambda xi, n_i, oi, ws, ws_n, st: L.p2v_forward_u8(handle, xi, lay, lp, n_i, cfg, n_cfg, oi, ws, ws_n, -1, st))

    def forward(self, images, bit_config, stop_after=-1, out=None, taps=None):
        """images: fp32 [B,C,H,W] on the plan's device -> fp32 logits [B, classes] (int8 grid * act_out scale).
        ``taps`` (dict): filled with 'qkv_output' / 'fc1_output' -> list of fp32 [B, tokens, 3D] / [B, tokens, hidden] tensors per
        block, the layer outputs before qact1 / GELU that the reference keeps for its analysis scripts (vit_fquant.py:301,
        layers_quant.py:326); written by the GEMM epilogues of the same launches."""
        images, cfg = self._check(images, bit_config)
        B = images.shape[0]
        with torch.cuda.device(self.device):
            ws, out = self.workspace(B), self._out(out, B)
            if taps is None:
                E.check(E.lib().p2v_forward(self._handle, E.ptr(images), B, cfg, len(bit_config), E.ptr(out), E.ptr(ws),
                                            ws.numel(), stop_after, E.stream_ptr(self.device)))
            else:
                qkv = [torch.empty(B, self.tokens, 3 * self.D, dtype=torch.float32, device=self.device) for _ in range(self.depth)]
                fc1 = [torch.empty(B, self.tokens, self.hidden, dtype=torch.float32, device=self.device) for _ in range(self.depth)]
                pq = (C.c_void_p * self.depth)(*[t.data_ptr() for t in qkv])
                pf = (C.c_void_p * self.depth)(*[t.data_ptr() for t in fc1])
                E.check(E.lib().p2v_forward_taps(self._handle, E.ptr(images), B, cfg, len(bit_config), E.ptr(out), E.ptr(ws), ws.numel(),
                                                 pq, pf, E.stream_ptr(self.device)))
                taps['qkv_output'], taps['fc1_output'] = qkv, fc1
        return out

    def tap_shapes(self, batch):
        """shapes of the ``forward_linear_taps`` buffers, in bit_config order: the patch-embed output channels last [B*patches, D],
        qkv / proj / fc1 / fc2 of each block [B, tokens, width], the head [B, classes]."""
        T, D = self.tokens, self.D
        blk = [(batch, T, 3 * D), (batch, T, D), (batch, T, self.hidden), (batch, T, D)]
        return [(batch * self.patches, D)] + blk * self.depth + [(batch, self.arch['num_classes'])]

    def forward_linear_taps(self, images, bit_config, want=None, out=None):
        """p2v_forward_linear_taps: logits plus the output of every linear layer (what cka_utility.py:26-113 hooks on QConv2d /
        QLinear).  Returns (logits, taps): taps[k] for bit_config index k is an fp32 tensor of ``tap_shapes`` (the patch-embed tap as
        the [B, D, H/P, W/P] view of the reference's QConv2d output), or None where ``want`` (indices) leaves it out."""
        images, cfg = self._check(images, bit_config)
        B = images.shape[0]
        shapes = self.tap_shapes(B)
        want = set(range(len(shapes))) if want is None else set(want)
        with torch.cuda.device(self.device):
            ws, out = self.workspace(B), self._out(out, B)
            bufs = [torch.empty(s, dtype=torch.float32, device=self.device) if k in want else None for k, s in enumerate(shapes)]
            ptrs = (C.c_void_p * len(bufs))(*[None if t is None else t.data_ptr() for t in bufs])
            E.check(E.lib().p2v_forward_linear_taps(self._handle, E.ptr(images), B, cfg, len(bit_config), E.ptr(out), E.ptr(ws),
                                                    ws.numel(), ptrs, E.stream_ptr(self.device)))
        g = self.arch['img_size'] // self.arch['patch_size']
        if bufs[0] is not None:
            bufs[0] = bufs[0].view(B, g, g, self.D).permute(0, 3, 1, 2)
        return out, bufs

    def ddv_stage_names(self, with_linear=False, stages='engine', attention=False):
        """names of the ``forward_ddv`` stages in module order (``ddv.stage_names``: the oracle's tap names, plus the QLinear outputs)."""
        from .ddv import stage_names
        if stages not in ('engine', 'full'):
            raise ValueError("forward_ddv: stages must be 'engine' or 'full', not %r" % (stages,))
        return stage_names(self.depth, with_linear, stages == 'full', attention)

    def ddv_attn_bytes(self, n):
        """bytes of the scratch ``forward_ddv(attention=True)`` needs for n pairs: the score-code and the exponent plane of ONE block's
        attention over the 2n images, rows pitched to whole 16-byte groups (2 * 2n * heads * tokens * round_up(tokens, 16))."""
        return int(E.lib().p2v_ddv_attn_scratch_bytes(self._handle, n))

    def ddv_tap_bytes(self, n):
        """bytes of the one fp32 buffer ``forward_ddv(with_linear=True)`` needs for n pairs: the largest single tap of 2n images."""
        return int(E.lib().p2v_ddv_tap_scratch_bytes(self._handle, n))

    def forward_ddv(self, images_2n, bit_config, with_linear=False, stages='engine', attention=False):
        """p2v_forward_ddv: ``images_2n`` holds n clean images followed by their n perturbed twins.  Returns (logits [2n, classes],
        stage names, sums): sums is fp64 [stages, n, 3] = (sum a.b, sum a.a, sum b.b) of every stage's activation on image i and on
        image n + i, reduced from the int8 codes between the launches of the ONE forward (``ddv.ddv_from_sums`` turns them into a
        DDV).  The only fp32 activation memory is one tap of 2n images (``ddv_tap_bytes``), and only with ``with_linear``.
        ``stages='full'`` (``P2V_DDV_STAGES_FULL``): also the stages behind the reference's remaining hook points - the stem's codes, the
        LayerNorm values, the mid codes of proj / fc2 - in the same one call; the tap buffer is then needed either way.
        ``attention`` (``P2V_DDV_STAGES_ATTN``, with either set): per block also ``attn.qact_attn1`` (the score codes) and
        ``attn.log_int_softmax`` (the log2 probabilities at the block's softmax width), both exact, from the tapped attention launch through one scratch of
        ``ddv_attn_bytes(n)`` that the next block reuses."""
        images, cfg = self._check(images_2n, bit_config)
        B = images.shape[0]
        if B % 2:
            raise AssertionError('forward_ddv takes n clean images followed by their n perturbed twins: %d images' % B)
        n = B // 2
        L = E.lib()
        names = self.ddv_stage_names(with_linear, stages, attention)
        if attention and not self.int_softmax:
            raise NotImplementedError('forward_ddv(attention=True): the softmax of a lis=False plan is the float one, its probabilities are not codes')
        full = stages == 'full'
        if full and not self.input_quant:
            raise NotImplementedError("forward_ddv(stages='full'): no qact_input stage on an input_quant=False plan")
        # one entry point for every stage set: without P2V_DDV_STAGES_ATTN p2v_forward_ddv_ex2 is p2v_forward_ddv(_ex), and the forward's
        # workspace does not depend on the stage set
        stage_set = (E.DDV_STAGES_FULL if full else E.DDV_STAGES_ENGINE) | (E.DDV_STAGES_ATTN if attention else 0)
        assert len(names) == L.p2v_ddv_stage_count_ex2(self._handle, int(with_linear), stage_set)
        with torch.cuda.device(self.device):
            ws = self.workspace(B, L.p2v_ddv_workspace_bytes(self._handle, n))
            out = self._out(None, B)
            sums = torch.empty(len(names), n, 3, dtype=torch.float64, device=self.device)
            tap = torch.empty(self.ddv_tap_bytes(n), dtype=torch.uint8, device=self.device) if (with_linear or full) else None
            att = torch.empty(self.ddv_attn_bytes(n), dtype=torch.uint8, device=self.device) if attention else None
            E.check(L.p2v_forward_ddv_ex2(self._handle, E.ptr(images), n, cfg, len(bit_config), E.ptr(out), E.ptr(ws), ws.numel(), int(with_linear),
                                          stage_set, E.ptr(tap), 0 if tap is None else tap.numel(), E.ptr(att), 0 if att is None else att.numel(),
                                          E.ptr(sums), E.stream_ptr(self.device)))
        return out, names, sums

    def forward_stats(self, images, bit_config=None, with_linear=False, stages='engine', attention=False, into=None):
        """p2v_forward_stats: the logits of ``images`` (any batch >= 1) and the ``stats.StageStats`` of every ``forward_ddv`` stage
        (``ddv_stage_names``), each reduced over all images and tokens by ONE launch right behind the launch that completes the stage:
        per channel the lowest and highest code, the integer sums, and the histogram of the codes (fp32 stages: of the exponent field).
        ``into``: a result of an earlier call with the same arguments - the batch is accumulated into its records on the device, without
        a host synchronisation, and it is returned.  Stage sets and refusals are ``forward_ddv``'s."""
        from .stats import StageStats
        images, cfg = self._check(images, bit_config)
        B = images.shape[0]
        L = E.lib()
        names = self.ddv_stage_names(with_linear, stages, attention)
        if attention and not self.int_softmax:
            raise NotImplementedError('forward_stats(attention=True): the softmax of a lis=False plan is the float one, its probabilities are not codes')
        full = stages == 'full'
        if full and not self.input_quant:
            raise NotImplementedError("forward_stats(stages='full'): no qact_input stage on an input_quant=False plan")
        stage_set = (E.DDV_STAGES_FULL if full else E.DDV_STAGES_ENGINE) | (E.DDV_STAGES_ATTN if attention else 0)
        key = ('plan', self.handle, bool(with_linear), stage_set)
        n = (B + 1) // 2
        with torch.cuda.device(self.device):
            if into is None:
                K = len(names)
                off, cols, kinds, scales = (C.c_longlong * K)(), (C.c_int32 * K)(), (C.c_int32 * K)(), (C.c_void_p * K)()
                got = L.p2v_forward_stats_layout(self._handle, int(with_linear), stage_set, K, off, cols, kinds, scales)
                if got < 0:
                    E.check(got)
                assert got == K, (got, K)
                by_ptr = {t.data_ptr(): t for t in self._keep}
                sc = [by_ptr[scales[k]][:cols[k]] if scales[k] else self.stage_scales.get(names[k]) for k in range(K)]
                into = StageStats.empty(names, list(cols), list(kinds), sc, self.device, offsets=list(off),
                                        nbytes=int(L.p2v_forward_stats_bytes(self._handle, int(with_linear), stage_set)), key=key)
            elif into.key != key or into.names != names:
                raise AssertionError('forward_stats(into=...): the result was made by another plan or with other stages')
            ws, out = self.workspace(B), self._out(None, B)
            tap = torch.empty(self.ddv_tap_bytes(n), dtype=torch.uint8, device=self.device) if (with_linear or full) else None
            att = torch.empty(self.ddv_attn_bytes(n), dtype=torch.uint8, device=self.device) if attention else None
            E.check(L.p2v_forward_stats(self._handle, E.ptr(images), B, cfg, len(bit_config), E.ptr(out), E.ptr(ws), ws.numel(), int(with_linear),
                                        stage_set, E.ptr(tap), 0 if tap is None else tap.numel(), E.ptr(att), 0 if att is None else att.numel(),
                                        E.ptr(into.arena), into.arena.numel(), E.stream_ptr(self.device)))
        return out, into

    def forward_grams(self, images, bit_config, with_linear=False, stages='engine'):
        """p2v_forward_grams: the logits of ``images`` (1 ... 512 images) and the raw Gram of every ``forward_ddv`` stage over the
        batch, taken from the live codes right behind the launch that completes the stage.  Returns (logits, names, grams, units):
        names = ``ddv_stage_names(with_linear, stages)``, grams fp64 [stages, B, B] - the exact integer sums of the stage values
        code * 2^m_c for the int8 stages, the fp32 Gram with a zero diagonal for the fp32 ones - and units fp64 [stages], the value of
        one integer step (values = integers * unit; CKA does not depend on it).  ``ops.cka_centre`` turns the Grams into the centred
        ones of ``cka._grams``.  Stage sets and refusals are ``forward_ddv``'s; the attention stages are not served."""
        images, cfg = self._check(images, bit_config)
        B = images.shape[0]
        L = E.lib()
        names = self.ddv_stage_names(with_linear, stages, False)
        full = stages == 'full'
        if full and not self.input_quant:
            raise NotImplementedError("forward_grams(stages='full'): no qact_input stage on an input_quant=False plan")
        stage_set = E.DDV_STAGES_FULL if full else E.DDV_STAGES_ENGINE
        n = (B + 1) // 2
        with torch.cuda.device(self.device):
            if not getattr(self, '_grams_ready', False):       # once per plan: the exponent bytes and units of the per-channel scale vectors
                if torch.cuda.is_current_stream_capturing():   # (a plan-time call: it synchronises the device and reads the scales back)
                    raise RuntimeError('forward_grams: the stream is capturing a graph, and neither p2v_plan_prepare_grams nor '
                                       'p2v_forward_grams can be captured: call forward_grams outside the capture')
                E.check(L.p2v_plan_prepare_grams(self._handle))
                self._grams_ready = True
            K = len(names)
            assert K == L.p2v_forward_grams_stage_count(self._handle, int(with_linear), stage_set)
            need = int(L.p2v_forward_grams_bytes(self._handle, B, int(with_linear), stage_set))
            if need == 0:
                E.check(L.p2v_forward_grams(self._handle, None, B, cfg, len(bit_config), None, None, 0, int(with_linear), stage_set, None, 0,
                                            None, 0, None, 0, None))     # raises with the validation message
            ws, out = self.workspace(B, need), self._out(None, B)
            grams = torch.empty(K, B, B, dtype=torch.float64, device=self.device)
            units = torch.empty(K, dtype=torch.float64, device=self.device)
            tap = torch.empty(self.ddv_tap_bytes(n), dtype=torch.uint8, device=self.device) if (with_linear or full) else None
            E.check(L.p2v_forward_grams(self._handle, E.ptr(images), B, cfg, len(bit_config), E.ptr(out), E.ptr(ws), ws.numel(), int(with_linear),
                                        stage_set, E.ptr(tap), 0 if tap is None else tap.numel(), E.ptr(grams), grams.numel() * 8, E.ptr(units),
                                        units.numel() * 8, E.stream_ptr(self.device)))
            # a one-scale stage's unit is the scale the plan was frozen with (the stage sites of the C layer do not carry it)
            one = [k for k, nm in enumerate(names) if nm in self.stage_scales]
            kinds = (C.c_int32 * K)()
            scales = (C.c_void_p * K)()
            L.p2v_forward_grams_layout(self._handle, int(with_linear), stage_set, K, None, None, kinds, scales)
            one = [k for k in one if kinds[k] == E.GRAM_I8 and not scales[k]]
            if one:
                units[torch.tensor(one, device=self.device)] = torch.tensor([self.stage_scales[names[k]] for k in one], dtype=torch.float64,
                                                                            device=self.device)
        return out, names, grams, units

    def slice_sizes(self, batch, n_streams=3):
        """Batch slices of ``forward_streams`` for up to ``n_streams`` side streams plus the caller's own stream (256 -> 68 + 68 + 68 + 52).
        Four kernels in flight on four hardware queues is what the device sustains - a fourth SIDE stream (five streams with the caller's)
        collapses to 57 k img/s, see ``engine.side_streams`` - and the caller's stream carries ~0.77 of a side slice.

        How many slices pays depends on the work per slice (profiles/r04_sweep_slices.txt, same-call sweeps over widths 192 / 384 / 768,
        197 / 577 tokens and batches of 16 ... 512): for the models whose blocks run the fused LayerNorm+GEMM kernels (widths up to 384) one
        slice per ~8 k rows (batch x tokens) at width 384 - proportionally more rows for narrower models - and at least 32 images per slice
        (the attention launch has images x heads workgroups): DeiT-S 32 images -> one slice, 64 -> two (+4 %), 128 -> three (+15 %),
        192 and more -> four (+20 %); 64 images at 577 tokens -> two (+29 %).  The MFMA-bound wide models gain from exactly TWO balanced slices
        on side streams (ViT-B b512 36.1 k img/s against 35.2 k on one stream and 35.8 k on three; DeiT-B W4 40.1 / 38.2 / 39.1 k)."""
        if n_streams <= 1 or batch < 2:
            return [batch]
        if self.D > 384:
            if batch < 64:
                return [batch]
            return [(batch + 1) // 2, batch // 2]
        target = 8192 * 384 // self.D                                   # rows (batch x tokens) per slice
        k = min((2 * batch * self.tokens + target) // (2 * target), batch // 32, n_streams + 1)
        if k <= 1:
            return [batch]
        d = 1000 * (k - 1) + 765                                        # the caller's slice is ~0.77 of a side slice (52 : 68)
        side = (batch * 1000 + d - 1) // d
        return [side] * (k - 1) + [batch - (k - 1) * side]

    def forward_streams(self, images, bit_config, out, n_streams=3, slices=None):
        """Same result as ``forward``; the batch is cut into contiguous slices (``slice_sizes`` or an explicit list) that run on
        their own workspaces, round robin over ``n_streams`` side HIP streams and the caller's own stream (the slice after the side streams' runs there).  Images are
        independent, so this is only a scheduling choice: kernels of one slice (e.g. a VALU-bound GELU epilogue) overlap latency-
        or MFMA-bound phases of another slice's kernels."""
        images, cfg = self._check(images, bit_config)
        L, handle, n_cfg = E.lib(), self._handle, len(bit_config)
        return self._run_slices(images, out, n_streams, slices, lambda: self.forward(images, bit_config, out=out),
                                lambda xi, n_i, oi, ws, ws_n, st: L.p2v_forward(handle, xi, n_i, cfg, n_cfg, oi, ws, ws_n, -1, st))

    def _cfgs(self, bit_configs):
        """``bit_configs`` (a sequence of bit lists of this plan's length) as the host array [n_lists][n_cfg] of p2v_forward_many"""
        lists = [list(bc) if bc is not None else None for bc in bit_configs]
        if not lists:
            raise AssertionError('forward_many needs at least one bit list')
        if any(bc is None for bc in lists):
            raise ValueError('None is not in list')        # bit_pool.index(None), vit_fquant.py:282
        if any(len(bc) != self.n_layers for bc in lists):
            raise ValueError('bit lists of %r entries, model needs %d' % (sorted({len(bc) for bc in lists}), self.n_layers))
        return self._cfg([b for bc in lists for b in bc]), len(lists)

    def forward_many_plan(self, bit_configs):
        """what ``forward_many`` runs for these lists, counted without a launch (p2v_forward_many_plan): stem runs, block runs, final norms,
        head GEMMs, copies of the residual stream (saves + restores) and snapshot slots.  A loop of ``forward`` runs ``len(bit_configs)``
        stems, norms and heads and ``len(bit_configs) * depth`` blocks."""
        cfgs, n_lists = self._cfgs(bit_configs)
        names = ('stems', 'blocks', 'norms', 'heads', 'copies', 'snapshots')
        vals = [C.c_int() for _ in names]
        E.check(E.lib().p2v_forward_many_plan(self._handle, cfgs, n_lists, self.n_layers, *[C.byref(v) for v in vals]))
        return {k: v.value for k, v in zip(names, vals)}

    def _forward_many(self, images, cfgs, n_lists, n_streams, slices, call):
        """the body of ``forward_many`` / ``forward_many_uint8`` behind their input checks; ``call(images_ptr, n, out_ptr, ws_ptr, ws_bytes,
        stream_ptr)`` is the entry point on a batch or a slice of it.  Every slice runs the whole tree of lists on its own stream and
        workspace into a [n_lists, n, classes] tensor of its own, which is copied into its columns of the result once the streams have joined."""
        L, B, nc = E.lib(), images.shape[0], self.arch['num_classes']
        ws_bytes = lambda n: L.p2v_forward_many_bytes(self._handle, n, cfgs, n_lists, self.n_layers)
        with torch.cuda.device(self.device):
            out = torch.empty(n_lists, B, nc, dtype=torch.float32, device=self.device)
            parts = {}

            def whole():
                ws = self.workspace(B, ws_bytes(B))
                E.check(call(E.ptr(images), B, E.ptr(out), E.ptr(ws), ws.numel(), E.stream_ptr(self.device)))

            def part(lo, hi):
                parts[lo, hi] = torch.empty(n_lists, hi - lo, nc, dtype=torch.float32, device=self.device)
                return parts[lo, hi]
            self._run_slices(images, out, n_streams, slices, whole, call, ws_bytes, part)
            for (lo, hi), t in parts.items():
                out[:, lo:hi].copy_(t)
        return out

    def forward_many(self, images, bit_configs, n_streams=1, slices=None):
        """``forward`` under every list of ``bit_configs`` in one call: fp32 [n_lists, B, classes], row l byte-equal to ``forward(images,
        bit_configs[l])``.  The lists share what they have in common (p2v_forward_many): a prefix tree over (stem entry, the four entries of
        block 0, 1, ...), every node run once, the residual stream saved where the tree branches.  ``n_streams`` / ``slices`` cut the batch
        as ``forward_streams`` does."""
        cfgs, n_lists = self._cfgs(bit_configs)
        images, _ = self._check(images, bit_configs[0])
        L, handle, n_cfg = E.lib(), self._handle, self.n_layers
        return self._forward_many(images, cfgs, n_lists, n_streams, slices,
                                  lambda xi, n_i, oi, ws, ws_n, st: L.p2v_forward_many(handle, xi, n_i, cfgs, n_lists, n_cfg, oi, ws, ws_n, st))

    def forward_many_uint8(self, images, lut, bit_configs, layout='NHWC', n_streams=1, slices=None):
        """``forward_many`` on uint8 images read through ``lut`` (``input_lut``): row l is byte-equal to ``forward_uint8(images, lut,
        bit_configs[l], layout)``."""
        cfgs, n_lists = self._cfgs(bit_configs)
        images, _ = self._check_u8(images, lut, bit_configs[0], layout)
        L, handle, n_cfg, lay, lp = E.lib(), self._handle, self.n_layers, E.LAYOUTS[layout], E.ptr(lut)
        return self._forward_many(images, cfgs, n_lists, n_streams, slices,
                                  lambda xi, n_i, oi, ws, ws_n, st: L.p2v_forward_many_u8(handle, xi, lay, lp, n_i, cfgs, n_lists, n_cfg, oi, ws, ws_n, st))

    @staticmethod
    def slice_streams(n_slices, n_side):
        """the stream of every slice: round robin over the ``n_side`` side streams and, as index ``n_side``, the caller's stream"""
        return [i % (n_side + 1) for i in range(n_slices)]

    def _slices(self, sizes, n_streams, ws_bytes=None):
        """what a sliced run needs, for ``_run_slices`` and ``profile_streams``: the borrowed side streams (the process's shared ones of this
        device, never new ones) and per slice (lo, hi, stream index of ``slice_streams``, its own grow-only workspace of ``ws_bytes(n)``
        bytes for its n images; default: p2v_workspace_bytes)"""
        n_side = min(len(sizes), max(n_streams, 1))
        self._streams = E.side_streams(self.device, n_side)
        self._ws_multi += [None] * (len(sizes) - len(self._ws_multi))
        L, rows, hi = E.lib(), [], 0
        for i, (n_i, j) in enumerate(zip(sizes, self.slice_streams(len(sizes), n_side))):
            n = ws_bytes(n_i) if ws_bytes else L.p2v_workspace_bytes(self._handle, n_i)
            if self._ws_multi[i] is None or self._ws_multi[i].numel() < n:
                self._ws_multi[i] = torch.empty(n, dtype=torch.uint8, device=self.device)
            rows.append((hi, hi + n_i, j, self._ws_multi[i]))
            hi += n_i
        return self._streams, rows

    def _run_slices(self, images, out, n_streams, slices, whole, launch, ws_bytes=None, part=None):
        """the body of ``forward_streams`` / ``forward_uint8_streams`` / ``forward_many`` behind their input checks: ``whole()`` runs a batch
        that stays in one piece, ``launch(images_ptr, n, out_ptr, ws_ptr, ws_bytes, stream_ptr)`` enqueues one slice
        (``engine.run_on_streams``).  ``ws_bytes(n)``: the workspace of a slice of n images when it is not p2v_workspace_bytes;
        ``part(lo, hi)``: what the slice of images lo .. hi writes when that is not ``out[lo:hi]`` (``out`` is then the caller's to check)"""
        B = images.shape[0]
        n_streams = min(n_streams, E.compute_side_streams(self.device))      # (one less while an input pipeline copies on engine.copy_stream)
        sizes = list(slices) if slices is not None else self.slice_sizes(B, n_streams)
        if sum(sizes) != B or min(sizes) < 1:
            raise AssertionError('slices %r do not cover a batch of %d' % (sizes, B))
        if part is None:
            self._check_out(out, B)
            part = lambda lo, hi: out[lo:hi]
        if len(sizes) == 1:
            return whole()
        with torch.cuda.device(self.device):
            side, rows = self._slices(sizes, n_streams, ws_bytes)
            jobs = [[] for _ in range(len(side) + 1)]                 # the calls of every stream, in slice order
            for lo, hi, j, ws in rows:
                args = (E.ptr(images[lo:hi]), hi - lo, E.ptr(part(lo, hi)), E.ptr(ws), ws.numel())
                jobs[j].append(lambda st, args=args: E.check(launch(*args, C.c_void_p(st.cuda_stream))))
            E.run_on_streams(self.device, side, jobs)
        return out

    def _profile_buffers(self):
        n_max = 7 * self.depth + 10
        return (C.c_float * n_max)(), (C.c_int32 * n_max)(), n_max

    @staticmethod
    def _profile_rows(n, ms, kind):
        """[(kind_name, ms), ...] of the ``n`` intervals a profiling call has filled in (or its error)"""
        if n < 0:
            E.check(n)
        return [(E.KERNEL_KINDS[kind[i]], float(ms[i])) for i in range(min(n, len(ms)))]

    def profile(self, images, bit_config):
        """per-launch times (ms, HIP events on the launch stream) of one forward: [(kind_name, ms), ...]; the last entry, 'event_gap', is an
        interval with no launch in it - what the event pair adds to every interval."""
        images, cfg = self._check(images, bit_config)
        B = images.shape[0]
        with torch.cuda.device(self.device):
            ws, out = self.workspace(B), self._out(None, B)
            ms, kind, n_max = self._profile_buffers()
            n = E.lib().p2v_forward_profile(self._handle, E.ptr(images), B, cfg, len(bit_config), E.ptr(out), E.ptr(ws), ws.numel(),
                                            E.stream_ptr(self.device), ms, kind, n_max)
        return self._profile_rows(n, ms, kind)

    def profile_streams(self, images, bit_config, n_streams=3, slices=None, rounds=3):
        """per-launch times UNDER OVERLAP: the slices of ``forward_streams`` run concurrently on their streams, each with HIP events
        between its launches (``p2v_forward_profile_begin`` / ``_end``); ``rounds`` consecutive steps are enqueued back to back so that
        the middle one runs in the steady state.  Returns (per-slice list of [(kind_name, ms), ...] of the middle round, wall ms of it).
        A batch that runs as ONE slice has no overlap: the isolated profile is returned."""
        images, cfg = self._check(images, bit_config)
        B = images.shape[0]
        n_streams = min(n_streams, E.compute_side_streams(self.device))
        sizes = list(slices) if slices is not None else self.slice_sizes(B, n_streams)
        if len(sizes) == 1:
            per = self.profile(images, bit_config)
            return [per], sum(ms for _, ms in per)
        if torch.cuda.is_current_stream_capturing():       # before the warm-up forward and the device synchronisation below
            raise NotImplementedError('profile_streams: the stream is capturing a graph and this call times every launch with events and '
                                      'synchronises the device; make it outside the capture')
        out = self._out(None, B)
        L = E.lib()
        with torch.cuda.device(self.device):
            self.forward_streams(images, bit_config, out, n_streams, sizes)          # (refuses slices that do not cover the batch; warms up)
            torch.cuda.synchronize(self.device)
            side, rows = self._slices(sizes, n_streams)
            streams = side + [torch.cuda.current_stream(self.device)]
            tokens = []
            try:
                for r in range(rounds):
                    row = []
                    tokens.append(row)
                    for lo, hi, j, ws in rows:
                        tok = C.c_void_p()
                        E.check(L.p2v_forward_profile_begin(self._handle, E.ptr(images[lo:hi]), hi - lo, cfg, len(bit_config), E.ptr(out[lo:hi]),
                                                            E.ptr(ws), ws.numel(), C.c_void_p(streams[j].cuda_stream), C.byref(tok)))
                        row.append(tok)
                res = []
                for row in tokens:
                    per = []
                    for j, tok in enumerate(row):
                        ms, kind, n_max = self._profile_buffers()
                        row[j] = None                                                     # ended (also when the call below fails)
                        per.append(self._profile_rows(L.p2v_forward_profile_end(tok, ms, kind, n_max), ms, kind))
                    res.append(per)
            finally:                         # a failed begin / end must not leak the tokens (events + bookkeeping) already handed out
                for row in tokens:
                    for tok in row:
                        if tok is not None:
                            L.p2v_forward_profile_end(tok, None, None, 0)
        mid = res[len(res) // 2]
        return mid, max(sum(ms for _, ms in per) for per in mid)

    def view(self, batch, name, rows, cols):
        """int8 view of a workspace activation buffer (parity tests)."""
        off = E.lib().p2v_workspace_view(self._handle, batch, name.encode())
        if off < 0:
            raise KeyError(name)
        return self._ws[off: off + rows * cols].view(torch.int8).reshape(rows, cols)

    def __del__(self):
        try:
            from . import ops
            ops._PLANS.pop(int(self._handle.value or 0), None)
        except Exception:
            pass
        try:
            if self._handle:
                E.lib().p2v_plan_destroy(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass
