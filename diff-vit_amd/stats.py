"""Stage statistics: which part of its code range every stage of a model uses, per channel, and how much of it sits on the rails - the
question behind the reference's ``forward(x, bit_config, plot=True)`` (models/plot_distrib.py:30-61 draws the per-channel max-of-max and
min-of-min over batch and tokens), answered on the fused engine.

    compute_stats(model, x, bit_config=None, with_linear=True, stages='engine', attention=False, into=None) -> StageStats
    code_stats_cpu(tensors)                  the plain-torch twin of ``torch.ops.p2vit.code_stats``
    StageStats                               ordered stage names, one record per stage, ``merge`` / ``cpu`` and the derived views

The stages are the DDV's (``ddv.stage_names`` / ``ddv.swin_stage_names``).  A stage's RECORD (``p2v_code_stats`` in include/p2vit.h) is
reduced over every image and token, per channel of the last dimension:

    hist[256]     int64: int8 codes at bin code + 128, unsigned bytes (the exponents k of the log2 softmax; 16 ... 255 = probability 0)
                  at the byte, fp32 values (layer outputs, LayerNorm values, logits) at their biased exponent field
    count, nonfinite[3] (NaN, +Inf, -Inf)
    lo[c], hi[c]  the lowest / highest code of channel c (int32); fp32: the value, over the finite elements, -0 < +0; a column without a
                  finite element keeps lo = +Inf, hi = -Inf
    sum[c], sumsq[c]   int64, integer kinds only

Every quantity is an integer or an order-independent extremum: records are exact, bitwise repeatable, and ``merge`` is exact.

On a fused model (``model_quant()`` state on a GPU) ``compute_stats`` makes ONE engine call (``FrozenPlan.forward_stats`` /
``SwinPlan.forward_stats``): one reduction launch right behind the launch that completes a stage, on the live int8 buffer.  Any other state
(a float model, ``-1`` entries, ``model_dequant()``, a CPU model) runs the module graph with forward hooks on the same-named modules, as
``compute_ddv`` does, and reduces the hooked fp32 outputs as F32 (``code_stats_cpu`` on CPU tensors, the op on GPU tensors).  The refusals
are ``compute_ddv``'s: a list ``bit_config`` for a Swin model, ``attention=True`` under ``Config(lis=False)``.

``python -m diff_vit_amd.stats --model deit_small --bits 8 --n 64 [--stages full] [--attention] [--no-ptf] [--no-lis] [--with-linear]``
prints one line per stage on the synthetic data of ``harness`` (range used, share on each rail, used bits, the three widest channels) and
writes ``stats_result/stats.pkl``.  Not covered: statistics on sliced streams, per-token ranges, float sums."""
import argparse
import os
import pickle

import torch

from . import ops
from . import engine as E

KINDS = {E.STAT_I8: 'i8', E.STAT_F32: 'f32', E.STAT_U8: 'u8'}
_HEAD = 2080            # bytes of hist[256], count, nonfinite[3]
_INT_MAX, _INT_MIN = 2 ** 31 - 1, -2 ** 31
_POS_INF, _NEG_INF = 0x7f800000, 0xff800000 - 2 ** 32       # fp32 bits as int32


def _key(bits):
    """fp32 bits (int32 tensor) <-> the int32 key whose signed order is the total order of the values, -0 < +0 (an involution)"""
    return bits ^ ((bits >> 31) & 0x7fffffff)


class StageStats:
    """The records of an ordered list of stages in one byte arena (device or host memory).

    ``names``; per stage ``cols``, ``kinds`` (``engine.STAT_*``) and ``scales`` (None, one float, or a per-channel fp32 tensor: the value
    of a code of channel c is ``code * scale[c]``); ``record(name)`` gives the fields as tensor views of the arena."""

    def __init__(self, names, cols, kinds, scales, arena, offsets, key=None):
        self.names, self.cols, self.kinds, self.scales = list(names), [int(c) for c in cols], [int(k) for k in kinds], list(scales)
        self.arena, self.offsets, self.key = arena, [int(o) for o in offsets], key
        self._index = {nm: k for k, nm in enumerate(self.names)}

    @classmethod
    def empty(cls, names, cols, kinds, scales, device, offsets=None, nbytes=None, key=None):
        """the records of no data at all: zero counts, lo / hi at their neutral elements (``p2v_stats_init`` on a GPU)"""
        device = torch.device(device)
        if offsets is None:
            offsets, o = [], 0
            for c in cols:
                offsets.append(o)
                o += ops.stats_record_bytes(c)
            nbytes = o
        arena = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
        st = cls(names, cols, kinds, scales, arena, offsets, key)
        if device.type == 'cuda':
            L = E.lib()
            with torch.cuda.device(device):
                for k in range(len(st.names)):
                    E.check(L.p2v_stats_init(E.C.c_void_p(arena.data_ptr() + st.offsets[k]), ops.stats_record_bytes(st.cols[k]), st.kinds[k],
                                             st.cols[k], E.stream_ptr(device)))
        else:
            for k in range(len(st.names)):
                r = st._fields(k)
                f32 = st.kinds[k] == E.STAT_F32
                r['lo'].view(torch.int32).fill_(_POS_INF if f32 else _INT_MAX)
                r['hi'].view(torch.int32).fill_(_NEG_INF if f32 else _INT_MIN)
        return st

    def _fields(self, k):
        o, c = self.offsets[k], self.cols[k]
        a = self.arena
        head = a[o:o + _HEAD].view(torch.int64)
        ext = torch.float32 if self.kinds[k] == E.STAT_F32 else torch.int32
        return {'hist': head[:256], 'count': head[256], 'nonfinite': head[257:260],
                'lo': a[o + _HEAD:o + _HEAD + 4 * c].view(ext), 'hi': a[o + _HEAD + 4 * c:o + _HEAD + 8 * c].view(ext),
                'sum': a[o + _HEAD + 8 * c:o + _HEAD + 16 * c].view(torch.int64),
                'sumsq': a[o + _HEAD + 16 * c:o + _HEAD + 24 * c].view(torch.int64)}

    def record(self, name):
        """the fields of stage ``name`` (views of the arena): hist, count, nonfinite, lo, hi, sum, sumsq"""
        return self._fields(self._index[name])

    def kind(self, name):
        return KINDS[self.kinds[self._index[name]]]

    def scale(self, name):
        return self.scales[self._index[name]]

    def __len__(self):
        return len(self.names)

    def cpu(self):
        """the same records in host memory (one copy; synchronises)"""
        sc = [s.cpu() if isinstance(s, torch.Tensor) else s for s in self.scales]
        return StageStats(self.names, self.cols, self.kinds, sc, self.arena.cpu(), self.offsets, self.key)

    def merge(self, other):
        """the records of both data sets together, exact: bins, counts and sums add, extrema combine (fp32 extrema in the total order
        of the values).  Commutative; a new StageStats on this one's device."""
        if self.names != other.names or self.cols != other.cols or self.kinds != other.kinds:
            raise AssertionError('merge: the two results hold different stages')
        out = StageStats(self.names, self.cols, self.kinds, self.scales, self.arena.clone(), self.offsets, self.key)
        if other.arena.device != out.arena.device:
            other = StageStats(other.names, other.cols, other.kinds, other.scales, other.arena.to(out.arena.device), other.offsets, other.key)
        for k in range(len(self.names)):
            a, b = out._fields(k), other._fields(k)
            head = out.arena[out.offsets[k]:out.offsets[k] + _HEAD].view(torch.int64)
            head += other.arena[other.offsets[k]:other.offsets[k] + _HEAD].view(torch.int64)
            a['sum'] += b['sum']
            a['sumsq'] += b['sumsq']
            if self.kinds[k] == E.STAT_F32:
                la, lb = _key(a['lo'].view(torch.int32)), _key(b['lo'].view(torch.int32))
                ha, hb = _key(a['hi'].view(torch.int32)), _key(b['hi'].view(torch.int32))
                a['lo'].view(torch.int32).copy_(_key(torch.minimum(la, lb)))
                a['hi'].view(torch.int32).copy_(_key(torch.maximum(ha, hb)))
            else:
                a['lo'].copy_(torch.minimum(a['lo'], b['lo']))
                a['hi'].copy_(torch.maximum(a['hi'], b['hi']))
        return out

    # ---- derived views -------------------------------------------------------------------------------------------------------------
    def _scale_vec(self, k, like):
        s = self.scales[k]
        if s is None:
            return None
        if isinstance(s, torch.Tensor):
            return s.to(like.device).float().reshape(-1)
        return torch.tensor(float(s), dtype=torch.float32, device=like.device)

    def channel_ranges(self, name):
        """(lo, hi) fp32 [cols]: the two curves of ``plot_distribution`` - per channel the lowest and highest VALUE, fl(lo * s_c) and
        fl(hi * s_c) for codes with a known scale, the codes themselves (as floats) without one, the values of an fp32 stage"""
        k = self._index[name]
        r = self._fields(k)
        if self.kinds[k] == E.STAT_F32:
            return r['lo'].clone(), r['hi'].clone()
        lo, hi = r['lo'].float(), r['hi'].float()
        s = self._scale_vec(k, lo)
        return (lo, hi) if s is None else (lo * s, hi * s)

    def rail_share(self, name):
        """(share of the elements in bin 0, share in bin 255): for int8 codes the shares clamped to -128 and to +127"""
        r = self.record(name)
        n = max(int(r['count']), 1)
        return int(r['hist'][0]) / n, int(r['hist'][255]) / n

    def used_bits(self, name):
        """entropy of the histogram in bits (fp64): 8 = every bin equally used, 0 = one bin"""
        r = self.record(name)
        h = r['hist'].double()
        p = h[h > 0] / h.sum().clamp(min=1)
        return float(-(p * torch.log2(p)).sum())

    def channel_mean_var(self, name, scaled=True):
        """(mean, variance) fp64 [cols] of the integer kinds, from the exact integer sums; ``scaled``: of the values code * s_c where
        the scale is known"""
        k = self._index[name]
        if self.kinds[k] == E.STAT_F32:
            raise NotImplementedError('channel_mean_var: an fp32 stage keeps no sums (a float sum would depend on the order)')
        r = self._fields(k)
        n = max(int(r['count']) // self.cols[k], 1)
        mean = r['sum'].double() / n
        var = r['sumsq'].double() / n - mean * mean
        s = self._scale_vec(k, mean) if scaled else None
        if s is not None:
            mean, var = mean * s.double(), var * s.double() ** 2
        return mean, var


def code_stats_cpu(tensors, names=None, scales=None, into=None):
    """the CPU twin of ``torch.ops.p2vit.code_stats``: a StageStats with one record per tensor [samples, ..., cols] (int8 codes, uint8
    bytes, anything else as fp32), reduced over everything but the last dimension, in int64.  ``into``: accumulate into that result."""
    tensors = [t.detach() for t in tensors]
    kinds = [{torch.int8: E.STAT_I8, torch.uint8: E.STAT_U8}.get(t.dtype, E.STAT_F32) for t in tensors]
    cols = [int(t.shape[-1]) for t in tensors]
    names = list(names) if names is not None else [str(k) for k in range(len(tensors))]
    if into is None:
        into = StageStats.empty(names, cols, kinds, scales if scales is not None else [None] * len(tensors), 'cpu')
    elif into.cols != cols or into.kinds != kinds or into.arena.device.type != 'cpu':
        raise AssertionError('code_stats_cpu(into=...): a CPU result with the same stages is needed')
    for k, t in enumerate(tensors):
        r = into._fields(k)
        x = t.cpu().reshape(-1, cols[k])
        if x.shape[0] == 0:
            continue
        r['count'] += x.numel()
        if kinds[k] == E.STAT_F32:
            bits = x.float().contiguous().view(torch.int32)
            e = (bits >> 23) & 255
            r['hist'] += torch.bincount(e.reshape(-1).long(), minlength=256)
            nan = (e == 255) & ((bits & 0x7fffff) != 0)
            inf = (e == 255) & ((bits & 0x7fffff) == 0)
            r['nonfinite'] += torch.stack([nan.sum(), (inf & (bits >= 0)).sum(), (inf & (bits < 0)).sum()])
            key, fin = _key(bits), e != 255
            lo = torch.where(fin, key, torch.full_like(key, _INT_MAX)).amin(0)
            hi = torch.where(fin, key, torch.full_like(key, _INT_MIN)).amax(0)
            some = fin.any(0)
            lo_old, hi_old = _key(r['lo'].view(torch.int32)), _key(r['hi'].view(torch.int32))
            r['lo'].view(torch.int32).copy_(torch.where(some, _key(torch.minimum(lo, lo_old)), r['lo'].view(torch.int32)))
            r['hi'].view(torch.int32).copy_(torch.where(some, _key(torch.maximum(hi, hi_old)), r['hi'].view(torch.int32)))
        else:
            v = x.long()
            r['hist'] += torch.bincount((v + (128 if kinds[k] == E.STAT_I8 else 0)).reshape(-1), minlength=256)
            r['lo'].copy_(torch.minimum(r['lo'], v.amin(0).int()))
            r['hi'].copy_(torch.maximum(r['hi'], v.amax(0).int()))
            r['sum'] += v.sum(0)
            r['sumsq'] += (v * v).sum(0)
    return into


def code_stats(tensors, names=None, scales=None, into=None):
    """``code_stats_cpu`` for GPU tensors through ``p2v_code_stats`` (the reduction of ``torch.ops.p2vit.code_stats``): a StageStats on
    the tensors' device; ``into`` accumulates without a host synchronisation."""
    kinds = [{torch.int8: E.STAT_I8, torch.uint8: E.STAT_U8}.get(t.dtype, E.STAT_F32) for t in tensors]
    cols = [int(t.shape[-1]) for t in tensors]
    names = list(names) if names is not None else [str(k) for k in range(len(tensors))]
    if into is None:
        into = StageStats.empty(names, cols, kinds, scales if scales is not None else [None] * len(tensors), tensors[0].device)
    elif into.cols != cols or into.kinds != kinds or into.arena.device != tensors[0].device:
        raise AssertionError('code_stats(into=...): a result with the same stages on %s is needed' % (tensors[0].device,))
    recs = [into.arena[into.offsets[k]:into.offsets[k] + ops.stats_record_bytes(cols[k])] for k in range(len(tensors))]
    ops._code_stats([t.detach() for t in tensors], recs)
    return into


def _compute_stats_swin(model, x, bit_config, with_linear, attention, into):
    from . import ddv
    if isinstance(bit_config, (list, tuple)):
        raise NotImplementedError('compute_stats: a Swin model has one weight width and no per-layer bit_config list '
                                  '(swin_quant.py:813-817); pass 8, 4 or None')
    if attention and bit_config is not None and not model.cfg.INT_SOFTMAX:
        raise NotImplementedError('compute_stats(attention=True): under Config(lis=False) the quantized softmax is the float one, its '
                                  'probabilities are not codes')
    dev = ddv._device_of(model)
    x = x.to(dev).float()
    quant_state = model.quant and all(m.quant and not m.calibrate for m in model._q_modules())
    if bit_config is not None and quant_state and dev.type == 'cuda':
        if int(bit_config) not in (4, 8):
            raise ValueError('%r is not in list' % (bit_config,))
        if model._plan is None or model._plan.bits != int(bit_config):
            model.freeze(dev, bits=int(bit_config))
        return model._plan.forward_stats(x, with_linear, attention=attention, into=into)[1]
    names = ddv.swin_stage_names(model.arch['depths'], with_linear, attention)
    mods = dict(model.named_modules())
    got, hooks = {}, []
    for nm in names:
        hooks.append(mods[nm].register_forward_hook(lambda m, i, o, nm=nm: got.__setitem__(nm, o.detach())))
    try:
        with torch.no_grad():
            model.act_out(model.head(model.forward_features(x)))
    finally:
        for h in hooks:
            h.remove()
    outs = [got[nm].float() if got[nm].dim() > 1 else got[nm].float().reshape(1, -1) for nm in names]
    return (code_stats if dev.type == 'cuda' else code_stats_cpu)(outs, names, into=into)


def compute_stats(model, x, bit_config=None, with_linear=True, stages='engine', attention=False, into=None):
    """the StageStats of ``model`` under ``bit_config`` on the images ``x`` [n, C, H, W] (module docstring).  ``into``: a result of an
    earlier call with the same arguments, accumulated into (a validation pass batch by batch) and returned."""
    attention = bool(attention)
    from . import ddv
    from .swin import SwinTransformer
    from .vit import VisionTransformer
    if stages not in ('engine', 'full'):
        raise ValueError("compute_stats: stages must be 'engine' or 'full', not %r" % (stages,))
    full = stages == 'full'
    if not isinstance(model, (SwinTransformer, VisionTransformer)):
        raise NotImplementedError('compute_stats covers the ViT / DeiT and the Swin models')
    if isinstance(model, SwinTransformer) and isinstance(bit_config, (list, tuple)):
        _compute_stats_swin(model, x, bit_config, with_linear, attention, into)       # raises
    if x.dim() != 4 or x.shape[0] < 1:
        raise AssertionError('compute_stats: the inputs must be one [n, C, H, W] batch')
    if isinstance(model, SwinTransformer):
        return _compute_stats_swin(model, x, bit_config, with_linear, attention, into)
    if attention and bit_config is not None and not model.cfg.INT_SOFTMAX:
        raise NotImplementedError('compute_stats(attention=True): under Config(lis=False) the quantized softmax is the float one, its '
                                  'probabilities are not codes')
    dev = ddv._device_of(model)
    x = x.to(dev).float()
    has_fp = bit_config is not None and any(int(b) == -1 for b in bit_config)
    fused_state = model._fused()
    if fused_state and not has_fp and dev.type == 'cuda':
        if bit_config is None:
            raise ValueError('None is not in list')              # bit_pool.index(None), vit_fquant.py:282
        if model._plan is None:
            model.freeze(dev)
        return model._plan.forward_stats(x, [int(b) for b in bit_config], with_linear, stages=stages, attention=attention, into=into)[1]
    if full and not getattr(model, 'input_quant', True):
        raise AttributeError("compute_stats(stages='full'): the model has no qact_input (input_quant=False), as in the reference's add_hooks")
    names = ddv.stage_names(model.depth, with_linear, full, attention)
    outs = ddv._hooked_outputs(model, x, bit_config, names, fused_state)
    return (code_stats if dev.type == 'cuda' else code_stats_cpu)(outs, names, into=into)


def _check_cli(args):
    """the refusals that need no model: before anything is built or run"""
    if args.attention and args.no_lis:
        raise NotImplementedError('--attention --no-lis: under Config(lis=False) the quantized softmax is the float one, its probabilities '
                                  'are not codes')
    if args.model.startswith('swin') and args.bits == 'mixed':
        raise NotImplementedError('--bits mixed: a Swin model has one weight width (swin_quant.py:813-817)')


def main(argv=None):
    p = argparse.ArgumentParser(description='stage statistics of a quantized model on synthetic data (plot_distrib.py)')
    p.add_argument('--model', default='deit_small')
    p.add_argument('--bits', default='8', choices=['8', '4', 'mixed'])
    p.add_argument('--n', default=64, type=int, help='images')
    p.add_argument('--batch', default=64, type=int, help='images per engine call (accumulated on the device)')
    p.add_argument('--stages', default='engine', choices=['engine', 'full'])
    p.add_argument('--attention', action='store_true', help='also the QActs inside the attention kernels')
    p.add_argument('--with-linear', action='store_true', help='also the fp32 outputs of the linear layers')
    p.add_argument('--no-ptf', action='store_true', help='Config(ptf=False): float LayerNorm (ViT / DeiT and Swin)')
    p.add_argument('--no-lis', action='store_true', help='Config(lis=False): float softmax (not with --attention)')
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--device', default='cuda')
    p.add_argument('--result-name', default='stats_result')
    p.add_argument('--softmax-bits', default=None, type=int, choices=[3, 4], help='width of the log-int-softmax (Config.BIT_TYPE_S: uint3 / uint4; default 4)')
    args = p.parse_args(argv)
    _check_cli(args)
    from . import harness, synth
    from .config import Config
    device = torch.device(args.device)
    q = harness.str2model(args.model)(cfg=Config(not args.no_ptf, not args.no_lis, 'minmax').set_softmax_bits(args.softmax_bits))
    is_swin = harness._is_swin(q)
    if not hasattr(q, 'arch') or not (is_swin or hasattr(q, 'depth')):
        raise NotImplementedError('the statistics tool covers the ViT / DeiT and the Swin models')
    if is_swin:
        q.load_state_dict(synth.swin_state_dict(q.state_dict(), args.seed))
        bits = int(args.bits)
    else:
        q.load_state_dict(synth.vit_state_dict(q.arch, args.seed), strict=False)
        L = 4 * q.depth + 2
        bits = {'8': [8] * L, '4': [4] * L, 'mixed': [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)]}[args.bits]
    q = q.to(device).eval()
    harness.calibrate_model(q, synth.images(args.seed + 1, 10, q.arch['img_size']).to(device))
    x = synth.images(args.seed + 2, args.n, q.arch['img_size']).to(device)
    st = None
    for i in range(0, args.n, args.batch):      # a validation pass: every batch accumulates into the same records on the device
        st = compute_stats(q, x[i:i + args.batch], bits, with_linear=args.with_linear, stages=args.stages, attention=args.attention, into=st)
    st = st.cpu()
    result = {}
    for nm in st.names:
        r = st.record(nm)
        lo, hi = st.channel_ranges(nm)
        fin = torch.isfinite(lo) & torch.isfinite(hi)
        width = torch.where(fin, hi - lo, torch.zeros_like(hi))
        top = torch.topk(width, min(3, width.numel())).indices.tolist()
        lo_r, hi_r = st.rail_share(nm)
        if st.kind(nm) == 'f32':
            used = 'values %+.4g ... %+.4g' % (float(lo[fin].min()) if fin.any() else float('nan'), float(hi[fin].max()) if fin.any() else float('nan'))
        else:
            used = 'codes %4d ... %4d' % (int(r['lo'].min()), int(r['hi'].max()))
        print('%-34s %-3s %-32s rails %.4f / %.4f  used bits %.2f  widest channels %s' % (nm, st.kind(nm), used, lo_r, hi_r, st.used_bits(nm), top))
        result[nm] = {k: v.numpy().copy() for k, v in r.items()}
        result[nm].update(kind=st.kind(nm), lo_value=lo.numpy(), hi_value=hi.numpy())
    os.makedirs(args.result_name, exist_ok=True)
    path = os.path.join(args.result_name, 'stats.pkl')
    with open(path, 'wb') as f:
        pickle.dump({'stages': st.names, 'records': result, 'bits': bits, 'n': args.n}, f)
    print('%d stages, %d images -> %s' % (len(st.names), args.n, path))
    return st


if __name__ == '__main__':
    main()
