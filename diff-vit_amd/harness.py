"""Evaluation harness of the hot path: the counterpart of the reference driver's ``validate / accuracy /
AverageMeter / seed / str2model`` and of its calibration sequence (test_quant.py:56-86,214-249,418-501).

Differences the build owns: a synthetic-data mode (no ImageFolder / torchvision / network),
``--mixed`` off by default (the reference's Hessian + Pareto search never completes as shipped, test_quant.py:186),
and images/sec reporting.  Everything else -- flag names, model-name map, the calibration call order, unpacking three
returns from ``model(data, bit_config, plot)``, top-k by ``output.topk(maxk, 1, True, True)`` and the print format --
follows the reference.
"""
import argparse
import contextlib
import io
import os
import random
import time

import numpy as np
import torch
import torch.nn as nn

from . import synth
from .config import Config
from . import vit


def build_parser():
    """same flags and defaults as test_quant.py:18-53 (plus --synthetic/--n-val for the offline mode)."""
    p = argparse.ArgumentParser(description='P2-ViT PoT-PTQ on MI355X')
    p.add_argument('--model', default='deit_tiny')
    p.add_argument('--data', default='/home/ubuntu/imagenet')
    p.add_argument('--quant', default=False, action='store_true')
    p.add_argument('--ptf', default=True)
    p.add_argument('--lis', default=True)
    p.add_argument('--no-ptf', dest='ptf', action='store_false', help='Config(ptf=False): layer-wise QActs around a float LayerNorm (ViT / DeiT and Swin)')
    p.add_argument('--no-lis', dest='lis', action='store_false',
                   help='Config(lis=False): float softmax instead of the log-int-softmax (ViT / DeiT and Swin)')
    p.add_argument('--softmax-bits', default=None, type=int, choices=[3, 4], help='width of the log-int-softmax (Config.BIT_TYPE_S: uint3 / uint4; default 4)')
    p.add_argument('--quant-method', default='minmax', choices=['minmax', 'ema', 'omse', 'percentile'])
    p.add_argument('--mixed', default=False, action='store_true')
    p.add_argument('--calib-batchsize', default=50, type=int, help='batchsize of calibration set')
    p.add_argument('--mode', default=1, type=int, help='calibration data: 1 Gaussian noise (offline default), 0 real data (--real-data), '
                   '2 images generated from the float model (psaq.generate_data)')
    p.add_argument('--psaq-iters', default=500, type=int, help='--mode 2: Adam steps per epoch of the data generation (generate_data.py:66)')
    p.add_argument('--calib-iter', default=6, type=int)
    p.add_argument('--val-batchsize', default=50, type=int, help='batchsize of validation set')
    p.add_argument('--num-workers', default=16, type=int)
    p.add_argument('--device', default='cuda', type=str, help='device')
    p.add_argument('--print-freq', default=100, type=int, help='print frequency')
    p.add_argument('--seed', default=0, type=int, help='seed')
    p.add_argument('--synthetic', default=True, action='store_true', help='synthetic ImageNet-shaped data and random-init weights')
    p.add_argument('--real-data', default=False, action='store_true',
                   help='evaluate on the ImageFolder tree under --data (val/, and train/ for --mode 0 calibration) through the PIL port of '
                        'build_transform (data.py; its equality with torchvision is unpinned)')
    p.add_argument('--pretrained', default=False, action='store_true', help='like the reference (test_quant.py:95): the checkpoint of the '
                   'torch-hub cache, <TORCH_HOME>/hub/checkpoints/<file> (checkpoint.PRETRAINED_FILES); never downloaded here')
    p.add_argument('--checkpoint', default='', help='local .pth / .npz checkpoint (checkpoint.load_checkpoint); default: seeded synthetic weights')
    p.add_argument('--n-val', default=500, type=int, help='number of synthetic validation images')
    p.add_argument('--bits', default=8, type=int, choices=[4, 8], help='uniform bit_config for the validation run')
    p.add_argument('--calib-on', default='host', choices=['host', 'model'], help="where the calibration pass runs: 'host' reproduces the reference's exponents exactly")
    p.add_argument('--uint8-input', default=False, action='store_true',
                   help='loaders yield uint8 NHWC crops (a quarter of the bytes to copy) and the model normalises them on the device '
                        '(forward_uint8 with the family\'s MODEL_STATS; logits identical to the fp32 loaders)')
    p.add_argument('--device-metrics', default=False, action='store_true',
                   help='score on the device (score.DeviceMeter): Prec@k with the lower-index-first tie rule and the fp64 loss, no host '
                        'synchronisation per batch; with --mixed the search scores whole populations batch-major (validate_many)')
    p.add_argument('--search-pop', default=25, type=int, help='--mixed: population size (test_quant.py:340)')
    p.add_argument('--search-iter', default=8, type=int, help='--mixed: evolutionary iterations (test_quant.py:343)')
    p.add_argument('--search-max-configs', default=50, type=int, help='--mixed: Pareto candidates kept (test_quant.py:281)')
    p.add_argument('--search-slack', default=1.1, type=float, help='--mixed: size constraint = slack x the all-4-bit model (test_quant.py:262)')
    p.add_argument('--hessian-batches', default=0, type=int,
                   help='--mixed: weight the search by the per-layer Hessian traces of this many batches (test_quant.py:147-191; 0: '
                        'every layer weighs 1)')
    p.add_argument('--hessian-batch-size', default=32, type=int, help='images per batch of --hessian-batches')
    p.add_argument('--hessian-probes', default='joint', choices=['joint', 'layer'],
                   help="'layer': one double backward per layer and probe, as the reference; 'joint': one per probe for all layers "
                        '(unbiased, noisier; hessian.hutchinson_traces)')
    return p


def str2model(name):
    """test_quant.py:56-68"""
    from . import swin
    d = {'deit_tiny': vit.deit_tiny_patch16_224, 'deit_small': vit.deit_small_patch16_224,
         'deit_base': vit.deit_base_patch16_224, 'vit_base': vit.vit_base_patch16_224,
         'vit_large': vit.vit_large_patch16_224, 'swin_tiny': swin.swin_tiny_patch4_window7_224,
         'swin_small': swin.swin_small_patch4_window7_224, 'swin_base': swin.swin_base_patch4_window7_224,
         'swin_base_384': swin.swin_base_patch4_window12_384, 'swin_large_384': swin.swin_large_patch4_window12_384}
    print('Model: %s' % name)
    return d[name]


def _is_swin(model):
    from .swin import SwinTransformer
    return isinstance(model, SwinTransformer)


def _forward(model, data, bit_config=None, stats=None):
    """``model(data, bit_config, plot)`` -> (output, FLOPs, distance).  The reference's Swin returns the logits alone and takes
    no bit_config (swin_quant.py:813-817); here a list of ``bit_config_length()`` entries gives every layer its width (a one-entry
    list keeps meaning "uniform"), FLOPs = ``layer_macs()`` and distance = the model's ``global_distance`` (filled by a calibration
    forward), both in bit-list order.
    ``stats`` = (mean, std): ``data`` is a uint8 NHWC batch for ``forward_uint8``."""
    if _is_swin(model):
        bits = 8 if not bit_config else (int(bit_config[0]) if len(bit_config) == 1 else [int(b) for b in bit_config])
        if stats is not None:
            return model.forward_uint8(data, bits, stats[0], stats[1], 'NHWC'), model.layer_macs(), model.global_distance
        return model(data, bits=bits), model.layer_macs(), model.global_distance
    if stats is not None:
        return model.forward_uint8(data, bit_config, stats[0], stats[1], 'NHWC')
    return model(data, bit_config, False)


def forward_many(model, data, bit_configs, stats=None):
    """[logits, ...]: those of ``_forward(model, data, bc, stats)`` for every ``bc`` of ``bit_configs``.  A fused ViT / DeiT model on a GPU
    runs lists without a -1 in ONE engine call that executes what the lists share once (``VisionTransformer.forward_many``, bit-equal to
    the per-list forwards).  Everything else is the per-list loop: any other model state, a list with -1, and Swin, whose forward is a
    recorded p2v_op sequence with no single buffer carried from block to block."""
    bit_configs = list(bit_configs)
    if bit_configs and not _is_swin(model) and model.many_on_engine(data, bit_configs):
        if stats is not None:
            return model.forward_many_uint8(data, bit_configs, stats[0], stats[1], 'NHWC')
        return model.forward_many(data, bit_configs)
    return [_forward(model, data, bc, stats)[0] for bc in bit_configs]


def uint8_stats(args):
    """(mean, std) of the model family (data.MODEL_STATS) when ``--uint8-input`` is on, else None"""
    if not getattr(args, 'uint8_input', False):
        return None
    from .data import MODEL_STATS, model_family
    mean, std, _ = MODEL_STATS[model_family(args.model)]
    return mean, std


def seed(seed=0):
    """test_quant.py:71-86"""
    os.environ['PYTHONHASHSEED'] = str(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


class AverageMeter(object):
    """test_quant.py:469-485"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def accuracy(output, target, topk=(1,)):
    """precision@k (test_quant.py:488-501)"""
    maxk = max(topk)
    batch_size = target.size(0)
    _, pred = output.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[:k].reshape(-1).float().sum(0).mul_(100.0 / batch_size) for k in topk]


def calibrate_model(model, calibrate_data, where='host'):
    """the reference's calibration sequence (test_quant.py:235-249): one forward with calibrate + last_calibrate
    open, then close and switch to quant.

    ``where='host'`` (default): the one-off float pass and the observers' power-of-two searches run on the host CPU, whatever device
    the model lives on (it is moved there and back).  The searches pick the minimum of four nearly equal MSE scores per channel
    (minmax.py:198-240, ptf.py:96-134); only the host path reproduces the reference's choices exponent for exponent (DeiT-S: 495 of
    495 calibrated tensors, tests/test_module_surface.py and the GPU test of the same name), and the batched search makes it a
    couple of seconds instead of the reference's minute.  ``where='model'`` runs everything on the model's device (GPU: faster
    again, scores in fp64, but the float pass rounds differently there and a few hundred of 262 760 exponents move by one)."""
    if where not in ('host', 'model'):
        raise ValueError("where must be 'host' or 'model'")
    dev = next(model.parameters()).device
    on_host = where == 'host' and dev.type != 'cpu'
    if on_host:
        model.cpu()
        calibrate_data = calibrate_data.cpu()
    # the pass is hundreds of small tensor operations: on a many-core host torch's default thread count makes it an order of magnitude
    # slower (EPYC 9575F, DeiT-S: 14.4 s at 128 threads, 2.2 s at 32, 0.9 s at 16 - tools/calib_threads.py; the calibrated state is identical)
    n_threads = torch.get_num_threads()
    cpu_pass = where == 'host' or dev.type == 'cpu'
    if cpu_pass and n_threads > 16:
        torch.set_num_threads(16)
    try:
        model.model_open_calibrate()
        with torch.no_grad():
            model.model_open_last_calibrate()
            output, FLOPs, global_distance = _forward(model, calibrate_data)
        model.model_close_calibrate()
        model.model_quant()
    finally:
        if torch.get_num_threads() != n_threads:
            torch.set_num_threads(n_threads)
    if on_host:
        model.to(dev)
    return output, FLOPs, global_distance


class SyntheticLoader:
    """ImageNet-shaped batches from the deterministic generator; labels = argmax of a float teacher pass are supplied
    by the caller (there is no dataset offline), default labels are a fixed pseudo-random class per image."""

    def __init__(self, n, batch_size, img_size=224, num_classes=1000, seed=0, device='cpu', targets=None, uint8=False):
        self.n, self.bs, self.img, self.seed, self.device, self.uint8 = n, batch_size, img_size, seed, device, uint8
        self.targets = targets if targets is not None else torch.from_numpy(
            (synth._stream(seed, 'labels', n) % np.uint64(num_classes)).astype(np.int64))

    def __len__(self):
        return (self.n + self.bs - 1) // self.bs

    def __iter__(self):
        for i in range(0, self.n, self.bs):
            k = min(self.bs, self.n - i)
            gen = synth.images_uint8 if self.uint8 else synth.images         # uint8: NHWC crops, as a loader of PIL images yields them
            yield gen(self.seed, k, self.img, offset=i).to(self.device), self.targets[i:i + k].to(self.device)


class DevicePrefetcher:
    """``for data, target in DevicePrefetcher(loader, device)``: the batches of ``loader`` on ``device`` (any dtype: fp32 images or the
    uint8 crops of ``forward_uint8``), batch i + 1 copied while batch i runs.  The reference's loop does ``data.cuda()`` and then the forward, one after the other (test_quant.py:425-431); at 256 x 3 x 224^2 fp32
    the copy (154 MB, 2.8 ms at 55 GB/s) is longer than the DeiT-S forward (2.5 ms).  The copies run on ``engine.copy_stream`` - a stream
    probed to have a dispatch pipe of its own, which the sliced forward then leaves alone: 82 k img/s from pinned host memory against 45 k
    for copy-then-forward and 50 k for a double buffer on an arbitrary fifth stream (profiles/r04_pcie.txt).  uint8 batches for
    ``forward_uint8`` (38.5 MB instead of 154 MB): 102 k img/s against 87 k for the same images as fp32, 3 % below resident input
    (profiles/uint8_input.txt).  Pinned batches
    (``DataLoader(pin_memory=True)``, as the reference's loaders are) copy asynchronously; pageable ones work, without the overlap."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        dev = self.device
        if dev.type != 'cuda':
            for data, target in self.loader:
                yield data.to(dev), target.to(dev)
            return
        from . import engine as E
        st = E.copy_stream(dev)
        try:
            ahead = None
            for data, target in self.loader:
                cur = torch.cuda.current_stream(dev)
                st.wait_stream(cur)                       # (the caching allocator may hand the copy a block the current stream just released)
                with torch.cuda.stream(st):
                    d, t = data.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(st)
                if ahead is not None:
                    yield self._hand_over(ahead, dev)
                ahead = (d, t, ev)
            if ahead is not None:
                yield self._hand_over(ahead, dev)
        finally:
            E.release_copy_stream(dev)                    # (also when the consumer stops early): all side streams serve the forward again

    @staticmethod
    def _hand_over(item, dev):
        d, t, ev = item
        cur = torch.cuda.current_stream(dev)
        cur.wait_event(ev)
        d.record_stream(cur)
        t.record_stream(cur)
        return d, t


def validate(args, val_loader, model, criterion, device, bit_config=None, device_metrics=False):
    """test_quant.py:418-466; additionally returns images/sec of the forward calls.  ``device_metrics=True``: the same pass scored by
    ``score.DeviceMeter`` (``_validate_device_metrics``); ``criterion`` is not used then."""
    if device_metrics:
        return _validate_device_metrics(args, val_loader, model, device, bit_config)
    batch_time, losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    model.eval()
    val_start_time = end = time.time()
    n_img, fwd = 0, 0.0
    stats = uint8_stats(args)
    for i, (data, target) in enumerate(DevicePrefetcher(val_loader, device)):
        t0 = time.time()
        with torch.no_grad():
            output, FLOPs, distance = _forward(model, data, bit_config, stats)
        if data.is_cuda:
            torch.cuda.synchronize()
        fwd += time.time() - t0
        n_img += data.size(0)
        loss = criterion(output, target)
        prec1, prec5 = accuracy(output.data, target, topk=(1, 5))
        losses.update(loss.data.item(), data.size(0))
        top1.update(prec1.data.item(), data.size(0))
        top5.update(prec5.data.item(), data.size(0))
        batch_time.update(time.time() - end)
        end = time.time()
        if i % args.print_freq == 0:
            print('Test: [{0}/{1}]\t'
                  'Time {batch_time.val:.3f} ({batch_time.avg:.3f})\t'
                  'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                  'Prec@1 {top1.val:.3f} ({top1.avg:.3f})\t'
                  'Prec@5 {top5.val:.3f} ({top5.avg:.3f})'.format(i, len(val_loader), batch_time=batch_time, loss=losses,
                                                                 top1=top1, top5=top5))
    val_end_time = time.time()
    print(' * Prec@1 {top1.avg:.3f} Prec@5 {top5.avg:.3f} Time {time:.3f}'.format(top1=top1, top5=top5,
                                                                              time=val_end_time - val_start_time))
    print(' * forward throughput %.1f images/sec' % (n_img / max(fwd, 1e-9)))
    return losses.avg, top1.avg, top5.avg


def _validate_device_metrics(args, val_loader, model, device, bit_config=None):
    """``validate`` without a host synchronisation per batch: every batch enqueues the forward and the two score kernels, the meter is
    read at ``print_freq`` batches and at the end.  Prec@k follows the defined tie rule (among equal logits the lower class index ranks
    first) and the loss is the fp64 cross-entropy; one more line reports the bracket [sure, possible] any tie order lands in.  The
    printed running values are the averages so far (there is no per-batch value without a read per batch)."""
    from .score import DeviceMeter
    meter = DeviceMeter((1, 5), device=device)
    model.eval()
    val_start_time = time.time()
    n_img = 0
    stats = uint8_stats(args)
    for i, (data, target) in enumerate(DevicePrefetcher(val_loader, device)):
        with torch.no_grad():
            output, FLOPs, distance = _forward(model, data, bit_config, stats)
        meter.update(output, target)
        n_img += data.size(0)
        if i % args.print_freq == 0:
            r = meter.result()
            t = (time.time() - val_start_time) / (i + 1)
            print('Test: [{0}/{1}]\t'
                  'Time {t:.3f} ({t:.3f})\t'
                  'Loss {loss:.4f} ({loss:.4f})\t'
                  'Prec@1 {top1:.3f} ({top1:.3f})\t'
                  'Prec@5 {top5:.3f} ({top5:.3f})'.format(i, len(val_loader), t=t, loss=r['loss'], top1=r['prec'][1], top5=r['prec'][5]))
    r = meter.result()
    val_end_time = time.time()
    print(' * Prec@1 {top1:.3f} Prec@5 {top5:.3f} Time {time:.3f}'.format(top1=r['prec'][1], top5=r['prec'][5],
                                                                              time=val_end_time - val_start_time))
    print(' * ties: Prec@1 in [{0:.3f}, {1:.3f}] Prec@5 in [{2:.3f}, {3:.3f}] (sure / possible under any tie order; {4} rows, {5} invalid labels)'
          .format(r['sure'][1], r['possible'][1], r['sure'][5], r['possible'][5], r['n'], r['invalid']))
    print(' * throughput %.1f images/sec (whole pass, scoring included)' % (n_img / max(val_end_time - val_start_time, 1e-9)))
    return r['loss'], r['prec'][1], r['prec'][5]


def validate_many(args, val_loader, model, device, bit_configs):
    """[(loss, top1, top5), ...] of ``validate(..., device_metrics=True)`` for every entry of ``bit_configs``, in input order, from ONE
    pass over the loader: batch-major, each batch is brought to the device once and forwarded under every distinct configuration into
    a meter slot of its own (duplicates are scored once).  The mixed-precision search scores a population this way instead of
    re-reading the validation set per candidate.  On a fused ViT / DeiT model the configurations of a batch are one engine call that
    runs their common prefixes once (``forward_many``); the logits, and so the results, are those of the per-list forwards."""
    from .score import DeviceMeter
    keys = [None if bc is None else tuple(int(b) for b in bc) for bc in bit_configs]
    distinct = list(dict.fromkeys(keys))
    if not distinct:
        return []
    meter = DeviceMeter((1, 5), slots=len(distinct), device=device)
    model.eval()
    stats = uint8_stats(args)
    lists = [None if bc is None else list(bc) for bc in distinct]
    for data, target in DevicePrefetcher(val_loader, device):
        with torch.no_grad():
            outputs = forward_many(model, data, lists, stats)
        for s, output in enumerate(outputs):
            meter.update(output, target, slot=s)
    res = {}
    for s, bc in enumerate(distinct):
        r = meter.result(s)
        res[bc] = (r['loss'], r['prec'][1], r['prec'][5])
    return [res[k] for k in keys]


def _hessian_batches(args, loader, device):
    """the first ``--hessian-batches`` batches of ``--hessian-batch-size`` images of the loader with its labels (uint8 batches through the
    fp32 table, like the calibration batch)"""
    xs, ys, have, want = [], [], 0, args.hessian_batches * args.hessian_batch_size
    for x, y in loader:
        x = x.to(device)
        if x.dtype == torch.uint8:
            from .data import expand_uint8, uint8_lut
            x = expand_uint8(x, uint8_lut(*uint8_stats(args)), 'NHWC')
        xs.append(x)
        ys.append(y.to(device))
        have += x.shape[0]
        if have >= want:
            break
    x, y = torch.cat(xs)[:want], torch.cat(ys)[:want]
    n = args.hessian_batch_size
    return [(x[i:i + n], y[i:i + n]) for i in range(0, x.shape[0], n)]


def build_model_and_loaders(args, device):
    """the model of ``--model`` (seeded synthetic weights, ``--pretrained`` or ``--checkpoint``) on ``device`` in eval mode, its validation
    loader and, for ``--real-data``, the training loader the mode-0 calibration reads (else None)"""
    cfg = Config(args.ptf, args.lis, args.quant_method).set_softmax_bits(args.softmax_bits)
    model = str2model(args.model)(pretrained=args.pretrained, cfg=cfg)
    arch = model.arch
    if args.pretrained:
        pass
    elif _is_swin(model):
        model.load_state_dict(synth.swin_state_dict(model.state_dict(), args.seed))
    else:
        model.load_state_dict(synth.vit_state_dict(arch, args.seed), strict=False)
    if args.checkpoint:
        from .checkpoint import load_checkpoint
        load_checkpoint(model, args.checkpoint)
    model = model.to(device).eval()
    train_loader = None
    if args.real_data:
        # test_quant.py:118-144: ImageFolder val / train trees with the model family's mean / std / crop
        from .data import build_loaders
        loader, train_loader = build_loaders(args.data, args.model, args.val_batchsize, args.calib_batchsize, 0, uint8=args.uint8_input,
                                             input_size=arch['img_size'])
    else:
        # labels: the float model's own top-1 ("agreement with fp32"), the metric BASELINE.json names besides images/sec
        u8 = args.uint8_input
        loader = SyntheticLoader(args.n_val, args.val_batchsize, arch['img_size'], arch['num_classes'], args.seed, device, uint8=u8)
        with torch.no_grad():
            tgt = torch.cat([_forward(model, d, None, uint8_stats(args))[0].argmax(1).cpu() for d, _ in loader])
        loader = SyntheticLoader(args.n_val, args.val_batchsize, arch['img_size'], arch['num_classes'], args.seed, device, tgt, uint8=u8)
    return model, loader, train_loader


def calibration_data(args, model, train_loader, device):
    """the calibration batch of ``--mode`` (test_quant.py:205-233): 0 the first training batch, 2 images generated from the float model,
    else Gaussian noise"""
    if args.mode == 0 and train_loader is not None:
        print('Calibrating with real data...')                       # test_quant.py:214-233, mode 0: the first training batch
        calib_data = next(iter(train_loader))[0].to(device)
        if calib_data.dtype == torch.uint8:                          # --uint8-input: the normalised batch, through the fp32 table
            from .data import expand_uint8, uint8_lut
            calib_data = expand_uint8(calib_data, uint8_lut(*uint8_stats(args)), 'NHWC')
    elif args.mode == 2:
        print('Generating data...')                                  # test_quant.py:205-208, mode 2: PSAQ-ViT images from the float model
        from .data import model_family
        from .psaq import generate_data
        calib_data = generate_data(model, args.calib_batchsize, iterations=args.psaq_iters, family=model_family(args.model))
        print('Calibrating with generated data...')
    else:
        print('Calibrating with Gaussian noise...')
        calib_data = synth.images(args.seed + 1, args.calib_batchsize, model.arch['img_size']).to(device)
    return calib_data


def main(argv=None):
    args = build_parser().parse_args(argv)
    seed(args.seed)
    device = torch.device(args.device)
    model, loader, train_loader = build_model_and_loaders(args, device)
    arch = model.arch
    criterion = nn.CrossEntropyLoss().to(device)
    bit_config = None
    mean_hessian = None
    if args.mixed and args.hessian_batches > 0:
        # test_quant.py:147-191, before the calibration as there: the float model's per-layer Hessian traces weight the search
        print('Calculating the sensitiveties via the averaged Hessian trace.......')
        from .hessian import mean_hessian as _mean_hessian
        mean_hessian = _mean_hessian(model, criterion, _hessian_batches(args, loader if train_loader is None else train_loader, device), probes=args.hessian_probes, seed=args.seed,
                                     select='layers' if _is_swin(model) else 'reference')
        print('\n***Trace: ', mean_hessian)
    if args.quant:
        calib_data = calibration_data(args, model, train_loader, device)
        _, FLOPs, global_distance = calibrate_model(model, calib_data, where=args.calib_on)
        if args.mixed:
            # test_quant.py:253-408 on the fast path: every candidate bit_config is one validate() over the HIP engine (the frozen
            # plan holds both weight widths per layer, so switching configurations costs nothing)
            from .search import mixed_precision_search
            quiet = argparse.Namespace(**{**vars(args), 'print_freq': 10 ** 9})

            def score(bc):
                with contextlib.redirect_stdout(io.StringIO()):
                    return validate(quiet, loader, model, criterion, device, bc)[1]
            score_many = None
            if args.device_metrics:
                score_many = lambda cfgs: [r[1] for r in validate_many(quiet, loader, model, device, cfgs)]
            # Swin: the candidates tie {qkv, proj} and {fc1, fc2} of a block and keep the convolution at 8 bits (search_ties)
            ranked, pop = mixed_precision_search(score, FLOPs, global_distance, seed=args.seed, pop_size=args.search_pop,
                                                 evo_iter=args.search_iter, max_configs=args.search_max_configs, slack=args.search_slack,
                                                 score_many=score_many, ties=model.search_ties() if _is_swin(model) else None,
                                                 mean_hessian=mean_hessian)
            print('best mixed-precision configuration: Prec@1 %.3f' % pop[0][1])
            print(pop[0][0])
            return validate(args, loader, model, criterion, device, pop[0][0], device_metrics=args.device_metrics) + (pop[0][0],)
        bit_config = [args.bits] * ((4 * arch['depth'] + 2) if 'depth' in arch else 1)
        print(bit_config)
    return validate(args, loader, model, criterion, device, bit_config, device_metrics=args.device_metrics)


if __name__ == '__main__':
    main()
