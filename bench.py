#!/usr/bin/env python3
"""Headline benchmark: images/sec of the PoT-PTQ quantized DeiT-S forward (int8, 224^2, batch 256 per GPU).

  python bench.py --gpus N --steps K --warmup W
  N>1 without a torch.distributed environment (WORLD_SIZE unset): bench.py starts the N ranks itself as a CHILD process
  (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>), before anything
  touches the GPU, relays rank 0's JSON line and exits with the child's code.  Under torch.distributed.run it is one rank.

One step = one quantized forward (fp32 images resident in HBM -> int8-grid logits) over one batch of 256
synthetic images per GPU, followed -- when N>1 -- by the single RCCL all-gather of the logits
(SURVEY.md 8e).  Weak scaling: per-GPU batch fixed.  Prints ONE JSON line on rank 0.

A plain run sets up (weights, host calibration, plan), runs W warm-up steps, times ONE loop of exactly K steps and prints the line
(`value`, `ms_per_step`, what ran).  --full adds what the headline does not need: 5 timed loops (median), top-1 against the fp32
model, the calibration against the reference fixture, the gathered logits against per-rank forwards, the roofline and per-kernel
profile, the CPU baseline.  --dump-outputs DIR writes the logits of the last timed step (DIR/logits.npy, float32); weights, images and
calibration come from fixed seeds, so two builds given the same arguments can be compared output for output.
"""
import argparse
import contextlib
import json
import os
import sys
import time

os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC: RCCL across processes needs it on this driver
# One hardware queue per HIP stream: the runtime's default of 4 is exhausted as soon as RCCL is initialised (its streams take queues of
# their own), two of the three slice streams then share one and the step falls from 2.64 to 3.6 ms (70 k img/s) on EVERY rank of a
# multi-GPU run - measured with a one-rank RCCL group, tools/gather_cost.py; 8 queues: 2.64 ms with the all-gather in the step.
# Read by the HIP runtime when it initialises, i.e. before the first HIP call of the process (diff_vit_amd sets the same default).
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MODEL, BATCH, SEED = 'deit_small', 256, 3
PEAK_INT8_TOPS = 5000.0   # dense int8 MFMA: 2x the ~2.5 PF dense bf16 rate (MI355X_MICROARCH.md, Matrix cores: I8 row)
PEAK_HBM_GBS = 8000.0     # HBM3E spec (same guide)


def algorithmic_work(kind, arch, B, bits=8):
    """(ops, bytes) of ONE launch of a kernel kind.  ops = 2*MAC of the dense contraction;
    bytes = compulsory HBM traffic (operands read once + result written once); 4-bit weights are stored packed, two per byte."""
    D, H, P = arch['embed_dim'], arch['num_heads'], arch['patch_size']
    T = (arch['img_size'] // P) ** 2 + 1
    Hd, M, hd, K0 = int(D * arch['mlp_ratio']), B * T, D // H, 3 * P * P
    g = lambda m, k, n, out_b=1, extra=0: (2.0 * m * k * n, m * k + n * k * bits // 8 + m * n * out_b + extra)
    return {
        'patchify': (0.0, B * 3 * arch['img_size'] ** 2 * 4 + B * (T - 1) * K0),
        'gemm_embed': g(B * (T - 1), K0, D),
        'fill_cls': (0.0, B * D),
        'layernorm': (0.0, 2 * M * D),
        'gemm_qkv': g(M, D, 3 * D),
        'attention': (4.0 * B * H * T * T * hd, M * 3 * D + M * D),
        'gemm_proj': g(M, D, D, extra=M * D),
        'gemm_fc1': g(M, D, Hd),
        'gemm_fc2': g(M, Hd, D, extra=M * D),
        'gemm_head': g(B, D, arch['num_classes'], out_b=4),
        'ln_gemm_qkv': g(M, D, 3 * D),           # LayerNorm fused in: reads the residual codes, writes the qkv codes
        'ln_gemm_fc1': g(M, D, Hd),
    }[kind]


def bench_swin(args, dva, dev, world, rank):
    """BASELINE config 4 family (parity-test case, not the headline line): Swin through the drop-in surface; the step is
    SwinPlan.forward (one p2v_run_ops replay per stream slice) + the all-gather of the logits."""
    with contextlib.redirect_stdout(sys.stderr):
        model = dva.harness.str2model(args.model)(cfg=dva.Config(True, True, 'minmax'))
    model.load_state_dict(dva.synth.swin_state_dict(model.state_dict(), SEED))
    model = model.to(dev).eval()
    arch = model.arch
    base = dva.synth.images(1000 + rank, args.batch, arch['img_size'])
    with torch.no_grad():
        if args.full:
            fp32_top1 = model(base.to(dev)).argmax(1).cpu()
        t_cal = time.perf_counter()
        dva.harness.calibrate_model(model, dva.synth.images(SEED, 2, arch['img_size']).to(dev))
        torch.cuda.synchronize()
        t_cal = time.perf_counter() - t_cal
    plan = model.freeze(dev, bits=args.bits)
    B = args.batch
    x = base.repeat((B + base.shape[0] - 1) // base.shape[0], 1, 1, 1)[:B].contiguous().to(dev)
    dist = args.dist
    sw_slices = [int(v) for v in args.slices.split(',')] if args.slices else None
    runner = dva.dp.DataParallelForward(lambda xs: plan.forward(xs, n_streams=args.streams, slices=sw_slices), arch['num_classes'], always_gather=args.force_dist)
    out, gat = [None], [None]

    def step():
        gat[0] = runner.local(x, world * B)
        out[0] = gat[0][rank * B:(rank + 1) * B] if world > 1 else gat[0]

    for _ in range(args.warmup):
        step()
    times = timed_repeats(step, args.steps, args.repeats, world, dev, dist)
    el = times[len(times) // 2]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, gat[0])
    line = headline(args, world, B, times, 'images/sec %s (quantized forward)' % args.model,
                    '%s PoT-PTQ forward, int%d weights, %dx%d, batch %d per GPU' % (args.model, args.bits, arch['img_size'], arch['img_size'], B))
    line['config'].update({'streams_per_gpu': args.streams, 'side_streams': dva.engine.SIDE_STREAM_REPORT.get(dev.index),
                           'collective': 'all_gather(logits)' if dist is not None else 'none', 'backend': args.backend if dist is not None else None,
                           **args.identity})
    calibration = {'seconds': round(t_cal, 2), 'device': 'gpu'}
    if not args.full:
        return finish(dict(line, calibration=calibration), rank, dist)
    # roofline of the dominant op kind: one launch = one stream slice, timed by p2v_run_ops_profile (HIP events on the launch stream)
    n_sl = len(sw_slices) if sw_slices else (args.streams if (args.streams > 1 and B >= 16 * args.streams) else 1)
    Bl = max(sw_slices) if sw_slices else (B + n_sl - 1) // n_sl
    prof = plan.profile(x[:Bl])
    prof = plan.profile(x[:Bl])
    rec = plan._recorded[(Bl, 0, True)]
    kinds = {}
    for i, (kind, epi, ms) in enumerate(prof):
        o = rec['ops'][i]
        name = kind + ('_' + {0: 'requant', 1: 'gelu', 2: 'resid', 4: 'head'}.get(epi, str(epi)) if kind in ('gemm', 'ln_gemm') else '')
        ops = 2.0 * o.M * o.K * o.N if kind in ('gemm', 'ln_gemm') else (4.0 * o.i0 * o.i1 * 49 * 32 * o.i2 if kind == 'window_attention' else 0.0)
        k = kinds.setdefault(name, [0, 0.0, 0.0])
        k[0] += 1; k[1] += ms; k[2] += ops
    dom = max(kinds, key=lambda n: kinds[n][1])
    n_l, ms_l, ops_l = kinds[dom]
    ach = ops_l / (ms_l * 1e-3) / 1e12
    roof = dict(kernel=dom, bound='mfma', achieved=round(ach, 2), peak=PEAK_INT8_TOPS, unit='TFLOP/s', frac=round(ach / PEAK_INT8_TOPS, 4),
                avg_launch_us=round(ms_l / n_l * 1e3, 2), launches_per_step=n_sl * n_l, images_per_launch=Bl, traffic=None)
    model_ops = n_sl * sum(v[2] for v in kinds.values())
    finish(dict(line, **{
        'roofline': roof,
        'top1_agreement_fp32': round(float((out[0][:base.shape[0]].argmax(1).cpu() == fp32_top1).float().mean()), 4),
        'model_mfma_frac': round(model_ops / (el / args.steps) / 1e12 / PEAK_INT8_TOPS, 4),
        'kernel_ms_per_step': {k: round(n_sl * v[1], 3) for k, v in sorted(kinds.items(), key=lambda kv: -kv[1][1])},
        'cpu_baseline': None, 'calibration': calibration,
    }), rank, dist)


def headline(args, world, B, times, metric, workload):
    """The part of the JSON line every run prints: the timed steps and what ran.  `times`: sorted seconds per timed loop."""
    el = times[len(times) // 2]                                      # median loop
    return {
        'metric': metric, 'value': round(world * B * args.steps / el, 1), 'unit': 'images/sec',
        'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(el / args.steps * 1e3, 3),
        'repeats': args.repeats, 'ms_per_step_min_max': [round(times[0] / args.steps * 1e3, 3), round(times[-1] / args.steps * 1e3, 3)],
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'int8' if args.bits == 8 else 'int4w/int8a', 'data': 'synthetic',
        'config': {'workload': workload, 'global_batch': world * B, 'parallelism': 'dp%d' % world},
    }


def finish(line, rank, dist):
    if rank == 0:
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(d, logits):
    """--dump-outputs: DIR/logits.npy, float32, one row per image.  Above DUMP_MAX_BYTES only a fixed, seeded sample of the rows is
    written (in row order), the same rows in every run with the same arguments."""
    import numpy as np
    a = logits.float().cpu().numpy()
    if a.nbytes > DUMP_MAX_BYTES:
        a = a[np.sort(np.random.RandomState(0).choice(len(a), DUMP_MAX_BYTES // a[0].nbytes, replace=False))]
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, 'logits.npy'), a)


def spawn_ranks(n):
    """`python bench.py --gpus N` on its own: run the N ranks as a child `torch.distributed.run` (never an exec: this process has
    not touched the GPU and does not need to), forward the child's output and exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', GPU_MAX_HW_QUEUES=os.environ.get('GPU_MAX_HW_QUEUES', '8')))
    sys.exit(r.returncode)


def timed_repeats(step, steps, repeats, world, dev, dist):
    """`repeats` timed loops of EXACTLY `steps` steps, each bracketed by barrier + torch.cuda.synchronize() on both sides; per loop
    the MAX over ranks; returns the sorted per-loop seconds.  `dist` is None when no process group exists."""
    out = []
    for _ in range(repeats):
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        out.append(el)
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=None, help='timed loops of --steps steps; the value is the median loop (default: 1, with --full 5)')
    ap.add_argument('--batch', type=int, default=BATCH, help='images per GPU (BASELINE config 2: 256)')
    ap.add_argument('--bits', type=int, default=8, choices=(4, 8))
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--streams', type=int, default=3, help='side HIP streams the per-GPU batch is sliced over; one more, smaller slice runs on the caller\'s stream (3: 68 + 68 + 68 + 52 of 256 images - four kernels in flight, FrozenPlan.slice_sizes)')
    ap.add_argument('--model', default=MODEL, choices=('deit_tiny', 'deit_small', 'deit_base', 'vit_base', 'swin_tiny', 'swin_base'))
    ap.add_argument('--backend', default='nccl', help='torch.distributed backend (nccl = RCCL; gloo for a rehearsal on one GPU)')
    ap.add_argument('--slices', default=None, help='explicit batch slices, e.g. 83,83,83,7 (default: FrozenPlan.slice_sizes)')
    ap.add_argument('--share-device', action='store_true', help='REHEARSAL ONLY: allow more ranks than visible GPUs (ranks then share devices; the line '
                    'says so in config.devices / distinct_devices).  Without it such a launch exits non-zero instead of printing an "N-GPU" number')
    ap.add_argument('--force-dist', action='store_true', help='initialise the process group and run the all-gather of the logits even at '
                    'world size 1 (under torch.distributed.run --nproc-per-node 1): exercises the RCCL branch on a one-GPU box')
    ap.add_argument('--full', action='store_true', help='also measure and check what the headline does not need: 5 timed loops, top-1 against '
                    'the fp32 model, calibration against the reference fixture, the gathered logits against per-rank forwards, the roofline '
                    'and per-kernel profile, the CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='after the timed steps, write the logits of the last step as DIR/logits.npy '
                    '(float32; rank 0: the gathered logits of all ranks)')
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1

    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        return spawn_ranks(args.gpus)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        sys.exit('bench.py --gpus %d was started with WORLD_SIZE=%d' % (args.gpus, world))
    if world > 1:      # the one-off host calibration of every rank runs at the same time: share the host cores instead of oversubscribing them
        torch.set_num_threads(max(1, min(32, (os.cpu_count() or 8) // world)))
    n_dev = torch.cuda.device_count()
    if world > n_dev and not args.share_device:
        sys.exit('bench.py: %d ranks but %d visible GPU(s): refusing to stack ranks on one device (an "%d-GPU" number would be a lie). '
                 'Pass --share-device for a rehearsal on fewer GPUs.' % (world, n_dev, world))
    hipq_before = torch.cuda.is_initialized()            # HIP initialised before the package could set GPU_MAX_HW_QUEUES?
    import diff_vit_amd as dva
    from diff_vit_amd import calib_io
    local = local % max(1, n_dev)
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if 'RANK' not in os.environ:           # --force-dist without a launcher: a one-rank group on a free local port
            import socket
            with socket.socket() as sk:
                sk.bind(('127.0.0.1', 0))
                os.environ.setdefault('MASTER_PORT', str(sk.getsockname()[1]))
            os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
        dist.init_process_group(args.backend, **({'device_id': dev} if args.backend == 'nccl' else {}))
    args.dist = dist
    # who is really here: every rank reports its device; rank 0 prints what the GROUP saw, not what the launcher was asked for
    props = torch.cuda.get_device_properties(dev)
    me = {'rank': rank, 'local_device': local, 'name': props.name, 'uuid': str(getattr(props, 'uuid', '')),
          'pci_bus_id': '%04x:%02x:%02x' % (getattr(props, 'pci_domain_id', 0), getattr(props, 'pci_bus_id', 0), getattr(props, 'pci_device_id', 0)),
          'host': os.uname().nodename}
    ident = [me]
    if dist is not None:
        ident = [None] * dist.get_world_size()
        dist.all_gather_object(ident, me)
    ranks_seen = dist.get_world_size() if dist is not None else 1
    if ranks_seen != world:
        sys.exit('bench.py: WORLD_SIZE=%d but the process group has %d ranks' % (world, ranks_seen))
    # two ranks share a device only if host, uuid, PCI address AND local index all coincide (a runtime that reports no uuid / PCI address still
    # tells ranks apart by their local index; per-rank visibility masks by uuid / PCI address)
    distinct = len({(d['host'], d['uuid'], d['pci_bus_id'], d['local_device']) for d in ident})
    if distinct < ranks_seen and not args.share_device:
        sys.exit('bench.py: %d ranks on %d distinct devices (%s): not an %d-GPU run' % (ranks_seen, distinct, ident, ranks_seen))
    args.identity = {'ranks_seen': ranks_seen, 'distinct_devices': distinct,
                     'devices': ['%d:%s/%s' % (d['rank'], d['pci_bus_id'], d['name']) for d in ident],
                     'shared_device_rehearsal': bool(distinct < ranks_seen),
                     'gpu_max_hw_queues': dict(dva.HW_QUEUES, hip_initialised_before_import=bool(hipq_before))}
    world = ranks_seen

    if args.model.startswith('swin'):
        return bench_swin(args, dva, dev, world, rank)
    arch = dva.synth.ARCHS[args.model]
    sd = dva.synth.vit_state_dict(arch, SEED)
    # the reference's flow through the drop-in surface: build, load, calibrate (float pass + observers, on the GPU),
    # model_quant(); the first quantized forward freezes the integer plan.  Calibration batch = the one the REAL
    # reference was calibrated on for tests/golden/deit_small.npz, so the resulting scales can be compared.
    with contextlib.redirect_stdout(sys.stderr):          # stdout carries exactly one JSON line
        model = dva.harness.str2model(args.model)(cfg=dva.Config(True, True, 'minmax'))
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).eval()
    base = dva.synth.images(1000 + rank, args.batch, arch['img_size'])
    if args.full:
        with torch.no_grad():                             # fp32 teacher on the distinct images, before any calibration
            fp32_top1 = model(base.to(dev))[0].argmax(1).cpu()
    t_cal = time.perf_counter()
    dva.harness.calibrate_model(model, dva.synth.images(SEED, 2, arch['img_size']).to(dev), where='host')    # exact exponents (harness.py)
    torch.cuda.synchronize()
    t_cal = time.perf_counter() - t_cal
    calib = model.export_calib()
    plan = model.freeze(dev)
    B = args.batch
    # every image of the batch is distinct (counter-based generator, seed 1000 + rank)
    x = base.repeat((B + base.shape[0] - 1) // base.shape[0], 1, 1, 1)[:B].contiguous().to(dev)
    if os.environ.get('P2V_BENCH_CONST_INPUT'):      # experiment (profiles/r03_slicing.txt): every image identical and constant -> low operand toggling
        x.fill_(0.25)
    bits = [args.bits] * (4 * arch['depth'] + 2)
    logits = torch.empty(B, arch['num_classes'], device=dev)
    # == model(x, bits)[0]; the per-GPU batch runs as contiguous slices on their own HIP streams (images are independent; the kernels
    # of one slice fill the latency/VALU gaps of the others; three side streams + the caller's stream = four kernels in flight measured best:
    # round 4, +1.7 % over three slices; a fourth SIDE stream collapses to 57 k img/s).  The N-GPU step is the product's data-parallel runner: every rank forwards
    # its own shard, then ONE all-gather of the logits -- dp.DataParallelForward, the class the gloo tests exercise.
    slices = [int(v) for v in args.slices.split(',')] if args.slices else plan.slice_sizes(B, args.streams)
    runner = dva.dp.DataParallelForward(lambda xs: plan.forward_streams(xs, bits, logits, args.streams, slices), arch['num_classes'],
                                        always_gather=args.force_dist)
    out = [None]

    def step():
        out[0] = runner.local(x, world * B)

    for _ in range(args.warmup):
        step()
    times = timed_repeats(step, args.steps, args.repeats, world, dev, dist)
    el = times[len(times) // 2]                                      # median loop
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out[0])
    line = headline(args, world, B, times, 'images/sec DeiT-S int8 224^2 b=256 (quantized forward)' if args.model == MODEL else 'images/sec %s (quantized forward)' % args.model,
                    args.model + ' PoT-PTQ forward, bit_config=[%d]*50, 224x224, batch %d per GPU' % (args.bits, B))
    line['config'].update({'streams_per_gpu': args.streams, 'side_streams': dva.engine.SIDE_STREAM_REPORT.get(dev.index), 'batch_slices': slices,
                           'collective': 'all_gather(logits)' if dist is not None else 'none', 'backend': args.backend if dist is not None else None})
    calibration = {'seconds': round(t_cal, 2), 'device': 'host cpu (float pass + observer searches; harness.calibrate_model where=host)'}
    if not args.full:
        line['config'].update(args.identity)
        return finish(dict(line, calibration=calibration), rank, dist)
    mine = calib_io.flatten(calib)
    ref_calib = calib_io.flatten(calib_io.load_npz(os.path.join(ROOT, 'tests', 'golden', 'deit_small.npz'))) if args.model == MODEL else mine
    # agreement with the REAL reference's calibration of the same weights/batch (float pass: expect ulp-level noise in the
    # PTF base scales and, on near-ties of the per-channel MSE search, an occasional exponent one step away)
    n_equal = sum(int(torch.equal(mine[k].reshape(-1), ref_calib[k].reshape(-1))) for k in ref_calib)
    exp_flips = sum(int((torch.log2(mine[k].reshape(-1) / ref_calib[k].reshape(-1)).abs() > 0.5).sum()) for k in ref_calib)
    n_elems = sum(ref_calib[k].numel() for k in ref_calib)
    gather_ok = None
    if dist is not None:
        # the gathered tensor holds every rank's logits: rank 0 recomputes each shard itself (rank r's images come from seed 1000 + r)
        assert out[0].shape[0] == world * B and torch.equal(out[0][rank * B:(rank + 1) * B], logits)
        if rank == 0:
            gather_ok = True
            chk = torch.empty_like(logits)
            for r in range(world):
                br = dva.synth.images(1000 + r, args.batch, arch['img_size'])
                xr = br.repeat((B + br.shape[0] - 1) // br.shape[0], 1, 1, 1)[:B].contiguous().to(dev)
                plan.forward_streams(xr, bits, chk, args.streams, slices)
                gather_ok = gather_ok and bool(torch.equal(chk, out[0][r * B:(r + 1) * B]))
            plan.forward_streams(x, bits, logits, args.streams, slices)       # restore this rank's logits for the checks below
    top1_fp32 = float((logits[:base.shape[0]].argmax(1).cpu() == fp32_top1).float().mean())   # BASELINE metric: top-1 vs fp32

    # ---- roofline of the dominant kernel: HIP events on the launch stream, measured live ----------------------
    # One LAUNCH in the timed region covers one batch slice (B / streams images, forward_streams): the profile passes time exactly those
    # launches - same kernels, same shapes - with events recorded on the launch stream between consecutive launches (the events are created
    # before the first launch is enqueued, p2v_forward_profile), (a) one slice alone = `isolated`, what rocprofv3 --kernel-trace of a
    # one-stream run shows, and (b) all slices concurrently = `under_overlap`, the regime of the headline.  Per kind: mean, median, min, max
    # over all launches of five passes.  The DOMINANT kernel is the kind with the largest share of the step under overlap.
    def stats(v):
        v = sorted(v)
        return {'mean': sum(v) / len(v), 'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}

    n_sl = len(slices)
    Bl = max(slices)
    prof, last_pass = {}, []
    n_pass = 5
    gaps = []
    for _ in range(n_pass):
        last_pass = plan.profile(x[:Bl], bits)
        gaps += [ms for kind, ms in last_pass if kind == 'event_gap']
        last_pass = [(kind, ms) for kind, ms in last_pass if kind != 'event_gap']
        for kind, ms in last_pass:
            prof.setdefault(kind, []).append(ms)
    # an interval = the launch + the handling of the event pair on the stream (measured: 1.5 - 2.5 us more than the kernel duration rocprofv3
    # --kernel-trace reports for the same launch).  The pass ends with an EMPTY interval (P2V_K_EVENT_GAP: two events, nothing between them);
    # it is reported as `event_gap_us` for orientation and NOT subtracted: two bare events cost more (4 - 5 us) than the pair adds around a kernel
    gap = sorted(gaps)[len(gaps) // 2] if gaps else 0.0
    # What the event pair adds to an interval WITH a kernel in it, calibrated on a kernel of known duration: k_stream_probe waits 20.0 us on the
    # constant-rate counter and rocprofv3 --kernel-trace reports it as PROBE_KERNEL_US (profiles/r04_kernel_stats_isolated.csv: 21.1 us average
    # over the 42 launches of exactly this train, 64 workgroups, alone on the stream); the same event chain around the train gives the interval,
    # and the difference is subtracted from every interval so that `avg_launch_us` is the kernel's duration as the profiler sees it
    # (uncorrected: +3 us = 11 - 14 % on these launches)
    PROBE_KERNEL_US = 21.1
    with torch.cuda.device(dev):
        st_cur = torch.cuda.current_stream(dev)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(41)]
        dva.engine.check(dva.engine.lib().p2v_stream_probe(st_cur.cuda_stream, 2, 20, 64, 0))
        evs[0].record(st_cur)
        for i in range(40):
            dva.engine.check(dva.engine.lib().p2v_stream_probe(st_cur.cuda_stream, 1, 20, 64, 0))
            evs[i + 1].record(st_cur)
        torch.cuda.synchronize(dev)
        iv = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(40))
    pair_ms = max(0.0, iv[len(iv) // 2] - PROBE_KERNEL_US * 1e-3)
    prof = {k: [max(ms - pair_ms, 0.0) for ms in v] for k, v in prof.items()}
    last_pass = [(kind, max(ms - pair_ms, 0.0)) for kind, ms in last_pass]
    iso = {k: stats(v) for k, v in prof.items()}
    launches = {k: len(v) // n_pass for k, v in prof.items()}                  # per slice and step
    tot = {k: n_sl * iso[k]['median'] * launches[k] for k in prof}             # per step: every slice issues the same launches
    ovl, ovl_wall = {}, None
    if n_sl > 1:
        acc_o, walls = {}, []
        for _ in range(3):
            per, wall = plan.profile_streams(x, bits, args.streams, slices, rounds=3)
            walls.append(wall)
            for pslice in per:
                for kind, ms in pslice:
                    if kind != 'event_gap':
                        acc_o.setdefault(kind, []).append(max(ms - pair_ms, 0.0))
        ovl = {k: stats(v) for k, v in acc_o.items()}
        ovl_wall = round(sorted(walls)[1], 3)
    tot_ovl = {k: ovl[k]['median'] * launches[k] for k in ovl} if ovl else tot
    dom = max(tot_ovl, key=tot_ovl.get)
    ops, byts = algorithmic_work(dom, arch, Bl, args.bits)
    avg_ms = iso[dom]['mean']
    if ops > 0:
        ach = ops / (avg_ms * 1e-3) / 1e12
        roof = dict(kernel=dom, bound='mfma', achieved=round(ach, 2), peak=PEAK_INT8_TOPS, unit='TFLOP/s',
                    frac=round(ach / PEAK_INT8_TOPS, 4))
        if ovl:
            roof['frac_under_overlap'] = round(ops / (ovl[dom]['mean'] * 1e-3) / 1e12 / PEAK_INT8_TOPS, 4)
    else:
        ach = byts / (avg_ms * 1e-3) / 1e9
        roof = dict(kernel=dom, bound='hbm', achieved=round(ach, 1), peak=PEAK_HBM_GBS, unit='GB/s',
                    frac=round(ach / PEAK_HBM_GBS, 4))
        if ovl:
            roof['frac_under_overlap'] = round(byts / (ovl[dom]['mean'] * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)
    roof['dominant_by'] = 'share of the step under overlap' if ovl else 'share of the isolated slice'
    # what the matrix pipe sustains on real data under the board's power limit (tools/ubench/mfma_power.hip, profiles/r03_mfma_power.txt):
    # the guide's peak is reached only with constant operands; listed beside it, never used for `frac`
    if roof['bound'] == 'mfma':
        roof['peak_sustained_measured'] = {'random_operands_in_registers': 3400.0, 'operands_from_lds': 2630.0, 'unit': 'TFLOP/s',
                                           'source': 'profiles/r03_mfma_power.txt (power-limited clock 1.66 / 1.41 GHz)'}
    us = lambda st: {k: round(v * 1e3, 2) for k, v in st.items()}
    roof['avg_launch_us'] = round(avg_ms * 1e3, 2)
    roof['event_pair_us'] = round(pair_ms * 1e3, 2)  # subtracted from the isolated intervals (calibrated on the 20 us probe kernel, see above)
    roof['event_gap_us'] = round(gap * 1e3, 2)       # an EMPTY event interval on the same stream (two bare events cost more; not used)
    roof['launch_us'] = us(iso[dom])
    roof['launch_us_under_overlap'] = us(ovl[dom]) if ovl else None
    # the launches of the dominant kind and of the fused LayerNorm+qkv kernel in program order (one per block) in the last isolated pass:
    # shows whether a deviation sits on one launch (e.g. block 0, right behind the stem) or on all of them
    roof['launch_us_by_block'] = {k: [round(ms * 1e3, 2) for kind, ms in last_pass if kind == k] for k in sorted({dom, 'ln_gemm_qkv'} & set(prof))}
    roof['launches_per_step'] = n_sl * launches[dom]
    roof['images_per_launch'] = Bl
    roof['algorithmic_per_launch'] = {'ops': ops, 'bytes': byts}
    # HBM-side bytes of that launch: PMC counters cannot be read inside the run (rocprofv3 wraps the process), so the figure is the
    # one tools/pmc.sh + tools/make_pmc_summary.py measured for the same launch size and committed; labelled as such, null if absent
    roof['traffic'], roof['traffic_source'] = None, None
    pmc = os.path.join(ROOT, 'profiles', 'pmc_summary.json' if args.model == MODEL else 'pmc_summary_%s.json' % args.model)
    if os.path.exists(pmc):
        try:
            t = json.load(open(pmc))
            if int(t.get('_images_per_launch', -1)) == Bl and t.get(dom) is not None:
                roof['traffic'], roof['traffic_source'] = t.get(dom), 'profiles/%s (separate rocprofv3 --pmc passes of this command, not this run)' % os.path.basename(pmc)
        except Exception:
            pass
    breakdown = {k: round(v, 3) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])}
    model_ops = sum(algorithmic_work(k, arch, Bl, args.bits)[0] * n_sl * launches[k] for k in prof)

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, 'oracle'))
        import p2vit_oracle as O           # test infrastructure: used here ONLY as the timed CPU baseline
        orc = O.OracleViT(arch, sd)
        orc.calib = calib
        # BASELINE.md section 3 protocol, bounded to about a minute and never sand-bagged: thread count tuned on a 16-image forward (at
        # all 128+ host threads this restatement runs 9x slower than at 16 on the EPYC 9575F box), then the batch of 16 / 64 with the
        # better images/sec (a 256-image forward takes 54 s = 4.7 img/s on that box: the softmax tensors leave the caches; measured once,
        # profiles/r02_k_bench.json), 1 warm-up + 3 timed forwards, median.
        n_host = os.cpu_count() or 1
        saved = torch.get_num_threads()
        x16 = x[:16].cpu()
        best_th, best_t = saved, None
        with torch.no_grad():
            orc.quant_forward(x16, bits)
            for th in [t for t in (8, 16, 32, 64) if t <= n_host] or [saved]:
                torch.set_num_threads(th)
                orc.quant_forward(x16, bits)
                t1 = time.perf_counter()
                orc.quant_forward(x16, bits)
                dt1 = time.perf_counter() - t1
                if best_t is None or dt1 < best_t:
                    best_th, best_t = th, dt1
            torch.set_num_threads(best_th)
            nb = 16
            if B >= 64 and best_t * 4 <= 8.0:            # try 64 images only if a forward is expected within 8 s
                x64 = x[:64].cpu()
                t1 = time.perf_counter()
                orc.quant_forward(x64, bits)
                if 64 / (time.perf_counter() - t1) > 16 / best_t:
                    nb = 64
            xc = x[:nb].cpu()
            ts = []
            for it in range(4):
                t1 = time.perf_counter()
                ref = orc.quant_forward(xc, bits)
                if it:
                    ts.append(time.perf_counter() - t1)
            ts.sort()
        torch.set_num_threads(saved)
        same = bool(torch.equal(ref, logits[:nb].cpu()))
        cpu = dict(value=round(nb / ts[1], 2), unit='images/sec', cores=best_th, kind='port', batch=nb,
                   sample='median of 3 forwards of %d images (same weights/bits/images as the GPU run) after 1 warm-up, %.1f s each; '
                          'oracle/p2vit_oracle.py torch-CPU restatement; torch threads %d picked from 8/16/32/64 on a 16-image forward; '
                          'host has %d hardware threads' % (nb, ts[1], best_th, n_host),
                   logits_equal_gpu=same)

    line['config'].update({'gathered_logits_equal_per_rank_forwards': gather_ok, **args.identity})
    finish(dict(line, **{
        'roofline': roof,
        'top1_agreement_fp32': round(top1_fp32, 4),
        'model_mfma_frac': round(model_ops / (el / args.steps) / 1e12 / PEAK_INT8_TOPS, 4),
        'kernel_ms_per_step': breakdown,
        'kernel_us_per_launch': {k: {'isolated': round(iso[k]['median'] * 1e3, 2), 'under_overlap': round(ovl[k]['median'] * 1e3, 2) if k in ovl else None,
                                     'share_under_overlap': round(tot_ovl[k] / sum(tot_ovl.values()), 3) if k in tot_ovl else None}
                                 for k in sorted(iso, key=lambda k: -tot_ovl.get(k, 0.0))},
        'overlap': {'longest_stream_ms_with_events': ovl_wall, 'note': 'medians over all launches; under_overlap = launch duration while the other slices '
                    'run (HIP events on each stream, FrozenPlan.profile_streams); isolated = one slice alone'} if ovl else None,
        'cpu_baseline': cpu,
        'calibration': dict(calibration, **{'tensors': len(ref_calib), 'tensors_bit_equal_reference': n_equal,
                                            'scale_elements': n_elems, 'elements_off_by_a_power_of_two': exp_flips}),
    }), rank, dist)


if __name__ == '__main__':
    main()
