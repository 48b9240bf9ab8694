"""GPU: what the stage statistics cost.  One process, one stream, alternating repeats, median [min .. max]:
  - DeiT-S at 256 images, all layers 8 bit, and Swin-B at 64 images: ms per call of forward, forward_ddv (n = half the batch) and
    forward_stats, each for the engine, FULL and attention stage sets (Swin has one list: without / with the attention stages);
  - the reduction alone (p2v_code_stats, one launch) on the stage shapes of those two models: us per launch and bytes read per second,
    against the 6.29 TB/s a float4 copy reaches on this device;
  - with --parent DIR (a built tree of the parent commit): bench.py and bench.py --model swin_base from both trees in turn, a fresh process
    each, three runs - the ranges and the md5 of the logits.
python tools/bench_stage_stats.py [--repeats 5] [--parent DIR]  ->  stdout (profiles/stage_stats.txt is one run of it)"""
import argparse, ctypes, hashlib, json, os, statistics, subprocess, sys, tempfile
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import diff_vit_amd as dva
from diff_vit_amd import engine as E

HBM = 6.29e12          # bytes / s of a float4 copy (measured peak of the device)


def spread(v):
    return statistics.median(v), min(v), max(v)


def event_ms(run, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(cases, repeats):
    """cases: name -> callable.  Every callable once to warm up, then `repeats` rounds through all of them in turn"""
    for run in cases.values():
        run()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(repeats):
        for k, run in cases.items():
            ms[k].append(event_ms(run))
    return {k: spread(v) for k, v in ms.items()}


def show(title, res, base):
    print(title, flush=True)
    for k, (m, lo, hi) in res.items():
        print('  %-44s %8.3f ms [%8.3f .. %8.3f]   %+7.3f ms over forward' % (k, m, lo, hi, m - res[base][0]), flush=True)


def vit_cases(repeats):
    arch = dva.synth.ARCHS['deit_small']
    m = dva.deit_small_patch16_224(cfg=dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(arch, 5), strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(5, 2, 224).cuda())
    m.freeze('cuda')
    plan, bits = m._plan, [8] * 50
    x = dva.synth.images(5, 256, 224, offset=100).cuda()
    cases = {'forward (one stream)': lambda: plan.forward(x, bits)}
    keep = {}
    for stages, att in (('engine', False), ('full', False), ('engine', True)):
        tag = stages + (' + attention' if att else '')
        cases['forward_ddv   %s' % tag] = lambda s=stages, a=att: plan.forward_ddv(x, bits, False, stages=s, attention=a)
        keep[tag] = plan.forward_stats(x, bits, False, stages=stages, attention=att)[1]
        cases['forward_stats %s' % tag] = lambda s=stages, a=att, t=tag: plan.forward_stats(x, bits, False, stages=s, attention=a, into=keep[t])
    show('DeiT-S, 256 images, [8] * 50 (forward_ddv: n = 128 pairs); records: %s bytes' % ', '.join('%s %d' % (k, v.arena.numel()) for k, v in keep.items()),
         alternate(cases, repeats), 'forward (one stream)')
    T, D = plan.tokens, plan.D
    shapes = [('qact1 / qact2 / qact4 [197][384] i8', 0, 256, T, D, D), ('attn.qact1 [197][1152] i8', 0, 256, T, 3 * D, 3 * D), ('mlp.qact1 [197][1536] i8', 0, 256, T, 4 * D, 4 * D),
              ('attn.qact_attn1 [6*197][197] pitch 208 i8', 0, 256, 6 * T, T, 208), ('attn.log_int_softmax [6*197][197] pitch 208 u8', 2, 256, 6 * T, T, 208),
              ('norm1 [197][384] f32', 1, 256, T, D, D), ('mlp.fc1 [197][1536] f32', 1, 256, T, 4 * D, 4 * D), ('act_out [1][1000] f32', 1, 256, 1, 1000, 1000)]
    del m, plan, keep
    torch.cuda.empty_cache()
    return shapes


def swin_cases(repeats):
    m = dva.swin_base_patch4_window7_224(cfg=dva.Config(True, True, 'minmax')).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    m = m.cuda()
    dva.harness.calibrate_model(m, dva.synth.images(5, 2, 224).cuda())
    x = dva.synth.images(5, 64, 224, offset=100).cuda()
    with torch.no_grad():
        m(x, bits=8)
    plan = m._plan
    cases = {'forward (one stream)': lambda: plan.forward(x, n_streams=1)}
    keep = {}
    for att in (False, True):
        tag = 'all stages' + (' + attention' if att else '')
        cases['forward_ddv   %s' % tag] = lambda a=att: plan.forward_ddv(x, False, attention=a)
        keep[tag] = plan.forward_stats(x, False, attention=att)[1]
        cases['forward_stats %s' % tag] = lambda a=att, t=tag: plan.forward_stats(x, False, attention=a, into=keep[t])
    show('Swin-B 224, 64 images, 8 bit (forward_ddv: n = 32 pairs; the model-diff sequences run unfused); records: %s bytes'
         % ', '.join('%s %d' % (k, v.arena.numel()) for k, v in keep.items()), alternate(cases, repeats), 'forward (one stream)')
    shapes = [('layers.0 qact1 [3136][128] i8', 0, 64, 3136, 128, 128), ('layers.0 mlp.qact1 [3136][512] i8', 0, 64, 3136, 512, 512),
              ('layers.0 attn.qact_attn1 [64*4*49][49] pitch 64 i8', 0, 64, 64 * 4 * 49, 49, 64), ('layers.2 qact1 [196][512] i8', 0, 64, 196, 512, 512),
              ('layers.2 downsample.qact1 [49][2048] i8', 0, 64, 49, 2048, 2048), ('layers.3 mlp.fc1 [49][4096] f32', 1, 64, 49, 4096, 4096), ('qact3 [1][1024] i8', 0, 64, 1, 1024, 1024)]
    del m, plan, keep
    torch.cuda.empty_cache()
    return shapes


def reduction_alone(shapes, repeats):
    print('the reduction alone (one p2v_code_stats launch, median of %d x 20 launches; the plane does not fit the 4 MiB L2 of an XCD unless noted):' % repeats, flush=True)
    L = E.lib()
    for name, kind, S, R, cols, rs in shapes:
        esz = 4 if kind == 1 else 1
        buf = torch.randint(0, 255, (S * R * rs * esz,), dtype=torch.uint8, device='cuda')
        if kind == 1:
            buf = torch.randn(S * R * rs, device='cuda').view(torch.uint8)
        rec = torch.empty(L.p2v_stats_bytes(cols), dtype=torch.uint8, device='cuda')
        E.check(L.p2v_stats_init(E.ptr(rec), rec.numel(), kind, cols, E.stream_ptr()))
        lay = (E.StatLayer * 1)()
        lay[0].base, lay[0].sample_stride, lay[0].row_stride, lay[0].samples, lay[0].rows, lay[0].cols, lay[0].dtype = buf.data_ptr(), R * rs, rs, S, R, cols, kind
        recs = (ctypes.c_void_p * 1)(rec.data_ptr())
        run = lambda: E.check(L.p2v_code_stats(lay, 1, recs, None, 0, E.stream_ptr()))
        run()
        torch.cuda.synchronize()
        m, lo, hi = spread([event_ms(run, 20) for _ in range(repeats)])
        nbytes = S * R * cols * esz
        print('  %-52s %8.1f us [%8.1f .. %8.1f]   %7.1f MB   %6.3f TB/s = %4.1f %% of the copy rate'
              % (name, m * 1e3, lo * 1e3, hi * 1e3, nbytes / 1e6, nbytes / (m * 1e-3) / 1e12, 100 * nbytes / (m * 1e-3) / HBM), flush=True)


def parent_check(parent, steps, warmup, repeats):
    """bench.py of the parent's tree and of this one, a fresh process each, in turn"""
    trees = (('parent', os.path.abspath(parent)), ('this', ROOT))
    for extra in ([], ['--model', 'swin_base']):
        vals, md5 = {'parent': [], 'this': []}, {'parent': set(), 'this': set()}
        for _ in range(repeats):
            for tag, tree in trees:
                with tempfile.TemporaryDirectory() as d:
                    out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--no-cpu-baseline',
                                          '--dump-outputs', d] + extra, cwd=tree, check=True, capture_output=True, text=True, timeout=900).stdout
                    vals[tag].append(json.loads(out.strip().splitlines()[-1])['value'])
                    with open(os.path.join(d, 'logits.npy'), 'rb') as f:
                        md5[tag].add(hashlib.md5(f.read()).hexdigest())
        p, t = spread(vals['parent']), spread(vals['this'])
        same = md5['parent'] == md5['this'] and len(md5['this']) == 1
        overlap = p[1] <= t[2] and t[1] <= p[2]
        print('bench.py %-18s parent %9.1f img/s [%9.1f .. %9.1f]   this %9.1f img/s [%9.1f .. %9.1f]   ranges %s   logits md5 %s (%s)'
              % (' '.join(extra) or '(default)', p[0], p[1], p[2], t[0], t[1], t[2], 'overlap' if overlap else 'DO NOT OVERLAP',
                 'equal' if same else 'DIFFER', sorted(md5['this'])[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also run bench.py from both trees in turn')
    ap.add_argument('--bench-steps', type=int, default=30)
    ap.add_argument('--bench-warmup', type=int, default=5)
    args = ap.parse_args()
    with torch.no_grad():
        shapes = vit_cases(args.repeats)
        shapes += swin_cases(args.repeats)
        reduction_alone(shapes, args.repeats)
    if args.parent:
        torch.cuda.empty_cache()
        parent_check(args.parent, args.bench_steps, args.bench_warmup, 3)


if __name__ == '__main__':
    main()
