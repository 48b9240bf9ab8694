"""GPU: what device-side scoring (score.DeviceMeter, harness.validate(device_metrics=True), harness.validate_many) buys at the headline
configuration (DeiT-S int8, batch 256), all legs in one process:
  (a) resident input   validate over 40 batches already in HBM: the default path against device_metrics=True, alternating, 5 repeats each
  (b) pinned host      25 random bit configurations x 20 batches from pinned host memory: config-major (one validate per configuration,
                       default path and device_metrics=True) against validate_many (batch-major: every batch is copied once)
  (c) kernels alone    the two score kernels at 256 x 1000 in a child process under `rocprofv3 --kernel-trace --stats` (a run of its own)
Also printed, not asserted: the distance of the fp64 loss to torch's fp32 cross-entropy on the same logits, and how many rows of the batch
have a tie at the top-1 / top-5 boundary.
python tools/score_bench.py [out.txt]            python tools/score_bench.py --kernels [reps]   (the child of leg (c))"""
import contextlib, csv, glob, io, json, os, random, statistics, subprocess, sys, tempfile, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import diff_vit_amd as dva

B, CLASSES = 256, 1000

if len(sys.argv) > 1 and sys.argv[1] == '--kernels':
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    g = torch.Generator().manual_seed(0)
    x = (torch.randint(-128, 128, (B, CLASSES), generator=g).float() * 2.0 ** -3).cuda()
    y = torch.randint(0, CLASSES, (B,), generator=g).cuda()
    m = dva.DeviceMeter(device='cuda')
    for _ in range(reps):
        m.update(x, y)
    print(json.dumps({'reps': reps, 'result': m.result()}))
    sys.exit(0)

out_path = sys.argv[1] if len(sys.argv) > 1 else None
H = dva.harness
dev = torch.device('cuda')
model = dva.deit_small_patch16_224(pretrained=False, cfg=dva.Config()).cuda().eval()
model.load_state_dict(dva.synth.vit_state_dict(dva.synth.ARCHS['deit_small'], 5), strict=False)
H.calibrate_model(model, dva.synth.images(5, 2, 224).cuda())
bc = [8] * 50
args = H.build_parser().parse_args(['--print-freq', '1000000'])
crit = torch.nn.CrossEntropyLoss().cuda()
host = dva.synth.images(5, 64, 224).repeat(4, 1, 1, 1).contiguous().pin_memory()
res_dev = host.cuda()
with torch.no_grad():
    logits = model(res_dev, bc, False)[0].clone()
tgt_dev = logits.argmax(1)
tgt_dev[::3] = (tgt_dev[::3] + 1) % CLASSES                                  # a third of the labels wrong: Prec@1 is not trivially 100
tgt_host = tgt_dev.cpu().pin_memory()


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0


def spread(v):
    return {'median': round(statistics.median(v)), 'min': round(min(v)), 'max': round(max(v)), 'all': [round(x) for x in v]}


lines, js = [], {}
# ---- (a) resident input
n_a = 40
resident = [(res_dev, tgt_dev)] * n_a
legs_a = {'default': lambda: H.validate(args, resident, model, crit, dev, bc),
          'device_metrics': lambda: H.validate(args, resident, model, None, dev, bc, device_metrics=True)}
for fn in legs_a.values():
    quiet(fn)                                                                # warm-up: side streams, allocator
rate_a, val_a = {k: [] for k in legs_a}, {}
for r in range(5):
    for k, fn in legs_a.items():
        val_a[k], t = quiet(fn)
        rate_a[k].append(B * n_a / t)
js['a_resident_img_per_s'] = {k: spread(v) for k, v in rate_a.items()}
js['a_results'] = {k: [round(float(x), 6) for x in v] for k, v in val_a.items()}
lines.append('(a) resident input, validate over %d batches of %d, 5 alternating repeats (img/s, whole call: forward + scoring)' % (n_a, B))
for k, v in js['a_resident_img_per_s'].items():
    lines.append('    %-28s median %7d   min %7d   max %7d   %s' % (k, v['median'], v['min'], v['max'], v['all']))
lines.append('    (loss, Prec@1, Prec@5): default %s   device_metrics %s' % (js['a_results']['default'], js['a_results']['device_metrics']))

# ---- (b) pinned host input, 25 configurations
n_b, n_cfg, reps_b = 20, 25, 3
pinned = [(host, tgt_host)] * n_b
rng = random.Random(0)
configs = [[8] + [rng.choice((4, 8)) for _ in range(49)] for _ in range(n_cfg)]
legs_b = {'config_major_default': lambda: [H.validate(args, pinned, model, crit, dev, c)[1] for c in configs],
          'config_major_device_metrics': lambda: [H.validate(args, pinned, model, None, dev, c, device_metrics=True)[1] for c in configs],
          'validate_many': lambda: [r[1] for r in H.validate_many(args, pinned, model, dev, configs)]}
quiet(lambda: H.validate_many(args, pinned[:2], model, dev, configs))          # warm-up: both weight widths of every layer touched once
rate_b, val_b = {k: [] for k in legs_b}, {}
for r in range(reps_b):
    for k, fn in legs_b.items():
        val_b[k], t = quiet(fn)
        rate_b[k].append(B * n_b * n_cfg / t)
js['b_pinned_img_per_s'] = {k: spread(v) for k, v in rate_b.items()}
js['b_same_top1_many_vs_config_major'] = val_b['validate_many'] == val_b['config_major_device_metrics']
lines.append('(b) pinned host input, %d random configurations x %d batches of %d, %d alternating repeats (forwarded img/s)' % (n_cfg, n_b, B, reps_b))
for k, v in js['b_pinned_img_per_s'].items():
    lines.append('    %-28s median %7d   min %7d   max %7d   %s' % (k, v['median'], v['min'], v['max'], v['all']))
lines.append('    validate_many == config-major device_metrics, all %d Prec@1 values: %s' % (n_cfg, js['b_same_top1_many_vs_config_major']))

# ---- ties and the distance to torch's fp32 loss, on the resident batch (printed, not asserted)
ranks, loss = torch.ops.p2vit.score_logits(logits, tgt_dev)
rk = ranks.cpu().numpy().astype('int64')
gt, lo, hi = rk[:, 0], rk[:, 1], rk[:, 2]
js['ties'] = {'rows': B, 'distinct_values_per_row_mean': round(float(sum(len(set(r.tolist())) for r in logits.cpu()) / B), 1),
              'top1_boundary_rows': int(((gt + lo + hi < 1) != (gt < 1)).sum()), 'top5_boundary_rows': int(((gt + lo + hi < 5) != (gt < 5)).sum())}
l32 = torch.nn.functional.cross_entropy(logits, tgt_dev, reduction='none')
l64 = torch.nn.functional.cross_entropy(logits.double(), tgt_dev, reduction='none')
js['loss_distance'] = {'max_abs_dev_fp64_vs_torch_fp32': float((loss - l32.double()).abs().max()),
                       'max_abs_dev_fp64_vs_torch_fp64': float((loss - l64).abs().max()),
                       'bound_at_1000_classes': float((CLASSES + 64) * 2.0 ** -52 * max(1.0, float(l64.abs().max())))}
lines.append('ties on the resident batch (synthetic weights): %s' % json.dumps(js['ties']))
lines.append('loss: %s' % json.dumps(js['loss_distance']))

# ---- (c) the two kernels alone: a child process under rocprofv3, a run of its own
reps_c = 200
with tempfile.TemporaryDirectory() as d:
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
           '--kernels', str(reps_c)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
    stats = sorted(glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True))
    kern = {}
    for f in stats:
        for row in csv.DictReader(open(f)):
            if 'k_score' in row.get('Name', ''):
                kern[row['Name'].split('(')[0]] = {'calls': int(row['Calls']), 'avg_us': round(float(row['AverageNs']) / 1e3, 2),
                                                   'min_us': round(float(row['MinNs']) / 1e3, 2), 'max_us': round(float(row['MaxNs']) / 1e3, 2)}
    js['c_kernels_256x1000'] = kern or {'error': 'no kernel stats (rc %d): %s' % (p.returncode, (p.stderr or p.stdout)[-300:])}
lines.append('(c) the score kernels alone at %d x %d, %d launches each, rocprofv3 --kernel-trace --stats (us)' % (B, CLASSES, reps_c))
for k, v in js['c_kernels_256x1000'].items():
    lines.append('    %-28s %s' % (k, v))
txt = '\n'.join(lines)
print(txt)
print(json.dumps(js))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, 'w').write(txt + '\n' + json.dumps(js) + '\n')
