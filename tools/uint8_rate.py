"""GPU: what uint8 input buys at the headline configuration (DeiT-S int8, batch 256), every regime in one process, rounds alternating:
  resident fp32     FrozenPlan.forward_streams on fp32 images already in HBM (bench.py's number)
  resident uint8    FrozenPlan.forward_uint8_streams on uint8 NHWC images already in HBM
  host-fed fp32     harness.DevicePrefetcher over pinned fp32 batches feeding forward_streams
  host-fed uint8    harness.DevicePrefetcher over pinned uint8 batches feeding forward_uint8_streams
  copy+fwd uint8    data.cuda() then the forward, one after the other (the reference's loop, test_quant.py:425-431)
Also the host -> device copy rate of one batch of each dtype.  python tools/uint8_rate.py [batches per pass] [rounds] [out.txt]

python tools/uint8_rate.py --patchify {warm,cold} [reps]: only the two patch kernels at one 68-image DeiT slice (the launch size of the
default slicing), for `rocprofv3 --kernel-trace --stats -- python tools/uint8_rate.py --patchify ...`.  warm: the same input every launch
(a 10 MB uint8 slice stays in the 256 MiB Infinity Cache, as inside the forward); cold: rotating over more than 256 MiB of inputs."""
import json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import diff_vit_amd as dva
from diff_vit_amd import data as D

if len(sys.argv) > 1 and sys.argv[1] == '--patchify':
    mode, reps = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 200
    E, B, S, P, Cn = dva.engine, 68, 224, 16, 3
    mean, std, _ = D.MODEL_STATS['deit']
    lut = D.uint8_lut(mean, std)
    inv_s = 32.0
    k_pad = 768
    n_buf = 1 if mode == 'warm' else 34                                 # cold: 34 x 10.2 MB uint8, 34 x 40.9 MB fp32 (> 256 MiB each)
    u8 = [dva.synth.images_uint8(7, B, S, offset=B * i).cuda() for i in range(min(n_buf, 2))]
    u8 = (u8 * n_buf)[:n_buf] if n_buf > 2 else u8
    u8 = [t.clone() for t in u8]
    f32 = [D.normalize_uint8(t.cpu(), mean, std).cuda() for t in u8]
    li8 = D.uint8_lut_i8(lut, inv_s).cuda()
    o32 = torch.empty(B * 196, k_pad, dtype=torch.int8, device='cuda')
    o8 = torch.empty_like(o32)
    L, st = E.lib(), E.stream_ptr()
    for r in range(reps):
        i = r % n_buf
        E.check(L.p2v_quantize_patchify(E.ptr(f32[i]), B, Cn, S, S, P, inv_s, E.ptr(o32), k_pad, st))
        E.check(L.p2v_u8_patchify(E.ptr(u8[i]), E.LAYOUT_NHWC, E.ptr(li8), B, Cn, S, S, P, E.ptr(o8), k_pad, st))
    torch.cuda.synchronize()
    assert torch.equal(o32, o8)
    # algorithmic bytes per launch: the input once, the patch matrix once (+ the 768-byte table)
    print(json.dumps({'mode': mode, 'reps': reps, 'bytes_fp32_kernel': B * Cn * S * S * 4 + B * 196 * k_pad,
                      'bytes_u8_kernel': B * Cn * S * S + B * 196 * k_pad + Cn * 256}))
    sys.exit(0)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else None
B = 256
mean, std, _ = D.MODEL_STATS['deit']
m = dva.deit_small_patch16_224(pretrained=False, cfg=dva.Config()).cuda().eval()
m.load_state_dict(dva.synth.vit_state_dict(dva.synth.ARCHS['deit_small'], 5), strict=False)
dva.harness.calibrate_model(m, dva.synth.images(5, 2, 224).cuda())
plan = m.freeze()
bc = [8] * 50
u8_host = dva.synth.images_uint8(5, 64, 224).repeat(4, 1, 1, 1).contiguous().pin_memory()
f32_host = D.normalize_uint8(u8_host, mean, std).contiguous().pin_memory()          # the same images, normalised on the host
u8_dev, f32_dev = u8_host.cuda(), f32_host.cuda()
lut = plan.input_lut(D.uint8_lut(mean, std))
out = torch.empty(B, 1000, device='cuda')
tgt = torch.zeros(B, dtype=torch.long).pin_memory()
fwd32 = lambda x: plan.forward_streams(x, bc, out, 3)
fwd8 = lambda x: plan.forward_uint8_streams(x, lut, bc, out, 'NHWC', 3)
for _ in range(5):                                   # the side streams are chosen here, before the copy stream exists
    fwd32(f32_dev); fwd8(u8_dev)
torch.cuda.synchronize()
assert torch.equal(fwd8(u8_dev).clone(), fwd32(f32_dev))                              # same logits


def resident(f, x):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f(x)
    torch.cuda.synchronize()
    return B * n / (time.perf_counter() - t0)


def host_fed(f, host):
    batches = [(host, tgt)] * n
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x, _ in dva.harness.DevicePrefetcher(batches, 'cuda'):
        f(x)
    torch.cuda.synchronize()
    return B * n / (time.perf_counter() - t0)


def copy_then_forward(f, host):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f(host.cuda(non_blocking=True))
        torch.cuda.synchronize()
    return B * n / (time.perf_counter() - t0)


def h2d(host):
    dst = torch.empty_like(host, device='cuda')
    dst.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        dst.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    return 10 * host.numel() * host.element_size() / (time.perf_counter() - t0) / 1e9


regimes = [('resident_fp32', lambda: resident(fwd32, f32_dev)), ('resident_uint8', lambda: resident(fwd8, u8_dev)),
           ('host_fed_fp32', lambda: host_fed(fwd32, f32_host)), ('host_fed_uint8', lambda: host_fed(fwd8, u8_host)),
           ('copy_then_forward_uint8', lambda: copy_then_forward(fwd8, u8_host))]
res = {k: [] for k, _ in regimes}
for r in range(rounds):
    for k, fn in regimes:
        res[k].append(fn())
gbs = {'h2d_fp32_GBps': h2d(f32_host), 'h2d_uint8_GBps': h2d(u8_host)}
best = {k: max(v) for k, v in res.items()}
lines = ['uint8 input, DeiT-S int8, batch 256, %d batches per pass, %d alternating rounds (img/s, best of rounds; all rounds listed)' % (n, rounds)]
for k, v in res.items():
    lines.append('  %-24s %9.0f   %s' % (k, best[k], ' '.join('%.0f' % x for x in v)))
lines.append('  host -> device copy of one batch: fp32 %.1f MB at %.1f GB/s, uint8 %.1f MB at %.1f GB/s' % (
    f32_host.numel() * 4 / 1e6, gbs['h2d_fp32_GBps'], u8_host.numel() / 1e6, gbs['h2d_uint8_GBps']))
lines.append('  host-fed uint8 / resident uint8: %.3f;  resident uint8 / resident fp32: %.3f;  host-fed uint8 / host-fed fp32: %.3f' % (
    best['host_fed_uint8'] / best['resident_uint8'], best['resident_uint8'] / best['resident_fp32'], best['host_fed_uint8'] / best['host_fed_fp32']))
txt = '\n'.join(lines)
print(txt)
print(json.dumps({'best_img_per_s': {k: round(v, 1) for k, v in best.items()}, **{k: round(v, 2) for k, v in gbs.items()}}))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, 'w').write(txt + '\n')
