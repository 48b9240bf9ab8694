"""Few-rows GEMM kernel against the tiled kernel, stand-alone launch times (p2v_gemm_i8, "gemm_rows" 1 against 2):
    python tools/bench_gemm_rows.py [M ...]
RESID (pre-folded table) at (K, N) = (384, 384) and (1536, 384), GELU (table) at (384, 1536); microseconds per launch over 200 back-to-back
launches between two HIP events (launch gaps included: the same for both kernels)."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import diff_vit_amd as dva  # noqa: E402

E = dva.engine
L = E.lib()


def layer(K, N, M, resid):
    g = torch.Generator().manual_seed(K + N)
    w = torch.randint(-100, 101, (N, K), generator=g, dtype=torch.int8).cuda()
    cs, b = torch.full((N,), 2.0 ** -13).cuda(), (torch.randn(N, generator=g) * 0.4).cuda()
    lin = E.Linear(E.ptr(w), E.ptr(cs), E.ptr(b))
    epi = E.Epilogue()
    keep = [w, cs, b]
    x = torch.randint(-100, 101, (M, K), generator=g, dtype=torch.int8).cuda()
    out = torch.randint(-100, 101, (M, N), generator=g, dtype=torch.int8).cuda()
    if resid:
        sc = [torch.full((N,), v).cuda() for v in (0.0131, 0.0173, 0.0209)]
        epi.s_mid, epi.s_res, epi.s_next, epi.residual = E.ptr(sc[0]), E.ptr(sc[1]), E.ptr(sc[2]), E.ptr(out)
        nb = L.p2v_resid_prefold_bytes(N)
        tab = torch.empty(nb // 4, device='cuda')
        ok = C.c_int(0)
        E.check(L.p2v_resid_prefold(C.byref(lin), C.byref(epi), N, E.ptr(tab), nb, C.byref(ok), None))
        if ok.value:
            epi.resid_tab = E.ptr(tab)
        keep += sc + [tab]
        kind = E.EPI_RESID
    else:
        epi.inv_s_out = 32.0
        epi.gelu = E.gelu_table(32.0, 'cuda')
        kind = E.EPI_GELU
    return lambda: E.check(L.p2v_gemm_i8(kind, E.ptr(x), K, M, K, N, C.byref(lin), C.byref(epi), E.ptr(out), N, None, E.stream_ptr())), keep


def us_per_launch(fn, n=200):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / n)
    return best


def main():
    ms = [int(v) for v in sys.argv[1:]] or [16, 68, 128, 256, 512, 1024]
    print('%-22s %6s %10s %10s' % ('shape (epilogue)', 'M', 'rows us', 'tiled us'))
    for K, N, resid in ((384, 384, True), (1536, 384, True), (384, 1536, False)):
        for M in ms:
            fn, keep = layer(K, N, M, resid)
            t = []
            try:
                for sw in (1, 2):
                    assert L.p2v_set_tuning(b'gemm_rows', sw) == 0
                    t.append(us_per_launch(fn))
            finally:
                L.p2v_set_tuning(b'gemm_rows', 0)
            print('%-22s %6d %10.2f %10.2f' % ('K=%d N=%d %s' % (K, N, 'RESID' if resid else 'GELU'), M, t[0], t[1]))


if __name__ == '__main__':
    main()
