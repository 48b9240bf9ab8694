"""GPU: randomized parity of the per-operator entry points against the oracle over odd shapes and extreme parameters.
python tools/fuzz_ops.py [SEED=0] [CASES=30] [--max-window W] [--only OP[,OP...]]
--max-window W (default 8, up to 12): the Swin window sizes also cycle through 9 .. W (the kernel for 65 .. 144 keys); the default case
stream is unchanged.  --only: run these operators' cases alone (ln, attn, gemm, winattn, ln_gemm), from a generator of their own."""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import diff_vit_amd as dva
import p2vit_oracle as O
E = dva.engine
L = E.lib()
MAX_WINDOW, ONLY = 8, None
for flag in ('--max-window', '--only'):
    if flag in sys.argv:
        at = sys.argv.index(flag)
        val = sys.argv[at + 1]
        del sys.argv[at:at + 2]
        if flag == '--max-window':
            MAX_WINDOW = int(val)
            assert 8 <= MAX_WINDOW <= 12, '--max-window takes 8 .. 12'
        else:
            ONLY = val.split(',')
            assert set(ONLY) <= {'ln', 'attn', 'gemm', 'winattn', 'ln_gemm'}, ONLY
WINDOWS = [7, 4, 8, 7, 2] + list(range(9, MAX_WINDOW + 1))
g = torch.Generator().manual_seed(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
fails = 0
stats = {'resid_tables': 0, 'resid_tables_usable': 0}


def rnd(*shape, std=1.0):
    return torch.randn(*shape, generator=g) * std


def ln_case(i):
    global fails
    C_ = int(torch.randint(1, 64, (1,), generator=g)) * 4 * int(torch.randint(1, 5, (1,), generator=g))
    C_ = min(C_, 1024)
    rows = int(torch.randint(1, 300, (1,), generator=g))
    codes = torch.clamp(torch.round(rnd(1, rows, C_, std=float(torch.rand(1, generator=g)) * 60 + 1)), -128, 127)
    if i % 5 == 0:
        codes[0, 0] = 7                       # zero-variance row: std = 0
    base = float(2.0 ** torch.randint(-9, 0, (1,), generator=g)) * (1.0 + 0.37 * (i % 3))
    in_scale = base * 2.0 ** torch.randint(0, 4, (C_,), generator=g).float()
    gamma = rnd(C_, std=1.0) * (10.0 ** float(torch.randint(-3, 2, (1,), generator=g)))
    if i % 4 == 1:
        gamma[::7] = 0.0
    if i % 4 == 2:
        gamma[3] = 1e-9
    beta = rnd(C_, std=0.5) * (100.0 if i % 6 == 3 else 1.0)
    cs = 2.0 ** torch.randint(-3, 3, (C_,), generator=g).float()
    s_a = float(2.0 ** torch.randint(-7, -1, (1,), generator=g))
    out_scale = s_a * cs * (1.0 if i % 7 else 1.3)      # sometimes NOT a power of two: generic chain
    ln = O.int_layernorm(codes * in_scale.reshape(1, 1, -1), in_scale, gamma, beta, out_scale)
    ref = torch.clamp(torch.round(ln * 1.0), -128, 127)[0]
    ref = torch.nan_to_num(ref, nan=0.0)
    s1 = in_scale.min()
    dev = [t.contiguous().cuda() for t in (codes[0].to(torch.int8), torch.round(in_scale / s1), gamma, beta, 1.0 / out_scale, torch.ones(C_))]
    os_dev = out_scale.contiguous().cuda()
    lnp = E.Ln(float(s1), *([E.ptr(t) for t in dev[1:]] + ([E.ptr(os_dev)] if i % 2 else [])))     # odd cases: exact division by the scale
    out = torch.zeros(rows, C_, dtype=torch.int8, device='cuda')
    E.check(L.p2v_int_layernorm(E.ptr(dev[0]), C_, rows, C_, C.byref(lnp), E.ptr(out), C_, E.stream_ptr()))
    got = out.cpu().float()
    # the same launch on constants folded ahead of it (p2v_ln_prefold, round 4): identical codes whatever the parameters
    nb = L.p2v_ln_prefold_bytes(C_)
    buf = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
    E.check(L.p2v_ln_prefold(C.byref(lnp), C_, E.ptr(buf), nb))
    out2 = torch.zeros(rows, C_, dtype=torch.int8, device='cuda')
    E.check(L.p2v_int_layernorm(E.ptr(dev[0]), C_, rows, C_, C.byref(lnp), E.ptr(out2), C_, E.stream_ptr()))
    finite = torch.isfinite(ln[0]).all(dim=1)            # rows with std == 0 give inf/nan in the reference: not compared
    if not torch.equal(out2.cpu()[finite], out.cpu()[finite]):
        fails += 1
        print('LN case %d C=%d rows=%d: pre-folded constants give %d other codes' % (i, C_, rows, int((out2.cpu()[finite] != out.cpu()[finite]).sum())))
    bad = int((got[finite] != ref[finite]).sum())
    if bad and i % 7 == 0 and i % 2 == 0:
        # non power-of-two output scale: the ABI takes 1/out_scale and multiplies where the reference divides (exact only for
        # powers of two, the P2-ViT case; include/p2vit.h): a multiplier on a dyadic boundary may land one step away
        if bad <= max(1, int(1e-4 * got[finite].numel())):       # one 8-bit multiplier off by one step: |diff| <= |x_q| / 2^N + 1
            bad = 0
    if bad:
        fails += 1
        print('LN case %d C=%d rows=%d: %d mismatches' % (i, C_, rows, bad))
        idx = ((got != ref) & finite.unsqueeze(1)).nonzero()
        for r_, c_ in idx[:4].tolist():
            xq = (codes[0, r_] * torch.round(in_scale / s1)).double()
            n = C_
            S1, S2 = xq.sum().float(), (xq * xq).sum().float()
            std = (s1 / n) * torch.sqrt((n * S2 - S1 * S1).double()).float()
            A = (s1 / std) * gamma[c_] / out_scale[c_]
            print('   row %d col %d got %g want %g | ln %.6f gamma %.6g beta %.6g out_scale %.6g A %.6g code %g mask %g' %
                  (r_, c_, float(got[r_, c_]), float(ref[r_, c_]), float(ln[0, r_, c_]), float(gamma[c_]), float(beta[c_]), float(out_scale[c_]),
                   float(A), float(codes[0, r_, c_]), float(torch.round(in_scale / s1)[c_])))



def ln_gemm_case(i):
    """p2v_ln_gemm_i8 against p2v_int_layernorm + p2v_gemm_i8 (bit-identical by contract) over random widths, rows and epilogues."""
    global fails
    C_ = int(torch.randint(1, 97, (1,), generator=g)) * 4                      # 4 .. 384
    N = int(torch.randint(1, 97, (1,), generator=g)) * 16                      # 16 .. 1536
    M = int(torch.randint(1, 400, (1,), generator=g))
    kind = E.EPI_GELU if i % 2 else E.EPI_REQUANT
    codes = torch.clamp(torch.round(rnd(M, C_, std=float(torch.rand(1, generator=g)) * 60 + 1)), -128, 127)
    in_scale = float(2.0 ** torch.randint(-9, 0, (1,), generator=g)) * 2.0 ** torch.randint(0, 4, (C_,), generator=g).float()
    gamma = rnd(C_, std=1.0); beta = rnd(C_, std=0.5)
    if i % 4 == 1:
        gamma[::5] = 0.0
    cs = 2.0 ** torch.randint(-2, 3, (C_,), generator=g).float()
    s_a = float(2.0 ** torch.randint(-6, -2, (1,), generator=g))
    out_scale = s_a * cs * (1.0 if i % 5 else 1.3)                             # sometimes the generic LayerNorm chain
    post = out_scale / cs / s_a if i % 5 else torch.ones(C_)
    s1 = in_scale.min()
    k_pad, n_pad = (C_ + 63) // 64 * 64, (N + 127) // 128 * 128
    wp = torch.zeros(n_pad, k_pad, dtype=torch.int8)
    wp[:N, :C_] = torch.clamp(torch.round(rnd(N, C_, std=30.0)), -128, 127).to(torch.int8)
    csl = torch.zeros(n_pad); csl[:N] = s_a * 2.0 ** torch.randint(-8, -5, (N,), generator=g).float()
    bp = torch.zeros(n_pad); bp[:N] = rnd(N, std=0.4)
    d = [t.contiguous().cuda() for t in (codes.to(torch.int8), torch.round(in_scale / s1), gamma, beta, 1.0 / out_scale, post, wp, csl, bp)]
    lnp = E.Ln(float(s1), *[E.ptr(t) for t in d[1:6]])
    wfrag = E.fragment_order(wp).cuda()
    lin = E.Linear(E.ptr(d[6]), E.ptr(d[7]), E.ptr(d[8]), E.ptr(wfrag))
    epi = E.Epilogue()
    inv_s = float(2.0 ** torch.randint(3, 6, (1,), generator=g))
    epi.inv_s_out = inv_s
    if kind == E.EPI_GELU and i % 4 != 3:
        epi.gelu = E.gelu_table(inv_s, 'cuda')
    cells = epi.gelu.cells if epi.gelu.table else 0
    if L.p2v_ln_gemm_fusable(kind, C_, N, cells) != 1:
        return
    ln_sep = torch.zeros(M, k_pad, dtype=torch.int8, device='cuda')
    E.check(L.p2v_int_layernorm(E.ptr(d[0]), C_, M, C_, C.byref(lnp), E.ptr(ln_sep), k_pad, E.stream_ptr()))
    out_sep = torch.zeros(M, N, dtype=torch.int8, device='cuda')
    E.check(L.p2v_gemm_i8(kind, E.ptr(ln_sep), k_pad, M, k_pad, N, C.byref(lin), C.byref(epi), E.ptr(out_sep), N, None, E.stream_ptr()))
    out_f = torch.full((M, N), 77, dtype=torch.int8, device='cuda')
    ln_f = torch.full((M, C_), 99, dtype=torch.int8, device='cuda')
    E.check(L.p2v_ln_gemm_i8(kind, E.ptr(d[0]), C_, M, C_, C.byref(lnp), N, C.byref(lin), C.byref(epi), E.ptr(out_f), N, E.ptr(ln_f), E.stream_ptr()))
    torch.cuda.synchronize()
    finite = torch.isfinite(O.int_layernorm(codes.unsqueeze(0) * in_scale.reshape(1, 1, -1), in_scale, gamma, beta, out_scale)[0]).all(dim=1).cuda()
    bad = int((out_f[finite] != out_sep[finite]).sum()) + int((ln_f[finite] != ln_sep[finite][:, :C_]).sum())
    if bad:
        fails += 1
        print('LN+GEMM case %d C=%d N=%d M=%d kind=%d: %d mismatches' % (i, C_, N, M, kind, bad))
    # ... and on LayerNorm constants folded ahead of the launch (p2v_ln_prefold): the same codes
    nb = L.p2v_ln_prefold_bytes(C_)
    buf = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
    E.check(L.p2v_ln_prefold(C.byref(lnp), C_, E.ptr(buf), nb))
    out2 = torch.zeros(M, N, dtype=torch.int8, device='cuda')
    E.check(L.p2v_ln_gemm_i8(kind, E.ptr(d[0]), C_, M, C_, C.byref(lnp), N, C.byref(lin), C.byref(epi), E.ptr(out2), N, None, E.stream_ptr()))
    if not torch.equal(out2[finite], out_f[finite]):
        fails += 1
        print('LN+GEMM case %d C=%d N=%d M=%d kind=%d: pre-folded LayerNorm constants give %d other codes' % (i, C_, N, M, kind, int((out2[finite] != out_f[finite]).sum())))


def attn_case(i):
    global fails
    hd = [32, 64, 48, 80, 96, 128][i % 6]             # every instantiated head dimension (two 64-deep MFMA steps per score from 80 on)
    H = int(torch.randint(1, 5, (1,), generator=g))
    N = [197, 50, 17, 33, 64, 650, 401][i % 7]      # 650 (and 401 at head_dim 128): beyond the resident kernel - the streaming one
    B = int(torch.randint(1, 4, (1,), generator=g))
    D = H * hd
    qkv = torch.clamp(torch.round(rnd(B, N, 3 * D, std=float(torch.rand(1, generator=g)) * 70 + 0.5)), -128, 127)
    if i % 3 == 0:
        qkv[0, :, :D] = 0
    e_q, e_at, e_a2 = int(torch.randint(2, 7, (1,), generator=g)), int(torch.randint(2, 9, (1,), generator=g)), int(torch.randint(1, 6, (1,), generator=g))
    s_q1, s_at, s_a2 = 2.0 ** -e_q, 2.0 ** -e_at, 2.0 ** -e_a2
    t = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    acc = t[0] @ t[1].transpose(-2, -1)
    scale = float(np.float32(hd ** -0.5))
    sc = torch.clamp(torch.round(((acc * (s_q1 * s_q1)) * scale) / s_at), -128, 127)
    k = O.lis_int(sc, torch.tensor([s_at]))
    o = (O.lis_probs(k) @ (t[2] * s_q1)).transpose(1, 2).reshape(B, N, D)
    ref = torch.clamp(torch.round(o / s_a2), -128, 127)
    x0, bb, cc = O.lis_consts(torch.tensor([s_at]))
    at = E.Attn(s_q1 * s_q1, scale, 1.0 / s_at, s_q1 / s_a2, x0, bb, cc)
    dq = qkv.to(torch.int8).cuda()
    out = torch.zeros(B * N, D, dtype=torch.int8, device='cuda')
    pk = torch.full((B, H, N, N), -1, dtype=torch.int8, device='cuda')
    E.check(L.p2v_lis_attention(E.ptr(dq), B, N, H, hd, C.byref(at), E.ptr(out), E.ptr(pk), E.stream_ptr()))
    b1, b2 = int((pk.cpu().long() != k).sum()), int((out.cpu().float().reshape(B, N, D) != ref).sum())
    if b1 or b2:
        fails += 1
        print('attention case %d B=%d N=%d H=%d hd=%d s_at=2^-%d: k mismatches %d, out mismatches %d' % (i, B, N, H, hd, e_at, b1, b2))


def gemm_case(i):
    global fails
    M = int(torch.randint(1, 700, (1,), generator=g))
    K = 64 * int(torch.randint(1, 25, (1,), generator=g))
    N = 16 * int(torch.randint(1, 40, (1,), generator=g))
    x = torch.clamp(torch.round(rnd(M, K, std=50)), -128, 127)
    w = torch.clamp(torch.round(rnd(N, K, std=40)), -128, 127)
    bias = rnd(N, std=0.5)
    s_x = float(2.0 ** torch.randint(-8, -2, (1,), generator=g))
    s_w = 2.0 ** torch.randint(-10, -4, (N,), generator=g).float()
    n_pad = (N + 127) // 128 * 128
    wp = torch.zeros(n_pad, K, dtype=torch.int8); wp[:N] = w.to(torch.int8)
    cs = torch.zeros(n_pad); cs[:N] = s_x * s_w
    bp = torch.zeros(n_pad); bp[:N] = bias
    dev = [t_.cuda() for t_ in (x.to(torch.int8), wp, cs, bp)]
    lin = E.Linear(E.ptr(dev[1]), E.ptr(dev[2]), E.ptr(dev[3]))
    y = O.qgemm(x, torch.tensor(s_x), w, s_w, bias)
    ymax = float(y.abs().max())
    s_out = float(2.0 ** np.ceil(np.log2(max(ymax, 1e-3) / 100.0)))
    for kind in (E.EPI_REQUANT, E.EPI_GELU):
        epi = E.Epilogue(); epi.inv_s_out = 1.0 / s_out
        out = torch.zeros(M, N, dtype=torch.int8, device='cuda')
        E.check(L.p2v_gemm_i8(kind, E.ptr(dev[0]), K, M, K, N, C.byref(lin), C.byref(epi), E.ptr(out), N, None, E.stream_ptr()))
        v = O.gelu_rn(y) if kind == E.EPI_GELU else y
        ref = torch.clamp(torch.round(v / s_out), -128, 127)
        bad = int((out.cpu().float() != ref).sum())
        if bad:
            fails += 1
            print('gemm case %d kind %d M=%d K=%d N=%d: %d mismatches' % (i, kind, M, K, N, bad))
    # residual epilogue with non power-of-two PTF scales
    res = torch.clamp(torch.round(rnd(M, N, std=50)), -128, 127)
    s_mid = (0.011 + 0.02 * torch.rand(N, generator=g)) * s_out * 8
    s_res = (0.013 + 0.02 * torch.rand(N, generator=g)) * 2.0 ** torch.randint(0, 4, (N,), generator=g).float() * s_out * 4
    s_next = (0.017 + 0.02 * torch.rand(N, generator=g)) * 2.0 ** torch.randint(0, 4, (N,), generator=g).float() * s_out * 4
    def padv(v):
        o_ = torch.ones(n_pad); o_[:N] = v; return o_.cuda()
    dv = [padv(s_mid), padv(s_res), padv(s_next), res.to(torch.int8).cuda()]
    epi = E.Epilogue()
    epi.s_mid, epi.s_res, epi.s_next, epi.residual = [E.ptr(t_) for t_ in dv]
    out = torch.zeros(M, N, dtype=torch.int8, device='cuda')
    E.check(L.p2v_gemm_i8(E.EPI_RESID, E.ptr(dev[0]), K, M, K, N, C.byref(lin), C.byref(epi), E.ptr(out), N, None, E.stream_ptr()))
    q3 = torch.clamp(torch.round(y / s_mid), -128, 127)
    ref = torch.clamp(torch.round((res * s_res + q3 * s_mid) / s_next), -128, 127)
    bad = int((out.cpu().float() != ref).sum())
    if bad:
        fails += 1
        print('gemm RESID case %d M=%d K=%d N=%d: %d mismatches' % (i, M, K, N, bad))
    # the same launch on the constants of p2v_resid_prefold (round 4): when the device certifies the table, identical codes
    nb = L.p2v_resid_prefold_bytes(N)
    tab = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
    usable = C.c_int(-1)
    E.check(L.p2v_resid_prefold(C.byref(lin), C.byref(epi), N, E.ptr(tab), nb, C.byref(usable), None))
    stats['resid_tables'] += 1
    if usable.value == 1:
        stats['resid_tables_usable'] += 1
        epi.resid_tab = E.ptr(tab)
        out2 = torch.zeros(M, N, dtype=torch.int8, device='cuda')
        E.check(L.p2v_gemm_i8(E.EPI_RESID, E.ptr(dev[0]), K, M, K, N, C.byref(lin), C.byref(epi), E.ptr(out2), N, None, E.stream_ptr()))
        bad = int((out2.cpu().float() != ref).sum())
        if bad:
            fails += 1
            print('gemm RESID (pre-folded) case %d M=%d K=%d N=%d: %d mismatches' % (i, M, K, N, bad))


def winattn_case(i):
    global fails
    import swin_oracle as SO
    ws = WINDOWS[i % len(WINDOWS)]
    mult = int(torch.randint(1, 4, (1,), generator=g))
    Hf = ws * mult
    shift = 0 if (mult == 1 or i % 2 == 0) else int(torch.randint(1, ws, (1,), generator=g))
    heads = int(torch.randint(1, 9, (1,), generator=g))
    B = int(torch.randint(1, 4, (1,), generator=g))
    C_, T, N = heads * 32, Hf * Hf, ws * ws
    qkv = torch.clamp(torch.round(rnd(B, T, 3 * C_, std=float(torch.rand(1, generator=g)) * 60 + 0.5)), -128, 127)
    tab = torch.clamp(torch.round(rnd((2 * ws - 1) ** 2, heads, std=40.0)), -128, 127)
    c = dict(qact1=float(2.0 ** -int(torch.randint(2, 7, (1,), generator=g))), qact_attn1=float(2.0 ** -int(torch.randint(1, 7, (1,), generator=g))),
             qact_table=float(2.0 ** -int(torch.randint(2, 8, (1,), generator=g))), qact2=float(2.0 ** -int(torch.randint(1, 7, (1,), generator=g))),
             qact3=float(2.0 ** -int(torch.randint(1, 6, (1,), generator=g))))
    idx = SO.window_index(Hf, Hf, ws, shift)
    nW = idx.shape[0]
    mask = region = None
    if shift:
        mask = SO.shifted_window_mask(Hf, Hf, ws, shift)
        region = dva.swin.shifted_window_regions(Hf, Hf, ws, shift)
    x0, bb, cc = O.lis_consts(torch.tensor([c['qact2']]))
    dev = dict(qkv=qkv.to(torch.int8).contiguous().cuda(), tab=tab.to(torch.int8).contiguous().cuda(), idx=idx.to(torch.int32).contiguous().cuda(),
               reg=None if region is None else region.to(torch.int8).contiguous().cuda())
    wa = E.WinAttn(c['qact1'], float(np.float32(32 ** -0.5)), c['qact_attn1'], c['qact_table'], c['qact2'], c['qact3'], x0, bb, cc,
                   E.ptr(dev['tab']), E.ptr(dev['idx']), E.ptr(dev['reg']) if dev['reg'] is not None else None, ws, nW, 0, 0)
    out = torch.zeros(B * T, C_, dtype=torch.int8, device='cuda')
    pk = torch.full((B, nW, heads, N, N), -1, dtype=torch.int8, device='cuda')
    E.check(L.p2v_window_attention(E.ptr(dev['qkv']), B, T, heads, 32, C.byref(wa), E.ptr(out), E.ptr(pk), E.stream_ptr()))
    out_nt = torch.zeros(B * T, C_, dtype=torch.int8, device='cuda')       # the instantiation without the tap stores
    E.check(L.p2v_window_attention(E.ptr(dev['qkv']), B, T, heads, 32, C.byref(wa), E.ptr(out_nt), None, E.stream_ptr()))
    if not torch.equal(out_nt, out):
        fails += 1
        print('window attention case %d: output with and without taps differs' % i)
    xw = qkv[:, idx.reshape(-1)].reshape(B * nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s1 = torch.tensor(c['qact1'])
    qs = (xw[0] * s1) * torch.tensor(32 ** -0.5, dtype=torch.float32)
    attn = (qs.double() @ (xw[1] * s1).double().transpose(-2, -1)).float()
    a1 = SO.q8(attn, c['qact_attn1'])
    bias = (tab * c['qact_table'])[SO.relative_position_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    a2 = SO.q8(a1 * c['qact_attn1'] + bias.unsqueeze(0), c['qact2'])
    xi = a2
    if mask is not None:
        xi = (a2.reshape(B, nW, heads, N, N) + torch.round(mask / c['qact2']).unsqueeze(1).unsqueeze(0)).reshape(B * nW, heads, N, N)
    k = O.lis_int(xi, torch.tensor([c['qact2']]))
    o = (O.lis_probs(k) @ (xw[2] * s1)).transpose(1, 2).reshape(B, nW * N, C_)
    q3 = SO.q8(o, c['qact3'])
    want = torch.zeros(B, T, C_)
    want[:, idx.reshape(-1)] = q3
    b1 = int((pk.cpu().long().reshape(B * nW, heads, N, N) != k.long()).sum())
    b2 = int((out.cpu().float().reshape(B, T, C_) != want).sum())
    if b1 or b2:
        fails += 1
        print('window attention case %d ws=%d Hf=%d shift=%d heads=%d B=%d scales %s: k mismatches %d, out mismatches %d' % (i, ws, Hf, shift, heads, B, c, b1, b2))


n = int(sys.argv[2]) if len(sys.argv) > 2 else 30
for i in range(n):
    for name, case in (('ln', ln_case), ('attn', attn_case), ('gemm', gemm_case), ('winattn', winattn_case), ('ln_gemm', ln_gemm_case)):
        if ONLY is None or name in ONLY:
            case(i)
torch.cuda.synchronize()
print('fuzz: %d cases per op, %d failing; pre-folded RESID tables certified %d of %d' % (n, fails, stats['resid_tables_usable'], stats['resid_tables']))
sys.exit(1 if fails else 0)
