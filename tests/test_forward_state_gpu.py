"""GPU: the whole-model entry points (p2v_forward, p2v_forward_u8, p2v_forward_taps, p2v_forward_linear_taps, p2v_forward_ddv) as a
caller sees them: what they need from the workspace on entry (nothing), what they write (the workspace buffers launch by launch, the dense
outputs, and no other byte) and what a workspace that has served other batch sizes, bit lists and entry points does to the next result
(nothing).  Through ctypes, every output operand in a sentinel arena (tests/_arena.py): the workspace of exactly p2v_workspace_bytes /
p2v_ddv_workspace_bytes bytes on a 256-byte boundary, the logits, every tap buffer at its tap_shapes extent, the fp64 sums, the DDV tap
scratch.  Fills: the two sentinels of _arena.py and 0x80 (-128 as a code, -0.0-like patterns as fp32).

Few tokens: 2, 5 and 10 tokens per image put several images into one 16-row query block of the attention kernel and into one row of
class-token GEMM tiles; against oracle.OracleViT.  Every comparison is bit equality."""
import ctypes as C
import math
from functools import partial

import numpy as np
import pytest
import torch

from _arena import SENTINELS, Arena
from _tuning import tuning
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

FILLS = SENTINELS + (0x80,)


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


@pytest.fixture(scope='module')
def plan(dva, micro):
    return dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])


def _sync():
    torch.cuda.synchronize()


def _cfg(bits):
    return (C.c_int8 * len(bits))(*[int(b) for b in bits])


def _bits(g, tag, L):
    return {'q8': [8] * L, 'q4': [4] * L, 'qmix': [int(b) for b in g['bit_qmix']]}[tag]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.contiguous().numpy().view(np.uint8), b.contiguous().numpy().view(np.uint8))


def _ws_arena(E, pl, batch, fill, ddv_pairs=0):
    L = E.lib()
    nb = L.p2v_ddv_workspace_bytes(pl._handle, ddv_pairs) if ddv_pairs else L.p2v_workspace_bytes(pl._handle, batch)
    assert nb > 0
    return Arena(1, nb, None, torch.uint8, fill, offset=0)


def _forward(E, pl, x, bits, fill, stop_after=-1, ws=None, u8=None):
    """p2v_forward on fp32 images x (device), or p2v_forward_u8 with u8 = (uint8 images on the device, layout, int8 table on the device)
    -> (logits [B][classes], the workspace's bytes); guards of both arenas checked.  ws: an arena to reuse (its whole width is offered)"""
    L = E.lib()
    B = (x if u8 is None else u8[0]).shape[0]
    ws = _ws_arena(E, pl, B, fill) if ws is None else ws
    out = Arena(B, pl.arch['num_classes'], None, torch.float32, fill)
    if u8 is None:
        E.check(L.p2v_forward(pl._handle, E.ptr(x), B, _cfg(bits), len(bits), out.ptr, ws.ptr, ws.width, stop_after, E.stream_ptr()))
    else:
        E.check(L.p2v_forward_u8(pl._handle, E.ptr(u8[0]), E.LAYOUTS[u8[1]], E.ptr(u8[2]), B, _cfg(bits), len(bits), out.ptr, ws.ptr, ws.width,
                                 stop_after, E.stream_ptr()))
    _sync()
    what = ('forward', B, bits[:3], hex(fill), stop_after, None if u8 is None else u8[1])
    wsb = ws.read(('workspace',) + what).numpy().reshape(-1)
    return out.read(('logits',) + what), wsb


def _u8_input(pl, x):
    """uint8 images and a table that reproduce the fp32 batch x exactly: the image bytes are the input codes + 128, the table maps them
    back (the kernels only gather through the table, include/p2vit.h) -> {layout: (images on the device, layout, table on the device)}"""
    inv_s = float(pl.inv_s_input)
    assert inv_s > 0 and math.frexp(inv_s)[0] == 0.5                       # a power of two: x * inv_s is exact
    q = torch.clamp(torch.round(x * inv_s), -128, 127)
    nchw = (q + 128).to(torch.uint8)
    lut = (torch.arange(256) - 128).to(torch.int8).reshape(1, 256).repeat(x.shape[1], 1).contiguous().cuda()
    return {'NCHW': (nchw.contiguous().cuda(), 'NCHW', lut), 'NHWC': (nchw.permute(0, 2, 3, 1).contiguous().cuda(), 'NHWC', lut)}


# --------------------------------------------------------------------------------------------------
# a. the micro model against the fixture, inside arenas
# --------------------------------------------------------------------------------------------------
SWITCHES = [dict(), dict(cls_rows=0), dict(ln_gemm=0), dict(attn_stream=1), dict(gemm_rows=2)]


@pytest.mark.parametrize('switch', SWITCHES, ids=lambda s: '-'.join('%s=%d' % kv for kv in s.items()) or 'default')
def test_micro_fixture_in_arenas(dva, micro, plan, switch):
    """p2v_forward and p2v_forward_u8 (both layouts) on the fixture's evaluation batch, q8 / q4 / qmix: the logits equal the fixture's bit
    for bit under each of the three fills of workspace and logits arena, no guard byte changes (checked in _forward)"""
    E = dva.engine
    g = micro['g']
    x = micro['x_ev'].cuda()
    u8 = _u8_input(plan, micro['x_ev'])
    with tuning(E.lib(), **switch):
        for tag in ('q8', 'q4', 'qmix'):
            bits = _bits(g, tag, plan.n_layers)
            ref = torch.from_numpy(g['logits/' + tag])
            for entry in (None, 'NHWC', 'NCHW'):
                for fill in FILLS:
                    out, _ = _forward(E, plan, x, bits, fill, u8=None if entry is None else u8[entry])
                    assert _same_bits(out, ref), (switch, tag, entry, hex(fill), int((out != ref).sum()))


# --------------------------------------------------------------------------------------------------
# b. the write map, launch by launch
# --------------------------------------------------------------------------------------------------
class Map:
    """the seven workspace buffers of a plan at one batch size as boolean masks over the workspace's bytes"""

    def __init__(self, E, pl, batch):
        L = E.lib()
        a = pl.arch
        self.B, self.T, self.D, self.Hd = batch, pl.tokens, pl.D, pl.hidden
        self.nbytes = L.p2v_workspace_bytes(pl._handle, batch)
        k_pad = (pl.in_chans * a['patch_size'] ** 2 + 63) // 64 * 64
        M = batch * pl.tokens
        self.shape = dict(patches=(batch * pl.patches, k_pad), x=(M, pl.D), ln=(M, pl.D), qkv=(M, 3 * pl.D), att=(M, pl.D), hid=(M, pl.hidden),
                          cls=(batch, pl.D))
        self.off = {k: int(L.p2v_workspace_view(pl._handle, batch, k.encode())) for k in self.shape}
        assert min(self.off.values()) == 0 and all(o % 256 == 0 for o in self.off.values())

    def mask(self, name, rows=None):
        """the bytes of `rows` (default: all) of buffer `name`"""
        r, c = self.shape[name]
        m = np.zeros(self.nbytes, dtype=bool)
        if rows is None:
            m[self.off[name]: self.off[name] + r * c] = True
        else:
            rows = np.asarray(rows, dtype=np.int64)
            assert rows.min() >= 0 and rows.max() < r
            m[(self.off[name] + rows[:, None] * c + np.arange(c, dtype=np.int64)[None, :]).reshape(-1)] = True
        return m

    def class_rows(self):
        return np.arange(self.B) * self.T

    def patch_rows(self):
        return np.setdiff1d(np.arange(self.B * self.T), self.class_rows())

    def covered(self):
        m = np.zeros(self.nbytes, dtype=bool)
        for k in self.shape:
            m |= self.mask(k)
        return m

    def targets(self, kinds):
        """per launch: the masks of what its kind writes (p2v_forward_profile's kind_out; the last LayerNorm is the final norm -> cls)"""
        last_ln = max(i for i, k in enumerate(kinds) if k == 'layernorm')
        table = dict(patchify=[('patches', None)], gemm_embed=[('x', self.patch_rows())], fill_cls=[('x', self.class_rows())],
                     layernorm=[('ln', None)], gemm_qkv=[('qkv', None)], attention=[('att', None)], gemm_proj=[('x', None)],
                     gemm_fc1=[('hid', None)], gemm_fc2=[('x', None)], gemm_head=[], ln_gemm_qkv=[('ln', None), ('qkv', None)],
                     ln_gemm_fc1=[('ln', None), ('hid', None)])
        return [[self.mask(*t) for t in ([('cls', None)] if i == last_ln else table[k])] for i, k in enumerate(kinds)]


@pytest.mark.parametrize('ln_gemm', [0, 1])
def test_write_map_launch_by_launch(dva, micro, plan, ln_gemm):
    """stop_after = s and s + (slots of launch k) on workspaces filled alike: the bytes that differ are launch k's writes.  They lie inside
    the buffer(s) its kind writes, at the rows x cols extent of p2v_workspace_view; where that target held only the fill before, the
    writes seen under the two sentinels together are that extent exactly (a written byte can equal one sentinel, not both).  ln_gemm = 0:
    every slot is one launch; ln_gemm = 1: a fused launch fills two slots and writes ln as well as qkv / hid.  Then, after a full
    stop_after = -1 run in both cls_rows settings, the alignment gaps between the buffers and the trailing 256 bytes still hold the
    fill, and the two settings differ only in x / att / hid / ln (include/p2vit.h, "cls_rows"), never in the class rows of x or att, nor in
    the logits."""
    E = dva.engine
    L = E.lib()
    x = micro['x_ev'].cuda()
    B = x.shape[0]
    bits = _bits(micro['g'], 'qmix', plan.n_layers)
    mp = Map(E, plan, B)
    with tuning(L, ln_gemm=ln_gemm):
        with tuning(L, cls_rows=0):                             # the launch list of the stop_after >= 0 runs: every row of the last block
            kinds = [k for k, _ in plan.profile(x, bits)]
        assert kinds[-1] == 'event_gap'
        kinds = kinds[:-1]
        fused = [k.startswith('ln_gemm') for k in kinds]
        assert any(fused) == bool(ln_gemm) and kinds[:3] == ['patchify', 'gemm_embed', 'fill_cls'] and kinds[-1] == 'gemm_head'
        stops = np.concatenate([[0], np.cumsum([2 if f else 1 for f in fused])])
        assert stops[-1] == 3 + 7 * plan.depth + 2
        targets = mp.targets(kinds)
        seen = [[np.zeros(mp.nbytes, dtype=bool) for _ in t] for t in targets]
        fresh = []
        for fill in SENTINELS:
            snaps = [_forward(E, plan, x, bits, fill, stop_after=int(s))[1] for s in stops]
            assert bool((snaps[0] == fill).all())
            fr = []
            for k, kind in enumerate(kinds):
                changed = snaps[k] != snaps[k + 1]
                allowed = np.zeros(mp.nbytes, dtype=bool)
                for t in targets[k]:
                    allowed |= t
                stray = np.nonzero(changed & ~allowed)[0]
                assert stray.size == 0, (k, kind, hex(fill), 'bytes outside the target changed', stray[:8].tolist())
                assert kind == 'gemm_head' or changed.any(), (k, kind)
                fr.append([bool((snaps[k][t] == fill).all()) for t in targets[k]])
                for s_, t in zip(seen[k], targets[k]):
                    s_ |= changed & t
            fresh.append(fr)
        assert fresh[0] == fresh[1]
        first = {}
        for k, kind in enumerate(kinds):
            for j, t in enumerate(targets[k]):
                if fresh[0][k][j]:
                    assert np.array_equal(seen[k][j], t), (k, kind, j, 'a fresh target was not written at its exact extent', int((seen[k][j] != t).sum()))
                    first[(kind, j)] = first.get((kind, j), 0) + 1
        assert sum(first.values()) == 8, first        # patches, the patch and the class rows of x, ln, qkv, att, hid, cls: each met fresh once
        # full runs: gaps, tail, and cls_rows = 1 against 0
        covered = mp.covered()
        assert int((~covered).sum()) > 256, 'this batch leaves no alignment gap: take another'
        for fill in SENTINELS:
            res = {}
            for cr in (1, 0):
                with tuning(L, cls_rows=cr):
                    res[cr] = _forward(E, plan, x, bits, fill)
                assert bool((res[cr][1][~covered] == fill).all()), (cr, hex(fill), 'a gap or the tail was written')
            assert _same_bits(res[1][0], res[0][0])
            may = mp.mask('x', mp.patch_rows()) | mp.mask('att', mp.patch_rows()) | mp.mask('hid') | mp.mask('ln')
            diff = res[1][1] != res[0][1]
            assert not (diff & ~may).any(), np.nonzero(diff & ~may)[0][:8].tolist()
            assert diff.any()                                                  # the class-row branch did leave rows stale


# --------------------------------------------------------------------------------------------------
# c. history, d. taps and DDV
# --------------------------------------------------------------------------------------------------
def _ddv(E, pl, x2n, bits, fill, with_linear, ws=None):
    """p2v_forward_ddv -> (logits, sums [stages][n][3]); workspace of exactly p2v_ddv_workspace_bytes, logits, sums and the tap scratch in arenas"""
    L = E.lib()
    n = x2n.shape[0] // 2
    ws = _ws_arena(E, pl, 2 * n, fill, ddv_pairs=n) if ws is None else ws
    stages = L.p2v_ddv_stage_count(pl._handle, int(with_linear))
    out = Arena(2 * n, pl.arch['num_classes'], None, torch.float32, fill)
    sums = Arena(stages * n, 3, None, torch.float64, fill)
    tb = L.p2v_ddv_tap_scratch_bytes(pl._handle, n)
    tap = Arena(1, tb, None, torch.uint8, fill) if with_linear else None
    E.check(L.p2v_forward_ddv(pl._handle, E.ptr(x2n), n, _cfg(bits), len(bits), out.ptr, ws.ptr, ws.width, int(with_linear),
                              tap.ptr if tap else None, tb if tap else 0, sums.ptr, E.stream_ptr()))
    _sync()
    what = ('forward_ddv', n, with_linear, hex(fill))
    ws.read(('workspace',) + what)
    if tap:
        tap.read(('tap scratch',) + what)
    return out.read(('logits',) + what), sums.read(('sums',) + what).reshape(stages, n, 3)


def test_workspace_history_does_not_reach_a_result(dva, micro, plan):
    """ONE workspace, sized for the largest call and filled once, serves B = 4 q8, B = 1 qmix, B = 3 q4, B = 4 q8, p2v_forward_ddv of 2
    pairs, B = 4 q8: every result equals the one from a fresh arena"""
    E = dva.engine
    L = E.lib()
    g = micro['g']
    xs = micro['x_ev'].cuda()
    bit = {t: _bits(g, t, plan.n_layers) for t in ('q8', 'q4', 'qmix')}
    for fill in SENTINELS:
        nb = max(L.p2v_workspace_bytes(plan._handle, 4), L.p2v_ddv_workspace_bytes(plan._handle, 2))
        ws = Arena(1, nb, None, torch.uint8, fill, offset=0)
        for step, (B, tag) in enumerate(((4, 'q8'), (1, 'qmix'), (3, 'q4'), (4, 'q8'), (-2, 'q8'), (4, 'q8'))):
            if B < 0:
                x = xs[:4].contiguous()
                got, want = _ddv(E, plan, x, bit[tag], fill, True, ws=ws), _ddv(E, plan, x, bit[tag], fill, True)
                assert _same_bits(got[1], want[1]), (step, hex(fill), 'sums')
                got, want = got[0], want[0]
            else:
                x = xs[6 - B:].contiguous()
                got, want = _forward(E, plan, x, bit[tag], fill, ws=ws)[0], _forward(E, plan, x, bit[tag], fill)[0]
                assert _same_bits(want, torch.from_numpy(g['logits/' + tag][6 - B:])), (step, tag)
            assert _same_bits(got, want), (step, B, tag, hex(fill))


def _tap_arenas(shapes, fill, want):
    return [Arena(int(np.prod(s[:-1])), s[-1], None, torch.float32, fill) if k in want else None for k, s in enumerate(shapes)]


def test_tap_entry_points_in_arenas(dva, micro, plan):
    """p2v_forward_taps (qkv / fc1 of every block), p2v_forward_linear_taps (all taps, and a subset with NULL for the others): every tap
    buffer an arena of exactly its tap_shapes extent.  Guards intact, logits equal to p2v_forward's, tap bytes equal to a plain-buffer
    call (pinned to the oracle in test_cka_gpu.py), identical under the three fills."""
    E = dva.engine
    L = E.lib()
    x = micro['x_ev'].cuda()
    B, depth, n_cfg = x.shape[0], plan.depth, plan.n_layers
    shapes = plan.tap_shapes(B)
    for tag in ('q8', 'qmix'):
        bits = _bits(micro['g'], tag, n_cfg)
        ref_logits = torch.from_numpy(micro['g']['logits/' + tag])
        _, plain = plan.forward_linear_taps(x, bits)
        _sync()
        plain = [t.cpu() for t in plain]
        plain[0] = plain[0].permute(0, 2, 3, 1).reshape(shapes[0]).contiguous()
        for fill in FILLS:
            # p2v_forward_taps
            ws, out = _ws_arena(E, plan, B, fill), Arena(B, plan.arch['num_classes'], None, torch.float32, fill)
            qkv = _tap_arenas([shapes[1 + 4 * i] for i in range(depth)], fill, set(range(depth)))
            fc1 = _tap_arenas([shapes[3 + 4 * i] for i in range(depth)], fill, set(range(depth)))
            pq, pf = (C.c_void_p * depth)(*[a.ptr.value for a in qkv]), (C.c_void_p * depth)(*[a.ptr.value for a in fc1])
            E.check(L.p2v_forward_taps(plan._handle, E.ptr(x), B, _cfg(bits), n_cfg, out.ptr, ws.ptr, ws.width, pq, pf, E.stream_ptr()))
            _sync()
            ws.read(('forward_taps workspace', tag, hex(fill)))
            assert _same_bits(out.read('forward_taps logits'), ref_logits)
            for i in range(depth):
                assert _same_bits(qkv[i].read(('qkv tap', i)).reshape(shapes[1 + 4 * i]), plain[1 + 4 * i]), (tag, i, hex(fill))
                assert _same_bits(fc1[i].read(('fc1 tap', i)).reshape(shapes[3 + 4 * i]), plain[3 + 4 * i]), (tag, i, hex(fill))
            # p2v_forward_linear_taps: everything, then proj / fc2 of the last block and the head alone
            for want in (set(range(n_cfg)), {4 * depth - 2, 4 * depth, n_cfg - 1}, {0}):
                ws, out = _ws_arena(E, plan, B, fill), Arena(B, plan.arch['num_classes'], None, torch.float32, fill)
                taps = _tap_arenas(shapes, fill, want)
                ptrs = (C.c_void_p * n_cfg)(*[None if a is None else a.ptr.value for a in taps])
                E.check(L.p2v_forward_linear_taps(plan._handle, E.ptr(x), B, _cfg(bits), n_cfg, out.ptr, ws.ptr, ws.width, ptrs, E.stream_ptr()))
                _sync()
                ws.read(('linear_taps workspace', tag, hex(fill), sorted(want)))
                assert _same_bits(out.read('linear_taps logits'), ref_logits)
                for k in sorted(want):
                    assert _same_bits(taps[k].read(('linear tap', k)).reshape(shapes[k]), plain[k]), (tag, k, hex(fill), sorted(want))


@pytest.mark.parametrize('with_linear', [0, 1])
def test_forward_ddv_in_arenas(dva, micro, plan, with_linear):
    """p2v_forward_ddv on three pairs: workspace (exactly p2v_ddv_workspace_bytes), logits, fp64 sums and the one tap buffer (exactly
    p2v_ddv_tap_scratch_bytes) in arenas; logits equal to p2v_forward's, sums equal to a plain-buffer call (pinned to the oracle in
    test_ddv_gpu.py), identical under the three fills"""
    E = dva.engine
    x = micro['x_ev'].cuda()
    for tag in ('q8', 'qmix'):
        bits = _bits(micro['g'], tag, plan.n_layers)
        _, _, plain = plan.forward_ddv(x, bits, with_linear=bool(with_linear))
        _sync()
        for fill in FILLS:
            out, sums = _ddv(E, plan, x, bits, fill, with_linear)
            assert _same_bits(out, torch.from_numpy(micro['g']['logits/' + tag])), (tag, hex(fill))
            assert _same_bits(sums, plain.cpu()), (tag, hex(fill), with_linear)


# --------------------------------------------------------------------------------------------------
# e. few tokens
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('img,patch,dim,depth,heads', [(8, 8, 64, 2, 2), (16, 8, 64, 2, 2), (16, 8, 144, 2, 3), (24, 8, 160, 1, 2)],
                         ids=['2tok', '5tok', '5tok-d144', '10tok-d160'])
def test_few_tokens_engine_vs_oracle(dva, oracle, img, patch, dim, depth, heads):
    """2, 5 and 10 tokens per image (head_dim 32, 48, 80; widths 144 and 160 are no multiples of the 64-deep k-tile, 160 x 3.5 = 560
    neither): a 16-row query block of the resident attention kernel, and the one query row of the class-row path, span several images of
    the dense [B T][D] buffers.  Batches 1, 3 and the first whose rows cross a 128-row tile; the three oracle-run images sit at the
    first, middle and last position.  cls_rows 1 / 0 x attn_stream 0 / 1 x the three fills, all inside the arenas of _forward."""
    E = dva.engine
    ratio = 3.5 if dim == 160 else 4.0
    arch = dict(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, num_classes=10, mlp_ratio=ratio)
    sd = dva.synth.vit_state_dict(arch, 33)
    m = dva.VisionTransformer(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, num_classes=10, mlp_ratio=ratio,
                              qkv_bias=True, norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(33, 2, img).cuda())
    x3 = dva.synth.images(33, 3, img, offset=700)
    L_ = 4 * depth + 2
    m(x3.cuda(), [8] * L_, False)                               # freezes the plan
    pl = m._plan
    T = pl.tokens
    assert T == (img // patch) ** 2 + 1 and T < 16
    orc = oracle.OracleViT(arch, sd)
    orc.calib = m.export_calib()
    big = 128 // T + 1
    assert (big - 1) * T <= 128 < big * T
    filler = dva.synth.images(77, big, img)
    for bits in ([8] * L_, [4] * L_, [4 if i % 3 == 1 else 8 for i in range(L_)]):
        ref = orc.quant_forward(x3, bits)
        assert len(torch.unique(ref)) > 1
        for B in (1, 3, big):
            pos = [0, B // 2, B - 1][:min(B, 3)] if B != 3 else [0, 1, 2]
            xb = filler[:B].clone()
            for i, p_ in enumerate(pos):
                xb[p_] = x3[i]
            xb = xb.cuda()
            for cr, st in ((1, 0), (0, 0), (1, 1), (0, 1)):
                with tuning(E.lib(), cls_rows=cr, attn_stream=st):
                    for fill in FILLS:
                        out, _ = _forward(E, pl, xb, bits, fill)
                        assert _same_bits(out[pos], ref[:len(pos)]), (img, dim, bits[:3], B, cr, st, hex(fill), int((out[pos] != ref[:len(pos)]).sum()))
