"""CPU: the FULL DDV stage set (every hook point of the reference's modeldiff_p2.add_hooks) - the stage lists and key maps, the module-graph
path of compute_ddv(..., stages='full') against the REAL reference's answers for all 30 keys of the micro-ViT (tests/golden/ddv_micro.npz),
the printed similarities over the full key list, and the argument refusals of the new entry points (made before the first HIP call).

Bounds: 1e-9 on a DDV entry, as in test_ddv.py (fp64 sums in two orders differ by at most 2 F 2^-53 relative to sqrt(aa bb); the
fake-quantised activations of the module graph are the reference's own)."""
import ctypes

import numpy as np
import pytest
import torch

from _ddv_full_ref import ddv_of, full_stage_values, load_reference_calibration
from conftest import golden_calib, golden_weights, load_golden
from test_ddv import micro_model


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def runs(dva, synth, oracle):
    """compute_ddv(..., stages='full') of the float micro model and of its quant-state twin under [8]*10 and [4]*10, computed once"""
    k = load_golden('ddv_micro')
    g = load_golden('micro_vit')
    x, xa = torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])
    m = micro_model(dva, synth, g)
    out = {'fp': dva.compute_ddv(m, x, xa, stages='full')}
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']))
    load_reference_calibration(m, golden_calib(g, oracle))
    assert m._fused()
    out['q8'] = dva.compute_ddv(m, x, xa, [8] * 10, stages='full')
    out['q4'] = dva.compute_ddv(m, x, xa, [4] * 10, stages='full')
    out['q8_engine_list'] = dva.compute_ddv(m, x, xa, [8] * 10)
    return k, out


def test_stage_lists_and_key_maps(dva):
    D = dva.ddv
    for depth in (1, 2, 12):
        eng0, eng1 = D.stage_names(depth, False), D.stage_names(depth, True)
        full0, full1 = D.stage_names(depth, False, full=True), D.stage_names(depth, True, True)
        assert (len(eng0), len(eng1)) == (5 * depth + 3, 9 * depth + 4)                 # unchanged
        assert (len(full0), len(full1)) == (9 * depth + 7, 13 * depth + 8)
        assert [n for n in full1 if n in eng1] == eng1 and [n for n in full0 if n in eng0] == eng0      # the engine list, in its order
        assert len(set(full1)) == len(full1)
        keys = D.reference_keys(depth, full=True)
        assert len(keys) == 10 * depth + 10
        assert keys['patch_embed'] == keys['patch_embed_qact'] == 'patch_embed.qact' and keys['pos_drop'] == 'qact1'
        assert set(keys.values()) - {'qact_pos'} <= set(full1)
        assert D.reference_keys(depth) == {r: s for r, s in keys.items() if s in eng1}      # the default map is the shared part
    assert D.stage_names(2, True)[:3] == ['qact1', 'blocks.0.attn.qkv', 'blocks.0.attn.qact1']
    assert D.stage_names(1, True, True) == [
        'qact_input', 'patch_embed.qact', 'qact_embed', 'qact1', 'blocks.0.norm1', 'blocks.0.attn.qkv', 'blocks.0.attn.qact1',
        'blocks.0.attn.qact2', 'blocks.0.attn.proj', 'blocks.0.attn.qact3', 'blocks.0.qact2', 'blocks.0.norm2', 'blocks.0.mlp.fc1',
        'blocks.0.mlp.qact1', 'blocks.0.mlp.fc2', 'blocks.0.mlp.qact2', 'blocks.0.qact4', 'norm', 'qact2', 'head', 'act_out']
    assert D.FULL_REFERENCE_KEYS == D.reference_keys(24, full=True) and D.REFERENCE_KEYS == D.reference_keys(24)
    assert len(D.REFERENCE_KEYS) == 6 * 24 + 4


@pytest.mark.parametrize('tag', ['q8', 'q4'])
def test_quantized_module_graph_full_matches_reference(dva, runs, tag):
    """all 30 keys of the reference's report for the quant-state micro model, within 1e-9"""
    k, out = runs
    d = out[tag]
    keys = [str(v) for v in k['keys/' + tag]]
    assert len(keys) == 30 and set(keys) == set(dva.ddv.reference_keys(2, full=True))
    assert list(d) == dva.ddv._with_qact_pos(dva.ddv.stage_names(2, True, True))
    assert d['qact_pos'].shape == (1,) and float(d['qact_pos'][0]) == 1.0 == float(k['ddv64/%s/qact_pos' % tag][0])
    worst = {}
    for r in keys:
        got = d[dva.ddv.FULL_REFERENCE_KEYS[r]].numpy()
        want = k['ddv64/%s/%s' % (tag, r)]
        assert got.shape == want.shape, r
        worst[r] = float(np.abs(got - want).max())
        print(tag, r, worst[r])
    bad = {r: e for r, e in worst.items() if not e <= 1e-9}
    assert not bad, bad


@pytest.mark.parametrize('tag', ['q8', 'q4'])
def test_oracle_restatement_of_the_new_stages(dva, oracle, synth, tag):
    """tests/_ddv_full_ref.py (what the GPU tests compare the engine with): the DDVs of its values are the reference's, to the last bits"""
    k, g = load_golden('ddv_micro'), load_golden('micro_vit')
    x = torch.cat((torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])), 0)
    bits = [8] * 10 if tag == 'q8' else [4] * 10
    vals, ints, _, _ = full_stage_values(oracle, synth.ARCHS['micro'], golden_weights(g), golden_calib(g, oracle), x, bits)
    RK = dva.ddv.reference_keys(2, full=True)
    new = [r for r in (str(v) for v in k['keys/' + tag]) if RK[r] in vals]
    assert len(new) == 4 * 2 + 6 - 1                         # every new key but qact_pos
    for r in new:
        err = float(np.abs(ddv_of(*vals[RK[r]]) - k['ddv64/%s/%s' % (tag, r)]).max())
        assert err <= 1e-12, (tag, r, err)
    # a clamped LayerNorm tap would be told apart: the unclamped integers leave the int8 range
    assert sum(int((t.abs() > 127).sum()) for t in ints) == (57 if tag == 'q8' else 56)


def test_full_keeps_the_engine_list_entries(runs):
    """the stages both lists have are the same tensors: equal entries, bit for bit"""
    _, out = runs
    for nm, v in out['q8_engine_list'].items():
        assert torch.equal(v, out['q8'][nm]), nm


def test_float_model_full_matches_reference(dva, runs):
    """the float micro model's 26 keys (no hook fires on qkv / fc1 of a float pass).  Like test_ddv.test_float_ddv_matches_reference this
    holds where the float pass is bit-equal to the reference's, i.e. on a host whose BLAS rounds like the fixture's; on a host where that
    test misses (block_0_mlp_fc2 3.0e-9 ... head 1.5e-7) this one misses by the same figures on the keys they share and by 1.4e-9 ... 9.4e-9
    on norm1 / norm2 / attn_qact3 / mlp_qact2 / final_norm of the blocks behind the first differing GEMM; qact_input ... block_0_qact2 agree to 2e-16."""
    k, out = runs
    d = out['fp']
    keys = [str(v) for v in k['keys/fp']]
    assert len(keys) == 26                                  # no hook fires on qkv / fc1 of a float pass (the SmoothQuant branch)
    worst = {}
    for r in keys:
        worst[r] = float(np.abs(d[dva.ddv.FULL_REFERENCE_KEYS[r]].numpy() - k['ddv64/fp/' + r]).max())
        print('fp', r, worst[r])
    bad = {r: e for r, e in worst.items() if not e <= 1e-9}
    assert not bad, bad


@pytest.mark.parametrize('tag', ['q8', 'q4'])
def test_reference_similarity_over_the_full_key_list(dva, runs, tag):
    """what calculate_and_print_similarities prints, one line per key of the float model's dict"""
    k, out = runs
    keys = [str(v) for v in k['keys']]
    RK = dva.ddv.FULL_REFERENCE_KEYS
    fp = {r: out['fp'][RK[r]] for r in keys}
    q = {r: out[tag][RK[r]] for r in keys}
    got = dva.ddv.reference_similarity(fp, q)
    assert list(got) == keys and len(keys) == 26
    assert np.allclose([got[r] for r in keys], k['printed/' + tag], rtol=0, atol=1e-6, equal_nan=True)
    s = dva.ddv.similarity(fp, q)
    assert list(s) == keys and all(-1 - 1e-12 <= s[r] <= 1 + 1e-12 for r in keys)


def test_qact_pos_entry(dva):
    one = dva.ddv._qact_pos_ddv(False, torch.device('cpu'))
    assert one.dtype == torch.float64 and one.tolist() == [1.0]
    assert torch.isnan(dva.ddv._qact_pos_ddv(True, torch.device('cpu'))).all()
    # the module-graph form of the same: a zero position embedding gives 0/0, as numpy does in the reference
    z = torch.zeros(1, 5, 16)
    assert torch.isnan(dva.ddv.ddv_from_sums(dva.ddv.pair_cosine_cpu([z], [z]))).all()


def test_refusals_without_gpu(dva, synth):
    E = dva.engine
    L = E.lib()
    with pytest.raises(ValueError):
        dva.compute_ddv(micro_model(dva, synth, load_golden('micro_vit')), torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), stages='all')
    h = ctypes.c_void_p()
    desc = E.ModelDesc(E.P2V_ABI_VERSION, 224, 16, 3, 384, 12, 6, 1536, 1000)
    E.check(L.p2v_plan_create(ctypes.byref(desc), ctypes.byref(h)))
    # stage counts: the old function is the stage_set = 0 case
    assert L.p2v_ddv_stage_count_ex(h, 0, E.DDV_STAGES_ENGINE) == L.p2v_ddv_stage_count(h, 0) == 63
    assert L.p2v_ddv_stage_count_ex(h, 1, E.DDV_STAGES_ENGINE) == L.p2v_ddv_stage_count(h, 1) == 112
    assert L.p2v_ddv_stage_count_ex(h, 0, E.DDV_STAGES_FULL) == 9 * 12 + 7 and L.p2v_ddv_stage_count_ex(h, 1, E.DDV_STAGES_FULL) == 13 * 12 + 8
    assert L.p2v_ddv_stage_count_ex(h, 1, 2) == E.E_ARG and b'stage_set' in L.p2v_last_error()
    assert L.p2v_ddv_workspace_bytes_ex(h, 4, E.DDV_STAGES_FULL) == L.p2v_ddv_workspace_bytes_ex(h, 4, 0) == L.p2v_ddv_workspace_bytes(h, 4) > 0
    assert L.p2v_ddv_workspace_bytes_ex(h, 4, 7) == 0
    cfg = (ctypes.c_int8 * 50)(*([8] * 50))
    one = ctypes.c_void_p(256)
    big = 1 << 40

    def call(stage_set, tap, tap_bytes, ws_bytes=big, n=4):
        return L.p2v_forward_ddv_ex(h, one, n, cfg, 50, one, one, ws_bytes, 0, stage_set, tap, tap_bytes, one, None)
    assert call(2, one, big) == E.E_ARG and b'unknown stage_set 2' in L.p2v_last_error()
    assert call(-1, one, big) == E.E_ARG
    # a plan without an input QAct (inv_s_input == 0, as a fresh plan and an input_quant = False one have it): no qact_input stage
    assert call(E.DDV_STAGES_FULL, one, big) == E.E_UNSUPPORTED and b'input QAct' in L.p2v_last_error()
    epi = E.Epilogue()
    E.check(L.p2v_plan_set_embed(h, 0.0, ctypes.byref(epi), one))
    assert call(E.DDV_STAGES_FULL, one, big) == E.E_UNSUPPORTED
    E.check(L.p2v_plan_set_embed(h, 64.0, ctypes.byref(epi), one))
    assert call(E.DDV_STAGES_FULL, one, big) == E.E_STATE and b'p2v_plan_set_embed_tap_cls' in L.p2v_last_error()
    assert L.p2v_plan_set_embed_tap_cls(h, None) == E.E_ARG
    E.check(L.p2v_plan_set_embed_tap_cls(h, one))
    # FULL needs the tap buffer whatever with_linear says, and a whole one
    assert call(E.DDV_STAGES_FULL, None, 0) == E.E_WORKSPACE and b'tap_scratch' in L.p2v_last_error()
    need = L.p2v_ddv_tap_scratch_bytes(h, 4)
    assert call(E.DDV_STAGES_FULL, one, need - 1) == E.E_WORKSPACE and b'tap_scratch' in L.p2v_last_error()
    assert call(E.DDV_STAGES_FULL, one, big, ws_bytes=L.p2v_workspace_bytes(h, 8)) == E.E_WORKSPACE and b'workspace' in L.p2v_last_error()
    assert call(E.DDV_STAGES_FULL, ctypes.c_void_p(264), big) == E.E_ARG                  # misaligned
    # past its own list the entry point runs p2v_forward's: the plan is incomplete (no HIP call so far)
    assert call(E.DDV_STAGES_FULL, one, big) == E.E_STATE
    assert call(E.DDV_STAGES_ENGINE, None, 0) == E.E_STATE
    L.p2v_plan_destroy(h)
    # the per-operator taps
    ln = E.Ln()
    args = (one, 64, 4, 64, ctypes.byref(ln), one, 64)
    assert L.p2v_int_layernorm_tap(*args, None, None) == E.E_ARG
    assert L.p2v_int_layernorm_tap(*args, ctypes.c_void_p(260), None) == E.E_ARG and b'16-byte' in L.p2v_last_error()
    assert L.p2v_int_layernorm_tap(one, 2052, 4, 2052, ctypes.byref(ln), one, 2052, one, None) == E.E_UNSUPPORTED
    assert b'2048' in L.p2v_last_error()
    assert L.p2v_int_layernorm_tap(one, 64, 0, 64, ctypes.byref(ln), one, 64, one, None) == E.E_SHAPE
    lin = E.Linear()
    assert L.p2v_gemm_embed_tap(one, 64, 4, 64, 64, ctypes.byref(lin), ctypes.byref(epi), one, 64, None, one, None) == E.E_ARG
    assert L.p2v_gemm_embed_tap(one, 64, 4, 64, 64, ctypes.byref(lin), ctypes.byref(epi), one, 64, one, one, None) == E.E_ARG    # no s_next / pos_deq
    assert b'EMBED' in L.p2v_last_error()
    assert L.p2v_gemm_embed_tap(one, 64, 4, 60, 64, ctypes.byref(lin), ctypes.byref(epi), one, 64, one, one, None) == E.E_SHAPE


def test_cli_prints_every_stage(dva, tmp_path, capsys):
    """python -m diff_vit_amd.ddv --stages full (module graph on the CPU, two seeds, one PGD step): one line and one pickle entry per hook point"""
    import os
    import pickle
    out = str(tmp_path / 'ddv_result')
    sim = dva.ddv.main(['--model', 'deit_tiny', '--n', '2', '--steps', '1', '--device', 'cpu', '--stages', 'full', '--result-name', out])
    want = dva.ddv._with_qact_pos(dva.ddv.stage_names(12, True, True))
    assert len(want) == 13 * 12 + 8 + 1
    printed = [ln.split()[0] for ln in capsys.readouterr().out.splitlines() if ' cosine ' in ln]
    assert printed == want == list(sim)
    with open(os.path.join(out, 'ddv.pkl'), 'rb') as f:
        res = pickle.load(f)
    assert list(res['float']) == want == list(res['quantized'])
    assert res['quantized']['qact_pos'].shape == (1,) and all(v.shape == (2,) for k, v in res['quantized'].items() if k != 'qact_pos')
