"""p2v_set_tuning switches for the GPU modules: the values they are restored to and a context manager that sets and restores them."""

# what the switches are restored to: the initialisers in diff-vit_amd/csrc (g_gemm_tile = 0 and g_resid_pre = 1 in p2vit_gemm.hip, g_gemm_rows = 0
# in p2vit_gemm_rows.hip, g_ln_rows = 4, the LayerNorm+GEMM version 2, ln_pre = 1 and ln_gemm = 1 (LayerNorm fused into qkv / fc1) in
# p2vit_ln.hip, attn_stream = 0 in p2vit_attn.hip, cls_rows = 1 (the last block on the class rows) in p2vit_capi.cpp).  p2v_set_tuning has no
# getter; a changed initialiser, or a P2V_* environment setting, has to be mirrored here
DEFAULTS = dict(gemm_tile=0, gemm_rows=0, resid_pre=1, ln_pre=1, ln_rows=4, ln_gemm_version=2, attn_stream=0, ln_gemm=1, cls_rows=1)


class tuning:
    """p2v_set_tuning switches for the duration of a block, restored on the way out"""

    def __init__(self, L, **kw):
        self.L, self.kw = L, kw

    def __enter__(self):
        for k, v in self.kw.items():
            assert self.L.p2v_set_tuning(k.encode(), v) == 0, (k, v)

    def __exit__(self, *exc):
        rcs = [self.L.p2v_set_tuning(k.encode(), DEFAULTS[k]) for k in self.kw]           # every switch first, then the verdict
        assert rcs == [0] * len(rcs), (list(self.kw), rcs)
