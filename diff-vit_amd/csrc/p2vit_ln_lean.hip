// p2vit_ln_lean.hip -- the lean forms of the pipelined fused LayerNorm + GEMM kernel (k_ln_gemm2, LG2_FORM_LEAN and LG2_FORM_LEAN_PM1) and their
// table.  A translation unit of its own: the code object of p2vit_ln.hip holds what it always held (tools/kernel_resources.py --digest).
#include "p2vit_ln_gemm.h"

// flat index (((post_mul != 1) * 2 + slot) * 6 + kt - 1) * 2 + (int8 weights)
constexpr int ln_gemm_lean_index(int e, bool pm1, int kt, bool w4) { return (((pm1 ? 0 : 1) * 2 + p2v_slot(kLnGemmEpi, e)) * 6 + kt - 1) * 2 + (w4 ? 0 : 1); }
struct LnGemmLeanAt {
  template <int I> static constexpr LnGemmLauncher at() {
    constexpr int E = kLnGemmEpi[I / 12 % 2];
    static_assert(ln_gemm_lean_index(E, I < 24, I / 2 % 6 + 1, !(I & 1)) == I, "decoded as the launcher encodes");
    return launch_ln_gemm_t<E, I / 2 % 6 + 1, I < 24 ? 5 : 4, !(I & 1)>;
  }
};
static const auto ln_gemm_lean_table = p2v_table<LnGemmLauncher, LnGemmLeanAt, 48>();
LnGemmLauncher p2v_ln_gemm_lean_launcher(int e, bool pm1, int kt, bool w4) { return ln_gemm_lean_table[ln_gemm_lean_index(e, pm1, kt, w4)]; }
