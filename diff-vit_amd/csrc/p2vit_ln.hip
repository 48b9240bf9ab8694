// p2vit_ln.hip -- integer LayerNorm (stand-alone) and the fused LayerNorm + GEMM kernels, with their launchers.
#include "p2vit_ln_row.h"
#include "p2vit_launch.h"

// ---------------------------------------------------------------------------------------------------
// K2: integer LayerNorm (QIntLayerNorm mode 'int', layers.py:255-289) + /channel_scale + qact0 clamp
// (vit_fquant.py:284-289).  One row per 32-lane half wave (12 bytes/lane at C=384), LN_ROWS rows per half
// wave so the five per-channel constant vectors stay in registers.  sum x and sum x^2 are exact integers;
// everything after mirrors the reference's fp32 operation order.
// ---------------------------------------------------------------------------------------------------

// rows per batch in the stand-alone kernel: with every constant in registers two rows cost 23 more VGPRs, i.e. the third wave per SIMD at
// C = 384 and 768 (measured 9 % / 6 % slower); with post_mul and the mask left in LDS (LN_LDSC) the pair fits
#ifndef LN_BATCH
#define LN_BATCH 2
#endif
#ifndef LN_LDSC
#define LN_LDSC true
#endif
// TAP: the value tap (a.tap_out, dense fp32 [rows][C]) - what a forward hook on the module sees, the UNCLAMPED integer of layers.py:288
// times out_scale - stored from inside the per-element chain (ln_apply); the codes are byte-identical to the launch without it
template <int NCH, int LANES, bool PRE, bool TAP = false>        // PRE: the constants were folded when the plan was created (LnPre)
__global__ __launch_bounds__(256) void k_int_layernorm(LnArgs a) {
  // per-channel constants are folded once per workgroup, shared through LDS, then held in registers (re-reading them from
  // LDS per row frees 46 VGPRs but measured 10 % slower: the kernel is bound by VALU issue, not by occupancy)
  __shared__ __attribute__((aligned(16))) float sG[NCH * LANES * 4], sB[NCH * LANES * 4], sP[NCH * LANES * 4];
  __shared__ __attribute__((aligned(16))) int sM[NCH * LANES * 4];
  const int tid = threadIdx.x, l32 = tid & (LANES - 1), hw = tid / LANES;   // l32: lane within the row group
  LnLane<NCH, LN_LDSC> L;
  // A workgroup lives for only a few rows (16 - 32): its first rows are requested BEFORE the constants are staged, so that one memory round
  // trip covers both (round 4; before, the row loads were issued behind the prologue's barrier: two exposed round trips per workgroup)
  const int LN_ROWS = a.rows_per_half;
  const long long row0 = ((long long)blockIdx.x * (256 / LANES) + hw) * LN_ROWS;
  const long long last_row = a.rows - 1;
  constexpr int R = LN_BATCH;                                      // rows per batch of ln_rows (the row scalars are computed once per batch)
  int colofs[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) colofs[i] = (l32 + LANES * i) * 4 < a.C ? (l32 + LANES * i) * 4 : 0;     // clamped: loads are unconditional
  unsigned wnext[R][NCH];
#pragma unroll
  for (int u = 0; u < R; ++u)
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      wnext[u][i] = *reinterpret_cast<const unsigned*>(a.x + (row0 + u < a.rows ? row0 + u : last_row) * a.row_stride + colofs[i]);
  if constexpr (PRE) {      // only post_mul and the mask go through LDS (LN_LDSC), one barrier; the folded constants are requested first
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (l32 + LANES * i) * 4;
      L.on[i] = c < a.C;
      L.gm[i] = *reinterpret_cast<const float4*>(a.pre.gm + c);
      L.bt[i] = *reinterpret_cast<const float4*>(a.pre.bt + c);
    }
    for (int t4 = tid; t4 < NCH * LANES; t4 += 256) {
      const int c = t4 * 4;
      float4 pmv = make_float4(0.f, 0.f, 0.f, 0.f), mk = pmv;
      if (c < a.C) {
        pmv = *reinterpret_cast<const float4*>(a.ln.post_mul + c);
        mk = *reinterpret_cast<const float4*>(a.ln.mask + c);
      }
      *reinterpret_cast<float4*>(sP + c) = pmv;
      *reinterpret_cast<float4*>(sM + c) = ln_scale_mask(mk);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (l32 + LANES * i) * 4;
      if constexpr (sizeof(L.pm) == sizeof(float4) * NCH) {
        L.pm[i] = *reinterpret_cast<const float4*>(sP + c);
        L.mkf[i] = *reinterpret_cast<const float4*>(sM + c);
      }
    }
    L.sPl = sP + l32 * 4;
    L.sMl = reinterpret_cast<const float*>(sM) + l32 * 4;
    L.cstride = LANES * 4;
    L.gmin = a.pre.gmin;
    L.gmax = a.pre.gmax;
    L.bmax = a.pre.bmax;
    L.pot = a.pre.pot != 0 && a.force_generic == 0;
    L.pm_one = a.pre.pm_one != 0;
  } else {
    ln_prepare<NCH, LANES>(a.ln, a.C, a.force_generic != 0, sG, sB, sP, sM, tid, 256, L);
  }
  // Row r+1 is requested at the top of the iteration of row r and first touched just before the stores of row r.  The two
  // empty asm statements pin that placement: left alone, hipcc sinks the loads of a loop-carried value to the loop end,
  // behind the stores, and waits vmcnt(0) there - two exposed memory round trips per row (measured: 3 us per row).
#pragma unroll
  for (int u = 0; u < R; ++u)
#pragma unroll
    for (int i = 0; i < NCH; ++i) asm volatile("" : "+v"(wnext[u][i]));   // first rows landed: no wait is merged into the loop head
#pragma unroll 1
  for (int rr = 0; rr < LN_ROWS; rr += R) {
    const long long row = row0 + rr;
    if (row >= a.rows) break;   // uniform within the row group; the reductions below stay inside it
    unsigned wcur[R][NCH];
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int i = 0; i < NCH; ++i) wcur[u][i] = L.on[i] ? wnext[u][i] : 0u;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const long long nrow = row + R + u < a.rows ? row + R + u : last_row;
#pragma unroll
      for (int i = 0; i < NCH; ++i) wnext[u][i] = *reinterpret_cast<const unsigned*>(a.x + nrow * a.row_stride + colofs[i]);
    }
    asm volatile("" ::: "memory");                 // the loads stay above this line
    unsigned outw[R][NCH];
    if constexpr (TAP) {
      float* taps[R];
#pragma unroll
      for (int u = 0; u < R; ++u) taps[u] = (rr + u < LN_ROWS && row + u < a.rows) ? a.tap_out + (row + u) * (long long)a.C : nullptr;
      if constexpr (R == 1) ln_row<NCH, LANES, decltype(L), true>(wcur[0], L, a.ln, a.C, l32, outw[0], taps[0]);
      else ln_rows<NCH, LANES, R, decltype(L), true>(wcur, L, a.ln, a.C, l32, outw, taps);
    } else {
    if constexpr (R == 1) ln_row<NCH, LANES>(wcur[0], L, a.ln, a.C, l32, outw[0]);
    else ln_rows<NCH, LANES, R>(wcur, L, a.ln, a.C, l32, outw);
    }
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
      for (int i = 0; i < NCH; ++i) asm volatile("" : "+v"(wnext[u][i]));   // the wait for the next rows lands here, ahead of the stores
#pragma unroll
    for (int u = 0; u < R; ++u) {
      if (rr + u >= LN_ROWS || row + u >= a.rows) continue;
      int8_t* dst = a.out + (row + u) * a.out_stride;
#pragma unroll
      for (int i = 0; i < NCH; ++i)
        if (L.on[i]) *reinterpret_cast<unsigned*>(dst + (l32 + LANES * i) * 4) = outw[u][i];
    }
  }
}

#include "p2vit_ln_gemm.h"



// ---------------------------------------------------------------------------------------------------
// host launchers (called from the C ABI in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
#ifdef P2V_DIAG
extern unsigned long long* g_gemm_stamps;
#endif
int g_ln_pre = 1;         // P2V_LN_PRE=0: ignore p2v_ln.pre, every workgroup folds the constants itself (A/B and parity runs; same codes)
int g_ln_generic = 0;     // P2V_LN_GENERIC=1
// LayerNorm + GEMM in one launch.  Returns -3 when the shape is outside what the fused kernel is instantiated for (callers then
// run p2v_launch_layernorm + p2v_launch_gemm).
int g_ln_gemm = 1;        // P2V_LN_GEMM=0: never fuse (A/B runs)
bool p2v_ln_gemm_supported(int epi, int C, int N, int table_cells) {
  if (!g_ln_gemm || (epi != P2V_EPI_REQUANT && epi != P2V_EPI_GELU)) return false;
  if (C % 4 || C > 384 || N % 16) return false;
  return ln_gemm_lds(C, N, ((C + GBK - 1) / GBK + 1) / 2, table_cells).total <= 80 * 1024;     // two workgroups per CU
}
// the fused launchers, in the order the code object holds their kernels (p2vit_launch.h): flat index
// (((3 - version) * 3 + slot) * 6 + kt - 1) * 2 + (int8 weights); null = not instantiated (versions 2 and 3 serve REQUANT and the table GELU only)
constexpr int ln_gemm_index(int e, int ver, int kt, bool w4) { return (((3 - ver) * 3 + p2v_slot(kLnGemmEpi, e)) * 6 + kt - 1) * 2 + (w4 ? 0 : 1); }
struct LnGemmAt {
  template <int I> static constexpr LnGemmLauncher at() {
    constexpr int E = kLnGemmEpi[I / 12 % 3], VER = 3 - I / 36;
    static_assert(ln_gemm_index(E, VER, I / 2 % 6 + 1, !(I & 1)) == I, "decoded as the launcher encodes");
    if constexpr (E != P2V_EPI_GELU || VER == 1) return launch_ln_gemm_t<E, I / 2 % 6 + 1, VER, !(I & 1)>;
    else return nullptr;
  }
};
static const auto ln_gemm_table = p2v_table<LnGemmLauncher, LnGemmAt, 108>();
int g_ln_gemm_lean = 1;  // P2V_LN_GEMM_LEAN=0: the general LayerNorm phase for every launch (A/B runs; same results)
int g_ln_gemm_ver = 2;   // P2V_LN_GEMM_V=1: the 4-wave kernel of round 2 for every launch (A/B runs; same results)
// g0.W must point to the FRAGMENT-ORDER copy of the weights (p2v_linear.w_frag; packed two codes per byte when g0.w4)
int p2v_launch_ln_gemm(int epi, const LnArgs& a_, const GemmArgs& g0, hipStream_t st) {
  const int cells = (epi == P2V_EPI_GELU && g0.ep.gelu.table) ? g0.ep.gelu.cells : 0;
  if (!p2v_ln_gemm_supported(epi, a_.C, g0.N, cells)) return -3;
  if (a_.row_stride < 0 || a_.row_stride > (1 << 24)) return -3;       // the kernels address a workgroup's 64 rows with 32-bit offsets
  LnArgs a = a_;
  a.force_generic = g_ln_generic;
  if (!g_ln_pre) a.pre.gm = nullptr;
  GemmArgs g = g0;
  g.tiles_n = (g.N + GBN - 1) / GBN;
#ifdef P2V_DIAG
  g.stamps = g_gemm_stamps;
#endif
  const int kt = (a.C + GBK - 1) / GBK;
  const int e = epi == P2V_EPI_REQUANT ? P2V_EPI_REQUANT : (cells ? P2V_EPI_GELU_TAB : P2V_EPI_GELU);
  // the dense 8-wave kernel: REQUANT and table GELU without activation taps; everything else runs the 4-wave kernel
  const int ver = ((g_ln_gemm_ver == 3 || g_ln_gemm_ver == 2) && !g.ep.tap_out && e != P2V_EPI_GELU) ? g_ln_gemm_ver : 1;
  const int kti = kt >= 1 && kt <= 5 ? kt : 6;
  // the lean LayerNorm phase: what a frozen plan launches (constants folded ahead with `pot` proven, whole k-tiles, no LayerNorm output)
  const bool lean = g_ln_gemm_lean && ver == 2 && a.pre.gm && a.pre.pot && !a.force_generic && a.C == kt * GBK && !a.out && !a.tap_out;
  const LnGemmLauncher launch = lean ? p2v_ln_gemm_lean_launcher(e, a.pre.pm_one != 0, kti, g.w4 != 0) : ln_gemm_table[ln_gemm_index(e, ver, kti, g.w4 != 0)];
  return launch ? launch(a, g, cells, st) : -3;
}

// the instantiations of k_int_layernorm, in the order the code object holds them (p2vit_launch.h): flat index
// (((untapped) * 2 + (row per half wave)) * 9 + nch) * 2 + (constants folded by the kernel).  A row per wave (64 lanes) holds 2..8 groups of
// 256 channels, a row per half wave 1..3 groups of 128; null = not instantiated
typedef void (*LnKernel)(LnArgs);
constexpr int ln_index(bool tap, bool half, int nch, bool pre) { return (((tap ? 0 : 2) + (half ? 1 : 0)) * 9 + nch) * 2 + (pre ? 0 : 1); }
struct LnAt {
  template <int I> static constexpr LnKernel at() {
    constexpr bool HALF = (I / 18 & 1) != 0;
    constexpr int NCH = I / 2 % 9;
    static_assert(ln_index(I < 36, HALF, NCH, !(I & 1)) == I, "decoded as the launcher encodes");
    if constexpr (HALF ? (NCH >= 1 && NCH <= 3) : (NCH >= 2 && NCH <= 8)) return k_int_layernorm<NCH, HALF ? 32 : 64, !(I & 1), (I < 36)>;
    else return nullptr;
  }
};
static const auto ln_table = p2v_table<LnKernel, LnAt, 72>();

int g_ln_rows = 4;        // P2V_LN_ROWS: consecutive rows per half wave
int p2v_launch_layernorm(const LnArgs& a_, hipStream_t st) {
  LnArgs a = a_;
  a.force_generic = g_ln_generic;
  if (!g_ln_pre) a.pre.gm = nullptr;
  if (a.C > 2048) return a.tap_out ? -1 : p2v_launch_layernorm_xwide(a, st);      // a row per workgroup (p2vit_ln_xwide.hip); below, nothing changes
  a.rows_per_half = g_ln_rows;
  const int LN_ROWS = g_ln_rows;
  // one row per WAVE above 384 channels (64 lanes x 4 channels x up to 8 groups = 2048 channels): the per-lane constants of a half-wave
  // row cost ~45 VGPRs per 128 channels (C = 768: 256 VGPRs, one wave per SIMD; a wave per row: 161, three)
  const bool wide = a.C > 384;
  const int nch = wide ? (a.C + 255) / 256 : (a.C + 127) / 128;
  const int rows_per_block = (wide ? 4 : 8) * LN_ROWS;
  dim3 grid((unsigned)((a.rows + rows_per_block - 1) / rows_per_block)), block(256);
  // tap_out: the value tap (p2v_int_layernorm_tap, the FULL stage set of p2v_forward_ddv_ex): same grid, same codes
  const LnKernel kernel = (nch >= 0 && nch <= 8) ? ln_table[ln_index(a.tap_out != nullptr, !wide, nch, a.pre.gm != nullptr)] : nullptr;
  if (!kernel) return -1;
  hipLaunchKernelGGL(kernel, grid, block, 0, st, a);
  CHECK_LAUNCH();
  return 0;
}
