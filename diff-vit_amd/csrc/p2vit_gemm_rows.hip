// p2vit_gemm_rows.hip -- int8 MFMA GEMM for a FEW activation rows (the class-token rows of the last ViT block: M = images of a slice).
#include "p2vit_epilogue.h"
#include "p2vit_launch.h"

// ---------------------------------------------------------------------------------------------------
// K1r: the layer GEMM when M is small.  The tiled kernel (k_gemm_dma) gets its parallelism from M: at M = 68 it is one or two
//   workgroups per 128 columns, each walking the whole K with a global-memory round trip per k-tile.  Here the parallelism comes
//   from N and from K: a workgroup of eight waves owns 64 rows x 32 columns, wave w contracts the k-steps [w * S / 8, (w + 1) * S / 8)
//   (S = K / 32 steps of v_mfma_i32_32x32x32_i8) with its W and X fragments loaded straight from global memory into registers - no
//   operand is shared between waves, so nothing is staged in LDS - up to GR_STEPS steps requested before the first MFMA waits.
//   The eight partial 64 x 32 tiles are added through LDS in two rounds (int32: exact, order-free; 4 slots of 8 KB) and wave 0 runs
//   the epilogue of the tiled kernel on the sum (gemm_epilogue_tile2 / gemm_epilogue_resid_pre: the same code, the same codes).
//   Operand roles and register layout as in gemm_compute_tile: A operand = W rows n0 + l31, B operand = X rows m0 (+ 32) + l31,
//   lane half h holds bytes [16 h, 16 h + 16) of the 32-deep step.
//   lda, ldo free; the residual is read at ldo by the lane that later writes the same 16 bytes, before it writes them: proj and fc2
//   run in place on strided rows (the class rows of the residual stream).
// ---------------------------------------------------------------------------------------------------
#define GR_STEPS 6                  // k-steps a wave holds in registers at once: 3 fragments x 4 VGPRs each
#define GR_SLOT_BYTES (2 * 16 * 64 * 4)
#define GR_SLOTS 4

template <int EPI, bool W4>
__global__ __launch_bounds__(512) void k_gemm_rows(GemmArgs g) {
  constexpr bool RES = EPI == P2V_EPI_RESID || EPI == P2V_EPI_RESID_PRE;
  constexpr int EPI_BYTES = EPI == P2V_EPI_RESID ? (int)sizeof(EpiLds) : (EPI == P2V_EPI_RESID_PRE ? (int)sizeof(ResidLds) : 2 * GBN * (int)sizeof(float));
  __shared__ __attribute__((aligned(16))) int8_t lds[GR_SLOTS * GR_SLOT_BYTES + EPI_BYTES];
  v4i* sP = reinterpret_cast<v4i*>(lds);                         // [slot][8 register quads][64 lanes]
  EpiLds* sE = reinterpret_cast<EpiLds*>(lds + GR_SLOTS * GR_SLOT_BYTES);
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];   // GELU threshold table (cells * 8 bytes)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 32;
  const int tn = n0 / GBN, nl = n0 % GBN;                        // the 128-column tile the per-channel constants are laid out by

  // ---- this wave's share of K, split by 32-deep steps
  const int nsteps = g.K >> 5;
  const int s0 = wave * nsteps / 8, s1 = (wave + 1) * nsteps / 8;
  int ma = m0 + l31, mb = ma + 32;
  ma = ma < g.M ? ma : g.M - 1;
  mb = mb < g.M ? mb : g.M - 1;
  const int8_t* pa = g.A + (long long)ma * g.lda + 16 * h;
  const int8_t* pb = g.A + (long long)mb * g.lda + 16 * h;
  // packed int4: row r of the 4 KB image of (column tile, k-tile) holds its 8-byte chunks c at position c ^ ((r >> 3) & 3) (p2v_linear)
  const int wr = nl + l31;
  const int8_t* pw = W4 ? g.W + ((long long)tn * (g.K / GBK) * GBN + wr) * 32 : g.W + (long long)(n0 + l31) * g.K + 16 * h;
  auto load_w = [&](int ks) -> v4i {
    if (W4) {
      const uint2 p = *reinterpret_cast<const uint2*>(pw + (long long)(ks >> 1) * (GBN * 32) + (((2 * (ks & 1) + h) ^ ((wr >> 3) & 3)) << 3));
      return unpack_w4(p.x, p.y);
    }
    return *reinterpret_cast<const v4i*>(pw + 32 * ks);
  };

  // ---- epilogue constants / GELU table / residual codes: requested ahead of the k-loop, visible after the barriers of the reduction
  if constexpr (EPI == P2V_EPI_RESID_PRE) {
    if (tid < P2V_RESID_TAB_ARRAYS * GBN / 4)
      reinterpret_cast<float4*>(sE)[tid] = reinterpret_cast<const float4*>(g.ep.resid_tab + (long long)tn * (P2V_RESID_TAB_ARRAYS * GBN))[tid];
  } else {
    gemm_stage_epilogue<EPI>(sE, tn * GBN, tid, g);
  }
  if (EPI == P2V_EPI_GELU_TAB)
    for (int i = tid; i < g.ep.gelu.cells; i += 512)
      reinterpret_cast<uint2*>(dyn_lds)[i] = reinterpret_cast<const uint2*>(g.ep.gelu.table)[i];
  uint4 resv[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  if (RES && wave == 0) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int m = m0 + mi * 32 + l31, n = n0 + 16 * h;
      if (m < g.M && n < g.N) resv[mi] = *reinterpret_cast<const uint4*>(g.ep.residual + (long long)m * g.ldo + n);
    }
  }

  v16i acc[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0;
  for (int s = s0; s < s1; s += GR_STEPS) {          // wave-uniform bounds
    v4i fw[GR_STEPS], fa[GR_STEPS], fb[GR_STEPS];
#pragma unroll
    for (int j = 0; j < GR_STEPS; ++j)
      if (s + j < s1) {
        fw[j] = load_w(s + j);
        fa[j] = *reinterpret_cast<const v4i*>(pa + 32 * (s + j));
        fb[j] = *reinterpret_cast<const v4i*>(pb + 32 * (s + j));
      }
#pragma unroll
    for (int j = 0; j < GR_STEPS; ++j)
      if (s + j < s1) {
        acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fw[j], fa[j], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fw[j], fb[j], acc[1], 0, 0, 0);
      }
  }

  // ---- sum of the eight partial tiles: waves 4-7 -> waves 0-3 -> wave 0
  auto put = [&](int slot) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      sP[(slot * 8 + q) * 64 + lane] = (v4i){acc[q >> 2][4 * (q & 3)], acc[q >> 2][4 * (q & 3) + 1], acc[q >> 2][4 * (q & 3) + 2], acc[q >> 2][4 * (q & 3) + 3]};
  };
  auto add = [&](int slot) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const v4i p = sP[(slot * 8 + q) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[q >> 2][4 * (q & 3) + i] += p[i];
    }
  };
  if (wave >= 4) put(wave - 4);
  __syncthreads();
  if (wave < 4) add(wave);
  __syncthreads();
  if (wave >= 1 && wave < 4) put(wave - 1);
  __syncthreads();
  if (wave != 0) return;
  add(0);
  add(1);
  add(2);
  if constexpr (EPI == P2V_EPI_RESID_PRE)
    gemm_epilogue_resid_pre<false>(acc, m0 + l31, n0, nl, h, g, reinterpret_cast<const ResidLds*>(sE), resv);
  else
    gemm_epilogue_tile2<EPI, false>(acc, m0 + l31, n0, nl, h, g, sE, resv, dyn_lds);
}

extern int g_resid_pre;
int g_gemm_rows = 0;      // P2V_GEMM_ROWS: 0 = the row kernel where the forward asks for it (class rows of the last block), 1 = wherever it applies, 2 = never

// the instantiations of k_gemm_rows, in the order the code object holds them (p2vit_launch.h): (int8 weights) * 5 + slot
typedef void (*GemmRowsKernel)(GemmArgs);
constexpr int kRowsEpi[5] = {P2V_EPI_REQUANT, P2V_EPI_GELU_TAB, P2V_EPI_GELU, P2V_EPI_RESID_PRE, P2V_EPI_RESID};
constexpr int gemm_rows_index(int e, bool w4) { return (w4 ? 0 : 5) + p2v_slot(kRowsEpi, e); }
struct GemmRowsAt {
  template <int I> static constexpr GemmRowsKernel at() {
    static_assert(gemm_rows_index(kRowsEpi[I % 5], I < 5) == I, "decoded as the launcher encodes");
    return k_gemm_rows<kRowsEpi[I % 5], (I < 5)>;
  }
};
static const auto gemm_rows_table = p2v_table<GemmRowsKernel, GemmRowsAt, 10>();

// which epilogue of the row kernel a REQUANT / GELU / RESID layer runs
static int gemm_rows_epilogue(int epi, const GemmArgs& g, unsigned tab_bytes) {
  if (epi == P2V_EPI_REQUANT) return P2V_EPI_REQUANT;
  if (epi == P2V_EPI_GELU) return tab_bytes ? P2V_EPI_GELU_TAB : P2V_EPI_GELU;
  return (g.ep.resid_tab && g_resid_pre) ? P2V_EPI_RESID_PRE : P2V_EPI_RESID;
}

// -3: not a shape / epilogue of the row kernel (the caller runs the tiled kernel)
int p2v_launch_gemm_rows(int epi, const GemmArgs& g0, hipStream_t st) {
  if (epi != P2V_EPI_REQUANT && epi != P2V_EPI_GELU && epi != P2V_EPI_RESID) return -3;
  if (g0.M <= 0 || g0.N <= 0 || g0.K <= 0 || g0.K % GBK_PAD || (g0.M + 63) / 64 > 65535) return -3;
  GemmArgs g = g0;
#ifdef P2V_DIAG
  g.stamps = nullptr;
#endif
  g.tiles_n = (g.N + GBN - 1) / GBN;
  const dim3 grid((unsigned)((g.N + 31) / 32), (unsigned)((g.M + 63) / 64)), block(512);
  // the GELU table rides in dynamic LDS behind the reduction slots and the column constants; a table that does not fit the 64 KB a
  // kernel gets by default takes the arithmetic epilogue: same codes
  unsigned tab_bytes = (epi == P2V_EPI_GELU && g.ep.gelu.table) ? (unsigned)g.ep.gelu.cells * 8u : 0u;
  if (GR_SLOTS * GR_SLOT_BYTES + 2 * GBN * (int)sizeof(float) + (int)tab_bytes > 64 * 1024) tab_bytes = 0;
  hipLaunchKernelGGL(gemm_rows_table[gemm_rows_index(gemm_rows_epilogue(epi, g, tab_bytes), g.w4 != 0)], grid, block, tab_bytes, st, g);
  CHECK_LAUNCH();
  return 0;
}
