// p2vit_ln_gemm.h -- the fused LayerNorm + GEMM kernels and the launcher of one instantiation.  Included by p2vit_ln.hip (the general forms)
// and by p2vit_ln_lean.hip (the lean forms of k_ln_gemm2, in a code object of their own, so that the one of p2vit_ln.hip stays as it is).
#pragma once
#include "p2vit_ln_row.h"
#include "p2vit_launch.h"

// ---------------------------------------------------------------------------------------------------
// K2b: LayerNorm fused into the GEMM that consumes it (norm1 -> qkv, norm2 -> fc1):  QIntLayerNorm 'int' -> /channel_scale ->
//   qact0 -> QLinear -> (GELU ->) QAct   (vit_fquant.py:431-434,284-293,307; layers_quant.py:305-316,331-333).
//   X-stationary: a workgroup owns 64 rows.  Prologue = the LayerNorm kernel's row code (ln_prepare / ln_row); its output codes
//   go to an LDS panel [K/64][64 rows][64 B] instead of HBM.  Main loop over the 128-column tiles of the layer: wave w computes
//   all 64 rows x columns [32w, 32w+32), so the W rows it needs are its own.  The plan stores these weights a second time in
//   MFMA-FRAGMENT ORDER (p2v_linear.w_frag: [column tile][wave][k-step][lane][16 B]), so the A operand of every MFMA is one fully
//   coalesced 1 KB global load straight into registers: no LDS staging for W, no barrier in the main loop, and all waits are
//   the compiler's own exact scoreboard (an LDS-DMA ring version of this kernel spent ~700 of 890 cycles per k-step on manual
//   wait counting, M0 set-up and DMA issue; profiles/r02_ln_gemm_timeline.txt).  The W fragments of column tile j+1 are requested
//   into the registers tile j has just consumed, one k-step behind the MFMAs: a full tile of lead.
//   What it removes per block: two LayerNorm launches, 2 x (read + write of the residual-sized tensor), and every re-read of the
//   activation panel by the 9 / 12 column-tile workgroups of the tiled kernel.
// ---------------------------------------------------------------------------------------------------
#define LG_BM 64
// W fragments of the fused kernels: 16 bytes per lane (one code per byte) or, for packed int4 weights (p2v_linear.packed4), 8 bytes
// per lane widened in registers like the tiled kernel's (unpack_w4: codes << 4, the 1/16 goes into the column scale)
template <bool W4> struct LgW { typedef uint4 raw; };
template <> struct LgW<true> { typedef uint2 raw; };
__device__ __forceinline__ v4i lg_wfrag(uint4 w) { return __builtin_bit_cast(v4i, w); }
__device__ __forceinline__ v4i lg_wfrag(uint2 w) { return unpack_w4(w.x, w.y); }
struct LnGemmLds {                        // byte offsets inside the dynamic LDS allocation
  int panel, consts, fold, table, total;
};
__host__ __device__ inline LnGemmLds ln_gemm_lds(int K, int N, int nch, int table_cells) {
  LnGemmLds o;
  const int kt = (K + GBK - 1) / GBK, tiles_n = (N + GBN - 1) / GBN;
  o.panel = 0;
  o.consts = o.panel + kt * LG_BM * GBK;
  o.fold = o.panel;        // the LayerNorm fold scratch (4 * nch * 512 B <= the panel) is dead before the first panel row is written
  o.table = o.consts + tiles_n * GBN * 2 * (int)sizeof(float);
  o.total = o.table + table_cells * 8;
  return o;
}

#ifdef P2V_DIAG
#define LG_STAMP(slot)                                                                                              \
  do {                                                                                                              \
    if (g.stamps && threadIdx.x == 0 && (slot) < 62) g.stamps[(long long)blockIdx.x * 64 + (slot)] = __builtin_readcyclecounter(); \
  } while (0)
#else
#define LG_STAMP(slot) do { } while (0)
#endif
template <int EPI, int KT, bool W4>      // KT = k-tiles of 64 channels (C <= 64*KT); W4: packed int4 fragment copy
__global__ __launch_bounds__(256, 2) void k_ln_gemm(LnArgs a, GemmArgs g) {
  typedef typename LgW<W4>::raw wraw;
  constexpr int NCH = (KT + 1) / 2;      // 128-channel groups of a LayerNorm row
  constexpr int NI = 2 * KT;             // k-steps of 32
  extern __shared__ __attribute__((aligned(1024))) unsigned char lg_smem[];
  LG_STAMP(0);
  const int C = a.C;
  const int cells = EPI == P2V_EPI_GELU_TAB ? g.ep.gelu.cells : 0;
  const LnGemmLds lay = ln_gemm_lds(C, g.N, NCH, cells);
  int8_t* panel = reinterpret_cast<int8_t*>(lg_smem + lay.panel);
  float* consts = reinterpret_cast<float*>(lg_smem + lay.consts);      // per column tile: colscale[128] | bias[128]
  const unsigned char* gtab = lg_smem + lay.table;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.x * LG_BM;
  const int tiles_n = g.tiles_n;

  // ---- W fragments of column tile 0 (registers): element ((j*4 + wave)*NI + i)*64 + lane of 16 bytes
  const wraw* wsrc = reinterpret_cast<const wraw*>(g.W) + (long long)wave * NI * 64 + lane;
  wraw wf[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) wf[i] = wsrc[i * 64];

  // ---- the 64 rows of the residual stream: one row per half wave, 8 rows each, two rows in flight ahead of the two being normalised
  constexpr int RPH = LG_BM / 8;                                       // rows per half wave
  static_assert(RPH % 2 == 0, "rows are processed in pairs");
  const int hw = tid >> 5;
  auto load_row = [&](int r, unsigned (&w)[NCH]) {
    long long row = (long long)m0 + hw * RPH + r;
    row = row < a.rows ? row : a.rows - 1;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (l31 + 32 * i) * 4;
      w[i] = *reinterpret_cast<const unsigned*>(a.x + row * a.row_stride + (c < C ? c : 0));
    }
  };
  unsigned win[2][NCH];
  load_row(0, win[0]);
  load_row(1, win[1]);
  // ---- per-column constants of the whole layer (REQUANT: 2^e folded in, see gemm_stage_epilogue) and the GELU table
  {
    const float fold = EPI == P2V_EPI_REQUANT ? g.ep.inv_s_out : (EPI == P2V_EPI_GELU_TAB ? g.ep.gelu.k : 1.0f);   // GELU_TAB: u = y * k, see gelu_tab_offset
    const float cfold = fold * (W4 ? 0.0625f : 1.0f);                   // packed int4: the accumulator holds 16 x the sum
    for (int n4 = tid; n4 < tiles_n * (GBN / 4); n4 += 256) {           // four columns per thread and turn
      const int j_ = n4 >> 5, c_ = (n4 & 31) * 4;
      const float4 cv = *reinterpret_cast<const float4*>(g.colscale + n4 * 4);   // arrays are padded to n_pad
      const float4 bv = *reinterpret_cast<const float4*>(g.bias + n4 * 4);
      *reinterpret_cast<float4*>(consts + j_ * 2 * GBN + c_) = make_float4(cv.x * cfold, cv.y * cfold, cv.z * cfold, cv.w * cfold);
      *reinterpret_cast<float4*>(consts + j_ * 2 * GBN + GBN + c_) = make_float4(bv.x * fold, bv.y * fold, bv.z * fold, bv.w * fold);
    }
    if (EPI == P2V_EPI_GELU_TAB)
      for (int i = tid; i < cells; i += 256)
        reinterpret_cast<uint2*>(lg_smem + lay.table)[i] = reinterpret_cast<const uint2*>(g.ep.gelu.table)[i];
  }
  LG_STAMP(1);
  // ---- LayerNorm -> LDS panel (and, on request, HBM)
  {
    float* sG = reinterpret_cast<float*>(lg_smem + lay.fold);
    float* sB = sG + NCH * 128;
    float* sP = sB + NCH * 128;
    int* sM = reinterpret_cast<int*>(sP + NCH * 128);
    LnLane<NCH> L;
    ln_prepare<NCH, 32>(a.ln, C, a.force_generic != 0, sG, sB, sP, sM, tid, 256, L);
    __syncthreads();        // every lane holds its folded constants in registers: the scratch (= the panel) may be overwritten
#pragma unroll 1
    for (int r = 0; r < RPH; r += 2) {
      unsigned wnext[2][NCH];
      if (r + 2 < RPH) {
        load_row(r + 2, wnext[0]);
        load_row(r + 3, wnext[1]);
      }
      unsigned wcur[2][NCH], outw2[2][NCH];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < NCH; ++i) wcur[u][i] = L.on[i] ? win[u][i] : 0u;
      ln_rows<NCH, 32, 2>(wcur, L, a.ln, C, l31, outw2);              // the pair shares one pass of the row-scalar arithmetic
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int lrow = hw * RPH + r + u;
        const unsigned (&outw)[NCH] = outw2[u];
        const long long row = (long long)m0 + lrow;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const int c = (l31 + 32 * i) * 4;
          if (c < KT * GBK)      // channels past C inside the last k-tile are zero
            *reinterpret_cast<unsigned*>(panel + (c >> 6) * (LG_BM * GBK) + lrow * GBK + ((((c & 63) >> 4) ^ ((lrow >> 2) & 3)) << 4) + (c & 15)) =
                L.on[i] ? outw[i] : 0u;
          if (a.out && L.on[i] && row < a.rows) *reinterpret_cast<unsigned*>(a.out + row * a.out_stride + c) = outw[i];
        }
      }
      if (r + 2 < RPH) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          win[0][i] = wnext[0][i];
          win[1][i] = wnext[1][i];
        }
      }
    }
  }
  LG_STAMP(2);
  __syncthreads();        // panel, constants and table are complete
  LG_STAMP(3);

  // X fragment addresses: rows l31 / 32+l31 of panel k-tile kt, chunk 2*ks + h
  const int8_t* pXa = panel + lds_off64(l31, h);
  const int8_t* pXb = panel + lds_off64(32 + l31, h);
  const int xks = (lds_off64(l31, 2 + h) - lds_off64(l31, h));           // +-32: the k-step-1 chunk of the same row
  v16i acc[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0;

  for (int j = 0; j < tiles_n; ++j) {
    const bool more = j + 1 < tiles_n;                                   // wave-uniform
    // the fragment loads are unconditional (the last tile re-requests itself): with a branch around them hipcc cannot count the
    // outstanding requests and waits vmcnt(0) at the top of every tile - i.e. for the output STORES of the tile before
    const wraw* wnext = wsrc + (long long)(more ? j + 1 : j) * 4 * NI * 64;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int off = (i >> 1) * (LG_BM * GBK) + (i & 1) * xks;
      const v4i xa = *reinterpret_cast<const v4i*>(pXa + off);
      const v4i xb = *reinterpret_cast<const v4i*>(pXb + off);
      const v4i wfi = lg_wfrag(wf[i]);
      acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wfi, xa, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wfi, xb, acc[1], 0, 0, 0);
      wf[i] = wnext[i * 64];                                             // the fragment of the next column tile, a tile ahead of its use
    }
    LG_STAMP(4 + 2 * j);
    const EpiLds* e = reinterpret_cast<const EpiLds*>(consts + j * 2 * GBN);
    {
      const uint4 nores[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
      gemm_epilogue_tile2<EPI>(acc, m0 + l31, j * GBN + 32 * wave, 32 * wave, h, g, e, nores, gtab);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][r] = 0;
    }
    LG_STAMP(5 + 2 * j);
  }
}

// ---------------------------------------------------------------------------------------------------
// K2c: the fused LayerNorm + GEMM kernel, dense form (round 3).  Same data flow as k_ln_gemm (64 rows per workgroup, LayerNorm
//   output in an LDS panel, W fragments straight from the fragment-order copy), reorganised around the two facts measured in
//   round 2 (tools/ubench/valu_rate.hip, profiles/r02_ln_gemm_timeline.txt): a wave alone on its SIMD issues one VALU
//   instruction per ~4.9 cycles, two waves one per ~2.7; and the matrix pipe sat idle through every epilogue.
//     * 8 waves (512 threads, one workgroup per CU, up to 256 registers per wave): two waves per SIMD in every phase.  The
//       LayerNorm phase runs on 16 half waves (4 rows each); in the GEMM phase wave group g = wave >> 2 owns the column tiles
//       g, g + 2, ..., so both groups stream different W tiles and run the same program half a tile apart.
//     * software pipeline across column tiles inside a wave: the MFMAs of the group's NEXT tile (second accumulator set) are
//       issued one at a time between the pieces of the CURRENT tile's epilogue - 24 half-pieces of 4-16 VALU instructions, in
//       program order, pinned with sched_barrier so hipcc cannot re-cluster them.  An MFMA holds the matrix pipe for 32 cycles
//       while the wave goes on issuing the epilogue's VALU work: the k-loop disappears under the epilogue.  Three copies of the
//       tile body: steady state (MFMAs + W prefetch for the tile after), next-to-last (MFMAs only), last (epilogue only).
//   Results are bit-identical to k_ln_gemm (same ln_prepare / ln_row, same epilogue arithmetic); k_ln_gemm stays for the
//   arithmetic GELU epilogue (scales without a table) and for launches with activation taps.
// ---------------------------------------------------------------------------------------------------
// MFMA q (0 .. 2*NI-1; k-step q>>1, row block q&1) of the next tile goes into half-piece (q*12)/NI of the 24 half-pieces
template <int NI>
__host__ __device__ constexpr int lg2_mfma_at(int hp) {
  for (int q = 0; q < 2 * NI; ++q)
    if ((q * 12) / NI == hp) return q;
  return -1;
}

// EPI: P2V_EPI_REQUANT or P2V_EPI_GELU_TAB;  KT = k-tiles of 64 channels (C <= 64*KT);  NG = wave groups (1: 4 waves, every wave all
// column tiles, two workgroups per CU; 2: 8 waves, the groups alternate column tiles, one workgroup per CU)
#ifndef LG2_LN_ROWS
#define LG2_LN_ROWS 2   /* 4 spills at C = 384 (196 B of scratch): 89.4 k against 98.6 k img/s */
#endif
// FORM 3 / 4 (LEAN, one wave group; 4: PM1): the LayerNorm phase of a launch from a frozen plan - constants folded at plan creation (LnPre)
// with `pot` proven, C == 64 * KT, no LayerNorm output to HBM.  No channel masks or clamps, post_mul == 1 (PM1) known at compile time, only
// the fast chain in the row loop (a wave in which a row fails the `fast` test of ln_scalars takes an unlikely branch to ln_apply as the general
// form runs it), row and panel offsets formed once per lane, the four sums of a row pair reduced together (half_wave_sum_pair), two register
// sets for the rows in flight instead of copies.  Same operations on the same values: bit-identical to the general form.  The lean forms are
// further values of the third template argument, not a new one: the general forms keep their names, and a body passed through a shared
// function compiles to other code (tools/kernel_resources.py --digest)
#define LG2_FORM_LEAN 3
#define LG2_FORM_LEAN_PM1 4
template <int EPI, int KT, int FORM, bool W4>
__global__ __launch_bounds__(256 * (FORM == 2 ? 2 : 1), 2) void k_ln_gemm2(LnArgs a, GemmArgs g) {
  typedef typename LgW<W4>::raw wraw;
  constexpr int NG = FORM == 2 ? 2 : 1;  // wave groups
  constexpr bool LEAN = FORM >= LG2_FORM_LEAN, PM1 = FORM == LG2_FORM_LEAN_PM1;
  constexpr int NT = 256 * NG;           // threads
  static_assert(EPI == P2V_EPI_REQUANT || EPI == P2V_EPI_GELU_TAB, "pipelined epilogues");
  static_assert(FORM >= 1 && FORM <= LG2_FORM_LEAN_PM1, "forms");
  constexpr int NCH = (KT + 1) / 2;      // 128-channel groups of a LayerNorm row
  constexpr int NI = 2 * KT;             // k-steps of 32
  extern __shared__ __attribute__((aligned(1024))) unsigned char lg_smem[];
  LG_STAMP(0);
  const int C = LEAN ? KT * GBK : a.C;
  const int cells = EPI == P2V_EPI_GELU_TAB ? g.ep.gelu.cells : 0;
  const LnGemmLds lay = ln_gemm_lds(C, g.N, NCH, cells);
  int8_t* panel = reinterpret_cast<int8_t*>(lg_smem + lay.panel);
  float* consts = reinterpret_cast<float*>(lg_smem + lay.consts);      // per column tile: colscale[128] | bias[128]
  const unsigned char* gtab = lg_smem + lay.table;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = NG == 1 ? 0 : (wave >> 2), cw = wave & 3;            // wave group (column-tile parity), 32-column block of a tile
  const int h = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.x * LG_BM;
  const int tiles_n = g.tiles_n;
  const int n_g = (tiles_n - grp + NG - 1) / NG;                       // column tiles of this group: j = grp + NG*it

  // ---- W fragments of the group's first tile (registers): element ((j*4 + cw)*NI + i)*64 + lane of 16 bytes
  const wraw* wsrc = reinterpret_cast<const wraw*>(g.W) + (long long)cw * NI * 64 + lane;
  auto wtile = [&](int it) {                                           // fragments of the group's it-th tile (clamped: loads are unconditional)
    int j = grp + NG * it;
    j = j < tiles_n ? j : tiles_n - 1;
    return wsrc + (long long)j * 4 * NI * 64;
  };
  // at C = 384 the LayerNorm phase (48 registers of per-channel constants, two rows in flight) and a whole tile of W fragments (48) do not fit
  // 256 registers together: hipcc spilled one fragment to scratch and reloaded it after the phase.  The LAST fragment of the first tile - used
  // eleven k-steps after the phase ends - is therefore requested after the LayerNorm phase
  constexpr int NI_EARLY = KT >= 6 ? NI - 1 : NI;
  wraw wf[NI];
  {
    const wraw* w0 = wtile(0);
#pragma unroll
    for (int i = 0; i < NI_EARLY; ++i) wf[i] = w0[i * 64];
  }

  // ---- the 64 rows of the residual stream: one row per half wave, 4 rows each, the second pair in flight while the first is normalised
  constexpr int RPH = LG_BM / (8 * NG);                                // rows per half wave
  static_assert(RPH % 2 == 0, "rows are processed in pairs");
  const int hw = tid >> 5;
  // 32-bit offsets from the workgroup's first row (64 rows x row stride < 2^31: checked by the launcher): the 64-bit row * stride
  // products of the first version cost ~20 VALU instructions per row pair
  const int8_t* xblk = a.x + (long long)m0 * a.row_stride;
  const int rstride = (int)a.row_stride;
  const int last_lr = (int)(a.rows - 1 - m0);                           // rows past the end re-read the last row (never stored)
  auto load_row = [&](int r, unsigned (&w)[NCH]) {
    int lr = hw * RPH + r;
    lr = lr < last_lr ? lr : last_lr;
    const int8_t* rp = xblk + lr * rstride;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (l31 + 32 * i) * 4;
      w[i] = *reinterpret_cast<const unsigned*>(rp + (c < C ? c : 0));
    }
  };
  constexpr int LR = LG2_LN_ROWS < RPH ? LG2_LN_ROWS : RPH;             // rows per LayerNorm batch (ln_rows)
  static_assert(RPH % LR == 0, "rows are processed in batches");
  unsigned win[LR][NCH];
  // LEAN: a row pair is addressed as uniform base + unsigned 32-bit lane offset, formed once per lane: the lane's first dword in the half
  // wave's first row and in the last row of the tensor (rows past the end re-read it: offsets grow with the row, so the clamp is a minimum).
  // ODD_LAST: C = 64 * KT with KT odd leaves the upper half of the last 128-channel group empty - those lanes read column 0, their mask is 0
  // and they store nothing; nothing else in the phase knows about channels past C
  constexpr bool ODD_LAST = (KT & 1) != 0;
  [[maybe_unused]] unsigned wnx[LR][NCH];                                // LEAN: the second register set of the rows in flight
  [[maybe_unused]] const bool lane_last_on = !ODD_LAST || l31 < 16;
  [[maybe_unused]] const unsigned row0_off = (unsigned)(hw * RPH * rstride + l31 * 4);
  [[maybe_unused]] const unsigned last_off = (unsigned)((last_lr < LG_BM - 1 ? last_lr : LG_BM - 1) * rstride + l31 * 4);
  [[maybe_unused]] const unsigned last_col = lane_last_on ? (unsigned)(128 * (NCH - 1)) : (unsigned)(-l31 * 4);     // added to a row offset
  auto lean_load = [&](int r, unsigned (&w)[LR][NCH]) {                  // rows r, r + 1 of the half wave (r: uniform)
#pragma unroll
    for (int u = 0; u < LR; ++u) {
      unsigned ro = row0_off + (unsigned)((r + u) * rstride);
      ro = ro < last_off ? ro : last_off;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        if (ODD_LAST && i == NCH - 1) w[u][i] = *reinterpret_cast<const unsigned*>(xblk + (ro + last_col));
        else w[u][i] = *reinterpret_cast<const unsigned*>(xblk + 128 * i + ro);
      }
    }
  };
  if constexpr (LEAN) {
    lean_load(0, win);
  } else {
#pragma unroll
    for (int u = 0; u < LR; ++u) load_row(u, win[u]);
  }
  // ---- per-column constants of the whole layer (REQUANT: 2^e folded in, see gemm_stage_epilogue) and the GELU table
  {
    const float fold = EPI == P2V_EPI_REQUANT ? g.ep.inv_s_out : (EPI == P2V_EPI_GELU_TAB ? g.ep.gelu.k : 1.0f);   // GELU_TAB: u = y * k, see gelu_tab_offset
    const float cfold = fold * (W4 ? 0.0625f : 1.0f);                   // packed int4: the accumulator holds 16 x the sum
    for (int n4 = tid; n4 < tiles_n * (GBN / 4); n4 += NT) {           // four columns per thread and turn
      const int j_ = n4 >> 5, c_ = (n4 & 31) * 4;
      const float4 cv = *reinterpret_cast<const float4*>(g.colscale + n4 * 4);   // arrays are padded to n_pad
      const float4 bv = *reinterpret_cast<const float4*>(g.bias + n4 * 4);
      *reinterpret_cast<float4*>(consts + j_ * 2 * GBN + c_) = make_float4(cv.x * cfold, cv.y * cfold, cv.z * cfold, cv.w * cfold);
      *reinterpret_cast<float4*>(consts + j_ * 2 * GBN + GBN + c_) = make_float4(bv.x * fold, bv.y * fold, bv.z * fold, bv.w * fold);
    }
    if (EPI == P2V_EPI_GELU_TAB)
      for (int i = tid; i < cells; i += NT)
        reinterpret_cast<uint2*>(lg_smem + lay.table)[i] = reinterpret_cast<const uint2*>(g.ep.gelu.table)[i];
  }
  LG_STAMP(1);
  // ---- LayerNorm -> LDS panel (and, on request, HBM)
  if constexpr (LEAN) {
    static_assert(RPH == 8 && LR == 2, "two turns of two row pairs; the panel swizzle below");
    LnLane<NCH> L;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (l31 + 32 * i) * 4;
      L.on[i] = (ODD_LAST && i == NCH - 1) ? lane_last_on : true;       // read by the unlikely branch only
      L.gm[i] = *reinterpret_cast<const float4*>(a.pre.gm + c);
      L.bt[i] = *reinterpret_cast<const float4*>(a.pre.bt + c);
      if constexpr (!PM1) L.pm[i] = L.on[i] ? *reinterpret_cast<const float4*>(a.ln.post_mul + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      L.mkf[i] = L.on[i] ? ln_scale_mask(*reinterpret_cast<const float4*>(a.ln.mask + c)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    L.gmin = a.pre.gmin;
    L.gmax = a.pre.gmax;
    L.bmax = a.pre.bmax;
    L.pot = true;             // the launcher selects this form for a.pre.pot without force_generic only
    L.pm_one = PM1;
    // panel offsets of the lane's dword in the half wave's rows 0 - 3 and 4 - 7: row lrow = hw * 8 + r swizzles the 16-byte chunk with
    // (lrow >> 2) & 3 = (2 hw + (r >> 2)) & 3; between rows of a turn and between channel groups the stride is constant
    const int pbase = (l31 >> 4) * (LG_BM * GBK) + hw * RPH * GBK + (l31 & 3) * 4;
    const int pofs[2] = {pbase + ((((l31 >> 2) & 3) ^ ((2 * hw) & 3)) << 4), pbase + 4 * GBK + ((((l31 >> 2) & 3) ^ ((2 * hw + 1) & 3)) << 4)};
    const int src_lane[2] = {(tid & 32) * 4, ((tid & 32) + 8) * 4};     // ds_bpermute address of the lanes that hold the row scalars
    // rows r, r + 1 (r = 0 or 2 within the turn) from `cur`; `nxt` receives the pair after them
    auto pair = [&](int turn, auto Rc, unsigned (&cur)[LR][NCH], unsigned (&nxt)[LR][NCH]) {
      constexpr int r = decltype(Rc)::value;
      if (r == 0 || turn == 0) lean_load(4 * turn + r + 2, nxt);
      float xq[2][NCH][4];
      int S1[2], S1k;
      unsigned S2[2], S2k;
      ln_sums<NCH>(cur[0], L, xq[0], S1[0], S2[0]);
      ln_sums<NCH>(cur[1], L, xq[1], S1[1], S2[1]);
      half_wave_sum_pair(S1, S2, S1k, S2k);                             // row u: valid in lanes 8u .. 8u + 3 (+ 16) of the half wave
      float rs, mos;
      bool fast;
      ln_scalars<NCH>(S1k, S2k, L, a.ln, C, rs, mos, fast);
      float rs_u[2], mos_u[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        rs_u[u] = __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane[u], __float_as_int(rs)));
        mos_u[u] = __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane[u], __float_as_int(mos)));
      }
      unsigned outw[2][NCH];
      // the lanes of banks 0 and 2 hold the verdicts of the four rows of this wave
      if (__builtin_expect((__builtin_amdgcn_ballot_w64(!fast) & 0x0F0F0F0F0F0F0F0Full) != 0, 0)) {
        const int fasti = fast ? 1 : 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const bool fast_u = __builtin_amdgcn_ds_bpermute(src_lane[u], fasti) != 0;
          ln_apply<NCH, 32>(xq[u], L, a.ln, l31, rs_u[u], mos_u[u], fast_u, outw[u]);
        }
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u) ln_apply<NCH, 32>(xq[u], L, a.ln, l31, rs_u[u], mos_u[u], true, outw[u]);   // the fast chain alone (L.pm_one: constant)
      }
      int8_t* prow = panel + (turn ? pofs[1] : pofs[0]);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < NCH; ++i)
          if (!(ODD_LAST && i == NCH - 1) || lane_last_on)
            *reinterpret_cast<unsigned*>(prow + (r + u) * GBK + 2 * i * (LG_BM * GBK)) = outw[u][i];
    };
#pragma unroll 1
    for (int turn = 0; turn < 2; ++turn) {
      pair(turn, std::integral_constant<int, 0>{}, win, wnx);
      pair(turn, std::integral_constant<int, 2>{}, wnx, win);
    }
  } else {
    float* sG = reinterpret_cast<float*>(lg_smem + lay.fold);
    float* sB = sG + NCH * 128;
    float* sP = sB + NCH * 128;
    int* sM = reinterpret_cast<int*>(sP + NCH * 128);
    LnLane<NCH> L;
    if (a.pre.gm) {         // folded when the plan was created (LnPre): straight into registers - no scratch, no barriers
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (l31 + 32 * i) * 4;
        L.on[i] = c < C;
        L.gm[i] = *reinterpret_cast<const float4*>(a.pre.gm + c);
        L.bt[i] = *reinterpret_cast<const float4*>(a.pre.bt + c);
        L.pm[i] = L.on[i] ? *reinterpret_cast<const float4*>(a.ln.post_mul + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        L.mkf[i] = L.on[i] ? ln_scale_mask(*reinterpret_cast<const float4*>(a.ln.mask + c)) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      L.gmin = a.pre.gmin;
      L.gmax = a.pre.gmax;
      L.bmax = a.pre.bmax;
      L.pot = a.pre.pot != 0 && a.force_generic == 0;
      L.pm_one = a.pre.pm_one != 0;
    } else {
      ln_prepare<NCH, 32>(a.ln, C, a.force_generic != 0, sG, sB, sP, sM, tid, NT, L);
      __syncthreads();      // every lane holds its folded constants in registers: the scratch (= the panel) may be overwritten
    }
#pragma unroll 1
    for (int r = 0; r < RPH; r += LR) {
      unsigned wnext[LR][NCH];
      if (r + LR < RPH) {
#pragma unroll
        for (int u = 0; u < LR; ++u) load_row(r + LR + u, wnext[u]);
      }
      unsigned wcur[LR][NCH], outw2[LR][NCH];
#pragma unroll
      for (int u = 0; u < LR; ++u)
#pragma unroll
        for (int i = 0; i < NCH; ++i) wcur[u][i] = L.on[i] ? win[u][i] : 0u;
      ln_rows<NCH, 32, LR>(wcur, L, a.ln, C, l31, outw2);             // the batch shares one pass of the row-scalar arithmetic
#pragma unroll
      for (int u = 0; u < LR; ++u) {
        const int lrow = hw * RPH + r + u;
        const unsigned (&outw)[NCH] = outw2[u];
        const long long row = (long long)m0 + lrow;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
          const int c = (l31 + 32 * i) * 4;
          if (c < KT * GBK)      // channels past C inside the last k-tile are zero
            *reinterpret_cast<unsigned*>(panel + (c >> 6) * (LG_BM * GBK) + lrow * GBK + ((((c & 63) >> 4) ^ ((lrow >> 2) & 3)) << 4) + (c & 15)) =
                L.on[i] ? outw[i] : 0u;
          if (a.out && L.on[i] && row < a.rows) *reinterpret_cast<unsigned*>(a.out + row * a.out_stride + c) = outw[i];
        }
      }
      if (r + LR < RPH) {
#pragma unroll
        for (int u = 0; u < LR; ++u)
#pragma unroll
          for (int i = 0; i < NCH; ++i) win[u][i] = wnext[u][i];
      }
    }
  }
  LG_STAMP(2);
  if constexpr (NI_EARLY < NI) wf[NI - 1] = wtile(0)[(NI - 1) * 64];
  __syncthreads();        // panel, constants and table are complete
  LG_STAMP(3);
  if (n_g <= 0) return;   // wave-uniform (a layer with a single column tile: the second group has nothing to do)

  // X fragment addresses: rows l31 / 32+l31 of panel k-tile kt, chunk 2*ks + h
  const int8_t* pXa = panel + lds_off64(l31, h);
  const int8_t* pXb = panel + lds_off64(32 + l31, h);
  const int xks = (lds_off64(l31, 2 + h) - lds_off64(l31, h));           // +-32: the k-step-1 chunk of the same row
#define LG2_XOFF(i) ((((i) >> 1) * (LG_BM * GBK)) + (((i) & 1) ? xks : 0))
  v16i acc[2], accn[2];                                                  // current tile (epilogue) / next tile (MFMAs)
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0;
  // ---- the group's first tile: plain k-loop (nothing to overlap with), W fragments of its second tile requested behind the MFMAs
  {
    const wraw* wn = wtile(1);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const v4i xa = *reinterpret_cast<const v4i*>(pXa + LG2_XOFF(i));
      const v4i xb = *reinterpret_cast<const v4i*>(pXb + LG2_XOFF(i));
      const v4i wfi = lg_wfrag(wf[i]);
      acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wfi, xa, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wfi, xb, acc[1], 0, 0, 0);
      wf[i] = wn[i * 64];
    }
  }
  LG_STAMP(4);
  // X fragments of k-step 0 for the first interleaved MFMAs (double-buffered by k-step parity; the panel is the same for every tile)
  v4i XA[2], XB[2];
  XA[0] = *reinterpret_cast<const v4i*>(pXa + LG2_XOFF(0));
  XB[0] = *reinterpret_cast<const v4i*>(pXb + LG2_XOFF(0));
  XA[1] = XA[0];
  XB[1] = XB[0];
  const int goff = (int)g.ep.gelu.off;
  const float glo = (float)-goff, ghi = (float)(cells - 1 - goff) + 0.5f;     // clamp bounds of u ahead of the floor
  const unsigned char* gtabz = gtab + goff * 8;                           // entry `off`: the cell of u in [0, 1)

  // One column tile: the epilogue of acc (tile j) in 24 half-pieces; with MF the 2*NI MFMAs of the group's next tile are issued
  // one per half-piece into accn (X fragments one k-step ahead); with LD the W fragment of the tile after next replaces the one
  // an MFMA pair has just consumed.
  v4i wcur = {0, 0, 0, 0};                                               // the widened fragment between the two MFMAs of a k-step
  // acc_ / accn_: the accumulators of this tile / of the next one.  The steady-state loop runs the body twice per turn with the two sets
  // exchanged instead of copying 32 registers per tile (COPY = false); the odd tile and the two tail forms copy the next set into the first
  auto tile_body = [&](auto MFc, auto LDc, auto COPYc, int j, const wraw* wnn, v16i (&acc)[2], v16i (&accn)[2]) {
    constexpr bool MF = decltype(MFc)::value, LD = decltype(LDc)::value, COPY = decltype(COPYc)::value;
    const float* cst = consts + j * 2 * GBN + 32 * cw + 4 * h;           // colscale of this wave's columns; bias at + GBN
    const int n_tile = j * GBN + 32 * cw;
    unsigned d[2][4];
    float4 cs = *reinterpret_cast<const float4*>(cst), bs = *reinterpret_cast<const float4*>(cst + GBN);
#define LG2_MFMA(HP)                                                                                                     \
    do {                                                                                                                 \
      constexpr int q_ = lg2_mfma_at<NI>(HP);                                                                            \
      if constexpr (MF && q_ >= 0) {                                                                                     \
        constexpr int i_ = q_ >> 1, nx_ = (i_ + 1) % NI;                                                                 \
        if constexpr ((q_ & 1) == 0) {                                                                                   \
          XA[nx_ & 1] = *reinterpret_cast<const v4i*>(pXa + LG2_XOFF(nx_));                                              \
          wcur = lg_wfrag(wf[i_]);                                                                                       \
          if constexpr (i_ == 0) accn[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wcur, XA[i_ & 1], (v16i){0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0, 0, 0); \
          else accn[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wcur, XA[i_ & 1], accn[0], 0, 0, 0);                      \
        } else {                                                                                                         \
          XB[nx_ & 1] = *reinterpret_cast<const v4i*>(pXb + LG2_XOFF(nx_));                                              \
          if constexpr (i_ == 0) accn[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wcur, XB[i_ & 1], (v16i){0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0, 0, 0); \
          else accn[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wcur, XB[i_ & 1], accn[1], 0, 0, 0);                      \
          if constexpr (LD) wf[i_] = wnn[i_ * 64];                                                                       \
        }                                                                                                                \
      }                                                                                                                  \
    } while (0)
#define LG2_FENCE() __builtin_amdgcn_sched_barrier(0)
    auto group = [&](auto GQc) {
      constexpr int gq = decltype(GQc)::value;
      const float4 csc = cs, bsc = bs;
      if (gq < 3) {                                                      // constants of the next group: an LDS round trip ahead
        cs = *reinterpret_cast<const float4*>(cst + 8 * (gq + 1));
        bs = *reinterpret_cast<const float4*>(cst + GBN + 8 * (gq + 1));
      }
      float y0[4], y1[4];
      // F.linear on fake-quantised operands: exact integer sum * (s_x*s_w[n]), then ONE rounding for the fp32 bias (layers.py:178)
      LG2_MFMA(6 * gq + 0);
      y0[0] = __builtin_fmaf((float)acc[0][4 * gq + 0], csc.x, bsc.x);
      y0[1] = __builtin_fmaf((float)acc[0][4 * gq + 1], csc.y, bsc.y);
      y0[2] = __builtin_fmaf((float)acc[0][4 * gq + 2], csc.z, bsc.z);
      y0[3] = __builtin_fmaf((float)acc[0][4 * gq + 3], csc.w, bsc.w);
      LG2_FENCE();
      LG2_MFMA(6 * gq + 1);
      y1[0] = __builtin_fmaf((float)acc[1][4 * gq + 0], csc.x, bsc.x);
      y1[1] = __builtin_fmaf((float)acc[1][4 * gq + 1], csc.y, bsc.y);
      y1[2] = __builtin_fmaf((float)acc[1][4 * gq + 2], csc.z, bsc.z);
      y1[3] = __builtin_fmaf((float)acc[1][4 * gq + 3], csc.w, bsc.w);
      LG2_FENCE();
      if constexpr (EPI == P2V_EPI_GELU_TAB) {
        uint2 e0[4], e1[4];
        LG2_MFMA(6 * gq + 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) e0[i] = *reinterpret_cast<const uint2*>(gtabz + gelu_tab_offset(y0[i], glo, ghi));
        LG2_FENCE();
        LG2_MFMA(6 * gq + 3);
#pragma unroll
        for (int i = 0; i < 4; ++i) e1[i] = *reinterpret_cast<const uint2*>(gtabz + gelu_tab_offset(y1[i], glo, ghi));
        LG2_FENCE();
        LG2_MFMA(6 * gq + 4);
        d[0][gq] = 0;
        P2V_GELU_SEL(0, "UNUSED_PAD", d[0][gq], y0[0], e0[0]);
        P2V_GELU_SEL(1, "UNUSED_PRESERVE", d[0][gq], y0[1], e0[1]);
        P2V_GELU_SEL(2, "UNUSED_PRESERVE", d[0][gq], y0[2], e0[2]);
        P2V_GELU_SEL(3, "UNUSED_PRESERVE", d[0][gq], y0[3], e0[3]);
        LG2_FENCE();
        LG2_MFMA(6 * gq + 5);
        d[1][gq] = 0;
        P2V_GELU_SEL(0, "UNUSED_PAD", d[1][gq], y1[0], e1[0]);
        P2V_GELU_SEL(1, "UNUSED_PRESERVE", d[1][gq], y1[1], e1[1]);
        P2V_GELU_SEL(2, "UNUSED_PRESERVE", d[1][gq], y1[2], e1[2]);
        P2V_GELU_SEL(3, "UNUSED_PRESERVE", d[1][gq], y1[3], e1[3]);
        LG2_FENCE();
      } else {       // REQUANT: the 2^e of the following QAct is folded into the constants; the byte packing saturates
        float r0[4], r1[4];
        LG2_MFMA(6 * gq + 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) r0[i] = pre_pack(y0[i]);
        LG2_FENCE();
        LG2_MFMA(6 * gq + 3);
#pragma unroll
        for (int i = 0; i < 4; ++i) r1[i] = pre_pack(y1[i]);
        LG2_FENCE();
        LG2_MFMA(6 * gq + 4);
        d[0][gq] = pack4_pre(r0[0], r0[1], r0[2], r0[3]);
        LG2_FENCE();
        LG2_MFMA(6 * gq + 5);
        d[1][gq] = pack4_pre(r1[0], r1[1], r1[2], r1[3]);
        LG2_FENCE();
      }
    };
    group(std::integral_constant<int, 0>{});
    group(std::integral_constant<int, 1>{});
    group(std::integral_constant<int, 2>{});
    group(std::integral_constant<int, 3>{});
#undef LG2_MFMA
#undef LG2_FENCE
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const uint4 o = halves_to_row16(d[b][0], d[b][1], d[b][2], d[b][3]);
      const int m = m0 + 32 * b + l31;
      if (m < g.M && n_tile + 16 * h < g.N)
        *reinterpret_cast<uint4*>(reinterpret_cast<int8_t*>(g.out) + (long long)m * g.ldo + n_tile + 16 * h) = o;
    }
    if constexpr (MF && COPY) {
      acc[0] = accn[0];
      acc[1] = accn[1];
    }
  };
  using T_ = std::integral_constant<bool, true>;
  using F_ = std::integral_constant<bool, false>;
  int it = 0;
  for (; it + 3 < n_g; it += 2) {
    tile_body(T_{}, T_{}, F_{}, grp + NG * it, wtile(it + 2), acc, accn);
    LG_STAMP(5 + it);
    tile_body(T_{}, T_{}, F_{}, grp + NG * (it + 1), wtile(it + 3), accn, acc);
    LG_STAMP(6 + it);
  }
  if (it + 2 < n_g) {
    tile_body(T_{}, T_{}, T_{}, grp + NG * it, wtile(it + 2), acc, accn);
    LG_STAMP(5 + it);
    ++it;
  }
  if (it + 1 < n_g) {
    tile_body(T_{}, F_{}, T_{}, grp + NG * it, wsrc, acc, accn);
    LG_STAMP(5 + it);
    ++it;
  }
  tile_body(F_{}, F_{}, T_{}, grp + NG * it, wsrc, acc, accn);
  LG_STAMP(5 + it);
#undef LG2_XOFF
}

template <int EPI, int KT, int VER, bool W4>
static int launch_ln_gemm_t(const LnArgs& a, const GemmArgs& g, int cells, hipStream_t st) {
  // VER 1: the 4-wave kernel; 2 / 3: k_ln_gemm2 with one / two wave groups; 4 / 5: its lean forms without / with post_mul == 1
  static_assert(LG2_FORM_LEAN == 3 && LG2_FORM_LEAN_PM1 == 4, "VER - 1 is the form");
  constexpr auto kernel = [] {
    if constexpr (VER == 1) return &k_ln_gemm<EPI, KT, W4>;
    else return &k_ln_gemm2<EPI, KT, VER - 1, W4>;
  }();
  const int smem = ln_gemm_lds(a.C, g.N, (KT + 1) / 2, cells).total;
  static P2vLdsGrant grant = {};
  const hipError_t e = grant.ensure(reinterpret_cast<const void*>(kernel), smem);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((g.M + LG_BM - 1) / LG_BM));
  hipLaunchKernelGGL(kernel, grid, dim3(VER == 3 ? 512 : 256), (unsigned)smem, st, a, g);
  CHECK_LAUNCH();
  return 0;
}
typedef int (*LnGemmLauncher)(const LnArgs&, const GemmArgs&, int, hipStream_t);
constexpr int kLnGemmEpi[3] = {P2V_EPI_REQUANT, P2V_EPI_GELU_TAB, P2V_EPI_GELU};
// the launcher of a lean form (p2vit_ln_lean.hip): e = REQUANT or GELU_TAB, kt = 1 .. 6
LnGemmLauncher p2v_ln_gemm_lean_launcher(int e, bool pm1, int kt, bool w4);
