// p2vit_ln_xwide.hip -- integer LayerNorm for rows of 2049 ... 4096 channels: the PatchMerging LayerNorm behind a 768-channel stage
// (4 * 768 = 3072 channels, Swin-L).  k_int_layernorm (p2vit_ln.hip) gives a row to one wave and keeps the row's constants in that
// wave's registers; at twelve to sixteen 256-channel groups that no longer fits 256 VGPRs.  Here a row belongs to the whole
// workgroup:
//   - lane t of 256 owns channels (t + 256 i) * 4 .. +3 for i < NCH, NCH = 3 (C <= 3072) or 4 (C <= 4096): a row is read and written
//     as NCH fully coalesced 1 KB pieces;
//   - the lane's gamma / out_scale and beta / out_scale stay in registers, post_mul and the PTF mask are re-read from LDS where they
//     are used (LnLane<NCH, true>), and the workgroup walks `rows_per_half` consecutive rows, so the constants are staged once;
//   - the arithmetic is the other kernels', code for code (p2vit_ln_row.h): ln_sums, then the row sums wave -> workgroup as INTEGERS
//     (int sum x_q, unsigned sum x_q^2) through LDS, so the totals do not depend on the order of the adds, then ln_scalars and
//     ln_apply in every lane.  Both chains (fast / generic, with the IEEE division of out_scale != NULL) and both constant sources
//     (p2v_ln.pre / the per-workgroup fold) come with those helpers;
//   - one barrier per row: the four wave sums of row r go to slot r & 1, so the writes of row r + 1 cannot meet the reads of row r,
//     and a wave reaches the writes of row r + 2 only through the barrier of row r + 1, behind every read of row r;
//   - row r + 1 is requested before the sums of row r and first touched before the stores of row r (as in k_int_layernorm).
// Exactness: sum x_q^2 <= C * (128 * mask_max)^2 must stay below 2^32 (mask 8 up to C = 4092, mask <= 4 at C = 4096) - the callers'
// bound (SwinPlan._ln).  No signed value ever holds it: the lane's part is <= 2^24, the adds are unsigned.
// Footprint: bytes [C, out_stride) of a row and rows >= `rows` are never written; loads past C re-read column 0, loads past the last
// row re-read the last row.
#include "p2vit_ln_row.h"

#define LX_LANES 256

template <int NCH, bool PRE>        // PRE: the constants were folded ahead of the launch (p2v_ln.pre)
__global__ __launch_bounds__(LX_LANES) void k_int_layernorm_xwide(LnArgs a) {
  constexpr int CP = NCH * LX_LANES * 4;          // channels the lanes cover
  // post_mul | mask | (fold only: gamma*io | beta*io, dead once every lane holds its own in registers) ; the row-sum slots and the
  // fold's extremes lie behind the mask: 48 KB + 128 B (PRE, NCH = 3) ... 64 KB (fold, NCH = 4)
  __shared__ __attribute__((aligned(16))) float smem[PRE ? 2 * CP + 32 : 4 * CP];
  float* sP = smem;
  int* sM = reinterpret_cast<int*>(smem + CP);
  int* sRed = reinterpret_cast<int*>(smem + 2 * CP);       // [2 slots][4 waves][S1, S2], then [4 waves][gmin, gmax, bmax]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  LnLane<NCH, true> L;
  const long long row0 = (long long)blockIdx.x * a.rows_per_half;        // (here: consecutive rows per WORKGROUP)
  const long long last_row = a.rows - 1;
  const long long row_end = row0 + a.rows_per_half < a.rows ? row0 + a.rows_per_half : a.rows;
  int colofs[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) colofs[i] = (tid + LX_LANES * i) * 4 < a.C ? (tid + LX_LANES * i) * 4 : 0;     // clamped: loads are unconditional
  // the first row is requested before the constants are staged: one memory round trip covers both
  unsigned wnext[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) wnext[i] = *reinterpret_cast<const unsigned*>(a.x + (row0 < a.rows ? row0 : last_row) * a.row_stride + colofs[i]);
  if constexpr (PRE) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {   // (the folded arrays are padded to a multiple of 256 channels, not to CP: guarded)
      const int c = (tid + LX_LANES * i) * 4;
      L.on[i] = c < a.C;
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), bv = gv, pmv = gv, mk = gv;
      if (L.on[i]) {
        gv = *reinterpret_cast<const float4*>(a.pre.gm + c);
        bv = *reinterpret_cast<const float4*>(a.pre.bt + c);
        pmv = *reinterpret_cast<const float4*>(a.ln.post_mul + c);
        mk = *reinterpret_cast<const float4*>(a.ln.mask + c);
      }
      L.gm[i] = gv;
      L.bt[i] = bv;
      *reinterpret_cast<float4*>(sP + c) = pmv;              // read back by this lane alone
      *reinterpret_cast<float4*>(sM + c) = ln_scale_mask(mk);
    }
    L.sPl = sP + tid * 4;
    L.sMl = reinterpret_cast<const float*>(sM) + tid * 4;
    L.cstride = LX_LANES * 4;
    L.gmin = a.pre.gmin;
    L.gmax = a.pre.gmax;
    L.bmax = a.pre.bmax;
    L.pot = a.pre.pot != 0 && a.force_generic == 0;
    L.pm_one = a.pre.pm_one != 0;
    __syncthreads();
  } else {
    ln_prepare<NCH, LX_LANES>(a.ln, a.C, a.force_generic != 0, smem + 2 * CP, smem + 3 * CP, sP, sM, tid, LX_LANES, L);
    __syncthreads();                  // every lane holds its gamma*io / beta*io: their LDS copies may be overwritten
    // ln_prepare leaves the extremes of the lane's wave: combine the four waves (min / max: any order gives the same value)
    int* sExt = sRed + 16;
    if (lane == 0) {
      sExt[wave * 3 + 0] = (int)__float_as_uint(L.gmin);
      sExt[wave * 3 + 1] = (int)__float_as_uint(L.gmax);
      sExt[wave * 3 + 2] = (int)__float_as_uint(L.bmax);
    }
    __syncthreads();
    int lo = sExt[0], hi = sExt[1], bh = sExt[2];           // positive floats order like their bit patterns
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      lo = min(lo, sExt[w * 3 + 0]);
      hi = max(hi, sExt[w * 3 + 1]);
      bh = max(bh, sExt[w * 3 + 2]);
    }
    L.gmin = __uint_as_float((unsigned)lo);
    L.gmax = __uint_as_float((unsigned)hi);
    L.bmax = __uint_as_float((unsigned)bh);
  }
  // Row r+1 is requested at the top of the iteration of row r and first touched just before the stores of row r; the empty asm
  // statements pin that placement (see k_int_layernorm).
#pragma unroll
  for (int i = 0; i < NCH; ++i) asm volatile("" : "+v"(wnext[i]));
  int slot = 0;
#pragma unroll 1
  for (long long row = row0; row < row_end; ++row) {        // uniform in the workgroup: the barrier below is reached by all or none
    unsigned wcur[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) wcur[i] = L.on[i] ? wnext[i] : 0u;
    const long long nrow = row + 1 < a.rows ? row + 1 : last_row;
#pragma unroll
    for (int i = 0; i < NCH; ++i) wnext[i] = *reinterpret_cast<const unsigned*>(a.x + nrow * a.row_stride + colofs[i]);
    asm volatile("" ::: "memory");                 // the loads stay above this line
    float xq[NCH][4], rs, mos;
    int S1;
    unsigned S2;
    bool fast;
    ln_sums<NCH>(wcur, L, xq, S1, S2);
    ln_reduce<64>(S1, S2);                          // the wave's sums, in every lane
    int* red = sRed + slot * 8;
    if (lane == 0) {
      red[wave * 2 + 0] = S1;
      red[wave * 2 + 1] = (int)S2;                  // (the bits; added as unsigned below)
    }
    __syncthreads();
    const int4 ra = *reinterpret_cast<const int4*>(red), rb = *reinterpret_cast<const int4*>(red + 4);
    S1 = (ra.x + ra.z) + (rb.x + rb.z);
    S2 = ((unsigned)ra.y + (unsigned)ra.w) + ((unsigned)rb.y + (unsigned)rb.w);
    slot ^= 1;
    ln_scalars<NCH>(S1, S2, L, a.ln, a.C, rs, mos, fast);
    unsigned outw[NCH];
    ln_apply<NCH, LX_LANES>(xq, L, a.ln, tid, rs, mos, fast, outw);
#pragma unroll
    for (int i = 0; i < NCH; ++i) asm volatile("" : "+v"(wnext[i]));     // the wait for the next row lands here, ahead of the stores
    int8_t* dst = a.out + row * a.out_stride;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (L.on[i]) *reinterpret_cast<unsigned*>(dst + (tid + LX_LANES * i) * 4) = outw[i];
  }
}

// rows per workgroup: enough to spread the 48 - 64 KB of staged constants over several rows, few enough to fill the device - two
// resident workgroups on each of 256 CUs take ceil(rows / 512) rows each once there are more than 4096 rows
int p2v_launch_layernorm_xwide(const LnArgs& a_, hipStream_t st) {
  if (a_.C <= 2048 || a_.C > 4096 || a_.C % 4 || a_.rows <= 0) return -1;
  LnArgs a = a_;
  const long long per = (a.rows + 511) / 512;
  a.rows_per_half = (int)(per > 8 ? per : 8);
  dim3 grid((unsigned)((a.rows + a.rows_per_half - 1) / a.rows_per_half)), block(LX_LANES);
  // [groups of 1024 channels - 3][constants folded by the kernel]
  static void (*const table[2][2])(LnArgs) = {{k_int_layernorm_xwide<3, true>, k_int_layernorm_xwide<3, false>},
                                              {k_int_layernorm_xwide<4, true>, k_int_layernorm_xwide<4, false>}};
  hipLaunchKernelGGL(table[a.C <= 3072 ? 0 : 1][a.pre.gm ? 0 : 1], grid, block, 0, st, a);
  CHECK_LAUNCH();
  return 0;
}
