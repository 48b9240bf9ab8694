// p2vit_float_ln_xwide.hip -- the float LayerNorm -> QAct of p2vit_float_ln.hip for rows of 2052 ... 4096 channels (multiples of 4): the
// PatchMerging LayerNorm of a Swin model under Config(ptf=False) behind a stage of more than 512 channels (4 * 768 = 3072 channels, Swin-L).
// k_float_layernorm gives a row to one wave, eight 4-channel groups per lane; here a row belongs to the whole workgroup:
//   - lane t of 256 owns the 4-channel groups t, t + 256, t + 512, t + 768 (C <= 4096: at most four of them), so a row is read and written
//     in fully coalesced 1 KB pieces;
//   - the arithmetic is k_float_layernorm's, unchanged: S1 = sum q and S2 = sum q^2 as exact integers, then in fp64, every operation
//     rounded on its own (this unit is compiled without contraction, as every unit is):
//         var = ((C S2 - S1^2) / (C C)) s_in s_in
//         r   = 1 / sqrt(var + eps)
//         y_c = ((((C q_c - S1) / C) s_in) r) gamma_c + beta_c
//         code_c = clamp(rne(y_c g_c), -128, 127)
//     (tests/_float_ops_ref.float_layernorm states the same expression);
//   - the lane's sums go wave-wide by shuffles, then the four wave sums through LDS, added in every lane: integers, so the totals - and
//     with them every code - do not depend on the launch geometry or on the order of the adds.
// Bounds (C <= 4096, |q| <= 128): S2 <= 2^26 and C S2 <= 2^38; |S1| <= 2^19 and S1^2 <= 2^38; |C q - S1| <= 2^19 + 2^19 < 2^32.  Every
// intermediate fits a 64-bit integer, and both numerators (C S2 - S1^2, C q - S1) are below 2^53: exact in fp64.
// Footprint: bytes [C, out_stride) of an output row and everything behind row `rows` - 1 are never written; no load passes channel C.
#include "p2vit_device.h"

#define FLX_LANES 256
#define FLX_GROUPS 4                 // 4-channel groups per lane: 256 * 4 * 4 = 4096 channels
#define FLX_MAX_C (FLX_LANES * FLX_GROUPS * 4)

__global__ __launch_bounds__(FLX_LANES) void k_float_layernorm_xwide(FloatLnArgs a) {
  __shared__ long long sRed[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long row = blockIdx.x;                    // one row per workgroup (grid = rows)
  const int C = a.C, groups = C >> 2;
  const int8_t* x = a.x + row * a.row_stride;
  int q[FLX_GROUPS];                                    // four codes each
  long long s1 = 0, s2 = 0;
#pragma unroll
  for (int k = 0; k < FLX_GROUPS; ++k) {
    const int gi = tid + FLX_LANES * k;
    q[k] = 0;
    if (gi < groups) {
      q[k] = *reinterpret_cast<const int*>(x + 4 * gi);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = (int)(int8_t)(q[k] >> (8 * e));
        s1 += v;
        s2 += v * v;
      }
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    s1 += __shfl_xor(s1, m);
    s2 += __shfl_xor(s2, m);
  }
  if (lane == 0) {
    sRed[wave][0] = s1;
    sRed[wave][1] = s2;
  }
  __syncthreads();                                      // reached by every lane: nothing above returns
  s1 = (sRed[0][0] + sRed[1][0]) + (sRed[2][0] + sRed[3][0]);
  s2 = (sRed[0][1] + sRed[1][1]) + (sRed[2][1] + sRed[3][1]);
  const double Cd = (double)C;
  const double var = (((double)((long long)C * s2 - s1 * s1) / (Cd * Cd)) * a.s_in) * a.s_in;
  const double r = 1.0 / sqrt(var + a.eps);
  int8_t* out = a.out + row * a.out_stride;
#pragma unroll
  for (int k = 0; k < FLX_GROUPS; ++k) {
    const int gi = tid + FLX_LANES * k;
    if (gi >= groups) continue;
    const float4 gm = *reinterpret_cast<const float4*>(a.gamma + 4 * gi);
    const float4 bt = *reinterpret_cast<const float4*>(a.beta + 4 * gi);
    const float4 gg = *reinterpret_cast<const float4*>(a.g + 4 * gi);
    const float gmv[4] = {gm.x, gm.y, gm.z, gm.w}, btv[4] = {bt.x, bt.y, bt.z, bt.w}, ggv[4] = {gg.x, gg.y, gg.z, gg.w};
    float yv[4];
    unsigned w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long v = (long long)(int8_t)(q[k] >> (8 * e));
      const double y = ((((double)((long long)C * v - s1) / Cd) * a.s_in) * r) * (double)gmv[e] + (double)btv[e];
      yv[e] = (float)y;
      double c = rint(y * (double)ggv[e]);
      c = c < -128.0 ? -128.0 : (c > 127.0 ? 127.0 : c);      // (a NaN cannot arise: eps > 0)
      w |= ((unsigned)(int)c & 255u) << (8 * e);
    }
    *reinterpret_cast<unsigned*>(out + 4 * gi) = w;
    if (a.tap_out) *reinterpret_cast<float4*>(a.tap_out + row * C + 4 * gi) = make_float4(yv[0], yv[1], yv[2], yv[3]);
  }
}

int p2v_launch_float_layernorm_xwide(const FloatLnArgs& a, hipStream_t st) {
  if (a.C <= 2048 || a.C > FLX_MAX_C || a.C % 4 || a.rows <= 0 || a.rows > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(k_float_layernorm_xwide, dim3((unsigned)a.rows), dim3(FLX_LANES), 0, st, a);
  CHECK_LAUNCH();
  return 0;
}
