// p2vit_float_ln.hip -- QIntLayerNorm in mode 'ln' (plain F.layer_norm, layers.py:241-243) followed by the division by the SmoothQuant
// channel scale and the QAct behind it, for the Config(ptf=False) plans: int8 codes in, int8 codes out.
//
// The row's input is code * s_in with ONE power-of-two s_in, so the statistics are integer sums (as in p2vit_ln_row.h) and the rest is
// stated in fp64, every operation rounded on its own (this unit is compiled without contraction, as every unit is):
//     S1 = sum q, S2 = sum q^2                                   exact integers
//     var = ((C S2 - S1^2) / (C C)) s_in s_in
//     r   = 1 / sqrt(var + eps)
//     y_c = ((((C q_c - S1) / C) s_in) r) gamma_c + beta_c
//     code_c = clamp(rne(y_c g_c), -128, 127)                    g_c = 1 / (channel_scale_c s_out), a power of two
// The order of the sums does not matter (integers), so the result does not depend on the launch geometry.  tests/_float_ops_ref.py states the
// same expression; DESIGN gives the measured distance to torch's fp32 F.layer_norm.
//
// One wave per row, four rows per workgroup; a lane takes the 4-channel groups lane, lane + 64, ... (C <= 2048: at most 8 of them).
#include "p2vit_device.h"

#define FLN_MAX_C 2048

__global__ __launch_bounds__(256) void k_float_layernorm(FloatLnArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const int C = a.C, groups = C >> 2;
  const int8_t* x = a.x + row * a.row_stride;
  int q[8];                                             // four codes each
  long long s1 = 0, s2 = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int gi = lane + 64 * k;
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
  const double Cd = (double)C;
  const double var = (((double)((long long)C * s2 - s1 * s1) / (Cd * Cd)) * a.s_in) * a.s_in;
  const double r = 1.0 / sqrt(var + a.eps);
  int8_t* out = a.out + row * a.out_stride;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int gi = lane + 64 * k;
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

// rows of up to 2048 channels: the kernel above; 2052 ... 4096: a row per workgroup (k_float_layernorm_xwide, p2vit_float_ln_xwide.hip)
int p2v_launch_float_layernorm(const FloatLnArgs& a, hipStream_t st) {
  if (a.C > FLN_MAX_C) return p2v_launch_float_layernorm_xwide(a, st);
  if (a.C < 4 || a.C % 4 || a.rows <= 0) return -1;
  hipLaunchKernelGGL(k_float_layernorm, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, st, a);
  CHECK_LAUNCH();
  return 0;
}
