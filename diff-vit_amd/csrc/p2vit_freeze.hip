// p2vit_freeze.hip -- the weight freeze on the device (p2v_freeze_weights, include/p2vit.h): fp32 weights [N][ldw] -> the codes
// clamp(rne(w / scale), lo, hi) in one of the four layouts the GEMM kernels read, zero padded to [round_up(N, 128)][round_up(K, 64)].
//
//   k_freeze<LAYOUT>   a pure streaming pass, no LDS, no barrier.  One thread owns ONE output chunk - the 16 codes of 16 consecutive k of
//                      one weight row: 16 bytes in the int8 layouts, 8 bytes in the packed ones - so consecutive threads store consecutive
//                      chunks (one coalesced 16- / 8-byte vector store each) and the layout is nothing but the map chunk -> (row, k0):
//                        ROWS_I8    chunk = n * (k_pad / 16) + k0 / 16
//                        FRAG_I8/P4 [tile][wave][k-step of 32][h][r]: n = 128 tile + 32 wave + r, k0 = 32 kstep + 16 h   (p2v_linear.w_frag)
//                        TILES_P4   [tile][k-tile of 64][row][position]: n = 128 tile + row, k0 = 64 ktile + 16 (position ^ ((row >> 3) & 3))
//                      The 16 source floats are four float4 loads where the chunk's address is 16-byte aligned and the quad lies inside the
//                      row (w is only 4-byte aligned and ldw is arbitrary), scalar loads with a bound test otherwise.  Nothing at n >= N or
//                      k >= K is read; those codes are 0.  IEEE division and rintf: what torch.round(w / s) computes for any scale.
#include "p2vit_kernels.h"

struct FreezeArgs {
  const float* w;
  long long ldw;
  int N, K;
  const float* scale;
  int per_row;          // scale[n] (n_scale == N) or scale[0]
  float lo, hi;
  int k_pad;
  long long chunks;     // n_pad * k_pad / 16
  void* out;
};

__device__ __forceinline__ int freeze_code(float x, float s, float lo, float hi) {
  return (int)fminf(fmaxf(rintf(__fdiv_rn(x, s)), lo), hi);
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void k_freeze(const FreezeArgs a) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.chunks) return;
  long long n;
  int k0;
  if (LAYOUT == P2V_W_ROWS_I8) {
    const int cpr = a.k_pad >> 4;
    n = c / cpr;
    k0 = (int)(c - n * cpr) << 4;
  } else if (LAYOUT == P2V_W_TILES_P4) {
    const int kt = a.k_pad >> 6;
    const int pos = (int)(c & 3), row = (int)((c >> 2) & 127);
    const long long t = c >> 9;                       // tile * kt + ktile
    const long long tile = t / kt;
    n = tile * 128 + row;
    k0 = ((int)(t - tile * kt) << 6) + ((pos ^ ((row >> 3) & 3)) << 4);
  } else {                                            // fragment order
    const int ks = a.k_pad >> 5;
    const int r = (int)(c & 31), h = (int)((c >> 5) & 1);
    const long long t = c >> 6;                       // (tile * 4 + wave) * ks + kstep
    const long long tw = t / ks;
    n = tw * 32 + r;                                  // 128 tile + 32 wave + r
    k0 = ((int)(t - tw * ks) << 5) + (h << 4);
  }
  int code[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) code[i] = 0;
  if (n < a.N && k0 < a.K) {
    const float s = a.scale[a.per_row ? n : 0];
    const float* __restrict__ p = a.w + n * a.ldw + k0;
    const bool aligned = ((uintptr_t)p & 15) == 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + 4 * q;
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      if (aligned && k + 4 <= a.K) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * q);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < a.K) x[j] = p[4 * q + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) code[4 * q + j] = k + j < a.K ? freeze_code(x[j], s, a.lo, a.hi) : 0;
    }
  }
  if (LAYOUT == P2V_W_ROWS_I8 || LAYOUT == P2V_W_FRAG_I8) {
    unsigned d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      d[q] = (unsigned)(code[4 * q] & 255) | (unsigned)(code[4 * q + 1] & 255) << 8 | (unsigned)(code[4 * q + 2] & 255) << 16 |
             (unsigned)(code[4 * q + 3] & 255) << 24;
    reinterpret_cast<uint4*>(a.out)[c] = make_uint4(d[0], d[1], d[2], d[3]);
  } else {                                            // byte j of dword 0 = code[j] | code[4+j] << 4, of dword 1 = code[8+j] | code[12+j] << 4
    unsigned d[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[0] |= (unsigned)((code[j] & 15) | (code[4 + j] & 15) << 4) << (8 * j);
      d[1] |= (unsigned)((code[8 + j] & 15) | (code[12 + j] & 15) << 4) << (8 * j);
    }
    reinterpret_cast<uint2*>(a.out)[c] = make_uint2(d[0], d[1]);
  }
}

// the caller (p2v_freeze_weights) has checked every argument: layout in 0 .. 3, out covers chunks * (16 | 8) bytes, chunks / 256 < 2^31
int p2v_launch_freeze_weights(const float* w, long long ldw, int N, int K, const float* scale, int n_scale, int bits, int layout, void* out,
                              hipStream_t st) {
  FreezeArgs a;
  a.w = w; a.ldw = ldw; a.N = N; a.K = K; a.scale = scale; a.per_row = n_scale != 1;
  a.lo = bits == 8 ? -128.f : -8.f; a.hi = bits == 8 ? 127.f : 7.f;
  const long long n_pad = ((long long)N + 127) / 128 * 128, k_pad = ((long long)K + 63) / 64 * 64;
  a.k_pad = (int)k_pad;
  a.chunks = n_pad * k_pad / 16;
  a.out = out;
  const dim3 grid((unsigned)((a.chunks + 255) / 256)), block(256);
  switch (layout) {
    case P2V_W_ROWS_I8: hipLaunchKernelGGL(k_freeze<P2V_W_ROWS_I8>, grid, block, 0, st, a); break;
    case P2V_W_FRAG_I8: hipLaunchKernelGGL(k_freeze<P2V_W_FRAG_I8>, grid, block, 0, st, a); break;
    case P2V_W_TILES_P4: hipLaunchKernelGGL(k_freeze<P2V_W_TILES_P4>, grid, block, 0, st, a); break;
    case P2V_W_FRAG_P4: hipLaunchKernelGGL(k_freeze<P2V_W_FRAG_P4>, grid, block, 0, st, a); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}
