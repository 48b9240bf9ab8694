// p2vit_attn_softmax.hip -- ViT attention with the FLOAT softmax of Config(lis=False) (QIntSoftmax with log_i_softmax = False: plain softmax of
// the dequantised qact_attn1 codes, not quantized, layers.py:387-395), restated on integers, for head_dim 32 / 64 and 1 .. P2V_MAX_TOKENS tokens.
//
// Structure of k_lis_attention_packed (p2vit_attn_packed.hip): one workgroup per (image, head), K and V^T of the head as int8 in LDS, a wave owns
// 16-query blocks, S^T = K . Q^T on v_mfma_i32_16x16x64_i8, the scores of 64 keys requantised at once to the negated qact_attn1 codes and kept
// as bytes nc + 127 four to a register, then the row maximum.  From there:
//     d_ij = max_j c_ij - c_ij in [0, 255],   E_ij = tab[d_ij]                       tab: 256 entries below 2^21, built by the plan (fp64 exp on the host)
//     num_ic = sum_j E_ij v_jc,  den_i = sum_j E_ij                                  exact integers
//     code_ic = clamp(rne((double(num_ic) / double(den_i)) av_mul), -128, 127)       one IEEE fp64 division; av_mul a power of two
// E splits into three 7-bit digits E = e0 + 128 e1 + 16384 e2, each a non-negative int8: three B operands of the 64-deep int8 MFMA against
// V^T, three int32 accumulators per 16-channel tile (|sum| <= 640 * 127 * 128 < 2^24), recombined in int64 (|num| < 2^39: exact as fp64).
// den_i <= 640 * 2^21 < 2^31 is summed in 32 unsigned bits.  Padded keys read the table's entry 256 = 0.  den_i >= tab[0] > 0 is the plan's
// (and the entry point's) to check.
// head_dim 32: K rows and the Q fragment are padded with zeros to the 64-deep contraction; V^T has 32 channel rows per key group.
//
// Optional tap: the qact_attn1 codes 127 - byte of every real (query, key) pair into a pitched plane (p2v_lis_attention_taps' score_codes).
#include "p2vit_device.h"
#include "p2vit_launch.h"

extern int g_attn_waves;     // P2V_ATTN_WAVES

template <int HD, int NG>
__global__ __launch_bounds__(512, 2) void k_softmax_attention(SmAttnArgs a) {
  static_assert((HD == 32 || HD == 64) && NG >= 1 && NG * 64 <= 640, "instantiation");
  constexpr int KROWS = NG * 64, NDT = HD / 16, NCH = HD / 16;      // NCH: 16-byte chunks of a real K / V row
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int8_t* sK = reinterpret_cast<int8_t*>(smem);                  // [KROWS][64] swizzled (columns [HD, 64) zero)
  unsigned char* sVt = smem + KROWS * 64;                        // [NG][HD channels][64 keys in operand order] swizzled
  unsigned* sTab = reinterpret_cast<unsigned*>(smem + KROWS * 64 + KROWS * HD);      // [257]
  typedef __attribute__((address_space(3))) const unsigned* lds_u32p;
  const int ebase = (int)(unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)reinterpret_cast<unsigned char*>(sTab);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int nwaves = (int)(blockDim.x >> 6);
  const int b = blockIdx.x / a.H, head = blockIdx.x % a.H;
  const int N = a.N, D = a.H * HD, ld = 3 * D;
  const int8_t* base = a.qkv + (long long)b * N * ld + head * HD;

  if (tid < 256) sTab[tid] = a.tab[tid];
  if (tid == 0) sTab[256] = 0u;

  // staging (k_lis_attention_packed's): a wave takes a 64-key group per turn; lane = (channel chunk c, key quad (j, g))
  {
    const int c = lane & 3, j = (lane >> 2) & 3;
    for (int grp = wave; grp < NG; grp += nwaves) {
      const int row0 = grp * 64 + 16 * j + 4 * g;
      uint4 kv[4], vv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        kv[u] = make_uint4(0, 0, 0, 0);
        vv[u] = make_uint4(0, 0, 0, 0);
        if (row0 + u < N && c < NCH) {
          kv[u] = *reinterpret_cast<const uint4*>(base + (long long)(row0 + u) * ld + D + c * 16);
          vv[u] = *reinterpret_cast<const uint4*>(base + (long long)(row0 + u) * ld + 2 * D + c * 16);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = row0 + u;
        *reinterpret_cast<uint4*>(sK + row * 64 + ((c ^ (((row >> 3) & 1) << 1)) << 4)) = kv[u];
      }
      if (c < NCH) {
        const unsigned vw[4][4] = {{vv[0].x, vv[0].y, vv[0].z, vv[0].w}, {vv[1].x, vv[1].y, vv[1].z, vv[1].w},
                                   {vv[2].x, vv[2].y, vv[2].z, vv[2].w}, {vv[3].x, vv[3].y, vv[3].z, vv[3].w}};
#pragma unroll
        for (int w = 0; w < 4; ++w) {                  // channels 16 c + 4 w + 0 .. 3: a 4 x 4 byte transposition
          const unsigned t0 = __builtin_amdgcn_perm(vw[1][w], vw[0][w], 0x05010400u);
          const unsigned t1 = __builtin_amdgcn_perm(vw[1][w], vw[0][w], 0x07030602u);
          const unsigned t2 = __builtin_amdgcn_perm(vw[3][w], vw[2][w], 0x05010400u);
          const unsigned t3 = __builtin_amdgcn_perm(vw[3][w], vw[2][w], 0x07030602u);
          const unsigned col[4] = {__builtin_amdgcn_perm(t2, t0, 0x05040100u), __builtin_amdgcn_perm(t2, t0, 0x07060302u),
                                   __builtin_amdgcn_perm(t3, t1, 0x05040100u), __builtin_amdgcn_perm(t3, t1, 0x07060302u)};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int ch = 16 * c + 4 * w + e;
            const int pos = g ^ ((w >> 1) << 1) ^ c;
            *reinterpret_cast<unsigned*>(sVt + grp * (HD * 64) + ch * 64 + pos * 16 + 4 * j) = col[e];
          }
        }
      }
    }
  }

  const float nmm = -(a.qk_scale * (a.s_qkv_sq * a.inv_s_attn));          // the NEGATED code is produced, see k_lis_attention
  const double avm = (double)a.av_mul;
  const int nqb = ((a.nq > 0 && a.nq < N ? a.nq : N) + 15) >> 4;
  __syncthreads();

  const int ksw = ((l15 >> 3) & 1) << 1;
  const int8_t* kfrag = sK + l15 * 64 + ((g ^ ksw) << 4);                 // + 1024 per 16-key block
  for (int qb = wave; qb < nqb; qb += nwaves) {
    const int qrow = qb * 16 + l15;
    v4i fq = {0, 0, 0, 0};
    if (g < NCH) fq = *reinterpret_cast<const v4i*>(base + (long long)(qrow < N ? qrow : N - 1) * ld + g * 16);

    // ---- scores -> bytes nc + 127, group by group
    unsigned codes[NG][4];
    float mnf = 255.f;
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
      v4i sc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        sc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(kfrag + (grp * 4 + j) * 1024), fq, (v4i){0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned w = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = __builtin_amdgcn_fmed3f(rintf((float)sc[j][r] * nmm), -127.f, 128.f) + 127.f;      // nc + 127 in [0, 255]
          if (grp == NG - 1) x = grp * 64 + 16 * j + 4 * g + r < N ? x : 255.f;                        // padding: out of the row minimum
          mnf = fminf(mnf, x);
          w = __builtin_amdgcn_cvt_pk_u8_f32(x, r, w);
        }
        codes[grp][j] = w;
      }
    }
    int mn = (int)mnf;                                                    // min of nc + 127 = 127 - (row max of the codes)
    {
      int o = __shfl_xor(mn, 16);
      mn = o < mn ? o : mn;
      o = __shfl_xor(mn, 32);
      mn = o < mn ? o : mn;
    }
    if (a.score_codes && qrow < N) {                                      // the tap: code = 127 - byte, columns [0, N) only
      int8_t* dst = a.score_codes + (((long long)b * a.H + head) * N + qrow) * a.pitch;
#pragma unroll
      for (int grp = 0; grp < NG; ++grp)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int key = grp * 64 + 16 * j + 4 * g;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (key + r < N) dst[key + r] = (int8_t)(127 - (int)((codes[grp][j] >> (8 * r)) & 255u));
        }
    }

    // ---- E = tab[byte - mn] as three 7-bit digit planes, P.V on the int8 MFMA; 4 d + c0 is the absolute LDS address of the entry
    const int c0 = ebase - 4 * mn;
    v4i o0[NDT], o1[NDT], o2[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o0[dt] = o1[dt] = o2[dt] = (v4i){0, 0, 0, 0};
    unsigned den = 0;
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
      v4i p0, p1, p2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned cw = codes[grp][j];
        unsigned w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int d4 = (int)(((cw >> (8 * r)) & 255u) << 2) + c0;
          if (grp == NG - 1) d4 = grp * 64 + 16 * j + 4 * g + r < N ? d4 : ebase + 1024;
          const unsigned E = *(lds_u32p)(uintptr_t)(unsigned)d4;
          den += E;
          w0 |= (E & 127u) << (8 * r);
          w1 |= ((E >> 7) & 127u) << (8 * r);
          w2 |= ((E >> 14) & 127u) << (8 * r);
        }
        p0[j] = (int)w0;
        p1[j] = (int)w1;
        p2[j] = (int)w2;
      }
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const v4i va = *reinterpret_cast<const v4i*>(sVt + grp * (HD * 64) + (dt * 16 + l15) * 64 + ((g ^ ksw ^ dt) << 4));
        o0[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, p0, o0[dt], 0, 0, 0);
        o1[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, p1, o1[dt], 0, 0, 0);
        o2[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, p2, o2[dt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    const double dend = (double)den;

    // qact2; lane owns channels 16 dt + 4 g .. + 3 of query l15.  Unconditional stores: a padding query row was computed from the Q fragment
    // of row N - 1, so its values ARE row N - 1's (see k_lis_attention)
    {
      const int qs = qrow < N ? qrow : N - 1;
      int8_t* dst = a.out + ((long long)b * N + qs) * D + head * HD + 4 * g;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        unsigned w = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long num = (long long)o0[dt][r] + 128LL * (long long)o1[dt][r] + 16384LL * (long long)o2[dt][r];
          double c = rint(((double)num / dend) * avm);
          c = c < -128.0 ? -128.0 : (c > 127.0 ? 127.0 : c);
          w |= ((unsigned)(int)c & 255u) << (8 * r);
        }
        *reinterpret_cast<unsigned*>(dst + dt * 16) = w;
      }
    }
  }
}

template <int HD, int NG>
static int launch_softmax_t(const SmAttnArgs& a, hipStream_t st) {
  constexpr size_t smem = (size_t)NG * 64 * (64 + HD) + 260 * 4;
  static_assert(smem <= 160 * 1024, "LDS of a CU");
  static P2vLdsGrant grant = {};
  if (smem > 64 * 1024) {
    const hipError_t e = grant.ensure(reinterpret_cast<const void*>(&k_softmax_attention<HD, NG>), (int)smem);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((k_softmax_attention<HD, NG>), dim3((unsigned)(a.B * a.H)), dim3(64 * g_attn_waves), smem, st, a);
  CHECK_LAUNCH();
  return 0;
}

// the launchers by (head_dim 64 first, ceil(tokens / 64) = 1 .. 10): index = 10 * (head_dim == 32) + groups - 1
typedef int (*SoftmaxLauncher)(const SmAttnArgs&, hipStream_t);
constexpr int softmax_index(int hd, int ng) { return 10 * (hd == 32 ? 1 : 0) + ng - 1; }
struct SoftmaxAt {
  template <int I> static constexpr SoftmaxLauncher at() {
    constexpr int hd = I < 10 ? 64 : 32, ng = I % 10 + 1;
    static_assert(softmax_index(hd, ng) == I, "index function");
    return launch_softmax_t<hd, ng>;
  }
};
static const auto softmax_table = p2v_table<SoftmaxLauncher, SoftmaxAt, 20>();

int p2v_launch_softmax_attention(const SmAttnArgs& a, int head_dim, hipStream_t st) {
  if ((head_dim != 32 && head_dim != 64) || a.N < 1 || a.N > P2V_MAX_TOKENS || a.B * a.H <= 0) return -1;
  return softmax_table[softmax_index(head_dim, (a.N + 63) / 64)](a, st);
}
