// p2vit_attn_packed.hip -- the ViT log-int-softmax attention for 609 .. P2V_MAX_TOKENS_PACKED tokens per image at head_dim 64: K and V of the
// head stay resident in LDS as in k_lis_attention (p2vit_attn_lis.h), where that kernel's registers and its bf16 V^T no longer fit.
//
// Structure of k_lis_attention: one workgroup per (image, head), eight waves, K and V^T staged once, a wave owns 16-query blocks,
// S^T = K . Q^T on v_mfma_i32_16x16x64_i8 (a score row on the 4 lanes {q, q+16, q+32, q+48}), the 257-entry exp_int table with its fp64
// reciprocals, the exact int64 row sum, the one-multiply fp64 quotient, log_round, the Q fragment requested one block ahead, unconditional
// stores.  Two things differ:
//
// (a) Score codes packed four to a register.  v4i s[NKB] would be 304 registers at 1216 keys.  The keys go in groups of 64 (four 16-key
//     blocks = four MFMAs); the scores of a group are requantised at once to the NEGATED qact_attn1 codes nc in [-127, 128] (the fp32 chain
//     of the streaming kernel: exact for any multiplier) and kept as the bytes nc + 127, four to a register: codes[group][j] byte r is key
//     64 group + 16 j + 4 g + r of lane (q, g) - 4 registers per group, 76 at 1216 keys.  The array is indexed by compile-time constants
//     only (a runtime index would send it to scratch), hence the template over the number of groups NG = ceil(tokens / 64), 10 .. 19; a
//     launch pads by fewer than 64 keys and only the last group tests key < N (padding -> the sentinel entry 256).
//
// (b) V^T as int8 and P.V on the int8 MFMA: K plus V^T cost 128 bytes per key, 155 648 B at 1216 keys, + 4 128 B of tables = 159 776 B of the
//     CU's 163 840.  The probability p = 2^-k, 0 <= k <= 15 (0 from k = 16 on), is the 16-bit integer h = p 2^15 = 0x8000 >> k, split into two
//     int8 planes of its NEGATIVE -h (negative because +128 is no int8):
//         A = -2^(7-k) for k <= 7, else 0;      B = -2^(15-k) for 8 <= k <= 15, else 0;      p = -(256 A + B) 2^-15  exactly,
//     both in [-128, -1] u {0}.  In 16-bit arithmetic n = -h has the low byte B (as int8) and (n + 0x80) the high byte A.  Then
//         sum_j p_j v_j = -(256 sum_j A_j v_j + sum_j B_j v_j) 2^-15:
//     two v_mfma_i32_16x16x64_i8 per 64 keys and 16-channel tile, both sums exact in int32.
//     Bound.  log_round gives 2^k >= ratio / 1.5 (the exponent is rounded up from a significand of 1.5 on).  ratio = rint(x) with
//     x = RN32(Sf / e_j) >= 1, Sf = RN32(S), S = sum_j e_j:  rint(x) >= x - 0.5 >= x / 1.5 for x >= 1.5, and for x < 1.5 the ratio is 1, k = 0,
//     p = 1 < 2.25 / x.  So p_j <= 2.25 / x_j <= 2.25 (e_j / S) (1 - 2^-24)^-2 and  sum_j p_j <= 2.25 (1 + 2^-22)  (largest seen on the CPU oracle: 1.496, the all-equal rows of the saturation tests).
//     With |v| <= 128:  |256 sum A v + sum B v| = 2^15 |sum p v| <= 2.25 (1 + 2^-22) 2^15 2^7 < 0.5625 * 2^24 + 3 < 2^24, and each plane sum
//     alone is no larger.  The combined integer is therefore exact in int32 AND as fp32, i.e. it is the real number k_lis_attention's fp32
//     accumulator holds (there in units of 2^-126), and the same single rounding follows: pack4_rne_sat(o * av_mul).
//
// Operand layout.  The score accumulators of a group leave lane (q, g) with keys 16 j + 4 g + r (j, r = 0 .. 3): exactly the 16 bytes of the
// B operand of the 64-deep MFMA, formal k index 16 g + 4 j + r  <->  key 16 j + 4 g + r.  V^T is staged with the keys of each group in that
// order, as [group][channel][64 B], so a channel row's A fragment is one 16-byte read.  Staging transposes bytes in registers: a thread
// takes 4 consecutive keys x 16 channels (four 16-byte loads), turns them with v_perm_b32 into 16 dwords (one channel, 4 keys each) and
// stores dwords.
// LDS banks.  K rows and V^T tiles are both rows of 64 B read as 16 rows x chunk g with ds_read_b128 (four 16-lane groups, bank = dword mod
// 64): chunk' = chunk ^ (((row >> 3) & 1) << 1) makes every group touch each bank once - k_lis_attention's swizzle.  V^T adds ^ (channel >> 4):
// uniform over a read (one channel tile), and it spreads the staging stores (ds_write_b32, bank = dword mod 32) of the four channel chunks
// that share a wave over 16 banks (2-way = no extra cycles) instead of 8.
//
// Softmax width (KLIM = 2^softmax_bits, 16 or 8): a template dimension here, because the clamp is part of the per-score shift.  At KLIM = 8 the
// probability is 0 from k = 8 on, so plane B is zero everywhere and its MFMAs and byte permutes are not issued; KLIM = 16 is the code it was.
//
// Not here: the probs_k tap (those launches keep the streaming kernel) and every other head_dim.
#include "p2vit_attn_lis.h"

template <int NG, int KLIM>
__global__ __launch_bounds__(512, 2) void k_lis_attention_packed(AttnKArgs a) {
  static_assert(NG >= 1 && NG * 64 <= P2V_MAX_TOKENS_PACKED, "key groups");
  static_assert(KLIM == 8 || KLIM == 16, "2^softmax_bits");
  constexpr int HD = 64, KROWS = NG * 64, NDT = HD / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int8_t* sK = reinterpret_cast<int8_t*>(smem);                  // [KROWS][64] swizzled
  unsigned char* sVt = smem + KROWS * HD;                        // [NG][64 channels][64 keys in operand order] swizzled
  unsigned char* lutE = smem + 2 * KROWS * HD;                   // [257] long long
  unsigned char* lutFR = lutE + 258 * 8;                         // [257] double, addressed by the same byte offset 8 d
  typedef __attribute__((address_space(3))) const long long* lds_i64p;
  typedef __attribute__((address_space(3))) const double* lds_f64p;
  const int ebase = (int)(unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lutE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int nwaves = (int)(blockDim.x >> 6);
  const int b = blockIdx.x / a.H, head = blockIdx.x % a.H;
  const int N = a.N, D = a.H * HD, ld = 3 * D;
  const int8_t* base = a.qkv + (long long)b * N * ld + head * HD;

  if (tid < 256) lis_table_entry(a.at, tid, reinterpret_cast<long long*>(lutE), reinterpret_cast<double*>(lutFR));
  if (tid == 0) lis_table_entry(a.at, 256, reinterpret_cast<long long*>(lutE), reinterpret_cast<double*>(lutFR));       // (four waves = 256 threads may be all there are)

  // staging: a wave takes a 64-key group per turn; lane = (channel chunk c, key quad (j, g)): keys 64 grp + 16 j + 4 g + 0 .. 3, channels 16 c + 0 .. 15.
  // All eight loads are requested before the first LDS store waits for one.
  {
    const int c = lane & 3, j = (lane >> 2) & 3;
    for (int grp = wave; grp < NG; grp += nwaves) {
      const int row0 = grp * 64 + 16 * j + 4 * g;
      uint4 kv[4], vv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        kv[u] = make_uint4(0, 0, 0, 0);
        vv[u] = make_uint4(0, 0, 0, 0);
        if (row0 + u < N) {
          kv[u] = *reinterpret_cast<const uint4*>(base + (long long)(row0 + u) * ld + D + c * 16);
          vv[u] = *reinterpret_cast<const uint4*>(base + (long long)(row0 + u) * ld + 2 * D + c * 16);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = row0 + u;
        *reinterpret_cast<uint4*>(sK + row * HD + ((c ^ (((row >> 3) & 1) << 1)) << 4)) = kv[u];
      }
      const unsigned vw[4][4] = {{vv[0].x, vv[0].y, vv[0].z, vv[0].w}, {vv[1].x, vv[1].y, vv[1].z, vv[1].w},
                                 {vv[2].x, vv[2].y, vv[2].z, vv[2].w}, {vv[3].x, vv[3].y, vv[3].z, vv[3].w}};
#pragma unroll
      for (int w = 0; w < 4; ++w) {                  // channels 16 c + 4 w + 0 .. 3: a 4 x 4 byte transposition
        const unsigned t0 = __builtin_amdgcn_perm(vw[1][w], vw[0][w], 0x05010400u);     // k0.b0 k1.b0 k0.b1 k1.b1
        const unsigned t1 = __builtin_amdgcn_perm(vw[1][w], vw[0][w], 0x07030602u);     // k0.b2 k1.b2 k0.b3 k1.b3
        const unsigned t2 = __builtin_amdgcn_perm(vw[3][w], vw[2][w], 0x05010400u);
        const unsigned t3 = __builtin_amdgcn_perm(vw[3][w], vw[2][w], 0x07030602u);
        const unsigned col[4] = {__builtin_amdgcn_perm(t2, t0, 0x05040100u), __builtin_amdgcn_perm(t2, t0, 0x07060302u),
                                 __builtin_amdgcn_perm(t3, t1, 0x05040100u), __builtin_amdgcn_perm(t3, t1, 0x07060302u)};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ch = 16 * c + 4 * w + e;         // (ch >> 3) & 1 = w >> 1, ch >> 4 = c
          const int pos = g ^ ((w >> 1) << 1) ^ c;
          *reinterpret_cast<unsigned*>(sVt + grp * 4096 + ch * 64 + pos * 16 + 4 * j) = col[e];
        }
      }
    }
  }

  // the NEGATED code is produced (round-half-even and the clamp are symmetric), see k_lis_attention
  const float nmm = -(a.at.qk_scale * (a.at.s_qkv_sq * a.at.inv_s_attn));
  const float avm = a.at.av_mul * 0x1p-15f;                               // the planes carry p 2^15; a power of two >= 2^-55: exact
  const int nqb = ((a.nq > 0 && a.nq < N ? a.nq : N) + 15) >> 4;          // a.nq: only the first query rows are wanted (whole 16-row blocks)
  v4i fq_next = {0, 0, 0, 0};
  if (wave < nqb) {
    const int qr0 = wave * 16 + l15;
    fq_next = *reinterpret_cast<const v4i*>(base + (long long)(qr0 < N ? qr0 : N - 1) * ld + g * 16);
  }
  __syncthreads();

  const int ksw = ((l15 >> 3) & 1) << 1;                                  // swizzle term of this lane's fragment rows (row = 16 x + l15)
  const int8_t* kfrag = sK + l15 * HD + ((g ^ ksw) << 4);                 // + 1024 per 16-key block
  for (int qb = wave; qb < nqb; qb += nwaves) {
    const int qrow = qb * 16 + l15;
    const v4i fq = fq_next;
    if (qb + nwaves < nqb) {
      const int qn = (qb + nwaves) * 16 + l15;
      fq_next = *reinterpret_cast<const v4i*>(base + (long long)(qn < N ? qn : N - 1) * ld + g * 16);
    }

    // ---- scores -> bytes nc + 127, group by group; the MFMAs of the next group are issued ahead of the requantisation of this one
    unsigned codes[NG][4];
    float mnf = 255.f;
    v4i sc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      sc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(kfrag + j * 1024), fq, (v4i){0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
      v4i sn[4];
      if (grp + 1 < NG) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          sn[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(*reinterpret_cast<const v4i*>(kfrag + ((grp + 1) * 4 + j) * 1024), fq,
                                                        (v4i){0, 0, 0, 0}, 0, 0, 0);
      }
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
      if (grp + 1 < NG) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j] = sn[j];
      }
      __builtin_amdgcn_sched_barrier(0);                                  // one group of MFMAs ahead, not all of them: their results are 16 registers each
    }
    int mn = (int)mnf;                                                    // min of nc + 127 = 127 - (row max of the codes)
    {
      int o = __shfl_xor(mn, 16);
      mn = o < mn ? o : mn;
      o = __shfl_xor(mn, 32);
      mn = o < mn ? o : mn;
    }
    // d = max - code = byte - mn in [0, 255]; 8 d + c0 is the absolute LDS address of the exp_int entry (padding: entry 256)
    const int c0 = ebase - 8 * mn;
#define P2V_PK_D8(cw, grp, j, r, d8)                                                                   \
  int d8 = (int)((((cw) >> (8 * (r))) & 255u) << 3) + c0;                                              \
  if ((grp) == NG - 1) d8 = (grp) * 64 + 16 * (j) + 4 * g + (r) < N ? d8 : ebase + 2048;
    long long S = 0;
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          P2V_PK_D8(codes[grp][j], grp, j, r, d8)
          S += *(lds_i64p)(uintptr_t)(unsigned)d8;
        }
      __builtin_amdgcn_sched_barrier(0);                                  // keep live ranges short
    }
    S += __shfl_xor(S, 16);
    S += __shfl_xor(S, 32);
    const double Sd = (double)(float)S;                                   // exp_int.sum(-1): exact, then one rounding

    // ---- probabilities as the two int8 planes and P.V
    v4i oA[NDT], oB[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) oA[dt] = oB[dt] = (v4i){0, 0, 0, 0};
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
      v4i pa, pb = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned h[4];
        // the table offsets are formed again from the packed bytes: left to itself the compiler keeps the 16 offsets per group of the sum
        // phase alive for this one, which is the register array (a) is there to avoid
        unsigned cw = codes[grp][j];
        asm volatile("" : "+v"(cw));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          P2V_PK_D8(cw, grp, j, r, d8)
          // round(sum / exp_int), layers.py:370: the correctly rounded fp32 quotient from one fp64 multiply (proof: k_lis_attention)
          const double rd = ((lds_f64p)(uintptr_t)(unsigned)d8)[258];
          const float ratio = rintf((float)(Sd * rd));
          const unsigned E = (__float_as_uint(ratio) + 0x00400000u) >> 23;        // log_round, layers.py:323-329: 127 + k, k >= 0 (ratio >= 1)
          if constexpr (KLIM == 16) h[r] = 0x8000u >> ((E < 143u ? E : 143u) - 127u);      // p 2^15; 0 from k = 16 on (layers.py:372-375)
          else h[r] = (0x80u >> ((E < 143u ? E : 143u) - 127u)) << 8;                        // uint3: 0 from k = 8 on
        }
        const v2u16 n01 = (v2u16){0, 0} - __builtin_bit_cast(v2u16, h[0] | (h[1] << 16));      // -h, 16-bit
        const v2u16 n23 = (v2u16){0, 0} - __builtin_bit_cast(v2u16, h[2] | (h[3] << 16));
        const v2u16 a01 = n01 + (v2u16){0x80, 0x80}, a23 = n23 + (v2u16){0x80, 0x80};
        pa[j] = (int)__builtin_amdgcn_perm(__builtin_bit_cast(unsigned, a23), __builtin_bit_cast(unsigned, a01), 0x07050301u);   // the high bytes
        if constexpr (KLIM == 16) pb[j] = (int)__builtin_amdgcn_perm(__builtin_bit_cast(unsigned, n23), __builtin_bit_cast(unsigned, n01), 0x06040200u);   // the low bytes
      }
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const v4i va = *reinterpret_cast<const v4i*>(sVt + grp * 4096 + (dt * 16 + l15) * 64 + ((g ^ ksw ^ dt) << 4));
        oA[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, pa, oA[dt], 0, 0, 0);
        if constexpr (KLIM == 16) oB[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, pb, oB[dt], 0, 0, 0);      // (KLIM = 8: plane B is zero)
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#undef P2V_PK_D8
    // qact2: (attn @ v) / s  with attn@v = O * s_q1   (vit_fquant.py:325-326); lane owns channels 16 dt + 4 g .. + 3.  Unconditional stores:
    // a padding query row (qrow >= N) was computed from the Q fragment of row N - 1, so its values ARE row N - 1's (see k_lis_attention)
    {
      const int qs = qrow < N ? qrow : N - 1;
      int8_t* dst = a.out + ((long long)b * N + qs) * D + head * HD + 4 * g;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (float)(-(256 * oA[dt][r] + oB[dt][r])) * avm;      // |.| < 2^24: exact
        *reinterpret_cast<unsigned*>(dst + dt * 16) = pack4_rne_sat(o[0], o[1], o[2], o[3]);
      }
    }
  }
}

template <int NG, int KLIM>
static int launch_packed_t(const AttnArgs& a, hipStream_t st) {
  constexpr size_t smem = (size_t)NG * 64 * 128 + 2 * 258 * 8;
  static_assert(smem <= 160 * 1024, "LDS of a CU");
  static P2vLdsGrant grant = {};                   // always beyond the default dynamic LDS limit
  const hipError_t e = grant.ensure(reinterpret_cast<const void*>(&k_lis_attention_packed<NG, KLIM>), (int)smem);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((k_lis_attention_packed<NG, KLIM>), dim3((unsigned)(a.B * a.H)), dim3(64 * g_attn_waves), smem, st, a);
  CHECK_LAUNCH();
  return 0;
}

// the launchers, in the order the code object holds their kernels (p2vit_launch.h): flat index ceil(tokens / 64) * 2 + (uint3); groups
// 10 .. 19 are instantiated
typedef int (*PackedLauncher)(const AttnArgs&, hipStream_t);
constexpr int packed_index(int ng, int klim) { return ng * 2 + (klim == 8 ? 1 : 0); }
struct PackedAt {
  template <int I> static constexpr PackedLauncher at() {
    constexpr int NG = I >> 1, KLIM = (I & 1) ? 8 : 16;
    static_assert(packed_index(NG, KLIM) == I, "decoded as the launcher encodes");
    if constexpr (NG >= 10) return launch_packed_t<NG, KLIM>;
    else return nullptr;
  }
};
static const auto packed_table = p2v_table<PackedLauncher, PackedAt, 40>();

// head_dim 64, no tap, tokens beyond the resident kernel's up to P2V_MAX_TOKENS_PACKED: one instantiation per ceil(tokens / 64)
int p2v_launch_attention_packed(const AttnArgs& a_, hipStream_t st) {
  AttnArgs a = a_;
  if (a.probs_k || a.B * a.H <= 0 || a.N > P2V_MAX_TOKENS_PACKED) return -1;
  if ((a.klim = p2v_attn_klim(a.klim)) < 0) return -1;
  const int ng = (a.N + 63) / 64, idx = packed_index(ng, a.klim);
  const PackedLauncher launch = (ng >= 0 && idx < (int)packed_table.size()) ? packed_table[idx] : nullptr;
  return launch ? launch(a, st) : -1;
}
