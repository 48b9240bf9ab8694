// p2vit_winattn_softmax.hip -- Swin window attention with the FLOAT softmax of Config(lis=False) (QIntSoftmax with log_i_softmax = False: the
// plain softmax of the dequantised qact2 codes plus the -100 mask, layers.py:387-395), restated on integers, for head_dim 32 and windows of
// 1 x 1 ... 12 x 12 tokens.
//
// Up to the qact2 codes the arithmetic is k_window_attention's / k_window_attention_wide's, code for code: q*scale rounded once per element
// (eta plane, two int8 dot products combined exactly in fp64), one rounding to fp32, qact_attn1, the relative-position bias pre-scaled by
// s_table / s_q2, the qact2 clamp; region ids and the linear bias index from sMeta; win_index for the loads and for the scatter of the output;
// one wave per (image, window, head), four heads per workgroup.  Behind the codes c_ij it is the table softmax of k_softmax_attention with
// the softmax scale s_q2:
//     U_i   = keys of the query's region (every key of the window without a mask); the row's own token is always in it
//     m_i   = max over U_i of c_ij;   E_ij = tab[m_i - c_ij] for j in U_i, 0 for masked keys and padding        tab: 256 entries below 2^21
//     num_ic = sum_j E_ij v_jc,  den_i = sum_j E_ij                                                             exact integers, den >= tab[0] > 0
//     code_ic = clamp(rne((double(num_ic) / double(den_i)) av_mul), -128, 127)                                  one IEEE fp64 division
// A masked key is exactly zero and outside the maximum: for s_q2 <= 2^-2 (the entry point refuses larger scales) the reference's -100 shifts
// its code by >= 400 > 255 below every key of U_i and exp(-36.25) 2^21 rounds to 0.
// P.V on the matrix unit, as in k_softmax_attention: E = e0 + 128 e1 + 16384 e2, three non-negative int8 digit planes as B operands of
// v_mfma_i32_16x16x64_i8 against V^T staged as int8; per-plane partial sums <= 144 * 127 * 128 < 2^22; recombined in int64 (|num| < 2^37).
// The score accumulator layout is the B operand's: lane (query l15, g) holds keys 64 grp + 16 j + 4 g + r, which is k index 16 g + 4 j + r of
// group grp, and V^T is staged in that order.
// NG = ceil(ws^2 / 64) is the template parameter: every score slot (grp, j, r) is compile-time indexed, the qact2 codes of a query block
// stay in registers as bytes c + 128 four to a register (12 registers at 144 keys) beside one membership bit per slot; 16-key blocks behind
// the window are skipped wave-uniformly.  Static LDS, no private segment (DESIGN 8h has the figures per instantiation).
#include "p2vit_device.h"
#include "p2vit_launch.h"

#define WSM_HD 32
#define WSM_VROW 80     // bytes of a V^T channel row of one 64-key group: 64 keys + 16 (row stride 20 dwords; stays 16-byte aligned)

template <int NG>
struct WinSm {
  static constexpr int KR = NG == 3 ? 144 : NG * 64;        // K rows / token records staged: ws <= 8, <= 11, 12
  static constexpr int NKB = KR / 16;                       // 16-key blocks that can hold a key
  static constexpr int MAXWS = NG == 1 ? 8 : (NG == 2 ? 11 : 12);
  static constexpr int TS = ((2 * MAXWS - 1) * (2 * MAXWS - 1) + 3) & ~3;      // floats per bias column
  static constexpr int NTI = (TS + 63) / 64;                // bias entries per lane
};

template <int NG>
__global__ __launch_bounds__(256, 2) void k_window_softmax_attention(WinSmArgs a) {
  typedef WinSm<NG> G;
  constexpr int KR = G::KR, NKB = G::NKB;
  static_assert(NG >= 1 && NG <= 3, "64-key groups");
  __shared__ __attribute__((aligned(16))) int8_t sK[4][KR * WSM_HD];                          // [KR][32]
  __shared__ __attribute__((aligned(16))) unsigned char sVt[4][NG * WSM_HD * WSM_VROW];       // [NG][32 channels][64 keys in operand order]
  __shared__ float sT[4][G::TS];                                                              // bias column of the head, times s_table / s_q2
  __shared__ unsigned sTab[257];                                                              // entry 256 = 0: masked keys and padding
  __shared__ int sRow[KR];                                                                    // row (within the image) of token t of this window
  __shared__ __attribute__((aligned(8))) unsigned short sMeta[KR];                            // per token: lin (y*(2ws-1)+x) | region << 10
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int ws = a.wa.ws, N = ws * ws, nW = a.wa.n_windows;
  const int hgroups = (a.H + 3) >> 2;
  const int blk = blockIdx.x;
  const int hg = blk % hgroups, w = (blk / hgroups) % nW, b = blk / (hgroups * nW);
  const int head = hg * 4 + wave;
  const int C = a.H * WSM_HD;
  const long long ldq = a.wa.qkv_stride ? a.wa.qkv_stride : 3 * C, ldo = a.wa.out_stride ? a.wa.out_stride : C;
  const bool hok = head < a.H;
  // loads first, as in k_window_attention: row table, bias column and region ids, then the softmax table, then K / V and the first Q block
  int rowj[NG];
#pragma unroll
  for (int p = 0; p < NG; ++p) {
    const int t = p * 64 + lane;
    rowj[p] = a.wa.win_index[w * N + (t < N ? t : 0)];
  }
  const int tsz = (2 * ws - 1) * (2 * ws - 1);
  int8_t tcode[G::NTI];
#pragma unroll
  for (int i = 0; i < G::NTI; ++i) {
    tcode[i] = 0;
    if (hok && lane + 64 * i < tsz) tcode[i] = a.wa.table_codes[(lane + 64 * i) * a.H + head];
  }
  int reg_t = 0;
  if (a.wa.region && tid < N) reg_t = (int)a.wa.region[w * N + tid];
  sTab[tid] = a.tab[tid];
  if (tid == 0) sTab[256] = 0u;
  if (tid < KR) {
    const int t = tid < N ? tid : 0;
    sMeta[tid] = (unsigned short)(((t / ws) * (2 * ws - 1) + (t % ws)) | (reg_t << 10));
    sRow[tid] = a.wa.win_index[w * N + t];
  }
  const int8_t* hbase = a.qkv + (long long)b * a.T * ldq + head * WSM_HD;
  uint4 kq[NG][2], vq[NG][2];
#pragma unroll
  for (int p = 0; p < NG; ++p) {
    kq[p][0] = kq[p][1] = vq[p][0] = vq[p][1] = make_uint4(0, 0, 0, 0);
    if (hok && p * 64 + lane < N) {
      const int8_t* base = hbase + (long long)rowj[p] * ldq;
      kq[p][0] = *reinterpret_cast<const uint4*>(base + C);
      kq[p][1] = *reinterpret_cast<const uint4*>(base + C + 16);
      vq[p][0] = *reinterpret_cast<const uint4*>(base + 2 * C);
      vq[p][1] = *reinterpret_cast<const uint4*>(base + 2 * C + 16);
    }
  }
  int rowq_next = __shfl(rowj[0], l15 < N ? l15 : N - 1);
  v4i qc_next = {0, 0, 0, 0};
  if (hok) qc_next = *reinterpret_cast<const v4i*>(hbase + (long long)rowq_next * ldq + (g & 1) * 16);
  const float inv_sa = 1.0f / a.wa.s_attn, inv_s2 = 1.0f / a.wa.s_q2;          // powers of two: exact
  // qact2((a1 * s_attn + code * s_table)) = clamp(rint(fma(a1, s_attn / s_q2, code * s_table / s_q2))): the bias column is staged already scaled
  const float tb_mul = a.wa.s_table * inv_s2, a1_mul = a.wa.s_attn * inv_s2;
#pragma unroll
  for (int i = 0; i < G::NTI; ++i)
    if (lane + 64 * i < tsz) sT[wave][lane + 64 * i] = (float)tcode[i] * tb_mul;
  {
    // key kk = 16 j + 4 gg + r of a group is k index 16 gg + 4 j + r of the P.V contraction
    const int slot = ((lane >> 2) & 3) * 16 + (lane >> 4) * 4 + (lane & 3);
#pragma unroll
    for (int p = 0; p < NG; ++p) {
      const int t = p * 64 + lane;
      if (t < KR) {
        *reinterpret_cast<uint4*>(&sK[wave][t * WSM_HD]) = kq[p][0];
        *reinterpret_cast<uint4*>(&sK[wave][t * WSM_HD + 16]) = kq[p][1];
      }
      const unsigned vw[8] = {vq[p][0].x, vq[p][0].y, vq[p][0].z, vq[p][0].w, vq[p][1].x, vq[p][1].y, vq[p][1].z, vq[p][1].w};
#pragma unroll
      for (int c = 0; c < WSM_HD; ++c) sVt[wave][(p * WSM_HD + c) * WSM_VROW + slot] = (unsigned char)(vw[c >> 2] >> (8 * (c & 3)));
    }
  }
  __syncthreads();
  if (!hok) return;
  const float sigma = a.wa.s_q1 * a.wa.qk_scale;                               // exact (s_q1 = 2^e)
  const float inv_u = __uint_as_float((unsigned)(254 - (int)(__float_as_uint(sigma) >> 23) + 23) << 23);   // 1 / ulp(sigma)
  // score = u * X,  X = (sigma / u) * S1 + S2 an integer below 2^53: RN32(u * X) = u * RN32(X)
  const float sig_m = sigma * inv_u;                                           // the 24-bit significand of sigma as an integer
  const double sig_int = (double)sig_m;
  const float x_mul = ((1.0f / inv_u) * a.wa.s_q1) * inv_sa;                   // u / s_attn: a power of two
  const double avm = (double)(a.wa.s_q1 / a.wa.s_q3);                          // a power of two (checked by the entry point)
  const int c0 = (ws - 1) * (2 * ws - 1) + (ws - 1);
  const int nqb = (N + 15) >> 4;
  const bool masked = a.wa.region != nullptr;
#pragma unroll 1
  for (int qb = 0; qb < nqb; ++qb) {
    const int qi = qb * 16 + l15;
    const int qr = qi < N ? qi : N - 1;
    const int rowq = rowq_next;
    const v4i qc = qc_next;
    if (qb + 1 < nqb) {                                                        // the next block's Q fragment, a block ahead
      const int qn = qi + 16 < N ? qi + 16 : N - 1;
      rowq_next = sRow[qn];
      qc_next = *reinterpret_cast<const v4i*>(hbase + (long long)rowq_next * ldq + (g & 1) * 16);
    }
    // eta plane (see k_window_attention): in units of u, eta = RN32(code * m) - code * m with m = sigma / u
    unsigned eh[2];
    {
      const unsigned qh[2] = {(unsigned)(g < 2 ? qc[0] : qc[2]), (unsigned)(g < 2 ? qc[1] : qc[3])};
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        float et[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float cf = (float)sx8(qh[d], e);
          const float v = cf * sig_m;                                           // RN32(code * m)
          et[e] = __builtin_fmaf(-cf, sig_m, v);                                // exact, an integer in [-64, 64]
        }
        eh[d] = pack4_pre(et[0], et[1], et[2], et[3]);
      }
    }
    const auto up0 = __builtin_amdgcn_permlane32_swap(0u, eh[0], false, false);   // [0]: upper half := eh of the lower half
    const auto up1 = __builtin_amdgcn_permlane32_swap(0u, eh[1], false, false);
    const v4i qeta = {(int)up0[0], (int)up1[0], (int)eh[0], (int)eh[1]};
    const v4i fq1 = g < 2 ? qc : (v4i){0, 0, 0, 0};
    const v4i fq2 = g < 2 ? (v4i){0, 0, 0, 0} : qeta;
    const unsigned mi = sMeta[qr];
    const float* trow = &sT[wave][(int)(mi & 1023u) + c0];                     // bias entry of key j: trow[-lin_j]
    const unsigned reg_i = mi >> 10;

    // ---- qact2 codes as bytes c + 128, membership in U_i one bit per slot, row maximum over U_i
    unsigned codes[NG][4], inu[NG];
    int mxb = 0;
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
      inu[grp] = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kb = grp * 4 + j;
        codes[grp][j] = 0u;
        if (kb >= NKB || kb * 16 >= N) continue;                               // wave-uniform: a block of padding
        const v4i fk = *reinterpret_cast<const v4i*>(&sK[wave][(kb * 16 + l15) * WSM_HD + (g & 1) * 16]);
        const v4i s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk, fq1, (v4i){0, 0, 0, 0}, 0, 0, 0);
        const v4i s2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk, fq2, (v4i){0, 0, 0, 0}, 0, 0, 0);
        const uint2 m4 = *reinterpret_cast<const uint2*>(&sMeta[kb * 16 + 4 * g]);
        unsigned wd = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned mj = ((r < 2 ? m4.x : m4.y) >> ((r & 1) * 16)) & 0xFFFFu;
          const double X = __builtin_fma(sig_int, (double)s1[r], (double)s2[r]);                   // exact
          const float a1 = __builtin_amdgcn_fmed3f(rintf((float)X * x_mul), -128.f, 127.f);       // ONE rounding, then qact_attn1
          const float a2 = __builtin_amdgcn_fmed3f(rintf(__builtin_fmaf(a1, a1_mul, trow[-(int)(mj & 1023u)])), -128.f, 127.f);   // qact2
          const int byte = (int)a2 + 128;
          const bool in = kb * 16 + 4 * g + r < N && (!masked || (mj >> 10) == reg_i);
          wd |= (unsigned)byte << (8 * r);
          inu[grp] |= in ? 1u << (4 * j + r) : 0u;
          mxb = in && byte > mxb ? byte : mxb;
        }
        codes[grp][j] = wd;
      }
      __builtin_amdgcn_sched_barrier(0);                                       // keep live ranges short
    }
    {
      int o = __shfl_xor(mxb, 16);
      mxb = o > mxb ? o : mxb;
      o = __shfl_xor(mxb, 32);
      mxb = o > mxb ? o : mxb;
    }

    // ---- E = tab[m - c] as three 7-bit digit planes, P.V on the int8 MFMA
    v4i o0[2], o1[2], o2[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) o0[dt] = o1[dt] = o2[dt] = (v4i){0, 0, 0, 0};
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
          const int d = mxb - (int)((cw >> (8 * r)) & 255u);                   // in [0, 255] for the keys of U_i
          const unsigned E = sTab[(inu[grp] >> (4 * j + r)) & 1u ? d : 256];
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
      for (int dt = 0; dt < 2; ++dt) {
        const v4i va = *reinterpret_cast<const v4i*>(&sVt[wave][(grp * WSM_HD + dt * 16 + l15) * WSM_VROW + g * 16]);
        o0[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, p0, o0[dt], 0, 0, 0);
        o1[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, p1, o1[dt], 0, 0, 0);
        o2[dt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, p2, o2[dt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    const double dend = (double)den;

    // qact3; lane owns channels 16 dt + 4 g .. + 3 of query l15
    if (qi < N) {
      int8_t* dst = a.out + ((long long)b * a.T + rowq) * ldo + head * WSM_HD + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        unsigned wd = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long num = (long long)o0[dt][r] + 128LL * (long long)o1[dt][r] + 16384LL * (long long)o2[dt][r];
          double c = rint(((double)num / dend) * avm);
          c = c < -128.0 ? -128.0 : (c > 127.0 ? 127.0 : c);
          wd |= ((unsigned)(int)c & 255u) << (8 * r);
        }
        *reinterpret_cast<unsigned*>(dst + dt * 16) = wd;
      }
    }
  }
}

template <int NG>
static int launch_winsm_t(const WinSmArgs& a, hipStream_t st) {
  const int hgroups = (a.H + 3) / 4;
  hipLaunchKernelGGL((k_window_softmax_attention<NG>), dim3((unsigned)(a.B * a.wa.n_windows * hgroups)), dim3(256), 0, st, a);
  CHECK_LAUNCH();
  return 0;
}

// the launchers by ceil(ws^2 / 64) = 1 .. 3: index = groups - 1
typedef int (*WinSmLauncher)(const WinSmArgs&, hipStream_t);
constexpr int winsm_index(int ng) { return ng - 1; }
struct WinSmAt {
  template <int I> static constexpr WinSmLauncher at() {
    static_assert(winsm_index(I + 1) == I, "index function");
    return launch_winsm_t<I + 1>;
  }
};
static const auto winsm_table = p2v_table<WinSmLauncher, WinSmAt, 3>();

int p2v_launch_window_softmax_attention(const WinSmArgs& a, hipStream_t st) {
  if (a.wa.ws < 1 || a.wa.ws > 12 || a.B * a.wa.n_windows * a.H <= 0) return -1;
  return winsm_table[winsm_index((a.wa.ws * a.wa.ws + 63) / 64)](a, st);
}
