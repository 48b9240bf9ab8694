// p2vit_winattn_wide.hip -- Swin window attention for windows of 9 x 9 ... 12 x 12 tokens (65 ... 144 keys), head_dim 32: the
// patch 4 / window 12 / 384^2 geometry of Swin-B and Swin-L, whose feature maps are 96, 48, 24 and 12 tokens wide.
//
// The arithmetic is k_window_attention's (p2vit_attn.hip), code for code: q*scale rounded once per element (eta plane, two int8 dot
// products combined exactly in fp64), one rounding to fp32, qact_attn1, the relative-position bias pre-scaled by s_table / s_q2,
// qact2, the -100 mask between region ids, the exp table with its clamp (256) and padding (257) entries, the exact int64 row sum,
// the quotient by one fp64 multiply, lis_prob_pair, an exact P.V product and pack4_rne_sat.  What differs is the bookkeeping of a
// window that no longer fits one lane per token:
//   - WS is a template parameter, so N = WS^2, the NKB = ceil(N / 16) key blocks and every score slot (kb, r) have compile-time
//     indices and stay in registers (36 slots per lane at 144 keys); a slot that is padding in every lane costs nothing and the
//     padding test is compiled only into the slots of the last key block;
//   - K, V^T, the row table and the token metadata are staged in passes of 64 tokens;
//   - V^T has a row stride of whole 32-key pairs (+4), zero-filled behind the window: the P.V product walks ceil(N / 32) pairs and
//     the half-empty last pair meets zero probabilities and zero values;
//   - the bias column holds (2 WS - 1)^2 <= 529 entries, and lin = y (2 WS - 1) + x <= 264 still fits the 10 bits of sMeta.
// Exactness of P.V in fp32 does not depend on the key count: the probabilities are 2^-k, k <= 15, with sum <= 2.25 (1 + 2^-22) over ANY
// number of keys (log_round and the rounded quotient each lose at most a factor 1.5), and |v| <= 128, so every partial sum is a
// multiple of 2^-15 below 2.25 * 2^7 * 2^15 < 2^24 such units - the bound the 64-key kernel relies on.
// LDS per workgroup at WS = 12: 4 x (4.5 KB K + 10.25 KB V^T + 2.1 KB bias) + 4 KB tables + 0.8 KB token tables = 73 920 B, two
// workgroups per CU (47 KB at WS = 9: three); 136 ... 182 VGPRs and no private segment in any instantiation (DESIGN 7 has the table).
#include "p2vit_attn_lis.h"

#define WW_HD 32
// slot (kb, r) of lane group g holds key kb*16 + 4g + r
#define WW_DEAD(kb, r) ((kb) * 16 + (r) >= N)           // padding in every lane: no arithmetic
#define WW_PAD(kb, r) ((kb) * 16 + 12 + (r) >= N)       // padding in some lane: the test is compiled in
#define WW_KEEP(x) asm volatile("" ::"v"(x))            // the value stays in its registers up to here

template <int WS>
struct WinWide {
  static constexpr int N = WS * WS;
  static constexpr int NKB = (N + 15) / 16;               // 16-key blocks: 6, 7, 8, 9
  static constexpr int NP = (NKB + 1) / 2;                // 32-key pairs of the P.V product
  static constexpr int KR = NKB * 16;                     // K rows staged (rows >= N are zero)
  static constexpr int VR = NP * 32;                      // V^T columns staged (columns >= N are zero)
  static constexpr int VSTRIDE = VR + 4;                  // bf16 elements; dword stride = 2*odd -> conflict-free b64 reads
  static constexpr int TSZ = (2 * WS - 1) * (2 * WS - 1);
  static constexpr int TS = (TSZ + 3) & ~3;               // floats per bias column
  static constexpr int NPASS = (VR + 63) / 64;            // staging passes of 64 tokens
  static constexpr int NTI = (TSZ + 63) / 64;             // bias entries per lane
  static constexpr size_t OFF_VT = (size_t)4 * KR * WW_HD;
  static constexpr size_t OFF_T = OFF_VT + (size_t)4 * WW_HD * VSTRIDE * 2;
  static constexpr size_t OFF_LUTE = OFF_T + (size_t)4 * TS * 4;
  static constexpr size_t OFF_LUTFR = OFF_LUTE + 258 * 8;
  static constexpr size_t OFF_ROW = OFF_LUTFR + 258 * 8;
  static constexpr size_t OFF_META = OFF_ROW + (size_t)KR * 4;
  static constexpr size_t SMEM = OFF_META + (size_t)KR * 2;
};

template <int WS, bool TAP>
__global__ __launch_bounds__(256, 2) void k_window_attention_wide(std::conditional_t<TAP, WinAttnArgs, WinAttnKArgs> a) {
  typedef WinWide<WS> G;
  constexpr int N = G::N, NKB = G::NKB, NP = G::NP, KR = G::KR, VR = G::VR, VSTRIDE = G::VSTRIDE, TSZ = G::TSZ;
  static_assert(WS >= 9 && WS <= 12, "window size");
  static_assert((WS - 1) * (2 * WS - 1) + (WS - 1) < 1024, "lin must fit the 10 bits of sMeta");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  int8_t* sK = reinterpret_cast<int8_t*>(smem) + wave * (KR * WW_HD);                                   // [KR][32]
  unsigned short* sVt = reinterpret_cast<unsigned short*>(smem + G::OFF_VT) + wave * (WW_HD * VSTRIDE);  // [32][VSTRIDE] bf16
  float* sT = reinterpret_cast<float*>(smem + G::OFF_T) + wave * G::TS;                                 // bias column of the head, times s_table / s_q2
  long long* lutE = reinterpret_cast<long long*>(smem + G::OFF_LUTE);
  double* lutFR = reinterpret_cast<double*>(smem + G::OFF_LUTFR);                                       // fp64 reciprocal of float(exp_int)
  int* sRow = reinterpret_cast<int*>(smem + G::OFF_ROW);                                                // row (within the image) of token t of this window
  unsigned short* sMeta = reinterpret_cast<unsigned short*>(smem + G::OFF_META);                        // per token: lin (y*(2ws-1)+x) | region << 10
  const int nW = a.wa.n_windows;
  const int hgroups = (a.H + 3) >> 2;
  const int blk = blockIdx.x;
  const int hg = blk % hgroups, w = (blk / hgroups) % nW, b = blk / (hgroups * nW);
  const int head = hg * 4 + wave;
  const int C = a.H * WW_HD;
  const long long ldq = a.wa.qkv_stride ? a.wa.qkv_stride : 3 * C, ldo = a.wa.out_stride ? a.wa.out_stride : C;
  const bool hok = head < a.H;
  // loads first, as in k_window_attention: row table, bias column and region ids, then the exp table, then K / V and the first Q block
  int rowj[G::NPASS];
#pragma unroll
  for (int p = 0; p < G::NPASS; ++p) {
    const int t = p * 64 + lane;
    rowj[p] = a.wa.win_index[w * N + (t < N ? t : 0)];
  }
  int8_t tcode[G::NTI];
#pragma unroll
  for (int i = 0; i < G::NTI; ++i) {
    tcode[i] = 0;
    if (hok && lane + 64 * i < TSZ) tcode[i] = a.wa.table_codes[(lane + 64 * i) * a.H + head];
  }
  int reg_t = 0;
  if (a.wa.region && tid < N) reg_t = (int)a.wa.region[w * N + tid];
  // exp table of the log-int-softmax; entry 256 = clamp value (masked pairs), 257 = padding
  for (int t = tid; t < 258; t += (int)blockDim.x) {
    int xi = -t;
    const int lim = 32 * a.wa.x0_int;
    xi = (xi < lim || t >= 256) ? lim : xi;
    const int q = xi / a.wa.x0_int;
    const int r = xi - a.wa.x0_int * q;
    const long long z = (long long)r * (r + a.wa.b_int) + a.wa.c_int;
    long long e = z << (32 - q);
    e = e < 0 ? 0 : e;
    if (t == 257) e = 0;
    const float ef = t == 257 ? 1.0f : (float)e;
    lutE[t] = e;
    lutFR[t] = 1.0 / (double)ef;
  }
  if (tid < KR) {
    const int t = tid < N ? tid : 0;
    sMeta[tid] = (unsigned short)(((t / WS) * (2 * WS - 1) + (t % WS)) | (reg_t << 10));
    sRow[tid] = a.wa.win_index[w * N + t];
  }
  const int8_t* hbase = a.qkv + (long long)b * a.T * ldq + head * WW_HD;
  uint4 kq[G::NPASS][2], vq[G::NPASS][2];
#pragma unroll
  for (int p = 0; p < G::NPASS; ++p) {
    kq[p][0] = kq[p][1] = vq[p][0] = vq[p][1] = make_uint4(0, 0, 0, 0);
    if (hok && p * 64 + lane < N) {
      const int8_t* base = hbase + (long long)rowj[p] * ldq;
      kq[p][0] = *reinterpret_cast<const uint4*>(base + C);
      kq[p][1] = *reinterpret_cast<const uint4*>(base + C + 16);
      vq[p][0] = *reinterpret_cast<const uint4*>(base + 2 * C);
      vq[p][1] = *reinterpret_cast<const uint4*>(base + 2 * C + 16);
    }
  }
  int rowq_next = __shfl(rowj[0], l15);                                        // N > 16: the first query block is full
  v4i qc_next = {0, 0, 0, 0};
  if (hok) qc_next = *reinterpret_cast<const v4i*>(hbase + (long long)rowq_next * ldq + (g & 1) * 16);
  const float inv_sa = 1.0f / a.wa.s_attn, inv_s2 = 1.0f / a.wa.s_q2;          // powers of two: exact
  // qact2((a1 * s_attn + code * s_table)) = clamp(rint(fma(a1, s_attn / s_q2, code * s_table / s_q2))): the bias column is staged already scaled
  const float tb_mul = a.wa.s_table * inv_s2, a1_mul = a.wa.s_attn * inv_s2;
#pragma unroll
  for (int i = 0; i < G::NTI; ++i)
    if (lane + 64 * i < TSZ) sT[lane + 64 * i] = (float)tcode[i] * tb_mul;
#pragma unroll
  for (int p = 0; p < G::NPASS; ++p) {
    const int t = p * 64 + lane;
    if (t < KR) {
      *reinterpret_cast<uint4*>(&sK[t * WW_HD]) = kq[p][0];
      *reinterpret_cast<uint4*>(&sK[t * WW_HD + 16]) = kq[p][1];
    }
    if (t < VR) {
      const unsigned vw[8] = {vq[p][0].x, vq[p][0].y, vq[p][0].z, vq[p][0].w, vq[p][1].x, vq[p][1].y, vq[p][1].z, vq[p][1].w};
#pragma unroll
      for (int c = 0; c < WW_HD; ++c) {
        const float f = (float)sx8(vw[c >> 2], c & 3);
        sVt[c * VSTRIDE + t] = (unsigned short)(__float_as_uint(f) >> 16);    // exact bf16
      }
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
  const float m100 = (float)(int)(100.0f * inv_s2);                            // 100 / sf as an integer
  const int klim = a.klim;                                                        // 2^softmax_bits: probability 0 from k = klim on
  const unsigned kc = lis_prob_const(klim);
  const float av_mul = (a.wa.s_q1 / a.wa.s_q3) * lis_prob_scale(klim);            // the probabilities are scaled by 2^-(127 - klim) (lis_prob_pair)
  constexpr int c0 = (WS - 1) * (2 * WS - 1) + (WS - 1);
  // per score slot of this lane: relative-position term and region of its key (the same for every query block), as staged: two
  // slots to a register (keys 4g + r and 4g + r + 1 are neighbours in sMeta)
  unsigned mj2[NKB][2];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      mj2[kb][h] = WW_DEAD(kb, 2 * h) ? 0u : *reinterpret_cast<const unsigned*>(&sMeta[kb * 16 + 4 * g + 2 * h]);
#define WW_META(kb, r) ((mj2[kb][(r) >> 1] >> (((r) & 1) * 16)) & 0xFFFFu)
#pragma unroll 1
  for (int qb = 0; qb < NKB; ++qb) {
    // the packed metadata is all that stays in registers across query blocks: what is derived from it (36 table offsets, 36 region ids)
    // is loop-invariant, and hoisted out of the loop it would not fit beside the score slots
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      asm volatile("" : "+v"(mj2[kb][0]));
      asm volatile("" : "+v"(mj2[kb][1]));
    }
    const int qi = qb * 16 + l15;
    const int qr = qi < N ? qi : N - 1;
    const int rowq = rowq_next;
    const v4i qc = qc_next;
    if (qb + 1 < NKB) {                                                        // the next block's Q fragment, a block ahead
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
    // MFMA operands and loads: a load that lands in an operand register of an MFMA issued just before it can change that MFMA's result
    // (seen on the MI355X with v_mfma_f32_16x16x32_bf16 and an LDS load into its A registers directly behind it: the data arrived before
    // the operand was read, and hipcc places no wait there).  So all K fragments are in registers before the first score MFMA, and
    // WW_KEEP holds operand registers past the loads that follow, so that the register allocator cannot hand them out again too early
    v4i s1[NKB], s2[NKB], fk[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) fk[kb] = *reinterpret_cast<const v4i*>(&sK[(kb * 16 + l15) * WW_HD + (g & 1) * 16]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      s1[kb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk[kb], fq1, (v4i){0, 0, 0, 0}, 0, 0, 0);
      s2[kb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk[kb], fq2, (v4i){0, 0, 0, 0}, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    const unsigned mi = sMeta[qr];
    const float* trow = &sT[(int)(mi & 1023u) + c0];                           // bias entry of key j: trow[-lin_j]
    const unsigned reg_i = mi >> 10;
    // qact_attn1 codes first, key block by key block: the fp64 operands of a slot die with it (left to the compiler, the conversions of all
    // 36 slots are hoisted above the mask / no-mask branch and their 144 registers spill)
    float xs[NKB][4];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (WW_DEAD(kb, r)) continue;
        const double X = __builtin_fma(sig_int, (double)s1[kb][r], (double)s2[kb][r]);         // exact
        xs[kb][r] = __builtin_amdgcn_fmed3f(rintf((float)X * x_mul), -128.f, 127.f);           // ONE rounding, then qact_attn1
      }
      if (kb == 0) {                                                           // the score MFMAs have read their operands by now
#pragma unroll
        for (int k2 = 0; k2 < NKB; ++k2) WW_KEEP(fk[k2]);
        WW_KEEP(fq1);
        WW_KEEP(fq2);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    float mx = -3.0e9f;
    auto scores = [&](auto MASKc) {
      constexpr bool MASK = decltype(MASKc)::value;                            // shifted windows: pairs from different regions get -100
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (WW_DEAD(kb, r)) continue;
          const float a1 = xs[kb][r];
          const float a2 = __builtin_amdgcn_fmed3f(rintf(__builtin_fmaf(a1, a1_mul, trow[-(int)(WW_META(kb, r) & 1023u)])), -128.f, 127.f);   // qact2
          float xi = a2;
          if constexpr (TAP) if (qi < N && kb * 16 + 4 * g + r < N) {            // the two QActs in front of the mask, from the registers that feed the next step
            const long long at = ((((long long)b * nW + w) * a.H + head) * N + qi) * a.pitch + kb * 16 + 4 * g + r;
            if (a.attn1_codes) a.attn1_codes[at] = (int8_t)(int)a1;
            if (a.qact2_codes) a.qact2_codes[at] = (int8_t)(int)a2;
          }
          if (MASK) xi -= (WW_META(kb, r) >> 10) != reg_i ? m100 : 0.f;
          if (WW_PAD(kb, r)) xi = kb * 16 + 4 * g + r < N ? xi : -3.0e9f;
          xs[kb][r] = xi;
          mx = fmaxf(mx, xi);
        }
        __builtin_amdgcn_sched_barrier(0);                                     // keep live ranges short
      }
    };
    if (a.wa.region) scores(std::integral_constant<bool, true>{});             // wave-uniform
    else scores(std::integral_constant<bool, false>{});
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    long long S = 0;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (WW_DEAD(kb, r)) continue;
        int d = (int)fminf(mx - xs[kb][r], 256.f);                             // integral values: exact
        if (WW_PAD(kb, r)) d = kb * 16 + 4 * g + r < N ? d : 257;
        s1[kb][r] = d;
        S += lutE[d];
        if (r == 3) __builtin_amdgcn_sched_barrier(0);
      }
    S += __shfl_xor(S, 16);
    S += __shfl_xor(S, 32);
    const float Sf = (float)S;
    const double Sd = (double)Sf;
    v4f o[2] = {(v4f){0.f, 0.f, 0.f, 0.f}, (v4f){0.f, 0.f, 0.f, 0.f}};
    v4i va_prev[2] = {(v4i){0, 0, 0, 0}, (v4i){0, 0, 0, 0}}, pb_prev = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      unsigned pk[4];
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) {
        float ratio[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int jj = 2 * e2 + e;
          const int kb = 2 * p + (jj >> 2), r = jj & 3;
          if (kb >= NKB || WW_DEAD(kb, r)) {
            ratio[e] = 4.0e9f;                                                 // -> probability 0
            continue;
          }
          // correctly rounded fp32 quotient, as in k_lis_attention; a padding key (entry 257: reciprocal 1) gives sum / 1 >= 2^32 -> k clamps -> 0
          ratio[e] = rintf((float)(Sd * lutFR[s1[kb][r]]));
          if constexpr (TAP) if (qi < N && kb * 16 + 4 * g + r < N) {
            const int k = (int)((__float_as_uint(ratio[e]) + 0x00400000u) >> 23) - 127;
            const long long trow = (((long long)b * nW + w) * a.H + head) * N + qi;
            if (a.probs_k) a.probs_k[trow * N + kb * 16 + 4 * g + r] = (int8_t)(k >= klim ? 16 : k);
            if (a.probs_kp) a.probs_kp[trow * a.pitch + kb * 16 + 4 * g + r] = (int8_t)(k >= klim ? 16 : k);
          }
        }
        pk[e2] = lis_prob_pair(ratio[0], ratio[1], kc);          // 2^-k * 2^-(127 - klim) as bf16, 0 from k = klim on (see k_lis_attention)
      }
      const v4i pb = {(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
      const v8bf fb = __builtin_bit_cast(v8bf, pb);
      // both V^T fragments are in registers before either MFMA is issued, and the operands of the previous pair's MFMAs stay allocated
      // until this pair's table gathers and fragment loads are issued (see WW_KEEP)
      v4i va[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const unsigned short* vp = &sVt[(dt * 16 + l15) * VSTRIDE + p * 32 + 4 * g];
        const uint2 lo = *reinterpret_cast<const uint2*>(vp);
        const uint2 hi = *reinterpret_cast<const uint2*>(vp + 16);
        va[dt] = (v4i){(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
      }
      __builtin_amdgcn_sched_barrier(0);
      WW_KEEP(va_prev[0]);
      WW_KEEP(va_prev[1]);
      WW_KEEP(pb_prev);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, va[dt]), fb, o[dt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      va_prev[0] = va[0];
      va_prev[1] = va[1];
      pb_prev = pb;
    }
    if (qi < N) {
      int8_t* dst = a.out + ((long long)b * a.T + rowq) * ldo + head * WW_HD + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        *reinterpret_cast<unsigned*>(dst + dt * 16) = pack4_rne_sat(o[dt][0] * av_mul, o[dt][1] * av_mul, o[dt][2] * av_mul, o[dt][3] * av_mul);
    }
    WW_KEEP(va_prev[0]);                                                         // ... past the output conversion: the next block's loads come behind it
    WW_KEEP(va_prev[1]);
    WW_KEEP(pb_prev);
  }
}

template <int WS, bool TAP>
static int launch_winattn_wide_t(const WinAttnArgs& a, hipStream_t st) {
  constexpr size_t smem = WinWide<WS>::SMEM;
  const int hgroups = (a.H + 3) / 4;
  const dim3 grid((unsigned)(a.B * a.wa.n_windows * hgroups));
  if (smem > 64 * 1024) {          // 12 x 12: beyond the default dynamic LDS limit
    static P2vLdsGrant grant = {};
    const hipError_t e = grant.ensure(reinterpret_cast<const void*>(&k_window_attention_wide<WS, TAP>), (int)smem);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL((k_window_attention_wide<WS, TAP>), grid, dim3(256), smem, st, a);
  CHECK_LAUNCH();
  return 0;
}

// windows of 9 x 9 ... 12 x 12 (p2v_launch_window_attention routes them here); -1: no instantiation
int p2v_launch_window_attention_wide(const WinAttnArgs& a, hipStream_t st) {
  // [ws - 9][untapped]
  static int (*const table[4][2])(const WinAttnArgs&, hipStream_t) = {{launch_winattn_wide_t<9, true>, launch_winattn_wide_t<9, false>},
                                                                      {launch_winattn_wide_t<10, true>, launch_winattn_wide_t<10, false>},
                                                                      {launch_winattn_wide_t<11, true>, launch_winattn_wide_t<11, false>},
                                                                      {launch_winattn_wide_t<12, true>, launch_winattn_wide_t<12, false>}};
  if (a.wa.ws < 9 || a.wa.ws > 12) return -1;
  return table[a.wa.ws - 9][a.tapped() ? 0 : 1](a, st);
}
