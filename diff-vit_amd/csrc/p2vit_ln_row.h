// p2vit_ln_row.h -- the integer LayerNorm of one row (QIntLayerNorm mode 'int', layers.py:255-289, + /channel_scale + qact0 clamp,
// vit_fquant.py:284-289): the per-lane constants, their fold, and the four steps sums / reduce / scalars / apply.  Shared by the
// stand-alone and the fused kernels (p2vit_ln.hip) and by the kernel for rows of 2049 ... 4096 channels (p2vit_ln_xwide.hip), so that
// every LayerNorm in the library runs the same operations on the same values.
#pragma once
#include "p2vit_epilogue.h"

// sum over the 32 lanes of a half wave, result in every lane: four DPP butterflies (no address registers, VALU rate) and
// one ds_swizzle for the distance-16 step.  After the xor-1/xor-2 steps the four lanes of a quad agree, so the mirrors
// of 8 and 16 lanes act as xor-4 and xor-8.
__device__ __forceinline__ int half_wave_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);   // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);   // row_mirror
  v += __builtin_amdgcn_ds_swizzle(v, 0x401F);                      // bitmask mode: lane ^ 16
  return v;
}

// The four sums of a row pair (S1 and S2 of rows 0 and 1) over the 32 lanes of a half wave, reduced TOGETHER: the first two exchange
// steps each halve what a lane carries, so 2 + 1 + 3 cross-lane adds replace the 4 x 5 of four half_wave_sum calls (integers: any order
// is exact).  A DPP move writes only the banks (4 lanes; bit b of the mask = lanes 4b .. 4b+3 of each row of 16) its bank mask names and
// keeps `old` elsewhere, so x = (partner's p | own q), y = (own p | partner's q) and x + y is p summed in one half of the banks, q in the other:
//   row_mirror      (lane i <-> 15 - i, bank b <-> 3 - b): banks 0,1 collect row 0, banks 2,3 row 1          4 values -> 2
//   row_half_mirror (lane i <-> 7 - i, bank 0 <-> 1, 2 <-> 3): banks 0,2 collect S1, banks 1,3 S2             2 values -> 1
//   xor 1, xor 2 inside the quad (one lane of every bank has been visited: the row of 16 is complete), xor 16
// Result: S1 / S2 of row r in the lanes of bank 2r (lanes 8r .. 8r+3 and 16 + 8r .. of the half wave); the lanes of banks 1 and 3 hold
// the two sums exchanged, which nobody reads.
template <int CTRL, int BANKS_P>
__device__ __forceinline__ int dpp_halve(int p, int q) {
  const int x = __builtin_amdgcn_update_dpp(q, p, CTRL, 0xF, BANKS_P, false);
  const int y = __builtin_amdgcn_update_dpp(p, q, CTRL, 0xF, BANKS_P ^ 0xF, false);
  return x + y;
}
__device__ __forceinline__ void half_wave_sum_pair(const int (&S1)[2], const unsigned (&S2)[2], int& S1k, unsigned& S2k) {
  const int a = dpp_halve<0x140, 0x3>(S1[0], S1[1]);                 // row_mirror
  const int b = dpp_halve<0x140, 0x3>((int)S2[0], (int)S2[1]);
  int v = dpp_halve<0x141, 0x5>(a, b);                               // row_half_mirror
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
  v += __builtin_amdgcn_ds_swizzle(v, 0x401F);                      // bitmask mode: lane ^ 16
  S1k = v;
  S2k = (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);   // the quads agree: the mirror of 8 lanes is the neighbouring bank
}

// generic per-element chain: every step of get_MN / the 'int' forward as written in the reference
// os > 0: the output scale itself - the two quotients are IEEE divisions like the reference's; os == 0: multiply by io = 1/scale
// (identical for powers of two)
// ln_elem_generic_o: the rounded integer x_q of layers.py:288, in front of post_mul and the clamp (what the value tap stores times out_scale)
__device__ __forceinline__ float ln_elem_generic_o(float xq, float g, float bta, float io, float rs, float mos, float os) {
  const float A = os > 0.f ? (rs * g) / os : (rs * g) * io;        // (s1/std)*gamma / out_scale
  const float absA = fabsf(A);
  int N = 134 - (int)(__float_as_uint(absA) >> 23);                // 7 - floor(log2|A|)   (get_MN, layers.py:234-238)
  N = N < 0 ? 0 : (N > 31 ? 31 : N);
  const float M = fminf(floorf(ldexpf(absA, N)), 255.f);           // floor(|A| * 2^N), clamped
  const float sM = copysignf(M, A);                                // A.sign() * M  (M == 0 when A == 0)
  const float tb = bta - mos * g;
  const float Bv = rintf(ldexpf(os > 0.f ? tb / os : tb * io, N)); // layers.py:283-286
  return rintf(ldexpf(sM * xq + Bv, -N));                          // layers.py:288
}
__device__ __forceinline__ float ln_elem_generic(float xq, float g, float bta, float io, float pm, float rs, float mos, float os) {
  const float o = ln_elem_generic_o(xq, g, bta, io, rs, mos, os);
  return rintf(o * pm);                                            // * out_scale / cs_next / s_next (clamped by the packing)
}

// Fast chain (used when 1/out_scale is a power of two for every channel, which is the P2-ViT case, and the row's
// multipliers are inside the unclamped range of get_MN).  With io = 2^e:  A = (rs*g)*io = rs*(g*io)  and
// (b - mos*g)*io = b*io - mos*(g*io)  with the same roundings, so g*io and b*io are folded once per workgroup (shared
// through LDS).  For 2^-24 <= |A| < 2^8:  N = 134 - exp(A) is unclamped and M = floor(|A| 2^N) in [128,255] is the top
// 8 significant bits of A, i.e.  sign*M*2^-N == A with the low 16 mantissa bits cleared =: T;  and
// rint(((sM*xq + Bv) rounded) * 2^-N) == rint(fma(T, xq, Bv*2^-N))  because T*xq is exact (8 x 11 bits) and scaling by
// 2^-N commutes with the rounding.  Bit-identical to the generic chain (tests drive both through P2V_LN_GENERIC=1).
// LANES = 32: one row per half wave (C <= 1024);  LANES = 64: one row per wave (PatchMerging rows of up to 2048 channels);
// LANES = 256: one row per workgroup (p2vit_ln_xwide.hip)
// per-lane view of the folded per-channel constants of a LayerNorm (held in registers across rows)
// LDSC: post_mul and the PTF mask are re-read from the workgroup's LDS copy where they are used (one ds_read_b128 per four channels and
// row) instead of living in 8 * NCH registers - the stand-alone kernel, whose scratch stays valid, then fits two rows per batch (ln_rows)
// in the register budget of three waves per SIMD
// The lane-resident PTF mask is kept TIMES 2^-16 (LN_XS), so x_q = code * mask arrives scaled by 2^-16 for free: the fast chain multiplies it by
// T * 2^16 (below), the partial sums are scaled back once per lane and row (powers of two: every product, sum and rounding is unchanged).
#define LN_XS 0x1p-16f
#define LN_XS_INV 65536.f
__device__ __forceinline__ float4 ln_scale_mask(float4 m) { return make_float4(m.x * LN_XS, m.y * LN_XS, m.z * LN_XS, m.w * LN_XS); }
template <int NCH, bool LDSC = false>
struct LnLane {
  bool on[NCH];
  float4 gm[NCH], bt[NCH];            // gamma*io, beta*io
  float4 pm[LDSC ? 1 : NCH];          // post_mul
  float4 mkf[LDSC ? 1 : NCH];         // PTF mask (in_scale / s1): 1, 2, 4 or 8 - times LN_XS
  const float* sPl;                   // LDSC: this lane's first four channels in the LDS copies, and the chunk stride in floats
  const float* sMl;
  int cstride;
  float gmin, gmax;                   // extreme |gamma*io| over all channels
  float bmax;                         // max |beta*io| over all channels (bound of the LayerNorm offset, see ln_row)
  bool pot;                           // 1/out_scale is a power of two for every channel and the fold is exact
  bool pm_one;                        // post_mul == 1 for every channel (norm1 of P2-ViT: out_scale / channel_scale / qact0 scale): no second requant
  __device__ __forceinline__ float4 post4(int i) const { return LDSC ? *reinterpret_cast<const float4*>(sPl + i * cstride) : pm[LDSC ? 0 : i]; }
  __device__ __forceinline__ float4 mask4(int i) const { return LDSC ? *reinterpret_cast<const float4*>(sMl + i * cstride) : mkf[LDSC ? 0 : i]; }
};

// Fold, test and publish the per-channel constants once per workgroup (every thread calls it; contains a barrier), then load this
// lane's channels: lane l of a row group owns channels (l + LANES*i)*4 .. +3.  gmin / gmax / bmax come out reduced over the lane's WAVE
// (over its half wave at LANES = 32): a row group of several waves (LANES = 256) combines them itself.
template <int NCH, int LANES, class LL>
__device__ __forceinline__ void ln_prepare(const p2v_ln& ln, int C, bool force_generic, float* sG, float* sB, float* sP, int* sM,
                                           int tid, int nthreads, LL& L) {
  const int l32 = tid & (LANES - 1);
  int potf = force_generic ? 0 : 1, pm1 = 1;
  for (int t4 = tid; t4 < NCH * LANES; t4 += nthreads) {   // one thread per 4 channels: fold, test, and publish
    const int c = t4 * 4;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), b = g, io = make_float4(1.f, 1.f, 1.f, 1.f), pmv = g, mk = g;
    if (c < C) {
      g = *reinterpret_cast<const float4*>(ln.gamma + c);
      b = *reinterpret_cast<const float4*>(ln.beta + c);
      io = *reinterpret_cast<const float4*>(ln.inv_out + c);
      pmv = *reinterpret_cast<const float4*>(ln.post_mul + c);
      mk = *reinterpret_cast<const float4*>(ln.mask + c);
    }
    const float g4[4] = {g.x, g.y, g.z, g.w}, b4[4] = {b.x, b.y, b.z, b.w}, i4[4] = {io.x, io.y, io.z, io.w};
    if (c < C) pm1 &= (int)(pmv.x == 1.f) & (int)(pmv.y == 1.f) & (int)(pmv.z == 1.f) & (int)(pmv.w == 1.f);
    float go[4], bo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned ib = __float_as_uint(i4[j]);
      const int p2 = (int)((ib & 0x807FFFFFu) == 0u) & (int)((ib >> 23) - 32u <= 190u);    // +2^e, far from under/overflow
      go[j] = g4[j] * i4[j];
      bo[j] = b4[j] * i4[j];
      const float ga = fabsf(go[j]), ba = fabsf(bo[j]);
      // the fold must be exact: no product may leave the normal range
      const int gok = (int)(g4[j] == 0.f) | ((int)(ga >= 1.0e-30f) & (int)(ga <= 1.0e30f));
      const int bok = (int)(b4[j] == 0.f) | ((int)(ba >= 1.0e-30f) & (int)(ba <= 1.0e30f));
      potf &= p2 & gok & bok;
    }
    *reinterpret_cast<float4*>(sG + c) = make_float4(go[0], go[1], go[2], go[3]);
    *reinterpret_cast<float4*>(sB + c) = make_float4(bo[0], bo[1], bo[2], bo[3]);
    *reinterpret_cast<float4*>(sP + c) = pmv;
    *reinterpret_cast<float4*>(sM + c) = ln_scale_mask(mk);
  }
  L.pot = __syncthreads_and(potf) != 0;
  L.pm_one = __syncthreads_and(pm1) != 0;
  // extreme |g io| over all channels (every row group covers all of them)
  float gmin = 3.0e38f, gmax = 0.f, bmax = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (l32 + LANES * i) * 4;
    L.on[i] = c < C;
    const float4 gv = *reinterpret_cast<const float4*>(sG + c);
    L.gm[i] = gv;
    L.bt[i] = *reinterpret_cast<const float4*>(sB + c);
    if (L.on[i]) bmax = fmaxf(bmax, fmaxf(fmaxf(fabsf(L.bt[i].x), fabsf(L.bt[i].y)), fmaxf(fabsf(L.bt[i].z), fabsf(L.bt[i].w))));
    if constexpr (sizeof(L.pm) == sizeof(float4) * NCH) {          // (the register-resident form)
      L.pm[i] = *reinterpret_cast<const float4*>(sP + c);
      L.mkf[i] = *reinterpret_cast<const float4*>(sM + c);
    }
    const float lo = fminf(fminf(fabsf(gv.x), fabsf(gv.y)), fminf(fabsf(gv.z), fabsf(gv.w)));
    const float hi = fmaxf(fmaxf(fabsf(gv.x), fabsf(gv.y)), fmaxf(fabsf(gv.z), fabsf(gv.w)));
    gmin = fminf(gmin, L.on[i] ? lo : 3.0e38f);
    gmax = fmaxf(gmax, L.on[i] ? hi : 0.f);
  }
  L.sPl = sP + l32 * 4;
  L.sMl = reinterpret_cast<const float*>(sM) + l32 * 4;
  L.cstride = LANES * 4;
  {   // positive floats order like their bit patterns: integer min/max butterflies inside the half wave
    int lo = (int)__float_as_uint(gmin), hi = (int)__float_as_uint(gmax), bh = (int)__float_as_uint(bmax);
#define LN_MM(ctrl) lo = min(lo, __builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xF, 0xF, false)); hi = max(hi, __builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xF, 0xF, false)); \
                    bh = max(bh, __builtin_amdgcn_update_dpp(bh, bh, ctrl, 0xF, 0xF, false));
    LN_MM(0xB1) LN_MM(0x4E) LN_MM(0x141) LN_MM(0x140)
#undef LN_MM
    lo = min(lo, __builtin_amdgcn_ds_swizzle(lo, 0x401F));
    hi = max(hi, __builtin_amdgcn_ds_swizzle(hi, 0x401F));
    bh = max(bh, __builtin_amdgcn_ds_swizzle(bh, 0x401F));
    if (LANES >= 64) {
      lo = min(lo, __shfl_xor(lo, 32));
      hi = max(hi, __shfl_xor(hi, 32));
      bh = max(bh, __shfl_xor(bh, 32));
    }
    L.gmin = __uint_as_float((unsigned)lo);
    L.gmax = __uint_as_float((unsigned)hi);
    L.bmax = __uint_as_float((unsigned)bh);
  }
}

// The LayerNorm of a row in four steps, shared by the one-row and the batched form below:
//   ln_sums   the lane's x_q = code * mask and its part of sum x_q, sum x_q^2
//   ln_reduce the sums over the row group (32 or 64 lanes), result in every lane
//   ln_scalars mean / std -> the two row scalars rs = s1 / std, mos = mean / std and the fast-chain test
//   ln_apply  the per-element chain with those scalars -> packed output codes
template <int NCH, class LL>
__device__ __forceinline__ void ln_sums(const unsigned (&wcur)[NCH], const LL& L, float (&xq)[NCH][4], int& S1, unsigned& S2) {
  S2 = 0;                                       // C * (128*8)^2 < 2^32 is the callers' bound (2^31 at C = 2048, mask 8): exact in 32 UNSIGNED bits
  // the lane's partial sums in fp32: |x_q| <= 1024, so sum x_q of 32 values and sum x_q^2 of 16 values (<= 2^24) are exact - full-rate
  // add / fma instead of 24-bit multiplies and three-operand adds (profiles/r03_op_cost.txt); the cross-lane sums stay integers.
  // xq[][] holds x_q * 2^-16 (the mask is stored scaled, LN_XS): the sums come out times 2^-16 / 2^-32 and are scaled back per lane
  float S1p = 0.f, S2p = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const unsigned w = wcur[i];
    const float4 mk_ = L.mask4(i);
    const float m4[4] = {mk_.x, mk_.y, mk_.z, mk_.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) xq[i][j] = (float)sx8(w, j) * m4[j];       // x_q * in_scale_mask  (layers.py:269-273) * 2^-16, exact; w == 0 past C
    S1p += (xq[i][0] + xq[i][1]) + (xq[i][2] + xq[i][3]);                  // (short dependency chains: a wave may be alone on its SIMD)
    S2p += __builtin_fmaf(xq[i][1], xq[i][1], xq[i][0] * xq[i][0]) + __builtin_fmaf(xq[i][3], xq[i][3], xq[i][2] * xq[i][2]);
    if ((i & 3) == 3 || i == NCH - 1) {
      S2 += (unsigned)(S2p * (LN_XS_INV * LN_XS_INV));
      S2p = 0.f;
    }
  }
  S1 = (int)(S1p * LN_XS_INV);
}
template <int LANES>
__device__ __forceinline__ void ln_reduce(int& S1, unsigned& S2) {
  S1 = half_wave_sum(S1);
  S2 = (unsigned)half_wave_sum((int)S2);        // two's-complement adds: the unsigned total is exact
  if (LANES == 64) {
    S1 += __shfl_xor(S1, 32);
    S2 += (unsigned)__shfl_xor((int)S2, 32);
  }
}
template <int NCH, class LL>
__device__ __forceinline__ void ln_scalars(int S1, unsigned S2, const LL& L, const p2v_ln& ln, int C, float& rs, float& mos, bool& fast) {
  const float s1 = ln.s1;
  const float Cf = (float)C;
  const float s1oC = s1 / Cf;
  const float S1f = (float)S1, S2f = (float)S2;                        // (S2 converts as the UNSIGNED value: it passes 2^31 beyond 2048 channels)
  const float mean = (S1f / Cf) * s1;                                  // x_q.mean(-1) * in_scale1
  const float stdv = s1oC * sqrtf(Cf * S2f - S1f * S1f);               // layers.py:276-277
  rs = s1 / stdv;
  mos = mean / stdv;
  // |A| = RN(rs*|g io|) is monotone in |g io|: the two extreme channels bound every channel exactly
  // ... and the offset Bv = rint(t * 2^N) (t = beta*io - mos*gamma*io) is rounded by adding and subtracting 1.5 * 2^(23-N), which is
  // rint on the 2^-N grid (ties to even included) as long as |t| * 2^N < 2^22: |t| <= bmax + |mos| gmax and N <= 134 - exp(rs * gmin),
  // so one comparison per row against 2^(exp(rs*gmin) - 112) bounds every channel (1 % margin for the roundings of t itself)
  const float amin = rs * L.gmin;
  const float tlim = __uint_as_float((((__float_as_uint(amin) >> 23) & 255u) + 15u) << 23);       // 2^22 * 2^-(134 - e_min)
  fast = L.pot && amin >= 0x1p-24f && rs * L.gmax < 256.f && (L.bmax + fabsf(mos) * L.gmax) * 1.01f < tlim;
}
// the value tap of a channel group (TAP forms only): o * out_scale[c] as fp32, o = the rounded integer in front of post_mul and the clamp
// (layers.py:288-289: what a forward hook on the module sees).  out_scale = 1 / inv_out, exact for powers of two; ln.out_scale where given
__device__ __forceinline__ void ln_tap_store(float* tap, int c, const p2v_ln& ln, const float (&o)[4]) {
  float4 os;
  if (ln.out_scale) {
    os = *reinterpret_cast<const float4*>(ln.out_scale + c);
  } else {
    const float4 io = *reinterpret_cast<const float4*>(ln.inv_out + c);
    os = make_float4(1.0f / io.x, 1.0f / io.y, 1.0f / io.z, 1.0f / io.w);
  }
  *reinterpret_cast<float4*>(tap + c) = make_float4(o[0] * os.x, o[1] * os.y, o[2] * os.z, o[3] * os.w);
}

// TAP: `tap` (the row's fp32 [C] values, or null for a row that is not stored) also receives o * out_scale; the codes are formed by the
// same instructions on the same values as without it
template <int NCH, int LANES, class LL, bool TAP = false>
__device__ __forceinline__ void ln_apply(const float (&xq)[NCH][4], const LL& L, const p2v_ln& ln, int l32, float rs, float mos, bool fast,
                                         unsigned (&outw)[NCH], float* tap = nullptr) {
  if (fast) {
    // A2 = A * 2^16 (rs scaled once per row): sign * M * 2^-N * 2^16 = A2 with its low 16 mantissa bits cleared multiplies the SCALED x_q
    // (xq[][] = x_q * 2^-16, LN_XS) - the same exact product as before; t = beta*io - mos*gamma*io is unchanged; and the magic constant of the
    // offset rounding, 1.5 * 2^(23-N), has exactly A2's exponent field: ONE v_and_or_b32 (round 3: and + add of 16 to the field)
    const float rs2 = rs * LN_XS_INV;
    auto chain = [&](auto PM1c) {
      constexpr bool PM1 = decltype(PM1c)::value;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const float g4[4] = {L.gm[i].x, L.gm[i].y, L.gm[i].z, L.gm[i].w}, b4[4] = {L.bt[i].x, L.bt[i].y, L.bt[i].z, L.bt[i].w};
        float p4[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (!PM1) {
          const float4 pm_ = L.post4(i);
          p4[0] = pm_.x; p4[1] = pm_.y; p4[2] = pm_.z; p4[3] = pm_.w;
        }
        float q[4];
        float ot[TAP ? 4 : 1];
#pragma unroll
        for (int j = 0; j < 4; j += 2) {   // two channels at a time: only the 3-source fma is packed (measured on gfx950, tools/ubench/valu_rate:
          // a wave alone on its SIMD issues a 2-source fp32 op every ~4.9 cycles, a v_pk_mul/add_f32 every ~13, a 3-source v_fma_f32 every ~8, v_pk_fma_f32 ~13)
          v2f T2, Bq2;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float A2 = rs2 * g4[j + e];                                       // A * 2^16 (exact scaling)
            const float t = b4[j + e] - mos * g4[j + e];
            const unsigned Ab = __float_as_uint(A2);
            T2[e] = __uint_as_float(Ab & 0xFFFF0000u);                              // sign * M * 2^-N * 2^16
            // Bv * 2^-N = t rounded to the 2^-N grid, N = 134 - exp(A): C = 1.5 * 2^(23-N) has the exponent field exp(A) + 16 = exp(A2)
            // (3 full-rate instructions instead of bfe, add, sub, ldexp, rndne, ldexp: tools/ubench/op_cost.hip, profiles/r03_op_cost.txt)
            unsigned Cmb;       // (Ab & 0x7F800000) | 0x00400000 as ONE instruction (hipcc emits and + or: a VOP3 takes no literal, so the two
                                // constants sit in a scalar and a vector register)
            asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(Cmb) : "v"(Ab), "s"(0x7F800000u), "v"(0x00400000u));
            const float Cm = __uint_as_float(Cmb);
            Bq2[e] = (t + Cm) - Cm;
          }
          const v2f x2 = {xq[i][j], xq[i][j + 1]};
          const v2f o2 = __builtin_elementwise_fma(T2, x2, Bq2);
          if (PM1) {                                                                // out * 1: the LayerNorm output IS the code
            q[j] = o2[0];
            q[j + 1] = o2[1];
          } else {
            q[j] = rintf(o2[0]) * p4[j];
            q[j + 1] = rintf(o2[1]) * p4[j + 1];
          }
          if constexpr (TAP) {
            ot[j] = rintf(o2[0]);
            ot[j + 1] = rintf(o2[1]);
          }
        }
        outw[i] = pack4_rne_sat(q[0], q[1], q[2], q[3]);                            // the (last) rounding is the packing's
        if constexpr (TAP)
          if (tap && L.on[i]) ln_tap_store(tap, (l32 + LANES * i) * 4, ln, ot);
      }
    };
    if (L.pm_one) chain(std::integral_constant<bool, true>{});      // wave-uniform
    else chain(std::integral_constant<bool, false>{});
  } else {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cc = L.on[i] ? (l32 + LANES * i) * 4 : 0;
      const float4 gv = *reinterpret_cast<const float4*>(ln.gamma + cc), bv = *reinterpret_cast<const float4*>(ln.beta + cc);
      const float4 iv = *reinterpret_cast<const float4*>(ln.inv_out + cc), pv = *reinterpret_cast<const float4*>(ln.post_mul + cc);
      const float g4[4] = {gv.x, gv.y, gv.z, gv.w}, b4[4] = {bv.x, bv.y, bv.z, bv.w};
      const float i4[4] = {iv.x, iv.y, iv.z, iv.w}, p4[4] = {pv.x, pv.y, pv.z, pv.w};
      float4 ov = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ln.out_scale) ov = *reinterpret_cast<const float4*>(ln.out_scale + cc);
      const float o4[4] = {ov.x, ov.y, ov.z, ov.w};
      float q[4];
      if constexpr (TAP) {
        float ot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ot[j] = ln_elem_generic_o(xq[i][j] * LN_XS_INV, g4[j], b4[j], i4[j], rs, mos, o4[j]);
          q[j] = rintf(ot[j] * p4[j]);
        }
        if (tap && L.on[i]) ln_tap_store(tap, cc, ln, ot);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = ln_elem_generic(xq[i][j] * LN_XS_INV, g4[j], b4[j], i4[j], p4[j], rs, mos, o4[j]);
      }
      outw[i] = pack4_sat(q[0], q[1], q[2], q[3]);
    }
  }
}

// One row: packed input codes wcur[i] (0 where the lane's channels lie past C) -> packed output codes outw[i].  Every lane of the
// row group (32 or 64 lanes) must call it: the sums are cross-lane reductions.
template <int NCH, int LANES, class LL, bool TAP = false>
__device__ __forceinline__ void ln_row(const unsigned (&wcur)[NCH], const LL& L, const p2v_ln& ln, int C, int l32, unsigned (&outw)[NCH],
                                       float* tap = nullptr) {
  float xq[NCH][4], rs, mos;
  int S1;
  unsigned S2;
  bool fast;
  ln_sums<NCH>(wcur, L, xq, S1, S2);
  ln_reduce<LANES>(S1, S2);
  ln_scalars<NCH>(S1, S2, L, ln, C, rs, mos, fast);
  ln_apply<NCH, LANES, LL, TAP>(xq, L, ln, l32, rs, mos, fast, outw, tap);
}

// R rows of a row group at once (round 3).  The row scalars - three IEEE divisions, a square root and the range tests, ~55 instructions
// that every lane of the group would repeat per row - are computed ONCE for the R rows: lane l keeps the sums of row (l mod R), runs the
// scalar chain on them, and row r's results are read back from lane r of the group (ds_bpermute).  Same operations on the same values
// as ln_row, only in other lanes: bit-identical.
template <int NCH, int LANES, int R, class LL, bool TAP = false>
__device__ __forceinline__ void ln_rows(const unsigned (&wcur)[R][NCH], const LL& L, const p2v_ln& ln, int C, int l32, unsigned (&outw)[R][NCH],
                                        float* const* taps = nullptr) {
  static_assert((R & (R - 1)) == 0 && R <= 8, "rows per batch");
  float xq[R][NCH][4];
  int S1k = 0;
  unsigned S2k = 0;
  const int mine = l32 & (R - 1);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int S1;
    unsigned S2;
    ln_sums<NCH>(wcur[r], L, xq[r], S1, S2);
    ln_reduce<LANES>(S1, S2);
    S1k = mine == r ? S1 : S1k;
    S2k = mine == r ? S2 : S2k;
  }
  float rs, mos;
  bool fast;
  ln_scalars<NCH>(S1k, S2k, L, ln, C, rs, mos, fast);
  const int fasti = fast ? 1 : 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float rs_r = __shfl(rs, r, LANES), mos_r = __shfl(mos, r, LANES);
    const bool fast_r = __shfl(fasti, r, LANES) != 0;
    ln_apply<NCH, LANES, LL, TAP>(xq[r], L, ln, l32, rs_r, mos_r, fast_r, outw[r], TAP ? taps[r] : nullptr);
  }
}
