// p2vit_gram.hip -- Gram matrices of a stage's int8 codes (p2v_code_grams / p2v_forward_grams, include/p2vit.h): G[i][j] = sum over the
// rows x cols elements of samples i and j of v_i * v_j, v = code * 2^shift[c], as an exact integer.
//
// A stage is n <= 512 samples of up to 2^31 elements: tall and skinny, like the fp32 Grams of p2vit_cka.hip, so the contraction is split.
// The K axis of v_mfma_i32_32x32x32_i8 is the feature axis of a sample, so X is its own B operand: lane (r, h) of the A operand holds 16
// bytes of sample ti * 32 + r, of the B operand the SAME 16 bytes of sample tj * 32 + r (the sum over k does not depend on how the 32 bytes
// of a step are dealt to the lanes, only on both operands dealing them alike).
//   k_gram_partial  one workgroup per (32 x 32 output tile with ti <= tj, chunk of P2V_GRAM_CHUNK = 8192 features).  A sample is walked as
//                   rows x 16-byte column groups (the last group of a row is zero-filled beyond `cols`); the four waves take a quarter of
//                   the chunk's 512 groups each, two groups (lane halves h = 0 / 1) per k-step.  The int32 accumulators of the four waves
//                   are added in int64 and stored as [chunk][tile][32][32]
//   k_gram_reduce   one thread per entry of G: the chunk partials in chunk order (int64), converted once; (i, j) with i > j reads the
//                   mirror entry, so G is exactly symmetric
//   k_gram_centre   p2v_cka_centre: k_cka_centre's rule on raw fp64 Grams with a row pitch (diagonal entries are never read)
// Overflow.  |code * code| <= 2^14 and a chunk holds 8192 = 2^13 features: a chunk's sum is at most 2^27 < 2^31 (a wave's share a quarter of
// that).  Shifted stages keep `code` on the A side and split w = code * 4^m (|w| <= 2^13) = 128 * b1 + b0 with b1 = (w + 64) >> 7 in
// [-64, 64] and b0 = w - 128 * b1 in [-64, 63] on the B side: two MFMAs per step, products at most 2^7 * 2^6 = 2^13, a chunk's sums at
// most 2^26 each; they are combined as 128 * S1 + S0 in int64.  No atomics, fixed order: bitwise repeatable.
#include "p2vit_device.h"

#define GRAM_GROUPS (P2V_GRAM_CHUNK / 16)     // 16-byte groups per chunk
#define GRAM_WAVE_STEPS (GRAM_GROUPS / 4 / 2) // k-steps of a wave
#define GRAM_STEPS 4                          // k-steps requested before the first MFMA waits

// tile index -> (ti, tj) of the upper triangle, row by row
__device__ __forceinline__ void gram_tile_of(int t, int T, int& ti, int& tj) {
  ti = 0;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  tj = ti + t;
}

// 16 bytes at p[0 .. 16) of which the first `valid` exist (the scalar tail of cos_load_i8); bytes beyond are zero and never read
__device__ __forceinline__ v4i gram_bytes(const int8_t* p, int valid, bool vec) {
  if (vec && valid >= 16) return *reinterpret_cast<const v4i*>(p);
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < valid) w[k >> 2] |= (unsigned)(unsigned char)p[k] << (8 * (k & 3));
  return (v4i){(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
}

// column group `cgi` of row `row` of a sample (null sample, a row beyond the stage: zeros)
__device__ __forceinline__ v4i gram_load(const int8_t* sample, long long row, int cgi, const GramDesc& d) {
  if (!sample || row >= d.rows) return (v4i){0, 0, 0, 0};
  return gram_bytes(sample + row * d.row_stride + 16 * cgi, d.cols - 16 * cgi, d.vec != 0);
}

// w = code * 4^m of 16 codes -> the byte planes b1, b0 with w = 128 * b1 + b0
__device__ __forceinline__ void gram_split(const v4i& codes, const v4i& shifts, v4i& b1, v4i& b0) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned hi = 0u, lo = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = (int)(signed char)((unsigned)codes[q] >> (8 * k));
      const int m = (int)(((unsigned)shifts[q] >> (8 * k)) & 3u);
      const int w = c << (2 * m);                      // c * 4^m (an arithmetic shift of a two's-complement int)
      const int h1 = (w + 64) >> 7;
      const int h0 = w - (h1 << 7);
      hi |= ((unsigned)h1 & 255u) << (8 * k);
      lo |= ((unsigned)h0 & 255u) << (8 * k);
    }
    b1[q] = (int)hi;
    b0[q] = (int)lo;
  }
}

template <bool SHIFT>
__global__ __launch_bounds__(256) void k_gram_partial(GramDesc d, int n, long long* __restrict__ partials) {
  __shared__ int red[SHIFT ? 2 : 1][4][1024];
  const int T = (n + 31) / 32, ntiles = T * (T + 1) / 2;
  const int tile = (int)(blockIdx.x % (unsigned)ntiles), chunk = (int)(blockIdx.x / (unsigned)ntiles);   // the tiles of a chunk side by side (shared rows in L2)
  int ti, tj;
  gram_tile_of(tile, T, ti, tj);
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = ti * 32 + r, j = tj * 32 + r;
  const int8_t* xa = i < n ? d.base + (long long)i * d.sample_stride : nullptr;
  const int8_t* xb = j < n ? d.base + (long long)j * d.sample_stride : nullptr;
  const bool diag = ti == tj;                                       // the B fragments are the A fragments
  const long long g0 = (long long)chunk * GRAM_GROUPS + (long long)wave * (GRAM_GROUPS / 4);   // first group of this wave
  long long row = (g0 + h) / d.cg;
  int cgi = (int)((g0 + h) % d.cg);
  const bool svec = SHIFT && ((unsigned long long)d.shift % 16 == 0);

  v16i acc[SHIFT ? 2 : 1];
#pragma unroll
  for (int a = 0; a < (SHIFT ? 2 : 1); ++a)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[a][q] = 0;

  for (int s = 0; s < GRAM_WAVE_STEPS; s += GRAM_STEPS) {
    if (g0 + 2 * s >= d.groups) break;                              // wave-uniform: nothing of the sample is left
    v4i fa[GRAM_STEPS], fb[GRAM_STEPS], fs[GRAM_STEPS];
#pragma unroll
    for (int u = 0; u < GRAM_STEPS; ++u) {
      fa[u] = gram_load(xa, row, cgi, d);
      fb[u] = diag ? fa[u] : gram_load(xb, row, cgi, d);
      if constexpr (SHIFT) fs[u] = row < d.rows ? gram_bytes(reinterpret_cast<const int8_t*>(d.shift) + 16 * cgi, d.cols - 16 * cgi, svec) : (v4i){0, 0, 0, 0};
      cgi += 2;                                                     // the next step of this lane half: two groups on
      while (cgi >= d.cg) { cgi -= d.cg; ++row; }
    }
#pragma unroll
    for (int u = 0; u < GRAM_STEPS; ++u) {
      if constexpr (SHIFT) {
        v4i b1, b0;
        gram_split(fb[u], fs[u], b1, b0);
        acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[u], b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[u], b1, acc[1], 0, 0, 0);
      } else {
        acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[u], fb[u], acc[0], 0, 0, 0);
      }
    }
  }
  // C/D map of the 32x32 MFMA: register q of lane (r, h) -> row (q & 3) + 8 (q >> 2) + 4 h (the A operand's sample), column r (the B operand's)
#pragma unroll
  for (int a = 0; a < (SHIFT ? 2 : 1); ++a)
#pragma unroll
    for (int q = 0; q < 16; ++q) red[a][wave][((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc[a][q];
  __syncthreads();
  long long* out = partials + ((long long)chunk * ntiles + tile) * 1024;
  for (int e = threadIdx.x; e < 1024; e += 256) {
    long long s0 = ((long long)red[0][0][e] + red[0][1][e]) + ((long long)red[0][2][e] + red[0][3][e]);
    if constexpr (SHIFT) {
      const long long s1 = ((long long)red[1][0][e] + red[1][1][e]) + ((long long)red[1][2][e] + red[1][3][e]);
      s0 += 128 * s1;
    }
    out[e] = s0;
  }
}

__global__ __launch_bounds__(256) void k_gram_reduce(int n, int nchunks, const long long* __restrict__ partials, double* __restrict__ G) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)n * n) return;
  const int i = (int)(idx / n), j = (int)(idx % n);
  const int a = i < j ? i : j, b = i < j ? j : i;                   // the mirror entry of the upper triangle (exact symmetry)
  const int T = (n + 31) / 32, ti = a >> 5, tj = b >> 5, ntiles = T * (T + 1) / 2;
  const int tile = ti * T - ti * (ti - 1) / 2 + (tj - ti);
  const long long* p = partials + (long long)tile * 1024 + (a & 31) * 32 + (b & 31);
  const long long step = (long long)ntiles * 1024;
  long long s = 0;
  for (int c = 0; c < nchunks; ++c) s += p[c * step];
  G[idx] = (double)s;
}

// one workgroup per layer; raw entry (i, j) of layer l at raw[l * layer_stride + i * pitch + j]
__global__ __launch_bounds__(256) void k_gram_centre(int n, const double* __restrict__ raw, long long pitch, long long layer_stride,
                                                     float* __restrict__ grams) {
  __shared__ double means[P2V_GRAM_MAX_N];
  __shared__ double corr;
  const long long nn = (long long)n * n;
  const double* G = raw + blockIdx.x * layer_stride;
  float* out = grams + blockIdx.x * nn;
  for (int t = threadIdx.x; t < n; t += 256) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += i == t ? 0.0 : G[(long long)i * pitch + t];   // gram.fill_diagonal_(0); gram.sum(0)
    means[t] = s / (double)(n - 2);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += means[k];
    corr = s / (double)(2 * (n - 1));
  }
  __syncthreads();
  for (int t = threadIdx.x; t < n; t += 256) means[t] -= corr;
  __syncthreads();
  for (long long e = threadIdx.x; e < nn; e += 256) {
    const int i = (int)(e / n), j = (int)(e % n);
    out[e] = i == j ? 0.f : (float)((G[(long long)i * pitch + j] - means[j]) - means[i]);
  }
}

// ---------------------------------------------------------------------------------------------------
// host launchers (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
GramDesc p2v_gram_desc(const p2v_gram_layer& l) {
  GramDesc d;
  d.base = reinterpret_cast<const int8_t*>(l.base);
  d.shift = l.shift;
  d.sample_stride = l.sample_stride;
  d.row_stride = l.row_stride;
  d.rows = l.rows;
  d.cols = l.cols;
  d.cg = (l.cols + 15) / 16;
  d.groups = (long long)l.rows * d.cg;
  d.nchunks = (int)((d.groups + GRAM_GROUPS - 1) / GRAM_GROUPS);
  d.vec = ((uintptr_t)l.base % 16 == 0 && l.sample_stride % 16 == 0 && l.row_stride % 16 == 0) ? 1 : 0;
  return d;
}

long long p2v_gram_items(const GramDesc& d, int n) {
  const long long T = (n + 31) / 32;
  return T * (T + 1) / 2 * d.nchunks;
}

int p2v_launch_gram_i8(const GramDesc& d, int n, long long* partials, double* G, hipStream_t st) {
  const long long items = p2v_gram_items(d, n);
  if (items >= (1LL << 31)) return -1;
  if (d.shift)
    hipLaunchKernelGGL(k_gram_partial<true>, dim3((unsigned)items), dim3(256), 0, st, d, n, partials);
  else
    hipLaunchKernelGGL(k_gram_partial<false>, dim3((unsigned)items), dim3(256), 0, st, d, n, partials);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)(((long long)n * n + 255) / 256)), dim3(256), 0, st, n, d.nchunks, partials, G);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_gram_centre(const double* raw, long long pitch, long long layer_stride, int L, int n, float* grams, hipStream_t st) {
  hipLaunchKernelGGL(k_gram_centre, dim3((unsigned)L), dim3(256), 0, st, n, raw, pitch, layer_stride, grams);
  CHECK_LAUNCH();
  return 0;
}
