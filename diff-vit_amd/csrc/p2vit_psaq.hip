// p2vit_psaq.hip -- the patch-similarity entropy of PSAQ-ViT's data generator and its gradient (p2v_patch_similarity_entropy,
// include/p2vit.h; generate_data.py:102-113, 128-134 with utils/kde.py:87-96 of the reference).
//
// av is [B*G][H][N][hd] fp32, one block's attn @ v.  Per group of one image: a = mean over heads of rows 1 .. N-1 (T = N - 1 rows of hd),
// A^ = a / max(|a|, 1e-8), S = A^ A^T; over the WHOLE call lo = min S, hi = max S, ten points x_k = linspace(lo, hi, 10); per image, over
// its n = G T^2 similarities, p_k = (c / n) sum_m exp(-(x_k - s_m)^2 / (2 h^2)), q = p + 1e-4, f = -q ln q, E_b = trapezoid of f over x;
// value = mean_b E_b.  The gradient is closed-form: Gamma = d value / d S element-wise from S, (Gamma + Gamma^T) A^ per group, then the
// normalisation, then / H into every head; row 0 of every group is zero.
//   k_psaq_rows     32 lanes per patch row: head mean in head order, |a|, A^ and |a| to the workspace
//   k_psaq_sims     one wave per 32 x 32 tile of the upper triangle of S on v_mfma_f32_32x32x2_f32 (exact fp32, an fmaf chain over hd);
//                   the tile and its mirror image are stored, so S is symmetric bit for bit; min / max of the workgroup to a partial
//   k_psaq_range    one workgroup: the partials -> lo, hi
//   k_psaq_density  one workgroup per (image, chunk of 4096 similarities): the ten point sums in fp64, a partial per chunk
//   k_psaq_finish   one workgroup: per image the chunk partials in chunk order, q, f, E_b and the ten coefficients
//                   w_k (-(ln q_k + 1)) (c / n) / (B h^2) of the gradient in fp64; value = mean E_b by a fixed tree
//   k_psaq_grad     one workgroup per (group, 32 patch rows): M = 2 Gamma(S) (S is symmetric) element-wise, M A^ on the MFMA - the four
//                   waves split the key rows and are added in wave order through LDS -, then d / d a = (g - A^ (A^ . g)) / |a| (g / eps
//                   under the clamp), / H, one store per head
// No atomics, every sum in a fixed order: the same input gives the same bytes.  The exponential's argument is formed in fp64 from the fp32
// similarity and rounded once; expf is the accurate one (the exponentials are 20 per similarity, far from a bottleneck).
#include <math.h>

#include "p2vit_device.h"

#define PSAQ_EPS 1e-8f
#define PSAQ_INV_2H2 5000.0                  // 1 / (2 h^2), h = 0.01
#define PSAQ_INV_H2 10000.0                  // 1 / h^2
#define PSAQ_C 39.894228040143268            // 1 / sqrt(2 pi h^2)

// linspace(lo, hi, 10) of the fp32 range, in fp64, from both ends like torch's
__device__ __forceinline__ void psaq_points(const float* __restrict__ range, double (&x)[PSAQ_POINTS]) {
  const double lo = (double)range[0], hi = (double)range[1], step = (hi - lo) / (PSAQ_POINTS - 1);
#pragma unroll
  for (int k = 0; k < PSAQ_POINTS; ++k) x[k] = k < PSAQ_POINTS / 2 ? lo + step * k : hi - step * (PSAQ_POINTS - 1 - k);
}

__device__ __forceinline__ float psaq_kernel(double d) { return expf((float)(-(d * d) * PSAQ_INV_2H2)); }

__global__ __launch_bounds__(256) void k_psaq_rows(const float* __restrict__ av, long long rows, int T, int H, int N, int hd,
                                                   float* __restrict__ ahat, float* __restrict__ norms) {
  const long long row = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int c = threadIdx.x & 31;
  const bool live = row < rows && 4 * c < hd;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const long long bg = row / T;
    const int t = (int)(row % T);
    const float* p = av + ((bg * H) * N + (t + 1)) * (long long)hd + 4 * c;
    for (int h = 0; h < H; ++h) {
      const float4 v = *reinterpret_cast<const float4*>(p + (long long)h * N * hd);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float fh = (float)H;
    s.x /= fh; s.y /= fh; s.z /= fh; s.w /= fh;
  }
  float ss = (s.x * s.x + s.y * s.y) + (s.z * s.z + s.w * s.w);
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 32);
  const float nrm = sqrtf(ss), den = fmaxf(nrm, PSAQ_EPS);
  if (live) {
    *reinterpret_cast<float4*>(ahat + row * hd + 4 * c) = make_float4(s.x / den, s.y / den, s.z / den, s.w / den);
    if (c == 0) norms[row] = nrm;
  }
}

// tile index -> (ti, tj) of the upper triangle, row by row
__device__ __forceinline__ void psaq_tile_of(int t, int TT, int& ti, int& tj) {
  ti = 0;
  while (t >= TT - ti) { t -= TT - ti; ++ti; }
  tj = ti + t;
}

__global__ __launch_bounds__(256) void k_psaq_sims(const float* __restrict__ ahat, int T, int hd, int nblk, float* __restrict__ sims,
                                                   float2* __restrict__ mm) {
  __shared__ float red[2][4];
  const long long bg = blockIdx.x / (unsigned)nblk;
  const int blk = (int)(blockIdx.x % (unsigned)nblk);
  const int TT = (T + 31) / 32, ntiles = TT * (TT + 1) / 2;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blk * 4 + wave;
  float lo = INFINITY, hi = -INFINITY;
  if (tile < ntiles) {                                              // wave-uniform
    int ti, tj;
    psaq_tile_of(tile, TT, ti, tj);
    const int i = ti * 32 + r, j = tj * 32 + r;
    const float* A = ahat + bg * T * hd;
    const float* xa = i < T ? A + (long long)i * hd : nullptr;
    const float* xb = j < T ? A + (long long)j * hd : nullptr;
    v16f acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int f = 0; f < hd; f += 8) {
      // lane (r, h) supplies A[i = r][k = h] and B[k = h][j = r] of the same feature: D[i][j] += a^_i . a^_j
      const int col = f + 4 * h;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 a = xa && col < hd ? *reinterpret_cast<const float4*>(xa + col) : z;
      const float4 b = xb && col < hd ? *reinterpret_cast<const float4*>(xb + col) : z;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    // C/D map of the 32x32 MFMA: register q of lane (r, h) -> row (q & 3) + 8 (q >> 2) + 4 h, column r
    float* S = sims + bg * T * T;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = ti * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
      if (row < T && j < T) {
        const float v = acc[q];
        S[(long long)row * T + j] = v;
        if (ti != tj) S[(long long)j * T + row] = v;                // the mirror tile: S[j][i] is this very number
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if (lane == 0) { red[0][wave] = lo; red[1][wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0)
    mm[blockIdx.x] = make_float2(fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3])),
                                 fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3])));
}

__global__ __launch_bounds__(256) void k_psaq_range(const float2* __restrict__ mm, long long count, float* __restrict__ range) {
  __shared__ float red[2][4];
  float lo = INFINITY, hi = -INFINITY;
  for (long long e = threadIdx.x; e < count; e += 256) {
    const float2 v = mm[e];
    lo = fminf(lo, v.x);
    hi = fmaxf(hi, v.y);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    range[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    range[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

__global__ __launch_bounds__(256) void k_psaq_density(const float* __restrict__ sims, long long n, int chunks, const float* __restrict__ range,
                                                      double* __restrict__ psums) {
  __shared__ double red[4][PSAQ_POINTS];
  const long long b = blockIdx.x / (unsigned)chunks;
  const int ch = (int)(blockIdx.x % (unsigned)chunks);
  double x[PSAQ_POINTS], acc[PSAQ_POINTS];
  psaq_points(range, x);
#pragma unroll
  for (int k = 0; k < PSAQ_POINTS; ++k) acc[k] = 0.0;
  const float* s = sims + b * n;
  const long long e0 = (long long)ch * PSAQ_CHUNK, e1 = e0 + PSAQ_CHUNK < n ? e0 + PSAQ_CHUNK : n;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const double sv = (double)s[e];
#pragma unroll
    for (int k = 0; k < PSAQ_POINTS; ++k) acc[k] += (double)psaq_kernel(x[k] - sv);
  }
#pragma unroll
  for (int k = 0; k < PSAQ_POINTS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < PSAQ_POINTS)
    psums[(long long)blockIdx.x * PSAQ_POINTS + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_psaq_finish(const double* __restrict__ psums, int B, long long n, int chunks,
                                                     const float* __restrict__ range, double* __restrict__ coef, double* __restrict__ value) {
  __shared__ double red[256];
  double x[PSAQ_POINTS];
  psaq_points(range, x);
  const double delta = ((double)range[1] - (double)range[0]) / (PSAQ_POINTS - 1);
  const double cn = PSAQ_C / (double)n;
  double mine = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < PSAQ_POINTS; ++k) {
      double p = 0.0;
      for (int c = 0; c < chunks; ++c) p += psums[((long long)b * chunks + c) * PSAQ_POINTS + k];
      const double q = cn * p + 1e-4, lq = log(q);
      const double w = (k == 0 || k == PSAQ_POINTS - 1) ? 0.5 * delta : delta;
      e += w * (-q * lq);
      coef[(long long)b * PSAQ_POINTS + k] = w * (-(lq + 1.0)) * cn * PSAQ_INV_H2 / (double)B;
    }
    mine += e;
  }
  red[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) value[0] = red[0] / (double)B;
}

template <int NC>
__global__ __launch_bounds__(256) void k_psaq_grad(const float* __restrict__ sims, const float* __restrict__ ahat, const float* __restrict__ norms,
                                                   const float* __restrict__ range, const double* __restrict__ coef, int G, int T, int H, int N,
                                                   int hd, float* __restrict__ grad) {
  __shared__ float g_s[32][NC * 32 + 1];
  __shared__ float dot_s[32];
  const int TT = (T + 31) / 32;
  const long long bg = blockIdx.x / (unsigned)TT;
  const int i0 = (int)(blockIdx.x % (unsigned)TT) * 32;
  const long long b = bg / G;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double x[PSAQ_POINTS], cf[PSAQ_POINTS];
  psaq_points(range, x);
#pragma unroll
  for (int k = 0; k < PSAQ_POINTS; ++k) cf[k] = coef[b * PSAQ_POINTS + k];
  const float* S = sims + bg * T * T;
  const float* A = ahat + bg * T * hd;
  const int i = i0 + r;
  v16f acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[c][q] = 0.f;
  for (int j0 = wave * 32; j0 < T; j0 += 128) {                     // the key tiles of this wave
    for (int kk = 0; kk < 32 && j0 + kk < T; kk += 2) {
      const int j = j0 + kk + h;
      // lane (r, h) supplies M[i = r][k = h] = (Gamma + Gamma^T)[i][j] = 2 Gamma(S[j][i]) and A^[j][column r] of every column tile
      float m = 0.f;
      if (i < T && j < T) {
        const double sv = (double)S[(long long)j * T + i];
        double gam = 0.0;
#pragma unroll
        for (int k = 0; k < PSAQ_POINTS; ++k) {
          const double d = x[k] - sv;
          gam += cf[k] * (double)psaq_kernel(d) * d;
        }
        m = (float)(2.0 * gam);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = c * 32 + r;
        const float bv = j < T && col < hd ? A[(long long)j * hd + col] : 0.f;
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(m, bv, acc[c], 0, 0, 0);
      }
    }
  }
  // the four waves' shares in wave order (C/D map: register q of lane (r, h) -> row (q & 3) + 8 (q >> 2) + 4 h, column r)
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
          g_s[row][c * 32 + r] = w == 0 ? acc[c][q] : g_s[row][c * 32 + r] + acc[c][q];
        }
    }
    __syncthreads();
  }
  {  // A^ . g per row: eight threads a row
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    float dot = 0.f;
    if (i0 + row < T)
      for (int d = sub; d < hd; d += 8) dot += A[(long long)(i0 + row) * hd + d] * g_s[row][d];
    dot += __shfl_xor(dot, 1);
    dot += __shfl_xor(dot, 2);
    dot += __shfl_xor(dot, 4);
    if (sub == 0) dot_s[row] = dot;
  }
  __syncthreads();
  const long long head_stride = (long long)N * hd;
  float* out = grad + bg * H * head_stride;
  for (int e = threadIdx.x; e < 32 * hd; e += 256) {
    const int row = e / hd, d = e % hd;
    if (i0 + row >= T) break;
    const long long t = i0 + row;
    const float nrm = norms[bg * T + t], g = g_s[row][d];
    const float ga = nrm > PSAQ_EPS ? (g - A[t * hd + d] * dot_s[row]) / nrm : g / PSAQ_EPS;
    const float v = ga / (float)H;
    for (int hh = 0; hh < H; ++hh) out[hh * head_stride + (t + 1) * hd + d] = v;
  }
  if (i0 == 0)                                                      // the dropped row of the group
    for (int e = threadIdx.x; e < H * hd; e += 256) out[(e / hd) * head_stride + e % hd] = 0.f;
}

// ---------------------------------------------------------------------------------------------------
// host launchers (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
static long long psaq_up(long long v) { return (v + 255) / 256 * 256; }

PsaqLayout p2v_psaq_layout(int B, int G, int N, int hd) {
  PsaqLayout w;
  const long long BG = (long long)B * G, T = N - 1, TT = (T + 31) / 32, n = (long long)G * T * T;
  w.sim_blocks = (int)((TT * (TT + 1) / 2 + 3) / 4);
  w.chunks = (int)((n + PSAQ_CHUNK - 1) / PSAQ_CHUNK);
  long long o = 0;
  w.sims = o;   o += psaq_up(BG * T * T * 4);
  w.ahat = o;   o += psaq_up(BG * T * hd * 4);
  w.norms = o;  o += psaq_up(BG * T * 4);
  w.mm = o;     o += psaq_up(BG * w.sim_blocks * 8);
  w.range = o;  o += 256;
  w.psums = o;  o += psaq_up((long long)B * w.chunks * PSAQ_POINTS * 8);
  w.coef = o;   o += psaq_up((long long)B * PSAQ_POINTS * 8);
  w.bytes = o;
  return w;
}

int p2v_launch_psaq(const PsaqArgs& a, void* ws, double* value, float* grad, hipStream_t st) {
  const PsaqLayout w = p2v_psaq_layout(a.B, a.G, a.N, a.hd);
  const long long BG = (long long)a.B * a.G, T = a.N - 1, TT = (T + 31) / 32, n = (long long)a.G * T * T;
  const long long row_blocks = (BG * T + 7) / 8, sim_blocks = BG * w.sim_blocks, den_blocks = (long long)a.B * w.chunks, grad_blocks = BG * TT;
  if (row_blocks >= (1LL << 31) || sim_blocks >= (1LL << 31) || den_blocks >= (1LL << 31) || grad_blocks >= (1LL << 31)) return -1;
  char* base = static_cast<char*>(ws);
  float* sims = reinterpret_cast<float*>(base + w.sims);
  float* ahat = reinterpret_cast<float*>(base + w.ahat);
  float* norms = reinterpret_cast<float*>(base + w.norms);
  float2* mm = reinterpret_cast<float2*>(base + w.mm);
  float* range = reinterpret_cast<float*>(base + w.range);
  double* psums = reinterpret_cast<double*>(base + w.psums);
  double* coef = reinterpret_cast<double*>(base + w.coef);
  hipLaunchKernelGGL(k_psaq_rows, dim3((unsigned)row_blocks), dim3(256), 0, st, a.av, BG * T, (int)T, a.H, a.N, a.hd, ahat, norms);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_psaq_sims, dim3((unsigned)sim_blocks), dim3(256), 0, st, ahat, (int)T, a.hd, w.sim_blocks, sims, mm);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_psaq_range, dim3(1), dim3(256), 0, st, mm, sim_blocks, range);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_psaq_density, dim3((unsigned)den_blocks), dim3(256), 0, st, sims, n, w.chunks, range, psums);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_psaq_finish, dim3(1), dim3(256), 0, st, psums, a.B, n, w.chunks, range, coef, value);
  CHECK_LAUNCH();
  const dim3 gg((unsigned)grad_blocks), gb(256);
  switch ((a.hd + 31) / 32) {
    case 1: hipLaunchKernelGGL(k_psaq_grad<1>, gg, gb, 0, st, sims, ahat, norms, range, coef, a.G, (int)T, a.H, a.N, a.hd, grad); break;
    case 2: hipLaunchKernelGGL(k_psaq_grad<2>, gg, gb, 0, st, sims, ahat, norms, range, coef, a.G, (int)T, a.H, a.N, a.hd, grad); break;
    case 3: hipLaunchKernelGGL(k_psaq_grad<3>, gg, gb, 0, st, sims, ahat, norms, range, coef, a.G, (int)T, a.H, a.N, a.hd, grad); break;
    default: hipLaunchKernelGGL(k_psaq_grad<4>, gg, gb, 0, st, sims, ahat, norms, range, coef, a.G, (int)T, a.H, a.N, a.hd, grad); break;
  }
  CHECK_LAUNCH();
  return 0;
}
