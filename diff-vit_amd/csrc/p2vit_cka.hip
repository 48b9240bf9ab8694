// p2vit_cka.hip -- the CKA model diff on the device (efficient_CKA.MinibatchCKA, DDV_CKA.MinibatchAdvCKA): grouped Gram matrices of
// many layers in one pass, their centring, and the HSIC inner products of the accumulators (p2v_cka_grams / p2v_hsic_accumulate,
// include/p2vit.h).
//
// Gram G = X Y^T of n <= 256 rows and F features (up to ~605 k for a ViT-B fc1 tap): tall and skinny, so the contraction is split.
//   k_cka_partial   one workgroup per (layer, chunk of 4096 features, 32x32 output tile); for X X^T only tiles ti <= tj.  Four waves
//                   take a quarter of the chunk each and run v_mfma_f32_32x32x2_f32 (exact fp32 products, an fmaf chain) over it with four
//                   independent accumulators (128 dependent steps each); the 16 partial sums of an output are added in fp64 in a fixed
//                   order and stored as fp32 [chunk][tile][32][32]
//   k_cka_reduce    one thread per gram entry: the chunk partials in chunk order, fp64
//   k_cka_centre    one workgroup per layer: zero diagonal, column means / (n-2), mean correction, subtract, zero diagonal (fp64)
// Nothing is accumulated with atomics, so every result is bitwise repeatable; the chunking depends on (n, F) only.
#include "p2vit_device.h"

typedef float v16f __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int cka_find_layer(const CkaDesc* d, int L, long long item) {
  int lo = 0, hi = L - 1;                     // last layer whose first item is <= item
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].item0 <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// tile index -> (ti, tj); sym: upper triangle row by row
__device__ __forceinline__ void cka_tile_of(int t, int T, bool sym, int& ti, int& tj) {
  if (!sym) { ti = t / T; tj = t % T; return; }
  ti = 0;
  while (t >= T - ti) { t -= T - ti; ++ti; }
  tj = ti + t;
}

// 32 features of one row for this lane: f + 8u + 4h + {0..3}, u = 0..3 (zeros outside [0, F) and for rows >= n)
__device__ __forceinline__ void cka_load(const float* row, long long f, long long F, int h, bool vec, float4 (&v)[4]) {
  if (!row) {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (vec && f + 32 <= F) {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(row + f + 8 * u + 4 * h);
    return;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long b = f + 8 * u + 4 * h;
    v[u].x = b + 0 < F ? row[b + 0] : 0.f;
    v[u].y = b + 1 < F ? row[b + 1] : 0.f;
    v[u].z = b + 2 < F ? row[b + 2] : 0.f;
    v[u].w = b + 3 < F ? row[b + 3] : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_cka_partial(const CkaDesc* __restrict__ descs, int L, int n, float* __restrict__ partials) {
  __shared__ double red[4][1024];
  const int l = cka_find_layer(descs, L, blockIdx.x);
  const CkaDesc d = descs[l];
  const int T = (n + 31) / 32;
  const int ntiles = d.sym ? T * (T + 1) / 2 : T * T;
  const long long local = (long long)blockIdx.x - d.item0;
  const int tile = (int)(local % ntiles), chunk = (int)(local / ntiles);   // the tiles of one chunk run side by side (shared rows in L2)
  int ti, tj;
  cka_tile_of(tile, T, d.sym != 0, ti, tj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int i = ti * 32 + r, j = tj * 32 + r;
  const float* xr = i < n ? d.x + (long long)i * d.ldx : nullptr;
  const float* yr = j < n ? d.y + (long long)j * d.ldy : nullptr;
  const bool vec = d.vec != 0;
  const long long f0 = (long long)chunk * P2V_CKA_CHUNK + wave * (P2V_CKA_CHUNK / 4);
  v16f acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[u][q] = 0.f;
  for (int s = 0; s < P2V_CKA_CHUNK / 4 / 32; ++s) {
    const long long f = f0 + 32 * s;
    if (f >= d.F) break;                                           // wave-uniform
    float4 xv[4], yv[4];
    cka_load(xr, f, d.F, h, vec, xv);
    cka_load(yr, f, d.F, h, vec, yv);
    // lane (r, h) supplies A[i=r][k=h] = x[i][.] and B[k=h][j=r] = y[j][.] of the same feature: D[i][j] += x_i . y_j
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].x, yv[u].x, acc[u], 0, 0, 0);
      acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].y, yv[u].y, acc[u], 0, 0, 0);
      acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].z, yv[u].z, acc[u], 0, 0, 0);
      acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u].w, yv[u].w, acc[u], 0, 0, 0);
    }
  }
  // C/D map of the 32x32 MFMA: register q of lane -> row (q & 3) + 8 (q >> 2) + 4 h, column r
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
    red[wave][row * 32 + r] = (((double)acc[0][q] + (double)acc[1][q]) + (double)acc[2][q]) + (double)acc[3][q];
  }
  __syncthreads();
  float* out = partials + d.part0 + ((long long)chunk * ntiles + tile) * 1024;
  for (int e = threadIdx.x; e < 1024; e += 256)
    out[e] = (float)(((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]);
}

__global__ __launch_bounds__(256) void k_cka_reduce(const CkaDesc* __restrict__ descs, int n, const float* __restrict__ partials,
                                                    double* __restrict__ g64, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long nn = (long long)n * n;
  const int l = (int)(idx / nn);
  const int i = (int)((idx % nn) / n), j = (int)(idx % n);
  const CkaDesc d = descs[l];
  double s = 0.0;
  if (i != j) {
    int a = i, b = j;
    if (d.sym && a > b) { a = j; b = i; }                          // X X^T: the mirror entry of the upper triangle (exact symmetry)
    const int T = (n + 31) / 32, ti = a >> 5, tj = b >> 5;
    const int ntiles = d.sym ? T * (T + 1) / 2 : T * T;
    const int tile = d.sym ? ti * T - ti * (ti - 1) / 2 + (tj - ti) : ti * T + tj;
    const float* p = partials + d.part0 + (long long)tile * 1024 + (a & 31) * 32 + (b & 31);
    const long long step = (long long)ntiles * 1024;
    for (int c = 0; c < d.nchunks; ++c) s += (double)p[c * step];
  }
  g64[idx] = s;                                                    // gram.diagonal().fill_(0)
}

__global__ __launch_bounds__(256) void k_cka_centre(int n, const double* __restrict__ g64, float* __restrict__ grams) {
  __shared__ double means[P2V_CKA_MAX_N];
  __shared__ double corr;
  const long long nn = (long long)n * n;
  const double* G = g64 + blockIdx.x * nn;
  float* out = grams + blockIdx.x * nn;
  const int t = threadIdx.x;
  if (t < n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += G[(long long)i * n + t];     // gram.sum(0)
    means[t] = s / (double)(n - 2);
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += means[k];
    corr = s / (double)(2 * (n - 1));
  }
  __syncthreads();
  if (t < n) means[t] -= corr;
  __syncthreads();
  for (long long e = t; e < nn; e += 256) {
    const int i = (int)(e / n), j = (int)(e % n);
    out[e] = i == j ? 0.f : (float)((G[e] - means[j]) - means[i]);
  }
}

// <a, b> over nn floats in fp64, fixed order; one workgroup per output
template <typename T>
__global__ __launch_bounds__(256) void k_hsic(const float* __restrict__ g1, int l1, const float* __restrict__ g2, int l2, long long nn,
                                              T* __restrict__ acc, T* __restrict__ self1, T* __restrict__ self2) {
  __shared__ double red[256];
  int b = blockIdx.x;
  const float *pa, *pb;
  T* dst;
  if (b < l1 * l2) {
    pa = g1 + (long long)(b / l2) * nn; pb = g2 + (long long)(b % l2) * nn; dst = acc + b;
  } else if ((b -= l1 * l2) < (self1 ? l1 : 0)) {
    pa = pb = g1 + (long long)b * nn; dst = self1 + b;
  } else {
    b -= self1 ? l1 : 0;
    pa = pb = g2 + (long long)b * nn; dst = self2 + b;
  }
  double s = 0.0;
  for (long long e = threadIdx.x; e < nn; e += 256) s += (double)pa[e] * (double)pb[e];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dst = (T)((double)*dst + red[0]);
}

// ---------------------------------------------------------------------------------------------------
// host launchers (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
CkaLayout p2v_cka_layout(const p2v_cka_layer* layers, int L, int n, std::vector<CkaDesc>* descs) {
  CkaLayout w;
  const int T = (n + 31) / 32;
  long long items = 0, parts = 0;
  for (int l = 0; l < L; ++l) {
    const p2v_cka_layer& a = layers[l];
    CkaDesc d;
    d.x = a.x;
    d.sym = (a.y == nullptr || a.y == a.x) ? 1 : 0;
    d.y = d.sym ? a.x : a.y;
    d.F = a.features;
    d.ldx = a.ldx;
    d.ldy = d.sym ? a.ldx : a.ldy;
    d.nchunks = (int)((a.features + P2V_CKA_CHUNK - 1) / P2V_CKA_CHUNK);
    const int ntiles = d.sym ? T * (T + 1) / 2 : T * T;
    d.vec = ((uintptr_t)d.x % 16 == 0 && (uintptr_t)d.y % 16 == 0 && d.ldx % 4 == 0 && d.ldy % 4 == 0) ? 1 : 0;
    d.item0 = items;
    d.part0 = parts;
    items += (long long)ntiles * d.nchunks;
    parts += (long long)ntiles * d.nchunks * 1024;
    if (descs) descs->push_back(d);
  }
  w.items = items;
  w.desc_off = 0;
  w.part_off = ((size_t)L * sizeof(CkaDesc) + 255) / 256 * 256;
  w.g64_off = w.part_off + ((size_t)parts * sizeof(float) + 255) / 256 * 256;
  w.total = w.g64_off + (size_t)L * n * n * sizeof(double);
  return w;
}

int p2v_launch_cka_grams(const std::vector<CkaDesc>& descs, const CkaLayout& w, int n, float* grams, void* ws, hipStream_t st) {
  const int L = (int)descs.size();
  char* base = reinterpret_cast<char*>(ws);
  CkaDesc* dd = reinterpret_cast<CkaDesc*>(base + w.desc_off);
  float* parts = reinterpret_cast<float*>(base + w.part_off);
  double* g64 = reinterpret_cast<double*>(base + w.g64_off);
  if (w.items >= (1LL << 31)) return -1;
  // pageable source on a stream that is NOT capturing (p2v_cka_grams refuses a capturing one): the runtime stages it before returning, so
  // the host vector may go away afterwards.  Recorded into a graph the copy node would keep the host pointer: replays would read freed memory
  hipError_t e = hipMemcpyAsync(dd, descs.data(), descs.size() * sizeof(CkaDesc), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_cka_partial, dim3((unsigned)w.items), dim3(256), 0, st, dd, L, n, parts);
  CHECK_LAUNCH();
  const long long total = (long long)L * n * n;
  hipLaunchKernelGGL(k_cka_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dd, n, parts, g64, total);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cka_centre, dim3((unsigned)L), dim3(256), 0, st, n, g64, grams);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_cka_raw(const CkaDesc& desc, const CkaLayout& w, int n, double* g64, void* ws, hipStream_t st) {
  char* base = reinterpret_cast<char*>(ws);
  CkaDesc* dd = reinterpret_cast<CkaDesc*>(base + w.desc_off);
  float* parts = reinterpret_cast<float*>(base + w.part_off);
  if (w.items >= (1LL << 31)) return -1;
  hipError_t e = hipMemcpyAsync(dd, &desc, sizeof(CkaDesc), hipMemcpyHostToDevice, st);      // (pageable source, eager stream only: staged before the
                                                                                             // call returns; p2v_code_grams / p2v_forward_grams refuse a capturing stream)
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_cka_partial, dim3((unsigned)w.items), dim3(256), 0, st, dd, 1, n, parts);
  CHECK_LAUNCH();
  const long long total = (long long)n * n;
  hipLaunchKernelGGL(k_cka_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dd, n, parts, g64, total);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_hsic(const float* g1, int l1, const float* g2, int l2, int n, void* acc, void* self1, void* self2, int dtype, hipStream_t st) {
  const unsigned blocks = (unsigned)(l1 * l2 + (self1 ? l1 : 0) + (self2 ? l2 : 0));
  const long long nn = (long long)n * n;
  if (dtype == 1)
    hipLaunchKernelGGL(k_hsic<double>, dim3(blocks), dim3(256), 0, st, g1, l1, g2, l2, nn, (double*)acc, (double*)self1, (double*)self2);
  else
    hipLaunchKernelGGL(k_hsic<float>, dim3(blocks), dim3(256), 0, st, g1, l1, g2, l2, nn, (float*)acc, (float*)self1, (float*)self2);
  CHECK_LAUNCH();
  return 0;
}
