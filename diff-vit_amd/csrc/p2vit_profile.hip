// p2vit_profile.hip -- ModelDiff's search-based generation of profiling inputs (dataset_utility.py:193-302) as a device loop: the state
// of the search (logits tables, seed logits, pairwise distances, divergence terms, score) stays in one caller-allocated block, and an
// iteration costs a 2-image forward per model plus the three launches here; include/p2vit.h has the semantics and the state layout.
//
//   prof_dist           THE distance: one wave, sqrt(sum_k ((double)a_k - (double)b_k)^2).  Lane l owns the 4-element chunks l, l + 64, ..
//                       of the row in ascending order whatever the alignment of a and b (an aligned full chunk is one 16-byte load, any
//                       other chunk up to four scalar loads: the loads differ, the sum does not), then a butterfly (xor 32 .. 1; a + b ==
//                       b + a bit for bit, so every lane holds the same sum).  (a - b)^2 == (b - a)^2 bit for bit: dist(a, b) == dist(b, a).
//   k_prof_copy         logits -> O and O0 of one model (initialisation)
//   k_prof_pairs        one wave per (i, j): D[i][j] = dist(T_i, T_j), D[i][i] = 0; with T0 also g[i] = dist(T_i, T0_i)
//   k_prof_candidates   image idx of the inputs twice into the staging batch, element pos + eps / - eps (fp32 additions)
//   k_prof_rows         one wave per (model, candidate, j): rowd[j] = dist(candidate row, O_j), 0 at j == idx; j == n: rowg = dist(candidate
//                       row, O0_idx)
//   k_prof_decide       one workgroup of 512.  prof_sums adds the n^2 positions of D (row and column idx replaced by rowd: the sum runs
//                       over the positions AFTER the substitution) and the n entries of g (entry idx replaced): thread t takes positions
//                       t, t + 512, .. in ascending order, the partials go through the wave butterfly and a fixed chain over the 8 waves.
//                       Thread 0 forms the scores, applies the rule of dataset_utility.py:292-301 and writes the trace row; on acceptance
//                       all threads commit row / column idx of D, g[idx], the row of O, the input element and the score.
//                       MODE 0 (initialisation): no substitution, one "candidate", writes the score only.
// A candidate whose rows equal the current rows gives rowd[j] == D[idx][j] == D[j][idx] and rowg == g[idx] bit for bit (one function, one
// order), so its sums and its score equal the stored ones bit for bit: the reference's `<=` keeps the inputs.  No atomics anywhere.
#include "p2vit_device.h"

ProfLayout p2v_profile_layout(int n, int classes) {
  ProfLayout L;
  L.n = n; L.classes = classes;
  long long at = 2;                                          // double 0: the score; double 1: padding (never written)
  for (int m = 0; m < 2; ++m) {
    L.d[m] = at; at += (long long)n * n;
    L.g[m] = at; at += n;
    L.rowd[m] = at; at += 2LL * n;
    L.rowg[m] = at; at += 2;
  }
  at = (at + 1) & ~1LL;                                      // the fp32 tables start 16-byte aligned
  long long f = at * 2;
  for (int m = 0; m < 2; ++m) {
    L.o[m] = f; f += (long long)n * classes;
    L.o0[m] = f; f += (long long)n * classes;
  }
  L.bytes = (f * 4 + 15) & ~15LL;
  return L;
}

__device__ __forceinline__ double prof_dist(const float* __restrict__ a, const float* __restrict__ b, int classes, int lane) {
  double s = 0.0;
  const int nch = (classes + 3) >> 2;
  for (int c = lane; c < nch; c += 64) {
    const int k0 = 4 * c;
    float x[4], y[4];
    const bool full = k0 + 4 <= classes;
    if (full && (((uintptr_t)(a + k0)) & 15) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(a + k0);
      x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = k0 + e < classes ? a[k0 + e] : 0.f;
    }
    if (full && (((uintptr_t)(b + k0)) & 15) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(b + k0);
      y[0] = q.x; y[1] = q.y; y[2] = q.z; y[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = k0 + e < classes ? b[k0 + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {                            // a padded element adds (0 - 0)^2 = +0: s + 0 == s
      const double df = (double)x[e] - (double)y[e];
      s += df * df;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return sqrt(s);
}

__global__ __launch_bounds__(256) void k_prof_copy(const float* __restrict__ src, long long count, float* __restrict__ o, float* __restrict__ o0) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) {
    const float v = src[i];
    o[i] = v;
    if (o0) o0[i] = v;
  }
}

// tasks [0, n*n): (i, j); tasks [n*n, n*n + n) when t0: g[i]
__global__ __launch_bounds__(256) void k_prof_pairs(const float* __restrict__ t, const float* __restrict__ t0, long long ld, int n, int classes,
                                                    double* __restrict__ D, double* __restrict__ g) {
  const int lane = threadIdx.x & 63;
  const long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long nn = (long long)n * n;
  if (task < nn) {
    const int i = (int)(task / n), j = (int)(task % n);
    const double d = i == j ? 0.0 : prof_dist(t + i * ld, t + j * ld, classes, lane);
    if (lane == 0) D[task] = d;
  } else if (t0 && task < nn + n) {
    const int i = (int)(task - nn);
    const double d = prof_dist(t + i * ld, t0 + i * ld, classes, lane);
    if (lane == 0) g[i] = d;
  }
}

__global__ __launch_bounds__(256) void k_prof_candidates(const float* __restrict__ src, long long elems, long long pos, float eps,
                                                         float* __restrict__ staging) {
  const long long c0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (c0 >= elems) return;
  const bool full = c0 + 4 <= elems;
  float x[4];
  if (full && (((uintptr_t)(src + c0)) & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(src + c0);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = c0 + e < elems ? src[c0 + e] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = c0 + e == pos ? (c == 0 ? x[e] + eps : x[e] - eps) : x[e];
    float* dst = staging + c * elems + c0;
    if (full && (((uintptr_t)dst) & 15) == 0) {
      *reinterpret_cast<float4*>(dst) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < elems) dst[e] = y[e];
    }
  }
}

// task = (m * 2 + c) * (n + 1) + j
__global__ __launch_bounds__(256) void k_prof_rows(const ProfLayout L, unsigned char* __restrict__ state, const float* __restrict__ cand0,
                                                   const float* __restrict__ cand1, int idx) {
  const int lane = threadIdx.x & 63;
  const long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = L.n, per = n + 1;
  if (task >= 4LL * per) return;
  const int mc = (int)(task / per), j = (int)(task % per), m = mc >> 1, c = mc & 1;
  double* sd = reinterpret_cast<double*>(state);
  const float* sf = reinterpret_cast<const float*>(state);
  const float* row = (m ? cand1 : cand0) + (long long)c * L.classes;
  if (j < n) {
    const double d = j == idx ? 0.0 : prof_dist(row, sf + L.o[m] + (long long)j * L.classes, L.classes, lane);
    if (lane == 0) sd[L.rowd[m] + (long long)c * n + j] = d;
  } else {
    const double d = prof_dist(row, sf + L.o0[m] + (long long)idx * L.classes, L.classes, lane);
    if (lane == 0) sd[L.rowg[m] + c] = d;
  }
}

// the sum over the n^2 positions of D and over the n entries of g for NC candidates of one model, positions of row / column idx and
// entry idx replaced by the candidate's (idx < 0: none replaced).  Every thread returns the totals.
#define PROF_T 512      // threads of the one-workgroup kernels (256 VGPRs each: the two candidates' eight sums stay in registers)
template <int NC>
__device__ __forceinline__ void prof_sums(const double* __restrict__ D, const double* __restrict__ g, const double* __restrict__ rowd,
                                          const double* __restrict__ rowg, int n, int idx, double (*red)[PROF_T / 64], double* sumD, double* sumG) {
  const int t = threadIdx.x;
  double aD[NC], aG[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) aD[c] = aG[c] = 0.0;
  const long long nn = (long long)n * n;
  int i = t / n, j = t % n;                                  // position p = i * n + j, advanced by PROF_T without a division per step
  const int di = PROF_T / n, dj = PROF_T % n;
  #pragma unroll 2
  for (long long p = t; p < nn; p += PROF_T) {
    if (i == idx || j == idx) {
      const int o = i == idx ? j : i;
#pragma unroll
      for (int c = 0; c < NC; ++c) aD[c] += rowd[(long long)c * n + o];
    } else {
      const double v = D[p];
#pragma unroll
      for (int c = 0; c < NC; ++c) aD[c] += v;
    }
    i += di; j += dj;
    if (j >= n) { j -= n; ++i; }
  }
  for (int e = t; e < n; e += PROF_T) {
    if (e == idx) {
#pragma unroll
      for (int c = 0; c < NC; ++c) aG[c] += rowg[c];
    } else {
      const double v = g[e];
#pragma unroll
      for (int c = 0; c < NC; ++c) aG[c] += v;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      aD[c] += __shfl_xor(aD[c], off, 64);
      aG[c] += __shfl_xor(aG[c], off, 64);
    }
  }
  __syncthreads();                                           // the cells may still be read from the previous model
  if ((t & 63) == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) { red[c][t >> 6] = aD[c]; red[2 + c][t >> 6] = aG[c]; }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double sD = red[c][0], sG = red[2 + c][0];
    for (int w = 1; w < PROF_T / 64; ++w) { sD += red[c][w]; sG += red[2 + c][w]; }
    sumD[c] = sD; sumG[c] = sG;
  }
}

template <int MODE>      // 0: initialisation (score of the tables as they are), 1: one iteration's decision
__global__ __launch_bounds__(PROF_T) void k_prof_decide(const ProfLayout L, unsigned char* __restrict__ state, const float* __restrict__ cand0,
                                                      const float* __restrict__ cand1, const float* __restrict__ staging,
                                                      float* __restrict__ inputs, long long elems, int idx, long long pos,
                                                      double* __restrict__ trace) {
  __shared__ double red[4][PROF_T / 64];
  __shared__ int s_dec;
  constexpr int NC = MODE ? 2 : 1;
  const int t = threadIdx.x, n = L.n;
  double* sd = reinterpret_cast<double*>(state);
  float* sf = reinterpret_cast<float*>(state);
  double sumD[2][NC], sumG[2][NC];
#pragma unroll
  for (int m = 0; m < 2; ++m)
    prof_sums<NC>(sd + L.d[m], sd + L.g[m], sd + L.rowd[m], sd + L.rowg[m], n, MODE ? idx : -1, red, sumD[m], sumG[m]);
  const double nn = (double)n * (double)n;
  double sc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)                               // dist1 * dist2 * div1 * div2, in this order (dataset_utility.py:258)
    sc[c] = (sumG[0][c] / (double)n) * (sumG[1][c] / (double)n) * (sumD[0][c] / nn) * (sumD[1][c] / nn);
  if constexpr (MODE == 0) {
    if (t == 0) sd[0] = sc[0];
    return;
  } else {
    if (t == 0) {
      const double cur = sd[0], r = sc[0], l = sc[1];
      const int dec = (r <= cur && l <= cur) ? 0 : (r > l ? 1 : 2);      // dataset_utility.py:292-301
      s_dec = dec;
      const double now = dec == 0 ? cur : (dec == 1 ? r : l);
      trace[0] = r; trace[1] = l; trace[2] = (double)dec; trace[3] = now;
      if (dec) {
        sd[0] = now;
        inputs[(long long)idx * elems + pos] = staging[(long long)(dec - 1) * elems + pos];
      }
    }
    __syncthreads();
    const int dec = s_dec;
    if (dec == 0) return;
    const int c = dec - 1;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      double* D = sd + L.d[m];
      const double* rd = sd + L.rowd[m] + (long long)c * n;
      for (int j = t; j < n; j += PROF_T) {
        const double v = rd[j];                              // rd[idx] == 0
        D[(long long)idx * n + j] = v;
        D[(long long)j * n + idx] = v;
      }
      if (t == 0) sd[L.g[m] + idx] = sd[L.rowg[m] + c];
      const float* row = (m ? cand1 : cand0) + (long long)c * L.classes;
      float* o = sf + L.o[m] + (long long)idx * L.classes;
      for (int k = t; k < L.classes; k += PROF_T) o[k] = row[k];
    }
  }
}

__global__ __launch_bounds__(PROF_T) void k_prof_mean(const double* __restrict__ D, int n, double* __restrict__ out) {
  __shared__ double red[4][PROF_T / 64];
  double sD[1], sG[1];
  prof_sums<1>(D, D, D, D, n, -1, red, sD, sG);
  if (threadIdx.x == 0) *out = sD[0] / ((double)n * (double)n);
}

// ---------------------------------------------------------------------------------------------------
// host side (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
static unsigned prof_wave_blocks(long long tasks) { return (unsigned)((tasks + 3) / 4); }

int p2v_launch_profile_init(void* state, int n, int classes, const float* logits1, const float* logits2, hipStream_t st) {
  const ProfLayout L = p2v_profile_layout(n, classes);
  unsigned char* s = reinterpret_cast<unsigned char*>(state);
  double* sd = reinterpret_cast<double*>(state);
  float* sf = reinterpret_cast<float*>(state);
  const long long count = (long long)n * classes, nn = (long long)n * n;
  for (int m = 0; m < 2; ++m) {
    hipLaunchKernelGGL(k_prof_copy, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, m ? logits2 : logits1, count, sf + L.o[m],
                       sf + L.o0[m]);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(k_prof_pairs, dim3(prof_wave_blocks(nn + n)), dim3(256), 0, st, sf + L.o[m], sf + L.o0[m], (long long)classes, n,
                       classes, sd + L.d[m], sd + L.g[m]);
    CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_prof_decide<0>, dim3(1), dim3(PROF_T), 0, st, L, s, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                     (float*)nullptr, 0LL, -1, 0LL, (double*)nullptr);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_profile_candidates(const float* inputs, long long elems, int idx, long long pos, float eps, float* staging, hipStream_t st) {
  const long long chunks = (elems + 3) / 4;
  hipLaunchKernelGGL(k_prof_candidates, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, inputs + (long long)idx * elems, elems, pos,
                     eps, staging);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_profile_step(void* state, int n, int classes, const float* cand1, const float* cand2, const float* staging, float* inputs,
                            long long elems, int idx, long long pos, double* trace, hipStream_t st) {
  const ProfLayout L = p2v_profile_layout(n, classes);
  unsigned char* s = reinterpret_cast<unsigned char*>(state);
  hipLaunchKernelGGL(k_prof_rows, dim3(prof_wave_blocks(4LL * (n + 1))), dim3(256), 0, st, L, s, cand1, cand2, idx);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_prof_decide<1>, dim3(1), dim3(PROF_T), 0, st, L, s, cand1, cand2, staging, inputs, elems, idx, pos, trace);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_profile_diversity(const float* logits, long long ld, int n, int classes, double* ws, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_prof_pairs, dim3(prof_wave_blocks((long long)n * n)), dim3(256), 0, st, logits, (const float*)nullptr, ld, n, classes, ws,
                     (double*)nullptr);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_prof_mean, dim3(1), dim3(PROF_T), 0, st, ws, n, out);
  CHECK_LAUNCH();
  return 0;
}
