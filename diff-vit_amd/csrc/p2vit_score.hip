// p2vit_score.hip -- scoring of the logits on the device: tie-aware ranks and the fp64 cross-entropy per row (p2v_score_logits), folded
// into running totals that stay in device memory (p2v_score_accumulate); include/p2vit.h has the record and totals layouts.
//
//   k_score_rows        one wave per row, four rows per workgroup.  x_y = logits[r][label] is loaded first, uniformly across the wave.
//                       Pass 1: per lane the maximum with its lowest index and the three counts against x_y; a lane walks an aligned row in
//                       float4 pieces (scalar head and tail where the row base is not 16-byte aligned), always in ascending j.  The wave
//                       reduces over a butterfly (xor 32, 16, .. 1).  Pass 2: sum_j exp((double)x_j - m) per lane in ascending j, the same
//                       butterfly in fp64 (a + b == b + a bit for bit, so every lane holds the same sum), then log(sum) + m - x_y.
//                       A label outside [0, classes) is never used as an index: gt = -1, eq_lo = eq_hi = 0, loss = 0, the real argmax.
//                       Columns [classes, ld) are never read.
//   k_score_accumulate  one workgroup.  Thread t takes records t, t + 256, .. in ascending order: integer counters per k, and the losses
//                       in fp64.  The counters go through wave butterflies and four LDS cells each (integer sums: any order is exact), the
//                       256 loss partials through a fixed LDS tree; one thread per value then adds to the slot.
// No atomics: every result is bitwise repeatable.
#include "p2vit_device.h"

#define SCORE_MAX_K 8

struct ScoreKs {
  int n_k;
  int k[SCORE_MAX_K];
};

struct ScoreLane {
  float mx;
  int am, gt, lo, hi;
};

__device__ __forceinline__ void score_take(ScoreLane& s, float x, int j, float xy, int y, bool valid) {
  if (x > s.mx || s.am < 0) { s.mx = x; s.am = j; }       // ascending j within a lane: the first maximum stays
  if (valid) {
    s.gt += x > xy;
    s.lo += (x == xy) & (j < y);
    s.hi += (x == xy) & (j > y);
  }
}

__global__ __launch_bounds__(256) void k_score_rows(const float* __restrict__ logits, long long ld, int rows, int classes,
                                                    const long long* __restrict__ labels, int* __restrict__ ranks, double* __restrict__ loss) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                   // whole waves leave: no barrier in this kernel
  const float* __restrict__ x = logits + r * ld;
  const long long yl = labels[r];
  const bool valid = yl >= 0 && yl < classes;
  const int y = valid ? (int)yl : 0;
  const float xy = valid ? x[y] : 0.f;
  // [0, head) scalar, nvec float4 pieces from the first 16-byte boundary, [tail0, classes) scalar
  const int head = min(classes, (int)((4 - (((uintptr_t)x >> 2) & 3)) & 3));
  const int nvec = (classes - head) >> 2;
  const int tail0 = head + 4 * nvec;
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + head);

  ScoreLane s = {0.f, -1, 0, 0, 0};
  if (lane < head) score_take(s, x[lane], lane, xy, y, valid);
  for (int v = lane; v < nvec; v += 64) {
    const float4 q = xv[v];
    const int j = head + 4 * v;
    score_take(s, q.x, j, xy, y, valid);
    score_take(s, q.y, j + 1, xy, y, valid);
    score_take(s, q.z, j + 2, xy, y, valid);
    score_take(s, q.w, j + 3, xy, y, valid);
  }
  if (tail0 + lane < classes) score_take(s, x[tail0 + lane], tail0 + lane, xy, y, valid);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float omx = __shfl_xor(s.mx, off, 64);
    const int oam = __shfl_xor(s.am, off, 64);
    if (oam >= 0 && (s.am < 0 || omx > s.mx || (omx == s.mx && oam < s.am))) { s.mx = omx; s.am = oam; }
    s.gt += __shfl_xor(s.gt, off, 64);
    s.lo += __shfl_xor(s.lo, off, 64);
    s.hi += __shfl_xor(s.hi, off, 64);
  }
  double l = 0.0;
  if (valid) {
    const double m = (double)s.mx;
    double e = 0.0;
    if (lane < head) e += exp((double)x[lane] - m);
    for (int v = lane; v < nvec; v += 64) {
      const float4 q = xv[v];
      e += exp((double)q.x - m);
      e += exp((double)q.y - m);
      e += exp((double)q.z - m);
      e += exp((double)q.w - m);
    }
    if (tail0 + lane < classes) e += exp((double)x[tail0 + lane] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off, 64);
    l = log(e) + m - (double)xy;
  }
  if (lane < 4) ranks[r * 4 + lane] = lane == 0 ? (valid ? s.gt : -1) : (lane == 1 ? s.lo : (lane == 2 ? s.hi : s.am));
  if (lane == 0) loss[r] = l;
}

// totals slot: int64 n, invalid, hit[n_k], sure[n_k], possible[n_k]; double loss_sum
__global__ __launch_bounds__(256) void k_score_accumulate(const int* __restrict__ ranks, const double* __restrict__ loss, int rows,
                                                          const ScoreKs ks, long long* __restrict__ totals) {
  __shared__ double red[256];
  __shared__ int cnt[2 + 3 * SCORE_MAX_K][4];
  const int t = threadIdx.x, nk = ks.n_k;
  int n = 0, inv = 0, hit[SCORE_MAX_K], sure[SCORE_MAX_K], poss[SCORE_MAX_K];
#pragma unroll
  for (int q = 0; q < SCORE_MAX_K; ++q) hit[q] = sure[q] = poss[q] = 0;
  double ls = 0.0;
  for (int r = t; r < rows; r += 256) {                     // at most 2^23 records per thread: the int32 counters hold them
    const int gt = ranks[4 * (long long)r], lo = ranks[4 * (long long)r + 1], hi = ranks[4 * (long long)r + 2];
    if (gt < 0) { ++inv; continue; }
    ++n;
    ls += loss[r];
#pragma unroll
    for (int q = 0; q < SCORE_MAX_K; ++q)
      if (q < nk) {
        hit[q] += gt + lo < ks.k[q];
        sure[q] += gt + lo + hi < ks.k[q];
        poss[q] += gt < ks.k[q];
      }
  }
  red[t] = ls;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n += __shfl_xor(n, off, 64);
    inv += __shfl_xor(inv, off, 64);
#pragma unroll
    for (int q = 0; q < SCORE_MAX_K; ++q) {
      hit[q] += __shfl_xor(hit[q], off, 64);
      sure[q] += __shfl_xor(sure[q], off, 64);
      poss[q] += __shfl_xor(poss[q], off, 64);
    }
  }
  if ((t & 63) == 0) {
    const int w = t >> 6;
    cnt[0][w] = n; cnt[1][w] = inv;
#pragma unroll
    for (int q = 0; q < SCORE_MAX_K; ++q) {
      cnt[2 + q][w] = hit[q]; cnt[2 + SCORE_MAX_K + q][w] = sure[q]; cnt[2 + 2 * SCORE_MAX_K + q][w] = poss[q];
    }
  }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t < 2 + 3 * nk) {                                     // slot cell t <- counter row c of the LDS table
    const int c = t < 2 ? t : 2 + ((t - 2) / nk) * SCORE_MAX_K + (t - 2) % nk;
    totals[t] += (long long)cnt[c][0] + cnt[c][1] + cnt[c][2] + cnt[c][3];
  }
  if (t == 255) {
    double* ps = reinterpret_cast<double*>(totals + 2 + 3 * nk);
    *ps = *ps + red[0];
  }
}

// ---------------------------------------------------------------------------------------------------
// host side (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
int p2v_launch_score_rows(const float* logits, long long ld, int rows, int classes, const long long* labels, int* ranks, double* loss,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_score_rows, dim3((unsigned)(((long long)rows + 3) / 4)), dim3(256), 0, st, logits, ld, rows, classes, labels, ranks, loss);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_score_accumulate(const int* ranks, const double* loss, int rows, const int* ks, int n_k, void* totals, hipStream_t st) {
  ScoreKs k;
  k.n_k = n_k;
  for (int q = 0; q < SCORE_MAX_K; ++q) k.k[q] = q < n_k ? ks[q] : 1;
  hipLaunchKernelGGL(k_score_accumulate, dim3(1), dim3(256), 0, st, ranks, loss, rows, k, reinterpret_cast<long long*>(totals));
  CHECK_LAUNCH();
  return 0;
}
