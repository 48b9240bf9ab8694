// p2vit_stats.hip -- stage statistics: which part of its code range a stage uses.  One strided plane (samples x rows x cols int8 codes,
// unsigned bytes or fp32 values) into one record (include/p2vit.h, p2v_code_stats): int64 hist[256], count, nonfinite[3], then per column
// lo / hi (int32, or the fp32 value) and, for the integer kinds, int64 sum / sumsq.  Every quantity is an integer or an order-independent
// extremum, so the record is defined exactly and integer atomics give the same bits whatever the grid.
//
//   k_stats<KIND>   one workgroup per (row range, column tile of 1024).  The plane is ONE list of samples * rows rows; a thread owns one
//                   16-byte column group (16 bytes or 4 floats) of the tile and walks the rows of its row lane, so the loads of a wave are
//                   contiguous along a row.  Per lane in registers: lo / hi / sum / sumsq of its columns (int32: a workgroup visits at most
//                   2^16 rows, |sum| <= 2^16 * 255 and sumsq <= 2^16 * 255^2 < 2^32 unsigned).  The histogram is private to a wave in LDS
//                   (uint32 bins, at most 2^16 * 1024 elements per workgroup).  After the walk the lanes of a column meet in LDS
//                   (ds_min / ds_max / ds_add_u64), then one global integer atomic per column and quantity and per non-empty bin.
//                   fp32 extrema run on the sign-magnitude key (an int32 whose order is the total order, -0 < +0) and reach the record,
//                   which holds the VALUE, through the sign-dependent pair signed min / unsigned max (and the mirror for hi).
//   k_stats_init    the empty record.
// Chosen against the partial-slot + combine form of p2vit_ddv.hip: a record has 256 + 4 * cols quantities where a cosine has 3, so slots
// would cost (256 + 4 * cols) * 8 bytes per workgroup and a second launch per stage; with at least 64 KB read per workgroup the atomics
// are a few percent of the traffic.
#include "p2vit_device.h"

#define ST_TILE 1024

// fp32 bits <-> the int32 key whose signed order is the total order of the values (an involution)
__device__ __forceinline__ int st_key(unsigned b) { return (int)(b ^ ((unsigned)((int)b >> 31) & 0x7fffffffu)); }

struct StatsRec {
  unsigned long long *hist, *count, *nonfinite, *sum, *sumsq;
  int *lo, *hi;
};
__device__ __forceinline__ StatsRec st_rec(void* rec, int cols) {
  StatsRec r;
  r.hist = reinterpret_cast<unsigned long long*>(rec);
  r.count = r.hist + 256;
  r.nonfinite = r.hist + 257;
  r.lo = reinterpret_cast<int*>(r.hist + 260);
  r.hi = r.lo + cols;
  r.sum = r.hist + 260 + cols;
  r.sumsq = r.sum + cols;
  return r;
}

template <int KIND, bool FULL>
__device__ __forceinline__ void st_walk(const StatsDesc& d, long long f0, long long f1, int lanes, int rl, int c0, int valid,
                                        unsigned* __restrict__ myh, int (&lo)[16], int (&hi)[16], int (&sm)[16], unsigned (&sq)[16],
                                        unsigned (&nf)[3]) {
  constexpr int PER = KIND == P2V_STAT_F32 ? 4 : 16;
  for (long long f = f0 + rl; f < f1; f += lanes) {
    const unsigned s = (unsigned)f / (unsigned)d.rows, r = (unsigned)f - s * (unsigned)d.rows;
    const long long o = (long long)s * d.sample_stride + (long long)r * d.row_stride + c0;
    if constexpr (KIND == P2V_STAT_F32) {
      const float* p = reinterpret_cast<const float*>(d.base) + o;
      unsigned b[4];
      if (FULL && d.vec) {
        const v4i v = *reinterpret_cast<const v4i*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = (unsigned)v[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = (FULL || j < valid) ? __float_as_uint(p[j]) : 0u;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (FULL || j < valid) {
          const unsigned e = (b[j] >> 23) & 255u;
          atomicAdd(&myh[e], 1u);
          if (e == 255u) {
            ++nf[(b[j] & 0x7fffffu) ? 0 : ((b[j] >> 31) ? 2 : 1)];
          } else {
            const int k = st_key(b[j]);
            lo[j] = min(lo[j], k);
            hi[j] = max(hi[j], k);
          }
        }
    } else {
      const uint8_t* p = reinterpret_cast<const uint8_t*>(d.base) + o;
      v4i v = {0, 0, 0, 0};
      if (FULL && d.vec) {
        v = *reinterpret_cast<const v4i*>(p);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (FULL || j < valid) v[j >> 2] |= (int)((unsigned)p[j] << (8 * (j & 3)));
      }
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (FULL || j < valid) {
          const int x = KIND == P2V_STAT_I8 ? (int)(int8_t)(v[j >> 2] >> (8 * (j & 3))) : (int)(((unsigned)v[j >> 2] >> (8 * (j & 3))) & 255u);
          atomicAdd(&myh[KIND == P2V_STAT_I8 ? x + 128 : x], 1u);
          lo[j] = min(lo[j], x);
          hi[j] = max(hi[j], x);
          sm[j] += x;
          sq[j] += (unsigned)(x * x);
        }
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_stats(const StatsDesc d) {
  constexpr int PER = KIND == P2V_STAT_F32 ? 4 : 16;
  constexpr bool INTK = KIND != P2V_STAT_F32;
  __shared__ unsigned s_hist[4][256];
  __shared__ int s_lo[ST_TILE], s_hi[ST_TILE];
  __shared__ unsigned long long s_sum[INTK ? ST_TILE : 1], s_sq[INTK ? ST_TILE : 1];
  __shared__ unsigned s_nf[3];
  const int t = threadIdx.x;
  const int tile = blockIdx.x % d.tiles, split = blockIdx.x / d.tiles;
  const int cb = tile * ST_TILE, tcols = min(ST_TILE, d.cols - cb);
  const long long f0 = (long long)split * d.rows_per_split, f1 = min(d.flat_rows, f0 + d.rows_per_split);
  for (int i = t; i < 4 * 256; i += 256) (&s_hist[0][0])[i] = 0u;
  for (int c = t; c < tcols; c += 256) {
    s_lo[c] = 0x7fffffff;
    s_hi[c] = (int)0x80000000;
    if (INTK) { s_sum[c] = 0ull; s_sq[c] = 0ull; }
  }
  if (t < 3) s_nf[t] = 0u;
  __syncthreads();

  const int ncg = (tcols + PER - 1) / PER;        // <= 256 (fp32) / 64 (bytes): every thread has one column group
  const int lanes = 256 / ncg, cgl = t % ncg, rl = t / ncg;
  if (rl < lanes && f0 + rl < f1) {
    const int c0 = cb + cgl * PER, valid = min(PER, d.cols - c0);
    int lo[16], hi[16], sm[16];
    unsigned sq[16], nf[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) { lo[j] = 0x7fffffff; hi[j] = (int)0x80000000; sm[j] = 0; sq[j] = 0u; }
    if (valid == PER) st_walk<KIND, true>(d, f0, f1, lanes, rl, c0, valid, s_hist[t >> 6], lo, hi, sm, sq, nf);
    else st_walk<KIND, false>(d, f0, f1, lanes, rl, c0, valid, s_hist[t >> 6], lo, hi, sm, sq, nf);
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (j < valid) {
        const int c = cgl * PER + j;
        atomicMin(&s_lo[c], lo[j]);
        atomicMax(&s_hi[c], hi[j]);
        if (INTK) {
          atomicAdd(&s_sum[c], (unsigned long long)(long long)sm[j]);
          atomicAdd(&s_sq[c], (unsigned long long)sq[j]);
        }
      }
    if (!INTK) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (nf[q]) atomicAdd(&s_nf[q], nf[q]);
    }
  }
  __syncthreads();

  const StatsRec R = st_rec(d.rec, d.cols);
  {
    const unsigned h = s_hist[0][t] + s_hist[1][t] + s_hist[2][t] + s_hist[3][t];
    if (h) atomicAdd(&R.hist[t], (unsigned long long)h);
  }
  if (t == 0 && tile == 0) atomicAdd(R.count, (unsigned long long)(f1 - f0) * (unsigned long long)d.cols);
  if (!INTK && t < 3 && s_nf[t]) atomicAdd(&R.nonfinite[t], (unsigned long long)s_nf[t]);
  for (int c = t; c < tcols; c += 256) {
    const int l = s_lo[c], h = s_hi[c];
    if (l > h) continue;                           // no (finite) element of this column in the workgroup's rows
    if (INTK) {
      atomicMin(&R.lo[cb + c], l);
      atomicMax(&R.hi[cb + c], h);
      atomicAdd(&R.sum[cb + c], s_sum[c]);
      atomicAdd(&R.sumsq[cb + c], s_sq[c]);
    } else {
      // the record holds fp32 bits: values without the sign bit order like signed ints, values with it in reverse like unsigned ints
      const unsigned bl = (unsigned)st_key((unsigned)l), bh = (unsigned)st_key((unsigned)h);
      if (bl >> 31) atomicMax(reinterpret_cast<unsigned*>(&R.lo[cb + c]), bl); else atomicMin(&R.lo[cb + c], (int)bl);
      if (bh >> 31) atomicMin(reinterpret_cast<unsigned*>(&R.hi[cb + c]), bh); else atomicMax(&R.hi[cb + c], (int)bh);
    }
  }
}

__global__ __launch_bounds__(256) void k_stats_init(unsigned* __restrict__ rec, int words, int kind, int cols) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= words) return;
  const int c = i - 2 * 260;                       // lo / hi start behind 260 int64
  unsigned v = 0u;
  if (c >= 0 && c < cols) v = kind == P2V_STAT_F32 ? 0x7f800000u : 0x7fffffffu;
  else if (c >= cols && c < 2 * cols) v = kind == P2V_STAT_F32 ? 0xff800000u : 0x80000000u;
  rec[i] = v;
}

// ---------------------------------------------------------------------------------------------------
// host side (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
// The row ranges: ~64 KB of the tile per workgroup, at most ~2048 workgroups per stage, at most 2^16 rows per workgroup (the 32-bit
// registers and bins above).  The record does not depend on it.  (Measured against ~16 KB and up to 4096 workgroups: the stage shapes of
// DeiT-S and Swin-B of 6 MB and more took 1.3 - 2.3 times as long - a workgroup's fixed part, the 28 KB of LDS it clears and its 256 + 4 * cols
// global atomics, weighs more than the occupancy gained; profiles/stage_stats.txt.)
StatsDesc p2v_stats_desc(const p2v_stat_layer& l, void* rec) {
  StatsDesc d;
  d.base = l.base; d.rec = rec;
  d.sample_stride = l.sample_stride; d.row_stride = l.row_stride;
  d.flat_rows = (long long)l.samples * l.rows;
  d.rows = l.rows; d.cols = l.cols; d.kind = l.dtype;
  const long long esz = l.dtype == P2V_STAT_F32 ? 4 : 1;
  d.vec = ((uintptr_t)l.base % 16 == 0 && l.sample_stride * esz % 16 == 0 && l.row_stride * esz % 16 == 0) ? 1 : 0;
  d.tiles = (l.cols + ST_TILE - 1) / ST_TILE;
  const long long row_bytes = (long long)(l.cols < ST_TILE ? l.cols : ST_TILE) * esz;
  long long ns = (d.flat_rows * row_bytes + 65535) / 65536;
  const long long cap = d.tiles >= 2048 ? 1 : 2048 / d.tiles;
  if (ns > cap) ns = cap;
  if (ns > d.flat_rows) ns = d.flat_rows;
  const long long min_ns = (d.flat_rows + 65535) / 65536;
  if (ns < min_ns) ns = min_ns;
  if (ns < 1) ns = 1;
  d.rows_per_split = (int)((d.flat_rows + ns - 1) / ns);
  d.nsplit = d.rows_per_split ? (int)((d.flat_rows + d.rows_per_split - 1) / d.rows_per_split) : 0;
  return d;
}

// the instantiations the library can select: one per element kind, indexed by P2V_STAT_*
typedef void (*StatsKernel)(const StatsDesc);
static const StatsKernel k_stats_table[3] = {k_stats<P2V_STAT_I8>, k_stats<P2V_STAT_F32>, k_stats<P2V_STAT_U8>};

int p2v_launch_stats(const StatsDesc& d, hipStream_t st) {
  if (d.flat_rows <= 0) return 0;
  if (d.kind < 0 || d.kind > 2 || d.flat_rows >= (1LL << 31) || (long long)d.tiles * d.nsplit >= (1LL << 31)) return -1;
  hipLaunchKernelGGL(k_stats_table[d.kind], dim3((unsigned)(d.tiles * d.nsplit)), dim3(256), 0, st, d);
  CHECK_LAUNCH();
  return 0;
}

int p2v_launch_stats_init(void* rec, size_t bytes, int kind, int cols, hipStream_t st) {
  const int words = (int)(bytes / 4);
  hipLaunchKernelGGL(k_stats_init, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, reinterpret_cast<unsigned*>(rec), words, kind, cols);
  CHECK_LAUNCH();
  return 0;
}
