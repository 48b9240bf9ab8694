// p2vit_ddv.hip -- the DDV model diff on the device (modeldiff_p2.compute_ddv:84-116): grouped pair-cosine sums.  For every (stage,
// sample) the three numbers a cosine needs, sum a.b, sum a.a, sum b.b over the sample's rows x cols elements (p2v_pair_cosine /
// p2v_forward_ddv, include/p2vit.h).
//
//   k_cos_partial   one workgroup per (stage, sample, split of the sample's rows).  A thread owns one 16-byte column group (16 int8 codes
//                   or 4 floats) and walks the rows of its row lane, so the loads of a wave are contiguous along a row.
//                     int8, no scale     v_dot4_i32_i8 on the dwords of the two loads; the per-load int32 (<= 16 * 2^14) goes into int64
//                     int8, scale[cols]  per-channel int32 sums over the thread's rows (<= 2^16 rows * 2^14: the splitting guarantees it),
//                                        then sum_c (double)s_c * (double)s_c * S_c in channel order, fp64
//                     fp32               fp64 products (exact) and fp64 accumulation in row order
//                     log2 exponents     (P2V_COS_LOG2K) a byte k is the probability 2^-k (0 from k = 16 on): the integer 2^(15-k), products
//                                        <= 2^30 into int64, the same tree and splits; converted once and scaled by 2^-30
//                   The 256 per-thread values are added over a fixed LDS tree and stored as the split's partial (int64 bits for the
//                   exact form, fp64 otherwise).
//   k_cos_combine   one thread per (stage, sample): the split partials in split order; int64 -> fp64 once for the exact form.
// No atomics: every result is bitwise repeatable, and the splitting depends on (n, rows, cols, dtype) only.
#include "p2vit_device.h"

#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_sdot4)
#define COS_DOT4(a, b, c) __builtin_amdgcn_sdot4((a), (b), (c), false)
#else
__device__ __forceinline__ int cos_dot4_sw(int a, int b, int c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c += (int)(int8_t)(a >> (8 * j)) * (int)(int8_t)(b >> (8 * j));
  return c;
}
#define COS_DOT4(a, b, c) cos_dot4_sw((a), (b), (c))
#endif

__device__ __forceinline__ int cos_find(const CosDesc* d, int L, long long item) {
  int lo = 0, hi = L - 1;                     // last stage whose first item is <= item
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].item0 <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// 16 codes at p (zeros from `valid` on); vec: the group is whole and 16-byte aligned
__device__ __forceinline__ v4i cos_load_i8(const int8_t* p, int valid, bool vec) {
  if (vec && valid >= 16) return *reinterpret_cast<const v4i*>(p);
  v4i v = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (j < valid) v[j >> 2] |= (int)((unsigned)(uint8_t)p[j] << (8 * (j & 3)));
  return v;
}
__device__ __forceinline__ float4 cos_load_f32(const float* p, int valid, bool vec) {
  if (vec && valid >= 4) return *reinterpret_cast<const float4*>(p);
  float4 v;
  v.x = valid > 0 ? p[0] : 0.f;
  v.y = valid > 1 ? p[1] : 0.f;
  v.z = valid > 2 ? p[2] : 0.f;
  v.w = valid > 3 ? p[3] : 0.f;
  return v;
}

template <typename T>
__device__ __forceinline__ void cos_block_sum(T (&red)[3][256], T s0, T s1, T s2, unsigned long long* out) {
  const int t = threadIdx.x;
  red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; red[2][t] += red[2][t + w];
    }
    __syncthreads();
  }
  if (t < 3) {
    const T v = red[t][0];
    unsigned long long bits;
    __builtin_memcpy(&bits, &v, 8);
    out[t] = bits;
  }
}

__device__ __forceinline__ void cos_partial_body(const CosDesc& d, long long local, unsigned long long* __restrict__ out) {
  __shared__ union { double d[3][256]; long long i[3][256]; } red;      // one tree buffer: int64 for the exact form, fp64 otherwise
  const int sample = (int)(local / d.nsplit), split = (int)(local % d.nsplit);
  const int r0 = split * d.rows_per_split, r1 = min(d.rows, r0 + d.rows_per_split);
  const int per = d.dtype == P2V_COS_F32 ? 4 : 16;               // elements of a 16-byte column group
  const int ncg = (d.cols + per - 1) / per;
  const int cgt = min(ncg, 256), lanes = 256 / cgt;              // column groups side by side, row lanes behind each other
  const int t = threadIdx.x, cgl = t % cgt, rl = t / cgt;
  const bool active = rl < lanes, vec = d.vec != 0;
  const long long s_off = (long long)sample * d.sample_stride;
  if (d.dtype == 0 && !d.scale) {
    long long sab = 0, saa = 0, sbb = 0;
    const int8_t* A = reinterpret_cast<const int8_t*>(d.a) + s_off;
    const int8_t* B = reinterpret_cast<const int8_t*>(d.b) + s_off;
    if (active)
      for (int cg = cgl; cg < ncg; cg += cgt) {
        const int c0 = cg * 16, valid = min(16, d.cols - c0);
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += lanes) {
          const long long o = (long long)r * d.row_stride + c0;
          const v4i va = cos_load_i8(A + o, valid, vec), vb = cos_load_i8(B + o, valid, vec);
          int ab = 0, aa = 0, bb = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            ab = COS_DOT4(va[q], vb[q], ab);
            aa = COS_DOT4(va[q], va[q], aa);
            bb = COS_DOT4(vb[q], vb[q], bb);
          }
          sab += ab; saa += aa; sbb += bb;
        }
      }
    cos_block_sum(red.i, sab, saa, sbb, out);
    return;
  }
  if (d.dtype == P2V_COS_LOG2K) {
    // exponents of the log2 softmax: p = 2^-k, k <= 15, else 0.  In units of 2^-15 the value is the integer 1 << (15 - k), the product of two at
    // most 2^30: sixteen of them fit a uint64 many times over, and the sample's sum stays below 2^53 (p2vit.h says why)
    long long sab = 0, saa = 0, sbb = 0;
    const int8_t* A = reinterpret_cast<const int8_t*>(d.a) + s_off;
    const int8_t* B = reinterpret_cast<const int8_t*>(d.b) + s_off;
    if (active)
      for (int cg = cgl; cg < ncg; cg += cgt) {
        const int c0 = cg * 16, valid = min(16, d.cols - c0);
#pragma unroll 2
        for (int r = r0 + rl; r < r1; r += lanes) {
          const long long o = (long long)r * d.row_stride + c0;
          const v4i va = cos_load_i8(A + o, valid, vec), vb = cos_load_i8(B + o, valid, vec);
          unsigned long long ab = 0, aa = 0, bb = 0;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const unsigned ka = ((unsigned)va[j >> 2] >> (8 * (j & 3))) & 255u, kb = ((unsigned)vb[j >> 2] >> (8 * (j & 3))) & 255u;
            const unsigned long long x = (j < valid && ka < 16u) ? 1ull << (15 - ka) : 0ull, y = (j < valid && kb < 16u) ? 1ull << (15 - kb) : 0ull;
            ab += x * y; aa += x * x; bb += y * y;
          }
          sab += (long long)ab; saa += (long long)aa; sbb += (long long)bb;
        }
      }
    cos_block_sum(red.i, sab, saa, sbb, out);
    return;
  }
  double dab = 0.0, daa = 0.0, dbb = 0.0;
  if (d.dtype == 0) {
    const int8_t* A = reinterpret_cast<const int8_t*>(d.a) + s_off;
    const int8_t* B = reinterpret_cast<const int8_t*>(d.b) + s_off;
    if (active)
      for (int cg = cgl; cg < ncg; cg += cgt) {
        const int c0 = cg * 16, valid = min(16, d.cols - c0);
        int cab[16], caa[16], cbb[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) cab[j] = caa[j] = cbb[j] = 0;
#pragma unroll 2
        for (int r = r0 + rl; r < r1; r += lanes) {
          const long long o = (long long)r * d.row_stride + c0;
          const v4i va = cos_load_i8(A + o, valid, vec), vb = cos_load_i8(B + o, valid, vec);
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int x = (int)(int8_t)(va[j >> 2] >> (8 * (j & 3))), y = (int)(int8_t)(vb[j >> 2] >> (8 * (j & 3)));
            cab[j] += x * y; caa[j] += x * x; cbb[j] += y * y;
          }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < valid) {
            const double s = (double)d.scale[c0 + j], s2 = s * s;
            dab += s2 * (double)cab[j]; daa += s2 * (double)caa[j]; dbb += s2 * (double)cbb[j];
          }
      }
  } else {
    const float* A = reinterpret_cast<const float*>(d.a) + s_off;
    const float* B = reinterpret_cast<const float*>(d.b) + s_off;
    if (active)
      for (int cg = cgl; cg < ncg; cg += cgt) {
        const int c0 = cg * 4, valid = min(4, d.cols - c0);
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += lanes) {
          const long long o = (long long)r * d.row_stride + c0;
          const float4 va = cos_load_f32(A + o, valid, vec), vb = cos_load_f32(B + o, valid, vec);
          dab += (double)va.x * (double)vb.x; daa += (double)va.x * (double)va.x; dbb += (double)vb.x * (double)vb.x;
          dab += (double)va.y * (double)vb.y; daa += (double)va.y * (double)va.y; dbb += (double)vb.y * (double)vb.y;
          dab += (double)va.z * (double)vb.z; daa += (double)va.z * (double)va.z; dbb += (double)vb.z * (double)vb.z;
          dab += (double)va.w * (double)vb.w; daa += (double)va.w * (double)va.w; dbb += (double)vb.w * (double)vb.w;
        }
      }
  }
  cos_block_sum(red.d, dab, daa, dbb, out);
}

__device__ __forceinline__ void cos_combine_body(const CosDesc& d, int sample, const unsigned long long* __restrict__ partials,
                                                 double* __restrict__ out) {
  const unsigned long long* p = partials + (d.item0 + (long long)sample * d.nsplit) * 3;
  if ((d.dtype == 0 && !d.scale) || d.dtype == P2V_COS_LOG2K) {
    long long s[3] = {0, 0, 0};
    for (int k = 0; k < d.nsplit; ++k)
#pragma unroll
      for (int q = 0; q < 3; ++q) s[q] += (long long)p[3 * k + q];
    const double unit = d.dtype == P2V_COS_LOG2K ? 0x1p-30 : 1.0;   // the exponent form counts in units of 2^-15 per value: a power of two, exact
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q] = (double)s[q] * unit;       // exact: |s| < 2^53 (checked by the host)
    return;
  }
  double s[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < d.nsplit; ++k)
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] += __longlong_as_double((long long)p[3 * k + q]);
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q] = s[q];
}

// grouped form: the stage records live in the workspace
__global__ __launch_bounds__(256) void k_cos_partial(const CosDesc* __restrict__ descs, int L, unsigned long long* __restrict__ partials) {
  const CosDesc d = descs[cos_find(descs, L, blockIdx.x)];
  cos_partial_body(d, (long long)blockIdx.x - d.item0, partials + (long long)blockIdx.x * 3);
}
__global__ __launch_bounds__(256) void k_cos_combine(const CosDesc* __restrict__ descs, int L, int n,
                                                     const unsigned long long* __restrict__ partials, double* __restrict__ sums) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= L * n) return;
  cos_combine_body(descs[idx / n], idx % n, partials, sums + (long long)idx * 3);
}
// one stage, its record in the kernel arguments (p2v_forward_ddv: nothing to upload between the launches of the forward)
__global__ __launch_bounds__(256) void k_cos_partial_one(const CosDesc d, unsigned long long* __restrict__ partials) {
  cos_partial_body(d, blockIdx.x, partials + (long long)blockIdx.x * 3);
}
__global__ __launch_bounds__(256) void k_cos_combine_one(const CosDesc d, int n, const unsigned long long* __restrict__ partials,
                                                         double* __restrict__ sums) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  cos_combine_body(d, idx, partials, sums + (long long)idx * 3);
}

// P2V_COS_I8_DEQ (internal; the attn.qact3 / mlp.qact2 stages of P2V_DDV_STAGES_FULL): int8 codes with per-channel scales where every VALUE is
// the fp32 product RN(code * scale[c]) - what the fake-quantising QAct hands to a forward hook (the PTF scales are no powers of two, so the
// product rounds).  fp64 products of those fp32 values (exact) and fp64 accumulation in row order, like the fp32 form; a kernel of its own,
// so that the three kernels above keep their code.
__global__ __launch_bounds__(256) void k_cos_partial_deq_one(const CosDesc d, unsigned long long* __restrict__ partials) {
  __shared__ double red[3][256];
  const long long local = blockIdx.x;
  const int sample = (int)(local / d.nsplit), split = (int)(local % d.nsplit);
  const int r0 = split * d.rows_per_split, r1 = min(d.rows, r0 + d.rows_per_split);
  const int ncg = (d.cols + 15) / 16;
  const int cgt = min(ncg, 256), lanes = 256 / cgt;
  const int t = threadIdx.x, cgl = t % cgt, rl = t / cgt;
  const bool active = rl < lanes, vec = d.vec != 0;
  const long long s_off = (long long)sample * d.sample_stride;
  const int8_t* A = reinterpret_cast<const int8_t*>(d.a) + s_off;
  const int8_t* B = reinterpret_cast<const int8_t*>(d.b) + s_off;
  double dab = 0.0, daa = 0.0, dbb = 0.0;
  if (active)
    for (int cg = cgl; cg < ncg; cg += cgt) {
      const int c0 = cg * 16, valid = min(16, d.cols - c0);
      float sc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) sc[j] = j < valid ? d.scale[c0 + j] : 0.f;
#pragma unroll 2
      for (int r = r0 + rl; r < r1; r += lanes) {
        const long long o = (long long)r * d.row_stride + c0;
        const v4i va = cos_load_i8(A + o, valid, vec), vb = cos_load_i8(B + o, valid, vec);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float x = (float)(int)(int8_t)(va[j >> 2] >> (8 * (j & 3))) * sc[j], y = (float)(int)(int8_t)(vb[j >> 2] >> (8 * (j & 3))) * sc[j];
          dab += (double)x * (double)y; daa += (double)x * (double)x; dbb += (double)y * (double)y;
        }
      }
    }
  cos_block_sum(red, dab, daa, dbb, partials + local * 3);
}

// one stage of a recorded sequence (P2V_OP_COS): its record sits in a device table that the closing k_cos_combine walks; the stage's workgroups
// write the partial slots [item0, item0 + n * nsplit) of that table's numbering
__global__ __launch_bounds__(256) void k_cos_partial_stage(const CosDesc* __restrict__ desc, unsigned long long* __restrict__ partials) {
  const CosDesc d = *desc;
  cos_partial_body(d, blockIdx.x, partials + (d.item0 + (long long)blockIdx.x) * 3);
}

// ---------------------------------------------------------------------------------------------------
// host side (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
// How a sample is split: ~16 KB per operand and workgroup, at most ~2048 workgroups per stage, at most 2^16 rows per workgroup (the int32
// per-channel sums of the scaled form).  A function of (n, rows, cols, dtype) only.
CosDesc p2v_cos_desc(const p2v_cos_layer& a, int n, long long item0) {
  CosDesc d;
  d.a = a.a; d.b = a.b; d.scale = a.scale;
  d.sample_stride = a.sample_stride; d.row_stride = a.row_stride;
  d.rows = a.rows; d.cols = a.cols; d.dtype = a.dtype;
  const long long esz = a.dtype == P2V_COS_F32 ? 4 : 1;
  d.vec = ((uintptr_t)a.a % 16 == 0 && (uintptr_t)a.b % 16 == 0 && a.sample_stride * esz % 16 == 0 && a.row_stride * esz % 16 == 0) ? 1 : 0;
  const long long bytes = (long long)a.rows * a.cols * esz;
  long long ns = (bytes + 16383) / 16384;
  const long long cap = n >= 2048 ? 1 : 2048 / n;
  if (ns > cap) ns = cap;
  if (ns > a.rows) ns = a.rows;
  const long long min_ns = ((long long)a.rows + 65535) / 65536;
  if (ns < min_ns) ns = min_ns;
  d.rows_per_split = (int)((a.rows + ns - 1) / ns);
  d.nsplit = (a.rows + d.rows_per_split - 1) / d.rows_per_split;
  d.item0 = item0;
  return d;
}

CosLayout p2v_cos_layout(const p2v_cos_layer* layers, int L, int n, std::vector<CosDesc>* descs) {
  CosLayout w;
  long long items = 0;
  for (int l = 0; l < L; ++l) {
    const CosDesc d = p2v_cos_desc(layers[l], n, items);
    items += (long long)n * d.nsplit;
    if (descs) descs->push_back(d);
  }
  w.items = items;
  w.desc_off = 0;
  w.part_off = ((size_t)L * sizeof(CosDesc) + 255) / 256 * 256;
  w.total = w.part_off + (size_t)items * 3 * sizeof(unsigned long long);
  return w;
}

int p2v_launch_pair_cosine(const std::vector<CosDesc>& descs, const CosLayout& w, int n, double* sums, void* ws, hipStream_t st) {
  const int L = (int)descs.size();
  char* base = reinterpret_cast<char*>(ws);
  CosDesc* dd = reinterpret_cast<CosDesc*>(base + w.desc_off);
  unsigned long long* parts = reinterpret_cast<unsigned long long*>(base + w.part_off);
  if (w.items >= (1LL << 31) || (long long)L * n >= (1LL << 31)) return -1;
  // pageable source on a stream that is NOT capturing (p2v_pair_cosine refuses a capturing one): the runtime stages it before returning, so
  // the host vector may go away afterwards.  Recorded into a graph the copy node would keep the host pointer - and these descriptors hold
  // device pointers: a replay would launch on garbage addresses
  hipError_t e = hipMemcpyAsync(dd, descs.data(), descs.size() * sizeof(CosDesc), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_cos_partial, dim3((unsigned)w.items), dim3(256), 0, st, dd, L, parts);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cos_combine, dim3((unsigned)(((long long)L * n + 255) / 256)), dim3(256), 0, st, dd, L, n, parts, sums);
  CHECK_LAUNCH();
  return 0;
}

// one stage of p2v_forward_ddv: `partials` holds n * d.nsplit * 3 slots and is reused by the next stage on the same stream
int p2v_launch_pair_cosine_one(const CosDesc& d, int n, unsigned long long* partials, double* sums, hipStream_t st) {
  if (d.dtype == P2V_COS_I8_DEQ) hipLaunchKernelGGL(k_cos_partial_deq_one, dim3((unsigned)(n * d.nsplit)), dim3(256), 0, st, d, partials);
  else hipLaunchKernelGGL(k_cos_partial_one, dim3((unsigned)(n * d.nsplit)), dim3(256), 0, st, d, partials);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(k_cos_combine_one, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, n, partials, sums);
  CHECK_LAUNCH();
  return 0;
}

// P2V_OP_COS: the stage whose record is *desc_dev (items = n * nsplit of that record); P2V_OP_COS_COMBINE: every stage of the table at once
int p2v_launch_cos_stage(const CosDesc* desc_dev, long long items, unsigned long long* partials, hipStream_t st) {
  if (items < 1 || items >= (1LL << 31)) return -1;
  hipLaunchKernelGGL(k_cos_partial_stage, dim3((unsigned)items), dim3(256), 0, st, desc_dev, partials);
  CHECK_LAUNCH();
  return 0;
}
int p2v_launch_cos_combine(const CosDesc* descs_dev, int L, int n, const unsigned long long* partials, double* sums, hipStream_t st) {
  if ((long long)L * n >= (1LL << 31)) return -1;
  hipLaunchKernelGGL(k_cos_combine, dim3((unsigned)(((long long)L * n + 255) / 256)), dim3(256), 0, st, descs_dev, L, n, partials, sums);
  CHECK_LAUNCH();
  return 0;
}
