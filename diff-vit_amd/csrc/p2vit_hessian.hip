// p2vit_hessian.hip -- the per-probe bookkeeping of the Hutchinson trace estimate (p2v_rademacher_fill, p2v_group_dot,
// p2v_hutchinson_init / p2v_hutchinson_step, include/p2vit.h; pyhessian/hessian.py:163-211 of the reference).  The double backward is
// torch's autograd; what stands here is what surrounds it: the +-1 probe vectors of all selected tensors in one launch, v . Hv of all of
// them in two, and the stopping rule of every layer on the device.
//
// One launch covers up to HS_MAX_SEGS segments (tensors).  Their table - pointers, lengths, generator keys and the prefix sums of their
// chunk counts - travels as the launch's kernel argument: the launch copies it into device-visible memory, nothing is uploaded,
// nothing synchronises and a graph capture records it.  A workgroup finds its segment by a bisection of the prefix table (wave-uniform).
// A chunk is 256 threads x 4 quads of 4 floats.  Quads start at the first 16-byte boundary of the segment, so the body moves as
// float4; the up to three elements in front of it (written by the first threads of chunk 0) and the tail behind the last whole quad are
// scalar.  Element and chunk arithmetic is 64-bit.
//   k_hs_fill      element e of a segment = +1 / -1 by bit e % 64 of splitmix64(key + e / 64); key is made on the host from
//                  (seed, layer, probe) - hs_key below, restated in hessian.rademacher_host - so a segment's values depend on nothing
//                  else in the call
//   k_hs_dot       per chunk: sum of (double)a[e] * (double)b[e] (each product exact), thread sums in element order, then a fixed
//                  shuffle tree and the four waves in wave order; one fp64 partial per chunk
//   k_hs_finish    one workgroup per segment: its partials, thread t taking t, t + 256, ..., then the same fixed tree; out[segment].
//                  With a state: the stopping rule of the segment's layer (hs_stop_update, one thread)
// No floating-point atomics: the same input gives the same bytes.  The running-layer counter is an integer.
#include "p2vit_device.h"

#define HS_THREADS 256
#define HS_ITERS 4                                  // quads per thread and chunk
#define HS_CHUNK_QUADS (HS_THREADS * HS_ITERS)      // 1024 quads = 4096 floats

struct HsFillTab {
  float* ptr[HS_MAX_SEGS];
  long long n[HS_MAX_SEGS];
  unsigned long long key[HS_MAX_SEGS];
  unsigned first[HS_MAX_SEGS + 1];                  // prefix sums of the chunk counts; first[n_segs] = the grid
  int n_segs;
};
struct HsDotTab {
  const float* a[HS_MAX_SEGS];
  const float* b[HS_MAX_SEGS];
  long long n[HS_MAX_SEGS];
  unsigned first[HS_MAX_SEGS + 1];
  int n_segs;
};
struct HsFinishTab {
  unsigned first[HS_MAX_SEGS + 1];
  int n_segs;
};

// per-layer stopping state (p2v_hutchinson_state_bytes): a 16-byte header, then one record per layer
struct HsHeader {
  int running;                                      // layers that have not stopped: the one word the host polls
  int n_layers;
  int pad[2];
};
struct HsLayer {
  double sum;                                       // values[0 .. i] added in index order
  double trace;                                     // the previous prefix mean (the result once done)
  int probes;                                       // probes consumed: stop index + 1 once done
  int done;
  int converged;                                    // stopped by the tolerance (not by running out of probes: the host decides that)
  int pad;
};

__host__ __device__ __forceinline__ unsigned long long hs_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// key of (seed, layer, probe): word j of the stream is splitmix64(key + j)
static unsigned long long hs_key(unsigned long long seed, int layer, unsigned long long probe) {
  return hs_splitmix64(hs_splitmix64(hs_splitmix64(seed) ^ (unsigned long long)(unsigned)layer) ^ probe);
}

__device__ __forceinline__ float hs_sign(unsigned long long word, long long e) { return (word >> (e & 63)) & 1ull ? 1.0f : -1.0f; }
__device__ __forceinline__ float hs_sign_at(unsigned long long key, long long e) {
  return hs_sign(hs_splitmix64(key + (unsigned long long)(e >> 6)), e);
}

// elements in front of the first 16-byte boundary (the pointer is 4-byte aligned), at most n
__host__ __device__ __forceinline__ int hs_head(const void* p, long long n) {
  const int h = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
  return (long long)h < n ? h : (int)n;
}
static unsigned hs_chunks(const void* p, long long n) {
  const long long quads = (n - hs_head(p, n) + 3) >> 2;
  const long long c = (quads + HS_CHUNK_QUADS - 1) / HS_CHUNK_QUADS;
  return (unsigned)(c < 1 ? 1 : c);                 // a segment that is all head still gets the chunk that writes it
}

// the segment of workgroup b: first[s] <= b < first[s + 1]
template <typename Tab>
__device__ __forceinline__ int hs_segment_of(const Tab& t, unsigned b) {
  int lo = 0, hi = t.n_segs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(HS_THREADS) void k_hs_fill(const HsFillTab t) {
  const int s = hs_segment_of(t, blockIdx.x);
  float* __restrict__ p = t.ptr[s];
  const long long n = t.n[s];
  const unsigned long long key = t.key[s];
  const long long c = (long long)(blockIdx.x - t.first[s]);
  const int h = hs_head(p, n);
  if (c == 0 && (int)threadIdx.x < h) p[threadIdx.x] = hs_sign_at(key, threadIdx.x);
  const long long quads = (n - h + 3) >> 2;
#pragma unroll
  for (int it = 0; it < HS_ITERS; ++it) {
    const long long q = c * HS_CHUNK_QUADS + it * HS_THREADS + threadIdx.x;
    if (q >= quads) break;
    const long long e0 = h + 4 * q;
    if (e0 + 3 < n) {
      const unsigned long long w0 = hs_splitmix64(key + (unsigned long long)(e0 >> 6));
      const unsigned long long w1 = ((e0 + 3) >> 6) == (e0 >> 6) ? w0 : hs_splitmix64(key + (unsigned long long)((e0 + 3) >> 6));
      float4 v;
      v.x = hs_sign(w0, e0);
      v.y = hs_sign(((e0 + 1) >> 6) == (e0 >> 6) ? w0 : w1, e0 + 1);
      v.z = hs_sign(((e0 + 2) >> 6) == (e0 >> 6) ? w0 : w1, e0 + 2);
      v.w = hs_sign(w1, e0 + 3);
      *reinterpret_cast<float4*>(p + e0) = v;
    } else {
      for (long long e = e0; e < n; ++e) p[e] = hs_sign_at(key, e);
    }
  }
}

// the workgroup's sum: 64 lanes by a fixed butterfly, the four waves in wave order; valid in thread 0
__device__ __forceinline__ double hs_block_sum(double v, double (&red)[HS_THREADS / 64]) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(HS_THREADS) void k_hs_dot(const HsDotTab t, double* __restrict__ partials) {
  __shared__ double red[HS_THREADS / 64];
  const int s = hs_segment_of(t, blockIdx.x);
  const float* __restrict__ a = t.a[s];
  const float* __restrict__ b = t.b[s];
  const long long n = t.n[s];
  const long long c = (long long)(blockIdx.x - t.first[s]);
  const int h = hs_head(a, n);
  const bool vec = (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0;      // b reaches its 16-byte boundary where a does
  double acc = 0.0;
  if (c == 0 && (int)threadIdx.x < h) acc = (double)a[threadIdx.x] * (double)b[threadIdx.x];
  const long long quads = (n - h + 3) >> 2;
#pragma unroll
  for (int it = 0; it < HS_ITERS; ++it) {
    const long long q = c * HS_CHUNK_QUADS + it * HS_THREADS + threadIdx.x;
    if (q >= quads) break;
    const long long e0 = h + 4 * q;
    if (e0 + 3 < n) {
      float4 x, y;
      if (vec) {
        x = *reinterpret_cast<const float4*>(a + e0);
        y = *reinterpret_cast<const float4*>(b + e0);
      } else {
        x = make_float4(a[e0], a[e0 + 1], a[e0 + 2], a[e0 + 3]);
        y = make_float4(b[e0], b[e0 + 1], b[e0 + 2], b[e0 + 3]);
      }
      acc += (double)x.x * (double)y.x;
      acc += (double)x.y * (double)y.y;
      acc += (double)x.z * (double)y.z;
      acc += (double)x.w * (double)y.w;
    } else {
      for (long long e = e0; e < n; ++e) acc += (double)a[e] * (double)b[e];
    }
  }
  const double total = hs_block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// hessian.py:177-209 for one layer and one new value: the prefix mean against the previous one.  Restated on the host as
// hessian.stop_scan; the operations (add, divide, subtract, abs, compare; no contraction) round the same on both.
__device__ __forceinline__ void hs_stop_update(HsHeader* hd, HsLayer* L, double value, int probe, double tol) {
  if (L->done) return;                              // a probe past the stop index: discarded
  const double sum = L->sum + value;
  const double mean = sum / (double)(probe + 1);
  const double trace = L->trace;
  L->sum = sum;
  L->probes = probe + 1;
  if (fabs(mean - trace) / (fabs(trace) + 1e-6) < tol) {
    L->done = 1;
    L->converged = 1;
    atomicSub(&hd->running, 1);
  } else {
    L->trace = mean;
  }
}

__global__ __launch_bounds__(HS_THREADS) void k_hs_finish(const HsFinishTab t, const double* __restrict__ partials, double* __restrict__ out,
                                                          void* state, int layer0, int probe, double tol) {
  __shared__ double red[HS_THREADS / 64];
  const int s = blockIdx.x;
  const unsigned p0 = t.first[s], p1 = t.first[s + 1];
  double acc = 0.0;
  for (unsigned p = p0 + threadIdx.x; p < p1; p += HS_THREADS) acc += partials[p];
  const double total = hs_block_sum(acc, red);
  if (threadIdx.x == 0) {
    out[s] = total;
    if (state) {
      HsHeader* hd = static_cast<HsHeader*>(state);
      hs_stop_update(hd, reinterpret_cast<HsLayer*>(hd + 1) + layer0 + s, total, probe, tol);
    }
  }
}

__global__ __launch_bounds__(HS_THREADS) void k_hs_init(void* state, int n_layers) {
  HsHeader* hd = static_cast<HsHeader*>(state);
  HsLayer* L = reinterpret_cast<HsLayer*>(hd + 1);
  if (threadIdx.x == 0) {
    hd->running = n_layers;
    hd->n_layers = n_layers;
    hd->pad[0] = hd->pad[1] = 0;
  }
  for (int l = threadIdx.x; l < n_layers; l += HS_THREADS) {
    L[l].sum = 0.0;
    L[l].trace = 0.0;
    L[l].probes = L[l].done = L[l].converged = L[l].pad = 0;
  }
}

// ---------------------------------------------------------------------------------------------------
// host launchers (argument validation in p2vit_capi.cpp)
// ---------------------------------------------------------------------------------------------------
size_t p2v_hs_state_bytes(int n_layers) { return sizeof(HsHeader) + (size_t)n_layers * sizeof(HsLayer); }

long long p2v_hs_dot_chunks(const p2v_seg2* segs, int n_segs) {
  long long total = 0;
  for (int s = 0; s < n_segs; ++s) total += hs_chunks(segs[s].a, segs[s].n);
  return total;
}

int p2v_launch_rademacher_fill(const p2v_seg* segs, int n_segs, unsigned long long seed, unsigned long long probe, hipStream_t st) {
  for (int s0 = 0; s0 < n_segs; s0 += HS_MAX_SEGS) {
    HsFillTab t;
    t.n_segs = n_segs - s0 < HS_MAX_SEGS ? n_segs - s0 : HS_MAX_SEGS;
    t.first[0] = 0;
    for (int s = 0; s < t.n_segs; ++s) {
      const p2v_seg& g = segs[s0 + s];
      t.ptr[s] = g.ptr;
      t.n[s] = g.n;
      t.key[s] = hs_key(seed, g.layer, probe);
      t.first[s + 1] = t.first[s] + hs_chunks(g.ptr, g.n);
    }
    hipLaunchKernelGGL(k_hs_fill, dim3(t.first[t.n_segs]), dim3(HS_THREADS), 0, st, t);
    CHECK_LAUNCH();
  }
  return 0;
}

// out[s] of every segment; state != null: the stopping update of layer s with `probe` and `tol` behind it
int p2v_launch_group_dot(const p2v_seg2* segs, int n_segs, double* out, double* partials, void* state, int probe, double tol, hipStream_t st) {
  long long base = 0;
  for (int s0 = 0; s0 < n_segs; s0 += HS_MAX_SEGS) {
    HsDotTab t;
    HsFinishTab f;
    t.n_segs = f.n_segs = n_segs - s0 < HS_MAX_SEGS ? n_segs - s0 : HS_MAX_SEGS;
    t.first[0] = f.first[0] = 0;
    for (int s = 0; s < t.n_segs; ++s) {
      const p2v_seg2& g = segs[s0 + s];
      t.a[s] = g.a;
      t.b[s] = g.b;
      t.n[s] = g.n;
      t.first[s + 1] = f.first[s + 1] = t.first[s] + hs_chunks(g.a, g.n);
    }
    hipLaunchKernelGGL(k_hs_dot, dim3(t.first[t.n_segs]), dim3(HS_THREADS), 0, st, t, partials + base);
    CHECK_LAUNCH();
    hipLaunchKernelGGL(k_hs_finish, dim3((unsigned)t.n_segs), dim3(HS_THREADS), 0, st, f, partials + base, out + s0, state, s0, probe, tol);
    CHECK_LAUNCH();
    base += t.first[t.n_segs];
  }
  return 0;
}

int p2v_launch_hutchinson_init(void* state, int n_layers, hipStream_t st) {
  hipLaunchKernelGGL(k_hs_init, dim3(1), dim3(HS_THREADS), 0, st, state, n_layers);
  CHECK_LAUNCH();
  return 0;
}
