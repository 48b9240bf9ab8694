// p2vit_launch.h -- host-only helpers of the launcher sections: the dynamic-LDS grant record and the builder of the instantiation tables.
// Every kernel family ends in one small selection function and one table; the tables are the list of instantiations the library can select.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <utility>

// The largest dynamic LDS size an instantiation has been granted so far, per device 0..15 (beyond the 64 KB a kernel gets by default the
// runtime has to be asked).  One record per instantiation: a zero-initialised `static P2vLdsGrant` next to the launch, so there is no lock
// and no lazy initialisation - the forward enqueues from several host threads, and a racing second thread only repeats the call with the
// same value.  A device index outside 0..15 asks every time.  The caller decides what a failure means.
struct P2vLdsGrant {
  int granted[16];
  hipError_t ensure(const void* fn, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
    if (dev >= 0 && bytes <= granted[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0) granted[dev] = bytes;
    return e;
  }
};

// table[i] = G::at<i>() for i in [0, N): G decodes the flat index into its template arguments and returns the kernel (or per-instantiation
// launcher) pointer, or null for a combination that is not instantiated.  The compiler instantiates in index order, and that is the order
// in which the kernels lie in the code object: the layouts (boolean dimensions true first, the epilogue lists) keep the order the kernels
// have always had, so that a build's device code compares equal to the build before it (tools/kernel_resources.py --digest).  A table has
// ONE constexpr index function: the launcher encodes with it, and G::at<i>() asserts that what it decoded from i encodes back to i
template <class T, class G, int... I>
constexpr std::array<T, sizeof...(I)> p2v_table_(std::integer_sequence<int, I...>) {
  return {{G::template at<I>()...}};
}
template <class T, class G, int N>
constexpr std::array<T, N> p2v_table() {
  return p2v_table_<T, G>(std::make_integer_sequence<int, N>{});
}

// position of an epilogue code in a table's list of them; -1: the table has none
template <int N>
constexpr int p2v_slot(const int (&codes)[N], int code) {
  for (int i = 0; i < N; ++i)
    if (codes[i] == code) return i;
  return -1;
}
