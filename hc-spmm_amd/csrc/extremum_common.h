// extremum_common.h -- the (value, position) order and the int32 lane vectors shared by spmm_extremum.hip (max / min with argmax)
// and spmm_multi.hip (sum, sum of squares, max and min in one pass).
#pragma once
#include "spmm_impl.h"

namespace hcspmm {

constexpr int kNone = 0x7fffffff;  // position of "no entry yet": loses to every entry

// tiny tasks per lane group: TinyT's, but two at L = 32 (four spilled 148 bytes per lane at five waves per SIMD)
template <int L> struct XTinyT {
  static constexpr int value = L >= 32 ? 2 : TinyT<L>::value;
};

// (MemI32, IntV: spmm_impl.h)
__device__ __forceinline__ int iget(const int& v, int) { return v; }
template <typename V> __device__ __forceinline__ int iget(const V& v, int i) { return v[i]; }
__device__ __forceinline__ void iset(int& v, int, int x) { v = x; }
template <typename V> __device__ __forceinline__ void iset(V& v, int i, int x) { v[i] = x; }

template <int VEC> __device__ __forceinline__ typename IntV<VEC>::type iload(const int* p) {
  return *reinterpret_cast<const typename MemI32<VEC>::type*>(p);
}
template <int VEC> __device__ __forceinline__ void istore(int* p, const typename IntV<VEC>::type& v) {
  __builtin_nontemporal_store(v, reinterpret_cast<typename MemI32<VEC>::type*>(p));
}

// (a, pa) comes before (b, pb) in the max order
__device__ __forceinline__ bool xbeats(float a, int pa, float b, int pb) {
  const bool an = a != a, bn = b != b;
  return an ? (!bn || pa < pb) : (!bn && (a > b || (a == b && pa < pb)));
}

__device__ __forceinline__ float xflip(float v, unsigned flip) { return __uint_as_float(__float_as_uint(v) ^ flip); }

}  // namespace hcspmm
