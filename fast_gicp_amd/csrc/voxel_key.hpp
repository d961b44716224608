// Voxel keys and the hash that places them in a table: coord = floor(p / res - 0.5)  (fast_vgicp_voxel.hpp:158-160 /
// vector3_hash.cuh:35-38), packed 21 bits per axis into one 64-bit key so bucket claims are a single 64-bit CAS.
// Plain C++: the kernels (through dev_math.hpp) and the stand-alone host check (tests/cpp/voxel_key_check.cpp) compile the same
// functions; tests/table_sim.py restates pack_key and hash_slot in numpy and is held to that program's output.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FVH_KEY_FN __device__ __forceinline__
#define FVH_KEY_HD_FN __host__ __device__ __forceinline__
#else
#define FVH_KEY_FN inline
#define FVH_KEY_HD_FN inline
#endif
#if defined(__GNUC__) || defined(__clang__)
#define FVH_CLZ32(x) __builtin_clz(x)
#else
static inline int fvh_clz32_portable(unsigned x) { int n = 0; while (!(x & 0x80000000u)) { x <<= 1; n++; } return n; }  // x != 0
#define FVH_CLZ32(x) fvh_clz32_portable(x)
#endif

#define FVH_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull
#define FVH_COORD_BIAS (1 << 20)

namespace fvh {

FVH_KEY_FN unsigned long long pack_key(int x, int y, int z) {
  return (unsigned long long)(unsigned)(x + FVH_COORD_BIAS) | ((unsigned long long)(unsigned)(y + FVH_COORD_BIAS) << 21) |
         ((unsigned long long)(unsigned)(z + FVH_COORD_BIAS) << 42);
}
FVH_KEY_HD_FN void unpack_key(unsigned long long k, int& x, int& y, int& z) {
  x = (int)(k & 0x1FFFFF) - FVH_COORD_BIAS;
  y = (int)((k >> 21) & 0x1FFFFF) - FVH_COORD_BIAS;
  z = (int)((k >> 42) & 0x1FFFFF) - FVH_COORD_BIAS;
}
FVH_KEY_FN bool coord_in_range(int x, int y, int z) {
  return (unsigned)(x + FVH_COORD_BIAS) < (1u << 21) && (unsigned)(y + FVH_COORD_BIAS) < (1u << 21) && (unsigned)(z + FVH_COORD_BIAS) < (1u << 21);
}
// (int)floor(v) is undefined for NaN/inf/huge v (a lidar return at infinity, a 1e9 outlier): test the floating value first.
// |f| < 2^20 - 2^12 leaves room for any neighbour offset the engine accepts and keeps the key inside its 21 bits.
template <typename T>
FVH_KEY_FN bool voxel_index_ok(T fx, T fy, T fz) {
  const T lim = (T)(FVH_COORD_BIAS - 4096);
  return fabs(fx) < lim && fabs(fy) < lim && fabs(fz) < lim;  // false for NaN
}
// 64-bit mix (murmur3 finaliser); the bucket layout is private so the hash is ours to choose
// Multiplicative (Fibonacci) hash of the packed voxel key: two 32-bit multiplies. The GOOD bits are the high ones -- every
// input bit reaches them -- so tables index with hash_slot() (top log2(capacity) bits), never with the low bits.
// (Round 1 used the 64-bit murmur finaliser: two 64-bit multiplies = eight quarter-rate 32-bit multiplies per lookup, ~5 % of
// the VALU time of the LM kernel's main loop, for a table whose keys are small consecutive integers.)
FVH_KEY_FN unsigned hash_key(unsigned long long k) {
  return (unsigned)k * 0x9E3779B1u + (unsigned)(k >> 32) * 0x85EBCA77u;
}
FVH_KEY_FN unsigned hash_slot(unsigned long long k, unsigned mask /* capacity - 1, capacity a power of two */) {
  return mask ? hash_key(k) >> FVH_CLZ32(mask) : 0u;
}

}  // namespace fvh
