// The word the workgroups of the cooperative small sort (kernels_sort.hpp, sort_coop_kernel) exchange their digit histograms in: ONE
// 8-byte granule = the counts of four consecutive bins, 11 bits each (a workgroup holds at most 1,024 keys, so a count is 0 ... 1,024),
// under ONE 20-bit tag that names the launch and the pass. A lane stores and loads a granule whole, so one tag vouches for all four
// counts: a workgroup publishes 1 KB per pass and reads 32 KB, half of what one {count, tag} word per bin took.
// Plain C++: the kernel and the stand-alone host check (tests/cpp/sort_granule_check.cpp) compile the same functions.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FVH_GRANULE_FN __host__ __device__ __forceinline__
#else
#define FVH_GRANULE_FN inline
#endif

namespace fvh {

constexpr int COOP_COUNT_BITS = 11;                                          // a workgroup's count of one bin: 0 ... 1,024
constexpr int COOP_GRANULE_COUNTS = 4;                                       // bins per granule
constexpr int COOP_HTAG_SHIFT = COOP_COUNT_BITS * COOP_GRANULE_COUNTS;       // 44: the tag sits above the counts
constexpr int COOP_HTAG_BITS = 64 - COOP_HTAG_SHIFT;                         // 20
constexpr unsigned COOP_COUNT_MASK = (1u << COOP_COUNT_BITS) - 1u;
constexpr unsigned COOP_HTAG_MASK = (1u << COOP_HTAG_BITS) - 1u;

// tag of launch `seq`, pass 0 / 1. Never 0 for the sequence numbers coop_next_seq hands out: 0 is what memory nobody wrote holds.
FVH_GRANULE_FN unsigned coop_htag(unsigned seq, int pass) { return ((seq << 1) | (unsigned)pass) & COOP_HTAG_MASK; }

// the sequence number after `seq`, skipping those whose pass-0 tag would be 0 (the first one handed out is 1; the tag repeats every
// 2^19 launches of an engine)
FVH_GRANULE_FN unsigned coop_next_seq(unsigned seq) {
  ++seq;
  if ((seq & (COOP_HTAG_MASK >> 1)) == 0) ++seq;
  return seq;
}

FVH_GRANULE_FN unsigned long long coop_granule_pack(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned tag) {
  return (unsigned long long)c0 | ((unsigned long long)c1 << COOP_COUNT_BITS) | ((unsigned long long)c2 << (2 * COOP_COUNT_BITS)) |
         ((unsigned long long)c3 << (3 * COOP_COUNT_BITS)) | ((unsigned long long)tag << COOP_HTAG_SHIFT);
}
FVH_GRANULE_FN unsigned coop_granule_tag(unsigned long long g) { return (unsigned)(g >> COOP_HTAG_SHIFT); }
FVH_GRANULE_FN unsigned coop_granule_count(unsigned long long g, int slot) { return (unsigned)(g >> (slot * COOP_COUNT_BITS)) & COOP_COUNT_MASK; }

}  // namespace fvh
