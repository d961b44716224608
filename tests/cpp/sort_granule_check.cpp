// Stand-alone host check of the histogram granule of the cooperative small sort (fast_gicp_amd/csrc/sort_granule.hpp): the same
// functions the kernel packs and unpacks with. Every count 0 ... 1,024 in every slot beside extreme neighbours, every tag bit, the
// tags on both sides of the points where they repeat, and the sequence numbers that are skipped because their tag would be 0.
#include <cstdio>
#include "sort_granule.hpp"

using namespace fvh;

static int fails = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (fails++ < 20) std::printf("MISMATCH line %d: %s\n", __LINE__, #cond); \
    }                                                                     \
  } while (0)

int main() {
  static_assert(COOP_COUNT_BITS * COOP_GRANULE_COUNTS + COOP_HTAG_BITS == 64, "a granule is one 64-bit word");
  static_assert(1024u <= COOP_COUNT_MASK, "a slot holds a whole workgroup's 1,024 keys");
  const unsigned others[] = {0u, 1u, 1023u, 1024u, COOP_COUNT_MASK};
  const unsigned tags[] = {1u, 2u, 0x55555u & COOP_HTAG_MASK, 0xAAAAAu & COOP_HTAG_MASK, COOP_HTAG_MASK - 1u, COOP_HTAG_MASK};
  long checked = 0;
  for (int slot = 0; slot < COOP_GRANULE_COUNTS; slot++)
    for (unsigned v = 0; v <= 1024u; v++)
      for (unsigned o : others)
        for (unsigned t : tags) {
          unsigned c[COOP_GRANULE_COUNTS];
          for (int s = 0; s < COOP_GRANULE_COUNTS; s++) c[s] = (s == slot) ? v : o;
          const unsigned long long g = coop_granule_pack(c[0], c[1], c[2], c[3], t);
          CHECK(coop_granule_tag(g) == t);
          for (int s = 0; s < COOP_GRANULE_COUNTS; s++) CHECK(coop_granule_count(g, s) == c[s]);
          CHECK(g != 0ull);  // a written granule never looks like fresh memory
          checked++;
        }
  // every tag bit alone survives the round trip and leaves the counts alone
  for (int b = 0; b < COOP_HTAG_BITS; b++) {
    const unsigned long long g = coop_granule_pack(1024u, 0u, 1024u, 0u, 1u << b);
    CHECK(coop_granule_tag(g) == (1u << b));
    CHECK(coop_granule_count(g, 0) == 1024u && coop_granule_count(g, 1) == 0u && coop_granule_count(g, 2) == 1024u && coop_granule_count(g, 3) == 0u);
  }
  // tags: the two passes of a launch differ, consecutive launches differ, and no sequence number that is handed out has tag 0
  const unsigned period = (COOP_HTAG_MASK >> 1) + 1u;  // launches after which the tags repeat
  const unsigned starts[] = {0u, period - 3u, 2u * period - 3u, 0xFFFFFFFFu - 2u * period, 0xFFFFFFFFu - 3u};
  for (unsigned s0 : starts) {
    unsigned seq = s0;
    for (int i = 0; i < 8; i++) {
      const unsigned next = coop_next_seq(seq);
      CHECK(next != seq);
      CHECK(coop_htag(next, 0) != 0u && coop_htag(next, 1) != 0u);
      CHECK(coop_htag(next, 0) != coop_htag(next, 1));
      CHECK(coop_htag(next, 0) <= COOP_HTAG_MASK && coop_htag(next, 1) <= COOP_HTAG_MASK);
      if (i > 0) CHECK(coop_htag(next, 0) != coop_htag(seq, 0) && coop_htag(next, 0) != coop_htag(seq, 1) && coop_htag(next, 1) != coop_htag(seq, 1));
      const unsigned step = next - seq;  // (wraps with the 32-bit counter)
      CHECK(step == 1u || (step == 2u && ((seq + 1u) & (COOP_HTAG_MASK >> 1)) == 0u));
      seq = next;
    }
  }
  CHECK(coop_next_seq(0u) == 1u);
  CHECK(coop_next_seq(period - 1u) == period + 1u);          // `period` itself would have tag 0 in pass 0
  CHECK(coop_next_seq(0xFFFFFFFFu) == 1u);                   // the 32-bit counter wraps past 0
  CHECK(coop_htag(period + 1u, 0) == coop_htag(1u, 0));       // the tags repeat after `period` launches, as documented
  std::printf("%ld granules checked, %d mismatches\n", checked, fails);
  return fails ? 1 : 0;
}
