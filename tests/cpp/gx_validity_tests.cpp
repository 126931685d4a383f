// gx_validity_tests -- the word arithmetic of cudf_amd/csrc/gx_validity.hpp (part (a): what the value kernels read validity words
// with) against bit-by-bit loops, on the CPU.  Includes that header alone and links no library.  Every bitmap is a heap array of
// exactly the words a call may read, so a build with -fsanitize=address,undefined turns a read behind the last requested bit into
// a report, and a shift by the operand's full width into another.
#include <stdint.h>
#include <stdio.h>

#include <memory>
#include <vector>

#include "../../cudf_amd/csrc/gx_validity.hpp"

static int failed = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (++failed <= 20) {                  \
        printf("FAILED %s: ", #cond);        \
        printf(__VA_ARGS__);                 \
        printf("\n");                        \
      }                                      \
    }                                        \
  } while (0)

static uint64_t splitmix(uint64_t& s)
{
  uint64_t x = (s += 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// pattern 0: all bits 0, 1: all bits 1, from 2 on: seeded random words
static std::unique_ptr<uint32_t[]> bitmap(int64_t nwords, int pattern)
{
  std::unique_ptr<uint32_t[]> m(new uint32_t[nwords]);
  uint64_t seed = 1000u + (uint64_t)pattern;
  for (int64_t w = 0; w < nwords; ++w) m[w] = pattern == 0 ? 0u : pattern == 1 ? 0xFFFFFFFFu : (uint32_t)splitmix(seed);
  return m;
}
static bool bit_of(const uint32_t* m, int64_t i) { return (m[i / 32] >> (i % 32)) & 1u; }

constexpr int PATTERNS = 6;

int main()
{
  for (int cnt = 0; cnt <= 32; ++cnt) {
    uint32_t want = 0;
    for (int k = 0; k < cnt; ++k) want |= 1u << k;
    CHECK(gx::low_mask32(cnt) == want, "cnt %d", cnt);
  }
  for (int cnt = 0; cnt <= 64; ++cnt) {
    uint64_t want = 0;
    for (int k = 0; k < cnt; ++k) want |= 1ull << k;
    CHECK(gx::low_mask64(cnt) == want, "cnt %d", cnt);
  }

  for (int pattern = 0; pattern < PATTERNS; ++pattern) {
    for (int64_t bit = 0; bit <= 95; ++bit) {
      for (int cnt = 1; cnt <= 32; ++cnt) {
        const auto m  = bitmap((bit + cnt + 31) / 32, pattern);  // ends at the word of the last requested bit
        uint32_t want = 0;
        for (int k = 0; k < cnt; ++k) want |= (bit_of(m.get(), bit + k) ? 1u : 0u) << k;
        const uint32_t got = gx::bits_from(m.get(), bit, cnt);
        CHECK(got == want, "bits_from pattern %d bit %lld cnt %d: %08x, want %08x", pattern, (long long)bit, cnt, got, want);
      }
      for (int span = 1; span <= 64; ++span) {
        const int64_t end = bit + span;
        const auto m      = bitmap((end - 1) / 32 + 1, pattern);  // ends at the word of end_bit - 1
        uint64_t want     = 0;
        for (int k = 0; k < span; ++k) want |= (uint64_t)(bit_of(m.get(), bit + k) ? 1u : 0u) << k;
        const uint64_t got = gx::bits_from64(m.get(), bit, end);
        CHECK(got == want, "bits_from64 pattern %d bit %lld span %d: %016llx, want %016llx", pattern, (long long)bit, span,
              (unsigned long long)got, (unsigned long long)want);
      }
      const auto m = bitmap(bit / 32 + 1, pattern);
      CHECK(gx::bit_is_set(m.get(), bit) == bit_of(m.get(), bit), "bit_is_set pattern %d bit %lld", pattern, (long long)bit);
      CHECK(gx::row_valid(m.get(), bit) == bit_of(m.get(), bit) && gx::row_valid(nullptr, bit), "row_valid bit %lld", (long long)bit);
    }
  }

  // every (begin, end) in a range of 4 words, empty ranges included, for the words in and around it
  for (int64_t begin = 0; begin <= 128; ++begin)
    for (int64_t end = begin; end <= 128; ++end)
      for (int64_t w = 0; w < 5; ++w) {
        uint32_t want = 0;
        for (int k = 0; k < 32; ++k)
          if (w * 32 + k >= begin && w * 32 + k < end) want |= 1u << k;
        const uint32_t got = gx::word_range_mask(w, begin, end);
        CHECK(got == want, "word_range_mask w %lld [%lld, %lld): %08x, want %08x", (long long)w, (long long)begin, (long long)end, got, want);
      }

  printf("gx_validity_tests: %d failed\n", failed);
  return failed ? 1 : 0;
}
