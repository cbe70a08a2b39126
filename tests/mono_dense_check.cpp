// Host-only check of csrc/rs_mono_dense.hpp: when may a staged single-chunk encode run
// the column kernel's dense entry?  Compiled and run by tests/test_mono_dense_cpu.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "rs_mono_dense.hpp"

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("line %d: expected %s\n", __LINE__, #cond);         \
            ++failures;                                                \
        }                                                              \
    } while (0)

int main() {
    using rs::DenseRows;
    using rs::mono_dense_ok;
    const uint32_t kFull = 0xFFFFFFFFu;  // ShardFormat's default: shards of whole 64-byte blocks
    alignas(64) static uint8_t buf[256];
    const uint8_t *o = buf, *r = buf + 128;
    for (int L = 7; L <= 11; ++L) {
        const uint32_t n = 1u << L;
        for (uint64_t S : {uint64_t(64), uint64_t(128), uint64_t(1024)}) {
            // N = M = 2^L, S a multiple of 64, aligned: dense
            EXPECT(mono_dense_ok(L, 1, DenseRows{o, S, 0, n}, DenseRows{r, S, 0, n}, kFull, 0, 0));
            // a row stride larger than S, and a batch with aligned stripe strides
            EXPECT(mono_dense_ok(L, 1, DenseRows{o, S + 64, 0, n}, DenseRows{r, S + 4, 0, n}, kFull, 0, 0));
            EXPECT(mono_dense_ok(L, 1, DenseRows{o, S, 0, n}, DenseRows{r, S, 0, n}, kFull, 0, 0, (n + 3) * S, (n + 3) * S));
            // a base off by 2: the geometry asks for byte-wise access (io_bytes) -- and the
            // condition looks at the pointers itself
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o + 2, S, 0, n}, DenseRows{r, S, 0, n}, uint32_t(S / 64 * 8), 0, 1));
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o + 2, S, 0, n}, DenseRows{r, S, 0, n}, kFull, 0, 0));
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S, 0, n}, DenseRows{r + 2, S, 0, n}, kFull, 0, 0));
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S + 2, 0, n}, DenseRows{r, S, 0, n}, kFull, 0, 0));
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S, 0, n}, DenseRows{r, S, 0, n}, kFull, 0, 0, n * S + 2, n * S));
            // a narrowed recovery span [lo, hi)
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S, 0, n}, DenseRows{r, S, 10, n}, kFull, 0, 0));
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S, 0, n}, DenseRows{r, S, 0, n - 1}, kFull, 0, 0));
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S, 0, n}, DenseRows{r, S, 3, 40}, kFull, 0, 0));
            // N < 2^L: no prefix form, the general entry zero-fills
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S, 0, n - 1}, DenseRows{r, S, 0, n}, kFull, 0, 0));
            EXPECT(!mono_dense_ok(L, 1, DenseRows{o, S, 0, n / 2 + 1}, DenseRows{r, S, 0, n}, kFull, 0, 0));
            // two source maps
            EXPECT(!mono_dense_ok(L, 2, DenseRows{o, S, 0, n}, DenseRows{r, S, 0, n}, kFull, 0, 0));
        }
        // S = 66: one whole block and a tail pack
        EXPECT(!mono_dense_ok(L, 1, DenseRows{o, 66, 0, n}, DenseRows{r, 66, 0, n}, 8, 1, 0));
        EXPECT(!mono_dense_ok(L, 1, DenseRows{o, 68, 0, n}, DenseRows{r, 68, 0, n}, 8, 2, 0));
        // the 32-bit lane offsets: stride < 2^24 and 2^L rows of it within 2^32 bytes
        const uint64_t top = (uint64_t(1) << 32) >> L;
        const uint64_t ok = top < (uint64_t(1) << 24) ? top : (uint64_t(1) << 24) - 4;
        EXPECT(mono_dense_ok(L, 1, DenseRows{o, ok, 0, n}, DenseRows{r, ok, 0, n}, kFull, 0, 0));
        EXPECT(!mono_dense_ok(L, 1, DenseRows{o, top + 4, 0, n}, DenseRows{r, 64, 0, n}, kFull, 0, 0));
        EXPECT(!mono_dense_ok(L, 1, DenseRows{o, 64, 0, n}, DenseRows{r, top + 4, 0, n}, kFull, 0, 0));
        EXPECT(!mono_dense_ok(L, 1, DenseRows{o, uint64_t(1) << 24, 0, n}, DenseRows{r, 64, 0, n}, kFull, 0, 0));
    }
    // transform sizes without a dense instantiation
    EXPECT(!mono_dense_ok(6, 1, DenseRows{o, 64, 0, 64}, DenseRows{r, 64, 0, 64}, kFull, 0, 0));
    EXPECT(!mono_dense_ok(12, 1, DenseRows{o, 64, 0, 4096}, DenseRows{r, 64, 0, 4096}, kFull, 0, 0));
    if (failures) return 1;
    printf("mono dense ok\n");
    return 0;
}
