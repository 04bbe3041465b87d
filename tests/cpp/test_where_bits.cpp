// The host-side bit helpers the filters from row attributes added to memex_amd/csrc/mx_filter_bits.h against a
// boolean model: copy_bits at every pair of alignments (the dealing of a selection over global rows to a shard's local rows),
// rows_below_word (the pattern mx_filter_invert XORs with) and combine_word.  Plain C++, built with the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../memex_amd/csrc/mx_filter_bits.h"

using namespace mx;

static bool bit(const std::vector<uint64_t> &w, uint64_t r) { return (w[r >> 6] >> (r & 63)) & 1; }

int main() {
    std::mt19937_64 rng(18);
    const uint64_t words = 7, bits = words * 64;
    std::vector<uint64_t> src(words), dst(words), before;
    for (int round = 0; round < 40; ++round) {
        for (auto &w : src) w = rng();
        for (uint64_t s = 0; s < 130; s += (round % 3) + 1)
            for (uint64_t d = 0; d < 130; d += (round % 2) + 1)
                for (uint64_t n : {0ull, 1ull, 31ull, 32ull, 63ull, 64ull, 65ull, 96ull, 128ull, 200ull}) {
                    for (auto &w : dst) w = rng();
                    before = dst;
                    copy_bits(dst, d, src, s, n);
                    for (uint64_t r = 0; r < bits; ++r) {
                        const bool want = r >= d && r < d + n ? bit(src, s + (r - d)) : bit(before, r);
                        if (bit(dst, r) != want) {
                            std::printf("copy_bits(d = %llu, s = %llu, n = %llu): bit %llu\n", (unsigned long long)d, (unsigned long long)s,
                                        (unsigned long long)n, (unsigned long long)r);
                            return 1;
                        }
                    }
                }
    }
    // three shards, blocks of 96 rows, 1000 rows: dealing and reading back (filter_rows' mapping) is the identity
    const uint64_t G = 3, R = 96, total = 1000;
    std::vector<uint64_t> sel((total + 63) / 64);
    for (auto &w : sel) w = rng();
    sel.back() &= rows_below_word(total, sel.size() - 1);
    std::vector<std::vector<uint64_t>> loc(G, std::vector<uint64_t>(8, 0));
    for (uint64_t b = 0; b * R < total; ++b) copy_bits(loc[b % G], (b / G) * R, sel, b * R, std::min(R, total - b * R));
    std::vector<uint64_t> back(sel.size(), 0);
    for (uint64_t b = 0; b * R < total; ++b) copy_bits(back, b * R, loc[b % G], (b / G) * R, std::min(R, total - b * R));
    if (back != sel) {
        std::printf("dealing 1000 rows to 3 shards and back\n");
        return 1;
    }
    for (uint64_t size : {0ull, 1ull, 63ull, 64ull, 65ull, 128ull, 130ull})
        for (uint64_t w = 0; w < 4; ++w)
            for (uint64_t r = 0; r < 64; ++r)
                if ((bool)((rows_below_word(size, w) >> r) & 1) != (w * 64 + r < size)) {
                    std::printf("rows_below_word(%llu, %llu)\n", (unsigned long long)size, (unsigned long long)w);
                    return 1;
                }
    const uint64_t x = 0xF0F0F0F0AAAA5555ull, y = 0xFF00FF00CCCC3333ull;
    if (combine_word(0, x, y) != (x & y) || combine_word(1, x, y) != (x | y) || combine_word(2, x, y) != (x & ~y) ||
        combine_word(3, x, y) != (x ^ y)) {
        std::printf("combine_word\n");
        return 1;
    }
    std::printf("OK where bits\n");
    return 0;
}
