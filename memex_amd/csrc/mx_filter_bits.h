// Host-side bit bookkeeping of a resident filter's mirror (mx_filter): plain C++, no GPU.  The mirror holds
// one allow bit per local row, bit r & 63 of word r >> 6.  tests/cpp/test_filter_bits.cpp holds it against a boolean model.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace mx {

using Ranges = std::vector<std::pair<uint64_t, uint64_t>>;  // half-open [lo, hi) ranges of ids or of rows

// the rows [a, b) of a host mirror join or leave the set
inline void edit_mirror(std::vector<uint64_t> &bits, uint64_t a, uint64_t b, bool allow) {
    for (uint64_t w = a >> 6; w * 64 < b && w < bits.size(); ++w) {
        const uint64_t lo = std::max(a, w * 64) - w * 64, hi = std::min(b, w * 64 + 64) - w * 64;
        const uint64_t sel = (hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
        if (allow) bits[w] |= sel;
        else bits[w] &= ~sel;
    }
}

// first position in [r, hi) whose bit equals `want`, or hi (hi <= 64 * bits.size())
inline uint64_t next_bit(const std::vector<uint64_t> &bits, uint64_t r, uint64_t hi, bool want) {
    while (r < hi) {
        uint64_t w = want ? bits[r >> 6] : ~bits[r >> 6];
        w &= ~0ull << (r & 63);
        if (w) return std::min<uint64_t>((r & ~63ull) + (uint64_t)__builtin_ctzll(w), hi);
        r = (r | 63ull) + 1;
    }
    return hi;
}

// the runs of set bits among the local rows [lo, hi) of a mirror, as global rows first + (r - lo), appended to out (adjacent runs join)
inline void append_runs(const std::vector<uint64_t> &bits, uint64_t lo, uint64_t hi, uint64_t first, Ranges &out) {
    hi = std::min<uint64_t>(hi, (uint64_t)bits.size() * 64);
    for (uint64_t r = lo < hi ? next_bit(bits, lo, hi, true) : hi; r < hi;) {
        const uint64_t e = next_bit(bits, r, hi, false);
        const uint64_t a = first + (r - lo), b = first + (e - lo);
        if (!out.empty() && out.back().second == a) out.back().second = b;
        else out.emplace_back(a, b);
        r = next_bit(bits, e, hi, true);
    }
}

// the n <= 64 bits of src from bit position s on, as the low bits of a word (s + n <= 64 * src.size())
inline uint64_t get_bits(const std::vector<uint64_t> &src, uint64_t s, unsigned n) {
    if (n == 0) return 0;
    const unsigned o = (unsigned)(s & 63);
    uint64_t v = src[s >> 6] >> o;
    if (o + n > 64) v |= src[(s >> 6) + 1] << (64 - o);  // (o > 0 here)
    return n == 64 ? v : v & ((1ull << n) - 1ull);
}

// the bits src[s, s + n) replace dst[d, d + n), at any two alignments (a selection over global rows dealt to a shard's local rows)
inline void copy_bits(std::vector<uint64_t> &dst, uint64_t d, const std::vector<uint64_t> &src, uint64_t s, uint64_t n) {
    while (n) {
        const unsigned o = (unsigned)(d & 63), take = (unsigned)std::min<uint64_t>(64 - o, n);
        const uint64_t m = (take == 64 ? ~0ull : (1ull << take) - 1ull) << o;
        dst[d >> 6] = (dst[d >> 6] & ~m) | (get_bits(src, s, take) << o);
        d += take;
        s += take;
        n -= take;
    }
}

// word w of the set "every row below size"
inline uint64_t rows_below_word(uint64_t size, uint64_t w) {
    return size >= (w + 1) * 64 ? ~0ull : size <= w * 64 ? 0ull : (1ull << (size - w * 64)) - 1ull;
}

// one word of mx_filter_combine: op 0 AND, 1 OR, 2 ANDNOT (x and not y), 3 XOR -- what filter_words_kernel computes
inline uint64_t combine_word(int op, uint64_t x, uint64_t y) { return op == 0 ? x & y : op == 1 ? x | y : op == 2 ? x & ~y : x ^ y; }

}  // namespace mx
