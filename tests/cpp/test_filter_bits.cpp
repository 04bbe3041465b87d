// The host mirror of a resident filter (memex_amd/csrc/mx_filter_bits.h) against a boolean model: range edits at every word edge,
// random edit sequences, and the export of runs over arbitrary windows.  Plain C++, no GPU; built with the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../memex_amd/csrc/mx_filter_bits.h"

using namespace mx;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);        \
            if (++fails > 20) exit(1);                                \
        }                                                             \
    } while (0)

static bool bit(const std::vector<uint64_t> &b, uint64_t r) { return (b[r >> 6] >> (r & 63)) & 1ull; }

static Ranges model_runs(const std::vector<char> &m, uint64_t lo, uint64_t hi, uint64_t first) {
    Ranges out;
    for (uint64_t r = lo; r < hi; ++r)
        if (m[r]) {
            if (!out.empty() && out.back().second == first + (r - lo)) out.back().second += 1;
            else out.emplace_back(first + (r - lo), first + (r - lo) + 1);
        }
    return out;
}

int main() {
    std::mt19937_64 rng(7);
    const uint64_t n = 20037, words = (n + 63) / 64;
    std::vector<uint64_t> bits(words, 0);
    std::vector<char> model(words * 64, 0);
    auto edit = [&](uint64_t a, uint64_t b, bool allow) {
        edit_mirror(bits, a, b, allow);
        for (uint64_t r = a; r < b && r < words * 64; ++r) model[r] = allow;
    };
    auto same = [&] {
        for (uint64_t r = 0; r < words * 64; ++r) CHECK(bit(bits, r) == (bool)model[r]);
        Ranges got;
        append_runs(bits, 0, n, 0, got);
        CHECK(got == model_runs(model, 0, n, 0));
    };
    // word edges
    for (uint64_t j : std::vector<uint64_t>{0, 1, 17, words - 2}) {
        for (auto ab : Ranges{{64 * j, 64 * j + 1}, {64 * j + 63, 64 * j + 65}, {64 * j + 1, 64 * j + 64}, {64 * j, 64 * j + 64},
                              {64 * j + 10, 64 * j + 20}, {64 * j + 5, 64 * j + 200}, {64 * j + 7, 64 * j + 7}}) {
            edit(ab.first, ab.second, true);
            same();
            edit(ab.first + 1, ab.second, false);
            same();
        }
    }
    edit(n - 5, n, true);                    // the last partial word
    same();
    edit(0, words * 64 + 1000, true);        // past the mirror: clipped to its words
    same();
    edit(0, words * 64, false);
    same();
    // random edit sequences, and runs over random windows with a global offset (what a sharded export asks for)
    for (int step = 0; step < 300; ++step) {
        const uint64_t a = rng() % n, len = step % 3 ? rng() % 200 : rng() % 5000;
        edit(a, std::min(a + len, n), rng() % 3 != 0);
        if (step % 10 == 0) same();
        const uint64_t lo = rng() % n, hi = lo + rng() % (n - lo + 1), first = rng() % 100000;
        Ranges got;
        append_runs(bits, lo, hi, first, got);
        CHECK(got == model_runs(model, lo, hi, first));
        // consecutive windows whose global rows are adjacent join their runs
        const uint64_t mid = lo + (hi - lo) / 2;
        Ranges two;
        append_runs(bits, lo, mid, first, two);
        append_runs(bits, mid, hi, first + (mid - lo), two);
        CHECK(two == got);
    }
    for (uint64_t r : std::vector<uint64_t>{0, 63, 64, n - 1}) {
        const uint64_t p = next_bit(bits, r, n, true), q = next_bit(bits, r, n, false);
        uint64_t wp = r, wq = r;
        while (wp < n && !model[wp]) ++wp;
        while (wq < n && model[wq]) ++wq;
        CHECK(p == wp && q == wq);
    }
    CHECK(next_bit(bits, n, n, true) == n);
    Ranges none;
    append_runs(bits, 500, 500, 0, none);
    append_runs(bits, 600, 500, 0, none);    // an empty window
    CHECK(none.empty());
    if (fails) return 1;
    printf("OK filter bits\n");
    return 0;
}
