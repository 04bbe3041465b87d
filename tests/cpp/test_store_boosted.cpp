// The C++ store mirror's boosted search (include/memex_hip.hpp: HipFlatStore::Prior, search_boosted, the VectorStorage forward) as a
// scripted driver: tests/test_boosted_store_gpu.py writes the vectors and the script, replays the same script on the Python mirror and
// compares the output lines -- _id strings, f32 and f64 bits.
//
//   test_store_boosted <workdir> <vectors.bin> <script.txt>
//   vectors.bin: int32 dim, int32 count, then count x dim f32.  Script lines (numbers are vector indices unless said otherwise):
//     INSERT first count per            rows first .. first + count - 1 under the _ids s<row>, documents d<row / per>
//     PRIOR                             make the prior
//     SET value_bits _id ...            one value for the named segments (set_document)
//     SETEACH _id:value_bits ...        one value per segment (set)
//     BOUND refresh                     -> the bound's bits
//     BOOST q limit weight_bits fetch   -> _id score prior combined ... and complete (fetch 0: the default)
//     VS_BOOST q limit weight_bits fetch   the same through a VectorStorage over the store
//     REMOVE _id ...
//     DELETE_ALL
//   Output: "R <line> <n> ..." per command, "E <line> <kind>" for an exception.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "memex_hip.hpp"

using namespace memex;

static float f32_of(const std::string &t) {
    const uint32_t b = (uint32_t)std::stoul(t, nullptr, 16);
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}
static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}
static uint64_t bits(double f) {
    uint64_t b;
    std::memcpy(&b, &f, sizeof b);
    return b;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <workdir> <vectors.bin> <script.txt>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    std::vector<std::vector<float>> pool;
    {
        std::ifstream f(argv[2], std::ios::binary);
        int32_t head[2] = {0, 0};
        if (!f.read((char *)head, sizeof head) || head[0] < 1 || head[1] < 0) return 2;
        pool.assign((size_t)head[1], std::vector<float>((size_t)head[0]));
        for (auto &v : pool)
            if (!f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(float)))) return 2;
    }
    std::shared_ptr<HipFlatStore> st = HipFlatStore::create(dir + "/col", 0, {});
    std::unique_ptr<HipFlatStore::Prior> prior;
    std::ifstream script(argv[3]);
    std::string ln;
    int no = 0;
    while (std::getline(script, ln)) {
        ++no;
        std::istringstream is(ln);
        std::string op, t;
        std::vector<std::string> a;
        is >> op;
        while (is >> t) a.push_back(t);
        try {
            if (op == "INSERT") {
                const size_t first = std::stoull(a[0]), count = std::stoull(a[1]), per = std::stoull(a[2]);
                std::vector<VectorData> data;
                for (size_t r = first; r < first + count; ++r)
                    data.push_back({"s" + std::to_string(r), "d" + std::to_string(r / per), "", pool.at(r), r % per});
                st->bulk_insert(data);
                std::printf("R %d 0\n", no);
            } else if (op == "PRIOR") {
                prior = std::make_unique<HipFlatStore::Prior>(st->make_prior());
                std::printf("R %d 0\n", no);
            } else if (op == "SET") {
                prior->set_document({a.begin() + 1, a.end()}, f32_of(a[0]));
                std::printf("R %d 0\n", no);
            } else if (op == "SETEACH") {
                std::vector<std::string> ids;
                std::vector<float> vals;
                for (auto &p : a) {
                    const size_t s = p.rfind(':');
                    ids.push_back(p.substr(0, s));
                    vals.push_back(f32_of(p.substr(s + 1)));
                }
                prior->set(ids, vals);
                std::printf("R %d 0\n", no);
            } else if (op == "BOUND") {
                std::printf("R %d 1 %08" PRIx32 "\n", no, bits(prior->bound(a[0] == "1")));
            } else if (op == "BOOST" || op == "VS_BOOST") {
                const std::vector<float> &q = pool.at(std::stoull(a[0]));
                const size_t limit = std::stoull(a[1]), fetch = std::stoull(a[3]);
                std::pair<std::vector<HipFlatStore::BoostedHit>, bool> r;
                if (op == "BOOST") {
                    r = st->search_boosted(q, limit, *prior, f32_of(a[2]), fetch);
                } else {
                    VectorStorage vs(st);  // (get_vector_storage would attach by a load, and a load makes the prior stale)
                    r = vs.search_boosted(q, limit, *prior, f32_of(a[2]), fetch);
                }
                std::printf("R %d %zu", no, r.first.size());
                for (auto &h : r.first)
                    std::printf(" %s %08" PRIx32 " %08" PRIx32 " %016" PRIx64, h._id.c_str(), bits(h.score), bits(h.prior), bits(h.combined));
                std::printf(" complete %d\n", r.second ? 1 : 0);
            } else if (op == "REMOVE") {
                std::printf("R %d 1 %08" PRIx32 "\n", no, (uint32_t)st->remove(a));
            } else if (op == "DELETE_ALL") {
                st->delete_all();
                std::printf("R %d 0\n", no);
            } else {
                std::fprintf(stderr, "line %d: unknown command %s\n", no, op.c_str());
                return 2;
            }
        } catch (const VectorStoreError &e) {
            std::printf("E %d VectorStoreError\n", no);
            std::fprintf(stderr, "line %d: %s\n", no, e.what());
        } catch (const std::exception &e) {
            std::printf("E %d other\n", no);
            std::fprintf(stderr, "line %d: %s\n", no, e.what());
        }
        std::fflush(stdout);
    }
    prior.reset();  // before its store
    return 0;
}
