// memex::HipFlatStore::compact (include/memex_hip.hpp over mx_index_compact): removed rows are dropped for good, the id map is
// renumbered, the store is saved, and a cold load of a copy of its files finds the same _ids.  Built and run by
// tests/test_compact_cpp.py.  Exit code 0 = all passed.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <random>
#include <string>

#include "memex_hip.hpp"

using namespace memex;
namespace fs = std::filesystem;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string tmp = argv[1];
    fs::create_directories(tmp);
    const std::string dir = tmp + "/c";
    constexpr int kDim = 24, kRows = 300;
    std::mt19937 rng(7);
    std::normal_distribution<float> nd;
    std::vector<VectorData> data;
    for (int i = 0; i < kRows; ++i) {
        VectorData v{"doc-" + std::to_string(i), "doc-" + std::to_string(i), "", std::vector<float>(kDim), 0};
        for (auto &x : v.vector) x = nd(rng);
        data.push_back(v);
    }
    HipFlatStore store(dir);
    store.bulk_insert(data);
    CHECK(store.compact() == (size_t)kRows);  // nothing removed: a no-op
    CHECK(store._id_map.size() == (size_t)kRows && store._id_map.at(1) == "doc-0");
    std::vector<std::string> gone;
    for (int i = 0; i < kRows; i += 3) gone.push_back("doc-" + std::to_string(i));
    CHECK(store.remove(gone) == gone.size());
    const size_t live = (size_t)kRows - gone.size();
    CHECK(store.compact() == live);
    CHECK(store._id_map.size() == live && store.nb_point() == live);
    for (size_t i = 1; i <= live; ++i) {  // new id i: the i-th kept row, in insertion order
        const size_t old = (i - 1) / 2 * 3 + 1 + (i - 1) % 2;
        CHECK(store._id_map.at(i) == "doc-" + std::to_string(old));
    }
    // every kept row finds itself first, under its own _id
    for (int i = 1; i < kRows; i += 7) {
        if (i % 3 == 0) continue;
        auto r = store.search(data[i].vector, 1);
        CHECK(r.size() == 1 && r[0].first == data[i]._id);
    }
    auto gone_r = store.search(data[0].vector, (size_t)kRows);
    CHECK(gone_r.size() == live);
    for (auto &p : gone_r) CHECK(std::stoi(p.first.substr(4)) % 3 != 0);
    // the files on disk: a cold load of a copy finds the same _ids
    const std::string copy = tmp + "/copy";
    fs::create_directories(copy);
    for (auto &e : fs::directory_iterator(dir)) fs::copy_file(e.path(), copy + "/" + e.path().filename().string());
    auto loaded = HipFlatStore::load(copy);
    CHECK(loaded->_id_map == store._id_map);
    CHECK(loaded->nb_point() == live);
    for (int i = 1; i < kRows; i += 11) {
        if (i % 3 == 0) continue;
        auto a = loaded->search(data[i].vector, 5), b = store.search(data[i].vector, 5);
        CHECK(a == b && a[0].first == data[i]._id);
    }
    // inserts after a compaction continue at live + 1
    store.bulk_insert({{"late", "late", "", data[0].vector, 0}});
    CHECK(store._id_map.at(live + 1) == "late");
    CHECK(store.search(data[0].vector, 1)[0].first == "late");
    store.delete_all();
    loaded->delete_all();
    std::printf("OK compact store\n");
    return 0;
}
