// A scripted driver over the two methods memex::HipFlatStore (include/memex_hip.hpp) got with grouped search with members (DESIGN.md
// 3.19): search_document_passages and search_spread.  tests/test_group_rows_store_gpu.py replays the same script on the Python mirror
// and compares the lines.
//
//   test_store_group_rows <workdir> <vectors.bin> <script.txt>     run the script; one output line per command
//
// vectors.bin: int32 dim, int32 count, then count x dim raw f32 -- a pool of vectors addressed by index.  Every score is printed as the
// 8 hex digits of its f32 bits: nothing passes through decimal text.
//
//   OPEN plain|sharded                          sharded: devices = {0, 0}
//   INSERT <_id>:<vec> ...                      ONE bulk_insert               REMOVE <_id> ...
//   GROUP <document> <_id> ...                  one grouping of the store: assign
//   PASSAGES <vec> <limit> <passages> <fetch>   fetch 0: the default
//   SPREAD <vec> <limit> <per_document> <fetch>
//
// Output: `R <line#> <complete> <n> ...`; per PASSAGES hit `<document or -> <members_complete> <m> <_id> <scorebits> ...`, per SPREAD hit
// `<document or -> <_id> <scorebits>`; the others print a count.  An exception prints `E <line#> <VectorStoreError kind or ->`.
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

static std::string bits_text(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    char buf[16];
    std::snprintf(buf, sizeof buf, "%08" PRIx32, b);
    return buf;
}
static const char *kind_name(VectorStoreError::Kind k) {
    static const char *names[] = {"ConnectionError", "DeleteError", "FileIOError", "InsertionError", "SearchError", "SerdeError", "SaveError",
                                  "Unsupported"};
    return names[(int)k];
}

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: test_store_group_rows <workdir> <vectors.bin> <script.txt>\n");
        return 2;
    }
    std::ifstream vf(argv[2], std::ios::binary);
    int32_t dim = 0, count = 0;
    vf.read(reinterpret_cast<char *>(&dim), 4);
    vf.read(reinterpret_cast<char *>(&count), 4);
    if (!vf || dim < 1 || count < 1) {
        std::fprintf(stderr, "bad vectors file\n");
        return 2;
    }
    std::vector<float> pool((size_t)dim * count);
    vf.read(reinterpret_cast<char *>(pool.data()), (std::streamsize)(pool.size() * 4));
    if (!vf) {
        std::fprintf(stderr, "short vectors file\n");
        return 2;
    }
    auto vec = [&](const std::string &t) {
        const size_t i = (size_t)std::stoul(t);
        if (i >= (size_t)count) throw std::invalid_argument("vector index");
        return std::vector<float>(pool.begin() + i * dim, pool.begin() + (i + 1) * dim);
    };
    std::ifstream sf(argv[3]);
    std::string ln;
    int no = 0;
    std::unique_ptr<HipFlatStore> st;
    std::unique_ptr<HipFlatStore::Grouping> grp;
    while (std::getline(sf, ln)) {
        ++no;
        std::istringstream is(ln);
        std::vector<std::string> a;
        for (std::string t; is >> t;) a.push_back(t);
        if (a.empty()) continue;
        const std::string op = a[0];
        a.erase(a.begin());
        try {
            std::string out;
            if (op == "OPEN") {
                st.reset(new HipFlatStore(std::string(argv[1]) + "/col", 0, a.at(0) == "sharded" ? std::vector<int>{0, 0} : std::vector<int>{}));
                out = " 0";
            } else if (op == "INSERT") {
                std::vector<VectorData> data;
                for (auto &t : a) {
                    const size_t c = t.find(':');
                    VectorData v;
                    v._id = t.substr(0, c);
                    v.document_id = "d";
                    v.vector = vec(t.substr(c + 1));
                    data.push_back(v);
                }
                st->bulk_insert(data);
                out = " " + std::to_string(data.size());
            } else if (op == "REMOVE") {
                out = " " + std::to_string(st->remove(a));
            } else if (op == "GROUP") {
                if (!grp) grp.reset(new HipFlatStore::Grouping(st->make_grouping()));
                grp->assign(a.at(0), std::vector<std::string>(a.begin() + 1, a.end()));
                out = " " + std::to_string(a.size() - 1);
            } else if ((op == "PASSAGES" || op == "SPREAD") && !grp) {
                throw std::invalid_argument("no grouping");
            } else if (op == "PASSAGES") {
                auto res = st->search_document_passages(vec(a.at(0)), std::stoul(a.at(1)), *grp, std::stoul(a.at(2)), std::stoul(a.at(3)));
                out = std::string(" ") + (res.second ? "1" : "0") + " " + std::to_string(res.first.size());
                for (auto &h : res.first) {
                    out += " " + (h.document ? *h.document : std::string("-")) + " " + (h.members_complete ? "1" : "0") + " " +
                           std::to_string(h.passages.size());
                    for (auto &p : h.passages) out += " " + p.first + " " + bits_text(p.second);
                }
            } else if (op == "SPREAD") {
                auto res = st->search_spread(vec(a.at(0)), std::stoul(a.at(1)), *grp, std::stoul(a.at(2)), std::stoul(a.at(3)));
                out = std::string(" ") + (res.second ? "1" : "0") + " " + std::to_string(res.first.size());
                for (auto &h : res.first) out += " " + (h.document ? *h.document : std::string("-")) + " " + h.segment + " " + bits_text(h.score);
            } else {
                throw std::invalid_argument("unknown command " + op);
            }
            std::printf("R %d%s\n", no, out.c_str());
        } catch (const VectorStoreError &e) {
            std::printf("E %d %s\n", no, kind_name(e.kind()));
        } catch (const std::exception &) {
            std::printf("E %d -\n", no);
        }
        std::fflush(stdout);
    }
    return 0;
}
