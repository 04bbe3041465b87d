// A scripted driver over the filter methods memex::HipFlatStore (include/memex_hip.hpp) got with the filters from row attributes
// (DESIGN.md 3.18): Filter::allow_where / deny_where / allow_documents / deny_documents / invert and HipFlatStore::combine_filters.
// tests/test_cpp_store_where_gpu.py replays the same script on the Python mirror and compares the lines.
//
//   test_store_where <workdir> <vectors.bin> <script.txt>     run the script; one output line per command
//
// vectors.bin: int32 dim, int32 count, then count x dim raw f32 -- a pool of vectors addressed by index.  Every float argument is the
// 8 hex digits of its f32 bits and every score is printed that way: nothing passes through decimal text.
//
//   OPEN plain|sharded                          sharded: devices = {0, 0}
//   INSERT <_id>:<vec> ...                      ONE bulk_insert               REMOVE <_id> ...
//   PRIOR <value> <_id> ...                     one prior of the store: set_document
//   GROUP <document> <_id> ...                  one grouping of the store: assign
//   FILTER <name>                               a new empty filter
//   WHERE <name> allow|deny <lo> <hi>           -> n_selected                 DOCS <name> allow|deny <document> ...   -> n_selected
//   INVERT <name>                               COMBINE <out> <a> <b> <op 0..3 or more>; out = `+<name>`: a new filter
//   COUNT <name>                                -> allowed live               IN <vec> <limit> <name>
//
// Output: `R <line#> <n> <_id> <scorebits> ...` for IN, `R <line#> <number> ...` for the others; an exception prints
// `E <line#> <VectorStoreError kind or ->`.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "memex_hip.hpp"

using namespace memex;

static float as_float(const std::string &s) {
    const uint32_t b = (uint32_t)std::stoul(s, nullptr, 16);
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t as_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static const char *kind_name(VectorStoreError::Kind k) {
    static const char *names[] = {"ConnectionError", "DeleteError", "FileIOError", "InsertionError", "SearchError", "SerdeError", "SaveError",
                                  "Unsupported"};
    return names[(int)k];
}

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: test_store_where <workdir> <vectors.bin> <script.txt>\n");
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
    std::unique_ptr<HipFlatStore::Prior> pri;
    std::unique_ptr<HipFlatStore::Grouping> grp;
    std::map<std::string, std::unique_ptr<HipFlatStore::Filter>> filters;
    auto flt = [&](const std::string &name) -> HipFlatStore::Filter & {
        auto it = filters.find(name);
        if (it == filters.end()) throw std::invalid_argument("no filter " + name);
        return *it->second;
    };
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
            } else if (op == "PRIOR") {
                if (!pri) pri.reset(new HipFlatStore::Prior(st->make_prior()));
                pri->set_document(std::vector<std::string>(a.begin() + 1, a.end()), as_float(a.at(0)));
                out = " " + std::to_string(a.size() - 1);
            } else if (op == "GROUP") {
                if (!grp) grp.reset(new HipFlatStore::Grouping(st->make_grouping()));
                grp->assign(a.at(0), std::vector<std::string>(a.begin() + 1, a.end()));
                out = " " + std::to_string(a.size() - 1);
            } else if (op == "FILTER") {
                filters[a.at(0)].reset(new HipFlatStore::Filter(st->make_filter({})));
                out = " 0";
            } else if (op == "WHERE") {
                HipFlatStore::Filter &f = flt(a.at(0));
                const float lo = as_float(a.at(2)), hi = as_float(a.at(3));
                out = " " + std::to_string(a.at(1) == "allow" ? f.allow_where(*pri, lo, hi) : f.deny_where(*pri, lo, hi));
            } else if (op == "DOCS") {
                HipFlatStore::Filter &f = flt(a.at(0));
                const std::vector<std::string> docs(a.begin() + 2, a.end());
                out = " " + std::to_string(a.at(1) == "allow" ? f.allow_documents(*grp, docs) : f.deny_documents(*grp, docs));
            } else if (op == "INVERT") {
                flt(a.at(0)).invert();
                out = " 0";
            } else if (op == "COMBINE") {
                const int code = std::stoi(a.at(3));
                if (a.at(0)[0] == '+') {
                    HipFlatStore::Filter made = st->combine_filters(flt(a.at(1)), flt(a.at(2)), code);
                    filters[a.at(0).substr(1)].reset(new HipFlatStore::Filter(std::move(made)));
                } else {
                    st->combine_filters(flt(a.at(1)), flt(a.at(2)), code, flt(a.at(0)));
                }
                out = " 0";
            } else if (op == "COUNT") {
                const auto c = flt(a.at(0)).count();
                out = " " + std::to_string(c.first) + " " + std::to_string(c.second);
            } else if (op == "IN") {
                const auto res = st->search_in(vec(a.at(0)), (size_t)std::stoul(a.at(1)), flt(a.at(2)));
                out = " " + std::to_string(res.size());
                char buf[16];
                for (auto &r : res) {
                    std::snprintf(buf, sizeof buf, "%08x", as_bits(r.second));
                    out += " " + r.first + " " + buf;
                }
            } else {
                std::fprintf(stderr, "line %d: unknown command %s\n", no, op.c_str());
                return 2;
            }
            std::printf("R %d%s\n", no, out.c_str());
        } catch (const VectorStoreError &e) {
            std::printf("E %d %s\n", no, kind_name(e.kind()));
        } catch (const std::exception &e) {
            std::printf("E %d -\n", no);
        }
    }
    filters.clear();  // the handles before the store they point at
    grp.reset();
    pri.reset();
    if (st) st->delete_all();
    return 0;
}
