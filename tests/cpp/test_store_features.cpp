// A scripted driver over memex::HipFlatStore (include/memex_hip.hpp): every method the feature pull requests added to the C++ mirror,
// one command per method, so tests/test_cpp_store_features_gpu.py can hold the mirror to tests/cpp_store_model.py line by line.
//
//   test_store_features <workdir> <vectors.bin> <script.txt>     run the script; one output line per command
//   test_store_features --parse <script.txt>                     print the script in canonical form (no store, no GPU)
//
// vectors.bin: int32 dim, int32 count, then count x dim raw f32 -- a pool of vectors, rows and queries alike, addressed by index.
// A vector argument is `<index>` or `<index>/<len>` (the first len values: a query of another dimension), `-` where it may be absent.
// Every float argument is the 8 hex digits of its f32 bits and every score is printed that way: nothing passes through decimal text.
//
//   OPEN plain|sharded                          sharded: devices = {0, 0}
//   INSERT <_id>:<vec> ...                      ONE bulk_insert
//   REMOVE <_id> ... | COMPACT | SAVE | RELOAD | DELETE_ALL
//   SEARCH <vec> <limit>                        WITHIN <vec> <limit> <_id> ...
//   FILTER <name> <_id> ...                     ALLOW / DENY <name> <_id> ...     COUNT <name>     IN <vec> <limit> <name>
//   ABOVE <vec> <min_score> <limit>             DIVERSE <vec> <limit> <fetch> <lambda>           (fetch 0: the header's default)
//   FUSED max|rrf <limit> <fetch> <m> <vec> x m [<weight> x m]
//   MORE <_id> <limit>
//   LIKE <limit> <vec|-> default|<alpha> <beta> <gamma> + <_id> ... - <_id> ...                  (default: the header's parameters)
//   RERANK <vec> <limit> <_id> ...              DUPS <min_score> <per_row>
//   VS_LIKE / VS_RERANK                         the same through get_vector_storage(...).search_like / rerank
//
// Output: `R <line#> <n> <_id> <scorebits> ...`; counts are entries too (`removed`, `kept`, `rows`, `live`, 8 hex digits); DUPS prints
// `R <line#> <pairs> <a> <b> <scorebits> ... T <n> <_id> ...`.  An exception prints `E <line#> <class> <VectorStoreError kind or ->`.
// A Filter points at its store, so RELOAD keeps a store that still has filters alive beside the fresh one instead of destroying it.
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

struct Cmd {
    int line = 0;
    std::string op;
    std::vector<std::string> args;  // canonical tokens
};

static bool parse_uint(const std::string &s, uint64_t &v) {
    if (s.empty() || s.size() > 18) return false;
    v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + (uint64_t)(c - '0');
    }
    return true;
}
static bool parse_bits(const std::string &s, uint32_t &v) {
    if (s.size() != 8) return false;
    v = 0;
    for (char c : s) {
        int h = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (h < 0) return false;
        v = v << 4 | (uint32_t)h;
    }
    return true;
}
static float as_float(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t as_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static std::string hex8(uint32_t b) {
    char buf[16];
    std::snprintf(buf, sizeof buf, "%08x", b);
    return buf;
}

// canonical token of one argument kind; false: malformed
static bool canon_uint(const std::string &t, std::string &out) {
    uint64_t v;
    if (!parse_uint(t, v)) return false;
    out = std::to_string(v);
    return true;
}
static bool canon_bits(const std::string &t, std::string &out) {
    uint32_t v;
    if (!parse_bits(t, v)) return false;
    out = hex8(v);
    return true;
}
static bool canon_vec(const std::string &t, std::string &out, bool may_be_absent = false) {
    if (t == "-") {
        out = t;
        return may_be_absent;
    }
    const size_t s = t.find('/');
    std::string a, b;
    if (!canon_uint(t.substr(0, s), a)) return false;
    out = a;
    if (s != std::string::npos) {
        if (!canon_uint(t.substr(s + 1), b)) return false;
        out += "/" + b;
    }
    return true;
}
static bool canon_name(const std::string &t, std::string &out) {
    out = t;
    return !t.empty();
}

static bool parse_line(const std::vector<std::string> &tok, Cmd &c) {
    c.op = tok[0];
    c.args.clear();
    const size_t n = tok.size() - 1;
    auto arg = [&](size_t i) -> const std::string & { return tok[i + 1]; };
    std::string t;
    auto fixed = [&](const char *kinds, bool rest_names) {  // u uint, h bits, v vec, n name; then any number of names
        const size_t k = std::strlen(kinds);
        if (n < k || (!rest_names && n != k)) return false;
        for (size_t i = 0; i < k; ++i) {
            const bool ok = kinds[i] == 'u' ? canon_uint(arg(i), t) : kinds[i] == 'h' ? canon_bits(arg(i), t)
                          : kinds[i] == 'v' ? canon_vec(arg(i), t) : canon_name(arg(i), t);
            if (!ok) return false;
            c.args.push_back(t);
        }
        for (size_t i = k; i < n; ++i) c.args.push_back(arg(i));
        return true;
    };
    const std::string &op = c.op;
    if (op == "OPEN") return n == 1 && (arg(0) == "plain" || arg(0) == "sharded") && fixed("n", false);
    if (op == "INSERT") {
        if (n == 0) return false;
        for (size_t i = 0; i < n; ++i) {
            const size_t s = arg(i).rfind(':');
            if (s == std::string::npos || s == 0 || !canon_uint(arg(i).substr(s + 1), t)) return false;
            c.args.push_back(arg(i).substr(0, s) + ":" + t);
        }
        return true;
    }
    if (op == "COMPACT" || op == "SAVE" || op == "RELOAD" || op == "DELETE_ALL") return n == 0;
    if (op == "REMOVE") return n >= 1 && fixed("", true);
    if (op == "SEARCH") return fixed("vu", false);
    if (op == "WITHIN" || op == "RERANK" || op == "VS_RERANK") return fixed("vu", true);
    if (op == "FILTER" || op == "ALLOW" || op == "DENY") return fixed("n", true);
    if (op == "COUNT") return fixed("n", false);
    if (op == "IN") return fixed("vun", false);
    if (op == "ABOVE") return fixed("vhu", false);
    if (op == "DIVERSE") return fixed("vuuh", false);
    if (op == "MORE") return fixed("nu", false);
    if (op == "DUPS") return fixed("hu", false);
    if (op == "FUSED") {
        uint64_t m = 0;
        if (n < 4 || (arg(0) != "max" && arg(0) != "rrf") || !parse_uint(arg(3), m) || (n != 4 + m && n != 4 + 2 * m)) return false;
        c.args.push_back(arg(0));
        for (size_t i = 1; i < 4; ++i) {
            if (!canon_uint(arg(i), t)) return false;
            c.args.push_back(t);
        }
        for (size_t i = 4; i < n; ++i) {
            if (!(i < 4 + m ? canon_vec(arg(i), t) : canon_bits(arg(i), t))) return false;
            c.args.push_back(t);
        }
        return true;
    }
    if (op == "LIKE" || op == "VS_LIKE") {
        if (n < 3 || !canon_uint(arg(0), t)) return false;
        c.args.push_back(t);
        if (!canon_vec(arg(1), t, true)) return false;
        c.args.push_back(t);
        size_t i = 2;
        if (arg(i) == "default") {
            c.args.push_back(arg(i++));
        } else {
            for (int j = 0; j < 3; ++j, ++i) {
                if (i >= n || !canon_bits(arg(i), t)) return false;
                c.args.push_back(t);
            }
        }
        if (i >= n || arg(i) != "+") return false;
        bool minus = false;
        for (; i < n; ++i) {
            if (arg(i) == "-") {
                if (minus) return false;
                minus = true;
            }
            c.args.push_back(arg(i));
        }
        return minus;
    }
    return false;
}

static bool parse_script(const char *path, std::vector<Cmd> &out) {
    std::ifstream f(path);
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        return false;
    }
    std::string ln;
    for (int no = 1; std::getline(f, ln); ++no) {
        std::istringstream ss(ln);
        std::vector<std::string> tok;
        for (std::string t; ss >> t;) tok.push_back(t);
        if (tok.empty()) continue;
        Cmd c;
        c.line = no;
        if (!parse_line(tok, c)) {
            std::fprintf(stderr, "%s:%d: malformed command: %s\n", path, no, ln.c_str());
            return false;
        }
        out.push_back(c);
    }
    return true;
}

struct Driver {
    std::string dir;
    int dim = 0;
    std::vector<std::vector<float>> pool;
    std::vector<int> devices;
    std::shared_ptr<HipFlatStore> st;
    std::vector<std::shared_ptr<HipFlatStore>> kept_for_filters;
    std::map<std::string, std::unique_ptr<HipFlatStore::Filter>> filters;

    std::vector<float> vec(const std::string &t) const {
        if (t == "-") return {};
        const size_t s = t.find('/');
        const size_t i = (size_t)std::stoull(t.substr(0, s));
        if (i >= pool.size()) throw std::out_of_range("vector index " + t);
        std::vector<float> v = pool[i];
        if (s != std::string::npos) v.resize(std::min<size_t>(v.size(), (size_t)std::stoull(t.substr(s + 1))));
        return v;
    }
    static float f32(const std::string &t) {
        uint32_t b = 0;
        parse_bits(t, b);
        return as_float(b);
    }
    static size_t num(const std::string &t) { return (size_t)std::stoull(t); }
    static std::vector<std::string> names(const Cmd &c, size_t from) { return {c.args.begin() + (long)from, c.args.end()}; }
    HipFlatStore::Filter &filter(const std::string &name) {
        auto it = filters.find(name);
        if (it == filters.end()) throw std::out_of_range("no filter " + name);
        return *it->second;
    }

    static void print(const Cmd &c, const std::vector<VectorSearchResult> &r) {
        std::printf("R %d %zu", c.line, r.size());
        for (auto &e : r) std::printf(" %s %s", e.first.c_str(), hex8(as_bits(e.second)).c_str());
        std::printf("\n");
    }
    static void print_counts(const Cmd &c, std::vector<std::pair<const char *, uint64_t>> v) {
        std::printf("R %d %zu", c.line, v.size());
        for (auto &e : v) std::printf(" %s %s", e.first, hex8((uint32_t)e.second).c_str());
        std::printf("\n");
    }

    std::vector<VectorSearchResult> like(const Cmd &c, bool through_storage) {
        const size_t limit = num(c.args[0]);
        const std::vector<float> v = vec(c.args[1]);
        const bool dflt = c.args[2] == "default";
        size_t i = dflt ? 3 : 5;
        std::vector<std::string> pos, neg;
        bool minus = false;
        for (++i; i < c.args.size(); ++i) {  // (args[i] was "+")
            if (c.args[i] == "-") minus = true;
            else (minus ? neg : pos).push_back(c.args[i]);
        }
        if (through_storage) {
            VectorStorage vs = get_vector_storage("hip://" + dir, "col", 0, devices);
            return dflt ? vs.search_like(pos, neg, limit, v) : vs.search_like(pos, neg, limit, v, f32(c.args[2]), f32(c.args[3]), f32(c.args[4]));
        }
        return dflt ? st->search_like(pos, neg, limit, v) : st->search_like(pos, neg, limit, v, f32(c.args[2]), f32(c.args[3]), f32(c.args[4]));
    }

    void run(const Cmd &c) {
        const std::string &op = c.op;
        const auto &a = c.args;
        if (op == "OPEN") {
            devices = a[0] == "sharded" ? std::vector<int>{0, 0} : std::vector<int>{};
            st = HipFlatStore::create(dir + "/col", 0, devices);
            print(c, {});
        } else if (op == "INSERT") {
            std::vector<VectorData> data;
            for (auto &t : a) {
                const size_t s = t.rfind(':');
                data.push_back({t.substr(0, s), "doc", "", vec(t.substr(s + 1)), data.size()});
            }
            st->bulk_insert(data);
            print(c, {});
        } else if (op == "REMOVE") {
            print_counts(c, {{"removed", st->remove(names(c, 0))}});
        } else if (op == "COMPACT") {
            print_counts(c, {{"kept", st->compact()}});
        } else if (op == "SAVE") {
            st->save();
            print(c, {});
        } else if (op == "RELOAD") {
            HipFlatStore::evict_resident();
            if (!filters.empty()) kept_for_filters.push_back(st);
            st.reset();
            st = HipFlatStore::load(dir + "/col", 0, devices);
            print(c, {});
        } else if (op == "DELETE_ALL") {
            st->delete_all();
            print(c, {});
        } else if (op == "SEARCH") {
            print(c, st->search(vec(a[0]), num(a[1])));
        } else if (op == "WITHIN") {
            print(c, st->search_within(vec(a[0]), num(a[1]), names(c, 2)));
        } else if (op == "FILTER") {
            filters.erase(a[0]);
            filters[a[0]] = std::make_unique<HipFlatStore::Filter>(st->make_filter(names(c, 1)));
            print(c, {});
        } else if (op == "ALLOW") {
            filter(a[0]).allow(names(c, 1));
            print(c, {});
        } else if (op == "DENY") {
            filter(a[0]).deny(names(c, 1));
            print(c, {});
        } else if (op == "COUNT") {
            auto n = filter(a[0]).count();
            print_counts(c, {{"rows", n.first}, {"live", n.second}});
        } else if (op == "IN") {
            print(c, st->search_in(vec(a[0]), num(a[1]), filter(a[2])));
        } else if (op == "ABOVE") {
            print(c, st->search_above(vec(a[0]), f32(a[1]), num(a[2])));
        } else if (op == "DIVERSE") {
            print(c, st->search_diverse(vec(a[0]), num(a[1]), num(a[2]), f32(a[3])));
        } else if (op == "FUSED") {
            const size_t m = num(a[3]);
            std::vector<std::vector<float>> vecs;
            std::vector<float> w;
            for (size_t i = 0; i < m; ++i) vecs.push_back(vec(a[4 + i]));
            for (size_t i = 4 + m; i < a.size(); ++i) w.push_back(f32(a[i]));
            print(c, st->search_fused(vecs, num(a[1]), a[0] == "max" ? MX_FUSE_MAX : MX_FUSE_RRF, num(a[2]), w));
        } else if (op == "MORE") {
            print(c, st->more_like(a[0], num(a[1])));
        } else if (op == "LIKE" || op == "VS_LIKE") {
            print(c, like(c, op == "VS_LIKE"));
        } else if (op == "RERANK") {
            print(c, st->rerank(vec(a[0]), names(c, 2), num(a[1])));
        } else if (op == "VS_RERANK") {
            VectorStorage vs = get_vector_storage("hip://" + dir, "col", 0, devices);
            print(c, vs.rerank(vec(a[0]), names(c, 2), num(a[1])));
        } else if (op == "DUPS") {
            std::vector<std::string> cut;
            auto pairs = st->find_duplicates(f32(a[0]), num(a[1]), &cut);
            std::printf("R %d %zu", c.line, pairs.size());
            for (auto &p : pairs) std::printf(" %s %s %s", p.a.c_str(), p.b.c_str(), hex8(as_bits(p.score)).c_str());
            std::printf(" T %zu", cut.size());
            for (auto &t : cut) std::printf(" %s", t.c_str());
            std::printf("\n");
        }
    }
};

static const char *kind_name(VectorStoreError::Kind k) {
    static const char *names[] = {"ConnectionError", "DeleteError", "FileIOError", "InsertionError", "SearchError", "SerdeError", "SaveError", "Unsupported"};
    return names[(int)k];
}

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "--parse") {
        std::vector<Cmd> script;
        if (!parse_script(argv[2], script)) return 2;
        for (auto &c : script) {
            std::printf("%s", c.op.c_str());
            for (auto &t : c.args) std::printf(" %s", t.c_str());
            std::printf("\n");
        }
        return 0;
    }
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <workdir> <vectors.bin> <script.txt> | --parse <script.txt>\n", argv[0]);
        return 2;
    }
    Driver d;
    d.dir = argv[1];
    {
        std::ifstream f(argv[2], std::ios::binary);
        int32_t head[2] = {0, 0};
        if (!f.read((char *)head, sizeof head) || head[0] < 1 || head[1] < 0) {
            std::fprintf(stderr, "cannot read %s\n", argv[2]);
            return 2;
        }
        d.dim = head[0];
        d.pool.assign((size_t)head[1], std::vector<float>((size_t)head[0]));
        for (auto &v : d.pool)
            if (!f.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(float)))) {
                std::fprintf(stderr, "%s is short\n", argv[2]);
                return 2;
            }
    }
    std::vector<Cmd> script;
    if (!parse_script(argv[3], script)) return 2;
    for (auto &c : script) {
        try {
            if (!d.st && c.op != "OPEN") throw std::logic_error("no store: OPEN first");
            d.run(c);
        } catch (const VectorStoreError &e) {
            std::printf("E %d VectorStoreError %s\n", c.line, kind_name(e.kind()));
            std::fprintf(stderr, "line %d: %s\n", c.line, e.what());
        } catch (const std::invalid_argument &e) {
            std::printf("E %d std::invalid_argument -\n", c.line);
            std::fprintf(stderr, "line %d: %s\n", c.line, e.what());
        } catch (const std::exception &e) {
            std::printf("E %d other -\n", c.line);
            std::fprintf(stderr, "line %d: %s\n", c.line, e.what());
        }
        std::fflush(stdout);
    }
    d.filters.clear();  // before their stores
    return 0;
}
