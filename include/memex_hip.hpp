// memex_hip.hpp -- header-only C++17 host mirror of memex's Rust surface over the C ABI
// (memex_hip.h).  The reference is compiled code (Rust); with no Rust toolchain in the build image
// this is the host side a compiled caller links against, with the reference's names, argument
// meaning and error behaviour:
//
//   reference (lib/libmemex/src)                         here (namespace memex)
//   storage/mod.rs:17-28   VectorData                    VectorData
//   storage/mod.rs:31-48   VectorStoreError (8 variants) VectorStoreError{kind(), what()}
//   storage/mod.rs:55-66   trait VectorStore             class VectorStore (abstract)
//   storage/local.rs:21-166 HnswStore                    class HipFlatStore (exact GPU search)
//   storage/mod.rs:69-93   VectorStorage (Arc<Mutex<..>>) class VectorStorage
//   storage/mod.rs:95-139  get_vector_storage            get_vector_storage (hnsw:// and hip://)
//   llm/embedding.rs:11-22 EmbeddingError / Result       EmbeddingError, EmbeddingResult
//   llm/embedding.rs:58-73 ModelConfig                   ModelConfig (L12-v2, 256, 86)
//   llm/embedding.rs:78-152 SentenceEmbedder             SentenceEmbedder::spawn/encode/encode_single
//   llm/embedding.rs:155-198 segment_text                segment_text (native Tokenizer; a whitespace stand-in without one)
//   llm/embedding.rs:163-195 tokenizers crate calls      Tokenizer (mx_tokenizer_*: WordPiece / byte-level BPE)
//   worker/tasks.rs:9-66    process_embeddings           process_embeddings (+ uuid5 / document_uuid / segment_uuid)
//   api/.../handlers.rs:55-109 handle_search_docs        search_docs
//
// The reference's async fns are blocking calls here (the C ABI is synchronous); the Rust shim in
// INTEGRATION.md wraps them in `async fn` again.
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <condition_variable>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <fstream>
#include <functional>
#include <future>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "memex_hip.h"

namespace memex {

// ---- storage/mod.rs -----------------------------------------------------------------------------
struct VectorData {  // mod.rs:17-28
    std::string _id, document_id, text;
    std::vector<float> vector;
    size_t segment_id = 0;
};

class VectorStoreError : public std::runtime_error {  // mod.rs:31-48
  public:
    enum Kind { ConnectionError, DeleteError, FileIOError, InsertionError, SearchError, SerdeError, SaveError, Unsupported };
    VectorStoreError(Kind k, const std::string &m) : std::runtime_error(m), kind_(k) {}
    Kind kind() const { return kind_; }

  private:
    Kind kind_;
};

inline VectorStoreError from_status(int rc, VectorStoreError::Kind dflt) {
    const std::string msg = mx_last_error() ? mx_last_error() : "";
    switch (rc) {
        case MX_EDEVICE: return {VectorStoreError::ConnectionError, msg};
        case MX_ESEARCH: return {VectorStoreError::SearchError, msg};
        case MX_EIO: return {VectorStoreError::FileIOError, msg};
        case MX_EUNSUPPORTED: return {VectorStoreError::Unsupported, msg};
        default: return {dflt, msg};
    }
}

using VectorSearchResult = std::pair<std::string, float>;  // (doc_id, score), mod.rs:51

class VectorStore {  // mod.rs:55-66
  public:
    virtual ~VectorStore() = default;
    virtual void delete_(const std::string &id) = 0;
    virtual void delete_all() = 0;
    virtual void bulk_insert(const std::vector<VectorData> &data) = 0;
    virtual void insert(const VectorData &data) = 0;
    virtual std::vector<VectorSearchResult> search(const std::vector<float> &vec, size_t limit) = 0;
    // relevance feedback over stored segments (no counterpart in the trait): a store that cannot reach its rows by _id refuses
    virtual std::vector<VectorSearchResult> search_like(const std::vector<std::string> &, const std::vector<std::string> &, size_t,
                                                        const std::vector<float> &, float, float, float) {
        throw VectorStoreError(VectorStoreError::Unsupported, "search_like");
    }
    // exact scores and ranking of named segments (no counterpart in the trait either); limit 0: all of them
    virtual std::vector<VectorSearchResult> rerank(const std::vector<float> &, const std::vector<std::string> &, size_t) {
        throw VectorStoreError(VectorStoreError::Unsupported, "rerank");
    }
};

// ---- storage/local.rs ---------------------------------------------------------------------------
constexpr const char *META_FILE = "vectors.meta.json";  // local.rs:19

class HipFlatStore : public VectorStore {
  public:
    std::string storage_path;
    std::map<size_t, std::string> _id_map;  // local.rs:24 (usize -> _id)

    // devices: empty = one index on `device`; several ordinals = the in-library sharded index
    // (mx_index_open_sharded: rows dealt to the GPUs in blocks, one exchange + merge per search)
    explicit HipFlatStore(const std::string &path, int device = 0, std::vector<int> devices = {})
        : storage_path(path), device_(device), devices_(std::move(devices)) {}  // ::new, local.rs:95
    ~HipFlatStore() override {
        if (idx_) mx_index_close(idx_);
    }
    HipFlatStore(const HipFlatStore &) = delete;
    HipFlatStore &operator=(const HipFlatStore &) = delete;

    // Process-wide registry of resident stores keyed by storage path.  The reference builds a store
    // per request / per task (handlers.rs:61-63, worker/lib.rs:190) and reloads the index each time
    // (storage/mod.rs:115-116); here every handle on a collection shares ONE store object -- GPU index
    // AND id map -- as long as the files it last wrote / read are unchanged on disk.
    static std::map<std::string, std::shared_ptr<HipFlatStore>> &registry() {
        static std::map<std::string, std::shared_ptr<HipFlatStore>> r;
        return r;
    }
    static std::mutex &registry_mu() {
        static std::mutex m;
        return m;
    }
    static void evict_resident() {
        std::lock_guard<std::mutex> lk(registry_mu());
        registry().clear();
    }
    static std::shared_ptr<HipFlatStore> create(const std::string &path, int device = 0, std::vector<int> devices = {}) {
        auto st = std::make_shared<HipFlatStore>(path, device, std::move(devices));
        std::lock_guard<std::mutex> lk(registry_mu());
        registry()[path] = st;
        return st;
    }

    static bool has_store(const std::string &path) {  // local.rs:110-113
        struct stat sb;
        return stat((path + "/" + META_FILE).c_str(), &sb) == 0;
    }

    static std::shared_ptr<HipFlatStore> load(const std::string &path, int device = 0, std::vector<int> devices = {}) {  // local.rs:115-141
        {   // resident and unchanged on disk: attach in O(1) (mx_index_load is O(1) too in that case)
            std::lock_guard<std::mutex> lk(registry_mu());
            auto it = registry().find(path);
            if (it != registry().end()) {
                auto &st = it->second;
                std::lock_guard<std::mutex> l2(st->mu_);
                if (st->meta_known_ && file_sig(path + "/" + META_FILE) == st->meta_sig_ && st->_id_map.size() == st->meta_ids_) {
                    if (st->_id_map.empty()) return st;
                    if (st->idx_ && mx_index_load(st->idx_, path.c_str()) == MX_OK && st->nb_point() == st->_id_map.size()) return st;
                }
            }
        }
        std::ifstream f(path + "/" + META_FILE);
        if (!f) throw VectorStoreError(VectorStoreError::FileIOError, "cannot open " + path + "/" + META_FILE);
        std::stringstream ss;
        ss << f.rdbuf();
        auto store = std::make_shared<HipFlatStore>(path, device, std::move(devices));
        store->_id_map = parse_id_map(ss.str());
        store->meta_sig_ = file_sig(path + "/" + META_FILE);
        store->meta_ids_ = store->_id_map.size();
        store->meta_known_ = true;
        if (!store->_id_map.empty()) {
            int dim = 0;
            uint64_t n = 0;
            int rc = mx_index_store_info(path.c_str(), &dim, &n);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::FileIOError);
            store->open(dim);
            rc = mx_index_load(store->idx_, path.c_str());
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::FileIOError);
            if (n != store->_id_map.size()) throw VectorStoreError(VectorStoreError::FileIOError, "vector / id count mismatch");
        }
        std::lock_guard<std::mutex> lk(registry_mu());
        registry()[path] = store;
        return store;
    }

    // local.rs:143-165.  The reference calls this after EVERY insert (local.rs:67) and rewrites both
    // files; a save into the store's own directory appends instead: mx_index_save adds the new rows to
    // vectors.mxflat, and the new "id":"_id" pairs are spliced in before the JSON object's closing brace.
    void save(const std::string &path_in = "") {
        std::lock_guard<std::mutex> lk(mu_);
        const std::string path = path_in.empty() ? storage_path : path_in;
        make_dirs(path);
        if (idx_) {
            int rc = mx_index_save(idx_, path.c_str());
            if (rc != MX_OK) throw VectorStoreError(VectorStoreError::SaveError, mx_last_error());
        }
        const std::string meta = path + "/" + META_FILE;
        const bool own = path == storage_path;
        const size_t n = _id_map.size();
        bool appended = false;
        if (own && meta_known_ && file_sig(meta) == meta_sig_ && meta_ids_ > 0 && meta_ids_ <= n) {
            appended = meta_ids_ == n;
            if (!appended) {
                std::fstream f(meta, std::ios::in | std::ios::out | std::ios::binary);
                char last = 0;
                if (f && f.seekg(-1, std::ios::end) && f.get(last) && last == '}') {  // the file ends the way this store left it
                    f.seekp(-1, std::ios::end);                                        // over the closing brace
                    for (size_t i = meta_ids_ + 1; i <= n; ++i) f << ",\"" << i << "\":\"" << escape(_id_map[i]) << "\"";
                    f << "}";
                    f.flush();
                    appended = (bool)f;
                }
            }
        }
        if (!appended) {
            // full rewrite through a temporary file: the vectors are already on disk, the id map must never be
            // left shorter than them (also the way out of a file the splice does not recognise)
            meta_known_ = false;
            const std::string tmp = meta + ".tmp";
            {
                std::ofstream f(tmp);
                if (!f) throw VectorStoreError(VectorStoreError::FileIOError, "cannot write " + tmp);
                f << "{";
                bool first = true;
                for (auto &kv : _id_map) {
                    f << (first ? "" : ",") << "\"" << kv.first << "\":\"" << escape(kv.second) << "\"";
                    first = false;
                }
                f << "}";
                f.flush();
                if (!f) throw VectorStoreError(VectorStoreError::FileIOError, "cannot write " + tmp);
            }
            if (std::rename(tmp.c_str(), meta.c_str()) != 0) throw VectorStoreError(VectorStoreError::FileIOError, "cannot replace " + meta);
        }
        if (own) {
            meta_sig_ = file_sig(meta);
            meta_ids_ = n;
            meta_known_ = true;
        }
    }

    void delete_(const std::string &) override {  // local.rs:29-32: unimplemented!()
        throw std::logic_error("Currently removing a single point is not supported");
    }

    void delete_all() override {  // local.rs:34-53
        std::remove((storage_path + "/" + META_FILE).c_str());
        if (mx_index_remove_files(storage_path.c_str()) != MX_OK) throw VectorStoreError(VectorStoreError::DeleteError, mx_last_error());
        if (idx_ && mx_index_clear(idx_) != MX_OK) throw VectorStoreError(VectorStoreError::DeleteError, mx_last_error());
        _id_map.clear();
        rows_of_.clear();
        rows_of_built_ = false;
        meta_known_ = false;
        meta_ids_ = 0;
    }

    // Remove every row whose _id is in `ids` (rows inserted twice under one _id all go) -- what delete_ (local.rs:29-32,
    // unimplemented!()) lacks.  Tombstones (mx_index_remove): ids stay stable, vectors.meta.json is unchanged, the removals are
    // saved beside the store (vectors.mxdead) before this returns.  An unknown _id removes nothing.  -> rows newly removed.
    size_t remove(const std::vector<std::string> &ids) {
        std::vector<uint64_t> rows;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || _id_map.empty()) return 0;
            if (!rows_of_built_) {  // once per store: later calls look their _ids up
                for (auto &kv : _id_map) rows_of_[kv.second].push_back(kv.first);
                rows_of_built_ = true;
            }
            std::set<std::string> seen;
            for (auto &id : ids) {
                if (!seen.insert(id).second) continue;
                auto it = rows_of_.find(id);
                if (it != rows_of_.end()) rows.insert(rows.end(), it->second.begin(), it->second.end());
            }
        }
        if (rows.empty()) return 0;
        uint64_t n = 0;
        if (mx_index_remove(idx_, rows.data(), rows.size(), &n) != MX_OK) throw VectorStoreError(VectorStoreError::DeleteError, mx_last_error());
        try {
            save();
        } catch (const VectorStoreError &e) {
            throw VectorStoreError(VectorStoreError::DeleteError, e.what());
        }
        return (size_t)n;
    }
    size_t remove(const std::string &id) { return remove(std::vector<std::string>{id}); }

    // Drop the rows remove() took out for good (mx_index_compact): the live rows get dense ids again and _id_map is renumbered
    // to match.  Saved before this returns: vectors.mxflat is rewritten whole, then vectors.meta.json through a temporary file; a
    // crash between the two leaves more ids than vectors, which load() rejects (FileIOError), never a wrong id -> _id mapping.
    // Nothing removed: a no-op.  -> rows kept.
    size_t compact() {
        uint64_t n_live = 0;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || _id_map.empty()) return 0;
            uint64_t size = 0, removed = 0;
            if (mx_index_size(idx_, &size) != MX_OK || mx_index_removed(idx_, &removed) != MX_OK)
                throw VectorStoreError(VectorStoreError::DeleteError, mx_last_error());
            if (removed == 0) return (size_t)size;
            std::vector<uint64_t> kept((size_t)(size - removed));
            if (mx_index_compact(idx_, kept.data(), kept.size(), &n_live) != MX_OK)
                throw VectorStoreError(VectorStoreError::DeleteError, mx_last_error());
            std::map<size_t, std::string> renumbered;
            for (size_t i = 0; i < (size_t)n_live; ++i) renumbered[i + 1] = _id_map.at((size_t)kept[i]);
            _id_map.swap(renumbered);
            rows_of_.clear();
            rows_of_built_ = false;
            meta_known_ = false;  // the id map is rewritten whole, never appended to
            meta_ids_ = 0;
        }
        try {
            save();
        } catch (const VectorStoreError &e) {
            throw VectorStoreError(VectorStoreError::DeleteError, e.what());
        }
        return (size_t)n_live;
    }

    // local.rs:55-69 semantics (ids in order, store persisted before returning), one transfer and
    // one incremental save instead of a save per vector
    void bulk_insert(const std::vector<VectorData> &data) override {
        if (data.empty()) return;
        const size_t d = data[0].vector.size();
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_) {
                open((int)d);
                if (nb_point() != _id_map.size()) mx_index_clear(idx_);  // a stale resident index under this key
            }
        }
        std::vector<float> flat;
        flat.reserve(data.size() * d);
        for (auto &v : data) {
            if (v.vector.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::InsertionError, "vector dimension mismatch");
            flat.insert(flat.end(), v.vector.begin(), v.vector.end());
        }
        uint64_t first = 0;
        int rc = mx_index_add(idx_, flat.data(), data.size(), &first);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::InsertionError);
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t i = 0; i < data.size(); ++i) {
                _id_map[(size_t)first + i] = data[i]._id;  // next_id = len + 1 (local.rs:63)
                if (rows_of_built_) rows_of_[data[i]._id].push_back((size_t)first + i);
            }
        }
        try {
            save();  // local.rs:67 `let _ = self.save(..)`: errors are ignored there too
        } catch (const VectorStoreError &) {
        }
    }

    void insert(const VectorData &data) override { bulk_insert({data}); }  // local.rs:62-69

    std::vector<VectorSearchResult> search(const std::vector<float> &vec, size_t limit) override {  // local.rs:71-91
        std::vector<VectorSearchResult> out;
        if (!idx_ || limit == 0) return out;
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        std::vector<uint64_t> ids(limit);
        std::vector<float> scores(limit);
        int32_t nf = 0;
        int rc = mx_index_search(idx_, vec.data(), 1, (int)limit, ids.data(), scores.data(), nullptr, &nf);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)ids[j]);
            if (it == _id_map.end())  // local.rs:80-83 panics; we raise
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, scores[j]);
        }
        return out;
    }

    // search() restricted to the rows inserted under the given _id strings (mx_index_search_filtered): the _ids go through the map
    // remove() builds, their ids into sorted runs (a document's segments are inserted in one call: one run per document).  An
    // unknown _id selects nothing; nothing selected -> no results.
    std::vector<VectorSearchResult> search_within(const std::vector<float> &vec, size_t limit, const std::vector<std::string> &ids) {
        std::vector<VectorSearchResult> out;
        std::vector<uint64_t> rows;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0 || _id_map.empty()) return out;
            if (!rows_of_built_) {
                for (auto &kv : _id_map) rows_of_[kv.second].push_back(kv.first);
                rows_of_built_ = true;
            }
            std::set<std::string> seen;
            for (auto &id : ids) {
                if (!seen.insert(id).second) continue;
                auto it = rows_of_.find(id);
                if (it != rows_of_.end()) rows.insert(rows.end(), it->second.begin(), it->second.end());
            }
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        std::sort(rows.begin(), rows.end());
        std::vector<uint64_t> ranges;  // [lo, hi) pairs of consecutive ids
        for (size_t i = 0; i < rows.size();) {
            size_t j = i + 1;
            while (j < rows.size() && rows[j] <= rows[j - 1] + 1) ++j;
            ranges.push_back(rows[i]);
            ranges.push_back(rows[j - 1] + 1);
            i = j;
        }
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        int32_t nf = 0;
        int rc = mx_index_search_filtered(idx_, vec.data(), 1, (int)limit, ranges.empty() ? nullptr : ranges.data(), ranges.size() / 2,
                                          found.data(), scores.data(), nullptr, &nf);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, scores[j]);
        }
        return out;
    }

    // A resident filter (mx_filter): the rows inserted under some _id strings -- one tenant's, one ACL group's, one tag's documents --
    // kept as a bitmap next to the rows and named in search_in().  bulk_insert of a document, then allow({its _ids}), is the
    // tenant-ingest flow.  After compact(), delete_all() or a reload every call but the destructor throws: make a new one.
    class Grouping;
    class Prior;
    class Filter {
      public:
        Filter(const Filter &) = delete;
        Filter &operator=(const Filter &) = delete;
        Filter(Filter &&o) noexcept : store_(o.store_), f_(o.f_) { o.f_ = nullptr; }
        ~Filter() {
            if (f_) mx_filter_destroy(f_);
        }
        void allow(const std::vector<std::string> &ids) { edit(ids, 1); }
        void deny(const std::vector<std::string> &ids) { edit(ids, 0); }
        // the rows whose value in `prior` lies in [lo, hi] join / leave the set (mx_filter_set_where): the device decides, the host
        // needs no copy of the values; rows nobody set read 0.  -> rows selected
        uint64_t allow_where(const Prior &prior, float lo = -INFINITY, float hi = INFINITY) { return where(prior, lo, hi, 1); }
        uint64_t deny_where(const Prior &prior, float lo = -INFINITY, float hi = INFINITY) { return where(prior, lo, hi, 0); }
        // every segment `grouping` holds under one of the document names joins / leaves the set (mx_filter_set_keys); unknown names
        // add nothing and no key is handed out for them.  -> rows selected
        uint64_t allow_documents(const Grouping &grouping, const std::vector<std::string> &documents) { return keys(grouping, documents, 1); }
        uint64_t deny_documents(const Grouping &grouping, const std::vector<std::string> &documents) { return keys(grouping, documents, 0); }
        // the complement within the rows the store holds at this moment (mx_filter_invert)
        void invert() {
            int rc = mx_filter_invert(f_);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        }
        // rows in the set, and those of them that are not removed
        std::pair<uint64_t, uint64_t> count() const {
            uint64_t a = 0, l = 0;
            int rc = mx_filter_count(f_, &a, &l);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            return {a, l};
        }

      private:
        friend class HipFlatStore;
        Filter(HipFlatStore *store, mx_filter *f) : store_(store), f_(f) {}
        uint64_t where(const Prior &prior, float lo, float hi, int allow) {
            uint64_t n = 0;
            int rc = mx_filter_set_where(f_, prior.p_, lo, hi, allow, &n);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            return n;
        }
        uint64_t keys(const Grouping &grouping, const std::vector<std::string> &documents, int allow) {
            std::vector<uint32_t> ks;
            {
                std::lock_guard<std::mutex> lk(store_->mu_);
                for (auto &d : documents) {
                    auto it = grouping.key_of_.find(d);
                    if (it != grouping.key_of_.end()) ks.push_back(it->second);
                }
            }
            uint64_t n = 0;
            int rc = mx_filter_set_keys(f_, grouping.g_, ks.empty() ? nullptr : ks.data(), ks.size(), allow, &n);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            return n;
        }
        void edit(const std::vector<std::string> &ids, int allow) {
            std::lock_guard<std::mutex> lk(store_->mu_);
            if (!store_->rows_of_built_) {
                for (auto &kv : store_->_id_map) store_->rows_of_[kv.second].push_back(kv.first);
                store_->rows_of_built_ = true;
            }
            std::vector<uint64_t> rows;
            for (auto &id : ids) {
                auto it = store_->rows_of_.find(id);
                if (it != store_->rows_of_.end()) rows.insert(rows.end(), it->second.begin(), it->second.end());
            }
            int rc = mx_filter_set_ids(f_, rows.empty() ? nullptr : rows.data(), rows.size(), allow);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        }
        HipFlatStore *store_;
        mx_filter *f_;
    };

    Filter make_filter(const std::vector<std::string> &ids) {
        mx_filter *f = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_) throw VectorStoreError(VectorStoreError::SearchError, "a filter needs a store with rows: insert first");
            int rc = mx_filter_create(idx_, &f);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        }
        Filter out(this, f);
        out.allow(ids);
        return out;
    }

    // out = a op b over the rows (mx_filter_combine), op one of MX_FILTER_AND, MX_FILTER_OR, MX_FILTER_ANDNOT (a and not b), MX_FILTER_XOR;
    // out may be a or b.  The three-argument form makes a new filter
    void combine_filters(const Filter &a, const Filter &b, int op, Filter &out) {
        int rc = mx_filter_combine(out.f_, a.f_, b.f_, op);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
    }
    Filter combine_filters(const Filter &a, const Filter &b, int op) {
        Filter out = make_filter({});
        combine_filters(a, b, op, out);
        return out;
    }

    // search() restricted to the rows of a resident filter (mx_index_search_with_filter)
    std::vector<VectorSearchResult> search_in(const std::vector<float> &vec, size_t limit, const Filter &flt) {
        std::vector<VectorSearchResult> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0) return out;
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        int32_t nf = 0;
        int rc = mx_index_search_with_filter(idx_, flt.f_, vec.data(), 1, (int)limit, found.data(), scores.data(), nullptr, &nf);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, scores[j]);
        }
        return out;
    }

    // every row whose score against vec is at least min_score, best first, at most limit (1 .. 4096) of them (mx_index_search_range):
    // a near-duplicate check before ingest, or context chosen by relevance rather than by count
    std::vector<VectorSearchResult> search_above(const std::vector<float> &vec, float min_score, size_t limit) {
        std::vector<VectorSearchResult> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0) return out;
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        int32_t nf = 0;
        uint64_t n_in_range = 0;
        int rc = mx_index_search_range(idx_, vec.data(), 1, &min_score, (int)std::min<size_t>(limit, (size_t)INT32_MAX), found.data(),
                                       scores.data(), nullptr, &nf, &n_in_range);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, scores[j]);
        }
        return out;
    }

    // the `limit` most relevant rows that do not repeat each other (mx_index_search_mmr: exact MMR re-ranking of the top-`fetch` rows),
    // in selection order: context for a prompt without the same passage from several overlapping windows.  fetch = 0: the default
    // min(max(4 * limit, 32), 1024); lambda = 1 is search()
    std::vector<VectorSearchResult> search_diverse(const std::vector<float> &vec, size_t limit, size_t fetch = 0, float lambda = 0.5f) {
        std::vector<VectorSearchResult> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0) return out;
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        if (fetch == 0) fetch = std::min<size_t>(std::max<size_t>(4 * limit, 32), 1024);
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        int32_t nf = 0;
        int rc = mx_index_search_mmr(idx_, vec.data(), 1, (int)std::min<size_t>(limit, (size_t)INT32_MAX),
                                     (int)std::min<size_t>(fetch, (size_t)INT32_MAX), lambda, found.data(), scores.data(), nullptr, &nf);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, scores[j]);
        }
        return out;
    }

    // one ranked list for SEVERAL query vectors -- the phrasings of a question, a question and a hypothetical answer, the last turns of a
    // conversation (mx_index_search_fused) -- each row once, with the score of its best vector.  mode MX_FUSE_MAX: the exact top-`limit`
    // by the best score over the vectors; MX_FUSE_RRF: reciprocal-rank fusion of their top-`fetch` lists (rrf_c = 60).  fetch = 0: the
    // default, limit for MAX and min(max(4 * limit, 32), 256) for RRF; weights: one per vector or empty (all ones), 0 leaves a vector out
    std::vector<VectorSearchResult> search_fused(const std::vector<std::vector<float>> &vecs, size_t limit, int mode = MX_FUSE_MAX,
                                                 size_t fetch = 0, const std::vector<float> &weights = {}) {
        std::vector<VectorSearchResult> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0 || vecs.empty()) return out;
        }
        std::vector<float> q;
        for (const std::vector<float> &v : vecs) {
            if (v.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
            q.insert(q.end(), v.begin(), v.end());
        }
        if (!weights.empty() && weights.size() != vecs.size())
            throw VectorStoreError(VectorStoreError::SearchError, "one weight per query vector expected");
        if (fetch == 0) fetch = mode == MX_FUSE_MAX ? limit : std::min<size_t>(std::max<size_t>(4 * limit, 32), 256);
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        int32_t nf = 0;
        int rc = mx_index_search_fused(idx_, q.data(), 1, (int)std::min<size_t>(vecs.size(), (size_t)INT32_MAX), weights.empty() ? nullptr : weights.data(),
                                       mode, (int)std::min<size_t>(limit, (size_t)INT32_MAX), (int)std::min<size_t>(fetch, (size_t)INT32_MAX), 60.0f,
                                       found.data(), scores.data(), nullptr, nullptr, nullptr, &nf);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, scores[j]);
        }
        return out;
    }

    // A resident grouping (mx_grouping): which segments belong to which document, one u32 key per row kept in HBM and named in
    // search_documents().  Every document name gets a key 1, 2, ... the first time it is seen; segments no call names are groups of
    // their own.  bulk_insert of a document, then assign(document, {its _ids}), is the ingest flow; release() un-groups.  The grouping
    // is not saved with the store: after compact(), delete_all() or a reload every call but the destructor throws: make a new one.
    class Grouping {
      public:
        Grouping(const Grouping &) = delete;
        Grouping &operator=(const Grouping &) = delete;
        Grouping(Grouping &&o) noexcept : store_(o.store_), g_(o.g_), key_of_(std::move(o.key_of_)), name_of_(std::move(o.name_of_)) {
            o.g_ = nullptr;
        }
        ~Grouping() {
            if (g_) mx_grouping_destroy(g_);
        }
        // document name -> the segment _ids under it, in one edit
        void assign_all(const std::map<std::string, std::vector<std::string>> &documents) {
            std::lock_guard<std::mutex> lk(store_->mu_);
            std::vector<std::pair<uint32_t, const std::vector<std::string> *>> pairs;
            for (auto &kv : documents) pairs.emplace_back(key_of(kv.first), &kv.second);
            set(pairs);
        }
        void assign(const std::string &document, const std::vector<std::string> &ids) { assign_all({{document, ids}}); }
        void release(const std::vector<std::string> &ids) {
            std::lock_guard<std::mutex> lk(store_->mu_);
            set({{0u, &ids}});
        }
        // the document name of a key; nothing for key 0 (ungrouped) or a key never handed out
        std::optional<std::string> document_of(uint32_t key) const {
            auto it = name_of_.find(key);
            return it == name_of_.end() ? std::nullopt : std::optional<std::string>(it->second);
        }
        // rows under a document, and those of them that are not removed
        std::pair<uint64_t, uint64_t> count() const {
            uint64_t a = 0, l = 0;
            int rc = mx_grouping_count(g_, &a, &l);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            return {a, l};
        }

      private:
        friend class HipFlatStore;
        friend class Filter;
        Grouping(HipFlatStore *store, mx_grouping *g) : store_(store), g_(g) {}
        uint32_t key_of(const std::string &document) {
            auto it = key_of_.find(document);
            if (it != key_of_.end()) return it->second;
            if (key_of_.size() >= 0xffffffffull) throw VectorStoreError(VectorStoreError::SearchError, "a grouping holds at most 2^32 - 1 documents");
            const uint32_t key = (uint32_t)key_of_.size() + 1;
            key_of_[document] = key;
            name_of_[key] = document;
            return key;
        }
        // (under the store's lock) one mx_grouping_set_ids call for all the pairs
        void set(const std::vector<std::pair<uint32_t, const std::vector<std::string> *>> &pairs) {
            store_->build_rows_of();
            std::vector<uint64_t> rows;
            std::vector<uint32_t> keys;
            for (auto &p : pairs) {
                std::set<std::string> seen;
                for (auto &id : *p.second) {
                    if (!seen.insert(id).second) continue;
                    auto it = store_->rows_of_.find(id);
                    if (it == store_->rows_of_.end()) continue;
                    rows.insert(rows.end(), it->second.begin(), it->second.end());
                    keys.insert(keys.end(), it->second.size(), p.first);
                }
            }
            int rc = mx_grouping_set_ids(g_, rows.empty() ? nullptr : rows.data(), keys.empty() ? nullptr : keys.data(), rows.size());
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        }
        HipFlatStore *store_;
        mx_grouping *g_;
        std::map<std::string, uint32_t> key_of_;
        std::map<uint32_t, std::string> name_of_;
    };

    Grouping make_grouping(const std::map<std::string, std::vector<std::string>> &documents = {}) {
        mx_grouping *g = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_) throw VectorStoreError(VectorStoreError::SearchError, "a grouping needs a store with rows: insert first");
            int rc = mx_grouping_create(idx_, &g);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        }
        Grouping out(this, g);
        if (!documents.empty()) out.assign_all(documents);
        return out;
    }

    // one document of a search_documents answer: its name (nothing for an ungrouped segment), its best segment, that segment's score,
    // and how many of the candidates looked at belong to it
    struct DocumentHit {
        std::optional<std::string> document;
        std::string segment;
        float score;
        int32_t group_rows;
    };

    // the `limit` best DOCUMENTS for vec, each by its best segment (mx_index_search_grouped), best first -> (hits, complete).  complete:
    // the hits are the exact top documents over the whole store (over flt's rows when given).  The candidates are the top-`fetch` rows
    // (fetch = 0: the default, 4 * limit clamped to [32, 256] and never below limit); when that answer is not complete the call asks
    // ONCE more with 4096 candidates
    std::pair<std::vector<DocumentHit>, bool> search_documents(const std::vector<float> &vec, size_t limit, const Grouping &grouping,
                                                               size_t fetch = 0, const Filter *flt = nullptr) {
        std::vector<DocumentHit> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0) return {out, true};
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        if (fetch == 0) fetch = std::min<size_t>(4096, std::max<size_t>(limit, std::min<size_t>(256, std::max<size_t>(32, 4 * limit))));
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        std::vector<uint32_t> keys(limit);
        std::vector<int32_t> rows(limit);
        int32_t nf = 0;
        uint8_t complete = 0;
        for (int step = 0; step < 2; ++step) {
            int rc = mx_index_search_grouped(idx_, grouping.g_, flt ? flt->f_ : nullptr, vec.data(), 1, (int)std::min<size_t>(limit, (size_t)INT32_MAX),
                                             (int)std::min<size_t>(fetch, (size_t)INT32_MAX), found.data(), scores.data(), nullptr, keys.data(),
                                             rows.data(), &nf, &complete);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            if (complete || fetch >= 4096) break;
            fetch = 4096;
        }
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.push_back(DocumentHit{grouping.document_of(keys[j]), it->second, scores[j], rows[j]});
        }
        return {out, complete != 0};
    }

    // one document of a search_document_passages answer: its name (nothing for an ungrouped segment), its best segments as (_id, score)
    // pairs, best first, and whether it has no further segment that belongs among them
    struct DocumentPassages {
        std::optional<std::string> document;
        std::vector<VectorSearchResult> passages;
        bool members_complete;
    };

    // the `limit` best DOCUMENTS for vec, each with its `passages` best segments (mx_index_search_group_rows) -> (hits, complete).  The
    // passages of a hit are always the exact best ones of their document.  fetch = 0: the default, 4 * limit * passages clamped to
    // [32, 256] and never below limit; when the answer is not complete the call asks ONCE more with 4096 candidates
    std::pair<std::vector<DocumentPassages>, bool> search_document_passages(const std::vector<float> &vec, size_t limit, const Grouping &grouping,
                                                                            size_t passages = 3, size_t fetch = 0,
                                                                            const Filter *flt = nullptr) {
        std::vector<DocumentPassages> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0 || passages == 0) return {out, true};
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        const int k = (int)std::min<size_t>(limit, (size_t)INT32_MAX), n = (int)std::min<size_t>(passages, (size_t)INT32_MAX);
        if (fetch == 0)
            fetch = std::min<size_t>(4096, std::max<size_t>(limit, std::min<size_t>(256, std::max<size_t>(32, 4 * (size_t)k * (size_t)n))));
        const size_t width = n <= 16 && (size_t)k * (size_t)n <= 4096 ? (size_t)k * (size_t)n : 1;  // (past the caps the call is refused)
        std::vector<uint64_t> found(width);
        std::vector<float> scores(width);
        std::vector<uint32_t> keys(limit);
        std::vector<int32_t> members(limit);
        std::vector<uint8_t> mdone(limit);
        int32_t nf = 0;
        uint8_t complete = 0;
        for (int step = 0; step < 2; ++step) {
            int rc = mx_index_search_group_rows(idx_, grouping.g_, flt ? flt->f_ : nullptr, vec.data(), 1, k, n,
                                                (int)std::min<size_t>(fetch, (size_t)INT32_MAX), found.data(), scores.data(), nullptr,
                                                keys.data(), nullptr, members.data(), mdone.data(), &nf, &complete);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            if (complete || fetch >= 4096) break;
            fetch = 4096;
        }
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            DocumentPassages hit{grouping.document_of(keys[j]), {}, mdone[j] != 0};
            for (int r = 0; r < members[j]; ++r) {
                auto it = _id_map.find((size_t)found[(size_t)j * n + r]);
                if (it == _id_map.end())
                    throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
                hit.passages.push_back({it->second, scores[(size_t)j * n + r]});
            }
            out.push_back(std::move(hit));
        }
        return {out, complete != 0};
    }

    // one segment of a search_spread answer: its document (nothing for an ungrouped segment), its _id and score
    struct SpreadHit {
        std::optional<std::string> document;
        std::string segment;
        float score;
    };

    // the `limit` best segments for vec with at most `per_document` segments of any one document (mx_index_search_capped), a flat
    // list, best first -> (hits, complete).  fetch = 0: the default of search_documents; when the answer is not complete the call asks
    // ONCE more with 4096 candidates
    std::pair<std::vector<SpreadHit>, bool> search_spread(const std::vector<float> &vec, size_t limit, const Grouping &grouping,
                                                          size_t per_document = 2, size_t fetch = 0, const Filter *flt = nullptr) {
        std::vector<SpreadHit> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0 || per_document == 0) return {out, true};
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        if (fetch == 0) fetch = std::min<size_t>(4096, std::max<size_t>(limit, std::min<size_t>(256, std::max<size_t>(32, 4 * limit))));
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        std::vector<uint32_t> keys(limit);
        int32_t nf = 0;
        uint8_t complete = 0;
        for (int step = 0; step < 2; ++step) {
            int rc = mx_index_search_capped(idx_, grouping.g_, flt ? flt->f_ : nullptr, vec.data(), 1, (int)std::min<size_t>(limit, (size_t)INT32_MAX),
                                            (int)std::min<size_t>(per_document, (size_t)INT32_MAX), (int)std::min<size_t>(fetch, (size_t)INT32_MAX),
                                            found.data(), scores.data(), nullptr, keys.data(), &nf, &complete);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            if (complete || fetch >= 4096) break;
            fetch = 4096;
        }
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.push_back(SpreadHit{grouping.document_of(keys[j]), it->second, scores[j]});
        }
        return {out, complete != 0};
    }

    // A resident prior (mx_prior): what the vectors do not say about a segment -- how recent, how important, how trusted -- one f32 per
    // row kept in HBM and added to the score by search_boosted().  Segments nobody set read 0.  bulk_insert of a document, then
    // set_document({its _ids}, value), is the ingest flow.  The prior is not saved with the store: after compact(), delete_all() or a
    // reload every call but the destructor throws: make a new one.
    class Prior {
      public:
        Prior(const Prior &) = delete;
        Prior &operator=(const Prior &) = delete;
        Prior(Prior &&o) noexcept : store_(o.store_), p_(o.p_) { o.p_ = nullptr; }
        ~Prior() {
            if (p_) mx_prior_destroy(p_);
        }
        // every row inserted under ids[i] gets values[i]; unknown _ids add nothing.  One mx_prior_set_ids call for all of them
        void set(const std::vector<std::string> &ids, const std::vector<float> &values) {
            if (ids.size() != values.size()) throw VectorStoreError(VectorStoreError::SearchError, "one value per _id");
            std::lock_guard<std::mutex> lk(store_->mu_);
            store_->build_rows_of();
            std::vector<uint64_t> rows;
            std::vector<float> vals;
            for (size_t i = 0; i < ids.size(); ++i) {
                auto it = store_->rows_of_.find(ids[i]);
                if (it == store_->rows_of_.end()) continue;
                rows.insert(rows.end(), it->second.begin(), it->second.end());
                vals.insert(vals.end(), it->second.size(), values[i]);
            }
            int rc = mx_prior_set_ids(p_, rows.empty() ? nullptr : rows.data(), vals.empty() ? nullptr : vals.data(), rows.size());
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        }
        // one value for all the segments of a document
        void set_document(const std::vector<std::string> &document_ids, float value) {
            set(document_ids, std::vector<float>(document_ids.size(), value));
        }
        // the upper bound of the values that `complete` is decided with; refresh: recomputed over the rows that are not removed
        float bound(bool refresh = false) const {
            float hi = 0.0f;
            int rc = mx_prior_bound(p_, refresh ? 1 : 0, &hi);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            return hi;
        }

      private:
        friend class HipFlatStore;
        friend class Filter;
        Prior(HipFlatStore *store, mx_prior *p) : store_(store), p_(p) {}
        HipFlatStore *store_;
        mx_prior *p_;
    };

    Prior make_prior() {
        mx_prior *p = nullptr;
        std::lock_guard<std::mutex> lk(mu_);
        if (!idx_) throw VectorStoreError(VectorStoreError::SearchError, "a prior needs a store with rows: insert first");
        int rc = mx_prior_create(idx_, &p);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        return Prior(this, p);
    }

    // one segment of a search_boosted answer: its _id, its score, its prior, and combined = (double)score + (double)weight * (double)prior
    struct BoostedHit {
        std::string _id;
        float score;
        float prior;
        double combined;
    };

    // the `limit` best segments for vec by score + weight * prior (mx_index_search_boosted), best first -> (hits, complete).  complete:
    // the hits are the exact top segments over the whole store (over flt's rows when given).  The candidates are the top-`fetch` rows
    // (fetch = 0: the default, 4 * limit clamped to [32, 256] and never below limit); when that answer is not complete the call asks
    // ONCE more with 4096 candidates
    std::pair<std::vector<BoostedHit>, bool> search_boosted(const std::vector<float> &vec, size_t limit, const Prior &prior, float weight = 1.0f,
                                                            size_t fetch = 0, const Filter *flt = nullptr) {
        std::vector<BoostedHit> out;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0) return {out, true};
        }
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        if (fetch == 0) fetch = std::min<size_t>(4096, std::max<size_t>(limit, std::min<size_t>(256, std::max<size_t>(32, 4 * limit))));
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit), priors(limit);
        std::vector<double> combined(limit);
        int32_t nf = 0;
        uint8_t complete = 0;
        for (int step = 0; step < 2; ++step) {
            int rc = mx_index_search_boosted(idx_, prior.p_, flt ? flt->f_ : nullptr, vec.data(), &weight, 1,
                                             (int)std::min<size_t>(limit, (size_t)INT32_MAX), (int)std::min<size_t>(fetch, (size_t)INT32_MAX),
                                             found.data(), scores.data(), nullptr, priors.data(), combined.data(), &nf, &complete);
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            if (complete || fetch >= 4096) break;
            fetch = 4096;
        }
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.push_back(BoostedHit{it->second, scores[j], priors[j], combined[j]});
        }
        return {out, complete != 0};
    }

    // more like this: the `limit` entries closest to what is stored under _id, the asked _id itself left out.  Every row stored under
    // _id is a query (mx_index_search_by_id: the rows never leave the device, the own row is taken out exactly); the union of their
    // answers is ranked by best score, each row once.  An unknown _id returns nothing.  Every list must hold limit + (rows under _id)
    // entries for the answer to be exact (the rows under _id take up places in it and are dropped below), and the library's lists end
    // at 4095: a larger sum throws Unsupported instead of answering from shortened lists
    std::vector<VectorSearchResult> more_like(const std::string &_id, size_t limit) {
        std::vector<VectorSearchResult> out;
        std::vector<uint64_t> mine;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0 || _id_map.empty()) return out;
            build_rows_of();
            auto it = rows_of_.find(_id);
            if (it != rows_of_.end()) mine.assign(it->second.begin(), it->second.end());
        }
        if (mine.empty()) return out;
        if (limit > 4095 || limit + mine.size() > 4095)
            throw VectorStoreError(VectorStoreError::Unsupported, "more_like: limit + the rows under the _id exceeds 4095");
        const size_t k = limit + mine.size();  // the rows under _id are the only entries dropped below
        const std::set<uint64_t> own(mine.begin(), mine.end());
        std::vector<uint64_t> found(mine.size() * k);
        std::vector<float> scores(found.size()), dists(found.size());
        std::vector<int32_t> nf(mine.size());
        int rc = mx_index_search_by_id(idx_, mine.data(), (int)mine.size(), (int)k, 1, found.data(), scores.data(), dists.data(), nf.data());
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::map<uint64_t, std::pair<float, float>> best;  // id -> (dist, score) of its best appearance
        for (size_t b = 0; b < mine.size(); ++b)
            for (int j = 0; j < nf[b]; ++j) {
                const uint64_t r = found[b * k + j];
                if (own.count(r)) continue;
                auto it = best.find(r);
                if (it == best.end() || dists[b * k + j] < it->second.first) best[r] = {dists[b * k + j], scores[b * k + j]};
            }
        std::vector<std::pair<std::pair<float, uint64_t>, float>> ranked;  // ((dist, id), score): the order search reports
        for (auto &kv : best) ranked.push_back({{kv.second.first, kv.first}, kv.second.second});
        std::sort(ranked.begin(), ranked.end());
        if (ranked.size() > limit) ranked.resize(limit);
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &r : ranked) {
            auto it = _id_map.find((size_t)r.first.second);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, r.second);
        }
        return out;
    }

    // relevance feedback (Rocchio) over segment _ids: more like `positive`, less like `negative`, the named segments themselves left
    // out.  Every row stored under a named _id is an example (mx_index_search_like: the rows never leave the device), scaled to unit
    // length and weighted beta / n_pos_rows or -gamma / n_neg_rows; vec (empty: none), the query the feedback is about, weighs alpha.
    // Unknown _ids are ignored; more than 16 rows in all: std::invalid_argument.  No example row and no vec returns nothing.
    // The weights are f32 divisions of the f32 parameters (beta / (float)n_pos_rows): the C ABI takes float weights, and the Python
    // mirror (memex_amd/storage.py) computes the same bits
    std::vector<VectorSearchResult> search_like(const std::vector<std::string> &positive, const std::vector<std::string> &negative = {},
                                                size_t limit = 10, const std::vector<float> &vec = {}, float alpha = 1.0f,
                                                float beta = 0.75f, float gamma = 0.15f) override {
        std::vector<VectorSearchResult> out;
        std::vector<uint64_t> ex;
        size_t n_pos = 0;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || limit == 0 || _id_map.empty()) return out;
            build_rows_of();
            for (const std::vector<std::string> *names : {&positive, &negative}) {
                for (const std::string &n : *names) {
                    auto it = rows_of_.find(n);
                    if (it != rows_of_.end()) ex.insert(ex.end(), it->second.begin(), it->second.end());
                }
                if (names == &positive) n_pos = ex.size();
            }
        }
        if (ex.size() > 16) throw std::invalid_argument("more than 16 example rows per request");
        if (!vec.empty() && vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        if (ex.empty() && vec.empty()) return out;
        std::vector<float> w;
        for (size_t i = 0; i < ex.size(); ++i) w.push_back(i < n_pos ? beta / (float)n_pos : -gamma / (float)(ex.size() - n_pos));
        if (ex.empty()) {  // the caller vector alone: one absent slot
            ex.push_back(0);
            w.push_back(0.0f);
        }
        const int k = (int)std::min<size_t>(limit, (size_t)INT32_MAX);
        std::vector<uint64_t> found(limit);
        std::vector<float> scores(limit);
        int32_t nf = 0;
        int rc = mx_index_search_like(idx_, vec.empty() ? nullptr : vec.data(), vec.empty() ? nullptr : &alpha, ex.data(), w.data(), 1,
                                      (int)ex.size(), k, 1, found.data(), scores.data(), nullptr, &nf, nullptr, nullptr);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::lock_guard<std::mutex> lk(mu_);
        for (int j = 0; j < nf; ++j) {
            auto it = _id_map.find((size_t)found[j]);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            out.emplace_back(it->second, scores[j]);
        }
        return out;
    }

    // Score the named segments against vec and rank them: the hits of a keyword backend, a cached result page, a caller's working set,
    // best first, cut to limit (0: all of them).  Every row stored under a named _id is a candidate (mx_index_score_ids: exact scores,
    // the rows never leave the device; lists of up to 4096 rows, longer candidate sets go as several lists of one call); a segment is
    // ranked by its best row in the (dist, id) order search reports and listed once.  Unknown _ids are skipped
    std::vector<VectorSearchResult> rerank(const std::vector<float> &vec, const std::vector<std::string> &ids, size_t limit = 0) override {
        std::vector<VectorSearchResult> out;
        std::vector<uint64_t> rows;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || _id_map.empty()) return out;
            build_rows_of();
            std::set<uint64_t> have;
            for (const std::string &n : ids) {
                auto it = rows_of_.find(n);
                if (it == rows_of_.end()) continue;
                for (uint64_t r : it->second)
                    if (have.insert(r).second) rows.push_back(r);
            }
        }
        if (rows.empty()) return out;
        if (vec.size() != (size_t)dim_) throw VectorStoreError(VectorStoreError::SearchError, "query dimension mismatch");
        const size_t m = std::min<size_t>(rows.size(), 4096), B = (rows.size() + m - 1) / m;
        rows.resize(B * m, 0);  // id 0: the padding of the last list
        std::vector<float> q(B * vec.size());
        for (size_t b = 0; b < B; ++b) std::copy(vec.begin(), vec.end(), q.begin() + b * vec.size());
        std::vector<float> scores(B * m), dists(B * m);
        std::vector<int32_t> order(B * m), nf(B);
        int rc = mx_index_score_ids(idx_, q.data(), (int)B, rows.data(), (int)m, scores.data(), dists.data(), order.data(), nf.data());
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
        std::vector<std::pair<std::pair<float, uint64_t>, float>> ranked;  // ((dist, id), score): the order search reports
        for (size_t b = 0; b < B; ++b)
            for (int r = 0; r < nf[b]; ++r) {
                const size_t at = b * m + (size_t)order[b * m + r];
                ranked.push_back({{dists[at], rows[at]}, scores[at]});
            }
        if (B > 1) std::sort(ranked.begin(), ranked.end());
        std::set<std::string> seen;
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &r : ranked) {
            auto it = _id_map.find((size_t)r.first.second);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            if (!seen.insert(it->second).second) continue;
            out.emplace_back(it->second, r.second);
            if (limit && out.size() >= limit) break;
        }
        return out;
    }

    struct DuplicatePair {
        std::string a, b;  // the _ids of the two rows, the one with the smaller row id first
        float score;
    };
    // The rows of the collection that repeat each other: every pair of live rows whose score reaches min_score, in row-id order -- an
    // exact self-join on the device (mx_index_search_range_by_id over ids 1 .. n in blocks of 512, cap = per_row, the own row
    // excluded).  truncated (optional): the _id of every row with more than per_row rows in range, whose list was cut.  The score is
    // symmetric bit for bit, so a pair is missing only if BOTH of its rows are in truncated; raise per_row (at most 4095) for those
    std::vector<DuplicatePair> find_duplicates(float min_score, size_t per_row = 64, std::vector<std::string> *truncated = nullptr) {
        std::vector<DuplicatePair> out;
        if (truncated) truncated->clear();
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!idx_ || _id_map.empty()) return out;
        }
        const uint64_t n = nb_point();
        const int cap = (int)std::min<size_t>(std::max<size_t>(per_row, 1), 4095);
        const size_t block = 512;
        std::map<std::pair<uint64_t, uint64_t>, float> pairs;  // (smaller id, larger id) -> score, each pair once
        std::vector<uint64_t> cut, q(block), found(block * cap), nr(block);
        std::vector<float> scores(block * cap), thr(block, min_score);
        std::vector<int32_t> nf(block);
        for (uint64_t lo = 0; lo < n; lo += block) {
            const int nb = (int)std::min<uint64_t>(block, n - lo);
            for (int b = 0; b < nb; ++b) q[b] = lo + b + 1;
            int rc = mx_index_search_range_by_id(idx_, q.data(), nb, thr.data(), cap, 1, found.data(), scores.data(), nullptr, nf.data(),
                                                 nr.data());
            if (rc != MX_OK) throw from_status(rc, VectorStoreError::SearchError);
            for (int b = 0; b < nb; ++b) {
                if (nr[b] > (uint64_t)cap) cut.push_back(q[b]);
                for (int j = 0; j < nf[b]; ++j) {
                    const uint64_t o = found[(size_t)b * cap + j];
                    pairs[{std::min(q[b], o), std::max(q[b], o)}] = scores[(size_t)b * cap + j];
                }
            }
        }
        std::lock_guard<std::mutex> lk(mu_);
        auto name = [&](uint64_t r) -> const std::string & {
            auto it = _id_map.find((size_t)r);
            if (it == _id_map.end())
                throw VectorStoreError(VectorStoreError::SearchError, "Internal inconsistency. Id from vector store not mapped.");
            return it->second;
        };
        for (auto &kv : pairs) out.push_back({name(kv.first.first), name(kv.first.second), kv.second});
        if (truncated)
            for (uint64_t r : cut) truncated->push_back(name(r));
        return out;
    }

    uint64_t nb_point() const {  // hnsw.get_nb_point() in the reference's test (local.rs:238)
        uint64_t n = 0;
        if (idx_) mx_index_size(idx_, &n);
        return n;
    }

  private:
    int device_ = 0, dim_ = 0;
    std::vector<int> devices_;
    mx_index *idx_ = nullptr;
    std::mutex mu_;
    // (mtime ns, size) of vectors.meta.json as last written / read, and how many ids it holds
    std::pair<long long, long long> meta_sig_{0, 0};
    size_t meta_ids_ = 0;
    bool meta_known_ = false;
    std::map<std::string, std::vector<size_t>> rows_of_;  // _id -> ids (remove): built by the first remove, kept on insert
    bool rows_of_built_ = false;

    void build_rows_of() {  // (under mu_)
        if (rows_of_built_) return;
        for (auto &kv : _id_map) rows_of_[kv.second].push_back(kv.first);
        rows_of_built_ = true;
    }

    static std::pair<long long, long long> file_sig(const std::string &p) {
        struct stat sb;
        if (stat(p.c_str(), &sb) != 0) return {-1, -1};
        return {(long long)sb.st_mtim.tv_sec * 1000000000LL + sb.st_mtim.tv_nsec, (long long)sb.st_size};
    }
    static void make_dirs(const std::string &dir) {  // create_dir_all (local.rs:144)
        std::string partial;
        for (size_t i = 0; i <= dir.size(); ++i)
            if (i == dir.size() || dir[i] == '/') {
                if (!partial.empty()) mkdir(partial.c_str(), 0755);
                if (i < dir.size()) partial += '/';
            } else {
                partial += dir[i];
            }
    }

    // keyed by the collection's path: every handle on this collection shares ONE resident GPU index
    void open(int dim) {
        const std::string key = storage_path + "@" + (devices_.empty() ? std::to_string(device_) : std::string("sharded"));
        int rc = devices_.empty() ? mx_index_open(key.c_str(), dim, device_, &idx_)
                                  : mx_index_open_sharded(key.c_str(), dim, (int)devices_.size(), devices_.data(), 0, &idx_);
        if (rc != MX_OK) throw from_status(rc, VectorStoreError::ConnectionError);
        dim_ = dim;
    }
    static std::string escape(const std::string &s) {
        std::string o;
        for (char c : s) {
            if (c == '"' || c == '\\') o += '\\';
            o += c;
        }
        return o;
    }
    // {"<usize>":"<id>", ...} as written by serde_json for HashMap<usize,String> (local.rs:156-163)
    static std::map<size_t, std::string> parse_id_map(const std::string &s) {
        std::map<size_t, std::string> m;
        size_t i = s.find('{');
        if (i == std::string::npos) throw VectorStoreError(VectorStoreError::SerdeError, "expected a JSON object");
        auto read_str = [&](std::string &out) {
            while (i < s.size() && s[i] != '"') {
                if (s[i] == '}') return false;
                ++i;
            }
            if (i >= s.size()) throw VectorStoreError(VectorStoreError::SerdeError, "unterminated JSON");
            ++i;
            out.clear();
            while (i < s.size() && s[i] != '"') {
                if (s[i] == '\\' && i + 1 < s.size()) ++i;
                out += s[i++];
            }
            if (i >= s.size()) throw VectorStoreError(VectorStoreError::SerdeError, "unterminated string");
            ++i;
            return true;
        };
        ++i;
        std::string k, v;
        while (read_str(k)) {
            if (!read_str(v)) throw VectorStoreError(VectorStoreError::SerdeError, "missing value");
            try {
                m[(size_t)std::stoull(k)] = v;
            } catch (const std::exception &) {
                throw VectorStoreError(VectorStoreError::SerdeError, "non-numeric key " + k);
            }
        }
        return m;
    }
};

class VectorStorage {  // mod.rs:69-93
  public:
    explicit VectorStorage(std::shared_ptr<VectorStore> c) : client(std::move(c)) {}
    std::shared_ptr<VectorStore> client;
    void add_vectors(const std::vector<VectorData> &points) {
        std::lock_guard<std::mutex> lk(*mu_);
        client->bulk_insert(points);
    }
    void delete_collection() {
        std::lock_guard<std::mutex> lk(*mu_);
        client->delete_all();
    }
    std::vector<VectorSearchResult> search(const std::vector<float> &query, size_t limit) {
        std::lock_guard<std::mutex> lk(*mu_);
        return client->search(query, limit);
    }
    std::vector<VectorSearchResult> search_like(const std::vector<std::string> &positive, const std::vector<std::string> &negative = {},
                                                size_t limit = 10, const std::vector<float> &vec = {}, float alpha = 1.0f,
                                                float beta = 0.75f, float gamma = 0.15f) {
        std::lock_guard<std::mutex> lk(*mu_);
        return client->search_like(positive, negative, limit, vec, alpha, beta, gamma);
    }
    std::vector<VectorSearchResult> rerank(const std::vector<float> &vec, const std::vector<std::string> &ids, size_t limit = 0) {
        std::lock_guard<std::mutex> lk(*mu_);
        return client->rerank(vec, ids, limit);
    }
    // (a prior belongs to a HipFlatStore: any other client is Unsupported)
    std::pair<std::vector<HipFlatStore::BoostedHit>, bool> search_boosted(const std::vector<float> &query, size_t limit,
                                                                          const HipFlatStore::Prior &prior, float weight = 1.0f,
                                                                          size_t fetch = 0, const HipFlatStore::Filter *flt = nullptr) {
        std::lock_guard<std::mutex> lk(*mu_);
        auto store = std::dynamic_pointer_cast<HipFlatStore>(client);
        if (!store) throw VectorStoreError(VectorStoreError::Unsupported, "search_boosted needs a HipFlatStore");
        return store->search_boosted(query, limit, prior, weight, fetch, flt);
    }

  private:
    std::shared_ptr<std::mutex> mu_ = std::make_shared<std::mutex>();
};

// mod.rs:95-139.  Called per request like the reference's; a collection that is already resident is
// attached, not reloaded.
inline VectorStorage get_vector_storage(const std::string &uri, const std::string &collection, int device = 0,
                                        std::vector<int> devices = {}) {
    const size_t p = uri.find("://");
    if (p == std::string::npos || p == 0) throw VectorStoreError(VectorStoreError::Unsupported, uri);
    const std::string scheme = uri.substr(0, p);
    if (scheme == "hnsw" || scheme == "hip") {  // the reference's file backend, now served from HBM
        const std::string storage = uri.substr(p + 3) + "/" + collection;
        std::string partial;
        for (size_t i = 0; i <= storage.size(); ++i)  // create_dir_all
            if (i == storage.size() || storage[i] == '/') {
                if (!partial.empty()) mkdir(partial.c_str(), 0755);
                if (i < storage.size()) partial += '/';
            } else {
                partial += storage[i];
            }
        std::shared_ptr<VectorStore> store;
        if (HipFlatStore::has_store(storage)) {
            store = HipFlatStore::load(storage, device, devices);
        } else {
            std::shared_ptr<HipFlatStore> res;
            {
                std::lock_guard<std::mutex> lk(HipFlatStore::registry_mu());
                auto it = HipFlatStore::registry().find(storage);
                if (it != HipFlatStore::registry().end() && it->second->_id_map.empty()) res = it->second;
            }
            store = res ? res : HipFlatStore::create(storage, device, devices);
        }
        return VectorStorage(store);
    }
    throw VectorStoreError(VectorStoreError::Unsupported, uri);  // opensearch+https is a remote client: out of scope
}

// ---- llm/embedding.rs ---------------------------------------------------------------------------
class EmbeddingError : public std::runtime_error {  // embedding.rs:11-16
  public:
    enum Kind { EncodingFailure, SetupError };
    EmbeddingError(Kind k, const std::string &m) : std::runtime_error(m), kind_(k) {}
    Kind kind() const { return kind_; }

  private:
    Kind kind_;
};

struct EmbeddingResult {  // embedding.rs:19-22
    std::string content;
    std::vector<float> vector;
};

enum class EmbeddingsModelType {  // embedding.rs:25-33
    DistiluseBaseMultilingualCased, BertBaseNliMeanTokens, AllMiniLmL12V2, AllMiniLmL6V2, AllDistilrobertaV1,
    ParaphraseAlbertSmallV2, SentenceT5Base
};

struct ModelConfig {  // embedding.rs:58-73
    EmbeddingsModelType model = EmbeddingsModelType::AllMiniLmL12V2;
    size_t max_length = 256;
    size_t stride = 86;
};

// STAND-IN tokenizer (the pretrained WordPiece vocabulary is not obtainable offline; a native
// WordPiece segmenter is SURVEY.md section 8 row f-1): lower-case, whitespace split, CRC-32 hash into
// [1000, vocab); [PAD]=0, [CLS]=101, [SEP]=102; windowing arithmetic as tokenizers 0.14.
struct WhitespaceHashTokenizer {
    int vocab = 30522;
    static std::vector<std::string> words(const std::string &text) {
        std::vector<std::string> w;
        std::string cur;
        for (unsigned char c : text) {
            if (std::isspace(c)) {
                if (!cur.empty()) w.push_back(cur), cur.clear();
            } else {
                cur += (char)std::tolower(c);
            }
        }
        if (!cur.empty()) w.push_back(cur);
        return w;
    }
    static uint32_t crc32(const std::string &s) {
        uint32_t c = 0xffffffffu;
        for (unsigned char ch : s) {
            c ^= ch;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
        }
        return ~c;
    }
    int word_id(const std::string &w) const { return 1000 + (int)(crc32(w) % (uint32_t)(vocab - 1000)); }
    std::vector<std::string> windows(const std::string &text, size_t max_length, size_t stride) const {
        const auto ws = words(text);
        std::vector<std::string> out;
        if (ws.empty()) return {""};
        const size_t step = max_length - stride;  // each overflow window starts max_length - stride later
        for (size_t start = 0;; start += step) {
            std::string seg;
            for (size_t i = start; i < ws.size() && i < start + max_length; ++i) seg += (i > start ? " " : "") + ws[i];
            out.push_back(seg);
            if (start + max_length >= ws.size()) break;
        }
        return out;
    }
    void encode_batch(const std::vector<std::string> &texts, size_t max_seq_length, std::vector<int32_t> &ids,
                      std::vector<int32_t> &lens, int &S) const {
        std::vector<std::vector<int32_t>> rows;
        S = 0;
        for (auto &t : texts) {
            std::vector<int32_t> r{101};
            for (auto &w : words(t)) {
                if (r.size() + 1 >= max_seq_length) break;
                r.push_back(word_id(w));
            }
            r.push_back(102);
            S = std::max<int>(S, (int)r.size());
            rows.push_back(std::move(r));
        }
        ids.assign(rows.size() * (size_t)S, 0);
        lens.clear();
        for (size_t i = 0; i < rows.size(); ++i) {
            std::copy(rows[i].begin(), rows[i].end(), ids.begin() + i * S);
            lens.push_back((int32_t)rows[i].size());
        }
    }
};

// The native tokenizer / segmenter (mx_tokenizer_*: WordPiece over a BERT vocab.txt, or byte-level BPE over vocab.json +
// merges.txt for the RoBERTa family): what Tokenizer::from_pretrained + with_truncation + encode / decode give
// segment_text (embedding.rs:163-195) and what rust-bert does to the segments before the forward.
class Tokenizer {
  public:
    static std::shared_ptr<Tokenizer> wordpiece(const std::string &vocab_txt, bool lowercase = true) {
        mx_tokenizer *h = nullptr;
        if (mx_tokenizer_create(vocab_txt.c_str(), lowercase ? 1 : 0, &h) != MX_OK)
            throw EmbeddingError(EmbeddingError::SetupError, mx_last_error());  // "Unable to load model", :166-169
        return std::shared_ptr<Tokenizer>(new Tokenizer(h));
    }
    static std::shared_ptr<Tokenizer> wordpiece_from_tokens(const std::vector<std::string> &tokens, bool lowercase = true) {
        std::string blob;
        for (const std::string &t : tokens) blob += t, blob += '\n';
        mx_tokenizer *h = nullptr;
        if (mx_tokenizer_create_from_memory(blob.data(), blob.size(), lowercase ? 1 : 0, &h) != MX_OK)
            throw EmbeddingError(EmbeddingError::SetupError, mx_last_error());
        return std::shared_ptr<Tokenizer>(new Tokenizer(h));
    }
    static std::shared_ptr<Tokenizer> bpe(const std::string &vocab_json, const std::string &merges_txt) {
        mx_tokenizer *h = nullptr;
        if (mx_tokenizer_create_bpe(vocab_json.c_str(), merges_txt.c_str(), &h) != MX_OK)
            throw EmbeddingError(EmbeddingError::SetupError, mx_last_error());
        return std::shared_ptr<Tokenizer>(new Tokenizer(h));
    }
    // tokenizer.json, the file Tokenizer::from_pretrained itself reads (embedding.rs:163): either kind, chosen by its "model"
    static std::shared_ptr<Tokenizer> from_file(const std::string &tokenizer_json) {
        mx_tokenizer *h = nullptr;
        if (mx_tokenizer_create_from_json(tokenizer_json.c_str(), &h) != MX_OK)
            throw EmbeddingError(EmbeddingError::SetupError, mx_last_error());
        return std::shared_ptr<Tokenizer>(new Tokenizer(h));
    }
    ~Tokenizer() { mx_tokenizer_destroy(h_); }
    Tokenizer(const Tokenizer &) = delete;
    Tokenizer &operator=(const Tokenizer &) = delete;

    std::vector<int32_t> encode(const std::string &text, bool add_special_tokens = false) const {
        std::vector<int32_t> ids(text.size() + 2);
        int n = 0;
        check(mx_tokenizer_encode(h_, text.c_str(), add_special_tokens ? 1 : 0, ids.data(), (int)ids.size(), &n), text);
        ids.resize((size_t)n);
        return ids;
    }
    std::string decode(const std::vector<int32_t> &ids, bool skip_special_tokens = true) const {
        size_t nb = 0;
        check(mx_tokenizer_decode(h_, ids.data(), (int)ids.size(), skip_special_tokens ? 1 : 0, nullptr, 0, &nb), "");
        std::string out(nb, '\0');
        check(mx_tokenizer_decode(h_, ids.data(), (int)ids.size(), skip_special_tokens ? 1 : 0, out.data(), nb, &nb), "");
        out.resize(nb ? nb - 1 : 0);
        return out;
    }
    // segment_text's windows for several documents in one call (documents are dealt to host threads)
    std::vector<std::vector<std::string>> windows_batch(const std::vector<std::string> &texts, size_t max_length, size_t stride) const {
        std::vector<const char *> ptrs;
        size_t bytes = 0;
        for (const std::string &t : texts) ptrs.push_back(t.c_str()), bytes += t.size();
        std::vector<int32_t> nseg(texts.size());
        std::string buf(bytes * 3 + 64 * texts.size() + 64, '\0');
        size_t nb = 0;
        for (int pass = 0; pass < 2; ++pass) {
            check(mx_tokenizer_segment_batch(h_, ptrs.data(), (int)texts.size(), (int)max_length, (int)stride, buf.data(), buf.size(), &nb,
                                             nseg.data()), "");
            if (nb <= buf.size()) break;
            buf.assign(nb, '\0');
        }
        std::vector<std::vector<std::string>> out(texts.size());
        const char *p = buf.data();
        for (size_t i = 0; i < texts.size(); ++i)
            for (int32_t k = 0; k < nseg[i]; ++k) {
                out[i].emplace_back(p);
                p += out[i].back().size() + 1;
            }
        return out;
    }
    std::vector<std::string> windows(const std::string &text, size_t max_length, size_t stride) const {
        return windows_batch({text}, max_length, stride)[0];
    }
    // [CLS] .. [SEP] rows, truncated to max_seq_length, [PAD]-padded to the batch maximum S
    void encode_batch(const std::vector<std::string> &texts, size_t max_seq_length, std::vector<int32_t> &ids, std::vector<int32_t> &lens,
                      int &S) const {
        std::vector<const char *> ptrs;
        for (const std::string &t : texts) ptrs.push_back(t.c_str());
        std::vector<int32_t> wide(texts.size() * max_seq_length);
        lens.assign(texts.size(), 0);
        S = 0;
        check(mx_tokenizer_encode_batch(h_, ptrs.data(), (int)texts.size(), (int)max_seq_length, wide.data(), (int)max_seq_length,
                                        lens.data(), &S), "");
        ids.resize(texts.size() * (size_t)S);
        for (size_t b = 0; b < texts.size(); ++b)
            std::copy(wide.begin() + b * max_seq_length, wide.begin() + b * max_seq_length + S, ids.begin() + b * (size_t)S);
    }
    int vocab_size() const {
        int n = 0;
        mx_tokenizer_vocab_size(h_, &n);
        return n;
    }

  private:
    explicit Tokenizer(mx_tokenizer *h) : h_(h) {}
    static void check(int rc, const std::string &text) {
        if (rc != MX_OK) throw EmbeddingError(EmbeddingError::EncodingFailure, text.empty() ? mx_last_error() : text);  // :176-179
    }
    mx_tokenizer *h_;
};

inline void check_segmentable(const ModelConfig &mc) {
    if (mc.model != EmbeddingsModelType::AllMiniLmL12V2 && mc.model != EmbeddingsModelType::AllMiniLmL6V2 &&
        mc.model != EmbeddingsModelType::AllDistilrobertaV1)
        throw EmbeddingError(EmbeddingError::SetupError, "Model not supported yet");  // :160
}

// embedding.rs:155-198.  `tok`: the model's tokenizer; without one the whitespace stand-in above (tests and benchmarks only)
inline std::vector<std::string> segment_text(const ModelConfig &mc, const std::string &text, const Tokenizer *tok = nullptr) {
    check_segmentable(mc);
    if (tok) return tok->windows(text, mc.max_length, mc.stride);
    return WhitespaceHashTokenizer{}.windows(text, mc.max_length, mc.stride);
}

// mx_encoder_cfg::precision of a configuration handed to SentenceEmbedder::spawn / load_pretrained_dir: "calibrate" -- open through
// mx_encoder_open_calibrated (memex_hip.h), which measures on the loaded weights which mode holds the score bar.  Distinct
// from the loaders' `precision < 0` = "the loader's choice by shape" (memex_pretrained.hpp), which is -1 everywhere.
constexpr int kPrecisionCalibrated = -2;

// The actor of embedding.rs:78-152: a dedicated thread owns the encoder; callers post
// (text, segment?, reply) messages on a queue bounded at 100 (sync_channel(100), :87).
class SentenceEmbedder {
  public:
    // `weights`: f32 blob in the order documented in memex_hip.h for `cfg`.
    // `cfg.precision == kPrecisionCalibrated`: the calibrated open with the library's probe and MX_CALIBRATE_BAR; calibration() is its report.
    // `tok`: the model's tokenizer (Tokenizer::wordpiece / ::bpe); nullptr = the whitespace stand-in (tests, benchmarks).
    static std::pair<std::thread, std::shared_ptr<SentenceEmbedder>> spawn(const ModelConfig &mc, const mx_encoder_cfg &cfg,
                                                                           std::vector<float> weights, size_t max_seq_length,
                                                                           int device = 0, std::shared_ptr<Tokenizer> tok = nullptr) {
        auto self = std::shared_ptr<SentenceEmbedder>(new SentenceEmbedder());
        std::promise<std::string> ready;
        auto fut = ready.get_future();
        std::thread th([self, mc, cfg, w = std::move(weights), max_seq_length, device, tok, pr = std::move(ready)]() mutable {
            self->runner(mc, cfg, w, max_seq_length, device, tok, pr);
        });
        const std::string err = fut.get();
        if (!err.empty()) {
            th.join();
            throw EmbeddingError(EmbeddingError::SetupError, err);
        }
        return {std::move(th), self};
    }
    std::vector<EmbeddingResult> encode(const std::string &text) { return call(text, true); }  // :138-142
    std::optional<EmbeddingResult> encode_single(const std::string &text) {                   // :146-151
        auto r = call(text, false);
        if (r.empty()) return std::nullopt;
        return r.back();
    }
    void shutdown() { post({"", false, nullptr, true}); }
    // the report of the calibrated open; nullptr when the precision was named by the caller
    const mx_encoder_calibration *calibration() const { return calibrated_ ? &calibration_ : nullptr; }

  private:
    bool calibrated_ = false;  // (written by the runner before spawn() returns)
    mx_encoder_calibration calibration_{};
    struct Msg {
        std::string text;
        bool segment;
        std::shared_ptr<std::promise<std::vector<EmbeddingResult>>> reply;
        bool stop = false;
    };
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Msg> q_;

    void post(Msg m) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return q_.size() < 100; });
        q_.push_back(std::move(m));
        cv_.notify_all();
    }
    std::vector<EmbeddingResult> call(const std::string &text, bool segment) {
        auto pr = std::make_shared<std::promise<std::vector<EmbeddingResult>>>();
        auto fut = pr->get_future();
        post({text, segment, pr});
        return fut.get();
    }
    void runner(const ModelConfig &mc, const mx_encoder_cfg &cfg, const std::vector<float> &w, size_t max_seq_length, int device,
                const std::shared_ptr<Tokenizer> &native, std::promise<std::string> &ready) {
        mx_encoder *enc = nullptr;
        if (mx_encoder_cfg_size() != sizeof(mx_encoder_cfg)) {  // this header and the loaded library disagree about the struct
            ready.set_value("mx_encoder_cfg size mismatch: header and libmemex_hip.so are different releases");
            return;
        }
        int rc;
        if (cfg.precision == kPrecisionCalibrated) {
            if (mx_encoder_calibration_size() != sizeof(mx_encoder_calibration)) {
                ready.set_value("mx_encoder_calibration size mismatch: header and libmemex_hip.so are different releases");
                return;
            }
            rc = mx_encoder_open_calibrated(nullptr, &cfg, w.data(), w.size() * sizeof(float), device, nullptr, nullptr, 0, 0, MX_CALIBRATE_BAR, 0,
                                            &enc, &calibration_);
            calibrated_ = rc == MX_OK;
        } else {
            rc = mx_encoder_create(&cfg, w.data(), w.size() * sizeof(float), device, &enc);  // create_model(), :99-100
        }
        if (rc != MX_OK) {
            ready.set_value(mx_last_error());
            return;
        }
        ready.set_value("");
        WhitespaceHashTokenizer tok{cfg.vocab};
        // Two stages: this thread segments and tokenises batch i+1 while `gpu` has batch i in mx_encoder_encode (host work per
        // document is about as long as its encoder pass).  A slot of one batch between them.
        using Reply = std::shared_ptr<std::promise<std::vector<EmbeddingResult>>>;
        struct Batch {
            std::vector<std::pair<Reply, std::vector<std::string>>> work;
            std::vector<int32_t> ids, lens;
            int S = 0;
            size_t rows = 0;
            bool last = false;
        };
        std::mutex smu;
        std::condition_variable scv;
        std::unique_ptr<Batch> slot;
        bool gpu_busy = false;
        std::thread gpu([&] {
            for (;;) {
                std::unique_ptr<Batch> b;
                {
                    std::unique_lock<std::mutex> lk(smu);
                    scv.wait(lk, [&] { return slot != nullptr; });
                    b = std::move(slot);
                    gpu_busy = true;
                    scv.notify_all();
                }
                if (b->last) return;
                try {
                    std::vector<float> out(b->rows * (size_t)cfg.hidden);
                    const int erc = mx_encoder_encode(enc, b->ids.data(), b->lens.data(), (int)b->rows, b->S, out.data());  // model.encode, :109
                    if (erc != MX_OK) throw EmbeddingError(EmbeddingError::EncodingFailure, mx_last_error());
                    size_t o = 0;
                    for (auto &wk : b->work) {
                        std::vector<EmbeddingResult> res;
                        for (size_t i = 0; i < wk.second.size(); ++i, ++o)
                            res.push_back({wk.second[i], std::vector<float>(out.begin() + o * cfg.hidden, out.begin() + (o + 1) * cfg.hidden)});
                        wk.first->set_value(std::move(res));
                    }
                } catch (...) {
                    for (auto &wk : b->work) {
                        try {
                            wk.first->set_exception(std::current_exception());
                        } catch (const std::future_error &) {  // already answered before the failure
                        }
                    }
                }
                std::lock_guard<std::mutex> lk(smu);
                gpu_busy = false;
            }
        });
        auto hand_over = [&](std::unique_ptr<Batch> b) {
            std::unique_lock<std::mutex> lk(smu);
            scv.wait(lk, [&] { return slot == nullptr; });
            slot = std::move(b);
            scv.notify_all();
        };
        bool stop = false;
        while (!stop) {
            // requests that queued up while the previous batch was on the GPU are embedded together
            // (the reference's runner takes one message per model.encode, :101-109; a row's embedding
            // does not depend on its batch).  With the GPU stage idle only half of what is waiting is taken:
            // synchronous callers come back with their next document only after a reply, so two smaller
            // batches keep both stages busy.
            std::vector<Msg> msgs;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return !q_.empty(); });
                bool idle;
                {
                    std::lock_guard<std::mutex> slk(smu);  // (the GPU stage never takes mu_: no lock-order cycle)
                    idle = !gpu_busy && slot == nullptr;
                }
                const size_t limit = idle ? std::max<size_t>(1, (q_.size() + 1) / 2) : 64;
                while (!q_.empty() && msgs.size() < limit) {
                    msgs.push_back(std::move(q_.front()));
                    q_.pop_front();
                }
                cv_.notify_all();
            }
            auto batch = std::make_unique<Batch>();
            // the documents of the drained requests are segmented together (one host thread per document)
            std::vector<std::vector<std::string>> pre;
            std::vector<size_t> pre_of(msgs.size(), (size_t)-1);
            if (native) {
                std::vector<std::string> docs;
                for (size_t i = 0; i < msgs.size(); ++i)
                    if (!msgs[i].stop && msgs[i].segment) pre_of[i] = docs.size(), docs.push_back(msgs[i].text);
                try {
                    check_segmentable(mc);
                    if (docs.size() > 1) pre = native->windows_batch(docs, mc.max_length, mc.stride);
                } catch (...) {  // reported per request below
                }
            }
            for (size_t i = 0; i < msgs.size(); ++i) {
                Msg &m = msgs[i];
                if (m.stop) {
                    stop = true;
                    continue;
                }
                try {
                    if (m.segment && pre_of[i] < pre.size()) batch->work.emplace_back(m.reply, std::move(pre[pre_of[i]]));
                    else batch->work.emplace_back(m.reply, m.segment ? segment_text(mc, m.text, native.get()) : std::vector<std::string>{m.text});  // :103-107
                } catch (...) {
                    m.reply->set_exception(std::current_exception());
                }
            }
            if (batch->work.empty()) continue;
            try {
                std::vector<std::string> flat;
                for (auto &wk : batch->work) flat.insert(flat.end(), wk.second.begin(), wk.second.end());
                if (native) native->encode_batch(flat, max_seq_length, batch->ids, batch->lens, batch->S);
                else tok.encode_batch(flat, max_seq_length, batch->ids, batch->lens, batch->S);
                batch->rows = flat.size();
            } catch (...) {
                for (auto &wk : batch->work) wk.first->set_exception(std::current_exception());
                continue;
            }
            hand_over(std::move(batch));
        }
        {
            auto fin = std::make_unique<Batch>();
            fin->last = true;
            hand_over(std::move(fin));
        }
        gpu.join();
        mx_encoder_destroy(enc);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// The two callers of the hot path, as far as the path goes (no SQL, no HTTP): what the worker does with a document
// (lib/worker/src/tasks.rs:9-66) and what the API does with a query (lib/api/src/endpoints/collections/handlers.rs:55-109).
// Segment ids are the reference's own: RFC 4122 version-5 UUIDs over its NAMESPACE (lib/libmemex/src/lib.rs:6).
// ---------------------------------------------------------------------------------------------------------------------
namespace detail {
inline void sha1(const std::string &msg, uint8_t out[20]) {
    uint32_t h[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
    std::string m = msg;
    const uint64_t bits = (uint64_t)msg.size() * 8;
    m.push_back((char)0x80);
    while (m.size() % 64 != 56) m.push_back('\0');
    for (int i = 7; i >= 0; --i) m.push_back((char)((bits >> (8 * i)) & 0xff));
    auto rol = [](uint32_t v, int n) { return (v << n) | (v >> (32 - n)); };
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[80];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)(uint8_t)m[off + 4 * i] << 24 | (uint32_t)(uint8_t)m[off + 4 * i + 1] << 16 |
                   (uint32_t)(uint8_t)m[off + 4 * i + 2] << 8 | (uint32_t)(uint8_t)m[off + 4 * i + 3];
        for (int i = 16; i < 80; ++i) w[i] = rol(w[i - 3] ^ w[i - 8] ^ w[i - 14] ^ w[i - 16], 1);
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
        for (int i = 0; i < 80; ++i) {
            uint32_t f, k;
            if (i < 20) f = (b & c) | (~b & d), k = 0x5a827999u;
            else if (i < 40) f = b ^ c ^ d, k = 0x6ed9eba1u;
            else if (i < 60) f = (b & c) | (b & d) | (c & d), k = 0x8f1bbcdcu;
            else f = b ^ c ^ d, k = 0xca62c1d6u;
            const uint32_t t = rol(a, 5) + f + e + k + w[i];
            e = d, d = c, c = rol(b, 30), b = a, a = t;
        }
        h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e;
    }
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(h[i] >> (24 - 8 * j));
}
}  // namespace detail

// Uuid::new_v5(namespace, name): SHA-1 over the namespace's 16 bytes and the name, version and variant bits set
inline std::string uuid5(const std::string &namespace_uuid, const std::string &name) {
    std::string bytes;
    int hi = -1;
    for (char c : namespace_uuid) {
        if (c == '-') continue;
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (v < 0) throw std::invalid_argument("uuid5: bad namespace");
        if (hi < 0) hi = v;
        else bytes.push_back((char)(hi << 4 | v)), hi = -1;
    }
    if (bytes.size() != 16 || hi >= 0) throw std::invalid_argument("uuid5: bad namespace");
    uint8_t d[20];
    detail::sha1(bytes + name, d);
    d[6] = (uint8_t)((d[6] & 0x0f) | 0x50);
    d[8] = (uint8_t)((d[8] & 0x3f) | 0x80);
    static const char *hex = "0123456789abcdef";
    std::string out;
    for (int i = 0; i < 16; ++i) {
        if (i == 4 || i == 6 || i == 8 || i == 10) out.push_back('-');
        out.push_back(hex[d[i] >> 4]);
        out.push_back(hex[d[i] & 15]);
    }
    return out;
}

inline const std::string &memex_namespace() {  // lib/libmemex/src/lib.rs:6
    static const std::string ns = "5fdfe40a-de2c-11ed-bfa7-00155deae876";
    return ns;
}
// db/document.rs:74: Uuid::new_v5(&NAMESPACE, task.id.to_string().as_bytes())
inline std::string document_uuid(int64_t task_id) { return uuid5(memex_namespace(), std::to_string(task_id)); }
// tasks.rs:36-40: Uuid::new_v5(&NAMESPACE, format!("{doc_uuid}-{idx}").as_bytes())
inline std::string segment_uuid(const std::string &doc_uuid, size_t idx) { return uuid5(memex_namespace(), doc_uuid + "-" + std::to_string(idx)); }

// tasks.rs:9-66 without the SQL: embedder.encode(content) -> one VectorData per window -> client.add_vectors.  Returns the
// VectorData the reference also writes to its `embeddings` table; a failing add_vectors is the caller's to log (it throws here).
inline std::vector<VectorData> process_embeddings(VectorStorage &client, SentenceEmbedder &embedder, int64_t task_id, const std::string &content) {
    const std::vector<EmbeddingResult> embeddings = embedder.encode(content);  // :19
    const std::string doc = document_uuid(task_id);                            // :28
    std::vector<VectorData> vectors;
    for (size_t idx = 0; idx < embeddings.size(); ++idx)                       // :34-56
        vectors.push_back(VectorData{segment_uuid(doc, idx), doc, embeddings[idx].content, embeddings[idx].vector, idx});
    client.add_vectors(vectors);                                               // :59
    return vectors;
}

// handlers.rs:72-85: embed the query, search; std::invalid_argument("Invalid query") where the handler rejects (:74-78)
inline std::vector<VectorSearchResult> search_docs(VectorStorage &client, SentenceEmbedder &embedder, const std::string &query, size_t limit = 10) {
    const std::optional<EmbeddingResult> res = embedder.encode_single(query);
    if (!res) throw std::invalid_argument("Invalid query");
    return client.search(res->vector, limit);
}

// search_docs for several texts at once (no counterpart in the reference): each is embedded with encode_single, the vectors go to
// HipFlatStore::search_fused and ONE list comes back.  std::invalid_argument("Invalid query") if any text embeds to nothing
inline std::vector<VectorSearchResult> search_docs_multi(HipFlatStore &store, SentenceEmbedder &embedder, const std::vector<std::string> &queries,
                                                         size_t limit = 10, int mode = MX_FUSE_MAX) {
    std::vector<std::vector<float>> vectors;
    for (const std::string &query : queries) {
        const std::optional<EmbeddingResult> res = embedder.encode_single(query);
        if (!res) throw std::invalid_argument("Invalid query");
        vectors.push_back(res->vector);
    }
    if (vectors.empty()) throw std::invalid_argument("Invalid query");
    return store.search_fused(vectors, limit, mode);
}

// tells a grouping which document the segments of a process_embeddings result belong to: every VectorData goes under its document_id
// (call it after the vectors were added)
inline void group_document(HipFlatStore::Grouping &grouping, const std::vector<VectorData> &vectors) {
    std::map<std::string, std::vector<std::string>> by_doc;
    for (const VectorData &v : vectors) by_doc[v.document_id].push_back(v._id);
    if (!by_doc.empty()) grouping.assign_all(by_doc);
}

// search_docs that answers in DOCUMENTS (no counterpart in the reference, whose handler returns segments): the `limit` best documents,
// each represented by its best segment (HipFlatStore::search_documents).  std::invalid_argument("Invalid query") where search_docs throws it
inline std::pair<std::vector<HipFlatStore::DocumentHit>, bool> search_documents(HipFlatStore &store, SentenceEmbedder &embedder,
                                                                                const HipFlatStore::Grouping &grouping, const std::string &query,
                                                                                size_t limit = 10) {
    const std::optional<EmbeddingResult> res = embedder.encode_single(query);
    if (!res) throw std::invalid_argument("Invalid query");
    return store.search_documents(res->vector, limit, grouping);
}

// ingest side of search_docs_recent: the segments of a process_embeddings result, written at time t, get the prior
// exp2((t - t0) / half_life).  The value is an f32: about 120 half-lives after t0 the epoch must be moved and the values written again
inline void stamp_document(HipFlatStore::Prior &prior, const std::vector<VectorData> &vectors, double t, double half_life, double t0) {
    const float value = (float)std::exp2((t - t0) / half_life);
    if (!std::isfinite(value)) throw std::invalid_argument("t is too far from t0 for an f32 prior: move t0 and stamp the documents again");
    std::vector<std::string> ids;
    for (const VectorData &v : vectors) ids.push_back(v._id);
    if (!ids.empty()) prior.set_document(ids, value);
}

// search_docs that prefers recent segments: a segment stamped at t is ranked by score + weight * exp2(-(now - t) / half_life).  The
// decay is folded into the query's weight, weight * exp2(-(now - t0) / half_life): the resident values are never rewritten
inline std::pair<std::vector<HipFlatStore::BoostedHit>, bool> search_docs_recent(HipFlatStore &store, SentenceEmbedder &embedder,
                                                                                 const HipFlatStore::Prior &prior, const std::string &query,
                                                                                 size_t limit, double now, double half_life, double t0,
                                                                                 double weight) {
    const std::optional<EmbeddingResult> res = embedder.encode_single(query);
    if (!res) throw std::invalid_argument("Invalid query");
    return store.search_boosted(res->vector, limit, prior, (float)(weight * std::exp2(-(now - t0) / half_life)));
}

}  // namespace memex
