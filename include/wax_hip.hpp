// wax_hip.hpp — header-only C++17 convenience wrapper over the C ABI in wax_hip.h.
// Mirrors the reference's VectorSearchEngine protocol (VectorSearchEngine.swift:10-18) for C++ hosts.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "wax_hip.h"

namespace wax_hip {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};

inline void check(int rc) {
    if (rc != WAX_HIP_OK) throw Error(rc, wax_hip_last_error());
}

class VectorEngine {
  public:
    static bool isAvailable() { return wax_hip_available() != 0; }
    VectorEngine(wax_hip_metric metric, uint32_t dimensions, int device = -1) {
        check(wax_hip_engine_create((uint8_t)metric, dimensions, device, &h_));
    }
    ~VectorEngine() { wax_hip_engine_destroy(h_); }
    VectorEngine(const VectorEngine&) = delete;
    VectorEngine& operator=(const VectorEngine&) = delete;

    uint32_t dimensions() const { return wax_hip_dimensions(h_); }
    uint64_t count() const { return wax_hip_count(h_); }

    std::vector<std::pair<uint64_t, float>> search(const std::vector<float>& vector, int topK) {
        // sized by topK alone (never by a row count read outside the engine's lock) and passed as the capacity
        const uint32_t cap = wax_hip_result_capacity(topK);
        std::vector<uint64_t> ids(cap);
        std::vector<float> scores(cap);
        uint32_t got = 0;
        check(wax_hip_search(h_, vector.data(), (uint32_t)vector.size(), topK, ids.data(), scores.data(), cap, &got));
        std::vector<std::pair<uint64_t, float>> out(got);
        for (uint32_t i = 0; i < got; ++i) out[i] = {ids[i], scores[i]};
        return out;
    }
    /// Batched filtered search: allow[q] null = no list for query q, minScores may be null. Returns per query [(frameId, score)].
    std::vector<std::vector<std::pair<uint64_t, float>>> searchBatchFiltered(const std::vector<float>& queries, uint32_t nq, int topK,
                                                                             const std::vector<const std::vector<uint64_t>*>& allow,
                                                                             const std::vector<float>* minScores) {
        const uint32_t dims = nq ? (uint32_t)(queries.size() / nq) : 0;
        const uint32_t stride = wax_hip_result_capacity(topK);
        std::vector<uint64_t> flat, begin(nq), len(nq);
        for (uint32_t q = 0; q < nq; ++q) {
            const std::vector<uint64_t>* a = q < allow.size() ? allow[q] : nullptr;
            begin[q] = flat.size();
            len[q] = a ? a->size() : WAX_HIP_NO_ALLOW_LIST;
            if (a) flat.insert(flat.end(), a->begin(), a->end());
        }
        std::vector<uint64_t> ids((size_t)nq * stride);
        std::vector<float> scores((size_t)nq * stride);
        std::vector<uint32_t> counts(nq);
        check(wax_hip_search_batch_filtered(h_, queries.data(), nq, dims, topK, flat.data(), flat.size(), begin.data(), len.data(),
                                            minScores ? minScores->data() : nullptr, ids.data(), scores.data(), stride, counts.data()));
        std::vector<std::vector<std::pair<uint64_t, float>>> out(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = 0; i < counts[q]; ++i) out[q].emplace_back(ids[(size_t)q * stride + i], scores[(size_t)q * stride + i]);
        return out;
    }
    /// searchBatchFiltered plus a row predicate per query (wax_hip_search_batch_predicate): `preds` holds one entry per query or is
    /// empty (no query has one). Query q is what searchPredicate(query q, topK, allow[q], cut q, preds[q]) returns.
    std::vector<std::vector<std::pair<uint64_t, float>>> searchBatchPredicate(const std::vector<float>& queries, uint32_t nq, int topK,
                                                                              const std::vector<const std::vector<uint64_t>*>& allow,
                                                                              const std::vector<float>* minScores,
                                                                              const std::vector<wax_hip_row_predicate>& preds) {
        if (!preds.empty() && preds.size() != nq) throw std::invalid_argument("searchBatchPredicate: one predicate per query, or none");
        const uint32_t dims = nq ? (uint32_t)(queries.size() / nq) : 0;
        const uint32_t stride = wax_hip_result_capacity(topK);
        std::vector<uint64_t> flat, begin(nq), len(nq);
        for (uint32_t q = 0; q < nq; ++q) {
            const std::vector<uint64_t>* a = q < allow.size() ? allow[q] : nullptr;
            begin[q] = flat.size();
            len[q] = a ? a->size() : WAX_HIP_NO_ALLOW_LIST;
            if (a) flat.insert(flat.end(), a->begin(), a->end());
        }
        std::vector<uint64_t> ids((size_t)nq * stride);
        std::vector<float> scores((size_t)nq * stride);
        std::vector<uint32_t> counts(nq);
        check(wax_hip_search_batch_predicate(h_, queries.data(), nq, dims, topK, flat.data(), flat.size(), begin.data(), len.data(),
                                             minScores ? minScores->data() : nullptr, preds.empty() ? nullptr : preds.data(), ids.data(),
                                             scores.data(), stride, counts.data()));
        std::vector<std::vector<std::pair<uint64_t, float>>> out(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = 0; i < counts[q]; ++i) out[q].emplace_back(ids[(size_t)q * stride + i], scores[(size_t)q * stride + i]);
        return out;
    }
    void add(uint64_t frameId, const std::vector<float>& v) { check(wax_hip_add(h_, frameId, v.data(), (uint32_t)v.size())); }
    /// Allow-list / minScore filtered search (UnifiedSearch.swift:1241-1258): best topK among the allowed frames.
    std::vector<std::pair<uint64_t, float>> searchFiltered(const std::vector<float>& q, int topK,
                                                           const std::vector<uint64_t>* allow, const float* minScore) {
        const uint32_t cap = wax_hip_result_capacity(topK);
        std::vector<uint64_t> ids(cap);
        std::vector<float> scores(cap);
        uint32_t n = 0;
        check(wax_hip_search_filtered(h_, q.data(), (uint32_t)q.size(), topK, allow ? 1 : 0,
                                      allow && !allow->empty() ? allow->data() : nullptr, allow ? allow->size() : 0,
                                      minScore ? 1 : 0, minScore ? *minScore : 0.0f, ids.data(), scores.data(), cap, &n));
        std::vector<std::pair<uint64_t, float>> out(n);
        for (uint32_t i = 0; i < n; ++i) out[i] = {ids[i], scores[i]};
        return out;
    }
    /// Per-row metadata for the predicate search (wax_hip_set_attributes): null = leave that column as it is.
    uint64_t setAttributes(const std::vector<uint64_t>& frameIds, const std::vector<int64_t>* timestamps, const std::vector<uint32_t>* flags) {
        uint64_t applied = 0;
        if (!frameIds.empty())
            check(wax_hip_set_attributes(h_, frameIds.data(), timestamps ? timestamps->data() : nullptr, flags ? flags->data() : nullptr,
                                         frameIds.size(), &applied));
        return applied;
    }
    /// One frame's attribute columns as getAttributes reads them back: (0, 0, false) for a frame the engine does not hold.
    struct Attributes {
        int64_t timestamp;
        uint32_t flags;
        bool found;
    };
    std::vector<Attributes> getAttributes(const std::vector<uint64_t>& frameIds) {
        std::vector<int64_t> ts(frameIds.size());
        std::vector<uint32_t> flags(frameIds.size());
        std::vector<uint8_t> found(frameIds.size());
        if (!frameIds.empty()) check(wax_hip_get_attributes(h_, frameIds.data(), frameIds.size(), ts.data(), flags.data(), found.data()));
        std::vector<Attributes> out(frameIds.size());
        for (size_t i = 0; i < out.size(); ++i) out[i] = {ts[i], flags[i], found[i] != 0};
        return out;
    }
    /// The timeline lane (wax_hip_timeline): the `limit` newest (or oldest) frames that pass `pred` (null = every frame), as
    /// (frameId, timestamp), ties by ascending frame id. limit <= 0 gives an empty answer.
    std::vector<std::pair<uint64_t, int64_t>> timeline(int limit, bool newestFirst, const wax_hip_row_predicate* pred) {
        const uint32_t cap = limit > 0 ? (uint32_t)(limit < WAX_HIP_TIMELINE_MAX_LIMIT ? limit : WAX_HIP_TIMELINE_MAX_LIMIT) : 0u;
        std::vector<uint64_t> ids(cap ? cap : 1);
        std::vector<int64_t> ts(cap ? cap : 1);
        uint32_t n = 0;
        check(wax_hip_timeline(h_, limit, newestFirst ? 1 : 0, pred, ids.data(), ts.data(), cap, &n));
        std::vector<std::pair<uint64_t, int64_t>> out(n);
        for (uint32_t i = 0; i < n; ++i) out[i] = {ids[i], ts[i]};
        return out;
    }
    /// FrameMeta.parentId of the listed frames for searchGrouped (wax_hip_set_parents): WAX_HIP_NO_PARENT = the frame is its own root.
    uint64_t setParents(const std::vector<uint64_t>& frameIds, const std::vector<uint64_t>& parentIds) {
        uint64_t applied = 0;
        if (frameIds.size() != parentIds.size()) throw std::runtime_error("setParents: one parent id per frame id");
        if (!frameIds.empty()) check(wax_hip_set_parents(h_, frameIds.data(), parentIds.data(), frameIds.size(), &applied));
        return applied;
    }
    /// The parents read back (wax_hip_get_parents): (parent, found) per frame; (WAX_HIP_NO_PARENT, false) for a frame the engine does not hold.
    std::vector<std::pair<uint64_t, bool>> getParents(const std::vector<uint64_t>& frameIds) {
        std::vector<uint64_t> parents(frameIds.size());
        std::vector<uint8_t> found(frameIds.size());
        if (!frameIds.empty()) check(wax_hip_get_parents(h_, frameIds.data(), frameIds.size(), parents.data(), found.data()));
        std::vector<std::pair<uint64_t, bool>> out(frameIds.size());
        for (size_t i = 0; i < out.size(); ++i) out[i] = {parents[i], found[i] != 0};
        return out;
    }
    /// What the grouped searches did (wax_hip_group_stats).
    wax_hip_group_stats_t groupStats() { wax_hip_group_stats_t st{}; check(wax_hip_group_stats(h_, &st)); return st; }
    /// One root of a grouped answer: its id, its score (its best member's) and its best members, best first.
    struct Group {
        uint64_t rootId;
        float score;
        std::vector<std::pair<uint64_t, float>> members;
    };
    /// The `limit` best roots by their best member and the perGroup best rows of each (wax_hip_search_grouped): what
    /// PhotoRAGOrchestrator.recall / VideoRAGOrchestrator.recall make of the vector lane, exactly. pred null = every row takes part.
    std::vector<Group> searchGrouped(const std::vector<float>& q, int limit, int perGroup, const float* minScore,
                                     const wax_hip_row_predicate* pred) {
        const uint32_t cap = limit > 0 ? (uint32_t)(limit < WAX_HIP_GROUP_MAX_LIMIT ? limit : WAX_HIP_GROUP_MAX_LIMIT) : 0u;
        const uint32_t width = perGroup < 1 ? 1u : (uint32_t)(perGroup < WAX_HIP_GROUP_MAX_MEMBERS ? perGroup : WAX_HIP_GROUP_MAX_MEMBERS);
        std::vector<uint64_t> roots(cap ? cap : 1), mids((size_t)(cap ? cap : 1) * width);
        std::vector<float> scores(cap ? cap : 1), mscores((size_t)(cap ? cap : 1) * width);
        std::vector<uint32_t> counts(cap ? cap : 1);
        uint32_t n = 0;
        check(wax_hip_search_grouped(h_, q.data(), (uint32_t)q.size(), limit, perGroup, minScore ? 1 : 0, minScore ? *minScore : 0.0f, pred,
                                     roots.data(), scores.data(), mids.data(), mscores.data(), counts.data(), &n));
        std::vector<Group> out(n);
        for (uint32_t g = 0; g < n; ++g) {
            out[g].rootId = roots[g];
            out[g].score = scores[g];
            for (uint32_t j = 0; j < counts[g]; ++j) out[g].members.push_back({mids[(size_t)g * width + j], mscores[(size_t)g * width + j]});
        }
        return out;
    }
    /// searchFiltered plus the row predicate (time range, denied flag bits): best topK among the frames that pass.
    std::vector<std::pair<uint64_t, float>> searchPredicate(const std::vector<float>& q, int topK, const std::vector<uint64_t>* allow,
                                                            const float* minScore, const wax_hip_row_predicate& pred) {
        const uint32_t cap = wax_hip_result_capacity(topK);
        std::vector<uint64_t> ids(cap);
        std::vector<float> scores(cap);
        uint32_t n = 0;
        check(wax_hip_search_predicate(h_, q.data(), (uint32_t)q.size(), topK, allow ? 1 : 0,
                                       allow && !allow->empty() ? allow->data() : nullptr, allow ? allow->size() : 0,
                                       minScore ? 1 : 0, minScore ? *minScore : 0.0f, &pred, ids.data(), scores.data(), cap, &n));
        std::vector<std::pair<uint64_t, float>> out(n);
        for (uint32_t i = 0; i < n; ++i) out[i] = {ids[i], scores[i]};
        return out;
    }
    /// The term SETS of the listed frames (wax_hip_set_terms): terms[i] replaces the whole set of frameIds[i]; an empty one clears it.
    uint64_t setTerms(const std::vector<uint64_t>& frameIds, const std::vector<std::vector<uint32_t>>& terms) {
        if (frameIds.size() != terms.size()) throw std::invalid_argument("setTerms: one term set per frame id");
        std::vector<uint32_t> flat, len(terms.size());
        std::vector<uint64_t> begin(terms.size());
        for (size_t i = 0; i < terms.size(); ++i) {
            begin[i] = flat.size();
            len[i] = (uint32_t)terms[i].size();
            flat.insert(flat.end(), terms[i].begin(), terms[i].end());
        }
        uint64_t applied = 0;
        if (!frameIds.empty())
            check(wax_hip_set_terms(h_, frameIds.data(), begin.data(), len.data(), flat.empty() ? nullptr : flat.data(), flat.size(), frameIds.size(),
                                    &applied));
        return applied;
    }
    /// The frame's term set, ascending; `found` (may be null) says whether the engine holds the frame.
    std::vector<uint32_t> getTerms(uint64_t frameId, bool* found = nullptr) {
        std::vector<uint32_t> out(WAX_HIP_TERMS_MAX_PER_ROW);
        uint32_t n = 0;
        uint8_t f = 0;
        check(wax_hip_get_terms(h_, frameId, out.data(), (uint32_t)out.size(), &n, &f));
        if (found) *found = f != 0;
        out.resize(n);
        return out;
    }
    /// searchPredicate among the frames whose term set holds every one of `required` (wax_hip_search_terms); pred null = no predicate.
    std::vector<std::pair<uint64_t, float>> searchTerms(const std::vector<float>& q, int topK, const std::vector<uint64_t>* allow,
                                                        const float* minScore, const wax_hip_row_predicate* pred,
                                                        const std::vector<uint32_t>& required) {
        const uint32_t cap = wax_hip_result_capacity(topK);
        std::vector<uint64_t> ids(cap);
        std::vector<float> scores(cap);
        uint32_t n = 0;
        check(wax_hip_search_terms(h_, q.data(), (uint32_t)q.size(), topK, allow ? 1 : 0,
                                   allow && !allow->empty() ? allow->data() : nullptr, allow ? allow->size() : 0,
                                   minScore ? 1 : 0, minScore ? *minScore : 0.0f, pred, required.empty() ? nullptr : required.data(),
                                   (uint32_t)required.size(), ids.data(), scores.data(), cap, &n));
        std::vector<std::pair<uint64_t, float>> out(n);
        for (uint32_t i = 0; i < n; ++i) out[i] = {ids[i], scores[i]};
        return out;
    }
    /// searchBatchPredicate plus a required-term set per query (wax_hip_search_batch_terms): `required` holds one entry per query (an
    /// empty one: no term filter for that query) or is empty (no query has one). Query q is what searchTerms(query q, ...) returns.
    std::vector<std::vector<std::pair<uint64_t, float>>> searchBatchTerms(const std::vector<float>& queries, uint32_t nq, int topK,
                                                                          const std::vector<const std::vector<uint64_t>*>& allow,
                                                                          const std::vector<float>* minScores,
                                                                          const std::vector<wax_hip_row_predicate>& preds,
                                                                          const std::vector<std::vector<uint32_t>>& required) {
        if (!preds.empty() && preds.size() != nq) throw std::invalid_argument("searchBatchTerms: one predicate per query, or none");
        if (!required.empty() && required.size() != nq) throw std::invalid_argument("searchBatchTerms: one term set per query, or none");
        const uint32_t dims = nq ? (uint32_t)(queries.size() / nq) : 0;
        const uint32_t stride = wax_hip_result_capacity(topK);
        std::vector<uint64_t> flat, begin(nq), len(nq), tbegin(required.size());
        std::vector<uint32_t> tflat, tlen(required.size());
        for (uint32_t q = 0; q < nq; ++q) {
            const std::vector<uint64_t>* a = q < allow.size() ? allow[q] : nullptr;
            begin[q] = flat.size();
            len[q] = a ? a->size() : WAX_HIP_NO_ALLOW_LIST;
            if (a) flat.insert(flat.end(), a->begin(), a->end());
        }
        for (size_t q = 0; q < required.size(); ++q) {
            tbegin[q] = tflat.size();
            tlen[q] = (uint32_t)required[q].size();
            tflat.insert(tflat.end(), required[q].begin(), required[q].end());
        }
        std::vector<uint64_t> ids((size_t)nq * stride);
        std::vector<float> scores((size_t)nq * stride);
        std::vector<uint32_t> counts(nq);
        check(wax_hip_search_batch_terms(h_, queries.data(), nq, dims, topK, flat.data(), flat.size(), begin.data(), len.data(),
                                         minScores ? minScores->data() : nullptr, preds.empty() ? nullptr : preds.data(),
                                         tflat.empty() ? nullptr : tflat.data(), tflat.size(), required.empty() ? nullptr : tbegin.data(),
                                         required.empty() ? nullptr : tlen.data(), ids.data(), scores.data(), stride, counts.data()));
        std::vector<std::vector<std::pair<uint64_t, float>>> out(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = 0; i < counts[q]; ++i) out[q].emplace_back(ids[(size_t)q * stride + i], scores[(size_t)q * stride + i]);
        return out;
    }
    /// What the term searches / the batched term searches did (wax_hip_term_stats, wax_hip_term_batch_stats).
    wax_hip_term_stats_t termStats() { wax_hip_term_stats_t st{}; check(wax_hip_term_stats(h_, &st)); return st; }
    wax_hip_term_batch_stats_t termBatchStats() { wax_hip_term_batch_stats_t st{}; check(wax_hip_term_batch_stats(h_, &st)); return st; }
    /// Pending-embedding replay: WAL putEmbedding payloads back to back (UnifiedSearchEngineCache.swift:252-283).
    uint64_t applyPutEmbeddings(const uint8_t* payloads, uint64_t len) {
        uint64_t applied = 0;
        check(wax_hip_apply_put_embeddings(h_, payloads, len, &applied));
        return applied;
    }
    void addBatch(const std::vector<uint64_t>& frameIds, const std::vector<float>& rowsRowMajor) {
        if (frameIds.empty()) return;
        check(wax_hip_add_batch(h_, frameIds.data(), rowsRowMajor.data(), frameIds.size(),
                                (uint32_t)(rowsRowMajor.size() / frameIds.size())));
    }
    /// Capacity for at least `rows` rows (wax_hip_reserve); columns and rows are kept.
    void reserve(uint64_t rows) { check(wax_hip_reserve(h_, rows)); }
    void remove(uint64_t frameId) { check(wax_hip_remove(h_, frameId)); }
    /// remove() for many ids in one compaction pass; returns the rows removed (absent ids are ignored, repeated ones count once).
    uint64_t removeBatch(const std::vector<uint64_t>& frameIds) {
        uint64_t removed = 0;
        if (!frameIds.empty()) check(wax_hip_remove_batch(h_, frameIds.data(), frameIds.size(), &removed));
        return removed;
    }
    std::vector<uint8_t> serialize() {
        uint8_t* p = nullptr;
        size_t len = 0;
        check(wax_hip_serialize(h_, &p, &len));
        std::vector<uint8_t> out(p, p + len);
        wax_hip_free(p);
        return out;
    }
    void deserialize(const std::vector<uint8_t>& bytes) { check(wax_hip_deserialize(h_, bytes.data(), bytes.size())); }
    wax_hip_engine* raw() { return h_; }

  private:
    wax_hip_engine* h_ = nullptr;
};

/// One query each against many stores of one device in one pass (wax_hip_search_many): pair i is (engines[i], row i of `queries`,
/// row-major engines.size() x dims). Returns per pair [(frameId, score)], each what engines[i]->search(query i, topK) returns.
inline std::vector<std::vector<std::pair<uint64_t, float>>> searchMany(const std::vector<VectorEngine*>& engines,
                                                                       const std::vector<float>& queries, int topK) {
    const uint32_t n = (uint32_t)engines.size();
    const uint32_t dims = n ? (uint32_t)(queries.size() / n) : 0;
    const uint32_t stride = wax_hip_result_capacity(topK);
    std::vector<wax_hip_engine*> raw(n);
    for (uint32_t i = 0; i < n; ++i) raw[i] = engines[i] ? engines[i]->raw() : nullptr;
    std::vector<uint64_t> ids((size_t)n * stride);
    std::vector<float> scores((size_t)n * stride);
    std::vector<uint32_t> counts(n);
    check(wax_hip_search_many(raw.data(), queries.data(), n, dims, topK, ids.data(), scores.data(), stride, counts.data()));
    std::vector<std::vector<std::pair<uint64_t, float>>> out(n);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back(ids[(size_t)i * stride + j], scores[(size_t)i * stride + j]);
    return out;
}

/// searchMany with a row predicate and a score cut per pair (wax_hip_search_many_predicate): `preds` / `minScores` hold one entry per
/// pair or are empty (no pair has one; a NaN cut means none for that pair). Pair i is what engines[i]->searchPredicate(query i, topK,
/// nullptr, cut i, pred i) returns.
inline std::vector<std::vector<std::pair<uint64_t, float>>> searchManyFiltered(const std::vector<VectorEngine*>& engines,
                                                                               const std::vector<float>& queries, int topK,
                                                                               const std::vector<wax_hip_row_predicate>& preds,
                                                                               const std::vector<float>& minScores = {}) {
    const uint32_t n = (uint32_t)engines.size();
    const uint32_t dims = n ? (uint32_t)(queries.size() / n) : 0;
    const uint32_t stride = wax_hip_result_capacity(topK);
    if ((!preds.empty() && preds.size() != n) || (!minScores.empty() && minScores.size() != n))
        throw std::invalid_argument("searchManyFiltered: one predicate / score cut per pair, or none");
    std::vector<wax_hip_engine*> raw(n);
    for (uint32_t i = 0; i < n; ++i) raw[i] = engines[i] ? engines[i]->raw() : nullptr;
    std::vector<uint64_t> ids((size_t)n * stride);
    std::vector<float> scores((size_t)n * stride);
    std::vector<uint32_t> counts(n);
    check(wax_hip_search_many_predicate(raw.data(), queries.data(), n, dims, topK, preds.empty() ? nullptr : preds.data(),
                                        minScores.empty() ? nullptr : minScores.data(), ids.data(), scores.data(), stride, counts.data()));
    std::vector<std::vector<std::pair<uint64_t, float>>> out(n);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back(ids[(size_t)i * stride + j], scores[(size_t)i * stride + j]);
    return out;
}

}  // namespace wax_hip
