// Native consumer of include/wax_hip.hpp and include/wax_hip.h with its own float64 model.
//
// A C++17 program that includes the wrapper and the standard library only (no HIP headers, no torch, no oracle). It calls every
// public member of wax_hip::VectorEngine, both free functions and the host-pointer exports that have no wrapper, and compares each
// answer with a brute-force model written as plain loops in double over the same inputs.
//
//   consumer [--model-only] SCORE_TOL TIE_TOL     (the two tolerances are tests/helpers.py's; they are not restated here)
//
// Scores follow VectorMetric.score(fromDistance:): cosine q.v / (|q||v|), dot q.v - 1, l2 -sum (q - v)^2.
// Every score must lie within SCORE_TOL of the model's; ids and counts must equal the model's. For ids to be decidable the program
// asserts, before the engine is touched, that the model's scores at ranks 1 .. k + 1 of the passing rows of each check differ from
// their neighbours by more than TIE_TOL unless the two rows are bit-equal copies (those must come back in the documented tie order).
// With k = 300 of 1 000 rows, or every row ranked, no seed of a free draw can give that (a few dozen of the ~1 000 neighbouring
// gaps fall below 2e-5 for any draw), so the generator redraws a row whose score against one of the store's five queries comes
// closer than 1.5 TIE_TOL to a row already drawn; the condition is still asserted per check, and a violation ends the program.
//
// Left to the Python tests, because a program without HIP headers cannot allocate device memory for them: wax_hip_add_batch_device,
// wax_hip_search_batch_hits_device, wax_hip_search_batch_submit_device / _collect_device, wax_hip_rrf_fuse_batch_device,
// wax_hip_set_row_base, wax_hip_search_shard_device, wax_hip_merge_hits_device, wax_hip_merge_batch_hits_device,
// wax_hip_timeline_device, and the probes (wax_hip_time_scan_kernel, wax_hip_time_stream_read, wax_hip_mirror8_snapshot,
// wax_hip_mirror8_keys, wax_hip_mirror_select_probe, wax_hip_mirror_lists_probe, wax_hip_timeline_probe, wax_hip_group_probe,
// wax_hip_term_mask_probe, wax_hip_term_mask_multi_probe).
//
// Modes: --model-only generates the inputs, runs the model, asserts the gap and filter conditions, prints `check <name>` for every
// check and never creates an engine. The default mode prints `ok <name>` / `FAIL <name>: <detail>` per check and
// `checks <n> failed <m>`; without a device it prints `no-device: ...` and exits 0. Every refusal tested here is one the library
// answers with a status before any launch.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <type_traits>

#include "wax_hip.hpp"

namespace {

using Hits = std::vector<std::pair<uint64_t, float>>;
using wax_hip::VectorEngine;

bool LIVE = true, QUIET = false;
double SCORE_TOL = 0, TIE_TOL = 0;
int n_checks = 0, n_failed = 0;
constexpr uint64_t SEED = 20240611;
constexpr uint32_t NQ = 5;

[[noreturn]] void fatal(const std::string& what) {
    std::printf("input condition violated: %s\n", what.c_str());
    std::exit(3);
}

void report(const std::string& name, const std::string& detail) {
    ++n_checks;
    if (!LIVE) { if (!QUIET) std::printf("check %s\n", name.c_str()); return; }
    if (detail.empty()) { std::printf("ok %s\n", name.c_str()); return; }
    ++n_failed;
    std::printf("FAIL %s: %s\n", name.c_str(), detail.c_str());
}

/// A check whose engine side is `body` (run only with a device); it returns "" or what went wrong.
void expect(const std::string& name, const std::function<std::string()>& body) { report(name, LIVE ? body() : std::string()); }

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// ---- the integer generator (splitmix64): every machine draws the same bytes -------------------------------------------------
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return next() % n; }
    double unit() { return (double)(next() >> 11) / 9007199254740992.0; }   // [0, 1), exact in double
    /// A bell-shaped value from integers alone: the sum of four 16-bit fields of one draw, centred.
    double bell() {
        const uint64_t z = next();
        const int64_t s4 = (int64_t)(z & 0xffff) + (int64_t)((z >> 16) & 0xffff) + (int64_t)((z >> 32) & 0xffff) + (int64_t)(z >> 48);
        return (double)(s4 - 2 * 65535) / 65536.0;
    }
};

// ---- the model: a store as plain vectors, scores in double -------------------------------------------------------------------
struct Store {
    uint32_t dims = 0;
    int metric = 0;
    std::vector<uint64_t> ids;
    std::vector<float> rows;
    std::vector<int64_t> ts;
    std::vector<uint32_t> flags;
    std::vector<uint64_t> parent;
    std::vector<std::vector<uint32_t>> terms;          // ascending, distinct
    std::vector<std::vector<float>> queries;           // the store's NQ queries
    std::vector<std::vector<double>> qscore;           // [query][row], kept for the generator's redraw rule
    size_t n() const { return ids.size(); }
    const float* row(size_t r) const { return rows.data() + r * dims; }
    long find(uint64_t id) const {
        for (size_t r = 0; r < ids.size(); ++r) if (ids[r] == id) return (long)r;
        return -1;
    }
    bool copies(size_t a, size_t b) const { return std::memcmp(row(a), row(b), dims * sizeof(float)) == 0; }
};

double model_score(int metric, const float* v, const float* q, uint32_t d) {
    double dot = 0, m = 0, qq = 0, l2 = 0;
    for (uint32_t j = 0; j < d; ++j) {
        const double a = q[j], b = v[j];
        dot += a * b; m += b * b; qq += a * a; l2 += (a - b) * (a - b);
    }
    if (metric == WAX_HIP_METRIC_COSINE) {
        const double vn = std::sqrt(m), qn = std::sqrt(qq);
        return (vn > 1e-6 && qn > 1e-6) ? dot / (vn * qn) : 0.0;       // score = 1 - distance
    }
    if (metric == WAX_HIP_METRIC_DOT) return dot - 1.0;                   // distance 1 - q.v, score -distance
    return -l2;
}

bool passes_pred(const wax_hip_row_predicate* p, int64_t ts, uint32_t flags) {
    if (!p) return true;
    return !(p->has_after && ts < p->after) && !(p->has_before && ts >= p->before) && (flags & p->deny_flags) == 0;
}

std::vector<float> draw_unit(Rng& rng, uint32_t dims, double scale) {
    std::vector<double> v(dims);
    double s = 0;
    for (auto& x : v) { x = rng.bell(); s += x * x; }
    const double inv = scale / std::sqrt(s);
    std::vector<float> out(dims);
    for (uint32_t j = 0; j < dims; ++j) out[j] = (float)(v[j] * inv);
    return out;
}

/// A new row for the store: redrawn until its score against every query keeps 1.5 TIE_TOL from every row other than `skip`.
std::vector<float> draw_row(Rng& rng, const Store& st, long skip, std::vector<double>* out_scores) {
    for (int tries = 0; tries < 10000; ++tries) {
        const double scale = st.metric == WAX_HIP_METRIC_COSINE ? 1.0 : 0.5 + 1.5 * rng.unit();
        std::vector<float> v = draw_unit(rng, st.dims, scale);
        std::vector<double> sc(st.queries.size());
        bool good = true;
        for (size_t q = 0; q < st.queries.size() && good; ++q) {
            sc[q] = model_score(st.metric, v.data(), st.queries[q].data(), st.dims);
            for (size_t r = 0; r < st.n() && good; ++r)
                if ((long)r != skip && std::fabs(st.qscore[q][r] - sc[q]) <= 1.5 * TIE_TOL) good = false;
        }
        if (good) { *out_scores = sc; return v; }
    }
    fatal("the generator found no row that keeps the gaps");
}

void push_row(Store& st, uint64_t id, const std::vector<float>& v, const std::vector<double>& sc) {
    st.ids.push_back(id);
    st.rows.insert(st.rows.end(), v.begin(), v.end());
    st.ts.push_back(0); st.flags.push_back(0); st.parent.push_back(WAX_HIP_NO_PARENT); st.terms.emplace_back();
    for (size_t q = 0; q < sc.size(); ++q) st.qscore[q].push_back(sc[q]);
}

void erase_row(Store& st, size_t r) {
    st.ids.erase(st.ids.begin() + (long)r);
    st.rows.erase(st.rows.begin() + (long)(r * st.dims), st.rows.begin() + (long)((r + 1) * st.dims));
    st.ts.erase(st.ts.begin() + (long)r); st.flags.erase(st.flags.begin() + (long)r);
    st.parent.erase(st.parent.begin() + (long)r); st.terms.erase(st.terms.begin() + (long)r);
    for (auto& qs : st.qscore) qs.erase(qs.begin() + (long)r);
}

/// The upsert of the interface: a held id keeps its row (and its columns), a new one is appended.
void upsert(Store& st, uint64_t id, const std::vector<float>& v, const std::vector<double>& sc) {
    const long r = st.find(id);
    if (r < 0) { push_row(st, id, v, sc); return; }
    std::copy(v.begin(), v.end(), st.rows.begin() + r * (long)st.dims);
    for (size_t q = 0; q < sc.size(); ++q) st.qscore[q][(size_t)r] = sc[q];
}

Store make_store(uint64_t seed, uint32_t dims, int metric, size_t n, const std::vector<std::vector<float>>& queries) {
    Rng rng(seed);
    Store st;
    st.dims = dims; st.metric = metric; st.queries = queries;
    st.qscore.resize(queries.size());
    std::vector<uint64_t> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = i;
    for (size_t i = n; i > 1; --i) std::swap(perm[i - 1], perm[rng.below(i)]);
    for (size_t r = 0; r < n; ++r) {
        const uint64_t id = perm[r] * 3 + 5;
        if (r > 0 && rng.below(6) == 0) {                                  // a bit-for-bit copy of an earlier row
            const size_t src = rng.below(r);
            std::vector<float> v(st.row(src), st.row(src) + dims);
            std::vector<double> sc(queries.size());
            for (size_t q = 0; q < queries.size(); ++q) sc[q] = st.qscore[q][src];
            push_row(st, id, v, sc);
        } else {
            std::vector<double> sc;
            std::vector<float> v = draw_row(rng, st, -1, &sc);
            push_row(st, id, v, sc);
        }
    }
    return st;
}

std::vector<std::vector<float>> make_queries(uint64_t seed, uint32_t dims) {
    Rng rng(seed ^ 0x51ed270b);
    std::vector<std::vector<float>> qs;
    for (uint32_t q = 0; q < NQ; ++q) qs.push_back(draw_unit(rng, dims, 1.0));
    return qs;
}

struct Spec {
    const float* q = nullptr;
    int topK = 10;
    const std::vector<uint64_t>* allow = nullptr;
    const float* minScore = nullptr;
    const wax_hip_row_predicate* pred = nullptr;
    const std::vector<uint32_t>* required = nullptr;
    bool filterMayBeTrivial = false;   // checks whose filter is MEANT to pass nothing (or everything)
};

struct Ranked { double score; size_t row; };

/// The passing rows of a check, best first by (score descending, row ascending), and the gap condition on ranks 1 .. k + 1.
std::vector<Ranked> model_rank(const Store& st, const Spec& s, const std::string& name, size_t k) {
    std::set<uint64_t> allowed;
    if (s.allow) allowed.insert(s.allow->begin(), s.allow->end());
    std::vector<Ranked> out;
    for (size_t r = 0; r < st.n(); ++r) {
        if (s.allow && !allowed.count(st.ids[r])) continue;
        if (!passes_pred(s.pred, st.ts[r], st.flags[r])) continue;
        bool has_all = true;
        if (s.required)
            for (uint32_t t : *s.required) if (!std::binary_search(st.terms[r].begin(), st.terms[r].end(), t)) has_all = false;
        if (!has_all) continue;
        out.push_back({model_score(st.metric, st.row(r), s.q, st.dims), r});
    }
    const bool filtered = s.allow || s.pred || (s.required && !s.required->empty());
    if (filtered && !s.filterMayBeTrivial && (out.empty() || out.size() == st.n()))
        fatal(name + ": the filter passes " + std::to_string(out.size()) + " of " + std::to_string(st.n()) + " rows");
    std::sort(out.begin(), out.end(), [](const Ranked& a, const Ranked& b) { return a.score != b.score ? a.score > b.score : a.row < b.row; });
    for (size_t i = 0; i + 1 < out.size() && i <= k; ++i)
        if (!(out[i].score - out[i + 1].score > TIE_TOL) && !st.copies(out[i].row, out[i + 1].row))
            fatal(name + fmt(": ranks %zu and %zu are %.3g apart", i + 1, i + 2, out[i].score - out[i + 1].score));
    return out;
}

size_t clamp_k(int topK) { return (size_t)std::min(std::max(topK, 1), WAX_HIP_MAX_RESULTS); }

/// What a search must return: `must` in order, then possibly a prefix of `maybe` (rows whose model score lies within SCORE_TOL of the
/// cut: an f32 score there may fall on either side of it).
struct Expected {
    std::vector<std::pair<uint64_t, double>> must, maybe;
    bool hasCut = false;
    float cut = 0;
};

Expected model_search(const Store& st, const Spec& s, const std::string& name) {
    const size_t k = clamp_k(s.topK);
    std::vector<Ranked> ranked = model_rank(st, s, name, k);
    if (ranked.size() > k) ranked.resize(k);
    Expected e;
    if (s.minScore && !std::isnan(*s.minScore)) { e.hasCut = true; e.cut = *s.minScore; }
    for (const Ranked& r : ranked) {
        if (!e.hasCut || r.score > (double)e.cut + SCORE_TOL) {
            if (!e.maybe.empty()) fatal(name + ": a row above the cut ranks behind one at the cut");
            e.must.push_back({st.ids[r.row], r.score});
        } else if (r.score >= (double)e.cut - SCORE_TOL) {
            e.maybe.push_back({st.ids[r.row], r.score});
        }
    }
    return e;
}

std::string compare(const Hits& got, const Expected& e) {
    if (got.size() < e.must.size() || got.size() > e.must.size() + e.maybe.size())
        return fmt("count %zu, model %zu (+%zu at the cut)", got.size(), e.must.size(), e.maybe.size());
    for (size_t i = 0; i < got.size(); ++i) {
        const auto& x = i < e.must.size() ? e.must[i] : e.maybe[i - e.must.size()];
        if (got[i].first != x.first) return fmt("rank %zu: id %llu, model %llu", i + 1, (unsigned long long)got[i].first, (unsigned long long)x.first);
        if (!(std::fabs((double)got[i].second - x.second) <= SCORE_TOL))
            return fmt("rank %zu: score %.9g, model %.9g", i + 1, (double)got[i].second, x.second);
        if (e.hasCut && got[i].second < e.cut) return fmt("rank %zu: score %.9g below the cut %.9g", i + 1, (double)got[i].second, (double)e.cut);
    }
    return "";
}

std::string same_bits(const Hits& a, const Hits& b, const char* what) {
    if (a.size() != b.size()) return fmt("%s: count %zu against %zu", what, a.size(), b.size());
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].first != b[i].first || std::memcmp(&a[i].second, &b[i].second, sizeof(float)) != 0)
            return fmt("%s: rank %zu is (%llu, %.9g) against (%llu, %.9g)", what, i + 1, (unsigned long long)a[i].first, (double)a[i].second,
                       (unsigned long long)b[i].first, (double)b[i].second);
    return "";
}

/// A cut halfway between the model's ranks r and r + 1 (1-based) of a check, or the first such boundary behind it whose two rows are
/// not copies: both neighbours are more than SCORE_TOL away.
float mid_cut(const Store& st, Spec s, size_t r, const std::string& name) {
    s.minScore = nullptr;
    const std::vector<Ranked> ranked = model_rank(st, s, name, clamp_k(s.topK));
    while (r < ranked.size() && st.copies(ranked[r - 1].row, ranked[r].row)) ++r;   // never between two copies: the next boundary down
    if (ranked.size() <= r) fatal(name + ": too few passing rows for the cut");
    return (float)(0.5 * (ranked[r - 1].score + ranked[r].score));
}

// ---- grouped search and timeline models ------------------------------------------------------------------------------------------
struct ModelGroup { uint64_t root; double score; size_t bestRow; std::vector<Ranked> members; };

std::vector<ModelGroup> model_grouped(const Store& st, const float* q, int limit, int perGroup, const float* cut, const wax_hip_row_predicate* pred,
                                      const std::string& name) {
    std::vector<ModelGroup> out;
    if (limit <= 0) return out;
    const size_t width = (size_t)std::min(std::max(perGroup, 1), WAX_HIP_GROUP_MAX_MEMBERS);
    std::map<uint64_t, std::vector<Ranked>> by_root;
    size_t passing = 0;
    for (size_t r = 0; r < st.n(); ++r) {
        if (!passes_pred(pred, st.ts[r], st.flags[r])) continue;
        ++passing;
        by_root[st.parent[r] == WAX_HIP_NO_PARENT ? st.ids[r] : st.parent[r]].push_back({model_score(st.metric, st.row(r), q, st.dims), r});
    }
    if (pred && (passing == 0 || passing == st.n())) fatal(name + ": the predicate passes none or all");
    for (auto& kv : by_root) {
        auto& m = kv.second;
        std::sort(m.begin(), m.end(), [](const Ranked& a, const Ranked& b) { return a.score != b.score ? a.score > b.score : a.row < b.row; });
        out.push_back({kv.first, m[0].score, m[0].row, m});
    }
    std::sort(out.begin(), out.end(), [](const ModelGroup& a, const ModelGroup& b) { return a.score != b.score ? a.score > b.score : a.root < b.root; });
    for (size_t g = 0; g + 1 < out.size() && g <= (size_t)limit; ++g)
        if (!(out[g].score - out[g + 1].score > TIE_TOL) && !st.copies(out[g].bestRow, out[g + 1].bestRow))
            fatal(name + fmt(": groups %zu and %zu are %.3g apart", g + 1, g + 2, out[g].score - out[g + 1].score));
    if (out.size() > (size_t)limit) out.resize((size_t)limit);
    for (auto& g : out) {
        for (size_t i = 0; i + 1 < g.members.size() && i <= width; ++i)
            if (!(g.members[i].score - g.members[i + 1].score > TIE_TOL) && !st.copies(g.members[i].row, g.members[i + 1].row))
                fatal(name + fmt(": members %zu and %zu of root %llu are too close", i + 1, i + 2, (unsigned long long)g.root));
        if (g.members.size() > width) g.members.resize(width);
    }
    if (cut) {
        std::vector<ModelGroup> kept;
        for (auto& g : out) {
            for (const auto& m : g.members)
                if (std::fabs(m.score - (double)*cut) <= SCORE_TOL) fatal(name + ": a member lies at the cut");
            if (g.score < (double)*cut) continue;
            while (!g.members.empty() && g.members.back().score < (double)*cut) g.members.pop_back();
            kept.push_back(g);
        }
        out = kept;
    }
    return out;
}

std::string compare_groups(const Store& st, const std::vector<VectorEngine::Group>& got, const std::vector<ModelGroup>& exp) {
    if (got.size() != exp.size()) return fmt("%zu groups, model %zu", got.size(), exp.size());
    for (size_t g = 0; g < got.size(); ++g) {
        if (got[g].rootId != exp[g].root) return fmt("group %zu: root %llu, model %llu", g, (unsigned long long)got[g].rootId, (unsigned long long)exp[g].root);
        if (!(std::fabs((double)got[g].score - exp[g].score) <= SCORE_TOL)) return fmt("group %zu: score %.9g, model %.9g", g, (double)got[g].score, exp[g].score);
        if (got[g].members.size() != exp[g].members.size()) return fmt("group %zu: %zu members, model %zu", g, got[g].members.size(), exp[g].members.size());
        for (size_t j = 0; j < got[g].members.size(); ++j) {
            if (got[g].members[j].first != st.ids[exp[g].members[j].row])
                return fmt("group %zu member %zu: id %llu, model %llu", g, j, (unsigned long long)got[g].members[j].first, (unsigned long long)st.ids[exp[g].members[j].row]);
            if (!(std::fabs((double)got[g].members[j].second - exp[g].members[j].score) <= SCORE_TOL))
                return fmt("group %zu member %zu: score %.9g, model %.9g", g, j, (double)got[g].members[j].second, exp[g].members[j].score);
        }
        if (!got[g].members.empty() && std::memcmp(&got[g].members[0].second, &got[g].score, sizeof(float)) != 0)
            return fmt("group %zu: member 0 does not carry the group's score", g);
    }
    return "";
}

using Timeline = std::vector<std::pair<uint64_t, int64_t>>;
Timeline model_timeline(const Store& st, int limit, bool newest, const wax_hip_row_predicate* pred, const std::string& name) {
    Timeline all;
    for (size_t r = 0; r < st.n(); ++r) if (passes_pred(pred, st.ts[r], st.flags[r])) all.push_back({st.ids[r], st.ts[r]});
    if (pred && (all.empty() || all.size() == st.n())) fatal(name + ": the predicate passes none or all");
    std::sort(all.begin(), all.end(), [newest](const std::pair<uint64_t, int64_t>& a, const std::pair<uint64_t, int64_t>& b) {
        if (a.second != b.second) return newest ? a.second > b.second : a.second < b.second;
        return a.first < b.first;
    });
    if (limit <= 0) all.clear();
    else if (all.size() > (size_t)limit) all.resize((size_t)limit);
    return all;
}

std::string compare_timeline(const Timeline& got, const Timeline& exp) {
    if (got.size() != exp.size()) return fmt("count %zu, model %zu", got.size(), exp.size());
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i] != exp[i]) return fmt("entry %zu: (%llu, %lld), model (%llu, %lld)", i, (unsigned long long)got[i].first, (long long)got[i].second,
                                         (unsigned long long)exp[i].first, (long long)exp[i].second);
    return "";
}

/// Runs `f`, which must throw E (and, for wax_hip::Error, with `status`); anything else is the detail of a failure.
template <class E>
std::string throws(const std::function<void()>& f, int status = 0) {
    (void)status;
    try {
        f();
    } catch (const E& err) {
        if constexpr (std::is_same<E, wax_hip::Error>::value) {
            if (err.status != status) return fmt("status %d, expected %d (%s)", err.status, status, err.what());
        } else if (dynamic_cast<const wax_hip::Error*>(static_cast<const std::exception*>(&err))) {
            return std::string("the library refused, not the wrapper: ") + err.what();
        }
        return "";
    }
    return "no exception";
}

wax_hip_row_predicate make_pred(bool after, int64_t a, bool before, int64_t b, uint32_t deny) {
    wax_hip_row_predicate p;
    std::memset(&p, 0, sizeof p);
    p.has_after = after; p.after = a; p.has_before = before; p.before = b; p.deny_flags = deny;
    return p;
}

void append_wal(std::vector<uint8_t>& out, uint64_t id, const std::vector<float>& v) {
    // WALEntryCodec.encode's putEmbedding payload: u8 opcode 0x04, u64 frameId LE, u32 dimension LE, dimension x f32 LE
    out.push_back(0x04);
    for (int i = 0; i < 8; ++i) out.push_back((uint8_t)(id >> (8 * i)));
    const uint32_t d = (uint32_t)v.size();
    for (int i = 0; i < 4; ++i) out.push_back((uint8_t)(d >> (8 * i)));
    for (float f : v) {
        uint32_t bits;
        std::memcpy(&bits, &f, 4);
        for (int i = 0; i < 4; ++i) out.push_back((uint8_t)(bits >> (8 * i)));
    }
}

// ---- one store's checks ---------------------------------------------------------------------------------------------------------
struct Bench {
    std::string pfx;
    Store m;
    std::unique_ptr<VectorEngine> e;
    Rng rng{0};
    uint64_t nextId = 0;

    std::vector<uint64_t> allowEmpty, allowSome, allowAbsent;
    std::vector<uint32_t> termOne{101}, termSixteen, termNone{999999}, termPair{100, 203}, termNothing;
    wax_hip_row_predicate pAfter = make_pred(true, 15, false, 777, 0), pBefore = make_pred(false, -5, true, 35, 0),
                          pBoth = make_pred(true, 10, true, 40, 0), pDeny = make_pred(false, 0, false, 0, WAX_HIP_FLAG_DELETED | WAX_HIP_FLAG_SURROGATE),
                          pMixed = make_pred(true, 5, false, 0, WAX_HIP_FLAG_SUPERSEDED), pNone = make_pred(false, 0, false, 0, 0);

    const float* q(size_t i) const { return m.queries[i].data(); }
    const std::vector<float>& qv(size_t i) const { return m.queries[i]; }
    std::vector<float> flatQueries() const {
        std::vector<float> f;
        for (const auto& x : m.queries) f.insert(f.end(), x.begin(), x.end());
        return f;
    }

    Hits call(const Spec& s, int kind, VectorEngine& eng) const {
        const std::vector<float> query(s.q, s.q + m.dims);
        switch (kind) {
            case 0: return eng.search(query, s.topK);
            case 1: return eng.searchFiltered(query, s.topK, s.allow, s.minScore);
            case 2: return eng.searchPredicate(query, s.topK, s.allow, s.minScore, s.pred ? *s.pred : pNone);
            default: return eng.searchTerms(query, s.topK, s.allow, s.minScore, s.pred, s.required ? *s.required : termNothing);
        }
    }
    /// One single-query check: kind 0 search, 1 searchFiltered, 2 searchPredicate, 3 searchTerms.
    void single(const std::string& name, const Spec& s, int kind) {
        const Expected exp = model_search(m, s, pfx + name);
        expect(pfx + name, [&] { return compare(call(s, kind, *e), exp); });
    }

    /// One batched check through the wrapper member of `kind` (1 searchBatchFiltered, 2 searchBatchPredicate, 3 searchBatchTerms):
    /// row q against the single-query wrapper (bits) and against the model.
    void batch(const std::string& name, int kind, int topK, const std::vector<const std::vector<uint64_t>*>& allow, const std::vector<float>* cuts,
               const std::vector<wax_hip_row_predicate>& preds, const std::vector<std::vector<uint32_t>>& required, bool trivialOk = false) {
        std::vector<Spec> specs(NQ);
        std::vector<Expected> exps;
        for (uint32_t i = 0; i < NQ; ++i) {
            Spec& s = specs[i];
            s.q = q(i); s.topK = topK;
            s.allow = i < allow.size() ? allow[i] : nullptr;
            s.minScore = cuts ? &(*cuts)[i] : nullptr;
            s.pred = preds.empty() ? nullptr : &preds[i];
            s.required = required.empty() ? nullptr : &required[i];
            s.filterMayBeTrivial = trivialOk || (s.allow && s.allow->empty()) || (s.pred && !s.pred->has_after && !s.pred->has_before && !s.pred->deny_flags);
            exps.push_back(model_search(m, s, pfx + name + fmt("[q%u]", i)));
        }
        expect(pfx + name, [&]() -> std::string {
            const std::vector<float> flat = flatQueries();
            std::vector<Hits> got;
            if (kind == 1) got = e->searchBatchFiltered(flat, NQ, topK, allow, cuts);
            else if (kind == 2) got = e->searchBatchPredicate(flat, NQ, topK, allow, cuts, preds);
            else got = e->searchBatchTerms(flat, NQ, topK, allow, cuts, preds, required);
            if (got.size() != NQ) return fmt("%zu rows for %u queries", got.size(), NQ);
            for (uint32_t i = 0; i < NQ; ++i) {
                std::string d = compare(got[i], exps[i]);
                if (d.empty()) d = same_bits(got[i], call(specs[i], kind, *e), "against the single-query wrapper");
                if (!d.empty()) return fmt("query %u: ", i) + d;
            }
            return "";
        });
    }

    void grouped(const std::string& name, size_t qi, int limit, int perGroup, const float* cut, const wax_hip_row_predicate* pred) {
        const std::vector<ModelGroup> exp = model_grouped(m, q(qi), limit, perGroup, cut, pred, pfx + name);
        expect(pfx + name, [&] { return compare_groups(m, e->searchGrouped(qv(qi), limit, perGroup, cut, pred), exp); });
    }

    void timeline(const std::string& name, int limit, bool newest, const wax_hip_row_predicate* pred) {
        const Timeline exp = model_timeline(m, limit, newest, pred, pfx + name);
        expect(pfx + name, [&] { return compare_timeline(e->timeline(limit, newest, pred), exp); });
    }

    std::vector<wax_hip_row_predicate> predsMixed() const { return {pNone, pAfter, pBoth, pDeny, pMixed}; }
    std::vector<std::vector<uint32_t>> requiredMixed() const { return {{}, termOne, termSixteen, {}, termPair}; }

    /// At least one search of every kind against the model: run after every mutation.
    void every_kind(const std::string& tag) {
        Spec s;
        s.q = q(0); s.topK = 10;
        single(tag + ".search", s, 0);
        s.q = q(1); s.allow = &allowSome;
        single(tag + ".searchFiltered", s, 1);
        s.q = q(2); s.allow = nullptr; s.pred = &pBoth;
        single(tag + ".searchPredicate", s, 2);
        s.q = q(3); s.pred = &pDeny; s.required = &termOne;
        single(tag + ".searchTerms", s, 3);
        const std::vector<const std::vector<uint64_t>*> allow{nullptr, &allowEmpty, &allowSome, &allowAbsent};
        batch(tag + ".searchBatchFiltered", 1, 10, allow, nullptr, {}, {});
        batch(tag + ".searchBatchPredicate", 2, 10, allow, nullptr, predsMixed(), {});
        batch(tag + ".searchBatchTerms", 3, 10, allow, nullptr, predsMixed(), requiredMixed());
        grouped(tag + ".searchGrouped", 4, 12, 3, nullptr, &pDeny);
        timeline(tag + ".timeline", 30, true, &pBoth);
    }

    void build_lists() {
        allowSome.clear(); allowAbsent.clear();
        for (size_t r = 0; r < m.n(); r += 3) allowSome.push_back(m.ids[r]);
        for (size_t r = 1; r < m.n(); r += 4) { allowAbsent.push_back(m.ids[r]); allowAbsent.push_back(m.ids[r] * 3); }   // ids = 0 mod 3 are never held
        allowAbsent.push_back(m.ids[1]);                                                                               // and one id twice
        termSixteen.clear();
        for (uint32_t t = 0; t < 16; ++t) termSixteen.push_back(1000 + t);
    }

    void run(uint32_t dims, wax_hip_metric metric, const char* label);
    void plain_and_filtered();
    void attributes_and_predicates();
    void parents_and_groups();
    void terms();
    void batches();
    void timelines();
    void unwrapped();
    void sharded();
    void mutations();
    void persistence();
};

void Bench::plain_and_filtered() {
    expect(pfx + "count_dimensions", [&] {
        return e->count() == m.n() && e->dimensions() == m.dims && e->raw() != nullptr ? std::string() : fmt("count %llu dims %u", (unsigned long long)e->count(), e->dimensions());
    });
    for (int k : {1, 10, 300, 1500}) {
        Spec s;
        s.q = q(0); s.topK = k;
        single(fmt("search.k%d", k), s, 0);
    }
    for (int kind = 1; kind <= 3; ++kind) {
        const std::string w = kind == 1 ? "searchFiltered" : kind == 2 ? "searchPredicate" : "searchTerms";
        Spec s;
        s.q = q((size_t)kind); s.topK = 10;
        single(w + ".allow_null", s, kind);
        s.allow = &allowEmpty; s.filterMayBeTrivial = true;
        single(w + ".allow_empty", s, kind);
        s.allow = &allowSome; s.filterMayBeTrivial = false;
        single(w + ".allow_present", s, kind);
        s.allow = &allowAbsent;
        single(w + ".allow_absent_ids", s, kind);
        // minScore = the model's fifth score, as an f32: the fifth row lies AT the cut and may fall on either side of it
        for (const std::vector<uint64_t>* a : {(const std::vector<uint64_t>*)nullptr, (const std::vector<uint64_t>*)&allowSome}) {
            Spec c;
            c.q = q((size_t)kind); c.topK = 10; c.allow = a;
            const std::vector<Ranked> ranked = model_rank(m, c, pfx + w + ".min_score", 10);
            if (ranked.size() < 6) fatal(pfx + w + ".min_score: fewer than six passing rows");
            const float fifth = (float)ranked[4].score;
            c.minScore = &fifth;
            single(w + (a ? ".min_score_fifth_allow" : ".min_score_fifth"), c, kind);
        }
    }
}

void Bench::attributes_and_predicates() {
    // column by column: timestamps alone, flags alone, then both for a part of the rows; absent ids do not count as applied
    std::vector<uint64_t> ids(m.ids);
    ids.push_back(3); ids.push_back(9);
    std::vector<int64_t> ts(ids.size());
    std::vector<uint32_t> fl(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) {
        ts[i] = (int64_t)rng.below(50) - 5;
        const uint64_t z = rng.next();
        fl[i] = (z % 5 == 0 ? WAX_HIP_FLAG_DELETED : 0u) | (z % 7 == 0 ? WAX_HIP_FLAG_SUPERSEDED : 0u) | (z % 11 == 0 ? WAX_HIP_FLAG_SURROGATE : 0u) |
                ((uint32_t)(z >> 40) & 3u) << WAX_HIP_FLAG_USER_SHIFT;
    }
    for (size_t r = 0; r < m.n(); ++r) m.ts[r] = ts[r];
    expect(pfx + "setAttributes.flags_null", [&] {
        const uint64_t a = e->setAttributes(ids, &ts, nullptr);
        return a == m.n() ? std::string() : fmt("applied %llu, model %zu", (unsigned long long)a, m.n());
    });
    auto read_back = [&](const std::string& name) {
        expect(pfx + name, [&]() -> std::string {
            std::vector<uint64_t> ask(m.ids);
            ask.push_back(6);
            const auto got = e->getAttributes(ask);
            if (got.size() != ask.size()) return "size";
            for (size_t r = 0; r < m.n(); ++r)
                if (!got[r].found || got[r].timestamp != m.ts[r] || got[r].flags != m.flags[r])
                    return fmt("row %zu: (%lld, %u, %d), model (%lld, %u)", r, (long long)got[r].timestamp, got[r].flags, (int)got[r].found, (long long)m.ts[r], m.flags[r]);
            if (got.back().found || got.back().timestamp != 0 || got.back().flags != 0) return "an absent id reads as found";
            return "";
        });
    };
    read_back("getAttributes.after_timestamps");
    for (size_t r = 0; r < m.n(); ++r) m.flags[r] = fl[r];
    expect(pfx + "setAttributes.timestamps_null", [&] {
        const uint64_t a = e->setAttributes(ids, nullptr, &fl);
        return a == m.n() ? std::string() : fmt("applied %llu, model %zu", (unsigned long long)a, m.n());
    });
    read_back("getAttributes.after_flags");
    std::vector<uint64_t> part;
    std::vector<int64_t> pts;
    std::vector<uint32_t> pfl;
    for (size_t r = 0; r < m.n(); r += 9) {
        part.push_back(m.ids[r]); pts.push_back((int64_t)rng.below(50) - 5); pfl.push_back((uint32_t)rng.below(8));
        m.ts[r] = pts.back(); m.flags[r] = pfl.back();
    }
    part.push_back(12); pts.push_back(1); pfl.push_back(1);
    expect(pfx + "setAttributes.both", [&] {
        const uint64_t a = e->setAttributes(part, &pts, &pfl);
        const uint64_t none = e->setAttributes({}, &pts, &pfl);
        return a == part.size() - 1 && none == 0 ? std::string() : fmt("applied %llu, model %zu", (unsigned long long)a, part.size() - 1);
    });
    read_back("getAttributes.after_both");

    const std::pair<const char*, const wax_hip_row_predicate*> cases[] = {{"after", &pAfter}, {"before", &pBefore}, {"both", &pBoth}, {"deny", &pDeny}};
    for (const auto& c : cases) {
        Spec s;
        s.q = q(2); s.topK = 10; s.pred = c.second;
        single(std::string("searchPredicate.") + c.first, s, 2);
        s.q = q(3);
        single(std::string("searchTerms.pred_") + c.first, s, 3);
    }
    Spec s;
    s.q = q(4); s.topK = 10; s.pred = &pMixed; s.allow = &allowAbsent;
    const float cut = mid_cut(m, s, 4, pfx + "searchPredicate.allow_cut");
    s.minScore = &cut;
    single("searchPredicate.allow_cut", s, 2);
}

void Bench::parents_and_groups() {
    std::vector<uint64_t> ids(m.ids), parents(m.n());
    for (size_t r = 0; r < m.n(); ++r) {
        if (r % 16 == 0) parents[r] = WAX_HIP_NO_PARENT;
        else if (r % 2 == 1) parents[r] = m.ids[r % 20 * 16];        // a held frame that is its own root
        else parents[r] = 900000 + r % 37;                            // roots the engine does not hold
        m.parent[r] = parents[r];
    }
    ids.push_back(3); parents.push_back(77);
    expect(pfx + "setParents", [&] {
        const uint64_t a = e->setParents(ids, parents);
        return a == m.n() && e->setParents({}, {}) == 0 ? std::string() : fmt("applied %llu, model %zu", (unsigned long long)a, m.n());
    });
    expect(pfx + "setParents.size_mismatch", [&] { return throws<std::runtime_error>([&] { e->setParents({5, 8}, {1}); }); });
    expect(pfx + "getParents", [&]() -> std::string {
        const auto got = e->getParents(ids);
        for (size_t r = 0; r < m.n(); ++r)
            if (!got[r].second || got[r].first != m.parent[r]) return fmt("row %zu: parent %llu, model %llu", r, (unsigned long long)got[r].first, (unsigned long long)m.parent[r]);
        return got.back().second || got.back().first != WAX_HIP_NO_PARENT ? "an absent id reads as found" : "";
    });
    wax_hip_group_stats_t before{};
    if (LIVE) before = e->groupStats();
    for (int pg : {1, 3, 8}) grouped(fmt("searchGrouped.per_group_%d", pg), 0, 12, pg, nullptr, nullptr);
    grouped("searchGrouped.limit_above_groups", 1, 400, 2, nullptr, nullptr);
    grouped("searchGrouped.limit_0", 1, 0, 2, nullptr, nullptr);
    grouped("searchGrouped.per_group_0", 1, 12, 0, nullptr, nullptr);
    grouped("searchGrouped.predicate", 2, 20, 3, nullptr, &pBoth);
    {
        // a cut between the eighth and ninth best rows of the store: later groups go, and so do members of the groups that stay
        Spec s;
        s.q = q(3); s.topK = 20;
        const float cut = mid_cut(m, s, 8, pfx + "searchGrouped.min_score");
        const auto all = model_grouped(m, q(3), 20, 8, nullptr, nullptr, pfx + "searchGrouped.min_score");
        const auto kept = model_grouped(m, q(3), 20, 8, &cut, nullptr, pfx + "searchGrouped.min_score");
        size_t members_all = 0, members_kept = 0;
        for (size_t g = 0; g < kept.size(); ++g) { members_all += all[g].members.size(); members_kept += kept[g].members.size(); }
        if (kept.empty() || kept.size() >= all.size() || members_kept >= members_all) fatal(pfx + "searchGrouped.min_score: the cut drops no group or no member");
        grouped("searchGrouped.min_score", 3, 20, 8, &cut, nullptr);
    }
    expect(pfx + "searchGrouped.limit_1025_refused", [&] {
        return throws<wax_hip::Error>([&] { e->searchGrouped(qv(0), WAX_HIP_GROUP_MAX_LIMIT + 1, 1, nullptr, nullptr); }, WAX_HIP_ERR_INVALID_ARGUMENT);
    });
    expect(pfx + "searchGrouped.per_group_9_refused", [&] {
        return throws<wax_hip::Error>([&] { e->searchGrouped(qv(0), 4, WAX_HIP_GROUP_MAX_MEMBERS + 1, nullptr, nullptr); }, WAX_HIP_ERR_INVALID_ARGUMENT);
    });
    expect(pfx + "c.search_grouped_refusals_write_nothing", [&]() -> std::string {
        // the same two refusals through the C call, into arrays large enough for what was asked and filled with a sentinel
        const size_t n = (size_t)(WAX_HIP_GROUP_MAX_LIMIT + 1) * (WAX_HIP_GROUP_MAX_MEMBERS + 1);
        std::vector<uint64_t> roots(n, 4242), mids(n, 4242);
        std::vector<float> rs(n, -7.0f), ms(n, -7.0f);
        std::vector<uint32_t> counts(n, 4242);
        for (int which = 0; which < 2; ++which) {
            uint32_t got = 0;
            const int rc = wax_hip_search_grouped(e->raw(), q(0), m.dims, which ? 4 : WAX_HIP_GROUP_MAX_LIMIT + 1, which ? WAX_HIP_GROUP_MAX_MEMBERS + 1 : 1, 0, 0.0f,
                                                  nullptr, roots.data(), rs.data(), mids.data(), ms.data(), counts.data(), &got);
            if (rc != WAX_HIP_ERR_INVALID_ARGUMENT) return fmt("refusal %d: status %d", which, rc);
            for (size_t i = 0; i < n; ++i)
                if (roots[i] != 4242 || mids[i] != 4242 || rs[i] != -7.0f || ms[i] != -7.0f || counts[i] != 4242) return fmt("refusal %d wrote entry %zu", which, i);
        }
        return "";
    });
    expect(pfx + "groupStats", [&] {
        // seven grouped searches reached the device above: limit 0 touches none, the two refusals neither
        const wax_hip_group_stats_t after = e->groupStats();
        return after.searches - before.searches == 7 && after.fused_scans + after.column_scans - before.fused_scans - before.column_scans == 7
                   ? std::string() : fmt("searches moved by %llu, expected 7", (unsigned long long)(after.searches - before.searches));
    });
}

void Bench::terms() {
    std::vector<uint64_t> ids(m.ids);
    std::vector<std::vector<uint32_t>> sets(m.n());
    for (size_t r = 0; r < m.n(); ++r) {
        std::vector<uint32_t>& s = sets[r];
        if (r % 13 == 0) {
            // the empty set
        } else if (r % 7 == 0) {
            for (uint32_t t = 0; t < 70; ++t) s.push_back(2063 - t % 64);      // 64 distinct terms, six of them twice, descending
        } else {
            s = {(uint32_t)(200 + r % 11), (uint32_t)(100 + r % 3)};
            if (r % 5 == 0) for (uint32_t t = 0; t < 16; ++t) s.push_back(1015 - t);
            if (r % 2 == 0) s.push_back(s[0]);                                    // a duplicate inside the set
        }
        m.terms[r] = s;
        std::sort(m.terms[r].begin(), m.terms[r].end());
        m.terms[r].erase(std::unique(m.terms[r].begin(), m.terms[r].end()), m.terms[r].end());
    }
    ids.push_back(3); sets.push_back({1, 2});
    expect(pfx + "setTerms", [&] {
        const uint64_t a = e->setTerms(ids, sets);
        return a == m.n() && e->setTerms({}, {}) == 0 ? std::string() : fmt("applied %llu, model %zu", (unsigned long long)a, m.n());
    });
    expect(pfx + "setTerms.size_mismatch", [&] { return throws<std::invalid_argument>([&] { e->setTerms({5, 8}, std::vector<std::vector<uint32_t>>(1)); }); });
    expect(pfx + "getTerms", [&]() -> std::string {
        for (size_t r = 0; r < m.n(); ++r) {
            bool found = false;
            if (e->getTerms(m.ids[r], &found) != m.terms[r] || !found) return fmt("row %zu: the set differs from the model's (ascending, distinct)", r);
        }
        bool found = true;
        return !e->getTerms(3, &found).empty() || found || !e->getTerms(6).empty() ? "an absent frame reads as found" : "";
    });
    expect(pfx + "setTerms.clear_and_restore", [&]() -> std::string {
        // an all-empty call (flat is empty: terms NULL) clears a set; the same call with the set puts it back
        const size_t r = 1;
        if (e->setTerms({m.ids[r]}, std::vector<std::vector<uint32_t>>(1)) != 1 || !e->getTerms(m.ids[r]).empty()) return "an empty set did not clear";
        return e->setTerms({m.ids[r]}, std::vector<std::vector<uint32_t>>(1, m.terms[r])) == 1 && e->getTerms(m.ids[r]) == m.terms[r] ? "" : "the set did not come back";
    });

    wax_hip_term_stats_t before{};
    if (LIVE) before = e->termStats();
    Spec s;
    s.q = q(3); s.topK = 10; s.required = &termOne;
    single("searchTerms.one_term", s, 3);
    s.required = &termSixteen;
    single("searchTerms.sixteen_terms", s, 3);
    s.required = &termNone; s.filterMayBeTrivial = true;
    single("searchTerms.term_nobody_holds", s, 3);
    s.filterMayBeTrivial = false; s.required = &termOne; s.pred = &pBoth; s.allow = &allowAbsent;
    const float cut = mid_cut(m, s, 3, pfx + "searchTerms.all_filters");
    s.minScore = &cut;
    single("searchTerms.all_filters", s, 3);
    expect(pfx + "termStats", [&] {
        const uint64_t moved = e->termStats().searches - before.searches;
        return moved == 4 ? std::string() : fmt("searches moved by %llu after four term searches", (unsigned long long)moved);
    });
    expect(pfx + "searchTerms.required_empty_is_searchPredicate", [&]() -> std::string {
        const uint64_t t0 = e->termStats().searches;
        const Hits a = e->searchTerms(qv(2), 10, &allowSome, nullptr, &pDeny, {});
        const Hits b = e->searchPredicate(qv(2), 10, &allowSome, nullptr, pDeny);
        if (e->termStats().searches != t0) return "a search without terms moved termStats.searches";
        return same_bits(a, b, "searchTerms({}) against searchPredicate");
    });
}

void Bench::batches() {
    const std::vector<const std::vector<uint64_t>*> mixed{nullptr, &allowEmpty, &allowSome, &allowAbsent};   // shorter than nq: query 4 has none
    const std::vector<const std::vector<uint64_t>*> none;
    const std::vector<const std::vector<uint64_t>*> nulls(NQ, nullptr);
    std::vector<float> cuts(NQ);
    for (uint32_t i = 0; i < NQ; ++i) {
        Spec s;
        s.q = q(i); s.topK = 10; s.allow = i < mixed.size() ? mixed[i] : nullptr;
        cuts[i] = (i == 1) ? -1e30f : (i == 3) ? std::numeric_limits<float>::quiet_NaN() : mid_cut(m, s, 3 + i, pfx + "batch.cuts");
    }
    batch("searchBatchFiltered.mixed_lists", 1, 10, mixed, nullptr, {}, {});
    batch("searchBatchFiltered.mixed_lists_cuts", 1, 10, mixed, &cuts, {}, {});
    batch("searchBatchFiltered.no_lists", 1, 10, none, nullptr, {}, {});
    batch("searchBatchFiltered.null_lists_k300", 1, 300, nulls, nullptr, {}, {});
    batch("searchBatchPredicate.preds_empty", 2, 10, mixed, &cuts, {}, {});
    batch("searchBatchPredicate.preds", 2, 10, mixed, nullptr, predsMixed(), {});
    batch("searchBatchPredicate.preds_no_lists", 2, 10, none, nullptr, predsMixed(), {});
    expect(pfx + "searchBatchPredicate.wrong_length", [&] {
        return throws<std::invalid_argument>([&] { e->searchBatchPredicate(flatQueries(), NQ, 10, none, nullptr, {pAfter, pBoth}); });
    });
    wax_hip_term_batch_stats_t before{};
    if (LIVE) before = e->termBatchStats();
    batch("searchBatchTerms.required_empty", 3, 10, mixed, nullptr, predsMixed(), {});
    expect(pfx + "termBatchStats.no_term_query", [&] {
        const wax_hip_term_batch_stats_t now = e->termBatchStats();
        return now.calls == before.calls && now.queries == before.queries ? "" : "a call without term sets moved the counters";
    });
    batch("searchBatchTerms.required", 3, 10, mixed, &cuts, predsMixed(), requiredMixed());
    expect(pfx + "termBatchStats.term_queries", [&] {
        // one call with three non-empty sets; the single-query wrapper calls made for the comparison do not count as batched calls
        const wax_hip_term_batch_stats_t now = e->termBatchStats();
        const uint64_t answered = (now.queries - before.queries) + (now.looped - before.looped) + (now.host_decided - before.host_decided);
        return now.calls - before.calls == 1 && answered == 3 ? std::string()
                                                              : fmt("calls moved by %llu, term queries by %llu", (unsigned long long)(now.calls - before.calls), (unsigned long long)answered);
    });
    batch("searchBatchTerms.required_no_lists_no_preds", 3, 10, none, nullptr, {}, requiredMixed());
    expect(pfx + "searchBatchTerms.wrong_lengths", [&]() -> std::string {
        std::string d = throws<std::invalid_argument>([&] { e->searchBatchTerms(flatQueries(), NQ, 10, none, nullptr, {pAfter}, {}); });
        if (d.empty()) d = throws<std::invalid_argument>([&] { e->searchBatchTerms(flatQueries(), NQ, 10, none, nullptr, {}, {termOne, termPair}); });
        return d;
    });
}

void Bench::timelines() {
    timeline("timeline.newest", 30, true, nullptr);
    timeline("timeline.oldest", 30, false, nullptr);
    timeline("timeline.newest_pred", 100, true, &pBoth);
    timeline("timeline.oldest_deny", 17, false, &pDeny);
    timeline("timeline.limit_0", 0, true, nullptr);
    timeline("timeline.limit_above_rows", 4096, false, &pMixed);
    expect(pfx + "timeline.limit_4097_refused", [&] {
        return throws<wax_hip::Error>([&] { e->timeline(WAX_HIP_TIMELINE_MAX_LIMIT + 1, true, nullptr); }, WAX_HIP_ERR_INVALID_ARGUMENT);
    });
}

/// The host-pointer exports that have no wrapper, called straight through wax_hip.h on the wrapper's handle.
void Bench::unwrapped() {
    Spec s;
    s.q = q(0); s.topK = 10;
    const Expected plain = model_search(m, s, pfx + "c.search_submit_collect");
    expect(pfx + "c.search_submit_collect", [&]() -> std::string {
        uint64_t t1 = 0, t2 = 0;
        wax_hip::check(wax_hip_search_submit(e->raw(), q(0), m.dims, 10, &t1));
        wax_hip::check(wax_hip_search_submit(e->raw(), q(1), m.dims, 10, &t2));
        std::vector<uint64_t> ids(10);
        std::vector<float> sc(10);
        uint32_t n = 0;
        wax_hip::check(wax_hip_search_collect(e->raw(), t2, ids.data(), sc.data(), 10, &n));   // collected out of order
        Hits second;
        for (uint32_t i = 0; i < n; ++i) second.push_back({ids[i], sc[i]});
        wax_hip::check(wax_hip_search_collect(e->raw(), t1, ids.data(), sc.data(), 10, &n));
        Hits first;
        for (uint32_t i = 0; i < n; ++i) first.push_back({ids[i], sc[i]});
        std::string d = compare(first, plain);
        if (d.empty()) d = same_bits(second, e->search(qv(1), 10), "ticket 2 against search");
        return d;
    });
    std::vector<Expected> per_query;
    for (uint32_t i = 0; i < NQ; ++i) {
        Spec b;
        b.q = q(i); b.topK = 7;
        per_query.push_back(model_search(m, b, pfx + "c.search_batch"));
    }
    expect(pfx + "c.search_batch", [&]() -> std::string {
        const uint32_t stride = 9;   // wider than top_k: the row stride is the caller's
        std::vector<uint64_t> ids(NQ * stride);
        std::vector<float> sc(NQ * stride);
        std::vector<uint32_t> counts(NQ);
        const std::vector<float> flat = flatQueries();
        wax_hip::check(wax_hip_search_batch(e->raw(), flat.data(), NQ, m.dims, 7, ids.data(), sc.data(), stride, counts.data()));
        for (uint32_t i = 0; i < NQ; ++i) {
            Hits got;
            for (uint32_t j = 0; j < counts[i] && j < stride; ++j) got.push_back({ids[i * stride + j], sc[i * stride + j]});
            const std::string d = compare(got, per_query[i]);
            if (!d.empty()) return fmt("query %u: ", i) + d;
        }
        return "";
    });
    expect(pfx + "c.search_batch_hits_to_results", [&]() -> std::string {
        const uint32_t stride = 8;
        std::vector<wax_hip_hit> hits(NQ * stride);
        std::vector<uint32_t> counts(NQ);
        const std::vector<float> flat = flatQueries();
        wax_hip::check(wax_hip_search_batch_hits(e->raw(), flat.data(), NQ, m.dims, 7, hits.data(), stride, counts.data()));
        for (uint32_t i = 0; i < NQ; ++i) {
            if (counts[i] != 7 || hits[i * stride + 7].key != INT64_MAX) return fmt("query %u: count %u, or no padding behind it", i, counts[i]);
            for (uint32_t j = 0; j + 1 < 7; ++j) if (hits[i * stride + j].key >= hits[i * stride + j + 1].key) return fmt("query %u: keys do not ascend", i);
            std::vector<uint64_t> ids(stride);
            std::vector<float> sc(stride);
            uint32_t n = 0;
            wax_hip::check(wax_hip_hits_to_results((uint8_t)m.metric, hits.data() + i * stride, stride, ids.data(), sc.data(), &n));
            Hits got;
            for (uint32_t j = 0; j < n; ++j) got.push_back({ids[j], sc[j]});
            std::string d = compare(got, per_query[i]);
            for (uint32_t j = 0; j < n && d.empty(); ++j)
                if ((long)(hits[i * stride + j].key & 0xffffffff) != m.find(ids[j])) d = fmt("hit %u: the key's row is not the frame's", j);
            if (!d.empty()) return fmt("query %u: ", i) + d;
        }
        return "";
    });
    Spec p;
    p.q = q(2); p.topK = 10; p.pred = &pBoth;
    const float pcut = mid_cut(m, p, 6, pfx + "c.search_predicate_submit");
    p.minScore = &pcut;
    const Expected pexp = model_search(m, p, pfx + "c.search_predicate_submit");
    expect(pfx + "c.search_predicate_submit", [&]() -> std::string {
        wax_hip_predicate_ticket_stats_t b{}, a{};
        wax_hip::check(wax_hip_predicate_ticket_stats(e->raw(), &b));
        uint64_t t = 0;
        wax_hip::check(wax_hip_search_predicate_submit(e->raw(), q(2), m.dims, 10, 1, pcut, &pBoth, &t));
        std::vector<uint64_t> ids(10);
        std::vector<float> sc(10);
        uint32_t n = 0;
        wax_hip::check(wax_hip_search_collect(e->raw(), t, ids.data(), sc.data(), 10, &n));
        wax_hip::check(wax_hip_predicate_ticket_stats(e->raw(), &a));
        Hits got;
        for (uint32_t i = 0; i < n; ++i) got.push_back({ids[i], sc[i]});
        std::string d = compare(got, pexp);
        if (d.empty()) d = same_bits(got, e->searchPredicate(qv(2), 10, nullptr, &pcut, pBoth), "ticket against searchPredicate");
        if (d.empty() && a.submitted - b.submitted != 1) d = fmt("submitted moved by %llu", (unsigned long long)(a.submitted - b.submitted));
        if (d.empty() && (a.rode - b.rode) + (a.deferred - b.deferred) + (a.host_decided - b.host_decided) != 1) d = "the ticket is in none of rode / deferred / host_decided";
        return d;
    });
    expect(pfx + "c.reserve_stats", [&]() -> std::string {
        wax_hip_stats_t b{}, a{};
        wax_hip::check(wax_hip_stats(e->raw(), &b));
        const uint64_t want = b.reserved_rows + 100;
        wax_hip::check(wax_hip_reserve(e->raw(), want));
        const Hits h1 = e->search(qv(0), 10);
        wax_hip::check(wax_hip_stats(e->raw(), &a));
        if (a.reserved_rows < want || e->count() != m.n()) return fmt("reserved %llu after reserve(%llu)", (unsigned long long)a.reserved_rows, (unsigned long long)want);
        if (a.searches - b.searches != 1 || a.rows_scanned - b.rows_scanned != m.n() || a.bytes_scanned - b.bytes_scanned != (uint64_t)m.n() * m.dims * 4)
            return fmt("one search moved searches by %llu, rows_scanned by %llu", (unsigned long long)(a.searches - b.searches), (unsigned long long)(a.rows_scanned - b.rows_scanned));
        e->reserve(a.reserved_rows * 2 + 1);                                                   // the wrapper's member, through growth
        wax_hip::check(wax_hip_stats(e->raw(), &a));
        if (a.reserved_rows < want * 2 + 1) return "the wrapper's reserve did not grow the store";
        std::string d = compare(h1, plain);
        if (d.empty()) d = same_bits(h1, e->search(qv(0), 10), "search across reserve");
        return d;
    });
    const std::vector<const std::vector<uint64_t>*> mixed{nullptr, &allowEmpty, &allowSome, &allowAbsent};
    expect(pfx + "c.set_get_tuning", [&]() -> std::string {
        if (wax_hip_get_tuning(e->raw(), "filter_batch") != 1) return "filter_batch does not default to 1";
        wax_hip::check(wax_hip_set_tuning(e->raw(), "filter_batch", 0));
        if (wax_hip_get_tuning(e->raw(), "filter_batch") != 0) return "filter_batch did not take 0";
        if (wax_hip_set_tuning(e->raw(), "no_such_key", 1) == WAX_HIP_OK) return "an unknown key was accepted";
        return "";
    });
    batch("c.tuning_changes_no_answer", 1, 10, mixed, nullptr, {}, {});
    expect(pfx + "c.tuning_restored", [&]() -> std::string {
        wax_hip::check(wax_hip_set_tuning(e->raw(), "filter_batch", 1));
        return wax_hip_get_tuning(e->raw(), "filter_batch") == 1 ? "" : "filter_batch did not take 1";
    });
    expect(pfx + "c.metric_device_of", [&]() -> std::string {
        const int dev = wax_hip_device_of(e->raw());
        if (wax_hip_metric_of(e->raw()) != (uint8_t)m.metric) return "metric_of";
        if (dev < 0 || dev >= wax_hip_device_count()) return fmt("device_of %d of %d", dev, wax_hip_device_count());
        return wax_hip_shard_count(e->raw()) == 1 && wax_hip_abi_version() == WAX_HIP_ABI_VERSION ? "" : "shard_count / abi_version";
    });
}

/// The same store on a two-shard handle (both shards on device 0): one search, one timeline and one batched term search equal the
/// single engine's.
void Bench::sharded() {
    expect(pfx + "c.sharded", [&]() -> std::string {
        const int devices[2] = {0, 0};
        wax_hip_engine* h = nullptr;
        wax_hip::check(wax_hip_engine_create_sharded((uint8_t)m.metric, m.dims, devices, 2, &h));
        struct Guard { wax_hip_engine* h; ~Guard() { wax_hip_engine_destroy(h); } } guard{h};
        wax_hip::check(wax_hip_set_tuning(h, "shard_min_mb", 0));
        wax_hip::check(wax_hip_add_batch(h, m.ids.data(), m.rows.data(), m.n(), m.dims));
        wax_hip::check(wax_hip_set_attributes(h, m.ids.data(), m.ts.data(), m.flags.data(), m.n(), nullptr));
        std::vector<uint64_t> tb(m.n());
        std::vector<uint32_t> tl(m.n()), tf;
        for (size_t r = 0; r < m.n(); ++r) { tb[r] = tf.size(); tl[r] = (uint32_t)m.terms[r].size(); tf.insert(tf.end(), m.terms[r].begin(), m.terms[r].end()); }
        wax_hip::check(wax_hip_set_terms(h, m.ids.data(), tb.data(), tl.data(), tf.data(), tf.size(), m.n(), nullptr));
        if (wax_hip_shard_count(h) != 2 || wax_hip_count(h) != m.n()) return fmt("%d shards, %llu rows", wax_hip_shard_count(h), (unsigned long long)wax_hip_count(h));
        uint64_t next_base = 0;
        for (int g = 0; g < 2; ++g) {
            int dev = -1;
            uint64_t base = 0, rows = 0;
            wax_hip::check(wax_hip_shard_info(h, g, &dev, &base, &rows));
            if (dev != 0 || base != next_base || rows == 0) return fmt("shard %d: device %d, base %llu, rows %llu", g, dev, (unsigned long long)base, (unsigned long long)rows);
            next_base += rows;
        }
        if (next_base != m.n()) return "the shards do not add up to the store";
        std::vector<uint64_t> ids(NQ * 10);
        std::vector<float> sc(NQ * 10);
        uint32_t n = 0;
        wax_hip::check(wax_hip_search(h, q(0), m.dims, 10, ids.data(), sc.data(), 10, &n));
        Hits got;
        for (uint32_t i = 0; i < n; ++i) got.push_back({ids[i], sc[i]});
        std::string d = same_bits(got, e->search(qv(0), 10), "sharded search");
        if (!d.empty()) return d;
        std::vector<uint64_t> tids(30);
        std::vector<int64_t> tts(30);
        wax_hip::check(wax_hip_timeline(h, 30, 1, &pBoth, tids.data(), tts.data(), 30, &n));
        Timeline tgot;
        for (uint32_t i = 0; i < n; ++i) tgot.push_back({tids[i], tts[i]});
        d = compare_timeline(tgot, e->timeline(30, true, &pBoth));
        if (!d.empty()) return "sharded timeline: " + d;
        const std::vector<wax_hip_row_predicate> preds = predsMixed();
        const std::vector<std::vector<uint32_t>> req = requiredMixed();
        std::vector<uint64_t> rb(NQ);
        std::vector<uint32_t> rl(NQ), rf;
        for (uint32_t i = 0; i < NQ; ++i) { rb[i] = rf.size(); rl[i] = (uint32_t)req[i].size(); rf.insert(rf.end(), req[i].begin(), req[i].end()); }
        std::vector<uint32_t> counts(NQ);
        const std::vector<float> flat = flatQueries();
        wax_hip::check(wax_hip_search_batch_terms(h, flat.data(), NQ, m.dims, 10, nullptr, 0, nullptr, nullptr, nullptr, preds.data(), rf.data(), rf.size(), rb.data(),
                                                  rl.data(), ids.data(), sc.data(), 10, counts.data()));
        const auto single = e->searchBatchTerms(flat, NQ, 10, {}, nullptr, preds, req);
        for (uint32_t i = 0; i < NQ; ++i) {
            Hits row;
            for (uint32_t j = 0; j < counts[i]; ++j) row.push_back({ids[i * 10 + j], sc[i * 10 + j]});
            d = same_bits(row, single[i], "sharded searchBatchTerms");
            if (!d.empty()) return fmt("query %u: ", i) + d;
        }
        return "";
    });
}

void Bench::mutations() {
    // removeBatch: held ids (some twice) and ids the engine never held
    std::vector<uint64_t> gone;
    for (size_t r = 2; r < m.n(); r += 10) gone.push_back(m.ids[r]);
    gone.push_back(gone[0]); gone.push_back(gone[3]); gone.push_back(3); gone.push_back(300000);
    size_t removed = 0;
    for (uint64_t id : gone) { const long r = m.find(id); if (r >= 0) { erase_row(m, (size_t)r); ++removed; } }
    expect(pfx + "removeBatch", [&] {
        const uint64_t got = e->removeBatch(gone);
        return got == removed && e->removeBatch({}) == 0 && e->count() == m.n() ? std::string() : fmt("removed %llu, model %zu", (unsigned long long)got, removed);
    });
    every_kind("after_removeBatch");

    const uint64_t one = m.ids[m.n() / 2];
    erase_row(m, m.n() / 2);
    expect(pfx + "remove", [&] {
        e->remove(one);
        e->remove(one);                                                   // an absent id is a no-op
        return e->count() == m.n() ? std::string() : fmt("count %llu, model %zu", (unsigned long long)e->count(), m.n());
    });
    every_kind("after_remove");

    // add as an upsert: the row keeps its place, its attributes, its parent and its terms; a new id is appended with none
    const size_t ur = 7;
    const uint64_t uid = m.ids[ur], nid = nextId++ * 3 + 5;
    std::vector<double> sc;
    const std::vector<float> uv = draw_row(rng, m, (long)ur, &sc);
    upsert(m, uid, uv, sc);
    const std::vector<float> nv = draw_row(rng, m, -1, &sc);
    upsert(m, nid, nv, sc);
    expect(pfx + "add_upsert", [&]() -> std::string {
        e->add(uid, uv);
        e->add(nid, nv);
        if (e->count() != m.n()) return fmt("count %llu, model %zu", (unsigned long long)e->count(), m.n());
        const auto at = e->getAttributes({uid, nid});
        const auto pa = e->getParents({uid, nid});
        if (!at[0].found || at[0].timestamp != m.ts[ur] || at[0].flags != m.flags[ur] || pa[0].first != m.parent[ur] || e->getTerms(uid) != m.terms[ur])
            return "the upserted row lost a column";
        if (!at[1].found || at[1].timestamp != 0 || at[1].flags != 0 || pa[1].first != WAX_HIP_NO_PARENT || !e->getTerms(nid).empty())
            return "the appended row does not read (0, 0), no parent, no terms";
        return "";
    });
    every_kind("after_add");

    // pending-embedding replay: held and new frames, one of them twice (the later record wins), as one byte stream
    std::vector<uint8_t> wal;
    std::vector<uint64_t> wal_ids{m.ids[11], nextId++ * 3 + 5, m.ids[200], nextId++ * 3 + 5, m.ids[11]};
    for (uint64_t id : wal_ids) {
        const std::vector<float> v = draw_row(rng, m, m.find(id), &sc);
        upsert(m, id, v, sc);
        append_wal(wal, id, v);
    }
    expect(pfx + "applyPutEmbeddings", [&]() -> std::string {
        const uint64_t applied = e->applyPutEmbeddings(wal.data(), wal.size());
        if (applied != wal_ids.size() || e->count() != m.n()) return fmt("applied %llu of %zu, count %llu, model %zu", (unsigned long long)applied, wal_ids.size(), (unsigned long long)e->count(), m.n());
        std::vector<uint8_t> bad(wal);
        bad.push_back(0x04); bad.push_back(1);                           // a truncated record: the stream changes nothing
        return throws<wax_hip::Error>([&] { e->applyPutEmbeddings(bad.data(), bad.size()); }, WAX_HIP_ERR_BAD_SEGMENT);
    });
    build_lists();
    every_kind("after_applyPutEmbeddings");
}

void Bench::persistence() {
    Store bare = m;
    for (size_t r = 0; r < bare.n(); ++r) { bare.ts[r] = 0; bare.flags[r] = 0; bare.parent[r] = WAX_HIP_NO_PARENT; bare.terms[r].clear(); }
    std::unique_ptr<VectorEngine> e2;
    if (LIVE) e2.reset(new VectorEngine((wax_hip_metric)m.metric, m.dims));
    expect(pfx + "serialize_deserialize", [&]() -> std::string {
        const std::vector<uint8_t> blob = e->serialize();
        const size_t want = 36 + m.n() * m.dims * 4 + 8 + m.n() * 8;
        if (blob.size() != want || std::memcmp(blob.data(), "MV2V", 4) != 0) return fmt("%zu bytes, expected %zu", blob.size(), want);
        if (std::memcmp(blob.data() + 36, m.rows.data(), m.rows.size() * 4) != 0) return "the row block is not the model's rows";
        if (std::memcmp(blob.data() + 36 + m.rows.size() * 4 + 8, m.ids.data(), m.n() * 8) != 0) return "the id block is not the model's ids";
        e2->deserialize(blob);
        if (e2->count() != m.n() || e2->dimensions() != m.dims) return "count / dimensions after deserialize";
        return e2->serialize() == blob ? "" : "the second engine serializes differently";
    });
    expect(pfx + "deserialize.columns_never_set", [&]() -> std::string {
        const auto at = e2->getAttributes(m.ids);
        const auto pa = e2->getParents(m.ids);
        for (size_t r = 0; r < m.n(); ++r) {
            bool found = false;
            if (!at[r].found || at[r].timestamp != 0 || at[r].flags != 0 || !pa[r].second || pa[r].first != WAX_HIP_NO_PARENT || !e2->getTerms(m.ids[r], &found).empty() || !found)
                return fmt("row %zu still carries a column", r);
        }
        return "";
    });
    expect(pfx + "deserialize.searches_repeat", [&]() -> std::string {
        std::string d = same_bits(e2->search(qv(0), 300), e->search(qv(0), 300), "search");
        if (d.empty()) d = same_bits(e2->searchFiltered(qv(1), 10, &allowSome, nullptr), e->searchFiltered(qv(1), 10, &allowSome, nullptr), "searchFiltered");
        return d;
    });
    // every row of the second engine reads (0, 0), its own root, no terms: the same checks against the bare model
    std::swap(m, bare);
    std::swap(e, e2);
    Spec s;
    s.q = q(0); s.topK = 10;
    single("second.search", s, 0);
    s.allow = &allowSome;
    single("second.searchFiltered", s, 1);
    s.allow = nullptr; s.pred = &pDeny; s.filterMayBeTrivial = true;      // (0, 0) passes the deny bits: every row
    single("second.searchPredicate", s, 2);
    s.required = &termOne;                                                // no row holds a term any more
    single("second.searchTerms", s, 3);
    const std::vector<const std::vector<uint64_t>*> allow{nullptr, &allowEmpty, &allowSome, &allowAbsent};
    batch("second.searchBatchFiltered", 1, 10, allow, nullptr, {}, {});
    batch("second.searchBatchPredicate", 2, 10, allow, nullptr, predsMixed(), {}, true);
    batch("second.searchBatchTerms", 3, 10, allow, nullptr, predsMixed(), requiredMixed(), true);
    {
        const auto exp = model_grouped(m, q(4), 12, 3, nullptr, nullptr, pfx + "second.searchGrouped");
        expect(pfx + "second.searchGrouped", [&] { return compare_groups(m, e->searchGrouped(qv(4), 12, 3, nullptr, nullptr), exp); });
    }
    timeline("second.timeline", 30, true, nullptr);
    std::swap(m, bare);
    std::swap(e, e2);
}

void Bench::run(uint32_t dims, wax_hip_metric metric, const char* label) {
    pfx = std::string(label) + ".";
    const uint64_t seed = SEED + dims * 16 + (uint64_t)metric;
    m = make_store(seed, dims, metric, 1000, make_queries(seed, dims));
    rng = Rng(seed ^ 0xabcdef);
    nextId = 1000;
    build_lists();
    if (LIVE) {
        e.reset(new VectorEngine(metric, dims));
        // the first 600 rows in one batch, the rest in a second: the store grows once under the wrapper
        const size_t first = 600;
        e->addBatch(std::vector<uint64_t>(m.ids.begin(), m.ids.begin() + first), std::vector<float>(m.rows.begin(), m.rows.begin() + first * dims));
        e->addBatch({}, {});
        e->addBatch(std::vector<uint64_t>(m.ids.begin() + first, m.ids.end()), std::vector<float>(m.rows.begin() + first * dims, m.rows.end()));
    }
    plain_and_filtered();
    attributes_and_predicates();
    parents_and_groups();
    terms();
    batches();
    timelines();
    unwrapped();
    sharded();
    mutations();
    persistence();
    e.reset();
}

// ---- many stores in one pass ---------------------------------------------------------------------------------------------------------
void many_stores() {
    const uint32_t dims = 64;
    const std::string pfx = "many.";
    const auto queries = make_queries(SEED + 99, dims);
    std::vector<Store> stores;
    for (uint64_t i = 0; i < 3; ++i) stores.push_back(make_store(SEED + 1000 + i, dims, WAX_HIP_METRIC_COSINE, 300, queries));
    Store empty;
    empty.dims = dims; empty.metric = WAX_HIP_METRIC_COSINE;
    stores.push_back(empty);
    Rng rng(SEED + 5);
    for (size_t i = 0; i < 2; ++i)                                          // the third store never gets attributes: it reads (0, 0)
        for (size_t r = 0; r < stores[i].n(); ++r) { stores[i].ts[r] = (int64_t)rng.below(50); stores[i].flags[r] = (uint32_t)rng.below(8); }
    const size_t pair_store[NQ] = {0, 1, 0, 2, 3};                          // store 0 twice, the empty one last
    std::vector<std::unique_ptr<VectorEngine>> engines;
    std::vector<VectorEngine*> pairs;
    if (LIVE) {
        for (auto& st : stores) {
            engines.emplace_back(new VectorEngine(WAX_HIP_METRIC_COSINE, dims));
            engines.back()->addBatch(st.ids, st.rows);
            bool any = false;
            for (uint32_t f : st.flags) any = any || f;
            if (any) engines.back()->setAttributes(st.ids, &st.ts, &st.flags);
        }
        for (size_t i = 0; i < NQ; ++i) pairs.push_back(engines[pair_store[i]].get());
    }
    std::vector<float> flat;
    for (const auto& qv : queries) flat.insert(flat.end(), qv.begin(), qv.end());
    const std::vector<wax_hip_row_predicate> preds{make_pred(true, 10, true, 40, 0), make_pred(false, 0, false, 0, 1), make_pred(false, 0, false, 0, 0),
                                                   make_pred(false, 0, true, 5, 6), make_pred(true, 1, false, 0, 0)};
    for (int mode = 0; mode < 4; ++mode) {
        // 0 searchMany; 1 searchManyFiltered with predicates; 2 with predicates and cuts; 3 with neither (IS searchMany)
        const std::string name = pfx + (mode == 0 ? "searchMany" : mode == 1 ? "searchManyFiltered.preds" : mode == 2 ? "searchManyFiltered.preds_cuts" : "searchManyFiltered.plain");
        const int topK = mode == 0 ? 400 : 10;                              // 400 > the 300 rows of a store: counts below the stride
        std::vector<float> cuts(NQ, std::numeric_limits<float>::quiet_NaN());
        std::vector<Spec> specs(NQ);
        std::vector<Expected> exps;
        for (size_t i = 0; i < NQ; ++i) {
            Spec& s = specs[i];
            s.q = queries[i].data(); s.topK = topK;
            if (mode == 1 || mode == 2) { s.pred = &preds[i]; s.filterMayBeTrivial = i >= 2; }
            if (mode == 2 && i < 2) { cuts[i] = mid_cut(stores[pair_store[i]], s, 4, name); s.minScore = &cuts[i]; }
            exps.push_back(model_search(stores[pair_store[i]], s, name + fmt("[pair %zu]", i)));
        }
        expect(name, [&]() -> std::string {
            std::vector<Hits> got;
            if (mode == 0) got = wax_hip::searchMany(pairs, flat, topK);
            else if (mode == 1) got = wax_hip::searchManyFiltered(pairs, flat, topK, preds);
            else if (mode == 2) got = wax_hip::searchManyFiltered(pairs, flat, topK, preds, cuts);
            else got = wax_hip::searchManyFiltered(pairs, flat, topK, {});
            if (got.size() != NQ) return "one row per pair";
            for (size_t i = 0; i < NQ; ++i) {
                std::string d = compare(got[i], exps[i]);
                if (d.empty()) {
                    const std::vector<float> qi(queries[i]);
                    const Hits alone = mode == 0 || mode == 3 ? pairs[i]->search(qi, topK)
                                                               : pairs[i]->searchPredicate(qi, topK, nullptr, mode == 2 && i < 2 ? &cuts[i] : nullptr, preds[i]);
                    d = same_bits(got[i], alone, "against the engine's own search");
                }
                if (!d.empty()) return fmt("pair %zu: ", i) + d;
            }
            return "";
        });
    }
    expect(pfx + "searchManyFiltered.wrong_lengths", [&]() -> std::string {
        std::string d = throws<std::invalid_argument>([&] { wax_hip::searchManyFiltered(pairs, flat, 10, {preds[0]}); });
        if (d.empty()) d = throws<std::invalid_argument>([&] { wax_hip::searchManyFiltered(pairs, flat, 10, {}, {0.5f}); });
        if (d.empty() && !wax_hip::searchMany({}, {}, 10).empty()) d = "no pairs, yet rows";
        return d;
    });
}

// ---- rank fusion ------------------------------------------------------------------------------------------------------------------
void rank_fusion() {
    // the rule at the top of rrf.hip: lanes in order, a lane of weight <= 0 skipped, position p adds weight / Float(max(0, k) + p + 1)
    // in f32 (lane order, then position order); bestRank = smallest p + 1; sorted by (score desc, bestRank asc, frameId asc)
    Rng rng(SEED + 77);
    const float weights[4] = {1.0f, 0.5f, 0.0f, 0.7f};
    const uint32_t lens[4] = {40, 25, 10, 30};
    std::vector<std::vector<uint64_t>> lists(4);
    for (int l = 0; l < 4; ++l)
        for (uint32_t p = 0; p < lens[l]; ++p) lists[(size_t)l].push_back(l == 2 ? 5000 + p : 5 + 3 * rng.below(60));   // lane 2's ids occur nowhere else
    const int32_t k = 60;
    struct Fused { uint64_t id; float score; uint32_t best, sources; };
    std::vector<Fused> exp;
    for (uint32_t l = 0; l < 4; ++l) {
        if (!(weights[l] > 0.0f)) continue;
        for (uint32_t p = 0; p < lists[l].size(); ++p) {
            const float add = weights[l] / (float)(std::max(0, k) + (int32_t)p + 1);
            auto it = std::find_if(exp.begin(), exp.end(), [&](const Fused& f) { return f.id == lists[l][p]; });
            if (it == exp.end()) exp.push_back({lists[l][p], add, p + 1, 1u << l});
            else { it->score += add; it->best = std::min(it->best, p + 1); it->sources |= 1u << l; }
        }
    }
    std::sort(exp.begin(), exp.end(), [](const Fused& a, const Fused& b) {
        if (a.score != b.score) return a.score > b.score;
        if (a.best != b.best) return a.best < b.best;
        return a.id < b.id;
    });
    expect("rrf.fuse", [&]() -> std::string {
        const uint64_t* ptrs[4] = {lists[0].data(), lists[1].data(), lists[2].data(), lists[3].data()};
        for (uint32_t cap : {(uint32_t)128, (uint32_t)7}) {
            std::vector<uint64_t> ids(cap + 1, 4242);
            std::vector<float> sc(cap);
            std::vector<uint32_t> best(cap), src(cap);
            uint32_t n = 0;
            wax_hip::check(wax_hip_rrf_fuse(weights, ptrs, lens, 4, k, -1, ids.data(), sc.data(), best.data(), src.data(), cap, &n));
            const size_t want = std::min((size_t)cap, exp.size());
            if (n != want || ids[cap] != 4242) return fmt("%u results into %u entries, model %zu", n, cap, want);
            for (size_t i = 0; i < want; ++i)
                if (ids[i] != exp[i].id || std::memcmp(&sc[i], &exp[i].score, 4) != 0 || best[i] != exp[i].best || src[i] != exp[i].sources)
                    return fmt("entry %zu: (%llu, %.9g, %u, %u), model (%llu, %.9g, %u, %u)", i, (unsigned long long)ids[i], (double)sc[i], best[i], src[i],
                               (unsigned long long)exp[i].id, (double)exp[i].score, exp[i].best, exp[i].sources);
        }
        return "";
    });
}

void wrapper_basics() {
    expect("wrapper.check_and_error", [&]() -> std::string {
        wax_hip::check(WAX_HIP_OK);
        wax_hip_engine* h = nullptr;
        const int rc = wax_hip_engine_create(WAX_HIP_METRIC_COSINE, 0, -1, &h);   // dimensions must be > 0: refused before any device work
        if (rc == WAX_HIP_OK) { wax_hip_engine_destroy(h); return "an engine of 0 dimensions was created"; }
        std::string d = throws<wax_hip::Error>([&] { wax_hip::check(rc); }, rc);
        if (d.empty()) d = throws<wax_hip::Error>([&] { VectorEngine bad(WAX_HIP_METRIC_COSINE, 0); }, rc);
        if (d.empty() && !VectorEngine::isAvailable()) d = "isAvailable is false on a device";
        if (d.empty() && (wax_hip_result_capacity(0) != 1 || wax_hip_result_capacity(50000) != WAX_HIP_MAX_RESULTS)) d = "result_capacity";
        return d;
    });
    expect("wrapper.empty_engine", [&]() -> std::string {
        VectorEngine e(WAX_HIP_METRIC_L2, 20);
        const std::vector<float> q(20, 0.25f);
        if (e.count() != 0 || !e.search(q, 5).empty() || !e.searchFiltered(q, 5, nullptr, nullptr).empty() || !e.timeline(5, true, nullptr).empty() ||
            !e.searchGrouped(q, 5, 2, nullptr, nullptr).empty())
            return "an empty engine answers something";
        return throws<wax_hip::Error>([&] { e.add(1, std::vector<float>(19, 1.0f)); }, WAX_HIP_ERR_DIM_MISMATCH);
    });
}

void run_all() {
    wrapper_basics();
    const std::pair<uint32_t, const char*> dimsets[] = {{64, "d64"}, {20, "d20"}};
    const std::pair<wax_hip_metric, const char*> metrics[] = {{WAX_HIP_METRIC_COSINE, "cosine"}, {WAX_HIP_METRIC_DOT, "dot"}, {WAX_HIP_METRIC_L2, "l2"}};
    for (const auto& d : dimsets)
        for (const auto& mt : metrics) {
            Bench b;
            b.run(d.first, mt.first, (std::string(d.second) + "." + mt.second).c_str());
        }
    many_stores();
    rank_fusion();
}

}  // namespace

int main(int argc, char** argv) {
    int a = 1;
    if (a < argc && std::strcmp(argv[a], "--model-only") == 0) { LIVE = false; ++a; }
    if (argc - a != 2) { std::printf("usage: consumer [--model-only] SCORE_TOL TIE_TOL\n"); return 2; }
    SCORE_TOL = std::atof(argv[a]);
    TIE_TOL = std::atof(argv[a + 1]);
    if (!(SCORE_TOL > 0) || !(TIE_TOL > 0)) { std::printf("the tolerances must be positive\n"); return 2; }
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    try {
        if (LIVE) {
            // the input conditions of EVERY check are asserted by a silent pass of the model before an engine exists
            LIVE = false; QUIET = true;
            run_all();
            LIVE = true; QUIET = false;
            n_checks = 0;
            VectorEngine probe(WAX_HIP_METRIC_COSINE, 4);                    // without a device this throws NO_DEVICE
        }
        run_all();
    } catch (const wax_hip::Error& err) {
        if (!VectorEngine::isAvailable() && err.status == WAX_HIP_ERR_NO_DEVICE && std::strlen(err.what()) > 0) {
            std::printf("no-device: %s\n", err.what());
            return 0;
        }
        std::printf("unexpected error %d: %s\n", err.status, err.what());
        return 9;
    } catch (const std::exception& err) {
        std::printf("unexpected exception: %s\n", err.what());
        return 10;
    }
    if (!LIVE) { std::printf("model ok: %d checks\n", n_checks); return 0; }
    std::printf("checks %d failed %d\n", n_checks, n_failed);
    return n_failed ? 1 : 0;
}
