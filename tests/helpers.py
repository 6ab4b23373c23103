"""Shared test infrastructure: an oracle-backed engine with the reference's store semantics,
the reference-case runner, and the parity comparison rule of SURVEY.md §8c."""
from __future__ import annotations

import json
import os

import numpy as np

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METRIC_NAMES = {"cosine": 0, "dot": 1, "l2": 2}


def load_golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


class OracleDimensionMismatch(Exception):
    pass


class OracleEngine:
    """CPU stand-in with MetalVectorEngine's store semantics (a9): upsert by frameId
    (MetalVectorEngine.swift:330-402), order-preserving remove (:423-444), MV2V serialize
    (:682-714) — search through oracle.search. TEST INFRASTRUCTURE ONLY."""

    def __init__(self, metric=0, dimensions=0, mode=oracle.MODE_TRUTH_F64):
        self.metric, self.dimensions, self.mode = int(metric), int(dimensions), mode
        self.rows, self.ids = [], []
        self.allocs, self.reuse = 1, 0

    @property
    def count(self):
        return len(self.ids)

    def add(self, frameId, vector):
        self.addBatch([frameId], [vector])

    def addBatch(self, frameIds, vectors):
        if len(frameIds) != len(vectors):
            raise ValueError("addBatch: frameIds.count != vectors.count")
        for v in vectors:
            if len(v) != self.dimensions:
                raise OracleDimensionMismatch(f"vector dimension mismatch: expected {self.dimensions}, got {len(v)}")
        for fid, v in zip(frameIds, vectors):
            v = np.asarray(v, dtype=np.float32)
            if fid in self.ids:
                self.rows[self.ids.index(fid)] = v  # firstIndex(of:) (:385)
            else:
                self.ids.append(int(fid))
                self.rows.append(v)

    def remove(self, frameId):
        if frameId in self.ids:
            i = self.ids.index(frameId)
            del self.ids[i]
            del self.rows[i]

    def matrix(self):
        if not self.rows:
            return np.zeros((0, self.dimensions), dtype=np.float32)
        return np.stack(self.rows).astype(np.float32)

    def searchFilteredHits(self, vector, topK, allow):
        """The reference's vector lane under FrameFilter(frameIds:): candidateLimit results from the engine
        (UnifiedSearch.swift:1195-1200), post-filtered by the allow-list (:1250), first topK kept."""
        if topK <= 0:
            return []
        limit = max(topK, min(topK * 3, 1000))
        allowed = set(int(a) for a in allow)
        return [h for h in self.search(vector, limit) if h[0] in allowed][:topK]

    def search(self, vector, topK):
        if self.count == 0:
            return []
        self.reuse += 1
        try:
            ids, scores, _, _ = oracle.search(self.metric, self.matrix(), np.array(self.ids, dtype=np.uint64),
                                              np.asarray(vector, dtype=np.float32), topK, self.mode)
        except oracle.DimensionMismatch as e:
            raise OracleDimensionMismatch(str(e))
        return [(int(i), float(s)) for i, s in zip(ids, scores)]

    def serialize(self):
        return oracle.mv2v_serialize(self.metric, self.matrix().reshape(self.count, self.dimensions),
                                     np.array(self.ids, dtype=np.uint64))

    def deserialize(self, data):
        rc, vec, ids = oracle.mv2v_parse(data, self.metric, self.dimensions)
        if rc not in (0,):
            raise ValueError(f"bad segment (check {rc})")
        self.rows = [r for r in vec]
        self.ids = [int(i) for i in ids]

    def debugBufferPoolStats(self):
        class S:
            pass
        s = S()
        s.transientAllocations, s.reuseCount = self.allocs, self.reuse
        return s


def run_reference_case(case, make_engine, normalize):
    """Replays one transcribed reference test against an engine factory and checks the
    reference's own assertions. `normalize(vec)` is the caller-side VectorMath.normalizeL2."""
    metric = METRIC_NAMES[case["metric"]]
    eng = make_engine(metric, case["dimensions"])
    saved = {}
    for op in case["ops"]:
        kind = op["op"]
        exp = op.get("expect", {})
        if kind == "add":
            eng.add(op["frameId"], op["vector"])
        elif kind == "addBatch":
            eng.addBatch(op["frameIds"], op["vectors"])
        elif kind == "remove":
            eng.remove(op["frameId"])
        elif kind == "serialize_deserialize_into_new_engine":
            blob = eng.serialize()
            if exp.get("blobNonEmpty"):
                assert len(blob) > 0
            eng2 = make_engine(metric, case["dimensions"])
            eng2.deserialize(blob)
            eng = eng2
        elif kind == "search":
            q = op["vector"]
            if op.get("normalizeQueryLikeCaller"):
                q = list(normalize(q))
            hits = eng.search(q, op["topK"])
            ids = [h[0] for h in hits]
            if exp.get("nonEmpty"):
                assert hits, case["name"]
            for c in exp.get("contains", []):
                assert c in ids, (case["name"], ids)
            for c in exp.get("notContains", []):
                assert c not in ids, (case["name"], ids)
            if "first" in exp:
                assert hits and ids[0] == exp["first"], (case["name"], hits)
            scores = [h[1] for h in hits]
            assert scores == sorted(scores, reverse=True), (case["name"], scores)
            if "save" in op:
                saved[op["save"]] = hits
        elif kind == "search_filtered":
            hits = eng.searchFilteredHits(op["vector"], op["topK"], op["allow"])
            ids = [h[0] for h in hits]
            if "idSetEquals" in exp:
                assert set(ids) == set(exp["idSetEquals"]), (case["name"], ids)
            scores = [h[1] for h in hits]
            assert scores == sorted(scores, reverse=True), (case["name"], scores)
        elif kind == "compare_first_scores":
            a, b = saved[op["a"]][0][1], saved[op["b"]][0][1]
            assert abs(a - b) < op["tolerance"], (a, b)
        elif kind == "pool_stats":
            st = eng.debugBufferPoolStats()
            if "transientAllocationsEqual" in exp:
                assert st.transientAllocations == saved[exp["transientAllocationsEqual"]].transientAllocations
            if "reuseCountAtLeast" in exp:
                assert st.reuseCount >= saved[exp["reuseCountAtLeast"]].reuseCount
            if "save" in op:
                saved[op["save"]] = st
        else:
            raise AssertionError(f"unknown op {kind}")
    return eng


SCORE_TOL = 1e-5   # north_star: "match the reference CPU path's returned indices/scores within 1e-5"
TIE_TOL = 2e-5     # ids may permute only inside groups whose oracle scores differ < 2e-5


def assert_parity(got_ids, got_scores, exp_ids, exp_scores, all_exp_scores=None, ctx=""):
    """The parity rule of SURVEY.md §8c, as the GPU tests apply it.

    1. Scores: |got - expected| <= SCORE_TOL (1e-5, the north star's tolerance) position by position — ALWAYS, whatever
       the ids are. (The engine's f32 distances and the oracle's f64 truth differ by a few 1e-7 on unit-norm data.)
    2. Ids: identical lists pass. Otherwise the oracle ranking is cut into NEAR-TIE GROUPS: maximal runs of neighbouring
       oracle scores closer than TIE_TOL (2e-5 = twice the score tolerance: two rows that close can legitimately swap
       between an f32 and an f64 evaluation). Inside a group the ids may appear in any order; as SETS every group must
       match exactly.
    3. The boundary group. `all_exp_scores` carries the oracle's scores for k + margin results, so a run that starts
       inside the top k and continues PAST rank k is seen as such. For that group the engine may hold a different
       member of the run than the oracle does (which of several rows within 2e-5 of each other makes the cut is not
       decidable at the stated tolerance), so set equality cannot be demanded: the rule is that the engine returns as many
       DISTINCT ids in those positions as the oracle, and rule 1 still pins each of them to the oracle's score at that
       position within 1e-5 — an id from outside the tied run would fail rule 1. Without `all_exp_scores` the run is
       only followed to rank k and the boundary group is held to set equality like any other (the strict form; the
       full-size parity tests pass the margin, the exact-tie tests — duplicates, constant rows — do not need one because
       the engine's (distance asc, row asc) order is the oracle's parity-mode order there)."""
    got_ids = [int(x) for x in got_ids]
    exp_ids = [int(x) for x in exp_ids]
    assert len(got_ids) == len(exp_ids), f"{ctx}: count {len(got_ids)} != {len(exp_ids)}"
    gs = np.asarray(got_scores, dtype=np.float64)
    es = np.asarray(exp_scores, dtype=np.float64)
    assert np.all(np.abs(gs - es) <= SCORE_TOL), f"{ctx}: max score err {np.max(np.abs(gs - es)) if len(gs) else 0}"
    if got_ids == exp_ids:
        return
    # build near-tie groups over the oracle ranking
    ext = np.asarray(all_exp_scores if all_exp_scores is not None else exp_scores, dtype=np.float64)
    n = len(exp_ids)
    i = 0
    while i < n:
        j = i
        while j + 1 < len(ext) and abs(ext[j] - ext[j + 1]) < TIE_TOL:
            j += 1
        hi = min(j, n - 1)
        grp_exp = set(exp_ids[i:hi + 1])
        grp_got = set(got_ids[i:hi + 1])
        if j >= n:  # group straddles the k boundary: got may contain boundary-tied ids outside exp
            assert len(grp_got) == len(grp_exp), f"{ctx}: duplicate ids at boundary"
        else:
            assert grp_got == grp_exp, f"{ctx}: ids differ outside a tie group at rank {i}: {got_ids} vs {exp_ids}"
        i = hi + 1


def bf16_adversarial_unit_vector(dims, frac=0.99, roll=0):
    """(frac, roll: variants — every element loses frac * 2^-8 of itself, the non-zeros start at element `roll`.) A unit vector (f32) whose bf16 rounding moves its self-similarity by ~2^-7: every non-zero element is (1 + 0.99 * 2^-8) * 2^-e,
    just below a rounding midpoint at the bottom of its binade (so rounding takes 2^-8 of it away), with the exponents chosen
    greedily so that the squares sum to 1 — the normalisation the engine applies then changes nothing. ~20 non-zeros, rest 0."""
    import numpy as np
    a = 2.0 ** -8 * frac
    rem, exps = (1 + a) ** -2, []
    for e in range(1, 14):
        c = int(rem // 4.0 ** -e)
        c = min(c, 3 if e < 6 else 10 ** 9)
        exps += [e] * c
        rem -= c * 4.0 ** -e
    x = np.zeros(dims, dtype=np.float64)
    x[:len(exps)] = [(1 + a) * 2.0 ** -e for e in exps]
    return np.roll((x / np.sqrt(np.sum(x * x))).astype(np.float32), roll)


# ---------------------------------------------------------------------------
# constructions for the edges of the bf16 mirror's exactness argument (tests/test_mirror_edges_*.py)

THRESHOLD = np.float32(1e-6)   # CosineDistance.metal:323, as an f32 constant (9.99999997e-7)


def bf16_rne(x):
    """f32 -> bf16 (round to nearest, ties to even) -> f32, in numpy integer arithmetic. NaN stays NaN (quieted), inf stays inf,
    a finite value beyond the largest bf16 (above 3.3895e38) becomes inf, denormals round like any other value."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    nan = (b & 0x7fffffff) > 0x7f800000
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    r = np.where(nan, ((b >> 16) | 0x40) << 16, r)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def _unit_orthogonal(rng, qhat, count):
    """`count` unit vectors (f64) orthogonal to the unit vector qhat."""
    u = rng.standard_normal((count, qhat.size))
    u -= (u @ qhat)[:, None] * qhat[None, :]
    return u / np.linalg.norm(u, axis=1)[:, None]


ANTI_TOP = 100                 # rows of the sparse top
ANTI_TOP_COS = -0.0500005      # best cosine: -0.05 with room for the f32 rounding of the rows (every f64 cosine stays <= -0.05)
ANTI_TOP_STEP = 1e-3
ANTI_GAP, ANTI_SPREAD = 0.02, 0.3


def anti_correlated_corpus(n, dims, seed, zero_at=None):
    """(rows f32 [n, dims], query f32 [dims]): unit rows that all lie in the half-space opposite the unit query (whose component
    `zero_at`, if given, is exactly 0). The ANTI_TOP most
    similar rows have cosines ANTI_TOP_COS - i * 1e-3; every other row lies at least ANTI_GAP below the last of them, uniformly over
    a further ANTI_SPREAD. Rows are c * q + sqrt(1 - c^2) * u, u a unit vector orthogonal to q; their places in the store are shuffled."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(dims)
    if zero_at is not None:
        q[zero_at] = 0.0
    q = (q / np.linalg.norm(q)).astype(np.float32)
    qhat = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
    c = np.empty(n)
    c[:ANTI_TOP] = ANTI_TOP_COS - ANTI_TOP_STEP * np.arange(ANTI_TOP)
    floor = c[ANTI_TOP - 1] - ANTI_GAP
    c[ANTI_TOP:] = floor - ANTI_SPREAD * rng.random(n - ANTI_TOP)
    c = c[rng.permutation(n)]
    rows = c[:, None] * qhat[None, :] + np.sqrt(1.0 - c * c)[:, None] * _unit_orthogonal(rng, qhat, n)
    return np.ascontiguousarray(rows, dtype=np.float32), q


THRESHOLD_TOP_COS, THRESHOLD_COS_STEP = 0.955, 1e-3
THRESHOLD_ULPS = 32            # norms 1e-6 * (1 + j * 2^-24), j in -32 .. 32


def threshold_rows(q, count, dims, seed):
    """`count` f32 rows c_i * q^ + sqrt(1 - c_i^2) * u_i (u_i a unit vector orthogonal to q) with distinct cosines c_i = 0.955 - i * 1e-3,
    scaled so that their f64 norms are 1e-6 * (1 + j * 2^-24), j cycling through -32 .. 32: rows a few ulp on either side of the
    `sqrt(m) > 1e-6` rule. Returns (rows, cosines, j)."""
    rng = np.random.default_rng(seed)
    qhat = np.asarray(q, dtype=np.float64)
    qhat = qhat / np.linalg.norm(qhat)
    assert qhat.size == dims
    c = THRESHOLD_TOP_COS - THRESHOLD_COS_STEP * np.arange(count)
    j = (np.arange(count) % (2 * THRESHOLD_ULPS + 1)) - THRESHOLD_ULPS
    rows = c[:, None] * qhat[None, :] + np.sqrt(1.0 - c * c)[:, None] * _unit_orthogonal(rng, qhat, count)
    rows *= (1e-6 * (1.0 + j * 2.0 ** -24))[:, None]
    return np.ascontiguousarray(rows, dtype=np.float32), c, j


def _dpp_group_sum(v, group):
    """The engine's cross-lane sum tree over aligned groups of `group` lanes (quad swaps, half-row mirror, row mirror, row
    broadcasts), in f32 on an array [..., 64]; the group's total is read from its last lane."""
    v = np.asarray(v, dtype=np.float32)
    lane = np.arange(64)
    v = v + v[..., lane ^ 1]
    v = v + v[..., lane ^ 2]
    if group >= 8:
        v = v + v[..., (lane & ~7) | (7 - (lane & 7))]
    if group >= 16:
        v = v + v[..., (lane & ~15) | (15 - (lane & 15))]
    if group >= 32:
        add = np.where((lane >> 4) & 1, v[..., (lane & ~15) - 1], np.float32(0))
        v = v + add.astype(np.float32)
    if group >= 64:
        add = np.where(lane >= 32, v[..., np.full(64, 31)], np.float32(0))
        v = v + add.astype(np.float32)
    return v


def _fma32(a, b, c):
    """a * b + c rounded once to f32 (the product of two f32 is exact in f64; the f64 sum is then rounded to f32 — a double
    rounding that differs from a fused multiply-add only on rare half-way cases, which does not matter to what this is used for:
    showing that two f32 summation ORDERS disagree)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def f32_norm2_chain_order(rows):
    """sum x^2 in f32 the way a 64-lane strided scalar chain does it: lane l owns the float4s l, l + 64, ... of the row and adds
    x, y, z, w of each to ONE accumulator in turn; the 64 lanes are then summed by the cross-lane tree."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dims = rows.shape
    assert dims % 4 == 0
    d4 = dims // 4
    x = rows.reshape(n, d4, 4)
    acc = np.zeros((n, 64), dtype=np.float32)
    for base in range(0, d4, 64):
        w = min(64, d4 - base)
        for comp in range(4):
            v = x[:, base:base + w, comp]
            acc[:, :w] = _fma32(v, v, acc[:, :w])
    return _dpp_group_sum(acc, 64)[:, 63]


def f32_norm2_scan_order(rows, group):
    """sum x^2 in f32 the way the f32 scan does it: `group` lanes per row, lane g owns the float4s g, g + group, ... and keeps
    FOUR accumulators (one per component), summed (x + y) + (z + w), then the cross-lane tree over the group
    (group = 32 at 384 dims, 64 at 768)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dims = rows.shape
    d4 = dims // 4
    assert dims % 4 == 0 and d4 % group == 0
    x = rows.reshape(n, d4 // group, group, 4)
    acc = np.zeros((n, group, 4), dtype=np.float32)
    for jj in range(d4 // group):
        acc = _fma32(x[:, jj], x[:, jj], acc)
    lane_sum = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    full = np.zeros((n, 64), dtype=np.float32)
    full[:, 64 - group:] = lane_sum
    return _dpp_group_sum(full, group)[:, 63]
