"""HIPVectorEngine — host-side mirror of the reference's `VectorSearchEngine` protocol
(Sources/WaxVectorSearch/VectorSearchEngine.swift:10-18) and of `MetalVectorEngine`'s concrete
surface (MetalVectorEngine.swift:144-146, 153, 318, 404, 682, 716), bound to libwaxhip's C ABI.

Method and argument names follow the Swift API (`search(vector:topK:)`, `addBatch(frameIds:vectors:)`
...) so the parity tests read like the reference's own tests. Everything that computes runs in the
HIP library; this file only marshals arguments. No CPU fallback exists.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .errors import EncodingError, InvalidToc, raise_for_status
from .vector_metric import VectorMetric

MAX_EMBEDDING_DIMENSIONS = 1_000_000  # Constants.maxEmbeddingDimensions (WaxCore/Constants.swift:51)
MAX_RESULTS = 10_000                  # MetalVectorEngine.maxResults (:18)
TIMELINE_MAX_LIMIT = 4096             # WAX_HIP_TIMELINE_MAX_LIMIT (include/wax_hip.h): the longest lane the fusion takes


def _as_f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _u64p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def pack_allow_lists(frameIds, nq: int):
    """Per-query allow-lists -> (flat u64 ids, begin, length) for wax_hip_search_batch_filtered. frameIds None: no lists (begin and
    length None). An entry None: no list (length NO_ALLOW_LIST). The same object given for several queries is packed once, so those
    queries share one (begin, length) and the library resolves their list once."""
    if frameIds is None:
        return np.zeros(0, dtype=np.uint64), None, None
    if len(frameIds) != nq:
        raise EncodingError("searchBatchFiltered: frameIds must hold one entry per query")
    begin = np.zeros(nq, dtype=np.uint64)
    length = np.full(nq, _abi.NO_ALLOW_LIST, dtype=np.uint64)
    parts, seen, off = [], {}, 0
    for q, lst in enumerate(frameIds):
        if lst is None:
            continue
        key = id(lst)
        if key not in seen:
            arr = np.ascontiguousarray(lst if isinstance(lst, np.ndarray) else list(lst), dtype=np.uint64).reshape(-1)
            seen[key] = (off, arr.size)
            parts.append(arr)
            off += arr.size
        begin[q], length[q] = seen[key]
    flat = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
    return np.ascontiguousarray(flat, dtype=np.uint64), begin, length


def clampTopK(topK: int) -> int:  # noqa: N802,N803 — MetalVectorEngine.clampTopK (:842-846)
    if topK < 1:
        return 1
    if topK > MAX_RESULTS:
        return MAX_RESULTS
    return int(topK)


class BufferPoolStats:
    """MetalVectorEngine.BufferPoolStats (:43-46)."""

    def __init__(self, transientAllocations: int, reuseCount: int):  # noqa: N803
        self.transientAllocations = transientAllocations
        self.reuseCount = reuseCount


class HIPVectorEngine:
    """MI355X brute-force vector engine (cosine / dot / l2) behind the VectorSearchEngine protocol."""

    # -- availability -------------------------------------------------------
    @staticmethod
    def isAvailable() -> bool:  # noqa: N802 — MetalVectorEngine.isAvailable (:144-146)
        return bool(_abi.lib().wax_hip_available())

    # -- lifecycle ----------------------------------------------------------
    def __init__(self, metric: VectorMetric = VectorMetric.cosine, dimensions: int = 0, device: int = -1,
                 devices: Optional[Sequence[int]] = None):
        """MetalVectorEngine.init(metric:dimensions:) (:153-274). `devices=[...]`: one engine row-sharded over several
        GPUs inside the library (wax_hip_engine_create_sharded): same API, same results."""
        self._lib = _abi.lib()
        self._h = ctypes.c_void_p()
        self.metric = VectorMetric(metric)
        self._dirty = False
        if dimensions < 0:
            raise InvalidToc("dimensions must be > 0")
        if devices is not None:
            devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            rc = self._lib.wax_hip_engine_create_sharded(int(self.metric), int(min(dimensions, 2**32 - 1)), devs, len(devices),
                                                         ctypes.byref(self._h))
        else:
            rc = self._lib.wax_hip_engine_create(int(self.metric), int(min(dimensions, 2**32 - 1)), int(device),
                                                 ctypes.byref(self._h))
        if rc != _abi.OK and rc == _abi.ERR_INVALID_ARGUMENT:
            raise InvalidToc(_abi.last_error())  # "dimensions must be > 0" is invalidToc in the reference (:155)
        raise_for_status(rc)
        self.dimensions = int(self._lib.wax_hip_dimensions(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.wax_hip_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @classmethod
    def load(cls, wax, metric: VectorMetric, dimensions: int, device: int = -1) -> "HIPVectorEngine":
        """MetalVectorEngine.load(from:metric:dimensions:) (:318-328): committed bytes, then pending WAL embeddings."""
        engine = cls(metric=metric, dimensions=dimensions, device=device)
        data = wax.readCommittedVecIndexBytes()
        if data is not None:
            engine.deserialize(data)
        for emb in wax.pendingEmbeddingMutations():
            engine.add(frameId=emb.frameId, vector=emb.vector)
        return engine

    # -- properties ---------------------------------------------------------
    @property
    def count(self) -> int:
        return int(self._lib.wax_hip_count(self._h))

    @property
    def device(self) -> int:
        return int(self._lib.wax_hip_device_of(self._h))

    @property
    def shardCount(self) -> int:  # noqa: N802
        return int(self._lib.wax_hip_shard_count(self._h))

    def shardInfo(self, shard: int) -> Tuple[int, int, int]:  # noqa: N802
        """(device ordinal, first global row, rows) of one shard."""
        dev = ctypes.c_int(0)
        base = ctypes.c_uint64(0)
        rows = ctypes.c_uint64(0)
        raise_for_status(self._lib.wax_hip_shard_info(self._h, int(shard), ctypes.byref(dev), ctypes.byref(base), ctypes.byref(rows)))
        return int(dev.value), int(base.value), int(rows.value)

    # -- mutation -----------------------------------------------------------
    def add(self, frameId: int, vector) -> None:  # noqa: N803
        """add(frameId:vector:) (:330-357): upsert by frame id."""
        v = _as_f32(vector).reshape(-1)
        rc = self._lib.wax_hip_add(self._h, int(frameId), _fp(v), v.size)
        raise_for_status(rc)
        self._dirty = True

    def addBatch(self, frameIds: Sequence[int], vectors) -> None:  # noqa: N802,N803
        """addBatch(frameIds:vectors:) (:359-402)."""
        n = len(frameIds)
        if n == 0:
            return  # :360
        if isinstance(vectors, np.ndarray) and vectors.ndim == 2:
            if vectors.shape[0] != n:
                raise EncodingError("addBatch: frameIds.count != vectors.count")
            mat = _as_f32(vectors)
            width = mat.shape[1]
        else:
            if len(vectors) != n:
                raise EncodingError("addBatch: frameIds.count != vectors.count")  # :361-363
            for vec in vectors:  # :367-370 — every vector validated before anything is written
                if len(vec) != self.dimensions:
                    raise EncodingError(f"vector dimension mismatch: expected {self.dimensions}, got {len(vec)}")
            mat = _as_f32(vectors).reshape(n, self.dimensions)
            width = self.dimensions
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64)
        rc = self._lib.wax_hip_add_batch(self._h, _u64p(ids), _fp(mat), n, width)
        raise_for_status(rc)
        self._dirty = True

    def addBatchStreaming(self, frameIds: Sequence[int], vectors, chunkSize: int = 256) -> None:  # noqa: N802,N803
        """addBatchStreaming(frameIds:vectors:chunkSize:) (:404-421)."""
        n = len(frameIds)
        if n == 0:
            return
        if len(vectors) != n:
            raise EncodingError("addBatchStreaming: frameIds.count != vectors.count")
        if n <= chunkSize:
            return self.addBatch(frameIds, vectors)
        for start in range(0, n, chunkSize):
            end = min(start + chunkSize, n)
            self.addBatch(frameIds[start:end], vectors[start:end])

    def addBatchDevice(self, frameIds, rows) -> None:  # noqa: N802,N803
        """Append rows that already live in this GPU's HBM (a torch tensor [n, dims] f32, contiguous)."""
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64)
        n = int(ids.size)
        if n == 0:
            return
        if tuple(rows.shape) != (n, self.dimensions):
            raise EncodingError(f"vector dimension mismatch: expected {self.dimensions}, got {int(rows.shape[-1])}")
        if not rows.is_contiguous() or str(rows.dtype) != "torch.float32":
            raise EncodingError("addBatchDevice: rows must be a contiguous float32 tensor")
        rc = self._lib.wax_hip_add_batch_device(self._h, _u64p(ids), ctypes.c_void_p(rows.data_ptr()), n,
                                                self.dimensions)
        raise_for_status(rc)
        self._dirty = True

    def applyPutEmbeddings(self, payloads: bytes) -> int:  # noqa: N802
        """Pending-embedding replay (UnifiedSearchEngineCache.swift:252-283): `payloads` is WAL putEmbedding entry
        payloads back to back (WALEntryCodec.swift:39-54); validated as a whole, applied as one addBatch.
        Returns the number of records applied."""
        data = bytes(payloads)
        applied = ctypes.c_uint64(0)
        rc = self._lib.wax_hip_apply_put_embeddings(self._h, data, len(data), ctypes.byref(applied))
        raise_for_status(rc)
        if applied.value:
            self._dirty = True
        return int(applied.value)

    @staticmethod
    def encodePutEmbedding(frameId: int, vector) -> bytes:  # noqa: N802,N803
        """WALEntryCodec.encode(.putEmbedding) (WALEntryCodec.swift:39-54): 0x04, u64 frameId, u32 dim, f32 LE."""
        v = np.ascontiguousarray(vector, dtype="<f4").reshape(-1)
        if v.size > 1_000_000:
            raise EncodingError("embedding dimension exceeds limit")
        return b"\x04" + int(frameId).to_bytes(8, "little") + int(v.size).to_bytes(4, "little") + v.tobytes()

    def remove(self, frameId: int) -> None:  # noqa: N803
        """remove(frameId:) (:423-444): order-preserving delete; unknown id is a no-op."""
        before = self.count
        rc = self._lib.wax_hip_remove(self._h, int(frameId))
        raise_for_status(rc)
        if self.count != before:
            self._dirty = True

    def removeBatch(self, frameIds: Sequence[int]) -> int:  # noqa: N802,N803
        """remove(frameId:) for many ids in one compaction pass (the loop of VectorSearchSession.swift:188-192 as one call):
        unknown ids are ignored, an id listed twice counts once, the surviving rows keep their order. Returns the rows removed."""
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64).reshape(-1)
        n = int(ids.size)
        if n == 0:
            return 0
        removed = ctypes.c_uint64(0)
        rc = self._lib.wax_hip_remove_batch(self._h, _u64p(ids), n, ctypes.byref(removed))
        raise_for_status(rc)
        if removed.value:
            self._dirty = True
        return int(removed.value)

    def reserve(self, rows: int) -> None:
        raise_for_status(self._lib.wax_hip_reserve(self._h, int(rows)))

    # -- search -------------------------------------------------------------
    def _result_capacity(self, topK: int) -> int:  # noqa: N803
        """Entries to allocate for one query's results. The row count is only a hint that keeps the arrays small on
        small engines (+64: room for rows added concurrently); the library is told the capacity and never writes
        past it, so a racing add can at worst truncate to the best `cap` results, never overflow."""
        return max(1, min(clampTopK(topK), self.count + 64))

    def searchArrays(self, vector, topK: int) -> Tuple[np.ndarray, np.ndarray]:  # noqa: N802,N803
        q = _as_f32(vector).reshape(-1)
        cap = self._result_capacity(topK)
        ids = np.empty(cap, dtype=np.uint64)
        scores = np.empty(cap, dtype=np.float32)
        got = ctypes.c_uint32(0)
        rc = self._lib.wax_hip_search(self._h, _fp(q), q.size, int(max(min(topK, 2**31 - 1), -2**31)), _u64p(ids),
                                      _fp(scores), cap, ctypes.byref(got))
        raise_for_status(rc)
        return ids[:got.value].copy(), scores[:got.value].copy()

    def searchFiltered(self, vector, topK: int, frameIds=None, minScore=None, timeRange=None,  # noqa: N802,N803
                       denyFlags: int = 0, requiredTerms=None) -> Tuple[np.ndarray, np.ndarray]:
        """The vector lane's candidate filters applied on the device (UnifiedSearch.swift:1241-1258): `frameIds` is
        FrameFilter.frameIds (allow-list; None = no list, empty = nothing allowed), `minScore` is SearchRequest.minScore,
        `timeRange` = (after | None, before | None) is SearchRequest.timeRange against the rows' timestamps (after inclusive,
        before exclusive: TimeRange.contains), `denyFlags` drops every row with one of these flag bits set (setAttributes).
        Returns the best topK among the frames that PASS (a pre-filter), best first, minus those scoring below minScore.
        A call without timeRange / denyFlags takes wax_hip_search_filtered, as before those arguments existed.
        `requiredTerms` is FrameFilter.metadataFilter through a TermDictionary (setTerms): only rows whose term set holds every one
        of these ids pass (wax_hip_search_terms). None or an empty list takes the paths above exactly; TermDictionary.NO_MATCH (a
        required string nobody ever interned) returns empty arrays without a call."""
        if requiredTerms is TermDictionary.NO_MATCH:
            return np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.float32)
        req = None if requiredTerms is None else np.ascontiguousarray(list(requiredTerms), dtype=np.uint32).reshape(-1)
        q = _as_f32(vector).reshape(-1)
        cap = self._result_capacity(topK)
        ids = np.empty(cap, dtype=np.uint64)
        scores = np.empty(cap, dtype=np.float32)
        got = ctypes.c_uint32(0)
        allow = None if frameIds is None else np.ascontiguousarray(list(frameIds) if not isinstance(frameIds, np.ndarray)
                                                                   else frameIds, dtype=np.uint64)
        head = (self._h, _fp(q), q.size, int(max(min(topK, 2**31 - 1), -2**31)),
                0 if allow is None else 1, None if allow is None or allow.size == 0 else _u64p(allow),
                0 if allow is None else int(allow.size),
                0 if minScore is None else 1, 0.0 if minScore is None else float(minScore))
        tail = (_u64p(ids), _fp(scores), cap, ctypes.byref(got))
        if req is not None and req.size:
            pred = ticket_predicate(timeRange, denyFlags, who="searchFiltered")
            rc = self._lib.wax_hip_search_terms(*head, ctypes.byref(pred), req.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), int(req.size), *tail)
        elif timeRange is None and not denyFlags:
            rc = self._lib.wax_hip_search_filtered(*head, *tail)
        else:
            after, before = (None, None) if timeRange is None else timeRange
            pred = _abi.RowPredicate(0 if after is None else 1, 0 if after is None else int(after),
                                     0 if before is None else 1, 0 if before is None else int(before), int(denyFlags) & 0xffffffff)
            rc = self._lib.wax_hip_search_predicate(*head, ctypes.byref(pred), *tail)
        raise_for_status(rc)
        return ids[:got.value].copy(), scores[:got.value].copy()

    def setAttributes(self, frameIds, timestamps=None, flags=None) -> int:  # noqa: N802,N803
        """Per-row metadata for the predicate search: FrameMeta.timestamp as int64 `timestamps`, and `flags` (uint32; bit 0
        deleted, bit 1 superseded, bit 2 surrogate, bits 8..31 the caller's). None leaves that column as it is. Ids the engine
        does not hold are skipped; an id listed twice takes its last entry. Returns the entries that named a held frame."""
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64).reshape(-1)
        n = int(ids.size)
        if n == 0:
            return 0
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.int64).reshape(-1)
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32).reshape(-1)
        if (ts is not None and ts.size != n) or (fl is not None and fl.size != n):
            raise EncodingError("setAttributes: one timestamp / flag word per frame id")
        applied = ctypes.c_uint64(0)
        rc = self._lib.wax_hip_set_attributes(
            self._h, _u64p(ids), None if ts is None else ts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            None if fl is None else fl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, ctypes.byref(applied))
        raise_for_status(rc)
        return int(applied.value)

    def getAttributes(self, frameIds) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:  # noqa: N802,N803
        """(timestamps int64, flags uint32, found bool) of the listed frames; (0, 0, False) for an id the engine does not hold."""
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64).reshape(-1)
        n = int(ids.size)
        ts = np.zeros(n, dtype=np.int64)
        fl = np.zeros(n, dtype=np.uint32)
        found = np.zeros(n, dtype=np.uint8)
        if n:
            rc = self._lib.wax_hip_get_attributes(
                self._h, _u64p(ids), n, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                fl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), found.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            raise_for_status(rc)
        return ts, fl, found.astype(bool)

    def setParents(self, frameIds, parentIds) -> int:  # noqa: N802,N803
        """FrameMeta.parentId of the listed frames for searchGrouped (wax_hip_set_parents): `parentIds` uint64, NO_PARENT (UInt64.max)
        = the frame is its own root. Ids the engine does not hold are skipped; an id listed twice takes its last entry. Returns the
        entries that named a held frame."""
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64).reshape(-1)
        par = np.ascontiguousarray(parentIds, dtype=np.uint64).reshape(-1)
        n = int(ids.size)
        if par.size != n:
            raise EncodingError("setParents: one parent id per frame id")
        if n == 0:
            return 0
        applied = ctypes.c_uint64(0)
        raise_for_status(self._lib.wax_hip_set_parents(self._h, _u64p(ids), _u64p(par), n, ctypes.byref(applied)))
        return int(applied.value)

    def getParents(self, frameIds) -> Tuple[np.ndarray, np.ndarray]:  # noqa: N802,N803
        """(parent ids uint64, found bool) of the listed frames; (NO_PARENT, False) for an id the engine does not hold."""
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64).reshape(-1)
        n = int(ids.size)
        par = np.full(n, _abi.NO_PARENT, dtype=np.uint64)
        found = np.zeros(n, dtype=np.uint8)
        if n:
            raise_for_status(self._lib.wax_hip_get_parents(self._h, _u64p(ids), n, _u64p(par),
                                                           found.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return par, found.astype(bool)

    def setTerms(self, frameIds, terms) -> int:  # noqa: N802,N803
        """The term SETS of the listed frames for searchFiltered(requiredTerms=...) (wax_hip_set_terms): `terms` is a sequence of
        iterables of int (uint32 ids of a TermDictionary), one per frame id, or a 2-D array [n, width]; each replaces the frame's whole set, an empty one clears
        it, duplicates collapse, at most TERMS_MAX_PER_ROW distinct terms. Ids the engine does not hold are skipped; an id listed
        twice takes its last entry. Returns the entries that named a held frame."""
        ids = np.ascontiguousarray(frameIds, dtype=np.uint64).reshape(-1)
        n = int(ids.size)
        if isinstance(terms, np.ndarray) and terms.ndim == 2:       # [n, width]: every set of the same size, without a Python loop
            if terms.shape[0] != n:
                raise EncodingError("setTerms: one term set per frame id")
            flat = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1)
            lens = np.full(n, terms.shape[1], dtype=np.uint32)
            begin = np.arange(n, dtype=np.uint64) * np.uint64(terms.shape[1])
        else:
            sets = [np.asarray(list(t) if not isinstance(t, np.ndarray) else t, dtype=np.uint32).reshape(-1) for t in terms]
            if len(sets) != n:
                raise EncodingError("setTerms: one term set per frame id")
            lens = np.array([t.size for t in sets], dtype=np.uint32)
            begin = np.zeros(n, dtype=np.uint64)
            np.cumsum(lens[:-1], out=begin[1:])
            flat = np.ascontiguousarray(np.concatenate(sets) if n else np.empty(0), dtype=np.uint32)
        if n == 0:
            return 0
        applied = ctypes.c_uint64(0)
        u32 = ctypes.POINTER(ctypes.c_uint32)
        raise_for_status(self._lib.wax_hip_set_terms(self._h, _u64p(ids), _u64p(begin), lens.ctypes.data_as(u32),
                                                     flat.ctypes.data_as(u32) if flat.size else None, int(flat.size), n, ctypes.byref(applied)))
        return int(applied.value)

    def getTerms(self, frameId: int):  # noqa: N802,N803
        """The frame's term set, ascending (uint32 array), or None for a frame the engine does not hold."""
        out = np.empty(_abi.TERMS_MAX_PER_ROW, dtype=np.uint32)
        got = ctypes.c_uint32(0)
        found = ctypes.c_uint8(0)
        raise_for_status(self._lib.wax_hip_get_terms(self._h, int(frameId), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), int(out.size),
                                                     ctypes.byref(got), ctypes.byref(found)))
        return out[:got.value].copy() if found.value else None

    def termStats(self) -> dict:  # noqa: N802
        """What the term searches did (wax_hip_term_stats): searches, device_masks, host_staged, host_decided, term_rows_uploaded,
        term_values_uploaded."""
        st = _abi.TermStats()
        raise_for_status(self._lib.wax_hip_term_stats(self._h, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _abi.TermStats._fields_}

    def searchGrouped(self, vector, limit: int, perGroup: int = 1, timeRange=None, denyFlags: int = 0, minScore=None):  # noqa: N802,N803
        """What PhotoRAGOrchestrator.recall / VideoRAGOrchestrator.recall make of the vector lane, exactly and on the device
        (wax_hip_search_grouped): the `limit` best roots (a row's root is its parent, or its own frame id) by their best member,
        ordered by (score descending, root id ascending), and the `perGroup` best rows of each. Only rows that pass `timeRange` /
        `denyFlags` (searchFiltered's meaning) take part; `minScore` drops groups and members below it. Returns (rootIds [g],
        rootScores [g], memberIds [g, perGroup] padded with UInt64.max, memberScores [g, perGroup] padded with 0, memberCounts [g])."""
        q = _as_f32(vector).reshape(-1)
        limit = int(max(min(limit, 2**31 - 1), -2**31))
        per = int(max(min(perGroup, 2**31 - 1), -2**31))
        pred = ticket_predicate(timeRange, denyFlags, who="searchGrouped")
        cap = max(0, min(limit, _abi.GROUP_MAX_LIMIT))
        width = max(1, min(per, _abi.GROUP_MAX_MEMBERS))
        roots = np.empty(cap, dtype=np.uint64)
        scores = np.empty(cap, dtype=np.float32)
        mids = np.empty((cap, width), dtype=np.uint64)
        mscores = np.empty((cap, width), dtype=np.float32)
        mcounts = np.empty(cap, dtype=np.uint32)
        got = ctypes.c_uint32(0)
        rc = self._lib.wax_hip_search_grouped(self._h, _fp(q), q.size, limit, per, 0 if minScore is None else 1,
                                              0.0 if minScore is None else float(minScore), ctypes.byref(pred), _u64p(roots), _fp(scores),
                                              _u64p(mids), _fp(mscores), mcounts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                              ctypes.byref(got))
        raise_for_status(rc)
        g = int(got.value)
        return roots[:g].copy(), scores[:g].copy(), mids[:g].copy(), mscores[:g].copy(), mcounts[:g].copy()

    def groupStats(self) -> dict:  # noqa: N802
        """What the grouped searches did (wax_hip_group_stats): searches, fused_scans, column_scans, member_rounds, group_slots,
        parent_rows_uploaded."""
        st = _abi.GroupStats()
        raise_for_status(self._lib.wax_hip_group_stats(self._h, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _abi.GroupStats._fields_}

    def timeline(self, limit: int, newestFirst: bool = True, timeRange=None, denyFlags: int = 0) -> Tuple[np.ndarray, np.ndarray]:  # noqa: N803
        """Wax.timeline(TimelineQuery) (TimelineQuery.swift:38-53) on the device: the `limit` newest (newestFirst) or oldest frames
        that pass `timeRange` = (after | None, before | None) and `denyFlags` (searchFiltered's meaning), ordered by timestamp and,
        among equal timestamps, by ascending frame id. Returns (frame ids uint64, timestamps int64). limit <= 0 returns nothing;
        limit > TIMELINE_MAX_LIMIT is refused."""
        limit = int(max(min(limit, 2**31 - 1), -2**31))
        pred = ticket_predicate(timeRange, denyFlags, who="timeline")
        cap = max(0, min(limit, TIMELINE_MAX_LIMIT))
        ids = np.empty(cap, dtype=np.uint64)
        ts = np.empty(cap, dtype=np.int64)
        got = ctypes.c_uint32(0)
        rc = self._lib.wax_hip_timeline(self._h, limit, 1 if newestFirst else 0, ctypes.byref(pred), _u64p(ids),
                                        ts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), cap, ctypes.byref(got))
        raise_for_status(rc)
        return ids[:got.value].copy(), ts[:got.value].copy()

    def timelineDevice(self, limit: int, out_ids, out_count, newestFirst: bool = True, timeRange=None, denyFlags: int = 0,  # noqa: N802,N803
                       stream: int = 0) -> None:
        """timeline() left in HBM (wax_hip_timeline_device): `out_ids` a torch uint64 / int64 tensor of at least `limit` elements and
        `out_count` one of at least one 32-bit element, both on this engine's device. Exactly `limit` ids are written, padded
        with UInt64.max, and the real count; the work is enqueued on `stream` (a raw hipStream_t, 0 = the null stream) and not
        synchronised — the ids are a lane for wax_hip_rrf_fuse_batch_device (stride = limit, pitch = 1) on the same stream."""
        limit = int(max(min(limit, 2**31 - 1), -2**31))
        pred = ticket_predicate(timeRange, denyFlags, who="timelineDevice")
        for t, width, need, what in ((out_ids, 8, max(limit, 0), "out_ids"), (out_count, 4, 1, "out_count")):
            if not getattr(t, "is_cuda", False) or not t.is_contiguous() or t.element_size() != width or t.numel() < need:
                raise EncodingError(f"timelineDevice: {what} must be a contiguous device tensor of {need} {width}-byte elements")
        rc = self._lib.wax_hip_timeline_device(self._h, limit, 1 if newestFirst else 0, ctypes.byref(pred),
                                               ctypes.c_void_p(out_ids.data_ptr()), ctypes.c_void_p(out_count.data_ptr()),
                                               ctypes.c_void_p(stream))
        raise_for_status(rc)

    def searchFilteredHits(self, vector, topK: int, allow) -> List[Tuple[int, float]]:  # noqa: N802,N803
        """searchFiltered as [(frameId, score)] (the shape the transcribed reference cases assert on)."""
        ids, scores = self.searchFiltered(vector, topK, frameIds=allow)
        return [(int(i), float(s)) for i, s in zip(ids, scores)]

    def search(self, vector, topK: int) -> List[Tuple[int, float]]:  # noqa: N803
        """VectorSearchEngine.search(vector:topK:) -> [(frameId, score)] best first (:446-627)."""
        ids, scores = self.searchArrays(vector, topK)
        return [(int(i), float(s)) for i, s in zip(ids, scores)]

    def submit(self, vector, topK: int) -> int:  # noqa: N803
        q = _as_f32(vector).reshape(-1)
        t = ctypes.c_uint64(0)
        rc = self._lib.wax_hip_search_submit(self._h, _fp(q), q.size, int(topK), ctypes.byref(t))
        raise_for_status(rc)
        return int(t.value)

    def submitFiltered(self, vector, topK: int, minScore=None, timeRange=None, denyFlags: int = 0) -> int:  # noqa: N802,N803
        """searchFiltered without an allow-list as a ticket (wax_hip_search_predicate_submit): collect(ticket, topK) returns what
        searchFiltered(vector, topK, minScore=..., timeRange=..., denyFlags=...) returns, bit for bit. Several such tickets in flight
        — and unfiltered ones beside them — share passes over the 8-bit code mirror on a store that takes it; every other ticket is
        answered by the blocking search at its collect. The ticket holds the engine's read lock until it is collected."""
        q = _as_f32(vector).reshape(-1)
        pred = ticket_predicate(timeRange, denyFlags)
        t = ctypes.c_uint64(0)
        rc = self._lib.wax_hip_search_predicate_submit(self._h, _fp(q), q.size, int(max(min(topK, 2**31 - 1), -2**31)),
                                                       0 if minScore is None else 1, 0.0 if minScore is None else float(minScore),
                                                       ctypes.byref(pred), ctypes.byref(t))
        raise_for_status(rc)
        return int(t.value)

    def predicateTicketStats(self) -> dict:  # noqa: N802
        """What became of the submitFiltered tickets (wax_hip_predicate_ticket_stats): submitted, rode, masked_passes, certified,
        fallbacks, deferred, host_decided, bitmap_builds, bitmap_hits."""
        st = _abi.PredicateTicketStats()
        raise_for_status(self._lib.wax_hip_predicate_ticket_stats(self._h, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _abi.PredicateTicketStats._fields_}

    def collect(self, ticket: int, topK: int) -> Tuple[np.ndarray, np.ndarray]:  # noqa: N803
        """`topK` sizes the result arrays: pass what was given to submit() (a smaller value truncates to the best)."""
        cap = clampTopK(topK)   # the ticket was answered on the row count at submit time: size by topK alone
        ids = np.empty(cap, dtype=np.uint64)
        scores = np.empty(cap, dtype=np.float32)
        got = ctypes.c_uint32(0)
        rc = self._lib.wax_hip_search_collect(self._h, int(ticket), _u64p(ids), _fp(scores), cap, ctypes.byref(got))
        raise_for_status(rc)
        return ids[:got.value].copy(), scores[:got.value].copy()

    def searchBatch(self, vectors, topK: int):  # noqa: N802,N803
        qs = _as_f32(vectors)
        if qs.ndim != 2:
            raise EncodingError("searchBatch: vectors must be [nq, dims]")
        nq, width = qs.shape
        kcap = max(1, min(clampTopK(topK), max(self.count, 1)))   # row width of the arrays (passed as the stride)
        ids = np.zeros((nq, kcap), dtype=np.uint64)
        scores = np.zeros((nq, kcap), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        rc = self._lib.wax_hip_search_batch(self._h, _fp(qs), nq, width, int(topK), _u64p(ids), _fp(scores), kcap,
                                            counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        raise_for_status(rc)
        return ids, scores, counts

    def searchBatchFiltered(self, vectors, topK: int, frameIds=None, minScore=None, timeRange=None, denyFlags=0):  # noqa: N802,N803
        """searchFiltered for a batch (wax_hip_search_batch_filtered / wax_hip_search_batch_predicate): `frameIds` is None or a
        length-nq sequence whose entries are None (no list) or an iterable of frame ids; `minScore` is None, one float, or a length-nq
        sequence (None entries: no cut). `timeRange` and `denyFlags` are each one value for all queries or a list of nq with None
        entries allowed, by searchManyFiltered's rules: one (after | None, before | None) tuple is one value, a LIST is per query.
        Returns (ids[nq, kcap], scores, counts) like searchBatch; row q equals searchFiltered for that query. A call without
        timeRange / denyFlags takes wax_hip_search_batch_filtered, as before those arguments existed. searchBatchTerms adds a
        required-term filter per query."""
        qs = _as_f32(vectors)
        if qs.ndim != 2:
            raise EncodingError("searchBatchFiltered: vectors must be [nq, dims]")
        nq, width = qs.shape
        kcap = max(1, min(clampTopK(topK), max(self.count, 1)))
        ids = np.zeros((nq, kcap), dtype=np.uint64)
        scores = np.zeros((nq, kcap), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        flat, begin, length = pack_allow_lists(frameIds, nq)
        cuts = None
        if minScore is not None:
            if np.ndim(minScore) == 0:
                cuts = np.full(nq, float(minScore), dtype=np.float32)
            else:
                if len(minScore) != nq:
                    raise EncodingError("searchBatchFiltered: minScore must hold one entry per query")
                cuts = np.array([np.nan if m is None else float(m) for m in minScore], dtype=np.float32)
        ranges = _per_pair(timeRange, nq, "timeRange", tuple_is_value=True, who="searchBatchFiltered", per="query")
        denies = _per_pair(denyFlags, nq, "denyFlags", who="searchBatchFiltered", per="query")
        preds = None
        if any(r is not None for r in ranges) or any(d for d in denies):
            preds = _row_predicates(ranges, denies)
        head = (self._h, _fp(qs), nq, width, int(max(min(topK, 2**31 - 1), -2**31)),
                None if flat.size == 0 else _u64p(flat), int(flat.size),
                None if begin is None else _u64p(begin), None if length is None else _u64p(length),
                None if cuts is None else _fp(cuts))
        tail = (_u64p(ids), _fp(scores), kcap, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        if preds is None:
            rc = self._lib.wax_hip_search_batch_filtered(*head, *tail)
        else:
            rc = self._lib.wax_hip_search_batch_predicate(*head, preds, *tail)
        raise_for_status(rc)
        return ids, scores, counts

    def searchBatchTerms(self, vectors, topK: int, requiredTerms, frameIds=None, minScore=None, timeRange=None, denyFlags=0):  # noqa: N802,N803
        """searchBatchFiltered with searchFiltered's `requiredTerms` PER QUERY (wax_hip_search_batch_terms): None, ONE filter for all
        queries (an iterable of term ids, or TermDictionary.NO_MATCH), or a list / tuple of nq entries, each None, an iterable of ids
        or NO_MATCH. A sequence that holds only ints is one filter. Row q equals searchFiltered(vectors[q], ..., requiredTerms=filter
        q). A NO_MATCH query gets count 0 and its vector is never sent; None or an empty filter is no term filter. With
        requiredTerms=None the call is searchBatchFiltered. The other arguments are searchBatchFiltered's."""
        if requiredTerms is None:
            return self.searchBatchFiltered(vectors, topK, frameIds=frameIds, minScore=minScore, timeRange=timeRange, denyFlags=denyFlags)
        qs = _as_f32(vectors)
        if qs.ndim != 2:
            raise EncodingError("searchBatchTerms: vectors must be [nq, dims]")
        nq, width = qs.shape
        terms = _per_query_terms(requiredTerms, nq)
        kcap = max(1, min(clampTopK(topK), max(self.count, 1)))
        ids = np.zeros((nq, kcap), dtype=np.uint64)
        scores = np.zeros((nq, kcap), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        live = [q for q in range(nq) if terms[q] is not TermDictionary.NO_MATCH]
        if not live:
            return ids, scores, counts
        n = len(live)

        def pick(value, what, tuple_is_value=False):
            per = _per_pair(value, nq, what, tuple_is_value=tuple_is_value, who="searchBatchTerms", per="query")
            return [per[q] for q in live]
        if frameIds is not None and len(frameIds) != nq:
            raise EncodingError("searchBatchTerms: frameIds must hold one entry per query")
        flat, begin, length = pack_allow_lists(None if frameIds is None else [frameIds[q] for q in live], n)
        cuts = None
        if minScore is not None:
            if np.ndim(minScore) == 0:
                cuts = np.full(n, float(minScore), dtype=np.float32)
            else:
                if len(minScore) != nq:
                    raise EncodingError("searchBatchTerms: minScore must hold one entry per query")
                cuts = np.array([np.nan if minScore[q] is None else float(minScore[q]) for q in live], dtype=np.float32)
        ranges = pick(timeRange, "timeRange", tuple_is_value=True)
        denies = pick(denyFlags, "denyFlags")
        preds = None
        if any(r is not None for r in ranges) or any(d for d in denies):
            preds = _row_predicates(ranges, denies)
        sets = [np.empty(0, dtype=np.uint32) if terms[q] is None else terms[q] for q in live]
        tlen = np.array([t.size for t in sets], dtype=np.uint32)
        tbegin = np.zeros(n, dtype=np.uint64)
        np.cumsum(tlen[:-1], out=tbegin[1:])
        tflat = np.ascontiguousarray(np.concatenate(sets), dtype=np.uint32)
        sub = qs if n == nq else np.ascontiguousarray(qs[live])
        s_ids = ids if n == nq else np.zeros((n, kcap), dtype=np.uint64)
        s_scores = scores if n == nq else np.zeros((n, kcap), dtype=np.float32)
        s_counts = counts if n == nq else np.zeros(n, dtype=np.uint32)
        u32 = ctypes.POINTER(ctypes.c_uint32)
        rc = self._lib.wax_hip_search_batch_terms(
            self._h, _fp(sub), n, width, int(max(min(topK, 2**31 - 1), -2**31)),
            None if flat.size == 0 else _u64p(flat), int(flat.size),
            None if begin is None else _u64p(begin), None if length is None else _u64p(length),
            None if cuts is None else _fp(cuts), preds,
            tflat.ctypes.data_as(u32) if tflat.size else None, int(tflat.size), _u64p(tbegin), tlen.ctypes.data_as(u32),
            _u64p(s_ids), _fp(s_scores), kcap, s_counts.ctypes.data_as(u32))
        raise_for_status(rc)
        if n != nq:
            ids[live], scores[live], counts[live] = s_ids, s_scores, s_counts
        return ids, scores, counts

    def termBatchStats(self) -> dict:  # noqa: N802
        """What searchBatchTerms did (wax_hip_term_batch_stats): calls, queries, sets, mask_launches, looped,
        host_decided."""
        st = _abi.TermBatchStats()
        raise_for_status(self._lib.wax_hip_term_batch_stats(self._h, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in _abi.TermBatchStats._fields_}

    def searchBatchHits(self, vectors, topK: int):  # noqa: N802,N803
        """Raw ranked candidates: int64[nq, kcap, 2] of (key, frame_id bits), ascending key, KEY_PAD padded."""
        qs = _as_f32(vectors)
        if qs.ndim != 2:
            raise EncodingError("searchBatchHits: vectors must be [nq, dims]")
        nq, width = qs.shape
        kcap = max(1, min(clampTopK(topK), max(self.count, 1)))
        hits = np.empty((nq, kcap, 2), dtype=np.int64)
        hits[:, :, 0] = _abi.KEY_PAD
        hits[:, :, 1] = -1
        counts = np.zeros(nq, dtype=np.uint32)
        rc = self._lib.wax_hip_search_batch_hits(self._h, _fp(qs), nq, width, int(topK),
                                                 hits.ctypes.data_as(ctypes.POINTER(_abi.Hit)), kcap,
                                                 counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        raise_for_status(rc)
        return hits, counts

    def searchBatchHitsDevice(self, d_queries_ptr: int, nq: int, topK: int, d_out_hits_ptr: int, out_stride: int,  # noqa: N802,N803
                              stream: int = 0) -> None:
        """Device-resident batch search: queries [nq, dims] f32 and the output [nq, out_stride] wax_hip_hit both live
        in this GPU's HBM (raw device pointers, e.g. torch tensors' data_ptr()); blocking; `stream` is the stream that
        produced the queries. Results are complete on return."""
        rc = self._lib.wax_hip_search_batch_hits_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), self.dimensions,
                                                        int(topK), ctypes.c_void_p(d_out_hits_ptr), int(out_stride),
                                                        ctypes.c_void_p(stream))
        raise_for_status(rc)

    def searchBatchSubmitDevice(self, d_queries_ptr: int, nq: int, topK: int, d_out_hits_ptr: int, out_stride: int,  # noqa: N802,N803
                                stream: int = 0) -> int:
        """Pipelined form of searchBatchHitsDevice: enqueues the batch and returns a ticket at once; the buffers must
        stay untouched until searchBatchCollectDevice(ticket)."""
        t = ctypes.c_uint64(0)
        rc = self._lib.wax_hip_search_batch_submit_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), self.dimensions,
                                                          int(topK), ctypes.c_void_p(d_out_hits_ptr), int(out_stride),
                                                          ctypes.c_void_p(stream), ctypes.byref(t))
        raise_for_status(rc)
        return int(t.value)

    def searchBatchCollectDevice(self, ticket: int) -> int:  # noqa: N802
        """Waits for a submitted batch (uncertified queries are re-run exactly, in place); returns how many were."""
        fb = ctypes.c_uint32(0)
        raise_for_status(self._lib.wax_hip_search_batch_collect_device(self._h, int(ticket), ctypes.byref(fb)))
        return int(fb.value)

    # -- sharded search (one engine per GPU; exchange over RCCL by the caller) ----
    def setRowBase(self, rowBase: int) -> None:  # noqa: N802,N803
        raise_for_status(self._lib.wax_hip_set_row_base(self._h, int(rowBase)))

    def searchShardDevice(self, vector, topK: int, out_hits_ptr: int, stream: int = 0) -> None:  # noqa: N802,N803
        q = _as_f32(vector).reshape(-1)
        rc = self._lib.wax_hip_search_shard_device(self._h, _fp(q), q.size, int(topK), ctypes.c_void_p(out_hits_ptr),
                                                   ctypes.c_void_p(stream))
        raise_for_status(rc)

    @staticmethod
    def mergeBatchHitsDevice(in_ptr: int, n_shards: int, nq: int, k_in: int, k: int, out_ptr: int, stream: int = 0) -> None:  # noqa: N802
        """[n_shards][nq][k_in] gathered hits (device) -> [nq][k] merged hits (device), one workgroup per query."""
        rc = _abi.lib().wax_hip_merge_batch_hits_device(ctypes.c_void_p(in_ptr), int(n_shards), int(nq), int(k_in), int(k),
                                                        ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream))
        raise_for_status(rc)

    @staticmethod
    def mergeHitsDevice(in_ptr: int, n: int, k: int, out_ptr: int, stream: int = 0) -> None:  # noqa: N802
        rc = _abi.lib().wax_hip_merge_hits_device(ctypes.c_void_p(in_ptr), int(n), int(k), ctypes.c_void_p(out_ptr),
                                                  ctypes.c_void_p(stream))
        raise_for_status(rc)

    @staticmethod
    def hitsToResults(metric: VectorMetric, hits: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:  # noqa: N802
        """hits: structured/2-column array of (int64 key, uint64 frame_id) pairs, shape [n, 2] viewed as int64."""
        raw = np.ascontiguousarray(hits).view(np.int64).reshape(-1, 2)
        n = raw.shape[0]
        ids = np.empty(max(n, 1), dtype=np.uint64)
        scores = np.empty(max(n, 1), dtype=np.float32)
        got = ctypes.c_uint32(0)
        rc = _abi.lib().wax_hip_hits_to_results(int(metric), raw.ctypes.data_as(ctypes.POINTER(_abi.Hit)), n,
                                                _u64p(ids), _fp(scores), ctypes.byref(got))
        raise_for_status(rc)
        return ids[:got.value].copy(), scores[:got.value].copy()

    # -- persistence --------------------------------------------------------
    def serialize(self) -> bytes:
        """serialize() (:682-714): "MV2V" segment, encoding 2."""
        out = ctypes.POINTER(ctypes.c_uint8)()
        length = ctypes.c_size_t(0)
        rc = self._lib.wax_hip_serialize(self._h, ctypes.byref(out), ctypes.byref(length))
        raise_for_status(rc)
        try:
            return ctypes.string_at(out, length.value)
        finally:
            self._lib.wax_hip_free(out)

    def deserialize(self, data: bytes) -> None:
        """deserialize(_:) (:716-815)."""
        data = bytes(data)
        rc = self._lib.wax_hip_deserialize(self._h, data, len(data))
        raise_for_status(rc)
        self._dirty = False  # :813

    def stageForCommit(self, into) -> None:  # noqa: N802 — stageForCommit(into:) (:818-828)
        if not self._dirty:
            return
        blob = self.serialize()
        into.stageVecIndexForNextCommit(bytes=blob, vectorCount=self.count, dimension=self.dimensions,
                                        similarity=self.metric.toVecSimilarity())
        self._dirty = False

    # -- observability ------------------------------------------------------
    def stats(self) -> _abi.Stats:
        st = _abi.Stats()
        raise_for_status(self._lib.wax_hip_stats(self._h, ctypes.byref(st)))
        return st

    def debugBufferPoolStats(self) -> BufferPoolStats:  # noqa: N802 — (:119-121)
        st = self.stats()
        return BufferPoolStats(int(st.transient_allocations), int(st.reuse_count))

    def setTuning(self, key: str, value: int) -> None:  # noqa: N802
        raise_for_status(self._lib.wax_hip_set_tuning(self._h, key.encode(), int(value)))

    def getTuning(self, key: str) -> int:  # noqa: N802
        return int(self._lib.wax_hip_get_tuning(self._h, key.encode()))

    def timeScanKernel(self, vector, topK: int, iters: int) -> float:  # noqa: N802,N803
        q = _as_f32(vector).reshape(-1)
        ms = ctypes.c_double(0.0)
        raise_for_status(self._lib.wax_hip_time_scan_kernel(self._h, _fp(q), q.size, int(topK), int(iters),
                                                            ctypes.byref(ms)))
        return float(ms.value)

    def timeStreamRead(self, iters: int) -> float:  # noqa: N802
        ms = ctypes.c_double(0.0)
        raise_for_status(self._lib.wax_hip_time_stream_read(self._h, int(iters), ctypes.byref(ms)))
        return float(ms.value)

    def mirror8Snapshot(self, first: int = 0, n=None):  # noqa: N802
        """What the device holds of the 8-bit code mirror for rows [first, first + n) (n None: up to the last coded row), for tests
        (wax_hip_mirror8_snapshot): (codes uint8 [n, dims], scale f32 [n], err f32 [n], max_norm, rows_coded). Raises unless the code
        mirror is valid; it is never built or refreshed here."""
        max_norm, rows = ctypes.c_float(0.0), ctypes.c_uint64(0)
        if n is None:
            raise_for_status(self._lib.wax_hip_mirror8_snapshot(self._h, 0, 0, None, None, ctypes.byref(max_norm), ctypes.byref(rows)))
            n = max(int(rows.value) - int(first), 0)
        codes = np.zeros((int(n), self.dimensions), dtype=np.uint8)
        meta = np.zeros((int(n), 2), dtype=np.float32)
        raise_for_status(self._lib.wax_hip_mirror8_snapshot(self._h, int(first), int(n), codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                            _fp(meta), ctypes.byref(max_norm), ctypes.byref(rows)))
        return codes, meta[:, 0].copy(), meta[:, 1].copy(), float(max_norm.value), int(rows.value)

    def mirror8Keys(self, query):  # noqa: N802
        """The f32 key (a lower bound of the distance) that the lone 8-bit scan computes for `query` at every coded row, for tests
        (wax_hip_mirror8_keys): f32 [rows_coded]. Raises unless the code mirror is valid; it is never built or refreshed here."""
        q = _as_f32(query)
        if q.shape != (self.dimensions,):
            raise EncodingError("mirror8Keys: query must be [dims]")
        rows = self.mirror8Snapshot(0, 0)[4]
        keys = np.zeros(rows, dtype=np.float32)
        raise_for_status(self._lib.wax_hip_mirror8_keys(self._h, _fp(q), _fp(keys), rows))
        return keys


def searchMany(engines, queries, topK: int):  # noqa: N802,N803
    """One query each against many stores of one device in one pass (wax_hip_search_many): pair i is (engines[i], queries[i]).
    Returns (ids, scores, counts) shaped like searchBatch's; row i is what engines[i].search(queries[i], topK) returns. An engine
    may be listed any number of times. Whatever the C call refuses (a sharded engine, mixed metrics or dimensions) is raised."""
    engines = list(engines)
    qs = _as_f32(queries)
    if qs.ndim != 2 or qs.shape[0] != len(engines):
        raise EncodingError("searchMany: queries must be [len(engines), dims]")
    n, width = qs.shape
    if any(not isinstance(e, HIPVectorEngine) for e in engines):
        raise TypeError("searchMany: engines must be HIPVectorEngine instances")
    kcap = max(1, min(clampTopK(topK), max([e.count for e in engines] + [1])))   # row width of the arrays (passed as the stride)
    ids = np.zeros((n, kcap), dtype=np.uint64)
    scores = np.zeros((n, kcap), dtype=np.float32)
    counts = np.zeros(n, dtype=np.uint32)
    if n == 0:
        return ids, scores, counts
    handles = (ctypes.c_void_p * n)(*[e._h.value for e in engines])
    rc = engines[0]._lib.wax_hip_search_many(handles, _fp(qs), n, width, int(max(min(topK, 2**31 - 1), -2**31)), _u64p(ids), _fp(scores),
                                             kcap, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    raise_for_status(rc)
    return ids, scores, counts


def timelineProbe(timestamps, flags, frameIds, limit: int, newestFirst: bool = True, timeRange=None, denyFlags: int = 0,  # noqa: N802,N803
                  grid: int = 0):
    """wax_hip_timeline_probe: the timeline's two kernels on host columns (`timestamps` / `flags` None = zeros), the selection run
    with `grid` workgroups (0 = the product's choice). Returns (ids[limit] padded with UInt64.max, timestamps[limit], count)."""
    ids = np.ascontiguousarray(frameIds, dtype=np.uint64).reshape(-1)
    n = int(ids.size)
    ts = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.int64).reshape(-1)
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32).reshape(-1)
    if (ts is not None and ts.size != n) or (fl is not None and fl.size != n):
        raise EncodingError("timelineProbe: one timestamp / flag word per frame id")
    limit = int(limit)
    pred = ticket_predicate(timeRange, denyFlags, who="timelineProbe")
    cap = max(0, min(limit, TIMELINE_MAX_LIMIT))
    out_ids = np.zeros(cap, dtype=np.uint64)
    out_ts = np.zeros(cap, dtype=np.int64)
    got = ctypes.c_uint32(0)
    i64p = ctypes.POINTER(ctypes.c_int64)
    rc = _abi.lib().wax_hip_timeline_probe(None if ts is None else ts.ctypes.data_as(i64p),
                                           None if fl is None else fl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                           _u64p(ids), n, limit, 1 if newestFirst else 0, ctypes.byref(pred), int(grid),
                                           _u64p(out_ids), out_ts.ctypes.data_as(i64p), ctypes.byref(got))
    raise_for_status(rc)
    return out_ids, out_ts, int(got.value)


def groupProbe(distances, slots, slotRoot, limit: int, perGroup: int = 1, bitmap=None, nSlots=None, grid: int = 0):  # noqa: N802,N803
    """wax_hip_group_probe: the grouped search's offers, selection, marking and member rounds on host columns. `distances` float32
    per row (taken bit for bit), `slots` uint32 per row (None = every row its own slot), `slotRoot` uint64 per slot (None = the slot's
    number), `bitmap` uint32 words (None = every row takes part). Returns (rootIds[limit] padded with UInt64.max, rootKeys[limit]
    padded with Int64.max, memberKeys[limit, perGroup] likewise, count)."""
    dist = np.ascontiguousarray(distances, dtype=np.float32).reshape(-1)
    n = int(dist.size)
    sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.uint32).reshape(-1)
    sr = None if slotRoot is None else np.ascontiguousarray(slotRoot, dtype=np.uint64).reshape(-1)
    bm = None if bitmap is None else np.ascontiguousarray(bitmap, dtype=np.uint32).reshape(-1)
    if sl is not None and sl.size != n:
        raise EncodingError("groupProbe: one slot per row")
    if bm is not None and bm.size != (n + 31) // 32:
        raise EncodingError("groupProbe: the bitmap holds one bit per row")
    n_slots = int(nSlots) if nSlots is not None else (int(sr.size) if sr is not None else (n if sl is None else int(sl.max()) + 1 if n else 0))
    if sr is not None and sr.size != n_slots:
        raise EncodingError("groupProbe: one root id per slot")
    limit, per = int(limit), int(perGroup)
    cap = max(0, min(limit, _abi.GROUP_MAX_LIMIT))
    width = max(1, min(per, _abi.GROUP_MAX_MEMBERS))
    roots = np.zeros(cap, dtype=np.uint64)
    rkeys = np.zeros(cap, dtype=np.int64)
    mkeys = np.zeros((cap, width), dtype=np.int64)
    got = ctypes.c_uint32(0)
    i64p, u32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint32)
    rc = _abi.lib().wax_hip_group_probe(_fp(dist), None if sl is None else sl.ctypes.data_as(u32p), None if sr is None else _u64p(sr),
                                        None if bm is None else bm.ctypes.data_as(u32p), n, n_slots, limit, per, int(grid),
                                        _u64p(roots), rkeys.ctypes.data_as(i64p), mkeys.ctypes.data_as(i64p), ctypes.byref(got))
    raise_for_status(rc)
    return roots, rkeys, mkeys, int(got.value)


def termMaskProbe(offsets, values, required, bitmapIn=None, grid: int = 1) -> np.ndarray:  # noqa: N802,N803
    """wax_hip_term_mask_probe: term_mask_kernel on a made-up CSR column — offsets [rows + 1], values [offsets[-1]], `required` 1 .. 16
    terms, `bitmapIn` (uint32 words, None = none) ANDed in, exactly `grid` workgroups. Returns the row bitmap (uint32 words)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    val = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
    req = np.ascontiguousarray(required, dtype=np.uint32).reshape(-1)
    rows = int(off.size) - 1
    if rows < 0 or (rows >= 0 and val.size != int(off[-1])):
        raise EncodingError("termMaskProbe: offsets of rows + 1 entries, values of offsets[-1] entries")
    words = (max(rows, 0) + 31) // 32
    bm = None if bitmapIn is None else np.ascontiguousarray(bitmapIn, dtype=np.uint32).reshape(-1)
    if bm is not None and bm.size != words:
        raise EncodingError("termMaskProbe: one bitmap word per 32 rows")
    out = np.zeros(words, dtype=np.uint32)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    raise_for_status(_abi.lib().wax_hip_term_mask_probe(off.ctypes.data_as(u32), val.ctypes.data_as(u32) if val.size else None, rows,
                                                        req.ctypes.data_as(u32) if req.size else None, int(req.size),
                                                        None if bm is None else bm.ctypes.data_as(u32), int(grid), out.ctypes.data_as(u32)))
    return out


def termMaskMultiProbe(offsets, values, sets, grid: int = 1):  # noqa: N802,N803
    """wax_hip_term_mask_multi_probe: term_mask_multi_kernel on a made-up CSR column — offsets [rows + 1], values [offsets[-1]] (distinct
    within a row), `sets` 1 .. 32 iterables of 1 .. 16 term ids, exactly `grid` workgroups. Returns (bitmaps uint32 [len(sets), words],
    counts uint32 [len(sets)])."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
    val = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
    reqs = [np.asarray(list(t) if not isinstance(t, np.ndarray) else t, dtype=np.uint32).reshape(-1) for t in sets]
    rows = int(off.size) - 1
    if rows < 0 or val.size != int(off[-1]):
        raise EncodingError("termMaskMultiProbe: offsets of rows + 1 entries, values of offsets[-1] entries")
    n = len(reqs)
    lens = np.array([t.size for t in reqs], dtype=np.uint32)
    begin = np.zeros(max(n, 1), dtype=np.uint64)
    if n:
        np.cumsum(lens[:-1], out=begin[1:n])
    flat = np.ascontiguousarray(np.concatenate(reqs) if n else np.empty(0), dtype=np.uint32)
    words = (max(rows, 0) + 31) // 32
    bitmaps = np.zeros((n, words), dtype=np.uint32)
    counts = np.zeros(max(n, 1), dtype=np.uint32)
    u32 = ctypes.POINTER(ctypes.c_uint32)
    raise_for_status(_abi.lib().wax_hip_term_mask_multi_probe(
        off.ctypes.data_as(u32), val.ctypes.data_as(u32) if val.size else None, rows, flat.ctypes.data_as(u32) if flat.size else None,
        _u64p(begin), lens.ctypes.data_as(u32) if n else None, n, int(grid), bitmaps.ctypes.data_as(u32) if bitmaps.size else None,
        counts.ctypes.data_as(u32)))
    return bitmaps, counts[:n]


def _per_query_terms(requiredTerms, nq: int) -> list:  # noqa: N803
    """searchBatchTerms' requiredTerms -> nq entries, each None (no term filter), a uint32 array or TermDictionary.NO_MATCH."""
    def one(t):
        if t is None or t is TermDictionary.NO_MATCH:
            return t
        a = np.ascontiguousarray(list(t) if not isinstance(t, np.ndarray) else t, dtype=np.uint32).reshape(-1)
        return a if a.size else None
    if requiredTerms is TermDictionary.NO_MATCH:
        return [requiredTerms] * nq
    if isinstance(requiredTerms, np.ndarray) and requiredTerms.ndim == 1:
        return [one(requiredTerms)] * nq
    seq = list(requiredTerms)
    if all(isinstance(t, (int, np.integer)) for t in seq):          # ids only (or nothing): one filter for all queries
        return [one(seq)] * nq
    if len(seq) != nq:
        raise EncodingError("searchBatchTerms: requiredTerms must be one filter or hold one entry per query")
    return [one(t) for t in seq]


class _NoMatch:
    """TermDictionary.NO_MATCH: a filter that names a string no frame was ever given."""
    def __repr__(self):
        return "TermDictionary.NO_MATCH"


class TermDictionary:
    """The caller's side of the term column: interns ("entry", key, value), ("tag", key, value) and ("label", s) to uint32 ids, so
    that FrameFilter.metadataFilter (SearchRequest.swift:130-145) becomes a list of required ids and a frame's
    FrameMeta.metadata.entries / tags / labels become its term set — exactly (no hashing, no collisions). The engine never sees
    a string."""
    NO_MATCH = _NoMatch()

    def __init__(self):
        self._ids = {}
        self._keys = []

    def __len__(self):
        return len(self._keys)

    def _intern(self, key) -> int:
        i = self._ids.get(key)
        if i is None:
            if len(self._keys) >= 0xffffffff:
                raise EncodingError("TermDictionary: more than 2^32 - 1 terms")
            i = len(self._keys)
            self._ids[key] = i
            self._keys.append(key)
        return i

    def entry(self, key: str, value: str) -> int:
        return self._intern(("entry", str(key), str(value)))

    def tag(self, key: str, value: str) -> int:
        return self._intern(("tag", str(key), str(value)))

    def label(self, s: str) -> int:
        return self._intern(("label", str(s)))

    def lookup(self, termId: int):  # noqa: N803
        """The ("entry" | "tag", key, value) or ("label", s) tuple behind an id."""
        return self._keys[int(termId)]

    def forFrame(self, entries=None, tags=None, labels=None) -> List[int]:  # noqa: N802
        """A frame's term set (interning what is new): `entries` a mapping, `tags` an iterable of (key, value), `labels` of strings."""
        out = {self.entry(k, v) for k, v in dict(entries or {}).items()}
        out |= {self.tag(k, v) for k, v in (tags or ())}
        out |= {self.label(s) for s in (labels or ())}
        return sorted(out)

    def forFilter(self, requiredEntries=None, requiredTags=None, requiredLabels=None):  # noqa: N802,N803
        """MetadataFilter -> the ids searchFiltered(requiredTerms=...) takes; NO_MATCH when a required string was never interned (no
        frame can hold it). Nothing is interned. An empty filter gives []."""
        keys = [("entry", str(k), str(v)) for k, v in dict(requiredEntries or {}).items()]
        keys += [("tag", str(k), str(v)) for k, v in (requiredTags or ())]
        keys += [("label", str(s)) for s in (requiredLabels or ())]
        out = set()
        for key in keys:
            i = self._ids.get(key)
            if i is None:
                return TermDictionary.NO_MATCH
            out.add(i)
        return sorted(out)


def ticket_predicate(timeRange=None, denyFlags=0, who: str = "submitFiltered") -> "_abi.RowPredicate":  # noqa: N803
    """submitFiltered's (and the timeline's) row predicate: `timeRange` None or (after | None, before | None), `denyFlags` a mask of 32 bits."""
    if timeRange is not None and (not isinstance(timeRange, (tuple, list)) or len(timeRange) != 2):
        raise EncodingError(f"{who}: timeRange must be None or (after | None, before | None)")
    after, before = (None, None) if timeRange is None else timeRange
    for bound in (after, before):
        if bound is not None and not (isinstance(bound, (int, np.integer)) and -2**63 <= int(bound) < 2**63):
            raise EncodingError(f"{who}: a timeRange bound must be an int64 or None")
    if not isinstance(denyFlags, (int, np.integer)) or not 0 <= int(denyFlags) <= 0xffffffff:
        raise EncodingError(f"{who}: denyFlags must be a mask of 32 bits")
    return _abi.RowPredicate(0 if after is None else 1, 0 if after is None else int(after),
                             0 if before is None else 1, 0 if before is None else int(before), int(denyFlags))


def _per_pair(value, n: int, what: str, tuple_is_value: bool = False, who: str = "searchManyFiltered", per: str = "pair") -> list:
    """One filter value for all n pairs (queries), or a sequence of n (None entries: none for that one) -> a list of n."""
    if isinstance(value, (list, np.ndarray)) or (isinstance(value, tuple) and not tuple_is_value):
        if len(value) != n:
            raise EncodingError(f"{who}: {what} must be one value or hold one entry per {per}")
        return list(value)
    return [value] * n


def _row_predicates(ranges: list, denies: list):
    """n (after | None, before | None) tuples (or None) and n deny masks (or None) -> wax_hip_row_predicate[n]."""
    n = len(ranges)
    preds = (_abi.RowPredicate * n)()
    for i in range(n):
        after, before = (None, None) if ranges[i] is None else ranges[i]
        preds[i] = _abi.RowPredicate(0 if after is None else 1, 0 if after is None else int(after),
                                     0 if before is None else 1, 0 if before is None else int(before),
                                     int(denies[i] or 0) & 0xffffffff)
    return preds


def searchManyFiltered(engines, queries, topK: int, timeRange=None, denyFlags=0, minScore=None):  # noqa: N802,N803
    """searchMany with the row predicate and score cut of searchFiltered per pair (wax_hip_search_many_predicate): row i is what
    engines[i].searchFiltered(queries[i], topK, timeRange=..., denyFlags=..., minScore=...) returns. Each filter is one value for all
    pairs or a list of n with None entries allowed: `timeRange` = (after | None, before | None) (one such tuple is one value; a
    LIST is per pair), `denyFlags` an int, `minScore` a float. Allow-lists per pair are not part of this call. Returns
    (ids, scores, counts) like searchMany."""
    engines = list(engines)
    qs = _as_f32(queries)
    if qs.ndim != 2 or qs.shape[0] != len(engines):
        raise EncodingError("searchManyFiltered: queries must be [len(engines), dims]")
    n, width = qs.shape
    if any(not isinstance(e, HIPVectorEngine) for e in engines):
        raise TypeError("searchManyFiltered: engines must be HIPVectorEngine instances")
    kcap = max(1, min(clampTopK(topK), max([e.count for e in engines] + [1])))   # row width of the arrays (passed as the stride)
    ids = np.zeros((n, kcap), dtype=np.uint64)
    scores = np.zeros((n, kcap), dtype=np.float32)
    counts = np.zeros(n, dtype=np.uint32)
    if n == 0:
        return ids, scores, counts
    ranges, denies, cuts_in = _per_pair(timeRange, n, "timeRange", tuple_is_value=True), _per_pair(denyFlags, n, "denyFlags"), _per_pair(minScore, n, "minScore")
    preds = None
    if any(r is not None for r in ranges) or any(d for d in denies):
        preds = _row_predicates(ranges, denies)
    cuts = None
    if any(c is not None for c in cuts_in):
        cuts = np.array([np.nan if c is None else float(c) for c in cuts_in], dtype=np.float32)
    handles = (ctypes.c_void_p * n)(*[e._h.value for e in engines])
    rc = engines[0]._lib.wax_hip_search_many_predicate(
        handles, _fp(qs), n, width, int(max(min(topK, 2**31 - 1), -2**31)), preds, None if cuts is None else _fp(cuts),
        _u64p(ids), _fp(scores), kcap, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    raise_for_status(rc)
    return ids, scores, counts
