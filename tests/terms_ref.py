"""A numpy restatement of the required-term search's contract (include/wax_hip.h, wax_hip_search_terms):
the pass set — rows whose term set holds every required term — then the exact top-k of the passing rows; the bitmap
term_mask_kernel writes; FrameFilter.metadataFilter restated from matches(metadataFilter:meta:) (UnifiedSearch.swift:1215-1239); and
a model of a store with its term sets under add / upsert / remove / removeBatch / setTerms / deserialize."""
import numpy as np

MAX_PER_ROW = 64        # WAX_HIP_TERMS_MAX_PER_ROW
MAX_REQUIRED = 16       # WAX_HIP_TERMS_MAX_REQUIRED
PIECE = 1024            # TERM_MASK_PIECE (wax_amd/csrc/kernels.h): values of a wave's span the wave-cooperative form consumes per loop iteration
CANDIDATE_LIMIT = 30    # the reference's over-fetch for topK 10 (candidateLimit, UnifiedSearch.swift:1195)


def pass_set(sets, required):
    """sets: one iterable of terms per row. True where the row's set contains every required term."""
    req = set(int(t) for t in required)
    return np.array([req <= set(int(t) for t in s) for s in sets], dtype=bool)


def csr_of(sets):
    """(offsets uint32 [rows + 1], values uint32) with each row's distinct terms ascending."""
    rows = [np.unique(np.asarray(list(s), dtype=np.uint32)) for s in sets]
    off = np.zeros(len(rows) + 1, dtype=np.uint32)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows])
    val = np.concatenate(rows).astype(np.uint32) if rows and off[-1] else np.empty(0, dtype=np.uint32)
    return off, val


def bitmap_of(passing):
    """bool per row -> uint32 words, bit r % 32 of word r // 32; the bits behind the last row clear."""
    passing = np.asarray(passing, dtype=bool)
    words = (len(passing) + 31) // 32
    padded = np.zeros(words * 32, dtype=bool)
    padded[:len(passing)] = passing
    return (padded.reshape(words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def bits_of(bitmap, n):
    words = np.asarray(bitmap, dtype=np.uint32)
    return ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)[:n]


def mask_model(sets, required, bitmap_in=None):
    """What term_mask_kernel writes for these rows."""
    p = pass_set(sets, required)
    if bitmap_in is not None:
        p &= bits_of(bitmap_in, len(p))
    return bitmap_of(p)


def topk_rows(scores, passing, k):
    """The k best passing rows by (score descending, row ascending): the tie rule of every search route."""
    rows = np.nonzero(np.asarray(passing, dtype=bool))[0]
    order = np.lexsort((rows, -np.asarray(scores, dtype=np.float64)[rows]))
    return rows[order[:k]]


def post_filter_rows(scores, passing, k, prefix=CANDIDATE_LIMIT):
    """What the reference returns: the filter applied to the `prefix` best rows of the UNFILTERED ranking, then the cut at k."""
    best = topk_rows(scores, np.ones(len(scores), dtype=bool), prefix)
    return best[np.asarray(passing, dtype=bool)[best]][:k]


# ---- matches(metadataFilter:meta:), UnifiedSearch.swift:1215-1239 -------------------------------------------------------------

def matches_metadata_filter(required_entries, required_tags, required_labels, entries, tags, labels):
    """entries: dict or None (meta.metadata?.entries); tags: list of (key, value); labels: list of str."""
    if required_entries:
        if entries is None:
            return False
        for key, value in required_entries.items():
            if entries.get(key) != value:
                return False
    for rk, rv in required_tags or ():
        if not any(k == rk and v == rv for k, v in tags):
            return False
    for label in required_labels or ():
        if label not in labels:
            return False
    return True


# ---- a store and its term sets -----------------------------------------------------------------------------------------------

class StoreModel:
    """Rows in store order: frame ids, vectors and term sets, under the mutations of the engine."""
    def __init__(self, dims):
        self.dims = dims
        self.ids = []
        self.rows = []
        self.sets = []

    def add(self, fid, row):
        fid = int(fid)
        if fid in self.ids:                                    # an upsert keeps its row — and the row's set
            self.rows[self.ids.index(fid)] = np.asarray(row, dtype=np.float32)
            return
        self.ids.append(fid)
        self.rows.append(np.asarray(row, dtype=np.float32))
        self.sets.append(())                                   # an appended row holds the empty set

    def add_batch(self, fids, rows):
        for f, r in zip(fids, rows):
            self.add(f, r)

    def remove(self, fid):
        if int(fid) in self.ids:
            i = self.ids.index(int(fid))
            del self.ids[i], self.rows[i], self.sets[i]

    def remove_batch(self, fids):
        for f in set(int(f) for f in fids):
            self.remove(f)

    def set_terms(self, fids, sets):
        for f, s in zip(fids, sets):
            if int(f) in self.ids:
                self.sets[self.ids.index(int(f))] = tuple(sorted(set(int(t) for t in s)))

    def drop_terms(self):                                      # deserialize
        self.sets = [() for _ in self.ids]

    def passing_ids(self, required):
        p = pass_set(self.sets, required)
        return np.asarray(self.ids, dtype=np.uint64)[p]

    def matrix(self):
        return np.stack(self.rows).astype(np.float32) if self.rows else np.empty((0, self.dims), dtype=np.float32)


# ---- made-up columns for the kernel's probe -----------------------------------------------------------------------------------

SPECIALS = np.arange(1, 17, dtype=np.uint32)   # sixteen terms no body holds; a row holds the first c of them (c = 0 .. 16)
COMMON = 99                                    # the term every row of a shape with `common` holds
NOBODY = 50                                    # no row holds it


def build_column(lens, special_count, common):
    """CSR of rows of lens[r] terms, ascending and distinct by construction: SPECIALS[:special_count[r]], then COMMON where
    common[r], then body terms 100 + 1000 j + jitter. A row too short for its specials and COMMON grows to hold them."""
    lens = np.asarray(lens, dtype=np.int64)
    c = np.asarray(special_count, dtype=np.int64)
    hc = np.asarray(common, dtype=np.int64)
    lens = np.maximum(lens, c + hc)
    assert lens.max(initial=0) <= MAX_PER_ROW
    off = np.zeros(len(lens) + 1, dtype=np.uint32)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    row = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(total) - off[:-1].astype(np.int64)[row]
    jitter = (row * 7919 + pos * 104729) % 1000
    body = 100 + (pos - c[row] - hc[row]) * 1000 + jitter
    val = np.where(pos < c[row], pos + 1, np.where((pos == c[row]) & (hc[row] == 1), COMMON, body)).astype(np.uint32)
    return off, val


def pass_csr(off, val, required):
    """The pass set straight from a CSR column (vectorised; pass_set's answer)."""
    n = len(off) - 1
    row = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    p = np.ones(n, dtype=bool)
    for t in set(int(t) for t in required):
        has = np.zeros(n, dtype=bool)
        has[row[val == t]] = True
        p &= has
    return p


def sets_of(off, val):
    return [tuple(int(t) for t in val[off[r]:off[r + 1]]) for r in range(len(off) - 1)]
