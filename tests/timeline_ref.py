"""The timeline lane's model and its shared case table (tests/test_timeline_cpu.py, tests/test_timeline_gpu.py).

The model restates TimelineQuery.filter (TimelineQuery.swift:38-53): filter the frames, stable-sort them on the timestamp alone,
take the prefix. `toc.frames` is indexed by frame id, so the frames enter the sort in ascending (unsigned) frame-id order and a stable
sort leaves equal timestamps in that order — for BOTH directions. `tie="row"` enters them in row order instead: what a selection that
broke ties by row would return, kept so that the CPU tests can show every tie case tells the two apart.
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np

FLAG_DELETED, FLAG_SUPERSEDED, FLAG_SURROGATE = 0x1, 0x2, 0x4
ID_PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
I64_MIN, I64_MAX = -2**63, 2**63 - 1
MAX_LIMIT = 4096


def passes(ts: int, fl: int, after: Optional[int], before: Optional[int], deny: int) -> bool:
    """TimelineQuery.contains plus the flag exclusions (wax_hip_row_predicate's rule: after inclusive, before exclusive)."""
    if after is not None and ts < after:
        return False
    if before is not None and ts >= before:
        return False
    return (fl & deny) == 0


def timeline_model(ts, flags, ids, limit: int, newest_first: bool, after=None, before=None, deny: int = 0, tie: str = "frame"):
    """(frame ids uint64, timestamps int64) of the answer. ts / flags None = zeros. Python integers throughout: no overflow anywhere."""
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1).tolist()
    n = len(ids)
    ts = [0] * n if ts is None else np.asarray(ts, dtype=np.int64).reshape(-1).tolist()
    fl = [0] * n if flags is None else np.asarray(flags, dtype=np.uint32).reshape(-1).tolist()
    assert len(set(ids)) == n, "frame ids are unique in a store"
    frames = list(range(n))
    if tie == "frame":
        frames.sort(key=lambda r: ids[r])                       # toc.frames: indexed by frame id
    else:
        assert tie == "row"
    kept = [r for r in frames if passes(ts[r], fl[r], after, before, deny)]
    kept = sorted(kept, key=lambda r: ts[r], reverse=bool(newest_first))   # stable in both directions, like Swift's sorted(by:)
    kept = kept[:limit] if limit > 0 else []
    return (np.array([ids[r] for r in kept], dtype=np.uint64), np.array([ts[r] for r in kept], dtype=np.int64))


def padded(ids: np.ndarray, limit: int) -> np.ndarray:
    """The device form's / the probe's id array: `limit` entries, UInt64.max behind the answer."""
    out = np.full(max(limit, 0), ID_PAD, dtype=np.uint64)
    out[:len(ids)] = ids
    return out


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    ts_kind: str            # asc | desc | equal | few | extremes | blocks | none
    id_kind: str            # row | shuffled | high
    flag_kind: str          # none | mod3 | all_deleted
    limit: int
    newest: bool
    after: Optional[int]
    before: Optional[int]
    deny: int
    count: int              # what the case CLAIMS the answer's length is (a closed form of its parameters, not a run of the model)
    tags: Tuple[str, ...] = ()

    @property
    def seed(self) -> int:
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) & 0x7fffffff


BLOCK = 7                   # ts_kind "blocks": timestamp = row // 7, so every timestamp is held by several rows


@lru_cache(maxsize=None)
def columns(case: Case):
    """(timestamps int64 | None, flags uint32 | None, frame ids uint64), seeded by the case's name; never modified."""
    rng = np.random.default_rng(case.seed)
    n, rows = case.n, np.arange(case.n, dtype=np.int64)
    ts = {"asc": lambda: 1000 + 3 * rows, "desc": lambda: 10**9 - 3 * rows, "equal": lambda: np.full(n, 77, dtype=np.int64),
          "few": lambda: rng.integers(-3, 4, size=n).astype(np.int64),
          "extremes": lambda: np.array([I64_MIN, -1, 0, I64_MAX], dtype=np.int64)[rng.integers(0, 4, size=n)],
          "blocks": lambda: rows // BLOCK, "none": lambda: None}[case.ts_kind]()
    ids = {"row": lambda: (rows + 100).astype(np.uint64),
           "shuffled": lambda: (rng.permutation(n) + 1).astype(np.uint64),
           # around 2^63: half of them have the top bit set, so a signed comparison would order them wrongly
           "high": lambda: (np.uint64(2**63 - n // 2) + rng.permutation(n).astype(np.uint64))}[case.id_kind]()
    fl = {"none": lambda: None,
          "mod3": lambda: np.array([FLAG_DELETED, FLAG_SUPERSEDED | 0x100, 0x200], dtype=np.uint32)[rows % 3],
          "all_deleted": lambda: np.full(n, FLAG_DELETED, dtype=np.uint32)}[case.flag_kind]()
    for a in (ts, ids, fl):
        if a is not None:
            a.setflags(write=False)
    return ts, fl, ids


@lru_cache(maxsize=None)
def expected(case: Case, tie: str = "frame"):
    ts, fl, ids = columns(case)
    return timeline_model(ts, fl, ids, case.limit, case.newest, case.after, case.before, case.deny, tie=tie)


SIZES = (257, 4096 + 1, 20000)
LIMITS = (1, 255, 256, 257, 1024, 1025, 4096)
WINDOW = (5, 25)            # after (inclusive), before (exclusive) of the boundary cases, in "blocks" timestamps
WINDOW_ROWS = BLOCK * (WINDOW[1] - WINDOW[0])   # 140 rows pass it (every size holds rows beyond block 25)


def _cases():
    out = []
    for n in SIZES:
        for newest in (False, True):
            o = "new" if newest else "old"
            out.append(Case(f"asc_{o}_{n}", n, "asc", "row", "none", 300, newest, None, None, 0, min(300, n)))
            out.append(Case(f"desc_{o}_{n}", n, "desc", "row", "none", 300, newest, None, None, 0, min(300, n)))
            out.append(Case(f"equal_shuffled_{o}_{n}", n, "equal", "shuffled", "none", 300, newest, None, None, 0, min(300, n), ("tie",)))
            out.append(Case(f"noattr_high_ids_{o}_{n}", n, "none", "high", "none", 300, newest, None, None, 0, min(300, n), ("tie",)))
            out.append(Case(f"extremes_{o}_{n}", n, "extremes", "shuffled", "none", min(n, MAX_LIMIT), newest, None, None, 0, min(n, MAX_LIMIT), ("tie",)))
            # the window, with room behind it (the limit does not cut) and cut one short of / exactly at / one above what passes
            out.append(Case(f"window_{o}_{n}", n, "blocks", "shuffled", "none", 256, newest, WINDOW[0], WINDOW[1], 0, WINDOW_ROWS, ("tie", "boundary")))
            out.append(Case(f"window_exact_{o}_{n}", n, "blocks", "shuffled", "none", WINDOW_ROWS, newest, WINDOW[0], WINDOW[1], 0, WINDOW_ROWS, ("tie",)))
            out.append(Case(f"window_above_{o}_{n}", n, "blocks", "shuffled", "none", WINDOW_ROWS + 1, newest, WINDOW[0], WINDOW[1], 0, WINDOW_ROWS, ("tie", "boundary")))
            out.append(Case(f"deny_{o}_{n}", n, "few", "shuffled", "mod3", 1024, newest, None, None, FLAG_DELETED | FLAG_SUPERSEDED, min(1024, n // 3), ("tie",)))
            out.append(Case(f"deny_user_bit_after_{o}_{n}", n, "asc", "row", "mod3", 64, newest, 1000 + 3 * 100, None, 0x100, min(64, (n - 100) - (n - 100 + 2) // 3)))   # rows 100 .. n - 1 without those with row % 3 == 1
        for i, limit in enumerate(LIMITS):
            out.append(Case(f"limit_{limit}_{n}", n, "few", "shuffled", "none", limit, i % 2 == 0, None, None, 0, min(limit, n), ("tie",)))
        out.append(Case(f"none_pass_flags_{n}", n, "asc", "row", "all_deleted", 30, True, None, None, FLAG_DELETED, 0))
        out.append(Case(f"none_pass_range_{n}", n, "asc", "row", "none", 30, False, 1000 + 3 * n, None, 0, 0))
    return out


CASES = _cases()
GRIDS = (1, 2, 3)
