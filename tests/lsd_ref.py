"""The BP+LSD law (include/qldpc_hip.h, "BP+LSD") in plain Python: the reference of the host stage
(csrc/lsd.hip), which in turn is the reference of the kernel.

Written literally, not as the native stages work: every round forms the clusters anew as connected
components and decides each cluster's validity by a fresh GF(2) elimination (cached per column set),
where the native stages keep one incremental basis.  Bit-vectors over rows are Python ints.

``decode`` also counts, per decode, the events the test table must exercise (``EVENTS``).
"""
from __future__ import annotations

import numpy as np

EVENTS = ("merge_invalid_invalid",   # a new cluster holding two or more clusters that were invalid
          "valid_made_invalid",      # an invalid new cluster holding a cluster that was valid
          "unsolvable",              # invalid clusters without boundary at the end
          "cut_short",               # a nomination of 0 < |boundary| < k columns
          "nominated_twice")         # a column nominated by two clusters in one round


def column_order(post) -> np.ndarray:
    """Columns in the law's order: ascending posterior, ties (-0 = +0 among them) by index."""
    return np.argsort(np.asarray(post, dtype=np.float64), kind="stable")


class Graph:
    def __init__(self, H):
        H = np.asarray(H)
        self.m, self.n = H.shape
        self.row_cols = [np.flatnonzero(H[i]).tolist() for i in range(self.m)]
        self.col_rows = [np.flatnonzero(H[:, j]).tolist() for j in range(self.n)]
        self.col_mask = [sum(1 << r for r in rows) for rows in self.col_rows]


def _osd0(cols, masks, s):
    """OSD-0 on the columns ``cols`` (in column order) with row masks ``masks``: (s in the span,
    the columns of the solution).  Echelon basis keyed by the lowest set bit, each vector with the
    combination of kept columns it stands for."""
    basis, kept = {}, []
    for j in cols:
        v, c = masks[j], 1 << len(kept)
        while v:
            p = v & -v
            if p not in basis:
                basis[p] = (v, c)
                kept.append(j)
                break
            v, c = v ^ basis[p][0], c ^ basis[p][1]
    c = 0
    while s:
        p = s & -s
        if p not in basis:
            return False, []
        s, c = s ^ basis[p][0], c ^ basis[p][1]
    return True, [kept[t] for t in range(len(kept)) if (c >> t) & 1]


def decode(g: Graph, synd, post, k: int):
    """(x [n] uint8, stats [4] int32 = valid, rounds, |A|, clusters; events dict)."""
    assert k >= 1
    order = column_order(post)
    rank = np.empty(g.n, np.int64)
    rank[order] = np.arange(g.n)
    rank = rank.tolist()
    smask = sum(1 << i for i in np.flatnonzero(np.asarray(synd) & 1).tolist())
    A, R = set(), set(np.flatnonzero(np.asarray(synd) & 1).tolist())
    ev = dict.fromkeys(EVENTS, 0)
    x = np.zeros(g.n, np.uint8)
    cache = {}

    def clusters():
        parent = {i: i for i in R}

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        for j in A:
            rows = g.col_rows[j]
            for r in rows[1:]:
                parent[find(r)] = find(rows[0])
        out = {}
        for i in R:
            out.setdefault(find(i), ([], []))[0].append(i)
        for j in A:
            out[find(g.col_rows[j][0])][1].append(j)
        res = []
        for rows, cols in out.values():
            cols.sort(key=rank.__getitem__)
            key = (tuple(cols), rows[0] if not cols else -1)
            if key not in cache:
                rmask = sum(1 << r for r in rows)
                cache[key] = _osd0(cols, g.col_mask, smask & rmask)
            res.append((rows, cols) + cache[key])
        return res

    rounds = 0
    old = {}  # row -> (cluster id, valid) of the round before
    while True:
        cl = clusters()
        for cid, (rows, cols, valid, sol) in enumerate(cl):
            olds = {old[r] for r in rows if r in old}
            if sum(1 for _, v in olds if not v) >= 2:
                ev["merge_invalid_invalid"] += 1
            if not valid and len(olds) >= 2:
                ev["valid_made_invalid"] += sum(1 for _, v in olds if v)
        old = {r: (cid, valid) for cid, (rows, _, valid, _) in enumerate(cl) for r in rows}
        picked = {}
        for rows, cols, valid, sol in cl:
            if valid:
                continue
            boundary = sorted({j for r in rows for j in g.row_cols[r] if j not in A}, key=rank.__getitem__)
            if 0 < len(boundary) < k:
                ev["cut_short"] += 1
            for j in boundary[:k]:
                picked[j] = picked.get(j, 0) + 1
        if not picked:
            break
        rounds += 1
        ev["nominated_twice"] += sum(1 for c in picked.values() if c >= 2)
        for j in picked:
            A.add(j)
            R.update(g.col_rows[j])
    ok = 1
    for rows, cols, valid, sol in cl:
        if valid:
            x[sol] = 1
        else:
            ok = 0
            ev["unsolvable"] += 1
    stats = np.array([ok, rounds, len(A), len(cl) if R else 0], np.int32)
    # what holds of every output of the law
    Hx = np.zeros(g.m, np.int64)
    for j in np.flatnonzero(x):
        Hx[g.col_rows[j]] ^= 1
    for rows, cols, valid, sol in cl:
        if valid:
            assert all(Hx[r] == ((smask >> r) & 1) for r in rows)
    return x, stats, ev


def decode_batch(H, synd, post, k: int):
    """(x [B, n], stats [B, 4], summed events) over a batch."""
    g = H if isinstance(H, Graph) else Graph(H)
    S, P = np.atleast_2d(synd), np.atleast_2d(post)
    X = np.zeros((S.shape[0], g.n), np.uint8)
    T = np.zeros((S.shape[0], 4), np.int32)
    tot = dict.fromkeys(EVENTS, 0)
    for b in range(S.shape[0]):
        X[b], T[b], ev = decode(g, S[b], P[b], k)
        for e in EVENTS:
            tot[e] += ev[e]
    return X, T, tot
