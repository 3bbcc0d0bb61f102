"""The BP+LSD law of higher order (include/qldpc_hip.h, "BP+LSD of higher order") in plain Python: the
reference of the host stage (csrc/lsd.hip, qldpc_osd_create_lsd_order), which in turn is the reference of
the kernel.

Written literally on ``lsd_ref``'s ``Graph`` and ``column_order``: every round forms the clusters anew as
connected components and eliminates each afresh; every candidate is built as a set of columns and weighed
by the integer weights ``wq`` it is given (``qldpc_lsd_weights``), so bit equality does not hang on a libm.

``decode`` also counts, per decode, the events the test table must exercise (``EVENTS``), and reports
``max_candidates``, the largest number of candidates after candidate 0 that a cluster of the decode had.
"""
from __future__ import annotations

import numpy as np

from lsd_ref import Graph, column_order

METHODS = {"lsd_0": 0, "lsd_e": 1, "lsd_cs": 2}

EVENTS = ("grown_valid",                # a valid cluster (free < w) nominated a column
          "growth_merged_valid",        # a new cluster holds two or more old clusters, a valid one among them
          "growth_invalidated",         # an invalid new cluster holds an old cluster that was valid
          "T_cut_short",                # a valid final cluster with 0 < |F| < w
          "replaced",                   # a candidate beat candidate 0 (the winner of a cluster is not x0)
          "tie_kept",                   # a candidate as heavy as the incumbent did not replace it
          "lighter_with_more_columns",  # a candidate replaced an incumbent that has fewer set bits
          "cs_single_beyond_T")         # lsd_cs: the winner of a cluster is {f} with f outside T


def _split(cols, masks, s):
    """Walk ``cols`` (in column order) as OSD-0 does: (valid, kept columns P, free columns F with dep(f) as a
    set of kept columns, the OSD-0 solution x0 as a set of columns).  Echelon basis keyed by the lowest set
    bit; each vector carries the set of kept columns it is the xor of, as a bit mask over P."""
    basis, kept, free = {}, [], []
    for j in cols:
        v, c = masks[j], 0
        while v:
            p = v & -v
            if p not in basis:
                basis[p] = (v, c | (1 << len(kept)))
                kept.append(j)
                break
            v, c = v ^ basis[p][0], c ^ basis[p][1]
        else:
            free.append((j, frozenset(kept[t] for t in range(len(kept)) if (c >> t) & 1)))
    c = 0
    while s:
        p = s & -s
        if p not in basis:
            return False, kept, free, frozenset()
        s, c = s ^ basis[p][0], c ^ basis[p][1]
    return True, kept, free, frozenset(kept[t] for t in range(len(kept)) if (c >> t) & 1)


def _candidates(method, F, w):
    """The candidate sets t after candidate 0, in the law's order, as tuples of indices into F."""
    T = min(w, len(F))
    if method == 1:
        for c in range(1, 1 << T):
            yield tuple(i for i in range(T) if (c >> i) & 1)
    else:
        for a in range(len(F)):
            yield (a,)
        for a in range(T):
            for b in range(a + 1, T):
                yield (a, b)


def decode(g: Graph, synd, post, k: int, method, w: int, wq):
    """(x0 [n] uint8, xw [n] uint8, stats [4] int32 = valid, rounds, |A|, clusters; events dict)."""
    method = METHODS.get(method, method)
    assert k >= 1 and method in (0, 1, 2) and w >= 0
    if method == 0:
        w = 0
    wq = [int(v) for v in wq]
    order = column_order(post)
    rank = np.empty(g.n, np.int64)
    rank[order] = np.arange(g.n)
    rank = rank.tolist()
    seeds = np.flatnonzero(np.asarray(synd) & 1).tolist()
    smask = sum(1 << i for i in seeds)
    A, R = set(), set(seeds)
    ev = dict.fromkeys(EVENTS + ("max_candidates",), 0)

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
            rmask = sum(1 << r for r in rows)
            res.append((rows, cols) + _split(cols, g.col_mask, smask & rmask))
        return res

    rounds = 0
    old = {}  # row -> (cluster id, valid) of the round before
    while True:
        cl = clusters()
        for cid, (rows, cols, valid, kept, free, x0) in enumerate(cl):
            assert len(free) == len(cols) - len(kept)  # free(C) = |cols| - rank
            olds = {old[r] for r in rows if r in old}
            if len(olds) >= 2 and any(v for _, v in olds):
                ev["growth_merged_valid"] += 1
                if not valid:
                    ev["growth_invalidated"] += 1
        old = {r: (cid, c[2]) for cid, c in enumerate(cl) for r in c[0]}
        picked = set()
        for rows, cols, valid, kept, free, x0 in cl:
            if valid and len(free) >= w:
                continue
            boundary = sorted({j for r in rows for j in g.row_cols[r] if j not in A}, key=rank.__getitem__)
            if valid and boundary:
                ev["grown_valid"] += 1
            picked.update(boundary[:k])
        if not picked:
            break
        rounds += 1
        for j in picked:
            A.add(j)
            R.update(g.col_rows[j])

    x0v, xwv = np.zeros(g.n, np.uint8), np.zeros(g.n, np.uint8)
    ok = 1
    for rows, cols, valid, kept, free, x0 in cl:
        if not valid:
            ok = 0
            continue
        weight = lambda s: sum(wq[j] for j in s)  # noqa: E731
        best, best_t = x0, None
        if 0 < len(free) < w:
            ev["T_cut_short"] += 1
        if w:
            T = min(w, len(free))
            ev["max_candidates"] = max(ev["max_candidates"], (1 << T) - 1 if method == 1 else len(free) + T * (T - 1) // 2)
        for t in _candidates(method, free, w) if w else ():
            x = x0
            for i in t:
                x = x ^ (free[i][1] | {free[i][0]})  # e_f + dep(f)
            if weight(x) < weight(best):
                if len(x) > len(best):
                    ev["lighter_with_more_columns"] += 1
                best, best_t = x, t
            elif weight(x) == weight(best):
                ev["tie_kept"] += 1
        if best_t is not None:
            ev["replaced"] += 1
            if method == 2 and len(best_t) == 1 and best_t[0] >= min(w, len(free)):
                ev["cs_single_beyond_T"] += 1
        x0v[sorted(x0)] = 1
        xwv[sorted(best)] = 1
    stats = np.array([ok, rounds, len(A), len(cl) if R else 0], np.int32)
    # what holds of every output of the law: both solve the syndrome on the rows of the valid clusters
    for x in (x0v, xwv):
        Hx = np.zeros(g.m, np.int64)
        for j in np.flatnonzero(x):
            Hx[g.col_rows[j]] ^= 1
        for rows, cols, valid, kept, free, _ in cl:
            if valid:
                assert all(Hx[r] == ((smask >> r) & 1) for r in rows)
    return x0v, xwv, stats, ev


def decode_batch(H, synd, post, k: int, method, w: int, wq):
    """(x0 [B, n], xw [B, n], stats [B, 4], summed events and the largest ``max_candidates``) over a batch."""
    g = H if isinstance(H, Graph) else Graph(H)
    S, P = np.atleast_2d(synd), np.atleast_2d(post)
    X0 = np.zeros((S.shape[0], g.n), np.uint8)
    XW = np.zeros((S.shape[0], g.n), np.uint8)
    T = np.zeros((S.shape[0], 4), np.int32)
    tot = dict.fromkeys(EVENTS + ("max_candidates",), 0)
    for b in range(S.shape[0]):
        X0[b], XW[b], T[b], ev = decode(g, S[b], P[b], k, method, w, wq)
        for e in EVENTS:
            tot[e] += ev[e]
        tot["max_candidates"] = max(tot["max_candidates"], ev["max_candidates"])
    return X0, XW, T, tot
