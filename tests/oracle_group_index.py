"""TEST INFRASTRUCTURE: the reference recipe the GPU tests hold ``vs_search_groups`` to, written as
plain loops, and an ``OracleGroupFlatIndex`` with FlatIndex's ``group_keys`` / ``search_groups`` surface
so ``VectorStore.search_grouped`` runs on the CPU.

Recipe (include/vs.h "grouped search"): the members ranked by the oracle's canonical fp64 score, ties
to the lower id; walked best first to the end; rows with the same non-negative key form a group, a row
with a negative key is a group of its own; the groups in order of first appearance, the first ``k`` of
them, each with its first ``g`` rows.  ``group_reference`` knows nothing of lists, tiers or rounds; it
also returns ``need[q]``, the 1-based rank at which the answer became complete, from which the tests
derive the tier a query must end in.  ``expected_rounds`` replays the contract's restricted rounds on
the same ranking (lists are prefixes of the ranking of a row subset) to say how many a query takes."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle_diverse_index import OracleDiverseFlatIndex
from oracle_remove_index import OracleRemoveFlatIndex
from oracle_sel_index import FLT_MAX
from photo_search_engine_amd.index import GroupedResult, group_args, group_key_array

KEY_PAD = np.iinfo(np.int64).min


def _ranking(xs, q, metric: str, ids):
    """Per query, the member ids in ``vs_search``'s total order, and their canonical scores."""
    S = O.canon_scores(xs[ids], q, metric)  # (nq, members) fp64
    orders = [np.lexsort((ids, -S[qi] if metric == "ip" else S[qi])) for qi in range(S.shape[0])]
    return S, orders


def group_reference(xs, q, keys, k: int, g: int, metric: str, mask=None):
    """(keys int64 nq x k, D float32 nq x k x g, I int64 nq x k x g, found int32 nq x k, sizes int64
    nq x k, need int64 nq) of ``search_groups(q, k, groups(keys), g)`` over rows ``xs`` (the values as
    stored; ``keys`` covers the first ``len(keys)`` of them); ``mask`` restricts the members."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    keys = np.asarray(keys, dtype=np.int64)
    nq, k, g = int(q.shape[0]), int(k), int(g)
    ip = metric == "ip"
    Ko = np.full((nq, k), KEY_PAD, dtype=np.int64)
    D = np.full((nq, k, g), -FLT_MAX if ip else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k, g), -1, dtype=np.int64)
    found = np.zeros((nq, k), dtype=np.int32)
    sizes = np.zeros((nq, k), dtype=np.int64)
    need = np.zeros((nq,), dtype=np.int64)
    member = np.ones((keys.shape[0],), dtype=bool)
    if mask is not None:
        member &= np.asarray(mask, dtype=bool)[: keys.shape[0]]
    ids = np.flatnonzero(member).astype(np.int64)
    if nq == 0 or ids.shape[0] == 0:
        return Ko, D, I, found, sizes, need
    size_m = {}
    for i in ids.tolist():
        tok = int(keys[i]) if keys[i] >= 0 else ("row", i)
        size_m[tok] = size_m.get(tok, 0) + 1
    target = min(k, len(size_m))
    S, orders = _ranking(xs, q, metric, ids)
    for qi in range(nq):
        slot_of = {}
        full = 0
        for rank, pos in enumerate(orders[qi].tolist(), start=1):
            row = int(ids[pos])
            tok = int(keys[row]) if keys[row] >= 0 else ("row", row)
            s = slot_of.get(tok)
            if s is None:
                if len(slot_of) == k:
                    continue
                s = slot_of[tok] = len(slot_of)
                Ko[qi, s] = keys[row]
                sizes[qi, s] = size_m[tok]
            if found[qi, s] == g:
                continue
            I[qi, s, found[qi, s]] = row
            D[qi, s, found[qi, s]] = np.float32(S[qi, pos])
            found[qi, s] += 1
            if found[qi, s] == min(g, size_m[tok]):
                full += 1
            if len(slot_of) == target and full == target and need[qi] == 0:
                need[qi] = rank
    return Ko, D, I, found, sizes, need


def _walk(rows, tokens, size_m, g, k_target):
    """The contract's walk over a list: {token: rows taken} in order of first appearance, complete?"""
    taken = {}
    full = 0
    for row, tok in zip(rows, tokens):
        if tok not in taken:
            if len(taken) == k_target:
                continue
            taken[tok] = []
        if len(taken[tok]) == min(g, size_m[tok]):
            continue
        taken[tok].append(row)
        if len(taken[tok]) == min(g, size_m[tok]):
            full += 1
        if len(taken) == k_target and full == k_target:
            return taken, True
    return taken, False


def expected_rounds(xs, q, keys, k: int, g: int, metric: str, first: int, limit: int, mask=None):
    """Per query, (tier, rounds): tier 0 / 1 / 2 = complete after the first list, after a deeper list,
    finished by restricted rounds, and the restricted rounds that takes -- the contract's scheme
    replayed on the reference ranking (first / limit as ``set_group_depth`` resolves them)."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    keys = np.asarray(keys, dtype=np.int64)
    member = np.ones((keys.shape[0],), dtype=bool)
    if mask is not None:
        member &= np.asarray(mask, dtype=bool)[: keys.shape[0]]
    ids = np.flatnonzero(member).astype(np.int64)
    members = int(ids.shape[0])
    if members == 0:
        return [(0, 0)] * int(q.shape[0])
    tok_of = {int(i): (int(keys[i]) if keys[i] >= 0 else ("row", int(i))) for i in ids.tolist()}
    size_m = {}
    for t in tok_of.values():
        size_m[t] = size_m.get(t, 0) + 1
    target = min(int(k), len(size_m))
    _, orders = _ranking(xs, q, metric, ids)
    out = []
    for order in orders:
        rank = [int(ids[p]) for p in order.tolist()]
        toks = [tok_of[r] for r in rank]
        L, Lmax = min(first, limit, members), min(limit, members)
        taken, done = _walk(rank[:L], toks[:L], size_m, g, target)
        tier = 0
        while not (done or L >= members) and L < Lmax:
            L, tier = min(4 * L, Lmax), 1
            taken, done = _walk(rank[:L], toks[:L], size_m, g, target)
        if done or L >= members:
            out.append((tier, 0))
            continue
        rounds = 0
        while True:
            short = [t for t, rows in taken.items() if len(rows) < min(g, size_m[t])]
            is_open = len(taken) < target
            if not short and not is_open:
                break
            keep = [(r, t) for r, t in zip(rank, toks) if t in short or (is_open and t not in taken)]
            if not keep:
                break
            rounds += 1
            depth = min(limit, len(keep))
            got, _ = _walk([r for r, _ in keep[:depth]], [t for _, t in keep[:depth]], size_m, g,
                           len(short) + target - len(taken))
            for t, rows in got.items():
                assert t not in taken or taken[t] == rows[: len(taken[t])]
                taken[t] = rows
            if depth >= len(keep):
                break
        out.append((2, rounds))
    return out


class OracleGroups:
    def __init__(self, index: "OracleGroupFlatIndex", keys) -> None:
        self.keys = group_key_array(keys, index.ntotal)
        self.generation = index._generation

    @property
    def count(self) -> int:
        return int(np.unique(self.keys[self.keys >= 0]).shape[0])

    @property
    def rows(self) -> int:
        return int(self.keys.shape[0])

    def close(self) -> None:
        pass


class OracleGroupFlatIndex(OracleDiverseFlatIndex, OracleRemoveFlatIndex):
    def group_keys(self, keys) -> OracleGroups:
        return OracleGroups(self, keys)

    def search_groups(self, q, k: int, groups, group_size: int = 1, sel=None) -> GroupedResult:
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"search_groups expects an (nq, {self.d}) array, got {q.shape}")
        try:
            k, g = group_args(k, group_size)
        except ValueError as e:
            raise RuntimeError(str(e))
        if groups.generation != self._generation or groups.rows > self.ntotal:
            raise RuntimeError("stale groups")
        return GroupedResult(*group_reference(self._x, q, groups.keys, k, g, "ip" if self.metric_type == 0 else "l2",
                                              self._mask(sel))[:5])


def oracle_group_factory(dimension: int, metric: str):
    return OracleGroupFlatIndex(dimension, "ip" if metric == "cosine" else "l2")


def burst_keys(nbase: int = 40, seed: int = 7, d: int = 72):
    """The burst id of every row of ``burst_corpus(d, nbase, seed=seed)``, shuffled alongside the rows
    (the same generator calls in the same order, with the ids riding the shuffle)."""
    rng = np.random.default_rng(seed)
    rng.standard_normal((nbase, d))
    burst = []
    for b in range(nbase):
        for _ in range(1 + (5 * b) % 12):
            rng.standard_normal(d)
            burst.append(b)
    burst = np.asarray(burst, dtype=np.int64)
    perm = np.arange(burst.shape[0])
    rng.shuffle(perm)  # (the permutation a shuffle of as many rows draws from this state)
    out = burst[perm]
    out.setflags(write=False)
    return out
