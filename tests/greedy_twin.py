"""The greedy representatives of an edge list in plain Python loops, written from the rule of include/bsq.h ("greedy representatives")
alone: nothing of the library is called.  The tests of the CPU twin and of the kernels compare against it and share the lists made
here."""
import numpy as np


def comes_before(key, u, v):
    """(key[u], u) < (key[v], v); key None is index order."""
    return u < v if key is None else (int(key[u]), u) < (int(key[v]), v)


def edges_of(row, col, n, weight=None):
    """{(u, v) with u < v: the largest weight of the entries that join them (0 without weights)}; an entry with row == col or an index
    outside 0 .. n - 1 is ignored."""
    edges = {}
    for k in range(len(row)):
        i, j = int(row[k]), int(col[k])
        if i == j or not 0 <= i < n or not 0 <= j < n:
            continue
        w = 0 if weight is None else int(weight[k])
        e = (min(i, j), max(i, j))
        edges[e] = max(edges.get(e, w), w)
    return edges


def greedy_reps(row, col, n, key=None, weight=None):
    """rep (int64, n): visit the nodes in the order; a node is a representative iff none of its neighbours that come before it is one.
    A member takes, among its representative neighbours that come before it, the one with the largest weight, ties (and all of them
    without weights) to the one that comes first in the order."""
    neighbours = [[] for _ in range(n)]
    for (i, j), w in edges_of(row, col, n, weight).items():
        neighbours[i].append((j, w))
        neighbours[j].append((i, w))
    order = sorted(range(n), key=(lambda v: v) if key is None else (lambda v: (int(key[v]), v)))
    visited, rep = [False] * n, [-1] * n
    for v in order:
        best = None  # (-weight, key, index): the smallest wins
        for u, w in neighbours[v]:
            if visited[u] and rep[u] == u:
                assert comes_before(key, u, v)
                cand = (-w, 0 if key is None else int(key[u]), u)
                best = cand if best is None or cand < best else best
        rep[v] = v if best is None else best[2]
        visited[v] = True
    return np.array(rep, np.int64)


def check_consequences(row, col, n, rep, key=None):
    """The consequences the header states, as assertions."""
    edges = edges_of(row, col, n)
    linked = set(edges) | {(j, i) for i, j in edges}
    for i, j in edges:
        assert not (rep[i] == i and rep[j] == j), "an entry joins two representatives"
    for i in range(n):
        r = int(rep[i])
        assert 0 <= r < n and rep[r] == r
        if r != i:
            assert (i, r) in linked, "a member without an entry to its representative"
            assert comes_before(key, r, i), "a representative that comes after its member"
        if key is None:
            assert r <= i


def random_list(seed, n, m, junk=True):
    """m random entries over n nodes in both orientations, with duplicates, self-entries and, with junk, indices outside 0 .. n - 1 at both
    ends of the range."""
    rng = np.random.default_rng(seed)
    row, col = rng.integers(0, n, m, dtype=np.int64), rng.integers(0, n, m, dtype=np.int64)
    dup = rng.integers(0, m, m // 10)
    row[: dup.size], col[: dup.size] = col[dup], row[dup]  # (a tenth of the list repeats entries, ends exchanged)
    if junk and m >= 8:
        at = rng.choice(m, 8, replace=False)
        row[at] = [-1, n, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, n - 1, 0, n - 1]
        col[at] = [0, n - 1, 0, n - 1, -1, n, np.iinfo(np.int64).max, np.iinfo(np.int64).min]
    return row, col


def path(n, perm=None):
    """The path 0 -- 1 -- ... -- n - 1, or the same path laid out through a permutation of the nodes."""
    a, b = np.arange(n - 1, dtype=np.int64), np.arange(1, n, dtype=np.int64)
    return (a, b) if perm is None else (np.ascontiguousarray(perm[a]), np.ascontiguousarray(perm[b]))


def complete(n):
    i, j = np.triu_indices(n, 1)
    return i.astype(np.int64), j.astype(np.int64)


def keys_and_weights(seed, n, m):
    """A key with many ties and a weight with many ties."""
    rng = np.random.default_rng(seed + 1000)
    return rng.integers(-3, 4, n, dtype=np.int64), rng.integers(-2, 3, m).astype(np.int32)


def families(seed=5, count=12, children=4, length=200):
    """The planted families of the pipeline tests as a packed DNA4 batch: (chars uint8, offsets int64, parent int64).  Each family is
    one random parent of `length` characters followed by its children, copies with about 2 % substitutions and 0 .. 4 characters trimmed
    from the end; parent[i] is the row of row i's parent (its own for a parent).  A parent is the longest row of its family, or as
    long as a child and earlier."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    rows, parent = [], []
    for _ in range(count):
        base = rng.integers(0, 4, length)
        first = len(rows)
        rows.append(base)
        parent.append(first)
        for _ in range(children):
            child = base.copy()
            hit = rng.random(length) < 0.02
            child[hit] = (child[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
            rows.append(child[: length - int(rng.integers(0, 5))])
            parent.append(first)
    offsets = np.zeros(len(rows) + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return letters[np.concatenate(rows)].copy(), offsets, np.array(parent, np.int64)
