"""A plain Python restatement of the two lifting rules of ccsd_lift (tests only): path sets by recursive enumeration with Python sets
(get_all_paths_from_nodes of the reference, cc_utils.py:1644-1689), the walk of networkx.cycle_basis with dicts, the incidence matrix by
loops (create_incidence_1_2, cc_utils.py:265-330).  It imports neither networkx nor the reference, so it runs wherever the tests run;
tests/test_lift.py checks the cycle walk against networkx itself where networkx is installed."""
import itertools
import math

import numpy as np


def edge_matrix(adj, mol=False, thr=0.5):
    """The graph ccsd_lift reads: pair (i, j), i < j, is an edge when the quantised adj[i][j] (row i = the smaller index) is non-zero;
    the diagonal and the lower triangle are ignored.  -> symmetric (N, N) bool."""
    a = np.asarray(adj, np.float32)
    on = (a >= 0.5) if mol else ~(a < np.float32(thr))
    up = np.triu(on, 1)
    return up | up.T


def neighbours(A):
    return {i: [int(j) for j in np.nonzero(A[i])[0]] for i in range(len(A))}


def _paths_from(n, g, length):
    if length == 1:
        return {frozenset([n])}
    out = set()
    for v in g[n]:
        for p in _paths_from(v, g, length - 1):
            if n not in p:
                out.add(frozenset([n]) | p)
    return out


def path_cells(A, sources=None, path_length=3):
    """The node sets path_based_lift_CC adds: every path of `path_length` nodes that starts at a source (None: every node)."""
    g = {n: nb for n, nb in neighbours(A).items() if nb}              # (the reference's graph dict holds the nodes that have an edge)
    out = set()
    for n in (range(len(A)) if sources is None else sources):
        if n in g:
            out |= _paths_from(n, g, path_length)
    return {c for c in out if len(c) == path_length}


def cycle_basis(A):
    """networkx.cycle_basis(networkx.from_numpy_array(A)) as lists of nodes: the nodes are 0..N-1 in order and every neighbour list
    ascends, so the roots are the highest nodes of their components, taken in descending order."""
    g = neighbours(A)
    gnodes = dict.fromkeys(range(len(A)))
    cycles = []
    while gnodes:
        root = gnodes.popitem()[0]
        stack, pred, used = [root], {root: root}, {root: set()}
        while stack:
            z = stack.pop()
            zused = used[z]
            for nbr in g[z]:
                if nbr not in used:
                    pred[nbr] = z
                    stack.append(nbr)
                    used[nbr] = {z}
                elif nbr not in zused:
                    pn = used[nbr]
                    cycle = [nbr, z]
                    p = pred[z]
                    while p not in pn:
                        cycle.append(p)
                        p = pred[p]
                    cycle.append(p)
                    cycles.append(cycle)
                    used[nbr].add(z)
        for node in pred:
            gnodes.pop(node, None)
    return cycles


def columns(N, d_min, d_max):
    """{node set: column} in get_cells' order (cc_utils.py:72-94), by enumeration."""
    return {frozenset(c): k for k, c in enumerate(itertools.chain.from_iterable(itertools.combinations(range(N), d) for d in range(d_min, d_max + 1)))}


def column_of(c, N, d_min):
    """The same column by counting the combinations that precede sorted(c) (tests/test_lift.py holds it against columns()): the sets of
    a smaller size, then for every position the sets that agree before it and hold a smaller node there."""
    nodes, d = sorted(c), len(c)
    k = sum(math.comb(N, s) for s in range(d_min, d))
    prev = -1
    for pos, x in enumerate(nodes):
        k += sum(math.comb(N - y - 1, d - pos - 1) for y in range(prev + 1, x))
        prev = x
    return k


def lift(adj, procedure, d_min, d_max, sources=None, mol=False, thr=0.5, dense=False):
    """What SampleOps.lift returns for a batch, as numpy arrays (rank2_cell_bits as uint64)."""
    adj = np.asarray(adj)
    B, N = adj.shape[:2]
    K, E = n_columns(N, d_min, d_max), N * (N - 1) // 2
    out = {"rank2_cell_bits": np.zeros((B, (K + 63) // 64), np.uint64), "rank2_cell_count": np.zeros(B, np.int32),
           "rank2_cell_hist": np.zeros((B, d_max - d_min + 1), np.int32), "rank2_nnz": np.zeros(B, np.int32), "lift_dropped": np.zeros(B, np.int32)}
    if dense:
        out["rank2"] = np.zeros((B, E, K), np.float32)
    edge_row = {p: e for e, p in enumerate(itertools.combinations(range(N), 2))}
    for b in range(B):
        A = edge_matrix(adj[b], mol, thr)
        cells = path_cells(A, sources) if procedure == "path_based" else [frozenset(c) for c in cycle_basis(A)]
        seen = set()
        for c in cells:
            if not d_min <= len(c) <= d_max:
                out["lift_dropped"][b] += 1
                continue
            if c in seen:
                continue
            seen.add(c)
            k = column_of(c, N, d_min)
            out["rank2_cell_bits"][b, k >> 6] |= np.uint64(1 << (k & 63))
            out["rank2_cell_count"][b] += 1
            out["rank2_cell_hist"][b, len(c) - d_min] += 1
            for i, j in itertools.combinations(sorted(c), 2):
                if A[i, j]:
                    out["rank2_nnz"][b] += 1
                    if dense:
                        out["rank2"][b, edge_row[(i, j)], k] = 1.0
    return out


def cyclomatic(A):
    """E - V + C of the graph on all N node slots (an isolated slot is a component of its own)."""
    N = len(A)
    comp = list(range(N))

    def find(x):
        while comp[x] != x:
            comp[x] = comp[comp[x]]
            x = comp[x]
        return x

    for i, j in zip(*np.nonzero(np.triu(A, 1))):
        comp[find(int(i))] = find(int(j))
    return int(np.triu(A, 1).sum()) - N + len({find(i) for i in range(N)})


def n_columns(N, d_min, d_max):
    return sum(math.comb(N, d) for d in range(d_min, d_max + 1))
