"""Pure-Python restatement of the NSPDK feature vector (ccsd_amd/csrc/ccsd_k_nspdk.h states the steps): what the reference's
vectorize(graphs, complexity=4, discrete=True) computes for graphs whose node and edge labels are integers, with CPython's hash of a
tuple of ints written out in 64-bit integer arithmetic, so that it does not depend on the interpreter that runs it.  Test infrastructure:
the expected side of tests/nspdk_cases.py beside the rows recorded from the reference itself (tests/golden/e4_nspdk.npz)."""
import math

U64 = (1 << 64) - 1
P1, P2, P5 = 11400714785074694791, 14029467366897019727, 2870177450012600261
MERSENNE = (1 << 61) - 1
M32, M16 = (1 << 32) - 1, (1 << 16) - 1
DEPTH = 4                      # radius and distance limit: complexity = 4


def int_hash(x: int) -> int:
    """hash(int) of CPython: sign(x) (|x| mod (2^61 - 1)), with -1 replaced by -2."""
    h = (abs(x) % MERSENNE) * (-1 if x < 0 else 1)
    return -2 if h == -1 else h


def tuple_hash(t) -> int:
    """hash(tuple of ints) of CPython >= 3.8, as a signed 64-bit value."""
    acc = P5
    for x in t:
        acc = (acc + (int_hash(x) & U64) * P2) & U64
        acc = ((acc << 31) | (acc >> 33)) & U64
        acc = (acc * P1) & U64
    acc = (acc + (len(t) ^ (P5 ^ 3527539))) & U64
    if acc == U64:
        return 1546275796
    return acc - (1 << 64) if acc >> 63 else acc


def H(t, mask: int) -> int:
    return (tuple_hash(tuple(t)) & mask) + 1


def graph_of(adj_int, labels):
    """(nodes, {(i, j): edge label, i < j}) of one quantised adjacency (N, N) of non-negative ints and labels (N,): a slot with a
    negative label holds no node; the diagonal and any edge with an absent endpoint are ignored."""
    N = len(labels)
    nodes = [i for i in range(N) if labels[i] >= 0]
    edges = {(i, j): int(adj_int[i][j]) for i in nodes for j in nodes if i < j and adj_int[i][j] != 0}
    return nodes, edges


def neighbourhoods(adj_int, labels, depth: int = DEPTH):
    """(nodes, layers, ngh) of one graph: per root the BFS layers of the expanded graph (even: nodes, odd: edge keys) and the
    neighbourhood hash after each layer."""
    nodes, edges = graph_of(adj_int, labels)
    nbr = {i: [] for i in nodes}                    # node -> [(other node, edge key)]
    for (i, j) in edges:
        nbr[i].append((j, (i, j)))
        nbr[j].append((i, (i, j)))
    vh_node = {i: H((( int_hash(int(labels[i])) & M16) + 1, len(nbr[i])), M32) for i in nodes}
    vh_edge = {e: H(((int_hash(l) & M16) + 1, 2), M32) for e, l in edges.items()}
    layers, ngh = {}, {}
    for r in nodes:
        seen_n, seen_e = {r}, set()
        lay = [[r]]                                 # lay[2 j]: nodes, lay[2 j + 1]: edge keys
        vals = [[vh_node[r]]]
        front = [r]
        while len(lay) <= 2 * depth:
            es = []
            for i in front:
                for (_, e) in nbr[i]:
                    if e not in seen_e:
                        seen_e.add(e)
                        es.append(e)
            if not es:
                break
            lay.append(es)
            vals.append([vh_edge[e] for e in es])
            nxt = []
            for (i, j) in es:
                for k in (i, j):
                    if k not in seen_n:
                        seen_n.add(k)
                        nxt.append(k)
            if not nxt:
                break
            lay.append(nxt)
            vals.append([vh_node[k] for k in nxt])
            front = nxt
        layers[r] = lay
        run, out = 0xAAAAAAAA, []
        for i, v in enumerate(vals):
            run ^= tuple_hash((run, H(sorted(v), M32), i))
            out.append((run & M32) + 1)
        ngh[r] = out
    return nodes, layers, ngh


def features(adj_int, labels, depth: int = DEPTH):
    """{index: value} of one graph, the blocks (rr, dd) in the order of their creation, and the blocks' counts."""
    nodes, layers, ngh = neighbourhoods(adj_int, labels, depth)
    blocks, order = {}, []
    for v in nodes:
        for dd in range(depth + 1):
            if 2 * dd >= len(layers[v]):
                continue
            for u in layers[v][2 * dd]:
                for rr in range(depth + 1):
                    if 2 * rr < len(ngh[v]) and 2 * rr < len(ngh[u]):
                        a, b = ngh[v][2 * rr], ngh[u][2 * rr]
                        if (rr, dd) not in blocks:
                            blocks[(rr, dd)] = {}
                            order.append((rr, dd))
                        blk = blocks[(rr, dd)]
                        for f in (H((min(a, b), max(a, b), 2 * rr, 2 * dd), M16), H((b, 2 * rr, 2 * dd), M16)):
                            blk[f] = blk.get(f, 0) + 1
    merged = {}
    for key in order:
        norm = math.sqrt(sum(c * c for c in blocks[key].values()))
        for f, c in blocks[key].items():
            merged[f] = c / norm                    # assignment: the block created last wins a shared index
    total = math.sqrt(sum(x * x for x in merged.values()))
    return {f: x / total for f, x in merged.items()}, order, blocks


def rows(adj_int, labels):
    """CSR (indptr, indices, values) as numpy arrays for a batch: adj_int (B, N, N), labels (B, N)."""
    import numpy as np

    indptr, idx, val = [0], [], []
    for a, l in zip(adj_int, labels):
        f = features(a.tolist(), l.tolist())[0] if (np.asarray(l) >= 0).any() else {}
        for k in sorted(f):
            idx.append(k)
            val.append(f[k])
        indptr.append(len(idx))
    return np.array(indptr, np.int64), np.array(idx, np.int32), np.array(val, np.float64)


def mmd_mean_form(a, b, drop_empty_b: bool = True):
    """[|mx|^2, |my|^2, mx . my, mmd] of two CSR sets in float64 numpy: the linear-kernel MMD through the two mean vectors."""
    import numpy as np

    means = []
    for (indptr, idx, val), drop in ((a, False), (b, drop_empty_b)):
        n = len(indptr) - 1
        if drop:
            n = int((np.diff(indptr) > 0).sum())
        m = np.zeros(65537)
        np.add.at(m, idx, val)
        means.append(m / n)
    xx, yy, xy = float(means[0] @ means[0]), float(means[1] @ means[1]), float(means[0] @ means[1])
    return [xx, yy, xy, xx + yy - 2 * xy]
