"""A plain Python restatement of ccsd_mol_correct (tests only): a tiny molecule object with a per-atom bond list in insertion order, and
the three steps of the reference's gen_mol walked literally on it -- construct_mol (formal charges while the bonds are added),
correct_mol (the over-valent atom's highest bond lowered, removed and re-added) and the largest fragment.  It is written from the rules
stated in ccsd_amd/csrc/ccsd_k_mol.h, imports neither rdkit nor the reference, and so runs wherever the tests run.  What rdkit decides in
the reference -- which atom is over-valent -- is the table max_valence[label][charge] here, as in the call under test."""
import numpy as np


def quantize_mol(adj):
    """quantize_mol of the reference (graph_utils.py:195-213) as finish_quant states it: >= 2.5 -> 3, >= 1.5 -> 2, >= 0.5 -> 1, else 0."""
    a = np.asarray(adj, np.float32)
    return (a >= np.float32(0.5)).astype(np.int64) + (a >= np.float32(1.5)) + (a >= np.float32(2.5))


class Mol:
    """Atoms by slot, bonds by unordered pair; bonds_of[a] lists a's bonds in the order they were added (rdkit's atom.GetBonds())."""

    def __init__(self, labels):
        self.label = {i: int(v) for i, v in enumerate(labels) if v >= 0}
        self.charge = {i: 0 for i in self.label}
        self.order = {}                       # (low slot, high slot) -> bond order
        self.bonds_of = {i: [] for i in self.label}
        self.valence = {i: 0 for i in self.label}

    def add_bond(self, a, b, order):
        key = (min(a, b), max(a, b))
        assert key not in self.order and order >= 1
        self.order[key] = order
        for u in (a, b):
            self.bonds_of[u].append(key)      # (a fresh bond goes to the END of both atoms' lists)
            self.valence[u] += order

    def remove_bond(self, a, b):
        key = (min(a, b), max(a, b))
        order = self.order.pop(key)
        for u in (a, b):
            self.bonds_of[u].remove(key)
            self.valence[u] -= order


def check_valency(mol, max_valence):
    """None when no atom is over-valent, else (slot, valence) of the FIRST over-valent atom in slot order."""
    for i in sorted(mol.label):
        if mol.valence[i] > max_valence[mol.label[i]][mol.charge[i]]:
            return i, mol.valence[i]
    return None


def construct_mol(q, labels, max_valence, charge_base):
    """q (N, N) integer bond orders of which pair (i, j), i < j, is read at [i][j].  Bonds enter in ascending (larger, smaller) order."""
    mol = Mol(labels)
    for start in sorted(mol.label):
        for end in sorted(mol.label):
            if end < start and q[end][start]:
                mol.add_bond(start, end, int(q[end][start]))
                bad = check_valency(mol, max_valence)
                if bad is not None:
                    idx, v = bad
                    base = charge_base[mol.label[idx]]
                    if base > 0 and v - base == 1:
                        mol.charge[idx] = 1
    return mol


def correct_mol(mol, max_valence):
    """-> (no_correct, decrements).  The queue is the atom's bonds in insertion order under a STABLE sort by descending order."""
    no_correct = check_valency(mol, max_valence) is None
    n = 0
    while True:
        bad = check_valency(mol, max_valence)
        if bad is None:
            break
        idx = bad[0]
        queue = sorted(mol.bonds_of[idx], key=lambda key: mol.order[key], reverse=True)
        if not queue:                         # (a negative maximum: the reference would spin; the call under test refuses such a table)
            break
        a, b = queue[0]
        t = mol.order[queue[0]] - 1
        mol.remove_bond(a, b)
        if t >= 1:
            mol.add_bond(a, b, t)
        n += 1
    return no_correct, n


def fragments(mol):
    """Connected components as sorted slot lists, in ascending order of their lowest slot."""
    nbrs = {i: set() for i in mol.label}
    for a, b in mol.order:
        nbrs[a].add(b)
        nbrs[b].add(a)
    seen, out = set(), []
    for root in sorted(mol.label):
        if root in seen:
            continue
        comp, todo = {root}, [root]
        while todo:
            for v in nbrs[todo.pop()]:
                if v not in comp:
                    comp.add(v)
                    todo.append(v)
        seen |= comp
        out.append(sorted(comp))
    return out


def mol_correct(adj, labels, max_valence, charge_base, largest_fragment=True):
    """The outputs of SampleOps.mol_correct as numpy arrays, molecule by molecule."""
    adj = np.asarray(adj, np.float32)
    labels = np.asarray(labels)
    B, N = labels.shape
    L = len(max_valence)
    assert labels.max(initial=-1) < L
    out = {"mol_adj": np.zeros((B, N, N), np.uint8), "mol_labels": np.full((B, N), -1, np.int32), "mol_charge": np.zeros((B, N), np.int8),
           "mol_no_correct": np.zeros(B, np.uint8), "mol_n_corrections": np.zeros(B, np.int32), "mol_n_fragments": np.zeros(B, np.int32),
           "mol_atoms": np.zeros(B, np.int32)}
    for b in range(B):
        mol = construct_mol(quantize_mol(adj[b]), labels[b], max_valence, charge_base)
        no_correct, n = correct_mol(mol, max_valence)
        frags = fragments(mol)
        keep = set(mol.label)
        if largest_fragment and frags:
            keep = set(max(frags, key=len))                              # (max returns the FIRST of equally long fragments)
        for i in keep:
            out["mol_labels"][b, i] = mol.label[i]
            out["mol_charge"][b, i] = mol.charge[i]
        for (i, j), o in mol.order.items():
            if i in keep and j in keep:
                out["mol_adj"][b, i, j] = out["mol_adj"][b, j, i] = o
        out["mol_no_correct"][b] = no_correct
        out["mol_n_corrections"][b] = n
        out["mol_n_fragments"][b] = len(frags)
        out["mol_atoms"][b] = len(keep)
    return out
