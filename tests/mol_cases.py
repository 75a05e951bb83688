"""Shared cases for molecule post-processing (ccsd_mol_correct, SampleOps.mol_correct, evaluation.MOL_TABLES, Sampler.molecules and
Sampler.evaluate(correct=True)): the inputs, the checks against the plain Python restatement of tests/mol_ref.py and the properties every
output has.  Shared by the host-emulation suite (tests/test_mol.py) and the GPU suite (tests/test_gpu_mol.py, -m gpu); `lib` / `device`
select the backend.  A restatement result is computed once per case and shared (reference())."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ccsd_amd import _lib
from ccsd_amd import evaluation as ev
from ccsd_amd import samples as samples_mod
from tests import mol_ref
from tests.helpers import sample_ops

QM9, ZINC = ev.MOL_TABLES["QM9"], ev.MOL_TABLES["ZINC250k"]
C_, N_, O_, F_ = 0, 1, 2, 3                  # the labels of both tables' first four rows
OUTPUTS = _lib.MOL_OUTPUTS
BELOW = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))


# ---- handcrafted molecules: labels, bonds (i, j, value of adj at BOTH [i][j] and [j][i]) or a dense adj, and what must come out ------------
def _adj(N, bonds, lower=None):
    a = np.zeros((N, N), np.float32)
    for i, j, v in bonds:
        a[i, j] = a[j, i] = v
    if lower is not None:                        # an asymmetric adjacency: the lower triangle says something else
        for i, j, v in lower:
            a[max(i, j), min(i, j)] = v
    return a


def _pad(labels, N, fill=-1):
    return list(labels) + [fill] * (N - len(labels))


HN = 12          # every handcrafted molecule is padded to 12 slots: one batch per setting of largest_fragment
# name -> (labels, adj, expected outputs with largest_fragment=True, ... =False); an expected mol_adj is given as bonds (i, j, order)
HAND = {
    # (a) N with four single bonds takes charge +1 and is not corrected; O with three likewise
    "a_charged_N": (_pad([N_, C_, C_, C_, C_], HN), _adj(HN, [(0, k, 1) for k in (1, 2, 3, 4)]),
                    dict(mol_charge=_pad([1], HN, 0), mol_no_correct=1, mol_n_corrections=0, mol_atoms=5, mol_n_fragments=1,
                         bonds=[(0, k, 1) for k in (1, 2, 3, 4)]), None),
    "a_charged_O": (_pad([C_, O_, C_, C_], HN), _adj(HN, [(1, 0, 1), (1, 2, 1), (1, 3, 1)]),
                    dict(mol_charge=_pad([0, 1], HN, 0), mol_no_correct=1, mol_n_corrections=0, mol_atoms=4), None),
    # (b) C with five single bonds loses the bond of lowest insertion number, (1, 0): atom 1 becomes a fragment of its own
    "b_overvalent_C": (_pad([C_] * 6, HN), _adj(HN, [(0, k, 1) for k in range(1, 6)]),
                       dict(mol_no_correct=0, mol_n_corrections=1, mol_n_fragments=2, mol_atoms=5, mol_labels=_pad([C_, -1, C_, C_, C_, C_], HN),
                            bonds=[(0, k, 1) for k in range(2, 6)]),
                       dict(mol_atoms=6, mol_labels=_pad([C_] * 6, HN), bonds=[(0, k, 1) for k in range(2, 6)])),
    # (c) a triple and two single bonds on a C: the triple is lowered first (and once is enough)
    "c_highest_first": (_pad([C_] * 4, HN), _adj(HN, [(0, 1, 1), (0, 2, 3), (0, 3, 1)]),
                        dict(mol_n_corrections=1, bonds=[(0, 1, 1), (0, 2, 2), (0, 3, 1)], mol_atoms=4), None),
    # (d) C with a triple (inserted first) and two double bonds, 7 > 4: the triple drops to 2 and is re-added with a FRESH number, so the
    # two older doubles are hit next, in their order: 2, 1, 1.  With the old number kept, the first bond would be hit twice: 1, 1, 2.
    "d_readded_goes_last": (_pad([C_] * 4, HN), _adj(HN, [(0, 1, 3), (0, 2, 2), (0, 3, 2)]),
                            dict(mol_n_corrections=3, bonds=[(0, 1, 2), (0, 2, 1), (0, 3, 1)], mol_atoms=4), None),
    # (e) the over-valent C at slot 0 masks the N at slot 6, which reaches 4 while C is still reported: N stays neutral and loses a bond
    # (both lose their bond to atom 1, which becomes a fragment of its own)
    "e_masking": (_pad([C_, C_, C_, C_, C_, C_, N_], HN), _adj(HN, [(0, k, 1) for k in range(1, 6)] + [(6, k, 1) for k in (1, 2, 3, 4)]),
                  dict(mol_charge=[0] * HN, mol_no_correct=0, mol_n_corrections=2, mol_atoms=6, mol_n_fragments=2,
                       bonds=[(0, k, 1) for k in range(2, 6)] + [(6, k, 1) for k in (2, 3, 4)]), None),
    #     ... and with the slots exchanged (N first) nothing masks it: charged, one correction
    "e_unmasked": (_pad([N_, C_, C_, C_, C_, C_, C_], HN), _adj(HN, [(6, k, 1) for k in range(1, 6)] + [(0, k, 1) for k in (1, 2, 3, 4)]),
                   dict(mol_charge=_pad([1], HN, 0), mol_no_correct=0, mol_n_corrections=1, mol_atoms=7, mol_n_fragments=1), None),
    # (f) two fragments of equal size: the one holding the lower slot wins; a larger fragment at higher slots wins over a smaller one
    "f_tie": (_pad([C_, O_, N_, C_], HN), _adj(HN, [(0, 1, 1), (2, 3, 2)]),
              dict(mol_n_fragments=2, mol_atoms=2, mol_labels=_pad([C_, O_], HN), bonds=[(0, 1, 1)]),
              dict(mol_n_fragments=2, mol_atoms=4, bonds=[(0, 1, 1), (2, 3, 2)])),
    "f_larger_later": (_pad([C_, O_, N_, C_, C_], HN), _adj(HN, [(0, 1, 1), (2, 3, 2), (3, 4, 1)]),
                       dict(mol_n_fragments=2, mol_atoms=3, mol_labels=_pad([-1, -1, N_, C_, C_], HN), bonds=[(2, 3, 2), (3, 4, 1)]), None),
    # (g) slots without an atom in the middle, and bonds pointing at them (ignored, whatever their order)
    "g_holes": ([C_, -1, C_, C_, -1, N_] + [-1] * (HN - 6), _adj(HN, [(0, 1, 3), (0, 2, 1), (2, 3, 2), (3, 4, 3), (3, 5, 1), (1, 4, 2), (5, 7, 3)]),
                dict(mol_no_correct=1, mol_n_corrections=0, mol_n_fragments=1, mol_atoms=4, mol_labels=[C_, -1, C_, C_, -1, N_] + [-1] * (HN - 6),
                     bonds=[(0, 2, 1), (2, 3, 2), (3, 5, 1)]), None),
    # (h) no atom at all (the bonds of the input are ignored); one atom
    "h_empty": ([-1] * HN, _adj(HN, [(0, 1, 3), (2, 5, 1)]),
                dict(mol_no_correct=1, mol_n_corrections=0, mol_n_fragments=0, mol_atoms=0, mol_labels=[-1] * HN, bonds=[]), None),
    "h_single": ([-1, -1, F_] + [-1] * (HN - 3), _adj(HN, [(2, 3, 1)]),
                 dict(mol_no_correct=1, mol_n_fragments=1, mol_atoms=1, bonds=[]), None),
    # (i) an asymmetric adjacency: the UPPER triangle (row = the smaller index) holds two triple bonds on C 0, the lower triangle nothing
    "i_triangle": (_pad([C_] * 3, HN), np.triu(_adj(HN, [(0, 1, 3), (0, 2, 3)])),
                   dict(mol_no_correct=0, mol_n_corrections=2, bonds=[(0, 1, 2), (0, 2, 2)], mol_atoms=3), None),
    "i_triangle_lower": (_pad([C_] * 3, HN), np.tril(_adj(HN, [(0, 1, 3), (0, 2, 3)])),
                         dict(mol_no_correct=1, mol_n_corrections=0, mol_n_fragments=3, bonds=[], mol_atoms=1), None),
    # (j) values exactly on the quantiser's bin edges and one float32 below them
    "j_edges": (_pad([C_] * 12, HN), _adj(HN, [(0, 1, 0.5), (2, 3, 1.5), (4, 5, 2.5), (6, 7, BELOW(0.5)), (8, 9, BELOW(1.5)), (10, 11, BELOW(2.5))]),
                dict(mol_n_fragments=7, mol_atoms=2),
                dict(mol_no_correct=1, mol_atoms=12, bonds=[(0, 1, 1), (2, 3, 2), (4, 5, 3), (8, 9, 1), (10, 11, 2)])),
}


def hand_batch():
    names = list(HAND)
    return names, np.stack([HAND[n][1] for n in names]), np.array([HAND[n][0] for n in names], np.int32)


def check_hand(got, largest_fragment):
    """The stated expectations of HAND on a result dict of numpy arrays (either the restatement's or the library's)."""
    names, _, _ = hand_batch()
    for b, name in enumerate(names):
        exp = HAND[name][2 if largest_fragment else 3]
        for key, want in (exp or {}).items():
            if key == "bonds":
                a = np.zeros((HN, HN), np.uint8)
                for i, j, o in want:
                    a[i, j] = a[j, i] = o
                assert np.array_equal(got["mol_adj"][b], a), (name, largest_fragment, got["mol_adj"][b])
            else:
                assert np.array_equal(got[key][b], np.asarray(want)), (name, largest_fragment, key, got[key][b], want)


# ---- random molecule-like batches --------------------------------------------------------------------------------------------------------------
def random_batch(B, N, table, seed, calm=0.4):
    """Raw adj (B, N, N) float32 and labels (B, N) int32.  A `calm` share of the molecules is grown within the neutral valences (nothing to
    correct); the others get bond orders and extra bonds drawn freely, so that corrections, charges and fragments are common.  Values lie
    within 0.4 of their bond order (the quantiser's bins are exercised), the adjacency is symmetric, a few slots hold no atom."""
    rng = np.random.default_rng(seed)
    L = len(table["max_valence"])
    p_lab = np.array([6.0, 3.0, 3.0] + [1.0] * (L - 3))
    p_lab /= p_lab.sum()
    adj = np.zeros((B, N, N), np.float32)
    labels = np.full((B, N), -1, np.int32)
    for b in range(B):
        n = int(rng.integers(1, N + 1))
        slots = list(range(n))
        if n > 2 and rng.random() < 0.3:                                 # holes among the atoms
            for s in rng.choice(n, size=min(2, n - 1), replace=False):
                slots.remove(int(s))
        labels[b, slots] = rng.choice(L, size=len(slots), p=p_lab)
        q = np.zeros((N, N), np.int64)
        if rng.random() < calm:
            room = {s: table["max_valence"][labels[b, s]][0] for s in slots}
            for k, s in enumerate(slots[1:], 1):
                if rng.random() < 0.08:
                    continue                                             # a new fragment
                t = slots[int(rng.integers(0, k))]
                o = min(int(rng.choice([1, 2, 3], p=[0.8, 0.15, 0.05])), room[s], room[t])
                if o:
                    q[s, t] = q[t, s] = o
                    room[s] -= o
                    room[t] -= o
        else:
            for k, s in enumerate(slots[1:], 1):
                if rng.random() < 0.12:
                    continue
                t = slots[int(rng.integers(0, k))]
                q[s, t] = q[t, s] = int(rng.choice([1, 2, 3], p=[0.55, 0.3, 0.15]))
            for _ in range(len(slots) // 3):
                s, t = (int(v) for v in rng.choice(N, size=2))           # (may point at a slot without an atom)
                if s != t:
                    q[s, t] = q[t, s] = int(rng.choice([1, 2, 3], p=[0.6, 0.25, 0.15]))
        noise = np.triu(rng.uniform(-0.4, 0.4, (N, N)), 1)
        adj[b] = (q + noise + noise.T).astype(np.float32)
        adj[b][np.arange(N), np.arange(N)] = rng.uniform(-1, 4, N)       # (the diagonal is never read)
    return adj, labels


def complete_triple(N):
    """The complete graph of triple bonds on N carbons: the longest repair loop (N = 64: 2016 bonds)."""
    return np.full((1, N, N), 3.0, np.float32), np.zeros((1, N), np.int32)


# name -> (maker of (adj, labels), table); B = 1, 5 and 257 leave the last workgroup of the device kernel partly empty
CASES = {
    "random_N9": (lambda: random_batch(257, 9, QM9, 11), QM9),
    "random_N38": (lambda: random_batch(96, 38, ZINC, 12), ZINC),
    "N1": (lambda: random_batch(5, 1, QM9, 13), QM9),
    "N2": (lambda: random_batch(5, 2, QM9, 14, calm=0.2), QM9),
    "N63": (lambda: random_batch(5, 63, ZINC, 15, calm=0.2), ZINC),
    "N64": (lambda: random_batch(5, 64, ZINC, 16, calm=0.2), ZINC),
    "N64_B1": (lambda: random_batch(1, 64, ZINC, 17, calm=0.0), ZINC),
    "complete_triple_N64": (lambda: complete_triple(64), QM9),
    "complete_triple_N7": (lambda: complete_triple(7), QM9),
    "N64_B257": (lambda: random_batch(257, 64, ZINC, 18, calm=0.3), ZINC),
    "held_N9": (lambda: random_batch(64, 9, QM9, 21, calm=1.0), QM9),              # nothing to correct: the held-out side of the evaluate cases
}
RANDOM = ("random_N9", "random_N38")


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "hand":
        _, adj, labels = hand_batch()
        return adj, labels, QM9
    make, table = CASES[name]
    adj, labels = make()
    return adj, labels, table


@functools.lru_cache(maxsize=None)
def reference(name, largest_fragment=True):
    """The restatement's outputs for a case: computed once, shared, never written to."""
    adj, labels, table = inputs(name)
    out = mol_ref.mol_correct(adj, labels, table["max_valence"], table["charge_base"], largest_fragment)
    for v in out.values():
        v.setflags(write=False)
    return out


def check_generator():
    """No random case passes vacuously: by the restatement alone, the random batches hold what the kernel can get wrong."""
    check_hand(reference("hand", True), True)
    check_hand(reference("hand", False), False)
    for name in RANDOM:
        adj, labels, table = inputs(name)
        ref = reference(name)
        B = len(labels)
        charged = [(labels[b][ref["mol_charge"][b] == 1]).tolist() for b in range(B)]
        assert (ref["mol_n_corrections"] >= 3).any(), name
        assert any(N_ in c for c in charged) and any(O_ in c for c in charged), name
        assert (ref["mol_n_fragments"] >= 3).any(), name
        share = ref["mol_no_correct"].mean()
        assert 0.2 <= share <= 0.8, (name, share)
        assert (labels < 0).any() and (ref["mol_atoms"] < (labels >= 0).sum(1)).any(), name      # holes; a fragment was dropped
    assert int(reference("complete_triple_N64")["mol_n_corrections"][0]) > 5000


# ---- running the call ----------------------------------------------------------------------------------------------------------------------------
def run(lib, device, adj, labels, table, largest_fragment=True, ops=None):
    ops = ops or sample_ops(lib, device)
    out = ops.mol_correct(torch.from_numpy(np.ascontiguousarray(adj)).to(device), torch.from_numpy(np.ascontiguousarray(labels)).to(device),
                          max_valence=table["max_valence"], charge_base=table["charge_base"], largest_fragment=largest_fragment)
    assert tuple(out) == OUTPUTS
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal(got, want, what):
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = np.nonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(1))[0]
        assert bad.size == 0, f"{what}: {k} differs from the restatement for molecules {bad[:8].tolist()} ({bad.size} in all)"


def check_properties(got, table, largest_fragment, what):
    """What holds for every output: no over-valent atom, a symmetric mol_adj with a zero diagonal and no bond at a slot without an atom,
    counters that agree with the tensors, and -- with the selection -- kept atoms that form one component."""
    a, lab, chg = got["mol_adj"].astype(np.int64), got["mol_labels"], got["mol_charge"]
    B, N = lab.shape
    on = lab >= 0
    assert np.array_equal(a, a.transpose(0, 2, 1)) and not a[:, np.arange(N), np.arange(N)].any(), what
    assert a.max(initial=0) <= 3 and not (a.sum(2)[~on]).any() and not chg[~on].any() and set(np.unique(chg)) <= {0, 1}, what
    mv = np.asarray(table["max_valence"])
    limit = mv[np.where(on, lab, 0), chg.astype(np.int64)]
    assert not ((a.sum(2) > limit) & on).any(), f"{what}: an over-valent atom remains"
    assert np.array_equal(got["mol_atoms"], on.sum(1)), what
    assert ((got["mol_n_corrections"] == 0) | (got["mol_no_correct"] == 0)).all(), what
    reach = (a > 0) | (np.eye(N, dtype=bool)[None] & on[:, :, None])
    for _ in range(max(1, int(np.ceil(np.log2(max(N, 2)))))):
        reach = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
    ncomp = np.array([len({row.tobytes() for row in reach[b][on[b]]}) for b in range(B)])
    if largest_fragment:
        assert (ncomp <= 1).all() and ((got["mol_n_fragments"] >= 1) == (got["mol_atoms"] >= 1)).all(), f"{what}: the kept atoms are not one component"
    else:
        assert np.array_equal(ncomp, got["mol_n_fragments"]), what


def check_fixed_point(lib, device, got, table, largest_fragment, what):
    """mol_correct of its own output, the charges discarded, changes nothing -- for the molecules none of whose kept atoms was charged (a
    charged atom's bonds exceed its neutral maximum by design)."""
    again = run(lib, device, got["mol_adj"].astype(np.float32), got["mol_labels"], table, largest_fragment)
    calm = ~(got["mol_charge"] != 0).any(1)
    assert calm.any() or len(calm) == 1, what
    for k in ("mol_adj", "mol_labels", "mol_charge", "mol_atoms"):
        assert np.array_equal(again[k][calm], got[k][calm]), (what, k)
    assert (again["mol_no_correct"][calm] == 1).all() and not again["mol_n_corrections"][calm].any(), what
    if largest_fragment:
        assert (again["mol_n_fragments"][calm] == (got["mol_atoms"][calm] > 0)).all(), what


def case_exact(lib, device, name, largest_fragment=True, properties=True):
    adj, labels, table = inputs(name)
    got = run(lib, device, adj, labels, table, largest_fragment)
    assert_equal(got, reference(name, largest_fragment), f"{name}, largest_fragment={largest_fragment}")
    if name == "hand":
        check_hand(got, largest_fragment)
    if properties:
        check_properties(got, table, largest_fragment, name)
        check_fixed_point(lib, device, got, table, largest_fragment, name)


# ---- the call as a pure function of its arguments (in the style of tests/purity_cases.py) ---------------------------------------------------------
GUARD = 4096


class _Torch:
    """torch, with `empty` carving from the middle of tensors filled with one byte: GUARD bytes on either side lie inside the allocation."""

    def __init__(self, fill):
        self.fill, self.items = fill, []

    def __getattr__(self, k):
        return getattr(torch, k)

    def empty(self, shape, dtype=torch.float32, device=None):
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        big = torch.full((n + (-n % 8) + 2 * GUARD,), self.fill, dtype=torch.uint8, device=device)
        self.items.append((big, n))
        return big[GUARD:GUARD + n].view(dtype).view(tuple(shape))

    def check(self, what):
        assert self.items, what
        for big, n in self.items:
            assert bool((big[:GUARD] == self.fill).all() & (big[GUARD + n:] == self.fill).all()), f"{what}: a guard around an output of {n} bytes was written"


@contextlib.contextmanager
def filled_outputs(fill):
    t = _Torch(fill)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(samples_mod, "torch", t)
        yield t


def case_pure(lib, device, name="random_N9"):
    """Inputs untouched; two calls bit-identical whatever the outputs held on entry (0xA5, then 0x5A: a byte the call leaves unwritten
    differs between the two); nothing written outside the outputs."""
    adj, labels, table = inputs(name)
    ops = sample_ops(lib, device)
    ta, tl = torch.from_numpy(adj.copy()).to(device), torch.from_numpy(labels.copy()).to(device)
    mv, cb = np.array(table["max_valence"], np.int32), np.array(table["charge_base"], np.int32)
    res = []
    for fill in (0xA5, 0x5A):
        with filled_outputs(fill) as g:
            out = ops.mol_correct(ta, tl, max_valence=mv, charge_base=cb)
            if device != "cpu":
                torch.cuda.synchronize()
            g.check(f"{name}, fill {fill:#x}")
            assert len(g.items) == len(OUTPUTS)
        res.append({k: v.cpu().numpy().copy() for k, v in out.items()})
    for k in OUTPUTS:
        assert np.array_equal(res[0][k], res[1][k]), f"{name}: {k} depends on what the output held on entry"
    assert_equal(res[0], reference(name), name)
    assert np.array_equal(ta.cpu().numpy(), adj) and np.array_equal(tl.cpu().numpy(), labels), "an input was written"
    assert np.array_equal(mv, np.array(table["max_valence"], np.int32)) and np.array_equal(cb, np.array(table["charge_base"], np.int32))


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------------------
def case_invalid(lib, device):
    ops = sample_ops(lib, device)
    z = lambda B, N: torch.zeros((B, N, N), dtype=torch.float32, device=device)
    lab = lambda B, N, v=0: torch.full((B, N), v, dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match=r"N = 65 outside 1\.\.64"):
        ops.mol_correct(z(1, 65), lab(1, 65))
    with pytest.raises(ValueError, match=r"L = 17 outside 1\.\.16"):
        ops.mol_correct(z(1, 4), lab(1, 4), max_valence=[[4, 4]] * 17, charge_base=[0] * 17)
    with pytest.raises(ValueError, match=r"L = 0 outside 1\.\.16"):
        ops.mol_correct(z(1, 4), lab(1, 4), max_valence=np.zeros((0, 2), np.int32), charge_base=np.zeros((0,), np.int32))
    with pytest.raises(ValueError, match=r"a label is >= L = 4"):
        ops.mol_correct(z(2, 4), torch.tensor([[0, 1, 2, 3], [0, -1, 4, 0]], dtype=torch.int32, device=device))
    assert ops.mol_correct(z(2, 4), torch.tensor([[0, 1, 2, 3], [0, -1, 8, 0]], dtype=torch.int32, device=device), dataset="ZINC250k")["mol_atoms"].tolist() == [1, 1]
    with pytest.raises(ValueError, match=r"max_valence of label 1 outside 0\.\.255"):
        ops.mol_correct(z(1, 4), lab(1, 4), max_valence=[[4, 4], [-1, 4]], charge_base=[0, 0])
    with pytest.raises(ValueError, match="dataset must be one of"):
        ops.mol_correct(z(1, 4), lab(1, 4), dataset="ENZYMES")
    with pytest.raises(ValueError, match="labels must be integer"):
        ops.mol_correct(z(1, 4), torch.zeros((1, 4), device=device))
    with pytest.raises(ValueError, match=r"max_valence must be \(L, 2\)"):
        ops.mol_correct(z(1, 4), lab(1, 4), max_valence=[4, 3], charge_base=[0, 0])
    # the status codes of the C call itself
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    i32p = C.POINTER(C.c_int32)
    mv, cb = np.array(QM9["max_valence"], np.int32), np.array(QM9["charge_base"], np.int32)

    def call(B, N, L, labels, mv=mv, cb=cb):
        res = {k: torch.zeros(max(B, 1) * max(N, 1) * max(N, 1), dtype=torch.int32, device=device) for k in OUTPUTS}
        out = _lib.MolOut(*[p(res[k]) for k in OUTPUTS])
        return lib.ccsd_mol_correct(C.byref(_lib.MolDims(B, N, L, 1)), p(z(max(B, 1), max(N, 1))), p(labels), mv.ctypes.data_as(i32p),
                                    cb.ctypes.data_as(i32p), C.byref(out), ops._stream())

    assert call(1, 4, 4, lab(1, 4)) == _lib.OK
    assert call(0, 4, 4, lab(1, 4)) == _lib.OK                                                   # B = 0: a no-op
    assert call(1, 65, 4, lab(1, 65)) == _lib.ERR_INVALID
    assert call(1, 0, 4, lab(1, 1)) == _lib.ERR_INVALID
    assert call(1, 4, 0, lab(1, 4)) == _lib.ERR_INVALID and call(1, 4, 17, lab(1, 4)) == _lib.ERR_INVALID
    assert call(1, 4, 4, lab(1, 4, 4)) == _lib.ERR_INVALID and b"a label is >= L = 4" in lib.ccsd_last_error()
    assert call(3, 4, 2, lab(3, 4, 1)) == _lib.OK and call(3, 4, 2, lab(3, 4, 2)) == _lib.ERR_INVALID
    assert call(1, 4, 4, None) == _lib.ERR_INVALID and call(-1, 4, 4, lab(1, 4)) == _lib.ERR_INVALID


# ---- Sampler.molecules / Sampler.evaluate(correct=True) through fake finished results -----------------------------------------------------------
MOL_CFG = {"is_cc": False, "data": {"data": "QM9", "dir": "./data", "max_node_num": 9, "min_edge_val": 1, "max_edge_val": 3}, "ckpt": "gdss_qm9"}


def fake_result(name="random_N9", rows=slice(None)):
    """What sample() returns of a molecule run, as far as molecules() / evaluate() read it: raw adj and raw x whose channel above 0.5 is the label."""
    adj, labels, _ = inputs(name)
    adj, labels = adj[rows], labels[rows]
    x = np.full(labels.shape + (4,), 0.1, np.float32)
    b, i = np.nonzero(labels >= 0)
    x[b, i, labels[b, i]] = 0.9
    return {"adj": torch.from_numpy(adj.copy()), "x": torch.from_numpy(x)}


def make_sampler(lib, cfg=MOL_CFG):
    from ccsd_amd import sampler as S

    s = S.get_sampler_from_config(cfg)
    s.extra = dict(lib=lib)
    return s


def case_sampler(lib, device):
    s = make_sampler(lib)
    assert s.is_mol and str(s.device0).startswith(str(device)[:3])
    res = fake_result()
    keys = set(res)
    mols = s.molecules(res)
    ref = reference("random_N9")
    assert set(mols) == set(OUTPUTS) | {"validity_wo_correction"}
    assert_equal({k: mols[k].cpu().numpy() for k in OUTPUTS}, ref, "Sampler.molecules")
    assert mols["validity_wo_correction"] == float(ref["mol_no_correct"].sum()) / len(ref["mol_no_correct"])
    assert_equal({k: v.cpu().numpy() for k, v in s.molecules(res, largest_fragment=False).items() if k in OUTPUTS}, reference("random_N9", False), "molecules, every fragment")
    # the held-out side: molecules that need no correction, left as given
    held = fake_result("held_N9")
    assert reference("held_N9")["mol_no_correct"].all()
    base = s.evaluate(res, held, nspdk=True)
    got = s.evaluate(res, held, nspdk=True, correct=True)
    assert set(base) == {"degree", "cluster", "nspdk"} and set(got) == set(base) | {"validity_wo_correction"}
    assert got["validity_wo_correction"] == mols["validity_wo_correction"]
    # ... equals the manual composition mol_correct -> describe -> eval_torch_batch
    kw = dict(device=s.device0, lib=lib)
    kept = mols["mol_atoms"] > 0
    pred_desc = ev.describe(mols["mol_adj"][kept].to(torch.float32), mol=True, nspdk=True, nspdk_labels=mols["mol_labels"][kept], **kw)
    held_desc = ev.describe(held["adj"], held["x"], mol=True, nspdk=True, **kw)
    want = ev.eval_torch_batch(held_desc, pred_desc, ["degree", "cluster", "nspdk"], mol=True, nspdk=True, **kw)
    assert {k: got[k] for k in want} == want, (got, want)
    # ... and without `correct` nothing changed: the composition the method has always been, on the samples as sampled
    raw_desc = ev.describe(res["adj"], res["x"], mol=True, nspdk=True, **kw)
    assert base == ev.eval_torch_batch(held_desc, raw_desc, ["degree", "cluster", "nspdk"], mol=True, nspdk=True, **kw)
    assert base["nspdk"] != got["nspdk"] and base["degree"] != got["degree"]
    assert set(res) == keys
    # a molecule without an atom is left out of the predicted side
    few = fake_result("hand")
    got_few = s.evaluate(few, held, nspdk=True, correct=True)
    m = s.molecules(few)
    k2 = m["mol_atoms"] > 0
    assert int((~k2).sum()) == 1
    d2 = ev.describe(m["mol_adj"][k2].to(torch.float32), mol=True, nspdk=True, nspdk_labels=m["mol_labels"][k2], **kw)
    want_few = ev.eval_torch_batch(held_desc, d2, ["degree", "cluster", "nspdk"], mol=True, nspdk=True, **kw)
    assert {k: got_few[k] for k in want_few} == want_few and got_few["validity_wo_correction"] == m["validity_wo_correction"]
    # complexes: rank1_distrib from the corrected bonds
    scc = make_sampler(lib, dict(MOL_CFG, is_cc=True, data=dict(MOL_CFG["data"], d_min=3, d_max=9)))
    cc = scc.evaluate(res, held, correct=True)
    assert set(cc) == {"degree", "cluster", "rank1_distrib", "validity_wo_correction"}
    wk = {"min_edge_val": 1, "max_edge_val": 3}
    pred_cc = dict(pred_desc, n_nodes=mols["mol_atoms"][kept])
    assert cc["rank1_distrib"] == ev.eval_CC_batch(held_desc, pred_cc, wk, ["rank1_distrib"], mol=True, **kw)["rank1_distrib"]
    # refusals
    for bad in (dict(MOL_CFG, data={"data": "community_small", "dir": "./data"}),):
        g = make_sampler(lib, bad)
        with pytest.raises(ValueError, match="molecule samplers"):
            g.molecules(res)
        with pytest.raises(ValueError, match="correct=True"):
            g.evaluate(res, held["adj"], correct=True)
    with pytest.raises(NotImplementedError, match="lift"):
        s.evaluate(res, held, lift=True, correct=True)
