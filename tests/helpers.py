"""Shared helpers for the test-suite (fixtures are data only: tests/golden/*.npz)."""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CKPT = os.path.join(ROOT, "ccsd_amd", "checkpoints")
# shipped checkpoints the package does not carry: converted weights kept as test fixtures only
GOLDEN_CKPT = os.path.join(GOLDEN, "ckpt")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def load_ckpt_np(name):
    """Neutral-format checkpoint -> (meta dict, {part: {key: torch tensor}}): ccsd_amd/checkpoints/ first, then
    tests/golden/ckpt/."""
    d = CKPT if os.path.exists(os.path.join(CKPT, name + ".json")) else GOLDEN_CKPT
    with open(os.path.join(d, name + ".json")) as f:
        meta = json.load(f)
    z = {}
    for fname in meta.get("files", [name + ".npz"]):          # fixtures: the state dict split into files of at most 1 MiB
        f = np.load(os.path.join(d, fname))
        z.update({k: f[k] for k in f.files})
    parts = {}
    for k in z:
        part, key = k.split("/", 1)
        # requires_grad mirrors nn.Parameter: ATen's linear() picks the same (non-XNNPACK) CPU kernel as
        # the reference's modules do, which makes the oracle bit-identical to it under torch.no_grad()
        parts.setdefault(part, {})[key] = torch.from_numpy(z[k]).requires_grad_(True)
    return meta, parts


def sample_ops(lib, dev):
    """The plan-free operations on finished samples (quantize, finish, cluster_hist, mmd, the spectra) over `lib` on `dev`."""
    from ccsd_amd.samples import SampleOps

    return SampleOps(dev, lib)


def rng_matches(g):
    """The goldens regenerate inputs/noise from torch's CPU generator; check that this torch
    build reproduces the stream the fixtures were made with."""
    torch.manual_seed(int(g["seed"]))
    return np.array_equal(torch.randn(8).numpy(), g["rng_probe"])


def make_flags(B, N, counts):
    f = torch.zeros(B, N)
    for b in range(B):
        f[b, : counts[b % len(counts)]] = 1.0
    return f


def make_flags_holes(B, N, counts, seed):
    """make_flags' counts (cycled over the batch) with the live nodes at seeded random positions instead of a prefix.  Every batch
    holds, and the function asserts it: a sample with node 0 off and node N - 1 on; another with node N - 1 off; a full sample;
    samples of 0, 1 and 2 nodes, the live ones not a prefix (with d_min = 3 no cell fits them).  `counts` must provide them: N, 0, 1, 2
    and, for the two partial samples, either two more counts in 1 .. N - 1 or the samples of 2 and 1 nodes themselves."""
    assert N >= 4 and B >= 4, (B, N)
    cs = [int(counts[b % len(counts)]) for b in range(B)]
    g = torch.Generator().manual_seed(seed)
    partial = sorted((b for b in range(B) if 0 < cs[b] < N), key=lambda b: (-cs[b], b))
    assert len(partial) >= 2, f"counts {cs}: no two partial samples"
    first_off, last_off = partial[0], partial[1]          # the two fullest partial samples take the two edge patterns
    f = torch.zeros(B, N)
    for b in range(B):
        c = cs[b]
        lo, hi = (1, N - 1) if b == first_off else (0, N - 1) if b == last_off else (0, N)      # nodes the draw may switch on
        fixed = [N - 1] if b == first_off else []
        for _ in range(1000):
            pool = torch.arange(lo, hi)[torch.randperm(hi - lo, generator=g)]
            on = sorted(fixed + pool[: c - len(fixed)].tolist())
            if c in (0, N) or on != list(range(c)):        # (never a prefix)
                break
        else:
            raise AssertionError(f"no pattern with holes for {c} of {N} nodes")
        f[b, on] = 1.0
    assert f.sum(1).tolist() == [float(c) for c in cs]
    have = set(cs)
    assert {0, 1, 2, N} <= have, f"counts {cs} lack one of 0, 1, 2, {N}"
    assert f[first_off, 0] == 0 and f[first_off, N - 1] == 1 and f[last_off, N - 1] == 0
    for b in range(B):
        assert cs[b] in (0, N) or f[b, : cs[b]].sum() < cs[b], f"sample {b} is a prefix"
    return f


STATE_KINDS = ("masked", "unmasked", "diag")


def make_state(kind, seed, B, N, Fd, is_cc, d_min, d_max, flags, scale=1.0):
    """(x, adj, rank2 or None) of one input class, from the draws of parity_cases.masked_state (same seed, same order):
    "masked"    parity_cases.masked_state itself;
    "unmasked"  the same draws without the masks -- the rows of switched-off nodes carry values; adj symmetric with a zero diagonal;
    "diag"      the masked state plus a random diagonal on the adjacency of the live nodes (drawn after everything else)."""
    from oracle import ccsd_oracle as O
    from tests.parity_cases import masked_state

    assert kind in STATE_KINDS, kind
    if kind == "masked":
        return masked_state(seed, B, N, Fd, is_cc, d_min, d_max, flags, scale)
    torch.manual_seed(seed)
    x = torch.randn(B, N, Fd) * scale
    a = torch.randn(B, N, N).triu(1) * scale
    adj = a + a.transpose(-1, -2)
    rank2 = torch.randn(B, *O.get_rank2_dim(N, d_min, d_max)) * scale if is_cc else None
    if kind == "diag":
        x, adj = O.mask_x(x, flags), O.mask_adjs(adj, flags)
        adj = adj + torch.diag_embed(torch.randn(B, N) * scale * flags)
        if is_cc:
            rank2 = O.mask_rank2(rank2, N, d_min, d_max, flags)
    return x, adj, rank2


def parse_case(case):
    """Name of a g5 sampler case -> (num_scales override or None, number of steps run or None = all): "k10" = a 10-scale SDE run to
    the end, "n1000_first3" = the checkpoint's 1000 scales, first 3 steps, "n1000" = the checkpoint's 1000 scales from the prior to
    the last step."""
    if case.startswith("k"):
        return int(case[1:]), None
    if "first" in case:
        return None, int(case.split("first")[1])
    return None, None
