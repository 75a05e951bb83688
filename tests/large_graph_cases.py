"""Cases of the tiled graph-network route (graph-only plans above 64 nodes, ccsd_amd/csrc/ccsd_k_lg.h), shared by the CPU suite
(host emulation, tests/test_large_graph.py) and the GPU suite (tests/test_gpu_large_graph.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from ccsd_amd import _lib
from ccsd_amd.engine import PCEngine
from oracle import ccsd_oracle as O
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np, load_golden, make_flags, rng_matches

# the two shipped generic-graph checkpoints above 64 nodes
LARGE = {"gdss_enzymes": 125, "gdss_grid": 361}


def resized(name, N, seed=None, noise=0.05):
    """(meta, weights) of a graph-only checkpoint at another node count (no ScoreNetworkX / ScoreNetworkA weight depends on N);
    with `seed`, every weight is perturbed by noise * N(0, 1) (a random-weight network of the same architecture)."""
    meta, parts = load_ckpt_np(name)
    meta = dict(meta, params_adj=dict(meta["params_adj"], max_node_num=N))
    meta["config"] = dict(meta["config"], data=dict(meta["config"]["data"], max_node_num=N))
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        parts = {p: {k: (v.detach() + noise * torch.randn(v.shape, generator=g)).requires_grad_(True) for k, v in d.items()}
                 for p, d in parts.items()}
    return meta, parts


def engine(meta, parts, lib, device, **kw):
    N, F = meta["params_adj"]["max_node_num"], meta["params_x"]["max_feat_num"]
    return PCEngine(meta["params_x"], parts["x"], meta["params_adj"], parts["adj"], None, None, N=N, F=F, is_cc=False, d_min=0,
                    d_max=0, device=device, lib=lib, **kw)


def case_forward_vs_oracle_src(meta, parts, lib, device, counts, what, seed=11, expect_lg=1, batch_hint=0, oracle=None,
                                scales=(("unit", 1.0), ("small", 0.3))):
    """Both networks' forward (raw nets and the score scaling at t = 0.5) on masked random inputs against the oracle.  `expect_lg`
    None leaves the route to the planner; `batch_hint` is the plan's (it picks k_xa's LDS budget); `oracle` is a dict that keeps
    the oracle's outputs for a later call on the same networks, inputs and seed (another plan of theirs).  Returns the plan's
    (large_graph, xa_variant, xa_lds_bytes)."""
    N, F = meta["params_adj"]["max_node_num"], meta["params_x"]["max_feat_num"]
    eng = engine(meta, parts, lib, device, batch_hint=batch_hint)
    route = tuple(eng.query(q) for q in ("large_graph", "xa_variant", "xa_lds_bytes"))
    assert expect_lg is None or route[0] == expect_lg
    flags = make_flags(len(counts), N, counts)
    dv = lambda t: t.to(device)
    for tag, scale in scales:
        x, adj, _ = pc.masked_state(seed, len(counts), N, F, False, 0, 0, flags, scale)
        for t, p in enumerate(["x", "adj"]):
            want = None if oracle is None else oracle.get((tag, p))
            if want is None:
                with torch.no_grad():
                    want = O.run_network(meta[f"params_{p}"], parts[p], x, adj, None, flags)
                if oracle is not None:
                    oracle[(tag, p)] = want
            got = eng.score(t, dv(x), dv(adj), None, dv(flags))
            pc.assert_close(got, want, f"{what} {tag} net_{p}")
            got2 = eng.score(t, dv(x), dv(adj), None, dv(flags), 0.25)
            pc.assert_close(got2, 0.25 * want, f"{what} {tag} 0.25 * net_{p}")
        # masks of the adj score just computed: zero outside the flags, zero diagonal
        a = got.cpu()
        fm = flags[:, :, None] * flags[:, None, :]
        assert torch.all(a[fm == 0] == 0) and torch.all(torch.diagonal(a, dim1=1, dim2=2) == 0)
    return route


def case_forced_vs_xa(name, lib, device, B, counts, seed=4, monkeypatch=None):
    """CCSD_LARGE_GRAPH=1 (read at plan creation) routes a plan k_xa serves through the tiled kernels: same forward within
    assert_close (the summation orders differ, so not bit for bit)."""
    meta, parts = load_ckpt_np(name)
    N, F = meta["params_adj"]["max_node_num"], meta["params_x"]["max_feat_num"]
    flags = make_flags(B, N, counts)
    x, adj, _ = pc.masked_state(seed, B, N, F, False, 0, 0, flags)
    dv = lambda t: t.to(device)
    monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)
    ref = engine(meta, parts, lib, device)
    assert ref.query("large_graph") == 0
    monkeypatch.setenv("CCSD_LARGE_GRAPH", "1")
    lg = engine(meta, parts, lib, device)
    monkeypatch.delenv("CCSD_LARGE_GRAPH")
    assert lg.query("large_graph") == 1
    for t, p in enumerate(["x", "adj"]):
        want = ref.score(t, dv(x), dv(adj), None, dv(flags)).cpu()
        got = lg.score(t, dv(x), dv(adj), None, dv(flags))
        pc.assert_close(got, want, f"{name} CCSD_LARGE_GRAPH=1 vs k_xa net_{p}")


def case_sampler_vs_golden(gname, case, lib, device):
    """G5 on the reference's own torch RNG (every draw from torch's CPU generator; case_pc_sampler_identical_seed for outputs that may be
    stored as summaries): the sampled state, the step count, the trajectory length and its last adjacency against the reference's at
    RTOL -- summarised arrays through their seeded subsample, and their row sums within the bound the element-wise tolerance implies
    (|sum(got - ref)| <= N * RTOL * scale) --; the quantised adjacency bit for bit except where the reference's value lies within that
    tolerance of the threshold (the fixtures' min_thr_dist: 6e-6 for ENZYMES, which no fp32 reordering can be held to)."""
    g = load_golden(f"g5_{gname}.npz")
    assert rng_matches(g)
    fn, models, flags, names = pc.sampler_from_golden(g, gname, case, lib, device, keep_traj=True)
    torch.manual_seed(int(g["seed"]))
    res = fn(*models, flags.to(device))

    def check(v, key, what):
        v = v.detach().cpu()
        if key in g.files:
            pc.assert_close(v, g[key], what)
            return v.reshape(-1), torch.from_numpy(g[key]).reshape(-1)
        idx = torch.from_numpy(g[f"{key}/idx"])
        ref = torch.from_numpy(g[f"{key}/val"])
        pc.assert_close(v.reshape(-1)[idx], ref, f"{what} (subsample)")
        rs, rref = v.double().sum(-1), torch.from_numpy(g[f"{key}/rowsum"])
        bound = v.shape[-1] * pc.RTOL * max(ref.abs().max().item(), 1e-6)
        assert (rs - rref).abs().max().item() <= bound, f"{what}: row sums differ by more than N * RTOL * scale"
        return v.reshape(-1)[idx], ref

    got_adj, ref_adj = None, None
    for p, v in zip(names, res):
        got, ref = check(v, f"{case}/{p}", f"{gname} {case} {p}")
        if p == "adj":
            got_adj, ref_adj = got, ref
    assert int(res[len(names)]) == int(g[f"{case}/nfe"])
    assert len(res[-1]) == int(g[f"{case}/traj_len"])
    check(res[-1][-1][1], f"{case}/traj_last_adj", "diff_traj[-1] adj")
    # quantised adjacency (graph_utils.quantize: > 0.5) on the same entries
    key = f"{case}/quantize_adj"
    qref = torch.from_numpy(g[key] if key in g.files else g[f"{key}/val"]).reshape(-1)
    tol = pc.RTOL * max(ref_adj.abs().max().item(), 1.0)
    safe = (ref_adj.double() - 0.5).abs() > tol
    assert safe.double().mean().item() > 0.999, "too many entries sit on the threshold"
    assert torch.equal((got_adj > 0.5).to(qref.dtype)[safe], qref[safe]), "quantize_adj differs away from the threshold"


def graph_pickle(path, sizes):
    import pickle

    import networkx as nx

    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump([nx.path_graph(n) for n in sizes], f)


def enzymes_folder(tmp_path, num_scales=None, batch_size=None):
    """A checkout-like folder: the gdss_enzymes checkpoint in the neutral format under checkpoints/ENZYMES/ (optionally with a short SDE
    and another training batch size, which sets the sampling batch)."""
    from tests.helpers import GOLDEN_CKPT

    with open(os.path.join(GOLDEN_CKPT, "gdss_enzymes.json")) as f:
        meta = json.load(f)
    arrays = {}
    for fname in meta.pop("files"):
        z = np.load(os.path.join(GOLDEN_CKPT, fname))
        arrays.update({k: z[k] for k in z.files})
    if batch_size:
        meta["config"]["data"]["batch_size"] = batch_size
    if num_scales:
        for p in ("x", "adj"):
            meta["config"]["sde"][p]["num_scales"] = num_scales
    d = tmp_path / "checkpoints" / "ENZYMES"
    os.makedirs(d, exist_ok=True)
    np.savez(d / "gdss_enzymes.npz", **arrays)
    with open(d / "gdss_enzymes.json", "w") as f:
        json.dump(meta, f)


ENZYMES_YAML = {
    "data": {"data": "ENZYMES", "dir": "./data"},
    "ckpt": "gdss_enzymes",
    "sampler": {"predictor": "S4", "corrector": "None", "snr": 0.15, "scale_eps": 0.7, "n_steps": 1},
    "sample": {"use_ema": False, "noise_removal": True, "probability_flow": False, "eps": 1.0e-4, "seed": 42},
}



def case_enzymes_yaml_run(lib, tmp_path, num_scales=5):
    """CCSD(type="sample", config=<yaml with ckpt gdss_enzymes>, folder=<checkout>).run() with a short SDE: node counts from the dataset
    pickle, the shipped sampling batch (64), the tiled route at N = 125.  The quantised adjacency is symmetric, has a zero diagonal and is
    zero outside the flags."""
    import yaml

    from ccsd_amd.diffusion import CCSD

    sizes = [int(v) for v in np.random.RandomState(3).randint(2, 126, 587)]
    graph_pickle(str(tmp_path / "data" / "ENZYMES.pkl"), sizes)
    enzymes_folder(tmp_path, num_scales=num_scales)
    os.makedirs(tmp_path / "config", exist_ok=True)
    with open(tmp_path / "config" / "sample_enzymes.yaml", "w") as f:
        yaml.safe_dump(ENZYMES_YAML, f)
    c = CCSD("sample", "sample_enzymes", folder=str(tmp_path), seed=42)
    out = c.run(gpus=1, rounds=1)
    sm = c.sampler
    assert sm.n_test == 117 and math.ceil(sm.n_test / sm.configt.data.batch_size) == 2       # ENZYMES: two sampling rounds
    a, fl = out["adj_int"].cpu(), out["flags"].cpu()
    assert a.shape == (64, 125, 125) and out["x"].shape == (64, 125, 10)
    assert torch.equal(a, a.transpose(1, 2)) and not torch.diagonal(a, dim1=1, dim2=2).any()
    assert not (a * (1 - fl[:, :, None] * fl[:, None, :])).any()
    assert set(fl.sum(1).long().tolist()) <= set(sizes[117:])
    return out


def case_planner_rejects(lib, device):
    """Above 64 nodes only graph-only plans of the route's shape plan; each rejection names its reason."""
    with pytest.raises(NotImplementedError, match="N <= 512"):
        engine(*resized("gdss_community_small", 513), lib, device)
    dummy = dict(nhid=4, num_layers=2, num_linears=2, c_init=2, c_hid=4, c_final=4, adim=4, num_heads=2, use_bn=False)
    a_gcn = dict(dummy, model_type="ScoreNetworkA", conv="GCN", max_feat_num=4, max_node_num=80)
    with pytest.raises(NotImplementedError, match="N <= 64"):       # combinatorial complexes
        PCEngine(None, None, None, None, None, None, N=80, F=4, is_cc=True, d_min=1, d_max=2, device=device, lib=lib)
    with pytest.raises(NotImplementedError, match="MLP"):            # conv = "MLP"
        PCEngine(None, None, dict(a_gcn, conv="MLP"), None, None, None, N=80, F=4, is_cc=False, device=device, lib=lib)
    gmh = dict(dummy, model_type="ScoreNetworkX_GMH", depth=2, conv="GCN", max_feat_num=4)
    with pytest.raises(NotImplementedError, match="GMH"):            # ScoreNetworkX_GMH
        PCEngine(gmh, None, a_gcn, None, None, None, N=80, F=4, is_cc=False, device=device, lib=lib)
    # ... while the same GCN networks plan at N = 80 and N = 512, and a graph of 64 nodes stays on k_xa
    for n, lg in ((80, 1), (512, 1), (64, 0)):
        eng = PCEngine(None, None, dict(a_gcn, max_node_num=n), None, None, None, N=n, F=4, is_cc=False, device=device, lib=lib)
        assert eng.query("large_graph") == lg, n


