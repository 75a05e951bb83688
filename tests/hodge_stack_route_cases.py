"""Cases of the tiled graph-network route for ScoreNetworkA_CC stacks of two or more HodgeAdjAttentionLayers (k_lg_hd_*,
ccsd_amd/csrc/ccsd_k_lg.h), shared by the CPU suite (host emulation, tests/test_hodge_stack_route.py) and the GPU suite
(tests/test_gpu_hodge_stack_route.py).  Every comparison takes parity_cases.assert_close at its default tolerance.

Where no fixture has a tensor of the network under test (layer-1 weights, a wider final MLP, K rows beyond the fixture's), arch_at
builds a same-architecture network: every tensor the fixture has (its K-row weights cut to K(N)), the rest drawn from a seeded
torch.Generator at nn.Linear's default scale.  The oracle is the specification for such networks."""
import json
import math
import os

import numpy as np
import pytest
import torch

from ccsd_amd import loader, plan
from ccsd_amd.engine import PCEngine
from oracle import ccsd_oracle as O
from tests import cc_large_graph_cases as cc
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np, load_golden, make_flags, rng_matches

NAMES = cc.NAMES
GRID = cc.GRID                       # grid_small_CC: c_hid_h 2, d 3..3, num_linears_h 1 (one hodge layer in the fixture)
ENZ = "ccsd_enzymes_small_CC"        # c_hid_h 4, d 3..4, num_linears_h 2: tiled rank-2 family, a true-MLP mlp_value
QM9 = "ccsd_qm9_CC"                  # c_hid_h 4, num_linears_h 1: fused rank-2 family, k_r2 hands the raw P_1 over
CS = "ccsd_community_small_CC"
# qm9_CC.yaml's / enzymes_small_CC.yaml's hodge settings
QM9_HODGE = dict(num_layers_h=2, c_hid_h=4, c_final_h=2, adim_h=4, nhid_h=4, num_heads_h=2, num_linears_h=1)
KAT_LAYERS = ["L3_n5", "L4_n6", "L3_n9"]
KAT_GENERAL = ["G3_n5", "G4_n6", "G3_n9", "G3_n12", "A3_n12", "A5_n5", "G6_n6"]
_cache = {}


def _drawn(key, shape, shapes, gen):
    """U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)): nn.Linear's default for weight [out][in] and bias; the graph / hodge convolution weights
    are [in][out], and a bias takes the fan-in of its weight."""
    wkey = key[: -len("bias")] + "weight" if key.endswith("bias") else key
    ws = shapes.get(wkey, shape)
    fan_in = ws[0] if ("ccnn_" in wkey or "gnn_" in wkey) else ws[-1]
    bound = 1.0 / math.sqrt(max(fan_in, 1))
    return (torch.rand(*shape, generator=gen) * 2 - 1) * bound


def arch_at(ckpt, N, seed=101, **adj_over):
    """(meta, parts) of the checkpoint's architecture at node count N with the A-network's parameters overridden by adj_over."""
    key = (ckpt, N, seed, tuple(sorted(adj_over.items())))
    if key not in _cache:
        meta, parts = load_ckpt_np(ckpt)
        at = lambda p: dict(p, max_node_num=N) if "max_node_num" in p else dict(p)
        pa = dict(at(meta["params_adj"]), **adj_over)
        meta = dict(meta, params_x=at(meta["params_x"]), params_adj=pa, params_rank2=at(meta["params_rank2"]))
        meta["config"] = dict(meta["config"], data=dict(meta["config"]["data"], max_node_num=N))
        gen = torch.Generator().manual_seed(seed)
        shapes = dict(plan.state_dict_shapes(pa))
        adj = {}
        for k, shape in shapes.items():
            have = parts["adj"].get(k)
            if have is not None and tuple(have.shape) == tuple(shape):
                t = have.detach().clone()
            elif have is not None and have.dim() == 2 and "ccnn_" in k and tuple(have.shape[1:]) == tuple(shape[1:]):
                t = have.detach()[: shape[0]].clone()          # K rows: the fixture's first K(N), drawn rows behind them
                if t.shape[0] < shape[0]:
                    t = torch.cat([t, _drawn(k, (shape[0] - t.shape[0], *shape[1:]), shapes, gen)], dim=0)
            else:
                t = _drawn(k, shape, shapes, gen)
            adj[k] = t.requires_grad_(True)
        _cache[key] = (meta, dict(parts, adj=adj))
    return _cache[key]


def forced(monkeypatch, on=True):
    if on:
        monkeypatch.setenv("CCSD_LARGE_GRAPH", "2")
    else:
        monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)


# ---- 1. forced route against k_xa, the oracle and the reference goldens
def case_forced_vs_xa(name, lib, device, counts, monkeypatch):
    """CCSD_LARGE_GRAPH=2 on a shipped two-layer checkpoint k_xa serves: large_graph == 1 with the rank-2 family unchanged; x, adj and
    rank2 against the oracle and the un-forced k_xa engine; the adj score zero on the diagonal and outside the flags."""
    cc.case_forced_vs_xa(name, lib, device, counts, ["x", "adj", "rank2"], monkeypatch)


def case_forced_vs_golden(name, lib, device, monkeypatch):
    """... and against the checkpoint's g1 reference outputs (unit and 0.3 scale, the score scaling at t = 0.5)."""
    forced(monkeypatch)
    eng, _, _ = pc.engine_from_ckpt(name, lib, device)
    assert eng.query("large_graph") == 1
    pc.case_forward_vs_reference_golden(name, lib, device)


# ---- 2. natural selection
def case_selection(lib, device, monkeypatch):
    """Without the switch, the grid_small_CC architecture with two hodge layers: N = 16 stays on k_xa, N = 17 (no k_xa layout) and
    N = 24 (E = 276 > 255) plan on the route; the enzymes_small_CC architecture at N = 14 too (plans without weights)."""
    forced(monkeypatch, False)
    for ckpt, N, lg in ((GRID, 16, 0), (GRID, 17, 1), (GRID, 24, 1), (ENZ, 14, 1), (ENZ, 13, 0)):
        meta, _ = arch_at(ckpt, N, num_layers_h=2)
        eng = cc.engine(meta, None, lib, device, weights=False)
        assert eng.query("large_graph") == lg, f"{ckpt} N = {N}: large_graph = {eng.query('large_graph')}"
        if not lg:
            assert eng.query("xa_lds_bytes") > 0


def case_natural_forwards(ckpt, N, counts, lib, device, monkeypatch, seed=9):
    """A naturally selected two-layer plan: the x and adj forwards and the t = 0.5 score scaling against the oracle."""
    forced(monkeypatch, False)
    meta, parts = arch_at(ckpt, N, num_layers_h=2)
    Nn, F, d_min, d_max = cc.dims(meta)
    flags = make_flags(len(counts), Nn, list(counts))
    state = pc.masked_state(seed, len(counts), Nn, F, True, d_min, d_max, flags)
    eng = cc.engine(meta, parts, lib, device)
    assert eng.query("large_graph") == 1
    args = [t.to(device) for t in state] + [flags.to(device)]
    want = cc.oracle_forwards(meta, parts, state, flags, ["x", "adj"])
    B = len(counts)
    for t, p in enumerate(["x", "adj"]):
        got = eng.score(t, *args)
        pc.assert_close(got, want[p], f"{ckpt}@{N}, two hodge layers, net_{p}")
        if p == "adj":
            cc.check_adj_masks(got, flags, f"{ckpt}@{N}")
        sde = loader.load_sde(meta["config"]["sde"][p])
        tt = torch.ones(B) * 0.5
        net = lambda x, a, r, f, p=p: O.run_network(meta[f"params_{p}"], parts[p], x, a, r, f)
        with torch.no_grad():
            wscore = O.make_score_fn(O.load_sde(meta["config"]["sde"][p]), net)(*state, flags, tt)
        ss = 1.0 if sde.kind == "VE" else float(-1.0 / sde.marginal_prob(torch.zeros(1, 1, 1), tt[:1])[1])
        pc.assert_close(eng.score(t, *args, ss), wscore, f"{ckpt}@{N}, two hodge layers, score_{p} t=0.5")


# ---- 3. three to six layers: the general hodge stack on the route
def case_kat(gname, tag, lib, device, monkeypatch):
    """One tag of kat_hodge_layers.npz / kat_hodge_general.npz forced onto the route against the reference constructor's output."""
    forced(monkeypatch)
    g = load_golden(gname)
    params = json.loads(str(g["meta"]))[tag]
    flags, x, adj, rank2 = (torch.from_numpy(g[f"{tag}/{k}"]).to(device) for k in ("flags", "x", "adj", "rank2"))
    sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/w/")}
    N, Fd = params["max_node_num"], params["max_feat_num"]
    eng = PCEngine(None, None, params, sd, None, None, N=N, F=Fd, is_cc=True, d_min=params["d_min"], d_max=params["d_max"],
                   device=device, lib=lib)
    assert eng.query("large_graph") == 1, f"{tag}: CCSD_LARGE_GRAPH=2 did not select the tiled graph-network route"
    assert eng.query("h_general") == 1
    got = eng.score(1, x, adj, rank2, flags)
    pc.assert_close(got, g[f"{tag}/out"], f"{gname} {tag} on the tiled route")
    cc.check_adj_masks(got, flags.cpu(), tag)


# ---- 4. production loop
def case_production_loop(name, counts, lib, device, predictor, corrector, snr, seps, monkeypatch):
    cc.case_forced_production_loop(lib, device, predictor, corrector, snr, seps, monkeypatch, name=name, counts=counts)


def case_nsteps2(lib, device, monkeypatch):
    cc.case_forced_nsteps2(lib, device, monkeypatch, name=ENZ, counts=(12, 7))


# ---- 5. planner
def case_planner(lib, device, monkeypatch):
    """The envelope's edges, forced and unforced (plans without weights)."""
    def plan_only(ckpt, N, **over):
        meta, _ = arch_at(ckpt, N, **over)
        return cc.engine(meta, None, lib, device, weights=False)

    for force in (False, True):
        forced(monkeypatch, force)
        with pytest.raises(NotImplementedError, match="two or more layers"):
            plan_only(GRID, 49, num_layers_h=2)
        with pytest.raises(NotImplementedError, match="two or more layers"):
            plan_only(GRID, 39, num_layers_h=2)                      # E = 741
        with pytest.raises(NotImplementedError, match="hodge attention dimensions above 16"):
            plan_only(GRID, 24, num_layers_h=2, adim_h=20)
        with pytest.raises(NotImplementedError, match="1 to 8 HodgeAdjAttentionLayers"):
            plan_only(GRID, 17, num_layers_h=9)
        eng = plan_only(GRID, 38, num_layers_h=2)                    # E = 703: the ceiling
        assert eng.query("large_graph") == 1
        # (eight layers of two channels: 36 graph + 18 hodge channels keep the final MLP a chained shape)
        eng = plan_only(GRID, 17, num_layers_h=8)
        assert eng.query("large_graph") == 1 and eng.query("h_general") == 1
    forced(monkeypatch, False)
    # route plans take no corrector fusion
    meta, _ = arch_at(ENZ, 14, num_layers_h=2)
    eng = cc.engine(meta, None, lib, device, weights=False, predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7)
    assert eng.query("large_graph") == 1 and eng.query("loop_form") == 1
    assert eng.query("tiled_fuse") == 0 and eng.query("fused_loop") == 0
    # the shipped two-layer checkpoints stay with k_xa without the switch
    for name in (QM9, ENZ):
        m, _ = load_ckpt_np(name)
        assert cc.engine(m, None, lib, device, weights=False).query("large_graph") == 0, f"{name} left k_xa without the switch"


# ---- 6. GPU only
def case_ceiling(lib, device, monkeypatch, counts=(38, 21), seed=13):
    """The grid architecture, two layers, at N = 38 (E = 703, K = 8436): the adj forward against the oracle."""
    forced(monkeypatch, False)
    meta, parts = arch_at(GRID, 38, num_layers_h=2)
    N, F, d_min, d_max = cc.dims(meta)
    flags = make_flags(len(counts), N, list(counts))
    state = pc.masked_state(seed, len(counts), N, F, True, d_min, d_max, flags)
    eng = cc.engine(meta, parts, lib, device)
    assert eng.query("large_graph") == 1
    got = eng.score(1, *[t.to(device) for t in state], flags.to(device))
    want = cc.oracle_forwards(meta, parts, state, flags, ["adj"])["adj"]
    pc.assert_close(got, want, "grid_small_CC@38, two hodge layers (E = 703), net_adj")
    cc.check_adj_masks(got, flags, "grid_small_CC@38")


CS_H2 = "ccsd_community_small_h2_CC"


def cs_h2():
    """community_small geometry (N = 20, E = 190, K = 1140) with qm9_CC's hodge settings and seeded weights."""
    return arch_at(CS, 20, seed=202, **QM9_HODGE)


def case_yaml_run(lib, tmp_path, num_scales=5, batch=8):
    """CCSD("sample", <yaml>, folder=<checkout with the checkpoint written here>).run(gpus=1) on the two-layer community_small
    network, a 5-scale SDE, batch 8: the route, shapes, finiteness, a symmetric 0/1 adjacency with a zero diagonal inside the flags."""
    import yaml

    from ccsd_amd.diffusion import CCSD

    meta, parts = cs_h2()
    arrays = {f"{p}/{k}": v.detach().numpy() for p in NAMES for k, v in parts[p].items()}
    arrays.update({f"ema_{k}": v for k, v in list(arrays.items())})
    meta = json.loads(json.dumps({k: v for k, v in meta.items() if k != "files"}))
    for p in NAMES:
        meta["config"]["sde"][p]["num_scales"] = num_scales
    meta["config"]["data"]["batch_size"] = batch
    data = meta["config"]["data"]
    d = tmp_path / "checkpoints" / data["data"]
    os.makedirs(d, exist_ok=True)
    np.savez(d / f"{CS_H2}.npz", **arrays)
    with open(d / f"{CS_H2}.json", "w") as f:
        json.dump(meta, f)
    cfg = {"is_cc": True, "data": data, "ckpt": CS_H2,
           "sampler": {"predictor": "Reverse", "corrector": "Langevin", "snr": 0.05, "scale_eps": 0.7, "n_steps": 1},
           "sample": dict(cc.GRID_YAML["sample"], divide_batch=1)}
    os.makedirs(tmp_path / "config", exist_ok=True)
    with open(tmp_path / "config" / "sample_community_small_h2_CC.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    c = CCSD("sample", "sample_community_small_h2_CC", folder=str(tmp_path))
    out = c.run(gpus=1, rounds=1)
    sm = c.sampler
    assert type(sm).__name__ == "Sampler_CC"
    assert sm.sampling_fn.engine().query("large_graph") == 1
    a, fl = out["adj_int"].cpu(), out["flags"].cpu()
    assert a.shape == (batch, 20, 20) and out["x"].shape == (batch, 20, data["max_feat_num"]) and out["rank2"].shape == (batch, 190, 1140)
    assert all(torch.isfinite(out[k]).all() for k in ("x", "adj", "rank2"))
    assert torch.equal(a, a.transpose(1, 2)) and not torch.diagonal(a, dim1=1, dim2=2).any()
    assert not (a * (1 - fl[:, :, None] * fl[:, None, :])).any()
