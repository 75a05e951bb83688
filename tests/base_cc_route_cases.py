"""Cases of the tiled graph-network route for ScoreNetworkA_Base_CC (k_lg_hb_*, ccsd_amd/csrc/ccsd_k_lg.h), shared by the CPU suite
(host emulation, tests/test_base_cc_route.py) and the GPU suite (tests/test_gpu_base_cc_route.py).  Every comparison takes
parity_cases.assert_close at its default tolerance.

No checkpoint of the reference has these architectures at these sizes: the fixtures' A-networks come from the reference's
constructors under a fixed seed (tools/make_golden.py base_cc_route), and the sizes no fixture covers (N = 18, N = 32) take weights
drawn here against the oracle."""
import math

import numpy as np
import pytest
import torch

from ccsd_amd import loader, plan
from ccsd_amd.engine import PCEngine
from oracle import ccsd_oracle as O
from tests import cc_large_graph_cases as cc
from tests import library_loop_cases as ll
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np, load_golden, make_flags, rng_matches

# config/grid_small_Base_CC.yaml's A-network (two HodgeBaselineLayers, widths 2, num_linears_h 1) at N = 49 (E = 1176, K = 18424)
# beside the X and F networks of cc_large/ccsd_grid_small_CC: a dense layer beyond E = 255, which the planner sends to the route
GRID = "base_cc_route/ccsd_grid_small_Base_CC"
GRID_GOLDEN = "ccsd_grid_small_Base_CC"
# config/ego_small_Base_CC.yaml's networks (THREE HodgeBaselineLayers: nhid_h 4, hidden_h 6, c_hid_h 4, c_final_h 6, num_linears_h 2)
# at N = 7, d 3..5 (E = 21, K = 91) and N = 12, d 3..4 (E = 66: four row tiles + 2)
EGO7, EGO7_GOLDEN = "base_cc_route/ccsd_ego_small_Base_CC_n7", "ccsd_ego_small_Base_CC_n7"
EGO12, EGO12_GOLDEN = "base_cc_route/ccsd_ego_small_Base_CC_n12", "ccsd_ego_small_Base_CC_n12"
NAMES = cc.NAMES
SHIPPED = ["ccsd_qm9_Base_CC", "ccsd_community_small_Base_CC", "ccsd_enzymes_small_Base_CC"]


def ego_params(N, d_max, **adj):
    """The three parameter dicts of the ego_small_Base_CC architecture at another geometry (+ overrides of the A-network's)."""
    meta, _ = load_ckpt_np(EGO7)
    pa = dict(meta["params_adj"], max_node_num=N, d_max=d_max, **adj)
    return meta["params_x"], pa, dict(meta["params_rank2"], max_node_num=N, d_max=d_max)


def plan_only(px, pa, pf, **kw):
    return PCEngine(px, None, pa, None, pf, None, N=pa["max_node_num"], F=pa["max_feat_num"], is_cc=True, d_min=pa["d_min"],
                    d_max=pa["d_max"], **kw)


def drawn_weights(params, seed):
    """A state dict of the network `params` describes (ccsd_amd.plan.state_dict_shapes): matrices N(0, 1 / fan-in), vectors N(0, 0.2)."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in plan.state_dict_shapes(params):
        std = 0.2 if len(shape) == 1 else 1.0 / math.sqrt(shape[-1])
        sd[key] = (torch.randn(*shape, generator=gen) * std).requires_grad_(True)
    return sd


def case_planner(lib, device, monkeypatch):
    """Without the switch: the three-layer architecture plans on the route at N = 7, 12, 18 and the grid architecture at N = 49, in
    the un-fused Langevin loop form (both raise on a planner without the feature); nine layers and blocks wider than 16 raise and
    name their reason; the shipped Base_CC checkpoints stay with k_xa."""
    monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)
    for N, d_max in ((7, 5), (12, 4), (18, 5)):
        eng = plan_only(*ego_params(N, d_max), device=device, lib=lib)
        assert eng.query("large_graph") == 1, f"three HodgeBaselineLayers at N = {N}: large_graph = {eng.query('large_graph')}"
    meta, _ = load_ckpt_np(GRID)
    eng = plan_only(meta["params_x"], meta["params_adj"], meta["params_rank2"], device=device, lib=lib, predictor="Reverse",
                    corrector="Langevin", snr=0.1, scale_eps=0.7)
    assert eng.query("large_graph") == 1
    assert eng.query("loop_form") == 1 and eng.query("tiled_fuse") == 0 and eng.query("fused_loop") == 0
    with pytest.raises(NotImplementedError, match="1 to 8 HodgeBaselineLayers"):
        plan_only(*ego_params(7, 5, num_layers_h=9), device=device, lib=lib)
    # (eight layers of two channels: 18 hodge + 24 graph channels keep the final MLP a chained shape)
    assert plan_only(*ego_params(7, 5, num_layers_h=8, c_hid_h=2, c_final_h=2), device=device, lib=lib).query("large_graph") == 1
    for force in ("0", "2"):
        monkeypatch.setenv("CCSD_LARGE_GRAPH", force)
        for over in (dict(hidden_h=17), dict(nhid_h=17)):
            with pytest.raises(NotImplementedError, match="ScoreNetworkA_Base_CC with BaselineBlocks wider than 16"):
                plan_only(*ego_params(7, 5, **over), device=device, lib=lib)
        with pytest.raises(NotImplementedError, match="ScoreNetworkA_Base_CC with BaselineBlocks wider than 16"):
            plan_only(meta["params_x"], dict(meta["params_adj"], nhid_h=17), meta["params_rank2"], device=device, lib=lib)
    monkeypatch.delenv("CCSD_LARGE_GRAPH")
    assert plan_only(*ego_params(7, 5, hidden_h=16, nhid_h=16), device=device, lib=lib).query("large_graph") == 1
    for name in SHIPPED:
        m, _ = load_ckpt_np(name)
        assert cc.engine(m, None, lib, device, weights=False).query("large_graph") == 0, f"{name} left k_xa without the switch"


def case_forced_vs_xa(name, lib, device, counts, monkeypatch):
    """CCSD_LARGE_GRAPH=2 on a shipped Base_CC checkpoint k_xa serves (two HodgeBaselineLayers): the x and adj forwards of the route
    against the oracle and against the un-forced k_xa engine; masks; the switch's value 1 leaves the plan on k_xa."""
    cc.case_forced_vs_xa(name, lib, device, counts, ["x", "adj"], monkeypatch)


def case_forced_ineligible(lib, device, monkeypatch):
    """ccsd_enzymes_small_Base_CC is not eligible for the route -- not for its hodge branch: its final MLP reads 46 graph + 18 hodge = 64
    channels, whose 128-wide hidden layers exceed the widest chained final-MLP shape (7 tiles = 112) k_lg_fin is built for -- and
    stays with k_xa under the switch."""
    meta, _ = load_ckpt_np("ccsd_enzymes_small_Base_CC")
    pa = meta["params_adj"]
    assert 2 * (pa["c_hid"] * (pa["num_layers"] - 1) + pa["c_final"] + pa["c_init"] + pa["c_hid_h"] + pa["c_final_h"] + pa["c_init"]) > 112
    monkeypatch.setenv("CCSD_LARGE_GRAPH", "2")
    assert cc.engine(meta, None, lib, device, weights=False).query("large_graph") == 0


def case_forwards_vs_golden(ckpt, gname, lib, device, score=False):
    """g1: the x and adj forwards at unit and 0.3 scale against the reference's outputs (the fixtures' flags hold full complexes, an
    empty, a one-node and a two-node one for the three-layer networks); the adj score is zero on the diagonal and outside the flags;
    score: the score_adj / score_x scaling at t = 0.5."""
    g = load_golden(f"g1_{gname}.npz")
    assert rng_matches(g)
    eng, meta, parts = pc.engine_from_ckpt(ckpt, lib, device)
    assert eng.query("large_graph") == 1
    N, F, d_min, d_max = cc.dims(meta)
    flags = torch.from_numpy(g["flags"])
    dv = lambda t: t.to(device)
    for tag, scale in (("unit", 1.0), ("small", 0.3)):
        state = pc.masked_state(int(g["seed"]), flags.shape[0], N, F, True, d_min, d_max, flags, scale)
        assert np.array_equal(state[1].numpy(), g[f"{tag}/adj"])
        args = [dv(t) for t in state] + [dv(flags)]
        for t, p in enumerate(["x", "adj"]):
            got = eng.score(t, *args)
            pc.assert_close(got, g[f"{tag}/net_{p}"], f"{gname} {tag} net_{p}")
            if p == "adj":
                cc.check_adj_masks(got, flags, f"{gname} {tag}")
            if score and tag == "unit":
                sde = loader.load_sde(meta["config"]["sde"][p])
                ss = float(-1.0 / sde.marginal_prob(torch.zeros(1, 1, 1), torch.ones(1) * 0.5)[1])
                pc.assert_close(eng.score(t, *args, ss), g[f"unit/score_{p}_t1"], f"{gname} score_{p} t=0.5")


def case_adj_vs_oracle(N, d_max, counts, lib, device, seed=31):
    """The three-layer architecture with drawn weights at a geometry no fixture covers: the adj forward against the oracle."""
    px, pa, pf = ego_params(N, d_max)
    w = drawn_weights(pa, seed)
    eng = PCEngine(px, drawn_weights(px, seed + 1), pa, w, pf, drawn_weights(pf, seed + 2), N=N, F=pa["max_feat_num"], is_cc=True,
                   d_min=pa["d_min"], d_max=d_max, device=device, lib=lib)
    assert eng.query("large_graph") == 1
    flags = make_flags(len(counts), N, list(counts))
    state = pc.masked_state(seed, len(counts), N, pa["max_feat_num"], True, pa["d_min"], d_max, flags)
    with torch.no_grad():
        want = O.run_network(pa, w, *state, flags)
    got = eng.score(1, *[t.to(device) for t in state], flags.to(device))
    pc.assert_close(got, want, f"three HodgeBaselineLayers at N = {N} net_adj vs the oracle")
    cc.check_adj_masks(got, flags, f"N = {N}")


def case_sampler_vs_golden(lib, device):
    """g5: two steps of ego_small_Base_CC.yaml's sampler (Euler, no corrector) at 4 scales, N = 7, every draw from torch's CPU generator."""
    pc.case_pc_sampler_identical_seed(EGO7_GOLDEN, EGO7, "n4_first2", lib, device)


def case_production_loop(lib, device, predictor, corrector, snr, seps):
    """parity_cases.case_production_loop_vs_oracle on the three-layer networks at N = 7, B = 2, two steps."""
    loop = 3 if predictor == "S4" else 1 if corrector == "Langevin" else 0
    pc.case_production_loop_vs_oracle(EGO7, lib, device, 2, [7, 5], 2, predictor, corrector, snr, seps,
                                      expect_route={"large_graph": 1, "loop_form": loop, "tiled_fuse": 0, "fused_loop": 0})


def case_nsteps2(lib, device):
    """sampler.n_steps = 2 (Reverse + Langevin), three layers at N = 7: the library loop == the step-wise driver, bit for bit."""
    _, fn, _, _, _ = ll.case_nsteps_library_vs_stepwise(EGO7, lib, device, 2, [7, 5], 2, "Reverse", 0.1, 0.7, 2)
    assert fn.engine().query("large_graph") == 1


def case_grid_library_vs_stepwise(lib, device, B=2, counts=(49, 30), steps=2, seed=23):
    """Grid architecture at N = 49: a two-step Reverse + Langevin ccsd_sampler_run == the step-wise driver, bit for bit."""
    su = ll.Setup(GRID, lib, device, "Reverse", "Langevin", 0.1, 0.7)
    flags = make_flags(B, su.N, list(counts)).to(device)
    fn = su.sampler(B, steps, seed)
    got = fn(*su.models, flags)
    assert fn.last_loop == "library" and fn.engine().query("large_graph") == 1 and fn.engine().query("loop_form") == 1
    fs = su.sampler(B, steps, seed, group=pc._FakeGroup())
    ref = fs(*su.models, flags)
    assert fs.last_loop == "stepwise"
    for p, a, b in zip(su.names, got[:su.nt], ref[:su.nt]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"grid_small_Base_CC: library loop != step-wise driver for {p}"


def case_grid_yaml_run(lib, tmp_path, num_scales=3):
    """CCSD(type="sample", config=<sample_grid_small_Base_CC.yaml's content with a short SDE>, folder=<checkout with the fixture as
    checkpoint>).run(gpus=1): the shipped batch of 8 in divide_batch = 4 pieces, on the route.  (The yaml samples with use_ema: the
    fixture's weights stand for the EMA ones too.)"""
    import json
    import os

    import yaml

    from ccsd_amd.diffusion import CCSD

    meta, parts = load_ckpt_np(GRID)
    arrays = {f"{p}/{k}": v.detach().numpy() for p in NAMES for k, v in parts[p].items()}
    arrays.update({f"ema_{k}": v for k, v in list(arrays.items())})
    meta = {k: v for k, v in meta.items() if k != "files"}
    for p in NAMES:
        meta["config"]["sde"][p]["num_scales"] = num_scales
    d = tmp_path / "checkpoints" / "grid_small_CC"
    os.makedirs(d, exist_ok=True)
    np.savez(d / "ccsd_grid_small_Base_CC.npz", **arrays)
    with open(d / "ccsd_grid_small_Base_CC.json", "w") as f:
        json.dump(meta, f)
    cfg = dict(cc.GRID_YAML, ckpt="ccsd_grid_small_Base_CC", sample=dict(cc.GRID_YAML["sample"], divide_batch=4))
    os.makedirs(tmp_path / "config", exist_ok=True)
    with open(tmp_path / "config" / "sample_grid_small_Base_CC.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    c = CCSD("sample", "sample_grid_small_Base_CC", folder=str(tmp_path))
    out = c.run(gpus=1, rounds=1)
    sm = c.sampler
    assert type(sm).__name__ == "Sampler_CC" and sm.divide_batch == 4
    assert sm.sampling_fn.engine().query("large_graph") == 1
    a, fl = out["adj_int"].cpu(), out["flags"].cpu()
    assert a.shape == (8, 49, 49) and out["x"].shape == (8, 49, 5) and out["rank2"].shape == (8, 1176, 18424)
    assert all(torch.isfinite(out[k]).all() for k in ("x", "adj", "rank2"))
    assert torch.equal(a, a.transpose(1, 2)) and not torch.diagonal(a, dim1=1, dim2=2).any()
    assert not (a * (1 - fl[:, :, None] * fl[:, None, :])).any()
