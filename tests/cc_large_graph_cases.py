"""Cases of the tiled graph-network route for combinatorial complexes with ScoreNetworkA_CC and ONE hodge layer (k_lg_hodge1,
ccsd_amd/csrc/ccsd_k_lg.h), shared by the CPU suite (host emulation, tests/test_cc_large_graph.py) and the GPU suite
(tests/test_gpu_cc_large_graph.py).  Every comparison takes parity_cases.assert_close at its default tolerance."""
import pytest
import torch

from ccsd_amd import loader
from ccsd_amd.engine import PCEngine
from oracle import ccsd_oracle as O
from tests import library_loop_cases as ll
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np, make_flags

# ccsd_grid_small_CC (N = 49, d_min = d_max = 3: E = 1176, K = 18424), the weights sample_grid_small_CC.yaml samples with.  The
# fixture lies in a folder of its own below tests/golden/ckpt/ (tests/test_large_graph.py pins the k_xa variant of every checkpoint
# in ckpt/ itself); load_ckpt_np finds it by this name.
GRID = "cc_large/ccsd_grid_small_CC"
GRID_GOLDEN = "ccsd_grid_small_CC"
# k_xa keeps an LDS layout for the architecture up to N = 42 and has none from N = 43 (E = 903, K = 12341)
CROSSOVER = 43
# the four weights of the architecture whose row count is K
K_ROWS = [f"layers_hodge.0.attn.{c}.ccnn_{q}.weight" for c in (0, 1) for q in ("q", "k")]
NAMES = ["x", "adj", "rank2"]
_cache = {}


def dims(meta):
    d = meta["config"]["data"]
    return d["max_node_num"], d["max_feat_num"], d["d_min"], d["d_max"]


def engine(meta, parts, lib, device, weights=True, **kw):
    N, F, d_min, d_max = dims(meta)
    w = (lambda p: parts[p]) if weights else (lambda p: None)
    return PCEngine(meta["params_x"], w("x"), meta["params_adj"], w("adj"), meta["params_rank2"], w("rank2"), N=N, F=F, is_cc=True,
                    d_min=d_min, d_max=d_max, device=device, lib=lib, **kw)


def grid_at(N):
    """The grid_small_CC architecture at another node count: every weight from the fixture, the four K-dependent hodge weights
    cut to their first K(N) rows (a same-architecture network with arbitrary weights)."""
    if N not in _cache:
        meta, parts = load_ckpt_np(GRID)
        K = O.get_rank2_dim(N, 3, 3)[1]
        meta = dict(meta, params_adj=dict(meta["params_adj"], max_node_num=N), params_rank2=dict(meta["params_rank2"], max_node_num=N))
        meta["config"] = dict(meta["config"], data=dict(meta["config"]["data"], max_node_num=N))
        adj = dict(parts["adj"])
        for k in K_ROWS:
            assert adj[k].shape[0] == 18424
            adj[k] = adj[k].detach()[:K].clone().requires_grad_(True)
        _cache[N] = (meta, dict(parts, adj=adj))
    return _cache[N]


def oracle_forwards(meta, parts, state, flags, targets):
    with torch.no_grad():
        return {p: O.run_network(meta[f"params_{p}"], parts[p], *state, flags) for p in targets}


def check_adj_masks(a, flags, what):
    a = a.detach().cpu()
    fm = flags[:, :, None] * flags[:, None, :]
    assert torch.all(a[fm == 0] == 0), f"{what}: the adj score is not zero outside the flags"
    assert torch.all(torch.diagonal(a, dim1=1, dim2=2) == 0), f"{what}: the adj score is not zero on the diagonal"


def case_forced_vs_xa(name, lib, device, counts, targets, monkeypatch, seed=4):
    """CCSD_LARGE_GRAPH=2 (read at plan creation) takes a one-hodge-layer combinatorial-complex plan that k_xa serves through the
    tiled kernels: large_graph == 1, and the forwards meet the oracle and the un-forced k_xa engine (within assert_close, not bit
    for bit: the summation orders differ); the adj score is zero on the diagonal and outside the flags.  (The switch's value 1
    forces graph-only plans alone and leaves combinatorial complexes on k_xa, as tests/golden/route_plans.json pins them.)"""
    meta, parts = load_ckpt_np(name)
    N, F, d_min, d_max = dims(meta)
    B = len(counts)
    flags = make_flags(B, N, counts)
    state = pc.masked_state(seed, B, N, F, True, d_min, d_max, flags)
    dv = lambda t: t.to(device)
    monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)
    ref = engine(meta, parts, lib, device)
    assert ref.query("large_graph") == 0
    monkeypatch.setenv("CCSD_LARGE_GRAPH", "1")
    assert engine(meta, parts, lib, device, weights=False).query("large_graph") == 0
    monkeypatch.setenv("CCSD_LARGE_GRAPH", "2")
    lg = engine(meta, parts, lib, device)
    monkeypatch.delenv("CCSD_LARGE_GRAPH")
    assert lg.query("large_graph") == 1, f"{name}: CCSD_LARGE_GRAPH=2 did not select the tiled graph-network route"
    assert lg.query("r2_family") == ref.query("r2_family")
    want = oracle_forwards(meta, parts, state, flags, targets)
    args = [dv(t) for t in state] + [dv(flags)]
    for p in targets:
        t = NAMES.index(p)
        got = lg.score(t, *args)
        pc.assert_close(got, want[p], f"{name} CCSD_LARGE_GRAPH=2 net_{p} vs the oracle")
        pc.assert_close(got, ref.score(t, *args).cpu(), f"{name} CCSD_LARGE_GRAPH=2 net_{p} vs k_xa")
        if p == "adj":
            check_adj_masks(got, flags, name)


def crossover_setup(lib, device, counts, seed=7):
    """(meta, parts, engine, state, flags) of the grid_small_CC architecture at the smallest node count k_xa cannot place."""
    meta, parts = grid_at(CROSSOVER)
    N, F, d_min, d_max = dims(meta)
    flags = make_flags(len(counts), N, counts)
    state = pc.masked_state(seed, len(counts), N, F, True, d_min, d_max, flags)
    return meta, parts, engine(meta, parts, lib, device), state, flags


def case_crossover_selection(lib, device, monkeypatch):
    """Without the switch: N = 43 plans on the tiled route, N = 42 stays with k_xa (plans without weights: the planner alone)."""
    monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)
    for N, lg in ((CROSSOVER, 1), (CROSSOVER - 1, 0)):
        meta, parts = grid_at(N)
        eng = engine(meta, parts, lib, device, weights=False)
        assert eng.query("large_graph") == lg, f"N = {N}: large_graph = {eng.query('large_graph')}"
        assert (eng.query("xa_lds_bytes") > 0) == (lg == 0)
        assert eng.query("r2_family") == 3


def case_crossover_forwards(lib, device, counts=(43, 17)):
    """N = 43, naturally selected: the x and adj forwards and the score scaling at t = 0.5 against the oracle (only P_0 and the
    graph kernels run: cheap on the emulation)."""
    meta, parts, eng, state, flags = crossover_setup(lib, device, list(counts))
    assert eng.query("large_graph") == 1
    dv = lambda t: t.to(device)
    args = [dv(t) for t in state] + [dv(flags)]
    want = oracle_forwards(meta, parts, state, flags, ["x", "adj"])
    B = len(counts)
    for t, p in enumerate(["x", "adj"]):
        got = eng.score(t, *args)
        pc.assert_close(got, want[p], f"grid_small_CC@{CROSSOVER} net_{p}")
        if p == "adj":
            check_adj_masks(got, flags, f"grid_small_CC@{CROSSOVER}")
        sde = loader.load_sde(meta["config"]["sde"][p])
        tt = torch.ones(B) * 0.5
        net = lambda x, a, r, f, p=p: O.run_network(meta[f"params_{p}"], parts[p], x, a, r, f)
        with torch.no_grad():
            wscore = O.make_score_fn(O.load_sde(meta["config"]["sde"][p]), net)(*state, flags, tt)
        ss = 1.0 if sde.kind == "VE" else float(-1.0 / sde.marginal_prob(torch.zeros(1, 1, 1), tt[:1])[1])
        pc.assert_close(eng.score(t, *args, ss), wscore, f"grid_small_CC@{CROSSOVER} score_{p} t=0.5")


def case_crossover_rank2(lib, device, counts=(43, 17)):
    """N = 43: the rank2 forward against the oracle -- k_gemm_h / k_hf_score at E = 903, beyond the 703 rows they had run at."""
    meta, parts, eng, state, flags = crossover_setup(lib, device, list(counts))
    dv = lambda t: t.to(device)
    want = oracle_forwards(meta, parts, state, flags, ["rank2"])["rank2"]
    pc.assert_close(eng.score(2, *[dv(t) for t in state], dv(flags)), want, f"grid_small_CC@{CROSSOVER} net_rank2 (E = 903)")


def case_forced_production_loop(lib, device, predictor, corrector, snr, seps, monkeypatch, name="ccsd_community_small_CC",
                                counts=(20, 11)):
    """parity_cases.case_production_loop_vs_oracle on the forced route, B = 2, two steps: ccsd_sampler_run value for value against
    the oracle on the exported draws, the step-wise driver bit for bit.  The plan takes the un-fused loop form of its sampler."""
    monkeypatch.setenv("CCSD_LARGE_GRAPH", "2")
    loop = 3 if predictor == "S4" else 1 if corrector == "Langevin" else 0
    pc.case_production_loop_vs_oracle(name, lib, device, 2, list(counts), 2, predictor, corrector, snr, seps,
                                      expect_route={"large_graph": 1, "loop_form": loop, "tiled_fuse": 0, "fused_loop": 0})


def case_forced_nsteps2(lib, device, monkeypatch, name="ccsd_community_small_CC", counts=(20, 11)):
    """sampler.n_steps = 2 (Reverse + Langevin) on the forced route: the library loop == the step-wise driver, bit for bit."""
    monkeypatch.setenv("CCSD_LARGE_GRAPH", "2")
    _, fn, _, _, _ = ll.case_nsteps_library_vs_stepwise(name, lib, device, 2, list(counts), 2, "Reverse", 0.1, 0.7, 2)
    assert fn.engine().query("large_graph") == 1


def case_planner_rejections(lib, device, monkeypatch):
    """What the route does not serve still raises, and names its reason: ScoreNetworkA_Base_CC and two hodge layers at a geometry
    k_xa cannot place (N = 49), under the switch too; combinatorial complexes above 64 nodes."""
    meta, parts = load_ckpt_np(GRID)
    N, F, d_min, d_max = dims(meta)

    def plan(params_adj, n=N):
        return PCEngine(meta["params_x"], None, dict(params_adj, max_node_num=n), None, dict(meta["params_rank2"], max_node_num=n), None,
                        N=n, F=F, is_cc=True, d_min=d_min, d_max=d_max, device=device, lib=lib)

    # (HodgeBaselineLayer blocks 24 wide: their hidden rows alone, 2 x 1176 x 24 floats, exceed a CU's LDS)
    base = dict(meta["params_adj"], model_type="ScoreNetworkA_Base_CC", nhid_h=24, hidden_h=24)
    two = dict(meta["params_adj"], num_layers_h=2)
    for force in (False, True):
        if force:
            monkeypatch.setenv("CCSD_LARGE_GRAPH", "2")
        else:
            monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)
        with pytest.raises(NotImplementedError, match="ScoreNetworkA_Base_CC"):
            plan(base)
        with pytest.raises(NotImplementedError, match="two or more layers"):
            plan(two)
        with pytest.raises(NotImplementedError, match="N <= 64"):
            plan(meta["params_adj"], 80)
    monkeypatch.delenv("CCSD_LARGE_GRAPH")
    # ... while the shipped architecture plans at its own geometry, on the tiled route, in the un-fused Langevin loop
    eng = PCEngine(meta["params_x"], None, meta["params_adj"], None, meta["params_rank2"], None, N=N, F=F, is_cc=True, d_min=d_min,
                   d_max=d_max, device=device, lib=lib, predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7)
    assert eng.query("large_graph") == 1 and eng.query("r2_family") == 3
    assert eng.query("loop_form") == 1 and eng.query("tiled_fuse") == 0 and eng.query("fused_loop") == 0


# ---- the node counts between the crossover and the shipped N = 49 at which E K > 2^22 made FastDiv(K) split flat Philox groups
# into the wrong row (206, 125 and 15 groups per complex: tests/test_probe.py); k_noise_norm and k_langevin_apply run on every step
# of the un-fused Langevin loop these plans take
SPLIT_NODE_COUNTS = (44, 45, 47)


def case_split_shape_production_loop(lib, device, N):
    """grid_at(N), Reverse + Langevin (snr 0.1, scale_eps 0.7), one step, B = 3 with node counts [N, 2, N] -- a full complex followed
    by a near-empty one, and a full one last in the batch -- through parity_cases.case_production_loop_vs_oracle: the oracle replays
    the draws ccsd_noise_draws exports (k_init_state splits flat groups by integer division), so a group the loop's kernels split
    into the wrong row shows as a difference; the step-wise driver (ccsd_corrector_norms / ccsd_corrector_apply) bit for bit."""
    pc.case_production_loop_vs_oracle(f"grid_small_CC@{N}", lib, device, 3, [N, 2, N], 1, "Reverse", "Langevin", 0.1, 0.7,
                                      source=grid_at(N), expect_route={"large_graph": 1, "loop_form": 1})


# ---- the real checkpoint at N = 49 (GPU suite: one rank2 forward takes minutes on the emulation)
def case_grid_forwards(lib, device):
    """g1: x and adj (and their score scaling at t = 0.5) against the reference's outputs; rank2 through its summary: the fixture's
    subsample, and the row sums within the bound the element-wise tolerance implies (|sum(got - ref)| <= K * RTOL * scale).  The
    CPU suite pins the oracle to the same summary bit for bit."""
    from tests.helpers import load_golden, rng_matches

    g = load_golden(f"g1_{GRID_GOLDEN}.npz")
    assert rng_matches(g)
    eng, meta, parts = pc.engine_from_ckpt(GRID, lib, device)
    assert eng.query("large_graph") == 1
    N, F, d_min, d_max = dims(meta)
    flags = torch.from_numpy(g["flags"])
    dv = lambda t: t.to(device)
    for tag, scale in (("unit", 1.0), ("small", 0.3)):
        state = pc.masked_state(int(g["seed"]), flags.shape[0], N, F, True, d_min, d_max, flags, scale)
        args = [dv(t) for t in state] + [dv(flags)]
        for t, p in enumerate(["x", "adj"]):
            pc.assert_close(eng.score(t, *args), g[f"{tag}/net_{p}"], f"{GRID_GOLDEN} {tag} net_{p}")
        r = eng.score(2, *args).cpu()
        key = f"{tag}/net_rank2"
        ref = torch.from_numpy(g[f"{key}/val"])
        pc.assert_close(r.reshape(-1)[torch.from_numpy(g[f"{key}/idx"])], ref, f"{GRID_GOLDEN} {tag} net_rank2 (subsample)")
        rs, rref = r.double().sum(-1), torch.from_numpy(g[f"{key}/rowsum"])
        bound = r.shape[-1] * pc.RTOL * max(ref.abs().max().item(), 1e-6)
        assert (rs - rref).abs().max().item() <= bound, f"{GRID_GOLDEN} {tag} net_rank2: row sums differ by more than K * RTOL * scale"
    for t, p in enumerate(["x", "adj"]):
        sde = loader.load_sde(meta["config"]["sde"][p])
        ss = float(-1.0 / sde.marginal_prob(torch.zeros(1, 1, 1), torch.ones(1) * 0.5)[1])
        state = pc.masked_state(int(g["seed"]), flags.shape[0], N, F, True, d_min, d_max, flags, 1.0)
        pc.assert_close(eng.score(t, *[dv(v) for v in state], dv(flags), ss), g[f"unit/score_{p}_t1"], f"{GRID_GOLDEN} score_{p} t=0.5")


def case_grid_sampler_vs_golden(lib, device):
    """g5: the first two steps of the shipped 1000-scale sampler, every draw from torch's CPU generator, against the oracle through
    the same seed and the reference's quantised adjacency (parity_cases.case_pc_sampler_vs_oracle: the form of
    case_pc_sampler_identical_seed for fixtures whose rank-2 arrays are summaries)."""
    pc.case_pc_sampler_vs_oracle(GRID_GOLDEN, GRID, "n1000_first2", lib, device)


def case_grid_production_loop(lib, device):
    """ccsd_sampler_run at sample_grid_small_CC.yaml's sampler settings, B = 2, counts [49, 30], two steps, against the oracle."""
    pc.case_production_loop_vs_oracle(GRID, lib, device, 2, [49, 30], 2, "Reverse", "Langevin", 0.1, 0.7,
                                      expect_route={"large_graph": 1, "loop_form": 1, "tiled_fuse": 0})


# ---- harness
GRID_YAML = {
    "is_cc": True,
    "data": {"data": "grid_small_CC", "dir": "./data", "batch_size": 8, "test_split": 0.2, "max_node_num": 49, "max_feat_num": 5,
             "init": "deg", "min_node_val": 1, "max_node_val": 1, "node_label": "weight", "min_edge_val": 1, "max_edge_val": 1,
             "edge_label": "weight", "d_min": 3, "d_max": 3, "lifting_procedure": "path_based", "lifting_procedure_kwargs": "basic"},
    "ckpt": "ccsd_grid_small_CC",
    "sampler": {"predictor": "Reverse", "corrector": "Langevin", "snr": 0.1, "scale_eps": 0.7, "n_steps": 1},
    "sample": {"divide_batch": 8, "cc_nb_eval": 1000, "use_ema": True, "noise_removal": True, "probability_flow": False,
               "eps": 1.0e-4, "seed": 12},
}


def grid_folder(tmp_path, num_scales):
    """A checkout-like folder: the fixture checkpoint in the neutral format under checkpoints/grid_small_CC/ with a short SDE.  The
    fixture holds the EMA-applied weights (its json: ema_applied, ema_params); the yaml's use_ema finds them as ema_<part>/ entries."""
    import json
    import os

    import numpy as np

    from tests.helpers import GOLDEN_CKPT

    with open(os.path.join(GOLDEN_CKPT, GRID + ".json")) as f:
        meta = json.load(f)
    assert meta["ema_applied"] is True
    arrays = {}
    for fname in meta.pop("files"):
        z = np.load(os.path.join(GOLDEN_CKPT, fname))
        arrays.update({k: z[k] for k in z.files})
    for p, names in meta["ema_params"].items():
        arrays.update({f"ema_{p}/{n}": arrays[f"{p}/{n}"] for n in names})
    for p in NAMES:
        meta["config"]["sde"][p]["num_scales"] = num_scales
    d = tmp_path / "checkpoints" / "grid_small_CC"
    os.makedirs(d, exist_ok=True)
    np.savez(d / "ccsd_grid_small_CC.npz", **arrays)
    with open(d / "ccsd_grid_small_CC.json", "w") as f:
        json.dump(meta, f)


def case_grid_yaml_run(lib, tmp_path, num_scales=5):
    """CCSD(type="sample", config=<sample_grid_small_CC.yaml's content with a 5-scale SDE>, folder=<checkout with the fixture
    checkpoint>).run(gpus=1): the shipped batch of 8 in divide_batch pieces, the tiled route at N = 49."""
    import os

    import numpy as np
    import yaml

    from ccsd_amd import sampler as S
    from ccsd_amd.diffusion import CCSD
    from tests.helpers import load_golden

    grid_folder(tmp_path, num_scales)
    os.makedirs(tmp_path / "config", exist_ok=True)
    with open(tmp_path / "config" / "sample_grid_small_CC.yaml", "w") as f:
        yaml.safe_dump(GRID_YAML, f)
    c = CCSD("sample", "sample_grid_small_CC", folder=str(tmp_path))
    out = c.run(gpus=1, rounds=1)
    sm = c.sampler
    assert type(sm).__name__ == "Sampler_CC" and sm.divide_batch == 8 and sm.n_test == 20
    assert sm.sampling_fn.engine().query("large_graph") == 1
    a, fl = out["adj_int"].cpu(), out["flags"].cpu()
    assert a.shape == (8, 49, 49) and out["x"].shape == (8, 49, 5) and out["rank2"].shape == (8, 1176, 18424)
    assert all(torch.isfinite(out[k]).all() for k in ("x", "adj", "rank2"))
    assert torch.equal(a, a.transpose(1, 2)) and not torch.diagonal(a, dim1=1, dim2=2).any()
    assert not (a * (1 - fl[:, :, None] * fl[:, None, :])).any()
    # g7_init_flags.npz holds no grid_small entry for the yaml's seed drawn one complex at a time (divide_batch = batch): the node
    # counts come from the training split of node_counts.json, as init_flags draws them after load_seed(sample.seed)
    assert not any(k.startswith("grid_small/s12_b1") for k in load_golden("g7_init_flags.npz").files)
    counts = S.train_node_counts(sm.configt)
    np.random.seed(12)
    want = torch.cat([S.init_flags(counts, sm.configt, 1) for _ in range(8)], dim=0)
    assert torch.equal(fl, want)
    return out
