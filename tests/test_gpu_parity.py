"""GPU suite (-m gpu): the HIP library on a real MI355X through the C ABI, against the reference goldens
(captured from the reference on CPU) and the CPU oracle on the same seeded inputs."""
import pytest

import bench
import torch

from tests import parity_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# shipped checkpoints the package does not carry: weights under tests/golden/ckpt/, reference goldens stored whole
SHIPPED = ["ccsd_enzymes_small_Base_CC", "gdss_qm9", "gdss_qm9_retrained", "gdss_ego_small", "gdss_ego_small_retrained",
           "gdss_enzymes_small_retrained"]


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib

    L = _lib.get_library()          # raises if libccsd_hip.so has not been built: no fallback
    assert L.is_hip
    assert torch.cuda.is_available()
    return L


@pytest.mark.parametrize("name", ["ccsd_qm9_CC", "ccsd_community_small_CC", "gdss_community_small",
                                  "ccsd_enzymes_small_CC", "gdss_zinc250k", "ccsd_qm9_Base_CC",
                                  "ccsd_community_small_Base_CC", *SHIPPED])
def test_forward_vs_reference_golden(lib, name):
    pc.case_forward_vs_reference_golden(name, lib, DEV)


EGO_CC = ["ccsd_ego_small_CC", "ccsd_ego_small_CC_v2"]


@pytest.mark.parametrize("name", EGO_CC)
def test_forward_vs_oracle_ego_small_cc(lib, name):
    """ego_small_CC / _v2 (E = 153, K = 12444): forwards and score scaling against the oracle computed in the test (their rank-2
    goldens are summaries, pinned to the oracle by the CPU suite)."""
    pc.case_forward_vs_oracle(name, lib, DEV)


@pytest.mark.parametrize("name", EGO_CC)
@pytest.mark.parametrize("case", ["k6", "n1000_first2"])
def test_pc_sampler_vs_oracle_ego_small_cc(lib, name, case):
    """Short sampler runs of ego_small_CC / _v2 at sample_ego_small_CC.yaml's settings (Euler + None) against the oracle."""
    pc.case_pc_sampler_vs_oracle(name, name, case, lib, DEV)


def test_model_objects(lib):
    pc.case_model_objects_forward(lib, DEV)


@pytest.mark.gpu
def test_kat_gmh(lib):
    pc.case_kat_gmh(lib, DEV)


def test_kat_small_general_paths(lib):
    pc.case_kat_small_general(lib, DEV)


@pytest.mark.parametrize("gname,ckpt,case", [
    ("ccsd_qm9_CC", "ccsd_qm9_CC", "k10"),
    ("ccsd_qm9_CC", "ccsd_qm9_CC", "k50"),
    ("ccsd_qm9_CC", "ccsd_qm9_CC", "n1000_first3"),
    ("ccsd_qm9_Base_CC", "ccsd_qm9_Base_CC", "n1000_first3"),
    ("ccsd_community_small_CC", "ccsd_community_small_CC", "k5"),
    ("ccsd_community_small_CC", "ccsd_community_small_CC", "n1000_first2"),
    ("gdss_community_small", "gdss_community_small", "k10"),
    ("gdss_community_small", "gdss_community_small", "n1000_first3"),
    ("ccsd_qm9_CC_nsteps2_none", "ccsd_qm9_CC", "k6"),
    ("ccsd_qm9_CC_langevin2", "ccsd_qm9_CC", "k4"),
    ("gdss_zinc250k", "gdss_zinc250k", "k5"),
    ("s4_ccsd_qm9_CC", "ccsd_qm9_CC", "k6"),
    ("s4_gdss_community_small", "gdss_community_small", "k5"),
    ("s4_ccsd_enzymes_small_CC", "ccsd_enzymes_small_CC", "k20"),
    ("s4_ccsd_enzymes_small_CC", "ccsd_enzymes_small_CC", "n1000_first2"),
    # subVPSDE (Euler / Reverse), probability_flow + Reverse (CC and graph-only), subVP(x) + VE mixed with n_steps = 2
    ("ccsd_qm9_CC_subvp_euler", "ccsd_qm9_CC", "k6"),
    ("ccsd_qm9_CC_subvp_reverse", "ccsd_qm9_CC", "k6"),
    ("ccsd_qm9_CC_pflow", "ccsd_qm9_CC", "k6"),
    ("gdss_community_small_pflow", "gdss_community_small", "k5"),
    ("ccsd_qm9_CC_subvp_mixed", "ccsd_qm9_CC", "k4"),
    # the metric's own length: the shipped 1000-scale qm9_CC set-up from the prior to the last step, every draw from the CPU generator
    ("ccsd_qm9_CC_full1000", "ccsd_qm9_CC", "n1000"),
    # shipped checkpoints the package does not carry (weights under tests/golden/ckpt/), at their own sample_*.yaml settings
    # (S4 on ccsd_enzymes_small_Base_CC at 6 scales: parity_cases.TRAJ_RTOL, test_fp64_arbiter_s4_enzymes_base_cc)
    *[(n, n, c) for n in SHIPPED for c in ("k6", "n1000_first2")],
])
def test_pc_sampler_identical_seed(lib, gname, ckpt, case):
    pc.case_pc_sampler_identical_seed(gname, ckpt, case, lib, DEV)


@pytest.mark.parametrize("case", ["k4", "k20"])
def test_fp64_arbiter_s4_enzymes(lib, case):
    """The two cases whose tolerance against the fp32 reference golden is wider than 1e-4 (parity_cases.TRAJ_RTOL), judged
    against the float64 trajectory: the product may not be further from it than the reference is."""
    r = pc.case_fp64_arbiter("s4_ccsd_enzymes_small_CC", "ccsd_enzymes_small_CC", case, lib, DEV)
    e_ref, e_mine, e_mut = r["rank2"]
    assert e_mut <= e_ref + e_mine + 1e-7
    assert e_ref > 0.9e-4, "the reference itself is no longer > 1e-4 from the exact trajectory: tighten TRAJ_RTOL"


def test_fp64_arbiter_s4_enzymes_base_cc(lib):
    """The third TRAJ_RTOL case (S4 on ccsd_enzymes_small_Base_CC, 6 scales) judged against the float64 trajectory."""
    r = pc.case_fp64_arbiter("ccsd_enzymes_small_Base_CC", "ccsd_enzymes_small_Base_CC", "k6", lib, DEV)
    e_ref, e_mine, e_mut = r["rank2"]
    assert e_mut <= e_ref + e_mine + 1e-7
    assert e_ref > 0.9e-4, "the reference itself is no longer > 1e-4 from the exact trajectory: tighten TRAJ_RTOL"


def test_fp64_arbiter_qm9(lib):
    """Control: on a well-conditioned case both the reference and the product sit within 2e-5 of the float64 trajectory."""
    r = pc.case_fp64_arbiter("ccsd_qm9_CC", "ccsd_qm9_CC", "k10", lib, DEV)
    for p, (e_ref, e_mine, _) in r.items():
        assert e_ref < 5e-5 and e_mine < 5e-5, (p, e_ref, e_mine)


def test_kat_cnum_more_hodge_powers(lib):
    pc.case_kat_cnum(lib, DEV)


def test_zinc5b_substitute(lib):
    pc.case_zinc5b(lib, DEV)


def test_philox_properties(lib):
    pc.case_philox_properties(lib, DEV)


def test_philox_calls_are_independent(lib):
    pc.case_philox_calls_are_independent(lib, DEV)


def test_philox_langevin_nsteps2(lib):
    pc.case_philox_langevin_nsteps2(lib, DEV)


def test_philox_prior_statistics(lib):
    pc.case_philox_prior_statistics(lib, DEV)


def test_error_behaviour(lib):
    pc.case_error_behaviour(lib, DEV)


def test_rank2_cells_sparse_output(lib):
    pc.case_rank2_cells(lib, DEV)


def test_one_step_vs_oracle_qm9_b64(lib):
    """Bigger, ragged batch (realistic QM9 node-count mix) against the oracle on the same draws."""
    pc.case_one_step_vs_oracle_large("ccsd_qm9_CC", lib, DEV, 64, [9, 9, 9, 8, 9, 7, 9, 9, 6, 9, 5, 9, 4, 9, 3, 2],
                                     "Reverse", "Langevin", 0.2, 0.7)


def test_one_step_vs_oracle_qm9_full_batch(lib):
    """The BASELINE batch itself (B = 1024: four co-resident workgroups per CU in k_xa, two rounds of k_r2, ScoreNetworkX on the
    idle wave) for one full PC step against the oracle on the same draws -- not only through size-independent properties."""
    pc.case_one_step_vs_oracle_large("ccsd_qm9_CC", lib, DEV, 1024, [9, 9, 8, 9, 7, 9, 9, 6, 9, 5, 9, 9, 4, 9, 8, 9, 3, 9, 7, 2, 9, 1],
                                     "Reverse", "Langevin", 0.2, 0.7, seed=11)


def test_one_step_vs_oracle_community_small_cc_b4(lib):
    pc.case_one_step_vs_oracle_large("ccsd_community_small_CC", lib, DEV, 4, [20, 12, 16, 18], "Euler", "Langevin", 0.05, 0.7)


def test_one_step_vs_oracle_edge_batches(lib):
    """Single-complex batch; a batch holding an empty graph (all flags 0), a 1-node and a 2-node graph (no rank-2 cell fits:
    d_min = 3)."""
    pc.case_one_step_vs_oracle_large("ccsd_qm9_CC", lib, DEV, 1, [7], "Reverse", "Langevin", 0.2, 0.7)
    pc.case_one_step_vs_oracle_large("ccsd_qm9_CC", lib, DEV, 5, [9, 0, 1, 2, 3], "Euler", "Langevin", 0.2, 0.7, seed=8)


def test_one_step_vs_oracle_base_cc(lib):
    """ScoreNetworkA_Base_CC checkpoints on ragged batches: qm9 (fused rank-2 kernel, block-weight ScoreNetworkF path) and
    community_small (tiled kernels, row-chunked HodgeBaselineLayer, 20-wide ScoreNetworkF head)."""
    pc.case_one_step_vs_oracle_large("ccsd_qm9_Base_CC", lib, DEV, 32, [9, 8, 9, 7, 6, 9, 5, 4], "Reverse", "Langevin", 0.2, 0.7)
    pc.case_one_step_vs_oracle_large("ccsd_community_small_Base_CC", lib, DEV, 3, [20, 13, 17], "Euler", "Langevin", 0.05, 0.7)


def test_full_size_qm9_philox_properties(lib):
    """BASELINE size (B=1024) for a few steps: size-independent properties of the state."""
    import numpy as np

    from ccsd_amd import loader, solver
    from oracle import ccsd_oracle as O
    from tests.helpers import load_ckpt_np

    meta, parts = load_ckpt_np("ccsd_qm9_CC")
    cfg = meta["config"]
    B, N, F = 1024, 9, 4
    rs = np.random.RandomState(42)
    counts = rs.choice([9, 8, 7, 6, 5, 4, 3, 2], size=B, p=np.array([10949, 1757, 294, 60, 15, 5, 1, 1]) / 13082.0)
    flags = torch.zeros(B, N)
    for b, c in enumerate(counts):
        flags[b, :c] = 1
    names = ["x", "adj", "rank2"]
    ms = [loader.load_model_from_ckpt(meta[f"params_{p}"], parts[p], DEV) for p in names]
    sd = [loader.load_sde(cfg["sde"][p]) for p in names]
    fn = solver.get_pc_sampler(sde_x=sd[0], sde_adj=sd[1], sde_rank2=sd[2], shape_x=(B, N, F), shape_adj=(B, N, N),
                               shape_rank2=(B, 36, 466), predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7,
                               n_steps=1, continuous=True, denoise=True, eps=1e-4, device=DEV, is_cc=True, d_min=3, d_max=9,
                               rng="philox", seed=42, max_steps=5, lib=lib)
    x, adj, rank2, nfe, traj = fn(*ms, flags.to(DEV))
    x, adj, rank2 = x.cpu(), adj.cpu(), rank2.cpu()
    assert nfe == 2000 and traj == []
    for t in (x, adj, rank2):
        assert torch.isfinite(t).all()
    assert torch.equal(x, O.mask_x(x, flags)) and torch.equal(adj, O.mask_adjs(adj, flags))
    assert torch.equal(rank2, O.mask_rank2(rank2, 9, 3, 9, flags))
    assert torch.allclose(adj, adj.transpose(-1, -2), atol=1e-5)
    # the state after 5 of 1000 VE steps is still prior-dominated: unit-ish scale on the live entries
    live = rank2[flags.sum(1) == 9]
    assert 0.5 < live.std().item() < 2.0


@pytest.mark.parametrize("env", [{"CCSD_NO_FUSED_R2": "1"}, {"CCSD_XA_PASS": "1"}, {"CCSD_XA_PASS": "2"}, {"CCSD_NO_FUSED_APPLY": "1"},
                                 {"CCSD_XA_GCH": "1"}])
def test_alternative_kernel_paths_qm9(lib, env, monkeypatch):
    """qm9_CC normally takes the fused LDS-resident rank-2 kernel and the 4-workgroups/CU graph-network layout; force the
    general tiled rank-2 kernels, the LDS-staged-weights variant and the 3/CU layout through the same parity cases."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pc.case_forward_vs_reference_golden("ccsd_qm9_CC", lib, DEV)
    pc.case_pc_sampler_identical_seed("ccsd_qm9_CC", "ccsd_qm9_CC", "k10", lib, DEV)
    pc.case_philox_properties(lib, DEV)


@pytest.mark.parametrize("threads", ["256", "512"])
def test_k_xa_thread_count_is_a_speed_matter_only(lib, threads, monkeypatch):
    """launch_xa gives a graph 1024 / 512 / 256 threads by batch (small test batches: 1024).  Any other count must reproduce the
    reference goldens the same way (per-sample norm sums re-associate, nothing else changes): the large-graph baked instance (zinc250k),
    the general instance behind the ENZYMES S4 sampler and a tiled-path CC checkpoint, with CCSD_XA_THREADS forcing the count."""
    monkeypatch.setenv("CCSD_XA_THREADS", threads)
    pc.case_pc_sampler_identical_seed("gdss_zinc250k", "gdss_zinc250k", "k5", lib, DEV)
    pc.case_pc_sampler_identical_seed("s4_ccsd_enzymes_small_CC", "ccsd_enzymes_small_CC", "n1000_first2", lib, DEV)
    pc.case_pc_sampler_identical_seed("ccsd_community_small_CC", "ccsd_community_small_CC", "k5", lib, DEV)
    pc.case_forward_vs_reference_golden("gdss_community_small", lib, DEV)


def test_full_size_community_small_cc_philox_properties(lib):
    """BASELINE configs[1] size (community_small_CC, B=512, E=190, K=1140: the tiled rank-2 kernels) for a few steps:
    size-independent properties of the state."""
    import numpy as np

    from ccsd_amd import loader, solver
    from oracle import ccsd_oracle as O
    from tests.helpers import load_ckpt_np

    meta, parts = load_ckpt_np("ccsd_community_small_CC")
    cfg = meta["config"]
    B, N, F = 512, 20, cfg["data"]["max_feat_num"]
    rs = np.random.RandomState(12)
    counts = rs.choice([12, 14, 16, 18, 20], size=B, p=np.array([29, 14, 23, 25, 9]) / 100.0)
    flags = torch.zeros(B, N)
    for b, c in enumerate(counts):
        flags[b, :c] = 1
    names = ["x", "adj", "rank2"]
    ms = [loader.load_model_from_ckpt(meta[f"params_{p}"], parts[p], DEV) for p in names]
    sd = [loader.load_sde(cfg["sde"][p]) for p in names]
    E, K = 190, 1140
    fn = solver.get_pc_sampler(sde_x=sd[0], sde_adj=sd[1], sde_rank2=sd[2], shape_x=(B, N, F), shape_adj=(B, N, N),
                               shape_rank2=(B, E, K), predictor="Euler", corrector="Langevin", snr=0.05, scale_eps=0.7,
                               n_steps=1, continuous=True, denoise=True, eps=1e-4, device=DEV, is_cc=True, d_min=3, d_max=3,
                               rng="philox", seed=12, max_steps=3, lib=lib)
    x, adj, rank2, nfe, traj = fn(*ms, flags.to(DEV))
    again = fn(*ms, flags.to(DEV))                       # second call of the closure: fresh draws
    assert not torch.equal(again[2], rank2)
    x, adj, rank2 = x.cpu(), adj.cpu(), rank2.cpu()
    assert nfe == 2000 and traj == []
    for t in (x, adj, rank2):
        assert torch.isfinite(t).all()
    assert torch.equal(x, O.mask_x(x, flags)) and torch.equal(adj, O.mask_adjs(adj, flags))
    fl, fr = O.rank2_flags(flags, N, 3, 3)
    assert torch.equal(rank2, rank2 * fl[:, :, None] * fr[:, None, :])
    assert torch.allclose(adj, adj.transpose(-1, -2), atol=1e-5)
    assert (adj.diagonal(dim1=-2, dim2=-1) == 0).all()
    live = rank2[flags.sum(1) == 20]
    assert 0.5 < live.std().item() < 2.0                 # 3 of 1000 VP steps: still prior-dominated


def test_ccsd_api_yaml_surface_on_gpu(lib, tmp_path):
    """CCSD(type="sample", config=<yaml>).run()-equivalent flow on the HIP path.  (i) qm9_CC (Reverse + Langevin, divide_batch = 2)
    with identical seeds against the oracle: float outputs and the quantised / relabelled / one-hot integer outputs; (ii) the
    same config with the production Philox noise and the shipped ENZYMES_small_CC config (S4 solver, EMA weights): properties."""
    from tests import test_harness as H

    cfg = dict(H.QM9_CC_YAML, sample=dict(H.QM9_CC_YAML["sample"], n_samples=32))
    pc.case_harness_vs_oracle(lib, tmp_path, "sample_qm9_CC_parity", cfg, "ccsd_qm9_CC", max_steps=12)
    out, c = H.run_harness(tmp_path, lib, None, "sample_qm9_CC", dict(H.QM9_CC_YAML, sample=dict(H.QM9_CC_YAML["sample"], n_samples=64)),
                           max_steps=20)
    assert out["adj"].is_cuda and out["adj"].shape == (64, 9, 9) and out["rank2"].shape == (64, 36, 466)
    assert torch.isfinite(out["rank2"]).all() and set(out["adj_int"].unique().tolist()) <= {0, 1, 2, 3}
    fl = out["flags"]
    assert torch.equal(out["adj"], out["adj"] * fl[:, :, None] * fl[:, None, :])
    # the two divide_batch chunks draw different noise (equal-flag samples of chunk 0 and chunk 1 are not copies)
    half = out["rank2"].shape[0] // 2
    a, b = out["rank2"][:half].flatten().double().cpu(), out["rank2"][half:].flatten().double().cpu()
    corr = ((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std())
    assert abs(corr.item()) < 0.05, f"divide_batch chunks are correlated: {corr.item():.3f}"
    out, c = H.run_harness(tmp_path, lib, None, "sample_enzymes_small_CC", H.ENZYMES_YAML, max_steps=10, rounds=1)
    assert out["adj"].shape[1:] == (12, 12) and torch.isfinite(out["rank2"]).all()
    H.check_flags_against_reference_golden(out, "ENZYMES_small", 42, 64)      # (f)2: the reference's own init_flags


def test_kat_hodge_layers_three_and_four(lib):
    pc.case_kat_hodge_layers(lib, DEV)


def test_kat_hodge_general_stack(lib):
    pc.case_kat_hodge_general(lib, DEV)


def test_production_loop_vs_oracle_qm9_full_batch(lib):
    """What bench.py times, at the BASELINE batch (B = 1024, realistic node-count mix): ccsd_sampler_run with in-kernel Philox
    and the Langevin apply fused into the predictor launches, eight PC steps (seven merged k_r2 launches), against the oracle
    replaying the exported draws -- plus bit equality with the step-wise loop at the same batch."""
    pc.case_production_loop_vs_oracle("ccsd_qm9_CC", lib, DEV, 1024, [9, 9, 8, 9, 7, 9, 9, 6, 9, 5, 9, 9, 4, 9, 8, 9, 3, 9, 7, 2, 9, 1],
                                      8, "Reverse", "Langevin", 0.2, 0.7, seed=17, expect_fused=True)


def test_production_loop_vs_oracle_community_small_cc_full_batch(lib):
    """BASELINE configs[1] at its own batch (community_small_CC, B = 512, the dataset's node-count mix): the tiled rank-2 kernels with
    the corrector riding on the projection passes, k_xa on 512 threads per graph -- two PC steps of ccsd_sampler_run against the oracle
    on the exported draws, and bit equality with the step-wise loop."""
    pc.case_production_loop_vs_oracle("ccsd_community_small_CC", lib, DEV, 512, [12] * 29 + [14] * 14 + [16] * 23 + [18] * 25 + [20] * 9,
                                      2, "Euler", "Langevin", 0.05, 0.7, seed=29, expect_fused=True)


def test_production_loop_vs_oracle_tiled_path(lib):
    """The same for the tiled rank-2 kernels (community_small_CC: E = 190, K = 1140) and for a graph-only checkpoint."""
    pc.case_production_loop_vs_oracle("ccsd_community_small_CC", lib, DEV, 6, [20, 12, 16, 18, 14, 20], 3, "Euler", "Langevin", 0.05, 0.7,
                                      seed=19)
    pc.case_production_loop_vs_oracle("gdss_community_small", lib, DEV, 16, [20, 12, 16, 18, 14], 3, "Euler", "Langevin", 0.05, 0.7,
                                      seed=23)


def test_production_loop_edge_flags(lib):
    """Edge cases of the flags (init_flags can draw any node count 1..N; 0 = an EMPTY complex is what the masks make of a padded
    batch slot): complexes with no node, one node (no edge, no cell), two nodes (one edge, no cell of rank 2) beside full ones, and a
    batch of ONE -- the production loop against the oracle on the exported draws, and bit equality with the step-wise loop."""
    pc.case_production_loop_vs_oracle("ccsd_qm9_CC", lib, DEV, 7, [0, 1, 2, 9, 3, 0, 9], 3, "Reverse", "Langevin", 0.2, 0.7, seed=31)
    pc.case_production_loop_vs_oracle("ccsd_qm9_CC", lib, DEV, 1, [5], 2, "Reverse", "Langevin", 0.2, 0.7, seed=37)
    # the one-workgroup-per-complex rank-2 kernels (B >= 256) with empty and near-empty complexes among full ones
    pc.case_production_loop_vs_oracle("ccsd_community_small_CC", lib, DEV, 256, [0, 1, 2, 20, 12, 3, 20, 16], 1, "Euler", "Langevin", 0.05, 0.7,
                                      seed=41, expect_fused=True)


QM9_MIX = [9, 9, 8, 9, 7, 9, 9, 6, 9, 5, 9, 9, 4, 9, 8, 9, 3, 9, 7, 2, 9, 1]
ENZ_MIX = [12, 11, 12, 9, 10, 12, 8, 12, 6, 12, 11, 5, 12, 10, 3, 12, 7]
EGO_MIX = [18, 17, 18, 12, 18, 9, 16, 18, 5, 18, 14, 2, 18, 11, 18, 7]
# the route the ego_small_CC plan takes (ccsd_plan_query): the tiled rank-2 kernels (k_gemm_h*, k_gemm_p*, k_hf_score), not k_r2 / k_ew1
EGO_ROUTE = {"fused_r2": 0, "ew1": 0, "fused_loop": 0}


def test_production_loop_corrector_free_qm9_full_batch(lib):
    """ccsd_sampler_run's predictor-only branch (corrector None) at the headline geometry (qm9_CC, B = 1024) against the oracle on the
    exported predictor draws: result, final state, and bit equality with the step-wise loop."""
    pc.case_production_loop_vs_oracle("ccsd_qm9_CC", lib, DEV, 1024, QM9_MIX, 4, "Euler", "None", 0.0, 0.0, seed=71, expect_fused=False)


def test_production_loop_corrector_free_traj(lib):
    """The same branch on a short run with the trajectory kept (ccsd_sampler_run's traj slots)."""
    pc.case_production_loop_vs_oracle("ccsd_qm9_CC", lib, DEV, 9, [9, 7, 8, 0, 4, 9, 1, 2, 6], 3, "Euler", "None", 0.0, 0.0, seed=73,
                                      keep_traj=True)
    pc.case_production_loop_vs_oracle("ccsd_qm9_CC", lib, DEV, 9, [9, 7, 8, 0, 4, 9, 1, 2, 6], 3, "S4", "None", 0.15, 0.7, seed=79,
                                      keep_traj=True)


def test_production_loop_s4_enzymes_small_cc_chunk(lib):
    """ccsd_sampler_run's S4 branch at the ENZYMES_small_CC YAML's chunk batch (cc_nb_eval 1000 / divide_batch 4 = 250)."""
    pc.case_production_loop_vs_oracle("ccsd_enzymes_small_CC", lib, DEV, 250, ENZ_MIX, 2, "S4", "None", 0.15, 0.7, seed=83, expect_fused=False)


def test_production_loop_s4_enzymes_small_base_cc(lib):
    """S4 with the ScoreNetworkA_Base_CC checkpoint of the same dataset (sample_enzymes_small_Base_CC.yaml)."""
    pc.case_production_loop_vs_oracle("ccsd_enzymes_small_Base_CC", lib, DEV, 250, ENZ_MIX, 2, "S4", "None", 0.15, 0.7, seed=89)


def test_production_loop_corrector_free_gdss_ego_small_retrained(lib):
    """Euler + None (sample_ego_small_retrained.yaml) on the graph-only ego_small checkpoint, N = 18."""
    pc.case_production_loop_vs_oracle("gdss_ego_small_retrained", lib, DEV, 250, EGO_MIX, 3, "Euler", "None", 0.0, 0.0, seed=97)


def test_production_loop_ego_small_cc_chunk(lib):
    """ego_small_CC (N = 18, d 3..5: E = 153, K = 12444, 7.6 MB of rank-2 state per complex) at its YAML's chunk batch, B = 250, Euler +
    None.  The oracle replays eight rows (b = 0, b = B - 1, mixed node counts): with corrector None no batch-mean norm couples the
    complexes, so each row of the batch evolves from its own prior, score and draws alone."""
    pc.case_production_loop_vs_oracle("ccsd_ego_small_CC", lib, DEV, 250, EGO_MIX, 2, "Euler", "None", 0.0, 0.0, seed=101,
                                      subset=[0, 3, 5, 8, 11, 100, 131, 249], expect_route=EGO_ROUTE)


def test_production_loop_ego_small_cc_beyond_4gib(lib):
    """The same loop at B = 600: one rank-2 state tensor is 4.6 GB, so every per-batch byte offset of the rank-2 kernels, the Philox
    draw kernels and the state copies passes 2^32 for the last complexes.  The oracle replays the last rows, rows just below and
    straddles the 2^32-byte boundary (b = 563; b = 564 is the first whose rank-2 block starts past it) and a middle one."""
    B = 600
    per = 153 * 12444 * 4
    assert 563 * per < 2 ** 32 < 564 * per
    pc.case_production_loop_vs_oracle("ccsd_ego_small_CC", lib, DEV, B, EGO_MIX, 2, "Euler", "None", 0.0, 0.0, seed=103,
                                      subset=[0, 300, 562, 563, 564, 598, 599], expect_route=EGO_ROUTE, stepwise=False)


def test_fused_r2_serves_nonaffine_shapes(lib):
    pc.case_fused_r2_nonaffine_shapes(lib, DEV)


def test_rccl_single_rank_group(lib):
    """First contact with RCCL on one GPU: the code an 8-GPU run takes -- init_process_group("nccl", device_id=...) in
    ccsd_amd.distributed.init, all_gather_into_tensor on device tensors in all_gather_samples, the 6-float all-reduce of the
    exact mode inside the step-wise loop -- executed on a 1-rank group (world_size 1 exercises the same calls; only the
    transport between ranks stays untested).  The sharded closure with exact=True must reproduce the plain closure bit for bit."""
    import os

    import torch.distributed as dist

    from ccsd_amd import distributed, loader
    from tests.helpers import load_ckpt_np

    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("LOCAL_RANK", "0")
    rank, world, dev = distributed.init(force_group=True, timeout_s=120)
    try:
        assert (rank, world, dev) == (0, 1, DEV) and dist.get_backend() == "nccl"
        ts = [torch.arange(24, device=DEV, dtype=torch.float32).view(4, 6), None, torch.randn(4, 3, 5, device=DEV)]
        out = distributed.all_gather_samples(ts, force=True)              # dist.all_gather_into_tensor over RCCL
        assert out[1] is None and torch.equal(out[0], ts[0]) and torch.equal(out[2], ts[2]) and out[0].data_ptr() != ts[0].data_ptr()
        sums = torch.arange(8, device=DEV, dtype=torch.float32)
        dist.all_reduce(sums)
        assert torch.equal(sums.cpu(), torch.arange(8, dtype=torch.float32))
        # the sharded seam on the 1-rank group, exact mode (all-reduce of the norm sums every corrector half-step, step-wise loop)
        meta, parts = load_ckpt_np("ccsd_qm9_CC")
        cfgt = loader.AttrDict(meta["config"])
        B = 16
        module = dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1)
        sample = dict(n_samples=B, probability_flow=False, noise_removal=True, eps=1e-4)
        names = ["x", "adj", "rank2"]
        ms = [loader.load_model_from_ckpt(meta[f"params_{p}"], parts[p], DEV) for p in names]
        from tests.helpers import make_flags

        flags = make_flags(B, 9, [9, 8, 9, 7, 5]).to(DEV)
        kw = dict(is_cc=True, d_min=3, d_max=9, rng="philox", seed=3, max_steps=3, lib=lib)
        sharded = distributed.load_sampling_fn_sharded(cfgt, module, sample, DEV, exact=True, **kw)
        assert hasattr(sharded, "inner"), "the 1-rank group did not take the sharded route"
        plain = loader.load_sampling_fn(cfgt, module, sample, DEV, **kw)
        a, b = sharded(*ms, flags), plain(*ms, flags)
        for p, u, v in zip(names, a[:3], b[:3]):
            assert torch.equal(u, v), f"1-rank exact mode != single-process run for {p}"
    finally:
        dist.destroy_process_group()


def test_zinc5b_production_loop_vs_oracle(lib):
    pc.case_zinc5b_production_loop(lib, DEV)


def test_one_workgroup_per_complex_kernels_bitwise(lib):
    """community_small_CC at B = 512: k_gemm_h_full / k_hp_full (one workgroup per complex, F streamed once) against the 64 x 64 tile
    kernels and the two-kernel predictor pass they replace, and the norms-pass form of k_hp_full (off by default) -- bit for bit."""
    pc.case_env_switches_bitwise(lib, DEV, [{"CCSD_NO_HP_FULL": "1"}, {"CCSD_NO_H_FULL": "1"}, {"CCSD_HP_FULL_NORMS": "1"},
                                            {"CCSD_NO_MLP_WT": "1"}])       # (the last: the block_linear MLPs on the untransposed weights)


def test_split_precision_experiment_error_bound(lib):
    """EXPERIMENT (CCSD_SPLIT_BF16=3, never the default): H = F F^T of the norms pass as three bf16 MFMA terms with fp32 accumulation
    (k_gemm_h_full<., ., 2>).  Per product the dropped terms are <= (2^-14 + 2^-15) |a b| (split_frag, ccsd_k_rank2.h); measured on
    community_small_CC at B = 512: the rank-2 score moves by a few 1e-6 of its scale.  Held here to 2e-5 (score) and to the parity
    tolerance 1e-4 on a 10-step trajectory against the exact-fp32 plan."""
    pc.case_split_precision(lib, DEV)


def test_geometry_instances_match_runtime_geometry_bitwise(lib):
    """k_xa<false, XA_PLAIN9> / k_r2<3, 1, true, false, QM9> == the run-time-geometry instances, bit for bit (production loop + scores)."""
    # the geometry-only instances k_xa<false, XA_PLAIN9> / k_r2<3, 1, true, false, 1> (CCSD_NO_BAKE keeps the plan off the baked ones)
    pc.case_geometry_instances_bitwise(lib, DEV, snr=0.25, expect=(4, 0), no_bake=True)
    # the bench line's configuration: the plan's architecture bytes equal the baked ones -- k_xa<false, XA_BAKED9> /
    # k_r2<3, 1, true, false, 2>, every plan field a compile-time constant
    pc.case_geometry_instances_bitwise(lib, DEV, B=1024, steps=3, expect=(7, 0))
    # baked instances are keyed on the ARCHITECTURE only: other sampler settings of the shipped network (snr, scale_eps, the shipped
    # YAML's chunk of 2500 falls into the same batch bucket) select the same instance ...
    pc.case_geometry_instances_bitwise(lib, DEV, B=1024, steps=2, snr=0.25, scale_eps=0.9, expect=(7, 0))
    # ... and CCSD_NO_BAKE holds it to the geometry-only instance of the same source
    pc.case_geometry_instances_bitwise(lib, DEV, B=1024, steps=2, expect=(4, 0), no_bake=True)
    # k_xa<true, XA_BAKED20> (community_small_CC, B = 512: channel stack in HBM, five AttentionLayers unrolled) at the shipped and at
    # another snr; k_xa<true, XA_PLAIN20> (geometry only) against k_xa<true, XA_PLAIN>
    pc.case_geometry_instances_bitwise(lib, DEV, B=512, steps=2, name="ccsd_community_small_CC", counts=(20, 12, 16, 18, 14, 20), expect=(8, 0),
                                       predictor="Euler", snr=0.05)
    pc.case_geometry_instances_bitwise(lib, DEV, B=512, steps=2, name="ccsd_community_small_CC", counts=(20, 12, 16, 18, 14, 20), expect=(8, 0),
                                       predictor="Euler", snr=0.06)
    pc.case_geometry_instances_bitwise(lib, DEV, B=512, steps=2, name="ccsd_community_small_CC", counts=(20, 12, 16, 18, 14, 20), expect=(5, 0),
                                       predictor="Euler", snr=0.05, no_bake=True)
    # qm9_Base_CC: k_xa stays the run-time-plan HodgeBaseline instance (1, 1); its non-affine k_r2 runs with the qm9 geometry compiled in
    pc.case_geometry_instances_bitwise(lib, DEV, B=64, steps=2, name="ccsd_qm9_Base_CC", expect=(1, 1))
    # zinc250k (graph-only, N = 38, batch 256): k_xa<true, XA_BAKED38>;  ENZYMES_small_CC (S4 sampler, batch 64): k_xa<false, XA_BAKEDENZ>
    # (the general variant, baked) and the (66, 715) instances of the tiled rank-2 kernels
    wz, we = bench.WORKLOADS["zinc250k"], bench.WORKLOADS["enzymes_small_CC"]
    pc.case_geometry_instances_bitwise(lib, DEV, B=256, steps=2, name="gdss_zinc250k", counts=(38, 30, 24, 36, 20), expect=(9, 0),
                                       predictor=wz["predictor"], corrector=wz["corrector"], snr=wz["snr"], scale_eps=wz["scale_eps"])
    pc.case_geometry_instances_bitwise(lib, DEV, B=64, steps=2, name="ccsd_enzymes_small_CC", counts=(12, 10, 8, 11, 6), expect=(10, 3),
                                       predictor=we["predictor"], corrector=we["corrector"], snr=we["snr"], scale_eps=we["scale_eps"])
