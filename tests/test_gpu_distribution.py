"""GPU (-m gpu): the first end-to-end comparison of the production loop -- in-kernel Philox noise, fused corrector, all 1000 steps of
the shipped qm9_CC set-up through ccsd_sampler_run, then finish() -- with the reference, in distribution (tests/distribution_cases.py).
1024 complexes with the fixture's 256 flag rows tiled four times, so that both samples have the same node-count mix."""
import pytest
import torch

from tests import distribution_cases as dc
from tests.helpers import load_ckpt_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261018


def test_production_loop_matches_the_reference_in_distribution(capsys):
    from ccsd_amd import loader, solver

    d, meta = dc.fixture()
    ck, parts = load_ckpt_np("ccsd_qm9_CC")
    cfg = ck["config"]
    N, F, d_min, d_max = cfg["data"]["max_node_num"], cfg["data"]["max_feat_num"], meta["d_min"], meta["d_max"]
    names = ["x", "adj", "rank2"]
    B = 1024
    flags = torch.from_numpy(d["flags"]).repeat(4, 1).to(DEV)
    models = [loader.load_model_from_ckpt(ck[f"params_{p}"], parts[p], DEV) for p in names]
    sdes = [loader.load_sde(cfg["sde"][p]) for p in names]
    assert sdes[1].N == meta["num_scales"] == 1000
    from ccsd_amd.plan import rank2_dim

    E, K = rank2_dim(N, d_min, d_max)
    smp = meta["sampler"]
    fn = solver.get_pc_sampler(sde_x=sdes[0], sde_adj=sdes[1], sde_rank2=sdes[2], shape_x=(B, N, F), shape_adj=(B, N, N),
                               shape_rank2=(B, E, K), predictor=smp["predictor"], corrector=smp["corrector"], snr=smp["snr"],
                               scale_eps=smp["scale_eps"], n_steps=smp["n_steps"], probability_flow=False, continuous=True,
                               denoise=meta["denoise"], eps=meta["eps"], is_cc=True, d_min=d_min, d_max=d_max, device=DEV,
                               rng="philox", seed=SEED)
    x, adj, rank2 = fn(*models, flags)[:3]
    torch.cuda.synchronize()
    assert torch.isfinite(adj).all() and torch.isfinite(rank2).all()
    from ccsd_amd import _lib
    from tests.helpers import sample_ops

    res = sample_ops(_lib.get_library(), DEV).finish(x, adj, rank2, flags, mol=True, d_min=d_min, d_max=d_max, dense_rank2=False,
                                                     dense_adj=False)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    got["cell_hist"] = got["rank2_cell_hist"]
    bins = dc.nonempty_bins(d)
    with capsys.disabled():
        dc.compare(dc.scalars(got, bins), dc.scalars(d, bins), "gpu(1024) vs ref(256)")
