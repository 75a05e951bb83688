"""CPU suite for the tiled graph-network route of one-hodge-layer combinatorial complexes (k_lg_hodge1; ccsd_amd/csrc/ccsd_k_lg.h):
the planner, the host emulation of the route against the oracle and against k_xa, and the oracle against the reference goldens of
ccsd_grid_small_CC.  (The rank-2 networks at that checkpoint's own geometry take minutes on the emulation: GPU suite.)"""
import numpy as np
import pytest
import torch

from oracle import ccsd_oracle as O
from tests import cc_large_graph_cases as cc
from tests import test_oracle_golden as OG
from tests.emu_util import emu_library
from tests.helpers import load_ckpt_np, load_golden, rng_matches

torch.set_num_threads(8)
DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_emu_forced_route_community_small_cc(lib, monkeypatch):
    """Tiled rank-2 family: x, adj and rank2 at B = 3 with a full, a partial and a two-node complex."""
    cc.case_forced_vs_xa("ccsd_community_small_CC", lib, DEV, [20, 11, 2], ["x", "adj", "rank2"], monkeypatch)


def test_emu_forced_route_zinc5b(lib, monkeypatch):
    """k_ew1 family (N = 38, E = 703, K = 8436): adj and x."""
    cc.case_forced_vs_xa("zinc250k_CC_5b", lib, DEV, [38, 9], ["adj", "x"], monkeypatch)


def test_planner_crossover(lib, monkeypatch):
    cc.case_crossover_selection(lib, DEV, monkeypatch)


def test_emu_crossover_forwards(lib):
    cc.case_crossover_forwards(lib, DEV)


@pytest.mark.parametrize("predictor,corrector,snr,seps", [("Reverse", "Langevin", 0.1, 0.7), ("S4", "None", 0.15, 0.7),
                                                          ("Euler", "None", 0.0, 0.0)])
def test_emu_forced_production_loop(lib, monkeypatch, predictor, corrector, snr, seps):
    cc.case_forced_production_loop(lib, DEV, predictor, corrector, snr, seps, monkeypatch)


def test_emu_forced_nsteps2_library_vs_stepwise(lib, monkeypatch):
    cc.case_forced_nsteps2(lib, DEV, monkeypatch)


def test_planner_rejections(lib, monkeypatch):
    cc.case_planner_rejections(lib, DEV, monkeypatch)


# ---- the oracle against the reference's ccsd_grid_small_CC outputs (bit for bit where the fixtures were made; OG._close's 2e-5 on
# ---- another host CPU for the arrays stored whole)
def _nets():
    meta, parts = load_ckpt_np(cc.GRID)
    assert meta["ema_applied"] is True and set(meta["ema_params"]) == set(cc.NAMES)
    nets = [(lambda x, a, r, f, p=p: O.run_network(meta[f"params_{p}"], parts[p], x, a, r, f)) for p in cc.NAMES]
    return meta, nets


def _check(out, g, key, what):
    """OG._check; for a summarised entry whose hash differs (another host CPU: sgemm blocking) the subsample and the row sums at the
    2e-5 the golden tests fall back to."""
    if key in g.files or str(g[f"{key}/sha256"]) == __import__("hashlib").sha256(np.ascontiguousarray(out).tobytes()).hexdigest():
        OG._check(out, g, key, what)
        return
    np.testing.assert_allclose(out.reshape(-1)[g[f"{key}/idx"]], g[f"{key}/val"], rtol=2e-5, atol=2e-5, err_msg=what)
    np.testing.assert_allclose(out.astype(np.float64).sum(-1), g[f"{key}/rowsum"], rtol=2e-5, atol=2e-5 * out.shape[-1], err_msg=what)


@pytest.mark.parametrize("tag,scale", [("unit", 1.0), ("small", 0.3)])
def test_oracle_vs_reference_g1_grid_small_cc(tag, scale):
    g = load_golden(f"g1_{cc.GRID_GOLDEN}.npz")
    assert rng_matches(g)
    meta, nets = _nets()
    N, F, d_min, d_max = cc.dims(meta)
    flags = torch.from_numpy(g["flags"])
    x, adj, rank2 = OG.masked_state(int(g["seed"]), flags.shape[0], N, F, True, d_min, d_max, flags, scale)
    assert np.array_equal(x.numpy(), g[f"{tag}/x"]) and np.array_equal(adj.numpy(), g[f"{tag}/adj"])
    with torch.no_grad():
        for p, net in zip(cc.NAMES, nets):
            _check(net(x, adj, rank2, flags).numpy(), g, f"{tag}/net_{p}", f"grid_small_CC {tag} net_{p}")
        if tag == "unit":
            for ti, tval in enumerate([1.0, 0.5, 1e-4]):
                for p, net in zip(cc.NAMES[:2], nets):
                    out = O.make_score_fn(O.load_sde(meta["config"]["sde"][p]), net)(x, adj, rank2, flags, torch.ones(flags.shape[0]) * tval)
                    _check(out.numpy(), g, f"unit/score_{p}_t{ti}", f"grid_small_CC score_{p} t{ti}")


def test_oracle_vs_reference_g5_grid_small_cc():
    """The first two steps of the shipped 1000-scale sampler (Reverse + Langevin, snr 0.1, scale_eps 0.7) at B = 2."""
    g = load_golden(f"g5_{cc.GRID_GOLDEN}.npz")
    assert rng_matches(g)
    case = "n1000_first2"
    fn, nets, flags, parts = OG.oracle_sampler_from_golden(g, cc.GRID, case)
    torch.manual_seed(int(g["seed"]))
    res = fn(*nets, flags)
    for p, v in zip(parts, res):
        _check(v.numpy(), g, f"{case}/{p}", f"grid_small_CC {case} {p}")
    assert int(res[len(parts)]) == int(g[f"{case}/nfe"]) and len(res[-1]) == int(g[f"{case}/traj_len"])
    OG._close(res[-1][-1][1].numpy(), g[f"{case}/traj_last_adj"])
    assert np.array_equal(O.quantize(res[1]).numpy(), g[f"{case}/quantize_adj"])
    q = O.quantize(res[2]).numpy().astype(np.uint8)
    if str(g[f"{case}/quantize_rank2/sha256"]) == __import__("hashlib").sha256(q.tobytes()).hexdigest():
        OG._check(q, g, f"{case}/quantize_rank2", "quantize_rank2", exact=True)
    else:       # (another host CPU: cells whose value sits on the threshold may flip)
        assert (q.reshape(-1)[g[f"{case}/quantize_rank2/idx"]] != g[f"{case}/quantize_rank2/val"]).mean() < 1e-4
