"""Cases of ScoreNetworkA_CC hodge branches up to 8 channels wide, whose true MLPs (num_linears_h >= 2) have hidden Linears 9 to 16 wide
("wide" plans: k_lg_hodge1_w / k_lg_hd_diag_w in ccsd_amd/csrc/ccsd_k_lg.h, k_gemm_p_w / k_hodge_value_w in ccsd_k_rank2.h), shared by the
CPU suite (host emulation, tests/test_hodge_wide.py) and the GPU suite (tests/test_gpu_hodge_wide.py).  Every comparison takes
parity_cases.assert_close at its default tolerance.

kat_hodge_wide.npz (tools/make_golden.py kat_hodge_wide; the N = 12 tag lies in kat_hodge_wide.1.npz, as its "files" entry says) holds the
reference constructor's networks and outputs; arch_at (tests/hodge_stack_route_cases.py) builds the other networks, for which the oracle is the
specification."""
import json
import os

import numpy as np
import pytest
import torch

from ccsd_amd.engine import PCEngine
from oracle import ccsd_oracle as O
from tests import cc_large_graph_cases as cc
from tests import hodge_stack_route_cases as hs
from tests import library_loop_cases as ll
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np, load_golden, make_flags

NAMES = cc.NAMES
QM9, ENZ, GRID = hs.QM9, hs.ENZ, hs.GRID
WIDE = ["W1_n5", "W2_n6", "W2_n9", "W3_n12"]          # some Linear of the hodge MLPs is 10, 12 or 16 wide
SINGLE = "S2_n9"                                      # W2_n9's widths with single Linears: the widest Linear is 8
TAGS = WIDE + [SINGLE]
forced = hs.forced
_kat = {}


def kat():
    """{key: array} of both fixture files."""
    if not _kat:
        g = load_golden("kat_hodge_wide.npz")
        for fname in json.loads(str(g["files"])):
            z = load_golden(fname)
            _kat.update({k: z[k] for k in z.files})
    return _kat


def kat_tag(tag):
    """(params, state dict, flags, x, adj, rank2, reference output) of one tag."""
    g = kat()
    params = json.loads(str(g["meta"]))[tag]
    sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g if k.startswith(f"{tag}/w/")}
    return (params, sd) + tuple(torch.from_numpy(g[f"{tag}/{k}"]) for k in ("flags", "x", "adj", "rank2", "out"))


def kat_engine(params, sd, lib, device):
    return PCEngine(None, None, params, sd, None, None, N=params["max_node_num"], F=params["max_feat_num"], is_cc=True,
                    d_min=params["d_min"], d_max=params["d_max"], device=device, lib=lib)


# ---- 1. the oracle against the reference
def case_oracle_vs_reference(tag):
    """oracle.run_network reproduces the reference constructor's output, on the terms of test_kat_hodge_general_mlp_value
    (tests/test_oracle_golden.py::_close: bit for bit where the fixtures were made, else rtol = atol = 2e-5)."""
    params, sd, flags, x, adj, rank2, out = kat_tag(tag)
    w = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    with torch.no_grad():
        got = O.run_network(params, w, x, adj, rank2, flags)
    if not np.array_equal(got.numpy(), out.numpy()):
        np.testing.assert_allclose(got.numpy(), out.numpy(), rtol=2e-5, atol=2e-5, err_msg=tag)


# ---- 2. the kernels against the reference
def case_kat(tag, lib, device, monkeypatch):
    """A wide tag, unforced: the route, the tiled rank-2 family, no k_xa layout; the adj score against the reference's output."""
    forced(monkeypatch, False)
    params, sd, flags, x, adj, rank2, out = kat_tag(tag)
    eng = kat_engine(params, sd, lib, device)
    route = {k: eng.query(k) for k in ("h_wide", "large_graph", "r2_family", "xa_lds_bytes")}
    assert route == {"h_wide": 1, "large_graph": 1, "r2_family": 3, "xa_lds_bytes": 0}, f"{tag}: {route}"
    if tag == "W3_n12":
        assert eng.query("h_general") == 1
    got = eng.score(1, *(t.to(device) for t in (x, adj, rank2, flags)))
    pc.assert_close(got, out, f"kat_hodge_wide {tag}")
    cc.check_adj_masks(got, flags, tag)


def case_kat_single(lib, device, monkeypatch):
    """S2_n9 (single Linears, 8 channels: not wide): k_xa unforced, the route under CCSD_LARGE_GRAPH=2; both against the reference's
    output and against each other."""
    params, sd, flags, x, adj, rank2, out = kat_tag(SINGLE)
    args = [t.to(device) for t in (x, adj, rank2, flags)]
    got = []
    for force in (False, True):
        forced(monkeypatch, force)
        eng = kat_engine(params, sd, lib, device)
        assert eng.query("h_wide") == 0
        assert eng.query("large_graph") == int(force)
        got.append(eng.score(1, *args).cpu())
        pc.assert_close(got[-1], out, f"kat_hodge_wide {SINGLE}, {'forced onto the route' if force else 'k_xa'}")
        cc.check_adj_masks(got[-1], flags, SINGLE)
    forced(monkeypatch, False)
    pc.assert_close(got[1], got[0], f"kat_hodge_wide {SINGLE}: the route vs k_xa")


# ---- 3. edge flags
def case_edge_flags(lib, device, monkeypatch, counts=(9, 5, 2, 1, 0), seed=17):
    """The W2_n9 network on complexes with 9, 5, 2, 1 and 0 nodes in one batch, against the oracle."""
    forced(monkeypatch, False)
    params, sd = kat_tag("W2_n9")[:2]
    N, F, d_min, d_max = params["max_node_num"], params["max_feat_num"], params["d_min"], params["d_max"]
    flags = make_flags(len(counts), N, list(counts))
    state = pc.masked_state(seed, len(counts), N, F, True, d_min, d_max, flags)
    eng = kat_engine(params, sd, lib, device)
    assert eng.query("h_wide") == 1
    w = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    with torch.no_grad():
        want = O.run_network(params, w, *state, flags)
    got = eng.score(1, *(t.to(device) for t in state), flags.to(device))
    pc.assert_close(got, want, f"W2_n9 network, node counts {counts}")
    cc.check_adj_masks(got, flags, "W2_n9 edge flags")
    assert not got.cpu()[3:].any(), "complexes with one node and without nodes have no edges: the adj score is zero"


# ---- 4. all three networks: enzymes_small_CC.yaml's architecture with the hodge branch as wide as the graph branch
ENZ_WIDE = dict(c_hid_h=8, c_final_h=4)
ENZ_COUNTS = (12, 7, 2)


def enz_wide():
    return hs.arch_at(ENZ, 12, **ENZ_WIDE)


def case_enz_forwards(lib, device, monkeypatch, seed=9):
    """x, adj and rank2 forwards and the t = 0.5 score scaling against the oracle (hodge_stack_route_cases.case_natural_forwards' form)."""
    from ccsd_amd import loader

    forced(monkeypatch, False)
    meta, parts = enz_wide()
    Nn, F, d_min, d_max = cc.dims(meta)
    counts = ENZ_COUNTS
    flags = make_flags(len(counts), Nn, list(counts))
    state = pc.masked_state(seed, len(counts), Nn, F, True, d_min, d_max, flags)
    eng = cc.engine(meta, parts, lib, device)
    assert eng.query("h_wide") == 1 and eng.query("large_graph") == 1 and eng.query("r2_family") == 3
    args = [t.to(device) for t in state] + [flags.to(device)]
    want = cc.oracle_forwards(meta, parts, state, flags, NAMES)
    B = len(counts)
    for t, p in enumerate(NAMES):
        got = eng.score(t, *args)
        pc.assert_close(got, want[p], f"enzymes_small_CC, c_hid_h 8, net_{p}")
        if p == "adj":
            cc.check_adj_masks(got, flags, "enzymes_small_CC, c_hid_h 8")
        sde = loader.load_sde(meta["config"]["sde"][p])
        tt = torch.ones(B) * 0.5
        net = lambda x, a, r, f, p=p: O.run_network(meta[f"params_{p}"], parts[p], x, a, r, f)
        with torch.no_grad():
            wscore = O.make_score_fn(O.load_sde(meta["config"]["sde"][p]), net)(*state, flags, tt)
        ss = 1.0 if sde.kind == "VE" else float(-1.0 / sde.marginal_prob(torch.zeros(1, 1, 1), tt[:1])[1])
        pc.assert_close(eng.score(t, *args, ss), wscore, f"enzymes_small_CC, c_hid_h 8, score_{p} t=0.5")


# ---- 5. production loop on that plan
def case_production_loop(lib, device, predictor, corrector, snr, seps, monkeypatch, counts=(12, 7)):
    """cc.case_forced_production_loop without the forcing: ccsd_sampler_run against the oracle on the exported draws, two steps, and
    the step-wise driver bit for bit; the plan takes the un-fused loop form of its sampler."""
    forced(monkeypatch, False)
    loop = 3 if predictor == "S4" else 1 if corrector == "Langevin" else 0
    pc.case_production_loop_vs_oracle("enzymes_small_CC, c_hid_h 8", lib, device, 2, list(counts), 2, predictor, corrector, snr, seps,
                                      source=enz_wide(),
                                      expect_route={"h_wide": 1, "large_graph": 1, "loop_form": loop, "tiled_fuse": 0, "fused_loop": 0})


def case_nsteps2(lib, device, monkeypatch, counts=(12, 7)):
    """sampler.n_steps = 2 (Reverse + Langevin): the library loop == the step-wise driver, bit for bit (cc.case_forced_nsteps2
    without the forcing; library_loop_cases.Setup takes its networks through _source)."""
    forced(monkeypatch, False)
    monkeypatch.setattr(ll, "_source", lambda name: enz_wide())
    _, fn, _, _, _ = ll.case_nsteps_library_vs_stepwise("enzymes_small_CC, c_hid_h 8", lib, device, 2, list(counts), 2, "Reverse", 0.1, 0.7, 2)
    assert fn.engine().query("large_graph") == 1 and fn.engine().query("h_wide") == 1


# ---- 6. planner
def case_planner(lib, device, monkeypatch):
    def plan_only(ckpt, N, **over):
        meta, _ = hs.arch_at(ckpt, N, **over)
        return cc.engine(meta, None, lib, device, weights=False)

    for force in (False, True):
        forced(monkeypatch, force)
        with pytest.raises(NotImplementedError, match="hodge MLP wider than 16"):
            plan_only(QM9, 9, c_hid_h=9, c_final_h=4)
        with pytest.raises(NotImplementedError, match="hodge MLP wider than 16"):
            plan_only(QM9, 9, c_hid_h=9, c_final_h=4, num_linears_h=2)
        with pytest.raises(NotImplementedError, match="hodge MLPs wider than 8 need the tiled graph-network route.*hodge attention dimensions above 16"):
            plan_only(QM9, 9, c_hid_h=8, c_final_h=4, num_linears_h=2, adim_h=20)
        with pytest.raises(NotImplementedError, match="hodge MLPs wider than 8 need the tiled graph-network route.*two or more layers"):
            plan_only(GRID, 39, num_layers_h=2, c_hid_h=8, c_final_h=4, num_linears_h=2)           # E = 741
            # the widest MLPs of the envelope (8 channels, four Linears), and a ragged general stack
        eng = plan_only(QM9, 9, c_hid_h=8, c_final_h=8, num_layers_h=1, num_linears_h=4)
        assert eng.query("h_wide") == 1 and eng.query("large_graph") == 1 and eng.query("r2_family") == 3 and eng.query("xa_lds_bytes") == 0
        # (36 graph + 19 hodge channels keep the final MLP a chained shape)
        eng = plan_only(GRID, 17, num_layers_h=4, c_hid_h=5, c_final_h=2, num_linears_h=2)
        assert eng.query("h_wide") == 1 and eng.query("large_graph") == 1 and eng.query("h_general") == 1
    forced(monkeypatch, False)
    # single Linears, 5 to 8 channels: not wide, the selection of narrower plans
    for over in (dict(c_hid_h=8, c_final_h=4), dict(c_hid_h=8, c_final_h=8, num_layers_h=1), dict(c_hid_h=5, c_final_h=3)):
        eng = plan_only(QM9, 9, **over)
        assert eng.query("h_wide") == 0 and eng.query("large_graph") == 0 and eng.query("xa_lds_bytes") > 0, over
    # num_linears_h = 2 with at most 4 channels (hid <= 8, enzymes_small_CC.yaml itself) stays narrow
    assert plan_only(ENZ, 12).query("h_wide") == 0
    # wide plans take no corrector fusion
    meta, _ = enz_wide()
    eng = cc.engine(meta, None, lib, device, weights=False, predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7)
    assert eng.query("h_wide") == 1 and eng.query("loop_form") == 1 and eng.query("tiled_fuse") == 0 and eng.query("fused_loop") == 0
    # the shipped checkpoints keep their kernels
    for name, family in ((QM9, 1), (ENZ, 3)):
        m, _ = load_ckpt_np(name)
        eng = cc.engine(m, None, lib, device, weights=False)
        assert eng.query("h_wide") == 0 and eng.query("large_graph") == 0 and eng.query("r2_family") == family, name


# ---- 7. GPU only
QM9_WIDE = "ccsd_qm9_wide_CC"


def case_yaml_run(lib, tmp_path, num_scales=5, batch=8):
    """CCSD("sample", <yaml>, folder=<checkout with the checkpoint written here>).run(gpus=1, rounds=1) on qm9_CC.yaml's architecture
    with c_hid_h 8 and num_linears_h 2 (seeded weights), a 5-scale SDE, batch 8: the route, shapes, finiteness, and the bonds (adj_int's
    relabelling, sampler.py:1219-1220: 3 = no bond) a symmetric 0/1 adjacency with a zero diagonal inside the flags."""
    import yaml

    from ccsd_amd.diffusion import CCSD
    from tests.test_harness import QM9_CC_YAML

    meta, parts = hs.arch_at(QM9, 9, seed=303, c_hid_h=8, num_linears_h=2)
    arrays = {f"{p}/{k}": v.detach().numpy() for p in NAMES for k, v in parts[p].items()}
    meta = json.loads(json.dumps({k: v for k, v in meta.items() if k != "files"}))
    for p in NAMES:
        meta["config"]["sde"][p]["num_scales"] = num_scales
    d = tmp_path / "checkpoints" / "QM9"
    os.makedirs(d, exist_ok=True)
    np.savez(d / f"{QM9_WIDE}.npz", **arrays)
    with open(d / f"{QM9_WIDE}.json", "w") as f:
        json.dump(meta, f)
    cfg = dict(QM9_CC_YAML, ckpt=QM9_WIDE, sample=dict(QM9_CC_YAML["sample"], divide_batch=1, n_samples=batch))
    os.makedirs(tmp_path / "config", exist_ok=True)
    with open(tmp_path / "config" / "sample_qm9_wide_CC.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    c = CCSD("sample", "sample_qm9_wide_CC", folder=str(tmp_path))
    out = c.run(gpus=1, rounds=1)
    sm = c.sampler
    assert type(sm).__name__ == "Sampler_mol_CC"
    eng = sm.sampling_fn.engine()
    assert eng.query("h_wide") == 1 and eng.query("large_graph") == 1 and eng.query("r2_family") == 3
    fl = out["flags"].cpu()
    assert out["adj"].shape == (batch, 9, 9) and out["x"].shape == (batch, 9, 4) and out["rank2"].shape == (batch, 36, 466)
    assert all(torch.isfinite(out[k]).all() for k in ("x", "adj", "rank2"))
    bonds = (out["adj_int"].cpu() != 3).to(torch.int64)
    assert set(out["adj_int"].unique().tolist()) <= {0, 1, 2, 3}
    assert torch.equal(bonds, bonds.transpose(1, 2)) and not torch.diagonal(bonds, dim1=1, dim2=2).any()
    assert not (bonds * (1 - fl[:, :, None] * fl[:, None, :]).to(torch.int64)).any()
