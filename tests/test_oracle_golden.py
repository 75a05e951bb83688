"""Pin the CPU oracle (oracle/ccsd_oracle.py) against vectors captured from the real reference.

The fixtures under tests/golden/ were produced by tools/make_golden.py, which imports the
upstream reference in the build container.  These tests run anywhere (no GPU, no reference).
"""
import contextlib
import json

import numpy as np
import pytest
import torch

from oracle import ccsd_oracle as O
from tests.helpers import load_ckpt_np, load_golden, parse_case, rng_matches

torch.set_num_threads(8)


def _close(out, ref, err_msg=""):
    """The oracle reproduces the reference bit-for-bit in the container the fixtures were made in
    (same ATen kernels).  On another host CPU the sgemm blocking may differ in the last bits, so
    fall back to a tight tolerance there instead of failing."""
    if np.array_equal(out, ref):
        return
    np.testing.assert_allclose(out, ref, rtol=2e-5, atol=2e-5, err_msg=err_msg)


def _check(out, g, key, err_msg="", exact=False):
    """`out` against the fixture entry `key`: stored whole (exact=True: integer outputs, bit for bit), or -- for tensors too large
    for a fixture (ego_small_CC's rank-2 outputs, tools/make_golden.py summarize) -- as the sha256 of the reference's bytes, a fixed
    subsample that holds every row's first and last entry, and float64 row sums.  The oracle reproduces those tensors bit for
    bit, so a summarized entry must match its hash, its subsample and its row sums exactly."""
    import hashlib

    if key in g.files:
        if exact:
            assert np.array_equal(out, g[key]), err_msg
        else:
            _close(out, g[key], err_msg)
        return
    out = np.ascontiguousarray(out)
    idx = g[f"{key}/idx"]
    assert out.size > idx.max() and g[f"{key}/rowsum"].shape == out.shape[:-1], err_msg
    assert np.array_equal(out.reshape(-1)[idx], g[f"{key}/val"]), f"{err_msg}: subsample differs from the reference's"
    assert np.array_equal(out.astype(np.float64).sum(axis=-1), g[f"{key}/rowsum"]), f"{err_msg}: row sums differ"
    assert hashlib.sha256(out.tobytes()).hexdigest() == str(g[f"{key}/sha256"]), f"{err_msg}: sha256 differs from the reference's"


CC = ["ccsd_qm9_CC", "ccsd_community_small_CC", "ccsd_enzymes_small_CC", "ccsd_qm9_Base_CC", "ccsd_community_small_Base_CC"]
GRAPH = ["gdss_community_small", "gdss_zinc250k"]
# shipped checkpoints the package does not carry (weights under tests/golden/ckpt/); ego_small_CC-sized rank-2 outputs are summaries
SHIPPED_CC = ["ccsd_enzymes_small_Base_CC", "ccsd_ego_small_CC", "ccsd_ego_small_CC_v2"]
SHIPPED_GRAPH = ["gdss_qm9", "gdss_qm9_retrained", "gdss_ego_small", "gdss_ego_small_retrained", "gdss_enzymes_small_retrained"]


def masked_state(seed, B, N, Fd, is_cc, d_min, d_max, flags, scale):
    torch.manual_seed(seed)
    x = O.mask_x(torch.randn(B, N, Fd) * scale, flags)
    a = torch.randn(B, N, N).triu(1) * scale
    adj = O.mask_adjs(a + a.transpose(-1, -2), flags)
    if not is_cc:
        return x, adj, None
    E, K = O.get_rank2_dim(N, d_min, d_max)
    return x, adj, O.mask_rank2(torch.randn(B, E, K) * scale, N, d_min, d_max, flags)


def nets_from_ckpt(name):
    meta, parts = load_ckpt_np(name)
    is_cc = meta["is_cc"]
    names = ["x", "adj"] + (["rank2"] if is_cc else [])
    nets = []
    for p in names:
        params, w = meta[f"params_{p}"], parts[p]
        if is_cc:
            nets.append(lambda x, a, r, f, params=params, w=w: O.run_network(params, w, x, a, r, f))
        else:
            nets.append(lambda x, a, f, params=params, w=w: O.run_network(params, w, x, a, None, f))
    return meta, nets


@pytest.mark.parametrize("name", CC + GRAPH + SHIPPED_CC + SHIPPED_GRAPH)
def test_g1_network_forward_and_score_fn(name):
    g = load_golden(f"g1_{name}.npz")
    assert rng_matches(g), "torch CPU RNG stream differs from the one the fixtures were made with"
    meta, nets = nets_from_ckpt(name)
    cfg, is_cc = meta["config"], meta["is_cc"]
    N, Fd = cfg["data"]["max_node_num"], cfg["data"]["max_feat_num"]
    d_min, d_max = (cfg["data"]["d_min"], cfg["data"]["d_max"]) if is_cc else (None, None)
    flags = torch.from_numpy(g["flags"])
    B = flags.shape[0]
    parts = ["x", "adj"] + (["rank2"] if is_cc else [])
    for tag, scale in (("unit", 1.0), ("small", 0.3)):
        x, adj, rank2 = masked_state(int(g["seed"]), B, N, Fd, is_cc, d_min, d_max, flags, scale)
        assert np.array_equal(x.numpy(), g[f"{tag}/x"]) and np.array_equal(adj.numpy(), g[f"{tag}/adj"])
        args = (x, adj, rank2, flags) if is_cc else (x, adj, flags)
        with torch.no_grad():
            for p, net in zip(parts, nets):
                out = net(*args).numpy()
                _check(out, g, f"{tag}/net_{p}", f"{name} {tag} {p}")
            if tag == "unit":
                sdes = [O.load_sde(cfg["sde"][p]) for p in parts]
                for ti, tval in enumerate([1.0, 0.5, 1e-4]):
                    t = torch.ones(B) * tval
                    for p, net, s in zip(parts, nets, sdes):
                        key = f"{tag}/score_{p}_t{ti}"
                        if key not in g.files and f"{key}/sha256" not in g.files:
                            continue
                        out = O.make_score_fn(s, net)(*args, t).numpy()
                        _check(out, g, key, key)


def test_g3_sde_tables_bit_exact():
    g = load_golden("g3_sde_tables.npz")
    ts = torch.linspace(1, 1e-4, 1000)
    assert np.array_equal(ts.numpy(), g["timesteps"])
    for kind, (k, bmin, bmax) in {"VP": ("VP", 0.1, 1.0), "VE": ("VE", 0.1, 1.0), "VE2": ("VE", 0.2, 1.0),
                                  "subVP": ("subVP", 0.1, 1.0)}.items():
        s = O.SDE(k, bmin, bmax, 1000)
        v = torch.ones(1000, 1, 1) * 0.5
        assert np.array_equal((ts * (s.N - 1) / s.T).long().numpy(), g[f"{kind}/timestep_idx"])
        drift, diff = s.sde(v, ts)
        assert np.array_equal(drift.numpy(), g[f"{kind}/sde_drift"])
        assert np.array_equal(diff.numpy(), g[f"{kind}/sde_diffusion"])
        assert np.array_equal(s.marginal_std(ts).numpy(), g[f"{kind}/marginal_std"])
        f, G = s.discretize(v, ts)
        assert np.array_equal(f.numpy(), g[f"{kind}/disc_f"])
        assert np.array_equal(G.numpy(), g[f"{kind}/disc_G"])
        if k != "VE":
            assert np.array_equal(s.alphas.numpy(), g[f"{kind}/alphas"])
        else:
            assert np.array_equal(s.discrete_sigmas.numpy(), g[f"{kind}/discrete_sigmas"])
        if k != "subVP":
            m, std = s.transition(v, ts, -0.5 / 1000)
            assert np.array_equal(m.numpy(), g[f"{kind}/trans_mean"])
            assert np.array_equal(std.numpy(), g[f"{kind}/trans_std"], equal_nan=True)


def test_g6_masks_and_utils_bit_exact():
    g = load_golden("g6_masks_utils.npz")
    for (N, d_min, d_max) in [(9, 3, 9), (20, 3, 3), (5, 3, 4), (12, 3, 4)]:
        tag = f"{N}_{d_min}_{d_max}"
        edges, inc = O.cell_tables(N, d_min, d_max)
        assert np.array_equal(inc.numpy().astype(np.uint8), g[f"{tag}/cell_incidence"])
        assert tuple(g[f"{tag}/dims"]) == O.get_rank2_dim(N, d_min, d_max) == (edges.shape[0], inc.shape[0])
        flags = torch.from_numpy(g[f"{tag}/flags"])
        fl, fr = O.rank2_flags(flags, N, d_min, d_max)
        assert np.array_equal(fl.numpy(), g[f"{tag}/fl"]) and np.array_equal(fr.numpy(), g[f"{tag}/fr"])
        assert np.array_equal(O.hodge_adj_flags(flags).numpy(), g[f"{tag}/fh"])
    a = torch.from_numpy(g["util/adj"])
    assert np.array_equal(O.adj_to_hodgedual(a).numpy(), g["util/hodgedual"])
    assert np.array_equal(O.hodgedual_to_adj(torch.from_numpy(g["util/hodge_in"])).numpy(), g["util/hodge_to_adj"])
    r = torch.from_numpy(g["util/rank2"])
    assert np.array_equal(O.pow_tensor_cc(r, 3, O._nodiag_mask(15)).numpy(), g["util/pow_cc"])
    assert np.array_equal(O.pow_tensor(a[:, 0], 3).numpy(), g["util/pow_adj"])
    q = torch.from_numpy(g["util/q_in"])
    assert np.array_equal(O.quantize(q).numpy(), g["util/quantize"])
    assert np.array_equal(O.quantize_mol(q), g["util/quantize_mol"])
    assert O.quantize_mol(q).dtype == np.int64


def test_kat_small_models_general_path():
    """Small nets built by the reference constructors, incl. num_linears_h=2 / num_layers_mlp=2."""
    g = load_golden("kat_small_models.npz")
    meta = json.loads(str(g["meta"]))
    flags, x, adj, rank2 = (torch.from_numpy(g[k]) for k in ("flags", "x", "adj", "rank2"))
    for tag, params in meta.items():
        w = {k[len(tag) + 3:]: torch.from_numpy(g[k]).requires_grad_(True) for k in g.files if k.startswith(f"{tag}/w/")}
        with torch.no_grad():
            out = O.run_network(params, w, x, adj, rank2, flags)
        _close(out.numpy(), g[f"{tag}/out"], tag)


def test_kat_gmh_models():
    """ScoreNetworkX_GMH built by the reference's constructor (no shipped checkpoint uses it)."""
    g = load_golden("kat_gmh_models.npz")
    meta = json.loads(str(g["meta"]))
    for tag, params in meta.items():
        flags, x, adj = (torch.from_numpy(g[f"{tag}/{k}"]) for k in ("flags", "x", "adj"))
        w = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/w/")}
        with torch.no_grad():
            out = O.run_network(params, w, x, adj, None, flags)
        _close(out.numpy(), g[f"{tag}/out"], tag)


G5 = [
    ("ccsd_qm9_CC", "ccsd_qm9_CC", ["k10", "k50", "n1000_first3"]),
    ("ccsd_community_small_CC", "ccsd_community_small_CC", ["k5", "n1000_first2"]),
    ("gdss_community_small", "gdss_community_small", ["k10", "n1000_first3"]),
    ("gdss_zinc250k", "gdss_zinc250k", ["k5"]),
    ("ccsd_qm9_Base_CC", "ccsd_qm9_Base_CC", ["k10", "n1000_first3"]),
    ("ccsd_qm9_CC_nsteps2_none", "ccsd_qm9_CC", ["k6"]),
    ("ccsd_qm9_CC_langevin2", "ccsd_qm9_CC", ["k4"]),
    # S4_solver (solver.py:1179-1563)
    ("s4_ccsd_enzymes_small_CC", "ccsd_enzymes_small_CC", ["k4", "k20", "n1000_first2"]),
    ("s4_ccsd_qm9_CC", "ccsd_qm9_CC", ["k6"]),
    ("s4_gdss_community_small", "gdss_community_small", ["k5"]),
    # subVPSDE (Euler; Reverse through the base-class discretize), probability_flow + Reverse, subVP on x only with n_steps = 2
    ("ccsd_qm9_CC_subvp_euler", "ccsd_qm9_CC", ["k6"]),
    ("ccsd_qm9_CC_subvp_reverse", "ccsd_qm9_CC", ["k6"]),
    ("ccsd_qm9_CC_pflow", "ccsd_qm9_CC", ["k6"]),
    ("gdss_community_small_pflow", "gdss_community_small", ["k5"]),
    ("ccsd_qm9_CC_subvp_mixed", "ccsd_qm9_CC", ["k4"]),
    # the shipped qm9_CC sampling set-up at FULL length: 1000 scales from the prior to the last step (B = 2)
    ("ccsd_qm9_CC_full1000", "ccsd_qm9_CC", ["n1000"]),
    # the shipped checkpoints of SHIPPED_CC / SHIPPED_GRAPH at their own sample_*.yaml settings
    *[(n, n, ["k6", "n1000_first2"]) for n in SHIPPED_CC + SHIPPED_GRAPH],
]


def oracle_sampler_from_golden(g, ckpt, case, noise=None):
    meta, nets = nets_from_ckpt(ckpt)
    cfg, is_cc = meta["config"], meta["is_cc"]
    sm = json.loads(str(g["sampler"]))
    N, Fd = cfg["data"]["max_node_num"], cfg["data"]["max_feat_num"]
    flags = torch.from_numpy(g["flags"])
    B = flags.shape[0]
    num_scales, max_steps = parse_case(case)
    parts = ["x", "adj"] + (["rank2"] if is_cc else [])
    sdes = []
    for p in parts:
        c = dict(cfg["sde"][p])
        c.update(sm.get("sde_override", {}).get(p, {}))
        if num_scales is not None:
            c["num_scales"] = num_scales
        sdes.append(O.load_sde(c))
    kw = dict(sde_x=sdes[0], sde_adj=sdes[1], shape_x=(B, N, Fd), shape_adj=(B, N, N), predictor=sm["predictor"],
              corrector=sm["corrector"], snr=sm["snr"], scale_eps=sm["scale_eps"], n_steps=sm["n_steps"],
              probability_flow=bool(sm.get("probability_flow", False)), continuous=True, denoise=True, eps=1e-4, n_diff_steps=max_steps, noise=noise)
    if is_cc:
        d_min, d_max = cfg["data"]["d_min"], cfg["data"]["d_max"]
        kw.update(is_cc=True, sde_rank2=sdes[2], shape_rank2=(B, *O.get_rank2_dim(N, d_min, d_max)), d_min=d_min, d_max=d_max)
    return (O.S4_solver if sm["predictor"] == "S4" else O.get_pc_sampler)(**kw), nets, flags, parts


@pytest.mark.parametrize("gname,ckpt,cases", G5)
def test_g5_pc_sampler_identical_seed(gname, ckpt, cases):
    """End-to-end sampler: same seed -> same prior and noise stream -> reference outputs."""
    g = load_golden(f"g5_{gname}.npz")
    assert rng_matches(g)
    for case in cases:
        fn, nets, flags, parts = oracle_sampler_from_golden(g, ckpt, case)
        torch.manual_seed(int(g["seed"]))
        res = fn(*nets, flags)
        for p, v in zip(parts, res):
            _check(v.numpy(), g, f"{case}/{p}", f"{gname} {case} {p}")
        assert int(res[len(parts)]) == int(g[f"{case}/nfe"])
        assert len(res[-1]) == int(g[f"{case}/traj_len"])
        _close(res[-1][-1][1].numpy(), g[f"{case}/traj_last_adj"])
        # integer outputs: bit-exact
        assert np.array_equal(O.quantize(res[1]).numpy(), g[f"{case}/quantize_adj"])
        assert np.array_equal(O.quantize_mol(res[1]), g[f"{case}/quantize_mol_adj"])
        if "rank2" in parts:
            _check(O.quantize(res[2]).numpy().astype(np.uint8), g, f"{case}/quantize_rank2", f"{gname} {case} quantize_rank2",
                   exact=True)


def test_kat_cnum_more_hodge_powers():
    g = load_golden("kat_cnum.npz")
    meta = json.loads(str(g["meta"]))
    for tag, params in meta.items():
        flags, rank2 = (torch.from_numpy(g[f"{tag}/{k}"]) for k in ("flags", "rank2"))
        w = {k[len(tag) + 3:]: torch.from_numpy(g[k]).requires_grad_(True) for k in g.files if k.startswith(f"{tag}/w/")}
        with torch.no_grad():
            out = O.run_network(params, w, None, None, rank2, flags)
        _close(out.numpy(), g[f"{tag}/out"], tag)


def test_kat_arch_sweep():
    """Six architectures of the architecture sweep (tests/arch_sweep_cases.py) built by the reference's constructors: an un-chained
    edge MLP with five adjacency powers, one and three heads, four Linears per edge MLP, one AttentionLayer; ScoreNetworkF 12 wide
    with four Linears."""
    g = load_golden("kat_arch_sweep.npz")
    meta = json.loads(str(g["meta"]))
    assert len(meta) == 6
    for tag, params in meta.items():
        t = {k: torch.from_numpy(g[f"{tag}/{k}"]) if f"{tag}/{k}" in g.files else None for k in ("flags", "x", "adj", "rank2")}
        w = {k[len(tag) + 3:]: torch.from_numpy(g[k]).requires_grad_(True) for k in g.files if k.startswith(f"{tag}/w/")}
        with torch.no_grad():
            out = O.run_network(params, w, t["x"], t["adj"], t["rank2"], t["flags"])
        _close(out.numpy(), g[f"{tag}/out"], tag)


def test_kat_hodge_layers_three_and_four():
    g = load_golden("kat_hodge_layers.npz")
    meta = json.loads(str(g["meta"]))
    for tag, params in meta.items():
        flags, x, adj, rank2 = (torch.from_numpy(g[f"{tag}/{k}"]) for k in ("flags", "x", "adj", "rank2"))
        w = {k[len(tag) + 3:]: torch.from_numpy(g[k]).requires_grad_(True) for k in g.files if k.startswith(f"{tag}/w/")}
        with torch.no_grad():
            out = O.run_network(params, w, x, adj, rank2, flags)
        _close(out.numpy(), g[f"{tag}/out"], tag)


def test_kat_hodge_general_mlp_value():
    """three / four HodgeAdjAttentionLayers with num_linears_h = 2, 3 (non-affine mlp_value behind a dense hodge layer)."""
    g = load_golden("kat_hodge_general.npz")
    meta = json.loads(str(g["meta"]))
    for tag, params in meta.items():
        flags, x, adj, rank2 = (torch.from_numpy(g[f"{tag}/{k}"]) for k in ("flags", "x", "adj", "rank2"))
        w = {k[len(tag) + 3:]: torch.from_numpy(g[k]).requires_grad_(True) for k in g.files if k.startswith(f"{tag}/w/")}
        with torch.no_grad():
            out = O.run_network(params, w, x, adj, rank2, flags)
        _close(out.numpy(), g[f"{tag}/out"], tag)


def test_zinc5b_substitute_networks_and_sampler():
    """SURVEY 8(d) substitute 5b (N = 38 CC, d_min = d_max = 3, zinc250k_CC.yaml hyper-parameters, reference-initialised
    weights): forwards and a 3-scale sampler run."""
    from tests import parity_cases as pc

    g, meta, sd, flags, (x, adj, rank2) = pc.zinc5b_setup()
    N, Fd, d_min, d_max, E, K = meta["dims"]
    pm = meta["params"]
    w = {p: {k: v.clone().requires_grad_(True) for k, v in sd[p].items()} for p in sd}
    with torch.no_grad():
        _close(O.run_network(pm["x"], w["x"], x, adj, rank2, flags).numpy(), g["x/out"], "5b x")
        _close(O.run_network(pm["adj"], w["adj"], x, adj, rank2, flags).numpy(), g["adj/out"], "5b adj")
        o = O.run_network(pm["rank2"], w["rank2"], x, adj, rank2, flags)
        _close(o[:, ::37, ::53].numpy(), g["rank2/out_sample"], "5b rank2")
    sdes = [O.load_sde(dict(meta["sde"][p], num_scales=3)) for p in ("x", "adj", "rank2")]
    nets = [(lambda x_, a_, r_, f_, p=p: O.run_network(pm[p], w[p], x_, a_, r_, f_)) for p in ("x", "adj", "rank2")]
    sm = meta["sampler"]
    B = flags.shape[0]
    fn = O.get_pc_sampler(sde_x=sdes[0], sde_adj=sdes[1], sde_rank2=sdes[2], shape_x=(B, N, Fd), shape_adj=(B, N, N),
                          shape_rank2=(B, E, K), predictor=sm["predictor"], corrector=sm["corrector"], snr=sm["snr"],
                          scale_eps=sm["scale_eps"], n_steps=1, probability_flow=False, continuous=True, denoise=True, eps=1e-4,
                          is_cc=True, d_min=d_min, d_max=d_max, keep_traj=False)
    torch.manual_seed(int(g["seed"]))
    res = fn(*nets, flags)
    _close(res[0].numpy(), g["k3/x"], "5b k3 x")
    _close(res[1].numpy(), g["k3/adj"], "5b k3 adj")
    _close(res[2][:, ::37, ::53].numpy(), g["k3/rank2_sample"], "5b k3 rank2")
    assert np.array_equal(O.quantize_mol(res[1]), g["k3/quantize_mol_adj"])


def test_registry_errors_match_reference():
    s = O.SDE("VE", 0.1, 1.0, 10)
    with pytest.raises(NotImplementedError):
        O.get_pc_sampler(s, s, (1, 3, 2), (1, 3, 3), predictor="Heun", continuous=True)
    with pytest.raises(NotImplementedError):
        O.get_pc_sampler(s, s, (1, 3, 2), (1, 3, 3), corrector="MALA", continuous=True)
    with pytest.raises(NotImplementedError):
        O.SDE("foo", 0.1, 1.0, 10)
    with pytest.raises(ValueError):
        O.run_network({"model_type": "nope"}, {}, None, None, None, None)


@contextlib.contextmanager
def ulp_perturbed_draws(pattern_seed):
    """Every torch.randn / randn_like draw moved by exactly one ulp, up or down by a seeded pattern (a 6e-8 relative change)."""
    rn, rl = torch.randn, torch.randn_like
    gen = np.random.default_rng(pattern_seed)

    def bump(t):
        up = torch.from_numpy(gen.integers(0, 2, size=tuple(t.shape)).astype(bool))
        return torch.nextafter(t, torch.where(up, torch.full_like(t, float("inf")), torch.full_like(t, float("-inf"))))
    torch.randn = lambda *s, **k: bump(rn(*s, **k))
    torch.randn_like = lambda t, **k: bump(rl(t, **k))
    try:
        yield
    finally:
        torch.randn, torch.randn_like = rn, rl


def test_traj_rtol_is_the_reference_one_ulp_sensitivity():
    """The only trajectory tolerances wider than 1e-4 (parity_cases.TRAJ_RTOL: S4 on ENZYMES_small_CC with 4 / 20 scales, S4 on
    enzymes_small_Base_CC with 6 scales) are
    pinned to a measurement on the reference algorithm alone: the oracle reproduces the golden bit for bit, and the same fp32
    run with every normal draw moved by one ulp ends `sens` away from it on rank2 (relative to the tensor's scale, the
    measure assert_close uses).  TRAJ_RTOL must lie within [1.5, 2.5] x the median sensitivity over four perturbation patterns:
    no implementation that rounds anywhere differently from the reference can be held to less, and a tolerance looser than that
    would hide defects."""
    from tests.parity_cases import TRAJ_RTOL
    ckpts = {"s4_ccsd_enzymes_small_CC": "ccsd_enzymes_small_CC", "ccsd_enzymes_small_Base_CC": "ccsd_enzymes_small_Base_CC"}
    assert set(TRAJ_RTOL) == {("s4_ccsd_enzymes_small_CC", "k4"), ("s4_ccsd_enzymes_small_CC", "k20"),
                              ("ccsd_enzymes_small_Base_CC", "k6")}
    for gname, case in sorted(TRAJ_RTOL):
        g = load_golden(f"g5_{gname}.npz")
        assert rng_matches(g)
        fn, nets, flags, parts = oracle_sampler_from_golden(g, ckpts[gname], case)
        torch.manual_seed(int(g["seed"]))
        plain = fn(*nets, flags)[2]
        ref = torch.from_numpy(g[f"{case}/rank2"])
        _close(plain.numpy(), ref.numpy(), f"the oracle no longer reproduces the {gname} golden: re-derive TRAJ_RTOL")
        scale = ref.abs().max().item()
        sens = []
        for pattern in range(4):
            with ulp_perturbed_draws(pattern):
                torch.manual_seed(int(g["seed"]))
                pert = fn(*nets, flags)[2]
            sens.append(((pert - plain).abs().max() / scale).item())
        med = float(np.median(sens))
        assert med > 0.5e-4, (gname, case, sens)
        assert 1.5 * med <= TRAJ_RTOL[(gname, case)] <= 2.5 * med, (gname, case, sens, TRAJ_RTOL[(gname, case)])
