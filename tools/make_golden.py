"""Generate the committed fixtures from the real reference (build container only).

Runs the upstream reference (imported read-only from /root/reference through
tools/refshim.py) and writes

  ccsd_amd/checkpoints/<name>.npz + <name>.json   neutral-format copies of the shipped
                                                  checkpoints (weights are data, not source)
  tests/golden/*.npz                              golden input/output vectors

Nothing here is imported by the product or by the tests; the tests only read the
.npz/.json files.  Re-run with:  python tools/make_golden.py
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import refshim  # noqa: E402

refshim.install()
import torch  # noqa: E402

from ccsd.src import solver as ref_solver  # noqa: E402
from ccsd.src import sde as ref_sde  # noqa: E402
from ccsd.src import losses as ref_losses  # noqa: E402
from ccsd.src.utils import loader as ref_loader  # noqa: E402
from ccsd.src.utils import cc_utils as ref_cc  # noqa: E402
from ccsd.src.utils import graph_utils as ref_gu  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CKPT = os.path.join(ROOT, "ccsd_amd", "checkpoints")
os.makedirs(GOLD, exist_ok=True)
os.makedirs(CKPT, exist_ok=True)

CHECKPOINTS = {
    # name -> (relative path, is_cc, sampler yaml)
    "ccsd_qm9_CC": ("checkpoints/QM9/ccsd_qm9_CC.pth", True),
    "ccsd_community_small_CC": ("checkpoints/community_small_CC/ccsd_community_small_CC.pth", True),
    "ccsd_enzymes_small_CC": ("checkpoints/ENZYMES_small_CC/ccsd_enzymes_small_CC.pth", True),
    "gdss_community_small": ("checkpoints/community_small/gdss_community_small.pth", False),
    "gdss_zinc250k": ("checkpoints/ZINC250k/gdss_zinc250k.pth", False),
    # ScoreNetworkA_Base_CC (HodgeBaselineLayer) ablation checkpoints
    "ccsd_qm9_Base_CC": ("checkpoints/QM9/ccsd_qm9_Base_CC.pth", True),
    "ccsd_community_small_Base_CC": ("checkpoints/community_small_CC/ccsd_community_small_Base_CC.pth", True),
}


def plain(o):
    """EasyDict / numpy scalars -> plain JSON-able python."""
    if isinstance(o, dict):
        return {str(k): plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    if isinstance(o, (np.integer,)):
        return int(o)
    if isinstance(o, (np.floating,)):
        return float(o)
    return o


# Shipped checkpoints within the N <= 38 envelope that the product does not package: their converted weights are test
# fixtures only (tests/golden/ckpt/, found there by tests/helpers.load_ckpt_np).  `python tools/make_golden.py shipped`
# writes these files and nothing else.
SHIPPED = {
    "ccsd_ego_small_CC": ("checkpoints/ego_small_CC/ccsd_ego_small_CC.pth", True),
    "ccsd_ego_small_CC_v2": ("checkpoints/ego_small_CC/ccsd_ego_small_CC_v2.pth", True),
    "ccsd_enzymes_small_Base_CC": ("checkpoints/ENZYMES_small_CC/ccsd_enzymes_small_Base_CC.pth", True),
    "gdss_qm9": ("checkpoints/QM9/gdss_qm9.pth", False),
    "gdss_qm9_retrained": ("checkpoints/QM9/gdss_qm9_retrained.pth", False),
    "gdss_ego_small": ("checkpoints/ego_small/gdss_ego_small.pth", False),
    "gdss_ego_small_retrained": ("checkpoints/ego_small/gdss_ego_small_retrained.pth", False),
    "gdss_enzymes_small_retrained": ("checkpoints/ENZYMES_small/gdss_enzymes_small_retrained.pth", False),
    # above 64 nodes: the tiled graph-network route (`python tools/make_golden.py large`)
    "gdss_enzymes": ("checkpoints/ENZYMES/gdss_enzymes.pth", False),
    "gdss_grid": ("checkpoints/grid/gdss_grid.pth", False),
    # ScoreNetworkA_CC with one hodge layer at N = 49: the tiled graph-network route for combinatorial complexes
    # (`python tools/make_golden.py grid_small_cc`; kept in a folder of its own, CC_LARGE_CKPT)
    "ccsd_grid_small_CC": ("checkpoints/grid_small_CC/ccsd_grid_small_CC.pth", True),
}
SHIPPED_CKPT = os.path.join(GOLD, "ckpt")
# (a folder below ckpt/: tests/test_large_graph.py pins the k_xa variant of every checkpoint that lies in ckpt/ itself)
CC_LARGE_CKPT = os.path.join(SHIPPED_CKPT, "cc_large")
MAX_FIXTURE = 1 << 20                # no committed file exceeds 1 MiB


def export_checkpoint(name, table=CHECKPOINTS, dest=CKPT, apply_ema=False):
    """apply_ema (fixtures of checkpoints whose sample_*.yaml sets use_ema): the EMA shadow parameters are copied over the state
    dicts' parameters (ema.copy_to(model.parameters()), sampler.py:469-471) in the returned checkpoint and in the files, so that
    the fixture holds the weights the shipped configuration samples with; the json says so ("ema_applied") and lists the
    parameters' names per part ("ema_params": a harness run with use_ema finds its ema_<part>/ entries among them)."""
    rel, is_cc = table[name]
    ck = refshim.load_reference_ckpt(rel)
    arrays = {}
    meta = {"name": name, "source": rel, "is_cc": is_cc, "config": plain(ck["model_config"])}
    if apply_ema:
        meta["ema_applied"], meta["ema_params"] = True, {}
        for part in ["x", "adj"] + (["rank2"] if is_cc else []):
            sd = ck[f"{part}_state_dict"]
            m = ref_loader.load_model_from_ckpt(ck[f"params_{part}"], sd, "cpu")
            names = [n for n, _ in m.named_parameters()]
            shadow = ck.pop(f"ema_{part}")["shadow_params"]
            assert len(names) == len(shadow)
            pre = "module." if any(k.startswith("module.") for k in sd) else ""
            for n, v in zip(names, shadow):
                assert sd[pre + n].shape == v.shape
                sd[pre + n] = v.detach().clone()
            meta["ema_params"][part] = [n[7:] if n.startswith("module.") else n for n in names]
    for part in ["x", "adj"] + (["rank2"] if is_cc else []):
        meta[f"params_{part}"] = plain(ck[f"params_{part}"])
        sd = ck[f"{part}_state_dict"]
        for k, v in sd.items():
            k = k[7:] if k.startswith("module.") else k
            arrays[f"{part}/{k}"] = v.detach().cpu().numpy().astype(np.float32)
        if f"ema_{part}" in ck:
            # torch_ema state: shadow_params in model.parameters() order (loader.py:169-184, sampler.py:469-471)
            m = ref_loader.load_model_from_ckpt(ck[f"params_{part}"], sd, "cpu")
            names = [n[7:] if n.startswith("module.") else n for n, _ in m.named_parameters()]
            shadow = ck[f"ema_{part}"]["shadow_params"]
            assert len(names) == len(shadow)
            for n, v in zip(names, shadow):
                arrays[f"ema_{part}/{n}"] = v.detach().cpu().numpy().astype(np.float32)
    os.makedirs(dest, exist_ok=True)
    if dest == CKPT:
        np.savez_compressed(os.path.join(dest, name + ".npz"), **arrays)
    else:
        # fixture files stay under MAX_FIXTURE: the state-dict weights (what every parity run uses) in <name>.npz (+ <name>.<i>.npz),
        # listed in meta["files"] for tests/helpers.load_ckpt_np.  The EMA shadow weights are not kept: no test reads them
        keys = [k for k in arrays if not k.startswith("ema_")]
        shards, cur, size = [], [], 0
        for k in keys:
            if cur and size + arrays[k].nbytes > MAX_FIXTURE - (64 << 10):
                shards.append(cur)
                cur, size = [], 0
            cur.append(k)
            size += arrays[k].nbytes
        if cur:
            shards.append(cur)
        meta["files"] = []
        for i, ks in enumerate(shards):
            fname = name + (".npz" if i == 0 else f".{i}.npz")
            np.savez_compressed(os.path.join(dest, fname), **{k: arrays[k] for k in ks})
            assert os.path.getsize(os.path.join(dest, fname)) <= MAX_FIXTURE, fname
            meta["files"].append(os.path.relpath(os.path.join(dest, fname), SHIPPED_CKPT))   # (as tests/helpers.load_ckpt_np joins them)
    with open(os.path.join(dest, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    return ck


def build_models(ck, is_cc):
    # ScoreNetworkF.__init__ does `default_mask(rows).unsqueeze_(0)` on the lru-cached tensor (ScoreNetwork_F.py:135-141,
    # cc_utils.py:932-942): every construction in one process adds a leading dimension to the shared mask and the third
    # one makes pow_tensor_cc's bmm fail.  A fresh cache per construction gives each model the (1, E, E) mask of a
    # first construction.
    ref_cc.default_mask.cache_clear()
    ms = [ref_loader.load_model_from_ckpt(ck["params_x"], ck["x_state_dict"], "cpu"),
          ref_loader.load_model_from_ckpt(ck["params_adj"], ck["adj_state_dict"], "cpu")]
    if is_cc:
        ms.append(ref_loader.load_model_from_ckpt(ck["params_rank2"], ck["rank2_state_dict"], "cpu"))
    for m in ms:
        m.eval()
    return ms


def make_flags(B, N, counts):
    f = torch.zeros(B, N)
    for b in range(B):
        f[b, : counts[b % len(counts)]] = 1.0
    return f


def rng_probe(seed):
    torch.manual_seed(seed)
    return torch.randn(8).numpy()


def masked_state(seed, B, N, Fdim, is_cc, d_min, d_max, flags, scale=1.0):
    torch.manual_seed(seed)
    x = ref_gu.mask_x(torch.randn(B, N, Fdim) * scale, flags)
    a = torch.randn(B, N, N).triu(1) * scale
    adj = ref_gu.mask_adjs(a + a.transpose(-1, -2), flags)
    if not is_cc:
        return x, adj, None
    E, K = ref_cc.get_rank2_dim(N, d_min, d_max)
    rank2 = ref_cc.mask_rank2(torch.randn(B, E, K) * scale, N, d_min, d_max, flags)
    return x, adj, rank2


SUMMARY_BYTES = 1 << 20      # arrays above this size are stored as a summary (summarize) in the shipped-checkpoint fixtures
SUMMARY_SAMPLES = 1 << 16


def summarize(key, a):
    """An array too large for a fixture -> {key}/sha256 of its bytes, a fixed subsample ({key}/idx, {key}/val: seeded flat
    indices that include every row's first and last entry) and its float64 row sums ({key}/rowsum, over the last axis)."""
    import hashlib

    a = np.ascontiguousarray(a)
    n, last = a.size, a.shape[-1]
    rows = np.arange(n // last, dtype=np.int64) * last
    rng = np.random.default_rng(20261016)
    idx = np.unique(np.concatenate([rows, rows + last - 1, rng.choice(n, SUMMARY_SAMPLES, replace=False)]))
    return {f"{key}/sha256": np.array(hashlib.sha256(a.tobytes()).hexdigest()), f"{key}/idx": idx,
            f"{key}/val": a.reshape(-1)[idx], f"{key}/rowsum": a.astype(np.float64).sum(axis=-1)}


def save_golden(fname, out, summarize_large=False):
    if summarize_large:
        limit = SUMMARY_BYTES if summarize_large is True else int(summarize_large)      # (an int: a lower threshold)
        for k in [k for k, v in out.items() if isinstance(v, np.ndarray) and v.nbytes > limit]:
            out.update(summarize(k, out.pop(k)))
    path = os.path.join(GOLD, fname)
    np.savez_compressed(path, **out)
    if summarize_large:
        assert os.path.getsize(path) <= MAX_FIXTURE, (fname, os.path.getsize(path))


def g1_network_forwards(name, ck, is_cc, B, counts, seed=1234, summarize_large=False, rank2_score=True):
    """G1/G2: per-network forward + score-fn scaling at three t (rank2_score=False: none for rank2 -- a third summarised rank-2
    array would take the file past MAX_FIXTURE at grid_small_CC's E)."""
    cfg = ck["model_config"]
    N, Fd = cfg["data"]["max_node_num"], cfg["data"]["max_feat_num"]
    d_min, d_max = (cfg["data"]["d_min"], cfg["data"]["d_max"]) if is_cc else (None, None)
    models = build_models(ck, is_cc)
    flags = make_flags(B, N, counts)
    out = {"flags": flags.numpy(), "seed": seed, "rng_probe": rng_probe(seed)}
    for tag, scale in (("unit", 1.0), ("small", 0.3)):
        x, adj, rank2 = masked_state(seed, B, N, Fd, is_cc, d_min, d_max, flags, scale)
        out[f"{tag}/x"], out[f"{tag}/adj"] = x.numpy(), adj.numpy()
        if is_cc:
            out[f"{tag}/rank2_checksum"] = np.array([rank2.double().sum().item(), rank2.abs().double().sum().item()])
        with torch.no_grad():
            args = (x, adj, rank2, flags) if is_cc else (x, adj, flags)
            for part, m in zip(["x", "adj", "rank2"], models):
                out[f"{tag}/net_{part}"] = m(*args).numpy()
            # G2 score functions
            sdes = [ref_loader.load_sde(cfg["sde"][p]) for p in (["x", "adj"] + (["rank2"] if is_cc else []))]
            for ti, tval in enumerate([1.0, 0.5, 1e-4]):
                t = torch.ones(B) * tval
                for part, m, s in zip(["x", "adj", "rank2"], models, sdes):
                    if tag != "unit" or (part == "rank2" and (ti != 1 or not rank2_score)):
                        continue
                    fn = (ref_losses.get_score_fn_cc if is_cc else ref_losses.get_score_fn)(s, m, train=False, continuous=True)
                    out[f"{tag}/score_{part}_t{ti}"] = fn(*args, t).numpy()
    save_golden(f"g1_{name}.npz", out, summarize_large)
    print("g1", name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.ndim > 1 and "net" in k})


def g3_sde_tables():
    out = {}
    ts = torch.linspace(1, 1e-4, 1000)
    out["timesteps"] = ts.numpy()
    for kind, (bmin, bmax) in {"VP": (0.1, 1.0), "VE": (0.1, 1.0), "VE2": (0.2, 1.0), "subVP": (0.1, 1.0)}.items():
        k = kind.rstrip("2")
        s = ref_loader.load_sde(refshim.EasyDict(type=k, beta_min=bmin, beta_max=bmax, num_scales=1000))
        v = torch.ones(1000, 1, 1) * 0.5
        out[f"{kind}/timestep_idx"] = (ts * (s.N - 1) / s.T).long().numpy()
        drift, diff = s.sde(v, ts)
        out[f"{kind}/sde_drift"], out[f"{kind}/sde_diffusion"] = drift.numpy(), diff.numpy()
        out[f"{kind}/marginal_std"] = s.marginal_prob(torch.zeros_like(v), ts)[1].numpy()
        f, G = s.discretize(v, ts)
        out[f"{kind}/disc_f"], out[f"{kind}/disc_G"] = f.numpy(), G.numpy()
        if k in ("VP", "subVP"):
            out[f"{kind}/alphas"] = s.alphas.numpy()
            out[f"{kind}/discrete_betas"] = s.discrete_betas.numpy()
        else:
            out[f"{kind}/discrete_sigmas"] = s.discrete_sigmas.numpy()
        if k != "subVP":
            m, std = s.transition(v, ts, -0.5 / 1000)
            out[f"{kind}/trans_mean"], out[f"{kind}/trans_std"] = m.numpy(), std.numpy()
    np.savez_compressed(os.path.join(GOLD, "g3_sde_tables.npz"), **out)


def g6_masks():
    out = {}
    for (N, d_min, d_max) in [(9, 3, 9), (20, 3, 3), (5, 3, 4), (12, 3, 4)]:
        E, K = ref_cc.get_rank2_dim(N, d_min, d_max)
        cells = ref_cc.get_cells(N, d_min, d_max)[0]
        inc = np.zeros((K, N), dtype=np.uint8)
        for c, s in enumerate(cells):
            inc[c, sorted(s)] = 1
        tag = f"{N}_{d_min}_{d_max}"
        out[f"{tag}/cell_incidence"] = inc
        out[f"{tag}/dims"] = np.array([E, K])
        flags = torch.ones(5, N)
        flags[1, N - 1] = 0
        flags[2, N - 2:] = 0
        flags[3, 0] = 0
        flags[4, 1:N - 1] = 0
        fl, fr = ref_cc.get_rank2_flags(torch.zeros(5, E, K), N, d_min, d_max, flags)
        fh = ref_cc.get_hodge_adj_flags(torch.zeros(5, E, E), flags)
        out[f"{tag}/flags"], out[f"{tag}/fl"], out[f"{tag}/fr"], out[f"{tag}/fh"] = flags.numpy(), fl.numpy(), fr.numpy(), fh.numpy()
    # small tensor utils
    torch.manual_seed(7)
    a = torch.randn(2, 3, 6, 6)
    a = a + a.transpose(-1, -2)
    h = ref_cc.adj_to_hodgedual(a)
    out["util/adj"], out["util/hodgedual"] = a.numpy(), h.numpy()
    hh = torch.randn(2, 3, 15, 15)
    out["util/hodge_in"], out["util/hodge_to_adj"] = hh.numpy(), ref_cc.hodgedual_to_adj(hh).numpy()
    r = torch.randn(2, 15, 20)
    out["util/rank2"] = r.numpy()
    out["util/pow_cc"] = ref_cc.pow_tensor_cc(r, 3, ref_cc.default_mask(15)).numpy()
    out["util/pow_adj"] = ref_gu.pow_tensor(a[:, 0], 3).numpy()
    q = torch.tensor([[-0.2, 0.49, 0.5, 1.49], [1.5, 2.49, 2.5, 7.0]])
    out["util/q_in"], out["util/quantize"], out["util/quantize_mol"] = q.numpy(), ref_gu.quantize(q).numpy(), ref_gu.quantize_mol(q)
    np.savez_compressed(os.path.join(GOLD, "g6_masks_utils.npz"), **out)


def g7_init_flags():
    """(f)2: `init_flags` of the reference on the shipped graph datasets (cc_utils.py:883-914 with is_cc=False: graphs_to_tensor +
    np.random.randint over the train split + node_flags, graph_utils.py:62-77), fed by the reference's own
    load_data(config, get_list=True) (data_loader.py:64-88).  One numpy seed per (dataset, batch).  The *_CC pickles hold
    toponetx objects and cannot be read here; the CC branch takes node_flags of the complexes' adjacency (cc_utils.py:909-913),
    i.e. of the same graphs in the same file order, so the graph-dataset flags pin both samplers."""
    from ccsd.src.utils.data_loader import dataloader as ref_dataloader

    out = {}
    meta = {}
    for name, N in (("community_small", 20), ("ego_small", 18), ("ENZYMES_small", 12), ("grid_small", 49)):
        cfg = refshim.EasyDict({"folder": refshim.REFERENCE_ROOT,
                                "data": {"data": name, "dir": "data", "batch_size": 24, "test_split": 0.2, "max_node_num": N}})
        train, test = ref_dataloader(cfg, get_graph_list=True)
        meta[name] = {"max_node_num": N, "n_train": len(train), "n_test": len(test), "cases": []}
        for seed, batch in ((12, None), (42, 7), (42, 64), (42, 128), (2024, 129)):
            np.random.seed(seed)
            fl = ref_cc.init_flags(train, cfg, batch)
            after = int(np.random.randint(0, 1 << 30))          # the stream position the call leaves behind
            key = f"{name}/s{seed}_b{batch or 0}"
            out[key] = fl.numpy().astype(np.float32)
            meta[name]["cases"].append({"seed": seed, "batch": batch, "key": key, "next_randint": after})
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(GOLD, "g7_init_flags.npz"), **out)
    print("wrote g7_init_flags", {k: v["n_train"] for k, v in meta.items()})


def g5_pc_runs(name, ck, is_cc, B, counts, sampler_cfg, cases, seed, min_dist=0.0, summarize_large=False):
    """Wrapper: when `min_dist` is given, the seed is advanced (by 100) until every case's final adjacency stays at least
    that far from every quantisation threshold, so that the bit-exact integer comparison has a margin."""
    for attempt in range(20):
        d = _g5_pc_runs(name, ck, is_cc, B, counts, sampler_cfg, cases, seed + 100 * attempt, summarize_large)
        if d >= min_dist:
            return
        print("g5", name, "seed", seed + 100 * attempt, "too close to a threshold:", d)
    raise RuntimeError("no seed with the requested threshold margin")


def _g5_pc_runs(name, ck, is_cc, B, counts, sampler_cfg, cases, seed, summarize_large=False, flags=None, keep=None):
    """G4/G5: end-to-end sampler runs; inputs are regenerated from the seed by the consumer
    (prior + every in-loop draw come from torch's global CPU generator in reference order).
    `flags`: the node flags to run with (default: make_flags(B, N, counts)).  `keep`: a dict that receives the final tensors of every
    case, {case: {"x", "adj", "rank2"}}; no fixture file is written then (f1_finish / d1_qm9_cc_n1000 reduce them to descriptors).
    sampler_cfg may carry `probability_flow` (default False) and `sde_override` = {part: sde dict} replacing the
    checkpoint's SDE for that part (subVP has no shipped checkpoint: the weights are just weights, the SDE
    arithmetic is what the case pins)."""
    cfg = ck["model_config"]
    N, Fd = cfg["data"]["max_node_num"], cfg["data"]["max_feat_num"]
    d_min, d_max = (cfg["data"]["d_min"], cfg["data"]["d_max"]) if is_cc else (None, None)
    models = build_models(ck, is_cc)
    flags = make_flags(B, N, counts) if flags is None else flags
    out = {"flags": flags.numpy(), "seed": seed, "rng_probe": rng_probe(seed),
           "sampler": json.dumps(sampler_cfg)}
    for case, (num_scales, max_steps) in cases.items():
        sdes = []
        for p in ["x", "adj"] + (["rank2"] if is_cc else []):
            c = dict(cfg["sde"][p])
            c.update(sampler_cfg.get("sde_override", {}).get(p, {}))
            if num_scales is not None:
                c["num_scales"] = num_scales
            sdes.append(ref_loader.load_sde(refshim.EasyDict(c)))
        kw = dict(sde_x=sdes[0], sde_adj=sdes[1], shape_x=(B, N, Fd), shape_adj=(B, N, N),
                  predictor=sampler_cfg["predictor"], corrector=sampler_cfg["corrector"], snr=sampler_cfg["snr"],
                  scale_eps=sampler_cfg["scale_eps"], n_steps=sampler_cfg["n_steps"],
                  probability_flow=bool(sampler_cfg.get("probability_flow", False)),
                  continuous=True, denoise=True, eps=1e-4, device="cpu")
        if is_cc:
            E, K = ref_cc.get_rank2_dim(N, d_min, d_max)
            kw.update(is_cc=True, sde_rank2=sdes[2], shape_rank2=(B, E, K), d_min=d_min, d_max=d_max)
        fn = ref_solver.S4_solver(**kw) if sampler_cfg["predictor"] == "S4" else ref_solver.get_pc_sampler(**kw)
        orig = ref_solver.trange
        if max_steps is not None:
            ref_solver.trange = lambda a, b, **k: range(a, min(b, max_steps))
        else:
            ref_solver.trange = lambda a, b, **k: range(a, b)
        try:
            torch.manual_seed(seed)
            res = fn(*models, flags)
        finally:
            ref_solver.trange = orig
        parts = ["x", "adj"] + (["rank2"] if is_cc else [])
        res = [r.clone() if isinstance(r, torch.Tensor) else r for r in res]  # quantize_mol mutates CPU inputs
        for p, v in zip(parts, res):
            out[f"{case}/{p}"] = v.numpy().copy()
        if keep is not None:
            keep[case] = {p: out[f"{case}/{p}"] for p in parts}
        out[f"{case}/nfe"] = np.array(res[len(parts)])
        traj = res[-1]
        out[f"{case}/traj_len"] = np.array(len(traj))
        out[f"{case}/traj_last_adj"] = traj[-1][1].numpy()
        out[f"{case}/quantize_adj"] = ref_gu.quantize(res[1]).numpy()
        out[f"{case}/quantize_mol_adj"] = ref_gu.quantize_mol(res[1].clone())
        if is_cc:
            out[f"{case}/quantize_rank2"] = ref_gu.quantize(res[2]).numpy().astype(np.uint8)
        # distance of the final adjacency to the nearest quantisation threshold (bit-exactness margin)
        thr = torch.tensor([0.5, 1.5, 2.5])
        out[f"{case}/min_thr_dist"] = np.array((res[1][..., None] - thr).abs().min().item())
        print("g5", name, case, "adj absmax", float(res[1].abs().max()), "min thr dist", float(out[f"{case}/min_thr_dist"]))
    dist = min(float(out[f"{case}/min_thr_dist"]) for case in cases)
    if keep is None:
        save_golden(f"g5_{name}.npz", out, summarize_large)
    return dist


def ref_descriptors(x, adj, rank2, d_min, d_max, mol):
    """Per-complex integer descriptors of finished samples, by the reference's own functions: the quantities its evaluators reduce to
    histograms (degree_worker, stats.py:36; rank1_distrib_worker / rank2_distrib_worker, cc_utils.py:1208-1334).
      degree_hist (B, N)  nx.degree_histogram of adjs_to_graphs(quantize(adj), True) (graph_utils.py:216-251), zero padded; degree_len (B,) its length
      edge_hist (B, 4)    pairs i < j by value of quantize_mol(adj) (mol) / quantize(adj)
      n_nodes (B,)        rows of x with any non-zero entry (cc_from_incidence's node rule, cc_utils.py:199-213)
      x_hist (B, F)       nodes with x[i, f] > 0.5
      cell_hist (B, d_max - d_min + 1)   columns of quantize(rank2) with any() set (cc_utils.py:247-249), by the size of get_cells' cell
      rank2_nnz (B,)      entries of quantize(rank2) that are set"""
    import networkx as nx

    x, adj = torch.as_tensor(x), torch.as_tensor(adj)
    B, N = adj.shape[0], adj.shape[-1]
    graphs = ref_gu.adjs_to_graphs(ref_gu.quantize(adj), True)
    out = {"degree_hist": np.zeros((B, N), np.int32), "degree_len": np.zeros(B, np.int32)}
    for b, G in enumerate(graphs):
        h = nx.degree_histogram(G)
        out["degree_hist"][b, :len(h)] = h
        out["degree_len"][b] = len(h)
    q = torch.as_tensor(ref_gu.quantize_mol(adj.clone())) if mol else ref_gu.quantize(adj).to(torch.int64)
    iu = np.triu_indices(N, 1)
    out["edge_hist"] = np.stack([np.bincount(q[b].numpy()[iu], minlength=4) for b in range(B)]).astype(np.int32)
    out["n_nodes"] = np.array([sum(int(x[b, i, :].any().item()) for i in range(N)) for b in range(B)], np.int32)
    out["x_hist"] = (x > 0.5).sum(dim=1).numpy().astype(np.int32)
    if rank2 is not None:
        cells = ref_cc.get_cells(N, d_min, d_max)[0]
        size = np.array([len(c) for c in cells])
        qr = ref_gu.quantize(torch.as_tensor(rank2))
        active = qr.bool().any(dim=1).numpy()
        out["cell_hist"] = np.stack([np.bincount(size[active[b]] - d_min, minlength=d_max - d_min + 1) for b in range(B)]).astype(np.int32)
        out["rank2_nnz"] = qr.sum(dim=(1, 2)).numpy().astype(np.int32)
    return out


# f1_finish.npz: name -> (checkpoint table, is_cc, B, node counts, sampler, cases, seed, mol): the g5 runs whose finished tensors it reads
F1_RUNS = {
    "ccsd_qm9_CC": (CHECKPOINTS, True, ["k10", "k50", "n1000_first3"], True),
    "ccsd_qm9_CC_full1000": (CHECKPOINTS, True, ["n1000"], True),
    "ccsd_community_small_CC": (CHECKPOINTS, True, ["k5", "n1000_first2"], False),
    "ccsd_ego_small_CC": (SHIPPED, True, ["k6", "n1000_first2"], False),
    "gdss_zinc250k": (CHECKPOINTS, False, ["k5"], True),
    "gdss_grid": (SHIPPED, False, ["n1000_first3"], False),
}


def f1_finish():
    """The reference's descriptors (ref_descriptors) of the reference's finished samples of the g5_* fixtures.  Where a g5 file holds a
    tensor only as a summary (ego_small_CC's rank2, grid's adj) the run is repeated here from the fixture's seed, checked against the
    summary's sha256, and f1 keeps what the descriptors depend on: the bits of quantize(rank2) (np.packbits) / quantize_mol(adj) as int8."""
    import hashlib

    ego = dict(predictor="Euler", corrector="None", snr=0.0, scale_eps=0.0, n_steps=1)
    grid = dict(predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7, n_steps=1)
    rerun = {"ccsd_ego_small_CC": ([18, 9], ego, {"k6": (6, None), "n1000_first2": (None, 2)}),
             "gdss_grid": ([361, 144], grid, {"n1000_first3": (None, 3)})}
    out, meta = {}, {}
    for name, (table, is_cc, cases, mol) in F1_RUNS.items():
        g = np.load(os.path.join(GOLD, f"g5_{name}.npz"))
        ckname = "ccsd_qm9_CC" if name == "ccsd_qm9_CC_full1000" else name
        ck = refshim.load_reference_ckpt(table[ckname][0])
        data = ck["model_config"]["data"]
        d_min, d_max = (int(data["d_min"]), int(data["d_max"])) if is_cc else (0, 0)
        kept = {}
        if name in rerun:
            counts, smp, cs = rerun[name]
            _g5_pc_runs(name, ck, is_cc, 2, counts, smp, cs, int(g["seed"]), keep=kept)
        meta[name] = {"is_cc": is_cc, "mol": mol, "d_min": d_min, "d_max": d_max, "cases": cases, "N": int(data["max_node_num"])}
        for case in cases:
            t = {}
            for p in ["x", "adj"] + (["rank2"] if is_cc else []):
                key = f"{case}/{p}"
                if key in g.files:
                    t[p] = g[key]
                else:
                    t[p] = kept[case][p]
                    assert hashlib.sha256(np.ascontiguousarray(t[p]).tobytes()).hexdigest() == str(g[key + "/sha256"]), (name, key)
                    if p == "rank2":
                        out[f"{name}/{case}/rank2_bits"] = np.packbits(ref_gu.quantize(torch.as_tensor(t[p])).numpy().astype(np.uint8))
                        out[f"{name}/{case}/rank2_shape"] = np.array(t[p].shape)
                    else:
                        out[f"{name}/{case}/adj_qmol"] = ref_gu.quantize_mol(torch.as_tensor(t[p]).clone()).astype(np.int8)
            for k, v in ref_descriptors(t["x"], t["adj"], t.get("rank2"), d_min, d_max, mol).items():
                out[f"{name}/{case}/{k}"] = v
        print("f1", name, cases)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(GOLD, "f1_finish.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_FIXTURE, os.path.getsize(path)
    print("wrote f1_finish", os.path.getsize(path))


# ---------------------------------------------------------------------------------------------
# e1_eval.npz: the reference's evaluators on small graph sets and histogram sets (`python tools/make_golden.py eval`)
# ---------------------------------------------------------------------------------------------
def _pyemd_stand_in(record):
    """pyemd is not installed here.  Stand-in module with pyemd.emd's documented behaviour: the minimum-cost flow between the two
    histograms on the caller's distance matrix, by scipy.optimize.linprog, plus |mass_x - mass_y| times extra_mass_penalty, whose
    default (-1) means max(distance_matrix).  record["tl"].mode == "closed": the closed form on a line metric instead of the program
    (sum |cdf_x - cdf_y| times the unit distance), with the same extra-mass rule; used to measure the difference between the two."""
    import types

    from scipy.optimize import linprog

    def emd(x, y, D, extra_mass_penalty=-1.0):
        x, y, D = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(D, np.float64)
        n = len(x)
        pen = D.max() if extra_mass_penalty == -1.0 else extra_mass_penalty
        mx, my = x.sum(), y.sum()
        extra = abs(mx - my) * pen
        if min(mx, my) == 0.0:
            return float(extra)
        if getattr(record["tl"], "mode", "lp") == "closed":
            assert abs(mx - my) < 1e-6, (x, y)           # (pmfs normalised in float32 miss mass 1 by ~1e-8: the closed form is then approximate)
            unit = D[0, 1] if n > 1 else 0.0
            return float(np.abs(np.cumsum(x) - np.cumsum(y)).sum() * unit + extra)
        A_ub = np.zeros((2 * n, n * n))
        for i in range(n):
            A_ub[i, i * n:(i + 1) * n] = 1.0
            A_ub[n + i, i::n] = 1.0
        res = linprog(D.reshape(-1), A_ub=A_ub, b_ub=np.concatenate([x, y]), A_eq=np.ones((1, n * n)), b_eq=[min(mx, my)],
                      bounds=(0, None), method="highs")
        assert res.status == 0, res.message
        record["programs"] = record.get("programs", 0) + 1
        return float(res.fun + extra)

    m = types.ModuleType("pyemd")
    m.emd = emd
    return m


class _StandInCC:
    """The two members of a toponetx CombinatorialComplex that rank1_distrib_worker, rank2_distrib_worker and is_empty_cc read,
    filled from per-complex counts: n_nodes rank-0 cells, edge_hist[v] rank-1 cells of value v >= 1, cell_hist[s - d_min] rank-2 cells of size s."""

    def __init__(self, n_nodes, edge_hist, cell_hist, d_min):
        import types

        r1 = {}
        for v in range(1, len(edge_hist)):
            for i in range(int(edge_hist[v])):
                r1[frozenset((("e", v, i), ("f", v, i)))] = {"label": v}
        r2 = {}
        for b, c in enumerate(cell_hist):
            for i in range(int(c)):
                r2[frozenset([("c", b, i, j) for j in range(d_min + b)])] = {}
        self.cells = types.SimpleNamespace(hyperedge_dict={0: {frozenset([i]): {} for i in range(int(n_nodes))}, 1: r1, 2: r2})

    def number_of_cells(self):
        return sum(len(v) for v in self.cells.hyperedge_dict.values())


def e1_graph_sets():
    """name -> (adjacency (B, N, N) int8, mol): the graphs of the clustering cases of tests/eval_cases.py."""
    from itertools import combinations

    rng = np.random.default_rng(20261018)

    def sym(B, N, p, masked=0, values=(1,)):
        a = np.zeros((B, N, N), np.int8)
        for b in range(B):
            n = N - masked * b
            u = np.triu((rng.random((n, n)) < p), 1)
            v = rng.choice(np.array(values, np.int8), size=(n, n))
            a[b, :n, :n] = u * v
            a[b] = a[b] + a[b].T
        return a

    def hub(N, inner):
        a = np.zeros((1, N, N), np.int8)
        a[0, 0, 1:] = a[0, 1:, 0] = 1
        for i, j in list(combinations(range(1, N), 2))[:inner]:
            a[0, i, j] = a[0, j, i] = 1
        return a

    sets = {"c07": (hub(6, 7), False),                                  # degree 5, 7 triangles: c = 0.7 -> bin 69 of 100
            "n17": (hub(17, 42), False),                                # degree 16, 42 triangles: c = 0.35 -> bin 34
            "k65": ((1 - np.eye(65, dtype=np.int8))[None], False),      # crosses a mask word; every c = 1 -> bin 99
            "n2": (np.array([[[0, 1], [1, 0]], [[0, 0], [0, 0]], [[1, 1], [1, 1]]], np.int8), False),
            "r65": (sym(3, 65, 0.3, masked=7), False),
            "r130": (sym(2, 130, 0.3, masked=11), False),
            "n512": (sym(2, 512, 0.05, masked=40), False),
            "mol9": (sym(4, 9, 0.45, masked=1, values=(1, 2, 3)), True)}
    small = np.zeros((4, 5, 5), np.int8)                                # edgeless; a single edge; a triangle + tail with a non-zero diagonal; diagonal only
    small[1, 1, 3] = small[1, 3, 1] = 1
    for i, j in ((0, 1), (1, 2), (0, 2), (2, 3)):
        small[2, i, j] = small[2, j, i] = 1
    small[2][np.diag_indices(5)] = 1
    small[3][np.diag_indices(5)] = 1
    sets["small5"] = (small, False)
    d = sym(3, 12, 0.4)
    d[:, np.arange(12), np.arange(12)] = 1
    sets["diag12"] = (d, False)
    # the two sets eval_graph_list scores against each other (the second holds an edgeless graph)
    sets["eval_ref"] = (sym(12, 12, 0.35, masked=0), False)
    pred = sym(9, 12, 0.55, masked=1)
    pred[8] = 0
    sets["eval_pred"] = (pred, False)
    return sets


def e1_mmd_sets():
    """name -> (rows1, rows2, emd): lists of 1-D histograms; emd = whether the linear programs are affordable at this size."""
    rng = np.random.default_rng(1018)

    def rows(n, L, ragged=False, dtype=np.int64, zero=()):
        out = []
        for i in range(n):
            l = int(rng.integers(1, L + 1)) if ragged else L
            r = rng.integers(0, 6, l).astype(dtype)
            if not r.any():
                r[0] = 1
            if i in zero:
                r[:] = 0
            out.append(r)
        return out

    return {"a": (rows(3, 2), rows(1, 2), True),
            "l1": (rows(3, 1), rows(2, 1), True),
            "ragged": (rows(5, 11, ragged=True), rows(3, 9, ragged=True), True),
            "zero_one": (rows(4, 7, dtype=np.float32, zero=(1,)), rows(3, 7, dtype=np.float32), True),      # (float32: the rank-2 worker's dtype)
            "zero_both": (rows(4, 6, ragged=True, zero=(0, 2)), rows(3, 8, ragged=True, zero=(1,)), True),
            "n65": (rows(65, 33), rows(3, 33), True),
            "n130": (rows(130, 100), rows(64, 100), False),
            "l512": (rows(3, 512), rows(1, 512), False),
            "l200": (rows(3, 200, ragged=True), rows(3, 200), False)}


def e1_eval():
    """e1_eval.npz: the reference's own clustering_worker, degree_worker, compute_mmd with gaussian_tv / gaussian / gaussian_emd,
    eval_graph_list and eval_CC_list on small inputs.  gaussian_emd runs on the stand-in pyemd above; meta holds the largest
    difference between its linear programs and the closed form, per kernel value and per score."""
    import time

    import threading

    record = {"tl": threading.local()}          # (disc() runs the kernel on a thread pool: the mode is per thread)
    sys.modules["pyemd"] = _pyemd_stand_in(record)
    from ccsd.src.evaluation import mmd as ref_mmd
    from ccsd.src.evaluation import stats as ref_stats

    ref_mmd.pyemd = sys.modules["pyemd"]
    t0 = time.time()
    out, meta = {}, {"graph_sets": {}, "mmd_sets": {}, "scores": {}, "lp_vs_closed": {}, "lp_vs_closed_kernel": 0.0, "lp_vs_closed_score": 0.0}

    def k_closed(x, y, **kw):        # gaussian_emd with the closed form behind pyemd.emd
        record["tl"].mode = "closed"
        try:
            return ref_mmd.gaussian_emd(x, y, **kw)
        finally:
            record["tl"].mode = "lp"

    def k_emd(x, y, **kw):           # gaussian_emd under both stand-ins: the program's value is the one returned
        kc = k_closed(x, y, **kw)
        kl = ref_mmd.gaussian_emd(x, y, **kw)
        meta["lp_vs_closed_kernel"] = max(meta["lp_vs_closed_kernel"], abs(float(kl) - float(kc)))
        return kl

    def closed(fn):
        return fn(k_closed)

    def emd_score(fn, tag):
        """fn(kernel) -> score: with the linear programs (returned) and with the closed form; meta["lp_vs_closed"][tag] = the largest
        |program - closed form| over the kernel values of this score, lp_vs_closed_kernel / _score the largest over all scores."""
        before, meta["lp_vs_closed_kernel"] = meta["lp_vs_closed_kernel"], 0.0
        lp = float(fn(k_emd))
        meta["lp_vs_closed"][tag] = meta["lp_vs_closed_kernel"]
        meta["lp_vs_closed_kernel"] = max(before, meta["lp_vs_closed_kernel"])
        meta["lp_vs_closed_score"] = max(meta["lp_vs_closed_score"], abs(lp - float(closed(fn))))
        return lp

    # ---- graphs: clustering_worker / degree_worker per graph
    graphs = {}
    for name, (adj, mol) in e1_graph_sets().items():
        out[f"graphs/{name}/adj"] = adj
        meta["graph_sets"][name] = {"mol": mol, "N": int(adj.shape[1]), "B": int(adj.shape[0])}
        q = ref_gu.quantize_mol(torch.as_tensor(adj, dtype=torch.float32)) if mol else ref_gu.quantize(torch.as_tensor(adj, dtype=torch.float32)).numpy()
        G = ref_gu.adjs_to_graphs(np.asarray(q, np.float32))
        graphs[name] = G
        for bins in (10, 100):
            out[f"graphs/{name}/cluster_hist{bins}"] = np.stack([ref_stats.clustering_worker((g, bins)) for g in G]).astype(np.int32)
        dh = np.zeros((len(G), adj.shape[1]), np.int32)
        dl = np.zeros(len(G), np.int32)
        for b, g in enumerate(G):
            h = ref_stats.degree_worker(g)
            dh[b, :len(h)], dl[b] = h, len(h)
        out[f"graphs/{name}/degree_hist"], out[f"graphs/{name}/degree_len"] = dh, dl
    # ---- eval_graph_list on two graph sets
    gr, gp = graphs["eval_ref"], graphs["eval_pred"]
    sc = meta["scores"]
    sc["degree/emd"] = emd_score(lambda k: ref_stats.degree_stats(gr, gp, k), "degree/emd")
    sc["cluster/emd"] = emd_score(lambda k: ref_stats.clustering_stats(gr, gp, k), "cluster/emd")
    sc["cluster10/emd"] = emd_score(lambda k: ref_stats.clustering_stats(gr, gp, k, bins=10), "cluster10/emd")
    sc["degree/tv"] = float(ref_stats.degree_stats(gr, gp, ref_mmd.gaussian_tv))
    sc["cluster/tv"] = float(ref_stats.clustering_stats(gr, gp, ref_mmd.gaussian_tv))
    meta["eval_graph_list"] = ref_stats.eval_graph_list(gr, gp, methods=["degree", "cluster"], kernels={"degree": k_emd, "cluster": k_emd})
    # ---- compute_mmd on histogram sets
    for name, (r1, r2, with_emd) in e1_mmd_sets().items():
        for side, rows in (("1", r1), ("2", r2)):
            L = max(len(r) for r in rows)
            pad = np.zeros((len(rows), L), rows[0].dtype)
            for i, r in enumerate(rows):
                pad[i, :len(r)] = r
            out[f"mmd/{name}/rows{side}"], out[f"mmd/{name}/lens{side}"] = pad, np.array([len(r) for r in rows], np.int32)
        meta["mmd_sets"][name] = {"emd": with_emd, "dtype": str(r1[0].dtype)}
        for sigma, scale in ((1.0, 1.0), (0.1, 100.0)):
            tag = f"mmd/{name}/s{sigma:g}_d{scale:g}"
            sc[tag + "/tv"] = float(ref_mmd.compute_mmd(r1, r2, kernel=ref_mmd.gaussian_tv, sigma=sigma))
            sc[tag + "/l2"] = float(ref_mmd.compute_mmd(r1, r2, kernel=ref_mmd.gaussian, sigma=sigma))
            if with_emd:
                sc[tag + "/emd"] = emd_score(lambda k: ref_mmd.compute_mmd(r1, r2, kernel=k, sigma=sigma, distance_scaling=scale), tag + "/emd")
        # raw vectors (orbit_stats_all's call: is_hist=False, sigma=30)
        f1_, f2_ = [r.astype(np.float64) * 7.5 for r in r1], [r.astype(np.float64) * 7.5 for r in r2]
        sc[f"mmd/{name}/raw_s30/l2"] = float(ref_mmd.compute_mmd(f1_, f2_, kernel=ref_mmd.gaussian, is_hist=False, sigma=30.0))
        print("e1 mmd", name, round(time.time() - t0, 1), "s", record.get("programs", 0), "programs")
    # ---- eval_CC_list over the descriptors of f1_finish.npz (qm9_CC: bonds 1..3, cells of 3..9 nodes)
    f1 = np.load(os.path.join(GOLD, "f1_finish.npz"))
    d_min, d_max = 3, 9
    cc_sets = {"ref": [("ccsd_qm9_CC", "k10"), ("ccsd_qm9_CC", "k50")], "pred": [("ccsd_qm9_CC", "n1000_first3"), ("ccsd_qm9_CC_full1000", "n1000")]}
    wk = {"min_edge_val": 1, "max_edge_val": 3, "edge_label": "label", "d_min": d_min, "d_max": d_max}
    desc = {side: {k: np.concatenate([f1[f"{n}/{c}/{k}"] for n, c in parts]) for k in ("n_nodes", "edge_hist", "cell_hist")} for side, parts in cc_sets.items()}
    meta["cc_sets"], meta["cc_worker_kwargs"] = cc_sets, wk

    def ccs(d, extra_empty):
        cc = [_StandInCC(d["n_nodes"][b], d["edge_hist"][b], d["cell_hist"][b], d_min) for b in range(len(d["n_nodes"]))]
        return cc + [_StandInCC(0, [0, 0, 0, 0], [0] * (d_max - d_min + 1), d_min)] * extra_empty

    kern = {"rank1_distrib": k_emd, "rank2_distrib": k_emd}
    for tag, er, ep, nb in (("plain", 0, 0, 1000), ("empties", 1, 1, 1000), ("first5", 0, 0, 5)):
        # ("empties": one complex without any cell appended to each side -- kept in the reference set, dropped from the predictions)
        meta[f"eval_CC_list/{tag}"] = ref_cc.eval_CC_list(ccs(desc["ref"], er), ccs(desc["pred"], ep), wk, methods=["rank1_distrib", "rank2_distrib"],
                                                          kernels=kern, cc_nb_eval=nb)
        sc[f"cc/{tag}/rank2/emd"] = emd_score(lambda k: ref_cc.rank2_distrib_stats(ccs(desc["ref"], er)[:nb], ccs(desc["pred"], ep)[:nb], wk, k), f"cc/{tag}/rank2/emd")
        sc[f"cc/{tag}/rank1/emd"] = emd_score(lambda k: ref_cc.rank1_distrib_stats(ccs(desc["ref"], er)[:nb], ccs(desc["pred"], ep)[:nb], wk, k), f"cc/{tag}/rank1/emd")
    meta["programs"] = record.get("programs", 0)
    meta["seconds"] = round(time.time() - t0, 1)
    meta["note"] = ("gaussian_emd ran on a stand-in pyemd (scipy.optimize.linprog on the reference's distance matrix, extra mass at pyemd's "
                    "documented default penalty max(distance_matrix)); lp_vs_closed_* = largest |program - closed form| seen here")
    out["meta"] = np.array(json.dumps(plain(meta)))
    path = os.path.join(GOLD, "e1_eval.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_FIXTURE, os.path.getsize(path)
    print("wrote e1_eval", os.path.getsize(path), "bytes;", meta["programs"], "programs,", meta["seconds"], "s; lp vs closed form:",
          meta["lp_vs_closed_kernel"], "(kernel)", meta["lp_vs_closed_score"], "(score)")


# ---------------------------------------------------------------------------------------------
# e3_orbit.npz: the reference's orbit counter and orbit_stats_all on the graph sets of e1_eval.npz (`python tools/make_golden.py orbit`)
# ---------------------------------------------------------------------------------------------
def e3_six4():
    """six4 (6, 4, 4): the six connected graphs on 4 nodes -- K4, C4, claw (centre 0), paw (triangle 0 1 2, tail 2 -- 3), diamond
    (0 and 1 of degree 3), P4 (0 - 1 - 2 - 3)."""
    edges = [[(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)], [(0, 1), (1, 2), (2, 3), (3, 0)], [(0, 1), (0, 2), (0, 3)],
             [(0, 1), (1, 2), (0, 2), (2, 3)], [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)], [(0, 1), (1, 2), (2, 3)]]
    a = np.zeros((6, 4, 4), np.int8)
    for b, es in enumerate(edges):
        for i, j in es:
            a[b, i, j] = a[b, j, i] = 1
    return a


def e3_orbit():
    """e3_orbit.npz: `orca node 4` of the reference's own counter on adjs_to_graphs of every graph set of e1_eval.npz and of six4, and
    the reference's orbit_stats_all / eval_graph_list on eval_ref against eval_pred.  The counter is compiled, at generation time only,
    into a temporary folder laid out as <tmp>/ccsd/src/evaluation/orca/ (orbit_stats_all writes its edge lists next to the binary and
    takes the folder above as `folder`); nothing compiled or copied from the reference is kept."""
    import tempfile
    import threading
    import time

    record = {"tl": threading.local()}
    sys.modules["pyemd"] = _pyemd_stand_in(record)
    from ccsd.src.evaluation import mmd as ref_mmd
    from ccsd.src.evaluation import stats as ref_stats

    ref_mmd.pyemd = sys.modules["pyemd"]
    e1 = np.load(os.path.join(GOLD, "e1_eval.npz"))
    e1_meta = json.loads(str(e1["meta"]))
    out, meta = {}, {"graph_sets": {}, "seconds": {}}
    with tempfile.TemporaryDirectory() as tmp:
        orca_dir = os.path.join(tmp, "ccsd", "src", "evaluation", "orca")
        os.makedirs(orca_dir)
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-o", os.path.join(orca_dir, "orca"),
                               os.path.join(refshim.REFERENCE_ROOT, "ccsd", "src", "evaluation", "orca", "orca.cpp")])
        sets = {name: (e1[f"graphs/{name}/adj"], e1_meta["graph_sets"][name]["mol"]) for name in e1_meta["graph_sets"]}
        sets["six4"] = (e3_six4(), False)
        out["graphs/six4/adj"] = sets["six4"][0]
        graphs = {}
        for name, (adj, mol) in sets.items():
            t0 = time.time()
            q = ref_gu.quantize_mol(torch.as_tensor(adj, dtype=torch.float32)) if mol else ref_gu.quantize(torch.as_tensor(adj, dtype=torch.float32)).numpy()
            q = np.asarray(q, np.float32)
            G = graphs[name] = ref_gu.adjs_to_graphs(q)
            B, N = adj.shape[:2]
            rows, nodes = np.zeros((B, N, 15), np.int64), np.zeros(B, np.int32)
            for b, g in enumerate(G):
                nodes[b] = g.number_of_nodes()
                if g.number_of_edges() == 0:
                    continue                       # (the one-node stand-in of an edgeless graph: every count is 0)
                cnt = ref_stats.orca(g, orca_dir)
                # orca's row r belongs to the r-th node of G.nodes() (edge_list_reindexed); a node of G is a slot of the adjacency
                slots = list(g.nodes())
                assert cnt.shape == (len(slots), 15) and slots == sorted(slots), (name, b)
                rows[b, slots] = cnt
            small = np.abs(rows).max() < 2 ** 31
            out[f"graphs/{name}/orca"] = rows.astype(np.int32) if small and rows.size > 100000 else rows
            out[f"graphs/{name}/nodes"] = nodes
            meta["graph_sets"][name] = {"mol": bool(mol), "N": int(N), "B": int(B)}
            meta["seconds"][name] = round(time.time() - t0, 3)           # (this machine's CPU: the reference's program, one process per graph)
            print("e3", name, meta["seconds"][name], "s")
        gr, gp = graphs["eval_ref"], graphs["eval_pred"]
        totals = {}
        real_compute = ref_stats.compute_mmd

        def spy(s1, s2, **kw):                     # orbit_stats_all's own rows, as it hands them to compute_mmd
            if kw.get("is_hist") is False:
                totals["ref"], totals["pred"] = np.array(s1, np.float64), np.array(s2, np.float64)
            return real_compute(s1, s2, **kw)

        ref_stats.compute_mmd = spy
        try:
            meta["orbit_stats_all"] = float(ref_stats.orbit_stats_all(gr, gp, ref_mmd.gaussian, folder=tmp))
        finally:
            ref_stats.compute_mmd = real_compute
        out["total_counts_ref"], out["total_counts_pred"] = totals["ref"], totals["pred"]
        meta["orbit_self"] = float(ref_stats.orbit_stats_all(gr, gr, ref_mmd.gaussian, folder=tmp))
        _, kernels = ref_loader.load_eval_settings("")
        assert kernels["orbit"] is ref_mmd.gaussian or kernels["orbit"].__name__ == "gaussian"
        meta["eval_graph_list"] = ref_stats.eval_graph_list(gr, gp, methods=["degree", "cluster", "orbit"],
                                                            kernels={"degree": ref_mmd.gaussian_emd, "cluster": ref_mmd.gaussian_emd,
                                                                     "orbit": ref_mmd.gaussian}, folder=tmp)
    meta["note"] = ("orca = the rows `orca node 4` prints for adjs_to_graphs of each graph, scattered to node slots (zeros for removed slots); "
                    "nodes = G.number_of_nodes(); total_counts_* = the rows orbit_stats_all hands to compute_mmd; gaussian_emd ran on a stand-in "
                    "pyemd (scipy.optimize.linprog), as in e1_eval.npz; seconds = the reference's counter per set on the generating machine's CPU")
    out["meta"] = np.array(json.dumps(plain(meta)))
    path = os.path.join(GOLD, "e3_orbit.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_FIXTURE // 4, os.path.getsize(path)
    print("wrote e3_orbit", os.path.getsize(path), "bytes; orbit_stats_all", meta["orbit_stats_all"], meta["eval_graph_list"])


# ---------------------------------------------------------------------------------------------
# e4_nspdk.npz: the reference's NSPDK vectoriser and compute_nspdk_mmd on the graph sets of tests/nspdk_cases.py
# (`python tools/make_golden.py nspdk`)
# ---------------------------------------------------------------------------------------------
def e4_graphs(adj, labels):
    """networkx graphs of a set: a slot with a non-negative label is a node carrying that INTEGER as its label (hash(int) is the int:
    the vectoriser's rows do not depend on the process); an edge between two nodes carries the bond order as its label."""
    import networkx as nx

    graphs = []
    for a, l in zip(adj, labels):
        g = nx.Graph()
        for i in np.nonzero(l >= 0)[0]:
            g.add_node(int(i), label=int(l[i]))
        for i, j in zip(*np.nonzero(np.triu(a, 1))):
            if l[i] >= 0 and l[j] >= 0:
                g.add_edge(int(i), int(j), label=int(a[i, j]))
        graphs.append(g)
    return graphs


def e4_nspdk():
    """e4_nspdk.npz: per graph set the adjacency and labels (as tests/nspdk_cases.py generates them), the CSR rows of the reference's
    vectorize(graphs, complexity=4, discrete=True), its compute_nspdk_mmd for the first half of the set against the rest and for mol9
    against itself, and the difference between that pairwise form and the float64 mean form of the reference's own rows."""
    import time

    sys.path.insert(0, ROOT)
    from tests import nspdk_cases as nc
    from tests import nspdk_ref

    record = {"tl": __import__("threading").local()}
    sys.modules.setdefault("pyemd", _pyemd_stand_in(record))
    from ccsd.src.evaluation import eden as ref_eden
    from ccsd.src.evaluation import mmd as ref_mmd

    out, meta = {}, {"sets": {}}
    graphs = {}
    for name, (adj, lab) in nc.graph_sets().items():
        G = graphs[name] = e4_graphs(adj, lab)
        t0 = time.time()
        X = ref_eden.vectorize(G, complexity=4, discrete=True).tocsr()
        sec = time.time() - t0
        X.sort_indices()
        assert X.shape == (len(G), 65537) and (X.data > 0).all()
        out[f"{name}/adj"], out[f"{name}/labels"] = adj.astype(np.int8), lab.astype(np.int32)
        out[f"{name}/indptr"], out[f"{name}/indices"], out[f"{name}/values"] = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.float64)
        s1, s2 = nc.split(name)
        mmd = float(ref_mmd.compute_nspdk_mmd(G[s1], G[s2], metric="nspdk", is_hist=False, n_jobs=None))
        rows = (out[f"{name}/indptr"], out[f"{name}/indices"], out[f"{name}/values"])
        cut = lambda sl: (rows[0][sl.start:sl.stop + 1] - rows[0][sl.start], rows[1][rows[0][sl.start]:rows[0][sl.stop]], rows[2][rows[0][sl.start]:rows[0][sl.stop]])
        mean_form = nspdk_ref.mmd_mean_form(cut(s1), cut(s2))[3]
        meta["sets"][name] = {"B": int(adj.shape[0]), "N": int(adj.shape[1]), "nnz": int(X.nnz), "max_row_nnz": int(np.diff(X.indptr).max()), "mmd": mmd,
                              "pairwise_minus_mean_form": mmd - mean_form, "vectorize_seconds": round(sec, 3)}
        print("e4", name, meta["sets"][name])
    meta["self"] = {"set": "mol9", "mmd": float(ref_mmd.compute_nspdk_mmd(graphs["mol9"], graphs["mol9"], metric="nspdk", is_hist=False, n_jobs=None))}
    meta["note"] = ("indptr / indices / values = the CSR rows of the reference's vectorize(graphs, complexity=4, discrete=True) on networkx graphs whose "
                    "node labels are the integers of `labels` (negative: no node) and whose edge labels are the bond orders of `adj`; mmd = "
                    "compute_nspdk_mmd(first half, rest, metric='nspdk'); vectorize_seconds = the reference's vectoriser on the generating machine's CPU")
    out["meta"] = np.array(json.dumps(plain(meta)))
    path = os.path.join(GOLD, "e4_nspdk.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_FIXTURE // 2, os.path.getsize(path)
    print("wrote e4_nspdk", os.path.getsize(path), "bytes; self", meta["self"])


# ---------------------------------------------------------------------------------------------
# e2_spectrum.npz: the reference's two spectral evaluators on small sets (`python tools/make_golden.py spectrum`)
# ---------------------------------------------------------------------------------------------
class _StandInComplex:
    """toponetx's CombinatorialComplex as far as cc_from_incidence, CC_to_incidence_matrices, is_empty_cc and the workers of
    eval_CC_list use it: add_cell(cell, rank, **attributes) files the attributes under cells.hyperedge_dict[rank][frozenset(cell)].
    (Whether toponetx adds the nodes of a higher cell that were never added as rank-0 cells does not matter here: every set below keeps
    the nodes of its edges and cells among its rank-0 cells, which are the first n indices -- what masked samples look like.)"""

    def __init__(self):
        import types

        self.cells = types.SimpleNamespace(hyperedge_dict={})

    def add_cell(self, cell, rank, **attr):
        self.cells.hyperedge_dict.setdefault(rank, {})[frozenset(cell)] = attr

    def number_of_cells(self):
        return sum(len(v) for v in self.cells.hyperedge_dict.values())


def e2_graph_sets():
    """name -> (adjacency (B, N, N) int8, mol, exact): `exact` sets are compared count by count (no bipartite component, margin checked)."""
    e1 = e1_graph_sets()
    sets = {k: (e1[k][0], e1[k][1], True) for k in ("mol9", "r65", "diag12")}

    def sym(rng, B, N, p, masked=0):
        a = np.zeros((B, N, N), np.int8)
        for b in range(B):
            n = N - masked * b
            u = np.triu((rng.random((n, n)) < p), 1)
            a[b, :n, :n] = u
            a[b] = a[b] + a[b].T
        return a

    # (seeds: the first of 0, 1, 2, ... whose set passes the margin and bipartite checks of e2_spectrum, searched there)
    sets["n125"] = (lambda rng: sym(rng, 2, 125, 0.08, masked=9), False, True)
    sets["s12a"] = (lambda rng: sym(rng, 4, 12, 0.4, masked=1), False, True)
    sets["s12b"] = (lambda rng: sym(rng, 3, 12, 0.6, masked=2), False, True)
    # bipartite landmarks (eigenvalue 2 exactly): path, even cycle, star, 3 x 4 grid, and a path beside a cycle (two components)
    N = 12
    bip = np.zeros((5, N, N), np.int8)

    def edge(b, i, j):
        bip[b, i, j] = bip[b, j, i] = 1

    for i in range(5):
        edge(0, i, i + 1)
    for i in range(8):
        edge(1, i, (i + 1) % 8)
    for i in range(1, 7):
        edge(2, 0, i)
    for r in range(3):
        for c in range(4):
            if c < 3:
                edge(3, 4 * r + c, 4 * r + c + 1)
            if r < 2:
                edge(3, 4 * r + c, 4 * r + c + 4)
    for i in range(3):
        edge(4, i, i + 1)
    for i in range(6):
        edge(4, 4 + i, 4 + (i + 1) % 6)
    sets["bip"] = (bip, False, False)
    return sets


def e2_complex_sets():
    """name -> (N, d_min, d_max, node counts of the ref side, of the pred side, seed)."""
    return {"e10": (5, 3, 4, [5, 4, 5], [5, 3], 1), "e36": (9, 3, 5, [9, 8, 7], [9, 6, 9], 2), "e66": (12, 3, 4, [12, 10], [11, 12], 3),
            "e190": (20, 3, 3, [20, 17], [18, 20], 4)}


def e2_spectrum():
    """e2_spectrum.npz: spectral_worker / spectral_stats / eval_graph_list on graph sets and hodge_laplacian_spectrum_worker /
    hodge_laplacian_spectrum_stats / eval_CC_list on complex sets, from the reference itself (networkx, scipy, torch on the host;
    gaussian_emd on the stand-in pyemd, the complexes on _StandInComplex)."""
    import threading
    import time
    from itertools import combinations

    import networkx as nx
    from scipy.linalg import eigvalsh as sp_eigvalsh

    record = {"tl": threading.local()}
    stand_in = _pyemd_stand_in(record)
    raw_emd, memo, lock = stand_in.emd, {}, threading.Lock()

    def emd(x, y, D, extra_mass_penalty=-1.0):       # (the same pair of rows comes back in eval_*_list: one program per pair)
        key = (getattr(record["tl"], "mode", "lp"), np.asarray(x).tobytes(), np.asarray(y).tobytes(), float(np.asarray(D).max()))
        with lock:
            if key in memo:
                return memo[key]
        v = raw_emd(x, y, D, extra_mass_penalty)
        with lock:
            memo[key] = v
        return v

    stand_in.emd = emd
    sys.modules["pyemd"] = stand_in
    from ccsd.src.evaluation import mmd as ref_mmd
    from ccsd.src.evaluation import stats as ref_stats

    ref_mmd.pyemd = stand_in
    ref_cc.CombinatorialComplex = _StandInComplex
    t0 = time.time()
    out = {}
    meta = {"graph_sets": {}, "complex_sets": {}, "scores": {}, "lp_vs_closed": {}, "f32_vs_f64": {}, "lp_vs_closed_kernel": 0.0}

    def k_closed(x, y, **kw):
        record["tl"].mode = "closed"
        try:
            return ref_mmd.gaussian_emd(x, y, **kw)
        finally:
            record["tl"].mode = "lp"

    def k_emd(x, y, **kw):
        kc = k_closed(x, y, **kw)
        kl = ref_mmd.gaussian_emd(x, y, **kw)
        meta["lp_vs_closed_kernel"] = max(meta["lp_vs_closed_kernel"], abs(float(kl) - float(kc)))
        return kl

    def emd_score(fn, tag):
        before, meta["lp_vs_closed_kernel"] = meta["lp_vs_closed_kernel"], 0.0
        lp = float(fn(k_emd))
        meta["lp_vs_closed"][tag] = meta["lp_vs_closed_kernel"]
        meta["lp_vs_closed_kernel"] = max(before, meta["lp_vs_closed_kernel"])
        return lp

    # ---- graphs
    BINS, RANGE = 200, (-1e-5, 2)
    interior = np.linspace(RANGE[0], RANGE[1], BINS + 1)[1:-1]

    def restated(adj, mol):
        """(counts, eigenvalues, n_eff) per graph in float64 with the clamp to [0, 2]: the definition of include/ccsd_hip.h."""
        cs, es, ns = [], [], []
        for a in adj:
            w = a.astype(np.float64) * (1 - np.eye(len(a)))
            if not mol:
                w = (w != 0).astype(np.float64)
            keep = w.sum(1) > 0
            w = w[keep][:, keep]
            if not keep.any():
                ev_ = np.zeros(1)
            else:
                d = w.sum(1)
                ev_ = np.linalg.eigvalsh(np.eye(len(d)) - w / np.sqrt(d[:, None] * d[None, :]))
            ev_ = np.clip(ev_, 0.0, 2.0)
            cs.append(np.histogram(ev_, bins=BINS, range=RANGE)[0])
            es.append(np.pad(ev_, (0, len(a) - len(ev_))))
            ns.append(len(ev_))
        return np.stack(cs).astype(np.int32), np.stack(es), np.array(ns, np.int32)

    def reference_graphs(adj, mol):
        q = ref_gu.quantize_mol(torch.as_tensor(adj, dtype=torch.float32)) if mol else ref_gu.quantize(torch.as_tensor(adj, dtype=torch.float32)).numpy()
        return ref_gu.adjs_to_graphs(np.asarray(q, np.float32))

    def reference_spectra(G, N):
        counts, eigs, n_eff = [], [], []
        for g in G:
            e = sp_eigvalsh(nx.normalized_laplacian_matrix(g).todense())           # spectral_worker's own first line
            c = np.histogram(e, bins=BINS, range=RANGE, density=False)[0]
            pmf = ref_stats.spectral_worker(g)
            assert np.array_equal(pmf, c / c.sum())
            counts.append(c)
            eigs.append(np.pad(e, (0, N - len(e))))
            n_eff.append(len(e))
        return np.stack(counts).astype(np.int32), np.stack(eigs), np.array(n_eff, np.int32)

    def margin_ok(G, eigs, n_eff):
        gap = min(np.abs(e[:n, None] - interior[None]).min() for e, n in zip(eigs, n_eff))
        bip = any(nx.is_bipartite(g.subgraph(c)) and len(c) > 1 for g in G for c in nx.connected_components(g))
        return gap, bip

    graphs = {}
    for name, (adj, mol, exact) in e2_graph_sets().items():
        seed = None
        if callable(adj):
            make = adj
            for seed in range(1000):
                adj = make(np.random.default_rng(20261019 + seed))
                G = reference_graphs(adj, mol)
                gap, bip = margin_ok(G, *reference_spectra(G, adj.shape[1])[1:])
                if gap >= 1e-9 and not bip:
                    break
            else:
                raise RuntimeError(name)
        G = reference_graphs(adj, mol)
        counts, eigs, n_eff = reference_spectra(G, adj.shape[1])
        gap, bip = margin_ok(G, eigs, n_eff)
        if exact and (gap < 1e-9 or bip):
            print("e2:", name, "fails the margin / bipartite check (gap", gap, "bipartite", bip, "): not compared count by count")
            exact = False
        rc, re_, rn = restated(adj, mol)
        assert np.array_equal(rn, n_eff), name
        if exact:
            assert np.array_equal(rc, counts), name
        graphs[name] = G
        out[f"graphs/{name}/adj"] = adj
        out[f"graphs/{name}/counts"], out[f"graphs/{name}/eig"], out[f"graphs/{name}/n_eff"] = counts, eigs, n_eff
        if not exact:
            out[f"graphs/{name}/expected_counts"] = rc
        meta["graph_sets"][name] = {"mol": mol, "N": int(adj.shape[1]), "B": int(adj.shape[0]), "exact": bool(exact), "seed": seed,
                                    "edge_margin": float(gap), "bipartite_component": bool(bip),
                                    "restated_vs_reference_eig": float(np.abs(re_ - np.clip(eigs, 0, 2)).max()),
                                    # informational: did np.histogram keep every eigenvalue of the reference (a top eigenvalue above 2 is dropped)
                                    "reference_kept_all": [bool(c.sum() == n) for c, n in zip(counts, n_eff)]}
        print("e2 graphs", name, "gap", gap, "bipartite", bip, round(time.time() - t0, 1), "s")
    meta["edge_margin_required"] = 1e-9
    meta["edge_margin_ok"] = all(v["edge_margin"] >= 1e-9 for v in meta["graph_sets"].values() if v["exact"])
    assert meta["edge_margin_ok"]
    sc = meta["scores"]
    for a, b in (("s12a", "s12b"), ("mol9", "s12b")):
        gr, gp = graphs[a], graphs[b]
        sc[f"spectral/{a}_{b}/emd"] = emd_score(lambda k: ref_stats.spectral_stats(gr, gp, k), f"spectral/{a}_{b}/emd")
        sc[f"spectral/{a}_{b}/tv"] = float(ref_stats.spectral_stats(gr, gp, ref_mmd.gaussian_tv))
        print("e2 spectral", a, b, round(time.time() - t0, 1), "s", record.get("programs", 0), "programs")
    meta["eval_graph_list"] = ref_stats.eval_graph_list(graphs["s12a"], graphs["s12b"], methods=["degree", "cluster", "spectral"],
                                                        kernels={"degree": k_emd, "cluster": k_emd, "spectral": k_emd})
    for m in ("degree", "cluster"):
        meta["lp_vs_closed"][f"eval_graph_list/{m}"] = meta["lp_vs_closed_kernel"]
    # ---- complexes
    def make_side(rng, N, d_min, d_max, counts):
        cells = [c for d in range(d_min, d_max + 1) for c in combinations(range(N), d)]
        edges = {e: i for i, e in enumerate(combinations(range(N), 2))}
        E, K = len(edges), len(cells)
        x = np.zeros((len(counts), N, 1), np.int8)
        adj = np.zeros((len(counts), N, N), np.int8)
        r2 = np.zeros((len(counts), E, K), np.int8)
        for b, n in enumerate(counts):
            x[b, :n] = 1
            u = np.triu(rng.random((n, n)) < 0.55, 1)
            adj[b, :n, :n] = u + u.T
            ok = [k for k, c in enumerate(cells) if max(c) < n]
            for k in rng.choice(ok, size=min(len(ok), int(rng.integers(2, 7))), replace=False) if b != 1 else []:
                # (a present cell is a column with any entry: the entries sit on the cell's own edges, present in the graph or not)
                rows = [edges[e] for e in combinations(cells[k], 2)]
                r2[b, rng.choice(rows, size=int(rng.integers(1, len(rows) + 1)), replace=False), k] = 1
        return x, adj, r2

    def to_ccs(x, adj, r2, d_min, d_max, empties=0):
        ccs = [ref_cc.cc_from_incidence([x[b].astype(np.float32), adj[b].astype(np.float32), r2[b].astype(np.float32)], d_min, d_max)
               for b in range(len(x))]
        return ccs + [_StandInComplex() for _ in range(empties)]

    def f64_rows(ccs, d_min, d_max, N):
        rows = []
        for cc in ccs:
            F = ref_cc.CC_to_incidence_matrices(cc, d_min, d_max)[2]
            if F.size:
                F = np.asarray(ref_cc.pad_rank2(F, node_number=N, d_min=d_min, d_max=d_max), np.float64)
                rows.append(np.linalg.eigvalsh(F @ F.T))
            else:
                rows.append(np.zeros(N * (N - 1) // 2))
        return rows

    for name, (N, d_min, d_max, n_ref, n_pred, seed) in e2_complex_sets().items():
        rng = np.random.default_rng(20261019 + seed)
        wk = {"min_edge_val": 1, "max_edge_val": 1, "edge_label": "label", "d_min": d_min, "d_max": d_max, "N": N}
        sides = {"ref": make_side(rng, N, d_min, d_max, n_ref), "pred": make_side(rng, N, d_min, d_max, n_pred)}
        worst = 0.0
        for side, (x, adj, r2) in sides.items():
            ccs = to_ccs(x, adj, r2, d_min, d_max)
            spec = np.stack([ref_cc.hodge_laplacian_spectrum_worker(cc, d_min, d_max, N) for cc in ccs])
            assert spec.dtype == np.float32 and spec.shape == (len(x), N * (N - 1) // 2)
            f64 = np.stack(f64_rows(ccs, d_min, d_max, N))
            worst = max(worst, float(np.abs(spec.astype(np.float64) - f64).max()))
            out[f"cc/{name}/{side}/x"], out[f"cc/{name}/{side}/adj"], out[f"cc/{name}/{side}/rank2"] = x, adj, r2
            out[f"cc/{name}/{side}/spectrum"] = spec
        meta["f32_vs_f64"][f"cc/{name}/eig"] = worst
        meta["complex_sets"][name] = {"N": N, "d_min": d_min, "d_max": d_max, "E": N * (N - 1) // 2, "worker_kwargs": wk}
        kern = {m: k_emd for m in ("hodge_laplacian_spectrum", "rank1_distrib", "rank2_distrib")}
        for tag, er, ep, nb in (("plain", 0, 0, 1000), ("empties", 1, 1, 1000), ("first2", 0, 0, 2)):
            cr, cp = to_ccs(*sides["ref"], d_min, d_max, er)[:nb], to_ccs(*sides["pred"], d_min, d_max, ep)[:nb]
            key = f"cc/{name}/{tag}/hodge/emd"
            sc[key] = emd_score(lambda k: ref_cc.hodge_laplacian_spectrum_stats(cr, cp, wk, k, is_parallel=False), key)
            sc[f"cc/{name}/{tag}/hodge/tv"] = float(ref_cc.hodge_laplacian_spectrum_stats(cr, cp, wk, ref_mmd.gaussian_tv, is_parallel=False))
            # the same scores from float64 eigenvalues rounded to float32 once
            rows = [[r.astype(np.float32) for r in f64_rows(c, d_min, d_max, N)] for c in (cr, [c for c in cp if not ref_cc.is_empty_cc(c)])]
            alt = float(ref_mmd.compute_mmd(rows[0], rows[1], kernel=k_emd))
            alt_tv = float(ref_mmd.compute_mmd(rows[0], rows[1], kernel=ref_mmd.gaussian_tv))
            meta["f32_vs_f64"][key] = abs(alt - sc[key])
            meta["f32_vs_f64"][f"cc/{name}/{tag}/hodge/tv"] = abs(alt_tv - sc[f"cc/{name}/{tag}/hodge/tv"])
            meta[f"eval_CC_list/{name}/{tag}"] = ref_cc.eval_CC_list(to_ccs(*sides["ref"], d_min, d_max, er), to_ccs(*sides["pred"], d_min, d_max, ep), wk,
                                                                     methods=list(kern), kernels=kern, cc_nb_eval=nb)
            for m in ("rank1_distrib", "rank2_distrib"):
                meta["lp_vs_closed"][f"eval_CC_list/{name}/{tag}/{m}"] = meta["lp_vs_closed_kernel"]
        print("e2 complexes", name, round(time.time() - t0, 1), "s", record.get("programs", 0), "programs")
    meta["programs"] = record.get("programs", 0)
    meta["seconds"] = round(time.time() - t0, 1)
    meta["note"] = ("gaussian_emd ran on a stand-in pyemd (scipy.optimize.linprog), the complexes on a stand-in CombinatorialComplex; lp_vs_closed = "
                    "largest |program - closed form| per score; f32_vs_f64 = largest difference between the reference's float32 eigenvalues (and "
                    "scores) and the same from float64 numpy.linalg.eigvalsh; edge_margin = smallest distance of a reference eigenvalue to an "
                    "interior bin edge")
    out["meta"] = np.array(json.dumps(plain(meta)))
    path = os.path.join(GOLD, "e2_spectrum.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_FIXTURE, os.path.getsize(path)
    print("wrote e2_spectrum", os.path.getsize(path), "bytes;", meta["programs"], "programs,", meta["seconds"], "s")


def d1_qm9_cc_n1000(B=256, seed=42, raw=None):
    """d1_qm9_CC_n1000.npz: ONE reference run of the shipped qm9_CC sampling set-up -- checkpoints/QM9/ccsd_qm9_CC.pth, the sampler block of
    config/sample_qm9_CC.yaml, all 1000 scales, B complexes, flags drawn as the harness draws them without the dataset blobs
    (ccsd_amd.sampler.init_flags on the shipped QM9 node-count histogram after np.random.seed(seed)), every draw from torch's CPU
    generator after torch.manual_seed(seed) -- reduced to the flags and ref_descriptors of the final tensors.  The host time the run took
    is recorded in the metadata.  `raw`: a path that also receives the final tensors (not a fixture; for inspection)."""
    import time

    import yaml

    from ccsd_amd import sampler as S
    from ccsd_amd.loader import AttrDict

    with open(os.path.join(refshim.REFERENCE_ROOT, "config", "sample_qm9_CC.yaml")) as f:
        y = yaml.safe_load(f)
    smp = dict(y["sampler"])
    ck = refshim.load_reference_ckpt(CHECKPOINTS["ccsd_qm9_CC"][0])
    data = ck["model_config"]["data"]
    with open(S._COUNTS) as f:
        hist = json.load(f)["QM9"]["test_histogram"]
    np.random.seed(seed)
    flags = S.init_flags(hist, AttrDict({"data": {"max_node_num": int(data["max_node_num"])}}), B, is_cc=True)
    kept = {}
    t0 = time.perf_counter()
    _g5_pc_runs("d1", ck, True, B, None, smp, {"n1000": (None, None)}, seed, flags=flags, keep=kept)
    seconds = time.perf_counter() - t0
    t = kept["n1000"]
    if raw:
        np.savez_compressed(raw, flags=flags.numpy(), **t)
    out = ref_descriptors(t["x"], t["adj"], t["rank2"], int(data["d_min"]), int(data["d_max"]), True)
    out["flags"] = flags.numpy().astype(np.float32)
    out["meta"] = np.array(json.dumps({
        "checkpoint": CHECKPOINTS["ccsd_qm9_CC"][0], "sampler": smp, "num_scales": int(ck["model_config"]["sde"]["adj"]["num_scales"]),
        "B": B, "numpy_seed": seed, "torch_seed": seed, "eps": 1e-4, "denoise": True,
        "flags": "ccsd_amd.sampler.init_flags(QM9 test_histogram of ccsd_amd/data/node_counts.json) after np.random.seed(numpy_seed)",
        "reference_run_seconds": round(seconds, 1), "host_threads": torch.get_num_threads(),
        "d_min": int(data["d_min"]), "d_max": int(data["d_max"])}))
    path = os.path.join(GOLD, "d1_qm9_CC_n1000.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_FIXTURE
    print("wrote d1_qm9_CC_n1000", os.path.getsize(path), "bytes;", round(seconds, 1), "s of reference time")


def kat_small_models():
    """Small randomly initialised networks built by the reference's own constructors (the same
    hyper-parameter family as its known-answer tests, tests/models/test_ScoreNetwork_A_CC.py:88-115,
    test_ScoreNetwork_F.py:45-66) including num_linears_h = 2 / num_layers_mlp = 2 (general, non-affine path)."""
    from ccsd.src.models.ScoreNetwork_A_CC import ScoreNetworkA_CC
    from ccsd.src.models.ScoreNetwork_F import ScoreNetworkF
    from ccsd.src.models.ScoreNetwork_X import ScoreNetworkX
    from ccsd.src.models.ScoreNetwork_A import ScoreNetworkA

    out = {}
    N, Fd, d_min, d_max = 5, 10, 3, 4
    pa = dict(max_feat_num=Fd, max_node_num=N, d_min=d_min, d_max=d_max, nhid=4, num_layers=2, num_linears=2,
              c_init=2, c_hid=2, c_final=2, adim=2, num_heads=2, conv="GCN", conv_hodge="HCN", use_bn=False,
              is_cc=True, nhid_h=2, num_layers_h=2, num_linears_h=2, c_hid_h=2, c_final_h=2, adim_h=2, num_heads_h=2)
    pf = dict(num_layers_mlp=2, num_layers=2, num_linears=2, nhid=2, c_hid=3, c_final=2, cnum=2, max_node_num=N,
              d_min=d_min, d_max=d_max, use_hodge_mask=True, use_bn=False, is_cc=True)
    px = dict(max_feat_num=Fd, depth=2, nhid=4, use_bn=False, is_cc=True)
    pg = dict(max_feat_num=Fd, max_node_num=N, nhid=4, num_layers=3, num_linears=2, c_init=2, c_hid=3, c_final=2,
              adim=4, num_heads=2, conv="GCN", use_bn=False, is_cc=False)
    torch.manual_seed(42)
    nets = {"adj": (ScoreNetworkA_CC(**pa), dict(pa, model_type="ScoreNetworkA_CC")),
            "rank2": (ScoreNetworkF(**pf), dict(pf, model_type="ScoreNetworkF")),
            "x": (ScoreNetworkX(**px), dict(px, model_type="ScoreNetworkX")),
            "gadj": (ScoreNetworkA(**pg), dict(pg, model_type="ScoreNetworkA"))}
    # biases are zero-initialised by the reference; perturb them so bias handling is exercised
    for m, _ in nets.values():
        for k, p in m.named_parameters():
            if k.endswith("bias"):
                p.data.normal_(0, 0.2)
        m.eval()
    B = 3
    flags = make_flags(B, N, [5, 4, 3])
    x, adj, rank2 = masked_state(99, B, N, Fd, True, d_min, d_max, flags)
    out["flags"], out["x"], out["adj"], out["rank2"] = flags.numpy(), x.numpy(), adj.numpy(), rank2.numpy()
    meta = {}
    with torch.no_grad():
        for tag, (m, p) in nets.items():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            meta[tag] = p
            args = (x, adj, flags) if tag == "gadj" else (x, adj, rank2, flags)
            out[f"{tag}/out"] = m(*args).numpy()
            # also with unmasked inputs and flags=None semantics (flags all ones)
    out["meta"] = json.dumps(meta)
    np.savez_compressed(os.path.join(GOLD, "kat_small_models.npz"), **out)


def kat_gmh_models():
    """Variants without a shipped checkpoint, randomly initialised by the reference's constructors (biases perturbed):
    ScoreNetworkX_GMH (ScoreNetwork_X.py:156-341) small (hyper-parameters of tests/models/test_ScoreNetwork_X.py) and at the
    width of GDSS's ZINC250k X-network; conv = "MLP" attention (attention.py:168-178) in ScoreNetworkX_GMH and ScoreNetworkA."""
    from ccsd.src.models.ScoreNetwork_X import ScoreNetworkX_GMH
    from ccsd.src.models.ScoreNetwork_A import ScoreNetworkA

    out, meta = {}, {}
    cases = {
        "small": (ScoreNetworkX_GMH, dict(max_feat_num=10, depth=2, nhid=4, num_linears=2, c_init=2, c_hid=3, c_final=2, adim=4,
                                          num_heads=2, conv="GCN", use_bn=False, is_cc=False), 5, [5, 4, 3]),
        "wide": (ScoreNetworkX_GMH, dict(max_feat_num=9, depth=3, nhid=16, num_linears=3, c_init=2, c_hid=8, c_final=4, adim=16,
                                         num_heads=4, conv="GCN", use_bn=False, is_cc=True), 12, [12, 9, 7, 2]),
        "mlpconv_x": (ScoreNetworkX_GMH, dict(max_feat_num=6, depth=2, nhid=8, num_linears=2, c_init=2, c_hid=4, c_final=3, adim=8,
                                              num_heads=4, conv="MLP", use_bn=False, is_cc=False), 9, [9, 7, 4]),
        "mlpconv_a": (ScoreNetworkA, dict(max_feat_num=6, max_node_num=9, nhid=8, num_layers=3, num_linears=2, c_init=2, c_hid=4,
                                          c_final=3, adim=8, num_heads=4, conv="MLP", use_bn=False, is_cc=False), 9, [9, 7, 4]),
    }
    torch.manual_seed(4242)
    for tag, (cls, p, N, counts) in cases.items():
        m = cls(**p)
        for k, prm in m.named_parameters():
            if k.endswith("bias"):
                prm.data.normal_(0, 0.2)
        m.eval()
        B = len(counts)
        flags = make_flags(B, N, counts)
        x, adj, _ = masked_state(77, B, N, p["max_feat_num"], False, None, None, flags)
        out[f"{tag}/flags"], out[f"{tag}/x"], out[f"{tag}/adj"] = flags.numpy(), x.numpy(), adj.numpy()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            out[f"{tag}/out"] = (m(x, adj, None, flags) if p["is_cc"] else m(x, adj, flags)).numpy()
        meta[tag] = dict(p, model_type=cls.__name__)
    out["meta"] = json.dumps(meta)
    np.savez_compressed(os.path.join(GOLD, "kat_gmh_models.npz"), **out)
    print("kat_gmh", {k: v.shape for k, v in out.items() if k.endswith("/out")})


def kat_zinc5b():
    """SURVEY 8(d) substitute 5b for the infeasible zinc250k_CC config (d_max = 24 -> K = 2.6e11): the same N = 38 and the
    hyper-parameters of config/zinc250k_CC.yaml:38-64 (loader.load_model_params, loader.py:461-566) with d_min = d_max = 3
    (E = 703, K = 8436), networks built and randomly initialised by the reference's constructors (biases perturbed), B = 2.
    rank-2 sized outputs (47 MB) are stored as a strided sample + checksums."""
    from ccsd.src.models.ScoreNetwork_A_CC import ScoreNetworkA_CC
    from ccsd.src.models.ScoreNetwork_F import ScoreNetworkF
    from ccsd.src.models.ScoreNetwork_X import ScoreNetworkX

    N, Fd, d_min, d_max = 38, 9, 3, 3
    px = dict(max_feat_num=Fd, depth=2, nhid=2, use_bn=False, is_cc=True)
    pa = dict(max_feat_num=Fd, max_node_num=N, d_min=d_min, d_max=d_max, nhid=2, nhid_h=2, num_layers=2, num_layers_h=1,
              num_linears=2, num_linears_h=1, c_init=2, c_hid=2, c_hid_h=2, c_final=2, c_final_h=2, adim=4, adim_h=2,
              num_heads=2, num_heads_h=2, conv="GCN", conv_hodge="HCN", use_bn=False, is_cc=True)
    pf = dict(num_layers_mlp=1, num_layers=1, num_linears=1, nhid=2, c_hid=2, c_final=2, cnum=1, max_node_num=N, d_min=d_min,
              d_max=d_max, use_hodge_mask=True, use_bn=False, is_cc=True)
    ref_cc.default_mask.cache_clear()
    torch.manual_seed(538)
    nets = {"x": (ScoreNetworkX(**px), dict(px, model_type="ScoreNetworkX")),
            "adj": (ScoreNetworkA_CC(**pa), dict(pa, model_type="ScoreNetworkA_CC")),
            "rank2": (ScoreNetworkF(**pf), dict(pf, model_type="ScoreNetworkF"))}
    for m, _ in nets.values():
        for k, p in m.named_parameters():
            if k.endswith("bias"):
                p.data.normal_(0, 0.2)
        m.eval()
    B, seed = 2, 77
    flags = make_flags(B, N, [38, 23])
    out = {"flags": flags.numpy(), "seed": seed, "rng_probe": rng_probe(seed)}
    meta = {}
    samp = lambda t: t[:, ::37, ::53].contiguous().numpy()
    x, adj, rank2 = masked_state(seed, B, N, Fd, True, d_min, d_max, flags, 1.0)
    with torch.no_grad():
        for tag, (m, p) in nets.items():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            meta[tag] = p
            o = m(x, adj, rank2, flags)
            if tag == "rank2":
                out["rank2/out_sample"] = samp(o)
                out["rank2/out_checksum"] = np.array([o.double().sum().item(), o.abs().double().sum().item(), o.abs().max().item()])
            else:
                out[f"{tag}/out"] = o.numpy()
    # short sampler run with the sampler block of config/zinc250k_CC.yaml:85-90 and its SDEs (:20-35), 3 scales
    sde_cfg = {"x": dict(type="VP", beta_min=0.1, beta_max=1.0), "adj": dict(type="VE", beta_min=0.2, beta_max=1.0),
               "rank2": dict(type="VE", beta_min=0.1, beta_max=1.0)}
    sm = dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.9, n_steps=1)
    sdes = [ref_loader.load_sde(refshim.EasyDict(dict(sde_cfg[p], num_scales=3))) for p in ("x", "adj", "rank2")]
    E, K = ref_cc.get_rank2_dim(N, d_min, d_max)
    fn = ref_solver.get_pc_sampler(sde_x=sdes[0], sde_adj=sdes[1], shape_x=(B, N, Fd), shape_adj=(B, N, N), predictor=sm["predictor"],
                                   corrector=sm["corrector"], snr=sm["snr"], scale_eps=sm["scale_eps"], n_steps=1,
                                   probability_flow=False, continuous=True, denoise=True, eps=1e-4, device="cpu", is_cc=True,
                                   sde_rank2=sdes[2], shape_rank2=(B, E, K), d_min=d_min, d_max=d_max)
    orig = ref_solver.trange
    ref_solver.trange = lambda a, b, **k: range(a, b)
    try:
        torch.manual_seed(seed)
        res = fn(nets["x"][0], nets["adj"][0], nets["rank2"][0], flags)
    finally:
        ref_solver.trange = orig
    out["k3/x"], out["k3/adj"] = res[0].numpy(), res[1].numpy()
    out["k3/rank2_sample"] = samp(res[2])
    out["k3/rank2_checksum"] = np.array([res[2].double().sum().item(), res[2].abs().double().sum().item(), res[2].abs().max().item()])
    out["k3/quantize_mol_adj"] = ref_gu.quantize_mol(res[1].clone())
    thr = torch.tensor([0.5, 1.5, 2.5])
    out["k3/min_thr_dist"] = np.array((res[1][..., None] - thr).abs().min().item())
    out["meta"] = json.dumps(dict(params=meta, sde=sde_cfg, sampler=sm, dims=[N, Fd, d_min, d_max, E, K]))
    np.savez_compressed(os.path.join(GOLD, "kat_zinc250k_CC_5b.npz"), **out)
    # the same weights as a neutral-format checkpoint (bench.py --workload zinc250k_CC_5b): no shipped checkpoint exists for it
    arrays = {f"{tag}/{k}": v.detach().cpu().numpy().astype(np.float32) for tag, (m, _) in nets.items() for k, v in m.state_dict().items()}
    cfg = {"is_cc": True,
           "data": {"data": "ZINC250k", "max_node_num": N, "max_feat_num": Fd, "d_min": d_min, "d_max": d_max, "batch_size": 1024},
           "sde": {p: dict(v, num_scales=1000) for p, v in sde_cfg.items()}, "sampler": sm}
    ck = {"name": "zinc250k_CC_5b", "source": "reference constructors with config/zinc250k_CC.yaml hyper-parameters, d_min = d_max = 3, "
          "random initialisation (tools/make_golden.py::kat_zinc5b)", "is_cc": True, "config": cfg}
    for tag, (_, prm) in nets.items():
        ck[f"params_{tag}"] = prm
    np.savez_compressed(os.path.join(CKPT, "zinc250k_CC_5b.npz"), **arrays)
    with open(os.path.join(CKPT, "zinc250k_CC_5b.json"), "w") as f:
        json.dump(ck, f, indent=1, sort_keys=True)
    print("kat_zinc5b: E, K =", E, K, "min thr dist", float(out["k3/min_thr_dist"]), {k: v.shape for k, v in out.items() if k.endswith("out") or k.endswith("sample")})


def kat_cnum():
    """ScoreNetworkF with more than two Hodge powers in its input (cnum = 3, 4: pow_tensor_cc, cc_utils.py:961-979), built by the
    reference's constructor: the affine case (single Linears) and the general per-element MLP case, at N = 5 (E = 10, K = 15) and
    N = 12 (E = 66, K = 715)."""
    from ccsd.src.models.ScoreNetwork_F import ScoreNetworkF

    out, meta = {}, {}
    cases = {
        "affine3": (5, 3, 4, dict(num_layers_mlp=1, num_layers=2, num_linears=1, nhid=3, c_hid=3, c_final=2, cnum=3), [5, 4, 3]),
        "general3": (5, 3, 4, dict(num_layers_mlp=2, num_layers=2, num_linears=2, nhid=4, c_hid=3, c_final=2, cnum=3), [5, 4, 3]),
        "affine4_n12": (12, 3, 4, dict(num_layers_mlp=1, num_layers=1, num_linears=1, nhid=2, c_hid=2, c_final=2, cnum=4), [12, 9]),
        "general4_nomask": (5, 3, 4, dict(num_layers_mlp=1, num_layers=2, num_linears=2, nhid=4, c_hid=2, c_final=2, cnum=4, use_hodge_mask=False), [5, 2]),
    }
    torch.manual_seed(909)
    for tag, (N, dmin, dmax, hp, counts) in cases.items():
        prm = dict(hp, max_node_num=N, d_min=dmin, d_max=dmax, use_bn=False, is_cc=True)
        prm.setdefault("use_hodge_mask", True)
        ref_cc.default_mask.cache_clear()
        m = ScoreNetworkF(**prm)
        for k, p_ in m.named_parameters():
            if k.endswith("bias"):
                p_.data.normal_(0, 0.2)
        m.eval()
        B = len(counts)
        flags = make_flags(B, N, counts)
        x, adj, rank2 = masked_state(31, B, N, 2, True, dmin, dmax, flags, 0.5)
        out[f"{tag}/flags"], out[f"{tag}/rank2"] = flags.numpy(), rank2.numpy()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            out[f"{tag}/out"] = m(x, adj, rank2, flags).numpy()
        meta[tag] = dict(prm, model_type="ScoreNetworkF")
    out["meta"] = json.dumps(meta)
    np.savez_compressed(os.path.join(GOLD, "kat_cnum.npz"), **out)
    print("kat_cnum", {k: (v.shape, float(np.abs(v).max())) for k, v in out.items() if k.endswith("/out")})


def kat_arch_sweep():
    """Six architectures of the architecture sweep (tests/arch_sweep_cases.py: KAT) built by the reference's constructors, biases
    perturbed, B = 4 with node counts [N, N // 2 + 1, 1 or 2, 0]: ScoreNetworkA with an un-chained edge MLP and five adjacency powers,
    one head, three heads on an attention dimension of 12, four Linears per edge MLP, a single AttentionLayer; ScoreNetworkF 12 wide
    with four Linears per HodgeNetworkLayer (N = 6, d = 3..4).  Weights, inputs, flags and outputs only."""
    from ccsd.src.models.ScoreNetwork_A import ScoreNetworkA
    from ccsd.src.models.ScoreNetwork_F import ScoreNetworkF

    base = dict(nhid=16, num_layers=3, num_linears=2, c_init=2, c_hid=8, c_final=4, adim=16, num_heads=4, conv="GCN")
    graph = {"chid12_cinit5": (dict(c_hid=12, c_init=5), 0.5), "heads1": (dict(num_heads=1), 1.0),
             "heads3": (dict(num_heads=3, adim=12, nhid=12), 1.0), "lin4": (dict(num_linears=4), 1.0),
             "layers1": (dict(num_layers=1, c_hid=4, c_final=4), 1.0)}
    out, meta = {}, {}
    torch.manual_seed(1212)
    for tag, (over, scale) in graph.items():
        N, Fd = 9, 4
        prm = dict(base, **over, max_feat_num=Fd, max_node_num=N, use_bn=False, is_cc=False)
        m = ScoreNetworkA(**prm)
        for k, p_ in m.named_parameters():
            if k.endswith("bias"):
                p_.data.normal_(0, 0.2)
        m.eval()
        flags = make_flags(4, N, [N, N // 2 + 1, 1, 0])
        x, adj, _ = masked_state(53, 4, N, Fd, False, None, None, flags, scale)
        out[f"{tag}/flags"], out[f"{tag}/x"], out[f"{tag}/adj"] = flags.numpy(), x.numpy(), adj.numpy()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            out[f"{tag}/out"] = m(x, adj, flags).numpy()
        meta[tag] = dict(prm, model_type="ScoreNetworkA")
    N, dmin, dmax = 6, 3, 4
    prm = dict(num_layers_mlp=1, num_layers=2, num_linears=4, nhid=12, c_hid=12, c_final=12, cnum=2, max_node_num=N, d_min=dmin,
               d_max=dmax, use_hodge_mask=True, use_bn=False, is_cc=True)
    ref_cc.default_mask.cache_clear()
    m = ScoreNetworkF(**prm)
    for k, p_ in m.named_parameters():
        if k.endswith("bias"):
            p_.data.normal_(0, 0.2)
    m.eval()
    flags = make_flags(4, N, [N, N // 2 + 1, 2, 0])
    x, adj, rank2 = masked_state(53, 4, N, 2, True, dmin, dmax, flags, 0.5)
    tag = "f_w12_lin4"
    out[f"{tag}/flags"], out[f"{tag}/rank2"] = flags.numpy(), rank2.numpy()
    with torch.no_grad():
        for k, v in m.state_dict().items():
            out[f"{tag}/w/{k}"] = v.numpy()
        out[f"{tag}/out"] = m(x, adj, rank2, flags).numpy()
    meta[tag] = dict(prm, model_type="ScoreNetworkF")
    out["meta"] = json.dumps(meta)
    path = os.path.join(GOLD, "kat_arch_sweep.npz")
    np.savez_compressed(path, **out)
    print("kat_arch_sweep", os.path.getsize(path), "bytes", {k: (v.shape, float(np.abs(v).max())) for k, v in out.items() if k.endswith("/out")})


def kat_hodge_layers():
    """ScoreNetworkA_CC with three and four HodgeAdjAttentionLayers (num_layers_h = 3, 4; num_linears_h = 1), built by the
    reference's constructor: no shipped checkpoint has more than two.  N = 5 (E = 10, K = 15; the geometry of kat_small_models, whose
    X / F networks complete a sampler in the tests), N = 6 (E = 15) and the qm9_CC
    geometry N = 9, d 3..9 (E = 36, K = 466)."""
    from ccsd.src.models.ScoreNetwork_A_CC import ScoreNetworkA_CC

    out, meta = {}, {}
    base = dict(nhid=4, num_layers=2, num_linears=2, c_init=2, c_hid=2, c_final=2, adim=2, num_heads=2, conv="GCN",
                conv_hodge="HCN", use_bn=False, is_cc=True, num_linears_h=1)
    cases = {
        "L3_n5": (5, 10, 3, 4, dict(nhid_h=2, num_layers_h=3, c_hid_h=2, c_final_h=2, adim_h=2, num_heads_h=2), [5, 4, 3]),
        "L4_n6": (6, 2, 3, 4, dict(nhid_h=4, num_layers_h=4, c_hid_h=3, c_final_h=2, adim_h=4, num_heads_h=2), [6, 4]),
        "L3_n9": (9, 4, 3, 9, dict(nhid_h=4, num_layers_h=3, c_hid_h=4, c_final_h=2, adim_h=4, num_heads_h=2), [9, 6]),
    }
    torch.manual_seed(1717)
    for tag, (N, Fd, dmin, dmax, hp, counts) in cases.items():
        prm = dict(base, **hp, max_feat_num=Fd, max_node_num=N, d_min=dmin, d_max=dmax)
        m = ScoreNetworkA_CC(**prm)
        for k, p_ in m.named_parameters():
            if k.endswith("bias"):
                p_.data.normal_(0, 0.2)
        m.eval()
        B = len(counts)
        flags = make_flags(B, N, counts)
        x, adj, rank2 = masked_state(57, B, N, Fd, True, dmin, dmax, flags, 0.5)
        for k, v in (("flags", flags), ("x", x), ("adj", adj), ("rank2", rank2)):
            out[f"{tag}/{k}"] = v.numpy()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            out[f"{tag}/out"] = m(x, adj, rank2, flags).numpy()
        meta[tag] = dict(prm, model_type="ScoreNetworkA_CC")
    out["meta"] = json.dumps(meta)
    np.savez_compressed(os.path.join(GOLD, "kat_hodge_layers.npz"), **out)
    print("kat_hodge_layers", {k: (v.shape, float(np.abs(v).max())) for k, v in out.items() if k.endswith("/out")})


def kat_hodge_general():
    """ScoreNetworkA_CC with three and four HodgeAdjAttentionLayers whose mlp_value / mlp_attention are true MLPs (num_linears_h = 2, 3:
    ELU between the Linears, hodge_attention.py:245-252), built by the reference's constructor: the rank-2 features of layer l >= 2,
    R_l = mask_rank2(mlp_value(cat_c H_c R_(l-1))) (hodge_attention.py:98, 322-323), are no longer an affine image of rank2 and must be
    materialised.  N = 5 (E = 10, K = 15), N = 6 (E = 15, K = 35), the qm9_CC geometry N = 9, d 3..9 (E = 36, K = 466) and N = 12, d 3..4
    (E = 66, K = 715)."""
    from ccsd.src.models.ScoreNetwork_A_CC import ScoreNetworkA_CC

    out, meta = {}, {}
    base = dict(nhid=4, num_layers=2, num_linears=2, c_init=2, c_hid=2, c_final=2, adim=2, num_heads=2, conv="GCN",
                conv_hodge="HCN", use_bn=False, is_cc=True)
    cases = {
        "G3_n5": (5, 10, 3, 4, dict(nhid_h=2, num_layers_h=3, num_linears_h=2, c_hid_h=2, c_final_h=2, adim_h=2, num_heads_h=2), [5, 4, 3]),
        "G4_n6": (6, 2, 3, 4, dict(nhid_h=4, num_layers_h=4, num_linears_h=2, c_hid_h=3, c_final_h=2, adim_h=4, num_heads_h=2), [6, 4]),
        "G3_n9": (9, 4, 3, 9, dict(nhid_h=4, num_layers_h=3, num_linears_h=3, c_hid_h=4, c_final_h=2, adim_h=4, num_heads_h=2), [9, 6]),
        # E = 66 > 64 (the ENZYMES_small_CC geometry): no fused rank-2 kernel, so the single-Linear stack takes the general route too
        "G3_n12": (12, 3, 3, 4, dict(nhid_h=4, num_layers_h=3, num_linears_h=2, c_hid_h=2, c_final_h=2, adim_h=4, num_heads_h=2), [12, 8]),
        "A3_n12": (12, 3, 3, 4, dict(nhid_h=4, num_layers_h=3, num_linears_h=1, c_hid_h=2, c_final_h=2, adim_h=4, num_heads_h=2), [12, 7]),
        # more than four layers (single Linears, and true MLPs)
        "A5_n5": (5, 10, 3, 4, dict(nhid_h=2, num_layers_h=5, num_linears_h=1, c_hid_h=2, c_final_h=2, adim_h=2, num_heads_h=2), [5, 3]),
        "G6_n6": (6, 2, 3, 4, dict(nhid_h=4, num_layers_h=6, num_linears_h=2, c_hid_h=2, c_final_h=3, adim_h=4, num_heads_h=2), [6, 5]),
    }
    torch.manual_seed(2718)
    for tag, (N, Fd, dmin, dmax, hp, counts) in cases.items():
        prm = dict(base, **hp, max_feat_num=Fd, max_node_num=N, d_min=dmin, d_max=dmax)
        m = ScoreNetworkA_CC(**prm)
        for k, p_ in m.named_parameters():
            if k.endswith("bias"):
                p_.data.normal_(0, 0.2)
        m.eval()
        B = len(counts)
        flags = make_flags(B, N, counts)
        x, adj, rank2 = masked_state(58, B, N, Fd, True, dmin, dmax, flags, 0.5)
        for k, v in (("flags", flags), ("x", x), ("adj", adj), ("rank2", rank2)):
            out[f"{tag}/{k}"] = v.numpy()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            out[f"{tag}/out"] = m(x, adj, rank2, flags).numpy()
        meta[tag] = dict(prm, model_type="ScoreNetworkA_CC")
    out["meta"] = json.dumps(meta)
    np.savez_compressed(os.path.join(GOLD, "kat_hodge_general.npz"), **out)
    print("kat_hodge_general", {k: (v.shape, float(np.abs(v).max())) for k, v in out.items() if k.endswith("/out")})


def kat_hodge_wide():
    """ScoreNetworkA_CC whose hodge branch is up to 8 channels wide, so that the true MLPs mlp_value / mlp_attention (num_linears_h >= 2)
    have hidden Linears 9 to 16 wide (hid = 2 max(cin, cout), hodge_attention.py:245-252), built by the reference's constructor; the graph
    branch is kat_hodge_general's.  Tags: one layer with the full 16 (W1_n5), two layers with a ragged 10 (W2_n6), the qm9_CC geometry with
    three Linears (W2_n9), three layers at E = 66 with hidden widths 12 and 16 (W3_n12: the general hodge stack), and the single-Linear
    counterpart of W2_n9 (S2_n9), whose widest Linear is 8."""
    from ccsd.src.models.ScoreNetwork_A_CC import ScoreNetworkA_CC

    out, meta = {}, {}
    base = dict(nhid=4, num_layers=2, num_linears=2, c_init=2, c_hid=2, c_final=2, adim=2, num_heads=2, conv="GCN",
                conv_hodge="HCN", use_bn=False, is_cc=True, nhid_h=4, adim_h=4, num_heads_h=2)
    cases = {
        "W1_n5": (5, 10, 3, 4, dict(num_layers_h=1, num_linears_h=2, c_hid_h=8, c_final_h=8), [5, 4, 3]),
        "W2_n6": (6, 2, 3, 4, dict(num_layers_h=2, num_linears_h=2, c_hid_h=5, c_final_h=3), [6, 4]),
        "W2_n9": (9, 4, 3, 9, dict(num_layers_h=2, num_linears_h=3, c_hid_h=8, c_final_h=4), [9, 6, 2]),
        "W3_n12": (12, 3, 3, 4, dict(c_init=3, num_layers_h=3, num_linears_h=2, c_hid_h=6, c_final_h=8), [12, 7]),
        "S2_n9": (9, 4, 3, 9, dict(num_layers_h=2, num_linears_h=1, c_hid_h=8, c_final_h=4), [9, 5]),
    }
    torch.manual_seed(3141)
    for tag, (N, Fd, dmin, dmax, hp, counts) in cases.items():
        prm = dict(base, **hp, max_feat_num=Fd, max_node_num=N, d_min=dmin, d_max=dmax)
        m = ScoreNetworkA_CC(**prm)
        for k, p_ in m.named_parameters():
            if k.endswith("bias"):
                p_.data.normal_(0, 0.2)
        m.eval()
        B = len(counts)
        flags = make_flags(B, N, counts)
        x, adj, rank2 = masked_state(59, B, N, Fd, True, dmin, dmax, flags, 0.5)
        for k, v in (("flags", flags), ("x", x), ("adj", adj), ("rank2", rank2)):
            out[f"{tag}/{k}"] = v.numpy()
        with torch.no_grad():
            for k, v in m.state_dict().items():
                out[f"{tag}/w/{k}"] = v.numpy()
            out[f"{tag}/out"] = m(x, adj, rank2, flags).numpy()
        meta[tag] = dict(prm, model_type="ScoreNetworkA_CC")
    # (the N = 12 tag's K = 715 rows of Wcat and rank2 would carry the file past 1 MiB: it goes into a second one, named in "files")
    second = {k: out.pop(k) for k in list(out) if k.startswith("W3_n12/")}
    out["meta"] = json.dumps(meta)
    out["files"] = json.dumps(["kat_hodge_wide.npz", "kat_hodge_wide.1.npz"])
    np.savez_compressed(os.path.join(GOLD, "kat_hodge_wide.npz"), **out)
    np.savez_compressed(os.path.join(GOLD, "kat_hodge_wide.1.npz"), **second)
    out.update(second)
    print("kat_hodge_wide", {k: (v.shape, float(np.abs(v).max())) for k, v in out.items() if k.endswith("/out")})


def reference_variant_status():
    """What the reference itself does with the two config switches no shipped config sets: use_bn=True (layers.py:219-224,
    262-275: BatchNorm1d(hidden) applied to (B, N, hidden) / (B, N, N, hidden) activations) and conv_hodge="MLP"
    (hodge_attention.py:100-102, 168-179: an MLP with input width K applied to the E x E hodge adjacency).  Exception types
    and messages of a forward pass are recorded; the product raises the same types for the same configurations."""
    from ccsd.src.models.ScoreNetwork_A import ScoreNetworkA
    from ccsd.src.models.ScoreNetwork_A_CC import ScoreNetworkA_CC
    from ccsd.src.models.ScoreNetwork_F import ScoreNetworkF
    from ccsd.src.models.ScoreNetwork_X import ScoreNetworkX, ScoreNetworkX_GMH

    torch.manual_seed(0)
    out = {}

    def attempt(tag, params, build, args):
        try:
            o = build().eval()(*args)
            out[tag] = {"params": params, "result": "ok", "shape": list(o.shape)}
        except Exception as e:      # noqa: BLE001 -- the point is to record whatever the reference raises
            out[tag] = {"params": params, "result": "error", "type": type(e).__name__, "message": str(e)}

    B = 2
    def inputs(N, Fd, E=None, K=None):
        x = torch.randn(B, N, Fd); a = torch.randn(B, N, N); a = a + a.transpose(1, 2)
        return x, a, (torch.randn(B, E, K) if E else None), torch.ones(B, N)

    px = dict(max_feat_num=3, depth=2, nhid=4, use_bn=True, is_cc=False)
    x, a, _, fl = inputs(5, 3)
    attempt("bn_x_N5_hidden22", dict(px, model_type="ScoreNetworkX"), lambda: ScoreNetworkX(**px), (x, a, fl))
    px8 = dict(max_feat_num=2, depth=1, nhid=2, use_bn=True, is_cc=False)        # N == 2 * fdim: the one shape that type-checks
    x, a, _, fl = inputs(8, 2)
    attempt("bn_x_N8_hidden8", dict(px8, model_type="ScoreNetworkX"), lambda: ScoreNetworkX(**px8), (x, a, fl))
    pa = dict(max_feat_num=2, max_node_num=8, nhid=4, num_layers=2, num_linears=2, c_init=2, c_hid=2, c_final=2, adim=4, num_heads=2,
              conv="GCN", use_bn=True, is_cc=False)
    attempt("bn_a", dict(pa, model_type="ScoreNetworkA"), lambda: ScoreNetworkA(**pa), (x, a, fl))
    pg = dict(max_feat_num=2, depth=2, nhid=4, num_linears=2, c_init=2, c_hid=2, c_final=2, adim=4, num_heads=2, conv="GCN", use_bn=True,
              is_cc=False)
    attempt("bn_x_gmh", dict(pg, model_type="ScoreNetworkX_GMH"), lambda: ScoreNetworkX_GMH(**pg), (x, a, fl))
    pf = dict(num_layers_mlp=2, num_layers=1, num_linears=2, nhid=2, c_hid=2, c_final=2, cnum=2, max_node_num=5, d_min=3, d_max=4,
              use_hodge_mask=True, use_bn=True, is_cc=True)
    ref_cc.default_mask.cache_clear()
    x, a, r, fl = inputs(5, 3, 10, 15)
    attempt("bn_f", dict(pf, model_type="ScoreNetworkF"), lambda: ScoreNetworkF(**pf), (x, a, r, fl))
    for (N, dmin, dmax) in ((5, 3, 4), (5, 3, 3), (6, 3, 3)):
        E, K = ref_cc.get_rank2_dim(N, dmin, dmax)
        pc_ = dict(max_feat_num=3, max_node_num=N, d_min=dmin, d_max=dmax, nhid=4, nhid_h=2, num_layers=2, num_layers_h=2, num_linears=2,
                   num_linears_h=1, c_init=2, c_hid=2, c_hid_h=2, c_final=2, c_final_h=2, adim=4, adim_h=2, num_heads=2, num_heads_h=2,
                   conv="GCN", conv_hodge="MLP", use_bn=False, is_cc=True)
        x, a, r, fl = inputs(N, 3, E, K)
        attempt(f"conv_hodge_mlp_N{N}_E{E}_K{K}", dict(pc_, model_type="ScoreNetworkA_CC"), lambda: ScoreNetworkA_CC(**pc_), (x, a, r, fl))
    with open(os.path.join(GOLD, "reference_variant_status.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for k, v in out.items():
        print("variant", k, v["result"], v.get("type", ""), v.get("message", v.get("shape")))


def reference_module_objects():
    """What the reference's own load_model_from_ckpt (loader.py:619-657) returns for the checkpoints the seam test feeds it
    (tests/test_seam_modules.py): per model the class name, the plain attributes its constructor stores, and the state_dict
    keys with the kind of tensor behind each.  The test rebuilds torch.nn.Modules of that description around the checkpoint's
    weights, so it runs without the reference."""
    out = {}
    for name in ("ccsd_qm9_CC", "ccsd_qm9_Base_CC"):
        with open(os.path.join(CKPT, name + ".json")) as f:
            meta = json.load(f)
        z = np.load(os.path.join(CKPT, name + ".npz"))
        out[name] = {}
        for p in ("x", "adj", "rank2"):
            sd = {k.split("/", 1)[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(p + "/")}
            ref_cc.default_mask.cache_clear()          # see build_models
            m = ref_loader.load_model_from_ckpt(refshim.EasyDict(meta[f"params_{p}"]), sd, "cpu")
            params, buffers = dict(m.named_parameters()), dict(m.named_buffers())
            out[name][p] = {
                "class": type(m).__name__,
                "attributes": {k: v for k, v in vars(m).items()
                               if not k.startswith("_") and k != "training" and isinstance(v, (bool, int, float, str))},
                "state_dict": [[k, "parameter" if k in params else "buffer" if k in buffers else "other"] for k in m.state_dict()],
            }
    with open(os.path.join(GOLD, "reference_module_objects.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("reference_module_objects", {n: {p: d["class"] for p, d in v.items()} for n, v in out.items()})


def kat_reference_held():
    """The known-answer vectors the REFERENCE'S OWN TESTS hold for the path (tests/models/test_ScoreNetwork_A_CC.py:119-162,
    test_ScoreNetwork_A_Base_CC.py:115-158, test_ScoreNetwork_F.py:69-106, test_hodge_attention.py:96-209, test_hodge_layers.py:143-375)
    as a fixture: tests/golden/kat_reference_held.npz.  Each reference test function is RUN here, unmodified, with the classes it
    constructs wrapped by a recorder: the fixture holds, per test, the constructor arguments, the weights the reference constructor
    drew (torch.manual_seed(42), in the test's own construction order), the tensors the module was called with, what it returned, and
    the EXPECTED values exactly as the reference test writes them (literal `expected_* = torch.tensor([...])` assignments, read from
    the test's syntax tree together with the slice of the output they are compared with and the atol).  The reference test's own
    assertions run too, so a wrong capture fails here.  A second, container-independent pin of the oracle (and, for the three whole
    networks, of the HIP path) next to the generated goldens."""
    import ast
    import importlib.util

    tests = [
        ("tests/models/test_ScoreNetwork_A_CC.py", "test_ScoreNetworkA_CC", ["ScoreNetworkA_CC"]),
        ("tests/models/test_ScoreNetwork_A_Base_CC.py", "test_ScoreNetworkA_Base_CC", ["ScoreNetworkA_Base_CC"]),
        ("tests/models/test_ScoreNetwork_F.py", "test_ScoreNetworkF", ["ScoreNetworkF"]),
        ("tests/models/test_hodge_attention.py", "test_HodgeAttention", ["HodgeAttention"]),
        ("tests/models/test_hodge_attention.py", "test_HodgeAdjAttentionLayer", ["HodgeAdjAttentionLayer"]),
        ("tests/models/test_hodge_layers.py", "test_DenseHCNConv", ["DenseHCNConv"]),
        ("tests/models/test_hodge_layers.py", "test_HodgeNetworkLayer", ["HodgeNetworkLayer"]),
        ("tests/models/test_hodge_layers.py", "test_BaselineBlock", ["BaselineBlock"]),
        ("tests/models/test_hodge_layers.py", "test_HodgeBaselineLayer", ["HodgeBaselineLayer"]),
    ]
    out, index = {}, {}
    for rel, tname, classes in tests:
        path = os.path.join(refshim.REFERENCE_ROOT, rel)
        spec = importlib.util.spec_from_file_location("ref_" + tname, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)                      # (seeds torch / numpy at import, like a pytest run of the file)
        records = []

        def wrap(cls):
            class Rec(cls):
                def __init__(self, *a, **k):
                    super().__init__(*a, **k)
                    self._rec = {"cls": cls.__name__, "args": plain(k if k else list(a)), "calls": []}
                    records.append(self)

                def forward(self, *a, **k):
                    res = super().forward(*a, **k)
                    keep = lambda t: t.detach().clone() if isinstance(t, torch.Tensor) else t       # (ints such as N, d_min pass through)
                    self._rec["calls"].append(([keep(t) for t in a], {n: keep(t) for n, t in k.items()},
                                               [r.detach().clone() for r in (res if isinstance(res, tuple) else (res,))]))
                    return res
            Rec.__name__ = cls.__name__
            return Rec

        for c in classes:
            setattr(mod, c, wrap(getattr(mod, c)))
        fn = getattr(mod, tname)
        # fixture values from the module's own fixture functions (pytest's wrappers hold the plain function), resolved recursively
        import inspect

        def fixture_value(name, cache={}):
            key = (tname, name)
            if key not in cache:
                raw = getattr(mod, name)._get_wrapped_function()
                cache[key] = raw(**{a: fixture_value(a) for a in inspect.signature(raw).parameters})
            return cache[key]

        fn(**{a: fixture_value(a) for a in inspect.signature(fn).parameters})       # the reference's assertions run here
        # literal expected values + the compared slice, from the test's syntax tree
        tree = ast.parse(open(path).read())
        fdef = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == tname)
        lits, checks = {}, []
        for n in ast.walk(fdef):
            if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id.startswith("expected"):
                lits[n.targets[0].id] = np.asarray(ast.literal_eval(n.value.args[0]), dtype=np.float32)
            if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "allclose":
                atol = next(ast.literal_eval(k.value) for k in n.keywords if k.arg == "atol")
                checks.append((ast.unparse(n.args[0]), n.args[1].id, float(atol)))
        rec = records[-1]._rec                               # the instance the value assertions are made on (the last one built)
        mdl = records[-1]
        key = tname[len("test_"):]
        for k2, v in mdl.state_dict().items():
            out[f"{key}/w/{k2}"] = v.detach().numpy().copy()
        args, kwargs, res = rec["calls"][-1]
        for i, t in enumerate(args):
            if isinstance(t, torch.Tensor):
                out[f"{key}/in/{i}"] = t.numpy()
        for nme, t in kwargs.items():
            if isinstance(t, torch.Tensor):
                out[f"{key}/kw/{nme}"] = t.numpy()
        for i, t in enumerate(res):
            out[f"{key}/out/{i}"] = t.numpy()
        for nme, v in lits.items():
            out[f"{key}/{nme}"] = v
        index[key] = {"cls": rec["cls"], "args": rec["args"], "n_in": len(args), "plain_in": {str(i): t for i, t in enumerate(args) if not isinstance(t, torch.Tensor)},
                      "plain_kw": {n: t for n, t in kwargs.items() if not isinstance(t, torch.Tensor)}, "tensor_kw": sorted(n for n, t in kwargs.items() if isinstance(t, torch.Tensor)), "n_out": len(res), "checks": checks, "source": f"{rel}::{tname}",
                      "models_built_before": len(records) - 1}
        print("kat_reference_held", key, "ok:", [c[0] for c in checks])
    out["index"] = np.array(json.dumps(index))
    np.savez_compressed(os.path.join(GOLD, "kat_reference_held.npz"), **out)


def reference_kat_status():
    """Run the reference's own known-answer tests for the path in this container and record the result."""
    files = ["tests/models", "tests/utils/test_graph_utils.py", "tests/utils/test_cc_utils.py",
             "tests/utils/test_models_utils.py"]
    code = ("import sys; sys.path.insert(0, %r); import refshim; refshim.install(); import pytest; "
            "sys.exit(pytest.main(['-q','-p','no:cacheprovider','--no-header','-k',"
            "'(ScoreNetwork or hodge or mask or noise or quantize or pow_tensor or get_cells or rank2_dim or get_ones or hodgedual or hodge_laplacian or default_mask) and not spectrum',"
            " *%r]))" % (HERE, files))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=refshim.REFERENCE_ROOT, env=env, capture_output=True, text=True)
    tail = (r.stdout.strip().splitlines() or [""])[-1]
    with open(os.path.join(GOLD, "reference_kat_status.json"), "w") as f:
        json.dump({"returncode": r.returncode, "summary": tail}, f, indent=1)
    print("reference KATs:", r.returncode, tail)


def shipped():
    """The eight shipped checkpoints of SHIPPED: converted weights under tests/golden/ckpt/, g1 forwards at the full node count
    and a smaller one, g5 short runs at the sampler settings of each checkpoint's own sample_*.yaml (a sibling's where it has
    none).  ego_small_CC-sized rank-2 tensors are stored as summaries (summarize)."""
    pc = dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1)       # sample_qm9*.yaml
    ego = dict(predictor="Euler", corrector="None", snr=0.0, scale_eps=0.0, n_steps=1)            # sample_ego_small*.yaml
    enz = dict(predictor="S4", corrector="None", snr=0.15, scale_eps=0.7, n_steps=1)              # sample_enzymes_small*.yaml
    runs = {                      # name -> (g1 counts, g5 sampler, g5 counts)
        "gdss_qm9": ([9, 6], pc, [9, 7]),
        "gdss_qm9_retrained": ([9, 6], pc, [9, 7]),
        "gdss_ego_small": ([18, 11], ego, [18, 9]),
        "gdss_ego_small_retrained": ([18, 11], ego, [18, 9]),
        "gdss_enzymes_small_retrained": ([12, 8], enz, [12, 9]),
        "ccsd_enzymes_small_Base_CC": ([12, 8], enz, [12, 9]),
        "ccsd_ego_small_CC": ([18, 11], ego, [18, 9]),
        "ccsd_ego_small_CC_v2": ([18, 11], ego, [18, 9]),
    }
    for name, (g1c, smp, g5c) in runs.items():
        _, is_cc = SHIPPED[name]
        ck = export_checkpoint(name, SHIPPED, SHIPPED_CKPT)
        big = name.startswith("ccsd_ego_small")
        g1_network_forwards(name, ck, is_cc, 2, g1c, summarize_large=big)
        g5_pc_runs(name, ck, is_cc, 2, g5c, smp, {"k6": (6, None), "n1000_first2": (None, 2)}, seed=42, min_dist=5e-3,
                   summarize_large=big)
        print("shipped", name)


def large_graph():
    """The two generic-graph checkpoints above 64 nodes (the tiled graph-network route): converted weights under tests/golden/ckpt/,
    g1 forwards of ENZYMES at B = 3, g5 first steps (arrays above 256 KB as summaries) of the shipped 1000-scale samplers:
    ENZYMES S4 (sample_enzymes.yaml), grid Reverse + Langevin (sample_grid.yaml)."""
    enz = dict(predictor="S4", corrector="None", snr=0.15, scale_eps=0.7, n_steps=1)
    grid = dict(predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7, n_steps=1)
    # (grid: no g1 file -- two 361 x 361 inputs alone exceed MAX_FIXTURE; its forward tests take the oracle on the committed weights)
    for name, g1c, smp, g5c in (("gdss_enzymes", [125, 37, 1], enz, [125, 60]), ("gdss_grid", None, grid, [361, 144])):
        ck = export_checkpoint(name, SHIPPED, SHIPPED_CKPT)
        if g1c:
            g1_network_forwards(name, ck, False, len(g1c), g1c, summarize_large=True)
        g5_pc_runs(name, ck, False, 2, g5c, smp, {"n1000_first3": (None, 3)}, seed=42, summarize_large=1 << 18)
        print("large graph", name)


def grid_small_cc():
    """ccsd_grid_small_CC (N = 49, d = 3: E = 1176, K = 18424; ScoreNetworkA_CC with one hodge layer): the weights
    sample_grid_small_CC.yaml samples with (use_ema: the EMA-applied ones) under tests/golden/ckpt/cc_large/, g1 forwards at B = 2 and
    the first two steps of the shipped 1000-scale sampler (Reverse + Langevin, snr 0.1, scale_eps 0.7, the yaml's seed), rank-2
    arrays as summaries."""
    name = "ccsd_grid_small_CC"
    smp = dict(predictor="Reverse", corrector="Langevin", snr=0.1, scale_eps=0.7, n_steps=1)
    ck = export_checkpoint(name, SHIPPED, CC_LARGE_CKPT, apply_ema=True)
    g1_network_forwards(name, ck, True, 2, [49, 30], summarize_large=True, rank2_score=False)
    g5_pc_runs(name, ck, True, 2, [49, 30], smp, {"n1000_first2": (None, 2)}, seed=12, summarize_large=True)
    print("grid_small_cc", name)


# ScoreNetworkA_Base_CC on the tiled graph-network route (`python tools/make_golden.py base_cc_route`): no such checkpoints ship, the
# A-networks come from the reference's constructor under a fixed seed (biases perturbed, as in the kat_* fixtures).  Kept in a folder
# of its own below ckpt/, like CC_LARGE_CKPT.
BASE_CC_CKPT = os.path.join(SHIPPED_CKPT, "base_cc_route")
# the A-network of config/grid_small_Base_CC.yaml (its `num_layers_mlp: !` keeps the file itself from loading)
GRID_BASE_ADJ = dict(model_type="ScoreNetworkA_Base_CC", is_cc=True, max_feat_num=5, max_node_num=49, nhid=24, num_layers=6, num_linears=2,
                     c_init=2, c_hid=4, c_final=4, adim=24, num_heads=4, conv="GCN", use_bn=False, d_min=3, d_max=3, nhid_h=2,
                     num_layers_h=2, num_linears_h=1, c_hid_h=2, c_final_h=2, hidden_h=2)


def _constructed(params, seed):
    """A network from the reference's constructor under torch.manual_seed(seed), biases drawn N(0, 0.2) (the reference zeroes them)."""
    ref_cc.default_mask.cache_clear()            # (see build_models)
    torch.manual_seed(seed)
    m = ref_loader.load_model(params)
    for k, p_ in m.named_parameters():
        if k.endswith("bias"):
            p_.data.normal_(0, 0.2)
    return m.eval()


def _write_constructed(name, cfg, params, state_dicts, note):
    """A checkpoint-shaped fixture under BASE_CC_CKPT (json + one npz below MAX_FIXTURE), and the dict build_models takes."""
    os.makedirs(BASE_CC_CKPT, exist_ok=True)
    arrays = {f"{p}/{k}": v.detach().cpu().numpy().astype(np.float32) for p, sd in state_dicts.items() for k, v in sd.items()}
    path = os.path.join(BASE_CC_CKPT, name + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= MAX_FIXTURE, (name, os.path.getsize(path))
    meta = {"name": name, "source": note, "is_cc": True, "config": plain(cfg), "files": [os.path.relpath(path, SHIPPED_CKPT)]}
    meta.update({f"params_{p}": plain(v) for p, v in params.items()})
    with open(os.path.join(BASE_CC_CKPT, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    ck = {"model_config": refshim.EasyDict(cfg)}
    for p in params:
        ck[f"params_{p}"], ck[f"{p}_state_dict"] = params[p], state_dicts[p]
    return ck


def base_cc_route():
    """(a) The A-network of grid_small_Base_CC.yaml (N = 49, two HodgeBaselineLayers) beside the X and F networks of the
    cc_large/ccsd_grid_small_CC fixture: g1 forwards at B = 2 (counts 49 and 30).  (b) The networks of ego_small_Base_CC.yaml (three
    HodgeBaselineLayers) at N = 7, d 3..5 (E = 21, K = 91): g1 forwards and two steps of the yaml's sampler (Euler, no corrector) at 4
    scales; at N = 12, d 3..4 (E = 66: four row tiles + 2): g1 forwards."""
    import yaml

    with open(os.path.join(CC_LARGE_CKPT, "ccsd_grid_small_CC.json")) as f:
        gm = json.load(f)
    z = {}
    for fname in gm["files"]:
        a = np.load(os.path.join(SHIPPED_CKPT, fname))
        z.update({k: a[k] for k in a.files})
    sds = {p: {k.split("/", 1)[1]: torch.from_numpy(v) for k, v in z.items() if k.startswith(p + "/")} for p in ("x", "rank2")}
    sds["adj"] = _constructed(GRID_BASE_ADJ, 4901).state_dict()
    cfg = dict(gm["config"], model=dict(gm["config"]["model"], adj="ScoreNetworkA_Base_CC", c_hid=4, hidden_h=2))
    name = "ccsd_grid_small_Base_CC"
    ck = _write_constructed(name, cfg, {"x": gm["params_x"], "adj": GRID_BASE_ADJ, "rank2": gm["params_rank2"]}, sds,
                            "A-network: reference constructor, torch.manual_seed(4901); X and F networks: cc_large/ccsd_grid_small_CC")
    g1_network_forwards(name, ck, True, 2, [49, 30], summarize_large=True, rank2_score=False)

    with open(os.path.join(refshim.REFERENCE_ROOT, "config", "ego_small_Base_CC.yaml")) as f:
        ego = yaml.safe_load(f)
    smp = dict(ego["sampler"], sde_override={p: {"num_scales": 4} for p in ("x", "adj", "rank2")})
    for N, d_max, counts, seed in ((7, 5, [7, 5, 0, 1, 2], 701), (12, 4, [12, 7, 0, 1, 2], 1201)):
        cfg = dict(ego, data=dict(ego["data"], max_node_num=N, d_max=d_max))
        px, pa, pf = ref_loader.load_model_params(refshim.EasyDict(cfg), is_cc=True)
        params = {"x": dict(px), "adj": dict(pa), "rank2": dict(pf)}
        sds = {p: _constructed(params[p], seed + i).state_dict() for i, p in enumerate(("x", "adj", "rank2"))}
        name = f"ccsd_ego_small_Base_CC_n{N}"
        ck = _write_constructed(name, cfg, params, sds, f"reference constructors, torch.manual_seed({seed} + part index)")
        g1_network_forwards(name, ck, True, len(counts), counts, summarize_large=True)
        if N == 7:
            g5_pc_runs(name, ck, True, 2, [7, 5], smp, {"n4_first2": (None, 2)}, seed=12)
    print("base_cc_route done")


# ---------------------------------------------------------------------------------------------
# e5_lift.npz: the reference's path_based lifting of graphs and what its evaluators make of the lifted complexes
# (`python tools/make_golden.py lift`)
# ---------------------------------------------------------------------------------------------
def e5_lift():
    """e5_lift.npz: convert_graphs_to_CCs(graphs, False, "path_based", "basic", max_nb_nodes=N) of the reference on two sets of 24 graphs
    at N = 12 and at N = 20 (d_min = d_max = 3), then its own CC_to_incidence_matrices, rank2_distrib_worker,
    hodge_laplacian_spectrum_worker and eval_CC_list on the lifted complexes.  Stored per graph: the cell bits of the padded incidence
    matrix, the size histogram, its number of ones and the float32 spectrum -- no dense tensor.  gaussian_emd ran on the stand-in pyemd,
    the complexes on _StandInComplex; lp_vs_closed / f32_vs_f64 as in e2_spectrum.npz.  The hodge score costs one linear program of
    E^2 variables per pair, so it is recorded on the first `hodge_nb` complexes of each side."""
    import threading
    import time

    import networkx as nx

    record = {"tl": threading.local()}
    stand_in = _pyemd_stand_in(record)
    sys.modules["pyemd"] = stand_in
    from ccsd.src.evaluation import mmd as ref_mmd

    ref_mmd.pyemd = stand_in
    ref_cc.CombinatorialComplex = _StandInComplex
    t0 = time.time()
    out, meta = {}, {"sets": {}, "lp_vs_closed": {}, "f32_vs_f64": {}}
    worst = {"v": 0.0}

    def k_emd(x, y, **kw):
        record["tl"].mode = "closed"
        try:
            kc = ref_mmd.gaussian_emd(x, y, **kw)
        finally:
            record["tl"].mode = "lp"
        kl = ref_mmd.gaussian_emd(x, y, **kw)
        worst["v"] = max(worst["v"], abs(float(kl) - float(kc)))
        return kl

    def graphs_of(rng, N, B, p, d_min, d_max):
        """B graphs with their lifted complexes.  A graph whose hodge Laplacian the reference's LAPACK call gives up on (the worker then
        returns zeros of the UNPADDED length, cc_utils.py:1013-1019) is drawn again: that path is the solver's, not the lifting's."""
        adj = np.zeros((B, N, N), np.int8)
        ccs, b = [], 0
        while b < B:
            n = N - int(rng.integers(0, 5)) if b else N              # (masked slots at the end, as finished samples have them)
            u = np.triu(rng.random((n, n)) < p[b % len(p)], 1)
            u[0, 1] |= not u.any()                                   # (path_based_lift_CC reads the rank-1 cells of its input: a graph has an edge)
            g = nx.Graph()
            g.add_nodes_from(range(n))
            for i, j in zip(*np.nonzero(u)):
                g.add_edge(int(i), int(j), label=1)
            (cc,) = ref_cc.convert_graphs_to_CCs([g], False, "path_based", "basic", max_nb_nodes=N)
            spec = ref_cc.hodge_laplacian_spectrum_worker(cc, d_min, d_max, N)
            F = ref_cc.CC_to_incidence_matrices(cc, d_min, d_max)[2]
            f64 = np.zeros(N * (N - 1) // 2)
            if F.size:
                F = np.asarray(ref_cc.pad_rank2(F, node_number=N, d_min=d_min, d_max=d_max), np.float64)
                f64 = np.linalg.eigvalsh(F @ F.T)
            # (... or returns without an exception what is no spectrum: NaNs, or values off by more than float32 can explain)
            if len(spec) != len(f64) or not np.isfinite(spec).all() or np.abs(spec - f64).max() > 1e-4 * max(1.0, f64.max()):
                meta["redrawn"] = meta.get("redrawn", 0) + 1
                continue
            adj[b] = 0
            adj[b, :n, :n] = u + u.T
            ccs.append(cc)
            b += 1
        return adj, ccs

    for N, hodge_nb in ((12, 6), (20, 3)):
        d_min = d_max = 3
        E, K = N * (N - 1) // 2, ref_cc.get_rank2_dim(N, d_min, d_max)[1]
        rng = np.random.default_rng(20261020 + N)
        wk = {"min_edge_val": 1, "max_edge_val": 1, "edge_label": "label", "d_min": d_min, "d_max": d_max, "N": N}
        ccs, f32 = {}, 0.0
        for side, p in (("ref", (0.15, 0.3, 0.5)), ("pred", (0.2, 0.4, 0.1))):
            adj, ccs[side] = graphs_of(rng, N, 24, p, d_min, d_max)
            bits = np.zeros((24, (K + 63) // 64), np.uint64)
            hist, nnz, spec = np.zeros((24, 1), np.int32), np.zeros(24, np.int32), np.zeros((24, E), np.float32)
            for b, cc in enumerate(ccs[side]):
                F = ref_cc.CC_to_incidence_matrices(cc, d_min, d_max)[2]
                if F.size:
                    F = np.asarray(ref_cc.pad_rank2(F, node_number=N, d_min=d_min, d_max=d_max))
                    assert F.shape == (E, K) and set(np.unique(F).tolist()) <= {0.0, 1.0}
                    for k in np.nonzero(F.any(0))[0]:
                        bits[b, k >> 6] |= np.uint64(1 << int(k & 63))
                    nnz[b] = int(F.sum())
                    f32 = max(f32, float(np.abs(np.linalg.eigvalsh(F.astype(np.float64) @ F.T.astype(np.float64)) -
                                                ref_cc.hodge_laplacian_spectrum_worker(cc, d_min, d_max, N).astype(np.float64)).max()))
                hist[b] = ref_cc.rank2_distrib_worker(cc, d_min, d_max)
                spec[b] = ref_cc.hodge_laplacian_spectrum_worker(cc, d_min, d_max, N)
                assert int(hist[b].sum()) == len(cc.cells.hyperedge_dict.get(2, {}))
            out[f"n{N}/{side}/adj"], out[f"n{N}/{side}/bits"], out[f"n{N}/{side}/hist"] = adj, bits, hist
            out[f"n{N}/{side}/nnz"], out[f"n{N}/{side}/spectrum"] = nnz, spec
        meta["f32_vs_f64"][f"n{N}/eig"] = f32
        kern = {m: k_emd for m in ("hodge_laplacian_spectrum", "rank1_distrib", "rank2_distrib")}
        worst["v"] = 0.0
        meta[f"eval_CC_list/n{N}"] = ref_cc.eval_CC_list(ccs["ref"], ccs["pred"], wk, methods=["rank1_distrib", "rank2_distrib"], kernels=kern, cc_nb_eval=1000)
        meta["lp_vs_closed"][f"eval_CC_list/n{N}"] = worst["v"]
        worst["v"] = 0.0
        meta[f"eval_CC_list/n{N}/first{hodge_nb}"] = ref_cc.eval_CC_list(ccs["ref"], ccs["pred"], wk, methods=list(kern), kernels=kern, cc_nb_eval=hodge_nb)
        meta["lp_vs_closed"][f"eval_CC_list/n{N}/first{hodge_nb}"] = worst["v"]
        # the hodge score again from float64 eigenvalues rounded to float32 once: what the solver's precision is worth in the score
        rows = []
        for side in ("ref", "pred"):
            r = []
            for cc in ccs[side][:hodge_nb]:
                if side == "pred" and ref_cc.is_empty_cc(cc):
                    continue
                F = ref_cc.CC_to_incidence_matrices(cc, d_min, d_max)[2]
                if F.size:
                    F = np.asarray(ref_cc.pad_rank2(F, node_number=N, d_min=d_min, d_max=d_max), np.float64)
                    r.append(np.linalg.eigvalsh(F @ F.T).astype(np.float32))
                else:
                    r.append(np.zeros(E, np.float32))
            rows.append(r)
        unrounded = float(ref_cc.hodge_laplacian_spectrum_stats(ccs["ref"][:hodge_nb], ccs["pred"][:hodge_nb], wk, k_emd, is_parallel=False))
        meta["f32_vs_f64"][f"eval_CC_list/n{N}/first{hodge_nb}"] = abs(float(ref_mmd.compute_mmd(rows[0], rows[1], kernel=k_emd)) - unrounded)
        meta["sets"][f"n{N}"] = {"N": N, "d_min": d_min, "d_max": d_max, "E": E, "K": K, "hodge_nb": hodge_nb, "worker_kwargs": wk}
        print("e5 lift n", N, round(time.time() - t0, 1), "s", record.get("programs", 0), "programs")
    meta["programs"], meta["seconds"] = record.get("programs", 0), round(time.time() - t0, 1)
    out["meta"] = np.array(json.dumps(plain(meta)))
    path = os.path.join(GOLD, "e5_lift.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= MAX_FIXTURE, os.path.getsize(path)
    print("wrote e5_lift", os.path.getsize(path), "bytes;", meta["programs"], "programs,", meta["seconds"], "s")


def main():
    only = set(sys.argv[1:])
    if only == {"lift"}:
        e5_lift()
        return
    if only == {"f1"}:
        f1_finish()
        return
    if only == {"eval"}:
        e1_eval()
        return
    if only == {"spectrum"}:
        e2_spectrum()
        return
    if only == {"orbit"}:
        e3_orbit()
        return
    if only == {"nspdk"}:
        e4_nspdk()
        return
    if only == {"d1"}:
        # ~a quarter of an hour of reference CPU time was the estimate; the fixture's metadata holds what it took
        d1_qm9_cc_n1000(raw=os.environ.get("CCSD_D1_RAW"))
        return
    if only == {"base_cc_route"}:
        base_cc_route()
        return
    if only == {"kat_hodge_wide"}:
        kat_hodge_wide()
        return
    if only == {"kat_arch_sweep"}:
        kat_arch_sweep()
        return
    if only == {"grid_small_cc"}:
        grid_small_cc()
        return
    if only == {"shipped"}:
        shipped()
        return
    if only == {"large"}:
        large_graph()
        return
    cks = {}
    for name in CHECKPOINTS:
        cks[name] = export_checkpoint(name)
        print("exported", name)
    if not only or "g3" in only:
        g3_sde_tables()
    if not only or "g6" in only:
        g6_masks()
    if not only or "g7" in only:
        g7_init_flags()
    if not only or "kat" in only:
        kat_small_models()
    if not only or "g1" in only:
        g1_network_forwards("ccsd_qm9_CC", cks["ccsd_qm9_CC"], True, 4, [9, 8, 7, 5])
        g1_network_forwards("ccsd_community_small_CC", cks["ccsd_community_small_CC"], True, 2, [20, 14])
        g1_network_forwards("ccsd_enzymes_small_CC", cks["ccsd_enzymes_small_CC"], True, 2, [12, 9])
        g1_network_forwards("gdss_community_small", cks["gdss_community_small"], False, 4, [20, 18, 14, 12])
        g1_network_forwards("gdss_zinc250k", cks["gdss_zinc250k"], False, 2, [38, 23])
    if not only or "g5" in only:
        g5_pc_runs("ccsd_qm9_CC", cks["ccsd_qm9_CC"], True, 4, [9, 8, 7, 5],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1),
                   {"k10": (10, None), "k50": (50, None), "n1000_first3": (None, 3)}, seed=42)
        g5_pc_runs("ccsd_community_small_CC", cks["ccsd_community_small_CC"], True, 2, [20, 14],
                   dict(predictor="Euler", corrector="Langevin", snr=0.05, scale_eps=0.7, n_steps=1),
                   {"k5": (5, None), "n1000_first2": (None, 2)}, seed=12)
        g5_pc_runs("gdss_community_small", cks["gdss_community_small"], False, 4, [20, 18, 14, 12],
                   dict(predictor="Euler", corrector="Langevin", snr=0.05, scale_eps=0.7, n_steps=1),
                   {"k10": (10, None), "n1000_first3": (None, 3)}, seed=12)
        g5_pc_runs("gdss_zinc250k", cks["gdss_zinc250k"], False, 2, [38, 23],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.9, n_steps=1),
                   {"k5": (5, None)}, seed=42)
        g5_pc_runs("ccsd_qm9_CC_nsteps2_none", cks["ccsd_qm9_CC"], True, 2, [9, 6],
                   dict(predictor="Euler", corrector="None", snr=0.2, scale_eps=0.7, n_steps=1),
                   {"k6": (6, None)}, seed=5)
        g5_pc_runs("ccsd_qm9_CC_langevin2", cks["ccsd_qm9_CC"], True, 2, [9, 6],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=2),
                   {"k4": (4, None)}, seed=6)
    if "full" in only:
        # One FULL-LENGTH run: the shipped sampling set-up of qm9_CC (1000 scales, Reverse + Langevin) from the prior to the last
        # step, every draw from torch's CPU generator.  ~2.5 minutes of reference CPU time: made on request only
        # (python tools/make_golden.py full), the other fixtures are unaffected.
        g5_pc_runs("ccsd_qm9_CC_full1000", cks["ccsd_qm9_CC"], True, 2, [9, 7],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1),
                   {"n1000": (None, None)}, seed=77, min_dist=5e-3)
    if not only or "s4" in only:
        # S4_solver (solver.py:1179-1563): the sampler the shipped ENZYMES_small_CC config selects
        s4 = dict(predictor="S4", corrector="None", snr=0.15, scale_eps=0.7, n_steps=1)
        g5_pc_runs("s4_ccsd_enzymes_small_CC", cks["ccsd_enzymes_small_CC"], True, 2, [12, 9], s4,
                   {"k4": (4, None), "k20": (20, None), "n1000_first2": (None, 2)}, seed=42)
        g5_pc_runs("s4_ccsd_qm9_CC", cks["ccsd_qm9_CC"], True, 4, [9, 8, 7, 5], s4, {"k6": (6, None)}, seed=7)
        g5_pc_runs("s4_gdss_community_small", cks["gdss_community_small"], False, 4, [20, 18, 14, 12], s4,
                   {"k5": (5, None)}, seed=9)
    if not only or "sdevar" in only:
        # subVPSDE (sde.py:672-786; Euler and, through the base-class discretize sde.py:93-111, Reverse) and
        # probability_flow=True with the Reverse predictor (sde.py:329-340).  No shipped config selects them.
        sub = dict(type="subVP", beta_min=0.1, beta_max=1.0)
        subv = {"x": sub, "adj": sub, "rank2": sub}
        g5_pc_runs("ccsd_qm9_CC_subvp_euler", cks["ccsd_qm9_CC"], True, 3, [9, 7, 5],
                   dict(predictor="Euler", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1, sde_override=subv),
                   {"k6": (6, None)}, seed=21, min_dist=5e-3)
        g5_pc_runs("ccsd_qm9_CC_subvp_reverse", cks["ccsd_qm9_CC"], True, 3, [9, 7, 5],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1, sde_override=subv),
                   {"k6": (6, None)}, seed=22, min_dist=5e-3)
        g5_pc_runs("ccsd_qm9_CC_pflow", cks["ccsd_qm9_CC"], True, 3, [9, 8, 6],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1, probability_flow=True),
                   {"k6": (6, None)}, seed=23, min_dist=5e-3)
        g5_pc_runs("gdss_community_small_pflow", cks["gdss_community_small"], False, 3, [20, 16, 12],
                   dict(predictor="Reverse", corrector="None", snr=0.05, scale_eps=0.7, n_steps=1, probability_flow=True),
                   {"k5": (5, None)}, seed=24, min_dist=5e-3)
        # mixed: subVP on x only, the checkpoint's VE on adj / rank2, Reverse + Langevin with two inner steps
        g5_pc_runs("ccsd_qm9_CC_subvp_mixed", cks["ccsd_qm9_CC"], True, 2, [9, 6],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=2, sde_override={"x": sub}),
                   {"k4": (4, None)}, seed=25, min_dist=5e-3)
    if not only or "zinc5b" in only:
        kat_zinc5b()
    if not only or "cnum" in only:
        kat_cnum()
    if not only or "hlayers" in only:
        kat_hodge_layers()
    if not only or "hgeneral" in only:
        kat_hodge_general()
    if not only or "gmh" in only:
        kat_gmh_models()
    if not only or "base" in only:
        # ScoreNetworkA_Base_CC (ScoreNetwork_A_Base_CC.py, hodge_layers.py:202-416): forwards and short sampler runs
        g1_network_forwards("ccsd_qm9_Base_CC", cks["ccsd_qm9_Base_CC"], True, 4, [9, 8, 7, 5])
        g1_network_forwards("ccsd_community_small_Base_CC", cks["ccsd_community_small_Base_CC"], True, 2, [20, 14])
        g5_pc_runs("ccsd_qm9_Base_CC", cks["ccsd_qm9_Base_CC"], True, 4, [9, 8, 7, 5],
                   dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1),
                   {"k10": (10, None), "n1000_first3": (None, 3)}, seed=42)
    if not only or "refkat" in only:
        reference_kat_status()
    if not only or "refheld" in only:
        kat_reference_held()
    if not only or "variants" in only:
        reference_variant_status()
    if not only or "modules" in only:
        reference_module_objects()


if __name__ == "__main__":
    main()
