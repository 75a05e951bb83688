"""Cases of the input classes the step calls promise to accept (include/ccsd_hip.h) and that no other file runs: node masks with holes
and states that are not masked.  Shared by the host-emulation suite (tests/test_state_classes.py) and the GPU suite
(tests/test_gpu_state_classes.py, -m gpu); `lib` / `device` select the backend.

    class   flags                         state (tests/helpers.make_state)
    H       holes (make_flags_holes)      masked
    U       prefix (make_flags)           unmasked: the rows of switched-off nodes carry values
    HU      holes                         unmasked
    D       prefix                        masked, plus a random diagonal on the adjacency

Everything against the oracle takes parity_cases.assert_close at its defaults; two instances of the same source must agree in bits.
Asymmetric adjacencies are not a class: their result is declared route-dependent (include/ccsd_hip.h), not pinned."""
import contextlib
import json

import pytest
import torch

from ccsd_amd import loader
from ccsd_amd.engine import PCEngine
from oracle import ccsd_oracle as O
from tests import arch_sweep_cases as sw
from tests import cc_large_graph_cases as cc
from tests import hodge_wide_cases as hw
from tests import large_graph_cases as lc
from tests import noise_cases as nc
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np, load_golden, make_flags, make_flags_holes, make_state

CLASSES = {"H": ("holes", "masked"), "U": ("prefix", "unmasked"), "HU": ("holes", "unmasked"), "D": ("prefix", "diag")}
NAMES = ["x", "adj", "rank2"]


def counts_of(N):
    """B = 6: a full sample, two partial ones (make_flags_holes gives them the two edge patterns) and the cell-free 0, 1, 2."""
    return [N, N - 2, N // 2 + 1, 0, 1, 2]


@contextlib.contextmanager
def environment(env, unset=()):
    """Plan switches are read from the environment at plan creation: `env` set and `unset` removed for the block through pytest's
    monkeypatch, which puts everything back as it was."""
    with pytest.MonkeyPatch.context() as mp:
        for k in unset:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        yield


def dims(meta):
    d = meta["config"]["data"]
    return (d["max_node_num"], d["max_feat_num"]) + ((d["d_min"], d["d_max"]) if meta["is_cc"] else (0, 0))


def engine(meta, parts, lib, device, env=None, unset=(), **kw):
    N, F, d_min, d_max = dims(meta)
    slots = []
    for p in NAMES:
        slots += [meta.get(f"params_{p}"), parts.get(p)]
    with environment(env or {}, unset):
        return PCEngine(*slots, N=N, F=F, is_cc=meta["is_cc"], d_min=d_min, d_max=d_max, device=device, lib=lib, **kw)


def class_inputs(cls, meta, seed, scale=1.0, counts=None):
    """(flags, state) of one class for the geometry of `meta`."""
    N, F, d_min, d_max = dims(meta)
    counts = counts or counts_of(N)
    how, kind = CLASSES[cls]
    flags = make_flags_holes(len(counts), N, counts, seed) if how == "holes" else make_flags(len(counts), N, counts)
    return flags, make_state(kind, seed, len(counts), N, F, meta["is_cc"], d_min, d_max, flags, scale)


def live_masks(meta, flags):
    """[x, adj, rank2] 0/1 masks of the entries that belong to live nodes."""
    N, F, d_min, d_max = dims(meta)
    B = flags.shape[0]
    m = [O.mask_x(torch.ones(B, N, F), flags), flags[:, :, None] * flags[:, None, :]]
    if meta["is_cc"]:
        m.append(O.mask_rank2(torch.ones(B, *O.get_rank2_dim(N, d_min, d_max)), N, d_min, d_max, flags))
    return m


def oracle_share(meta, parts, p, state, flags, ref):
    """The float32 oracle against its own float64 evaluation, as the share of assert_close's allowances it uses up (condition (c) of
    arch_sweep_cases.case_conditions, which holds random-weight networks to a quarter)."""
    f64 = lambda t: None if t is None else t.double()
    with torch.no_grad(), pc.f64_arithmetic():
        exact = O.run_network(meta[f"params_{p}"], {k: v.detach().double() for k, v in parts[p].items()}, *(f64(t) for t in state), flags.double())
    scale = ref.abs().max().item()
    err = (ref.double() - exact).abs()
    big = exact.abs() > 1e-2 * scale
    return max((err.max() / (pc.RTOL * scale)).item(), (err / (pc.RTOL * exact.abs() + pc.ATOL_SCALE * scale))[big].max().item())


# ---- a. forwards: ccsd_score for every target against O.run_network on the same tensors
def check_forwards(route, meta, parts, engines, device, classes=tuple(CLASSES), seed=5, scale=1.0, counts=None, bit_equal=(),
                   random_weights=False, flag_check=None):
    """Every network of `meta` on every class, through every engine of `engines` ({label: engine}, plans of the same networks), against
    the oracle computed once per class.  bit_equal: classes on which the engines must agree in bits.  random_weights: the oracle must
    lie within a quarter of the tolerance of its float64 evaluation on these inputs (else the case's scale is too large for the
    comparison to mean the kernel).  flag_check(flags): asserts what the case needs of its holed flags."""
    targets = [p for p in NAMES if f"params_{p}" in meta and parts.get(p) is not None]
    dv = lambda t: None if t is None else t.to(device)
    for cls in classes:
        flags, state = class_inputs(cls, meta, seed, scale, counts)
        if flag_check is not None and CLASSES[cls][0] == "holes":
            flag_check(flags)
        args = [dv(t) for t in state] + [dv(flags)]
        outs = {}
        for p in targets:
            with torch.no_grad():
                want = O.run_network(meta[f"params_{p}"], parts[p], *state, flags)
            if random_weights:
                share = oracle_share(meta, parts, p, state, flags, want)
                assert share <= 0.25, f"{route} {cls}: the float32 oracle's net_{p} uses {share:.2f} of the tolerance against float64: lower the scale"
            for label, eng in engines.items():
                got = eng.score(NAMES.index(p), *args)
                pc.assert_close(got, want, f"{route} [{label}] class {cls} net_{p}")
                if p == "adj":
                    cc.check_adj_masks(got, flags, f"{route} [{label}] class {cls}")
                outs.setdefault(p, []).append((label, got.cpu()))
        if cls in bit_equal:
            for p, got in outs.items():
                for label, g in got[1:]:
                    assert torch.equal(got[0][1], g), f"{route} class {cls} net_{p}: [{got[0][0]}] and [{label}] differ in bits"


def expect(eng, what, **route):
    for q, v in route.items():
        assert eng.query(q) == v, f"{what}: plan query {q} = {eng.query(q)}, expected {v}"
    return eng


def case_forward_qm9_instances(lib, device):
    """k_xa + fused k_r2, qm9_CC: the baked-plan instance (the bench batch's plan: xa_variant 7, k_r2<3, 1, true, false, 2>), its
    geometry-only twin under CCSD_NO_BAKE (4, k_r2<.., 1>) and the run-time instances under CCSD_NO_GEO (0, k_r2<.., 0>): each against
    the oracle, and all three in equal bits on every class."""
    meta, parts = load_ckpt_np("ccsd_qm9_CC")
    sdes = [loader.load_sde(meta["config"]["sde"][p]) for p in NAMES]
    kw = dict(sdes=sdes, predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1, eps=1e-4, batch_hint=1024)
    engs = {"baked": expect(engine(meta, parts, lib, device, **kw), "qm9_CC", xa_variant=7, r2_instance=31102, fused_r2=1, large_graph=0),
            "no bake": expect(engine(meta, parts, lib, device, {"CCSD_NO_BAKE": "1"}, **kw), "qm9_CC CCSD_NO_BAKE", xa_variant=4, r2_instance=31101),
            "no geo": expect(engine(meta, parts, lib, device, {"CCSD_NO_GEO": "1"}, **kw), "qm9_CC CCSD_NO_GEO", xa_variant=0, r2_instance=31100)}
    check_forwards("k_xa + fused k_r2 (qm9_CC)", meta, parts, engs, device, bit_equal=tuple(CLASSES))


# name -> (what the plan must answer, seed)
CHECKPOINTS = {
    "ccsd_community_small_CC": dict(large_graph=0, r2_family=3, h_general=0),                   # k_xa + tiled rank-2
    "ccsd_enzymes_small_CC": dict(large_graph=0, r2_family=3, xa_variant=10),                  # two hodge layers: k_xa<., XA_GEN>, baked
    "ccsd_qm9_Base_CC": dict(large_graph=0, xa_variant=1, r2_family=1),
    "ccsd_community_small_Base_CC": dict(large_graph=0, xa_variant=1, r2_family=3),
    "gdss_community_small": dict(large_graph=0, r2_family=0, xa_variant=5),
    "gdss_zinc250k": dict(large_graph=0, r2_family=0, xa_variant=6),                           # channel stack in HBM
}


def case_forward_checkpoint(name, lib, device, classes=tuple(CLASSES)):
    meta, parts = load_ckpt_np(name)
    eng = expect(engine(meta, parts, lib, device), name, **CHECKPOINTS[name])
    check_forwards(name, meta, parts, {"default": eng}, device, classes)


def case_forward_ew1(lib, device, N=12):
    """k_ew1: the zinc250k_CC substitute's architecture (cnum = 1, affine) at N = 12, d = 3..4, the smallest N whose plan is k_ew1's."""
    meta, parts, _ = pc.zinc5b_at(N, 3, 4)
    eng = expect(engine(meta, parts, lib, device), f"zinc250k_CC_5b@{N}", r2_family=2, large_graph=0)
    check_forwards(f"k_ew1 (zinc250k_CC_5b@{N})", meta, parts, {"default": eng}, device)


def _kat_source(params, sd):
    N, F = params["max_node_num"], params["max_feat_num"]
    meta = {"is_cc": True, "params_adj": params,
            "config": {"data": dict(max_node_num=N, max_feat_num=F, d_min=params["d_min"], d_max=params["d_max"])}}
    return meta, {"adj": {k: v.clone().requires_grad_(True) for k, v in sd.items()}}


def case_forward_hodge_general(lib, device, tag="G3_n5"):
    """The general hodge stack: a reference-built ScoreNetworkA_CC with three layers of true-MLP mlp_value (kat_hodge_general)."""
    g = load_golden("kat_hodge_general.npz")
    params = json.loads(str(g["meta"]))[tag]
    sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/w/")}
    meta, parts = _kat_source(params, sd)
    eng = expect(engine(meta, parts, lib, device), tag, h_general=1)
    check_forwards(f"general hodge stack ({tag})", meta, parts, {"default": eng}, device)


def case_forward_hodge_wide(lib, device, tag="W2_n9"):
    """A wide plan (hodge MLPs 9 to 16 wide: the 16-wide kernels of the tiled route and of the tiled rank-2 family), kat_hodge_wide."""
    params, sd = hw.kat_tag(tag)[:2]
    meta, parts = _kat_source(params, sd)
    eng = expect(engine(meta, parts, lib, device, unset=("CCSD_LARGE_GRAPH",)), tag, h_wide=1, large_graph=1, r2_family=3)
    check_forwards(f"wide hodge plan ({tag})", meta, parts, {"default": eng}, device)


FORCED = {"gdss_community_small": "1", "ccsd_qm9_CC": "2", "ccsd_qm9_Base_CC": "2"}


def case_forward_forced_tiled(name, lib, device):
    """The tiled graph-network route (k_lg_*) forced onto a plan k_xa serves, next to the k_xa plan of the same networks."""
    meta, parts = load_ckpt_np(name)
    engs = {"k_xa": expect(engine(meta, parts, lib, device), name, large_graph=0),
            "tiled": expect(engine(meta, parts, lib, device, {"CCSD_LARGE_GRAPH": FORCED[name]}), f"{name} CCSD_LARGE_GRAPH={FORCED[name]}",
                            large_graph=1)}
    check_forwards(f"tiled graph route forced ({name})", meta, parts, engs, device)


def case_forward_n70(lib, device):
    """The tiled route where it is the only one: the arch sweep's base architecture at N = 70, graph-only, random weights at the
    sweep's scales.  The off-node mask is one 64-bit word up to N = 64; here holes lie on both sides of index 64."""
    case = sw.GRAPH_70[0]
    assert case.N == 70 and case.name == "base@70"
    meta, parts = case.source()

    def both_sides(flags):
        off = flags[:3] == 0            # (the full sample has no hole; the two partial ones carry them)
        assert off[:, :64].any() and off[:, 64:].any() and flags[1:3, 64:].any(), "no holes on both sides of index 64"

    eng = expect(engine(meta, parts, lib, device), case.name, large_graph=1)
    check_forwards("tiled graph route (N = 70)", meta, parts, {"default": eng}, device, scale=case.scale, random_weights=True,
                   flag_check=both_sides)


def case_forward_word_edge_graph(N, lib, device, arch="gdss_community_small"):
    """The node sweep's builder (perturbed weights of a graph-only checkpoint) at the edges of the 64-bit off-node word: N = 33, and
    N = 64 with node 63 off in one sample and on in another."""
    meta, parts = lc.resized(arch, N, seed=N)

    def last_node(flags):
        assert (flags[:, N - 1] == 0).any() and (flags[:, N - 1] == 1).any()

    # community_small's networks leave k_xa for the tiled route behind N = 49 (node_sweep_cases.LAST_XA)
    eng = expect(engine(meta, parts, lib, device), f"{arch}@{N}", large_graph=int(N > 49), r2_family=0, xa_variant=0)
    check_forwards(f"{arch}@{N}", meta, parts, {"default": eng}, device, random_weights=True, flag_check=last_node)


def case_forward_word_edge_complex(N, lib, device):
    """... and a complex plan: the grid_small_CC architecture at N (cc.grid_at), x and adj."""
    meta, parts = cc.grid_at(N)
    meta = {k: v for k, v in meta.items() if k != "params_rank2"}       # (the rank-2 score at E K = 3 10^6 is not what the case is about)
    parts = {p: parts[p] for p in ("x", "adj")}
    eng = expect(engine(meta, parts, lib, device), f"grid_small_CC@{N}", large_graph=0, xa_variant=0)      # (k_xa serves it to N = 42)
    check_forwards(f"grid_small_CC@{N}", meta, parts, {"default": eng}, device, random_weights=True)


# ---- b. step calls with host-supplied noise against the oracle's updates on the same tensors
STEP_PLANS = {
    "ccsd_qm9_CC": ("Reverse", "Langevin", 0.2, 0.7),
    "ccsd_community_small_CC": ("Euler", "Langevin", 0.05, 0.7),
    "gdss_community_small": ("Euler", "Langevin", 0.05, 0.7),
    "ccsd_enzymes_small_CC": ("S4", "None", 0.15, 0.7),
}
EPS = 1e-4


def check_update(got, want, masks, what):
    """Entries of live nodes within the tolerance; entries of switched-off nodes too: every update kernel writes there what the
    reference's update carries (its score and its noise are masked, so pa * in for a predictor, the input for a corrector)."""
    for p, g, w, m in zip(NAMES, got, want, masks):
        g = g.detach().cpu()
        pc.assert_close(g * m, w * m, f"{what} {p}, live entries")
        pc.assert_close(g * (1 - m), w * (1 - m), f"{what} {p}, entries of switched-off nodes")


def oracle_s4_step(tgs, sdes, fns, snr, seps, state, flags, vec_t, dt, src):
    """One step of O.S4_solver's loop body (oracle/ccsd_oracle.py) on a state of the caller's: the solver masks its prior, which an
    unmasked class must not be.  Returns (state, means)."""
    B = flags.shape[0]
    state = list(state)
    vec_dt = torch.ones(B) * (dt / 2)
    scores = [fn(*state, flags, vec_t) for fn in fns]
    sdrift = [-sd.sde(v, vec_t)[1][:, None, None] ** 2 * sc for sd, v, sc in zip(sdes, state, scores)]
    timestep = (vec_t * (sdes[0].N - 1) / sdes[0].T).long()
    for k, (tg, sd) in enumerate(zip(tgs, sdes)):
        z = tg.noise(state[k], flags, src)
        gn = torch.norm(scores[k].reshape(B, -1), dim=-1)
        zn = torch.norm(z.reshape(B, -1), dim=-1)
        alpha = sd.alphas[timestep] if sd.kind == "VP" else torch.ones_like(vec_t)
        step = (snr * zn.mean() / gn.mean()) ** 2 * 2 * alpha
        state[k] = state[k] + step[:, None, None] * scores[k] + torch.sqrt(step * 2)[:, None, None] * z * seps
    trans = [sd.transition(v, vec_t, vec_dt) for sd, v in zip(sdes, state)]
    for k, tg in enumerate(tgs):
        state[k] = trans[k][0] + trans[k][1][:, None, None] * tg.noise(state[k], flags, src)
    for k in range(len(state)):
        state[k] = state[k] + sdrift[k] * dt
    trans = [sd.transition(v, vec_t + vec_dt, vec_dt) for sd, v in zip(sdes, state)]
    means = [t[0] for t in trans]
    for k, tg in enumerate(tgs):
        state[k] = trans[k][0] + trans[k][1][:, None, None] * tg.noise(state[k], flags, src)
    return state, means


def case_step_calls(name, cls, lib, device, step=0, seed=23):
    """ccsd_predictor, ccsd_corrector_norms + ccsd_corrector_apply (Langevin plans) or ccsd_corrector_norms + ccsd_s4_apply (S4) at
    one step, each on the class's state itself with raw host draws, against euler_update / reverse_update / langevin_update (S4:
    oracle_s4_step) fed the same tensors; the six norm sums each to the tolerance of its own magnitude."""
    predictor, corrector, snr, seps = STEP_PLANS[name]
    meta, parts = load_ckpt_np(name)
    cfg, is_cc = meta["config"], meta["is_cc"]
    names = NAMES[: 3 if is_cc else 2]
    nt = len(names)
    N, F, d_min, d_max = dims(meta)
    eng = engine(meta, parts, lib, device, sdes=[loader.load_sde(cfg["sde"][p]) for p in names], predictor=predictor, corrector=corrector,
                 snr=snr, scale_eps=seps, n_steps=1, eps=EPS)
    flags, state = class_inputs(cls, meta, seed)
    state = list(state[:nt])
    B = flags.shape[0]
    masks = live_masks(meta, flags)
    osd = [O.load_sde(cfg["sde"][p]) for p in names]
    tgs = [O._Target("x"), O._Target("adj")] + ([O._Target("rank2", N, d_min, d_max)] if is_cc else [])
    nets = pc._oracle_nets(meta, parts, is_cc, names)
    fns = [O.make_score_fn(s, n) for s, n in zip(osd, nets)]
    vec_t = torch.ones(B) * torch.linspace(osd[1].T, EPS, osd[1].N)[step]
    g = torch.Generator().manual_seed(seed + 1)
    draw = lambda: [torch.randn(t.shape, generator=g) for t in state]
    dv = lambda ts: [t.to(device) for t in ts] + [None] * (3 - nt)
    dstate, dflags = dv(state), flags.to(device)
    what = f"{name} class {cls} step {step}"

    def check_sums(got, want):
        got = got.cpu()
        for i in [k for k in range(6) if k % 3 < nt]:
            pc.assert_close(got[i:i + 1], torch.tensor([want[i]]), f"{what}: norm sum {i}")

    def raw_sums(z):
        """ccsd_corrector_norms' six sums: sum_b ||net_p[b]|| of the RAW network outputs (the score's scaling enters the step size
        apart), sum_b ||z_p[b]|| of the masked draws."""
        args = state + ([] if is_cc else [None])
        net = [torch.norm(O.run_network(meta[f"params_{p}"], parts[p], *args, flags).reshape(B, -1), dim=-1).sum().item() for p in names]
        zn = [torch.norm(tg.noise(v, flags, O.RecordedNoise([zk])).reshape(B, -1), dim=-1).sum().item() for tg, v, zk in zip(tgs, state, z)]
        pad = [0.0] * (3 - nt)
        return net + pad + zn + pad

    with torch.no_grad():
        if predictor == "S4":
            z = [draw() for _ in range(3)]
            want_sums = raw_sums(z[0])
            want, want_mean = oracle_s4_step(tgs, osd, fns, snr, seps, state, flags, vec_t, -1.0 / osd[1].N,
                                             O.RecordedNoise([t for zz in z for t in zz]))
            if CLASSES[cls][1] == "masked" and step == 0:       # on a masked state the restated step is S4_solver's own first step, bit for bit
                kw = dict(shape_x=(B, N, F), shape_adj=(B, N, N), snr=snr, scale_eps=seps, continuous=True, eps=EPS, is_cc=is_cc, keep_traj=False,
                          n_diff_steps=1, prior=state, final=[], noise=O.RecordedNoise([t for zz in z for t in zz]))
                if is_cc:
                    kw.update(sde_rank2=osd[2], shape_rank2=tuple(state[2].shape), d_min=d_min, d_max=d_max)
                res = O.S4_solver(osd[0], osd[1], **kw)(*nets, flags)
                assert all(torch.equal(a, b) for a, b in zip(res[:nt], want_mean)) and all(torch.equal(a, b) for a, b in zip(kw["final"], want))
            sums = torch.zeros(8, device=device)
            out, mean = eng.alloc_state(B), eng.alloc_state(B)
            eng.corrector_norms(step, 0, dstate, dstate, dflags, dv(z[0]), 0, 0, sums)
            check_sums(sums, want_sums)
            eng.s4_apply(step, dstate, dflags, dv(z[0]), dv(z[1]), dv(z[2]), 0, 0, sums, out, mean)
            check_update(out[:nt], want, masks, f"{what} ccsd_s4_apply out")
            check_update(mean[:nt], want_mean, masks, f"{what} ccsd_s4_apply mean")
            return
        # predictor
        z = draw()
        pred = O.reverse_update if predictor == "Reverse" else O.euler_update
        res = [pred(tg, sd, fn, False, state, flags, vec_t, O.RecordedNoise([zk])) for tg, sd, fn, zk in zip(tgs, osd, fns, z)]
        out, mean = eng.alloc_state(B), eng.alloc_state(B)
        eng.predictor(step, dstate, dflags, dv(z), 0, 0, out, mean)
        check_update(out[:nt], [r[0] for r in res], masks, f"{what} ccsd_predictor out")
        check_update(mean[:nt], [r[1] for r in res], masks, f"{what} ccsd_predictor mean")
        # Langevin corrector
        z = draw()
        res = [O.langevin_update(tg, sd, fn, snr, seps, 1, state, flags, vec_t, O.RecordedNoise([zk]))
               for tg, sd, fn, zk in zip(tgs, osd, fns, z)]
        want_sums = raw_sums(z)
        sums = torch.zeros(8, device=device)
        out = eng.alloc_state(B)
        eng.corrector_norms(step, 0, dstate, dstate, dflags, dv(z), 0, 0, sums)
        check_sums(sums, want_sums)
        eng.corrector_apply(step, 0, dstate, dflags, dv(z), 0, 0, sums, out)
        check_update(out[:nt], [r[0] for r in res], masks, f"{what} ccsd_corrector_apply out")


# ---- c. the production loop with holed flags
# form -> (checkpoint, predictor, corrector, snr, scale_eps, steps, what the plan must answer)
LOOPS = {
    "fused_merged_folded": ("ccsd_qm9_CC", "Reverse", "Langevin", 0.2, 0.7, 3, dict(loop_form=2, merged_r2=1, fold_sums=1)),
    "tiled_fuse": ("ccsd_community_small_CC", "Euler", "Langevin", 0.05, 0.7, 2, dict(loop_form=2, tiled_fuse=1)),
    "s4": ("ccsd_enzymes_small_CC", "S4", "None", 0.15, 0.7, 2, dict(loop_form=3)),
    "predictor_only": ("ccsd_qm9_CC", "Euler", "None", 0.0, 0.0, 3, dict(loop_form=0)),
    "graph_only": ("gdss_community_small", "Euler", "Langevin", 0.05, 0.7, 2, dict(r2_family=0)),
}


def case_production_loop(form, lib, device, seed=71):
    """ccsd_sampler_run (in-kernel Philox noise) under flags with holes against the oracle on the exported draws: its prior is masked
    by the same flags, so the loop's masked-state precondition holds."""
    name, predictor, corrector, snr, seps, steps, route = LOOPS[form]
    N = dims(load_ckpt_np(name)[0])[0]
    counts = counts_of(N)
    flags = make_flags_holes(len(counts), N, counts, seed)
    pc.case_production_loop_vs_oracle(name, lib, device, len(counts), counts, steps, predictor, corrector, snr, seps, seed=seed,
                                      expect_route=route, flags=flags)


def case_one_step_holes(name, lib, device, predictor, corrector, snr, seps, seed=73):
    """One full PC step of the Python-driven step-wise loop, host-supplied noise, under flags with holes."""
    N = dims(load_ckpt_np(name)[0])[0]
    counts = counts_of(N)
    pc.case_one_step_vs_oracle_large(name, lib, device, len(counts), counts, predictor, corrector, snr, seps, seed=seed,
                                     flags=make_flags_holes(len(counts), N, counts, seed))


def case_full_kernels_b256(lib, device, B=256, seed=79):
    """Device only.  community_small_CC at B = 256, the smallest batch at which the plan selects the one-workgroup-per-complex kernels
    k_gemm_h_full / k_hp_full, under flags with holes: the default plan against the plans with each of them switched off, bit for bit,
    with the plan queries saying that each side ran what it should."""
    N = 20
    counts = [20, 18, 11, 0, 1, 2, 16, 14, 12, 20]
    flags = make_flags_holes(B, N, counts, seed)
    pc.case_env_switches_bitwise(lib, device, [{"CCSD_NO_HP_FULL": "1"}, {"CCSD_NO_H_FULL": "1"}], B=B, flags=flags,
                                 expect=[dict(h_full=1, hp_full=1), dict(h_full=1, hp_full=0), dict(h_full=0, hp_full=0)])


# ---- d. the noise stream under holed flags
NOISE_SLOTS = {"qm9_CC": [None, (0, 0), (0, 1)],               # prior and predictor draw: the column map; corrector draw: the flat map
               "zinc250k_CC_5b": [(0, 1)],                       # a k_ew1 plan's predictor draw: the flat map at E K = 5.9 10^6
               "gdss_community_small": [None, (0, 0)]}
NOISE_MAPS = {"qm9_CC": {False, True}, "zinc250k_CC_5b": {True}, "gdss_community_small": set()}      # rank-2 group maps a plan's slots must cover


def case_noise(plan, lib, device, bound, seed=1, sample_offset=7):
    """ccsd_init_state and ccsd_noise_draws under flags with holes against tests/philox_ref.py masked in numpy (noise_cases.check_draws:
    switched-off entries exactly 0, adj bit-symmetric, live values within `bound`)."""
    eng, _ = nc.engine_for(plan, lib, device)
    flags = make_flags_holes(nc.B, eng.N, nc.counts_for(eng.N), 83)
    maps = set()
    for hs in NOISE_SLOTS[plan]:
        nc.case_stream(plan, lib, device, seed, sample_offset, hs, bound, flags=flags)
        if eng.is_cc:
            maps.add(False if hs is None else nc.is_flat(plan, hs[1]))
    assert maps == NOISE_MAPS[plan], f"{plan}: rank-2 group maps covered {maps}"


# ---- e. the off-node word of a complex at its last bit
def case_complex_masks(N, d, lib, device, seed=89):
    """A complex plan whose node count fills the 64-bit off-node word (N = 64; d = (d_min, d_max)), holed flags with node N - 1 off in
    one sample and on in others.  Only complex plans build the word (k_flagbits) and the byte tables (k_masktab), so a graph-only plan
    at N = 64 reads neither.  The plan is the zinc250k_CC substitute's ScoreNetworkF alone (cnum = 1, affine: k_ew1, which reads the
    byte tables); the x and adj networks and an oracle of 8.4 10^7 rank-2 entries per sample are not what the word is about.  Checked,
    every tensor generated and compared on the device:
      ccsd_score(rank2) on an unmasked state (class HU)   zero exactly where flags_left * flags_right is (k_masktab's tables);
      ccsd_init_state, ccsd_noise_draws (0, 0)            x, adj, rank2 zero exactly where the masks are -- the column map and the
                                                          flat map of the rank-2 draw (edge_on / cell_on on the word itself).
    A live entry may be 0.0 by chance (a draw whose cosine is 0: at most 2^-22 of them), so live entries are held to: every live
    row and every live column has a non-zero entry, and at most 1e-5 of the live entries are zero -- a mask that drops one node
    zeroes whole rows, at least 1 / E of the live entries.  Where E K is small (the emulation's twin) the score also meets the oracle."""
    meta, parts, _ = pc.zinc5b_at(N, *d)
    meta = {k: v for k, v in meta.items() if k not in ("params_x", "params_adj")}
    parts = {"rank2": parts["rank2"]}
    _, F, d_min, d_max = dims(meta)
    eng = expect(engine(meta, parts, lib, device, predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1),
                 f"zinc250k_CC_5b ScoreNetworkF@{N}", r2_family=2, ew1=1)
    counts = counts_of(N)
    B = len(counts)
    flags = make_flags_holes(B, N, counts, seed)
    assert (flags[:, N - 1] == 0).any() and (flags[1:3, N - 1] == 1).any()
    fl, fr = (t.to(device).bool() for t in O.rank2_flags(flags, N, d_min, d_max))
    live = {"x": flags.to(device).bool()[:, :, None].expand(B, N, F),
            "adj": (flags[:, :, None] * flags[:, None, :] * (1 - torch.eye(N))).to(device).bool(),
            "rank2": fl[:, :, None] & fr[:, None, :]}
    dflags = flags.to(device)

    def check(t, p, what):
        m = live[p]
        assert torch.isfinite(t).all(), f"{what} {p}: not finite"
        assert torch.where(m, torch.zeros_like(t), t).count_nonzero().item() == 0, f"{what} {p}: entries of switched-off nodes are not 0"
        nz = (t != 0) & m
        assert torch.equal(nz.any(dim=2), m.any(dim=2)) and torch.equal(nz.any(dim=1), m.any(dim=1)), f"{what} {p}: a live row or column is all 0"
        assert (m.sum() - nz.sum()).item() <= 1e-5 * m.sum().item(), f"{what} {p}: zeros among the live entries"

    E, K = O.get_rank2_dim(N, d_min, d_max)
    gen = torch.Generator(device=device).manual_seed(seed)
    rank2 = torch.randn(B, E, K, device=device, generator=gen)
    x, adj = torch.zeros(B, N, F, device=device), torch.zeros(B, N, N, device=device)
    out = eng.score(2, x, adj, rank2, dflags)
    check(out, "rank2", f"ScoreNetworkF@{N} score")
    if E * K <= 1 << 20:
        with torch.no_grad():
            want = O.run_network(meta["params_rank2"], parts["rank2"], x.cpu(), adj.cpu(), rank2.cpu(), flags)
        pc.assert_close(out, want, f"ScoreNetworkF@{N} net_rank2, class HU")
    del out, rank2
    st = eng.alloc_state(B)
    for what, call in (("prior", lambda: eng.init_state(dflags, st, None, seed, 7)),
                       ("draws (0, 0)", lambda: eng.noise_draws(dflags, 0, 0, st, seed, 7))):
        for t in st:
            t.fill_(float("nan"))
        call()
        for p, t in zip(NAMES, st):
            check(t, p, f"ScoreNetworkF@{N} {what}")
        assert torch.equal(st[1], st[1].transpose(1, 2)), f"{what}: adj is not symmetric"
