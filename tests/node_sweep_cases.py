"""Cases of the node-count sweep: the graph-network kernel k_xa, the tiled route that takes over from it, and the small rank-2
geometries at every node count up to 64 -- between the shipped checkpoints' geometries, where k_xa's LDS layout, its channel-group
size, the geometry-only instances and the rank-2 family change from one N to the next.  Shared by the CPU suite (host emulation,
a bounded list: tests/test_node_sweep.py) and the GPU suite (the full sweep: tests/test_gpu_node_sweep.py).  Every comparison
takes parity_cases.assert_close at its default tolerance."""
from ccsd_amd.engine import PCEngine
from tests import cc_large_graph_cases as cc
from tests import large_graph_cases as lc
from tests import parity_cases as pc
from tests.helpers import load_ckpt_np, make_flags

# ---- A. graph-only architectures at every node count 2..64
# architecture -> the last node count k_xa has an LDS layout for (from the next one on the plan takes the tiled route)
LAST_XA = {"gdss_community_small": 49, "gdss_zinc250k": 57, "gdss_qm9": 57, "gdss_ego_small": 54}
ARCHS = list(LAST_XA)
NODES = range(2, 65)
HINTS = (0, 8)                      # ccsd_config_t.batch_hint: a bare engine's, and a solver's at B = 8 (the largest LDS budget)
BANDS = {"2-16": range(2, 17), "17-32": range(17, 33), "33-48": range(33, 49), "49-64": range(49, 65)}
BAND_PARAMS = [(a, b, h) for a in ARCHS for b in BANDS for h in HINTS]
# node counts of the bounded (emulated) sweep: around the 16-row tile edges, each architecture's last k_xa N and first route N, 64
TILE_EDGES = (2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49)
# geometry-only k_xa instance (xa_variant) -> (N it is compiled for, the shipped architecture of that N)
GEO_INSTANCE = {4: (9, "gdss_qm9"), 5: (20, "gdss_community_small"), 6: (38, "gdss_zinc250k")}
ROUTE_QUERIES = ("large_graph", "xa_variant", "xa_lds_bytes")

RAN = {}                            # (architecture, N, hint) -> (large_graph, xa_variant, xa_lds_bytes) of the plans that ran
_oracle = {}                        # (architecture, N) -> the oracle's outputs, kept from the first hint to the last


def bounded_nodes(arch):
    return sorted(set(TILE_EDGES) | {LAST_XA[arch], LAST_XA[arch] + 1, 64})


def counts_of(N):
    return [N, N // 2 + 1, 1, 0]


def case_band(arch, nodes, hint, lib, device):
    """lc.case_forward_vs_oracle_src (x and adj forwards at scale 1.0 and 0.3, the 0.25-scaled score, the adj score's masks) for
    perturbed weights of `arch` at every N of `nodes`, four graphs of N, N // 2 + 1, 1 and 0 nodes, on the route the planner
    chooses; records the plan's route in RAN."""
    for N in nodes:
        meta, parts = lc.resized(arch, N, seed=N)
        keep = _oracle.setdefault((arch, N), {})
        RAN[(arch, N, hint)] = lc.case_forward_vs_oracle_src(meta, parts, lib, device, counts_of(N), f"{arch}@{N} hint {hint}",
                                                             expect_lg=None, batch_hint=hint, oracle=keep)
        if hint == HINTS[-1]:
            del _oracle[(arch, N)]


def plan_table(arch, lib, device):
    """{(N, hint): (large_graph, xa_variant, xa_lds_bytes)} for N = 2..64 and both hints: plans without weights, the planner alone."""
    meta, _ = load_ckpt_np(arch)
    F = meta["params_x"]["max_feat_num"]
    table = {}
    for N in NODES:
        pa = dict(meta["params_adj"], max_node_num=N)
        for hint in HINTS:
            eng = PCEngine(meta["params_x"], None, pa, None, None, None, N=N, F=F, is_cc=False, d_min=0, d_max=0, device=device,
                              lib=lib, batch_hint=hint)
            table[(N, hint)] = tuple(eng.query(q) for q in ROUTE_QUERIES)
    return table


def format_table(arch, table):
    """One line per node count: the route at hint 0 and at hint 8 (`*`: a plan that ran in this session)."""
    lines = [f"{arch}: N | large_graph xa_variant xa_lds_bytes at batch_hint 0 | at batch_hint 8   (* = ran)"]
    for N in NODES:
        cells = ["%d %2d %6d%s" % (*table[(N, h)], "*" if (arch, N, h) in RAN else " ") for h in HINTS]
        lines.append(f"  {N:2d} | " + " | ".join(cells))
    return "\n".join(lines)


def case_coverage(arch, lib, device, bands=None):
    """What the sweep was written for, asserted on the planner's table of `arch` (every plan that ran must be in it as it ran):
    the ceiling of k_xa, both routes below 65 nodes, a k_xa plan at N >= 49, a batch hint that changes the LDS layout, and the
    geometry-only instances 5 and 6 under an architecture they were not written for.  `bands`: the node counts the suite's band
    tests run (default: every band) -- together they must hold every N the assertions name.  Returns the table, formatted."""
    table = plan_table(arch, lib, device)
    for (a, N, h), route in RAN.items():
        if a == arch:
            assert table[(N, h)] == route, f"{arch}@{N} hint {h}: ran {route}, the weightless plan says {table[(N, h)]}"
    swept = set().union(*(bands if bands is not None else BANDS.values()))
    last = LAST_XA[arch]
    for h in HINTS:
        lg = {N: table[(N, h)][0] for N in NODES}
        assert max(N for N in NODES if lg[N] == 0) == last, f"{arch} hint {h}: the last k_xa node count moved"
        assert all(lg[N] == (N > last) for N in NODES), f"{arch} hint {h}: the routes interleave"
        assert all((table[(N, h)][2] > 0) == (N <= last) for N in NODES)
    assert last >= 49 and {last, last + 1} <= swept, f"{arch}: no k_xa plan at N >= 49, or the crossover is not swept"
    differ = [N for N in NODES if table[(N, 0)][2] != table[(N, 8)][2]]
    assert differ and set(differ) & swept, f"{arch}: batch_hint 8 never changes xa_lds_bytes"
    for var, (N, shipped) in GEO_INSTANCE.items():
        if var != 4 and arch != shipped:     # (variant 4 has F = 4 compiled in: case_variant4_other_architectures)
            assert table[(N, 0)][1] == var and N in swept, f"{arch}@{N}: xa_variant {table[(N, 0)][1]}, expected the instance {var}"
    return format_table(arch, table)


def feat_cut(meta, parts, F):
    """A graph-only checkpoint with its node features cut to the first F: the weights whose shape depends on max_feat_num
    (ScoreNetworkX's first layer and final MLP, of F + depth * nhid inputs and twice as many hidden units; the first attention
    layer's q / k / v) cut to their leading rows and columns -- a same-architecture network with arbitrary weights."""
    px = meta["params_x"]
    fin0, fin = px["max_feat_num"] + px["depth"] * px["nhid"], F + px["depth"] * px["nhid"]
    cut = {px["max_feat_num"]: F, fin0: fin, 2 * fin0: 2 * fin}
    assert len(cut) == 3 and px["nhid"] not in cut
    meta = dict(meta, params_x=dict(px, max_feat_num=F), params_adj=dict(meta["params_adj"], max_feat_num=F))
    meta["config"] = dict(meta["config"], data=dict(meta["config"]["data"], max_feat_num=F))
    out = {"x": {}, "adj": {}}
    for k, v in parts["x"].items():
        v = v.detach()
        if k == "layers.0.weight":
            v = v[:F]
        elif k.startswith("final."):
            v = v[tuple(slice(0, cut.get(s, s)) for s in v.shape)]
        out["x"][k] = v.clone().requires_grad_(True)
    for k, v in parts["adj"].items():
        v = v.detach()
        if k.startswith("layers.0.attn.") and k.endswith(".weight"):
            v = v[:F]
        out["adj"][k] = v.clone().requires_grad_(True)
    return meta, out


VARIANT4_ARCHS = ("gdss_community_small", "gdss_ego_small")


def case_variant4_other_architectures(lib, device):
    """xa_variant 4 (k_xa<false, XA_PLAIN9>: N = 9, F = 4, ldn = 16 compiled in) under architectures other than gdss_qm9's: it is
    selected by geometry alone, but its geometry includes the feature count, and of the four swept architectures only gdss_qm9
    has four features.  So: community_small's and ego_small's networks with their features cut to four (feat_cut), at N = 9, both
    hints -- three and two GCN layers 32 wide and five attention layers in an instance that had run with two 16 wide and three."""
    for arch in VARIANT4_ARCHS:
        meta, parts = feat_cut(*lc.resized(arch, 9, seed=9), 4)
        keep = {}
        for hint in HINTS:
            route = lc.case_forward_vs_oracle_src(meta, parts, lib, device, counts_of(9), f"{arch} (4 features)@9 hint {hint}",
                                                  expect_lg=0, batch_hint=hint, oracle=keep)
            assert route[1] == 4, f"{arch} with 4 features at N = 9, hint {hint}: xa_variant {route[1]}, expected the N = 9 instance"


# ---- B. the grid_small_CC architecture (d_min = d_max = 3) on k_xa and the small rank-2 geometries
CC_FUSED_LAST = 11                  # fused k_r2 serves to N = 11 (E = 55, K = 165); the tiled family (r2_family 3) from N = 12
CC_FORWARD_NODES = range(3, 25)     # x, adj and rank2: E = 3, 6, 10, 15, 21, 28, ... one row either side of the 16-row tiles
CC_XA_NODES = (31, 32, 33, 38, 41, 42)      # x and adj only: the 152 KB layouts, the variant-6 instance under a CC plan, the last k_xa N
CC_LOOP_NODES = range(3, 14)
CC_LOOPS = {"reverse_langevin": ("Reverse", "Langevin", 0.1, 0.7, 1), "euler_none": ("Euler", "None", 0.0, 0.0, 2)}
CC_R2_LDS = {3: 1476, 11: 59188}


def case_cc_forwards(N, lib, device, targets=("x", "adj", "rank2")):
    """cc.grid_at(N), four complexes of N, N // 2 + 1, 2 and 0 nodes: the forwards in `targets` against the oracle, the adj score's
    masks, and the plan's route: k_xa (with the geometry-only instance at N = 20 and 38), fused k_r2 to N = 11, the tiled rank-2
    family from N = 12."""
    meta, parts = cc.grid_at(N)
    _, F, d_min, d_max = cc.dims(meta)
    eng = cc.engine(meta, parts, lib, device)
    what = f"grid_small_CC@{N}"
    assert eng.query("large_graph") == 0 and eng.query("xa_lds_bytes") > 0, f"{what}: not a k_xa plan"
    assert eng.query("xa_variant") == {20: 5, 38: 6}.get(N, 0), f"{what}: xa_variant {eng.query('xa_variant')}"
    fused = N <= CC_FUSED_LAST
    assert eng.query("fused_r2") == int(fused) and eng.query("r2_family") == (1 if fused else 3), \
        f"{what}: fused_r2 {eng.query('fused_r2')}, r2_family {eng.query('r2_family')}: the k_r2 / tiled crossover moved"
    assert (eng.query("r2_lds_bytes") > 0) == fused
    if N in CC_R2_LDS:
        assert eng.query("r2_lds_bytes") == CC_R2_LDS[N]
    counts = [N, N // 2 + 1, 2, 0]
    flags = make_flags(len(counts), N, counts)
    state = pc.masked_state(N, len(counts), N, F, True, d_min, d_max, flags)
    want = cc.oracle_forwards(meta, parts, state, flags, targets)
    args = [t.to(device) for t in state] + [flags.to(device)]
    for p in targets:
        got = eng.score(cc.NAMES.index(p), *args)
        pc.assert_close(got, want[p], f"{what} net_{p}")
        if p == "adj":
            cc.check_adj_masks(got, flags, what)


def case_cc_loop(N, loop, lib, device):
    """The production loop of cc.grid_at(N) against the oracle on the exported draws, B = 3 with node counts [N, 2, N]: one step of
    Reverse + Langevin, or two of Euler without a corrector (the mean one corrector-free step returns holds no draw, so a single
    step cannot tell the draw slots apart, which case_production_loop_vs_oracle checks)."""
    predictor, corrector, snr, seps, steps = CC_LOOPS[loop]
    pc.case_production_loop_vs_oracle(f"grid_small_CC@{N}", lib, device, 3, [N, 2, N], steps, predictor, corrector, snr, seps,
                                      source=cc.grid_at(N), expect_route={"large_graph": 0, "fused_r2": int(N <= CC_FUSED_LAST)})


# ---- C. the zinc250k_CC substitute's architecture at d = 3..4: fused k_r2, then the element-wise family k_ew1
# N -> (ew1, ew1_fuse): K = 5, 15, 35, 70, 126, 210, 495 on k_r2; K = 715 and 1001 (odd: the rank-2 side cannot ride on the projection
# GEMM) and K = 1820 and 2380 (even) on k_ew1
ZINC5B_ROUTE = {4: (0, 0), 5: (0, 0), 6: (0, 0), 7: (0, 0), 8: (0, 0), 9: (0, 0), 11: (0, 0),
                12: (1, 0), 13: (1, 0), 15: (1, 1), 16: (1, 1)}
assert {f for e, f in ZINC5B_ROUTE.values() if e} == {0, 1}, "both values of ew1_fuse must occur on k_ew1: extend the list"


def case_zinc5b_loop(N, lib, device):
    """pc.zinc5b_at(N, 3, 4) at the fixture's own sampler, one step, B = 3 with node counts [N, 2, N], through the production loop
    against the oracle; the plan's rank-2 route is pinned per N."""
    meta, parts, sm = pc.zinc5b_at(N, 3, 4)
    ew1, fuse = ZINC5B_ROUTE[N]
    pc.case_production_loop_vs_oracle(f"zinc250k_CC_5b@{N} d=3..4", lib, device, 3, [N, 2, N], 1, sm["predictor"], sm["corrector"],
                                      sm["snr"], sm["scale_eps"], seed=29, source=(meta, parts),
                                      expect_route={"large_graph": 0, "fused_r2": 1 - ew1, "ew1": ew1, "ew1_fuse": fuse})


# ---- D. the production loop where k_xa is least tested: the last k_xa node counts (gcn_tile<4> / GTM(4) inside k_xa) and two
# layouts between the shipped geometries; the solver's batch_hint = 4 takes the largest LDS budget
XA_LOOP_SHAPES = [("gdss_community_small", 49), ("gdss_ego_small", 54), ("gdss_zinc250k", 57), ("gdss_qm9", 10), ("gdss_community_small", 25)]
XA_LOOP_SHAPES_BOUNDED = [("gdss_community_small", 25), ("gdss_qm9", 10)]
XA_LOOPS = {"euler_langevin": ("Euler", "Langevin", 0.05, 0.7), "s4_none": ("S4", "None", 0.15, 0.7)}


def case_xa_loop(arch, N, loop, lib, device):
    """Two steps of the production loop, B = 4 with node counts [N, N // 2 + 1, 1, 0], perturbed weights of `arch` at N, on k_xa."""
    predictor, corrector, snr, seps = XA_LOOPS[loop]
    assert N <= LAST_XA[arch]
    pc.case_production_loop_vs_oracle(f"{arch}@{N}", lib, device, 4, counts_of(N), 2, predictor, corrector, snr, seps,
                                      source=lc.resized(arch, N, seed=N), expect_route={"large_graph": 0})
