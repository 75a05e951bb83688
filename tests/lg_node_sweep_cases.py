"""Cases of the node-count sweep of the tiled graph-network route (k_lg_*, ccsd_amd/csrc/ccsd_k_lg.h) above 64 nodes, up to its
ceiling CCSD_LG_MAXN = 512: one node past and exactly at the multiples of the route's tile sizes (16, 32, 64), an even N whose N^2
is no multiple of 64, both sides of k_lg_sym's second grid-stride pass (N = 256 | 257 at c_hid = 8) and the ceiling with its
neighbour.  Shared by the CPU suite (host emulation, a bounded list: tests/test_lg_node_sweep.py) and the GPU suite (the full list:
tests/test_gpu_lg_node_sweep.py).

Reference and tolerance.  At these sizes the fp32 oracle's adjacency network is badly conditioned for most weights and inputs
(DESIGN.md section 3), so the expected value of every forward is the oracle run in float64 on the same inputs and the same weights
widened to double (reference()), and the bound is the float64 arbiter's rule: the product is at most max(RTOL, 1.5 e_ref) from it,
e_ref the fp32 oracle's own distance on that very case.  Every case must have e_ref <= E_REF_CAP = RTOL / 4 -- asserted, a cap on
the inputs and not a measurement: then the bound in force is RTOL itself, and a badly conditioned reference cannot hide an error.
parity_cases.assert_close's element-wise check runs against the float64 result at the same rtol."""
import torch

from oracle import ccsd_oracle as O
from tests import large_graph_cases as lc
from tests import parity_cases as pc
from tests import purity_cases as pu
from tests.helpers import load_ckpt_np, make_flags_holes

RTOL = pc.RTOL
E_REF_CAP = RTOL / 4
FACTOR = 1.5                        # case_fp64_arbiter's
MAXN = 512                          # CCSD_LG_MAXN (ccsd_plan.h)

# node counts of the device sweep; the emulation runs EMU_NODES (DESIGN.md section 3 states the measured times)
NODES = (65, 66, 80, 81, 95, 96, 127, 128, 129, 160, 192, 193, 255, 256, 257, 320, 384, 385, 448, 496, 497, 511, 512)
EMU_NODES = (65, 66, 96, 128, 129)
# groups of node counts per GPU test, by the work of their oracles (~ N^2 per network and precision)
GROUPS = {"65-81": (65, 66, 80, 81), "95-129": (95, 96, 127, 128, 129), "160-193": (160, 192, 193), "255-257": (255, 256, 257),
          "320": (320,), "384": (384,), "385": (385,), "448": (448,), "496": (496,), "497": (497,), "511": (511,), "512": (512,)}
assert tuple(n for g in GROUPS.values() for n in g) == NODES


# ---- families: the weights at N and the inputs of a forward
def masked(scale):
    """parity_cases.masked_state at `scale` (seed N)"""
    return lambda N, F, flags: pc.masked_state(N, flags.shape[0], N, F, False, 0, 0, flags, scale)[:2]


def graph_like(N, F, flags):
    """x = mask_x(randn); adj = a symmetric Bernoulli(4 / (N - 1)) 0/1 graph plus 0.1 randn, upper triangle mirrored, mask_adjs."""
    B = flags.shape[0]
    g = torch.Generator().manual_seed(1000 + N)
    x = O.mask_x(torch.randn(B, N, F, generator=g), flags)
    a = (torch.rand(B, N, N, generator=g) < 4.0 / (N - 1)).float() + 0.1 * torch.randn(B, N, N, generator=g)
    a = a.triu(1)
    return x, O.mask_adjs(a + a.transpose(-1, -2), flags)


# family -> (architecture, name of its 0.01 * N(0, 1) weight noise or None: the weights as shipped, inputs)
# Q: gdss_qm9's architecture (3 attention layers, adim 16, F = 4); C: gdss_community_small's (5 layers, adim 32, nhid 32, F = 10)
FAMILIES = {
    "Q shipped 1.0": ("gdss_qm9", None, masked(1.0)),
    "Q shipped 0.3": ("gdss_qm9", None, masked(0.3)),
    "Q noise 1.0": ("gdss_qm9", "Q noise", masked(1.0)),
    "Q noise 0.3": ("gdss_qm9", "Q noise", masked(0.3)),
    "C": ("gdss_community_small", "C", graph_like),
}
# Seed of the weight noise: N, except where the fp32 oracle of that network is more than E_REF_CAP / 2 from the float64 result on
# the sweep's inputs -- there the first of N + 1000, N + 2000, ... within E_REF_CAP / 2.  Found on the CPU from the two oracles
# alone, before any product run.  Half the cap, because the fp32 oracle's rounding depends on the host's BLAS threads: between two
# hosts e_ref of one case moved by a factor of up to two; the tests assert the cap itself.  DESIGN.md section 3 lists the e_ref of
# the seeds passed over.
WEIGHT_SEED = {("Q noise", 384): 1384, ("Q noise", 448): 1448, ("Q noise", 511): 3511, ("Q noise", 512): 1512,
               ("C", 80): 1080, ("C", 320): 1320, ("C", 385): 3385, ("C", 496): 3496, ("C", 511): 1511}


def source(family, N):
    arch, noise, _ = FAMILIES[family]
    return lc.resized(arch, N, seed=None if noise is None else WEIGHT_SEED.get((noise, N), N), noise=0.01)


def sweep_flags(N):
    """B = 6: N live nodes; N - 1 (the last row and column off); N // 2 + 1; 1; 0; and one sample of helpers.make_flags_holes with
    switched-off nodes on both sides of the last 64-node boundary below N (the sample whose last node is off)."""
    edge = 64 * ((N - 1) // 64)
    f = torch.zeros(6, N)
    for b, c in enumerate([N, N - 1, N // 2 + 1, 1, 0]):
        f[b, :c] = 1.0
    counts = [N, N - 3, N - 8, 0, 1, 2]
    for seed in range(N, N + 64):
        h = make_flags_holes(6, N, counts, seed)[2]               # the second fullest partial sample: node N - 1 off
        if (h[:edge] == 0).any() and (h[edge:] == 0).any() and h[:edge].any() and (N - edge < 2 or h[edge:].any()):
            break
    else:
        raise AssertionError(f"N = {N}: no holed sample with holes on both sides of node {edge}")
    assert h[N - 1] == 0 and h.sum() == N - 8
    f[5] = h
    return f


# ---- reference
_refs = {}                          # (family, N) -> (flags, x, adj, {p: (float64 result, e_ref)})
MEASURED = {}                       # (family, N, backend, p) -> (e_ref, product error): what the tests print


def _to64(w):
    return {k: v.detach().double() for k, v in w.items()}


def reference(family, N):
    """The inputs of (family, N) and, per network, the oracle's float64 result on them with e_ref, the fp32 oracle's distance from
    it relative to its scale.  Computed once per process, shared by every test of the case, never modified."""
    key = (family, N)
    if key not in _refs:
        meta, parts = source(family, N)
        flags = sweep_flags(N)
        x, adj = FAMILIES[family][2](N, meta["params_x"]["max_feat_num"], flags)
        res = {}
        for p in ("x", "adj"):
            with torch.no_grad():
                ref32 = O.run_network(meta[f"params_{p}"], parts[p], x, adj, None, flags)
                with pc.f64_arithmetic():
                    exact = O.run_network(meta[f"params_{p}"], _to64(parts[p]), x.double(), adj.double(), None, flags.double())
            assert exact.dtype == torch.float64
            scale = max(exact.abs().max().item(), 1e-6)
            res[p] = (exact, (ref32.double() - exact).abs().max().item() / scale)
        _refs[key] = (flags, x, adj, res)
    return _refs[key]


def check_conditioning(family, N):
    """e_ref <= RTOL / 4 on both forwards of (family, N): the cap on the inputs.  -> {p: e_ref}"""
    out = {}
    for p, (_, e_ref) in reference(family, N)[3].items():
        assert e_ref <= E_REF_CAP, (f"{family}@{N} net_{p}: the fp32 oracle is {e_ref:.2e} from the float64 result, above "
                                    f"RTOL / 4 = {E_REF_CAP:.1e}: replace the case (another seed, architecture or input family)")
        out[p] = e_ref
    return out


def check_against_f64(got, exact, e_ref, what, factor=1.0):
    """The arbiter's rule and assert_close's element-wise check, against `factor` * the float64 result.  -> the product's error"""
    exact = exact * factor
    g = got.detach().cpu().double()
    assert g.shape == exact.shape and torch.isfinite(g).all(), what
    scale = max(exact.abs().max().item(), 1e-6)
    e_mine = (g - exact).abs().max().item() / scale
    assert e_mine <= max(RTOL, FACTOR * e_ref), (f"{what}: the product is {e_mine:.2e} from the float64 result, the fp32 oracle "
                                                 f"{e_ref:.2e}")
    pc.assert_close(got, exact, what, RTOL)
    return e_mine


def check_adj_masks(got, flags, what):
    a = got.detach().cpu()
    fm = flags[:, :, None] * flags[:, None, :]
    assert torch.all(a[fm == 0] == 0) and torch.all(torch.diagonal(a, dim1=1, dim2=2) == 0), f"{what}: the adj score's masks"


def case_forward(family, N, lib, device, eng=None):
    """The x and adj forwards of (family, N) on the route the planner picks -- the raw network and the 0.25-scaled score -- against
    the float64 oracle; large_graph == 1; the adj score zero outside flags (x) flags and on the diagonal."""
    check_conditioning(family, N)
    flags, x, adj, res = reference(family, N)
    what = f"{family}@{N}"
    if eng is None:
        eng = lc.engine(*source(family, N), lib, device)
    assert eng.query("large_graph") == 1, f"{what}: not on the tiled route"
    dv = lambda t: t.to(device)
    for t, p in enumerate(("x", "adj")):
        exact, e_ref = res[p]
        got = eng.score(t, dv(x), dv(adj), None, dv(flags))
        e_mine = check_against_f64(got, exact, e_ref, f"{what} net_{p}")
        got2 = eng.score(t, dv(x), dv(adj), None, dv(flags), 0.25)
        e2 = check_against_f64(got2, exact, e_ref, f"{what} 0.25 * net_{p}", 0.25)
        MEASURED[(family, N, str(device), p)] = (e_ref, max(e_mine, e2))
        print(f"lg sweep {what} {device} net_{p}: e_ref {e_ref:.2e}, product {max(e_mine, e2):.2e}")
        if p == "adj":
            check_adj_masks(got, flags, what)
            check_adj_masks(got2, flags, f"{what} (scaled)")


def case_group(family, nodes, lib, device):
    for N in nodes:
        case_forward(family, N, lib, device)
        _refs.pop((family, N), None)          # (no other test reads it)


# ---- step calls and the library loop (family Q, the 0.01-noise weights)
LOOP_FAMILY = "Q noise 1.0"            # (a loop takes the weights alone)
LOOP_NODES = (128, 256, 512)
LOOP_EMU_NODES = (128,)
LOOPS = {"reverse_langevin": ("Reverse", "Langevin", 0.1, 0.7, 1), "s4_none": ("S4", "None", 0.15, 0.7, 2)}


def case_loop(N, loop, lib, device):
    """pc.case_production_loop_vs_oracle at N, B = 3 with node counts [N, N // 2 + 1, N - 1]: one step of Reverse + Langevin (the
    NORMS partials of k_lg_fin, ceil(N^2 / 64) per sample, reduced by k_lg_epi; the PRED epilogue), or two of S4 without a corrector."""
    predictor, corrector, snr, seps, steps = LOOPS[loop]
    pc.case_production_loop_vs_oracle(f"{LOOP_FAMILY}@{N}", lib, device, 3, [N, N // 2 + 1, N - 1], steps, predictor, corrector, snr,
                                      seps, source=source(LOOP_FAMILY, N), expect_route={"large_graph": 1})


# ---- the planner's edge, run and not just planned
def _up(n):
    return (n + 255) // 256 * 256


def lg_workspace_bytes(meta, B):
    """carve_ws (ccsd_api.h) of a graph-only plan on the tiled route without a multi-iteration corrector, restated in Python's
    integers: every piece rounded up to 256 bytes."""
    px, pa = meta["params_x"], meta["params_adj"]
    N, F = pa["max_node_num"], px["max_feat_num"]
    NN = N * N
    L, c_init, c_hid, c_final, nhid, adim = (pa[k] for k in ("num_layers", "c_init", "c_hid", "c_final", "nhid", "adim"))
    couts = [c_final if l == L - 1 else c_hid for l in range(L)]
    cins = [c_init] + couts[:-1]
    a_fdim = c_init + sum(couts)
    x_fdim = F + px["depth"] * px["nhid"]
    # Q | K | V side by side, padded to 16 columns; the first layer's attention dimension is nhid (plan_attn_layer)
    cp = max((2 * (nhid if l == 0 else adim) + nhid + 15) // 16 * 16 for l in range(L))
    cin = max(cins)
    fx = max(F, px["nhid"], nhid)
    E = N * (N - 1) // 2
    tiles = (NN + 63) // 64
    parts = [B * 8,                                                 # offbits; the pieces of complexes and hodge branches are empty
             B * N * F * 4, B * NN * 4, B * 16,                     # net_x, net_adj, norm2
             B * E * 2 * 4, B * E * 4, B * 2 * 4, 64,               # part, zpart, part2, sums
             B * a_fdim * NN * 4, B * cin * NN * 4, B * cin * N * 4, B * cin * N * cp * 4, B * cin * N * cp * 4,
             B * N * fx * 4, B * N * fx * 4, B * N * x_fdim * 4, B * N * px["nhid"] * 4, B * N * F * 4, B * tiles * 2 * 4]
    return sum(_up(n) for n in parts)


def case_planner_ceiling(lib, device):
    """ccsd_workspace_bytes(B) of the N = 512 plans for B = 1 and 6 against the carve restated in Python's integers (the channel stack
    alone is B * fdim * 2^20 bytes); N = 513 is still rejected with its message."""
    for family in ("Q noise 1.0", "C"):
        meta, parts = source(family, MAXN)
        eng = lc.engine(meta, parts, lib, device)
        assert eng.query("large_graph") == 1
        for B in (1, 6):
            want = lg_workspace_bytes(meta, B)
            got = pu.ws_bytes(eng, B)
            assert got == want, f"{family}@{MAXN} B = {B}: ccsd_workspace_bytes {got}, the carve {want}"
    import pytest
    with pytest.raises(NotImplementedError, match="N <= 512"):
        lc.engine(*lc.resized("gdss_qm9", MAXN + 1), lib, device)
    with pytest.raises(NotImplementedError, match="N <= 512"):
        lc.engine(*lc.resized("gdss_community_small", MAXN + 1), lib, device)


def case_guarded_ceiling(lib, device, family="Q noise 1.0"):
    """One N = 512 forward (x and adj) with the workspace at exactly ccsd_workspace_bytes(6) between two 0xA5 guards
    and the outputs between guards: the guarded run is the plan's first, so a store past the end is a failed assertion."""
    N = MAXN
    eng = lc.engine(*source(family, N), lib, device)
    n = pu.ws_bytes(eng, 6)
    big = pu.guarded_workspace(eng, n, None, device)
    with pu.guarded() as g:
        case_forward(family, N, lib, device, eng=eng)
        g.check(f"{family}@{N}")
    pu.check_workspace_guards(big, n, f"{family}@{N}")
