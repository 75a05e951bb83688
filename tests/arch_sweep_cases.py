"""Cases of the architecture sweep: the network hyper-parameters across the planner's width edges, where ccsd_plan.h picks another
code path -- the edge MLP of an AttentionLayer chained (16 wide) or block-wise, the chain shapes of ScoreNetworkX's and
ScoreNetworkA's final MLPs, the per-layer packing (mcs, cp, dsplit, nchunk), the geometry-only k_xa instance of N = 9 under
architectures it was not written for, and ScoreNetworkF's widths 9..32 on the fused k_r2 and on the tiled family.  Shared by the CPU
suite (host emulation: tests/test_arch_sweep.py) and the GPU suite (tests/test_gpu_arch_sweep.py).  Weights are seeded random
tensors of the shapes ccsd_amd.plan.state_dict_shapes names; every comparison takes parity_cases.assert_close at its default
tolerance against oracle.run_network on the same state dict; the plan query "mlp_forms" proves which MLP form ran.

Two readings of the sweep's list that the code fixes: (1) `nhid` of the one-change cases (6, 12, 20, 48, 64, and 8 at depth 8) is
the model's nhid, ScoreNetworkX's and ScoreNetworkA's alike, as a YAML file sets it; the ScoreNetworkX final-MLP edges change
ScoreNetworkX's nhid alone (10, 14, 22: an AttentionLayer's first attention dimension is nhid, and four heads do not divide 14 or
22).  (2) ScoreNetworkF "widths w" are nhid = c_hid = w and the widest c_final that keeps the final MLP's c_hid + c_final + cnum
inputs within 32 (F_WIDTHS)."""
import json
import math

import pytest
import torch

from ccsd_amd.engine import PCEngine
from ccsd_amd.plan import attn_layer_dims, fnet_layer_dims, gmh_layer_dims, state_dict_shapes
from oracle import ccsd_oracle as O
from tests import cc_large_graph_cases as cc
from tests import large_graph_cases as lc
from tests import parity_cases as pc
from tests.helpers import load_golden, make_flags

SDE = dict(type="VE", beta_min=0.1, beta_max=1.0, num_scales=1000)
BASE_X = dict(model_type="ScoreNetworkX", depth=2, nhid=16)
BASE_A = dict(model_type="ScoreNetworkA", nhid=16, num_layers=3, num_linears=2, c_init=2, c_hid=8, c_final=4, adim=16, num_heads=4,
              conv="GCN")
BASE_F = dict(model_type="ScoreNetworkF", num_layers_mlp=1, num_layers=2, num_linears=2, nhid=4, c_hid=4, c_final=2, cnum=2,
              use_hodge_mask=True)
# kat_gmh_models' "small" (ScoreNetworkX_GMH), "mlpconv_x" and "mlpconv_a" parameters: (params, N)
GMH_SMALL = (dict(model_type="ScoreNetworkX_GMH", max_feat_num=10, depth=2, nhid=4, num_linears=2, c_init=2, c_hid=3, c_final=2, adim=4,
                  num_heads=2, conv="GCN"), 5)
MLPCONV_X = (dict(model_type="ScoreNetworkX_GMH", max_feat_num=6, depth=2, nhid=8, num_linears=2, c_init=2, c_hid=4, c_final=3, adim=8,
                  num_heads=4, conv="MLP"), 9)
MLPCONV_A = (dict(model_type="ScoreNetworkA", max_feat_num=6, max_node_num=9, nhid=8, num_layers=3, num_linears=2, c_init=2, c_hid=4,
                  c_final=3, adim=8, num_heads=4, conv="MLP"), 9)
# ScoreNetworkF "widths w": (nhid, c_hid, c_final)
F_WIDTHS = {12: (12, 12, 12), 16: (16, 16, 14), 17: (17, 17, 13), 31: (31, 27, 3)}
QUERIES = ("mlp_forms", "large_graph", "xa_variant", "r2_family")

# seeds chosen so that both conditions on the inputs hold (case_conditions); every other case takes its place in its list
SEEDS = {"heads8": 702, "afin49": 702, "afin56": 700, "afin57": 700, "afin70": 703, "nhid48": 700, "f_tiled_w16": 700, "f_tiled_w12_n20": 701, "f_nhid32": 702}

RAN = {}            # case name -> {query: value} of the plans that ran
_oracle = {}        # case name -> the oracle's outputs, computed once and shared by every test of the case
_sources = {}       # case name -> (meta, weights)


def counts_of(N, is_cc=False):
    return [N, N // 2 + 1, 2 if is_cc else 1, 0]


def make_weights(params, seed, gain=1.0, bias=0.2):
    """A state dict for arbitrary `params`: glorot-uniform weights times `gain`, N(0, bias^2) biases, from a generator of its own."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in state_dict_shapes(params):
        if k.endswith("bias"):
            t = bias * torch.randn(shape, generator=g)
        else:
            t = (2 * torch.rand(shape, generator=g) - 1) * gain * math.sqrt(6.0 / (shape[-2] + shape[-1]))
        sd[k] = t.requires_grad_(True)
    return sd


class Case:
    """One architecture at one geometry.  `about`: the layer whose width the case is about, as unit specs (units_of)."""

    def __init__(self, name, about, N, F, px=None, pa=None, pf=None, d=(0, 0), seed=0, gain=1.0, scale=1.0, env=None):
        self.name, self.about, self.N, self.F, self.d, self.seed, self.gain, self.scale = name, about, N, F, d, seed, gain, scale
        self.is_cc = pf is not None
        self.env = env or {}
        geo = dict(max_node_num=N, d_min=d[0], d_max=d[1], is_cc=True) if self.is_cc else {}
        self.params = {}
        if px is not None:
            self.params["x"] = dict(px, max_feat_num=F, is_cc=self.is_cc)
        if pa is not None:
            self.params["adj"] = dict(dict(pa, **(geo if pa["model_type"] != "ScoreNetworkA" else {})), max_feat_num=F, max_node_num=N,
                                      is_cc=self.is_cc)
        if pf is not None:
            self.params["rank2"] = dict(pf, **geo)

    def at(self, N, scale=None, gain=None):
        """The same architecture at another node count (no weight shape of a graph-only network depends on N)."""
        assert not self.is_cc
        strip = lambda p: None if p is None else {k: v for k, v in p.items() if k not in ("max_feat_num", "max_node_num", "is_cc")}
        return Case(f"{self.name}@{N}", self.about, N, self.F, strip(self.params.get("x")), strip(self.params.get("adj")),
                    seed=self.seed, gain=gain or self.gain, scale=scale or self.scale)

    def source(self):
        """(meta in the checkpoint layout, {part: state dict})"""
        if self.name not in _sources:
            data = dict(max_node_num=self.N, max_feat_num=self.F)
            if self.is_cc:
                data.update(d_min=self.d[0], d_max=self.d[1])
            meta = {"is_cc": self.is_cc, "name": self.name, "config": {"data": data, "sde": {p: dict(SDE) for p in self.params}}}
            parts = {}
            for i, (p, prm) in enumerate(self.params.items()):
                meta[f"params_{p}"] = prm
                parts[p] = make_weights(prm, 7919 * self.seed + i, self.gain)
            _sources[self.name] = (meta, parts)
        return _sources[self.name]

    def engine(self, lib, device, weights=True, monkeypatch=None, **kw):
        meta, parts = self.source()
        slots = []
        for p in ("x", "adj", "rank2"):
            slots += [self.params.get(p), parts[p] if weights and p in parts else None]
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)
        try:
            return PCEngine(*slots, N=self.N, F=self.F, is_cc=self.is_cc, d_min=self.d[0], d_max=self.d[1], device=device, lib=lib, **kw)
        finally:
            for k in self.env:
                monkeypatch.delenv(k)

    def inputs(self, tag="unit"):
        counts = counts_of(self.N, self.is_cc)
        flags = make_flags(len(counts), self.N, counts)
        scale = self.scale * {"unit": 1.0, "small": 0.3}[tag]
        return pc.masked_state(11, len(counts), self.N, self.F, self.is_cc, *self.d, flags, scale), flags

    def oracle(self, tag, part, weights=None):
        """The oracle's output of network `part` on inputs(tag): computed once per case and kept (`weights`: another state dict,
        not kept)."""
        key = (tag, part)
        keep = _oracle.setdefault(self.name, {})
        if weights is None and key in keep:
            return keep[key]
        state, flags = self.inputs(tag)
        with torch.no_grad():
            out = O.run_network(self.params[part], weights or self.source()[1][part], *state, flags)
        if weights is None:
            keep[key] = out
        return out

    def tags(self):
        return ("unit", "small") if not self.is_cc and len(self.params) == 2 else ("unit",)


# ---- the unit of a layer: what condition (b) zeroes.  A spec is a tuple; units_of turns it into (part, [(key, dim, index)]).
def _mlp_unit(prefix):
    return [(prefix + "linears.0.weight", 0, -1), (prefix + "linears.0.bias", 0, -1), (prefix + "linears.1.weight", 1, -1)]


def units_of(case, spec):
    kind, args = spec[0], spec[1:]
    pa, px, pf = case.params.get("adj"), case.params.get("x"), case.params.get("rank2")
    if kind == "edge":          # hidden unit of AttentionLayer l's edge MLP (ScoreNetworkA)
        return "adj", _mlp_unit(f"layers.{args[0]}.mlp.")
    if kind == "xedge":         # ... of ScoreNetworkX_GMH's
        return "x", _mlp_unit(f"layers.{args[0]}.mlp.")
    if kind == "edge_lin":      # single-Linear edge MLP: the last output channel of the last layer's, and its column of the final MLP
        L = pa["num_layers"]
        return "adj", [(f"layers.{L - 1}.mlp.linear.weight", 0, -1), (f"layers.{L - 1}.mlp.linear.bias", 0, -1), ("final.linears.0.weight", 1, -1)]
    if kind in ("attn", "xattn"):   # the last attention dimension of layer l: the last column of Q and of K, every input channel
        part, prm = ("adj", pa) if kind == "attn" else ("x", px)
        l = args[0]
        cin = (attn_layer_dims(prm) if kind == "attn" else gmh_layer_dims(prm))[l][0]
        ops = []
        for c in range(cin):
            for g in "qk":
                pre = f"layers.{l}.attn.{c}.gnn_{g}."
                if prm.get("conv", "GCN") == "MLP":
                    ops += [(pre + "linears.1.weight", 0, -1), (pre + "linears.1.bias", 0, -1)]
                else:
                    ops += [(pre + "weight", 1, -1), (pre + "bias", 0, -1)]
        return part, ops
    if kind == "gcn":           # the last unit of ScoreNetworkX's GCN layer l: its column, the next layer's row, the final MLP's column
        l, depth, nhid = args[0], px["depth"], px["nhid"]
        ops = [(f"layers.{l}.weight", 1, -1), (f"layers.{l}.bias", 0, -1), ("final.linears.0.weight", 1, case.F + (l + 1) * nhid - 1)]
        if l + 1 < depth:
            ops.append((f"layers.{l + 1}.weight", 0, -1))
        return "x", ops
    if kind in ("mc", "xmc"):   # the last node feature AttentionLayer l hands on (multi_channel's last output), and its rows in layer l + 1
        part, prm = ("adj", pa) if kind == "mc" else ("x", px)
        l = args[0]
        dims = attn_layer_dims(prm) if kind == "mc" else gmh_layer_dims(prm)
        ops = [(f"layers.{l}.multi_channel.linears.1.weight", 0, -1), (f"layers.{l}.multi_channel.linears.1.bias", 0, -1)]
        assert l + 1 < len(dims)
        for c in range(dims[l + 1][0]):
            for g in "qkv":
                pre = f"layers.{l + 1}.attn.{c}.gnn_{g}."
                if prm.get("conv", "GCN") == "MLP" and g != "v":       # (an MLP's Linear is [out][in], a GCN weight [in][out])
                    ops.append((pre + "linears.0.weight", 1, -1))
                else:
                    ops.append((pre + "weight", 0, -1))
        if kind == "xmc":
            ops.append(("final.linears.0.weight", 1, case.F + (l + 1) * prm["nhid"] - 1))
        return part, ops
    if kind == "xfin":
        return "x", _mlp_unit("final.")
    if kind == "afin":
        return "adj", _mlp_unit("final.")
    if kind == "fhid":          # hidden unit of HodgeNetworkLayer l's MLP (ScoreNetworkF)
        return "rank2", _mlp_unit(f"layers.{args[0]}.layer.")
    if kind == "fchan":         # the last output channel of HodgeNetworkLayer l, its column in layer l + 1 and in the final MLP
        l, n, dims = args[0], pf["num_linears"], fnet_layer_dims(pf)
        last = f"layers.{l}.layer." + ("linear" if n == 1 else f"linears.{n - 1}")
        fin = "final." + ("linear" if pf["num_layers_mlp"] == 1 else "linears.0")
        ops = [(last + ".weight", 0, -1), (last + ".bias", 0, -1), (fin + ".weight", 1, pf["cnum"] + sum(d[1] for d in dims[:l + 1]) - 1)]
        if l + 1 < len(dims):
            ops.append((f"layers.{l + 1}.layer." + ("linear" if n == 1 else "linears.0") + ".weight", 1, -1))
        return "rank2", ops
    if kind == "ffin":
        return "rank2", _mlp_unit("final.")
    raise KeyError(kind)


def case_figures(case):
    """{what: figure} of the two conditions: max |oracle output| per compared tensor, and how far (in max|ref|) zeroing the last
    unit of each layer the case is about moves the output."""
    figures = {}
    for tag in case.tags():
        state, flags = case.inputs(tag)
        f64 = lambda t: None if t is None else t.double()
        for part in case.params:
            ref = case.oracle(tag, part)
            scale = ref.abs().max().item()
            figures[("max", tag, part)] = scale
            # the float32 oracle against its own evaluation in float64, as the share of assert_close's two allowances it uses up
            with torch.no_grad():
                exact = O.run_network(case.params[part], {k: v.detach().double() for k, v in case.source()[1][part].items()},
                                      *(f64(t) for t in state), flags.double())
            err = (ref.double() - exact).abs()
            big = exact.abs() > 1e-2 * scale
            figures[("oracle32", tag, part)] = max((err.max() / (pc.RTOL * scale)).item(),
                                                   (err / (pc.RTOL * exact.abs() + pc.ATOL_SCALE * scale))[big].max().item())
    for spec in case.about:
        part, ops = units_of(case, spec)
        w = {k: v.detach().clone() for k, v in case.source()[1][part].items()}
        for key, dim, idx in ops:
            assert w[key].select(dim, idx).abs().max() > 0, (case.name, key)
            w[key].select(dim, idx).zero_()
        w = {k: v.requires_grad_(True) for k, v in w.items()}
        ref = case.oracle("unit", part)
        figures[("moved", part) + tuple(spec)] = (case.oracle("unit", part, w) - ref).abs().max().item() / ref.abs().max().item()
    return figures


def case_conditions(case):
    """The two conditions on a case's inputs, on the oracle alone.  (a) max |oracle output| of every compared tensor lies in
    [1e-2, 1e2]: the scale-relative tolerance means what it says.  (b) with the last unit of the layer the case is about zeroed, the
    output moves by more than 1e-2 max|ref| -- 100 times what assert_close allows: a kernel that dropped or mis-indexed the last
    channel of the padded width would fail the comparison.  And one on the reference, which (a) presupposes: (c) the float32 oracle
    lies within a quarter of assert_close's allowances of its own float64 evaluation.  Random weights can make a network
    ill-conditioned in float32 -- one attention head at 70 nodes put the oracle 0.45 of the allowance from the float64 value, and a
    kernel as exact as the oracle then missed the oracle while both met the float64 value -- and a comparison against such a
    reference measures the reference.  Seeds (SEEDS) are chosen by these conditions alone, never by a kernel's result."""
    assert case.about, f"{case.name}: no layer named"
    for what, v in case_figures(case).items():
        if what[0] == "oracle32":
            assert v <= 0.25, f"{case.name}: the float32 oracle's net_{what[2]} on the {what[1]} inputs uses {v:.2f} of assert_close's allowance against float64"
        elif what[0] == "max":
            assert 1e-2 <= v <= 1e2, f"{case.name}: max |oracle net_{what[2]}| = {v:.3e} on the {what[1]} inputs, outside [1e-2, 1e2]"
        else:
            assert v > 1e-2, f"{case.name}: zeroing the last unit of {what[2:]} moves net_{what[1]} by {v:.3e} max|ref|, not more than 1e-2"


# ---- A. graph-only architectures: the base, one thing changed at a time
def graph(name, about, N=9, F=4, x=None, a=None, both=None, **kw):
    return Case(name, about, N, F, dict(BASE_X, **(both or {}), **(x or {})), dict(BASE_A, **(both or {}), **(a or {})), **kw)


def _afin(fdim, L, c_final, c_init):
    assert 8 * (L - 1) + c_final + c_init == fdim
    return graph(f"afin{fdim}", [("afin",)], a=dict(num_layers=L, c_final=c_final, c_init=c_init), scale=0.5 if c_init > 4 else 1.0)


GRAPH = [
    graph("base", [("edge", 1)]),
    graph("chid9", [("edge", 1)], a=dict(c_hid=9)),
    graph("chid12", [("edge", 1)], a=dict(c_hid=12)),
    graph("chid16", [("edge", 1)], N=12, F=5, a=dict(c_hid=16, c_final=16)),
    graph("cinit1", [("edge", 0)], a=dict(c_init=1)),
    graph("cinit5", [("edge", 0)], a=dict(c_init=5), scale=0.5),
    graph("cinit9", [("edge", 0)], a=dict(c_init=9), scale=0.4),
    graph("heads1", [("attn", 1)], a=dict(num_heads=1)),
    graph("heads3", [("attn", 1)], a=dict(num_heads=3, adim=12), both=dict(nhid=12)),
    graph("heads8", [("attn", 1)], a=dict(num_heads=8)),
    graph("adim8_nhid20", [("attn", 1), ("mc", 0)], a=dict(adim=8), both=dict(nhid=20)),
    graph("nhid6", [("gcn", 0), ("mc", 0)], both=dict(nhid=6)),
    graph("nhid48", [("gcn", 0), ("mc", 0)], both=dict(nhid=48), x=dict(depth=1)),
    graph("nhid64", [("gcn", 0), ("mc", 0)], F=3, both=dict(nhid=64)),
    graph("lin1", [("edge_lin",)], a=dict(num_linears=1)),
    graph("lin4", [("edge", 1)], a=dict(num_linears=4)),
    graph("layers1", [("edge", 0)], a=dict(num_layers=1, c_hid=4, c_final=4)),
    graph("layers8", [("edge", 7)], a=dict(num_layers=8, c_hid=4)),
    graph("depth1", [("gcn", 0)], x=dict(depth=1)),
    graph("depth8", [("gcn", 7)], x=dict(depth=8), both=dict(nhid=8)),
    graph("F1", [("xfin",)], F=1),
    graph("F17", [("xfin",)], F=17),
    graph("F40", [("xfin",)], F=40),
    # ScoreNetworkX's final MLP: F + depth * nhid inputs
    graph("xfin24", [("xfin",)], F=4, x=dict(nhid=10)),
    graph("xfin25", [("xfin",)], F=5, x=dict(nhid=10)),
    graph("xfin32", [("xfin",)], F=4, x=dict(nhid=14)),
    graph("xfin33", [("xfin",)], F=5, x=dict(nhid=14)),
    graph("xfin48", [("xfin",)], F=4, x=dict(nhid=22)),
    graph("xfin49", [("xfin",)], F=5, x=dict(nhid=22)),
    # ScoreNetworkA's final MLP: c_hid * (L - 1) + c_final + c_init inputs
    _afin(32, 4, 6, 2), _afin(33, 4, 7, 2), _afin(40, 5, 6, 2), _afin(41, 5, 7, 2), _afin(48, 6, 6, 2), _afin(49, 6, 7, 2),
    _afin(56, 7, 6, 2), _afin(57, 7, 7, 2), _afin(64, 8, 6, 2), _afin(65, 8, 7, 2), _afin(70, 8, 8, 6),
]
for _i, _c in enumerate(GRAPH):
    _c.seed = SEEDS.get(_c.name, 100 + _i)
GRAPH_BY_NAME = {c.name: c for c in GRAPH}
# the second geometries: k_xa's 152 KB layouts at N = 40 (xa_variant 0), and the tiled route at N = 70 wherever it accepts the plan
# at 70 nodes unit inputs and unit-gain weights put the float32 oracle up to ten times assert_close's allowance from its float64
# evaluation (condition (c) of case_conditions): inputs at 0.3 (0.12 under the fifth power of the adjacency) and weights at 0.8
SCALE_70, GAIN_70 = {"cinit5": 0.12}, 0.8
GRAPH_40 = [GRAPH_BY_NAME[n].at(40) for n in ("chid9", "heads1")]
# the plans the tiled route refuses at N = 70, with the planner's reason
ROUTE_REFUSES = {
    **{n: "edge MLPs wider than 16 features" for n in ("chid9", "chid12", "chid16", "cinit9")},
    **{n: "final MLPs of 57 to 64 input channels without hodge MLPs wider than 8" for n in ("afin57", "afin64")},
    **{n: "final MLPs wider than 64 input channels" for n in ("afin65", "afin70")},
}
GRAPH_70 = [c.at(70, SCALE_70.get(c.name, 0.3), GAIN_70) for c in GRAPH if c.name not in ROUTE_REFUSES]


def bands(cases, n=8):
    return {f"{cases[i].name}..{cases[min(i + n, len(cases)) - 1].name}": cases[i:i + n] for i in range(0, len(cases), n)}


GRAPH_BANDS = {**bands(GRAPH), **bands(GRAPH_40), **bands(GRAPH_70, 6)}
# the route cases of the bounded (emulated) sweep, 3 to 4 s each there: every form of the two final MLPs, the head counts, ragged nhid,
# one and four Linears, the deepest stacks
GRAPH_70_BOUNDED = [c for c in GRAPH_70 if c.name.split("@")[0] in ("heads1", "heads3", "nhid6", "nhid64", "lin1", "layers8", "depth8", "xfin24",
                                                                     "afin41", "afin56")]
GRAPH_BANDS_BOUNDED = {**bands(GRAPH), **bands(GRAPH_40), **bands(GRAPH_70_BOUNDED, 2)}


# what the planner must answer (CCSD_CHAIN_SHAPES: 16-feature tiles of input, hidden = 2 * input, output)
def x_fin_form(fdim):
    """ScoreNetworkX's final MLP (CCSD_CHAIN_XFIN): {2, 3, 1} to 24 inputs, {3, 6, 1} to 48, block-wise beyond."""
    return 2 if fdim <= 24 else 5 if fdim <= 48 else 0


def a_fin_form(fdim):
    """ScoreNetworkA's (CCSD_CHAIN_AFIN): {2, 4, 1} to 32 inputs, {3, 5, 1} to 40, {3, 6, 1} to 48, {4, 7, 1} to 56, block-wise beyond."""
    return 3 if fdim <= 32 else 4 if fdim <= 40 else 5 if fdim <= 48 else 6 if fdim <= 56 else 0


def record(case, eng):
    RAN[case.name] = {q: eng.query(q) for q in QUERIES}
    return RAN[case.name]


def forms(v):
    """mlp_forms -> (x_fin, a_fin, edge_mask)"""
    return v & 15, (v >> 4) & 15, v >> 8


def case_graph(case, lib, device):
    """lc.case_forward_vs_oracle_src (x and adj forwards at scale 1.0 and 0.3, the 0.25-scaled score, the adj score's masks) on the
    route the planner chooses; the plan's MLP forms are recorded, and pinned where the case is about them."""
    meta, parts = case.source()
    keep = _oracle.setdefault(case.name, {})
    route = lc.case_forward_vs_oracle_src(meta, parts, lib, device, counts_of(case.N), case.name, expect_lg=int(case.N > 64), oracle=keep,
                                          scales=(("unit", case.scale), ("small", 0.3 * case.scale)))
    got = record(case, case.engine(lib, device, weights=False))
    assert (got["large_graph"], got["xa_variant"]) == route[:2]
    x_fin, a_fin, edge = forms(got["mlp_forms"])
    px, pa = case.params["x"], case.params["adj"]
    L = pa["num_layers"]
    assert x_fin == x_fin_form(case.F + px["depth"] * px["nhid"]), (case.name, x_fin)
    assert a_fin == a_fin_form(pa["c_hid"] * (L - 1) + pa["c_final"] + pa["c_init"]), (case.name, a_fin)
    want = sum(1 << l for l, (cin, cout, *_) in enumerate(attn_layer_dims(pa)) if 2 * max(cin, cout) <= 16)
    assert edge == want, f"{case.name}: edge_mask {edge:#x}, expected {want:#x}"


def case_route_refuses(lib, device):
    """N = 70 has the tiled route alone: the plans it does not serve are refused with the planner's reason, the others plan."""
    for c in GRAPH:
        at = c.at(70)
        if c.name in ROUTE_REFUSES:
            with pytest.raises(NotImplementedError, match="N > 64 needs the tiled graph-network route, which does not serve " + ROUTE_REFUSES[c.name]):
                at.engine(lib, device, weights=False)
        else:
            assert at.engine(lib, device, weights=False).query("large_graph") == 1


# ---- B. ScoreNetworkX_GMH and conv = "MLP": one network per plan
def _single(name, about, base, part, **over):
    prm, N = base
    prm = dict(prm, **over)
    F = prm.pop("max_feat_num")
    prm.pop("max_node_num", None)
    return Case(name, about, N, F, **{"px" if part == "x" else "pa": prm})


SINGLE = [
    _single("gmh_chid9", [("xedge", 0)], GMH_SMALL, "x", c_hid=9),
    _single("gmh_heads1", [("xattn", 0)], GMH_SMALL, "x", num_heads=1),
    _single("gmh_nhid12", [("xmc", 0)], GMH_SMALL, "x", nhid=12),
    _single("gmh_lin4", [("xedge", 0)], GMH_SMALL, "x", num_linears=4),
    _single("mlpconv_chid9", [("edge", 1)], MLPCONV_A, "adj", c_hid=9),
    _single("mlpconv_heads1", [("xattn", 0)], MLPCONV_X, "x", num_heads=1),
    _single("mlpconv_nhid12", [("xmc", 0)], MLPCONV_X, "x", nhid=12),
    _single("mlpconv_lin4", [("edge", 1)], MLPCONV_A, "adj", num_linears=4),
]
for _i, _c in enumerate(SINGLE):
    _c.seed = 300 + _i


def case_single(case, lib, device, monkeypatch=None):
    """The forward of every network of the case (and the 0.25-scaled score) against the oracle, on the unit inputs."""
    eng = case.engine(lib, device, monkeypatch=monkeypatch)
    got = record(case, eng)
    state, flags = case.inputs()
    args = [None if t is None else t.to(device) for t in state] + [flags.to(device)]
    for p in case.params:
        t = cc.NAMES.index(p)
        want = case.oracle("unit", p)
        out = eng.score(t, *args)
        pc.assert_close(out, want, f"{case.name} net_{p}")
        pc.assert_close(eng.score(t, *args, 0.25), 0.25 * want, f"{case.name} 0.25 * net_{p}")
        if p == "adj":
            cc.check_adj_masks(out, flags, case.name)
    return got


# ---- C. ScoreNetworkF: fused k_r2 (widths up to 16), the tiled family beyond it or under CCSD_NO_FUSED_R2
TILED = {"CCSD_NO_FUSED_R2": "1"}


def fnet(name, about, N=6, d=(3, 4), widths=None, env=None, scale=0.5, **over):
    prm = dict(BASE_F, **over)
    if widths:
        prm.update(zip(("nhid", "c_hid", "c_final"), F_WIDTHS[widths]))
    return Case(name, about, N, 2, pf=prm, d=d, scale=scale, env=env)


FNET = [
    fnet("f_base", [("fhid", 0)]),
    fnet("f_nhid8", [("fhid", 0)], nhid=8), fnet("f_nhid9", [("fhid", 0)], nhid=9), fnet("f_nhid12", [("fhid", 1)], nhid=12),
    fnet("f_chid8", [("fchan", 0)], c_hid=8), fnet("f_chid9", [("fchan", 0)], c_hid=9), fnet("f_chid12", [("fchan", 0)], c_hid=12),
    fnet("f_cfin8", [("fchan", 1)], c_final=8), fnet("f_cfin9", [("fchan", 1)], c_final=9),
    fnet("f_layers4", [("fchan", 2)], num_layers=4),
    fnet("f_lin4", [("fhid", 1)], num_linears=4),
    fnet("f_mlp3", [("ffin",)], num_layers_mlp=3),
    fnet("f_cnum1_w12", [("fhid", 1), ("fchan", 0)], widths=12, cnum=1),
    fnet("f_nomask_w12", [("fhid", 1), ("fchan", 0)], widths=12, use_hodge_mask=False),
    fnet("f_tiled_w12", [("fhid", 1), ("fchan", 0)], widths=12, env=TILED),
    fnet("f_tiled_w16", [("fhid", 1), ("fchan", 0)], widths=16, env=TILED),
    fnet("f_tiled_w17", [("fhid", 1), ("fchan", 0)], widths=17),
    fnet("f_tiled_w12_n13", [("fhid", 1), ("fchan", 0)], N=13, d=(3, 3), widths=12),
]
# only on the GPU (5 to 7 s each on the emulation)
FNET_GPU = [
    fnet("f_tiled_w12_n20", [("fhid", 1), ("fchan", 0)], scale=0.25, N=20, d=(3, 3), widths=12),
    fnet("f_tiled_w31_n20", [("fhid", 1), ("fchan", 0)], scale=0.25, N=20, d=(3, 3), widths=31),
    fnet("f_tiled_w12_n16", [("fhid", 1), ("fchan", 0)], scale=0.25, N=16, d=(3, 4), widths=12),
]
for _i, _c in enumerate(FNET + FNET_GPU):
    _c.seed = SEEDS.get(_c.name, 400 + _i)
FNET_BANDS = bands(FNET + FNET_GPU, 7)


def f_width(case):
    """The widest Linear of the HodgeNetworkLayers."""
    pf = case.params["rank2"]
    return max(pf["nhid"] if pf["num_linears"] > 1 else 0, pf["c_hid"], pf["c_final"])


def f_family(case):
    """The rank-2 family the planner must choose: fused k_r2 (1) while every Linear of ScoreNetworkF, the final MLP's included, is at
    most 16 wide (CCSD_FW) and at most two Hodge powers enter; else, or under CCSD_NO_FUSED_R2, the tiled family (3)."""
    pf = case.params["rank2"]
    fdim = pf["c_hid"] * (pf["num_layers"] - 1) + pf["c_final"] + pf["cnum"]
    widest = max(f_width(case), fdim * (2 if pf["num_layers_mlp"] > 1 else 1))
    return 1 if widest <= 16 and pf["cnum"] <= 2 and not case.env and case.N <= 11 else 3


def case_fnet(case, lib, device, monkeypatch):
    got = case_single(case, lib, device, monkeypatch)
    assert got["r2_family"] == f_family(case), f"{case.name}: r2_family {got['r2_family']}"


# ---- D. one step of the production loop behind these MLP forms
def _loop_cc():
    pa = dict(model_type="ScoreNetworkA_CC", nhid=4, num_layers=2, num_linears=2, c_init=2, c_hid=2, c_final=2, adim=2, num_heads=2,
              conv="GCN", conv_hodge="HCN", nhid_h=2, num_layers_h=1, num_linears_h=1, c_hid_h=2, c_final_h=2, adim_h=2, num_heads_h=2)
    pf = dict(BASE_F, nhid=12, c_hid=8, c_final=4)         # (a final MLP of 14 inputs: the widest the fused k_r2 serves is 16)
    return Case("loop_f_w12", [], 6, 2, dict(BASE_X, depth=2, nhid=4), pa, pf, d=(3, 4), seed=500, scale=0.5)


LOOPS = {"chid9": GRAPH_BY_NAME["chid9"], "xfin49": GRAPH_BY_NAME["xfin49"], "afin57": GRAPH_BY_NAME["afin57"], "f_w12": _loop_cc()}
LOOP_FORMS = {"chid9": lambda v: forms(v)[2] == 0, "xfin49": lambda v: forms(v)[0] == 0, "afin57": lambda v: forms(v)[1] == 0,
              "f_w12": lambda v: True}


def case_loop(key, lib, device):
    """Reverse + Langevin, one step, B = 3 with node counts [N, 2, N], through ccsd_sampler_run against the oracle on the exported draws."""
    case = LOOPS[key]
    N = case.N
    eng = case.engine(lib, device, weights=False)
    assert LOOP_FORMS[key](eng.query("mlp_forms")), (key, eng.query("mlp_forms"))
    route = {"large_graph": 0}
    if case.is_cc:
        route.update(r2_family=1)
    pc.case_production_loop_vs_oracle(f"arch sweep {case.name}", lib, device, 3, [N, 2, N], 1, "Reverse", "Langevin", 0.1, 0.7,
                                      source=case.source(), expect_route=route)


# ---- E. coverage of the plans that ran
def case_coverage(names):
    """Asserted over RAN[name] for name in `names`: every form of the two final MLPs -- with the wide-hodge plan whose final MLP
    k_lg_fin_w runs (case_route_final_mlp), a form no graph-only plan reaches --, both kinds of edge mask, the N = 9 instance of k_xa
    under the architectures it had not run, and both rank-2 families above 8 wide."""
    missing = [n for n in names if n not in RAN]
    assert not missing, f"cases that did not run before the coverage test: {missing}"
    got = {n: RAN[n] for n in names}
    fm = {n: forms(r["mlp_forms"]) for n, r in got.items() if n in GRAPH_BY_NAME or "@" in n}
    assert {0, 2, 5} <= {f[0] for f in fm.values()}, "a form of ScoreNetworkX's final MLP did not run"
    a_fin = {f[1] for f in fm.values()}
    assert RAN_WIDE, "the wide-hodge plan did not run before the coverage test"
    a_fin.add(forms(RAN_WIDE["mlp_forms"])[1])
    assert {0, 3, 4, 5, 6, 7} <= a_fin, f"forms of ScoreNetworkA's final MLP that ran: {sorted(a_fin)}"
    full = lambda n: (1 << (GRAPH_BY_NAME[n.split('@')[0]].params["adj"]["num_layers"])) - 1
    assert any(f[2] == full(n) for n, f in fm.items()) and any(f[2] != full(n) for n, f in fm.items())
    assert any(f[2] == 0 for f in fm.values()), "no plan ran with every edge MLP un-chained"
    for n in ("chid9", "heads1", "depth8", "nhid48"):
        assert got[n]["xa_variant"] == 4 and got[n]["large_graph"] == 0, f"{n}: xa_variant {got[n]['xa_variant']}, expected the N = 9 instance"
    for n in ("chid9@40", "heads1@40"):
        assert got[n]["xa_variant"] == 0 and got[n]["large_graph"] == 0
    assert all(r["large_graph"] == int(n.endswith("@70")) for n, r in got.items())
    byname = {c.name: c for c in FNET + FNET_GPU}
    for family in (1, 3):
        assert any(got[n]["r2_family"] == family and f_width(byname[n]) > 8 for n in names if n in byname), \
            f"r2_family {family} did not run with a ScoreNetworkF width above 8"


RAN_WIDE = {}


def case_route_final_mlp(lib, device, monkeypatch):
    """A plan whose final MLP runs in k_lg_fin_w (the afin_lg shape, index 7): only wide-hodge plans have it.  hodge_wide_cases'
    enzymes_small_CC architecture with c_hid_h 8 at N = 12 (46 graph + 14 hodge channels); the adj forward against the oracle."""
    from tests import hodge_stack_route_cases as hs
    from tests import hodge_wide_cases as hw

    hw.forced(monkeypatch, False)
    meta, parts = hs.arch_at(hw.ENZ, 12, **hw.ENZ_WIDE)
    eng = cc.engine(meta, parts, lib, device)
    v = eng.query("mlp_forms")
    Nn, F, d_min, d_max = cc.dims(meta)
    counts = [12, 7, 2, 0]
    flags = make_flags(len(counts), Nn, counts)
    state = pc.masked_state(9, len(counts), Nn, F, True, d_min, d_max, flags)
    want = cc.oracle_forwards(meta, parts, state, flags, ["adj"])["adj"]
    got = eng.score(1, *(t.to(device) for t in state), flags.to(device))
    pc.assert_close(got, want, "enzymes_small_CC, c_hid_h 8, net_adj")
    cc.check_adj_masks(got, flags, "enzymes_small_CC, c_hid_h 8")
    assert eng.query("h_wide") == 1 and eng.query("large_graph") == 1
    RAN_WIDE["mlp_forms"] = v
    return v


# ---- F. the envelope of ccsd_build_plan: the last accepted value plans (and runs: its case is in the sweep), the first rejected one
# raises the planner's message, and the library still creates and runs a good plan after the rejection
def _f_over(**over):
    return fnet("rejected", [], **over)


ENVELOPE = {
    # limit -> (the case of the last accepted value, the first rejected architecture, exception, the planner's message)
    "num_linears 4|5": ("lin4", lambda: graph("r", [], a=dict(num_linears=5)), NotImplementedError, "MLP with more than 4"),
    "depth 8|9": ("depth8", lambda: graph("r", [], x=dict(depth=9), both=dict(nhid=8)), NotImplementedError, "x_depth out of range"),
    "num_layers 8|9": ("layers8", lambda: graph("r", [], a=dict(num_layers=9, c_hid=4)), NotImplementedError, "a_num_layers out of range"),
    "f_num_layers 4|5": ("f_layers4", lambda: _f_over(num_layers=5), NotImplementedError, "f_num_layers out of range"),
    "cnum 4|5": ("f_cnum4", lambda: _f_over(cnum=5), NotImplementedError, r"cnum in 1\.\.4"),
    "ScoreNetworkF layer 32|33": ("f_nhid32", lambda: _f_over(nhid=33), NotImplementedError, "ScoreNetworkF layer wider than 32"),
    "ScoreNetworkF final MLP 32|33": ("f_fin32", lambda: _f_over(c_hid=27, c_final=4), NotImplementedError, "ScoreNetworkF final MLP wider than 32"),
    "adim / heads": ("heads3", lambda: graph("r", [], a=dict(num_heads=3)), ValueError, "attn_dim not divisible into head chunks"),
    "num_layers 1, c_hid != c_final": ("layers1", lambda: graph("r", [], a=dict(num_layers=1, c_hid=8, c_final=4)), ValueError,
                                       "num_layers==1 needs c_hid==c_final"),
}
FNET_EDGE = [
    fnet("f_cnum4", [("fhid", 1)], scale=0.25, cnum=4),
    fnet("f_nhid32", [("fhid", 1)], nhid=32),
    fnet("f_fin32", [("fchan", 0)], c_hid=27, c_final=3),
]
for _i, _c in enumerate(FNET_EDGE):
    _c.seed = SEEDS.get(_c.name, 600 + _i)
ACCEPTED = {c.name: c for c in GRAPH + FNET + FNET_EDGE}


def case_envelope(limit, lib, device, monkeypatch, run=True):
    """`run`: one forward of the last accepted architecture against the oracle (the GPU suite; the CPU suite runs these cases in
    its own sweep and only plans them here)."""
    accepted, rejected, exc, message = ENVELOPE[limit]
    case = ACCEPTED[accepted]
    if run:
        (case_fnet if case.is_cc else case_single)(case, lib, device, monkeypatch)
    else:
        case.engine(lib, device, weights=False, monkeypatch=monkeypatch)
    with pytest.raises(exc, match=message):
        rejected().engine(lib, device, weights=False, monkeypatch=monkeypatch)
    # the library after the rejection: a good plan, created and run
    case_single(GRAPH_BY_NAME["base"], lib, device)


# ---- G. the reference's constructors at six of these architectures (tests/golden/kat_arch_sweep.npz, tools/make_golden.py)
KAT = {"chid12_cinit5": dict(c_hid=12, c_init=5), "heads1": dict(num_heads=1), "heads3": dict(num_heads=3, adim=12, nhid=12),
       "lin4": dict(num_linears=4), "layers1": dict(num_layers=1, c_hid=4, c_final=4), "f_w12_lin4": None}


def kat():
    g = load_golden("kat_arch_sweep.npz")
    return g, json.loads(str(g["meta"]))


def kat_tag(g, tag):
    sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]).requires_grad_(True) for k in g.files if k.startswith(f"{tag}/w/")}
    return sd, {k: torch.from_numpy(g[f"{tag}/{k}"]) for k in ("flags", "x", "adj", "rank2", "out") if f"{tag}/{k}" in g.files}


def case_kat_params():
    """The fixture's six architectures are the sweep's."""
    _, meta = kat()
    assert set(meta) == set(KAT)
    for tag, over in KAT.items():
        prm = meta[tag]
        if over is None:
            want = dict(BASE_F, num_linears=4)
            want.update(zip(("nhid", "c_hid", "c_final"), F_WIDTHS[12]))
            assert prm["max_node_num"] == 6 and (prm["d_min"], prm["d_max"]) == (3, 4)
        else:
            want = dict(BASE_A, **over)
            assert prm["max_node_num"] <= 9 and prm["max_feat_num"] == 4
        assert {k: prm[k] for k in want} == want, tag


def case_kat_engine(tag, lib, device):
    """The engine against the reference's output, directly."""
    g, meta = kat()
    prm = meta[tag]
    sd, t = kat_tag(g, tag)
    dv = lambda k: t[k].to(device) if k in t else None
    B = t["flags"].shape[0]
    assert B == 4
    if prm["model_type"] == "ScoreNetworkF":
        N = prm["max_node_num"]
        eng = PCEngine(None, None, None, None, prm, sd, N=N, F=2, is_cc=True, d_min=prm["d_min"], d_max=prm["d_max"], device=device, lib=lib)
        x, adj = torch.zeros(B, N, 2, device=device), torch.zeros(B, N, N, device=device)
        got = eng.score(2, x, adj, dv("rank2"), dv("flags"))
    else:
        eng = PCEngine(None, None, prm, sd, None, None, N=prm["max_node_num"], F=prm["max_feat_num"], is_cc=False, device=device, lib=lib)
        got = eng.score(1, dv("x"), dv("adj"), None, dv("flags"))
        cc.check_adj_masks(got, t["flags"], tag)
    pc.assert_close(got, t["out"], f"kat_arch_sweep {tag}")
