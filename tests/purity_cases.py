"""Cases that pin every call as a pure function of its arguments ("Purity of calls").  Shared by the host-emulation
suite (tests/test_purity.py) and the GPU suite (tests/test_gpu_purity.py, -m gpu); `lib` / `device` select the backend.

    1  the planned calls do not depend on what the workspace holds on entry and touch nothing outside it     case_workspace
    2  the same for the scratch buffers of the plan-free operations                                           case_op
    3  a sample does not depend on its batch: row order, batch size, position in the Philox stream          case_batch
    4  live plans do not disturb each other; the plan-owned off-bit buffer survives growing                   case_interleaved, case_growth,
                                                                                                              case_two_streams
    5  the launches and copies of a call that read a caller's tensor or the workspace are ordered on the       case_stream_unit, case_stream_op
       caller's stream (device only; what the construction cannot see is listed at on_side_stream)

Every comparison is torch.equal; the one tolerance is SUMS_BOUND (the six batch norm sums across batch sizes).  The workspace and
the scratch buffers are controlled by wrapping PCEngine._workspace / SampleOps._scratch on the instance under test; outputs are put
between guards by handing ccsd_amd.engine / ccsd_amd.samples a torch whose `empty` carves from a 0xA5-filled tensor (guarded): the
product's own code allocates, the test decides where."""
import contextlib
import ctypes as C
import json
import time

import numpy as np
import pytest
import torch

from ccsd_amd import engine as engine_mod
from ccsd_amd import loader
from ccsd_amd import samples as samples_mod
from tests import arch_sweep_cases as sw
from tests import eval_cases as ec
from tests import finish_cases as fc
from tests import hodge_wide_cases as hw
from tests import lift_cases as lc
from tests import parity_cases as pc
from tests import spectrum_cases as spc
from tests import state_class_cases as sc
from tests.helpers import load_ckpt_np, load_golden, make_flags, make_flags_holes, sample_ops

NAMES = sc.NAMES
GUARD = 4096                        # bytes on either side; a multiple of 256, so the slice between keeps the base's alignment
FILL = 0xA5
PAT32 = int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])
SEED, OFFSET = 5, 7                 # Philox seed and sample_offset of the units that draw in the kernel
PERM = [3, 0, 5, 1, 4, 2]
# The six batch norm sums across batch sizes: relative distance of the float32 sequential sum of the six per-row norms (taken from the
# B = 1 calls) to their float64 sum, the largest over every route and sum on the emulation (gdss_community_small forced tiled: 1.098e-7;
# the others 2.8e-8 .. 8.2e-8), and four times it: the allowance for any other order over six terms (the device adds them in a
# butterfly; five roundings of 2^-24 each bound every order by 3.0e-7).
SUMS_MEASURED = 1.10e-7
SUMS_BOUND = 4 * SUMS_MEASURED


# ---- guarded allocations ------------------------------------------------------------------------------------------------------------
class Guarded:
    """Allocations carved from the middle of 0xA5-filled tensors: GUARD bytes on either side lie inside the allocation, so a stray
    store shows as a failed assertion."""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype=torch.float32, device=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
        pad = -n % 8
        big = torch.full((n + pad + 2 * GUARD,), FILL, dtype=torch.uint8, device=device)
        self.items.append((big, n))
        return big[GUARD:GUARD + n].view(dtype).view(shape)

    def check(self, what):
        for big, n in self.items:
            ok = (big[:GUARD] == FILL).all() & (big[GUARD + n:] == FILL).all()
            assert ok.item(), f"{what}: a guard around an output of {n} bytes was written"


def assert_written(t, what):
    """No float32 / int32 element still holds the fill."""
    left = (t.contiguous().view(torch.int32) == PAT32).sum().item()
    assert left == 0, f"{what}: {left} of {t.numel()} output elements were not written"


class _Torch:
    """torch, with `empty` carving from a Guarded."""

    def __init__(self, g):
        self._g = g

    def __getattr__(self, k):
        return getattr(torch, k)

    def empty(self, *shape, dtype=torch.float32, device=None):
        return self._g.new(shape[0] if len(shape) == 1 else shape, dtype, device)


@contextlib.contextmanager
def guarded():
    """Inside the block every torch.empty of PCEngine and SampleOps (outputs, alloc_state) lies between guards."""
    g = Guarded()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine_mod, "torch", _Torch(g))
        mp.setattr(samples_mod, "torch", _Torch(g))
        yield g


def pin_workspace(eng, t):
    """`eng` passes the uint8 tensor `t`, whole and at its exact size, as the workspace of every call (the reduce hook looks for
    the sums in eng._ws)."""
    eng._ws = t
    eng._workspace = lambda B: (C.c_void_p(t.data_ptr()), t.numel())


def guarded_workspace(eng, n, fill, device):
    """Pins to `eng` a workspace of exactly `n` bytes, every byte `fill` (None: left at 0xA5), in the middle of a 0xA5 tensor -> that
    tensor.  Every condition runs between guards, so that a store past the end is a failed assertion on either backend."""
    big = filled(n + 2 * GUARD, FILL, device)
    if fill is not None:
        big[GUARD:GUARD + n] = fill
    pin_workspace(eng, big[GUARD:GUARD + n])
    return big


def check_workspace_guards(big, n, what):
    ok = (big[:GUARD] == FILL).all() & (big[GUARD + n:] == FILL).all()
    assert ok.item(), f"{what}: a guard around the workspace was written"


def ws_bytes(eng, B):
    return eng.lib.ccsd_workspace_bytes(eng.handle, B)


def filled(n, v, device):
    return torch.full((n,), v, dtype=torch.uint8, device=device)


# ---- routes -------------------------------------------------------------------------------------------------------------------------
class Route:
    """One plan: `source` () -> (meta, parts); step = (predictor, corrector, snr, scale_eps) or None (a single network: score
    only); env / unset: the plan switches; expect: what the plan must answer; kw: further PCEngine arguments."""

    def __init__(self, name, source, step=("Euler", "Langevin", 0.1, 0.7), env=None, unset=(), expect=None, kw=None, scale=1.0, B=6,
                 loop_steps=0):
        self.name, self.source, self.step, self.env, self.unset = name, source, step, env or {}, unset
        self.expect, self.kw, self.scale, self.B, self.loop_steps = expect or {}, kw or {}, scale, B, loop_steps

    def build(self, lib, device, **over):
        meta, parts = self.source()
        kw = {}
        if self.step is not None:
            names = NAMES[: 3 if meta["is_cc"] else 2]
            predictor, corrector, snr, seps = self.step
            kw.update(sdes=[loader.load_sde(meta["config"]["sde"][p]) for p in names], predictor=predictor, corrector=corrector, snr=snr,
                      scale_eps=seps, n_steps=1, eps=sc.EPS)
        kw.update(self.kw, **over)
        eng = sc.expect(sc.engine(meta, parts, lib, device, self.env, self.unset, **kw), self.name, **self.expect)
        eng.purity_predictor = kw.get("predictor")          # (apply() picks the update half by it)
        return eng


def _ckpt(name):
    return lambda: load_ckpt_np(name)


def _ew1():
    return pc.zinc5b_at(12, 3, 4)[:2]


def _kat_general(tag="G3_n5"):
    g = load_golden("kat_hodge_general.npz")
    params = json.loads(str(g["meta"]))[tag]
    return sc._kat_source(params, {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/w/")})


def _kat_wide(tag="W2_n9"):
    return sc._kat_source(*hw.kat_tag(tag)[:2])


def _n70():
    return sw.GRAPH_70[0].source()


_QM9 = dict(step=sc.STEP_PLANS["ccsd_qm9_CC"], kw=dict(batch_hint=1024))
ROUTES = {r.name: r for r in [
    Route("qm9_CC", _ckpt("ccsd_qm9_CC"), expect=dict(xa_variant=7, r2_instance=31102, fused_r2=1, large_graph=0), **_QM9),
    Route("qm9_CC no bake", _ckpt("ccsd_qm9_CC"), env={"CCSD_NO_BAKE": "1"}, expect=dict(xa_variant=4, r2_instance=31101), **_QM9),
    Route("qm9_CC no geo", _ckpt("ccsd_qm9_CC"), env={"CCSD_NO_GEO": "1"}, expect=dict(xa_variant=0, r2_instance=31100), **_QM9),
    Route("community_small_CC", _ckpt("ccsd_community_small_CC"), step=sc.STEP_PLANS["ccsd_community_small_CC"],
          expect=sc.CHECKPOINTS["ccsd_community_small_CC"]),
    Route("enzymes_small_CC", _ckpt("ccsd_enzymes_small_CC"), step=sc.STEP_PLANS["ccsd_enzymes_small_CC"],
          expect=sc.CHECKPOINTS["ccsd_enzymes_small_CC"]),
    Route("qm9_Base_CC", _ckpt("ccsd_qm9_Base_CC"), expect=sc.CHECKPOINTS["ccsd_qm9_Base_CC"]),
    Route("community_small_Base_CC", _ckpt("ccsd_community_small_Base_CC"), expect=sc.CHECKPOINTS["ccsd_community_small_Base_CC"]),
    Route("gdss_community_small", _ckpt("gdss_community_small"), step=sc.STEP_PLANS["gdss_community_small"],
          expect=sc.CHECKPOINTS["gdss_community_small"]),
    Route("gdss_zinc250k", _ckpt("gdss_zinc250k"), expect=sc.CHECKPOINTS["gdss_zinc250k"]),
    Route("zinc250k_CC_5b@12", _ew1, step=("Reverse", "Langevin", 0.2, 0.7), expect=dict(r2_family=2, large_graph=0)),
    Route("G3_n5", _kat_general, step=None, expect=dict(h_general=1)),
    Route("W2_n9", _kat_wide, step=None, unset=("CCSD_LARGE_GRAPH",), expect=dict(h_wide=1, large_graph=1, r2_family=3)),
    Route("gdss_community_small tiled", _ckpt("gdss_community_small"), step=sc.STEP_PLANS["gdss_community_small"],
          env={"CCSD_LARGE_GRAPH": sc.FORCED["gdss_community_small"]}, expect=dict(large_graph=1)),
    Route("qm9_CC tiled", _ckpt("ccsd_qm9_CC"), step=sc.STEP_PLANS["ccsd_qm9_CC"], env={"CCSD_LARGE_GRAPH": sc.FORCED["ccsd_qm9_CC"]},
          expect=dict(large_graph=1)),
    Route("qm9_Base_CC tiled", _ckpt("ccsd_qm9_Base_CC"), env={"CCSD_LARGE_GRAPH": sc.FORCED["ccsd_qm9_Base_CC"]}, expect=dict(large_graph=1)),
    Route("base@70", _n70, expect=dict(large_graph=1), scale=sw.GRAPH_70[0].scale),
]}
# device only: the one-workgroup-per-complex kernels k_gemm_h_full / k_hp_full, selected from B = 256
ROUTE_B256 = Route("community_small_CC B=256", _ckpt("ccsd_community_small_CC"), step=sc.STEP_PLANS["ccsd_community_small_CC"],
                   kw=dict(batch_hint=256), expect=dict(h_full=1, hp_full=1), B=256)
# the loop forms of state_class_cases.LOOPS, a Langevin plan with two inner iterations (the third state buffer lives in the workspace)
LOOP_ROUTES = {form: Route(f"loop {form}", _ckpt(name), step=(predictor, corrector, snr, seps), expect=route, loop_steps=steps)
               for form, (name, predictor, corrector, snr, seps, steps, route) in sc.LOOPS.items()}
LOOP_ROUTES["nsteps2"] = Route("loop nsteps2", _ckpt("ccsd_qm9_CC"), step=sc.STEP_PLANS["ccsd_qm9_CC"], kw=dict(n_steps=2), loop_steps=2)
STREAM_ROUTES = ["qm9_CC", "community_small_CC", "gdss_community_small tiled"]
_engines = {}


def engine_of(route, lib, device):
    """The route's plan, built once per backend and shared by the cases.  pin_workspace replaces a cached engine's _workspace for
    good, so a case never relies on what an earlier one pinned: each pins its own workspace before its first call."""
    key = (route.name, id(lib), str(device))
    if key not in _engines:
        _engines[key] = route.build(lib, device)
    return _engines[key]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
class Inputs:
    """Class "H" inputs of a route on the device: holed flags, the masked state, three sets of host draws."""

    def __init__(self, flags, state, z):
        self.flags, self.state, self.z = flags, state, z

    @property
    def B(self):
        return self.flags.shape[0]

    def tensors(self):
        return [self.flags] + [t for ts in [self.state] + self.z for t in ts if t is not None]

    def like(self, tensors):
        """The same structure around other tensors (the order of tensors())."""
        it = iter(tensors)
        flags = next(it)
        take = lambda ts: [None if t is None else next(it) for t in ts]
        return Inputs(flags, take(self.state), [take(z) for z in self.z])

    def rows(self, idx):
        i = torch.as_tensor(idx, device=self.flags.device)
        return self.like([t.index_select(0, i).contiguous() for t in self.tensors()])


def inputs_of(route, device, seed=5, extra=()):
    """B = 6 with 0, 1 and 2 live nodes next to a full sample (state_class_cases.counts_of); `extra`: further node counts."""
    meta, _ = route.source()
    N = sc.dims(meta)[0]
    if route.B == 6:
        counts = sc.counts_of(N) + list(extra)
        flags, state = sc.class_inputs("H", meta, seed, route.scale, counts)
    else:
        return _inputs_large(route, meta, device, seed, route.B + len(extra))
    g = torch.Generator().manual_seed(seed + 1)
    z = [[None if t is None else torch.randn(t.shape, generator=g) for t in state] for _ in range(3)]
    dv = lambda ts: [None if t is None else t.to(device) for t in ts]
    return Inputs(flags.to(device), dv(state), [dv(k) for k in z])


def _inputs_large(route, meta, device, seed, B):
    """The B = 256 route: the flags of state_class_cases.case_full_kernels_b256, the masked state and ONE set of draws generated on
    the device (a rank-2 tensor is 10^9 bytes)."""
    N, F, d_min, d_max = sc.dims(meta)
    flags = make_flags_holes(B, N, [20, 18, 11, 0, 1, 2, 16, 14, 12, 20], seed)
    fl, fr = (t.to(device) for t in sc.O.rank2_flags(flags, N, d_min, d_max))
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, device=device, generator=g)
    E, K = sc.O.get_rank2_dim(N, d_min, d_max)
    flags = flags.to(device)
    a = rnd(B, N, N).triu(1)
    state = [rnd(B, N, F) * flags[:, :, None], (a + a.transpose(1, 2)) * flags[:, :, None] * flags[:, None, :], rnd(B, E, K) * fl[:, :, None] * fr[:, None, :]]
    return Inputs(flags, state, [[rnd(B, N, F), rnd(B, N, N), rnd(B, E, K)], [None] * 3, [None] * 3])


def targets_of(route):
    meta, parts = route.source()
    return [k for k, p in enumerate(NAMES) if f"params_{p}" in meta and parts.get(p) is not None]


# ---- units: a call, or the pair of calls the header ties together through the workspace ----------------------------------------------
def step_of(eng):
    return 1 if eng.diff_steps > 1 else 0


def new_sums(eng):
    t = engine_mod.torch.empty(8, device=eng.device)          # (guarded inside guarded())
    return t.zero_()


def _named(prefix, ts):
    return {f"{prefix}.{p}": t for p, t in zip(NAMES, ts) if t is not None}


def u_score(target):
    return lambda eng, i: {f"net_{NAMES[target]}": eng.score(target, *i.state, i.flags)}


def u_predictor(host):
    def run(eng, i, offset=OFFSET):
        out, mean = eng.alloc_state(i.B), eng.alloc_state(i.B)
        eng.predictor(step_of(eng), i.state, i.flags, i.z[0] if host else None, SEED, offset, out, mean)
        return {**_named("out", out), **_named("mean", mean)}
    return run


def norms(eng, i, sums):
    eng.corrector_norms(step_of(eng), 0, i.state, i.state, i.flags, i.z[0], 0, 0, sums)


def apply(eng, i, sums):
    """The update half of the pair the plan's predictor calls for: ccsd_s4_apply or ccsd_corrector_apply."""
    out = eng.alloc_state(i.B)
    if eng.purity_predictor == "S4":
        mean = eng.alloc_state(i.B)
        eng.s4_apply(step_of(eng), i.state, i.flags, i.z[0], i.z[1], i.z[2], 0, 0, sums, out, mean)
        return {**_named("out", out), **_named("mean", mean)}
    eng.corrector_apply(step_of(eng), 0, i.state, i.flags, i.z[0], 0, 0, sums, out)
    return _named("out", out)


def u_pair(eng, i):
    sums = new_sums(eng)
    norms(eng, i, sums)
    res = apply(eng, i, sums)
    res["sums"] = sums
    return res


def u_loop(steps, hook=False):
    def run(eng, i):
        state, scratch, result = (eng.alloc_state(i.B) for _ in range(3))
        calls = []
        eng.init_state(i.flags, state, None, SEED, OFFSET)
        eng.run(i.flags, state, scratch, result, SEED, OFFSET, 0, steps, reduce=(lambda s: calls.append(s.numel())) if hook else None)
        if hook:
            assert calls and set(calls) == {6}, f"the reduce hook saw {calls}"
        return {**_named("state", state), **_named("result", result)}
    return run


def units_of(route, eng):
    """name -> unit of every call the route's plan serves."""
    if route.loop_steps:
        units = {"sampler_run": u_loop(route.loop_steps)}
        if route.step[1] == "Langevin" or route.step[0] == "S4":
            units["sampler_run_ex"] = u_loop(route.loop_steps, hook=True)
        return units
    units = {f"score {NAMES[t]}": u_score(t) for t in targets_of(route)}
    if route.step is None:
        return units
    if route.B != 6:                # (the large batch: the rank-2 score and the pair run k_gemm_h_full / k_hp_full)
        return {"score rank2": units["score rank2"], "norms+corrector_apply": u_pair}
    if route.step[0] != "S4":
        units["predictor host"] = u_predictor(True)
        units["predictor philox"] = u_predictor(False)
    units["norms+s4_apply" if route.step[0] == "S4" else "norms+corrector_apply"] = u_pair
    return units


def run_unit(eng, unit, i, what, check=True):
    """One unit with its outputs between guards -> {name: cpu tensor}; every output element written, every guard intact."""
    with guarded() as g:
        res = unit(eng, i)
        g.check(what)
        if check:
            for k, t in res.items():
                if k != "sums":
                    assert_written(t, f"{what} {k}")
        return {k: t.cpu().clone() for k, t in res.items()}


def assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs in bits ({(got[k] != want[k]).sum().item()} elements)"


# ---- 1. workspace independence ------------------------------------------------------------------------------------------------------
def case_workspace(route, lib, device, only=None):
    """Every unit of the route under the four workspace conditions ("Purity of calls"): (a) zeros, (b) 0xFF,
    (c) stale from the same unit at B + 3 on other inputs, the larger tensor passed on unchanged, (d) exact size between guards --
    which every condition has here, (d) being the one filled with the guards' own 0xA5.  Poison goes in front of a unit, never
    inside one."""
    eng = engine_of(route, lib, device)
    i = inputs_of(route, device)
    N = eng.N
    other = inputs_of(route, device, seed=17, extra=(N - 1, 2, N))
    n, n_big = ws_bytes(eng, i.B), ws_bytes(eng, other.B)
    assert 0 < n <= n_big
    for name, unit in units_of(route, eng).items():
        if only is not None and name not in only:
            continue
        what = f"{route.name} {name}"
        # (d) first: a store past the end lands in a guard before any run without one
        big = guarded_workspace(eng, n, None, device)
        exact = run_unit(eng, unit, i, f"{what} (d)")
        check_workspace_guards(big, n, f"{what} (d)")
        big = guarded_workspace(eng, n, 0x00, device)
        want = run_unit(eng, unit, i, f"{what} (a)")
        check_workspace_guards(big, n, f"{what} (a)")
        for k, t in want.items():
            assert torch.isfinite(t).all(), f"{what} (a): {k} is not finite"
        assert_same(exact, want, f"{what}: exact-size workspace of 0xA5 between guards against 0x00")
        big = guarded_workspace(eng, n, 0xFF, device)
        assert_same(run_unit(eng, unit, i, f"{what} (b)"), want, f"{what}: workspace 0xFF against 0x00")
        check_workspace_guards(big, n, f"{what} (b)")
        big = guarded_workspace(eng, n_big, 0x00, device)
        run_unit(eng, unit, other, f"{what} (c, B = {other.B})")
        assert_same(run_unit(eng, unit, i, f"{what} (c)"), want, f"{what}: stale workspace of B = {other.B} against 0x00")
        check_workspace_guards(big, n_big, f"{what} (c)")


def case_pad_geometry():
    """The complex routes reach both paddings: E % 4 != 0 (pad columns of H, Ep) and K % 4 != 0 (Kp)."""
    geo = {}
    for r in ROUTES.values():
        meta, _ = r.source()
        if meta["is_cc"]:
            N, _, d_min, d_max = sc.dims(meta)
            geo[r.name] = sc.O.get_rank2_dim(N, d_min, d_max)
    assert any(E % 4 for E, _ in geo.values()) and any(K % 4 for _, K in geo.values()), geo
    assert geo["community_small_CC"][0] == 190


# ---- 3. independence of a sample from its batch -------------------------------------------------------------------------------------
def case_batch(route, lib, device):
    """Rows of ccsd_score, ccsd_predictor (host and Philox noise) and of the apply half given the B = 6 sums: under a permutation of
    the batch, alone (B = 1) and as the first three (B = 3).  ccsd_init_state row by row.  The six sums against the float64 sum of the
    per-row norms of the B = 1 calls, within SUMS_BOUND."""
    eng = engine_of(route, lib, device)
    full = inputs_of(route, device)
    B = full.B
    assert B == 6
    guarded_workspace(eng, ws_bytes(eng, B), 0xFF, device)     # (the sub-batches run in the same, larger and stale, tensor)
    units = units_of(route, eng)
    pair = [k for k in units if k.startswith("norms+")]
    plain = {k: u for k, u in units.items() if k not in pair and k != "predictor philox"}
    want = {k: run_unit(eng, u, full, f"{route.name} {k}", check=False) for k, u in plain.items()}
    sums = None
    if pair:
        sums = new_sums(eng)
        norms(eng, full, sums)
        want["apply"] = {k: t.cpu().clone() for k, t in apply(eng, full, sums).items()}
    if "predictor philox" in units:
        want["philox"] = {k: t.cpu() for k, t in units["predictor philox"](eng, full).items()}
    prior = eng.alloc_state(B)
    eng.init_state(full.flags, prior, None, SEED, OFFSET)
    prior = [None if t is None else t.cpu().clone() for t in prior]
    row_norms = torch.zeros(B, 6, dtype=torch.float64)
    for rows in [PERM, [0, 1, 2]] + [[b] for b in range(B)]:
        sub = full.rows(rows)
        what = f"{route.name} rows {rows} of B = {B}"
        pick = lambda d: {k: t[rows] for k, t in d.items()}
        for k, u in plain.items():
            assert_same(run_unit(eng, u, sub, what, check=False), pick(want[k]), f"{what}: {k}")
        if pair:
            s = new_sums(eng)
            norms(eng, sub, s)
            if len(rows) == 1:
                row_norms[rows[0]] = s[:6].double().cpu()
            s.copy_(sums)                                        # the same six sums
            assert_same({k: t.cpu() for k, t in apply(eng, sub, s).items()}, pick(want["apply"]), f"{what}: {pair[0]} given the B = {B} sums")
        if rows == list(range(rows[0], rows[0] + len(rows))):   # a run of the batch: its rows sit at sample_offset + rows[0]
            if "philox" in want:
                got = units["predictor philox"](eng, sub, offset=OFFSET + rows[0])
                assert_same({k: t.cpu() for k, t in got.items()}, pick(want["philox"]), f"{what}: ccsd_predictor, Philox noise at offset + {rows[0]}")
            st = eng.alloc_state(len(rows))
            eng.init_state(sub.flags, st, None, SEED, OFFSET + rows[0])
            for p, a, b in zip(NAMES, st, prior):
                assert a is None or torch.equal(a.cpu(), b[rows]), f"{what}: ccsd_init_state {p} at offset + {rows[0]}"
    if pair:
        got = sums[:6].double().cpu()
        ref64 = row_norms.sum(0)
        seq32 = torch.zeros(6, dtype=torch.float32)
        for b in range(B):
            seq32 = seq32 + row_norms[b].float()
        live = ref64 > 0
        assert live[[0, 1, 3, 4]].all() and torch.equal(got[~live], ref64[~live])
        measured = ((seq32.double() - ref64).abs()[live] / ref64[live]).max().item()
        seen = ((got - ref64).abs()[live] / ref64[live]).max().item()
        print(f"six sums {route.name}: float32 sequential sum against float64 {measured:.3e} (recorded {SUMS_MEASURED:.1e}), "
              f"observed {seen:.3e}, bound {SUMS_BOUND:.1e}")
        assert measured <= SUMS_MEASURED, f"{route.name}: float32 sequential sum against float64 {measured:.3e}: above the recorded {SUMS_MEASURED:.2e}"
        assert seen <= SUMS_BOUND, f"{route.name}: the six sums are {seen:.3e} from the float64 sum of the per-row norms (bound {SUMS_BOUND:.1e})"


# ---- 4. plans side by side ----------------------------------------------------------------------------------------------------------
def _trio(lib, device):
    """P = qm9_CC, Q = gdss_community_small, P' = a second plan of qm9_CC; their inputs; the solo results of their units."""
    rp, rq = ROUTES["qm9_CC"], ROUTES["gdss_community_small"]
    plans = {"P": (rp, engine_of(rp, lib, device), inputs_of(rp, device, 31)), "Q": (rq, engine_of(rq, lib, device), inputs_of(rq, device, 32)),
             "P'": (rp, rp.build(lib, device), inputs_of(rp, device, 33))}
    solo = {}
    for tag, (_, eng, i) in plans.items():
        pin_workspace(eng, filled(ws_bytes(eng, i.B), 0, device))
        solo[tag] = {"score": u_score(1)(eng, i), "predictor": u_predictor(True)(eng, i), "pair": u_pair(eng, i)}
        solo[tag] = {k: {n: t.cpu().clone() for n, t in v.items()} for k, v in solo[tag].items()}
    return plans, solo


def case_interleaved(lib, device):
    """Units of three live plans interleaved on one stream, each bit-equal to the plan's solo result: with separate workspaces, a
    corrector pair split by another plan's call; with ONE workspace tensor for all three, pairs unsplit (a unit is self-contained)."""
    plans, solo = _trio(lib, device)
    got = {tag: {} for tag in plans}
    pending = {}

    def do(tag, what):
        _, eng, i = plans[tag]
        if what == "norms":
            pending[tag] = new_sums(eng)
            norms(eng, i, pending[tag])
        elif what == "apply":
            got[tag]["pair"] = dict(apply(eng, i, pending[tag]), sums=pending.pop(tag))
        else:
            got[tag][what] = {"score": u_score(1), "predictor": u_predictor(True), "pair": u_pair}[what](eng, i)

    def compare(how):
        for tag in plans:
            assert set(got[tag]) == {"score", "predictor", "pair"}
            for k, res in got[tag].items():
                assert_same({n: t.cpu() for n, t in res.items()}, solo[tag][k], f"{how}: plan {tag} {k}")
            got[tag].clear()

    for tag, (_, eng, i) in plans.items():
        pin_workspace(eng, filled(ws_bytes(eng, i.B), 0xFF, device))
    for tag, what in [("P", "norms"), ("Q", "score"), ("P", "apply"), ("P'", "norms"), ("Q", "norms"), ("P", "score"), ("P'", "apply"),
                      ("P'", "predictor"), ("Q", "apply"), ("P", "predictor"), ("Q", "predictor"), ("P'", "score")]:
        do(tag, what)
    compare("separate workspaces")
    shared = filled(max(ws_bytes(eng, i.B) for _, eng, i in plans.values()), 0xFF, device)
    for _, eng, _ in plans.values():
        pin_workspace(eng, shared)
    for tag, what in [("P", "pair"), ("Q", "score"), ("P'", "predictor"), ("Q", "pair"), ("P", "score"), ("P'", "pair"), ("Q", "predictor"),
                      ("P'", "score"), ("P", "predictor")]:
        do(tag, what)
    compare("one shared workspace")


def case_growth(lib, device):
    """The plan-owned off-bit buffer of ccsd_init_state / ccsd_noise_draws across growing: B = 2, 300, 2 on one plan, each bit-equal
    to the same call on a fresh plan.  gdss_community_small: graph-only, so B = 300 stays small."""
    route = ROUTES["gdss_community_small"]
    N = sc.dims(route.source()[0])[0]

    def calls(eng, B):
        flags = make_flags(B, N, sc.counts_of(N)).to(device)
        out = []
        for call in (lambda st: eng.init_state(flags, st, None, SEED, OFFSET), lambda st: eng.noise_draws(flags, 1, 0, st, SEED, OFFSET)):
            st = eng.alloc_state(B)
            for t in st[:2]:
                t.fill_(float("nan"))
            call(st)
            out += [t.cpu().clone() for t in st[:2]]
        return out

    one = route.build(lib, device)
    for B in (2, 300, 2):
        got, want = calls(one, B), calls(route.build(lib, device), B)
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.isfinite(a).all() and torch.equal(a, b), f"B = {B}: tensor {k} differs from a fresh plan's"


def case_two_streams(lib, device, steps=3):
    """Device only.  P and P' run ccsd_sampler_run on two streams at the same time, each with its own workspace and states, each
    bit-equal to its solo run.  Both streams start behind equal sleeps and must both still be busy when the last enqueue returns, so
    neither queue ran to its end before the other had work."""
    route = LOOP_ROUTES["fused_merged_folded"]
    engs = [route.build(lib, device), route.build(lib, device)]
    ins = [inputs_of(route, device, 51), inputs_of(route, device, 52)]
    unit = u_loop(steps)
    solo = [{k: t.cpu().clone() for k, t in unit(e, i).items()} for e, i in zip(engs, ins)]
    streams = [side_stream(device)]
    streams.append(side_stream(device, streams[0]))              # (two streams that share no hardware queue: runs_beside)
    for e, i in zip(engs, ins):
        pin_workspace(e, filled(ws_bytes(e, i.B), 0xFF, device))
    t0 = time.perf_counter()
    for e, i in zip(engs, ins):
        unit(e, i)
    enqueue = time.perf_counter() - t0
    torch.cuda.synchronize(device)
    sleep_ms = max(10 * 3 * enqueue * 1e3, 5.0)
    got, done = [None, None], []
    # both streams sleep first, for the same time, long enough for every round of both to be enqueued behind the sleeps: when the
    # sleeps end, both queues hold all their work and the device runs them side by side
    for k in (0, 1):
        with torch.cuda.stream(streams[k]):
            torch.cuda._sleep(int(sleep_ms * cycles_per_ms(device)))
    for rep in range(3):
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                got[k] = unit(engs[k], ins[k])
    for k in (0, 1):
        done.append(torch.cuda.Event())
        done[k].record(streams[k])
    pending = [not ev.query() for ev in done]
    for s in streams:
        s.synchronize()
    print(f"two streams: enqueue of one round {enqueue * 1e3:.3f} ms, sleep {sleep_ms:.2f} ms")
    assert all(pending), f"a stream had finished its work when the other's last enqueue returned ({pending}): the {sleep_ms:.2f} ms sleep was too short, the runs may not have overlapped"
    for k in (0, 1):
        assert_same({n: t.cpu() for n, t in got[k].items()}, solo[k], f"plan {k} beside the other on a second stream")


# ---- 5. stream discipline (device only) ---------------------------------------------------------------------------------------------
# calls that may synchronise the host (include/ccsd_hip.h): exempt from the pending-event assertion, not from the bit-equality
HOST_SYNC = {"nspdk_features", "init_state growing"}
_clock = {}


def cycles_per_ms(device):
    """torch.cuda._sleep's cycle rate, measured once."""
    if device not in _clock:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        torch.cuda.synchronize(device)
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
        torch.cuda.synchronize(device)
        _clock[device] = 20_000_000 / a.elapsed_time(b)
    return _clock[device]


def runs_beside(device, a, b):
    """Whether work on stream `b` runs while stream `a` is busy.  The runtime maps streams onto a few hardware queues (4 by default),
    and two streams that share one run in order whatever the API promises: a launch gone astray onto such a stream would still wait,
    and the side-stream construction could not tell it."""
    with torch.cuda.stream(a):
        torch.cuda._sleep(int(2.0 * cycles_per_ms(device)))
        ea = torch.cuda.Event()
        ea.record(a)
    with torch.cuda.stream(b):
        torch.zeros(8, device=device).add_(1)
        eb = torch.cuda.Event()
        eb.record(b)
    eb.synchronize()
    beside = not ea.query()
    a.synchronize()
    return beside


_side = {}


def side_stream(device, beside=None):
    """A non-blocking stream on which work demonstrably runs beside the null stream (and beside `beside`), found once."""
    key = (str(device), beside)
    if key not in _side:
        cycles_per_ms(device)
        for _ in range(32):
            s = torch.cuda.Stream(device)
            others = [torch.cuda.default_stream(device)] + ([] if beside is None else [beside])
            if s not in others and all(runs_beside(device, s, o) and runs_beside(device, o, s) for o in others):
                _side[key] = s
                break
        else:
            raise AssertionError("no stream that runs beside the null stream: every candidate shares its hardware queue")
    return _side[key]


def poison_like(t):
    return torch.full_like(t, float("nan")) if t.dtype.is_floating_point else torch.full_like(t, -1)


def on_side_stream(device, tensors, call, what, may_sync=False, side_call=None, prepare=None):
    """`call(tensors)` on the default stream, then on a side stream behind a sleep and the copies that give its input buffers their
    values.  `prepare()` runs right before the side-stream run and fills the workspace or scratch of the call with 0xFF, so that it does
    not hold the bit-identical intermediates of the default-stream run.  A launch or copy the library issued on another stream would
    not wait for the sleep: it reads poison -- from the inputs, or from the workspace, which the launches ordered before it have not
    yet written -- and NaN reaches the outputs.  NOT detectable: a memset on another stream (it reads nothing and zeroes early, what
    the ordered one would have done), and a launch all of whose operands are plan-owned (weights, tables, the off-bit buffer of
    ccsd_init_state), which hold the same values in both runs.  The side stream is one that demonstrably runs beside the null stream
    (side_stream): one that shares the null stream's hardware queue would order the stray launch by accident.  The event recorded behind the copies must still be pending when the
    call returns -- else the sleep was too short to tell."""
    call(tensors)                                                # (warm: the first launch of a kernel loads its code object)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    bufs = [poison_like(t) for t in tensors]
    for b, t in zip(bufs, tensors):
        b.copy_(t, non_blocking=True)
    want = call(bufs)
    enqueue = time.perf_counter() - t0
    torch.cuda.synchronize(device)
    want = {k: t.cpu().clone() for k, t in want.items()}
    sleep_ms = max(10 * enqueue * 1e3, 2.0)
    print(f"{what}: host-side enqueue {enqueue * 1e3:.3f} ms, sleep {sleep_ms:.2f} ms")
    s = side_stream(device)
    bufs = [poison_like(t) for t in tensors]
    if prepare is not None:
        prepare()
    torch.cuda.synchronize(device)
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(sleep_ms * cycles_per_ms(device)))
        for b, t in zip(bufs, tensors):
            b.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
        got = (side_call or call)(bufs)
        pending = not ev.query()
    s.synchronize()
    assert may_sync or pending, f"{what}: the input copies had completed when the call returned: the {sleep_ms:.2f} ms sleep was too short to tell"
    got = {k: t.cpu() for k, t in got.items()}
    assert_same(got, want, f"{what}: on a side stream against the default stream")


def case_stream_harness(device):
    """on_side_stream itself, in plain torch: work ordered on the side stream passes; the same work issued on the null stream, which a
    non-blocking stream does not order against, starts under the sleep, reads the poison and fails the comparison."""
    t = [torch.arange(1024, dtype=torch.float32, device=device)]
    on_side_stream(device, t, lambda bufs: {"y": bufs[0] * 2}, "a torch kernel on the current stream")

    def astray(bufs):
        with torch.cuda.stream(torch.cuda.default_stream(device)):
            return {"y": bufs[0] * 2}

    with pytest.raises(AssertionError, match="on a side stream against the default stream"):
        on_side_stream(device, t, lambda bufs: {"y": bufs[0] * 2}, "a torch kernel on the null stream", side_call=astray)
    # two stages through a kept scratch buffer, the second reading nothing but the scratch: astray, it passes while the scratch still
    # holds the first run's values, and fails once the scratch is refilled in front of the side-stream run
    scratch = torch.full((1024,), float("nan"), device=device)

    def staged(second_astray):
        def run(bufs):
            torch.mul(bufs[0], 2, out=scratch)
            with torch.cuda.stream(torch.cuda.default_stream(device) if second_astray else torch.cuda.current_stream(device)):
                return {"y": scratch + 1}
        return run

    refill = lambda: scratch.fill_(float("nan"))
    on_side_stream(device, t, staged(False), "two stages in order", prepare=refill)
    on_side_stream(device, t, staged(False), "second stage astray, scratch stale", side_call=staged(True))      # (the blind spot)
    with pytest.raises(AssertionError, match="on a side stream against the default stream"):
        on_side_stream(device, t, staged(False), "second stage astray, scratch refilled", side_call=staged(True), prepare=refill)


def case_stream_unit(route, lib, device):
    eng = engine_of(route, lib, device)
    i = inputs_of(route, device)
    ws = filled(ws_bytes(eng, i.B), 0xFF, device)
    pin_workspace(eng, ws)
    for name, unit in units_of(route, eng).items():
        on_side_stream(device, i.tensors(), lambda ts: unit(eng, i.like(ts)), f"{route.name} {name}", prepare=lambda: ws.fill_(0xFF))


# ---- 2. the plan-free operations ----------------------------------------------------------------------------------------------------
# Inputs: the smallest fixtures the suites of the operations already build (finish_cases.inputs, lift_cases.random_graphs,
# eval_cases.mmd_set, spectrum_cases.solver_matrices), as CPU tensors.
def _graphs(B, N, p, seed):
    return torch.from_numpy(lc.random_graphs(B, N, p, seed))


def _finish_inputs():
    """finish_cases' geometry n5: N = 5, d = 3..4: E = 10, K = 15 (K % 4 = 3), B = 3: B E K = 450 (% 4 = 2)."""
    t = fc.inputs("n5")
    assert tuple(t["rank2"].shape) == (3, 10, 15)
    return [t["x"], t["adj"], t["rank2"], t["flags"]]


def _mmd_inputs():
    """eval_cases' set n130_l200: n1 = 130, n2 = 3 (no multiples of 64), L = 200 (no multiple of 32), ragged, with rows without mass."""
    r1, l1, r2, l2 = ec.mmd_set("n130_l200")
    assert r1.shape == (130, 200) and r2.shape == (3, 200) and (l1 < 200).any()
    return [torch.from_numpy(a) for a in (r1, l1, r2, l2)]


def _sym64(n, B):
    return torch.from_numpy(spc.solver_matrices(n, B)["random"])


def _hodge_inputs(lib, device):
    """The complexes of finish_cases' n5: the adjacency and the cell bits finish() gives for it."""
    return [fc.inputs("n5")["adj"], fc.run(lib, device, "n5", False)["rank2_cell_bits"]]


def _op_finish(ops, ts):
    return ops.finish(ts[0], ts[1], ts[2], ts[3], d_min=3, d_max=4)


def _op_mmd(ops, ts):
    return {"mmd": ops.mmd(ts[0], ts[2], "emd", lens1=ts[1], lens2=ts[3])}


def _op_nspdk_mmd(ops, ts):
    a, b = ({"nspdk_indptr": ts[k], "nspdk_indices": ts[k + 1], "nspdk_values": ts[k + 2]} for k in (0, 3))
    return {"nspdk_mmd": ops.nspdk_mmd(a, b)}


def _op_hodge(ops, ts):
    return {"hodge": ops.hodge_spectrum(ts[0], ts[1], d_min=3, d_max=4)}


# name -> (inputs () -> [cpu tensors], call (ops, tensors) -> {name: tensor}, the scratch the call asks for (lib, tensors) -> bytes or None)
OPS = {
    "finish": (_finish_inputs, _op_finish, None),
    "cluster_hist": (lambda: [fc.inputs("g65")["adj"]], lambda ops, ts: ops.cluster_hist(ts[0]), None),
    "orbit_counts": (lambda: [_graphs(3, 9, 0.4, 6)], lambda ops, ts: ops.orbit_counts(ts[0], per_node=True), None),
    "nspdk_features": (lambda: [_graphs(3, 9, 0.3, 7), torch.randint(0, 3, (3, 9), generator=torch.Generator().manual_seed(8))],
                       lambda ops, ts: ops.nspdk_features(ts[0], ts[1]), lambda lib, ts: lib.ccsd_nspdk_workspace_bytes(3, 9)),
    "mmd": (_mmd_inputs, _op_mmd, lambda lib, ts: lib.ccsd_mmd_workspace_bytes(130, 3, 200)),
    "eigvalsh n=5": (lambda: [_sym64(5, 3)], lambda ops, ts: {"w": ops.eigvalsh(ts[0])}, lambda lib, ts: lib.ccsd_eig_workspace_bytes(3, 5)),
    "eigvalsh n=129": (lambda: [_sym64(129, 2)], lambda ops, ts: {"w": ops.eigvalsh(ts[0])}, lambda lib, ts: lib.ccsd_eig_workspace_bytes(2, 129)),
    "spectral_hist": (lambda: [_graphs(3, 9, 0.4, 13)], lambda ops, ts: ops.spectral_hist(ts[0], eig=True),
                      lambda lib, ts: lib.ccsd_spectral_workspace_bytes(3, 9)),
    "lift path_based": (lambda: [_graphs(3, 9, 0.4, 16)], lambda ops, ts: ops.lift(ts[0], "path_based", d_min=3, d_max=3), None),
    "lift path_based dense": (lambda: [_graphs(3, 9, 0.4, 16)], lambda ops, ts: ops.lift(ts[0], "path_based", d_min=3, d_max=3, dense=True), None),
    "lift cycles": (lambda: [_graphs(3, 12, 0.3, 17)], lambda ops, ts: ops.lift(ts[0], "cycles", d_min=3, d_max=4), None),
    "lift cycles dense": (lambda: [_graphs(3, 12, 0.3, 17)], lambda ops, ts: ops.lift(ts[0], "cycles", d_min=3, d_max=4, dense=True), None),
}
_nspdk_rows = {}


def _nspdk_mmd_inputs(lib, device):
    """Two sets of rows from nspdk_features itself (5 and 3 graphs, one without an edge)."""
    key = (id(lib), str(device))
    if key not in _nspdk_rows:
        ops = sample_ops(lib, device)
        out = []
        for B, seed in ((5, 21), (3, 22)):
            adj = _graphs(B, 9, 0.3, seed)
            adj[0] = 0
            r = ops.nspdk_features(adj.to(device))
            out += [r["nspdk_indptr"].cpu(), r["nspdk_indices"].cpu(), r["nspdk_values"].cpu()]
        _nspdk_rows[key] = out
    return _nspdk_rows[key]


def op_parts(name, lib, device):
    if name == "nspdk_mmd":
        return (lambda: _nspdk_mmd_inputs(lib, device)), _op_nspdk_mmd, lambda lib, ts: lib.ccsd_nspdk_mmd_workspace_bytes(5, 3)
    if name == "hodge_spectrum":
        return (lambda: _hodge_inputs(lib, device)), _op_hodge, lambda lib, ts: lib.ccsd_hodge_workspace_bytes(3, 5)
    return OPS[name]


OP_NAMES = list(OPS) + ["nspdk_mmd", "hodge_spectrum"]


def case_op(name, lib, device):
    """A plan-free operation: scratch filled with 0x00 against 0xFF in equal bits; the scratch at exactly the size the
    *_workspace_bytes call returns, between guards, and the outputs between guards: every guard intact."""
    make, call, scratch = op_parts(name, lib, device)
    ts = [t.to(device) for t in make()]
    ops = sample_ops(lib, device)
    asked = []

    def with_fill(v):
        def _scratch(nbytes, dev):
            t = torch.full((max(int(nbytes), 8) // 8 + 1,), 0, dtype=torch.float64, device=dev)
            t.view(torch.uint8).fill_(v)
            asked.append(int(nbytes))
            return t
        ops._scratch = _scratch
        return {k: t.cpu().clone() for k, t in call(ops, ts).items()}

    want = with_fill(0x00)
    assert_same(with_fill(0xFF), want, f"{name}: scratch 0xFF against 0x00")
    assert (scratch is None) == (not asked), f"{name}: scratch requests {asked}"
    held = []

    def exact(nbytes, dev):
        """Exactly `nbytes` between guards, as a float64 tensor (the wrapper passes numel() * 8 as the size)."""
        assert nbytes == scratch(lib, ts), f"{name}: the wrapper asks for {nbytes} bytes, the size call returns {scratch(lib, ts)}"
        n = (int(nbytes) + 7) // 8 * 8
        big = filled(max(n, 8) + 2 * GUARD, FILL, dev)
        held.append((big, max(n, 8)))
        return big[GUARD:GUARD + max(n, 8)].view(torch.float64)

    ops._scratch = exact
    with guarded() as g:
        got = {k: t.cpu().clone() for k, t in call(ops, ts).items()}
        g.check(name)
    for big, n in held:
        assert (big[:GUARD] == FILL).all().item() and (big[GUARD + n:] == FILL).all().item(), f"{name}: a guard around the scratch was written"
    assert_same(got, want, f"{name}: exact-size scratch and outputs between guards")


def case_stream_op(name, lib, device):
    make, call, _ = op_parts(name, lib, device)
    ts = [t.to(device) for t in make()]
    ops = sample_ops(lib, device)
    held = {}

    def _scratch(nbytes, dev):
        """One buffer per requested size, kept: the side-stream run gets the buffer the default-stream runs used, refilled."""
        n = max(int(nbytes), 8) // 8 + 1
        if n not in held:
            held[n] = torch.empty(n, dtype=torch.float64, device=dev)
            held[n].view(torch.uint8).fill_(0xFF)
        return held[n]

    def refill():
        for t in held.values():
            t.view(torch.uint8).fill_(0xFF)

    ops._scratch = _scratch
    on_side_stream(device, ts, lambda bufs: call(ops, bufs), name, may_sync=name in HOST_SYNC, prepare=refill)


def case_stream_init_state(lib, device):
    """ccsd_init_state on a side stream: at the plan's first batch (no buffer to grow: asynchronous) and growing (it may synchronise)."""
    route = ROUTES["gdss_community_small"]
    eng, small = route.build(lib, device), route.build(lib, device)
    N = eng.N

    def call(eng, B):
        def run(ts):
            st = eng.alloc_state(B)
            eng.init_state(ts[0], st, None, SEED, OFFSET)
            return _named("prior", st)
        return run

    f6, f40 = (make_flags_holes(B, N, sc.counts_of(N), 60 + B).to(device) for B in (6, 40))
    on_side_stream(device, [f6], call(eng, 6), "init_state")
    call(small, 6)([f6])            # `small` holds a buffer for 6 samples: its call at B = 40 on the side stream is the one that grows
    on_side_stream(device, [f40], call(eng, 40), "init_state growing", may_sync=True, side_call=call(small, 40))
