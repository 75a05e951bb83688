"""Cases of the library loop with a reduce hook (ccsd_sampler_run_ex) and with several Langevin inner iterations, shared by the
host-emulation suite (tests/test_library_loop.py) and the GPU suite (tests/test_library_loop_gpu.py, -m gpu).  `lib` / `device`
select the backend as in tests/parity_cases.py.  Every comparison is against ccsd_sampler_run, the step-wise driver, the plain
single-process run or the oracle: no fixture of its own."""
import json
import os
import socket
import subprocess
import sys

import torch

from ccsd_amd import loader, solver
from ccsd_amd.plan import rank2_dim
from oracle import ccsd_oracle as O
from tests import parity_cases as pc
from tests.helpers import ROOT, load_ckpt_np, make_flags

# (checkpoint, predictor, corrector, snr, scale_eps, node counts, expected CCSD_QUERY_LOOP_FORM): one plan per loop form and per
# kernel family that serves a norms pass
FORMS = {
    "qm9_langevin_fused_merged": ("ccsd_qm9_CC", "Reverse", "Langevin", 0.2, 0.7, [9, 7, 8, 0, 4, 9, 5, 6], 2),
    "community_small_cc_tiled_fuse": ("ccsd_community_small_CC", "Euler", "Langevin", 0.05, 0.7, [20, 12, 16, 18, 14, 20], 2),
    "graph_only_langevin": ("gdss_community_small", "Euler", "Langevin", 0.05, 0.7, [20, 12, 16, 18, 14], 1),
    "enzymes_small_cc_s4": ("ccsd_enzymes_small_CC", "S4", "None", 0.15, 0.7, [12, 9, 5, 11, 12, 7], 3),
    "zinc5b_ew1": ("zinc250k_CC_5b", "Reverse", "Langevin", 0.2, 0.9, [38, 23, 31], 2),
    "qm9_corrector_free": ("ccsd_qm9_CC", "Euler", "None", 0.0, 0.0, [9, 7, 8, 0, 4, 9, 5, 6], 0),
}


def _source(name):
    """(meta in the checkpoint layout, weights) of a shipped checkpoint or of the N = 38 substitute (tests/golden)."""
    if name != "zinc250k_CC_5b":
        return load_ckpt_np(name)
    _, meta5, sd, _, _ = pc.zinc5b_setup()
    N, Fd, d_min, d_max, _, _ = meta5["dims"]
    meta = {"is_cc": True, "config": {"data": {"max_node_num": N, "max_feat_num": Fd, "d_min": d_min, "d_max": d_max},
                                      "sde": {p: dict(meta5["sde"][p], num_scales=1000) for p in ("x", "adj", "rank2")}}}
    parts = {}
    for p in ("x", "adj", "rank2"):
        meta[f"params_{p}"] = meta5["params"][p]
        parts[p] = {k: v.clone().requires_grad_(True) for k, v in sd[p].items()}
    return meta, parts


class Setup:
    """One sampler configuration on one backend: the models, the SDEs and closures of get_pc_sampler / S4_solver for it."""

    def __init__(self, name, lib, device, predictor, corrector, snr, seps, n_steps=1):
        self.name, self.lib, self.device = name, lib, device
        self.predictor, self.corrector, self.snr, self.seps, self.n_steps = predictor, corrector, snr, seps, n_steps
        self.meta, self.parts = _source(name)
        cfg = self.cfg = self.meta["config"]
        self.is_cc = self.meta["is_cc"]
        self.N, self.F = cfg["data"]["max_node_num"], cfg["data"]["max_feat_num"]
        self.names = ["x", "adj"] + (["rank2"] if self.is_cc else [])
        self.nt = len(self.names)
        self.models = [loader.load_model_from_ckpt(self.meta[f"params_{p}"], self.parts[p], device) for p in self.names]

    def kwargs(self, B):
        kw = dict(shape_x=(B, self.N, self.F), shape_adj=(B, self.N, self.N), predictor=self.predictor, corrector=self.corrector,
                  snr=self.snr, scale_eps=self.seps, n_steps=self.n_steps, probability_flow=False, continuous=True, denoise=True,
                  eps=1e-4)
        if self.is_cc:
            d_min, d_max = self.cfg["data"]["d_min"], self.cfg["data"]["d_max"]
            kw.update(is_cc=True, shape_rank2=(B, *rank2_dim(self.N, d_min, d_max)), d_min=d_min, d_max=d_max)
        return kw

    def sampler(self, B, steps, seed, **extra):
        sd = [loader.load_sde(self.cfg["sde"][p]) for p in self.names]
        skw = dict(sde_x=sd[0], sde_adj=sd[1])
        if self.is_cc:
            skw["sde_rank2"] = sd[2]
        make = solver.S4_solver if self.predictor == "S4" else solver.get_pc_sampler
        return make(device=self.device, rng="philox", seed=seed, max_steps=steps, lib=self.lib, **skw, **self.kwargs(B), **extra)

    def engine(self, B, seed=1):
        """The PCEngine of a closure for batch B (built by a zero-step call: the prior draw only)."""
        fn = self.sampler(B, 0, seed)
        fn(*self.models, make_flags(B, self.N, [self.N]).to(self.device))
        return fn.engine()


def engine_run(eng, flags, steps, seed, reduce=None, use_reduce=True, traj=True):
    """init_state + PCEngine.run on buffers of its own -> (state, result, traj rows of the steps run), everything cloned to the
    host.  use_reduce=False calls run without the keyword: plain ccsd_sampler_run."""
    B = flags.shape[0]
    state, scratch, result = (eng.alloc_state(B) for _ in range(3))
    nt = 3 if eng.is_cc else 2
    tr = None
    if traj:
        per = sum(s[1] * s[2] for s in eng.shapes(B)[:nt])
        tr = torch.zeros(steps, per, device=eng.device)      # (the loop writes row `step` of the steps it runs: first_step = 0 here)
    eng.init_state(flags, state, None, seed, 0)
    if use_reduce:
        eng.run(flags, state, scratch, result, seed, 0, 0, steps, tr, reduce=reduce)
    else:
        eng.run(flags, state, scratch, result, seed, 0, 0, steps, tr)
    host = lambda ts: [t.detach().cpu().clone() for t in ts[:nt]]
    return host(state), host(result), (tr[:steps].detach().cpu().clone() if traj else None)


def case_hook_identity(form, lib, device, B, steps, seed=13):
    """A hooked run whose hook only counts == ccsd_sampler_run, bit for bit in x, adj, rank2 (the state), the result and the
    trajectory; the hook fires steps x n_steps times for Langevin, steps times for S4, never for corrector None."""
    name, predictor, corrector, snr, seps, counts, loop_form = FORMS[form]
    su = Setup(name, lib, device, predictor, corrector, snr, seps)
    eng = su.engine(B)
    assert eng.query("loop_form") == loop_form, f"{form}: loop form {eng.query('loop_form')}, expected {loop_form}"
    flags = make_flags(B, su.N, counts).to(device)
    plain = engine_run(eng, flags, steps, seed, use_reduce=False)
    calls = []

    def count(sums):
        assert sums.dtype == torch.float32 and tuple(sums.shape) == (6,) and sums.device.type == torch.device(device).type
        calls.append(1)

    hooked = engine_run(eng, flags, steps, seed, reduce=count)
    none = engine_run(eng, flags, steps, seed, reduce=None)
    want = steps if predictor == "S4" else steps * su.n_steps if corrector == "Langevin" else 0
    assert len(calls) == want, f"{form}: the hook fired {len(calls)} times, expected {want}"
    for what, run in (("hooked", hooked), ("reduce=None", none)):
        for part, a, b in zip(("state", "result"), plain[:2], run[:2]):
            for p, u, v in zip(su.names, a, b):
                assert torch.isfinite(u).all()
                assert torch.equal(u, v), f"{form}: {what} run != ccsd_sampler_run in {part} {p}"
        assert torch.equal(plain[2], run[2]), f"{form}: {what} run != ccsd_sampler_run in the trajectory"
    assert plain[2].abs().sum() > 0


def _differs(a, b, rtol):
    scale = max(b.abs().max().item(), 1e-6)
    return (a - b).abs().max().item() > rtol * scale


def case_hook_values_are_consumed(lib, device, B, steps, predictor, rtol, seed=19, name="ccsd_qm9_CC"):
    """The sums the hook sees are what the kernels consume: the six sums of every norms pass of a batch-B run, written by a hook
    into a run of the first B/2 complexes (same seed, sample_offset 0), make that run reproduce rows 0 .. B/2-1 of the full
    one -- bit for bit on the emulation (rtol = 0), assert_close(rtol) on the GPU, where the threads per graph of k_xa depend on
    the batch.  The same half-batch run with a hook that does nothing must differ."""
    corrector, snr, seps = ("None", 0.15, 0.7) if predictor == "S4" else ("Langevin", 0.2, 0.7)
    su = Setup(name, lib, device, predictor, corrector, snr, seps)
    eng = su.engine(B)
    counts = [9, 7, 8, 3, 4, 9, 5, 6, 2, 9, 1]
    flags = make_flags(B, su.N, counts).to(device)
    half = B // 2
    rec = []
    full = engine_run(eng, flags, steps, seed, reduce=lambda s: rec.append(s.clone()))
    assert len(rec) == steps
    it = iter(rec)
    fed = engine_run(eng, flags[:half].contiguous(), steps, seed, reduce=lambda s: s.copy_(next(it)))
    noop = engine_run(eng, flags[:half].contiguous(), steps, seed, reduce=lambda s: None)
    differ = False
    for part, a, b, c in zip(("state", "result", "traj"), full, fed, noop):
        if part == "traj":       # sample 0 of every step: the same row in both runs
            a, b, c = [a], [b], [c]
            names = ["traj"]
        else:
            a = [t[:half] for t in a]
            names = su.names
        for p, u, v, w in zip(names, a, b, c):
            what = f"{name} {predictor}: half batch fed with the full batch's sums, {part} {p}"
            print(f"{what}: max abs diff {(u - v).abs().max().item():.3e} (scale {u.abs().max().item():.3e}); "
                  f"no-op hook {(u - w).abs().max().item():.3e}")
            if rtol == 0:
                assert torch.equal(u, v), what
            else:
                pc.assert_close(v, u, what, rtol=rtol)
            differ = differ or _differs(w, u, rtol)
    assert differ, f"{name} {predictor}: a half-batch run with per-shard sums equals the full batch -- the hook's values are not what the kernels read"


def case_nsteps_library_vs_stepwise(name, lib, device, B, counts, steps, predictor, snr, seps, n_steps, seed=23, keep_traj=False):
    """sampler.n_steps = k inside the library loop: the closure reports last_loop == "library" and equals the step-wise driver
    (reached with a group object while torch.distributed is uninitialised) bit for bit; ccsd_sampler_run itself returns CCSD_OK."""
    import torch.distributed as dist

    assert not (dist.is_available() and dist.is_initialized())
    su = Setup(name, lib, device, predictor, "Langevin", snr, seps, n_steps=n_steps)
    flags = make_flags(B, su.N, counts).to(device)
    fn = su.sampler(B, steps, seed, keep_traj=keep_traj)
    got = fn(*su.models, flags)
    assert fn.last_loop == "library", f"{name} n_steps={n_steps}: the closure took the {fn.last_loop} loop"
    assert fn.engine().query("loop_form") == 4
    fs = su.sampler(B, steps, seed, keep_traj=keep_traj, group=pc._FakeGroup())
    ref = fs(*su.models, flags)
    assert fs.last_loop == "stepwise"
    for p, a, b in zip(su.names, got[:su.nt], ref[:su.nt]):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"{name} n_steps={n_steps}: library loop != step-wise driver for {p}"
    assert int(got[su.nt]) == int(ref[su.nt])
    if keep_traj:
        assert len(got[-1]) == steps == len(ref[-1])
        for i, (gs, ws) in enumerate(zip(got[-1], ref[-1])):
            for p, a, b in zip(su.names, gs, ws):
                assert torch.equal(a, b), f"{name} n_steps={n_steps}: traj[{i}] {p} differs from the step-wise driver's"
    # the C call on buffers of our own: CCSD_OK (PCEngine.run raises on any other status), the same state and result
    state, result, _ = engine_run(fn.engine(), flags, steps, seed, use_reduce=False, traj=False)
    for p, a, b in zip(su.names, got[:su.nt], result):
        assert torch.equal(a.cpu(), b), f"{name} n_steps={n_steps}: ccsd_sampler_run on fresh buffers differs in {p}"
    return su, fn, flags, got, state


def case_nsteps_vs_oracle(lib, device, B=5, counts=(9, 7, 8, 0, 4), steps=2, n_steps=2, seed=29):
    """qm9_CC, n_steps = 2, in the library loop against the oracle value for value: the draws of phases 0 .. n_steps exported by
    ccsd_noise_draws, replayed through RecordedNoise in the order the oracle consumes them (target-major within a step: every
    inner iteration of one target before the next target draws, solver.py:1131-1137)."""
    su, fn, flags, got, state = case_nsteps_library_vs_stepwise("ccsd_qm9_CC", lib, device, B, list(counts), steps, "Reverse", 0.2, 0.7,
                                                                n_steps, seed=seed)
    eng = fn.engine()
    host = lambda ts: [t.detach().cpu().clone() for t in ts[:su.nt]]
    buf = eng.alloc_state(B)
    eng.init_state(flags, buf, None, seed, 0)
    prior = host(buf)
    draws = []
    for step in range(steps):
        phase = []
        for ph in range(n_steps + 1):
            eng.noise_draws(flags, step, ph, buf, seed, 0)
            phase.append(host(buf))
        for k in range(su.nt):
            draws += [phase[it][k] for it in range(n_steps)]
        draws += phase[n_steps]
    so = [O.load_sde(su.cfg["sde"][p]) for p in su.names]
    nets = [(lambda x, a, r, f, p=p: O.run_network(su.meta[f"params_{p}"], su.parts[p], x, a, r, f)) for p in su.names]
    rec, final = O.RecordedNoise(draws), []
    ofn = O.get_pc_sampler(n_diff_steps=steps, keep_traj=False, noise=rec, prior=prior, final=final, sde_x=so[0], sde_adj=so[1],
                           sde_rank2=so[2], **su.kwargs(B))
    want = ofn(*nets, flags.cpu())
    assert rec.i == len(draws) == steps * su.nt * (n_steps + 1), "the oracle consumed a different number of draws"
    for p, a, b in zip(su.names, got[:su.nt], want):
        pc.assert_close(a, b, f"qm9_CC n_steps={n_steps} library loop vs oracle, result {p}")
    for p, a, b in zip(su.names, state, final):
        pc.assert_close(a, b, f"qm9_CC n_steps={n_steps} library loop vs oracle, state {p}")


def case_hook_failure(lib, device, B=6, steps=4, seed=31):
    """A reduce that raises on its second call: PCEngine.run raises that same exception, the hook was called exactly twice, and
    the engine is usable afterwards -- a following plain run equals one on a fresh engine."""
    su = Setup("ccsd_qm9_CC", lib, device, "Reverse", "Langevin", 0.2, 0.7)
    eng = su.engine(B)
    flags = make_flags(B, su.N, [9, 7, 8, 0, 4, 6]).to(device)
    boom = RuntimeError("reduce failed on purpose")
    calls = []

    def bad(sums):
        calls.append(1)
        if len(calls) == 2:
            raise boom

    try:
        engine_run(eng, flags, steps, seed, reduce=bad)
    except RuntimeError as e:
        assert e is boom, f"PCEngine.run raised {e!r}, not the hook's own exception"
    else:
        raise AssertionError("PCEngine.run swallowed the hook's exception")
    assert len(calls) == 2, f"the hook was called {len(calls)} times"
    after = engine_run(eng, flags, steps, seed, use_reduce=False)
    fresh = engine_run(su.engine(B), flags, steps, seed, use_reduce=False)
    for part, a, b in zip(("state", "result"), after[:2], fresh[:2]):
        for p, u, v in zip(su.names, a, b):
            assert torch.isfinite(u).all() and torch.equal(u, v), f"after a failed hook the engine's plain run differs in {part} {p}"
    assert torch.equal(after[2], fresh[2])


# ---- two gloo ranks on the emulation -----------------------------------------------------------------------------------------------
# (tag, checkpoint, predictor, corrector, snr, scale_eps, n_steps, node counts)
GLOO_SETTINGS = [("langevin_n1", "ccsd_qm9_CC", "Reverse", "Langevin", 0.2, 0.7, 1, [9, 7, 8, 3, 4, 9, 5, 6]),
                 ("langevin_n2", "ccsd_qm9_CC", "Reverse", "Langevin", 0.2, 0.7, 2, [9, 7, 8, 3, 4, 9, 5, 6]),
                 ("s4_enzymes", "ccsd_enzymes_small_CC", "S4", "None", 0.15, 0.7, 1, [12, 9, 5, 11])]
GLOO_STEPS, GLOO_SEED = 2, 5


def gloo_run(setting, lib, rank, world, group):
    tag, name, predictor, corrector, snr, seps, n_steps, counts = setting
    su = Setup(name, lib, "cpu", predictor, corrector, snr, seps, n_steps=n_steps)
    flags = make_flags(len(counts), su.N, counts)
    B = len(counts) // world
    fn = su.sampler(B, GLOO_STEPS, GLOO_SEED, sample_offset=rank * B, group=group)
    res = fn(*su.models, flags[rank * B:(rank + 1) * B])
    return res[:su.nt], fn.last_loop


def gloo_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from ccsd_amd import distributed
    from tests.emu_util import emu_library

    r, w, dev = distributed.init()
    assert (r, w, dev) == (rank, world, "cpu")
    torch.set_num_threads(2)
    lib = emu_library()
    out = {}
    for setting in GLOO_SETTINGS:
        res, loop = gloo_run(setting, lib, rank, world, dist.group.WORLD)
        loops = [None] * world
        dist.all_gather_object(loops, loop)
        full = distributed.all_gather_samples(res)
        out[setting[0]] = ([t.numpy() for t in full], loops)
    if rank == 0:
        q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def case_two_gloo_ranks(lib):
    """Exact mode over two gloo ranks, each driving its shard through the host emulation: both ranks take the library loop (the
    all-reduce is its reduce hook) and the gathered batch equals the single-process run at 2e-6."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = q.get(timeout=900)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for setting in GLOO_SETTINGS:
        tag = setting[0]
        single, loop = gloo_run(setting, lib, 0, 1, None)
        assert loop == "library"
        got, loops = out[tag]
        assert loops == ["library", "library"], f"{tag}: the ranks took {loops}"
        for p, a, b in zip(["x", "adj", "rank2"], single, got):
            b = torch.from_numpy(b)
            print(f"{tag} {p}: 2 ranks vs single process, max abs diff {(a - b).abs().max().item():.3e} (scale {a.abs().max().item():.3e})")
            pc.assert_close(b, a, f"{tag}: 2-rank exact mode vs single process, {p}", rtol=2e-6)


# ---- one rank over RCCL, in a process of its own -----------------------------------------------------------------------------------
QM9_MIX = [9, 9, 8, 9, 7, 9, 9, 6, 9, 5, 9, 9, 4, 9, 8, 9, 3, 9, 7, 2, 9, 1]
CS_MIX = [12] * 29 + [14] * 14 + [16] * 23 + [18] * 25 + [20] * 9
RCCL_SETTINGS = [("ccsd_qm9_CC", 1024, 8, QM9_MIX, dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=1)),
                 ("ccsd_community_small_CC", 512, 2, CS_MIX, dict(predictor="Euler", corrector="Langevin", snr=0.05, scale_eps=0.7, n_steps=1))]


def seam_closures(name, B, steps, module, device, lib=None, seed=3):
    """(sharded exact closure, plain closure, models, cfg) of a shipped checkpoint through the drop-in seam."""
    from ccsd_amd import distributed

    meta, parts = load_ckpt_np(name)
    data = dict(meta["config"]["data"])
    # (the batch of non-molecule datasets is data.batch_size, of QM9 / ZINC250k sample.n_samples: loader.load_sampling_fn)
    data["batch_size"] = B
    cfgt = loader.AttrDict(dict(meta["config"], data=data))
    sample = dict(n_samples=B, probability_flow=False, noise_removal=True, eps=1e-4)
    names = ["x", "adj", "rank2"]
    ms = [loader.load_model_from_ckpt(meta[f"params_{p}"], parts[p], device) for p in names]
    kw = dict(is_cc=True, d_min=data["d_min"], d_max=data["d_max"], rng="philox", seed=seed, max_steps=steps)
    if lib is not None:
        kw["lib"] = lib
    sharded = distributed.load_sampling_fn_sharded(cfgt, module, sample, device, exact=True, **kw)
    plain = loader.load_sampling_fn(cfgt, module, sample, device, **kw)
    return sharded, plain, ms, data


def rccl_child():
    """Runs in a fresh process: a forced 1-rank RCCL group; load_sampling_fn_sharded(exact=True) must equal the plain closure bit
    for bit and take the library loop.  Prints one JSON line."""
    import torch.distributed as dist

    from ccsd_amd import distributed

    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("LOCAL_RANK", "0")
    rank, world, dev = distributed.init(force_group=True, timeout_s=120)
    out = {"backend": dist.get_backend(), "cases": []}
    try:
        assert (rank, world) == (0, 1) and dev.startswith("cuda") and dist.get_backend() == "nccl"
        for name, B, steps, mix, module in RCCL_SETTINGS:
            sharded, plain, ms, data = seam_closures(name, B, steps, module, dev)
            assert hasattr(sharded, "inner"), "the 1-rank group did not take the sharded route"
            flags = make_flags(B, data["max_node_num"], mix).to(dev)
            a, b = sharded(*ms, flags), plain(*ms, flags)
            torch.cuda.synchronize()
            equal = all(bool(torch.equal(u, v)) and bool(torch.isfinite(u).all()) for u, v in zip(a[:3], b[:3]))
            out["cases"].append({"name": name, "B": B, "steps": steps, "equal": equal, "exact_loop": sharded.inner.last_loop,
                                 "plain_loop": plain.last_loop})
    finally:
        dist.destroy_process_group()
    print(json.dumps(out), flush=True)


def case_rccl_single_rank_child(timeout_s=420):
    """Start rccl_child in a process of its own (the pytest process may own a group already), under a timeout."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.library_loop_cases", "rccl-child"]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout_s)
    assert p.returncode == 0, f"the RCCL child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, p.stdout[-2000:]
    out = json.loads(lines[-1])
    assert out["backend"] == "nccl" and len(out["cases"]) == len(RCCL_SETTINGS)
    for c in out["cases"]:
        assert c["exact_loop"] == "library" and c["plain_loop"] == "library", c
        assert c["equal"], f"1-rank exact mode over RCCL != the plain closure: {c}"


if __name__ == "__main__":
    if sys.argv[1:] == ["rccl-child"]:
        rccl_child()
    else:
        raise SystemExit("usage: python -m tests.library_loop_cases rccl-child")
