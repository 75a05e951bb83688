#!/usr/bin/env python
"""Rate of the exact multi-GPU mode on ONE rank: what the reduce hook of the library loop costs, and what it saves.

Workload: bench.py's (qm9_CC, B = 1024, the shipped sampler, 1000 steps per call).  Three closures are timed, each after a
warm-up call of the same shape, with a host clock around a device synchronise:

  independent       loader.load_sampling_fn                           (per-shard norms; what bench.py times)
  exact             distributed.load_sampling_fn_sharded(exact=True)  on a forced 1-rank RCCL group: one all-reduce of the six
                                                                      Langevin norm sums per norms pass
  exact_stepwise    the same closure with the Python-driven step-wise driver forced (pc_sampler.force_stepwise)

One JSON line on stdout: the three rates (samples * steps / s), the time per step, and the loop each closure took
(`last_loop`).  No GPU: exit status 2, nothing is measured.  One rank only: more than one rank is not measured by this tool.

  python tools/bench_exact.py [--steps 1000] [--batch 1024] [--reps 1] [--root DIR] [--label NAME]

--root: the repository tree whose ccsd_amd is measured (default: the one this file lives in), for A/B runs against a
checkout of another commit; a tree without `last_loop` / `force_stepwise` reports null and ignores the forcing.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=1, help="timed calls per closure (interleaved); the median is reported")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    os.chdir(root)

    import torch

    if not torch.cuda.is_available():
        print("bench_exact.py: no GPU visible -- nothing measured", file=sys.stderr)
        return 2
    import __graft_entry__ as ge

    ge.build()
    import bench
    import torch.distributed as dist
    from ccsd_amd import distributed, loader

    assert os.path.dirname(os.path.abspath(loader.__file__)) == os.path.join(root, "ccsd_amd"), loader.__file__
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("LOCAL_RANK", "0")
    rank, world, dev = distributed.init(force_group=True, timeout_s=300)
    if world != 1:
        raise SystemExit("bench_exact.py measures one rank")
    wname = "qm9_CC"
    wl = bench.WORKLOADS[wname]
    ck, names, is_cc = bench.load_workload(wname, dev)
    cfgt = ck["config"]
    data = cfgt["data"]
    B, steps = args.batch, args.steps
    data["batch_size"] = B
    models = [loader.load_model_from_ckpt(ck[f"params_{p}"], ck[f"{p}_state_dict"], dev) for p in names]
    module = dict(predictor=wl["predictor"], corrector=wl["corrector"], snr=wl["snr"], scale_eps=wl["scale_eps"], n_steps=1)
    sample = dict(n_samples=B, probability_flow=False, noise_removal=True, eps=1e-4)
    kw = dict(is_cc=is_cc, d_min=data["d_min"], d_max=data["d_max"], rng="philox", seed=42, max_steps=steps)
    flags = bench.hist_flags(B, data["max_node_num"], wl["hist"]).to(dev)

    def exact_closure(force_stepwise):
        fn = distributed.load_sampling_fn_sharded(cfgt, module, sample, dev, exact=True, **kw)
        assert hasattr(fn, "inner"), "the 1-rank group did not take the sharded route"
        if force_stepwise:
            fn.inner.force_stepwise = True
        return fn, fn.inner

    plain = loader.load_sampling_fn(cfgt, module, sample, dev, **kw)
    closures = {"independent": (plain, plain), "exact": exact_closure(False), "exact_stepwise": exact_closure(True)}
    times = {k: [] for k in closures}
    outs = {}
    try:
        for k, (fn, inner) in closures.items():          # warm-up of the same shape (the first call also builds the plan)
            outs[k] = fn(*models, flags)
            torch.cuda.synchronize()
        for _ in range(max(1, args.reps)):
            for k, (fn, inner) in closures.items():
                inner.calls = 0                          # (every timed call draws the warm-up's stream: the same work)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(*models, flags)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
    finally:
        dist.destroy_process_group()
    res = {"tool": "bench_exact", "label": args.label, "workload": wname, "B": B, "steps": steps, "ranks": 1,
           "note": "1 rank; more than one rank not measured", "device": torch.cuda.get_device_name(0), "backend": "nccl"}
    for k, (fn, inner) in closures.items():
        t = sorted(times[k])[len(times[k]) // 2]
        res[k] = {"samples_steps_per_s": B * steps / t, "ms_per_step": 1e3 * t / steps, "seconds": times[k],
                  "last_loop": getattr(inner, "last_loop", None)}
    # 1 rank: the all-reduce is the identity, so the three closures must have produced the same samples
    res["exact_equals_independent"] = all(bool(torch.equal(a, b)) for a, b in zip(outs["exact"][:3], outs["independent"][:3]))
    res["stepwise_equals_independent"] = all(bool(torch.equal(a, b)) for a, b in zip(outs["exact_stepwise"][:3], outs["independent"][:3]))
    res["exact_over_independent"] = res["exact"]["samples_steps_per_s"] / res["independent"]["samples_steps_per_s"]
    res["exact_over_stepwise"] = res["exact"]["samples_steps_per_s"] / res["exact_stepwise"]["samples_steps_per_s"]
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
