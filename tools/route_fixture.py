"""The plan of every shipped checkpoint, as the library reports it, under every plan-shaping switch the suites set.

    python tools/route_fixture.py [--write]     (CPU only: uses the host emulation of the kernel source, tests/emu)

For each checkpoint under ccsd_amd/checkpoints/ and tests/golden/ckpt/ -- at its shipped sampler settings and the batch of its bench
workload (bench.WORKLOADS) or of its training YAML (config.data.batch_size) -- and each entry of SWITCHES, one plan is created and
its eight original plan queries and ccsd_workspace_bytes at B in {1, batch, 2 * batch} are recorded; where a switch makes plan
creation fail, the exception type and message are recorded instead.  --write stores the records in tests/golden/route_plans.json;
tests/test_route.py compares the library against that file, so a change that moves any plan fails there.  The file is regenerated
only when a plan is MEANT to move (a planner change), never to make a routing refactor pass.

The route fields behind the appended query codes are pinned by tests/golden/route_expected.json, which is written by hand from the
kernel lists of profiles/ and README.md; this tool never touches it."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_plans.json")
# the eight query codes that exist on both sides of the route refactor (ccsd_hip.h: CCSD_QUERY_FUSED_R2 .. CCSD_QUERY_LARGE_GRAPH)
BASE_QUERIES = ["fused_r2", "xa_variant", "r2_lds_bytes", "xa_lds_bytes", "fused_loop", "merged_r2", "ew1", "large_graph"]
# every switch combination tests/ sets at plan creation ("" = none)
SWITCHES = ["", "CCSD_NO_FUSED_R2=1", "CCSD_XA_PASS=1", "CCSD_XA_PASS=2", "CCSD_NO_FUSED_APPLY=1", "CCSD_XA_GCH=1", "CCSD_NO_GEO=1",
            "CCSD_NO_BAKE=1", "CCSD_HODGE_GENERAL=1", "CCSD_LARGE_GRAPH=1"]
# checkpoints whose JSON carries no sampler section: the sampler of the dataset's sample_*.yaml (qm9: Reverse + Langevin)
DEFAULT_SAMPLER = dict(predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7)

import bench  # noqa: E402
from ccsd_amd import loader  # noqa: E402
from ccsd_amd.engine import PCEngine  # noqa: E402
from tests.helpers import CKPT, GOLDEN_CKPT, load_ckpt_np  # noqa: E402


def checkpoints():
    return sorted(f[:-5] for d in (CKPT, GOLDEN_CKPT) for f in os.listdir(d) if f.endswith(".json"))


def settings(name, meta):
    """(sampler keywords, batch) a checkpoint ships with: its bench workload when it has one, its own YAML otherwise."""
    for wl in bench.WORKLOADS.values():
        if wl["ckpt"] == name:
            return {k: wl[k] for k in ("predictor", "corrector", "snr", "scale_eps")}, wl["batch"]
    s = meta["config"].get("sampler")
    kw = {k: s[k] for k in ("predictor", "corrector", "snr", "scale_eps")} if s else dict(DEFAULT_SAMPLER)
    return kw, meta["config"]["data"]["batch_size"]


class Case:
    """One checkpoint, loaded once; engine(switch) creates its plan under a switch."""

    def __init__(self, name):
        self.name = name
        self.meta, self.parts = load_ckpt_np(name)
        self.sampler, self.batch = settings(name, self.meta)

    def engine(self, lib, switch=""):
        meta, parts, cfg, is_cc = self.meta, self.parts, self.meta["config"], self.meta["is_cc"]
        names = ["x", "adj"] + (["rank2"] if is_cc else [])
        sdes = [loader.load_sde(cfg["sde"][p]) for p in names]
        kw = dict(d_min=cfg["data"]["d_min"], d_max=cfg["data"]["d_max"]) if is_cc else {}
        # exactly this switch for the duration of plan creation: an inherited one is set aside, and put back afterwards
        keys = sorted({sw.partition("=")[0] for sw in SWITCHES if sw})
        saved = {k: os.environ.pop(k) for k in keys if k in os.environ}
        key, _, val = switch.partition("=")
        if key:
            os.environ[key] = val
        try:
            return PCEngine(meta["params_x"], parts["x"], meta["params_adj"], parts["adj"], meta.get("params_rank2") if is_cc else None,
                            parts.get("rank2") if is_cc else None, N=cfg["data"]["max_node_num"], F=cfg["data"]["max_feat_num"],
                            is_cc=is_cc, sdes=sdes, n_steps=1, denoise=True, eps=1e-4, device="cpu", batch_hint=self.batch, lib=lib,
                            **self.sampler, **kw)
        finally:
            os.environ.pop(key, None)
            os.environ.update(saved)


def query(eng, lib, what):
    v = C.c_int64(0)
    lib.check(lib.ccsd_plan_query(eng.handle, what, C.byref(v)))
    return v.value


def record(case, lib, switch):
    """{"batch", "query": {name: value}, "workspace": {B: bytes}} or {"batch", "error": [exception type, message]}."""
    from ccsd_amd import _lib
    try:
        eng = case.engine(lib, switch)
    except (ValueError, NotImplementedError, _lib.CcsdError) as e:
        return {"batch": case.batch, "error": [type(e).__name__, str(e)]}
    return {"batch": case.batch,
            "query": {q: query(eng, lib, _lib.QUERIES[q]) for q in BASE_QUERIES},
            "workspace": {str(B): int(lib.ccsd_workspace_bytes(eng.handle, B)) for B in (1, case.batch, 2 * case.batch)}}


def main():
    from tests.emu_util import emu_library
    lib = emu_library()
    out = {}
    for name in checkpoints():
        case = Case(name)
        out[name] = {sw: record(case, lib, sw) for sw in SWITCHES}
        base = out[name][""]
        print(name, case.sampler["predictor"], case.sampler["corrector"], "B =", case.batch, base.get("query", base.get("error")), flush=True)
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
