"""The C-ABI library: loads without a GPU, exports every symbol include/ccsd_hip.h declares, and its
host-only entry points (config validation, sizes) behave.  No compute calls here."""
import ctypes as C
import os
import re

import pytest

from ccsd_amd import _lib, plan
from tests.helpers import ROOT, load_ckpt_np


def header_functions():
    src = open(os.path.join(ROOT, "include", "ccsd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ccsd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _lib.get_library()


def test_exports_match_header(lib):
    names = header_functions()
    assert names, "no functions parsed from the header"
    for n in names:
        assert hasattr(lib.c, n), f"libccsd_hip.so does not export {n}"
    assert set(names) == set(_lib.EXPORTS), (set(names) ^ set(_lib.EXPORTS))


def test_weight_count_and_dims_host_only(lib):
    meta, parts = load_ckpt_np("ccsd_qm9_CC")
    cfg = plan.make_config(meta["params_x"], meta["params_adj"], meta["params_rank2"], predictor="Reverse",
                           corrector="Langevin", snr=0.2, scale_eps=0.7, diff_steps=1000)
    blob = plan.pack_weights(meta["params_x"], parts["x"], meta["params_adj"], parts["adj"], meta["params_rank2"], parts["rank2"])
    assert lib.ccsd_weight_count(C.byref(cfg)) == blob.size == 42764      # 42,764 parameters
    E, K = C.c_int32(), C.c_int64()
    lib.ccsd_rank2_dims(C.byref(cfg), C.byref(E), C.byref(K))
    assert (E.value, K.value) == (36, 466)
    meta, parts = load_ckpt_np("ccsd_community_small_CC")
    cfg = plan.make_config(meta["params_x"], meta["params_adj"], meta["params_rank2"])
    assert lib.ccsd_weight_count(C.byref(cfg)) == 228764
    lib.ccsd_rank2_dims(C.byref(cfg), C.byref(E), C.byref(K))
    assert (E.value, K.value) == (190, 1140)


def test_invalid_configs_are_rejected(lib):
    meta, _ = load_ckpt_np("ccsd_qm9_CC")
    cfg = plan.make_config(meta["params_x"], meta["params_adj"], meta["params_rank2"])
    cfg.abi_version = 99
    assert lib.ccsd_weight_count(C.byref(cfg)) == 0
    assert b"abi_version" in lib.ccsd_last_error()
    cfg = plan.make_config(meta["params_x"], dict(meta["params_adj"], num_layers_h=9), meta["params_rank2"])
    assert lib.ccsd_weight_count(C.byref(cfg)) == 0           # 9 hodge layers: outside the HIP envelope (1..8 are built)
    assert b"HodgeAdjAttentionLayers" in lib.ccsd_last_error()
    cfg = plan.make_config(meta["params_x"], dict(meta["params_adj"], num_layers_h=3), meta["params_rank2"])
    assert lib.ccsd_weight_count(C.byref(cfg)) > 0
    cfg = plan.make_config(meta["params_x"], dict(meta["params_adj"], num_layers_h=3, num_linears_h=2), meta["params_rank2"])
    assert lib.ccsd_weight_count(C.byref(cfg)) > 0            # (true-MLP mlp_value behind dense hodge layers: the general hodge stack)
    # use_bn / conv_hodge="MLP": the reference's own forward fails on these shapes, with these exception types
    with pytest.raises(RuntimeError, match="running_mean should contain 9 elements not 48"):
        plan.make_config(dict(meta["params_x"], use_bn=True), meta["params_adj"], meta["params_rank2"])
    with pytest.raises(RuntimeError, match="mat1 and mat2 shapes cannot be multiplied"):
        plan.make_config(meta["params_x"], dict(meta["params_adj"], conv_hodge="MLP"), meta["params_rank2"])
    with pytest.raises(NotImplementedError):
        plan.make_config(meta["params_x"], dict(meta["params_adj"], conv_hodge="GAT"), meta["params_rank2"])
    # ... while use_bn on a network whose MLPs are single Linears creates no BatchNorm at all (layers.py:205-224): it runs
    assert plan.make_config(meta["params_x"], meta["params_adj"], dict(meta["params_rank2"], use_bn=True)).f_num_linears == 1
    with pytest.raises(NotImplementedError):
        plan.make_config(meta["params_x"], dict(meta["params_adj"], conv="GAT"), meta["params_rank2"])
    assert plan.make_config(meta["params_x"], dict(meta["params_adj"], conv="MLP"), meta["params_rank2"]).a_conv_mlp == 1
    with pytest.raises(NotImplementedError):
        plan.make_config(meta["params_x"], meta["params_adj"], meta["params_rank2"], predictor="Heun")


def test_product_path_has_no_cpu_fallback():
    """Without a GPU the engine must refuse to run rather than fall back to anything."""
    import torch

    from ccsd_amd.engine import PCEngine

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    meta, parts = load_ckpt_np("gdss_community_small")
    with pytest.raises(_lib.CcsdError):
        PCEngine(meta["params_x"], parts["x"], meta["params_adj"], parts["adj"], None, None, N=20, F=10, is_cc=False, device="cpu")
    with pytest.raises(_lib.CcsdError):
        PCEngine(meta["params_x"], parts["x"], meta["params_adj"], parts["adj"], None, None, N=20, F=10, is_cc=False, device="cuda")


def test_pack_weights_errors():
    meta, parts = load_ckpt_np("ccsd_qm9_CC")
    bad = dict(parts["x"])
    bad.pop("final.linears.0.bias")
    with pytest.raises(ValueError):
        plan.pack_weights(meta["params_x"], bad, meta["params_adj"], parts["adj"], meta["params_rank2"], parts["rank2"])


def test_unshipped_switches_fail_like_the_reference():
    """use_bn=True and conv_hodge="MLP": tests/golden/reference_variant_status.json holds what the REFERENCE's forward does for a
    set of configurations (captured by tools/make_golden.py): the product raises the same exception type with the same
    message where the reference raises, and says NotImplementedError for the two degenerate shapes on which the reference's
    code happens to type-check (N == hidden width; E == K)."""
    import json

    st = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_variant_status.json")))
    nodes = {"bn_x_N5_hidden22": 5, "bn_x_N8_hidden8": 8, "bn_x_gmh": 8}
    assert len(st) >= 8
    for tag, v in st.items():
        p = v["params"]
        err = plan.reference_forward_error(p, p.get("max_node_num") or nodes[tag], 2)
        if v["result"] == "error":
            assert type(err).__name__ == v["type"] and str(err) == v["message"], (tag, err, v)
        else:
            assert isinstance(err, NotImplementedError), (tag, err)
    # the model containers construct (as the reference's modules do) and fail at the first forward / sampler build
    from ccsd_amd import loader

    m = loader.load_model(dict(st["bn_f"]["params"]))
    assert m.params["use_bn"] is True


# The four workspace sizes of the plan-free entry points: ((arguments), bytes, ccsd_last_error of a refused size).  The literals were
# RECORDED from the emulation library of the commit before these entry points moved to ccsd_api_samples.h -- not computed by the code under
# test: the layouts must stay byte for byte.  n = 128 | 129 lie on the two sides of CCSD_EIG_LDS_MAXN (E = 120 | 136 for N = 16 | 17), and
# B = 3 is above the emulation's slab grid (CCSD_EIG_MAX_GRID = 2 there), where the slabs stop growing with B.
_EIG_ERR = "ccsd_eig_workspace_bytes: B must be >= 1 and n in 1..512"
_MMD_ERR = "ccsd_mmd_workspace_bytes: n1, n2 must be in 1..1048576 and L in 1..65536"
_SPECTRAL_ERR = "ccsd_spectral_workspace_bytes: B must be >= 1 and N in 2..512"
_HODGE_ERR = "ccsd_hodge_workspace_bytes: B must be >= 1 and N >= 2"
WORKSPACE_BYTES = {
    "ccsd_mmd_workspace_bytes": [
        ((1, 1, 1), 2072, None), ((3, 2, 5), 6168, None), ((64, 65, 10), 16952, None), ((200, 130, 100), 362280, None),
        ((0, 3, 5), 0, _MMD_ERR), ((3, 3, 0), 0, _MMD_ERR), ((1048577, 1, 1), 0, _MMD_ERR), ((1, 1, 65537), 0, _MMD_ERR),
    ],
    "ccsd_eig_workspace_bytes": [
        ((1, 1), 0, None), ((5, 128), 0, None), ((1, 129), 133128, None), ((2, 129), 266256, None), ((3, 129), 266256, None),
        ((7, 512), 4202496, None), ((0, 4), 0, _EIG_ERR), ((1, 0), 0, _EIG_ERR), ((1, 513), 0, _EIG_ERR),
    ],
    "ccsd_spectral_workspace_bytes": [
        ((1, 2), 56, None), ((3, 5), 736, None), ((4, 128), 528400, None), ((1, 129), 267296, None), ((3, 129), 668752, None),
        ((5, 512), 14708760, None), ((0, 5), 0, _SPECTRAL_ERR), ((1, 1), 0, _SPECTRAL_ERR), ((1, 513), 0, _SPECTRAL_ERR),
    ],
    "ccsd_hodge_workspace_bytes": [
        ((1, 2), 8, None), ((3, 5), 2400, None), ((2, 16), 230400, None), ((1, 17), 297024, None), ((3, 17), 742016, None),
        ((2, 32), 7880448, None), ((0, 5), 0, _HODGE_ERR), ((1, 1), 0, _HODGE_ERR),
        ((1, 33), 0, "ccsd_hodge_workspace_bytes: N = 33: E = N (N - 1) / 2 = 528 is above CCSD_EIG_MAXN = 512: the solver is a Jacobi iteration "
                     "of O(n^3) per sweep with one matrix per compute unit, which larger matrices are out of reach of"),
    ],
}


@pytest.mark.parametrize("fn", list(WORKSPACE_BYTES))
def test_emu_workspace_bytes_are_the_recorded_ones(fn):
    from tests.emu_util import emu_library

    emu = emu_library()
    for args, want, err in WORKSPACE_BYTES[fn]:
        assert getattr(emu, fn)(*args) == want, (fn, args)
        if err is not None:
            assert emu.ccsd_last_error().decode() == err, (fn, args)


def _ckpt_engine(name, **kw):
    from tests import parity_cases as pc

    return lambda lib: pc.engine_from_ckpt(name, lib, "cpu", **kw)[0]


def _zinc5b_engine(lib):
    """The N = 38 substitute of test_zinc5b_substitute (tests/parity_cases.py::zinc5b_setup), without its inputs."""
    import json

    import torch

    from ccsd_amd.engine import PCEngine
    from tests.helpers import load_golden

    g = load_golden("kat_zinc250k_CC_5b.npz")
    meta = json.loads(str(g["meta"]))
    sd = {tag: {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/w/")} for tag in ("x", "adj", "rank2")}
    N, Fd, d_min, d_max, _, _ = meta["dims"]
    pm = meta["params"]
    return PCEngine(pm["x"], sd["x"], pm["adj"], sd["adj"], pm["rank2"], sd["rank2"], N=N, F=Fd, is_cc=True, d_min=d_min, d_max=d_max,
                    device="cpu", lib=lib)


def _kat_general_engine(tag):
    def make(lib):
        import json

        import torch

        from tests import hodge_wide_cases as hw
        from tests.helpers import load_golden

        g = load_golden("kat_hodge_general.npz")
        sd = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/w/")}
        return hw.kat_engine(json.loads(str(g["meta"]))[tag], sd, lib, "cpu")
    return make


def _kat_wide_engine(tag):
    def make(lib):
        from tests import hodge_wide_cases as hw

        return hw.kat_engine(*hw.kat_tag(tag)[:2], lib, "cpu")
    return make


# ccsd_workspace_bytes(plan, B) at B = 1 and B = 5, one plan per branch of the workspace carve-up (carve_ws, ccsd_amd/csrc/ccsd_api.h):
# name -> (engine maker, environment at plan creation, the route queries that name the branch, (bytes at B = 1, bytes at B = 5)).  The
# literals were RECORDED from the emulation library of the commit before every entry point's prologue began to carve once per call -- not
# computed by the code under test: the layout must stay byte for byte.  The queries are asserted first, so that a route switch left in the
# caller's environment fails by naming the branch the plan took, not by a bare byte count.
PLAN_WORKSPACE_BYTES = {
    "ccsd_qm9_CC": (_ckpt_engine("ccsd_qm9_CC"), {}, dict(r2_family=1, large_graph=0), (127744, 626944)),                                   # fused family: second projection set
    "ccsd_enzymes_small_CC": (_ckpt_engine("ccsd_enzymes_small_CC"), {}, dict(r2_family=3, large_graph=0), (293120, 1453824)),              # tiled family, K slices of P_1
    "ccsd_community_small_CC": (_ckpt_engine("ccsd_community_small_CC"), {}, dict(r2_family=3, large_graph=0), (1099776, 5490944)),
    "zinc5b substitute": (_zinc5b_engine, {}, dict(r2_family=2, ew1=1), (25814528, 129064960)),                                     # k_ew1
    "ccsd_qm9_Base_CC": (_ckpt_engine("ccsd_qm9_Base_CC"), {}, dict(r2_family=1, large_graph=0), (76032, 370432)),
    "gdss_community_small": (_ckpt_engine("gdss_community_small"), {}, dict(r2_family=0, large_graph=0), (67072, 328960)),
    "kat_hodge_general G3_n5": (_kat_general_engine("G3_n5"), {}, dict(h_general=1, large_graph=0), (17152, 69376)),                        # general hodge stack on k_xa
    "kat_hodge_general G3_n5 on the route": (_kat_general_engine("G3_n5"), {"CCSD_LARGE_GRAPH": "2"}, dict(h_general=1, large_graph=1), (23296, 92160)),
    "kat_hodge_wide W3_n12": (_kat_wide_engine("W3_n12"), {}, dict(h_wide=1, h_general=1, large_graph=1), (996608, 4960512)),                         # wide hodge MLPs (route, general stack)
    "gdss_enzymes": (_ckpt_engine("gdss_enzymes"), {}, dict(r2_family=0, large_graph=1), (4950528, 24739840)),                              # N = 125: graph-only route
    # the third state buffer of a Langevin corrector with two inner iterations
    "ccsd_qm9_CC, n_steps = 2": (_ckpt_engine("ccsd_qm9_CC", predictor="Reverse", corrector="Langevin", snr=0.2, scale_eps=0.7, n_steps=2), {},
                                 dict(r2_family=1, loop_form=4),
                                 (195840, 965120)),
}


@pytest.mark.parametrize("name", list(PLAN_WORKSPACE_BYTES))
def test_emu_plan_workspace_bytes_are_the_recorded_ones(name, monkeypatch):
    from tests.emu_util import emu_library

    emu = emu_library()
    make, env, route, want = PLAN_WORKSPACE_BYTES[name]
    monkeypatch.delenv("CCSD_LARGE_GRAPH", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = make(emu)
    assert {q: eng.query(q) for q in route} == route, name
    assert (emu.ccsd_workspace_bytes(eng.handle, 1), emu.ccsd_workspace_bytes(eng.handle, 5)) == want, name

