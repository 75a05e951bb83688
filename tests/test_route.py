"""CPU suite: the route of every shipped configuration -- which kernels its plan selects -- pinned against committed fixtures.

tests/golden/route_plans.json (tools/route_fixture.py --write) holds, for every checkpoint under ccsd_amd/checkpoints/ and
tests/golden/ckpt/ at its shipped sampler and batch and under every plan-shaping switch the suites set, the eight original plan
queries and the workspace sizes as the library reported them BEFORE routing moved into resolve_route(): a change that moves any plan
fails here.  tests/golden/route_expected.json (written by hand from the measured kernel lists and the rules of the commit before) pins the route
fields behind the appended query codes in all 18 x 10 cells; the host emulation resolves them exactly as the product does."""
import json
import os
import sys

import pytest

from ccsd_amd import _lib
from tests.emu_util import emu_library
from tests.helpers import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import route_fixture as rf  # noqa: E402

with open(rf.FIXTURE) as _f:
    PLANS = json.load(_f)
with open(os.path.join(GOLDEN, "route_expected.json")) as _f:
    EXPECTED = {k: v for k, v in json.load(_f).items() if not k.startswith("_")}
# the appended query codes: every one of them is asserted in every (checkpoint, switch) cell
ROUTE_KEYS = ["r2_family", "r2_instance", "loop_form", "h_full", "hp_full", "p0_narrow", "tiled_fuse", "ew1_fuse", "h_general", "geo_ek"]


def expected_route(name, switch):
    """The hand-written row of a cell: the checkpoint's base row, updated with what it lists for the switch."""
    want = dict(EXPECTED[name]["base"])
    want.update({k: v for k, v in EXPECTED[name]["switches"].get(switch, {}).items() if not k.startswith("_")})
    return want


@pytest.fixture(scope="module")
def lib():
    return emu_library()


@pytest.fixture(scope="module")
def cases():
    cache = {}
    return lambda name: cache.setdefault(name, rf.Case(name))


def test_fixtures_cover_every_checkpoint_and_switch():
    assert sorted(PLANS) == rf.checkpoints() == sorted(EXPECTED)
    for name, by_switch in PLANS.items():
        assert sorted(by_switch) == sorted(rf.SWITCHES), name
        assert sorted(EXPECTED[name]["base"]) == sorted(ROUTE_KEYS), name
        for switch, delta in EXPECTED[name]["switches"].items():
            assert switch in rf.SWITCHES and switch and set(delta) - {"_source"} <= set(ROUTE_KEYS) and delta["_source"], (name, switch)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plans_did_not_move(lib, cases, name):
    """Queries 0 .. 7 and ccsd_workspace_bytes at B in {1, batch, 2 * batch} (or the same failure of plan creation) under every switch."""
    for switch in rf.SWITCHES:
        assert rf.record(cases(name), lib, switch) == PLANS[name][switch], (name, switch)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_route_of_shipped_configuration(lib, cases, name):
    """All ten appended codes, unswitched and under every switch, against the hand-written rows."""
    for switch in rf.SWITCHES:
        eng = cases(name).engine(lib, switch)
        got = {k: rf.query(eng, lib, _lib.QUERIES[k]) for k in ROUTE_KEYS}
        assert got == expected_route(name, switch), (name, switch, EXPECTED[name]["switches"].get(switch, EXPECTED[name])["_source"])


def test_route_fixture_leaves_the_environment_alone(lib, cases, monkeypatch):
    """An inherited switch neither leaks into a plan nor is lost by creating one."""
    monkeypatch.setenv("CCSD_NO_BAKE", "1")
    assert rf.query(cases("ccsd_qm9_CC").engine(lib, ""), lib, _lib.QUERIES["xa_variant"]) == 7
    assert os.environ["CCSD_NO_BAKE"] == "1"


def test_headline_routes(lib, cases):
    """The anchors a reader should recognise, spelled out."""
    q = lambda name, what, switch="": rf.query(cases(name).engine(lib, switch), lib, _lib.QUERIES[what])
    assert q("ccsd_qm9_CC", "xa_variant") == 7 and q("ccsd_qm9_CC", "r2_instance") == 31102 and q("ccsd_qm9_CC", "merged_r2") == 1
    assert q("ccsd_qm9_CC", "xa_variant", "CCSD_NO_BAKE=1") == 4 and q("ccsd_qm9_CC", "xa_variant", "CCSD_NO_GEO=1") == 0
    assert q("ccsd_community_small_CC", "xa_variant") == 8 and q("ccsd_community_small_CC", "hp_full") == 1
    assert q("zinc250k_CC_5b", "r2_family") == 2 and q("ccsd_enzymes_small_CC", "xa_variant") == 10
    assert q("ccsd_enzymes_small_CC", "xa_variant", "CCSD_NO_BAKE=1") == 3 and q("ccsd_enzymes_small_CC", "loop_form") == 3
