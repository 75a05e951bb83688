"""CPU suite for the lifting of graphs to combinatorial complexes (ccsd_lift, SampleOps.lift, evaluation.lift_settings, the lift= paths
of describe, eval_CC_batch and Sampler.evaluate) over the host emulation of k_lift_paths, k_lift_cycles and k_lift_dense: every output
exact against the plain Python restatement of tests/lift_ref.py and against the reference's own lifting (tests/golden/e5_lift.npz), the
restatement's cycle walk against networkx itself where networkx is installed."""
import itertools

import numpy as np
import pytest

from tests import lift_cases as lc
from tests import lift_ref as lr
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_restated_cycle_walk_is_networkx_cycle_basis():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(2026)
    seen = 0
    for t in range(300):
        N = int(rng.integers(5, 41))
        u = np.triu(rng.random((N, N)) < rng.choice([0.05, 0.1, 0.2, 0.4]), 1)
        A = u | u.T
        want = nx.cycle_basis(nx.from_numpy_array(A.astype(np.int64)))
        assert lr.cycle_basis(A) == want, (t, N)
        assert len(want) == lr.cyclomatic(A)
        seen += len(want)
    assert seen > 1000


def test_restated_path_rule_closed_forms():
    """get_all_paths_from_nodes restated with sets against the two closed forms the kernel uses: a middle node adjacent to the other two
    with a source among those two; with every node a source, at least 2 of the 3 pairs."""
    rng = np.random.default_rng(7)
    for t in range(60):
        N = int(rng.integers(3, 11))
        u = np.triu(rng.random((N, N)) < rng.choice([0.2, 0.5, 0.9]), 1)
        A = u | u.T
        for src in (None, [], [0], [N - 1, 1], list(range(0, N, 2))):
            S = set(range(N)) if src is None else set(src)
            want = {frozenset(c) for c in itertools.combinations(range(N), 3)
                    if any(A[m, a] and A[m, b] and (a in S or b in S) for m, a, b in ((c[0], c[1], c[2]), (c[1], c[0], c[2]), (c[2], c[0], c[1])))}
            assert lr.path_cells(A, src) == want, (t, src)


def test_restated_column_rank_is_the_enumeration():
    for N, d_min, d_max in ((5, 3, 5), (9, 3, 5), (7, 1, 7), (12, 3, 4)):
        col = lr.columns(N, d_min, d_max)
        assert len(col) == lr.n_columns(N, d_min, d_max)
        assert all(lr.column_of(c, N, d_min) == k for c, k in col.items())


def test_golden_holds_the_reference_lifting():
    z, meta = lc.e5()
    assert set(meta["sets"]) == {"n12", "n20"}
    for name, info in meta["sets"].items():
        for side in ("ref", "pred"):
            adj = z[f"{name}/{side}/adj"]
            assert adj.shape == (24, info["N"], info["N"]) and z[f"{name}/{side}/bits"].shape == (24, (info["K"] + 63) // 64)
            # the restatement reproduces the reference bit for bit, without any kernel
            want = lr.lift(adj, "path_based", info["d_min"], info["d_max"])
            assert np.array_equal(want["rank2_cell_bits"], z[f"{name}/{side}/bits"]) and np.array_equal(want["rank2_nnz"], z[f"{name}/{side}/nnz"])
            assert np.array_equal(want["rank2_cell_hist"], z[f"{name}/{side}/hist"])


@pytest.mark.parametrize("case", lc.PATH_CASES, ids=str)
def test_emu_paths_against_the_restatement(lib, case):
    lc.case_paths(lib, DEV, case)


@pytest.mark.parametrize("name", ["n12", "n20"])
def test_emu_paths_against_the_reference(lib, name):
    lc.case_golden_paths(lib, DEV, name)


@pytest.mark.parametrize("name", ["n12", "n20"])
def test_emu_lifted_scores_against_the_reference(lib, name):
    lc.case_golden_scores(lib, DEV, name)


@pytest.mark.parametrize("key", list(lc.special_graphs()) + lc.CYCLE_RANDOM, ids=str)
def test_emu_cycles_against_the_restatement(lib, key):
    lc.case_cycles(lib, DEV, key)


@pytest.mark.parametrize("case", lc.DENSE_CASES, ids=str)
def test_emu_dense_output_and_finish_round_trip(lib, case):
    lc.case_dense(lib, DEV, case)


def test_emu_lift_overwrites_its_outputs(lib):
    lc.case_overwrite(lib, DEV)


def test_emu_lift_quantiser_and_upper_triangle(lib):
    lc.case_quantiser(lib, DEV)


def test_emu_lift_bad_arguments(lib):
    lc.case_bad_args(lib, DEV)


def test_emu_lift_is_opt_in(lib):
    lc.case_opt_in(lib, DEV)


def test_emu_sampler_evaluate_lifts_the_held_out_graphs(lib, tmp_path):
    lc.case_sampler_evaluate_cc(lib, tmp_path)


def test_emu_graph_sampler_evaluate_with_lift(lib, tmp_path):
    lc.case_sampler_evaluate_graph(lib, tmp_path)
