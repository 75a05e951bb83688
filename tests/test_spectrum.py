"""CPU suite for the spectral scores (ccsd_eigvalsh, ccsd_spectral_hist, ccsd_hodge_spectrum, the spectra=True paths of
ccsd_amd/evaluation.py and Sampler.evaluate) over the host emulation of k_eigvalsh / k_norm_laplacian / k_hodge_laplacian: the solver
against numpy.linalg.eigvalsh, histogram counts bit-exact against the reference's spectral_worker (tests/golden/e2_spectrum.npz) and a
numpy restatement, hodge spectra against the reference's float32 spectra, and the scores against the reference's own."""
import numpy as np
import pytest

from tests import spectrum_cases as sc
from tests.emu_util import emu_library

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    return emu_library()


def test_fixture_records_its_checks():
    z, meta = sc.e2()
    assert meta["edge_margin_ok"] and meta["edge_margin_required"] == 1e-9
    exact = sc.exact_graph_sets()
    assert {"r65", "diag12", "n125", "s12a", "s12b"} <= set(exact) and "bip" not in exact
    assert all(meta["graph_sets"][k]["edge_margin"] >= 1e-9 and not meta["graph_sets"][k]["bipartite_component"] for k in exact)
    assert meta["graph_sets"]["n125"]["N"] == 125 and meta["graph_sets"]["mol9"]["mol"]
    assert sorted(v["E"] for v in meta["complex_sets"].values()) == [10, 36, 66, 190]
    assert set(k for k in meta["f32_vs_f64"] if k.endswith("/eig")) == {f"cc/{n}/eig" for n in meta["complex_sets"]}


@pytest.mark.parametrize("n", sc.SOLVER_SIZES)
def test_emu_solver_against_numpy(lib, n):
    sc.case_solver(lib, DEV, n)


def test_emu_solver_overflow_trap(lib):
    sc.case_solver_trap(lib, DEV)


def test_emu_solver_walks_the_batch(lib):
    sc.case_solver_batch_walk(lib, DEV)


def test_emu_spectral_above_the_lds_size(lib):
    sc.case_spectral_above_lds(lib, DEV)


def test_emu_solver_bad_dims(lib):
    sc.case_solver_bad_dims(lib, DEV)


@pytest.mark.parametrize("name", ["r65", "diag12", "n125", "s12a", "s12b"])
def test_emu_spectral_hist(lib, name):
    sc.case_spectral(lib, DEV, name)


def test_emu_spectral_mol9(lib):
    sc.case_spectral_mol9(lib, DEV)


def test_emu_spectral_bipartite_landmarks(lib):
    sc.case_spectral_landmarks(lib, DEV)


def test_emu_spectral_small_graphs(lib):
    sc.case_spectral_small(lib, DEV)


def test_emu_spectral_bad_dims(lib):
    sc.case_spectral_bad_dims(lib, DEV)


@pytest.mark.parametrize("name", ["e10", "e36", "e66", "e190"])
def test_emu_hodge_spectrum(lib, name):
    sc.case_hodge(lib, DEV, name)


def test_emu_hodge_small_complexes(lib):
    sc.case_hodge_small(lib, DEV)


def test_emu_hodge_too_large(lib):
    sc.case_hodge_too_large(lib, DEV)


def test_emu_spectral_scores(lib):
    sc.case_spectral_scores(lib, DEV)


@pytest.mark.parametrize("name", ["e10", "e36", "e66", "e190"])
def test_emu_hodge_scores(lib, name):
    sc.case_hodge_scores(lib, DEV, name)


def test_emu_spectra_are_opt_in(lib):
    sc.case_opt_in(lib, DEV)


def test_emu_sampler_evaluate_with_spectra(lib, tmp_path):
    import os

    from tests.test_harness import QM9_CC_YAML, run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=2)
    (fname,) = os.listdir(tmp_path / "samples")
    sc.case_sampler_evaluate(out, c.sampler, str(tmp_path / "samples" / fname))
