"""GPU suite (-m gpu) for the spectral scores on the MI355X: the cases of tests/test_spectrum.py on k_eigvalsh, k_norm_laplacian and
k_hodge_laplacian themselves, plus the largest matrix the solver takes."""
import pytest

from tests import spectrum_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from ccsd_amd import _lib
    return _lib.get_library()


@pytest.mark.parametrize("n", sc.SOLVER_SIZES)
def test_solver_against_numpy(lib, n):
    sc.case_solver(lib, DEV, n)


def test_solver_largest_size(lib):
    sc.case_solver(lib, DEV, 512, B=2)


def test_solver_overflow_trap(lib):
    sc.case_solver_trap(lib, DEV)


def test_solver_walks_the_batch(lib):
    sc.case_solver_batch_walk(lib, DEV)


def test_spectral_above_the_lds_size(lib):
    sc.case_spectral_above_lds(lib, DEV)


def test_solver_bad_dims(lib):
    sc.case_solver_bad_dims(lib, DEV)


@pytest.mark.parametrize("name", ["r65", "diag12", "n125", "s12a", "s12b"])
def test_spectral_hist(lib, name):
    sc.case_spectral(lib, DEV, name)


def test_spectral_mol9(lib):
    sc.case_spectral_mol9(lib, DEV)


def test_spectral_bipartite_landmarks(lib):
    sc.case_spectral_landmarks(lib, DEV)


def test_spectral_small_graphs(lib):
    sc.case_spectral_small(lib, DEV)


def test_spectral_bad_dims(lib):
    sc.case_spectral_bad_dims(lib, DEV)


@pytest.mark.parametrize("name", ["e10", "e36", "e66", "e190"])
def test_hodge_spectrum(lib, name):
    sc.case_hodge(lib, DEV, name)


def test_hodge_small_complexes(lib):
    sc.case_hodge_small(lib, DEV)


def test_hodge_too_large(lib):
    sc.case_hodge_too_large(lib, DEV)


def test_spectral_scores(lib):
    sc.case_spectral_scores(lib, DEV)


@pytest.mark.parametrize("name", ["e10", "e36", "e66", "e190"])
def test_hodge_scores(lib, name):
    sc.case_hodge_scores(lib, DEV, name)


def test_spectra_are_opt_in(lib):
    sc.case_opt_in(lib, DEV)


def test_sampler_evaluate_with_spectra(lib, tmp_path):
    import os

    from tests.test_harness import QM9_CC_YAML, run_harness

    out, c = run_harness(tmp_path, lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=6)
    (fname,) = os.listdir(tmp_path / "samples")
    sc.case_sampler_evaluate(out, c.sampler, str(tmp_path / "samples" / fname))
