"""CPU side of the distribution check (tests/distribution_cases.py): the fixture itself, and the identical comparison applied to its
two halves (128 reference complexes against the other 128) -- the reference alone stays within the bound."""
import numpy as np

from tests import distribution_cases as dc


def test_fixture_is_one_full_reference_run():
    d, meta = dc.fixture()
    assert meta["B"] == 256 and meta["num_scales"] == 1000 and meta["checkpoint"].endswith("ccsd_qm9_CC.pth")
    assert meta["sampler"] == {"predictor": "Reverse", "corrector": "Langevin", "snr": 0.2, "scale_eps": 0.7, "n_steps": 1}
    assert meta["reference_run_seconds"] > 0
    assert d["flags"].shape == (256, 9) and d["degree_hist"].shape == (256, 9) and d["edge_hist"].shape == (256, 4)
    assert d["cell_hist"].shape == (256, 7) and d["x_hist"].shape == (256, 4)
    # flags drawn as the harness draws them: the recorded numpy seed reproduces them
    from ccsd_amd import sampler as S
    from ccsd_amd.loader import AttrDict
    import json

    with open(S._COUNTS) as f:
        hist = json.load(f)["QM9"]["test_histogram"]
    np.random.seed(meta["numpy_seed"])
    fl = S.init_flags(hist, AttrDict({"data": {"max_node_num": 9}}), 256, is_cc=True)
    assert np.array_equal(fl.numpy(), d["flags"])
    # masked slots carry nothing: no more nodes than flags, degree histogram over all nine slots
    assert (d["n_nodes"] <= d["flags"].sum(-1)).all() and (d["degree_hist"].sum(-1) <= 9).all()
    assert len(dc.scalars(d)) >= 15


def test_reference_halves_agree_within_the_bound(capsys):
    d, _ = dc.fixture()
    bins = dc.nonempty_bins(d)
    a = dc.scalars({k: v[:128] for k, v in d.items()}, bins)
    b = dc.scalars({k: v[128:] for k, v in d.items()}, bins)
    with capsys.disabled():
        dc.compare(a, b, "ref[:128] vs ref[128:]")
