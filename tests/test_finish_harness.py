"""Sampler.sample() finishes through SampleOps.finish (one C call): every key it returned before keeps the value the three separate
calls -- quantize, quantize(...).to(uint8), rank2_cells -- give on the same tensors, the descriptors are new keys, and
dense_rank2=False drops exactly the dense incidence tensors.  CPU: over the host emulation, with the machinery of tests/test_harness.py."""
import os

import numpy as np
import torch

from tests.emu_util import emu_library
from tests.finish_cases import numpy_descriptors
from tests.helpers import sample_ops
from tests.test_harness import ENZYMES_YAML, QM9_CC_YAML, run_harness

OLD_MOL_CC = {"adj_int", "adj_onehot", "x_onehot", "rank2", "rank2_int", "rank2_cell_bits", "rank2_cell_count", "flags", "x", "adj",
              "sampling_time"}
NEW_GRAPH = {"n_nodes", "degree", "degree_hist", "edge_hist", "x_hist"}
NEW_CC = {"rank2_cell_hist", "rank2_nnz"}


def separate_calls(lib, out, mol):
    """What sample() computed before this feature, on the tensors it returned."""
    q = sample_ops(lib, "cpu")
    want = {}
    if mol:
        s = q.quantize(out["adj"], -1.0) - 1
        s[s == -1] = 3
        want["adj_int"] = s
        want["adj_onehot"] = torch.nn.functional.one_hot(s, num_classes=4).permute(0, 3, 1, 2)
        xi = torch.where(out["x"] > 0.5, 1, 0)
        want["x_onehot"] = torch.concat([xi, 1 - xi.sum(dim=-1, keepdim=True)], dim=-1)
    else:
        want["adj_int"] = q.quantize(out["adj"], 0.5)
    if "rank2" in out:
        want["rank2_int"] = q.quantize(out["rank2"], 0.5).to(torch.uint8)
        want["rank2_cell_bits"], want["rank2_cell_count"] = q.rank2_cells(out["rank2"], 0.5)
    return want


def test_sample_qm9_cc_keeps_old_keys_and_adds_descriptors(tmp_path):
    lib = emu_library()
    out, c = run_harness(tmp_path, lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=2)
    assert set(out) == OLD_MOL_CC | NEW_GRAPH | NEW_CC
    for k, w in separate_calls(lib, out, mol=True).items():
        assert out[k].dtype == w.dtype and torch.equal(out[k], w), k
    want = numpy_descriptors(out["x"], out["adj"], out["rank2"], 3, 9, mol=True)
    for k in NEW_GRAPH | NEW_CC:
        assert out[k].dtype == torch.int32 and np.array_equal(out[k].numpy(), want[k]), k
    assert int(out["rank2_cell_hist"].sum()) == int(out["rank2_cell_count"].sum())
    # the saved file holds every key
    (fname,) = os.listdir(tmp_path / "samples")
    with np.load(tmp_path / "samples" / fname) as z:
        assert set(z.files) == set(out)
        assert np.array_equal(z["degree_hist"], out["degree_hist"].numpy()) and np.array_equal(z["rank2_nnz"], out["rank2_nnz"].numpy())


def test_sample_dense_rank2_false_drops_exactly_the_dense_tensors(tmp_path):
    lib = emu_library()
    full, _ = run_harness(tmp_path / "a", lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=2)
    lean, _ = run_harness(tmp_path / "b", lib, None, "sample_qm9_CC", QM9_CC_YAML, max_steps=2, dense_rank2=False)
    assert set(full) - set(lean) == {"rank2", "rank2_int"} and set(lean) <= set(full)
    for k in lean:
        if k != "sampling_time":
            assert torch.equal(lean[k], full[k]), k
    (fname,) = os.listdir(tmp_path / "b" / "samples")
    with np.load(tmp_path / "b" / "samples" / fname) as z:
        assert set(z.files) == set(lean)


def test_sample_generic_cc_dataset(tmp_path):
    """Sampler_CC (quantize mode, S4 solver): the same through the generic-dataset loop."""
    lib = emu_library()
    out, c = run_harness(tmp_path, lib, None, "sample_enzymes_small_CC", ENZYMES_YAML, max_steps=1, rounds=1)
    assert set(out) == (OLD_MOL_CC - {"adj_onehot", "x_onehot"}) | NEW_GRAPH | NEW_CC
    for k, w in separate_calls(lib, out, mol=False).items():
        assert out[k].dtype == w.dtype and torch.equal(out[k], w), k
    want = numpy_descriptors(out["x"], out["adj"], out["rank2"], 3, 4, mol=False)
    for k in NEW_GRAPH | NEW_CC:
        assert np.array_equal(out[k].numpy(), want[k]), k
    assert out["edge_hist"][:, 2:].sum() == 0
