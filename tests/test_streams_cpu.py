"""What the stream tests rest on, checked without a GPU (tests/stream_cases.py): the inventory of workloads accounts for
every entry of include/icpmi.h and every class of icpmi/ with a ``run`` method; ``owned_tensors`` finds what it must;
``poison_`` leaves the byte patterns it promises; the workloads' inputs are deterministic."""
import ast
import glob
import os
import types

import numpy as np
import pytest

import stream_cases as sc
from conftest import PKG


def test_every_entry_of_the_header_is_reached_or_excluded_with_a_reason():
    from icpmi import _lib
    exports = set(_lib.EXPORTS)                                   # read from include/icpmi.h by icpmi/_header.py
    reached, excluded = set(sc.reached_entries()), set(sc.EXCLUDED_ENTRIES)
    assert reached <= exports, sorted(reached - exports)
    assert excluded <= exports, sorted(excluded - exports)
    assert not reached & excluded, sorted(reached & excluded)
    assert reached | excluded == exports, sorted(exports - reached - excluded)
    assert all(isinstance(why, str) and len(why) > 20 for why in sc.EXCLUDED_ENTRIES.values())
    # an entry excluded for taking no stream really takes none: its last parameter is not the `void* stream` of the others
    header = open(_lib.HEADER_PATH).read()
    for name, why in sc.EXCLUDED_ENTRIES.items():
        at = header.index(name + "(")
        prototype = header[at:header.index(";", at)]
        assert ("stream" not in prototype) == (why == sc.NO_STREAM), name
    for name in reached:
        at = header.index(name + "(")
        assert "void* stream" in header[at:header.index(";", at)], name
    # the docstring lists every one of them
    for name in exports:
        assert f"- {name}: " in sc.__doc__, name
    assert "NOT ACCOUNTED FOR" not in sc.__doc__


def classes_with_run():
    found = set()
    for path in glob.glob(os.path.join(PKG, "icpmi", "*.py")):
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.ClassDef) and any(isinstance(f, ast.FunctionDef) and f.name == "run" for f in node.body):
                found.add(node.name)
    return found


def test_every_class_with_a_run_method_is_built_by_a_workload_or_excluded():
    have = classes_with_run()
    assert {"IcpBatch", "GridMatchBatch", "GridSearchBatch", "HistoryMatch", "RunIcpPairBatch"} <= have       # the walk finds them
    reached, excluded = set(sc.reached_classes()), set(sc.EXCLUDED_CLASSES)
    assert reached | excluded == have, (sorted(have - reached - excluded), sorted((reached | excluded) - have))
    assert not reached & excluded
    for name in have:
        assert f"- {name}: " in sc.__doc__, name


def test_the_planned_workloads_are_all_there():
    names = set(sc.WORKLOADS)
    assert {"icp_two_stage_wide", "icp_p2p_two_stage", "icp_exhaustive_3d", "icp_exhaustive_p2l", "icp_big_target", "icp_gated",
            "voxel_large", "nn_set", "nn_set_sweep", "normals_set", "rotation_search_batch", "feature_align_batch", "run_icp_pair_batch",
            "submap_rotation_search", "history_match", "history_world_rows", "grid_match", "grid_search", "grid_likelihood_field",
            "grid_occupancy_planes", "grid_cast", "grid_check", "grid_beam", "particle_round", "grid_update_tiles", "grid_update_atomic",
            "grid_update_owner", "information"} <= names
    assert sc.WORKLOADS["icp_p2p_two_stage"].options == {"ICP2_STAGES": "2"}
    assert {sc.WORKLOADS[f"grid_update_{p}"].options["ICPMI_RAYCAST"] for p in ("tiles", "atomic", "owner")} == {"tiles", "atomic", "owner"}
    for w in sc.WORKLOADS.values():
        assert w.entries and all(callable(f) for f in (w.inputs, w.build, w.run, w.outputs, w.compare)), w.name


def test_owned_tensors_finds_nested_and_repeated_tensors():
    import torch
    a, b, c, d = torch.zeros(3), torch.ones((2, 2)), torch.arange(4, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8)

    class Inner:
        def __init__(self):
            self.own, self.shared, self.host, self.note = b, a, np.zeros(3), "text"
            self.fn = lambda: 0

    class Outer:
        def __init__(self):
            self.first = a
            self.inner = Inner()
            self.again = self.inner                               # the same object under a second name
            self.parts = [c, (d, {"k": a, "view": a[:]})]         # a repeat, and a second tensor over exactly the same memory
            self.half = a[1:]                                     # other memory: listed
            self.empty = torch.zeros(0)                           # nothing to poison: left out
            self.loop = self                                      # a cycle

    found = sc.owned_tensors(Outer(), device_type="cpu")
    assert list(found) == ["first", "inner.own", "parts[0]", "parts[1][0]", "half"], list(found)
    assert found["first"] is a and found["inner.own"] is b and found["parts[0]"] is c and found["parts[1][0]"] is d
    assert sc.owned_tensors(Outer()) == {}                        # nothing on a GPU here
    ns = types.SimpleNamespace(x=a, deep=types.SimpleNamespace(y=[b]))
    assert list(sc.owned_tensors(ns, device_type="cpu")) == ["x", "deep.y[0]"]


def test_poison_leaves_nan_in_floats_and_zero_bytes_in_integers():
    import torch
    tensors = [torch.ones(5, dtype=torch.float64), torch.ones((2, 3), dtype=torch.float32), torch.full((4,), 7, dtype=torch.int32),
               torch.full((4,), -3, dtype=torch.int64), torch.full((9,), 255, dtype=torch.uint8), torch.full((3,), 9, dtype=torch.int16),
               torch.ones(3, dtype=torch.bool)]
    view = tensors[0][1:3]                                        # a view is poisoned with its owner
    sc.poison_(tensors)
    for t in tensors[:2]:
        assert bool(torch.isnan(t).all())
    assert bool(torch.isnan(view).all())
    for t in tensors[2:]:
        assert t.numpy().tobytes() == bytes(t.numel() * t.element_size()), t.dtype


@pytest.mark.parametrize("name", list(sc.WORKLOADS))
def test_inputs_are_deterministic(name):
    w = sc.WORKLOADS[name]
    make = w.inputs.__wrapped__                                   # past the cache: generated twice
    a, b = make(0), make(0)
    assert a.keys() == b.keys() and len(a) > 0
    for key in a:
        xs, ys = (v if isinstance(v, list) else [v] for v in (a[key], b[key]))
        assert len(xs) == len(ys) > 0
        for x, y in zip(xs, ys):
            assert isinstance(x, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, key)
    if name in ("icp_two_stage_wide", "history_match"):           # another seed is another input set
        c = make(1)
        assert any(x.tobytes() != y.tobytes() for x, y in zip(a["clouds"], c["clouds"]))


def test_the_large_batch_has_the_shapes_its_paths_need():
    inp = sc.WORKLOADS["icp_two_stage_wide"].inputs(0)
    rows = np.array([len(c) for c in inp["clouds"]])
    B = sc.LARGE_B
    assert len(rows) == 2 * B and B >= 1024
    wide = np.array(sc.WIDE_PAIRS)
    assert len(wide) == 16 and (rows[wide] > 1536).all() and (rows[B + wide] > 1536).all()          # before the filter; the GPU test counts after
    narrow = np.setdiff1d(np.arange(B), wide)
    assert rows[narrow].max() <= 128 and rows[B + narrow].max() <= 128 and rows[narrow].min() >= 32
    assert len(sc.FAR_PAIRS) == 16 and not set(sc.FAR_PAIRS) & set(sc.WIDE_PAIRS)
    assert len(sc.WORKLOADS["icp_big_target"].inputs(0)["clouds"][1]) == 4097
    assert len(sc.WORKLOADS["voxel_large"].inputs(0)["clouds"][0]) == 8193
