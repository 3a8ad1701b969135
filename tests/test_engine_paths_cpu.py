"""The engine's one dispatch decision (`Model._Engine._path`, walked over the op list by `_plan`) without a GPU: for every conv and head
op of SSD300 and SSD512 it names the kernel family that tests/golden/engine_paths.json holds.  That table was recorded on an MI355X
from the commit BEFORE `_path` existed -- after one training forward per mode, (layer, kind) of its batched weight table; for the
f32x3 mode, which lays its filters out layer by layer, the kinds of the weight-cache entries that forward left -- when the forward,
the backward and the weight table each wrote the ladder out for themselves."""
import inspect
import json
import os

import pytest

from objectdetection_ssd_amd import Model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_paths.json")
MODES = {"f32": {}, "direct": {"wino": False}, "bf16": {"bf16": True}, "x3": {"x3": True}}
# weight-table kind -> (family, adjoint filter layout)
FAMILY = {"b16": ("b16", False), "wino": ("wino", False), "wino_adj": ("wino", True), "x31": ("x31", False), "layout": ("direct", False)}


@pytest.fixture(scope="module")
def golden():
    from objectdetection_ssd_amd import _lib
    _lib.load()                                     # the decision asks the library which GEMM form its Winograd filters take
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("bs", (2, 32))             # 32: fc7 and seq8.0 cross the 1x1 limb-GEMM threshold (X31_MIN_PIXELS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("variant", (300, 512))
def test_every_layer_takes_the_recorded_path(golden, variant, mode, bs):
    eng = Model._Engine(variant)
    for k, v in MODES[mode].items():
        setattr(eng, k, v)
    want = golden[f"{variant}/{mode}/{bs}"]
    plan = list(eng._plan(bs, variant, variant))
    assert [op["p"] for op, _, _, _ in plan] == [o["p"] for o in eng.ops if o["op"] in ("conv", "head")]
    assert set(want) == {L.key for _, L, _, _ in plan}
    for op, L, g, path in plan:
        assert L is eng.layers[op["p"]] and L.head == (op["op"] == "head")
        assert (path.kind, path.adj) == FAMILY[want[L.key]], (L.key, path)
        assert eng._table_kind(path) == want[L.key]                       # what the weight table lays out for it
        if L.head:                                                        # a head: no pool fusion, no adjoint form, no ReLU bits, no 1x1 path
            assert path.pool is None and not path.adj and not path.bits and path.kind != "x31"
        assert not path.cast16 or (L.head and path.kind == "b16")
        assert not (path.keep or path.bits or path.adj or path.pool or path.wino_wgrad) or path.kind == "wino"


def test_layer_records_name_the_engine_s_parameters():
    for variant, n_conf in ((300, 21), (512, 2), (300, 256)):
        eng = Model._Engine(variant, n_conf)
        names = [n for op in eng.ops if op["op"] in ("conv", "head") for L in (eng.layers[op["p"]],)
                 for pair in zip(L.weights, L.biases) for n in pair]
        assert sorted(names) == sorted(n for n in eng.names if not n.startswith(("model.features.0.", "rescaling")))
        for op in eng.ops:
            if op["op"] == "head":
                L = eng.layers[op["p"]]
                assert (L.rows0, L.co, L.co_pad, L.ld16) == (4 * op["a"], op["a"] * (4 + n_conf), -(-L.co // 32) * 32, -(-L.co // 64) * 64)


def test_head_gradient_rows_are_split_at_the_loc_rows():
    import torch
    L = Model._Engine(300).layers["c_7"]
    grads = {}
    dw, db = torch.arange(L.co * 2.).view(L.co, 2), torch.arange(float(L.co))
    L.hand(grads, dw, db)
    assert list(grads) == ["c_7_bb.weight", "c_7_cl.weight", "c_7_bb.bias", "c_7_cl.bias"]      # the order a gradient listener hears them in
    assert torch.equal(torch.cat((grads["c_7_bb.weight"], grads["c_7_cl.weight"])), dw) and grads["c_7_bb.weight"].shape[0] == 24
    assert torch.equal(torch.cat((grads["c_7_bb.bias"], grads["c_7_cl.bias"])), db) and grads["c_7_bb.bias"].shape[0] == 24


def test_forward_backward_and_weight_table_read_one_decision():
    """The predicates of the ladder are called by `_path` (and by each other) only: the forward asks `_path` and records the answer, the
    backward reads the record, the weight table walks `_plan`, which asks `_path`."""
    E = Model._Engine
    ladder = ("_t16", "_head16", "_wino_ok", "_x31_ok", "_adj_ok", "_wino_wgrad_ok")
    src = {f: inspect.getsource(getattr(E, f)) for f in ("_forward_ops", "_conv_forward", "_backward_ops", "_prepare_weights_batched", "_plan")}
    for f, text in src.items():
        assert not [p for p in ladder if "self." + p + "(" in text], f
    assert 'aux["path:" + L.key] = self._path(' in src["_forward_ops"]
    assert 'aux["path:" + L.key]' in src["_backward_ops"] and "self._path(" not in src["_backward_ops"]
    assert "self._path(" in src["_plan"] and "self._plan(" in src["_prepare_weights_batched"]
    assert "self._path(" not in src["_conv_forward"] and "self._path(" not in src["_prepare_weights_batched"]
