"""The engine's cache of re-laid filters (`Model._FilterCache`, `_Filter`, the family table `_FAMILIES`) without a GPU.

1. What `_Engine._prepare_weights_batched` builds -- per job, in order: layer, family, the job's numbers, shape and dtype of both
   output buffers, and where its record lands in the cache -- equals tests/golden/weight_jobs.json.  That file was recorded from commit
   af48c27, the last one in which the per-layer routines and the table each wrote the cache's entry shapes out by hand, with
   `ops.WeightTable` replaced by the stub below and a CPU zeros tensor for x.  It names cache keys the way that commit did
   ("wino:<layer>", "x31:<layer>", "b16:<layer>", the bare layer for `layout` and `first`); `_old_key` maps today's
   (family slot, layer) onto that.
2. The cache's semantics, with family builders that count their calls and return CPU tensors."""
import json
import os
from dataclasses import replace

import pytest
import torch

from objectdetection_ssd_amd import Model, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_jobs.json")
MODES = {"f32": {}, "direct": {"wino": False}, "bf16": {"bf16": True}}


class _StubTable:
    """`ops.WeightTable` without a device: keeps the jobs, runs nothing."""

    def __init__(self, jobs, device):
        self.jobs, self.keep = jobs, []

    def run(self):
        pass


@pytest.fixture(scope="module")
def limb_form():
    """The library's limb-GEMM switch (`ssd_wino_uses_x3`, a host query), on as by default whatever the environment says; the
    callable sets it, and the switch goes back to the environment's value afterwards."""
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()

    def set_(on):
        assert lib.ssd_tune_set_wino_x3(int(on)) == 0
    set_(1)
    try:
        yield set_
    finally:
        assert lib.ssd_tune_set_wino_x3(-1) == 0


@pytest.fixture(scope="module")
def params():
    return {300: Model.SSD_300()._forward_params(), 512: Model.SSD_512()._forward_params()}


def _shape(t):
    return None if t is None else [list(t.shape), str(t.dtype).replace("torch.", "")]


def _old_key(slot, layer):
    return layer if slot in ("first", "layout") else slot + ":" + layer


@pytest.mark.parametrize("bs", (2, 32))             # 32: fc7 and seq8.0 cross the 1x1 limb-GEMM threshold (X31_MIN_PIXELS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("variant", (300, 512))
def test_weight_table_jobs_and_records_are_those_of_the_recorded_commit(monkeypatch, limb_form, params, variant, mode, bs):
    with open(GOLDEN) as f:
        want = json.load(f)[f"{variant}/{mode}/{bs}"]
    assert len(want) == {300: 29, 512: 32}[variant]
    monkeypatch.setattr(ops, "WeightTable", _StubTable)
    eng, P = Model._Engine(variant), params[variant]
    for k, v in MODES[mode].items():
        setattr(eng, k, v)
    assert eng.uses_weight_table()
    x = torch.zeros(1, 3, variant, variant).expand(bs, 3, variant, variant)
    eng._prepare_weights_batched(x, P)
    fill = eng._wcache.fill
    assert len(fill.table.jobs) == len(fill.entries) == len(eng._wcache)
    got = []
    for j, (what, L, fwd, bwd) in zip(fill.table.jobs, fill.entries):
        assert j["out_fwd"] is fwd and j["out_bwd"] is bwd
        at = [k for k, rec in eng._wcache.items() if rec.fwd is fwd]
        assert len(at) == 1
        rec = eng._wcache[at[0]]
        assert rec.bwd is bwd and rec.fwd_limbs is None and rec.bwd_limbs is None and rec.oihw is None
        assert rec.sig == Model._FilterCache.sig(Model._FAMILIES[what], L, P)
        got.append({"layer": L.key, "family": what,
                    "job": [j["kind"], j["co0"], j["co"], j["ci"], j["taps"], j["co_pad"], j.get("pad1", 0), bool(j.get("adj", False))],
                    "out_fwd": _shape(fwd), "out_bwd": _shape(bwd), "cache_key": _old_key(*at[0])})
    assert got == want
    assert eng._wcache.kinds() == {row["layer"]: row["family"] for row in want}
    # the table is rebuilt only when its key changes; the records are new ones every step, on the same buffers
    eng._wcache.clear()
    assert len(eng._wcache) == 0 and eng._wcache.fill is fill
    eng._prepare_weights_batched(x, P)
    assert eng._wcache.fill is fill and len(eng._wcache) == len(want)


# ---- cache semantics -----------------------------------------------------------------------------------------------------------------
class _Counting:
    """Stand-ins for the per-layer builders: CPU tensors, calls counted by name."""

    def __init__(self):
        self.calls = []

    def family(self, name, eng_family):
        def build(eng, L, w, adj):
            self.calls.append((name, L.key, adj))
            return w.clone(), (w + 1 if name != "layout" else None)
        return replace(eng_family, build=build)

    def op(self, name):
        def fn(t, *a):
            self.calls.append((name,))
            return t + 2
        return fn

    def count(self, name):
        return sum(1 for c in self.calls if c[0] == name)


@pytest.fixture()
def stubbed(monkeypatch):
    """An SSD300 engine on CPU parameters whose `layout` and Winograd families build through `_Counting`."""
    c = _Counting()
    for name in ("layout", "wino", "wino_adj"):
        monkeypatch.setitem(Model._FAMILIES, name, c.family(name, Model._FAMILIES[name]))
    monkeypatch.setattr(ops, "weight_ihwo", c.op("ihwo"))
    monkeypatch.setattr(ops, "weight_split3", c.op("split3"))
    eng = Model._Engine(300)
    P = {n: torch.nn.Parameter(torch.randn(4, 3)) for n in eng.names}
    return eng, P, c


def test_lookup_hits_while_every_source_tensor_is_unchanged(stubbed):
    eng, P, c = stubbed
    L = eng.layers["c_7"]                                   # a head: two source tensors
    rec = eng._filter("layout", L, P)
    assert c.count("layout") == 1 and rec.sig == tuple((P[n].data_ptr(), P[n]._version) for n in L.weights)
    assert torch.equal(rec.fwd, torch.cat([P[n] for n in L.weights]).detach()) and rec.oihw is not None
    assert eng._filter("layout", L, P) is rec and c.count("layout") == 1          # the second lookup is a hit
    assert list(eng._wcache) == [("layout", "c_7")]
    with torch.no_grad():
        P[L.weights[1]].mul_(2.0)                           # version bump of the second tensor
    rec2 = eng._filter("layout", L, P)
    assert rec2 is not rec and c.count("layout") == 2 and eng._wcache[("layout", "c_7")] is rec2
    P = dict(P)
    P[L.weights[0]] = torch.nn.Parameter(P[L.weights[0]].detach().clone())        # other storage, version 0 again
    rec3 = eng._filter("layout", L, P)
    assert rec3 is not rec2 and c.count("layout") == 3
    assert eng._filter("layout", L, P) is rec3 and c.count("layout") == 3
    eng._wcache.clear()
    assert len(eng._wcache) == 0 and eng._wcache.tensors() == []
    assert eng._filter("layout", L, P) is not rec3 and c.count("layout") == 4


def test_winograd_records_also_depend_on_the_adjoint_flag_and_the_limb_form(stubbed, limb_form):
    eng, P, c = stubbed
    L = eng.layers["model.features.2"]
    w = P[L.weights[0]]
    rec = eng._filter("wino", L, P)
    assert rec.sig == ((w.data_ptr(), w._version), True, False) and c.calls == [("wino", L.key, False)]
    assert eng._filter("wino", L, P) is rec
    adj = eng._filter("wino_adj", L, P)                     # the other form: same slot, rebuilt
    assert adj is not rec and adj.sig[-1] is True and c.calls[-1] == ("wino_adj", L.key, True)
    assert list(eng._wcache) == [("wino", L.key)] and eng._wcache[("wino", L.key)] is adj
    assert eng._filter("wino_adj", L, P) is adj and len(c.calls) == 2
    try:
        limb_form(0)
        off = eng._filter("wino_adj", L, P)
        assert off is not adj and off.sig[-2:] == (False, True) and len(c.calls) == 3
        assert eng._filter("wino_adj", L, P) is off
    finally:
        limb_form(1)
    assert eng._filter("wino_adj", L, P) is not off and len(c.calls) == 4
    # the other families' signatures carry neither
    assert Model._FilterCache.sig(Model._FAMILIES["b16"], L, P) == ((w.data_ptr(), w._version),)


def test_backward_layout_and_limb_planes_are_built_on_first_request_once(stubbed):
    eng, P, c = stubbed
    L = eng.layers["conv_fc7"]
    rec = eng._filter("layout", L, P)
    assert rec.bwd is None and rec.fwd_limbs is None and c.count("ihwo") == 0 and c.count("split3") == 0
    eng._filter("layout", L, P)
    assert rec.bwd is None and c.count("ihwo") == 0         # a forward-only reader launches nothing more
    assert eng._filter("layout", L, P, need_bwd=True) is rec
    assert torch.equal(rec.bwd, rec.oihw + 2) and c.count("ihwo") == 1
    eng._filter("layout", L, P, need_bwd=True)
    eng._filter("layout", L, P)
    assert c.count("ihwo") == 1 and c.count("split3") == 0 and rec.fwd_limbs is None and rec.bwd_limbs is None
    # limb planes: only in the f32x3 mode and the bf16 mode on f32 tensors
    for flags in ({"bf16": True}, {"x3": True}, {"bf16": True, "bf16_tensors": False}):
        eng2, c.calls = Model._Engine(300), []
        for k, v in flags.items():
            setattr(eng2, k, v)
        r = eng2._filter("layout", L, P)
        if flags == {"bf16": True}:
            assert r.fwd_limbs is None and c.count("split3") == 0
            continue
        assert torch.equal(r.fwd_limbs, r.fwd + 2) and r.bwd_limbs is None and c.count("split3") == 1
        eng2._filter("layout", L, P, need_bwd=True)
        eng2._filter("layout", L, P, need_bwd=True)
        assert torch.equal(r.bwd_limbs, r.bwd + 2) and c.count("split3") == 2 and c.count("ihwo") == 1


def test_tensors_lists_every_tensor_of_every_record_and_a_swapped_in_cache_leaves_the_old_one_alone(stubbed):
    eng, P, c = stubbed
    eng.x3 = True
    a = eng._filter("layout", eng.layers["conv_fc7"], P, need_bwd=True)
    b = eng._filter("wino", eng.layers["model.features.2"], P)
    held = [a.fwd, a.bwd, a.fwd_limbs, a.bwd_limbs, a.oihw, b.fwd, b.bwd]
    assert all(torch.is_tensor(t) for t in held) and b.oihw is None and b.fwd_limbs is None
    assert sorted(map(id, eng._wcache.tensors())) == sorted(map(id, held))
    before, fields = dict(eng._wcache), {k: dict(vars(r)) for k, r in eng._wcache.items()}
    shared, eng._wcache = eng._wcache, Model._FilterCache()            # what GraphedForward does around its capture
    try:
        other = eng._filter("layout", eng.layers["conv_fc7"], P)
        assert other is not a and list(eng._wcache) == [("layout", "conv_fc7")] and eng._wcache.fill is None
    finally:
        eng._wcache = shared
    assert eng._wcache.keys() == before.keys() and all(eng._wcache[k] is v for k, v in before.items())
    assert all(vars(eng._wcache[k])[f] is v for k, d in fields.items() for f, v in d.items())
    assert eng._filter("layout", eng.layers["conv_fc7"], P) is a
