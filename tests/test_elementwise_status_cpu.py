"""Which status every entry point of csrc/elementwise.hip and csrc/elementwise_bf16.hip returns for a defective call, held to the rule
include/ssd_gfx950.h states (REFUSALS): NULL, then shape, then alignment, then workspace -- never to what a build happens to return --
and the same for the f32 and the bf16 entry of one operation.

An entry's arguments are listed in the order of its C signature, each as (name, kind, value of the valid call):
  P  required pointer, 16-byte aligned     p  optional one, given in the valid call     n  optional, not given (NULL)
  R  required pointer without an alignment rule         u  a value no rule looks at
  A4 / A8  required argmax codes aligned to 4 / 8 bytes, a4 / a8 optional ones (given)
  W  the workspace (required), Z its size: the entry's query, S the stream (NULL), i / z / f  int, size_t, float
"""
import itertools

import pytest
import torch

OK_PTR, ODD_PTR, ODD_BYTES = 0x10000, 0x10004, 0x10002
OK, BAD_SHAPE, WORKSPACE, NULL, LAUNCH, ALIGN = 0, -1, -2, -3, -4, -5
ORDER = [NULL, BAD_SHAPE, ALIGN, WORKSPACE]                  # where several apply, the first of these is returned

_POOL_DIMS = [("N", "i", 2), ("H", "i", 7), ("W", "i", 10), ("C", "i", 8), ("k", "i", 3), ("stride", "i", 2), ("pad", "i", 1), ("Ho", "i", 4),
              ("Wo", "i", 5), ("stream", "S")]
_HEAD_DIMS = [("N", "i", 2), ("HW", "i", 9), ("A", "i", 4), ("prior_off", "i", 8), ("P", "i", 100), ("ncls", "i", 3), ("stream", "S")]
_L2 = [("M", "i", 5), ("C", "i", 512)]
_SGD = [("param", "R"), ("grad", "R"), ("buf", "R"), ("n", "z", 16), ("lr", "f", 0.1), ("momentum", "f", 0.9), ("weight_decay", "f", 0.0),
        ("grad_scale_dev", "u", None), ("first_step", "i", 1)]
_LAYOUT = [("w", "R"), ("o", "R"), ("Co", "i", 8), ("Ci", "i", 4), ("R", "i", 3), ("S", "i", 3), ("Co_pad", "i", 8), ("stream", "S")]

ENTRIES = {
    "ssd_maxpool_fwd": [("x", "P"), ("y", "P"), ("argmax", "a4")] + _POOL_DIMS,
    "ssd_maxpool_fwd_bf16": [("x", "P"), ("y", "P"), ("argmax", "a8")] + _POOL_DIMS,
    "ssd_maxpool_bwd": [("dy", "P"), ("argmax", "A4"), ("dx", "P"), ("relu_mask", "p"), ("accumulate", "i", 1)] + _POOL_DIMS,
    "ssd_maxpool_bwd_bf16": [("dy", "P"), ("argmax", "A8"), ("dx", "P"), ("relu_mask", "p"), ("y_gate", "n"), ("accumulate", "i", 1)] + _POOL_DIMS,
    "ssd_maxpool_bwd_gated": [("dy", "P"), ("argmax", "A4"), ("y_gate", "P"), ("dx", "P")] + _POOL_DIMS,
    "ssd_maxpool_bwd_bf16:gated": [("dy", "P"), ("argmax", "A8"), ("dx", "P"), ("relu_mask", "n"), ("y_gate", "p"), ("accumulate", "i", 0)] + _POOL_DIMS,
    "ssd_l2norm_fwd": [("x", "P"), ("gamma", "P"), ("y", "P")] + _L2 + [("stream", "S")],
    "ssd_l2norm_fwd_bf16": [("x", "P"), ("gamma", "P"), ("y", "P")] + _L2 + [("stream", "S")],
    "ssd_l2norm_bwd": [("x", "P"), ("gamma", "P"), ("dy", "P"), ("dx", "P"), ("dgamma", "R")] + _L2 + [("workspace", "W"), ("workspace_bytes", "Z"), ("stream", "S")],
    "ssd_l2norm_bwd_bf16": [("x", "P"), ("gamma", "P"), ("dy", "P"), ("dx", "P"), ("dgamma", "R")] + _L2 + [("workspace", "W"), ("workspace_bytes", "Z"), ("stream", "S")],
    "ssd_heads_scatter": [("packed", "R"), ("ld", "i", 32), ("loc", "R"), ("conf", "R")] + _HEAD_DIMS,
    "ssd_heads_gather": [("dloc", "R"), ("dconf", "R"), ("packed", "R"), ("ld", "i", 32)] + _HEAD_DIMS,
    "ssd_heads_gather_bf16": [("dloc", "R"), ("dconf", "R"), ("packed", "R"), ("ld", "i", 32)] + _HEAD_DIMS,
    "ssd_cast_f32_bf16": [("x", "P"), ("y", "P"), ("n", "z", 64), ("stream", "S")],
    "ssd_cast_bf16_f32": [("x", "P"), ("y", "P"), ("n", "z", 64), ("stream", "S")],
    "ssd_channel_affine": [("x", "P"), ("scale", "P"), ("shift", "P"), ("y", "P"), ("M", "z", 5), ("C", "i", 8), ("relu", "i", 0), ("stream", "S")],
    "ssd_weight_oihw_to_ohwi": _LAYOUT,
    "ssd_weight_oihw_to_ihwo": _LAYOUT,
    "ssd_im2col_first": [("x", "R"), ("out", "P"), ("N", "i", 1), ("H", "i", 4), ("W", "i", 4), ("stream", "S")],
    "ssd_im2col_nchw3": [("x", "R"), ("out", "P"), ("N", "i", 1), ("H", "i", 16), ("W", "i", 16), ("R", "i", 7), ("S", "i", 7), ("stride", "i", 2),
                         ("pad", "i", 3), ("Ho", "i", 8), ("Wo", "i", 8), ("Kpad", "i", 148), ("stream", "S")],
    "ssd_clock_probe": [("out", "R"), ("stream", "S")],
    "ssd_graph_node_counts": [("graph", "R"), ("kernel_nodes", "R"), ("total_nodes", "R")],
    "ssd_sgd_momentum": _SGD + [("stream", "S")],
    "ssd_sgd_momentum_guarded": _SGD + [("skip_dev", "R"), ("stream", "S")],
}
WORKSPACE_QUERY = {"ssd_l2norm_bwd": "ssd_l2norm_bwd_workspace", "ssd_l2norm_bwd_bf16": "ssd_l2norm_bwd_bf16_workspace"}


def _ints(name, *values):
    return [(f"{name}{v}", {name: v}) for v in values]


_COUNTS = lambda *names: [d for nm in names for d in _ints(nm, 0, -1)]                                   # noqa: E731
_POOL_SHAPE = _COUNTS("N", "H", "W", "C", "Ho", "Wo") + _ints("k", 0, 16) + _ints("stride", 0) + _ints("pad", -1)
# forward only: 2*pad > k, and a last window (row / column) that starts past the input
_POOL_FWD_SHAPE = _POOL_SHAPE + _ints("pad", 2) + _ints("Ho", 6) + _ints("Wo", 7)
_HEAD_SHAPE = _COUNTS("N", "HW", "A", "ncls") + _ints("ld", 27) + _ints("prior_off", -1, 65)
_L2_SHAPE = _ints("M", 0, -1) + _ints("C", 0, 256, 1024)
_LAYOUT_SHAPE = _COUNTS("Co", "Ci", "R", "S") + _ints("Co_pad", 4)

# the BAD_SHAPE defects of each entry beyond what its argument kinds imply; "C no multiple of the vector" carries one label in both dtypes
SHAPE = {
    "ssd_maxpool_fwd": _POOL_FWD_SHAPE + [("Cvec", {"C": 6})],
    "ssd_maxpool_fwd_bf16": _POOL_FWD_SHAPE + [("Cvec", {"C": 12})],
    "ssd_maxpool_bwd": _POOL_SHAPE + [("Cvec", {"C": 6})],
    "ssd_maxpool_bwd_bf16": _POOL_SHAPE + [("Cvec", {"C": 12}), ("gate-with-mask", {"y_gate": OK_PTR})],
    "ssd_maxpool_bwd_gated": _POOL_SHAPE + [("Cvec", {"C": 6})],
    "ssd_maxpool_bwd_bf16:gated": _POOL_SHAPE + [("Cvec", {"C": 12}), ("gate-with-mask", {"relu_mask": OK_PTR}), ("gate-with-accumulate", {"accumulate": 1})],
    "ssd_l2norm_fwd": _L2_SHAPE, "ssd_l2norm_fwd_bf16": _L2_SHAPE, "ssd_l2norm_bwd": _L2_SHAPE, "ssd_l2norm_bwd_bf16": _L2_SHAPE,
    "ssd_heads_scatter": _HEAD_SHAPE, "ssd_heads_gather": _HEAD_SHAPE, "ssd_heads_gather_bf16": _HEAD_SHAPE,
    "ssd_cast_f32_bf16": _ints("n", 0, 12), "ssd_cast_bf16_f32": _ints("n", 0, 12),
    "ssd_channel_affine": _ints("M", 0) + _ints("C", 0, -4, 6),
    "ssd_weight_oihw_to_ohwi": _LAYOUT_SHAPE, "ssd_weight_oihw_to_ihwo": _LAYOUT_SHAPE,
    "ssd_im2col_first": _COUNTS("N", "H", "W"),
    "ssd_im2col_nchw3": _COUNTS("N", "H", "W", "R", "S") + _ints("stride", 0) + _ints("pad", -1) + _ints("Kpad", 150, 144) + _ints("Ho", 9, 0) +
    _ints("Wo", 9, 0),
    "ssd_clock_probe": [], "ssd_graph_node_counts": [], "ssd_sgd_momentum": [], "ssd_sgd_momentum_guarded": [],
}
assert set(SHAPE) == set(ENTRIES)
# an ALIGN defect of the bf16 entries only: codes aligned to 4 bytes are the f32 entries' valid call
ALIGN_EXTRA = {e: [("argmax4", {"argmax": ODD_PTR})] for e in ("ssd_maxpool_fwd_bf16", "ssd_maxpool_bwd_bf16", "ssd_maxpool_bwd_bf16:gated")}

# f32 entry -> bf16 entry of the same operation, and the labels only one of the two has (the bf16 backward is one entry for both forms:
# its gate is optional, so a NULL there is the ungated call, and giving it next to a mask or accumulate is its own defect)
PAIRS = {
    "ssd_maxpool_fwd": ("ssd_maxpool_fwd_bf16", {"argmax4"}),
    "ssd_maxpool_bwd": ("ssd_maxpool_bwd_bf16", {"argmax4", "gate-with-mask"}),
    "ssd_maxpool_bwd_gated": ("ssd_maxpool_bwd_bf16:gated", {"argmax4", "gate-with-mask", "gate-with-accumulate", "null:y_gate"}),
    "ssd_l2norm_fwd": ("ssd_l2norm_fwd_bf16", set()),
    "ssd_l2norm_bwd": ("ssd_l2norm_bwd_bf16", set()),
    "ssd_heads_gather": ("ssd_heads_gather_bf16", set()),
}


def defects(entry):
    """[(label, {argument: value}, status the header states)]"""
    out = []
    for name, kind, *_ in ENTRIES[entry]:
        if kind in ("P", "R", "A4", "A8", "W"):
            out.append((f"null:{name}", {name: None}, NULL))
        if kind in ("P", "p"):
            out.append((f"odd:{name}", {name: ODD_PTR}, ALIGN))
        if kind in ("A4", "A8", "a4", "a8"):
            out.append((f"odd:{name}", {name: ODD_BYTES}, ALIGN))
        if kind == "Z":
            out.append(("ws-1", {name: -1}, WORKSPACE))
    out += [(la, ch, BAD_SHAPE) for la, ch in SHAPE[entry]]
    out += [(la, ch, ALIGN) for la, ch in ALIGN_EXTRA.get(entry, [])]
    assert len({la for la, _, _ in out}) == len(out), entry
    return out


def cases(entry):
    """every single defect, and every pair that does not set one argument twice with the status that comes first in ORDER"""
    d = defects(entry)
    out = list(d)
    for (la, ca, sa), (lb, cb, sb) in itertools.combinations(d, 2):
        if not set(ca) & set(cb):
            out.append((f"{la}+{lb}", {**ca, **cb}, min(sa, sb, key=ORDER.index)))
    return out


def call(lib, entry, changes):
    args = []
    for name, kind, *value in ENTRIES[entry]:
        if kind == "Z":
            m, c = (changes.get(k, dict((a[0], a[2]) for a in _L2)[k]) for k in ("M", "C"))
            args.append(getattr(lib, WORKSPACE_QUERY[entry])(max(m, 1), c) + changes.get(name, 0))
        elif name in changes:
            args.append(changes[name])
        elif kind in ("n", "S"):
            args.append(None)
        elif kind in ("i", "z", "f", "u"):
            args.append(value[0])
        else:
            args.append(OK_PTR)
    return getattr(lib, entry.split(":")[0])(*args)


@pytest.fixture(scope="module")
def lib():
    """Every case is refused before anything is enqueued, so the made-up pointers are never dereferenced; where a GPU is present the
    tests still do not run, so that a tuple some change made acceptable can never reach a launch on a shared machine."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no launch can succeed")
    from objectdetection_ssd_amd import _lib
    return _lib.load()


def test_the_table_lists_every_entry_point_of_the_two_source_files():
    import os
    import re
    from objectdetection_ssd_amd import _lib
    found = set()
    for f in ("elementwise.hip", "elementwise_bf16.hip"):
        with open(os.path.join(_lib.PKG, "csrc", f)) as fh:
            found |= set(re.findall(r'^extern "C" \w[\w\s\*]*?\b(ssd_\w+)\(', fh.read(), re.M))
    no_pointers_or_queries = {"ssd_abi_version", "ssd_status_string", "ssd_l2norm_bwd_workspace", "ssd_l2norm_bwd_bf16_workspace"}
    assert found - no_pointers_or_queries == {e.split(":")[0] for e in ENTRIES}
    for e in ENTRIES:                                        # the table's argument count is the binding's
        assert len(ENTRIES[e]) == len(_lib.SIGNATURES[e.split(":")[0]][1]), e


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_defect_and_pair_returns_the_status_the_header_states(lib, entry):
    got = [(la, call(lib, entry, ch), want) for la, ch, want in cases(entry)]
    wrong = [g for g in got if g[1] != g[2]]
    assert not wrong, f"{entry}: {len(wrong)} of {len(got)} statuses differ (defects, got, stated): {wrong[:20]}"


@pytest.mark.parametrize("f32", list(PAIRS))
def test_f32_and_bf16_entries_of_one_operation_refuse_the_same_defects(lib, f32):
    bf16, one_sided = PAIRS[f32]
    a = {la: call(lib, f32, ch) for la, ch, _ in cases(f32)}
    b = {la: call(lib, bf16, ch) for la, ch, _ in cases(bf16)}
    single = lambda d: {la for la in d if "+" not in la}                      # noqa: E731
    assert single(a) ^ single(b) <= one_sided, sorted(single(a) ^ single(b))
    differ = [(la, a[la], b[la]) for la in a if la in b and a[la] != b[la]]
    assert not differ, f"{f32} / {bf16} disagree on (defects, f32, bf16): {differ[:20]}"
    assert len(set(a) & set(b)) >= len(a) // 2
