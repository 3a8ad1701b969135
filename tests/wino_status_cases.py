"""The argument tuples of tests/test_wino_status_cpu.py: for every exported Winograd entry point that takes pointers, one valid call on
a small geometry (made-up pointer values, as in tests/test_host_cpu.py) and that call with every single defect and every pair of
defects from a fixed list.  Every tuple is one the library must refuse before it enqueues anything; the status it returns --
which of several applicable ones wins included -- is recorded in tests/golden/wino_status.json (`python tests/wino_status_cases.py
--record`, run against the library the statuses are to be held to, on a machine without a GPU).

An entry's arguments are listed in the order of its C signature, each as (name, kind[, value]):
  P  required f32 pointer, 16-byte aligned          p  optional one (given in the valid call)      n  optional, not given
  R  required pointer whose alignment is not checked
  B / b  required / optional 64-bit mask words (8-byte aligned)          a  optional argmax bytes (4-byte aligned), A required
  G  the geometry (NULL is a defect too), H the geometry of the layer below (ssd_wino4_adj_output_to_planes)
  W  the workspace pointer, Zf / Zd / Zw / Zg its size: forward, data-gradient, weight-gradient, weight-gradient-GEMM query
  i  an int (value given), u a pointer or int no rule looks at (passed as given), S the stream (NULL)
"""
import itertools
import json
import os

OK_PTR, ODD_PTR, ODD_BYTES = 0x10000, 0x10004, 0x10002
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_status.json")

# ops.make_geom arguments of the valid call: 2 x 10 x 10 x 64 -> 64 channels, 3x3 / stride 1 / pad 1
GEOM = dict(n=2, h=10, w=10, ci=64, co=64, k=3, stride=1, pad=1, dil=1)
POOL_HW = 5                                                  # the 2x2 / stride-2 pool of that map

_FWD = [("x", "P"), ("U_fwd", "P"), ("bias", "u", OK_PTR), ("y", "P"), ("ldy", "i", 64), ("g", "G"), ("relu", "i", 1)]
_POOL = [("x", "P"), ("U_fwd", "P"), ("bias", "p"), ("y_pooled", "P"), ("argmax", "a"), ("g", "G"), ("ceil_mode", "i", 0)]
_WS = lambda z: [("workspace", "W"), ("workspace_bytes", z), ("stream", "S")]
_POOLED_SRC = [("dpool", "P"), ("argmax", "A"), ("y_pooled", "P"), ("Hp", "i", POOL_HW), ("Wp", "i", POOL_HW), ("ldy", "i", 64)]

ENTRIES = {
    "ssd_conv3x3_wino_fwd": _FWD + [("mo", "i", 4)] + _WS("Zf"),
    "ssd_conv3x3_wino_fwd_keep": _FWD + [("planes_keep", "P")] + _WS("Zf"),
    "ssd_conv3x3_wino_fwd_keep_bits": _FWD + [("planes_keep", "P"), ("relu_bits_out", "b")] + _WS("Zf"),
    "ssd_conv3x3_wino_fwd_pool": _POOL + [("planes_keep", "p")] + _WS("Zf"),
    "ssd_conv3x3_wino_fwd_pool_bits": _POOL + [("planes_keep", "p"), ("relu_bits_out", "b")] + _WS("Zf"),
    # valid call: the unpooled form (y given); y_pooled and argmax are the optional ones
    "ssd_conv3x3_wino_fwd_from_planes": [("planes", "P"), ("U_fwd", "P"), ("bias", "p"), ("y", "P"), ("ldy", "i", 64), ("y_pooled", "n"),
                                         ("argmax", "a"), ("g", "G"), ("relu", "i", 1), ("ceil_mode", "i", 0)] + _WS("Zf"),
    "ssd_conv3x3_wino_dgrad": [("dy", "P"), ("ldy", "i", 64), ("U_bwd", "P"), ("Co_pad", "i", 64), ("dx", "P"), ("relu_mask", "p"),
                               ("accumulate", "i", 0), ("g", "G"), ("mo", "i", 4)] + _WS("Zd"),
    "ssd_conv3x3_wino_dgrad_bits": [("dy", "P"), ("ldy", "i", 64), ("U_bwd", "P"), ("Co_pad", "i", 64), ("dx", "P"), ("relu_bits", "B"),
                                    ("accumulate", "i", 0), ("g", "G")] + _WS("Zd"),
    "ssd_conv3x3_wino_dgrad_planes": [("dy_planes", "P"), ("U_bwd", "P"), ("Co_pad", "i", 64), ("dx", "P"), ("relu_mask", "p"),
                                      ("accumulate", "i", 0), ("g", "G")] + _WS("Zd"),
    "ssd_conv3x3_wino_dgrad_planes_bits": [("dy_planes", "P"), ("U_bwd", "P"), ("Co_pad", "i", 64), ("dx", "P"), ("relu_bits", "B"),
                                           ("accumulate", "i", 0), ("g", "G")] + _WS("Zd"),
    "ssd_conv3x3_wino_wgrad": [("x", "P"), ("dy", "P"), ("ldy", "i", 64), ("dw_oihw", "P"), ("dbias", "u", OK_PTR), ("g", "G"),
                               ("mo", "i", 4)] + _WS("Zw"),
    "ssd_conv3x3_wino_wgrad_planes": [("planes", "P"), ("dy", "P"), ("ldy", "i", 64), ("dw_oihw", "P"), ("dbias", "u", OK_PTR), ("g", "G"),
                                      ("dgrad_planes_out", "p")] + _WS("Zw"),
    "ssd_conv3x3_wino_wgrad_planes_pooled": [("planes", "P")] + _POOLED_SRC + [("dw_oihw", "P"), ("dbias", "u", OK_PTR), ("g", "G"),
                                                                             ("dgrad_planes_out", "p")] + _WS("Zw"),
    "ssd_wino4_dy_transform": [("dy", "P"), ("ldy", "i", 64), ("g", "G"), ("wgrad_planes", "P"), ("dgrad_planes_out", "p"),
                               ("bias_partial", "p"), ("stream", "S")],
    "ssd_wino4_dy_transform_pooled": _POOLED_SRC + [("g", "G"), ("wgrad_planes", "P"), ("dgrad_planes_out", "p"), ("bias_partial", "p"),
                                                    ("stream", "S")],
    # bias_partial is required because dbias is asked for
    "ssd_wino4_wgrad_gemm": [("wgrad_planes", "P"), ("x_planes", "P"), ("ldy", "i", 64), ("bias_partial", "R"), ("dw_oihw", "P"),
                             ("dbias", "u", OK_PTR), ("g", "G")] + _WS("Zg"),
    # valid call: the forward filter only (U_bwd NULL), which makes U_fwd the required one
    "ssd_wino_weights": [("w_oihw", "R"), ("U_fwd", "R"), ("U_bwd", "u", None), ("Co", "i", 64), ("Ci", "i", 64), ("Co_pad", "i", 64),
                         ("mo", "i", 4), ("stream", "S")],
    "ssd_wino_weights_adj": [("w_oihw", "R"), ("U_adj", "R"), ("Co", "i", 64), ("Ci", "i", 64), ("Co_pad", "i", 64), ("stream", "S")],
    "ssd_conv3x3_wino_dgrad_adj_gemm": [("y_planes", "P"), ("ldy", "i", 64), ("U_adj", "P"), ("md_planes", "P"), ("g", "G"), ("stream", "S")],
    "ssd_wino4_adj_output": [("md_planes", "P"), ("dx", "P"), ("relu_mask", "p"), ("relu_bits", "b"), ("accumulate", "i", 0), ("g", "G"),
                             ("stream", "S")],
    "ssd_wino4_adj_output_to_planes": [("md_planes", "P"), ("relu_mask", "p"), ("relu_bits", "b"), ("g", "G"), ("g_below", "H"),
                                       ("y_planes", "P"), ("bias_partial", "p"), ("stream", "S")],
}

# ---- the defects an entry takes beyond those its argument kinds imply (a NULL for every required pointer and the geometry, a
# misaligned value for every pointer with an alignment rule, a workspace one byte short) -----------------------------------------------
# A defect is (label, {argument or "g.<make_geom argument>": value}).  Listed per entry are only defects that entry refuses: a
# value some entry accepts (ldy = 72 in the forward, dilation 4 outside the pooled and planes forms, Ci = 48 outside the forward) is
# no defect there.
_GEOM_ALL = [("5x5", {"g.k": 5, "g.pad": 2}), ("stride2", {"g.stride": 2}), ("pad2", {"g.pad": 2}), ("dil5", {"g.dil": 5, "g.pad": 5})]
_DIL4 = ("dil4", {"g.dil": 4, "g.pad": 4})
_CO62, _CI48, _CI62 = ("Co62", {"g.co": 62}), ("Ci48", {"g.ci": 48}), ("Ci62", {"g.ci": 62})
_MO3 = ("mo3", {"mo": 3})


def _ints(name, *values):
    return [(f"{name}{v}", {name: v}) for v in values]


_LDY_FWD = _ints("ldy", 60, 66)                              # below Co; no multiple of 4
_LDY_ALL = _ints("ldy", 60, 66, 72)                          # ... and a multiple of 4 but not of 32 / not Co itself
_CO_PAD = _ints("Co_pad", 32, 66, 72)                        # below Co; no multiple of 4; no multiple of 32

EXTRA = {
    "ssd_conv3x3_wino_fwd": _GEOM_ALL + [_CI48, _MO3] + _LDY_FWD,
    "ssd_conv3x3_wino_fwd_keep": _GEOM_ALL + [_CI48] + _LDY_FWD,
    "ssd_conv3x3_wino_fwd_keep_bits": _GEOM_ALL + [_CI48] + _LDY_FWD,
    "ssd_conv3x3_wino_fwd_pool": _GEOM_ALL + [_DIL4, _CO62, _CI48],
    "ssd_conv3x3_wino_fwd_pool_bits": _GEOM_ALL + [_DIL4, _CO62, _CI48],
    "ssd_conv3x3_wino_fwd_from_planes": _GEOM_ALL + [_DIL4, _CO62, _CI48] + _LDY_FWD,
    "ssd_conv3x3_wino_dgrad": _GEOM_ALL + [_CI62, _MO3] + _LDY_ALL + _CO_PAD,
    "ssd_conv3x3_wino_dgrad_bits": _GEOM_ALL + [_CI62] + _LDY_ALL + _CO_PAD,
    "ssd_conv3x3_wino_dgrad_planes": _GEOM_ALL + [_CI62] + _CO_PAD,
    "ssd_conv3x3_wino_dgrad_planes_bits": _GEOM_ALL + [_CI62] + _CO_PAD,
    "ssd_conv3x3_wino_wgrad": _GEOM_ALL + [_CI62, _MO3] + _LDY_FWD,
    "ssd_conv3x3_wino_wgrad_planes": _GEOM_ALL + [_CI62] + _LDY_FWD,
    "ssd_conv3x3_wino_wgrad_planes_pooled": _GEOM_ALL + [_DIL4, _CO62, _CI62] + _LDY_ALL + _ints("Hp", 4, 6),
    "ssd_wino4_dy_transform": _GEOM_ALL + _LDY_FWD,
    "ssd_wino4_dy_transform_pooled": _GEOM_ALL + [_DIL4, _CO62] + _LDY_ALL + _ints("Hp", 4, 6),
    "ssd_wino4_wgrad_gemm": _GEOM_ALL + [_CI62] + _LDY_FWD,
    "ssd_wino_weights": [_MO3] + _ints("Co_pad", 32),
    "ssd_wino_weights_adj": _ints("Co_pad", 32),
    "ssd_conv3x3_wino_dgrad_adj_gemm": _GEOM_ALL + [_DIL4, _CI62] + _LDY_ALL,
    "ssd_wino4_adj_output": _GEOM_ALL + [_DIL4, _CI62],
    "ssd_wino4_adj_output_to_planes": _GEOM_ALL + [_DIL4, _CI62],
}
assert set(EXTRA) == set(ENTRIES)


def defects(entry):
    """Every defect of one entry, in a fixed order: those its argument kinds imply, then EXTRA[entry]."""
    out = []
    for name, kind, *_ in ENTRIES[entry]:
        if kind in "PRBAWGH":
            out.append((f"null:{name}", {name: None}))
        if kind in "PpnBbW":
            out.append((f"odd:{name}", {name: ODD_PTR}))
        if kind in "Aa":
            out.append((f"odd:{name}", {name: ODD_BYTES}))
        if kind.startswith("Z"):
            out.append(("ws-1", {name: -1}))                 # relative to the queried size
    return out + EXTRA[entry]


def cases(entry):
    """[(label, {argument: value})]: every single defect and every pair that does not set one argument twice"""
    d = defects(entry)
    out = [(la, dict(ch)) for la, ch in d]
    for (la, ca), (lb, cb) in itertools.combinations(d, 2):
        if not set(ca) & set(cb):
            out.append((f"{la}+{lb}", {**ca, **cb}))
    return out


def arguments(entry, changes, sizes, make_geom, byref):
    """The ctypes arguments of `entry` for the valid call (`changes` empty) or a defective one.  sizes: {"Zf": bytes, ...} of the valid
    geometry; make_geom: ops.make_geom; byref: ctypes.byref.  The geometries are returned too: they must outlive the call."""
    geom = dict(GEOM, **{k[2:]: v for k, v in changes.items() if k.startswith("g.")})
    g, below = make_geom(**geom), make_geom(**dict(GEOM, co=GEOM["ci"]))
    args = []
    for name, kind, *value in ENTRIES[entry]:
        if name in changes and not kind.startswith("Z"):
            v = changes[name]
            args.append(v if kind not in "GH" else None)
        elif kind in "PpRBbAW":
            args.append(OK_PTR)
        elif kind in "naS":
            args.append(None)
        elif kind == "G":
            args.append(byref(g))
        elif kind == "H":
            args.append(byref(below))
        elif kind.startswith("Z"):
            args.append(sizes[kind] + changes.get(name, 0))
        else:
            args.append(value[0])
    return args, (g, below)


def _sizes(lib, make_geom, byref):
    g = byref(make_geom(**GEOM))
    return {"Zf": lib.ssd_conv3x3_wino_workspace(g, 0, 4), "Zd": lib.ssd_conv3x3_wino_workspace(g, 1, 4),
            "Zw": lib.ssd_conv3x3_wino_wgrad_workspace(g, 64, 4), "Zg": lib.ssd_wino4_wgrad_gemm_workspace(g, 64)}


def statuses(lib, make_geom, byref):
    """{entry: {label: status}} of the loaded library, over every case"""
    sizes = _sizes(lib, make_geom, byref)
    assert all(v > 0 for v in sizes.values()), sizes
    out = {}
    for entry in ENTRIES:
        fn = getattr(lib, entry)
        out[entry] = {}
        for label, changes in cases(entry):
            args, keep = arguments(entry, changes, sizes, make_geom, byref)
            out[entry][label] = fn(*args)
    return out


def _record():
    """Write the fixture from the importable library.  Refuses where a GPU is present (a tuple the library accepted would be launched
    on made-up pointers) and where the library accepts any tuple: 0, or SSD_ERR_LAUNCH (-4) from the launch that fails without a GPU."""
    import ctypes
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from objectdetection_ssd_amd import _lib, ops
    if torch.cuda.is_available():
        raise SystemExit("record on a machine without a GPU")
    got = statuses(_lib.load(), ops.make_geom, ctypes.byref)
    accepted = [(e, la, s) for e, d in got.items() for la, s in d.items() if s in (0, -4)]
    if accepted:
        raise SystemExit("accepted, so no defect of that entry:\n" + "\n".join(f"  {e} {la}: {s}" for e, la, s in accepted))
    with open(FIXTURE, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(d) for d in got.values())} cases of {len(got)} entries -> {FIXTURE}")


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        _record()
