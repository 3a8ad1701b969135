"""The argument tuples of tests/test_wino_status_cpu.py: for every exported Winograd entry point that takes pointers, one valid call on
a small geometry and the defects that entry takes beyond those its argument kinds imply.  tests/status_grid.py explains the argument
kinds and turns the tables into the grid of single defects and pairs; the recorded statuses are tests/golden/wino_status.json
(`python tests/wino_status_cases.py --record`, on a machine without a GPU).
"""
from status_grid import OK_PTR, Grid

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
def _sizes(lib, make_geom, byref):
    g = byref(make_geom(**GEOM))
    return {"Zf": lib.ssd_conv3x3_wino_workspace(g, 0, 4), "Zd": lib.ssd_conv3x3_wino_workspace(g, 1, 4),
            "Zw": lib.ssd_conv3x3_wino_wgrad_workspace(g, 64, 4), "Zg": lib.ssd_wino4_wgrad_gemm_workspace(g, 64)}


_GRID = Grid("wino_status.json", ENTRIES, EXTRA, GEOM, _sizes)
FIXTURE, defects, cases, arguments, statuses = _GRID.fixture, _GRID.defects, _GRID.cases, _GRID.arguments, _GRID.statuses

if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        _GRID.record()
