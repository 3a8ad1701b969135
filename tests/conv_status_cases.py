"""The argument tuples of tests/test_conv_status_cpu.py: for every exported entry point of the direct convolution (csrc/conv_igemm.hip,
csrc/conv_wgrad.hip), one valid call on a small geometry and the defects that entry takes beyond those its argument kinds imply.
tests/status_grid.py explains the argument kinds and turns the tables into the grid of single defects and pairs; the recorded
statuses are tests/golden/conv_status.json (`python tests/conv_status_cases.py --record`, on a machine without a GPU).
"""
from status_grid import OK_PTR, Grid

# ops.make_geom arguments of the valid call: 2 x 10 x 10 x 64 -> 64 channels, 3x3 / stride 1 / pad 1 ...
GEOM = dict(n=2, h=10, w=10, ci=64, co=64, k=3, stride=1, pad=1, dil=1)
# ... and of the halo entries', which answer 1 ("not a halo case") on a map below 30 x 30
HALO_GEOM = dict(GEOM, n=1, h=32, w=32)

_TAIL = [("stream", "S")]
_WS = [("workspace", "p"), ("workspace_bytes", "i", 1 << 20)] + _TAIL            # optional: too small a one only means no K slices
_WGRAD_WS = [("workspace", "W"), ("workspace_bytes", "Zw")] + _TAIL


def _fwd(src="P"):
    return [("x", src), ("w_ohwi", src), ("bias", "u", OK_PTR), ("y", "R"), ("ldy", "i", 64), ("g", "G"), ("relu", "i", 1)]


def _fwd3(src):                                                                  # limb planes: w_rows follows them
    f = _fwd(src)
    return f[:2] + [("w_rows", "i", 64)] + f[2:]


def _dgrad(src="P"):
    return [("dy", src), ("ldy", "i", 64), ("w_ihwo", src), ("Co_pad", "i", 64), ("dx", "R"), ("relu_mask", "u", OK_PTR),
            ("accumulate", "i", 0), ("g", "G")]


_WGRAD = [("x", "P"), ("dy", "P"), ("ldy", "i", 64), ("dw_oihw", "R"), ("dbias", "u", OK_PTR), ("g", "G")] + _WGRAD_WS

ENTRIES = {
    "ssd_conv2d_fwd": _fwd() + _TAIL,
    "ssd_conv2d_fwd_ws": _fwd() + _WS,
    "ssd_conv2d_fwd_bf16": _fwd() + _TAIL,
    "ssd_conv2d_fwd_bf16_ws": _fwd() + _WS,
    "ssd_conv2d_fwd_accum": _fwd() + _TAIL,
    "ssd_conv2d_fwd_accum_bf16": _fwd() + _TAIL,
    "ssd_conv2d_fwd_x3": _fwd3("P") + _TAIL,
    "ssd_conv2d_dgrad": _dgrad() + _TAIL,
    "ssd_conv2d_dgrad_ws": _dgrad() + _WS,
    "ssd_conv2d_dgrad_bf16": _dgrad() + _TAIL,
    "ssd_conv2d_dgrad_bf16_ws": _dgrad() + _WS,
    "ssd_conv2d_dgrad_x3": _dgrad() + _TAIL,
    # recorded before these two had an alignment rule: test_conv_status_cpu.py holds them to it apart from the grid
    "ssd_conv3x3_halo_fwd_bf16": _fwd3("R") + _TAIL,
    "ssd_conv3x3_halo_dgrad_bf16": _dgrad("R") + _TAIL,
    # the size query covers the bf16 plan too, which wants more on this geometry: one byte less still holds the f32 plan
    "ssd_conv2d_wgrad": _WGRAD[:-2] + [("workspace_bytes", "i", 1 << 24)] + _TAIL,
    "ssd_conv2d_wgrad_bf16": _WGRAD,
    "ssd_conv3x3_wgrad_bf16t": _WGRAD,
}

# ---- the defects an entry takes beyond those its argument kinds imply.  Listed per entry are only defects that entry refuses: a
# value some entry accepts (Ci = 48 outside the forward, ldy = 66 in the forward, a contradictory Ho in the weight gradient) is no
# defect there.  No two values of a pair make up for each other (ldy = Co_pad = 96 would be a valid data gradient).
_HO = ("Ho+1", {"g.Ho": 11})                                 # the geometry contradicts itself
_HALO_HO = ("Ho+1", {"g.Ho": 33})
_HUGE = ("huge", {"g.n": 1 << 19})                           # a source beyond what a 32-bit buffer offset reaches
_CI48, _CI62 = ("Ci48", {"g.ci": 48}), ("Ci62", {"g.ci": 62})


def _ints(name, *values):
    return [(f"{name}{v}", {name: v}) for v in values]


_FWD_X = [_HO, _HUGE, _CI48, _CI62] + _ints("ldy", 60)                             # ldy below Co
_DGRAD_X = [_HO, _HUGE, _CI62] + _ints("ldy", 60, 66, 96) + _ints("Co_pad", 32, 72)    # ldy != Co_pad; Co_pad below Co, no multiple of 32
_WGRAD_X = [_CI62] + _ints("ldy", 60, 66)                                          # ldy below Co, no multiple of 4

EXTRA = {e: _FWD_X for e in ENTRIES if "_fwd" in e}
EXTRA.update({e: _DGRAD_X for e in ENTRIES if "_dgrad" in e})
EXTRA.update({e: _WGRAD_X for e in ENTRIES if "_wgrad" in e})
EXTRA["ssd_conv2d_fwd_x3"] = _FWD_X + _ints("w_rows", 32)                          # limb planes with fewer rows than Co
EXTRA["ssd_conv3x3_halo_fwd_bf16"] = [_HALO_HO] + _FWD_X[1:] + _ints("w_rows", 32)
EXTRA["ssd_conv3x3_halo_dgrad_bf16"] = [_HALO_HO] + _DGRAD_X[1:]

GEOM_OF = {"ssd_conv3x3_halo_fwd_bf16": HALO_GEOM, "ssd_conv3x3_halo_dgrad_bf16": HALO_GEOM}


def _sizes(lib, make_geom, byref):
    return {"Zw": lib.ssd_conv2d_wgrad_workspace(byref(make_geom(**GEOM)))}


GRID = Grid("conv_status.json", ENTRIES, EXTRA, GEOM, _sizes, geom_of=GEOM_OF, valid_launches=True)

if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        GRID.record()
