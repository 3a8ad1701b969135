"""Convolution geometries of the bench steps and the host plan queries of the convolution dispatchers (shared by the exact-kernel tests)."""
import ctypes as C


def bench_geometries(variant, bs, n_confs):
    """(n, h, w, ci, co, k, stride, pad, dil) of every convolution of Model.build_ops(variant) at batch bs -- the walk of the engine's
    weight preparation (Model._Engine._prepare_weights_batched) -- with the heads' fused loc + conf rows for each conf width"""
    from objectdetection_ssd_amd import Model, ops
    hw = {"x": (variant, variant)}
    out = []
    for op in Model.build_ops(variant):
        kind = op["op"]
        if kind in ("conv_first", "l2norm"):
            hw[op["y"]] = hw[op["x"]]
        elif kind == "pool":
            h, w = hw[op["x"]]
            hw[op["y"]] = (ops.pool_out(h, op["k"], op["s"], op["pad"], op["ceil"]), ops.pool_out(w, op["k"], op["s"], op["pad"], op["ceil"]))
        elif kind == "conv":
            h, w = hw[op["x"]]
            g = ops.make_geom(bs, h, w, op["ci"], op["co"], op["k"], op["s"], op["pad"], op["dil"])
            hw[op["y"]] = (g.Ho, g.Wo)
            out.append((bs, h, w, op["ci"], op["co"], op["k"], op["s"], op["pad"], op["dil"]))
        elif kind == "head":
            h, w = hw[op["x"]]
            for nc in n_confs:
                out.append((bs, h, w, op["ci"], op["a"] * (4 + nc), 3, 1, 1, 1))
    return list(dict.fromkeys(out))


def wgrad_plan(geo, bf16):
    """ssd_conv2d_wgrad_plan: (kernel, tile, stages, f32 patch shape, bf16 form, nsplit, per split, tap reduction)"""
    from objectdetection_ssd_amd import _lib, ops
    g = ops.make_geom(*geo)
    pl = (C.c_int * 8)()
    _lib.check(_lib.load().ssd_conv2d_wgrad_plan(C.byref(g), int(bf16), pl), "wgrad_plan")
    return tuple(pl)


def bf16_plan(n, h, w, k, n_out):
    """ssd_conv3x3_bf16_plan: (position space, N tile, halo pieces, persistent)"""
    from objectdetection_ssd_amd import _lib
    pl = (C.c_int * 4)()
    _lib.check(_lib.load().ssd_conv3x3_bf16_plan(n, h, w, k, n_out, pl), "conv3x3_bf16_plan")
    return tuple(pl)


def halo_shape(geo, direction, planes):
    from objectdetection_ssd_amd import _lib, ops
    g = ops.make_geom(*geo)
    r = _lib.load().ssd_conv3x3_halo_shape(C.byref(g), direction, planes)
    assert r >= 0, r
    return r
