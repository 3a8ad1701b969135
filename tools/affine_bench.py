"""What the random affine warp costs on the device, against a copy of the same bytes and against the batch it follows.

    python tools/affine_bench.py [--windows 7] [--launches 20] [--parent-lib PATH] [--out profiles/affine_bench.json]

  1  ssd_affine_warp_f32 on a resident (32,3,300,300) float32 batch -- the C entry alone, matrices and output already on the device --
     with 32 matrices drawn in the dataset's default ranges ("warp_drawn") and with 32 identities ("warp_identity"), against
     Tensor.copy_ of the same tensor ("copy"), which reads and writes the same bytes.
  2  RawBatch.to of 32 resident 500 x 375 sources (the upload left out: the arena is on the device, the call is what .to() runs behind
     it), all 32 warped ("to_warped": resize, then ops.affine_warp) against none warped ("to_plain": the resize alone).  --parent-lib: a
     libssd_gfx950.so built from the parent commit, loaded beside this build's; its ssd_preprocess_u8 runs the none-warped batch in the
     same windows into the same buffers ("resize_kernels_parent" beside "resize_kernels"): the existing entry must cost what it cost.
Interleaved in one process: every window runs every form once; medians over the windows; two clock probes bracket the timed section.
No bar on any time: the file reports times and ratios.

Prints one JSON line per measurement and writes all of them to --out.
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from objectdetection_ssd_amd import Dataset, _lib, ops  # noqa: E402

B, H, W = 32, 375, 500
OUT = (300, 300)
RESULTS = []


def emit(d):
    RESULTS.append(d)
    print(json.dumps(d), flush=True)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v, digits=4):
    return {"median": round(median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_of_median": round((max(v) - min(v)) / median(v), 4)}


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


class Warp:
    """the C entry alone: input, output and matrices on the device"""

    def __init__(self, x, out, mats):
        self.lib, self.x, self.out, self.mats = _lib.load(), x, out, np.ascontiguousarray(mats, np.float32)
        self.dev = torch.from_numpy(self.mats.copy()).to(x.device)
        self.fill = (C.c_float * 3)(*Dataset.affine_fill())

    def __call__(self):
        n, _, h, w = self.x.shape
        _lib.check(self.lib.ssd_affine_warp_f32(self.x.data_ptr(), self.out.data_ptr(), self.dev.data_ptr(), self.mats.ctypes.data, n, h, w,
                                                C.addressof(self.fill), torch.cuda.current_stream().cuda_stream), "affine_bench")


class Resize:
    """ssd_preprocess_u8 alone, of this build's library or another's, descriptors, output and workspace on the device"""

    def __init__(self, arena, descs, lib=None, buffers_of=None):
        self.lib, self.arena, self.descs = lib or _lib.load(), arena, descs
        self.dev = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(arena.device)
        nbytes = self.lib.ssd_preprocess_workspace(C.byref(descs), len(descs), *OUT)
        if buffers_of is not None:                                   # the same output and workspace: where they lie is part of the time
            assert buffers_of.ws.numel() == nbytes
            self.ws, self.out = buffers_of.ws, buffers_of.out
        else:
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=arena.device)
            self.out = torch.empty((len(descs), 3) + OUT, dtype=torch.float32, device=arena.device)
        self.m, self.s, self.f = (C.c_float * 3)(*Dataset.MEAN), (C.c_float * 3)(*Dataset.STD), (C.c_uint8 * 3)(*Dataset.FILLER_U8)

    def __call__(self):
        _lib.check(self.lib.ssd_preprocess_u8(self.arena.data_ptr(), self.dev.data_ptr(), C.byref(self.descs), len(self.descs), OUT[0], OUT[1],
                                              C.addressof(self.m), C.addressof(self.s), C.addressof(self.f), self.out.data_ptr(),
                                              self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream), "affine_bench")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libssd_gfx950.so, for the none-warped resize through its entry")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("affine_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    t_end = time.time() + 3.0                                        # spin-up, as bench.py does before it times anything
    spin = torch.randn(4096, 4096, device=dev)
    while time.time() < t_end:
        spin = (spin @ spin).clamp_(-1, 1)
    torch.cuda.synchronize()

    rng = np.random.default_rng(0)
    distinct = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(16)]
    rb = Dataset.pack_batch([distinct[i % 16] for i in range(B)])
    arena = rb.arena.to(dev)
    descs = (_lib.ImageDesc * B)()
    for d, p, o in zip(descs, rb.plans, rb.offsets):
        d.src_offset, d.src_h, d.src_w = o, p.src_h, p.src_w
        d.canvas_h, d.canvas_w, d.place_top, d.place_left = p.canvas
        d.crop_top, d.crop_left, d.crop_h, d.crop_w = p.crop
    args = (OUT, Dataset.MEAN, Dataset.STD, Dataset.FILLER_U8)
    draw = random.Random(0)
    drawn = np.asarray([Dataset.plan_affine(OUT[1], OUT[0], draw)[1] for _ in range(B)], np.float32)
    ident = np.tile(np.asarray((1, 0, 0, 0, 1, 0), np.float32), (B, 1))
    fill = Dataset.affine_fill()

    x = ops.preprocess_u8(arena, descs, *args)
    out, dst = torch.empty_like(x), torch.empty_like(x)
    # nothing to time unless the warp is right: the identity is a copy, and a drawn warp leaves the frame's middle near its source
    if not torch.equal(ops.affine_warp(x, ident, fill), x):
        raise SystemExit("the identity warp is not a copy; nothing to time")
    moved = ops.affine_warp(x, drawn, fill)
    if torch.equal(moved, x) or not bool(torch.isfinite(moved).all()):
        raise SystemExit("a drawn warp changed nothing, or made something that is not finite; nothing to time")

    resize = Resize(arena, descs)
    forms = {
        "warp_drawn": Warp(x, out, drawn),
        "warp_identity": Warp(x, out, ident),
        "copy": lambda: dst.copy_(x),
        "to_plain": lambda: ops.preprocess_u8(arena, descs, *args),
        "to_warped": lambda: ops.affine_warp(ops.preprocess_u8(arena, descs, *args), drawn, fill),
        "resize_kernels": resize,
    }
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        for name in ("ssd_preprocess_workspace", "ssd_preprocess_u8"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        resize()
        want = resize.out.clone()
        forms["resize_kernels_parent"] = Resize(arena, descs, parent, resize)
        resize.out.zero_()
        forms["resize_kernels_parent"]()
        if not torch.equal(resize.out, want):
            raise SystemExit("this build's ssd_preprocess_u8 does not compute what the parent's computes")
    for fn in forms.values():
        fn(); fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    pa = ops.clock_probe(dev)
    for _ in range(a.windows):
        for name, fn in forms.items():
            ms[name].append(event_ms(fn, a.launches))
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    nbytes = x.numel() * 4
    for name in forms:
        d = {"what": name, "images": B, "output_size": list(OUT), "ms": stats(ms[name]), "windows": a.windows, "launches_per_window": a.launches}
        if name in ("warp_drawn", "warp_identity", "copy"):
            d["bytes_read_plus_written"] = 2 * nbytes
            d["tb_per_s_of_those_bytes"] = round(2 * nbytes / median(ms[name]) * 1e-9, 3)
        else:
            d["source_size"] = [H, W]
        emit(d)
    m = {k: median(v) for k, v in ms.items()}
    summary = {"what": "affine_warp_against_copy_and_resize", "shader_mhz_average": None if clock != clock else round(clock),
               "warp_drawn_ms": round(m["warp_drawn"], 4), "warp_identity_ms": round(m["warp_identity"], 4), "copy_ms": round(m["copy"], 4),
               "warp_drawn_over_copy": round(m["warp_drawn"] / m["copy"], 3), "warp_identity_over_copy": round(m["warp_identity"] / m["copy"], 3),
               "to_plain_ms": round(m["to_plain"], 4), "to_warped_ms": round(m["to_warped"], 4),
               "to_warped_over_to_plain": round(m["to_warped"] / m["to_plain"], 3)}
    if a.parent_lib:
        p = ms["resize_kernels_parent"]
        summary["existing_entry_against_parent"] = {"this_ms": round(m["resize_kernels"], 4), "parent_ms": round(median(p), 4),
                                                    "parent_window_spread_ms": round(max(p) - min(p), 4)}
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/affine_bench.py", "device": torch.cuda.get_device_name(0), "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
