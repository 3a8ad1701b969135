"""What composing mosaics on the device costs, against the plain resize of the same sources.

    python tools/mosaic_bench.py [--windows 7] [--launches 20] [--parent-lib PATH] [--out profiles/mosaic_bench.json]

Synthetic 500 x 375 sources (random pixels, identity plans) already in HBM, output 300 x 300:
     a   a mosaic batch of 32: 128 sources, four tiles per image around centres drawn in (0.25, 0.75) of the frame, one call of
         ops.preprocess_tiles_u8
     b   ops.preprocess_u8 over the same 128 sources, each to a full 300 x 300 image
     c   ops.preprocess_u8 over 32 of them: a plain batch of 32
"call" is the ops function (descriptor upload, output allocation, three kernels) between device events; "kernels" is the C entry alone
with the descriptors, the output and the workspace already on the device.  Interleaved in one process: every window runs every form
once; medians over the windows; two clock probes bracket the timed section.  (a) reads the sources (b) reads, computes a narrower
horizontal pass and writes a quarter of (b)'s output, so (a) must not exceed (b): the file records whether it holds.  Where (a) sits
against (c) is reported, not set in advance.  --parent-lib: a libssd_gfx950.so built from the parent commit, loaded beside this build's;
its ssd_preprocess_u8 runs (b) and (c) in the same windows into the same buffers ("kernels_parent"): the existing entry must cost what
it cost.

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

H, W = 375, 500
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


def image_descs(rb, n):
    descs = (_lib.ImageDesc * n)()
    for d, p, o in zip(descs, rb.plans, rb.offsets):
        d.src_offset, d.src_h, d.src_w = o, p.src_h, p.src_w
        d.canvas_h, d.canvas_w, d.place_top, d.place_left = p.canvas
        d.crop_top, d.crop_left, d.crop_h, d.crop_w = p.crop
    return descs


class Resident:
    """one form with everything on the device: the C entry alone"""

    def __init__(self, arena, descs, n_images, tiles, lib=None, buffers_of=None):
        self.lib, self.arena, self.descs, self.n, self.tiles = lib or _lib.load(), arena, descs, n_images, tiles
        self.dev = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).to(arena.device)
        query = self.lib.ssd_preprocess_tiles_workspace if tiles else self.lib.ssd_preprocess_workspace
        nbytes = query(C.byref(descs), len(descs), n_images, *OUT) if tiles else query(C.byref(descs), len(descs), *OUT)
        if buffers_of is not None:                                   # the same output and workspace: where they lie is part of the time
            assert buffers_of.ws.numel() == nbytes
            self.ws, self.out = buffers_of.ws, buffers_of.out
        else:
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=arena.device)
            self.out = torch.empty((n_images, 3) + OUT, dtype=torch.float32, device=arena.device)
        self.m, self.s, self.f = (C.c_float * 3)(*Dataset.MEAN), (C.c_float * 3)(*Dataset.STD), (C.c_uint8 * 3)(*Dataset.FILLER_U8)

    def __call__(self):
        tail = (OUT[0], OUT[1], C.addressof(self.m), C.addressof(self.s), C.addressof(self.f), self.out.data_ptr(), self.ws.data_ptr(),
                self.ws.numel(), torch.cuda.current_stream().cuda_stream)
        if self.tiles:
            st = self.lib.ssd_preprocess_tiles_u8(self.arena.data_ptr(), self.dev.data_ptr(), C.byref(self.descs), len(self.descs), self.n, *tail)
        else:
            st = self.lib.ssd_preprocess_u8(self.arena.data_ptr(), self.dev.data_ptr(), C.byref(self.descs), len(self.descs), *tail)
        _lib.check(st, "mosaic_bench")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libssd_gfx950.so, for (b) and (c) through its entry")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mosaic_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mosaic_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    t_end = time.time() + 3.0                                        # spin-up, as bench.py does before it times anything
    spin = torch.randn(4096, 4096, device=dev)
    while time.time() < t_end:
        spin = (spin @ spin).clamp_(-1, 1)
    torch.cuda.synchronize()

    rng = np.random.default_rng(0)
    distinct = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(16)]
    rb = Dataset.pack_batch([distinct[i % 16] for i in range(128)])
    arena = rb.arena.to(dev)
    descs128, descs32 = image_descs(rb, 128), image_descs(rb, 32)
    draw = random.Random(0)
    tiles = (_lib.TileDesc * 128)()
    centres = []
    for i in range(32):
        cx, cy = draw.randint(int(0.25 * OUT[1]), int(0.75 * OUT[1])), draw.randint(int(0.25 * OUT[0]), int(0.75 * OUT[0]))
        centres.append((cx, cy))
        for k, (top, left, h, w) in enumerate(((0, 0, cy, cx), (0, cx, cy, OUT[1] - cx), (cy, 0, OUT[0] - cy, cx), (cy, cx, OUT[0] - cy, OUT[1] - cx))):
            t = tiles[4 * i + k]
            t.src = descs128[4 * i + k]
            t.out_image, t.dst_top, t.dst_left, t.dst_h, t.dst_w = i, top, left, h, w
    args = (OUT, Dataset.MEAN, Dataset.STD, Dataset.FILLER_U8)
    # nothing to time unless the mosaic is right: image 0 against the full-frame resize of its sources' tiles, one by one
    got = ops.preprocess_tiles_u8(arena, tiles, 32, *args)
    for k in range(4):
        t = tiles[k]
        one = (_lib.TileDesc * 1)(t)
        one[0].out_image, one[0].dst_top, one[0].dst_left = 0, 0, 0
        want = ops.preprocess_tiles_u8(arena, one, 1, (t.dst_h, t.dst_w), *args[1:])
        if not torch.equal(got[0, :, t.dst_top:t.dst_top + t.dst_h, t.dst_left:t.dst_left + t.dst_w], want[0]):
            raise SystemExit("the mosaic's tiles are not the resizes of their sources; nothing to time")
    full = (_lib.TileDesc * 1)()
    full[0].src = descs128[0]
    full[0].dst_h, full[0].dst_w = OUT
    if not torch.equal(ops.preprocess_tiles_u8(arena, full, 1, *args)[0], ops.preprocess_u8(arena, descs32, *args)[0]):
        raise SystemExit("a full-frame tile is not the plain resize; nothing to time")

    forms = {
        "a_mosaic_32_call": lambda: ops.preprocess_tiles_u8(arena, tiles, 32, *args),
        "b_plain_128_call": lambda: ops.preprocess_u8(arena, descs128, *args),
        "c_plain_32_call": lambda: ops.preprocess_u8(arena, descs32, *args),
        "a_mosaic_32_kernels": Resident(arena, tiles, 32, True),
        "b_plain_128_kernels": Resident(arena, descs128, 128, False),
        "c_plain_32_kernels": Resident(arena, descs32, 32, False),
    }
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        for name in ("ssd_preprocess_workspace", "ssd_preprocess_u8"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        forms["b_plain_128_kernels"]()
        want = forms["b_plain_128_kernels"].out.clone()
        forms["b_plain_128_kernels_parent"] = Resident(arena, descs128, 128, False, parent, forms["b_plain_128_kernels"])
        forms["c_plain_32_kernels_parent"] = Resident(arena, descs32, 32, False, parent, forms["c_plain_32_kernels"])
        forms["b_plain_128_kernels_parent"].out.zero_()
        forms["b_plain_128_kernels_parent"]()
        if not torch.equal(forms["b_plain_128_kernels_parent"].out, want):
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
    src_bytes, out_bytes = H * W * 3, 3 * OUT[0] * OUT[1] * 4
    shape = {"a": (128, 32), "b": (128, 128), "c": (32, 32)}
    for name in forms:
        n_src, n_out = shape[name[0]]
        m = median(ms[name])
        emit({"what": name, "sources": n_src, "source_size": [H, W], "output_images": n_out, "output_size": list(OUT), "ms": stats(ms[name]),
              "output_images_per_s": round(n_out / m * 1e3), "sources_per_s": round(n_src / m * 1e3),
              "bytes_read_sources_plus_written_output": n_src * src_bytes + n_out * out_bytes,
              "windows": a.windows, "launches_per_window": a.launches})
    summary = {"what": "mosaic_against_plain", "shader_mhz_average": None if clock != clock else round(clock),
               "mosaic_centres_first_4": centres[:4]}
    for kind in ("call", "kernels"):
        ma, mb, mc = (median(ms[f"{k}_{kind}"]) for k in ("a_mosaic_32", "b_plain_128", "c_plain_32"))
        summary[kind] = {"a_ms": round(ma, 4), "b_ms": round(mb, 4), "c_ms": round(mc, 4), "a_over_b": round(ma / mb, 3),
                         "a_over_c": round(ma / mc, 3), "a_not_above_b": bool(ma <= mb)}
    if a.parent_lib:
        summary["existing_entry_against_parent"] = {
            k: {"this_ms": round(median(ms[f"{k}_kernels"]), 4), "parent_ms": round(median(ms[f"{k}_kernels_parent"]), 4),
                "parent_window_spread_ms": round(max(ms[f"{k}_kernels_parent"]) - min(ms[f"{k}_kernels_parent"]), 4)}
            for k in ("b_plain_128", "c_plain_32")}
    emit(summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/mosaic_bench.py", "device": torch.cuda.get_device_name(0), "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
