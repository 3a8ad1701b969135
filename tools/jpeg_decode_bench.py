"""What the device JPEG decoder (csrc/jpeg.hip) costs per batch, against the host decoder it replaces, and what it costs a train step.

    python tools/jpeg_decode_bench.py [--windows 7] [--launches 10] [--steps 6] [--no-step] [--out profiles/jpeg_decode_bench.json]

1. Decode of synthetic VOC-sized images (500 x 375, quality 75, 4:2:0), batch 32 and 256, streams resident in the device arena:
     leg a   no restart markers: ONE lane per image decodes the entropy-coded data (the intended degradation)
     leg b   Pillow's restart_marker_rows=1: one lane per MCU row, 24 per image
   "call" is ops.jpeg_decode_ (descriptor upload, two memsets, three kernels) between device events; "entropy", "idct", "colour" are
   the three kernels launched alone through the C entry's `stages` argument with the descriptors already on the device.  The
   yardstick is Pillow decoding the SAME bytes on a 16-thread pool in this process (host clock).  Interleaved: every window runs
   every form once; medians over the windows; two clock probes bracket the section.
2. The batch-32 bf16 train step alone, and with the decode of the next batch (leg a, leg b) enqueued on a side stream before each
   step; host clock around a window of steps that ends in a device synchronise.

Prints one JSON line per measurement and writes all of them to --out.
"""
import argparse
import concurrent.futures as cf
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from objectdetection_ssd_amd import Dataset, Losses, Model, _lib, ops  # noqa: E402
from objectdetection_ssd_amd.ddp import FlatSGDDataParallel  # noqa: E402

H, W = 375, 500
DISTINCT = 16                # distinct images; a batch cycles through them
RESULTS = []


def emit(d):
    RESULTS.append(d)
    print(json.dumps(d), flush=True)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v, digits=3):
    return {"median": round(median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_of_median": round((max(v) - min(v)) / median(v), 4)}


def images(seed=0):
    """smooth structure plus texture noise: about the compressed size of a photograph at quality 75"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(DISTINCT):
        f = rng.uniform(0.01, 0.08, (3, 2))
        base = np.stack([127 + 90 * np.sin(xx * f[c, 0] + yy * f[c, 1] + c) for c in range(3)], -1)
        px = np.clip(base + rng.normal(0, 14, (H, W, 3)), 0, 255).astype(np.uint8)
        legs = []
        for kw in ({}, {"restart_marker_rows": 1}):
            b = io.BytesIO()
            Image.fromarray(px).save(b, "JPEG", quality=75, subsampling="4:2:0", **kw)
            legs.append(b.getvalue())
        out.append(legs)
    return out


class Batch:
    """B streams resident on the device, their descriptors and segment table on both sides"""

    def __init__(self, blobs, dev):
        rb = Dataset.pack_batch(blobs)
        self.blobs, self.B = blobs, len(blobs)
        self.arena = torch.empty(rb.device_bytes, dtype=torch.uint8, device=dev)
        first = min(rb.host_offsets)
        self.arena[rb.device_bytes - (rb.arena.numel() - first):] = rb.arena[first:].to(dev)
        self.descs = (_lib.JpegDesc * self.B)()
        segs = []
        for d, h, ho, o in zip(self.descs, rb.headers, rb.host_offsets, rb.offsets):
            ops.jpeg_fill_desc(d, h, rb.device_bytes - (rb.arena.numel() - first) + ho - first, o, h.height * h.width * 3, len(segs))
            segs.extend(int(s) - h.data_begin for s in h.seg_offsets)
        self.segs = np.asarray(segs, np.int32)
        self.lib = _lib.load()
        self.ws_bytes = self.lib.ssd_jpeg_decode_workspace(C.byref(self.descs), self.B)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.d_dev = torch.from_numpy(np.frombuffer(bytes(self.descs), np.uint8).copy()).to(dev)
        self.s_dev = torch.from_numpy(self.segs).to(dev)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.stream_bytes = int(sum(h.data_end - h.data_begin for h in rb.headers))

    def call(self):
        return ops.jpeg_decode_(self.arena, self.descs, self.segs)

    def stage(self, stages):
        _lib.check(self.lib.ssd_jpeg_decode_u8(self.arena.data_ptr(), self.arena.numel(), self.d_dev.data_ptr(), C.byref(self.descs),
                                               self.s_dev.data_ptr(), self.segs.ctypes.data, int(self.segs.size), self.B,
                                               self.status.data_ptr(), self.ws.data_ptr(), self.ws_bytes, stages,
                                               torch.cuda.current_stream().cuda_stream), "jpeg stage")


def pillow_decode(blob):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def decode_section(a, dev, imgs):
    pool = cf.ThreadPoolExecutor(16)
    batches = {}
    for bs in (32, 256):
        for leg, name in enumerate(("a_no_restart", "b_restart_rows_1")):
            b = Batch([imgs[i % DISTINCT][leg] for i in range(bs)], dev)
            st = b.call()
            ref = pillow_decode(b.blobs[1])
            got = b.arena[b.descs[1].dst_offset:b.descs[1].dst_offset + H * W * 3].cpu().numpy().reshape(H, W, 3)
            if st.any().item() or not np.array_equal(got, ref):
                raise SystemExit(f"{name} batch {bs}: the decoder does not reproduce Pillow; nothing to time")
            batches[(bs, name)] = b
    forms = ("call", "entropy", "idct", "colour", "pillow_16_threads")
    ms = {(k, f): [] for k in batches for f in forms}
    for b in batches.values():                                     # warm every form
        for _ in range(2):
            b.call(); b.stage(ops.JPEG_ENTROPY); b.stage(ops.JPEG_IDCT); b.stage(ops.JPEG_COLOUR)
        list(pool.map(pillow_decode, b.blobs[:32]))
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for _ in range(a.windows):
        for key, b in batches.items():
            ms[(key, "call")].append(event_ms(b.call, a.launches))
            ms[(key, "entropy")].append(event_ms(lambda: b.stage(ops.JPEG_ENTROPY), a.launches))
            ms[(key, "idct")].append(event_ms(lambda: b.stage(ops.JPEG_IDCT), a.launches))
            ms[(key, "colour")].append(event_ms(lambda: b.stage(ops.JPEG_COLOUR), a.launches))
            t0 = time.perf_counter()
            list(pool.map(pillow_decode, b.blobs))
            ms[(key, "pillow_16_threads")].append((time.perf_counter() - t0) * 1e3)
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    for (bs, name), b in batches.items():
        m = {f: median(ms[((bs, name), f)]) for f in forms}
        emit({"what": f"jpeg_decode_{name}_b{bs}", "images": bs, "size": [H, W], "quality": 75, "sampling": "4:2:0",
              "entropy_coded_bytes_per_image": b.stream_bytes // bs, "segments_per_image": int(b.descs[0].n_segments),
              "ms": {f: stats(ms[((bs, name), f)]) for f in forms},
              "images_per_s_device_call": round(bs / m["call"] * 1e3), "images_per_s_pillow_16_threads": round(bs / m["pillow_16_threads"] * 1e3),
              "windows": a.windows, "launches_per_window": a.launches})
    emit({"what": "jpeg_decode_section_clock", "shader_mhz_average": None if clock != clock else round(clock),
          "host_threads_of_the_pillow_pool": 16})
    pool.shutdown()
    return batches


def step_section(a, dev, batches):
    x, classes, boxes = bench.synth_batch(32, 1234, dev)
    torch.manual_seed(0)
    net = Model.SSD_300().to(dev).train()
    net.conv_dtype = "bf16"
    tr = FlatSGDDataParallel(net, lr=1e-4)
    side = torch.cuda.Stream()

    def step():
        tr.zero_grad()
        loc, conf = net(x)
        l1, l2, n_pos = Losses.ssd((loc, conf), classes, boxes, norm_mode=1, with_n_pos=True)
        (l1 + l2).backward()
        tr.reduce_and_step(n_pos)

    def with_decode(b):
        def fn():
            with torch.cuda.stream(side):
                b.call()
            step()
        return fn
    forms = {"step_alone": step, "step_with_decode_a": with_decode(batches[(32, "a_no_restart")]),
             "step_with_decode_b": with_decode(batches[(32, "b_restart_rows_1")])}
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    mhz = {k: [] for k in forms}
    for _ in range(a.windows):
        for name, fn in forms.items():
            fn()
            torch.cuda.synchronize()
            pa = ops.clock_probe(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            pb = ops.clock_probe(dev)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            mhz[name].append(ops.shader_mhz(pa, pb))
    for name in forms:
        m = median(mhz[name])
        emit({"what": f"train_step_b32_bf16_{name}", "ms_per_step": stats(ms[name]), "images_per_s": round(32 / median(ms[name]) * 1e3),
              "shader_mhz_median": None if m != m else round(m), "windows": a.windows, "steps_per_window": a.steps})
    tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--no-step", action="store_true", help="the decode section only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    t_end = time.time() + 3.0                                        # spin-up, as bench.py does before it times anything
    spin = torch.randn(4096, 4096, device=dev)
    while time.time() < t_end:
        spin = (spin @ spin).clamp_(-1, 1)
    torch.cuda.synchronize()
    batches = decode_section(a, dev, images())
    if not a.no_step:
        step_section(a, dev, batches)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/jpeg_decode_bench.py", "device": torch.cuda.get_device_name(0), "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
