"""What the device JPEG decoder (csrc/jpeg.hip, csrc/jpeg_split.hip) costs per batch, against the host decoder it replaces, and what it
costs a train step.

    python tools/jpeg_decode_bench.py [--windows 7] [--launches 10] [--steps 6] [--no-step] [--entropy both|segment|split]
                                      [--subsequence-bytes 64,128,256,512] [--out profiles/jpeg_split_bench.json]

1. Decode of synthetic VOC-sized images (500 x 375, quality 75, 4:2:0), batch 32 and 256, streams resident in the device arena:
     leg a   no restart markers: one segment per image
     leg b   Pillow's restart_marker_rows=1: one segment per MCU row, 24 per image
   with the entropy decode of the parent ("segment": one lane per restart segment) beside the new one ("split": many lanes per segment,
   at ops.JPEG_SUBSEQUENCE_BYTES, and on leg a of batch 32 at every size of --subsequence-bytes).  "call" is ops.jpeg_decode_
   (descriptor upload, two memsets, the kernels) between device events; "entropy", "idct", "colour" are the stages launched alone
   through the C entry's `stages` argument with the descriptors already on the device ("entropy" of "split" is its four kernels: plan,
   de-stuff, synchronise, write).  The yardstick is Pillow decoding the SAME bytes on a 16-thread pool in this process (host clock).
   Interleaved: every window runs every form once; medians over the windows; two clock probes bracket the section.
2. The restart interval swept on the same images (batch 32; 32 to 384 MCUs per segment, a row being 32, and none): "segment" against
   "split" per segment length -- what ops.JPEG_SPLIT_AUTO_BYTES is read from.
3. The batch-32 bf16 train step alone, and with the decode of the next batch (leg a under either entropy decode, leg b) enqueued on a
   side stream before each step; host clock around a window of steps that ends in a device synchronise.

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
SWEEP_MCUS = (32, 40, 48, 56, 64, 96, 128, 192, 256, 384)     # MCUs per restart segment (a row has 32); 0 = no restart markers


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
        legs = {}
        for mcus in (0,) + SWEEP_MCUS:
            b = io.BytesIO()
            Image.fromarray(px).save(b, "JPEG", quality=75, subsampling="4:2:0", **({"restart_marker_blocks": mcus} if mcus else {}))
            legs[mcus] = b.getvalue()
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
        self.d_dev = self.s_dev = None
        self.ws = {}
        self.status = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.stream_bytes = int(sum(h.data_end - h.data_begin for h in rb.headers))
        self.longest_segment = int(max(max(np.diff(list(h.seg_offsets) + [h.data_end + 2])) - 2 for h in rb.headers))

    def call(self, entropy="segment", sub=None):
        return ops.jpeg_decode_(self.arena, self.descs, self.segs, entropy=entropy, subsequence_bytes=sub)

    def _workspace(self, entropy, sub):
        key = (entropy, sub)
        if key not in self.ws:
            if entropy == "split":
                n = self.lib.ssd_jpeg_decode_split_workspace(C.byref(self.descs), self.B, self.segs.ctypes.data, int(self.segs.size), sub)
            else:
                n = self.lib.ssd_jpeg_decode_workspace(C.byref(self.descs), self.B)
            self.ws[key] = torch.empty(n, dtype=torch.uint8, device=self.arena.device)
            self.d_dev = torch.from_numpy(np.frombuffer(bytes(self.descs), np.uint8).copy()).to(self.arena.device)
            self.s_dev = torch.from_numpy(self.segs).to(self.arena.device)
        return self.ws[key]

    def stage(self, stages, entropy="segment", sub=None):
        sub = ops.JPEG_SUBSEQUENCE_BYTES if sub is None else sub
        ws = self._workspace(entropy, sub)
        args = (self.arena.data_ptr(), self.arena.numel(), self.d_dev.data_ptr(), C.byref(self.descs), self.s_dev.data_ptr(),
                self.segs.ctypes.data, int(self.segs.size), self.B, self.status.data_ptr(), ws.data_ptr(), ws.numel(), stages,
                torch.cuda.current_stream().cuda_stream)
        if entropy == "split":
            _lib.check(self.lib.ssd_jpeg_decode_split_u8(*args, sub, None), "jpeg split stage")
        else:
            _lib.check(self.lib.ssd_jpeg_decode_u8(*args), "jpeg stage")


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


def checked_batch(blobs, dev, name, modes):
    b = Batch(blobs, dev)
    ref = pillow_decode(b.blobs[1])
    for entropy in modes:
        b.arena[b.descs[1].dst_offset:b.descs[1].dst_offset + H * W * 3].zero_()
        st = b.call(entropy)
        got = b.arena[b.descs[1].dst_offset:b.descs[1].dst_offset + H * W * 3].cpu().numpy().reshape(H, W, 3)
        if st.any().item() or not np.array_equal(got, ref):
            raise SystemExit(f"{name} ({entropy}): the decoder does not reproduce Pillow; nothing to time")
    return b


def decode_section(a, dev, imgs):
    pool = cf.ThreadPoolExecutor(16)
    batches = {}
    for bs in (32, 256):
        for mcus, name in ((0, "a_no_restart"), (32, "b_restart_rows_1")):
            batches[(bs, name)] = checked_batch([imgs[i % DISTINCT][mcus] for i in range(bs)], dev, f"{name} batch {bs}", a.modes)
    forms = {}                                                      # name -> fn(batch); None = the Pillow pool
    for e in a.modes:
        forms[f"call_{e}"] = lambda b, e=e: b.call(e)
        forms[f"entropy_{e}"] = lambda b, e=e: b.stage(ops.JPEG_ENTROPY, e)
    forms["idct"] = lambda b: b.stage(ops.JPEG_IDCT, a.modes[0])
    forms["colour"] = lambda b: b.stage(ops.JPEG_COLOUR, a.modes[0])
    sized = {}
    if "split" in a.modes:
        for sub in a.subs:
            sized[f"call_split_{sub}"] = lambda b, sub=sub: b.call("split", sub)
            sized[f"entropy_split_{sub}"] = lambda b, sub=sub: b.stage(ops.JPEG_ENTROPY, "split", sub)

    def forms_of(key):
        return dict(forms, **sized) if key == (32, "a_no_restart") else forms
    ms = {(k, f): [] for k in batches for f in list(forms_of(k)) + ["pillow_16_threads"]}
    for key, b in batches.items():                                  # warm every form
        for fn in forms_of(key).values():
            fn(b); fn(b)
        list(pool.map(pillow_decode, b.blobs[:32]))
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for _ in range(a.windows):
        for key, b in batches.items():
            for f, fn in forms_of(key).items():
                ms[(key, f)].append(event_ms(lambda: fn(b), a.launches))
            t0 = time.perf_counter()
            list(pool.map(pillow_decode, b.blobs))
            ms[(key, "pillow_16_threads")].append((time.perf_counter() - t0) * 1e3)
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    for (bs, name), b in batches.items():
        fs = list(forms_of((bs, name))) + ["pillow_16_threads"]
        row = {"what": f"jpeg_decode_{name}_b{bs}", "images": bs, "size": [H, W], "quality": 75, "sampling": "4:2:0",
               "entropy_coded_bytes_per_image": b.stream_bytes // bs, "segments_per_image": int(b.descs[0].n_segments),
               "longest_segment_bytes": b.longest_segment, "default_subsequence_bytes": ops.JPEG_SUBSEQUENCE_BYTES,
               "ms": {f: stats(ms[((bs, name), f)]) for f in fs},
               "images_per_s_pillow_16_threads": round(bs / median(ms[((bs, name), "pillow_16_threads")]) * 1e3),
               "windows": a.windows, "launches_per_window": a.launches}
        for e in a.modes:
            row[f"images_per_s_device_call_{e}"] = round(bs / median(ms[((bs, name), f"call_{e}")]) * 1e3)
        emit(row)
    emit({"what": "jpeg_decode_section_clock", "shader_mhz_average": None if clock != clock else round(clock),
          "host_threads_of_the_pillow_pool": 16})
    pool.shutdown()
    return batches


def sweep_section(a, dev, imgs):
    """"segment" against "split" (default subsequence size) as the restart interval of the same images grows"""
    batches = {mcus: checked_batch([imgs[i % DISTINCT][mcus] for i in range(32)], dev, f"sweep {mcus} MCUs", a.modes)
               for mcus in SWEEP_MCUS + (0,)}
    ms = {(mcus, e): [] for mcus in batches for e in a.modes}
    for b in batches.values():
        for e in a.modes:
            b.call(e); b.call(e)
    torch.cuda.synchronize()
    for _ in range(a.windows):
        for mcus, b in batches.items():
            for e in a.modes:
                ms[(mcus, e)].append(event_ms(lambda: b.call(e), a.launches))
    for mcus, b in batches.items():
        emit({"what": "jpeg_decode_restart_sweep_b32", "mcus_per_segment": mcus or None, "segments_per_image": int(b.descs[0].n_segments),
              "longest_segment_bytes": b.longest_segment, "subsequence_bytes": ops.JPEG_SUBSEQUENCE_BYTES,
              "ms_call": {e: stats(ms[(mcus, e)]) for e in a.modes}, "windows": a.windows, "launches_per_window": a.launches})


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

    def with_decode(b, entropy):
        def fn():
            with torch.cuda.stream(side):
                b.call(entropy)
            step()
        return fn
    forms = {"step_alone": step}
    for e in a.modes:
        forms[f"step_with_decode_a_{e}"] = with_decode(batches[(32, "a_no_restart")], e)
    forms["step_with_decode_b_segment"] = with_decode(batches[(32, "b_restart_rows_1")], a.modes[0])
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
    ap.add_argument("--entropy", choices=("both", "segment", "split"), default="both", help="which entropy decode(s) to time")
    ap.add_argument("--subsequence-bytes", default="64,128,256,512", help="sizes of the split decode on the no-restart batch of 32")
    ap.add_argument("--no-sweep", action="store_true", help="skip the restart-interval sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_split_bench.json"))
    a = ap.parse_args()
    a.modes = ("segment", "split") if a.entropy == "both" else (a.entropy,)
    a.subs = [int(v) for v in a.subsequence_bytes.split(",") if v]
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_decode_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    t_end = time.time() + 3.0                                        # spin-up, as bench.py does before it times anything
    spin = torch.randn(4096, 4096, device=dev)
    while time.time() < t_end:
        spin = (spin @ spin).clamp_(-1, 1)
    torch.cuda.synchronize()
    imgs = images()
    batches = decode_section(a, dev, imgs)
    if not a.no_sweep:
        sweep_section(a, dev, imgs)
    if not a.no_step:
        step_section(a, dev, batches)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/jpeg_decode_bench.py", "device": torch.cuda.get_device_name(0), "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
