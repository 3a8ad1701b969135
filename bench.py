"""bench.py -- SSD300-VGG16 train step throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

One "step" = Model.SSD_300 forward + Losses.ssd (match, loss) + backward through every
kernel + ONE gradient all-reduce over RCCL (N > 1) + fused SGD, on one batch of 32
synthetic 300x300 images per GPU (BASELINE.json configs[1]; weak scaling), f32.
Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, the untimed spin-up, the warm-up and timed
steps, --dump-outputs, the line.  --full adds everything else the benchmark measures, each in runs
of its own after the timed steps (the live traffic passes before them):
  roofline     -- the dominant kernel (by summed time) of the step, timed per launch with HIP
                  events on the stream the kernels run on, against the f32-MFMA peak; its
                  `traffic` from two rocprofv3 --pmc child runs (--live-traffic);
  cpu_baseline -- the oracle's torch-CPU restatement of the same step on the host's cores
                  (rank 0, N=1 only, bounded sample), and loss_delta_vs_cpu;
  config.f32_mfma_only / bf16_operand_mode / graph_step -- the same step in other forms (N=1);
  config.host_enqueue_ms_per_step -- host time to enqueue one step.
The --no-cpu-baseline / --no-roofline / --no-bf16-leg / --live-traffic off switches trim a --full run.

--dump-outputs DIR writes what rank 0's last timed step returned as DIR/<name>.npy (float32 /
float64, under 64 MB; see dump_train_outputs).  The time-bounded spin-up leaves no SGD update
behind, so with the same arguments the warm-up and timed steps see the same weights, momentum and
batch on every run and two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

PER_GPU_BATCH = 32
TRAIN_GFLOP_PER_IMAGE = 187.930        # BASELINE.md section 3 (fwd + dgrad + wgrad, no dgrad for conv1_1)
PEAK_F32_MFMA_TFLOPS = 157.3           # MI355X_MICROARCH.md chip-level parameters
DUMP_MAX_BYTES = 64 << 20              # --dump-outputs: all files together
DUMP_SAMPLE = 1 << 21                  # --dump-outputs: elements of the parameter / gradient samples


def synth_batch(bs: int, seed: int, dev):
    """randn images; 1 + min(Poisson(1.4), 7) boxes per image."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(bs, 3, 300, 300, generator=g)
    rng = np.random.default_rng(seed)
    boxes, classes = [], []
    for _ in range(bs):
        n = 1 + min(int(rng.poisson(1.4)), 7)
        x1 = rng.uniform(0, .6, n); y1 = rng.uniform(0, .6, n)
        w = rng.uniform(.08, .6, n); h = rng.uniform(.08, .6, n)
        b = np.stack([x1, y1, np.minimum(x1 + w, 1.), np.minimum(y1 + h, 1.)], 1).astype(np.float32)
        boxes.append(torch.from_numpy(b).to(dev))
        classes.append(torch.from_numpy(rng.integers(0, 20, n).astype(np.float32)).to(dev))
    return x.to(dev), classes, boxes


_T0 = time.perf_counter()


def note(msg: str) -> None:
    """progress line on stderr (the JSON line on stdout stays the only stdout output): a run that prints nothing for minutes looks hung"""
    if os.environ.get("RANK", "0") == "0":
        print(f"[bench +{time.perf_counter() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def cpu_quota_cores():
    """CPUs the container's cgroup lets this process use at once (cpu.max / cfs quota), or None when unlimited / unknown."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else max(1, int(float(q) / float(per) + 0.999))
    except Exception:
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else max(1, (q + per - 1) // per)
    except Exception:
        return None


def host_cores():
    n = os.cpu_count() or 1
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        pass
    return n


_LIVE_PMC = None     # {"fetch": {kernel: (kb_sum, dispatches)}, "write": {...}, "note": str} from live_traffic_passes(), or None


def live_traffic_passes(argv_tail, timeout_s: float = 150.0):
    """HBM-side traffic of THIS invocation's kernels: two `rocprofv3 --pmc` passes (FETCH_SIZE; WRITE_SIZE -- separate passes, counters only,
    MI355X_MICROARCH.md section HBM) over a short run of this same file, started as CHILD processes before this process touches the GPU
    (one GPU user at a time; the program itself after `--`).  Returns per-kernel sums or a note saying why not.  Any failure -- no profiler
    on the box, a non-zero exit, the time limit -- leaves the committed file of the round as the source, and the line says so."""
    import csv
    import glob
    import re
    import shutil
    import signal
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"note": "rocprofv3 not found on this box"}
    tmp = tempfile.mkdtemp(prefix="ssd_bench_pmc_", dir="/tmp")
    out = {"note": ""}
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for key, counters in (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"])):
            d = os.path.join(tmp, key)
            cmd = [prof, "--kernel-trace", "--pmc", *counters, "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), *argv_tail]
            t0 = time.perf_counter()
            p = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = p.wait(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)            # the process group this call started, nothing else
                p.wait()
                return {"note": f"the {key} pass exceeded {timeout_s:.0f} s and was stopped"}
            if rc != 0:
                return {"note": f"the {key} pass exited with code {rc}"}
            files = glob.glob(os.path.join(d, "*", "*counter_collection.csv"))
            if not files:
                return {"note": f"the {key} pass wrote no counter file"}
            acc = {}
            with open(files[0]) as f:
                for r in csv.DictReader(f):
                    if r["Counter_Name"] != counters[0]:
                        continue
                    k = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
                    k = re.sub(r"\(.*", "", k).replace("void ", "")
                    a = acc.setdefault(k, [0.0, set()])
                    a[0] += float(r["Counter_Value"])
                    a[1].add(r["Dispatch_Id"])
            out[key] = {k: (v[0], len(v[1])) for k, v in acc.items()}
            out["note"] += f"{key} pass {time.perf_counter() - t0:.0f} s; "
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def live_traffic_of(tag: str):
    """(bytes per launch, launches) of the kernel instantiation with the largest fetch sum whose name starts with `tag`, from the live passes."""
    if not _LIVE_PMC or "fetch" not in _LIVE_PMC or "write" not in _LIVE_PMC:
        return None
    keys = [k for k in _LIVE_PMC["fetch"] if k.startswith(tag) and k in _LIVE_PMC["write"]]
    if not keys:
        return None
    k = max(keys, key=lambda q: _LIVE_PMC["fetch"][q][0])
    (fkb, nf), (wkb, nw) = _LIVE_PMC["fetch"][k], _LIVE_PMC["write"][k]
    if nf != nw or nf == 0:
        return None
    # gfx950: FETCH_SIZE counts 64 B per 128-B request of a 16-B-per-lane streaming read -> doubled (MI355X_MICROARCH.md section HBM)
    return round((2 * fkb + wkb) * 1024 / nf, -4), nf, k


def cpu_baseline(max_threads: int = 16, variant: int = 300, bs_big: int = PER_GPU_BATCH, all_cores_budget_s: float = 45.0):
    """SURVEY.md section 8(d) / BASELINE.md section 4: the oracle (CPU restatement of the reference path: the same ATen CPU kernels
    the reference dispatches to) timed on this box's host cores for the same synthetic step at bs=2 and bs=32, fwd / loss / bwd / SGD
    separately, 2 warm-up + 5 timed iterations, median -- TWICE: with `max_threads` threads (one GPU's CPU share of the box) and with
    every host core the process may run on (the spec's "all host cores").  The all-cores leg at bs=32 is cut short after
    `all_cores_budget_s` seconds of timed work (at least one timed iteration; the count is reported) so that the default bench run
    stays within minutes.  `value` is the faster of the two bs=32 medians, `cores` the thread count it was measured with.  Also
    returns the oracle's losses of the bs=32 batch at the seed-0 weights (first iteration, before any update) for `loss_delta_vs_cpu`."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ssd_oracle as O
    have = host_cores()
    first_losses = None
    pri = None if variant == 300 else O.create_priors_ssd512()

    def leg(threads, plan, budget_s=None):
        nonlocal first_losses
        torch.set_num_threads(threads)
        res = {}
        for bs, warm, iters in plan:
            note(f"cpu_baseline: {threads} threads, bs={bs}: {warm} warm-up + {iters} timed")
            params = {k: v.requires_grad_(True) for k, v in O.ssd300_random_params(0, variant=variant).items()}
            opt = torch.optim.SGD(list(params.values()), lr=1e-4, momentum=0.9, weight_decay=5e-4)
            x, classes, boxes = synth_batch(bs, 1234, "cpu")
            if variant == 512:
                x = torch.randn(bs, 3, 512, 512, generator=torch.Generator().manual_seed(1234))
            rows, t_timed = [], 0.0
            for it in range(warm + iters):
                t0 = time.perf_counter()
                opt.zero_grad()
                loc, conf = O.ssd300_forward(x, params, variant=variant)
                t1 = time.perf_counter()
                l1, l2 = O.multibox_loss_torch(loc, conf, boxes, classes, pri_cxcywh=pri)
                t2 = time.perf_counter()
                (l1 + l2).backward()
                t3 = time.perf_counter()
                opt.step()
                t4 = time.perf_counter()
                rows.append((t1 - t0, t2 - t1, t3 - t2, t4 - t3))
                if it == 0 and bs == bs_big and first_losses is None:
                    first_losses = (float(l1.detach()), float(l2.detach()))
                if it >= warm:
                    t_timed += t4 - t0
                    if budget_s is not None and bs == bs_big and t_timed > budget_s:
                        break
            timed = rows[warm:]
            med = np.median(np.asarray(timed), axis=0)
            res[bs] = {"images_per_sec": round(bs / float(med.sum()), 3), "fwd_s": round(float(med[0]), 4), "loss_s": round(float(med[1]), 4),
                       "bwd_s": round(float(med[2]), 4), "sgd_s": round(float(med[3]), 4), "warmup": warm, "timed": len(timed)}
        return res

    share = max(1, min(have, max_threads))       # one GPU's CPU share on the box is 16 cores
    plan = ((2, 2, 5), (bs_big, 2, 5)) if variant == 300 else ((2, 1, 2), (bs_big, 0, 1))      # SSD512: ~3x the work per image, fewer runs
    legs = {share: leg(share, plan)}
    skipped = None
    if have > share and variant == 300:
        # "all host cores" on a box whose cgroup gives this process a 16-core quota means hundreds of threads on 16 cores (measured on this
        # pool: 256 threads, 0.024 images/s at bs=2 -- 41 s per step -- against 6.9 with 16).  So: ask the cgroup first; without an answer
        # probe with ONE bs=2 step; run the bs=32 leg only where the thread count is not an oversubscription.
        quota = cpu_quota_cores()
        if quota is not None and quota < have:
            skipped = {"threads": have, "cgroup_cpu_quota_cores": quota,
                       "note": f"the container's CPU quota is {quota} cores of the {have} the scheduler reports: a {have}-thread run is an "
                               f"oversubscription (measured once on this pool: 0.024 images/s at bs=2), not a bigger machine -- not run; "
                               f"the {share}-thread figures are the host-core baseline of this box"}
            if quota > share:
                legs[quota] = leg(quota, ((2, 2, 5), (bs_big, 1, 5)), budget_s=all_cores_budget_s)
        else:
            probe = leg(have, ((2, 0, 1),))
            if probe[2]["images_per_sec"] >= 0.67 * legs[share][2]["images_per_sec"]:
                legs[have] = leg(have, ((2, 2, 5), (bs_big, 1, 5)), budget_s=all_cores_budget_s)
            else:
                skipped = {"threads": have, "bs2_probe": probe[2],
                           "note": f"{have} threads are slower than {share} on the bs=2 step (oversubscribed CPU share): the bs={bs_big} leg with all "
                                   "host cores was not run"}
    torch.set_num_threads(share)
    best = max(legs, key=lambda t: legs[t][bs_big]["images_per_sec"])
    cpu_model = ""
    try:
        cpu_model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except Exception:
        pass
    out = {"value": legs[best][bs_big]["images_per_sec"], "unit": "images/sec", "cores": best, "host_cores": have, "cpu": cpu_model,
           "kind": "port",
           "sample": f"oracle torch-CPU train step (fwd+loss+bwd+SGD) of SSD{variant} on the bench's own synthetic batch; bs=2 and bs={bs_big}, "
                     f"2 warm-up + 5 timed each, medians, with {share} threads (one GPU's CPU share) and with all {have} host cores "
                     f"(that leg's bs={bs_big} run: 1 warm-up, timed iterations cut after {all_cores_budget_s:.0f} s -- count in `timed`); "
                     f"value = the faster bs={bs_big} median ({best} threads)",
           "by_threads": {str(t): {"bs2": r[2], f"bs{bs_big}": r[bs_big]} for t, r in legs.items()},
           **({"all_host_cores_leg": skipped} if skipped else {}),
           "bs2": legs[best][2], f"bs{bs_big}": legs[best][bs_big]}
    return out, first_losses


def gpu_losses_at_oracle_weights(dev, bs: int, conv_dtype: str = "f32"):
    """The HIP path's (loc_loss, conf_loss) for the bench batch at the oracle's seed-0 weights -- what `cpu_baseline` evaluated
    on the CPU (reference normalisation, norm_mode 0)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ssd_oracle as O
    from objectdetection_ssd_amd import Losses, Model
    net = Model.SSD_300()
    named = dict(net.named_parameters())
    with torch.no_grad():
        for k, v in O.ssd300_random_params(0).items():
            named[k].copy_(v)
    net = net.to(dev).train()
    net.conv_dtype = conv_dtype
    x, classes, boxes = synth_batch(bs, 1234, dev)
    with torch.no_grad():
        l1, l2 = Losses.ssd(net(x), classes, boxes)
    return float(l1.item()), float(l2.item())


class conv_flop_counter:
    """Counts the direct-convolution FLOPs of every convolution the ops layer launches inside the `with` block (2*M*Co*K each):
    the algorithmic work of one pass, read off the geometry of the calls themselves."""

    NAMES = ("conv2d_fwd", "conv2d_fwd_x3", "conv2d_fwd_wino", "conv2d_fwd_wino_pool", "conv2d_dgrad", "conv2d_dgrad_x3", "conv2d_dgrad_wino",
             "conv2d_wgrad", "conv2d_wgrad_wino", "wino_wgrad_gemm", "wino_dgrad_adj_gemm", "conv2d_fwd_wino_from_planes")

    def __enter__(self):
        from objectdetection_ssd_amd import ops
        self.ops, self.saved, self.flops = ops, {}, 0.0
        for n in self.NAMES:
            f = getattr(ops, n)
            self.saved[n] = f

            def wrapped(*a, _f=f, **k):
                g = next((v for v in list(a) + list(k.values()) if isinstance(v, ops.ConvGeom)), None)
                if g is not None:
                    self.flops += ops.conv_flops(g)
                return _f(*a, **k)
            setattr(ops, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(self.ops, n, f)
        return False


def timed_cpu(fn, min_seconds: float = 3.0, max_iters: int = 5):
    """median wall time of fn() on the host: one warm-up, then up to max_iters runs or min_seconds, whichever comes first"""
    fn()
    ts = []
    t_all = time.perf_counter()
    while len(ts) < max_iters and (not ts or time.perf_counter() - t_all < min_seconds):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), len(ts)


def aux_workload(args, world, rank, dev):
    """configs[4]: no exchange step in either half, so N ranks are N independent replicas."""
    from objectdetection_ssd_amd import Losses, Model
    bs = args.batch
    g = torch.Generator().manual_seed(1234 + rank)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    threads = max(1, min(host_cores(), 16))
    roof_kind, per_pass_flops, per_pass_bytes, cpu_fn, cpu_units, cpu_sample, prof_net = None, None, None, None, 0, "", None
    if args.workload == "resnet34":
        torch.manual_seed(0)
        net = Model.SSD_resnet34(20).to(dev).eval()
        if args.conv_dtype == "f32x3":
            raise SystemExit("SSD_resnet34 supports --conv-dtype f32 or bf16")
        net.conv_dtype = args.conv_dtype
        x = torch.randn(bs, 3, 224, 224, generator=g).to(dev)
        step = lambda: net(x)                                              # noqa: E731
        metric = "images/sec SSD_resnet34 eval forward (224x224, 63 priors)"
        dtype = args.conv_dtype
        with conv_flop_counter() as fc:
            with torch.no_grad():
                net(x)
        roof_kind, per_pass_flops = "mfma", fc.flops

        def cpu_fn():
            import ssd_oracle as O
            st = O.ssd_resnet34_random_state(0)
            with torch.no_grad():
                O.ssd_resnet34_forward(torch.randn(4, 3, 224, 224), st)
        cpu_units, cpu_sample = 4, "oracle ssd_resnet34_forward (torch-CPU, eval mode) on 4 images of 224x224, state built inside the timed call"
    elif args.workload in ("infer", "infer-graph"):
        # SSD300 inference forward (no decode) at --batch images: eager launches vs one HIP-graph replay
        torch.manual_seed(0)
        net = Model.SSD_300().to(dev).eval()
        net.conv_dtype = args.conv_dtype
        x = torch.randn(bs, 3, 300, 300, generator=g).to(dev)
        if args.workload == "infer-graph":
            gf = net.graphed_forward(x)
            step = lambda: gf(x)                                            # noqa: E731
        else:
            def step():
                with torch.no_grad():
                    return net(x)
        metric = f"images/sec SSD300-VGG16 inference forward ({'HIP graph replay' if args.workload == 'infer-graph' else 'eager launches'})"
        dtype = args.conv_dtype
        extra = {}
        roof_kind, per_pass_flops, prof_net = "mfma", 62.747e9 * bs, net        # forward conv FLOPs per image

        def cpu_fn():
            import ssd_oracle as O
            with torch.no_grad():
                O.ssd300_forward(torch.randn(2, 3, 300, 300), cpu_fn.params)
        if not args.no_cpu_baseline:
            import ssd_oracle as _O
            cpu_fn.params = _O.ssd300_random_params(0)
        cpu_units, cpu_sample = 2, "oracle ssd300_forward (torch-CPU) on 2 images of 300x300"
    elif args.workload == "preprocess":
        # (f)-3: VOC-sized 8-bit images (375x500 / 500x375 / 333x500) already in HBM -> normalised (bs,3,300,300)
        from objectdetection_ssd_amd import Dataset, _lib, ops
        rng = np.random.default_rng(1234 + rank)
        shapes = [((375, 500), (500, 375), (333, 500), (500, 333))[i % 4] for i in range(bs)]
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
        descs = (_lib.ImageDesc * bs)()
        parts, off = [], 0
        for i, a in enumerate(imgs):
            d = descs[i]
            d.src_offset, d.src_h, d.src_w = off, a.shape[0], a.shape[1]
            d.canvas_h, d.canvas_w, d.place_top, d.place_left = a.shape[0], a.shape[1], 0, 0
            d.crop_top, d.crop_left, d.crop_h, d.crop_w = 0, 0, a.shape[0], a.shape[1]
            parts.append(a.reshape(-1)); off += a.size
        arena = torch.from_numpy(np.concatenate(parts)).to(dev)
        step = lambda: ops.preprocess_u8(arena, descs)                      # noqa: E731
        metric = "images/sec device input pipeline (PIL-exact resize to 300x300 + normalize, VOC-sized sources)"
        dtype = "u8 -> f32"
        extra = {"algorithmic_bytes_per_image": int(off / bs + 3 * 300 * 300 * 4)}
        roof_kind, per_pass_bytes = "hbm", float(off + bs * 3 * 300 * 300 * 4)

        def cpu_fn():
            import ssd_oracle as O
            for a in imgs[:8]:
                O.preprocess_image(a)
        cpu_units, cpu_sample = 8, "oracle preprocess_image (numpy restatement of Pillow's resize + normalise) on 8 of the VOC-sized images"
    elif args.workload == "map":
        # (f)-4: 4952 images (VOC07 test size) x 200 detections, ~2.4 GT per image, resident in HBM
        from objectdetection_ssd_amd import ops
        rng = np.random.default_rng(1234 + rank)
        n_img, per = 4952, 200
        D = n_img * per
        gcnt = 1 + np.minimum(rng.poisson(1.4, n_img), 7)
        G = int(gcnt.sum())
        gx = rng.uniform(0, .6, (G, 2)); gwh = rng.uniform(.08, .4, (G, 2))
        gb = np.concatenate([gx, gx + gwh], 1).astype(np.float32)
        gimg = np.repeat(np.arange(n_img), gcnt)
        gstart = np.concatenate([[0], np.cumsum(gcnt)])
        pick = (gstart[:-1, None] + rng.integers(0, 1 << 30, (n_img, per)) % gcnt[:, None]).reshape(-1)
        db = (gb[pick] + rng.normal(0, .05, (D, 4))).astype(np.float32)
        gc = rng.integers(0, 20, G)
        dc = np.where(rng.uniform(size=D) < .7, gc[pick], rng.integers(0, 20, D))
        t32 = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)     # noqa: E731
        a_ = (t32(db, torch.float32), t32(dc, torch.int32), t32(rng.uniform(0, 1, D), torch.float32),
              t32(np.arange(n_img + 1) * per, torch.int32), t32(gb, torch.float32), t32(gc, torch.int32), t32(gstart, torch.int32))
        levels = torch.arange(0, 1.1, 0.1).double().numpy()
        step = lambda: ops.map_eval(*a_, levels, 20)                        # noqa: E731
        metric = "evaluated images/sec, 20-class 11-point mAP (4952 images x 200 detections per pass)"
        dtype = "f32 IoU / f64 precision-recall"
        bs = n_img
        extra = {"detections": D, "ground_truth": G}
        roof_kind, per_pass_bytes = "hbm", float(D * 24 + G * 20 + (n_img + 1) * 8)      # boxes + class + score per detection, box + class per GT, offsets
        n_cpu = 300

        def cpu_fn():
            import ssd_oracle as O
            dstart = np.arange(n_cpu + 1) * per
            O.get_map([db[dstart[i]:dstart[i + 1]] for i in range(n_cpu)], [dc[dstart[i]:dstart[i + 1]] for i in range(n_cpu)],
                      [np.linspace(1, 0, per, dtype=np.float32)] * n_cpu, [gb[gstart[i]:gstart[i + 1]] for i in range(n_cpu)],
                      [gc[gstart[i]:gstart[i + 1]] for i in range(n_cpu)])
        cpu_units, cpu_sample = n_cpu, f"oracle get_map (numpy restatement of Util.get_map) on the first {n_cpu} images x {per} detections"
    else:
        l = (torch.randn(bs, 8732, 4, generator=g)).to(dev)
        c = (3 * torch.randn(bs, 8732, 21, generator=g)).to(dev)
        wh = torch.tensor([[500, 375]] * bs, dtype=torch.float32).to(dev)
        step = lambda: Losses.inference_batch_padded(l, c, wh)             # noqa: E731  (padded tensors + counts: no host sync inside the pass)
        metric = "images/sec batched decode + per-class NMS + top-200 (8732 priors, conf ~ 3*randn)"
        dtype = "f32"
        roof_kind, per_pass_bytes = "hbm", float(bs * 8732 * 25 * 4)                   # 0.87 MB read per image

        def cpu_fn():
            import ssd_oracle as O
            ln, cn = l[:2].cpu().numpy(), c[:2].cpu().numpy()
            for i in range(2):
                O.decode_nms(ln[i], cn[i], 500.0, 375.0)
        cpu_units, cpu_sample = 2, "oracle decode_nms (numpy restatement of Losses.inference) on 2 of the images"
    if args.workload in ("resnet34", "decode"):
        extra = {}

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        line = {"metric": metric, "value": round(bs * world * args.steps / elapsed, 2), "unit": "images/sec", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
                "config": dict({"workload": f"{args.workload} (see --help), {bs} images per pass per GPU", "global_batch": bs * world,
                                "parallelism": f"replicas x{world}"}, **extra)}
        if roof_kind == "hbm":
            ach = per_pass_bytes / (ms * 1e-3) / 1e9
            line["roofline"] = {"bound": "hbm", "kernel": "whole pass (every kernel of the workload between the two fences)",
                                "achieved": round(ach, 2), "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 5), "traffic": None,
                                "algorithmic_bytes_per_pass": int(per_pass_bytes),
                                "note": "launch- / latency-bound at this size: the pass is a handful of short dependent kernels, not a stream"}
        elif roof_kind == "mfma":
            peak = 2500.0 if args.conv_dtype == "bf16" else PEAK_F32_MFMA_TFLOPS
            ach = per_pass_flops / (ms * 1e-3) / 1e12
            line["roofline"] = {"bound": "mfma", "kernel": "whole pass (direct-convolution FLOPs of every convolution / ms_per_step)",
                                "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": None,
                                "algorithmic_gflop_per_pass": round(per_pass_flops / 1e9, 2),
                                "note": "a speed-up-over-direct figure where Winograd layers execute fewer FLOPs than counted"}
            if prof_net is not None and args.workload == "infer" and not args.no_roofline:
                line["roofline"]["dominant_kernel"] = roofline_of(prof_net, step, args.conv_dtype, ms)
        if cpu_fn is not None and world == 1 and not args.no_cpu_baseline:
            torch.set_num_threads(threads)
            sec, iters = timed_cpu(cpu_fn)
            line["cpu_baseline"] = {"value": round(cpu_units / sec, 3), "unit": "images/sec", "cores": threads, "host_cores": host_cores(), "kind": "port",
                                    "sample": cpu_sample + f"; median of {iters} timed runs after one warm-up, {threads} torch threads"}
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


def roofline_of(net, step, conv_dtype: str, ms: float, layers: bool = False) -> dict:
    """The `roofline` object of one configuration: three more steps in the engine's profiling mode (every conv kernel between two HIP
    events on the stream it is launched on; the batched Winograd GEMMs additionally by the library's own per-launch events), the kernel
    with the largest summed time against the dense MFMA peak of the dtype it multiplies in."""
    eng = net._engine
    agg = {}
    rows = []
    from objectdetection_ssd_amd import _lib as _l
    import ctypes as _C
    gemm_tag = "igemm_kernel<64, 64, 2, 2, 1, true"
    fused_tag = "wino4_gemm_out_kernel"
    x3_tags = {4: "gemm_planes_x3_kernel", 5: "gemm_tn_x3_kernel"}       # Winograd plane GEMMs from three bf16 limbs per f32 operand (csrc/gemm_x3.hip)
    exec_flops = 0.0
    for _ in range(3):
        eng.prof = []
        _l.check(_l.load().ssd_prof_gemm_begin(), "prof")        # the batched Winograd GEMM launches, each by itself
        step()
        torch.cuda.synchronize()
        ms_buf, fl_buf, kind_buf = (_C.c_float * 1024)(), (_C.c_double * 1024)(), (_C.c_int * 1024)()
        ng = _l.load().ssd_prof_gemm_collect_kinds(ms_buf, fl_buf, kind_buf, 1024)
        for i in range(max(ng, 0)):
            a = agg.setdefault(x3_tags.get(kind_buf[i], fused_tag if kind_buf[i] == 1 else gemm_tag), [0.0, 0.0, 0])
            a[0] += ms_buf[i] * 1e-3; a[1] += fl_buf[i]; a[2] += 1
        for label, tag, flops, e0, e1, executed in eng.prof:
            exec_flops += executed
            dt = e0.elapsed_time(e1) * 1e-3
            a = agg.setdefault(tag, [0.0, 0.0, 0])
            a[0] += dt; a[1] += flops; a[2] += 1
            rows.append((label, tag, flops, dt))
        eng.prof = None
    # dominant KERNEL: the Winograd ops are composites (two transform kernels around sixteen batched GEMMs), listed in by_kernel
    # but not eligible -- a roofline row has to be one kernel that the rocprof summary can be held against
    tag, (tsum, fsum, n) = max(((k, v) for k, v in agg.items() if not k.startswith("winograd")), key=lambda kv: kv[1][0])
    ach = fsum / tsum / 1e12
    # HBM bytes per launch of the dominant kernel: from the counter passes this invocation ran as child processes before its timed run
    # (live_traffic_passes), else from the committed PMC passes of the round's profile run (a pointer, and the line says which)
    traffic = None
    traffic_file = "r04_bf16_traffic.json" if conv_dtype == "bf16" else "r04_traffic.json"
    traffic_src = f"profiles/{traffic_file}: the PMC passes of this round's profile run, not this invocation"
    live = live_traffic_of(tag) if conv_dtype == (_LIVE_PMC or {}).get("conv_dtype") else None
    if live is not None:
        traffic = live[0]
        traffic_src = (f"LIVE: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE, two child runs of this bench.py invocation before its timed run "
                       f"({live[1]} launches of {live[2]}; (2 x FETCH_SIZE + WRITE_SIZE) x 1024 / launches; {_LIVE_PMC['note'].strip()})")
    else:
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", traffic_file)))
            if tj["kernel"] == tag:
                traffic = tj["bytes_per_launch"]
            if _LIVE_PMC is not None and _LIVE_PMC.get("note"):
                traffic_src += f" (live passes: {_LIVE_PMC['note'].strip()})"
        except Exception:
            pass
    # dense peak of the dtype the kernel multiplies in; an f32x3 product costs six bf16 MFMAs, so its ceiling in
    # algorithmic f32 FLOPs is a sixth of the bf16 peak
    on_bf16_mfma = "bf16" in tag or (conv_dtype == "bf16" and tag.startswith("conv3x3_halo"))
    if tag in x3_tags.values():
        peak, peak_note = 2500.0, ("bf16 MFMA dense (v_mfma_f32_32x32x16_bf16): this kernel multiplies f32 operands as three exact bf16 limbs each, six "
                                   "limb products per f32 product; `achieved` is its EXECUTED bf16 MFMA rate over whole tiles (the f32-equivalent rate "
                                   "of the Winograd-domain product is a sixth of it, against 157.3 TFLOP/s of the f32 MFMA it replaces; the ops it serves "
                                   "are the `winograd_3x3` row of by_kernel, in direct-convolution FLOPs)")
    elif conv_dtype == "f32" or (conv_dtype == "bf16" and not on_bf16_mfma):
        peak, peak_note = PEAK_F32_MFMA_TFLOPS, "f32 MFMA dense"
    elif conv_dtype == "bf16":
        peak, peak_note = 2500.0, "bf16 MFMA dense (v_mfma_f32_32x32x16_bf16); `achieved` counts the direct convolution's FLOPs of the launches, not the tile padding"
    else:
        peak, peak_note = round(2500.0 / 6, 1), "bf16 MFMA dense / 6 limb products per f32 product"
    if tag == fused_tag:
        peak_note += ("; the fused Winograd kernel (36 plane GEMMs + output transform, all planes' accumulators in registers): `achieved` is "
                      "its EXECUTED rate over the whole kernel, epilogue included")
    if tag == gemm_tag:
        peak_note += ("; this is the batched GEMM inside the Winograd ops, timed by itself: `achieved` is its EXECUTED rate (4/9 resp. 1/4 of "
                      "the direct convolution's FLOPs plus tile padding); the ops it serves are the `winograd_3x3` row of by_kernel, in "
                      "direct-convolution FLOPs")
    if tag.startswith("winograd"):
        peak_note += ("; the ops of this tag are Winograd F(2x2,3x3) convolutions (input transform + 16 batched igemm_kernel<64,64> "
                      "GEMMs + output transform): `achieved` counts the direct convolution's FLOPs, the GEMMs execute 2.25x fewer")
    roof = {"bound": "mfma", "kernel": tag + ", ...>", "achieved": round(ach, 2),
                       "peak": peak, "peak_note": peak_note, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                       "traffic": traffic, "traffic_unit": f"bytes per launch ({traffic_src})", "launches_timed": n, "avg_launch_ms": round(tsum / n * 1e3, 4),
                       "avg_launch_gflop": round(fsum / n / 1e9, 3),
                       "step_executed_gflop": round(exec_flops / 3 / 1e9, 1),
                       "step_executed_frac": round(exec_flops / 3 / (ms * 1e-3) / 1e12 / (2500.0 if conv_dtype == "bf16" else PEAK_F32_MFMA_TFLOPS), 4),
                       "step_executed_note": "MFMA FLOPs the step's convolution kernels execute (Winograd layers: 36 multiplies per 4x4 tile) / "
                                             "ms_per_step / " + ("bf16" if conv_dtype == "bf16" else "f32") + " MFMA peak -- the whole-step roofline fraction",
                       "all_conv_kernels_tflops": round(sum(a[1] for a in agg.values()) / sum(a[0] for a in agg.values()) / 1e12, 2),
                       "by_kernel": {k: {"ms_per_step": round(a[0] / 3 * 1e3, 3), "tflops": round(a[1] / a[0] / 1e12, 2),
                                         "launches_per_step": a[2] // 3} for k, a in sorted(agg.items())}}
    if tag in x3_tags.values():      # the same launches counted as f32 products (one per six limb MFMAs): algorithmic Winograd-domain FLOPs / time
        roof["f32_product_tflops"] = round(ach / 6.0, 2)
        roof["f32_product_note"] = ("achieved / 6: the Winograd-domain f32 products these launches deliver per second; against it the f32 MFMA "
                                    "peak is 157.3 TFLOP/s and the bf16 peak / 6 = 416.7 -- `frac` is the same fraction either way")
    if layers:                       # per-layer table: mean over the three profiled steps
        per = {}
        for label, tag, flops, dt in rows:
            e = per.setdefault(label, [tag, flops, 0.0, 0])
            e[2] += dt; e[3] += 1
        for label, (tag, flops, tsum_l, cnt) in per.items():
            dt = tsum_l / cnt
            print(f"{label:32s} {tag:28s} {flops / 1e9:9.2f} GF {dt * 1e3:8.3f} ms {flops / dt / 1e12:7.2f} TF/s", file=sys.stderr)
    return roof


def dump_train_outputs(out_dir: str, last: dict, l1, l2, n_pos, trainer) -> dict:
    """--dump-outputs: what the last timed train step handed its caller, one DIR/<name>.npy per array:
      loss_loc, loss_conf, n_pos     float64 (1,): the un-normalised loss sums and the positive-prior count of the step (norm_mode 1)
      params_sample, grads_sample    float32: the parameters after the step's SGD update and the gradient that made it, at the same
                                     DUMP_SAMPLE flat-buffer positions (seeded choice; the full buffers are 105 MB each)
      loc, conf                      float32 (k, priors, 4 / 21): the step's forward outputs for its first k images, k = the whole
                                     batch unless that exceeds DUMP_MAX_BYTES (eager step only: the graph replay keeps them internal)
    Returns the manifest that goes on the JSON line."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {name: np.array([float(t.item())], np.float64) for name, t in (("loss_loc", l1), ("loss_conf", l2), ("n_pos", n_pos))}
    n = trainer.n
    pick = np.sort(np.random.default_rng(0).choice(n, size=min(n, DUMP_SAMPLE), replace=False))
    idx = torch.from_numpy(pick).to(trainer.flat_param.device)
    arrays["params_sample"] = trainer.flat_param[idx].float().cpu().numpy()
    arrays["grads_sample"] = trainer.flat_grad[:n][idx].float().cpu().numpy()
    if "loc" in last:
        room = DUMP_MAX_BYTES - sum(a.nbytes for a in arrays.values()) - (1 << 16)      # (1 << 16): the .npy headers
        per_image = (last["loc"][0].numel() + last["conf"][0].numel()) * 4
        k = min(last["loc"].shape[0], room // per_image)
        arrays["loc"] = last["loc"][:k].float().cpu().numpy()
        arrays["conf"] = last["conf"][:k].float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total < DUMP_MAX_BYTES, total
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "bytes": total, "arrays": {name: list(a.shape) for name, a in arrays.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=PER_GPU_BATCH, help="images per GPU")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, measure everything else (roofline, live traffic, cpu_baseline and loss_delta_vs_cpu, the "
                         "f32-MFMA-only / bf16 / graph-step legs, host enqueue time); a plain run prints the headline line alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without cpu_baseline / loss_delta_vs_cpu")
    ap.add_argument("--live-traffic", default="auto", choices=("auto", "on", "off"),
                    help="--full: roofline.traffic from two rocprofv3 --pmc passes run by this invocation as child processes BEFORE its timed run "
                         "(auto: at N = 1 for the SSD300 train workload when a GPU and rocprofv3 are present; adds about half a minute); off: the committed "
                         "file of the round")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the roofline pass")
    ap.add_argument("--no-bf16-leg", action="store_true", help="--full without the short f32-MFMA-only, bf16-operand and graph-step runs")
    ap.add_argument("--layers", action="store_true", help="--full: print the per-launch table of the roofline pass to stderr")
    ap.add_argument("--conv-dtype", default="f32", choices=("f32", "f32x3", "bf16"),
                    help="bf16 = BASELINE configs[2] (bf16-operand fwd/dgrad convs, f32 accumulate); not the headline bench line")
    ap.add_argument("--variant", type=int, default=300, choices=(300, 512), help="512 = build-defined SSD512 (not a bench line)")
    ap.add_argument("--workload", default="train", choices=("train", "resnet34", "decode", "preprocess", "map", "infer", "infer-graph"),
                    help="train = the headline line (BASELINE configs[1]); resnet34 / decode = the two halves of configs[4] "
                         "(SSD_resnet34 eval forward at 224x224; batched per-class NMS decode of SSD300-shaped outputs): replicas only")
    ap.add_argument("--wino-min-ci", type=int, default=-1, help="tuning aid: Winograd for 3x3/s1 layers with at least this many input channels (0 = off)")
    ap.add_argument("--wino-tile", type=int, default=-1, choices=(-1, 2, 4), help="tuning aid: Winograd output tile of forward / dgrad")
    ap.add_argument("--wino-wgrad-min-ci", type=int, default=-1, help="tuning aid: Winograd weight gradient from this many input channels")
    ap.add_argument("--wino-wgrad-max-hw", type=int, default=-1, help="tuning aid: Winograd weight gradient on maps up to this size (0 = off)")
    ap.add_argument("--wino-min-hw", type=int, default=-1, help="tuning aid: Winograd only on maps of at least this size")
    ap.add_argument("--xform-blocks", type=int, default=-1, help="tuning aid: grid cap of the Winograd transform kernels")
    ap.add_argument("--no-overlap-tail", action="store_true", help="tuning aid: everything on one stream")
    ap.add_argument("--overlap-wgrad", action="store_true", help="tuning aid: Winograd weight-gradient GEMMs on their own stream")
    ap.add_argument("--no-batch-weights", action="store_true", help="tuning aid: filter transforms / re-layouts layer by layer")
    ap.add_argument("--no-wino-dilated", action="store_true", help="tuning aid: fc6 (dilation 4) on the direct kernels")
    ap.add_argument("--no-fuse-pool", action="store_true", help="tuning aid: conv -> ReLU -> 2x2 pool as separate kernels")
    ap.add_argument("--wino-wgrad-nt", action="store_true", help="tuning aid: Winograd weight gradient on transposed planes (NT GEMM)")
    ap.add_argument("--no-keep-planes", action="store_true", help="tuning aid: the Winograd weight gradient transforms x again")
    ap.add_argument("--no-dual-dy", action="store_true", help="tuning aid: weight and data gradient transform dy separately")
    ap.add_argument("--no-first-wino", action="store_true", help="tuning aid: conv1_1 writes its activation tensor, conv1_2 transforms it (two kernels)")
    ap.add_argument("--no-adjoint-dgrad", action="store_true", help="tuning aid: rotated-filter Winograd data gradients everywhere (second dy plane set)")
    ap.add_argument("--no-adjoint-chain", action="store_true", help="tuning aid: adjoint data gradients written out as tensors between chained layers")
    ap.add_argument("--overlap-allreduce", action="store_true",
                    help="force the sliced all-reduce that runs while the backward is still running (ddp.py overlap=True; the default whenever N > 1)")
    ap.add_argument("--no-overlap-allreduce", action="store_true", help="one all-reduce of the whole gradient buffer after the backward")
    ap.add_argument("--grad-dtype", default="auto", choices=("auto", "f32", "bf16"),
                    help="payload of the weight-gradient all-reduce: bf16 = 52.6 MB instead of 105 MB (auto: bf16 with --conv-dtype bf16, else f32)")
    ap.add_argument("--igemm-lds-pad", type=int, default=-1, help="tuning aid: extra dynamic LDS bytes per igemm block (-1 = library default)")
    ap.add_argument("--spinup-seconds", type=float, default=3.0,
                    help="run untimed steps for this long BEFORE the --warmup steps: a device that has been idle starts the process at a low "
                         "shader clock and takes seconds to reach the clock it then holds (measured on this pool: the same step 23.96 ms in the "
                         "first half second of load, 20.08 ms two seconds later); the timed region is still exactly --steps steps after "
                         "--warmup steps.  0 = none.  Reported in config.spinup")
    ap.add_argument("--graph-step", default="off", choices=("on", "off"),
                    help="time the train step as ONE captured HIP graph replay per step (ddp.GraphedTrainStep) instead of ~250 eager launches. "
                         "Default off: at batch 32 the step is GPU-bound and the replay measures slower on the device than the eager two-stream "
                         "schedule; a --full run reports the replay's numbers beside the headline (config.graph_step)")
    ap.add_argument("--graph-one-stream", action="store_true", help="capture the whole step on one stream (default: the tiny-map group on its second stream inside the graph, as in the eager step)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only to rehearse N>1 on one GPU)")
    ap.add_argument("--one-device", action="store_true", help="rehearsal: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="plumbing check: start the ranks, init the process group, all-reduce one number, print the world size and stop "
                         "before anything touches a GPU")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (losses, forward outputs, samples of the updated parameters "
                         "and of their gradient) to DIR/<name>.npy; train workload only")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.workload != "train":
        raise SystemExit("--dump-outputs: only the train workload writes its outputs")
    if not args.full:
        if args.layers or args.live_traffic == "on":
            raise SystemExit("--layers and --live-traffic on report on the roofline pass, which only a --full run makes")
        # a plain run: the headline and nothing else (the switches below are how a --full run leaves a part out)
        args.no_cpu_baseline = args.no_roofline = args.no_bf16_leg = True
        args.live_traffic = "off"

    # `python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks ourselves, one process per GPU, BEFORE
    # anything in this process touches the GPU (a process that has initialised HIP must not be replaced or forked into ranks).
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd).returncode)

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world_env != args.gpus:
        # a launcher that started a different number of ranks than --gpus says would silently mislabel the line
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world_env} ranks")
    if args.rendezvous_only:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        dist.init_process_group("gloo" if args.backend == "nccl" and not torch.cuda.is_available() else args.backend,
                                rank=rank, world_size=world_env)
        t = torch.ones(1)
        dist.all_reduce(t)
        world = dist.get_world_size()
        assert world == args.gpus == int(t.item()), (world, args.gpus, float(t))
        if rank == 0:
            print(json.dumps({"rendezvous": True, "n_gpus": world, "backend": dist.get_backend(), "ranks_counted": int(t.item())}))
        dist.destroy_process_group()
        return
    global _LIVE_PMC
    if (args.live_traffic != "off" and world_env == 1 and args.workload == "train" and args.variant == 300 and torch.cuda.device_count() > 0):
        # (device_count() does not initialise the GPU on this image; is_available() below does -- the children run before it)
        note("live traffic: two rocprofv3 --pmc child runs (FETCH_SIZE, WRITE_SIZE)")
        # the same engine flags as this run (later options win): one step, every kernel on one stream, none of the extra legs
        tail = sys.argv[1:] + ["--steps", "1", "--warmup", "1", "--spinup-seconds", "0", "--no-cpu-baseline", "--no-bf16-leg", "--no-overlap-tail",
                               "--live-traffic", "off", "--graph-step", "off", "--dump-outputs", ""]
        _LIVE_PMC = live_traffic_passes(tail)
        _LIVE_PMC["conv_dtype"] = args.conv_dtype
        note("live traffic: " + (_LIVE_PMC.get("note") or "done"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the gfx950 HIP extension is the only compute path")
    if args.one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    world = 1
    if world_env > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
        world = dist.get_world_size()            # n_gpus of the JSON line is the world size RCCL actually formed
        if world != args.gpus:
            raise SystemExit(f"bench.py: process group has {world} ranks, --gpus says {args.gpus}")

    from objectdetection_ssd_amd import Losses, Model
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel

    if args.workload != "train":
        return aux_workload(args, world, rank, dev)

    if args.wino_wgrad_nt:
        from objectdetection_ssd_amd import _lib
        _lib.check(_lib.load().ssd_tune_set_wino_wgrad_tn(0), "tune")
    if args.xform_blocks > 0:
        from objectdetection_ssd_amd import _lib
        _lib.check(_lib.load().ssd_tune_set_wino_xform_blocks(args.xform_blocks), "tune")
    if args.igemm_lds_pad >= 0:
        from objectdetection_ssd_amd import _lib
        _lib.check(_lib.load().ssd_tune_set_igemm_lds_pad(args.igemm_lds_pad), "tune")
    torch.manual_seed(0)                                   # same initial weights on every rank
    net = (Model.SSD_300() if args.variant == 300 else Model.SSD_512()).to(dev).train()
    net.conv_dtype = args.conv_dtype
    if args.wino_min_ci >= 0:
        net._engine.wino = args.wino_min_ci > 0
        net._engine.WINO_MIN_CI = args.wino_min_ci
    if args.wino_tile > 0:
        net._engine.WINO_TILE = args.wino_tile
    if args.wino_wgrad_min_ci >= 0:
        net._engine.WINO_WGRAD_MIN_CI = args.wino_wgrad_min_ci
    if args.wino_wgrad_max_hw >= 0:
        net._engine.WINO_WGRAD_MAX_HW = args.wino_wgrad_max_hw
    if args.wino_min_hw >= 0:
        net._engine.WINO_MIN_HW = args.wino_min_hw
    net._engine.overlap_tail = not args.no_overlap_tail
    net._engine.overlap_wgrad = args.overlap_wgrad
    if args.no_batch_weights:
        net._engine.batch_weights = False
    if args.no_wino_dilated:
        net._engine.wino_dilated = False
    if args.no_fuse_pool:
        net._engine.fuse_pool = False
    if args.no_keep_planes:
        net._engine.keep_planes = False
    if args.no_dual_dy:
        net._engine.dual_dy = False
    if args.no_first_wino:
        net._engine.first_wino = False
    if args.no_adjoint_dgrad:
        net._engine.adjoint_dgrad = False
    if args.no_adjoint_chain:
        net._engine.adjoint_chain = False
    train_gflop = TRAIN_GFLOP_PER_IMAGE
    if args.variant == 512:
        # direct-convolution FLOPs of one SSD512 train step per image, from the geometry of the step's own convolution calls
        with conv_flop_counter() as fc:
            xp = torch.randn(1, 3, 512, 512, device=dev)
            lo_, co_ = net(xp)
            (lo_.sum() + co_.sum()).backward()
        net.zero_grad(set_to_none=True)
        conv1_1 = 2.0 * 512 * 512 * 64 * 27
        train_gflop = (fc.flops + 2 * conv1_1) / 1e9              # conv1_1 runs its own kernels (forward + weight gradient, no data gradient)
    grad_bf16 = args.grad_dtype == "bf16" or (args.grad_dtype == "auto" and args.conv_dtype == "bf16")
    trainer = FlatSGDDataParallel(net, lr=1e-4, momentum=0.9, weight_decay=5e-4,
                                  overlap=(True if args.overlap_allreduce else False if args.no_overlap_allreduce else None),
                                  grad_dtype=torch.bfloat16 if (grad_bf16 and world > 1) else torch.float32, time_exchange=world > 1)
    trainer.broadcast_parameters(0)
    bs = args.batch
    x, classes, boxes = synth_batch(bs, 1234 + rank, dev)
    if args.variant == 512:
        x = torch.randn(bs, 3, 512, 512, generator=torch.Generator().manual_seed(1234 + rank)).to(dev)

    last = {}                                              # --dump-outputs: the forward outputs of the latest eager step

    def eager_step():
        trainer.zero_grad()
        loc, conf = net(x)
        if args.dump_outputs:
            last["loc"], last["conf"] = loc.detach(), conf.detach()
        l1, l2, n_pos = Losses.ssd((loc, conf), classes, boxes, norm_mode=1, with_n_pos=True)     # un-normalised sums (ddp.py)
        (l1 + l2).backward()
        trainer.reduce_and_step(n_pos)
        return l1, l2, n_pos

    use_graph = args.graph_step == "on"
    gstep = None
    if use_graph:
        from objectdetection_ssd_amd.ddp import GraphedTrainStep
        gstep = GraphedTrainStep(net, trainer, max_boxes_per_image=8, warmup=2, two_streams=not args.graph_one_stream)

        def step():
            return gstep(x, classes, boxes)
        note("graph step: two eager steps + capture")
        for _ in range(3):                                 # two eager steps (pools, workspaces, momentum) + the capturing one: set-up, not warm-up
            step()
        torch.cuda.synchronize()
        note(f"graph captured: {gstep.kernel_nodes} kernel nodes")
    else:
        step = eager_step

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    from objectdetection_ssd_amd import ops as _ops
    spin_steps, spin_t0 = 0, time.perf_counter()
    if args.spinup_seconds > 0:
        note(f"spin-up: untimed steps for {args.spinup_seconds:.1f} s (device clock ramp)")
        # how many steps fit in the spin-up depends on the device's speed: its SGD updates are undone below, so that the warm-up and
        # timed steps start from the same weights and momentum on every run
        state0 = (trainer.flat_param.clone(), trainer.flat_mom.clone(), trainer._has_momentum, trainer.steps)
        while True:
            for _ in range(5):
                step()
            spin_steps += 5
            torch.cuda.synchronize()
            go = time.perf_counter() - spin_t0 < args.spinup_seconds
            if world > 1:                                  # one decision for all ranks, so that every rank issues the same collectives
                t = torch.tensor([1 if go else 0], device=dev, dtype=torch.int32)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                go = bool(t.item())
            if not go:
                break
        with torch.no_grad():
            trainer.flat_param.copy_(state0[0])
            trainer.flat_mom.copy_(state0[1])
        trainer._has_momentum, trainer.steps = state0[2], state0[3]
        net.invalidate_weight_cache()
        del state0
        torch.cuda.synchronize()
    note(f"{args.warmup} warm-up + {args.steps} timed steps")
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    probe_a = _ops.clock_probe(dev)              # two tiny launches bracket the timed steps: average shader clock held
    for _ in range(args.steps):
        l1, l2, n_pos_local = step()
    probe_b = _ops.clock_probe(dev)
    fence()
    elapsed = time.perf_counter() - t0
    exposed_ms = trainer.exposed_exchange_ms(last=args.steps) if world > 1 else None
    mhz = _ops.shader_mhz(probe_a, probe_b)
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms = elapsed / args.steps * 1e3
    ips = bs * world * args.steps / elapsed
    note(f"timed: {ms:.3f} ms/step")
    dumped = None
    if args.dump_outputs and rank == 0:                    # before anything below runs another step over the same buffers
        dumped = dump_train_outputs(args.dump_outputs, last if gstep is None else {}, l1, l2, n_pos_local, trainer)
        note(f"outputs of the last timed step: {dumped['bytes'] / 2**20:.1f} MB in {args.dump_outputs}")
    # --full: host-side enqueue time of ONE step into an empty queue (diagnostic: the step is GPU-bound while this stays below
    # ms_per_step; several steps back to back would measure the queue's back-pressure instead)
    host_ms = host_eager_ms = None
    if args.full:
        host_ms = host_eager_ms = 0.0
        for _ in range(3):
            fence()
            h0 = time.perf_counter()
            step()
            host_ms += (time.perf_counter() - h0) / 3 * 1e3
        fence()
        if gstep is not None:
            for _ in range(3):
                fence()
                h0 = time.perf_counter()
                eager_step()
                host_eager_ms += (time.perf_counter() - h0) / 3 * 1e3
            fence()
    n_pos = float(trainer.flat_grad[trainer.n].item())
    loss = (float(l1.item()) + float(l2.item())) / max(float(n_pos_local.item()), 1.0)
    # self-check of the collective path: every rank adds 1 and its own rank id; rank 0 prints what arrived
    ranks_seen, rank_id_sum = 1, 0
    if world > 1:
        t = torch.tensor([1.0, float(rank)], device=dev, dtype=torch.float64)
        dist.all_reduce(t)
        ranks_seen, rank_id_sum = int(t[0].item()), int(t[1].item())
        if ranks_seen != world or rank_id_sum != world * (world - 1) // 2:
            raise SystemExit(f"bench.py: the all-reduce saw {ranks_seen} ranks (id sum {rank_id_sum}), expected {world}")

    out = {"metric": "images/sec SSD300-VGG16 train step" if args.variant == 300 else "images/sec SSD512-VGG16 (build-defined) train step",
           "value": round(ips, 2), "unit": "images/sec",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": {"f32": "f32" + (" (tensors, accumulators, loss, SGD; the Winograd-domain products of the layers with >= 256 reduction channels are "
                                      "formed from three EXACT bf16 limbs per f32 operand on the bf16 MFMA -- six limb products per f32 product, dropped "
                                      "terms <= 2^-26 -- measured no further from f64 than the f32 MFMA; SSD_WINO_X3=0 selects the f32 MFMA)"
                                      if _ops.wino_x3(4, 256) and net._engine.wino else ""),
                     "f32x3": "f32 (fwd/dgrad products from three bf16 limbs per operand, f32 accumulate)",
                     "bf16": "bf16 operands (convs), f32 accumulate / loss"}[args.conv_dtype], "data": "synthetic",
           "config": {"workload": (f"SSD300-VGG16 train step (fwd + MultiBox loss + bwd + all-reduce + SGD), "
                                   f"batch {bs}/GPU, 300x300x3, 21 classes, 8732 priors (BASELINE configs[1])") if args.variant == 300 else
                                  (f"build-defined SSD512-VGG16 train step (NOT in the reference; BASELINE configs[3] per-GPU leg): fwd + MultiBox loss + "
                                   f"bwd + all-reduce + SGD, batch {bs}/GPU, 512x512x3, 21 classes, 24564 priors"),
                      "global_batch": bs * world, "per_gpu_batch": bs, "parallelism": f"dp{world}" + (" (gradient all-reduce overlapped with backward)" if (trainer.overlap and world > 1) else ""),
                      "gradient_exchange": {"overlapped_with_backward": bool(trainer.overlap and world > 1),
                                            "payload_bytes": (0 if world == 1 else
                                                              (trainer.n_w * 2 + (trainer.n - trainer.n_w + 1) * 4) if trainer.flat_grad16 is not None
                                                              else (trainer.n + 1) * 4),
                                            "weight_payload_dtype": "bf16" if trainer.flat_grad16 is not None else "f32",
                                            "exposed_ms_per_step_rank0": None if exposed_ms is None else round(exposed_ms, 4),
                                            "note": "exposed = HIP-event time on the compute stream from reaching the exchange's wait point to "
                                                    "the last collective's completion (what the backward did not hide); null on one GPU"},
                      "ranks_seen": ranks_seen, "backend": (dist.get_backend() if world > 1 else "none (single process)"),
                      "collective_env": {k: v for k, v in os.environ.items() if k.startswith(("NCCL_", "RCCL_", "HSA_ENABLE_IPC", "TORCH_NCCL_"))},
                      "train_gflop_per_image": round(train_gflop, 3),
                      "direct_conv_tflops_per_gpu": round(train_gflop * ips / world / 1e3, 2),
                      "direct_conv_flops_over_f32_mfma_peak": round(train_gflop * ips / world / 1e3 / PEAK_F32_MFMA_TFLOPS, 4),
                      "direct_conv_note": "algorithmic (direct-convolution) FLOPs of the step / time: a speed-up-over-direct figure, NOT a roofline "
                                          "fraction (Winograd executes 1/4 .. 4/9 of them); the executed fraction is roofline.step_executed_frac of a --full line",
                      "last_loss_per_rank": round(loss, 5), "n_pos_global_last": n_pos,
                      "conv_algorithm": ("f32 throughout; Winograd F(%dx%d,3x3) for forward / dgrad of the 3x3 stride-1 layers with >= %d input "
                                         "channels (the 2x2 max pools fused into its output transform) and for the weight gradients of those with >= %d channels on maps <= %d px, direct MFMA "
                                         "kernels for the rest" % (net._engine.WINO_TILE, net._engine.WINO_TILE, net._engine.WINO_MIN_CI,
                                                                   net._engine.WINO_WGRAD_MIN_CI, net._engine.WINO_WGRAD_MAX_HW)
                                         + ("; plane GEMMs with >= 256 reduction channels (and the weight-gradient GEMMs of layers with >= 128 x 128 "
                                            "channels) on the bf16 MFMA from three exact bf16 limbs per operand (csrc/gemm_x3.hip)"
                                            if _ops.wino_x3(4, 256) else ""))
                      if (net._engine.wino and args.conv_dtype == "f32") else "direct MFMA kernels",
                      "spinup": {"seconds": args.spinup_seconds, "untimed_steps": spin_steps,
                                 "note": "untimed steps run before the warm-up steps so that the timed region sees the shader clock the device HOLDS under "
                                         "this load, not the ramp from idle (bench.py --spinup-seconds; 0 disables)"},
                      "host_enqueue_ms_per_step": None if host_ms is None else round(host_ms, 2),
                      "step_launch": ({"form": "one HIP graph replay per step (ddp.GraphedTrainStep: forward + loss + backward"
                                               + (" + SGD" if world == 1 else "; all-reduce + SGD issued behind it") + ")",
                                       "kernel_launches_in_graph": gstep.kernel_nodes,
                                       "host_enqueue_ms_per_step_eager": None if host_eager_ms is None else round(host_eager_ms, 2),
                                       "note": "bitwise equal to the eager step (tests/test_gpu_path.py::test_graphed_train_step_is_bitwise_the_eager_step)"}
                                      if gstep is not None else {"form": "eager: every kernel launched from Python"}),
                      "shader_clock_mhz_during_timed_steps": round(mhz, 0),
                      "f32_mfma_peak_at_that_clock_tflops": round(PEAK_F32_MFMA_TFLOPS * mhz / 2400.0, 1)}}
    if dumped is not None:
        out["dump_outputs"] = dumped

    # ---- roofline of the dominant kernel: per-launch HIP events on the launch stream -----------------
    if not args.no_roofline and rank != 0:
        for _ in range(3):                 # keep the collectives of rank 0's profiling steps matched
            eager_step()
    if not args.no_roofline and rank == 0:
        note("roofline pass (per-launch events)")
        out["roofline"] = roofline_of(net, eager_step, args.conv_dtype, ms, args.layers)
    if world == 1 and args.conv_dtype == "f32" and args.variant == 300 and not args.no_bf16_leg and _ops.wino_x3(4, 256) and net._engine.wino:
        # the same step with EVERY product on the f32 MFMA (the limb GEMMs switched off), a few steps beside the headline: what the
        # three-limb form buys on this device, and the number to hold against a reader who wants v_mfma_f32_32x32x2_f32 only
        from objectdetection_ssd_amd import _lib as _l3
        note("f32-MFMA-only leg")
        try:
            _l3.check(_l3.load().ssd_tune_set_wino_x3(0), "tune")
            net.invalidate_weight_cache()
            for _ in range(3):
                step()
            fence()
            m0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            fence()
            mms = (time.perf_counter() - m0) / args.steps * 1e3
        finally:
            _l3.check(_l3.load().ssd_tune_set_wino_x3(-1), "tune")
            net.invalidate_weight_cache()
        out["config"]["f32_mfma_only"] = {"images_per_sec": round(bs / mms * 1e3, 1), "ms_per_step": round(mms, 3), "steps": args.steps,
                                          "note": "same process, same batch, SSD_WINO_X3=0: all Winograd-domain and 1x1 products on v_mfma_f32_32x32x2_f32 / "
                                                  "16x16x4_f32 (the round-2 arithmetic); `value` uses three exact bf16 limbs per f32 operand for the long reductions"}
    if world == 1 and args.conv_dtype == "f32" and args.variant == 300 and not args.no_bf16_leg:
        # BASELINE configs[2] ("bf16 convs", 32 images per GPU): the same step with bf16-operand forward / dgrad / 3x3-wgrad convolutions
        # (f32 accumulate, f32 loss and optimizer), a few steps beside the headline so that the driver's record holds a number for it.
        # NOT `value`: the headline stays the f32 configuration the metric is quoted on.
        note("bf16 leg")
        net.conv_dtype = "bf16"
        for _ in range(3):
            step()
        fence()
        b0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        bms = (time.perf_counter() - b0) / args.steps * 1e3
        out["config"]["bf16_operand_mode"] = {"images_per_sec": round(bs / bms * 1e3, 1), "ms_per_step": round(bms, 3), "steps": args.steps,
                                              "note": "BASELINE configs[2] per-GPU leg: bf16 convolutions (VGG trunk: activations and gradients stored in "
                                                      "bf16), f32 accumulate / loss / SGD; same batch, same process",
                                              "direct_conv_tflops": round(TRAIN_GFLOP_PER_IMAGE * bs / bms, 2)}
        if not args.no_roofline:
            out["config"]["bf16_operand_mode"]["roofline"] = roofline_of(net, eager_step, "bf16", bms)
        net.conv_dtype = "f32"
    if world == 1 and gstep is None and args.variant == 300 and not args.no_bf16_leg:
        # the same step replayed from ONE HIP graph (ddp.GraphedTrainStep), a few steps beside the headline: host enqueue time and device time
        from objectdetection_ssd_amd.ddp import GraphedTrainStep
        note("graph-step leg")
        keep_overlap = trainer.overlap
        g2 = GraphedTrainStep(net, trainer, max_boxes_per_image=8, warmup=0, two_streams=not args.graph_one_stream)
        for _ in range(3):
            g2(x, classes, boxes)
        fence()
        g0 = time.perf_counter()
        for _ in range(args.steps):
            g2(x, classes, boxes)
        fence()
        gms = (time.perf_counter() - g0) / args.steps * 1e3
        ghost = 0.0
        for _ in range(3):
            fence()
            h0 = time.perf_counter()
            g2(x, classes, boxes)
            ghost += (time.perf_counter() - h0) / 3 * 1e3
        fence()
        trainer.overlap = keep_overlap
        out["config"]["graph_step"] = {"ms_per_step": round(gms, 3), "images_per_sec": round(bs / gms * 1e3, 1), "host_enqueue_ms_per_step": round(ghost, 2),
                                       "kernel_launches_in_graph": g2.kernel_nodes, "steps": args.steps,
                                       "note": "ddp.GraphedTrainStep: forward + loss + backward + SGD replayed from one HIP graph (bitwise equal to the "
                                               "eager step: tests/test_gpu_path.py::test_graphed_train_step_is_bitwise_the_eager_step); `value` is the "
                                               "eager step, whose host enqueue time is config.host_enqueue_ms_per_step"}
        del g2
    if world > 1:
        dist.barrier()
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        note("cpu baseline")
        out["cpu_baseline"], cpu_losses = cpu_baseline(variant=args.variant, bs_big=bs)
        if args.variant == 300 and cpu_losses is not None:
            # BASELINE.json metric: "loss delta vs CPU" -- same seeded batch, same seed-0 weights, HIP path vs the oracle
            g1, g2 = gpu_losses_at_oracle_weights(dev, bs, args.conv_dtype)
            out["loss_delta_vs_cpu"] = {"loc": abs(g1 - cpu_losses[0]), "conf": abs(g2 - cpu_losses[1]),
                                        "gpu": [g1, g2], "cpu": list(cpu_losses), "batch": bs,
                                        "tolerance": 1e-4, "conv_dtype": args.conv_dtype,
                                        "within_tolerance": bool(abs(g1 - cpu_losses[0]) <= 1e-4 * max(1.0, abs(cpu_losses[0])) and
                                                                 abs(g2 - cpu_losses[1]) <= 1e-4 * max(1.0, abs(cpu_losses[1])))}
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
