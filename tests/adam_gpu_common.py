"""What the two GPU test files of the fused Adam step share: the SSD_300 trainer at batch 2 that tests/test_graph_replay.py and
tests/test_grad_clip_gpu.py use, and the hand-back of pooled streams and cached workspaces those files' lifetime tests rely on."""
import gc

import numpy as np
import torch

import ssd_oracle as O
from helpers import synth_gt

DEV = "cuda:0"
BS = 2
_PARAMS = []
STREAM_OWNERS = []            # engines and graph steps built by a module: each takes streams from torch's pool


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def batch(seed, bs=BS):
    x = t(np.random.default_rng(100 + seed).standard_normal((bs, 3, 300, 300), dtype=np.float32))
    boxes, classes = synth_gt(np.random.default_rng(200 + seed), bs)
    return x, [t(c) for c in classes], [t(b) for b in boxes]


def trainer(lr=1e-4, **kw):
    from objectdetection_ssd_amd import Model
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    if not _PARAMS:
        _PARAMS.append(O.ssd300_random_params(8))
    net = Model.SSD_300()
    named = dict(net.named_parameters())
    with torch.no_grad():
        for k, v in _PARAMS[0].items():
            named[k].copy_(v)
    net = net.to(DEV).train()
    STREAM_OWNERS.append(net._engine)
    return net, FlatSGDDataParallel(net, lr=lr, weight_decay=1e-2, **kw)


def hand_back_streams_and_workspaces():
    """Generator body of a module-scoped autouse fixture (tests/test_grad_clip_gpu.py explains why): the workspace cache as it was,
    and torch's stream pool (32 per device, round-robin) at the position it had."""
    from objectdetection_ssd_amd import ops
    before = dict(ops._ws_cache)
    yield
    torch.cuda.synchronize()
    taken = 0
    for o in STREAM_OWNERS:
        taken += sum(getattr(o, a, None) is not None for a in ("_side_stream", "_wgrad_stream", "_stream"))
    del STREAM_OWNERS[:]
    ops._ws_cache.clear()
    ops._ws_cache.update(before)
    gc.collect()
    for _ in range(-taken % 32):
        torch.cuda.Stream(device=DEV)


def same_bits(a, b):
    """Bitwise equality of two f32 device tensors up to the payload of NaNs."""
    a, b = a.detach(), b.detach()
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, 0.0, 1.0, -1.0).view(torch.int32),
                                                                       torch.nan_to_num(b, 0.0, 1.0, -1.0).view(torch.int32))
