"""Gradient-norm clipping and the non-finite step guard, the parts that need no GPU: the numpy restatement against torch's own
clip_grad_norm_, the exported symbols, argument checking of both optimizers, and the data-parallel bookkeeping at world 2 under
gloo with torch stand-ins for the GPU-only `ops` wrappers (as tests/test_ddp_gloo.py stands in for `sgd_momentum_`)."""
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import grad_clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssd_grad_norm_partials", "ssd_grad_clip_finalize", "ssd_sgd_momentum_guarded")


# ---- the restatement against torch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
@pytest.mark.parametrize("factor", [0.5, 0.999, 1.0, 1.5, 1e-4])
def test_ref_coefficient_is_torchs_bit_for_bit(norm_type, factor):
    """torch returns the f32 total norm and scales the gradients in place by its coefficient: a gradient element that was 1.0 holds
    the coefficient afterwards.  The restatement, given torch's own norm, must produce the same bits."""
    g = torch.Generator().manual_seed(3)
    ps = [nn.Parameter(torch.zeros(s)) for s in ((1,), (3,), (7, 5), (1000,))]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)
    ps[1].grad[1] = 1.0                                            # the probe
    ref_norm = R.total_norm([p.grad.numpy() for p in ps], norm_type)
    max_norm = float(ref_norm) * factor
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=norm_type)
    assert total.dtype == torch.float32
    n = sum(p.numel() for p in ps)                                 # torch sums in f32: within n roundings of the f64 norm, not equal to it
    assert abs(total.item() - float(ref_norm)) <= n * 2.0 ** -24 * float(ref_norm)
    coef = R.clip_coef(np.float32(total.item()), max_norm)
    got = np.float32(ps[1].grad[1].item())
    if float(coef) < 1.0:
        assert got.tobytes() == coef.tobytes(), (got, coef)
    else:
        assert got == np.float32(1.0) and coef == np.float32(1.0)


def test_ref_norm_handles_wide_magnitudes_nan_and_pre_scale():
    a = np.array([1e18, -3e-20, 2.0, 0.0], np.float32)
    assert R.total_norm([a]) == np.float32(np.sqrt(np.float64(np.float32(1e18)) ** 2 + np.float64(np.float32(3e-20)) ** 2 + 4.0))
    assert R.total_norm([a], float("inf")) == np.float32(1e18)
    assert R.total_norm([np.array([1.0, -7.0], np.float32)], float("inf")) == np.float32(7.0)
    assert np.isnan(R.total_norm([np.array([1.0, np.nan], np.float32)], float("inf")))
    assert np.isnan(R.total_norm([np.array([1.0, np.nan], np.float32)]))
    assert R.total_norm([np.array([3.0, 4.0], np.float32)], pre_scale=0.25) == np.float32(1.25)
    assert R.clip_coef(np.float32(np.inf), 1.0) == 0.0 and np.isnan(R.clip_coef(np.float32(np.nan), 1.0))
    assert R.clip_coef(np.float32(5.0), None) == 1.0 and R.grad_scale(np.float32(1.0), 0.3) == np.float32(0.3)
    assert R.skips(np.inf, True) and R.skips(np.nan, True) and not R.skips(np.inf, False) and not R.skips(1.0, True)


# ---- exports and arguments -------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from objectdetection_ssd_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ssd_gfx950.h")).read()
    declared = set(re.findall(r"\b(ssd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.ssd_abi_version() == 1
    # the grid of the norm pass depends on n alone (host-side query)
    assert lib.ssd_grad_norm_slots(0) == 0 and lib.ssd_grad_norm_slots(4) == 1 and lib.ssd_grad_norm_slots(4096) == 1
    assert lib.ssd_grad_norm_slots(4100) == 2 and lib.ssd_grad_norm_slots(1 << 30) == lib.ssd_grad_norm_slots(1 << 28)


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 5, 3)          # 135 + 5 params: slots are padded to multiples of 4
        self.b = nn.Conv2d(5, 7, 1)
        self.g = nn.Parameter(torch.ones(1, 6, 1, 1))
        self._engine = types.SimpleNamespace(names=["a.weight", "a.bias", "b.weight", "b.bias", "g"], _wcache={"x": 1})


BAD = [dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan")), dict(max_grad_norm="1"),
       dict(norm_type=1.0), dict(norm_type=3), dict(norm_type=float("nan")), dict(norm_type=None),
       dict(skip_nonfinite=1), dict(skip_nonfinite=None), dict(skip_nonfinite="yes")]


@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v!r}" for d in BAD for k, v in d.items()])
def test_bad_clip_arguments_are_refused_by_both_optimizers(kw):
    from objectdetection_ssd_amd import optim
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    with pytest.raises(ValueError):
        optim.SGD([nn.Parameter(torch.zeros(3))], lr=0.1, **kw)
    with pytest.raises(ValueError):
        FlatSGDDataParallel(_Tiny(), lr=0.1, **kw)


def test_good_clip_arguments_and_state_dict_layout():
    from objectdetection_ssd_amd import optim
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    p = nn.Parameter(torch.zeros(3))
    plain = torch.optim.SGD([p], lr=0.1, momentum=0.9)
    for kw in (dict(), dict(max_grad_norm=2), dict(max_grad_norm=0.5, norm_type=float("inf")), dict(skip_nonfinite=True, norm_type=2)):
        o = optim.SGD([p], lr=0.1, momentum=0.9, **kw)
        assert (o.max_grad_norm, o.skip_nonfinite) == (kw.get("max_grad_norm"), kw.get("skip_nonfinite", False))
        assert o.grad_norm is None and o.clip_coef is None and o.skipped_steps is None       # no step yet
        sd = o.state_dict()
        assert set(sd) == set(plain.state_dict()) and sd["state"] == {}                      # torch's layout, no new state entries
        assert set(sd["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
        plain.load_state_dict(sd)
        t = FlatSGDDataParallel(_Tiny(), lr=0.1, **kw)
        assert set(t.state_dict()) == {"state", "param_groups", "flat_steps"}


# ---- world 2 under gloo ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torch_sgd(param, grad, buf, lr, momentum, weight_decay, grad_scale=None, first_step=False):
    g = grad * grad_scale if grad_scale is not None else grad.clone()
    g = g + weight_decay * param
    if first_step:
        buf.copy_(g)
    else:
        buf.mul_(momentum).add_(g)
    param.sub_(lr * buf)


def _install_standins(ops, log):
    """TEST stand-ins for the GPU-only wrappers, on CPU tensors: one partial slot per range."""
    def slots(n):
        return 1 if n else 0

    def partials_(grad, partials, slot0, norm_type=2.0):
        assert grad.numel() % 4 == 0 and grad.dtype == torch.float32 and partials.dtype == torch.float64
        log.append(("norm", grad.data_ptr(), grad.numel()))
        g = grad.double()
        partials[slot0] = (g * g).sum() if norm_type == 2 else (torch.tensor(float("nan")) if g.isnan().any() else g.abs().max())
        return slot0 + 1

    def finalize_(partials, n_slots, norm_type, max_norm, pre_scale, guard, state):
        log.append(("finalize", n_slots))
        pre = pre_scale.reshape(()).clone() if pre_scale is not None else torch.tensor(1.0)
        if norm_type == 2:
            total = (partials[:n_slots].sum().sqrt() * pre.double()).float()
        else:
            total = partials[:n_slots].max().float() * pre
        coef = torch.tensor(1.0)
        if max_norm is not None:
            coef = torch.clamp(float(max_norm) / (total + 1e-6), max=1.0)          # clip_grad_norm_'s own line
        skip = int(bool(guard) and not bool(torch.isfinite(total)))
        state[0], state[1], state[2] = total, coef, pre * coef
        ist = state.view(torch.int32)
        ist[3] = skip
        ist[4] += skip

    def guarded_(param, grad, buf, lr, momentum, weight_decay, grad_scale, first_step, skip):
        log.append(("sgd", int(skip)))
        if int(skip) == 0:
            _torch_sgd(param, grad, buf, lr, momentum, weight_decay, grad_scale, first_step)

    def unguarded_(*a, **k):
        log.append(("plain",))
        _torch_sgd(*a, **k)

    ops.grad_norm_slots, ops.grad_norm_partials_, ops.grad_clip_finalize_ = slots, partials_, finalize_
    ops.sgd_momentum_guarded_, ops.sgd_momentum_ = guarded_, unguarded_


def _clip_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from objectdetection_ssd_amd import ddp
        log = []
        _install_standins(ddp.ops, log)
        torch.manual_seed(0)
        tr = ddp.FlatSGDDataParallel(_Tiny(), lr=0.1, max_grad_norm=0.05, skip_nonfinite=True)
        tr.broadcast_parameters(0)
        out = []
        for step in range(4):
            tr.zero_grad()
            g = torch.Generator().manual_seed(1000 * step + rank)
            for p in tr.params:
                p.grad = torch.randn(p.shape, generator=g)
            if step == 2 and rank == 1:
                tr.params[0].grad.view(-1)[5] = float("inf")       # one rank's overflow reaches every rank through the sum
            tr.reduce_gradients(torch.tensor(3.0 + rank))
            reduced = [v.clone().numpy() for v in tr.grad_views]
            before = tr.flat_param.clone()
            del log[:]
            tr.step()
            # the norm reads flat_grad[:n] -- not the count slot, not the pad -- once, then one finalise, then two guarded launches
            assert log[0] == ("norm", tr.flat_grad.data_ptr(), tr.n) and log[1] == ("finalize", 1), log
            assert [e[0] for e in log[2:]] == ["sgd", "sgd"], log
            out.append(dict(reduced=reduced, inv=float(tr.inv_npos), norm=float(tr.grad_norm), coef=float(tr.clip_coef),
                            skipped=int(tr.skipped_steps), par=tr.flat_param.clone().numpy(), mom=tr.flat_mom.clone().numpy(),
                            moved=not torch.equal(before, tr.flat_param)))
        tr.max_grad_norm, tr.skip_nonfinite = None, False           # switched off: the plain launches again
        tr.zero_grad()
        for p in tr.params:
            p.grad = torch.ones(p.shape)
        tr.reduce_gradients(torch.tensor(1.0))
        del log[:]
        tr.step()
        assert log == [("plain",), ("plain",)], log
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_clipped_data_parallel_step_world2():
    """Both ranks read the same reduced buffer, so they report the same norm -- the f64 norm of the reduced gradient times
    1 / n_pos_global, to 1 f32 ulp -- apply the same coefficient and end with bit-identical parameters; a non-finite gradient on
    ONE rank skips the step on both."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_clip_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = out[0][1], out[1][1]
    for step, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["par"], y["par"]) and np.array_equal(x["mom"], y["mom"]), step
        assert x["inv"] == y["inv"] == 1.0 / 7.0 or abs(x["inv"] - 1.0 / 7.0) < 1e-8
        if step == 2:
            assert not np.isfinite(x["norm"]) and not np.isfinite(y["norm"])
            assert not x["moved"] and not y["moved"] and x["skipped"] == y["skipped"] == 1
            continue
        ref = R.total_norm(x["reduced"], 2.0, pre_scale=x["inv"])
        assert R.ulps(x["norm"], ref) <= 1 and x["norm"] == y["norm"], (step, x["norm"], float(ref))
        coef = R.clip_coef(np.float32(x["norm"]), 0.05)
        assert coef < 1.0 and np.float32(x["coef"]) == coef and x["coef"] == y["coef"]
        assert x["moved"] and x["skipped"] == (1 if step > 2 else 0)
