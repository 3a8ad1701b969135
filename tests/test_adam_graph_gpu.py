"""The replayed train step over an AdamW trainer with a cosine schedule, the weight EMA, clipping and the guard: captured once,
right after the warm-up, and bitwise the same five steps run eagerly on an identically seeded net."""
import numpy as np
import pytest
import torch

from adam_gpu_common import STREAM_OWNERS, batch, hand_back_streams_and_workspaces, same_bits, trainer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_streams_and_workspaces_as_found():
    yield from hand_back_streams_and_workspaces()


def test_graphed_adamw_step_is_captured_once_and_is_the_eager_step():
    from objectdetection_ssd_amd import Losses
    from objectdetection_ssd_amd.ddp import GraphedTrainStep
    from objectdetection_ssd_amd.optim import LRSchedule
    kw = dict(optimizer="adamw", schedule=LRSchedule.cosine(8, warmup_steps=2), ema_decay=0.9, max_grad_norm=50.0, skip_nonfinite=True)
    (n0, t0), (n1, t1) = trainer(**kw), trainer(**kw)
    gstep = GraphedTrainStep(n1, t1, max_boxes_per_image=8, warmup=2)
    STREAM_OWNERS.append(gstep)
    graph = None
    for step in range(5):
        x, cl, bx = batch(step)
        t0.zero_grad()
        l1, l2, n_pos = Losses.ssd(n0(x), cl, bx, norm_mode=1, with_n_pos=True)
        (l1 + l2).backward()
        t0.reduce_and_step(n_pos)
        g1, g2, gn = gstep(x, cl, bx)
        torch.cuda.synchronize()
        assert np.isfinite(float(l1)) and np.isfinite(float(l2)), f"the eager step diverged at step {step}"
        assert float(g1) == float(l1) and float(g2) == float(l2) and float(gn) == float(n_pos), (step, float(g1), float(l1))
        for name in ("flat_param", "flat_mom", "flat_sq", "flat_ema"):
            assert torch.equal(getattr(t0, name), getattr(t1, name)), f"{name} differs after step {step}"
        assert t0._adam_state.cpu().numpy().tobytes() == t1._adam_state.cpu().numpy().tobytes()
        assert torch.equal(t0._sched_state, t1._sched_state) and same_bits(t0._clip_state[:3], t1._clip_state[:3])
        assert int(t1.adam_steps) == int(t1.step_count) == step + 1 == t1.steps == t0.steps and int(t1.skipped_steps) == 0
        print(f"step {step}: clip coefficient {float(t1.clip_coef)!r}, lr {t1.current_lr.tolist()}, ema weight {float(t1.ema_weight)!r}")
        if step < 2:
            assert gstep.graph is None
        elif step == 2:                                              # no first launch of another form to wait for: captured at once
            graph = gstep.graph
            assert graph is not None
            print(f"kernel nodes of the captured AdamW step: {gstep.kernel_nodes}")
    assert gstep.graph is graph, "the step was captured again"
    t0.close()
    t1.close()
