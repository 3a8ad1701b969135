"""`ddp.GraphedTrainStep(conf_loss="focal")`: the captured step with the sigmoid focal classification term is bitwise the eager step
with `Losses.ssd(..., conf_loss="focal", norm_mode=1)`, captured once; an object built without the keywords has the signature it
always had and captures the graph of one built with `conf_loss="ce"`; the focal graph holds the two more launches of the term."""
import numpy as np
import pytest
import torch

from test_box_loss_graph_gpu import _batch, _nets      # the smallest net and batch of that test

pytestmark = pytest.mark.gpu
FOCAL = dict(conf_loss="focal", focal_alpha=0.25, focal_gamma=2.0)


def test_the_captured_focal_step_is_the_eager_one_bit_for_bit():
    from objectdetection_ssd_amd import Losses
    from objectdetection_ssd_amd.ddp import GraphedTrainStep
    nets, trs = _nets(2, 0.9)
    for net in nets:
        net.init_conf_prior()
    gstep = GraphedTrainStep(nets[1], trs[1], max_boxes_per_image=8, warmup=2, **FOCAL)
    assert gstep._signature()[-3:] == ("focal", 0.25, 2.0)
    graph = None
    for it in range(5):                                            # two warm-up steps, then three replays
        x, cl, bx = _batch(it)
        trs[0].zero_grad()
        l1, l2, n_pos = Losses.ssd(nets[0](x), cl, bx, norm_mode=1, with_n_pos=True, **FOCAL)
        (l1 + l2).backward()
        trs[0].reduce_and_step(n_pos)
        g1, g2, gn = gstep(x, cl, bx)
        torch.cuda.synchronize()
        assert np.isfinite(l1.item()) and np.isfinite(l2.item()) and l2.item() > 0
        assert float(g1) == l1.item() and float(g2) == l2.item() and float(gn) == float(n_pos), (it, float(g2), l2.item())
        assert torch.equal(trs[0].flat_param, trs[1].flat_param), f"weights differ after step {it}"
        assert torch.equal(trs[0].flat_mom, trs[1].flat_mom), f"momentum differs after step {it}"
        if it == gstep.warmup:
            graph = gstep.graph
            assert graph is not None
        elif it > gstep.warmup:
            assert gstep.graph is graph                            # one capture
    # the term is not the cross entropy
    x, cl, bx = _batch(0)
    with torch.no_grad():
        out = nets[0](x)
    assert Losses.ssd(out, cl, bx, norm_mode=1, **FOCAL)[1].item() != Losses.ssd(out, cl, bx, norm_mode=1)[1].item()


def test_the_default_captures_the_graph_it_always_did():
    from objectdetection_ssd_amd.ddp import GraphedTrainStep
    nets, trs = _nets(3, 0.0)
    steps = [GraphedTrainStep(nets[0], trs[0], max_boxes_per_image=8, warmup=1),
             GraphedTrainStep(nets[1], trs[1], max_boxes_per_image=8, warmup=1, conf_loss="ce", focal_alpha=0.5, focal_gamma=1.0),
             GraphedTrainStep(nets[2], trs[2], max_boxes_per_image=8, warmup=1, **FOCAL)]
    assert steps[0].conf_loss == "ce" and steps[0]._signature()[-1] == "l1" and steps[0]._signature() == steps[1]._signature()
    assert steps[2]._signature()[:-3] == steps[0]._signature()
    for it in range(3):
        x, cl, bx = _batch(20 + it)
        a = [float(v) for v in steps[0](x, cl, bx)]
        b = [float(v) for v in steps[1](x, cl, bx)]
        c = [float(v) for v in steps[2](x, cl, bx)]
        assert a == b
        if it == 0:                                                # the same weights still: only the classification term differs
            assert c[0] == a[0] and c[2] == a[2] and c[1] != a[1]
    torch.cuda.synchronize()
    assert all(s.graph is not None and s.kernel_nodes is not None for s in steps)
    assert steps[0].kernel_nodes == steps[1].kernel_nodes
    assert steps[2].kernel_nodes == steps[0].kernel_nodes + 2      # the dense pass and its sum beside the three launches
    assert torch.equal(trs[0].flat_param, trs[1].flat_param)
