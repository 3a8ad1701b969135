"""`ddp.GraphedTrainStep(match="atss")`: the captured step with the ATSS matching is bitwise the eager step with
`Losses.ssd(..., match="atss", norm_mode=1)` over replays with different targets (the static box buffer holds spare rows, which must
be nobody's match), captured once; an object built without the keywords has the signature it always had and captures the graph of one
built with `match="iou"`; the ATSS graph holds the assignment pass beside the launches of the loss."""
import numpy as np
import pytest
import torch

from test_box_loss_graph_gpu import _batch, _nets      # the smallest net and batch of that test

pytestmark = pytest.mark.gpu
ATSS = dict(match="atss", atss_topk=9)


def test_the_captured_atss_step_is_the_eager_one_bit_for_bit():
    from objectdetection_ssd_amd import Losses
    from objectdetection_ssd_amd.ddp import GraphedTrainStep
    nets, trs = _nets(2, 0.9)
    gstep = GraphedTrainStep(nets[1], trs[1], max_boxes_per_image=8, warmup=2, loc_loss="giou", **ATSS)
    assert gstep.match == "atss" and gstep.atss_topk == 9 and gstep._signature()[-2:] == ("atss", 9)
    graph = None
    for it in range(4):                                            # two warm-up steps, then two replays with other targets
        x, cl, bx = _batch(it)
        trs[0].zero_grad()
        l1, l2, n_pos = Losses.ssd(nets[0](x), cl, bx, norm_mode=1, with_n_pos=True, loc_loss="giou", **ATSS)
        (l1 + l2).backward()
        trs[0].reduce_and_step(n_pos)
        g1, g2, gn = gstep(x, cl, bx)
        torch.cuda.synchronize()
        assert np.isfinite(l1.item()) and np.isfinite(l2.item()) and float(n_pos) > 0
        assert float(g1) == l1.item() and float(g2) == l2.item() and float(gn) == float(n_pos), (it, float(g1), l1.item())
        assert torch.equal(trs[0].flat_param, trs[1].flat_param), f"weights differ after step {it}"
        assert torch.equal(trs[0].flat_mom, trs[1].flat_mom), f"momentum differs after step {it}"
        if it == gstep.warmup:
            graph = gstep.graph
            assert graph is not None
        elif it > gstep.warmup:
            assert gstep.graph is graph                            # one capture
    # the rule is not the IoU rule
    x, cl, bx = _batch(0)
    with torch.no_grad():
        out = nets[0](x)
    assert Losses.ssd(out, cl, bx, norm_mode=1, with_n_pos=True, **ATSS)[2].item() != Losses.ssd(out, cl, bx, norm_mode=1, with_n_pos=True)[2].item()


def test_the_default_captures_the_graph_it_always_did():
    from objectdetection_ssd_amd.ddp import GraphedTrainStep
    nets, trs = _nets(3, 0.0)
    steps = [GraphedTrainStep(nets[0], trs[0], max_boxes_per_image=8, warmup=1),
             GraphedTrainStep(nets[1], trs[1], max_boxes_per_image=8, warmup=1, match="iou", atss_topk=5),
             GraphedTrainStep(nets[2], trs[2], max_boxes_per_image=8, warmup=1, **ATSS)]
    assert steps[0].match == "iou" and steps[0]._signature()[-1] == "l1" and steps[0]._signature() == steps[1]._signature()
    assert steps[2]._signature()[:-2] == steps[0]._signature()
    for it in range(3):
        x, cl, bx = _batch(20 + it)
        a = [float(v) for v in steps[0](x, cl, bx)]
        b = [float(v) for v in steps[1](x, cl, bx)]
        c = [float(v) for v in steps[2](x, cl, bx)]
        assert a == b
        if it == 0:
            assert c[2] != a[2]
    torch.cuda.synchronize()
    assert all(s.graph is not None and s.kernel_nodes is not None for s in steps)
    assert steps[0].kernel_nodes == steps[1].kernel_nodes
    assert steps[2].kernel_nodes >= steps[0].kernel_nodes + 1      # the assignment pass (its memset may or may not count as a kernel)
    assert torch.equal(trs[0].flat_param, trs[1].flat_param)
    with pytest.raises(ValueError):
        GraphedTrainStep(nets[0], trs[0], match="nearest")
    with pytest.raises(ValueError):
        GraphedTrainStep(nets[0], trs[0], match="atss", atss_topk=33)
