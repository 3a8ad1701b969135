"""CPU restatement of the sigmoid focal classification term of the MultiBox loss (ssd_multibox_loss_focal, conf_mode 1; DESIGN.md
section 4m), in torch, parametrised by dtype, the gradient by autograd.

conf is (bs, P, C); columns 0 .. C-2 are one-against-all logits, column C-1 (the background column) is not read.  For every prior that
is not ignored and every column c < C-1, with x = conf[i, p, c], t = (cls[i, p] == c) and z = x where t, -x elsewhere:
    FL = a_t exp(-gamma softplus(z)) softplus(-z),      a_t = alpha where t, 1 - alpha elsewhere; 1 everywhere where alpha < 0
which is alpha_t (1 - p_t)^gamma times the binary cross entropy with logits (1 - p_t = sigmoid(-z) = exp(-softplus(z))).
conf_loss = the sum of FL / n_pos (norm_mode 0) or the sum (norm_mode 1); dconf is its gradient -- `backward()` of that value, the
derivative is written out nowhere in this file -- and is zero in column C-1 and in the rows of ignored priors.  Matching, `pos`, `obj`,
`cls` and `ign` are tests/ignore_loss_ref.multibox_loss's.

`python tests/focal_loss_cases.py --record` measures, for every case of tests/focal_loss_cases.py and every parameter set, the distance
of the float32 restatement from the float64 one and writes tests/golden/focal_loss_ref_distance.json."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focal_loss_ref_distance.json")
PARAMS = ((0.25, 2.0), (0.5, 0.0), (-1.0, 1.5), (0.75, 5.0))          # (alpha, gamma)


def param_id(alpha, gamma):
    return f"a{alpha:g}-g{gamma:g}"


def elementwise(x, t, alpha, gamma):
    """FL of logits x against targets t (1.0 / 0.0), any shape, in x's dtype"""
    z = torch.where(t > 0.5, x, -x)
    a_t = torch.ones_like(x) if alpha < 0 else torch.where(t > 0.5, torch.full_like(x, alpha), torch.full_like(x, 1.0 - alpha))
    return a_t * torch.exp(-gamma * F.softplus(z)) * F.softplus(-z)


def conf_side(conf, cls, ign, n_pos, alpha, gamma, dtype=torch.float64, norm_mode=0):
    """loss_sum (the sum of FL), conf_loss and dconf (bs, P, C) of it, computed in `dtype`, returned as float64"""
    conf = np.asarray(conf, np.float32)
    bs, P, C = conf.shape
    x = torch.tensor(conf[..., :C - 1], dtype=dtype, requires_grad=True)
    t = torch.tensor(np.asarray(cls)[..., None] == np.arange(C - 1)[None, None], dtype=dtype)
    live = torch.tensor(~np.asarray(ign, bool), dtype=dtype)[..., None]
    fl = elementwise(x, t, alpha, gamma) * live
    total = fl.sum()
    value = total / n_pos if norm_mode == 0 else total
    value.backward()
    dconf = np.zeros((bs, P, C), np.float64)
    dconf[..., :C - 1] = x.grad.double().numpy()
    return dict(loss_sum=float(total.detach().double()), conf_loss=float(value.detach().double()), dconf=dconf,
                finite=bool(torch.isfinite(fl).all()) and bool(torch.isfinite(x.grad).all()))


def distance(case, base, alpha, gamma):
    """d32 of a case and parameter set: max |float32 restatement - float64| / max |float64| of dconf (elementwise arithmetic: the
    same on every run; the float32 loss sum depends on how the summation is split and is not recorded)"""
    a = conf_side(case.conf, base["cls"], base["ign"], base["n_pos"], alpha, gamma, torch.float32)
    b = conf_side(case.conf, base["cls"], base["ign"], base["n_pos"], alpha, gamma, torch.float64)
    big = np.abs(b["dconf"]).max()
    return dict(dconf=float(np.abs(a["dconf"] - b["dconf"]).max() / big))
