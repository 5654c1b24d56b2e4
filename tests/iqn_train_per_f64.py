"""tests/iqn_train_f64.py's float64 statement of one IQN gradient step, extended by the importance weights of prioritized replay: element b's loss terms are
scaled by w[b],

    loss = (1 / B) sum_b w[b] * (|tau_l[b,i] - 1[td < 0]| * huber).sum(i).mean(j)        delta[b] = mean_ij |td[b,i,j]|

followed by the same clip and Adam.  The bars are that module's (`compare_step`); `compare_abs_td` holds the new output to them.  Plain helper module, no fixtures."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import torch

import iqn_train_f64 as H


def f64_step_weighted(local, target, exp, taus_target, taus_local, gamma_n, weights, m=None, v=None, t=0, lr=H.LR):
    """H.f64_step with weights [B]: the same namespace plus abs_td [B] (float64 numpy)."""
    local64, target64 = copy.deepcopy(local).double(), copy.deepcopy(target).double()
    params = list(local64.parameters())
    td, y = H._td(local64, target64, exp, taus_target, taus_local, gamma_n)
    a = td.abs()
    huber = torch.where(a <= 1.0, 0.5 * td * td, a - 0.5)
    weight = (taus_local.double().unsqueeze(2) - (td.detach() < 0).double()).abs()
    w = weights.double().to(td.device).view(-1)
    loss = ((weight * huber).sum(dim=1).mean(dim=1) * w).mean()
    grads = torch.autograd.grad(loss, params)
    g = torch.cat([x.reshape(-1) for x in grads])
    norm = float(torch.linalg.vector_norm(g))
    g = g * min(1.0, H.MAX_NORM / (norm + 1e-6))
    p0 = torch.cat([p.detach().reshape(-1) for p in params])
    dev = p0.device
    m0 = torch.zeros_like(p0) if m is None else torch.as_tensor(m, dtype=torch.float64, device=dev).reshape(-1)
    v0 = torch.zeros_like(p0) if v is None else torch.as_tensor(v, dtype=torch.float64, device=dev).reshape(-1)
    t1 = int(t) + 1
    m1 = H.B1 * m0 + (1 - H.B1) * g
    v1 = H.B2 * v0 + (1 - H.B2) * g * g
    p1 = p0 - lr / (1 - H.B1 ** t1) * m1 / (v1.sqrt() / math.sqrt(1 - H.B2 ** t1) + H.EPS)
    tdd = td.detach()
    n = lambda x: x.cpu().numpy()
    return SimpleNamespace(loss=float(loss.detach()), norm=norm, grad=n(g), params=n(p1), m=n(m1), v=n(v1), t=t1, p0=n(p0), abs_td=n(tdd.abs().mean(dim=(1, 2))),
                           lin_share=float((tdd.abs() > 1.0).double().mean()), min_abs_td=float(tdd.abs().min()),
                           min_kink=float((tdd.abs() - 1.0).abs().min()), max_abs_y=float(y.abs().max()))


def case_weights(B, seed=0):
    """Importance weights as the sampler hands them out: in (0, 1], the largest exactly 1."""
    g = torch.Generator().manual_seed(9000 + B + seed)
    w = 0.05 + 0.95 * torch.rand(B, generator=g)
    return (w / w.max()).float()


def compare_abs_td(ref_abs_td, fused_abs_td, eager_abs_td, label="", rows=None):
    """The elements' mean |TD error| of the fused step against float64, under compare_step's bar for a vector: MAX_FACTOR x eager's largest error + FLOOR x the
    largest entry."""
    ref = np.asarray(ref_abs_td, dtype=np.float64)
    ef = float(np.abs(np.asarray(fused_abs_td, dtype=np.float64) - ref).max())
    ee = float(np.abs(np.asarray(eager_abs_td, dtype=np.float64) - ref).max())
    bar = H.MAX_FACTOR * ee + H.FLOOR * float(np.abs(ref).max())
    line = f"{label:34s} {'abs_td max':14s} fused {ef:10.3e}  eager {ee:10.3e}  bar {bar:10.3e}"
    if rows is not None:
        rows.append(line)
    assert ef <= bar, line
