"""Acting after a PyTorch gradient step (`IQNAgent.train` with `use_fused_train = False`, train_iqn --torch-train) uses the NEW weights.

The act kernel works from a cached weight image that is rebuilt when a parameter's version counter moves (iqn/fused_act.py).  torch.optim.Adam(fused=True) --
the optimizer of the PyTorch path on the GPU -- writes the weights without moving it, so `train` tells the act context itself.  Without that call acting went on
with the image of its first pack for the whole run."""
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _agent(torch, lr):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=32, BUFFER_SIZE=256, device=DEV, seed=5, LR=lr)
    ag.use_fused_train = False
    g = torch.Generator().manual_seed(1)
    ag.memory.add_batch(torch.rand(256, 26, generator=g).to(DEV), torch.randint(0, 9, (256,), generator=g).to(DEV), (torch.rand(256, generator=g) - 0.5).to(DEV),
                        torch.rand(256, 26, generator=g).to(DEV), (torch.rand(256, generator=g) < 0.1).float().to(DEV))
    return ag


def test_q_values_of_the_act_kernel_follow_a_torch_gradient_step(torch):
    from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
    ag = _agent(torch, lr=1e-2)      # a learning rate at which one step moves every Q-value visibly
    states = torch.rand(64, 26, generator=torch.Generator().manual_seed(2)).to(DEV)
    taus = torch.rand(64, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    before = ag.qvals_batch(states, taus=taus).clone()      # the act kernel packs its weight image here
    flat0 = torch.cat([p.detach().reshape(-1) for p in ag.qnetwork_local.parameters()]).clone()
    for _ in range(3):
        ag.train_from_memory()
    assert not torch.equal(flat0, torch.cat([p.detach().reshape(-1) for p in ag.qnetwork_local.parameters()]))
    after = ag.qvals_batch(states, taus=taus).clone()
    assert not torch.equal(before, after)                   # the kernel saw the step ...
    weights_changed(ag.qnetwork_local)
    assert torch.equal(after, ag.qvals_batch(states, taus=taus))      # ... all of it: a forced re-pack changes nothing
    with torch.no_grad():      # and it is the network PyTorch holds now: the kernel's float32-class rounding is far below what three steps at this rate move
        eager = ag.qnetwork_local.get_qvals(states, 1.0, taus=taus)
    err_after, err_before = float((after - eager).abs().max()), float((before - eager).abs().max())
    print("act kernel vs PyTorch: after the steps", err_after, "| the image from before the steps", err_before)
    assert err_before > 10 * err_after
