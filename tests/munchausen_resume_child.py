"""Child process of tests/test_munchausen_gpu.py::test_train_from_memory_is_sample_step_finish_and_resumes_in_a_fresh_process: a fresh agent with the Munchausen
target loads the saved state, takes the remaining gradient steps and saves what the parent compares.  Usage: munchausen_resume_child.py STATE STEPS OUT."""
import sys

import torch


def main(state_path, steps, out_path):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    sd = torch.load(state_path)
    ag = IQNAgent(26, 9, BATCH_SIZE=32, seed=991, BUFFER_SIZE=int(sd["ring"]["capacity"]), device="cuda:0", munchausen=True, **sd["option"])      # (another seed: everything comes from the state)
    ag.memory.load_state_dict(sd["ring"])
    ag.load_state_dict(sd["agent"])
    loss = None
    for _ in range(int(steps)):
        loss = ag.train_from_memory()
    ft = ag._fused
    torch.save(dict(local=ft.local.cpu(), exp_avg=ft.exp_avg.cpu(), exp_avg_sq=ft.exp_avg_sq.cpu(), step=ft.step_dev.cpu(), loss=loss.detach().cpu().reshape(1).clone(),
                    rng=ft.rng_state.cpu()), out_path)


if __name__ == "__main__":
    main(*sys.argv[1:4])
