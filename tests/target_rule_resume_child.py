"""Child process of tests/test_target_rule_gpu.py: one `train_iqn` run in the current directory (which holds config.json), in a process of its own -- the straight
run, the stopped one, or the fresh process that resumes it.  Usage: target_rule_resume_child.py DEVICE [train_iqn arguments ...]."""
import sys


def main(device, *args):
    from distributional_rl_navigation_amd import train_iqn
    train_iqn.main(["-C", "config.json", "-D", device, "--run-name", "toy", *args])


if __name__ == "__main__":
    main(*sys.argv[1:])
