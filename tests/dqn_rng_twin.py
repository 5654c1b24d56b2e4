"""Host twin of the draws of the DQN collect kernels (csrc/dqn_collect.hip: mn_dqn_act_rng, mn_dqn_actor_group_act), from the functions of
tests/rng_twin.py: row e of act call number `ctr` under `seed` draws u01(e, draw_keys(seed, ctr)); the action rule is the IQN epilogue's
(`rng_twin.explore_action`).  In the grouped launch `e` is the row inside the actor's group.  No torch, no GPU.  Plain helper module, no fixtures."""
import numpy as np

import rng_twin


def dqn_act_uniforms(seed, ctr, n):
    """The [n] exploration uniforms of one act call, float32."""
    return rng_twin.u01(np.arange(n, dtype=np.uint64), *rng_twin.draw_keys(seed, ctr))


def dqn_actions(seed, ctr, eps, greedy):
    """The actions of one act call given every row's greedy action: greedy iff u > eps, else min((int)(u / eps * 9.0f), 8); !(eps > 0): greedy everywhere."""
    greedy = np.asarray(greedy)
    return rng_twin.explore_action(dqn_act_uniforms(seed, ctr, greedy.shape[0]), eps, greedy)
