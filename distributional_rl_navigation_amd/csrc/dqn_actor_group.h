// dqn_actor_group.h -- what dqn_collect.hip (create / destroy / act) and replay.hip (append) share of an mn_dqn_actor_group: the device table row of one
// actor and the host object.  The kernels that read the table index it by blockIdx.y alone, so every pointer of a row arrives through scalar loads.
#pragma once
#include <stdint.h>

#include "marinenav_hip.h"

struct DqnActorRow {
    const float *weights[18];      // the network, in the order of the C ABI
    float *image;                  // the actor's permuted weight image
    uint64_t seed;                 // of its exploration draws
    float *ring_states, *ring_next_states;
    int64_t *ring_actions;
    float *ring_rewards, *ring_dones;
};

struct mn_dqn_actor_group {
    DqnActorRow *table_dev;
    int n_groups, rows;            // G, rows per group
    int device, n_cu;
    int grid;                      // workgroups per group of the act launch; 0: the default share (mn_dqn_actor_group_set_grid)
    bool rings;                    // every actor has its five ring arrays
};
