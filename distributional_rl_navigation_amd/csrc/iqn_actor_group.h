// iqn_actor_group.h -- what iqn_act.hip (create / destroy / act) and replay.hip (append) share of an mn_iqn_actor_group: the device table row of one
// actor and the host object.  The kernels that read the table index it by blockIdx.y alone, so every pointer of a row arrives through scalar loads.
#pragma once
#include <stdint.h>

#include "marinenav_hip.h"

struct IqnActorRow {
    const float *weights[14];      // the network, in the order of the C ABI
    float *consts;                 // the context's scale / bound constants
    uint32_t *packed;              // ... and its split-f16 weight image
    uint64_t *rng_state;           // {seed, call counter}
    float *draws;                  // [33 rows]
    uint32_t *rows_buf;            // the context's GreedyRows: 4 words, then the list [rows]
    float *ring_states, *ring_next_states;
    int64_t *ring_actions;
    float *ring_rewards, *ring_dones;
};

struct mn_iqn_actor_group {
    IqnActorRow *table_dev;
    int n_groups, rows;            // G, rows per group
    int device, n_cu;
    bool rings;                    // every actor has its five ring arrays
    mn_iqn_ctx *ctx[MN_IQN_MAX_ACTORS];
    uint32_t *rows_buf[MN_IQN_MAX_ACTORS];      // each context's greedy-row buffer as the table holds it (a larger single call would replace it)
};
