/* mi_nstep.h — C ABI of libmirl_nstep.so: n-step returns (Sutton 1988; the multi-step target of Rainbow, Hessel et al. 2018) under prioritized dueling Double
 * DQN on CartPole-v1, for gfx950.
 *
 * An eighth library beside libmirl.so (include/mi_rl.h), libmirl_pg.so, libmirl_c51.so, libmirl_iqn.so, libmirl_qr.so, libmirl_ddqn.so and libmirl_pdd.so
 * (include/mi_pdd.h).  It needs no symbol of the other seven.  It has NO acting and NO forward entry point: multi-step returns change the target alone, so an engine
 * acts and evaluates through libmirl_pdd.so on the same ring and the same 11,019-float vectors, and trains through this library.  The prioritized sampler stays
 * libmirl's mi_per_*, as for libmirl_pdd.so.
 *
 * Everything is mi_pdd.h's — the network and its flat layout, THE definition of the two action values and of argmax, the weighted loss with the unweighted td_abs,
 * the backward, the slab layout and summation order (MI_NS_MAX_SLABS workgroups, stride MI_NS_SLAB_STRIDE), Adam, the ring layout, the stream-4 sampling contract —
 * with ONE change, the target.  Read mi_pdd.h for those; the conventions (return codes, device pointers, 16-byte alignment, nothing synchronises) are its too.
 *
 * Numerics contract of the n-step target, fp32 (tests/_nstep_ref.py states it in torch).  Batch row b has flat ring index i = slot s_0, env e; n = n_step;
 * H = head_slot, the slot of the newest observation (global_step % slots: no action has been taken from it yet); succ(s) = (s + 1) % slots; every read is at
 * [s][e].  The walk is csrc/mi_nwalk.h's:
 *     s_1 = succ(s_0);  R = rewards[s_1];  g = gamma;  m = 1                          (step 1 is always taken)
 *     while m < n and terminated[s_m] == 0 and s_m != H:
 *         m += 1;  s_m = succ(s_{m-1})
 *         R = R + g * rewards[s_m]                                                    (a product, then a sum: not fused)
 *         g = g * gamma
 *     lg = terminated[s_m] ? 0.0f : g
 *     a* = argmax of the ONLINE network at observations[s_m]  -> next_actions[b], written for terminated rows too
 *     target[b] = R + lg * q'_{a*}(observations[s_m]), q' the TARGET network        (a product, then a sum)
 *     horizon[b] = m
 *   What follows from it:
 *   - n_step == 1 is mi_pdd.h's target expression for expression (R = r[nx], lg = terminated[nx] ? 0 : gamma): every output of mi_ns_grad then equals
 *     mi_pdd_grad's bit for bit, whatever head_slot is, and horizon is 1 everywhere.
 *   - The walk never uses a transition whose action has not been taken: it stops on reaching H.
 *   - The one exception is step 1 of a row that sits ON H after the ring has wrapped — dqn.py's stale row, which uniform sampling over the full ring already draws.
 *     Step 1 is taken there (so that n_step == 1 stays PDD) and the walk then runs on from s_1.
 *   - A terminated step ends the walk with no bootstrap; a termination at step n exactly gives the full reward sum and lg = 0.
 *   - Rewards and flags beyond the stop are selected out, never multiplied by zero: they may hold NaN.  Intermediate observations s_k, 0 < k < m, are not read.
 *   - `terminated` excludes TimeLimit truncation and the ring stores no truncation flag, so a walk runs on THROUGH a truncation into the reset observation and the
 *     next episode's rewards, exactly as the one-step target bootstraps from the reset observation there.  A `done` flag in the ring would remove this; the ring
 *     layout is shared with five other libraries and is not this library's to change.
 *   - 1 <= n_step <= MI_NS_MAX_N, n_step < slots, 0 <= head_slot < slots; anything else is MI_NS_EINVAL.
 */
#ifndef MI_NSTEP_H
#define MI_NSTEP_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_NS_VERSION 1
#define MI_NS_NPARAMS 11019
#define MI_NS_H1 120
#define MI_NS_H2 84
#define MI_NS_W1 0
#define MI_NS_B1 480
#define MI_NS_W2 600
#define MI_NS_B2 10680
#define MI_NS_WV 10764
#define MI_NS_BV 10848
#define MI_NS_WA 10849
#define MI_NS_BA 11017
#define MI_NS_MAX_SLABS 128
#define MI_NS_SLAB_STRIDE 11020   /* MI_NS_NPARAMS + the row losses' sum (a multiple of 4) */
#define MI_NS_MAX_N 16            /* the longest walk (Rainbow uses 3) */

enum { MI_NS_OK = 0, MI_NS_EINVAL = -1, MI_NS_EHIP = -2 };

/* layout-identical to mi_pdd_ring_t */
typedef struct mi_ns_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_ns_ring_t;

/* mi_pdd_batch_t with three members behind it */
typedef struct mi_ns_batch_t {
    const float* params;         /* [11,019] online network (mi_ns_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [11,019] */
    int64_t* idx;                /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    float* current;              /* [batch] out: the online value of the stored action */
    float* target;               /* [batch] out */
    int32_t* next_actions;       /* [batch] out: the online network's greedy action at the bootstrap observation s_m */
    float* grads;                /* [11,019] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_ns_workspace_bytes(batch) */
    uint64_t sample_seed;
    uint64_t sample_update;
    int64_t sample_upper;        /* > 0: row b's index is drawn in the launch (stream 4) and stored in idx; 0: idx is given */
    int32_t batch;               /* >= 1 */
    float gamma;
    void* mid_event;             /* nullable hipEvent_t recorded on `stream` between the two launches of mi_ns_grad / mi_ns_update (timing tools) */
    const float* weights;        /* [batch] nullable: the importance weight of each row (NULL: every row weighs exactly 1) */
    float* td_abs;               /* [batch] out, required by mi_ns_grad / mi_ns_update: |target - current|, unweighted */
    int32_t* horizon;            /* [batch] out, required by all three: m, the steps the row's walk took */
    int32_t n_step;              /* 1 .. MI_NS_MAX_N, < slots */
    int64_t head_slot;           /* 0 .. slots - 1: global_step % slots at the time of the call */
} mi_ns_batch_t;

/* layout-identical to mi_pdd_adam_t */
typedef struct mi_ns_adam_t {
    float* exp_avg;              /* [11,019] */
    float* exp_avg_sq;           /* [11,019] */
    int64_t step;                /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_ns_adam_t;

int mi_ns_version(void);
const char* mi_ns_last_error(void);
const char* mi_ns_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: NS_ALLSRC) */
size_t mi_ns_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* next_actions [batch], target [batch] and horizon [batch] of the rows b->idx; one launch.  Reads of `b`: params, target_params, idx, next_actions, target,
 * horizon, batch, gamma, n_step, head_slot */
int mi_ns_target(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, void* stream);

/* weighted loss, |td|, horizon and gradient of one batch: two launches (walk + targets + online forward + loss + backward into per-workgroup slabs; fixed-order
 * slab sum) */
int mi_ns_grad(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, void* stream);
/* the same two launches, the second of which also applies optimizer.step() to every gradient element it has just summed: bit-identical to mi_ns_grad followed by
 * libmirl's mi_adam */
int mi_ns_update(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, const mi_ns_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
