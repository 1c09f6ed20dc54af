/* mi_pdd.h — C ABI of libmirl_pdd.so: prioritized dueling Double DQN (Wang et al. 2016: the dueling head under van Hasselt's double target, trained on
 * Schaul's prioritized replay) on CartPole-v1, for gfx950.
 *
 * A seventh library beside libmirl.so (include/mi_rl.h), libmirl_pg.so (include/mi_reinforce.h), libmirl_c51.so (include/mi_c51.h), libmirl_iqn.so
 * (include/mi_iqn.h), libmirl_qr.so (include/mi_qr.h) and libmirl_ddqn.so (include/mi_ddqn.h).  It needs no symbol of the other six; the one thing it shares is the
 * env handle made by libmirl's mi_env_create (a host struct of device pointers, csrc/mi_common.h `struct mi_env`), which this library reads and advances.  The
 * prioritized SAMPLER (the priorities ring, its chunk sums, the importance weights, the priority scatter) stays libmirl's mi_per_*: this library only takes a
 * weight per batch row and gives |td| per batch row back.
 *
 * The reference has no script that combines the three.  The algorithm is dqn.py's loop, storage, seeding order, printed line and hyper-parameters with three
 * changes: the QNetwork of dueling_dqn.py, the double target (the ONLINE network chooses the successor's action, the TARGET network values it) and per.py's
 * weighted loss.  The yardsticks are the C oracle's DQN acting (oracle/cpu_ref.py: dqn_act_steps), a float64 torch restatement (tests/_pdd_ref.py), libmirl's
 * dueling image run through libmirl_ddqn.so, and the same algorithm written as a plain torch script (tools/capture_pdd_ref.py).
 *
 * Conventions
 *   - every call returns MI_PDD_OK (0) or a negative MI_PDD_E* code; mi_pdd_last_error() gives the text (thread-local).  NULL / 0 arguments are errors, never
 *     crashes.
 *   - all pointers are DEVICE pointers unless said otherwise; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: everything is enqueued on `stream`.
 *   - parameter vectors, observation arrays and the workspace must be 16-byte aligned (they are read and written as float4); anything else is MI_PDD_EINVAL.
 *
 * Network and flat parameter layout (order of parameters(), 11,019 floats: libmirl's MI_DUELING layout, the QNetwork of dueling_dqn.py):
 *     W1 [120][4] at 0, b1 [120] at 480, W2 [84][120] at 600, b2 [84] at 10,680, Wv [84] at 10,764, bv at 10,848, Wa [2][84] at 10,849, ba [2] at 11,017
 *     Linear(4,120) -> ReLU -> Linear(120,84) -> ReLU -> { value Linear(84,1), advantage Linear(84,2) } -> value + (advantage - mean advantage)
 *   The head starts at an odd offset: it is read element by element, never as float4.
 *
 * Numerics contract, fp32 (tests/_pdd_ref.py states the same algorithm in torch).  fmaf(a, b, c) is the fused a * b + c; nothing else is contracted.  "chain over
 * k of (w_k, v_k) from s" means acc = s; for ascending k: acc = fmaf(w_k, v_k, acc).
 *   Torso (csrc/mi_torso.h, the expressions of mi_c51.h / mi_qr.h / mi_ddqn.h):
 *     z1_u = fmaf(W1[u][3], x3, fmaf(W1[u][2], x2, fmaf(W1[u][1], x1, fmaf(W1[u][0], x0, b1[u]))));  h1_u = max(z1_u, 0)
 *     P_c[o] = chain over k = 40 c .. 40 c + 39 of (W2[o][k], h1_k) from b2[o] for c = 0 and from 0 for c = 1, 2
 *     z2_o = (P_0[o] + P_1[o]) + P_2[o];  h2_o = max(z2_o, 0)
 *   THE definition of the two action values — one for the acting launch, mi_pdd_target, mi_pdd_grad / mi_pdd_update and mi_pdd_forward alike:
 *     v   = chain over k < 84 of (Wv[k], h2_k) from bv
 *     A_a = chain over k < 84 of (Wa[a][k], h2_k) from ba[a]             (three independent chains; the bias is each chain's start)
 *     m   = (A_0 + A_1) * 0.5f                                           (the mean over the two actions of ONE row, dueling_dqn.py:40)
 *     q_a = v + (A_a - m)
 *     argmax = (q_1 > q_0) ? 1 : 0                                       (a bit-for-bit tie goes to action 0, as torch.argmax)
 *   Target of batch row b with ring row i and successor nx:
 *     a* = argmax of the ONLINE network at obs[nx]  -> next_actions[b], written for terminated rows too
 *     target[b] = r[nx] + lg * q'_{a*}, q' the TARGET network's values at obs[nx], lg = terminated[nx] ? 0 : gamma   (a product and a sum, not fused)
 *   Loss and gradient, inv = 1.0f / (float)B, w_b = weights[b], or exactly 1.0f when `weights` is NULL:
 *     current[b] = q_a of the online network at obs[i], a = (actions[i] != 0);  td = target[b] - current[b]
 *     td_abs[b] = fabsf(td)                                              (unweighted, per.py:144: the new priority)
 *     rowloss_b = w_b * (td * td)
 *     d = -(((2.0f * td) * w_b) * inv)                                   (d loss / d current[b])
 *     loss = SUMROWS(rowloss) * inv, the rows added in the slab order below
 *   Backward of row b, e = 0.5f * d (exact):
 *     dbv += d, dWv[k] += d * h2_k
 *     dba[a] += e, dba[1 - a] += -e, dWa[a][k] += e * h2_k, dWa[1 - a][k] += (-e) * h2_k        (every "+= x * h" is acc = fmaf(x, h, acc) over the rows the
 *                                                                                                 workgroup owns; q_a = v + 0.5 A_a - 0.5 A_{1-a})
 *     dz2_k = h2_k > 0 ? (d * Wv[k]) + (e * (Wa[a][k] - Wa[1 - a][k])) : 0                       (a difference, two products, one sum: nothing fused)
 *     dW2[o][k] += dz2_o * h1_k, db2[o] += dz2_o
 *     dh1_k = R_0 + R_1, R_c = chain over o = 42 c .. 42 c + 41 of (dz2_o, W2[o][k]) from 0;  dz1 = h1 > 0 ? dh1 : 0
 *     dW1[u][c] += dz1_u * x_c, db1[u] += dz1_u
 *   Summation order over the rows: workgroup g of G = min(B, MI_PDD_MAX_SLABS) owns rows g, g + G, ... and accumulates them in that order into its slab (from 0);
 *   the G slabs are added in 16 groups (g mod 16), each in ascending g on four interleaved accumulators ((s0 + s1) + (s2 + s3)), the 16 group sums in ascending
 *   group.  No floating-point atomics anywhere: two runs give the same bits.
 *   Adam: torch's single-tensor Adam, the element step and the host-side coefficients of libmirl's mi_adam (bit-identical to it).
 *
 * Replay ring: the layout and successor rule of libmirl's DQN ring: observations f32 [slots][N][4], actions i64 [slots][N], rewards f32 [slots][N], terminated u8
 *   [slots][N]; slot g % slots holds obs_g and the action taken from it, slot (g + 1) % slots the resulting reward / terminated / next observation (the RESET
 *   observation after a done).  A flat index is slot * N + env; its successor is ((slot + 1) % slots) * N + env.  `terminated` excludes TimeLimit truncation.
 *
 * RNG contract (counter-based Philox4x32-10 as in mi_rl.h), libmirl's streams 0, 3 and 4 unchanged, no new stream:
 *   - reset noise: stream 0, idx = episode[n]
 *   - exploration: stream 3, idx = the env step counter step_ctr[n]: u = (w0 >> 8) / 2^24 is compared with epsilon, w1 & 1 is the random action.
 *     epsilon = (float)max(slope * global_step + start_e, end_e), the double arithmetic of dqn.py rounded once to f32 as mi_dqn_act_steps does, slope =
 *     (end_e - start_e) / (exploration_fraction * total_timesteps).  A step with global_step < learning_starts takes the random action whatever epsilon says.
 *   - uniform minibatch sampling (sample_upper > 0): stream 4, env := update index, idx := row b; index = (w0 | w1 << 32) mod upper   (the contract of mi_dqn_sample)
 */
#ifndef MI_PDD_H
#define MI_PDD_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h" /* mi_episode_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_PDD_VERSION 1
#define MI_PDD_NPARAMS 11019
#define MI_PDD_H1 120
#define MI_PDD_H2 84
#define MI_PDD_W1 0
#define MI_PDD_B1 480
#define MI_PDD_W2 600
#define MI_PDD_B2 10680
#define MI_PDD_WV 10764
#define MI_PDD_BV 10848
#define MI_PDD_WA 10849
#define MI_PDD_BA 11017
#define MI_PDD_MAX_SLABS 128
#define MI_PDD_SLAB_STRIDE 11020   /* MI_PDD_NPARAMS + the row losses' sum (a multiple of 4) */
#define MI_PDD_MAX_STEPS_PER_CALL 64

enum { MI_PDD_OK = 0, MI_PDD_EINVAL = -1, MI_PDD_EHIP = -2 };

typedef struct mi_pdd_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_pdd_ring_t;

typedef struct mi_pdd_act_t {
    const float* params;             /* [11,019] online network */
    float* obs_cur;                  /* [N][4] carried in / out */
    const int64_t* forced_actions;   /* [n_steps][N] nullable */
    const double* forced_resets;     /* [n_steps][N][4] nullable */
    mi_episode_t* episodes;          /* [max_ep], nullable together with max_ep == 0 */
    int32_t* episode_stats;          /* [4] nullable: the call zeroes it, the launch accumulates {finished episodes, sum of lengths, longest, slots handed out} */
    int64_t global_step;             /* time steps already taken */
    int64_t total_timesteps;
    int64_t learning_starts;         /* steps before it take the keyed random action (0: no such steps) */
    double start_e;                  /* epsilon = max(slope * global_step + start_e, end_e) */
    double end_e;
    double exploration_fraction;
    int32_t n_steps;                 /* 1 .. 64 */
    int32_t max_ep;
} mi_pdd_act_t;

/* mi_ddqn_batch_t with two members behind it */
typedef struct mi_pdd_batch_t {
    const float* params;         /* [11,019] online network (mi_pdd_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [11,019] */
    int64_t* idx;                /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    float* current;              /* [batch] out: the online value of the stored action */
    float* target;               /* [batch] out */
    int32_t* next_actions;       /* [batch] out: the online network's greedy action at the successor */
    float* grads;                /* [11,019] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_pdd_workspace_bytes(batch) */
    uint64_t sample_seed;
    uint64_t sample_update;
    int64_t sample_upper;        /* > 0: row b's index is drawn in the launch (stream 4) and stored in idx; 0: idx is given */
    int32_t batch;               /* >= 1 */
    float gamma;
    void* mid_event;             /* nullable hipEvent_t recorded on `stream` between the two launches of mi_pdd_grad / mi_pdd_update (timing tools) */
    const float* weights;        /* [batch] nullable: the importance weight of each row (NULL: every row weighs exactly 1) */
    float* td_abs;               /* [batch] out, required by mi_pdd_grad / mi_pdd_update: |target - current|, unweighted */
} mi_pdd_batch_t;

typedef struct mi_pdd_adam_t {
    float* exp_avg;              /* [11,019] */
    float* exp_avg_sq;           /* [11,019] */
    int64_t step;                /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_pdd_adam_t;

int mi_pdd_version(void);
const char* mi_pdd_last_error(void);
const char* mi_pdd_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: PDD_ALLSRC) */
size_t mi_pdd_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* q [n][2] of obs [n][4] */
int mi_pdd_forward(const float* params, const float* obs, int n, float* q, void* stream);

/* a->n_steps (<= 64) time steps of the N envs of `handle` (a CartPole handle of libmirl's mi_env_create; N must equal ring->n_envs), ONE launch: epsilon-greedy
 * action, env.step with auto-reset and the 500-step TimeLimit, ring store; t of an episode record = the step index within the call */
int mi_pdd_act_steps(void* handle, const mi_pdd_ring_t* ring, const mi_pdd_act_t* a, void* stream);

/* next_actions [batch] and target [batch] of the rows b->idx from b->params (the action) and b->target_params (its value); one launch.  Reads of `b`: params,
 * target_params, idx, next_actions, target, batch, gamma */
int mi_pdd_target(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, void* stream);

/* weighted loss, |td| and gradient of one batch: two launches (targets + online forward + loss + backward into per-workgroup slabs; fixed-order slab sum) */
int mi_pdd_grad(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, void* stream);
/* the same two launches, the second of which also applies optimizer.step() to every gradient element it has just summed: bit-identical to mi_pdd_grad followed by
 * libmirl's mi_adam */
int mi_pdd_update(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, const mi_pdd_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
