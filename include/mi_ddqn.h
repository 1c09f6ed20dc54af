/* mi_ddqn.h — C ABI of libmirl_ddqn.so: Double DQN (van Hasselt, Guez, Silver 2016) on CartPole-v1, for gfx950.
 *
 * A sixth library beside libmirl.so (include/mi_rl.h), libmirl_pg.so (include/mi_reinforce.h), libmirl_c51.so (include/mi_c51.h), libmirl_iqn.so
 * (include/mi_iqn.h) and libmirl_qr.so (include/mi_qr.h).  It needs no symbol of the other five; the one thing it shares is the env handle made by libmirl's
 * mi_env_create (a host struct of device pointers, csrc/mi_common.h `struct mi_env`), which this library reads and advances.
 *
 * The reference has no double_dqn.py.  The algorithm is dqn.py's loop, storage, seeding order, printed line and hyper-parameters with the TD target replaced: the
 * ONLINE network chooses the successor's action, the TARGET network values it.  The yardsticks are the C oracle's DQN acting (oracle/cpu_ref.py: dqn_act_steps),
 * the identity Double DQN == DQN whenever the two networks are equal bit for bit, a float64 torch restatement (tests/_ddqn_ref.py) and the same algorithm written
 * as a plain torch script (tools/capture_ddqn_ref.py).
 *
 * Conventions
 *   - every call returns MI_DDQN_OK (0) or a negative MI_DDQN_E* code; mi_ddqn_last_error() gives the text (thread-local).  NULL / 0 arguments are errors, never
 *     crashes.
 *   - all pointers are DEVICE pointers unless said otherwise; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: everything is enqueued on `stream`.
 *   - parameter vectors, observation arrays and the workspace must be 16-byte aligned (they are read and written as float4); anything else is MI_DDQN_EINVAL.
 *
 * Network and flat parameter layout (order of parameters(), 10,934 floats: libmirl's MI_DQN layout, the QNetwork of dqn.py):
 *     W1 [120][4] at 0, b1 [120] at 480, W2 [84][120] at 600, b2 [84] at 10,680, W3 [2][84] at 10,764, b3 [2] at 10,932
 *     Linear(4,120) -> ReLU -> Linear(120,84) -> ReLU -> Linear(84,2)
 *
 * Numerics contract, fp32 (tests/_ddqn_ref.py states the same algorithm in torch).  fmaf(a, b, c) is the fused a * b + c; nothing else is contracted.  "chain over
 * k of (w_k, v_k) from s" means acc = s; for ascending k: acc = fmaf(w_k, v_k, acc).
 *   Torso (the expressions of mi_c51.h / mi_qr.h):
 *     z1_u = fmaf(W1[u][3], x3, fmaf(W1[u][2], x2, fmaf(W1[u][1], x1, fmaf(W1[u][0], x0, b1[u]))));  h1_u = max(z1_u, 0)
 *     P_c[o] = chain over k = 40 c .. 40 c + 39 of (W2[o][k], h1_k) from b2[o] for c = 0 and from 0 for c = 1, 2
 *     z2_o = (P_0[o] + P_1[o]) + P_2[o];  h2_o = max(z2_o, 0)
 *   THE definition of the two action values — one for the acting launch, mi_ddqn_target, mi_ddqn_grad / mi_ddqn_update and mi_ddqn_forward alike:
 *     q_a = chain over k < 84 of (W3[a][k], h2_k) from b3[a]              (two independent chains, a = 0 and a = 1; the bias is each chain's start)
 *     argmax = (q_1 > q_0) ? 1 : 0                                       (a bit-for-bit tie goes to action 0, as torch.argmax)
 *   Target of batch row b with ring row i and successor nx:
 *     a* = argmax of the ONLINE network at obs[nx]  -> next_actions[b], written for terminated rows too
 *     target[b] = r[nx] + lg * q'_{a*}, q' the TARGET network's values at obs[nx], lg = terminated[nx] ? 0 : gamma   (a product and a sum, not fused)
 *   Loss and gradient, inv = 1.0f / (float)B:
 *     current[b] = q_a of the online network at obs[i], a = (actions[i] != 0);  td = target[b] - current[b];  rowloss_b = td * td
 *     d = -((2.0f * td) * inv)                                           (d loss / d current[b]; the other action's value has no gradient)
 *     loss = SUMROWS(rowloss) * inv, the rows added in the slab order below
 *   Backward of row b:
 *     dW3[a][k] += d * h2_k, db3[a] += d (fmaf accumulation over the rows the workgroup owns; row 1 - a is not touched)
 *     dz2_k = h2_k > 0 ? d * W3[a][k] : 0
 *     dW2[o][k] += dz2_o * h1_k, db2[o] += dz2_o
 *     dh1_k = R_0 + R_1, R_c = chain over o = 42 c .. 42 c + 41 of (dz2_o, W2[o][k]) from 0;  dz1 = h1 > 0 ? dh1 : 0
 *     dW1[u][c] += dz1_u * x_c, db1[u] += dz1_u
 *   Summation order over the rows: workgroup g of G = min(B, MI_DDQN_MAX_SLABS) owns rows g, g + G, ... and accumulates them in that order into its slab (from 0);
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
 *   - minibatch sampling: stream 4, env := update index, idx := row b; index = (w0 | w1 << 32) mod upper        (the contract of mi_dqn_sample)
 */
#ifndef MI_DDQN_H
#define MI_DDQN_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h" /* mi_episode_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_DDQN_VERSION 1
#define MI_DDQN_NPARAMS 10934
#define MI_DDQN_H1 120
#define MI_DDQN_H2 84
#define MI_DDQN_W1 0
#define MI_DDQN_B1 480
#define MI_DDQN_W2 600
#define MI_DDQN_B2 10680
#define MI_DDQN_W3 10764
#define MI_DDQN_B3 10932
#define MI_DDQN_MAX_SLABS 128
#define MI_DDQN_SLAB_STRIDE 10936   /* MI_DDQN_NPARAMS + the row losses' sum + one float of padding (a multiple of 4) */
#define MI_DDQN_MAX_STEPS_PER_CALL 64

enum { MI_DDQN_OK = 0, MI_DDQN_EINVAL = -1, MI_DDQN_EHIP = -2 };

typedef struct mi_ddqn_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_ddqn_ring_t;

typedef struct mi_ddqn_act_t {
    const float* params;             /* [10,934] online network */
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
} mi_ddqn_act_t;

typedef struct mi_ddqn_batch_t {
    const float* params;         /* [10,934] online network (mi_ddqn_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [10,934] */
    int64_t* idx;                /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    float* current;              /* [batch] out: the online value of the stored action */
    float* target;               /* [batch] out */
    int32_t* next_actions;       /* [batch] out: the online network's greedy action at the successor */
    float* grads;                /* [10,934] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_ddqn_workspace_bytes(batch) */
    uint64_t sample_seed;
    uint64_t sample_update;
    int64_t sample_upper;        /* > 0: row b's index is drawn in the launch (stream 4) and stored in idx; 0: idx is given */
    int32_t batch;               /* >= 1 */
    float gamma;
    void* mid_event;             /* nullable hipEvent_t recorded on `stream` between the two launches of mi_ddqn_grad / mi_ddqn_update (timing tools) */
} mi_ddqn_batch_t;

typedef struct mi_ddqn_adam_t {
    float* exp_avg;              /* [10,934] */
    float* exp_avg_sq;           /* [10,934] */
    int64_t step;                /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_ddqn_adam_t;

int mi_ddqn_version(void);
const char* mi_ddqn_last_error(void);
const char* mi_ddqn_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: DDQN_ALLSRC) */
size_t mi_ddqn_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* q [n][2] of obs [n][4] */
int mi_ddqn_forward(const float* params, const float* obs, int n, float* q, void* stream);

/* a->n_steps (<= 64) time steps of the N envs of `handle` (a CartPole handle of libmirl's mi_env_create; N must equal ring->n_envs), ONE launch: epsilon-greedy
 * action, env.step with auto-reset and the 500-step TimeLimit, ring store; t of an episode record = the step index within the call */
int mi_ddqn_act_steps(void* handle, const mi_ddqn_ring_t* ring, const mi_ddqn_act_t* a, void* stream);

/* next_actions [batch] and target [batch] of the rows b->idx from b->params (the action) and b->target_params (its value); one launch.  Reads of `b`: params,
 * target_params, idx, next_actions, target, batch, gamma */
int mi_ddqn_target(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, void* stream);

/* loss and gradient of one batch: two launches (targets + online forward + loss + backward into per-workgroup slabs; fixed-order slab sum) */
int mi_ddqn_grad(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, void* stream);
/* the same two launches, the second of which also applies optimizer.step() to every gradient element it has just summed: bit-identical to mi_ddqn_grad followed by
 * libmirl's mi_adam */
int mi_ddqn_update(const mi_ddqn_ring_t* ring, const mi_ddqn_batch_t* b, const mi_ddqn_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
