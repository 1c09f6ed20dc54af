/* mi_qr.h — C ABI of libmirl_qr.so: QR-DQN (quantile-regression DQN, Dabney et al. 2018) on CartPole-v1, for gfx950.
 *
 * A fifth library beside libmirl.so (include/mi_rl.h), libmirl_pg.so (include/mi_reinforce.h), libmirl_c51.so (include/mi_c51.h) and libmirl_iqn.so
 * (include/mi_iqn.h).  It needs no symbol of the other four; the one thing it shares is the env handle made by libmirl's mi_env_create (a host struct of device
 * pointers, csrc/mi_common.h `struct mi_env`), which this library reads and advances.
 *
 * The reference has no qrdqn.py.  The algorithm is c51.py's loop with the head and the loss replaced; the yardstick is the same algorithm written as a plain torch
 * script (tools/capture_qrdqn_ref.py: autograd, optim.Adam, CPU), whose run the fixtures under tests/golden/qrdqn_* hold.
 *
 * Conventions
 *   - every call returns MI_QR_OK (0) or a negative MI_QR_E* code; mi_qr_last_error() gives the text (thread-local).  NULL / 0 arguments are errors, never crashes.
 *   - all pointers are DEVICE pointers unless said otherwise; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: everything is enqueued on `stream`.
 *   - parameter vectors, observation arrays and the workspace must be 16-byte aligned (they are read and written as float4); anything else is MI_QR_EINVAL.
 *
 * Network and flat parameter layout (order of parameters(), 21,644 floats):
 *     W1 [120][4] at 0, b1 [120] at 480, W2 [84][120] at 600, b2 [84] at 10,680, W3 [128][84] at 10,764, b3 [128] at 21,516
 *     Linear(4,120) -> ReLU -> Linear(120,84) -> ReLU -> Linear(84, 2 * 64) -> Unflatten(2, 64)
 *   Row a * 64 + i of W3 is action a, quantile i.  Fractions tau_i = (2 i + 1) / 128 (exact in f32); kappa = 1.  Compile-time constants of this library.
 *
 * Numerics contract, fp32 (tests/_qrdqn_ref.py restates exactly this).  fmaf(a, b, c) is the fused a * b + c; nothing else is contracted.  "chain over k of
 * (w_k, v_k) from s" means acc = s; for ascending k: acc = fmaf(w_k, v_k, acc).
 *   Torso (the expressions of mi_c51.h):
 *     z1_u = fmaf(W1[u][3], x3, fmaf(W1[u][2], x2, fmaf(W1[u][1], x1, fmaf(W1[u][0], x0, b1[u]))));  h1_u = max(z1_u, 0)
 *     P_c[o] = chain over k = 40 c .. 40 c + 39 of (W2[o][k], h1_k) from b2[o] for c = 0 and from 0 for c = 1, 2
 *     z2_o = (P_0[o] + P_1[o]) + P_2[o];  h2_o = max(z2_o, 0)
 *   Quantiles: theta_{a,i} = chain over k < 84 of (W3[a * 64 + i][k], h2_k) from b3[a * 64 + i]
 *   Action values through the COLLAPSED head (the mean of a linear head is a linear head).  Each launch forms, once, from the parameters it is given:
 *     wbar_a[k] = s * (1.0f / 64), s = 0; for ascending i < 64: s = s + W3[a * 64 + i][k]          (the scaling is exact)
 *     bbar_a    = s * (1.0f / 64), s = 0; for ascending i < 64: s = s + b3[a * 64 + i]
 *     q_a = chain over k < 84 of (wbar_a[k], h2_k) from bbar_a;  a* = (q_1 > q_0) ? 1 : 0 (a tie goes to action 0, as torch.argmax)
 *   The acting launch never evaluates the 128-row head; the update evaluates 64 rows per network and batch row (the greedy action's, the stored action's).
 *   Targets of row b: next_actions[b] = a* of the TARGET network at the successor observation; target_j = r + lg * theta'_{a*,j}, lg = terminated ? 0 : gamma
 *     (a product and a sum, not fused).
 *   Loss and gradient of current_i = theta_{a,i} (a the stored action, online network), inv = 1.0f / (float)(B * 64):
 *     u_ij = target_j - current_i;  au = |u_ij|;  L_ij = au <= 1 ? (0.5f * u_ij) * u_ij : au - 0.5f;  c_ij = min(max(u_ij, -1), 1)
 *     w_ij = |tau_i - (u_ij < 0 ? 1 : 0)|
 *     for c < 4: T_c = sum over j = 16 c .. 16 c + 15 ascending of w_ij * L_ij, S_c likewise of w_ij * c_ij (products rounded, then added: acc = acc + term from 0)
 *     L_i = ((T_0 + T_1) + T_2) + T_3;  G_i = ((S_0 + S_1) + S_2) + S_3;  dcurrent_i = -(G_i * inv);  rowloss_b = sum over ascending i of L_i from 0
 *     loss = SUMROWS(rowloss) * inv.  mi_qr_quantile_huber: SUMROWS adds the rows in ascending b from 0; mi_qr_grad / mi_qr_update: in the slab order below.
 *     This is the continuous Huber (0.5 u^2 inside kappa): neither the loss nor its gradient jumps at |u| = 1 or at u = 0 (w is discontinuous at 0, where L = c = 0).
 *   Backward of row b, d_i = dcurrent_i (the other action's rows have no gradient):
 *     dW3[a * 64 + i][k] += d_i * h2_k, db3[a * 64 + i] += d_i (fmaf accumulation over the rows the workgroup owns)
 *     dh2_k = (Q_0 + Q_1) + Q_2, Q_c = chain over i = 22 c .. min(22 c + 21, 63) of (d_i, W3[a * 64 + i][k]) from 0;  dz2 = h2 > 0 ? dh2 : 0
 *     dW2[o][k] += dz2_o * h1_k, db2[o] += dz2_o
 *     dh1_k = R_0 + R_1, R_c = chain over o = 42 c .. 42 c + 41 of (dz2_o, W2[o][k]) from 0;  dz1 = h1 > 0 ? dh1 : 0
 *     dW1[u][c] += dz1_u * x_c, db1[u] += dz1_u
 *   Summation order over the rows: workgroup g of G = min(B, MI_QR_MAX_SLABS) owns rows g, g + G, ... and accumulates them in that order into its slab (from 0);
 *   the G slabs are added in 16 groups (g mod 16), each in ascending g on four interleaved accumulators ((s0 + s1) + (s2 + s3)), the 16 group sums in ascending
 *   group.  No floating-point atomics anywhere: two runs give the same bits.
 *   Adam: torch's single-tensor Adam, the element step and the host-side coefficients of libmirl's mi_adam (bit-identical to it).
 *
 * Replay ring: the layout and successor rule of mi_c51_ring_t: observations f32 [slots][N][4], actions i64 [slots][N], rewards f32 [slots][N], terminated u8
 *   [slots][N]; slot g % slots holds obs_g and the action taken from it, slot (g + 1) % slots the resulting reward / terminated / next observation (the RESET
 *   observation after a done).  A flat index is slot * N + env; its successor is ((slot + 1) % slots) * N + env.  `terminated` excludes TimeLimit truncation.
 *
 * RNG contract (counter-based Philox4x32-10 as in mi_rl.h), libmirl's streams unchanged, no new stream:
 *   - reset noise: stream 0, idx = episode[n]
 *   - exploration: stream 3, idx = the env step counter step_ctr[n]: u = (w0 >> 8) / 2^24 is compared (as a double) with epsilon, w1 & 1 is the random action.
 *     epsilon = max(slope * global_step + start_e, end_e) in double, slope = (end_e - start_e) / (exploration_fraction * total_timesteps).  No learning_starts clause.
 *   - minibatch sampling: stream 4, env := update index, idx := row b; index = (w0 | w1 << 32) mod upper        (the contract of mi_dqn_sample)
 */
#ifndef MI_QR_H
#define MI_QR_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h" /* mi_episode_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_QR_VERSION 1
#define MI_QR_NPARAMS 21644
#define MI_QR_N_QUANT 64
#define MI_QR_H1 120
#define MI_QR_H2 84
#define MI_QR_W1 0
#define MI_QR_B1 480
#define MI_QR_W2 600
#define MI_QR_B2 10680
#define MI_QR_W3 10764
#define MI_QR_B3 21516
#define MI_QR_MAX_SLABS 128
#define MI_QR_SLAB_STRIDE 21648   /* MI_QR_NPARAMS + the row losses' sum + three floats of padding (a multiple of 4) */
#define MI_QR_MAX_STEPS_PER_CALL 64

enum { MI_QR_OK = 0, MI_QR_EINVAL = -1, MI_QR_EHIP = -2 };

typedef struct mi_qr_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_qr_ring_t;

typedef struct mi_qr_act_t {
    const float* params;             /* [21,644] online network */
    float* obs_cur;                  /* [N][4] carried in / out */
    const int64_t* forced_actions;   /* [n_steps][N] nullable */
    const double* forced_resets;     /* [n_steps][N][4] nullable */
    mi_episode_t* episodes;          /* [max_ep], nullable together with max_ep == 0 */
    int32_t* episode_stats;          /* [4] nullable: the call zeroes it, the launch accumulates {finished episodes, sum of lengths, longest, slots handed out} */
    int64_t global_step;             /* time steps already taken */
    int64_t total_timesteps;
    double start_e;                  /* epsilon = max(slope * global_step + start_e, end_e) */
    double end_e;
    double exploration_fraction;
    int32_t n_steps;                 /* 1 .. 64 */
    int32_t max_ep;
} mi_qr_act_t;

typedef struct mi_qr_batch_t {
    const float* params;         /* [21,644] online network (mi_qr_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [21,644] */
    int64_t* idx;                /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    float* current;              /* [batch][64] out, nullable: the online quantiles of the stored action */
    float* target;               /* [batch][64] out */
    int32_t* next_actions;       /* [batch] out: the target network's greedy action */
    float* grads;                /* [21,644] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_qr_workspace_bytes(batch) */
    uint64_t sample_seed;
    uint64_t sample_update;
    int64_t sample_upper;        /* > 0: row b's index is drawn in the launch (stream 4) and stored in idx; 0: idx is given */
    int32_t batch;               /* >= 1 */
    float gamma;
    void* mid_event;             /* nullable hipEvent_t recorded on `stream` between the two launches of mi_qr_grad / mi_qr_update (timing tools) */
} mi_qr_batch_t;

typedef struct mi_qr_adam_t {
    float* exp_avg;              /* [21,644] */
    float* exp_avg_sq;           /* [21,644] */
    int64_t step;                /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_qr_adam_t;

int mi_qr_version(void);
const char* mi_qr_last_error(void);
const char* mi_qr_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: QR_ALLSRC) */
size_t mi_qr_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* quantiles [n][2][64] and / or q [n][2] (either may be NULL, not both) of obs [n][4]; q comes through the collapsed head */
int mi_qr_forward(const float* params, const float* obs, int n, float* quantiles, float* q, void* stream);

/* a->n_steps (<= 64) time steps of the N envs of `handle` (a CartPole handle of libmirl's mi_env_create; N must equal ring->n_envs), ONE launch: epsilon-greedy
 * action, env.step with auto-reset and the 500-step TimeLimit, ring store; t of an episode record = the step index within the call */
int mi_qr_act_steps(void* handle, const mi_qr_ring_t* ring, const mi_qr_act_t* a, void* stream);

/* next_actions [batch] and target [batch][64] of the rows b->idx from b->target_params; one launch.  Reads of `b`: target_params, idx, next_actions, target,
 * batch, gamma */
int mi_qr_target(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, void* stream);

/* the loss stage alone: current [batch][64], target [batch][64] -> loss [1] and dcurrent [batch][64]; one launch */
int mi_qr_quantile_huber(const float* current, const float* target, int batch, float* loss, float* dcurrent, void* stream);

/* loss and gradient of one batch: two launches (targets + online forward + loss + backward into per-workgroup slabs; fixed-order slab sum) */
int mi_qr_grad(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, void* stream);
/* the same two launches, the second of which also applies optimizer.step() to every gradient element it has just summed: bit-identical to mi_qr_grad followed by
 * libmirl's mi_adam */
int mi_qr_update(const mi_qr_ring_t* ring, const mi_qr_batch_t* b, const mi_qr_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
