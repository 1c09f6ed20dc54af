/* mi_c51.h — C ABI of libmirl_c51.so: C51 categorical DQN on CartPole-v1 (reference deep_rl/c51.py) for gfx950.
 *
 * A third library beside libmirl.so (include/mi_rl.h) and libmirl_pg.so (include/mi_reinforce.h).  It needs no symbol of the other two; the one thing it shares is the
 * env handle made by libmirl's mi_env_create (a host struct of device pointers, csrc/mi_common.h `struct mi_env`), which this library reads and advances.
 *
 * Conventions
 *   - every call returns MI_C51_OK (0) or a negative MI_C51_E* code; mi_c51_last_error() gives the text (thread-local).  NULL / 0 arguments are errors, never crashes.
 *   - all pointers are DEVICE pointers unless said otherwise; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: everything is enqueued on `stream`.
 *   - parameter vectors, observation arrays and the workspace must be 16-byte aligned (they are read and written as float4); anything else is MI_C51_EINVAL.
 *
 * Network (c51.py:24-37) and flat parameter layout (order of q_network.parameters(), 27,934 floats):
 *     W1 [120][4] at 0, b1 [120] at 480, W2 [84][120] at 600, b2 [84] at 10,680, W3 [202][84] at 10,764, b3 [202] at 27,732
 *     Linear(4,120) -> ReLU -> Linear(120,84) -> ReLU -> Linear(84, 2 * 101) -> Unflatten(2, 101) -> softmax(-1)
 *   Row a * 101 + j of W3 is action a, atom j.  Support z_j = -100 + 2 j (v_min = -100, v_max = 100, n_atoms = 101: compile-time constants of this library).
 *
 * Numerics contract, fp32 (tests/_c51_ref.py restates exactly this).  fmaf(a, b, c) is the fused a * b + c; nothing else is contracted.
 *   z1_u = fmaf(W1[u][3], x3, fmaf(W1[u][2], x2, fmaf(W1[u][1], x1, fmaf(W1[u][0], x0, b1[u]))));  h1_u = max(z1_u, 0)
 *   P_c[o] = chain over k = 40 c .. 40 c + 39 ascending of acc = fmaf(W2[o][k], h1_k, acc), starting from b2[o] for c = 0 and from 0 for c = 1, 2
 *   z2_o = (P_0[o] + P_1[o]) + P_2[o];  h2_o = max(z2_o, 0)
 *   logit_r = chain over k = 0 .. 83 ascending of acc = fmaf(W3[r][k], h2_k, acc), starting from b3[r]
 *   Softmax of one action's 101 logits: m = max_j logit_j;  e_j = expf(logit_j - m);  s = TREE2(e);  p_j = e_j / s;  q = TREE2(p_j * z_j)
 *     TREE2(v): lane i of a 64-lane wave forms v_i + v_{i + 64} (just v_i for i + 64 > 100; for q: fmaf(p_{i+64}, z_{i+64}, p_i * z_i)), then the balanced pairwise sum over
 *     the 64 lanes in natural order, (t0 + t1) + (t2 + t3) ... six levels.  expf / logf: the device library's (<= 1 ulp).
 *   argmax over the two actions: a = (q_1 > q_0) ? 1 : 0 (a tie goes to action 0, as torch.argmax).
 *   Projection of row b with reward r, terminated flag `term`, next_probs p = the target network's distribution of its greedy action (c51.py:132-154):
 *     tz = min(max(r + (gamma * z_j) * (1 - term), -100), 100);  b_j = (tz + 100) / 2;  l_j = floor(b_j);  u_j = ceil(b_j)
 *     wl_j = ((u_j + (l_j == u_j ? 1 : 0)) - b_j) * p_j;  wu_j = (b_j - l_j) * p_j
 *     m_k = 0; then + wl_j for every j with l_j == k in ascending j; then + wu_j for every j with u_j == k in ascending j      (index_add_ on the CPU: bit-identical)
 *   Loss and gradient of one batch of B rows, p = the online network's distribution of the STORED action (c51.py:156-158), invB = 1.0f / B:
 *     rowloss = -TREE2(m_k * logf(p_k + 1e-8f));  loss = SUMROWS(rowloss) * invB
 *     g_k = -m_k / (p_k + 1e-8f);  S = TREE2(p_k * g_k);  dlogit_k = (p_k * (g_k - S)) * invB            (not p - m: the 1e-8 is inside the log)
 *     dW3[r][k] += dlogit_j * h2_k, db3[r] += dlogit_j for r = a * 101 + j (fmaf accumulation over the rows)
 *     dh2_k = (Q_0 + Q_1) + Q_2, Q_c = chain over j = 34 c .. min(34 c + 33, 100) ascending of fmaf(dlogit_j, W3[a * 101 + j][k], acc) from 0;  dz2 = h2 > 0 ? dh2 : 0
 *     dW2[o][k] += dz2_o * h1_k, db2[o] += dz2_o
 *     dh1_k = R_0 + R_1, R_c = chain over o = 42 c .. 42 c + 41 ascending of fmaf(dz2_o, W2[o][k], acc) from 0;  dz1 = h1 > 0 ? dh1 : 0
 *     dW1[u][c] += dz1_u * x_c, db1[u] += dz1_u
 *   Summation order over the rows: workgroup g of G = min(B, MI_C51_MAX_SLABS) owns rows g, g + G, ... and accumulates them in that order into its slab; the G slabs
 *   are added in 16 groups (g mod 16), each in ascending g on four interleaved accumulators ((s0 + s1) + (s2 + s3)), the 16 group sums in ascending group.
 *   No floating-point atomics anywhere: two runs give the same bits.
 *   Adam: torch's single-tensor Adam, the element step and the host-side coefficients of libmirl's mi_adam (bit-identical to it).
 *
 * Replay ring: the layout and successor rule of mi_rl.h "DQN": observations f32 [slots][N][4], actions i64 [slots][N], rewards f32 [slots][N], terminated u8 [slots][N];
 *   slot g % slots holds obs_g and the action taken from it, slot (g + 1) % slots the resulting reward / terminated / next observation (the RESET observation after a
 *   done).  A flat index is slot * N + env; its successor is ((slot + 1) % slots) * N + env.  `terminated` excludes TimeLimit truncation.
 *
 * RNG contract (counter-based Philox4x32-10 as in mi_rl.h), libmirl's streams unchanged:
 *   - reset noise: stream 0, idx = episode[n]
 *   - exploration: stream 3, idx = the env step counter step_ctr[n]: u = (w0 >> 8) / 2^24 is compared (as a double) with epsilon, w1 & 1 is the random action.
 *     epsilon = max(slope * global_step + start_e, end_e) in double (c51.py:48,93).  There is no learning_starts clause: c51.py has none.
 *   - minibatch sampling: stream 4, env := update index, idx := row b; index = (w0 | w1 << 32) mod upper        (the contract of mi_dqn_sample)
 */
#ifndef MI_C51_H
#define MI_C51_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h" /* mi_episode_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_C51_VERSION 1
#define MI_C51_NPARAMS 27934
#define MI_C51_N_ATOMS 101
#define MI_C51_V_MIN (-100.0f)
#define MI_C51_V_MAX 100.0f
#define MI_C51_H1 120
#define MI_C51_H2 84
#define MI_C51_W1 0
#define MI_C51_B1 480
#define MI_C51_W2 600
#define MI_C51_B2 10680
#define MI_C51_W3 10764
#define MI_C51_B3 27732
#define MI_C51_MAX_SLABS 128
#define MI_C51_SLAB_STRIDE 27936   /* MI_C51_NPARAMS + the row losses' sum + one float of padding */
#define MI_C51_MAX_STEPS_PER_CALL 64

enum { MI_C51_OK = 0, MI_C51_EINVAL = -1, MI_C51_EHIP = -2 };

typedef struct mi_c51_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_c51_ring_t;

typedef struct mi_c51_batch_t {
    const float* params;         /* [27,934] online network (mi_c51_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [27,934] */
    int64_t* idx;                /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    float* target_probs;         /* [batch][101] out */
    int32_t* next_actions;       /* [batch] out: the target network's greedy action (c51.py:144) */
    float* probs;                /* [batch][101] out, nullable: the online distribution of the stored action (c51.py:156) */
    float* grads;                /* [27,934] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_c51_workspace_bytes(batch) */
    uint64_t sample_seed;
    uint64_t sample_update;
    int64_t sample_upper;        /* > 0: row b's index is drawn in the launch (stream 4) and stored in idx; 0: idx is given */
    int32_t batch;               /* >= 1 */
    float gamma;
    void* mid_event;             /* nullable hipEvent_t recorded on `stream` between the two launches of mi_c51_grad / mi_c51_update (timing tools) */
} mi_c51_batch_t;

typedef struct mi_c51_adam_t {
    float* exp_avg;              /* [27,934] */
    float* exp_avg_sq;           /* [27,934] */
    int64_t step;                /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_c51_adam_t;

int mi_c51_version(void);
const char* mi_c51_last_error(void);
const char* mi_c51_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: C51_ALLSRC) */
size_t mi_c51_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* QNetwork.get_probs (c51.py:36-37) and the action values of :99 for obs [n][4]: probs [n][2][101] and / or q [n][2] (either may be NULL, not both) */
int mi_c51_forward(const float* params, const float* obs, int n, float* probs, float* q, void* stream);

/* n_steps (<= 64) iterations of c51.py:91-116 for the N envs of `handle` (a CartPole handle of libmirl's mi_env_create; N must equal ring->n_envs), ONE launch:
 * epsilon-greedy action, env.step with auto-reset, ring store.  global_step = time steps already taken.  obs_cur [N][4] carried in / out.  forced_actions i64
 * [n_steps][N] / forced_resets f64 [n_steps][N][4] nullable (teacher forcing).  episodes [max_ep] + episode_stats i32 [4] nullable together: the call zeroes
 * episode_stats, the launch accumulates {finished episodes, sum of their lengths, longest, slots handed out in `episodes`}; t = the step index within the call. */
int mi_c51_act_steps(void* handle, const float* params, int n_steps, int64_t global_step, const mi_c51_ring_t* ring, double start_e, double end_e,
                     double exploration_fraction, int64_t total_timesteps, float* obs_cur, const int64_t* forced_actions, const double* forced_resets,
                     mi_episode_t* episodes, int32_t* episode_stats, int max_ep, void* stream);

/* next_actions [batch] and target_probs [batch][101] of the rows idx [batch] from target_params (c51.py:132-154); one launch */
int mi_c51_target(const float* target_params, const mi_c51_ring_t* ring, const int64_t* idx, int batch, float gamma, int32_t* next_actions, float* target_probs,
                  void* stream);

/* loss and gradient of one batch (c51.py:124-158): two launches (targets + forward + backward into per-workgroup slabs; fixed-order slab sum) */
int mi_c51_grad(const mi_c51_ring_t* ring, const mi_c51_batch_t* b, void* stream);
/* the same two launches, the second of which also applies optimizer.step() to every gradient element it has just summed: bit-identical to mi_c51_grad followed by
 * libmirl's mi_adam */
int mi_c51_update(const mi_c51_ring_t* ring, const mi_c51_batch_t* b, const mi_c51_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
