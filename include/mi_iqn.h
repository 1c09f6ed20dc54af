/* mi_iqn.h — C ABI of libmirl_iqn.so: IQN (implicit quantile network, reference deep_rl/iqn.py) re-targeted to CartPole-v1, for gfx950.
 *
 * A fourth library beside libmirl.so (include/mi_rl.h), libmirl_pg.so (include/mi_reinforce.h) and libmirl_c51.so (include/mi_c51.h).  It needs no symbol of the
 * other three; the one thing it shares is the env handle made by libmirl's mi_env_create (csrc/mi_common.h `struct mi_env`), which this library reads and advances.
 *
 * Conventions
 *   - every call returns MI_IQN_OK (0) or a negative MI_IQN_E* code; mi_iqn_last_error() gives the text (thread-local).  NULL / 0 arguments are errors, never crashes.
 *   - all pointers are DEVICE pointers unless said otherwise; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: everything is enqueued on `stream`.
 *   - parameter vectors, observation arrays and the workspace must be 16-byte aligned (they are read and written as float4); anything else is MI_IQN_EINVAL.
 *
 * Networks (iqn.py:32-113 with the Atari FeaturesExtractor re-targeted: each Conv2d(c_in, c_out, k, s) is Linear(c_in, c_out), spatial extent 1 x 1) and the flat
 * parameter layout, the order of the optimizer's parameter list (iqn.py:170), 44,898 floats:
 *     F.W1 [32][4] at 0, F.b1 [32] at 128, F.W2 [64][32] at 160, F.b2 [64] at 2,208, F.W3 [64][64] at 2,272, F.b3 [64] at 6,368          FeaturesExtractor
 *     C.W [64][64] at 6,432, C.b [64] at 10,528                                                                                       CosineEmbeddingNetwork(64, 64)
 *     Q.W1 [512][64] at 10,592, Q.b1 [512] at 43,360, Q.W2 [2][512] at 43,872, Q.b2 [2] at 44,896                                     QuantileNetwork(2, 64)
 *
 * Numerics contract, fp32 (tests/_iqn_ref.py restates exactly this).  fmaf(a, b, c) is the fused a * b + c; nothing else is contracted.  "chain over k of (w_k, v_k)
 * from s" means acc = s; for ascending k: acc = fmaf(w_k, v_k, acc) — what v_mfma_f32_16x16x4_f32 computes bit for bit when s is its C operand.
 *   Features of an observation x [4]:
 *     h1_u = max(chain over k < 4 of (F.W1[u][k], x_k) from F.b1[u], 0);  h2_o = max(chain over k < 32 of (F.W2[o][k], h1_k) from F.b2[o], 0)
 *     emb_e = max(chain over k < 64 of (F.W3[e][k], h2_k) from F.b3[e], 0)
 *   Tau embedding of one tau:
 *     arg_k = tau * MI_IQN_I_PI[k] (one f32 multiply; the table holds the f32 values of iqn.py:71, pi_f32 * k rounded once);  c_k = cosf(arg_k), the device library's
 *     te_e = max(chain over k < 64 of (C.W[e][k], c_k) from C.b[e], 0)
 *   Quantiles of (x, tau): prod_e = emb_e * te_e (the Hadamard product, before the head);  z_u = chain over e < 64 of (Q.W1[u][e], prod_e) from Q.b1[u];  h_u = max(z_u, 0)
 *     The 512 hidden units are split over four partial chains by S_c = { u : (u >> 3) & 3 == c } (blocks of 8 units, dealt round-robin):
 *     P_c[a] = chain over u in S_c ascending of (Q.W2[a][u], h_u) from (c == 0 ? Q.b2[a] : 0);  quantile_a = ((P_0[a] + P_1[a]) + P_2[a]) + P_3[a]
 *   Action values over K taus: s = 0; for ascending i < K: s = s + quantile_a(i);  q_a = s / (float)K.  argmax: a = (q_1 > q_0) ? 1 : 0 (a tie goes to action 0).
 *   Targets of row b (iqn.py:252-278): next_actions[b] = argmax of q over the 32 next_taus with the TARGET networks at the successor observation;
 *     target_j = r + lg * nq_j, nq_j the target networks' quantile of that action at tau_dashes[j], lg = terminated ? 0 : gamma (a product and a sum, not fused).
 *   Loss and gradient of current (iqn.py:281-289), kappa = 1, inv = 1.0f / (float)(B * 64):
 *     d_ij = target_j - current_i;  ad = |d_ij|;  huber_ij = ad <= 1 ? d_ij * d_ij : ad - 0.5f     (d * d, not d * d / 2: the value jumps at kappa, as the reference's)
 *     w_ij = |tau_i - (d_ij < 0 ? 1 : 0)|;  g_ij = ad <= 1 ? 2 * d_ij : (d_ij > 0 ? 1 : -1)
 *     for c < 4: T_c = sum over j = 16 c .. 16 c + 15 ascending of w_ij * huber_ij, S_c likewise of w_ij * g_ij (products rounded, then added: acc = acc + term from 0)
 *     L_i = ((T_0 + T_1) + T_2) + T_3;  G_i = ((S_0 + S_1) + S_2) + S_3;  dcurrent_i = -(G_i * inv);  rowloss_b = sum over ascending i of L_i from 0
 *     loss = SUMROWS(rowloss) * inv.  mi_iqn_quantile_huber: SUMROWS adds the rows in ascending b; mi_iqn_grad / mi_iqn_update: in the slab order below.
 *   Backward of row b with stored action a, dout_i = dcurrent_i (the other action's output has no gradient):
 *     dQ.b2[a] = sum over ascending i of dout_i;  dQ.W2[a][u] = chain over i of (dout_i, h_u(i)) from 0
 *     dz_u(i) = z_u(i) > 0 ? dout_i * Q.W2[a][u] : 0;  dQ.b1[u] = sum over ascending i of dz_u(i);  dQ.W1[u][e] = chain over i of (dz_u(i), prod_e(i)) from 0
 *     dprod_e(i) = ((R_0 + R_1) + R_2) + R_3, R_c = chain over u in S_c ascending of (dz_u(i), Q.W1[u][e]) from 0
 *     dte_e(i) = te_e(i) > 0 ? dprod_e(i) * emb_e : 0;  dC.b[e] = sum over ascending i of dte_e(i);  dC.W[e][k] = chain over i of (dte_e(i), c_k(i)) from 0
 *     demb_e = chain over i of (dprod_e(i), te_e(i)) from 0;  dz3_e = emb_e > 0 ? demb_e : 0;  dF.b3 = dz3;  dF.W3[e][k] = dz3_e * h2_k
 *     dz2_k = h2_k > 0 ? (chain over e of (dz3_e, F.W3[e][k]) from 0) : 0;  dF.b2 = dz2;  dF.W2[o][k] = dz2_o * h1_k
 *     dz1_k = h1_k > 0 ? (chain over o of (dz2_o, F.W2[o][k]) from 0) : 0;  dF.b1 = dz1;  dF.W1[u][k] = dz1_u * x_k
 *   Summation over the rows: workgroup g of G = min(B, MI_IQN_MAX_SLABS) owns rows g, g + G, ... and adds each row's gradient (as formed above) to its slab in that
 *   order (slab = slab + row, from 0); the G slabs are added in 16 groups (g mod 16), each in ascending g on four interleaved accumulators ((s0 + s1) + (s2 + s3)),
 *   the 16 group sums in ascending group.  No floating-point atomics anywhere: two runs give the same bits.
 *   Adam: torch's single-tensor Adam, the element step and the host-side coefficients of libmirl's mi_adam (bit-identical to it).
 *
 * Replay ring: the layout and successor rule of mi_c51_ring_t (observations f32 [slots][N][4], no uint8 storage and no / 255).  upper = min(global_step, slots) * N.
 *
 * RNG contract (counter-based Philox4x32-10 keyed as in mi_rl.h), libmirl's streams 0 - 8 unchanged:
 *   - reset noise: stream 0, idx = episode[n]
 *   - exploration: stream 3, idx = step_ctr[n]: u = (w0 >> 8) / 2^24 compared (as a double) with epsilon, w1 & 1 the random action.  The step explores when
 *     global_step < learning_starts or u < epsilon, epsilon = max(1 + slope * global_step, final_epsilon) in double (iqn.py:187-189)
 *   - minibatch index: stream 4, env := update index, idx := row b; index = (w0 | w1 << 32) mod upper
 *   - acting taus: stream 9, env n, idx = step_ctr[n] * 8 + m: word w of that block is tau 4 m + w of the step's 32
 *   - online taus / next_taus / tau_dashes: streams 10 / 11 / 12, env := update index, idx := b * 16 + m: word w is tau 4 m + w of row b (next_taus use m < 8)
 *   Each tau is (word >> 8) / 2^24, torch.rand's f32 grid.  Every tau input can be forced through a nullable pointer (teacher forcing).
 */
#ifndef MI_IQN_H
#define MI_IQN_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h" /* mi_episode_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_IQN_VERSION 1
#define MI_IQN_NPARAMS 44898
#define MI_IQN_EMB 64            /* embedding_dim */
#define MI_IQN_NCOS 64           /* num_cosines */
#define MI_IQN_HID 512
#define MI_IQN_N_TAU 64          /* num_tau_samples */
#define MI_IQN_N_TAU_PRIME 64    /* num_tau_prime_samples */
#define MI_IQN_N_QUANT 32        /* num_quantile_samples (acting, greedy next action) */
#define MI_IQN_FW1 0
#define MI_IQN_FB1 128
#define MI_IQN_FW2 160
#define MI_IQN_FB2 2208
#define MI_IQN_FW3 2272
#define MI_IQN_FB3 6368
#define MI_IQN_CW 6432
#define MI_IQN_CB 10528
#define MI_IQN_QW1 10592
#define MI_IQN_QB1 43360
#define MI_IQN_QW2 43872
#define MI_IQN_QB2 44896
#define MI_IQN_MAX_SLABS 64
#define MI_IQN_SLAB_STRIDE 44900 /* MI_IQN_NPARAMS + the row losses' sum + one float of padding */
#define MI_IQN_MAX_STEPS_PER_CALL 64

/* bit patterns of the 64 f32 multipliers i_pi of iqn.py:71 (np.pi * torch.arange(1, 65)), as captured from the reference (tests/golden/iqn_ref_trace.npz "i_pi") */
#define MI_IQN_I_PI_BITS \
    0x40490fdbu, 0x40c90fdbu, 0x4116cbe4u, 0x41490fdbu, 0x417b53d2u, 0x4196cbe4u, 0x41afede0u, 0x41c90fdbu, 0x41e231d6u, 0x41fb53d2u, 0x420a3ae7u, 0x4216cbe4u, \
    0x42235ce2u, 0x422fede0u, 0x423c7eddu, 0x42490fdbu, 0x4255a0d9u, 0x426231d6u, 0x426ec2d4u, 0x427b53d2u, 0x4283f268u, 0x428a3ae7u, 0x42908365u, 0x4296cbe4u, \
    0x429d1463u, 0x42a35ce2u, 0x42a9a561u, 0x42afede0u, 0x42b6365eu, 0x42bc7eddu, 0x42c2c75cu, 0x42c90fdbu, 0x42cf585au, 0x42d5a0d9u, 0x42dbe958u, 0x42e231d6u, \
    0x42e87a55u, 0x42eec2d4u, 0x42f50b53u, 0x42fb53d2u, 0x4300ce28u, 0x4303f268u, 0x430716a7u, 0x430a3ae7u, 0x430d5f26u, 0x43108365u, 0x4313a7a5u, 0x4316cbe4u, \
    0x4319f024u, 0x431d1463u, 0x432038a3u, 0x43235ce2u, 0x43268121u, 0x4329a561u, 0x432cc9a0u, 0x432fede0u, 0x4333121fu, 0x4336365eu, 0x43395a9eu, 0x433c7eddu, \
    0x433fa31du, 0x4342c75cu, 0x4345eb9cu, 0x43490fdbu

enum { MI_IQN_OK = 0, MI_IQN_EINVAL = -1, MI_IQN_EHIP = -2 };

typedef struct mi_iqn_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_iqn_ring_t;

typedef struct mi_iqn_act_t {
    const float* params;             /* [44,898] online networks */
    float* obs_cur;                  /* [N][4] carried in / out */
    const int64_t* forced_actions;   /* [n_steps][N] nullable */
    const double* forced_resets;     /* [n_steps][N][4] nullable */
    const float* forced_taus;        /* [n_steps][N][32] nullable */
    float* taus_out;                 /* [n_steps][N][32] nullable out: the taus of every greedy step (exploring and forced-action steps leave their rows untouched) */
    mi_episode_t* episodes;          /* [max_ep], nullable together with max_ep == 0 */
    int32_t* episode_stats;          /* [4] nullable: the call zeroes it, the launch accumulates {finished episodes, sum of lengths, longest, slots handed out} */
    int64_t global_step;             /* time steps already taken */
    int64_t learning_starts;
    double slope, final_epsilon;
    int32_t n_steps;                 /* 1 .. 64 */
    int32_t max_ep;
} mi_iqn_act_t;

typedef struct mi_iqn_batch_t {
    const float* params;             /* [44,898] online networks (mi_iqn_update writes it: the caller owns it mutable) */
    const float* target_params;      /* [44,898] */
    int64_t* idx;                    /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    const float* forced_taus;        /* [batch][64] nullable */
    const float* forced_next_taus;   /* [batch][32] nullable */
    const float* forced_tau_dashes;  /* [batch][64] nullable */
    float* taus;                     /* [batch][64] out: the online taus used */
    float* current;                  /* [batch][64] out: current_action_quantiles (iqn.py:249) */
    float* target;                   /* [batch][64] out: target_action_quantiles (:276) */
    int32_t* next_actions;           /* [batch] out (:261) */
    float* grads;                    /* [44,898] out */
    float* loss;                     /* [1] out */
    void* workspace;                 /* mi_iqn_workspace_bytes(batch) */
    uint64_t seed;
    uint64_t update;                 /* the update index keying streams 4, 10, 11, 12 */
    int64_t sample_upper;            /* > 0: row b's index is drawn in the launch (stream 4) and stored in idx; 0: idx is given */
    int32_t batch;                   /* >= 1 */
    float gamma;
    void* mid_event;                 /* nullable hipEvent_t recorded between the two launches of mi_iqn_grad / mi_iqn_update (timing tools) */
} mi_iqn_batch_t;

typedef struct mi_iqn_adam_t {
    float* exp_avg;              /* [44,898] */
    float* exp_avg_sq;           /* [44,898] */
    int64_t step;                /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_iqn_adam_t;

int mi_iqn_version(void);
const char* mi_iqn_last_error(void);
const char* mi_iqn_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: IQN_ALLSRC) */
size_t mi_iqn_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* quantiles [n][k][2] and / or q [n][2] (either may be NULL, not both) of obs [n][4] at taus [n][k], 1 <= k <= 64 (iqn.py:196-200) */
int mi_iqn_forward(const float* params, const float* obs, const float* taus, int n, int k, float* quantiles, float* q, void* stream);

/* a->n_steps iterations of iqn.py:185-217 for the N envs of `handle` (a CartPole handle of libmirl's mi_env_create; N must equal ring->n_envs), ONE launch */
int mi_iqn_act_steps(void* handle, const mi_iqn_ring_t* ring, const mi_iqn_act_t* a, void* stream);

/* next_actions and target of the rows b->idx from b->target_params (iqn.py:252-278); one launch.  Reads of `b`: target_params, idx, forced_next_taus,
 * forced_tau_dashes, next_actions, target, seed, update, batch, gamma */
int mi_iqn_target(const mi_iqn_ring_t* ring, const mi_iqn_batch_t* b, void* stream);

/* the loss stage alone: current [batch][64], target [batch][64], taus [batch][64] -> loss [1] and dcurrent [batch][64]; one launch */
int mi_iqn_quantile_huber(const float* current, const float* target, const float* taus, int batch, float* loss, float* dcurrent, void* stream);

/* loss and gradient of one batch (iqn.py:225-292): two launches (targets + forward + backward into per-workgroup slabs; fixed-order slab sum) */
int mi_iqn_grad(const mi_iqn_ring_t* ring, const mi_iqn_batch_t* b, void* stream);
/* the same two launches, the second of which also applies optimizer.step() to every gradient element it has just summed: bit-identical to mi_iqn_grad followed by
 * libmirl's mi_adam */
int mi_iqn_update(const mi_iqn_ring_t* ring, const mi_iqn_batch_t* b, const mi_iqn_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
