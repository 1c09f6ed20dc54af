/* mi_rainbow.h — C ABI of libmirl_rainbow.so: Rainbow (Hessel et al. 2018) on CartPole-v1 for gfx950 — a distributional (C51), noisy, n-step, dueling,
 * Double DQN whose row loss is the replay priority.
 *
 * A tenth library beside libmirl.so (include/mi_rl.h), libmirl_pg.so, libmirl_c51.so (include/mi_c51.h), libmirl_iqn.so, libmirl_qr.so, libmirl_ddqn.so,
 * libmirl_pdd.so (include/mi_pdd.h), libmirl_nstep.so (include/mi_nstep.h) and libmirl_noisy.so (include/mi_noisy.h).  It needs no symbol of the other nine.  The
 * prioritized sampler stays libmirl's mi_per_*.  The conventions (return codes, device pointers, 16-byte alignment, nothing synchronises), the ring layout, the
 * streams 0, 3 and 4, the walk (csrc/mi_nwalk.h), the torso (csrc/mi_torso.h), the slab summation order and Adam are those headers'.
 *
 * Network, MI_RB_NPARAMS = 36,774 floats.  The torso 4 -> 120 -> 84 is plain, at 0 .. 10,763 (W1 [120][4], b1 [120], W2 [84][120], b2 [84]).  Behind it two NOISY
 * streams produce MI_RB_N_ATOMS = 51 atoms each (a compile-time constant, Rainbow's own number):
 *     the means mu at MI_RB_WV = 10,764 in the order Wv[51][84] bv[51] Wa[2][51][84] ba[2][51]: 13,005 floats (MI_RB_NHEAD)
 *     the sigmas at MI_RB_SIGMA = 23,769 in the same order
 *   Head ROW r < 153: r < 51 is value atom j = r; r = 51 + a * 51 + j is advantage atom j of action a.  The slab stride is MI_RB_SLAB_STRIDE = 36,776.
 *   The support is a run-time pair v_min < v_max (both finite; anything else is MI_RB_EINVAL) in the act, batch and forward arguments:
 *     dz = (v_max - v_min) / 50;   z_j = v_min + dz * j            (a product, then a sum; nothing is contracted that is not written fmaf)
 *
 * Numerics contract, fp32 (tests/_rainbow_ref.py restates it).  Torso: mi_c51.h's z1, h1, P_c, z2, h2.
 *   y_r = chain over k = 0 .. 83 ascending of acc = fmaf(theta[r][k], h2_k, acc), starting from the row's effective bias
 *   v_j = y_j, A[a][j] = y_{51 + a * 51 + j};   l[a][j] = v_j + (A[a][j] - 0.5f * (A[0][j] + A[1][j]))
 *   Softmax of one action's 51 logits by one 64-lane wave, lane j holding atom j: m = max_j l_j;  e_j = expf(l_j - m);  s = TREE(e);  p_j = e_j / s;
 *     q = TREE(p_j * z_j).  TREE(v): lanes 51 .. 63 hold 0; the balanced pairwise sum over the 64 lanes in natural order, (t0 + t1) + (t2 + t3) ..., six levels.
 *   argmax: a = (q_1 > q_0) ? 1 : 0, as mi_pdd.h.
 *
 * Noise: mi_noisy.h's contract, widened.  One SAMPLE keyed (seed, a, b, stream) is MI_RB_NXI = 321 numbers xi_c = sgn(z_c) * sqrtf(|z_c|) with mi_noisy.h's
 *   expression for z; the Philox counter is b * 512 + c:  mi_philox(seed, a, b * 512 + c, stream, r).
 *   c: 0 .. 83 the value stream's inputs, 84 .. 134 its outputs (atom j at 84 + j), 135 .. 218 the advantage stream's inputs, 219 .. 320 its outputs (219 + a * 51 + j).
 *   eps of a weight = output factor * input factor (ONE product, in this order), of a bias = the output factor.
 *   theta = mu + sigma * eps: a product, then a sum.
 *   Streams: 13 (acting: (a, b) = (env_id, step counter) with the env handle's seed, a fresh head per env and greedy step) and 14 (learning: update u = sample_update
 *   with seed = sample_seed draws (u, 0) for the ONLINE and (u, 1) for the TARGET network; one online sample serves obs[i] and obs[s_m]) keep mi_noisy.h's meaning and
 *   keying.  A different library's networks never share a launch with libmirl_noisy.so's, so reusing the two tags is safe; the tag has 4 bits and ONLY TAG 15 IS FREE.
 *   `noisy` == 0: eps == 0, no draw is made, and the sigma gradient is exact +0.
 *
 * Target of batch row i:  (s_m, R, lg, m) = nw_walk(ring, i, total, n_step, head_slot, gamma) as mi_nstep.h;  a* = the ONLINE network's argmax at obs[s_m] under the
 *   online sample;  p' = the TARGET network's distribution of a* at obs[s_m] under the target sample.  Projection (mi_c51.h's with R for r and lg * z_j for
 *   (gamma * z_j) * (1 - term)):
 *     tz = min(max(R + lg * z_j, v_min), v_max);  b_j = (tz - v_min) / dz;  l_j = floor(b_j);  u_j = ceil(b_j)
 *     wl_j = ((u_j + (l_j == u_j ? 1 : 0)) - b_j) * p'_j;  wu_j = (b_j - l_j) * p'_j
 *     m_k = 0; then + wl_j for every j with l_j == k in ascending j; then + wu_j for every j with u_j == k in ascending j
 *   horizon[b] = m, next_actions[b] = a*, target_probs[b][k] = m_k.
 * Loss and gradient, p = the online distribution of the STORED action at obs[i] under the online sample, invB = 1.0f / B, w_b = weights[b] (1 when weights is NULL):
 *     rowloss_b = -TREE(m_k * logf(p_k + 1e-8f));  loss = SUMROWS(w_b * rowloss_b) * invB;  prio[b] = max(rowloss_b, 0), UNWEIGHTED
 *     (Rainbow's priority: the row's cross-entropy against the projected target, not the KL divergence; it takes td_abs's place in mi_per_update_priorities_sums)
 *     g_k = -m_k / (p_k + 1e-8f);  S = TREE(p_k * g_k);  dl_k = (p_k * (g_k - S)) * (w_b * invB)
 *     dueling backward: dv_j = dl_j;  e_j = 0.5f * dl_j;  dA[a][j] = e_j;  dA[1 - a][j] = -e_j            (d_r: the one of these that belongs to head row r)
 *     g[r][k] += d_r * h2_k (fmaf over the rows), gb[r] += d_r
 *     dh2_k = (Q_0 + Q_1) + Q_2, Q_c = chain over j = 0 .. 50 ascending of fmaf(d_{51 c + j}, theta[51 c + j][k], acc) from 0;  dz2 = h2 > 0 ? dh2 : 0
 *     then mi_c51.h's dW2, db2, dh1, dW1, db1 (csrc/mi_torso.h: ts_backward)
 *     grads[mu_t] = g_t;  grads[sigma_t] = g_t * eps_t: one product per slab at the slab store (noisy == 0: +0)
 *   Rows: workgroup g of G = min(B, MI_RB_MAX_SLABS) owns rows g, g + G, ... in that order; the slabs are summed as mi_c51.h states.  No floating-point atomics: two
 *   runs give the same bits.
 */
#ifndef MI_RAINBOW_H
#define MI_RAINBOW_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h" /* mi_episode_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_RB_VERSION 1
#define MI_RB_N_ATOMS 51
#define MI_RB_NPARAMS 36774
#define MI_RB_H1 120
#define MI_RB_H2 84
#define MI_RB_W1 0
#define MI_RB_B1 480
#define MI_RB_W2 600
#define MI_RB_B2 10680
#define MI_RB_WV 10764
#define MI_RB_BV 15048
#define MI_RB_WA 15099
#define MI_RB_BA 23667
#define MI_RB_SIGMA 23769         /* sigma of head element t at MI_RB_SIGMA + t, t < MI_RB_NHEAD */
#define MI_RB_NHEAD 13005
#define MI_RB_NROWS 153
#define MI_RB_NXI 321
#define MI_RB_MAX_SLABS 128
#define MI_RB_SLAB_STRIDE 36776   /* MI_RB_NPARAMS + the row losses' sum, rounded up to a multiple of 4 */
#define MI_RB_MAX_N 16
#define MI_RB_MAX_STEPS_PER_CALL 64
#define MI_RB_STREAM_ACT 13
#define MI_RB_STREAM_LEARN 14

enum { MI_RB_OK = 0, MI_RB_EINVAL = -1, MI_RB_EHIP = -2 };

/* layout-identical to mi_pdd_ring_t */
typedef struct mi_rb_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_rb_ring_t;

/* mi_nz_act_t with the support in the place of `reserved` and behind it */
typedef struct mi_rb_act_t {
    const float* params;             /* [36,774] online network */
    float* obs_cur;                  /* [N][4] carried in / out */
    const int64_t* forced_actions;   /* [n_steps][N] nullable */
    const double* forced_resets;     /* [n_steps][N][4] nullable */
    mi_episode_t* episodes;          /* [max_ep], nullable together with max_ep == 0 */
    int32_t* episode_stats;          /* [4] nullable */
    int64_t global_step;
    int64_t total_timesteps;
    int64_t learning_starts;
    double start_e;                  /* epsilon = max(slope * global_step + start_e, end_e); 0 and 0: every step past learning_starts is greedy */
    double end_e;
    double exploration_fraction;
    int32_t n_steps;                 /* 1 .. 64 */
    int32_t max_ep;
    int32_t noisy;                   /* 0: the mean network acts; else every greedy step draws its own head */
    float v_min;
    float v_max;
    int32_t reserved;
} mi_rb_act_t;

typedef struct mi_rb_batch_t {
    const float* params;         /* [36,774] online network (mi_rb_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [36,774] */
    int64_t* idx;                /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    float* target_probs;         /* [batch][51] out */
    int32_t* next_actions;       /* [batch] out: a* */
    float* probs;                /* [batch][51] out, nullable: the online distribution of the stored action */
    float* grads;                /* [36,774] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_rb_workspace_bytes(batch) */
    uint64_t sample_seed;        /* also the seed of the two learning samples */
    uint64_t sample_update;      /* also u, the key of the two learning samples */
    int64_t sample_upper;
    int32_t batch;
    float gamma;
    void* mid_event;
    const float* weights;        /* [batch] nullable */
    float* prio;                 /* [batch] out: max(rowloss, 0) */
    int32_t* horizon;            /* [batch] out */
    int32_t n_step;              /* 1 .. MI_RB_MAX_N, < slots */
    int32_t noisy;               /* 0: both networks are their means */
    int64_t head_slot;
    float v_min;
    float v_max;
} mi_rb_batch_t;

/* layout-identical to mi_pdd_adam_t */
typedef struct mi_rb_adam_t {
    float* exp_avg;              /* [36,774] */
    float* exp_avg_sq;           /* [36,774] */
    int64_t step;
    double lr, beta1, beta2, eps;
} mi_rb_adam_t;

/* the key of one noise sample (mi_nz_key_t) */
typedef struct mi_rb_key_t {
    uint64_t seed, a, b;
    uint32_t stream;             /* 0 .. 15 */
    uint32_t reserved;
} mi_rb_key_t;

int mi_rb_version(void);
const char* mi_rb_last_error(void);
const char* mi_rb_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: RB_ALLSRC) */
size_t mi_rb_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* the sample of (seed, a, b, stream) as the kernels form it: xi_out [321]; fin_out [153][84] and fout_out [153], the input and output factors head row r uses
 * (eps of its weight k is fout[r] * fin[r][k], of its bias fout[r]); one one-workgroup launch */
int mi_rb_noise(uint64_t seed, uint64_t a, uint64_t b, uint32_t stream, float* xi_out, float* fin_out, float* fout_out, void* hip_stream);

/* probs [n][2][51] and / or q [n][2] (either may be NULL, not both) of obs [n][4]; key == NULL: the mean network, else every row under the ONE sample of *key */
int mi_rb_forward(const float* params, const float* obs, int n, const mi_rb_key_t* key, float v_min, float v_max, float* probs, float* q, void* stream);

/* mi_nz_act_steps for this network */
int mi_rb_act_steps(void* handle, const mi_rb_ring_t* ring, const mi_rb_act_t* a, void* stream);

/* next_actions [batch], target_probs [batch][51] and horizon [batch] of the rows idx [batch]; one launch */
int mi_rb_target(const mi_rb_ring_t* ring, const mi_rb_batch_t* b, void* stream);
/* loss, gradient, prio (and next_actions, target_probs, horizon, probs): two launches; mi_rb_update's second launch also applies Adam (bit-identical to mi_rb_grad
 * followed by libmirl's mi_adam) */
int mi_rb_grad(const mi_rb_ring_t* ring, const mi_rb_batch_t* b, void* stream);
int mi_rb_update(const mi_rb_ring_t* ring, const mi_rb_batch_t* b, const mi_rb_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
