/* mi_noisy.h — C ABI of libmirl_noisy.so: noisy-net exploration (Fortunato et al. 2018, factorised Gaussian noise, as Rainbow uses it: Hessel et al. 2018) on
 * n-step prioritized dueling Double DQN on CartPole-v1, for gfx950.
 *
 * A ninth library beside libmirl.so (include/mi_rl.h), libmirl_pg.so, libmirl_c51.so, libmirl_iqn.so, libmirl_qr.so, libmirl_ddqn.so, libmirl_pdd.so
 * (include/mi_pdd.h) and libmirl_nstep.so (include/mi_nstep.h).  It needs no symbol of the other eight.  Unlike libmirl_nstep.so it has its own acting and forward
 * entry points: the noise changes both.  The prioritized sampler stays libmirl's mi_per_*.
 *
 * Everything is mi_nstep.h's (and through it mi_pdd.h's) — the torso, THE definition of the two action values and of argmax, the walk, the double target
 * R + lg * q'_{a*}(obs[s_m]), weights, td_abs, horizon, loss, the backward, the slab summation order, Adam, the ring layout, the streams 0, 3 and 4 — with ONE
 * change: the 255-element dueling head is a distribution (mu, sigma), and every evaluation uses an effective head theta = mu + sigma * eps.  Read those two headers
 * for the rest; the conventions (return codes, device pointers, 16-byte alignment, nothing synchronises) are theirs too.
 *
 * Parameters, MI_NZ_NPARAMS = 11,274 floats:
 *     elements 0 .. 11,018: mi_pdd.h's vector unchanged — the torso (10,764 floats) and the head's means mu in the order Wv[84] bv Wa[2][84] ba[2] at MI_NZ_WV
 *     elements 11,019 .. 11,273: the head's sigma in the same order, at MI_NZ_SIGMA
 *   The slab stride is MI_NZ_SLAB_STRIDE = 11,276.  Only the two streams behind the torso are noisy (Rainbow's noisy value and advantage streams behind its
 *   convolutional torso); csrc/mi_torso.h's torso stays plain.
 *
 * Numerics and RNG contract of the noise, fp32 (tests/_noisy_ref.py restates it in numpy).
 *   One noise SAMPLE, keyed by (seed, a, b, stream), is 171 numbers xi_c = sgn(z_c) * sqrtf(|z_c|), c = 0 .. 170.  z_c is libmirl's keyed normal (mi_sac.hip's
 *   expression), one Philox4x32-10 call per number:
 *       mi_philox(seed, a, b * 256 + c, stream, r)
 *       u1 = ((float)(r[0] >> 8) + 0.5f) * 2^-24;   u2 = (float)(r[1] >> 8) * 2^-24
 *       z  = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2)
 *   The meaning of c: 0 .. 83 the value stream's inputs, 84 the value output, 85 .. 168 the advantage stream's inputs, 169 and 170 the advantage outputs.
 *   The element noise eps, in head order:
 *       Wv[k]:    xi_84 * xi_k
 *       bv:       xi_84
 *       Wa[j][k]: xi_{169 + j} * xi_{85 + k}
 *       ba[j]:    xi_{169 + j}
 *   The effective head is theta_t = mu_t + sigma_t * eps_t: a product, then a sum (nothing is contracted).
 *   Which sample where:
 *   - Acting: step `ctr` (the env's step counter) of env `env_id` draws (a, b) = (env_id, ctr) on stream 13 with the env handle's seed: one fresh network per env
 *     and step, whether or not earlier steps explored.
 *   - Update u = sample_update with seed = sample_seed: the ONLINE network draws (u, 0) and the TARGET network (u, 1) on stream 14.  ONE online sample serves both
 *     obs[i] and the bootstrap observation obs[s_m] (Rainbow's single reset_noise per learn call); the target's sample is independent of it.
 *   - Streams 13 and 14 are new; the stream tag has 4 bits and 0 .. 12 are taken.
 *   Gradient: the gradient g_t of effective head element t is accumulated exactly as mi_nstep.h's head gradient; then grads[MI_NZ_WV + t] = g_t and
 *   grads[MI_NZ_SIGMA + t] = g_t * eps_t (one product per slab, the slabs summed in the order of mi_pdd.h).  The torso's backward reads the effective head.
 *   `noisy` (int32 in the act, batch and forward arguments): 0 means eps == 0 and no draw is made.  Then every output of mi_nz_grad, mi_nz_target and mi_nz_forward
 *   equals mi_ns_grad's, mi_ns_target's and mi_pdd_forward's on the first 11,019 floats bit for bit, mi_nz_act_steps leaves the ring, env state and episode log
 *   mi_pdd_act_steps leaves, and the sigma gradient is exact zeros.  These are the library's anchors and the engine's evaluation mode.
 */
#ifndef MI_NOISY_H
#define MI_NOISY_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h" /* mi_episode_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MI_NZ_VERSION 1
#define MI_NZ_NPARAMS 11274
#define MI_NZ_H1 120
#define MI_NZ_H2 84
#define MI_NZ_W1 0
#define MI_NZ_B1 480
#define MI_NZ_W2 600
#define MI_NZ_B2 10680
#define MI_NZ_WV 10764
#define MI_NZ_BV 10848
#define MI_NZ_WA 10849
#define MI_NZ_BA 11017
#define MI_NZ_SIGMA 11019         /* sigma of head element t at MI_NZ_SIGMA + t, t < MI_NZ_NHEAD */
#define MI_NZ_NHEAD 255
#define MI_NZ_NXI 171
#define MI_NZ_MAX_SLABS 128
#define MI_NZ_SLAB_STRIDE 11276   /* MI_NZ_NPARAMS + the row losses' sum, rounded up to a multiple of 4 */
#define MI_NZ_MAX_N 16
#define MI_NZ_MAX_STEPS_PER_CALL 64
#define MI_NZ_STREAM_ACT 13
#define MI_NZ_STREAM_LEARN 14

enum { MI_NZ_OK = 0, MI_NZ_EINVAL = -1, MI_NZ_EHIP = -2 };

/* layout-identical to mi_pdd_ring_t */
typedef struct mi_nz_ring_t {
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_nz_ring_t;

/* mi_pdd_act_t with `noisy` behind it */
typedef struct mi_nz_act_t {
    const float* params;             /* [11,274] online network */
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
    int32_t reserved;
} mi_nz_act_t;

/* mi_ns_batch_t as an identical prefix, with `noisy` behind it */
typedef struct mi_nz_batch_t {
    const float* params;         /* [11,274] online network (mi_nz_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [11,274] */
    int64_t* idx;                /* [batch] */
    float* current;              /* [batch] out */
    float* target;               /* [batch] out */
    int32_t* next_actions;       /* [batch] out */
    float* grads;                /* [11,274] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_nz_workspace_bytes(batch) */
    uint64_t sample_seed;        /* also the seed of the two learning samples */
    uint64_t sample_update;      /* also u, the key of the two learning samples */
    int64_t sample_upper;
    int32_t batch;
    float gamma;
    void* mid_event;
    const float* weights;        /* [batch] nullable */
    float* td_abs;               /* [batch] out */
    int32_t* horizon;            /* [batch] out */
    int32_t n_step;              /* 1 .. MI_NZ_MAX_N, < slots */
    int64_t head_slot;
    int32_t noisy;               /* 0: both networks are their means */
    int32_t reserved;
} mi_nz_batch_t;

/* layout-identical to mi_pdd_adam_t */
typedef struct mi_nz_adam_t {
    float* exp_avg;              /* [11,274] */
    float* exp_avg_sq;           /* [11,274] */
    int64_t step;
    double lr, beta1, beta2, eps;
} mi_nz_adam_t;

/* the key of one noise sample */
typedef struct mi_nz_key_t {
    uint64_t seed, a, b;
    uint32_t stream;             /* 0 .. 15 */
    uint32_t reserved;
} mi_nz_key_t;

int mi_nz_version(void);
const char* mi_nz_last_error(void);
const char* mi_nz_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: NZ_ALLSRC) */
size_t mi_nz_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* the sample of (seed, a, b, stream) as the kernels form it: xi_out [171], eps_out [255] in head order; one one-workgroup launch */
int mi_nz_noise(uint64_t seed, uint64_t a, uint64_t b, uint32_t stream, float* xi_out, float* eps_out, void* hip_stream);

/* q [n][2] of obs [n][4]; key == NULL: the mean network (mi_pdd_forward on the first 11,019 floats), else every row under the ONE sample of *key (a host struct) */
int mi_nz_forward(const float* params, const float* obs, int n, const mi_nz_key_t* key, float* q, void* stream);

/* mi_pdd_act_steps with a freshly drawn head at every greedy step */
int mi_nz_act_steps(void* handle, const mi_nz_ring_t* ring, const mi_nz_act_t* a, void* stream);

/* mi_ns_target / mi_ns_grad / mi_ns_update under the two learning samples */
int mi_nz_target(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, void* stream);
int mi_nz_grad(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, void* stream);
int mi_nz_update(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, const mi_nz_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
