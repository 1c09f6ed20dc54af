/* mi_reinforce.h — C ABI of libmirl_pg.so: REINFORCE on CartPole-v1 (reference deep_rl/reinforce.py) for gfx950.
 *
 * A second library beside libmirl.so (include/mi_rl.h).  It depends on no symbol of the other one; the only thing they share is the env handle made by
 * libmirl's mi_env_create (a host struct of device pointers, csrc/mi_common.h `struct mi_env`), which this library reads and advances in the same process.
 *
 * Conventions
 *   - every call returns MI_PG_OK (0) or a negative MI_PG_E* code; mi_pg_last_error() gives the text (thread-local).  NULL / 0 arguments are errors, never crashes.
 *   - all pointers in the argument structs are DEVICE pointers unless said otherwise; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: every launch is enqueued on `stream`.
 *
 * Network (reinforce.py:40-46) and flat parameter layout (order of agent.parameters(), 898 floats):
 *     W1 [128][4] at 0, b1 [128] at 512, W2 [2][128] at 640, b2 [2] at 896
 *     Linear(4,128) -> Dropout(p = 0.6) -> ReLU -> Linear(128,2) -> Softmax(-1)
 *
 * Numerics contract, fp32 (tests/_reinforce_ref.py restates exactly this):
 *     z_j  = fmaf(W1[j][3], x3, fmaf(W1[j][2], x2, fmaf(W1[j][1], x1, fmaf(W1[j][0], x0, b1[j]))))          k ascending, starting from the bias
 *     h_j  = keep_j ? max(z_j * 2.5f, 0) : 0          (1 / (1 - 0.6) is 2.5 in f32; eval mode (no mask): h_j = max(z_j, 0))
 *     q_a[i] = fmaf(W2[a][i + 64], h_{i+64}, W2[a][i] * h_i)      i = 0..63 (lane i owns units i and i + 64)
 *     l_a  = b2[a] + TREE(q_a)      TREE: balanced pairwise sum over i in natural order: (q0 + q1) + (q2 + q3) ... six levels
 *     m = max(l0, l1); e_a = exp(l_a - m); s = e0 + e1; p_a = e_a / s; log_prob = (l_a - m) - log(s)     exp / log: hardware v_exp_f32 / v_log_f32 (~1 ulp)
 *     action: a = (u >= p0) ? 1 : 0 with u the env-step's STREAM_ACTION uniform (the PPO rollout's inverse-CDF draw)
 *     CartPole step: fp64, bit-identical to libmirl's mi_env_step; done = terminated or 500 steps (TimeLimit); reward 1 per step
 *   Returns of one episode of `len` rows (reinforce.py:67,73):
 *     R_t = fmaf(gamma, R_{t+1}, 1.0f), R_len = 0;   mean = SUM(R) / len;   var = SUM((R - mean)^2) / (len - 1);   Rn_t = (R_t - mean) / (sqrt(var) + 0.006737947f)
 *     SUM: lane i adds its rows t = i, i + 64, ... in ascending t (the squares by fmaf), then TREE over the 64 lanes.  len == 1 gives NaN as in the reference.
 *   Gradient of  sum_n sum_t -log_prob[n][t] * Rn[n][t]  (reinforce.py:74; a SUM over envs too): forward recompute per valid row with the stored mask,
 *     dl_a = Rn * (p_a - [a == action]), back through W2, ReLU, mask x 2.5, W1.  Summation order: workgroup g owns envs g, g + G, ... (G = min(N, 1024)),
 *     its wave w the rows t = w, w + 8, ... of each, in that order; the 8 waves are added in wave order; the G slabs in 16 groups (g mod 16), each group in
 *     ascending g on four interleaved accumulators ((s0 + s1) + (s2 + s3)), the 16 group sums in ascending group.  No floating-point atomics: two runs give
 *     the same bits.
 *   Adam: torch's single-tensor Adam, the element step and the host-side coefficients of libmirl's mi_adam (bit-identical to it).
 *
 * RNG contract (counter-based Philox4x32-10 as in mi_rl.h: counter = {env id lo, env id hi, idx lo, (idx hi << 4) | stream}, key = seed)
 *   - reset noise: STREAM_RESET (0), idx = episode[n]           — libmirl's stream, unchanged
 *   - action uniform: STREAM_ACTION (1), env-step index step_ctr[n] — libmirl's stream, unchanged
 *   - dropout: MI_PG_STREAM_DROPOUT (8).  Unit u of env-step c (= step_ctr[n] of that step) of global env id E:
 *         block b = (u & 63) >> 1,  word w = 2 * (u & 1) + (u >> 6),  r = philox(seed, E, idx = 32 * c + b, stream 8)[w];  keep  <=>  r < 0x66666666  (P = 0.4)
 *     A pure function of (seed, E, c, u): env E's episode is the same alone (env_id_base = E, N = 1) or as one of 4,096.
 *   - the masks an episode used are STORED (128 bits per row, mask_bits[row][u >> 5] bit (u & 31)); the gradient kernel reads them.
 *
 * Storage: env-major rows, row(n, t) = n * MI_PG_ROWS + t, t = 0 .. 500.  Row len[n] of `observations` holds the terminal observation; rows t >= len[n] of
 * log_probs / returns / b_returns are 0 after an update (reinforce.py:53-54 allocates fresh zeros per episode); the other arrays are left as they were there.
 */
#ifndef MI_REINFORCE_H
#define MI_REINFORCE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_PG_VERSION 1
#define MI_PG_NPARAMS 898
#define MI_PG_HID 128
#define MI_PG_MAX_STEPS 500
#define MI_PG_ROWS 501            /* env.spec.max_episode_steps + 1 (reinforce.py:53) */
#define MI_PG_STREAM_DROPOUT 8u
#define MI_PG_KEEP_BELOW 0x66666666u   /* floor(0.4 * 2^32) */
#define MI_PG_MAX_SLABS 1024

enum { MI_PG_OK = 0, MI_PG_EINVAL = -1, MI_PG_EHIP = -2, MI_PG_ESTATE = -4 };

typedef struct mi_pg_buffers_t {
    float* params;               /* [898] */
    float* exp_avg;              /* [898] Adam moments (mi_pg_update only) */
    float* exp_avg_sq;           /* [898] */
    float* grads;                /* [898] out */
    float* observations;         /* [N][501][4] */
    int32_t* actions;            /* [N][501] */
    float* log_probs;            /* [N][501] */
    float* returns;              /* [N][501] raw R */
    float* b_returns;            /* [N][501] normalised */
    uint32_t* mask_bits;         /* [N][501][4] */
    int32_t* lengths;            /* [N] */
    float* ep_returns;           /* [N] episodic return (RecordEpisodeStatistics' r) */
    void* workspace;             /* mi_pg_workspace_bytes(N) */
    const double* forced_reset;  /* optional [N][4]: replaces the keyed reset noise (teacher forcing) */
    const int32_t* forced_actions; /* optional [N][500] */
    const uint32_t* forced_masks;  /* optional [N][500][4] */
} mi_pg_buffers_t;

typedef struct mi_pg_hparams_t {
    float gamma;
    int32_t reserved;
    int64_t opt_step;            /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_pg_hparams_t;

int mi_pg_version(void);
const char* mi_pg_last_error(void);
const char* mi_pg_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: PG_ALLSRC) */
size_t mi_pg_workspace_bytes(int n_envs);   /* 0 for n_envs <= 0 */

/* probs[n][2] for obs[n][4]; mask_bits [n][4] or NULL (eval mode: no dropout, no 2.5 scale) */
int mi_pg_forward(const float* params, const float* obs, int n, const uint32_t* mask_bits, float* probs, void* stream);

/* One launch: every env of `env` (a CartPole handle of libmirl's mi_env_create) plays one episode from a fresh reset to its own done.  Fills observations,
 * actions, log_probs, mask_bits, lengths, ep_returns; advances the handle (state = the terminal state, elapsed = ep_len = len, ep_ret = return, episode += 1,
 * step_ctr += len), so a following update continues every stream. */
int mi_pg_rollout_episodes(void* env, const mi_pg_buffers_t* b, void* stream);
/* returns / b_returns from lengths (rewards are 1 per step) */
int mi_pg_returns(const mi_pg_buffers_t* b, int n_envs, float gamma, void* stream);
/* grads from observations / actions / mask_bits / b_returns / lengths at params (two launches: per-workgroup slabs, fixed-order slab sum) */
int mi_pg_grad(const mi_pg_buffers_t* b, int n_envs, void* stream);
int mi_pg_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, int64_t step, double lr, double beta1, double beta2, double eps,
               void* stream);
/* rollout + returns + grad + Adam: four launches (Adam rides on the slab sum), no host synchronisation; bit-identical to the four calls above in sequence */
int mi_pg_update(void* env, const mi_pg_buffers_t* b, const mi_pg_hparams_t* h, void* stream);

#ifdef __cplusplus
}
#endif
#endif
