/* mi_mdqn.h — C ABI of libmirl_mdqn.so: Munchausen DQN (Vieillard, Pietquin, Geist, NeurIPS 2020) on CartPole-v1, for gfx950.
 *
 * The twelfth library.  Like libmirl_nstep.so it has training calls only: acting and the forward pass of the plain QNetwork stay libmirl_ddqn.so's
 * (include/mi_ddqn.h), on the same ring and the same 10,934-float vectors.  mi_md_ring_t and mi_md_adam_t are laid out as mi_ddqn_ring_t and mi_ddqn_adam_t; the batch
 * is mi_ddqn_batch_t with two outputs and three hyper-parameters behind it.  It needs no symbol of any other library.
 *
 * The reference has no munchausen_dqn.py.  The algorithm is dqn.py's / double_dqn.py's loop, storage, seeding order, printed line, hyper-parameters, epsilon-greedy
 * acting, MSE loss and Adam, with the TD target replaced: the scaled, clipped log-policy of the stored action is added to the reward, and the bootstrap is the soft
 * (entropy-regularised) value; both come from the TARGET network.  The yardsticks are a float64 torch restatement in the paper's own form (tests/_mdqn_ref.py), the
 * identity to Double DQN below, and the same algorithm written as a plain torch script (tools/capture_mdqn_ref.py).
 *
 * Conventions: those of mi_ddqn.h.  Every call returns MI_MD_OK (0) or a negative MI_MD_E* code, mi_md_last_error() gives the text (thread-local); NULL / 0
 * arguments are errors, never crashes; all pointers are DEVICE pointers, `stream` is a hipStream_t (NULL: the default stream); no call synchronises the host,
 * allocates or frees; parameter vectors, observation arrays and the workspace must be 16-byte aligned, anything else is MI_MD_EINVAL.
 *
 * Network and flat parameter layout: mi_ddqn.h's (libmirl's MI_DQN layout, the QNetwork of dqn.py), 10,934 floats.
 *
 * Numerics contract, fp32 (tests/_mdqn_ref.py states the same algorithm in torch).  fmaf(a, b, c) is the fused a * b + c and is written out where it is meant;
 * nothing else is contracted.
 *   Torso and THE definition of the two action values q_0, q_1 of a network at an observation: mi_ddqn.h's, unchanged.
 *   Soft-max quantities of the two action values (q0, q1) of a network at an observation, it = 1.0f / tau:
 *     v     = fmaxf(q0, q1)
 *     u_a   = (q_a - v) * it                 (<= 0, one of them exactly 0)
 *     lse   = logf(expf(u_0) + expf(u_1))    (the accurate expf / logf of mi_common.h's two-action soft-max, not the fast intrinsics)
 *     slp_a = tau * (u_a - lse)              (tau * ln pi_a)
 *     V     = v + tau * lse                  (the soft value sum_a pi_a (q_a - tau ln pi_a) in closed form)
 *   Target of batch row b with ring row i, successor nx, stored action a = (actions[i] != 0) and lg = terminated[nx] ? 0 : gamma; the TARGET network is evaluated
 *   at obs[i] and at obs[nx]:
 *     bonus[b]        = fminf(fmaxf(slp_a of the TARGET network at obs[i], clip_lo), 0.0f)
 *     soft_value[b]   = V of the TARGET network at obs[nx]
 *     next_actions[b] = (q1 > q0) of the TARGET network at obs[nx]       (a diagnostic; a bit-for-bit tie goes to action 0; written for terminated rows too)
 *     target[b]       = (r[nx] + alpha * bonus[b]) + lg * soft_value[b]  (two products and two sums, none fused)
 *   The bonus is not masked by `terminated`: it belongs to (s, a).
 *   Loss, gradient, backward, slab ownership (G = min(B, MI_MD_MAX_SLABS)), the fixed-order slab sum and the Adam step that rides on it: mi_ddqn.h's, unchanged, with
 *   current[b] the ONLINE network's value of the stored action at obs[i].  The target carries no gradient.  No floating-point atomics: two runs give the same bits.
 *   Identity: with alpha = 0, a tau so small that expf(u) underflows to 0 for the smaller action value at every successor (then lse = logf(1) = 0 and V = v), and a
 *   target network equal to the online one bit for bit, target, current, loss and grads are mi_ddqn_grad's bit for bit, and next_actions too.
 *
 * Replay ring and minibatch sampling (Philox stream 4): mi_ddqn.h's.
 */
#ifndef MI_MDQN_H
#define MI_MDQN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_MD_VERSION 1
#define MI_MD_NPARAMS 10934
#define MI_MD_H1 120
#define MI_MD_H2 84
#define MI_MD_W1 0
#define MI_MD_B1 480
#define MI_MD_W2 600
#define MI_MD_B2 10680
#define MI_MD_W3 10764
#define MI_MD_B3 10932
#define MI_MD_MAX_SLABS 128
#define MI_MD_SLAB_STRIDE 10936   /* MI_MD_NPARAMS + the row losses' sum + one float of padding (a multiple of 4) */

enum { MI_MD_OK = 0, MI_MD_EINVAL = -1, MI_MD_EHIP = -2 };

typedef struct mi_md_ring_t {    /* == mi_ddqn_ring_t */
    float* observations;         /* [slots][N][4] */
    int64_t* actions;            /* [slots][N] */
    float* rewards;              /* [slots][N] */
    uint8_t* terminated;         /* [slots][N] */
    int64_t slots;               /* >= 2 */
    int32_t n_envs;              /* >= 1 */
    int32_t reserved;
} mi_md_ring_t;

typedef struct mi_md_batch_t {   /* mi_ddqn_batch_t with bonus, soft_value, alpha, tau and clip_lo behind it */
    const float* params;         /* [10,934] online network (mi_md_update writes it: the caller owns it mutable) */
    const float* target_params;  /* [10,934] */
    int64_t* idx;                /* [batch] flat ring indices: an input, or written when sample_upper > 0 */
    float* current;              /* [batch] out: the online value of the stored action */
    float* target;               /* [batch] out */
    int32_t* next_actions;       /* [batch] out: the target network's greedy action at the successor (a diagnostic) */
    float* grads;                /* [10,934] out */
    float* loss;                 /* [1] out */
    void* workspace;             /* mi_md_workspace_bytes(batch) */
    uint64_t sample_seed;
    uint64_t sample_update;
    int64_t sample_upper;        /* > 0: row b's index is drawn in the launch (stream 4) and stored in idx; 0: idx is given */
    int32_t batch;               /* >= 1 */
    float gamma;
    void* mid_event;             /* nullable hipEvent_t recorded on `stream` between the two launches of mi_md_grad / mi_md_update (timing tools) */
    float* bonus;                /* [batch] out: the clipped tau * ln pi(a | s) of the target network, before the factor alpha */
    float* soft_value;           /* [batch] out: the target network's soft value at the successor */
    float alpha;                 /* finite */
    float tau;                   /* > 0, finite, and so is 1.0f / tau */
    float clip_lo;               /* <= 0 (the paper's l0) */
} mi_md_batch_t;

typedef struct mi_md_adam_t {    /* == mi_ddqn_adam_t */
    float* exp_avg;              /* [10,934] */
    float* exp_avg_sq;           /* [10,934] */
    int64_t step;                /* 1-based index of THIS optimizer step */
    double lr, beta1, beta2, eps;
} mi_md_adam_t;

int mi_md_version(void);
const char* mi_md_last_error(void);
const char* mi_md_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: MD_ALLSRC) */
size_t mi_md_workspace_bytes(int batch);   /* 0 for batch <= 0 */

/* bonus, soft_value, next_actions and target [batch] of the rows b->idx from b->target_params; one launch, exactly the first pass of the gradient launch.  Reads of
 * `b`: target_params, idx, bonus, soft_value, next_actions, target, batch, gamma, alpha, tau, clip_lo */
int mi_md_target(const mi_md_ring_t* ring, const mi_md_batch_t* b, void* stream);

/* loss and gradient of one batch: two launches (targets + online forward + loss + backward into per-workgroup slabs; fixed-order slab sum) */
int mi_md_grad(const mi_md_ring_t* ring, const mi_md_batch_t* b, void* stream);
/* the same two launches, the second of which also applies optimizer.step() to every gradient element it has just summed: bit-identical to mi_md_grad followed by
 * libmirl's mi_adam */
int mi_md_update(const mi_md_ring_t* ring, const mi_md_batch_t* b, const mi_md_adam_t* opt, void* stream);

#ifdef __cplusplus
}
#endif
#endif
