/* mi_eval.h — C ABI of libmirl_eval.so: greedy policy evaluation on CartPole-v1 for gfx950.
 *
 * An eleventh library beside libmirl.so (include/mi_rl.h), libmirl_pg.so, libmirl_c51.so (include/mi_c51.h), libmirl_iqn.so, libmirl_qr.so (include/mi_qr.h),
 * libmirl_ddqn.so (include/mi_ddqn.h), libmirl_pdd.so (include/mi_pdd.h), libmirl_nstep.so, libmirl_noisy.so (include/mi_noisy.h) and libmirl_rainbow.so
 * (include/mi_rainbow.h).  It needs no symbol of the other ten and no env handle: an evaluation episode is keyed (seed, env id, episode 0), runs from its reset to
 * its end inside ONE launch and leaves nothing behind but its outputs.  No ring, no auto-reset, no epsilon, no noise, no Philox draw besides the reset.
 *
 * Conventions
 *   - every call returns MI_EV_OK (0) or a negative MI_EV_E* code; mi_ev_last_error() gives the text (thread-local).  NULL, zero, misaligned and out-of-range
 *     arguments are errors before any HIP call, never crashes.
 *   - all pointers are DEVICE pointers; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: everything is enqueued on `stream`.
 *   - parameter vectors and observation arrays must be 16-byte aligned (they are read as float4); anything else is MI_EV_EINVAL.
 *   - the parameters are only read.
 *
 * Head kinds.  All share the torso 4 -> 120 -> 84 at the flat offsets of csrc/mi_torso.h (W1 [120][4] at 0, b1 [120] at 480, W2 [84][120] at 600, b2 [84] at
 * 10,680); the head starts at 10,764.  The two action values of a kind are THE action values of the library that owns the kind: the expressions, chains and orders
 * below restate that library's header and give the same bits as its forward call.
 *   MI_EV_DUELING  the first 11,019 floats read.  mi_pdd.h (dueling DQN, PDD, n-step; also the mean network of NoisyDuelingQNetwork, whose 11,274-float vector
 *                  holds the same 11,019 means in front: mi_noisy.h).  Wv [84] at 10,764, bv at 10,848, Wa [2][84] at 10,849, ba [2] at 11,017.
 *   MI_EV_QR       21,644 floats read.  mi_qr.h's collapsed head.  W3 [128][84] at 10,764 (row a * 64 + i: action a, quantile i), b3 [128] at 21,516.
 *   MI_EV_C51      27,934 floats read.  mi_c51.h, 101 atoms, the support a run-time pair here.  W3 [202][84] at 10,764 (row a * 101 + j), b3 [202] at 27,732.
 *   MI_EV_RAINBOW  the first 23,769 floats read (the means; no sigma is touched).  mi_rainbow.h with noisy == 0, 51 atoms.  Wv [51][84] at 10,764, bv [51] at
 *                  15,048, Wa [2][51][84] at 15,099, ba [2][51] at 23,667.
 *   The plain QNetwork (DQN, PER, Double DQN; 10,934 floats) has NO kind: its two owners disagree.  libmirl's mi_dqn_forward adds layer 2 on two interleaved
 *   60-term accumulators and the bias last, mi_ddqn_forward on three 40-term chains from the bias; the two differ in the last bits on almost every row, so no
 *   values could be "the owner's forward, bit for bit" for both.  The kind value 0 is kept free for it.
 *   IQN is out of scope: it has a torso of its own and draws its taus, so a greedy IQN step is not a function of the parameters and the observation alone.  PPO and
 *   REINFORCE are out of scope too: their policies are stochastic, and REINFORCE already runs whole episodes in libmirl_pg.so.
 *
 * Numerics contract, fp32.  fmaf(a, b, c) is the fused a * b + c; nothing else is contracted.  "chain over k of (w_k, v_k) from s" means acc = s; for ascending k:
 * acc = fmaf(w_k, v_k, acc).
 *   Torso (mi_c51.h / mi_pdd.h):
 *     z1_u = fmaf(W1[u][3], x3, fmaf(W1[u][2], x2, fmaf(W1[u][1], x1, fmaf(W1[u][0], x0, b1[u]))));  h1_u = max(z1_u, 0)
 *     P_c[o] = chain over k = 40 c .. 40 c + 39 of (W2[o][k], h1_k) from b2[o] for c = 0 and from 0 for c = 1, 2
 *     z2_o = (P_0[o] + P_1[o]) + P_2[o];  h2_o = max(z2_o, 0)
 *   DUELING (mi_pdd.h):   v = chain of (Wv[k], h2_k) from bv;  A_a = chain of (Wa[a][k], h2_k) from ba[a];  m = (A_0 + A_1) * 0.5f;  q_a = v + (A_a - m)
 *   QR (mi_qr.h):         wbar[a][k] = (serial sum over ascending i < 64 of W3[a * 64 + i][k], from 0) * (1.0f / 64.0f), bbar[a] likewise of b3[a * 64 + i];
 *                         q_a = chain over k < 84 of (wbar[a][k], h2_k) from bbar[a]
 *   C51 (mi_c51.h):       logit[a][j] = chain over k < 84 of (W3[a * 101 + j][k], h2_k) from b3[a * 101 + j];  dz = (v_max - v_min) / 100;  z_j = v_min + dz * j
 *                         (a product, then a sum: with (-100, 100) dz is 2 exactly and z_j is mi_c51.h's -100 + 2 j).  One 64-lane wave per action, lane i holding
 *                         atoms i and i + 64 (the latter masked past atom 100):  m = max_j logit_j;  e_j = expf(logit_j - m);
 *                         s = TREE(e_i + e_{i + 64});  p_j = e_j / s;  q_a = TREE(fmaf(p_{i + 64}, z_{i + 64}, p_i * z_i))   (p_i * z_i alone where i + 64 > 100)
 *   RAINBOW (mi_rainbow.h, noisy == 0):  y_r = chain over k < 84 of (mu[r][k], h2_k) from the row's bias mean;  v_j = y_j, A[a][j] = y_{51 + 51 a + j};
 *                         l[a][j] = v_j + (A[a][j] - 0.5f * (A[0][j] + A[1][j]));  dz = (v_max - v_min) / 50;  z_j = v_min + dz * j;  one wave per action, lane j
 *                         holding atom j (lanes 51 .. 63: atom 50 repeated in the max, 0 in every sum):  m = max l_j;  e_j = expf(l_j - m);  s = TREE(e);
 *                         p_j = e_j / s;  q_a = TREE(p_j * z_j)
 *   TREE(v): the balanced pairwise sum over the 64 lanes in natural order, (t0 + t1) + (t2 + t3) ..., six levels.
 *   Greedy action: a = (q_1 > q_0) ? 1 : 0.  A bit-for-bit tie goes to action 0; a NaN comparison is false: action 0.
 *   gap = |q_1 - q_0| (fp32).  min_gap starts at +infinity and takes gap where gap < min_gap, so a NaN gap never enters it.
 *
 * Episode e, 0 <= e < n_episodes (libmirl's CartPole-v1: csrc/mi_common.h)
 *   env id = env_id_base + e.  Start state: mi_reset_noise(seed, env id, 0) — Philox stream 0, idx = episode 0 — or forced_starts[e][0 .. 3] when given (fp64).
 *   Observation of a state: its four fp64 numbers each rounded once to fp32, as mi_ddqn_act_steps forms it.
 *   Step t = 0, 1, ...: the network is evaluated at the observation (under forced actions too); the action is forced_actions[e][t] != 0 when given, else the greedy
 *   one; mi_cartpole_step (fp64, no contraction) advances the state.  The episode ends with the step that terminates, or with the 500th step.  truncated[e] = 1
 *   exactly when the 500th step does not terminate: termination on step 500 wins.  lengths[e] = the steps taken (1 .. 500); returns[e] = the fp32 sum of 1.0f per
 *   step; min_gap[e] = the smallest gap over the steps taken; actions[e][t] is written for t < lengths[e] only, the bytes behind stay as they were.
 *   The step loop has the compile-time bound 500: the launch ends whatever the parameters hold, NaN included.
 *   Workgroup g of G = min(n_episodes, max_workgroups or MI_EV_DEFAULT_WORKGROUPS) runs episodes g, g + G, ...: episode e's outputs do not depend on G, on
 *   n_episodes or on what ran beside it, and nothing is carried between calls.
 */
#ifndef MI_EVAL_H
#define MI_EVAL_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_EV_VERSION 1
#define MI_EV_MAX_STEPS 500            /* CartPole-v1's TimeLimit: the row length of actions / forced_actions */
#define MI_EV_DEFAULT_WORKGROUPS 1024  /* 4 per compute unit of a 256-CU MI355X */
#define MI_EV_NPARAMS_DUELING 11019
#define MI_EV_NPARAMS_QR 21644
#define MI_EV_NPARAMS_C51 27934
#define MI_EV_NPARAMS_RAINBOW 23769
#define MI_EV_C51_ATOMS 101
#define MI_EV_RAINBOW_ATOMS 51
#define MI_EV_QR_QUANT 64

enum { MI_EV_OK = 0, MI_EV_EINVAL = -1, MI_EV_EHIP = -2 };
enum { MI_EV_DUELING = 1, MI_EV_QR = 2, MI_EV_C51 = 3, MI_EV_RAINBOW = 4 };   /* 0 is free: see "Head kinds" */

typedef struct mi_ev_args_t {
    const float* params;             /* the kind's parameters (see above), 16-byte aligned; only read */
    float* returns;                  /* [E] out, nullable */
    int32_t* lengths;                /* [E] out */
    uint8_t* truncated;              /* [E] out, nullable */
    float* min_gap;                  /* [E] out, nullable */
    uint8_t* actions;                /* [E][500] out, nullable: row e written for t < lengths[e] only */
    const uint8_t* forced_actions;   /* [E][500] nullable */
    const double* forced_starts;     /* [E][4] nullable */
    uint64_t seed;
    uint64_t env_id_base;
    int32_t kind;                    /* MI_EV_DUELING .. MI_EV_RAINBOW */
    int32_t n_episodes;              /* E >= 1 */
    int32_t max_workgroups;          /* 0: MI_EV_DEFAULT_WORKGROUPS, else >= 1 */
    float v_min;                     /* read by MI_EV_C51 and MI_EV_RAINBOW only: finite, v_min < v_max, finite span */
    float v_max;
    int32_t reserved;
} mi_ev_args_t;

int mi_ev_version(void);
const char* mi_ev_last_error(void);
const char* mi_ev_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: EV_ALLSRC) */

/* q [n][2] of obs [n][4] through the device functions the episode loop uses; v_min / v_max as in mi_ev_args_t */
int mi_ev_forward(const float* params, int kind, float v_min, float v_max, const float* obs, int n, float* q, void* stream);

/* a->n_episodes greedy episodes, ONE launch */
int mi_ev_episodes(const mi_ev_args_t* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
