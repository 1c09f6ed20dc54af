/* mi_ars.h — C ABI of libmirl_ars.so: Augmented Random Search (Mania, Guy, Recht 2018; ARS V2-t with discrete actions, V1 with normalize = 0) on CartPole-v1
 * for gfx950.
 *
 * A thirteenth library beside libmirl.so (include/mi_rl.h) and the eleven others.  It needs no symbol of the other twelve, no env handle, no ring, no optimizer and
 * no backward pass: an iteration is whole episodes of 2 N slightly different LINEAR policies run side by side, one lane each, and one small update launch.
 *
 * Conventions (those of mi_eval.h)
 *   - every call returns MI_ARS_OK (0) or a negative MI_ARS_E* code; mi_ars_last_error() gives the text (thread-local).  NULL, zero, misaligned and out-of-range
 *     arguments are errors before any HIP call, never crashes.
 *   - all pointers are DEVICE pointers; `stream` is a hipStream_t (NULL: the default stream).
 *   - no call synchronises the host, allocates or frees: everything is enqueued on `stream`.
 *
 * State, all device-resident and each 16-byte aligned
 *   policy     f32 [2][4]   M, row a = action a; no bias.  A fresh run starts from zeros.
 *   stats      f64 [9]      n, So[4], Soo[4]: the count, the sums and the sums of squares of every observation a TRAINING episode acted on
 *   norm       f64 [8]      mu[4], scale[4]; a fresh run starts from 0 / 1.  Read by every episode; written by the update with normalize != 0 only.
 *   iteration  i64 [1]      k.  Read by the training episodes on the device, incremented by the update on the device.
 *
 * Numerics contract.  fp64 unless said otherwise; every product, sum, difference, quotient and square root is rounded on its own (round to nearest even; nothing is
 * contracted into a fused multiply-add).  (double) of an f32 is exact.
 *
 * The draw.  Direction i < N of iteration k has delta_i, f32 [8], element c = 4 a + j belonging to M[a][j]:
 *     mi_philox(seed, i, 8 k + c, 15, r)                                                 (csrc/mi_common.h; stream 15 — the 4-bit stream field's 0 .. 14 are taken)
 *     u1 = ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);   u2 = (float)(r[1] >> 8) * (1.0f / 16777216.0f)
 *     delta_i[c] = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2)          (fp32: libmirl's keyed normal, mi_noisy.h's z_c)
 *   The key holds i and k but not N: the directions of N = 3 are the first three of N = 8.  The logarithm, the square root and the cosine are the device library's
 *   fp32 routines: this draw is the one output that is held to a float64 restatement within a bound and not bit for bit.
 *
 * Training episode e = 2 i + s, i < N, s in {0, 1}  (sigma = +1 for s = 0, -1 for s = 1)
 *   w[a][j] = (double)M[a][j] + sigma * ((double)noise * (double)delta_i[4 a + j])       (the product of two f32 is exact in fp64: one rounding)
 *   start    mi_reset_noise(seed, env_id_base + e, k)                                   (Philox stream 0: both signs of a direction start differently)
 *   step t = 0, 1, ...  with the fp64 state (y_0 .. y_3):
 *     o_j = (double)(float)y_j                                                          (the observation: the state rounded once to f32)
 *     n += 1;  So_j += o_j;  Soo_j += o_j * o_j                                         (the episode's partials, in step order, from zeros)
 *     x_j = (o_j - mu_j) * scale_j
 *     s_a = ((w[a][0] * x_0 + w[a][1] * x_1) + w[a][2] * x_2) + w[a][3] * x_3
 *     action = (s_1 > s_0) ? 1 : 0                                                       (a tie goes to action 0; a NaN compares false: action 0)
 *     mi_cartpole_step advances the state.
 *   The episode ends with the step that terminates, or with the 500th step; truncated[e] = 1 exactly when the 500th step does not terminate.  lengths[e] = the
 *   steps taken (1 .. 500), returns[e] = (float)lengths[e], actions[e][t] is written for t < lengths[e] only, partials[e] = {n, So[4], Soo[4]}.
 *   Lane s = 0 of a direction also writes deltas[i][0 .. 7].
 *
 * Evaluation episode e < n_episodes (the mode of n_episodes >= 1; noise must be 0)
 *   w = (double)M, start mi_reset_noise(seed, env_id_base + e, 0), the current norm; steps, actions and outputs as above.  No delta is drawn, neither deltas nor
 *   partials are written, iteration is not read: nothing of the state changes.
 *
 * Update (one launch of one workgroup), given returns [2 N] (whole numbers 0 .. 500, as the episodes write them) and deltas [N][8]
 *   rp_i = returns[2 i], rm_i = returns[2 i + 1];  key_i = (rp_i > rm_i) ? rp_i : rm_i
 *   rank_i = #{ j : key_j > key_i, or key_j == key_i and j < i };   direction i is SELECTED where rank_i < b   (b = n_top; exactly b directions)
 *   S1 = sum of rp_i + rm_i, S2 = sum of rp_i^2 + rm_i^2 over the selected i, in integers ((int) of each return: exact for whole numbers)
 *   sigma_R = sqrt((double)(2 b S2 - S1^2) / (double)(4 b^2))                            (the population deviation of the 2 b selected returns: one division, one root)
 *   if sigma_R == 0 (2 b S2 == S1^2): M keeps its bits.  Otherwise, for c < 8:
 *     g_c = the sum over the selected i in ASCENDING i, serially from 0, of ((double)rp_i - (double)rm_i) * (double)deltas[i][c]
 *     M[c] = (float)((double)M[c] + ((double)step_size / ((double)b * sigma_R)) * g_c)
 *   stats[c], c < 9:  stats[c] = (...((stats[c] + partials[0][c]) + partials[1][c]) ... + partials[2 N - 1][c]): serially in ASCENDING e onto the old value
 *   with normalize != 0, for j < 4, from the NEW stats:
 *     mu_j = So_j / n;  v = Soo_j / n - mu_j * mu_j;  var = (v > 0) ? v : 0;  sd = sqrt(var);  scale_j = (sd < 1e-7) ? 0 : 1 / sd
 *     (they serve the NEXT iteration's episodes; a NaN v gives var = 0 and scale = 0)
 *   iteration += 1
 *
 * Launch shape.  Episodes: 64-thread workgroups (one wave each), lane = episode; workgroup g of G = min(ceil(E / 64), max_workgroups or MI_ARS_DEFAULT_WORKGROUPS)
 * runs the episode blocks g, g + G, ...: episode e's outputs do not depend on G, on E or on what ran beside it.  The step loop has the compile-time bound 500,
 * so the launch ends whatever M holds, NaN included; a wave leaves the loop when all its lanes are done.
 */
#ifndef MI_ARS_H
#define MI_ARS_H
#include <stddef.h>
#include <stdint.h>

#include "mi_rl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ARS_VERSION 1
#define MI_ARS_MAX_STEPS 500            /* CartPole-v1's TimeLimit: the row length of actions */
#define MI_ARS_MAX_DIRECTIONS 4096
#define MI_ARS_DEFAULT_WORKGROUPS 1024
#define MI_ARS_NPARAMS 8
#define MI_ARS_NSTATS 9
#define MI_ARS_STREAM 15                /* the Philox stream of the directions */

enum { MI_ARS_OK = 0, MI_ARS_EINVAL = -1, MI_ARS_EHIP = -2 };

typedef struct mi_ars_args_t {
    float* policy;           /* [2][4] state, 16-byte aligned */
    double* stats;           /* [9] state, 16-byte aligned */
    double* norm;            /* [8] state, 16-byte aligned */
    int64_t* iteration;      /* [1] state, 16-byte aligned */
    float* deltas;           /* [N][8]: out of the training episodes, in of the update; 16-byte aligned */
    float* returns;          /* [E]: out of the episodes, in of the update; mi_ars_iterate: [n_iterations][2 N] */
    int32_t* lengths;        /* [E] out; mi_ars_iterate: [n_iterations][2 N] */
    uint8_t* truncated;      /* [E] out, nullable (mi_ars_iterate: the last iteration's) */
    uint8_t* actions;        /* [E][500] out, nullable: row e written for t < lengths[e] only (mi_ars_iterate: the last iteration's) */
    double* partials;        /* [2 N][9]: out of the training episodes, in of the update; 8-byte aligned */
    uint64_t seed;
    uint64_t env_id_base;
    int32_t n_directions;    /* N: 1 .. MI_ARS_MAX_DIRECTIONS (training mode, E = 2 N) */
    int32_t n_top;           /* b: 1 .. N */
    int32_t n_episodes;      /* 0: training mode; >= 1: evaluation mode with E = n_episodes (noise must be 0; N and b are not read) */
    int32_t max_workgroups;  /* 0: MI_ARS_DEFAULT_WORKGROUPS, else >= 1 */
    int32_t normalize;       /* the update recomputes norm (V2) or leaves it (V1) */
    float step_size;         /* alpha: finite */
    float noise;             /* nu: finite, >= 0 */
    int32_t reserved;
} mi_ars_args_t;

int mi_ars_version(void);
const char* mi_ars_last_error(void);
const char* mi_ars_source_id(void);   /* 12 hex digits over the code of this library's own sources (csrc/Makefile: ARS_ALLSRC) */

/* the episodes of one iteration (training mode) or n_episodes greedy episodes (evaluation mode): ONE launch */
int mi_ars_episodes(const mi_ars_args_t* a, void* stream);

/* the update of one iteration from a->returns, a->deltas and a->partials: ONE launch */
int mi_ars_update(const mi_ars_args_t* a, void* stream);

/* n_iterations times (episodes, update): 2 n launches, nothing read back between them; iteration t writes returns / lengths rows t */
int mi_ars_iterate(const mi_ars_args_t* a, int n_iterations, void* stream);

#ifdef __cplusplus
}
#endif
#endif
