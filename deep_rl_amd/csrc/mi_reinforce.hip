// mi_reinforce.hip — libmirl_pg.so: REINFORCE on CartPole-v1 (reference reinforce.py) for gfx950.  C ABI, numerics and RNG contract: include/mi_reinforce.h.
//
//   pg_episode_kernel   one launch plays all N episodes.  ONE ENV PER WAVE, lane i = hidden units i and i + 64: the step is a 500-deep dependent chain of a tiny
//                       network, so what counts is the latency of one step and how many SIMDs have a wave — 4,096 envs are 4,096 waves (4 per SIMD, every SIMD
//                       busy), one env is one wave at the shortest step this file can write.  The fp64 physics runs in every lane (same cost as in one).
//   pg_returns_kernel   one wave per env: backward recurrence in registers, lane-parallel mean / unbiased std / normalisation.
//   pg_grad_kernel      one wave per row, lane = the same two units; per-workgroup slabs.   pg_reduce_kernel   fixed-order slab sum (+ Adam).
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"

#include "../../include/mi_reinforce.h"

#include <stdarg.h>

#define PG_W1 0
#define PG_B1 512
#define PG_W2 640
#define PG_B2 896
#define PG_NP MI_PG_NPARAMS
#define PG_ROWS MI_PG_ROWS
#define PG_T MI_PG_MAX_STEPS
#define PG_GRAD_WAVES 8
#define PG_EXP_M5 0.006737947f   // np.exp(-5) in f32 (reinforce.py:9,73)

// ---- error plumbing of this library ----------------------------------------------------------------
static thread_local char pg_err[512] = "";
static void pg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(pg_err, sizeof(pg_err), fmt, ap);
    va_end(ap);
}
#define PG_CHECK_ARG(cond, msg)                                       \
    do {                                                              \
        if (!(cond)) {                                                \
            pg_set_error("%s: invalid argument: %s", __func__, msg);  \
            return MI_PG_EINVAL;                                      \
        }                                                             \
    } while (0)
#define PG_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            pg_set_error("%s: %s failed: %s", __func__, #call, hipGetErrorString(e_));    \
            return MI_PG_EHIP;                                                            \
        }                                                                                 \
    } while (0)

#ifndef MI_PG_SOURCE_ID
#define MI_PG_SOURCE_ID "unknown"
#endif
extern "C" int mi_pg_version(void) { return MI_PG_VERSION; }
extern "C" const char* mi_pg_last_error(void) { return pg_err; }
extern "C" const char* mi_pg_source_id(void) { return MI_PG_SOURCE_ID; }
extern "C" size_t mi_pg_workspace_bytes(int n_envs) {
    if (n_envs <= 0) return 0;
    return (size_t)(n_envs < MI_PG_MAX_SLABS ? n_envs : MI_PG_MAX_SLABS) * PG_NP * sizeof(float);
}

#ifdef PG_STAMPS   // diagnostic build: wave 0 of workgroup 0 stores the 100 MHz wall clock at every 16th step of its episode (read back by mi_debug_pg_stamps)
static __device__ unsigned long long pg_stamps[64];
#define PG_STAMP(t) do { if (blockIdx.x == 0 && threadIdx.x == 0 && ((t) & 15) == 0 && ((t) >> 4) < 64) pg_stamps[(t) >> 4] = p2p_clock(); } while (0)
extern "C" int mi_debug_pg_stamps(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(pg_stamps), sizeof(pg_stamps)) == hipSuccess ? 0 : -2; }
#else
#define PG_STAMP(t) do {} while (0)
#endif

// ---- the policy as one wave sees it: lane i holds units i and i + 64 --------------------------------
struct pg_weights {
    float w1a[4], w1b[4], b1a, b1b, w20a, w20b, w21a, w21b, b20, b21;
};
__device__ __forceinline__ pg_weights pg_load_weights(const float* __restrict__ P, int lane) {
    pg_weights w;
    const float4 a = reinterpret_cast<const float4*>(P + PG_W1)[lane], b = reinterpret_cast<const float4*>(P + PG_W1)[lane + 64];
    w.w1a[0] = a.x; w.w1a[1] = a.y; w.w1a[2] = a.z; w.w1a[3] = a.w;
    w.w1b[0] = b.x; w.w1b[1] = b.y; w.w1b[2] = b.z; w.w1b[3] = b.w;
    w.b1a = P[PG_B1 + lane]; w.b1b = P[PG_B1 + lane + 64];
    w.w20a = P[PG_W2 + lane]; w.w20b = P[PG_W2 + lane + 64];
    w.w21a = P[PG_W2 + 128 + lane]; w.w21b = P[PG_W2 + 128 + lane + 64];
    w.b20 = P[PG_B2]; w.b21 = P[PG_B2 + 1];
    return w;
}

// keyed dropout of env-step `ctr` (mi_reinforce.h "RNG contract"): lane i computes block i >> 1 and takes words 2 (i & 1) and 2 (i & 1) + 1 for units i and i + 64
__device__ __forceinline__ void pg_keyed_mask(uint64_t seed, uint64_t env_id, uint64_t ctr, int lane, bool& keep_a, bool& keep_b) {
    uint32_t r[4];
    mi_philox(seed, env_id, ctr * 32u + (uint64_t)(lane >> 1), MI_PG_STREAM_DROPOUT, r);
    const uint32_t ra = (lane & 1) ? r[2] : r[0], rb = (lane & 1) ? r[3] : r[1];
    keep_a = ra < MI_PG_KEEP_BELOW;
    keep_b = rb < MI_PG_KEEP_BELOW;
}
// the same two bits from 128 stored ones: unit u is bit (u & 31) of word u >> 5
__device__ __forceinline__ void pg_stored_mask(const uint4 m, int lane, bool& keep_a, bool& keep_b) {
    const uint32_t wa = lane < 32 ? m.x : m.y, wb = lane < 32 ? m.z : m.w;
    keep_a = (wa >> (lane & 31)) & 1u;
    keep_b = (wb >> (lane & 31)) & 1u;
}

// sum over the 64 lanes, result in every lane, entirely on the VALU: the DPP row stages of wave_sum, then the four rows by permlane swaps (groups_sum) instead of two
// LDS round trips.  The same balanced pairwise tree over the lanes in natural order (mi_reinforce.h: TREE), so the same bits.
__device__ __forceinline__ float pg_wave_sum(float v) {
    v += dpp_xor1(v);
    v += dpp_xor2(v);
    v += dpp_half_mirror(v);
    v += dpp_mirror(v);
    return groups_sum(v);
}

// forward of one row; DROPOUT = false: eval mode.  ha / hb: this lane's two activations; l0 / l1: the logits in every lane
template <bool DROPOUT>
__device__ __forceinline__ void pg_forward_row(const pg_weights& w, const float4 x, bool keep_a, bool keep_b, float& ha, float& hb, float& l0, float& l1) {
    float za = w.b1a, zb = w.b1b;
    za = __builtin_fmaf(w.w1a[0], x.x, za); zb = __builtin_fmaf(w.w1b[0], x.x, zb);
    za = __builtin_fmaf(w.w1a[1], x.y, za); zb = __builtin_fmaf(w.w1b[1], x.y, zb);
    za = __builtin_fmaf(w.w1a[2], x.z, za); zb = __builtin_fmaf(w.w1b[2], x.z, zb);
    za = __builtin_fmaf(w.w1a[3], x.w, za); zb = __builtin_fmaf(w.w1b[3], x.w, zb);
    if (DROPOUT) {
        ha = keep_a ? fmaxf(za * 2.5f, 0.0f) : 0.0f;
        hb = keep_b ? fmaxf(zb * 2.5f, 0.0f) : 0.0f;
    } else {
        ha = fmaxf(za, 0.0f);
        hb = fmaxf(zb, 0.0f);
    }
    const float q0 = __builtin_fmaf(w.w20b, hb, w.w20a * ha), q1 = __builtin_fmaf(w.w21b, hb, w.w21a * ha);
    l0 = w.b20 + pg_wave_sum(q0);
    l1 = w.b21 + pg_wave_sum(q1);
}
__device__ __forceinline__ void pg_softmax2(float l0, float l1, float& p0, float& p1, float& lp0, float& lp1) {
    const float m = fmaxf(l0, l1);
    const float d0 = l0 - m, d1 = l1 - m;
    const float e0 = mi_fast_exp(d0), e1 = mi_fast_exp(d1);
    const float s = e0 + e1;
    p0 = e0 / s; p1 = e1 / s;
    const float ls = mi_fast_log(s);
    lp0 = d0 - ls; lp1 = d1 - ls;
}

// =====================================================================================================
// episodes
// =====================================================================================================
template <bool FORCED>
__global__ void __launch_bounds__(256) pg_episode_kernel(mi_env e, mi_pg_buffers_t b) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (n >= e.n) return;   // the whole wave
    const pg_weights w = pg_load_weights(b.params, lane);
    const uint64_t env_id = e.env_id_base + (uint64_t)n;
    double s[4];
    if (FORCED && b.forced_reset) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = b.forced_reset[4 * (size_t)n + k];
    } else {
        mi_reset_noise(e.seed, env_id, e.episode[n], s);
    }
    uint64_t ctr = e.step_ctr[n];
    const size_t row0 = (size_t)n * PG_ROWS;
    float4* const obs = reinterpret_cast<float4*>(b.observations) + row0;
    uint4* const mbits = reinterpret_cast<uint4*>(b.mask_bits) + row0;
    int t = 0, done = 0;
    float4 x = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
    uint32_t ur[4];   // the action uniforms' Philox block: one block feeds 4 env-steps (mi_action_uniform), so it is recomputed every 4th step only
    mi_philox(e.seed, env_id, ctr >> 2, STREAM_ACTION, ur);
    while (!done) {
        PG_STAMP(t);
        bool keep_a, keep_b;
        if (FORCED && b.forced_masks) pg_stored_mask(reinterpret_cast<const uint4*>(b.forced_masks)[(size_t)n * PG_T + t], lane, keep_a, keep_b);
        else pg_keyed_mask(e.seed, env_id, ctr, lane, keep_a, keep_b);
        float ha, hb, l0, l1, p0, p1, lp0, lp1;
        pg_forward_row<true>(w, x, keep_a, keep_b, ha, hb, l0, l1);
        pg_softmax2(l0, l1, p0, p1, lp0, lp1);
        const uint32_t sel = (uint32_t)ctr & 3u;
        const float u = mi_u32_to_uniform(sel == 0 ? ur[0] : sel == 1 ? ur[1] : sel == 2 ? ur[2] : ur[3]);
        int a = (u >= p0) ? 1 : 0;
        if (FORCED && b.forced_actions) a = b.forced_actions[(size_t)n * PG_T + t] != 0 ? 1 : 0;
        a = __builtin_amdgcn_readfirstlane(a);
        const unsigned long long ma = __ballot(keep_a), mb = __ballot(keep_b);
        if (lane == 0) {
            obs[t] = x;
            b.actions[row0 + t] = a;
            b.log_probs[row0 + t] = a ? lp1 : lp0;
            mbits[t] = make_uint4((uint32_t)ma, (uint32_t)(ma >> 32), (uint32_t)mb, (uint32_t)(mb >> 32));
        }
        int term;
        mi_cartpole_step(s[0], s[1], s[2], s[3], a, term);
        ++t; ++ctr;
        if (__builtin_amdgcn_readfirstlane((uint32_t)ctr & 3u) == 0) mi_philox(e.seed, env_id, ctr >> 2, STREAM_ACTION, ur);
        done = __builtin_amdgcn_readfirstlane((term || t >= PG_T) ? 1 : 0);
        x = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
    }
    for (int i = t + lane; i < PG_ROWS; i += 64) b.log_probs[row0 + i] = 0.0f;
    if (lane == 0) {
        obs[t] = x;   // the terminal observation
        b.lengths[n] = t;
        b.ep_returns[n] = (float)t;
        e.x[n] = s[0]; e.x_dot[n] = s[1]; e.theta[n] = s[2]; e.theta_dot[n] = s[3];
        e.elapsed[n] = t; e.ep_ret[n] = (float)t; e.ep_len[n] = t;
        e.episode[n] += 1;
        e.step_ctr[n] = ctr;
    }
}

// =====================================================================================================
// returns + per-episode normalisation (one wave per env)
// =====================================================================================================
__global__ void __launch_bounds__(256) pg_returns_kernel(mi_pg_buffers_t b, int n_envs, float gamma) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (n >= n_envs) return;
    int len = b.lengths[n];
    len = len < 0 ? 0 : (len > PG_T ? PG_T : len);
    float* const R = b.returns + (size_t)n * PG_ROWS;
    float* const Rn = b.b_returns + (size_t)n * PG_ROWS;
    // every lane runs the recurrence in registers; the lane that owns row t (t & 63) stores it
    float acc = 0.0f;
    for (int t = len - 1; t >= 0; --t) {
        acc = __builtin_fmaf(gamma, acc, 1.0f);
        if ((t & 63) == lane) R[t] = acc;
    }
    float part = 0.0f;
    for (int t = lane; t < len; t += 64) part += R[t];   // rows this lane stored itself
    const float mean = pg_wave_sum(part) / (float)len;
    float sq = 0.0f;
    for (int t = lane; t < len; t += 64) { const float d = R[t] - mean; sq = __builtin_fmaf(d, d, sq); }
    const float var = pg_wave_sum(sq) / (float)(len - 1);
    const float denom = sqrtf(var) + PG_EXP_M5;
    for (int t = lane; t < len; t += 64) Rn[t] = (R[t] - mean) / denom;
    for (int t = len + lane; t < PG_ROWS; t += 64) { R[t] = 0.0f; Rn[t] = 0.0f; }
}

// =====================================================================================================
// gradient: per-workgroup slabs, then a fixed-order sum (+ Adam)
// =====================================================================================================
__global__ void __launch_bounds__(64 * PG_GRAD_WAVES) pg_grad_kernel(mi_pg_buffers_t b, int n_envs, float* __restrict__ slabs) {
    __shared__ float red[PG_GRAD_WAVES][PG_NP + 2];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const pg_weights w = pg_load_weights(b.params, lane);
    float g1a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g1b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float gb1a = 0.0f, gb1b = 0.0f, g20a = 0.0f, g20b = 0.0f, g21a = 0.0f, g21b = 0.0f, gb20 = 0.0f, gb21 = 0.0f;
    for (int n = blockIdx.x; n < n_envs; n += gridDim.x) {
        int len = b.lengths[n];
        len = len < 0 ? 0 : (len > PG_T ? PG_T : len);   // ragged: only the valid rows of this env are visited
        const size_t row0 = (size_t)n * PG_ROWS;
        // the next row's four loads are in flight while this row is computed (a row is a few hundred cycles of arithmetic behind a memory round trip)
        int t = wv;
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint4 m = make_uint4(0u, 0u, 0u, 0u);
        int a = 0;
        float rn = 0.0f;
        if (t < len) {
            x = reinterpret_cast<const float4*>(b.observations)[row0 + t]; m = reinterpret_cast<const uint4*>(b.mask_bits)[row0 + t];
            a = b.actions[row0 + t]; rn = b.b_returns[row0 + t];
        }
        for (; t < len; t += PG_GRAD_WAVES) {
            const int tn = t + PG_GRAD_WAVES < len ? t + PG_GRAD_WAVES : t;   // the last row re-reads itself: no access behind the episode's end
            const float4 xn = reinterpret_cast<const float4*>(b.observations)[row0 + tn];
            const uint4 mn = reinterpret_cast<const uint4*>(b.mask_bits)[row0 + tn];
            const int an = b.actions[row0 + tn];
            const float rnn = b.b_returns[row0 + tn];
            bool keep_a, keep_b;
            pg_stored_mask(m, lane, keep_a, keep_b);
            float ha, hb, l0, l1, p0, p1, lp0, lp1;
            pg_forward_row<true>(w, x, keep_a, keep_b, ha, hb, l0, l1);
            pg_softmax2(l0, l1, p0, p1, lp0, lp1);
            const float dl0 = rn * (p0 - (a == 0 ? 1.0f : 0.0f)), dl1 = rn * (p1 - (a == 0 ? 0.0f : 1.0f));
            g20a = __builtin_fmaf(dl0, ha, g20a); g20b = __builtin_fmaf(dl0, hb, g20b);
            g21a = __builtin_fmaf(dl1, ha, g21a); g21b = __builtin_fmaf(dl1, hb, g21b);
            gb20 += dl0; gb21 += dl1;
            // h > 0 only where the unit was kept and its pre-activation positive: d h / d z = 2.5 there, 0 elsewhere
            const float dza = ha > 0.0f ? __builtin_fmaf(dl1, w.w21a, dl0 * w.w20a) * 2.5f : 0.0f;
            const float dzb = hb > 0.0f ? __builtin_fmaf(dl1, w.w21b, dl0 * w.w20b) * 2.5f : 0.0f;
            g1a[0] = __builtin_fmaf(dza, x.x, g1a[0]); g1a[1] = __builtin_fmaf(dza, x.y, g1a[1]);
            g1a[2] = __builtin_fmaf(dza, x.z, g1a[2]); g1a[3] = __builtin_fmaf(dza, x.w, g1a[3]);
            g1b[0] = __builtin_fmaf(dzb, x.x, g1b[0]); g1b[1] = __builtin_fmaf(dzb, x.y, g1b[1]);
            g1b[2] = __builtin_fmaf(dzb, x.z, g1b[2]); g1b[3] = __builtin_fmaf(dzb, x.w, g1b[3]);
            gb1a += dza; gb1b += dzb;
            x = xn; m = mn; a = an; rn = rnn;
        }
    }
    float* const r = red[wv];
#pragma unroll
    for (int k = 0; k < 4; ++k) { r[PG_W1 + 4 * lane + k] = g1a[k]; r[PG_W1 + 4 * (lane + 64) + k] = g1b[k]; }
    r[PG_B1 + lane] = gb1a; r[PG_B1 + lane + 64] = gb1b;
    r[PG_W2 + lane] = g20a; r[PG_W2 + lane + 64] = g20b;
    r[PG_W2 + 128 + lane] = g21a; r[PG_W2 + 128 + lane + 64] = g21b;
    if (lane == 0) { r[PG_B2] = gb20; r[PG_B2 + 1] = gb21; }
    __syncthreads();
    for (int i = threadIdx.x; i < PG_NP; i += 64 * PG_GRAD_WAVES) {
        float sum = red[0][i];
#pragma unroll
        for (int k = 1; k < PG_GRAD_WAVES; ++k) sum += red[k][i];
        slabs[(size_t)blockIdx.x * PG_NP + i] = sum;
    }
}

struct pg_adam_consts { float w1, b2, w2, step_size, rbc2, eps; };
// the host-side coefficients exactly as libmirl's mi_adam forms them
static pg_adam_consts pg_adam_host(int64_t step, double lr, double beta1, double beta2, double eps) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    pg_adam_consts k;
    k.w1 = (float)(1.0 - beta1); k.b2 = (float)beta2; k.w2 = (float)(1.0 - beta2);
    k.step_size = (float)(lr / bc1); k.rbc2 = (float)(1.0 / sqrt(bc2)); k.eps = (float)eps;
    return k;
}

// 32 parameters x 16 slab groups per workgroup: thread (j, k) adds the slabs g = k, k + 16, ... of parameter j in ascending g on four interleaved accumulators, the 16
// group sums are then added in ascending k.  (One thread per parameter walking all 1,024 slabs is a chain of 256 dependent memory round trips.)
#define PG_RED_GROUPS 16
__global__ void __launch_bounds__(32 * PG_RED_GROUPS) pg_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float* __restrict__ grads, float* __restrict__ p,
                                                                        float* __restrict__ m, float* __restrict__ v, pg_adam_consts k, int adam) {
    __shared__ float part[PG_RED_GROUPS][32];
    const int j = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + j;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (i < PG_NP) {
        int g = grp;
        for (; g + 3 * PG_RED_GROUPS < n_slabs; g += 4 * PG_RED_GROUPS) {
            s0 += slabs[(size_t)(g + 0 * PG_RED_GROUPS) * PG_NP + i]; s1 += slabs[(size_t)(g + 1 * PG_RED_GROUPS) * PG_NP + i];
            s2 += slabs[(size_t)(g + 2 * PG_RED_GROUPS) * PG_NP + i]; s3 += slabs[(size_t)(g + 3 * PG_RED_GROUPS) * PG_NP + i];
        }
        if (g < n_slabs) s0 += slabs[(size_t)g * PG_NP + i];
        if (g + PG_RED_GROUPS < n_slabs) s1 += slabs[(size_t)(g + PG_RED_GROUPS) * PG_NP + i];
        if (g + 2 * PG_RED_GROUPS < n_slabs) s2 += slabs[(size_t)(g + 2 * PG_RED_GROUPS) * PG_NP + i];
    }
    part[grp][j] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (grp != 0 || i >= PG_NP) return;
    float sum = part[0][j];
#pragma unroll
    for (int q = 1; q < PG_RED_GROUPS; ++q) sum += part[q][j];
    grads[i] = sum;
    if (adam) {
        float mi = m[i], vi = v[i];
        p[i] = mi_adam_elem(p[i], sum, mi, vi, k.w1, k.b2, k.w2, k.step_size, k.rbc2, k.eps);
        m[i] = mi; v[i] = vi;
    }
}

__global__ void __launch_bounds__(256) pg_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int n,
                                                      pg_adam_consts k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float mi = m[i], vi = v[i];
    p[i] = mi_adam_elem(p[i], g[i], mi, vi, k.w1, k.b2, k.w2, k.step_size, k.rbc2, k.eps);
    m[i] = mi; v[i] = vi;
}

__global__ void __launch_bounds__(256) pg_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, const uint32_t* __restrict__ mask_bits,
                                                         float* __restrict__ probs) {
    const int lane = threadIdx.x & 63;
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (row >= n) return;
    const pg_weights w = pg_load_weights(params, lane);
    const float4 x = reinterpret_cast<const float4*>(obs)[row];
    float ha, hb, l0, l1, p0, p1, lp0, lp1;
    if (mask_bits) {
        bool keep_a, keep_b;
        pg_stored_mask(reinterpret_cast<const uint4*>(mask_bits)[row], lane, keep_a, keep_b);
        pg_forward_row<true>(w, x, keep_a, keep_b, ha, hb, l0, l1);
    } else {
        pg_forward_row<false>(w, x, true, true, ha, hb, l0, l1);
    }
    pg_softmax2(l0, l1, p0, p1, lp0, lp1);
    if (lane == 0) { probs[2 * (size_t)row] = p0; probs[2 * (size_t)row + 1] = p1; }
}

// ---- C ABI -------------------------------------------------------------------------------------------
static int pg_check_rollout(const mi_env* e, const mi_pg_buffers_t* b) {
    PG_CHECK_ARG(e != nullptr && b != nullptr, "env / buffers is NULL");
    PG_CHECK_ARG(e->kind == MI_ENV_CARTPOLE_V1 && e->n > 0, "env is not a CartPole-v1 handle");
    PG_CHECK_ARG(b->params && b->observations && b->actions && b->log_probs && b->mask_bits && b->lengths && b->ep_returns, "a rollout buffer is NULL");
    return MI_PG_OK;
}
static int pg_launch_rollout(const mi_env* e, const mi_pg_buffers_t* b, hipStream_t s) {
    const int blocks = (e->n + 3) / 4;
    if (b->forced_reset || b->forced_actions || b->forced_masks) pg_episode_kernel<true><<<blocks, 256, 0, s>>>(*e, *b);
    else pg_episode_kernel<false><<<blocks, 256, 0, s>>>(*e, *b);
    PG_HIP(hipGetLastError());
    return MI_PG_OK;
}
static int pg_launch_returns(const mi_pg_buffers_t* b, int n_envs, float gamma, hipStream_t s) {
    pg_returns_kernel<<<(n_envs + 3) / 4, 256, 0, s>>>(*b, n_envs, gamma);
    PG_HIP(hipGetLastError());
    return MI_PG_OK;
}
static int pg_launch_grad(const mi_pg_buffers_t* b, int n_envs, const pg_adam_consts& k, int adam, hipStream_t s) {
    const int slabs = n_envs < MI_PG_MAX_SLABS ? n_envs : MI_PG_MAX_SLABS;
    pg_grad_kernel<<<slabs, 64 * PG_GRAD_WAVES, 0, s>>>(*b, n_envs, (float*)b->workspace);
    PG_HIP(hipGetLastError());
    pg_reduce_kernel<<<(PG_NP + 31) / 32, 32 * PG_RED_GROUPS, 0, s>>>((const float*)b->workspace, slabs, b->grads, b->params, b->exp_avg, b->exp_avg_sq, k, adam);
    PG_HIP(hipGetLastError());
    return MI_PG_OK;
}
static int pg_check_grad(const mi_pg_buffers_t* b, int n_envs) {
    PG_CHECK_ARG(b != nullptr && n_envs > 0, "buffers is NULL or n_envs <= 0");
    PG_CHECK_ARG(b->params && b->grads && b->observations && b->actions && b->mask_bits && b->b_returns && b->lengths && b->workspace, "a gradient buffer is NULL");
    return MI_PG_OK;
}

extern "C" int mi_pg_forward(const float* params, const float* obs, int n, const uint32_t* mask_bits, float* probs, void* stream) {
    PG_CHECK_ARG(params && obs && probs && n > 0, "bad arguments");
    pg_forward_kernel<<<(n + 3) / 4, 256, 0, (hipStream_t)stream>>>(params, obs, n, mask_bits, probs);
    PG_HIP(hipGetLastError());
    return MI_PG_OK;
}

extern "C" int mi_pg_rollout_episodes(void* env, const mi_pg_buffers_t* b, void* stream) {
    const mi_env* e = (const mi_env*)env;
    const int rc = pg_check_rollout(e, b);
    if (rc != MI_PG_OK) return rc;
    return pg_launch_rollout(e, b, (hipStream_t)stream);
}

extern "C" int mi_pg_returns(const mi_pg_buffers_t* b, int n_envs, float gamma, void* stream) {
    PG_CHECK_ARG(b != nullptr && n_envs > 0, "buffers is NULL or n_envs <= 0");
    PG_CHECK_ARG(b->returns && b->b_returns && b->lengths, "a returns buffer is NULL");
    return pg_launch_returns(b, n_envs, gamma, (hipStream_t)stream);
}

extern "C" int mi_pg_grad(const mi_pg_buffers_t* b, int n_envs, void* stream) {
    const int rc = pg_check_grad(b, n_envs);
    if (rc != MI_PG_OK) return rc;
    return pg_launch_grad(b, n_envs, pg_adam_consts{}, 0, (hipStream_t)stream);
}

extern "C" int mi_pg_adam(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n, int64_t step, double lr, double beta1, double beta2, double eps,
                          void* stream) {
    PG_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && n > 0 && step >= 1, "bad arguments");
    pg_adam_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(params, grads, exp_avg, exp_avg_sq, n, pg_adam_host(step, lr, beta1, beta2, eps));
    PG_HIP(hipGetLastError());
    return MI_PG_OK;
}

extern "C" int mi_pg_update(void* env, const mi_pg_buffers_t* b, const mi_pg_hparams_t* h, void* stream) {
    const mi_env* e = (const mi_env*)env;
    int rc = pg_check_rollout(e, b);
    if (rc != MI_PG_OK) return rc;
    PG_CHECK_ARG(h != nullptr && h->opt_step >= 1, "hparams is NULL or opt_step < 1");
    rc = pg_check_grad(b, e->n);
    if (rc != MI_PG_OK) return rc;
    PG_CHECK_ARG(b->returns && b->exp_avg && b->exp_avg_sq, "a returns / optimizer buffer is NULL");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = pg_launch_rollout(e, b, s)) != MI_PG_OK) return rc;
    if ((rc = pg_launch_returns(b, e->n, h->gamma, s)) != MI_PG_OK) return rc;
    return pg_launch_grad(b, e->n, pg_adam_host(h->opt_step, h->lr, h->beta1, h->beta2, h->eps), 1, s);
}
