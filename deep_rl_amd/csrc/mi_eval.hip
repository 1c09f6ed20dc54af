// mi_eval.hip — libmirl_eval.so: greedy policy evaluation on CartPole-v1 for gfx950.  C ABI and numerics contract: include/mi_eval.h.
//
// One 256-thread workgroup runs one episode at a time, from its keyed reset to its end, with the network resident across all the episodes it owns:
//   the torso      mi_torso.h's register layout (thread c * 84 + o a 40-wide third of row o of W2, thread u < 120 row u of W1), as it is;
//   the head       held as the owning library's acting launch holds it: DUELING (mi_pdd.hip) in LDS in parameter order, every thread forming
//                  both action values from workgroup-uniform broadcasts; QR (mi_qr.hip) collapsed once per workgroup and kept in every thread's registers; C51
//                  (mi_c51.hip) thread r < 202 row r of W3 in registers, one wave per action for the softmax; RAINBOW (mi_rainbow.hip, the mean network) thread
//                  r < 153 head row r in registers, the dueling combine and the softmax by one wave per action;
//   the env        the fp64 state lives in thread 0's registers alone.  Thread 0 takes the step and publishes the next observation and the done flag through LDS;
//                  one barrier per step hands them to the workgroup (the torso's three publish everything else).
//   ev_episode_kernel<KIND, FORCED>   workgroup g runs episodes g, g + G, ...; the step loop is a `for` with the bound 500 and a workgroup-uniform break.
//   ev_forward_kernel<KIND>           the action values of n observations through the same ev_net<KIND>::values.
// The expressions of every head are copies of the owning library's (their sources are pinned by their ids; sharing them is a change to those libraries of its own).
// All arithmetic on the VALU in fp32 with the orders of the header; no atomics, no inline assembly.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_torso.h"

#include "../../include/mi_eval.h"

#include <math.h>
#include <stdarg.h>

#define EV_H1 TS_H1
#define EV_H2 TS_H2
#define EV_HEAD (TS_B2 + TS_H2)               // 10,764: where every head starts
#define EV_T MI_EV_MAX_STEPS
static_assert(EV_T == CP_MAX_STEPS, "the TimeLimit of mi_common.h's CartPole-v1");
static_assert(EV_HEAD == 10764 && EV_HEAD % 4 == 0, "the head behind the torso");
// DUELING: Wv [84], bv, Wa [2][84], ba [2]
#define EV_DU_N 255
#define EV_DU_BV EV_H2
#define EV_DU_WA (EV_H2 + 1)
#define EV_DU_BA (EV_DU_WA + 2 * EV_H2)
static_assert(MI_EV_NPARAMS_DUELING == EV_HEAD + EV_DU_N && EV_DU_BA + 2 == EV_DU_N, "mi_pdd.h's layout");
// QR: W3 [128][84], b3 [128]
#define EV_QR_NQ MI_EV_QR_QUANT
#define EV_QR_B3 (EV_HEAD + 2 * EV_QR_NQ * EV_H2)
static_assert(MI_EV_NPARAMS_QR == EV_QR_B3 + 2 * EV_QR_NQ && EV_QR_NQ == 64, "mi_qr.h's layout");
// C51: W3 [202][84], b3 [202]
#define EV_C5_NA MI_EV_C51_ATOMS
#define EV_C5_NL (2 * EV_C5_NA)
#define EV_C5_B3 (EV_HEAD + EV_C5_NL * EV_H2)
static_assert(MI_EV_NPARAMS_C51 == EV_C5_B3 + EV_C5_NL && EV_C5_NL <= 256 && EV_C5_NA <= 128, "mi_c51.h's layout; one W3 row per thread, two atoms per lane");
// RAINBOW (means): Wv [51][84], bv [51], Wa [2][51][84], ba [2][51]
#define EV_RB_NA MI_EV_RAINBOW_ATOMS
#define EV_RB_NR (3 * EV_RB_NA)
#define EV_RB_BV (EV_RB_NA * EV_H2)
#define EV_RB_WA (EV_RB_BV + EV_RB_NA)
#define EV_RB_BA (EV_RB_WA + 2 * EV_RB_NA * EV_H2)
static_assert(MI_EV_NPARAMS_RAINBOW == EV_HEAD + EV_RB_BA + 2 * EV_RB_NA && EV_RB_NR <= 256 && EV_RB_NA <= 64, "mi_rainbow.h's layout; one head row per thread, one atom per lane");

// ---- error plumbing (this library's own: it does not include mi_ring.h) ------------------------------
static thread_local char ev_err[512] = "";
static void ev_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ev_err, sizeof(ev_err), fmt, ap);
    va_end(ap);
}
#define EV_CHECK_ARG(cond, msg)                                       \
    do {                                                              \
        if (!(cond)) {                                                \
            ev_set_error("%s: invalid argument: %s", __func__, msg);  \
            return MI_EV_EINVAL;                                      \
        }                                                             \
    } while (0)
#define EV_HIP(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            ev_set_error("%s: %s failed: %s", __func__, #call, hipGetErrorString(e_));    \
            return MI_EV_EHIP;                                                            \
        }                                                                                 \
    } while (0)
static bool ev_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

#ifndef MI_EV_SOURCE_ID
#define MI_EV_SOURCE_ID "unknown"
#endif
extern "C" int mi_ev_version(void) { return MI_EV_VERSION; }
extern "C" const char* mi_ev_last_error(void) { return ev_err; }
extern "C" const char* mi_ev_source_id(void) { return MI_EV_SOURCE_ID; }

// ---- the network as one workgroup holds it ------------------------------------------------------------
struct ev_smem {
    float h1[EV_H1];
    float p2[3][EV_H2];                 // layer 2's partial chains
    float h2[EV_H2];
    float hd[256];                      // DUELING: the head in parameter order
    float wbar[2][EV_H2];               // QR: the collapsed head on its way into the registers
    float bbar[2];
    float y[2 * (EV_C5_NA + 3)];        // C51: logit[a][j] at a * 104 + j; RAINBOW: the 153 head rows' outputs
    float q[2];                         // C51 / RAINBOW: the two action values
    float4 x;                           // the env's hand-off: the observation of the step to come ...
    int done;                           // ... and whether the step just taken ended the episode
};
struct ev_support { float v_min, v_max, dz; };

// the balanced pairwise sum over the 64 lanes in natural order, result in every lane, VALU only (mi_c51.hip's c5_wave_sum)
__device__ __forceinline__ float ev_wave_sum(float v) {
    v += dpp_xor1(v);
    v += dpp_xor2(v);
    v += dpp_half_mirror(v);
    v += dpp_mirror(v);
    return groups_sum(v);
}
__device__ __forceinline__ float ev_wave_max(float v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ float ev_atom(const ev_support& z, int j) { return z.v_min + z.dz * (float)j; }   // a product, then a sum

// ev_net<KIND>: load() once per workgroup (it ends in a barrier where the head goes through LDS); values() of the row in sm.h2 — called by the whole workgroup behind
// ts_row — gives both action values to every thread.  Behind values() sm.h2 / sm.y / sm.q are next written behind at least two barriers of the next ts_row.
template <int KIND> struct ev_net;

template <> struct ev_net<MI_EV_DUELING> {   // mi_dueling.h: du_load_head, du_values
    __device__ __forceinline__ void load(const float* __restrict__ P, ev_smem& sm, const ev_support&, int t) {
        if (t < EV_DU_N) sm.hd[t] = P[EV_HEAD + t];
        __syncthreads();
    }
    __device__ __forceinline__ void values(ev_smem& sm, int, float& q0, float& q1) const {
        const float* const hd = sm.hd;
        float v = hd[EV_DU_BV], a0 = hd[EV_DU_BA], a1 = hd[EV_DU_BA + 1];
#pragma unroll
        for (int k = 0; k < EV_H2; ++k) {
            const float h = sm.h2[k];
            v = __builtin_fmaf(hd[k], h, v);
            a0 = __builtin_fmaf(hd[EV_DU_WA + k], h, a0);
            a1 = __builtin_fmaf(hd[EV_DU_WA + EV_H2 + k], h, a1);
        }
        const float m = (a0 + a1) * 0.5f;
        q0 = v + (a0 - m);
        q1 = v + (a1 - m);
    }
};

template <> struct ev_net<MI_EV_QR> {   // mi_qr.hip: qr_collapse, qr_policy (the collapsed head in every thread's registers)
    float wb0[EV_H2], wb1[EV_H2], bb0, bb1;
    __device__ __forceinline__ void load(const float* __restrict__ P, ev_smem& sm, const ev_support&, int t) {
        if (t < 2 * EV_H2) {   // thread a * 84 + k: column k of action a's 64 rows
            const int a = t / EV_H2, k = t - a * EV_H2;
            const float* const col = P + EV_HEAD + (size_t)(a * EV_QR_NQ) * EV_H2 + k;
            float s = 0.0f;
#pragma unroll 16
            for (int i = 0; i < EV_QR_NQ; ++i) s = s + col[(size_t)i * EV_H2];
            sm.wbar[a][k] = s * (1.0f / 64.0f);
        } else if (t < 2 * EV_H2 + 2) {
            const int a = t - 2 * EV_H2;
            float s = 0.0f;
#pragma unroll 16
            for (int i = 0; i < EV_QR_NQ; ++i) s = s + P[EV_QR_B3 + a * EV_QR_NQ + i];
            sm.bbar[a] = s * (1.0f / 64.0f);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < EV_H2; ++k) { wb0[k] = sm.wbar[0][k]; wb1[k] = sm.wbar[1][k]; }
        bb0 = sm.bbar[0]; bb1 = sm.bbar[1];
    }
    __device__ __forceinline__ void values(ev_smem& sm, int, float& q0, float& q1) const {
        q0 = bb0; q1 = bb1;
#pragma unroll
        for (int k = 0; k < EV_H2; ++k) {
            const float h = sm.h2[k];
            q0 = __builtin_fmaf(wb0[k], h, q0);
            q1 = __builtin_fmaf(wb1[k], h, q1);
        }
    }
};

template <> struct ev_net<MI_EV_C51> {   // mi_c51.hip: c5_load_weights, c5_forward_row, c5_softmax_wave, c5_probs_row
    float w3[EV_H2], b3;
    ev_support z;
    __device__ __forceinline__ void load(const float* __restrict__ P, ev_smem&, const ev_support& z_, int t) {
        const int r = t < EV_C5_NL ? t : EV_C5_NL - 1;
        const float4* src = reinterpret_cast<const float4*>(P + EV_HEAD + (size_t)r * EV_H2);   // 10,764 and 84 are multiples of 4
#pragma unroll
        for (int k = 0; k < EV_H2 / 4; ++k) { const float4 v = src[k]; w3[4 * k] = v.x; w3[4 * k + 1] = v.y; w3[4 * k + 2] = v.z; w3[4 * k + 3] = v.w; }
        b3 = P[EV_C5_B3 + r];
        z = z_;
    }
    __device__ __forceinline__ void values(ev_smem& sm, int t, float& q0, float& q1) const {
        if (t < EV_C5_NL) {
            float acc = b3;
#pragma unroll
            for (int k = 0; k < EV_H2; ++k) acc = __builtin_fmaf(w3[k], sm.h2[k], acc);
            const int a = t >= EV_C5_NA ? 1 : 0;
            sm.y[a * (EV_C5_NA + 3) + t - a * EV_C5_NA] = acc;
        }
        __syncthreads();
        const int wv = t >> 6, lane = t & 63;
        if (wv < 2) {   // one wave per action, all 64 lanes active: lane i holds atoms i and i + 64, the tail masked in the max, the sum and every reduction
            const float* const logit = sm.y + wv * (EV_C5_NA + 3);
            const bool hi = lane + 64 < EV_C5_NA;
            const float llo = logit[lane], lhi = hi ? logit[lane + 64] : llo;
            const float m = ev_wave_max(fmaxf(llo, lhi));
            const float elo = expf(llo - m), ehi = hi ? expf(lhi - m) : 0.0f;
            const float s = ev_wave_sum(hi ? elo + ehi : elo);
            const float plo = elo / s;
            const float phi = hi ? ehi / s : 0.0f;
            const float q = ev_wave_sum(hi ? __builtin_fmaf(phi, ev_atom(z, lane + 64), plo * ev_atom(z, lane)) : plo * ev_atom(z, lane));
            if (lane == 0) sm.q[wv] = q;
        }
        __syncthreads();
        q0 = sm.q[0]; q1 = sm.q[1];
    }
};

template <> struct ev_net<MI_EV_RAINBOW> {   // mi_rainbow.hip with noisy == 0: rb_policy<false>, rb_softmax
    float mu[EV_H2], bmu;
    ev_support z;
    __device__ __forceinline__ void load(const float* __restrict__ P, ev_smem&, const ev_support& z_, int t) {
        const int r = t < EV_RB_NR ? t : EV_RB_NR - 1;
        // (the advantage rows start at an odd offset: read element by element, once per workgroup)
        const float* const src = P + EV_HEAD + (r < EV_RB_NA ? r * EV_H2 : EV_RB_WA + (r - EV_RB_NA) * EV_H2);
#pragma unroll
        for (int k = 0; k < EV_H2; ++k) mu[k] = src[k];
        bmu = P[EV_HEAD + (r < EV_RB_NA ? EV_RB_BV + r : EV_RB_BA + (r - EV_RB_NA))];
        z = z_;
    }
    __device__ __forceinline__ void values(ev_smem& sm, int t, float& q0, float& q1) const {
        if (t < EV_RB_NR) {
            float acc = bmu;
#pragma unroll
            for (int k = 0; k < EV_H2; ++k) acc = __builtin_fmaf(mu[k], sm.h2[k], acc);
            sm.y[t] = acc;
        }
        __syncthreads();
        const int wv = t >> 6, lane = t & 63;
        if (wv < 2) {
            const bool valid = lane < EV_RB_NA;
            const int j = valid ? lane : EV_RB_NA - 1;   // the tail repeats atom 50 in the max and is 0 in every sum
            const float v = sm.y[j], a0 = sm.y[EV_RB_NA + j], a1 = sm.y[2 * EV_RB_NA + j];
            const float l = v + ((wv ? a1 : a0) - 0.5f * (a0 + a1));
            const float m = ev_wave_max(l);
            const float e = valid ? expf(l - m) : 0.0f;
            const float s = ev_wave_sum(e);
            const float p = e / s;
            const float q = ev_wave_sum(p * ev_atom(z, lane));
            if (lane == 0) sm.q[wv] = q;
        }
        __syncthreads();
        q0 = sm.q[0]; q1 = sm.q[1];
    }
};

__device__ __forceinline__ ev_support ev_make_support(int kind, float v_min, float v_max) {
    return ev_support{v_min, v_max, (v_max - v_min) / (float)((kind == MI_EV_C51 ? EV_C5_NA : EV_RB_NA) - 1)};
}

// =====================================================================================================
// forward API
// =====================================================================================================
template <int KIND>
__global__ void __launch_bounds__(256) ev_forward_kernel(const float* __restrict__ params, float v_min, float v_max, const float* __restrict__ obs, int n,
                                                         float* __restrict__ q) {
    __shared__ ev_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, params, t);
    ev_net<KIND> net;
    net.load(params, sm, ev_make_support(KIND, v_min, v_max), t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        ts_row(w, x, sm, t);
        float q0, q1;
        net.values(sm, t, q0, q1);
        if (t == 0) { q[2 * (size_t)row] = q0; q[2 * (size_t)row + 1] = q1; }
    }
}

// =====================================================================================================
// episodes
// =====================================================================================================
template <int KIND, bool FORCED>
__global__ void __launch_bounds__(256) ev_episode_kernel(mi_ev_args_t a) {
    __shared__ ev_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, a.params, t);
    ev_net<KIND> net;
    net.load(a.params, sm, ev_make_support(KIND, a.v_min, a.v_max), t);
    for (int e = blockIdx.x; e < a.n_episodes; e += gridDim.x) {
        // the env's state is thread 0's alone (the other threads carry dead copies)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (t == 0) {
            double rs[4];
            if (FORCED && a.forced_starts) {
#pragma unroll
                for (int k = 0; k < 4; ++k) rs[k] = a.forced_starts[4 * (size_t)e + k];
            } else {
                mi_reset_noise(a.seed, a.env_id_base + (uint64_t)e, 0, rs);
            }
            s0 = rs[0]; s1 = rs[1]; s2 = rs[2]; s3 = rs[3];
            // the last readers of sm.x (the previous episode's last step) are four barriers back
            sm.x = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
        }
        __syncthreads();
        int len = 0, trunc = 0;
        float ret = 0.0f, mg = __builtin_inff();
        const uint8_t* const forced = FORCED && a.forced_actions ? a.forced_actions + (size_t)e * EV_T : nullptr;
        uint8_t* const trace = a.actions ? a.actions + (size_t)e * EV_T : nullptr;
        for (int s = 0; s < EV_T; ++s) {
            const float4 x = sm.x;
            ts_row(w, x, sm, t);
            float q0, q1;
            net.values(sm, t, q0, q1);
            if (t == 0) {
                const float gap = fabsf(q1 - q0);
                mg = gap < mg ? gap : mg;
                int act = q1 > q0 ? 1 : 0;   // torch.argmax: the first index on a tie; a NaN compares false
                if (FORCED && forced) act = forced[s] != 0 ? 1 : 0;
                int term;
                mi_cartpole_step(s0, s1, s2, s3, act, term);
                len += 1; ret += 1.0f;
                trunc = !term && len >= EV_T;
                if (trace) trace[s] = (uint8_t)act;
                // every thread read sm.x and the previous sm.done before this step's first barrier
                sm.x = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
                sm.done = term || trunc;
            }
            __syncthreads();
            if (sm.done) break;   // workgroup-uniform
        }
        if (t == 0) {
            a.lengths[e] = len;
            if (a.returns) a.returns[e] = ret;
            if (a.truncated) a.truncated[e] = (uint8_t)trunc;
            if (a.min_gap) a.min_gap[e] = mg;
        }
    }
}

// ---- C ABI -------------------------------------------------------------------------------------------
static bool ev_categorical(int kind) { return kind == MI_EV_C51 || kind == MI_EV_RAINBOW; }
static bool ev_support_ok(float v_min, float v_max) { return isfinite(v_min) && isfinite(v_max) && v_min < v_max && isfinite(v_max - v_min); }

extern "C" int mi_ev_forward(const float* params, int kind, float v_min, float v_max, const float* obs, int n, float* q, void* stream) {
    EV_CHECK_ARG(params && obs && n > 0 && q, "bad arguments");
    EV_CHECK_ARG(kind >= MI_EV_DUELING && kind <= MI_EV_RAINBOW, "kind must be MI_EV_DUELING .. MI_EV_RAINBOW");
    EV_CHECK_ARG(ev_aligned(params) && ev_aligned(obs), "params and obs must be 16-byte aligned");
    EV_CHECK_ARG(!ev_categorical(kind) || ev_support_ok(v_min, v_max), "the support needs finite v_min < v_max");
    const int grid = n < 1024 ? n : 1024;
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case MI_EV_DUELING: ev_forward_kernel<MI_EV_DUELING><<<grid, 256, 0, s>>>(params, v_min, v_max, obs, n, q); break;
        case MI_EV_QR: ev_forward_kernel<MI_EV_QR><<<grid, 256, 0, s>>>(params, v_min, v_max, obs, n, q); break;
        case MI_EV_C51: ev_forward_kernel<MI_EV_C51><<<grid, 256, 0, s>>>(params, v_min, v_max, obs, n, q); break;
        default: ev_forward_kernel<MI_EV_RAINBOW><<<grid, 256, 0, s>>>(params, v_min, v_max, obs, n, q); break;
    }
    EV_HIP(hipGetLastError());
    return MI_EV_OK;
}

template <int KIND>
static void ev_launch(const mi_ev_args_t& a, int grid, bool forced, hipStream_t s) {
    if (forced)
        ev_episode_kernel<KIND, true><<<grid, 256, 0, s>>>(a);
    else
        ev_episode_kernel<KIND, false><<<grid, 256, 0, s>>>(a);
}

extern "C" int mi_ev_episodes(const mi_ev_args_t* a, void* stream) {
    EV_CHECK_ARG(a != nullptr, "args is NULL");
    EV_CHECK_ARG(a->params != nullptr && a->lengths != nullptr, "params or lengths is NULL");
    EV_CHECK_ARG(ev_aligned(a->params), "params must be 16-byte aligned");
    EV_CHECK_ARG(a->kind >= MI_EV_DUELING && a->kind <= MI_EV_RAINBOW, "kind must be MI_EV_DUELING .. MI_EV_RAINBOW");
    EV_CHECK_ARG(a->n_episodes >= 1, "n_episodes must be >= 1");
    EV_CHECK_ARG(a->max_workgroups >= 0, "max_workgroups must be 0 (the default) or >= 1");
    EV_CHECK_ARG(!a->forced_starts || ((uintptr_t)a->forced_starts & 7u) == 0, "forced_starts must be 8-byte aligned");
    EV_CHECK_ARG(((uintptr_t)a->lengths & 3u) == 0 && ((uintptr_t)a->returns & 3u) == 0 && ((uintptr_t)a->min_gap & 3u) == 0, "lengths, returns and min_gap must be 4-byte aligned");
    EV_CHECK_ARG(!ev_categorical(a->kind) || ev_support_ok(a->v_min, a->v_max), "the support needs finite v_min < v_max");
    const int cap = a->max_workgroups > 0 ? a->max_workgroups : MI_EV_DEFAULT_WORKGROUPS;
    const int grid = a->n_episodes < cap ? a->n_episodes : cap;
    const bool forced = a->forced_actions || a->forced_starts;
    hipStream_t s = (hipStream_t)stream;
    switch (a->kind) {
        case MI_EV_DUELING: ev_launch<MI_EV_DUELING>(*a, grid, forced, s); break;
        case MI_EV_QR: ev_launch<MI_EV_QR>(*a, grid, forced, s); break;
        case MI_EV_C51: ev_launch<MI_EV_C51>(*a, grid, forced, s); break;
        default: ev_launch<MI_EV_RAINBOW>(*a, grid, forced, s); break;
    }
    EV_HIP(hipGetLastError());
    return MI_EV_OK;
}
