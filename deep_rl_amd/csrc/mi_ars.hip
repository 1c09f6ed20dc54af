// mi_ars.hip — libmirl_ars.so: Augmented Random Search on CartPole-v1 for gfx950.  C ABI and numerics contract: include/mi_ars.h.
//
//   ars_episode_kernel<TRAIN>   one LANE per episode, 64-thread workgroups: the lane draws its direction (TRAIN), forms its fp64 policy, and runs its episode from the
//                               keyed reset to the end in registers — the state, the 8 weights, the normaliser and the 9 partial sums.  No LDS, no barrier, no
//                               exchange between lanes; the step loop is a `for` with the bound 500 and a per-lane break, so a wave leaves it when its last lane does.
//   ars_update_kernel           one 1024-thread workgroup: waves 0 .. 14 rank every direction against every other (key and index as one 64-bit number in LDS) and add
//                               the integer sums of the selected returns while wave 15's lanes 0 .. 8 fold the partials serially; then wave 0's lanes 0 .. 7 fold the
//                               step serially while wave 1 forms the normaliser; k + 1.
// Every fp64 operation of the contract is an explicit round-to-nearest intrinsic; the file is built with -ffp-contract=off like the rest.  No atomics on floats, no
// inline assembly.  Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"

#include "../../include/mi_ars.h"

#include <math.h>
#include <stdarg.h>

#define ARS_T MI_ARS_MAX_STEPS
#define ARS_WG 64
#define ARS_UPD_WG 1024
#define ARS_RANK_T (ARS_UPD_WG - 64)   // the threads that rank; the last wave folds the statistics beside them
static_assert(ARS_T == CP_MAX_STEPS, "the TimeLimit of mi_common.h's CartPole-v1");
static_assert(MI_ARS_STREAM == 15 && MI_ARS_NPARAMS == 8 && MI_ARS_NSTATS == 9, "include/mi_ars.h");

// ---- error plumbing (this library's own) --------------------------------------------------------------
static thread_local char ars_err[512] = "";
static void ars_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ars_err, sizeof(ars_err), fmt, ap);
    va_end(ap);
}
#define ARS_CHECK_ARG(cond, msg)                                       \
    do {                                                               \
        if (!(cond)) {                                                 \
            ars_set_error("%s: invalid argument: %s", __func__, msg);  \
            return MI_ARS_EINVAL;                                      \
        }                                                              \
    } while (0)
#define ARS_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            ars_set_error("%s: %s failed: %s", __func__, #call, hipGetErrorString(e_));    \
            return MI_ARS_EHIP;                                                            \
        }                                                                                  \
    } while (0)
static bool ars_aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

#ifndef MI_ARS_SOURCE_ID
#define MI_ARS_SOURCE_ID "unknown"
#endif
extern "C" int mi_ars_version(void) { return MI_ARS_VERSION; }
extern "C" const char* mi_ars_last_error(void) { return ars_err; }
extern "C" const char* mi_ars_source_id(void) { return MI_ARS_SOURCE_ID; }

// libmirl's keyed normal (mi_sac.hip: keyed_normal) on this library's stream
__device__ __forceinline__ float ars_normal(uint64_t seed, uint64_t a, uint64_t b) {
    uint32_t r[4];
    mi_philox(seed, a, b, MI_ARS_STREAM, r);
    const float u1 = ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// =====================================================================================================
// episodes
// =====================================================================================================
template <bool TRAIN>
__global__ void __launch_bounds__(ARS_WG) ars_episode_kernel(mi_ars_args_t a, float* __restrict__ returns, int32_t* __restrict__ lengths, int n_ep) {
    const float4 m0 = reinterpret_cast<const float4*>(a.policy)[0], m1 = reinterpret_cast<const float4*>(a.policy)[1];
    const float M[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
    double mu[4], sc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { mu[j] = a.norm[j]; sc[j] = a.norm[4 + j]; }
    const uint64_t k = TRAIN ? (uint64_t)a.iteration[0] : 0;
    for (int e = blockIdx.x * ARS_WG + threadIdx.x; e < n_ep; e += gridDim.x * ARS_WG) {
        double w[8];
        if (TRAIN) {
            const int i = e >> 1;
            const double sig_nu = (e & 1) ? -(double)a.noise : (double)a.noise;   // sigma * nu: the sign is exact
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float d = ars_normal(a.seed, (uint64_t)i, k * 8 + (uint64_t)c);
                if (!(e & 1)) a.deltas[8 * (size_t)i + c] = d;
                w[c] = __dadd_rn((double)M[c], __dmul_rn(sig_nu, (double)d));
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) w[c] = (double)M[c];
        }
        double y[4];
        mi_reset_noise(a.seed, a.env_id_base + (uint64_t)e, k, y);
        double pn = 0.0, so[4] = {0.0, 0.0, 0.0, 0.0}, soo[4] = {0.0, 0.0, 0.0, 0.0};
        int len = 0, trunc = 0;
        uint8_t* const trace = a.actions ? a.actions + (size_t)e * ARS_T : nullptr;
        for (int t = 0; t < ARS_T; ++t) {
            double x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double o = (double)(float)y[j];
                if (TRAIN) { so[j] = __dadd_rn(so[j], o); soo[j] = __dadd_rn(soo[j], __dmul_rn(o, o)); }
                x[j] = __dmul_rn(__dsub_rn(o, mu[j]), sc[j]);
            }
            if (TRAIN) pn = __dadd_rn(pn, 1.0);
            const double s0 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(w[0], x[0]), __dmul_rn(w[1], x[1])), __dmul_rn(w[2], x[2])), __dmul_rn(w[3], x[3]));
            const double s1 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(w[4], x[0]), __dmul_rn(w[5], x[1])), __dmul_rn(w[6], x[2])), __dmul_rn(w[7], x[3]));
            const int act = s1 > s0 ? 1 : 0;   // a tie and a NaN: action 0
            int term;
            mi_cartpole_step(y[0], y[1], y[2], y[3], act, term);
            len += 1;
            trunc = !term && len >= ARS_T;
            if (trace) trace[t] = (uint8_t)act;
            if (term || trunc) break;   // per lane: the wave goes on while any lane is live
        }
        lengths[e] = len;
        returns[e] = (float)len;
        if (a.truncated) a.truncated[e] = (uint8_t)trunc;
        if (TRAIN) {
            double* const p = a.partials + (size_t)e * MI_ARS_NSTATS;
            p[0] = pn;
#pragma unroll
            for (int j = 0; j < 4; ++j) { p[1 + j] = so[j]; p[5 + j] = soo[j]; }
        }
    }
}

// =====================================================================================================
// update
// =====================================================================================================
// the order of the ranks as one unsigned number: the key's bits made monotonic (returns are not negative, so -0 does not occur) above the index counted downwards —
// comp_j > comp_i exactly when key_j > key_i, or key_j == key_i and j < i
__device__ __forceinline__ unsigned long long ars_comp(float key, int i) {
    const uint32_t u = __float_as_uint(key);
    return ((unsigned long long)(u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u)) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
}

__global__ void __launch_bounds__(ARS_UPD_WG) ars_update_kernel(mi_ars_args_t a, const float* __restrict__ returns) {
    __shared__ ulonglong2 comp2[MI_ARS_MAX_DIRECTIONS / 2];
    __shared__ float dif[MI_ARS_MAX_DIRECTIONS];   // rp_i - rm_i: exact in fp32 for whole numbers up to 500, and (double) of it is the contract's fp64 difference
    __shared__ uint8_t sel[MI_ARS_MAX_DIRECTIONS];
    __shared__ unsigned long long s12[2];
    __shared__ double st[MI_ARS_NSTATS];
    unsigned long long* const comp = reinterpret_cast<unsigned long long*>(comp2);
    const int t = threadIdx.x, N = a.n_directions, b = a.n_top, N2 = (N + 1) >> 1;
    if (t < 2) s12[t] = 0ull;
    for (int i = t; i < 2 * N2; i += ARS_UPD_WG) {
        if (i < N) {
            const float rp = returns[2 * i], rm = returns[2 * i + 1];
            comp[i] = ars_comp(rp > rm ? rp : rm, i);
            dif[i] = rp - rm;
        } else {
            comp[i] = 0ull;   // the pad of an odd N: above nothing
        }
    }
    __syncthreads();
    if (t < ARS_RANK_T) {   // waves 0 .. 14: the ranks and the integer sums of the selected returns
        unsigned long long p1 = 0ull, p2 = 0ull;
        for (int i = t; i < N; i += ARS_RANK_T) {
            const unsigned long long ci = comp[i];
            int rank = 0;
#pragma unroll 4
            for (int j = 0; j < N2; ++j) {
                const ulonglong2 c = comp2[j];
                rank += (c.x > ci ? 1 : 0) + (c.y > ci ? 1 : 0);
            }
            const bool s = rank < b;
            sel[i] = s ? 1 : 0;
            if (s) {
                const long long rp = (long long)(int)returns[2 * i], rm = (long long)(int)returns[2 * i + 1];
                p1 += (unsigned long long)(rp + rm);
                p2 += (unsigned long long)(rp * rp + rm * rm);
            }
        }
        if (p1 | p2) { atomicAdd(&s12[0], p1); atomicAdd(&s12[1], p2); }   // integers: the order does not matter
    } else if (t < ARS_RANK_T + MI_ARS_NSTATS) {   // wave 15, beside the ranks: the partials, onto the old value in ascending e
        const int c = t - ARS_RANK_T;
        double s = a.stats[c];
        const double* const p = a.partials + c;
        const int E = 2 * N;
        // the loads do not depend on the chain: 32 of them are in flight in front of the 32 additions that consume them
#pragma unroll 32
        for (int e = 0; e < E; ++e) s = __dadd_rn(s, p[(size_t)e * MI_ARS_NSTATS]);
        a.stats[c] = s;
        st[c] = s;
    }
    __syncthreads();
    if (t < MI_ARS_NPARAMS) {   // wave 0: the step
        const long long S1 = (long long)s12[0], S2 = (long long)s12[1];
        const long long num = 2ll * b * S2 - S1 * S1;
        if (num != 0) {
            const double sigma = __dsqrt_rn(__ddiv_rn((double)num, (double)(4ll * b * b)));
            double g = 0.0;
            // every delta is loaded, selected or not, so that the loads run ahead of the serial chain; an unselected direction leaves g as it is
#pragma unroll 32
            for (int i = 0; i < N; ++i) {
                const double gn = __dadd_rn(g, __dmul_rn((double)dif[i], (double)a.deltas[8 * (size_t)i + t]));
                g = sel[i] ? gn : g;
            }
            const double coef = __ddiv_rn((double)a.step_size, __dmul_rn((double)b, sigma));
            a.policy[t] = (float)__dadd_rn((double)a.policy[t], __dmul_rn(coef, g));
        }
    } else if (t >= 64 && t < 68 && a.normalize) {   // wave 1, beside the step: the normaliser of the next iteration
        const int j = t - 64;
        const double n = st[0];
        const double m = __ddiv_rn(st[1 + j], n);
        const double v = __dsub_rn(__ddiv_rn(st[5 + j], n), __dmul_rn(m, m));
        const double sd = __dsqrt_rn(v > 0.0 ? v : 0.0);
        a.norm[j] = m;
        a.norm[4 + j] = sd < 1e-7 ? 0.0 : __ddiv_rn(1.0, sd);
    }
    if (t == 128) a.iteration[0] = a.iteration[0] + 1;
}

// ---- C ABI -------------------------------------------------------------------------------------------
static int ars_check_state(const mi_ars_args_t* a, const char* fn) {
    if (!(a->policy && a->stats && a->norm && a->iteration)) { ars_set_error("%s: invalid argument: policy, stats, norm or iteration is NULL", fn); return MI_ARS_EINVAL; }
    if (!(ars_aligned(a->policy, 16) && ars_aligned(a->stats, 16) && ars_aligned(a->norm, 16) && ars_aligned(a->iteration, 16))) {
        ars_set_error("%s: invalid argument: policy, stats, norm and iteration must be 16-byte aligned", fn);
        return MI_ARS_EINVAL;
    }
    return MI_ARS_OK;
}
static int ars_check_train(const mi_ars_args_t* a, const char* fn) {
    const char* msg = nullptr;
    if (a->n_directions < 1 || a->n_directions > MI_ARS_MAX_DIRECTIONS) msg = "n_directions must be 1 .. MI_ARS_MAX_DIRECTIONS";
    else if (a->n_top < 1 || a->n_top > a->n_directions) msg = "n_top must be 1 .. n_directions";
    else if (!(a->noise >= 0.0f) || !isfinite(a->noise)) msg = "noise must be finite and >= 0";
    else if (!isfinite(a->step_size)) msg = "step_size must be finite";
    else if (!a->deltas || !a->partials || !a->returns) msg = "deltas, partials or returns is NULL";
    else if (!ars_aligned(a->deltas, 16) || !ars_aligned(a->partials, 8) || !ars_aligned(a->returns, 4)) msg = "deltas must be 16-byte, partials 8-byte and returns 4-byte aligned";
    if (msg) { ars_set_error("%s: invalid argument: %s", fn, msg); return MI_ARS_EINVAL; }
    return MI_ARS_OK;
}
static int ars_check_episodes(const mi_ars_args_t* a, const char* fn) {
    int rc = ars_check_state(a, fn);
    if (rc) return rc;
    const char* msg = nullptr;
    if (a->n_episodes < 0) msg = "n_episodes must be 0 (training mode) or >= 1";
    else if (a->max_workgroups < 0) msg = "max_workgroups must be 0 (the default) or >= 1";
    else if (!a->returns || !a->lengths) msg = "returns or lengths is NULL";
    else if (!ars_aligned(a->returns, 4) || !ars_aligned(a->lengths, 4)) msg = "returns and lengths must be 4-byte aligned";
    else if (a->n_episodes >= 1 && !(a->noise == 0.0f)) msg = "noise must be 0 in evaluation mode (n_episodes >= 1)";
    if (msg) { ars_set_error("%s: invalid argument: %s", fn, msg); return MI_ARS_EINVAL; }
    return a->n_episodes == 0 ? ars_check_train(a, fn) : MI_ARS_OK;
}

static void ars_launch_episodes(const mi_ars_args_t& a, float* returns, int32_t* lengths, hipStream_t s) {
    const int n_ep = a.n_episodes >= 1 ? a.n_episodes : 2 * a.n_directions;
    const int blocks = (n_ep + ARS_WG - 1) / ARS_WG, cap = a.max_workgroups > 0 ? a.max_workgroups : MI_ARS_DEFAULT_WORKGROUPS;
    const int grid = blocks < cap ? blocks : cap;
    if (a.n_episodes >= 1)
        ars_episode_kernel<false><<<grid, ARS_WG, 0, s>>>(a, returns, lengths, n_ep);
    else
        ars_episode_kernel<true><<<grid, ARS_WG, 0, s>>>(a, returns, lengths, n_ep);
}

extern "C" int mi_ars_episodes(const mi_ars_args_t* a, void* stream) {
    ARS_CHECK_ARG(a != nullptr, "args is NULL");
    const int rc = ars_check_episodes(a, __func__);
    if (rc) return rc;
    ars_launch_episodes(*a, a->returns, a->lengths, (hipStream_t)stream);
    ARS_HIP(hipGetLastError());
    return MI_ARS_OK;
}

extern "C" int mi_ars_update(const mi_ars_args_t* a, void* stream) {
    ARS_CHECK_ARG(a != nullptr, "args is NULL");
    int rc = ars_check_state(a, __func__);
    if (rc) return rc;
    if ((rc = ars_check_train(a, __func__))) return rc;
    ars_update_kernel<<<1, ARS_UPD_WG, 0, (hipStream_t)stream>>>(*a, a->returns);
    ARS_HIP(hipGetLastError());
    return MI_ARS_OK;
}

extern "C" int mi_ars_iterate(const mi_ars_args_t* a, int n_iterations, void* stream) {
    ARS_CHECK_ARG(a != nullptr, "args is NULL");
    ARS_CHECK_ARG(n_iterations >= 1, "n_iterations must be >= 1");
    ARS_CHECK_ARG(a->n_episodes == 0, "n_episodes must be 0: iterations are training mode");
    const int rc = ars_check_episodes(a, __func__);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t row = 2 * (size_t)a->n_directions;
    for (int it = 0; it < n_iterations; ++it) {
        ars_launch_episodes(*a, a->returns + it * row, a->lengths + it * row, s);
        ARS_HIP(hipGetLastError());
        ars_update_kernel<<<1, ARS_UPD_WG, 0, s>>>(*a, a->returns + it * row);
        ARS_HIP(hipGetLastError());
    }
    return MI_ARS_OK;
}
