// mi_c51.hip — libmirl_c51.so: C51 categorical DQN on CartPole-v1 (reference c51.py) for gfx950.  C ABI, numerics and RNG contract: include/mi_c51.h.
//
// One 256-thread workgroup evaluates one network row at a time with the WHOLE network in its registers (112 KB: thread r < 202 holds row r of W3, thread c * 84 + o a
// 40-wide third of row o of W2, thread u < 120 row u of W1), loaded once per launch and kept across everything the workgroup does:
//   c51_act_kernel      a workgroup walks its envs (n = g, g + G, ...), each through all steps of the chunk: weights resident across the steps, fp64 physics in every
//                       thread (same cost as in one), exploring steps skip the forward.
//   c51_grad_kernel     a workgroup walks its batch rows twice: with the TARGET network it writes next_actions / target_probs (softmax, greedy action, categorical
//                       projection per target atom), then with the ONLINE network forward + backward of the same rows into register accumulators — one slab per workgroup.
//   c51_reduce_kernel   fixed-order slab sum (+ Adam).
// The torso (layout, loader, ts_row, ts_backward, ts_store) is mi_torso.h's, shared with mi_qr.hip and mi_ddqn.hip; the host side of acting and of the gradient entry
// points is mi_ring.h's.  All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"

#include "../../include/mi_c51.h"

#define C5_H1 MI_C51_H1
#define C5_H2 MI_C51_H2
#define C5_NA MI_C51_N_ATOMS
#define C5_NL (2 * MI_C51_N_ATOMS)
#define C5_W3 MI_C51_W3
#define C5_B3 MI_C51_B3
#define C5_NP MI_C51_NPARAMS
#define C5_STRIDE MI_C51_SLAB_STRIDE
static_assert(MI_C51_OK == RG_OK && MI_C51_EINVAL == RG_EINVAL && MI_C51_EHIP == RG_EHIP && MI_C51_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_C51_W1 == TS_W1 && MI_C51_B1 == TS_B1 && MI_C51_W2 == TS_W2 && MI_C51_B2 == TS_B2 && MI_C51_H1 == TS_H1 && MI_C51_H2 == TS_H2, "mi_torso.h holds this torso");

#ifndef MI_C51_SOURCE_ID
#define MI_C51_SOURCE_ID "unknown"
#endif
extern "C" int mi_c51_version(void) { return MI_C51_VERSION; }
extern "C" const char* mi_c51_last_error(void) { return rg_err; }
extern "C" const char* mi_c51_source_id(void) { return MI_C51_SOURCE_ID; }
static int c5_slabs(int batch) { return rg_slabs(batch, MI_C51_MAX_SLABS); }
extern "C" size_t mi_c51_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)c5_slabs(batch) * C5_STRIDE * sizeof(float);
}

// ---- the network as one workgroup holds it ------------------------------------------------------------
struct c5_weights {
    float w3[C5_H2]; float b3;          // thread r < 202: row r of W3
    ts_torso ts;
};
struct c5_smem {
    float h1[C5_H1];
    float p2[3][C5_H2];                 // layer 2's partial chains; the backward's partial chains of dh2
    float h2[C5_H2];
    float logit[2][C5_NA + 3];
    float q[2];
    float rowloss;
    float wl[C5_NA], wu[C5_NA];         // the projection's image (l_j, u_j, wl_j, wu_j)
    int li[C5_NA], ui[C5_NA];
    float dl[C5_NA];                    // dlogit of the stored action
    float dz2[C5_H2];
    float ph[2][C5_H1];                 // the backward's partial chains of dh1
};

__device__ __forceinline__ void c5_load_weights(c5_weights& w, const float* __restrict__ P, int t) {
    {
        const int r = t < C5_NL ? t : C5_NL - 1;
        const float4* src = reinterpret_cast<const float4*>(P + C5_W3 + (size_t)r * C5_H2);   // 10,764 and 84 are multiples of 4
#pragma unroll
        for (int k = 0; k < C5_H2 / 4; ++k) { const float4 v = src[k]; w.w3[4 * k] = v.x; w.w3[4 * k + 1] = v.y; w.w3[4 * k + 2] = v.z; w.w3[4 * k + 3] = v.w; }
        w.b3 = P[C5_B3 + r];
    }
    ts_load(w.ts, P, t);
}

// the balanced pairwise sum over the 64 lanes in natural order (mi_c51.h: TREE2's second half), result in every lane, VALU only
__device__ __forceinline__ float c5_wave_sum(float v) {
    v += dpp_xor1(v);
    v += dpp_xor2(v);
    v += dpp_half_mirror(v);
    v += dpp_mirror(v);
    return groups_sum(v);
}
__device__ __forceinline__ float c5_wave_max(float v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = fmaxf(v, __shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ float c5_atom(int j) { return MI_C51_V_MIN + 2.0f * (float)j; }

// layers 1 - 3 of one row: sm.h1, sm.h2, sm.logit are valid for every thread when it returns
__device__ __forceinline__ void c5_forward_row(const c5_weights& w, const float4 x, c5_smem& sm, int t) {
    ts_row(w.ts, x, sm, t);
    if (t < C5_NL) {
        float acc = w.b3;
#pragma unroll
        for (int k = 0; k < C5_H2; ++k) acc = __builtin_fmaf(w.w3[k], sm.h2[k], acc);
        const int a = t >= C5_NA ? 1 : 0;
        sm.logit[a][t - a * C5_NA] = acc;
    }
    __syncthreads();
}

// softmax of action `a`'s logits by ONE wave (all 64 lanes active): lane i gets p_i and p_{i + 64} (0 past atom 100), every lane the action value q.
__device__ __forceinline__ void c5_softmax_wave(const c5_smem& sm, int a, int lane, float& plo, float& phi, float& q) {
    const bool hi = lane + 64 < C5_NA;           // the 101-atom axis does not fill two waves: the tail is masked in the max, the sum and every reduction
    const float llo = sm.logit[a][lane], lhi = hi ? sm.logit[a][lane + 64] : llo;
    const float m = c5_wave_max(fmaxf(llo, lhi));
    const float elo = expf(llo - m), ehi = hi ? expf(lhi - m) : 0.0f;
    const float s = c5_wave_sum(hi ? elo + ehi : elo);
    plo = elo / s;
    phi = hi ? ehi / s : 0.0f;
    q = c5_wave_sum(hi ? __builtin_fmaf(phi, c5_atom(lane + 64), plo * c5_atom(lane)) : plo * c5_atom(lane));
}

// forward + both softmaxes: waves 0 and 1 return their action's distribution; sm.q valid for every thread on return
__device__ __forceinline__ void c5_probs_row(const c5_weights& w, const float4 x, c5_smem& sm, int t, float& plo, float& phi) {
    c5_forward_row(w, x, sm, t);
    const int wv = t >> 6, lane = t & 63;
    plo = 0.0f; phi = 0.0f;
    if (wv < 2) {
        float q;
        c5_softmax_wave(sm, wv, lane, plo, phi, q);
        if (lane == 0) sm.q[wv] = q;
    }
    __syncthreads();
}

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) c51_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, float* __restrict__ probs,
                                                          float* __restrict__ q) {
    __shared__ c5_smem sm;
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    c5_weights w;
    c5_load_weights(w, params, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        float plo, phi;
        c5_probs_row(w, x, sm, t, plo, phi);
        if (wv < 2) {
            if (probs) {
                float* const dst = probs + ((size_t)row * 2 + wv) * C5_NA;
                dst[lane] = plo;
                if (lane + 64 < C5_NA) dst[lane + 64] = phi;
            }
            if (q && lane == 0) q[2 * (size_t)row + wv] = sm.q[wv];
        }
        __syncthreads();
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the whole network is resident in `w`
struct c5_policy {
    const c5_weights& w;
    c5_smem& sm;
    int t;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t, uint64_t) {
        float plo, phi;
        c5_probs_row(w, x, sm, t, plo, phi);
        const int a = sm.q[1] > sm.q[0] ? 1 : 0;   // torch.argmax: the first index on a tie
        __syncthreads();
        return a;
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) c51_act_kernel(mi_env e, const float* __restrict__ params, int n_steps, long long global_step, mi_c51_ring_t ring, rg_eps_tab eps,
                                                      float* __restrict__ obs_cur, const int64_t* __restrict__ forced_actions, const double* __restrict__ forced_resets,
                                                      mi_episode_t* __restrict__ episodes, int32_t* __restrict__ episode_stats, int max_ep) {
    __shared__ c5_smem sm;
    const int t = threadIdx.x;
    c5_weights w;
    c5_load_weights(w, params, t);
    c5_policy policy{w, sm, t};
    const rg_act_args a{obs_cur, forced_actions, forced_resets, episodes, episode_stats, global_step, 0, n_steps, max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// next_actions[b] and target_probs[b][:] of ring row `i` (flat index) from the target network held in `w`
__device__ __forceinline__ void c5_target_row(const c5_weights& w, const mi_c51_ring_t& ring, long long i, float gamma, c5_smem& sm, int t, int32_t* __restrict__ next_action,
                                              float* __restrict__ m_out) {
    const long long N = ring.n_envs, total = ring.slots * N;
    const long long nx = i + N >= total ? i + N - total : i + N;   // ((slot + 1) % slots) * N + env
    const float4 x = reinterpret_cast<const float4*>(ring.observations)[nx];
    const float r = ring.rewards[nx];
    const float live = ring.terminated[nx] ? 0.0f : 1.0f;
    float plo, phi;
    c5_probs_row(w, x, sm, t, plo, phi);
    const int a = sm.q[1] > sm.q[0] ? 1 : 0;
    const int wv = t >> 6, lane = t & 63;
    if (wv == a) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            if (j < C5_NA) {
                const float p = h ? phi : plo;
                const float tz = fminf(fmaxf(r + (gamma * c5_atom(j)) * live, MI_C51_V_MIN), MI_C51_V_MAX);
                const float b = (tz + 100.0f) / 2.0f;
                const float l = floorf(b), u = ceilf(b);
                sm.li[j] = (int)l; sm.ui[j] = (int)u;
                sm.wl[j] = ((u + (l == u ? 1.0f : 0.0f)) - b) * p;
                sm.wu[j] = (b - l) * p;
            }
        }
    }
    __syncthreads();
    if (t < C5_NA) {   // per target atom: the lower contributions in ascending j, then the upper ones (index_add_'s order)
        float m = 0.0f;
        for (int j = 0; j < C5_NA; ++j) if (sm.li[j] == t) m += sm.wl[j];
        for (int j = 0; j < C5_NA; ++j) if (sm.ui[j] == t) m += sm.wu[j];
        m_out[t] = m;
    }
    if (t == 0) *next_action = a;
    __syncthreads();
}

__global__ void __launch_bounds__(256) c51_target_kernel(const float* __restrict__ target_params, mi_c51_ring_t ring, const int64_t* __restrict__ idx, int batch, float gamma,
                                                         int32_t* __restrict__ next_actions, float* __restrict__ target_probs) {
    __shared__ c5_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    c5_weights w;
    c5_load_weights(w, target_params, t);
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        long long i = idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        c5_target_row(w, ring, i, gamma, sm, t, next_actions + b, target_probs + (size_t)b * C5_NA);
    }
}

__global__ void __launch_bounds__(256) c51_grad_kernel(mi_c51_ring_t ring, mi_c51_batch_t bt, float* __restrict__ slabs) {
    __shared__ c5_smem sm;
    const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
    const long long total = ring.slots * (long long)ring.n_envs;
    c5_weights w;
    // ---- pass 1, target network: indices, next_actions, target_probs of this workgroup's rows ----
    c5_load_weights(w, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        c5_target_row(w, ring, i, bt.gamma, sm, t, bt.next_actions + b, bt.target_probs + (size_t)b * C5_NA);
    }
    __threadfence_block();   // pass 2 reads the target_probs this workgroup wrote (c5_target_row ends in a barrier)
    __syncthreads();
    // ---- pass 2, online network: forward + backward into register accumulators ----
    c5_load_weights(w, bt.params, t);
    float g3[C5_H2], gb3 = 0.0f, loss = 0.0f;
    ts_grads g;
#pragma unroll
    for (int k = 0; k < C5_H2; ++k) g3[k] = 0.0f;
    ts_zero(g);
    const float invB = 1.0f / (float)bt.batch;
    const float* __restrict__ P = bt.params;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, false);   // recomputed, not re-read
        const float4 x = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        float plo, phi;
        c5_probs_row(w, x, sm, t, plo, phi);
        if (wv == a) {   // one wave, all lanes active
            const bool hi = lane + 64 < C5_NA;
            const float* const m = bt.target_probs + (size_t)b * C5_NA;
            const float mlo = m[lane], mhi = hi ? m[lane + 64] : 0.0f;
            const float dlo = plo + 1e-8f, dhi = phi + 1e-8f;
            const float tl = mlo * logf(dlo), th = hi ? mhi * logf(dhi) : 0.0f;
            const float rowloss = -c5_wave_sum(hi ? tl + th : tl);
            const float glo = -mlo / dlo, ghi = hi ? -mhi / dhi : 0.0f;
            const float pl = plo * glo, ph = phi * ghi;
            const float S = c5_wave_sum(hi ? pl + ph : pl);
            sm.dl[lane] = (plo * (glo - S)) * invB;
            if (hi) sm.dl[lane + 64] = (phi * (ghi - S)) * invB;
            if (lane == 0) sm.rowloss = rowloss;
            if (bt.probs) {
                float* const dst = bt.probs + (size_t)b * C5_NA;
                dst[lane] = plo;
                if (hi) dst[lane + 64] = phi;
            }
        }
        __syncthreads();
        if (t == 0) loss += sm.rowloss;
        // layer 3: thread r owns row r of dW3
        if (t < C5_NL && (t >= C5_NA ? 1 : 0) == a) {
            const float d = sm.dl[t - a * C5_NA];
            gb3 += d;
#pragma unroll
            for (int k = 0; k < C5_H2; ++k) g3[k] = __builtin_fmaf(d, sm.h2[k], g3[k]);
        }
        // dh2: thread c * 84 + k sums its third of the atoms; W3's column k comes from memory (consecutive threads, consecutive addresses)
        if (t < 3 * C5_H2) {
            const int c = t / C5_H2, k = t - c * C5_H2;
            const int j0 = 34 * c, j1 = j0 + 34 < C5_NA ? j0 + 34 : C5_NA;
            const float* const col = P + C5_W3 + (size_t)(a * C5_NA) * C5_H2 + k;
            float acc = 0.0f;
            for (int j = j0; j < j1; ++j) acc = __builtin_fmaf(sm.dl[j], col[(size_t)j * C5_H2], acc);
            sm.p2[c][k] = acc;
        }
        __syncthreads();
        if (t < C5_H2) sm.dz2[t] = sm.h2[t] > 0.0f ? (sm.p2[0][t] + sm.p2[1][t]) + sm.p2[2][t] : 0.0f;
        __syncthreads();
        ts_backward(g, sm.h1, sm.dz2, sm.ph, x, P, t);
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * C5_STRIDE;
    if (t < C5_NL) {
        float4* const dst = reinterpret_cast<float4*>(slab + C5_W3 + (size_t)t * C5_H2);
#pragma unroll
        for (int k = 0; k < C5_H2 / 4; ++k) dst[k] = make_float4(g3[4 * k], g3[4 * k + 1], g3[4 * k + 2], g3[4 * k + 3]);
        slab[C5_B3 + t] = gb3;
    }
    ts_store(g, slab, t);
    if (t == 0) { slab[C5_NP] = loss; slab[C5_NP + 1] = 0.0f; }
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) c51_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv_batch, float* __restrict__ grads,
                                                                         float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                         rg_adam_consts k, int adam) {
    rg_reduce<C5_NP, C5_STRIDE>(slabs, n_slabs, inv_batch, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_c51_forward(const float* params, const float* obs, int n, float* probs, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && n > 0 && (probs || q), "bad arguments");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    c51_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, n, probs, q);
    RG_HIP(hipGetLastError());
    return MI_C51_OK;
}

extern "C" int mi_c51_act_steps(void* handle, const float* params, int n_steps, int64_t global_step, const mi_c51_ring_t* ring, double start_e, double end_e,
                                double exploration_fraction, int64_t total_timesteps, float* obs_cur, const int64_t* forced_actions, const double* forced_resets,
                                mi_episode_t* episodes, int32_t* episode_stats, int max_ep, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    RG_CHECK_ARG(e != nullptr && params && obs_cur, "NULL pointer");
    RG_CHECK_ARG(global_step >= 0 && total_timesteps > 0 && exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, global_step, (end_e - start_e) / (exploration_fraction * (double)total_timesteps), start_e, end_e);
    int grid;
    const int rc = rg_act_prelude(e, ring, params, obs_cur, n_steps, max_ep, episodes, episode_stats, s, grid);
    if (rc != MI_C51_OK) return rc;
    if (forced_actions || forced_resets)
        c51_act_kernel<true><<<grid, 256, 0, s>>>(*e, params, n_steps, (long long)global_step, *ring, tab, obs_cur, forced_actions, forced_resets, episodes, episode_stats, max_ep);
    else
        c51_act_kernel<false><<<grid, 256, 0, s>>>(*e, params, n_steps, (long long)global_step, *ring, tab, obs_cur, nullptr, nullptr, episodes, episode_stats, max_ep);
    RG_HIP(hipGetLastError());
    return MI_C51_OK;
}

extern "C" int mi_c51_target(const float* target_params, const mi_c51_ring_t* ring, const int64_t* idx, int batch, float gamma, int32_t* next_actions, float* target_probs,
                             void* stream) {
    RG_CHECK_ARG(target_params && idx && next_actions && target_probs && batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(target_params), "target_params must be 16-byte aligned");
    const int rc = rg_check_ring(ring);
    if (rc != MI_C51_OK) return rc;
    c51_target_kernel<<<batch < 1024 ? batch : 1024, 256, 0, (hipStream_t)stream>>>(target_params, *ring, idx, batch, gamma, next_actions, target_probs);
    RG_HIP(hipGetLastError());
    return MI_C51_OK;
}

// mi_c51_grad (update false: opt is not looked at) and mi_c51_update
static int c5_grad(const mi_c51_ring_t* ring, const mi_c51_batch_t* b, const mi_c51_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_c51_batch_t& bt) { return bt.target_probs != nullptr; });
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<C5_NP>(c51_grad_kernel, c51_reduce_kernel, ring, b, c5_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_c51_grad(const mi_c51_ring_t* ring, const mi_c51_batch_t* b, void* stream) { return c5_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_c51_update(const mi_c51_ring_t* ring, const mi_c51_batch_t* b, const mi_c51_adam_t* opt, void* stream) {
    return c5_grad(ring, b, opt, true, (hipStream_t)stream);
}
