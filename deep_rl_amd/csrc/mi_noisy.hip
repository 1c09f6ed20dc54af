// mi_noisy.hip — libmirl_noisy.so: noisy-net exploration on n-step prioritized dueling Double DQN on CartPole-v1 for gfx950.  C ABI, numerics and RNG contract:
// include/mi_noisy.h (and include/mi_nstep.h / include/mi_pdd.h, which it refers to for everything but the noise).
//
// The form of mi_nstep.hip and mi_pdd.hip: one 256-thread workgroup evaluates one row at a time with the torso(s) in its registers and the 255-element dueling
// head(s) in LDS, one element per thread.  The noise sits where a thread already owns its element: thread t < 255 derives THAT element's eps itself (at most two
// Philox calls and two Box-Muller values; the output factors are recomputed redundantly across threads) and writes mu_t + sigma_t * eps_t into sm.hd, so forming the
// effective head needs no LDS exchange and no barrier of its own — the torso's three barriers publish it as they publish a loaded head.
//   nz_act_kernel      rg_act_loop as it is, instantiated with and without the noise (without it the kernel is pdd_act_kernel).  policy.greedy forms a fresh head
//                      per greedy env step ahead of du_torso_rows.  The acting launch uses only the online network, so the two copies sm.hd[0] / sm.hd[1] ALTERNATE between greedy steps: step k writes the copy step k - 2 read, and every wave has
//                      left step k - 2's du_values before any passes the three barriers of step k - 1.  No barrier is added.
//   nz_forward_kernel  the action values of n observations under one sample, or the mean network.
//   nz_target_kernel   pass 1 alone; both heads formed once per launch.
//   nz_grad_kernel     ns_grad_kernel with both heads formed once per launch; eps_t waits in LDS (a word per thread, read by its writer: no barrier) for the slab
//                      store, where slab[SIGMA + t] = gh * eps_t.
//   nz_reduce_kernel   fixed-order slab sum (+ Adam) over 11,274 elements.
//   nz_noise_kernel    one sample written out as the kernels form it (the tests' view of the draw).
// The dueling head in LDS, the three-evaluation torso rows, the action values, the gradient row, the slab epilogue and the walk's hand-off are mi_dueling.h's,
// shared with mi_pdd.hip and mi_nstep.hip; this library forms the head it puts there and adds the sigma half of the slab.  nz_normal is a copy of mi_sac.hip's
// keyed_normal expression with the stream as an argument (that file cannot be included).
// All arithmetic on the VALU in fp32; no floating-point atomics, no inline assembly, no device-wide hand-off inside a launch.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"
#include "mi_nwalk.h"
#include "mi_dueling.h"

#include "../../include/mi_noisy.h"

#define PD_SIGMA MI_NZ_SIGMA                  // the head's first sigma (its first mean is DU_HEAD)
#define PD_NP MI_NZ_NPARAMS
#define PD_STRIDE MI_NZ_SLAB_STRIDE
static_assert(MI_NZ_OK == RG_OK && MI_NZ_EINVAL == RG_EINVAL && MI_NZ_EHIP == RG_EHIP && MI_NZ_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_NZ_W1 == TS_W1 && MI_NZ_B1 == TS_B1 && MI_NZ_W2 == TS_W2 && MI_NZ_B2 == TS_B2 && MI_NZ_H1 == TS_H1 && MI_NZ_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_NZ_WV == DU_HEAD + DU_WV && MI_NZ_BV == DU_HEAD + DU_BV && MI_NZ_WA == DU_HEAD + DU_WA && MI_NZ_BA == DU_HEAD + DU_BA && MI_NZ_NHEAD == DU_NHEAD,
              "mi_dueling.h holds this head");
static_assert(PD_SIGMA == DU_HEAD + DU_NHEAD && PD_NP == PD_SIGMA + DU_NHEAD, "mu and then sigma");
static_assert(MI_NZ_NXI == 2 * TS_H2 + 3 && MI_NZ_NXI <= 256, "84 + 1 value factors, 84 + 2 advantage factors; b * 256 + c keys them");
static_assert(PD_STRIDE % 4 == 0 && PD_STRIDE > PD_NP, "float4 stores");
static_assert(MI_NZ_MAX_N == NW_MAX_N, "mi_nwalk.h walks this far");
static_assert(MI_NZ_STREAM_ACT < 16 && MI_NZ_STREAM_LEARN < 16, "the stream tag has 4 bits");

#ifndef MI_NZ_SOURCE_ID
#define MI_NZ_SOURCE_ID "unknown"
#endif
extern "C" int mi_nz_version(void) { return MI_NZ_VERSION; }
extern "C" const char* mi_nz_last_error(void) { return rg_err; }
extern "C" const char* mi_nz_source_id(void) { return MI_NZ_SOURCE_ID; }
static int nz_slabs(int batch) { return rg_slabs(batch, MI_NZ_MAX_SLABS); }
extern "C" size_t mi_nz_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)nz_slabs(batch) * PD_STRIDE * sizeof(float);
}

// ---- the noise ----------------------------------------------------------------------------------------
struct nz_key { uint64_t seed, a, b; uint32_t stream; };
// z_c of the sample `k`: mi_sac.hip's keyed_normal expression
__device__ __forceinline__ float nz_normal(const nz_key& k, int c) {
    uint32_t r[4];
    mi_philox(k.seed, k.a, k.b * 256ull + (uint64_t)c, k.stream, r);
    const float u1 = ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)(r[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}
// xi_c = sgn(z) * sqrtf(|z|)
__device__ __forceinline__ float nz_xi(const nz_key& k, int c) {
    const float z = nz_normal(k, c);
    const float s = sqrtf(fabsf(z));
    return z > 0.0f ? s : (z < 0.0f ? -s : 0.0f);
}
// eps of head element t < 255: the output factor, times the input factor for a weight
__device__ __forceinline__ float nz_eps(const nz_key& k, int t) {
    int co, ci;   // the factors' indices; ci < 0: a bias
    if (t < DU_BV) { co = TS_H2; ci = t; }
    else if (t == DU_BV) { co = TS_H2; ci = -1; }
    else if (t < DU_BA) { const int rel = t - DU_WA, j = rel / TS_H2; co = 2 * TS_H2 + 1 + j; ci = TS_H2 + 1 + (rel - j * TS_H2); }
    else { co = 2 * TS_H2 + 1 + (t - DU_BA); ci = -1; }
    const float xo = nz_xi(k, co);
    return ci >= 0 ? xo * nz_xi(k, ci) : xo;
}

// ---- the head as this library holds it -------------------------------------------------------------------
// mi_dueling.h's state, where sm.hd is the EFFECTIVE head (acting: two alternating copies of the online head), and the gradient launch's eps
struct nz_smem : du_smem {
    float eps[256];                     // the gradient launch: eps of the online head, a word per thread, read only by its writer
};

// the effective head mu + sigma * eps of the parameters P under sample k into sm.hd[net] (noisy == 0: the mean head, no draw); returns eps_t (0 when off or t == 255)
__device__ __forceinline__ float nz_form_head(nz_smem& sm, int net, const float* __restrict__ P, const nz_key& k, int noisy, int t) {
    float eps = 0.0f;
    if (t < DU_NHEAD) {
        const float mu = P[DU_HEAD + t];
        if (noisy) {
            eps = nz_eps(k, t);
            sm.hd[net][t] = mu + P[PD_SIGMA + t] * eps;   // -ffp-contract=off: a product, then a sum
        } else {
            sm.hd[net][t] = mu;
        }
    }
    return eps;
}

// =====================================================================================================
// the sample, written out
// =====================================================================================================
__global__ void __launch_bounds__(256) nz_noise_kernel(nz_key k, float* __restrict__ xi_out, float* __restrict__ eps_out) {
    const int t = threadIdx.x;
    if (t < MI_NZ_NXI) xi_out[t] = nz_xi(k, t);
    if (t < DU_NHEAD) eps_out[t] = nz_eps(k, t);
}

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) nz_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, nz_key key, int noisy,
                                                         float* __restrict__ q) {
    __shared__ nz_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, params, t);
    nz_form_head(sm, DU_ONLINE, params, key, noisy, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        du_torso_rows<true, false>(w, w, x, x, sm, t);
        float q0, q1;
        du_values(sm, DU_ROW, DU_ONLINE, q0, q1);
        if (t == 0) { q[2 * (size_t)row] = q0; q[2 * (size_t)row + 1] = q1; }
        // no barrier here: sm.h2 is next written behind two barriers of the next du_torso_rows, which no wave passes before all have read it
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the online torso in `w`, mu_t and sigma_t of this thread's head element in registers, the effective head in LDS
template <bool NOISY>
struct nz_policy {
    const ts_torso& w;
    nz_smem& sm;
    int t;
    uint64_t seed;
    float mu, sigma;
    int cur;   // the copy of sm.hd the last greedy step read (workgroup-uniform); NOISY false: always 0, the mean head loaded at the kernel's start
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t env_id, uint64_t ctr) {
        if (NOISY) {
            // the other copy: its last readers (the greedy step before the previous one) left du_values before any wave passed the previous step's three barriers
            cur ^= 1;
            if (t < DU_NHEAD) sm.hd[cur][t] = mu + sigma * nz_eps(nz_key{seed, env_id, ctr, MI_NZ_STREAM_ACT}, t);
        }
        du_torso_rows<true, false>(w, w, x, x, sm, t);   // its barriers publish the head
        float q0, q1;
        du_values(sm, DU_ROW, NOISY ? cur : 0, q0, q1);
        return du_argmax(q0, q1);
    }
};

// NOISY false is pdd_act_kernel: the draw's code and registers are not in that instantiation at all
template <bool FORCED, bool NOISY>
__global__ void __launch_bounds__(256) nz_act_kernel(mi_env e, mi_nz_ring_t ring, mi_nz_act_t a_, rg_eps_tab eps) {
    __shared__ nz_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, a_.params, t);
    du_load_head(sm, 0, a_.params, t);
    const float sigma = NOISY && t < DU_NHEAD ? a_.params[PD_SIGMA + t] : 0.0f;
    const float mu = NOISY && t < DU_NHEAD ? a_.params[DU_HEAD + t] : 0.0f;
    __syncthreads();
    nz_policy<NOISY> policy{w, sm, t, e.seed, mu, sigma, 0};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient (the rows of mi_nstep.hip, under the two learning samples)
// =====================================================================================================
__global__ void __launch_bounds__(256) nz_target_kernel(mi_nz_ring_t ring, mi_nz_batch_t bt) {
    __shared__ nz_smem sm;
    __shared__ du_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    nz_form_head(sm, DU_ONLINE, bt.params, nz_key{bt.sample_seed, bt.sample_update, 0, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    nz_form_head(sm, DU_TARGET, bt.target_params, nz_key{bt.sample_seed, bt.sample_update, 1, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    ts_torso on, tg;
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        const float4 xn = du_walk_row(ring, bt, i, total, wk[par], t);
        du_torso_rows<false, true>(on, tg, xn, xn, sm, t);
        int a_star; float tgt;
        du_target_value(sm, wk[par].R, wk[par].lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.horizon[b] = wk[par].m; }
        par ^= 1;
    }
}

__global__ void __launch_bounds__(256) nz_grad_kernel(mi_nz_ring_t ring, mi_nz_batch_t bt, float* __restrict__ slabs) {
    __shared__ nz_smem sm;
    __shared__ du_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    // the two heads, once per launch, ahead of the torsos' loads (the draw's temporaries are dead before the 2 x 46 resident floats arrive); eps_t of the online
    // head waits in this thread's LDS word for the slab store
    sm.eps[t] = nz_form_head(sm, DU_ONLINE, bt.params, nz_key{bt.sample_seed, bt.sample_update, 0, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    nz_form_head(sm, DU_TARGET, bt.target_params, nz_key{bt.sample_seed, bt.sample_update, 1, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    ts_torso on, tg;   // the online network is loaded once and serves both online passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    du_grads G;   // G.gh: the gradient of EFFECTIVE head element t; the torso's backward reads the effective head
    du_zero(G);
    const float inv = 1.0f / (float)bt.batch;
    const du_elem he = du_classify(t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        const float4 xn = du_walk_row(ring, bt, i, total, wk[par], t);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float wb = bt.weights ? bt.weights[b] : 1.0f;
        du_grad_row(G, sm, on, tg, xi, xn, a, wk[par].R, wk[par].lg, wb, inv, he, bt.params, t, [&](int a_star, float tgt, float cur, float td) {
            bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.current[b] = cur; bt.td_abs[b] = fabsf(td); bt.horizon[b] = wk[par].m;
        });
        par ^= 1;
    }
    float* const slab = slabs + (size_t)blockIdx.x * PD_STRIDE;
    if (t < DU_NHEAD) slab[PD_SIGMA + t] = bt.noisy ? G.gh * sm.eps[t] : 0.0f;   // one product; off: exact zeros
    du_store(G, slab, PD_NP, t);
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) nz_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                        float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                        rg_adam_consts k, int adam) {
    rg_reduce<PD_NP, PD_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_nz_noise(uint64_t seed, uint64_t a, uint64_t b, uint32_t stream, float* xi_out, float* eps_out, void* hip_stream) {
    RG_CHECK_ARG(xi_out && eps_out, "xi_out or eps_out is NULL");
    RG_CHECK_ARG(stream < 16u, "stream must be in [0, 16)");
    nz_noise_kernel<<<1, 256, 0, (hipStream_t)hip_stream>>>(nz_key{seed, a, b, stream}, xi_out, eps_out);
    RG_HIP(hipGetLastError());
    return MI_NZ_OK;
}

extern "C" int mi_nz_forward(const float* params, const float* obs, int n, const mi_nz_key_t* key, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && n > 0 && q, "bad arguments");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    RG_CHECK_ARG(key == nullptr || key->stream < 16u, "the key's stream must be in [0, 16)");
    const nz_key k = key ? nz_key{key->seed, key->a, key->b, key->stream} : nz_key{0, 0, 0, 0};
    nz_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, n, k, key ? 1 : 0, q);
    RG_HIP(hipGetLastError());
    return MI_NZ_OK;
}

extern "C" int mi_nz_act_steps(void* handle, const mi_nz_ring_t* ring, const mi_nz_act_t* a, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    DU_ACT_EPSILON(e, a, tab);
    int grid;
    const int rc = rg_act_prelude(e, ring, a->params, a->obs_cur, a->n_steps, a->max_ep, a->episodes, a->episode_stats, s, grid);
    if (rc != MI_NZ_OK) return rc;
    const bool forced = a->forced_actions || a->forced_resets;
    if (a->noisy) {
        if (forced) nz_act_kernel<true, true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
        else nz_act_kernel<false, true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    } else {
        if (forced) nz_act_kernel<true, false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
        else nz_act_kernel<false, false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    }
    RG_HIP(hipGetLastError());
    return MI_NZ_OK;
}

extern "C" int mi_nz_target(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_NZ_OK) return rc;
    DU_CHECK_TARGET(b);
    DU_CHECK_WALK(ring, b);
    nz_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_NZ_OK;
}

// mi_nz_grad (update false: opt is not looked at) and mi_nz_update
static int nz_grad(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, const mi_nz_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_nz_batch_t& bt) { return bt.current && bt.target && bt.td_abs; });
    if (rc != RG_OK) return rc;
    DU_CHECK_WALK(ring, b);
    if (update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<PD_NP>(nz_grad_kernel, nz_reduce_kernel, ring, b, nz_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_nz_grad(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, void* stream) { return nz_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_nz_update(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, const mi_nz_adam_t* opt, void* stream) {
    return nz_grad(ring, b, opt, true, (hipStream_t)stream);
}
