// mi_noisy.hip — libmirl_noisy.so: noisy-net exploration on n-step prioritized dueling Double DQN on CartPole-v1 for gfx950.  C ABI, numerics and RNG contract:
// include/mi_noisy.h (and include/mi_nstep.h / include/mi_pdd.h, which it refers to for everything but the noise).
//
// The form of mi_nstep.hip and mi_pdd.hip: one 256-thread workgroup evaluates one row at a time with the torso(s) in its registers and the 255-element dueling
// head(s) in LDS, one element per thread.  The noise sits where a thread already owns its element: thread t < 255 derives THAT element's eps itself (at most two
// Philox calls and two Box-Muller values; the output factors are recomputed redundantly across threads) and writes mu_t + sigma_t * eps_t into sm.hd, so forming the
// effective head needs no LDS exchange and no barrier of its own — the torso's three barriers publish it as they publish a loaded head.
//   nz_act_kernel      rg_act_loop as it is, instantiated with and without the noise (without it the kernel is pdd_act_kernel).  policy.greedy forms a fresh head
//                      per greedy env step ahead of pd_torso_rows.  The acting launch uses only the online network, so the two copies sm.hd[0] / sm.hd[1] ALTERNATE between greedy steps: step k writes the copy step k - 2 read, and every wave has
//                      left step k - 2's pd_values before any passes the three barriers of step k - 1.  No barrier is added.
//   nz_forward_kernel  the action values of n observations under one sample, or the mean network.
//   nz_target_kernel   pass 1 alone; both heads formed once per launch.
//   nz_grad_kernel     ns_grad_kernel with both heads formed once per launch; eps_t waits in LDS (a word per thread, read by its writer: no barrier) for the slab
//                      store, where slab[SIGMA + t] = gh * eps_t.
//   nz_reduce_kernel   fixed-order slab sum (+ Adam) over 11,274 elements.
//   nz_noise_kernel    one sample written out as the kernels form it (the tests' view of the draw).
// pd_smem, pd_torso_rows, pd_values, pd_argmax, pd_target_value and the walk's hand-off are COPIES of mi_nstep.hip's / mi_pdd.hip's: those libraries' sources are
// pinned by their ids.  nz_normal is a copy of mi_sac.hip's keyed_normal expression with the stream as an argument (that file cannot be included).
// All arithmetic on the VALU in fp32; no floating-point atomics, no inline assembly, no device-wide hand-off inside a launch.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"
#include "mi_nwalk.h"

#include "../../include/mi_noisy.h"

#define PD_H1 MI_NZ_H1
#define PD_H2 MI_NZ_H2
#define PD_HEAD MI_NZ_WV                      // the head's first mean
#define PD_SIGMA MI_NZ_SIGMA                  // the head's first sigma
#define PD_NHEAD MI_NZ_NHEAD                  // 255: Wv[84] bv Wa[2][84] ba[2]
#define PD_WV 0                               // offsets inside the head
#define PD_BV (MI_NZ_BV - MI_NZ_WV)
#define PD_WA (MI_NZ_WA - MI_NZ_WV)
#define PD_BA (MI_NZ_BA - MI_NZ_WV)
#define PD_NP MI_NZ_NPARAMS
#define PD_STRIDE MI_NZ_SLAB_STRIDE
static_assert(MI_NZ_OK == RG_OK && MI_NZ_EINVAL == RG_EINVAL && MI_NZ_EHIP == RG_EHIP && MI_NZ_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_NZ_W1 == TS_W1 && MI_NZ_B1 == TS_B1 && MI_NZ_W2 == TS_W2 && MI_NZ_B2 == TS_B2 && MI_NZ_H1 == TS_H1 && MI_NZ_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_NZ_WV == TS_B2 + TS_H2 && MI_NZ_BV == MI_NZ_WV + PD_H2 && MI_NZ_WA == MI_NZ_BV + 1 && MI_NZ_BA == MI_NZ_WA + 2 * PD_H2 && PD_SIGMA == MI_NZ_BA + 2, "the head");
static_assert(PD_NHEAD == PD_SIGMA - PD_HEAD && PD_NP == PD_SIGMA + PD_NHEAD && PD_NHEAD <= 256, "one head element per thread, mu and then sigma");
static_assert(MI_NZ_NXI == 2 * PD_H2 + 3 && MI_NZ_NXI <= 256, "84 + 1 value factors, 84 + 2 advantage factors; b * 256 + c keys them");
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
    if (t < PD_BV) { co = PD_H2; ci = t; }
    else if (t == PD_BV) { co = PD_H2; ci = -1; }
    else if (t < PD_BA) { const int rel = t - PD_WA, j = rel / PD_H2; co = 2 * PD_H2 + 1 + j; ci = PD_H2 + 1 + (rel - j * PD_H2); }
    else { co = 2 * PD_H2 + 1 + (t - PD_BA); ci = -1; }
    const float xo = nz_xi(k, co);
    return ci >= 0 ? xo * nz_xi(k, ci) : xo;
}

// ---- the network as one workgroup holds it (mi_pdd.hip's, copied) -----------------------------------------
enum { PD_ROW = 0, PD_NEXT = 1, PD_TGT = 2, PD_EVALS = 3 };
enum { PD_ONLINE = 0, PD_TARGET = 1 };
struct pd_smem {
    float h1[PD_EVALS][PD_H1];
    float p2[PD_EVALS][3][PD_H2];       // layer 2's partial chains
    float h2[PD_EVALS][PD_H2];
    float hd[2][256];                   // [network] (acting: two alternating copies of the online head): the EFFECTIVE head in parameter order; element 255 is never touched
    float dz2[PD_H2];
    float ph[2][PD_H1];                 // the backward's partial chains of dh1
    float eps[256];                     // the gradient launch: eps of the online head, a word per thread, read only by its writer
};

// the mean head of the parameters P into sm.hd[net], element by element (it starts at an odd offset); the caller's next barrier (every torso evaluation has
// three) publishes it
__device__ __forceinline__ void pd_load_head(pd_smem& sm, int net, const float* __restrict__ P, int t) {
    if (t < PD_NHEAD) sm.hd[net][t] = P[PD_HEAD + t];
}
// the effective head mu + sigma * eps of the parameters P under sample k into sm.hd[net] (noisy == 0: the mean head, no draw); returns eps_t (0 when off or t == 255)
__device__ __forceinline__ float nz_form_head(pd_smem& sm, int net, const float* __restrict__ P, const nz_key& k, int noisy, int t) {
    float eps = 0.0f;
    if (t < PD_NHEAD) {
        const float mu = P[PD_HEAD + t];
        if (noisy) {
            eps = nz_eps(k, t);
            sm.hd[net][t] = mu + P[PD_SIGMA + t] * eps;   // -ffp-contract=off: a product, then a sum
        } else {
            sm.hd[net][t] = mu;
        }
    }
    return eps;
}

template <bool ROW, bool NEXT>
__device__ __forceinline__ void pd_torso_rows(const ts_torso& on, const ts_torso& tg, const float4 xi, const float4 xn, pd_smem& sm, int t) {
    if (t < PD_H1) {
        if (ROW) sm.h1[PD_ROW][t] = ts_h1(on, xi);
        if (NEXT) { sm.h1[PD_NEXT][t] = ts_h1(on, xn); sm.h1[PD_TGT][t] = ts_h1(tg, xn); }
    }
    __syncthreads();
    if (t < 3 * PD_H2) {
        const int c = t / PD_H2, o = t - c * PD_H2;
        if (ROW) sm.p2[PD_ROW][c][o] = ts_p2(on, &sm.h1[PD_ROW][TS_W2C * c]);
        if (NEXT) { sm.p2[PD_NEXT][c][o] = ts_p2(on, &sm.h1[PD_NEXT][TS_W2C * c]); sm.p2[PD_TGT][c][o] = ts_p2(tg, &sm.h1[PD_TGT][TS_W2C * c]); }
    }
    __syncthreads();
    if (t < PD_H2) {
        if (ROW) sm.h2[PD_ROW][t] = ts_h2(sm.p2[PD_ROW], t);
        if (NEXT) { sm.h2[PD_NEXT][t] = ts_h2(sm.p2[PD_NEXT], t); sm.h2[PD_TGT][t] = ts_h2(sm.p2[PD_TGT], t); }
    }
    __syncthreads();
}

// THE two action values (mi_pdd.h) of evaluation `ev` through the head sm.hd[net], in every thread
__device__ __forceinline__ void pd_values(const pd_smem& sm, int ev, int net, float& q0, float& q1) {
    const float* const hd = sm.hd[net];
    float v = hd[PD_BV], a0 = hd[PD_BA], a1 = hd[PD_BA + 1];
#pragma unroll
    for (int k = 0; k < PD_H2; ++k) {
        const float h = sm.h2[ev][k];
        v = __builtin_fmaf(hd[PD_WV + k], h, v);
        a0 = __builtin_fmaf(hd[PD_WA + k], h, a0);
        a1 = __builtin_fmaf(hd[PD_WA + PD_H2 + k], h, a1);
    }
    const float m = (a0 + a1) * 0.5f;
    q0 = v + (a0 - m);
    q1 = v + (a1 - m);
}
__device__ __forceinline__ int pd_argmax(float q0, float q1) { return q1 > q0 ? 1 : 0; }   // torch.argmax: the first index on a tie

__device__ __forceinline__ void pd_target_value(const pd_smem& sm, float r, float lg, int& a_star, float& tgt) {
    float q0, q1, t0, t1;
    pd_values(sm, PD_NEXT, PD_ONLINE, q0, q1);
    pd_values(sm, PD_TGT, PD_TARGET, t0, t1);
    a_star = pd_argmax(q0, q1);
    tgt = r + lg * (a_star ? t1 : t0);   // -ffp-contract=off: a product, then a sum
}

// =====================================================================================================
// the sample, written out
// =====================================================================================================
__global__ void __launch_bounds__(256) nz_noise_kernel(nz_key k, float* __restrict__ xi_out, float* __restrict__ eps_out) {
    const int t = threadIdx.x;
    if (t < MI_NZ_NXI) xi_out[t] = nz_xi(k, t);
    if (t < PD_NHEAD) eps_out[t] = nz_eps(k, t);
}

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) nz_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, nz_key key, int noisy,
                                                         float* __restrict__ q) {
    __shared__ pd_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, params, t);
    nz_form_head(sm, PD_ONLINE, params, key, noisy, t);
    for (int row = blockIdx.x; row < n; row += gridDim.x) {
        const float4 x = reinterpret_cast<const float4*>(obs)[row];
        pd_torso_rows<true, false>(w, w, x, x, sm, t);
        float q0, q1;
        pd_values(sm, PD_ROW, PD_ONLINE, q0, q1);
        if (t == 0) { q[2 * (size_t)row] = q0; q[2 * (size_t)row + 1] = q1; }
        // no barrier here: sm.h2 is next written behind two barriers of the next pd_torso_rows, which no wave passes before all have read it
    }
}

// =====================================================================================================
// acting
// =====================================================================================================
// the greedy action of rg_act_loop: the online torso in `w`, mu_t and sigma_t of this thread's head element in registers, the effective head in LDS
template <bool NOISY>
struct nz_policy {
    const ts_torso& w;
    pd_smem& sm;
    int t;
    uint64_t seed;
    float mu, sigma;
    int cur;   // the copy of sm.hd the last greedy step read (workgroup-uniform); NOISY false: always 0, the mean head loaded at the kernel's start
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t env_id, uint64_t ctr) {
        if (NOISY) {
            // the other copy: its last readers (the greedy step before the previous one) left pd_values before any wave passed the previous step's three barriers
            cur ^= 1;
            if (t < PD_NHEAD) sm.hd[cur][t] = mu + sigma * nz_eps(nz_key{seed, env_id, ctr, MI_NZ_STREAM_ACT}, t);
        }
        pd_torso_rows<true, false>(w, w, x, x, sm, t);   // its barriers publish the head
        float q0, q1;
        pd_values(sm, PD_ROW, NOISY ? cur : 0, q0, q1);
        return pd_argmax(q0, q1);
    }
};

// NOISY false is pdd_act_kernel: the draw's code and registers are not in that instantiation at all
template <bool FORCED, bool NOISY>
__global__ void __launch_bounds__(256) nz_act_kernel(mi_env e, mi_nz_ring_t ring, mi_nz_act_t a_, rg_eps_tab eps) {
    __shared__ pd_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, a_.params, t);
    pd_load_head(sm, 0, a_.params, t);
    const float sigma = NOISY && t < PD_NHEAD ? a_.params[PD_SIGMA + t] : 0.0f;
    const float mu = NOISY && t < PD_NHEAD ? a_.params[PD_HEAD + t] : 0.0f;
    __syncthreads();
    nz_policy<NOISY> policy{w, sm, t, e.seed, mu, sigma, 0};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient (mi_nstep.hip's, copied, under the two learning samples)
// =====================================================================================================
struct ns_walk_lds { float R, lg; int m; int pad; };
__device__ __forceinline__ float4 ns_walk_row(const mi_nz_ring_t& ring, const mi_nz_batch_t& bt, long long i, long long total, ns_walk_lds& out, int t) {
    float4 xn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t < 128) {
        const nw_walk_t w = nw_walk(ring, i, total, bt.n_step, bt.head_slot, bt.gamma);
        xn = reinterpret_cast<const float4*>(ring.observations)[w.at];
        if (t == 0) { out.R = w.R; out.lg = w.lg; out.m = w.m; }
    }
    return xn;
}

__global__ void __launch_bounds__(256) nz_target_kernel(mi_nz_ring_t ring, mi_nz_batch_t bt) {
    __shared__ pd_smem sm;
    __shared__ ns_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    nz_form_head(sm, PD_ONLINE, bt.params, nz_key{bt.sample_seed, bt.sample_update, 0, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    nz_form_head(sm, PD_TARGET, bt.target_params, nz_key{bt.sample_seed, bt.sample_update, 1, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    ts_torso on, tg;
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        const float4 xn = ns_walk_row(ring, bt, i, total, wk[par], t);
        pd_torso_rows<false, true>(on, tg, xn, xn, sm, t);
        int a_star; float tgt;
        pd_target_value(sm, wk[par].R, wk[par].lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.horizon[b] = wk[par].m; }
        par ^= 1;
    }
}

__global__ void __launch_bounds__(256) nz_grad_kernel(mi_nz_ring_t ring, mi_nz_batch_t bt, float* __restrict__ slabs) {
    __shared__ pd_smem sm;
    __shared__ ns_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    // the two heads, once per launch, ahead of the torsos' loads (the draw's temporaries are dead before the 2 x 46 resident floats arrive); eps_t of the online
    // head waits in this thread's LDS word for the slab store
    sm.eps[t] = nz_form_head(sm, PD_ONLINE, bt.params, nz_key{bt.sample_seed, bt.sample_update, 0, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    nz_form_head(sm, PD_TARGET, bt.target_params, nz_key{bt.sample_seed, bt.sample_update, 1, MI_NZ_STREAM_LEARN}, bt.noisy, t);
    ts_torso on, tg;   // the online network is loaded once and serves both online passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    float gh = 0.0f, loss = 0.0f;   // gh: the gradient of effective head element t (t < 255)
    ts_grads g;
    ts_zero(g);
    const float inv = 1.0f / (float)bt.batch;
    const float* __restrict__ P = bt.params;
    // what head element t is: a value weight, the value bias, an advantage weight of action hact, or an advantage bias of action hact; hk its h2 index
    const int hrel = t - PD_WA;
    const bool is_wv = t < PD_BV, is_bv = t == PD_BV, is_wa = t >= PD_WA && t < PD_BA, is_ba = t >= PD_BA && t < PD_NHEAD;
    const int hact = is_wa ? hrel / PD_H2 : t - PD_BA;
    const int hk = is_wv ? t : (is_wa ? hrel - hact * PD_H2 : 0);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        const float4 xn = ns_walk_row(ring, bt, i, total, wk[par], t);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float wb = bt.weights ? bt.weights[b] : 1.0f;
        pd_torso_rows<true, true>(on, tg, xi, xn, sm, t);
        // ---- pass 1, obs[s_m]: the online argmax, the target network's value of it ----
        int a_star; float tgt;
        pd_target_value(sm, wk[par].R, wk[par].lg, a_star, tgt);
        // ---- pass 2, obs[i]: the stored action's online value, |td|, the weighted loss, the backward into register accumulators ----
        float c0, c1;
        pd_values(sm, PD_ROW, PD_ONLINE, c0, c1);
        const float cur = a ? c1 : c0;
        const float td = tgt - cur;
        const float d = -(((2.0f * td) * wb) * inv);
        const float e = 0.5f * d;
        if (t == 0) {
            bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.current[b] = cur; bt.td_abs[b] = fabsf(td); bt.horizon[b] = wk[par].m;
            loss += wb * (td * td);
        }
        // the head: q_a = v + 0.5 A_a - 0.5 A_{1 - a}
        {
            const float h = sm.h2[PD_ROW][hk];
            const float es = hact == a ? e : -e;
            if (is_wv) gh = __builtin_fmaf(d, h, gh);
            else if (is_wa) gh = __builtin_fmaf(es, h, gh);
            else if (is_bv) gh += d;
            else if (is_ba) gh += es;
        }
        if (t < PD_H2) {   // the torso's backward reads the effective head
            const float* const hd = sm.hd[PD_ONLINE];
            const float wa_a = hd[PD_WA + a * PD_H2 + t], wa_o = hd[PD_WA + (1 - a) * PD_H2 + t];
            sm.dz2[t] = sm.h2[PD_ROW][t] > 0.0f ? (d * hd[PD_WV + t]) + (e * (wa_a - wa_o)) : 0.0f;
        }
        __syncthreads();
        ts_backward(g, sm.h1[PD_ROW], sm.dz2, sm.ph, xi, P, t);   // sm.h1 / sm.ph / sm.dz2 are then the next row's
        par ^= 1;
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * PD_STRIDE;
    if (t < PD_NHEAD) {
        slab[PD_HEAD + t] = gh;
        slab[PD_SIGMA + t] = bt.noisy ? gh * sm.eps[t] : 0.0f;   // one product; off: exact zeros
    }
    ts_store(g, slab, t);
    if (t == 0) slab[PD_NP] = loss;
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
    RG_CHECK_ARG(e != nullptr && a != nullptr, "NULL pointer");
    RG_CHECK_ARG(a->global_step >= 0 && a->total_timesteps > 0 && a->exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    RG_CHECK_ARG(a->learning_starts >= 0, "learning_starts < 0");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, (a->end_e - a->start_e) / (a->exploration_fraction * (double)a->total_timesteps), a->start_e, a->end_e);
    for (int k = 0; k < RG_MAX_STEPS; ++k) tab.v[k] = (double)(float)tab.v[k];   // DQN compares the draw with epsilon as an f32 (mi_pdd_act_steps)
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

// the members only the walk needs (a macro: the error text names the entry point that was called); mi_nstep.hip's three checks
#define NZ_CHECK_WALK(ring, b)                                                                                                                          \
    do {                                                                                                                                                \
        RG_CHECK_ARG((b)->horizon != nullptr, "horizon is NULL");                                                                                       \
        RG_CHECK_ARG((b)->n_step >= 1 && (b)->n_step <= MI_NZ_MAX_N && (int64_t)(b)->n_step < (ring)->slots, "n_step must be in [1, 16] and below slots"); \
        RG_CHECK_ARG((b)->head_slot >= 0 && (b)->head_slot < (ring)->slots, "head_slot outside [0, slots)");                                            \
    } while (0)

extern "C" int mi_nz_target(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_NZ_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->next_actions && b->target && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params), "params and target_params must be 16-byte aligned");
    NZ_CHECK_WALK(ring, b);
    nz_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_NZ_OK;
}

// mi_nz_grad (update false: opt is not looked at) and mi_nz_update
static int nz_grad(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, const mi_nz_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_nz_batch_t& bt) { return bt.current && bt.target && bt.td_abs; });
    if (rc != RG_OK) return rc;
    NZ_CHECK_WALK(ring, b);
    if (update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<PD_NP>(nz_grad_kernel, nz_reduce_kernel, ring, b, nz_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_nz_grad(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, void* stream) { return nz_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_nz_update(const mi_nz_ring_t* ring, const mi_nz_batch_t* b, const mi_nz_adam_t* opt, void* stream) {
    return nz_grad(ring, b, opt, true, (hipStream_t)stream);
}
