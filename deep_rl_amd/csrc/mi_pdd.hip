// mi_pdd.hip — libmirl_pdd.so: prioritized dueling Double DQN on CartPole-v1 for gfx950.  C ABI, numerics and RNG contract: include/mi_pdd.h.
//
// The form of mi_ddqn.hip: one 256-thread workgroup evaluates one row at a time with the torso in its registers (thread c * 84 + o a 40-wide third of row o of W2,
// thread u < 120 row u of W1), loaded once per launch; the 255-element dueling heads (value row, advantage rows, three biases) lie in LDS in parameter order and every
// thread forms both action values itself from workgroup-uniform broadcasts, so a forward pass costs the torso's three barriers and none for the head.  The gradient
// launch holds BOTH networks' torsos (2 x 46 floats per thread) beside its accumulators and evaluates the three torsos of a batch row — online at obs[i], online at
// obs[nx], target at obs[nx] — between the same three barriers.  The head's gradient is ONE accumulator per thread: thread t < 255 owns element 10,764 + t.
//   pdd_act_kernel      a workgroup walks its envs, each through all steps of the chunk; exploring and pre-learning_starts steps skip the network.
//   pdd_grad_kernel     a workgroup walks its batch rows: pass 1 on obs[nx] (online argmax a*, the target network's value of a* -> next_actions / target), pass 2 on
//                       obs[i] (online forward -> current, |td|, weighted loss, backward into register accumulators) — one slab per workgroup.
//   pdd_reduce_kernel   fixed-order slab sum (+ Adam).
//   pdd_target_kernel   pass 1 alone.
//   pdd_forward_kernel  the action values of n observations.
// The torso's layout, loader, per-thread pieces, backward and slab store are mi_torso.h's; the host side of acting and of the gradient entry points is mi_ring.h's.
// pd_torso_rows is a copy of mi_ddqn.hip's dd_torso_rows (the three-evaluation torso helper): both libraries' sources are pinned by their ids, sharing it is a change
// to mi_torso.h of its own.  All arithmetic on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"

#include "../../include/mi_pdd.h"

#define PD_H1 MI_PDD_H1
#define PD_H2 MI_PDD_H2
#define PD_HEAD MI_PDD_WV                       // the head's first element
#define PD_NHEAD (MI_PDD_NPARAMS - MI_PDD_WV)   // 255: Wv[84] bv Wa[2][84] ba[2]
#define PD_WV 0                                 // offsets inside the head
#define PD_BV (MI_PDD_BV - MI_PDD_WV)
#define PD_WA (MI_PDD_WA - MI_PDD_WV)
#define PD_BA (MI_PDD_BA - MI_PDD_WV)
#define PD_NP MI_PDD_NPARAMS
#define PD_STRIDE MI_PDD_SLAB_STRIDE
static_assert(MI_PDD_OK == RG_OK && MI_PDD_EINVAL == RG_EINVAL && MI_PDD_EHIP == RG_EHIP && MI_PDD_MAX_STEPS_PER_CALL == RG_MAX_STEPS, "mi_ring.h returns these");
static_assert(MI_PDD_W1 == TS_W1 && MI_PDD_B1 == TS_B1 && MI_PDD_W2 == TS_W2 && MI_PDD_B2 == TS_B2 && MI_PDD_H1 == TS_H1 && MI_PDD_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_PDD_WV == TS_B2 + TS_H2 && MI_PDD_BV == MI_PDD_WV + PD_H2 && MI_PDD_WA == MI_PDD_BV + 1 && MI_PDD_BA == MI_PDD_WA + 2 * PD_H2 && PD_NP == MI_PDD_BA + 2, "the head");
static_assert(PD_NHEAD == 255 && PD_NHEAD <= 256, "one head element per thread");
static_assert(PD_STRIDE % 4 == 0 && PD_STRIDE > PD_NP, "float4 stores");

#ifndef MI_PDD_SOURCE_ID
#define MI_PDD_SOURCE_ID "unknown"
#endif
extern "C" int mi_pdd_version(void) { return MI_PDD_VERSION; }
extern "C" const char* mi_pdd_last_error(void) { return rg_err; }
extern "C" const char* mi_pdd_source_id(void) { return MI_PDD_SOURCE_ID; }
static int pd_slabs(int batch) { return rg_slabs(batch, MI_PDD_MAX_SLABS); }
extern "C" size_t mi_pdd_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)pd_slabs(batch) * PD_STRIDE * sizeof(float);
}

// ---- the network as one workgroup holds it ------------------------------------------------------------
// the evaluations a workgroup keeps side by side: ROW the online network at obs[i], NEXT the online network at obs[nx], TGT the target network at obs[nx]
enum { PD_ROW = 0, PD_NEXT = 1, PD_TGT = 2, PD_EVALS = 3 };
enum { PD_ONLINE = 0, PD_TARGET = 1 };
struct pd_smem {
    float h1[PD_EVALS][PD_H1];
    float p2[PD_EVALS][3][PD_H2];       // layer 2's partial chains
    float h2[PD_EVALS][PD_H2];
    float hd[2][256];                   // [network]: the head in parameter order (PD_WV, PD_BV, PD_WA, PD_BA); element 255 is never touched
    float dz2[PD_H2];
    float ph[2][PD_H1];                 // the backward's partial chains of dh1
};

// the head of the parameters P into sm.hd[net], element by element (it starts at an odd offset); the caller's next barrier (every torso evaluation has three)
// publishes it
__device__ __forceinline__ void pd_load_head(pd_smem& sm, int net, const float* __restrict__ P, int t) {
    if (t < PD_NHEAD) sm.hd[net][t] = P[PD_HEAD + t];
}

// layers 1 and 2: with ROW the online torso `on` at xi (-> sm.h1 / sm.h2 [PD_ROW]), with NEXT the online torso at xn (-> [PD_NEXT]) and the target torso `tg` at xn
// (-> [PD_TGT]), all between the same three barriers; the results are valid for every thread when it returns
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

// THE two action values (mi_pdd.h) of evaluation `ev` through the head of network `net`, in every thread (three independent chains; the reads are workgroup-uniform
// broadcasts)
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

// =====================================================================================================
// forward API
// =====================================================================================================
__global__ void __launch_bounds__(256) pdd_forward_kernel(const float* __restrict__ params, const float* __restrict__ obs, int n, float* __restrict__ q) {
    __shared__ pd_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, params, t);
    pd_load_head(sm, PD_ONLINE, params, t);
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
// the greedy action of rg_act_loop: the online torso in `w`, its head in LDS
struct pd_policy {
    const ts_torso& w;
    pd_smem& sm;
    int t;
    __device__ __forceinline__ int greedy(const float4& x, int, int, uint64_t, uint64_t) {
        pd_torso_rows<true, false>(w, w, x, x, sm, t);
        float q0, q1;
        pd_values(sm, PD_ROW, PD_ONLINE, q0, q1);
        // no barrier here: sm.h2 is next written behind two barriers of the next pd_torso_rows, which no wave passes before all have read it
        return pd_argmax(q0, q1);
    }
};

template <bool FORCED>
__global__ void __launch_bounds__(256) pdd_act_kernel(mi_env e, mi_pdd_ring_t ring, mi_pdd_act_t a_, rg_eps_tab eps) {
    __shared__ pd_smem sm;
    const int t = threadIdx.x;
    ts_torso w;
    ts_load(w, a_.params, t);
    pd_load_head(sm, PD_ONLINE, a_.params, t);
    __syncthreads();
    pd_policy policy{w, sm, t};
    const rg_act_args a{a_.obs_cur, a_.forced_actions, a_.forced_resets, a_.episodes, a_.episode_stats, a_.global_step, a_.learning_starts, a_.n_steps, a_.max_ep};
    rg_act_loop<FORCED>(e, ring, a, eps, policy);
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// the successor of flat ring index i: ((slot + 1) % slots) * N + env
__device__ __forceinline__ long long pd_successor(const mi_pdd_ring_t& ring, long long i, long long total) {
    const long long N = ring.n_envs;
    return i + N >= total ? i + N - total : i + N;
}
// pass 1 of a row whose evaluations PD_NEXT / PD_TGT are in sm: a* by the online head, the target network's value of a* (every thread holds both)
__device__ __forceinline__ void pd_target_value(const pd_smem& sm, float r, float lg, int& a_star, float& tgt) {
    float q0, q1, t0, t1;
    pd_values(sm, PD_NEXT, PD_ONLINE, q0, q1);
    pd_values(sm, PD_TGT, PD_TARGET, t0, t1);
    a_star = pd_argmax(q0, q1);
    tgt = r + lg * (a_star ? t1 : t0);   // -ffp-contract=off: a product, then a sum
}

__global__ void __launch_bounds__(256) pdd_target_kernel(mi_pdd_ring_t ring, mi_pdd_batch_t bt) {
    __shared__ pd_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    pd_load_head(sm, PD_ONLINE, bt.params, t);
    pd_load_head(sm, PD_TARGET, bt.target_params, t);
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        const long long nx = pd_successor(ring, i, total);
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        pd_torso_rows<false, true>(on, tg, xn, xn, sm, t);
        int a_star; float tgt;
        pd_target_value(sm, r, lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; }
    }
}

__global__ void __launch_bounds__(256) pdd_grad_kernel(mi_pdd_ring_t ring, mi_pdd_batch_t bt, float* __restrict__ slabs) {
    __shared__ pd_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;   // the online network is loaded once and serves both online passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    pd_load_head(sm, PD_ONLINE, bt.params, t);
    pd_load_head(sm, PD_TARGET, bt.target_params, t);
    float gh = 0.0f, loss = 0.0f;   // gh: the gradient of head element t (t < 255)
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
        const long long nx = pd_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        const float wb = bt.weights ? bt.weights[b] : 1.0f;
        pd_torso_rows<true, true>(on, tg, xi, xn, sm, t);
        // ---- pass 1, obs[nx]: the online argmax, the target network's value of it ----
        int a_star; float tgt;
        pd_target_value(sm, r, lg, a_star, tgt);
        // ---- pass 2, obs[i]: the stored action's online value, |td|, the weighted loss, the backward into register accumulators ----
        float c0, c1;
        pd_values(sm, PD_ROW, PD_ONLINE, c0, c1);
        const float cur = a ? c1 : c0;
        const float td = tgt - cur;
        const float d = -(((2.0f * td) * wb) * inv);
        const float e = 0.5f * d;
        if (t == 0) {
            bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.current[b] = cur; bt.td_abs[b] = fabsf(td);
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
        if (t < PD_H2) {
            const float* const hd = sm.hd[PD_ONLINE];
            const float wa_a = hd[PD_WA + a * PD_H2 + t], wa_o = hd[PD_WA + (1 - a) * PD_H2 + t];
            sm.dz2[t] = sm.h2[PD_ROW][t] > 0.0f ? (d * hd[PD_WV + t]) + (e * (wa_a - wa_o)) : 0.0f;
        }
        __syncthreads();
        ts_backward(g, sm.h1[PD_ROW], sm.dz2, sm.ph, xi, P, t);   // sm.h1 / sm.ph / sm.dz2 are then the next row's
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * PD_STRIDE;
    if (t < PD_NHEAD) slab[PD_HEAD + t] = gh;
    ts_store(g, slab, t);
    if (t == 0) slab[PD_NP] = loss;
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) pdd_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                         float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                         rg_adam_consts k, int adam) {
    rg_reduce<PD_NP, PD_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int mi_pdd_forward(const float* params, const float* obs, int n, float* q, void* stream) {
    RG_CHECK_ARG(params && obs && n > 0 && q, "bad arguments");
    RG_CHECK_ARG(rg_aligned(params) && rg_aligned(obs), "params and obs must be 16-byte aligned");
    pdd_forward_kernel<<<n < 1024 ? n : 1024, 256, 0, (hipStream_t)stream>>>(params, obs, n, q);
    RG_HIP(hipGetLastError());
    return MI_PDD_OK;
}

extern "C" int mi_pdd_act_steps(void* handle, const mi_pdd_ring_t* ring, const mi_pdd_act_t* a, void* stream) {
    const mi_env* e = (const mi_env*)handle;
    RG_CHECK_ARG(e != nullptr && a != nullptr, "NULL pointer");
    RG_CHECK_ARG(a->global_step >= 0 && a->total_timesteps > 0 && a->exploration_fraction > 0.0, "global_step < 0, total_timesteps <= 0 or exploration_fraction <= 0");
    RG_CHECK_ARG(a->learning_starts >= 0, "learning_starts < 0");
    hipStream_t s = (hipStream_t)stream;
    rg_eps_tab tab;
    rg_eps_fill(tab, a->global_step, (a->end_e - a->start_e) / (a->exploration_fraction * (double)a->total_timesteps), a->start_e, a->end_e);
    for (int k = 0; k < RG_MAX_STEPS; ++k) tab.v[k] = (double)(float)tab.v[k];   // DQN compares the draw with epsilon as an f32 (mi_dqn_act_steps)
    int grid;
    const int rc = rg_act_prelude(e, ring, a->params, a->obs_cur, a->n_steps, a->max_ep, a->episodes, a->episode_stats, s, grid);
    if (rc != MI_PDD_OK) return rc;
    if (a->forced_actions || a->forced_resets)
        pdd_act_kernel<true><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    else
        pdd_act_kernel<false><<<grid, 256, 0, s>>>(*e, *ring, *a, tab);
    RG_HIP(hipGetLastError());
    return MI_PDD_OK;
}

extern "C" int mi_pdd_target(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_PDD_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->next_actions && b->target && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params), "params and target_params must be 16-byte aligned");
    pdd_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_PDD_OK;
}

// mi_pdd_grad (update false: opt is not looked at) and mi_pdd_update
static int pd_grad(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, const mi_pdd_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_pdd_batch_t& bt) { return bt.current && bt.target && bt.td_abs; });
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<PD_NP>(pdd_grad_kernel, pdd_reduce_kernel, ring, b, pd_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_pdd_grad(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, void* stream) { return pd_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_pdd_update(const mi_pdd_ring_t* ring, const mi_pdd_batch_t* b, const mi_pdd_adam_t* opt, void* stream) {
    return pd_grad(ring, b, opt, true, (hipStream_t)stream);
}
