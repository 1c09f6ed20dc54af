// mi_mdqn.hip — libmirl_mdqn.so: Munchausen DQN on CartPole-v1 for gfx950.  C ABI and numerics contract: include/mi_mdqn.h.
//
// The form of mi_ddqn.hip, mirrored: one 256-thread workgroup evaluates one batch row at a time with BOTH networks' torsos in its registers (2 x 46 floats per thread,
// loaded once per launch) and both two-row heads in LDS, and evaluates the three torsos of a row — online at obs[i], target at obs[i], target at obs[nx] — between
// the same three barriers.  Every thread then forms the action values and the soft-max quantities itself from workgroup-uniform LDS broadcasts, so the Munchausen
// target costs no barrier of its own.
//   mdqn_grad_kernel     a workgroup walks its batch rows: pass 1 on the target network (its log-policy of the stored action at obs[i] -> bonus, its soft value at
//                        obs[nx] -> soft_value / next_actions / target), pass 2 on obs[i] (online forward -> current, loss, backward into register accumulators) — one
//                        slab per workgroup.
//   mdqn_reduce_kernel   fixed-order slab sum (+ Adam).
//   mdqn_target_kernel   pass 1 alone.
// No acting and no forward kernel: those are libmirl_ddqn.so's.  The torso is mi_torso.h's, the host side of the gradient entry points mi_ring.h's.  All arithmetic
// on the VALU in fp32 with the summation orders of the header; no floating-point atomics.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"

#include "../../include/mi_mdqn.h"

#define MD_H1 MI_MD_H1
#define MD_H2 MI_MD_H2
#define MD_W3 MI_MD_W3
#define MD_B3 MI_MD_B3
#define MD_NP MI_MD_NPARAMS
#define MD_STRIDE MI_MD_SLAB_STRIDE
static_assert(MI_MD_OK == RG_OK && MI_MD_EINVAL == RG_EINVAL && MI_MD_EHIP == RG_EHIP, "mi_ring.h returns these");
static_assert(MI_MD_W1 == TS_W1 && MI_MD_B1 == TS_B1 && MI_MD_W2 == TS_W2 && MI_MD_B2 == TS_B2 && MI_MD_H1 == TS_H1 && MI_MD_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MD_STRIDE % 4 == 0 && MD_STRIDE > MD_NP, "float4 stores");

#ifndef MI_MD_SOURCE_ID
#define MI_MD_SOURCE_ID "unknown"
#endif
extern "C" int mi_md_version(void) { return MI_MD_VERSION; }
extern "C" const char* mi_md_last_error(void) { return rg_err; }
extern "C" const char* mi_md_source_id(void) { return MI_MD_SOURCE_ID; }
static int md_slabs(int batch) { return rg_slabs(batch, MI_MD_MAX_SLABS); }
extern "C" size_t mi_md_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)md_slabs(batch) * MD_STRIDE * sizeof(float);
}

// ---- the network as one workgroup holds it ------------------------------------------------------------
// the evaluations a workgroup keeps side by side: ROW the online network at obs[i], TROW the target network at obs[i], TGT the target network at obs[nx]
enum { MD_ROW = 0, MD_TROW = 1, MD_TGT = 2, MD_EVALS = 3 };
enum { MD_ONLINE = 0, MD_TARGET = 1 };
struct md_smem {
    float h1[MD_EVALS][MD_H1];
    float p2[MD_EVALS][3][MD_H2];       // layer 2's partial chains
    float h2[MD_EVALS][MD_H2];
    float w3[2][2][MD_H2];              // [network][action]: the heads
    float b3[2][2];
    float dz2[MD_H2];
    float ph[2][MD_H1];                 // the backward's partial chains of dh1
};

// the head of the parameters P into sm.w3[net] / sm.b3[net]; the caller's next barrier (every torso evaluation has three) publishes it
__device__ __forceinline__ void md_load_head(md_smem& sm, int net, const float* __restrict__ P, int t) {
    if (t < 2 * MD_H2) sm.w3[net][t / MD_H2][t % MD_H2] = P[MD_W3 + t];
    else if (t < 2 * MD_H2 + 2) sm.b3[net][t - 2 * MD_H2] = P[MD_B3 + t - 2 * MD_H2];
}

// layers 1 and 2: the target torso `tg` at xi (-> sm.h1 / sm.h2 [MD_TROW]) and at xn (-> [MD_TGT]) and, with ROW, the online torso `on` at xi (-> [MD_ROW]), all
// between the same three barriers; the results are valid for every thread when it returns
template <bool ROW>
__device__ __forceinline__ void md_torso_rows(const ts_torso& on, const ts_torso& tg, const float4 xi, const float4 xn, md_smem& sm, int t) {
    if (t < MD_H1) {
        if (ROW) sm.h1[MD_ROW][t] = ts_h1(on, xi);
        sm.h1[MD_TROW][t] = ts_h1(tg, xi);
        sm.h1[MD_TGT][t] = ts_h1(tg, xn);
    }
    __syncthreads();
    if (t < 3 * MD_H2) {
        const int c = t / MD_H2, o = t - c * MD_H2;
        if (ROW) sm.p2[MD_ROW][c][o] = ts_p2(on, &sm.h1[MD_ROW][TS_W2C * c]);
        sm.p2[MD_TROW][c][o] = ts_p2(tg, &sm.h1[MD_TROW][TS_W2C * c]);
        sm.p2[MD_TGT][c][o] = ts_p2(tg, &sm.h1[MD_TGT][TS_W2C * c]);
    }
    __syncthreads();
    if (t < MD_H2) {
        if (ROW) sm.h2[MD_ROW][t] = ts_h2(sm.p2[MD_ROW], t);
        sm.h2[MD_TROW][t] = ts_h2(sm.p2[MD_TROW], t);
        sm.h2[MD_TGT][t] = ts_h2(sm.p2[MD_TGT], t);
    }
    __syncthreads();
}

// THE two action values (mi_ddqn.h) of evaluation `ev` through the head of network `net`, in every thread (two independent chains; the reads are workgroup-uniform
// broadcasts)
__device__ __forceinline__ void md_values(const md_smem& sm, int ev, int net, float& q0, float& q1) {
    q0 = sm.b3[net][0]; q1 = sm.b3[net][1];
#pragma unroll
    for (int k = 0; k < MD_H2; ++k) {
        const float h = sm.h2[ev][k];
        q0 = __builtin_fmaf(sm.w3[net][0][k], h, q0);
        q1 = __builtin_fmaf(sm.w3[net][1][k], h, q1);
    }
}

// the soft-max quantities of (q0, q1) (mi_mdqn.h): v the maximum, u0 / u1 the scaled distances to it, lse = ln(e^u0 + e^u1); -ffp-contract=off keeps every
// product and sum its own
__device__ __forceinline__ void md_softmax(float q0, float q1, float it, float& v, float& u0, float& u1, float& lse) {
    v = fmaxf(q0, q1);
    u0 = (q0 - v) * it;
    u1 = (q1 - v) * it;
    lse = logf(expf(u0) + expf(u1));
}

// pass 1 of a row whose evaluations MD_TROW / MD_TGT are in sm, all through the TARGET head (every thread holds every result)
struct md_row_target { float bonus, soft, tgt; int next_action; };
__device__ __forceinline__ md_row_target md_target_value(const md_smem& sm, int a, float r, float lg, float alpha, float tau, float it, float clip_lo) {
    md_row_target o;
    float q0, q1, v, u0, u1, lse;
    md_values(sm, MD_TROW, MD_TARGET, q0, q1);
    md_softmax(q0, q1, it, v, u0, u1, lse);
    const float slp = tau * ((a ? u1 : u0) - lse);
    o.bonus = fminf(fmaxf(slp, clip_lo), 0.0f);
    md_values(sm, MD_TGT, MD_TARGET, q0, q1);
    md_softmax(q0, q1, it, v, u0, u1, lse);
    o.soft = v + tau * lse;
    o.next_action = q1 > q0 ? 1 : 0;   // torch.argmax: the first index on a tie
    o.tgt = (r + alpha * o.bonus) + lg * o.soft;
    return o;
}

// the successor of flat ring index i: ((slot + 1) % slots) * N + env
__device__ __forceinline__ long long md_successor(const mi_md_ring_t& ring, long long i, long long total) {
    const long long N = ring.n_envs;
    return i + N >= total ? i + N - total : i + N;
}

__global__ void __launch_bounds__(256) mdqn_target_kernel(mi_md_ring_t ring, mi_md_batch_t bt) {
    __shared__ md_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso tg;
    ts_load(tg, bt.target_params, t);
    md_load_head(sm, MD_TARGET, bt.target_params, t);
    const float it = 1.0f / bt.tau;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        long long i = bt.idx[b];
        i = i < 0 ? 0 : (i >= total ? total - 1 : i);   // a bad index reads a valid row, never past the ring
        const long long nx = md_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        md_torso_rows<false>(tg, tg, xi, xn, sm, t);
        const md_row_target o = md_target_value(sm, a, r, lg, bt.alpha, bt.tau, it, bt.clip_lo);
        if (t == 0) { bt.next_actions[b] = o.next_action; bt.target[b] = o.tgt; bt.bonus[b] = o.bonus; bt.soft_value[b] = o.soft; }
        // no barrier here: sm.h2 is next written behind two barriers of the next md_torso_rows, which no wave passes before all have read it
    }
}

__global__ void __launch_bounds__(256) mdqn_grad_kernel(mi_md_ring_t ring, mi_md_batch_t bt, float* __restrict__ slabs) {
    __shared__ md_smem sm;
    const int t = threadIdx.x;
    const long long total = ring.slots * (long long)ring.n_envs;
    ts_torso on, tg;   // the target network is loaded once and serves both of its passes
    ts_load(on, bt.params, t);
    ts_load(tg, bt.target_params, t);
    md_load_head(sm, MD_ONLINE, bt.params, t);
    md_load_head(sm, MD_TARGET, bt.target_params, t);
    float g3 = 0.0f, gb3 = 0.0f, loss = 0.0f;
    ts_grads g;
    ts_zero(g);
    const float inv = 1.0f / (float)bt.batch;
    const float it = 1.0f / bt.tau;
    const float* __restrict__ P = bt.params;
    for (int b = blockIdx.x; b < bt.batch; b += gridDim.x) {
        const long long i = rg_row_index(bt.sample_seed, bt.sample_update, bt.sample_upper, bt.idx, b, total, t == 0);
        const long long nx = md_successor(ring, i, total);
        const float4 xi = reinterpret_cast<const float4*>(ring.observations)[i];
        const float4 xn = reinterpret_cast<const float4*>(ring.observations)[nx];
        const int a = ring.actions[i] != 0 ? 1 : 0;
        const float r = ring.rewards[nx];
        const float lg = ring.terminated[nx] ? 0.0f : bt.gamma;
        md_torso_rows<true>(on, tg, xi, xn, sm, t);
        // ---- pass 1, the target network: the stored action's clipped log-policy at obs[i], the soft value at obs[nx] ----
        const md_row_target o = md_target_value(sm, a, r, lg, bt.alpha, bt.tau, it, bt.clip_lo);
        // ---- pass 2, obs[i]: the stored action's online value, the loss, the backward into register accumulators ----
        float c0, c1;
        md_values(sm, MD_ROW, MD_ONLINE, c0, c1);
        const float cur = a ? c1 : c0;
        const float td = o.tgt - cur;
        const float d = -((2.0f * td) * inv);
        if (t == 0) {
            bt.next_actions[b] = o.next_action; bt.target[b] = o.tgt; bt.bonus[b] = o.bonus; bt.soft_value[b] = o.soft; bt.current[b] = cur;
            loss += td * td;
        }
        // layer 3: thread a' * 84 + k owns dW3[a'][k], thread 168 + a' db3[a']; the other action's row is not touched
        if (t < 2 * MD_H2) {
            if (t / MD_H2 == a) g3 = __builtin_fmaf(d, sm.h2[MD_ROW][t % MD_H2], g3);
        } else if (t - 2 * MD_H2 == a) {
            gb3 += d;
        }
        if (t < MD_H2) sm.dz2[t] = sm.h2[MD_ROW][t] > 0.0f ? d * sm.w3[MD_ONLINE][a][t] : 0.0f;
        __syncthreads();
        ts_backward(g, sm.h1[MD_ROW], sm.dz2, sm.ph, xi, P, t);   // sm.h1 / sm.ph / sm.dz2 are then the next row's
    }
    // ---- the workgroup's slab ----
    float* const slab = slabs + (size_t)blockIdx.x * MD_STRIDE;
    if (t < 2 * MD_H2) slab[MD_W3 + t] = g3;
    else if (t < 2 * MD_H2 + 2) slab[MD_B3 + t - 2 * MD_H2] = gb3;
    ts_store(g, slab, t);
    if (t == 0) { slab[MD_NP] = loss; slab[MD_NP + 1] = 0.0f; }
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) mdqn_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                          float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                          rg_adam_consts k, int adam) {
    rg_reduce<MD_NP, MD_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
// the three hyper-parameters: tau and its reciprocal finite and positive (a subnormal tau would make 0 * inf of a tie), alpha finite, clip_lo <= 0 (NaN fails all)
template <class BATCH>
static int md_check_knobs(const BATCH* b) {
    RG_CHECK_ARG(b->tau > 0.0f && std::isfinite(b->tau) && std::isfinite(1.0f / b->tau), "tau must be > 0 and finite, and so must 1 / tau");
    RG_CHECK_ARG(std::isfinite(b->alpha), "alpha must be finite");
    RG_CHECK_ARG(b->clip_lo <= 0.0f, "clip_lo must be <= 0");
    return RG_OK;
}

extern "C" int mi_md_target(const mi_md_ring_t* ring, const mi_md_batch_t* b, void* stream) {
    int rc = rg_check_ring(ring);
    if (rc != MI_MD_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->target_params && b->idx && b->next_actions && b->target && b->bonus && b->soft_value && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->target_params), "target_params must be 16-byte aligned");
    rc = md_check_knobs(b);
    if (rc != MI_MD_OK) return rc;
    mdqn_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_MD_OK;
}

// mi_md_grad (update false: opt is not looked at) and mi_md_update
static int md_grad(const mi_md_ring_t* ring, const mi_md_batch_t* b, const mi_md_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_md_batch_t& bt) { return bt.current && bt.target && bt.bonus && bt.soft_value; });
    if (rc == RG_OK) rc = md_check_knobs(b);
    if (rc == RG_OK && update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<MD_NP>(mdqn_grad_kernel, mdqn_reduce_kernel, ring, b, md_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_md_grad(const mi_md_ring_t* ring, const mi_md_batch_t* b, void* stream) { return md_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_md_update(const mi_md_ring_t* ring, const mi_md_batch_t* b, const mi_md_adam_t* opt, void* stream) {
    return md_grad(ring, b, opt, true, (hipStream_t)stream);
}
