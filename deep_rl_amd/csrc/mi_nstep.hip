// mi_nstep.hip — libmirl_nstep.so: n-step returns under prioritized dueling Double DQN on CartPole-v1 for gfx950.  C ABI and numerics contract: include/mi_nstep.h
// (and include/mi_pdd.h, which it refers to for everything but the target).
//
// The form of mi_pdd.hip: one 256-thread workgroup evaluates one batch row at a time with BOTH networks' torsos in its registers, the two 255-element dueling heads
// in LDS, and a row's three torso evaluations — online at obs[i], online at obs[s_m], target at obs[s_m] — between the same three barriers; the head's gradient is
// ONE accumulator per thread.  The kernels differ from mi_pdd.hip's only in where xn, r and lg come from: the walk of mi_nwalk.h, computed ahead of the row's first
// barrier by the two waves that need the bootstrap observation there (lane k loads step k + 1: one flag load and one reward load per walk; the observation at s_m is
// the one dependent load) and handed to the other waves through three LDS words that the row's first barrier publishes — it adds no barrier — and in the int32
// horizon they write out.  (The walk in every thread, with its 2 x 16 unrolled loads, spilled to scratch beside the two resident torsos: mi_nwalk.h.)
//   ns_target_kernel   pass 1 alone.
//   ns_grad_kernel     a workgroup walks its batch rows: the ring walk, pass 1 on obs[s_m], pass 2 on obs[i] — one slab per workgroup.
//   ns_reduce_kernel   fixed-order slab sum (+ Adam).
// There is no acting and no forward kernel: n-step returns change neither, an engine acts and evaluates through libmirl_pdd.so.
// pd_smem, pd_load_head, pd_torso_rows, pd_values, pd_argmax and pd_target_value are COPIES of mi_pdd.hip's (as mi_pdd.hip copied dd_torso_rows from mi_ddqn.hip):
// that library's sources are pinned by its id, sharing them is a change to mi_torso.h of its own.  The torso's layout, loader, per-thread pieces, backward and slab
// store are mi_torso.h's; the host side of the gradient entry points is mi_ring.h's.  All arithmetic on the VALU in fp32 with the summation orders of mi_pdd.h; no
// floating-point atomics, no inline assembly, no device-wide hand-off inside a launch.
// Uses mi_common.h read-only for the device helpers; none of its host-side macros (they call into libmirl.so).
#include "mi_common.h"
#include "mi_ring.h"
#include "mi_torso.h"
#include "mi_nwalk.h"

#include "../../include/mi_nstep.h"

#define PD_H1 MI_NS_H1
#define PD_H2 MI_NS_H2
#define PD_HEAD MI_NS_WV                      // the head's first element
#define PD_NHEAD (MI_NS_NPARAMS - MI_NS_WV)   // 255: Wv[84] bv Wa[2][84] ba[2]
#define PD_WV 0                               // offsets inside the head
#define PD_BV (MI_NS_BV - MI_NS_WV)
#define PD_WA (MI_NS_WA - MI_NS_WV)
#define PD_BA (MI_NS_BA - MI_NS_WV)
#define PD_NP MI_NS_NPARAMS
#define PD_STRIDE MI_NS_SLAB_STRIDE
static_assert(MI_NS_OK == RG_OK && MI_NS_EINVAL == RG_EINVAL && MI_NS_EHIP == RG_EHIP, "mi_ring.h returns these");
static_assert(MI_NS_W1 == TS_W1 && MI_NS_B1 == TS_B1 && MI_NS_W2 == TS_W2 && MI_NS_B2 == TS_B2 && MI_NS_H1 == TS_H1 && MI_NS_H2 == TS_H2, "mi_torso.h holds this torso");
static_assert(MI_NS_WV == TS_B2 + TS_H2 && MI_NS_BV == MI_NS_WV + PD_H2 && MI_NS_WA == MI_NS_BV + 1 && MI_NS_BA == MI_NS_WA + 2 * PD_H2 && PD_NP == MI_NS_BA + 2, "the head");
static_assert(PD_NHEAD == 255 && PD_NHEAD <= 256, "one head element per thread");
static_assert(PD_STRIDE % 4 == 0 && PD_STRIDE > PD_NP, "float4 stores");
static_assert(MI_NS_MAX_N == NW_MAX_N, "mi_nwalk.h walks this far");

#ifndef MI_NS_SOURCE_ID
#define MI_NS_SOURCE_ID "unknown"
#endif
extern "C" int mi_ns_version(void) { return MI_NS_VERSION; }
extern "C" const char* mi_ns_last_error(void) { return rg_err; }
extern "C" const char* mi_ns_source_id(void) { return MI_NS_SOURCE_ID; }
static int ns_slabs(int batch) { return rg_slabs(batch, MI_NS_MAX_SLABS); }
extern "C" size_t mi_ns_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return (size_t)ns_slabs(batch) * PD_STRIDE * sizeof(float);
}

// ---- the network as one workgroup holds it (mi_pdd.hip's, copied) -----------------------------------------
// the evaluations a workgroup keeps side by side: ROW the online network at obs[i], NEXT the online network at obs[s_m], TGT the target network at obs[s_m]
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

// pass 1 of a row whose evaluations PD_NEXT / PD_TGT are in sm: a* by the online head, the target network's value of a* (every thread holds both); r is the walk's
// reward sum R, lg its bootstrap factor
__device__ __forceinline__ void pd_target_value(const pd_smem& sm, float r, float lg, int& a_star, float& tgt) {
    float q0, q1, t0, t1;
    pd_values(sm, PD_NEXT, PD_ONLINE, q0, q1);
    pd_values(sm, PD_TGT, PD_TARGET, t0, t1);
    a_star = pd_argmax(q0, q1);
    tgt = r + lg * (a_star ? t1 : t0);   // -ffp-contract=off: a product, then a sum
}

// =====================================================================================================
// targets, loss, gradient
// =====================================================================================================
// what the walk of a row hands to the waves that do not compute it
struct ns_walk_lds { float R, lg; int m; int pad; };
// The walk of ring row i (mi_nwalk.h) in waves 0 and 1 — the waves whose threads t < PD_H1 read the bootstrap observation in layer 1 — and that observation, the
// one dependent load, for them (the other waves get zeros and never look at them).  Thread 0 leaves R, lg and m in `out`, which the first of the row's three torso
// barriers publishes; every thread reads them behind the third.  `out` alternates between two copies from row to row: a wave that is already past row b's last
// barrier writes the other copy, and the copy of row b is next written behind the three barriers of row b + 1, which no wave passes before all have read it.
__device__ __forceinline__ float4 ns_walk_row(const mi_ns_ring_t& ring, const mi_ns_batch_t& bt, long long i, long long total, ns_walk_lds& out, int t) {
    float4 xn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t < 128) {
        const nw_walk_t w = nw_walk(ring, i, total, bt.n_step, bt.head_slot, bt.gamma);
        xn = reinterpret_cast<const float4*>(ring.observations)[w.at];
        if (t == 0) { out.R = w.R; out.lg = w.lg; out.m = w.m; }
    }
    return xn;
}

__global__ void __launch_bounds__(256) ns_target_kernel(mi_ns_ring_t ring, mi_ns_batch_t bt) {
    __shared__ pd_smem sm;
    __shared__ ns_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
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
        const float4 xn = ns_walk_row(ring, bt, i, total, wk[par], t);
        pd_torso_rows<false, true>(on, tg, xn, xn, sm, t);
        int a_star; float tgt;
        pd_target_value(sm, wk[par].R, wk[par].lg, a_star, tgt);
        if (t == 0) { bt.next_actions[b] = a_star; bt.target[b] = tgt; bt.horizon[b] = wk[par].m; }
        par ^= 1;
    }
}

__global__ void __launch_bounds__(256) ns_grad_kernel(mi_ns_ring_t ring, mi_ns_batch_t bt, float* __restrict__ slabs) {
    __shared__ pd_smem sm;
    __shared__ ns_walk_lds wk[2];
    int par = 0;   // which of wk this row uses
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
        if (t < PD_H2) {
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
    if (t < PD_NHEAD) slab[PD_HEAD + t] = gh;
    ts_store(g, slab, t);
    if (t == 0) slab[PD_NP] = loss;
}

__global__ void __launch_bounds__(32 * RG_RED_GROUPS) ns_reduce_kernel(const float* __restrict__ slabs, int n_slabs, float inv, float* __restrict__ grads,
                                                                        float* __restrict__ loss, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                                        rg_adam_consts k, int adam) {
    rg_reduce<PD_NP, PD_STRIDE>(slabs, n_slabs, inv, grads, loss, p, m, v, k, adam);
}

// ---- C ABI -------------------------------------------------------------------------------------------
// the members only this library's batch has (a macro: the error text names the entry point that was called)
#define NS_CHECK_WALK(ring, b)                                                                                                                          \
    do {                                                                                                                                                \
        RG_CHECK_ARG((b)->horizon != nullptr, "horizon is NULL");                                                                                       \
        RG_CHECK_ARG((b)->n_step >= 1 && (b)->n_step <= MI_NS_MAX_N && (int64_t)(b)->n_step < (ring)->slots, "n_step must be in [1, 16] and below slots"); \
        RG_CHECK_ARG((b)->head_slot >= 0 && (b)->head_slot < (ring)->slots, "head_slot outside [0, slots)");                                            \
    } while (0)

extern "C" int mi_ns_target(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, void* stream) {
    const int rc = rg_check_ring(ring);
    if (rc != MI_NS_OK) return rc;
    RG_CHECK_ARG(b != nullptr, "batch is NULL");
    RG_CHECK_ARG(b->params && b->target_params && b->idx && b->next_actions && b->target && b->batch > 0, "bad arguments");
    RG_CHECK_ARG(rg_aligned(b->params) && rg_aligned(b->target_params), "params and target_params must be 16-byte aligned");
    NS_CHECK_WALK(ring, b);
    ns_target_kernel<<<b->batch < 1024 ? b->batch : 1024, 256, 0, (hipStream_t)stream>>>(*ring, *b);
    RG_HIP(hipGetLastError());
    return MI_NS_OK;
}

// mi_ns_grad (update false: opt is not looked at) and mi_ns_update
static int ns_grad(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, const mi_ns_adam_t* opt, bool update, hipStream_t s) {
    int rc = rg_check_batch(ring, b, INT_MAX, "batch <= 0", [](const mi_ns_batch_t& bt) { return bt.current && bt.target && bt.td_abs; });
    if (rc != RG_OK) return rc;
    NS_CHECK_WALK(ring, b);
    if (update) rc = rg_check_opt(opt);
    if (rc != RG_OK) return rc;
    return rg_launch_grad<PD_NP>(ns_grad_kernel, ns_reduce_kernel, ring, b, ns_slabs(b->batch), 1.0f / (float)b->batch, update ? opt : nullptr, s);
}
extern "C" int mi_ns_grad(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, void* stream) { return ns_grad(ring, b, nullptr, false, (hipStream_t)stream); }
extern "C" int mi_ns_update(const mi_ns_ring_t* ring, const mi_ns_batch_t* b, const mi_ns_adam_t* opt, void* stream) {
    return ns_grad(ring, b, opt, true, (hipStream_t)stream);
}
