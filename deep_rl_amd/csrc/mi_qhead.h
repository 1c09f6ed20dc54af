// mi_qhead.h — the plain two-action head and the second half of a gradient row as one 256-thread workgroup holds them, shared by mi_ddqn.hip and mi_mdqn.hip: the
// head's layout, the LDS state of a row's three torso evaluations, the head loader, the two action values, the argmax, the ring successor, the three torso
// evaluations of a row, pass 2 of a gradient row (the stored action's value, td, the loss term, the head's gradient, dz2, the torso's backward), the slab epilogue
// and the clamped batch index of the target kernels.  Every `__global__`, every C entry point, pass 1 (what a row's target IS) and each library's own output
// stores stay in the library; nothing here knows which library includes it and nothing is exported: every entity is static or inline.
// Each library static_asserts its own MI_X_W3 / B3 / NPARAMS / SLAB_STRIDE against the offsets below.  Every sum keeps the order include/mi_ddqn.h states; FMAs
// are explicit.
#pragma once
#include "mi_torso.h"

#define QH_W3 10764            // the head behind the torso: W3 [2][84], b3 [2]
#define QH_B3 10932
#define QH_NP 10934            // parameters; a slab holds them, the row losses' sum and one float of padding
#define QH_STRIDE 10936
static_assert(QH_W3 == TS_B2 + TS_H2 && QH_B3 == QH_W3 + 2 * TS_H2 && QH_NP == QH_B3 + 2 && 2 * TS_H2 + 2 <= 256, "the head");
static_assert(QH_STRIDE % 4 == 0 && QH_STRIDE >= QH_NP + 2, "float4 stores");

// ---- the network as one workgroup holds it ------------------------------------------------------------
// the evaluations a workgroup keeps side by side: ROW the online network at obs[i]; what slots 1 and 2 hold is the library's (it names them)
enum { QH_ROW = 0, QH_EVALS = 3 };
enum { QH_ONLINE = 0, QH_TARGET = 1 };
struct qh_smem {
    float h1[QH_EVALS][TS_H1];
    float p2[QH_EVALS][3][TS_H2];       // layer 2's partial chains
    float h2[QH_EVALS][TS_H2];
    float w3[2][2][TS_H2];              // [network][action]: the heads
    float b3[2][2];
    float dz2[TS_H2];
    float ph[2][TS_H1];                 // the backward's partial chains of dh1
};

// the head of the parameters P into sm.w3[net] / sm.b3[net]; the caller's next barrier (every torso evaluation has three) publishes it
__device__ __forceinline__ void qh_load_head(qh_smem& sm, int net, const float* __restrict__ P, int t) {
    if (t < 2 * TS_H2) sm.w3[net][t / TS_H2][t % TS_H2] = P[QH_W3 + t];
    else if (t < 2 * TS_H2 + 2) sm.b3[net][t - 2 * TS_H2] = P[QH_B3 + t - 2 * TS_H2];
}

// layers 1 and 2: with S0 the torso w0 at x0 (-> sm.h1 / sm.h2 [0]), with S12 the torso w1 at x1 (-> [1]) and the torso w2 at x2 (-> [2]), all between the same
// three barriers; the results are valid for every thread when it returns.  No barrier has to follow what reads them: sm.h2 is next written behind two barriers of
// the next qh_torso_rows, which no wave passes before all have read it.
template <bool S0, bool S12>
__device__ __forceinline__ void qh_torso_rows(const ts_torso& w0, const float4 x0, const ts_torso& w1, const float4 x1, const ts_torso& w2, const float4 x2,
                                              qh_smem& sm, int t) {
    if (t < TS_H1) {
        if (S0) sm.h1[0][t] = ts_h1(w0, x0);
        if (S12) { sm.h1[1][t] = ts_h1(w1, x1); sm.h1[2][t] = ts_h1(w2, x2); }
    }
    __syncthreads();
    if (t < 3 * TS_H2) {
        const int c = t / TS_H2, o = t - c * TS_H2;
        if (S0) sm.p2[0][c][o] = ts_p2(w0, &sm.h1[0][TS_W2C * c]);
        if (S12) { sm.p2[1][c][o] = ts_p2(w1, &sm.h1[1][TS_W2C * c]); sm.p2[2][c][o] = ts_p2(w2, &sm.h1[2][TS_W2C * c]); }
    }
    __syncthreads();
    if (t < TS_H2) {
        if (S0) sm.h2[0][t] = ts_h2(sm.p2[0], t);
        if (S12) { sm.h2[1][t] = ts_h2(sm.p2[1], t); sm.h2[2][t] = ts_h2(sm.p2[2], t); }
    }
    __syncthreads();
}

// THE two action values (mi_ddqn.h) of evaluation `ev` through the head of network `net`, in every thread (two independent chains; the reads are workgroup-uniform
// broadcasts)
__device__ __forceinline__ void qh_values(const qh_smem& sm, int ev, int net, float& q0, float& q1) {
    q0 = sm.b3[net][0]; q1 = sm.b3[net][1];
#pragma unroll
    for (int k = 0; k < TS_H2; ++k) {
        const float h = sm.h2[ev][k];
        q0 = __builtin_fmaf(sm.w3[net][0][k], h, q0);
        q1 = __builtin_fmaf(sm.w3[net][1][k], h, q1);
    }
}
__device__ __forceinline__ int qh_argmax(float q0, float q1) { return q1 > q0 ? 1 : 0; }   // torch.argmax: the first index on a tie

// ---- the batch row ------------------------------------------------------------------------------------
// the successor of flat ring index i: ((slot + 1) % slots) * N + env
template <class RING>
__device__ __forceinline__ long long qh_successor(const RING& ring, long long i, long long total) {
    const long long N = ring.n_envs;
    return i + N >= total ? i + N - total : i + N;
}
// the batch index of a target kernel: a bad index reads a valid row, never past the ring
__device__ __forceinline__ long long qh_clamp_index(long long i, long long total) { return i < 0 ? 0 : (i >= total ? total - 1 : i); }

// a workgroup's register accumulators: the torso's, thread a' * 84 + k's dW3[a'][k] (g3), thread 168 + a''s db3[a'] (gb3) and, in thread 0, the loss
struct qh_grads { float g3, gb3, loss; ts_grads g; };
__device__ __forceinline__ void qh_zero(qh_grads& G) { G.g3 = 0.0f; G.gb3 = 0.0f; G.loss = 0.0f; ts_zero(G.g); }

// Pass 2 of one batch row into G, behind qh_torso_rows<true, ..> of it: the stored action a's online value at xi = obs[i], td against the row's target `tgt`, the
// loss term, the head's gradient, dz2, the torso's backward.  Thread 0 calls store(cur, td) where a row's outputs are written.  `inv` is 1 / batch, P the online
// parameters.  Three barriers (one behind dz2, ts_backward's two), the last ends it: sm's h1 / ph / dz2 are then the next row's.
template <class STORE>
__device__ __forceinline__ void qh_grad_row(qh_grads& G, qh_smem& sm, int a, float tgt, float inv, const float4 xi, const float* __restrict__ P, int t, STORE store) {
    float c0, c1;
    qh_values(sm, QH_ROW, QH_ONLINE, c0, c1);
    const float cur = a ? c1 : c0;
    const float td = tgt - cur;
    const float d = -((2.0f * td) * inv);
    if (t == 0) {
        store(cur, td);
        G.loss += td * td;
    }
    // layer 3: thread a' * 84 + k owns dW3[a'][k], thread 168 + a' db3[a']; the other action's row is not touched
    if (t < 2 * TS_H2) {
        if (t / TS_H2 == a) G.g3 = __builtin_fmaf(d, sm.h2[QH_ROW][t % TS_H2], G.g3);
    } else if (t - 2 * TS_H2 == a) {
        G.gb3 += d;
    }
    if (t < TS_H2) sm.dz2[t] = sm.h2[QH_ROW][t] > 0.0f ? d * sm.w3[QH_ONLINE][a][t] : 0.0f;
    __syncthreads();
    ts_backward(G.g, sm.h1[QH_ROW], sm.dz2, sm.ph, xi, P, t);
}

// the workgroup's slab: the head, the torso, the loss and the zeroed padding behind the parameters
__device__ __forceinline__ void qh_store(const qh_grads& G, float* __restrict__ slab, int t) {
    if (t < 2 * TS_H2) slab[QH_W3 + t] = G.g3;
    else if (t < 2 * TS_H2 + 2) slab[QH_B3 + t - 2 * TS_H2] = G.gb3;
    ts_store(G.g, slab, t);
    if (t == 0) { slab[QH_NP] = G.loss; slab[QH_NP + 1] = 0.0f; }
}
