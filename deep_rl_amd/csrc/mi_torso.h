// mi_torso.h — the 4 -> 120 -> 84 ReLU torso as one 256-thread workgroup holds it, shared by mi_c51.hip, mi_qr.hip and mi_ddqn.hip: the register layout (thread
// c * 84 + o a 40-wide third of row o of W2, thread u < 120 row u of W1), its loader, layers 1 and 2 forward, their backward from dz2 into register accumulators and
// the slab store of those.  Heads, losses, the formation of dz2 and every `__global__` stay in the library; nothing here knows which library includes it.
// Each library static_asserts its own MI_X_W1 .. B2 / H1 / H2 against the offsets below.  Every sum keeps the order its header (include/mi_*.h) states.
#pragma once

#define TS_H1 120
#define TS_H2 84
#define TS_W1 0                // parameter (and slab) offsets of the torso: W1 [120][4], b1 [120], W2 [84][120], b2 [84]
#define TS_B1 480
#define TS_W2 600
#define TS_B2 10680
#define TS_W2C 40              // columns of W2 per thread (three threads per row)
static_assert(TS_B1 == TS_W1 + 4 * TS_H1 && TS_W2 == TS_B1 + TS_H1 && TS_B2 == TS_W2 + TS_H2 * TS_H1 && 3 * TS_W2C == TS_H1 && 3 * TS_H2 <= 256, "the layout");
static_assert(TS_W1 % 4 == 0 && TS_W2 % 4 == 0 && TS_H1 % 4 == 0 && TS_W2C % 4 == 0, "float4 loads and stores");

struct ts_torso {
    float w2[TS_W2C]; float b2;         // thread c * 84 + o < 252: W2[o][40 c .. 40 c + 39]; b2 is the chain's start (the bias for c = 0, else 0)
    float w1[4]; float b1;              // thread u < 120
};

__device__ __forceinline__ void ts_load(ts_torso& w, const float* __restrict__ P, int t) {
    {
        const int tt = t < 3 * TS_H2 ? t : 3 * TS_H2 - 1;
        const int c = tt / TS_H2, o = tt - c * TS_H2;
        const float4* src = reinterpret_cast<const float4*>(P + TS_W2 + (size_t)o * TS_H1 + TS_W2C * c);   // 600, 120 and 40 are multiples of 4
#pragma unroll
        for (int k = 0; k < TS_W2C / 4; ++k) { const float4 v = src[k]; w.w2[4 * k] = v.x; w.w2[4 * k + 1] = v.y; w.w2[4 * k + 2] = v.z; w.w2[4 * k + 3] = v.w; }
        w.b2 = c == 0 ? P[TS_B2 + o] : 0.0f;
    }
    {
        const int u = t < TS_H1 ? t : TS_H1 - 1;
        const float4 v = reinterpret_cast<const float4*>(P + TS_W1)[u];
        w.w1[0] = v.x; w.w1[1] = v.y; w.w1[2] = v.z; w.w1[3] = v.w;
        w.b1 = P[TS_B1 + u];
    }
}

// ---- the per-thread pieces ---------------------------------------------------------------------------
// unit u = t < 120 of layer 1
__device__ __forceinline__ float ts_h1(const ts_torso& w, const float4 x) {
    float z = w.b1;
    z = __builtin_fmaf(w.w1[0], x.x, z); z = __builtin_fmaf(w.w1[1], x.y, z);
    z = __builtin_fmaf(w.w1[2], x.z, z); z = __builtin_fmaf(w.w1[3], x.w, z);
    return fmaxf(z, 0.0f);
}
// the 40-term partial chain of thread c * 84 + o < 252; h1c points at h1[40 c]
__device__ __forceinline__ float ts_p2(const ts_torso& w, const float* __restrict__ h1c) {
    float acc = w.b2;
#pragma unroll
    for (int k = 0; k < TS_W2C; ++k) acc = __builtin_fmaf(w.w2[k], h1c[k], acc);
    return acc;
}
// unit o = t < 84 of layer 2 from its three partial chains p2[c][o]
__device__ __forceinline__ float ts_h2(const float (&p2)[3][TS_H2], int o) { return fmaxf((p2[0][o] + p2[1][o]) + p2[2][o], 0.0f); }

// layers 1 and 2 of one row; SM has h1[120], p2[3][84], h2[84], all valid for every thread when it returns (three barriers, the third ends it)
template <class SM>
__device__ __forceinline__ void ts_row(const ts_torso& w, const float4 x, SM& sm, int t) {
    if (t < TS_H1) sm.h1[t] = ts_h1(w, x);
    __syncthreads();
    if (t < 3 * TS_H2) {
        const int c = t / TS_H2, o = t - c * TS_H2;
        sm.p2[c][o] = ts_p2(w, &sm.h1[TS_W2C * c]);
    }
    __syncthreads();
    if (t < TS_H2) sm.h2[t] = ts_h2(sm.p2, t);
    __syncthreads();
}

// ---- backward ----------------------------------------------------------------------------------------
struct ts_grads {
    float g2[TS_W2C]; float gb2;        // the threads of ts_torso own the same elements of the gradient (gb2: c = 0 only)
    float g1[4]; float gb1;
};
__device__ __forceinline__ void ts_zero(ts_grads& g) {
    g.g1[0] = 0.0f; g.g1[1] = 0.0f; g.g1[2] = 0.0f; g.g1[3] = 0.0f;
    g.gb2 = 0.0f; g.gb1 = 0.0f;
#pragma unroll
    for (int k = 0; k < TS_W2C; ++k) g.g2[k] = 0.0f;
}
// one row's layers 2 and 1 into g, from dz2[84] valid in LDS (the caller's barrier) and the row's h1[120] and input x; W2's columns come from the parameters P
// (consecutive threads, consecutive addresses), dh1 as two 42-row partial chains through ph.  Two barriers, the second ends it: h1, dz2 and ph are then free.
__device__ __forceinline__ void ts_backward(ts_grads& g, const float* h1, const float* dz2, float (&ph)[2][TS_H1], const float4 x,
                                            const float* __restrict__ P, int t) {
    if (t < 3 * TS_H2) {
        const int c = t / TS_H2, o = t - c * TS_H2;
        const float d = dz2[o];
        if (c == 0) g.gb2 += d;
#pragma unroll
        for (int k = 0; k < TS_W2C; ++k) g.g2[k] = __builtin_fmaf(d, h1[TS_W2C * c + k], g.g2[k]);
    }
    if (t < 2 * TS_H1) {
        const int c = t / TS_H1, k = t - c * TS_H1;
        const float* const col = P + TS_W2 + (size_t)(42 * c) * TS_H1 + k;   // rows 42 c .. 42 c + 41 of column k, in ascending order
        const float* const dz = dz2 + 42 * c;
        float acc = 0.0f;
        for (int o = 0; o < 42; ++o) acc = __builtin_fmaf(dz[o], col[(size_t)o * TS_H1], acc);
        ph[c][k] = acc;
    }
    __syncthreads();
    if (t < TS_H1) {
        const float d = h1[t] > 0.0f ? ph[0][t] + ph[1][t] : 0.0f;
        g.gb1 += d;
        g.g1[0] = __builtin_fmaf(d, x.x, g.g1[0]); g.g1[1] = __builtin_fmaf(d, x.y, g.g1[1]);
        g.g1[2] = __builtin_fmaf(d, x.z, g.g1[2]); g.g1[3] = __builtin_fmaf(d, x.w, g.g1[3]);
    }
    __syncthreads();
}

// the torso's part of a workgroup's slab (16-byte aligned: a slab's stride is a multiple of 4)
__device__ __forceinline__ void ts_store(const ts_grads& g, float* __restrict__ slab, int t) {
    if (t < 3 * TS_H2) {
        const int c = t / TS_H2, o = t - c * TS_H2;
        float4* const dst = reinterpret_cast<float4*>(slab + TS_W2 + (size_t)o * TS_H1 + TS_W2C * c);
#pragma unroll
        for (int k = 0; k < TS_W2C / 4; ++k) dst[k] = make_float4(g.g2[4 * k], g.g2[4 * k + 1], g.g2[4 * k + 2], g.g2[4 * k + 3]);
        if (c == 0) slab[TS_B2 + o] = g.gb2;
    }
    if (t < TS_H1) {
        reinterpret_cast<float4*>(slab + TS_W1)[t] = make_float4(g.g1[0], g.g1[1], g.g1[2], g.g1[3]);
        slab[TS_B1 + t] = g.gb1;
    }
}
