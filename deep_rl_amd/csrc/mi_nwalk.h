// mi_nwalk.h — the n-step walk along the replay ring (include/mi_nstep.h: the numerics contract), as a device header for the ring-replay libraries that form a
// multi-step target: libmirl_nstep.so today, a Rainbow library later.  It needs the including library's ring struct by its member names only (rewards, terminated,
// n_envs: the layout of mi_ring.h's rings) and nothing of the host.
//
// From the flat ring index i of a batch row it gives the flat index of the bootstrap observation s_m, the discounted reward sum R, the bootstrap's factor lg and the
// number of steps m taken:
//     s_1 = succ(s_0); R = r[s_1]; g = gamma; m = 1
//     while m < n and terminated[s_m] == 0 and s_m != head: m += 1; s_m = succ(s_{m-1}); R = R + g * r[s_m]; g = g * gamma          (a product, then a sum)
//     lg = terminated[s_m] ? 0 : g
//
// Form.  ONE WAVE computes it: nw_walk is called by all 64 lanes of a wave with wave-uniform operands and returns the same result in every lane.  Lane k holds step
// k + 1: its cell's address is i + (k + 1) N (mod the ring), so all n flag loads and all n reward loads are ONE load instruction each, issued before anything is
// looked at — every address is inside the ring (n < slots: the n successors are n distinct cells), so loading beyond the stop is safe — and the walk is one memory
// latency deep, not n.  The stop is the first set bit of a ballot over "terminated or on the head"; the reward sum then takes the m rewards in step order from their
// lanes (v_readlane), so a reward beyond the stop is never multiplied by zero: it is never read out of its lane, and it may be NaN.  Lanes k >= n repeat step n's
// address and are masked out of the ballot.  The observation at s_m is the caller's one dependent load.  No LDS, no barrier.
// (The first form of this header computed the walk in every thread of the workgroup with 2 x 16 unrolled loads; beside the two resident torsos of the gradient
// kernel that spilled 86 SGPRs and 4 VGPRs to scratch.  A library whose kernels need the result in every wave publishes it through LDS behind a barrier its row
// already has: mi_nstep.hip.)
// With n == 1 the result is (succ(i), r[succ(i)], terminated[succ(i)] ? 0 : gamma, 1) whatever `head` is: the one-step target's operands, expression for expression.
//
// Limitation: `terminated` excludes TimeLimit truncation and the ring stores no truncation flag (mi_ring.h: rg_act_loop), so a walk runs on through a truncation into
// the reset observation and the rewards behind it, exactly as the one-step target bootstraps from the reset observation there.
#pragma once

#define NW_MAX_N 16   // the most steps a walk takes (MI_NS_MAX_N); a wave has 64 lanes, one per step

struct nw_walk_t {
    long long at;   // flat ring index of s_m: where the bootstrap observation lies
    float R;        // r_1 + gamma r_2 + ... + gamma^(m-1) r_m
    float lg;       // gamma^m, or 0 when step m terminated
    int m;          // steps taken, 1 .. n
};

// i in [0, total), total = slots * n_envs, 1 <= n <= NW_MAX_N, n < slots, head in [0, slots): the slot of the newest observation (no action taken from it yet).
// All 64 lanes of the calling wave must be active and hold the same operands.
template <class RING>
__device__ __forceinline__ nw_walk_t nw_walk(const RING& ring, long long i, long long total, int n, long long head, float gamma) {
    static_assert(NW_MAX_N <= 64, "one lane per step");
    const long long N = ring.n_envs;
    const int lane = (int)(threadIdx.x & 63u);
    const int step = lane < n ? lane + 1 : n;                 // lanes past n repeat step n
    long long j = i + (long long)step * N;                    // step * N < total: one wrap at the most
    j = j >= total ? j - total : j;
    const float r = ring.rewards[j];
    const unsigned char f = ring.terminated[j];
    const long long h = j - head * N;                         // the head's cells are head * N .. head * N + N - 1
    const bool stop = f != 0 || (h >= 0 && h < N);
    // step n stops whatever it holds; bits past n are dropped
    const unsigned long long stops = (__builtin_amdgcn_ballot_w64(stop) | (1ull << (n - 1))) & (~0ull >> (64 - n));
    nw_walk_t w;
    w.m = __builtin_ctzll(stops) + 1;
    w.R = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), 0));
    float g = gamma;
    for (int k = 1; k < w.m; ++k) {                           // wave-uniform trip count
        const float rk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), k));
        w.R = w.R + g * rk;                                   // -ffp-contract=off: a product, then a sum
        g = g * gamma;
    }
    w.lg = __builtin_amdgcn_readlane((int)f, w.m - 1) != 0 ? 0.0f : g;
    w.at = i + (long long)w.m * N;
    w.at = w.at >= total ? w.at - total : w.at;
    return w;
}
