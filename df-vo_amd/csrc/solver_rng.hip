// numpy's global RandomState on the device: MT19937 seeding (np.random.seed) and the `repeat` shuffles of
// compute_pose_2d2d (/root/reference/libs/tracker/E_tracker.py:222-229: np.arange + np.random.shuffle per repeat).  The
// stream is one sequential chain; see tracker.h on sequential semantics.
#include "tracker.h"

namespace dfvo {

__global__ void k_mt_seed(uint32_t* __restrict__ st, uint32_t seed) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int pos = 0; pos < 624; pos++) {
        st[pos] = seed;
        seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)pos + 1u;
    }
    st[624] = 624;
}

// `repeat` consecutive draws of  perm = np.arange(n); np.random.shuffle(perm)  (n = info[0] on the device).
// MT19937 block regeneration (624 words, three dependency-free phases) and tempering run on all 256
// threads; the Fisher-Yates chain itself is sequential (masked rejection + data-dependent swaps) and runs
// on lane 0 out of LDS, handing control back whenever the block of tempered words is exhausted.
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}
__device__ __forceinline__ uint32_t mt_mix(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((uint32_t)(-(int32_t)(y & 1)) & 0x9908b0dfu);
}

__device__ __forceinline__ uint32_t mt_mask_of(uint32_t v) {
    v |= v >> 1;
    v |= v >> 2;
    v |= v >> 4;
    v |= v >> 8;
    v |= v >> 16;
    return v;
}

// Two phases per group of `group` repeats (as many as fit the LDS):
//  A  the masked-rejection draws  j_i = random_interval(i), i = n-1 .. 1  of every repeat, in stream order.
//     One sequential chain, run on wave 0 with every loop-carried value wave-uniform (v_readlane of a
//     64-word batch + scalar compare/branch), the MT19937 block regeneration + tempering on all threads.
//  B  the swap chains  p[i] <-> p[j_i]  of the repeats, one lane per repeat in lockstep out of LDS
//     (the repeats are independent once their j lists are known).
// snap (optional) [repeat + 1][MT_SNAP_STRIDE]: the stream's state before the first shuffle and behind each one -- where the
// reference would have raised in the middle of its repeat loop, the bookkeeping kernel hands the caller the state the
// reference left behind (mt_restore_after_raise).
__global__ __launch_bounds__(256) void k_mt_shuffle_all(uint32_t* __restrict__ st, const int* __restrict__ n_ptr,
                                                         int repeat, int group, int cap, int* __restrict__ perm_all,
                                                         uint32_t* __restrict__ snap) {
    __shared__ uint32_t key[624], outw[624];
    __shared__ int s_pos, s_rep, s_i;
    extern __shared__ int s_dyn[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int n = *n_ptr;
    if (snap)
        for (int i = t; i < 625; i += 256) snap[i] = st[i];
    if (n <= 1) {  // nothing is drawn
        if (t == 0 && n == 1)
            for (int r = 0; r < repeat; ++r) perm_all[(size_t)r * cap] = 0;
        if (snap)
            for (int r = 1; r <= repeat; ++r)
                for (int i = t; i < 625; i += 256) snap[(size_t)r * MT_SNAP_STRIDE + i] = st[i];
        return;
    }
    int* p = s_dyn;                                                      // [group][n]
    unsigned short* jl = reinterpret_cast<unsigned short*>(s_dyn + (size_t)group * n);  // [group][n]
    for (int i = t; i < 624; i += 256) {
        key[i] = st[i];
        outw[i] = mt_temper(st[i]);
    }
    if (t == 0) {
        s_pos = (int)st[624];
        s_rep = 0;
        s_i = n - 1;
    }
    __syncthreads();
    for (int g0 = 0; g0 < repeat; g0 += group) {
        const int g_end = g0 + group < repeat ? g0 + group : repeat;
        for (int i = t; i < (g_end - g0) * n; i += 256) p[i] = i % n;
        // ---- phase A
        for (;;) {
            if (t < 64) {
                int pos = __builtin_amdgcn_readfirstlane(s_pos);
                int rep = __builtin_amdgcn_readfirstlane(s_rep);
                int i = __builtin_amdgcn_readfirstlane(s_i);
                const unsigned long long lt = (1ull << lane) - 1ull;
                while (pos < 624 && rep < g_end) {
                    // a batch of up to 64 tempered words under one mask regime: word k is accepted iff
                    // (w_k & mask) <= i - c_k, c_k = accepts before k.  Solved as a fixed point of wave ballots:
                    // starting from the optimistic set the iterates alternate between super- and subsets of the
                    // answer and agree with it on a strictly growing prefix.
                    const int cnt = 624 - pos < 64 ? 624 - pos : 64;
                    const uint32_t mask = mt_mask_of((uint32_t)i);
                    const int lim = i - (int)(mask >> 1);  // accepts left before the mask shrinks (or the repeat ends)
                    const bool have = lane < cnt;
                    const uint32_t m = have ? (outw[pos + lane] & mask) : 0xffffffffu;
                    unsigned long long acc = __ballot(have && m <= (uint32_t)i);
                    for (;;) {
                        const int c = __popcll(acc & lt);
                        const unsigned long long nxt = __ballot(have && c < lim && m <= (uint32_t)(i - c));
                        if (nxt == acc) break;
                        acc = nxt;
                    }
                    const int c = __popcll(acc & lt);
                    if ((acc >> lane) & 1ull) jl[(rep - g0) * n + (i - c)] = (unsigned short)m;
                    const int total = __popcll(acc);
                    // the batch ends at the word that exhausted the regime, otherwise all words were consumed
                    const int used = total == lim ? 64 - __builtin_clzll(acc) : cnt;
                    pos += used;
                    i -= total;
                    if (i == 0) {
                        ++rep;
                        i = n - 1;
                        if (snap) {  // (wave-uniform branch) the state behind this repeat's shuffle
                            uint32_t* d = snap + (size_t)rep * MT_SNAP_STRIDE;
                            for (int k = lane; k < 624; k += 64) d[k] = key[k];
                            if (lane == 0) d[624] = (uint32_t)pos;
                        }
                    }
                }
                if (lane == 0) {
                    s_pos = pos;
                    s_rep = rep;
                    s_i = i;
                }
            }
            __syncthreads();
            if (s_rep >= g_end) break;
            // block regeneration: key[i] <- key[i+397 mod 624] ^ twist(key[i], key[i+1]) in three dependency-free
            // ranges [0,227) [227,454) [454,623), then word 623
            uint32_t v = 0;
            if (t < 227) v = mt_mix(key[t], key[t + 1], key[t + 397]);
            __syncthreads();
            if (t < 227) key[t] = v;
            __syncthreads();
            if (t < 227) v = mt_mix(key[227 + t], key[228 + t], key[t]);
            __syncthreads();
            if (t < 227) key[227 + t] = v;
            __syncthreads();
            if (t < 169) v = mt_mix(key[454 + t], key[455 + t], key[227 + t]);
            __syncthreads();
            if (t < 169) key[454 + t] = v;
            __syncthreads();
            if (t == 0) {
                key[623] = mt_mix(key[623], key[0], key[396]);
                s_pos = 0;
            }
            __syncthreads();
            for (int i = t; i < 624; i += 256) outw[i] = mt_temper(key[i]);
            __syncthreads();
        }
        // ---- phase B
        if (t < g_end - g0) {
            int* pr = p + (size_t)t * n;
            const unsigned short* jr = jl + (size_t)t * n;
            int i = n - 1;
            for (; i >= 8; i -= 8) {
                int jj[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) jj[u] = jr[i - u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int a = pr[jj[u]], b = pr[i - u];
                    pr[jj[u]] = b;
                    pr[i - u] = a;
                }
            }
            for (; i >= 1; --i) {
                const int j = jr[i];
                const int a = pr[j], b = pr[i];
                pr[j] = b;
                pr[i] = a;
            }
        }
        __syncthreads();
        for (int r = g0; r < g_end; ++r)
            for (int i = t; i < n; i += 256) perm_all[(size_t)r * cap + i] = p[(size_t)(r - g0) * n + i];
        __syncthreads();
    }
    for (int i = t; i < 624; i += 256) st[i] = key[i];
    if (t == 0) st[624] = (uint32_t)s_pos;
}

int enqueue_mt_seed(TrackerBuffers& tb, uint32_t seed, hipStream_t s) {
    hipLaunchKernelGGL(k_mt_seed, dim3(1), dim3(1), 0, s, tb.mt_state, seed);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// `repeat` x (perm = np.arange(n); np.random.shuffle(perm)) from the device-resident numpy stream `mt_state`;
// n = *d_n on the device (n_host bounds it), perm[r * perm_stride + i]
int enqueue_mt_shuffle(uint32_t* mt_state, const int* d_n, int n_host, int repeat, int perm_stride, int* perm,
                       hipStream_t s, uint32_t* snap) {
    const size_t per_rep = 6 * (size_t)(n_host > 0 ? n_host : 1);  // int permutation + uint16 draw list
    DFVO_ARG_CHECK(per_rep <= 144 * 1024, "shuffle: too many keypoints for the LDS permutation buffer");
    int group = (int)((144 * 1024) / per_rep);
    if (group > repeat) group = repeat;
    const size_t perm_lds = per_rep * group + 16;
    if (int rc_lds = ensure_dyn_lds((const void*)k_mt_shuffle_all, perm_lds)) return rc_lds;
    hipLaunchKernelGGL(k_mt_shuffle_all, dim3(1), dim3(256), perm_lds, s, mt_state, d_n, repeat, group, perm_stride, perm, snap);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

}  // namespace dfvo
