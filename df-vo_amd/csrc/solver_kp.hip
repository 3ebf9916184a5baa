// Keypoint selection of the tracker: local_bestN, bestN_flow_kp, the rigid-flow keypoints and the sampled keypoints.
// Reference call sites (paths relative to /root/reference):
//   libs/matching/kp_selection.py:33-71,74-200    bestN_flow_kp, local_bestN
//   libs/matching/kp_selection.py:203-378         opt_rigid_flow_kp, sampled_kp
//   libs/matching/keypoint_sampler.py:76-163      kp1 = pixel grid, kp2 = kp1 + flow
// np.argpartition's order is kept by running numpy's own selection (kp_select.h); see tracker.h on sequential
// semantics.  Built with -ffp-contract=off.
#include "kp_select.h"
#include "np_legacy.h"   // sm::rigid_flow_px
#include "ransac_dev.h"  // wave_sum
#include "tracker.h"

namespace dfvo {

// ------------------------------------------------------------------------------------------------
// numpy's introselect with the long partition passes run by the whole 256-thread workgroup.
// One pass of the unguarded Hoare partition  for(;;){ do ll++ while(v[ll]<p); do hh-- while(p<v[hh]); if(hh<ll)
// break; swap }  is equivalent to: L_k = k-th position (ascending, from low+2) whose value is not < pivot, R_k =
// k-th position (descending, from high-1) whose value is not > pivot; swap (L_k, R_k) for every k with L_k <= R_k
// (K of them, the pairs are disjoint); the scans of the crossing iteration stop at min(L_K, R_{K-1}) and
// max(R_K, L_{K-1}) because the slots exchanged last now hold stoppers.  The stopper lists are built with an
// ordered ballot/scan compaction, K by a count, the swaps one pair per thread.  Pivot choice, bookkeeping and the
// final short ranges stay on thread 0 (sm::kp_introselect_cp_from), so the resulting order is numpy's.
// ------------------------------------------------------------------------------------------------
constexpr int KP_PAR_MIN = 256;  // ranges shorter than this finish sequentially

// exclusive scan of `v` over the 256 threads; *total = the grand total.  (Two 16-bit counters packed into one int scan
// as two independent sums while neither overflows.)
__device__ __forceinline__ int kp_block_excl_scan(int v, int* s_wsum /*4 ints*/, int* total) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; w++) base += s_wsum[w];
    *total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    __syncthreads();
    return base + inc - v;
}

// Pos = unsigned short: key / tosort / Lpos / Rpos live in LDS and a cell has fewer than 65536 candidates (k_kp_cell,
// k_kp_cell_rigid); the two stopper counts share one packed scan.  Pos = int: the arrays live in global memory and are too
// long for 16-bit positions (k_bestn_select selects over the whole image); two plain scans, and a block-level fence in
// front of every barrier that hands global writes to other threads.
template <typename Pos>
__device__ void kp_introselect_block(float* key, Pos* tosort, int num, int kth, Pos* Lpos, Pos* Rpos, int* s_ctl /*8 ints*/,
                                     int* s_wsum /*4 ints*/) {
    constexpr bool in_global = sizeof(Pos) == 4;
    const int t = threadIdx.x;
    if (kth < 3 || kth == num - 1 || num < KP_PAR_MIN) {  // shortcuts of the scalar algorithm / small inputs
        if (t == 0) sm::kp_introselect_cp<Pos>(key, tosort, num, kth, 0);
        __syncthreads();
        return;
    }
    auto swap = [&](int i, int j) {
        const Pos ti = tosort[i];
        tosort[i] = tosort[j];
        tosort[j] = ti;
        const float ki = key[i];
        key[i] = key[j];
        key[j] = ki;
    };
    int low = 0, high = num - 1, depth_limit = sm::kp_msb((unsigned)num) * 2;
    while (low + 1 < high) {
        if (high - low < KP_PAR_MIN || depth_limit <= 0) break;  // thread 0 finishes (incl. the median-of-medians path)
        if (t == 0) {  // median of three -> pivot at low, its companion at low + 1
            const int mid = low + (high - low) / 2;
            if (sm::kp_lt(key[high], key[mid])) swap(high, mid);
            if (sm::kp_lt(key[high], key[low])) swap(high, low);
            if (sm::kp_lt(key[low], key[mid])) swap(low, mid);
            swap(mid, low + 1);
        }
        if constexpr (in_global) __threadfence_block();
        __syncthreads();
        const float pivot = key[low];
        // stopper lists over [low+1 .. high]: left stoppers from low+2 (high is one by construction), right stoppers
        // down from high-1 (low+1 is one by construction); each thread owns a contiguous segment
        const int r0 = low + 1, n_r = high - low;  // positions r0 .. r0 + n_r - 1
        const int seg = (n_r + 255) / 256;
        const int p0 = r0 + t * seg, p1 = p0 + seg < r0 + n_r ? p0 + seg : r0 + n_r;
        int cl = 0, cr = 0;
        for (int p = p0; p < p1; ++p) {
            const float v = key[p];
            cl += (p >= low + 2 && !sm::kp_lt(v, pivot)) ? 1 : 0;
            cr += (p <= high - 1 && !sm::kp_lt(pivot, v)) ? 1 : 0;
        }
        int nL, nR, il, ir;
        if constexpr (in_global) {
            il = kp_block_excl_scan(cl, s_wsum, &nL);
            ir = kp_block_excl_scan(cr, s_wsum, &nR);
        } else {
            int total;
            const int ex = kp_block_excl_scan(cl | (cr << 16), s_wsum, &total);
            nL = total & 0xffff, nR = total >> 16;
            il = ex & 0xffff, ir = ex >> 16;
        }
        for (int p = p0; p < p1; ++p) {
            const float v = key[p];
            if (p >= low + 2 && !sm::kp_lt(v, pivot)) Lpos[il++] = (Pos)p;
            if (p <= high - 1 && !sm::kp_lt(pivot, v)) Rpos[nR - 1 - (ir++)] = (Pos)p;
        }
        if constexpr (in_global) __threadfence_block();
        __syncthreads();
        // K = number of leading pairs with L_k <= R_k (monotone predicate)
        const int npair = nL < nR ? nL : nR;
        int cnt = 0;
        for (int k = t; k < npair; k += 256) cnt += Lpos[k] <= Rpos[k] ? 1 : 0;
        int K;
        (void)kp_block_excl_scan(cnt, s_wsum, &K);
        if constexpr (!in_global) K &= 0xffff;
        for (int k = t; k < K; k += 256) {
            const int a = Lpos[k], b = Rpos[k];
            if (a != b) swap(a, b);
        }
        if constexpr (in_global) __threadfence_block();
        __syncthreads();
        if (t == 0) {
            // crossing iteration: the scans run on from (L_{K-1}, R_{K-1}) and stop at the next original stopper or at
            // the nearest slot exchanged earlier (it now holds a stopper), whichever comes first.  When the last
            // exchanged pair was a self-pair (L == R, value == pivot) that slot lies behind both scans and the
            // pair before it takes its place.  K < nL, nR: the lists end with the sentinels high / low+1.
            int ll = Lpos[K], hh = Rpos[K];
            if (K > 0) {
                int rp = Rpos[K - 1], lp = Lpos[K - 1];
                if (rp == lp) {
                    rp = K > 1 ? Rpos[K - 2] : 0x7fffffff;
                    lp = K > 1 ? Lpos[K - 2] : -1;
                }
                ll = ll < rp ? ll : rp;
                hh = hh > lp ? hh : lp;
            }
            swap(low, hh);
            int nlow = low, nhigh = high;
            if (hh >= kth) nhigh = hh - 1;
            if (hh <= kth) nlow = ll;
            s_ctl[0] = nlow;
            s_ctl[1] = nhigh;
        }
        if constexpr (in_global) __threadfence_block();
        __syncthreads();
        low = s_ctl[0];
        high = s_ctl[1];
        depth_limit--;
        __syncthreads();
    }
    if (t == 0) sm::kp_introselect_cp_from<Pos>(key, tosort, kth, 0, low, high, depth_limit);
    __syncthreads();
}

// bestN_flow_kp (kp_selection.py:33-71, ablation_correspondences_best_n.yml): np.where(flow_diff >= 0) keeps every
// non-NaN pixel in row-major order; np.argpartition(values, N)[:N] then picks N of them in introselect order
__global__ void k_bestn_fill(const float* __restrict__ diff, int n, float* __restrict__ key, int* __restrict__ tosort,
                             int* __restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int ok = 0;
    if (i < n) {
        const float v = diff[i];
        key[i] = v;
        tosort[i] = i;
        ok = v >= 0.f ? 1 : 0;
    }
    const int c = wave_sum(ok);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// one workgroup: (only when some pixels fail `>= 0`) ordered compaction, then the selection and the gather of the
// first N picks; info[0] = number of keypoints (0 when the image has N or fewer candidates: numpy would raise)
__global__ __launch_bounds__(256) void k_bestn_select(const float* __restrict__ diff, const float* __restrict__ flow, int H,
                                                       int W, int N, float* __restrict__ key, int* __restrict__ tosort,
                                                       int* __restrict__ map, int* __restrict__ Lpos, int* __restrict__ Rpos,
                                                       const int* __restrict__ count, double* __restrict__ kp1,
                                                       double* __restrict__ kp2, int* __restrict__ info, int tracker_info) {
    // tracker_info: info is a tracker's kp_info [n, good_kp_found, regions] and not the one-int result size
    __shared__ int s_ctl[8], s_wsum[4], s_base;
    const int t = threadIdx.x;
    const int n = H * W;
    int cnt = *count;
    const bool identity = cnt == n;
    if (!identity) {  // ordered compaction of the pixels that pass `>= 0`
        if (t == 0) s_base = 0;
        __syncthreads();
        for (int c0 = 0; c0 < n; c0 += 256) {
            const int e = c0 + t;
            const float v = e < n ? diff[e] : -1.f;
            const int f = (e < n && v >= 0.f) ? 1 : 0;
            int tot;
            const int ex = kp_block_excl_scan(f, s_wsum, &tot);
            if (f) {
                const int pos = s_base + ex;
                key[pos] = v;
                tosort[pos] = pos;
                map[pos] = e;
            }
            __syncthreads();
            if (t == 0) s_base += tot;
            __syncthreads();
        }
        cnt = s_base;
    }
    if (cnt <= N) {  // kth = N out of bounds
        if (t == 0) {
            info[0] = 0;
            if (tracker_info) info[1] = info[2] = 0;
        }
        return;
    }
    __threadfence_block();
    __syncthreads();
    kp_introselect_block(key, tosort, cnt, N, Lpos, Rpos, s_ctl, s_wsum);
    __threadfence_block();
    __syncthreads();
    for (int i = t; i < N; i += 256) {
        const int c = tosort[i];
        const int e = identity ? c : map[c];
        const int y = e / W, x = e - y * W;
        kp1[i * 2] = (double)x;
        kp1[i * 2 + 1] = (double)y;
        kp2[i * 2] = (double)x + (double)flow[e];
        kp2[i * 2 + 1] = (double)y + (double)flow[(size_t)n + e];
    }
    if (t == 0) {
        info[0] = N;
        if (tracker_info) {
            info[1] = 1;  // keypoint_sampler.py:96: only local_bestN clears good_kp_found
            info[2] = 0;
        }
    }
}

int enqueue_bestn_flow_kp(BestNBuffers& bb, const float* d_flow, const float* d_diff, int H, int W, int N, hipStream_t s,
                          double* d_kp1, double* d_kp2, int* d_info) {
    DFVO_ARG_CHECK(H > 0 && W > 0 && N >= 1 && (long long)H * W < (1ll << 30), "bestN: bad size");
    DFVO_ARG_CHECK((d_kp1 != nullptr) == (d_kp2 != nullptr) && (d_kp1 != nullptr) == (d_info != nullptr),
                   "bestN: the destination is kp1, kp2 and info together");
    const int n = H * W;
    if (int rc = bb.ensure((size_t)n, d_kp1 ? 0 : N)) return rc;
    float* key = bb.key_base + 8;
    DFVO_HIP_CHECK(hipMemsetAsync(bb.count, 0, sizeof(int) * 4, s));
    hipLaunchKernelGGL(k_bestn_fill, dim3(cdiv(n, 256)), dim3(256), 0, s, d_diff, n, key, bb.tosort, bb.count);
    hipLaunchKernelGGL(k_bestn_select, dim3(1), dim3(256), 0, s, d_diff, d_flow, H, W, N, key, bb.tosort, bb.map, bb.Lpos,
                       bb.Rpos, bb.count, d_kp1 ? d_kp1 : bb.kp, d_kp1 ? d_kp2 : bb.kp + 2 * (size_t)N, d_kp1 ? d_info : bb.count + 1,
                       d_kp1 ? 1 : 0);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// one 256-thread block per grid cell: ordered (row-major) compaction of the candidates into LDS, then
// lane 0 runs numpy's introselect on them (keys carried along with the indices, see kp_select.h); writes
// the picked local indices in argpartition order.
// Blocks [cells, cells + KP_CNT_BLOCKS) do not select: they count the pixels of the whole consistency map `mask_map` under the
// threshold (kp_selection.py:158: mask.sum() < N * 0.1 -> "not enough keypoints") into count_partial[], which k_kp_gather adds up
// (round 6: was a memset + k_kp_count in front of this launch, two more dependent launches on the path to the first pose).
__global__ __launch_bounds__(256) void k_kp_cell(const float* __restrict__ diff, int H, int W, int num_row, int num_col,
                                                  float thre, int n_best, int cap, int* __restrict__ cell_count,
                                                  int* __restrict__ cell_sel /*[cells][n_best] (y<<16|x)*/,
                                                  unsigned short* __restrict__ lidx_all /*[cells][cap]*/, int par,
                                                  const float* __restrict__ mask_map, int* __restrict__ count_partial,
                                                  const float* __restrict__ depth_diff /*nullable*/, float depth_thre) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    if ((int)blockIdx.x >= num_row * num_col) {
        __shared__ int s_cnt[4];
        const int b = blockIdx.x - num_row * num_col, n = H * W;
        int c = 0;
        for (int i = b * 256 + threadIdx.x; i < n; i += KP_CNT_BLOCKS * 256) c += mask_map[i] < thre ? 1 : 0;
        c = wave_sum(c);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) count_partial[b] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        return;
    }
    float* vals = reinterpret_cast<float*>(smem_raw) + 4;  // 4 floats of slack on either side: the 4-wide scans over-read
    unsigned short* tosort = reinterpret_cast<unsigned short*>(vals + cap + 4);
    unsigned short* Lpos = tosort + cap + 2;  // stopper lists of the workgroup-parallel partition (par != 0)
    unsigned short* Rpos = Lpos + cap + 2;
    __shared__ int s_ctl[8], s_wsum[4];
    unsigned short* lidx = lidx_all + (size_t)blockIdx.x * cap;  // candidate -> tile element (global scratch)
    __shared__ int s_base, s_wave[4];
    const int cell = blockIdx.x;
    const int row = cell / num_col, col = cell - row * num_col;
    int y0, y1, x0, x1;
    sm::kp_cell_bounds(H, W, num_row, num_col, row, col, &y0, &y1, &x0, &x1);
    const int th = sm::kp_slice_len(y0, y1, H), tw = sm::kp_slice_len(x0, x1, W);
    const int total = th * tw;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    // the cell's values in batches of eight loads per thread (round 6: one load per compaction step left eighteen dependent
    // round trips to memory in front of the selection of a KITTI-sized cell)
    constexpr int KB = 8;
    float vb[KB];
    // depth_diff (kp_selection.depth_consistency, kp_selection.py:145-148): a candidate must also lie under depth_thre in
    // that map -- bit u of dmask: element u of the batch does; the ranking key stays the score alone
    unsigned dmask = ~0u;
    for (int c0 = 0; c0 < total; c0 += 256) {
        const int e = c0 + t;
        const int slot = (c0 / 256) % KB;
        if (slot == 0) {
            if (depth_diff) dmask = 0u;
#pragma unroll
            for (int u = 0; u < KB; ++u) {
                const int eu = c0 + u * 256 + t;
                vb[u] = 0.f;
                if (eu < total) {
                    const int ly = eu / tw, lx = eu - ly * tw;
                    vb[u] = diff[(size_t)(y0 + ly) * W + x0 + lx];
                    if (depth_diff) dmask |= (depth_diff[(size_t)(y0 + ly) * W + x0 + lx] < depth_thre ? 1u : 0u) << u;
                }
            }
        }
        bool f = false;
        float v = 0.f;
        if (e < total) {
            v = vb[0];
#pragma unroll
            for (int u = 1; u < KB; ++u) v = slot == u ? vb[u] : v;
            f = v < thre && ((dmask >> slot) & 1u);
        }
        const unsigned long long b = __ballot(f);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; w++) off += s_wave[w];
        if (f) {
            const int pos = off + before;
            vals[pos] = v;
            tosort[pos] = (unsigned short)pos;
            lidx[pos] = (unsigned short)e;
        }
        __syncthreads();
        if (t == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    const int cnt = s_base;
    const int pick = cnt < n_best ? cnt : n_best;
    if (pick > 0) {
        if (par) {
            kp_introselect_block(vals, tosort, cnt, pick - 1, Lpos, Rpos, s_ctl, s_wsum);
        } else if (t == 0) {
            sm::kp_introselect_cp<unsigned short>(vals, tosort, cnt, pick - 1, 0);
        }
    }
    if (t == 0) cell_count[cell] = pick;
    __syncthreads();
    if (t < pick) {
        const int e = lidx[tosort[t]];
        const int ly = e / tw, lx = e - ly * tw;
        cell_sel[cell * n_best + t] = ((y0 + ly) << 16) | (x0 + lx);
    }
}

// concatenate the cells (row-major cell order), build kp1 (pixel grid) and kp2 = kp1 + flow.  count_partial (optional): the
// KP_CNT_BLOCKS partial counts of k_kp_cell's counting blocks, else *total_good is the count.  (Round 6: the cell counts go to
// LDS in one parallel read and the (cell, k) items are spread over the threads -- the loop over the cells with a dependent
// global read each was 45 us of one workgroup.)
__global__ __launch_bounds__(256) void k_kp_gather(const int* __restrict__ cell_count, const int* __restrict__ cell_sel,
                                                    int cells, int n_best, const float* __restrict__ flow, int H, int W,
                                                    const int* __restrict__ total_good, const int* __restrict__ count_partial,
                                                    int min_total, int min_regions,
                                                    double* __restrict__ kp1, double* __restrict__ kp2,
                                                    int* __restrict__ info /*[n, good_kp_found, regions]*/,
                                                    const int* __restrict__ skip) {
    __shared__ int s_off[1025], s_cnt[1024], s_good;
    if (skip && *skip) return;  // (the iterative scale loop's rounds behind its last one)
    const int t = threadIdx.x;
    for (int c = t; c < cells; c += 256) s_cnt[c] = cell_count[c];
    __syncthreads();
    if (t == 0) {
        int acc = 0, regions = 0;
        for (int c = 0; c < cells; c++) {
            s_off[c] = acc;
            acc += s_cnt[c];
            regions += s_cnt[c] != 0;
        }
        s_off[cells] = acc;
        int good = 0;
        if (count_partial)
            for (int b = 0; b < KP_CNT_BLOCKS; ++b) good += count_partial[b];
        else
            good = *total_good;
        const bool enough = !(good < min_total);            // (mask.sum() < N*0.1) -> fail
        const bool diverse = !(regions < min_regions);      // good_region_cnt < rows*cols*0.1 -> fail
        info[0] = (enough && diverse) ? acc : 0;
        info[1] = (enough && diverse) ? 1 : 0;
        info[2] = regions;
        s_good = (enough && diverse) ? 1 : 0;
    }
    __syncthreads();
    if (!s_good) return;
    for (int i = t; i < cells * n_best; i += 256) {
        const int c = i / n_best, k = i - c * n_best;
        if (k < s_cnt[c]) {
            const int code = cell_sel[i];
            const int y = code >> 16, x = code & 0xffff;
            const int o = s_off[c] + k;
            kp1[o * 2] = (double)x;
            kp1[o * 2 + 1] = (double)y;
            kp2[o * 2] = (double)x + (double)flow[(size_t)y * W + x];
            kp2[o * 2 + 1] = (double)y + (double)flow[(size_t)H * W + (size_t)y * W + x];
        }
    }
}

// ================================================================================================
// rigid-flow keypoints (RigidFlow layer + opt_rigid_flow_kp, the "kp_depth" correspondences of
// scale_recovery.method iterative / the extended-paper configurations)
// ================================================================================================
// RigidFlow(depth, T, K, inv_K, normalized=False) (geometry/rigid_flow.py, backprojection.py:56-62,
// transformation3d.py:29, projection.py:46-52, layers.py PixToFlow:262) and its distance to the optical flow
// (E_tracker.py:685-689), all in float32.  Every matmul row is a short dot product that torch's CPU GEMM evaluates as
// a0*b0 rounded, then fused multiply-adds in ascending k; written out the same way, the result is bit-identical to the
// torch-CPU oracle.  Kinv: 3x3, T: 4x4, K: 3x3 (its 4th column in the reference is zero).
__global__ void k_rigid_flow_diff(const float* __restrict__ depth, const float* __restrict__ flow, int H, int W,
                                  const float* __restrict__ mats /*Kinv[9] | T[16] | K[9]*/, float* __restrict__ rdiff,
                                  float* __restrict__ rflow /*optional [2,H,W]*/, const int* __restrict__ skip) {
    if (skip && *skip) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const float x = (float)(i % W), y = (float)(i / W);
    float rx, ry;
    sm::rigid_flow_px(mats, mats + 9, mats + 25, x, y, depth[i], &rx, &ry);
    if (rflow) {
        rflow[i] = rx;
        rflow[(size_t)H * W + i] = ry;
    }
    const float dx = rx - flow[i], dy = ry - flow[(size_t)H * W + i];
    rdiff[i] = sqrtf(dx * dx + dy * dy);  // np.linalg.norm(axis=0) on float32: sqrt(x*x + y*y), each step rounded
}

// opt_rigid_flow_kp (kp_selection.py:203-324), one workgroup per grid cell: candidates = pixels of the cell (last row /
// column dropped) with rigid-flow distance < thr_r AND forward-backward distance < thr_o, in row-major order;
// "uniform" picks every step-th candidate, "best" the num_to_pick smallest scores in numpy's argpartition order.
// uniform_only: the selection of the "best" set is left out and cell_sel is not written (scale_recovery_iterative reads the
// uniform set alone, E_tracker.py:541-542; the two sets have the same count per cell)
__global__ __launch_bounds__(256) void k_kp_cell_rigid(const float* __restrict__ odiff, const float* __restrict__ rdiff,
                                                        int H, int W, int num_row, int num_col, float thr_o, float thr_r,
                                                        int score_rigid, int n_best, int cap, int* __restrict__ cell_count,
                                                        int* __restrict__ cell_sel, int* __restrict__ cell_sel_uni,
                                                        unsigned short* __restrict__ lidx_all, int par, int uniform_only,
                                                        const int* __restrict__ skip) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* vals = reinterpret_cast<float*>(smem_raw) + 4;
    unsigned short* tosort = reinterpret_cast<unsigned short*>(vals + cap + 4);
    unsigned short* Lpos = tosort + cap + 2;
    unsigned short* Rpos = Lpos + cap + 2;
    __shared__ int s_ctl[8], s_wsum[4];
    unsigned short* lidx = lidx_all + (size_t)blockIdx.x * cap;
    __shared__ int s_base, s_wave[4];
    if (skip && *skip) return;
    const int cell = blockIdx.x;
    const int row = cell / num_col, col = cell - row * num_col;
    int y0, y1, x0, x1;
    sm::kp_cell_bounds(H, W, num_row, num_col, row, col, &y0, &y1, &x0, &x1);
    const int th = sm::kp_slice_len(y0, y1, H), tw = sm::kp_slice_len(x0, x1, W);
    const int total = th * tw;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < total; c0 += 256) {
        const int e = c0 + t;
        bool f = false;
        float v = 0.f;
        if (e < total) {
            const int ly = e / tw, lx = e - ly * tw;
            const size_t g = (size_t)(y0 + ly) * W + x0 + lx;
            const float vr = rdiff[g], vo = odiff[g];
            f = (vr < thr_r) && (vo < thr_o);
            v = score_rigid ? vr : vo;
        }
        const unsigned long long b = __ballot(f);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; w++) off += s_wave[w];
        if (f) {
            const int pos = off + before;
            vals[pos] = v;
            tosort[pos] = (unsigned short)pos;
            lidx[pos] = (unsigned short)e;
        }
        __syncthreads();
        if (t == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    const int cnt = s_base;
    const int pick = cnt < n_best ? cnt : n_best;
    if (pick > 0) {
        const int step = cnt / pick;  // np.arange(0, cnt, step)[:pick]
        if (t < pick) {
            const int e = lidx[t * step];
            const int ly = e / tw, lx = e - ly * tw;
            cell_sel_uni[cell * n_best + t] = ((y0 + ly) << 16) | (x0 + lx);
        }
        if (uniform_only) {
        } else if (par) {
            kp_introselect_block(vals, tosort, cnt, pick - 1, Lpos, Rpos, s_ctl, s_wsum);
        } else if (t == 0) {
            sm::kp_introselect_cp<unsigned short>(vals, tosort, cnt, pick - 1, 0);
        }
    }
    if (t == 0) cell_count[cell] = pick;
    if (uniform_only) return;
    __syncthreads();
    if (t < pick) {
        const int e = lidx[tosort[t]];
        const int ly = e / tw, lx = e - ly * tw;
        cell_sel[cell * n_best + t] = ((y0 + ly) << 16) | (x0 + lx);
    }
}

// the refusals and the launch geometry shared by enqueue_rigid_flow_kp and the rounds of the iterative scale loop
int rigid_flow_kp_geometry(int H, int W, const RigidKpConfig& cfg, int* cells_out, int* n_best_out, int* cap_out, size_t* lds_out,
                           int* par_out) {
    const int cells = cfg.num_row * cfg.num_col;
    DFVO_ARG_CHECK(cells > 0 && cells <= 1024 && H < 65536 && W < 65536, "rigid_flow_kp: grid too large");
    const int n_best = cfg.num_bestN / cells;
    DFVO_ARG_CHECK(n_best >= 1 && n_best <= 256, "rigid_flow_kp: n_best out of range");
    const int cap = sm::kp_axis_cap(H, cfg.num_row) * sm::kp_axis_cap(W, cfg.num_col);
    DFVO_ARG_CHECK(cap < 65536, "rigid_flow_kp: cell larger than 65535 pixels");
    size_t lds = (size_t)cap * (4 + 2) + 32;
    DFVO_ARG_CHECK(lds <= 158 * 1024, "rigid_flow_kp: cell does not fit in LDS");
    const int par = lds + (size_t)cap * 4 + 16 <= 150 * 1024 ? 1 : 0;
    if (par) lds += (size_t)cap * 4 + 16;
    *cells_out = cells, *n_best_out = n_best, *cap_out = cap, *lds_out = lds, *par_out = par;
    return DFVO_OK;
}

int enqueue_rigid_flow_kp_round(RigidKpBuffers& rb, const float* d_flow, const float* d_odiff, const float* d_depth32, int H,
                                int W, const RigidKpConfig& cfg, float* d_rdiff_out, const int* d_skip, hipStream_t s) {
    int cells, n_best, cap, par;
    size_t lds;
    if (int rc_g = rigid_flow_kp_geometry(H, W, cfg, &cells, &n_best, &cap, &lds, &par)) return rc_g;
    // (the caller ensured rb for this size before it enqueued the first round: no allocation between the rounds)
    DFVO_ARG_CHECK((size_t)H * W <= rb.depth32.n && cells * n_best <= rb.sel_cap && (size_t)cells * cap <= rb.lidx.n,
                   "rigid_flow_kp round: buffers not ensured for this size");
    if (int rc_lds = ensure_dyn_lds((const void*)k_kp_cell_rigid, lds)) return rc_lds;
    hipLaunchKernelGGL(k_rigid_flow_diff, dim3(cdiv(H * W, 256)), dim3(256), 0, s, d_depth32, d_flow, H, W, rb.mats, d_rdiff_out,
                       (float*)nullptr, d_skip);
    hipLaunchKernelGGL(k_kp_cell_rigid, dim3(cells), dim3(256), lds, s, d_odiff, (const float*)d_rdiff_out, H, W, cfg.num_row,
                       cfg.num_col, cfg.opt_thre, cfg.rigid_thre, cfg.score_rigid, n_best, cap, rb.cell_count, rb.cell_sel,
                       rb.cell_sel_uni, rb.lidx, par, 1, d_skip);
    const size_t sc = (size_t)rb.sel_cap * 2;
    hipLaunchKernelGGL(k_kp_gather, dim3(1), dim3(256), 0, s, rb.cell_count, rb.cell_sel_uni, cells, n_best, d_flow, H, W,
                       rb.zero, (const int*)nullptr, 0, 0, rb.kp + 2 * sc, rb.kp + 3 * sc, rb.info + 4, d_skip);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// rigid flow of the reference depth under `T` (ref -> cur), its distance to the optical flow (kept in rb.rdiff), then
// the two keypoint sets: rb.kp = [kp1_best | kp2_best | kp1_uniform | kp2_uniform], each sel_cap x 2 doubles;
// rb.info[0] = their common count.  d_rdiff_override (optional) replaces the computed distance map.
int enqueue_rigid_flow_kp(RigidKpBuffers& rb, const float* d_flow, const float* d_odiff, const float* d_depth32, int H,
                          int W, const RigidKpConfig& cfg, const float* d_rdiff_override, hipStream_t s) {
    int cells, n_best, cap, par;
    size_t lds;
    if (int rc_g = rigid_flow_kp_geometry(H, W, cfg, &cells, &n_best, &cap, &lds, &par)) return rc_g;
    int rc = rb.ensure(H, W, cells, n_best, cap);
    if (rc != DFVO_OK) return rc;
    if (int rc_lds = ensure_dyn_lds((const void*)k_kp_cell_rigid, lds)) return rc_lds;
    const float* rdiff = d_rdiff_override;
    if (!rdiff) {
        float m[34];
        for (int i = 0; i < 9; i++) m[i] = cfg.Kinv[i];
        for (int i = 0; i < 16; i++) m[9 + i] = cfg.T[i];
        for (int i = 0; i < 9; i++) m[25 + i] = cfg.K[i];
        DFVO_HIP_CHECK(hipMemcpyAsync(rb.mats, m, sizeof(m), hipMemcpyHostToDevice, s));
        DFVO_HIP_CHECK(hipStreamSynchronize(s));  // `m` is a stack buffer
        hipLaunchKernelGGL(k_rigid_flow_diff, dim3(cdiv(H * W, 256)), dim3(256), 0, s, d_depth32, d_flow, H, W, rb.mats,
                           rb.rdiff, (float*)nullptr, (const int*)nullptr);
        rdiff = rb.rdiff;
    }
    hipLaunchKernelGGL(k_kp_cell_rigid, dim3(cells), dim3(256), lds, s, d_odiff, rdiff, H, W, cfg.num_row, cfg.num_col,
                       cfg.opt_thre, cfg.rigid_thre, cfg.score_rigid, n_best, cap, rb.cell_count, rb.cell_sel,
                       rb.cell_sel_uni, rb.lidx, par, 0, (const int*)nullptr);
    // both sets in cell order; no "enough keypoints" rules here (the reference asserts a non-empty selection)
    const size_t sc = (size_t)rb.sel_cap * 2;
    hipLaunchKernelGGL(k_kp_gather, dim3(1), dim3(256), 0, s, rb.cell_count, rb.cell_sel, cells, n_best, d_flow, H, W, rb.zero,
                       (const int*)nullptr, 0, 0, rb.kp, rb.kp + sc, rb.info, (const int*)nullptr);
    hipLaunchKernelGGL(k_kp_gather, dim3(1), dim3(256), 0, s, rb.cell_count, rb.cell_sel_uni, cells, n_best, d_flow, H, W,
                       rb.zero, (const int*)nullptr, 0, 0, rb.kp + 2 * sc, rb.kp + 3 * sc, rb.info + 4, (const int*)nullptr);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// the same behind a device-side hand-over (solver_refine.hip): rb.mats and the skip flag were written on the device, the best
// set goes straight to the second pass's keypoint buffers
int enqueue_rigid_flow_kp_dev(RigidKpBuffers& rb, const float* d_flow, const float* d_odiff, const float* d_depth32, int H, int W,
                              const RigidKpConfig& cfg, const int* d_skip, double* d_kp1, double* d_kp2, int* d_info, hipStream_t s) {
    DFVO_ARG_CHECK(d_flow && d_odiff && d_depth32 && d_kp1 && d_kp2 && d_info, "rigid_flow_kp (device matrices): null argument");
    int cells, n_best, cap, par;
    size_t lds;
    if (int rc_g = rigid_flow_kp_geometry(H, W, cfg, &cells, &n_best, &cap, &lds, &par)) return rc_g;
    DFVO_ARG_CHECK((size_t)H * W <= rb.depth32.n && cells * n_best <= rb.sel_cap && (size_t)cells * cap <= rb.lidx.n,
                   "rigid_flow_kp (device matrices): buffers not ensured for this size");
    if (int rc_lds = ensure_dyn_lds((const void*)k_kp_cell_rigid, lds)) return rc_lds;
    hipLaunchKernelGGL(k_rigid_flow_diff, dim3(cdiv(H * W, 256)), dim3(256), 0, s, d_depth32, d_flow, H, W, rb.mats, rb.rdiff.p,
                       (float*)nullptr, d_skip);
    hipLaunchKernelGGL(k_kp_cell_rigid, dim3(cells), dim3(256), lds, s, d_odiff, (const float*)rb.rdiff.p, H, W, cfg.num_row,
                       cfg.num_col, cfg.opt_thre, cfg.rigid_thre, cfg.score_rigid, n_best, cap, rb.cell_count, rb.cell_sel,
                       rb.cell_sel_uni, rb.lidx, par, 0, d_skip);
    const size_t sc = (size_t)rb.sel_cap * 2;
    hipLaunchKernelGGL(k_kp_gather, dim3(1), dim3(256), 0, s, rb.cell_count, rb.cell_sel, cells, n_best, d_flow, H, W, rb.zero,
                       (const int*)nullptr, 0, 0, d_kp1, d_kp2, d_info, d_skip);
    hipLaunchKernelGGL(k_kp_gather, dim3(1), dim3(256), 0, s, rb.cell_count, rb.cell_sel_uni, cells, n_best, d_flow, H, W,
                       rb.zero, (const int*)nullptr, 0, 0, rb.kp + 2 * sc, rb.kp + 3 * sc, rb.info + 4, d_skip);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// sampled_kp (kp_selection.py:327-378): the k-th pixel (row-major) of the cropped grid [y0:y1, x0:x1] for every k of
// the uniform index list; kp1 = (x, y), kp2 = kp1 + flow (float32 promoted to float64, as numpy does)
__global__ void k_kp_sampled(const float* __restrict__ flow, int H, int W, int y0, int x0, int cw,
                             const int* __restrict__ idx, int n, double* __restrict__ kp1, double* __restrict__ kp2,
                             int* __restrict__ info /*optional: a tracker's kp_info [n, good_kp_found, regions]*/) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (info && i == 0) {
        info[0] = n;
        info[1] = 1;
        info[2] = 0;
    }
    if (i >= n) return;
    const int k = idx[i];
    const int yy = y0 + k / cw, xx = x0 + k % cw;
    const double x = (double)xx, y = (double)yy;
    kp1[i * 2] = x;
    kp1[i * 2 + 1] = y;
    kp2[i * 2] = x + (double)flow[(size_t)yy * W + xx];
    kp2[i * 2 + 1] = y + (double)flow[((size_t)H + yy) * W + xx];
}

int enqueue_kp_sampled(const float* d_flow, int H, int W, int y0, int y1, int x0, int x1, const int* d_idx, int n,
                       double* d_kp1, double* d_kp2, hipStream_t s, int* d_info) {
    DFVO_ARG_CHECK(0 <= y0 && y0 < y1 && y1 <= H && 0 <= x0 && x0 < x1 && x1 <= W, "sampled_kp: crop outside the image");
    if (n <= 0) return DFVO_OK;
    hipLaunchKernelGGL(k_kp_sampled, dim3(cdiv(n, 256)), dim3(256), 0, s, d_flow, H, W, y0, x0, x1 - x0, d_idx, n, d_kp1, d_kp2,
                       d_info);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

// numpy's linspace: arange(n) * (stop / (n - 1)), the last element set to stop, then truncated (all values are >= 0)
void generate_kp_samples(int y0, int y1, int x0, int x1, int n, int* h_idx) {
    const double stop = (double)((long long)(x1 - x0) * (y1 - y0) - 1);
    const double step = n > 1 ? stop / (double)(n - 1) : 0.0;
    for (int i = 0; i < n; ++i) h_idx[i] = (int)((double)i * step);
    if (n > 1) h_idx[n - 1] = (int)stop;
}

// score_method 'flow_ratio' (kp_selection.py:137-141,155): mask and score are flow_diff / |flow| per pixel, float32 as numpy
// evaluates it -- np.linalg.norm over the 2-vector = sqrt(x*x + y*y) with separately rounded products and sum
__global__ void k_flow_ratio(const float* __restrict__ flow, const float* __restrict__ diff, int px, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= px) return;
    const float fx = flow[i], fy = flow[px + i];
    const float xx = __fmul_rn(fx, fx), yy = __fmul_rn(fy, fy);
    out[i] = __fdiv_rn(diff[i], __fsqrt_rn(__fadd_rn(xx, yy)));
}

int enqueue_local_bestn(TrackerBuffers& tb, const float* d_flow, const float* d_diff, int H, int W, int num_row,
                        int num_col, int num_bestN, float thre, hipStream_t s, int score_method, const float* d_depth_diff,
                        float depth_thre) {
    const int cells = num_row * num_col;
    DFVO_ARG_CHECK(cells > 0 && cells <= 1024 && H < 65536 && W < 65536, "local_bestN: grid too large");
    const int n_best = num_bestN / cells;  // math.floor(N / (rows*cols))
    DFVO_ARG_CHECK(n_best >= 1 && n_best <= 256, "local_bestN: n_best out of range");
    const int cap = sm::kp_axis_cap(H, num_row) * sm::kp_axis_cap(W, num_col);
    DFVO_ARG_CHECK(cap < 65536, "local_bestN: cell larger than 65535 pixels");
    size_t lds = (size_t)cap * (4 + 2) + 32;
    DFVO_ARG_CHECK(lds <= 158 * 1024, "local_bestN: cell does not fit in LDS");
    // the workgroup-parallel partition needs two more index lists; very large cells keep the single-lane selection
    const int par = lds + (size_t)cap * 4 + 16 <= 150 * 1024 ? 1 : 0;
    if (par) lds += (size_t)cap * 4 + 16;
    int rc = tb.ensure_kp(cells * n_best, cells, n_best);
    if (rc != DFVO_OK) return rc;
    if (int rc_l = tb.grow_lidx(cells, cap)) return rc_l;
    if (int rc_lds = ensure_dyn_lds((const void*)k_kp_cell, lds)) return rc_lds;
    const float* d_key = d_diff;  // what the cells threshold and rank: the consistency map, or its ratio to the flow magnitude
    if (score_method == 1) {
        if (int rc_r = tb.grow_ratio_map(H, W)) return rc_r;
        hipLaunchKernelGGL(k_flow_ratio, dim3(cdiv(H * W, 256)), dim3(256), 0, s, d_flow, d_diff, H * W, tb.ratio_map);
        d_key = tb.ratio_map;
    }
    // (the counting blocks read the consistency map itself, whatever the cells rank: kp_selection.py:158)
    hipLaunchKernelGGL(k_kp_cell, dim3(cells + KP_CNT_BLOCKS), dim3(256), lds, s, d_key, H, W, num_row, num_col, thre, n_best, cap,
                       tb.cell_count, tb.cell_sel, tb.lidx, par, d_diff, tb.kp_total + KPT_CELL_PARTIAL, d_depth_diff, depth_thre);
    // thresholds exactly as the python float comparisons: count < N*0.1 ; regions < rows*cols*0.1
    const int min_total = (int)ceil((double)num_bestN * 0.1);
    const int min_regions = (int)ceil((double)cells * 0.1);
    hipLaunchKernelGGL(k_kp_gather, dim3(1), dim3(256), 0, s, tb.cell_count, tb.cell_sel, cells, n_best, d_flow, H, W,
                       tb.kp_total + KPT_GOOD, tb.kp_total + KPT_CELL_PARTIAL, min_total, min_regions, tb.kp_ref, tb.kp_cur, tb.kp_info,
                       (const int*)nullptr);
    DFVO_HIP_CHECK(hipGetLastError());
    return DFVO_OK;
}

}  // namespace dfvo
