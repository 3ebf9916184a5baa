// Lock-step host emulation of dfvo::kp_introselect_block (df-vo_amd/csrc/solver_kp.hip): every statement of the device
// code is executed for all 256 "threads" before the next one, a barrier is a sequence point, kp_block_excl_scan is a plain
// prefix sum.  Per-thread variables are arrays indexed by t; variables every thread holds with the same value (low, high,
// depth_limit, pivot, nL, nR, K) are scalars.  What it proves on the host: the stopper-list restatement of the unguarded
// Hoare pass (the comment above kp_introselect_block) leaves the same (key, tosort) state as sm::kp_introselect_cp.
// Keep it in step with the device code, statement by statement; it does not replace the device test.
#pragma once
#include <cstring>
#include <vector>

#include "../../df-vo_amd/csrc/kp_select.h"

namespace kp_lockstep {

constexpr int NT = 256;

// Pos = unsigned short: the two stopper counts share one packed 16-bit scan; Pos = int: two plain scans.
// key[-4 .. num+3] readable, tosort[num], Lpos / Rpos [num + 2] (the kernels give them cap + 2 >= num + 2).
template <typename Pos>
void introselect_block(float* key, Pos* tosort, int num, int kth, Pos* Lpos, Pos* Rpos, int par_min) {
    constexpr bool in_global = sizeof(Pos) == 4;
    if (kth < 3 || kth == num - 1 || num < par_min) {  // t == 0
        sm::kp_introselect_cp<Pos>(key, tosort, num, kth, 0);
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
    // exclusive scan over the first `live` threads: the others hold 0, own no element and are not written out (a short range
    // keeps most of the 256 threads idle, and the exhaustive sweep of kp_block_lockstep_check.cpp runs millions of those)
    auto excl_scan = [](const int* v, int* ex, int live, int* total) {
        int acc = 0;
        for (int t = 0; t < live; t++) {
            ex[t] = acc;
            acc += v[t];
        }
        *total = acc;
    };
    int p0[NT], p1[NT], cl[NT], cr[NT], il[NT], ir[NT], packed[NT], ex[NT], cnt[NT];
    int s_ctl[2];
    int low = 0, high = num - 1, depth_limit = sm::kp_msb((unsigned)num) * 2;
    while (low + 1 < high) {
        if (high - low < par_min || depth_limit <= 0) break;
        {  // t == 0
            const int mid = low + (high - low) / 2;
            if (sm::kp_lt(key[high], key[mid])) swap(high, mid);
            if (sm::kp_lt(key[high], key[low])) swap(high, low);
            if (sm::kp_lt(key[low], key[mid])) swap(low, mid);
            swap(mid, low + 1);
        }
        // ---- barrier
        const float pivot = key[low];
        const int r0 = low + 1, n_r = high - low;
        const int seg = (n_r + 255) / 256;
        const int live = (n_r + seg - 1) / seg < NT ? (n_r + seg - 1) / seg : NT;  // threads with p0 < p1
        for (int t = 0; t < live; t++) {
            p0[t] = r0 + t * seg;
            p1[t] = p0[t] + seg < r0 + n_r ? p0[t] + seg : r0 + n_r;
            cl[t] = cr[t] = 0;
        }
        for (int t = 0; t < live; t++)
            for (int p = p0[t]; p < p1[t]; ++p) {
                const float v = key[p];
                cl[t] += (p >= low + 2 && !sm::kp_lt(v, pivot)) ? 1 : 0;
                cr[t] += (p <= high - 1 && !sm::kp_lt(pivot, v)) ? 1 : 0;
            }
        int nL, nR;
        if (in_global) {
            excl_scan(cl, il, live, &nL);
            excl_scan(cr, ir, live, &nR);
        } else {
            int total;
            for (int t = 0; t < live; t++) packed[t] = cl[t] | (cr[t] << 16);
            excl_scan(packed, ex, live, &total);
            nL = total & 0xffff, nR = total >> 16;
            for (int t = 0; t < live; t++) il[t] = ex[t] & 0xffff, ir[t] = ex[t] >> 16;
        }
        for (int t = 0; t < live; t++)
            for (int p = p0[t]; p < p1[t]; ++p) {
                const float v = key[p];
                if (p >= low + 2 && !sm::kp_lt(v, pivot)) Lpos[il[t]++] = (Pos)p;
                if (p <= high - 1 && !sm::kp_lt(pivot, v)) Rpos[nR - 1 - (ir[t]++)] = (Pos)p;
            }
        // ---- barrier
        const int npair = nL < nR ? nL : nR;
        const int live_k = npair < NT ? npair : NT;
        for (int t = 0; t < live_k; t++) {
            cnt[t] = 0;
            for (int k = t; k < npair; k += 256) cnt[t] += Lpos[k] <= Rpos[k] ? 1 : 0;
        }
        int K;
        excl_scan(cnt, ex, live_k, &K);
        if (!in_global) K &= 0xffff;
        // one pair per thread and round; within a round every statement of `swap` runs for all threads before the next
        for (int k0 = 0; k0 < K; k0 += 256) {
            int a[NT], b[NT];
            Pos ti[NT];
            float ki[NT];
            const int live_s = K - k0 < NT ? K - k0 : NT;
            for (int t = 0; t < live_s; t++) a[t] = Lpos[k0 + t], b[t] = Rpos[k0 + t];
            for (int t = 0; t < live_s; t++)
                ti[t] = tosort[a[t]];
            for (int t = 0; t < live_s; t++)
                if (a[t] != b[t]) tosort[a[t]] = tosort[b[t]];
            for (int t = 0; t < live_s; t++)
                if (a[t] != b[t]) tosort[b[t]] = ti[t];
            for (int t = 0; t < live_s; t++)
                ki[t] = key[a[t]];
            for (int t = 0; t < live_s; t++)
                if (a[t] != b[t]) key[a[t]] = key[b[t]];
            for (int t = 0; t < live_s; t++)
                if (a[t] != b[t]) key[b[t]] = ki[t];
        }
        // ---- barrier
        {  // t == 0
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
        // ---- barrier
        low = s_ctl[0];
        high = s_ctl[1];
        depth_limit--;
    }
    sm::kp_introselect_cp_from<Pos>(key, tosort, kth, 0, low, high, depth_limit);  // t == 0
}

// Runs the emulation and the scalar selection on copies of v[0 .. num) in buffers with exactly the documented slack (four
// floats on either side of the keys, num + 2 stopper slots), so that an address sanitizer sees any read or write beyond
// it.  Returns 0 when the whole (key, tosort) states agree; fills tosort_out / key_out (optional) with the emulation's.
template <typename Pos>
int run_and_compare(const float* v, int num, int kth, int par_min, int* tosort_out, float* key_out) {
    std::vector<float> ka(num + 8, 0.f), kb(num + 8, 0.f);
    std::vector<Pos> ta(num), tb(num), L(num + 2), R(num + 2);
    for (int i = 0; i < num; i++) {
        ka[4 + i] = kb[4 + i] = v[i];
        ta[i] = tb[i] = (Pos)i;
    }
    introselect_block<Pos>(ka.data() + 4, ta.data(), num, kth, L.data(), R.data(), par_min);
    sm::kp_introselect_cp<Pos>(kb.data() + 4, tb.data(), num, kth, 0);
    int bad = 0;
    for (int i = 0; i < num; i++) {
        unsigned ua, ub;
        memcpy(&ua, &ka[4 + i], 4);
        memcpy(&ub, &kb[4 + i], 4);
        bad |= (ta[i] != tb[i]) || (ua != ub);
        if (tosort_out) tosort_out[i] = (int)ta[i];
        if (key_out) key_out[i] = ka[4 + i];
    }
    for (int i = 0; i < 4; i++) bad |= ka[i] != 0.f || ka[num + 4 + i] != 0.f;  // the slack is read, never written
    return bad;
}

}  // namespace kp_lockstep
