// Stand-alone check of the nets' layer packing (df-vo_amd/csrc/dev_mem.h, net_layers.hip): this program is linked with
// net_layers.hip compiled as plain C++ and with no HIP library -- the HIP entry points come from hip_stub.h, and the host
// functions the unit links against (the weight packers, their sizes and the two mode switches) are the trivial ones below:
// sizes and zeros, with the modes settable by the case so that every packing branch is taken.  Built with
// -fsanitize=address,undefined and run by tests/test_net_layers_cpu.py: net_layers_check <case> ; exit status 0 = the case holds.
#include <algorithm>

#include "hip_stub.h"

#include "../../df-vo_amd/csrc/nets.h"

// ---- the host functions of the unit under test ----
static int g_split_mode = 0, g_wino_mode = 0;
namespace dfvo {
int conv_split_mode() { return g_split_mode; }
int conv_fp32_winograd_mode() { return g_wino_mode; }
bool conv_wino_rule_may_accept(int, long long) { return true; }
int conv_pick_bn(int, long long) { return 32; }  // (conv_cout_pad rounds to it)
static size_t taps(int c0, int c1, int kh, int kw) { return (size_t)(c0 + c1) * kh * kw; }
template <class T>
static size_t fill(T* out, size_t n) {
    if (out) std::fill(out, out + n, T(0));
    return n;
}
void conv_pack_weights(const float*, const float*, int, int c0, int c1, int kh, int kw, int cout_pad, const float*, const float*,
                       float* out_w, float* out_b) {
    fill(out_w, (size_t)(conv_ksteps(kh, kw, c0, c1) * 4 + 8) * cout_pad * 4);
    fill(out_b, (size_t)cout_pad);
}
size_t conv_pack_weights_f16s(const float*, int cout, int c0, int c1, const float*, unsigned short* out) {
    return fill(out, 2 * taps(c0, c1, 3, 3) * round_up(cout, 32));
}
void conv_build_f16g_table(int c0, int c1, int kh, int kw, std::vector<uint32_t>* tab) { tab->assign(4 * taps(c0, c1, kh, kw), 0u); }
size_t conv_pack_weights_f16g(const float*, int cout, int c0, int c1, int kh, int kw, const float*, unsigned short* out) {
    return fill(out, 2 * taps(c0, c1, kh, kw) * round_up(cout, 32));
}
size_t conv_pack_weights_f32g(const float*, int cout, int c0, int c1, int kh, int kw, const float*, float* out) {
    return fill(out, taps(c0, c1, kh, kw) * round_up(cout, 32));
}
size_t conv_wino_f32_weight_floats(int cout, int c0, int c1) { return 16 * (size_t)(c0 + c1) * round_up(cout, 32); }
void conv_pack_weights_wino_f32(const float*, int cout, int c0, int c1, const float*, float* out) {
    fill(out, conv_wino_f32_weight_floats(cout, c0, c1));
}
size_t conv_head_weight_floats(int cout, int c0, int c1, int k) { return taps(c0, c1, k, k) * cout; }
void conv_pack_head_weights(const float*, int cout, int c0, int c1, int k, const float*, float* out) {
    fill(out, conv_head_weight_floats(cout, c0, c1, k));
}
}  // namespace dfvo

// ---- what the cases look at ----
struct Arr {
    const void* p;
    size_t n, elem;
};
template <class T>
static Arr arr(const DevArr<T>& a) {
    return Arr{a.p, a.n, sizeof(T)};
}
static std::vector<Arr> members(const ConvLayer& L) {
    return {arr(L.wp), arr(L.bias), arr(L.wf), arr(L.wg), arr(L.gtab), arr(L.wg32), arr(L.wu), arr(L.wh)};
}
// the rule: every pointer null with n == 0, or a live block that holds its `n` elements
static bool sound(const ConvLayer& L) {
    for (const Arr& a : members(L)) {
        if (!a.p && a.n) return false;
        if (a.p) {
            auto it = g_blocks.find((void*)a.p);
            if (it == g_blocks.end() || it->second < a.n * a.elem) return false;
        }
    }
    return true;
}
static size_t held(const ConvLayer& L) {
    size_t k = 0;
    for (const Arr& a : members(L)) k += a.p != nullptr;
    return k;
}

// one layer of 8 -> 8 channels, 3 x 3 (the smallest that reaches every packing), and a 2-channel head
static ParamStore params() {
    ParamStore ps;
    ps.t["body.weight"] = HostTensor{std::vector<float>(8 * 8 * 9, 0.5f), {8, 8, 3, 3}};
    ps.t["body.bias"] = HostTensor{std::vector<float>(8, 0.f), {8}};
    ps.t["head.weight"] = HostTensor{std::vector<float>(2 * 8 * 9, 0.5f), {2, 8, 3, 3}};
    ps.t["head.bias"] = HostTensor{std::vector<float>(2, 0.f), {2}};
    return ps;
}
static int pack(const ParamStore& ps, const char* name, ConvLayer* L) {
    return make_conv(ps, std::string(name) + ".weight", std::string(name) + ".bias", 8, 0, 64, nullptr, nullptr, L);
}
static void set_mode(int split, int wino) { g_split_mode = split, g_wino_mode = wino; }

// the packings each mode leaves on the body layer: {wp, bias} + ...
static void expect_body(const ConvLayer& L, int split, int wino) {
    CHECK(L.wp.p && L.bias.p && !L.wh.p);
    CHECK((L.wf.p != nullptr) == (split >= 4) && (L.wg.p != nullptr) == (split >= 4));
    CHECK((L.wg32.p != nullptr) == (split == 0) && L.gtab.p);
    CHECK((L.wu.p != nullptr) == (split == 0 && wino != 0) && L.wino_mode == (split == 0 ? wino : 0));
}

// every allocation of a packing fails in turn: no member claims what it does not hold, nothing is live once the layer is gone,
// and packing the same layer again afterwards succeeds and holds one packing only
static void fail_each(int split, int wino) {
    const ParamStore ps = params();
    set_mode(split, wino);
    for (const char* name : {"body", "head"}) {
        int n_allocs = 0;
        {
            ConvLayer L;
            arm(-1);
            CHECK(pack(ps, name, &L) == DFVO_OK && sound(L));
            n_allocs = g_allocs;
            CHECK((size_t)n_allocs == held(L) && g_blocks.size() == held(L));
            if (!strcmp(name, "body")) expect_body(L, split, wino);
            else CHECK(L.wh.p && !L.wu.p);
        }
        CHECK(g_blocks.empty());
        // body: wp, bias + (wg32, gtab [, wu] | wf, wg, gtab); head: wp, bias, wh + (nothing | wf, wg, gtab)
        CHECK(n_allocs == (strcmp(name, "body") ? (split == 0 ? 3 : 6) : split == 0 && wino ? 5 : split == 0 ? 4 : 5));
        for (int k = 0; k < n_allocs; ++k) {
            {
                ConvLayer L;
                arm(k);
                CHECK(pack(ps, name, &L) == DFVO_ERR_HIP);
                CHECK(g_last_error.find("hipMalloc") != std::string::npos);
                CHECK(sound(L) && held(L) == (size_t)k && g_blocks.size() == (size_t)k);
                arm(-1);
                CHECK(pack(ps, name, &L) == DFVO_OK && sound(L) && g_allocs == n_allocs);
                CHECK(held(L) == (size_t)n_allocs && g_blocks.size() == (size_t)n_allocs);  // the failed attempt's blocks are gone
            }
            CHECK(g_blocks.empty());
        }
    }
}
static void fail_each_fp32() { fail_each(0, 0); }
static void fail_each_f16x3() { fail_each(4, 0); }
static void fail_each_fp32_wino2() { fail_each(0, 2); }

// make_conv twice on one layer, the second time in another precision: only the second packing is live
static void repack_frees_first() {
    const ParamStore ps = params();
    ConvLayer L;
    arm(-1);
    set_mode(4, 0);
    CHECK(pack(ps, "body", &L) == DFVO_OK);
    expect_body(L, 4, 0);
    const std::map<void*, size_t> first = g_blocks;
    set_mode(0, 2);
    CHECK(pack(ps, "body", &L) == DFVO_OK && sound(L));
    expect_body(L, 0, 2);
    CHECK(g_blocks.size() == held(L) && held(L) == 5);
    for (const Arr& a : members(L)) CHECK(!a.p || g_blocks.count((void*)a.p) == 1);
    CHECK((size_t)g_frees == first.size());  // each block of the first packing, once (hip_stub.h checks for a second free)
    set_mode(0, 0);
    CHECK(pack(ps, "head", &L) == DFVO_OK && sound(L) && L.wh.p && !L.wu.p && !L.wg32.p && held(L) == 3 && g_blocks.size() == 3);
}

// a std::vector<ConvLayer> resized (its layers move) and destroyed: every block is freed exactly once
static void vector_of_layers() {
    const ParamStore ps = params();
    set_mode(0, 2);
    arm(-1);
    {
        std::vector<ConvLayer> v(2);
        CHECK(pack(ps, "body", &v[0]) == DFVO_OK && pack(ps, "head", &v[1]) == DFVO_OK);
        const float* wp0 = v[0].wp;
        const size_t live = g_blocks.size();
        v.resize(40);  // reallocates: the layers are moved, not copied
        CHECK(v[0].wp.p == wp0 && g_blocks.size() == live && g_frees == 0 && sound(v[0]) && sound(v[1]) && held(v[39]) == 0);
        CHECK(pack(ps, "body", &v[39]) == DFVO_OK);
        v.resize(1);
        CHECK(g_blocks.size() == held(v[0]) && sound(v[0]));
    }
    CHECK(g_blocks.empty() && g_frees == g_allocs);
}

static void alloc_zeroed_cases() {
    arm(-1);
    arm_memset(-1);
    {
        DevArr<float> a;
        CHECK(a.alloc(64) == DFVO_OK);
        memset(a.p, 0xff, 64 * sizeof(float));
        const float* old = a;
        CHECK(a.alloc_zeroed(100) == DFVO_OK && a.n == 100 && g_blocks.count((void*)old) == 0 && g_blocks.size() == 1);
        for (size_t i = 0; i < a.n; ++i) CHECK(a.p[i] == 0.f);
        CHECK(upload_floats(std::vector<float>(7, 2.f), &a) == DFVO_OK && a.n == 7 && a.p[6] == 2.f && g_blocks.size() == 1);
        arm_memset(0);
        CHECK(a.alloc_zeroed(50) == DFVO_ERR_HIP && !a.p && a.n == 0 && g_blocks.empty());
        CHECK(g_last_error.find("hipMemset") != std::string::npos);
        arm_memset(-1);
        arm(0);
        CHECK(a.alloc_zeroed(50) == DFVO_ERR_HIP && !a.p && a.n == 0 && g_blocks.empty());
        arm(-1);
        CHECK(a.alloc_zeroed(50) == DFVO_OK && a.p && a.n == 50);
    }
    CHECK(g_blocks.empty());
}

static void detach_case() {
    arm(-1);
    float* q = nullptr;
    {
        PinnedArr<float> a;
        CHECK(a.alloc(16) == DFVO_OK);
        q = a.detach();
        CHECK(q && !a.p && a.n == 0 && a.detach() == nullptr);
    }
    CHECK(g_blocks.count(q) == 1 && g_blocks.size() == 1 && g_frees == 0);  // the array died, the block did not
    CHECK(hipHostFree(q) == hipSuccess);
}

int main(int argc, char** argv) {
    const std::map<std::string, std::function<void()>> cases = {
        {"fail_each_fp32", fail_each_fp32},
        {"fail_each_f16x3", fail_each_f16x3},
        {"fail_each_fp32_wino2", fail_each_fp32_wino2},
        {"repack_frees_first", repack_frees_first},
        {"vector_of_layers", vector_of_layers},
        {"alloc_zeroed", alloc_zeroed_cases},
        {"detach", detach_case},
    };
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        for (const auto& c : cases) printf("%s\n", c.first.c_str());
        return 0;
    }
    auto it = argc == 2 ? cases.find(argv[1]) : cases.end();
    if (it == cases.end()) {
        fprintf(stderr, "usage: net_layers_check --list | <case>\n");
        return 2;
    }
    it->second();
    // whatever a case left behind is a leak (the leak checker of the sanitizer sees the same at exit)
    CHECK(g_blocks.empty() && g_streams.empty() && g_events.empty());
    if (g_failed) return 1;
    printf("%s: ok\n", it->first.c_str());
    return 0;
}
