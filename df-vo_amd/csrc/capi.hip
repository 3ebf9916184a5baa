// extern "C" surface declared in include/dfvo_hip.h (part 1: device helpers, operators, nets).
#include "../../include/dfvo_hip.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "nets.h"
#include "ops.h"
#include "resize_lanczos.h"
#include "capi_types.h"

namespace dfvo {
static thread_local std::string g_err;
void set_last_error(const std::string& s) { g_err = s; }
const char* last_error() { return g_err.c_str(); }

int ensure_dyn_lds(const void* kernel, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> configured;
    int dev = 0;
    DFVO_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = configured[{dev, kernel}];
    if (bytes > have) {
        DFVO_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = bytes;
    }
    return DFVO_OK;
}
}  // namespace dfvo

using namespace dfvo;


#define API_TRY(expr)                   \
    do {                                \
        int _rc = (expr);               \
        if (_rc != DFVO_OK) return _rc; \
    } while (0)

extern "C" {

const char* dfvo_last_error(void) { return dfvo::last_error(); }

int dfvo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int dfvo_set_device(int ordinal) {
    DFVO_HIP_CHECK(hipSetDevice(ordinal));
    return DFVO_OK;
}
int dfvo_sync_device(void) {
    DFVO_HIP_CHECK(hipDeviceSynchronize());
    return DFVO_OK;
}
int dfvo_malloc(void** d_ptr, size_t bytes) {
    DFVO_HIP_CHECK(hipMalloc(d_ptr, bytes));
    return DFVO_OK;
}
int dfvo_free(void* d_ptr) {
    DFVO_HIP_CHECK(hipFree(d_ptr));
    return DFVO_OK;
}
int dfvo_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
    DFVO_HIP_CHECK(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return DFVO_OK;
}
int dfvo_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
    DFVO_HIP_CHECK(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return DFVO_OK;
}

// ------------------------------------------------------------------------------------------------
// The operator entry points below keep their device temporaries in local DevArrs.  Their rule: between the first enqueue
// that reads a local array and the end of its scope, every path passes a hipStreamSynchronize of that stream -- finish().

// waits for the stream behind a launch (the caller's temporaries die after it); the launch's error wins over the stream's
static int finish(int rc, hipStream_t s) {
    hipError_t e = hipStreamSynchronize(s);
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(e);
    return DFVO_OK;
}

int dfvo_conv2d(const dfvo_conv_desc* d, const float* d_src0, const float* d_src1, const float* h_w,
                const float* h_bias, const float* d_res, float* d_dst, void* stream) {
    DFVO_ARG_CHECK(d && d_src0 && h_w && d_dst, "dfvo_conv2d: null argument");
    DFVO_ARG_CHECK(d->c1 == 0 || d_src1, "dfvo_conv2d: c1 > 0 needs d_src1");
    DFVO_ARG_CHECK(d->dst_zero_to == 0 || (d->dst_zero_to >= d->cout && d->dst_co + d->dst_zero_to <= d->dst_cs),
                   "dfvo_conv2d: dst_zero_to outside the destination view");
    hipStream_t s = (hipStream_t)stream;
    const int Ho = (d->H + 2 * d->pad_h - d->kh) / d->stride + 1;
    const int Wo = (d->W + 2 * d->pad_w - d->kw) / d->stride + 1;
    const long long M = (long long)d->N * Ho * Wo;
    const int cout_pad = conv_cout_pad(d->cout, M);
    const int ksteps = conv_ksteps(d->kh, d->kw, d->c0, d->c1);
    std::vector<float> pw((size_t)(ksteps * 4 + 8) * cout_pad * 4), pb(cout_pad);  // slack: see make_conv
    conv_pack_weights(h_w, h_bias, d->cout, d->c0, d->c1, d->kh, d->kw, cout_pad, nullptr, nullptr, pw.data(),
                      pb.data());
    ConvLayer L;  // (its packings are read by run_conv's launch alone; the stream is waited for behind it, before L goes)
    API_TRY(L.wp.alloc(pw.size()));
    API_TRY(L.bias.alloc(pb.size()));
    DFVO_HIP_CHECK(hipMemcpy(L.wp, pw.data(), pw.size() * sizeof(float), hipMemcpyHostToDevice));
    DFVO_HIP_CHECK(hipMemcpy(L.bias, pb.data(), pb.size() * sizeof(float), hipMemcpyHostToDevice));
    API_TRY(make_f16s_weights(h_w, d->cout, d->c0, d->c1, d->kh, d->kw, nullptr, &L));
    API_TRY(make_f16g_weights(h_w, d->cout, d->c0, d->c1, d->kh, d->kw, nullptr, &L));
    L.stride = d->stride;
    L.pad_h = d->pad_h;
    L.pad_w = d->pad_w;
    L.pad_mode = d->pad_mode;
    L.m_hint = M;
    API_TRY(make_wino_weights(h_w, d->cout, d->c0, d->c1, d->kh, d->kw, nullptr,
                              d->stride == 1 && d->pad_h == 1 && d->pad_w == 1 && d->pad_mode == PAD_ZERO && d->up0 == 0, &L));
    API_TRY(make_head_weights(h_w, d->cout, d->c0, d->c1, d->kh, d->kw, nullptr, &L));
    L.cout = d->cout;
    L.cout_pad = cout_pad;
    L.c0 = d->c0;
    L.c1 = d->c1;
    L.kh = d->kh;
    L.kw = d->kw;
    L.ksteps = ksteps;
    L.act = d->act;
    L.act_param = d->act_param;
    // split-K workspace + tile tickets (as the nets own one each): process-wide, calls are serialised by the sync below
    // (on the heap and never freed: no object with static storage duration holds a DevArr, see dev_mem.h)
    static DevArr<float>* const conv2d_ws = new DevArr<float>();
    static std::mutex conv2d_mu;
    std::lock_guard<std::mutex> conv2d_lock(conv2d_mu);
    if (!conv2d_ws->p) (void)conv2d_ws->alloc_zeroed((size_t)4 << 20);
    int rc = run_conv(L, d->N, d->H, d->W, View{d_src0, d->cs0, d->co0}, d->up0, View{d_src1, d->cs1, d->co1}, d_res,
                      d->res_cs, d->res_co, d_dst, d->dst_cs, d->dst_co, d->dst_zero_to, s, nullptr,
                      conv2d_ws->p ? conv2d_ws : nullptr);
    return finish(rc, s);
}

int dfvo_set_conv_precision(const char* name) { return conv_set_precision(name); }
const char* dfvo_get_conv_precision(void) { return conv_get_precision(); }
int dfvo_f16s_overflow_count(unsigned long long* h_count, int reset) { return conv_f16s_overflow_count(h_count, reset); }
int dfvo_set_fp32_winograd(int mode) { return conv_set_fp32_winograd(mode); }
int dfvo_get_fp32_winograd(void) { return conv_fp32_winograd_mode(); }
int dfvo_fp32_winograd_launches(unsigned long long* h_count, int reset) { return conv_fp32_winograd_launches(h_count, reset); }

int dfvo_conv_profile_begin(void) {
    conv_profile_begin();
    return DFVO_OK;
}
int dfvo_conv_profile_end(double* h_ms19, double* h_flops19, int* h_launches19) {
    DFVO_ARG_CHECK(h_ms19 && h_flops19 && h_launches19, "dfvo_conv_profile_end: null argument");
    return conv_profile_end(h_ms19, h_flops19, h_launches19);
}
int dfvo_conv_profile_end_bytes(double* h_ms24, double* h_flops24, int* h_launches24, double* h_bytes24) {
    DFVO_ARG_CHECK(h_ms24 && h_flops24 && h_launches24 && h_bytes24, "dfvo_conv_profile_end_bytes: null argument");
    return conv_profile_end(h_ms24, h_flops24, h_launches24, h_bytes24);
}

int dfvo_correlation(const float* d_first, const float* d_second, int N, int H, int W, int C, int stride,
                     float slope, float* d_out, void* stream) {
    DFVO_ARG_CHECK(d_first && d_second && d_out, "dfvo_correlation: null argument");
    DFVO_ARG_CHECK(stride == 1 || stride == 2, "dfvo_correlation: stride must be 1 or 2");
    return launch_correlation(d_first, C, 0, d_second, C, 0, 0, N, H, W, C, stride, d_out, 52, slope,
                              (hipStream_t)stream);
}

// host table -> a local array of the caller
static int upload_table(const float* h, int n, DevArr<float>* d) {
    DFVO_ARG_CHECK(h && n > 0, "null host table");
    API_TRY(d->alloc((size_t)n));
    DFVO_HIP_CHECK(hipMemcpy(d->p, h, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    return DFVO_OK;
}

static std::vector<float> lin_default(int n) {
    std::vector<float> v(n);
    const float step = n > 1 ? 2.f / (float)(n - 1) : 0.f;
    const int half = n / 2;
    for (int i = 0; i < n; ++i) v[i] = i < half ? -1.f + step * (float)i : 1.f - step * (float)(n - i - 1);
    return v;
}

int dfvo_backward_warp(const float* d_src, const float* d_flow, float mult, int N, int H, int W, int C,
                       const float* h_lin_x, const float* h_lin_y, float* d_dst, void* stream) {
    DFVO_ARG_CHECK(d_src && d_flow && d_dst, "dfvo_backward_warp: null argument");
    hipStream_t s = (hipStream_t)stream;
    std::vector<float> lx = h_lin_x ? std::vector<float>(h_lin_x, h_lin_x + W) : lin_default(W);
    std::vector<float> ly = h_lin_y ? std::vector<float>(h_lin_y, h_lin_y + H) : lin_default(H);
    DevArr<float> dx, dy;  // (nothing is enqueued before launch_warp: the early returns leave no reader behind)
    API_TRY(dx.alloc(W));
    API_TRY(dy.alloc(H));
    DFVO_HIP_CHECK(hipMemcpy(dx, lx.data(), W * sizeof(float), hipMemcpyHostToDevice));
    DFVO_HIP_CHECK(hipMemcpy(dy, ly.data(), H * sizeof(float), hipMemcpyHostToDevice));
    return finish(launch_warp(d_src, C, 0, 0, d_flow, 2, 0, mult, N, H, W, C, dx, dy, d_dst, C, 0, 0, s), s);
}

int dfvo_warp_view(const float* d_src, int scs, int sco, int swap, const float* d_flow, int fcs, int fco, float mult, int N,
                   int H, int W, int C, const float* h_lin_x, const float* h_lin_y, float* d_dst, int dcs, int dco,
                   int append_flow, int step, void* stream) {
    DFVO_ARG_CHECK(d_src && d_flow && d_dst && N > 0 && H > 1 && W > 1 && C > 0 && step >= 1, "dfvo_warp_view: bad argument");
    DFVO_ARG_CHECK(sco + C <= scs && fco + 2 <= fcs && dco + C + (append_flow ? 4 : 0) <= dcs, "dfvo_warp_view: view too narrow");
    hipStream_t s = (hipStream_t)stream;
    DevArr<float> dx, dy;
    int rc = upload_table(h_lin_x, W, &dx);
    if (rc == DFVO_OK) rc = upload_table(h_lin_y, H, &dy);
    if (rc == DFVO_OK)
        rc = launch_warp(d_src, scs, sco, swap, d_flow, fcs, fco, mult, N, H, W, C, dx, dy, d_dst, dcs, dco, append_flow, s, step);
    return finish(rc, s);
}

int dfvo_correlation_view(const float* d_first, int cs1, int co1, const float* d_second, int cs2, int co2, int swap2, int N,
                          int H, int W, int C, int stride, float slope, float* d_out, int dcs, void* stream) {
    DFVO_ARG_CHECK(d_first && d_second && d_out && N > 0 && H > 0 && W > 0 && C > 0, "dfvo_correlation_view: null argument");
    DFVO_ARG_CHECK(stride == 1 || stride == 2, "dfvo_correlation_view: stride must be 1 or 2");
    DFVO_ARG_CHECK(co1 + C <= cs1 && co2 + C <= cs2 && dcs >= 49, "dfvo_correlation_view: view too narrow");
    hipStream_t s = (hipStream_t)stream;
    return finish(launch_correlation(d_first, cs1, co1, d_second, cs2, co2, swap2, N, H, W, C, stride, d_out, dcs, slope, s),
                  s);
}

int dfvo_flow_mean(const float* d_flow, int fcs, int fco, int N, int HW, float* d_mean, void* stream) {
    DFVO_ARG_CHECK(d_flow && d_mean && N > 0 && HW > 0 && fco + 2 <= fcs, "dfvo_flow_mean: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = flow_mean_scratch_floats(N);
    DevArr<float> scratch;
    API_TRY(scratch.alloc(n));
    auto enqueue = [&]() -> int {
        DFVO_HIP_CHECK(hipMemsetAsync(scratch, 0, n * sizeof(float), s));
        return launch_flow_mean(d_flow, fcs, fco, N, HW, scratch, d_mean, s);
    };
    return finish(enqueue(), s);
}

int dfvo_reg_prep(const float* d_img, const float* d_flow, int fcs, int fco, float mult, const float* d_mean, int N, int H,
                  int W, const float* h_lin_x, const float* h_lin_y, float* d_dst, void* stream) {
    DFVO_ARG_CHECK(d_img && d_flow && d_mean && d_dst && N > 0 && H > 1 && W > 1 && fco + 2 <= fcs, "dfvo_reg_prep: bad argument");
    hipStream_t s = (hipStream_t)stream;
    DevArr<float> dx, dy;
    int rc = upload_table(h_lin_x, W, &dx);
    if (rc == DFVO_OK) rc = upload_table(h_lin_y, H, &dy);
    if (rc == DFVO_OK) rc = launch_reg_prep(d_img, d_flow, fcs, fco, mult, d_mean, N, H, W, dx, dy, d_dst, s);
    return finish(rc, s);
}

int dfvo_reg_head(const float* d_dist, int dist_cs, int k, const float* d_flow, int fcs, int fco, const float* h_wx, float bx,
                  const float* h_wy, float by, int N, int H, int W, float* d_dst, int dcs, int dco, void* stream) {
    DFVO_ARG_CHECK(d_dist && d_flow && d_dst && N > 0 && H > 0 && W > 0 && k >= 1 && k <= 9 && (k & 1), "dfvo_reg_head: bad argument");
    DFVO_ARG_CHECK(dist_cs >= k * k && fco + 2 <= fcs && dco + 2 <= dcs, "dfvo_reg_head: view too narrow");
    hipStream_t s = (hipStream_t)stream;
    DevArr<float> wx, wy;
    int rc = upload_table(h_wx, k * k, &wx);
    if (rc == DFVO_OK) rc = upload_table(h_wy, k * k, &wy);
    if (rc == DFVO_OK) rc = launch_reg_head(d_dist, dist_cs, k, d_flow, fcs, fco, wx, bx, wy, by, N, H, W, d_dst, dcs, dco, s);
    return finish(rc, s);
}

int dfvo_deconv_variant(int C, int cs) { return deconv_dw_variant(cs, 0, cs, 0, C, deconv_blk_enabled()); }
int dfvo_correlation_variant(int C, int cs1, int co1, int cs2, int co2) {
    return correlation_variant(C, cs1, co1, cs2, co2, correlation_rt_enabled());
}
int dfvo_reg_head_variant(const float* d_dist, int dist_cs, int k, const float* d_flow, int fcs, int fco, const float* d_dst, int dcs,
                          int dco) {
    return reg_head_variant(d_dist, dist_cs, k, d_flow, fcs, fco, d_dst, dcs, dco, reg_head_vec_enabled());
}

int dfvo_flow_post(const float* d_netflow, int fcs, int fco, int h, int w, float scale, int H, int W, float* d_fwd,
                   float* d_bwd, float* d_diff, void* stream) {
    DFVO_ARG_CHECK(d_netflow && d_fwd && d_bwd && d_diff && h > 0 && w > 0 && H > 1 && W > 1 && fco + 2 <= fcs,
                   "dfvo_flow_post: bad argument");
    hipStream_t s = (hipStream_t)stream;
    return finish(launch_flow_post(d_netflow, fcs, fco, h, w, scale, H, W, d_fwd, d_bwd, d_diff, s), s);
}

int dfvo_img_u8_to_flow_input(const uint8_t* d_img, int H, int W, float* d_dst, int th, int tw, void* stream) {
    DFVO_ARG_CHECK(d_img && d_dst && H > 0 && W > 0 && th > 0 && tw > 0, "dfvo_img_u8_to_flow_input: bad argument");
    hipStream_t s = (hipStream_t)stream;
    return finish(launch_img_u8_to_flow_input(d_img, H, W, d_dst, th, tw, s), s);
}

int dfvo_maxpool3x3s2(const float* d_src, int N, int H, int W, int C, float* d_dst, void* stream) {
    DFVO_ARG_CHECK(d_src && d_dst && N > 0 && H > 0 && W > 0 && C > 0, "dfvo_maxpool3x3s2: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int rc = launch_maxpool3x3s2(d_src, N, H, W, C, d_dst, s);
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(hipStreamSynchronize(s));
    return DFVO_OK;
}

int dfvo_deconv_dw4x4s2(const float* d_src, int N, int H, int W, int C, int cs, const float* h_weight, float* d_dst,
                        void* stream) {
    DFVO_ARG_CHECK(d_src && h_weight && d_dst && cs >= C, "dfvo_deconv_dw4x4s2: bad argument");
    hipStream_t s = (hipStream_t)stream;
    DevArr<float> dw;
    API_TRY(dw.alloc((size_t)C * 16));
    DFVO_HIP_CHECK(hipMemcpy(dw, h_weight, (size_t)C * 16 * sizeof(float), hipMemcpyHostToDevice));
    return finish(launch_deconv_dw(d_src, cs, 0, N, H, W, C, dw, d_dst, cs, 0, s), s);
}

int dfvo_resize_bilinear(const float* d_src, int N, int H, int W, int C, float* d_dst, int Ho, int Wo,
                         int align_corners, void* stream) {
    DFVO_ARG_CHECK(d_src && d_dst, "dfvo_resize_bilinear: null argument");
    return launch_resize_bilinear(d_src, N, H, W, C, d_dst, Ho, Wo, align_corners, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
static int store_param(ParamStore* ps, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(name && h && ndim >= 0 && ndim <= 8 && (ndim == 0 || shape), "set_param: bad argument");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        DFVO_ARG_CHECK(shape[i] > 0, "set_param: non-positive dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(h, h + n);
    ps->t[name] = std::move(t);
    return DFVO_OK;
}

int dfvo_flownet_create(int img_h, int img_w, void* stream, dfvo_flownet** out) {
    DFVO_ARG_CHECK(out, "dfvo_flownet_create: null out");
    dfvo_flownet* n = new dfvo_flownet();
    int rc = n->net.init(img_h, img_w, (hipStream_t)stream);
    if (rc != DFVO_OK) {
        delete n;
        return rc;
    }
    *out = n;
    return DFVO_OK;
}
void dfvo_flownet_destroy(dfvo_flownet* n) {
    delete n;  // (null is fine; FlowNet's destructor and its arrays do the rest)
}
int dfvo_flownet_set_param(dfvo_flownet* n, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(n, "null net");
    DFVO_ARG_CHECK(!n->net.finalized, "set_param after finalize");
    return store_param(&n->net.params, name, h, ndim, shape);
}
int dfvo_flownet_finalize(dfvo_flownet* n) {
    DFVO_ARG_CHECK(n, "null net");
    return n->net.finalize();
}
int dfvo_flow_target_size(int img_h, int img_w, int* net_h, int* net_w) {
    DFVO_ARG_CHECK(net_h && net_w && img_h >= 32 && img_w >= 32, "dfvo_flow_target_size: bad argument");
    flow_target_size(img_h, img_w, net_h, net_w);
    return DFVO_OK;
}
int dfvo_flownet_net_size(const dfvo_flownet* n, int* h, int* w) {
    DFVO_ARG_CHECK(n && h && w, "null argument");
    *h = n->net.H;
    *w = n->net.W;
    return DFVO_OK;
}
int dfvo_flownet_set_graph(dfvo_flownet* n, int enable) {
    DFVO_ARG_CHECK(n, "null net");
    n->net.use_graph = enable != 0;
    return DFVO_OK;
}
int dfvo_flownet_forward(dfvo_flownet* n, const uint8_t* d_ref, const uint8_t* d_cur, float* d_fwd, float* d_bwd,
                         float* d_diff) {
    DFVO_ARG_CHECK(n && d_ref && d_cur && d_fwd && d_bwd && d_diff, "dfvo_flownet_forward: null argument");
    return n->net.forward(d_ref, d_cur, d_fwd, d_bwd, d_diff);
}
int dfvo_flownet_forward_host(dfvo_flownet* n, const uint8_t* h_ref, const uint8_t* h_cur, float* h_fwd,
                              float* h_bwd, float* h_diff) {
    DFVO_ARG_CHECK(n && h_ref && h_cur && h_fwd && h_bwd && h_diff, "dfvo_flownet_forward_host: null argument");
    FlowNet& f = n->net;
    DFVO_ARG_CHECK(f.finalized, "forward before finalize");
    const size_t ib = (size_t)f.imgH * f.imgW * 3, px = (size_t)f.imgH * f.imgW;
    DFVO_HIP_CHECK(hipMemcpyAsync(f.u8_ref.p, h_ref, ib, hipMemcpyHostToDevice, f.stream));
    DFVO_HIP_CHECK(hipMemcpyAsync(f.u8_cur.p, h_cur, ib, hipMemcpyHostToDevice, f.stream));
    API_TRY(f.forward((const uint8_t*)f.u8_ref.p, (const uint8_t*)f.u8_cur.p, f.out_fwd.p, f.out_bwd.p, f.out_diff.p));
    DFVO_HIP_CHECK(hipMemcpyAsync(h_fwd, f.out_fwd.p, 2 * px * sizeof(float), hipMemcpyDeviceToHost, f.stream));
    DFVO_HIP_CHECK(hipMemcpyAsync(h_bwd, f.out_bwd.p, 2 * px * sizeof(float), hipMemcpyDeviceToHost, f.stream));
    DFVO_HIP_CHECK(hipMemcpyAsync(h_diff, f.out_diff.p, px * sizeof(float), hipMemcpyDeviceToHost, f.stream));
    DFVO_HIP_CHECK(hipStreamSynchronize(f.stream));
    return DFVO_OK;
}
double dfvo_flownet_last_flops(const dfvo_flownet* n) { return n ? n->net.flops_last : 0.0; }
int dfvo_flownet_get_level_flow(dfvo_flownet* n, int level, float* h_out, int* h, int* w) {
    DFVO_ARG_CHECK(n && h_out && level >= 2 && level <= 6, "dfvo_flownet_get_level_flow: bad argument");
    FlowNet& f = n->net;
    DFVO_ARG_CHECK(f.finalized, "get_level_flow before finalize");
    const int hh = f.lh[level], ww = f.lw[level];
    std::vector<float> tmp((size_t)2 * hh * ww * 4);
    DFVO_HIP_CHECK(hipStreamSynchronize(f.stream));
    DFVO_HIP_CHECK(hipMemcpy(tmp.data(), f.lv[level].flow.p, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)2 * hh * ww; ++i) {
        h_out[i * 2] = tmp[i * 4];
        h_out[i * 2 + 1] = tmp[i * 4 + 1];
    }
    if (h) *h = hh;
    if (w) *w = ww;
    return DFVO_OK;
}
int dfvo_flownet_sync(dfvo_flownet* n) {
    DFVO_ARG_CHECK(n, "null net");
    DFVO_HIP_CHECK(hipStreamSynchronize(n->net.stream));
    return DFVO_OK;
}

// ------------------------------------------------------------------------------------------------
int dfvo_depthnet_create(int feed_h, int feed_w, float min_depth, float max_depth, float baseline_mult, void* stream,
                         dfvo_depthnet** out) {
    DFVO_ARG_CHECK(out, "dfvo_depthnet_create: null out");
    dfvo_depthnet* n = new dfvo_depthnet();
    n->net.min_depth = min_depth;
    n->net.max_depth = max_depth;
    n->net.baseline_mult = baseline_mult;
    int rc = n->net.init(feed_h, feed_w, (hipStream_t)stream);
    if (rc != DFVO_OK) {
        delete n;
        return rc;
    }
    *out = n;
    return DFVO_OK;
}
void dfvo_depthnet_destroy(dfvo_depthnet* n) {
    delete n;
}
int dfvo_depthnet_set_param(dfvo_depthnet* n, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(n, "null net");
    DFVO_ARG_CHECK(!n->net.finalized, "set_param after finalize");
    return store_param(&n->net.params, name, h, ndim, shape);
}
int dfvo_depthnet_finalize(dfvo_depthnet* n) {
    DFVO_ARG_CHECK(n, "null net");
    return n->net.finalize();
}
int dfvo_depthnet_set_graph(dfvo_depthnet* n, int enable) {
    DFVO_ARG_CHECK(n, "null net");
    n->net.use_graph = enable != 0;
    return DFVO_OK;
}
int dfvo_depthnet_forward(dfvo_depthnet* n, const uint8_t* d_img, float* d_depth) {
    DFVO_ARG_CHECK(n && d_img && d_depth, "dfvo_depthnet_forward: null argument");
    return n->net.forward(d_img, d_depth);
}
int dfvo_depthnet_forward_host(dfvo_depthnet* n, const uint8_t* h_img, float* h_depth) {
    DFVO_ARG_CHECK(n && h_img && h_depth, "dfvo_depthnet_forward_host: null argument");
    DepthNet& d = n->net;
    DFVO_ARG_CHECK(d.finalized, "forward before finalize");
    const size_t px = (size_t)d.H * d.W;
    DFVO_HIP_CHECK(hipMemcpyAsync(d.u8_in.p, h_img, px * 3, hipMemcpyHostToDevice, d.stream));
    API_TRY(d.forward((const uint8_t*)d.u8_in.p, d.depth.p));
    DFVO_HIP_CHECK(hipMemcpyAsync(h_depth, d.depth.p, px * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    DFVO_HIP_CHECK(hipStreamSynchronize(d.stream));
    return DFVO_OK;
}
int dfvo_depthnet_forward_image_host(dfvo_depthnet* n, const uint8_t* h_img, int img_h, int img_w, float* h_depth) {
    DFVO_ARG_CHECK(n && h_img && h_depth && img_h > 0 && img_w > 0, "dfvo_depthnet_forward_image_host: bad argument");
    DepthNet& d = n->net;
    DFVO_ARG_CHECK(d.finalized, "forward before finalize");
    if (n->resize.H != img_h || n->resize.W != img_w || n->resize.oh != d.H || n->resize.ow != d.W)
        API_TRY(n->resize.init(img_h, img_w, d.H, d.W));
    const size_t bytes = (size_t)img_h * img_w * 3;
    API_TRY(n->img_full.grow(bytes));
    const size_t px = (size_t)d.H * d.W;
    DFVO_HIP_CHECK(hipMemcpyAsync(n->img_full, h_img, bytes, hipMemcpyHostToDevice, d.stream));
    API_TRY(n->resize.enqueue(n->img_full, (uint8_t*)d.u8_in.p, d.stream));
    API_TRY(d.forward((const uint8_t*)d.u8_in.p, d.depth.p));
    DFVO_HIP_CHECK(hipMemcpyAsync(h_depth, d.depth.p, px * sizeof(float), hipMemcpyDeviceToHost, d.stream));
    DFVO_HIP_CHECK(hipStreamSynchronize(d.stream));
    return DFVO_OK;
}
int dfvo_lanczos_coeffs(int in_size, int out_size, int* h_bounds, int* h_coeffs, int coeff_cap, int* ksize) {
    return lanczos_coeffs_host(in_size, out_size, h_bounds, h_coeffs, coeff_cap, ksize);
}
int dfvo_resize_lanczos_u8(const uint8_t* d_src, int H, int W, uint8_t* d_dst, int out_h, int out_w, void* stream) {
    DFVO_ARG_CHECK(d_src && d_dst, "dfvo_resize_lanczos_u8: null argument");
    LanczosResizer r;
    int rc = r.init(H, W, out_h, out_w);
    if (rc == DFVO_OK) rc = r.enqueue(d_src, d_dst, (hipStream_t)stream);
    return finish(rc, (hipStream_t)stream);  // the tables die with r, behind the wait
}
int dfvo_resize_linear_u8(const uint8_t* d_src, int H, int W, int C, uint8_t* d_dst, int out_h, int out_w, void* stream) {
    return enqueue_resize_linear_u8(d_src, H, W, C, d_dst, out_h, out_w, (hipStream_t)stream);
}
int dfvo_read_image_tail_u8(const uint8_t* d_decoded, int img_h, int img_w, int bgr, int y0, int y1, int x0, int x1, uint8_t* d_dst,
                            int out_h, int out_w, void* stream) {
    DFVO_ARG_CHECK(d_decoded && d_dst && img_h > 0 && img_w > 0 && 0 <= y0 && y0 < y1 && y1 <= img_h && 0 <= x0 && x0 < x1 && x1 <= img_w,
                   "dfvo_read_image_tail_u8: crop outside the frame");
    return enqueue_resize_linear_u8(d_decoded + ((size_t)y0 * img_w + x0) * 3, y1 - y0, x1 - x0, 3, d_dst, out_h, out_w,
                                    (hipStream_t)stream, img_w, bgr);
}
double dfvo_depthnet_last_flops(const dfvo_depthnet* n) { return n ? n->net.flops_last : 0.0; }
int dfvo_depthnet_sync(dfvo_depthnet* n) {
    DFVO_ARG_CHECK(n, "null net");
    DFVO_HIP_CHECK(hipStreamSynchronize(n->net.stream));
    return DFVO_OK;
}
// ------------------------------------------------------------------------------------------------
int dfvo_posenet_create(int feed_h, int feed_w, float baseline_mult, void* stream, dfvo_posenet** out) {
    DFVO_ARG_CHECK(out, "dfvo_posenet_create: null out");
    dfvo_posenet* n = new dfvo_posenet();
    n->net.baseline_mult = baseline_mult;
    int rc = n->net.init(feed_h, feed_w, (hipStream_t)stream);
    if (rc != DFVO_OK) {
        delete n;
        return rc;
    }
    *out = n;
    return DFVO_OK;
}
void dfvo_posenet_destroy(dfvo_posenet* n) {
    delete n;
}
int dfvo_posenet_set_param(dfvo_posenet* n, const char* name, const float* h, int ndim, const int* shape) {
    DFVO_ARG_CHECK(n, "null net");
    DFVO_ARG_CHECK(!n->net.finalized, "set_param after finalize");
    return store_param(&n->net.params, name, h, ndim, shape);
}
int dfvo_posenet_finalize(dfvo_posenet* n) {
    DFVO_ARG_CHECK(n, "null net");
    return n->net.finalize();
}
int dfvo_posenet_set_graph(dfvo_posenet* n, int enable) {
    DFVO_ARG_CHECK(n, "null net");
    n->net.use_graph = enable != 0;
    return DFVO_OK;
}
int dfvo_posenet_forward(dfvo_posenet* n, const uint8_t* d_img0, const uint8_t* d_img1, float* d_pose16, float* d_params6) {
    DFVO_ARG_CHECK(n && d_img0 && d_img1 && d_pose16, "dfvo_posenet_forward: null argument");
    return n->net.forward(d_img0, d_img1, d_pose16, d_params6);
}
int dfvo_posenet_forward_images_host(dfvo_posenet* n, const uint8_t* h_img0, const uint8_t* h_img1, int img_h, int img_w,
                                     float* h_pose16) {
    DFVO_ARG_CHECK(n && h_img0 && h_img1 && h_pose16 && img_h > 0 && img_w > 0, "dfvo_posenet_forward_images_host: bad argument");
    PoseNet& p = n->net;
    DFVO_ARG_CHECK(p.finalized, "forward before finalize");
    if (n->resize.H != img_h || n->resize.W != img_w || n->resize.oh != p.H || n->resize.ow != p.W)
        API_TRY(n->resize.init(img_h, img_w, p.H, p.W));
    const size_t bytes = (size_t)img_h * img_w * 3, pitch = (bytes + 15) / 16 * 16;
    API_TRY(n->img_full.grow(2 * pitch));
    uint8_t* feed0 = (uint8_t*)p.u8_in.p;
    uint8_t* feed1 = (uint8_t*)(p.u8_in.p + p.u8_frame_floats());
    DFVO_HIP_CHECK(hipMemcpyAsync(n->img_full.p, h_img0, bytes, hipMemcpyHostToDevice, p.stream));
    DFVO_HIP_CHECK(hipMemcpyAsync(n->img_full.p + pitch, h_img1, bytes, hipMemcpyHostToDevice, p.stream));
    API_TRY(n->resize.enqueue(n->img_full.p, feed0, p.stream));
    API_TRY(n->resize.enqueue(n->img_full.p + pitch, feed1, p.stream));
    API_TRY(p.forward(feed0, feed1, p.out.p, p.out.p + 16));
    DFVO_HIP_CHECK(hipMemcpyAsync(h_pose16, p.out.p, 16 * sizeof(float), hipMemcpyDeviceToHost, p.stream));
    DFVO_HIP_CHECK(hipStreamSynchronize(p.stream));
    return DFVO_OK;
}
double dfvo_posenet_last_flops(const dfvo_posenet* n) { return n ? n->net.flops_last : 0.0; }
int dfvo_posenet_sync(dfvo_posenet* n) {
    DFVO_ARG_CHECK(n, "null net");
    DFVO_HIP_CHECK(hipStreamSynchronize(n->net.stream));
    return DFVO_OK;
}
int dfvo_depth_postprocess(const float* d_depth, int h, int w, int H, int W, int y0, int y1, int x0, int x1,
                           float min_depth, float max_depth, float* d_raw, double* d_proc, void* stream) {
    DFVO_ARG_CHECK(d_depth && d_raw && d_proc, "dfvo_depth_postprocess: null argument");
    DFVO_ARG_CHECK(h >= 1 && w >= 1 && H >= 1 && W >= 1, "dfvo_depth_postprocess: empty map");
    return launch_depth_post(d_depth, h, w, H, W, y0, y1, x0, x1, min_depth, max_depth, d_raw, d_proc,
                             (hipStream_t)stream);
}
int dfvo_depth_consistency(const float* d_cur_depth, const float* d_ref_depth, int H, int W, const float* h_K, const float* h_Kinv,
                           const float* h_T, float* d_out, void* stream) {
    return launch_depth_consistency(d_cur_depth, d_ref_depth, H, W, h_K, h_Kinv, h_T, d_out, (hipStream_t)stream);
}
int dfvo_depth_consistency_dev(const float* d_cur_depth, const float* d_ref_depth, int H, int W, const float* h_K, const float* h_Kinv,
                               const float* d_T16, float* d_out, void* stream) {
    return launch_depth_consistency_dev(d_cur_depth, d_ref_depth, H, W, h_K, h_Kinv, d_T16, d_out, (hipStream_t)stream);
}
int dfvo_depth_consistency_host(const float* h_cur_depth, const float* h_ref_depth, int H, int W, const float* h_K, const float* h_Kinv,
                                const float* h_T, float* h_out) {
    DFVO_ARG_CHECK(h_cur_depth && h_ref_depth && h_out && H >= 2 && W >= 2, "dfvo_depth_consistency_host: bad argument");
    const size_t px = (size_t)H * W;
    DevArr<float> buf;  // current | reference | result, each on a 16-byte boundary
    const size_t pitch = (px + 3) / 4 * 4;
    API_TRY(buf.alloc(3 * pitch));
    DFVO_HIP_CHECK(hipMemcpyAsync(buf.p, h_cur_depth, px * sizeof(float), hipMemcpyHostToDevice, nullptr));
    DFVO_HIP_CHECK(hipMemcpyAsync(buf.p + pitch, h_ref_depth, px * sizeof(float), hipMemcpyHostToDevice, nullptr));
    int rc = launch_depth_consistency(buf.p, buf.p + pitch, H, W, h_K, h_Kinv, h_T, buf.p + 2 * pitch, nullptr);
    if (rc == DFVO_OK && hipMemcpyAsync(h_out, buf.p + 2 * pitch, px * sizeof(float), hipMemcpyDeviceToHost, nullptr) != hipSuccess) {
        set_last_error("dfvo_depth_consistency_host: copying the result failed");
        rc = DFVO_ERR_HIP;
    }
    return finish(rc, nullptr);  // the buffer dies behind the wait
}
int dfvo_read_depth_u16(const uint16_t* d_src_u16, int src_h, int src_w, double scale, int H, int W, int y0, int y1, int x0, int x1,
                        double min_depth, double max_depth, float* d_raw_f32, double* d_proc_f64, void* stream) {
    DFVO_ARG_CHECK(d_src_u16 && d_raw_f32 && d_proc_f64, "dfvo_read_depth_u16: null argument");
    DFVO_ARG_CHECK(src_h >= 1 && src_w >= 1 && H >= 1 && W >= 1, "dfvo_read_depth_u16: empty map");
    DFVO_ARG_CHECK(scale > 0.0 && scale <= 1.7976931348623157e308, "dfvo_read_depth_u16: scale must be finite and > 0");
    DFVO_ARG_CHECK(0 <= y0 && y0 <= y1 && y1 <= H && 0 <= x0 && x0 <= x1 && x1 <= W, "dfvo_read_depth_u16: crop outside the image");
    return launch_read_depth_u16(d_src_u16, src_h, src_w, scale, H, W, y0, y1, x0, x1, min_depth, max_depth, d_raw_f32, d_proc_f64,
                                 (hipStream_t)stream);
}

}  // extern "C"
