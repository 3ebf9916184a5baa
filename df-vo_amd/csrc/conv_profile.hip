// The per-launch profile of the convolution kernels: HIP events on the launch stream between conv_profile_begin() and
// conv_profile_end() (bench.py's roofline leg, DFVO_CONV_PROFILE_CSV).  Host only: every family's launcher brackets its launch
// with one ConvProfScope (conv.h).
#include "conv.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace dfvo {

struct ConvProfEntry {
    hipEvent_t e0, e1;
    int cfg;
    double flops;
    // N H W Ho Wo cin cout k stride gx gy gz.  gx gy gz are what the launcher passes to ConvProfScope::done(), three conventions:
    //   fp32 kernels (cfg 0-18): the grid -- gz = split-K slices, heads gy = gz = 1
    //   window f16 kernels (cfg 19): gx gy = the grid, gz = the skeleton (1 conv_win_f16s.h, 2 conv_win_f16s2.h, mixed heights too)
    //   generic kernels (cfg 20-23): gx = the grid, gy = cout blocks per wave TC, gz = 100 KSP + 1 (K slices per workgroup);
    //     the tap-window kernel: gy = 0, gz = 7; the fp32 twin conv_gemm_f32g: gy = 0
    int shape[12];
    // the instantiation that ran: "igemm<2,2,4,4>", "f16g<4,1,2,rag> np3", "win3<2,2,4,2,3> tickets" (ConvProfScope::done)
    char variant[48];
};
static std::vector<ConvProfEntry>* g_prof = nullptr;

ConvProfScope::ConvProfScope(const ConvParams& p, hipStream_t stream, int cfg_id) : p_(p), stream_(stream), cfg_(cfg_id) {
    if (!g_prof) return;
    if ((err_ = hipEventCreate(&e0_)) != hipSuccess) return;
    if ((err_ = hipEventCreate(&e1_)) == hipSuccess) err_ = hipEventRecord(e0_, stream_);
}
ConvProfScope::~ConvProfScope() {
    if (e0_) (void)hipEventDestroy(e0_);
    if (e1_) (void)hipEventDestroy(e1_);
}
int ConvProfScope::done(int gx, int gy, int gz, const char* variant, int f16_terms, int splitk) {
    if (err_ != hipSuccess) {  // of the constructor: reported here, where the launcher can return it
        set_last_error(std::string("conv profile events: ") + hipGetErrorString(err_));
        return DFVO_ERR_HIP;
    }
    if (!e1_ || !g_prof) return DFVO_OK;  // no profile is running
    DFVO_HIP_CHECK(hipEventRecord(e1_, stream_));
    g_prof->push_back({e0_, e1_, cfg_, p_.useful_flops,
                       {p_.N, p_.H, p_.W, p_.Ho, p_.Wo, (p_.G0 + p_.G1) * 4, p_.cout, p_.kh, p_.stride, gx, gy, gz}, {0}});
    snprintf(g_prof->back().variant, sizeof(g_prof->back().variant), "%s%s%s", variant,
             f16_terms == 3 ? " np3" : (f16_terms == 1 ? " np1" : ""),
             splitk == CONV_SPLITK_TICKETS ? " tickets" : (splitk == CONV_SPLITK_EPILOGUE ? " epilogue" : ""));
    e0_ = e1_ = nullptr;  // conv_profile_end() destroys them
    return DFVO_OK;
}

void conv_profile_begin() {
    if (!g_prof) g_prof = new std::vector<ConvProfEntry>();
    g_prof->clear();
}
// cfg ids (BM x BN): 0 <2,2,4,4> 128x128  1 <1,4,2,2> 32x128  3 <2,2,2,2> 64x64  5 <2,2,2,1> 64x32  7 <4,1,1,1> 64x16
//   8 <1,4,4,2> 64x128  9 <2,2,4,2> 128x64  10 <4,1,2,2> 128x32  11 <4,1,2,1> 128x16
//   2 4 6: retired, always zero -- the 256-row tiles <4,1,4,4> <4,1,4,2> <4,1,4,1>, which no tile rule ever chose, are no
//   longer built; the rows keep their numbers so that every other row keeps its own
//   LDS-window 3x3 kernel: 12 (8x16)x128  13 (8x16)x64  14 (8x16)x32  15 (4x16)x128
//   16 7x7 heads  17 5x5 heads  18 3x3 heads (direct kernel for cout <= 2; the window kernel (8x16)x16 above that)
//   19 f16 window kernels  20 21 f16 ring kernel (streaming, K-sliced; 20 also the tap-window kernel)  22 23 its fp32 twin
// bytes (optional): ALGORITHMIC HBM bytes of the launches of a configuration -- fp32 input map once + fp32 output map once +
// fp32 weights once (the figure SURVEY.md section 8d prices the streaming layers with); what the kernels really moved comes
// from the PMC passes under profiles/
int conv_profile_end(double* ms, double* flops, int* launches, double* bytes) {
    for (int i = 0; i < CONV_NUM_CFGS; i++) {
        ms[i] = 0;
        flops[i] = 0;
        launches[i] = 0;
        if (bytes) bytes[i] = 0;
    }
    if (!g_prof) return DFVO_OK;
    // DFVO_CONV_PROFILE_CSV=<path>: one line per launch (tuning aid; tests/test_conv_variants_gpu.py reads the last column).
    // variant, the last column, names the instantiation that ran from the launcher's own template arguments and contains
    // commas itself: igemm<WM,WN,TM,TN>, win3<WM,WN,TM,TN,KS>, head<KS,CO,py1|py2>, f16s<WC,WR,TC,TR>, f16s2<WC,WR,TC,TR>,
    // f16s2mix<WC,WR,TC,TRA,TRB>, f16g<WP,KSP,TC[,rag]>, taps<TH,TC>, f32g<WP,KSP,TC>, wino<WN>; then " np3" / " np1" for the
    // kernels that come in f16x3 and f16 form, then " tickets" / " epilogue" for a launch whose K slices over grid.z were
    // finished inside the kernel / by conv_splitk_epilogue
    const char* csv_path = getenv("DFVO_CONV_PROFILE_CSV");
    FILE* csv = csv_path ? fopen(csv_path, "a") : nullptr;
    if (csv) fprintf(csv, "cfg,N,H,W,Ho,Wo,cin,cout,k,stride,gx,gy,gz,us,tflops,variant\n");
    for (auto& e : *g_prof) {
        float t = 0.f;
        DFVO_HIP_CHECK(hipEventSynchronize(e.e1));
        DFVO_HIP_CHECK(hipEventElapsedTime(&t, e.e0, e.e1));
        ms[e.cfg] += t;
        if (csv)
            fprintf(csv, "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%.4f,%.4f,%s\n", e.cfg, e.shape[0], e.shape[1], e.shape[2],
                    e.shape[3], e.shape[4], e.shape[5], e.shape[6], e.shape[7], e.shape[8], e.shape[9], e.shape[10],
                    e.shape[11], t * 1e3, e.flops / (t * 1e-3) / 1e12, e.variant);
        flops[e.cfg] += e.flops;
        launches[e.cfg] += 1;
        if (bytes) {
            const double opx = (double)e.shape[0] * e.shape[3] * e.shape[4], ipx = (double)e.shape[0] * e.shape[1] * e.shape[2];
            const double macs_per_px = opx > 0 ? e.flops / (2.0 * opx) : 0.0;  // cout x cin x kh x kw
            bytes[e.cfg] += 4.0 * (ipx * e.shape[5] + opx * e.shape[6] + macs_per_px);
        }
        (void)hipEventDestroy(e.e0);
        (void)hipEventDestroy(e.e1);
    }
    if (csv) fclose(csv);
    delete g_prof;
    g_prof = nullptr;
    return DFVO_OK;
}

}  // namespace dfvo
