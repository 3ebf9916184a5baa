// Packing and upload of one conv layer's weights (host only; the counterpart of solver_buffers.hip for the nets).  Every
// packing is a DevArr member of ConvLayer: each function releases what it is about to replace, so a layer may be packed
// again -- after a failed attempt or in another precision -- and holds only the last packing afterwards.
#include "nets.h"

namespace dfvo {

const HostTensor* ParamStore::get(const std::string& name) const {
    auto it = t.find(name);
    return it == t.end() ? nullptr : &it->second;
}

template <class T>
static int upload(const T* h, size_t n, DevArr<T>* d, size_t slack = 0) {
    DFVO_TRY(d->alloc(n + slack));
    DFVO_HIP_CHECK(hipMemcpy(d->p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return DFVO_OK;
}

int upload_floats(const std::vector<float>& h, DevArr<float>* d) {
    DFVO_TRY(d->alloc_zeroed(h.size()));
    DFVO_HIP_CHECK(hipMemcpy(d->p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return DFVO_OK;
}

int make_conv(const ParamStore& ps, const std::string& wname, const std::string& bname, int c0, int c1,
              long long M_hint, const float* scale, const float* shift, ConvLayer* L, bool wino_geometry) {
    const HostTensor* w = ps.get(wname);
    if (!w) {
        set_last_error("missing parameter " + wname);
        return DFVO_ERR_STATE;
    }
    DFVO_ARG_CHECK(w->shape.size() == 4, "conv weight must be 4-D: " + wname);
    const HostTensor* b = bname.empty() ? nullptr : ps.get(bname);
    if (!bname.empty() && !b) {
        set_last_error("missing parameter " + bname);
        return DFVO_ERR_STATE;
    }
    L->cout = w->shape[0];
    DFVO_ARG_CHECK(w->shape[1] == c0 + c1, "conv weight cin mismatch: " + wname);
    L->c0 = c0;
    L->c1 = c1;
    L->kh = w->shape[2];
    L->kw = w->shape[3];
    L->cout_pad = conv_cout_pad(L->cout, M_hint);
    L->m_hint = M_hint;
    L->ksteps = conv_ksteps(L->kh, L->kw, c0, c1);
    std::vector<float> pw((size_t)(L->ksteps * 4 + 8) * L->cout_pad * 4), pb(L->cout_pad);  // +8 k-groups: the window kernel rounds each source up to 4 groups
    conv_pack_weights(w->data.data(), b ? b->data.data() : nullptr, L->cout, c0, c1, L->kh, L->kw, L->cout_pad,
                      scale, shift, pw.data(), pb.data());
    DFVO_TRY(L->wp.alloc(pw.size()));
    DFVO_TRY(L->bias.alloc(pb.size()));
    DFVO_HIP_CHECK(hipMemcpy(L->wp, pw.data(), pw.size() * sizeof(float), hipMemcpyHostToDevice));
    DFVO_HIP_CHECK(hipMemcpy(L->bias, pb.data(), pb.size() * sizeof(float), hipMemcpyHostToDevice));
    DFVO_TRY(make_f16s_weights(w->data.data(), L->cout, c0, c1, L->kh, L->kw, scale, L));
    DFVO_TRY(make_f16g_weights(w->data.data(), L->cout, c0, c1, L->kh, L->kw, scale, L));
    DFVO_TRY(make_wino_weights(w->data.data(), L->cout, c0, c1, L->kh, L->kw, scale, wino_geometry, L));
    return make_head_weights(w->data.data(), L->cout, c0, c1, L->kh, L->kw, scale, L);
}

// (the kernels read wf, wg, wg32 and gtab in whole vectors: 256 bytes of slack behind each, in elements)
int make_f16s_weights(const float* w_oihw, int cout, int c0, int c1, int kh, int kw, const float* scale, ConvLayer* L) {
    L->wf.release();
    L->f16_terms = conv_split_mode() == 5 ? 1 : 3;
    if (conv_split_mode() < 4 || kh != 3 || kw != 3) return DFVO_OK;
    std::vector<unsigned short> wf(conv_pack_weights_f16s(w_oihw, cout, c0, c1, scale, nullptr));
    conv_pack_weights_f16s(w_oihw, cout, c0, c1, scale, wf.data());
    DFVO_TRY(upload(wf.data(), wf.size(), &L->wf, 256 / sizeof(unsigned short)));
    L->wf_cout_pad = round_up(cout, 32);
    return DFVO_OK;
}

int make_f16g_weights(const float* w_oihw, int cout, int c0, int c1, int kh, int kw, const float* scale, ConvLayer* L) {
    L->wg32.release();
    L->wg.release();
    L->gtab.release();
    // exact fp32: the register-ring kernel's fp32 weights + the table -- only for layers launch_conv can send there
    // (conv_f32g_takes: launches of at most 8192 output pixels, not the one- / two-channel heads).  m_hint is the builder's
    // pixel count of the layer's INPUT map for the whole batch: a stride-2 Features layer launched one frame at a time has an
    // eighth of it, hence the factor.  The large-map layers used to carry a second, never-read copy of their weights
    // (round-4 advisor); dfvo_conv2d (no hint) packs always.
    const bool f32g = conv_split_mode() == 0 && kh <= 31 && kw <= 31 && (L->m_hint <= 0 || L->m_hint <= 8 * 8192) && cout > 2;
    if (!f32g && (conv_split_mode() < 4 || kh > 31 || kw > 31)) return DFVO_OK;
    std::vector<uint32_t> tab;
    conv_build_f16g_table(c0, c1, kh, kw, &tab);
    if (f32g) {
        std::vector<float> wg(conv_pack_weights_f32g(w_oihw, cout, c0, c1, kh, kw, scale, nullptr));
        conv_pack_weights_f32g(w_oihw, cout, c0, c1, kh, kw, scale, wg.data());
        DFVO_TRY(upload(wg.data(), wg.size(), &L->wg32, 256 / sizeof(float)));
    } else {
        std::vector<unsigned short> wg(conv_pack_weights_f16g(w_oihw, cout, c0, c1, kh, kw, scale, nullptr));
        conv_pack_weights_f16g(w_oihw, cout, c0, c1, kh, kw, scale, wg.data());
        DFVO_TRY(upload(wg.data(), wg.size(), &L->wg, 256 / sizeof(unsigned short)));
    }
    DFVO_TRY(upload(tab.data(), tab.size(), &L->gtab, 256 / sizeof(uint32_t)));
    L->wg_cout_pad = round_up(cout, 32);
    L->g_steps = (int)(tab.size() / 4);
    return DFVO_OK;
}

// fp32 Winograd: U of the 3x3 layers packed in "fp32" while the switch is on.  The decision is the layer's from here on
// (launch_conv looks at the pointer, never at the switch), so a captured graph replays what was packed.  U is 16 / 9 of the
// weight bytes: it is not packed for a layer that no launch can hand to the kernel -- geometry_ok false (the builder knows
// the layer runs with a stride, reflection padding or the upsampled source), or, in mode 1, a width or a map (m_hint pixels
// at the most) that the size rule never accepts.  launch_conv still declines per launch what the kernel does not compute.
int make_wino_weights(const float* w_oihw, int cout, int c0, int c1, int kh, int kw, const float* scale, bool geometry_ok,
                      ConvLayer* L) {
    L->wu.release();
    L->wino_mode = 0;
    const int mode = conv_fp32_winograd_mode();
    if (conv_split_mode() != 0 || mode == 0 || kh != 3 || kw != 3 || cout <= 2 || !geometry_ok) return DFVO_OK;
    if (mode == 1 && !conv_wino_rule_may_accept(cout, L->m_hint)) return DFVO_OK;
    std::vector<float> wu(conv_wino_f32_weight_floats(cout, c0, c1));
    conv_pack_weights_wino_f32(w_oihw, cout, c0, c1, scale, wu.data());
    DFVO_TRY(upload(wu.data(), wu.size(), &L->wu));
    L->wino_mode = mode;
    return DFVO_OK;
}

int make_head_weights(const float* w, int cout, int c0, int c1, int kh, int kw, const float* scale, ConvLayer* L) {
    L->wh.release();
    if (cout > 2 || kh != kw || (kh != 3 && kh != 5 && kh != 7)) return DFVO_OK;
    std::vector<float> ph(conv_head_weight_floats(cout, c0, c1, kh));
    conv_pack_head_weights(w, cout, c0, c1, kh, scale, ph.data());
    return upload(ph.data(), ph.size(), &L->wh);
}

}  // namespace dfvo
