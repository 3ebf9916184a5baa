/* libdfvo_hip.so -- C ABI of the MI355X (gfx950) DF-VO tracking hot path.
 *
 * The reference (Huangying-Zhan/DF-VO) has no FFI: its boundary is the Python class surface that
 * libs/dfvo.py consumes.  This header is the C ABI placed underneath that
 * surface; each entry point names the reference call site it replaces (paths relative to
 * /root/reference).  The Python mirror classes in df-vo_amd/libs bind these symbols with ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, a negative DFVO_ERR_* code otherwise;
 *     dfvo_last_error() returns a thread-local human readable message for the last failure.
 *   - "d_" arguments are DEVICE pointers (HBM), "h_" arguments are HOST pointers.  Nothing is
 *     retained after the call returns unless stated.
 *   - `stream` is a hipStream_t passed as void* (NULL = the object's own stream).
 *   - images are uint8 HWC RGB; activations are NHWC float32; dense maps are row-major.
 *   - handles are opaque, not re-entrant per handle, independent across handles.
 */
#ifndef DFVO_HIP_H
#define DFVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFVO_OK 0
#define DFVO_ERR_HIP (-1)
#define DFVO_ERR_ARG (-2)
#define DFVO_ERR_STATE (-3)
#define DFVO_ERR_RANGE (-4) /* f16x3 / f16 packing: an activation left f16's range in this call (see dfvo_f16s_overflow_count) */
#define DFVO_ERR_EMPTY_SELECTION (-5) /* dfvo_scale_recovery_iterative: a round selected no rigid-flow keypoint (the reference asserts) */
#define DFVO_ERR_NO_CONSENSUS (-6)    /* dfvo_scale_recovery_iterative: sklearn's "RANSAC could not find a valid consensus set" */
#define DFVO_ERR_JPEG (-7)            /* dfvo_jpeg_probe / _entropy_decode: a file that is refused or corrupt; the message says which */

const char* dfvo_last_error(void);
/* number of visible HIP devices (0 when there is none); never fails */
int dfvo_device_count(void);
int dfvo_set_device(int ordinal);
int dfvo_sync_device(void);

/* ---- raw device memory helpers (plumbing for hosts without torch) ---- */
int dfvo_malloc(void** d_ptr, size_t bytes);
int dfvo_free(void* d_ptr);
int dfvo_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int dfvo_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);

/* =====================================================================================
 * Unit-testable operators (each is one kernel launch; used by the nets below)
 * ===================================================================================== */

/* torch.nn.Conv2d + bias + activation (+ residual, + reflection pad, + x2 nearest upsample of
 * source 0, + channel concat of two sources) as an fp32 MFMA implicit GEMM.
 *   lite_flow_net.py:39-75,121-129,171-179,211-240; depth_decoder.py:50-65; layers.py:106-136
 * Weights are given in torch OIHW layout on the HOST (cin = c0 + c1) and packed internally. */
typedef struct dfvo_conv_desc {
    int N, H, W;              /* input batch / spatial size the taps index (after upsample) */
    int kh, kw, stride, pad_h, pad_w;
    int pad_mode;             /* 0 zeros, 1 reflect */
    int c0, cs0, co0, up0;    /* source 0: logical channels, floats per pixel, channel offset, x2 nearest */
    int c1, cs1, co1;         /* source 1 (c1 = 0: absent) */
    int cout;
    int act;                  /* 0 none, 1 leaky(act_param), 2 relu, 3 elu(act_param), 4 sigmoid */
    float act_param;
    int res_cs, res_co;       /* residual view (used when d_res != NULL) */
    int dst_cs, dst_co;
    int dst_zero_to;          /* != 0: the epilogue also zero-fills channels [cout, dst_zero_to) of dst (the flow net's
                                 distance convolutions pad k*k to a multiple of 4 this way) */
} dfvo_conv_desc;
int dfvo_conv2d(const dfvo_conv_desc* desc, const float* d_src0, const float* d_src1, const float* h_weight_oihw,
                const float* h_bias, const float* d_res, float* d_dst, void* stream);

/* Per-launch timing of the conv kernel family with HIP events recorded on the launch stream (the
 * roofline leg of bench.py).  Between begin and end every conv launch is bracketed by two events;
 * end() returns, per tile configuration (0: 128x128, 1: 32x128, 2: 256x64, 3: 64x64, 4: 256x32,
 * 5: 64x32, 6: 256x16, 7: 64x16, 8: 64x128, 9: 128x64, 10: 128x32, 11: 128x16, 12-15: the LDS-window 3x3 kernel
 * with (8x16)x128, (8x16)x64, (8x16)x32, (4x16)x128 tiles, 16/17/18: the 7x7 / 5x5 / 3x3 one- and two-channel
 * heads (direct kernel; wider 5x5 / 7x7 layers use the window kernel under the same ids); arrays of 19), the
 * summed duration [ms], useful FLOPs and launch count.
 * Do not use while a hipGraph capture is active (disable graphs on the nets first). */
/* arithmetic of the convolution layers packed AFTER this call (nets are packed at *_finalize):
 *   "fp32"   exact fp32 MFMA (v_mfma_f32_16x16x4_f32), the library default
 *   "f16x3"  fp32-class: operands split into two f16 planes (22 mantissa bits), three exact products per term on
 *            v_mfma_f32_32x32x16_f16, fp32 accumulate (df-vo_amd/csrc/conv_win_f16s.h); what bench.py's headline and
 *            the drop-in classes (DeepModel.initialize_models) select
 *   "f16"    NOT fp32-class: operands rounded to f16 (the hi plane alone), one product per term, fp32 accumulate, fp32
 *            activations between layers -- BASELINE config 5's "fp16 flow" (hard part 4: reported
 *            separately, with its flow / keypoint / pose deltas); the one- and two-channel heads stay exact fp32
 * Also read once from the environment variable DFVO_CONV_PRECISION. */
int dfvo_set_conv_precision(const char* name);
/* the current setting ("fp32" | "f16x3" | "f16"): a caller that sets it for its own nets restores it afterwards */
const char* dfvo_get_conv_precision(void);
/* Which scikit-learn the scale-recovery RANSAC (sklearn.linear_model.RANSACRegressor, E_tracker.py:618-636) reproduces
 * where the versions differ: r2_score of a one-sample consensus set is nan from 0.22 on (every later trial with the same
 * inlier count then wins), 1.0 / 0.0 in 0.20.3 -- the version the reference pins (envs/requirement.yml:233) and the
 * default here.  version: "<major>.<minor>[.patch]" of the scikit-learn to reproduce (process-wide, takes effect with the
 * next scale recovery). */
int dfvo_set_sklearn_compat(const char* version);
/* f16x3 range report: the hi plane of the split is f16, so an activation with |x| > 65504 does not fit -- it becomes
 * +-inf and propagates as inf / NaN into the layer's output (never a silently clamped product).  Every splitting kernel
 * counts the threads that saw such an activation, the packer the weights (those are clamped, and counted);
 * *h_count = events since the last reset (0 = the f16x3 result is the 22-bit split of the true operands everywhere).
 * reset != 0 clears the counter. */
int dfvo_f16s_overflow_count(unsigned long long* h_count, int reset);
/* Opt-in Winograd F(2x2,3x3) for the layers packed in "fp32" (df-vo_amd/csrc/conv_wino_f32.hip): all-fp32 arithmetic, 16
 * instead of 36 multiplications per 2x2 output tile, NOT bit-identical to the direct fp32 kernels (its error bound is the
 * fp32 row's constant on the magnitudes of the transformed products: tests/wino_bounds.py).
 * 0 off (default); 1 on (experimental): 3x3 / stride-1 / zero-pad-1 layers with cout > 2 that the size rule accepts run as
 * Winograd (64- and 128-wide layers on maps of at least 30000 pixels: DESIGN.md section 5d);
 * 2 on for every such layer whatever its size (unit tests).  Reflection padding and the x2-upsampled source stay on the
 * direct kernels.  No effect on layers packed as f16x3 / f16.
 * Read when a layer is packed (nets: *_finalize; dfvo_conv2d: per call); also from DFVO_FP32_WINOGRAD once. */
int dfvo_set_fp32_winograd(int mode);
int dfvo_get_fp32_winograd(void);
/* launches of the Winograd kernel since the last reset (counted on the host when the launch is enqueued; a replayed
 * hipGraph does not count again).  reset != 0 clears the counter. */
int dfvo_fp32_winograd_launches(unsigned long long* h_count, int reset);
int dfvo_conv_profile_begin(void);
int dfvo_conv_profile_end(double* h_ms24, double* h_flops24, int* h_launches24);
/* the same, plus the ALGORITHMIC HBM bytes of each configuration's launches (fp32 input map + output map + weights, each
 * once: SURVEY.md section 8d's price of the streaming layers) -- the numerator of bench.py's roofline.hbm entry */
int dfvo_conv_profile_end_bytes(double* h_ms24, double* h_flops24, int* h_launches24, double* h_bytes24);

/* correlation.py:38-106,281-340 (_FunctionCorrelation.forward) followed by leaky_relu(slope)
 * (lite_flow_net.py:145,148).  NHWC inputs [N,H,W,C]; output [N,ceil(H/s),ceil(W/s),52], 49 used.
 * slope = 1 gives the bare correlation. */
int dfvo_correlation(const float* d_first, const float* d_second, int N, int H, int W, int C, int stride,
                     float slope, float* d_out, void* stream);

/* Backward() bilinear warp, lite_flow_net.py:10-28.  h_lin_x/h_lin_y: torch.linspace(-1,1,W/H)
 * tables (HOST; NULL = library formula). */
int dfvo_backward_warp(const float* d_src, const float* d_flow, float flow_mult, int N, int H, int W, int C,
                       const float* h_lin_x, const float* h_lin_y, float* d_dst, void* stream);

/* The flow net's non-conv launches with every argument the net passes (FlowNet::enqueue_levels), for the per-operator
 * tests.  NHWC float views (pointer, floats per pixel, channel offset); h_lin_x / h_lin_y: torch.linspace(-1,1,W/H) on the
 * HOST.  Each call returns after the launch has finished on `stream`.
 * dfvo_warp_view: Backward() of source sample (swap ? N-1-n : n) at (x, y) + flow * mult into dst channels [dco, dco + C);
 * append_flow: dst channels C, C+1 = the flow, C+2, C+3 = 0; step > 1: only the pixels y % step == 0, x % step == 0.
 * C, scs, sco, dcs and dco are multiples of 4.  dfvo_warp_view and dfvo_reg_prep refuse H < 2 or W < 2 with DFVO_ERR_ARG (and so
 * do the launchers under them): the sampling grid divides by (W - 1) / 2 and (H - 1) / 2. */
int dfvo_warp_view(const float* d_src, int scs, int sco, int swap, const float* d_flow, int fcs, int fco, float mult, int N,
                   int H, int W, int C, const float* h_lin_x, const float* h_lin_y, float* d_dst, int dcs, int dco,
                   int append_flow, int step, void* stream);
/* correlation of first[n] with second[swap2 ? N-1-n : n] + leaky_relu(slope) into d_out [N, ceil(H/s), ceil(W/s), dcs] */
int dfvo_correlation_view(const float* d_first, int cs1, int co1, const float* d_second, int cs2, int co2, int swap2, int N,
                          int H, int W, int C, int stride, float slope, float* d_out, int dcs, void* stream);
/* per-sample mean of a 2-channel flow view over H*W pixels -> d_mean [N][2] (lite_flow_net.py:255) */
int dfvo_flow_mean(const float* d_flow, int fcs, int fco, int N, int HW, float* d_mean, void* stream);
/* Regularization input, lite_flow_net.py:244-255: d_dst [N,H,W,4] = (sqrt(sum_c (img[n] - warp(img[N-1-n]))^2 + 1e-6),
 * flow - mean[n], 0); d_img NHWC4, d_mean [N][2] on the device */
int dfvo_reg_prep(const float* d_img, const float* d_flow, int fcs, int fco, float mult, const float* d_mean, int N, int H,
                  int W, const float* h_lin_x, const float* h_lin_y, float* d_dst, void* stream);
/* Regularization output head, lite_flow_net.py:256-264: softmax of -dist^2 over the k*k taps, weighted with the zero-padded
 * k x k unfold of the flow and moduleScaleX / Y (h_wx, h_wy: k*k floats each); k odd, 1 .. 9 */
int dfvo_reg_head(const float* d_dist, int dist_cs, int k, const float* d_flow, int fcs, int fco, const float* h_wx, float bx,
                  const float* h_wy, float by, int N, int H, int W, float* d_dst, int dcs, int dco, void* stream);
/* Which kernel the three dispatching launchers run for given arguments: the launchers call the same pure functions
 * (df-vo_amd/csrc/ops.h), with the same environment switches, read once per process.  Nothing is launched.
 * dfvo_deconv_variant: dfvo_deconv_dw4x4s2(C, cs) -> 0 k_deconv_dw4_blk (cs a multiple of 4 with room for C's last quad, C <= 512,
 *   DFVO_DECONV_BLK not 0), 1 k_deconv_dw4 (such a view otherwise), 2 k_deconv_dw (any other cs).  The two quad kernels write the
 *   pad channels [C, round_up(C, 4)) of the destination as zeros; the scalar kernel writes channels [0, C) alone.
 * dfvo_correlation_variant: 100 K + 10 TH + TW, K = C / 32 for k_correlation_rt<K> (C = 32, 64, 96, 128, 192 unless DFVO_CORR_RT=0)
 *   and 0 for k_correlation, TH x TW the output tile; -1 where dfvo_correlation_view refuses (C or a view no multiple of 4, a tile
 *   beyond 160 KB of LDS: C > 352).
 * dfvo_reg_head_variant: k for k_reg_head_v<k> (k = 3, 5, 7; d_dist 16-byte aligned with dist_cs a multiple of 4 and at least
 *   round_up(k * k, 4); flow and destination views 8-byte aligned; DFVO_REG_HEAD_V not 0), 0 for k_reg_head. */
int dfvo_deconv_variant(int C, int cs);
int dfvo_correlation_variant(int C, int cs1, int co1, int cs2, int co2);
int dfvo_reg_head_variant(const float* d_dist, int dist_cs, int k, const float* d_flow, int fcs, int fco, const float* d_dst, int dcs,
                          int dco);
/* the net's output stage: level-2 flow x scale, bilinear (align_corners) to H x W, x (W/w, H/h) -> d_fwd / d_bwd [2,H,W]
 * (samples 0 / 1), d_diff [H,W] = forward-backward consistency (deep_flow.py:107-129,171-196) */
int dfvo_flow_post(const float* d_netflow, int fcs, int fco, int h, int w, float scale, int H, int W, float* d_fwd,
                   float* d_bwd, float* d_diff, void* stream);
/* uint8 [H,W,3] -> float NHWC4 [th,tw,4] = bilinear (align_corners) of u8 / 255, channel 3 = 0 (the net's input) */
int dfvo_img_u8_to_flow_input(const uint8_t* d_img, int H, int W, float* d_dst, int th, int tw, void* stream);

/* depthwise ConvTranspose2d(k=4, s=2, p=1, bias=False), lite_flow_net.py:109,117. h_weight [C,1,4,4] */
int dfvo_deconv_dw4x4s2(const float* d_src, int N, int H, int W, int C, int cs, const float* h_weight,
                        float* d_dst, void* stream);

/* F.max_pool2d(kernel_size=3, stride=2, padding=1) on dense NHWC, C % 4 == 0 (the monodepth2 encoder's pool; NaN propagates
 * as in torch) -- d_dst [N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C] */
int dfvo_maxpool3x3s2(const float* d_src, int N, int H, int W, int C, float* d_dst, void* stream);

/* F.interpolate(mode='bilinear') on dense NHWC, C % 4 == 0 */
/* uint8 [H,W,3] -> uint8 [out_h,out_w,3], bit-exact with Pillow's Image.resize((out_w,out_h), Image.LANCZOS): 22-bit
 * fixed-point coefficient tables, horizontal pass then vertical pass, each rounded to uint8 (replaces the host-side
 * PIL call at deep_models.py:195-199).  Builds the tables per call; the nets keep theirs resident. */
int dfvo_resize_lanczos_u8(const uint8_t* d_src, int H, int W, uint8_t* d_dst, int out_h, int out_w, void* stream);
/* the resize's fixed-point tables for one axis (host only, no device needed): h_bounds [out_size][2] = (first input
 * sample, count), h_coeffs [out_size][*ksize] 22-bit coefficients (coeff_cap ints available) -- Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc */
int dfvo_lanczos_coeffs(int in_size, int out_size, int* h_bounds, int* h_coeffs, int coeff_cap, int* ksize);
/* uint8 [H,W,C] (C <= 4) -> uint8 [out_h,out_w,C] = cv2.resize(img, (out_w, out_h)) with the default INTER_LINEAR, the
 * resize of the loaded frame to the configured size in read_image (libs/general/utils.py:51): OpenCV 3.4.3's 11-bit
 * fixed-point bilinear arithmetic (exact 2 x 2 decimation: its (a + b + c + d + 2) >> 2 area path).  Asynchronous on
 * `stream`. */
int dfvo_resize_linear_u8(const uint8_t* d_src, int H, int W, int C, uint8_t* d_dst, int out_h, int out_w, void* stream);
/* Everything of read_image (libs/general/utils.py:44-51) behind the decoder, in one launch on the decoded frame as cv2.imread
 * left it: cv2.cvtColor(img, COLOR_BGR2RGB) (bgr != 0: channel order reversed while reading), the crop img[y0:y1, x0:x1]
 * (pass 0, img_h, 0, img_w for none; the caller evaluates int(img_h * crop[0][0]) ... as utils.py:47-49 does) and
 * cv2.resize(img, (out_w, out_h)) with dfvo_resize_linear_u8's arithmetic.  d_decoded uint8 [img_h, img_w, 3], d_dst uint8
 * [out_h, out_w, 3].  PNG / JPEG entropy decoding stays on the host (bit-serial). */
int dfvo_read_image_tail_u8(const uint8_t* d_decoded, int img_h, int img_w, int bgr, int y0, int y1, int x0, int x1, uint8_t* d_dst,
                            int out_h, int out_w, void* stream);
/* The same tail for a 1-channel decoded frame, d_decoded uint8 [img_h, img_w] (KITTI's grey cameras; any file cv2.imread would
 * replicate into three equal channels): d_dst uint8 [out_h, out_w, 3] holds exactly the bytes dfvo_read_image_tail_u8 writes for
 * the replicated frame, from a third of the source bytes. */
int dfvo_read_image_tail_gray_u8(const uint8_t* d_decoded, int img_h, int img_w, int y0, int y1, int x0, int x1, uint8_t* d_dst,
                                 int out_h, int out_w, void* stream);
/* Device frame ring: the upload stage of a sequence read from disk.  `slots` pinned staging buffers of capacity_bytes each with
 * matching device buffers, one non-blocking stream of the ring's own and one event per slot.
 * Threads: every dfvo_frame_ring_* call comes from ONE thread (the consumer, which also drives the pipeline); decoder threads only
 * write decoded frames into the staging memory dfvo_frame_ring_staging hands out, and the caller orders those writes before the
 * slot's submit.
 * dfvo_frame_ring_submit_image: one asynchronous copy of the staged uint8 [img_h, img_w, channels] frame (channels 3, or 1 for a
 * grey frame), then dfvo_read_image_tail_u8 / _gray_u8 with these arguments into d_dst uint8 [out_h, out_w, 3], then an event
 * record; returns without waiting.  dfvo_frame_ring_submit_raw: the copy of `bytes` staged bytes straight into d_dst and the
 * event, no kernel (the uint16 [src_h, src_w] depth images dfvo_pipeline_enqueue_nets_depth takes).  d_dst is the caller's and
 * stays allocated until the slot's wait has returned.
 * dfvo_frame_ring_wait: hipEventSynchronize on the slot's event -- the hand-over point of the pipeline's ordering contract below
 * (a frame is complete when handed to dfvo_pipeline_enqueue_nets / _set_ref_image); a slot with nothing submitted returns at once.
 * DFVO_ERR_ARG, with a message and nothing enqueued: a frame larger than the staging capacity, a slot outside the ring, a crop
 * outside the frame, a submit on a slot whose last submit has not been waited for.
 * dfvo_frame_ring_pending: the number of such slots.  dfvo_frame_ring_destroy synchronises the ring's stream first. */
typedef struct dfvo_frame_ring dfvo_frame_ring;
int dfvo_frame_ring_create(int slots, size_t capacity_bytes, dfvo_frame_ring** out);
void dfvo_frame_ring_destroy(dfvo_frame_ring* ring);
int dfvo_frame_ring_staging(dfvo_frame_ring* ring, int slot, void** h_staging, size_t* capacity_bytes);
int dfvo_frame_ring_submit_image(dfvo_frame_ring* ring, int slot, int img_h, int img_w, int channels, int bgr, int y0, int y1, int x0,
                                 int x1, uint8_t* d_dst, int out_h, int out_w);
int dfvo_frame_ring_submit_raw(dfvo_frame_ring* ring, int slot, size_t bytes, void* d_dst);
int dfvo_frame_ring_wait(dfvo_frame_ring* ring, int slot);
int dfvo_frame_ring_pending(dfvo_frame_ring* ring, int* n_pending);
/* Raw camera frames: bilinear Bayer demosaic and undistortion through a per-pixel table, in one launch (what the RobotCar SDK does on
 * the host: sdk_python/image.py load_image = demosaicing_CFA_Bayer_bilinear, camera_model.py undistort = scipy.ndimage.map_coordinates
 * of order 1 per channel, astype(uint8)).  Only the pixels of the box [y0, y1) x [x0, x1) of d_rgb uint8 [h, w, 3] are written -- the
 * crop the read-image tail will read; the rest of the plane is left as it is.
 * Demosaic: plane P_c holds the mosaic where the site's colour is c and 0 elsewhere; `pattern` names the colours of sites (0,0),
 * (0,1), (1,0), (1,1).  R and B are P convolved with [[1,2,1],[2,4,2],[1,2,1]] / 4, G with [[0,1,0],[1,4,1],[0,1,0]] / 4, the plane
 * extended over the border by `border`: DFVO_BORDER_REFLECT maps -1 -> 0 and n -> n - 1 (scipy.ndimage.convolve's default),
 * DFVO_BORDER_MIRROR -1 -> 1 and n -> n - 2 (needs h, w >= 2).  Every value is a multiple of 1/4, exact.  Under REFLECT the
 * one-pixel frame of a plane can exceed 255 (a site counted twice); its byte is the truncated value's low 8 bits.
 * Remap: the table holds, for every output pixel, the (x, y) of its sample in the source frame V (the demosaiced mosaic, float64,
 * or the distorted uint8 RGB frame).  Outside 0 <= y <= h - 1, 0 <= x <= w - 1 the pixel is 0 on all channels; else with
 * fy = floor(y), ty = y - fy, wy = {1 - ty, ty} (x alike): t = 0; for a, b in (0, 1): c = V[min(fy + a, h - 1)][min(fx + b, w - 1)];
 * c = c * wy[a]; c = c * wx[b]; t = t + c -- float64, every operation rounded once, nothing contracted; the byte is t truncated.
 * dfvo_undistort_create: map_xy float64 [2][h * w] on the host, the x coordinates then the y coordinates, row-major -- the layout
 * of the SDK's <camera>_distortion_lut.bin; kept on the device interleaved.  A non-finite entry is DFVO_ERR_ARG.
 * dfvo_undistort_mosaic_u8: d_mosaic uint8 [img_h, img_w]; map NULL = demosaic only, else a map of that size.
 * dfvo_undistort_rgb_u8: d_src uint8 [h, w, 3] of the map's size, not d_rgb.  d_rgb is 4-byte aligned.  Asynchronous on `stream`.
 * Argument errors are DFVO_ERR_ARG with a message, before anything is enqueued. */
typedef struct dfvo_undistort_map dfvo_undistort_map;
enum { DFVO_BAYER_RGGB = 0, DFVO_BAYER_BGGR = 1, DFVO_BAYER_GRBG = 2, DFVO_BAYER_GBRG = 3 };
enum { DFVO_BORDER_REFLECT = 0, DFVO_BORDER_MIRROR = 1 };
int dfvo_undistort_create(int h, int w, const double* map_xy, dfvo_undistort_map** out);
void dfvo_undistort_destroy(dfvo_undistort_map* map);
int dfvo_undistort_mosaic_u8(const dfvo_undistort_map* map, const uint8_t* d_mosaic, int img_h, int img_w, int pattern, int border,
                             int y0, int y1, int x0, int x1, uint8_t* d_rgb, void* stream);
int dfvo_undistort_rgb_u8(const dfvo_undistort_map* map, const uint8_t* d_src, int y0, int y1, int x0, int x1, uint8_t* d_rgb,
                          void* stream);
/* A staged mosaic through the ring: the asynchronous copy of the slot's uint8 [img_h, img_w] frame, dfvo_undistort_mosaic_u8 with
 * these arguments into one RGB plane the ring owns (allocated at the first such submit; every submit runs on the ring's one
 * stream, so one plane serves all slots), dfvo_read_image_tail_u8 of the box into d_dst uint8 [out_h, out_w, 3], the slot's event.
 * `map` (or NULL) stays alive until the slot's wait has returned.  Errors as dfvo_frame_ring_submit_image's. */
int dfvo_frame_ring_submit_mosaic(dfvo_frame_ring* ring, int slot, const dfvo_undistort_map* map, int pattern, int border, int img_h,
                                  int img_w, int y0, int y1, int x0, int x1, uint8_t* d_dst, int out_h, int out_w);
int dfvo_resize_bilinear(const float* d_src, int N, int H, int W, int C, float* d_dst, int Ho, int Wo,
                         int align_corners, void* stream);
/* Baseline JPEG frames: the bit-serial Huffman pass on the host, everything behind it on the device, with the arithmetic of
 * libjpeg-turbo's default decompression path restated exactly -- the pixels are Pillow's (libjpeg-turbo) byte for byte for every
 * file a conforming encoder wrote (docs/parity.md; parity with OpenCV's decoder is not established).
 * Decoded: baseline sequential (SOF0), 8-bit samples, 8-bit quantisation tables, Huffman coding, one interleaved scan of one
 * component (grey) or three (YCbCr, luma sampling 1x1, 2x1 or 2x2, chroma 1x1), restart intervals.  DFVO_ERR_JPEG with a message
 * that names the reason: progressive and every other SOFn, 12-bit samples, 16-bit tables, arithmetic coding, four components, any
 * other sampling, more than one scan, a missing table, a Huffman code that is not in its table, a coefficient index past 63, data
 * that ends early, a bad restart marker, bytes that are no JPEG, a capacity that is too small (nothing is truncated).  No input
 * makes either host call read outside h_bytes[0 .. n) or write outside h_dst[0 .. capacity_bytes).
 * The buffer (dfvo_jpeg_entropy_decode's h_dst, 8-byte aligned; dfvo_jpeg_decode_u8's d_coeffs is its device copy): the
 * dfvo_jpeg_info at byte 0, and from byte plane_offset[c] the quantised coefficients of component c as int16 in natural
 * (de-zigzagged) order, 64 per block, the blocks in raster order of the component's padded grid blocks_h[c] x blocks_w[c] (whole
 * MCUs); info.bytes in all, at most DFVO_JPEG_HEADER_BYTES + 6 bytes per pixel of the padded frame.
 * dfvo_jpeg_probe: the header only (sizes a ring: info.bytes).  dfvo_jpeg_entropy_decode: the whole host pass; neither touches
 * the device, both are re-entrant (decoder threads call them).
 * dfvo_jpeg_decode_u8: dequantisation, the 13-bit "slow integer" IDCT (columns, then rows), triangle-filter upsampling over the
 * component's own downsampled size with the edge sample replicated, 16-bit fixed-point YCbCr -> RGB; d_dst uint8 [height, width,
 * 3], or [height, width] for a one-component file.  At most two launches, asynchronous on `stream`.  d_coeffs is the workspace:
 * its coefficients are overwritten.  `info` (host) is checked against the layout of its own size and sampling (DFVO_ERR_ARG).
 * Coefficient data no conforming encoder writes decodes deterministically and memory-safely, to pixels that need not be libjpeg's. */
#define DFVO_JPEG_HEADER_BYTES 512
typedef struct dfvo_jpeg_info {
    int32_t width, height, components;  /* components: 1 (grey) or 3 (YCbCr) */
    int32_t h_samp, v_samp;             /* luma sampling factors; chroma is 1x1 */
    int32_t blocks_w[3], blocks_h[3];   /* padded block grid per component */
    int32_t comp_w[3], comp_h[3];       /* the component's own (downsampled) size in samples */
    uint16_t quant[3][64];              /* the component's quantisation table, natural order */
    int32_t reserved;
    uint64_t plane_offset[3];           /* bytes from the start of the buffer to the component's coefficients */
    uint64_t bytes;                     /* header and coefficients */
} dfvo_jpeg_info;
int dfvo_jpeg_probe(const uint8_t* h_bytes, size_t n, dfvo_jpeg_info* info);
int dfvo_jpeg_entropy_decode(const uint8_t* h_bytes, size_t n, void* h_dst, size_t capacity_bytes, dfvo_jpeg_info* info);
int dfvo_jpeg_decode_u8(uint8_t* d_coeffs, const dfvo_jpeg_info* info, uint8_t* d_dst, void* stream);
/* A staged JPEG through the ring: the slot's staging memory holds what dfvo_jpeg_entropy_decode wrote.  The asynchronous copy of
 * its header and coefficients, dfvo_jpeg_decode_u8 into the ring's shared plane (dfvo_frame_ring_submit_mosaic's, grown the same
 * way), dfvo_read_image_tail_u8 -- _gray_u8 for a one-component file -- of the box into d_dst uint8 [out_h, out_w, 3], the slot's
 * event.  Errors as dfvo_frame_ring_submit_image's; a header that is not the layout of its own size is DFVO_ERR_ARG. */
int dfvo_frame_ring_submit_jpeg(dfvo_frame_ring* ring, int slot, int y0, int y1, int x0, int x1, uint8_t* d_dst, int out_h, int out_w);

/* =====================================================================================
 * LiteFlowNet forward/backward flow + consistency   (replaces LiteFlow.inference_flow,
 * lite_flow.py:89-148, behind DeepModel.forward_flow, deep_models.py:144-182)
 * ===================================================================================== */
typedef struct dfvo_flownet dfvo_flownet;
int dfvo_flownet_create(int img_h, int img_w, void* stream, dfvo_flownet** out);
void dfvo_flownet_destroy(dfvo_flownet* net);
/* state_dict entry by its key (lite_flow.py:45-46), float32 HOST data; also accepts the optional
 * "aux.linspace_x.<level>" / "aux.linspace_y.<level>" tables (level 2..6). */
int dfvo_flownet_set_param(dfvo_flownet* net, const char* name, const float* h_data, int ndim, const int* shape);
int dfvo_flownet_finalize(dfvo_flownet* net);
/* flow-net input size for an image size (host only, no device needed): DeepFlow.get_target_size (deep_flow.py:89-105) as
 * the reference really evaluates it -- its rebinding of h / w makes the result (floor, floor) multiples of 32 (KITTI
 * 376 x 1241 -> 352 x 1216) unless float64 rounding tips it to (ceil, ceil) (192 x 640 -> 224 x 672) */
int dfvo_flow_target_size(int img_h, int img_w, int* net_h, int* net_w);
int dfvo_flownet_net_size(const dfvo_flownet* net, int* net_h, int* net_w);
int dfvo_flownet_set_graph(dfvo_flownet* net, int enable);
/* device in, device out: ref/cur uint8 [H,W,3]; fwd,bwd float [2,H,W]; diff float [H,W] */
int dfvo_flownet_forward(dfvo_flownet* net, const uint8_t* d_ref, const uint8_t* d_cur, float* d_fwd, float* d_bwd,
                         float* d_diff);
/* host in, host out (synchronous) */
int dfvo_flownet_forward_host(dfvo_flownet* net, const uint8_t* h_ref, const uint8_t* h_cur, float* h_fwd,
                              float* h_bwd, float* h_diff);
/* conv + correlation FLOPs (2 x MAC, unpadded) enqueued by the last forward */
double dfvo_flownet_last_flops(const dfvo_flownet* net);
/* debugging / parity: copy the final flow of pyramid level 2..6 ([2,h,w,2] float, HOST) */
int dfvo_flownet_get_level_flow(dfvo_flownet* net, int level, float* h_out, int* h, int* w);
int dfvo_flownet_sync(dfvo_flownet* net);

/* =====================================================================================
 * monodepth2 depth  (replaces Monodepth2DepthNet.inference_depth, monodepth2.py:91-139,
 * behind DeepModel.forward_depth, deep_models.py:184-206)
 * ===================================================================================== */
typedef struct dfvo_depthnet dfvo_depthnet;
int dfvo_depthnet_create(int feed_h, int feed_w, float min_depth, float max_depth, float baseline_mult,
                         void* stream, dfvo_depthnet** out);
void dfvo_depthnet_destroy(dfvo_depthnet* net);
/* keys of encoder.pth ("encoder.conv1.weight", ...) and depth.pth ("decoder.0.conv.conv.weight", ...) */
int dfvo_depthnet_set_param(dfvo_depthnet* net, const char* name, const float* h_data, int ndim, const int* shape);
int dfvo_depthnet_finalize(dfvo_depthnet* net);
int dfvo_depthnet_set_graph(dfvo_depthnet* net, int enable);
/* img uint8 [feed_h, feed_w, 3] -> depth float [feed_h, feed_w] (metres, x baseline multiplier) */
int dfvo_depthnet_forward(dfvo_depthnet* net, const uint8_t* d_img, float* d_depth);
int dfvo_depthnet_forward_host(dfvo_depthnet* net, const uint8_t* h_img, float* h_depth);
/* DeepModel.forward_depth in one call (deep_models.py:184-206): host uint8 image [img_h,img_w,3] of any size ->
 * Pillow-exact LANCZOS resize to the feed size on the device -> net -> host depth [feed_h,feed_w] */
int dfvo_depthnet_forward_image_host(dfvo_depthnet* net, const uint8_t* h_img, int img_h, int img_w, float* h_depth);
double dfvo_depthnet_last_flops(const dfvo_depthnet* net);
int dfvo_depthnet_sync(dfvo_depthnet* net);

/* =====================================================================================
 * monodepth2 two-frame pose net  (replaces Monodepth2PoseNet.inference / inference_pose,
 * pose/monodepth2/monodepth2.py:86-119, behind DeepModel.forward_pose, deep_models.py:208-230)
 * ResnetEncoder(18, False, 2) + PoseDecoder(num_ch_enc, 1, 2) + transformation_from_parameters(invert=True);
 * packed in the conv precision in force at dfvo_posenet_finalize, like the other nets.
 * ===================================================================================== */
typedef struct dfvo_posenet dfvo_posenet;
/* feed size: multiples of 32; baseline_mult multiplies the translation column (stereo_baseline_multiplier) */
int dfvo_posenet_create(int feed_h, int feed_w, float baseline_mult, void* stream, dfvo_posenet** out);
void dfvo_posenet_destroy(dfvo_posenet* net);
/* keys of pose_encoder.pth ("encoder.conv1.weight" [64,6,7,7], ...) and pose.pth ("net.0.weight", ... "net.3.bias") */
int dfvo_posenet_set_param(dfvo_posenet* net, const char* name, const float* h_data, int ndim, const int* shape);
int dfvo_posenet_finalize(dfvo_posenet* net);
int dfvo_posenet_set_graph(dfvo_posenet* net, int enable);
/* two device images uint8 [feed_h, feed_w, 3] (channel order of the net input: image 0's RGB, then image 1's) ->
 * d_pose16: row-major float 4x4, the relative pose from image 1 to image 0, translation x baseline_mult;
 * d_params6 (may be NULL): frame 0's raw axis-angle (3) and translation (3), before the multiplier.
 * Asynchronous on the net's stream (dfvo_posenet_sync). */
int dfvo_posenet_forward(dfvo_posenet* net, const uint8_t* d_img0, const uint8_t* d_img1, float* d_pose16, float* d_params6);
/* DeepModel.forward_pose in one blocking call: two host uint8 images [img_h,img_w,3] -> Pillow-exact LANCZOS resize of
 * each to the feed size on the device -> net -> host float[16] */
int dfvo_posenet_forward_images_host(dfvo_posenet* net, const uint8_t* h_img0, const uint8_t* h_img1, int img_h, int img_w,
                                     float* h_pose16);
double dfvo_posenet_last_flops(const dfvo_posenet* net);
int dfvo_posenet_sync(dfvo_posenet* net);
/* dfvo.py:314-319 + utils.py:89-114: nearest resize to (H,W), crop rows/cols, range mask.
 * d_depth float [h,w] -> d_raw float [H,W], d_proc double [H,W].  The resize is cv2.resize's INTER_NEAREST: source column
 * min(floor(x * (1.0 / ((double)W / w))), w - 1), rows alike.  d_raw holds the resized map bit for bit; d_proc is
 * (double)d_raw inside rows [y0, y1), columns [x0, x1) where min_depth < d_raw < max_depth (both strict, compared in
 * float), else 0.0.  One deliberate difference from the reference: a NaN or infinite depth fails the range test and
 * gives d_proc = 0.0 (d_raw passes its bits through), where utils.py's depth * mask gives NaN -- the solvers read
 * d_proc and treat 0 as "no depth".  h, w, H, W >= 1, else DFVO_ERR_ARG.  Asynchronous on `stream`. */
int dfvo_depth_postprocess(const float* d_depth, int h, int w, int H, int W, int y0, int y1, int x0, int x1,
                           float min_depth, float max_depth, float* d_raw, double* d_proc, void* stream);
/* depth.depth_src gt: read_depth behind the decoder (utils.py:55-73: cv2.imread(path, -1) / scale_factor, cv2.resize
 * INTER_NEAREST to the image size; scale_factor 500 in kitti.py, 5000 in tum.py / kinect.py) and preprocess_depth
 * (utils.py:89-114) in one launch.  d_src_u16 uint16 [src_h,src_w] (the decoded depth image; rows need no alignment beyond
 * 2 bytes) -> d_raw_f32 float [H,W], d_proc_f64 double [H,W].  Source pixel: the INTER_NEAREST index of
 * dfvo_depth_postprocess.  v = (double)u16 / scale, an IEEE float64 division; d_raw_f32 = (float)v; d_proc_f64 = v inside rows
 * [y0, y1), columns [x0, x1) where min_depth < v < max_depth (both strict, compared in float64, as the reference compares a
 * float64 array), else 0.0 -- a sensor hole (u16 == 0) gives 0.  DFVO_ERR_ARG, before anything is launched, for a null pointer,
 * a size below 1, a scale that is not finite or not > 0, or a crop that is not 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W.
 * Asynchronous on `stream`. */
int dfvo_read_depth_u16(const uint16_t* d_src_u16, int src_h, int src_w, double scale, int H, int W, int y0, int y1, int x0,
                        int x1, double min_depth, double max_depth, float* d_raw_f32, double* d_proc_f64, void* stream);
/* kp_selection.depth_consistency (DepthConsistency.warp_and_reproj_depth + compute_depth_diff, method depth_ratio,
 * libs/matching/depth_consistency.py:69-151) in one launch, float32 per pixel:
 *   P = K^-1 (x, y, 1) d_cur;  P' = T[:3, :] (P, 1);  reproj = P'_z;  pixel = (K P')_xy / ((K P')_z + 1e-7), normalised
 *   /(W - 1), /(H - 1), (. - 0.5) * 2;  warp = bilinear sample of d_ref at it, border padding, corners aligned (torch 1.1's
 *   grid_sample);  out = clamp(|warp - reproj| / reproj, 0, 1) -- a NaN stays a NaN, as torch.clamp leaves it.
 * d_cur_depth / d_ref_depth: the raw depths of the current and the reference frame, float [H,W]; h_K, h_Kinv: host float[9],
 * row-major; h_T: host float[16], row-major, the pose from the current to the reference frame (DeepModel.forward_pose).
 * d_cur_depth and d_out 16-byte aligned, H, W >= 2.  Asynchronous on `stream`; _host is the blocking host-array form. */
int dfvo_depth_consistency(const float* d_cur_depth, const float* d_ref_depth, int H, int W, const float* h_K, const float* h_Kinv,
                           const float* h_T, float* d_out, void* stream);
int dfvo_depth_consistency_host(const float* h_cur_depth, const float* h_ref_depth, int H, int W, const float* h_K,
                                const float* h_Kinv, const float* h_T, float* h_out);
/* dfvo_depth_consistency with the pose in device memory: d_T16 is a device float[16], row-major (4-byte aligned), as
 * dfvo_posenet_forward leaves it.  The kernel reads it in stream order -- it may be the output of work enqueued earlier on
 * `stream` -- and the host never does: no wait, no copy.  For the same 16 floats the map is bit-identical to
 * dfvo_depth_consistency's.  Asynchronous on `stream`. */
int dfvo_depth_consistency_dev(const float* d_cur_depth, const float* d_ref_depth, int H, int W, const float* h_K,
                               const float* h_Kinv, const float* d_T16, float* d_out, void* stream);

/* =====================================================================================
 * Pose solvers (wavefront-parallel RANSAC, f64).  Host arrays in / out, synchronous: these are the
 * calls the Python mirror classes make where the reference calls OpenCV.
 * ===================================================================================== */
typedef struct dfvo_tracker dfvo_tracker;
int dfvo_tracker_create(void* stream, dfvo_tracker** out);
void dfvo_tracker_destroy(dfvo_tracker* trk);
/* Device time [ms] of the stages of the LAST dfvo_compute_pose_2d2d / dfvo_find_scale_from_depth call on this tracker, under
 * the reference's Timer sub-keys (E_tracker.py:197-296,597-638; libs/general/timer.py), from HIP events between the
 * kernels of the chain.  h_ms8 = {find H, GRIC-H (incl. find H, nested as in the reference), find-Ess (shuffles + the
 * `repeat` five-point RANSACs, one batched launch sequence here), GRIC-E, find-Ess (full) (shuffles .. best-model
 * bookkeeping), recover pose, triangulation (+ depth ratios), scale ransac}; -1 for a stage the last call did not run. */
int dfvo_tracker_stage_ms(dfvo_tracker* trk, double* h_ms8);

/* cv2.findEssentialMat(points1, points2, focal, pp, RANSAC, prob, threshold)
 * (E_tracker.py:59-67,231-239).  h_pts [n][2] doubles.  h_E[9], h_mask[n] (0/1).
 * h_info[5] = {found, iterations replayed, winning iteration, winning model, inlier count}.
 * max_iters: 1000 reproduces OpenCV 3.4.3 (not a Python parameter there). */
int dfvo_find_essential_mat(dfvo_tracker* trk, const double* h_pts1, const double* h_pts2, int n, double focal,
                            double ppx, double ppy, double prob, double threshold, int max_iters, double* h_E,
                            uint8_t* h_mask, int* h_info);
/* cv2.findHomography(src, dst, RANSAC, ransacReprojThreshold, maxIters=2000, confidence)
 * (E_tracker.py:188-194,199-205) including the least-squares refit and the LM refinement. */
int dfvo_find_homography(dfvo_tracker* trk, const double* h_pts1, const double* h_pts2, int n, double thr,
                         int max_iters, double confidence, double* h_H, uint8_t* h_mask, int* h_info);
/* cv2.recoverPose(E, points1, points2, focal, pp) (E_tracker.py:73-75,251-253,292-295).
 * h_R[9], h_t[3], h_mask[n] (0/255), *h_good = cheirality count. */
int dfvo_recover_pose(dfvo_tracker* trk, const double* h_E, const double* h_pts1, const double* h_pts2, int n,
                      double focal, double ppx, double ppy, double* h_R, double* h_t, uint8_t* h_mask, int* h_good);
/* cv2.triangulatePoints(P1, P2, x1, x2) (ops_3d.py:63): P 3x4, x [2][n], X4 [4][n] */
int dfvo_triangulate_points(dfvo_tracker* trk, const double* h_P1, const double* h_P2, const double* h_x1,
                            const double* h_x2, int n, double* h_X4);

/* ---- the global numpy RandomState threaded through the device (np.random.shuffle at
 * E_tracker.py:225-228 / pnp_tracker.py:91-92; sklearn RANSACRegressor's random_state=None at
 * E_tracker.py:618-636).  State layout = np.random.get_state(): key[624] then pos, as uint32[625]. */
int dfvo_tracker_seed(dfvo_tracker* trk, uint32_t seed);                 /* np.random.seed(seed) */
int dfvo_tracker_set_rng_state(dfvo_tracker* trk, const uint32_t* h_state625);
int dfvo_tracker_get_rng_state(dfvo_tracker* trk, uint32_t* h_state625);

/* local_bestN keypoint selection (kp_selection.py:74-200 behind KeypointSampler.kp_selection,
 * keypoint_sampler.py:76-143), score_method "flow", depth consistency off.
 * h_flow float [2,H,W], h_diff float [H,W]; h_kp1/h_kp2 double [num_bestN][2] (x,y), *n_out rows valid;
 * *good_kp_found 0 when either "insufficient keypoint" rule fires.  The order of the keypoints is
 * numpy's scalar-introselect argpartition order, cell by cell. */
int dfvo_kp_local_bestn(dfvo_tracker* trk, const float* h_flow, const float* h_diff, int H, int W, int num_row,
                        int num_col, int num_bestN, float thre, double* h_kp1, double* h_kp2, int* n_out,
                        int* good_kp_found);
/* same with cfg.kp_selection.local_bestN.score_method (kp_selection.py:137-141,151-156): 'flow' thresholds and ranks the
 * consistency map itself (what dfvo_kp_local_bestn does), 'flow_ratio' the map divided by the flow magnitude per pixel
 * (float32, numpy's evaluation order); the "enough good pixels" rule stays on the map itself (kp_selection.py:121) */
#define DFVO_KP_SCORE_FLOW 0
#define DFVO_KP_SCORE_FLOW_RATIO 1
int dfvo_kp_local_bestn_ex(dfvo_tracker* trk, const float* h_flow, const float* h_diff, int H, int W, int num_row,
                           int num_col, int num_bestN, float thre, int score_method, double* h_kp1, double* h_kp2,
                           int* n_out, int* good_kp_found);
/* same with kp_selection.depth_consistency.enable (kp_selection.py:118-119,145-148): h_depth_diff float [H,W] is
 * ref_data['depth_diff'] (dfvo_depth_consistency); a cell's candidates are the pixels with score < thre AND depth_diff <
 * depth_thre (a NaN in either map fails its comparison).  The ranking key is the score alone, the "enough good pixels" rule
 * stays on h_diff alone, the order is numpy's over the masked candidates. */
int dfvo_kp_local_bestn_depth(dfvo_tracker* trk, const float* h_flow, const float* h_diff, const float* h_depth_diff, int H,
                              int W, int num_row, int num_col, int num_bestN, float thre, float depth_thre, int score_method,
                              double* h_kp1, double* h_kp2, int* n_out, int* good_kp_found);
/* bestN_flow_kp (kp_selection.py:33-71, ablation_correspondences_best_n.yml): the num_bestN pixels of the whole image
 * with the least forward-backward inconsistency, in np.argpartition(flow_diff[flow_diff >= 0], num_bestN)[:num_bestN]
 * order (numpy's scalar introselect).  *n_out = num_bestN, or 0 when the image has no more than num_bestN candidates
 * (numpy raises there). */
int dfvo_kp_bestn(dfvo_tracker* trk, const float* h_flow, const float* h_diff, int H, int W, int num_bestN,
                  double* h_kp1, double* h_kp2, int* n_out);
/* sampled_kp (kp_selection.py:327-378, the "uniform" correspondences of ablation_correspondences_uniform.yml): for each
 * index k of h_idx[n] (KeypointSampler.generate_kp_samples' linspace over the cropped grid [y0:y1, x0:x1], row-major)
 * kp1 = (x, y) of that pixel and kp2 = kp1 + flow there; h_kp1 / h_kp2 [n,2] */
int dfvo_kp_sampled(dfvo_tracker* trk, const float* h_flow, int H, int W, int y0, int y1, int x0, int x1,
                    const int* h_idx, int n, double* h_kp1, double* h_kp2);

/* EssTracker.kp_selection_good_depth (E_tracker.py:645-705): RigidFlow layer of the reference
 * depth under the ref -> cur motion (geometry/{rigid_flow,reprojection,backprojection,transformation3d,projection}.py,
 * float32), its per-pixel distance to the optical flow, then opt_rigid_flow_kp (kp_selection.py:203-324): per grid
 * cell the pixels with rigid distance < rigid_flow_thre and forward-backward distance < optical_flow_thre; "best" =
 * argpartition by the score, "uniform" = every step-th candidate.  h_raw_depth float [H,W] (the unprocessed CNN depth of
 * the reference frame), h_flow float [2,H,W], h_flow_diff float [H,W].  Outputs [num_bestN,2] doubles each, *n_out rows
 * valid (same count for both sets); h_rigid_flow_diff (optional, float [H,W]) receives the distance map ("rigid_flow_mask");
 * h_rigid_diff_override (optional) is used instead of the computed map. */
typedef struct dfvo_rigid_kp_cfg {
    int num_row, num_col, num_bestN;       /* kp_selection.rigid_flow_kp.{num_row,num_col,num_bestN} */
    double rigid_flow_thre, optical_flow_thre;
    int score_method;                      /* 0 "opt_flow", 1 "rigid_flow" */
    double K[9], Kinv[9];                  /* intrinsics and np.linalg.inv of them (cast to float32 like .float()) */
    double T_ref_to_cur[16];               /* ref_data['rigid_flow_pose'].pose */
} dfvo_rigid_kp_cfg;
int dfvo_kp_rigid_flow(dfvo_tracker* trk, const float* h_flow, const float* h_flow_diff, const float* h_raw_depth, int H,
                       int W, const dfvo_rigid_kp_cfg* cfg, const float* h_rigid_diff_override, double* h_kp1_best,
                       double* h_kp2_best, double* h_kp1_uniform, double* h_kp2_uniform, int* n_out,
                       float* h_rigid_flow_diff);

/* EssTracker.compute_pose_2d2d (E_tracker.py:154-307).  validity_method DFVO_VALIDITY_GRIC (default configuration):
 * homography + GRIC-H, `repeat` x (shuffle, findEssentialMat, GRIC-E), best-of by inlier count, recoverPose,
 * cheirality > 10 %.  DFVO_VALIDITY_FLOW (ablation_model_sel_flow.yml): the pair is tracked only when the mean keypoint
 * displacement exceeds validity_thre (else identity and no RandomState draw); a repeat is valid when the cheirality
 * count of recoverPose(E_rep) exceeds 10 % of the keypoints, and it can only become the best model above 5 %
 * (out: h_gric = the mean displacement, rep_gric[] = the per-repeat cheirality counts).
 * DFVO_VALIDITY_HOMO_RATIO (E_tracker.py:186-194,243-250): findHomography with ransacReprojThreshold 0.2; a repeat is
 * valid while H_inliers.sum() / (H_inliers.sum() + inliers.sum()) < validity_thre (out: h_gric = the homography's
 * inlier count, rep_gric[] = the ratios; fewer than 5 keypoints, where the reference raises: identity).
 * Consumes the tracker's RandomState for the shuffles.
 * Where the reference raises inside the call, the answer is: R = identity, t = 0, major_valid = 0, every rep_valid[] = 0,
 * cheirality = 0, h_inliers all ones, and the RandomState advanced by exactly the shuffles the reference drew before it
 * raised.  That is (a) GRIC validity with more than 10 keypoints and no homography found (h_found = 0;
 * homography_residual(None) raises before the repeat loop): no shuffle; (b) any validity method, findEssentialMat
 * returning None in repeat r (`inv(K.T) @ None`, `None.sum()`, recoverPose(None); e.g. two views equal bit for bit):
 * r + 1 shuffles.  rep_inliers[] / rep_gric[] still report what the device computed for every repeat.
 * findEssentialMat with exactly 5 points is OpenCV's single kernel run: first model, all five points inliers. */
#define DFVO_VALIDITY_GRIC 0
#define DFVO_VALIDITY_FLOW 1
#define DFVO_VALIDITY_HOMO_RATIO 2
typedef struct dfvo_pose2d2d_cfg {
    double fx, cx, cy;       /* focal = fx, principal point (E_tracker.py:231-239) */
    double reproj_thre;      /* e_tracker.ransac.reproj_thre */
    int repeat;              /* e_tracker.ransac.repeat (or 3) */
    int max_iters;           /* 1000 = OpenCV 3.4.3 */
    double KinvT[9];         /* np.linalg.inv(K.T) */
    double Kinv[9];          /* np.linalg.inv(K)   */
    int validity_method;     /* e_tracker.validity.method: DFVO_VALIDITY_GRIC / _FLOW / _HOMO_RATIO */
    double validity_thre;    /* e_tracker.validity.thre (flow, homo_ratio) */
} dfvo_pose2d2d_cfg;
typedef struct dfvo_pose2d2d_out {
    double R[9], t[3];       /* pose cur -> ref (identity / zero when rejected) */
    int n, best_inlier_cnt, num_valid, major_valid, cheirality, h_found;
    double h_gric;
    int rep_inliers[8], rep_valid[8];
    double rep_gric[8];
} dfvo_pose2d2d_out;
int dfvo_compute_pose_2d2d(dfvo_tracker* trk, const double* h_kp_ref, const double* h_kp_cur, int n,
                           const dfvo_pose2d2d_cfg* cfg, dfvo_pose2d2d_out* out, uint8_t* h_inliers);

/* EssTracker.find_scale_from_depth (E_tracker.py:571-643): triangulate (ops_3d.py:44-67), scatter to a
 * sparse depth map (ops_3d.py:15-41), depth ratios on valid pixels, sklearn RANSACRegressor on them.
 * h_T21 4x4; h_depth double [H,W].  *scale = -1 when fewer than 11 valid ratios.
 * method DFVO_SCALE_DEPTH_RATIO: .fit(depth_ratio, ones); DFVO_SCALE_ABS_DIFF: .fit(depth_tri, depth_pred)
 * (scale_recovery.ransac.method, E_tracker.py:626-635).
 * h_info[4] = {n_valid, n_trials, n_inliers, status}.  Consumes the tracker's RandomState. */
#define DFVO_SCALE_DEPTH_RATIO 0
#define DFVO_SCALE_ABS_DIFF 1
typedef struct dfvo_scale_cfg {
    double cx, cy, fx, fy;
    int min_samples, max_trials;
    double stop_prob, thre;
    int method;              /* DFVO_SCALE_DEPTH_RATIO / DFVO_SCALE_ABS_DIFF */
} dfvo_scale_cfg;
int dfvo_find_scale_from_depth(dfvo_tracker* trk, const double* h_kp1, const double* h_kp2, int n,
                               const double* h_T21, const double* h_depth, int H, int W, const dfvo_scale_cfg* cfg,
                               double* scale, int* h_info);
/* The same call without the H x W upload (3.7 MB of float64 at KITTI size, from pageable memory, per pair): the reference reads
 * depth2 only under the sparse triangulated map, i.e. at the pixels (int(kp2.x), int(kp2.y)) (E_tracker.py:604-612,
 * ops_3d.py:29-40).  h_depth_at_kp2 [n] = depth2[int(kp2[i].y), int(kp2[i].x)] (truncation toward zero; any value where that
 * pixel is outside the H x W map or the coordinate is not finite -- such keypoints are dropped before the value is read).
 * h_rng625 (optional, in / out): numpy RandomState words to run under, replaced by the advanced state -- saves the two
 * blocking dfvo_tracker_{set,get}_rng_state round trips of the mirror.  Same result as dfvo_find_scale_from_depth, bit for bit. */
int dfvo_find_scale_from_depth_at_kp(dfvo_tracker* trk, const double* h_kp1, const double* h_kp2, int n, const double* h_T21,
                                     const double* h_depth_at_kp2, int H, int W, const dfvo_scale_cfg* cfg,
                                     uint32_t* h_rng625, double* scale, int* h_info);
/* The regression stage on its own -- sklearn.linear_model.RANSACRegressor(LinearRegression(fit_intercept=False),
 * min_samples, max_trials, stop_probability, residual_threshold).fit(x[:, None], y) as E_tracker.py:618-636 builds it --
 * on raw host arrays: h_x [n], h_y [n] or NULL for y = 1 (the depth-ratio case).  Consumes the tracker's RandomState as
 * sklearn consumes np.random.  coef: estimator_.coef_[0, 0]; h_info as above (status -1: "RANSAC could not find a valid
 * consensus set", where sklearn raises ValueError).  cfg->cx .. fy and method are not read. */
int dfvo_ransac_regressor(dfvo_tracker* trk, const double* h_x, const double* h_y, int n, const dfvo_scale_cfg* cfg,
                          double* coef, int* h_info);

/* EssTracker.scale_recovery_iterative (E_tracker.py:509-569; scale_recovery.method "iterative", ablation_scale_iterative.yml and
 * the tracking half of the *_extend.yml configurations): up to five rounds of [rigid_flow_pose = inv([R | t * scale]),
 * kp_selection_good_depth under it (dfvo_kp_rigid_flow, uniform set), find_scale_from_depth], until the scale moves by less
 * than 0.001.  All five rounds are enqueued at once; a device record carries the scale from round to round and makes the
 * rounds behind the last one return at once, so the host neither waits nor copies between rounds, and a round that does not
 * run draws nothing from the RandomState.
 * Inputs, uploaded once: h_flow float [2,H,W], h_flow_diff float [H,W], h_raw_depth_ref float [H,W] (ref_data['raw_depth']),
 * h_depth_cur double [H,W] (cur_data['depth']).  cfg: as for dfvo_kp_rigid_flow, T_ref_to_cur is not read.  h_E_pose: 4x4,
 * cur -> ref with unit translation; h_T21 (optional): its inverse as find_scale_from_depth receives it (NULL: the closed form
 * [R^T | -R^T t]).  kp_src DFVO_ITER_KP_DEPTH: each round's scale comes from that round's uniform keypoints;
 * DFVO_ITER_KP_BEST: from the fixed set h_kp_best_ref / h_kp_best_cur [n_kp_best,2] (the other two are then ignored).
 * h_rng625 (in / out): numpy RandomState words to run under, replaced by the advanced state.
 * out: the scale, the rounds completed and the per-round records; h_kp_ref / h_kp_cur [num_bestN,2]: the uniform keypoints
 * of the last round that ran (out->n_kp rows); h_rigid_flow_diff (optional, float [H,W]): that round's distance map.
 * Returns DFVO_ERR_EMPTY_SELECTION where the reference's "sampling threshold is too small." assertion fires and
 * DFVO_ERR_NO_CONSENSUS where sklearn raises; the outputs then hold what the reference had written when it raised (the
 * previous round's keypoints and map for the former, this round's for the latter; out->n_iter rounds completed), and
 * nothing at all is written when the first round selects nothing.  The tracker stays usable after either. */
#define DFVO_ITER_KP_DEPTH 0
#define DFVO_ITER_KP_BEST 1
typedef struct dfvo_scale_iter_out {
    double scale;            /* scale of the last completed round (prev_scale when none completed) */
    int n_iter;              /* rounds completed, 0 .. 5 */
    int n_kp;                /* rows of h_kp_ref / h_kp_cur */
    int kp_round;            /* the round those keypoints and the distance map belong to (-1: none) */
    int status;              /* 0 finished, 1 empty selection, 2 no consensus set */
    double scale_in[5];      /* scale each round's rigid_flow_pose was built with */
    double scale_out[5];     /* scale each round found (-1: fewer than 11 valid depth ratios) */
    int n_kp_round[5];       /* uniform keypoints of each round (-1: the round did not run) */
    float device_ms;         /* device time of the five enqueued rounds (HIP events around them, uploads and results outside) */
} dfvo_scale_iter_out;
int dfvo_scale_recovery_iterative(dfvo_tracker* trk, const float* h_flow, const float* h_flow_diff, const float* h_raw_depth_ref,
                                  const double* h_depth_cur, int H, int W, const dfvo_rigid_kp_cfg* cfg,
                                  const dfvo_scale_cfg* scfg, const double* h_E_pose, const double* h_T21, double prev_scale,
                                  int kp_src, const double* h_kp_best_ref, const double* h_kp_best_cur, int n_kp_best,
                                  uint32_t* h_rng625, dfvo_scale_iter_out* out, double* h_kp_ref, double* h_kp_cur,
                                  float* h_rigid_flow_diff);

/* PnpTracker.compute_pose_3d2d (pnp_tracker.py:45-125): masks (kp2 inside the image, depth_1[int(kp1)] != 0 and
 * in (min_depth, max_depth)), unprojection_kp (ops_3d.py:70-94), `repeat` x [np.random.shuffle +
 * cv2.solvePnPRansac(iterationsCount = iters, reprojectionError = reproj_thre)], best by inlier count,
 * cv2.Rodrigues.  h_kp1 / h_kp2 [n][2] doubles, h_depth double [H,W] (depth of view 1).
 * out->R / tvec: the solvePnP pose (view-1 points -> view-2 camera); the caller inverts it like the reference
 * does (pose.pose = pose.inv_pose).  h_keep[n] (optional): 1 where the keypoint survived the masks.
 * Consumes the tracker's RandomState (one shuffle per repeat, drawn even when too few points remain).
 * Coplanar object points take cvFindExtrinsicCameraParams2's planar (homography) initialisation, as OpenCV does. */
typedef struct dfvo_pose3d2d_cfg {
    double fx, fy, cx, cy;
    double Kinv[9];                 /* Intrinsics.inv_mat, row-major */
    double min_depth, max_depth;    /* cfg.depth.{min,max}_depth */
    int repeat;                     /* cfg.pnp_tracker.ransac.repeat if is_iterative else 3 */
    int iters;                      /* cfg.pnp_tracker.ransac.iter */
    double reproj_thre;             /* cfg.pnp_tracker.ransac.reproj_thre */
} dfvo_pose3d2d_cfg;
typedef struct dfvo_pose3d2d_out {
    int found, best_inliers, n_filtered, status;
    double rvec[3], tvec[3], R[9];
} dfvo_pose3d2d_out;
int dfvo_compute_pose_3d2d(dfvo_tracker* trk, const double* h_kp1, const double* h_kp2, int n, const double* h_depth,
                           int H, int W, const dfvo_pose3d2d_cfg* cfg, dfvo_pose3d2d_out* out, uint8_t* h_keep);
/* The same call without the H x W upload: the reference reads depth_1 only at kp1's pixels (pnp_tracker.py:71-77:
 * depth_1[kp1[:, 1].astype(int), kp1[:, 0].astype(int)], truncation toward zero, negative indices wrapping as numpy's do).
 * h_depth_at_kp1 [n] = that value per keypoint (any value where the wrapped index is still outside the map: the keypoint is
 * dropped before the value is read).  h_rng625 (optional, in / out) as in dfvo_find_scale_from_depth_at_kp.  Same result as
 * dfvo_compute_pose_3d2d, bit for bit. */
int dfvo_compute_pose_3d2d_at_kp(dfvo_tracker* trk, const double* h_kp1, const double* h_kp2, int n, const double* h_depth_at_kp1,
                                 int H, int W, const dfvo_pose3d2d_cfg* cfg, uint32_t* h_rng625, dfvo_pose3d2d_out* out,
                                 uint8_t* h_keep);

/* =====================================================================================
 * Fused per-pair pipeline: images in HBM -> relative pose, everything between on the device
 * (libs/dfvo.py:299-345 deep_model_inference + :121-262 tracking, hybrid E-tracker path).
 * DFVO_PIPELINE_SLOTS slots buffer the net outputs so that the nets of the following pairs run under the solvers of pair k.
 * ===================================================================================== */
typedef struct dfvo_pipeline dfvo_pipeline;
typedef struct dfvo_pipeline_cfg {
    int img_h, img_w, feed_h, feed_w;
    float net_min_depth, net_max_depth, baseline_mult;   /* monodepth2.py:74-89 */
    double min_depth, max_depth;                         /* cfg.depth.{min,max}_depth (utils.py:89-114) */
    double depth_crop[4];                                /* y0 y1 x0 x1 fractions (cfg.crop.depth_crop) */
    double fx, fy, cx, cy;
    double KinvT[9], Kinv[9];
    int kp_num_row, kp_num_col, kp_num_bestN;
    double kp_thre;
    double e_reproj_thre;
    int e_repeat, e_max_iters;
    int scale_min_samples, scale_max_trials;
    double scale_stop_prob, scale_thre;
    uint32_t seed;                                       /* np.random.seed(cfg.seed), run.py:81-84 */
    int pnp_repeat, pnp_iters;                           /* cfg.pnp_tracker.ransac.{repeat,iter} */
    double pnp_reproj_thre;                              /* cfg.pnp_tracker.ransac.reproj_thre */
} dfvo_pipeline_cfg;
#define DFVO_TRACK_E 0                 /* pose from the essential matrix + depth scale */
#define DFVO_TRACK_CONSTANT_MOTION 1   /* not enough keypoints: caller reuses the previous motion (dfvo.py:157-161) */
#define DFVO_TRACK_NEEDS_PNP 2         /* E rejected or scale == -1 and no reference depth is known yet (first pair) */
#define DFVO_TRACK_PNP 3               /* E rejected or scale == -1: pose from the PnP fallback (dfvo.py:225-250) */
#define DFVO_TRACK_DEEP_POSE 4         /* tracking_method deep_pose: the pose net's matrix (dfvo.py:252-255) */
typedef struct dfvo_track_out {
    double R[9], t[3];        /* DFVO_TRACK_E: E-tracker pose cur -> ref (t has unit norm or is zero);
                                 DFVO_TRACK_PNP: the solvePnP pose (ref points -> cur camera; identity when no repeat
                                 found a model), which the caller inverts as pnp_tracker.py:118 does;
                                 DFVO_TRACK_DEEP_POSE: the pose net's float32 [R|t], cur -> ref, converted exactly; scale 1 */
    double scale;
    int status, n_kp, good_kp_found, best_inlier_cnt, num_valid, cheirality;
    int scale_n_valid, scale_n_trials, scale_n_inliers;
    int pnp_found, pnp_inliers, pnp_n_filtered;
} dfvo_track_out;
/* Stream placement (dfvo_pipeline_create and dfvo_session_create; df-vo_amd/csrc/stream_pool.hip).  Both objects drive several
 * HIP streams whose hardware queues should sit on different dispatch pipes of the command processor (two busy streams on one
 * pipe slow each other's launches 2.5 x).  Which pipe a stream lands on follows the PROCESS's stream creation order, so the
 * objects create twelve candidates and classify them by a ~10 ms timing probe.  The probe is a measurement:
 *   - a classification is accepted when it has the shape of a process whose queues are all its own (four groups of three)
 *     or when two passes agree stream for stream; a positive ("these two share a pipe") has to show twice in a row;
 *   - when no pass is accepted, or a measurement fails, ONE line goes to stderr and every role keeps a stream in the
 *     runtime's creation order (slower by up to a third, never wrong);
 *   - environment: DFVO_STREAM_POOL=creation skips the probe; DFVO_STREAM_PROBE_VERBOSE=1 prints every pass;
 *     DFVO_STREAM_POOL_FORCE_FAIL=1 (test hook) makes every measurement fail. */
int dfvo_pipeline_create(const dfvo_pipeline_cfg* cfg, dfvo_pipeline** out);
void dfvo_pipeline_destroy(dfvo_pipeline* p);
int dfvo_pipeline_set_flow_param(dfvo_pipeline* p, const char* name, const float* h_data, int ndim, const int* shape);
int dfvo_pipeline_set_depth_param(dfvo_pipeline* p, const char* name, const float* h_data, int ndim, const int* shape);
int dfvo_pipeline_finalize(dfvo_pipeline* p);
int dfvo_pipeline_seed(dfvo_pipeline* p, uint32_t seed);
/* The tracking configurations beyond default_configuration.yml (ablation_correspondences_best_n.yml, _uniform.yml,
 * ablation_model_sel_flow.yml, ablation_tracker_pnp.yml and the unshipped branches flow_ratio / homo_ratio / abs_diff).
 * All zero = the default configuration; a pipeline on which dfvo_pipeline_set_options is never called runs exactly that.
 * Legal after dfvo_pipeline_create and before the first dfvo_pipeline_enqueue_nets / _set_ref_depth / _set_ref_image; it
 * allocates every buffer the chosen keypoint source needs.  kp_source:
 *   LOCAL_BESTN  kp_selection.py:74-200, the grid of dfvo_pipeline_cfg (kp_num_row x kp_num_col, kp_num_bestN, kp_thre)
 *   BESTN        kp_selection.py:33-71: the kp_num_bestN most consistent pixels of the whole image, in np.argpartition's
 *                order.  An image with kp_num_bestN or fewer non-NaN pixels (numpy raises there) reports no good keypoints.
 *   SAMPLED      kp_selection.py:327-378 at the kp_sampled_num indices of keypoint_sampler.py:52-74 over flow_crop
 * good_kp_found is always 1 for BESTN / SAMPLED (keypoint_sampler.py:96).
 * tracking_method PNP (dfvo.py:165,225: no E-tracker, PnP on every pair): dfvo_pipeline_track_begin enqueues the keypoint
 * stage and the PnP chain, dfvo_pipeline_track_end only waits for it; status DFVO_TRACK_PNP, or DFVO_TRACK_NEEDS_PNP while
 * no reference depth is known; the inlier mask of dfvo_pipeline_get_keypoints is all ones. */
#define DFVO_KP_SOURCE_LOCAL_BESTN 0
#define DFVO_KP_SOURCE_BESTN 1
#define DFVO_KP_SOURCE_SAMPLED 2
#define DFVO_SCALE_DEPTH_RATIO 0
#define DFVO_SCALE_ABS_DIFF 1
#define DFVO_TRACKING_HYBRID 0
#define DFVO_TRACKING_PNP 1
#define DFVO_TRACKING_DEEP_POSE 2  /* needs dfvo_pipeline_set_pose_net (enable) first */
typedef struct dfvo_pipeline_opts {
    int kp_source;        /* DFVO_KP_SOURCE_* */
    int kp_score_method;  /* local_bestN only: DFVO_KP_SCORE_FLOW | DFVO_KP_SCORE_FLOW_RATIO */
    int kp_sampled_num;   /* sampled: cfg.kp_selection.sampled_kp.num_kp */
    double flow_crop[4];  /* sampled: y0 y1 x0 x1 fractions (cfg.crop.flow_crop) */
    int validity_method;  /* DFVO_VALIDITY_GRIC | _FLOW | _HOMO_RATIO */
    double validity_thre; /* e_tracker.validity.thre (unused under GRIC) */
    int scale_method;     /* DFVO_SCALE_DEPTH_RATIO | DFVO_SCALE_ABS_DIFF (scale_recovery.ransac.method) */
    int tracking_method;  /* DFVO_TRACKING_HYBRID | DFVO_TRACKING_PNP | DFVO_TRACKING_DEEP_POSE */
} dfvo_pipeline_opts;
int dfvo_pipeline_set_options(dfvo_pipeline* p, const dfvo_pipeline_opts* opts);
int dfvo_pipeline_set_graph(dfvo_pipeline* p, int enable);   /* hipGraph replay of the nets (default on) */
/* monodepth2's two-frame pose net in the fused pipeline (deep_pose.enable; DeepModel.forward_pose, deep_models.py:217-230) and
 * its two consumers: kp_selection.depth_consistency (the depth-difference map masks local_bestN's candidates,
 * kp_selection.py:118-148) and tracking_method deep_pose (dfvo.py:252-255).  A pipeline on which dfvo_pipeline_set_pose_net is
 * never called enqueues, allocates and waits for exactly what it did without it.
 * The pose lane runs on the depth stream inside dfvo_pipeline_enqueue_nets / _enqueue_nets_depth, in stream order: the current
 * frame's LANCZOS feed image (the depth net's, or made for the pose net alone), the reference frame's (d_ref resized, or with
 * d_ref == NULL the previous call's current feed), the net, and with depth_consistency the map of dfvo_depth_consistency_dev
 * over the slot's raw depth, the reference frame's raw depth and the pose, all in device memory.  The reference raw depth is
 * the raw depth of the slot the previous dfvo_pipeline_enqueue_nets* call filled, or what dfvo_pipeline_set_ref_image /
 * _set_ref_depth (d_feed) / _set_ref_depth_u16 / _set_ref_raw_depth left if one of them came since; a pair with neither is
 * refused.  The keypoint stage waits for the lane on the device; the host never waits for the net after the first pair (which
 * tunes and captures it).  baseline_mult is dfvo_pipeline_cfg's.
 * dfvo_pipeline_set_pose_param: the keys of dfvo_posenet_set_param; before dfvo_pipeline_finalize (with the net enabled after
 * dfvo_pipeline_finalize, before that dfvo_pipeline_set_pose_net call).
 * dfvo_pipeline_set_pose_net: state rule of dfvo_pipeline_set_options, and ahead of it where both are called: DFVO_ERR_ARG once a
 * pair or a reference depth was enqueued, for depth_consistency without enable, with a keypoint source other than
 * DFVO_KP_SOURCE_LOCAL_BESTN (the only one the reference masks) or with a NaN threshold.  tracking_method
 * DFVO_TRACKING_DEEP_POSE needs enable, and excludes depth_consistency (nothing selects keypoints).
 * Under DFVO_TRACKING_DEEP_POSE neither the depth net nor the flow net runs (dfvo.py:302): dfvo_pipeline_enqueue_nets* enqueue
 * the pose lane only, dfvo_pipeline_prefetch_track is accepted and does nothing, dfvo_pipeline_track_end reports status
 * DFVO_TRACK_DEEP_POSE, scale 1, n_kp 0, draws nothing from the RandomState and rolls no depth; dfvo_pipeline_get_flow and
 * dfvo_pipeline_get_keypoints return DFVO_ERR_ARG.
 * dfvo_pipeline_set_pose_override: a device float[16] the pair enqueued into `slot` uses in the place of the net's matrix; set
 * before the slot's dfvo_pipeline_enqueue_nets*, complete then and unchanged until the slot's dfvo_pipeline_track_end, which
 * withdraws it (as NULL does).
 * dfvo_pipeline_get_pose_net: what the slot's last pair used -- the 4x4 and (depth_consistency; else h_depth_diff must be NULL)
 * the float [H,W] depth-difference map.  Waits for the device. */
typedef struct dfvo_pipeline_pose_opts {
    int enable;             /* deep_pose.enable */
    int depth_consistency;  /* kp_selection.depth_consistency.enable */
    float depth_thre;       /* kp_selection.depth_consistency.thre */
} dfvo_pipeline_pose_opts;
int dfvo_pipeline_set_pose_param(dfvo_pipeline* p, const char* name, const float* h_data, int ndim, const int* shape);
int dfvo_pipeline_set_pose_net(dfvo_pipeline* p, const dfvo_pipeline_pose_opts* opts);
int dfvo_pipeline_set_pose_override(dfvo_pipeline* p, int slot, const float* d_pose16);
int dfvo_pipeline_get_pose_net(dfvo_pipeline* p, int slot, float* h_pose16, float* h_depth_diff);
/* scale_recovery.method "iterative" in the fused pipeline (ablation_scale_iterative.yml, the tracking half of the *_extend.yml
 * files): EssTracker.scale_recovery_iterative (see dfvo_scale_recovery_iterative) takes the place of find_scale_from_depth in
 * the chain dfvo_pipeline_track_begin enqueues.  The loop starts and ends on the device: its first kernel reads the E-tracker's
 * pose (a zero translation ends the call there, dfvo.py:182: status 3 "not run", no RandomState draw, nothing written) and
 * EssTracker.prev_scale, which the pipeline carries on the device from pair to pair (0 after dfvo_pipeline_create; written
 * once per completed round, the scale -1 included; a pair that completes no round leaves it as it was).  The flow, the
 * consistency map and the current frame's processed depth are the ones the pair tracks with; ref_data['raw_depth'] is the
 * raw depth of the reference frame, which dfvo_pipeline_set_ref_depth (d_feed) / _set_ref_image / _set_ref_raw_depth supply
 * for the first pair and every pair's roll-over supplies for the next.
 * kp_src DFVO_ITER_KP_DEPTH: each round's scale comes from that round's uniform rigid-flow keypoints; DFVO_ITER_KP_BEST: from the
 * pipeline's tracked keypoints, whichever kp_source produced them (at most 16384).  num_row / num_col / num_bestN /
 * rigid_flow_thre / optical_flow_thre: kp_selection.rigid_flow_kp.  There is no score_method: the loop reads only the uniform
 * set (E_tracker.py:541-542), which does not depend on the score (kp_selection.py:203-324).
 * Same state rule as dfvo_pipeline_set_options (call that one first when both are used): before the first
 * dfvo_pipeline_enqueue_nets / _set_ref_*.  DFVO_ERR_ARG, with a message, for what the rigid-flow keypoint launcher refuses at
 * the pipeline's img_h x img_w (grid, num_bestN per cell, cell size) and for more than 16384 keypoints in the scale stage.
 * Allocates every buffer of the loop; enable = 0 switches the method off again.  Nothing changes for a pipeline on which this
 * is never called: it enqueues exactly what it enqueued before.
 * dfvo_pipeline_track_end: where the reference raises (the "sampling threshold is too small." assertion, sklearn's "could not
 * find a valid consensus set") it returns DFVO_ERR_EMPTY_SELECTION / DFVO_ERR_NO_CONSENSUS -- after the pair is over: the slot
 * is idle, the depths are rolled over, the pipeline stays usable; prev_scale and the RandomState hold what the reference had at
 * the raise, `out` the E-tracker's pose (status DFVO_TRACK_E, scale of the last completed round or 0).  A scale of -1 takes the
 * PnP fallback as before. */
typedef struct dfvo_pipeline_iter_opts {
    int enable;               /* 1: scale_recovery.method iterative */
    int kp_src;               /* DFVO_ITER_KP_DEPTH | DFVO_ITER_KP_BEST (scale_recovery.kp_src) */
    int num_row, num_col;     /* kp_selection.rigid_flow_kp.num_row / num_col */
    int num_bestN;            /* kp_selection.rigid_flow_kp.num_bestN */
    double rigid_flow_thre;   /* kp_selection.rigid_flow_kp.rigid_flow_thre */
    double optical_flow_thre; /* kp_selection.rigid_flow_kp.optical_flow_thre */
} dfvo_pipeline_iter_opts;
int dfvo_pipeline_set_iterative(dfvo_pipeline* p, const dfvo_pipeline_iter_opts* opts);
/* The trackers' iterative keypoint refinement in the fused pipeline (the iterative_kp blocks of e_tracker, scale_recovery and
 * pnp_tracker, dfvo.py:194-222 and :236-244, under scale_recovery.method simple): a tracker runs once on the pipeline's tracked
 * keypoints with 3 shuffled RANSACs (compute_pose_2d2d / compute_pose_3d2d with is_iterative False), the rigid-flow keypoints
 * "kp_depth" are selected where the forward flow agrees with the rigid flow of the reference frame's raw depth under the pose
 * just found (kp_selection_good_depth, E_tracker.py:645-705: the best set, scored by e_score_rigid / pnp_score_rigid), and the
 * tracker runs again on them with the configured `repeat`.
 *   e_enable      second E pass when pass one has a translation; the rigid-flow pose is inv([R | t * scale]), inv([R | 0]) when
 *                 the scale is -1.  R, t and the inlier mask become the second pass's; a second pass without translation takes
 *                 the PnP fallback.
 *   scale_enable  (needs e_enable) find_scale_from_depth again on kp_depth when the second pass has a translation; a scale
 *                 other than -1 replaces pass one's, -1 takes the PnP fallback.
 *   pnp_enable    inside the PnP branch (the hybrid fallback and tracking_method PNP): PnP on the tracked keypoints with 3
 *                 repeats, kp_depth under that pose (the identity when no repeat found a model), PnP on kp_depth.
 * RandomState draws of a pair, in order: shuffles of E pass one, scale RANSAC one, shuffles of E pass two, scale RANSAC two,
 * shuffles of PnP one, shuffles of PnP two; a stage that does not run draws nothing.
 * The hand-over between the passes stays on the device (a one-lane kernel builds the rigid-flow pose from the device results
 * and reads its gate there); the host reads the kp_depth count from pinned memory, because the second pass's launch geometry
 * and its "more than 10 keypoints" rule need it.  dfvo_pipeline_track_begin enqueues pass one and the E selection behind it,
 * dfvo_pipeline_track_end the second passes: a pair refined by the E-tracker has three host waits (keypoint count, pass one
 * with the kp_depth count, pass two), one more for each PnP pass of the fallback.
 * State rule of dfvo_pipeline_set_options (call that one first when both are used).  DFVO_ERR_ARG, with a message: all three
 * enables zero together with a non-zero score; scale_enable without e_enable; dfvo_pipeline_set_iterative's method or
 * tracking_method DFVO_TRACKING_DEEP_POSE beside it; e_enable under DFVO_TRACKING_PNP (no E-tracker runs); what the rigid-flow
 * keypoint launcher refuses at img_h x img_w; more than 16384 kp_depth keypoints with scale_enable.  An all-zero block switches
 * the refinement off.  Allocates every buffer of the second passes; a pipeline on which this is never called enqueues,
 * allocates and waits for exactly what it did before.
 * An empty selection (the reference's "sampling threshold is too small." assertion) makes dfvo_pipeline_track_end return
 * DFVO_ERR_EMPTY_SELECTION after the pair is over, as under dfvo_pipeline_set_iterative: the slot idle, the depths rolled
 * over, the RandomState what the reference had at the raise, `out` the pose of the pass before the selection.
 * dfvo_track_out keeps its meaning: the final R, t, scale and the last pass's counts.  dfvo_pipeline_get_keypoints keeps
 * returning the tracked set with pass one's inlier mask. */
#define DFVO_REFINE_SCORE_OPT_FLOW 0
#define DFVO_REFINE_SCORE_RIGID_FLOW 1
typedef struct dfvo_pipeline_refine_opts {
    int e_enable;             /* e_tracker.iterative_kp.enable */
    int scale_enable;         /* scale_recovery.iterative_kp.enable */
    int pnp_enable;           /* pnp_tracker.iterative_kp.enable */
    int e_score_rigid;        /* e_tracker.iterative_kp.score_method: DFVO_REFINE_SCORE_* */
    int pnp_score_rigid;      /* pnp_tracker.iterative_kp.score_method */
    int num_row, num_col;     /* kp_selection.rigid_flow_kp.num_row / num_col */
    int num_bestN;            /* kp_selection.rigid_flow_kp.num_bestN */
    double rigid_flow_thre;   /* kp_selection.rigid_flow_kp.rigid_flow_thre */
    double optical_flow_thre; /* kp_selection.rigid_flow_kp.optical_flow_thre */
} dfvo_pipeline_refine_opts;
int dfvo_pipeline_set_refine(dfvo_pipeline* p, const dfvo_pipeline_refine_opts* opts);
/* what the refinement did for the pair last collected from `slot` (until the slot's next dfvo_pipeline_track_begin) */
typedef struct dfvo_refine_out {
    int e_ran;         /* the kp_depth selection of the E refinement ran (pass one had a translation) */
    int scale_ran;     /* the second scale stage ran (second pass with a translation, scale_enable) */
    int pnp_ran;       /* the kp_depth selection of the PnP refinement ran */
    int empty;         /* 1: that selection was empty (dfvo_pipeline_track_end returned DFVO_ERR_EMPTY_SELECTION) */
    int n_kp;          /* kp_depth keypoints of the pair's last selection (0: none ran) */
    int n_inliers;     /* kp_depth keypoints of the E refinement = entries of the second pass's inlier mask (0: it did not run) */
    int pnp_found1;    /* PnP pass one found a model */
    int pad;
    double R1[9], t1[3]; /* E pass one's pose (identity, 0 when the pair ran no E-tracker) */
    double scale1;       /* pass one's scale (0: no scale stage ran) */
    double scale2;       /* the second scale stage's result (0: it did not run) */
    double pnp_R1[9], pnp_t1[3]; /* PnP pass one: Rodrigues(rvec), tvec (identity, 0 without a model) */
} dfvo_refine_out;
/* h_kp_ref / h_kp_cur (optional, double [cap,2]): kp_depth of the reference / current frame, the first min(n_kp, cap) rows;
 * h_inliers (optional, uint8 [cap]): the second E pass's inlier mask, min(n_inliers, cap) entries; h_rigid_flow_diff (optional,
 * float [H,W]): the distance map of the pair's last selection.  DFVO_ERR_ARG unless dfvo_pipeline_set_refine switched a
 * refinement on.  Waits for the device. */
int dfvo_pipeline_get_refine(dfvo_pipeline* p, int slot, dfvo_refine_out* out, int cap, double* h_kp_ref, double* h_kp_cur,
                             uint8_t* h_inliers, float* h_rigid_flow_diff);
/* EssTracker.prev_scale as the pipeline carries it (host double in / out; both wait for the chain stream; _set needs no pair
 * pending) */
int dfvo_pipeline_get_prev_scale(dfvo_pipeline* p, double* h_scale);
int dfvo_pipeline_set_prev_scale(dfvo_pipeline* p, double scale);
/* depth.depth_src (dfvo.py:296-319): where the depth of a frame comes from.  DFVO_DEPTH_NET (all zero, the default: a pipeline
 * on which this is never called enqueues exactly what it enqueued before): monodepth2.  DFVO_DEPTH_EXTERNAL (depth_src gt): a
 * 16-bit depth image per frame, uint16 [src_h,src_w] on the device as the decoder left it, through dfvo_read_depth_u16 with
 * `scale` (the loader's scale_factor: 500 kitti.py, 5000 tum.py / kinect.py), the crop and the depth range of
 * dfvo_pipeline_cfg; the pipeline then has no depth net: dfvo_pipeline_finalize needs no depth parameters and neither builds
 * nor captures it, dfvo_pipeline_net_flops counts the flow net only.  Everything behind the slot's raw / processed depth (scale
 * recovery, the iterative loop and its raw roll-over, the PnP fallback, tracking_method PNP, every depth override) is the same
 * in both modes.  State rule: after dfvo_pipeline_create, before dfvo_pipeline_finalize and the first
 * dfvo_pipeline_enqueue_nets / _set_ref_*.  In EXTERNAL mode dfvo_pipeline_enqueue_nets, dfvo_pipeline_set_ref_image and
 * dfvo_pipeline_set_ref_depth with d_feed return DFVO_ERR_ARG; in NET mode dfvo_pipeline_enqueue_nets_depth and
 * dfvo_pipeline_set_ref_depth_u16 do. */
#define DFVO_DEPTH_NET 0
#define DFVO_DEPTH_EXTERNAL 1
typedef struct dfvo_pipeline_depth_src {
    int source;       /* DFVO_DEPTH_NET | DFVO_DEPTH_EXTERNAL */
    double scale;     /* EXTERNAL: depth [m] = u16 / scale; finite, > 0 */
    int src_h, src_w; /* EXTERNAL: size of the depth images, >= 1 (any size: resized INTER_NEAREST to img_h x img_w) */
} dfvo_pipeline_depth_src;
int dfvo_pipeline_set_depth_source(dfvo_pipeline* p, const dfvo_pipeline_depth_src* src);
/* number of output slots: the host may run the nets this many pairs ahead of the solver stage (the nets of pairs
 * k+1 .. k+3 queue up behind each other on their streams while dfvo_pipeline_track(k) blocks the host) */
#define DFVO_PIPELINE_SLOTS 4
/* Ordering contract for every device frame handed to the three calls below: they are ASYNCHRONOUS and read the frame on
 * the pipeline's own non-blocking HIP streams.  (1) The frame must be complete when the call is made -- work still queued
 * on another stream (e.g. a resize on the caller's stream) is not waited for.  (2) The frame must stay unchanged, and
 * allocated, until dfvo_pipeline_track() of that slot has returned (enqueue_nets) / until dfvo_pipeline_sync() or the
 * first dfvo_pipeline_track() after the call has returned (set_ref_depth, set_ref_image).
 * The 16-bit depth image of dfvo_pipeline_enqueue_nets_depth / dfvo_pipeline_set_ref_depth_u16 stands under the same contract
 * as the frame it belongs to: complete when handed over (its upload drained), unchanged and allocated until the slot's
 * dfvo_pipeline_track() / dfvo_pipeline_track_end() has returned (enqueue_nets_depth) / until dfvo_pipeline_sync() or the first
 * dfvo_pipeline_track() after the call has returned (set_ref_depth_u16). */
/* enqueue both nets for one pair into `slot` (0 .. DFVO_PIPELINE_SLOTS-1); returns at once.  d_* uint8 device images:
 * ref/cur [img_h,img_w,3], cur_feed [feed_h,feed_w,3] (the PIL-LANCZOS resized current frame) or NULL: the current frame
 * is then resized on the device (dfvo_resize_lanczos_u8's arithmetic) ahead of the depth net.
 * d_ref == NULL (sequences): the reference frame is the current frame of the previous dfvo_pipeline_enqueue_nets call.
 * LiteFlowNet's image pyramid and Features (lite_flow_net.py:78-86, 307-309) are functions of one frame each; the
 * reference's model call runs them on both frames of every pair, i.e. twice per frame of a sequence.  Here the pyramids
 * the previous pass computed for that frame are carried over (device copies, ordered by an event between the flow-net
 * instances) and only the new frame runs through Features: same values, 15 GFLOP less per pair at KITTI size. */
int dfvo_pipeline_enqueue_nets(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur,
                               const uint8_t* d_cur_feed);
/* depth of the very first reference frame (dfvo.py computes the depth of every frame as it becomes `cur`; the first
 * frame never is): exactly one of d_feed (uint8 [feed_h,feed_w,3], runs the depth net) or d_depth_override (processed
 * depth, double [H,W]).  Later reference depths roll over from the current frame of each tracked pair. */
int dfvo_pipeline_set_ref_depth(dfvo_pipeline* p, const uint8_t* d_feed, const double* d_depth_override);
/* same from the full-size first frame [img_h,img_w,3]: device LANCZOS resize, then the depth net */
int dfvo_pipeline_set_ref_image(dfvo_pipeline* p, const uint8_t* d_img);
/* DFVO_DEPTH_EXTERNAL (dfvo_pipeline_set_depth_source).  _enqueue_nets_depth is dfvo_pipeline_enqueue_nets with the current
 * frame's depth image, uint16 [src_h,src_w], in the place of the depth net: one dfvo_read_depth_u16 launch on the depth stream
 * writes the slot's raw and processed depth, ordered behind a pending roll-over of the reference depth as the depth net's
 * output stage is; the flow half (d_ref, d_cur, the d_ref == NULL carry-over) is the same.  _set_ref_depth_u16 is the depth
 * image of the very first reference frame: it writes the reference side's raw and processed depth (so the iterative scale
 * loop needs no dfvo_pipeline_set_ref_raw_depth) and orders the chain's stream behind it on the device. */
int dfvo_pipeline_enqueue_nets_depth(dfvo_pipeline* p, int slot, const uint8_t* d_ref, const uint8_t* d_cur,
                                     const uint16_t* d_depth_u16);
int dfvo_pipeline_set_ref_depth_u16(dfvo_pipeline* p, const uint16_t* d_depth_u16);
/* The raw-depth counterparts of the processed-depth overrides, for callers that bring their own depth (iterative scale
 * recovery only; float [H,W] on the device).  _set_ref_raw_depth: ref_data['raw_depth'] of the first pair (copied; counts as
 * an enqueue for the state rule of dfvo_pipeline_set_options).  _set_raw_depth_override: the raw depth of `slot`'s current
 * frame, which rolls over to the reference side in dfvo_pipeline_track_end in place of the depth net's; valid until that call
 * (NULL withdraws it), the array stays allocated as d_depth_override of dfvo_pipeline_track_begin does. */
int dfvo_pipeline_set_ref_raw_depth(dfvo_pipeline* p, const float* d_raw);
int dfvo_pipeline_set_raw_depth_override(dfvo_pipeline* p, int slot, const float* d_raw);
/* Optional: enqueue the RNG-independent half of the solver stage of `slot` (keypoint selection, homography RANSAC +
 * refinement, GRIC-H) right after dfvo_pipeline_enqueue_nets(slot, ...).  It waits for the slot's flow outputs on the
 * device and runs on its own stream, i.e. under the nets / solver stage of earlier pairs; dfvo_pipeline_track(slot)
 * then only adds the numpy-RandomState consumers (shuffles, five-point RANSAC, scale, PnP), in pair order.  The
 * overrides, when given, must be the ones later passed to dfvo_pipeline_track.  Returns at once. */
int dfvo_pipeline_prefetch_track(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override);
/* keypoint selection + E-tracker + scale recovery (+ the PnP fallback when the E-tracker result is rejected) on the
 * outputs in `slot` (waits for its nets).  Optional device overrides replace the forward flow [2,H,W] / consistency
 * map [H,W] / processed depth [H,W] double that feed the solver stage (used by bench.py). Synchronous. */
int dfvo_pipeline_track(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override,
                        const double* d_depth_override, dfvo_track_out* out);
/* The same in two halves, so that the host can enqueue the nets of the pairs ahead while the chain of this pair runs:
 * _begin waits for the slot's keypoint stage and enqueues the RandomState-ordered chain + the copy of its results into
 * pinned host memory; _end waits for them, runs the PnP fallback where the reference takes it and rolls the reference
 * depth over.  Pairs must be begun and ended in order, and pair k + 1 must not be begun before pair k was ended (the PnP
 * fallback of pair k consumes the RandomState ahead of pair k + 1's shuffles).  dfvo_pipeline_track = _begin + _end.
 * Lifetime of the overrides with the split calls: _end enqueues the roll-over copy of the reference depth (from
 * d_depth_override when one was given to _begin) and returns WITHOUT waiting for it; a caller-owned d_depth_override must
 * therefore stay unchanged and allocated until the next dfvo_pipeline_track_end / dfvo_pipeline_sync has returned (the
 * flow / consistency overrides: until _end of their own pair has returned).  The pipeline's own buffers are ordered on
 * the device (the depth stream's next write of the slot waits for the copy). */
int dfvo_pipeline_track_begin(dfvo_pipeline* p, int slot, const float* d_flow_override, const float* d_diff_override,
                              const double* d_depth_override);
int dfvo_pipeline_track_end(dfvo_pipeline* p, int slot, dfvo_track_out* out);
int dfvo_pipeline_get_flow(dfvo_pipeline* p, int slot, float* h_fwd, float* h_bwd, float* h_diff, float* h_raw_depth,
                           double* h_depth);
/* inspection: the reference frame's depths as the next pair will read them -- raw (float [H,W]; written by
 * dfvo_pipeline_set_ref_depth (d_feed) / _set_ref_image / _set_ref_raw_depth, and by the roll-over while the iterative scale
 * recovery is on) and processed (double [H,W]); either may be NULL.  Waits for the device. */
int dfvo_pipeline_get_ref_depth(dfvo_pipeline* p, float* h_raw_depth, double* h_depth);
/* inspection (tests, debugging): keypoints selected for `slot` (kp_best of ref / cur, double [n][2], x,y), the E-tracker's
 * best inlier mask (uint8 [n]; ref_data['inliers'], dfvo.py:179) -- up to `cap` entries, *n_out = the full count -- and the
 * numpy RandomState the pipeline carries from pair to pair (uint32 key[624] + pos, np.random.get_state() layout) */
int dfvo_pipeline_get_keypoints(dfvo_pipeline* p, int slot, int cap, double* h_kp_ref, double* h_kp_cur,
                                uint8_t* h_inliers, int* n_out);
/* the iterative scale loop's record of the pair last collected from `slot` (dfvo_pipeline_set_iterative; until the slot's next
 * dfvo_pipeline_track_begin): `out` as dfvo_scale_recovery_iterative documents it, with one more status value, 3 "not run", for
 * a pair whose E-tracker pose had no translation or that never reached the scale stage (n_iter 0, kp_round -1, n_kp 0;
 * device_ms is not measured here: 0).  h_kp_ref / h_kp_cur (optional, [cap,2]): the uniform keypoints of the last round that
 * selected any, the first min(out->n_kp, cap) rows; h_rigid_flow_diff (optional, float [H,W]): that round's distance map. */
int dfvo_pipeline_get_iterative(dfvo_pipeline* p, int slot, dfvo_scale_iter_out* out, int cap, double* h_kp_ref, double* h_kp_cur,
                                float* h_rigid_flow_diff);
int dfvo_pipeline_get_rng_state(dfvo_pipeline* p, uint32_t* h_state625);
int dfvo_pipeline_set_rng_state(dfvo_pipeline* p, const uint32_t* h_state625);
int dfvo_pipeline_sync(dfvo_pipeline* p);
/* The stream layout in use, as one line of text in buf[n] (DFVO_ERR_ARG when it does not fit; 256 bytes do):
 *   "layout=lanes groups=4 queues=4 streams=4 trk=3 rep0=3 rep1=3 depth=2 pre0=2 pre1=2 flow=0 flow_x=1"
 * layout   wide: a stream per role, placed by dispatch pipe (eight or more hardware queues) | lanes: four streams, one per
 *          hardware queue, the roles of a lane on one stream (four to seven queues; GPU_MAX_HW_QUEUES defaults to 4) |
 *          creation: no usable measurement, freshly created streams.  DFVO_STREAM_LAYOUT=auto|wide|lanes (read by
 *          dfvo_pipeline_create) forces one.
 * groups / queues   dispatch-pipe groups and hardware queues the pipeline's twelve candidate streams were found to span (0: no
 *          measurement)
 * streams  distinct streams the roles run on; per role the index of its stream among them (equal = the same stream; -1 =
 *          the role does not exist, flow_x with one flow-net instance) */
int dfvo_pipeline_stream_layout(dfvo_pipeline* p, char* buf, int n);
double dfvo_pipeline_net_flops(const dfvo_pipeline* p);

/* ---- frame session: the reference's own synchronous call order, fast (df-vo_amd/csrc/session.hip) ----
 * /root/reference/libs/dfvo.py calls, per frame k: DeepModel.forward_depth([img_k]) (dfvo.py:312), forward_flow(cur, ref)
 * (:324), KeypointSampler.kp_selection (:147), EssTracker.compute_pose_2d2d (:168), scale_recovery (:198) -- blocking
 * calls, host numpy arrays in and out.  Everything they need is known at the first of them; dfvo_session_push_frame
 * (called by the DeepModel mirror from forward_depth) uploads the frame ONCE and enqueues, each on its own stream: the
 * depth net of frame k, the flow net of (k - 1, k) (frame k - 1's pyramids carried over), both outputs into pinned host
 * buffers, and -- when the KeypointSampler / EssTracker mirrors registered their configurations (kp, pose non-NULL) --
 * local_bestN and the RandomState-independent half of compute_pose_2d2d (findHomography + refinement + GRIC-H) behind the
 * flow net.  The later calls wait for an event and hand out the result; each validates that it is asked for exactly what
 * was enqueued (generation, configuration, keypoint arrays byte for byte, RandomState word for word) and otherwise runs the
 * plain entry point.
 * Results are identical to the plain entry points' (tests/test_dropin_gpu.py).  Host pointers returned here are pinned
 * buffers owned by the session, valid until two further frames have been pushed.  Not re-entrant. */
typedef struct dfvo_session dfvo_session;
typedef struct dfvo_session_kp_cfg {
    int num_row, num_col, num_bestN;  /* kp_selection.local_bestN.{num_row, num_col, num_bestN} */
    float thre;                       /* .thre */
    int score_method;                 /* DFVO_KP_SCORE_FLOW / DFVO_KP_SCORE_FLOW_RATIO */
} dfvo_session_kp_cfg;
int dfvo_session_create(dfvo_flownet* flow, dfvo_depthnet* depth, dfvo_tracker* trk, int img_h, int img_w, dfvo_session** out);
void dfvo_session_destroy(dfvo_session* s);
int dfvo_session_reset(dfvo_session* s);             /* forget the held frame (a new sequence) */
int dfvo_session_invalidate_carry(dfvo_session* s);  /* someone else ran the flow net: recompute both pyramids next time */
int dfvo_session_quiesce(dfvo_session* s);           /* a plain solver call is about to use the tracker: wait for the speculative stage */
/* h_img uint8 [img_h, img_w, 3] (copied into the session's pinned ring before the call returns); *generation = index of this
 * frame since create / reset.  flags: DFVO_PUSH_NO_FLOW = depth net only -- no flow pass of (generation - 1, generation), no
 * speculative stage (a caller that never asked for the flow of the last pushes; the next pair runs both frames through
 * Features). */
#define DFVO_PUSH_NO_FLOW 1
int dfvo_session_push_frame(dfvo_session* s, const uint8_t* h_img, const dfvo_session_kp_cfg* kp, const dfvo_pose2d2d_cfg* pose,
                            int flags, long long* generation);
/* float [feed_h, feed_w].  DFVO_ERR_RANGE (pointer still set) when the depth net of this frame drove an activation out of
 * f16's range under an f16x3 / f16 packing: the map holds inf / NaN.  Every read of such a generation returns it. */
int dfvo_session_depth(dfvo_session* s, long long generation, const float** h_depth);
/* flow of (generation - 1, generation): fwd / bwd float [2, img_h, img_w], diff float [img_h, img_w]; DFVO_ERR_RANGE as above */
int dfvo_session_flow(dfvo_session* s, long long generation, const float** h_fwd, const float** h_bwd, const float** h_diff);
/* the session's pinned copy of frame `generation` (the newest or the one before), uint8 [img_h, img_w, 3]: what was uploaded --
 * the mirror compares the frames handed to forward_flow with it byte for byte */
int dfvo_session_frame(dfvo_session* s, long long generation, const uint8_t** h_frame);
/* Buffer lifetime: the pointers dfvo_session_depth / _flow return belong to ring slot generation % 3 and are overwritten by
 * the push of generation + 3.  A caller that still references them then (or at dfvo_session_destroy) takes them over:
 * h_old4 = {depth, fwd, bwd, diff} of that slot, the session allocates itself fresh ones; release each with dfvo_host_free. */
int dfvo_session_detach_slot(dfvo_session* s, long long generation, void** h_old4);
int dfvo_host_free(void* h_pinned);
int dfvo_session_keypoints(dfvo_session* s, long long generation, const dfvo_session_kp_cfg* kp, const double** h_kp_ref,
                           const double** h_kp_cur, int* n, int* good_kp_found);
/* The RandomState-consuming half of compute_pose_2d2d (shuffles, five-point RANSACs, GRIC-E, recoverPose) enqueued AHEAD of
 * the call, as soon as the keypoints of `generation` exist, under the RandomState the caller has now (h_rng625: numpy's 624
 * key words + position).  The DeepModel mirror calls it from forward_flow.  *enqueued = 1 when it was. */
int dfvo_session_pose_ahead(dfvo_session* s, long long generation, const uint32_t* h_rng625, const dfvo_pose2d2d_cfg* cfg,
                            int* enqueued);
/* dfvo_compute_pose_2d2d through the session, under the RandomState h_rng625 (np.random's state at the call; the tracker's
 * device copy is set from it unless the result enqueued ahead is handed out).  *used_resident = 2: the call had been enqueued
 * ahead under exactly this RandomState, these keypoints and this configuration; 1: only the RandomState-consuming half had
 * to run; 0: the plain entry point ran.  Read the advanced state back with dfvo_tracker_get_rng_state. */
int dfvo_session_pose_2d2d(dfvo_session* s, const double* h_kp_ref, const double* h_kp_cur, int n, const dfvo_pose2d2d_cfg* cfg,
                           dfvo_pose2d2d_out* out, uint8_t* h_inliers, const uint32_t* h_rng625, int* used_resident);

/* ---- the dense panels of the frame drawer (libs/general/frame_drawer.py:410-512) ----
 * FrameDrawer.main draws, per frame, the depth / disparity map (matplotlib magma), the forward and backward flow
 * (flowlib.flow_to_image: the Middlebury wheel) and the consistency maps (jet), each cvtColor'ed to BGR and cv2.resize'd into
 * a cell of the window.  dfvo_vis owns the window canvas (uint8 BGR [window_h, window_w, 3], zero at creation) in HBM and the
 * reference's quarter-grid rectangles int(h / 4 * r), int(w / 4 * c):
 *     DFVO_VIS_CELL_DEPTH rows 2-3 cols 2-3 | DFVO_VIS_CELL_FLOW1 rows 2-3 cols 3-4
 *     DFVO_VIS_CELL_FLOW2 rows 3-4 cols 2-3 ('flow2', 'rigid_flow_diff' and 'warp_diff' share it) | DFVO_VIS_CELL_OPT_FLOW_DIFF rows 3-4 cols 3-4
 * A draw call colours only the <= 4 source pixels a cell pixel samples and blends them with dfvo_resize_linear_u8's
 * arithmetic (the exact-half area path included); what needs the whole map -- the maximum flow radius, the exact 90th
 * percentile of the disparity -- runs in front of it on the device.  Results equal the reference's numpy (NEP 50) /
 * matplotlib arithmetic; maps of up to 1280 x 1920.  Every draw call returns when the cell is drawn. */
typedef struct dfvo_vis dfvo_vis;
#define DFVO_VIS_CELLS 4
#define DFVO_VIS_CELL_DEPTH 0
#define DFVO_VIS_CELL_FLOW1 1
#define DFVO_VIS_CELL_FLOW2 2
#define DFVO_VIS_CELL_OPT_FLOW_DIFF 3
#define DFVO_VIS_MAP_VALUE 0     /* colour the map itself: Normalize(0, vmax) */
#define DFVO_VIS_MAP_DISPARITY 1 /* colour 1 / (map + 1e-3), map == 0 -> 0; vmax = np.percentile(.., 90) */
#define DFVO_VIS_MAGMA 0
#define DFVO_VIS_JET 1
#define DFVO_VIS_COUNTERS 8
int dfvo_vis_create(int window_h, int window_w, dfvo_vis** out);
void dfvo_vis_destroy(dfvo_vis* v);
int dfvo_vis_cell_rect(const dfvo_vis* v, int cell, int* y0x0y1x1);
/* draw_flow (frame_drawer.py:446-459): h_flow float [2, H, W].  *n_unknown = pixels with |u| or |v| > 1e7: flow_to_image
 * zeroes those in the CALLER's array (flowlib.py:203-205); a caller that mirrors it applies that write when the count is not 0. */
int dfvo_vis_draw_flow(dfvo_vis* v, int cell, const float* h_flow, int H, int W, long long* n_unknown);
/* draw_depth / draw_flow_consistency / draw_rigid_flow_consistency (:410-444, 461-512): h_map float32 / float64 [H, W].
 * kind DFVO_VIS_MAP_VALUE uses vmax_in; DFVO_VIS_MAP_DISPARITY computes it.  *vmax_out = the vmax used; when it is negative
 * matplotlib's Normalize raises and the cell is left as it was. */
int dfvo_vis_draw_map(dfvo_vis* v, int cell, const void* h_map, int is_f64, int H, int W, int kind, int cmap, double vmax_in,
                      double* vmax_out);
/* The panels of the session's newest generation from its device-resident buffers, behind the events that guard them, in ONE
 * panel launch: cells = bit mask (1 << DFVO_VIS_CELL_*): FLOW1 forward flow, FLOW2 backward flow, OPT_FLOW_DIFF the
 * consistency map (jet, diff_vmax), DEPTH the raw depth [feed_h, feed_w] (magma; depth_kind / depth_vmax as in
 * dfvo_vis_draw_map).  n_unknown2[2]: unknown pixels of the forward / backward flow.  Reads the session, changes nothing in it.
 * DFVO_ERR_STATE when a requested buffer no longer holds that generation (dfvo_vis_session_cells). */
int dfvo_vis_draw_session(dfvo_vis* v, dfvo_session* s, long long generation, int cells, double diff_vmax, int depth_kind,
                          double depth_vmax, long long* n_unknown2, double* depth_vmax_out);
/* Which cells dfvo_vis_draw_session can serve now (bit mask): the session's device buffers are the nets' own output buffers,
 * and any other pass on the same net (dfvo_flownet_forward_host on another pair, dfvo_depthnet_forward* on another frame)
 * overwrites them while the session's generation and pinned host copies stay.  A cell whose bit is clear must be drawn from
 * the host array (dfvo_vis_draw_flow / _map); dfvo_vis_draw_session returns DFVO_ERR_STATE for it. */
int dfvo_vis_session_cells(dfvo_session* s, long long generation, int* cells);
int dfvo_vis_clear_cell(dfvo_vis* v, int cell);
/* cell >= 0: that cell, uint8 BGR [cell_h, cell_w, 3]; cell = -1: the whole canvas */
int dfvo_vis_fetch(dfvo_vis* v, int cell, uint8_t* h_dst);
/* counters since creation: [0] panels drawn from session buffers, [1] panels drawn from uploaded arrays, [2] panel launches,
 * [3] percentile selects, [4] cells cleared, [5] bytes uploaded, [6] bytes fetched, [7] 0 */
int dfvo_vis_counters(const dfvo_vis* v, long long* out);
/* device time of the last draw call (reductions + panel launch), from HIP events */
int dfvo_vis_device_ms(const dfvo_vis* v, float* ms);
/* flowlib.flow_to_image at full resolution: h_rgb uint8 RGB [H, W, 3] */
int dfvo_vis_flow_rgb(dfvo_vis* v, const float* h_flow, int H, int W, uint8_t* h_rgb, long long* n_unknown);
/* np.percentile(disparity, 90) of h_depth[n] (float32 / float64), exact: the two neighbouring order statistics by a radix
 * select, numpy's _lerp; *out = the value widened to double */
int dfvo_vis_disparity_percentile90(dfvo_vis* v, const void* h_depth, int is_f64, int n, double* out);

/* DFVO.update_global_pose (dfvo.py:109-119: t_w += R_w t, then R_w = R_w R) over a whole gathered sequence in ONE launch,
 * constant-motion rows included (dfvo.py:157-161: a row with status 1 reuses the previous pair's relative motion).
 * rows [n][17] = relative pose cur -> ref (4x4 row major) | status (the layout of dist.allgather_poses); first [16] = pose
 * of frame 0 (NULL: identity); poses [n+1][16] out.  *h_bad_row = index of the first status-2 row (a pair that needed the
 * PnP fallback but had no reference depth), -1 when there is none.  The _device variant takes device pointers (the
 * gathered rows are already in HBM after the RCCL all-gather) and a HIP stream. */
int dfvo_compose_trajectory(const double* h_rows, int n, const double* h_first, double* h_poses, int* h_bad_row);
int dfvo_compose_trajectory_device(const double* d_rows, int n, const double* d_first, double* d_poses, int* h_bad_row,
                                   void* stream);

/* ---- the data-parallel exchange step (SURVEY.md section 8e / 8b "dfvo_allgather_poses") ----
 * Every rank tracks its chunks of frame pairs with no activation exchange; ONE RCCL ncclAllGather per job then hands every
 * rank all relative poses (rows of DFVO_POSE_ROW = 17 doubles: 4x4 row-major cur -> ref pose | status), after which each
 * rank (or rank 0) composes the trajectories with dfvo_compose_trajectory.  Replaces the sequential hand-over of
 * update_global_pose between frames (dfvo.py:109-119,157-161) for chunks tracked on different GPUs.
 * dfvo_comm wraps one RCCL communicator (bound with dlopen("librccl.so.1") at first use; its absence is an error, there is
 * no fallback).  Bootstrap as with NCCL: rank 0 calls dfvo_comm_unique_id and ships the DFVO_COMM_ID_BYTES bytes to every
 * rank by any out-of-band means (file, socket, MPI, torch's store); every rank calls dfvo_comm_create (collective; select
 * the GPU with dfvo_set_device first).
 * dfvo_allgather_poses: h_rows [n_local][17] of this rank, counts[world] = rows of every rank (deterministic: the chunking
 * is a function of the job, so no count exchange precedes the collective), h_out [sum counts][17] in rank order.  Ranks
 * pad to max(counts) rows for the fixed-size collective; the padding is trimmed here.  Synchronous.
 * _device: the bare collective on caller-owned device buffers (d_send [rows_per_rank][17], d_recv [world][rows_per_rank]
 * [17]) on `stream` (NULL: the communicator's own), asynchronous. */
#define DFVO_COMM_ID_BYTES 128
#define DFVO_POSE_ROW 17
typedef struct dfvo_comm dfvo_comm;
int dfvo_comm_unique_id(uint8_t* h_id128);
int dfvo_comm_create(const uint8_t* h_id128, int world, int rank, dfvo_comm** out);
int dfvo_comm_destroy(dfvo_comm* c);
int dfvo_allgather_poses(dfvo_comm* c, const double* h_rows, int n_local, const int* counts, double* h_out);
int dfvo_allgather_poses_device(dfvo_comm* c, const double* d_send, int rows_per_rank, double* d_recv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFVO_HIP_H */
