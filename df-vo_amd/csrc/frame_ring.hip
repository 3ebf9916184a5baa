// Device frame ring (include/dfvo_hip.h, dfvo_frame_ring_*): the upload stage of a sequence read from disk.  Decoder threads
// write decoded frames into pinned staging slots; the consumer thread submits a slot -- one async copy on the ring's own
// stream, the read-image tail into the caller's output frame, an event -- and later waits on the slot's event, which is the
// hand-over point of the pipeline's frame contract (complete when enqueue_nets / set_ref_image is called).
#include "../../include/dfvo_hip.h"

#include <string.h>

#include <vector>

#include "dev_mem.h"
#include "jpeg.h"
#include "resize_lanczos.h"
#include "undistort.h"

using namespace dfvo;

struct dfvo_frame_ring {
    struct Slot {
        PinnedArr<uint8_t> staging;  // the decoded frame as the decoder left it
        DevArr<uint8_t> dev;         // its device copy (image submits; a raw submit copies into the caller's plane)
        hipEvent_t done = nullptr;
        bool pending = false;        // submitted, not waited for
    };
    std::vector<Slot> slots;
    size_t capacity = 0;  // bytes per slot
    DevArr<uint8_t> rgb;  // the demosaiced, undistorted plane of a mosaic submit, the decoded plane of a JPEG submit: one for all slots (one stream orders its uses)
    hipStream_t stream = nullptr;

    // every member is released here whether or not init completed (the arrays free themselves)
    ~dfvo_frame_ring() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (Slot& s : slots)
            if (s.done) (void)hipEventDestroy(s.done);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int init(int n, size_t bytes) {
        capacity = bytes;
        slots.resize((size_t)n);
        DFVO_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (Slot& s : slots) {
            int rc = s.staging.alloc(bytes);
            if (rc == DFVO_OK) rc = s.dev.alloc(bytes);
            if (rc != DFVO_OK) return rc;
            DFVO_HIP_CHECK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        }
        return DFVO_OK;
    }
};

#define RING_SLOT_CHECK(fn)                                                                             \
    DFVO_ARG_CHECK(r, fn ": null ring");                                                                \
    DFVO_ARG_CHECK(slot >= 0 && (size_t)slot < r->slots.size(), fn ": slot outside the ring")

extern "C" {

int dfvo_read_image_tail_gray_u8(const uint8_t* d_decoded, int img_h, int img_w, int y0, int y1, int x0, int x1, uint8_t* d_dst,
                                 int out_h, int out_w, void* stream) {
    DFVO_ARG_CHECK(d_decoded && d_dst && img_h > 0 && img_w > 0 && 0 <= y0 && y0 < y1 && y1 <= img_h && 0 <= x0 && x0 < x1 && x1 <= img_w,
                   "dfvo_read_image_tail_gray_u8: crop outside the frame");
    return enqueue_resize_linear_gray_u8(d_decoded + (size_t)y0 * img_w + x0, y1 - y0, x1 - x0, d_dst, out_h, out_w, (hipStream_t)stream,
                                         img_w);
}

int dfvo_frame_ring_create(int slots, size_t capacity_bytes, dfvo_frame_ring** out) {
    DFVO_ARG_CHECK(out, "dfvo_frame_ring_create: null out");
    *out = nullptr;
    DFVO_ARG_CHECK(slots >= 1 && slots <= 1024, "dfvo_frame_ring_create: slots outside 1 .. 1024");
    DFVO_ARG_CHECK(capacity_bytes >= 1 && capacity_bytes <= ((size_t)1 << 31), "dfvo_frame_ring_create: capacity outside 1 .. 2^31 bytes");
    dfvo_frame_ring* r = new dfvo_frame_ring();
    const int rc = r->init(slots, capacity_bytes);
    if (rc != DFVO_OK) {
        delete r;
        return rc;
    }
    *out = r;
    return DFVO_OK;
}

void dfvo_frame_ring_destroy(dfvo_frame_ring* r) { delete r; }

int dfvo_frame_ring_staging(dfvo_frame_ring* r, int slot, void** h_staging, size_t* capacity_bytes) {
    RING_SLOT_CHECK("dfvo_frame_ring_staging");
    DFVO_ARG_CHECK(h_staging, "dfvo_frame_ring_staging: null out");
    *h_staging = r->slots[slot].staging.p;
    if (capacity_bytes) *capacity_bytes = r->capacity;
    return DFVO_OK;
}

int dfvo_frame_ring_submit_image(dfvo_frame_ring* r, int slot, int img_h, int img_w, int channels, int bgr, int y0, int y1, int x0,
                                 int x1, uint8_t* d_dst, int out_h, int out_w) {
    RING_SLOT_CHECK("dfvo_frame_ring_submit_image");
    dfvo_frame_ring::Slot& s = r->slots[slot];
    DFVO_ARG_CHECK(!s.pending, "dfvo_frame_ring_submit_image: the slot's last submit has not been waited for");
    DFVO_ARG_CHECK(channels == 1 || channels == 3, "dfvo_frame_ring_submit_image: channels is 1 (grey) or 3");
    DFVO_ARG_CHECK(!(bgr && channels == 1), "dfvo_frame_ring_submit_image: bgr on a 1-channel frame");
    DFVO_ARG_CHECK(d_dst && out_h > 0 && out_w > 0, "dfvo_frame_ring_submit_image: no output frame");
    DFVO_ARG_CHECK(img_h > 0 && img_w > 0 && (size_t)img_h * (size_t)img_w * (size_t)channels <= r->capacity,
                   "dfvo_frame_ring_submit_image: the frame is larger than the staging capacity");
    DFVO_ARG_CHECK(0 <= y0 && y0 < y1 && y1 <= img_h && 0 <= x0 && x0 < x1 && x1 <= img_w,
                   "dfvo_frame_ring_submit_image: crop outside the frame");
    const size_t bytes = (size_t)img_h * img_w * channels;
    DFVO_HIP_CHECK(hipMemcpyAsync(s.dev.p, s.staging.p, bytes, hipMemcpyHostToDevice, r->stream));
    // from here on the slot is in flight whatever fails: wait() drains it
    s.pending = true;
    int rc;
    if (channels == 1)
        rc = dfvo_read_image_tail_gray_u8(s.dev.p, img_h, img_w, y0, y1, x0, x1, d_dst, out_h, out_w, r->stream);
    else
        rc = dfvo_read_image_tail_u8(s.dev.p, img_h, img_w, bgr, y0, y1, x0, x1, d_dst, out_h, out_w, r->stream);
    const hipError_t e = hipEventRecord(s.done, r->stream);  // (behind the copy also when the tail's launch failed)
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(e);
    return DFVO_OK;
}

int dfvo_frame_ring_submit_mosaic(dfvo_frame_ring* r, int slot, const dfvo_undistort_map* map, int pattern, int border, int img_h,
                                  int img_w, int y0, int y1, int x0, int x1, uint8_t* d_dst, int out_h, int out_w) {
    RING_SLOT_CHECK("dfvo_frame_ring_submit_mosaic");
    dfvo_frame_ring::Slot& s = r->slots[slot];
    DFVO_ARG_CHECK(!s.pending, "dfvo_frame_ring_submit_mosaic: the slot's last submit has not been waited for");
    DFVO_ARG_CHECK(d_dst && out_h > 0 && out_w > 0, "dfvo_frame_ring_submit_mosaic: no output frame");
    DFVO_ARG_CHECK(img_h > 0 && img_w > 0 && (size_t)img_h * (size_t)img_w <= r->capacity,
                   "dfvo_frame_ring_submit_mosaic: the frame is larger than the staging capacity");
    int rc = check_undistort_mosaic("dfvo_frame_ring_submit_mosaic", map, img_h, img_w, pattern, border, y0, y1, x0, x1);
    if (rc != DFVO_OK) return rc;
    const size_t bytes = (size_t)img_h * img_w;
    // (a plane that has to grow is freed first, and hipFree waits for the kernels that still use it)
    rc = r->rgb.grow(bytes * 3);
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(hipMemcpyAsync(s.dev.p, s.staging.p, bytes, hipMemcpyHostToDevice, r->stream));
    // from here on the slot is in flight whatever fails: wait() drains it
    s.pending = true;
    rc = enqueue_undistort_mosaic(map, s.dev.p, img_h, img_w, pattern, border, y0, y1, x0, x1, r->rgb.p, r->stream);
    if (rc == DFVO_OK) rc = dfvo_read_image_tail_u8(r->rgb.p, img_h, img_w, 0, y0, y1, x0, x1, d_dst, out_h, out_w, r->stream);
    const hipError_t e = hipEventRecord(s.done, r->stream);
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(e);
    return DFVO_OK;
}

int dfvo_frame_ring_submit_jpeg(dfvo_frame_ring* r, int slot, int y0, int y1, int x0, int x1, uint8_t* d_dst, int out_h, int out_w) {
    RING_SLOT_CHECK("dfvo_frame_ring_submit_jpeg");
    dfvo_frame_ring::Slot& s = r->slots[slot];
    DFVO_ARG_CHECK(!s.pending, "dfvo_frame_ring_submit_jpeg: the slot's last submit has not been waited for");
    DFVO_ARG_CHECK(d_dst && out_h > 0 && out_w > 0, "dfvo_frame_ring_submit_jpeg: no output frame");
    DFVO_ARG_CHECK(r->capacity >= sizeof(dfvo_jpeg_info), "dfvo_frame_ring_submit_jpeg: the staging capacity holds no header");
    dfvo_jpeg_info info;  // (a copy: the decoder thread is done with the slot, but the checks and the launches see one header)
    memcpy(&info, s.staging.p, sizeof(info));
    DFVO_ARG_CHECK(info.bytes >= DFVO_JPEG_HEADER_BYTES && info.bytes <= r->capacity,
                   "dfvo_frame_ring_submit_jpeg: the header and coefficients are larger than the staging capacity");
    DFVO_ARG_CHECK(info.width > 0 && info.height > 0 && 0 <= y0 && y0 < y1 && y1 <= info.height && 0 <= x0 && x0 < x1 && x1 <= info.width,
                   "dfvo_frame_ring_submit_jpeg: crop outside the frame");
    const int channels = info.components == 1 ? 1 : 3;
    // (a plane that has to grow is freed first, and hipFree waits for the kernels that still use it)
    int rc = r->rgb.grow((size_t)info.height * info.width * channels);
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(hipMemcpyAsync(s.dev.p, s.staging.p, (size_t)info.bytes, hipMemcpyHostToDevice, r->stream));
    // from here on the slot is in flight whatever fails: wait() drains it
    s.pending = true;
    rc = enqueue_jpeg_decode(s.dev.p, &info, r->rgb.p, r->stream, "dfvo_frame_ring_submit_jpeg");
    if (rc == DFVO_OK)
        rc = channels == 1 ? dfvo_read_image_tail_gray_u8(r->rgb.p, info.height, info.width, y0, y1, x0, x1, d_dst, out_h, out_w, r->stream)
                           : dfvo_read_image_tail_u8(r->rgb.p, info.height, info.width, 0, y0, y1, x0, x1, d_dst, out_h, out_w, r->stream);
    const hipError_t e = hipEventRecord(s.done, r->stream);
    if (rc != DFVO_OK) return rc;
    DFVO_HIP_CHECK(e);
    return DFVO_OK;
}

int dfvo_frame_ring_submit_raw(dfvo_frame_ring* r, int slot, size_t bytes, void* d_dst) {
    RING_SLOT_CHECK("dfvo_frame_ring_submit_raw");
    dfvo_frame_ring::Slot& s = r->slots[slot];
    DFVO_ARG_CHECK(!s.pending, "dfvo_frame_ring_submit_raw: the slot's last submit has not been waited for");
    DFVO_ARG_CHECK(d_dst, "dfvo_frame_ring_submit_raw: no output plane");
    DFVO_ARG_CHECK(bytes >= 1 && bytes <= r->capacity, "dfvo_frame_ring_submit_raw: the plane is larger than the staging capacity");
    DFVO_HIP_CHECK(hipMemcpyAsync(d_dst, s.staging.p, bytes, hipMemcpyHostToDevice, r->stream));
    s.pending = true;
    DFVO_HIP_CHECK(hipEventRecord(s.done, r->stream));
    return DFVO_OK;
}

int dfvo_frame_ring_wait(dfvo_frame_ring* r, int slot) {
    RING_SLOT_CHECK("dfvo_frame_ring_wait");
    dfvo_frame_ring::Slot& s = r->slots[slot];
    if (!s.pending) return DFVO_OK;
    const hipError_t e = hipEventSynchronize(s.done);
    s.pending = false;
    DFVO_HIP_CHECK(e);
    return DFVO_OK;
}

int dfvo_frame_ring_pending(dfvo_frame_ring* r, int* n_pending) {
    DFVO_ARG_CHECK(r && n_pending, "dfvo_frame_ring_pending: null argument");
    int n = 0;
    for (const dfvo_frame_ring::Slot& s : r->slots) n += s.pending ? 1 : 0;
    *n_pending = n;
    return DFVO_OK;
}

}  // extern "C"
