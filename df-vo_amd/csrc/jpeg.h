// The device half of the JPEG decode as the frame ring enqueues it (jpeg.hip; include/dfvo_hip.h, dfvo_jpeg_decode_u8).
#pragma once
#include "dfvo_common.h"

namespace dfvo {

// `info` is checked against the layout of its own size and sampling (DFVO_ERR_ARG, message prefixed with `fn`) before anything
// is launched; d_coeffs is the device copy of the entropy pass's buffer and is used as the workspace
int enqueue_jpeg_decode(uint8_t* d_coeffs, const dfvo_jpeg_info* info, uint8_t* d_dst, hipStream_t s, const char* fn);

}  // namespace dfvo
