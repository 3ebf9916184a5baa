// The input stage's operator (undistort.hip): bilinear Bayer demosaic and the order-1 remap through a per-pixel table.
#pragma once
#include "dev_mem.h"

struct dfvo_undistort_map {
    int h = 0, w = 0;
    dfvo::DevArr<double> xy;  // [h * w][2]: (x, y) of the source sample of every output pixel, one 16-byte load each
};

namespace dfvo {

// the argument checks of dfvo_undistort_mosaic_u8 under the caller's name; nothing is enqueued
int check_undistort_mosaic(const char* fn, const dfvo_undistort_map* map, int img_h, int img_w, int pattern, int border, int y0, int y1,
                           int x0, int x1);
// d_mosaic uint8 [img_h, img_w] -> the box of d_rgb uint8 [img_h, img_w, 3]; arguments as check_undistort_mosaic passed them
int enqueue_undistort_mosaic(const dfvo_undistort_map* map, const uint8_t* d_mosaic, int img_h, int img_w, int pattern, int border,
                             int y0, int y1, int x0, int x1, uint8_t* d_rgb, hipStream_t s);

}  // namespace dfvo
