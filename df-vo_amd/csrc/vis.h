// Dense drawer panels (vis.hip): what the translation units of the C surface share.
#pragma once
#include "dfvo_common.h"

namespace dfvo {

enum VisKind { VIS_WHEEL = 0, VIS_CMAP = 1, VIS_DISP = 2 };  // Middlebury wheel | colour map of the map | ... of 1 / (map + 1e-3)
enum VisCmap { VIS_CMAP_MAGMA = 0, VIS_CMAP_JET = 1 };
constexpr int VIS_MAX_PANELS = 4;

// one panel of a launch (kernel argument, by value): a source map in HBM and the rectangle of the canvas it is resized into
struct VisPanel {
    int kind, f64, cmap;
    int H, W;               // source map
    int y0, x0, ch, cw;     // cell of the canvas
    int area2;              // the cell is exactly half the map in both axes: cv2.resize's 2 x 2 area path
    double scale_x, scale_y;
    const void* src;               // [H, W] float32 / float64, or the flow [2, H, W] float32
    const unsigned* maxrad_bits;   // wheel: bits of max sqrt(u^2 + v^2) (float32), a NaN pattern when a radius is NaN
    const double* vmax_dev;        // colour maps: Normalize's vmax when it is computed on the device (else null, vmax below)
    double vmax;
};
struct VisPanels {
    VisPanel p[VIS_MAX_PANELS];
};

// what a frame session lends the drawer: its nets' output buffers and the events recorded behind the nets that write them.
// The pinned host ring the mirrors compare arrays with is a COPY of these: equality with the ring admits an array only
// while have_flow / have_depth say the device side still is what was copied
struct VisSessionSources {
    const float *fwd = nullptr, *bwd = nullptr, *diff = nullptr, *depth = nullptr;
    int H = 0, W = 0, depth_h = 0, depth_w = 0;
    hipEvent_t e_net = nullptr, e_depth = nullptr;
    bool have_flow = false, have_depth = false;  // the buffers still hold that generation (no other pass overwrote them)
};

}  // namespace dfvo

// session.hip: the device buffers of `generation` (the newest pushed frame only)
int dfvo_session_vis_sources(dfvo_session* s, long long generation, dfvo::VisSessionSources* out);
