// ssrlcv_amd/csrc/cc_label.h -- the connected-component labelling of a float map (include/ssrlcv_hip.h "disparity post-filters"
// items 1-2) for the files that call it: disparity_filter.hip defines it (components, speckles) and objects.hip calls it
// (surface objects).  The kernels and their description stay at the head of disparity_filter.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svcc {

constexpr int kTileW = 64, kTileH = 16;  // the tile of k_cc_tile: a tile-local root lies in the tile of its pixels

// labels <- for a tile-local root the component's label, for every other pixel its tile-local root: the label is
// labels[labels[p]], UINT32_MAX for an invalid pixel; counts <- at every component's root its size.  w h >= 1 and below 2^31;
// both arrays hold w h words and may hold anything on entry.  Three launches on `stream`.
void label_components(const float* disparity, uint32_t w, uint32_t h, float maxDiff, uint32_t* labels, uint32_t* counts, hipStream_t stream);

}  // namespace svcc
