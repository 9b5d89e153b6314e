// ssrlcv_amd/csrc/mesh_corners.h -- which corners of a cell a triangle of the grid mesh has (include/ssrlcv_hip.h "disparity mesh"
// item 3): the one definition mesh.hip's triangle list and normals and render.hip's rasteriser share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The corners of triangle t of a cell whose diagonal is b-c (bc) or a-d, as offsets (di, dj) from corner a packed two bits a
// corner: a = 0, b = 1, c = 2, d = 3, so di = corner & 1, dj = corner >> 1.
//   a-d: T0 = (a, c, d), T1 = (a, d, b);   b-c: T0 = (a, c, b), T1 = (b, c, d)
__device__ __forceinline__ void triangle_corners(bool bc, int t, uint32_t (&corner)[3]) {
  if (!bc) {
    corner[0] = 0u;
    corner[1] = t == 0 ? 2u : 3u;
    corner[2] = t == 0 ? 3u : 1u;
  } else {
    corner[0] = t == 0 ? 0u : 1u;
    corner[1] = 2u;
    corner[2] = t == 0 ? 1u : 3u;
  }
}

// the nodes of triangle t of cell (ci, cj) of a grid gw nodes wide
__device__ __forceinline__ void triangle_nodes(uint32_t gw, uint32_t ci, uint32_t cj, bool bc, int t, uint32_t (&node)[3]) {
  uint32_t corner[3];
  triangle_corners(bc, t, corner);
#pragma unroll
  for (int k = 0; k < 3; ++k) node[k] = (cj + (corner[k] >> 1)) * gw + ci + (corner[k] & 1u);
}
