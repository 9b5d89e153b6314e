// ssrlcv_amd/host/GridMesh.hpp -- the triangle mesh of a disparity map as a value (include/ssrlcv_hip.h "disparity mesh"):
// what DisparityFactory::generateMesh returns and MeshFactory::setSurface takes.  Both maps are in state gpu; a grid without a
// cell (gw or gh below 2) still holds one unused byte in `cells`, because a Unity is never empty.
#pragma once
#include "Unity.hpp"

namespace ssrlcv {

struct GridMesh {
  unsigned int gw = 0, gh = 0;                        // the nodes of the sampling grid
  ptr::value<Unity<unsigned int>> vertexIndex;        // [gw gh]: the node's vertex, UINT32_MAX for none
  ptr::value<Unity<unsigned char>> cells;             // [(gw - 1) (gh - 1)]: bit 0 / 1 = triangle T0 / T1, bit 2 = diagonal b-c
  unsigned int vertexCount = 0;                       // the vertices are 0 .. vertexCount - 1, generateMatches' records
  unsigned long numCells() const { return gw >= 2 && gh >= 2 ? (unsigned long)(gw - 1) * (gh - 1) : 0ul; }
};

}  // namespace ssrlcv
