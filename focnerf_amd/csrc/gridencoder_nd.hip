// gridencoder_nd.hip — the grid encoder for input dimensions 4 and 5 (gridencoder.cu:393-398, 437-442, 633-638 dispatch D in {2,3,4,5}).
//
// The NeRF networks of the path are D = 3 (and D = 2 for the background), which gridencoder.hip serves with D known at compile time
// (unrolled corners, shared index terms, row-pair loads, the binned backward). D = 4 / 5 — space-time grids, dnerf-style callers — take
// D as a RUNTIME value: 16 / 32 corners per (point, level) fully unrolled for every (D, C, dtype) multiplied the build time of the
// library several times over for shapes no FOC network uses. This file holds no kernel text of its own: it instantiates the general
// kernels of ge_common.h (forward with dy_dx, atomic backward, grad_inputs, grad_tv: the same arithmetic and layouts as D = 2, 3, the
// same 1-D level decode for the backward and grad_tv, blockIdx.y = level for the forward) for GeDimRT and every (C, dtype), and is a
// translation unit of its own so that they compile beside gridencoder.hip.
#include "ge_common.h"

int ge_nd_dispatch(GeOp op, const GeCall &a) { return ge_dispatch<GeDimRT>(op, a); }      // the caller has checked D (4 or 5: GeDimRT::MAX)
