// Launcher of the LV geometry kernel (lvgeom.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Per frame f of masks (F,H,W) uint8: area[f] = pixels equal to label, geom[f * CLASFV_LV_STRIDE ..] = length,
// radii[0..9], volume (the arguments of clasfv_lv_geometry, already checked by it: H * W <= CLASFV_LV_MAX_PIXELS).
// One launch, one workgroup per frame.
hipError_t launch_lv_geometry(const uint8_t* masks, int64_t F, int H, int W, int label, double sy, double sx,
                              int32_t* area, double* geom, hipStream_t s);
