// Launcher of the mask cleanup kernel (cleanup.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Every frame of frames (F,H,W) uint8 cleaned in place by the rule of clasfv_fuse_votes' CLASFV_FUSE_CLEAN
// (include/clasfv.h). H * W <= CLASFV_CLEAN_MAX_PIXELS, 1 <= holesize <= 32767.
hipError_t launch_cleanup_frames(uint8_t* frames, int64_t F, int H, int W, int holesize, hipStream_t s);
