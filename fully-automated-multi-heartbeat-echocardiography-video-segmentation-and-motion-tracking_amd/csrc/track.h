// Launcher of the label / image tracking kernels (track.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// out (P,N,C,H,W): frame p is img after p + 1 warps through motion frames t0, t0 + t_step, ... (the
// arguments of clasfv_track, already checked by it). mode: CLASFV_TRACK_BILINEAR or CLASFV_TRACK_NEAREST,
// optionally with CLASFV_TRACK_FORCE_STEPS or CLASFV_TRACK_FORCE_LDS. The LDS path (one launch, the plane on
// the chip) serves planes of at most CLASFV_TRACK_LDS_AUTO_PIXELS pixels, or under FORCE_LDS every plane of at
// most CLASFV_TRACK_LDS_MAX_PIXELS; everything else runs as P launches through HBM.
hipError_t launch_track(const float* img, int N, int C, int H, int W, const float* motion, int64_t m_sn, int64_t m_sc,
                        int64_t m_st, int t0, int t_step, int P, int mode, float* out, hipStream_t s);
