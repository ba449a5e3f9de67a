// Launcher of the annotated-video kernels (render.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The arguments of clasfv_render_annotated, already checked by it (count * (Hp + Ht + Hs) * Wo * 3 < 2^32,
// H * W < 2^31, workspace and volume 8-byte aligned). Two launches: the min / max of the finite volumes into
// workspace[0..1], then the frames.
struct RenderParams {
  const float* video;     // (3,T,H,W)
  const uint8_t* masks;   // (T,H,W)
  const uint8_t* truth;   // (T,H,W) or nullptr
  const double* volume;   // T doubles, `vstride` elements apart
  const uint8_t* title;   // (Ht,Wo,3) or nullptr
  double* workspace;      // CLASFV_RENDER_WORKSPACE_BYTES
  uint8_t* out;           // (count, Hp + Ht + Hs, Wo, 3)
  int64_t vstride;
  int T, H, W, first, count, Hp, Wo, Ht, Hs, label;
  double thickness;
};
constexpr int CLASFV_RENDER_WORKSPACE_BYTES = 16;  // two doubles: min, max
hipError_t launch_render_annotated(const RenderParams& p, hipStream_t s);
