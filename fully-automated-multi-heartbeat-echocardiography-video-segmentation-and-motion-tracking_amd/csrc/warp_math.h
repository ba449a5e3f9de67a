// Device arithmetic shared by the warp kernels (plumbing.hip) and the tracking kernels (track.hip): one
// copy, because both are pinned bit for bit to PyTorch's CPU kernels.
#pragma once
#include <hip/hip_runtime.h>

// torch.linspace(-1, 1, n) on the CPU: step = 2/(n-1); first half fma(step, i, -1), second half
// fma(-step, n-1-i, 1) (the kernel is built with FMA contraction).
__device__ inline float linspace_pm1(int i, int n) {
  if (n == 1) return -1.f;
  const float step = 2.0f / (float)(n - 1);
  return (i < n / 2) ? fmaf(step, (float)i, -1.f) : fmaf(-step, (float)(n - 1 - i), 1.f);
}
