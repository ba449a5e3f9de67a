// Tracking: one frame pushed through a chain of motion fields, every intermediate frame kept.
//
// Reference: apply_sequence_deformation / get_deformed_label_forback (src/visualization_utils.py:58-130)
// warp a label or image frame by frame through the motion head's forward (channels 0,1) or backward
// (2,3) fields, grid_mode "nearest" for labels and "bilinear" for images. Step p of such a chain needs
// the whole plane of step p - 1, so a loop of warp launches writes every plane to HBM and reads it back.
//
// track_lds_kernel keeps the plane on the chip instead: one 1024-thread workgroup per (n, c) plane holds
// it in two LDS buffers of H * W floats that swap roles after every step (step p gathers from one and
// writes the other; one barrier per step orders the writes of step p before the gathers of step p + 1 and
// the gathers of step p before the writes of step p + 1). Per step it reads two motion floats per pixel
// from HBM (coalesced; the next step's are fetched into registers before this step's arithmetic, so the
// loads are in flight across the barrier) and writes each tracked frame to HBM once. The gathers are
// 32-bit LDS reads at data-dependent addresses of a row-major plane: a smooth flow keeps the 64 lanes of a
// wave within a few neighbouring rows, and no layout is conflict-free for an arbitrary one; the LDS writes
// are unit-stride. 2 * 20480 * 4 B is the whole 160 KiB of a CU, so the kernel has no static LDS.
//
// track_step_kernel is the same step from HBM to HBM, one launch per step, over the whole chip: for planes
// that do not fit (224 x 224) and, by default, for every plane above CLASFV_TRACK_LDS_AUTO_PIXELS -- one CU
// advances a plane by about 1 ns per pixel and step (VALU-bound), and above a few thousand pixels that is
// more than a launch costs (measured: DESIGN.md, "Tracking"). Both compute a step exactly as warp_kernel
// (plumbing.hip) does, bit for bit; nearest mode rounds the same clipped source coordinate half to even
// (PyTorch's CPU kernel: nearbyint) and gathers.
#include "common.h"
#include "track.h"
#include "warp_math.h"

// As in plumbing.hip: every fused multiply-add is written out (fmaf); nothing else may be contracted.
#pragma clang fp contract(off)

namespace {

constexpr int TRACK_THREADS = 1024;
constexpr int TRACK_MAX_DEVICES = 64;  // devices whose LDS attribute is remembered; beyond, it is set per launch
constexpr int TRACK_PPT = (CLASFV_TRACK_LDS_MAX_PIXELS + TRACK_THREADS - 1) / TRACK_THREADS;  // pixels per thread
constexpr size_t TRACK_LDS_MAX = 2 * sizeof(float) * (size_t)CLASFV_TRACK_LDS_MAX_PIXELS;
static_assert(TRACK_LDS_MAX <= 160 * 1024, "two planes of CLASFV_TRACK_LDS_MAX_PIXELS floats must fit one CU's LDS");

// Where pixel (i, j) displaced by (fx, fy) samples its source plane: the arithmetic of warp_kernel, FMAs
// written out. Nearest mode keeps only the offset of the rounded coordinate (the border clip keeps it in range).
template <int MODE>
struct Taps {
  int o;                       // y0 * W + x0 (bilinear) or y * W + x (nearest)
  float wnw, wne, wsw, wse;    // corner weights
  bool in_x1, in_y1;           // x0 + 1 < W, y0 + 1 < H: corners outside read as 0
  __device__ Taps(int i, int j, int H, int W, float fx, float fy) {
    const float sx = (float)W * 0.5f, sy = (float)H * 0.5f;
    const float gx = linspace_pm1(j, W) + fx;
    const float gy = linspace_pm1(i, H) + fy;
    const float ix = fminf((float)(W - 1), fmaxf(fmaf(gx + 1.f, sx, -0.5f), 0.f));
    const float iy = fminf((float)(H - 1), fmaxf(fmaf(gy + 1.f, sy, -0.5f), 0.f));
    if constexpr (MODE == CLASFV_TRACK_NEAREST) {
      o = (int)rintf(iy) * W + (int)rintf(ix);
      wnw = wne = wsw = wse = 0.f;
      in_x1 = in_y1 = false;
    } else {
      const float fx0 = floorf(ix), fy0 = floorf(iy);
      const int x0 = (int)fx0, y0 = (int)fy0;
      const float we = ix - fx0, ee = (fx0 + 1.f) - ix, wn = iy - fy0, ws = (fy0 + 1.f) - iy;
      wnw = ws * ee, wne = ws * we, wsw = wn * ee, wse = wn * we;
      in_x1 = x0 + 1 < W, in_y1 = y0 + 1 < H;
      o = y0 * W + x0;
    }
  }
  __device__ float sample(const float* src, int W) const {
    if constexpr (MODE == CLASFV_TRACK_NEAREST) return src[o];
    const float vnw = src[o];
    const float vne = in_x1 ? src[o + 1] : 0.f;
    const float vsw = in_y1 ? src[o + W] : 0.f;
    const float vse = (in_x1 && in_y1) ? src[o + W + 1] : 0.f;
    return fmaf(vse, wse, fmaf(vsw, wsw, fmaf(vne, wne, vnw * wnw)));
  }
};

// One workgroup per (n, c) plane; `frame` = N * C * H * W floats between two output frames.
template <int MODE>
__global__ __launch_bounds__(TRACK_THREADS) void track_lds_kernel(const float* __restrict__ img, int C, int H, int W,
                                                                  const float* __restrict__ motion, int64_t m_sn,
                                                                  int64_t m_sc, int64_t m_st, int t0, int t_step, int P,
                                                                  size_t frame, FastDiv div_w, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float planes[];
  const int HW = H * W;
  const int nc = blockIdx.x, n = nc / C;
  float* cur = planes;
  float* nxt = planes + HW;
  const float* mp = motion + n * m_sn + t0 * m_st;
  float* o = out + (size_t)nc * HW;
  float mx[TRACK_PPT], my[TRACK_PPT];
#pragma unroll
  for (int k = 0; k < TRACK_PPT; ++k) {
    const int pix = threadIdx.x + k * TRACK_THREADS;
    if (pix < HW) {
      cur[pix] = img[(size_t)nc * HW + pix];
      mx[k] = mp[pix];
      my[k] = mp[m_sc + pix];
    }
  }
  __syncthreads();
  for (int p = 0; p < P; ++p) {
    // Opaque copies of H and W per step: otherwise the compiler hoists every pixel's row, column and
    // linspace values out of this loop (60 more live registers beside the 40 of mx, my) and spills.
    int Hp = H, Wp = W;
    asm volatile("" : "+s"(Hp), "+s"(Wp));
    const bool more = p + 1 < P;
    const float* mnext = more ? mp + t_step * m_st : mp;
#pragma unroll
    for (int k = 0; k < TRACK_PPT; ++k) {
      const int pix = threadIdx.x + k * TRACK_THREADS;
      if (pix < HW) {
        const float fx = mx[k], fy = my[k];
        if (more) {  // the next step's flow: in flight during this step's arithmetic and the barrier
          mx[k] = mnext[pix];
          my[k] = mnext[m_sc + pix];
        }
        const int i = fdiv(pix, div_w), j = pix - i * Wp;  // a per-lane division by W costs as much as the sampling
        const float v = Taps<MODE>(i, j, Hp, Wp, fx, fy).sample(cur, Wp);
        nxt[pix] = v;
        o[pix] = v;
      }
    }
    __syncthreads();
    float* t = cur;
    cur = nxt;
    nxt = t;
    mp = mnext;
    o += frame;
  }
}

// One step from HBM to HBM, as warp_kernel: the taps of a pixel serve all C channels. `motion` is the step's
// frame, src the previous output frame (img for step 0), dst the next; they never overlap.
template <int MODE>
__global__ void track_step_kernel(const float* __restrict__ src, int N, int C, int H, int W,
                                  const float* __restrict__ motion, int64_t m_sn, int64_t m_sc,
                                  float* __restrict__ dst) {
  const size_t HW = (size_t)H * W;
  const size_t total = (size_t)N * HW;
  for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
    const int n = (int)(g / HW);
    const int pix = (int)(g - (size_t)n * HW);
    const int i = pix / W, j = pix - i * W;
    const float* mp = motion + n * m_sn + pix;
    const Taps<MODE> taps(i, j, H, W, mp[0], mp[m_sc]);
    for (int c = 0; c < C; ++c) {
      const size_t plane = ((size_t)n * C + c) * HW;
      dst[plane + pix] = taps.sample(src + plane, W);
    }
  }
}

template <int MODE>
hipError_t track_launch(const float* img, int N, int C, int H, int W, const float* motion, int64_t m_sn, int64_t m_sc,
                        int64_t m_st, int t0, int t_step, int P, bool lds, float* out, hipStream_t s) {
  const size_t HW = (size_t)H * W;
  const size_t frame = (size_t)N * C * HW;
  if (lds) {
    const size_t lds_bytes = 2 * sizeof(float) * HW;
    if (lds_bytes > 64 * 1024) {
      // The default limit on dynamic LDS is 64 KiB; the attribute belongs to the current device, so it is raised
      // once per device and instantiation, to all the kernel may ask. Two threads racing here both set it.
      static bool attr[TRACK_MAX_DEVICES] = {};
      int dev = 0;
      hipError_t e = hipGetDevice(&dev);
      if (e != hipSuccess) return e;
      if (dev < 0 || dev >= TRACK_MAX_DEVICES || !attr[dev]) {
        e = hipFuncSetAttribute((const void*)track_lds_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)TRACK_LDS_MAX);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < TRACK_MAX_DEVICES) attr[dev] = true;
      }
    }
    hipLaunchKernelGGL(track_lds_kernel<MODE>, dim3(N * C), dim3(TRACK_THREADS), lds_bytes, s, img, C, H, W, motion,
                       m_sn, m_sc, m_st, t0, t_step, P, frame, fast_div((unsigned)W), out);
    return hipGetLastError();
  }
  const size_t total = (size_t)N * HW;
  size_t blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  for (int p = 0; p < P; ++p) {
    const float* src = p ? out + (size_t)(p - 1) * frame : img;
    hipLaunchKernelGGL(track_step_kernel<MODE>, dim3((unsigned)blocks), dim3(256), 0, s, src, N, C, H, W,
                       motion + (t0 + (int64_t)p * t_step) * m_st, m_sn, m_sc, out + (size_t)p * frame);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_track(const float* img, int N, int C, int H, int W, const float* motion, int64_t m_sn, int64_t m_sc,
                        int64_t m_st, int t0, int t_step, int P, int mode, float* out, hipStream_t s) {
  // One CU advances a plane by about 1 ns per pixel and step; a launch of the step kernel, which spreads the
  // plane over the chip, costs about 3 us ("Tracking"): the LDS path is the default only for planes
  // small enough to win that trade, and for every plane that fits under CLASFV_TRACK_FORCE_LDS.
  const size_t HW = (size_t)H * W;
  const bool fits = HW <= CLASFV_TRACK_LDS_MAX_PIXELS;
  const bool lds = fits && !(mode & CLASFV_TRACK_FORCE_STEPS) &&
                   ((mode & CLASFV_TRACK_FORCE_LDS) || HW <= CLASFV_TRACK_LDS_AUTO_PIXELS);
  if ((mode & ~(CLASFV_TRACK_FORCE_STEPS | CLASFV_TRACK_FORCE_LDS)) == CLASFV_TRACK_NEAREST)
    return track_launch<CLASFV_TRACK_NEAREST>(img, N, C, H, W, motion, m_sn, m_sc, m_st, t0, t_step, P, lds, out, s);
  return track_launch<CLASFV_TRACK_BILINEAR>(img, N, C, H, W, motion, m_sn, m_sc, m_st, t0, t_step, P, lds, out, s);
}
