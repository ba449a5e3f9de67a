// LV geometry: area, long-axis length, ten disk radii and Simpson volume of every frame of a mask video.
//
// Reference: get2dPucks + computeSimpsonVolume (src/utils/echo_utils.py:259-385), which the reference runs on
// the ED / ES frames for the EF (src/fuse_utils.py:105-148) and on every frame for the volume curve
// (src/visualization_utils.py:487-493). The rules are restated in include/clasfv.h (clasfv_lv_geometry) and in
// DESIGN.md, "LV geometry"; the host functions of echo.py are the oracle.
//
// lv_geometry_kernel: one 1024-thread workgroup per frame, one launch per batch. The frame is read from HBM
// once, as one flag byte per pixel in LDS (bit 0: the pixel equals `label`; bit 1, added by the rim scan: its
// 4-neighbourhood is mixed); every later scan reads LDS and does arithmetic for rim pixels only. In order:
//   1. stage + moments: n, sum i, sum j, sum i^2, sum ij, sum j^2 in 64-bit integers (per thread, then per wave
//      by shuffles, then one LDS integer atomic per wave and moment);
//   2. thread 0: n * sum(ab) - sum(a) * sum(b) exactly in 128-bit integers -> covariance (one rounding, then
//      the spacings) -> closed-form eigenvectors of the symmetric 2 x 2 matrix, oriented as the reference;
//   3. rim scan: marks the rim and takes min / max of the major-axis coordinate (doubles as order-preserving
//      64-bit keys, integer max);
//   4. the slab medians by exact selection: |minor coordinate| is a non-negative double, whose bit pattern is
//      monotone, so a radix select from the top digit down finds, per slab, the element of a given rank. A
//      digit is 4 bits (16 scans): ten slabs of 16 counters are 640 B, and at CLASFV_LV_MAX_PIXELS the frame
//      leaves 1 KiB of the CU's LDS for all state. Each scan recomputes a rim pixel's coordinates and slab
//      (the same instructions every time, so the same values). The rim scan also lists the rim pixels in the
//      LDS the frame leaves free (up to an entry per pixel: every 112 x 112 frame fits whatever its rim), and
//      the scans then take one listed pixel per lane; a frame with more rim pixels than entries (a checkerboard
//      above ~32,500 pixels, any frame near the size limit) is scanned from its flag bytes instead, rim pixel
//      by rim pixel within a lane -- slower, never capped;
//   5. one more scan for the upper middle element of an even slab (the least value above the lower middle one,
//      unless that value occurs often enough to be both), then radii, length and volume by threads 0..9.
// Only integer atomics and exact selections cross threads, so a frame's results do not depend on thread order,
// on F or on the frame's place in the batch. Everything is float64; nothing is contracted into FMAs.
#include <math.h>

#include "clasfv.h"
#include "common.h"
#include "lvgeom.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int LV_THREADS = 1024;
constexpr int LV_NP = CLASFV_LV_NPUCKS;
constexpr int LV_DIGIT = 4;                  // bits per radix pass
constexpr int LV_BINS = 1 << LV_DIGIT;
constexpr int LV_PASSES = 64 / LV_DIGIT;
constexpr int LV_STATE_BYTES = 1024;         // LvState, then the frame's flag bytes
constexpr int LV_MAX_DEVICES = 64;           // devices whose LDS attribute is remembered (as track.hip)
constexpr unsigned MEMBER = 1, RIM = 2;
constexpr unsigned RIM_X4 = RIM * 0x01010101u;

struct LvState {
  u64 mom[6];          // n, sum i, sum j, sum i*i, sum i*j, sum j*j over the member pixels
  u64 kmin_c, kmax;    // max of ~key and of key of the rim's major-axis coordinates (0: no rim pixel)
  unsigned nrim, pad;  // rim pixels counted by the rim scan
  double ci, cj;       // mean member coordinate
  double a00, a10;     // major axis (i, j components)
  double a01, a11;     // minor axis
  u64 sel[LV_NP];      // per slab: the digits of the selected value found so far; at the end the radius
  u64 next[LV_NP];     // per slab: least value above the selected one
  unsigned hist[LV_NP][LV_BINS];
};
static_assert(sizeof(LvState) <= LV_STATE_BYTES, "the state must fit beside a frame of CLASFV_LV_MAX_PIXELS bytes");
static_assert(LV_STATE_BYTES + CLASFV_LV_MAX_PIXELS <= 160 * 1024, "state and frame must fit one CU's LDS");
static_assert(CLASFV_LV_MAX_PIXELS % 4 == 0 && CLASFV_LV_STRIDE == LV_NP + 2, "layout");

// Order-preserving map of a finite double onto unsigned 64-bit integers, never 0 or ~0.
__device__ inline u64 key_of(double x) {
  const u64 b = (u64)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ inline double value_of(u64 k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__device__ inline u64 wave_sum(u64 v) {
  for (int o = 32; o; o >>= 1) v += (u64)__shfl_xor((long long)v, o);
  return v;
}
__device__ inline u64 wave_max(u64 v) {
  for (int o = 32; o; o >>= 1) {
    const u64 w = (u64)__shfl_xor((long long)v, o);
    v = w > v ? w : v;
  }
  return v;
}

// n * sab - sa * sb, exact in 128-bit integers; to double with one rounding when it is below 2^64 (every frame
// but a line of more than ~60000 pixels), with two otherwise.
__device__ double central_moment(u64 n, u64 sab, u64 sa, u64 sb) {
  const __int128 v = (__int128)n * (__int128)sab - (__int128)sa * (__int128)sb;
  const bool neg = v < 0;
  const unsigned __int128 u = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
  const u64 hi = (u64)(u >> 64), lo = (u64)u;
  double d = (double)lo;
  if (hi) d = (double)hi * 18446744073709551616.0 + d;
  return neg ? -d : d;
}

struct Proj {
  double sy, sx, ci, cj, a00, a10, a01, a11;
  __device__ double along(int i, int j) const { return ((double)i * sy - ci) * a00 + ((double)j * sx - cj) * a10; }
  __device__ double across(int i, int j) const { return ((double)i * sy - ci) * a01 + ((double)j * sx - cj) * a11; }
};

// Slab of x: k with cut[k] <= x < cut[k + 1] (numpy.digitize - 1); LV_NP for the pixel at cut[LV_NP] = hi.
__device__ inline int slab_of(double x, const double (&cut)[LV_NP + 1]) {
  int c = 0;
#pragma unroll
  for (int k = 0; k <= LV_NP; ++k) c += x >= cut[k] ? 1 : 0;
  return c - 1;
}

__global__ __launch_bounds__(LV_THREADS) void lv_geometry_kernel(const uint8_t* __restrict__ masks, int64_t F, int H,
                                                                 int W, int label, double sy, double sx,
                                                                 FastDiv div_w, int cap,
                                                                 int32_t* __restrict__ area,
                                                                 double* __restrict__ geom) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lv_lds[];
  LvState& st = *reinterpret_cast<LvState*>(lv_lds);
  unsigned char* px = lv_lds + LV_STATE_BYTES;
  const unsigned* px4 = reinterpret_cast<const unsigned*>(px);
  const int HW = H * W, words = (HW + 3) >> 2;
  unsigned* list = reinterpret_cast<unsigned*>(px + 4 * words);  // `cap` rim pixel indices
  const int tid = threadIdx.x;
  const bool lane0 = (tid & 63) == 0;

  for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
    __syncthreads();  // every thread is done with the previous frame's state
    for (int k = tid; k < (int)(sizeof(LvState) / sizeof(unsigned)); k += LV_THREADS)
      reinterpret_cast<unsigned*>(&st)[k] = 0;

    // 1. stage the frame as flag bytes (the tail of the last word as background); moments of the members
    const uint8_t* src = masks + f * (int64_t)HW;
    u64 n = 0, si = 0, sj = 0, sii = 0, sij = 0, sjj = 0;
    for (int p = tid; p < words * 4; p += LV_THREADS) {
      unsigned char m = 0;
      if (p < HW && (int)src[p] == label) {
        m = MEMBER;
        const int i = fdiv(p, div_w), j = p - i * W;
        n += 1, si += (u64)i, sj += (u64)j;
        sii += (u64)i * (u64)i, sij += (u64)i * (u64)j, sjj += (u64)j * (u64)j;
      }
      px[p] = m;
    }
    __syncthreads();
    n = wave_sum(n), si = wave_sum(si), sj = wave_sum(sj), sii = wave_sum(sii), sij = wave_sum(sij), sjj = wave_sum(sjj);
    if (lane0 && n) {
      atomicAdd(&st.mom[0], n), atomicAdd(&st.mom[1], si), atomicAdd(&st.mom[2], sj);
      atomicAdd(&st.mom[3], sii), atomicAdd(&st.mom[4], sij), atomicAdd(&st.mom[5], sjj);
    }
    __syncthreads();

    // 2. principal axes
    if (tid == 0) {
      n = st.mom[0], si = st.mom[1], sj = st.mom[2];
      area[f] = (int32_t)n;
      if (n >= 2) {
        const double dn = (double)n, den = dn * (dn - 1.0);
        const double cross = central_moment(n, st.mom[4], si, sj);
        const double vi = central_moment(n, st.mom[3], si, si) / den * (sy * sy);
        const double vj = central_moment(n, st.mom[5], sj, sj) / den * (sx * sx);
        double m0, m1;  // major axis
        if (cross == 0.0) {  // diagonal covariance: the coordinate axes; i first only when its variance is larger
          m0 = vi > vj ? 1.0 : 0.0, m1 = vi > vj ? 0.0 : 1.0;
          st.a01 = m1, st.a11 = m0;
        } else {
          const double b = cross / den * (sy * sx);
          const double t = (vi - vj) * 0.5, r = hypot(t, b);
          // eigenvector of the larger eigenvalue (vi + vj) / 2 + r, in the form without cancellation
          if (t >= 0.0) m0 = t + r, m1 = b;
          else m0 = b, m1 = r - t;
          const double h = hypot(m0, m1);
          m0 /= h, m1 /= h;
          if (m0 < 0.0) m0 = -m0, m1 = -m1;  // each axis points along its own coordinate
          st.a01 = -m1, st.a11 = m0;
        }
        st.a00 = m0, st.a10 = m1;
        st.ci = (double)si / dn * sy, st.cj = (double)sj / dn * sx;
      }
    }
    __syncthreads();
    n = st.mom[0];
    double* g = geom + f * CLASFV_LV_STRIDE;
    if (n < 2) {  // no member: (1, zeros); one member: (0, zeros)
      if (tid < CLASFV_LV_STRIDE) g[tid] = (tid == 0 && n == 0) ? 1.0 : 0.0;
      continue;
    }
    const Proj pr{sy, sx, st.ci, st.cj, st.a00, st.a10, st.a01, st.a11};

    // 3. the rim, and the extent of its major-axis coordinate. A neighbour's flag byte may gain its RIM bit
    // while it is read here: only its MEMBER bit is looked at, and a byte store does not touch that.
    u64 kmn = 0, kmx = 0;
    for (int p = tid; p < HW; p += LV_THREADS) {
      const int i = fdiv(p, div_w), j = p - i * W;
      const unsigned m = px[p] & MEMBER;
      const unsigned s = (px[i > 0 ? p - W : p] & MEMBER) + (px[i < H - 1 ? p + W : p] & MEMBER) +
                         (px[j > 0 ? p - 1 : p] & MEMBER) + (px[j < W - 1 ? p + 1 : p] & MEMBER);
      if (s != 4 * m) {
        px[p] = (unsigned char)(m | RIM);
        const unsigned e = atomicAdd(&st.nrim, 1u);
        if (e < (unsigned)cap) list[e] = (unsigned)p;
        const u64 k = key_of(pr.along(i, j));
        kmn = ~k > kmn ? ~k : kmn;
        kmx = k > kmx ? k : kmx;
      }
    }
    kmn = wave_max(kmn), kmx = wave_max(kmx);
    if (lane0 && kmx) atomicMax(&st.kmin_c, kmn), atomicMax(&st.kmax, kmx);
    __syncthreads();
    if (st.kmax == 0) {  // every pixel a member: no rim, nothing is defined
      if (tid < CLASFV_LV_STRIDE) g[tid] = __longlong_as_double(0x7ff8000000000000ll);
      continue;
    }
    // The later scans visit the rim pixels from the list, one pixel per lane, when all of them fit it (in any
    // order: only integer counts and exact minima come of them), else from the flag bytes, four per 32-bit load.
    const int nrim = (int)st.nrim;
    const bool listed = nrim <= cap;
    auto for_each_rim = [&](auto&& fn) {
      if (listed) {
        for (int e = tid; e < nrim; e += LV_THREADS) fn((int)list[e]);
      } else {
        for (int w = tid; w < words; w += LV_THREADS) {
          const unsigned v = px4[w];
          if (!(v & RIM_X4)) continue;
          for (int q = 0; q < 4; ++q)
            if ((v >> (8 * q)) & RIM) fn(4 * w + q);
        }
      }
    };
    const double lo = value_of(~st.kmin_c), hi = value_of(st.kmax);
    const double length = hi - lo, step = length / (double)LV_NP;
    double cut[LV_NP + 1];
#pragma unroll
    for (int k = 0; k < LV_NP; ++k) cut[k] = (double)k * step + lo;  // numpy.linspace's arithmetic
    cut[LV_NP] = hi;

    // 4. per slab, the element of rank (count - 1) / 2 of |minor coordinate|: radix select, top digit first
    unsigned count = 0, rank = 0, equal = 0;  // of slab tid (threads 0..9)
    for (int pass = 0; pass < LV_PASSES; ++pass) {
      const int shift = 64 - LV_DIGIT * (pass + 1);
      for_each_rim([&](int p) {
        const int i = fdiv(p, div_w), j = p - i * W;
        const int k = slab_of(pr.along(i, j), cut);
        if ((unsigned)k >= (unsigned)LV_NP) return;  // the pixel attaining hi is in no slab
        const u64 bits = (u64)__double_as_longlong(fabs(pr.across(i, j)));
        // the digits above this pass's agree with the selection so far (none in pass 0: 63 + 1 bits shifted out)
        if ((((bits ^ st.sel[k]) >> (shift + LV_DIGIT - 1)) >> 1) == 0)
          atomicAdd(&st.hist[k][(unsigned)(bits >> shift) & (LV_BINS - 1)], 1u);
      });
      __syncthreads();
      if (tid < LV_NP) {
        if (pass == 0) {
          for (int b = 0; b < LV_BINS; ++b) count += st.hist[tid][b];
          rank = count ? (count - 1) / 2 : 0;
          st.next[tid] = ~0ull;
        }
        if (count) {
          unsigned below = 0;
          int b = 0;
          for (; b < LV_BINS - 1; ++b) {
            const unsigned c = st.hist[tid][b];
            if (below + c > rank) break;
            below += c;
          }
          rank -= below;              // rank among the elements that share the digits so far
          equal = st.hist[tid][b];    // after the last pass: how often the selected value occurs
          st.sel[tid] |= (u64)b << shift;
        }
        for (int b = 0; b < LV_BINS; ++b) st.hist[tid][b] = 0;
      }
      __syncthreads();
    }

    // 5. the least value above the selected one (the upper middle element of an even slab, unless the selected
    // value itself occurs again at rank + 1)
    for_each_rim([&](int p) {
      const int i = fdiv(p, div_w), j = p - i * W;
      const int k = slab_of(pr.along(i, j), cut);
      if ((unsigned)k >= (unsigned)LV_NP) return;
      const u64 bits = (u64)__double_as_longlong(fabs(pr.across(i, j)));
      if (bits > st.sel[k]) atomicMin(&st.next[k], bits);
    });
    __syncthreads();
    if (tid < LV_NP) {
      double r = __longlong_as_double(0x7ff8000000000000ll);  // empty slab
      if (count) {
        r = __longlong_as_double((long long)st.sel[tid]);
        if (!(count & 1)) {
          const double up = rank + 1 < equal ? r : __longlong_as_double((long long)st.next[tid]);
          r = (r + up) / 2.0;
        }
      }
      g[1 + tid] = r;
      st.sel[tid] = (u64)__double_as_longlong(r);
    }
    __syncthreads();
    if (tid == 0) {
      double t[LV_NP];
      for (int k = 0; k < LV_NP; ++k) {
        const double r = __longlong_as_double((long long)st.sel[k]);
        t[k] = M_PI * r * r * length / (double)LV_NP;
      }
      // numpy.sum of ten doubles: eight partial sums pairwise, then the rest in order
      double v = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
      v += t[8];
      v += t[9];
      g[0] = length;
      g[1 + LV_NP] = v;
    }
  }
}

}  // namespace

hipError_t launch_lv_geometry(const uint8_t* masks, int64_t F, int H, int W, int label, double sy, double sx,
                              int32_t* area, double* geom, hipStream_t s) {
  const size_t HW = (size_t)H * W;
  if (HW > CLASFV_LV_MAX_PIXELS) return hipErrorInvalidValue;  // clasfv_lv_geometry refuses it first
  // the rim list takes the LDS the frame leaves free, up to an entry per pixel
  const size_t frame_bytes = (HW + 3) & ~(size_t)3, lds_max = LV_STATE_BYTES + CLASFV_LV_MAX_PIXELS;
  const size_t room = (lds_max - LV_STATE_BYTES - frame_bytes) / sizeof(unsigned);
  const int cap = (int)(room < HW ? room : HW);
  const size_t lds_bytes = LV_STATE_BYTES + frame_bytes + sizeof(unsigned) * (size_t)cap;
  if (lds_bytes > 64 * 1024) {
    // The default limit on dynamic LDS is 64 KiB; raised once per device, to all the kernel may ask (track.hip).
    static bool attr[LV_MAX_DEVICES] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= LV_MAX_DEVICES || !attr[dev]) {
      e = hipFuncSetAttribute((const void*)lv_geometry_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              LV_STATE_BYTES + CLASFV_LV_MAX_PIXELS);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < LV_MAX_DEVICES) attr[dev] = true;
    }
  }
  const unsigned grid = (unsigned)(F < 65536 ? F : 65536);
  hipLaunchKernelGGL(lv_geometry_kernel, dim3(grid), dim3(LV_THREADS), lds_bytes, s, masks, F, H, W, label, sy, sx,
                     fast_div((unsigned)W), cap, area, geom);
  return hipGetLastError();
}
