// Annotated LV video: overlay pane, title band and volume-curve strip of every frame, as RGB bytes.
//
// Reference: make_annotated_gif (src/visualization_utils.py:476-539), which builds each frame on the host from
// echonet_overlay(gray, seg, vis=False) (:346-437), a cv2.resize(INTER_NEAREST) and two matplotlib figures. The
// rules this file implements are stated in include/clasfv.h (clasfv_render_annotated) and restated in numpy
// in tests/render_oracle.py; DESIGN.md, "Annotated video", has the measurements.
//
// render_minmax_kernel: one workgroup; min and max of the finite volumes into the caller's workspace (exact
//   selections, so the order of the lanes does not matter).
// render_annotated_kernel: the call's output is ONE flat byte array (a row is 3 * Wo bytes, 1659 at Wo = 553:
//   no multiple of 4). A lane assembles a whole aligned 16-byte piece of it -- the six pixels it touches, 5 1/3
//   of them inside -- and stores it with one 16-byte store, so a wave writes 1 KiB of consecutive bytes. The
//   bytes before the first and after the last aligned piece (at most 15 each) are written one per lane by the
//   lanes after the last piece. Inside a piece the gray value is computed once per source pixel: neighbouring
//   output pixels of an upscaled pane share it. Pixel indices are 32-bit (the call's output is below 2^32 bytes;
//   clasfv_render_annotated refuses more) and decoded by two multiply-high divisions per piece.
// A pixel's value depends on (frame, row, column) and the inputs only: not on `first`, `count`, the alignment of
// out or the lane that writes it. Geometry and gray are float64 with nothing contracted into FMAs.
#include <math.h>

#include "clasfv.h"
#include "common.h"
#include "render.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int RD_THREADS = 256;
constexpr int RD_MAX_BLOCKS = 2048;  // 8 workgroups per CU; the pieces beyond are walked grid-stride
constexpr unsigned LIME = 50u | 205u << 8 | 50u << 16;  // matplotlib's limegreen, as R | G << 8 | B << 16

struct RenderArgs {
  const float* video;
  const uint8_t* masks;
  const uint8_t* truth;
  const double* volume;
  const uint8_t* title;
  const double* minmax;
  uint8_t* out;
  int64_t vstride;
  size_t plane;        // T * H * W
  double ify, ifx;     // source rows / columns per pane row / column
  double S, half;      // samples per strip column; half the line thickness
  unsigned head, n16, nedge, tail0;  // bytes before the first piece, pieces, head + tail bytes, first tail byte
  unsigned frame_px;   // (Hp + Ht + Hs) * Wo
  int T, H, W, first, Hp, Wo, Ht, Hs, label;
  FastDiv div_frame, div_wo;
};

__device__ inline bool finite(double v) { return fabs(v) < INFINITY; }

__global__ __launch_bounds__(RD_THREADS) void render_minmax_kernel(const double* __restrict__ volume, int64_t stride,
                                                                   int T, double* __restrict__ out) {
  __shared__ double s_lo[RD_THREADS / 64], s_hi[RD_THREADS / 64];
  double lo = INFINITY, hi = -INFINITY;  // lo > hi: no finite volume
  for (int k = threadIdx.x; k < T; k += RD_THREADS) {
    const double v = volume[(int64_t)k * stride];
    if (finite(v)) lo = v < lo ? v : lo, hi = v > hi ? v : hi;
  }
  for (int o = 32; o; o >>= 1) {
    const double l = __shfl_xor(lo, o), h = __shfl_xor(hi, o);
    lo = l < lo ? l : lo, hi = h > hi ? h : hi;
  }
  if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo, s_hi[threadIdx.x >> 6] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < RD_THREADS / 64; ++w) lo = s_lo[w] < lo ? s_lo[w] : lo, hi = s_hi[w] > hi ? s_hi[w] : hi;
    out[0] = lo, out[1] = hi;
  }
}

// floor(255 * clip(x, 0, 1)); a NaN gives 0
__device__ inline unsigned quantise(double x) {
  x = x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0;
  return (unsigned)(255.0 * x);
}

struct Painter {
  const RenderArgs& a;
  double yhi, sy;    // strip: value of row 0's top edge, rows per unit
  bool curve;        // the video has a finite volume
  // the row being painted (set_row): what changes only with (frame, row) is worked out once per row of a piece
  int kind;          // 0: pane, 1: title band, 2: strip
  int frame;         // video frame
  size_t base;       // pane: index of the source row's first pixel in a (T,H,W) plane
  const uint8_t* band_row;  // title: the row's bytes, or nullptr
  double r0, r1, di; // strip: the row's edges r and r + 1; the frame as a double
  int prev_sc;       // pane: source column of prev_px (-1: none)
  unsigned prev_px;

  __device__ explicit Painter(const RenderArgs& args) : a(args) {
    const double vmin = a.minmax[0], vmax = a.minmax[1];
    curve = vmin <= vmax;
    const double ylo = vmin - 100.0;
    yhi = vmax + 100.0;
    sy = (double)a.Hs / (yhi - ylo);
  }

  __device__ void set_row(int f, int row) {
    frame = a.first + f;
    if (row < a.Hp) {
      int sr = (int)floor((double)row * a.ify);
      sr = sr < a.H - 1 ? sr : a.H - 1;
      kind = 0, base = ((size_t)frame * a.H + sr) * a.W, prev_sc = -1;
    } else if (row - a.Hp < a.Ht) {
      kind = 1, band_row = a.title ? a.title + (size_t)(row - a.Hp) * a.Wo * 3 : nullptr;
    } else {
      kind = 2, r0 = (double)(row - a.Hp - a.Ht), r1 = r0 + 1.0, di = (double)frame;
    }
  }

  __device__ unsigned pane(int col) {
    int sc = (int)floor((double)col * a.ifx);
    sc = sc < a.W - 1 ? sc : a.W - 1;
    if (sc != prev_sc) {  // neighbouring pixels of an upscaled pane share their source pixel
      prev_sc = sc;
      const size_t src = base + sc;
      const double g = ((double)a.video[src] * 0.2989 + (double)a.video[a.plane + src] * 0.5870) +
                       (double)a.video[2 * a.plane + src] * 0.1140;
      const bool m = (int)a.masks[src] == a.label;
      bool fp = m, fn = false;  // R and G lifted; B lifted
      if (a.truth) {
        const bool t = (int)a.truth[src] == a.label;
        fp = m && !t, fn = !m && t;
      }
      const unsigned q = quantise(g);
      const unsigned lifted = (fp || fn) ? quantise(g + 0.3) : q;
      const unsigned rg = fp ? lifted : q, b = fn ? lifted : q;
      prev_px = rg | rg << 8 | b << 16;
    }
    return prev_px;
  }

  __device__ unsigned band(int col) const {
    if (!band_row) return 0;
    const uint8_t* t = band_row + 3 * col;
    return (unsigned)t[0] | (unsigned)t[1] << 8 | (unsigned)t[2] << 16;
  }

  // Column x of the strip row: is the row met by a drawable segment's widened span over the column?
  __device__ unsigned strip(int x) const {
    if (!curve) return 0;
    const double A = (double)x * a.S;
    double B = (double)(x + 1) * a.S;
    B = B < di ? B : di;
    if (!(A <= B)) return 0;
    int k1 = (int)ceil(B) - 1;
    k1 = k1 < frame - 1 ? k1 : frame - 1;
    bool on = false;
    for (int k = (int)floor(A); k <= k1; ++k) {
      const double v0 = a.volume[(int64_t)k * a.vstride], v1 = a.volume[(int64_t)(k + 1) * a.vstride];
      if (!(finite(v0) && finite(v1))) continue;
      const double dk = (double)k, dk1 = dk + 1.0, dv = v1 - v0;
      const double ta = dk > A ? dk : A, tb = dk1 < B ? dk1 : B;
      const double va = v0 + (ta - dk) * dv, vb = v0 + (tb - dk) * dv;
      const double ya = (yhi - va) * sy, yb = (yhi - vb) * sy;
      const double top = (ya < yb ? ya : yb) - a.half, bot = (ya > yb ? ya : yb) + a.half;
      on |= r1 > top && r0 <= bot;
    }
    return on ? LIME : 0u;
  }

  __device__ unsigned pixel(int col) { return kind == 0 ? pane(col) : kind == 1 ? band(col) : strip(col); }
};

__global__ __launch_bounds__(RD_THREADS) void render_annotated_kernel(const RenderArgs a) {
  Painter paint(a);
  const int FH = a.Hp + a.Ht + a.Hs;
  const unsigned nwork = a.n16 + a.nedge, stride = gridDim.x * RD_THREADS;
  for (unsigned p = blockIdx.x * RD_THREADS + threadIdx.x; p < nwork; p += stride) {
    const bool piece = p < a.n16;
    unsigned byte0;
    if (piece) {
      byte0 = a.head + 16u * p;
    } else {
      const unsigned e = p - a.n16;
      byte0 = e < a.head ? e : a.tail0 + (e - a.head);
    }
    const unsigned q0 = byte0 / 3u, ch0 = byte0 - 3u * q0;
    int f = fdiv((int)q0, a.div_frame);
    const int rem = (int)(q0 - (unsigned)f * a.frame_px);
    int row = fdiv(rem, a.div_wo), col = rem - row * a.Wo;
    paint.set_row(f, row);
    if (!piece) {
      a.out[byte0] = (uint8_t)(paint.pixel(col) >> (8 * ch0));
      continue;
    }
    unsigned px[6];  // the pixels the piece touches; the sixth is inside with at least its first byte
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      px[j] = paint.pixel(col);
      if (++col == a.Wo && j < 5) {
        col = 0;
        if (++row == FH) row = 0, ++f;
        paint.set_row(f, row);
      }
    }
    const u64 w0 = (u64)px[0] | (u64)px[1] << 24 | (u64)px[2] << 48;
    const u64 w1 = (u64)(px[2] >> 16) | (u64)px[3] << 8 | (u64)px[4] << 32 | (u64)px[5] << 56;
    const u64 w2 = (u64)(px[5] >> 8);
    u64 lo = w0, hi = w1;
    if (ch0) {
      const unsigned sh = 8 * ch0;
      lo = (w0 >> sh) | (w1 << (64 - sh));
      hi = (w1 >> sh) | (w2 << (64 - sh));
    }
    *reinterpret_cast<uint4*>(a.out + byte0) =
        uint4{(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
  }
}

}  // namespace

hipError_t launch_render_annotated(const RenderParams& p, hipStream_t s) {
  const int FH = p.Hp + p.Ht + p.Hs;
  const uint64_t total = (uint64_t)p.count * FH * p.Wo * 3;
  if (total == 0 || total >> 32 || (uint64_t)p.H * p.W >> 31) return hipErrorInvalidValue;  // refused by the caller first
  hipLaunchKernelGGL(render_minmax_kernel, dim3(1), dim3(RD_THREADS), 0, s, p.volume, p.vstride, p.T, p.workspace);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  RenderArgs a;
  a.video = p.video, a.masks = p.masks, a.truth = p.truth, a.volume = p.volume, a.title = p.title;
  a.minmax = p.workspace, a.out = p.out, a.vstride = p.vstride;
  a.plane = (size_t)p.T * p.H * p.W;
  a.ify = 1.0 / ((double)p.Hp / (double)p.H);
  a.ifx = 1.0 / ((double)p.Wo / (double)p.W);
  a.S = (double)(p.T + 1) / (double)p.Wo;
  a.half = p.thickness / 2.0;
  unsigned head = (unsigned)((16 - ((uintptr_t)p.out & 15)) & 15);
  if (head > total) head = (unsigned)total;
  a.head = head;
  a.n16 = (unsigned)((total - head) / 16);
  a.tail0 = head + 16u * a.n16;
  a.nedge = head + (unsigned)(total - a.tail0);
  a.frame_px = (unsigned)FH * (unsigned)p.Wo;
  a.T = p.T, a.H = p.H, a.W = p.W, a.first = p.first, a.Hp = p.Hp, a.Wo = p.Wo, a.Ht = p.Ht, a.Hs = p.Hs;
  a.label = p.label;
  a.div_frame = fast_div(a.frame_px), a.div_wo = fast_div((unsigned)p.Wo);
  const uint64_t nwork = (uint64_t)a.n16 + a.nedge, blocks = (nwork + RD_THREADS - 1) / RD_THREADS;
  hipLaunchKernelGGL(render_annotated_kernel, dim3((unsigned)(blocks < RD_MAX_BLOCKS ? blocks : RD_MAX_BLOCKS)),
                     dim3(RD_THREADS), 0, s, a);
  return hipGetLastError();
}
