// Mask cleanup: keep the label-1 component of largest filled area and fill its small holes, frame by frame.
//
// Reference: cleanupBinary / cleanupSegmentation (src/utils/camus_validate.py:284-352), which the reference's
// validation loops apply to every network output. The rule is stated in include/clasfv.h (clasfv_fuse_votes,
// CLASFV_FUSE_CLEAN) and in DESIGN.md, "Mask cleanup"; tests/cleanup_oracle.py restates it twice on the host.
//
// cleanup_frames_kernel: one 1024-thread workgroup per frame, one launch per batch, after the fusion kernel
// on the same stream. The frame is read from HBM once into LDS, cleaned there, and only the pixels that
// change are stored back. LDS per pixel: one flag byte and one 16-bit label (3 B; a pixel index fits 16 bits
// because H * W <= CLASFV_CLEAN_MAX_PIXELS = 53248 < 65535).
//
// One primitive, label_components, serves the three steps of the rule: it labels the pixels that satisfy a
// predicate on their flag byte, under 4- or 8-connectivity, each component named by its least pixel index,
// and leaves the component's size in the label slot of that root pixel (whose flag byte gets ROOT).
//   a. every pixel points at its left neighbour if that one satisfies the predicate too, else at itself; then
//      ceil(log2 W) rounds of pointer jumping bring every pixel of a row run to the run's first pixel;
//   b. union-find over the row above: a pixel is united with N (8-connectivity: else with NW and NE). A union
//      links the larger root below the smaller with a 16-bit atomic min, retried until it meets a root (the
//      lock-free union of Allegretti, Bolelli, Grana, "Optimized Block-Based Algorithms to Label Connected
//      Components on GPUs", 2019). A parent is always a smaller index, so a tree's root is its least pixel
//      and the finished forest is the same whatever the order of the unions;
//   c. every pixel reads its root; the roots count themselves, the others add 1 to their root's slot.
// There is no per-hop iteration: a one-pixel-wide spiral costs one pass like any other frame, with longer
// root walks. The ISA has no 16-bit LDS atomics: the min is a compare-and-swap loop on the containing
// 32-bit word, the size count a 32-bit add of 1 or 1 << 16 (a size is at most 53248, so no carry leaves the
// half). Phases that store plain 16-bit labels and phases that use word atomics are separated by barriers.
//
// Per frame: (1) members 8-connected; the largest plain area A. (2) A component of n pixels has filled area
// at most ub(n) = n for n < 8 (a hole pixel's eight neighbours are in the frame and are component or hole
// pixels, so a hole needs a ring of >= 8) and n + (n - 4)^2 / 4 otherwise (holes of r rows and c columns
// have >= 2 (r + 2) and >= 2 (c + 2) ring pixels: the first and last pixel of every row and column of their
// dilation). Candidates are the components with ub(n) >= A, visited in index order and skipped once ub(n)
// cannot beat the best filled area so far. A single candidate (every ordinary frame) is kept at no further
// cost. Else, per candidate with n >= 8: flag its pixels, label the unflagged pixels 8-connected, mark the
// roots of components with a pixel on the frame edge, filled area = H * W - pixels of marked components;
// then the members are labelled again (the one label array was reused). (3) The kept component is flagged,
// the other pixels are labelled 4-connected, and components smaller than holesize are filled.
// Only integer LDS atomics (min, add, max) and block-wide reductions cross threads; every racing plain
// access is a 16-bit label that only ever moves to another ancestor, or a flag byte rewritten with the same
// bit. A frame's bytes do not depend on thread order, on F or on the frame's place in the batch.
#include "clasfv.h"
#include "cleanup.h"
#include "common.h"

namespace {

typedef unsigned short u16;

constexpr int CL_THREADS = 1024;
constexpr int CL_STATE_BYTES = 256;   // ClState, then the labels, then the flag bytes
constexpr int CL_GRID_MAX = 4096;     // workgroups per launch; the grid loops over further frames
constexpr int CL_MAX_DEVICES = 64;    // devices whose LDS attribute is remembered (as track.hip)
constexpr unsigned NONE = 0xFFFFu;    // label of a pixel outside the predicate; "no root" in searches
constexpr unsigned MEMBER = 1, KEPT = 2, INR = 4, ROOT = 8, EDGE = 16;

struct ClState {
  unsigned acc;  // the block-wide reduction in flight
};
static_assert(sizeof(ClState) <= CL_STATE_BYTES, "state");
static_assert(CL_STATE_BYTES + 3 * CLASFV_CLEAN_MAX_PIXELS <= 160 * 1024, "labels and flags must fit one CU's LDS");
static_assert(CLASFV_CLEAN_MAX_PIXELS < 0xFFFF && CLASFV_CLEAN_MAX_PIXELS % 4 == 0, "a pixel index is a 16-bit label");

enum { RED_SUM, RED_MIN, RED_MAX };

// Block-wide integer reduction; every thread gets the result. The leading barrier also ends the phase before.
template <int OP>
__device__ unsigned block_reduce(ClState& st, unsigned v, int tid) {
  for (int o = 32; o; o >>= 1) {
    const unsigned w = (unsigned)__shfl_xor((int)v, o);
    v = OP == RED_SUM ? v + w : OP == RED_MIN ? (w < v ? w : v) : (w > v ? w : v);
  }
  __syncthreads();
  if (tid == 0) st.acc = OP == RED_MIN ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  if ((tid & 63) == 0) {
    if (OP == RED_SUM) atomicAdd(&st.acc, v);
    else if (OP == RED_MIN) atomicMin(&st.acc, v);
    else atomicMax(&st.acc, v);
  }
  __syncthreads();
  return st.acc;
}

__device__ inline unsigned find_root(const volatile u16* L, unsigned x) {
  for (;;) {
    const unsigned l = L[x];
    if (l == x) return x;
    x = l;  // l < x: the walk ends
  }
}

// L[i] = min(L[i], v) atomically; returns the value before.
__device__ inline unsigned atomic_min16(u16* L, unsigned i, unsigned v) {
  unsigned* w = reinterpret_cast<unsigned*>(L) + (i >> 1);
  const unsigned sh = (i & 1) * 16;
  unsigned old = *reinterpret_cast<volatile unsigned*>(w);
  for (;;) {
    const unsigned cur = (old >> sh) & 0xFFFFu;
    if (cur <= v) return cur;
    const unsigned got = atomicCAS(w, old, (old & ~(0xFFFFu << sh)) | (v << sh));
    if (got == old) return cur;
    old = got;
  }
}

__device__ inline void unite(u16* L, unsigned a, unsigned b) {
  for (;;) {
    a = find_root(L, a), b = find_root(L, b);
    if (a == b) return;
    if (a < b) { const unsigned t = a; a = b; b = t; }
    const unsigned old = atomic_min16(L, a, b);
    if (old == a) return;  // a was a root and now hangs below b
    a = old;               // a had got a parent meanwhile: that tree is united with b's next
  }
}

struct Frame {
  u16* L;
  unsigned char* px;
  int H, W, HW, HWp;
  FastDiv div_w;
  __device__ bool is(int p, unsigned mask, unsigned want) const { return (px[p] & mask) == want; }
  // after label_components, for a pixel of the predicate:
  __device__ unsigned root_of(int p) const { return (px[p] & ROOT) ? (unsigned)p : (unsigned)L[p]; }
  __device__ unsigned size_of(unsigned r) const { return L[r]; }
};

// Labels the pixels with (flag & mask) == want; see the file comment. Ends with a barrier.
__device__ void label_components(const Frame& fr, unsigned mask, unsigned want, bool conn8, int tid) {
  u16* L = fr.L;
  volatile u16* Lv = fr.L;
  const int W = fr.W, HW = fr.HW;
  for (int p = tid; p < fr.HWp; p += CL_THREADS) {
    unsigned l = NONE;
    if (p < HW) {
      const unsigned m = fr.px[p];
      if ((m & mask) == want) {
        const int j = p - fdiv(p, fr.div_w) * W;
        l = (j > 0 && fr.is(p - 1, mask, want)) ? (unsigned)(p - 1) : (unsigned)p;
      }
      if (m & (ROOT | EDGE)) fr.px[p] = (unsigned char)(m & ~(ROOT | EDGE));
    }
    L[p] = (u16)l;
  }
  __syncthreads();
  // a. row runs by pointer jumping, in place: a racing read sees the old or the new parent, both in the run
  for (int s = 1; s < W; s <<= 1) {
    for (int p = tid; p < HW; p += CL_THREADS) {
      const unsigned l = Lv[p];
      if (l == NONE || l == (unsigned)p) continue;
      const unsigned l2 = Lv[l];
      if (l2 != l) Lv[p] = (u16)l2;
    }
    __syncthreads();
  }
  // b. unions with the row above (every store of this phase is a word atomic)
  for (int p = W + tid; p < HW; p += CL_THREADS) {
    if (!fr.is(p, mask, want)) continue;
    const int j = p - fdiv(p, fr.div_w) * W, q = p - W;
    const bool n = fr.is(q, mask, want);
    const bool nw = j > 0 && fr.is(q - 1, mask, want), ne = j < W - 1 && fr.is(q + 1, mask, want);
    if (n) {
      // joined already through the left neighbour when p - 1, q - 1 and q all satisfy the predicate
      if (!(nw && fr.is(p - 1, mask, want))) unite(L, (unsigned)p, (unsigned)q);
    } else if (conn8) {
      if (nw) unite(L, (unsigned)p, (unsigned)(q - 1));
      if (ne) unite(L, (unsigned)p, (unsigned)(q + 1));
    }
  }
  __syncthreads();
  // c. roots (no root changes any more, so a racing read only finds a shorter walk), then sizes
  for (int p = tid; p < HW; p += CL_THREADS) {
    if (Lv[p] == NONE) continue;
    const unsigned r = find_root(Lv, (unsigned)p);
    if (r != (unsigned)p) Lv[p] = (u16)r;
  }
  __syncthreads();
  for (int p = tid; p < HW; p += CL_THREADS)
    if (Lv[p] == (unsigned)p) fr.px[p] |= ROOT;
  __syncthreads();
  for (int p = tid; p < HW; p += CL_THREADS)
    if (fr.px[p] & ROOT) L[p] = 1;
  __syncthreads();
  for (int p = tid; p < HW; p += CL_THREADS) {
    if ((fr.px[p] & ROOT) || !fr.is(p, mask, want)) continue;
    const unsigned r = Lv[p];
    atomicAdd(reinterpret_cast<unsigned*>(L) + (r >> 1), 1u << ((r & 1) * 16));
  }
  __syncthreads();
}

// Upper bound of the filled area of a component of n pixels (file comment).
__device__ inline unsigned filled_bound(unsigned n) { return n < 8 ? n : n + ((n - 4) * (n - 4) + 3) / 4; }

__global__ __launch_bounds__(CL_THREADS) void cleanup_frames_kernel(uint8_t* __restrict__ frames, int64_t F, int H, int W,
                                                                    int holesize, FastDiv div_w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
  ClState& st = *reinterpret_cast<ClState*>(cl_lds);
  const int HW = H * W, HWp = (HW + 3) & ~3;
  const Frame fr{reinterpret_cast<u16*>(cl_lds + CL_STATE_BYTES), cl_lds + CL_STATE_BYTES + 2 * HWp, H, W, HW, HWp, div_w};
  const int tid = threadIdx.x;

  for (int64_t f = blockIdx.x; f < F; f += gridDim.x) {
    uint8_t* img = frames + f * (int64_t)HW;
    __syncthreads();  // every thread is done with the previous frame's LDS
    unsigned any = 0;
    for (int p = tid; p < HWp; p += CL_THREADS) {
      const unsigned m = (p < HW && img[p] == 1) ? MEMBER : 0;
      fr.px[p] = (unsigned char)m;
      any |= m;
    }
    if (!block_reduce<RED_MAX>(st, any, tid)) continue;  // no member: the frame stays as it is

    // 1. members, 8-connected; the largest plain area
    label_components(fr, MEMBER, MEMBER, true, tid);
    unsigned v = 0, c = 0;
    for (int p = tid; p < HW; p += CL_THREADS)
      if (fr.px[p] & ROOT) v = max(v, fr.size_of(p));
    const unsigned amax = block_reduce<RED_MAX>(st, v, tid);
    for (int p = tid; p < HW; p += CL_THREADS)
      if ((fr.px[p] & ROOT) && filled_bound(fr.size_of(p)) >= amax) ++c;
    const unsigned ncand = block_reduce<RED_SUM>(st, c, tid);

    // 2. the candidate of greatest filled area, the first in index order among equals
    unsigned best_f = 0, best_r = NONE;
    for (int cur = -1;;) {
      v = NONE;
      for (int p = tid; p < HW; p += CL_THREADS) {
        if (p <= cur || !(fr.px[p] & ROOT)) continue;
        const unsigned ub = filled_bound(fr.size_of(p));
        if (ub >= amax && ub > best_f) {
          v = (unsigned)p;
          break;  // a thread's pixels ascend
        }
      }
      const unsigned r = block_reduce<RED_MIN>(st, v, tid);
      if (r >= NONE) break;
      if (ncand == 1) {
        best_r = r;
        break;
      }
      const unsigned n = fr.size_of(r);
      unsigned filled = n;
      if (n >= 8) {
        for (int p = tid; p < HW; p += CL_THREADS)
          if ((fr.px[p] & MEMBER) && fr.root_of(p) == r) fr.px[p] |= INR;
        __syncthreads();
        label_components(fr, INR, 0, true, tid);
        for (int p = tid; p < HW; p += CL_THREADS) {
          if (fr.px[p] & INR) continue;
          const int i = fdiv(p, div_w), j = p - i * W;
          if (i == 0 || i == H - 1 || j == 0 || j == W - 1) fr.px[fr.root_of(p)] |= EDGE;  // the same bit from every writer
        }
        __syncthreads();
        c = 0;
        for (int p = tid; p < HW; p += CL_THREADS)
          if (!(fr.px[p] & INR) && (fr.px[fr.root_of(p)] & EDGE)) ++c;
        filled = (unsigned)HW - block_reduce<RED_SUM>(st, c, tid);
        for (int p = tid; p < HW; p += CL_THREADS) fr.px[p] &= (unsigned char)~INR;
        __syncthreads();
        label_components(fr, MEMBER, MEMBER, true, tid);  // the members' labels again
      }
      if (filled > best_f) best_f = filled, best_r = r;
      cur = (int)r;
    }

    // 3. keep it; fill the small 4-connected components of the rest; store what changed
    for (int p = tid; p < HW; p += CL_THREADS)
      if ((fr.px[p] & MEMBER) && fr.root_of(p) == best_r) fr.px[p] |= KEPT;
    __syncthreads();
    label_components(fr, KEPT, 0, false, tid);
    for (int p = tid; p < HW; p += CL_THREADS) {
      const unsigned m = fr.px[p];
      if (m & KEPT) continue;
      const bool fill = fr.size_of(fr.root_of(p)) < (unsigned)holesize;
      if (fill && !(m & MEMBER)) img[p] = 1;
      else if (!fill && (m & MEMBER)) img[p] = 0;
    }
  }
}

}  // namespace

hipError_t launch_cleanup_frames(uint8_t* frames, int64_t F, int H, int W, int holesize, hipStream_t s) {
  const size_t HW = (size_t)H * W;
  if (F < 1 || H < 1 || W < 1 || HW > CLASFV_CLEAN_MAX_PIXELS || holesize < 1 || holesize > 32767)
    return hipErrorInvalidValue;  // clasfv_fuse_votes refuses these first
  const size_t lds_bytes = CL_STATE_BYTES + 3 * ((HW + 3) & ~(size_t)3);
  if (lds_bytes > 64 * 1024) {
    // The default limit on dynamic LDS is 64 KiB; raised once per device, to all the kernel may ask (track.hip).
    static bool attr[CL_MAX_DEVICES] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= CL_MAX_DEVICES || !attr[dev]) {
      e = hipFuncSetAttribute((const void*)cleanup_frames_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              CL_STATE_BYTES + 3 * CLASFV_CLEAN_MAX_PIXELS);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < CL_MAX_DEVICES) attr[dev] = true;
    }
  }
  const unsigned grid = (unsigned)(F < CL_GRID_MAX ? F : CL_GRID_MAX);
  hipLaunchKernelGGL(cleanup_frames_kernel, dim3(grid), dim3(CL_THREADS), lds_bytes, s, frames, F, H, W, holesize,
                     fast_div((unsigned)W));
  return hipGetLastError();
}
