// CLAS-FV engine: network plan, weight folding, workspace arena and the C ABI (include/clasfv.h).
//
// Reference module: R2plus1D_18_MotionNet (src/model/R2plus1D_18_MotionNet.py:10-71) on top of
// torchvision 0.6.0 r2plus1d_18. The 242 state-dict entries are accepted under the reference key
// names (optionally "module."-prefixed, motion_segment.py:69-72); clasfv_finalize folds every
// eval-mode BatchNorm into the preceding convolution, pads channel counts for the kernels
// (45->48, 230->240, 460->480, 921->960) and uploads everything to HBM once.
#include <cxxabi.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "clasfv.h"
#include "common.h"
#include "cleanup.h"
#include "lvgeom.h"
#include "plumbing.h"
#include "render.h"
#include "track.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return fail(CLASFV_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

constexpr double kBnEps = 1e-5;

struct Param {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
  int64_t numel() const {
    int64_t n = 1;
    for (auto d : shape) n *= d;
    return n;
  }
};

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Padded channel count of an activation tensor: a multiple of the K step (16 fp32 / 32 bf16
// channels) whose 16-channel count has a divisor in {9,8,6,5,4,3} (a legal N tile). The network
// input keeps 3 + 1 fp32 channels (stem kernel).
int pad_channels(int c, bool bf16) {
  if (c == 3) return 4;
  const int step = bf16 ? 32 : 16;
  int cp = round_up(c, step);
  auto ok = [](int cp_) {
    for (int nt : {9, 8, 6, 5, 4, 3})
      if ((cp_ / 16) % nt == 0) return true;
    return false;
  };
  while (!ok(cp)) cp += step;
  return cp;
}

enum Role { STEM_S, STEM_T, SP1, TP1, SP2, TP2, DS, PROJ };

// The weight images of a Conv (Conv::img); a kKernels row names the one its kernel takes as ConvParams::w.
enum Image {
  IMG_W,       // weights [cout_alloc][Kp], dtype of the conv's input
  IMG_WINO,    // Winograd F(2x2,3x3) transformed weights (fp32 stride-1 1x3x3 convs)
  IMG_WINO4,   // Winograd F(4x4,3x3) transformed weights (the same convs, cout_p % 48 == 0)
  IMG_WINO4W,  // the same for conv_wino4w's wide output-channel blocks (wino4w_ntn(cout_p) > 0)
  IMG_WINO4R,  // the same values in conv_wino4r's (12 row waves) order
  IMG_WINOT,   // Winograd F(4,3)-in-time transformed weights (fp32 stride-1 3x1x1 convs)
  IMG_WS16,    // the stem's bf16 pieces: hi, lo [64][7 kh][8 kw][4 c] (bf16 engines); hi, mid, lo [48][7][8][4] (fp32)
  IMG_X3,      // fp32 engines' implicit-GEMM convs: 3-piece bf16 image for conv_dma_x3
  N_IMAGES
};

struct Conv {
  Role role;
  std::string w, bn;  // parameter name prefixes (".weight" / BN module)
  int cin, cout, cin_p, cout_p;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  int K, Kp, cout_alloc;
  int cin2 = 0;  // second input of a dual 1x1x1 conv (decoder P01 = W0 f_stem + W1 f_layer1)
  int stem = 0, in_bf16 = 0, out_bf16 = 0;
  void* img[N_IMAGES] = {};  // device weight images, by Image
  float* db = nullptr;       // folded-BN bias (fp32)
};

// Frees every device image of c and its bias, and nulls the pointers.
void free_conv_images(Conv& c) {
  for (void*& p : c.img) {
    (void)hipFree(p);
    p = nullptr;
  }
  (void)hipFree(c.db);
  c.db = nullptr;
}

// fp32 stride-1 3x1x1 convs run on the fused temporal Winograd kernel, fp32 stride-1 1x3x3 convs on
// the fused spatial one (CLASFV_VARIANT_NO_WINOGRAD: both on the direct implicit GEMM).
bool use_winot(const Conv& c, bool bf16, int vflags) {
  if (vflags & CLASFV_VARIANT_NO_WINOGRAD) return false;
  return !bf16 && (c.role == STEM_T || c.role == TP1 || c.role == TP2) && c.kt == 3 && c.kh == 1 && c.kw == 1 &&
         c.st == 1 && c.cin_p % 8 == 0 && c.cout_p % 64 == 0;
}

bool use_wino(const Conv& c, bool bf16, int vflags) {
  if (vflags & CLASFV_VARIANT_NO_WINOGRAD) return false;
  return !bf16 && (c.role == SP1 || c.role == SP2) && c.kt == 1 && c.kh == 3 && c.kw == 3 && c.sh == 1 &&
         c.sw == 1 && c.cin_p % 16 == 0 && c.cout_p % 48 == 0;
}

// The weight images clasfv_finalize uploads for a conv (after layout_conv), as a mask of 1 << Image, for an
// engine of this compute dtype and these variants: the upload functions ask here, and so does mark_images,
// so pick_kernel sees the same images on a finalized handle and on max_clips' device-less plan.
constexpr int bit(Image i) { return 1 << i; }
int images_of(const Conv& c, bool bf16, int vflags) {
  int m = bit(IMG_W);
  if (!c.in_bf16 && !c.stem && c.Kp % 16 == 0) m |= bit(IMG_X3);  // conv_dma_x3's split image of the same weights
  if (use_wino(c, bf16, vflags)) {
    m |= bit(IMG_WINO);
    if (c.cout_p % 48 == 0 && c.cin_p % 8 == 0) m |= bit(IMG_WINO4);
    if (c.cin_p % 8 == 0 && wino4w_weight_floats(c.cin_p, c.cout_p)) m |= bit(IMG_WINO4W);
    if (c.cin_p % 8 == 0 && wino4r_weight_floats(c.cin_p, c.cout_p)) m |= bit(IMG_WINO4R);
  }
  if (use_winot(c, bf16, vflags)) m |= bit(IMG_WINOT);
  // conv_stem_x3's pieces (fp32 engines, 48 channels) / conv_stem_bf16's (bf16 engines, 64)
  if (c.stem && c.kh == 7 && c.kw == 7 && c.cin <= 4 && (bf16 ? c.cout_p == 64 : c.cout_p == 48)) m |= bit(IMG_WS16);
  return m;
}
// Marks the images of images_of present without a device: pointers that are never read.
void mark_images(Conv& c, bool bf16, int vflags) {
  const int m = images_of(c, bf16, vflags);
  void* const some = &c;
  for (int i = 0; i < N_IMAGES; ++i) c.img[i] = (m >> i & 1) ? some : nullptr;
  // the folded-BN bias of a backbone conv (the projections have none): stem_bf16_supported asks for it, and
  // without it the device-less plan put the bf16 engines' stem on conv_stem_f32
  c.db = c.role != PROJ ? reinterpret_cast<float*>(some) : nullptr;
}

// Every CLASFV_VARIANT_* bit of include/clasfv.h with the environment variable that sets it: a switch
// is on when its variable is set to anything, a `zero_form` one when its variable starts with '0'.
struct VariantSwitch {
  int bit;
  const char* env;
  bool zero_form;
};
constexpr VariantSwitch kVariants[] = {
    {CLASFV_VARIANT_NO_WINOGRAD, "CLASFV_WINOGRAD", true},
    {CLASFV_VARIANT_NO_WINO_PATCH, "CLASFV_NO_WINO_PATCH", false},
    {CLASFV_VARIANT_WINOT_REFERENCE, "CLASFV_WINOT_REFERENCE", false},
    {CLASFV_VARIANT_NO_C8, "CLASFV_NO_C8", false},
    {CLASFV_VARIANT_NO_STEM_BF16, "CLASFV_NO_STEM_BF16", false},
    {CLASFV_VARIANT_NO_PATCH_BF16, "CLASFV_NO_PATCH_BF16", false},
    {CLASFV_VARIANT_NO_DECODER_BF16, "CLASFV_NO_DECODER_BF16", false},
    {CLASFV_VARIANT_WINOT_NO_TS1, "CLASFV_WINOT_TS1", true},
    {CLASFV_VARIANT_NO_SPLIT_K, "CLASFV_NO_SPLIT_K", false},
    {CLASFV_VARIANT_NO_WINO4, "CLASFV_NO_WINO4", false},
    {CLASFV_VARIANT_NO_DECODER_X3, "CLASFV_NO_DECODER_X3", false},
    {CLASFV_VARIANT_NO_DMA_X3, "CLASFV_NO_DMA_X3", false},
    {CLASFV_VARIANT_NO_STEM_X3, "CLASFV_NO_STEM_X3", false},
    {CLASFV_VARIANT_NO_WINO4W, "CLASFV_NO_WINO4W", false},
    {CLASFV_VARIANT_NO_PATCH32, "CLASFV_NO_PATCH32", false},
    {CLASFV_VARIANT_NO_PROJ_X3, "CLASFV_NO_PROJ_X3", false},
    {CLASFV_VARIANT_NO_WINO4R, "CLASFV_NO_WINO4R", false},
    {CLASFV_VARIANT_NO_DMA_BUF, "CLASFV_NO_DMA_BUF", false},
    {CLASFV_VARIANT_W4R_CACHED_STORES, "CLASFV_W4R_CACHED_STORES", false},
    {CLASFV_VARIANT_PATCH32_CACHED_STORES, "CLASFV_PATCH32_CACHED_STORES", false},
    {CLASFV_VARIANT_NO_DMA_W, "CLASFV_NO_DMA_W", false},
    {CLASFV_VARIANT_NO_TWALK, "CLASFV_NO_TWALK", false},
    {CLASFV_VARIANT_NO_DMA_X3_WIDE, "CLASFV_NO_DMA_X3_WIDE", false},
};

// Kernel-variant flags and tuning overrides from the environment (read once, at clasfv_create).
int env_variants() {
  int f = 0;
  for (const VariantSwitch& v : kVariants) {
    const char* e = getenv(v.env);
    if (e && (!v.zero_form || e[0] == '0')) f |= v.bit;
  }
  return f;
}

// the bits clasfv_set_kernel_variants accepts (the retired bits are rejected)
constexpr int variant_mask() {
  int m = 0;
  for (const VariantSwitch& v : kVariants) m |= v.bit;
  return m;
}
constexpr int kVariantMask = variant_mask();

int env_int(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : 0;
}

// Channel padding, K extent and dtypes of one conv for the engine's compute dtype.
void layout_conv(Conv& c, bool bf16) {
  c.stem = (c.role == STEM_S);
  c.in_bf16 = bf16 && !c.stem;
  c.out_bf16 = bf16 && c.role != PROJ;
  c.cin_p = pad_channels(c.cin, bf16);
  c.cout_p = c.role == PROJ ? c.cout : pad_channels(c.cout, bf16);
  c.K = c.kt * c.kh * c.kw * c.cin_p + c.cin2;
  c.Kp = round_up(c.K, c.in_bf16 ? 32 : 16);
  c.cout_alloc = c.cout_p;  // every tile width used divides cout_p
}

Conv make_conv(Role role, const std::string& w, const std::string& bn, int cin, int cout, int kt, int kh, int kw,
               int st, int sh, int sw, int pt, int ph, int pw) {
  Conv c;
  c.role = role;
  c.w = w;
  c.bn = bn;
  c.cin = cin;
  c.cout = cout;
  c.kt = kt, c.kh = kh, c.kw = kw, c.st = st, c.sh = sh, c.sw = sw, c.pt = pt, c.ph = ph, c.pw = pw;
  layout_conv(c, false);
  return c;
}

int midplanes(int i, int o) { return (i * o * 27) / (i * 9 + 3 * o); }

// Engine-wide kernel switches: CLASFV_VARIANT_* flags and the implicit-GEMM / patch-kernel tile
// overrides (0: automatic).
struct Tuning {
  int vflags = 0, conv_nt = 0, patch_nt = 0;
};

}  // namespace

struct clasfv_engine {
  int device = 0;
  std::vector<Param> params;
  std::unordered_map<std::string, int> index;
  std::vector<Conv> convs;  // backbone, execution order
  Conv proj[5];             // decoder projections (stem, layer1..4) -> 64 channels
  float *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *wh = nullptr, *bh = nullptr;
  void* w2x3 = nullptr;  // W2 as three bf16 pieces in the decoder's MFMA lane order (fp32 engines)
  bool ready = false;
  int dtype = CLASFV_DTYPE_FP32;  // compute dtype of the encoder convs
  Tuning tune;                    // kernel variants / tile overrides (environment at create)
  float* zero = nullptr;  // 256 zero bytes for padding taps
  // One forward context per launch stream: the workspace arena (activations, mid tensors, decoder taps
  // and index table) and the side stream with its fork / join events. The decoder projections of the
  // stem/layer1, layer2 and layer3 taps run on the side stream as soon as their tap exists, filling the
  // CUs the backbone's later (small-grid) convs leave idle; the decoder waits for them (events, no host
  // synchronisation). Forwards issued on different streams own different contexts, so they may run
  // concurrently on one handle (a serving pipeline with two videos in flight): each one's arena is
  // touched only by work ordered on its own stream. Forwards on one stream reuse its context in order.
  struct Ctx {
    hipStream_t stream = nullptr;  // the launch stream this context belongs to
    char* arena = nullptr;
    size_t arena_bytes = 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    uint64_t last_use = 0;
  };
  std::vector<Ctx*> ctxs;
  uint64_t ctx_clock = 0;
  // (T, H, W) -> the largest batch one pass of the network can address (max_clips), for the handle's
  // finalized state: emptied by whatever changes a kernel choice (finalize, dtype, variants)
  std::map<std::array<int, 3>, int> clip_limit;
  // per-kernel HIP-event timing of clasfv_forward (clasfv_set_kernel_timing)
  bool ktime = false;
  std::vector<hipEvent_t> evs;  // event pool; evs[0..nev) recorded since the last read
  int nev = 0;
  struct Rec {
    const char* name;
    double gflop;   // algorithmic (direct-convolution MACs x 2, unpadded channels)
    double xgflop;  // MFMA work the launch executes (Winograd-domain products, padded channels/tiles)
    int e0, e1;
  };
  std::vector<Rec> recs;
  // launch log (clasfv_set_launch_log): what CLASFV_LAUNCH noted for every launch of clasfv_forward,
  // clasfv_run_conv and clasfv_run_decoder since the last clasfv_launch_log
  bool llog = false;
  struct LogRec {
    const char* label;  // into `labels`
    long grid;
    int passes, conv;  // conv: the diagnostics' conv index, -1 for pack_input and the decoder
  };
  std::vector<LogRec> log;
  std::unordered_map<const void*, std::string> labels;  // kernel function -> instantiation label (label_of)
};

namespace {

void add_param(clasfv_engine* e, const std::string& name, std::vector<int64_t> shape) {
  Param p;
  p.name = name;
  p.shape = std::move(shape);
  e->index[name] = (int)e->params.size();
  e->params.push_back(std::move(p));
}

void add_bn(clasfv_engine* e, const std::string& pre, int c) {
  add_param(e, pre + ".weight", {c});
  add_param(e, pre + ".bias", {c});
  add_param(e, pre + ".running_mean", {c});
  add_param(e, pre + ".running_var", {c});
  add_param(e, pre + ".num_batches_tracked", {});
}

// Build the layer plan and the state-dict table in the reference's registration order.
void build_plan(clasfv_engine* e) {
  const std::string R = "r2plus1d_model.";
  auto reg = [&](const Conv& c) {
    add_param(e, c.w + ".weight", {c.cout, c.cin, c.kt, c.kh, c.kw});
    add_bn(e, c.bn, c.cout);
    e->convs.push_back(c);
  };
  reg(make_conv(STEM_S, R + "stem.0", R + "stem.1", 3, 45, 1, 7, 7, 1, 2, 2, 0, 3, 3));
  reg(make_conv(STEM_T, R + "stem.3", R + "stem.4", 45, 64, 3, 1, 1, 1, 1, 1, 1, 0, 0));
  int inplanes = 64;
  const int planes_l[4] = {64, 128, 256, 512}, stride_l[4] = {1, 2, 2, 2};
  for (int li = 0; li < 4; ++li) {
    const int planes = planes_l[li], stride = stride_l[li];
    for (int b = 0; b < 2; ++b) {
      const int st = b == 0 ? stride : 1;
      const int cin1 = b == 0 ? inplanes : planes;
      const int mid = midplanes(cin1, planes);
      const std::string pre = R + "layer" + std::to_string(li + 1) + "." + std::to_string(b) + ".";
      reg(make_conv(SP1, pre + "conv1.0.0", pre + "conv1.0.1", cin1, mid, 1, 3, 3, 1, st, st, 0, 1, 1));
      reg(make_conv(TP1, pre + "conv1.0.3", pre + "conv1.1", mid, planes, 3, 1, 1, st, 1, 1, 1, 0, 0));
      reg(make_conv(SP2, pre + "conv2.0.0", pre + "conv2.0.1", planes, mid, 1, 3, 3, 1, 1, 1, 0, 1, 1));
      reg(make_conv(TP2, pre + "conv2.0.3", pre + "conv2.1", mid, planes, 3, 1, 1, 1, 1, 1, 1, 0, 0));
      if (b == 0 && (stride != 1 || inplanes != planes))
        reg(make_conv(DS, pre + "downsample.0", pre + "downsample.1", inplanes, planes, 1, 1, 1, stride, stride,
                      stride, 0, 0, 0));
    }
    inplanes = planes;
  }
  add_param(e, R + "fc.weight", {400, 512});
  add_param(e, R + "fc.bias", {400});
  add_param(e, "comb_1_layer.weight", {64, 1024, 1, 1, 1});
  add_param(e, "comb_1_layer.bias", {64});
  add_bn(e, "comb_batch_norm_1", 64);
  add_param(e, "comb_2_layer.weight", {64, 64, 1, 1, 1});
  add_param(e, "comb_2_layer.bias", {64});
  add_bn(e, "comb_batch_norm_2", 64);
  add_param(e, "motion_head.weight", {4, 64, 1, 1, 1});
  add_param(e, "motion_head.bias", {4});
  add_param(e, "segmentation_head.weight", {2, 64, 1, 1, 1});
  add_param(e, "segmentation_head.bias", {2});
  // decoder projections: proj[0] is the dual 1x1x1 conv over (stem, layer1) -> P01; proj[1] unused
  const int tap_c[5] = {64, 64, 128, 256, 512};
  for (int i = 0; i < 5; ++i) e->proj[i] = make_conv(PROJ, "", "", tap_c[i], 64, 1, 1, 1, 1, 1, 1, 0, 0, 0);
  e->proj[0].cin2 = 64;
  layout_conv(e->proj[0], false);
}

const std::vector<float>& P(clasfv_engine* e, const std::string& n) { return e->params[e->index.at(n)].data; }

void bn_scale_shift(clasfv_engine* e, const std::string& bn, int c, std::vector<double>& s, std::vector<double>& t) {
  const auto& g = P(e, bn + ".weight");
  const auto& b = P(e, bn + ".bias");
  const auto& m = P(e, bn + ".running_mean");
  const auto& v = P(e, bn + ".running_var");
  s.resize(c);
  t.resize(c);
  for (int i = 0; i < c; ++i) {
    s[i] = (double)g[i] / sqrt((double)v[i] + kBnEps);
    t[i] = (double)b[i] - (double)m[i] * s[i];
  }
}

template <class T>  // T: float, or void for a Conv image
int upload(const std::vector<float>& h, T** d) {
  HIP_TRY(hipMalloc(d, h.size() * sizeof(float)));
  HIP_TRY(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return CLASFV_OK;
}

// float -> bf16 bits, round to nearest even (weights are finite).
uint16_t to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7FFF + ((u >> 16) & 1);
  return (uint16_t)(u >> 16);
}

int upload_u16(const std::vector<uint16_t>& b, void** d) {
  HIP_TRY(hipMalloc(d, b.size() * sizeof(uint16_t)));
  HIP_TRY(hipMemcpy(*d, b.data(), b.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  return CLASFV_OK;
}

int upload_bf16(const std::vector<float>& h, void** d) {
  std::vector<uint16_t> b(h.size());
  for (size_t i = 0; i < h.size(); ++i) b[i] = to_bf16(h[i]);
  return upload_u16(b, d);
}

// Folded, padded [cout_alloc][Kp] weight image of one conv. `wsrc(o, c, tap)` returns the raw weight of
// input column c < cols (c.cin; the concatenated width of a decoder projection, whose one tap has no stride).
template <class F>
int upload_conv(Conv& c, int cols, F wsrc, const std::vector<double>& scale, const std::vector<double>& shift,
                bool has_bias) {
  std::vector<float> w((size_t)c.cout_alloc * c.Kp, 0.f);
  const int taps = c.kt * c.kh * c.kw;
  for (int o = 0; o < c.cout; ++o)
    for (int tap = 0; tap < taps; ++tap)
      for (int ci = 0; ci < cols; ++ci)
        w[(size_t)o * c.Kp + (size_t)tap * c.cin_p + ci] = (float)((double)wsrc(o, ci, tap) * scale[o]);
  int rc = c.in_bf16 ? upload_bf16(w, &c.img[IMG_W]) : upload(w, &c.img[IMG_W]);
  if (rc) return rc;
  if (images_of(c, false, 0) & bit(IMG_X3)) {  // conv_dma_x3's split image of the same weights
    std::vector<uint16_t> x3(dma_x3_weight_elems(c.cout_alloc, c.Kp));
    dma_x3_weight_image(w.data(), c.cout_alloc, c.Kp, x3.data());
    if ((rc = upload_u16(x3, &c.img[IMG_X3]))) return rc;
  }
  if (has_bias) {
    std::vector<float> b(c.cout_alloc, 0.f);
    for (int o = 0; o < c.cout; ++o) b[o] = (float)shift[o];
    rc = upload(b, &c.db);
  }
  return rc;
}

// BN-folded weights w[cout][cin][taps] of c as double products, unrounded: what the Winograd weight
// transforms take (upload_conv rounds the same products to float first, on purpose).
std::vector<double> folded_weights(const Conv& c, const std::vector<float>& w, const std::vector<double>& s, int taps) {
  const size_t per_o = (size_t)c.cin * taps;
  std::vector<double> wf((size_t)c.cout * per_o);
  for (int o = 0; o < c.cout; ++o)
    for (size_t i = 0; i < per_o; ++i) wf[o * per_o + i] = (double)w[o * per_o + i] * s[o];
  return wf;
}

// The spatial Winograd images of a 1x3x3 conv (use_wino), each where its kernel has a tile for the widths.
int upload_wino_images(Conv& c, const std::vector<float>& w, const std::vector<double>& s) {
  const std::vector<double> wf = folded_weights(c, w, s, 9);
  int rc;
  std::vector<float> u((size_t)16 * c.cin_p * c.cout_p);
  wino_transform_weights(wf.data(), c.cout, c.cin, c.cout_p, c.cin_p, u.data());
  if ((rc = upload(u, &c.img[IMG_WINO]))) return rc;
  const int m = images_of(c, false, 0);  // (called for a use_wino conv: the widths decide the rest)
  const struct {
    Image img;
    size_t (*floats)(int cin_p, int cout_p);
    void (*transform)(const double* w, int cout, int cin, int cout_p, int cin_p, float* U);
  } f4x4[] = {{IMG_WINO4, wino4_weight_floats, wino4_transform_weights},
              {IMG_WINO4W, wino4w_weight_floats, wino4w_transform_weights},
              {IMG_WINO4R, wino4r_weight_floats, wino4r_transform_weights}};
  for (const auto& f : f4x4) {
    if (!(m & bit(f.img))) continue;
    std::vector<float> u4(f.floats(c.cin_p, c.cout_p));
    f.transform(wf.data(), c.cout, c.cin, c.cout_p, c.cin_p, u4.data());
    if ((rc = upload(u4, &c.img[f.img]))) return rc;
  }
  return CLASFV_OK;
}

// The temporal Winograd image of a 3x1x1 conv (use_winot).
int upload_winot_image(Conv& c, const std::vector<float>& w, const std::vector<double>& s) {
  const std::vector<double> wf = folded_weights(c, w, s, 3);
  std::vector<float> u((size_t)6 * c.cin_p * c.cout_p);
  winot_transform_weights(wf.data(), c.cout, c.cin, c.cout_p, c.cin_p, u.data());
  return upload(u, &c.img[IMG_WINOT]);
}

// fn(k, raw weight, its output channel's BN scale) for every 7x7 tap of the stem, k its offset in a
// [cout_p][7 kh][8 kw][4 c] image: the K order conv_stem_x3 and conv_stem_bf16 share.
template <class F>
void for_stem_taps(const Conv& c, const std::vector<float>& w, const std::vector<double>& s, F fn) {
  for (int o = 0; o < c.cout; ++o)
    for (int ci = 0; ci < c.cin; ++ci)
      for (int kh = 0; kh < 7; ++kh)
        for (int kw = 0; kw < 7; ++kw)
          fn((((size_t)o * 7 + kh) * 8 + kw) * 4 + ci, w[((size_t)o * c.cin + ci) * 49 + kh * 7 + kw], s[o]);
}

// The stem's split-bf16 images (IMG_WS16); each kernel's pieces keep their own rounding.
int upload_stem_images(Conv& c, const std::vector<float>& w, const std::vector<double>& s, bool bf16) {
  if (!(images_of(c, bf16, 0) & bit(IMG_WS16))) return CLASFV_OK;
  if (!bf16) {  // conv_stem_x3's pieces
    const size_t img = (size_t)48 * 7 * 8 * 4;
    std::vector<float> ws(3 * img, 0.f);  // hi, mid, lo: bf16 of the remainder, in double
    for_stem_taps(c, w, s, [&](size_t k, float wv, double scale) {
      double r = (double)(float)((double)wv * scale);
      for (int pc = 0; pc < 3; ++pc) {
        const uint32_t hb = (uint32_t)to_bf16((float)r) << 16;
        float f;
        memcpy(&f, &hb, 4);
        ws[pc * img + k] = f;
        r -= f;
      }
    });
    return upload_bf16(ws, &c.img[IMG_WS16]);
  }
  {  // conv_stem_bf16's K order
    const size_t img = (size_t)64 * 7 * 8 * 4;
    std::vector<float> ws(2 * img, 0.f);  // hi image, then lo = bf16(w - hi)
    for_stem_taps(c, w, s, [&](size_t k, float wv, double scale) {
      const float v = (float)((double)wv * scale);
      const uint32_t hb = (uint32_t)to_bf16(v) << 16;
      float hi;
      memcpy(&hi, &hb, 4);
      ws[k] = hi;
      ws[img + k] = v - hi;
    });
    return upload_bf16(ws, &c.img[IMG_WS16]);
  }
  return CLASFV_OK;
}

// Every device image of one backbone conv, BN folded, for the engine's compute dtype and variants.
int finalize_conv(clasfv_engine* h, Conv& c, bool bf16) {
  free_conv_images(c);
  std::vector<double> s, t;
  bn_scale_shift(h, c.bn, c.cout, s, t);
  const auto& w = P(h, c.w + ".weight");
  const int taps = c.kt * c.kh * c.kw;
  const int cin = c.cin;
  int rc = upload_conv(
      c, cin, [&](int o, int ci, int tap) { return w[((size_t)o * cin + ci) * taps + tap]; }, s, t, true);
  const int m = images_of(c, bf16, h->tune.vflags);
  if (!rc && (m & bit(IMG_WINO))) rc = upload_wino_images(c, w, s);
  if (!rc) rc = upload_stem_images(c, w, s, bf16);
  if (!rc && (m & bit(IMG_WINOT))) rc = upload_winot_image(c, w, s);
  return rc;
}

// comb_1 + BN1 folded, split per tap (concat order stem, layer1, layer2, layer3, layer4)
int finalize_projections(clasfv_engine* h) {
  std::vector<double> s, t;
  bn_scale_shift(h, "comb_batch_norm_1", 64, s, t);
  const auto& w1 = P(h, "comb_1_layer.weight");
  const std::vector<double> zero(64, 0.0);
  const int col0[5] = {0, 64, 128, 256, 512};
  for (int i = 0; i < 5; ++i) {
    if (i == 1) continue;  // folded into the dual proj[0]
    Conv& c = h->proj[i];
    free_conv_images(c);
    const int o0 = col0[i];
    if (int rc = upload_conv(
            c, c.cin + c.cin2, [&](int o, int ci, int) { return w1[(size_t)o * 1024 + o0 + ci]; }, s, zero, false))
      return rc;
  }
  return CLASFV_OK;
}

// The decoder's own weights: comb_1's bias through BN1, comb_2 + BN2 folded, and the two heads as one
// 8-row matrix (seg0, seg1, mot0..mot3, 0, 0).
int finalize_decoder(clasfv_engine* h) {
  std::vector<double> s, t;
  bn_scale_shift(h, "comb_batch_norm_1", 64, s, t);
  const auto& bias1 = P(h, "comb_1_layer.bias");
  std::vector<float> b1(64);
  for (int o = 0; o < 64; ++o) b1[o] = (float)(s[o] * (double)bias1[o] + t[o]);
  bn_scale_shift(h, "comb_batch_norm_2", 64, s, t);
  const auto& w2 = P(h, "comb_2_layer.weight");
  const auto& bias2 = P(h, "comb_2_layer.bias");
  std::vector<float> w2f(64 * 64), b2(64);
  for (int o = 0; o < 64; ++o) {
    for (int k = 0; k < 64; ++k) w2f[o * 64 + k] = (float)((double)w2[o * 64 + k] * s[o]);
    b2[o] = (float)(s[o] * (double)bias2[o] + t[o]);
  }
  const auto& ws = P(h, "segmentation_head.weight");
  const auto& bs = P(h, "segmentation_head.bias");
  const auto& wm = P(h, "motion_head.weight");
  const auto& bm = P(h, "motion_head.bias");
  std::vector<float> whf(8 * 64, 0.f), bhf(8, 0.f);
  for (int k = 0; k < 64; ++k) {
    whf[0 * 64 + k] = ws[k];
    whf[1 * 64 + k] = ws[64 + k];
    for (int m = 0; m < 4; ++m) whf[(2 + m) * 64 + k] = wm[m * 64 + k];
  }
  bhf[0] = bs[0];
  bhf[1] = bs[1];
  for (int m = 0; m < 4; ++m) bhf[2 + m] = bm[m];
  for (float** d : {&h->b1, &h->w2, &h->b2, &h->wh, &h->bh}) {
    (void)hipFree(*d);
    *d = nullptr;
  }
  // W2 and the head weights as hi + mid + lo bf16 pieces in the X3 decoder's lane order
  std::vector<uint16_t> w2x3(DECODER_X3_ELEMS);
  decoder_x3_weights(w2f.data(), whf.data(), w2x3.data());
  (void)hipFree(h->w2x3);
  h->w2x3 = nullptr;
  int rc = upload(b1, &h->b1);
  if (!rc) rc = upload(w2f, &h->w2);
  if (!rc) rc = upload_u16(w2x3, &h->w2x3);
  if (!rc) rc = upload(b2, &h->b2);
  if (!rc) rc = upload(whf, &h->wh);
  if (!rc) rc = upload(bhf, &h->bh);
  return rc;
}

struct Shape5 {
  int n, t, h, w, c;
  size_t numel() const { return (size_t)n * t * h * w * c; }
  int64_t voxels() const { return (int64_t)n * t * h * w; }
};

// Algorithmic FLOPs of one conv (2 per MAC over the unpadded channels).
double conv_gflop(const Conv& c, const Shape5& out) {
  const double m = (double)out.n * out.t * out.h * out.w;
  return 2.0 * m * c.cout * (double)(c.cin + c.cin2) * c.kt * c.kh * c.kw * 1e-9;
}

// MFMA work one launch of a kernel executes for conv c (2 FLOP per multiply-add issued to the
// matrix cores, padded channels and partial tiles included), one function per formula (kKernels):
// Winograd F(2x2,3x3) issues 16 products per 2x2 output tile and (input, output) channel pair
// instead of 36, F(2x4,3x3) 24 per 2x4 tile instead of 72, F(4,3) in time 6 per 4 frames instead of
// 12; the implicit GEMMs issue ceil(M / BM) * BM rows x cout_p x Kp.
// F(4x4,3x3): 36 products per 4x4 tile and channel pair, 16-tile groups (counted by the kernels' files)
ConvParams wino4_exec_shape(const Conv& c, const Shape5& out) {
  ConvParams p{};
  p.N = out.n, p.Ti = p.To = out.t, p.Hi = p.Ho = out.h, p.Wi = p.Wo = out.w;
  p.Cin = c.cin_p, p.Cout = c.cout_p;
  return p;
}
double xg_wino4r(const Conv& c, const Shape5& out) { return wino4r_exec_gflop(wino4_exec_shape(c, out)); }
double xg_wino4w(const Conv& c, const Shape5& out) { return wino4w_exec_gflop(wino4_exec_shape(c, out)); }
double xg_wino4(const Conv& c, const Shape5& out) { return wino4_exec_gflop(wino4_exec_shape(c, out)); }
double xg_wino(const Conv& c, const Shape5& out) {
  const double nt = (double)out.n * out.t;
  const double cc = (double)c.cin_p * c.cout_p;
  return 2.0 * nt * ((out.h + 1) / 2) * ((out.w + 1) / 2) * 16.0 * cc * 1e-9;
}
double xg_winot(const Conv& c, const Shape5& out) {
  const double cc = (double)c.cin_p * c.cout_p;
  return 2.0 * out.n * (out.t / 4) * (double)out.h * out.w * 6.0 * cc * 1e-9;
}
// Split-bf16 ("x3") kernels of the fp32 engines run on the bf16 matrix pipe: their work is counted
// in that pipe's own products, six bf16 products per product of the fp32 GEMM they compute (the
// f32-MFMA kernels count f32 products), so each kernel's rate compares with the peak of the pipe it
// issues to (bench.py rates them against 2.5 PFLOP/s, the f32 ones against 157.3 TFLOP/s).
double xg_stem_x3(const Conv&, const Shape5& out) {  // 6 x the fp32 GEMM (K = 7 rows x 8 taps x 4 channels)
  return 6 * 2.0 * ceil((double)out.n * out.t * out.h * out.w / 256.0) * 256.0 * 48.0 * 224.0 * 1e-9;
}
double xg_stem_bf16(const Conv&, const Shape5& out) {
  return 3 * 2.0 * ceil((double)out.n * out.t * out.h * out.w / 256.0) * 256.0 * 64.0 * 224.0 * 1e-9;
}
double xg_patch_bf16(const Conv& c, const Shape5& out) {  // frames x 64-pixel tiles: 2 x 8x8 for 1x3x3, 4 x 64 flat for 3x1x1
  const int fr = c.kt == 1 ? 2 : 4;
  const double px = c.kt == 1 ? (double)((out.h + 7) / 8 * 8) * ((out.w + 7) / 8 * 8)
                              : (double)((out.h * out.w + 63) / 64 * 64);
  return 2.0 * out.n * ((out.t + fr - 1) / fr * fr) * px * c.cout_p * (double)c.Kp * 1e-9;
}
double xg_proj_x3(const Conv& c, const Shape5& out) {  // 32-voxel items, 6 x the fp32 GEMM it computes
  return 6 * 2.0 * ceil((double)out.n * out.t * out.h * out.w / 32.0) * 32.0 * c.cout_p * (double)c.Kp * 1e-9;
}
double xg_twalk_bf16(const Conv& c, const Shape5& out) {  // 32-pixel columns; 3T - 2 taps per output column (clip ends)
  return 2.0 * out.n * ((out.h * out.w + 31) / 32 * 32) * (double)c.cout_p * c.cin_p * (3.0 * out.t - 2.0) * 1e-9;
}
double xg_patch32_bf16(const Conv& c, const Shape5& out) {  // 4 frames x 8x8-pixel tiles
  return 2.0 * out.n * ((out.t + 3) / 4 * 4) * (double)((out.h + 7) / 8 * 8) * ((out.w + 7) / 8 * 8) * c.cout_p *
         (double)c.Kp * 1e-9;
}
// conv_dma_x3: six bf16 products per product of the fp32 GEMM it computes (K padded to 32-deep pairs)
// (M tiles of bm rows: 128, or the wide form's 256)
double xg_dma_x3_rows(const Conv& c, const Shape5& out, double bm) {
  const double m = (double)out.n * out.t * out.h * out.w;
  return 6 * 2.0 * (ceil(m / bm) * bm) * c.cout_p * (double)((c.Kp + 31) / 32 * 32) * 1e-9;
}
double xg_dma_x3(const Conv& c, const Shape5& out) { return xg_dma_x3_rows(c, out, 128.0); }
double xg_gemm(const Conv& c, const Shape5& out) {  // launch_conv's kernels: 128-row M tiles
  const double m = (double)out.n * out.t * out.h * out.w;
  return 2.0 * (ceil(m / 128.0) * 128.0) * c.cout_p * (double)c.Kp * 1e-9;
}

// The conv kernels pick_kernel chooses among. kKernels has one row per enumerator, in this order.
enum Kernel {
  K_WINO4R, K_WINO4W, K_WINO4, K_WINO_Q, K_WINO, K_STEM_BF16, K_STEM_X3, K_WINOT, K_PATCH_BF16, K_PATCH32_BF16,
  K_TWALK_BF16, K_PROJ_X3, K_DMA_X3, K_STEM_F32, K_DMA_W, K_DMA
};

struct KernelInfo {
  Kernel id;
  const char* name;  // reported by clasfv_kernel_timing and clasfv_run_conv
  Image image;       // the Conv image the kernel takes as ConvParams::w
  int off;           // the CLASFV_VARIANT_* bits that switch the kernel off, any of them
  // the kernel's gate over the conv's parameters; nullptr: an implicit GEMM of last resort, which takes any
  // conv. (A bit that chooses a form inside a launcher is read by the gate the launcher re-asks, not here.)
  bool (*supported)(const ConvParams& p);
  // 8-channel-blocked layout: kernels that may write it (y_c8) / read it (x_c8). Measured per
  // producer (30 clips, profiles/r02j_*): stem and conv_wino_q (layer1, layer2) write the blocked
  // layout at no cost while the temporal kernels after them gain 7-24 %; conv_wino (layer3) broke
  // even and stays channels-last.
  bool writes_c8, reads_c8;
  double (*xgflop)(const Conv& c, const Shape5& out);  // MFMA work of one launch, see above
};
constexpr int V_NO4 = CLASFV_VARIANT_NO_WINO4, V_NO4W = CLASFV_VARIANT_NO_WINO4W, V_NO4R = CLASFV_VARIANT_NO_WINO4R,
              V_NOPB = CLASFV_VARIANT_NO_PATCH_BF16;
constexpr KernelInfo kKernels[] = {
    {K_WINO4R, "conv_wino4r", IMG_WINO4R, V_NO4 | V_NO4W | V_NO4R, wino4r_supported, true, false, xg_wino4r},
    {K_WINO4W, "conv_wino4w", IMG_WINO4W, V_NO4 | V_NO4W, wino4w_supported, true, false, xg_wino4w},
    {K_WINO4, "conv_wino4", IMG_WINO4, V_NO4, wino4_supported, true, false, xg_wino4},
    {K_WINO_Q, "conv_wino_q", IMG_WINO, CLASFV_VARIANT_NO_WINO_PATCH, winoq_supported, true, false, xg_wino},
    {K_WINO, "conv_wino", IMG_WINO, 0, wino_supported, false, false, xg_wino},
    {K_STEM_BF16, "conv_stem_bf16", IMG_WS16, CLASFV_VARIANT_NO_STEM_BF16, stem_bf16_supported, false, false, xg_stem_bf16},
    {K_STEM_X3, "conv_stem_x3", IMG_WS16, CLASFV_VARIANT_NO_STEM_X3, stem_x3_supported, true, false, xg_stem_x3},
    {K_WINOT, "conv_winot", IMG_WINOT, 0, winot_supported, false, true, xg_winot},
    {K_PATCH_BF16, "conv_patch_bf16", IMG_W, V_NOPB, patch_bf16_supported, false, false, xg_patch_bf16},
    {K_PATCH32_BF16, "conv_patch32_bf16", IMG_W, V_NOPB | CLASFV_VARIANT_NO_PATCH32, patch32_bf16_supported, false, false,
     xg_patch32_bf16},
    {K_TWALK_BF16, "conv_twalk_bf16", IMG_W, V_NOPB | CLASFV_VARIANT_NO_TWALK, twalk_bf16_supported, false, false,
     xg_twalk_bf16},
    {K_PROJ_X3, "conv_proj_x3", IMG_X3, CLASFV_VARIANT_NO_PROJ_X3 | CLASFV_VARIANT_NO_DMA_X3, proj_x3_supported, false, false,
     xg_proj_x3},
    {K_DMA_X3, "conv_dma_x3", IMG_X3, CLASFV_VARIANT_NO_DMA_X3, dma_x3_supported, false, false, xg_dma_x3},
    {K_STEM_F32, "conv_stem_f32", IMG_W, 0, nullptr, true, false, xg_gemm},
    {K_DMA_W, "conv_dma_w", IMG_W, 0, dma_w_ok, false, false, xg_gemm},
    {K_DMA, "conv_dma", IMG_W, 0, nullptr, false, false, xg_gemm},
};
constexpr bool kernels_in_order() {
  int i = 0;
  for (const KernelInfo& k : kKernels)
    if (k.id != i++) return false;
  return i == K_DMA + 1;
}
static_assert(kernels_in_order(), "kKernels: one row per Kernel enumerator, in the enum's order");

// Conv parameters of c over an input of shape `in` (output shape in `out`; tensors unset).
ConvParams conv_params(const Conv& c, const Shape5& in, Shape5& out) {
  out.n = in.n;
  out.t = (in.t + 2 * c.pt - c.kt) / c.st + 1;
  out.h = (in.h + 2 * c.ph - c.kh) / c.sh + 1;
  out.w = (in.w + 2 * c.pw - c.kw) / c.sw + 1;
  out.c = c.cout_p;
  ConvParams p{};
  p.w = c.img[IMG_W];
  p.bias = c.db;
  p.N = in.n, p.Ti = in.t, p.Hi = in.h, p.Wi = in.w, p.Cin = in.c;
  p.To = out.t, p.Ho = out.h, p.Wo = out.w, p.Cout = out.c;
  p.KT = c.kt, p.KH = c.kh, p.KW = c.kw, p.st = c.st, p.sh = c.sh, p.sw = c.sw, p.pt = c.pt, p.ph = c.ph, p.pw = c.pw;
  p.K = c.K, p.Kp = c.Kp;
  // (an M past int is clamped, not wrapped: conv_size_error refuses it before anything reads p.M)
  p.M = (int)std::min<int64_t>(out.voxels(), INT32_MAX);
  p.Cin2 = c.cin2;
  p.stem = c.stem;
  p.in_bf16 = c.in_bf16;
  p.out_bf16 = c.out_bf16;
  return p;
}

// Whether kernel k can run c with parameters p: its weight image is there, no variant bit of p.vflags
// switches it off, and its gate accepts p.
bool can_run(Kernel k, const Conv& c, const ConvParams& p) {
  const KernelInfo& ki = kKernels[k];
  return c.img[ki.image] && !(p.vflags & ki.off) && (!ki.supported || ki.supported(p));
}

// The kernel of c with parameters p (p.vflags selects A/B variants): the first of this list that can run it.
Kernel pick_kernel(const Conv& c, const ConvParams& p) {
  // 7x7 maps (layer4 at 112x112 clips): the split-bf16 direct GEMM beats F(4x4)'s partial edge tiles
  // (convbench 0.284 vs 0.312 ms per 1152-channel launch, profiles/r03p_dma_x3_tiles.txt); per-clip
  // shape rule
  if (c.img[IMG_WINO4] && p.Ho * p.Wo <= 64 && !p.y_c8 && can_run(K_DMA_X3, c, p)) return K_DMA_X3;
  for (Kernel k : {K_WINO4R, K_WINO4W, K_WINO4, K_WINO_Q, K_WINO, K_STEM_BF16, K_STEM_X3})
    if (can_run(k, c, p)) return k;
  // temporal convs on <= 256-voxel clip maps (layer4, T = 4): split-K 4 on the split-bf16 direct GEMM
  // beats the one-tile-row F(4,3) form (convbench 0.119 vs 0.145 ms with both split sums)
  if (c.img[IMG_WINOT] && (long)p.To * p.Ho * p.Wo <= 256 && !p.x_c8 && !p.y_c8 && can_run(K_DMA_X3, c, p))
    return K_DMA_X3;
  for (Kernel k : {K_WINOT, K_PROJ_X3, K_PATCH32_BF16, K_TWALK_BF16, K_PATCH_BF16, K_DMA_X3})
    if (can_run(k, c, p)) return k;
  if (c.stem) return K_STEM_F32;
  // bf16 direct convs with whole 128-B tap rows (launch_dma takes conv_dma_w at the 128-row M tile)
  return can_run(K_DMA_W, c, p) ? K_DMA_W : K_DMA;
}

// Whether the mid tensor between producer `a` (input shape `in`) and consumer `b` goes through HBM
// in the 8-channel-blocked layout: `a` runs on a kernel that writes it and `b` on one that reads it
// (conv_winot where launch_winot takes conv_winot5; CLASFV_VARIANT_NO_C8: always channels-last).
// The choice depends on flags and on the shape of one clip only, never on the batch (no *_supported test
// reads ConvParams::w): a batch whose blocked mid tensor conv_winot5 cannot address is refused by
// run_conv, like a batch past any other limit of a clip's kernel, so max_clips stops below it and a
// clip's launches, layouts included, are those of its shape whatever N is.
bool c8_pair(const Conv& a, const Conv& b, const Shape5& in_batch, const Tuning& tu) {
  if (tu.vflags & CLASFV_VARIANT_NO_C8) return false;
  Shape5 in = in_batch, mid, out;
  in.n = 1;
  ConvParams pa = conv_params(a, in, mid);
  ConvParams pb = conv_params(b, mid, out);
  pa.vflags = pb.vflags = tu.vflags;
  return kKernels[pick_kernel(a, pa)].writes_c8 && !a.out_bf16 && kKernels[pick_kernel(b, pb)].reads_c8 &&
         winot_c8_ok(pb);
}

// Split-K into S partial sums in the caller's scratch, where S > 1 and the scratch holds them.
void split_k(ConvParams& p, int S, void* scratch, size_t scratch_bytes) {
  if (S > 1 && scratch && (size_t)S * p.M * p.Cout * sizeof(float) <= scratch_bytes) {
    p.part = reinterpret_cast<float*>(scratch);
    p.n_split = S;
  }
}

// ---- size limits ("Size limits") ---------------------------------------------------------
// Every *_supported gate implies the addressing assumptions of its own kernel. What no gate can say is
// checked here before any launch (k: the kernel of one clip of the shape, kn: the kernel pick_kernel
// gives the whole batch): nullptr when every address the launch forms is in range, else the reason.
//  * M and the input's voxel count are ints in ConvParams, the FastDiv decodes and every grid.
//  * The kernel is the one a single clip of the shape runs on. The size clauses of the gates would
//    otherwise hand a large batch to the next kernel of pick_kernel's list, often one of another rounding
//    family (F(4x4) -> F(2x2) -> conv_dma_x3), and a clip's bits would depend on its batch.
//    conv_dma_w -> conv_dma, at the 2^31 bytes where conv_dma_w's buffer DMAs end, is refused like the rest
//    although the two are bit-identical: the launch plan promises one kernel name per conv whatever N is.
//    (launch_winot's conv_winot5 -> conv_winot over a channels-last input and the buffer -> pointer forms
//    of conv_dma / conv_dma_x3 are switches between bit-identical forms of one kernel, made inside its
//    launcher, and stay.)
//  * gemm_size_error, once split-K is decided -- the implicit GEMMs (the list's last resort, so nothing
//    catches what they cannot address): their pointer forms offset x and x2 by 32-bit element counts,
//    and their grid is an int.
const char* conv_size_error(Kernel k, Kernel kn, const Shape5& in, const Shape5& out) {
  constexpr int64_t k31 = (int64_t)1 << 31;
  if (out.voxels() >= k31) return "the output has 2^31 voxels or more";
  if (in.voxels() >= k31) return "the input has 2^31 voxels or more";
  if (kn != k)
    return "the batch is past the size limit of the kernel one clip of this shape runs on";
  return nullptr;
}
const char* gemm_size_error(const KernelInfo& k, const ConvParams& p, const Shape5& in, const Shape5& out) {
  constexpr int64_t k31 = (int64_t)1 << 31, k32 = (int64_t)1 << 32;
  if (k.id == K_DMA_X3 || k.id == K_DMA_W || k.id == K_DMA || k.id == K_STEM_F32) {
    if (in.voxels() * p.Cin >= k32 || (p.x2 && in.voxels() * p.Cin2 >= k32))
      return "an input of the implicit GEMM has 2^32 elements or more";
    // 128-row M tiles, N tiles of >= 16 channels, n_split K ranges
    if ((out.voxels() / 128 + 1) * (p.Cout / 16 + 1) * (p.n_split > 1 ? p.n_split : 1) >= k31)
      return "the implicit GEMM's grid has 2^31 blocks or more";
  }
  return nullptr;
}

// One conv call: the conv, its tensors and layouts, and the scratch offered for split-K sums (none: no split).
struct ConvCall {
  const Conv* conv;
  Shape5 in;                 // of x (and x2)
  const void *x, *x2, *res;  // x2: the dual projection's second input; res: the residual added to y; or nullptr
  void* y;
  bool relu;
  int x_c8, y_c8;
  void* scratch;
  size_t scratch_bytes;
};

// What decide_conv decided about a call: all launch_built needs, and all clasfv_forward_plan records.
struct ConvBuilt {
  const Conv* conv;
  const KernelInfo* kernel;  // the kKernels row, from the moment it is chosen: also of a call refused after that
  ConvParams p;              // what the launcher takes
  Shape5 out;
  int split_asked;  // the split-K factor the per-clip rule asked for (p.n_split is the one granted)
  int mt, bn;       // the implicit GEMMs' tile
};

// MFMA work of the launch decide_conv built: the kernel row's count, over conv_dma_x3's 256-row M tiles
// where its launcher takes the wide form.
double built_xgflop(const ConvBuilt& b) {
  if (b.kernel->id == K_DMA_X3 && dma_x3_wide_ok(b.p)) return xg_dma_x3_rows(*b.conv, b.out, 256.0);
  return b.kernel->xgflop(*b.conv, b.out);
}

// Decides how call cc runs on an engine with tuning tu and padding source zero_block: b is the kernel pick_kernel
// chooses and its launch. A shape that kernel cannot address is refused (CLASFV_EBADSHAPE). Launches nothing.
int decide_conv(const ConvCall& cc, const void* zero_block, const Tuning& tu, ConvBuilt& b) {
  const Conv& c = *cc.conv;
  const Shape5& in = cc.in;
  b = ConvBuilt{&c};
  if (in.c != c.cin_p) return fail(CLASFV_EINVAL, "internal: channel mismatch");
  Shape5& out = b.out;
  ConvParams& p = b.p = conv_params(c, in, out);
  p.vflags = tu.vflags, p.patch_nt = tu.patch_nt;
  p.x = cc.x, p.x2 = cc.x2, p.res = cc.res, p.y = cc.y, p.zero = zero_block;
  p.relu = cc.relu ? 1 : 0, p.x_c8 = cc.x_c8, p.y_c8 = cc.y_c8;
  // the kernel of one clip of the shape, whatever the batch (conv_size_error)
  ConvParams p1 = p;
  p1.N = 1, p1.M = (int)(out.voxels() / out.n);
  const KernelInfo& k = kKernels[pick_kernel(c, p1)];
  const Kernel kn = pick_kernel(c, p);
  b.kernel = &k;
  if (const char* why = conv_size_error(k.id, kn, in, out))
    return fail(CLASFV_EBADSHAPE, std::string(k.name) + ": " + why + " (N=" + std::to_string(in.n) + " T=" +
                                      std::to_string(in.t) + " H=" + std::to_string(in.h) + " W=" + std::to_string(in.w) +
                                      " C=" + std::to_string(in.c) + ")");
  if ((p.y_c8 && !k.writes_c8) || (p.x_c8 && !k.reads_c8))
    return fail(CLASFV_EINVAL, "internal: 8-channel-blocked layout on an unsupported kernel");
  if (p.x_c8 && k.id == K_WINOT && !winot_c8_ok(p))  // only launch_winot's conv_winot5 form reads the layout
    return winot_c8_ok(p1) ? fail(CLASFV_EBADSHAPE, "conv_winot: the 8-channel-blocked input has 2^32 bytes or more")
                           : fail(CLASFV_EINVAL, "internal: 8-channel-blocked layout on an unsupported kernel");
  p.w = c.img[k.image];
  b.mt = 2, b.bn = 0;
  int asked = 1;  // split-K on the smallest maps (per-clip shape rule), partial sums in the caller's scratch
  if (k.id == K_WINOT) {
    asked = winot_split_for(p);
  } else if (k.id == K_DMA_X3) {
    asked = dma_split_for(p, 2);
  } else if (k.id == K_DMA_W || k.id == K_DMA) {
    conv_pick_tile(p.M, c.cout_p, tu.conv_nt, &b.mt, &b.bn);
    asked = dma_split_for(p, b.mt);
  }
  // A caller that offers no scratch asks for no split (clasfv_run_conv's contract, and the walk's for every
  // conv that does not read MID); one that offers it is owed the rule's factor, and a scratch too small
  // for the sums shows as split_asked > n_split in the plan (tests/plan_audit.py, check E).
  if (!cc.scratch) asked = 1;
  split_k(p, asked, cc.scratch, cc.scratch_bytes);
  b.split_asked = asked > 1 ? asked : 1;
  if (const char* why = gemm_size_error(k, p, in, out)) return fail(CLASFV_EBADSHAPE, std::string(k.name) + ": " + why);
  return CLASFV_OK;
}

// Launches what decide_conv decided on stream s.
int launch_built(const ConvBuilt& b, hipStream_t s) {
  const Conv& c = *b.conv;
  const ConvParams& p = b.p;
  const int mt = b.mt, bn = b.bn;
  switch (b.kernel->id) {  // no default: a Kernel without a launch is a compiler warning
    case K_WINO4R: HIP_TRY(launch_wino4r(p, s)); break;
    case K_WINO4W: HIP_TRY(launch_wino4w(p, s)); break;
    case K_WINO4: HIP_TRY(launch_wino4(p, s)); break;
    case K_WINO_Q: HIP_TRY(launch_winoq(p, s)); break;
    case K_WINO: HIP_TRY(launch_wino(p, s)); break;
    case K_STEM_BF16: HIP_TRY(launch_stem_bf16(p, s)); break;
    case K_STEM_X3: HIP_TRY(launch_stem_x3(p, s)); break;
    case K_WINOT: HIP_TRY(launch_winot(p, s)); break;
    case K_PATCH_BF16: HIP_TRY(launch_patch_bf16(p, s)); break;
    case K_PATCH32_BF16: HIP_TRY(launch_patch32_bf16(p, s)); break;
    case K_TWALK_BF16: HIP_TRY(launch_twalk_bf16(p, s)); break;
    case K_PROJ_X3: HIP_TRY(launch_proj_x3(p, s)); break;
    case K_DMA_X3: HIP_TRY(launch_dma_x3(p, dma_x3_bn(c.cout_p), s)); break;
    case K_STEM_F32: HIP_TRY(launch_conv(p, 2, c.cout_p, s)); break;  // one N tile (48 fp32 / 64 bf16 channels)
    case K_DMA_W:
    case K_DMA: HIP_TRY(launch_conv(p, mt, bn, s)); break;
  }
  return CLASFV_OK;
}

// Workspace layout for one (N,T,H,W).
struct Layout {
  size_t off[32];
  size_t bytes[32];  // of each buffer, without the slack up to the next one
  size_t total;
};
enum Buf { XIN, S0, X0, MID, TA, DSB, L1A, L1, L2A, L2, L3A, L3, L4A, L4, P01, PP2, PP3, PP4, DIDX, NBUF };
constexpr const char* kBufNames[NBUF] = {"XIN", "S0",  "X0", "MID", "TA",  "DSB", "L1A", "L1",  "L2A", "L2",
                                         "L3A", "L3",  "L4A", "L4", "P01", "PP2", "PP3", "PP4", "DIDX"};

void make_layout(int N, int T, int H, int W, Layout& L) {
  const size_t T1 = T, H2 = H / 2, W2 = W / 2;
  size_t sz[NBUF];
  sz[XIN] = (size_t)N * T * H * W * 4;
  sz[S0] = (size_t)N * T1 * H2 * W2 * 48;
  sz[X0] = (size_t)N * T1 * H2 * W2 * 64;
  const size_t l1 = (size_t)N * T1 * H2 * W2 * 64;
  const size_t l2 = (size_t)N * (T / 2) * (H / 4) * (W / 4) * 128;
  const size_t l3 = (size_t)N * (T / 4) * (H / 8) * (W / 8) * 256;
  const size_t l4 = (size_t)N * (T / 8) * (H / 16) * (W / 16) * 512;
  size_t mid = (size_t)N * T1 * H2 * W2 * 144;
  mid = std::max(mid, (size_t)N * T1 * (H / 4) * (W / 4) * 240);
  mid = std::max(mid, (size_t)N * (T / 2) * (H / 8) * (W / 8) * 480);
  mid = std::max(mid, (size_t)N * (T / 4) * (H / 16) * (W / 16) * 960);
  sz[MID] = mid;
  sz[TA] = std::max(std::max(l1, l2), std::max(l3, l4));
  sz[DSB] = std::max(l2, std::max(l3, l4));
  sz[L1A] = sz[L1] = l1;
  sz[L2A] = sz[L2] = l2;
  sz[L3A] = sz[L3] = l3;
  sz[L4A] = sz[L4] = l4;
  sz[P01] = (size_t)N * T1 * H2 * W2 * 64;
  sz[PP2] = (size_t)N * (T / 2) * (H / 4) * (W / 4) * 64;
  sz[PP3] = (size_t)N * (T / 4) * (H / 8) * (W / 8) * 64;
  sz[PP4] = (size_t)N * (T / 8) * (H / 16) * (W / 16) * 64;
  sz[DIDX] = decoder_index_bytes(T, H, W) / sizeof(float);  // the decoder's source-index table
  size_t o = 0;
  for (int i = 0; i < NBUF; ++i) {
    L.off[i] = o;
    L.bytes[i] = sz[i] * sizeof(float);
    o += (L.bytes[i] + 255) / 256 * 256;
  }
  L.total = o;
}

// Record one timing event on s (pool grows on demand); returns its index or -1 on failure.
int tick(clasfv_engine* h, hipStream_t s) {
  if (h->nev == (int)h->evs.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return -1;
    h->evs.push_back(e);
  }
  if (hipEventRecord(h->evs[h->nev], s) != hipSuccess) return -1;
  return h->nev++;
}

float tap_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// The decoder's parameters over four tap projections (tap[i] of shape tsh[i]) for an (N, T, H, W)
// output; idx is the launch's index table (decoder_index_bytes(T, H, W) of device memory).
DecParams decoder_params(const clasfv_engine* h, const float* const tap[4], const Shape5 tsh[4], float* seg, float* mot,
                         int N, int T, int H, int W, void* idx) {
  DecParams d{};
  for (int i = 0; i < 4; ++i) {
    d.tap[i].p = tap[i];
    d.tap[i].T = tsh[i].t;
    d.tap[i].H = tsh[i].h;
    d.tap[i].W = tsh[i].w;
    d.tap[i].st = tap_scale(tsh[i].t, T);
    d.tap[i].sh = tap_scale(tsh[i].h, H);
    d.tap[i].sw = tap_scale(tsh[i].w, W);
  }
  d.b1 = h->b1;
  d.w2 = h->w2;
  d.b2 = h->b2;
  d.wh = h->wh;
  d.bh = h->bh;
  d.seg = seg;
  d.mot = mot;
  d.N = N, d.T = T, d.H = H, d.W = W;
  d.bf16 = h->dtype == CLASFV_DTYPE_BF16 && !(h->tune.vflags & CLASFV_VARIANT_NO_DECODER_BF16);
  d.w2x3 = h->w2x3;
  d.x3 = h->dtype != CLASFV_DTYPE_BF16 && !(h->tune.vflags & CLASFV_VARIANT_NO_DECODER_X3);
  d.idx = idx;
  return d;
}

// Makes the handle's device current for the scope of an ABI call and restores the caller's.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

#define DEVICE_GUARD(dev)                                                                       \
  DeviceGuard _guard(dev);                                                                      \
  if (_guard.err != hipSuccess)                                                                 \
    return fail(CLASFV_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(_guard.err))

// The forward context of launch stream s, or nullptr when the stream has none yet.
clasfv_engine::Ctx* find_ctx(const clasfv_engine* h, hipStream_t s) {
  for (auto* c : h->ctxs)
    if (c->stream == s) return c;
  return nullptr;
}

// The forward context of launch stream s with an arena of at least `bytes`: created on first use; past
// kMaxCtx streams the least recently used one is taken over once the device is idle (no queued work
// can still be using its arena).
int acquire_ctx(clasfv_engine* h, hipStream_t s, size_t bytes, clasfv_engine::Ctx** out) {
  clasfv_engine::Ctx* cx = find_ctx(h, s);
  if (!cx) {
    constexpr size_t kMaxCtx = 4;
    if (h->ctxs.size() < kMaxCtx) {
      cx = new clasfv_engine::Ctx();
      h->ctxs.push_back(cx);
    } else {
      HIP_TRY(hipDeviceSynchronize());
      cx = h->ctxs.front();
      for (auto* c : h->ctxs)
        if (c->last_use < cx->last_use) cx = c;
    }
    cx->stream = s;
  }
  cx->last_use = ++h->ctx_clock;
  if (bytes > cx->arena_bytes) {
    // The arena may still be in use by work queued earlier on its stream.
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(cx->arena);
    cx->arena = nullptr;
    cx->arena_bytes = 0;
    HIP_TRY(hipMalloc(&cx->arena, bytes));
    cx->arena_bytes = bytes;
  }
  *out = cx;
  return CLASFV_OK;
}

// Conv i of the diagnostics' numbering: the backbone convs in execution order, then the decoder
// projections proj[0], proj[2], proj[3], proj[4] (tap index in *tap; -1 for a backbone conv).
const Conv* probe_conv(const clasfv_engine* h, int i, int* tap) {
  static const int kTap[4] = {0, 2, 3, 4};
  const int nb = (int)h->convs.size();
  if (i < 0 || i >= nb + 4) return nullptr;
  if (tap) *tap = i < nb ? -1 : kTap[i - nb];
  return i < nb ? &h->convs[i] : &h->proj[kTap[i - nb]];
}

// The diagnostics' index of a conv of h (probe_conv's numbering).
int conv_index(const clasfv_engine* h, const Conv& c) {
  const int nb = (int)h->convs.size();
  if (&c >= h->convs.data() && &c < h->convs.data() + nb) return (int)(&c - h->convs.data());
  const int i = (int)(&c - h->proj);
  return nb + (i == 0 ? 0 : i - 1);
}

// The instantiation label of a kernel function: the name the compiler registered it under with the HIP
// runtime, demangled, without the anonymous namespace, the return type and the parameter list:
// "_ZN12_GLOBAL__N_111conv_winot5ILi4ELi4ELi2EEEv10ConvParamsiii7FastDiv" -> "conv_winot5<4, 4, 2>".
std::string label_of(const void* kernel) {
  const char* mangled = hipKernelNameRefByPtr(kernel, nullptr);
  if (!mangled) return "?";
  // the C++ runtime's demangler may predate __bf16's code (DF16b): hand it the half type's (Dh; both are
  // builtin types, so no substitution index moves; no kernel here takes a half) and rename it after
  std::string m(mangled);
  for (size_t a; (a = m.find("DF16b")) != std::string::npos;) m.replace(a, 5, "Dh");
  int status = 0;
  char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &status);
  std::string t(d && status == 0 ? d : mangled);
  free(d);
  for (size_t a; (a = t.find("half")) != std::string::npos;) t.replace(a, 4, "__bf16");
  const std::string anon = "(anonymous namespace)::";
  for (size_t a; (a = t.find(anon)) != std::string::npos;) t.erase(a, anon.size());
  if (t.compare(0, 5, "void ") == 0) t.erase(0, 5);  // a template instantiation's return type
  const size_t lt = t.find('<'), par = t.find('(');
  if (lt != std::string::npos && lt < par) {  // keep through the '>' that closes the template arguments
    int depth = 0;
    for (size_t i = lt; i < t.size(); ++i) {
      if (t[i] == '<') ++depth;
      if (t[i] == '>' && --depth == 0) return t.substr(0, i + 1);
    }
  }
  return t.substr(0, par);
}

// The launch log around one launcher call: log_begin empties the thread's ring, log_end appends what the
// launcher noted (in launch order) to the handle's log.
constexpr size_t kMaxLog = 1 << 16;  // a log nobody reads stops growing here
void log_begin(const clasfv_engine* h) {
  if (h->llog) g_launch_ring.n = 0;
}
void log_end(clasfv_engine* h, int conv) {
  if (!h->llog) return;
  const LaunchRing& r = g_launch_ring;
  for (unsigned i = 0; i < r.n && i < 4 && h->log.size() < kMaxLog; ++i) {
    auto it = h->labels.find(r.e[i].kernel);
    if (it == h->labels.end()) it = h->labels.emplace(r.e[i].kernel, label_of(r.e[i].kernel)).first;
    h->log.push_back({it->second.c_str(), r.e[i].grid, r.e[i].passes, conv});
  }
}

// decide_conv and, unless it refuses the call, launch_built on s with the launch log around it.
int run_conv(clasfv_engine* h, const ConvCall& cc, hipStream_t s, ConvBuilt& b) {
  if (int rc = decide_conv(cc, h->zero, h->tune, b)) return rc;
  log_begin(h);
  const int rc = launch_built(b, s);
  log_end(h, conv_index(h, *cc.conv));
  return rc;
}

// The network's launches over n clips of (T, H, W), in forward order, on a workspace laid out by L at
// `arena`: pack(xin) packs the input, run(call, out) and run_side(call, out) run one ConvCall and give its
// output shape (the latter a decoder projection that may overlap layer4 until join()), decode(taps, shapes,
// idx) runs the decoder. Each returns a CLASFV code, and the first failure ends the walk. clasfv_forward
// launches through it; the plan walks it with runners that decide every launch and launch none.
template <class Pack, class Run, class RunSide, class Join, class Decode>
int walk_network(const clasfv_engine* h, const Layout& L, char* arena, int N, int T, int H, int W, Pack pack, Run run_,
                 RunSide run_side_, Join join, Decode decode) {
  auto buf = [&](int b) { return reinterpret_cast<void*>(arena + L.off[b]); };
  // scratch for a temporal conv reading MID: the rest of MID past its input
  const size_t mid_bytes = L.off[MID + 1] - L.off[MID];
  auto run = [&](const Conv& c, const void* xin, const Shape5& in, void* y, Shape5& out, const void* res, bool relu,
                 int x_c8, int y_c8) {
    ConvCall cc{&c, in, xin, nullptr, res, y, relu, x_c8, y_c8, nullptr, 0};
    // Which convs may split is a property of the walk, not of sizes: those that read MID (the temporal
    // convs) are offered what is left of it, even when that is nothing, and no other conv is offered any.
    if (xin == buf(MID)) {
      const size_t used =
          std::min(mid_bytes, ((size_t)in.n * in.t * in.h * in.w * in.c * sizeof(float) + 255) / 256 * 256);
      cc.scratch = arena + L.off[MID] + used;
      cc.scratch_bytes = mid_bytes - used;
    }
    return run_(cc, out);
  };
  auto run_side = [&](const Conv& c, const void* xin, const Shape5& in, void* y, Shape5& out, const void* x2) {
    return run_side_(ConvCall{&c, in, xin, x2, nullptr, y, false, 0, 0, nullptr, 0}, out);
  };
  int rc;
  if ((rc = pack(buf(XIN)))) return rc;
  Shape5 sx{N, T, H, W, 4}, s0, sx0;
  Shape5 sp, sp2, sp3, sp4;  // decoder tap projections
  size_t ci = 0;
  // Conv2Plus1D mid tensors (and the stem's) are 8-channel-blocked where c8_pair allows
  const int c8s = c8_pair(h->convs[0], h->convs[1], sx, h->tune);
  if ((rc = run(h->convs[ci++], buf(XIN), sx, buf(S0), s0, nullptr, true, 0, c8s))) return rc;
  if ((rc = run(h->convs[ci++], buf(S0), s0, buf(X0), sx0, nullptr, true, c8s, 0))) return rc;
  const int outs[4][2] = {{L1A, L1}, {L2A, L2}, {L3A, L3}, {L4A, L4}};
  void* cur = buf(X0);
  Shape5 cs = sx0, taps_shape[5];
  void* taps[5];
  taps[0] = cur;
  taps_shape[0] = cs;
  for (int li = 0; li < 4; ++li) {
    for (int b = 0; b < 2; ++b) {
      const Conv& sp1 = h->convs[ci++];
      const Conv& tp1 = h->convs[ci++];
      const Conv& sp2 = h->convs[ci++];
      const Conv& tp2 = h->convs[ci++];
      const Conv* ds = (ci < h->convs.size() && h->convs[ci].role == DS) ? &h->convs[ci++] : nullptr;
      Shape5 sm, sa, sm2, so, sd;
      const int c8a = c8_pair(sp1, tp1, cs, h->tune);
      if ((rc = run(sp1, cur, cs, buf(MID), sm, nullptr, true, 0, c8a))) return rc;
      if ((rc = run(tp1, buf(MID), sm, buf(TA), sa, nullptr, true, c8a, 0))) return rc;
      const int c8b = c8_pair(sp2, tp2, sa, h->tune);
      if ((rc = run(sp2, buf(TA), sa, buf(MID), sm2, nullptr, true, 0, c8b))) return rc;
      const void* res = cur;
      if (ds) {
        if ((rc = run(*ds, cur, cs, buf(DSB), sd, nullptr, false, 0, 0))) return rc;
        res = buf(DSB);
      }
      void* out = buf(outs[li][b]);
      if ((rc = run(tp2, buf(MID), sm2, out, so, res, true, c8b, 0))) return rc;
      cur = out;
      cs = so;
    }
    taps[li + 1] = cur;
    taps_shape[li + 1] = cs;
    // decoder projections at tap resolution (P01 = W0 f0 + W1 f1, P2, P3) on the side stream while
    // layer4 runs: its convs (600-920 blocks for 30 clips, 1.2-1.8 rounds of the chip's block slots)
    // leave CUs idle that the projections fill (forked earlier, P01 only shared layer2's full grids:
    // r03i trace, no gain); P4 after layer4 on s
    if (li == 2) {
      if ((rc = run_side(h->proj[0], taps[0], taps_shape[0], buf(P01), sp, taps[1]))) return rc;
      if ((rc = run_side(h->proj[2], taps[2], taps_shape[2], buf(PP2), sp2, nullptr))) return rc;
      if ((rc = run_side(h->proj[3], taps[3], taps_shape[3], buf(PP3), sp3, nullptr))) return rc;
    }
  }
  if ((rc = run(h->proj[4], taps[4], taps_shape[4], buf(PP4), sp4, nullptr, false, 0, 0))) return rc;
  if ((rc = join())) return rc;  // the side stream's projections are complete before the decoder

  const Shape5 tsh[4] = {sp, sp2, sp3, sp4};
  const int tb[4] = {P01, PP2, PP3, PP4};
  const float* tp[4];
  for (int i = 0; i < 4; ++i) tp[i] = reinterpret_cast<const float*>(buf(tb[i]));
  return decode(tp, tsh, buf(DIDX));
}

// The sub-batches of an N-clip call whose passes take nb clips each: body(sub, n0, n, L) for clips
// [n0, n0 + n) on the layout L of a forward of n clips. The last, shorter sub-batch runs in the layout
// of a forward of its own size (it fits the arena, which is sized for nb). The first failure ends the
// loop. clasfv_forward launches through it and clasfv_forward_plan records through it.
template <class Body>
int for_sub_batches(int N, int nb, int T, int H, int W, Body body) {
  Layout L;
  make_layout(nb, T, H, W, L);
  int sub = 0;
  for (int n0 = 0; n0 < N; n0 += nb, ++sub) {
    const int n = std::min(nb, N - n0);
    if (n != nb) make_layout(n, T, H, W, L);
    if (int rc = body(sub, n0, n, L)) return rc;
  }
  return CLASFV_OK;
}

// Where the clips of a sub-batch that starts at clip n0 begin in the caller's tensors, in elements.
struct CallerOffsets {
  size_t x, seg, mot;
};
CallerOffsets caller_offsets(int n0, int T, int H, int W) {
  const size_t clip = (size_t)T * H * W;
  return {(size_t)n0 * 3 * clip, (size_t)n0 * 2 * clip, (size_t)n0 * 4 * clip};
}

// ---- the launch plan (clasfv_forward_plan, max_clips) ---------------------------------------------------
// clasfv_forward's sub-batch loop and walk with runners that record instead of launching: decide_conv hands
// back the ConvParams the launcher would take, and every range below is what those parameters (or the
// decoder's) make the kernel address. No memory is behind the addresses (only pointer identity and
// null-ness are read). The first launch outside its kernel's limits ends the walk (CLASFV_EBADSHAPE).
struct PlanRecorder {
  std::vector<clasfv_plan_launch_t> launches;
  std::vector<clasfv_plan_buffer_t> buffers;
};

// Sub-batch `sub` of a call: clips [n0, n0 + n) on the layout L of a forward of n clips.
int plan_sub_batch(const clasfv_engine* h, PlanRecorder& rec, int sub, int n0, int n, int T, int H, int W,
                   const Layout& L) {
  char* const arena = reinterpret_cast<char*>(256);
  bool side_pending = false;  // SideJoin::pending of clasfv_forward
  for (int b = 0; b < NBUF; ++b)
    rec.buffers.push_back({sub, n, b, 0, kBufNames[b], (int64_t)L.off[b], (int64_t)L.bytes[b], (int64_t)L.total});
  auto launch = [&](int stream, int kind, int conv, const char* kernel) -> clasfv_plan_launch_t& {
    clasfv_plan_launch_t l{};
    l.sub_batch = sub, l.stream = stream, l.kind = kind, l.conv = conv, l.kernel = kernel;
    l.split_asked = l.split_granted = 1;
    l.x_elem = l.y_elem = 4;
    rec.launches.push_back(l);
    return rec.launches.back();
  };
  auto add = [&](clasfv_plan_launch_t& l, int buffer, int role, int write, int64_t offset, int64_t bytes) {
    if (l.n_ranges < CLASFV_PLAN_MAX_RANGES) l.range[l.n_ranges++] = {buffer, role, write, 0, offset, bytes};
  };
  // a range of the arena: the buffer is the one its first byte lies in
  auto add_arena = [&](clasfv_plan_launch_t& l, const void* p, int role, int write, int64_t bytes) {
    const int64_t off = reinterpret_cast<const char*>(p) - arena;
    int b = 0;
    while (b + 1 < NBUF && off >= (int64_t)L.off[b + 1]) ++b;
    add(l, b, role, write, off, bytes);
  };
  const CallerOffsets at = caller_offsets(n0, T, H, W);
  const int64_t clip = (int64_t)T * H * W;
  auto pack = [&](void* xin) {
    clasfv_plan_launch_t& l = launch(0, CLASFV_PLAN_PACK, -1, "pack_input_kernel");
    add(l, CLASFV_PLAN_EXT_CLIP, CLASFV_PLAN_X, 0, (int64_t)at.x * 4, (int64_t)n * 3 * clip * 4);
    add_arena(l, xin, CLASFV_PLAN_Y, 1, (int64_t)n * clip * 4 * 4);  // launch_pack_input: 3 + 1 fp32 channels
    return (int)CLASFV_OK;
  };
  auto conv = [&](int stream, const ConvCall& cc, Shape5& out) {
    ConvBuilt cb;
    if (int rc = decide_conv(cc, arena, h->tune, cb)) return rc;
    out = cb.out;
    const ConvParams& p = cb.p;
    const int xe = p.in_bf16 ? 2 : 4, ye = p.out_bf16 ? 2 : 4;
    const int64_t vin = (int64_t)p.N * p.Ti * p.Hi * p.Wi, m = (int64_t)p.N * p.To * p.Ho * p.Wo;
    const int64_t part = (int64_t)p.n_split * m * p.Cout * 4;
    const bool split = p.n_split > 1;
    const int index = conv_index(h, *cc.conv);
    clasfv_plan_launch_t& l = launch(stream, CLASFV_PLAN_CONV, index, cb.kernel->name);
    auto describe = [&](clasfv_plan_launch_t& d) {
      d.split_asked = cb.split_asked, d.split_granted = split ? p.n_split : 1;
      d.x_c8 = p.x_c8, d.y_c8 = p.y_c8, d.relu = p.relu, d.has_res = p.res != nullptr;
      d.x_elem = xe, d.y_elem = ye;
    };
    auto epilogue = [&](clasfv_plan_launch_t& d) {  // what the launch that writes y addresses beside its sums
      if (p.res) add_arena(d, p.res, CLASFV_PLAN_RES, 0, m * p.Cout * ye);
      add_arena(d, p.y, CLASFV_PLAN_Y, 1, m * p.Cout * ye);
    };
    describe(l);
    add_arena(l, p.x, CLASFV_PLAN_X, 0, vin * p.Cin * xe);
    if (p.x2) add_arena(l, p.x2, CLASFV_PLAN_X2, 0, vin * p.Cin2 * xe);
    if (!split) {
      epilogue(l);
      return (int)CLASFV_OK;
    }
    add_arena(l, p.part, CLASFV_PLAN_PART, 1, part);
    clasfv_plan_launch_t& ssum = launch(stream, CLASFV_PLAN_SPLIT_SUM, index, "split_sum_kernel");
    describe(ssum);
    add_arena(ssum, p.part, CLASFV_PLAN_PART, 0, part);
    epilogue(ssum);
    return (int)CLASFV_OK;
  };
  auto run = [&](const ConvCall& cc, Shape5& out) { return conv(0, cc, out); };
  auto run_side = [&](const ConvCall& cc, Shape5& out) {
    launch(1, CLASFV_PLAN_FORK, -1, "");  // ev_fork recorded on s, awaited by the side stream
    side_pending = true;
    return conv(1, cc, out);
  };
  auto join = [&]() {
    if (side_pending) launch(0, CLASFV_PLAN_JOIN, -1, "");  // ev_join recorded on the side stream, awaited by s
    side_pending = false;
    return (int)CLASFV_OK;
  };
  auto decode = [&](const float* const tp[4], const Shape5 tsh[4], void* idx) {
    const DecParams d = decoder_params(h, tp, tsh, nullptr, nullptr, n, T, H, W, idx);
    if (!decoder_addressable(d)) return fail(CLASFV_EBADSHAPE, "decoder_kernel: a tap has 2^31 floats or more");
    const int64_t table = (int64_t)decoder_index_bytes(d.T, d.H, d.W);
    clasfv_plan_launch_t& li = launch(0, CLASFV_PLAN_DEC_INDEX, -1, "decoder_index_kernel");
    add_arena(li, d.idx, CLASFV_PLAN_IDX, 1, table);
    clasfv_plan_launch_t& l = launch(0, CLASFV_PLAN_DECODER, -1, "decoder_kernel");
    for (int i = 0; i < 4; ++i)
      add_arena(l, d.tap[i].p, CLASFV_PLAN_TAP, 0, (int64_t)d.N * d.tap[i].T * d.tap[i].H * d.tap[i].W * 64 * 4);
    add_arena(l, d.idx, CLASFV_PLAN_IDX, 0, table);
    add(l, CLASFV_PLAN_EXT_SEG, CLASFV_PLAN_Y, 1, (int64_t)at.seg * 4, (int64_t)d.N * 2 * clip * 4);
    add(l, CLASFV_PLAN_EXT_MOTION, CLASFV_PLAN_Y, 1, (int64_t)at.mot * 4, (int64_t)d.N * 4 * clip * 4);
    return (int)CLASFV_OK;
  };
  return walk_network(h, L, arena, n, T, H, W, pack, run, run_side, join, decode);
}

// Whether every launch of a forward over N clips of (T, H, W) is inside its kernel's limits (a CLASFV
// code; the refusal's reason in clasfv_last_error): its plan as one pass, kept by nobody.
int forward_fits(const clasfv_engine* h, int N, int T, int H, int W) {
  if ((int64_t)N * T * H * W >= ((int64_t)1 << 31)) return fail(CLASFV_EBADSHAPE, "the clips have 2^31 voxels or more");
  Layout L;
  make_layout(N, T, H, W, L);
  PlanRecorder unread;
  return plan_sub_batch(h, unread, 0, 0, N, T, H, W, L);
}

// The largest N for which forward_fits (0: not even one clip; the reason stays in clasfv_last_error).
// Every limit is an upper bound on a size that grows with N, so the fitting N are 1 .. max_clips.
int max_clips(const clasfv_engine* h, int T, int H, int W) {
  if (forward_fits(h, 1, T, H, W)) return 0;
  int64_t lo = 1, hi = ((int64_t)1 << 31) / ((int64_t)T * H * W) + 1;  // fits(lo), !fits(hi)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) / 2;
    (forward_fits(h, (int)mid, T, H, W) == CLASFV_OK ? lo : hi) = mid;
  }
  return (int)lo;
}

int forward_plan(const clasfv_engine* h, int N, int T, int H, int W, PlanRecorder& rec) {
  const int nb = std::min(N, max_clips(h, T, H, W));
  if (nb < 1) return forward_fits(h, 1, T, H, W);
  return for_sub_batches(N, nb, T, H, W, [&](int sub, int n0, int n, const Layout& L) {
    return plan_sub_batch(h, rec, sub, n0, n, T, H, W, L);
  });
}

}  // namespace

extern "C" {

const char* clasfv_last_error(void) { return g_err.c_str(); }
int clasfv_version(void) { return CLASFV_ABI_VERSION; }
#ifndef CLASFV_SOURCE_HASH
#define CLASFV_SOURCE_HASH "unhashed"
#endif
const char* clasfv_source_hash(void) { return "clasfv-source-hash:" CLASFV_SOURCE_HASH; }

int clasfv_create(int device, clasfv_t* out) {
  if (!out) return fail(CLASFV_EINVAL, "null out");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(CLASFV_EINVAL, "bad device index");
  auto* e = new clasfv_engine();
  e->device = device;
  e->tune.vflags = env_variants();
  e->tune.conv_nt = env_int("CLASFV_CONV_NT");
  e->tune.patch_nt = env_int("CLASFV_PATCH_NT");
  build_plan(e);
  *out = e;
  return CLASFV_OK;
}

int clasfv_destroy(clasfv_t h) {
  if (!h) return CLASFV_OK;
  DeviceGuard guard(h->device);
  for (auto& c : h->convs) free_conv_images(c);
  for (auto& c : h->proj) free_conv_images(c);
  for (auto* c : h->ctxs) {
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    (void)hipFree(c->arena);
    delete c;
  }
  (void)hipFree(h->b1);
  (void)hipFree(h->w2);
  (void)hipFree(h->w2x3);
  (void)hipFree(h->b2);
  (void)hipFree(h->wh);
  (void)hipFree(h->bh);
  (void)hipFree(h->zero);
  for (auto e : h->evs) (void)hipEventDestroy(e);
  delete h;
  return CLASFV_OK;
}

int clasfv_param_count(clasfv_t h) { return h ? (int)h->params.size() : CLASFV_EINVAL; }

int clasfv_param_info(clasfv_t h, int i, const char** name, int* ndim, int64_t dims[5]) {
  if (!h || i < 0 || i >= (int)h->params.size()) return fail(CLASFV_EINVAL, "bad param index");
  const Param& p = h->params[i];
  if (name) *name = p.name.c_str();
  if (ndim) *ndim = (int)p.shape.size();
  if (dims)
    for (size_t d = 0; d < p.shape.size(); ++d) dims[d] = p.shape[d];
  return CLASFV_OK;
}

int clasfv_load_param(clasfv_t h, const char* name, const float* data, int64_t numel) {
  if (!h || !name) return fail(CLASFV_EINVAL, "null argument");
  std::string n(name);
  if (n.rfind("module.", 0) == 0) n = n.substr(7);
  auto it = h->index.find(n);
  if (it == h->index.end()) return fail(CLASFV_EINVAL, "unknown parameter: " + n);
  Param& p = h->params[it->second];
  if (n.size() > 20 && n.compare(n.size() - 20, 20, ".num_batches_tracked") == 0) {
    p.loaded = true;
    return CLASFV_OK;
  }
  if (numel != p.numel()) return fail(CLASFV_EINVAL, "size mismatch for " + n);
  if (!data) return fail(CLASFV_EINVAL, "null data");
  p.data.assign(data, data + numel);
  p.loaded = true;
  h->ready = false;
  return CLASFV_OK;
}

int clasfv_finalize(clasfv_t h) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  for (const auto& p : h->params)
    if (!p.loaded && p.name.find(".fc.") == std::string::npos)
      return fail(CLASFV_ENOTREADY, "parameter not loaded: " + p.name);
  DEVICE_GUARD(h->device);
  // forwards still in flight on any stream read the weight images replaced below
  HIP_TRY(hipDeviceSynchronize());
  const bool bf16 = h->dtype == CLASFV_DTYPE_BF16;
  for (auto& c : h->convs) layout_conv(c, bf16);
  for (auto& c : h->proj) layout_conv(c, bf16);
  for (auto& c : h->convs)
    if (int rc = finalize_conv(h, c, bf16)) return rc;
  if (int rc = finalize_projections(h)) return rc;
  if (int rc = finalize_decoder(h)) return rc;
  if (!h->zero) {
    HIP_TRY(hipMalloc(&h->zero, 256));
    HIP_TRY(hipMemset(h->zero, 0, 256));
  }
  HIP_TRY(hipDeviceSynchronize());
  h->clip_limit.clear();
  h->ready = true;
  return CLASFV_OK;
}

int64_t clasfv_workspace_bytes(clasfv_t h) {
  if (!h) return 0;
  int64_t b = 0;
  for (auto* c : h->ctxs) b += (int64_t)c->arena_bytes;
  return b;
}

int clasfv_set_compute_dtype(clasfv_t h, int dtype) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  if (dtype != CLASFV_DTYPE_FP32 && dtype != CLASFV_DTYPE_BF16) return fail(CLASFV_EINVAL, "unknown dtype");
  if (dtype != h->dtype) {
    h->dtype = dtype;
    h->ready = false;  // weights must be re-laid-out: call clasfv_finalize again
    h->clip_limit.clear();
  }
  return CLASFV_OK;
}

int clasfv_get_compute_dtype(clasfv_t h) { return h ? h->dtype : CLASFV_EINVAL; }

int clasfv_set_kernel_variants(clasfv_t h, int flags) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  if (flags & ~kVariantMask) return fail(CLASFV_EINVAL, "unknown kernel-variant bit");
  if ((flags ^ h->tune.vflags) & CLASFV_VARIANT_NO_WINOGRAD) h->ready = false;  // weight images change
  h->tune.vflags = flags;
  h->clip_limit.clear();
  return CLASFV_OK;
}

int clasfv_get_kernel_variants(clasfv_t h) { return h ? h->tune.vflags : CLASFV_EINVAL; }

// What the network's strides need of a clip: whole 8-frame and 16-pixel steps, at least one of each.
static bool clip_shape_ok(int T, int H, int W) { return T >= 8 && H >= 16 && W >= 16 && !(T % 8 || H % 16 || W % 16); }

// The plan of an engine of this dtype and these variants with every weight image clasfv_finalize would
// upload marked present: no device is touched, and nothing of it may be launched.
static int plan_only(clasfv_engine* e, int T, int H, int W, int dtype, int variants) {
  if (!clip_shape_ok(T, H, W))
    return fail(CLASFV_EBADSHAPE, "shape must satisfy T % 8 == 0, H % 16 == 0, W % 16 == 0");
  if (dtype != CLASFV_DTYPE_FP32 && dtype != CLASFV_DTYPE_BF16) return fail(CLASFV_EINVAL, "unknown dtype");
  if (variants & ~kVariantMask) return fail(CLASFV_EINVAL, "unknown kernel-variant bit");
  e->dtype = dtype;
  e->tune.vflags = variants;
  build_plan(e);
  const bool bf16 = dtype == CLASFV_DTYPE_BF16;
  for (auto& c : e->convs) layout_conv(c, bf16), mark_images(c, bf16, variants);
  for (auto& c : e->proj) layout_conv(c, bf16), mark_images(c, bf16, variants);
  return CLASFV_OK;
}

int clasfv_max_clips(int T, int H, int W, int dtype, int variants) {
  clasfv_engine e;
  if (int rc = plan_only(&e, T, H, W, dtype, variants)) return rc;
  return max_clips(&e, T, H, W);
}

int clasfv_clips_fit(int N, int T, int H, int W, int dtype, int variants) {
  if (N < 1) return fail(CLASFV_EINVAL, "N must be >= 1");
  clasfv_engine e;
  if (int rc = plan_only(&e, T, H, W, dtype, variants)) return rc;
  return forward_fits(&e, N, T, H, W);
}

int clasfv_forward_plan(int N, int T, int H, int W, int dtype, int variants, int cap_launches,
                        clasfv_plan_launch_t* launches, int* n_launches, int cap_buffers, clasfv_plan_buffer_t* buffers,
                        int* n_buffers) {
  if (N < 1) return fail(CLASFV_EINVAL, "N must be >= 1");
  if (cap_launches < 0 || cap_buffers < 0) return fail(CLASFV_EINVAL, "negative cap");
  clasfv_engine e;
  if (int rc = plan_only(&e, T, H, W, dtype, variants)) return rc;
  PlanRecorder rec;
  if (int rc = forward_plan(&e, N, T, H, W, rec)) return rc;
  if (n_launches) *n_launches = (int)rec.launches.size();
  if (n_buffers) *n_buffers = (int)rec.buffers.size();
  if ((launches && rec.launches.size() > (size_t)cap_launches) || (buffers && rec.buffers.size() > (size_t)cap_buffers))
    return fail(CLASFV_EINVAL, "forward plan: cap too small");
  if (launches) std::copy(rec.launches.begin(), rec.launches.end(), launches);
  if (buffers) std::copy(rec.buffers.begin(), rec.buffers.end(), buffers);
  return CLASFV_OK;
}

int clasfv_plan_conv_info(int dtype, int i, int channels[5], int kernel[3], int stride[3], int padding[3],
                          int* in_dtype, int* out_dtype) {
  if (dtype != CLASFV_DTYPE_FP32 && dtype != CLASFV_DTYPE_BF16) return fail(CLASFV_EINVAL, "unknown dtype");
  clasfv_engine e;
  e.dtype = dtype;
  build_plan(&e);
  return clasfv_conv_info(&e, i, nullptr, nullptr, nullptr, channels, kernel, stride, padding, in_dtype, out_dtype);
}

int clasfv_forward(clasfv_t h, const float* x, int N, int T, int H, int W, float* seg, float* mot, void* stream) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  if (!h->ready) return fail(CLASFV_ENOTREADY, "clasfv_finalize has not been called");
  if (!x || !seg || !mot) return fail(CLASFV_EINVAL, "null tensor");
  if (N < 1) return fail(CLASFV_EINVAL, "N must be >= 1");
  if (!clip_shape_ok(T, H, W))
    return fail(CLASFV_EBADSHAPE, "shape must satisfy T % 8 == 0, H % 16 == 0, W % 16 == 0 (got T=" +
                                      std::to_string(T) + " H=" + std::to_string(H) + " W=" + std::to_string(W) + ")");
  // The largest batch every kernel of the network can address in one pass (per handle state and clip
  // shape, kept): a larger N runs as consecutive sub-batches of that many clips. A clip's kernels, and
  // so its bits, are those of its shape whatever N is.
  const std::array<int, 3> key{T, H, W};
  auto hit = h->clip_limit.find(key);
  if (hit == h->clip_limit.end()) hit = h->clip_limit.emplace(key, max_clips(h, T, H, W)).first;
  const int nb = std::min(N, hit->second);
  if (nb < 1) return forward_fits(h, 1, T, H, W);  // one clip of the shape is past a kernel's limit: the reason
  hipStream_t s = (hipStream_t)stream;
  DEVICE_GUARD(h->device);
  Layout L;
  make_layout(nb, T, H, W, L);
  clasfv_engine::Ctx* cx = nullptr;  // this stream's context
  if (int rc_ = acquire_ctx(h, s, L.total, &cx)) return rc_;
  int last_ev = h->ktime ? tick(h, s) : -1;
  auto timed = [&](const char* name, double gflop, double xgflop) {
    if (last_ev < 0) return;
    const int e = tick(h, s);
    if (e >= 0) h->recs.push_back({name, gflop, xgflop, last_ev, e});
    last_ev = e;
  };
  if (!cx->side) {
    HIP_TRY(hipStreamCreateWithFlags(&cx->side, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&cx->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&cx->ev_join, hipEventDisableTiming));
  }
  // Once work is forked to the side stream, every exit of this call (the error returns included)
  // leaves s ordered after everything queued there, so the caller's next use of the arena or the
  // outputs cannot race the projections.
  struct SideJoin {
    clasfv_engine::Ctx* cx;
    hipStream_t s;
    bool pending = false;
    hipError_t join() {
      if (!pending) return hipSuccess;
      pending = false;
      hipError_t e = hipEventRecord(cx->ev_join, cx->side);
      return e != hipSuccess ? e : hipStreamWaitEvent(s, cx->ev_join, 0);
    }
    ~SideJoin() { (void)join(); }
  } side_join{cx, s};
  // a decoder projection on the side stream once its tap is complete on s (timed with its own events;
  // with kernel timing on, the layer4 launches on s run concurrently with these, so their event
  // intervals overlap: the per-kernel sums of a forward exceed its wall time by about the overlap)
  auto run_side = [&](const ConvCall& cc, Shape5& out) {
    HIP_TRY(hipEventRecord(cx->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(cx->side, cx->ev_fork, 0));
    side_join.pending = true;
    const int e0 = h->ktime ? tick(h, cx->side) : -1;
    ConvBuilt b;
    if (int rc_ = run_conv(h, cc, cx->side, b)) return rc_;
    out = b.out;
    if (e0 >= 0) {
      const int e1 = tick(h, cx->side);
      const Conv& c = *cc.conv;
      if (e1 >= 0) h->recs.push_back({b.kernel->name, conv_gflop(c, out), built_xgflop(b), e0, e1});
    }
    return (int)CLASFV_OK;
  };
  auto run = [&](const ConvCall& cc, Shape5& out) {
    ConvBuilt b;
    if (int rc_ = run_conv(h, cc, s, b)) return rc_;
    out = b.out;
    timed(b.kernel->name, conv_gflop(*cc.conv, out), built_xgflop(b));
    return (int)CLASFV_OK;
  };
  auto join = [&]() {
    HIP_TRY(side_join.join());
    return (int)CLASFV_OK;
  };
  return for_sub_batches(N, nb, T, H, W, [&](int, int n0, int n, const Layout& Ls) {
    const CallerOffsets at = caller_offsets(n0, T, H, W);
    const float* xs = x + at.x;
    float *segs = seg + at.seg, *mots = mot + at.mot;
    auto pack = [&](void* xin) {
      log_begin(h);
      HIP_TRY(launch_pack_input(xs, reinterpret_cast<float*>(xin), n, T, H * W, s));
      log_end(h, -1);
      timed("pack_input_kernel", 0.0, 0.0);
      return (int)CLASFV_OK;
    };
    auto decode = [&](const float* const tp[4], const Shape5 tsh[4], void* idx) {
      const DecParams d = decoder_params(h, tp, tsh, segs, mots, n, T, H, W, idx);
      log_begin(h);
      HIP_TRY(launch_decoder(d, s));
      log_end(h, -1);
      // comb_2 (64x64) and the heads (6 useful of the 16 rows of their MFMA tile) per output voxel, in the
      // products of the pipe they run on: fp32 engines six split-bf16 products each (bf16 pipe), bf16
      // engines three for comb_2 and six for the heads (bf16 pipe), the no_decoder_x3 variant one f32
      // product each (f32 pipe)
      const double dec_px = d.x3 ? 6.0 * (64 * 64 + 64 * 16) : d.bf16 ? 3.0 * 64 * 64 + 6.0 * 64 * 16 : 64 * 64 + 64 * 16;
      timed(d.x3 || d.bf16 ? "decoder_kernel" : "decoder_kernel_f32", 2.0 * n * (double)T * H * W * (64 * 64 + 64 * 6) * 1e-9,
            2.0 * n * (double)T * H * W * dec_px * 1e-9);
      return (int)CLASFV_OK;
    };
    return walk_network(h, Ls, cx->arena, n, T, H, W, pack, run, run_side, join, decode);
  });
}

int clasfv_set_kernel_timing(clasfv_t h, int enable) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  h->ktime = enable != 0;
  h->recs.clear();
  h->nev = 0;
  return CLASFV_OK;
}

int clasfv_kernel_timing(clasfv_t h, int cap, const char** names, int* launches, double* ms, double* gflop,
                         double* xgflop) {
  if (!h || cap < 0 || (cap > 0 && (!names || !launches || !ms || !gflop || !xgflop)))
    return fail(CLASFV_EINVAL, "bad argument");
  if (h->nev > 0) HIP_TRY(hipEventSynchronize(h->evs[h->nev - 1]));
  int n = 0;
  for (const auto& r : h->recs) {
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, h->evs[r.e0], h->evs[r.e1]));
    int i = 0;
    while (i < n && strcmp(names[i], r.name) != 0) ++i;
    if (i == n) {
      if (n == cap) return fail(CLASFV_EINVAL, "kernel timing: cap too small");
      names[n] = r.name;
      launches[n] = 0;
      ms[n] = gflop[n] = xgflop[n] = 0.0;
      ++n;
    }
    launches[i] += 1;
    ms[i] += t;
    gflop[i] += r.gflop;
    xgflop[i] += r.xgflop;
  }
  h->recs.clear();
  h->nev = 0;
  return n;
}

int clasfv_set_launch_log(clasfv_t h, int enable) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  h->llog = enable != 0;
  h->log.clear();
  return CLASFV_OK;
}

int clasfv_launch_log(clasfv_t h, int cap, const char** labels, int64_t* grids, int* passes, int* convs) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  if (cap < 0 || (cap > 0 && (!labels || !grids || !passes || !convs))) return fail(CLASFV_EINVAL, "bad argument");
  if (h->log.size() > (size_t)cap) return fail(CLASFV_EINVAL, "launch log: cap too small");
  const int n = (int)h->log.size();
  for (int i = 0; i < n; ++i) {
    labels[i] = h->log[i].label;
    grids[i] = h->log[i].grid;
    passes[i] = h->log[i].passes;
    convs[i] = h->log[i].conv;
  }
  h->log.clear();
  return n;
}

int clasfv_fill_workspace(clasfv_t h, int byte, void* stream) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  if (byte < 0 || byte > 255) return fail(CLASFV_EINVAL, "fill byte must be in [0, 255]");
  hipStream_t s = (hipStream_t)stream;
  const clasfv_engine::Ctx* cx = find_ctx(h, s);
  if (!cx || !cx->arena) return fail(CLASFV_EINVAL, "no workspace exists for this stream yet");
  DEVICE_GUARD(h->device);
  HIP_TRY(hipMemsetAsync(cx->arena, byte, cx->arena_bytes, s));
  return CLASFV_OK;
}

int clasfv_workspace_view(clasfv_t h, void* stream, void** base, int64_t* bytes) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  const clasfv_engine::Ctx* cx = find_ctx(h, (hipStream_t)stream);
  if (!cx || !cx->arena) return fail(CLASFV_EINVAL, "no workspace exists for this stream yet");
  if (base) *base = cx->arena;
  if (bytes) *bytes = (int64_t)cx->arena_bytes;
  return CLASFV_OK;
}

// ---- diagnostics: one conv / the decoder alone, through the forward's own dispatch ---------------

int clasfv_conv_count(clasfv_t h) { return h ? (int)h->convs.size() + 4 : CLASFV_EINVAL; }

int clasfv_conv_info(clasfv_t h, int i, const char** prefix, const char** bn_prefix, int* tap, int channels[5],
                     int kernel[3], int stride[3], int padding[3], int* in_dtype, int* out_dtype) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  int tp = -1;
  const Conv* pc = probe_conv(h, i, &tp);
  if (!pc) return fail(CLASFV_EINVAL, "bad conv index");
  Conv c = *pc;  // padded widths and dtypes of the handle's current compute dtype
  layout_conv(c, h->dtype == CLASFV_DTYPE_BF16);
  if (prefix) *prefix = pc->w.c_str();
  if (bn_prefix) *bn_prefix = pc->bn.c_str();
  if (tap) *tap = tp;
  if (channels) channels[0] = c.cin, channels[1] = c.cout, channels[2] = c.cin_p, channels[3] = c.cout_p, channels[4] = c.cin2;
  if (kernel) kernel[0] = c.kt, kernel[1] = c.kh, kernel[2] = c.kw;
  if (stride) stride[0] = c.st, stride[1] = c.sh, stride[2] = c.sw;
  if (padding) padding[0] = c.pt, padding[1] = c.ph, padding[2] = c.pw;
  if (in_dtype) *in_dtype = c.in_bf16 ? CLASFV_DTYPE_BF16 : CLASFV_DTYPE_FP32;
  if (out_dtype) *out_dtype = c.out_bf16 ? CLASFV_DTYPE_BF16 : CLASFV_DTYPE_FP32;
  return CLASFV_OK;
}

int clasfv_run_conv(clasfv_t h, int i, const void* x, int N, int T, int H, int W, const void* x2, const void* res,
                    int relu, int x_c8, int y_c8, void* y, void* scratch, int64_t scratch_bytes,
                    const char** kernel_name, void* stream) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  if (!h->ready) return fail(CLASFV_ENOTREADY, "clasfv_finalize has not been called");
  const Conv* c = probe_conv(h, i, nullptr);
  if (!c) return fail(CLASFV_EINVAL, "bad conv index");
  if (!x || !y) return fail(CLASFV_EINVAL, "null tensor");
  if (N < 1 || T < 1 || H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad shape");
  if ((c->cin2 != 0) != (x2 != nullptr)) return fail(CLASFV_EINVAL, "second input: needed by the dual projection only");
  if (scratch_bytes < 0 || (scratch_bytes > 0 && !scratch)) return fail(CLASFV_EINVAL, "bad scratch");
  if (T + 2 * c->pt < c->kt || H + 2 * c->ph < c->kh || W + 2 * c->pw < c->kw)
    return fail(CLASFV_EINVAL, "input smaller than the kernel");
  DEVICE_GUARD(h->device);
  const Shape5 in{N, T, H, W, c->cin_p};
  const ConvCall cc{c, in, x, x2, res, y, relu != 0, x_c8, y_c8, scratch_bytes ? scratch : nullptr, (size_t)scratch_bytes};
  ConvBuilt b;
  const int rc = run_conv(h, cc, (hipStream_t)stream, b);
  if (kernel_name) *kernel_name = b.kernel ? b.kernel->name : "";
  return rc;
}

int clasfv_run_decoder(clasfv_t h, const float* p01, const float* p2, const float* p3, const float* p4, int N, int T,
                       int H, int W, float* seg, float* mot, void* stream) {
  if (!h) return fail(CLASFV_EINVAL, "null handle");
  if (!h->ready) return fail(CLASFV_ENOTREADY, "clasfv_finalize has not been called");
  if (!p01 || !p2 || !p3 || !p4 || !seg || !mot) return fail(CLASFV_EINVAL, "null tensor");
  if (N < 1 || T < 1 || H < 2 || W < 2) return fail(CLASFV_EINVAL, "bad shape");
  if (H % 8 || W % 16) return fail(CLASFV_EBADSHAPE, "decoder tiles: H % 8 == 0 and W % 16 == 0");
  hipStream_t s = (hipStream_t)stream;
  // tap resolutions as the backbone produces them: the stem halves H and W, layer2..4 halve T, H, W
  // (3-wide kernels, stride 2, padding 1: d -> (d - 1) / 2 + 1)
  auto half = [](int d) { return (d - 1) / 2 + 1; };
  const float* taps[4] = {p01, p2, p3, p4};
  Shape5 tsh[4];
  int t = T, hh = half(H), ww = half(W);
  for (int k = 0; k < 4; ++k) {
    if (k) t = half(t), hh = half(hh), ww = half(ww);
    tsh[k] = Shape5{N, t, hh, ww, 64};
  }
  if (!decoder_addressable(decoder_params(h, taps, tsh, seg, mot, N, T, H, W, nullptr)))
    return fail(CLASFV_EBADSHAPE, "decoder_kernel: every tap must have fewer than 2^31 floats, and the grid fewer than "
                                  "2^31 blocks");
  DEVICE_GUARD(h->device);
  // the index table lives where the forward keeps it: in this stream's arena, sized and laid out for a
  // whole forward of this shape (a later clasfv_forward of the shape reuses the arena as it stands)
  Layout L;
  make_layout(N, T, H, W, L);
  clasfv_engine::Ctx* cx = nullptr;
  if (int rc = acquire_ctx(h, s, L.total, &cx)) return rc;
  log_begin(h);
  HIP_TRY(launch_decoder(decoder_params(h, taps, tsh, seg, mot, N, T, H, W, cx->arena + L.off[DIDX]), s));
  log_end(h, -1);
  return CLASFV_OK;
}

int clasfv_build_clips(const float* video, int T, int H, int W, const int32_t* table, int n, int interp, float* clips,
                       void* stream) {
  if (!video || !table || !clips || n < 0 || T < 1 || H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad argument");
  if (n == 0) return CLASFV_OK;
  HIP_TRY(launch_build_clips(video, T, H * W, table, n, interp, clips, (hipStream_t)stream));
  return CLASFV_OK;
}

// Shared argument check of clasfv_pass_labels[_margin]. Beyond the pointers: every pass must have the
// clips its frames are read from (what fuse_utils.clip_table raises for), and T is a grid dimension.
static int check_pass_labels(const void* in, int K, const int32_t* clip0, int T, int step, int H, int W, int interp,
                             const void* labels) {
  if (!in || !clip0 || !labels || K < 1 || K > CLASFV_MAX_PASSES || T < 1 || step < 1)
    return fail(CLASFV_EINVAL, "bad argument (K must be in [1, 64])");
  if (H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad argument (H and W must be >= 1)");
  if (T > 65535) return fail(CLASFV_EINVAL, "bad argument (T must be <= 65535)");
  if ((int64_t)(K - 1) * step >= T) return fail(CLASFV_EINVAL, "bad argument ((K - 1) * step must be < T)");
  for (int k = 0; k < K; ++k) {
    const int tk = T - k * step;
    const int q = tk >> 5, r = tk & 31;
    const int nk = r > 16 ? q + 1 : r < 16 ? q : q + (q & 1);  // round half to even, as build_clips
    if (nk == 0) return fail(CLASFV_EINVAL, "a pass has too few frames for one 32-frame clip");
    if (clip0[k] < 0) return fail(CLASFV_EINVAL, "negative pass_clip0 entry");
    // Without resampling frame f of the pass is frame f of its clips: 32 * nk > tk would need a clip that
    // cannot be built (clip_table's ValueError), 32 * nk < tk leaves frames [32 * nk, tk) without logits.
    if (!interp && r != 0) return fail(CLASFV_EINVAL, "interpolate == 0 needs every pass length to be a multiple of 32");
  }
  return CLASFV_OK;
}

int clasfv_pass_labels(const float* logits, int K, const int32_t* clip0, int T, int step, int H, int W, int interp,
                       uint8_t* labels, void* stream) {
  if (int rc = check_pass_labels(logits, K, clip0, T, step, H, W, interp, labels)) return rc;
  HIP_TRY(launch_pass_labels(logits, K, clip0, T, step, H * W, interp, 0, labels, (hipStream_t)stream));
  return CLASFV_OK;
}

int clasfv_pass_labels_margin(const float* margin, int K, const int32_t* clip0, int T, int step, int H, int W,
                              int interp, uint8_t* labels, void* stream) {
  if (int rc = check_pass_labels(margin, K, clip0, T, step, H, W, interp, labels)) return rc;
  HIP_TRY(launch_pass_labels(margin, K, clip0, T, step, H * W, interp, 1, labels, (hipStream_t)stream));
  return CLASFV_OK;
}

int clasfv_logit_margin(const float* logits, int n, int H, int W, float* margin, void* stream) {
  if (!logits || !margin || n < 0 || H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad argument");
  if (n == 0) return CLASFV_OK;
  HIP_TRY(launch_logit_margin(logits, n, H * W, margin, (hipStream_t)stream));
  return CLASFV_OK;
}

int clasfv_fuse_votes(const uint8_t* labels, int K, int T, int step, int H, int W, int method, uint8_t* fused,
                      void* stream) {
  if (!labels || !fused || K < 1 || K > CLASFV_MAX_PASSES || T < 1 || step < 1 || T - (step - 1) < 1)
    return fail(CLASFV_EINVAL, "bad argument (K must be in [1, 64])");
  // CLASFV_FUSE_CLEAN and its hole threshold (bits 16..30) ride on the method; bit 31 belongs to nobody
  const unsigned bits = (unsigned)method;
  const bool clean = (bits & CLASFV_FUSE_CLEAN) != 0;
  const int holes = (int)((bits >> 16) & 0x7FFFu);
  if ((bits >> 31) || (holes && !clean))
    return fail(CLASFV_EINVAL, "unknown method (hole threshold without CLASFV_FUSE_CLEAN, or bit 31)");
  const int fuse = (int)(bits & 0xFFFFu & ~(unsigned)CLASFV_FUSE_CLEAN);  // what launch_fuse_votes takes
  const int m = fuse & ~CLASFV_FUSE_FORCE_GENERIC;
  if (m != CLASFV_FUSE_MAJORITY && m != CLASFV_FUSE_SIMPLE && m != CLASFV_FUSE_STAPLE && m != CLASFV_FUSE_ITKVOTING)
    return fail(CLASFV_EINVAL, "unknown method");
  if (H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad argument (H and W must be >= 1)");
  if ((m == CLASFV_FUSE_MAJORITY || m == CLASFV_FUSE_ITKVOTING) && T - (step - 1) > 65535)
    return fail(CLASFV_EINVAL, "bad argument (majority / ITK voting take at most 65535 output frames)");
  if (m == CLASFV_FUSE_SIMPLE && (int64_t)H * W > CLASFV_SIMPLE_MAX_HW)
    return fail(CLASFV_EBADSHAPE, "SIMPLE keeps one frame's estimate in LDS: H * W must be <= 162816");
  if (clean && (int64_t)H * W > CLASFV_CLEAN_MAX_PIXELS)
    return fail(CLASFV_EBADSHAPE, "CLASFV_FUSE_CLEAN keeps one frame's labels in LDS: H * W must be <= 53248");
  HIP_TRY(launch_fuse_votes(labels, K, T, step, H * W, fuse, fused, (hipStream_t)stream));
  if (clean)
    HIP_TRY(launch_cleanup_frames(fused, (int64_t)(T - (step - 1)), H, W, holes ? holes : CLASFV_CLEAN_DEFAULT_HOLES,
                                  (hipStream_t)stream));
  return CLASFV_OK;
}

// Byte ranges of the warp entry points' tensors, for their overlap refusals. An empty range overlaps nothing.
struct ByteSpan { uintptr_t lo, hi; };
static ByteSpan dense_span(const void* p, uint64_t floats) {
  return {(uintptr_t)p, (uintptr_t)p + floats * sizeof(float)};
}
// motion (N,2,H,W) with element strides m_sn, m_sc (either sign) and dense H * W planes
static ByteSpan motion_span(const float* motion, int N, int H, int W, int64_t m_sn, int64_t m_sc) {
  const int64_t dn = (int64_t)(N - 1) * m_sn;
  const int64_t lo = (dn < 0 ? dn : 0) + (m_sc < 0 ? m_sc : 0), hi = (dn > 0 ? dn : 0) + (m_sc > 0 ? m_sc : 0);
  return {(uintptr_t)(motion + lo), (uintptr_t)(motion + hi + (int64_t)H * W)};
}
static bool spans_overlap(const ByteSpan& a, const ByteSpan& b) {
  return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi;
}

int clasfv_warp(const float* img, int N, int C, int H, int W, const float* motion, int64_t m_sn, int64_t m_sc,
                float* out, void* stream) {
  if (!img || !motion || !out || N < 1 || C < 1 || H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad argument");
  // every block reads img and motion while others write out
  const ByteSpan o = dense_span(out, (uint64_t)N * C * H * W);
  if (spans_overlap(o, dense_span(img, (uint64_t)N * C * H * W))) return fail(CLASFV_EINVAL, "out overlaps img");
  if (spans_overlap(o, motion_span(motion, N, H, W, m_sn, m_sc))) return fail(CLASFV_EINVAL, "out overlaps motion");
  HIP_TRY(launch_warp(img, N, C, H, W, motion, m_sn, m_sc, out, (hipStream_t)stream));
  return CLASFV_OK;
}

int clasfv_warp_backward(const float* grad_out, const float* img, int N, int C, int H, int W, const float* motion,
                         int64_t m_sn, int64_t m_sc, float* grad_img, float* grad_motion, void* stream) {
  if (!grad_out || !img || !motion || (!grad_img && !grad_motion) || N < 1 || C < 1 || H < 1 || W < 1)
    return fail(CLASFV_EINVAL, "bad argument");
  const ByteSpan in[3] = {dense_span(grad_out, (uint64_t)N * C * H * W), dense_span(img, (uint64_t)N * C * H * W),
                          motion_span(motion, N, H, W, m_sn, m_sc)};
  const ByteSpan gi = dense_span(grad_img, grad_img ? (uint64_t)N * C * H * W : 0);
  const ByteSpan gm = dense_span(grad_motion, grad_motion ? (uint64_t)N * 2 * H * W : 0);
  for (const ByteSpan& r : in) {
    if (spans_overlap(gi, r)) return fail(CLASFV_EINVAL, "grad_img overlaps an input");
    if (spans_overlap(gm, r)) return fail(CLASFV_EINVAL, "grad_motion overlaps an input");
  }
  if (spans_overlap(gi, gm)) return fail(CLASFV_EINVAL, "grad_img overlaps grad_motion");
  HIP_TRY(launch_warp_backward(grad_out, img, N, C, H, W, motion, m_sn, m_sc, grad_img, grad_motion,
                               (hipStream_t)stream));
  return CLASFV_OK;
}

int clasfv_track(const float* img, int N, int C, int H, int W, const float* motion, int64_t m_sn, int64_t m_sc,
                 int64_t m_st, int T, int t0, int t_step, int P, int mode, float* out, void* stream) {
  if (!img || !motion || !out) return fail(CLASFV_EINVAL, "bad argument (null pointer)");
  if (N < 1 || C < 1 || H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad argument (N, C, H and W must be >= 1)");
  if (P < 1) return fail(CLASFV_EINVAL, "bad argument (P must be >= 1)");
  if (t_step != 1 && t_step != -1) return fail(CLASFV_EINVAL, "bad argument (t_step must be +1 or -1)");
  const int64_t t_last = t0 + (int64_t)(P - 1) * t_step;
  if (T < 1 || t0 < 0 || t0 >= T || t_last < 0 || t_last >= T)
    return fail(CLASFV_EINVAL, "bad argument (every frame t0 + p * t_step, p < P, must lie in [0, T))");
  const int both = CLASFV_TRACK_FORCE_STEPS | CLASFV_TRACK_FORCE_LDS, m = mode & ~both;
  if ((m != CLASFV_TRACK_BILINEAR && m != CLASFV_TRACK_NEAREST) || (mode & both) == both)
    return fail(CLASFV_EINVAL, "unknown mode");
  if ((int64_t)H * W > INT32_MAX || (int64_t)N * C > INT32_MAX)
    return fail(CLASFV_EBADSHAPE, "H * W and N * C must be < 2^31");
  // step 0 reads img while out[0] is written (out[p - 1] while out[p], which never overlap)
  const uintptr_t i0 = (uintptr_t)img, o0 = (uintptr_t)out;
  const uint64_t frame = (uint64_t)N * C * H * W * sizeof(float);
  if (i0 < o0 + frame * (uint64_t)P && o0 < i0 + frame) return fail(CLASFV_EINVAL, "out overlaps img");
  HIP_TRY(launch_track(img, N, C, H, W, motion, m_sn, m_sc, m_st, t0, t_step, P, mode, out, (hipStream_t)stream));
  return CLASFV_OK;
}

int clasfv_lv_geometry(const uint8_t* masks, int64_t F, int H, int W, int label, double sy, double sx, int32_t* area,
                       double* geom, void* stream) {
  if (!masks || !area || !geom) return fail(CLASFV_EINVAL, "bad argument (null pointer)");
  if (F < 1 || H < 1 || W < 1) return fail(CLASFV_EINVAL, "bad argument (F, H and W must be >= 1)");
  if (label < 0 || label > 255) return fail(CLASFV_EINVAL, "bad argument (label must be in [0, 255])");
  if (!(isfinite(sy) && isfinite(sx) && sy > 0.0 && sx > 0.0))
    return fail(CLASFV_EINVAL, "bad argument (the spacings must be finite and positive)");
  if ((int64_t)H * W > CLASFV_LV_MAX_PIXELS)
    return fail(CLASFV_EBADSHAPE, "the frame is kept in LDS: H * W must be <= 162816");
  HIP_TRY(launch_lv_geometry(masks, F, H, W, label, sy, sx, area, geom, (hipStream_t)stream));
  return CLASFV_OK;
}

int64_t clasfv_render_workspace_bytes(void) { return CLASFV_RENDER_WORKSPACE_BYTES; }

int clasfv_render_annotated(const float* video, const uint8_t* masks, const uint8_t* truth, int T, int H, int W,
                            const double* volume, int64_t volume_stride, const uint8_t* title, int first, int count,
                            int Hp, int Wo, int Ht, int Hs, int label, double thickness, void* workspace,
                            uint8_t* out, void* stream) {
  if (!video || !masks || !volume || !workspace || !out) return fail(CLASFV_EINVAL, "bad argument (null pointer)");
  if (T < 1 || H < 1 || W < 1 || Hp < 1 || Wo < 1 || Ht < 0 || Hs < 0)
    return fail(CLASFV_EINVAL, "bad argument (T, H, W, Hp and Wo must be >= 1, Ht and Hs >= 0)");
  if (count < 1) return fail(CLASFV_EINVAL, "bad argument (count must be >= 1)");
  if (first < 0 || first >= T || count > T - first)
    return fail(CLASFV_EINVAL, "bad argument (the frames [first, first + count) must lie in [0, T))");
  if (label < 0 || label > 255) return fail(CLASFV_EINVAL, "bad argument (label must be in [0, 255])");
  if (!(isfinite(thickness) && thickness >= 0.0))
    return fail(CLASFV_EINVAL, "bad argument (the thickness must be finite and not negative)");
  if (volume_stride < 1) return fail(CLASFV_EINVAL, "bad argument (volume_stride must be >= 1)");
  if (((uintptr_t)volume | (uintptr_t)workspace) & 7)
    return fail(CLASFV_EINVAL, "bad argument (volume_dev and workspace_dev must be 8-byte aligned)");
  const uint64_t frame = (uint64_t)(Hp + (int64_t)Ht + Hs) * (uint64_t)Wo * 3, total = frame * (uint64_t)count;
  if ((uint64_t)H * W >> 31 || frame >> 32 || total >> 32)
    return fail(CLASFV_EBADSHAPE, "the output of one call must be below 2^32 bytes and H * W below 2^31");
  const uint64_t thw = (uint64_t)T * H * W;
  if (thw > (1ull << 60) / 12 || (uint64_t)volume_stride > (1ull << 60) / ((uint64_t)T * 8))
    return fail(CLASFV_EBADSHAPE, "the inputs are past what 64-bit offsets address");
  const uintptr_t o0 = (uintptr_t)out;
  auto overlaps = [&](const void* p, uint64_t bytes) {
    const uintptr_t i0 = (uintptr_t)p;
    return p && bytes && i0 < o0 + total && o0 < i0 + bytes;
  };
  if (overlaps(video, thw * 12) || overlaps(masks, thw) || overlaps(truth, thw) ||
      overlaps(volume, ((uint64_t)(T - 1) * (uint64_t)volume_stride + 1) * 8) ||
      overlaps(title, (uint64_t)Ht * Wo * 3) || overlaps(workspace, CLASFV_RENDER_WORKSPACE_BYTES))
    return fail(CLASFV_EINVAL, "out overlaps an input or the workspace");
  RenderParams p;
  p.video = video, p.masks = masks, p.truth = truth, p.volume = volume, p.title = title;
  p.workspace = (double*)workspace, p.out = out, p.vstride = volume_stride;
  p.T = T, p.H = H, p.W = W, p.first = first, p.count = count, p.Hp = Hp, p.Wo = Wo, p.Ht = Ht, p.Hs = Hs;
  p.label = label, p.thickness = thickness;
  HIP_TRY(launch_render_annotated(p, (hipStream_t)stream));
  return CLASFV_OK;
}

int clasfv_preprocess_video(const uint8_t* frames, int T, int Hs, int Ws, int H, int W, float* out, void* stream) {
  if (!frames || !out || T < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || H > 65535 || T > 65535)
    return fail(CLASFV_EINVAL, "bad argument");
  HIP_TRY(launch_preprocess_video(frames, T, Hs, Ws, H, W, out, (hipStream_t)stream));
  return CLASFV_OK;
}

int64_t clasfv_zeroone_workspace_bytes(void) { return (int64_t)sizeof(float) * zeroone_partials_floats(); }

int clasfv_zeroone_normalize(float* video, int64_t n, float* workspace, void* stream) {
  if (!video || !workspace || n < 1) return fail(CLASFV_EINVAL, "bad argument");
  HIP_TRY(launch_zeroone_normalize(video, n, workspace, (hipStream_t)stream));
  return CLASFV_OK;
}

}  // extern "C"
