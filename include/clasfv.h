/*
 * clasfv.h -- C ABI of the MI355X-native CLAS-FV engine (libclasfv.so, gfx950).
 *
 * Drop-in boundary for the reference hot path (yc015/fully-automated-multi-heartbeat-echocardiography-
 * video-segmentation-and-motion-tracking @ /root/reference):
 *   model forward      R2plus1D_18_MotionNet.forward(x) -> (seg, motion)
 *                        src/model/R2plus1D_18_MotionNet.py:26-71
 *   checkpoint load    model.load_state_dict(torch.load(path)["model"])    motion_segment.py:69-72
 *   clip plumbing      divide_to_consecutive_clips / segment_a_video_with_fusion
 *                        src/fuse_utils.py:16-100
 *   motion warp        generate_2dmotion_field + F.grid_sample(border, align_corners=False)
 *                        src/transform_utils.py:14-34, src/visualization_utils.py:128
 *   normaliser         zeroone_normalizer                                  src/echonet_dataset.py:38-50
 *
 * Conventions
 *   - Plain C types only. Tensors are dense row-major fp32 (labels: uint8) in the reference's
 *     layouts (N,C,T,H,W). Pointers marked _dev are device (HBM) pointers owned by the caller;
 *     the library owns weights and its workspace.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). All launches are
 *     stream-ordered and asynchronous; no call synchronises the device except clasfv_finalize.
 *   - Every function returns CLASFV_OK (0) or a negative error code; clasfv_last_error() returns
 *     a thread-local message for the last failure. A handle is not re-entrant: calls on one handle
 *     must be serialised by the caller (one handle per device per process).
 */
#ifndef CLASFV_H
#define CLASFV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  CLASFV_OK = 0,
  CLASFV_EINVAL = -1,     /* bad argument / unknown parameter name */
  CLASFV_EBADSHAPE = -2,  /* shape not supported: T % 8, H % 16, W % 16 must be 0 (forward); frame too large (SIMPLE);
                             a tensor past what the kernel addresses (see "Size limits" below) */
  CLASFV_ENOTREADY = -3,  /* forward before clasfv_finalize / missing parameters */
  CLASFV_EHIP = -4,       /* HIP runtime error (message in clasfv_last_error) */
  CLASFV_ENOMEM = -5
};

/* ABI revision: bumped whenever an exported function changes its parameter list. Callers check
 * clasfv_version() == CLASFV_ABI_VERSION after loading the library (the ctypes binding does).
 *   1  round 1
 *   2  clasfv_zeroone_normalize takes a caller-owned workspace; clasfv_kernel_timing reports xgflop
 *   3  kernel variants (clasfv_set_kernel_variants), CLASFV_FUSE_FORCE_GENERIC */
#define CLASFV_ABI_VERSION 3

/* MAJORITY: ties -> 0; ITKVOTING: itk::LabelVotingImageFilter with its default undecided label
 * (max label + 1): ties -> 2. */
enum { CLASFV_FUSE_MAJORITY = 0, CLASFV_FUSE_SIMPLE = 1, CLASFV_FUSE_STAPLE = 2, CLASFV_FUSE_ITKVOTING = 3 };
/* OR-ed into a clasfv_fuse_votes method: run SIMPLE on its generic kernel instead of the packed
 * 16-vote one (A/B testing; results are identical). */
#define CLASFV_FUSE_FORCE_GENERIC 0x100
/* OR-ed into a clasfv_fuse_votes method: clean every fused frame in place after the fusion (the rule is
 * stated at clasfv_fuse_votes). CLASFV_FUSE_CLEAN_HOLES(n), n in 1..32767, sets the hole threshold in bits
 * 16..30; without it (n = 0) the threshold is the reference's default, CLASFV_CLEAN_DEFAULT_HOLES. */
#define CLASFV_FUSE_CLEAN 0x200
#define CLASFV_FUSE_CLEAN_HOLES(n) ((n) << 16)
#define CLASFV_CLEAN_DEFAULT_HOLES 128
/* Largest frame CLASFV_FUSE_CLEAN takes, in pixels. The cleanup kernel keeps one frame in the 160 KiB of a
 * CU's LDS as a 16-bit label and a flag byte per pixel, 3 B, beside 256 B of state: 52 * 1024 pixels, the
 * packed SIMPLE kernel's limit (224 x 224 = 50176 fits). A label is a pixel index, so 32-bit labels would halve
 * the limit and lose 224 x 224. */
#define CLASFV_CLEAN_MAX_PIXELS 53248
enum { CLASFV_DTYPE_FP32 = 0, CLASFV_DTYPE_BF16 = 1 };
/* One more kernel-variant bit (CLASFV_NO_DMA_X3_WIDE in the environment; see the enum below):
 * conv_dma_x3's 128-voxel x 80- / 96-channel blocks on the fp32 engines' 240- and 480-channel convs,
 * instead of its wide form's 256-voxel x 240-channel blocks. The two are bit-identical; the bit serves
 * A/B timing and the tests that hold one against the other. */
#define CLASFV_VARIANT_NO_DMA_X3_WIDE 268435456

/* Kernel-variant switches (A/B testing against the kernels each product kernel replaced; every
 * variant computes the same function -- NO_SPLIT_K the same sums in another fp32 summation order,
 * NO_WINO4 the same convolutions through F(2x2,3x3) instead of F(4x4,3x3) fp32 rounding).
 * Read once, at clasfv_create, from the environment variable named in the comment (set = on), or set
 * with clasfv_set_kernel_variants. Bits 131072, 1048576, 2097152, 8388608 and 33554432 are retired
 * (round-5 A/B forms that measured slower; they live only in tools/convbench now) and rejected. */
enum {
  CLASFV_VARIANT_NO_WINOGRAD = 1,      /* CLASFV_WINOGRAD=0: fp32 stride-1 convs on the direct implicit GEMM */
  CLASFV_VARIANT_NO_WINO_PATCH = 2,    /* CLASFV_NO_WINO_PATCH: conv_wino instead of conv_wino_q */
  CLASFV_VARIANT_WINOT_REFERENCE = 4,  /* CLASFV_WINOT_REFERENCE: conv_winot instead of conv_winot5 */
  CLASFV_VARIANT_NO_C8 = 8,            /* CLASFV_NO_C8: channels-last mid tensors everywhere */
  CLASFV_VARIANT_NO_STEM_BF16 = 16,    /* CLASFV_NO_STEM_BF16: bf16 engines run the fp32 stem */
  CLASFV_VARIANT_NO_PATCH_BF16 = 32,   /* CLASFV_NO_PATCH_BF16: bf16 stride-1 convs on conv_dma */
  CLASFV_VARIANT_NO_DECODER_BF16 = 64, /* CLASFV_NO_DECODER_BF16: bf16 engines run the fp32 decoder */
  CLASFV_VARIANT_WINOT_NO_TS1 = 128,   /* CLASFV_WINOT_TS1=0: T % 8 != 0 temporal convs on conv_winot */
  CLASFV_VARIANT_NO_SPLIT_K = 256,     /* CLASFV_NO_SPLIT_K: conv_winot5 grids smaller than the chip unsplit */
  CLASFV_VARIANT_NO_WINO4 = 512,       /* CLASFV_NO_WINO4: conv_wino_q (F(2x2,3x3)) instead of conv_wino4 (F(4x4,3x3)) */
  CLASFV_VARIANT_NO_DECODER_X3 = 1024, /* CLASFV_NO_DECODER_X3: fp32 engines run comb_2 on fp32 MFMAs, not split bf16 */
  CLASFV_VARIANT_NO_DMA_X3 = 2048,     /* CLASFV_NO_DMA_X3: fp32 strided / 1x1x1 convs on conv_dma (fp32 MFMA), not conv_dma_x3 */
  CLASFV_VARIANT_NO_STEM_X3 = 4096,    /* CLASFV_NO_STEM_X3: fp32 engines' stem on conv_stem_f32 (fp32 MFMA), not conv_stem_x3 */
  CLASFV_VARIANT_NO_WINO4W = 8192,     /* CLASFV_NO_WINO4W: conv_wino4 (48-channel blocks) instead of conv_wino4w (wide blocks) */
  CLASFV_VARIANT_NO_PATCH32 = 16384,   /* CLASFV_NO_PATCH32: bf16 1x3x3 convs on conv_patch_bf16 (16x16x32 tiles) instead of conv_patch32_bf16 (32x32x16) */
  CLASFV_VARIANT_NO_PROJ_X3 = 32768,   /* CLASFV_NO_PROJ_X3: the decoder's 128-deep tap projections on conv_dma_x3 instead of the persistent conv_proj_x3 */
  CLASFV_VARIANT_NO_WINO4R = 65536,    /* CLASFV_NO_WINO4R: wide-block 1x3x3 convs on conv_wino4w (4 quadrant waves, one per SIMD) instead of conv_wino4r (12 row waves, three per SIMD) */
  CLASFV_VARIANT_NO_DMA_BUF = 262144,  /* CLASFV_NO_DMA_BUF: conv_dma_x3's LDS-DMAs from 64-bit pointers instead of 32-bit buffer offsets */
  CLASFV_VARIANT_W4R_CACHED_STORES = 524288, /* CLASFV_W4R_CACHED_STORES: conv_wino4r's output stores cached instead of non-temporal */
  CLASFV_VARIANT_PATCH32_CACHED_STORES = 4194304, /* CLASFV_PATCH32_CACHED_STORES: conv_patch32_bf16's output stores cached (the product's are non-temporal) */
  CLASFV_VARIANT_NO_DMA_W = 16777216,       /* CLASFV_NO_DMA_W: the bf16 engines' direct convs on conv_dma (64-B LDS rows) instead of conv_dma_w (128-B rows) */
  CLASFV_VARIANT_NO_TWALK = 67108864        /* CLASFV_NO_TWALK: the bf16 engines' 64-channel temporal convs (layer1, stem) on conv_patch_bf16 instead of the frame-walking conv_twalk_bf16 (round 6) */
};

typedef struct clasfv_engine* clasfv_t;

const char* clasfv_last_error(void);
/* CLASFV_ABI_VERSION of the loaded library. */
int clasfv_version(void);
/* Content hash of the sources the library was compiled from ("clasfv-source-hash:<16 hex>",
 * computed by the build over csrc/ and this header): a binding can refuse a library older than its
 * sources without trusting file times. Does not change the ABI revision (a new export only). */
const char* clasfv_source_hash(void);

/* ---- model: replaces R2plus1D_18_MotionNet.__init__/load_state_dict/forward ------------------ */
int clasfv_create(int device, clasfv_t* out);
int clasfv_destroy(clasfv_t h);
/* Number / name / shape of the 242 state-dict entries the engine accepts (reference key names,
 * e.g. "r2plus1d_model.stem.0.weight"); shape is written to dims[0..*ndim). */
int clasfv_param_count(clasfv_t h);
int clasfv_param_info(clasfv_t h, int i, const char** name, int* ndim, int64_t dims[5]);
/* Copy one state-dict entry from host memory. A "module." prefix (nn.DataParallel checkpoints,
 * motion_segment.py:69) is accepted. num_batches_tracked entries are accepted and ignored. */
int clasfv_load_param(clasfv_t h, const char* name, const float* host_data, int64_t numel);
/* Fold eval-mode BatchNorm into the convolutions, pad channels for the kernels, upload to HBM. */
int clasfv_finalize(clasfv_t h);
/* seg_dev (N,2,T,H,W) logits and motion_dev (N,4,T,H,W) tanh outputs from x_dev (N,3,T,H,W).
   Stream-ordered on `stream` (a hipStream_t; NULL = the default stream), no host synchronisation.
   The handle keeps one workspace per launch stream (up to 4; a fifth stream takes over the least
   recently used one after a device synchronisation), so forwards issued on different streams may run
   concurrently; calls on one handle must come from one host thread at a time.
   Size limits: every kernel addresses its tensors in 32 bits somewhere ("Size limits"), and
   nothing is launched outside those limits. N is not limited by them: a batch of more clips than
   clasfv_max_clips reports for the shape runs as consecutive sub-batches of that many clips (the
   workspace is sized for one sub-batch), and a clip's outputs are bit-identical whatever N is.
   CLASFV_EBADSHAPE, before the first launch, when a single clip of the shape is past a limit
   (clasfv_max_clips == 0: for instance T * H * W >= 2^31). */
int clasfv_forward(clasfv_t h, const float* x_dev, int N, int T, int H, int W, float* seg_dev,
                   float* motion_dev, void* stream);
/* Bytes of library workspace currently held (the per-stream activation arenas; each grows to the
   largest N*T*H*W seen on its stream). */
int64_t clasfv_workspace_bytes(clasfv_t h);
/* The largest number of (T, H, W) clips one pass of the network takes, for an engine of compute dtype
 * `dtype` (CLASFV_DTYPE_*) and kernel variants `variants` (CLASFV_VARIANT_* bits): the largest N for which
 * every launch of clasfv_forward stays inside its kernel's addressing limits on the kernel a single clip
 * of the shape runs on. 0 when one clip is already past a limit; CLASFV_EBADSHAPE / CLASFV_EINVAL for
 * a shape clasfv_forward does not take / an unknown dtype or variant bit. Host arithmetic only: needs
 * neither a handle nor a device. New export only: the ABI revision is unchanged. */
int clasfv_max_clips(int T, int H, int W, int dtype, int variants);
/* The test clasfv_max_clips searches with: CLASFV_OK when every launch of one pass over N clips is inside
 * its kernel's limits, CLASFV_EBADSHAPE (the first launch that is not, in clasfv_last_error) otherwise. */
int clasfv_clips_fit(int N, int T, int H, int W, int dtype, int variants);
/* Compute dtype of the encoder: CLASFV_DTYPE_FP32 (default; exact-fp32 MFMA, the reference's
 * precision) or CLASFV_DTYPE_BF16 (bf16 activations/weights, fp32 accumulation; BASELINE config[4],
 * Dice tolerance 1e-2). The decoder head runs in fp32 either way. A change takes effect at the next
 * clasfv_finalize. */
int clasfv_set_compute_dtype(clasfv_t h, int dtype);
int clasfv_get_compute_dtype(clasfv_t h);
/* Kernel-variant switches (CLASFV_VARIANT_* bits). A change of CLASFV_VARIANT_NO_WINOGRAD needs the
 * next clasfv_finalize (the Winograd weight images are built there); the others apply to the next
 * clasfv_forward. */
int clasfv_set_kernel_variants(clasfv_t h, int flags);
int clasfv_get_kernel_variants(clasfv_t h);

/* ---- instrumentation (bench.py's live roofline; not on the reference's interface) ------------ */
/* enable != 0: every later clasfv_forward records one HIP event on its stream before its first
 * launch and one after each launch, so each kernel's device time is the gap between two events.
 * Enabling or disabling drops what was recorded. */
int clasfv_set_kernel_timing(clasfv_t h, int enable);
/* Waits for the recorded events, aggregates the launches recorded since the last call per kernel
 * and clears them. Entry i: names[i] (static string, e.g. "conv_wino"), launches[i], ms[i] (summed
 * device time), gflop[i] (summed algorithmic GFLOP, 2 per MAC over unpadded channels: the direct
 * convolution the launch replaces), xgflop[i] (summed GFLOP the launch issues to the matrix cores:
 * Winograd-domain products, padded channels and partial tiles included -- the roofline numerator).
 * Returns the number of entries (<= cap) or a negative error code. */
int clasfv_kernel_timing(clasfv_t h, int cap, const char** names, int* launches, double* ms,
                         double* gflop, double* xgflop);

/* ---- diagnostics: the launch log (new exports only: the ABI revision is unchanged) ------------ */
/* enable != 0: every later clasfv_forward, clasfv_run_conv and clasfv_run_decoder on this handle records
 * each kernel it launches. Enabling or disabling drops what was recorded. Off (the default), a launch
 * costs a few host stores more than without the log. */
int clasfv_set_launch_log(clasfv_t h, int enable);
/* The launches recorded since the last call, in launch order, and clears them. Entry i: labels[i], the
 * instantiation launched as the compiler spells it (e.g. "conv_winot5<4, 4, 2>"; a string owned by the
 * handle, valid until clasfv_destroy; derived from the kernel's address at the launch site, never typed
 * by hand: treat it as an opaque key whose part before '<' is the kernel's name); grids[i], its blocks;
 * passes[i], the largest number of work items one wave or block of the launch processes in turn (1
 * unless the launcher caps its grid: conv_stem_x3, conv_stem_bf16, conv_proj_x3, pack_input_kernel);
 * convs[i], the conv it belongs to (clasfv_conv_info's numbering; a split-K launch and its
 * split_sum_kernel share one) or -1 for pack_input_kernel and the decoder's kernels. Returns the number
 * of entries; CLASFV_EINVAL, with the log kept, when more than cap are waiting. At most 65536 launches
 * are kept between two calls. */
int clasfv_launch_log(clasfv_t h, int cap, const char** labels, int64_t* grids, int* passes, int* convs);
/* Fill the whole workspace arena of the context that belongs to `stream` (the buffers clasfv_forward
 * carves out of it and the slack between them) with `byte`, by hipMemsetAsync on that stream:
 * stream-ordered, no synchronisation. For tests that a result does not depend on what the arena held
 * (0xFF in every byte is a NaN in fp32 and in bf16). CLASFV_EINVAL for a null handle, a byte outside
 * [0, 255], or a stream no clasfv_forward / clasfv_run_decoder has created a context for yet. */
int clasfv_fill_workspace(clasfv_t h, int byte, void* stream);
/* The arena of the context that belongs to `stream`: its device address in *base_dev and its size in
 * *bytes (either may be NULL). The arena is the library's: read it, after synchronising the stream, and
 * write it only through clasfv_fill_workspace; the address holds until a forward of a larger shape on
 * the stream, or a fifth stream, replaces the arena. For tests that compare what a forward wrote with
 * clasfv_forward_plan. CLASFV_EINVAL as clasfv_fill_workspace: a null handle, or a stream without a
 * context. */
int clasfv_workspace_view(clasfv_t h, void* stream, void** base_dev, int64_t* bytes);

/* ---- diagnostics: the launch plan (new exports only: the ABI revision is unchanged) ----------- */
/* What clasfv_forward issues for N clips of (T, H, W) on an engine of compute dtype `dtype` and kernel
 * variants `variants`, recorded by the forward's own walk of the network (the same sub-batch loop, the
 * same layout, the same kernel choice and split-K rule, with nothing launched): every launch in issue
 * order with the memory it reads and writes, the fork and join events of the side stream as markers,
 * and the buffers of each sub-batch's arena layout. Host arithmetic only: needs neither a handle nor a
 * device. DESIGN.md, "The arena's contract", states what a plan must satisfy; tests/plan_audit.py
 * checks it. */
enum {
  CLASFV_PLAN_PACK = 0,       /* pack_input_kernel: the clip into XIN */
  CLASFV_PLAN_CONV = 1,       /* a conv kernel (with a split granted it writes partial sums, not y) */
  CLASFV_PLAN_SPLIT_SUM = 2,  /* split_sum_kernel: the partial sums, bias, residual and ReLU into y */
  CLASFV_PLAN_DEC_INDEX = 3,  /* decoder_index_kernel: the decoder's source-index table */
  CLASFV_PLAN_DECODER = 4,    /* decoder_kernel */
  CLASFV_PLAN_FORK = 5,       /* marker: the side stream waits for everything issued on the caller's so far */
  CLASFV_PLAN_JOIN = 6        /* marker: the caller's stream waits for everything issued on the side stream so far */
};
/* What a range is to its launch. */
enum {
  CLASFV_PLAN_X = 0,     /* the conv's input, x_elem bytes per element */
  CLASFV_PLAN_X2 = 1,    /* the second input of the dual projection, x_elem */
  CLASFV_PLAN_RES = 2,   /* the residual, y_elem */
  CLASFV_PLAN_Y = 3,     /* the output, y_elem */
  CLASFV_PLAN_PART = 4,  /* split-K partial sums, fp32 */
  CLASFV_PLAN_IDX = 5,   /* the decoder's index table, 16-byte entries */
  CLASFV_PLAN_TAP = 6    /* a projected tap the decoder reads, fp32 */
};
/* Buffer ids of the caller's tensors; offsets are bytes from the tensor's start. The arena's buffers
 * have the ids 0 .. of clasfv_plan_buffer_t. */
enum { CLASFV_PLAN_EXT_CLIP = -1, CLASFV_PLAN_EXT_SEG = -2, CLASFV_PLAN_EXT_MOTION = -3 };
#define CLASFV_PLAN_MAX_RANGES 8
typedef struct clasfv_plan_range {
  int32_t buffer; /* arena buffer id, or CLASFV_PLAN_EXT_* */
  int32_t role;   /* CLASFV_PLAN_X .. */
  int32_t write;  /* 1: written, 0: read */
  int32_t pad_;
  int64_t offset; /* bytes from the arena's base (from the tensor's start for CLASFV_PLAN_EXT_*) */
  int64_t bytes;
} clasfv_plan_range_t;
typedef struct clasfv_plan_launch {
  int32_t sub_batch;    /* index of the sub-batch of the call */
  int32_t stream;       /* 0: the caller's stream, 1: the side stream */
  int32_t kind;         /* CLASFV_PLAN_PACK .. */
  int32_t conv;         /* clasfv_conv_info's index as the launch log reports it, or -1 */
  const char* kernel;   /* static string: the kernel's name as clasfv_kernel_timing reports it ("" for a marker) */
  int32_t split_asked;  /* split-K factor the per-clip rule asks for (1: none) */
  int32_t split_granted; /* the factor the launch runs with */
  int32_t x_c8, y_c8, relu, has_res;
  int32_t x_elem, y_elem; /* bytes per element of the input and of the output */
  int32_t n_ranges, pad_;
  clasfv_plan_range_t range[CLASFV_PLAN_MAX_RANGES];
} clasfv_plan_launch_t;
typedef struct clasfv_plan_buffer {
  int32_t sub_batch;   /* the layout is per sub-batch: a shorter last one has its own */
  int32_t clips;       /* clips of the sub-batch */
  int32_t id;          /* 0 ..: XIN, S0, X0, MID, TA, DSB, L1A, L1, ... P01, PP2, PP3, PP4, DIDX */
  int32_t pad_;
  const char* name;    /* static string */
  int64_t offset, bytes; /* of the buffer in the arena; bytes includes no slack */
  int64_t total;       /* bytes of the sub-batch's whole layout; the first one's is the arena clasfv_forward allocates */
} clasfv_plan_buffer_t;
/* Writes up to cap_launches launches and cap_buffers buffer rows and the counts there are in *n_launches
 * and *n_buffers (any pointer may be NULL with its cap 0: call once to size, once to fill). CLASFV_EINVAL
 * for N < 1, an unknown dtype or variant bit, or a cap smaller than the count when its array is given;
 * CLASFV_EBADSHAPE as clasfv_forward. */
int clasfv_forward_plan(int N, int T, int H, int W, int dtype, int variants, int cap_launches,
                        clasfv_plan_launch_t* launches, int* n_launches, int cap_buffers,
                        clasfv_plan_buffer_t* buffers, int* n_buffers);
/* Conv i of an engine of compute dtype `dtype`, as clasfv_conv_info reports it for a handle of that
 * dtype (prefixes and tap omitted), without a handle or a device. */
int clasfv_plan_conv_info(int dtype, int i, int channels[5], int kernel[3], int stride[3], int padding[3],
                          int* in_dtype, int* out_dtype);

/* ---- diagnostics: one layer alone (for layer-level tests; not on the reference's interface) - */
/* New exports only: the ABI revision is unchanged. Convs are numbered in execution order: the
 * backbone's (stem.0, stem.3, layer1.0.conv1.0.0, ...), then the decoder's tap projections P01 (dual
 * input: stem tap and layer1 tap), P2, P3, P4. */
int clasfv_conv_count(clasfv_t h);
/* Conv i for the handle's current compute dtype. prefix / bn_prefix: state-dict prefixes of the conv
 * weight and its BatchNorm ("" for a projection, whose weights are columns of comb_1_layer: *tap is
 * its tap 0, 2, 3 or 4, and -1 for a backbone conv). channels = {cin, cout, cin_p, cout_p, cin2}
 * (cin_p, cout_p: padded widths of the engine's tensors; cin2: width of the second input, P01 only);
 * kernel, stride, padding as (t, h, w); in / out dtype CLASFV_DTYPE_*. Any output pointer may be NULL. */
int clasfv_conv_info(clasfv_t h, int i, const char** prefix, const char** bn_prefix, int* tap, int channels[5],
                     int kernel[3], int stride[3], int padding[3], int* in_dtype, int* out_dtype);
/* Run conv i alone, exactly as clasfv_forward would (same kernel choice, variants, weight images and
 * split-K rule), on caller-owned device tensors in the engine's layouts: x (N,T,H,W,cin_p)
 * channels-last, or 8-channel-blocked [cin_p/8][N*T*H*W][8] when x_c8; y and res (may be NULL, may
 * alias y) the same over the conv's output voxels and cout_p; x2 the second input of P01 (NULL
 * otherwise); dtypes as clasfv_conv_info reports. scratch: split-K partial sums (4 * M * cout_p
 * floats enable it; NULL / 0: never split). *kernel_name: the kernel that ran (static string).
 * CLASFV_EINVAL for a layout the chosen kernel does not take. The kernel is the one a single clip of
 * (T, H, W) runs on; CLASFV_EBADSHAPE, with nothing launched and *kernel_name set to that kernel, when
 * the N clips are past what it addresses (2^31 input bytes for the F(4x4) kernels, 2^31 elements for
 * conv_wino_q / conv_wino / conv_winot / conv_twalk_bf16, 2^30 voxels for the bf16 patch kernels, 2^32
 * input elements for conv_dma / conv_dma_x3) or when the input or the output has 2^31 voxels or more. */
int clasfv_run_conv(clasfv_t h, int i, const void* x_dev, int N, int T, int H, int W, const void* x2_dev,
                    const void* res_dev, int relu, int x_c8, int y_c8, void* y_dev, void* scratch_dev,
                    int64_t scratch_bytes, const char** kernel_name, void* stream);
/* Run the decoder alone over caller-supplied 64-channel projected taps (channels-last fp32) with the
 * handle's head weights: p01 at (T, H', W'), H' = (H - 1) / 2 + 1, and p2, p3, p4 each halving T, H'
 * and W' again the same way (d -> (d - 1) / 2 + 1). H % 8 == 0 and W % 16 == 0, every tap below 2^31
 * floats and the grid N * T * (H / 8) * (W / 16) below 2^31 blocks (CLASFV_EBADSHAPE, before any launch or
 * allocation). */
int clasfv_run_decoder(clasfv_t h, const float* p01_dev, const float* p2_dev, const float* p3_dev,
                       const float* p4_dev, int N, int T, int H, int W, float* seg_dev, float* motion_dev,
                       void* stream);

/* ---- clip plumbing: replaces src/fuse_utils.py:16-100 ----------------------------------------- */
/* Build n clips (n,3,32,H,W) from the normalised video (3,T,H,W). Clip i is frames
 * [table[2i+1], table[2i+1]+32) of the temporally shifted video video[:, table[2i]:], resampled
 * to 32*round(T_k/32) frames (align_corners=False, as F.interpolate) when interpolate != 0 and
 * T_k % 32 != 0. table_dev is a device int32 array of 2n entries. */
int clasfv_build_clips(const float* video_dev, int T, int H, int W, const int32_t* table_dev, int n,
                       int interpolate, float* clips_dev, void* stream);
/* For each shifted pass k < K: softmax over the 2 classes of the pass's clips' logits
 * (logits_dev + pass_clip0[k] clips, each (2,32,H,W)), resample to T_k = T - k*step frames
 * (align_corners=False) when T_k % 32 != 0 and interpolate != 0, argmax -> labels_dev[k][0..T_k)
 * (labels_dev is (K,T,H,W) uint8; frames [T_k, T) of row k are not written). pass_clip0 is a host array
 * of K ints. CLASFV_EINVAL, before anything is launched, for H < 1 or W < 1, T > 65535,
 * (K - 1) * step >= T, a pass whose T_k rounds to no clip (round(T_k / 32) == 0, half to even), and, with
 * interpolate == 0, a pass with T_k % 32 != 0 (its frames would be read from clips that
 * clasfv_build_clips cannot build, or have no logits at all). */
int clasfv_pass_labels(const float* logits_dev, int K, const int32_t* pass_clip0, int T, int step, int H,
                       int W, int interpolate, uint8_t* labels_dev, void* stream);
/* Same labels from logit margins d = l1 - l0 ((n,32,H,W) per clip, clasfv_logit_margin) instead of
 * the two logit planes: bit-identical, because the 2-class softmax depends on the logits only
 * through fl(l1 - l0). Used for the multi-GPU exchange (half the bytes on xGMI). */
int clasfv_pass_labels_margin(const float* margin_dev, int K, const int32_t* pass_clip0, int T, int step,
                              int H, int W, int interpolate, uint8_t* labels_dev, void* stream);
/* margin_dev (n,32,H,W) = logits_dev[:,1] - logits_dev[:,0] for n clips of (2,32,H,W) logits. Pointers
 * need float alignment only (16-byte-aligned ones take the vector path). */
int clasfv_logit_margin(const float* logits_dev, int n, int H, int W, float* margin_dev, void* stream);
/* Per-frame label fusion over the K <= 64 shifted passes (fuse_utils.py:82-100). Output (T',H,W)
 * uint8 with T' = T - (step - 1). method: CLASFV_FUSE_MAJORITY, CLASFV_FUSE_SIMPLE,
 * CLASFV_FUSE_STAPLE or CLASFV_FUSE_ITKVOTING (LabelFusion's methods, fuse_utils.py:95; SIMPLE,
 * STAPLE and ITK voting are restated from their published definitions: LabelFusion itself is absent,
 * so their parity is unpinned). CLASFV_EINVAL for H < 1 or W < 1 and, for MAJORITY / ITKVOTING, T' > 65535.
 * SIMPLE keeps one frame's state in LDS: H * W <= 162816 (160 KB less 1 KB; e.g. 403 x 403), else
 * CLASFV_EBADSHAPE; the packed kernel (K <= 16) serves H * W <= 53248, the generic one everything else.
 *
 * method | CLASFV_FUSE_CLEAN [| CLASFV_FUSE_CLEAN_HOLES(holesize)]: after the fusion kernel, one more launch
 * on the same stream cleans every fused frame in place (one workgroup per frame, the frame in LDS; no
 * workspace): cleanupBinary of the reference (src/utils/camus_validate.py:284-352) for label 1 -- keep the
 * connected component of largest filled area, fill its holes below holesize. With K = 1 and
 * CLASFV_FUSE_MAJORITY the call cleans an existing 0/1 mask video. A new flag only: the ABI revision is
 * unchanged, and every method without the flag launches exactly what it launched before. The rule, per
 * fused frame (this statement is the definition; scikit-image is the reference's implementation of it):
 *   1. Members are the pixels equal to 1. Components of members are 8-connected (skimage.measure.label's
 *      default in 2-D). A frame without members is left as it is.
 *   2. The filled area of a component R is H * W less the pixels outside R that an 8-connected path of
 *      pixels outside R joins to the outside of the frame, the frame taken as padded with one ring of
 *      non-members (regionprops' filled_area: binary_fill_holes with a 3 x 3 structure of ones on the
 *      region's own image). Other components lying in R's holes count towards R.
 *   3. The component of greatest filled area is kept; among equals, the one whose first pixel in row-major
 *      order comes first. (The reference leaves a tie to the order numpy.argsort happens to give, so parity
 *      at a tie is undefined; this rule is defined.)
 *   4. Of the pixels outside the kept component, every 4-connected component of fewer than holesize pixels
 *      joins it, whether or not it touches the frame edge (remove_small_holes(connectivity=1), which is
 *      remove_small_objects on the complement and does not look at the border: a corner pocket cut off by
 *      the kept component is filled). holesize = 1 fills nothing.
 *   5. A pixel becomes 1 if kept or filled; otherwise 0 where it was 1; otherwise it keeps its value (ITK
 *      voting's undecided 2 passes through unless filled over).
 * The result is idempotent, and a frame's bytes do not depend on T', on the frame's place in the call or on
 * thread order. scikit-image is not available to this project, so the rule's parity is unpinned, like
 * SIMPLE's and STAPLE's. CLASFV_EINVAL, before any HIP call, for hole-threshold bits without
 * CLASFV_FUSE_CLEAN, bit 31 or any other unknown bit; CLASFV_EBADSHAPE, before any launch (so nothing is
 * fused either), for H * W > CLASFV_CLEAN_MAX_PIXELS with the flag. */
int clasfv_fuse_votes(const uint8_t* labels_dev, int K, int T, int step, int H, int W, int method,
                      uint8_t* fused_dev, void* stream);

/* ---- motion warp (src/transform_utils.py:14-34 + grid_sample) ------------------------------------ */
/* out (N,C,H,W) = bilinear sample of img at (linspace_W[j] + motion[n,0,i,j],
 * linspace_H[i] + motion[n,1,i,j]), border padding, align_corners=False. motion is (N,2,H,W) with
 * arbitrary element strides for n and the channel (so a slice motion[:, 0:2, t] of (N,4,T,H,W) can
 * be passed directly): element (n,c,i,j) at motion_dev[n*m_sn + c*m_sc + i*W + j]. img_dev and motion_dev
 * may overlap each other; out_dev must overlap neither. CLASFV_EINVAL, before any HIP call, for a null
 * pointer, N, C, H or W < 1, or out overlapping img or motion (the bytes from the first to the last
 * element the strides reach). */
int clasfv_warp(const float* img_dev, int N, int C, int H, int W, const float* motion_dev, int64_t m_sn,
                int64_t m_sc, float* out_dev, void* stream);

/* Gradients of clasfv_warp (training losses, src/clasfv_losses.py:29-136, backpropagate through it):
 * grad_img_dev (N,C,H,W) += d loss / d img (atomically accumulated: zero it first; may be NULL),
 * grad_motion_dev (N,2,H,W) dense = d loss / d motion (may be NULL), from grad_out_dev (N,C,H,W).
 * grad_motion is bit-exact vs PyTorch's CPU grid_sample backward; grad_img matches it to float
 * rounding (different summation order). motion strides as in clasfv_warp. The inputs may overlap each
 * other; CLASFV_EINVAL, before any HIP call, for grad_img or grad_motion overlapping an input or each
 * other. */
int clasfv_warp_backward(const float* grad_out_dev, const float* img_dev, int N, int C, int H, int W,
                         const float* motion_dev, int64_t m_sn, int64_t m_sc, float* grad_img_dev,
                         float* grad_motion_dev, void* stream);

/* ---- tracking (src/visualization_utils.py:58-130) ------------------------------------------------ */
/* A chain of clasfv_warp steps that keeps every frame: out (P,N,C,H,W), time-major and dense; frame p is
 * img (N,C,H,W) after p + 1 warps, through motion frames t0, t0 + t_step, ..., t0 + (P-1) * t_step
 * (apply_sequence_deformation called with growing end_index; get_deformed_label_forback's series).
 * motion_dev points at the first channel of the pair to use (the caller offsets to channel 2 for the
 * backward fields, as for clasfv_warp); element (n,c,t,i,j) is at
 * motion_dev[n*m_sn + c*m_sc + t*m_st + i*W + j], so a (N,4,T,H,W) tensor is used in place.
 * mode: CLASFV_TRACK_BILINEAR (each step bit-identical to clasfv_warp) or CLASFV_TRACK_NEAREST
 * (grid_sample mode="nearest": the clipped source coordinate rounded half to even; for label maps).
 * Two paths, the same values bit for bit. LDS path: ONE launch, one workgroup per (n, c) plane, the plane
 * in two LDS buffers of H * W floats (planes of up to CLASFV_TRACK_LDS_MAX_PIXELS fit: 2 * 20480 * 4 B =
 * the 160 KiB of a CU). Step path: P launches through HBM over the whole chip. By default planes of
 * H * W <= CLASFV_TRACK_LDS_AUTO_PIXELS take the LDS path (measured faster there: one CU is VALU-bound on
 * larger planes) and all others the step path; CLASFV_TRACK_FORCE_LDS takes the LDS path for
 * every plane that fits, CLASFV_TRACK_FORCE_STEPS the step path always (tests, A/B timing).
 * Stream-ordered; no handle, no workspace. out_dev must not overlap img_dev. CLASFV_EINVAL, before any
 * HIP call, for a null pointer, P < 1, t_step other than +1 / -1, a used frame outside [0, T), an
 * unknown mode (both FORCE flags included), N, C, H or W < 1 or out overlapping img; CLASFV_EBADSHAPE for
 * H * W or N * C >= 2^31. */
#define CLASFV_TRACK_BILINEAR 0
#define CLASFV_TRACK_NEAREST 1
#define CLASFV_TRACK_FORCE_STEPS 0x100 /* OR into mode: take the per-step path (tests, A/B timing) */
#define CLASFV_TRACK_FORCE_LDS 0x200   /* OR into mode: take the LDS path whenever the plane fits */
#define CLASFV_TRACK_LDS_MAX_PIXELS 20480
#define CLASFV_TRACK_LDS_AUTO_PIXELS 2304
int clasfv_track(const float* img_dev, int N, int C, int H, int W, const float* motion_dev, int64_t m_sn,
                 int64_t m_sc, int64_t m_st, int T, int t0, int t_step, int P, int mode, float* out_dev,
                 void* stream);

/* ---- LV geometry (src/utils/echo_utils.py:259-385, src/visualization_utils.py:487-493) ----------- */
/* Area, long-axis length, the ten disk radii and the Simpson volume of every frame of masks_dev (F,H,W)
 * uint8, in ONE launch (one workgroup per frame, the frame in LDS): get2dPucks(frame == label, (sy, sx))
 * and computeSimpsonVolume of the reference, per frame, in float64. A pixel belongs to the structure iff it
 * equals `label` (so ITK voting's undecided label 2 is background for label 1). area_dev[f] is the pixel
 * count; geom_dev[f * CLASFV_LV_STRIDE ..] holds length, radii[0..9], volume.
 * Per frame, with coordinates (i * sy, j * sx) over the n member pixels: n = 0 gives (1, zeros, 0) and
 * n = 1 gives (0, zeros, 0). Otherwise the axes are the eigenvectors of the sample covariance (divisor
 * n - 1), larger eigenvalue first; an exactly diagonal covariance yields the coordinate axes, i first only
 * when var_i > var_j; each axis k is negated when its own k-th component is negative. The rim is every pixel
 * whose 4-neighbourhood, frame edges replicated, is mixed; each rim pixel less the mean member coordinate is
 * projected onto (major, minor); lo, hi = min, max along the major axis, length = hi - lo; cut k =
 * lo + k * (hi - lo) / 10 and cut 10 = hi; a rim pixel is in slab k iff cut k <= x < cut k + 1 (the pixel
 * attaining hi is in none, as in the reference); radius k = median of |minor| over slab k (mean of the two
 * middle values for an even count, NaN for an empty slab); volume = sum pi * r^2 * length / 10 (NaN when a
 * radius is). A frame without rim (every pixel a member) gives NaN length, radii and volume.
 * The moments are exact integers and min, max and medians exact selections, so a frame's results do not
 * depend on F or on its place in the batch; they agree with the host functions to float64 rounding except
 * where a rim pixel ties with a cut ("LV geometry"). Any rim count up to H * W is served.
 * Stream-ordered; no handle, no workspace; masks_dev needs no alignment. CLASFV_EINVAL, before any HIP
 * call, for a null pointer, F < 1, H or W < 1, label outside [0, 255] or a spacing that is not finite and
 * positive; CLASFV_EBADSHAPE for H * W > CLASFV_LV_MAX_PIXELS. */
#define CLASFV_LV_NPUCKS 10
#define CLASFV_LV_STRIDE 12         /* doubles per frame: length, radii[10], volume */
#define CLASFV_LV_MAX_PIXELS 162816 /* as SIMPLE fusion: one frame's bytes beside the kernel's LDS state */
int clasfv_lv_geometry(const uint8_t* masks_dev, int64_t F, int H, int W, int label, double sy, double sx,
                       int32_t* area_dev, double* geom_dev, void* stream);

/* ---- annotated video (src/visualization_utils.py:346-437, 476-539) ------------------------------ */
/* Frames [first, first + count) of make_annotated_gif's video for a T-frame clip, as out_dev
 * (count, Hp + Ht + Hs, Wo, 3) uint8 RGB, dense; out_dev needs no alignment. New exports only: the ABI
 * revision is unchanged. A frame is three bands, top to bottom; frame i depends on (T, i) and the inputs
 * only, not on first, count or its place in the call.
 *
 * Overlay pane, Hp x Wo: echonet_overlay(gray, seg, vis=False) resized to nearest. From video_dev (3,T,H,W)
 * float32, g = (v0 * 0.2989 + v1 * 0.5870) + v2 * 0.1140 in float64, each product and sum rounded (no FMA).
 * R = G = B = g; a pixel of masks_dev (T,H,W) uint8 that equals `label` has R = G = g + 0.3
 * (labColorMap_EchoNet[1]). With truth_dev (T,H,W) uint8 (may be NULL) the pane is the reference's
 * difference image I_gt instead: R = G = g + 0.3 where prediction == label and truth != label, B = g + 0.3
 * where prediction != label and truth == label. A channel x becomes the byte floor(255 * clip(x, 0, 1)), a
 * NaN the byte 0: truncation is this project's rule (the reference hands its float frames to matplotlib and
 * imagemagick, a path that is not reproducible pixel for pixel and is not the target). Pane pixel (r, c)
 * shows source pixel (min(floor(r * ify), H - 1), min(floor(c * ifx), W - 1)) with
 * ify = 1.0 / ((double)Hp / H), ifx = 1.0 / ((double)Wo / W): INTER_NEAREST as OpenCV's source defines it
 * (the pane is pinned to this rule, not to a cv2 build). Hp and Wo are free, downscaling included; the
 * reference uses Hp = Wo = 553.
 *
 * Title band, Ht x Wo: a copy of title_dev (Ht,Wo,3) uint8, black when title_dev is NULL. Ht may be 0.
 *
 * Curve strip, Hs x Wo (Hs may be 0): the volume curve up to frame i in lime green (50, 205, 50) on black,
 * on the reference's axes: x spans [0, T + 1] over the Wo columns, y spans [vmin - 100, vmax + 100] over the
 * Hs rows, upward, vmin and vmax the least and largest finite volume of the WHOLE video (none finite: a
 * black strip). volume k is volume_dev[k * volume_stride] (doubles; a clasfv_lv_geometry output is read in
 * place with geom_dev + 11 and stride CLASFV_LV_STRIDE). All in float64, every operation rounded:
 *   S = (double)(T + 1) / Wo, yhi = vmax + 100, sy = (double)Hs / (yhi - (vmin - 100)), h = thickness / 2.
 *   Column x of frame i covers the samples [A, B], A = x * S, B = min((x + 1) * S, i); nothing unless A <= B.
 *   For every k from floor(A) to min(ceil(B) - 1, i - 1) with volume k and volume k + 1 both finite:
 *     ta = max(k, A), tb = min(k + 1, B), dv = v[k + 1] - v[k],
 *     va = v[k] + (ta - k) * dv, vb = v[k] + (tb - k) * dv, ya = (yhi - va) * sy, yb = (yhi - vb) * sy,
 *     top = min(ya, yb) - h, bot = max(ya, yb) + h (min(p, q) = p < q ? p : q, max likewise);
 *     row r is lime iff r + 1 > top and r <= bot for some such k ([r, r + 1) meets [top, bot]).
 * So a segment with a NaN or infinite end is not drawn, frame 0 has an empty strip, several samples per column
 * (T + 1 > Wo) are legal and nothing is anti-aliased.
 *
 * workspace_dev: caller-owned device scratch of clasfv_render_workspace_bytes() bytes (vmin and vmax, found
 * on the device by a one-workgroup reduction before the frames), used in stream order: concurrent calls on
 * different streams need different workspaces. Stream-ordered, two launches; no synchronisation, no handle;
 * the volumes never visit the host. CLASFV_EINVAL, before any HIP call, for a null video_dev, masks_dev,
 * volume_dev, workspace_dev or out_dev; T, H, W, Hp or Wo < 1, Ht or Hs < 0; count < 1 or frames outside
 * [0, T); label outside [0, 255]; a thickness that is negative or not finite; volume_stride < 1; volume_dev
 * or workspace_dev not 8-byte aligned; out_dev overlapping an input or the workspace. CLASFV_EBADSHAPE when
 * the output of the call has 2^32 bytes or more (pixel indices are 32-bit: render the video in chunks of
 * frames, which gives the same bytes) or H * W >= 2^31. */
int64_t clasfv_render_workspace_bytes(void);
int clasfv_render_annotated(const float* video_dev, const uint8_t* masks_dev, const uint8_t* truth_dev, int T,
                            int H, int W, const double* volume_dev, int64_t volume_stride,
                            const uint8_t* title_dev, int first, int count, int Hp, int Wo, int Ht, int Hs,
                            int label, double thickness, void* workspace_dev, uint8_t* out_dev, void* stream);

/* ---- preprocessing (motion_segment.py:96-106, src/echonet_dataset.py:38-50) --------------------- */
/* frames_dev (T,Hs,Ws,3) uint8 RGB -> out_dev (3,T,H,W) float32, resized as
 * F.interpolate(size=(T,H,W), mode="trilinear", align_corners=True) on the (1,3,T,Hs,Ws) float
 * video (bit-exact vs PyTorch's CPU kernel). Not normalised: follow with clasfv_zeroone_normalize. */
int clasfv_preprocess_video(const uint8_t* frames_dev, int T, int Hs, int Ws, int H, int W, float* out_dev,
                            void* stream);
/* In place: per channel c of video (3, n_per_channel) subtract the channel min, divide by the max.
 * workspace_dev: caller-owned device scratch of clasfv_zeroone_workspace_bytes() bytes, used in
 * stream order (concurrent calls on different streams need different workspaces). */
int64_t clasfv_zeroone_workspace_bytes(void);
int clasfv_zeroone_normalize(float* video_dev, int64_t n_per_channel, float* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLASFV_H */
