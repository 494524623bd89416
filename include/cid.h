/*
 * cid.h — C ABI of the MI355X-native denoise forward ("cid" = celebrity image denoiser).
 *
 * The reference has no FFI: its boundary for this path is the torch.nn.Module protocol on the
 * object stored in PT_MODELS["denoise"] (reference backend/app.py:319-320).  Each entry point
 * below names the reference interface it stands in for.  All pointers are plain host or device
 * addresses; no torch types cross this boundary.  Device memory (weights blob, workspace, input,
 * output) is owned by the caller — in the Python host layer that is PyTorch-ROCm's allocator.
 *
 * Threading: a handle is not re-entrant — one forward in flight per handle, matching the
 * reference's single-threaded use (backend/app.py:358-359,433).
 * Errors: every function returns CID_OK (0) or a CID_ERR_* code; cid_last_error(h) holds the text.
 */
#ifndef CID_H_
#define CID_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cid_handle_s* cid_handle_t;

enum {
    CID_OK = 0,
    CID_ERR_INVALID = 1,   /* null pointer / bad argument                                   */
    CID_ERR_SHAPE = 2,     /* tensor shape not accepted (e.g. H or W < 4, wrong weight dims) */
    CID_ERR_KEY = 3,       /* unknown state_dict key                                        */
    CID_ERR_STATE = 4,     /* call out of order (forward before weights attached, ...)      */
    CID_ERR_WORKSPACE = 5, /* workspace too small or misaligned                             */
    CID_ERR_HIP = 6        /* a HIP runtime call or kernel launch failed                    */
};

/* Number of parameter tensors (24) and scalars (1,827,587) of the module.
 * reference: DenoiseGenerator.__init__, backend/app.py:39-78. */
#define CID_NUM_PARAMS 24
#define CID_NUM_PARAM_ELEMS 1827587

/* Kernel launches of one forward, in order (names: cid_launch_name). */
#define CID_NUM_LAUNCHES 12

const char* cid_version(void);

/* DenoiseGenerator()  — backend/app.py:320 (constructor; here: host-side state only). */
int cid_create(cid_handle_t* out);
/* garbage collection of the module. */
void cid_destroy(cid_handle_t h);
/* Python exception text — the reference raises; this ABI returns codes + this string. */
const char* cid_last_error(cid_handle_t h);

/*
 * Module.load_state_dict, one tensor at a time — backend/app.py:272 (via load_state_safely,
 * :257-274).  `key` is a reference state_dict key ("down1.0.weight", "up2.bias", ...; any
 * "module." prefix already stripped by the caller), `host_data` fp32 in the reference layout
 * (Conv2d [Cout,Cin,3,3], ConvTranspose2d [Cin,Cout,2,2], bias [Cout]), `shape`/`ndim` its
 * dims.  The tensor is repacked into the kernels' layout inside the handle's host staging blob.
 * Unknown key -> CID_ERR_KEY; wrong shape -> CID_ERR_SHAPE (the reference's size-mismatch error).
 */
int cid_set_weight(cid_handle_t h, const char* key, const float* host_data, const int64_t* shape, int ndim);

/* Module.state_dict()[key] — backend/trainingcode/denoise_gan_code/training.py:361.
 * Unpacks the staged tensor back into reference layout (`host_out` holds `count` floats). */
int cid_get_weight(cid_handle_t h, const char* key, float* host_out, size_t count);

/* How many of the 24 tensors have not been set since cid_create (strict=True check). */
int cid_missing_weights(cid_handle_t h, int* missing);

/* i-th state_dict key in reference order, NULL if i is out of range. */
const char* cid_param_key(int i);

/* Size in bytes of the packed device weights blob (the unit the multi-GPU path broadcasts). */
size_t cid_packed_weights_bytes(void);

/*
 * Module.to(device) for the parameters — backend/app.py:320.  Copies the packed staging blob
 * to `device_blob` (caller-owned, >= cid_packed_weights_bytes(), 256-byte aligned) on `stream`
 * (hipStream_t, may be NULL) and attaches it.
 */
int cid_upload_weights(cid_handle_t h, void* device_blob, void* stream);

/* Copy the packed host staging blob out (`bytes` must equal cid_packed_weights_bytes()): the
 * exact bytes cid_upload_weights sends to the device, for transports that move it themselves. */
int cid_export_packed(cid_handle_t h, void* host_out, size_t bytes);
/* Replace the host staging blob with packed bytes produced by another handle's
 * cid_export_packed / device blob; afterwards all 24 tensors count as set and cid_get_weight
 * returns them in reference layout. */
int cid_import_packed(cid_handle_t h, const void* host_in, size_t bytes);

/*
 * The packed blob built on the DEVICE from the 24 parameter tensors: `dev_params` holds 24 device pointers to fp32 tensors in the
 * reference layouts, in cid_param_key order (down1.0.weight, down1.0.bias, ... upconv1.2.bias), each at least 4-byte aligned.  One
 * kernel on `stream` writes every byte of `device_blob` (caller-owned, >= cid_packed_weights_bytes(), 256-byte aligned; its
 * previous contents do not matter) and the blob is attached: what cid_set_weight x 24 + cid_upload_weights produce for the same
 * values, byte for byte — the Winograd transforms in double rounded once, the half pieces, the LDS slot tables and the zeros of
 * the alignment gaps included — without the device-to-host copies, the host transforms and the upload.  Asynchronous, no host
 * synchronisation, no memcpy.  A training loop calls it after every optimizer step.
 * The handle's HOST copy is NOT updated: cid_get_weight, cid_export_packed, cid_upload_weights and cid_missing_weights keep
 * seeing what cid_set_weight / cid_import_packed last gave it (the convention of cid_disc_pack_weights_device).
 * Outside the byte-for-byte contract: parameter values that are fp32 subnormals, larger than 65504 in magnitude (the half
 * pieces overflow) or not finite.
 *   CID_ERR_INVALID    null dev_params or device_blob; a null parameter pointer or one that is not 4-byte aligned
 *   CID_ERR_WORKSPACE  device_blob not 256-byte aligned
 * All of these are found before anything is launched.
 */
int cid_pack_weights_device(cid_handle_t h, const float* const* dev_params, void* device_blob, void* stream);

/*
 * The segments of the packed blob in blob order: index 0, 1, ... until CID_ERR_INVALID.  `name` is "<family>:<layer>" for the
 * per-layer segments — w (direct kernels), b (bias), u / u42 (Winograd F(2x2,3x3) / F(4x2,3x3) filters), h (fp16 fragments), s16
 * (split16 pieces), raw_w / raw_b (reference-layout copies) —, "tab:32", "tab:16", "tab42:8", "tab42:4" for the LDS slot tables and
 * "hz", "hzs" for the fused last layer's fragments.  A segment's alignment padding counts to it, so the entries tile
 * [0, cid_packed_weights_bytes()) exactly.  Any of the three outputs may be NULL.  Lets a comparison of two blobs name where
 * they differ.
 */
int cid_packed_segment(int index, const char** name, size_t* offset_bytes, size_t* bytes);

/* Adopt a device blob that already holds packed weights (e.g. filled by an RCCL broadcast from
 * the rank that ran cid_upload_weights).  No copy. */
int cid_attach_weights(cid_handle_t h, const void* device_blob);

/* Output spatial size of the forward: Ho = 4*floor(H/4), Wo = 4*floor(W/4) (two floor-mode
 * 2x2 pools, two x2 transposed convs, skip tensors cropped top-left) — backend/app.py:80-103.
 * H or W < 4 -> CID_ERR_SHAPE (the reference raises "Output size is too small"). */
int cid_out_shape(int H, int W, int* Ho, int* Wo);

/* Bytes of scratch device memory one forward of [N,3,H,W] needs (activation arena, NHWC fp32). */
int cid_workspace_bytes(int N, int H, int W, size_t* bytes);

/*
 * Module.__call__(x) / forward — backend/app.py:433 (net(x_pt)), :80-103.
 * in_nchw : device, fp32, contiguous [N,3,H,W], values nominally in [-1,1]  (app.py:401-406)
 * out_nchw: device, fp32, contiguous [N,3,Ho,Wo], tanh range                (app.py:103)
 * workspace: device scratch, 256-byte aligned, >= cid_workspace_bytes(N,H,W)
 * stream  : hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing.
 */
int cid_forward(cid_handle_t h, const float* in_nchw, float* out_nchw, int N, int H, int W,
                void* workspace, size_t workspace_bytes, void* stream);

/*
 * The forward with the reference's pre/post-processing folded into the first and last kernel
 * (SURVEY.md 8f row f1).  Formats:
 *   CID_FMT_F32_NCHW  fp32 [N,3,H,W] — what cid_forward takes/returns
 *   CID_FMT_U8_NHWC   uint8 [N,H,W,3], PIL/numpy image layout.  As input it is normalised on the fly,
 *                     (u8/255 - 0.5)/0.5 in fp32 = ToTensor + Normalize(0.5,0.5), backend/app.py:401-405;
 *                     as output it is (uint8)(clamp(y*0.5+0.5, 0, 1)*255), truncating like
 *                     ToPILImage's mul(255).byte(), backend/app.py:435,471-472.
 * Any combination is allowed; cid_forward == cid_forward_ex(F32_NCHW, F32_NCHW).
 */
enum { CID_FMT_F32_NCHW = 0, CID_FMT_U8_NHWC = 1 };
int cid_forward_ex(cid_handle_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W,
                   void* workspace, size_t workspace_bytes, void* stream);

/*
 * The reference's view transform alone — backend/app.py:435 (y*0.5+0.5, clamp to [0,1]) and :471-472 (ToPILImage: mul(255).byte(),
 * truncating), as the iterated caller applies it to EVERY fed-back iteration (denoise_eavl_iter.py:97-110): a device fp32
 * [N,3,H,W] tensor in tanh range -> device uint8 [N,H,W,3].  Same arithmetic as cid_forward_ex's CID_FMT_U8_NHWC output, for callers that
 * keep the fp32 tensor (to feed it back) and also want its image.  No handle: it needs no weights.
 */
int cid_view_u8(const float* in_nchw, void* out_u8_nhwc, int N, int H, int W, void* stream);

/*
 * The reference server's handling of arbitrary upload sizes (backend/app.py:276-281 get_padding, :384-385
 * transforms.Pad(padding, fill=0) in front of ToTensor/Normalize, :474-480 crop of the result), as index arithmetic in the
 * first and the last kernel — no padded copy of the image and no uncropped output exist:
 *   in   : [N,3,H,W] fp32 or [N,H,W,3] uint8 — the caller's image, UNPADDED
 *   the network runs on [H + pad_top + pad_bottom, W + pad_left + pad_right]; the band around the image is uint8 0, i.e.
 *          (0/255 - 0.5)/0.5 = -1.0 (for CID_FMT_F32_NCHW input the band is -1.0 as well)
 *   out  : [N,3,H,W] fp32 or [N,H,W,3] uint8 — rows [pad_top, pad_top + H) and columns [pad_left, pad_left + W) of the
 *          network's output; that window must exist (it does when the padded size is a multiple of 4, the reference's rule),
 *          otherwise CID_ERR_SHAPE
 * workspace: cid_workspace_bytes(N, H + pad_top + pad_bottom, W + pad_left + pad_right).  With all pads zero and H, W multiples
 * of 4 this is cid_forward_ex.  Pads outside [0, 4096] -> CID_ERR_INVALID.
 */
int cid_forward_padded(cid_handle_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W,
                       int pad_left, int pad_top, int pad_right, int pad_bottom, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Same forward, with a HIP event recorded on `stream` around every kernel launch; synchronises
 * the stream and writes the CID_NUM_LAUNCHES per-launch durations in milliseconds to launch_ms.
 * Measurement aid for bench.py's roofline object; not part of the reference surface.
 */
int cid_forward_timed(cid_handle_t h, const float* in_nchw, float* out_nchw, int N, int H, int W,
                      void* workspace, size_t workspace_bytes, void* stream, float* launch_ms);

/*
 * Per-launch timing across many forwards without a host sync per forward (bench.py's timed
 * region).  cid_timing_begin arms the handle: each of the next `max_forwards` cid_forward calls
 * records CID_NUM_LAUNCHES+1 HIP events on its stream.  cid_timing_end synchronises `stream`,
 * writes the per-launch durations summed over the recorded forwards (milliseconds) to
 * launch_ms_sum[CID_NUM_LAUNCHES] and the number of forwards to *forwards, and disarms.
 */
int cid_timing_begin(cid_handle_t h, int max_forwards);
int cid_timing_end(cid_handle_t h, void* stream, float* launch_ms_sum, int* forwards);

/* Name of the i-th launch ("down1.0", ..., "upconv1.2"), the reference layer(s) it computes. */
const char* cid_launch_name(int i);
/* Device kernel symbol prefix of the i-th launch under the handle's current algorithm (to match
 * rocprofv3 kernel-trace rows). */
const char* cid_launch_kernel(cid_handle_t h, int i);

/*
 * Algorithm of the eight GEMM-shaped 3x3 convolutions (down1[2] ... upconv1[0]); head, tail and the
 * transposed convolutions are unaffected (except under CID_ALGO_SPLIT16, which runs the transposed convolutions in its own arithmetic too).  All compute the reference's nn.Conv2d(k=3,p=1) in fp32 (exact-fp32 MFMA):
 *   CID_ALGO_DIRECT     implicit GEMM, 9 taps: 9 multiplies per output pixel and (ci,co)
 *   CID_ALGO_WINOGRAD64 Winograd F(2x2,3x3): 4 multiplies per pixel (round 1's default)
 *   CID_ALGO_WINOGRAD42 Winograd F(4x2,3x3), tiles 4 wide x 2 high, interpolation points 0, +-3/4, +-3/2, inf: 3 multiplies
 *                       per pixel: the default
 *   CID_ALGO_SPLIT16    (round 4, OPT-IN, not exact-fp32 MFMA) split-operand convolution on the fp16 MFMA: fp32 tensors in and out; every fp32 operand is
 *                       taken as hi + lo with hi = half(x), lo = half(x - hi) (22 bits of mantissa), every product as hi*hi + hi*lo + lo*hi on
 *                       v_mfma_f32_16x16x32_f16 with fp32 accumulators (lo*lo, 2^-22 relative, dropped).  9 multiplies per pixel (direct form), each on three
 *                       half products.  Measured against a float64 evaluation (profiles/r04_accuracy_study.txt, He-gain weights, faces / white noise, units of
 *                       1e-6): 5.1 / 8.6 where the exact-fp32 direct kernel has 4.2 / 6.3, the Winograd default 2.2 / 4.0 and ATen fp32 2.2 / 2.5 — the least accurate
 *                       of the four algorithms, inside the 1e-5 contract with the thinnest margin.  It passes every 1e-5 parity test of the suite, but its arithmetic type is
 *                       "fp32 operands as two halfs, fp16 MFMA, fp32 accumulate": the default and the headline benchmark stay on CID_ALGO_WINOGRAD42.
 *                       CID_TAIL_FUSED works under it: upconv1[2]'s contraction runs in the same split-operand arithmetic in upconv1[0]'s epilogue and
 *                       leaves the 27 fp32 planes k_conv_tail_z sums.
 * (value 1 was round 1's first Winograd kernel, removed: same bits as WINOGRAD64, slower.)
 * No reference counterpart (the reference leaves the choice to ATen/oneDNN/cuDNN).
 */
enum { CID_ALGO_DIRECT = 0, CID_ALGO_WINOGRAD64 = 2, CID_ALGO_WINOGRAD42 = 3, CID_ALGO_SPLIT16 = 4 };

/*
 * Storage type of activations and weights between the first and the last kernel (BASELINE configs[4]):
 *   CID_DTYPE_F32  the reference's arithmetic (default): fp32 storage, exact-fp32 MFMA
 *   CID_DTYPE_F16  IEEE half storage, v_mfma_f32_32x32x16_f16 with fp32 accumulators, bias/ReLU/pool in fp32,
 *                  one rounding to half per stored element; direct implicit GEMM for all ten GEMM layers.
 * The caller-side tensors (cid_forward / cid_forward_ex) keep their formats; only the arena and the weight
 * segments read change.  A different numerical contract from the reference's fp32 (tolerances: tests/): against the fp32
 * forward, max|delta| <= 5e-3 on image-like inputs and <= 7e-3 on white noise in [-1, 1] with He-gain weights (the format's
 * own error: 4.7e-3 at most over 64 images of 128x128 in a CPU emulation of the rounding points, plus a margin).  Each
 * launch's stored halfs are round-to-nearest-even (subnormals kept) of its fp32 result within the fp32 summation bound
 * (oracle/f16_oracle.py, tests/test_f16_launches.py).
 */
enum { CID_DTYPE_F32 = 0, CID_DTYPE_F16 = 1 };   /* (the half path's kernels use v_mfma_f32_16x16x32_f16 since round 2) */
int cid_set_compute_dtype(cid_handle_t h, int dtype);
int cid_get_compute_dtype(cid_handle_t h, int* dtype);
int cid_set_conv_algo(cid_handle_t h, int algo);
int cid_get_conv_algo(cid_handle_t h, int* algo);
/*
 * How the last layer (upconv1[2] = Conv2d(64,3,3,p=1) + tanh, backend/app.py:77,103) runs; same function:
 *   CID_TAIL_FUSED  (default) its 64 -> 27 (tap x channel) contraction runs in the epilogue of upconv1[0]'s kernel, on the
 *                   tile still in LDS; the last launch is the nine-tap shifted sum + bias + tanh over 27 fp32 planes (CID_DTYPE_F32; needs
 *                   a Winograd algorithm or CID_ALGO_SPLIT16, with CID_ALGO_DIRECT the handle behaves as CID_TAIL_TILES) or over 7 planes
 *                   of 4 halfs (the same 27 rows 3 tap + co and a pad; CID_DTYPE_F16, with every conv algorithm, round 4).
 *   CID_TAIL_BANDS  separate kernel: a workgroup slides down a band of rows, the contraction is computed once per pixel
 *                   (images up to 128 pixels wide, wider ones take CID_TAIL_TILES; CID_DTYPE_F16 takes its own tiled kernel)
 *   CID_TAIL_TILES  separate kernel: 8x32-pixel tiles, the contraction is computed over each tile's halo (round 1's kernel)
 */
enum { CID_TAIL_FUSED = 0, CID_TAIL_BANDS = 1, CID_TAIL_TILES = 2 };
int cid_set_tail_algo(cid_handle_t h, int algo);
int cid_get_tail_algo(cid_handle_t h, int* algo);
/* Algorithmic work of the i-th launch for an [N,3,H,W] forward: conv/convT FLOPs (2*MAC) and
 * fp32 bytes (input activations + output activations + weights, each once) — SURVEY.md 8(a). */
int cid_launch_work(int i, int N, int H, int W, double* flops, double* bytes);
/* The same per LAUNCH under the handle's configuration: launches 1 and 3 also count the 2x2-pooled tensor they write (pool1 / pool2,
 * backend/app.py:48,56, run in their epilogues: SURVEY.md 8(a) rows a3 / a6 less the pools' reads); with CID_TAIL_FUSED launch 10 also carries
 * upconv1[2]'s FLOPs and writes 27 planes instead of 64 channels, and launch 11 only sums, adds the bias and applies tanh. */
int cid_launch_work_ex(cid_handle_t h, int i, int N, int H, int W, double* flops, double* bytes);

/*
 * Where the output of one of the reference module's stages lives in the workspace of an [N,3,H,W] forward (NHWC,
 * fp32 — or half elements from the same base when the compute dtype is CID_DTYPE_F16).  `stage` is the attribute name of
 * the reference module whose forward-hook output it is (backend/app.py:42-78): "down1", "pool1", "down2", "pool2",
 * "bottleneck", "up2", "upconv2", "up1", plus "upconv1.0" (upconv1[0] after its ReLU: the last layer's input) and the first
 * convolution of each two-conv block after its ReLU: "down1.0" (64 x H x W), "down2.0" (128 x H/2 x W/2), "bottleneck.0"
 * (256 x H/4 x W/4) and "upconv2.0" (128 channels, the size of "up2").  Element (n, y, x, c) of the stage is at
 *     offset_bytes/elem_size + ((n*Hs + y)*Ws + x)*pixel_stride + channel_offset + c        for y < Hs, x < Ws, c < C.
 * With CID_TAIL_FUSED the "upconv1.0" region holds the fused tail's z planes instead and the formula does not apply; z row
 * r = 3 tap + co (tap = 3 kh + kw) is upconv1[2]'s contraction sum_ci upconv1.0[ci] * W[co][ci][kh][kw] at each pixel:
 *     CID_DTYPE_F32  fp32 z[N][27][Hs][Ws]
 *     CID_DTYPE_F16  half z[N][7 groups][Hs][Ws][4]: row r is slot r % 4 of group r / 4; slot 3 of group 6 is a zero pad.
 * Skip tensors ("down1", "down2") are stored only over the region the concat keeps (top-left crop, app.py:90-92,97-99).
 * "upconv1" (pre-tanh) is never stored: it is fused into the last kernel.  Testing aid for per-stage parity.
 */
int cid_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                   int* pixel_stride, int* channel_offset);

/*
 * Multi-GPU (one process per GPU, batch sharded): the job's ONE collective — an RCCL broadcast of the
 * packed weights blob over xGMI from the rank that loaded the checkpoint — as a C entry point, so that a host which is
 * not PyTorch can distribute weights too.  The reference has no distributed code; nothing here replaces a reference call.
 *   comm   : an ncclComm_t (opaque pointer) spanning the ranks; create it with RCCL directly or with the three helpers
 *            below (thin wrappers over ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy; the 128-byte unique id
 *            travels from rank 0 to the others by whatever control channel the host has).
 *   before : root has run cid_upload_weights; every other rank has attached an allocated, 256-byte aligned device buffer
 *            of cid_packed_weights_bytes() with cid_attach_weights.
 *   after  : every rank's attached blob holds root's weights (in place, on `stream`); non-root handles have also
 *            refreshed their host copy (the call synchronises `stream` there), so cid_get_weight returns the new tensors.
 * RCCL is resolved at run time from the process (dlopen of librccl.so.1): CID_ERR_STATE if it is not available.
 */
int cid_comm_available(void);   /* 1 if RCCL could be resolved in this process (the three calls below can work), else 0; no side effect */
int cid_comm_unique_id(void* id128);
int cid_comm_init_rank(void** comm, int nranks, const void* id128, int rank);
int cid_comm_destroy(void* comm);
int cid_comm_count(void* comm, int* nranks);   /* ncclCommCount: how many ranks RCCL itself says the communicator spans */
int cid_broadcast_weights(cid_handle_t h, void* comm, int root, int rank, void* stream);

/*
 * Image-quality metrics of denoised batches — the reference denoise trainer's evaluation, DenoiseGANTrainer.evaluate
 * (backend/trainingcode/denoise_gan_code/training.py:378-392, once per batch at :432), on device tensors.  LPIPS (:282) has weights
 * and therefore its own handle: cid_lpips below.  No handle here: no weights are involved.
 *
 * For each image pair (a, b) of a batch (3 channels, H x W), three per-image values:
 *   PSNR     skimage peak_signal_noise_ratio(a, b, data_range=2.0) on float32 inputs (training.py:380): d = a - b and d*d in fp32,
 *            mse = mean of d*d over the 3*H*W values accumulated in fp64, psnr = 10*log10(2.0^2 / mse); mse == 0 gives +inf.
 *   SSIM     skimage structural_similarity(a, b, channel_axis=2, data_range=2.0) with its defaults (training.py:381): per channel,
 *            7x7 uniform (box) means ux, uy, uxx, uyy, uxy of a, b, a^2, b^2, ab; sample covariance cn = 49/48: vx = cn(uxx-ux^2),
 *            vy = cn(uyy-uy^2), vxy = cn(uxy-ux*uy); C1 = (0.01*2)^2, C2 = (0.03*2)^2;
 *            S = (2ux*uy+C1)(2vxy+C2) / ((ux^2+uy^2+C1)(vx+vy+C2)), averaged over the pixels at least 3 from every border (skimage's
 *            crop(S, 3): no border mode is involved).  The image's value is the mean of its 3 channels.  Needs H >= 7 and W >= 7.
 *   MS-SSIM  pytorch_msssim.MS_SSIM(data_range=1.0) v1.0 (training.py:283, :390) on x*0.5+0.5 (fp32): 11-tap Gaussian window,
 *            sigma 1.5, float32 like torch (exp(-(k-5)^2/4.5), normalised), applied as a VALID separable convolution;
 *            per level and channel, with Gaussian moments and compensation 1, C1 = 0.01^2, C2 = 0.03^2:
 *              cs = mean((2sxy+C2)/(sx^2+sy^2+C2)),  ssim = mean((2mx*my+C1)/(mx^2+my^2+C1) * cs_map);
 *            5 levels, between them avg_pool2d(2, stride 2, padding (H%2, W%2), count_include_pad) of both images (a side s becomes
 *            (s+1)/2); per channel prod_{l<4} relu(cs_l)^w_l * relu(ssim_4)^w_4 with w = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333];
 *            the image's value is the mean of its 3 channels.  Needs min(H, W) > 160, as pytorch_msssim asserts.
 * Operand formats (each operand its own): CID_FMT_F32_NCHW fp32 [N,3,H,W] in [-1,1]; CID_FMT_U8_NHWC uint8 [N,H,W,3], read as
 * (u/255 - 0.5)/0.5 in fp32 with true divisions (the forward's u8 input arithmetic): a u8 image and its normalised fp32 copy give
 * bit-identical metrics.
 *
 * cid_quality_workspace_bytes: device scratch one cid_quality call needs (per-tile partial sums; with MS-SSIM the pooled levels 1-4).
 * cid_quality: asynchronous on `stream` (hipStream_t, NULL = default stream).  out: device double [N][3] = psnr_db, ssim, ms_ssim;
 * columns not requested are NaN.  Every argument is checked on the host before any launch:
 *   CID_ERR_INVALID    null pointer, unknown format, misaligned fp32 operand or out, metrics 0 or with unknown bits
 *   CID_ERR_SHAPE      N < 1, H or W < 7 with SSIM, min(H, W) <= 160 with MS-SSIM, a plane of 2^31 pixels or more
 *   CID_ERR_WORKSPACE  workspace smaller than cid_quality_workspace_bytes() or not 256-byte aligned
 * Reductions are deterministic (per-tile partial sums reduced in a fixed order in fp64, no atomics) and an image's tiling does not
 * depend on N: an image's three values are bit-identical whatever batch it is in.
 */
enum { CID_METRIC_PSNR = 1, CID_METRIC_SSIM = 2, CID_METRIC_MS_SSIM = 4 };
int cid_quality_workspace_bytes(int N, int H, int W, int metrics, size_t* bytes);
int cid_quality(const void* a, int a_fmt, const void* b, int b_fmt, int N, int H, int W, int metrics, double* out,
                void* workspace, size_t workspace_bytes, void* stream);

/*
 * Noise synthesis — the five noise kinds the reference's denoise trainer is trained on (DenoiseDataset over
 * ['gaussian', 'salt_pepper', 'speckle', 'poisson', 'uniform'], backend/trainingcode/denoise_gan_code/training.py:247), each made
 * from a clean uint8 image as noise_generation.py:6-39 does, with the reference's formulas and defaults.  No handle: no weights.
 *
 * clean_u8_nhwc and out_u8_nhwc are device uint8 [N,H,W,3]; out may equal clean (in place) but must not overlap it otherwise.
 * Random draws come from counter-based splitmix64 streams, not np.random: image n uses seed' = seed + first_index + n and element
 * e = (y*W + x)*3 + c; u = (z >> 11) * 2^-53 with z = splitmix64(splitmix64(seed' ^ stream) + e).  An image's noise depends only on
 * (seed, its global index first_index + n, H, W).  Arithmetic is float64 in the order below; the result is clip(v, 0, 255)
 * truncated to uint8.  The bit-defined restatement is synth.add_noise_np.
 *   GAUSSIAN     params (mean, sigma), reference (0, 25), noise_generation.py:6-10: z = sqrt(-2 log(1-u1)) cos(2 pi u2) on streams
 *                1 and 2, v = img + (mean + sigma*z).  With mean 0 this is exactly synth.add_gaussian_noise (bench.py's inputs).
 *   SPECKLE      params (mean, sigma), reference (0, 0.1), :24-28: the same z on streams fnv1a64("noise:speckle:u1" / ":u2"),
 *                v = img + img*(mean + sigma*z).
 *   UNIFORM      params (low, high), reference (0, 25), :35-39: v = img + (low + (high-low)*u), stream fnv1a64("noise:uniform").
 *   POISSON      no params, :30-33: lambda = the pixel value, k by inversion (p = exp(-lambda), c = p; while u >= c and k < 1023:
 *                k += 1, p = (p*lambda)/k, c += p) on stream fnv1a64("noise:poisson"); exp(-lambda) is the host libm's.  The result is
 *                k mod 256: the reference's np.random.poisson(u8).astype(np.uint8) wraps, so about 48 % of the pixels at 255 come out
 *                dark (P(k >= 256 | lambda = 255)).  This quirk is reproduced on purpose.
 *   SALT_PEPPER  params (salt_prob, pepper_prob), reference (0.02, 0.02), :12-22: n = int(float(H*W*3) * prob) draws of each;
 *                draw j: row = floor(z_row(j) * (H-1) / 2^64), col = floor(z_col(j) * (W-1) / 2^64) (the last row and column are never
 *                hit, as with randint(0, H-1)); all 3 channels of the pixel become 255 (salt), then 0 (pepper: pepper wins a
 *                collision).  Streams fnv1a64("noise:salt_pepper:salt_row" / ":salt_col" / ":pepper_row" / ":pepper_col").
 * Asynchronous on `stream` (hipStream_t, NULL = default stream).  Every argument is checked on the host before any launch:
 *   CID_ERR_INVALID  null pointer, unknown kind, nparams not the kind's count (params may be NULL when it is 0), a non-finite
 *                    parameter, sigma < 0, a probability outside [0, 1], low > high
 *   CID_ERR_SHAPE    N < 1, H or W < 1 (< 2 for SALT_PEPPER: numpy's randint(0, 0) raises), H*W*3 >= 2^31
 */
enum { CID_NOISE_GAUSSIAN = 0, CID_NOISE_SALT_PEPPER = 1, CID_NOISE_SPECKLE = 2, CID_NOISE_POISSON = 3, CID_NOISE_UNIFORM = 4 };
int cid_add_noise(const void* clean_u8_nhwc, void* out_u8_nhwc, int N, int H, int W, int kind, const double* params, int nparams,
                  uint64_t seed, uint64_t first_index, void* stream);

/*
 * The trainer's discriminator — DenoiseDiscriminator (backend/trainingcode/denoise_gan_code/training.py:77-98), which the trainer calls
 * three times per step (:412, :413, :421) in train mode (:397) and whose outputs give the per-epoch "G Loss" / "D Loss" (:414-424, :455).
 * Its own handle: the generator's handle and packed blob are specific to the generator.  cid_disc_forward keeps nothing for a backward
 * pass; cid_disc_forward_saved / cid_disc_backward (below) are the pair that does.
 *
 *   0 Conv2d(3,64,3,p=1)  1 LeakyReLU(0.2)                        2 Conv2d(64,64,3,s=2,p=1)   3 BatchNorm2d(64)   4 LeakyReLU(0.2)
 *   5 Conv2d(64,128,3,p=1)   6 BatchNorm2d(128)   7 LeakyReLU(0.2)   8 Conv2d(128,128,3,s=2,p=1) 9 BatchNorm2d(128) 10 LeakyReLU(0.2)
 *  11 AdaptiveAvgPool2d(1)  12 Conv2d(128,1,1)  13 Sigmoid;   forward(x) = model(x).view(-1): one probability per image.
 * For an H x W input, layer 2 gives H2 = (H-1)/2 + 1 (integer division) and layer 8 H4 = (H2-1)/2 + 1; any H, W >= 1 is valid.
 *
 * cid_disc_set_weight takes the ten convolution tensors by their state_dict keys "model.{0,2,5,8,12}.{weight,bias}" (fp32, reference
 * layout [Cout,Cin,kh,kw] / [Cout]); they are packed into the kernels' layout on the host.  The BatchNorm tensors ("model.{3,6,9}.*")
 * are not staged (CID_ERR_KEY): they are passed as device pointers at every forward, so that train-mode updates land in the caller's
 * own buffers.  cid_disc_upload_weights copies the packed blob (cid_disc_packed_weights_bytes(), 256-byte aligned, caller-owned) to
 * the device and attaches it; it needs all ten tensors (CID_ERR_STATE otherwise).
 *
 * cid_disc_forward: in is fp32 [N,3,H,W] in [-1,1] (CID_FMT_F32_NCHW, what the trainer feeds) or uint8 [N,H,W,3] (CID_FMT_U8_NHWC,
 * decoded as (u/255 - 0.5)/0.5 with the forward's arithmetic: a u8 image and its normalised fp32 copy give identical bits); out_prob
 * is device fp32 [N].  bn[0..2] describe model.3, model.6, model.9:
 *   eval (training = 0): BatchNorm uses the running buffers, (z - running_mean) * rsqrt(running_var + eps) * gamma + beta;
 *            num_batches_tracked and momentum are not read.
 *   train (training = 1): BatchNorm normalises with the batch mean and the biased batch variance over N*Hl*Wl values per channel,
 *            then updates the buffers in place: running = (1 - m) * running + m * batch_stat, with the UNBIASED variance for
 *            running_var, and num_batches_tracked += 1.  m = momentum, or with CID_DISC_MOMENTUM_NONE (nn.BatchNorm2d(momentum=None))
 *            m = 1 / num_batches_tracked after the increment.  The statistics, the updates and the counter run on the device:
 *            there is no host synchronisation inside a forward.  A BatchNorm input with one value per channel (N*H4*W4 == 1) is
 *            CID_ERR_SHAPE, where torch raises "Expected more than 1 value per channel when training".
 * Arithmetic: fp32 convolutions (exact-fp32 MFMA for layers 2, 5, 8), batch statistics, the average pool, the 1x1 layer and the sigmoid
 * in fp64.  Deterministic: per-tile partial sums reduced in a fixed order, no atomics; an image's tiling does not depend on N, so in
 * eval mode an image's probability is bit-identical in any batch.  Asynchronous on `stream` (hipStream_t, NULL = default stream).
 * Every argument is checked on the host before any launch:
 *   CID_ERR_INVALID    null pointer (num_batches_tracked only in train mode), unknown format, misaligned fp32 operand, eps not
 *                      finite or negative, in train mode a momentum that is not finite or negative other than CID_DISC_MOMENTUM_NONE
 *   CID_ERR_SHAPE      N < 1, H < 1, W < 1, H*W >= 2^31, train mode with N*H4*W4 == 1
 *   CID_ERR_WORKSPACE  workspace smaller than cid_disc_workspace_bytes(N, H, W, training) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_disc_losses: the trainer's loss arithmetic of one batch (training.py:412-424) from the two probability vectors of
 * p_real = D(clean) and p_fake = D(denoised) (device fp32 [N]) and the two image batches (fp32 [N,3,H,W] or uint8 [N,H,W,3], each its
 * own format) -> device double out[4] = d_loss = BCE(p_real, 1) + BCE(p_fake, 0), g_loss = content + 0.001 * adv,
 * content_loss = MSE(denoised, clean), adv_loss = BCE(p_fake, 1).  BCE clamps its logs at -100 as nn.BCELoss does.  One workgroup,
 * fp64, fixed order.  CID_ERR_INVALID for a null pointer, an unknown format or a misaligned operand; CID_ERR_SHAPE for N, H or W < 1.
 */
typedef struct cid_disc_s* cid_disc_t;
typedef struct {
    const float* gamma;              /* device fp32 [C] (weight)  */
    const float* beta;               /* device fp32 [C] (bias)    */
    float* running_mean;             /* device fp32 [C], updated in train mode */
    float* running_var;              /* device fp32 [C], updated in train mode */
    int64_t* num_batches_tracked;    /* device int64 [1], updated in train mode */
    double eps;                      /* the container's eps       */
    double momentum;                 /* the container's momentum, or CID_DISC_MOMENTUM_NONE */
} cid_disc_bn;
#define CID_DISC_MOMENTUM_NONE (-1.0)
#define CID_DISC_NUM_WEIGHTS 10
int cid_disc_create(cid_disc_t* out);
void cid_disc_destroy(cid_disc_t d);
const char* cid_disc_last_error(cid_disc_t d);
int cid_disc_set_weight(cid_disc_t d, const char* key, const float* host_data, const int64_t* shape, int ndim);
size_t cid_disc_packed_weights_bytes(void);
int cid_disc_upload_weights(cid_disc_t d, void* device_blob, void* stream);
int cid_disc_workspace_bytes(int N, int H, int W, int training, size_t* bytes);
int cid_disc_forward(cid_disc_t d, const void* in, int in_fmt, float* out_prob, int N, int H, int W, const cid_disc_bn* bn,
                     int training, void* workspace, size_t workspace_bytes, void* stream);
int cid_disc_losses(const float* p_real, const float* p_fake, const void* denoised, int d_fmt, const void* clean, int c_fmt,
                    int N, int H, int W, double* out, void* stream);

/*
 * The discriminator's backward pass (the trainer's d_loss.backward(), training.py:410-417, and the adversarial half of its generator
 * step, :421-425).  Gradients of model.0 ... model.13 in fp32; every reduction accumulates in fp64 in a fixed order, no atomics;
 * the GEMMs of layers 2, 5, 8 (data and weight gradient) run on the exact-fp32 MFMA.  The same call twice gives the same bits, and
 * in eval mode the input gradient of an image does not depend on the batch it sits in.
 *
 * cid_disc_forward_saved is cid_disc_forward with a caller-owned PER-CALL buffer of cid_disc_saved_bytes(N, H, W, training) bytes
 * (256-byte aligned) in place of the workspace: the activated a0, the raw z2, z5, z8, each BatchNorm's (scale, shift) and
 * (mean, invstd) and, in train mode, the statistics slabs stay there for the backward pass.  One buffer per forward call: the
 * trainer runs D(clean) and D(denoised.detach()) before one backward through both.  Probabilities and BatchNorm buffer updates are
 * bit-identical to cid_disc_forward; the argument checks and error codes are the same, with CID_ERR_WORKSPACE for the saved buffer.
 *
 * cid_disc_backward: `in`, N, H, W, `training` and `saved` are those of the cid_disc_forward_saved call to differentiate (the
 * packed weights must still be the ones that call used; bn[l].gamma is read, the other cid_disc_bn fields are not); grad_prob is
 * device fp32 [N], the gradient of the loss with respect to the probabilities.  `g` holds device fp32 pointers for the results in the
 * reference layouts: w[i], b[i] for model.{0,2,5,8,12} ([Cout,Cin,kh,kw] / [Cout]), gamma[l], beta[l] for model.{3,6,9}, input
 * [N,3,H,W].  A null pointer skips that output and the work only it needs (no layer-0 data gradient without `input`; nothing
 * below the deepest layer asked for).  Results OVERWRITE; accumulation is the caller's (autograd's) job.  A uint8 input has no
 * gradient.  Train mode differentiates through the batch statistics of that forward call; eval mode treats the running buffers as
 * constants.  Asynchronous on `stream`, no host synchronisation; workspace of cid_disc_backward_workspace_bytes(), 256-byte aligned.
 *   CID_ERR_INVALID    null in / grad_prob / bn / bn[l].gamma / saved / g / workspace, unknown format, misaligned fp32 pointer,
 *                      training not 0 or 1, g->input with a uint8 input
 *   CID_ERR_SHAPE      as cid_disc_forward
 *   CID_ERR_WORKSPACE  saved buffer or workspace too small or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_disc_pack_weights_device builds the forward's packed blob from the ten parameter tensors in DEVICE memory (fp32, reference
 * layouts, in the order model.0.weight, model.0.bias, model.2.weight, ... model.12.bias) with one kernel on `stream` and attaches
 * it: what cid_disc_set_weight x 10 + cid_disc_upload_weights produce, byte for byte, without the device-to-host copies.  A
 * training loop calls it after every optimizer step.
 */
typedef struct {
    float* w[5];         /* model.0, 2, 5, 8, 12 .weight */
    float* b[5];         /* model.0, 2, 5, 8, 12 .bias   */
    float* gamma[3];     /* model.3, 6, 9 .weight        */
    float* beta[3];      /* model.3, 6, 9 .bias          */
    float* input;        /* fp32 [N,3,H,W]               */
} cid_disc_grads;
int cid_disc_saved_bytes(int N, int H, int W, int training, size_t* bytes);
int cid_disc_forward_saved(cid_disc_t d, const void* in, int in_fmt, float* out_prob, int N, int H, int W, const cid_disc_bn* bn,
                           int training, void* saved, size_t saved_bytes, void* stream);
int cid_disc_backward_workspace_bytes(int N, int H, int W, int training, size_t* bytes);
int cid_disc_backward(cid_disc_t d, const void* in, int in_fmt, const float* grad_prob, int N, int H, int W, const cid_disc_bn* bn,
                      int training, const void* saved, size_t saved_bytes, const cid_disc_grads* g, void* workspace,
                      size_t workspace_bytes, void* stream);
int cid_disc_pack_weights_device(cid_disc_t d, const float* const* dev_params, void* device_blob, void* stream);

/*
 * The SRGAN trainer's discriminator — SRGANDiscriminator (backend/trainingcode/srgan_code/sr_ganTrainGNew.py:54-80), which that
 * trainer calls three times per step (:395-404) for d_loss = BCE(D(hr), 1) + BCE(D(fake), 0) and adv_loss = BCE(D(fake), 1).
 * cid_srd_forward keeps nothing for a backward pass (cid_srd_forward_saved below does).  Its own handle and blob, as cid_disc_* has.
 *
 *   model.0 ... model.10 are DenoiseDiscriminator's layers 0 ... 10 (above); then
 *  11 Conv2d(128,256,3,p=1)  12 BatchNorm2d(256)  13 LeakyReLU(0.2)  14 AdaptiveAvgPool2d(1)  15 Conv2d(256,512,1)  16 LeakyReLU(0.2)
 *  17 Conv2d(512,1,1)  18 Sigmoid;   forward(x) = model(x).view(-1): one probability per image.  H2, H4 as above; any H, W >= 1.
 *
 * cid_srd_set_weight takes the fourteen convolution tensors by their state_dict keys "model.{0,2,5,8,11,15,17}.{weight,bias}" (fp32,
 * reference layout); the BatchNorm tensors ("model.{3,6,9,12}.*") are not staged (CID_ERR_KEY) but passed at every forward as
 * bn[0..3], a cid_disc_bn each, with the eval / train semantics of cid_disc_forward.  cid_srd_upload_weights needs all fourteen
 * (CID_ERR_STATE otherwise) and waits for its copy.
 *
 * cid_srd_forward: arguments, formats, arithmetic, determinism and asynchrony as cid_disc_forward.  Layer 11 runs on the same exact-fp32
 * MFMA kernel as layers 5 and 8, as two 128-channel halves; the head (average pool, both 1x1 layers, sigmoid) accumulates in fp64
 * in a fixed order, one workgroup per image, so in eval mode an image's probability is bit-identical in any batch.  The argument
 * checks, their order and their codes are cid_disc_forward's (with four BatchNorms), all before any launch; train mode with
 * N*H4*W4 == 1 is CID_ERR_SHAPE ("Expected more than 1 value per channel when training").
 *
 * cid_srd_workspace_bytes(N, H, W, training), with a256(v) = v rounded up to a multiple of 256 and every tensor fp32:
 *     a256(4 * N * max(64*H*W, 128*H2*W2, 256*H4*W4))      region A: a0, then z5, then z11
 *   + a256(4 * N * max(64*H2*W2, 128*H4*W4))               region B: z2, then z8
 *   + a256(4 * 4 * 256 * 2)                                (scale, shift) pairs of the four BatchNorms
 *   + in train mode, for (Ho, Wo, TH, C) in (H2, W2, 16, 64), (H2, W2, 8, 128), (H4, W4, 8, 128), (H4, W4, 8, 256):
 *       a256(8 * C * 2 * N * ceil(Ho / TH) * ceil(Wo / 16))  fp64 per-tile partial sums of z and z^2
 *
 * cid_srd_losses: p_real = D(hr_img) and p_fake = D(fake_hr) (device fp32 [N]) -> device double out[2] = d_loss = BCE(p_real, 1) +
 * BCE(p_fake, 0), adv_loss = BCE(p_fake, 1), logs clamped at -100 as nn.BCELoss does (the BCE term of cid_disc_losses).  One workgroup,
 * fp64, fixed order.  CID_ERR_INVALID for a null or misaligned pointer, CID_ERR_SHAPE for N < 1.
 */
typedef struct cid_srd_s* cid_srd_t;
#define CID_SRD_NUM_WEIGHTS 14
int cid_srd_create(cid_srd_t* out);
void cid_srd_destroy(cid_srd_t d);
const char* cid_srd_last_error(cid_srd_t d);
int cid_srd_set_weight(cid_srd_t d, const char* key, const float* host_data, const int64_t* shape, int ndim);
size_t cid_srd_packed_weights_bytes(void);
int cid_srd_upload_weights(cid_srd_t d, void* device_blob, void* stream);
int cid_srd_workspace_bytes(int N, int H, int W, int training, size_t* bytes);
int cid_srd_forward(cid_srd_t d, const void* in, int in_fmt, float* out_prob, int N, int H, int W, const cid_disc_bn* bn,
                    int training, void* workspace, size_t workspace_bytes, void* stream);
int cid_srd_losses(const float* p_real, const float* p_fake, int N, double* out, void* stream);

/*
 * The SRGAN discriminator's backward pass (that trainer's d_loss.backward(), sr_ganTrainGNew.py:399, and the adversarial half of
 * g_loss.backward(), :408).  The family mirrors cid_disc_forward_saved / cid_disc_backward above: the same conventions for what is
 * null, what is overwritten, determinism (the same call twice gives the same bits; in eval mode an image's input gradient does not
 * depend on its batch), asynchrony, and the same argument checks in the same order with the same codes, with four BatchNorms and
 * seven convolutions.  Gradients of model.0 ... model.17 in fp32; every reduction accumulates in fp64 in a fixed order, no atomics;
 * the GEMMs of layers 2, 5, 8, 11 (data and weight gradient) run on the exact-fp32 MFMA.
 *
 * cid_srd_forward_saved is cid_srd_forward with a caller-owned PER-CALL buffer in place of the workspace.  It keeps, without overlap,
 * the activated a0, the raw z2, z5, z8, z11, each BatchNorm's (scale, shift) and (mean, invstd), per image the 256 pooled means of a12
 * and the 512 pre-activations of model.15 in fp64 (the backward's head never reads z11), and in train mode the statistics slabs.
 * Probabilities and BatchNorm buffer updates are bit-identical to cid_srd_forward.  cid_srd_saved_bytes(N, H, W, training), with
 * a256 as above:
 *     a256(4*N*64*H*W) + a256(4*N*64*H2*W2) + a256(4*N*128*H2*W2) + a256(4*N*128*H4*W4) + a256(4*N*256*H4*W4)      a0, z2, z5, z8, z11
 *   + a256(4 * 4*256*2) + a256(8 * 4*256*2)                 (scale, shift) in fp32 and (mean, invstd) in fp64 of the four BatchNorms
 *   + a256(8 * N*256) + a256(8 * N*512)                     pooled means, hidden pre-activations
 *   + in train mode the four slabs of cid_srd_workspace_bytes
 *
 * cid_srd_backward: arguments as cid_disc_backward; `g` holds w[i], b[i] for model.{0,2,5,8,11,15,17}, gamma[l], beta[l] for
 * model.{3,6,9,12} and input [N,3,H,W].  Every pointer may be null: only what is asked for is written, the chain stops at the lowest
 * stage asked for (head > BatchNorm 12 > model.11 > BatchNorm 9 > ... > model.0 > input), a uint8 input has no gradient.  The slope of
 * model.16's LeakyReLU is decided on the saved fp64 pre-activation, as the forward decides it.  Error codes as cid_disc_backward.
 *
 * cid_srd_pack_weights_device builds the forward's blob from the fourteen parameter tensors in DEVICE memory (order model.0.weight,
 * model.0.bias, model.2.weight, ... model.17.bias) with one kernel and attaches it: byte for byte what cid_srd_set_weight x 14 +
 * cid_srd_upload_weights produce, model.11's two 128-channel halves and the zero padding between segments included.
 *
 * cid_srd_saved_masks is a testing aid as cid_disc_saved_masks: the six LeakyReLU decisions as the backward takes them, uint8 (1 where
 * the slope is 1): masks[0] a0 [N,64,H,W], masks[1..4] the outputs of BatchNorm 3, 6, 9, 12 ([N,64,H2,W2], [N,128,H2,W2],
 * [N,128,H4,W4], [N,256,H4,W4]), masks[5] the hidden layer [N,512].
 */
typedef struct {
    float* w[7];         /* model.0, 2, 5, 8, 11, 15, 17 .weight */
    float* b[7];         /* model.0, 2, 5, 8, 11, 15, 17 .bias   */
    float* gamma[4];     /* model.3, 6, 9, 12 .weight            */
    float* beta[4];      /* model.3, 6, 9, 12 .bias              */
    float* input;        /* fp32 [N,3,H,W]                       */
} cid_srd_grads;
int cid_srd_saved_bytes(int N, int H, int W, int training, size_t* bytes);
int cid_srd_forward_saved(cid_srd_t d, const void* in, int in_fmt, float* out_prob, int N, int H, int W, const cid_disc_bn* bn,
                          int training, void* saved, size_t saved_bytes, void* stream);
int cid_srd_backward_workspace_bytes(int N, int H, int W, int training, size_t* bytes);
int cid_srd_backward(cid_srd_t d, const void* in, int in_fmt, const float* grad_prob, int N, int H, int W, const cid_disc_bn* bn,
                     int training, const void* saved, size_t saved_bytes, const cid_srd_grads* g, void* workspace,
                     size_t workspace_bytes, void* stream);
int cid_srd_pack_weights_device(cid_srd_t d, const float* const* dev_params, void* device_blob, void* stream);
int cid_srd_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int training, unsigned char* const* masks,
                        void* stream);

/*
 * The ESRGAN trainer's discriminator — Discriminator (backend/trainingcode/esrgan_code/models.py:36-71), which that trainer calls
 * three times per step (esrgan_train.py:104-119) for d_loss = 0.5 * (BCEWithLogits(D(clean), 1) + BCEWithLogits(D(denoised), 0)) and
 * g_loss = MSE(denoised, clean) + 1e-3 * BCEWithLogits(D(denoised), 1).  Its own handle and blob; the backward pass follows below.
 *
 *   conv1 Conv2d(3,64,3,s=2,p=1)  conv2 Conv2d(64,128,3,s=2,p=1)  conv3 Conv2d(128,256,3,s=2,p=1)  conv4 Conv2d(256,512,3,s=2,p=1),
 *   LeakyReLU(0.2) after each; then view(N,-1) and fc = Linear(512*H4*W4, 1).  The output is the LOGIT, one per image: no sigmoid.
 *   Layer sizes: H1 = (H-1)/2 + 1 (integer division), H2 = (H1-1)/2 + 1, H3, H4 likewise, and the same for W.
 *
 * The linear layer fixes the input size, so a handle is created for one (H, W): cid_esd_create(&d, H, W) with
 * 1 <= H, W <= CID_ESD_MAX_SIDE (CID_ERR_SHAPE otherwise; the bound keeps fc.weight, 512*H4*W4 floats, at 128 MiB and every
 * per-image pixel index within an int).  A uint8 input is decoded as ToTensor() does, u / 255 in [0,1] (the ESRGAN range, the
 * arithmetic of cid_esr_forward), so a uint8 batch and its fp32 copy give identical bits.
 *
 * cid_esd_set_weight takes the ten tensors by their state_dict keys "conv{1,2,3,4}.{weight,bias}" ([Cout,Cin,3,3] / [Cout]),
 * "fc.weight" ([1, 512*H4*W4] for the handle's input size, CID_ERR_SHAPE otherwise) and "fc.bias" ([1]), fp32 in the reference
 * layout; any other key is CID_ERR_KEY.  The packed blob of cid_esd_packed_weights_bytes(H, W) bytes (0 for a size cid_esd_create
 * refuses) holds, each segment 64-float aligned: conv1 as it came, weights then biases; conv2, conv3, conv4 as COUT/64 blocks, one
 * per 64-channel part, [CIN/8][9 taps][8][64] (element ((ci/8 * 9 + tap) * 8 + ci%8) * 64 + co%64 of block co/64) followed by the
 * part's 64 biases; fc.weight permuted from the reference's NCHW flatten (feature c*H4*W4 + y*W4 + x) into the activations' C8 order
 * (position ((c/8 * H4*W4 + y*W4 + x) * 8 + c%8); fc.bias.  cid_esd_upload_weights needs all ten (CID_ERR_STATE otherwise) and waits
 * for its copy.  cid_esd_export_packed copies the same bytes to host memory instead (CID_ERR_STATE while a tensor is missing,
 * CID_ERR_WORKSPACE for a buffer smaller than the blob), for transports that move the blob themselves and for tests of the layout.
 *
 * cid_esd_forward: `in` is device fp32 [N,3,H,W] (CID_FMT_F32_NCHW) or uint8 [N,H,W,3] (CID_FMT_U8_NHWC), out_logit device fp32 [N].
 * conv1 runs on the VALU, conv2 ... conv4 on the exact-fp32 MFMA with one accumulation chain per output element, the linear layer in
 * fp64 in a fixed order, one workgroup per image: an image's logit depends only on (H, W), never on N or on its position in the batch.
 * No atomics.  Asynchronous on `stream`; any N >= 1 (batches above 65,535 images run as several launches).  Checked before any launch,
 * in this order:
 *   CID_ERR_INVALID    null in / out_logit / workspace, unknown format, misaligned fp32 pointer
 *   CID_ERR_SHAPE      N < 1; H or W different from the handle's
 *   CID_ERR_WORKSPACE  workspace smaller than cid_esd_workspace_bytes or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_esd_workspace_bytes(N, H, W), with a256(v) = v rounded up to a multiple of 256: the four ACTIVATED tensors a1 ... a4 (fp32, the
 * C8 layout of cid_disc_forward, LeakyReLU applied) in four distinct regions, which is what a backward pass needs of the forward:
 *     a1 at 0                          4 * N *  64 * H1 * W1 bytes
 *     a2 at a256(|a1|)                 4 * N * 128 * H2 * W2
 *     a3 at a256(|a1|) + a256(|a2|)    4 * N * 256 * H3 * W3
 *     a4 at ... + a256(|a3|)           4 * N * 512 * H4 * W4;        total = a256(|a1|) + a256(|a2|) + a256(|a3|) + a256(|a4|)
 *
 * cid_esd_losses: logit_real = D(clean), logit_fake = D(denoised) (device fp32 [N]) -> device double out3[3] = the means over the
 * batch of BCEWithLogits(real, 1), BCEWithLogits(fake, 0), BCEWithLogits(fake, 1), each term max(x,0) - x*y + log1p(exp(-|x|)) in
 * fp64, one workgroup, fixed order: d_loss = 0.5 * (out3[0] + out3[1]), gan_loss = out3[2].  cid_esd_trainer_losses adds the pixel
 * loss over denoised / clean (fp32 [N,3,H,W] or uint8 [N,H,W,3] read as u / 255; the reduction of cid_disc_losses) and forms the
 * trainer's sums on the device: out4[4] = d_loss, gan_loss, pixel_loss = MSE(denoised, clean), g_loss = pixel_loss + 1e-3 * gan_loss
 * (a rounded product, then a rounded sum).  Both: CID_ERR_INVALID for a null or misaligned pointer or an unknown format,
 * CID_ERR_SHAPE for N < 1 (or H, W outside 1 ... CID_ESD_MAX_SIDE).
 */
typedef struct cid_esd_s* cid_esd_t;
#define CID_ESD_NUM_WEIGHTS 10
#define CID_ESD_MAX_SIDE 4096
int cid_esd_create(cid_esd_t* out, int H, int W);
void cid_esd_destroy(cid_esd_t d);
const char* cid_esd_last_error(cid_esd_t d);
int cid_esd_set_weight(cid_esd_t d, const char* key, const float* host_data, const int64_t* shape, int ndim);
size_t cid_esd_packed_weights_bytes(int H, int W);
int cid_esd_upload_weights(cid_esd_t d, void* device_blob, void* stream);
int cid_esd_export_packed(cid_esd_t d, void* host_dst, size_t bytes);
int cid_esd_workspace_bytes(int N, int H, int W, size_t* bytes);
int cid_esd_forward(cid_esd_t d, const void* in, int in_fmt, float* out_logit, int N, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream);
int cid_esd_losses(const float* logit_real, const float* logit_fake, int N, double* out3, void* stream);
int cid_esd_trainer_losses(const float* logit_real, const float* logit_fake, const void* denoised, int d_fmt, const void* clean,
                           int c_fmt, int N, int H, int W, double* out4, void* stream);

/*
 * The ESRGAN discriminator's backward pass (that trainer's d_loss.backward(), esrgan_train.py:107, and the adversarial half of
 * g_loss.backward(), :119).  The family mirrors cid_srd_forward_saved / cid_srd_backward above where the model allows it: there is no
 * BatchNorm, so no `bn`, no `training` and no masks entry; the LeakyReLU decisions are a_l > 0 on the saved activated tensors.
 * Gradients of conv1 ... conv4 and fc in fp32; every reduction across workgroups accumulates in fp64 in a fixed order, no atomics; the
 * GEMMs of conv2, conv3, conv4 (data and weight gradient) run on the exact-fp32 MFMA, conv1 on the VALU.  The same call twice gives
 * the same bits; an image's input gradient depends only on its grad_logit value and (H, W), never on N or its place in the batch.
 *
 * cid_esd_saved_bytes(N, H, W) is the formula of cid_esd_workspace_bytes, and returns its codes: a1 ... a4 at the offsets listed
 * there, each rounded up to 256 bytes.  cid_esd_forward_saved is cid_esd_forward with a caller-owned PER-CALL buffer in place of the
 * workspace: the same launches, the same argument checks in the same order with the same codes (a saved buffer that is too small or
 * not 256-byte aligned is CID_ERR_WORKSPACE), and logits and the four saved tensors byte-identical to cid_esd_forward.
 *
 * cid_esd_backward: `in`, in_fmt, N, H, W and `saved` are those of the cid_esd_forward_saved call to differentiate, grad_logit the
 * device fp32 [N] gradient of the loss with respect to the logits; the packed weights must still be the ones that call used.  `g`
 * holds device fp32 pointers in the order conv1, conv2, conv3, conv4, fc and the reference layouts: w [Cout,Cin,3,3] and b [Cout] for
 * the convolutions, w[4] = fc.weight [1, 512*H4*W4] in the reference's NCHW-flatten order (not C8), b[4] = fc.bias [1], and input
 * [N,3,H,W].  Results OVERWRITE their outputs.  A null pointer skips that output and the work only it needs: the chain runs fc >
 * conv4 > conv3 > conv2 > conv1 > input and stops at the deepest stage asked for; without g->input there is no conv1 data gradient.
 * A uint8 input has no gradient.  Asynchronous on `stream`, no host synchronisation; any N >= 1.  Checked before any launch, in this
 * order:
 *   CID_ERR_INVALID    null in / grad_logit / saved / g / workspace, unknown format, misaligned fp32 operand or gradient pointer,
 *                      g->input with a uint8 input
 *   CID_ERR_SHAPE      N < 1; H or W different from the handle's (the forward's message)
 *   CID_ERR_WORKSPACE  saved buffer smaller than cid_esd_saved_bytes, workspace smaller than cid_esd_backward_workspace_bytes, or
 *                      either not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_esd_backward_workspace_bytes(N, H, W), with a256 as above, T(l) = ceil(H_l / 4) * ceil(W_l / 16) the weight-gradient items per
 * image of conv l and S(l) = min(N * T(l), max(s_l, ceil(N * T(l) / 2048))) its splits, s_2 = 64, s_3 = 16, s_4 = 2 (a workgroup adds at
 * most 2,048 items into its fp32 accumulators):
 *     a256(4*N*64*H1*W1) + a256(4*N*128*H2*W2) + a256(4*N*256*H3*W3)                      gradients of a1, a2, a3
 *   + a256(4 * 9 * max(S(2)*128*64, S(3)*256*128, S(4)*512*256))                          fp32 weight-gradient partials
 *   + a256(8 * max(S(2)*128, S(3)*256, S(4)*512))                                         fp64 bias-gradient partials
 *   + a256(8 * 64*28 * min(N * ceil(H1*W1 / 64), 256))                                    fp64 partials of conv1
 *
 * cid_esd_pack_weights_device builds the forward's blob from the ten parameter tensors in DEVICE memory (state_dict order:
 * conv1.weight, conv1.bias, ... conv4.bias, fc.weight, fc.bias) with one kernel and attaches it: byte for byte what
 * cid_esd_export_packed hands out after cid_esd_set_weight x 10, the C8 permutation of fc.weight, the zero padding that aligns every
 * segment to 64 floats and fc.bias's own segment included.  CID_ERR_INVALID for a null or misaligned pointer, CID_ERR_WORKSPACE for
 * a blob that is not 256-byte aligned.
 */
typedef struct {
    float* w[5];         /* conv1, conv2, conv3, conv4, fc .weight */
    float* b[5];         /* conv1, conv2, conv3, conv4, fc .bias   */
    float* input;        /* fp32 [N,3,H,W]                         */
} cid_esd_grads;
int cid_esd_saved_bytes(int N, int H, int W, size_t* bytes);
int cid_esd_forward_saved(cid_esd_t d, const void* in, int in_fmt, float* out_logit, int N, int H, int W, void* saved,
                          size_t saved_bytes, void* stream);
int cid_esd_backward_workspace_bytes(int N, int H, int W, size_t* bytes);
int cid_esd_backward(cid_esd_t d, const void* in, int in_fmt, const float* grad_logit, int N, int H, int W, const void* saved,
                     size_t saved_bytes, const cid_esd_grads* g, void* workspace, size_t workspace_bytes, void* stream);
int cid_esd_pack_weights_device(cid_esd_t d, const float* const* dev_params, void* device_blob, void* stream);

/*
 * The generator's backward pass — g_loss.backward() through DenoiseGenerator in the trainer's generator step
 * (backend/trainingcode/denoise_gan_code/training.py:420-426; the module itself :59-74).  fp32 NCHW in and out, CID_DTYPE_F32 only.
 *
 * cid_forward_saved is cid_forward with a caller-owned PER-CALL buffer of cid_saved_bytes(N, H, W) bytes (= cid_workspace_bytes, 256-byte
 * aligned) in place of the arena; it has the arena's layout, so cid_stage_view applies to it, "upconv1.0" included: the last layer
 * always runs as CID_TAIL_TILES here (the fused form never stores upconv1.0, which the backward pass reads), whatever the handle's
 * tail algorithm, and the handle is not changed.  The 3x3 layers run under the handle's conv algorithm.  H and W must be multiples
 * of 4 (CID_ERR_SHAPE otherwise): for other sizes the skip tensors are stored only over the crop the concat keeps, so the max-pool
 * routing outside it cannot be recovered.  cid_forward keeps accepting every size.  CID_DTYPE_F16 -> CID_ERR_STATE.
 *
 * cid_backward: `in`, N, H, W and `saved` are those of the cid_forward_saved call to differentiate, `out` its output y and grad_out
 * the gradient of the loss with respect to y (both fp32 [N,3,H,W]); the packed weights must still be the ones that call used.
 * `grads` holds device fp32 pointers for the results in kLayers order (cid_param_key(2 l) / (2 l + 1): down1.0, down1.2, down2.0,
 * down2.2, bottleneck.0, bottleneck.2, up2, upconv2.0, upconv2.2, up1, upconv1.0, upconv1.2) and reference layouts: Conv2d weights
 * [Cout,Cin,3,3], the two ConvTranspose2d weights [Cin,Cout,2,2], biases [Cout], input [N,3,H,W].  A null pointer skips that output
 * and the work only it needs (no weight-gradient launch for a layer with neither pointer, nothing below the deepest layer asked
 * for); a gradient's bits do not depend on which others were asked for.  Results OVERWRITE; accumulation is the caller's
 * (autograd's) job.  `saved` is only read; the gradients of the activations live in `workspace`
 * (cid_backward_workspace_bytes(N, H, W), 256-byte aligned).  Asynchronous on `stream`, no host synchronisation.
 *
 * What is computed is the reference graph: dz of the last layer = grad_out * (1 - y^2); a 3x3 convolution's data gradient is the full
 * correlation with flipped taps and zero padding, its weight gradient the contraction over N*H*W; ReLU's mask is a > 0 of the stored
 * activation; the concat's gradient slices go to the transposed convolution and the skip; max-pool routes the gradient to the first
 * element in window scan order (0,0), (0,1), (1,0), (1,1) equal to the pooled value (ATen's rule).  Matrix work runs on the exact-fp32
 * MFMA; every sum over pixels or images (bias gradients, the partial weight-gradient tiles, the two K = 27 layers) accumulates in fp64
 * in a fixed order, no atomics: the same call twice gives the same bits.  Every argument is checked before any launch, in this order:
 *   CID_ERR_INVALID    null handle / in / out / grad_out / saved / grads / workspace, misaligned fp32 pointer
 *   CID_ERR_STATE      compute dtype CID_DTYPE_F16
 *   CID_ERR_SHAPE      as cid_forward, or H or W not a multiple of 4
 *   CID_ERR_WORKSPACE  saved buffer or workspace too small or not 256-byte aligned
 *   CID_ERR_STATE      no weights attached
 */
typedef struct {
    float* w[12];        /* weight gradients, kLayers order, reference shapes */
    float* b[12];        /* bias gradients                                    */
    float* input;        /* fp32 [N,3,H,W]                                    */
} cid_grads;
int cid_saved_bytes(int N, int H, int W, size_t* bytes);
int cid_forward_saved(cid_handle_t h, const float* in, float* out, int N, int H, int W, void* saved, size_t saved_bytes, void* stream);
int cid_backward_workspace_bytes(int N, int H, int W, size_t* bytes);
int cid_backward(cid_handle_t h, const float* in, const float* out, const float* grad_out, int N, int H, int W, const void* saved,
                 size_t saved_bytes, const cid_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The trainer's optimizer step — g_optimizer.step() / d_optimizer.step() of training.py:239-240, 417, 426: torch.optim.Adam with default
 * flags — for up to CID_ADAM_MAX_TENSORS fp32 tensors in ONE kernel on `stream`.  No handle (as cid_quality); asynchronous, no host
 * synchronisation, no memcpy, no allocation.  `tensors[i]` names one parameter in DEVICE memory: param, exp_avg and exp_avg_sq are
 * updated in place (`count` contiguous elements each, every element written exactly once), grad is only read; each pointer at least
 * 4-byte aligned.  `step` is that tensor's step number INCLUDING this update (>= 1; torch counts steps per parameter, so the tensors of
 * one call may differ).  count == 0 is a no-op entry; a tensor that is not to be updated is left out of the table.  After the call a
 * generator or discriminator handle needs cid_pack_weights_device / cid_disc_pack_weights_device before its next forward.
 *
 * Per element, in double from the fp32 operands, without contraction, each stored value rounded once (round-to-nearest-even):
 *   g  = (double)grad                      ; if weight_decay != 0:  g = g + weight_decay * (double)p        (L2, not decoupled)
 *   m' = (float)( (double)m * beta1 + (1 - beta1) * g )
 *   v' = (float)( (double)v * beta2 + ((1 - beta2) * g) * g )
 *   bc1 = 1 - beta1^t,  bc2 = 1 - beta2^t                  (host, double, pow(); t = the tensor's `step`)
 *   p' = (float)( (double)p - (lr / bc1) * ( (double)m' / ( sqrt((double)v') / sqrt(bc2) + eps ) ) )
 * with 1 - beta1, 1 - beta2, lr / bc1 and sqrt(bc2) formed once on the host in double.  m' and v' need only IEEE multiply and add, so
 * they are the same bits wherever the tree is evaluated; p' goes through a double sqrt and two double divisions.  A tensor's results
 * do not depend on which other tensors share the call or on its place in the table.
 * Outside the tree: amsgrad, maximize, decoupled weight decay (AdamW), tensors that are not fp32, capture-time step counters.
 * Every argument error is found before anything is launched, in this order:
 *   CID_ERR_INVALID    null tensors or hp; ntensors outside 1..CID_ADAM_MAX_TENSORS; a null or not 4-byte-aligned pointer in an entry
 *                      with count > 0; count < 0 (or beyond 2^44) or step < 1; a hyper-parameter that is not finite or out of range
 *                      (lr < 0, a beta outside [0, 1), eps < 0, weight_decay < 0); any two of the written ranges (param, exp_avg,
 *                      exp_avg_sq over all entries) overlapping each other or a grad range
 *   CID_ERR_HIP        launch failure
 */
typedef struct { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t count; int64_t step; } cid_adam_tensor;
typedef struct { double lr, beta1, beta2, eps, weight_decay; } cid_adam_hyper;
#define CID_ADAM_MAX_TENSORS 32
int cid_adam_step(const cid_adam_tensor* tensors, int ntensors, const cid_adam_hyper* hp, void* stream);

/*
 * Bicubic resize — PIL's Image.resize(image_size, resample=BICUBIC) on uint8 RGB, the first step of every reference entry point
 * (noise_generation.py:61, denoisegan_eval.py, denoise_eavl_iter.py:89, training.py:303-304), on device batches and bit for bit:
 * Pillow's 8-bit resampler is integer arithmetic (22-bit fixed-point coefficients, a uint8 intermediate between its two passes).
 * The bit-defined restatement is synth.resize_bicubic_np (tables: synth.resize_tables_np).  No generator handle: no weights.
 *
 * Tables of one axis, from inS to outS samples, in double precision without FMA contraction, casts truncating:
 *   scale = inS / outS;  fs = max(scale, 1.0);  support = 2.0 * fs;  ksize = (int)ceil(support) * 2 + 1
 *   for xx in 0 .. outS-1:
 *     center = (xx + 0.5) * scale
 *     xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), inS);  n = xmax - xmin
 *     w[x] = cubic((x + xmin - center + 0.5) * (1.0 / fs)),  x = 0 .. n-1
 *     ww = w[0] + w[1] + ... (in that order);  if ww != 0: w[x] = w[x] / ww
 *     k[x] = (int)(w[x] < 0 ? -0.5 + w[x] * 4194304.0 : 0.5 + w[x] * 4194304.0)        (22 bits; k[x] = 0 for n <= x < ksize)
 *     bounds[xx] = (xmin, n)
 *   cubic(t): a = -0.5; t = |t|;  t < 1: ((a + 2) * t - (a + 3)) * t * t + 1;  t < 2: (((t - 5) * t + 8) * t - 4) * a;  else 0
 * One pass over an axis, per channel, in int32 (no overflow: a row's absolute coefficients sum to under 1.4 * 2^22, data <= 255):
 *   out = clamp((2^21 + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)                                     (arithmetic shift)
 * The horizontal pass runs first, if Ws != Wd, into a uint8 intermediate of Hs x Wd; the vertical pass second, if Hs != Hd.  A pass
 * whose axis keeps its size is skipped (not run with identity coefficients); with neither the result is a copy.  The rounding of
 * the intermediate to uint8 is part of the definition.
 *
 * cid_resize_plan_create builds both axes' tables on the host, uploads them into device memory the plan owns (on the current
 * device) and chooses the launch geometry; it may synchronise, and is the only resize call that may.  On a machine without a GPU
 * the plan is created with its host tables only: cid_resize_plan_table works, cid_resize returns CID_ERR_STATE.
 *   CID_ERR_INVALID  null `out`, a filter other than CID_RESAMPLE_BICUBIC
 *   CID_ERR_SHAPE    a side below 1 or above 16384; Hs*Ws*3 or Hd*Wd*3 >= 2^31; a downscale factor inS/outS above 64 on either axis
 *                    (ksize at most 257: a tile's band of intermediate rows always fits in LDS).  Upscaling is unbounded within the
 *                    side limit (ksize 5).
 * cid_resize_plan_table reads a table back from the plan's host copy (no GPU involved): axis 0 is vertical, 1 horizontal; bounds
 * holds [out*2] ints (xmin, n), coeffs [out*ksize] ints; either may be NULL to query ksize only.  CID_ERR_INVALID for a null plan or
 * ksize or an unknown axis.
 * cid_resize: src is device uint8 [N,Hs,Ws,3]; dst is CID_FMT_U8_NHWC [N,Hd,Wd,3] or CID_FMT_F32_NCHW [N,3,Hd,Wd], the latter as
 * (u/255.0f - 0.5f)/0.5f with true divisions — the forward's uint8 input arithmetic, so the float result fed to cid_forward gives
 * the bits of the uint8 result fed to cid_forward_ex(CID_FMT_U8_NHWC).  One kernel on `stream` (hipStream_t, NULL = default
 * stream), asynchronous, no host synchronisation; the intermediate lives in LDS.  dst must not overlap src.  Offsets are 64-bit:
 * N*Hs*Ws*3 may exceed 2^31.  Checked on the host before the launch:
 *   CID_ERR_INVALID  null plan, src or dst; unknown format; an fp32 dst that is not 4-byte aligned; N < 1
 *   CID_ERR_STATE    a plan created without a GPU
 * Known departure of Pillow itself from this definition (outside the 64x limit): for a 7-pixel-wide source downscaled 200x or more
 * in height and upscaled in width (800x7, 900x7, 1000x7 -> 4x16), Pillow 12.2's bytes equal a vertical-first evaluation.
 */
typedef struct cid_resize_plan_s* cid_resize_plan_t;
enum { CID_RESAMPLE_BICUBIC = 3 };                      /* Pillow's number for the filter */
int cid_resize_plan_create(cid_resize_plan_t* out, int Hs, int Ws, int Hd, int Wd, int filter);
void cid_resize_plan_destroy(cid_resize_plan_t p);
int cid_resize_plan_table(cid_resize_plan_t p, int axis, int* ksize, int* bounds, int* coeffs);
int cid_resize(cid_resize_plan_t p, const void* src_u8_nhwc, void* dst, int dst_fmt, int N, void* stream);

/*
 * The server's second model — ESRGANGenerator(num_residuals = 8) (backend/app.py:188-218; the same class in
 * backend/trainingcode/esrgan_code/models.py:6-34), the "esrgan" branch of /enhance (app.py:387-397).  Eval mode, fp32:
 *
 *   x1  = PReLU(Conv2d(3, 64, 9, padding=4)(x))                                         initial.0, initial.1 (one slope)
 *   x  <- x + BatchNorm(Conv3x3(PReLU(BatchNorm(Conv3x3(x)))))   R times, from x1        residuals.i.block.{0,1,2,3,4}
 *   out = Conv2d(64, 3, 9, padding=4)(x1 + x2)                                           final; no tanh, no clamp
 *
 * Its own handle and blob, as the discriminator has.  cid_esr_create fixes R = num_residuals (0 <= R <= CID_ESR_MAX_RESIDUALS,
 * CID_ERR_INVALID otherwise); with R = 0 the reference's empty nn.Sequential is the identity and out = final(x1 + x1).
 * cid_esr_param_key(h, i) enumerates the module's state_dict keys in its order (5 + 15 R of them, BatchNorm buffers and
 * num_batches_tracked included; NULL past the end).  cid_esr_set_weight takes each of them as host fp32 in the reference layout
 * (Conv2d [Cout,Cin,k,k]; bias, BatchNorm weight / bias / running_mean / running_var [C]; a PReLU slope [1]); a num_batches_tracked
 * key (ndim 0) is accepted and ignored.  Unknown key -> CID_ERR_KEY, wrong shape -> CID_ERR_SHAPE.  cid_esr_set_bn_eps gives the eps
 * of BatchNorm `which` (0: block.1, 1: block.4) of residual block `block` (default 1e-5, nn.BatchNorm2d's).
 * cid_esr_missing_weights counts the tensors still unset (num_batches_tracked never counts).  cid_esr_upload_weights packs the
 * blob (cid_esr_packed_weights_bytes(h), 256-byte aligned, caller-owned device memory), copies it and attaches it; it needs every
 * tensor (CID_ERR_STATE otherwise) and waits for its copy, as cid_disc_upload_weights does.  Each BatchNorm is folded there into
 * y = fmaf(s, z, t) with s = gamma / sqrt(running_var + eps) and t = beta - running_mean * s, derived in fp64 and rounded once to
 * fp32 (train-mode BatchNorm: cid_esr_forward_train, below).  PReLU is v > 0 ? v : a * v for any slope a.
 *
 * cid_esr_forward: in is fp32 [N,3,H,W] in [0,1] (CID_FMT_F32_NCHW; the server feeds ToTensor() alone) or uint8 [N,H,W,3]
 * (CID_FMT_U8_NHWC), read as (float)u / 255.0f with a true division: a uint8 image and its /255 fp32 copy give identical bits.
 * out is the raw fp32 [N,3,H,W], or uint8 [N,H,W,3] as the server's clamp(0,1) -> ToPILImage view (app.py:251-254):
 * (uint8)(clamp(v, 0, 1) * 255.0f), a truncation.  Any H, W >= 1.  1 + 2 R + 1 launches on `stream` (hipStream_t, NULL = default
 * stream), no host synchronisation; the trunk runs on exact-fp32 MFMA, head and tail on the VALU.  Every sum has a fixed order and
 * an image's tiles depend only on (H, W): an image's result is bit-identical in any batch.  Checked on the host before any launch:
 *   CID_ERR_INVALID    null pointer, unknown format, misaligned fp32 operand
 *   CID_ERR_SHAPE      N < 1, H < 1, W < 1, H*W >= 2^31
 *   CID_ERR_WORKSPACE  workspace smaller than cid_esr_workspace_bytes(N, H, W) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_esr_stage_view (testing aid): where the last forward of an [N,3,H,W] input left `stage` in its workspace: "x1", or "tail_in",
 * the tensor the last launch read (x1 + x2).  Both are fp32 with C channels in blocks of *channel_block = 8: element (n, c, y, x) is
 * at (((n * (C/8) + c/8) * Hs + y) * Ws + x) * 8 + c % 8 floats past offset_bytes.  Unknown stage -> CID_ERR_KEY.
 */
typedef struct cid_esr_s* cid_esr_t;
#define CID_ESR_MAX_RESIDUALS 16
int cid_esr_create(cid_esr_t* out, int num_residuals);
void cid_esr_destroy(cid_esr_t h);
const char* cid_esr_last_error(cid_esr_t h);
const char* cid_esr_param_key(cid_esr_t h, int i);
int cid_esr_set_weight(cid_esr_t h, const char* key, const void* host_data, const int64_t* shape, int ndim);
int cid_esr_set_bn_eps(cid_esr_t h, int block, int which, double eps);
int cid_esr_missing_weights(cid_esr_t h, int* count);
size_t cid_esr_packed_weights_bytes(cid_esr_t h);
int cid_esr_upload_weights(cid_esr_t h, void* device_blob, void* stream);
int cid_esr_workspace_bytes(int N, int H, int W, size_t* bytes);
int cid_esr_forward(cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream);
int cid_esr_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block);

/*
 * The same generator in TRAIN mode: the first line of the ESRGAN trainer's step, denoised = G(noisy) after G.train()
 * (backend/trainingcode/esrgan_code/esrgan_train.py:89-121).  Forward only; the output carries no gradient.
 *
 * cid_esr_forward_train is cid_esr_forward with the 2 R BatchNorms on the statistics of THIS batch.  bn[0 .. 2R-1] describe
 * residuals.0.block.1, residuals.0.block.4, residuals.1.block.1, ..., a cid_disc_bn each, with the semantics of cid_sr_forward_train:
 * device pointers, eps and momentum as the containers hold them (CID_DISC_MOMENTUM_NONE for momentum=None), normalisation with the
 * batch mean and the BIASED batch variance over N*H*W values per channel, running = (1 - m) * running + m * batch_stat with the
 * UNBIASED variance for running_var, num_batches_tracked += 1, all on the device without host synchronisation.  Convolution weights,
 * biases and PReLU slopes come from the blob cid_esr_upload_weights made; its folded (s, t) are not read and the blob is not changed,
 * so upload again before the next cid_esr_forward.  in, out, in_fmt and out_fmt are cid_esr_forward's; the output is the raw sum.
 *
 * A block's output is r_i = r_{i-1} + BN_{2i+1}(z_{2i+1}) (r_{-1} = x1), and BN_{2i+1}'s statistics exist only after the convolution
 * that makes z_{2i+1} has run over the whole batch.  So the next block's first convolution forms r_i = res + fmaf(scale, z, shift)
 * (eval's expression and association) while it stages its input, and the tile that owns a pixel stores it: each element of r_i is
 * written once, and the block outputs alternate between two tensors, apart from x1.  The tail's input
 * x1 + (r_{R-2} + BN_{2R-1}(z_{2R-1})) is an elementwise launch.  Launches for R >= 1 (4 R + 4): head, 2 R x (convolution,
 * statistics), one counter launch, the sum, tail.  Each convolution stores its raw z and per-tile fp64 sums of z and z^2 (one slab row
 * per tile); the statistics launch reduces them in a fixed order.  No atomics: the same call on the same buffers gives the same bits.
 * With R = 0 there is no BatchNorm: the call is cid_esr_forward's two launches on this workspace, bn may be NULL and N*H*W == 1 is
 * accepted.  Checked on the host before any launch (a refused call updates nothing):
 *   CID_ERR_INVALID    null pointer (any of bn[l]'s five included), unknown format, misaligned fp32 operand, an eps or momentum that
 *                      is not finite or negative (other than CID_DISC_MOMENTUM_NONE)
 *   CID_ERR_SHAPE      N < 1, H < 1, W < 1, H*W >= 2^31; with R > 0, N*H*W == 1 ("Expected more than 1 value per channel when training")
 *   CID_ERR_WORKSPACE  workspace smaller than cid_esr_train_workspace_bytes(N, H, W, R) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_esr_train_workspace_bytes: with a(v) = v rounded up to 256, t = N * 64 * H * W * 4 and tiles = ceil(H/16) * ceil(W/16),
 *   5 a(t)                                 x1, the two raw z tensors the convolutions alternate between, the two tensors the block
 *                                          outputs and the tail's input alternate between
 *   + a(64 * 2 * N * tiles * 8)            the slab (reused by all 2 R convolutions)
 *   + 2 R * a(64 * 2 * 4)                  one (scale, shift) table per BatchNorm, each kept
 * (num_residuals outside [0, CID_ESR_MAX_RESIDUALS] -> CID_ERR_INVALID).  cid_esr_train_stage_view is cid_esr_stage_view for that
 * workspace: "x1" and "tail_in".
 */
int cid_esr_train_workspace_bytes(int N, int H, int W, int num_residuals, size_t* bytes);
int cid_esr_forward_train(cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, const cid_disc_bn* bn,
                          void* workspace, size_t workspace_bytes, void* stream);
int cid_esr_train_stage_view(const char* stage, int N, int H, int W, int num_residuals, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                             int* channel_block);

/*
 * The backward pass of that train-mode generator: g_loss.backward() of the ESRGAN trainer's step (esrgan_train.py:115-121) from
 * grad_out = d loss / d denoised down to every parameter.  The family mirrors cid_sr_forward_saved / cid_sr_backward (below): per-call
 * saved buffer, what is null is not written and costs no launch of its own, the same call twice gives the same bits, no host
 * synchronisation.  There is no input gradient: noisy is data.  With R = 0 there is no BatchNorm and bn may be NULL.
 *
 * cid_esr_forward_saved is cid_esr_forward_train with an fp32 output and a caller-owned PER-CALL saved buffer next to the workspace
 * (cid_esr_train_workspace_bytes; x1 and the slab stay there: the backward forms x1 from v0).  out and the BatchNorm buffer updates are
 * bit-identical to cid_esr_forward_train.  The saved buffer keeps, without overlap: the head's sums v0 before its PReLU, the 2 R raw
 * z_l, the block outputs r_0 .. r_{R-2}, tail_in, and the 2 R (scale, shift) and (mean, invstd) tables.  Every PReLU mask of the
 * backward is decided on a saved PRE-activation (v0, or BN_2i(z_2i) recomputed with the forward's own fmaf), so it is the forward's
 * decision for any slope, 0 and negative ones included.
 * cid_esr_saved_bytes(N, H, W, R), with a(v) = v rounded up to 256 and t = N * 64 * H * W * 4:
 *     (R >= 1 ? 3 R + 1 : 2) a(t) + a(2R*64*2*4) + a(2R*64*2*8)
 *
 * cid_esr_backward: `in` is the forward's input (the head's weight gradient reads it, fp32 or uint8 as the forward reads it), grad_out
 * fp32 [N,3,H,W] (the output is the raw sum, so it is taken as it is), bn the forward's array (only gamma is read).  `g` holds one
 * pointer per parameter tensor in the module's layouts; a null pointer means the tensor is not wanted.  With r_{-1} = x1 and G_i the
 * gradient of r_i: final gives dT = d tail_in; the outer skip gives G_{R-1} = dT; block i gives BN_{2i+1}'s and convolution 2i+1's
 * gradients from G_i, then BN_2i's, the block's slope's and convolution 2i's, and G_{i-1} = G_i + (convolution 2i's data gradient),
 * added in that order; d x1 = G_{-1} + dT in that order (R = 0: dT + dT); then the head.  BatchNorm's backward carries the two batch
 * sums, dz = k * (g - m1 - xh * m2); the 3x3 data and weight gradients and final's run on the exact-fp32 MFMA, a weight gradient
 * accumulating in fp32 inside one workgroup's range of tiles; the head's K = 243 weight gradient runs in fp64 on the VALU; every
 * reduction across workgroups is fp64 in a fixed order through a slab (or per-workgroup partials) and a reduce launch, no atomics.
 * The workspace may hold anything on entry.  cid_esr_backward_workspace_bytes(N, H, W, R), with strips = ceil(H*W / 512):
 *     (R >= 1 ? 4 : 2) a(t) + a(64*8*4) + a(64*3*N*strips*8) + a(64*8) + a(128*4*64*144*4) + a(128*64*8) + a(512*64*244*8)
 * Checked on the host before any launch:
 *   CID_ERR_INVALID    null h / in / grad_out / saved / g / workspace, with R > 0 null bn / bn[l].gamma, unknown format, misaligned
 *                      fp32 pointer (the gradient tensors included)
 *   CID_ERR_SHAPE      as cid_esr_forward_train
 *   CID_ERR_WORKSPACE  saved buffer or workspace too small or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_esr_pack_weights_device builds the forward's blob from the parameter tensors in DEVICE memory with one launch and attaches it:
 * byte for byte what cid_esr_set_weight + cid_esr_set_bn_eps + cid_esr_upload_weights produce, the zero gaps and the 2 R eval-mode
 * folds (taken in fp64 from bn[l]'s gamma, beta, running_mean, running_var and eps, rounded as the host rounds them) included.
 * dev_params holds the 3 + 9 R + 2 parameter tensors in the module's order: initial.0.weight, initial.0.bias, initial.1.weight, per
 * block block.0.weight block.0.bias block.1.weight block.1.bias block.2.weight block.3.weight block.3.bias block.4.weight block.4.bias,
 * final.weight, final.bias.  A trainer calls it after every optimizer step.
 *   CID_ERR_INVALID    null h / dev_params / device_blob, a null or not 4-byte-aligned parameter pointer, with R > 0 a null bn, gamma,
 *                      beta, running_mean or running_var, an eps that is not finite or negative
 *   CID_ERR_WORKSPACE  device_blob not 256-byte aligned
 *
 * cid_esr_saved_masks is a testing aid as cid_sr_saved_masks: the 1 + R PReLU decisions as the backward takes them, uint8 [N,64,H,W]
 * (1 where the slope is 1): masks[0] the head, masks[1 + i] block i's PReLU (after residuals.i.block.1).
 */
typedef struct {
    float* head_w;        /* initial.0.weight [64,3,9,9]                                          */
    float* head_b;        /* initial.0.bias [64]                                                  */
    float* head_slope;    /* initial.1.weight [1]                                                 */
    float* conv_w[32];    /* residuals.i.block.0.weight (2i), residuals.i.block.3.weight (2i+1)   */
    float* conv_b[32];    /* their biases                                                         */
    float* gamma[32];     /* residuals.i.block.1.weight (2i), residuals.i.block.4.weight (2i+1)   */
    float* beta[32];      /* their biases                                                         */
    float* slope[16];     /* residuals.i.block.2.weight [1]                                       */
    float* final_w;       /* final.weight [3,64,9,9]                                              */
    float* final_b;       /* final.bias [3]                                                       */
} cid_esr_grads;
int cid_esr_saved_bytes(int N, int H, int W, int num_residuals, size_t* bytes);
int cid_esr_forward_saved(cid_esr_t h, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, void* saved,
                          size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int cid_esr_backward_workspace_bytes(int N, int H, int W, int num_residuals, size_t* bytes);
int cid_esr_backward(cid_esr_t h, const void* in, int in_fmt, const float* grad_out, int N, int H, int W, const cid_disc_bn* bn,
                     const void* saved, size_t saved_bytes, const cid_esr_grads* g, void* workspace, size_t workspace_bytes, void* stream);
int cid_esr_pack_weights_device(cid_esr_t h, const float* const* dev_params, const cid_disc_bn* bn, void* device_blob, void* stream);
int cid_esr_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int num_residuals, unsigned char* const* masks,
                        void* stream);

/*
 * The server's third model — SRGANGenerator(scale_factor = 4) (backend/app.py:145-186; the same class in
 * backend/trainingcode/srgan_code/sr_ganTrainGNew.py:19-51), the "srgan" branch of /enhance.  Eval mode, fp32:
 *
 *   x0  = PReLU(Conv2d(3, 64, 9, padding=4)(x))                                          initial.0, initial.1
 *   r   = five times  b <- BatchNorm(Conv3x3(PReLU(BatchNorm(Conv3x3(b))))), from x0      res_blocks.i.{0,1,2,3,4}; NO skip per block
 *   t   = Conv3x3(r) + x0                                                                mid (bias, no BatchNorm)
 *   u  <- PReLU(PixelShuffle(2)(Conv2d(64, 256, 3, padding=1)(u)))  log2(scale) times     upscale.{3k, 3k+2}, from t
 *   out = tanh(Conv2d(64, 3, 9, padding=4)(u))                                           final
 *
 * PixelShuffle(2) is out[n, c, 2y+i, 2x+j] = in[n, 4c + 2i + j, y, x].  Its own handle and blob, mirroring cid_esr_* one for one.
 * cid_sr_create fixes scale_factor = 1, 2, 4 or 8 (0 to 3 upscale stages; anything else -> CID_ERR_INVALID).  cid_sr_param_key
 * enumerates the module's state_dict keys in its order (82 + 3 * stages of them).  cid_sr_set_weight, cid_sr_set_bn_eps (block 0..4;
 * which 0: res_blocks.i.1, 1: res_blocks.i.4), cid_sr_missing_weights, cid_sr_packed_weights_bytes and cid_sr_upload_weights behave
 * as their cid_esr_* namesakes, errors included; each BatchNorm is folded into y = fmaf(s, z, t) in fp64 at upload, and `mid` runs
 * with (s, t) = (1, 0).  PReLU is v > 0 ? v : a * v for any slope a.
 *
 * cid_sr_forward: in is the UNPADDED image, fp32 [N,3,H,W] already normalised to [-1,1] (CID_FMT_F32_NCHW) or uint8 [N,H,W,3]
 * (CID_FMT_U8_NHWC), read as ((float)u / 255.0f - 0.5f) / 0.5f with true divisions (ToTensor + Normalize(0.5, 0.5)): a uint8 image
 * and its normalised fp32 copy give identical bits.  The server's Pad(fill=0) is index arithmetic, as in cid_forward_padded: the
 * network runs on Hp x Wp = (H + pad_top + pad_bottom) x (W + pad_left + pad_right), the band around the image reads as -1.0 and no
 * padded copy exists.  Pads must lie in [0, 4096].  out is the WHOLE padded result, as the server shows it (app.py:481-485 crops only
 * the input's picture): fp32 [N,3,s*Hp,s*Wp] = tanh(.), or uint8 [N,s*Hp,s*Wp,3] as the server's view
 * (uint8)(clamp(tanhf(v) * 0.5f + 0.5f, 0, 1) * 255.0f), a truncation.  flags & CID_SR_RAW gives the fp32 sums before tanh instead
 * (a testing aid).  Any H, W >= 1.  1 + 11 + stages + 1 launches on `stream`, no host synchronisation; trunk and upscale stages run on
 * exact-fp32 MFMA, head and tail on the VALU; the 256-channel tensor before a PixelShuffle is never stored.  Every sum has a fixed
 * order and an image's tiles depend only on the padded size: an image's result is bit-identical in any batch.  Checked on the host
 * before any launch:
 *   CID_ERR_INVALID    null pointer, unknown format, misaligned fp32 operand, unknown flags, CID_SR_RAW with a uint8 output,
 *                      a pad outside [0, 4096]
 *   CID_ERR_SHAPE      N < 1, H < 1, W < 1, s^2 * Hp * Wp >= 2^31
 *   CID_ERR_WORKSPACE  workspace smaller than cid_sr_workspace_bytes(N, Hp, Wp, scale_factor) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_sr_stage_view (testing aid): where the last forward over a padded Hp x Wp input left `stage` in its workspace: "x0", "trunk"
 * (= mid(r) + x0), "up1" (the first upscale stage's output; with two or more stages), "up2" (with three) and "tail_in" (the last
 * stage's output, or "trunk" at scale 1).  All are fp32 with 64 channels in blocks of 8, laid out as cid_esr_stage_view describes,
 * of size *Hs x *Ws.  Unknown or absent stage -> CID_ERR_KEY; a scale that is not 1, 2, 4 or 8 -> CID_ERR_INVALID.
 */
typedef struct cid_sr_s* cid_sr_t;
enum { CID_SR_RAW = 1 };
int cid_sr_create(cid_sr_t* out, int scale_factor);
void cid_sr_destroy(cid_sr_t h);
const char* cid_sr_last_error(cid_sr_t h);
const char* cid_sr_param_key(cid_sr_t h, int i);
int cid_sr_set_weight(cid_sr_t h, const char* key, const void* host_data, const int64_t* shape, int ndim);
int cid_sr_set_bn_eps(cid_sr_t h, int block, int which, double eps);
int cid_sr_missing_weights(cid_sr_t h, int* count);
size_t cid_sr_packed_weights_bytes(cid_sr_t h);
int cid_sr_upload_weights(cid_sr_t h, void* device_blob, void* stream);
int cid_sr_workspace_bytes(int N, int Hp, int Wp, int scale_factor, size_t* bytes);
int cid_sr_forward(cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, int pad_left, int pad_top,
                   int pad_right, int pad_bottom, unsigned flags, void* workspace, size_t workspace_bytes, void* stream);
int cid_sr_stage_view(const char* stage, int N, int Hp, int Wp, int scale_factor, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                      int* channel_block);

/*
 * The same generator in TRAIN mode: the first line of the SRGAN trainer's step, fake_hr = self.generator(lr_img)
 * (sr_ganTrainGNew.py:393, after self.generator.train()).  Forward only; the output carries no gradient.
 *
 * cid_sr_forward_train is cid_sr_forward with the ten BatchNorms on the statistics of THIS batch.  bn[0..9] describe
 * res_blocks.0.1, res_blocks.0.4, res_blocks.1.1, ... res_blocks.4.4, a cid_disc_bn each (device pointers, so that the updates land in
 * the caller's own buffers; eps and momentum as the containers hold them, CID_DISC_MOMENTUM_NONE for momentum=None), with the
 * train semantics documented for cid_disc_forward(training = 1): each BatchNorm normalises with the batch mean and the BIASED batch
 * variance over N*H*W values per channel, then running = (1 - m) * running + m * batch_stat with the UNBIASED variance for
 * running_var, and num_batches_tracked += 1; m = momentum, or 1 / num_batches_tracked after the increment.  All of it runs on the
 * device; there is no host synchronisation.  Convolution weights, biases and PReLU slopes come from the blob cid_sr_upload_weights
 * made; the (s, t) it folded from the running statistics are not read, and the blob is not changed: after a train forward the
 * running statistics differ from the ones the blob was folded from, so upload again before the next cid_sr_forward.
 * There are no pad arguments (the trainer does not pad): the network runs on H x W.  in, out, in_fmt, out_fmt and flags are
 * cid_sr_forward's (head and tail are its launches).  Launches: head, 10 x (convolution, statistics), one counter launch, mid,
 * log2(s) upscale stages, tail.  A convolution stores its raw result z and per-tile fp64 sums of z and z^2 (one slab row per tile);
 * the statistics launch reduces them in a fixed order in fp64 to (scale, shift) = (gamma / sqrt(var + eps), beta - mean * scale),
 * rounded once to fp32; the next convolution applies fmaf(scale, z, shift), and PReLU where the block has one, while it stages its
 * input.  No atomics: the same call on the same buffers gives the same bits (an image's result depends on its batch, as the
 * statistics do).  N*H*W == 1 is CID_ERR_SHAPE ("Expected more than 1 value per channel when training").  Checked on the host before
 * any launch:
 *   CID_ERR_INVALID    null pointer (any of bn[l]'s five included), unknown format, misaligned fp32 operand, unknown flags,
 *                      CID_SR_RAW with a uint8 output, an eps or momentum that is not finite or negative (other than
 *                      CID_DISC_MOMENTUM_NONE)
 *   CID_ERR_SHAPE      N < 1, H < 1, W < 1, s^2 * H * W >= 2^31, N*H*W == 1
 *   CID_ERR_WORKSPACE  workspace smaller than cid_sr_train_workspace_bytes(N, H, W, scale_factor) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_sr_train_workspace_bytes: with a(v) = v rounded up to 256, t = N * 64 * H * W * 4 and tiles = ceil(H/16) * ceil(W/16),
 *   4 a(t)                                 x0, the two raw z tensors the convolutions alternate between, mid's result
 *   + sum_{k=1..stages} a(4^k t)           the upscale stages' outputs
 *   + a(64 * 2 * N * tiles * 8)            the slab (reused by all ten convolutions)
 *   + a(10 * 64 * 2 * 4)                   the ten (scale, shift) tables
 * cid_sr_train_stage_view is cid_sr_stage_view for that workspace: "x0", "trunk", "up1", "up2", "tail_in".
 */
int cid_sr_train_workspace_bytes(int N, int H, int W, int scale_factor, size_t* bytes);
int cid_sr_forward_train(cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, unsigned flags,
                         const cid_disc_bn* bn, void* workspace, size_t workspace_bytes, void* stream);
int cid_sr_train_stage_view(const char* stage, int N, int H, int W, int scale_factor, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                            int* channel_block);

/*
 * The backward pass of that train-mode generator: g_loss.backward() of the SRGAN trainer's step (sr_ganTrainGNew.py:408) from
 * grad_out = d loss / d fake_hr down to every parameter.  The family mirrors cid_srd_forward_saved / cid_srd_backward: per-call saved
 * buffer, what is null is not written, the same call twice gives the same bits, no host synchronisation.  There is no input
 * gradient: lr_img is data.
 *
 * cid_sr_forward_saved is cid_sr_forward_train with an fp32 output and a caller-owned PER-CALL saved buffer next to the workspace
 * (cid_sr_train_workspace_bytes; what the backward does not need stays there: the activated x0 and stage outputs, the slab).  out
 * and the BatchNorm buffer updates are bit-identical to cid_sr_forward_train.  The saved buffer keeps, without overlap: the head's
 * sums v0 before its PReLU, the ten raw z_l, mid's result t, every upscale stage's shuffled sums v_k before its PReLU, the ten
 * (scale, shift) and (mean, invstd) tables, and out.  Every PReLU mask of the backward is decided on a saved PRE-activation (v0, v_k,
 * or BN_l(z_l) recomputed with the forward's own fmaf), so it is the forward's decision for any slope, 0 and negative ones included.
 * cid_sr_saved_bytes(N, H, W, scale), with a(v) = v rounded up to 256 and t = N * 64 * H * W * 4:
 *     12 a(t) + sum_{k=1..stages} a(4^k t) + a(10*64*2*4) + a(10*64*2*8) + a(N*3*sH*sW*4)
 *
 * cid_sr_backward: `in` is the forward's input (the head's weight gradient reads it, fp32 or uint8 through the forward's own
 * normalisation), grad_out fp32 [N,3,sH,sW], flags the forward's (CID_SR_RAW: grad_out belongs to the sums before tanh), bn the
 * forward's array (only gamma is read).  `g` holds one pointer per parameter tensor in the module's layouts; a null pointer means the
 * tensor is not wanted.  The whole chain runs whatever is asked for.  BatchNorm's backward carries the two batch sums,
 * dz = k * (g - m1 - xh * m2); the GEMM-shaped gradients (3x3 data and weight gradients of the trunk and the upscale stages, final's
 * data and weight gradient) run on the exact-fp32 MFMA, a weight gradient accumulating in fp32 inside one workgroup's range of
 * tiles; the head's K = 243 weight gradient runs in fp64 on the VALU; every reduction across workgroups is fp64 in a fixed order
 * through a slab (or per-workgroup partials) and a reduce launch, no atomics.  The workspace may hold anything on entry.  Checked on the host before any launch:
 *   CID_ERR_INVALID    null h / in / grad_out / bn / bn[l].gamma / saved / g / workspace, unknown format or flags, misaligned fp32
 *                      pointer (the gradient tensors included)
 *   CID_ERR_SHAPE      as cid_sr_forward_train
 *   CID_ERR_WORKSPACE  saved buffer or workspace too small or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_sr_pack_weights_device builds the forward's blob from the parameter tensors in DEVICE memory with one launch and attaches it:
 * byte for byte what cid_sr_set_weight + cid_sr_set_bn_eps + cid_sr_upload_weights produce, mid's identity fold, the zero gaps and the
 * ten eval-mode folds (taken in fp64 from bn[l]'s gamma, beta, running_mean, running_var and eps, rounded as the host rounds them)
 * included.  dev_params holds the 3 + 45 + 2 + 3 * stages + 2 parameter tensors in the module's order: initial.0.weight,
 * initial.0.bias, initial.1.weight, per block 0.weight 0.bias 1.weight 1.bias 2.weight 3.weight 3.bias 4.weight 4.bias, mid.weight,
 * mid.bias, per stage (3k).weight (3k).bias (3k+2).weight, final.weight, final.bias.  A trainer calls it after every optimizer step.
 *   CID_ERR_INVALID    null h / dev_params / bn / device_blob, a null or not 4-byte-aligned parameter pointer, a null gamma, beta,
 *                      running_mean or running_var, an eps that is not finite or negative
 *   CID_ERR_WORKSPACE  device_blob not 256-byte aligned
 *
 * cid_sr_saved_masks is a testing aid as cid_srd_saved_masks: the 1 + 5 + stages PReLU decisions as the backward takes them, uint8
 * (1 where the slope is 1): masks[0] the head [N,64,H,W], masks[1..5] the blocks' PReLUs (after res_blocks.i.1) [N,64,H,W],
 * masks[6 + k] stage k [N,64,2^(k+1) H,2^(k+1) W].
 */
typedef struct {
    float* head_w;        /* initial.0.weight [64,3,9,9]                         */
    float* head_b;        /* initial.0.bias [64]                                 */
    float* head_slope;    /* initial.1.weight [1]                                */
    float* conv_w[10];    /* res_blocks.i.0.weight (2i), res_blocks.i.3.weight (2i+1) */
    float* conv_b[10];    /* their biases                                        */
    float* gamma[10];     /* res_blocks.i.1.weight (2i), res_blocks.i.4.weight (2i+1) */
    float* beta[10];      /* their biases                                        */
    float* slope[5];      /* res_blocks.i.2.weight [1]                           */
    float* mid_w;         /* mid.weight [64,64,3,3]                              */
    float* mid_b;         /* mid.bias [64]                                       */
    float* up_w[3];       /* upscale.3k.weight [256,64,3,3]                      */
    float* up_b[3];       /* upscale.3k.bias [256]                               */
    float* up_slope[3];   /* upscale.(3k+2).weight [1]                           */
    float* final_w;       /* final.weight [3,64,9,9]                             */
    float* final_b;       /* final.bias [3]                                      */
} cid_sr_grads;
int cid_sr_saved_bytes(int N, int H, int W, int scale_factor, size_t* bytes);
int cid_sr_forward_saved(cid_sr_t h, const void* in, int in_fmt, float* out, int N, int H, int W, unsigned flags, const cid_disc_bn* bn,
                         void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int cid_sr_backward_workspace_bytes(int N, int H, int W, int scale_factor, size_t* bytes);
int cid_sr_backward(cid_sr_t h, const void* in, int in_fmt, const float* grad_out, int N, int H, int W, unsigned flags,
                    const cid_disc_bn* bn, const void* saved, size_t saved_bytes, const cid_sr_grads* g, void* workspace,
                    size_t workspace_bytes, void* stream);
int cid_sr_pack_weights_device(cid_sr_t h, const float* const* dev_params, const cid_disc_bn* bn, void* device_blob, void* stream);
int cid_sr_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int scale_factor, unsigned char* const* masks,
                       void* stream);

/*
 * The server's fourth model — CGANGenerator(n_classes = 10, latent_dim = 100) (backend/app.py:105-143), the "cgan" branch of /enhance,
 * label-conditioned branch (cond a 1-D integer tensor).  Eval mode, fp32; the output is always 64 x 64:
 *
 *   x    = cat(z [N,100], label_emb[label] [N,100])                                       label_emb
 *   a0   = ReLU(BatchNorm(l1(x).view(N,128,8,8)))                                          l1, model.0, model.1
 *   a_k  = ReLU(BatchNorm(ConvTranspose2d(C, C', 4, stride=2, padding=1)(a_{k-1})))        model.{2,3,4}, {5,6,7}, {8,9,10}
 *                                                                                         128 -> 128 -> 64 -> 32 channels, 8 -> 64 pixels
 *   out  = tanh(Conv2d(32, 3, 3, padding=1)(a_3))                                          model.11
 *
 * The reference hard-codes view(-1, 100, 1, 1), so latent_dim is 100 and only n_classes is a parameter.  Its image-conditioned branch
 * (a 4-D cond, app.py:139-143) feeds 6 channels to BatchNorm2d(128) and raises for every input; it is not built.  Its own handle and
 * blob, mirroring cid_sr_* one for one.  cid_cg_create fixes n_classes (1 .. 2^20; anything else -> CID_ERR_INVALID).
 * cid_cg_param_key enumerates the module's 31 state_dict keys in its order; ConvTranspose2d weights are [Cin,Cout,4,4] as PyTorch
 * stores them.  cid_cg_set_weight, cid_cg_set_bn_eps (which 0..3: model.0, model.3, model.6, model.9), cid_cg_missing_weights,
 * cid_cg_packed_weights_bytes and cid_cg_upload_weights behave as their cid_sr_* namesakes, errors included; each BatchNorm is folded
 * into y = fmaf(s, v, t) in fp64 at upload.  ReLU is v < 0 ? 0 : v.
 *
 * cid_cg_latent: the input the server draws with torch.randn(N,100,1,1) (app.py:428), from the counter-based hash streams of
 * cid_add_noise: z_out[i, e] (fp32 [N,100], device) = (float)box_muller(u1, u2) with u1, u2 element e of the streams
 * fnv1a64("cgan:z:u1") and fnv1a64("cgan:z:u2") under seed (seed + first_index + i), so image i's latent does not depend on the batch
 * it is drawn in.  One launch.  CID_ERR_INVALID: null or misaligned pointer; CID_ERR_SHAPE: N outside [1, 2^18].
 *
 * cid_cg_forward: z is fp32 [N,100] and labels int64 [N], both on the device; out is fp32 [N,3,64,64] = tanh(.) (CID_FMT_F32_NCHW), or
 * uint8 [N,64,64,3] (CID_FMT_U8_NHWC) as the server's view (uint8)(clamp(tanhf(v) * 0.5f + 0.5f, 0, 1) * 255.0f), a truncation
 * (app.py:435, 472).  flags & CID_CG_RAW gives the fp32 sums before tanh instead (a testing aid).  The labels are read on the device
 * and NOT range-checked on the host (that would need a synchronisation): a label outside [0, n_classes) never indexes out of bounds;
 * that image's whole output is NaN (fp32) or 0 (uint8) and no other image changes.  1 + 3 + 1 launches on `stream`, no host
 * synchronisation: the linear and the three transposed convolutions run on exact-fp32 MFMA (each transposed convolution as four 2 x 2
 * convolutions, one per output parity), the tail on the VALU.  In the linear the images are the GEMM's columns; every sum has a fixed
 * order: an image's result is bit-identical in any batch and at any position in it.  Checked on the host before any launch:
 *   CID_ERR_INVALID    null pointer, unknown format, misaligned operand, unknown flags, CID_CG_RAW with a uint8 output
 *   CID_ERR_SHAPE      N outside [1, 2^18]
 *   CID_ERR_WORKSPACE  workspace smaller than cid_cg_workspace_bytes(N) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_cg_stage_view (testing aid): where the last forward over N images left `stage` in its workspace: "l1" (a0, 128 channels, 8 x 8),
 * "t1" (128, 16 x 16), "t2" (64, 32 x 32), "t3" (32, 64 x 64), all after BatchNorm and ReLU, fp32 in channel blocks of 8, laid out as
 * cid_esr_stage_view describes.  Unknown stage -> CID_ERR_KEY.
 */
typedef struct cid_cg_s* cid_cg_t;
enum { CID_CG_RAW = 1 };
int cid_cg_create(cid_cg_t* out, int n_classes);
void cid_cg_destroy(cid_cg_t h);
const char* cid_cg_last_error(cid_cg_t h);
const char* cid_cg_param_key(cid_cg_t h, int i);
int cid_cg_set_weight(cid_cg_t h, const char* key, const void* host_data, const int64_t* shape, int ndim);
int cid_cg_set_bn_eps(cid_cg_t h, int which, double eps);
int cid_cg_missing_weights(cid_cg_t h, int* count);
size_t cid_cg_packed_weights_bytes(cid_cg_t h);
int cid_cg_upload_weights(cid_cg_t h, void* device_blob, void* stream);
int cid_cg_workspace_bytes(int N, size_t* bytes);
int cid_cg_latent(uint64_t seed, uint64_t first_index, int N, float* z_out, void* stream);
int cid_cg_forward(cid_cg_t h, const float* z, const int64_t* labels, void* out, int out_fmt, int N, unsigned flags, void* workspace,
                   size_t workspace_bytes, void* stream);
int cid_cg_stage_view(const char* stage, int N, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block);

/*
 * LPIPS — lpips.LPIPS(net='alex') of lpips 0.1.4 (version='0.1', lpips=True, spatial=False, eval mode), the third number of the
 * reference trainers' evaluation (denoise_gan_code/training.py:282,389; srgan_code/sr_ganTrainGNew.py:264,372;
 * cgan_code/training5barrev.py:20,140).  THE DEFINITION (kept here and nowhere else):
 *
 *   1. forward(in0, in1, normalize=False): with normalize=True each input becomes 2*x - 1 first.  Inputs are meant to lie in [-1,1].
 *   2. Scaling layer: (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450).  The zero padding of
 *      the first convolution applies to the SCALED tensor: a padded position is 0, not (0 - shift) / scale.
 *   3. torchvision AlexNet `features`, five taps, each taken after a ReLU:
 *        relu1  Conv2d(3,64,11,stride 4,pad 2) + ReLU
 *        relu2  MaxPool2d(3,2) -> Conv2d(64,192,5,pad 2) + ReLU
 *        relu3  MaxPool2d(3,2) -> Conv2d(192,384,3,pad 1) + ReLU
 *        relu4  Conv2d(384,256,3,pad 1) + ReLU
 *        relu5  Conv2d(256,256,3,pad 1) + ReLU
 *      Pools have no padding and use floor mode: H1 = (H-7)/4 + 1, H2 = (H1-3)/2 + 1, H3 = (H2-3)/2 + 1 (integer division; the same
 *      for W); relu3, relu4 and relu5 are H3 x W3.  The smallest accepted side is 31 (maps 7 -> 3 -> 1).
 *   4. Per tap k and tower: xhat = x / (sqrt(sum_c x^2) + 1e-10) per pixel.
 *   5. Layer distance d_k = mean over pixels of sum_c w_k[c] * (xhat0 - xhat1)^2; w_k is the 1x1 `lin` convolution (no bias, no
 *      clamp, dropout inert in eval mode).
 *   6. d = d_0 + ... + d_4, one value per image pair (the package returns it as fp32 [N,1,1,1]).
 *
 * The three trainers call it on x*0.5+0.5 with normalize=False, so the network sees [0,1] images where it expects [-1,1];
 * CID_LPIPS_UNIT_VIEW reproduces that call (v*0.5f+0.5f on both operands before the scaling layer) and does not correct it.
 *
 * State-dict names (cid_lpips_param_key order, 17 tensors, fp32): scaling_layer.shift, scaling_layer.scale ([1,3,1,1]);
 * net.slice1.0, net.slice2.3, net.slice3.6, net.slice4.8, net.slice5.10 .weight / .bias ([Cout,Cin,k,k] / [Cout]);
 * lin0.model.1.weight ... lin4.model.1.weight ([1,C,1,1], C = 64, 192, 384, 256, 256).  The module repeats the five lin tensors
 * under lins.<k>.model.1.weight; those aliases are the caller's to drop.  The package's weight file holds only the lin* keys, the
 * backbone is torchvision's alexnet state dict (features.{0,3,6,8,10}.*).
 *
 * Its own handle and blob, mirroring cid_cg_* one for one: cid_lpips_set_weight (CID_ERR_KEY for any other name, CID_ERR_SHAPE for a
 * size mismatch), cid_lpips_missing_weights, cid_lpips_packed_weights_bytes and cid_lpips_upload_weights (needs all 17 tensors,
 * CID_ERR_STATE otherwise) behave as their namesakes.
 *
 * cid_lpips: a and b are fp32 [N,3,H,W] (CID_FMT_F32_NCHW, read as they are) or uint8 [N,H,W,3] (CID_FMT_U8_NHWC, read as
 * (u/255 - 0.5)/0.5 like cid_quality: a uint8 image and its normalised fp32 copy give identical bits), each its own format.
 * out is device double [N]; layers, if not NULL, device double [N][5] = d_0 ... d_4.  Both towers run as one batch of 2 N images:
 * 1 + 4 + 1 launches on `stream`, no host synchronisation.  relu1 is computed on the VALU, relu2 ... relu5 on the exact-fp32 MFMA with
 * the max-pools taken while the operand is staged (no pooled tensor exists); from the stored fp32 taps on, everything (channel sums
 * of squares, sqrt, + 1e-10, the divisions, the weighted squared differences, the pixel mean, the layer sum) is double in a fixed
 * order, so the distance's only error is the taps'.  No atomics; every sum's order depends on (H, W) and the pixel alone: an image
 * pair's result is bit-identical in any batch and at any position in it, d(x, x) is exactly 0 and d(a, b) == d(b, a) bit for bit.
 * Checked on the host before any launch:
 *   CID_ERR_INVALID    null pointer (layers may be NULL), unknown format, misaligned fp32 operand / out / layers, unknown flags
 *   CID_ERR_SHAPE      N outside [1, 2^20], H or W < 31, H*W >= 2^31, or a map too wide for the convolution kernel's LDS tile
 *                      (sides up to 1024 are accepted)
 *   CID_ERR_WORKSPACE  workspace smaller than cid_lpips_workspace_bytes(N, H, W) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded
 *
 * cid_lpips_stage_view (testing aid): where the last call over N pairs left `stage` = "relu1" ... "relu5" in its workspace: fp32 in
 * channel blocks of 8 as cid_esr_stage_view describes, 2 N images (operand a's N, then operand b's N).  Unknown stage -> CID_ERR_KEY.
 */
typedef struct cid_lpips_s* cid_lpips_t;
enum { CID_LPIPS_UNIT_VIEW = 1 };
#define CID_LPIPS_NUM_WEIGHTS 17
int cid_lpips_create(cid_lpips_t* out);
void cid_lpips_destroy(cid_lpips_t h);
const char* cid_lpips_last_error(cid_lpips_t h);
const char* cid_lpips_param_key(cid_lpips_t h, int i);
int cid_lpips_set_weight(cid_lpips_t h, const char* key, const void* host_data, const int64_t* shape, int ndim);
int cid_lpips_missing_weights(cid_lpips_t h, int* count);
size_t cid_lpips_packed_weights_bytes(cid_lpips_t h);
int cid_lpips_upload_weights(cid_lpips_t h, void* device_blob, void* stream);
int cid_lpips_workspace_bytes(int N, int H, int W, size_t* bytes);
int cid_lpips_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block);
int cid_lpips(cid_lpips_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
              double* layers, void* workspace, size_t workspace_bytes, void* stream);

/*
 * VGG16 features — what the reference's trainers build on torchvision's vgg16: lpips.LPIPS(net='vgg') of lpips 0.1.4, the ESRGAN
 * trainer's perceptual metric (esrgan_code/esrgan_train.py:65,133), and VGGPerceptualLoss, the content loss of the SRGAN and denoise
 * trainers (srgan_code/sr_ganTrainGNew.py:83-94,217,405; denoise_gan_code/training.py:101-111).  Eval mode, fp32; the content loss
 * also has its input gradient (cid_vgg_content_backward, below).
 * THE DEFINITION (kept here and nowhere else):
 *
 *   1. The backbone is torchvision vgg16 `features`, every convolution Conv2d(Cin,Cout,3,pad 1) + ReLU, every pool MaxPool2d(2,2)
 *      without padding, floor mode (an odd last row or column is dropped).  By `features` index:
 *        slice1   0: 3->64     2: 64->64                          relu1_2   H1 x W1 = H x W
 *        slice2   pool,  5: 64->128    7: 128->128                relu2_2   H2 = H1 / 2
 *        slice3   pool, 10: 128->256  12: 256->256  14: 256->256  relu3_3   H3 = H2 / 2
 *        slice4   pool, 17: 256->512  19: 512->512  21: 512->512  relu4_3   H4 = H3 / 2
 *        slice5   pool, 24: 512->512  26: 512->512  28: 512->512  relu5_3   H5 = H4 / 2      (integer division; the same for W)
 *   2. cid_vgg_lpips is LPIPS as cid_lpips defines it (items 1, 2 and 4 - 6 there: normalize, the scaling layer with the zero padding
 *      applied to the SCALED tensor, unit vectors per pixel, d_k with the 1x1 `lin` weights, d = d_0 + ... + d_4) over the five taps
 *      relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of 64, 128, 256, 512, 512 channels.  The smallest accepted side is 16 (H5 = 1).
 *      CID_LPIPS_UNIT_VIEW has cid_lpips's meaning.
 *   3. cid_vgg_content_loss is MSELoss()(features[:16](a), features[:16](b)) per image pair: out[n] = mean over the 256 * H3 * W3
 *      values of (relu3_3(a_n) - relu3_3(b_n))^2.  The operands enter the first convolution as they are read: no scaling layer and no
 *      ImageNet normalisation, which is what the reference's class does with its [-1,1] tensors.  The trainer's scalar is the mean
 *      of out.  The smallest accepted side is 4 (H3 = 1).  CID_LPIPS_UNIT_VIEW applies v*0.5f+0.5f first here too.
 *
 * State-dict names (cid_vgg_param_key order, 33 tensors, fp32): scaling_layer.shift, scaling_layer.scale ([1,3,1,1]);
 * net.slice1.{0,2}, net.slice2.{5,7}, net.slice3.{10,12,14}, net.slice4.{17,19,21}, net.slice5.{24,26,28} .weight / .bias
 * ([Cout,Cin,3,3] / [Cout]); lin0.model.1.weight ... lin4.model.1.weight ([1,C,1,1], C = 64, 128, 256, 512, 512).  The lins.* aliases
 * are the caller's to drop.  The package's weight file holds only the lin* keys; the backbone is torchvision's vgg16 state dict
 * (features.N.* -> net.sliceK.N.*).  The reference's VGGPerceptualLoss names the same first seven convolutions slice.N.*.
 *
 * The handle mirrors cid_lpips_* one for one, with one difference: cid_vgg_upload_weights accepts either all 33 tensors or exactly
 * the 14 tensors of net.slice1 ... net.slice3; the second form serves cid_vgg_content_loss only (cid_vgg_lpips returns
 * CID_ERR_STATE on it).  Any other set of tensors is CID_ERR_STATE.
 *
 * Operands, out, layers, flags and guarantees are cid_lpips's: a and b are fp32 [N,3,H,W] or uint8 [N,H,W,3] (read as
 * (u/255 - 0.5)/0.5; the same bits as the normalised fp32 copy), out is device double [N], layers (cid_vgg_lpips only, may be NULL)
 * device double [N][5].  Both towers run as one batch of 2 N images: 1 + 12 + 1 launches on `stream` (1 + 6 + 1 for the content
 * loss), no host synchronisation.  The first convolution runs on the VALU, the other twelve on the exact-fp32 MFMA with the pools
 * taken while the operand is staged (no pooled tensor exists); from the stored fp32 taps on everything is double in a fixed order.
 * No atomics, and no launch dimension other than grid.x grows with N; every sum's order depends on (H, W) and the pixel alone: an
 * image pair's result is bit-identical in any batch and at any position in it, the value of (x, x) is exactly 0 and (a, b) gives
 * the bits of (b, a).  `what` selects the form a workspace or a view is for: CID_VGG_LPIPS or CID_VGG_CONTENT.
 * THE LARGEST ACCEPTED SIDE IS 512 (H and W each): the convolution kernel stages whole rows of a map in LDS, and its widest plane
 * holds the rows a run of columns touches in a map up to 512 wide.  Checked on the host before any launch:
 *   CID_ERR_INVALID    null pointer (layers may be NULL), unknown format or form, misaligned fp32 operand / out / layers, unknown flags
 *   CID_ERR_SHAPE      N outside [1, 2^20], H or W < 16 (cid_vgg_lpips) or < 4 (cid_vgg_content_loss), H or W > 512,
 *                      or more than (2^31 - 1) * 64 pixels in the 2 N images
 *   CID_ERR_WORKSPACE  workspace smaller than cid_vgg_workspace_bytes(what, N, H, W) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded, or cid_vgg_lpips on a handle that holds slice1 ... slice3 only
 *
 * cid_vgg_stage_view (testing aid): where the last call left `stage` = "relu1" ... "relu5" (the five taps above; "relu1" ... "relu3"
 * for CID_VGG_CONTENT) in its workspace, in the layout cid_lpips_stage_view describes.  Unknown stage -> CID_ERR_KEY.
 */
typedef struct cid_vgg_s* cid_vgg_t;
enum { CID_VGG_LPIPS = 0, CID_VGG_CONTENT = 1 };
#define CID_VGG_NUM_WEIGHTS 33
#define CID_VGG_MAX_SIDE 512
int cid_vgg_create(cid_vgg_t* out);
void cid_vgg_destroy(cid_vgg_t h);
const char* cid_vgg_last_error(cid_vgg_t h);
const char* cid_vgg_param_key(cid_vgg_t h, int i);
int cid_vgg_set_weight(cid_vgg_t h, const char* key, const void* host_data, const int64_t* shape, int ndim);
int cid_vgg_missing_weights(cid_vgg_t h, int* count);
size_t cid_vgg_packed_weights_bytes(cid_vgg_t h);
int cid_vgg_upload_weights(cid_vgg_t h, void* device_blob, void* stream);
int cid_vgg_workspace_bytes(int what, int N, int H, int W, size_t* bytes);
int cid_vgg_stage_view(int what, const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block);
int cid_vgg_lpips(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
                  double* layers, void* workspace, size_t workspace_bytes, void* stream);
int cid_vgg_content_loss(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * The input gradient of the content loss — what the SRGAN trainer's generator step takes from VGGPerceptualLoss
 * (srgan_code/sr_ganTrainGNew.py:403-409: content_loss = vgg_loss(fake_hr, hr_img); g_loss.backward()).  The weights are frozen, so
 * there is no weight gradient; operand b (the trainer's hr_img) never requires one, so there is none for b either.
 *
 * cid_vgg_content_loss_saved is cid_vgg_content_loss — the same definition, the same kernels, the same `out` bits — with a
 * caller-owned PER-CALL arena of cid_vgg_saved_bytes(N, H, W) bytes, 256-byte aligned, in place of the workspace.  It leaves the seven
 * activations of both towers there, each in its own tensor (the plain call overwrites four of them in its two scratch tensors).
 * Operand a must be fp32 [N,3,H,W]: a uint8 image has no gradient, and fmt_a = CID_FMT_U8_NHWC is CID_ERR_INVALID.  b may be either
 * format.  Shape limits are cid_vgg_content_loss's: 4 <= H, W <= 512.
 *
 * cid_vgg_content_backward(h, grad_out, grad_a, N, H, W, flags, saved, saved_bytes, stream): N, H, W, flags and `saved` are those of
 * the cid_vgg_content_loss_saved call to differentiate, on the same weights.  grad_out is device double [N] = dL/d out[n], read on
 * the device; grad_a is device fp32 [N,3,H,W]:
 *     grad_a[n] = grad_out[n] * d out[n] / d a[n],
 * with the factor 0.5 of v*0.5f+0.5f included under CID_LPIPS_UNIT_VIEW.  1 + 6 + 1 launches on `stream`, no host synchronisation:
 * the seed, six data gradients on the exact-fp32 MFMA (each a 3x3 convolution of the gradient with the flipped, transposed weights,
 * summed as the forward sums: chains cut every 4 chunks of 4 channels, partial sums added in order) with both max-pool backwards
 * taken while the operand is staged (first maximum of the 2x2 window in row-major order, v > max || isnan(v): ATen's rule; no
 * unpooled tensor exists), and the first convolution's backward on the VALU.  A ReLU's mask is `saved activation > 0`.  No atomics:
 * grad_a[n] depends on pair n and grad_out[n] alone, bit-identical in any batch, at any position in it and across runs.
 *
 * The data-gradient weights are a second blob of cid_vgg_backward_weights_bytes(h) bytes (about 7 MB), which only handles that run
 * a backward pay for: cid_vgg_upload_backward_weights(h, device_blob, stream) packs it from the 14 tensors of net.slice1 ...
 * net.slice3 (any missing: CID_ERR_STATE; blob not 256-byte aligned: CID_ERR_WORKSPACE).  cid_vgg_upload_weights drops it: upload
 * it again after the forward blob.
 *
 * The arena holds, after the 7 activations ("relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3"; 2 N images
 * each, operand a's N first), the 7 gradient tensors the backward stores, each written exactly once, N images, fp32.  With L the
 * scalar sum_n grad_out[n] * out[n], z the value of a convolution before its ReLU and p a max-pool's output:
 *     "grad3_3"    dL/d z3_3 = grad_out[n] * 2 / (256 H3 W3) * (relu3_3(a) - relu3_3(b)) where relu3_3(a) > 0, else 0
 *                  (formed in double, rounded once)                                                     [N,256,H3,W3]
 *     "grad3_2"    dL/d z3_2: masked by relu3_2 > 0                                                     [N,256,H3,W3]
 *     "grad3_1"    dL/d z3_1: masked by relu3_1 > 0                                                     [N,256,H3,W3]
 *     "gradpool2"  dL/d p2, the gradient of the second pool's OUTPUT: no mask, no routing yet           [N,128,H3,W3]
 *     "grad2_1"    dL/d z2_1: masked by relu2_1 > 0 (dL/d z2_2, gradpool2 routed through the pool and
 *                  masked by relu2_2 > 0, exists only in the staging of this launch)                    [N,128,H2,W2]
 *     "gradpool1"  dL/d p1, the gradient of the first pool's output                                     [N,64,H2,W2]
 *     "grad1_1"    dL/d z1_1: masked by relu1_1 > 0 (dL/d z1_2 likewise exists only in staging)         [N,64,H,W]
 * cid_vgg_saved_view (testing aid) gives a stage's byte offset in the arena, its image count (2 N or N), channels, size and
 * channel block (the C8 layout cid_lpips_stage_view describes).  Unknown stage -> CID_ERR_KEY.
 *
 * Everything refused is refused on the host before any launch:
 *   CID_ERR_INVALID    null pointer, unknown format or flags, fmt_a not fp32, misaligned fp32 operand / out / grad_out / grad_a
 *   CID_ERR_SHAPE      as cid_vgg_content_loss
 *   CID_ERR_WORKSPACE  arena smaller than cid_vgg_saved_bytes(N, H, W) or not 256-byte aligned
 *   CID_ERR_STATE      weights not uploaded; cid_vgg_content_backward: backward weights not uploaded
 */
int cid_vgg_saved_bytes(int N, int H, int W, size_t* bytes);
int cid_vgg_saved_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* images, int* C, int* Hs, int* Ws, int* channel_block);
int cid_vgg_content_loss_saved(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags,
                               double* out, void* saved, size_t saved_bytes, void* stream);
size_t cid_vgg_backward_weights_bytes(cid_vgg_t h);
int cid_vgg_upload_backward_weights(cid_vgg_t h, void* device_blob, void* stream);
int cid_vgg_content_backward(cid_vgg_t h, const double* grad_out, float* grad_a, int N, int H, int W, unsigned flags, void* saved,
                             size_t saved_bytes, void* stream);

/*
 * Testing aid (no reference counterpart): fills the LDS of every CU with NaN on `stream`.  LDS is not cleared between
 * kernels, so a forward enqueued after it exposes any kernel that reads LDS words it has not written.
 */
int cid_debug_poison_lds(void* stream);
/*
 * Testing aid (no reference counterpart): cid_adam_step with HOST pointers, run on the CPU by the calling thread: the same argument
 * checks, the same table and the same work-item code as the kernel (csrc/optim_kernels.h is __host__ __device__), one (work item,
 * lane) after the other.  It holds the index arithmetic and the expression tree against synth.adam_step_np without a GPU.
 */
int cid_debug_adam_step_host(const cid_adam_tensor* tensors, int ntensors, const cid_adam_hyper* hp);
/*
 * Testing aid (no reference counterpart): the four LeakyReLU masks of a cid_disc_forward_saved call exactly as the backward kernels
 * decide them, uint8 (1 where the slope is 1, 0 where it is 0.2): masks[0] [N,64,H,W] (model.1), masks[1] [N,64,H2,W2] (model.4),
 * masks[2] [N,128,H2,W2] (model.7), masks[3] [N,128,H4,W4] (model.10).  LeakyReLU's derivative is discontinuous, so a gradient check
 * against a float64 reference is only meaningful with the reference on the same side of zero at every unit.
 */
int cid_disc_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int training, unsigned char* const* masks,
                         void* stream);
/*
 * Testing / measurement aid (no reference counterpart; process-wide): workgroups per CU of the Winograd F(4x2) launches.
 * k >= 1: a launch with more (tile, column block) items than k workgroups per CU is run by that many WALKING workgroups
 * (default 2; the kernel's LDS use admits no more).  0: every item gets its own workgroup.  Both must give the same bits.
 * Returns the previous value; a negative argument only queries.
 */
int cid_debug_winograd_workgroups_per_cu(int k);
/* Measurement aid (process-wide; default 0): bit mask over the column-block counts NB (2, 4) whose WALKING Winograd F(4x2) launches give every XCD
 * group ONE column block of a tile range instead of all NB blocks of its tiles back to back (profiles/r04_xnb_experiment.txt: bit-identical results,
 * -3 % fabric traffic, +-0 time).  Returns the previous mask; a negative argument only queries. */
int cid_debug_winograd_column_block_per_xcd(int mask);
/* The same for the 3x3 launches of the fp16-storage path (k_conv3x3_h16): k walking workgroups per CU (at most 3), 0 = one item per workgroup — the
 * DEFAULT since round 4 (measured faster once the epilogue lost its LDS staging: profiles/r04_ab_f16_walk_vs_not.txt); walking stays a tested option for the
 * launches without a fused pool (down1[2] and down2[2] always take one item per workgroup). */
int cid_debug_half_workgroups_per_cu(int k);

#ifdef __cplusplus
}
#endif
#endif /* CID_H_ */
